"""Request checks and device tables of the commitments computed from resident
squares (csrc/commit_layout.hpp) on the CPU: tests/host/commit_layout_check.cpp,
a stand-alone host program, compares the subtree width and the mountain-range
split with an independent restatement for every share count 1 .. 16385 and
65536, checks the tables of a mixed batch and that each refusal class is
refused naming the blob.  The sizes are also compared here with the
mountain-range function the Python side keeps (trees.py)."""
import os
import subprocess

import pytest

from celestia_da import trees

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "commit_layout_check.cpp")

# count -> (subtree width, number of subtrees, the last sizes)
SPOTS = {
    65: (2, 33, [2, 1]),
    129: (4, 33, [4, 1]),
    191: (4, 49, [4, 2, 1]),
    2049: (64, 33, [64, 1]),
    4097: (128, 33, [128, 1]),
    16383: (128, 134, [128, 64, 32, 16, 8, 4, 2, 1]),
    16385: (256, 65, [256, 1]),
    65536: (256, 256, [256]),
}


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True, timeout=180)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return dict(f.split("=") for f in out.stdout.split()[1:])


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=all"])])
def test_commit_layout_check(tmp_path, name, flags):
    f = _run(tmp_path, "commit_layout_check_" + name, flags)
    assert int(f["checked"]) == 16386
    assert int(f["maxtrees"]) == 134  # 16383 shares: 127 trees of 128, then 64 .. 1
    for count, (w, t, tail) in SPOTS.items():
        assert int(f[f"w{count}"]) == w and int(f[f"t{count}"]) == t, count
        got = [int(x) for x in f[f"tail{count}"].split(",")]
        assert got[-len(tail):] == tail, (count, got)
    counts = [1, 64, 65, 127, 129, 191, 256, 1, 3, 2, 1]
    assert int(f["batch_shares"]) == sum(counts)
    sizes = [s for c in counts for s in trees.merkle_mountain_range_sizes(c, _width(c))]
    assert int(f["batch_subtrees"]) == len(sizes) and int(f["batch_work"]) == sum(s >= 2 for s in sizes)
    assert int(f["refused"]) == 18


def _width(count, threshold=64):
    """inclusion.SubTreeWidth in integers."""
    s = trees.round_up_power_of_two(-(-count // threshold))
    r = 0
    while r * r < count:
        r += 1
    return min(s, trees.round_up_power_of_two(r))


def test_sizes_equal_trees_py():
    """The spot values against trees.merkle_mountain_range_sizes, and the
    greatest number of subtrees of any blob that fits a k = 128 square."""
    for count, (w, t, tail) in SPOTS.items():
        assert _width(count) == w
        sizes = trees.merkle_mountain_range_sizes(count, w)
        assert len(sizes) == t and sizes[-len(tail):] == tail and sum(sizes) == count
    assert max(len(trees.merkle_mountain_range_sizes(c, _width(c))) for c in range(1, 16385)) == 134
