"""Request checks, output layout and the closed-form node rule of the batched
range-proof producer (csrc/prove_layout.hpp) on the CPU:
tests/host/prove_layout_check.cpp, a stand-alone host program, compares the
rule with nmt's recursive buildRangeProof for every range of every tree up to
128 leaves, checks the prefix sums and descriptors of a whole batch and that
each invalid request class is refused.  The closed form is also compared here
with proof.range_proof_nodes, the specification the Python side keeps."""
import os
import subprocess

import pytest

from celestia_da import proof

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "prove_layout_check.cpp")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True, timeout=180)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return dict(f.split("=") for f in out.stdout.split()[1:])


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=all"])])
def test_prove_layout_check(tmp_path, name, flags):
    fields = _run(tmp_path, "prove_layout_check_" + name, flags)
    # every range of trees of 1, 2, 4 .. 128 leaves
    assert int(fields["ranges"]) == sum(w * (w + 1) // 2 for w in (1, 2, 4, 8, 16, 32, 64, 128)) == 11050
    assert int(fields["nodes"]) > 0 and int(fields["batch"]) == 2 * 8 * 36 and int(fields["refused"]) == 15


def _closed_form(m, s, e):
    out = [(m - b, (s >> b) - 1) for b in range(m - 1, -1, -1) if (s >> b) & 1]
    out += [(m - b, ((e - 1) >> b) + 1) for b in range(m) if not ((e - 1) >> b) & 1]
    return out


def test_closed_form_equals_range_proof_nodes():
    for m in range(0, 8):
        w = 1 << m
        for s in range(w):
            for e in range(s + 1, w + 1):
                got = _closed_form(m, s, e)
                assert got == proof.range_proof_nodes(w, s, e), (w, s, e)
                assert len(got) == bin(s).count("1") + m - bin(e - 1).count("1")
