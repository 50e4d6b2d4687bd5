"""Host arithmetic of the namespace producer across squares
(csrc/ns_squares_layout.hpp) on the CPU: tests/host/ns_squares_layout_check.cpp,
a stand-alone host program, round-trips the packed range word for w = 2 ..
32768, compares the nmt and merkle descriptors filled from hand-made hit tables
(absence proofs, whole rows, single cells) with a per-proof computation, checks
that each capacity is refused one short, that the re-check rejects each
malformed hit record, and that the workspace carve never overlaps and is
monotone.  Built plain and with the address and undefined-behaviour sanitizers.
The workspace size the library reports is compared with the same bound.  No GPU."""
import os
import subprocess

import pytest

from celestia_da import _abi

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "ns_squares_layout_check.cpp")


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=all"])])
def test_ns_squares_layout_check(tmp_path, name, flags):
    exe = str(tmp_path / ("ns_squares_layout_check_" + name))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True, timeout=180)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    fields = dict(f.split("=") for f in out.stdout.split()[1:])
    assert int(fields["tables"]) == 7 and int(fields["proofs"]) == 7 + 4 + 5 + 3
    # 15 widths, both kinds, the extremes of start and end
    assert int(fields["words"]) >= 15 * 2 * 8
    assert int(fields["rejected"]) >= 13 + 2 + 7 + 10 + 6 * 8 + 4
    # k x n_sq x n_q x proofs_cap
    assert int(fields["carves"]) == 5 * 3 * 4 * 4


def test_workspace_size_of_the_library():
    L = _abi.lib()
    size = L.dagpu_nmt_namespace_squares_workspace_size
    assert size(3, 1, 1, 0) == 0 and size(0, 1, 1, 0) == 0 and size(8, 0, 1, 0) == 0
    assert size(128, 1 << 20, 1 << 20, 0) == 0  # 2^48 (query, square, row)
    # the issue's workload: 64 squares of k = 128, 1,024 namespaces: 4 B per (query, square, row) and small change
    lanes = 1024 * 64 * 256
    got = size(128, 64, 1024, 0)
    assert 4 * lanes <= got <= 4 * lanes + lanes // 8 + lanes // 2048 + 4 * 1024 * 64 + 32 * 1024 + 16 * 256
    # 48 B per proof of proofs_cap
    assert 48 * 5000 <= size(128, 64, 1024, 5000) - got <= 48 * 5000 + 5 * 256
    assert size(8, 3, 5, 7) >= size(8, 3, 5, 0) >= size(8, 2, 5, 0) >= size(8, 2, 4, 0) > 0
    assert _abi.NS_HIT_WORDS == 6
