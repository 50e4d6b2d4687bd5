"""Workspace layouts of Repair (csrc/repair_layout.hpp) and of the unsliced NMT
pass (csrc/pipe_carve.hpp nmt_carve) on the CPU: tests/host/repair_layout_check.cpp,
a stand-alone host program, walks both over k = 1, 2, 4, .., 8192 and
n in {1, 2, 3, 5, 64, 257} and checks that every region is 256-aligned, holds
what its users index, is disjoint from the others and ends inside the size.
The sizes themselves are a public ABI value (callers allocate by them), so they
are pinned to tests/golden/ws_sizes.json, recorded from the library before the
layouts became single lists."""
import json
import os
import subprocess

import pytest

from celestia_da import _abi

from conftest import GOLDEN, ROOT

KS = [1 << i for i in range(14)]
NS = [1, 2, 3, 5, 64, 257]


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(os.path.join(GOLDEN, "ws_sizes.json")))
    assert g["columns"] == ["k", "n", "dagpu_workspace_size", "dagpu_repair_workspace_size"]
    table = {(k, n): (ws, rep) for k, n, ws, rep in g["rows"]}
    assert sorted(table) == [(k, n) for k in KS for n in NS]
    return table


def test_layout_regions_and_sizes(tmp_path, golden):
    exe = str(tmp_path / "repair_layout_check")
    src = os.path.join(ROOT, "tests", "host", "repair_layout_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, src], check=True, timeout=120)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = {}
    for line in out.stdout.splitlines():
        k, n, nmt, rep = map(int, line.split())
        got[(k, n)] = (nmt, rep)
    assert sorted(got) == sorted(golden)
    for key, (nmt, rep) in got.items():
        # the entry points add 256 to the layouts' ends
        assert rep == golden[key][1] - 256, key
        assert nmt == golden[key][0] - 256, key


def test_abi_workspace_sizes_unchanged(golden):
    L = _abi.lib()  # loads without a GPU; the size functions touch no device
    for (k, n), (ws, rep) in golden.items():
        assert L.dagpu_workspace_size(k, n) == ws, (k, n)
        assert L.dagpu_repair_workspace_size(k, n) == rep, (k, n)
