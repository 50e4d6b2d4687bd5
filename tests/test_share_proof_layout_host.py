"""Layout of the batch proof store, the request checks of the producer across
squares and NewShareInclusionProof's row split (csrc/share_proof_layout.hpp) on
the CPU: tests/host/share_proof_layout_check.cpp, a stand-alone host program,
compares the split with a loop written from pkg/proof/proof.go for every range
of every ODS up to k = 8, checks the prefix sums and descriptors of a mixed
batch, one refusal per invalid class and the DAH-tree addressing.  The same
split is compared here, through the library, with the arithmetic inside
proof.new_share_inclusion_proof, and the store's sizes and offsets with the
single-square stores'.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from celestia_da import _abi, device
from celestia_da.da import DAError

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host", "share_proof_layout_check.cpp")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True, timeout=180)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return dict(f.split("=") for f in out.stdout.split()[1:])


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined",
                                                       "-fno-sanitize-recover=all"])])
def test_share_proof_layout_check(tmp_path, name, flags):
    fields = _run(tmp_path, "share_proof_layout_check_" + name, flags)
    # every range of the ODS for k = 1, 2, 4, 8
    assert int(fields["ranges"]) == sum(k * k * (k * k + 1) // 2 for k in (1, 2, 4, 8)) == 2227
    assert int(fields["rows"]) > int(fields["ranges"])
    assert int(fields["batch"]) == 48 and int(fields["refused"]) == 6 + 9 + 2
    # every (leaf, level) of the trees of 4, 8, 16, 32 leaves
    assert int(fields["aunts"]) == sum(n * (n.bit_length() - 1) for n in (4, 8, 16, 32))


def _split_like_new_share_inclusion_proof(k, start, end):
    """The arithmetic of proof.new_share_inclusion_proof (proof.py), row by row."""
    start_row, end_row = start // k, (end - 1) // k
    start_leaf, end_leaf = start % k, (end - 1) % k
    out = []
    for i, row in enumerate(range(start_row, end_row + 1)):
        s = start_leaf if i == 0 else 0
        e = end_leaf if row == end_row else k - 1
        out.append((row, s, e + 1))
    return out


@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_split_equals_python_arithmetic(k):
    ranges = [(s % 3, s, e) for s in range(k * k) for e in range(s + 1, k * k + 1)]
    req, span = device.share_proof_requests(k, 3, ranges)
    assert span[0] == 0 and span[-1] == len(req)
    for i, (sq, s, e) in enumerate(ranges):
        got = [tuple(int(v) for v in r) for r in req[span[i]:span[i + 1]]]
        assert got == [(sq, 0, row, a, b) for row, a, b in _split_like_new_share_inclusion_proof(k, s, e)], (k, s, e)


def test_split_refusals_write_nothing():
    L = _abi.lib()
    for bad in ([2, 0, 1], [-1, 0, 1], [0, -1, 3], [0, 3, 3], [0, 5, 4], [1, 0, 17]):
        sreq = np.array([[0, 0, 16], bad, [1, 3, 9]], np.int64)
        req = np.full((64, 5), -7, np.int64)
        span = np.full(4, -7, np.int64)
        n_req = ctypes.c_size_t(99)
        rc = L.dagpu_share_proof_requests(4, 2, 3, _abi.addr(sreq), _abi.addr(req), 64, _abi.addr(span),
                                          ctypes.byref(n_req))
        assert rc == _abi.ERR_ARG and (req == -7).all() and (span == -7).all() and n_req.value == 99, bad
        with pytest.raises(DAError):
            device.share_proof_requests(4, 2, sreq)
    # k must be a power of two; too small a capacity
    sreq = np.array([[0, 0, 16]], np.int64)
    req = np.full((4, 5), -7, np.int64)
    n_req = ctypes.c_size_t(99)
    assert L.dagpu_share_proof_requests(3, 1, 1, _abi.addr(sreq), _abi.addr(req), 4, None,
                                        ctypes.byref(n_req)) == _abi.ERR_ARG
    assert L.dagpu_share_proof_requests(4, 1, 1, _abi.addr(sreq), _abi.addr(req), 3, None,
                                        ctypes.byref(n_req)) == _abi.ERR_ARG
    assert (req == -7).all() and n_req.value == 99
    assert L.dagpu_share_proof_requests(4, 1, 1, _abi.addr(sreq), _abi.addr(req), 4, None,
                                        ctypes.byref(n_req)) == _abi.OK
    assert n_req.value == 4 and req.tolist() == [[0, 0, r, 0, 4] for r in range(4)]


@pytest.mark.parametrize("k", [1, 2, 4, 8, 128])
@pytest.mark.parametrize("n", [1, 3, 64])
def test_store_sizes_and_offsets(k, n):
    L = _abi.lib()
    col_off, dah_off = ctypes.c_size_t(0), ctypes.c_size_t(0)
    size = L.dagpu_proof_store_size(k, n, ctypes.byref(col_off), ctypes.byref(dah_off))
    rows, cols, dah = L.dagpu_row_nodes_size(k), L.dagpu_col_nodes_size(k), (8 * k - 1) * 32
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    assert col_off.value == up(n * rows) and dah_off.value == col_off.value + up(n * cols)
    assert size == dah_off.value + up(n * dah)
    assert L.dagpu_proof_store_workspace_size(k, n) > 0
    assert L.dagpu_nmt_prove_squares_workspace_size(1000) >= (4 * 1000 + 2) * 8


def test_store_sizes_invalid():
    L = _abi.lib()
    for k, n in ((0, 1), (3, 1), (4, 0), (1 << 20, 1)):
        assert L.dagpu_proof_store_size(k, n, None, None) == 0
        assert L.dagpu_proof_store_workspace_size(k, n) == 0
