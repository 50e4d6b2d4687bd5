"""Square plans (csrc/square.cpp dagpu_square_plan, dagpu_square_plan_check) and
the host executor (dagpu_square_plan_write_host), which runs the per-share
function of csrc/square_write.hpp that the kernel runs: plan + write gives the
bytes of dagpu_square_construct / dagpu_square_build, which
tests/test_square_native.py pins to the Python mirror of pkg/square.  Every
comparison is exact byte equality against those two calls.  Host only, no GPU.
"""
import ctypes
import random

import numpy as np
import pytest

from celestia_da import _abi
from celestia_da import blobtx as bt
from celestia_da import shares as sh
from celestia_da import square as sq

from square_corpus import corpus, two_wide_blobs
from test_square_host import NS1, normal_txs, random_blob_txs

CORPUS = corpus()


def _packed(txs):
    return np.frombuffer(b"".join(txs), np.uint8)


def _check(plan, src_bytes, plan_bytes=None):
    plan = np.ascontiguousarray(plan)
    return _abi.lib().dagpu_square_plan_check(_abi.addr(plan), plan.size if plan_bytes is None else plan_bytes,
                                              src_bytes)


def _host_result(txs, m):
    """('ok', k, ods) or ('error', type, message) of the host constructor."""
    try:
        k, ods = sq.construct_native(txs, m)
    except (sh.ShareError, ValueError) as e:
        return ("error", type(e), str(e))
    return ("ok", k, ods)


@pytest.mark.parametrize("case", range(len(CORPUS)), ids=[c[0] for c in CORPUS])
def test_plan_and_host_write_equal_construct(case):
    _, txs, m = CORPUS[case]
    want = _host_result(txs, m)
    if want[0] == "error":
        with pytest.raises(want[1]) as got:
            sq.plan_native(txs, m)
        assert str(got.value) == want[2]
        return
    k, plan = sq.plan_native(txs, m)
    assert k == want[1]
    src = _packed(txs)
    assert _check(plan, src.size) == 0
    got = sq.write_plan_host(plan, txs, k)
    assert got.shape == want[2].shape and (got == want[2]).all()
    # the checker: a truncated plan, and a source one byte short of the real one
    assert _check(plan[:-16].copy(), src.size) == _abi.ERR_ARG
    assert _check(plan, src.size, plan.size - 4) == _abi.ERR_ARG
    if src.size:
        assert _check(plan, src.size - 1) == _abi.ERR_ARG


def test_corpus_covers_what_it_claims():
    """k = 1 for the empty block, and both kinds of padding share in the host
    constructor's square of the two wide blobs."""
    assert sq.construct_native([])[0] == 1
    k, ods = sq.construct_native(two_wide_blobs())
    shares = [bytes(s) for s in ods.reshape(k * k, 512)]
    reserved = bytes(28) + b"\xff" + b"\x01" + bytes(482)
    ns_padding = NS1 + b"\x01" + bytes(482)
    assert shares.count(reserved) == 1 and shares.index(reserved) == 3
    assert shares.count(ns_padding) == 1 and shares.index(ns_padding) == 75
    assert shares[4][:29] == NS1 and shares[76][:29] != NS1
    # the corpus reaches every width from 1 to 64 (the larger random blocks are
    # 64 wide) and holds rejected blocks too
    widths = {r[1] for r in (_host_result(t, m) for _, t, m in CORPUS) if r[0] == "ok"}
    assert widths == {1, 2, 4, 8, 16, 32, 64}
    assert any(_host_result(t, m)[0] == "error" for _, t, m in CORPUS)


def test_build_mode_matches_build():
    rng = random.Random(13)
    normal = normal_txs(rng, 5)
    pfbs = random_blob_txs(rng, 5, 3000)
    txs = pfbs[:2] + normal + pfbs[2:]
    k, ods, kept = sq.build_native(txs, max_square_size=4)
    assert len(kept) < len(txs)  # oversubscribed
    pk, plan, pkept = sq.plan_native(txs, 4, build=True)
    assert pk == k and pkept == kept
    assert (sq.write_plan_host(plan, txs, k) == ods).all()


def _errors_match(txs, m):
    with pytest.raises(Exception) as want:
        sq.construct_native(txs, m)
    with pytest.raises(Exception) as got:
        sq.plan_native(txs, m)
    assert type(got.value) is type(want.value) and str(got.value) == str(want.value)
    return str(got.value)


def test_errors_match_construct():
    """The failing inputs of test_square_native.test_construct_errors_match
    and test_invalid_blobs: same exception (return code) and message."""
    rng = random.Random(1)
    send = normal_txs(rng, 250)
    pfbs = random_blob_txs(rng, 100, 1024)
    seen = [_errors_match(txs, m) for txs, m in ((send[:5] + pfbs + send[5:], 128), (send, 2), (pfbs, 2))]
    assert "can not be appended after blob tx" in seen[0] and "not enough space" in seen[1]
    for bad in (0, 13):
        assert "max square size must be" in _errors_match([b"x"], bad)
    for blob in (sh.Blob(NS1[1:], b""), sh.Blob(NS1[1:], b"d", share_version=1)):
        _errors_match([bt.marshal_blob_tx(b"pfb", blob)], 128)
    # the return codes themselves, and the argument errors of the shared prologue
    L = _abi.lib()
    out = np.empty(4096, np.uint8)
    need, k = ctypes.c_size_t(0), ctypes.c_uint32(0)
    buf, lens = sq._pack(send)
    rc = L.dagpu_square_plan(None, _abi.addr(buf), _abi.addr(lens), len(send), 2, 64, None, _abi.addr(out), out.size,
                             ctypes.addressof(need), ctypes.addressof(k))
    assert rc == _abi.ERR_SQUARE
    rc = L.dagpu_square_plan(None, None, None, 0, 64, 0, None, _abi.addr(out), out.size, ctypes.addressof(need),
                             ctypes.addressof(k))
    assert rc == _abi.ERR_ARG and L.dagpu_last_error(None).decode() == "subtree_root_threshold must be > 0"


def test_small_plan_buffer_reports_the_size():
    L = _abi.lib()
    txs = CORPUS[-1][1]
    k, plan = sq.plan_native(txs)
    buf, lens = sq._pack(txs)
    out = np.full(64, 0xA5, np.uint8)
    need, got_k = ctypes.c_size_t(0), ctypes.c_uint32(0)
    rc = L.dagpu_square_plan(None, _abi.addr(buf), _abi.addr(lens), len(txs), 128, 64, None, _abi.addr(out), out.size,
                             ctypes.addressof(need), ctypes.addressof(got_k))
    assert rc == _abi.ERR_ARG and need.value == plan.size and got_k.value == k
    assert L.dagpu_last_error(None).decode() == f"plan buffer too small: need {plan.size} bytes"
    assert (out == 0xA5).all()


def test_row_pitch_leaves_the_rest_untouched():
    for name in ("two_wide_blobs", "random_3", "tiny"):
        txs, m = next((t, m) for n, t, m in CORPUS if n == name)
        k, ods = sq.construct_native(txs, m)
        _, plan = sq.plan_native(txs, m)
        pitch = 2 * k * 512
        out = np.full(2 * k * pitch, 0xA5, np.uint8)  # an EDS-sized buffer, Q0 its window
        sq.write_plan_host(plan, txs, k, row_pitch=pitch, out=out)
        grid = out.reshape(2 * k, pitch)
        assert (grid[:k, :k * 512].reshape(-1) == ods).all()
        assert (grid[:k, k * 512:] == 0xA5).all() and (grid[k:] == 0xA5).all()


def test_plans_from_several_threads():
    from concurrent.futures import ThreadPoolExecutor
    blocks = [t for n, t, m in CORPUS if n.startswith("random_") and _host_result(t, m)[0] == "ok"]
    want = [sq.plan_native(t)[1].tobytes() for t in blocks]
    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(lambda t: sq.plan_native(t)[1].tobytes(), blocks * 4))
    assert got == want * 4
