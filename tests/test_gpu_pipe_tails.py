"""The sliced dagpu_extend_batch_device (csrc/dagpu.cpp extend_batch_sliced):
top-half leaves after the row pass, in-kernel status reset, the top tree
levels and the DAH once over the whole batch.  Small shapes with uneven cuts;
every comparison is bit-exact."""
import functools

import numpy as np
import pytest
import torch

import oracle
from celestia_da import da, synth
from celestia_da.device import DeviceSquares

pytestmark = pytest.mark.gpu

PUSH_ORDER = 1  # kStatusPushOrder (csrc/kernels.hpp): the device status word's bit

SMALL = [(k, n, s) for k in (1, 2, 4, 16) for (n, s) in ((17, 2), (26, 3), (35, 4), (67, 8))]
SHAPES = SMALL + [(128, 33, 4)]


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def squares(k, n, seed=0):
    """(n, k*k*512) sorted random blob squares, generated once per shape"""
    return synth.blob_squares(k, 7100 + 13 * k + seed, 0, n, threads=8)


@functools.lru_cache(maxsize=None)
def oracle_results(k, n, seed=0):
    """(row roots, column roots, DAHs) of squares(k, n, seed) from the CPU oracle, computed once"""
    rr, cr, dah = [], [], []
    for sq in squares(k, n, seed):
        _, r, c, d = oracle.extend_and_dah(sq.reshape(k * k, 512), k, want_eds=False)
        rr.append(r)
        cr.append(c)
        dah.append(np.frombuffer(d, np.uint8))
    return np.stack(rr), np.stack(cr), np.stack(dah)


def run(ds, monkeypatch, slices, m=None, ods=None):
    """one call under DAGPU_PIPE_SLICES=slices into poisoned outputs -> host copies"""
    monkeypatch.setenv("DAGPU_PIPE_SLICES", str(slices))
    for t in (ds.row_roots, ds.col_roots, ds.dah):
        t.fill_(0xA5)
    ds.status.fill_(-77)
    if ods is None:
        ds.extend()
        m = ds.n
    else:
        m = ds.extend_from(ods)
    torch.cuda.synchronize()
    return (ds.row_roots[:m].cpu().numpy(), ds.col_roots[:m].cpu().numpy(), ds.dah[:m].cpu().numpy(),
            ds.status[:m].cpu().numpy(), ds.eds[:m].cpu().numpy())


def same(got, want):
    for g, w, name in zip(got, want, ("row roots", "column roots", "DAH", "status", "EDS")):
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "separate"])
@pytest.mark.parametrize("k,n,slices", SHAPES, ids=lambda v: str(v))
def test_bit_exact_across_slicings(ctx, monkeypatch, k, n, slices, in_place):
    ods = squares(k, n)
    ds = DeviceSquares(k, n, ctx=ctx, in_place=in_place)
    ds.load_ods(ods)
    want = run(ds, monkeypatch, 1)
    assert (want[3] == 0).all()
    got = run(ds, monkeypatch, slices)
    same(got, want)
    if k <= 16:
        orr, ocr, odah = oracle_results(k, n)
        assert np.array_equal(got[0], orr) and np.array_equal(got[1], ocr) and np.array_equal(got[2], odah)


def test_unsliced_path_untouched(ctx, monkeypatch):
    """n = 7 at k = 16 is below the slicing threshold (S = 1) whatever is asked for"""
    k, n = 16, 7
    ods = squares(k, n)
    ds = DeviceSquares(k, n, ctx=ctx)
    ds.load_ods(ods)
    rr, cr, dah, st, _ = run(ds, monkeypatch, 4)
    _, hrr, hcr, hdah, hst = da.extend_batch(ods.reshape(-1), [k] * n, ctx)
    assert np.array_equal(dah, hdah) and (st == 0).all() and (hst == 0).all()
    assert np.array_equal(rr, np.stack(hrr)) and np.array_equal(cr, np.stack(hcr))


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "separate"])
def test_status_per_square_and_reset(ctx, monkeypatch, in_place):
    """Push-order violations in one square of the second slice and one of the
    last slice (cuts 0, 8, 17, 26, 35): exactly those report it.  Sorted data in
    the same buffers then gives 0 everywhere: the leaf launch reset the words."""
    k, n, slices = 16, 35, 4
    bad = (10, 30)
    good = squares(k, n)
    ods = good.copy()
    for i, (a, b) in zip(bad, ((0, 1), (k * 3 + 2, k * 4 + 2))):  # a row pair, a column pair
        sh = ods[i].reshape(k * k, 512)
        sh[[a, b]] = sh[[b, a]]
    ds = DeviceSquares(k, n, ctx=ctx, in_place=in_place)
    ds.load_ods(ods)
    want = np.zeros(n, np.int32)
    want[list(bad)] = PUSH_ORDER
    st1 = run(ds, monkeypatch, 1)[3]
    assert np.array_equal(st1, want)
    got = run(ds, monkeypatch, slices)
    assert np.array_equal(got[3], want), got[3]
    ds.load_ods(good)
    monkeypatch.setenv("DAGPU_PIPE_SLICES", str(slices))
    ds.extend()  # onto the status words the call above left behind
    torch.cuda.synchronize()
    assert (ds.status.cpu().numpy() == 0).all()
    orr, ocr, odah = oracle_results(k, n)
    assert np.array_equal(ds.dah.cpu().numpy(), odah) and np.array_equal(ds.row_roots.cpu().numpy(), orr)


def test_stale_deferred_state(ctx, monkeypatch):
    """n = 35, then extend_from with 17 other squares on the same buffers: the
    batch-wide records and namespace tables are rewritten by every call"""
    k, n, m = 16, 35, 17
    ds = DeviceSquares(k, n, ctx=ctx)
    ds.load_ods(squares(k, n))
    run(ds, monkeypatch, 4)
    other = squares(k, m, seed=1)
    assert not np.array_equal(other, squares(k, n)[:m])
    rr, cr, dah, st, _ = run(ds, monkeypatch, 4, ods=torch.from_numpy(other.copy()).cuda())
    fresh = DeviceSquares(k, m, ctx=ctx)
    fresh.load_ods(other)
    want = run(fresh, monkeypatch, 1)
    assert np.array_equal(rr, want[0]) and np.array_equal(cr, want[1]) and np.array_equal(dah, want[2])
    assert (st == 0).all()
    orr, ocr, odah = oracle_results(k, m, seed=1)
    assert np.array_equal(dah, odah) and np.array_equal(rr, orr) and np.array_equal(cr, ocr)


def test_workspace_bound(ctx, monkeypatch):
    """dagpu_workspace_size(k, n) plus a 4 KiB guard: the largest shape leaves the guard alone"""
    k, n, slices = 128, 33, 4
    ds = DeviceSquares(k, n, ctx=ctx, in_place=True)
    size = ctx._L.dagpu_workspace_size(k, n)
    assert ds.workspace.numel() == size
    ds.workspace = torch.empty((size + 4096,), dtype=torch.uint8, device=ds.eds.device)
    ds.workspace[size:].fill_(0x5C)
    ds.load_ods(squares(k, n))
    got = run(ds, monkeypatch, slices)
    assert bool((ds.workspace[size:] == 0x5C).all())
    ds.workspace = ds.workspace[:size].clone()
    same(run(ds, monkeypatch, 1), got)
