"""Squares assembled on the GPU from raw txs (dagpu_square_write_device,
csrc/square_write.hip; square.construct_device, DeviceSquares.load_txs) against
the host constructor dagpu_square_construct (square.construct_native), byte for
byte: the corpus of tests/square_corpus.py batched by square width, Q0 written
in place at the EDS row pitch and extended, one full 128 x 128 block, and the
host-side rejection of a batch of mixed widths."""
import collections

import numpy as np
import pytest
import torch

from celestia_da import _abi, da, square as sq
from celestia_da.device import DeviceSquares, write_squares_device

from square_corpus import corpus, full_block

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def by_width():
    """{k: [(name, txs, host ODS, plan)]} of the corpus blocks Construct accepts."""
    groups = collections.defaultdict(list)
    for name, txs, m in corpus():
        try:
            k, ods = sq.construct_native(txs, m)
        except sq.ShareError:
            continue
        pk, plan = sq.plan_native(txs, m)
        assert pk == k
        groups[k].append((name, txs, ods, plan))
    return dict(groups)


def _write(ctx, k, blocks, lead=0):
    n = len(blocks)
    out = torch.full((n * k * k * 512,), 0xA5, dtype=torch.uint8, device="cuda")
    write_squares_device(k, [b[3] for b in blocks], [b"".join(b[1]) for b in blocks], out, k * k * 512, k * 512,
                         ctx=ctx, lead=lead)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, k * k * 512)


def test_corpus_batched_by_width(ctx, by_width):
    """Every accepted corpus block, one call per width: n >= 3 different blocks
    of unequal source lengths packed back to back behind 5 unused bytes."""
    assert sorted(by_width) == [1, 2, 4, 8, 16, 32, 64]
    assert any(len(v) >= 3 and len({len(b"".join(b[1])) for b in v}) >= 3 for v in by_width.values())
    for k, blocks in sorted(by_width.items()):
        got = _write(ctx, k, blocks, lead=5)
        for (name, _, ods, _), g in zip(blocks, got):
            assert (g == ods).all(), (k, name, int((g != ods).argmax()))


def test_single_block_calls(ctx, by_width):
    """n = 1, the source at offsets 0 and 3 of the uploaded buffer."""
    for k, blocks in sorted(by_width.items()):
        for lead in (0, 3):
            got = _write(ctx, k, blocks[-1:], lead=lead)
            assert (got[0] == blocks[-1][2]).all(), (k, blocks[-1][0], lead)


def test_construct_device(ctx, by_width):
    for k in (1, 16):
        name, txs, ods, _ = by_width[k][0]
        dk, dev = sq.construct_device(txs, ctx=ctx)
        assert dk == k and dev.is_cuda and (dev.cpu().numpy() == ods).all(), name


def test_q0_in_place_then_extend(ctx, by_width):
    k, blocks = max(by_width.items(), key=lambda kv: (len(kv[1]) >= 3 and kv[0] >= 4, kv[0]))
    blocks = blocks[:4]
    n = len(blocks)
    assert n >= 3 and k >= 4
    d = DeviceSquares(k, n, ctx=ctx, in_place=True)
    d.eds.fill_(0xA5)
    d.load_txs([b[1] for b in blocks])
    torch.cuda.synchronize()
    eds = d.eds.cpu().numpy().reshape(n, 2 * k, 2 * k * 512)
    for i, b in enumerate(blocks):
        assert (eds[i, :k, :k * 512].reshape(-1) == b[2]).all(), b[0]
    assert (eds[:, :k, k * 512:] == 0xA5).all() and (eds[:, k:] == 0xA5).all()
    d.extend()
    ref = DeviceSquares(k, n, ctx=ctx)
    ref.load_ods(np.stack([b[2] for b in blocks]))
    ref.extend()
    torch.cuda.synchronize()
    assert (d.status.cpu() == 0).all() and (ref.status.cpu() == 0).all()
    assert torch.equal(d.dah.cpu(), ref.dah.cpu())
    assert torch.equal(d.row_roots.cpu(), ref.row_roots.cpu()) and torch.equal(d.col_roots.cpu(), ref.col_roots.cpu())
    # the packed target of load_txs
    p = DeviceSquares(k, n, ctx=ctx)
    p.ods.fill_(0xA5)
    p.load_txs([b[1] for b in blocks], threads=1)
    torch.cuda.synchronize()
    assert (p.ods.cpu().numpy() == np.stack([b[2] for b in blocks])).all()


def test_full_block(ctx):
    """The one large case: 2,000 normal + 2,000 blob txs, k = 128."""
    txs = full_block()
    k, ods = sq.construct_native(txs)
    assert k == 128
    dk, dev = sq.construct_device(txs, ctx=ctx)
    assert dk == k and (dev.cpu().numpy() == ods).all()


def test_width_mismatch_launches_nothing(ctx, by_width):
    a, b = by_width[4][0], by_width[8][0]
    out = torch.full((2 * 8 * 8 * 512,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(da.DAError) as e:
        write_squares_device(8, [b[3], a[3]], [b"".join(b[1]), b"".join(a[1])], out, 8 * 8 * 512, 8 * 512, ctx=ctx)
    assert e.value.code == _abi.ERR_ARG
    assert "block 1" in str(e.value) and "width 4" in str(e.value) and "width 8" in str(e.value)
    torch.cuda.synchronize()
    assert (out.cpu() == 0xA5).all()
    d = DeviceSquares(8, 2, ctx=ctx, in_place=True)
    d.eds.fill_(0xA5)
    with pytest.raises(da.DAError, match="block 1 has square width 4"):
        d.load_txs([b[1], a[1]])
    torch.cuda.synchronize()
    assert (d.eds.cpu() == 0xA5).all()
    # a plan the checker rejects never reaches the kernel either
    with pytest.raises(da.DAError, match="block 0: square plan"):
        write_squares_device(8, [b[3][:-16].copy()], [b"".join(b[1])], out, 8 * 8 * 512, 8 * 512, ctx=ctx)
    torch.cuda.synchronize()
    assert (out.cpu() == 0xA5).all()
