"""ValidateBlobTx's stateless rules on the GPU (csrc/blobtx_check.hip:
dagpu_blob_tx_validate_device, device.validate_blob_txs_device,
DeviceSquares.validate_blob_txs / check_commitments(expected="declared") /
process_proposals) against dagpu_blob_tx_validate_host word for word and byte
for byte, against the expected words of the one-tx-per-kind block, and against
square.expected_commitments for every accepted block."""
import random

import numpy as np
import pytest
import torch

from celestia_da import _abi, blobtx as bt, da, shares as sh, square as sq
from celestia_da.device import DeviceSquares, plan_squares_device, validate_blob_txs_device

import blobtx_validate_cases as cases
from blobtx_validate_cases import K, NS, word

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


def _base_of(rec):
    counts = np.where(rec["plan_bytes"] == 0, 0, rec["nblob"]).astype(np.uint64)
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(counts, dtype=np.uint64)])


def _device_and_host(ctx, blocks, tie=True):
    """Plan `blocks` on the device, validate them there and with the host
    executor over the downloaded arena and records: the outputs must be equal.
    Returns (planned, tx_status, block_status, expected) as uint32 / uint8 arrays."""
    p = plan_squares_device(blocks, ctx=ctx)
    tx_status, block_status, expected = validate_blob_txs_device(p, blob_base="plans" if tie else None, ctx=ctx)
    torch.cuda.synchronize()
    got = (tx_status.cpu().numpy().view(np.uint32), block_status.cpu().numpy().view(np.uint32),
           expected.cpu().numpy())
    rec = p.records_host()
    base = _base_of(rec) if tie else None
    want = cases.validate_host(blocks, p.arena.cpu().numpy(), np.ascontiguousarray(rec), base)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)
    return (p,) + got


def test_every_kind(ctx):
    """One tx per kind in one block, the normal tx first; the planner refuses
    the block (an empty blob, invalid namespaces), so nothing is tied."""
    kinds = cases.kind_cases()
    names = ["NON_BLOB_TX_HAS_PFB"] + [k for k in bt.KIND_NAMES if k != "NON_BLOB_TX_HAS_PFB"]
    block = [kinds[k][0] for k in names]
    p, tx_status, block_status, expected = _device_and_host(ctx, [block], tie=False)
    assert tx_status.tolist() == [word(k, kinds[k][1]) for k in names]
    assert block_status.tolist() == [[0, word("NON_BLOB_TX_HAS_PFB", 1)]] and expected.shape == (0, 32)
    # the same block behind an accepted one, tied: the refused block owns no rows
    rng = random.Random(1)
    first = [cases.valid_tx(rng, 2)]
    p, tx_status, block_status, expected = _device_and_host(ctx, [first, block])
    assert p.status_host()[0] == 0 and p.status_host()[1] != 0
    assert tx_status.tolist() == [0] + [word(k, kinds[k][1]) for k in names]
    assert block_status.tolist() == [[0xFFFFFFFF, 0], [0, word("NON_BLOB_TX_HAS_PFB", 1)]]
    assert np.array_equal(expected, sq.expected_commitments(first, p.plans_host()[0]))


def _batch():
    rng = random.Random(2)
    big = [cases.normal_tx(rng) for _ in range(10)] + \
          [cases.valid_tx(rng, 1, sizes=(1, 40, 100)) for _ in range(290)]
    multi = [cases.normal_tx(rng)] + [cases.valid_tx(rng, n) for n in (5, 1, 70, 3, 2)]
    return [big, [], [cases.normal_tx(rng) for _ in range(7)], multi]


def test_batch_of_four(ctx):
    """300 txs (the lanes cross a 256-tx chunk and a workgroup boundary), an
    empty block, normal txs only, multi-blob txs."""
    blocks = _batch()
    p, tx_status, block_status, expected = _device_and_host(ctx, blocks)
    assert (p.status_host() == 0).all() and not tx_status.any() and tx_status.size == 300 + 0 + 7 + 6
    assert block_status.tolist() == [[0xFFFFFFFF, 0]] * 4
    base = _base_of(p.records_host())
    assert [int(base[i + 1] - base[i]) for i in range(4)] == [290, 0, 0, 81]
    for i, plan in enumerate(p.plans_host()):
        assert np.array_equal(expected[int(base[i]):int(base[i + 1])], sq.expected_commitments(blocks[i], plan)), i


def test_lowest_failing_tx(ctx):
    kinds = cases.kind_cases()
    blocks = _batch()
    for lo, hi in (("BAD_SIGNER", "NAMESPACE_MISMATCH"), ("NAMESPACE_MISMATCH", "BAD_SIGNER")):
        b = list(blocks[0])
        b[5], b[290] = kinds[lo][0], kinds[hi][0]
        _, tx_status, block_status, _ = _device_and_host(ctx, [blocks[3], b, blocks[0]], tie=False)
        assert block_status.tolist() == [[0xFFFFFFFF, 0], [5, word(lo, kinds[lo][1])], [0xFFFFFFFF, 0]]
        assert tx_status[6 + 290] == word(hi, kinds[hi][1]) and np.count_nonzero(tx_status) == 2


def _k16_block(rng, ntx=24):
    """Valid blob txs whose square has width 16: 24 txs of two blobs of 3 and 2 shares."""
    return [cases.normal_tx(rng), cases.normal_tx(rng)] + \
           [cases.valid_tx(rng, 2, sizes=(1000, 1400)) for _ in range(ntx)]


def test_end_to_end_k16(ctx):
    rng = random.Random(3)
    blocks = [_k16_block(rng) for _ in range(4)]
    # block 1: the PFB of tx 9 declares its second commitment with one bit flipped
    t, _ = bt.unmarshal_blob_tx(blocks[1][9])
    p = bt.pfb_of_tx(t.tx)
    good = p.share_commitments[1]
    p.share_commitments[1] = good[:7] + bytes([good[7] ^ 0x10]) + good[8:]
    blocks[1][9] = cases.blob_tx(t.blobs, p)
    flipped_off = len(b"".join(blocks[1][:9])) + bt.blob_data_offsets(blocks[1][9])[1][0]
    # block 2: tx 7 is an invalid blob tx the planner has no quarrel with
    t, _ = bt.unmarshal_blob_tx(blocks[2][7])
    p = bt.pfb_of_tx(t.tx)
    p.signer = p.signer[:-1] + ("q" if p.signer[-1] != "q" else "p")
    blocks[2][7] = cases.blob_tx(t.blobs, p)
    assert [sq.plan_native(b)[0] for b in blocks] == [16] * 4

    d = DeviceSquares(16, 4, ctx=ctx)
    with pytest.raises(ValueError, match="not resident"):
        d.validate_blob_txs()
    d.load_txs(blocks)  # the host-plan route uploads no raw txs
    with pytest.raises(ValueError, match="not resident"):
        d.check_commitments(expected="declared")
    d.load_txs(blocks, plan="device")
    com, st, sqs = d.check_commitments(expected="declared")
    tx_status, block_status, expected = d._validated
    torch.cuda.synchronize()
    rec, keys = d.blob_table()
    st, sqs = st.cpu().numpy(), sqs.cpu().numpy()
    assert sqs[0] == 0 and sqs[3] == 0 and sqs[1] == _abi.COMMIT_MISMATCH and sqs[2] == _abi.COMMIT_MISMATCH
    hit = np.flatnonzero(st)
    mine = np.flatnonzero((keys[:, 0] == 1) & (keys[:, 1] == flipped_off))
    assert len(mine) == 1 and set(hit[rec[hit, 0] == 1]) == {int(mine[0])}
    # block 2: exactly the two blobs of the invalid tx, whose rows are zero
    rows2 = hit[rec[hit, 0] == 2]
    assert len(rows2) == 2 and not expected.cpu().numpy()[rows2].any()
    assert set(hit) == set(rows2) | {int(mine[0])}
    assert block_status.cpu().numpy().view(np.uint32).tolist() == \
        [[0xFFFFFFFF, 0], [0xFFFFFFFF, 0], [7, word("BAD_SIGNER")], [0xFFFFFFFF, 0]]
    # the valid blocks' tables are square.expected_commitments'
    table = expected.cpu().numpy()
    for i in (0, 3):
        rows = np.flatnonzero(rec[:, 0] == i)
        assert np.array_equal(table[rows], sq.expected_commitments(blocks[i], d._host_plans()[i]))
        assert np.array_equal(table[rows], com.cpu().numpy()[rows])

    with pytest.raises(ValueError, match="extend"):
        d.process_proposals(data_hashes=[bytes(32)] * 4)
    assert d.process_proposals() == [(True, ""), (False, "invalid blob tx: ErrInvalidShareCommitment"),
                                     (False, "invalid blob tx 7: ErrInvalidAddress"), (True, "")]
    d.extend()
    torch.cuda.synchronize()
    hashes = [bytes(h) for h in d.dah.cpu().numpy()]
    hashes[3] = hashes[3][:31] + bytes([hashes[3][31] ^ 1])
    assert d.process_proposals(data_hashes=hashes) == [
        (True, ""), (False, "invalid blob tx: ErrInvalidShareCommitment"),
        (False, "invalid blob tx 7: ErrInvalidAddress"), (False, "proposed data root differs from calculated data root")]
    # a normal tx that carries a PFB
    blocks[0][1] = cases.kind_cases()["NON_BLOB_TX_HAS_PFB"][0]
    d.load_txs(blocks, plan="device")
    assert d.process_proposals()[0] == (False, "tx 1 has PFB but is not a blob tx")


def test_refusals_enqueue_nothing(ctx):
    rng = random.Random(4)
    blocks = [[cases.valid_tx(rng, 2)], [cases.valid_tx(rng, 1), cases.valid_tx(rng, 3)]]
    p = plan_squares_device(blocks, ctx=ctx)
    base = _base_of(p.records_host())
    L = ctx._L
    tx_status = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    block_status = torch.full((2, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    expected = torch.full((int(base[2]), 32), 0x5A, dtype=torch.uint8, device="cuda")
    ws = torch.empty((L.dagpu_blob_tx_validate_workspace_size(2, 3, int(base[2])) + 16,), dtype=torch.uint8,
                     device="cuda")

    def call(**over):
        a = dict(src=_abi.addr(p.src), offs=_abi.addr(p.src_offs), ntx=_abi.addr(p.ntx), lens=_abi.addr(p.tx_lens),
                 plans=_abi.addr(p.arena), records=_abi.addr(p.records), base=_abi.addr(base),
                 tx_status=_abi.addr(tx_status), block_status=_abi.addr(block_status), expected=_abi.addr(expected),
                 ws=_abi.addr(ws))
        a.update(over)
        return L.dagpu_blob_tx_validate_device(ctx.handle, 2, a["src"], a["offs"], p.src_bytes, a["ntx"], a["lens"],
                                               a["plans"], p.arena_cap, a["records"], a["base"], a["tx_status"],
                                               a["block_status"], a["expected"], a["ws"], None)

    descending = base.copy()
    descending[1] = descending[2] + 1
    late = base.copy() + 1
    short = p.tx_lens.copy()
    short[0] -= 1
    refusals = [("null", dict(tx_status=None)), ("null", dict(block_status=None)), ("null", dict(offs=None)),
                ("null", dict(ntx=None)), ("null", dict(expected=None)), ("null", dict(plans=None)),
                ("null", dict(records=None)), ("null d_src", dict(src=None)), ("tx_lens is required", dict(lens=None)),
                ("aligned", dict(ws=_abi.addr(ws) + 8)), ("aligned", dict(block_status=_abi.addr(block_status) + 4)),
                ("aligned", dict(records=_abi.addr(p.records) + 8)), ("ascend", dict(base=_abi.addr(descending))),
                ("start at 0", dict(base=_abi.addr(late))), ("add up", dict(lens=_abi.addr(short)))]
    for text, over in refusals:
        assert call(**over) == _abi.ERR_ARG, (text, over)
        assert text in ctx.last_error(), (text, ctx.last_error())
    assert L.dagpu_blob_tx_validate_device(None, 2, None, None, 0, None, None, None, 0, None, None, None, None, None,
                                           None, None) == _abi.ERR_ARG
    torch.cuda.synchronize()
    assert (tx_status == 0x5A5A5A5A).all() and (block_status == 0x5A5A5A5A).all() and (expected == 0x5A).all()
    # the accepted call writes all of them, with the caller's workspace and with the library's
    want = cases.validate_host(blocks, p.arena.cpu().numpy(), np.ascontiguousarray(p.records_host()), base)
    for over in ({}, dict(ws=None)):
        tx_status.fill_(0x5A5A5A5A), block_status.fill_(0x5A5A5A5A), expected.fill_(0x5A)
        assert call(**over) == 0, ctx.last_error()
        torch.cuda.synchronize()
        assert np.array_equal(tx_status[:3].cpu().numpy().view(np.uint32), want[0]) and tx_status[3] == 0x5A5A5A5A
        assert np.array_equal(block_status.cpu().numpy().view(np.uint32), want[1])
        assert np.array_equal(expected.cpu().numpy(), want[2])
        assert np.array_equal(want[2][:2], sq.expected_commitments(blocks[0], p.plans_host()[0]))
