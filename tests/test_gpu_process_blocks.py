"""Raw txs to verdicts with no host step in between (csrc/commit_plan.hip, the
counted kernels of csrc/blob_commit.hip, commit_plan_host.cpp;
device.commit_plan_device / proposal_check_device / proposal_verdict_device,
DeviceSquares.process_blocks):
  * the layout image, counts and blob_base built on the device equal the image
    restated in Python from the plans' blob tables and dagpu_commit_plan_host
    over the downloaded arena, word for word;
  * the counted commitment route equals check_commitments(expected="declared")
    bit for bit, also in a child process on the test build with a grid of two
    workgroups, so that the stride loops go round;
  * process_blocks equals da.process_proposal per block, codes and strings, in
    the reference's order, and downloads nothing but the verdicts;
  * refusals enqueue nothing."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import oracle
from celestia_da import _abi, da, square as sq
from celestia_da.device import DeviceSquares, commit_plan_device, plan_squares_device

import blobtx_validate_cases as cases
import process_blocks_cases as pc
from conftest import ORACLE, PKG, ROOT

pytestmark = pytest.mark.gpu

CODE = {name: i for i, name in enumerate(_abi.VERDICT_NAMES)}
NONE = _abi.BLOBTX_NONE


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


def _rejected_block(rng):
    """square.Construct refuses a normal tx behind a blob tx."""
    return [cases.valid_tx(rng, 1), cases.normal_tx(rng)]


def _k8_block(rng):
    block = [cases.normal_tx(rng)] + [pc.sized_tx(rng, (5, 9), i) for i in range(2)]
    assert sq.plan_native(block)[0] == 8
    return block


def test_layout_image(ctx):
    """Blobs of 1, 2, 64, 65 and 129 shares (65: 32 subtrees of 2 and one of 1;
    129: 32 of 4 and one of 1), a block of normal txs only, one the planner
    rejects and one of width 8."""
    rng = random.Random(41)
    blocks = [[cases.normal_tx(rng), pc.sized_tx(rng, (1, 2, 64, 65))], [cases.normal_tx(rng) for _ in range(3)],
              _rejected_block(rng), [pc.sized_tx(rng, (129, 2))], _k8_block(rng), pc.k16_block(rng)]
    n = len(blocks)
    p = plan_squares_device(blocks, ctx=ctx)
    got = commit_plan_device(p, 16, ctx=ctx)
    torch.cuda.synchronize()
    assert p._rec is None and p._plans is None  # nothing was downloaded to lay the tables out
    tables = got.tables.cpu().numpy().view(np.uint32)
    counts = got.counts.cpu().numpy().view(np.uint32)
    base = got.blob_base.cpu().numpy().view(np.uint64)
    rec, plans = p.records_host(), p.plans_host()
    assert [int(rec[i]["k"]) for i in (0, 3, 4, 5)] == [16, 16, 8, 16] and rec[2]["status"] != 0
    records = [(i, int(t[0]), int(t[1])) for i, plan in enumerate(plans)
               if plan is not None and rec[i]["k"] == 16 for t in sq.plan_blobs(plan)]
    assert sorted(r[2] for r in records if r[0] in (0, 3)) == [1, 2, 2, 64, 65, 129]
    words, want_counts, want_base = pc.python_layout(records, 16, n)
    assert np.array_equal(counts, want_counts) and np.array_equal(base, want_base)
    assert want_counts[3] == 32 + 32 and want_counts[4] == 64  # the 64-share blob: 64 one-leaf subtrees
    assert np.array_equal(tables[:words.size], words)
    host = pc.plan_host(16, n, p.arena.cpu().numpy(), np.ascontiguousarray(rec))
    assert np.array_equal(host[0][:words.size], words) and np.array_equal(host[1], counts)
    assert np.array_equal(host[2], base)
    # the same arena for width 8: only block 4 contributes
    got8 = commit_plan_device(p, 8, ctx=ctx)
    torch.cuda.synchronize()
    records8 = [(4, int(t[0]), int(t[1])) for t in sq.plan_blobs(plans[4])]
    words8, counts8, base8 = pc.python_layout(records8, 8, n)
    assert np.array_equal(got8.counts.cpu().numpy().view(np.uint32), counts8)
    assert np.array_equal(got8.blob_base.cpu().numpy().view(np.uint64), base8)
    assert np.array_equal(got8.tables.cpu().numpy().view(np.uint32)[:words8.size], words8)


def test_counted_route_equals_check_commitments(ctx):
    report = pc.counted_route_report(ctx).split()
    # 48 + 6 + 3 + 48 blobs; 32 + 32 + 32 work items; the flipped row and the two rows of the bad signer
    assert report == ["SAME", "105", "96", "3"], report


def test_counted_route_on_a_grid_of_two():
    """The test build caps the counted kernels' grids at DAGPU_TEST_COMMIT_GRID
    workgroups: with 2, every stride loop goes round many times (105 blobs,
    96 work items, 560 shares).  The product library never reads the variable."""
    script = ("import sys; sys.path[:0] = sys.argv[1:]; import process_blocks_cases as pc; pc.child_main()")
    env = dict(os.environ, DAGPU_LIB=os.path.join(PKG, "libdagpu_test.so"), DAGPU_TEST_COMMIT_GRID="2")
    r = subprocess.run([sys.executable, "-c", script, PKG, ORACLE, os.path.join(ROOT, "tests"), ROOT], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["SAME", "105", "96", "3"], r.stdout
    assert b"DAGPU_TEST_COMMIT_GRID" not in open(os.path.join(PKG, "libdagpu.so"), "rb").read()
    assert b"DAGPU_TEST_COMMIT_GRID" in open(os.path.join(PKG, "libdagpu_test.so"), "rb").read()


def _data_root(shares):
    k = sq.size(len(shares))
    return oracle.extend_and_dah(np.frombuffer(b"".join(shares), np.uint8).reshape(k * k, 512), k)[3]


def _root_of(block):
    try:
        return _data_root(sq.construct(block).square_bytes())
    except ValueError:
        return bytes(32)


def _compare(d, blocks, hashes=None, sizes=None, other_width=()):
    """process_blocks against da.process_proposal block by block."""
    got = d.process_blocks(blocks, data_hashes=hashes, square_sizes=sizes)
    assert d._planned._rec is None and d._planned._plans is None  # nothing but the verdicts came back
    records = d.verdicts.tolist()
    planner = d._planned.status_host()
    for i, block in enumerate(blocks):
        want = da.process_proposal(block, data_hash=None if hashes is None else hashes[i],
                                   square_size=None if sizes is None else sizes[i],
                                   create_commitment=pc.commitment, data_root=_data_root)
        if i in other_width and want[2][0] in (CODE["ACCEPT"], CODE["DATA_ROOT_DIFFERS"]):
            # no square of this width was written: never an accept
            assert got[i] == (False, da.verdict_reason(CODE["NOT_JUDGED"])) and records[i][0] == CODE["NOT_JUDGED"], i
            continue
        assert got[i] == want[:2], (i, got[i], want)
        code, tx, word, aux = want[2]
        if code == CODE["CONSTRUCT_FAILED"]:
            word = int(planner[i])  # the mirror does not restate the planner's word
            assert word != 0
        assert records[i] == [code, tx, word, aux], (i, records[i], want)
    return got


def test_verdicts_in_the_reference_order(ctx):
    rng = random.Random(42)
    blocks = [pc.k16_block(rng) for _ in range(6)]
    blocks[1][9] = pc.flip_commitment(blocks[1][9])  # the tx-9 mismatch
    blocks[2][7] = pc.bad_signer(blocks[2][7])       # the tx-7 bad signer
    blocks[3][9] = pc.flip_commitment(blocks[3][9])  # both in one block: tx 12 stateless, tx 9 mismatch
    blocks[3][12] = pc.bad_signer(blocks[3][12])
    blocks[4][1] = cases.kind_cases()["NON_BLOB_TX_HAS_PFB"][0]
    hashes = [_root_of(b) for b in blocks]
    hashes[5] = hashes[5][:31] + bytes([hashes[5][31] ^ 1])  # a wrong data hash
    d = DeviceSquares(16, 6, ctx=ctx)
    got = _compare(d, blocks, hashes, [16] * 6)
    assert got == [(True, ""), (False, "invalid blob tx 9: ErrInvalidShareCommitment"),
                   (False, "invalid blob tx 7: ErrInvalidAddress"),
                   (False, "invalid blob tx 9: ErrInvalidShareCommitment"),
                   (False, "tx 1 has PFB but is not a blob tx"),
                   (False, "proposed data root differs from calculated data root")]
    assert d.verdicts[1].tolist() == [CODE["INVALID_SHARE_COMMITMENT"], 9, 0, 1]
    # without hashes and sizes the last block passes
    assert _compare(d, blocks)[5] == (True, "")
    # the follow-ups of load_txs(plan="device") work on the same object
    assert len(d.tx_table()) > 0


def test_verdicts_of_blocks_without_a_square(ctx):
    rng = random.Random(43)
    both = pc.k16_block(rng)
    both[9] = pc.bad_signer(pc.flip_commitment(both[9]))  # one tx failing both ways: the stateless word
    rejected_stateless = _rejected_block(rng)
    rejected_stateless[0] = pc.bad_signer(rejected_stateless[0])
    blocks = [pc.k16_block(rng), _rejected_block(rng), _k8_block(rng), both, rejected_stateless, _k8_block(rng)]
    hashes = [_root_of(b) for b in blocks]
    sizes = [32, 16, 8, 16, 16, 16]  # block 0: a wrong square size; block 5: width 8 proposed as 16
    d = DeviceSquares(16, 6, ctx=ctx)
    got = _compare(d, blocks, hashes, sizes, other_width=(2, 5))
    assert got[0] == (False, "proposed square size differs from calculated square size")
    assert got[1] == (False, "failure to compute data square from transactions:")
    assert got[3] == (False, "invalid blob tx 9: ErrInvalidAddress")
    assert got[4] == (False, "invalid blob tx 0: ErrInvalidAddress")
    assert got[5] == (False, "proposed square size differs from calculated square size")
    assert d.verdicts[0].tolist() == [CODE["SQUARE_SIZE_DIFFERS"], NONE, 0, 16]
    assert d.verdicts[5].tolist() == [CODE["SQUARE_SIZE_DIFFERS"], NONE, 0, 8]
    assert not any(accept for accept, _ in got[1:])


def test_a_batch_with_no_blob(ctx):
    rng = random.Random(44)
    blocks = [[cases.normal_tx(rng) for _ in range(200)] for _ in range(3)] + [[cases.normal_tx(rng)]]
    assert [sq.plan_native(b)[0] for b in blocks] == [16, 16, 16, 1]
    hashes = [_root_of(b) for b in blocks]
    d = DeviceSquares(16, 4, ctx=ctx)
    got = _compare(d, blocks, hashes, None, other_width=(3,))
    assert got[:3] == [(True, "")] * 3
    assert d.proposal_check.counts.cpu().numpy().tolist() == [0] * 8
    assert not d.proposal_check.blob_base.cpu().numpy().any()


def test_process_proposals_is_unchanged(ctx):
    """The parent's composition on the object process_blocks left returns what
    it returns behind load_txs(plan="device")."""
    blocks = pc.counted_blocks()
    d = DeviceSquares(16, 4, ctx=ctx)
    d.load_txs(blocks, plan="device")
    d.extend()
    torch.cuda.synchronize()
    hashes = [bytes(h) for h in d.dah.cpu().numpy()]
    before = d.process_proposals(data_hashes=hashes)
    e = DeviceSquares(16, 4, ctx=ctx)
    mine = e.process_blocks(blocks, data_hashes=hashes)
    assert e.process_proposals(data_hashes=hashes) == before
    assert before == [(False, "invalid blob tx: ErrInvalidShareCommitment"), (True, ""), (True, ""),
                      (False, "invalid blob tx 7: ErrInvalidAddress")]
    assert mine == [(False, "invalid blob tx 9: ErrInvalidShareCommitment"), (True, ""), (True, ""),
                    (False, "invalid blob tx 7: ErrInvalidAddress")]


def test_refusals_enqueue_nothing(ctx):
    rng = random.Random(45)
    blocks = [pc.k16_block(rng), [pc.sized_tx(rng, (65, 3))]]
    n, k, cap = 2, 16, 2 * 16 * 16
    d = DeviceSquares(k, n, ctx=ctx)
    p = plan_squares_device(blocks, ctx=ctx, k=k, out=d.ods.view(-1), square_stride=k * k * 512, row_pitch=k * 512)
    torch.cuda.synchronize()
    L = ctx._L
    ntx = int(p.tx_lens.size)

    def filled(shape, dtype):
        return torch.full(shape, 0x5A if dtype == torch.uint8 else 0x5A5A5A5A, dtype=dtype, device="cuda")

    outs = dict(tx_status=filled((ntx,), torch.int32), block_status=filled((n, 2), torch.int32),
                expected=filled((cap, 32), torch.uint8), commitments=filled((cap, 32), torch.uint8),
                blob_status=filled((cap,), torch.int32), row_tx=filled((cap, 2), torch.int32),
                square_status=filled((n,), torch.int32), counts=filled((8,), torch.int32),
                blob_base=filled((2 * (n + 1),), torch.int32))
    verdicts = filled((n, 4), torch.int32)
    ws = torch.empty((L.dagpu_proposal_check_workspace_size(k, n, ntx) + 16,), dtype=torch.uint8, device="cuda")
    hashes, sizes = np.zeros(32 * n, np.uint8), np.full(n, k, np.uint32)

    def check(**over):
        a = dict(k=k, src=_abi.addr(p.src), offs=_abi.addr(p.src_offs), ntx=_abi.addr(p.ntx), lens=_abi.addr(p.tx_lens),
                 plans=_abi.addr(p.arena), records=_abi.addr(p.records), squares=_abi.addr(d.ods), pitch=k * 512,
                 threshold=64, ws=_abi.addr(ws), **{name: _abi.addr(t) for name, t in outs.items()})
        a.update(over)
        return L.dagpu_proposal_check_device(
            ctx.handle, a["k"], n, a["src"], a["offs"], p.src_bytes, a["ntx"], a["lens"], a["plans"], p.arena_cap,
            a["records"], a["squares"], k * k * 512, a["pitch"], a["threshold"], a["tx_status"], a["block_status"],
            a["expected"], a["commitments"], a["blob_status"], a["row_tx"], a["square_status"], a["counts"],
            a["blob_base"], a["ws"], None)

    def verdict(**over):
        a = dict(k=k, records=_abi.addr(p.records), block_status=_abi.addr(outs["block_status"]),
                 blob_status=_abi.addr(outs["blob_status"]), row_tx=_abi.addr(outs["row_tx"]),
                 blob_base=_abi.addr(outs["blob_base"]), status=_abi.addr(d.status), dah=_abi.addr(d.dah),
                 hashes=_abi.addr(hashes), sizes=_abi.addr(sizes), verdicts=_abi.addr(verdicts), ws=_abi.addr(ws))
        a.update(over)
        return L.dagpu_proposal_verdict_device(ctx.handle, a["k"], n, a["records"], a["block_status"],
                                               a["blob_status"], a["row_tx"], a["blob_base"], a["status"], a["dah"],
                                               a["hashes"], a["sizes"], a["verdicts"], a["ws"], None)

    arg, unsupported = _abi.ERR_ARG, _abi.ERR_UNSUPPORTED
    refusals = [(check, "null", arg, dict(commitments=None)), (check, "null", arg, dict(row_tx=None)),
                (check, "null", arg, dict(squares=None)), (check, "null", arg, dict(counts=None)),
                (check, "null", arg, dict(tx_status=None)), (check, "null", arg, dict(offs=None)),
                (check, "aligned", arg, dict(ws=_abi.addr(ws) + 8)),
                (check, "aligned", arg, dict(records=_abi.addr(p.records) + 8)),
                (check, "multiples of 16", arg, dict(squares=_abi.addr(d.ods) + 8)),
                (check, "power of two", arg, dict(k=12)), (check, "above 1024", unsupported, dict(k=2048)),
                (check, "threshold", arg, dict(threshold=0)), (check, "row_pitch below", arg, dict(pitch=k * 512 - 16)),
                (verdict, "null", arg, dict(verdicts=None)), (verdict, "null", arg, dict(row_tx=None)),
                (verdict, "null", arg, dict(records=None)), (verdict, "without d_dah", arg, dict(dah=None)),
                (verdict, "aligned", arg, dict(ws=_abi.addr(ws) + 8)),
                (verdict, "aligned", arg, dict(verdicts=_abi.addr(verdicts) + 4)),
                (verdict, "power of two", arg, dict(k=12)), (verdict, "above 1024", unsupported, dict(k=2048))]
    for call, text, code, over in refusals:
        assert call(**over) == code, (text, over)
        assert text in ctx.last_error(), (text, ctx.last_error())
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert (t == (0x5A if t.dtype == torch.uint8 else 0x5A5A5A5A)).all(), name
    assert (verdicts == 0x5A5A5A5A).all()
    # the accepted calls write their outputs, with the caller's workspace and with the library's
    for over in ({}, dict(ws=None)):
        assert check(**over) == 0, ctx.last_error()
        d.extend()
        assert verdict(**over) == 0, ctx.last_error()
        torch.cuda.synchronize()
        # 48 blobs of 3 shares (one-leaf subtrees), then 65 shares (32 subtrees of 2 and one of 1) and 3
        assert outs["counts"].cpu().numpy().tolist()[:4] == [50, 48 * 3 + 68, 48 * 3 + 33 + 3, 32]
        assert outs["blob_base"].cpu().numpy().view(np.uint64).tolist() == [0, 48, 50]
        assert not outs["blob_status"].any() and not outs["square_status"].any()
        assert (outs["row_tx"][:50] >= 0).all()
        # hashes of zeros: both blocks' data roots differ
        assert verdicts.cpu().numpy().tolist() == [[CODE["DATA_ROOT_DIFFERS"], -1, 0, 0]] * 2
