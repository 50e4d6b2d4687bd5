"""The device planner on the GPU (csrc/square_plan.hip: dagpu_square_plan_device,
dagpu_square_construct_device, DeviceSquares.load_txs(plan="device")) against
the host planner and the host square (square.plan_native, construct_native):
plans byte for byte, every downloaded plan through dagpu_square_plan_check,
statuses as the host's errors map, squares bit for bit in the packed layout and
as Q0 at the EDS pitch, untouched windows for what the call skips."""
import collections

import numpy as np
import pytest
import torch

from celestia_da import _abi, da, square as sq
from celestia_da.device import DeviceSquares, construct_squares_device, plan_squares_device

import square_plan_device_cases as cases
from square_corpus import corpus, full_block
from test_square_plan_device_host import check_block, host_verdict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


def _by_width(blocks):
    """{(k, max square size): [(name, txs, m, host ODS)]} of the blocks; k = 0: those Construct rejects."""
    groups = collections.defaultdict(list)
    for name, txs, m in blocks:
        try:
            k, ods = sq.construct_native(txs, m)
        except sq.ShareError:
            k, ods = 0, None
        groups[(k, m)].append((name, txs, m, ods))
    return dict(groups)


@pytest.fixture(scope="module")
def corpus_by_width():
    return _by_width(corpus())


@pytest.fixture(scope="module")
def crafted_by_width():
    return _by_width(cases.all_blocks())


def _check_plans(p, blocks):
    """Plans, records and statuses of a PlannedSquares against the host planner."""
    L = _abi.lib()
    rec, status, plans = p.records_host(), p.status_host(), p.plans_host()
    used = int(max((int(r["plan_off"]) + int(r["plan_bytes"]) for r in rec), default=0))
    arena = p.arena[:used].cpu().numpy() if used else np.zeros(0, np.uint8)
    spans = sorted((int(r["plan_off"]), int(r["plan_off"]) + int(r["plan_bytes"])) for r in rec if r["plan_bytes"])
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    for i, (name, txs, m, _) in enumerate(blocks):
        word = int(status[i])
        kind, index = sq.plan_status(word)
        if kind == _abi.PLAN_WIDTH:  # the writer's verdict on a block the planner accepted
            assert index == int(rec[i]["k"]) and int(rec[i]["status"]) == 0
            word = 0
        r = rec[i].copy()
        r["status"] = word
        if check_block(name, txs, m, arena, r, word):
            assert L.dagpu_square_plan_check(_abi.addr(plans[i]), plans[i].size, sum(map(len, txs))) == 0, name


def _construct(ctx, k, m, blocks, in_place):
    n = len(blocks)
    if in_place:
        stride, pitch = 4 * k * k * 512, 2 * k * 512
    else:
        stride, pitch = k * k * 512, k * 512
    out = torch.full((n * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    p = construct_squares_device(k, [b[1] for b in blocks], out, stride, pitch, max_square_size=m, ctx=ctx)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    if in_place:
        rows = host.reshape(n, 2 * k, 2 * k * 512)
        assert (rows[:, :k, k * 512:] == 0xA5).all() and (rows[:, k:] == 0xA5).all()
        return p, np.ascontiguousarray(rows[:, :k, :k * 512]).reshape(n, k * k * 512)
    return p, host.reshape(n, k * k * 512)


def _check_width_groups(ctx, groups):
    for (k, m), blocks in sorted(groups.items()):
        if k == 0:  # the rejected blocks: planned in one call, no square
            _check_plans(plan_squares_device([b[1] for b in blocks], max_square_size=m, ctx=ctx), blocks)
            continue
        for in_place in (False, True):
            p, got = _construct(ctx, k, m, blocks, in_place)
            assert (p.status_host() == 0).all()
            for (name, _, _, ods), g in zip(blocks, got):
                assert (g == ods).all(), (k, name, in_place, int((g != ods).argmax()))
        _check_plans(p, blocks)


def test_corpus_by_width(ctx, corpus_by_width):
    assert sorted({k for k, _ in corpus_by_width}) == [0, 1, 2, 4, 8, 16, 32, 64]
    _check_width_groups(ctx, corpus_by_width)


def test_crafted_blocks_by_width(ctx, crafted_by_width):
    """The hand-made parser and layout blocks of the CPU list, one batch per
    width and max square size; the first-failure blocks have max square size 2 and 4."""
    groups = crafted_by_width
    assert len(groups[(0, 128)]) >= 40 and (128, 128) in groups and (0, 2) in groups and len(groups[(0, 4)]) >= 5
    _check_width_groups(ctx, groups)


@pytest.mark.parametrize("name,blocks,m", cases.batches(), ids=[b[0] for b in cases.batches()])
def test_batches(ctx, name, blocks, m):
    _check_plans(plan_squares_device(blocks, max_square_size=m, ctx=ctx), [(f"{name}[{i}]", txs, m, None)
                                                                              for i, txs in enumerate(blocks)])


def test_plan_device_equals_emulation(ctx):
    """square.plan_device and square.plan_emulate: the same records (but for
    where each plan lies in the arena), statuses and plans."""
    blocks = [txs for name, txs, m in cases.all_blocks() if m == 128 and "_at_1638" not in name]
    arena, rec, status = sq.plan_device(blocks, ctx=ctx)
    e_arena, e_rec, e_status = sq.plan_emulate(blocks)
    host = arena.cpu().numpy()
    assert (status == e_status).all() and (status != 0).any() and (status == 0).any()
    for field in ("src_off", "plan_bytes", "k", "status", "nblob"):
        assert (rec[field] == e_rec[field]).all(), field
    for r, e in zip(rec, e_rec):
        got, want = sq.plan_of(host, r), sq.plan_of(e_arena, e)
        assert (got is None) == (want is None) and (got is None or got.tobytes() == want.tobytes())


def test_mixed_call(ctx, crafted_by_width):
    """One accepted block of width k, one of another width, one rejected: only
    the accepted square changes; the other windows and the bytes between rows
    keep their 0xA5."""
    k, other = 8, 16
    good, wide, bad = crafted_by_width[(k, 128)][0], crafted_by_width[(other, 128)][0], crafted_by_width[(0, 128)][-1]
    blocks = [wide, good, bad]
    for in_place in (False, True):
        stride, pitch = (4 * k * k * 512, 2 * k * 512) if in_place else (k * (k * 512 + 16) + 64, k * 512 + 16)
        out = torch.full((3 * stride,), 0xA5, dtype=torch.uint8, device="cuda")
        p = construct_squares_device(k, [b[1] for b in blocks], out, stride, pitch, ctx=ctx)
        status = p.status_host()
        host = out.cpu().numpy().reshape(3, stride)
        assert (host[0] == 0xA5).all() and (host[2] == 0xA5).all()
        rows = host[1][:k * pitch].reshape(k, pitch)
        assert (rows[:, :k * 512].reshape(-1) == good[3]).all()
        assert (rows[:, k * 512:] == 0xA5).all() and (host[1][k * pitch:] == 0xA5).all()
        assert sq.plan_status(status[0]) == (_abi.PLAN_WIDTH, other) and status[1] == 0
        _, _, err = host_verdict(bad[1], 128)
        assert sq.plan_status(status[2])[0] == err[0] and (err[1] is None or sq.plan_status(status[2])[1] == err[1])
        _check_plans(p, blocks)


def test_load_txs_device(ctx, corpus_by_width, crafted_by_width):
    """load_txs(plan="device") then extend(): the DAHs of the plan="host"
    route; check_commitments through the lazily downloaded plans; a rejected
    block raises the host route's exception."""
    k = 32
    blocks = [b[1] for b in corpus_by_width[(k, 128)][:4]]
    n = len(blocks)
    assert n >= 3
    for in_place in (True, False):
        dev, ref = DeviceSquares(k, n, ctx=ctx, in_place=in_place), DeviceSquares(k, n, ctx=ctx, in_place=in_place)
        dev.load_txs(blocks, plan="device")
        ref.load_txs(blocks, plan="host")
        dev.extend()
        ref.extend()
        torch.cuda.synchronize()
        assert (dev.status.cpu() == 0).all() and torch.equal(dev.dah.cpu(), ref.dah.cpu())
        assert torch.equal(dev.eds.cpu(), ref.eds.cpu())
        assert (dev.blob_table()[0] == ref.blob_table()[0]).all() and (dev.blob_table()[1] == ref.blob_table()[1]).all()
        com_d, st_d, sq_d = dev.check_commitments()
        com_r, _, _ = ref.check_commitments()
        torch.cuda.synchronize()
        assert torch.equal(com_d.cpu(), com_r.cpu()) and (st_d.cpu() == 0).all() and (sq_d.cpu() == 0).all()
    rejected = next(b[1] for b in crafted_by_width[(0, 128)] if b[0] == "share_version_1_alone")
    for route in ("host", "device"):
        d = DeviceSquares(k, n, ctx=ctx)
        with pytest.raises(sq.ShareError) as e:
            d.load_txs(blocks[:n - 1] + [rejected], plan=route)
        if route == "host":
            want = str(e.value)
        else:
            assert str(e.value) == want
    other = corpus_by_width[(64, 128)][0][1]
    errors = []
    for route in ("host", "device"):
        with pytest.raises(da.DAError) as e:
            DeviceSquares(k, n, ctx=ctx).load_txs(blocks[:n - 1] + [other], plan=route)
        errors.append(str(e.value))
    assert errors[0] == errors[1]
    # a block of another width in front of a rejected one: both routes raise the rejected block's error
    errors = []
    for route in ("host", "device"):
        with pytest.raises(sq.ShareError) as e:
            DeviceSquares(k, n, ctx=ctx).load_txs([other] + blocks[:n - 2] + [rejected], plan=route)
        errors.append(str(e.value))
    assert errors[0] == errors[1]


def test_full_block(ctx):
    """2,000 normal + 2,000 blob txs, k = 128: plan bytes and square equal the host's."""
    txs = full_block()
    k, ods = sq.construct_native(txs)
    assert k == 128
    out = torch.empty((k * k * 512,), dtype=torch.uint8, device="cuda")
    p = construct_squares_device(k, [txs], out, k * k * 512, k * 512, ctx=ctx)
    assert p.status_host()[0] == 0
    assert (out.cpu().numpy() == ods).all()
    _check_plans(p, [("full_block", txs, 128, ods)])
