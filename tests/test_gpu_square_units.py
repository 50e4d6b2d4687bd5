"""The tx index of squares resident in HBM (dagpu_square_units_device,
dagpu_square_read_units_device, csrc/square_units.hip; device.unit_table_device,
read_units_device, DeviceSquares.tx_table / tx_ranges / read_tx_units /
tx_proofs) against the host executor dagpu_square_units_host, the host loop that
emulates the kernels, and the Python mirror (tests/square_units_cases.py): the
corpus batched by width in both layouts, the hand-made k = 64 squares, the
tampered squares with the emulation's verdicts, a table that is too small, an
enqueue-only run on a side stream, selected units gathered into a pre-filled
buffer, and tx inclusion proofs against proof.new_tx_inclusion_proof."""
import collections

import numpy as np
import pytest
import torch

from celestia_da import _abi, da, proof
from celestia_da import shares as sh
from celestia_da import square as sq
from celestia_da.da import DAError
from celestia_da.device import DeviceSquares, read_units_device, scan_squares_device, unit_table_device

import square_read_cases as rc
import square_units_cases as cases
from test_gpu_square_read import SENTINEL, place
from test_square_host import NS1, NS2, NS3, blob_txs

pytestmark = pytest.mark.gpu

OK, HOST, OVERFLOW = _abi.UNITS_OK, _abi.UNITS_HOST, _abi.UNITS_OVERFLOW


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


def host_tables(L, k, host, n, stride, pitch, cap):
    """The scan, the host executor's and the emulation's tables of n squares
    where they lie in `host`; a square the serial walk refuses has executor None."""
    rec = np.zeros((n, k * k), sq.seq_dtype())
    scan = np.zeros((n, 8), np.int32)
    assert L.dagpu_square_scan_host(k, n, _abi.addr(host), stride, pitch, k * k, _abi.addr(rec), _abi.addr(scan)) == 0
    emu_u, emu_s = np.zeros((n, max(cap, 1)), sq.unit_dtype()), np.zeros((n, 8), np.int32)
    assert L.dagpu_square_units_emulate_host(k, n, _abi.addr(host), stride, pitch, k * k, _abi.addr(rec),
                                             _abi.addr(scan), cap, _abi.addr(emu_u), _abi.addr(emu_s)) == 0
    serial = []
    for i in range(n):
        u, s = np.zeros(max(cap, 1), sq.unit_dtype()), np.zeros(8, np.int32)
        code = L.dagpu_square_units_host(k, 1, host.ctypes.data + i * stride, stride, pitch, k * k, _abi.addr(rec[i]),
                                         _abi.addr(scan[i]), cap, _abi.addr(u), _abi.addr(s))
        serial.append((u, s) if code == 0 else None)
    return scan, serial, emu_u, emu_s


def units_of(L, k, squares):
    """The largest unit count among the squares, by the host executor."""
    host = np.concatenate([rc.ods_of(s) for s in squares])
    _, serial, _, _ = host_tables(L, k, host, len(squares), k * k * 512, k * 512, 0)
    return max(int(s[1]) if s[0] == OVERFLOW else int(s[2]) for _, s in (x for x in serial if x is not None))


def run_units(ctx, k, squares, in_place, cap=None, stream=None):
    """The device's tables of n squares against the host's.  Returns the device's summaries."""
    L, n = ctx._L, len(squares)
    if cap is None:
        cap = max(1, units_of(L, k, squares))
    buf, stride, pitch, host = place(k, squares, in_place)
    scan, serial, emu_u, emu_s = host_tables(L, k, host, n, stride, pitch, cap)
    records, summary, shost = scan_squares_device(k, buf, stride, pitch, ctx=ctx)
    assert (shost == scan).all()
    if stream is None:
        units, usum, uhost = unit_table_device(k, buf, stride, pitch, records, summary, cap, ctx=ctx)
        assert (usum.cpu().numpy() == uhost).all()
    else:  # enqueue only: a caller's workspace, no host summary
        ws = torch.empty((L.dagpu_square_units_workspace_size(k, n),), dtype=torch.uint8, device="cuda")
        stream.wait_stream(torch.cuda.current_stream())
        units, usum, none = unit_table_device(k, buf, stride, pitch, records, summary, cap, ctx=ctx, stream=stream,
                                              summary_host=False, workspace=ws)
        assert none is None
        stream.synchronize()
        uhost = usum.cpu().numpy()
    got = np.ascontiguousarray(units.cpu().numpy()).view(sq.unit_dtype()).reshape(n, cap)
    for i in range(n):
        # the emulation is the device's algorithm: the same summary, HOST verdicts and their share included
        assert uhost[i].tobytes() == emu_s[i].tobytes(), (i, uhost[i], emu_s[i])
        if uhost[i, 0] == HOST:
            continue
        # anything else is the host executor's answer, byte for byte
        u, s = serial[i]
        assert uhost[i].tobytes() == s.tobytes(), (i, uhost[i], s)
        m = min(int(s[2]), cap)
        assert got[i, :m].tobytes() == u[:m].tobytes(), i
    assert (buf.cpu().numpy() == host).all()
    return uhost


@pytest.fixture(scope="module")
def by_width():
    groups = collections.defaultdict(list)
    for _, k, s, _ in cases.squares():
        groups[k].append(s)
    return dict(groups)


@pytest.mark.parametrize("in_place", [False, True], ids=["packed", "q0_in_place"])
@pytest.mark.parametrize("k", [1, 2, 4, 8, 16, 32, 64])
def test_corpus_batched_by_width(ctx, by_width, k, in_place):
    squares = by_width[k]
    seen = 0
    for at in range(0, len(squares), 8):
        batch = [squares[(at + i) % len(squares)] for i in range(8)]
        uhost = run_units(ctx, k, batch, in_place)
        assert (uhost[:, 0] == OK).all()  # no square the splitters made goes to the host
        seen += int(uhost[:, 2].sum())
    assert seen > 0


@pytest.mark.parametrize("in_place", [False, True], ids=["packed", "q0_in_place"])
def test_hand_made_squares(ctx, in_place):
    squares = [s for _, _, s, _ in rc.hand_made()]
    uhost = run_units(ctx, 64, squares, in_place)
    assert list(uhost[:, 0]) == [OK, OK] and uhost[0, 2] == 0 and uhost[1, 3] > 63 and uhost[1, 4] >= 3


@pytest.mark.parametrize("in_place", [False, True], ids=["packed", "q0_in_place"])
def test_tampered_squares(ctx, in_place):
    table = cases.tampered()
    squares = [s for _, s, _ in table] + [cases.tamper_base(), rc.tampered()[0][1]]
    uhost = run_units(ctx, 4, squares, in_place)
    want = [HOST if must else OK for _, _, must in table] + [OK, _abi.UNITS_SCAN]
    assert list(uhost[:, 0]) == want


def test_table_too_small(ctx, by_width):
    squares = by_width[4][:8]
    counts = [units_of(ctx._L, 4, [s]) for s in squares]
    most = max(counts)
    assert most >= 2 and counts.count(most) == 1
    uhost = run_units(ctx, 4, squares, False, cap=most - 1)  # the first records are compared there
    for c, row in zip(counts, uhost):
        assert list(row[:3]) == ([OVERFLOW, most, most] if c == most else [OK, 0, c])


def test_enqueue_only_on_a_side_stream(ctx, by_width):
    batch = by_width[4][:8]
    uhost = run_units(ctx, 4, batch, True, stream=torch.cuda.Stream())
    assert (uhost[:, 0] == OK).all() and uhost[:, 2].sum() > 0


# ---- selected units ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def block8():
    """A k = 8 block: one-byte txs first and last, a 5,000-byte tx, three PFBs."""
    rng = np.random.default_rng(8)
    sizes = (1, 300, 5000, 130, 127, 300, 1)
    txs = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    txs += blob_txs([NS1, NS2, NS3], [[2000], [3000], [1000]])
    square = sq.construct(txs)
    assert square.size() == 8
    units = txs[:len(sizes)] + sh.parse_txs(rc.compact_range(list(square), sh.PAY_FOR_BLOB_NAMESPACE))
    assert len(units) == len(sizes) + 3
    return txs, units


def test_read_tx_units(ctx, block8):
    txs, want = block8
    d = DeviceSquares(8, 1, ctx=ctx)
    d.load_txs([txs])
    units, summary = d.tx_table()
    n = len(want)
    assert list(summary[0, :5]) == [OK, 0, n, n - 3, 3]
    assert d.tx_ranges() == [[(r.start, r.end) for r in (sq.tx_share_range(txs, i) for i in range(n))]]
    # one by one, all at once, and in another order
    assert [d.read_tx_units([(0, i)])[0] for i in range(n)] == want
    assert d.read_tx_units([(0, i) for i in range(n)]) == want
    assert d.read_tx_units([(0, n - 1), (0, 2), (0, 0), (0, 2)]) == [want[n - 1], want[2], want[0], want[2]]
    assert d.read_tx_units([]) == []
    with pytest.raises(DAError, match=f"txIndex {n} out of bounds"):
        d.read_tx_units([(0, 0), (0, n)])
    # the payload buffer keeps every byte outside [offset, offset + len)
    ix = d._tx_index
    records, where = ix["records"], ix["where"]
    selections = [list(range(n)), [2], [0], [n - 4], [n - 3], [n - 1], [n - 4, 0, n - 1, n - 3]]
    assert len(want[2]) == 5000 and len(want[0]) == 1 == len(want[n - 4])
    for sel in selections:
        need = sum(rc.up16(len(want[i])) for i in sel)
        payload = torch.full((need + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        offsets, totals, _ = read_units_device(8, where[0], where[1], where[2], records, ix["d_units"],
                                               ix["d_summary"], [(0, i) for i in sel], need, ctx=ctx, payload=payload)
        torch.cuda.synchronize()
        assert totals.cpu().tolist() == [len(sel), need, 0]
        got, at = payload.cpu().numpy(), 0
        for off, i in zip(offsets.cpu().tolist(), sel):
            assert off == at
            assert got[off:off + len(want[i])].tobytes() == want[i]
            at += rc.up16(len(want[i]))
            assert (got[off + len(want[i]):at] == SENTINEL).all()
        assert (got[at:] == SENTINEL).all()
    # a pair that names no unit yields length 0 and the flag; too small a buffer leaves the unit out
    payload = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
    offsets, totals, _ = read_units_device(8, where[0], where[1], where[2], records, ix["d_units"], ix["d_summary"],
                                           [(0, n), (1, 0), (0, 0), (0, 1)], 16, ctx=ctx, payload=payload)
    torch.cuda.synchronize()
    assert totals.cpu().tolist() == [4, 16 + rc.up16(300), _abi.READ_UNITS_INVALID | _abi.READ_UNITS_OVERFLOW]
    assert offsets.cpu().tolist() == [0, 0, 0, 16]
    got = payload.cpu().numpy()
    assert got[:1].tobytes() == want[0] and (got[1:] == SENTINEL).all()


# ---- tx inclusion proofs -----------------------------------------------------------------------

BLOCKS = {2: ("delimiter_straddles", "unit_ends_with_share", "blob_position_1", "txs_end_on_boundary_then_pfbs"),
          4: ("tx_5000", "blob_position_2", "pfb_many_blobs_shared_ns", None)}  # None: the tamper base's block


@pytest.mark.parametrize("k", [2, 4])
def test_tx_proofs(ctx, k):
    named = {name: (w, txs) for name, w, _, txs in cases.squares()}
    blocks = [list(cases.tamper_txs()) if name is None else list(named[name][1]) for name in BLOCKS[k]]
    assert all(name is None or named[name][0] == k for name in BLOCKS[k])
    d = DeviceSquares(k, 4, ctx=ctx, in_place=True)
    d.load_txs(blocks)
    d.extend()
    torch.cuda.synchronize()
    assert (d.status.cpu() == 0).all()
    units, summary = d.tx_table()
    assert [int(x) for x in summary[:, 2]] == [len(b) for b in blocks]
    assert summary[:, 3].sum() > 0 and summary[:, 4].sum() > 0
    pairs = [(i, t) for i, b in enumerate(blocks) for t in range(len(b))]
    got = d.tx_proofs(pairs)
    roots = [d.dah[i].cpu().numpy().tobytes() for i in range(4)]
    for (i, t), p in zip(pairs, got):
        want = proof.new_tx_inclusion_proof(blocks[i], t, ctx=ctx)
        assert p.data == want.data and p.share_proofs == want.share_proofs and p.row_proof == want.row_proof, (i, t)
        assert p.namespace_id == want.namespace_id and p.namespace_version == want.namespace_version
        assert p == want
        p.validate(roots[i])
    with pytest.raises(DAError, match=f"txIndex {len(blocks[1])} out of bounds") as e:
        d.tx_proofs([(0, 0), (1, len(blocks[1]))])
    assert e.value.code == _abi.ERR_ARG


def test_tx_table_answers_a_host_square_on_the_host(ctx):
    table = {name: s for name, s, _ in cases.tampered()}
    base = cases.tamper_base()
    squares = [base, table["reserved_cleared_where_a_unit_starts"], base,
               table["byte_in_the_padding_behind_the_last_unit"]]
    d = DeviceSquares(4, 4, ctx=ctx)
    d.load_ods(np.stack([rc.ods_of(s) for s in squares]))
    _, _, dev = unit_table_device(4, d.ods.view(-1), 16 * 512, 4 * 512, *scan_squares_device(
        4, d.ods.view(-1), 16 * 512, 4 * 512, ctx=ctx)[:2], 16, ctx=ctx)
    assert list(dev[:, 0]) == [OK, HOST, OK, HOST]
    units, summary = d.tx_table()
    for i, s in enumerate(squares):
        u, sm = sq.units_native(rc.ods_of(s), 4)
        assert summary[i].tobytes() == sm.tobytes() and sm[0] == OK
        assert units[i, :len(u)].tobytes() == u.tobytes() and not units[i, len(u):].tobytes().strip(b"\0")
    assert summary[3, 2] == summary[0, 2] + 1
    # the units of a square the host answered are cut from its download, the others gathered in HBM
    want = [cases.mirror_units(s)[1] for s in (base, base)]
    assert d.read_tx_units([(0, 1), (1, 2), (2, 0), (3, 5), (1, 0)]) == [
        want[0][1], want[0][2], want[0][0], rc.ods_of(squares[3])[4 * 512 + 34 + 202:][:5].tobytes(), want[0][0]]
    # a serial walk that fails raises the reference's message
    d.load_ods(np.stack([rc.ods_of(s) for s in (base, table["overflowing_varint_at_a_unit_start"], base, base)]))
    assert d._tx_index is None
    with pytest.raises(sq.ShareError, match="varint overflows a 64-bit integer"):
        d.tx_table()


def test_tx_table_sizes_its_table_again(ctx):
    """700 one-byte txs in 3 shares: far more units a share than the first table allows for."""
    name, k, shares, txs = next(c for c in cases.squares() if c[0] == "many_small_txs")
    d = DeviceSquares(k, 1, ctx=ctx)
    d.load_txs([list(txs)])
    units, summary = d.tx_table()
    u, sm = sq.units_native(rc.ods_of(shares), k)
    assert list(summary[0, :4]) == [OK, 0, 700, 700] and summary[0].tobytes() == sm.tobytes()
    assert units.shape == (1, 700) and units[0].tobytes() == u.tobytes()
    assert d.read_tx_units([(0, 699), (0, 237)]) == [txs[699], txs[237]]
