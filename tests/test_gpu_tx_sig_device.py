"""Tx signatures on the GPU (csrc/tx_sig.hip: dagpu_secp256k1_verify_device,
dagpu_tx_signers_device, dagpu_tx_sig_verify_device; device.secp256k1_verify_device,
tx_signers_device, verify_tx_signatures_device, DeviceSquares.verify_signatures)
against the host executors word for word and byte for byte, against the Python
mirror (blobtx.check_signature, signer_of_tx) and against the expected words of
the OpenSSL fixture, the edge set and the one-tx-per-kind block."""
import numpy as np
import pytest
import torch

from celestia_da import _abi, da, square as sq
from celestia_da.device import (DeviceSquares, plan_squares_device, secp256k1_verify_device, tx_signers_device,
                                verify_tx_signatures_device)

import tx_sig_cases as cases
from tx_sig_cases import K, word

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def _device_host_mirror(ctx, blocks, accts, table=None, chain_id=cases.CHAIN_ID, **kw):
    """The tx call on the device, the host executor and the mirror over the
    same batch: all equal.  Returns (tx_status, block_status, signers)."""
    p = plan_squares_device(blocks, ctx=ctx)
    out = verify_tx_signatures_device(p, chain_id, accts, pubkeys=table, ctx=ctx, **kw)
    only = tx_signers_device(p, ctx=ctx, stream=kw.get("stream"))
    torch.cuda.synchronize()
    got = tuple(_host(t) for t in out)
    want = cases.verify_host(blocks, accts, table, chain_id)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)
    mirror_tx, mirror_block = cases.mirror_words(blocks, accts, table, chain_id)
    assert np.array_equal(got[0], mirror_tx) and np.array_equal(got[1], mirror_block)
    assert np.array_equal(got[2], cases.mirror_signers(blocks)) and np.array_equal(_host(only), got[2])
    return got


def test_raw_call(ctx):
    """The fixture and the edge set: fewer than 256 items, one workgroup, part of it idle."""
    all_cases = cases.fixture_cases() + cases.edge_cases()
    digests, sigs, pubkeys = (torch.from_numpy(a).cuda() for a in cases.raw_arrays(all_cases))
    status = secp256k1_verify_device(digests, sigs, pubkeys, ctx=ctx)
    torch.cuda.synchronize()
    got = _host(status)
    assert np.array_equal(got, cases.raw_host(all_cases))
    for (name, *_, want), w in zip(all_cases, got.tolist()):
        assert w == K[want], (name, w)
    assert secp256k1_verify_device(digests[:0], sigs[:0], pubkeys[:0], ctx=ctx).numel() == 0
    with pytest.raises(ValueError, match="pubkeys"):
        secp256k1_verify_device(digests, sigs, pubkeys[:, :32].contiguous(), ctx=ctx)


def test_raw_call_across_workgroups(ctx):
    """600 items over three workgroups, the last partly filled; valid and
    invalid items alternate, so every wave holds both."""
    base = cases.fixture_cases() + cases.edge_cases()
    many = [base[i % len(base)] for i in range(600)]
    digests, sigs, pubkeys = (torch.from_numpy(a).cuda() for a in cases.raw_arrays(many))
    side = torch.cuda.Stream()
    status = secp256k1_verify_device(digests, sigs, pubkeys, ctx=ctx, stream=side)
    side.synchronize()
    assert _host(status).tolist() == [K[c[4]] for c in many]


def test_every_kind(ctx):
    names, txs, accts, table, words = cases.kind_block()
    tx_status, block_status, _ = _device_host_mirror(ctx, [txs], accts, table)
    assert tx_status.tolist() == words
    rejecting = [i for i, w in enumerate(words) if w & 0xFF >= _abi.SIG_REJECTING]
    assert block_status.tolist() == [[rejecting[0], words[rejecting[0]],
                                      sum(1 <= w & 0xFF < _abi.SIG_REJECTING for w in words), 0]]


def test_batch_of_four(ctx):
    """300 signed txs (the lanes cross a 256-lane workgroup), an empty block, 7
    txs, 5 txs; normal txs and BlobTxs mixed."""
    blocks, accts = cases.batch_of_four()
    tx_status, block_status, signers = _device_host_mirror(ctx, blocks, accts)
    assert tx_status.size == 312 and np.count_nonzero(tx_status) == 4
    assert block_status.tolist() == [[40, word("SIG_MISMATCH"), 0, 0], [0xFFFFFFFF, 0, 0, 0],
                                     [3, word("SIG_BAD_LENGTH", 40), 1, 0], [0xFFFFFFFF, 0, 0, 0]]
    assert signers[299, 33] == 0 and int(signers[299, 40:48].view(np.uint64)[0]) == 299


def test_table_keys(ctx):
    """The stored keys of every account as the table: the txs verify against
    them; one wrong row rejects its tx alone."""
    blocks, accts = cases.batch_of_four()
    blocks, accts = blocks[2:], accts[300:]
    table = cases.mirror_signers(blocks)[:, :33].copy()
    table[1] = np.frombuffer(cases.ec.pubkey_of(12345), np.uint8)
    tx_status, block_status, _ = _device_host_mirror(ctx, blocks, accts, table)
    assert tx_status[1] == word("SIG_MISMATCH") and block_status[0].tolist() == [1, word("SIG_MISMATCH"), 1, 0]


def test_long_tx(ctx):
    """One 70 KB tx among short ones: the streamed hash over more than a
    thousand SHA-256 blocks, one lane diverging."""
    blocks, accts = cases.long_tx_block()
    tx_status, block_status, _ = _device_host_mirror(ctx, blocks, accts)
    assert not tx_status.any() and block_status.tolist() == [[0xFFFFFFFF, 0, 0, 0]]
    wrong = accts.copy()
    wrong[2] += 1
    tx_status, _, _ = _device_host_mirror(ctx, blocks, wrong)
    assert tx_status.tolist() == [0, 0, word("SIG_MISMATCH"), 0, 0, 0]


def test_second_stream_and_workspace(ctx):
    blocks, accts = cases.batch_of_four()
    blocks, accts = blocks[1:], accts[300:]
    ntx = sum(len(b) for b in blocks)
    ws = torch.empty((ctx._L.dagpu_tx_sig_verify_workspace_size(len(blocks), ntx) + 64,), dtype=torch.uint8,
                     device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    a = _device_host_mirror(ctx, blocks, accts, stream=side, workspace=ws)
    b = _device_host_mirror(ctx, blocks, accts, chain_id=cases.CHAIN_ID + "2", stream=side, workspace=ws)
    assert a[1].tolist() == [[0xFFFFFFFF, 0, 0, 0], [3, word("SIG_BAD_LENGTH", 40), 1, 0], [0xFFFFFFFF, 0, 0, 0]]
    assert b[1].tolist() == [[0xFFFFFFFF, 0, 0, 0], [0, word("SIG_MISMATCH"), 1, 0], [0, word("SIG_MISMATCH"), 0, 0]]
    with pytest.raises(ValueError, match="workspace"):
        verify_tx_signatures_device(plan_squares_device(blocks, ctx=ctx), "c", accts, ctx=ctx, workspace=ws[:64])
    with pytest.raises(da.DAError, match="longer than 64"):
        verify_tx_signatures_device(plan_squares_device(blocks, ctx=ctx), "c" * 65, accts, ctx=ctx)
    with pytest.raises(ValueError, match="account_numbers"):
        verify_tx_signatures_device(plan_squares_device(blocks, ctx=ctx), "c", accts[:-1], ctx=ctx)


def test_refusals_enqueue_nothing(ctx):
    blocks, accts = cases.batch_of_four()
    blocks, accts = blocks[3:], accts[307:]
    p = plan_squares_device(blocks, ctx=ctx)
    L = ctx._L
    d_accts = torch.from_numpy(accts.view(np.int64).copy()).cuda()
    tx_status = torch.full((5,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    block_status = torch.full((1, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    signers = torch.full((5, 48), 0x5A, dtype=torch.uint8, device="cuda")
    ws = torch.empty((L.dagpu_tx_sig_verify_workspace_size(1, 5) + 16,), dtype=torch.uint8, device="cuda")
    chain = np.frombuffer(cases.CHAIN_ID.encode(), np.uint8).copy()

    def call(**over):
        a = dict(src=_abi.addr(p.src), offs=_abi.addr(p.src_offs), ntx=_abi.addr(p.ntx), lens=_abi.addr(p.tx_lens),
                 chain_len=chain.size, accts=_abi.addr(d_accts), tx_status=_abi.addr(tx_status),
                 block_status=_abi.addr(block_status), signers=_abi.addr(signers), ws=_abi.addr(ws))
        a.update(over)
        return L.dagpu_tx_sig_verify_device(ctx.handle, 1, a["src"], a["offs"], p.src_bytes, a["ntx"], a["lens"],
                                            _abi.addr(chain), a["chain_len"], a["accts"], None, a["tx_status"],
                                            a["block_status"], a["signers"], a["ws"], None)

    short = p.tx_lens.copy()
    short[0] -= 1
    for text, over in (("null", dict(tx_status=None)), ("null", dict(block_status=None)), ("null", dict(signers=None)),
                       ("null", dict(offs=None)), ("null", dict(ntx=None)), ("null d_src", dict(src=None)),
                       ("null d_account_numbers", dict(accts=None)), ("tx_lens is required", dict(lens=None)),
                       ("aligned", dict(ws=_abi.addr(ws) + 8)), ("aligned", dict(tx_status=_abi.addr(tx_status) + 2)),
                       ("aligned", dict(signers=_abi.addr(signers) + 4)), ("aligned", dict(accts=_abi.addr(d_accts) + 4)),
                       ("longer than 64", dict(chain_len=65)), ("add up", dict(lens=_abi.addr(short)))):
        assert call(**over) == _abi.ERR_ARG, (text, over)
        assert text in ctx.last_error(), (text, ctx.last_error())
    assert L.dagpu_tx_sig_verify_device(None, 1, *([None] * 2), 0, *([None] * 3), 0, *([None] * 7)) == _abi.ERR_ARG
    torch.cuda.synchronize()
    assert (tx_status == 0x5A5A5A5A).all() and (block_status == 0x5A5A5A5A).all() and (signers == 0x5A).all()
    # the accepted call writes all of them, with the caller's workspace and with the library's
    want = cases.verify_host(blocks, accts)
    for over in ({}, dict(ws=None)):
        tx_status.fill_(0x5A5A5A5A), block_status.fill_(0x5A5A5A5A), signers.fill_(0x5A)
        assert call(**over) == 0, ctx.last_error()
        torch.cuda.synchronize()
        for g, w in zip((tx_status, block_status, signers), want):
            assert np.array_equal(_host(g), w)


def test_after_process_blocks(ctx):
    """DeviceSquares.verify_signatures over the batch process_blocks left
    resident; process_blocks' own outputs stay as they were."""
    blocks, accts = cases.batch_of_four()
    k = sq.plan_native(blocks[0])[0]
    d = DeviceSquares(k, 4, ctx=ctx)
    with pytest.raises(ValueError, match="not resident"):
        d.verify_signatures(cases.CHAIN_ID, accts)
    verdicts = d.process_blocks(blocks)
    torch.cuda.synchronize()
    records = d.verdicts.copy()
    check_words = _host(d.proposal_check.tx_status).copy()
    dah, eds = d.dah.clone(), d.eds.clone()
    assert verdicts[0] == (True, ""), verdicts
    tx_status, block_status, signers = d.verify_signatures(cases.CHAIN_ID, accts)
    torch.cuda.synchronize()
    want = cases.verify_host(blocks, accts)
    for g, w in zip((tx_status, block_status, signers), want):
        assert np.array_equal(_host(g), w)
    assert _host(block_status)[0].tolist() == [40, word("SIG_MISMATCH"), 0, 0]
    assert np.array_equal(d.verdicts, records) and np.array_equal(_host(d.proposal_check.tx_status), check_words)
    assert torch.equal(d.dah, dah) and torch.equal(d.eds, eds)
    assert d.process_blocks(blocks) == verdicts and np.array_equal(d.verdicts, records)
    # load_txs(plan="device") leaves the same batch resident
    d2 = DeviceSquares(k, 1, ctx=ctx)
    d2.load_txs(blocks[:1], plan="device")
    got = d2.verify_signatures(cases.CHAIN_ID, accts[:300])
    torch.cuda.synchronize()
    assert np.array_equal(_host(got[0]), want[0][:300])
