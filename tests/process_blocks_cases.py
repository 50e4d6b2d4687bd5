"""Helpers and blocks shared by test_commit_plan_host.py and
test_gpu_process_blocks.py: commit_layout's image restated in Python,
dagpu_commit_plan_host as a function, blocks whose squares have width 16 with
blobs of chosen share counts, and the comparison of the counted commitment
route with check_commitments that the GPU test also runs in a child process
on the test build of the library."""
import random

import numpy as np

import pyref
from celestia_da import _abi, blobtx as bt, shares as sh, square as sq, trees

import blobtx_validate_cases as cases


def python_layout(records, k, n, threshold=64):
    """commit_layout's image in Python from (nblobs, 3) {square, first_share,
    share_count} records: (words, counts, blob_base)."""
    blob, share_pre, sub_pre, sub, work, most = [], [0], [0], [], [], 0
    per_block = [0] * n
    for b, (square, first, count) in enumerate(np.asarray(records).reshape(-1, 3).tolist()):
        per_block[square] += 1
        blob += [square, first]
        sizes = trees.merkle_mountain_range_sizes(count, trees.subtree_width(count, threshold))
        leaf = share_pre[-1]
        for s in sizes:
            if s >= 2:
                work.append(len(sub) // 3)
            sub += [b, leaf, s]
            leaf += s
        share_pre.append(leaf)
        sub_pre.append(sub_pre[-1] + len(sizes))
        most = max(most, len(sizes))
    words = np.array(blob + share_pre + sub_pre + sub + work, np.uint32)
    counts = np.array([len(share_pre) - 1, share_pre[-1], sub_pre[-1], len(work), most, 0, 0, 0], np.uint32)
    return words, counts, np.concatenate([[0], np.cumsum(per_block)]).astype(np.uint64)


def plan_host(k, n, arena, rec, threshold=64):
    """dagpu_commit_plan_host: (tables, counts, blob_base)."""
    L = _abi.lib()
    tables = np.full(L.dagpu_commit_plan_table_words(k, n), 0xA5A5A5A5, np.uint32)
    counts = np.full(8, 0xA5A5A5A5, np.uint32)
    base = np.full(n + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    rc = L.dagpu_commit_plan_host(k, n, _abi.addr(arena), arena.size, _abi.addr(rec), threshold, _abi.addr(tables),
                                  _abi.addr(counts), _abi.addr(base))
    assert rc == 0, L.dagpu_last_error(None).decode()
    return tables, counts, base


def blob_bytes(shares: int) -> int:
    """A data length that fills exactly `shares` sparse shares."""
    return 400 if shares == 1 else 478 + (shares - 2) * 482 + 100


def sized_tx(rng, share_counts, first_ns=0) -> bytes:
    """A valid BlobTx with one blob per entry of share_counts, namespaces ascending."""
    blobs = [sh.Blob.new(cases.NS[(first_ns + i) % len(cases.NS)], rng.randbytes(blob_bytes(c)))
             for i, c in enumerate(share_counts)]
    return cases.blob_tx(blobs, cases.pfb_of(blobs))


def k16_block(rng, ntx=24):
    """Valid blob txs whose square has width 16: two normal txs, then ntx txs of two 3-share blobs."""
    return [cases.normal_tx(rng), cases.normal_tx(rng)] + \
           [cases.valid_tx(rng, 2, sizes=(1000, 1400)) for _ in range(ntx)]


def flip_commitment(raw, blob=1):
    """The BlobTx with one bit of its blob-th declared commitment flipped."""
    t, _ = bt.unmarshal_blob_tx(raw)
    p = bt.pfb_of_tx(t.tx)
    good = p.share_commitments[blob]
    p.share_commitments[blob] = good[:7] + bytes([good[7] ^ 0x10]) + good[8:]
    return cases.blob_tx(t.blobs, p)


def bad_signer(raw):
    """The BlobTx with a signer whose checksum fails: an invalid blob tx the planner has no quarrel with."""
    t, _ = bt.unmarshal_blob_tx(raw)
    p = bt.pfb_of_tx(t.tx)
    p.signer = p.signer[:-1] + ("q" if p.signer[-1] != "q" else "p")
    return cases.blob_tx(t.blobs, p)


def commitment(ns, data):
    """pyref.create_commitment, through the cache the cases fill while they build their PFBs."""
    key = (bytes(ns), bytes(data))
    if key not in cases._commitments:
        cases._commitments[key] = pyref.create_commitment(bytes(ns), bytes(data))
    return cases._commitments[key]


def counted_blocks():
    """Four blocks of width 16 for the counted commitment route: blobs of 65
    and 129 shares (subtrees of 2 and 4 leaves: work items), of 64 shares and
    less (one-leaf subtrees), a flipped commitment at tx 9 and a bad signer."""
    rng = random.Random(31)
    blocks = [k16_block(rng), [cases.normal_tx(rng), sized_tx(rng, (1, 2, 64, 65)), sized_tx(rng, (2, 1), 4)],
              [sized_tx(rng, (129, 1)), sized_tx(rng, (65,), 3)], k16_block(rng)]
    blocks[0][9] = flip_commitment(blocks[0][9])
    blocks[3][7] = bad_signer(blocks[3][7])
    assert [sq.plan_native(b)[0] for b in blocks] == [16] * 4
    return blocks


def counted_route_report(ctx):
    """check_commitments(expected="declared") against proposal_check_device on
    counted_blocks(): a line "SAME nblobs nwork mismatches" when every output
    is equal bit for bit, else what differs."""
    import torch

    from celestia_da.device import DeviceSquares, proposal_check_device
    blocks = counted_blocks()
    d = DeviceSquares(16, len(blocks), ctx=ctx)
    d.load_txs(blocks, plan="device")
    com, st, sqs = d.check_commitments(expected="declared")
    expected = d._validated[2]
    check = proposal_check_device(d._planned, 16, d.ods.view(-1), 16 * 16 * 512, 16 * 512, ctx=ctx)
    torch.cuda.synchronize()
    nb = int(com.shape[0])
    counts = check.counts.cpu().numpy().view(np.uint32)
    if int(counts[0]) != nb or int(check.blob_base[-1]) != nb:
        return f"DIFFER counts {counts.tolist()} against {nb} blobs"
    for name, got, want in (("commitments", check.commitments[:nb], com), ("blob status", check.blob_status[:nb], st),
                            ("square status", check.square_status, sqs), ("expected", check.expected[:nb], expected),
                            ("blob status past the rows", check.blob_status[nb:].any(), torch.tensor(False).cuda())):
        if not torch.equal(got, want):
            return f"DIFFER {name}"
    return f"SAME {nb} {int(counts[3])} {int((st != 0).sum())}"


def child_main():
    from celestia_da import da
    ctx = da.Context(0)
    print(counted_route_report(ctx))
    ctx.close()
