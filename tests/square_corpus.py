"""Blocks of txs shared by tests/test_square_plan.py (host) and
tests/test_gpu_square_device.py (GPU): every shape at which the share writer
of csrc/square_write.hpp takes another path.  Built from the helpers of
test_square_host.py; each entry is (name, txs, max_square_size).  An entry may
be a block that square.Construct rejects (some BLOB_POSITION_CASES, some random
seeds): the tests then compare the error instead of the square."""
import functools
import random

from celestia_da import blobtx as bt
from celestia_da import shares as sh

from test_square_host import BLOB_POSITION_CASES, NS1, NS2, NS3, blob_txs, normal_txs, pfb_tx, random_blob_txs

SINGLE_TX_SIZES = (1, 473, 474, 475, 477, 478, 479, 952, 953, 956, 957, 5000)
BLOB_SIZES = (1, 477, 478, 479, 478 + 482, 478 + 482 + 1)
RANDOM_SEEDS = tuple(range(12))


def random_block(seed):
    """The block of test_square_native.test_random_blocks for this seed."""
    rng = random.Random(seed)
    n_normal = rng.randrange(0, 200)
    txs = [rng.randbytes(rng.choice([1, 50, 300, 477, 1000, 3000])) for _ in range(n_normal)]
    nss = [sh.new_namespace_v0(bytes([rng.randrange(1, 6)]) * 10) for _ in range(8)]
    for _ in range(rng.randrange(0, 80)):
        blobs = [sh.Blob.new(rng.choice(nss), rng.randbytes(rng.choice([1, 477, 478, 479, 960, 2000, 20000])))
                 for _ in range(rng.randrange(1, 4))]
        txs.append(bt.marshal_blob_tx(pfb_tx([len(b.data) for b in blobs]), *blobs))
    return txs


def two_wide_blobs():
    """Two blobs of more than 64 shares each (subtree width 2).  One normal tx
    (1 share) and two 330-B PFBs (2 shares) end at share 3, so the first blob
    starts at 4 behind one reserved padding share; it has 71 shares, so the
    second starts at 76 behind one padding share in the first's namespace."""
    rng = random.Random(42)
    first = sh.available_bytes_from_sparse_shares(71)
    second = sh.available_bytes_from_sparse_shares(90) - 7
    return normal_txs(rng, 1) + blob_txs([NS1, NS2], [[first], [second]], rng)


def full_block():
    """2,000 normal + 2,000 blob txs, k = 128: the input of
    test_gpu_square.test_native_construct_to_dah."""
    rng = random.Random(7)
    return normal_txs(rng, 2000, 300) + random_blob_txs(rng, 2000, 3000)


@functools.lru_cache(maxsize=None)
def corpus():
    rng = random.Random(2025)
    out = [("empty", [], 128), ("tiny", [b"\x01"], 128), ("zero_length_tx", [b"", b"\x07", b""], 128)]
    for n in SINGLE_TX_SIZES:
        out.append((f"tx_{n}", [rng.randbytes(n)], 128))
    # a tx of 128 B or more has a 2-byte delimiter.  Units of 473 and 478 stream
    # bytes put the next delimiters at 473|474 and 951|952: across the end of the
    # first (474 B of content) and of the second (478 B) share
    out.append(("delimiter_straddles", [rng.randbytes(n) for n in (471, 476, 300)], 128))
    # units of 474 and 478 stream bytes end at the last byte of shares 0 and 1
    out.append(("unit_ends_with_share", [rng.randbytes(n) for n in (472, 476, 100)], 128))
    # one-byte txs: 237 units in a share, a segment seam in every 8-byte word
    out.append(("many_small_txs", [rng.randbytes(1) for _ in range(700)], 128))
    for i, (size, nss, sizes, _) in enumerate(BLOB_POSITION_CASES):
        out.append((f"blob_position_{i}", blob_txs(nss, sizes), size))
    for n in BLOB_SIZES:
        out.append((f"blob_{n}", blob_txs([NS2], [[n]], rng), 128))
    out.append(("two_wide_blobs", two_wide_blobs(), 128))
    out.append(("pfb_many_blobs_shared_ns", blob_txs([NS2, NS1, NS1, NS3, NS1], [[100, 900, 300, 2000], [500]], rng),
                128))
    for seed in RANDOM_SEEDS:
        out.append((f"random_{seed}", random_block(seed), 128))
    return tuple(out)
