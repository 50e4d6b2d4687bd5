"""da.process_proposal, the readable mirror of the data-parallel part of
ProcessProposal for one block, on the cases of tests/blobtx_validate_cases.py:
every kind, the flipped commitment, a wrong data hash, a wrong square size and
an undecodable normal tx.  The commitment and the data root come from the CPU
oracle here (pyref.create_commitment, oracle.extend_and_dah), so that no device
is needed."""
import random

import numpy as np
import pytest

import oracle
import pyref
from celestia_da import _abi, blobtx as bt, da, square as sq

import blobtx_validate_cases as cases
from process_blocks_cases import flip_commitment

CODE = {name: i for i, name in enumerate(_abi.VERDICT_NAMES)}
NONE = _abi.BLOBTX_NONE


def data_root(shares):
    k = sq.size(len(shares))
    return oracle.extend_and_dah(np.frombuffer(b"".join(shares), np.uint8).reshape(k * k, 512), k)[3]


def mirror(txs, **kw):
    return da.process_proposal(txs, create_commitment=pyref.create_commitment, data_root=data_root, **kw)


def _block(rng, ntx=6):
    return [cases.normal_tx(rng), cases.normal_tx(rng)] + [cases.valid_tx(rng, 2, sizes=(300, 700)) for _ in range(ntx)]


def test_accept_and_the_later_steps():
    rng = random.Random(21)
    block = _block(rng)
    k = sq.construct(block).size()
    root = data_root(sq.construct(block).square_bytes())
    assert mirror(block) == (True, "", (CODE["ACCEPT"], NONE, 0, 0))
    assert mirror(block, data_hash=root, square_size=k) == (True, "", (CODE["ACCEPT"], NONE, 0, 0))
    wrong = root[:31] + bytes([root[31] ^ 1])
    assert mirror(block, data_hash=wrong, square_size=k) == \
        (False, "proposed data root differs from calculated data root", (CODE["DATA_ROOT_DIFFERS"], NONE, 0, 0))
    # the square size is compared before the data root
    assert mirror(block, data_hash=wrong, square_size=2 * k) == \
        (False, "proposed square size differs from calculated square size", (CODE["SQUARE_SIZE_DIFFERS"], NONE, 0, k))
    assert mirror([])[0] and mirror([], square_size=1)[0]


@pytest.mark.parametrize("kind", [k for k in bt.KIND_NAMES if k != "OK"])
def test_every_kind(kind):
    rng = random.Random(22)
    raw, index = cases.kind_cases()[kind]
    block = _block(rng)
    at = 1 if kind == "NON_BLOB_TX_HAS_PFB" else 5
    block[at] = raw
    word = cases.word(kind, index)
    if kind == "NON_BLOB_TX_HAS_PFB":
        want = (False, f"tx {at} has PFB but is not a blob tx", (CODE["NON_BLOB_TX_HAS_PFB"], at, word, 0))
    else:
        want = (False, f"invalid blob tx {at}: {bt.error_name(cases.K[kind])}", (CODE["INVALID_BLOB_TX"], at, word, 0))
    assert mirror(block, square_size=1) == want  # the tx loop comes before the square size


def test_flipped_commitment_and_the_lowest_tx():
    rng = random.Random(23)
    block = _block(rng, 12)
    block[9] = flip_commitment(block[9])
    want9 = (False, "invalid blob tx 9: ErrInvalidShareCommitment", (CODE["INVALID_SHARE_COMMITMENT"], 9, 0, 1))
    assert mirror(block) == want9
    # a stateless failure at tx 12 does not hide the mismatch at tx 9 ...
    signer = cases.kind_cases()["BAD_SIGNER"][0]
    later = list(block)
    later[12] = signer
    assert mirror(later) == want9
    # ... one at tx 7 comes first, and a tx that fails both ways reports the stateless rule
    earlier = list(block)
    earlier[7] = signer
    assert mirror(earlier)[2] == (CODE["INVALID_BLOB_TX"], 7, cases.word("BAD_SIGNER"), 0)
    t, _ = bt.unmarshal_blob_tx(block[9])
    p = bt.pfb_of_tx(t.tx)
    p.signer = "s"
    both = list(block)
    both[9] = cases.blob_tx(t.blobs, p)
    assert mirror(both)[2] == (CODE["INVALID_BLOB_TX"], 9, cases.word("BAD_SIGNER"), 0)
    # a create_commitment that fails is ErrCalculateCommitment of that blob
    def failing(ns, data):
        raise ValueError("push order")
    assert da.process_proposal(block[:4], create_commitment=failing)[1:] == \
        ("invalid blob tx 2: ErrCalculateCommitment", (CODE["CALCULATE_COMMITMENT"], 2, 0, 0))


def test_undecodable_normal_tx_is_skipped():
    rng = random.Random(24)
    block = [b"\x0a\x05abc", b"\xff\xff\xff"] + _block(rng)[2:]
    assert bt.check_tx(block[0]) == (0, 0) and bt.check_tx(block[1]) == (0, 0)
    assert mirror(block) == (True, "", (CODE["ACCEPT"], NONE, 0, 0))


def test_construct_failure_follows_the_tx_loop():
    rng = random.Random(25)
    # a normal tx behind a blob tx: square.Construct refuses the block
    block = [cases.valid_tx(rng, 1), cases.normal_tx(rng)]
    assert mirror(block, square_size=1) == \
        (False, "failure to compute data square from transactions:", (CODE["CONSTRUCT_FAILED"], NONE, 0, 0))
    block[0] = flip_commitment(block[0], 0)
    assert mirror(block)[2] == (CODE["INVALID_SHARE_COMMITMENT"], 0, 0, 0)
