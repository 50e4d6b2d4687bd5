"""The NMT leaf and level kernels on the index maps of csrc/nmt_coords.hpp,
against the CPU oracle, at the shapes where the maps change form: squares and
levels with fewer lanes of work than a 256-lane workgroup (several squares
share one: k = 1, 2, 4 and the top levels of every k), levels that span several
workgroups (k = 16, 64), and squares other than the first (n = 3).  Every row
root, column root, DAH and status word is compared, bit-exact."""
import numpy as np
import pytest
import torch

import oracle
from celestia_da import da, synth
from celestia_da.device import DeviceSquares

pytestmark = pytest.mark.gpu

PUSH_ORDER = 1  # dagpu_extend_batch_device's status bit


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


_ORACLE = {}


def reference(k, seed):
    """(ods, row roots, column roots, dah) of a seeded square, computed once."""
    if (k, seed) not in _ORACLE:
        ods = synth.random_blob_square(k, seed)
        _, rr, cr, dah = oracle.extend_and_dah(ods, k, nthreads=8)
        _ORACLE[(k, seed)] = (ods, rr, cr, dah)
    return _ORACLE[(k, seed)]


def extend(ctx, k, squares):
    ds = DeviceSquares(k, len(squares), ctx=ctx)
    ds.status.fill_(-1)  # the call itself must clear every word
    ds.load_ods(np.stack([s.reshape(-1) for s in squares]))
    ds.extend()
    torch.cuda.synchronize()
    return (ds.row_roots.cpu().numpy(), ds.col_roots.cpu().numpy(), ds.dah.cpu().numpy(),
            ds.status.cpu().numpy())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("k", [1, 2, 4, 8, 16, 64])
def test_roots_dah_status_match_oracle(ctx, k, n):
    refs = [reference(k, 1300 + 7 * k + i) for i in range(n)]
    rr, cr, dah, status = extend(ctx, k, [r[0] for r in refs])
    assert (status == 0).all(), status
    for i, (_, orr, ocr, odah) in enumerate(refs):
        assert (rr[i] == orr).all(), (k, i)
        assert (cr[i] == ocr).all(), (k, i)
        assert dah[i].tobytes() == odah, (k, i)


def test_push_order_in_the_middle_square_only(ctx):
    k = 8
    refs = [reference(k, 1300 + 7 * k + i) for i in range(3)]
    bad = refs[1][0].copy()
    bad[[0, 1]] = bad[[1, 0]]  # the first two shares of row 0, out of namespace order
    with pytest.raises(oracle.OracleError):
        oracle.extend_and_dah(bad, k)
    rr, cr, dah, status = extend(ctx, k, [refs[0][0], bad, refs[2][0]])
    assert list(status) == [0, PUSH_ORDER, 0]
    for i in (0, 2):
        _, orr, ocr, odah = refs[i]
        assert (rr[i] == orr).all() and (cr[i] == ocr).all() and dah[i].tobytes() == odah
