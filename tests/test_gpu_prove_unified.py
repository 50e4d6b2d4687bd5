"""The two paths that the single-square and the across-squares proof producers
share as one set of kernels (nmt_prove.hip): a single-square call whose column
and cell bases are null, and a batch proof store of one square.  The helpers
and the specifications are those of test_gpu_nmt_prove_batch.py and
test_gpu_share_proofs.py."""
import ctypes

import numpy as np
import pytest
import torch

from celestia_da import _abi, da, device
from test_gpu_nmt_prove_batch import Square
from test_gpu_share_proofs import Batch, _check_against_single_square

pytestmark = pytest.mark.gpu

OK = _abi.OK


@pytest.fixture(scope="module")
def ctx():
    c = da.Context(0)
    yield c
    c.close()


def test_rows_alone_without_columns_and_square(ctx):
    """Row requests with neither the column nodes nor the square (both null),
    namespaces wanted: nodes, namespaces and descriptors of the full call."""
    k = 2
    s = Square(ctx, k, 4100 + k)
    w = s.w
    reqs = [(0, 0, 0, 1), (0, w - 1, w - 1, w), (0, 1, 0, w), (0, 2, 1, 3), (0, w - 1, 0, 1), (0, 0, w - 1, w)]
    nodes, ns, _, desc = device.nmt_prove_batch_device(s.nodes, reqs, eds=s.nodes.eds, ctx=ctx)
    assert nodes.cpu().numpy().tobytes() == b"".join(n for r in reqs for n in s.range_proof(*r))
    dev = nodes.device
    req = np.array(reqs, np.int64)
    out_nodes = torch.full((nodes.numel() + 90,), 0xA5, dtype=torch.uint8, device=dev)
    out_ns = torch.full((29 * len(reqs),), 0xA5, dtype=torch.uint8, device=dev)
    d2 = np.zeros((len(reqs), 8), np.int64)
    total = ctypes.c_size_t(0)
    L = ctx._L
    ws = torch.empty(L.dagpu_nmt_prove_workspace_size(len(reqs)), dtype=torch.uint8, device=dev)
    rc = L.dagpu_nmt_prove_batch_device(
        ctx.handle, k, len(reqs), req.ctypes.data, None, s.nodes.nodes.data_ptr(), None, out_nodes.data_ptr(),
        nodes.numel() // 90, out_ns.data_ptr(), None, 0, d2.ctypes.data, ctypes.byref(total), ws.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == OK and 90 * total.value == nodes.numel() > 0
    assert torch.equal(out_nodes[:nodes.numel()], nodes) and bool((out_nodes[nodes.numel():] == 0xA5).all())
    assert torch.equal(out_ns, ns) and (d2 == desc).all()


def test_producer_on_a_batch_of_one(ctx):
    """n_sq = 1: the store of one square gives what the single-square call
    gives on that square's exports, rows and columns."""
    k = 2
    b = Batch(ctx, k, [7400 + k])
    w = b.w
    reqs = [(0, axis, index, s, e) for axis in (0, 1) for index in (0, w - 1)
            for s, e in ((0, 1), (w - 1, w), (0, w), (1, 3))]
    out = device.nmt_prove_squares_device(b.store, reqs)
    _check_against_single_square(b, reqs, out)
    ref = device.nmt_prove_batch_device(b.ref[0], [r[1:] for r in reqs], eds=b.ref[0].eds)
    torch.cuda.synchronize()
    assert torch.equal(out.nodes, ref[0]) and torch.equal(out.namespaces, ref[1]) and torch.equal(out.shares, ref[2])
    assert out.nodes.numel() > 0 and (out.desc[:, :6] == ref[3][:, :6]).all()
