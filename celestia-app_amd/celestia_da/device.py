"""Device-resident batched pipeline (block replay / sync batches).

PyTorch is used only as the device allocator and stream provider; the work is
the HIP kernels behind dagpu_extend_batch_device (include/dagpu.h).  Inputs are
already resident in HBM and only the roots/DAH (or nothing) come back.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import _abi
from .da import Context, DAError, default_context

ROOT = _abi.ROOT_SIZE


def _stream_handle(stream: Optional[torch.cuda.Stream]) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def nmt_verify_batch_device(desc, namespaces: torch.Tensor, leaves: torch.Tensor, leaf_len: int,
                            nodes: torch.Tensor, roots: torch.Tensor, ctx: Optional[Context] = None,
                            stream: Optional[torch.cuda.Stream] = None,
                            workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dagpu_nmt_verify_batch_device: many nmt inclusion proofs against data
    already in HBM; returns the (n,) int32 status tensor on the device (0 or
    ERR_PROOF per proof), enqueued on `stream` (no sync of the results).

    desc: (n, 8) int64 on the HOST (proof.PackedNMT.desc); namespaces (29 B
    each), leaves (leaf_len bytes each), nodes and roots (90 B each): uint8
    tensors on one device.  With leaf_len == 512 `leaves` may be an extended
    square itself (cell (r, c) = leaf r * 2k + c)."""
    import numpy as np
    c = ctx or default_context()
    d = np.ascontiguousarray(np.asarray(desc, dtype=np.int64).reshape(-1, 8))
    n = int(d.shape[0])
    dev = leaves.device
    for t in (namespaces, leaves, nodes, roots):
        if t.dtype != torch.uint8 or t.device != dev or not t.is_contiguous():
            raise ValueError("namespaces, leaves, nodes and roots must be contiguous uint8 tensors on one device")
    n_leaves = leaves.numel() // leaf_len if leaf_len else int(d[:, 2].clip(min=0).sum())
    n_proven = int(d[:, 2].clip(min=0, max=max(n_leaves, 0)).sum())
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        status = torch.empty((n,), dtype=torch.int32, device=dev)
        if workspace is None:
            workspace = torch.empty((c._L.dagpu_nmt_verify_workspace_size(n, n_proven),), dtype=torch.uint8,
                                    device=dev)
    if workspace.numel() < c._L.dagpu_nmt_verify_workspace_size(n, n_proven):
        raise ValueError("workspace smaller than dagpu_nmt_verify_workspace_size")
    rc = c._L.dagpu_nmt_verify_batch_device(
        c.handle, n, _abi.addr(d), _abi.addr(namespaces), namespaces.numel() // 29, _abi.addr(leaves), n_leaves,
        leaf_len, _abi.addr(nodes), nodes.numel() // ROOT, _abi.addr(roots), roots.numel() // ROOT,
        _abi.addr(status), _abi.addr(workspace), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return status


def nmt_prove_batch_device(nodes, requests, eds: Optional[torch.Tensor] = None, ctx: Optional[Context] = None,
                           stream: Optional[torch.cuda.Stream] = None,
                           workspace: Optional[torch.Tensor] = None):
    """dagpu_nmt_prove_batch_device: nmt ProveRange for many (axis, index,
    start, end) requests on the row (axis 0) and column (axis 1) trees of one
    resident square, enqueued on `stream` (no sync of the results).

    nodes: inclusion.EDSAxisNodes; requests: (n, 4) int64-like on the HOST.
    With `eds` (the square on the device, e.g. nodes.eds) the proven cells are
    gathered too.  Returns (proof_nodes, namespaces, shares, desc): uint8 device
    tensors of 90 B per node, 29 B per proof and 512 B per proven cell (None
    without `eds`), and the (n, 8) int64 HOST descriptors in the layout
    nmt_verify_batch_device takes, for a roots table cat(row_roots, col_roots).
    namespaces[i] is the namespace of the range's first leaf: a range over
    several namespaces gets a correct proof that no single namespace verifies
    (proof.parse_namespace rejects such ranges)."""
    import ctypes

    import numpy as np
    c = ctx or nodes.ctx
    req = np.ascontiguousarray(np.asarray(requests, dtype=np.int64).reshape(-1, _abi.PROVE_REQ_WORDS))
    n = int(req.shape[0])
    w, dev = nodes.w, nodes.nodes.device
    if eds is not None and (eds.dtype != torch.uint8 or eds.device != dev or not eds.is_contiguous()
                            or eds.numel() != w * w * 512):
        raise ValueError("eds must be the contiguous (2k)^2 x 512 uint8 square on the nodes' device")
    # capacities from the requests as given; the library validates them
    m = w.bit_length() - 1
    start, last = req[:, 2].clip(0, w), (req[:, 3] - 1).clip(0, w - 1)

    def popcount(v):
        return np.unpackbits(v.astype(">u4").view(np.uint8)).reshape(len(v), 32).sum(axis=1)

    # popcount(start) + log2(2k) - popcount(end - 1) nodes per proof
    nodes_cap = int((popcount(start) + m - popcount(last)).sum()) if n else 0
    shares_cap = int((req[:, 3] - req[:, 2]).clip(0, w).sum()) if eds is not None else 0
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        out_nodes = torch.empty((nodes_cap * ROOT,), dtype=torch.uint8, device=dev)
        out_ns = torch.empty((n * 29,), dtype=torch.uint8, device=dev)
        out_shares = torch.empty((shares_cap * 512,), dtype=torch.uint8, device=dev) if eds is not None else None
        if workspace is None:
            workspace = torch.empty((c._L.dagpu_nmt_prove_workspace_size(n),), dtype=torch.uint8, device=dev)
    if workspace.numel() < c._L.dagpu_nmt_prove_workspace_size(n):
        raise ValueError("workspace smaller than dagpu_nmt_prove_workspace_size")
    desc = np.zeros((n, _abi.NMT_DESC_WORDS), np.int64)
    total = ctypes.c_size_t(0)
    rc = c._L.dagpu_nmt_prove_batch_device(
        c.handle, nodes.k, n, _abi.addr(req), _abi.addr(eds), _abi.addr(nodes.nodes), _abi.addr(nodes.col_inner),
        _abi.addr(out_nodes), nodes_cap, _abi.addr(out_ns), _abi.addr(out_shares), shares_cap, _abi.addr(desc),
        ctypes.byref(total), _abi.addr(workspace), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return out_nodes[:total.value * ROOT], out_ns, out_shares, desc


class StoreSquare:
    """One square of a ProofStore with the attributes of an
    inclusion.EDSAxisNodes (ctx, k, w, eds, nodes, col_inner, col_roots()), all
    views into the store and the batch: what nmt_prove_batch_device,
    proof.prove_ranges, proof.prove_namespaces and nmt_namespace_ranges_device
    take in its place.  Nothing is hashed."""

    def __init__(self, store: "ProofStore", i: int):
        self.ctx, self.k, self.w = store.ctx, store.k, store.w
        self.eds = store.eds[i * store.square_stride:i * store.square_stride + store.w * store.w * 512]
        self.nodes = store.store[i * store.row_bytes:(i + 1) * store.row_bytes]
        self.col_inner = store.store[store.col_off + i * store.col_bytes:store.col_off + (i + 1) * store.col_bytes]

    def col_roots(self) -> torch.Tensor:
        """(2k, 96) view of the column roots: the top level of the column store."""
        return self.col_inner.view(-1, 96)[-self.w:]


class ProofStore:
    """dagpu_proof_store_device: every row-tree and column-tree node and the
    DAH tree of ALL squares of a batch in one device buffer, built by a number
    of launches that does not depend on the batch (enqueued on `stream`, no
    sync).  eds_batch: a contiguous cuda uint8 tensor holding the extended
    squares, square i at byte i * square_stride (default: back to back).

    store:  the buffer; square i's row / column slices are byte for byte the
            stores of inclusion.EDSAxisNodes (see square(i))
    n, k, w, row_bytes, col_bytes, dah_bytes, col_off, dah_off: its layout"""

    def __init__(self, k: int, eds_batch: torch.Tensor, square_stride: Optional[int] = None,
                 ctx: Optional[Context] = None, stream: Optional[torch.cuda.Stream] = None):
        import ctypes
        self.ctx = ctx or default_context()
        self.k, self.w = int(k), 2 * int(k)
        one = self.w * self.w * 512
        if not isinstance(eds_batch, torch.Tensor) or not eds_batch.is_cuda or eds_batch.dtype != torch.uint8 \
                or not eds_batch.is_contiguous():
            raise ValueError("eds_batch must be a contiguous cuda uint8 tensor")
        self.eds = eds_batch.view(-1)
        self.square_stride = one if square_stride is None else int(square_stride)
        if self.square_stride < one or self.square_stride % 16:
            raise ValueError("square_stride must be a multiple of 16 B and at least one extended square")
        self.n = 0 if self.eds.numel() < one else 1 + (self.eds.numel() - one) // self.square_stride
        L = self.ctx._L
        col_off, dah_off = ctypes.c_size_t(0), ctypes.c_size_t(0)
        size = L.dagpu_proof_store_size(self.k, self.n, ctypes.byref(col_off), ctypes.byref(dah_off))
        if size == 0:
            raise DAError(_abi.ERR_ARG, f"no proof store for k = {k} and {self.n} squares")
        self.col_off, self.dah_off = col_off.value, dah_off.value
        self.row_bytes, self.col_bytes = L.dagpu_row_nodes_size(self.k), L.dagpu_col_nodes_size(self.k)
        self.dah_bytes = (4 * self.w - 1) * 32
        dev = self.eds.device
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            self.store = torch.empty((size,), dtype=torch.uint8, device=dev)
            ws = torch.empty((L.dagpu_proof_store_workspace_size(self.k, self.n),), dtype=torch.uint8, device=dev)
        self.ctx.check(L.dagpu_proof_store_device(self.ctx.handle, self.k, self.n, _abi.addr(self.eds),
                                                  self.square_stride, _abi.addr(self.store), _abi.addr(ws),
                                                  _stream_handle(s)))

    def square(self, i: int) -> StoreSquare:
        if not 0 <= i < self.n:
            raise IndexError(f"square {i} of {self.n}")
        return StoreSquare(self, i)

    def dah_tree(self) -> torch.Tensor:
        """(n, 8k - 1, 32) view of the DAH region: per square the 4k leaf
        hashes, then each level above; the last digest is the data root."""
        return self.store[self.dah_off:self.dah_off + self.n * self.dah_bytes].view(self.n, 4 * self.w - 1, 32)

    def data_roots(self) -> torch.Tensor:
        """(n, 32) view of the data roots: the top of each square's DAH tree."""
        return self.dah_tree()[:, -1, :]


class SquaresProofs(NamedTuple):
    """What nmt_prove_squares_device returns: uint8 device tensors (shares None
    without shares=True; axis_roots, leaf_hashes and aunts None without
    to_data_root=True) and the two HOST descriptor arrays."""
    nodes: torch.Tensor                  # 90 B per proof node
    namespaces: torch.Tensor             # 29 B per request
    shares: Optional[torch.Tensor]       # 512 B per proven cell
    axis_roots: Optional[torch.Tensor]   # 90 B per request
    leaf_hashes: Optional[torch.Tensor]  # 32 B per request
    aunts: Optional[torch.Tensor]        # log2(4k) x 32 B per request
    desc: "object"                       # (n, 8) int64: nmt_verify_batch_device, roots table = axis_roots
    mdesc: "object"                      # (n, 6) int64: dagpu_merkle_verify_batch, roots = store.data_roots()


def nmt_prove_squares_device(store: ProofStore, requests, shares: bool = True, to_data_root: bool = True,
                             ctx: Optional[Context] = None, stream: Optional[torch.cuda.Stream] = None,
                             workspace: Optional[torch.Tensor] = None) -> SquaresProofs:
    """dagpu_nmt_prove_squares_device: nmt ProveRange for many (square, axis,
    index, start, end) requests across the squares of a ProofStore, and with
    to_data_root the merkle proof of each proven tree's root under its
    square's data root, enqueued on `stream` (no sync of the results).
    requests: (n, 5) int64-like on the HOST.  Outputs as nmt_prove_batch_device,
    request by request; see SquaresProofs."""
    import ctypes

    import numpy as np
    c = ctx or store.ctx
    req = np.ascontiguousarray(np.asarray(requests, dtype=np.int64).reshape(-1, _abi.PROVE_SQ_REQ_WORDS))
    n = int(req.shape[0])
    w, dev = store.w, store.store.device
    m = w.bit_length() - 1
    start, last = req[:, 3].clip(0, w), (req[:, 4] - 1).clip(0, w - 1)

    def popcount(v):
        return np.unpackbits(v.astype(">u4").view(np.uint8)).reshape(len(v), 32).sum(axis=1)

    # capacities from the requests as given; the library validates them
    nodes_cap = int((popcount(start) + m - popcount(last)).sum()) if n else 0
    shares_cap = int((req[:, 4] - req[:, 3]).clip(0, w).sum()) if shares else 0
    la = m + 1  # log2(4k) aunts per proof
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    need = c._L.dagpu_nmt_prove_squares_workspace_size(n)
    with torch.cuda.stream(s):
        out_nodes = torch.empty((nodes_cap * ROOT,), dtype=torch.uint8, device=dev)
        out_ns = torch.empty((n * 29,), dtype=torch.uint8, device=dev)
        out_shares = torch.empty((shares_cap * 512,), dtype=torch.uint8, device=dev) if shares else None
        out_roots = torch.empty((n * ROOT,), dtype=torch.uint8, device=dev) if to_data_root else None
        out_lh = torch.empty((n * 32,), dtype=torch.uint8, device=dev) if to_data_root else None
        out_aunts = torch.empty((n * la * 32,), dtype=torch.uint8, device=dev) if to_data_root else None
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    if workspace.numel() < need:
        raise ValueError("workspace smaller than dagpu_nmt_prove_squares_workspace_size")
    desc = np.zeros((n, _abi.NMT_DESC_WORDS), np.int64)
    mdesc = np.zeros((n, _abi.MERKLE_DESC_WORDS), np.int64) if to_data_root else None
    total = ctypes.c_size_t(0)
    rc = c._L.dagpu_nmt_prove_squares_device(
        c.handle, store.k, store.n, n, _abi.addr(req), _abi.addr(store.eds) if shares else None,
        store.square_stride, _abi.addr(store.store), _abi.addr(out_nodes), nodes_cap, _abi.addr(out_ns),
        _abi.addr(out_shares) if shares else None, shares_cap, _abi.addr(out_roots) if to_data_root else None,
        _abi.addr(out_lh) if to_data_root else None, _abi.addr(out_aunts) if to_data_root else None,
        _abi.addr(desc), _abi.addr(mdesc) if to_data_root else None, ctypes.byref(total), _abi.addr(workspace),
        _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return SquaresProofs(out_nodes[:total.value * ROOT], out_ns, out_shares, out_roots, out_lh, out_aunts, desc,
                         mdesc)


def share_proof_requests(k: int, n_sq: int, ranges):
    """dagpu_share_proof_requests: NewShareInclusionProof's row split of
    (square, start, end) ranges of row-major ODS share indexes.  Returns (req
    (n_req, 5) int64, span (n + 1,) int64): range i owns requests
    span[i] .. span[i + 1].  Host arithmetic; raises DAError(ERR_ARG) on an
    invalid range."""
    import ctypes

    import numpy as np
    sreq = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 3))
    n = int(sreq.shape[0])
    # a range touches at most (end - 1) // k - start // k + 1 rows
    cap = int(((sreq[:, 2] - 1).clip(0, k * k) // k - sreq[:, 1].clip(0, k * k) // k + 1).clip(0).sum()) if n else 0
    req = np.zeros((max(cap, 1), _abi.PROVE_SQ_REQ_WORDS), np.int64)
    span = np.zeros(n + 1, np.int64)
    n_req = ctypes.c_size_t(0)
    rc = _abi.lib().dagpu_share_proof_requests(k, n_sq, n, _abi.addr(sreq), _abi.addr(req), cap, _abi.addr(span),
                                               ctypes.byref(n_req))
    if rc != 0:
        raise DAError(rc, f"invalid share range for {n_sq} squares of width {k}")
    return req[:n_req.value], span


def _ns_table(namespaces):
    """(n_q, 29) uint8 HOST array of a list of 29-B namespaces (or such an array)."""
    import numpy as np
    if isinstance(namespaces, np.ndarray):
        q = np.ascontiguousarray(namespaces, dtype=np.uint8).reshape(-1, 29)
    else:
        if any(len(n) != 29 for n in namespaces):
            raise ValueError("namespaces must be 29 bytes each")
        q = np.frombuffer(b"".join(bytes(n) for n in namespaces), np.uint8).reshape(-1, 29).copy()
    return q


def nmt_namespace_ranges_device(nodes, namespaces, ctx: Optional[Context] = None,
                                stream: Optional[torch.cuda.Stream] = None,
                                workspace: Optional[torch.Tensor] = None):
    """dagpu_nmt_namespace_ranges_device: where every namespace of a list lies
    in every ROW tree of one resident square (nodes: inclusion.EDSAxisNodes).
    Returns (ranges, counts): ranges an (n_q, 2k, 3) int32 HOST array of
    (kind, start, end) with kind _abi.NS_OUTSIDE / NS_PRESENT / NS_ABSENT, counts
    an int64[4] HOST array (proofs with kind != 0, absence proofs, proof nodes,
    proven cells).  Synchronises `stream` once."""
    import numpy as np
    c = ctx or nodes.ctx
    q = _ns_table(namespaces)
    n_q, w, dev = int(q.shape[0]), nodes.w, nodes.nodes.device
    ranges = np.zeros((n_q, w, 3), np.int32)
    counts = np.zeros(4, np.int64)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    need = c._L.dagpu_nmt_namespace_workspace_size(nodes.k, n_q)
    if workspace is None:
        with torch.cuda.stream(s):
            workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    if workspace.numel() < need:
        raise ValueError("workspace smaller than dagpu_nmt_namespace_workspace_size")
    rc = c._L.dagpu_nmt_namespace_ranges_device(c.handle, nodes.k, n_q, _abi.addr(q), _abi.addr(nodes.nodes),
                                                _abi.addr(ranges), _abi.addr(counts), _abi.addr(workspace),
                                                _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return ranges, counts


def nmt_prove_namespace_batch_device(nodes, namespaces, caps=None, ctx: Optional[Context] = None,
                                     stream: Optional[torch.cuda.Stream] = None,
                                     workspace: Optional[torch.Tensor] = None):
    """dagpu_nmt_prove_namespace_batch_device: nmt ProveNamespace of every
    namespace of a list on every ROW tree of one resident square (nodes:
    inclusion.EDSAxisNodes, whose `eds` is gathered from), enqueued on `stream`.

    caps = (proofs, nodes, cells, leaf_hashes) sizes the outputs; a capacity too
    small raises DAError(ERR_ARG) (the library reports the need).  Without caps
    the need is taken from nmt_namespace_ranges_device first (a second search).

    Returns (proof_nodes, namespaces, shares, leaf_hashes, desc, pairs, counts):
    uint8 device tensors of 90 B per node, 29 B per query, 512 B per proven cell
    and 90 B per absence proof; desc the (n, 9) int64 HOST descriptors
    nmt_verify_namespace_batch_device takes against the row roots (ns_index =
    query, root_index = row); pairs the (n, 2) int32 HOST (query, row) of each
    proof; counts as nmt_namespace_ranges_device.  Rows a namespace is outside
    of have no entry: their proof is the empty proof."""
    import numpy as np
    c = ctx or nodes.ctx
    q = _ns_table(namespaces)
    n_q, dev = int(q.shape[0]), nodes.nodes.device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    need = c._L.dagpu_nmt_namespace_workspace_size(nodes.k, n_q)
    if workspace is None:
        with torch.cuda.stream(s):
            workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    if workspace.numel() < need:
        raise ValueError("workspace smaller than dagpu_nmt_namespace_workspace_size")
    if caps is None:
        caps = nmt_namespace_ranges_device(nodes, q, ctx=c, stream=s, workspace=workspace)[1][[0, 2, 3, 1]]
    n_p, n_nodes, n_cells, n_lh = (int(v) for v in caps)
    with torch.cuda.stream(s):
        out_nodes = torch.empty((n_nodes * ROOT,), dtype=torch.uint8, device=dev)
        out_ns = torch.empty((n_q * 29,), dtype=torch.uint8, device=dev)
        out_shares = torch.empty((n_cells * 512,), dtype=torch.uint8, device=dev)
        out_lh = torch.empty((n_lh * ROOT,), dtype=torch.uint8, device=dev)
    desc = np.zeros((n_p, _abi.NMT_NS_DESC_WORDS), np.int64)
    pairs = np.zeros((n_p, 2), np.int32)
    counts = np.zeros(4, np.int64)
    rc = c._L.dagpu_nmt_prove_namespace_batch_device(
        c.handle, nodes.k, n_q, _abi.addr(q), _abi.addr(nodes.eds), _abi.addr(nodes.nodes),
        _abi.addr(out_nodes) if n_nodes else None, n_nodes, _abi.addr(out_ns) if n_q else None,
        _abi.addr(out_shares) if n_cells else None, n_cells, _abi.addr(out_lh) if n_lh else None, n_lh,
        _abi.addr(desc) if n_p else None, _abi.addr(pairs) if n_p else None, n_p, _abi.addr(counts),
        _abi.addr(workspace), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    n = int(counts[0])
    return (out_nodes[:int(counts[2]) * ROOT], out_ns, out_shares[:int(counts[3]) * 512],
            out_lh[:int(counts[1]) * ROOT], desc[:n], pairs[:n], counts)


def nmt_namespace_squares_count_device(store: ProofStore, namespaces, per: bool = True,
                                       ctx: Optional[Context] = None, stream: Optional[torch.cuda.Stream] = None,
                                       workspace: Optional[torch.Tensor] = None):
    """dagpu_nmt_namespace_squares_count_device: how many namespace proofs a
    list of namespaces has over ALL squares of a ProofStore.  Returns (counts,
    per): counts an int64[4] HOST array (proofs with kind != 0, absence proofs,
    proof nodes, proven cells), per the (n_q, n_sq) int32 HOST array of proofs
    per (query, square) -- which squares hold a namespace -- or None with
    per=False.  Synchronises `stream` once."""
    import numpy as np
    c = ctx or store.ctx
    q = _ns_table(namespaces)
    n_q, dev = int(q.shape[0]), store.store.device
    counts = np.zeros(4, np.int64)
    per_out = np.zeros((n_q, store.n), np.int32) if per else None
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    need = c._L.dagpu_nmt_namespace_squares_workspace_size(store.k, store.n, n_q, 0)
    if need == 0:
        raise DAError(_abi.ERR_ARG, f"{n_q} namespaces x {store.n} squares x {store.w} rows overflow")
    if workspace is None:
        with torch.cuda.stream(s):
            workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    if workspace.numel() < need:
        raise ValueError("workspace smaller than dagpu_nmt_namespace_squares_workspace_size")
    rc = c._L.dagpu_nmt_namespace_squares_count_device(
        c.handle, store.k, store.n, n_q, _abi.addr(q), _abi.addr(store.store), _abi.addr(counts),
        _abi.addr(per_out) if per and n_q else None, _abi.addr(workspace), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return counts, per_out


class NamespaceSquaresProofs(NamedTuple):
    """What nmt_prove_namespace_squares_device returns: uint8 device tensors
    (axis_roots, dah_leaf_hashes and aunts None without to_data_root=True) and
    the HOST arrays."""
    nodes: torch.Tensor                      # 90 B per proof node
    namespaces: torch.Tensor                 # 29 B per query
    shares: torch.Tensor                     # 512 B per proven cell
    leaf_hashes: torch.Tensor                # 90 B per absence proof
    axis_roots: Optional[torch.Tensor]       # 90 B per proof: its row root
    dah_leaf_hashes: Optional[torch.Tensor]  # 32 B per proof
    aunts: Optional[torch.Tensor]            # log2(4k) x 32 B per proof
    desc: "object"    # (n, 9) int64: nmt_verify_namespace_batch_device, roots table = axis_roots
    mdesc: "object"   # (n, 6) int64: dagpu_merkle_verify_batch, roots = store.data_roots(); None without to_data_root
    hits: "object"    # (n, 6) int32: query, square, row, kind, start, end
    counts: "object"  # int64[4]: proofs, absence proofs, proof nodes, proven cells


def nmt_prove_namespace_squares_device(store: ProofStore, namespaces, caps=None, to_data_root: bool = True,
                                       ctx: Optional[Context] = None, stream: Optional[torch.cuda.Stream] = None,
                                       workspace: Optional[torch.Tensor] = None) -> NamespaceSquaresProofs:
    """dagpu_nmt_prove_namespace_squares_device: nmt ProveNamespace of every
    namespace of a list on every ROW tree of every square of a ProofStore, in
    (query, square, row) order, and with to_data_root the merkle proof of each
    row root under its square's data root; enqueued on `stream`.

    caps = (proofs, nodes, cells, leaf_hashes) sizes the outputs as in
    nmt_prove_namespace_batch_device; a capacity too small raises
    DAError(ERR_ARG).  Without caps the need is taken from
    nmt_namespace_squares_count_device first (a second search)."""
    import numpy as np
    c = ctx or store.ctx
    q = _ns_table(namespaces)
    n_q, dev = int(q.shape[0]), store.store.device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    if caps is None:
        caps = nmt_namespace_squares_count_device(store, q, per=False, ctx=c, stream=s)[0][[0, 2, 3, 1]]
    n_p, n_nodes, n_cells, n_lh = (int(v) for v in caps)
    need = c._L.dagpu_nmt_namespace_squares_workspace_size(store.k, store.n, n_q, n_p)
    if need == 0:
        raise DAError(_abi.ERR_ARG, f"{n_q} namespaces x {store.n} squares x {store.w} rows overflow")
    la = store.w.bit_length()  # log2(4k) aunts per proof
    with torch.cuda.stream(s):
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
        out_nodes = torch.empty((n_nodes * ROOT,), dtype=torch.uint8, device=dev)
        out_ns = torch.empty((n_q * 29,), dtype=torch.uint8, device=dev)
        out_shares = torch.empty((n_cells * 512,), dtype=torch.uint8, device=dev)
        out_lh = torch.empty((n_lh * ROOT,), dtype=torch.uint8, device=dev)
        out_roots = torch.empty((n_p * ROOT,), dtype=torch.uint8, device=dev) if to_data_root else None
        out_dlh = torch.empty((n_p * 32,), dtype=torch.uint8, device=dev) if to_data_root else None
        out_aunts = torch.empty((n_p * la * 32,), dtype=torch.uint8, device=dev) if to_data_root else None
    if workspace.numel() < need:
        raise ValueError("workspace smaller than dagpu_nmt_namespace_squares_workspace_size")
    desc = np.zeros((n_p, _abi.NMT_NS_DESC_WORDS), np.int64)
    mdesc = np.zeros((n_p, _abi.MERKLE_DESC_WORDS), np.int64) if to_data_root else None
    hits = np.zeros((n_p, _abi.NS_HIT_WORDS), np.int32)
    counts = np.zeros(4, np.int64)
    rc = c._L.dagpu_nmt_prove_namespace_squares_device(
        c.handle, store.k, store.n, n_q, _abi.addr(q), _abi.addr(store.eds), store.square_stride,
        _abi.addr(store.store), _abi.addr(out_nodes) if n_nodes else None, n_nodes,
        _abi.addr(out_ns) if n_q else None, _abi.addr(out_shares) if n_cells else None, n_cells,
        _abi.addr(out_lh) if n_lh else None, n_lh,
        _abi.addr(out_roots) if to_data_root and n_p else None, _abi.addr(out_dlh) if to_data_root and n_p else None,
        _abi.addr(out_aunts) if to_data_root and n_p else None, _abi.addr(desc) if n_p else None,
        _abi.addr(mdesc) if to_data_root and n_p else None, _abi.addr(hits) if n_p else None, n_p, _abi.addr(counts),
        _abi.addr(workspace), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    n = int(counts[0])
    return NamespaceSquaresProofs(
        out_nodes[:int(counts[2]) * ROOT], out_ns, out_shares[:int(counts[3]) * 512], out_lh[:int(counts[1]) * ROOT],
        out_roots[:n * ROOT] if to_data_root else None, out_dlh[:n * 32] if to_data_root else None,
        out_aunts[:n * la * 32] if to_data_root else None, desc[:n], mdesc[:n] if to_data_root else None, hits[:n],
        counts)


def nmt_verify_namespace_batch_device(desc, namespaces: torch.Tensor, leaves: torch.Tensor, leaf_len: int,
                                      nodes: torch.Tensor, leaf_hashes: torch.Tensor, roots: torch.Tensor,
                                      ctx: Optional[Context] = None, stream: Optional[torch.cuda.Stream] = None,
                                      workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dagpu_nmt_verify_namespace_batch_device: nmt Proof.VerifyNamespace
    (presence with completeness, absence, empty) for many proofs against data
    already in HBM; returns the (n,) int32 status tensor on the device, enqueued
    on `stream`.  desc: (n, 9) int64 on the HOST (the eight words of
    nmt_verify_batch_device plus leaf_hash_index into `leaf_hashes`, 90 B each,
    -1 = none); the tensors as nmt_verify_batch_device."""
    import numpy as np
    c = ctx or default_context()
    d = np.ascontiguousarray(np.asarray(desc, dtype=np.int64).reshape(-1, _abi.NMT_NS_DESC_WORDS))
    n = int(d.shape[0])
    dev = roots.device
    for t in (namespaces, leaves, nodes, leaf_hashes, roots):
        if t.dtype != torch.uint8 or t.device != dev or not t.is_contiguous():
            raise ValueError("namespaces, leaves, nodes, leaf_hashes and roots must be contiguous uint8 tensors "
                             "on one device")
    n_leaves = leaves.numel() // leaf_len if leaf_len else int(d[:, 2].clip(min=0).sum())
    n_proven = int(d[:, 2].clip(min=0, max=max(n_leaves, 0)).sum())
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    need = c._L.dagpu_nmt_verify_namespace_workspace_size(n, n_proven)
    with torch.cuda.stream(s):
        status = torch.empty((n,), dtype=torch.int32, device=dev)
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    if workspace.numel() < need:
        raise ValueError("workspace smaller than dagpu_nmt_verify_namespace_workspace_size")
    rc = c._L.dagpu_nmt_verify_namespace_batch_device(
        c.handle, n, _abi.addr(d), _abi.addr(namespaces), namespaces.numel() // 29,
        _abi.addr(leaves) if leaves.numel() else None, n_leaves, leaf_len,
        _abi.addr(nodes) if nodes.numel() else None, nodes.numel() // ROOT,
        _abi.addr(leaf_hashes) if leaf_hashes.numel() else None, leaf_hashes.numel() // ROOT,
        _abi.addr(roots), roots.numel() // ROOT, _abi.addr(status), _abi.addr(workspace), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return status


def write_squares_device(k: int, plans, srcs, out: torch.Tensor, square_stride: int, row_pitch: int,
                         ctx: Optional[Context] = None, stream: Optional[torch.cuda.Stream] = None,
                         lead: int = 0) -> None:
    """dagpu_square_write_device: the squares of n plans (square.plan_native;
    uint8 arrays) and their blocks' packed txs (srcs: n bytes-likes, uploaded
    back to back behind `lead` unused bytes) written into `out` (cuda uint8),
    square i at byte i * square_stride, rows row_pitch bytes apart.  Enqueued
    on `stream`; returns once the plans and txs have left host memory."""
    import numpy as np
    c = ctx or default_context()
    n, dev = len(plans), out.device
    if len(srcs) != n:
        raise ValueError("one packed txs buffer per plan")
    if n == 0:
        return
    if out.dtype != torch.uint8 or not out.is_contiguous() or \
            out.numel() < (n - 1) * square_stride + (k - 1) * row_pitch + k * 512:
        raise ValueError("out must be a contiguous cuda uint8 tensor holding n squares at the given strides")
    offs = np.zeros(n + 1, np.uint64)
    offs[0] = lead
    for i, b in enumerate(srcs):
        offs[i + 1] = offs[i] + len(b)
    total = int(offs[n])
    host = torch.empty((max(total, 1),), dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    for i, b in enumerate(srcs):
        if len(b):
            hv[int(offs[i]):int(offs[i + 1])] = np.frombuffer(b, np.uint8)
    plans = [np.ascontiguousarray(p, dtype=np.uint8) for p in plans]
    sizes = np.array([p.size for p in plans], np.uint64)
    ptrs = np.array([_abi.addr(p) for p in plans], np.uint64)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        d_src = host.to(dev, non_blocking=True)
        ws = torch.empty((c._L.dagpu_square_write_workspace_size(n, int(sizes.sum())),), dtype=torch.uint8,
                         device=dev)
    rc = c._L.dagpu_square_write_device(c.handle, k, n, _abi.addr(ptrs), _abi.addr(sizes), _abi.addr(d_src),
                                        _abi.addr(offs), total, _abi.addr(out), square_stride, row_pitch,
                                        _abi.addr(ws), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    # the pinned staging buffer goes back to torch's host cache, which reuses
    # it only after the copy queued above has run
    del host


class PlannedSquares:
    """What dagpu_square_plan_device / dagpu_square_construct_device left in
    HBM for n blocks: the plan arena, one record and one status word per block
    (square.plan_record_dtype, _abi.PLAN_*), and the packed txs they refer to.
    Nothing is downloaded until it is asked for."""

    def __init__(self, n, arena, records, status, src, src_lens, stream):
        self.n, self.arena, self.records, self.status = n, arena, records, status
        self.src, self.src_lens, self._stream = src, src_lens, stream
        self._rec = self._plans = None
        # the request as the planner took it (host arrays), for validate_blob_txs_device
        self.src_offs = self.ntx = self.tx_lens = None
        self.src_bytes = self.arena_cap = 0

    def status_host(self):
        """The n status words: the one read a caller needs to go on."""
        self._stream.synchronize()
        return self.status[:self.n].cpu().numpy().view("<u4").copy()

    def records_host(self):
        from . import square as sq
        if self._rec is None:
            self._stream.synchronize()
            self._rec = self.records.cpu().numpy().view(sq.plan_record_dtype())[:self.n].copy()
        return self._rec

    def plans_host(self):
        """Each block's plan as a uint8 array (None for a rejected block): the
        used part of the arena, downloaded once."""
        import numpy as np
        if self._plans is None:
            rec = self.records_host()
            used = int(max((int(r["plan_off"]) + int(r["plan_bytes"]) for r in rec), default=0))
            arena = self.arena[:used].cpu().numpy() if used else np.zeros(0, np.uint8)
            self._plans = [None if int(r["plan_bytes"]) == 0 else
                           arena[int(r["plan_off"]):int(r["plan_off"]) + int(r["plan_bytes"])].copy() for r in rec]
        return self._plans


def plan_squares_device(blocks, max_square_size: int = 128, threshold: int = 64, device: int = 0,
                        ctx: Optional[Context] = None, stream: Optional[torch.cuda.Stream] = None,
                        k: Optional[int] = None, out: Optional[torch.Tensor] = None, square_stride: int = 0,
                        row_pitch: int = 0, threads: int = 16) -> PlannedSquares:
    """dagpu_square_plan_device over n blocks of raw txs (each a sequence of
    bytes): one upload of the packed batch, then the planner's kernels; no
    layout on the host.  With k and out (cuda uint8) it is
    dagpu_square_construct_device: the squares of width k are written behind
    the planner in the same enqueue, square i at out + i * square_stride, rows
    row_pitch apart; a rejected block, or one of another width, leaves its
    window untouched and says so in its status word.  Enqueued on `stream`."""
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    c = ctx or default_context()
    n = len(blocks)
    dev = out.device if out is not None else torch.device("cuda", device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    # pack: the lengths, then every block's txs straight into the pinned staging
    # buffer, blocks side by side on the pool (the copies release the GIL)
    ntx = np.array([len(b) for b in blocks], np.uint32)
    workers = max(1, min(16, int(threads), n))
    pool = ThreadPoolExecutor(workers) if workers > 1 else None
    each = pool.map if pool else map
    per = list(each(lambda b: np.fromiter(map(len, b), np.uint64, len(b)), blocks))
    lens = np.concatenate(per) if per else np.zeros(0, np.uint64)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([int(v.sum()) for v in per], dtype=np.uint64)
    total = int(offs[n])
    host = torch.empty((max(total, 1),), dtype=torch.uint8).pin_memory()
    hv = host.numpy()

    def fill(i):
        if offs[i + 1] > offs[i]:
            hv[int(offs[i]):int(offs[i + 1])] = np.frombuffer(b"".join(blocks[i]), np.uint8)
    list(each(fill, range(n)))
    if pool:
        pool.shutdown()
    cap = c._L.dagpu_square_plan_device_arena_size(n, int(lens.size), max_square_size)
    with torch.cuda.stream(s):
        d_src = host.to(dev, non_blocking=True)
        arena = torch.empty((max(cap, 16),), dtype=torch.uint8, device=dev)
        records = torch.empty((max(n, 1) * _abi.PLAN_RECORD_BYTES,), dtype=torch.uint8, device=dev)
        status = torch.zeros((max(n, 4),), dtype=torch.int32, device=dev)
        ws = torch.empty((max(c._L.dagpu_square_plan_device_workspace_size(n, int(lens.size), max_square_size), 16),),
                         dtype=torch.uint8, device=dev)
    common = (_abi.addr(d_src), _abi.addr(offs), total, _abi.addr(ntx),
              _abi.addr(lens) if lens.size else None, max_square_size, threshold, _abi.addr(arena), cap,
              _abi.addr(records))
    if out is None:
        rc = c._L.dagpu_square_plan_device(c.handle, n, *common, _abi.addr(status), _abi.addr(ws), _stream_handle(s))
    else:
        if out.dtype != torch.uint8 or not out.is_contiguous() or \
                (n and out.numel() < (n - 1) * square_stride + (k - 1) * row_pitch + k * 512):
            raise ValueError("out must be a contiguous cuda uint8 tensor holding n squares at the given strides")
        rc = c._L.dagpu_square_construct_device(c.handle, k, n, *common, _abi.addr(out), square_stride, row_pitch,
                                                _abi.addr(status), _abi.addr(ws), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    # the workspace is read by kernels still queued: torch's allocator reuses it
    # only for work queued on the same stream behind them
    del host
    p = PlannedSquares(n, arena, records, status, d_src, [int(offs[i + 1] - offs[i]) for i in range(n)], s)
    p.src_offs, p.ntx, p.tx_lens, p.src_bytes, p.arena_cap = offs, ntx, lens, total, cap
    return p


def validate_blob_txs_device(planned: PlannedSquares, blob_base="plans", ctx: Optional[Context] = None,
                             stream: Optional[torch.cuda.Stream] = None):
    """dagpu_blob_tx_validate_device over the txs plan_squares_device left in
    HBM: the stateless rules of ValidateBlobTx on every tx where it lies, and
    the table of the commitments the MsgPayForBlobs declare.

    blob_base: (n + 1,) uint64-like on the HOST, block i's plan blobs own rows
    [blob_base[i], blob_base[i + 1]) of the table; "plans" (the default) takes
    each accepted block's blob count from the planner's records (one small
    read), which is DeviceSquares.blob_table()'s order; None ties nothing.
    Returns cuda tensors (tx_status (ntx_total,) int32, block_status (n, 2)
    int32 {lowest failing tx or -1, its word}, expected (rows, 32) uint8); a
    word is kind | index << 8 (blobtx.KIND_NAMES).  Enqueued on `stream`: it
    does not synchronise."""
    import numpy as np
    c = ctx or default_context()
    n, dev = planned.n, planned.src.device
    if planned.src_offs is None:
        raise ValueError("planned carries no request: it must come from plan_squares_device")
    if isinstance(blob_base, str):
        if blob_base != "plans":
            raise ValueError("blob_base is an array, None or 'plans'")
        rec = planned.records_host()
        counts = np.where(rec["plan_bytes"] == 0, 0, rec["nblob"]).astype(np.uint64)
        blob_base = np.concatenate([np.zeros(1, np.uint64), np.cumsum(counts, dtype=np.uint64)])
    elif blob_base is not None:
        blob_base = np.ascontiguousarray(np.asarray(blob_base, dtype=np.uint64).reshape(-1))
        if blob_base.size != n + 1:
            raise ValueError("blob_base holds n + 1 offsets")
    rows = int(blob_base[n]) if blob_base is not None and n else 0
    ntx_total = int(planned.tx_lens.size)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        tx_status = torch.empty((max(ntx_total, 1),), dtype=torch.int32, device=dev)
        block_status = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
        expected = torch.empty((max(rows, 1), 32), dtype=torch.uint8, device=dev)
        ws = torch.empty((max(c._L.dagpu_blob_tx_validate_workspace_size(n, ntx_total, rows), 16),),
                         dtype=torch.uint8, device=dev)
    rc = c._L.dagpu_blob_tx_validate_device(
        c.handle, n, _abi.addr(planned.src), _abi.addr(planned.src_offs), planned.src_bytes, _abi.addr(planned.ntx),
        _abi.addr(planned.tx_lens) if ntx_total else None, _abi.addr(planned.arena), planned.arena_cap,
        _abi.addr(planned.records), _abi.addr(blob_base), _abi.addr(tx_status), _abi.addr(block_status),
        _abi.addr(expected), _abi.addr(ws), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return tx_status[:ntx_total], block_status[:n], expected[:rows]


def secp256k1_verify_device(digests: torch.Tensor, sigs: torch.Tensor, pubkeys: torch.Tensor,
                            ctx: Optional[Context] = None, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """dagpu_secp256k1_verify_device: n secp256k1 ECDSA verifications, one lane
    each.  digests (n, 32), sigs (n, 64; big-endian r | s) and pubkeys (n, 33;
    compressed) are contiguous cuda uint8 tensors.  Returns the (n,) int32
    status words (_abi.SIG_KIND_NAMES: 0, or BAD_PUBKEY, OUT_OF_RANGE, HIGH_S,
    MISMATCH), enqueued on `stream`: it does not synchronise."""
    c = ctx or default_context()
    n = int(digests.shape[0]) if digests.dim() else 0
    for t, width, name in ((digests, 32, "digests"), (sigs, 64, "sigs"), (pubkeys, 33, "pubkeys")):
        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (n, width):
            raise ValueError(f"{name} must be a contiguous cuda uint8 tensor of shape (n, {width})")
    dev = digests.device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        status = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
    rc = c._L.dagpu_secp256k1_verify_device(c.handle, n, _abi.addr(digests), _abi.addr(sigs), _abi.addr(pubkeys),
                                            _abi.addr(status), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return status[:n]


def tx_signers_device(planned: PlannedSquares, ctx: Optional[Context] = None,
                      stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """dagpu_tx_signers_device over the txs plan_squares_device left in HBM:
    the (ntx_total, 48) uint8 signer records {pubkey[33], kind, pad[6],
    sequence u64}: the key each tx carries and the sequence it declares, for
    the host's account lookup, nonce comparison and address check.  Enqueued on
    `stream`."""
    c = ctx or default_context()
    n, dev = planned.n, planned.src.device
    if planned.src_offs is None:
        raise ValueError("planned carries no request: it must come from plan_squares_device")
    ntx_total = int(planned.tx_lens.size)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        signers = torch.empty((max(ntx_total, 1), _abi.SIGNER_RECORD_BYTES), dtype=torch.uint8, device=dev)
        ws = torch.empty((max(c._L.dagpu_tx_sig_verify_workspace_size(n, ntx_total), 16),), dtype=torch.uint8,
                         device=dev)
    rc = c._L.dagpu_tx_signers_device(
        c.handle, n, _abi.addr(planned.src), _abi.addr(planned.src_offs), planned.src_bytes, _abi.addr(planned.ntx),
        _abi.addr(planned.tx_lens) if ntx_total else None, _abi.addr(signers), _abi.addr(ws), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return signers[:ntx_total]


def verify_tx_signatures_device(planned: PlannedSquares, chain_id, account_numbers, pubkeys=None,
                                ctx: Optional[Context] = None, stream: Optional[torch.cuda.Stream] = None,
                                workspace: Optional[torch.Tensor] = None):
    """dagpu_tx_sig_verify_device over the txs plan_squares_device left in HBM:
    the stateless half of the SigVerificationDecorator, one secp256k1 ECDSA
    verification over SHA-256(SignDoc) per tx (SIGN_MODE_DIRECT, one signer).

    chain_id: str or bytes, at most 64 bytes.  account_numbers: (ntx_total,)
    uint64-like, one per tx in batch order (a cuda int64 tensor is taken as it
    is, anything else is uploaded).  pubkeys: None, or (ntx_total, 33) uint8:
    the accounts' stored keys; a row whose first byte is 0 means none, a
    present row is used instead of the key the tx carries.
    Returns cuda tensors (tx_status (ntx_total,) int32, block_status (n, 4)
    int32 {lowest tx with a rejecting kind or -1, its word, number of
    not-judged txs, 0}, signers (ntx_total, 48) uint8); a word is kind |
    index << 8 (_abi.SIG_KIND_NAMES; blobtx.check_signature is the mirror).
    Enqueued on `stream`: it does not synchronise."""
    import numpy as np
    c = ctx or default_context()
    n, dev = planned.n, planned.src.device
    if planned.src_offs is None:
        raise ValueError("planned carries no request: it must come from plan_squares_device")
    ntx_total = int(planned.tx_lens.size)
    chain = chain_id.encode() if isinstance(chain_id, str) else bytes(chain_id)
    chain_buf = np.frombuffer(chain, np.uint8).copy()
    s = stream if stream is not None else torch.cuda.current_stream(dev)

    def table(v, dtype, shape, name):
        if isinstance(v, torch.Tensor) and v.is_cuda:
            if v.dtype != dtype or not v.is_contiguous() or tuple(v.shape) != shape:
                raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape}")
            return v
        a = np.ascontiguousarray(v.cpu().numpy() if isinstance(v, torch.Tensor) else v,
                                 np.uint64 if dtype == torch.int64 else np.uint8)
        if a.shape != shape:
            raise ValueError(f"{name} must have shape {shape}")
        a = a.view(np.int64) if dtype == torch.int64 else a
        return torch.from_numpy(a.copy()).to(dev, non_blocking=False)

    with torch.cuda.stream(s):
        accts = table(account_numbers, torch.int64, (ntx_total,), "account_numbers")
        keys = None if pubkeys is None else table(pubkeys, torch.uint8, (ntx_total, 33), "pubkeys")
        tx_status = torch.empty((max(ntx_total, 1),), dtype=torch.int32, device=dev)
        block_status = torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev)
        signers = torch.empty((max(ntx_total, 1), _abi.SIGNER_RECORD_BYTES), dtype=torch.uint8, device=dev)
        need = max(c._L.dagpu_tx_sig_verify_workspace_size(n, ntx_total), 16)
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
        elif workspace.dtype != torch.uint8 or not workspace.is_cuda or workspace.numel() < need:
            raise ValueError(f"workspace must be a cuda uint8 tensor of at least {need} bytes")
    rc = c._L.dagpu_tx_sig_verify_device(
        c.handle, n, _abi.addr(planned.src), _abi.addr(planned.src_offs), planned.src_bytes, _abi.addr(planned.ntx),
        _abi.addr(planned.tx_lens) if ntx_total else None, _abi.addr(chain_buf) if chain_buf.size else None,
        chain_buf.size, _abi.addr(accts) if ntx_total else None, _abi.addr(keys), _abi.addr(tx_status),
        _abi.addr(block_status), _abi.addr(signers), _abi.addr(workspace), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return tx_status[:ntx_total], block_status[:n], signers[:ntx_total]


class CommitPlan(NamedTuple):
    """commit_plan_device's outputs, cuda tensors at capacity: the table image
    (uint32 words, commit_layout's), the counts record {nblobs, nshares, nsub,
    nwork, max_subtrees, 0, 0, 0} and blob_base (n + 1 int64)."""
    tables: torch.Tensor
    counts: torch.Tensor
    blob_base: torch.Tensor


def commit_plan_device(planned: PlannedSquares, k: int, threshold: int = 64, ctx: Optional[Context] = None,
                       stream: Optional[torch.cuda.Stream] = None) -> CommitPlan:
    """dagpu_commit_plan_device: the tables of the commitment check for the
    blocks of width k, laid out on the device from the plans and records
    plan_squares_device left in HBM.  Nothing is downloaded; enqueued on
    `stream`."""
    c = ctx or default_context()
    n, dev = planned.n, planned.arena.device
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    L = c._L
    with torch.cuda.stream(s):
        tables = torch.empty((max(L.dagpu_commit_plan_table_words(k, n), 4),), dtype=torch.int32, device=dev)
        counts = torch.zeros((_abi.COMMIT_COUNT_WORDS,), dtype=torch.int32, device=dev)
        blob_base = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        ws = torch.empty((max(L.dagpu_commit_plan_workspace_size(k, n), 16),), dtype=torch.uint8, device=dev)
    rc = L.dagpu_commit_plan_device(c.handle, k, n, _abi.addr(planned.arena), planned.arena_cap,
                                    _abi.addr(planned.records), threshold, _abi.addr(tables), _abi.addr(counts),
                                    _abi.addr(blob_base), _abi.addr(ws), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return CommitPlan(tables, counts, blob_base)


class ProposalCheck(NamedTuple):
    """proposal_check_device's outputs, cuda tensors.  The per-row tensors are
    sized by the capacity n * k * k; rows [0, blob_base[n]) are meaningful."""
    tx_status: torch.Tensor      # (ntx_total,) int32
    block_status: torch.Tensor   # (n, 2) int32
    expected: torch.Tensor       # (cap, 32) uint8
    commitments: torch.Tensor    # (cap, 32) uint8
    blob_status: torch.Tensor    # (cap,) int32
    row_tx: torch.Tensor         # (cap, 2) int32: {tx in the block, blob in the tx} or -1
    square_status: torch.Tensor  # (n,) int32
    counts: torch.Tensor         # (8,) int32
    blob_base: torch.Tensor      # (n + 1,) int64


def proposal_check_device(planned: PlannedSquares, k: int, squares: torch.Tensor, square_stride: int,
                          row_pitch: int, threshold: int = 64, ctx: Optional[Context] = None,
                          stream: Optional[torch.cuda.Stream] = None) -> ProposalCheck:
    """dagpu_proposal_check_device over what construct_squares_device left in
    HBM: ValidateBlobTx's stateless rules, the commitment layout, the tie of
    every plan blob to its declared commitment and the commitments of the
    squares, compared on the device.  One enqueue on `stream`, no read."""
    c = ctx or default_context()
    n, dev = planned.n, planned.src.device
    if planned.src_offs is None:
        raise ValueError("planned carries no request: it must come from plan_squares_device")
    ntx_total = int(planned.tx_lens.size)
    cap = max(n * k * k, 1)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    L = c._L
    with torch.cuda.stream(s):
        out = ProposalCheck(
            torch.empty((max(ntx_total, 1),), dtype=torch.int32, device=dev),
            torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev),
            torch.empty((cap, 32), dtype=torch.uint8, device=dev),
            torch.empty((cap, 32), dtype=torch.uint8, device=dev),
            torch.empty((cap,), dtype=torch.int32, device=dev),
            torch.empty((cap, 2), dtype=torch.int32, device=dev),
            torch.empty((max(n, 1),), dtype=torch.int32, device=dev),
            torch.zeros((_abi.COMMIT_COUNT_WORDS,), dtype=torch.int32, device=dev),
            torch.zeros((n + 1,), dtype=torch.int64, device=dev))
        ws = torch.empty((max(L.dagpu_proposal_check_workspace_size(k, n, ntx_total), 16),), dtype=torch.uint8,
                         device=dev)
    rc = L.dagpu_proposal_check_device(
        c.handle, k, n, _abi.addr(planned.src), _abi.addr(planned.src_offs), planned.src_bytes,
        _abi.addr(planned.ntx), _abi.addr(planned.tx_lens) if ntx_total else None, _abi.addr(planned.arena),
        planned.arena_cap, _abi.addr(planned.records), _abi.addr(squares), square_stride, row_pitch, threshold,
        *(_abi.addr(t) for t in out), _abi.addr(ws), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return out._replace(tx_status=out.tx_status[:ntx_total], block_status=out.block_status[:n],
                        square_status=out.square_status[:n])


def proposal_verdict_device(planned: PlannedSquares, k: int, check: ProposalCheck,
                            extend_status: Optional[torch.Tensor] = None, dah: Optional[torch.Tensor] = None,
                            data_hashes=None, square_sizes=None, ctx: Optional[Context] = None,
                            stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """dagpu_proposal_verdict_device: (n, 4) int32 {code, tx, word, aux} per
    block (_abi.VERDICT_NAMES) in ProcessProposal's order, from the planner's
    records, proposal_check_device's outputs, extend's status and data roots,
    and the proposed data_hashes ((n, 32) bytes) and square_sizes (n ints) on
    the HOST, either of which may be None.  Enqueued on `stream`."""
    import numpy as np
    c = ctx or default_context()
    n, dev = planned.n, planned.records.device
    hashes = sizes = None
    if data_hashes is not None:
        hashes = np.frombuffer(b"".join(bytes(h) for h in data_hashes), np.uint8).copy()
        if hashes.size != 32 * n:
            raise ValueError("data_hashes holds 32 bytes per block")
    if square_sizes is not None:
        sizes = np.ascontiguousarray(np.asarray(square_sizes, dtype=np.uint32).reshape(-1))
        if sizes.size != n:
            raise ValueError("square_sizes holds one width per block")
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    L = c._L
    with torch.cuda.stream(s):
        verdicts = torch.empty((max(n, 1), 4), dtype=torch.int32, device=dev)
        ws = torch.empty((max(L.dagpu_proposal_verdict_workspace_size(k, n, 0), 16),), dtype=torch.uint8, device=dev)
    rc = L.dagpu_proposal_verdict_device(
        c.handle, k, n, _abi.addr(planned.records), _abi.addr(check.block_status), _abi.addr(check.blob_status),
        _abi.addr(check.row_tx), _abi.addr(check.blob_base),
        _abi.addr(extend_status) if extend_status is not None else None, _abi.addr(dah) if dah is not None else None,
        _abi.addr(hashes) if hashes is not None else None, _abi.addr(sizes) if sizes is not None else None,
        _abi.addr(verdicts), _abi.addr(ws), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return verdicts[:n]


def construct_squares_device(k: int, blocks, out: torch.Tensor, square_stride: int, row_pitch: int,
                             max_square_size: int = 128, threshold: int = 64, ctx: Optional[Context] = None,
                             stream: Optional[torch.cuda.Stream] = None, threads: int = 16) -> PlannedSquares:
    """dagpu_square_construct_device: plan n blocks of raw txs on the device
    and write their squares of width k into `out`, in one enqueue (see
    plan_squares_device)."""
    return plan_squares_device(blocks, max_square_size, threshold, ctx=ctx, stream=stream, k=k, out=out,
                               square_stride=square_stride, row_pitch=row_pitch, threads=threads)


def blob_commitments_device(k: int, blobs, squares: torch.Tensor, square_stride: int, row_pitch: int,
                            expected=None, threshold: int = 64, ctx: Optional[Context] = None,
                            stream: Optional[torch.cuda.Stream] = None):
    """dagpu_blob_commitments_device: inclusion.CreateCommitment of many share
    ranges of squares resident in HBM, compared with `expected` on the device.

    blobs: (nblobs, 3) int64-like on the HOST, {square, first_share,
    share_count}; squares: a contiguous cuda uint8 tensor holding n squares,
    square i at byte i * square_stride, rows row_pitch bytes apart (n is what
    the tensor holds at that stride); expected: (nblobs, 32) uint8, a cuda
    tensor or a host array (uploaded on `stream`), or None.  Returns
    (commitments (nblobs, 32) uint8, status (nblobs,) int32, square_status (n,)
    int32) as cuda tensors; status bits _abi.COMMIT_MISMATCH /
    COMMIT_PUSH_ORDER, square_status the OR over each square's blobs.  Enqueued
    on `stream`: it does not synchronise."""
    import numpy as np
    c = ctx or default_context()
    rec = np.ascontiguousarray(np.asarray(blobs, dtype=np.int64).reshape(-1, 3))
    nb, dev = int(rec.shape[0]), squares.device
    if squares.dtype != torch.uint8 or not squares.is_contiguous():
        raise ValueError("squares must be a contiguous cuda uint8 tensor")
    one = (k - 1) * row_pitch + k * 512
    n = 0 if squares.numel() < one else 1 + (squares.numel() - one) // square_stride if square_stride else 1
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    need = c._L.dagpu_blob_commitments_workspace_size(k, nb, int(rec[:, 2].clip(min=0).sum()))
    with torch.cuda.stream(s):
        if expected is not None and not isinstance(expected, torch.Tensor):
            host = np.array(expected, dtype=np.uint8).reshape(-1)  # a writable copy for torch
            expected = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)
        out = torch.empty((nb, 32), dtype=torch.uint8, device=dev)
        status = torch.empty((nb,), dtype=torch.int32, device=dev)
        sq_status = torch.empty((n,), dtype=torch.int32, device=dev)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    if expected is not None and (expected.dtype != torch.uint8 or expected.device != dev
                                 or not expected.is_contiguous() or expected.numel() != nb * 32):
        raise ValueError("expected must hold 32 bytes per blob, contiguous uint8 on the squares' device")
    rc = c._L.dagpu_blob_commitments_device(
        c.handle, k, n, nb, _abi.addr(rec), _abi.addr(squares), square_stride, row_pitch, threshold, _abi.addr(out),
        _abi.addr(expected) if expected is not None and nb else None, _abi.addr(status),
        _abi.addr(sq_status) if n else None, _abi.addr(ws), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return out, status, sq_status


def _squares_held(k: int, squares: torch.Tensor, square_stride: int, row_pitch: int) -> int:
    """How many squares a contiguous uint8 tensor holds at these strides."""
    if squares.dtype != torch.uint8 or not squares.is_contiguous():
        raise ValueError("squares must be a contiguous cuda uint8 tensor")
    one = (k - 1) * row_pitch + k * 512
    return 0 if squares.numel() < one else 1 + (squares.numel() - one) // square_stride if square_stride else 1


def scan_squares_device(k: int, squares: torch.Tensor, square_stride: int, row_pitch: int,
                        seq_cap: Optional[int] = None, ctx: Optional[Context] = None,
                        stream: Optional[torch.cuda.Stream] = None, summary_host: bool = True):
    """dagpu_square_scan_device: shares.ParseShares of the squares a cuda uint8
    tensor holds (square i at byte i * square_stride, rows row_pitch apart).
    Returns (records, summary, host): records an (n, seq_cap, 64) uint8 cuda
    tensor of dagpu_seq_record (square.seq_dtype()), seq_cap = k*k by default;
    summary (n, 8) int32 on the device; host its copy as a numpy array, for
    which the call waits, or None with summary_host=False, when everything is
    only enqueued on `stream`.  Records past a square's sequence count keep
    what torch.empty left there."""
    import numpy as np
    c = ctx or default_context()
    n, dev = _squares_held(k, squares, square_stride, row_pitch), squares.device
    cap = k * k if seq_cap is None else int(seq_cap)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        records = torch.empty((n, cap, _abi.SEQ_RECORD_BYTES), dtype=torch.uint8, device=dev)
        summary = torch.empty((n, _abi.SCAN_SUMMARY_WORDS), dtype=torch.int32, device=dev)
        ws = torch.empty((max(c._L.dagpu_square_scan_workspace_size(k, n), 16),), dtype=torch.uint8, device=dev)
    host = np.zeros((n, _abi.SCAN_SUMMARY_WORDS), np.int32) if summary_host else None
    rc = c._L.dagpu_square_scan_device(c.handle, k, n, _abi.addr(squares), square_stride, row_pitch, cap,
                                       _abi.addr(records), _abi.addr(summary), _abi.addr(host), _abi.addr(ws),
                                       _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return records, summary, host


def read_sequences_device(k: int, squares: torch.Tensor, square_stride: int, row_pitch: int, records: torch.Tensor,
                          summary: torch.Tensor, payload_cap: int, namespaces=None,
                          classes: int = _abi.READ_BLOBS | _abi.READ_COMPACT, ctx: Optional[Context] = None,
                          stream: Optional[torch.cuda.Stream] = None, payload: Optional[torch.Tensor] = None):
    """dagpu_square_read_device over a scan's records and summary (both on the
    device): the payload of the non-padding sequences of the classes in
    `classes` (_abi.READ_BLOBS, READ_COMPACT) and of `namespaces` (29-byte
    values on the host; None: all), gathered into a cuda uint8 tensor of
    payload_cap bytes (`payload`, when given, is written in place).  Returns
    (selected (n*seq_cap,) int32 indices into the record table (the uint32 the
    library writes), offsets (n*seq_cap,) int64, totals (3,) int64 {n_selected,
    payload_bytes, overflow}, payload), all on the device and only enqueued on
    `stream`; entries past n_selected are not written."""
    import numpy as np
    c = ctx or default_context()
    n, dev = _squares_held(k, squares, square_stride, row_pitch), squares.device
    if records.dim() != 3 or records.shape[0] != n or records.shape[2] != _abi.SEQ_RECORD_BYTES \
            or not records.is_contiguous() or records.dtype != torch.uint8:
        raise ValueError("records must be the (n, seq_cap, 64) uint8 tensor of scan_squares_device")
    cap = int(records.shape[1])
    ns = None
    if namespaces is not None:
        ns = np.frombuffer(b"".join(bytes(x) for x in namespaces), np.uint8).copy()
        if ns.size != 29 * len(namespaces):
            raise ValueError("namespaces are 29 bytes each")
    n_ns = 0 if ns is None else len(namespaces)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        selected = torch.empty((n * cap,), dtype=torch.int32, device=dev)
        offsets = torch.empty((n * cap,), dtype=torch.int64, device=dev)
        totals = torch.empty((3,), dtype=torch.int64, device=dev)
        if payload is None:
            payload = torch.empty((max(int(payload_cap), 16),), dtype=torch.uint8, device=dev)
        ws = torch.empty((max(c._L.dagpu_square_read_workspace_size(k, n, cap, n_ns), 16),), dtype=torch.uint8,
                         device=dev)
    rc = c._L.dagpu_square_read_device(c.handle, k, n, _abi.addr(squares), square_stride, row_pitch, cap,
                                       _abi.addr(records), _abi.addr(summary), _abi.addr(ns) if n_ns else None, n_ns,
                                       classes, _abi.addr(selected), _abi.addr(offsets), _abi.addr(totals),
                                       _abi.addr(payload), int(payload_cap), _abi.addr(ws), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return selected, offsets, totals, payload


def unit_table_device(k: int, squares: torch.Tensor, square_stride: int, row_pitch: int, records: torch.Tensor,
                      summary: torch.Tensor, unit_cap: int, ctx: Optional[Context] = None,
                      stream: Optional[torch.cuda.Stream] = None, summary_host: bool = True,
                      workspace: Optional[torch.Tensor] = None):
    """dagpu_square_units_device over a scan's records and summary (both on the
    device): where every tx and wrapped PFB of the squares lies.  Returns
    (units, unit_summary, host): units an (n, unit_cap, 32) uint8 cuda tensor of
    dagpu_unit_record (square.unit_dtype()), unit_summary (n, 8) int32 on the
    device, host its copy as a numpy array, for which the call waits, or None
    with summary_host=False, when everything is only enqueued on `stream`
    (`workspace`, dagpu_square_units_workspace_size bytes, is allocated when
    not given).  Records past a square's unit count keep what torch.empty left."""
    import numpy as np
    c = ctx or default_context()
    n, dev = _squares_held(k, squares, square_stride, row_pitch), squares.device
    if records.dim() != 3 or records.shape[0] != n or records.shape[2] != _abi.SEQ_RECORD_BYTES \
            or not records.is_contiguous() or records.dtype != torch.uint8:
        raise ValueError("records must be the (n, seq_cap, 64) uint8 tensor of scan_squares_device")
    cap, seq_cap = int(unit_cap), int(records.shape[1])
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        units = torch.empty((n, max(cap, 1), _abi.UNIT_RECORD_BYTES), dtype=torch.uint8, device=dev)
        unit_summary = torch.empty((n, _abi.UNITS_SUMMARY_WORDS), dtype=torch.int32, device=dev)
        ws = workspace if workspace is not None else torch.empty(
            (max(c._L.dagpu_square_units_workspace_size(k, n), 16),), dtype=torch.uint8, device=dev)
    host = np.zeros((n, _abi.UNITS_SUMMARY_WORDS), np.int32) if summary_host else None
    rc = c._L.dagpu_square_units_device(c.handle, k, n, _abi.addr(squares), square_stride, row_pitch, seq_cap,
                                        _abi.addr(records), _abi.addr(summary), cap, _abi.addr(units),
                                        _abi.addr(unit_summary), _abi.addr(host), _abi.addr(ws), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return units[:, :cap], unit_summary, host


def read_units_device(k: int, squares: torch.Tensor, square_stride: int, row_pitch: int, records: torch.Tensor,
                      units: torch.Tensor, unit_summary: torch.Tensor, pairs, payload_cap: int,
                      ctx: Optional[Context] = None, stream: Optional[torch.cuda.Stream] = None,
                      payload: Optional[torch.Tensor] = None):
    """dagpu_square_read_units_device: the data bytes of the units `pairs`
    ((m, 2) of {square, unit index}, on the host) names in unit_table_device's
    table, gathered into a cuda uint8 tensor of payload_cap bytes (`payload`,
    when given, is written in place).  Returns (offsets (m,) int64, totals (3,)
    int64 {m, payload_bytes, flags}, payload), all on the device and only
    enqueued on `stream`.  flags: _abi.READ_UNITS_OVERFLOW, and
    _abi.READ_UNITS_INVALID for a pair that names no unit of a square whose
    code is UNITS_OK (it yields length 0; the unit summary is on the device, so
    the library cannot refuse it up front)."""
    import numpy as np
    c = ctx or default_context()
    n, dev = _squares_held(k, squares, square_stride, row_pitch), squares.device
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint32).reshape(-1, 2))
    m = len(pairs)
    if units.dim() != 3 or units.shape[0] != n or units.shape[2] != _abi.UNIT_RECORD_BYTES \
            or not units.is_contiguous() or units.dtype != torch.uint8:
        raise ValueError("units must be the contiguous (n, unit_cap, 32) uint8 tensor of unit_table_device")
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        offsets = torch.empty((max(m, 1),), dtype=torch.int64, device=dev)
        totals = torch.empty((3,), dtype=torch.int64, device=dev)
        if payload is None:
            payload = torch.empty((max(int(payload_cap), 16),), dtype=torch.uint8, device=dev)
        ws = torch.empty((max(c._L.dagpu_square_read_units_workspace_size(m), 16),), dtype=torch.uint8, device=dev)
    rc = c._L.dagpu_square_read_units_device(c.handle, k, n, _abi.addr(squares), square_stride, row_pitch,
                                             int(records.shape[1]), _abi.addr(records), int(units.shape[1]),
                                             _abi.addr(units), _abi.addr(unit_summary), _abi.addr(pairs) if m else None,
                                             m, _abi.addr(offsets), _abi.addr(totals), _abi.addr(payload),
                                             int(payload_cap), _abi.addr(ws), _stream_handle(s))
    if rc != 0:
        raise DAError(rc, c.last_error())
    return offsets[:m], totals, payload


class DeviceSquares:
    """n squares of width k resident on one GPU.

    ods:  (n, k*k*512) uint8   eds: (n, 4k^2*512) uint8
    row_roots/col_roots: (n, 2k, 90)   dah: (n, 32)   status: (n,) int32
    """

    def __init__(self, k: int, n: int, device: int = 0, ctx: Optional[Context] = None,
                 with_ods: bool = True, in_place: bool = False):
        self.k, self.n = int(k), int(n)
        self.ctx = ctx or default_context()
        dev = torch.device("cuda", device)
        w = 2 * self.k
        # in_place: the ODS lives in Q0 of the EDS buffer itself (rows at the EDS
        # row pitch), the zero-copy input of dagpu_extend_batch_device (d_ods = NULL)
        self.in_place = bool(in_place)
        self.ods = (torch.empty((n, self.k * self.k * 512), dtype=torch.uint8, device=dev)
                    if with_ods and not in_place else None)
        self.eds = torch.empty((n, w * w * 512), dtype=torch.uint8, device=dev)
        self.row_roots = torch.empty((n, w, ROOT), dtype=torch.uint8, device=dev)
        self.col_roots = torch.empty((n, w, ROOT), dtype=torch.uint8, device=dev)
        self.dah = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        self.status = torch.zeros((n,), dtype=torch.int32, device=dev)
        ws = self.ctx._L.dagpu_workspace_size(self.k, self.n)
        self.workspace = torch.empty((ws,), dtype=torch.uint8, device=dev)
        # tensors of started repairs, held until their join (dagpu_repair_start:
        # the buffers must stay valid until the joined stream has passed the repair)
        self._held = {}
        # load_txs: each block's plan and the length of its packed txs, for
        # blob_table / check_commitments
        self._plans = None
        self._src_lens = None
        # load_txs(plan="device"): what the planner left in HBM (PlannedSquares), and
        # validate_blob_txs()'s (tx_status, block_status, expected) over it
        self._planned = self._validated = None
        # extend() / roots() have filled self.dah for the squares now loaded
        self._dah_ready = False
        # scan(): (records, summary, host summary, (buffer, square_stride, row_pitch))
        self._scan = None
        # proof_store(): the ProofStore of self.eds, until the squares change;
        # tx_table(): the unit table of the squares, for as long
        self._proof_store = self._tx_index = None

    def q0(self) -> torch.Tensor:
        """(n, k, k*512) view of Q0 inside the EDS buffer."""
        w = 2 * self.k
        return self.eds.view(self.n, w, w * 512)[:, :self.k, :self.k * 512]

    def load_ods(self, ods) -> None:
        """Copy n ODS (anything viewable as (n, k*k*512) uint8) to where extend()
        reads them: self.ods, or Q0 of the EDS when in_place."""
        self._proof_store = self._tx_index = None
        self._planned = self._validated = None
        self._dah_ready = False
        src = ods if isinstance(ods, torch.Tensor) else torch.from_numpy(ods)
        src = src.reshape(self.n, self.k, self.k * 512)
        if self.in_place:
            self.q0().copy_(src)
        else:
            self.ods.view(self.n, self.k, self.k * 512).copy_(src)

    def load_txs(self, blocks, stream: Optional[torch.cuda.Stream] = None, threads: int = 16,
                 max_square_size: Optional[int] = None, threshold: Optional[int] = None, plan: str = "host") -> None:
        """n blocks of raw txs (each a sequence of bytes) -> their squares where
        extend() reads them, with no ODS on the host: every block is planned on
        the host (square.plan_native's dagpu_square_plan, on a pool of at most
        16 threads), txs and plans are uploaded and dagpu_square_write_device
        writes self.ods, or Q0 of the EDS at the EDS row pitch when in_place.
        Raises ShareError as square.construct_native does, and DAError when a
        block's square width is not self.k (nothing is written then).

        plan="device": no layout on the host.  One upload of the packed batch,
        one dagpu_square_construct_device (classify, plan and write on the
        GPU), one read of n status words.  A block the planner rejects is
        planned again on the host (square.plan_native) to raise the same
        ShareError / DAError with the same message, and as on the host route a
        rejected block's error comes before any block's width error.  The one difference from
        the host route: the accepted blocks' squares have been written when a
        rejected block, or one of another width, raises.  The plans stay in HBM and are downloaded when
        blob_table() / check_commitments() first ask for them."""
        from concurrent.futures import ThreadPoolExecutor

        from . import square as sq
        if len(blocks) != self.n:
            raise ValueError(f"{self.n} blocks expected, got {len(blocks)}")
        self._proof_store = self._tx_index = None
        self._planned = self._validated = None
        self._dah_ready = False
        if self.ods is None and not self.in_place:
            raise ValueError("no ODS buffer: DeviceSquares(with_ods=False) takes its input through extend_from")
        m = sq.SQUARE_SIZE_UPPER_BOUND if max_square_size is None else max_square_size
        t = sq.SUBTREE_ROOT_THRESHOLD if threshold is None else threshold

        if plan == "device":
            return self._load_txs_device(blocks, stream, m, t, threads)
        if plan != "host":
            raise ValueError("plan is 'host' or 'device'")

        def plan_one(txs):
            buf, lens = sq._pack(txs)
            k, p = sq._plan_packed(buf, lens, len(txs), m, t)
            return k, p, buf[:int(lens.sum())]

        workers = max(1, min(16, int(threads), self.n))
        if workers == 1:
            planned = [plan_one(b) for b in blocks]
        else:
            with ThreadPoolExecutor(workers) as pool:
                planned = list(pool.map(plan_one, blocks))
        for i, (k, _, _) in enumerate(planned):
            if k != self.k:
                raise DAError(_abi.ERR_ARG, f"block {i} has square width {k}, these squares have width {self.k}")
        w = 2 * self.k
        out, stride, pitch = ((self.eds, w * w * 512, w * 512) if self.in_place
                              else (self.ods, self.k * self.k * 512, self.k * 512))
        write_squares_device(self.k, [p for _, p, _ in planned], [b for _, _, b in planned], out.view(-1), stride,
                             pitch, ctx=self.ctx, stream=stream)
        self._plans = [p for _, p, _ in planned]
        self._src_lens = [int(b.size) for _, _, b in planned]

    def _load_txs_device(self, blocks, stream, m: int, t: int, threads: int) -> None:
        from . import square as sq
        w = 2 * self.k
        out, stride, pitch = ((self.eds, w * w * 512, w * 512) if self.in_place
                              else (self.ods, self.k * self.k * 512, self.k * 512))
        self._plans = self._src_lens = None
        p = construct_squares_device(self.k, blocks, out.view(-1), stride, pitch, max_square_size=m, threshold=t,
                                     ctx=self.ctx, stream=stream, threads=threads)
        words = [sq.plan_status(v) + (int(v),) for v in p.status_host()]
        # the host route plans every block before it looks at any width: a
        # rejected block's error comes before any block's width error
        for i, (kind, _, word) in enumerate(words):
            if kind and kind != _abi.PLAN_WIDTH:
                sq.plan_native(blocks[i], m, t)  # raises the host's error for this block
                raise DAError(_abi.ERR_ARG, f"block {i}: the device planner's status {word} where the host "
                                            f"planner accepts the block")
        for i, (kind, index, _) in enumerate(words):
            if kind == _abi.PLAN_WIDTH:
                raise DAError(_abi.ERR_ARG, f"block {i} has square width {index}, these squares have width {self.k}")
        self._plans = p  # downloaded by _host_plans when first asked for
        self._src_lens = p.src_lens
        self._planned = p

    def _host_plans(self):
        if isinstance(self._plans, PlannedSquares):
            self._plans = self._plans.plans_host()
        return self._plans

    def blob_table(self):
        """Every blob of the batch load_txs wrote, block by block in plan order:
        (records, keys), records the (nblobs, 3) int64 {square, first_share,
        share_count} that blob_commitments_device takes, keys the (nblobs, 2)
        int64 {block, data_off}, data_off the offset of the blob's data in the
        block's packed txs (square.plan_blobs)."""
        import numpy as np

        from . import square as sq
        if self._plans is None:
            raise ValueError("no plans: blob_table follows load_txs")
        rec, key = [], []
        for i, p in enumerate(self._host_plans()):
            t = sq.plan_blobs(p).astype(np.int64)
            rec.append(np.stack([np.full(len(t), i, np.int64), t[:, 0], t[:, 1]], axis=1))
            key.append(np.stack([np.full(len(t), i, np.int64), t[:, 2]], axis=1))
        return np.concatenate(rec).reshape(-1, 3), np.concatenate(key).reshape(-1, 2)

    def check_commitments(self, expected=None, stream: Optional[torch.cuda.Stream] = None,
                          threshold: Optional[int] = None):
        """The share commitment of every blob of the batch from the squares
        load_txs wrote (the ODS, or Q0 of the EDS when in_place: before or after
        extend(), which never changes Q0), compared on the device with
        `expected` ((nblobs, 32), in blob_table order) when given.  Returns
        blob_commitments_device's (commitments, status, square_status), enqueued
        on `stream`: one read of square_status tells which blocks to reject.
        expected="declared": the table validate_blob_txs() filled on the device
        from the blocks' MsgPayForBlobs (it runs first if it has not run)."""
        from . import square as sq
        if isinstance(expected, str):
            if expected != "declared":
                raise ValueError("expected is a (nblobs, 32) table, None or 'declared'")
            expected = (self._validated or self.validate_blob_txs(stream=stream))[2]
        rec, _ = self.blob_table()
        w = 2 * self.k
        buf, stride, pitch = ((self.eds, w * w * 512, w * 512) if self.in_place
                              else (self.ods, self.k * self.k * 512, self.k * 512))
        return blob_commitments_device(self.k, rec, buf.view(-1), stride, pitch, expected=expected,
                                       threshold=sq.SUBTREE_ROOT_THRESHOLD if threshold is None else threshold,
                                       ctx=self.ctx, stream=stream)

    # ---- ValidateBlobTx (dagpu_blob_tx_validate_device) and ProcessProposal's verdict ----

    def validate_blob_txs(self, stream: Optional[torch.cuda.Stream] = None):
        """The stateless rules of ValidateBlobTx over every tx of the batch
        load_txs(plan="device") left in HBM, and the commitments their
        MsgPayForBlobs declare in blob_table() order: validate_blob_txs_device's
        (tx_status, block_status, expected), enqueued on `stream` and kept for
        check_commitments(expected="declared") / process_proposals()."""
        if self._planned is None:
            raise ValueError("the txs are not resident in HBM: validate_blob_txs follows load_txs(plan='device'); "
                             "the host-plan route uploads no raw txs the device could walk")
        self._validated = validate_blob_txs_device(self._planned, ctx=self.ctx, stream=stream)
        return self._validated

    def verify_signatures(self, chain_id, account_numbers, pubkeys=None,
                          stream: Optional[torch.cuda.Stream] = None):
        """The tx signatures of the batch load_txs(plan="device") or
        process_blocks left in HBM: verify_tx_signatures_device's (tx_status,
        block_status, signers), enqueued on `stream`.  account_numbers (and
        pubkeys, the accounts' stored keys) hold one entry per tx in batch
        order.  It reads the raw txs only: the squares, the verdicts and
        every other result of the batch stay as they are."""
        if self._planned is None:
            raise ValueError("the txs are not resident in HBM: verify_signatures follows load_txs(plan='device') "
                             "or process_blocks")
        return verify_tx_signatures_device(self._planned, chain_id, account_numbers, pubkeys=pubkeys, ctx=self.ctx,
                                           stream=stream)

    def process_proposals(self, data_hashes=None, stream: Optional[torch.cuda.Stream] = None):
        """The data-parallel part of ProcessProposal (app/process_proposal.go:53-164)
        for every block of the batch: [(accept, reason)], reason "" for an
        accepted block.  Composes the planner's status, validate_blob_txs()'s
        block words and check_commitments(expected="declared")'s square status
        (each runs here if it has not), and, when data_hashes ((n, 32) bytes)
        is given, extend()'s / roots()'s data roots against them; the
        per-block words come back in one read.  A block's first reason in this
        order is reported, with the reference's log strings; the reference
        would name the tx of a commitment mismatch, which the square status
        does not carry.  Signatures, the ante handler and upgrade messages are
        not checked."""
        import numpy as np

        from . import blobtx as btx
        s = stream if stream is not None else torch.cuda.current_stream(self.eds.device)
        if self._planned is None:
            raise ValueError("the txs are not resident in HBM: process_proposals follows load_txs(plan='device')")
        _, block_status, _ = self._validated or self.validate_blob_txs(stream=s)
        _, _, sq_status = self.check_commitments(expected="declared", stream=s)
        with torch.cuda.stream(s):
            words = [self._planned.status[:self.n].view(self.n, 1), block_status, sq_status[:self.n].view(self.n, 1)]
            if data_hashes is not None:
                if not self._dah_ready:
                    raise ValueError("data_hashes given before extend() or roots() computed the data roots")
                want = np.frombuffer(b"".join(bytes(h) for h in data_hashes), np.uint8).copy()
                if want.size != 32 * self.n:
                    raise ValueError("data_hashes holds 32 bytes per block")
                want = torch.from_numpy(want.reshape(self.n, 32)).to(self.dah.device, non_blocking=True)
                words.append((self.dah != want).any(dim=1).to(torch.int32).view(self.n, 1))
            host = torch.cat(words, dim=1).cpu().numpy().view(np.uint32)
        pfb_kind = btx.KIND_NAMES.index("NON_BLOB_TX_HAS_PFB")
        out = []
        for plan, tx, word, commit, *root in host.tolist():
            if plan:
                out.append((False, "failure to compute data square from transactions:"))
            elif tx != _abi.BLOBTX_NONE and word & 0xFF == pfb_kind:
                out.append((False, f"tx {tx} has PFB but is not a blob tx"))
            elif tx != _abi.BLOBTX_NONE:
                out.append((False, f"invalid blob tx {tx}: {btx.error_name(word & 0xFF)}"))
            elif commit & _abi.COMMIT_PUSH_ORDER:
                out.append((False, "invalid blob tx: ErrCalculateCommitment"))
            elif commit & _abi.COMMIT_MISMATCH:
                out.append((False, "invalid blob tx: ErrInvalidShareCommitment"))
            elif root and root[0]:
                out.append((False, "proposed data root differs from calculated data root"))
            else:
                out.append((True, ""))
        return out

    def process_blocks(self, blocks, data_hashes=None, square_sizes=None,
                       stream: Optional[torch.cuda.Stream] = None, threads: int = 16):
        """ProcessProposal's data-parallel part (app/process_proposal.go:53-164)
        for n blocks of raw txs as upload, enqueue and one read: the planner and
        the square writer (construct_squares_device, its status not read),
        proposal_check_device, extend(), proposal_verdict_device, then one
        .cpu() of the n x 4 verdict words.  Returns [(accept, reason)] with the
        reference's log strings in the reference's order (da.verdict_reason;
        da.process_proposal is the readable mirror); the raw records stay in
        self.verdicts ((n, 4) uint32 {code, tx, word, aux}, _abi.VERDICT_NAMES)
        and the check's tensors in self.proposal_check.  Nothing a proposer can
        put into a block raises: a block the planner rejects, or one of
        another width (NOT_JUDGED, never an accept), has its record.  The
        plans stay in HBM for tx_table(), proof_store() and the other
        follow-ups; nothing else is downloaded."""
        import numpy as np

        from . import da as _da, square as sq
        if len(blocks) != self.n:
            raise ValueError(f"{self.n} blocks expected, got {len(blocks)}")
        if self.ods is None and not self.in_place:
            raise ValueError("no ODS buffer: DeviceSquares(with_ods=False) takes its input through extend_from")
        self._proof_store = self._tx_index = None
        self._planned = self._validated = None
        self._plans = self._src_lens = None
        self._dah_ready = False
        s = stream if stream is not None else torch.cuda.current_stream(self.eds.device)
        w = 2 * self.k
        out, stride, pitch = ((self.eds, w * w * 512, w * 512) if self.in_place
                              else (self.ods, self.k * self.k * 512, self.k * 512))
        p = construct_squares_device(self.k, blocks, out.view(-1), stride, pitch,
                                     max_square_size=sq.SQUARE_SIZE_UPPER_BOUND, threshold=sq.SUBTREE_ROOT_THRESHOLD,
                                     ctx=self.ctx, stream=s, threads=threads)
        check = proposal_check_device(p, self.k, out.view(-1), stride, pitch, threshold=sq.SUBTREE_ROOT_THRESHOLD,
                                      ctx=self.ctx, stream=s)
        self.extend(stream=s)
        verdicts = proposal_verdict_device(p, self.k, check, extend_status=self.status, dah=self.dah,
                                           data_hashes=data_hashes, square_sizes=square_sizes, ctx=self.ctx, stream=s)
        with torch.cuda.stream(s):
            self.verdicts = verdicts.cpu().numpy().view(np.uint32)
        self.proposal_check = check
        self._plans = p
        self._src_lens = p.src_lens
        self._planned = p
        return [(int(v[0]) == 0, _da.verdict_reason(*(int(x) for x in v))) for v in self.verdicts]

    # ---- square read (dagpu_square_scan_device / dagpu_square_read_device) ----

    def _resident(self, from_eds: Optional[bool] = None):
        """(buffer, square_stride, row_pitch) of the squares: Q0 of the EDS when
        in_place, when there is no ODS buffer or when from_eds is set (after a
        repair the content is there), else the ODS batch."""
        w = 2 * self.k
        if self.in_place or self.ods is None or from_eds:
            return self.eds.view(-1), w * w * 512, w * 512
        return self.ods.view(-1), self.k * self.k * 512, self.k * 512

    def _fetch(self, i: int, where):
        """fetch(first, end) -> List[Share] of square i, downloaded row by row."""
        from .shares import Share
        buf, stride, pitch = where
        k = self.k

        def fetch(a, b):
            b = min(b, k * k)
            if a >= b:
                return []
            r0, r1 = a // k, (b - 1) // k
            rows = [buf[i * stride + r * pitch:i * stride + r * pitch + k * 512].cpu().numpy().tobytes()
                    for r in range(r0, r1 + 1)]
            flat = b"".join(rows)
            return [Share(flat[(s - r0 * k) * 512:(s - r0 * k + 1) * 512]) for s in range(a, b)]
        return fetch

    def scan(self, stream: Optional[torch.cuda.Stream] = None, from_eds: Optional[bool] = None,
             seq_cap: Optional[int] = None, check: bool = True):
        """shares.ParseShares of every square where it lies (dagpu_square_scan_device);
        the records and summary stay on the device (self._scan).  Returns the (n, 8) int32 summary on the host.  With
        check, a square the reference refuses raises ShareError with the
        mirror's message: the mirror runs on the offending share or sequence
        alone, downloaded."""
        import numpy as np

        from . import square as sq
        where = self._resident(from_eds)
        records, summary, host = scan_squares_device(self.k, where[0], where[1], where[2], seq_cap=seq_cap,
                                                     ctx=self.ctx, stream=stream)
        records, summary, host = records[:self.n], summary[:self.n], host[:self.n]
        self._scan = (records, summary, host, where)
        if check:
            for i in range(self.n):
                if host[i, 0] != _abi.SCAN_OK:
                    cap = int(records.shape[1])
                    rec = records[i, :min(int(host[i, 3]), cap)].cpu().numpy().view(sq.seq_dtype()).reshape(-1)
                    sq.raise_scan_error(host[i], np.ascontiguousarray(rec), self._fetch(i, where))
        return host

    def _parsed(self, classes: int, namespaces=None, stream: Optional[torch.cuda.Stream] = None,
                from_eds: Optional[bool] = None):
        """One square.ParsedSquare per square over a fresh scan: the payload of
        the sequences of `classes` / `namespaces` gathered in HBM and
        downloaded, nothing else.  A square the reference refuses raises when
        its ParsedSquare is asked for content."""
        import numpy as np

        from . import square as sq
        self.scan(stream=stream, from_eds=from_eds, check=False)
        records, summary, host, where = self._scan
        ok = host[:, 0] == _abi.SCAN_OK
        need = 0
        if classes & _abi.READ_BLOBS:
            need += int(host[ok, 5].astype(np.int64).sum())
        if classes & _abi.READ_COMPACT:
            need += int(host[ok, 6].astype(np.int64).sum())
        cap = int(records.shape[1])
        selected, offsets, totals, payload = read_sequences_device(
            self.k, where[0], where[1], where[2], records, summary, need, namespaces=namespaces, classes=classes,
            ctx=self.ctx, stream=stream)
        s = stream if stream is not None else torch.cuda.current_stream(self.eds.device)
        with torch.cuda.stream(s):
            nsel, nbytes, over = (int(v) for v in totals.cpu())
            assert not over, "the payload buffer was sized from the summary"
            slots = selected[:nsel].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            offs = offsets[:nsel].cpu().numpy()
            data = payload[:nbytes].cpu().numpy()
            top = max(1, int(host[:, 3].clip(max=cap).max()))
            rec = np.ascontiguousarray(records[:, :top].cpu().numpy()).view(sq.seq_dtype()).reshape(self.n, top)
        at = {int(slot): int(off) for slot, off in zip(slots, offs)}
        out = []
        for i in range(self.n):
            r = rec[i, :min(int(host[i, 3]), cap)]

            def get(j, i=i, r=r):
                o = at[i * cap + j]
                return data[o:o + int(r["payload"][j])].tobytes()
            out.append(sq.ParsedSquare(self.k, r, host[i], get, self._fetch(i, where)))
        return out

    def read_blobs(self, namespaces=None, stream: Optional[torch.cuda.Stream] = None,
                   from_eds: Optional[bool] = None):
        """Every square's blobs (of `namespaces`, 29-byte values; all by
        default) as shares.parse_blobs returns them: a List[Blob] per square.
        Only the blobs' bytes cross PCIe."""
        return [p.blobs(namespaces) for p in self._parsed(_abi.READ_BLOBS, namespaces, stream, from_eds)]

    def read_txs(self, stream: Optional[torch.cuda.Stream] = None, from_eds: Optional[bool] = None):
        """Per square (txs, wrapped PFBs): shares.parse_txs of the tx namespace's
        and of the PFB namespace's shares."""
        return [(p.txs(), p.wrapped_pfbs()) for p in self._parsed(_abi.READ_COMPACT, None, stream, from_eds)]

    def deconstruct(self, pfb_blob_sizes, stream: Optional[torch.cuda.Stream] = None,
                    from_eds: Optional[bool] = None):
        """square.Deconstruct of every square: the List of its txs, BlobTxs
        re-assembled (square.ParsedSquare.deconstruct over the gathered payload;
        pfb_blob_sizes(tx) -> the blob sizes of a PFB, as square.deconstruct
        takes it)."""
        return [p.deconstruct(pfb_blob_sizes)
                for p in self._parsed(_abi.READ_BLOBS | _abi.READ_COMPACT, None, stream, from_eds)]

    # ---- tx index (dagpu_square_units_device / dagpu_square_read_units_device) ----

    def tx_table(self, stream: Optional[torch.cuda.Stream] = None, from_eds: Optional[bool] = None):
        """Where every tx and wrapped PFB of every square lies: scan(), then
        dagpu_square_units_device over its records; kept until the squares
        change.  Returns (units, summary): units an (n, top) host array of
        square.unit_dtype(), row i holding square i's summary[i, 2] units in
        block tx order (txs, then PFBs: the index NewTxInclusionProof takes),
        zero past them; summary the (n, 8) int32 unit summaries.  A square the
        device hands to the host (UNITS_HOST) is downloaded and answered by the
        host executor, dagpu_square_units_host, which raises ShareError with the
        reference's message where parse_txs fails; its summary row is then the
        host executor's.  A square with a scan error raises as scan() does."""
        import numpy as np

        from . import square as sq
        if self._tx_index is not None and self._tx_index["from_eds"] == bool(from_eds):
            return self._tx_index["units"], self._tx_index["summary"]
        scan = self.scan(stream=stream, from_eds=from_eds)
        records, summary, _, where = self._scan
        s = stream if stream is not None else torch.cuda.current_stream(self.eds.device)
        # a unit takes two bytes at least; four to a share is far above what blocks hold: a
        # square with more overflows and is indexed again at its true count
        cap = max(1, int(np.minimum(scan[:, 6] // 2 + 1, 4 * (scan[:, 6] // 474 + 1)).max()))
        d_units, d_summary, host = unit_table_device(self.k, where[0], where[1], where[2], records, summary, cap,
                                                     ctx=self.ctx, stream=s)
        over = host[:, 0] == _abi.UNITS_OVERFLOW
        if over.any():
            cap = int(host[over, 1].max())
            d_units, d_summary, host = unit_table_device(self.k, where[0], where[1], where[2], records, summary, cap,
                                                         ctx=self.ctx, stream=s)
        d_units, d_summary, host = d_units[:self.n].contiguous(), d_summary[:self.n], host[:self.n].copy()
        top = max(1, int(host[:, 2].max()))
        with torch.cuda.stream(s):
            units = np.ascontiguousarray(d_units[:, :top].cpu().numpy()).view(sq.unit_dtype()).reshape(self.n, top)
        units = units.copy()
        on_host = {}
        for i in np.nonzero(host[:, 0] == _abi.UNITS_HOST)[0]:
            i = int(i)
            buf, stride, pitch = where
            with torch.cuda.stream(s):
                ods = buf[i * stride:i * stride + (self.k - 1) * pitch + self.k * 512].cpu().numpy()
                rec = records[i].cpu().numpy().view(sq.seq_dtype()).reshape(-1)
            u, sm = sq.units_native(ods, self.k, records=rec, scan=scan[i], row_pitch=pitch)
            if len(u) > units.shape[1]:
                units = np.concatenate([units, np.zeros((self.n, len(u) - units.shape[1]), units.dtype)], axis=1)
            units[i] = 0
            units[i, :len(u)] = u
            host[i] = sm
            on_host[i] = (ods, rec, pitch)
        for i in range(self.n):
            units[i, int(host[i, 2]):] = 0
        self._tx_index = {"from_eds": bool(from_eds), "units": units, "summary": host, "d_units": d_units,
                          "d_summary": d_summary, "on_host": on_host, "records": records, "where": where}
        return units, host

    def tx_ranges(self, stream: Optional[torch.cuda.Stream] = None, from_eds: Optional[bool] = None):
        """Per square the list of (start, end) share ranges of its units in
        block tx order: Builder.FindTxShareRange of every tx index."""
        units, summary = self.tx_table(stream, from_eds)
        return [[(int(u["start_share"]), int(u["end_share"])) for u in units[i, :int(summary[i, 2])]]
                for i in range(self.n)]

    def _tx_units(self, pairs, stream, from_eds=None):
        """The table's records of (square, tx index) pairs, checked as NewTxInclusionProof checks the index."""
        units, summary = self.tx_table(stream, from_eds)
        pairs = [(int(a), int(b)) for a, b in pairs]
        for i, t in pairs:
            if not 0 <= i < self.n:
                raise ValueError(f"square {i} of {self.n}")
            if not 0 <= t < int(summary[i, 2]):
                raise DAError(_abi.ERR_ARG, f"txIndex {t} out of bounds")
        return pairs, [units[i, t] for i, t in pairs]

    def read_tx_units(self, pairs, stream: Optional[torch.cuda.Stream] = None, from_eds: Optional[bool] = None):
        """The bytes of the txs named by (square, tx index) pairs, a PFB as its
        wrapped IndexWrapper bytes (what shares.parse_txs returns): gathered in
        HBM straight from the table (dagpu_square_read_units_device), one
        download of just those bytes.  The host holds the unit summaries, so an
        index past a square's units raises DAError(ERR_ARG, "txIndex N out of
        bounds") before anything runs; units of a square the host executor
        answered are cut from that square's download."""
        import numpy as np

        from . import square as sq
        pairs, recs = self._tx_units(pairs, stream, from_eds)
        ix = self._tx_index
        out = [None] * len(pairs)
        dev = [j for j, (i, _) in enumerate(pairs) if i not in ix["on_host"]]
        for j, (i, _) in enumerate(pairs):
            if i in ix["on_host"]:
                ods, rec, pitch = ix["on_host"][i]
                out[j] = sq.unit_bytes(ods, self.k, pitch, rec, recs[j])
        if dev:
            records, where = ix["records"], ix["where"]
            need = sum((int(recs[j]["len"]) + 15) & ~15 for j in dev)
            s = stream if stream is not None else torch.cuda.current_stream(self.eds.device)
            offsets, totals, payload = read_units_device(
                self.k, where[0], where[1], where[2], records, ix["d_units"], ix["d_summary"],
                [pairs[j] for j in dev], need, ctx=self.ctx, stream=s)
            with torch.cuda.stream(s):
                flat = torch.cat([totals.view(torch.uint8), offsets.view(torch.uint8), payload[:need]]).cpu().numpy()
            m = len(dev)
            tot, offs, data = flat[:24].view(np.int64), flat[24:24 + 8 * m].view(np.int64), flat[24 + 8 * m:]
            assert int(tot[2]) == 0 and int(tot[1]) == need, "the pairs were checked against the summaries"
            for j, o in zip(dev, offs):
                out[j] = data[int(o):int(o) + int(recs[j]["len"])].tobytes()
        return out

    def tx_proofs(self, pairs, stream: Optional[torch.cuda.Stream] = None):
        """proof.NewTxInclusionProof (pkg/proof/proof.go:23-45) for (square, tx
        index) pairs spread over the batch: share_proofs over the table's share
        ranges, in the tx namespace, or the PFB namespace for a PFB; each equals
        proof.new_tx_inclusion_proof(block's txs, index) field for field.  One
        produce call and one download for the list; no square is rebuilt.  An
        index past a square's units raises DAError(ERR_ARG, "txIndex N out of
        bounds")."""
        from . import shares as sh
        pairs, recs = self._tx_units(pairs, stream)
        ranges = [(i, int(u["start_share"]), int(u["end_share"])) for (i, _), u in zip(pairs, recs)]
        ns = [sh.PAY_FOR_BLOB_NAMESPACE if int(u["flags"]) & _abi.SEQ_PFB else sh.TX_NAMESPACE for u in recs]
        return self.share_proofs(ranges, namespaces=ns, stream=stream)

    # ---- share proofs to the data root (dagpu_proof_store_device / dagpu_nmt_prove_squares_device) ----

    def proof_store(self, stream: Optional[torch.cuda.Stream] = None) -> ProofStore:
        """The ProofStore of self.eds: built once (enqueued on `stream`) and
        kept until extend*, repair*, load_ods or load_txs change the squares."""
        if self._proof_store is None:
            self._proof_store = ProofStore(self.k, self.eds, ctx=self.ctx, stream=stream)
        return self._proof_store

    def share_proofs(self, ranges, namespaces=None, stream: Optional[torch.cuda.Stream] = None):
        """proof.NewShareInclusionProof (pkg/proof/proof.go:58-165) for a list
        of ranges = (square, start, end) of row-major ODS share indexes, spread
        over the batch: a List[proof.ShareProof], each equal field for field to
        proof.new_share_inclusion_proof of that square.  namespaces: one 29-B
        namespace per range; None takes the namespace of the range's first
        share, and a range whose shares carry different namespaces raises the
        DAError of proof.parse_namespace.  One produce call and one download for
        the whole list; nothing is hashed beyond the cached proof_store()."""
        import numpy as np

        from . import proof as pf
        ranges = [tuple(int(v) for v in r) for r in ranges]
        if namespaces is not None and len(namespaces) != len(ranges):
            raise ValueError("one namespace per range")
        if not ranges:
            return []
        req, span = share_proof_requests(self.k, self.n, ranges)
        store = self.proof_store(stream)
        s = stream if stream is not None else torch.cuda.current_stream(self.eds.device)
        out = nmt_prove_squares_device(store, req, shares=True, to_data_root=True, ctx=self.ctx, stream=s)
        parts = (out.nodes, out.shares, out.axis_roots, out.leaf_hashes, out.aunts)
        with torch.cuda.stream(s):
            host = torch.cat(parts).cpu().numpy().tobytes()
        at = np.cumsum([0] + [t.numel() for t in parts])
        nodes, cells, roots, hashes, aunts = (host[at[j]:at[j + 1]] for j in range(len(parts)))
        la = (4 * self.k).bit_length() - 1
        proofs = []
        for i, (_, start, end) in enumerate(ranges):
            rows = range(int(span[i]), int(span[i + 1]))
            d = out.desc[rows.start:rows.stop]
            data = [cells[512 * j:512 * (j + 1)] for j in range(int(d[0, 3]), int(d[-1, 3] + d[-1, 2]))]
            ns = pf.parse_namespace(data, 0, len(data)) if namespaces is None else bytes(namespaces[i])
            proofs.append(pf.ShareProof(
                data=data,
                share_proofs=[pf.NMTProof(int(q[0]), int(q[1]),
                                          [nodes[90 * j:90 * (j + 1)] for j in range(int(q[5]), int(q[5] + q[4]))])
                              for q in d],
                namespace_id=ns[1:],
                row_proof=pf.RowProof(
                    [roots[90 * r:90 * (r + 1)] for r in rows],
                    [pf.MerkleProof(4 * self.k, int(req[r, 2]), hashes[32 * r:32 * (r + 1)],
                                    [aunts[32 * (r * la + a):32 * (r * la + a + 1)] for a in range(la)])
                     for r in rows],
                    start // self.k, (end - 1) // self.k),
                namespace_version=ns[0]))
        return proofs

    def blob_proofs(self, rows=None, stream: Optional[torch.cuda.Stream] = None):
        """One proof.ShareProof per blob of blob_table() (or of its selected
        `rows`), to the data root of the blob's block: share_proofs over
        (square, first_share, first_share + share_count)."""
        rec, _ = self.blob_table()
        if rows is not None:
            rec = rec[list(rows)]
        return self.share_proofs([(int(sq), int(a), int(a + c)) for sq, a, c in rec], stream=stream)

    def namespace_proofs(self, namespaces, stream: Optional[torch.cuda.Stream] = None):
        """proof.prove_namespaces_squares over the cached proof_store():
        out[q][square] = list of (row, NMTProof, shares, MerkleProof) for every
        namespace of the list on every square of the batch."""
        from . import proof as pf
        return pf.prove_namespaces_squares(self.proof_store(stream), namespaces, stream=stream)

    def _ck(self, rc: int) -> None:
        if rc != 0:
            raise DAError(rc, self.ctx.last_error())

    def extend(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        """ODS -> EDS -> roots -> DAH, enqueued on `stream` (no sync)."""
        self._proof_store = self._tx_index = None
        self._dah_ready = True
        L = self.ctx._L
        self._ck(L.dagpu_extend_batch_device(
            self.ctx.handle, self.k, self.n, _abi.addr(self.ods), _abi.addr(self.eds),
            _abi.addr(self.row_roots), _abi.addr(self.col_roots), _abi.addr(self.dah),
            _abi.addr(self.status), _abi.addr(self.workspace), _stream_handle(stream)))

    def extend_from(self, ods: torch.Tensor, stream: Optional[torch.cuda.Stream] = None) -> int:
        """Extend the first m = ods.shape[0] (<= n) squares taking their ODS
        from `ods` ((m, k*k*512) uint8 on this device, e.g. a window of a
        resident block-replay shard) instead of self.ods.  Returns m."""
        m = int(ods.shape[0])
        if m > self.n or ods.dtype != torch.uint8 or ods.device != self.eds.device \
                or not ods.is_contiguous() or ods.numel() != m * self.k * self.k * 512:
            raise ValueError("ods must be a contiguous (m <= n, k*k*512) uint8 tensor on this device")
        self._proof_store = self._tx_index = None
        L = self.ctx._L
        self._ck(L.dagpu_extend_batch_device(
            self.ctx.handle, self.k, m, _abi.addr(ods), _abi.addr(self.eds),
            _abi.addr(self.row_roots), _abi.addr(self.col_roots), _abi.addr(self.dah),
            _abi.addr(self.status), _abi.addr(self.workspace), _stream_handle(stream)))
        return m

    def extend_rs(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        self._proof_store = self._tx_index = None
        self._ck(self.ctx._L.dagpu_extend_rs_device(
            self.ctx.handle, self.k, self.n, _abi.addr(self.ods), _abi.addr(self.eds),
            _stream_handle(stream)))

    def repair(self, present: torch.Tensor, status: torch.Tensor, workspace: torch.Tensor,
               stream: Optional[torch.cuda.Stream] = None, byz: Optional[torch.Tensor] = None) -> None:
        """Device-resident rsmt2d Repair of self.eds against self.row/col_roots.
        present: (n, (2k)^2) uint8, updated in place; status: (n,) int32;
        byz (optional): (n, 4) int32 on the device -> failing axis per square
        (dagpu_repair_batch_device_ex)."""
        self._proof_store = self._tx_index = None
        L = self.ctx._L
        if byz is None:
            self._ck(L.dagpu_repair_batch_device(
                self.ctx.handle, self.k, self.n, _abi.addr(self.eds), _abi.addr(present),
                _abi.addr(self.row_roots), _abi.addr(self.col_roots), _abi.addr(status),
                _abi.addr(workspace), _stream_handle(stream)))
            return
        if byz.dtype != torch.int32 or byz.numel() != 4 * self.n or byz.device != self.eds.device:
            raise ValueError("byz must be an (n, 4) int32 tensor on this device")
        self._ck(L.dagpu_repair_batch_device_ex(
            self.ctx.handle, self.k, self.n, _abi.addr(self.eds), _abi.addr(present),
            _abi.addr(self.row_roots), _abi.addr(self.col_roots), _abi.addr(status), _abi.addr(byz),
            _abi.addr(workspace), _stream_handle(stream)))

    def repair_start(self, present: torch.Tensor, status: torch.Tensor, workspace: torch.Tensor,
                     stream: Optional[torch.cuda.Stream] = None, first: int = 0, count: Optional[int] = None) -> int:
        """dagpu_repair_start on squares [first, first + count) (default all):
        returns at once with a handle for repair_join; the crossword runs on a
        library worker thread and stream forked from `stream`.  present /
        status / workspace as repair() (status and present indexed from
        `first`; workspace sized for `count` squares)."""
        import ctypes
        self._proof_store = self._tx_index = None
        count = self.n - first if count is None else count
        w = 2 * self.k
        h = ctypes.c_uint64(0)
        self._ck(self.ctx._L.dagpu_repair_start(
            self.ctx.handle, self.k, count, self.eds.data_ptr() + first * w * w * 512,
            present.data_ptr() + first * w * w, self.row_roots.data_ptr() + first * w * ROOT,
            self.col_roots.data_ptr() + first * w * ROOT, status.data_ptr() + 4 * first, workspace.data_ptr(),
            _stream_handle(stream), ctypes.byref(h)))
        # the repair runs on the library's stream: keep its tensors (a temporary
        # workspace included) out of the caching allocator until the join
        self._held[h.value] = (present, status, workspace)
        return h.value

    def repair_join(self, handle: int, stream: Optional[torch.cuda.Stream] = None) -> None:
        """dagpu_repair_join: `stream` waits for the started repair.  The tensors
        held since repair_start are released in `stream`'s order: record_stream
        makes the caching allocator wait for the work queued on the join stream
        (which includes the repair) before it reuses their blocks, whichever
        stream allocated them."""
        js = stream if stream is not None else torch.cuda.current_stream()
        self._proof_store = self._tx_index = None
        try:
            self._ck(self.ctx._L.dagpu_repair_join(self.ctx.handle, handle, int(js.cuda_stream)))
        finally:
            for t in self._held.pop(handle, ()):
                t.record_stream(js)

    def repair_workspace(self, count: Optional[int] = None) -> torch.Tensor:
        ws = self.ctx._L.dagpu_repair_workspace_size(self.k, self.n if count is None else count)
        return torch.empty((ws,), dtype=torch.uint8, device=self.eds.device)

    def roots(self, stream: Optional[torch.cuda.Stream] = None) -> None:
        self._dah_ready = True
        self._ck(self.ctx._L.dagpu_roots_device(
            self.ctx.handle, self.k, self.n, _abi.addr(self.eds), _abi.addr(self.row_roots),
            _abi.addr(self.col_roots), _abi.addr(self.dah), _abi.addr(self.status),
            _abi.addr(self.workspace), _stream_handle(stream)))
