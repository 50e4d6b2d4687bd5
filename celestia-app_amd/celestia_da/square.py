"""Original data square construction, host-side mirror of
pkg/square:

  Builder (NewBuilder, AppendTx, AppendBlobTx, Export, FindBlobStartingIndex,
      BlobShareLength, FindTxShareRange, GetWrappedPFB)  pkg/square/builder.go
  Build, Construct, Deconstruct, TxShareRange, BlobShareRange, Square,
      Size, EmptySquare, WriteSquare                     pkg/square/square.go
  inclusion.BlobMinSquareSize                            pkg/inclusion/blob_share_commitment_rules.go:76

The square this produces is the ODS the GPU path extends: `square_bytes()`
feeds `da.extend_shares` / `device.DeviceSquares`, and blob commitments can be
read back from the GPU-built EDS with `inclusion.get_commitment`.

`Deconstruct` needs the blob sizes of each PFB; the reference decodes the
cosmos-sdk tx (MsgPayForBlobs.BlobSizes) with a `TxDecoder` argument, and this
mirror takes the same role as a callable `pfb_blob_sizes(tx) -> list[int]`.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

from . import blobtx as btx
from . import shares as sh
from .inclusion import next_share_index
from .trees import subtree_width
from .shares import Blob, Range, Share, ShareError

# pkg/appconsts/v1: SquareSizeUpperBound 128, SubtreeRootThreshold 64;
# initial_consts.go: DefaultGovMaxSquareSize 64
SQUARE_SIZE_UPPER_BOUND = 128
SUBTREE_ROOT_THRESHOLD = 64
DEFAULT_GOV_MAX_SQUARE_SIZE = 64
LATEST_VERSION = 1


def square_size_upper_bound(app_version: int = LATEST_VERSION) -> int:
    return SQUARE_SIZE_UPPER_BOUND


def subtree_root_threshold(app_version: int = LATEST_VERSION) -> int:
    return SUBTREE_ROOT_THRESHOLD


def blob_min_square_size(share_count: int) -> int:
    return sh.round_up_power_of_two(int(math.ceil(math.sqrt(float(share_count)))))


def size(n_shares: int) -> int:
    """square.Size / da.SquareSize."""
    return sh.round_up_power_of_two(int(math.ceil(math.sqrt(float(n_shares)))))


class Square(list):
    """[]shares.Share."""

    def size(self) -> int:
        return size(len(self))

    def equals(self, other: Sequence[Share]) -> bool:
        return len(self) == len(other) and all(a.to_bytes() == b.to_bytes() for a, b in zip(self, other))

    def is_empty(self) -> bool:
        return self.equals(empty_square())

    def wrapped_pfbs(self) -> List[bytes]:
        r = sh.get_share_range_for_namespace(self, sh.PAY_FOR_BLOB_NAMESPACE)
        return sh.parse_txs(self[r.start:r.end])

    def square_bytes(self) -> List[bytes]:
        return sh.to_bytes(self)


def empty_square() -> Square:
    return Square(sh.tail_padding_shares(sh.MIN_SHARE_COUNT))


@dataclass
class Element:
    blob: Blob
    pfb_index: int
    blob_index: int
    num_shares: int
    max_padding: int

    def max_share_offset(self) -> int:
        return self.num_shares + self.max_padding


def _new_element(blob: Blob, pfb_index: int, blob_index: int, threshold: int) -> Element:
    n = sh.sparse_shares_needed(len(blob.data))
    return Element(blob, pfb_index, blob_index, n, subtree_width(n, threshold) - 1)


def _worst_case_share_indexes(blobs: int, app_version: int) -> List[int]:
    m = square_size_upper_bound(app_version)
    return [m * m] * blobs


class Builder:
    def __init__(self, max_square_size: int, app_version: int = LATEST_VERSION, *txs: bytes):
        if max_square_size <= 0:
            raise ShareError("max square size must be strictly positive")
        if not sh.is_power_of_two(max_square_size):
            raise ShareError("max square size must be a power of two")
        self.max_capacity = max_square_size * max_square_size
        self.current_size = 0
        self.txs: List[bytes] = []
        self.pfbs: List[btx.IndexWrapper] = []
        self.blobs: List[Element] = []
        self.tx_counter = sh.CompactShareCounter()
        self.pfb_counter = sh.CompactShareCounter()
        self.done = False
        self.subtree_root_threshold = subtree_root_threshold(app_version)
        self.app_version = app_version
        seen_blob_tx = False
        for idx, tx in enumerate(txs):
            blob_tx, is_blob = btx.unmarshal_blob_tx(tx)
            if is_blob:
                seen_blob_tx = True
                if not self.append_blob_tx(blob_tx):
                    raise ShareError(f"not enough space to append blob tx at index {idx}")
            else:
                if seen_blob_tx:
                    raise ShareError(f"normal tx at index {idx} can not be appended after blob tx")
                if not self.append_tx(tx):
                    raise ShareError(f"not enough space to append tx at index {idx}")

    def _can_fit(self, n: int) -> bool:
        return self.current_size + n <= self.max_capacity

    def append_tx(self, tx: bytes) -> bool:
        diff = self.tx_counter.add(len(tx))
        if self._can_fit(diff):
            self.txs.append(bytes(tx))
            self.current_size += diff
            self.done = False
            return True
        self.tx_counter.revert()
        return False

    def append_blob_tx(self, blob_tx: btx.BlobTx) -> bool:
        iw = btx.IndexWrapper(blob_tx.tx, _worst_case_share_indexes(len(blob_tx.blobs), self.app_version))
        pfb_diff = self.pfb_counter.add(iw.size())
        elems = [_new_element(b, len(self.pfbs), i, self.subtree_root_threshold) for i, b in enumerate(blob_tx.blobs)]
        max_blob_shares = sum(e.max_share_offset() for e in elems)
        if self._can_fit(pfb_diff + max_blob_shares):
            self.blobs.extend(elems)
            self.pfbs.append(iw)
            self.current_size += pfb_diff + max_blob_shares
            self.done = False
            return True
        self.pfb_counter.revert()
        return False

    def is_empty(self) -> bool:
        return self.tx_counter.size() == 0 and self.pfb_counter.size() == 0

    def export(self) -> Square:
        if self.is_empty():
            return empty_square()
        ss = blob_min_square_size(self.current_size)
        self.blobs.sort(key=lambda e: e.blob.namespace())  # stable, like sort.SliceStable
        tx_writer = sh.CompactShareSplitter(sh.TX_NAMESPACE, sh.SHARE_VERSION_ZERO)
        for tx in self.txs:
            tx_writer.write_tx(tx)
        non_reserved_start = self.tx_counter.size() + self.pfb_counter.size()
        cursor = end_of_last_blob = non_reserved_start
        blob_writer = sh.SparseShareSplitter()
        for i, e in enumerate(self.blobs):
            cursor = next_share_index(cursor, e.num_shares, self.subtree_root_threshold)
            if i == 0:
                non_reserved_start = cursor
            padding = cursor - end_of_last_blob
            if padding > e.max_padding:
                raise ShareError(f"blob has {padding} padding shares, but {e.max_padding} was the max possible")
            self.pfbs[e.pfb_index].share_indexes[e.blob_index] = cursor
            if i > 0:
                blob_writer.write_namespace_padding_shares(padding)
            blob_writer.write(e.blob)
            cursor += e.num_shares
            end_of_last_blob = cursor
        pfb_writer = sh.CompactShareSplitter(sh.PAY_FOR_BLOB_NAMESPACE, sh.SHARE_VERSION_ZERO)
        for iw in self.pfbs:
            pfb_writer.write_tx(iw.marshal())
        if self.pfb_counter.size() < pfb_writer.count():
            raise ShareError(f"pfbCounter.Size() < pfbTxWriter.Count(): {self.pfb_counter.size()} < "
                             f"{pfb_writer.count()}")
        square = write_square(tx_writer, pfb_writer, blob_writer, non_reserved_start, ss)
        self.done = True
        return square

    def _pfb_offset(self, pfb_index: int) -> int:
        if pfb_index < len(self.txs):
            raise ShareError(f"pfbIndex {pfb_index} does not match a pfb")
        pfb_index -= len(self.txs)
        if pfb_index >= len(self.pfbs):
            raise ShareError(f"pfbIndex {pfb_index} out of range")
        return pfb_index

    def find_blob_starting_index(self, pfb_index: int, blob_index: int) -> int:
        p = self._pfb_offset(pfb_index)
        if blob_index < 0:
            raise ShareError(f"blobIndex {blob_index} must not be negative")
        if not self.done:
            self.export()
        if blob_index >= len(self.pfbs[p].share_indexes):
            raise ShareError(f"blobIndex {blob_index} out of range")
        return self.pfbs[p].share_indexes[blob_index]

    def blob_share_length(self, pfb_index: int, blob_index: int) -> int:
        p = self._pfb_offset(pfb_index)
        if blob_index < 0:
            raise ShareError(f"blobIndex {blob_index} must not be negative")
        for e in self.blobs:
            if e.pfb_index == p and e.blob_index == blob_index:
                return e.num_shares
        raise ShareError("blob not found")

    def find_tx_share_range(self, tx_index: int) -> Range:
        if not self.done:
            self.export()
        if tx_index < 0:
            raise ShareError(f"txIndex {tx_index} must not be negative")
        if tx_index >= len(self.txs) + len(self.pfbs):
            raise ShareError(f"txIndex {tx_index} out of range")
        txw, pfw = sh.CompactShareCounter(), sh.CompactShareCounter()
        for i in range(tx_index):
            if i < len(self.txs):
                txw.add(len(self.txs[i]))
            else:
                pfw.add(self.pfbs[i - len(self.txs)].size())
        start = txw.size() + pfw.size() - 1
        if tx_index < len(self.txs):
            if txw.remainder == 0:
                start += 1
            txw.add(len(self.txs[tx_index]))
        else:
            if pfw.remainder == 0:
                start += 1
            pfw.add(self.pfbs[tx_index - len(self.txs)].size())
        return Range(start, txw.size() + pfw.size())

    def get_wrapped_pfb(self, tx_index: int) -> btx.IndexWrapper:
        if tx_index < 0:
            raise ShareError(f"txIndex {tx_index} must not be negative")
        if tx_index < len(self.txs):
            raise ShareError(f"txIndex {tx_index} does not match a pfb")
        if tx_index >= len(self.txs) + len(self.pfbs):
            raise ShareError(f"txIndex {tx_index} out of range")
        if not self.done:
            self.export()
        return self.pfbs[tx_index - len(self.txs)]

    def num_pfbs(self) -> int:
        return len(self.pfbs)

    def num_txs(self) -> int:
        return len(self.txs) + len(self.pfbs)


def write_square(tx_writer: sh.CompactShareSplitter, pfb_writer: sh.CompactShareSplitter,
                 blob_writer: sh.SparseShareSplitter, non_reserved_start: int, square_size: int) -> Square:
    total = square_size * square_size
    pfb_start = tx_writer.count()
    padding_start = pfb_start + pfb_writer.count()
    if non_reserved_start < padding_start:
        raise ShareError(f"nonReservedStart {non_reserved_start} is too small to fit all PFBs and txs")
    padding = sh.reserved_padding_shares(non_reserved_start - padding_start)
    end_of_last_blob = non_reserved_start + blob_writer.count()
    if total < end_of_last_blob:
        raise ShareError(f"square size {total} is too small to fit all blobs")
    tx_shares = tx_writer.export()
    pfb_shares = pfb_writer.export()
    square: List[Optional[Share]] = [None] * total
    square[0:len(tx_shares)] = tx_shares
    square[pfb_start:pfb_start + len(pfb_shares)] = pfb_shares
    if blob_writer.count() > 0:
        square[padding_start:padding_start + len(padding)] = padding
        bl = blob_writer.export()
        square[non_reserved_start:non_reserved_start + len(bl)] = bl
    if total > end_of_last_blob:
        tail = sh.tail_padding_shares(total - end_of_last_blob)
        square[end_of_last_blob:] = tail
    if any(s is None for s in square) or len(square) != total:
        # Go leaves zero-valued shares here; the layout rules above never do
        raise ShareError("square has unwritten shares")
    return Square(square)


def build(txs: Sequence[bytes], app_version: int = LATEST_VERSION,
          max_square_size: int = SQUARE_SIZE_UPPER_BOUND) -> Tuple[Square, List[bytes]]:
    """square.Build: the square and the txs that fit (normal txs first)."""
    b = Builder(max_square_size, app_version)
    normal, blob_txs = [], []
    for tx in txs:
        t, is_blob = btx.unmarshal_blob_tx(tx)
        if is_blob:
            if b.append_blob_tx(t):
                blob_txs.append(tx)
        elif b.append_tx(tx):
            normal.append(tx)
    return b.export(), normal + blob_txs


def construct(txs: Sequence[bytes], app_version: int = LATEST_VERSION,
              max_square_size: int = SQUARE_SIZE_UPPER_BOUND) -> Square:
    """square.Construct: every tx must fit, normal txs before blob txs."""
    return Builder(max_square_size, app_version, *txs).export()


def deconstruct(square: Sequence[Share], pfb_blob_sizes: Callable[[bytes], Sequence[int]]) -> List[bytes]:
    """square.Deconstruct: the txs (blob txs re-assembled from the square)."""
    sq = Square(square)
    if sq.is_empty():
        return []
    tr = sh.get_share_range_for_namespace(sq, sh.TX_NAMESPACE)
    if tr.start != 0:
        raise ShareError(f"expected txs to start at index 0, but got {tr.start}")
    wr = sh.get_share_range_for_namespace(sq[tr.end:], sh.PAY_FOR_BLOB_NAMESPACE)
    if wr.is_empty():
        return sh.parse_txs(sq[tr.start:tr.end])
    if wr.start != 0:
        raise ShareError(f"expected PFBs to start directly after non PFBs at index {tr.end}, but got {wr.start}")
    wr.add(tr.end)
    txs = sh.parse_txs(sq[tr.start:tr.end])
    for i, wb in enumerate(sh.parse_txs(sq[wr.start:wr.end])):
        iw, ok = btx.unmarshal_index_wrapper(wb)
        if not ok:
            raise ShareError(f"expected wrapped PFB at index {i}")
        if not iw.share_indexes:
            raise ShareError(f"wrapped PFB {i} has no blobs attached")
        sizes = list(pfb_blob_sizes(iw.tx))
        if len(sizes) != len(iw.share_indexes):
            raise ShareError(f"expected PFB to have {len(iw.share_indexes)} blob sizes, but got {len(sizes)}")
        blobs = []
        for j, si in enumerate(iw.share_indexes):
            parsed = sh.parse_blobs(sq[si:si + sh.sparse_shares_needed(sizes[j])])
            if len(parsed) != 1:
                raise ShareError(f"expected to parse a single blob, but got {len(parsed)}")
            blobs.append(parsed[0])
        txs.append(btx.marshal_blob_tx(iw.tx, *blobs))
    return txs


# ---- native construction (libdagpu: csrc/square.cpp, dagpu_square_construct/_build) ----------

def _pack(txs: Sequence[bytes]):
    import numpy as np
    lens = np.array([len(t) for t in txs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(bytes(t) for t in txs) or b"\x00", dtype=np.uint8).copy()
    return buf, lens


def _native(fn: str, txs, max_square_size: int, threshold: int, kept=None):
    import ctypes

    import numpy as np

    from . import _abi
    L = _abi.lib()
    buf, lens = _pack(txs)
    k = ctypes.c_uint32(0)
    cap = max(1, max_square_size) ** 2 * sh.SHARE_SIZE
    out = np.empty(cap, np.uint8)
    args = [None, _abi.addr(buf), _abi.addr(lens), len(txs), max_square_size, threshold, _abi.addr(out), cap,
            ctypes.addressof(k)]
    if kept is not None:
        args.append(_abi.addr(kept))
    rc = getattr(L, fn)(*args)
    if rc != 0:
        msg = L.dagpu_last_error(None).decode()
        raise ShareError(msg) if rc == _abi.ERR_SQUARE else ValueError(f"{fn}: status {rc}: {msg}")
    return int(k.value), out[:int(k.value) ** 2 * sh.SHARE_SIZE]


def construct_native(txs: Sequence[bytes], max_square_size: int = SQUARE_SIZE_UPPER_BOUND,
                     threshold: int = SUBTREE_ROOT_THRESHOLD):
    """square.Construct in the library's C++ (dagpu_square_construct): (k, ODS
    bytes as a (k*k*512,) uint8 array), byte-identical to construct(txs)."""
    return _native("dagpu_square_construct", txs, max_square_size, threshold)


def build_native(txs: Sequence[bytes], max_square_size: int = SQUARE_SIZE_UPPER_BOUND,
                 threshold: int = SUBTREE_ROOT_THRESHOLD):
    """square.Build in C++ (dagpu_square_build): (k, ODS bytes, kept txs in the
    order Build returns them: normal txs, then blob txs)."""
    import numpy as np
    kept = np.zeros(max(1, len(txs)), np.uint8)
    k, ods = _native("dagpu_square_build", txs, max_square_size, threshold, kept)
    normal = [t for i, t in enumerate(txs) if kept[i] and not btx.unmarshal_blob_tx(t)[1]]
    blob = [t for i, t in enumerate(txs) if kept[i] and btx.unmarshal_blob_tx(t)[1]]
    return k, ods, normal + blob


# ---- plan on the host, write on the device (csrc/square.cpp dagpu_square_plan,
# csrc/square_write.hip dagpu_square_write_device) -------------------------------

PLAN_GUESS = 64 << 10  # first plan buffer; a full 4,000-tx block needs ~0.2 MB and asks again


def _plan_packed(buf, lens, ntx: int, max_square_size: int, threshold: int, kept=None):
    """dagpu_square_plan on txs already packed (buf, lens): (k, plan as a uint8
    array).  Raises as _native does."""
    import ctypes

    import numpy as np

    from . import _abi
    L = _abi.lib()
    k, need = ctypes.c_uint32(0), ctypes.c_size_t(0)
    plan = np.empty(PLAN_GUESS, np.uint8)
    for _ in range(2):
        rc = L.dagpu_square_plan(None, _abi.addr(buf), _abi.addr(lens), ntx, max_square_size, threshold,
                                 _abi.addr(kept), _abi.addr(plan), plan.size, ctypes.addressof(need),
                                 ctypes.addressof(k))
        if rc == _abi.ERR_ARG and need.value > plan.size:
            plan = np.empty(need.value, np.uint8)  # the call reported the size
            continue
        break
    if rc != 0:
        msg = L.dagpu_last_error(None).decode()
        raise ShareError(msg) if rc == _abi.ERR_SQUARE else ValueError(f"dagpu_square_plan: status {rc}: {msg}")
    return int(k.value), plan[:need.value]


def plan_native(txs: Sequence[bytes], max_square_size: int = SQUARE_SIZE_UPPER_BOUND,
                threshold: int = SUBTREE_ROOT_THRESHOLD, build: bool = False):
    """The layout half of construct_native / build_native (dagpu_square_plan):
    (k, plan bytes) or, with build=True, (k, plan bytes, kept txs).  The plan
    refers to the txs packed back to back (b"".join(txs)); write_plan_host or
    construct_device turn it into the ODS.  Raises as construct_native does."""
    import numpy as np
    buf, lens = _pack(txs)
    if not build:
        return _plan_packed(buf, lens, len(txs), max_square_size, threshold)
    kept = np.zeros(max(1, len(txs)), np.uint8)
    k, plan = _plan_packed(buf, lens, len(txs), max_square_size, threshold, kept)
    normal = [t for i, t in enumerate(txs) if kept[i] and not btx.unmarshal_blob_tx(t)[1]]
    blob = [t for i, t in enumerate(txs) if kept[i] and btx.unmarshal_blob_tx(t)[1]]
    return k, plan, normal + blob


def plan_blobs(plan):
    """dagpu_square_plan_blobs: the blob table of a plan as an (nblob, 4) uint32
    array {first_share, share_count, data_off, data_len} in plan order
    (ascending first_share).  data_off is the offset of the blob's data in the
    block's packed txs.  Raises ValueError for a plan the check refuses."""
    import ctypes

    import numpy as np

    from . import _abi
    L = _abi.lib()
    plan = np.ascontiguousarray(plan, dtype=np.uint8)
    n = ctypes.c_size_t(0)
    rc = L.dagpu_square_plan_blobs(_abi.addr(plan), plan.size, None, 0, ctypes.byref(n))
    out = np.zeros((n.value, 4), np.uint32)
    if n.value:
        rc = L.dagpu_square_plan_blobs(_abi.addr(plan), plan.size, _abi.addr(out), n.value, ctypes.byref(n))
    if rc != 0:
        raise ValueError(f"dagpu_square_plan_blobs: status {rc}: {L.dagpu_last_error(None).decode()}")
    return out


def expected_commitments(txs: Sequence[bytes], plan):
    """The share commitments the block's PFBs declare, as an (nblob, 32) uint8
    array in plan order: each BlobTx's MsgPayForBlobs is decoded
    (blobtx.pfb_of_tx) and its blobs are tied to the plan's through the offset
    of their data in the packed txs.  Raises ShareError when a PFB's counts
    disagree with its blobs (ErrBlobSizeMismatch, ErrInvalidShareCommitments of
    x/blob/types/blob_tx.go) or a plan blob matches no blob of the txs."""
    import numpy as np
    declared = {}
    at = 0
    for raw in txs:
        raw = bytes(raw)
        t, ok = btx.unmarshal_blob_tx(raw)
        if ok:
            pfb = btx.pfb_of_tx(t.tx)
            if len(pfb.blob_sizes) != len(t.blobs):
                raise ShareError(f"ErrBlobSizeMismatch: actual {len(t.blobs)} declared {len(pfb.blob_sizes)}")
            if len(pfb.share_commitments) != len(t.blobs):
                raise ShareError(f"ErrInvalidShareCommitments: {len(pfb.share_commitments)} commitments for "
                                 f"{len(t.blobs)} blobs")
            for j, (off, ln) in enumerate(btx.blob_data_offsets(raw)):
                if pfb.blob_sizes[j] != ln:
                    raise ShareError(f"ErrBlobSizeMismatch: actual {ln} declared {pfb.blob_sizes[j]}")
                if len(pfb.share_commitments[j]) != 32:
                    raise ShareError(f"ErrInvalidShareCommitments: commitment {j} has "
                                     f"{len(pfb.share_commitments[j])} bytes")
                declared[at + off] = pfb.share_commitments[j]
        at += len(raw)
    table = plan_blobs(plan)
    out = np.zeros((len(table), 32), np.uint8)
    for i, row in enumerate(table):
        c = declared.get(int(row[2]))
        if c is None:
            raise ShareError(f"plan blob {i} (data at {int(row[2])}) is no blob of these txs")
        out[i] = np.frombuffer(c, np.uint8)
    return out


def write_plan_host(plan, txs: Sequence[bytes], k: int, row_pitch: Optional[int] = None, out=None):
    """dagpu_square_plan_write_host: the ODS of a plan and its txs, computed
    share by share with the function the kernel runs.  Returns `out` (a uint8
    array of k rows row_pitch bytes apart, default packed)."""
    import numpy as np

    from . import _abi
    L = _abi.lib()
    src = np.frombuffer(b"".join(bytes(t) for t in txs), np.uint8)
    pitch = k * sh.SHARE_SIZE if row_pitch is None else row_pitch
    if out is None:
        out = np.empty(k * pitch, np.uint8)
    plan = np.ascontiguousarray(plan, dtype=np.uint8)
    rc = L.dagpu_square_plan_write_host(_abi.addr(plan), plan.size, _abi.addr(src) if src.size else None, src.size,
                                        _abi.addr(out), pitch)
    if rc != 0:
        raise ValueError(f"dagpu_square_plan_write_host: status {rc}: {L.dagpu_last_error(None).decode()}")
    return out


def construct_device(txs: Sequence[bytes], device: int = 0, ctx=None,
                     max_square_size: int = SQUARE_SIZE_UPPER_BOUND, threshold: int = SUBTREE_ROOT_THRESHOLD):
    """square.Construct with the ODS assembled on the GPU: plan on the host,
    upload the raw txs and the plan, write the shares in HBM
    (dagpu_square_write_device).  Returns (k, ODS as a (k*k*512,) cuda uint8
    tensor), byte-identical to construct_native(txs)."""
    import torch

    from .device import write_squares_device
    k, plan = plan_native(txs, max_square_size, threshold)
    ods = torch.empty((k * k * sh.SHARE_SIZE,), dtype=torch.uint8, device=torch.device("cuda", device))
    write_squares_device(k, [plan], [b"".join(bytes(t) for t in txs)], ods, k * k * sh.SHARE_SIZE,
                         k * sh.SHARE_SIZE, ctx=ctx)
    return k, ods


# ---- plan on the device (csrc/square_plan.hip dagpu_square_plan_device; the
# same algorithm as host loops: dagpu_square_plan_emulate_host) ----------------

def plan_record_dtype():
    """One record of dagpu_square_plan_device per block."""
    import numpy as np
    return np.dtype([("plan_off", "<u8"), ("src_off", "<u8"), ("plan_bytes", "<u4"), ("k", "<u4"),
                     ("status", "<u4"), ("nblob", "<u4")])


def plan_status(word: int):
    """(kind, index) of a planner status word (_abi.PLAN_*)."""
    return int(word) & 0xFF, int(word) >> 8


def pack_blocks(blocks, lead: int = 0):
    """The planner's input for n blocks of txs: (src, src_offs, ntx, tx_lens):
    every tx of every block back to back behind `lead` unused bytes (uint8),
    the n + 1 block offsets (uint64), the tx count of each block (uint32) and
    all tx lengths (uint64)."""
    import numpy as np
    flat = [bytes(t) for b in blocks for t in b]
    src = np.frombuffer(bytes(lead) + b"".join(flat), np.uint8).copy()
    lens = np.array([len(t) for t in flat], np.uint64)
    ntx = np.array([len(b) for b in blocks], np.uint32)
    offs = np.zeros(len(blocks) + 1, np.uint64)
    at = lead
    for i, b in enumerate(blocks):
        offs[i] = at
        at += sum(len(t) for t in b)
    offs[len(blocks)] = at
    return src, offs, ntx, lens


def plan_of(arena, record):
    """The plan a record names, cut from the (host) arena; None for a rejected block."""
    if int(record["status"]) & 0xFF not in (0, 6) or int(record["plan_bytes"]) == 0:
        return None
    return arena[int(record["plan_off"]):int(record["plan_off"]) + int(record["plan_bytes"])]


def plan_emulate(blocks, max_square_size: int = SQUARE_SIZE_UPPER_BOUND, threshold: int = SUBTREE_ROOT_THRESHOLD):
    """dagpu_square_plan_emulate_host: the device planner's algorithm as host
    loops over n blocks of txs.  Returns (arena, records, status): the plan
    arena (uint8 array), one plan_record_dtype record and one status word per
    block; plan_of(arena, records[i]) equals plan_native(blocks[i])[1] for an
    accepted block, and status[i] is nonzero exactly when plan_native raises."""
    import numpy as np

    from . import _abi
    L = _abi.lib()
    n = len(blocks)
    src, offs, ntx, lens = pack_blocks(blocks)
    cap = L.dagpu_square_plan_device_arena_size(n, int(lens.size), max_square_size)
    arena = np.zeros(max(cap, 16), np.uint8)
    rec = np.zeros(max(n, 1), plan_record_dtype())
    status = np.zeros(max(n, 4), np.uint32)
    rc = L.dagpu_square_plan_emulate_host(n, _abi.addr(src) if src.size else None, _abi.addr(offs), src.size,
                                          _abi.addr(ntx), _abi.addr(lens) if lens.size else None, max_square_size,
                                          threshold, _abi.addr(arena), cap, _abi.addr(rec), _abi.addr(status))
    if rc != 0:
        raise ValueError(f"dagpu_square_plan_emulate_host: status {rc}: {L.dagpu_last_error(None).decode()}")
    return arena, rec[:n], status[:n]


def plan_device(blocks, max_square_size: int = SQUARE_SIZE_UPPER_BOUND, threshold: int = SUBTREE_ROOT_THRESHOLD,
                device: int = 0, ctx=None, stream=None):
    """dagpu_square_plan_device over n blocks of txs: one upload of the packed
    txs, the planner's kernels, no host layout.  Returns (arena, records,
    status): the plan arena as a cuda uint8 tensor, and the records and status
    words downloaded (numpy, as plan_emulate returns them)."""
    from .device import plan_squares_device
    p = plan_squares_device(blocks, max_square_size=max_square_size, threshold=threshold, device=device, ctx=ctx,
                            stream=stream)
    return p.arena, p.records_host(), p.status_host()


def tx_share_range(txs: Sequence[bytes], tx_index: int, app_version: int = LATEST_VERSION) -> Range:
    return Builder(square_size_upper_bound(app_version), app_version, *txs).find_tx_share_range(tx_index)


def blob_share_range(txs: Sequence[bytes], tx_index: int, blob_index: int,
                     app_version: int = LATEST_VERSION) -> Range:
    b = Builder(square_size_upper_bound(app_version), app_version, *txs)
    start = b.find_blob_starting_index(tx_index, blob_index)
    return Range(start, start + b.blob_share_length(tx_index, blob_index))


# ---- square read: sequences, blobs and tx streams back out of a square ------------------
# (csrc/square_read.hpp; dagpu_square_scan_host / dagpu_square_scan_device,
# dagpu_square_read_device, dagpu_compact_units).  The scan is shares.ParseShares,
# the units are parseRawData; the checks of Deconstruct are made on the records.

def seq_dtype():
    """numpy dtype of dagpu_seq_record (64 B)."""
    import numpy as np
    return np.dtype([("ns", "u1", 32), ("first", "<u4"), ("count", "<u4"), ("seq_len", "<u4"), ("flags", "<u4"),
                     ("reserved", "<u4"), ("payload", "<u4"), ("pad", "<u4", 2)])


def raise_scan_error(summary, records, fetch) -> None:
    """Raise what the mirror raises for a scan summary whose code is not OK:
    the mirror runs on the offending share or sequence alone, which
    fetch(first, end) -> List[Share] hands over (downloaded when the square is
    on the device).  Returns when the code is OK."""
    from . import _abi
    code, index = int(summary[0]), int(summary[1])
    if code == _abi.SCAN_OK:
        return
    if code == _abi.SCAN_OVERFLOW:
        raise ShareError(f"square has {index} share sequences, the record table holds {len(records)}")
    if code in (_abi.SCAN_NAMESPACE, _abi.SCAN_INCONSISTENT):
        sh.parse_shares(fetch(index, index + 1), False)
    else:
        at = int(records["first"].searchsorted(index))
        count = int(records["count"][at]) if at < len(records) and records["first"][at] == index else 1
        sh.parse_shares(fetch(index, index + count), False)
    raise ShareError(f"scan code {code} at share {index}, which the mirror accepts")


def compact_units(stream, reserved: int) -> List[bytes]:
    """dagpu_compact_units: the units of a compact sequence's payload, from its
    first share's reserved bytes on (shares.parse_txs of the sequence's shares)."""
    import ctypes

    import numpy as np

    from . import _abi
    L = _abi.lib()
    buf = np.frombuffer(stream, np.uint8) if not hasattr(stream, "ctypes") else np.ascontiguousarray(stream, np.uint8)
    cap = max(1, buf.size // 2)  # a unit takes two bytes at least, but for the last
    off, ln = np.empty(cap + 1, np.uint64), np.empty(cap + 1, np.uint64)
    n = ctypes.c_size_t(0)
    rc = L.dagpu_compact_units(_abi.addr(buf) if buf.size else None, buf.size, reserved, _abi.addr(off),
                               _abi.addr(ln), cap + 1, ctypes.byref(n))
    if rc != 0:
        msg = L.dagpu_last_error(None).decode()
        raise ShareError(msg) if rc == _abi.ERR_SQUARE else ValueError(f"dagpu_compact_units: status {rc}: {msg}")
    raw = buf.tobytes()
    return [raw[int(off[i]):int(off[i]) + int(ln[i])] for i in range(n.value)]


class ParsedSquare:
    """One scanned square: its sequence records (a structured array of
    seq_dtype(), in share order), its 8-word summary, and two callables that
    reach its bytes: payload(j) -> bytes of record j's payload, and
    fetch(first, end) -> List[Share].  Made by parse_native (host executor) and
    by DeviceSquares (the payloads gathered in HBM)."""

    def __init__(self, k: int, records, summary, payload, fetch):
        self.k, self.records, self.summary = int(k), records, summary
        self._payload, self._fetch = payload, fetch

    def check(self) -> None:
        raise_scan_error(self.summary, self.records, self._fetch)

    def sequences(self, flag: int):
        """Indices of the non-padding records with class flag `flag`."""
        from . import _abi
        f = self.records["flags"]
        return [int(j) for j in ((f & flag != 0) & (f & _abi.SEQ_PADDING == 0)).nonzero()[0]]

    def _all_shares(self):
        """The host route of a square with a share of another version, which
        parse_blobs / parse_txs refuse only inside the range they are given."""
        return self._fetch(0, self.k * self.k) if int(self.summary[2]) >= 0 else None

    def blobs(self, namespaces=None) -> List[Blob]:
        """shares.parse_blobs of the square's sparse shares (of the namespaces
        given, all by default)."""
        from . import _abi
        self.check()
        want = None if namespaces is None else {bytes(n) for n in namespaces}
        shares = self._all_shares()
        if shares is not None:
            return [b for b in sh.parse_blobs([s for s in shares if not s.is_compact_share()])
                    if want is None or b.namespace() in want]
        out = []
        for j in self.sequences(_abi.SEQ_SPARSE):
            ns = self.records["ns"][j][:sh.NAMESPACE_SIZE].tobytes()
            if want is None or ns in want:
                out.append(Blob.new(ns, self._payload(j), 0))
        return out

    def _units(self, flag: int) -> List[bytes]:
        from . import _abi
        self.check()
        shares = self._all_shares()
        if shares is not None:
            ns = sh.TX_NAMESPACE if flag == _abi.SEQ_TX else sh.PAY_FOR_BLOB_NAMESPACE
            return sh.parse_txs([s for s in shares if s.namespace() == ns])
        out = []
        for j in self.sequences(flag):
            out.extend(compact_units(self._payload(j), int(self.records["reserved"][j])))
        return out

    def txs(self) -> List[bytes]:
        """shares.parse_txs of the tx namespace's shares."""
        from . import _abi
        return self._units(_abi.SEQ_TX)

    def wrapped_pfbs(self) -> List[bytes]:
        """Square.wrapped_pfbs: shares.parse_txs of the PFB namespace's shares."""
        from . import _abi
        return self._units(_abi.SEQ_PFB)

    def _run(self, flag: int):
        """The records of one compact namespace as get_share_range_for_namespace
        sees its shares: (first record, number of records, share range), or None
        when no share has the namespace."""
        ns = sh.TX_NAMESPACE if flag == 2 else sh.PAY_FOR_BLOB_NAMESPACE
        idx = (self.records["flags"] & flag != 0).nonzero()[0]
        if len(idx) == 0:
            return None
        a, b = int(idx[0]), int(idx[-1])
        if b - a + 1 != len(idx):
            return a, len(idx), None  # not one run of shares: the host route
        r = self.records
        return a, len(idx), Range(int(r["first"][a]), int(r["first"][b] + r["count"][b]))

    def deconstruct(self, pfb_blob_sizes: Callable[[bytes], Sequence[int]]) -> List[bytes]:
        """square.deconstruct on the records: the same checks in the same order
        with the same messages.  A square that the records do not settle (a tx
        or PFB namespace of several sequences, a share of another version,
        shares out of namespace order, a share index that is not the first
        share of a blob of the declared size) takes the host route: its shares
        are fetched and square.deconstruct runs on them."""
        from . import _abi
        self.check()
        r, total = self.records, self.k * self.k

        def host_route():
            return deconstruct(self._fetch(0, total), pfb_blob_sizes)

        ns = [bytes(x[:sh.NAMESPACE_SIZE]) for x in r["ns"]]
        if int(self.summary[2]) >= 0 or self.k == 1 or any(a > b for a, b in zip(ns, ns[1:])):
            return host_route()
        tx, pfb = self._run(_abi.SEQ_TX), self._run(_abi.SEQ_PFB)
        for run in (tx, pfb):
            if run is not None and (run[1] != 1 or r["flags"][run[0]] & _abi.SEQ_PADDING):
                return host_route()
        tr = Range() if tx is None else tx[2]
        if tr.start != 0:
            raise ShareError(f"expected txs to start at index 0, but got {tr.start}")
        txs = [] if tx is None else compact_units(self._payload(tx[0]), int(r["reserved"][tx[0]]))
        if pfb is None:
            return txs
        if pfb[2].start != tr.end:
            raise ShareError(f"expected PFBs to start directly after non PFBs at index {tr.end}, but got "
                             f"{pfb[2].start - tr.end}")
        firsts = r["first"]
        for i, wb in enumerate(compact_units(self._payload(pfb[0]), int(r["reserved"][pfb[0]]))):
            iw, ok = btx.unmarshal_index_wrapper(wb)
            if not ok:
                raise ShareError(f"expected wrapped PFB at index {i}")
            if not iw.share_indexes:
                raise ShareError(f"wrapped PFB {i} has no blobs attached")
            sizes = list(pfb_blob_sizes(iw.tx))
            if len(sizes) != len(iw.share_indexes):
                raise ShareError(f"expected PFB to have {len(iw.share_indexes)} blob sizes, but got {len(sizes)}")
            blobs = []
            for j, si in enumerate(iw.share_indexes):
                at = int(firsts.searchsorted(si))
                if at >= len(r) or int(firsts[at]) != si or not r["flags"][at] & _abi.SEQ_SPARSE \
                        or r["flags"][at] & _abi.SEQ_PADDING \
                        or int(r["count"][at]) != sh.sparse_shares_needed(sizes[j]):
                    return host_route()
                blobs.append(Blob.new(ns[at], self._payload(at), 0))
            txs.append(btx.marshal_blob_tx(iw.tx, *blobs))
        return txs


def scan_native(ods, k: Optional[int] = None, seq_cap: Optional[int] = None, row_pitch: Optional[int] = None):
    """dagpu_square_scan_host of one square (a uint8 array, or a list of
    512-byte shares): (k, records[:min(n_sequences, seq_cap)], summary (8,)
    int32).  Raises nothing for a square the reference refuses: the summary
    tells."""
    import numpy as np

    from . import _abi
    L = _abi.lib()
    if not hasattr(ods, "dtype"):
        ods = np.frombuffer(b"".join(s.to_bytes() if isinstance(s, Share) else bytes(s) for s in ods), np.uint8)
    ods = np.ascontiguousarray(ods, np.uint8).reshape(-1)
    pitch = row_pitch
    if k is None:
        k = math.isqrt(ods.size // sh.SHARE_SIZE)
    if pitch is None:
        pitch = k * sh.SHARE_SIZE
    if ods.size < (k - 1) * pitch + k * sh.SHARE_SIZE:
        raise ValueError("ods holds less than one square of this width")
    cap = k * k if seq_cap is None else seq_cap
    rec = np.zeros(max(cap, 1), seq_dtype())
    summary = np.zeros(_abi.SCAN_SUMMARY_WORDS, np.int32)
    rc = L.dagpu_square_scan_host(k, 1, _abi.addr(ods), k * pitch, pitch, cap, _abi.addr(rec), _abi.addr(summary))
    if rc != 0:
        raise ValueError(f"dagpu_square_scan_host: status {rc}: {L.dagpu_last_error(None).decode()}")
    return k, rec[:min(int(summary[3]), cap)], summary


def parse_native(ods, k: Optional[int] = None) -> ParsedSquare:
    """One square on the host (a uint8 array of k*k*512 bytes, or a list of
    shares) scanned by the host executor: a ParsedSquare whose blobs(), txs(),
    wrapped_pfbs() and deconstruct() equal the mirror's parse_blobs, parse_txs
    and deconstruct of the same shares."""
    import numpy as np
    if not hasattr(ods, "dtype"):
        ods = np.frombuffer(b"".join(s.to_bytes() if isinstance(s, Share) else bytes(s) for s in ods), np.uint8)
    k, rec, summary = scan_native(ods, k)
    rows = np.ascontiguousarray(ods, np.uint8).reshape(k * k, sh.SHARE_SIZE)

    def payload(j):
        r = rec[j]
        first, count, n = int(r["first"]), int(r["count"]), int(r["payload"])
        head = 38 if r["flags"] & 6 else 34  # compact / sparse start share
        parts = [rows[first, head:]] + [rows[s, head - 4:] for s in range(first + 1, first + count)]
        return np.concatenate(parts)[:n].tobytes()

    def fetch(a, b):
        return [Share(rows[i].tobytes()) for i in range(a, min(b, k * k))]

    return ParsedSquare(k, rec, summary, payload, fetch)


def unit_dtype():
    """numpy dtype of dagpu_unit_record (32 B)."""
    import numpy as np
    return np.dtype([("start_share", "<u4"), ("end_share", "<u4"), ("seq", "<u4"), ("flags", "<u4"),
                     ("offset", "<u8"), ("len", "<u8")])


def units_native(ods, k: Optional[int] = None, unit_cap: Optional[int] = None, emulate: bool = False,
                 records=None, scan=None, row_pitch: Optional[int] = None):
    """The tx index of one host square (a uint8 array, or a list of shares):
    (units[:min(n_units, unit_cap)] of unit_dtype(), unit summary (8,) int32).
    By default the host executor, dagpu_square_units_host: the serial walk,
    which raises ShareError with the reference's message for a varint that
    overflows, and ValueError for first reserved bytes outside the share's
    content.  emulate=True runs the device algorithm as a host loop instead
    (dagpu_square_units_emulate_host), whose summary may say UNITS_HOST.
    records / scan: the square's scan when the caller has it (scan_native's)."""
    import numpy as np

    from . import _abi
    L = _abi.lib()
    if not hasattr(ods, "dtype"):
        ods = np.frombuffer(b"".join(s.to_bytes() if isinstance(s, Share) else bytes(s) for s in ods), np.uint8)
    ods = np.ascontiguousarray(ods, np.uint8).reshape(-1)
    if k is None:
        k = math.isqrt(ods.size // sh.SHARE_SIZE)
    pitch = k * sh.SHARE_SIZE if row_pitch is None else row_pitch
    if records is None:
        _, records, scan = scan_native(ods, k, row_pitch=pitch)
    records = np.ascontiguousarray(records)
    scan = np.ascontiguousarray(scan, np.int32)
    seq_cap = max(len(records), int(scan[3]) if int(scan[0]) == _abi.SCAN_OK else 0)
    if len(records) < seq_cap:
        raise ValueError("fewer records than the scan summary counts")
    if unit_cap is not None:
        cap = int(unit_cap)
    else:  # two bytes to a unit at least, of the compact shares' content
        cap = int(scan[6]) // 2 + 1 if int(scan[0]) == _abi.SCAN_OK else 1
    units = np.zeros(max(cap, 1), unit_dtype())
    summary = np.zeros(_abi.UNITS_SUMMARY_WORDS, np.int32)
    fn = L.dagpu_square_units_emulate_host if emulate else L.dagpu_square_units_host
    rc = fn(k, 1, _abi.addr(ods), k * pitch, pitch, seq_cap, _abi.addr(records) if len(records) else None,
            _abi.addr(scan), cap, _abi.addr(units), _abi.addr(summary))
    if rc != 0:
        msg = L.dagpu_last_error(None).decode()
        raise ShareError(msg) if rc == _abi.ERR_SQUARE else ValueError(f"dagpu_square_units_host: status {rc}: {msg}")
    return units[:min(int(summary[2]), cap)].copy(), summary


def unit_bytes(ods, k: int, row_pitch: int, records, unit) -> bytes:
    """The data bytes of one unit record of a host square: bytes [offset,
    offset + len) of its sequence's payload."""
    import numpy as np
    first = int(records["first"][int(unit["seq"])])
    a, n = int(unit["offset"]), int(unit["len"])
    ods = np.asarray(ods, np.uint8).reshape(-1)

    def share(j):
        s = first + j
        at = (s // k) * row_pitch + (s % k) * sh.SHARE_SIZE
        return ods[at + (38 if j == 0 else 34):at + sh.SHARE_SIZE]
    j0 = 0 if a < 474 else 1 + (a - 474) // 478
    j1 = 0 if a + n - 1 < 474 else 1 + (a + n - 1 - 474) // 478
    base = 0 if j0 == 0 else 474 + 478 * (j0 - 1)
    return np.concatenate([share(j) for j in range(j0, j1 + 1)])[a - base:a - base + n].tobytes()


def deconstruct_device(squares, pfb_blob_sizes: Callable[[bytes], Sequence[int]]) -> List[List[bytes]]:
    """square.Deconstruct of every square of a device.DeviceSquares, from where
    it lies in HBM: scan, gather of every blob and both tx streams, download of
    that payload alone, then the checks of deconstruct on the records."""
    return squares.deconstruct(pfb_blob_sizes)
