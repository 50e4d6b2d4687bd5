"""Original data squares whose namespaces use all 29 bytes, for the tests of
every kernel that hashes, compares, packs or searches a namespace
(tests/test_ns_corpus_host.py, tests/test_gpu_ns_corpus.py).  A helper module,
not a test file; every function is deterministic.

The other inputs of the suite keep bytes 0..18 of a namespace all 0x00 or all
0xFF, so neighbours first differ at byte 19 or later.  Here the first differing
byte of adjacent Q0 cells takes every position 0..28, on both axes:

ladder      share j carries the first j mod 30 bytes of one random 29-byte stem
            and random bytes behind them, so the sorted square steps down the
            stem byte by byte and back up (prefix 29 is the whole stem: runs of
            equal namespaces)
runs        full-entropy namespaces in runs of 1 .. 2k shares; inside a run the
            bytes 29..31 of the shares go from FF FF FF to 00 00 00, so a
            comparison that looked past byte 28 would see a descent
edges       the 29 namespaces 00*29 with one byte 01, ladder shares, the 29
            namespaces FF*29 with one byte FE, then shares that carry the parity
            namespace FF*29 itself: one whole Q0 row and half of the row before
            it in the row-major layout (the last column and a half in the
            column-major one).  A k = 8 square has 64 cells, fewer than 58 + 12,
            so at k = 8 part 0 holds the near-zero and part 1 the near-parity
            namespaces; from k = 16 on one square holds all 58 and `part` only
            reseeds the ladder shares
max_row_end a ladder square whose last Q0 cell holds FF*28 FE, the largest
            namespace below the parity one, with the parity quadrant behind it
violations  a ladder square with one Q0 cell's namespace rewritten so that
            exactly one adjacency of one axis is out of order
parity_then_smaller  a Q0 cell with FF*29 followed in its row by a smaller one

layout "row" is the square as sorted (rsmt2d's row-major order); "col" is the
k x k grid transposed, sorted order running down the columns.  Both are valid:
every row and every column of either is in push order."""
import numpy as np

from celestia_da import synth

PARITY = b"\xff" * 29
TAIL_PADDING = b"\xff" * 28 + b"\xfe"
VIOLATION_BYTES = (0, 7, 13, 24, 27, 28)    # word 0, a word's last byte, a middle word, the masked word
POSITION_CLASSES = ("even_odd", "odd_even", "last_pair")


def near_zero(p: int) -> bytes:
    return bytes(p) + b"\x01" + bytes(28 - p)


def near_parity(p: int) -> bytes:
    return b"\xff" * p + b"\xfe" + b"\xff" * (28 - p)


NEAR = [near_zero(p) for p in range(29)] + [near_parity(p) for p in range(29)]


def _layout(sorted_shares: np.ndarray, k: int, layout: str) -> np.ndarray:
    assert layout in ("row", "col") and sorted_shares.shape == (k * k, 512)
    if layout == "row":
        return np.ascontiguousarray(sorted_shares)
    return np.ascontiguousarray(sorted_shares.reshape(k, k, 512).transpose(1, 0, 2)).reshape(k * k, 512)


def _ladder_shares(n: int, rng, inner: bool = False) -> np.ndarray:
    """n unsorted ladder shares.  inner: byte 0 of every namespace in 02..FD, so
    the shares sort between the near-zero and the near-parity namespaces."""
    s = rng.integers(0, 256, size=(n, 512), dtype=np.uint8)
    stem = rng.integers(0, 256, size=29, dtype=np.uint8)
    if inner:
        stem[0] = np.clip(stem[0], 2, 0xFD)
        s[:, 0] = np.clip(s[:, 0], 2, 0xFD)
    for j in range(n):
        s[j, :j % 30] = stem[:j % 30]
    return s


def ladder(k: int, seed: int, layout: str = "row") -> np.ndarray:
    rng = np.random.default_rng(seed)
    return _layout(synth.sort_shares(_ladder_shares(k * k, rng)), k, layout)


def runs(k: int, seed: int, layout: str = "row") -> np.ndarray:
    rng = np.random.default_rng(seed)
    n = k * k
    s = rng.integers(0, 256, size=(n, 512), dtype=np.uint8)
    lengths, left = [], n
    while left:  # the shortest and the longest run first, then random ones
        want = (1, 2 * k)[len(lengths)] if len(lengths) < 2 else int(rng.integers(1, 2 * k + 1))
        lengths.append(min(want, left))
        left -= lengths[-1]
    ns = sorted({bytes(rng.integers(0, 256, size=29, dtype=np.uint8)) for _ in range(len(lengths))})
    assert len(ns) == len(lengths)
    i = 0
    for run, length in zip(ns, lengths):
        s[i:i + length, :29] = np.frombuffer(run, np.uint8)
        high = (length + 1) // 2
        s[i:i + high, 29:32] = 0xFF
        s[i + high:i + length, 29:32] = 0x00
        i += length
    return _layout(s, k, layout)


def edges(k: int, layout: str = "row", part: int = 0) -> np.ndarray:
    assert k >= 8 and part in (0, 1)
    rng = np.random.default_rng(7000 + 2 * k + part)
    n = k * k
    if k == 8:
        near = NEAR[:29] if part == 0 else NEAR[29:]
    else:
        near = NEAR
    n_parity = k + k // 2
    s = rng.integers(0, 256, size=(n, 512), dtype=np.uint8)
    fill = n - len(near) - n_parity
    assert fill >= 0
    s[:fill] = _ladder_shares(fill, rng, inner=True)
    for i, x in enumerate(near):
        s[fill + i, :29] = np.frombuffer(x, np.uint8)
    s[fill + len(near):, :29] = 0xFF
    return _layout(synth.sort_shares(s), k, layout)


def max_row_end(k: int, seed: int) -> np.ndarray:
    ods = ladder(k, seed, "row").copy()
    ods[k * k - 1, :29] = np.frombuffer(TAIL_PADDING, np.uint8)
    return ods


def namespaces(ods: np.ndarray, k: int):
    """ns[r][c]: the 29-byte namespace of Q0 cell (r, c)."""
    return [[ods[r * k + c, :29].tobytes() for c in range(k)] for r in range(k)]


def out_of_order(ods: np.ndarray, k: int):
    """Every adjacency of Q0 that nmt's Push rejects, as (axis, tree, position):
    axis 0 = the pair (tree, position), (tree, position + 1) of a row, axis 1 =
    the pair (position, tree), (position + 1, tree) of a column.  A plain scan
    with bytes comparison."""
    ns = namespaces(ods, k)
    out = []
    for t in range(k):
        for p in range(k - 1):
            if ns[t][p + 1] < ns[t][p]:
                out.append((0, t, p))
            if ns[p + 1][t] < ns[p][t]:
                out.append((1, t, p))
    return out


def first_difference(a: bytes, b: bytes):
    """The first byte position where a and b differ, None when equal."""
    for p in range(len(a)):
        if a[p] != b[p]:
            return p
    return None


def _positions(k: int, cls: str):
    if cls == "last_pair":
        return [k - 2]
    if cls == "even_odd":
        return [p for p in range(0, k - 2, 2)]
    return [p for p in range(1, k - 2, 2)]


def violations(base: np.ndarray, k: int):
    """Yields (ods, axis, position_class, byte): `base` with the namespace of one
    cell raised above its successor on `axis`, first differing from it at `byte`
    and smaller behind it, while the cell stays not above its successor on the
    other axis.  The position class says where the out-of-order pair lies in its
    tree: inside a level-1 pair, across two pairs, or the last pair of Q0."""
    assert k >= 4 and not out_of_order(base, k)
    ns = namespaces(base, k)
    turn = 0
    for axis in (0, 1):
        for cls in POSITION_CLASSES:
            for byte in VIOLATION_BYTES:
                turn += 1
                cells = [(t, p) for t in range(k) for p in _positions(k, cls)]
                cells = cells[turn * 5 % len(cells):] + cells[:turn * 5 % len(cells)]
                for t, p in cells:
                    r, c = (t, p) if axis == 0 else (p, t)
                    succ = ns[r][c + 1] if axis == 0 else ns[r + 1][c]
                    if succ[byte] == 0xFF or not any(succ[byte + 1:] or b"\x01"):
                        continue
                    value = succ[:byte] + bytes([succ[byte] + 1]) + bytes(28 - byte)
                    orow, ocol = (r + 1, c) if axis == 0 else (r, c + 1)
                    other = ns[orow][ocol] if orow < k and ocol < k else PARITY    # the parity quadrant
                    if other < value:
                        continue
                    # above its successor, so above its predecessors too: (axis, t, p) is the one pair out of order
                    ods = base.copy()
                    ods[r * k + c, :29] = np.frombuffer(value, np.uint8)
                    yield ods, axis, cls, byte
                    break
                else:
                    raise AssertionError("no cell for axis %d, %s, byte %d: change the base" % (axis, cls, byte))


def parity_then_smaller(k: int, seed: int) -> np.ndarray:
    """A ladder square whose cell (k - 1, k / 2) carries FF*29: the next cell of
    the last row is smaller, the column below it is the parity quadrant."""
    ods = ladder(k, seed, "row").copy()
    ods[(k - 1) * k + k // 2, :29] = 0xFF
    return ods


# ---- queries, trees and tampers shared by the host and the GPU tests -----------------------

TAMPER_BYTES = (0, 7, 13, 24, 28)


def flip_byte(b: bytes, at: int, mask: int = 1) -> bytes:
    return b[:at] + bytes([b[at] ^ mask]) + b[at + 1:]


def queries(ods: np.ndarray, k: int):
    """The namespaces to search a square for: every distinct namespace of the
    square; each with its last byte +1 and -1; each with one byte flipped in every
    64-bit word of a big-endian key (bytes 0..7, 8..15, 16..23, 24..28), the byte
    moving with the namespace's rank; the 58 near-namespaces; 00*29, the tail
    padding namespace and FF*29.  Without duplicates, in that order."""
    own = sorted({ods[i, :29].tobytes() for i in range(k * k)})
    out = list(own)
    for i, x in enumerate(own):
        out.append(x[:28] + bytes([(x[28] + 1) & 0xFF]))
        out.append(x[:28] + bytes([(x[28] - 1) & 0xFF]))
        for word in range(4):
            out.append(flip_byte(x, 8 * word + i % (8 if word < 3 else 5), 1 << (i % 8)))
    out += NEAR + [bytes(29), TAIL_PADDING, PARITY]
    seen, uniq = set(), []
    for x in out:
        if x not in seen:
            seen.add(x)
            uniq.append(x)
    return uniq


def leaf_namespace(eds: np.ndarray, k: int, r: int, c: int) -> bytes:
    return eds[r, c, :29].tobytes() if r < k and c < k else PARITY


def axis_trees(eds: np.ndarray, k: int, model):
    """trees[axis][index]: nmt_namespace_model.Tree of every row (axis 0) and
    column (axis 1) of an extended square (2k, 2k, 512), hashed with pyref."""
    w = 2 * k
    leaf = [[model.pyref.leaf(leaf_namespace(eds, k, r, c), eds[r, c].tobytes()) for c in range(w)] for r in range(w)]
    return [[model.Tree(leaf[i]) for i in range(w)], [model.Tree([leaf[r][i] for r in range(w)]) for i in range(w)]]


def namespace_tampers(nid: bytes, nodes, turn: int):
    """(class, nid, nodes): the proof with the min or max namespace of one of its
    nodes changed at one byte, and with the claimed namespace changed at one
    byte, for every byte of TAMPER_BYTES.  `turn` moves the node and the field."""
    out = []
    for i, p in enumerate(TAMPER_BYTES):
        if nodes:
            at = (turn + i) % len(nodes)
            field = 29 * ((turn + i) // len(nodes) % 2)
            bad = list(nodes)
            bad[at] = flip_byte(nodes[at], field + p, 0x10)
            out.append(("node_%s_byte_%d" % ("max" if field else "min", p), nid, bad))
        out.append(("claimed_byte_%d" % p, flip_byte(nid, p, 0x10), list(nodes)))
    return out
