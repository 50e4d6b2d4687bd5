"""Child process of tests/test_gpu_rs_arms.py: one group of GF(2^8) codec cases
per run, against the test build of the library (DAGPU_LIB = libdagpu_test.so),
whose dispatchers count launches per kernel arm (csrc/kernels.hpp RsArm, read
and reset through dagpu_test_rs_arms).

Every case compares the whole output buffer bit for bit with the oracle
(oracle.encode / oracle.decode / oracle.extend_and_dah) and the arm counters
that moved with the arm the case is meant to reach.  A failed case prints one
`FAIL <case>: <what>` line; the run ends with `DONE <group> <cases>`.

    python rs_arms_child.py <group>
"""
import contextlib
import ctypes
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(_ROOT, "celestia-app_amd"), os.path.join(_ROOT, "oracle")]

import numpy as np  # noqa: E402

import oracle  # noqa: E402
from celestia_da import _abi, da, synth  # noqa: E402

# csrc/kernels.hpp RsArm, in order; counts[arm * 8 + log2(k)]
ARMS = ("enc_packed", "enc_packed_rev", "enc_sliced4", "enc_sliced2", "fill_sliced2", "fill_sliced2_rev",
        "dec_small", "dec_packed128", "dec_sliced128")
NKS = 8
DEC_ARMS = ("dec_small", "dec_packed128", "dec_sliced128")

_fails = []
_ncases = 0


def arms(reset=True):
    """{(arm, k): launches} of the counters that are not zero."""
    L = _abi.lib()
    f = L.dagpu_test_rs_arms
    f.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    f.restype = ctypes.c_int
    out = np.zeros(len(ARMS) * NKS, np.uint64)
    total = f(out.ctypes.data, out.size, 1 if reset else 0)
    assert total == out.size, (total, out.size)
    return {(ARMS[i // NKS], 1 << (i % NKS)): int(c) for i, c in enumerate(out) if c}


@contextlib.contextmanager
def switches(env):
    """The library reads its DAGPU_* switches from the environment per launch."""
    for name, value in env.items():
        os.environ[name] = value
    try:
        yield
    finally:
        for name in env:
            del os.environ[name]


def case(name, problems):
    global _ncases
    _ncases += 1
    for p in problems:
        _fails.append(f"FAIL {name}: {p}")
        print(_fails[-1], flush=True)


def diff(got, want):
    """First difference of two equal-shape uint8 arrays, as text (None: equal)."""
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return None
    i = tuple(int(x) for x in bad[0])
    return f"{len(bad)} bytes differ, first at {i}: got {int(got[i]):#04x}, oracle {int(want[i]):#04x}"


def arm_problem(got, want):
    return None if got == want else f"arms moved {got}, expected {want}"


# --- dagpu_encode -------------------------------------------------------------

def encode_case(ctx, name, k, nvec, shard, want_arm, env=None):
    rng = np.random.default_rng([k, nvec, shard])
    data = rng.integers(0, 256, (nvec, k, shard), dtype=np.uint8)
    want = np.stack([oracle.encode(d) for d in data])
    par = np.full_like(data, 0x5A)
    with switches(env or {}):
        arms()
        ctx.check(ctx._L.dagpu_encode(ctx.handle, k, nvec, shard, _abi.addr(data), _abi.addr(par)))
        got = arms()
    d = diff(par, want)
    case(name, [p for p in (d and "parity: " + d, arm_problem(got, {(want_arm, k): 1})) if p])


def group_encode_tail(ctx):
    """Whole 512-B chunks followed by a partial one: always the packed encoder."""
    for k in (1, 2, 4, 8, 16, 32, 64, 128):
        for shard in (576, 1088):
            for nvec in (3, 4):
                encode_case(ctx, f"encode tail k={k} shard={shard} nvec={nvec}", k, nvec, shard, "enc_packed")


def group_encode_whole(ctx):
    """Whole chunks, nvec % 4 == 0: every encoder arm.  (16, 1024) gives a block
    count that is a multiple of 8 (the XCD remap) with two chunks per shard in
    both bit-sliced kernels."""
    for k in (16, 32, 64, 128):
        for nvec, shard in ((4, 512), (16, 1024)):
            tag = f"k={k} nvec={nvec} shard={shard}"
            encode_case(ctx, f"encode whole {tag} default", k, nvec, shard,
                        "enc_sliced2" if k == 128 else "enc_sliced4")
            if k == 128:
                encode_case(ctx, f"encode whole {tag} DAGPU_ENC_SLICED2=0", k, nvec, shard, "enc_sliced4",
                            {"DAGPU_ENC_SLICED2": "0"})
            encode_case(ctx, f"encode whole {tag} DAGPU_ENC_SLICED=0", k, nvec, shard, "enc_packed",
                        {"DAGPU_ENC_SLICED": "0"})


# --- dagpu_decode -------------------------------------------------------------

PATTERNS = ("random_k", "random_k_plus_quarter", "data_lost", "parity_lost")


def pattern(kind, k, rng):
    idx = np.arange(2 * k)
    if kind == "data_lost":
        return idx >= k
    if kind == "parity_lost":
        return idx < k
    p = np.zeros(2 * k, bool)
    p[rng.choice(2 * k, k + (k // 4 if kind == "random_k_plus_quarter" else 0), replace=False)] = True
    return p


def decode_case(ctx, name, k, shard, kind, fill, want_arm, env=None, nvec=2):
    """nvec vectors with erasures of one kind; missing shards hold `fill` on
    input (the ABI rebuilds them without reading them)."""
    rng = np.random.default_rng([k, shard, PATTERNS.index(kind), fill])
    data = rng.integers(0, 256, (nvec, k, shard), dtype=np.uint8)
    full = np.stack([np.concatenate([d, oracle.encode(d)]) for d in data])
    present = np.stack([pattern(kind, k, rng) for _ in range(nvec)])
    want = np.stack([oracle.decode(full[v] * present[v][:, None], present[v]) for v in range(nvec)])
    buf = full.copy()
    buf[~present] = fill
    given = buf[present].copy()
    pres8 = present.astype(np.uint8)
    with switches(env or {}):
        arms()
        ctx.check(ctx._L.dagpu_decode(ctx.handle, k, nvec, shard, _abi.addr(buf), _abi.addr(pres8)))
        got = arms()
    problems = []
    if not np.array_equal(want, full):
        problems.append("oracle.decode does not return the codeword oracle.encode made")
    if not np.array_equal(buf[present], given):
        problems.append("a present shard came back changed")
    d = diff(buf, want)
    if d:
        problems.append("shards: " + d)
    a = arm_problem(got, {(want_arm, k): 1})
    if a:
        problems.append(a)
    case(name, problems)


def group_decode_tail(ctx):
    """Shard sizes that end in a partial chunk (512-B chunks of the small
    decoder, 256-B chunks of the packed k = 128 decoder)."""
    for ki, k in enumerate((1, 2, 4, 8, 16, 32, 64, 128)):
        for si, shard in enumerate((320, 576)):
            for pi, kind in enumerate(PATTERNS):
                fill = 0xA5 if (ki + si + pi) % 2 else 0
                decode_case(ctx, f"decode tail k={k} shard={shard} {kind} fill={fill:#x}", k, shard, kind, fill,
                            "dec_packed128" if k == 128 else "dec_small")


def group_decode_k128_whole(ctx):
    """k = 128 on whole 512-B chunks: the bit-sliced decoder by default, the
    packed one (256-B chunks 0..3 all live at shard = 1024) under
    DAGPU_DEC_SLICED=0; then locator sharing feeding the packed decoder."""
    k = 128
    for si, shard in enumerate((512, 1024)):
        for pi, kind in enumerate(PATTERNS):
            fill = 0xA5 if (si + pi) % 2 else 0
            tag = f"decode whole k=128 shard={shard} {kind} fill={fill:#x}"
            decode_case(ctx, tag + " default", k, shard, kind, fill, "dec_sliced128")
            decode_case(ctx, tag + " DAGPU_DEC_SLICED=0", k, shard, kind, 0xA5 - fill, "dec_packed128",
                        {"DAGPU_DEC_SLICED": "0"})
    # runs of equal erasure patterns share their error locators
    nvec, shard = 24, 512
    rng = np.random.default_rng(nvec + k)
    data = rng.integers(0, 256, (nvec, k, shard), dtype=np.uint8)
    full = np.stack([np.concatenate([d, oracle.encode(d)]) for d in data])
    present = np.zeros((nvec, 2 * k), np.uint8)
    v = 0
    while v < nvec:
        run = int(rng.integers(1, 6))
        pat = np.zeros(2 * k, np.uint8)
        pat[rng.choice(2 * k, k + int(rng.integers(0, k + 1)), replace=False)] = 1
        present[v:v + run] = pat
        v += run
    want = np.stack([oracle.decode(full[v] * present[v][:, None], present[v]) for v in range(nvec)])
    buf = (full * present[:, :, None]).copy()
    with switches({"DAGPU_DEC_SLICED": "0"}):
        arms()
        ctx.check(ctx._L.dagpu_decode(ctx.handle, k, nvec, shard, _abi.addr(buf), _abi.addr(present)))
        got = arms()
    d = diff(buf, want)
    case("decode batch shared patterns (24, 128, 512) DAGPU_DEC_SLICED=0",
         [p for p in (d and "shards: " + d, arm_problem(got, {("dec_packed128", k): 1})) if p])


# --- squares ------------------------------------------------------------------

def only_arm_problem(got, arm, k):
    """Launch counts depend on the pipeline; the set of arms must be {arm}."""
    return None if set(got) == {(arm, k)} else f"arms moved {got}, expected only {(arm, k)}"


def group_square(ctx):
    """The square path at k = 128 on the two alternative encoders: the row pass
    with its Q0 copy, the column pass strides, and several squares per launch."""
    import torch
    from celestia_da.device import DeviceSquares

    k, n = 128, 3
    w = 2 * k
    one = synth.random_blob_square(k, 1281)
    ref_one = oracle.extend_and_dah(one, k, nthreads=8)
    many = synth.blob_squares(k, 1282, 0, n)
    ref_many = [oracle.extend_and_dah(many[i].reshape(k * k, 512), k, nthreads=8) for i in range(n)]
    for env, arm in (({"DAGPU_ENC_SLICED2": "0"}, "enc_sliced4"), ({"DAGPU_ENC_SLICED": "0"}, "enc_packed")):
        tag = " ".join(f"{a}={b}" for a, b in env.items())
        with switches(env):
            arms()
            eds = da.extend_shares(one, ctx)
            got = arms()
        problems = []
        d = diff(eds.data, ref_one[0])
        if d:
            problems.append("EDS: " + d)
        if b"".join(eds.row_roots()) != ref_one[1].tobytes() or b"".join(eds.col_roots()) != ref_one[2].tobytes():
            problems.append("roots differ from the oracle's")
        problems.append(only_arm_problem(got, arm, k))
        case(f"extend_shares k=128 {tag}", [p for p in problems if p])

        ds = DeviceSquares(k, n, ctx=ctx)
        ds.load_ods(many)
        ds.eds.fill_(0x5A)
        with switches(env):
            arms()
            ds.extend()
            torch.cuda.synchronize()
            got = arms()
        problems = []
        out = ds.eds.cpu().numpy().reshape(n, w, w, 512)
        dah = ds.dah.cpu().numpy()
        for i in range(n):
            d = diff(out[i], ref_many[i][0])
            if d:
                problems.append(f"square {i} EDS: " + d)
            if dah[i].tobytes() != ref_many[i][3]:
                problems.append(f"square {i}: DAH differs from the oracle's")
        problems.append(only_arm_problem(got, arm, k))
        case(f"DeviceSquares(128, 3).extend {tag}", [p for p in problems if p])
        del ds
        torch.cuda.empty_cache()


def group_repair(ctx):
    """Repair at k = 128 through the packed decoder (DAGPU_DEC_SLICED=0), with
    and without the fill route: the two maximal erasure patterns come back as
    the original square, and a corrupted present share is reported as the
    default decoder reports it."""
    k = 128
    w = 2 * k
    eds, rr, cr, _ = oracle.extend_and_dah(synth.random_blob_square(k, 1283), k, nthreads=8)
    rng = np.random.default_rng(1283)
    sub = np.zeros((w, w), bool)
    sub[np.ix_(rng.choice(w, k, replace=False), rng.choice(w, k, replace=False))] = True
    q3 = np.zeros((w, w), bool)
    q3[k:, k:] = True
    bad = eds * sub[:, :, None]
    r, c = np.argwhere(sub)[int(rng.integers(k * k))]
    bad[r, c, 300] ^= 0x40

    def byz_report(env):
        with switches(env):
            arms()
            try:
                da.repair(bad, sub, rr, cr, ctx)
                rep = ("no error",)
            except da.DAError as e:
                rep = (type(e).__name__, e.code, getattr(e, "axis", None), getattr(e, "index", None), e.byz)
            return rep, arms()

    rep_default, got = byz_report({})
    dec = {a: n for a, n in got.items() if a[0] in DEC_ARMS}
    problems = []
    if rep_default[0] != "ErrByzantineData" or rep_default[2] is None:
        problems.append(f"default decoder: expected ErrByzantineData with an axis, got {rep_default}")
    if set(dec) != {("dec_sliced128", k)}:
        problems.append(f"decode arms moved {dec}, expected only dec_sliced128")
    case("repair k=128 corrupted share, default decoder", problems)

    for fill_env in ({}, {"DAGPU_REPAIR_FILL": "0"}):
        env = dict({"DAGPU_DEC_SLICED": "0"}, **fill_env)
        tag = " ".join(f"{a}={b}" for a, b in env.items())
        for pname, pres in (("subgrid", sub), ("q3", q3)):
            with switches(env):
                arms()
                problems = []
                try:
                    fixed, p = da.repair(eds * pres[:, :, None], pres, rr, cr, ctx)
                    d = diff(fixed, eds)
                    if d:
                        problems.append("repaired EDS: " + d)
                    if not p.all():
                        problems.append("cells left missing")
                except da.DAError as e:
                    problems.append(f"repair failed: {e}")
                got = arms()
            dec = {a: n for a, n in got.items() if a[0] in DEC_ARMS}
            if set(dec) != {("dec_packed128", k)}:
                problems.append(f"decode arms moved {dec}, expected only dec_packed128")
            case(f"repair k=128 {pname} {tag}", problems)
        rep, got = byz_report(env)
        dec = {a: n for a, n in got.items() if a[0] in DEC_ARMS}
        problems = []
        if rep != rep_default:
            problems.append(f"report {rep} differs from the default decoder's {rep_default}")
        if set(dec) != {("dec_packed128", k)}:
            problems.append(f"decode arms moved {dec}, expected only dec_packed128")
        case(f"repair k=128 corrupted share {tag}", problems)


GROUPS = {
    "encode_tail": group_encode_tail,
    "encode_whole": group_encode_whole,
    "decode_tail": group_decode_tail,
    "decode_k128_whole": group_decode_k128_whole,
    "square": group_square,
    "repair": group_repair,
}


def main():
    group = sys.argv[1]
    ctx = da.Context(0)
    try:
        GROUPS[group](ctx)
    finally:
        ctx.close()
    print(f"DONE {group} {_ncases} cases, {len(_fails)} failed", flush=True)


if __name__ == "__main__":
    main()
