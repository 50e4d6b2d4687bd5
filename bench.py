"""bench.py -- headline benchmark of the MI355X DA hot path.

Metric (BASELINE.json): EDS+DAH squares/sec for 128x128 -> 256x256 squares
(configs[1]): ODS resident in HBM -> Leopard RS extension -> NMT row/col roots
-> DAH, per square, bit-exact with the reference.  One step = one pass of the
hot path over one batch of `--batch` distinct squares per GPU.  Multi-GPU:
squares are independent, each rank extends its own batch (weak scaling, no
data-path collective); the barrier + max-over-ranks timing follows the driver
contract.

A plain run (`--gpus 1 --steps N --warmup W`) sets up, warms up, times the N
steps and prints the headline line; `--dump-outputs DIR` also writes what the
last timed step computed as DIR/<name>.npy.

With `--full`, also reported: RS GB/s (algorithmic bytes 4k^2*512 per square
over the RS kernels' time), NMT SHA-256 compressions/s (983,550 per k=128
square, each leaf hashed once), the roofline of the dominant kernel measured
with HIP events on the launch stream, the headline bit-exact check, the block
replay, the end-to-end and other-config lines, and the CPU oracle ("port") on
host cores.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "celestia-app_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

# --- work units --------------------------------
SHARE = 512
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
VALU_PEAK_TOPS = 78.64         # 256 CU x 4 SIMD x 32 lanes x 2.4 GHz int32 ops/s (/1e12)
# measured SHA-256 compression ceiling of this chip (tools/valu_bench, profiles/valu_bench_r01.log):
# 28.6 G compressions/s = 39.6 T int32 ops/s; VOP3 forms issue at ~1 wave-instr/clk/CU, not 2
VALU_MEASURED_TOPS = 39.6
# Minimal CDNA4 int32 ops per SHA-256 compression with v_alignbit rotates,
# v_bitop3 (xor3/ch/maj) and v_add3: 64 rounds x 14 + 48 schedule words x 10 + 8.
OPS_PER_COMPRESSION = 64 * 14 + 48 * 10 + 8


def compressions(k: int):
    """SHA-256 compressions per square, split (leaves, tree nodes, dah)."""
    w = 2 * k
    leaves = 9 * w * w                 # 542-B leaf message, each cell hashed once
    nodes = 3 * 2 * w * (w - 1)        # 181-B inner node messages
    dah = 2 * (2 * w) + 2 * (2 * w - 1)
    return leaves, nodes, dah


def rs_bytes(k: int) -> int:
    return 4 * k * k * SHARE           # read Q0 + write Q1..Q3


def dist_init():
    """One process per GPU over RCCL (torch.distributed "nccl").  With
    DAGPU_BENCH_SHARED_GPU=1 every rank uses GPU 0 and the collectives run over
    gloo, host-staged: a rehearsal of the N>1 code path on a one-GPU box (the
    numbers it prints are not scaling numbers)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # DAGPU_BENCH_FORCE_DIST=1 (under torch.distributed.run) keeps the process
    # group even at one rank, so the N > 1 code path -- RCCL collectives
    # included -- runs on a one-GPU box (tests/test_gpu_bench_checks.py)
    if world > 1 or os.environ.get("DAGPU_BENCH_FORCE_DIST") == "1":
        import torch.distributed as dist
        import datetime
        if os.environ.get("DAGPU_BENCH_SHARED_GPU") == "1":
            dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=300))
            return dist, rank, world, 0
        dist.init_process_group("nccl", device_id=torch.device("cuda", local),
                                timeout=datetime.timedelta(seconds=300))
        return dist, rank, world, local
    return None, 0, 1, 0


def _host_staged(dist) -> bool:
    return dist is not None and dist.get_backend() == "gloo"


def barrier(dist):
    if dist is not None:
        dist.barrier()


def max_over_ranks(dist, v: float, local: int) -> float:
    if dist is None:
        return v
    dev = torch.device("cpu") if _host_staged(dist) else torch.device("cuda", local)
    t = torch.tensor([v], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def all_gather_rows(dist, world, t):
    """All-gather of equal-shaped per-rank tensors along dim 0 (RCCL on device;
    gloo through host memory)."""
    if dist is None:
        return t
    if _host_staged(dist):
        h = t.cpu()
        parts = [torch.empty_like(h) for _ in range(world)]
        dist.all_gather(parts, h)
        return torch.cat(parts).to(t.device)
    allg = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(allg, t)
    return allg


def per_rank_ms(dist, world, ms: float):
    """Every rank's own ms per step (its stream drained, before the barrier)."""
    if dist is None:
        return [ms]
    got = [None] * world
    dist.all_gather_object(got, float(ms))
    return got


def ranks_report(dist, rank_ms, numa_report):
    """N > 1 context for the bench line: per-rank step times (min / max / all),
    each rank's GPU, NUMA node and affinity, the collective library and its
    version, and the GPU-to-GPU links the KFD topology offers (xGMI point to
    point or PCIe) -- what a first scaling line needs to explain itself."""
    from celestia_da import numa
    world = len(rank_ms)
    placement = [None] * world
    dist.all_gather_object(placement, numa_report)
    backend = dist.get_backend()
    rep = {"backend": backend, "world": world,
           "step_ms": {"min": min(rank_ms), "max": max(rank_ms), "per_rank": [round(x, 4) for x in rank_ms]},
           "placement": placement}
    try:
        v = torch.cuda.nccl.version()
        rep["rccl_version"] = ".".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
    except Exception as e:  # noqa: BLE001 -- report, never fail the bench on it
        rep["rccl_version"] = f"unavailable ({type(e).__name__})"
    links = numa.gpu_links()
    mine = [p.get("pci") for p in placement if p]
    rep["links"] = {pci: links.get(pci) for pci in dict.fromkeys(mine)}
    if backend == "gloo":
        rep["transport"] = "gloo over host memory (DAGPU_BENCH_SHARED_GPU rehearsal, one GPU)"
    else:
        peers = [links.get(a, {}).get("xgmi", []) for a in mine]
        all_xgmi = all(b in peers[i] for i, a in enumerate(mine) for b in mine if b != a) if mine else False
        rep["transport"] = ("RCCL P2P over xGMI (every rank pair directly linked)" if all_xgmi and len(set(mine)) > 1
                            else "RCCL (not every rank pair has a direct xGMI link: PCIe / host path)")
    return rep


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(seconds: float, threads: int):
    """CPU baseline on the host cores (BASELINE.md fallback for the Go path
    pkg/da/data_availability_header.go:44-75, which cannot be built here):
    oracle/da_simd.c -- GFNI/AVX-512 (or AVX2 PSHUFB) GF(2^8) mul-add with
    per-constant tables built once, x86 SHA extensions, the reference's work
    (each leaf hashed in its row and its column tree), rows/columns/trees over
    `threads` OpenMP threads.  Timed on configs[1] (k=128, the headline's unit)
    and configs[0] (k=64) random-blob squares, `seconds` each; the EDS is
    written to host memory as ExtendShares returns it."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    from celestia_da import synth

    res = {}
    for k in (128, 64):
        ods = synth.blob_squares(k, 90000 + k, 0, 4, threads=threads)
        sq = oracle.SimdSquare(k)
        sq.run(ods[0], threads)  # warm
        n, t0 = 0, time.perf_counter()
        while True:
            sq.run(ods[n % len(ods)], threads)
            n += 1
            el = time.perf_counter() - t0
            if el >= seconds:
                break
        res[k] = (n, el)
    n, el = res[128]
    n64, el64 = res[64]
    # thread scaling at k = 128 (bounded: ~2 s per point), so the figure can be
    # read against hosts with more usable cores than this lease
    scaling = {}
    ods128 = synth.blob_squares(128, 90128, 0, 4, threads=threads)
    sq = oracle.SimdSquare(128)
    t = 1
    while t < threads:
        sq.run(ods128[0], t)  # warm (thread team of this size)
        m, t0 = 0, time.perf_counter()
        while True:
            sq.run(ods128[m % len(ods128)], t)
            m += 1
            if time.perf_counter() - t0 >= min(2.0, seconds):
                break
        e = time.perf_counter() - t0
        scaling[str(t)] = {"squares_per_s": m / e, "per_thread": m / e / t}
        t *= 2
    scaling[str(threads)] = {"squares_per_s": n / el, "per_thread": n / el / threads}
    quota = cgroup_cpus()
    return {
        "value": n / el,
        "unit": "squares/s",
        "cores": threads,
        "kind": "simd-port",
        "k": 128,
        "per_core_squares_per_s": n / el / threads,
        "thread_scaling": scaling,
        "usable_cpus": threads,
        "cgroup_cpu_quota": quota,
        "cpu_share_note": (f"{threads} of the host's {os.cpu_count()} CPUs usable by this process "
                           f"(cgroup quota {quota}); gpu_over_cpu compares against this per-lease share"),
        "cpu_model": cpu_model(),
        "host_cpus_visible": os.cpu_count(),
        "isa": oracle.simd_isa(),
        "sample": f"{n} random-blob 128x128 squares, ExtendShares+NewDataAvailabilityHeader "
                  f"(oracle/da_simd.c, {threads} threads, {el:.1f} s wall; leaves hashed per row and "
                  f"column tree as the reference does)",
        "configs0_k64": {"squares_per_s": n64 / el64, "ms_per_square": el64 / n64 * 1e3,
                         "sample": f"{n64} random-blob 64x64 squares, {el64:.1f} s wall"},
        "note": "C restatement of the Go path (no Go toolchain here), not the Go reference itself",
    }


def load_traffic(kernel: str):
    """(HBM bytes per launch of `kernel`, the profile's tag) from the committed
    rocprofv3 PMC summary (profiles/pmc_traffic.json written by
    tools/pmc_summary.py, FETCH_SIZE doubled per the gfx950 correction), or
    (None, None).  The tag names the round/build the counters came from."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        e = json.load(open(path)).get(kernel, {})
        return e.get("hbm_bytes_per_launch"), e.get("tag")
    except Exception:
        return None, None


def load_stress_pmc(kernel: str):
    """Committed counters of a GF(2^16) stress kernel (profiles/pmc_stress.json,
    tools/pmc_stress.py over a tools/gpu_pmc_gf16.sh run): VALU wave-instructions
    per clock per CU and the fraction of wave cycles parked on s_waitcnt, with
    the profile's tag; None if absent."""
    path = os.path.join(ROOT, "profiles", "pmc_stress.json")
    try:
        e = json.load(open(path))[kernel]
        return {"valu_per_clk_per_cu": e["valu_per_clk_per_cu"], "wait_inst_frac": e.get("wait_inst_frac"),
                "counters_tag": e.get("tag"), "counters_source": "profiles/pmc_stress.json (rocprofv3 --pmc, "
                                                                   "separate passes)"}
    except Exception:
        return None


def gf16_kernel_names(k: int):
    """(forward encoder, decoder) kernel names the library runs at width k
    (csrc/rs_gf16.hip / rs_gf16_wide.hip launch selection), as rocprofv3 /
    tools/pmc_stress.py name them."""
    if k == 512:  # round 6: the quarter-lane kernels
        return "leo16_encode_q_kernel<512, false>", "leo16_decode_q_kernel<512>"
    if k == 256:
        return "leo16_encode_h_kernel<256, false>", "leo16_decode_h_kernel<256>"
    ng = {1024: 8, 2048: 8, 4096: 4, 8192: 2}  # slice widths (encoder m = k, decoder n = 2k)
    eg = {8: 4, 4: 4, 2: 2, 1: 1}
    dg = {8: 8, 4: 4, 2: 2, 1: 1}
    e_ng = ng.get(k, 1)
    d_ng = ng.get(2 * k, 1)
    enc = f"leo16w_encode_kernel<{e_ng}, {eg[e_ng]}>"
    if k == 1024:  # round 6: the quarter-lane kernels (encoder 8 waves, decoder 16)
        return "leo16_encode_q_kernel<1024, false>", "leo16_decode_q_kernel<1024>"
    if k == 2048:  # round 6: the quarter-lane encoder (16 waves), the wide decoder
        enc = "leo16_encode_q_kernel<2048, false>"
    return enc, f"leo16w_decode_kernel<{d_ng}, {dg[d_ng]}>"


def stress_roofline(kernel: str, alg_bytes: float, ms: float, launches: int, pmc_name: str, work: str):
    """Roofline entry of a stress line's dominant kernel: algorithmic bytes per
    launch over its average launch time (HIP events of the library's profiled
    pass) against the HBM peak, plus the committed counters of that kernel."""
    if not ms or not launches:
        return None
    avg = ms / launches
    ach = alg_bytes / launches / (avg * 1e-3) / 1e9
    r = {"kernel": kernel, "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
         "frac": ach / HBM_PEAK_GBS, "avg_launch_ms": avg, "launches": launches, "work": work}
    pmc = load_stress_pmc(pmc_name)
    if pmc:
        r.update(pmc)
    return r


def valu_issue(k: int, B: int, ms_step: float, leaf_ms: float):
    """Whole-step VALU issue rate: the kernels' VALU wave-instructions per step
    (rocprofv3 SQ_INSTS_VALU per launch, profiles/pmc_valu.json, collected on
    this same k=128 x 256-square step by tools/gpu_profile.sh) over the measured
    step time x CUs x the clock the chip holds (GRBM_GUI_ACTIVE of the leaf
    launch, summed over MI355X's 8 XCDs, over this run's leaf time).  The
    ceiling of any stream with slow-class ops (v_alignbit, v_add3, v_perm) is
    ~1 wave-instruction per clock per CU (profiles/issue_bench_r01.log)."""
    path = os.path.join(ROOT, "profiles", "pmc_valu.json")
    try:
        d = json.load(open(path))
        per = {n: d[n]["valu_wave_instr_per_launch"] for n in
               ("rs_encode_sliced2", "nmt_leaves", "nmt_trees_l1", "nmt_trees_ln", "dah")}
        grbm = d["nmt_leaves"]["grbm_gui_active_per_launch"]
        tag = d["nmt_leaves"].get("tag")
    except Exception:
        return None
    if k != 128 or B != 256 or not grbm or not leaf_ms:
        return None
    levels = 8  # tree levels at k = 128: level 1 + 7 level launches
    total = 2 * per["rs_encode_sliced2"] + per["nmt_leaves"] + per["nmt_trees_l1"] \
        + (levels - 1) * per["nmt_trees_ln"] + per["dah"]
    clock = grbm / 8 / (leaf_ms * 1e-3)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return {"estimate": True,
            "wave_instr_per_step_committed": total, "clock_ghz_est": clock / 1e9, "cus": cus,
            "wave_instr_per_clk_per_cu_est": total / (ms_step * 1e-3 * cus * clock),
            "ceiling": 1.0, "counts_build": tag,
            "source": f"ESTIMATE: instruction and GRBM cycle counts committed in profiles/pmc_valu.json "
                      f"(build {tag}, another run and box) divided by this run's step and leaf times; "
                      f"stale if a kernel changed since {tag}"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the headline: bit-exact check, per-kernel times and roofline, block replay, "
                         "end-to-end, the other configs and the CPU baseline (each has its own --no-* switch)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (roots, DAHs, status, a seeded sample of EDS "
                         "shares) as DIR/<name>.npy, float32 (headline mode, rank 0)")
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--batch", type=int, default=256,
                    help="squares per GPU per step (SURVEY.md §8d: C2 batches of >= 256 squares)")
    ap.add_argument("--distinct", type=int, default=256, help="distinct generated squares per GPU")
    ap.add_argument("--repair-slices", type=int, default=1,
                    help="--mode repair: the batch as this many asynchronous calls on their own streams")
    ap.add_argument("--pattern", choices=["subgrid", "q3"], default="subgrid",
                    help="--mode repair: kept cells = a random k x k sub-grid (configs[3]) or Q3 only")
    ap.add_argument("--cpu-seconds", type=float, default=8.0, help="CPU baseline time per k (64 and 128)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="CPU baseline threads (0 = all usable host cores)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--separate-ods", dest="in_place", action="store_false",
                    help="keep the ODS in its own buffer (the row pass then also copies Q0 into the EDS); "
                         "default: ODS resident in Q0 of the EDS buffer (dagpu_extend_batch_device, d_ods = NULL)")
    ap.add_argument("--mode", choices=["extend", "mixed", "repair", "split"], default="extend",
                    help="extend: configs[1] (headline); mixed: configs[2]; repair: configs[3]; "
                         "split: configs[4] oversized square over all ranks")
    ap.add_argument("--split-k", type=int, nargs="*", default=[256, 512],
                    help="split stress square widths (k); also run after the headline when N > 1")
    ap.add_argument("--split-steps", type=int, default=3)
    ap.add_argument("--no-split", action="store_true", help="skip the split stress at N > 1")
    ap.add_argument("--no-e2e", action="store_true", help="skip the PCIe-inclusive end-to-end measurement")
    ap.add_argument("--no-configs", action="store_true",
                    help="skip the configs[2] mixed batch and configs[3] repair lines of the default run")
    ap.add_argument("--replay-blocks", type=int, default=8192, help="configs[4] block replay length")
    ap.add_argument("--no-replay", action="store_true", help="skip the block replay measurement")
    ap.add_argument("--no-check", dest="check", action="store_false",
                    help="skip the headline bit-exact check (rocprofv3 counter runs only: its host-API "
                         "launches of 16-square chunks would mix into the per-launch averages)")
    ap.add_argument("--replay-dump", default=None,
                    help="write the sampled replay DAHs (block -> hex) to this JSON file (tests)")
    args = ap.parse_args()
    if args.dump_outputs and args.mode != "extend":
        ap.error("--dump-outputs applies to the headline (--mode extend)")
    if args.mode == "split":
        return bench_split_main(args)
    if args.mode == "mixed":
        return bench_mixed(args)
    if args.mode == "repair":
        return bench_repair(args)

    # before anything touches the GPU: this rank's threads and its pinned
    # replay shard on its GPU's NUMA node (celestia_da/numa.py)
    from celestia_da import numa
    numa_report = numa.bind(0 if os.environ.get("DAGPU_BENCH_SHARED_GPU") == "1"
                            else int(os.environ.get("LOCAL_RANK", "0")))
    dist, rank, world, local = dist_init()
    torch.cuda.set_device(local)
    from celestia_da import _abi, da, synth
    from celestia_da.device import DeviceSquares

    k, B = args.k, args.batch
    ctx = da.Context(local)
    ds = DeviceSquares(k, B, device=local, ctx=ctx, in_place=args.in_place)
    # distinct synthetic squares (seeded run, rank r takes squares r*B ..), replicated
    # up to the batch size if --distinct is smaller
    nd = min(args.distinct, B)
    host = synth.blob_squares(k, HEADLINE_SEED, rank * B, nd, threads=host_threads())
    batch_ods = host if nd == B else np.stack([host[i % nd] for i in range(B)])
    ds.load_ods(batch_ods)
    torch.cuda.synchronize()

    stream = torch.cuda.current_stream()
    for _ in range(args.warmup):
        ds.extend(stream)
    torch.cuda.synchronize()
    st = ds.status.cpu().numpy()
    if (st != 0).any():
        raise SystemExit(f"rank {rank}: status error {st}")

    # ---- timed region: exactly `steps` passes ----
    L = ctx._L
    barrier(dist)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ds.extend(stream)
    torch.cuda.synchronize()
    el_own = time.perf_counter() - t0  # this rank's own work (before waiting for the others)
    barrier(dist)
    el = time.perf_counter() - t0
    el_max = max_over_ranks(dist, el, local)
    squares = B * args.steps * world
    value = squares / el_max
    ms_step = el_max / args.steps * 1e3
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ds)

    out = {
        "metric": "EDS+DAH squares/sec (128→256 sq, node) + RS GB/s & NMT SHA-256 hashes/sec",
        "value": value,
        "unit": "squares/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_step,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic random-namespace blob shares (sorted, seeded), device-resident",
        "config": {
            "workload": f"{k}x{k} ODS -> {2*k}x{2*k} EDS + NMT row/col roots + DAH (configs[1])",
            "k": k,
            "squares_per_gpu_per_step": B,
            "global_batch": B * world,
            "parallelism": f"squares sharded over {world} GPU(s), no collective",
            "ods_layout": "in place (Q0 of the EDS buffer)" if args.in_place else "separate ODS buffer",
        },
    }
    if not args.full:  # a plain run: the headline alone
        st = ds.status.cpu().numpy()
        if (st != 0).any():
            raise SystemExit(f"rank {rank}: status error {st}")
        if rank == 0:
            print(json.dumps(out), flush=True)
        ctx.close()
        if dist is not None:
            dist.destroy_process_group()
        return

    rank_ms = per_rank_ms(dist, world, el_own / args.steps * 1e3)
    # the timed batch proves its own output before anything else runs on it
    headline_check = (check_headline(dist, local, ctx, ds, batch_ods) if args.check
                      else {"bit_exact": None, "skipped": "--no-check (profiling run)"})
    del batch_ods

    # ---- per-kernel times: a separate profiled pass (HIP events on the launch
    # stream around every kernel; the library runs the batch serially while
    # profiling, so each kernel's interval is its own) ----
    L.dagpu_profile_enable(ctx.handle, 1)
    L.dagpu_profile_read(ctx.handle, None, None, 1)
    for _ in range(min(args.steps, 10)):
        ds.extend(stream)
    torch.cuda.synchronize()
    L.dagpu_profile_enable(ctx.handle, 0)
    tot = np.zeros(_abi.PROFILE_KERNELS.__len__(), np.float64)
    cnt = np.zeros(len(_abi.PROFILE_KERNELS), np.uint64)
    L.dagpu_profile_read(ctx.handle, _abi.addr(tot), _abi.addr(cnt), 1)
    st = ds.status.cpu().numpy()
    if (st != 0).any():
        raise SystemExit(f"rank {rank}: status error {st}")

    # mean per launch of each kernel id; one launch of each per step except the
    # trees (one launch sequence per step, summed by the library per scope)
    per = {name: (tot[i] / cnt[i] if cnt[i] else 0.0) for i, name in enumerate(_abi.PROFILE_KERNELS)}
    lv, nd_, dh = compressions(k)
    comp_sq = lv + nd_ + dh
    kernel_ms_step = sum(per[n] for n in ("rs_row", "rs_col", "nmt_leaves", "nmt_trees", "dah"))
    rs_ms = per["rs_row"] + per["rs_col"]
    rs_gbs = rs_bytes(k) * B / (rs_ms * 1e-3) / 1e9 if rs_ms else None
    nmt_ms = per["nmt_leaves"] + per["nmt_trees"] + per["dah"]
    comp_per_s = comp_sq * B / (nmt_ms * 1e-3) if nmt_ms else None

    # dominant kernel roofline
    dom = max(("rs_row", "rs_col", "nmt_leaves", "nmt_trees"), key=lambda n: per[n])
    if dom.startswith("rs"):
        nvec = k if dom == "rs_row" else 2 * k
        alg = (2 * nvec * k * SHARE) * B + (k * k * SHARE * B if dom == "rs_row" else 0)
        ach = alg / (per[dom] * 1e-3) / 1e9
        roof = {"kernel": dom, "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": ach / HBM_PEAK_GBS}
    else:
        comp = (lv if dom == "nmt_leaves" else nd_) * B
        ach = comp * OPS_PER_COMPRESSION / (per[dom] * 1e-3) / 1e12
        roof = {"kernel": dom, "bound": "valu", "achieved": ach, "peak": VALU_PEAK_TOPS,
                "unit": "Tint32op/s", "frac": ach / VALU_PEAK_TOPS,
                "work": f"{comp} SHA-256 compressions x {OPS_PER_COMPRESSION} int32 ops",
                "measured_ceiling": VALU_MEASURED_TOPS, "frac_of_measured": ach / VALU_MEASURED_TOPS}
    roof["traffic"], roof["traffic_tag"] = load_traffic(
        {"rs_row": "rs_encode_sliced2", "rs_col": "rs_encode_sliced2"}.get(dom, dom))
    roof["traffic_source"] = ("profiles/pmc_traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the "
                              "headline step, per launch, tagged with the build they came from")
    roof["avg_launch_ms"] = per[dom]

    out.update({
        "rs_gbs": rs_gbs,
        "nmt_sha256_compressions_per_s": comp_per_s,
        "kernel_ms_per_step": {n: per[n] for n in per if per[n]},
        "kernel_ms_note": "separate profiled pass (HIP events around each kernel on the launch stream); the timed steps run unprofiled",
        "kernel_sum_ms_per_step": kernel_ms_step,
        "roofline": roof,
        "valu_issue": valu_issue(k, B, ms_step, per["nmt_leaves"]),
        "headline_bit_exact": headline_check["bit_exact"],
        "headline_check": headline_check,
    })
    # single-square latency first: after the replay's 64 GiB page-locked
    # allocation the same device->host copies ran slower (k=128 with the EDS
    # returned: 1.40 vs 0.89 ms, profiles/single_square_r02.log)
    single = bench_single(ctx) if world == 1 and not args.no_e2e else None
    if not args.no_replay:
        out["block_replay"] = bench_replay(dist, rank, world, local, ctx, ds, args.replay_blocks,
                                           args.replay_dump, numa_report)
    if world == 1 and not args.no_e2e:
        del ds
        torch.cuda.empty_cache()
        out["end_to_end"] = bench_e2e(ctx, local, k, np.stack([host[i % nd] for i in range(B)]),
                                      max(3, args.steps // 4))
        out["end_to_end"]["single_square"] = single
        out["end_to_end"]["square_construct"] = bench_construct(ctx)
    if world == 1 and not args.no_configs:
        # configs[2] and configs[3] (and the GF(2^16) stress repair) at bounded
        # step counts, so that the driver's own run records them too
        if "ds" in locals():
            del ds
            torch.cuda.empty_cache()
        out["other_configs"] = {
            "configs[2]_mixed_4096": run_mixed(ctx, 3, 1),
            # 10 timed steps (round 6; 3 before): round-over-round changes of a few
            # per cent must be resolvable (verdict r05).  The 256 squares as 4
            # started repairs (dagpu_repair_start / _join, each slice's crossword on
            # its own stream, so one slice's host turnarounds and last tree levels
            # overlap another's kernels): 17.19-17.44 k vs 17.01-17.14 k squares/s
            # as one batch, same box (profiles/repair_slices_ab_r06.log; 8 slices:
            # 16.97-17.12 k, 16: 16.26-16.34 k); the one-batch call stays beside it.
            "configs[3]_repair_k128": run_repair(ctx, 128, 256, 10, 2, slices=4),
            "configs[3]_repair_k128_one_batch": run_repair(ctx, 128, 256, 10, 2),
            "repair_k512_gf16": run_repair(ctx, 512, 2, 10, 2),
            # the other maximal erasure pattern (Q3 only kept): the reverse fill's case
            "repair_k128_q3": run_repair(ctx, 128, 256, 10, 2, pattern="q3"),
            "repair_k512_gf16_q3": run_repair(ctx, 512, 2, 10, 2, pattern="q3"),
            # configs[4] stress square through the split path at P = 1 (the N > 1 line
            # carries the same square split over every rank as split_stress)
            # 40 steps (round 6; 20 before, 5 before that): each step ends in the
            # status read-back, so the next step's first launch latency is in every
            # step; more steps only steady the mean (split k = 512 1.199 ms at 20,
            # 1.177-1.187 at 40, profiles/split_n2r_ab_r06.log)
            "configs[4]_split_k256": bench_split(None, 0, 1, local, ctx, 256, 40, 3),
            "configs[4]_split_k512": bench_split(None, 0, 1, local, ctx, 512, 40, 3),
        }
    if rank == 0 and world == 1 and not args.no_cpu:
        out["cpu_baseline"] = cpu_baseline(args.cpu_seconds, args.cpu_threads or host_threads())
        out["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
        out["gpu_over_cpu_core"] = value / out["cpu_baseline"]["per_core_squares_per_s"]
    if dist is not None:
        out["ranks"] = ranks_report(dist, rank_ms, numa_report)
    if dist is not None and not args.no_split:
        # configs[4] stress: one oversized square split over all ranks (RCCL all-to-all)
        if "ds" in locals():
            del ds
        torch.cuda.empty_cache()
        out["split_stress"] = {str(sk): bench_split(dist, rank, world, local, ctx, sk, args.split_steps, 1)
                               for sk in args.split_k}
    if rank == 0:
        print(json.dumps(out), flush=True)
    ctx.close()
    if dist is not None:
        dist.destroy_process_group()


DUMP_SEED = 0xD0A7
# rows kept per dumped array (float32): 2 x 65536 x 90 roots + 16384 x (32 + 1)
# + 4096 x 512 EDS bytes = 57.7 MB, under the 64 MB a dump may take
DUMP_ROWS = {"row_roots": 65536, "col_roots": 65536, "dah": 16384, "status": 16384, "eds_sample": 4096}


def _dump_rows(t, max_rows: int, seed: int):
    """Rows of the 2-D tensor `t` as float32: all of them, or a sorted seeded
    sample of `max_rows` (the same rows for the same shape, run after run)."""
    n = int(t.shape[0])
    if n > max_rows:
        idx = np.sort(np.random.default_rng(seed).choice(n, max_rows, replace=False))
        t = t[torch.from_numpy(idx).to(t.device)]
    return t.cpu().numpy().astype(np.float32)


def dump_outputs(path: str, ds) -> None:
    """--dump-outputs: what the last timed step left in the caller's buffers of
    dagpu_extend_batch_device -- every row/column root, DAH and status of the
    batch (a seeded sample of squares' rows past DUMP_ROWS) and a seeded sample
    of 512-byte EDS shares (the whole EDS is 32 MiB per k = 128 square) -- as
    <path>/<name>.npy, bytes as float32.  Called after the synchronise that
    ends the timed region."""
    os.makedirs(path, exist_ok=True)
    w = 2 * ds.k
    arrays = {"row_roots": ds.row_roots.view(ds.n * w, -1), "col_roots": ds.col_roots.view(ds.n * w, -1),
              "dah": ds.dah, "status": ds.status.view(ds.n, 1), "eds_sample": ds.eds.view(ds.n * w * w, SHARE)}
    for i, (name, t) in enumerate(arrays.items()):
        np.save(os.path.join(path, name + ".npy"), _dump_rows(t, DUMP_ROWS[name], DUMP_SEED + i))


def check_headline(dist, local, ctx, ds, batch_ods):
    """Bit-exactness of the timed configuration itself (ODS in place or not,
    the RS/NMT slice pipeline as the timed steps ran it): every DAH and every
    row/column root of the last timed step against the drop-in host API
    dagpu_extend_batch on the same host ODS (its own, unsliced kernel chain;
    oracle-pinned in tests/test_gpu_parity.py).  Fatal on every rank on any
    mismatch.  DAGPU_BENCH_CORRUPT=headline flips one byte to prove it fires."""
    from celestia_da import da

    torch.cuda.synchronize()
    dah = ds.dah.cpu().numpy()
    rr = ds.row_roots.cpu().numpy()
    cr = ds.col_roots.cpu().numpy()
    st = ds.status.cpu().numpy()
    if os.environ.get("DAGPU_BENCH_CORRUPT") == "headline":
        dah[len(dah) - 1, 7] ^= 0x10
    n = ds.n
    _, hrr, hcr, hdah, hst = da.extend_batch(batch_ods.reshape(-1), [ds.k] * n, ctx)
    bad_dah = int((hdah != dah).any(axis=1).sum())
    bad_roots = sum(int(not (np.array_equal(hrr[i], rr[i]) and np.array_equal(hcr[i], cr[i]))) for i in range(n))
    ok = bad_dah == 0 and bad_roots == 0 and bool((st == 0).all()) and bool((hst == 0).all())
    _fail(dist, not ok, local, f"headline bit-exact check ({bad_dah} DAHs, {bad_roots} root sets differ)")
    return {"bit_exact": ok, "squares": n, "dah_mismatches": bad_dah, "root_mismatches": bad_roots,
            "against": "dagpu_extend_batch (host API, unsliced) on the same host ODS",
            "pipeline_slices": int(os.environ.get("DAGPU_PIPE_SLICES", "0")) or "default"}


def bench_e2e(ctx, local, k, host_ods, steps, total=256):
    """C2 end to end through the drop-in host API
    `dagpu_extend_batch`: ODS batches start in page-locked host memory (as a
    caller that allocates them with dagpu_host_alloc / registers them would),
    the library pipelines them in 128 MiB chunks (H2D on a copy stream while
    the previous chunk is extended) and returns roots + DAHs to host memory.
    `total` squares per call (the batch repeated).  Not the headline `value`."""
    from celestia_da import da
    B = min(host_ods.shape[0], total)
    host_ods = host_ods[:B]
    reps = max(1, total // B)
    n = B * reps
    pin = torch.empty((n, host_ods.shape[1]), dtype=torch.uint8).pin_memory()
    for r in range(reps):
        pin[r * B:(r + 1) * B].copy_(torch.from_numpy(host_ods))
    arr = pin.numpy()
    ks = [k] * n
    _, _, _, dah0, st0 = da.extend_batch(arr, ks, ctx)
    t0 = time.perf_counter()
    for _ in range(steps):
        _, _, _, dah, st = da.extend_batch(arr, ks, ctx)
    el = time.perf_counter() - t0
    ok = bool((dah == dah0).all() and (st == 0).all() and (reps == 1 or (dah[:B] == dah[B:2 * B]).all()))
    return {"squares_per_s": n * steps / el, "ms_per_call": el / steps * 1e3, "squares_per_call": n,
            "h2d_bytes_per_square": k * k * SHARE, "d2h_bytes_per_square": 2 * 2 * k * 90 + 32,
            "h2d_GBps": n * steps * k * k * SHARE / el / 1e9, "dah_repeat_ok": ok,
            "note": "dagpu_extend_batch on pinned host ODS: chunked H2D on a copy stream overlapping the "
                    "previous chunk's kernels; roots+DAHs back to host"}


def bench_construct(ctx, calls=20):
    """Native square construction (pkg/square/square.go:22-63 ->
    dagpu_square_construct, host C++): a synthetic full block (2,000 normal txs
    + 2,000 blob txs -> a 128x128 square), the C call alone on pre-packed tx
    buffers (median of `calls`), and txs -> DataHash as app/extend_block.go:14-22
    runs it per block (construct, then dagpu_extend_shares roots only).  Checked:
    the ODS equals the Python mirror's (celestia_da/square.py) once."""
    import ctypes

    from celestia_da import _abi, da, square, synth
    L = ctx._L
    txs = synth.block_txs(2000, 2000, 4242)
    buf, lens = square._pack(txs)
    cap = 128 * 128 * SHARE
    ods = da.PinnedBuffer(cap)
    k = ctypes.c_uint32(0)
    rr, cr, dah = np.empty(256 * 90, np.uint8), np.empty(256 * 90, np.uint8), np.empty(32, np.uint8)
    t_c, t_e2e = [], []
    for i in range(calls + 2):
        t0 = time.perf_counter()
        rc = L.dagpu_square_construct(None, _abi.addr(buf), _abi.addr(lens), len(txs), 128, 64, ods.ptr, cap,
                                      ctypes.addressof(k))
        t1 = time.perf_counter()
        if rc != 0:
            raise SystemExit(f"dagpu_square_construct: status {rc}")
        kk = int(k.value)
        rc = L.dagpu_extend_shares(ctx.handle, ods.ptr, kk * kk, SHARE, 0, _abi.addr(rr), _abi.addr(cr),
                                   _abi.addr(dah))
        t2 = time.perf_counter()
        if rc != 0:
            raise SystemExit(f"dagpu_extend_shares after construct: status {rc}")
        if i >= 2:
            t_c.append((t1 - t0) * 1e3)
            t_e2e.append((t2 - t0) * 1e3)
    want = np.frombuffer(b"".join(square.construct(txs).square_bytes()), np.uint8)
    same = bool(kk == 128 and np.array_equal(ods.array[:kk * kk * SHARE], want))
    ods.close()
    if not same:
        raise SystemExit("native square construction differs from the Python mirror")
    return {"k": kk, "txs": len(txs), "construct_ms_p50": float(np.median(t_c)),
            "construct_ms_max": float(np.max(t_c)), "txs_to_dah_ms_p50": float(np.median(t_e2e)),
            "matches_python_mirror": same,
            "note": "dagpu_square_construct on pre-packed tx buffers (C++ host code, no GPU); "
                    "txs_to_dah = construct + dagpu_extend_shares (roots + DAH) of the square"}


def bench_single(ctx, ks=(64, 128), calls=60, trace=True):
    """Drop-in latency of ONE square per call, as the production callers use it
    (app/process_proposal.go:147-161, app/prepare_proposal.go:95-107):
    dagpu_extend_shares from page-locked host shares, with eds_out NULL (roots +
    DAH only), with the whole EDS returned to page-locked host memory, and to
    pageable memory (an ordinary Go slice: the copies then run after the kernel
    chain is queued, synchronously on the calling thread).
    p50/p99 over `calls` calls after 5 warm-up calls, per k."""
    from celestia_da import _abi, da, synth

    L = ctx._L
    res = {}
    if trace:
        L.dagpu_profile_enable(ctx.handle, 2)
    for k in ks:
        w = 2 * k
        src = da.PinnedBuffer(k * k * SHARE)
        src.array[:] = synth.blob_squares(k, 0xC0FFEE + k, 0, 1).reshape(-1)
        edsb = da.PinnedBuffer(w * w * SHARE)
        rr = np.empty(w * 90, np.uint8)
        cr = np.empty(w * 90, np.uint8)
        dah = np.empty(32, np.uint8)
        r = {}
        stages = np.zeros(len(_abi.STAGES), np.float32)
        pageable = np.empty(w * w * SHARE, np.uint8)  # an ordinary (Go-heap-like) caller buffer
        pageable.fill(0)
        for mode, eds_ptr in (("roots_only", 0), ("with_eds", edsb.ptr), ("with_eds_pageable", _abi.addr(pageable))):
            lat, tl = [], []
            for i in range(5 + calls):
                t0 = time.perf_counter()
                rc = L.dagpu_extend_shares(ctx.handle, src.ptr, k * k, SHARE, eds_ptr, _abi.addr(rr),
                                           _abi.addr(cr), _abi.addr(dah))
                t = time.perf_counter() - t0
                if rc != 0:
                    raise SystemExit(f"dagpu_extend_shares k={k}: status {rc}")
                if i >= 5:
                    lat.append(t * 1e3)
                    if trace:  # stage timeline of this call (HIP events, read after it returned)
                        L.dagpu_profile_stages(ctx.handle, _abi.addr(stages))
                        tl.append(stages.copy())
            lat = np.array(lat)
            r[mode] = {"p50_ms": float(np.percentile(lat, 50)), "p99_ms": float(np.percentile(lat, 99)),
                       "mean_ms": float(lat.mean())}
            if trace:
                tl = np.array(tl)
                order = np.argsort(lat)
                name = lambda row: {s: round(float(v), 4) for s, v in zip(_abi.STAGES, row) if v >= 0}  # noqa: E731
                r[mode]["stages_median_ms"] = name(np.median(tl, axis=0))
                r[mode]["stages_slowest"] = [dict(name(tl[j]), wall_ms=round(float(lat[j]), 4))
                                             for j in order[-3:][::-1]]
        want = da.new_data_availability_header(da.extend_shares(src.array.reshape(k * k, SHARE), ctx)).hash()
        r["dah_ok"] = dah.tobytes() == want
        res[str(k)] = r
        src.close()
        edsb.close()
        if not r["dah_ok"]:
            raise SystemExit(f"single-square DAH mismatch at k={k}")
    if trace:
        L.dagpu_profile_enable(ctx.handle, 0)
    return res


REPLAY_SEED = 0x5EED_B10C
HEADLINE_SEED = 1_000_003


def cgroup_cpus():
    """CPUs granted by the cgroup v2 CPU quota (None when unlimited)."""
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            return int(quota) / int(period)
    except (OSError, ValueError):
        pass
    return None


def host_threads() -> int:
    """CPU threads this process may use: the affinity mask, capped by a cgroup
    CPU quota when one is set (a GPU box's share is smaller than the machine
    `nproc` reports), and split between the ranks of this node."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n // int(os.environ.get("LOCAL_WORLD_SIZE", "1")))


def _fail(dist, bad: bool, local: int, what: str):
    """Make a failed check fatal on EVERY rank (max-reduce of the flag)."""
    flag = max_over_ranks(dist, 1.0 if bad else 0.0, local)
    if flag:
        print(f"FATAL: {what} failed (rank-local: {bad})", file=sys.stderr, flush=True)
        raise SystemExit(3)


def bench_replay(dist, rank, world, local, ctx, ds, n_blocks, dump=None, numa_report=None):
    """configs[4] block replay (app/extend_block.go:14-22, per block as in
    app/test/integration_test.go:355-379): n_blocks consecutive DISTINCT k x k
    squares (seeded, csrc/synth.cpp), contiguous shards per rank.

    Each rank generates its shard into page-locked host memory (untimed) and
      1. host-streamed: pushes the whole shard through the drop-in host API
         dagpu_extend_batch (chunked H2D on a copy stream overlapping the
         previous chunk's kernels) -> roots + DAHs in host memory;
      2. device-resident: the shard uploaded to HBM (untimed), extended
         ds.n squares per launch sequence -> DAHs in HBM;
    then every DAH is all-gathered to every rank.  Checks, all fatal on every
    rank: status, host-streamed == device-resident DAHs, each rank's gathered
    slice against that rank's SHA-256 digest of its own DAHs (all-gathered
    separately), and rank 0 regenerates the first and last block of EVERY
    rank's shard and recomputes them through the single-square host path
    (dagpu_extend_shares).  DAGPU_BENCH_CORRUPT=replay-gather|replay-compute
    injects a wrong DAH to prove the checks fire."""
    import hashlib

    from celestia_da import da, replay, synth

    corrupt = os.environ.get("DAGPU_BENCH_CORRUPT", "")
    k, B = ds.k, ds.n
    ob = k * k * SHARE
    mine = replay.shard_range(n_blocks, rank, world)
    n = len(mine)
    per_rank = (n_blocks + world - 1) // world
    dev = ds.eds.device
    t0 = time.perf_counter()
    host = da.PinnedBuffer(max(n, 1) * ob)
    alloc_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    synth.blob_squares(k, REPLAY_SEED, mine.start, n, out=host.array, threads=host_threads())
    gen_s = time.perf_counter() - t0

    # 1. host-streamed through dagpu_extend_batch
    barrier(dist)
    t0 = time.perf_counter()
    _, _, _, dah_h, st_h = da.extend_batch(host.array[:n * ob], [k] * n, ctx)
    el_h = max_over_ranks(dist, time.perf_counter() - t0, local)
    bad = bool((st_h != 0).any())

    # 2. device-resident distinct squares
    free, _ = torch.cuda.mem_get_info(dev)
    dev_res = None
    if n * ob < 0.8 * free:
        shard = torch.empty((max(n, 1), ob), dtype=torch.uint8, device=dev)
        shard[:n].copy_(torch.from_numpy(host.array[:n * ob]).view(n, ob))
        out = torch.zeros((per_rank, 32), dtype=torch.uint8, device=dev)
        st = torch.zeros((per_rank,), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream()
        torch.cuda.synchronize()
        barrier(dist)
        t0 = time.perf_counter()
        for off in range(0, n, B):
            m = ds.extend_from(shard[off:off + min(B, n - off)], stream)
            out[off:off + m].copy_(ds.dah[:m], non_blocking=True)
            st[off:off + m].copy_(ds.status[:m], non_blocking=True)
        torch.cuda.synchronize()
        el_d = max_over_ranks(dist, time.perf_counter() - t0, local)
        del shard
        bad = bad or bool((st[:n] != 0).any())
        dev_res = {"squares_per_s": n_blocks / el_d, "seconds": el_d,
                   "note": f"shard resident in HBM, {B} squares per launch sequence"}
        if corrupt == "replay-compute" and rank == world - 1 and n:
            out[0, 0] ^= 1
        bad = bad or not bool(torch.equal(out[:n].cpu(), torch.from_numpy(dah_h)))
    else:
        out = torch.zeros((per_rank, 32), dtype=torch.uint8, device=dev)
        out[:n].copy_(torch.from_numpy(dah_h))

    # every DAH to every rank + per-rank digests of the local DAHs
    dig = torch.frombuffer(bytearray(hashlib.sha256(out[:n].cpu().numpy().tobytes()).digest()),
                           dtype=torch.uint8).to(dev)
    allg = all_gather_rows(dist, world, out).cpu()
    digs = all_gather_rows(dist, world, dig.view(1, 32)).cpu()
    if corrupt == "replay-gather" and rank == 0:
        allg[(world - 1) * per_rank, 0] ^= 1
    for r in range(world):
        n_r = len(replay.shard_range(n_blocks, r, world))
        got = allg[r * per_rank:r * per_rank + n_r].numpy().tobytes()
        bad = bad or hashlib.sha256(got).digest() != bytes(digs[r].numpy())
    sampled = {}
    if rank == 0:  # first and last block of every rank's shard, recomputed independently
        for r in range(world):
            sh = replay.shard_range(n_blocks, r, world)
            for b in sorted({sh.start, sh.stop - 1}) if len(sh) else []:
                sq = synth.blob_squares(k, REPLAY_SEED, b, 1)[0].reshape(k * k, SHARE)
                want = da.new_data_availability_header(da.extend_shares(sq, ctx)).hash()
                got = bytes(allg[r * per_rank + (b - sh.start)].numpy())
                sampled[b] = got.hex()
                bad = bad or got != want
    host.close()
    _fail(dist, bad, local, "block replay DAH check")
    numa_all = [numa_report]
    if dist is not None:
        numa_all = [None] * world
        dist.all_gather_object(numa_all, numa_report)
    if dump and rank == 0:
        json.dump({"k": k, "seed": REPLAY_SEED, "blocks": n_blocks, "sampled_dah": sampled},
                  open(dump, "w"))
    return {"blocks": n_blocks, "distinct_squares": n_blocks, "per_rank": per_rank,
            "host_streamed": {"squares_per_s": n_blocks / el_h, "seconds": el_h,
                              "h2d_GBps_per_rank": n * ob / el_h / 1e9,
                              "note": "page-locked host ODS -> dagpu_extend_batch (chunked H2D on a "
                                      "copy stream) -> roots + DAHs in host memory"},
            "device_resident": dev_res,
            "gen_seconds": gen_s, "pin_alloc_seconds": alloc_s,
            "numa": numa_all,
            "bit_exact": True,
            "checks": "status; host-streamed == device-resident DAHs; every rank's gathered slice vs "
                      "its own digest; first+last block of every shard recomputed by rank 0 "
                      "(dagpu_extend_shares); any failure exits non-zero on all ranks"}


def bench_split(dist, rank, world, local, ctx, k, steps, warmup):
    """configs[4] stress: ONE k x k square split over all `world` ranks (rows ->
    one all-to-all -> column slabs; celestia_da.split).  Returns squares/s, the
    per-square time (max over ranks) and whether the DAH equals the single-GPU
    path's DAH for the same square."""
    from celestia_da import split, synth
    from celestia_da.device import DeviceSquares

    dev = torch.device("cuda", local)
    ods = synth.random_blob_square(k, 512_000 + k).reshape(-1)
    rows = k // world
    mine = torch.from_numpy(ods[rank * rows * k * SHARE:(rank + 1) * rows * k * SHARE].copy()).to(dev)
    part = split.SplitPart(k, world, rank, ctx, dev)
    for _ in range(warmup):
        _, _, dah = split.extend_split_distributed(dist, part, mine)
    torch.cuda.synchronize()
    barrier(dist)
    t0 = time.perf_counter()
    for _ in range(steps):
        _, _, dah = split.extend_split_distributed(dist, part, mine)
    torch.cuda.synchronize()
    barrier(dist)
    el = max_over_ranks(dist, time.perf_counter() - t0, local)
    # one profiled pass (HIP events around each launch of this rank): the RS
    # passes' roofline; the timed steps above run unprofiled
    L = ctx._L
    L.dagpu_profile_enable(ctx.handle, 1)
    L.dagpu_profile_read(ctx.handle, None, None, 1)
    split.extend_split_distributed(dist, part, mine)
    torch.cuda.synchronize()
    L.dagpu_profile_enable(ctx.handle, 0)
    from celestia_da import _abi
    tot = np.zeros(len(_abi.PROFILE_KERNELS), np.float64)
    cnt = np.zeros(len(_abi.PROFILE_KERNELS), np.uint64)
    L.dagpu_profile_read(ctx.handle, _abi.addr(tot), _abi.addr(cnt), 1)
    prof = {n: float(tot[i]) for i, n in enumerate(_abi.PROFILE_KERNELS) if cnt[i]}
    # this rank's column pass: 2k/P column vectors, each k shards read + k written
    enc = gf16_kernel_names(k)[0]
    roof = stress_roofline("rs_col (GF(2^16) column encode)", (2 * k // world) * 2 * k * SHARE,
                           prof.get("rs_col"), int(cnt[1]), enc or f"leo16 encode k={k}",
                           f"{2 * k // world} column vectors x (k read + k written) x 512 B") if cnt[1] else None
    ok = True
    if rank == 0:  # same square through the ordinary single-GPU pipeline
        ds = DeviceSquares(k, 1, device=local, ctx=ctx)
        ds.ods[0].copy_(torch.from_numpy(ods))
        ds.extend()
        torch.cuda.synchronize()
        got = dah.cpu().clone()
        if os.environ.get("DAGPU_BENCH_CORRUPT") == "split":
            got[0] ^= 1
        ok = bool(torch.equal(ds.dah[0].cpu(), got))
        del ds
    del part
    torch.cuda.empty_cache()
    _fail(dist, not ok, local, f"split square k={k}: DAH differs from the single-GPU pipeline")
    return {"k": k, "parts": world, "squares_per_s": steps / el, "ms_per_square": el / steps * 1e3,
            "rs_gbs": rs_bytes(k) * steps / el / 1e9, "dah_matches_single_gpu": ok,
            "kernel_ms_profiled_pass": prof, "roofline": roof,
            "collective": f"all_to_all_single over {world} ranks, {dist.get_backend() if dist else 'none'}"}


def bench_split_main(args):
    dist, rank, world, local = dist_init()
    torch.cuda.set_device(local)
    from celestia_da import da

    ctx = da.Context(local)
    res = {str(k): bench_split(dist, rank, world, local, ctx, k, args.steps, args.warmup) for k in args.split_k}
    if rank == 0:
        first = res[str(args.split_k[-1])]
        print(json.dumps({"metric": "oversized square EDS+DAH squares/sec (configs[4] stress, split over all GPUs)",
                          "value": first["squares_per_s"], "unit": "squares/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup, "ms_per_step": first["ms_per_square"],
                          "higher_is_better": True, "scaling": "strong", "dtype": "u8",
                          "data": "synthetic random-namespace blob shares", "config": {
                              "workload": "configs[4] stress square split with all-to-all", "k": args.split_k,
                              "parallelism": f"rows/columns over {world} GPU(s)"}, "split": res}), flush=True)
    ctx.close()
    if dist is not None:
        dist.destroy_process_group()


MIXED_SEED = 4096


def mixed_batch(ctx, dev=0):
    """configs[2] input: 4096 squares, k = 2^u with u ~ U{0..7} (seeded), every
    square distinct (seeded run MIXED_SEED + k, csrc/synth.cpp), grouped by k
    into device-resident batches, each ODS in Q0 of its EDS buffer (the layout
    of the headline step).  Returns (ks, {k: DeviceSquares}, {k: host ODS})."""
    from celestia_da import synth
    from celestia_da.device import DeviceSquares

    rng = np.random.default_rng(MIXED_SEED)
    ks = [int(2 ** u) for u in rng.integers(0, 8, 4096)]
    groups, hosts = {}, {}
    for k in sorted(set(ks)):
        n = ks.count(k)
        ds = DeviceSquares(k, n, device=dev, ctx=ctx, in_place=True)
        hosts[k] = synth.blob_squares(k, MIXED_SEED + k, 0, n, threads=host_threads())
        ds.load_ods(hosts[k])
        groups[k] = ds
    return ks, groups, hosts


def run_mixed(ctx, steps, warmup):
    """configs[2]: a batch of 4096 distinct mixed-size squares (k = 2^u,
    u ~ U{0..7}, seeded), one launch sequence per distinct k per step, each k
    group on its own stream.  bit_exact (fatal if false): the concurrent run's
    DAHs equal the one-stream run's and the host API's (dagpu_extend_batch) for
    every square, every status is 0."""
    from celestia_da import da

    ks, groups, hosts = mixed_batch(ctx)
    # Squares of different k are independent: each k group runs on its own
    # stream (forked from and joined back to the current one), so the small-k
    # groups' latency-bound tree tops overlap the large-k groups' work.
    streams = {k: torch.cuda.Stream() for k in groups}

    def step(concurrent):
        cur = torch.cuda.current_stream()
        for k, ds in groups.items():
            if concurrent:
                streams[k].wait_stream(cur)
                ds.extend(streams[k])
            else:
                ds.extend(cur)
        if concurrent:
            for st in streams.values():
                cur.wait_stream(st)

    def timed(concurrent):
        for _ in range(warmup):
            step(concurrent)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(concurrent)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def results():
        return {k: (ds.dah.cpu().clone(), ds.status.cpu().clone()) for k, ds in groups.items()}

    torch.cuda.synchronize()
    serial = timed(False)
    r_serial = results()
    for ds in groups.values():
        ds.dah.zero_()
        ds.status.fill_(-1)
    el = timed(True)
    r_conc = results()
    ok = True
    for k in groups:
        _, _, _, hdah, hst = da.extend_batch(hosts[k].reshape(-1), [k] * groups[k].n, ctx)
        ok = ok and bool((r_serial[k][1] == 0).all() and (r_conc[k][1] == 0).all() and (hst == 0).all())
        ok = ok and torch.equal(r_serial[k][0], r_conc[k][0]) and (r_conc[k][0].numpy() == hdah).all()
    if not ok:
        print("FATAL: mixed batch results differ between runs / the host API", file=sys.stderr)
        raise SystemExit(3)
    comp = sum(sum(compressions(k)) for k in ks)
    del groups
    torch.cuda.empty_cache()
    return {"squares_per_s": 4096 * steps / el, "ms_per_step": el / steps * 1e3, "steps": steps,
            "sha256_compressions_per_s": comp * steps / el, "streams": len(streams),
            "one_stream_ms_per_step": serial / steps * 1e3, "bit_exact": bool(ok),
            "squares_per_k": {str(k): ks.count(k) for k in sorted(set(ks))}}


def bench_mixed(args):
    from celestia_da import da

    torch.cuda.set_device(0)
    r = run_mixed(da.Context(0), args.steps, args.warmup)
    out = {"metric": "mixed-batch squares/sec (4096 squares, k=1..128)", "value": r["squares_per_s"],
           "unit": "squares/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": r["ms_per_step"], "higher_is_better": True, "dtype": "u8",
           "data": "synthetic random-namespace blob shares, 4096 distinct squares",
           "sha256_compressions_per_s": r["sha256_compressions_per_s"], "streams": r["streams"],
           "one_stream_ms_per_step": r["one_stream_ms_per_step"], "bit_exact": r["bit_exact"],
           "config": {"workload": "configs[2]: 4096 mixed squares per step", "squares_per_k": r["squares_per_k"]}}
    print(json.dumps(out), flush=True)


REPAIR_SEED = 777


def run_repair(ctx, k, B, steps, warmup, distinct=None, pattern="subgrid", slices=1):
    """configs[3]: rsmt2d Repair of B distinct k x k squares with the maximal
    recoverable erasure pattern (a random k x k sub-grid kept, 3k^2 cells
    erased; pattern "q3": the k x k sub-grid of parity rows and parity columns,
    which the reverse fill rebuilds), every row/column root re-verified.  Timed with HIP events around
    the repair only (each step first restores the damaged input).  bit_exact
    (fatal if false): the repaired EDS equals the extended one, status 0.
    slices > 1: the batch as that many started repairs (dagpu_repair_start,
    each crossword on its own worker thread and stream), joined back to the
    timed stream, so that one slice's round trips overlap another's kernels."""
    from celestia_da import synth
    from celestia_da.device import DeviceSquares

    w = 2 * k
    ds = DeviceSquares(k, B, ctx=ctx)
    nd = min(distinct or B, B)
    host = synth.blob_squares(k, REPAIR_SEED, 0, nd, threads=host_threads())
    ds.load_ods(np.stack([host[i % nd] for i in range(B)]))
    ds.extend()
    rng = np.random.default_rng(5)
    pres = np.zeros((B, w, w), np.uint8)
    for i in range(B):
        if pattern == "q3":
            pres[i][k:, k:] = 1
        else:
            pres[i][np.ix_(rng.choice(w, k, replace=False), rng.choice(w, k, replace=False))] = 1
    pres_t = torch.from_numpy(pres.reshape(B, -1)).cuda()
    ref = ds.eds.clone()
    damaged = (ds.eds.view(B, w * w, 512) * pres_t.view(B, w * w, 1)).view(B, -1).clone()
    present = pres_t.clone()
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    cut = [B * j // slices for j in range(slices + 1)]
    if slices == 1:
        ws = ds.repair_workspace()
    else:
        wss = [ds.repair_workspace(cut[j + 1] - cut[j]) for j in range(slices)]
        ws = None

    def repair_step():
        if slices == 1:
            ds.repair(present, status, ws)
            return
        hs = [ds.repair_start(present, status, wss[j], first=cut[j], count=cut[j + 1] - cut[j])
              for j in range(slices)]
        for h in hs:
            ds.repair_join(h)

    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for i in range(warmup + steps):
        ds.eds.copy_(damaged)
        present.copy_(pres_t)
        if i >= warmup:
            ev[i - warmup][0].record()
        repair_step()
        if i >= warmup:
            ev[i - warmup][1].record()
    torch.cuda.synchronize()
    ok = bool(torch.equal(ds.eds, ref)) and int(status.abs().sum()) == 0
    if not ok:
        print(f"FATAL: repair k={k} did not restore the extended square", file=sys.stderr)
        raise SystemExit(3)
    ms = sum(a.elapsed_time(b) for a, b in ev) / steps
    # one more step, profiled (HIP events around every decode / fill launch),
    # for the decoder's roofline; checked like the timed ones
    from celestia_da import _abi
    L = ctx._L
    ds.eds.copy_(damaged)
    present.copy_(pres_t)
    torch.cuda.synchronize()
    L.dagpu_profile_enable(ctx.handle, 1)
    L.dagpu_profile_read(ctx.handle, None, None, 1)
    repair_step()
    torch.cuda.synchronize()
    L.dagpu_profile_enable(ctx.handle, 0)
    tot = np.zeros(len(_abi.PROFILE_KERNELS), np.float64)
    cnt = np.zeros(len(_abi.PROFILE_KERNELS), np.uint64)
    L.dagpu_profile_read(ctx.handle, _abi.addr(tot), _abi.addr(cnt), 1)
    sched = ctx.repair_stats()
    if not (torch.equal(ds.eds, ref) and int(status.abs().sum()) == 0):
        print(f"FATAL: profiled repair k={k} did not restore the extended square", file=sys.stderr)
        raise SystemExit(3)
    idec = _abi.PROFILE_KERNELS.index("decode")
    ifil = _abi.PROFILE_KERNELS.index("repair_fill")
    prof = {"decode_ms": float(tot[idec]), "decode_launches": int(cnt[idec]),
            "fill_ms": float(tot[ifil]), "fill_launches": int(cnt[ifil]), "schedule": sched}
    # a decoded vector reads its k given shards and writes its k missing ones
    dec_name = "leo8_decode128_sliced_kernel" if k == 128 else gf16_kernel_names(k)[1]
    roof = stress_roofline(f"decode ({dec_name})", sched["decodes"] * 2 * k * SHARE, prof["decode_ms"],
                           prof["decode_launches"], dec_name,
                           f"{sched['decodes']} decoded vectors x (k read + k written) x 512 B") \
        if sched["decodes"] and prof["decode_launches"] else None
    del ds, ref, damaged, ws
    torch.cuda.empty_cache()
    return {"k": k, "squares": B, "pattern": pattern, "slices": slices, "squares_per_s": B / (ms * 1e-3),
            "ms_per_step": ms,
            "steps": steps, "bit_exact": ok, "decode_gbs": rs_bytes(k) * B / (ms * 1e-3) / 1e9,
            "profiled_pass": prof, "roofline": roof}


def bench_repair(args):
    from celestia_da import da

    torch.cuda.set_device(0)
    r = run_repair(da.Context(0), args.k, args.batch, args.steps, args.warmup, args.distinct, args.pattern,
                   args.repair_slices)
    kept = "Q3 kept" if args.pattern == "q3" else "random k x k sub-grid kept"
    out = {"metric": f"Repair squares/sec (k={args.k}, maximal erasure, roots re-verified)",
           "value": r["squares_per_s"], "unit": "squares/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": r["ms_per_step"], "higher_is_better": True,
           "bit_exact": r["bit_exact"], "decode_gbs": r["decode_gbs"],
           "config": {"workload": f"configs[3]: {args.batch} squares {args.k}x{args.k}, 3k^2 cells erased each "
                                  f"({kept})"}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
