#!/usr/bin/env python
"""bench.py -- RGB-D frames/s of the MI355X dense-SLAM hot path.

Headline (N = 1, BASELINE.json configs[1]): the synthetic 640x480 RGB-D stream
with known poses (1000 distinct frames, resident in HBM before the timed region)
integrated into an 8 mm / 16^3-block VoxelBlockGrid (tsdf f32, weight u16,
colour u16 -- the slam::Model layout): per frame block touch + hash activation
+ per-voxel TSDF / weight / colour update. A "step" is one batch of `--batch`
frames (default 8000 = eight passes over the stream, so that the driver's 20
timed steps last more than a second); every frame does the full per-frame work, the
uint16 weights stay far below their range (a voxel is seen by <= 183 frames of
a pass).

Multi-GPU (`--gpus N`; launched by torchrun, or self-spawned when WORLD_SIZE is
unset): one process per GPU over RCCL, STRONG scaling in both schemes -- the
job is the same stream (`--batch` frames per step in total) whatever N is.
  blocks (headline): every rank sees every frame and runs the cheap block
        touch, but activates / integrates only the blocks it owns; no
        data-path collective; the union of the ranks' grids is bit-identical
        to the single-GPU grid.
  frames (`config.frame_sharded`, beside it): rank r integrates frames r,
        r + N, ... of the same stream into a private grid; INSIDE the timed
        region the owner-partitioned exchange (all-to-all of block IDs and
        voxel rows to the owning rank, folded in by the running-mean merge
        kernel: o3dmi_vbg_merge_frame_sharded, RCCL inside the library) turns
        the N partial models into one, laid out as the blocks scheme leaves
        it.
`--dist-backend gloo` (or O3DMI_DIST_BACKEND) runs the same code with several
ranks sharing whatever GPUs are visible (rank -> device rank % device_count):
a functional dry run of the N > 1 path on a 1-GPU box, not a scaling number
(`config.dry_run`).

Prints ONE JSON line (rank 0). A plain run (`--gpus N --steps K --warmup W`)
sets up, warms up, times the K steps and prints the contract fields (metric,
value, unit, ms_per_step, ...) and a small `config`; before it,
`--dump-outputs DIR` writes the grid the timed steps built (dump_outputs).
With `--full` the line also holds
  cold_pass_frames_per_s, drop_in
                one pass over the stream into an empty grid; the reference's
                call shapes (two calls or one call per frame, host-fed batch).
  roofline      dominant kernel (FrameStepKernel): SURVEY 8(d) algorithmic
                bytes / HIP-event kernel time (`frac`), counter-measured fabric
                bytes / the same time (`frac_hbm`: FETCH_SIZE x2 + WRITE_SIZE,
                factors calibrated in profiles/r2a_hbm_calibration.json) and the
                share of SIMD cycles that issue vector-ALU work (`frac_valu`,
                SQ counters). The counters are collected live by rocprofv3
                passes over a short run of this same script (rank 0, N = 1).
  secondary     the ICP half of BASELINE's metric: configs[0] (point-to-plane
                ICP on two 100k-point clouds) and the configs[2] tracking loop
                (multi-scale ICP + integrate + ray cast) at 1280x720 and
                640x480, each with its 8(d) byte accounting and the CPU oracle
                timed beside it.
  cpu_baseline  Open3D's own DepthTouchCPU / IntegrateCPU bodies (oracle/_ref)
                on this host's cores over a bounded sample of the same stream.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

VOXEL = 0.008
RES = 16
TRUNC = 8.0
DEPTH_SCALE = 1000.0
DEPTH_MAX = 3.0
W, H = 640, 480
N_UNIQUE = 1000           # configs[1]: the 1000-frame stream
HBM_PEAK_GBS = 8000.0     # MI355X_MICROARCH.md: 8 TB/s spec
# u16 grid with colour, read+write per voxel
BYTES_PER_BLOCK = 4096 * 24
IMAGE_BYTES = W * H * 2 + W * H * 3
BLOCK_HEADER_BYTES = 16   # buf index + key
N_SIMD = 256 * 4
# VALU issue cost of a wave64 instruction on gfx950, MEASURED (tools/
# calib_valu.hip, profiles/r5b_valu_calibration.json): 2.4 cycles for plain
# float32 mul / add / fma, integer add, shift, move; 4.3 for packed float32,
# conversions, compares, selects, truncation, 24-bit multiplies; 8.3 for
# v_rcp_f32. No counter tells the classes apart (SQ_ACTIVE_INST_VALU reads 1
# per instruction whatever its class, 2 for a transcendental); the integrate
# role's mix on the path of a frame that updates its voxels, walked through
# its ISA and priced per class (tools/valu_cost.py, profiles/r5_valu_mix.txt:
# 118 instructions, 415 cycles per wave and frame), averages:
VALU_FULL, VALU_HALF = 2.4, 4.3
VALU_CYCLES_PER_INST = 3.5


def valu_fractions(insts, simd_cycles):
    """SQ_INSTS_VALU of a launch -> share of the SIMDs' cycles that issue
    vector-ALU work: at the kernel's own instruction mix, and the bounds the
    two cost classes put on any mix."""
    if not insts or not simd_cycles:
        return None, None
    per = insts / (N_SIMD * simd_cycles)
    return per * VALU_CYCLES_PER_INST, [per * VALU_FULL, per * VALU_HALF]
N_XCD = 8
KERNEL = "FrameStepKernel"
METRIC = ("RGB-D frames/s, TSDF integrate with known poses (configs[1]: touch "
          "+ activate + integrate into an 8 mm / 16^3 VoxelBlockGrid); the ICP "
          "+ integrate + ray-cast loop (configs[2]) is in loop_frames_per_s "
          "(its first tracked frame untimed as warm-up; the whole run in "
          "loop_frames_per_s_with_first_frame)")
DUMP_BLOCKS = 384         # blocks of the grid written by --dump-outputs


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8000,
                    help="frames per step (per GPU)")
    ap.add_argument("--block-count", type=int, default=50000,
                    help="initial hash capacity: the reference's advised map "
                         "size (docs/tutorial/t_reconstruction_system/"
                         "voxel_block_grid.rst: 50 000; the stream creates "
                         "5 745 blocks). Rounds 1-3 needed 524 288 here for "
                         "the run-ahead bound of 12-frame groups; since round "
                         "4 groups are issued on an estimate of what they add "
                         "(within 0.4 % of the 524 288 figure)")
    ap.add_argument("--frames-per-launch", type=int, default=12,
                    help="consecutive frames applied per launch to register-"
                         "resident blocks (1..16); results are identical. 12: "
                         "128.4 k frames/s against 125.2 k for 8 and 126.1 k "
                         "for 16 on the same box")
    ap.add_argument("--event-stride", type=int, default=16,
                    help="bracket every n-th integrate launch with HIP events "
                         "(0 = none; the roofline is then not measured)")
    ap.add_argument("--sharding", choices=["frames", "blocks"],
                    default="frames",
                    help="multi-GPU scheme of the headline value at N > 1. "
                         "`frames` (default since round 6; the split BASELINE's "
                         "north star describes): rank r integrates frames r, "
                         "r + N, ... into a private grid, one owner-"
                         "partitioned all-to-all merge closes the timed "
                         "region; block set and weights equal the single "
                         "stream's, TSDF within 1e-4, colour within the "
                         "rounding of the running mean. `blocks`: every rank "
                         "sees every frame and integrates the blocks it owns "
                         "(sliced touch + one all-gather per chunk); the "
                         "union of the grids is the single stream's bit for "
                         "bit. Worst-rank emulation on one GPU (profiles/"
                         "r6d_emu_all_ranks.txt): frames 1.99x / 3.8x / 6.9x "
                         "at 2 / 4 / 8 ranks before the merge, blocks 1.91x / "
                         "3.03x / 4.75x")
    ap.add_argument("--dist-backend", choices=["nccl", "gloo"],
                    default=os.environ.get("O3DMI_DIST_BACKEND", "nccl"),
                    help="torch.distributed backend; gloo = functional dry "
                         "run with ranks sharing the visible GPUs")
    ap.add_argument("--emulate-world", type=int, default=0,
                    help="diagnostics, single process: run ONE rank's share "
                         "of an N-rank job on this GPU (no collective) to "
                         "read the per-rank cost of both schemes")
    ap.add_argument("--emulate-rank", default="all",
                    help="which rank of --emulate-world: a number, or `all` "
                         "(default): the ranks 0..N-1 one after the other; "
                         "`value` is then the WORST rank's (a job lasts as "
                         "long as its slowest rank), the spread is in "
                         "config.emulated_ranks_ms_per_step")
    ap.add_argument("--allow-transport-fallback", action="store_true",
                    help="N > 1 on the nccl backend: if the library's own "
                         "RCCL communicator cannot be made on every rank, "
                         "fall back to the torch.distributed transport "
                         "instead of failing the run (config.transport says "
                         "which one carried the collectives)")
    ap.add_argument("--touch", choices=["sliced", "replicated"],
                    default="sliced",
                    help="block-ownership scheme at N > 1: `sliced` = rank r "
                         "touches its band of ray tiles, candidate keys are "
                         "all-gathered per chunk of 16 launches, blocks are "
                         "integrated from the raw images (SURVEY 8(e) as "
                         "specified); `replicated` = every rank runs the "
                         "whole front role (rounds 1-3)")
    ap.add_argument("--force-sliced", action="store_true",
                    help="diagnostics: the sliced path (band touch, gathered "
                         "records, raw-image integrate role) on ONE rank")
    ap.add_argument("--depth-only", action="store_true",
                    help="diagnostics: grid without colour (tsdf + weight)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-pmc", action="store_true",
                    help="skip the live rocprofv3 counter passes")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the ICP legs (configs[0] / configs[2])")
    ap.add_argument("--pmc-inner", action="store_true",
                    help=argparse.SUPPRESS)  # the run rocprofv3 wraps
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-configs4", action="store_true",
                    help="skip the configs[4] leg (4 mm voxels, > 500 k "
                         "blocks, ICP on 2 x 1 M points)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: cold pass, drop-in "
                         "call shapes, the other multi-GPU scheme, roofline "
                         "and live counters, ICP legs, configs[4], CPU "
                         "baseline, bench_detail.json (the --no-* switches "
                         "above thin it out). Without it a run sets up, "
                         "warms up, times the steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the grid they built "
                         "as DIR/<name>.npy (float32 / float64; see "
                         "dump_outputs)")
    return ap.parse_args()


# ---------------------------------------------------------------------------
# multi-GPU launch


def maybe_spawn(a):
    """`python bench.py --gpus N` without torchrun: re-exec under
    torch.distributed.run, one rank per GPU."""
    if a.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    # No port is picked here: the c10d rendezvous binds port 0 itself and the
    # workers reuse the agent's store (picking a port by bind-close and
    # handing the number on raced with EADDRINUSE in round 4).
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MASTER_PORT", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node", str(a.gpus), "--rdzv-backend=c10d",
           "--rdzv-endpoint=127.0.0.1:0", "--local-addr", "127.0.0.1",
           os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


# ---------------------------------------------------------------------------
# CPU baseline (checker code, timed only here)


def cpu_baseline(frames_cpu, K, Ts, budget_s):
    """CPU path timed beside the GPU on a bounded sample of the same stream:
    touch + activate + integrate of its first frames.

    kind "reference": oracle/_ref -- Open3D's own DepthTouchCPU / IntegrateCPU
    bodies compiled from the reference sources (OpenMP stand-in for TBB's
    parallel_for, a sharded concurrent set for tbb::concurrent_unordered_set),
    block activation through the oracle's hash map. Falls back to kind "port"
    (the restated oracle) when the prebuilt _ref is absent. A few thread
    counts are tried on the first frames and the fastest is kept (the
    reference lets TBB pick)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _oracle as orc
    import _ref as ref
    use_ref = ref.available()
    impl = ref if use_ref else orc
    cores = os.cpu_count() or 1

    def run(n_threads, frames, budget):
        impl.set_threads(n_threads)
        cap = 16384
        h = orc.HashMap(cap)
        tsdf = np.zeros((cap, RES, RES, RES), np.float32)
        wgt = np.zeros((cap, RES, RES, RES), np.uint16)
        col = np.zeros((cap, RES, RES, RES, 3), np.uint16)
        n = 0
        phase = [0.0, 0.0, 0.0]  # touch, activate + find, integrate (seconds)
        t0 = time.perf_counter()
        for (d, c), T in frames:
            ta = time.perf_counter()
            keys = impl.depth_touch(d, K, T, RES, VOXEL, VOXEL * TRUNC,
                                    DEPTH_SCALE, DEPTH_MAX)
            tb = time.perf_counter()
            h.activate(keys)
            buf, _ = h.find(keys)
            tc = time.perf_counter()
            impl.integrate(d, c, buf, h.key_buffer(), tsdf, wgt, col, K, K, T,
                           RES, VOXEL, VOXEL * TRUNC, DEPTH_SCALE, DEPTH_MAX)
            td = time.perf_counter()
            phase[0] += tb - ta
            phase[1] += tc - tb
            phase[2] += td - tc
            n += 1
            if time.perf_counter() - t0 > budget:
                break
        return n / (time.perf_counter() - t0), n, [1e3 * x / n for x in phase]

    frames = list(zip(frames_cpu, Ts))
    cands = sorted({c for c in (8, 16, 32, 64, 128, cores) if c <= cores})
    probe = {c: run(c, frames[:6], budget_s * 0.08)[0] for c in cands}
    best = max(probe, key=probe.get)
    fps, n, phase_ms = run(best, frames, budget_s * 0.5)
    return {"value": fps, "unit": "frames/s", "cores": best,
            "kind": "reference" if use_ref else "port", "frames": n,
            # the choice made visible: frames/s of the 6-frame
            # probe at every thread count tried
            "thread_scaling_frames_per_s": {str(c): round(v, 1)
                                            for c, v in sorted(probe.items())},
            "ms_per_frame": {"touch": phase_ms[0],
                             "activate_find": phase_ms[1],
                             "integrate": phase_ms[2]},
            "sample": "first %d frames of the same 640x480 stream (touch + "
                      "activate + integrate, u16 grid with colour); %s; best "
                      "of %s threads on a %d-thread host"
                      % (n, "Open3D DepthTouchCPU/IntegrateCPU bodies via "
                            "oracle/_ref" if use_ref else "restated oracle",
                         cands, cores)}


# ---------------------------------------------------------------------------
# live counters: rocprofv3 passes over a short run of this script

PMC_PASSES = {
    "fetch": ["FETCH_SIZE"],
    "write": ["WRITE_SIZE"],
    "sq": ["SQ_WAVES", "SQ_WAVE_CYCLES", "SQ_INSTS_VALU",
           "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_ANY", "SQ_WAIT_ANY",
           "SQ_WAIT_INST_ANY", "SQ_BUSY_CYCLES", "GRBM_GUI_ACTIVE"],
}


def _pmc_pass(counters, tmp, tag, inner=None, want=None):
    """One rocprofv3 --pmc run (kernel trace only beside it, as the pool
    requires); returns {counter: mean per launch of the wanted kernel}, n.
    Default: the headline stream and the fused colour instantiation of
    FrameStepKernel; `inner` / `want(name)` select another command / kernel.
    "_avg_kernel_ns" = the kernel's mean duration in the same run's trace."""
    out_dir = os.path.join(tmp, tag)
    if inner is None:
        inner = [sys.executable, os.path.abspath(__file__), "--pmc-inner",
                 "--steps", "2", "--warmup", "1", "--batch", "200",
                 "--no-cpu-baseline", "--no-pmc", "--no-secondary"]
    if want is None:
        # the fused colour instantiation: <u16, u16, true, div, form>
        want = lambda name: KERNEL in name and ", true," in name
    cmd = ["rocprofv3"] + (["--pmc"] + counters if counters else []) + \
        ["--kernel-trace", "--output-format", "csv", "-d", out_dir, "-o",
         "pmc", "--"] + inner
    env = dict(os.environ, TMPDIR="/tmp")
    r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True,
                       text=True, timeout=600)
    files = glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"),
                      recursive=True)
    if r.returncode != 0 or (counters and not files):
        raise RuntimeError("rocprofv3 %s: rc %d %s" % (tag, r.returncode,
                                                       r.stderr[-300:]))
    acc, disp = {}, set()
    for f in files:
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                if not want(name):
                    continue
                acc[row["Counter_Name"]] = acc.get(row["Counter_Name"], 0.0) + \
                    float(row["Counter_Value"])
                disp.add(row["Dispatch_Id"])
    n = max(1, len(disp))
    res = {k: v / n for k, v in acc.items()}
    durs, t_lo, t_hi = [], None, None
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"),
                       recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if want(row["Kernel_Name"]):
                    a0, a1 = int(row["Start_Timestamp"]), \
                        int(row["End_Timestamp"])
                    durs.append(a1 - a0)
                    t_lo = a0 if t_lo is None else min(t_lo, a0)
                    t_hi = a1 if t_hi is None else max(t_hi, a1)
    if durs:
        res["_avg_kernel_ns"] = float(np.mean(durs))
        res["_sum_kernel_ns"] = float(np.sum(durs))
        res["_span_ns"] = float(t_hi - t_lo)
        if not counters:
            n = len(durs)
    return res, n


def hbm_counters(inner, want):
    """FETCH_SIZE / WRITE_SIZE passes over `inner` for the kernels `want`
    selects -> {traffic bytes per launch, kernel us (under the profiler),
    frac_hbm} or {error}."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not on PATH"}
    tmp = tempfile.mkdtemp(prefix="o3dmi_pmc4_", dir="/tmp")
    try:
        rd, n1 = _pmc_pass(["FETCH_SIZE"], tmp, "fetch", inner, want)
        wr, _ = _pmc_pass(["WRITE_SIZE"], tmp, "write", inner, want)
        traffic = 2.0 * rd.get("FETCH_SIZE", 0.0) * 1024.0 + \
            wr.get("WRITE_SIZE", 0.0) * 1024.0
        ns = rd.get("_avg_kernel_ns") or wr.get("_avg_kernel_ns")
        out = {"traffic_bytes_per_launch": traffic,
               "traffic_read_bytes": 2.0 * rd.get("FETCH_SIZE", 0.0) * 1024.0,
               "traffic_write_bytes": wr.get("WRITE_SIZE", 0.0) * 1024.0,
               "launches_profiled": n1,
               "kernel_us_under_profiler": ns / 1e3 if ns else None}
        if ns:
            out["frac_hbm"] = traffic / (ns * 1e-9) / 1e9 / HBM_PEAK_GBS
        return out
    except Exception as e:
        return {"error": str(e)[:300]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def pmc_live():
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not on PATH"
    tmp = tempfile.mkdtemp(prefix="o3dmi_pmc_", dir="/tmp")
    try:
        res, n = {}, 0
        for tag, counters in PMC_PASSES.items():
            vals, n = _pmc_pass(counters, tmp, tag)
            res.update(vals)
        res["launches"] = n
        return res, None
    except Exception as e:  # counters are evidence, not the product
        return None, str(e)[:300]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def pmc_committed():
    """Fallback: the newest committed summary of tools/profile_step_pmc.sh."""
    pdir = os.path.join(ROOT, "profiles")
    for fn in sorted(os.listdir(pdir) if os.path.isdir(pdir) else [],
                     reverse=True):
        if "_step_pmc" in fn and fn.endswith(".json"):
            try:
                with open(os.path.join(pdir, fn)) as f:
                    d = json.load(f)
                for k, v in d.items():
                    if KERNEL in k and ", true," in k and "FETCH_SIZE" in v:
                        v = dict(v)
                        v["launches"] = v.pop("dispatches", 0)
                        return v, "profiles/" + fn
            except Exception:
                pass
    return None, None


# ---------------------------------------------------------------------------
# secondary: the ICP half of the metric


# ---------------------------------------------------------------------------
# configs[4] on one GPU: 4 mm voxels, the scene scaled to 8 m, a map of more
# than 524 287 blocks (the reference's `index_t = int` linear voxel index
# overflows there, cpp/open3d/t/geometry/kernel/VoxelBlockGridImpl.h:40; ours
# is int64) whose working set is far beyond the 256 MB Infinity Cache, and
# point-to-plane ICP on two 1 M-point clouds.

C4_VOXEL = 0.004
C4_DEPTH_SCALE = 500.0    # the same images read at twice the metric depth
C4_DEPTH_MAX = 6.0
C4_CAPACITY = 1 << 21     # 2 M blocks = 96 GiB of voxel state
C4_BALLAST = 540000       # active blocks before the stream starts
C4_FRAMES_PER_LAUNCH = 12
C4_FRAME_STEP = 5         # every 5th frame of the 1000-frame stream


def configs4_integrate(n_frames=200, event_stride=1, fpl=None, passes=1,
                       per_launch=False):
    """One cold pass of n_frames frames into the big map (+ `passes` - 1 warm
    passes over the same frames); returns the measurement of the COLD pass
    (and the warm ones under "warm_passes")."""
    import ctypes as C
    import torch
    from open3d_amd import _lib, geometry, synthetic
    from open3d_amd.core import stream
    fpl = fpl or C4_FRAMES_PER_LAUNCH
    dev = torch.device("cuda", torch.cuda.current_device())
    K = synthetic.intrinsics(W, H)
    ds, cs, Ts = [], [], []
    for k in range(0, n_frames * C4_FRAME_STEP, C4_FRAME_STEP):
        d, c, _, T = synthetic.render_frames(k, 1, W, H, device=dev)
        ds.append(d[0].contiguous())
        cs.append(c[0].contiguous())
        T2 = T[0].copy()
        T2[:3, 3] *= 2.0          # the world scaled by 2
        Ts.append(T2)
    g = geometry.VoxelBlockGrid(["tsdf", "weight", "color"],
                                [torch.float32, torch.uint16, torch.uint16],
                                [1, 1, 3], C4_VOXEL, RES, C4_CAPACITY)
    # ballast: 540 k active blocks far from the scene, so that every block of
    # the stream gets a buffer index beyond the reference's int range
    i = torch.arange(C4_BALLAST, dtype=torch.int32, device=dev)
    keys = torch.stack([100000 + i % 1000, 100000 + i // 1000,
                        torch.full_like(i, 100000)], 1).contiguous()
    _lib.check(_lib.lib().o3dmi_hash_activate(
        g.hashmap()._h, _lib.ptr(keys), C4_BALLAST, None, None, None,
        stream()), "activate ballast")
    assert g.hashmap().size() == C4_BALLAST
    # which division forms the launches of the pass use (the on-device proof
    # was started when the grid was created; 2 / 3 = all short forms)
    forms = int(_lib.lib().o3dmi_vbg_division_forms(
        C.c_float(C4_VOXEL), C.c_float(TRUNC), 0))
    batch = g.prepare_frames(ds, cs, K, K, Ts)
    n_launch = (n_frames + fpl - 1) // fpl
    runs = []
    for p in range(passes):
        g.profile_begin(n_launch + 8, event_stride)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.integrate_frames(batch, depth_scale=C4_DEPTH_SCALE,
                           depth_max=C4_DEPTH_MAX,
                           trunc_voxel_multiplier=TRUNC, frames_per_launch=fpl)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        prof = g.profile_end()
        r = {"frames_per_s": n_frames / dt, "wall_ms": dt * 1e3, "prof": prof}
        if per_launch:
            per = g.profile_launches()
            r["per_launch_ms"] = [round(float(x), 4) for x in per["ms"]]
            r["per_launch_distinct"] = per["distinct_blocks"].tolist()
            r["per_launch_map_size"] = per["map_size"].tolist()
        runs.append(r)
    dt = runs[0]["wall_ms"] * 1e-3
    prof = runs[0]["prof"]
    hm = g.hashmap()
    n_blocks = hm.size()
    act = hm.active_buf_indices()
    max_index = int(act.max().item())
    launches = max(1, prof["launches"])
    k_ms = prof["integrate_ms"] / launches
    min_read = (prof["distinct_blocks"] * (BYTES_PER_BLOCK // 2 +
                                           BLOCK_HEADER_BYTES) +
                prof["frames"] * (IMAGE_BYTES + W * H * 8)) / launches
    min_bytes = (prof["distinct_blocks"] * (BYTES_PER_BLOCK +
                                            BLOCK_HEADER_BYTES) +
                 prof["frames"] * (IMAGE_BYTES + 2 * W * H * 8)) / launches
    alg_bytes = (prof["block_frames"] * (BYTES_PER_BLOCK + BLOCK_HEADER_BYTES)
                 + prof["frames"] * IMAGE_BYTES) / launches
    out = {"workload": "%d frames (every %dth of the 640x480 stream, scene "
                       "scaled x2: depth scale %g, depth_max %g m) -> 4 mm "
                       "VoxelBlockGrid(16^3), capacity %d blocks, %d blocks "
                       "active before the stream (ballast), one cold pass"
                       % (n_frames, C4_FRAME_STEP, C4_DEPTH_SCALE,
                          C4_DEPTH_MAX, C4_CAPACITY, C4_BALLAST),
           "frames_per_s": n_frames / dt, "ms_per_frame": dt / n_frames * 1e3,
           "wall_ms_per_launch": dt * 1e3 / n_launch,
           "frames_per_launch": fpl, "division_forms": forms,
           "active_blocks": int(n_blocks),
           "stream_blocks": int(n_blocks - C4_BALLAST),
           "voxel_state_bytes_of_the_stream": int(n_blocks - C4_BALLAST) *
                                              BYTES_PER_BLOCK // 2,
           "max_buffer_index": max_index,
           "max_linear_voxel_index": (max_index + 1) * RES ** 3 - 1,
           "reference_index_limit": 2 ** 31 - 1,
           "avg_blocks_per_frame": prof["block_frames"] /
                                   max(1, prof["frames"]),
           "roofline": {"bound": "valu", "kernel": KERNEL, "unit": "GB/s",
                        "peak": HBM_PEAK_GBS, "avg_kernel_ms": k_ms,
                        "fused_minimum_bytes_per_launch": min_bytes,
                        "minimum_read_bytes_per_launch": min_read,
                        "achieved": min_bytes / (k_ms * 1e-3) / 1e9
                        if k_ms > 0 else None,
                        "frac": min_bytes / (k_ms * 1e-3) / 1e9 /
                                HBM_PEAK_GBS if k_ms > 0 else None,
                        "equivalent_gbps": alg_bytes / (k_ms * 1e-3) / 1e9
                        if k_ms > 0 else None,
                        "distinct_blocks_per_launch":
                            prof["distinct_blocks"] / launches}}
    if per_launch:
        out["per_launch_ms"] = runs[0]["per_launch_ms"]
        out["per_launch_distinct_blocks"] = runs[0]["per_launch_distinct"]
        out["per_launch_map_size"] = runs[0]["per_launch_map_size"]
    if passes > 1:
        out["warm_passes"] = [
            {"frames_per_s": r["frames_per_s"],
             "avg_kernel_ms": r["prof"]["integrate_ms"] /
                              max(1, r["prof"]["launches"])}
            for r in runs[1:]]
    del g
    torch.cuda.empty_cache()
    return out


def kernel_counters(inner, want):
    """The kernels `want` selects in the command `inner`, measured four times
    over -- once under `rocprofv3 --kernel-trace` alone (their durations) and
    once per counter block (FETCH_SIZE; WRITE_SIZE; the SQ set), each pass with
    only the kernel trace beside it -> per launch: traffic bytes (FETCH_SIZE x
    2 + WRITE_SIZE, factors calibrated in profiles/r2a_hbm_calibration.json),
    kernel us without and with counters, VALU issue share, wave-cycle split.
    Every pass runs the SAME command, i.e. the same frames and launches."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not on PATH"}
    tmp = tempfile.mkdtemp(prefix="o3dmi_pmc4_", dir="/tmp")
    try:
        tr, n0 = _pmc_pass([], tmp, "trace", inner, want)
        rd, n1 = _pmc_pass(["FETCH_SIZE"], tmp, "fetch", inner, want)
        wr, _ = _pmc_pass(["WRITE_SIZE"], tmp, "write", inner, want)
        sq, _ = _pmc_pass(PMC_PASSES["sq"], tmp, "sq", inner, want)
        read = 2.0 * rd.get("FETCH_SIZE", 0.0) * 1024.0
        write = wr.get("WRITE_SIZE", 0.0) * 1024.0
        out = {"traffic_bytes_per_launch": read + write,
               "traffic_read_bytes": read, "traffic_write_bytes": write,
               "launches_profiled": n1 or n0,
               "kernel_us_trace_only": (tr.get("_avg_kernel_ns") or 0) / 1e3
               or None,
               "kernel_us_under_counters":
                   (rd.get("_avg_kernel_ns") or 0) / 1e3 or None,
               "kernel_us_sum_trace_only": tr.get("_sum_kernel_ns", 0) / 1e3,
               "span_us_trace_only": tr.get("_span_ns", 0) / 1e3}
        if sq.get("GRBM_GUI_ACTIVE") and sq.get("SQ_ACTIVE_INST_VALU"):
            cyc = sq["GRBM_GUI_ACTIVE"] / N_XCD
            wc = max(1.0, sq.get("SQ_WAVE_CYCLES", 1.0))
            out["frac_valu"], out["frac_valu_bounds"] = valu_fractions(
                sq.get("SQ_INSTS_VALU"), cyc)
            out["valu_insts_per_launch"] = sq.get("SQ_INSTS_VALU")
            out["avg_waves_per_simd"] = sq.get("SQ_WAVE_CYCLES", 0) * 4.0 / \
                (N_SIMD * cyc)
            out["wave_cycle_split"] = {
                "issuing": sq.get("SQ_ACTIVE_INST_ANY", 0) / wc,
                "waiting_memory_or_barrier": sq.get("SQ_WAIT_ANY", 0) / wc,
                "issue_stalled": sq.get("SQ_WAIT_INST_ANY", 0) / wc}
        return out
    except Exception as e:
        return {"error": str(e)[:300]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def attach_counters(roof, k, k_ms):
    """Counter fractions of a leg: bytes of the profiled passes over the kernel
    time of the TIMED pass (`k_ms`, HIP events); the kernel-trace pass of the
    same command is reported beside it."""
    roof.update(k)
    if "error" in k or not k_ms:
        return
    roof["frac_hbm"] = k["traffic_bytes_per_launch"] / (k_ms * 1e-3) / 1e9 / \
        HBM_PEAK_GBS
    if k.get("kernel_us_trace_only"):
        roof["frac_hbm_on_trace_time"] = k["traffic_bytes_per_launch"] / (
            k["kernel_us_trace_only"] * 1e-6) / 1e9 / HBM_PEAK_GBS
    mr = roof.get("minimum_read_bytes_per_launch")
    if mr:
        roof["read_overfetch"] = k["traffic_read_bytes"] / mr


def configs4_leg():
    import importlib.util
    out = {}
    try:
        r = configs4_integrate(per_launch=True, passes=2)
        inner = [sys.executable, os.path.abspath(__file__), "--leg",
                 "configs4-integrate"]
        # the SAME 200-frame cold pass under the profiler (the
        # counters used to come from a 48-frame run)
        attach_counters(r["roofline"], kernel_counters(
            inner, lambda name: KERNEL in name and ", true," in name),
            r["roofline"]["avg_kernel_ms"])
        out["integrate_4mm_over_500k_blocks"] = r
    except Exception as e:
        out["integrate_4mm_over_500k_blocks"] = {"error": str(e)[:300]}
    try:
        spec = importlib.util.spec_from_file_location(
            "bench_slam", os.path.join(ROOT, "tools", "bench_slam.py"))
        bs = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bs)
        r = bs.mode_icp(types.SimpleNamespace(points=1000000, repeat=5,
                                              estimation="p2plane",
                                              no_cpu=True))
        icp = {k: r[k] for k in ("ms_per_icp", "iterations",
                                 "ms_per_iteration", "fitness", "inlier_rmse",
                                 "pose_err_vs_ground_truth_rad_m", "roofline")
               if k in r}
        inner = [sys.executable, os.path.join(ROOT, "tools", "bench_slam.py"),
                 "--mode", "icp", "--points", "1000000", "--repeat", "2",
                 "--no-cpu"]
        k = hbm_counters(inner, lambda name: "SearchAccumulateKernel" in name)
        if "error" not in k and k.get("kernel_us_under_profiler"):
            bpi = (icp.get("roofline") or {}).get("bytes_per_point_iteration")
            if bpi:
                k["algorithmic_bytes_per_launch"] = 1000000 * bpi
                k["frac_algorithmic"] = 1000000 * bpi / (
                    k["kernel_us_under_profiler"] * 1e-6) / 1e9 / HBM_PEAK_GBS
        icp["search_kernel"] = k
        out["icp_2x1M"] = icp
    except Exception as e:
        out["icp_2x1M"] = {"error": str(e)[:300]}
    return out


# ---------------------------------------------------------------------------
# The headline kernel with DRAM in the loop. The looped configs[1] stream keeps
# re-visiting 5 745 blocks = 276 MB of voxel state, about the size of the 256
# MB Infinity Cache, and FETCH_SIZE / WRITE_SIZE count Infinity-Cache hits
# (MI355X_MICROARCH.md): the headline's `frac_hbm` is fabric traffic, not DRAM
# traffic. Here the same 1000 resident images are integrated into DRAM_COPIES
# disjoint copies of the scene in turn (copy c = the scene moved by c x 16 m:
# the extrinsics change, the images do not), so a block's state has been
# pushed out by > 1 GB of other blocks before its next visit.

DRAM_COPIES = 5
DRAM_OFFSET_M = 16.0


def headline_dram_resident(a, event_stride=8, passes=2):
    import torch
    from open3d_amd import geometry, synthetic
    dev = torch.device("cuda", torch.cuda.current_device())
    K = synthetic.intrinsics(W, H)
    ds, cs, Ts = [], [], []
    for k in range(N_UNIQUE):
        d, c, _, T = synthetic.render_frames(k, 1, W, H, device=dev)
        ds.append(d[0].contiguous())
        cs.append(c[0].contiguous())
        Ts.append(T[0])
    g = geometry.VoxelBlockGrid(["tsdf", "weight", "color"],
                                [torch.float32, torch.uint16, torch.uint16],
                                [1, 1, 3], VOXEL, RES, 65536)
    batches = []
    for c in range(DRAM_COPIES):
        # scene moved by o: p' = p + o, the camera sees the same image when
        # its extrinsic becomes T . translate(-o)
        o = np.array([DRAM_OFFSET_M * c, 0.0, 0.0])
        Tc = []
        for T in Ts:
            T2 = np.array(T, dtype=np.float64, copy=True)
            T2[:3, 3] = T2[:3, 3] - T2[:3, :3] @ o
            Tc.append(T2)
        batches.append(g.prepare_frames(ds, cs, K, K, Tc))

    def one_pass():
        for b in batches:
            g.integrate_frames(b, depth_scale=DEPTH_SCALE, depth_max=DEPTH_MAX,
                               trunc_voxel_multiplier=TRUNC,
                               frames_per_launch=a.frames_per_launch)

    one_pass()                      # creates the blocks (cold)
    torch.cuda.synchronize()
    n_launch = passes * DRAM_COPIES * (
        (N_UNIQUE + a.frames_per_launch - 1) // a.frames_per_launch)
    g.profile_begin(n_launch // max(1, event_stride) + 64, event_stride)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(passes):
        one_pass()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    prof = g.profile_end()
    launches = max(1, prof["launches"])
    k_ms = prof["integrate_ms"] / launches
    n_blocks = int(g.hashmap().size())
    min_read = (prof["distinct_blocks"] * (BYTES_PER_BLOCK // 2 +
                                           BLOCK_HEADER_BYTES) +
                prof["frames"] * (IMAGE_BYTES + W * H * 8)) / launches
    min_bytes = (prof["distinct_blocks"] * (BYTES_PER_BLOCK +
                                            BLOCK_HEADER_BYTES) +
                 prof["frames"] * (IMAGE_BYTES + 2 * W * H * 8)) / launches
    out = {"workload": "the configs[1] images integrated into %d disjoint "
                       "copies of the scene in turn (poses moved by c x %g m), "
                       "%d passes after the one that creates the blocks"
                       % (DRAM_COPIES, DRAM_OFFSET_M, passes),
           "frames_per_s": passes * DRAM_COPIES * N_UNIQUE / dt,
           "active_blocks": n_blocks,
           "voxel_state_bytes": n_blocks * BYTES_PER_BLOCK // 2,
           "frames_per_launch": a.frames_per_launch,
           "roofline": {"bound": "valu", "kernel": KERNEL, "unit": "GB/s",
                        "peak": HBM_PEAK_GBS, "avg_kernel_ms": k_ms,
                        "fused_minimum_bytes_per_launch": min_bytes,
                        "minimum_read_bytes_per_launch": min_read,
                        "frac": min_bytes / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
                        if k_ms > 0 else None}}
    del g, batches
    torch.cuda.empty_cache()
    return out


def headline_dram_leg(a):
    try:
        r = headline_dram_resident(a)
        inner = [sys.executable, os.path.abspath(__file__), "--leg",
                 "headline-dram", "--frames-per-launch",
                 str(a.frames_per_launch)]
        attach_counters(r["roofline"], kernel_counters(
            inner, lambda name: KERNEL in name and ", true," in name),
            r["roofline"]["avg_kernel_ms"])
        return r
    except Exception as e:
        return {"error": str(e)[:300]}


# ---------------------------------------------------------------------------
# per-kernel accounting of the tracking loop (configs[2]) from a kernel trace

# (family, substrings of the kernel name; "::X" = a name that STARTS with X
# after its namespace, so that ScatterKernel does not match SortScatterKernel)
KERNEL_FAMILIES = [
    ("search_G8", "SearchAccumulateKernel<float, 8,"),
    ("search_G16", "SearchAccumulateKernel<float, 16,"),
    ("search_G32", "SearchAccumulateKernel<float, 32,"),
    ("final_sum", "FinalSumKernel"),
    ("voxel_down_sample", ("::Vds", "::SortHist", "::SortScatter",
                           "::PostCounts")),
    ("index_build", ("::CountKernel", "::AssignRangesKernel",
                     "::ScatterKernel")),
    ("ray_cast", ("::RayCastKernel", "::EstimateRangeKernel",
                  "::RangeFillKernel")),
    ("unproject", ("::UnprojectKernel", "::TransformNormalsKernel")),
    ("integrate", ("::FrameStepKernel", "::ExportListKeysKernel")),
    ("fill_copy", ("__amd_rocclr_fillBuffer", "__amd_rocclr_copyBuffer")),
]


def cpp_kernel_rooflines(exe, w, h, n_frames, levels):
    """Runs examples/icp_slam once under `rocprofv3 --kernel-trace --stats` and
    returns, per kernel family of the tracking frame: launches and us per
    frame, SURVEY 8(d) algorithmic bytes per launch and the fraction of the HBM
    peak they amount to over the family's mean launch duration; plus launches
    per frame and the share of the loop's wall time a kernel was running.
    `levels`: the per-level sizes of the Python leg's accounting (same stream
    shape): [{source_points, target_points, visited_records_per_query}, ...]
    coarse -> fine."""
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not on PATH"}
    tmp = tempfile.mkdtemp(prefix="o3dmi_ktrace_", dir="/tmp")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format",
               "csv", "-d", tmp, "-o", "icp", "--", exe, str(n_frames), str(w),
               str(h)]
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"),
                           capture_output=True, text=True, timeout=600)
        tr = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"),
                       recursive=True)
        if r.returncode != 0 or not tr:
            return {"error": "rocprofv3 rc %d %s" % (r.returncode,
                                                     r.stderr[-200:])}
        rows = []
        with open(tr[0]) as fh:
            for row in csv.DictReader(fh):
                rows.append((int(row["Start_Timestamp"]),
                             int(row["End_Timestamp"]), row["Kernel_Name"]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rows.sort()
    # the tracking loop = from the first search launch to the last kernel
    first = next((i for i, x in enumerate(rows) if "SearchAccumulate" in x[2]),
                 0)
    loop = rows[first:]
    frames = max(1, n_frames - 1)
    span = loop[-1][1] - loop[0][0]
    busy, cur_end = 0, loop[0][0]
    for a0, a1, _ in loop:            # union of the kernel intervals
        if a1 > cur_end:
            busy += a1 - max(a0, cur_end)
            cur_end = a1
    lv = {k: v for k, v in zip(("search_G32", "search_G16", "search_G8"),
                               levels)} if levels and len(levels) == 3 else {}
    pix = w * h
    cloud = (w // 2) * (h // 2)

    def alg_bytes(fam):
        # SURVEY 8(d), per LAUNCH of the family
        if fam in lv:
            q = lv[fam]["source_points"]
            return q * (12 + 12 + 27 * 8 +
                        lv[fam]["visited_records_per_query"] * 16 + 32)
        if fam == "final_sum":
            return 512 * 32 * 8
        if fam == "voxel_down_sample" and lv:
            # per launch of a chain of ~7 (3 bucketed): 12 B x 2 + 8 B slot +
            # 2 passes x 16 B + 24 B attributes per input point, spread over
            # the launches of a level; input sizes: frame cloud, then levels
            n_in = [cloud] + [l["source_points"] for l in levels[::-1][:2]]
            return sum(n * 88 for n in n_in) / 3.0 / 7.0
        if fam == "index_build" and lv:
            return sum(l["target_points"] for l in levels) * 64 / 3.0 / 3.0
        if fam == "ray_cast":
            return pix * (7.5 * 6 + 48 + 16) / 3.0
        if fam == "unproject":
            return cloud * (4 + 12 + 24) * 2 / 3.0
        return None

    fams = {}
    counted = set()
    for name, pat in KERNEL_FAMILIES:
        pats = (pat,) if isinstance(pat, str) else pat
        sel = [x for x in loop if any(p in x[2] for p in pats)]
        counted.update(id(x) for x in sel)
        if not sel:
            continue
        tot = sum(x[1] - x[0] for x in sel) / 1e3
        avg = tot / len(sel)
        ent = {"launches_per_frame": len(sel) / frames,
               "us_per_frame": tot / frames, "avg_us": avg}
        b = alg_bytes(name)
        if b:
            ent["algorithmic_bytes_per_launch"] = b
            ent["achieved_gbps"] = b / (avg * 1e-6) / 1e9
            ent["frac"] = ent["achieved_gbps"] / HBM_PEAK_GBS
        fams[name] = ent
    rest = [x for x in loop if id(x) not in counted]
    if rest:
        fams["other"] = {"launches_per_frame": len(rest) / frames,
                         "us_per_frame": sum(x[1] - x[0] for x in rest) / 1e3 /
                                         frames,
                         "names": sorted({x[2].split("(")[0][-40:]
                                          for x in rest})[:8]}
    return {"kernels": fams, "launches_per_frame": len(loop) / frames,
            "kernel_us_per_frame": sum(x[1] - x[0] for x in loop) / 1e3 / frames,
            "wall_us_per_frame_under_trace": span / 1e3 / frames,
            "gpu_busy_frac": busy / span if span > 0 else None,
            "basis": "rocprofv3 --kernel-trace of examples/icp_slam (this "
                     "run), from the first search launch to the last kernel; "
                     "frac = SURVEY 8(d) algorithmic bytes per launch / mean "
                     "launch duration / 8 TB/s; level sizes and visited "
                     "records per query from the Python leg's accounting of "
                     "the same stream shape; a search launch also writes the "
                     "moved query back (12 B)"}


def secondary_legs():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "bench_slam", os.path.join(ROOT, "tools", "bench_slam.py"))
    bs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bs)
    out = {}
    a = types.SimpleNamespace(points=100000, repeat=10, estimation="p2plane",
                              no_cpu=False)
    r = bs.mode_icp(a)
    out["configs0_icp_2x100k"] = {
        k: r[k] for k in ("ms_per_icp", "iterations", "ms_per_iteration",
                          "fitness", "inlier_rmse", "roofline",
                          "cpu_oracle_ms_per_icp", "cpu_oracle_threads",
                          "cpu_oracle_ms_per_iteration_phase",
                          "pose_err_vs_oracle_rad_m",
                          "same_iterations_as_oracle") if k in r}
    for tag, vga in (("configs2_loop_1280x720", False),
                     ("configs2_loop_640x480", True)):
        base = dict(frames=60, frame_step=2, block_count=65536, phases=False,
                    vga=vga, cpu_frames=1, host_counts=False)
        bs.mode_slam(types.SimpleNamespace(**dict(base, frames=8,
                                                  cpu_frames=0)))  # warm-up
        r = bs.mode_slam(types.SimpleNamespace(**base))
        out[tag] = {k: r[k] for k in (
            "workload", "frames", "frames_per_s", "ms_per_frame",
            "icp_iterations_per_frame", "source_points", "target_points",
            "final_pose_err_rad_m", "roofline",
            "cpu_oracle_ms_per_multiscale_icp", "cpu_oracle_threads")
            if k in r}
        out[tag]["harness"] = "Python (ctypes) caller of the C ABI"
        # The same loop from a plain C++ caller of the C ABI
        # (examples/icp_slam.cpp: analytic room, closed-form poses, checks its
        # own trajectory): the rate without the interpreter between the calls.
        exe = os.path.join(ROOT, "examples", "icp_slam")
        if os.path.exists(exe):
            w, h = (640, 480) if vga else (1280, 720)
            # The loop is ONE host thread in a tight loop with the device (14
            # launch / mailbox hops per frame), and left to the scheduler a
            # process runs in one of two regimes ~10 % apart (1.30-1.46 k or
            # 1.65-1.72 k frames/s at VGA on the same box; not the NUMA node:
            # `taskset` to eight cores of the GPU's node shows both). Started
            # under a ONE-CPU affinity mask of the GPU's node -- `taskset -c
            # <cpu>`, what a deployment does with a latency-critical control
            # thread -- it is in the fast one every time
            # (profiles/r6i_pinning.txt). The five runs below are started that
            # way; three runs without it are kept beside them.
            cpus = sorted(os.sched_getaffinity(0))
            one = {cpus[min(2, len(cpus) - 1)]}

            def run_once(pin):
                return subprocess.run(
                    [exe, "60", str(w), str(h)], capture_output=True,
                    text=True, timeout=300,
                    preexec_fn=(lambda: os.sched_setaffinity(0, pin))
                    if pin else None)
            # (the host is shared: a CPU may be somebody else's -- one probe
            # run on each of three candidates, the fastest takes the five)
            best = None
            for c in sorted({cpus[min(2, len(cpus) - 1)], cpus[len(cpus) // 4],
                             cpus[len(cpus) // 2]}):
                pr = run_once({c})
                if pr.returncode == 0 and pr.stdout.strip():
                    f = json.loads(
                        pr.stdout.strip().splitlines()[-1])["frames_per_s"]
                    if best is None or f > best[0]:
                        best = (f, c)
            if best is not None:
                one = {best[1]}
            runs, err = [], None
            for _ in range(5):
                pr = run_once(one)
                if pr.returncode != 0 or not pr.stdout.strip():
                    err = {"error": (pr.stderr or "failed")[-300:]}
                    break
                runs.append(json.loads(pr.stdout.strip().splitlines()[-1]))
            unpinned = []
            for _ in range(3 if err is None else 0):
                pr = run_once(None)
                if pr.returncode == 0 and pr.stdout.strip():
                    unpinned.append(json.loads(
                        pr.stdout.strip().splitlines()[-1])["frames_per_s"])
            if err is None:
                runs.sort(key=lambda d: d["frames_per_s"])
                med = dict(runs[len(runs) // 2])  # the median run
                med["frames_per_s_of_5_runs"] = [d["frames_per_s"]
                                                 for d in runs]
                med["pinned_to_cpu"] = sorted(one)[0]
                med["frames_per_s_unpinned"] = sorted(unpinned)
                try:
                    med["per_kernel"] = cpp_kernel_rooflines(
                        exe, w, h, 60,
                        (out[tag].get("roofline") or {}).get("levels"))
                except Exception as e:  # evidence, not the product
                    med["per_kernel"] = {"error": str(e)[:200]}
                err = med
            out[tag + "_cpp_caller"] = err
    return out


# ---------------------------------------------------------------------------


def gpu_partition_modes():
    """Compute / memory partition modes of the box (rocm-smi), or None: the
    DRAM-resident legs read differently on boxes in different modes."""
    try:
        r = subprocess.run(["rocm-smi", "--showcomputepartition",
                            "--showmemorypartition"], capture_output=True,
                           text=True, timeout=20)
        out = {}
        for ln in r.stdout.splitlines():
            low = ln.lower()
            if "gpu[0]" in low and "partition" in low and ":" in ln:
                k = "compute" if "compute" in low else "memory"
                out[k] = ln.rsplit(":", 1)[1].strip()
        return out or None
    except Exception:
        return None


def pin_to_gpu_numa_node(device_index):
    """One process per GPU, on the CPUs of the GPU's own NUMA node: the ICP
    legs are a host in a loop with the device (a mailbox word polled over
    PCIe, a launch per iteration), and from the far socket of the two-socket
    host every hop is longer (examples/icp_slam at VGA: 1320 - 1337 frames/s
    on the GPU's node, 1275 - 1311 on the other, anything between the two
    unpinned). Child processes inherit the mask. Returns the CPU list used, or
    None when the topology cannot be read (nothing is changed then)."""
    try:
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        buf = ctypes.create_string_buffer(64)
        if hip.hipDeviceGetPCIBusId(buf, 64, int(device_index)) != 0:
            return None
        bdf = buf.value.decode().lower()
        with open("/sys/bus/pci/devices/%s/local_cpulist" % bdf) as f:
            spec = f.read().strip()
        cpus = set()
        for part in spec.split(","):
            if not part:
                continue
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
        cpus &= os.sched_getaffinity(0)
        if not cpus:
            return None
        os.sched_setaffinity(0, cpus)
        return spec
    except Exception:
        return None


# ---------------------------------------------------------------------------
# --dump-outputs: what the timed path hands its caller


def dump_sample(n_blocks, n_sample=DUMP_BLOCKS, seed=0):
    """Positions, in key order, of the blocks whose voxels are written: a
    fixed, seeded sample of the active blocks (all of them when few)."""
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(n_blocks, size=min(n_sample, n_blocks),
                              replace=False))


def dump_outputs(g, out_dir):
    """The grid after the last timed step, as a caller of integrate_frames
    receives it: `block_keys` = every active block's key (sorted; buffer
    slots are handed out concurrently, so their order is not stable), and for
    a seeded sample of DUMP_BLOCKS of those blocks (`sample_block_keys`) each
    attribute's voxels ({n, 16, 16, 16, channels}, float32; about 31 MB with
    colour). Returns the names written."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    hm = g.hashmap()
    buf = hm.active_buf_indices().long()
    keys = hm.key_tensor()[buf].cpu().numpy().astype(np.int64)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    keys, buf = keys[order], buf[torch.from_numpy(order).to(buf.device)]
    pick = dump_sample(len(keys))
    idx = buf[torch.from_numpy(pick).to(buf.device)]
    arrays = {"block_keys": keys.astype(np.float64),
              "sample_block_keys": keys[pick].astype(np.float64)}
    for name in g.attr_names:
        t = g.attribute(name)
        if t.dtype == torch.uint16:  # gathered through its int16 view
            t = t.view(torch.int16)[idx].to(torch.int32) & 0xFFFF
        else:
            t = t[idx]
        arrays[name] = t.to(torch.float32).cpu().numpy()
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), arr)
    return sorted(arrays)


def main():
    a = parse()
    if a.leg == "configs4-integrate":  # the run rocprofv3 wraps
        import torch
        torch.cuda.set_device(0)
        print(json.dumps(configs4_integrate(event_stride=0)))
        return
    if a.leg == "headline-dram":
        import torch
        torch.cuda.set_device(0)
        print(json.dumps(headline_dram_resident(a, event_stride=0, passes=1)))
        return
    maybe_spawn(a)
    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        n_dev = max(1, torch.cuda.device_count())
        if a.dist_backend == "nccl":
            assert world <= n_dev, \
                "RCCL needs one GPU per rank (%d ranks, %d GPUs); use " \
                "--dist-backend gloo for a dry run" % (world, n_dev)
        torch.cuda.set_device(local_rank % n_dev)
        dist.init_process_group(a.dist_backend, rank=rank, world_size=world)
        assert dist.get_world_size() == world
    else:
        torch.cuda.set_device(0)
    assert a.gpus == world, \
        "--gpus %d but %d rank(s) were launched" % (a.gpus, world)
    dev = torch.device("cuda", torch.cuda.current_device())
    all_cpus = os.sched_getaffinity(0)
    pinned_cpus = pin_to_gpu_numa_node(torch.cuda.current_device())

    import __graft_entry__ as ge
    if rank == 0 and not os.path.exists(
            os.path.join(ROOT, "open3d_amd", "lib", "libo3d_mi355x.so")):
        ge.build()
    if dist is not None:
        dist.barrier()
    from open3d_amd import geometry, synthetic
    from open3d_amd.sharding import Comm
    # the library's own collectives: RCCL inside the library when the job runs
    # on it, torch.distributed calls (gloo) for the dry run
    # (under --dist-backend nccl a failed library communicator is FATAL unless
    # --allow-transport-fallback: a scaling line must not say "nccl" while the
    # all-gathers stage through the host)
    comm = Comm.for_backend(
        dist, allow_fallback=a.allow_transport_fallback) \
        if dist is not None else None
    comm_check = comm.self_check() if comm is not None else None
    if comm is not None and a.touch == "sliced":
        # integrate_frames on a grid with block ownership then splits the
        # touch over the ranks and all-gathers the candidate keys (RCCL inside
        # the library on the "nccl" backend)
        comm.install()
    elif a.touch == "replicated":
        os.environ["O3DMI_NO_SLICED_TOUCH"] = "1"
    # share of the job this process does: (rank, world) of the real job, or
    # of the emulated one
    e_world = a.emulate_world if (world == 1 and a.emulate_world > 1) else world
    emu_all = e_world != world and str(a.emulate_rank) == "all"
    e_rank = (0 if emu_all else int(a.emulate_rank)) \
        if e_world != world else rank

    K = synthetic.intrinsics(W, H)

    def render(frame_ids):
        ds, cs, ts = [], [], []
        for k in frame_ids:
            d, c, _, T = synthetic.render_frames(k, 1, W, H, device=dev)
            ds.append(d[0].contiguous())
            cs.append(c[0].contiguous())
            ts.append(T[0])
        return ds, cs, ts

    def make_grid(owner=None):
        if a.depth_only:
            g = geometry.VoxelBlockGrid(["tsdf", "weight"],
                                        [torch.float32, torch.uint16], [1, 1],
                                        VOXEL, RES, a.block_count)
        else:
            g = geometry.VoxelBlockGrid(
                ["tsdf", "weight", "color"],
                [torch.float32, torch.uint16, torch.uint16], [1, 1, 3], VOXEL,
                RES, a.block_count)
        g.owner_world = 1
        if owner is not None:
            g.set_block_ownership(*owner)
            g.owner_world = owner[1]
        return g

    def barrier():
        if dist is not None:
            dist.barrier()

    def timed_run(g, depths, colors, Ts, steps, warmup, merge):
        """`warmup` untimed steps, then exactly `steps` steps between barrier
        + synchronize pairs; a step = a.batch frames, the stream looped."""
        n_u = len(depths)
        # The frames are resident and the same on every pass: their pointer
        # and pose arrays are marshalled once (a C++ caller would hand the
        # arrays over as they are), keyed by the slice of the stream.
        prepared = {}
        # One rank's share of an N-rank job on this GPU with the sliced touch:
        # what the all-gather would deliver (every rank's wire segments, per
        # chunk) is computed once per slice of the stream, OUTSIDE the timed
        # region; inside it the rank touches its own band, copies the
        # gathered segments (the stand-in for the collective) and applies them.
        sliced_emu = (world == 1 and a.touch == "sliced" and
                      (g.owner_world > 1 or a.force_sliced))

        def batch_of(lo, m):
            if (lo, m) not in prepared:
                b = g.prepare_frames(
                    depths[lo:lo + m],
                    colors[lo:lo + m] if colors is not None else None, K, K,
                    Ts[lo:lo + m])
                gath = g.gather_slices(
                    b, max(1, g.owner_world), DEPTH_SCALE, DEPTH_MAX, TRUNC,
                    a.frames_per_launch) if sliced_emu else None
                prepared[(lo, m)] = (b, gath)
            return prepared[(lo, m)]

        def batch_of_step(lo):
            # ONE native call per step: the step's a.batch frames (the stream
            # looped) as one pointer / pose array -- the sliced path's first
            # chunks of a call have nothing to overlap with, so a call per
            # 1000-frame pass paid that 8 times per step (DESIGN r4 10.1)
            key = ("step", lo)
            if key not in prepared:
                ids = [(lo + i) % n_u for i in range(a.batch)]
                b = g.prepare_frames(
                    [depths[i] for i in ids],
                    [colors[i] for i in ids] if colors is not None else None,
                    K, K, [Ts[i] for i in ids])
                gath = g.gather_slices(
                    b, max(1, g.owner_world), DEPTH_SCALE, DEPTH_MAX, TRUNC,
                    a.frames_per_launch) if sliced_emu else None
                prepared[key] = (b, gath)
            return prepared[key]

        def run_step(s):
            lo = (s * a.batch) % n_u
            left = a.batch
            while left > 0:
                m = left
                b, gath = batch_of_step(lo)
                if gath is not None:
                    g.integrate_frames_sliced(
                        b, gath, depth_scale=DEPTH_SCALE, depth_max=DEPTH_MAX,
                        trunc_voxel_multiplier=TRUNC,
                        frames_per_launch=a.frames_per_launch)
                else:
                    g.integrate_frames(b, depth_scale=DEPTH_SCALE,
                                       depth_max=DEPTH_MAX,
                                       trunc_voxel_multiplier=TRUNC,
                                       frames_per_launch=a.frames_per_launch)
                left -= m
                lo = (lo + m) % n_u

        for s in range(warmup):
            run_step(s)
        torch.cuda.synchronize()
        barrier()
        # capacity = bracketed launches (every event_stride-th), not frames
        n_launch = steps * a.batch // max(1, a.frames_per_launch)
        g.profile_begin(min(8192, n_launch // max(1, a.event_stride) + 64),
                        a.event_stride)
        torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        for s in range(warmup, warmup + steps):
            run_step(s)
        merge_ms = None
        if merge:
            torch.cuda.synchronize()
            tm = time.perf_counter()
            g.merge_frame_sharded(comm)
            torch.cuda.synchronize()
            merge_ms = (time.perf_counter() - tm) * 1e3
        torch.cuda.synchronize()
        barrier()
        elapsed = time.perf_counter() - t0
        prof = g.profile_end()
        if dist is not None:
            tt = torch.tensor([elapsed], dtype=torch.float64,
                              device="cpu" if a.dist_backend == "gloo" else dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            elapsed = float(tt.item())
        return elapsed, prof, merge_ms

    # Both schemes do the SAME job: `a.batch` frames of the one stream per
    # step. blocks: every rank walks all of them (touch + prepare) and
    # integrates the blocks it owns. frames: rank r walks frames r, r + N, ...
    # (a.batch / N per step) and the merge closes the timed region.
    by_blocks = a.sharding == "blocks" and e_world > 1

    rendered = {}

    def stream_for(blocks):
        ids = list(range(N_UNIQUE)) if blocks or e_world == 1 else \
            list(range(e_rank, N_UNIQUE, e_world))
        key = (ids[0], len(ids))
        if key not in rendered:
            rendered.clear()  # one stream resident at a time
            rendered[key] = render(ids)
        d, c, t = rendered[key]
        return d, (None if a.depth_only else c), t

    def run_scheme(blocks, steps, warmup):
        depths, colors, Ts = stream_for(blocks)
        torch.cuda.synchronize()
        g = make_grid((e_rank, e_world) if blocks and e_world > 1 else None)
        per_rank = a.batch if blocks or e_world == 1 else a.batch // e_world
        saved, a.batch = a.batch, per_rank
        try:
            el, prof, mm = timed_run(g, depths, colors, Ts, steps, warmup,
                                     merge=(dist is not None and not blocks))
        finally:
            a.batch = saved
        return g, el, prof, mm, (depths, colors, Ts)

    g, elapsed, prof, merge_ms, (depths, colors, Ts) = run_scheme(
        by_blocks, a.steps, a.warmup)
    emu_ranks_ms = None
    if emu_all:
        # every rank's share in turn on this GPU; the job lasts as long as its
        # slowest rank: keep that one's run for `value` and the roofline
        emu_ranks_ms = [elapsed / a.steps * 1e3]
        for r in range(1, e_world):
            worst = (g, elapsed, prof, merge_ms)
            del g
            e_rank = r
            g, el_r, prof_r, mm_r, _ = run_scheme(by_blocks, a.steps, a.warmup)
            emu_ranks_ms.append(el_r / a.steps * 1e3)
            if el_r > worst[1]:
                del worst
                elapsed, prof, merge_ms = el_r, prof_r, mm_r
            else:
                del g
                torch.cuda.empty_cache()
                g, elapsed, prof, merge_ms = worst
        e_rank = int(np.argmax(emu_ranks_ms))
    n_blocks = g.hashmap().size()
    total_frames = a.steps * a.batch          # the job, whatever N is
    fps = total_frames / elapsed

    if a.pmc_inner:  # the run rocprofv3 wraps: nothing else to do
        return
    if a.dump_outputs and rank == 0:
        dump_outputs(g, a.dump_outputs)
    if not a.full:
        # a plain run: the headline and nothing else (what follows is --full)
        if rank == 0:
            cfg = {"frames_per_step": a.batch, "block_count": a.block_count,
                   "frames_per_launch": a.frames_per_launch,
                   "timed_region_s": elapsed, "active_blocks": int(n_blocks),
                   "merge_ms": merge_ms,
                   "emulated_ranks_ms_per_step": emu_ranks_ms,
                   "emulated_rank_of_world": [e_rank, e_world]
                   if e_world != world else None}
            line = {"metric": METRIC, "value": fps, "unit": "frames/s",
                    "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                    "ms_per_step": elapsed / a.steps * 1e3,
                    "higher_is_better": True, "scaling": "strong",
                    "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                    "config": _r({k: v for k, v in cfg.items()
                                  if v is not None})}
            print(json.dumps(line), flush=True)
        if dist is not None:
            torch.cuda.synchronize()
            comm.destroy()
            dist.destroy_process_group()
        return

    # configs[1] taken literally: ONE pass over the 1000 frames into an EMPTY
    # grid (every block is created on the way; the looped headline spends
    # 159 / 160 of its time on blocks that already exist)
    cold = None
    if e_world == 1:
        ts = []
        for _ in range(3):
            gc = make_grid()
            pb = gc.prepare_frames(depths, colors, K, K, Ts)
            torch.cuda.synchronize()
            tc = time.perf_counter()
            gc.integrate_frames(pb, depth_scale=DEPTH_SCALE,
                                depth_max=DEPTH_MAX,
                                trunc_voxel_multiplier=TRUNC,
                                frames_per_launch=a.frames_per_launch)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - tc)
            del gc, pb
        ts.sort()
        cold = {"frames_per_s": len(depths) / ts[len(ts) // 2],
                "ms_per_pass": ts[len(ts) // 2] * 1e3,
                "ms_of_3_passes": [t * 1e3 for t in ts],
                "what": "one pass over the %d-frame stream into a freshly "
                        "created grid (capacity %d), grid creation outside "
                        "the timed region" % (len(depths), a.block_count)}

    # What a drop-in user gets: the reference's own call shape
    # -- GetUniqueBlockCoordinates -> Integrate, one frame per pair of calls
    # (VoxelBlockGrid.cpp:212-245,292-326; caller slam/Model.cpp:91-106) -- the
    # fused one-call-per-frame form, and the batch call fed from HOST memory.
    api_legs = None
    if e_world == 1:
        api_legs = {}
        n_api = min(300, len(depths))

        def timed(fn, n):
            fn(0)  # warm-up (first-call allocations)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for i in range(n):
                fn(i)
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t)
        try:
            ga = make_grid()
            ga.integrate_frames(depths, colors, K, K, Ts,
                                depth_scale=DEPTH_SCALE, depth_max=DEPTH_MAX,
                                trunc_voxel_multiplier=TRUNC)  # blocks exist

            def two_step(i):
                bc = ga.compute_unique_block_coordinates(
                    depths[i], K, Ts[i], DEPTH_SCALE, DEPTH_MAX, TRUNC)
                ga.integrate(bc, depths[i],
                             colors[i] if colors is not None else None, K, K,
                             Ts[i], DEPTH_SCALE, DEPTH_MAX, TRUNC)

            def one_call(i):
                ga.integrate_frame(depths[i],
                                   colors[i] if colors is not None else None,
                                   K, K, Ts[i], DEPTH_SCALE, DEPTH_MAX, TRUNC)
            api_legs["api_two_step_frames_per_s"] = timed(two_step, n_api)
            api_legs["integrate_frame_frames_per_s"] = timed(one_call, n_api)
            api_legs["what"] = (
                "%d frames of the same stream into a grid that holds its "
                "blocks; api_two_step = get_unique_block_coordinates (one "
                "host wait for the count, as upstream) + integrate per "
                "frame through the Python mirror; integrate_frame = the "
                "fused one-call form" % n_api)
            del ga
        except Exception as e:
            api_legs["error"] = str(e)[:300]
        # host-fed: the same stream from PINNED HOST memory, copied in slices
        # on a copy stream into two device staging sets while the previous
        # slice integrates (PCIe Gen5 x16: 1.536 MB per frame)
        try:
            n_hf, sl = min(960, len(depths)), 96
            gh = make_grid()
            hd = torch.stack([depths[i] for i in range(n_hf)]).cpu().pin_memory()
            hc = torch.stack([colors[i] for i in range(n_hf)]).cpu().pin_memory() \
                if colors is not None else None
            dd = [torch.empty_like(hd[:sl], device=dev) for _ in range(2)]
            dc = [torch.empty_like(hc[:sl], device=dev) for _ in range(2)] \
                if hc is not None else None
            copy_stream = torch.cuda.Stream()
            main_stream = torch.cuda.current_stream()
            ev_copied = [torch.cuda.Event() for _ in range(2)]
            ev_used = [torch.cuda.Event() for _ in range(2)]

            def host_fed_pass():
                for k, lo in enumerate(range(0, n_hf, sl)):
                    b = k & 1
                    with torch.cuda.stream(copy_stream):
                        if k >= 2:
                            copy_stream.wait_event(ev_used[b])
                        dd[b].copy_(hd[lo:lo + sl], non_blocking=True)
                        if dc is not None:
                            dc[b].copy_(hc[lo:lo + sl], non_blocking=True)
                        ev_copied[b].record(copy_stream)
                    main_stream.wait_event(ev_copied[b])
                    gh.integrate_frames(
                        [dd[b][i] for i in range(sl)],
                        [dc[b][i] for i in range(sl)] if dc is not None
                        else None, K, K, Ts[lo:lo + sl],
                        depth_scale=DEPTH_SCALE, depth_max=DEPTH_MAX,
                        trunc_voxel_multiplier=TRUNC,
                        frames_per_launch=a.frames_per_launch)
                    ev_used[b].record(main_stream)
            host_fed_pass()  # creates the blocks, warms the staging
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(2):
                host_fed_pass()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            api_legs["host_fed_frames_per_s"] = 2 * n_hf / dt
            api_legs["host_fed_pcie_gbps"] = 2 * n_hf * IMAGE_BYTES / dt / 1e9
            api_legs["host_fed_what"] = (
                "%d frames from pinned host memory, %d-frame slices copied "
                "on a copy stream into two device staging sets while the "
                "previous slice integrates (integrate_frames per slice)"
                % (n_hf, sl))
            del gh, hd, hc, dd, dc
        except Exception as e:
            api_legs["host_fed_error"] = str(e)[:300]
        torch.cuda.empty_cache()

    # the other multi-GPU scheme beside the headline (short run)
    other = None
    if e_world > 1:
        del g
        torch.cuda.empty_cache()
        o_blocks = not by_blocks
        st = max(2, a.steps // 5)
        try:
            g2, e2, _, m2, _ = run_scheme(o_blocks, st, 1)
            other = {"sharding": "blocks" if o_blocks else "frames",
                     "scaling": "strong", "frames_per_s": st * a.batch / e2,
                     "steps": st, "ms_per_step": e2 / st * 1e3, "merge_ms": m2,
                     "active_blocks_this_rank": int(g2.hashmap().size())}
            del g2
        except Exception as e:  # the headline above must still be printed
            other = {"sharding": "blocks" if o_blocks else "frames",
                     "error": str(e)[:300]}

    # ---- roofline of the dominant kernel over the bracketed launches --------
    # 8(d) unit = one active block x one frame (98 304 B of voxel state
    # read + written, + 16 B header), + the frame's images once.
    launches = max(1, prof["launches"])
    alg_bytes = (prof["block_frames"] * (BYTES_PER_BLOCK + BLOCK_HEADER_BYTES)
                 + prof["frames"] * IMAGE_BYTES) / launches
    k_ms_events = prof["integrate_ms"] / launches
    # what an event pair costs by itself on this stream (nothing between the
    # two records): part of every bracketed launch's time, NOT subtracted
    evs = [(torch.cuda.Event(enable_timing=True),
            torch.cuda.Event(enable_timing=True)) for _ in range(128)]
    torch.cuda.synchronize()
    for e0, e1 in evs:
        e0.record()
        e1.record()
    torch.cuda.synchronize()
    bracket_ms = float(np.median([e0.elapsed_time(e1) for e0, e1 in evs]))
    # The fractions below are taken on the event time MINUS that bracket (round
    # 6): rocprofv3's kernel-trace duration of the same
    # launches is what it agrees with (77.8 us against 81.9 - 5.8 in round 5),
    # and launches x kernel time then fits inside ms_per_step.
    k_ms = max(k_ms_events - bracket_ms, 0.0)
    achieved = alg_bytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
    # (frames per launch as bracketed: 12 per group launch, up to 192 per chunk
    # launch of the sliced path)
    n_timed_launches = a.steps * a.batch / max(
        1.0, prof["frames"] / launches if prof["frames"] else
        a.frames_per_launch)
    # What has to cross the fabric per launch when the frames of a group are
    # applied to register-resident blocks (the fused minimum): every DISTINCT
    # block of the group once in and once out (98 304 B + header), every
    # frame's images in once, every frame's prepared records (8 B / pixel) out
    # by the front role of the launch that prepared them and in once by the
    # integrate role of the next.
    RECORD_BYTES = W * H * 8
    sliced_launches = e_world > 1 and by_blocks and a.touch == "sliced"
    # which form of the chunk launch the library takes (StreamIntegrateSliced:
    # O3DMI_SLICED_RAW, else raw from 4 ranks): the RAW form reads the images
    # themselves (2 + 3 B per pixel) and has no records at all
    raw_env = os.environ.get("O3DMI_SLICED_RAW")
    sliced_raw = sliced_launches and (
        raw_env[0] == "1" if raw_env else e_world >= 4)
    rec_rw = 0 if sliced_raw else 2 * RECORD_BYTES
    rec_r = 0 if sliced_raw else RECORD_BYTES
    min_bytes = (prof["distinct_blocks"] * (BYTES_PER_BLOCK +
                                            BLOCK_HEADER_BYTES)
                 + prof["frames"] * (IMAGE_BYTES + rec_rw)) / launches
    min_read = (prof["distinct_blocks"] * (BYTES_PER_BLOCK // 2 +
                                           BLOCK_HEADER_BYTES)
                + prof["frames"] * (IMAGE_BYTES + rec_r)) / launches
    # the STRICT minimum: distinct blocks once in and out + the raw images --
    # without the kernel's own prepared records (written by one launch's front
    # role and read back by the next launch's integrate role)
    strict_bytes = (prof["distinct_blocks"] * (BYTES_PER_BLOCK +
                                               BLOCK_HEADER_BYTES)
                    + prof["frames"] * IMAGE_BYTES) / launches
    min_gbps = min_bytes / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
    roof = {"bound": "valu",
            "kernel": "ChunkIntegrateKernel" if sliced_launches else KERNEL,
            "achieved": min_gbps,
            "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": min_gbps / HBM_PEAK_GBS,
            "fused_minimum_bytes_per_launch": min_bytes,
            "strict_minimum_bytes_per_launch": strict_bytes,
            "frac_strict": (strict_bytes / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
                            if k_ms > 0 else None),
            "sliced_form": ("raw" if sliced_raw else "records")
            if sliced_launches else None,
            "minimum_read_bytes_per_launch": min_read,
            "distinct_blocks_per_launch": prof["distinct_blocks"] / launches,
            "equivalent_gbps": achieved,
            "equivalent_frac": achieved / HBM_PEAK_GBS,
            "algorithmic_bytes_per_launch": alg_bytes,
            "avg_kernel_ms": k_ms,
            "avg_kernel_ms_by_events": k_ms_events,
            "empty_event_bracket_ms": bracket_ms,
            "kernel_time_basis": "HIP events around every %d-th launch minus "
                                 "the empty event bracket" % a.event_stride,
            "wall_ms_per_launch": elapsed * 1e3 / n_timed_launches,
            "frames_per_launch": prof["frames"] / launches,
            "traffic": None, "frac_hbm": None, "frac_valu": None,
            "frac_bound": None, "read_overfetch": None}
    roof_note = (
        "`achieved` / `frac`: the fused-minimum bytes of a launch (distinct "
        "blocks of the frame group once in + once out, images in, prepared "
        "records out + in) / HIP-event kernel time / 8 TB/s -- a fraction of "
        "the HBM peak that cannot exceed 1. `equivalent_gbps` is SURVEY "
        "8(d)'s per-frame convention (every voxel of an active block charged "
        "for every frame): how much reference-style traffic a launch stands "
        "for, not what DRAM carried. `frac_hbm` = counter bytes (FETCH_SIZE x "
        "2 + WRITE_SIZE, both factors calibrated on copy kernels with this "
        "kernel's access widths: profiles/r2a_hbm_calibration.json) / the "
        "same kernel time / 8 TB/s; the counters sit on the L2's fabric side "
        "and count Infinity-Cache hits, and the looped stream's 276 MB of "
        "voxel state is about the size of that cache: `frac_hbm` of the "
        "headline is FABRIC traffic; `dram_resident` is the same kernel on a "
        "1.4 GB working set, where the counters are DRAM traffic. "
        "`read_overfetch` = counter reads / minimum reads. The binding roof "
        "is vector-ALU issue (`bound`: bit-exact float32 arithmetic per "
        "voxel): `frac_valu` = `frac_bound` = SQ_INSTS_VALU x 3.5 cycles "
        "(the integrate role's instruction mix priced with the MEASURED "
        "issue cost of each class: 2.4 cycles plain float32 / integer, 4.3 "
        "packed float32 / compare / select / convert, 8.3 reciprocal -- "
        "profiles/r5b_valu_calibration.json, r5_valu_mix.txt) / (1024 SIMDs "
        "x GRBM_GUI_ACTIVE / 8 XCDs), under the profiler; "
        "`frac_valu_bounds` = the same at 2.4 and at 4.3 cycles for every "
        "instruction. `frac_strict` = distinct blocks once in + out and the "
        "raw images, WITHOUT the kernel's own prepared records, over the "
        "same time and peak. `avg_kernel_ms` is the HIP-event bracket of every "
        "16th launch (`avg_kernel_ms_by_events`) minus the event pair's own "
        "cost on this stream (`empty_event_bracket_ms`): the duration "
        "rocprofv3's kernel trace reports for the same launches, and the one "
        "for which launches x kernel time fits inside `ms_per_step`.")
    if e_world == 1 and rank == 0 and not a.no_pmc:
        pmc, why = pmc_live()
        src = "live rocprofv3 passes (this run)"
        if pmc is None:
            pmc, src2 = pmc_committed()
            src = "%s (live collection failed: %s)" % (src2, why) \
                if pmc else None
        if pmc:
            traffic = 2.0 * pmc.get("FETCH_SIZE", 0.0) * 1024.0 + \
                pmc.get("WRITE_SIZE", 0.0) * 1024.0
            roof["traffic"] = traffic
            roof["traffic_read_bytes"] = 2.0 * pmc.get("FETCH_SIZE", 0) * 1024
            roof["traffic_write_bytes"] = pmc.get("WRITE_SIZE", 0) * 1024.0
            roof["traffic_source"] = src
            roof["read_overfetch"] = roof["traffic_read_bytes"] / min_read
            if k_ms > 0:
                roof["frac_hbm"] = traffic / (k_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
            if pmc.get("GRBM_GUI_ACTIVE") and pmc.get("SQ_ACTIVE_INST_VALU"):
                cyc = pmc["GRBM_GUI_ACTIVE"] / N_XCD
                roof["frac_valu"], roof["frac_valu_bounds"] = valu_fractions(
                    pmc.get("SQ_INSTS_VALU"), cyc)
                roof["frac_bound"] = roof["frac_valu"]
                roof["valu_insts_per_launch"] = pmc.get("SQ_INSTS_VALU")
                roof["kernel_cycles_profiled"] = cyc
                roof["avg_waves_per_simd"] = pmc.get("SQ_WAVE_CYCLES", 0) * \
                    4.0 / (N_SIMD * cyc)
                wc = max(1.0, pmc.get("SQ_WAVE_CYCLES", 1.0))
                roof["wave_cycle_split"] = {
                    "issuing": pmc.get("SQ_ACTIVE_INST_ANY", 0) / wc,
                    "waiting_memory_or_barrier": pmc.get("SQ_WAIT_ANY", 0) / wc,
                    "issue_stalled": pmc.get("SQ_WAIT_INST_ANY", 0) / wc}
            roof["counter_launches"] = pmc.get("launches")

    sharding = ("none" if e_world == 1 else
                ("one stream, blocks split by ownership, block touch sliced "
                 "over the ranks: ONE all-gather of candidate {key, frame "
                 "bits} records per chunk of frames (RCCL inside the library); "
                 "union of the grids bit-identical to one GPU's"
                 if a.touch == "sliced" else
                 "one stream, blocks split by ownership, every rank touches "
                 "every ray (no data-path collective); union of the grids "
                 "bit-identical to one GPU's")
                if by_blocks
                else "frames r, r+N, ... of the one stream per rank; closing "
                     "exchange inside the timed region: all-to-all of block "
                     "IDs + voxel rows to the owning rank, folded in there")
    out = {
        "metric": METRIC,
        "loop_frames_per_s": None,  # filled from the configs[2] legs
        "value": fps, "unit": "frames/s", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": elapsed / a.steps * 1e3,
        "higher_is_better": True,
        "scaling": "strong", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "cold_pass_frames_per_s": cold["frames_per_s"] if cold else None,
        "drop_in": ({k: v for k, v in api_legs.items()
                     if not k.endswith("what")} if api_legs else None),
        "config": {"workload": "configs[1]: the 1000-frame synthetic 640x480 "
                               "RGB-D stream (looped, %d frames per GPU in the "
                               "timed region) -> 8 mm VoxelBlockGrid(16^3), "
                               "grid (tsdf f32, weight u16, color u16), known "
                               "poses" % (a.steps * a.batch),
                   "frames_per_step": a.batch, "block_count": a.block_count,
                   "host_cpus": pinned_cpus,
                   "gpu_partition": gpu_partition_modes()
                   if rank == 0 and e_world == 1 else None,
                   "timed_region_s": elapsed,
                   "frames_per_launch": a.frames_per_launch,
                   "active_blocks": int(n_blocks),
                   "map_capacity_after": int(g.hashmap().capacity())
                   if e_world == 1 else None,
                   "avg_blocks_per_frame": prof["block_frames"] /
                                           max(1, prof["frames"]),
                   "sharding": sharding,
                   "parity_vs_single_stream": (
                       None if e_world == 1 else
                       "bit-identical union of the grids" if by_blocks else
                       "block set and weights exact, TSDF <= 1e-4, colour "
                       "within the rounding of the running mean"),
                   "touch": (a.touch if by_blocks else None),
                   "merge_ms": merge_ms,
                   "dist_backend": a.dist_backend if world > 1 else None,
                   # what actually carried the collectives, and how many ranks
                   # the installed communicator spans (ncclCommCount)
                   "transport": comm.transport if comm is not None else None,
                   "rccl_ranks": comm.rccl_ranks() if comm is not None
                   else None,
                   "comm_self_check": comm_check,
                   "emulated_ranks_ms_per_step": emu_ranks_ms,
                   "dry_run": (world > 1 and a.dist_backend == "gloo") or None,
                   "emulated_rank_of_world": [e_rank, e_world]
                   if e_world != world else None,
                   "block_sharded" if not by_blocks else "frame_sharded":
                       other},
        "roofline": roof,
    }
    detail = {"roofline_note": roof_note, "cold_pass": cold,
              "drop_in": api_legs,
              "api": "integrate_frames, one call per step of %d frames, "
                     "argument blocks prepared once (prepare_frames)"
                     % a.batch}
    frames_cpu = None
    if e_world == 1 and not a.no_cpu_baseline:
        frames_cpu = [(depths[i].cpu().numpy(), colors[i].cpu().numpy())
                      for i in range(min(64, len(depths)))]
    secondary = None
    if e_world == 1 and not a.no_secondary:
        del g
        torch.cuda.empty_cache()
        try:
            secondary = secondary_legs()
        except Exception as e:
            secondary = {"error": str(e)[:300]}
        del depths, colors
        torch.cuda.empty_cache()
        if not a.no_pmc:
            secondary["headline_dram_resident"] = headline_dram_leg(a)
        if not a.no_configs4:
            secondary["configs4"] = configs4_leg()
        detail["secondary"] = secondary
    if frames_cpu is not None:
        # the CPU baseline gets the whole host (it picks its own thread
        # count): the GPU-node pinning is lifted for it
        here = os.sched_getaffinity(0)
        try:
            os.sched_setaffinity(0, all_cpus)
            cb = cpu_baseline(frames_cpu, K, Ts, a.cpu_seconds)
        finally:
            os.sched_setaffinity(0, here)
        detail["cpu_baseline"] = dict(cb)
        cb["sample"] = "first %d frames of the same stream; %s; best of " \
                       "several thread counts" % (
                           cb["frames"],
                           "Open3D DepthTouchCPU / IntegrateCPU bodies "
                           "(oracle/_ref) over an OpenMP stand-in for TBB "
                           "with a lock-serialised block-touch set: context, "
                           "not the reference's own scaling"
                           if cb["kind"] == "reference"
                           else "restated oracle")
        out["cpu_baseline"] = cb
    if rank == 0:
        line = compact_line(out, secondary)
        detail["line"] = out
        wrote = []
        for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
            if os.path.isdir(d):
                try:
                    with open(os.path.join(d, "bench_detail.json"), "w") as f:
                        json.dump(detail, f)
                    wrote.append(os.path.relpath(
                        os.path.join(d, "bench_detail.json"), ROOT))
                except OSError:
                    pass
        line["detail"] = wrote[0] if wrote else None
        print(json.dumps(line), flush=True)
    if dist is not None:
        torch.cuda.synchronize()
        comm.destroy()
        dist.destroy_process_group()


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and
            d[k] is not None}


def _r(x, n=4):
    """Numbers of the line rounded to n significant digits (keeps it short)."""
    if isinstance(x, float):
        return float("%.*g" % (n, x))
    if isinstance(x, dict):
        return {k: _r(v, n) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, n) for v in x]
    return x


def compact_line(out, secondary):
    """The ONE line the driver keeps (it stores ~8 KB): the contract fields,
    `roofline`, `cpu_baseline` and one small object per BASELINE config; small
    objects first. Everything else -- notes, per-kernel tables, per-launch
    series, workload descriptions -- goes to bench_detail.json."""
    line = {k: out.get(k) for k in (
        "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
        "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
        "loop_frames_per_s", "loop_frames_per_s_with_first_frame",
        "cold_pass_frames_per_s")}
    if out.get("drop_in"):
        line["drop_in"] = _r(out["drop_in"])
    sec = secondary or {}
    c0 = sec.get("configs0_icp_2x100k") or {}
    if c0:
        line["configs0"] = _r(dict(
            _pick(c0, ("ms_per_icp", "iterations", "ms_per_iteration",
                       "pose_err_vs_oracle_rad_m", "same_iterations_as_oracle",
                       "cpu_oracle_ms_per_icp", "cpu_oracle_threads")),
            frac=(c0.get("roofline") or {}).get("frac")))
    c2 = {}
    for tag, key in (("1280x720", "configs2_loop_1280x720"),
                     ("640x480", "configs2_loop_640x480")):
        py, cpp = sec.get(key) or {}, sec.get(key + "_cpp_caller") or {}
        if not py and not cpp:
            continue
        pk = cpp.get("per_kernel") or {}
        c2[tag] = _r(dict(
            frames_per_s=cpp.get("frames_per_s"),
            # (behind the first tracked frame = the warm-up; the whole run,
            # as rounds 1-5 reported it, is with_first_frame)
            with_first_frame=cpp.get("frames_per_s_with_first_frame"),
            first_frame_ms=cpp.get("first_frame_ms"),
            runs=cpp.get("frames_per_s_of_5_runs"),
            runs_unpinned=cpp.get("frames_per_s_unpinned"),
            pinned_to_cpu=cpp.get("pinned_to_cpu"),
            icp_iterations_per_frame=cpp.get("icp_iterations_per_frame",
                                             py.get("icp_iterations_per_frame")),
            launches_per_frame=pk.get("launches_per_frame"),
            # share of the UNTRACED frame (median run) a kernel was running:
            # the trace's kernel time over that run's frame time (the traced
            # run's own wall clock carries the tracer: gpu_busy_frac_traced)
            gpu_busy_frac=(pk.get("kernel_us_per_frame") *
                           cpp.get("frames_per_s") * 1e-6
                           if pk.get("kernel_us_per_frame") and
                           cpp.get("frames_per_s") else None),
            gpu_busy_frac_traced=pk.get("gpu_busy_frac"),
            kernel_us_per_frame=pk.get("kernel_us_per_frame"),
            python_frames_per_s=py.get("frames_per_s"),
            cpu_oracle_ms_per_multiscale_icp=py.get(
                "cpu_oracle_ms_per_multiscale_icp"),
            error=cpp.get("error")))
        c2[tag] = {k: v for k, v in c2[tag].items() if v is not None}
    if c2:
        loop = {tag: c2[tag].get("frames_per_s") for tag in c2
                if c2[tag].get("frames_per_s") is not None}
        if loop:
            # the loop BASELINE's metric names (ICP + integrate + ray cast),
            # at top level next to `value`: behind the first tracked frame
            # (the warm-up), and over the whole 59-frame run as rounds 1-5
            # reported it
            line["loop_frames_per_s"] = loop
            whole = {tag: c2[tag].get("with_first_frame") for tag in c2
                     if c2[tag].get("with_first_frame") is not None}
            if whole:
                line["loop_frames_per_s_with_first_frame"] = whole
        c2["caller"] = ("examples/icp_slam (C++, median of 5 runs of 60 "
                        "frames, the first tracked frame untimed as warm-up, "
                        "each run started under a one-CPU affinity mask; "
                        "runs_unpinned: left to the scheduler)")
        line["configs2"] = c2
    c4 = (sec.get("configs4") or {})
    c4i = c4.get("integrate_4mm_over_500k_blocks") or {}
    if c4i:
        ro = c4i.get("roofline") or {}
        line["configs4"] = _r(dict(
            _pick(c4i, ("frames_per_s", "wall_ms_per_launch",
                        "frames_per_launch", "active_blocks",
                        "max_linear_voxel_index", "division_forms", "error")),
            warm_pass_frames_per_s=((c4i.get("warm_passes") or [{}])[0]).get(
                "frames_per_s"),
            warm_pass_kernel_ms=((c4i.get("warm_passes") or [{}])[0]).get(
                "avg_kernel_ms"),
            **_pick(ro, ("avg_kernel_ms", "kernel_us_trace_only", "frac",
                         "frac_hbm", "frac_hbm_on_trace_time", "frac_valu",
                         "read_overfetch", "traffic_bytes_per_launch",
                         "fused_minimum_bytes_per_launch"))))
        icp = c4.get("icp_2x1M") or {}
        if icp:
            sk = icp.get("search_kernel") or {}
            line["configs4"]["icp_2x1M"] = _r(dict(
                _pick(icp, ("ms_per_icp", "iterations", "ms_per_iteration",
                            "error")),
                search_kernel_us=sk.get("kernel_us_under_profiler"),
                search_frac_hbm=sk.get("frac_hbm"),
                search_frac_algorithmic=sk.get("frac_algorithmic")))
    dr = sec.get("headline_dram_resident") or {}
    if dr:
        ro = dr.get("roofline") or {}
        line["dram_resident"] = _r(dict(
            _pick(dr, ("frames_per_s", "active_blocks", "voxel_state_bytes",
                       "error")),
            **_pick(ro, ("avg_kernel_ms", "kernel_us_trace_only", "frac",
                         "frac_hbm", "frac_valu", "read_overfetch",
                         "traffic_bytes_per_launch",
                         "fused_minimum_bytes_per_launch"))))
    cfg = dict(out["config"])
    cfg["workload"] = cfg["workload"][:200]
    line["config"] = _r({k: v for k, v in cfg.items() if v is not None})
    line["roofline"] = _r({k: v for k, v in out["roofline"].items()
                           if k not in ("traffic_source",)})
    if "cpu_baseline" in out:
        line["cpu_baseline"] = _r(out["cpu_baseline"])
    if secondary and "error" in secondary:
        line["secondary_error"] = secondary["error"]
    return line


if __name__ == "__main__":
    main()
