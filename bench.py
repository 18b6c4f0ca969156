#!/usr/bin/env python3
"""bench.py -- ms/LM-iter and M-observations/s through Jacobian + Schur build + solve.

A *step* is one Levenberg-Marquardt outer iteration (one linearisation + all its damping
tries + their cost evaluations; the unit `itno` counts in reference PSBA/levmar.cpp:100), run by
the library's own LM loop over the C ABI.  LM converges on these problems in ~15 iterations and
then stalls (tries per iteration become rounding noise), so the K timed steps are run
as segments of at most --segment (10) iterations, each segment restarting from the initial
parameters: every timed step is a productive iteration, and exactly K of them are timed.
Workload (config.workload):
  venice-shaped   the 52 real cameras of data/Venice-52-64053-cams.txt x 64053 synthetic points,
                  mean track 5.42 -- the configuration the north star quotes its roofline target
                  on; *synthetic-shaped*, because the real Venice-52-64053 point file is missing
                  from the reference checkout (default)
  trafalgar50-shaped  the 50 real cameras of data/Trafalgar-50-20431-cams.txt x 20431 synthetic
                  points (BASELINE configs[2]; its point file is missing too)
  54cams          the reference's data/54cams.txt + 54pts.txt, fixed K (BASELINE configs[1])
  trafalgar21     the reference's data/Trafalgar-21-11315-*.txt
  cfg5            BASELINE configs[4]: 2000 cameras on a circle, 10 views per point, dense
                  12000 x 12000 S on the MFMA panel chain; --cfg5-points scales the point count
                  (default 200000 = 2 M observations; 2000000 is the full configuration)
Multi-GPU: 3-D points are sharded over ranks and [tril(S) | ea] is summed with one RCCL all-reduce per
damping try.  --scaling strong (default): ONE problem of the workload's size is split over the ranks
with psba_partition_points -- the north star's 1/2/4/8-GPU figures and BASELINE configs[3]
("Venice-52-64053, points sharded across 4 MI355X") are this:
  python -m torch.distributed.run --nnodes=1 --nproc-per-node 4 --master-addr 127.0.0.1 \
      bench.py --gpus 4            (or simply: python bench.py --gpus 4, see below)
--scaling weak: every rank owns its own shard of the workload's size over the same cameras.  With N > 1
the strong line also carries the weak figure and a sharded cfg5 figure (2000 cameras, 200 k points split
over the ranks, the dense factorization's wide update sharded by block column) as extra keys, with the
bytes each collective moves per damping try.
Launch: under torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in the environment) every
process is one rank.  Started plainly as `python bench.py --gpus N` with N > 1 and no WORLD_SIZE, this
process only SPAWNS the N ranks -- as child processes, before it has imported the library or touched a
GPU (never a re-exec of a process that has initialised the GPU) --, relays rank 0's JSON line and exits
non-zero if any rank failed.
Plain run vs --full: a plain run sets up, warms up, times the K steps (no HIP events on the stream) and
prints the headline line.  --full also times the graded kernel pair with HIP events inside the timed steps
(roofline), times --spread-segments further segments one by one, runs a per-kernel HIP-event pass, the CPU
baselines (--no-cpu-baseline skips them), the clustered-tracks and full-size cfg5 extras of the default
workload and, with N > 1, the multi-GPU extras (--no-extras skips them).
--dump-outputs DIR: right after the K timed steps, what a caller of the LM loop holds -- the refined camera
and point parameters and the LM result's initial and final cost -- as float64 DIR/<name>.npy (see
dump_outputs).  The inputs are generated from fixed seeds or read from tests/golden/data, so two builds run
with the same arguments can be compared output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# psba_amd (which loads the HIP library) is imported by load_library(), called from main() AFTER the decision
# to spawn ranks: the spawning parent must not initialise a GPU runtime.
psba_amd = capi = synth = None


def load_library():
    global psba_amd, capi, synth
    import psba_amd as _p  # loads the HIP library before torch brings its own runtime
    from psba_amd import capi as _c, synth as _s
    psba_amd, capi, synth = _p, _c, _s


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start N children of this very command line, one per
    GPU, with the rendezvous variables torch.distributed.run would set; rank 0's stdout is captured and
    its JSON line printed once; every other output goes to stderr.  Returns the exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=sys.stderr))
    out0, _ = procs[0].communicate()
    codes = [procs[0].returncode]
    deadline = time.time() + 120
    for p in procs[1:]:
        try:
            codes.append(p.wait(timeout=max(1.0, deadline - time.time())))
        except subprocess.TimeoutExpired:  # rank 0 is gone and this one hangs in a collective
            p.kill()
            codes.append(p.wait())
    lines = [ln for ln in out0.decode(errors="replace").splitlines() if ln.strip()]
    json_lines = [ln for ln in lines if ln.lstrip().startswith("{")]
    for ln in lines:
        if ln not in json_lines[-1:]:
            print(ln, file=sys.stderr)
    bad = [(r, c) for r, c in enumerate(codes) if c != 0]
    if bad or not json_lines:
        print(f"[bench] ranks failed (rank, exit code): {bad}; JSON lines from rank 0: {len(json_lines)}", file=sys.stderr)
        return next((c for _, c in bad if c), 1) or 1
    print(json_lines[-1], flush=True)
    return 0


def stub_rank(args, rank, world):
    """PSBA_BENCH_STUB=1 (tests/test_host.py): the launch plumbing without the GPU work -- rendezvous over
    gloo, barrier, max over ranks, ONE JSON line from rank 0, labelled as a stub (value null)."""
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    seen = [None] * world
    dist.all_gather_object(seen, (rank, int(os.environ.get("LOCAL_RANK", "-1")), os.getpid()))
    dist.barrier()
    t = torch.tensor([0.001 * (rank + 1)], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if os.environ.get("PSBA_BENCH_STUB_FAIL_RANK") == str(rank):
        raise SystemExit(7)
    if rank == 0:
        print("a stray line on rank 0's stdout (RCCL banners look like this)")
        print(json.dumps({"stub": True, "metric": "stub", "value": None, "n_gpus": world, "steps": args.steps,
                          "warmup": args.warmup, "scaling": args.scaling, "ranks_seen": seen,
                          "max_over_ranks": float(t[0])}), flush=True)
    else:
        print(f"rank {rank} says hello on its stdout")  # must not reach the parent's stdout
    dist.destroy_process_group()

FP64_VECTOR_PEAK_TFLOPS = 78.6  # vendor figure quoted in SURVEY.md 8(d): fp64 vector (= matrix) peak; = 256 CU x 4 SIMD x 16 lanes x 2 x 2.4 GHz
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s peak


def pmc_traffic(workload, pair_us):
    """HBM bytes per launch of the graded kernel pair (k_schur_lds + k_schur_reduce) from the newest
    committed rocprofv3 PMC passes (profiles/r*_profile.json, written by scripts/summarize_prof.py):
    2 x FETCH_SIZE + WRITE_SIZE, KiB -> bytes.  The factor 2 is the gfx950 correction of
    /opt/skills/guides/MI355X_MICROARCH.md, section HBM ("FETCH_SIZE reports exactly 1/2 of the
    bytes of a wide coalesced streaming read"); the raw counters are returned beside it.  A profile
    whose recorded time for the pair differs from this run's by more than 20 % belongs to other
    code (boxes of the pool differ by up to 8 % on this pair): the traffic is then not quoted (bench.py itself cannot collect PMC counters)."""
    import glob
    best = None

    def graded(name):  # (the runs layout of a clustered-tracks extra in the same profile is another kernel)
        return ("k_schur_lds<" in name or "k_schur_reduce" in name) and "k_schur_lds_runs" not in name

    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_profile.json"))):
        try:
            d = json.load(open(f))
            if d["bench"]["config"]["workload"] != workload:
                continue
            fetch = write = 0.0
            seen = 0
            for name, c in d["pmc_avg_per_launch_KiB"].items():
                if graded(name) and "FETCH_SIZE" in c and "WRITE_SIZE" in c:
                    fetch += c["FETCH_SIZE"]
                    write += c["WRITE_SIZE"]
                    seen += 1
            prof_us = sum(float(r["AverageNs"]) for r in d["kernel_stats"] if graded(r["Name"])) / 1e3
            if seen == 2:
                best = {"bytes": (2 * fetch + write) * 1024.0, "file": os.path.basename(f), "fetch_kib_raw": fetch,
                        "write_kib_raw": write, "profile_pair_us": prof_us, "git_head": d.get("git_head")}
        except Exception:
            continue
    if best and not (0.8 * best["profile_pair_us"] <= pair_us <= 1.2 * best["profile_pair_us"]):
        best["stale"] = True
    return best


def load_workload(name, rank, nranks, strong, cfg5_points):
    """Returns (this rank's problem, data kind).  weak: shard `rank` of the generator (its own
    points over the same cameras); strong: the one problem split with psba_partition_points."""
    data = os.path.join(ROOT, "tests", "golden", "data")
    gens = {"venice-shaped": lambda sh: synth.venice_shaped(shard=sh),
            "trafalgar50-shaped": lambda sh: synth.trafalgar50_shaped(shard=sh),
            "cfg5": lambda sh: synth.cfg5(n_pts=cfg5_points, shard=sh)}
    if name in gens:
        if strong and nranks > 1:
            return capi.shard_problem(gens[name](0), nranks, rank), "synthetic"
        return gens[name](rank), "synthetic"
    if name == "54cams":
        kk = np.array([851.57945, 330.24755, 262.19500, 1.00169, 0.0])
        full = psba_amd.read_problem(os.path.join(data, "54cams.txt"), os.path.join(data, "54pts.txt"), kk)
    elif name == "trafalgar21":
        full = psba_amd.read_problem(os.path.join(data, "Trafalgar-21-11315-cams.txt"),
                                     os.path.join(data, "Trafalgar-21-11315-pts.txt"))
    else:
        raise SystemExit(f"unknown workload {name}")
    # a file is one problem: always split (strong scaling)
    return (capi.shard_problem(full, nranks, rank) if nranks > 1 else full), "reference data/*.txt"


def clustered_extra(device, cluster=16):
    """the same 52 cameras and point count with CLUSTERED tracks (runs of `cluster` consecutive
    points sharing one camera set: what real reconstructions look like in file order; the headline's uniform draw is
    the worst case for block locality in S).  The graded pair (one HIP-event span over the assembly + reduce kernels)
    and a short LM run; an extra key, never the headline."""
    prob = synth.venice_shaped(cluster=cluster)
    h = psba_amd.Psba(device)
    h.upload_problem(prob)
    plan_runs = capi.schur_plan(prob["nC"], prob["nP"], prob["iidx"], prob["jidx"])["run_tasks"]
    h.linearize(1.0, 1.0)
    mu = 1e-3 * h.max_diag()
    h.profile_enable(1 << capi.K_SCHUR)
    for _ in range(5):
        h.schur_assemble(mu)
    h.profile_reset()
    for _ in range(30):
        h.schur_assemble(mu)
    ms, n = h.profile_get(capi.K_SCHUR)
    pair_us = 1e3 * ms / max(n, 1)
    b = h.algorithmic_bytes(capi.K_SCHUR)
    h.profile_enable(0)

    def seg():
        h.reset_params()
        t = time.perf_counter()
        r, _ = h.levmar(max_iter=10, tr_handoff=False, log_cap=0)
        return r, time.perf_counter() - t
    for _ in range(5):
        seg()
    done, dt = 0, 0.0
    for _ in range(3):
        r, d_ = seg()
        done += r.iters
        dt += d_
    h.close()
    return {"tracks": f"runs of {cluster} consecutive points share one camera set", "n_obs": int(prob["nO"]),
            "schur_layout": "runs (a thread sums a run of one block's products in registers)" if plan_runs else "rows of 16 bank pairs",
            "pair_us": pair_us, "roofline_frac": b / (pair_us * 1e-6) / 1e9 / HBM_PEAK_GBS,
            "ms_per_lm_iter": 1e3 * dt / max(done, 1), "M_obs_per_s": prob["nO"] * done / dt / 1e6}


def cfg5_extra(device):
    """BASELINE configs[4] at FULL size on one GPU (synth.cfg5(): 2000 cameras x 2 M points x 20 M
    observations, dense 12 000 x 12 000 S), as an extra key of the default bench line: ms per LM
    iteration over a few restart segments, per-kernel times, and the MFMA fraction of the dense
    factorization recomputed as nA^3 / 3 / (Cholesky time) / 78.6 TFLOP/s."""
    t_gen = time.perf_counter()
    prob = synth.cfg5()
    t_up = time.perf_counter()
    h = psba_amd.Psba(device)
    h.upload_problem(prob)
    t_run = time.perf_counter()
    iters_per_seg, segs = 3, 3

    def seg():
        h.reset_params()
        r, _ = h.levmar(max_iter=iters_per_seg, tr_handoff=False, log_cap=0)
        return r
    seg()  # untimed
    t0 = time.perf_counter()
    done = tries = 0
    res = None
    for _ in range(segs):
        res = seg()
        done += res.iters
        tries += res.tries
    dt = time.perf_counter() - t0
    h.profile_enable(True)
    h.profile_reset()
    seg()
    kern = {}
    for k, name in enumerate(capi.KERNEL_NAMES):
        ms, n = h.profile_get(k)
        if n:
            kern[name] = {"avg_us": round(1e3 * ms / n, 1), "launches": n}
    h.profile_enable(False)
    nA = 6 * int(prob["nC"])
    chol_us = kern.get("cholesky", {}).get("avg_us")
    out = {"workload": "cfg5 (SURVEY 8d): 2000 cameras x 2,000,000 points x 20,000,000 observations, full size, 1 GPU",
           "steps": done, "damping_tries": tries, "segments": f"{segs} restart segments of {iters_per_seg} LM iterations after one untimed",
           "ms_per_lm_iter": 1e3 * dt / max(done, 1), "M_obs_per_s": prob["nO"] * done / dt / 1e6,
           "init_cost": res.init_err, "final_cost": res.final_err, "schur_path": h.schur_path(),
           "kernels_us": kern,
           "cholesky_mfma": ({"flops": nA ** 3 / 3.0, "avg_us": chol_us, "achieved_tflops": nA ** 3 / 3.0 / (chol_us * 1e-6) / 1e12,
                              "peak_tflops": FP64_VECTOR_PEAK_TFLOPS, "frac": nA ** 3 / 3.0 / (chol_us * 1e-6) / 1e12 / FP64_VECTOR_PEAK_TFLOPS}
                             if chol_us else None),
           "host_seconds": {"generate": round(t_up - t_gen, 1), "upload_and_plan": round(t_run - t_up, 1)}}
    h.close()
    return out


class Ranks:
    """The launcher-side plumbing of one rank: rendezvous, barrier, max / sum over ranks (gloo; the
    data-path collectives are RCCL inside the library, on the library's stream)."""

    def __init__(self):
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.dist = None
        if self.world > 1:
            import torch.distributed as dist
            dist.init_process_group("gloo", rank=self.rank, world_size=self.world)
            self.dist = dist

    def barrier(self):
        if self.dist is not None:
            self.dist.barrier()

    def max(self, x):
        if self.dist is None:
            return x
        import torch
        t = torch.tensor([x], dtype=torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t[0])

    def sum_ints(self, xs):
        if self.dist is None:
            return [int(x) for x in xs]
        import torch
        t = torch.tensor(list(xs), dtype=torch.int64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return [int(x) for x in t]

    def handle(self, prob):
        """One handle on this rank's GPU with the problem uploaded, inside a fresh communicator if N > 1."""
        h = psba_amd.Psba(self.local_rank)  # one process per GPU (RCCL refuses two ranks on one device)
        if self.world > 1 or os.environ.get("PSBA_BENCH_REHEARSE"):
            uid = [psba_amd.Psba.comm_unique_id() if self.rank == 0 else None]
            if self.dist is not None:
                self.dist.broadcast_object_list(uid, src=0)
            # RCCL prints a version banner on stdout at communicator creation; stdout carries exactly
            # one JSON line, so the banner goes to stderr
            sys.stdout.flush()
            saved = os.dup(1)
            os.dup2(2, 1)
            try:
                h.comm_init(self.world, self.rank, uid[0])
            finally:
                os.dup2(saved, 1)
                os.close(saved)
        h.upload_problem(prob)
        return h


def collective_bytes(n_cams, world, chol_sharded):
    """Bytes one rank hands to RCCL per damping try: the all-reduce of [tril(S) | e_a] in
    canonical block order (e_a rides in the diagonal blocks), the all-reduce of the try's scalars (16 partial
    sets of 4 sums + 2 status flags), and -- when the dense factorization's wide update is sharded -- the
    broadcasts of the factor's 64-column blocks (the lower triangle once per factorization)."""
    if world == 1:
        return {"allreduce_S_ea": 0, "allreduce_scalars": 0, "broadcast_factor_columns": 0}
    nA = 6 * n_cams
    n32 = (nA + 31) // 32 * 32
    return {"allreduce_S_ea": n_cams * (n_cams + 1) // 2 * 36 * 8, "allreduce_scalars": 66 * 8,
            "broadcast_factor_columns": (n32 * (n32 + 1) // 2 + n32) * 8 if chol_sharded else 0}


def run_steps(h, n, segment):
    """n LM iterations in segments that restart from the initial parameters; returns
    (iterations done, damping tries, last result)."""
    done = tries = 0
    res = None
    while done < n:
        ts = time.perf_counter()
        h.reset_params()  # the uploaded (initial) parameters again, device side
        res, _ = h.levmar(max_iter=min(segment, n - done), tr_handoff=False, log_cap=0)
        if os.environ.get("PSBA_BENCH_DEBUG"):
            print(f"[bench] segment of {res.iters}: {1e6 * (time.perf_counter() - ts):.1f} us", file=sys.stderr)
        if res.iters == 0:
            raise SystemExit("LM made no iteration: cannot time steps")
        done += res.iters
        tries += res.tries
    return done, tries, res


def timed_pass(rk, h, prob, steps, warmup, segment, settle=True, events=True):
    """Settle, W untimed warm-up iterations, then EXACTLY `steps` LM iterations between barriers, MAX over
    ranks.  Returns a dict (elapsed seconds, steps done, tries, totals over ranks, the graded pair's time:
    NaN without `events`)."""
    # events (--full): HIP events on the graded kernel only during the timed region (every timed launch
    # costs two event records on the stream); the other kernel classes are timed in an extra pass afterwards.
    # Enabled before anything runs, so that the event pool is created AND used before the timing
    # starts (growing the runtime's signal pool has been seen to stall the stream for ~0.8 ms).
    if events:
        h.profile_enable(int(os.environ.get("PSBA_BENCH_PROF_MASK", 1 << capi.K_SCHUR)))
    # device wake-up, before the W warm-up steps: a fresh process (more so on a fresh box) runs
    # its first milliseconds of sustained load at a lower clock and has been seen to stall ~0.8 ms
    # once or twice early on (PSBA_BENCH_DEBUG=1 prints the segment times).  Untimed segments are
    # run until three in a row agree to 2 % (at least 12, at most 60: 25-120 ms), which puts that
    # behind us whatever W and K are.
    if settle and not os.environ.get("PSBA_BENCH_NO_SETTLE"):
        times = []
        while len(times) < 60:
            ts = time.perf_counter()
            run_steps(h, segment, segment)
            times.append(rk.max(time.perf_counter() - ts))  # every rank must take the same number of segments
            if len(times) >= 12 and max(times[-3:]) <= 1.02 * min(times[-3:]):
                break
            if len(times) >= 3 and times[-1] > 0.25:  # long steps (cfg5): three segments are plenty
                break
    if warmup > 0:
        run_steps(h, warmup, segment)
    h.profile_reset()
    rk.barrier()
    t0 = time.perf_counter()
    steps_done, tries_done, res = run_steps(h, steps, segment)  # every levmar call returns with its stream drained
    t1 = time.perf_counter()
    rk.barrier()
    elapsed = rk.max(t1 - t0)
    n_obs_total, n_pts_total = rk.sum_ints([prob["nO"], prob["nP"]])
    pair_us = float("nan")
    if events:
        # PSBA_K_SCHUR alone in the mask = ONE span over k_schur_lds + k_schur_reduce: S does not exist
        # before the reduce ends, so the pair is what the roofline is quoted on
        ms, n = h.profile_get(capi.K_SCHUR)
        pair_us = 1e3 * ms / max(n, 1)
        h.profile_enable(0)
    return {"elapsed": elapsed, "steps_done": steps_done, "tries": tries_done, "res": res, "n_obs": n_obs_total,
            "n_pts": n_pts_total, "pair_us": pair_us}


def spread_pass(rk, h, n, segment):
    """--full: n further segments, each timed by itself (max over ranks), outside the K timed steps; ms per LM
    iteration of each."""
    seg_ms = []
    for _ in range(max(n, 0)):
        rk.barrier()
        ts = time.perf_counter()
        d_, _, _ = run_steps(h, segment, segment)
        seg_ms.append(1e3 * rk.max(time.perf_counter() - ts) / max(d_, 1))
    return seg_ms


DUMP_BYTES = 64 * 10**6


def dump_outputs(h, res, out_dir, rank, world):
    """--dump-outputs: the handle's current parameters right after the last timed step and that step's LM
    result, as a caller of psba_levmar receives them: cameras.npy (n_cams x camera block), points.npy
    (n_pts x 3; points_rank<r>.npy per rank when N > 1) and lm_cost.npy ([initial cost, final cost] of the
    last segment), all float64.  Points beyond the 64 MB budget are written as a fixed sample: the rows
    numpy.random.default_rng(0) draws without replacement, in ascending order."""
    os.makedirs(out_dir, exist_ok=True)
    cams, pts = h.get_params()
    budget = (DUMP_BYTES - cams.nbytes - (64 << 10)) // world  # 64 KiB: the costs and the .npy headers
    if pts.nbytes > budget:
        rows = np.random.default_rng(0).choice(len(pts), budget // pts[0].nbytes, replace=False)
        pts = pts[np.sort(rows)]
    if rank == 0:  # the cameras are the same on every rank
        np.save(os.path.join(out_dir, "cameras.npy"), cams)
        np.save(os.path.join(out_dir, "lm_cost.npy"), np.array([res.init_err, res.final_err]))
    np.save(os.path.join(out_dir, "points.npy" if world == 1 else f"points_rank{rank}.npy"), pts)


def per_kernel_pass(h, steps, segment):
    """Untimed extra pass: HIP-event time of every kernel class, each by itself."""
    kern = {}
    h.profile_enable(True)
    h.profile_reset()
    run_steps(h, min(steps, segment), segment)
    for k, name in enumerate(capi.KERNEL_NAMES):
        ms, n = h.profile_get(k)
        if n:
            kern[name] = {"avg_us": 1e3 * ms / n, "launches": n}
    h.profile_enable(False)
    return kern


def extra_multi_gpu(rk, workload, strong, steps, warmup, segment, cfg5_points):
    """One more measured configuration of an N > 1 run (an extra key of the JSON line)."""
    prob, _ = load_workload(workload, rk.rank, rk.world, strong, cfg5_points)
    h = rk.handle(prob)
    chol_sharded = bool(h.chol_dist_shape()[2]) and not os.environ.get("PSBA_CHOL_REPLICATED")
    r = timed_pass(rk, h, prob, steps, warmup, segment, settle=(workload != "cfg5"))
    kern = per_kernel_pass(h, steps, segment)
    h.close()
    return {"workload": workload + (f" split over {rk.world} ranks" if strong else f" x{rk.world} shards"),
            "scaling": "strong" if strong else "weak", "n_cams": int(prob["nC"]), "n_pts": r["n_pts"], "n_obs": r["n_obs"],
            "steps": r["steps_done"], "damping_tries": r["tries"],
            "ms_per_lm_iter": 1e3 * r["elapsed"] / max(r["steps_done"], 1),
            "M_obs_per_s": r["n_obs"] * r["steps_done"] / r["elapsed"] / 1e6, "final_cost": r["res"].final_err,
            "kernels_us_rank0": {k: round(v["avg_us"], 2) for k, v in kern.items()},
            "dense_factorization": "wide update sharded by 64-column block" if chol_sharded else "replicated",
            "bytes_per_try_per_rank": collective_bytes(int(prob["nC"]), rk.world, chol_sharded)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="venice-shaped")
    ap.add_argument("--segment", type=int, default=10, help="LM iterations per restart segment")
    ap.add_argument("--cpu-iters", type=int, default=30, help="--full: LM iterations of the CPU baseline sample")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="strong",
                    help="N > 1: strong = ONE problem split over the ranks (north star, BASELINE configs[3]); "
                         "weak = one shard of the workload's size per rank")
    ap.add_argument("--no-extras", action="store_true", help="--full, N > 1: skip the weak-scaling and sharded-cfg5 extra keys")
    ap.add_argument("--cfg5-points", type=int, default=200000, help="points of the cfg5 workload (2000000 = full)")
    ap.add_argument("--spread-segments", type=int, default=10,
                    help="--full: extra segments timed one by one after the K steps, for the median / spread fields")
    ap.add_argument("--full", action="store_true",
                    help="also the roofline, spread, per-kernel, CPU-baseline and extra-configuration measurements")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the parameters and costs after the last timed step as DIR/<name>.npy "
                         "(bench_out/ is kept out of git)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # no launcher: this process becomes the launcher.  Nothing above has touched a GPU runtime.
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if os.environ.get("PSBA_BENCH_STUB"):
        return stub_rank(args, int(os.environ.get("RANK", "0")), world)

    load_library()
    rk = Ranks()
    rank = rk.rank

    file_workload = args.workload in ("54cams", "trafalgar21")
    strong = args.scaling == "strong" or file_workload
    prob, data_kind = load_workload(args.workload, rank, world, strong, args.cfg5_points)
    h = rk.handle(prob)
    chol_sharded = world > 1 and bool(h.chol_dist_shape()[2]) and not os.environ.get("PSBA_CHOL_REPLICATED")
    r = timed_pass(rk, h, prob, args.steps, args.warmup, args.segment, events=args.full)
    elapsed, steps_done, tries_done, res = r["elapsed"], r["steps_done"], r["tries"], r["res"]
    n_obs_total, n_pts_total, pair_us = r["n_obs"], r["n_pts"], r["pair_us"]
    if args.dump_outputs:
        dump_outputs(h, res, args.dump_outputs, rank, world)

    out = None
    if rank == 0:
        config = {"workload": args.workload + ("" if world == 1 else
                                               (f" split over {world} ranks" if strong else f" x{world} shards")),
                  "n_cams": int(prob["nC"]), "n_pts": n_pts_total, "n_obs": n_obs_total,
                  "lm": "levmar, TR hand-off disabled", "parallelism": f"points sharded x{world}"}
        if data_kind == "synthetic":
            config["tracks"] = ("uniform-random cameras per point (SURVEY 8d stand-in; worst case for block locality: "
                                "two neighbouring points share a block of S with probability ~1 %)")
        out = {
            "metric": "M-observations/sec through Jacobian+Schur build+solve (ms/LM-iter in ms_per_step)",
            "value": n_obs_total * steps_done / elapsed / 1e6,
            "unit": "M-obs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / max(steps_done, 1),
            "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None,
            "dtype": "f64", "data": data_kind,
            "config": config,
            "steps_completed": steps_done, "damping_tries": tries_done, "lm_flag": res.flag, "segment": args.segment,
            "init_cost": res.init_err, "final_cost": res.final_err,
            "schur_path": {0: "lds-partitions", 1: "owner (products sorted by camera pair)", 2: "global-atomics",
                           3: "ring (experiment)", 4: "block-sparse (owner)"}.get(h.schur_path(), str(h.schur_path())),
        }
        if world > 1 or os.environ.get("PSBA_BENCH_REHEARSE"):
            out["multi_gpu"] = {"hardware_note": "first N > 1 measurements come from the driver's node: the builder has one GPU",
                                "dense_factorization": "wide update sharded by 64-column block" if chol_sharded else "replicated",
                                "bytes_per_try_per_rank": collective_bytes(int(prob["nC"]), world, chol_sharded)}
    if args.full:
        full_measurements(args, rk, h, prob, res, pair_us, out)
    h.close()
    if args.full:
        full_extras(args, rk, strong, out)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if rk.dist is not None:
        rk.dist.destroy_process_group()


def full_measurements(args, rk, h, prob, res, pair_us, out):
    """--full, on the headline's handle after its timed steps: spread segments, per-kernel HIP-event pass,
    roofline of the graded pair (its HIP events ran inside the timed steps), CPU baselines.  Every rank takes
    part in the spread segments; the keys go into rank 0's line (`out`)."""
    seg_ms = spread_pass(rk, h, args.spread_segments, args.segment)
    kern = per_kernel_pass(h, args.steps, args.segment)
    world = rk.world
    if rk.rank == 0:
        sch_bytes = h.algorithmic_bytes(capi.K_SCHUR)
        sch_us = pair_us
        achieved = sch_bytes / (sch_us * 1e-6) / 1e9 if sch_us == sch_us and sch_us > 0 else float("nan")
        seg_sorted = sorted(seg_ms)
        # the K timed steps are one sample; these are further segments of the same length timed one
        # by one right after it (ms per LM iteration)
        out["ms_per_step_segments"] = ({"n": len(seg_ms), "median": seg_sorted[len(seg_sorted) // 2],
                                        "min": seg_sorted[0], "max": seg_sorted[-1]} if seg_ms else None)
        out["kernels_us"] = {k: round(v["avg_us"], 3) for k, v in kern.items()}
        out["roofline"] = {"kernel": "schur assemble (W/Y/S/ea): k_schur_lds + k_schur_reduce, one HIP-event span over both",
                           "bound": "hbm", "achieved": achieved,
                           "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                           "algorithmic_bytes_per_launch": sch_bytes, "avg_launch_us": sch_us,
                           "traffic": None}
        # SURVEY 8(d) also asks for the kernel's FP64 rate: nP*50 (V^-1) + nO*(108 Y + 36 e_a) +
        # P_sym*216 flops per launch, P_sym = sum_i k_i (k_i + 1) / 2 products
        ii = np.asarray(prob["iidx"])
        k = np.bincount(ii, minlength=int(prob["nP"])).astype(np.int64)
        sch_flops = float(int(prob["nP"]) * 50 + int(prob["nO"]) * 144 + int((k * (k + 1) // 2).sum()) * 216)
        out["roofline"]["fp64"] = {"algorithmic_flops_per_launch": sch_flops,
                                   "achieved": sch_flops / (sch_us * 1e-6) / 1e12 if sch_us > 0 else None,
                                   "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
                                   "frac": sch_flops / (sch_us * 1e-6) / 1e12 / FP64_VECTOR_PEAK_TFLOPS if sch_us > 0 else None}
        tr = pmc_traffic(args.workload, pair_us) if world == 1 else None
        if tr:
            out["roofline"]["traffic_profile"] = tr
            if not tr.get("stale"):
                out["roofline"]["traffic"] = tr["bytes"]
                out["roofline"]["traffic_source"] = ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command, "
                                                     "profiles/" + tr["file"] + " (2 x FETCH_SIZE + WRITE_SIZE)")
        if args.workload == "cfg5" and not args.no_cpu_baseline:
            # the oracle factors the dense 12000 x 12000 S with a plain triple loop: minutes per try
            out["cpu_baseline"] = {"value": None, "unit": "M-obs/s", "cores": 1, "kind": "port",
                                   "sample": "not run: one dense 12000 x 12000 Cholesky of the single-thread oracle "
                                             "takes minutes, far beyond the bounded sample"}
        elif world == 1 and not args.no_cpu_baseline:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from oracle_lib import Oracle  # the checker, timed as the CPU baseline ("port")
            tc, cpu_iters, ores = 0.0, 0, None
            while cpu_iters < args.cpu_iters:  # same segments as the GPU run
                o = Oracle(prob)
                t = time.perf_counter()
                ores, _ = o.levmar(max_iter=min(args.segment, args.cpu_iters - cpu_iters), tr_handoff=False,
                                   log_cap=0)
                tc += time.perf_counter() - t
                cpu_iters += ores.iters
            out["cpu_baseline"] = {
                "value": prob["nO"] * cpu_iters / tc / 1e6, "unit": "M-obs/s", "cores": 1, "kind": "port",
                "ms_per_lm_iter": 1e3 * tc / max(cpu_iters, 1),
                "sample": f"{cpu_iters} LM iterations (segments of {args.segment}) of the same {args.workload} "
                          f"problem ({prob['nO']} observations), oracle/psba_oracle.c single thread",
                "final_cost": ores.final_err,
            }
            # the last segment of both runs has the same length => costs must agree
            if ores.iters == res.iters:
                out["cost_rel_diff_vs_cpu"] = abs(res.final_err - ores.final_err) / ores.final_err
            # SURVEY 8(d) also asks for the all-core figure: the OpenMP build of the same source
            from oracle_lib import levmar_all_cores
            t = time.perf_counter()
            levmar_all_cores(prob, max_iter=1)  # thread pool start-up outside the timing
            one = time.perf_counter() - t
            # bounded: if one iteration on all cores is not clearly faster than the serial one the
            # team is not getting the CPUs it thinks it has -- report that instead of waiting it out
            tc, cpu_iters, threads = 0.0, 0, 1
            if one > 3 * out["cpu_baseline"]["ms_per_lm_iter"] * 1e-3:
                args.cpu_iters = 0
                out["cpu_baseline_all_cores"] = {"value": None, "unit": "M-obs/s", "cores": None, "kind": "port",
                                                 "sample": f"skipped: one OpenMP iteration took {one:.2f} s"}
            while cpu_iters < args.cpu_iters:
                t = time.perf_counter()
                pres, threads = levmar_all_cores(prob, max_iter=min(args.segment, args.cpu_iters - cpu_iters))
                tc += time.perf_counter() - t
                cpu_iters += pres.iters
            if cpu_iters:
                out["cpu_baseline_all_cores"] = {
                    "value": prob["nO"] * cpu_iters / tc / 1e6, "unit": "M-obs/s", "cores": threads,
                    "kind": "port", "ms_per_lm_iter": 1e3 * tc / max(cpu_iters, 1),
                    "sample": f"{cpu_iters} LM iterations (segments of {args.segment}) of the same problem, "
                              f"oracle/psba_oracle.c built with OpenMP ({threads} threads)",
                    "final_cost": pres.final_err,
                }


def full_extras(args, rk, strong, out):
    """--full, after the headline's handle is closed: the other measured configurations as extra keys of
    rank 0's line (`out`)."""
    rank, world, local_rank = rk.rank, rk.world, rk.local_rank
    # N > 1, default workload: the other two multi-GPU configurations as extra keys (every rank takes part).
    # (PSBA_BENCH_REHEARSE=1: the same code path on ONE GPU -- a one-rank RCCL communicator, the extras included --
    # which is all of the multi-GPU flow a single-GPU box can rehearse)
    rehearse = bool(os.environ.get("PSBA_BENCH_REHEARSE"))
    if (world > 1 or rehearse) and args.workload == "venice-shaped" and not args.no_extras:
        extras = {}
        for key, (wl, st, steps, warm) in {("weak_scaling" if strong else "strong_scaling"):
                                           ("venice-shaped", not strong, args.steps, args.warmup),
                                           "cfg5_sharded": ("cfg5", True, 4, 1)}.items():
            try:
                extras[key] = extra_multi_gpu(rk, wl, st, steps, warm, args.segment if wl != "cfg5" else 2, args.cfg5_points)
            except BaseException as e:  # a rank that drops out here would hang the others in a collective:
                print(f"[bench] rank {rank}: extra {key} failed: {e!r}", file=sys.stderr)  # say so and stop the extras
                extras[key] = {"error": repr(e)}
                break
        if rank == 0:
            out.update(extras)
    if rank == 0:
        # the full-size cfg5 in the driver's view (an extra key, never the headline value)
        if world == 1 and args.workload == "venice-shaped" and not os.environ.get("PSBA_BENCH_NO_CLUSTERED"):
            try:
                out["clustered_tracks"] = clustered_extra(local_rank)
            except Exception as e:
                out["clustered_tracks"] = {"error": repr(e)}
        if world == 1 and args.workload == "venice-shaped" and not os.environ.get("PSBA_BENCH_NO_CFG5"):
            try:
                out["cfg5_full_size"] = cfg5_extra(local_rank)
            except Exception as e:  # the headline line must not depend on the extra
                out["cfg5_full_size"] = {"error": repr(e)}


if __name__ == "__main__":
    main()
