#!/usr/bin/env python3
"""bench.py -- throughput of the F2-NeRF per-ray hot path on MI355X (BASELINE.json metric).

A "step" is one full training iteration of the hot path over one batch of synthetic random-pose rays that is
already resident in HBM: PersSampler (octree intersection + perspective-warped march) -> no-grad density pre-pass
+ early stop -> occupancy update -> fused hash-grid/field MLP -> fused SH/colour MLP -> compositing -> losses ->
backward (compositing, colour MLP, field MLP, hash scatter) -> fused Adam.  Nothing is skipped or cached.

Workload at N=1: BASELINE config[1] "ngp_fox wanjinyou.yaml, 8192 rays/batch, 1xMI355X fp16 fused MLP" on the
serialised fox scene state (tests/golden/fox_state.npz), fresh-initialised table (training start: fineness 16).
Multi-GPU (launched by torch.distributed.run, one rank per GPU): rays shard across ranks (weak scaling: 8192
rays per rank); one RCCL all-reduce (AVG) of the gradient buffers per step + one all-reduce (MAX) of the octree
occupancy votes so that every replica prunes identically.

`--gpus N` without a torch.distributed environment re-executes itself under `torch.distributed.run` with N ranks on
127.0.0.1 (the driver launches the N ranks itself; both ways end in the same code).

Prints ONE JSON line on rank 0: metric/value/unit, ms_per_step, dtype, higher_is_better.  A plain run sets up, warms up, times
--steps steps and prints that line; `--dump-outputs DIR` writes what the last timed step computed as .npy files before it prints
(dump_outputs).  `--full` adds the extras below (each `--no-...` option still drops its own):
  steady_state -- STEADY_STEPS more steps after a timed region shorter than that
  roofline     -- HBM-roofline fraction of the dominant kernel, its duration measured live with HIP events on
                  the launch stream during the timed region (algorithmic bytes per sample: DESIGN.md section 4)
  cpu_baseline -- the CPU oracle (port of the reference path; the reference has no CPU path) timed on this box's
                  host cores on a bounded sample (rank 0, N=1 only).
  converged    -- (rank 0, N=1 only) SURVEY 8(d) config 2 state (ii): the same scene TRAINED for 20 000 iterations on the
                  reference's fox photographs at dataset.factor 2 (ExpRunner::Train: adaptive ray batch, octree
                  subdivision / pruning at the milestones), its test-view PSNR by the reference's definition, and then the
                  same full train step timed in that state (pruned 1e5-node octree, trained table, rays of 5..400
                  samples, rho > 1) with its own dominant-kernel line; then the PSNR study (psnr_numerics_ab).
  other_configs -- (rank 0, N=1 only) BASELINE configs 3-5 as short runs of this script with --full, in their own processes.
  scatter_counters -- the kernel library's hash-scatter counters over the whole process.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# algorithmic bytes per sample of the three field kernels (DESIGN.md section 4 / SURVEY.md section 8(d)):
# 16 levels x 8 corners x 4 B of table traffic + the per-sample streams each kernel must touch
# The dominant kernel of a step is hash_gather_planes_kernel: the 16-level gather of the density pre-pass, one launch
# per step over every marched sample (profiles/*_kernel_stats.csv).  Algorithmic bytes per sample: 16 levels x 8
# corners x 4 B of table reads + point (12) + transform index (4) + the 64 B of f16 feature planes it writes.
DOMINANT = "hash_gather"
ALGO_BYTES = {"hash_gather": 512 + 12 + 4 + 64}
# HBM-side bytes per launch of that kernel from rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate counter passes,
# profiles/run_profiles.sh; FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950), recorded per round in
# profiles/<tag>_traffic.json; null when that file is absent.
TRAFFIC_FILE = next((p for p in (os.path.join(ROOT, "profiles", "r06_traffic.json"), os.path.join(ROOT, "profiles", "r05_traffic.json"), os.path.join(ROOT, "profiles", "r04_traffic.json"), os.path.join(ROOT, "profiles", "r03_traffic.json"), os.path.join(ROOT, "profiles", "r02_traffic.json"),
                                 os.path.join(ROOT, "profiles", "r01_traffic.json")) if os.path.exists(p)), "")
HBM_PEAK_GBS = 8000.0
# What actually bounds that kernel: 128 independent 4-byte reads per sample from an L2-resident table slice.  The chip
# serves at most ~263 G such lane-requests/s whatever the cache policy or access width (tools/gather_policy_probe.py,
# profiles/r01_gather_policy_probe.txt: each request moves a whole line from L2 into a CU's L1) -- reported next to the
# HBM fraction as roofline.request_ceiling.
GATHER_REQ_PEAK = 263.0e9
STEADY_STEPS = 300  # length of the steady-state region reported next to a shorter timed region
L2_PEAK_TBS = 34.5  # aggregate L2 bandwidth of the eight XCDs (MI355X_MICROARCH.md, L2 section)

# Algorithmic HBM bytes per MARCHED sample of the kernels that can dominate a step:
#   hash_gather  16 levels x 8 corners x 4 B + point 12 + warp index 4 + 64 B of f16 feature planes written
#   ray_march    dt 4 + t 4 + (warp, node) 8 written into the ray's slot + 16 B per leaf-list entry read (~1 entry / 2 samples)
#   field_bwd    ONE C-ABI call = MLP backward + hash_bin + hash_bin_accumulate, per MEANINGFUL sample: 512 B of gradient payload
#                into the table (16 levels x 8 corners x 4 B) + 64 B saved MLP input + 64 B dL/dfeat
ALGO_BYTES_CONVERGED = {"hash_gather": 592, "ray_march": 16 + 8, "field_bwd": 512 + 64 + 64, "oct_intersect": 16}
MEANINGFUL_UNIT = {"field_bwd", "shade_bwd", "field_shade_fwd", "composite_train"}  # calls whose rows are the surviving samples
# timed calls that run on the sampler's side streams, underneath the main queue (Renderer.h): never what bounds a step
SIDE_STREAM_CALLS = {"ray_march", "oct_intersect", "oct_repair", "march_repair", "pack_samples", "pack_repair"}


NODE_DT = np.dtype({"names": ["center", "side_len", "parent", "childs", "is_leaf_node", "trans_idx"],
                    "formats": [("<f4", 3), "<f4", "<i4", ("<i4", 8), "u1", "<i4"], "offsets": [0, 12, 16, 20, 52, 56], "itemsize": 64})


def psnr_runs(args, n_runs):
    """n_runs complete trainings (ExpRunner::Train, args.train_iters iterations, fox photographs) in this process and with this
    process's numerics (f2n_numerics_mode: the product build, or the reference-numerics build when the environment says
    F2N_REFERENCE_NUMERICS=1), run r from seed 2022 + r -- since round 4 two product runs from ONE seed are bit-identical, so the
    spread of PSNR@20k has to come from the seeds (ray batches, noise, background, edge samples; the scene's hash primes stay
    those of the committed state).  The LAST run repeats seed 2022 and is only compared with run 0 (`same_seed_rerun`: parameter
    checksums after 1 / 10 / 100 / 1000 iterations and the final PSNR -- identical for the product, not for the reference
    numerics, whose packed-f16 atomics race).  Per run: test PSNR by the reference's definition (mean and per view), training wall
    time, the checksums, and the set of surviving leaves."""
    from f2_nerf_amd import runtime, fox_data, capi
    st = dict(np.load(os.path.join(ROOT, "tests", "golden", "fox_state.npz")))
    sc, images = fox_data.scene(args.factor)
    ds = runtime.make_dataset(sc, images)
    runs, leaf_sets = [], []
    rerun_seed = not getattr(args, "psnr_no_rerun", False)
    seed0 = int(getattr(args, "psnr_seed0", 2022))
    seeds = [seed0 + r for r in range(n_runs)] + ([seed0] if (n_runs > 0 and rerun_seed) else [])
    partial = getattr(args, "psnr_partial", "")
    for seed in seeds:
        runner, cfg, _ = runtime.make_runner(st, args.preset, ["train.end_iter=%d" % args.train_iters], seed=2022)
        torch.manual_seed(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sums = {}
        for stop in (1, 10, 100, 1000):
            if stop < args.train_iters:
                runner.train(ds, stop, 1)
                stt = runner.states()  # [4] table, [8] field MLP, [9] colour MLP (fp32): integer sums of the bit patterns
                sums[str(stop)] = [int(stt[i].contiguous().view(torch.int32).to(torch.int64).sum().item()) for i in (4, 8, 9)]
        runner.train(ds, args.train_iters, 1)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        views = [float(v) for v in runner.test_images(ds)]
        nodes = runner.tree_nodes().cpu().numpy().view(NODE_DT)
        leaf = (nodes["trans_idx"] >= 0) & (nodes["childs"] < 0).all(1)
        key = np.ascontiguousarray(np.concatenate([nodes["center"][leaf], nodes["side_len"][leaf, None]], 1), np.float32).view(np.uint64)
        with np.errstate(over="ignore"):
            leaf_sets.append(np.unique(key[:, 0] * np.uint64(0x9E3779B97F4A7C15) ^ key[:, 1]))
        runs.append({"seed": seed, "psnr_test_mean": round(views[-1], 3), "psnr_test_per_view": [round(v, 2) for v in views[:-1]],
                     "train_wall_s": round(wall, 2), "octree_nodes": int(len(nodes)), "valid_leaves": int(leaf.sum()),
                     "param_checksums_at_iter": sums})
        del runner
        if partial:  # (a study that is cut short keeps what it has: tools/psnr_study.sh)
            with open(partial, "w") as f:
                json.dump({"numerics_mode": int(capi.lib().f2n_numerics_mode()), "runs": runs}, f)
    if not rerun_seed:
        runs.append(dict(runs[0]))
        leaf_sets.append(leaf_sets[0])
    rerun, rerun_leaves = runs.pop(), leaf_sets.pop()  # the repeated seed: compared with run 0 only
    first_diff = None
    for stop in ("1", "10", "100", "1000"):
        if tuple(runs[0]["param_checksums_at_iter"].get(stop, ())) != tuple(rerun["param_checksums_at_iter"].get(stop, ())):
            first_diff = int(stop)
            break
    inter0 = len(np.intersect1d(leaf_sets[0], rerun_leaves, assume_unique=True))
    same_seed = {"seed": seed0, "psnr_run0": runs[0]["psnr_test_mean"], "psnr_rerun": rerun["psnr_test_mean"],
                 "checksums_part_at_checkpoint": first_diff,
                 "identical": (first_diff is None and runs[0]["psnr_test_mean"] == rerun["psnr_test_mean"]) if rerun_seed else None,
                 "surviving_leaf_sets_jaccard": round(inter0 / max(len(leaf_sets[0]) + len(rerun_leaves) - inter0, 1), 4)}
    jac = []
    for i in range(n_runs):
        for j in range(i + 1, n_runs):
            inter = len(np.intersect1d(leaf_sets[i], leaf_sets[j], assume_unique=True))
            jac.append(inter / max(len(leaf_sets[i]) + len(leaf_sets[j]) - inter, 1))
    m = np.array([r["psnr_test_mean"] for r in runs])
    pv = np.array([r["psnr_test_per_view"] for r in runs])
    out = {"numerics": capi.build_info(), "numerics_mode": int(capi.lib().f2n_numerics_mode()), "runs": n_runs,
           "seeds": [r["seed"] for r in runs],
           "psnr_mean": round(float(m.mean()), 3), "psnr_std": round(float(m.std(ddof=1)) if n_runs > 1 else 0.0, 3),
           "psnr_min": round(float(m.min()), 3), "psnr_max": round(float(m.max()), 3), "psnr_per_run": [float(v) for v in m],
           "per_view_mean": [round(float(v), 2) for v in pv.mean(0)],
           "per_view_std": [round(float(v), 2) for v in (pv.std(0, ddof=1) if n_runs > 1 else np.zeros(pv.shape[1]))],
           "train_wall_s": [r["train_wall_s"] for r in runs], "valid_leaves": [r["valid_leaves"] for r in runs],
           "surviving_leaf_sets_jaccard_across_seeds": {"min": round(min(jac), 4), "mean": round(float(np.mean(jac)), 4)} if jac else None,
           "same_seed_rerun": same_seed,
           "corr_psnr_vs_valid_leaves": round(float(np.corrcoef(m, [r["valid_leaves"] for r in runs])[0, 1]), 3) if n_runs > 2 else None}
    return out


def pool_psnr_estimates(delta, se_unpaired, paired, runs_a, runs_b, path=None):
    """The pooled estimate of (reference numerics - product) PSNR@20k over the committed sessions and this invocation's."""
    path = path or os.path.join(ROOT, "profiles", "psnr_estimates.json")
    est = []
    if os.path.exists(path):
        with open(path) as f:
            est = list(json.load(f).get("estimates", []))
    if delta is not None and se_unpaired and se_unpaired > 0:
        est.append({"session": "this invocation of bench.py", "runs": "%d + %d" % (runs_a, runs_b), "delta_db": round(float(delta), 4),
                    "standard_error_unpaired_db": round(float(se_unpaired), 4),
                    "standard_error_paired_db": (paired or {}).get("standard_error_db"), "paired_delta_db": (paired or {}).get("mean_db")})

    def pool(key_order):
        d, w = [], []
        for e in est:
            se_ = next((e.get(k) for k in key_order if e.get(k)), None)
            if se_:
                d.append(e["delta_db"])
                w.append(1.0 / se_ ** 2)
        if not w:
            return None
        w, d = np.array(w), np.array(d)
        m, se_p = float((w * d).sum() / w.sum()), float(1.0 / np.sqrt(w.sum()))
        return {"delta_db": round(m, 4), "standard_error_db": round(se_p, 4), "interval_95_db": [round(m - 1.96 * se_p, 3), round(m + 1.96 * se_p, 3)],
                "heterogeneity_chi2": round(float((w * (d - m) ** 2).sum()), 2), "dof": len(d) - 1}
    up = pool(("standard_error_unpaired_db", "standard_error_paired_db"))
    pp = pool(("standard_error_paired_db", "standard_error_unpaired_db"))
    verdict = "inconclusive"
    if up:
        lo, hi = up["interval_95_db"]
        verdict = True if (lo >= -0.1 and hi <= 0.1) else (False if (lo > 0.1 or hi < -0.1) else "inconclusive")
    return {"file": "profiles/psnr_estimates.json", "estimates": est, "pooled_unpaired": up, "pooled_paired_for_comparison": pp, "within_0p1_db": verdict}


def psnr_numerics_ab(args):
    """PSNR@20k as a distribution, and as an A/B of the two numerics (round-2 verdict, "make the PSNR claim testable"): two
    worker processes of this script (one per build of the kernel library: include/f2n_abi.h f2n_numerics_mode) train the fox
    scene args.psnr_runs / args.psnr_ref_runs times, ONE AFTER THE OTHER (until round 4 they shared the GPU: a training then
    took three times as long, so nothing was gained, and a co-tenant is the one condition under which two product trainings
    from one seed have been seen to part -- DESIGN.md section 7, "reproducibility")."""
    out = {}
    for tag, n, envv in (("product", args.psnr_runs, "0"), ("reference_numerics", args.psnr_ref_runs, "1")):
        if n <= 0:
            continue
        env = dict(os.environ, F2N_REFERENCE_NUMERICS=envv)
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        cmd = [sys.executable, os.path.abspath(__file__), "--psnr-worker", str(n), "--train-iters", str(args.train_iters),
               "--factor", str(args.factor), "--preset", args.preset]
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
        so = se = ""
        try:
            so, se = p.communicate(timeout=1500)
            out[tag] = json.loads(so.strip().splitlines()[-1])
        except Exception as e:
            p.kill()
            out[tag] = {"error": (str(e) + " | " + (se or "")[-400:])[:600]}
    a, b = out.get("product", {}), out.get("reference_numerics", {})
    if "psnr_mean" in a and "psnr_mean" in b:
        delta = b["psnr_mean"] - a["psnr_mean"]
        # standard error of the difference of the two means (run-to-run spread of each numerics / sqrt of its run count)
        se = float(np.sqrt(a["psnr_std"] ** 2 / max(a["runs"], 1) + b["psnr_std"] ** 2 / max(b["runs"], 1)))
        out["delta_mean_db_reference_minus_product"] = round(delta, 3)
        out["delta_standard_error_db"] = round(se, 3)
        out["ranges_overlap"] = bool(a["psnr_min"] <= b["psnr_max"] and b["psnr_min"] <= a["psnr_max"])
        # the 0.1 dB question can only be answered by a comparison that RESOLVES 0.1 dB: standard error of the difference < 0.1
        out["within_0p1_db"] = (bool(abs(delta) <= 0.1) if se < 0.1 else "inconclusive")
        out["resolution_note"] = ("standard error of the difference %.3f dB %s 0.1 dB" % (se, "<" if se < 0.1 else ">=")) + \
                                 ("" if se < 0.1 else ": this invocation cannot answer the 0.1 dB question; see pooled_evidence")
        out["delta_within_2_standard_errors_of_zero"] = bool(abs(delta) <= 2 * se)
        # the two builds ran the same seeds: the paired differences remove the seed-to-seed spread from the comparison
        k = min(len(a.get("psnr_per_run", [])), len(b.get("psnr_per_run", [])))
        if k >= 2:
            dif = np.array(b["psnr_per_run"][:k]) - np.array(a["psnr_per_run"][:k])
            out["paired_by_seed"] = {"seeds": a.get("seeds", [])[:k], "differences_db": [round(float(v), 3) for v in dif],
                                     "mean_db": round(float(dif.mean()), 3),
                                     "standard_error_db": round(float(dif.std(ddof=1) / np.sqrt(k)), 3)}
        # An invocation with a handful of runs cannot resolve 0.1 dB (a product training is ~15 s, a reference-numerics one ~28 s), so
        # its estimate is FOLDED INTO the pooled one over every session that exists (profiles/psnr_estimates.json; round-5 verdict,
        # next 4b): inverse-variance weights on the unpaired standard errors (a session that only has a paired one enters with it), and
        # within_0p1_db is read off the pooled 95 % interval -- true: inside +-0.1 dB, false: outside, else "inconclusive".
        out["within_0p1_db_this_invocation"] = out.pop("within_0p1_db")
        pooled = pool_psnr_estimates(delta, se, out.get("paired_by_seed"), a["runs"], b["runs"])
        out["pooled_evidence"] = pooled
        out["within_0p1_db"] = pooled["within_0p1_db"]
        out["within_0p1_db_source"] = "95 %% interval of the pooled estimate over %d sessions (this invocation included), unpaired standard errors" % len(pooled["estimates"])
    out["note"] = ("run r of either build trains from seed 2022 + r, same explicit schedule; the two workers run one after the other "
                   "(their train_wall_s include the checkpoints' host round trips). "
                   "reference_numerics = libf2n_hip_refnum.so: hash gradient by per-addend packed-f16 atomics in arrival order "
                   "(Hash3DAnchored.cu:145-153) and an f16 accumulator in the MLP forward products; product = fp32 MFMA accumulation, "
                   "owner-binned hash-gradient sums rounded to f16 once")
    return out


def other_configs(args):
    """BASELINE configs 3-5 as short runs of this script in their own processes (one at a time: they are timed), so that the
    default bench line carries a number for each: the llff and nerf-360 presets on the synthetic rigs, wanjinyou_big at the
    file's log2 20 and at the 2^22 BASELINE.json names.  Counters for the big-table points: profiles/r03_big{20,22}_*."""
    out = {}
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    for tag, extra in (("llff", ["--preset", "llff"]), ("nerf-360", ["--preset", "nerf-360"]),
                       ("wanjinyou_big_log2_20", ["--preset", "wanjinyou_big", "--log2", "20"]),
                       ("wanjinyou_big_log2_22", ["--preset", "wanjinyou_big", "--log2", "22"])):
        cmd = [sys.executable, os.path.abspath(__file__), "--full", "--steps", str(args.other_steps), "--warmup", "10", "--no-cpu-baseline",
               "--no-converged", "--no-steady", "--other-configs", "0"] + extra
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
            ln = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
            rf = ln.get("roofline") or {}
            out[tag] = {"value": ln["value"], "unit": ln["unit"], "ms_per_step": round(ln["ms_per_step"], 4), "steps": ln["steps"],
                        "workload": ln["config"]["workload"], "meaningful_samples_per_step": round(ln["config"]["meaningful_samples_per_step"]),
                        "dominant_kernel_ms": rf.get("avg_kernel_ms"), "hbm_frac_algorithmic": rf.get("frac"),
                        "traffic_bytes_per_launch": rf.get("traffic"), "traffic_rate": (rf.get("traffic_rate") or {}).get("frac")}
        except Exception as e:
            out[tag] = {"error": str(e)[:200]}
    return out


def converged_leg(args, st, dev):
    """SURVEY 8(d) config 2, state (ii).  Trains the scene for args.train_iters iterations on the fox photographs with the
    reference's loop (ExpRunner::Train), reports the test PSNR (reference definition: 8-bit quantised prediction,
    ExpRunner.cpp:360-369), then times full train steps on real training batches in that state."""
    from f2_nerf_amd import runtime, fox_data
    host = runtime.host()
    t_load = time.perf_counter()
    sc, images = fox_data.scene(args.factor)
    ds = runtime.make_dataset(sc, images)
    runner, cfg, _ = runtime.make_runner(st, args.preset, ["train.end_iter=%d" % args.train_iters], seed=2022, device=dev)
    runner.speculative_sampling = {"auto": 2, "on": 1, "off": 0}[args.speculation]
    if args.speculation_depth >= 1:
        runner.speculation_depth = args.speculation_depth
    if args.march_blocks >= 0:
        runner.march_blocks = args.march_blocks
    torch.manual_seed(2022)
    torch.cuda.synchronize()
    t_load = time.perf_counter() - t_load
    t0 = time.perf_counter()
    s = runner.train(ds, args.train_iters, 1)
    torch.cuda.synchronize()
    train_wall = time.perf_counter() - t0
    runner.test_image_psnr(ds, int(sc["test_set"][0]))  # untimed: the first render allocates its (larger) chunk buffers
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    views = [float(v) for v in runner.test_images(ds)]
    torch.cuda.synchronize()
    test_wall = time.perf_counter() - t1
    out = {"state": "after %d iterations of ExpRunner::Train on the ngp_fox photographs at dataset.factor %d (%dx%d), %s.yaml"
                    % (runner.iter_step, args.factor, int(sc["image_hw"][0]), int(sc["image_hw"][1]), args.preset),
           "train_wall_s": round(train_wall, 2), "train_iterations": int(s["iterations"]),
           "train_ray_samples_per_s": s["total_meaningful"] / train_wall, "train_rays_per_s": s["total_rays"] / train_wall,
           "psnr_test_mean": round(views[-1], 3), "psnr_test_runs": 1, "psnr_test_per_view": [round(v, 2) for v in views[:-1]],
           "psnr_test_note": "ONE training run (seed 2022; a rerun of the seed reproduces it bit for bit: psnr_numerics_ab.product.same_seed_rerun); "
                             "its distribution over seeds is psnr_numerics_ab.product",
           "psnr_definition": "reference (ExpRunner.cpp:360-369): prediction clipped and quantised to 8 bit, 20 log10(1/sqrt(mse)), "
                              "test views = every 8th image", "test_views_wall_s": round(test_wall, 2),
           "image_hw": [int(v) for v in sc["image_hw"]], "octree_nodes": runner.n_nodes(), "setup_s": round(t_load, 1)}
    # ---- timed steps in the converged state: the reference's own loop carries on (ExpRunner::Train: a fresh random batch of
    # the adaptive size drawn on the device every iteration, next batch's sampling prefetched, octree compaction when due) ----
    K = args.converged_steps
    runner.end_iter = runner.iter_step + K + 64  # (the schedule's last stretch: the learning rate is at its floor either way)
    runner.train(ds, runner.iter_step + 16, 1)
    runner.flush()
    c0 = runner.counters()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s2 = runner.train(ds, runner.iter_step + K, 1)
    runner.flush()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    c1 = runner.counters()
    K = int(s2["iterations"])
    R = s2["total_rays"] / max(K, 1)
    nm, na = c1["total_meaningful"] - c0["total_meaningful"], c1["total_marched"] - c0["total_marched"]
    out.update({"rays_per_batch": round(R, 1), "steps": K, "ms_per_step": el / K * 1e3, "value": nm / el, "unit": "ray-samples/s",
                "marched_samples_per_s": na / el, "rho_marched_over_meaningful": na / max(nm, 1),
                "meaningful_samples_per_step": nm / K, "marched_samples_per_step": na / K, "rays_per_s": R * K / el,
                "timed_loop": "ExpRunner::Train (native loop, fresh batches, ray generation and octree maintenance included)",
                # batches whose intersection + march ran AHEAD of the previous step's stat update / behind it (ProcOctree
                # iterations), rays walked again because a leaf on their list died in that update, stat updates so far
                "speculative_sampling": {k: int(v) for k, v in runner.speculation_counters().items()}})
    R = max(16, runner.cur_batch_size())
    n_batches = 16
    batches = [ds.rand_rays_data(R, 1) for _ in range(n_batches)]

    def step(i):
        b, nb, nb2 = batches[i % n_batches], batches[(i + 1) % n_batches], batches[(i + 2) % n_batches]
        if runner.speculation_depth >= 2:
            return runner.train_step(b[0], b[1], b[2], b[3], b[4], True, nb[0], nb[1], nb[2], nb2[0], nb2[1])
        return runner.train_step(b[0], b[1], b[2], b[3], b[4], True, nb[0], nb[1], nb[2])
    for i in range(4):
        step(i)
    # per-kernel HIP-event breakdown of 40 more steps (events on the launch streams; not part of the timed region above)
    host.ExpRunner.enable_kernel_timing(["*"])
    KB = 40
    nab = 0
    c_kb0 = runner.counters()
    for i in range(KB):
        nab += step(i)["n_samples"]
    torch.cuda.synchronize()
    t = host.ExpRunner.collect_kernel_timing()
    host.ExpRunner.disable_kernel_timing()
    per = {k: v[1] / KB for k, v in t.items()}
    out["timed_calls_ms_per_step"] = {k: round(v, 4) for k, v in sorted(per.items(), key=lambda kv: -kv[1])}
    # the step is bounded by its MAIN queue: the dominant kernel is looked for there; what ran underneath it on the side streams
    # (the sampler of the batches ahead: ~99 % overlapped) is listed, not priced against a roofline
    main_q = {k: v for k, v in per.items() if k not in SIDE_STREAM_CALLS}
    dom = max(main_q, key=main_q.get)
    nmb = (runner.counters()["total_meaningful"] - c_kb0["total_meaningful"])
    smp = runner.get_samples(batches[0][0], batches[0][1], batches[0][2])
    per_ray = (smp["pts_idx_bounds"][:, 1] - smp["pts_idx_bounds"][:, 0]).cpu().numpy()
    out["samples_per_ray"] = {"mean": round(float(per_ray.mean()), 1), "p50": int(np.percentile(per_ray, 50)),
                              "p99": int(np.percentile(per_ray, 99)), "max": int(per_ray.max())}
    roof = {"bound": "hbm", "kernel": dom + (" (one C-ABI call: field MLP backward + hash_bin + hash_bin_accumulate)" if dom == "field_bwd" else ""),
            "queue": "main", "avg_kernel_ms": round(per[dom], 4), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "main_queue_calls_ms_per_step": {k: round(v, 4) for k, v in sorted(main_q.items(), key=lambda kv: -kv[1])},
            "overlapped_on_side_streams_ms_per_step": {k: round(v, 4) for k, v in sorted(per.items(), key=lambda kv: -kv[1]) if k in SIDE_STREAM_CALLS}}
    if dom in ALGO_BYTES_CONVERGED:
        units = (nmb if dom in MEANINGFUL_UNIT else nab) / KB
        ach = units * ALGO_BYTES_CONVERGED[dom] / (per[dom] * 1e-3) / 1e9
        roof.update({"achieved": round(ach, 2), "frac": round(ach / HBM_PEAK_GBS, 5),
                     "bytes_per_sample": ALGO_BYTES_CONVERGED[dom], "unit_of_work": "meaningful sample" if dom in MEANINGFUL_UNIT else "marched sample",
                     "samples_per_launch": int(units)})
    # the gather (one launch per step over every marched sample) against the same bound, whichever call dominates
    if "hash_gather" in per:
        g = nab / KB * ALGO_BYTES_CONVERGED["hash_gather"] / (per["hash_gather"] * 1e-3) / 1e9
        roof["hash_gather"] = {"avg_kernel_ms": round(per["hash_gather"], 4), "achieved": round(g, 2), "frac": round(g / HBM_PEAK_GBS, 5),
                               "bytes_per_marched_sample": 592}
    if dom == "ray_march":  # latency-bound: the launch lasts as long as its longest ray
        roof["latency_model"] = {"longest_ray_steps": int(per_ray.max()), "us_per_step_of_longest_ray": round(per[dom] * 1e3 / max(int(per_ray.max()), 1), 3)}
    out["roofline"] = roof
    return out


def _scatter_counters():
    from f2_nerf_amd import capi
    try:
        c = capi.debug_counters()
    except Exception as e:  # (a diagnostic: never the reason a bench line is lost)
        return {"error": str(e)[:200]}
    import numpy as np
    return {"records_applied_by_atomics": c[0], "slices_summed_in_fp64_instead_of_fixed_point": c[1], "records_through_overflow_lists": c[3],
            # (debug variant of the library only; 0 otherwise) the largest sum of |addend| any slice's owner saw: the fixed-point route holds < 96
            "largest_slice_sum_of_abs_addends": float(np.array(c[2], np.int32).view(np.float32))}


DUMP_TABLE_SAMPLE = 1 << 21  # hash-table entries written by --dump-outputs (8 MiB of fp32): the whole table of 2^19 x 16 x 2 is 64 MiB


def dump_outputs(out_dir, runner, last, n_marched, n_meaningful):
    """--dump-outputs: what the last timed step computed, as a caller of train_step receives it -- its loss terms, its sample
    count (with the marched / meaningful samples of all timed steps: a step's own survivor count is still on the device when
    it returns), the parameters and octree its update left behind -- one float32 / float64 .npy file each (~9 MiB at the default
    preset).  The hash table is sampled at DUMP_TABLE_SAMPLE positions drawn from a fixed seed, so two runs with the same
    arguments compare entry for entry."""
    os.makedirs(out_dir, exist_ok=True)
    st = runner.states()  # checkpoint order: [2] visit counts, [4] table, [8] field MLP, [9] colour MLP, [10] appearance embeddings
    table = st[4].reshape(-1)
    if table.numel() > DUMP_TABLE_SAMPLE:
        pos = np.sort(np.random.default_rng(0).integers(0, table.numel(), DUMP_TABLE_SAMPLE))
        table = table[torch.from_numpy(pos).to(table.device)]
    nodes = runner.tree_nodes().cpu().numpy().view(NODE_DT)
    out = {"loss": np.array([float(last["loss"])]), "mse": np.array([float(last["mse"])]),
           "sample_counts": np.array([last["n_rays"], last["n_samples"], n_marched, n_meaningful], np.float64),
           "hash_table_sample": table.float().cpu().numpy(), "field_mlp": st[8].float().cpu().numpy(),
           "color_mlp": st[9].float().cpu().numpy(), "app_emb": st[10].float().cpu().numpy(),
           "octree_visit_counts": st[2].double().cpu().numpy(),
           "octree_nodes": np.concatenate([nodes["center"], nodes["side_len"][:, None], nodes["trans_idx"][:, None]], 1).astype(np.float64)}
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=800)   # >= 1 s of timed region at ~1.2 ms per step
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--preset", default="wanjinyou", help="wanjinyou (BASELINE config 2, the headline) | wanjinyou_big | free: the fox scene; "
                    "llff | nerf-360: synthetic forward-facing / inward-ring rigs (f2-nerf_amd/rigs.py), octree built on the device")
    ap.add_argument("--log2", type=int, default=0, help="override field.log2_table_size (e.g. 22 for BASELINE config 5's stress point)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-steady", action="store_true", help="skip the %d-step steady-state region that follows a shorter timed region" % STEADY_STEPS)
    ap.add_argument("--no-converged", action="store_true", help="skip the converged-state leg (train 20k iterations, PSNR, timed steps)")
    ap.add_argument("--train-iters", type=int, default=20000, help="iterations of the converged leg's training run")
    ap.add_argument("--converged-steps", type=int, default=600, help="timed steps in the converged state")
    ap.add_argument("--factor", type=int, default=2, choices=[2, 8], help="image resolution of the converged leg (dataset.factor)")
    ap.add_argument("--psnr-runs", type=int, default=4, help="trainings of the PSNR distribution with the product numerics (0: skip)")
    ap.add_argument("--psnr-ref-runs", type=int, default=3, help="... with the reference-numerics build of the kernel library (0: skip)")
    ap.add_argument("--psnr-worker", type=int, default=0, help=argparse.SUPPRESS)  # internal: run N trainings, print their summary
    ap.add_argument("--psnr-no-rerun", action="store_true", help=argparse.SUPPRESS)  # worker: no repeat of seed 2022 at the end
    ap.add_argument("--psnr-seed0", type=int, default=2022, help=argparse.SUPPRESS)  # worker: run r trains from seed psnr_seed0 + r
    ap.add_argument("--psnr-partial", default="", help=argparse.SUPPRESS)  # worker: file that holds the runs finished so far
    ap.add_argument("--other-configs", type=int, default=1, help="1: also run BASELINE configs 3-5 briefly (own processes) and report "
                    "them in the line (N=1, default preset only); 0: skip")
    ap.add_argument("--other-steps", type=int, default=60, help="timed steps of each of those runs")
    ap.add_argument("--breakdown", action="store_true", help="print a per-kernel HIP-event breakdown to stderr")
    ap.add_argument("--marker-pause", action="store_true", help="sleep 0.3 s before the timed region (marker for profiles/timeline_rocpd.py)")
    ap.add_argument("--speculation", choices=["auto", "on", "off"], default="auto", help="sampling of the next batch AHEAD of the stat "
                    "update with repair behind it (Renderer::PreSampleSpecBegin): auto = while no leaf has died lately (the "
                    "default of the host), on / off = A/B (profiles/r03_speculation_experiments.txt, r04_pipeline_experiments.txt)")
    ap.add_argument("--speculation-depth", type=int, default=-1, help="A/B: batches sampled ahead of their step (1 or 2: Renderer.h "
                    "spec_depth_); -1 = host default")
    ap.add_argument("--march-blocks", type=int, default=-1, help="A/B: > 0 marches speculative batches on that many persistent one-wave "
                    "blocks (rays sorted by leaf count), 0 on one block per four rays; -1 = host default")
    ap.add_argument("--knob", action="append", default=[], help="A/B: NAME=VALUE sets an ExpRunner property (tail_repair, march_blocks, "
                    "speculation_depth, ...) on the headline runner; repeatable")
    ap.add_argument("--dp-buckets", type=int, default=0, help="data-parallel runs: table all-reduce in that many buckets (0 = the host's default, 4; 1 = one all-reduce)")
    ap.add_argument("--dp-overlap", type=int, default=-1, help="data-parallel runs: 1 pipelined / 0 blocking gradient exchange; -1 = default (pipelined)")
    ap.add_argument("--diag-no-nan-check", action="store_true", help="diagnostic only: drop the per-step gradient finiteness check")
    ap.add_argument("--full", action="store_true", help="also measure the extras of the line (steady_state, roofline, cpu_baseline, "
                    "converged + PSNR study, other_configs, scatter_counters); a plain run times the headline only")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write what the last timed step computed to DIR/<name>.npy "
                    "(dump_outputs)")
    args = ap.parse_args()

    if args.psnr_worker > 0:
        if not torch.cuda.is_available():
            sys.exit("bench.py needs an MI355X")
        torch.cuda.set_device(0)
        import f2_nerf_amd  # noqa: F401
        print(json.dumps(psnr_runs(args, args.psnr_worker)), flush=True)
        return
    if args.gpus > 1 and "RANK" not in os.environ:
        # stand-alone multi-GPU invocation: one process per GPU over RCCL, exactly as the driver launches it
        import socket
        sock = socket.socket()
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
        sock.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        if os.environ.get("F2N_BENCH_DRY_RUN") == "1":  # (tests/test_parallel_cpu.py: the launcher's command, not the run)
            print(" ".join(cmd))
            return
        os.execvp(sys.executable, cmd)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and not (os.environ.get("F2N_BENCH_FORCE_DP") == "1" and world == 1):
        sys.exit("bench.py --gpus %d was launched with WORLD_SIZE=%d" % (args.gpus, world))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # F2N_BENCH_FORCE_DP=1 (under torch.distributed.run --nproc-per-node 1) exercises the collective path with one rank
    dp = world > 1 or (os.environ.get("F2N_BENCH_FORCE_DP") == "1" and "RANK" in os.environ)
    if dp:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    if not torch.cuda.is_available():
        sys.exit("bench.py needs an MI355X: the hot path has no CPU implementation")
    dev = "cuda:%d" % local_rank
    torch.cuda.set_device(dev)
    # the steps' random draws (march noise, background colours, edge samples) are keyed by the default generator's seed
    # (host/KeyedDraws.h), which is drawn afresh in every process unless set: the same arguments give the same inputs
    torch.manual_seed(2022)

    import f2_nerf_amd  # noqa: F401
    from f2_nerf_amd import runtime
    overrides = ["field.log2_table_size=%d" % args.log2] if args.log2 > 0 else []
    from f2_nerf_amd import rigs
    if args.preset in rigs.PRESET_RIG:   # synthetic rig: same seed on every rank -> identical scene, octree and replica
        runner, cfg, st = rigs.build_runner(args.preset, overrides, seed=2022, device=dev)
        scene_name = "synthetic %s rig (%d cameras, %d octree nodes built on the device)" % (
            rigs.PRESET_RIG[args.preset], len(st["poses"]), runner.n_nodes())
    else:
        st = dict(np.load(os.path.join(ROOT, "tests", "golden", "fox_state.npz")))
        runner, cfg, _ = runtime.make_runner(st, args.preset, overrides, seed=2022, device=dev)   # identical replica on every rank
        scene_name = "ngp_fox"
    log2 = int(cfg["field"]["log2_table_size"])
    if args.diag_no_nan_check:
        runner.check_nan = False
    runner.speculative_sampling = {"auto": 2, "on": 1, "off": 0}[args.speculation]
    if args.speculation_depth >= 1:
        runner.speculation_depth = args.speculation_depth
    if args.march_blocks >= 0:
        runner.march_blocks = args.march_blocks
    for kv in args.knob:
        k, v = kv.split("=")
        setattr(runner, k, type(getattr(runner, k))(int(v)))

    if dp:
        from f2_nerf_amd import parallel
        # per step: all-reduce(AVG) of the 17*2^log2-half active prefix of the fp16 hash-gradient table + MLP/app_emb
        # gradients, and all-reduce(MAX) of the octree occupancy votes (f2-nerf_amd/parallel.py)
        if args.dp_buckets > 0:
            runtime.host().dp_set_table_buckets(args.dp_buckets)
        # (--dp-overlap 1 / 0 force the pipelined / blocking exchange; a forced one-rank world installs its hooks too)
        parallel.attach(runner, log2, overlap=None if args.dp_overlap < 0 else args.dp_overlap == 1, hooks_for_one_rank=(world == 1))

    # synthetic random-pose batches, resident in HBM before the timed region (per-rank RNG stream)
    rng = np.random.default_rng(1000 + rank)
    n_batches = 8
    batches = [runtime.to_dev(*runtime.synthetic_ray_batch(st, args.rays, rng), device=dev) for _ in range(n_batches)]

    def barrier():
        if dp:
            dist.barrier()
        torch.cuda.synchronize()

    def step(i):
        # the next batch's rays are handed over as well: their sampling is prefetched on a side stream underneath this
        # step's backward kernels (the reference draws its rays at the top of every iteration, ExpRunner.cpp:88-91)
        # (two-deep sampling pipeline: the batch after next as well -- it is walked and marched two steps ahead of its use)
        b, nb, nb2 = batches[i % n_batches], batches[(i + 1) % n_batches], batches[(i + 2) % n_batches]
        # (data-parallel ranks run the same program: since round 4 the two-deep pipeline stays on under dp_world > 1)
        if runner.speculation_depth >= 2:
            return runner.train_step(b[0], b[1], b[2], b[3], b[4], True, nb[0], nb[1], nb[2], nb2[0], nb2[1])
        return runner.train_step(b[0], b[1], b[2], b[3], b[4], True, nb[0], nb[1], nb[2])

    for i in range(args.warmup):
        step(i)
    host = runtime.host()
    kernel_timing = rank == 0 and args.full  # (the roofline's HIP events ride in the timed steps of a --full run only)
    if kernel_timing:
        host.ExpRunner.enable_kernel_timing([DOMINANT, "field_mlp_prepass", "field_fwd_cached", "field_fwd", "field_bwd",
                                             "shade_fwd", "shade_bwd"])
    c0 = runner.counters()  # (flushes)
    if dp:  # per-rank diagnostics of the gradient exchange (DataParallel::EnableTiming): what it took, what of it was exposed
        runner.dp_enable_timing(True)
        runner.dp_collect_timing()
    barrier()
    if args.marker_pause:
        time.sleep(0.3)
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        last = step(args.warmup + i)
    runner.flush()  # the last step's survivor count / flags (and, data-parallel, its all-reduce + Adam) belong to the timed region
    barrier()
    elapsed = time.perf_counter() - t0
    c1 = runner.counters()
    n_marched = c1["total_marched"] - c0["total_marched"]
    n_meaningful = c1["total_meaningful"] - c0["total_meaningful"]
    dp_diag = None
    if dp:
        n_ex, ex_ms, n_wt, wt_ms = runner.dp_collect_timing()
        runner.dp_enable_timing(False)
        mine = torch.tensor([ex_ms / max(n_ex, 1), wt_ms / max(n_wt, 1), n_ex], dtype=torch.float64, device=dev)
        allt = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allt, mine)
        dp_diag = {"dp_exchange_ms": [round(float(t[0]), 4) for t in allt], "dp_wait_ms": [round(float(t[1]), 4) for t in allt],
                   "exchanges_timed": [int(t[2]) for t in allt], "small_buffers_exchanged_beside_the_scatter_rank0": int(runner.dp_small_exchanges_early()),
                   "note": "per rank, per step: dp_exchange_ms = first table bucket started -> flat small-gradient buffer reduced, on the "
                           "communicator's stream (its waits for the scatter's later buckets included); dp_wait_ms = what the compute stream "
                           "waited for that exchange at the top of the next step (the part of it the step did not hide)"}
    timing = {}
    if kernel_timing:
        timing = host.ExpRunner.collect_kernel_timing()
        host.ExpRunner.disable_kernel_timing()
    if args.dump_outputs and rank == 0 and last is not None:  # (before the steady-state steps of --full move the state on)
        dump_outputs(args.dump_outputs, runner, last, n_marched, n_meaningful)

    # A short timed region (the driver's 20 steps = 22 ms) sits on the first iterations of a fresh scene; the steady state of
    # this workload is reported next to it: STEADY_STEPS more steps, no kernel timers inside, same barrier bracket (every rank).
    steady = None
    if args.full and args.steps < STEADY_STEPS and not args.no_steady:
        cs0 = runner.counters()
        barrier()
        ts0 = time.perf_counter()
        for i in range(STEADY_STEPS):
            step(args.warmup + args.steps + i)
        runner.flush()
        barrier()
        tse = time.perf_counter() - ts0
        cs1 = runner.counters()
        steady = {"steps": STEADY_STEPS, "ms_per_step": tse / STEADY_STEPS * 1e3,
                  "value_this_rank": (cs1["total_meaningful"] - cs0["total_meaningful"]) / tse, "unit": "ray-samples/s",
                  "note": "follows the timed region; no HIP-event kernel timers inside; the early stop starts to remove samples "
                          "as the scene trains, so meaningful samples per step fall slowly along it"}

    counts = torch.tensor([elapsed, float(n_meaningful), float(n_marched)], dtype=torch.float64, device=dev)
    replicas = None
    if dp:
        # replicas must be bit-identical after the timed steps (same reduced gradients, same octree decisions on every rank):
        # order-free integer checksums of table / MLPs / octree, gathered on rank 0
        stt = runner.states()
        mine = torch.tensor([int(stt[i].contiguous().view(torch.int32).to(torch.int64).sum().item()) for i in (4, 8, 9)] +
                            [int(stt[0].to(torch.int64).sum().item()), runner.n_nodes()], dtype=torch.int64, device=dev)
        allc = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allc, mine)
        sums = [[int(v) for v in t.tolist()] for t in allc]
        replicas = {"identical": all(s_ == sums[0] for s_ in sums), "checksums_table_fieldmlp_colormlp_nodes_nnodes": sums,
                    "rccl_comm_ranks": int(runner.dp_comm_ranks()), "torch_distributed_world": world}
    if dp:
        tmax = counts[:1].clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        tot = counts[1:].clone()
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        elapsed, n_meaningful, n_marched = float(tmax[0]), float(tot[0]), float(tot[1])

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = n_meaningful / elapsed
        rho = n_marched / max(n_meaningful, 1.0)
        # --- roofline of the dominant kernel ---
        roofline = None
        if timing and DOMINANT in timing:
            launches, total_ms = timing[DOMINANT]
            avg_ms = total_ms / max(launches, 1)
            samples_per_launch = n_marched / world / args.steps
            achieved = samples_per_launch * ALGO_BYTES[DOMINANT] / (avg_ms * 1e-3) / 1e9
            traffic = None
            # per-workload counter files (profiles/run_profiles.sh): the headline workload, or the big-table stress points
            tfile = TRAFFIC_FILE
            if args.preset == "wanjinyou_big":  # (2^21 and up: the slice-binned gather of round 4, four kernels behind one call)
                # (the newest counter pass of this table size: round 5 re-took 2^20 after the binned gather was extended to it)
                tfile = next((f for f in (os.path.join(ROOT, "profiles", "r%02d_big%d_traffic.json" % (r, log2)) for r in (6, 5, 4, 3)) if os.path.exists(f)), "")
            elif args.preset in ("llff", "nerf-360") and args.log2 in (0, 19) and args.rays == 8192:
                # (round 6: the rigs' own counter passes -- BENCH_EXTRA="--preset llff" bash profiles/run_profiles.sh r06_llff)
                tfile = os.path.join(ROOT, "profiles", "r06_%s_traffic.json" % args.preset)
            elif args.preset != "wanjinyou" or args.log2 not in (0, 19) or args.rays != 8192:
                tfile = ""  # (no counters were collected for this workload)
            traffic_source = None
            if tfile and os.path.exists(tfile):
                with open(tfile) as f:
                    per_kernel = json.load(f)
                traffic = sum(v.get("hbm_bytes_per_launch", 0.0) for k, v in per_kernel.items()
                              if "hash_gather_planes_kernel" in k or "gather_request_kernel" in k or "gather_serve_kernel" in k or "gather_blend_kernel" in k) or None
                # (PMC counters cannot ride in a timed run: the figure is READ from the committed counter pass of this workload)
                traffic_source = "%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of profiles/run_profiles.sh; not measured in this run)" % os.path.relpath(tfile, ROOT)
            roofline = {"bound": "hbm", "kernel": "hash_gather_planes_kernel", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
                        "traffic_source": traffic_source,
                        "avg_kernel_ms": round(avg_ms, 4), "launches": launches, "bytes_per_sample": ALGO_BYTES[DOMINANT],
                        "samples_per_launch": int(samples_per_launch),
                        "request_ceiling": {"achieved": round(samples_per_launch * 128 / (avg_ms * 1e-3) / 1e9, 1),
                                            "peak": GATHER_REQ_PEAK / 1e9, "unit": "G 4-byte gathers/s",
                                            "frac": round(samples_per_launch * 128 / (avg_ms * 1e-3) / GATHER_REQ_PEAK, 4)},
                        # what physically bounds it: each of the 128 hashed reads of a sample pulls one 128-byte line out of
                        # an XCD's L2 into a CU's L1 (the primes are random on all three axes: no two corners share a line)
                        "l2_line_bandwidth": {"achieved": round(samples_per_launch * 128 * 128 / (avg_ms * 1e-3) / 1e12, 2),
                                              "peak": L2_PEAK_TBS, "unit": "TB/s (128-byte lines, L2 -> L1, all 8 XCDs)",
                                              "frac": round(samples_per_launch * 128 * 128 / (avg_ms * 1e-3) / 1e12 / L2_PEAK_TBS, 4),
                                              "model": "128 lines per sample = no line shared between samples: exact for the fox scene at "
                                                       "fineness 16; an upper bound (frac may exceed 1) where consecutive samples of a ray share "
                                                       "cells -- short march steps: llff / nerf-360 presets, converged scenes -- and the "
                                                       "run-combining kernel reads a shared cell once"},
                        # whole-path fractions from the same run -- table bytes 512*(rho+2) per meaningful sample
                        # against 8 TB/s, MLP flops (61440 + 6144 rho) against the 2.5 PFLOP/s dense f16 peak
                        "whole_path": {"gather_scatter_frac_of_hbm": round(value / max(world, 1) * 512 * (rho + 2) / 8.0e12, 5),
                                       "mlp_frac_of_mfma": round(value / max(world, 1) * (61440 + 6144 * rho) / 2.5e15, 5)},
                        "timed_calls_ms_per_step": {k: round(v[1] / args.steps, 4) for k, v in timing.items()}}
            if traffic:  # counter traffic against the same launch's duration: what the memory side actually moved per second
                roofline["traffic_rate"] = {"achieved": round(traffic / (avg_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                            "frac": round(traffic / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                            "note": "FETCH_SIZE (x2, gfx950) + WRITE_SIZE per launch / launch duration: far below 1 with an L2-"
                                                    "resident table (2^19: the reads never leave the XCD), ~0.75 where every 4-byte read "
                                                    "pulls a 128-byte line across the fabric (2^20; 2^22 before round 4's slice-binned gather: "
                                                    "profiles/r03_big22_pmc_tcc.csv, profiles/r04_binned_gather.txt)"}
        cpu_baseline = None
        if world == 1 and args.full and not args.no_cpu_baseline:
            try:
                env = dict(os.environ, F2N_ORACLE_OMP="1")
                out = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "baseline.py")], capture_output=True,
                                     text=True, timeout=600, env=env)
                cpu_baseline = json.loads(out.stdout.strip().splitlines()[-1])
            except Exception as e:  # the baseline is a reported extra, never the thing measured
                cpu_baseline = {"error": str(e)[:200]}
        converged = None
        if world == 1 and args.full and not args.no_converged and scene_name == "ngp_fox":
            try:
                converged = converged_leg(args, st, dev)
            except Exception as e:  # reported next to the headline, never instead of it
                import traceback
                converged = {"error": (str(e) + " | " + traceback.format_exc()[-600:])[:900]}
            if args.psnr_runs > 0 or args.psnr_ref_runs > 0:  # (after every timed region)
                try:
                    converged["psnr_numerics_ab"] = psnr_numerics_ab(args)
                except Exception as e:
                    converged["psnr_numerics_ab"] = {"error": str(e)[:300]}
        others = None
        if world == 1 and args.full and args.other_configs and args.preset == "wanjinyou" and args.log2 in (0, 19) and not args.no_converged:
            try:
                torch.cuda.empty_cache()
                others = other_configs(args)
            except Exception as e:
                others = {"error": str(e)[:300]}
        training_representative = None
        if converged and "value" in converged:
            training_representative = {
                "value": converged["value"], "unit": "ray-samples/s", "ms_per_step": converged["ms_per_step"],
                "note": "a 20 000-iteration training spends > 90 % of its steps in this regime (pruned ~1.4e5-node octree, adaptive ~14 k rays, "
                        "rho ~2): quote THIS figure for training throughput; `value` above is the fresh-table state BASELINE config 2 is "
                        "quoted on (rho = 1, nothing early-stops), the flattering one of the two (round-4 verdict, weak 9)"}
        line = {
            "metric": "training ray-samples/s (%s)" % ("ngp_fox" if scene_name == "ngp_fox" else args.preset), "value": value, "unit": "ray-samples/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
            "config": {"workload": "%s %s.yaml, %d rays/batch/GPU, 2^%d x16 table, the first %d iterations of training from "
                                   "the fresh-initialised table (fineness %.1f), synthetic random-pose rays, full train step "
                                   "(fwd+bwd+Adam+octree update)" % (scene_name, args.preset, args.rays, log2, args.warmup + args.steps, runner.fineness),
                       "rays_per_batch": args.rays, "parallelism": "ray-dp%d" % world,
                       "rays_per_s": args.rays * world * args.steps / elapsed,
                       "marched_samples_per_s": n_marched / elapsed, "rho_marched_over_meaningful": rho,
                       "meaningful_samples_per_step": n_meaningful / args.steps},
            "training_representative": training_representative,
            "steady_state": steady, "roofline": roofline, "cpu_baseline": cpu_baseline, "converged": converged, "replicas": replicas,
            "data_parallel": dp_diag,
            "other_configs": others,
            # whole process so far (timed steps, converged leg, other configs): 0 atomic records = every hash-gradient sum was order-free
            "scatter_counters": _scatter_counters() if args.full else None,
            # buffers are sized for the worst case on purpose (1024 sample slots per ray, scatter queues): what that costs of 288 GB
            "peak_hbm_gib": {"allocated": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                             "reserved_by_allocator": round(torch.cuda.max_memory_reserved() / 2 ** 30, 2),
                             "note": "torch allocator only; the C-ABI library's own workspaces (scatter queues, planes) add ~1.3 GiB"},
        }
        print(json.dumps(line), flush=True)

    if args.breakdown and rank == 0:
        host.ExpRunner.enable_kernel_timing(["*"])
        for i in range(5):
            step(i)
        torch.cuda.synchronize()
        t = host.ExpRunner.collect_kernel_timing()
        host.ExpRunner.disable_kernel_timing()
        tot = sum(v[1] for v in t.values())
        for k, v in sorted(t.items(), key=lambda kv: -kv[1][1]):
            print("  %-22s launches %3d  %8.3f ms/step  %5.1f%%" % (k, v[0] // 5, v[1] / 5, 100 * v[1] / tot), file=sys.stderr)
        print("  sum of timed kernels: %.3f ms/step" % (tot / 5), file=sys.stderr)
    if dp:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
