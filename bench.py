#!/usr/bin/env python3
"""Benchmark of the planning hot path: python bench.py --gpus N --steps K --warmup W

One "step" = one inner planning iteration (forward, criterion, backward-data, Adam + projection;
paule/paule.py:910-1211 without the log-step block) over the whole per-GPU batch, on synthetic
inputs already resident in HBM.  Default workload = the configuration BASELINE.json's metric is quoted
on (cfg3): B = 256 utterances x 300 CP frames per GPU, objective acoustic_semvec, model set A
(ForwardModel L1/H720 + EmbeddingModel L2/H720), bf16 GEMMs.  N > 1: the batch dimension is sharded,
one process per GPU, no collective inside the loop; one RCCL all_gather of the final CP trajectories
afterwards (timed separately).  Rank 0 prints ONE JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (batch per GPU, frames, objective, dtype, model set)
    # cfg1: the reference's own case -- ONE utterance, Paule's default models, acoustic + semantic objective; the CPU baseline
    # of this config runs the oracle in float64 (the reference's dtype) on that one utterance
    "cfg1": dict(batch=1, frames=300, objective="acoustic_semvec", dtype="f32", model_set="A", cpu_f64=True),
    # the same single utterance in bf16: one 16-row group on the 16-row fused launches (lstm_fused16.h)
    "cfg1_bf16": dict(batch=1, frames=300, objective="acoustic_semvec", dtype="bf16", model_set="A", cpu_f64=True),
    "cfg2": dict(batch=64, frames=300, objective="acoustic", dtype="f32", model_set="A"),
    "cfg3": dict(batch=256, frames=300, objective="acoustic_semvec", dtype="bf16", model_set="A"),
    "cfg3_f32": dict(batch=256, frames=300, objective="acoustic_semvec", dtype="f32", model_set="A"),
    "cfg3_setB": dict(batch=256, frames=300, objective="acoustic_semvec", dtype="bf16", model_set="B"),
    "cfg3_setC": dict(batch=256, frames=300, objective="acoustic_semvec", dtype="bf16", model_set="C"),   # older embedder (8f rank 4)
    "cfg3_soma": dict(batch=256, frames=300, objective="acoustic_semvec", dtype="bf16", model_set="A", tube=True),   # + somatosensory path
    "cfg5": dict(batch=16, frames=2000, objective="acoustic_semvec", dtype="bf16", model_set="A"),
    # cfg5's whole batch (128 utterances) on ONE GPU: a 2000-step sweep costs about the same for 128 rows as for 16 (step latency),
    # so sharding cfg5 over 8 GPUs buys little over this (Measured)
    "cfg5_128": dict(batch=128, frames=2000, objective="acoustic_semvec", dtype="bf16", model_set="A"),
    "cfg2_setB": dict(batch=64, frames=300, objective="acoustic", dtype="f32", model_set="B"),
    "cfg5_setB": dict(batch=16, frames=2000, objective="acoustic_semvec", dtype="bf16", model_set="B"),
    # small enough for several ranks to share ONE GPU (two persistent sweeps side by side need all their workgroups resident):
    # used with --dist-backend gloo --device-index 0 to rehearse the multi-rank path on a one-GPU box
    "rehearsal": dict(batch=8, frames=60, objective="acoustic_semvec", dtype="bf16", model_set="A"),
    # cfg4's whole batch (2048 utterances) on ONE GPU: 15.5 GB of the 288 GB; 64 batch groups swept 8 at a time
    "cfg4_1gpu": dict(batch=2048, frames=300, objective="acoustic_semvec", dtype="bf16", model_set="A"),
    # one pred_optimizer step of the continued learning (paule/paule.py:1372-1377), batch_size = 8 (:404)
    "train8": dict(batch=8, frames=300, objective="acoustic", dtype="bf16", model_set="A", train=True),
    "train8_f32": dict(batch=8, frames=300, objective="acoustic", dtype="f32", model_set="A", train=True),
}
PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3}   # dense MFMA peaks, MI355X_MICROARCH.md chip-level parameters
DUMP_LIMIT = 64 << 20   # bytes that --dump-outputs writes at most
DUMP_SEED = 20200905


def dump_outputs(dirname, outputs):
    """--dump-outputs: writes every array of ``outputs`` (name -> tensor / array, rows first) as DIR/<name>.npy, float32 (float64
    stays float64).  When all of them together exceed DUMP_LIMIT, every array keeps the same share of its rows, drawn with a
    fixed seed, and DIR/<name>_rows.npy lists the rows kept: two builds write the same sample.  Returns the names written."""
    import numpy as np
    arrs = {}
    for name, v in outputs.items():
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        arrs[name] = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
    total = sum(a.nbytes for a in arrs.values())
    if total > DUMP_LIMIT:
        share = 0.95 * DUMP_LIMIT / total   # room for the row lists
        for name in list(arrs):
            a = arrs[name]
            if a.ndim == 0 or a.shape[0] < 2:
                continue
            rows = np.sort(np.random.default_rng(DUMP_SEED).choice(a.shape[0], size=max(1, int(a.shape[0] * share)), replace=False))
            arrs[name] = np.ascontiguousarray(a[rows])
            arrs[name + "_rows"] = rows.astype(np.float64)
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrs.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    progress(f"outputs of the last timed step written to {dirname} ({sum(a.nbytes for a in arrs.values()) / 2**20:.1f} MiB)")
    return sorted(arrs)


def cpu_baseline(wl_args, objective, seconds_budget=25.0, full=False):
    """The CPU oracle (torch nn.LSTM + autograd + Adam: the operators the reference executes) on a bounded sample
    of the same workload, float32, all host cores.  Baseline, not target."""
    import torch
    from oracle import planner as op
    from paule_amd import synthetic
    # the GPU box gives one GPU a share of 16 host cores; os.cpu_count() reports the whole machine and
    # over-subscribing OpenMP threads stalls torch for minutes
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    nthreads = max(1, min(avail, 16))
    torch.set_num_threads(nthreads)
    f64 = bool(wl_args.get("cpu_f64"))
    cdt = torch.float64 if f64 else torch.float32
    def run(n_utt, min_iters, budget, max_iters):
        wl = synthetic.make_workload(n_utt, wl_args["frames"], wl_args["model_set"])
        orc = op.OraclePlanner(op.forward_model_from_state_dict(wl.pred_sd, cdt),
                               op.embedding_model_from_state_dict(wl.emb_sd, cdt), objective=objective,
                               dtype=cdt)
        orc.set_targets(wl.target_mel, wl.target_semvec)
        orc.set_cp(wl.cp0)
        orc.step(1)   # warm-up
        iters, t0 = 0, time.perf_counter()
        while iters < min_iters or (time.perf_counter() - t0 < budget and iters < max_iters):
            orc.step(1)
            iters += 1
        return iters, time.perf_counter() - t0

    B = wl_args["batch"]
    sample_b = min(16, B)
    progress(f"cpu baseline: {nthreads} threads, sample of {sample_b} utterances")
    # a short sample first: it is the baseline itself when the full batch would cost minutes, and the estimate that decides otherwise
    s_iters, s_dt = run(sample_b, 2, 4.0 if not full and B > sample_b else seconds_budget, 50)
    sample_it_s = sample_b * s_iters / s_dt / B          # planning iterations/s at the full batch, extrapolated from the sample
    # SURVEY 8d asks for 1 warm-up + 3 timed iterations AT the configuration's batch.  The oracle is ~2.4 x slower per utterance at
    # B = 256 than on 16 utterances (r2: 0.115 vs 0.272 it/s), so the sample flatters the CPU; the full batch is timed whenever its
    # estimated cost (4 iterations) stays under a minute
    est_full = 4 * (B / sample_b) * (s_dt / s_iters) * 2.4
    desc = f"T={wl_args['frames']}, {objective}, model set {wl_args['model_set']}, {'float64' if f64 else 'float32'}, torch CPU oracle"
    if B > sample_b and (full or est_full < 60.0):
        progress(f"cpu baseline: full batch of {B} utterances (estimated {est_full:.0f} s)")
        f_iters, f_dt = run(B, 3, 0.0, 3)
        return dict(value=f_iters / f_dt, unit=f"planning iters/sec at batch={B}", utt_iters_per_s=B * f_iters / f_dt,
                    cores=torch.get_num_threads(), kind="port",
                    sample=f"{B} utterances x {f_iters} iterations after 1 warm-up, {desc} ({f_dt:.1f} s)",
                    sample16_value=sample_it_s,
                    sample16=f"{sample_b} utterances x {s_iters} iterations ({s_dt:.1f} s): {sample_it_s:.3f} it/s extrapolated -- the small sample flatters the CPU")
    return dict(value=sample_it_s,
                unit=f"planning iters/sec at batch={B}" + ("" if B == sample_b else " (extrapolated from the sample)"),
                utt_iters_per_s=sample_b * s_iters / s_dt, cores=torch.get_num_threads(), kind="port",
                sample=f"{sample_b} utterances x {s_iters} iterations, {desc} ({s_dt:.1f} s)"
                       + ("" if B == sample_b else f"; the full batch was estimated at {est_full:.0f} s and not timed (--cpu-full forces it)"))


def cpu_baseline_train(cfg, seconds_budget=20.0):
    """OracleTrainer (torch autograd + torch.optim.Adam on the CPU) on the same mini-batch, float32."""
    import torch
    from oracle import planner as op
    from paule_amd import synthetic
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(avail, 16)))
    wl = synthetic.make_workload(cfg["batch"], cfg["frames"], cfg["model_set"])
    tr = op.OracleTrainer(op.forward_model_from_state_dict(wl.pred_sd, torch.float32), dtype=torch.float32)
    cp, mel = wl.cp0.float(), wl.target_mel.float()
    tr.train_pred_step(cp, mel)
    n, t0 = 0, time.perf_counter()
    while n < 2 or (time.perf_counter() - t0 < seconds_budget and n < 30):
        tr.train_pred_step(cp, mel)
        n += 1
    dt = time.perf_counter() - t0
    return dict(value=n / dt, unit="optimiser steps/s", cores=torch.get_num_threads(), kind="port",
                sample=f"{n} steps, mini-batch {cfg['batch']} x {cfg['frames']} frames, model set {cfg['model_set']}, float32, "
                       f"torch CPU oracle ({dt:.1f} s)")


def bench_train(args, cfg):
    """One step = one optimiser step of the predictive model on a mini-batch resident in HBM (pl_train_pred_step)."""
    import torch
    from paule_amd import synthetic
    from paule_amd.engine import HipPlanner
    B, T = cfg["batch"], cfg["frames"]
    wl = synthetic.make_workload(B, T, cfg["model_set"])
    eng = HipPlanner(wl.pred_sd, None, batch=B, n_frames=T, objective="acoustic", dtype=cfg["dtype"])
    cp, mel = wl.cp0.float().cuda(), wl.target_mel.float().cuda()
    for _ in range(max(1, args.warmup)):
        eng.train_pred_step(cp, mel)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = [eng.train_pred_step(cp, mel) for _ in range(args.steps)]
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    eng.synchronize()
    dumped = None
    if args.dump_outputs:   # the last step's loss and the parameters it left (what pred_model.load_state_dict receives)
        outs = {"loss": losses[-1].reshape(1)}
        outs.update({f"pred.{k}": v for k, v in eng.get_weights("pred").items()})
        dumped = dump_outputs(args.dump_outputs, outs)
    H, I, M = 720, 30, 60
    per_frame = 4 * H * (I + H) + H * M
    flops = 2 * B * T * per_frame * 3                      # forward + backward-data + weight gradients
    ms, fl = eng.bench_kernel("bwd_sweep", "pred", reps=5)
    eng.synchronize()
    peak = PEAK_TFLOPS[cfg["dtype"]]
    out = {"metric": f"pred_model optimiser steps/sec, mini-batch={B} x {T}-frame CP trajs", "value": args.steps / elapsed,
           "unit": "steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": cfg["dtype"],
           "data": "synthetic (random-init weights, random smooth inputs / targets)",
           "config": {"workload": f"{args.config}: continued learning of the predictive model, mini-batch {B} x {T} frames, "
                                  f"model set {cfg['model_set']}, RMSE + Adam(lr 0.001)"},
           "algorithmic_gflop_per_step": flops / 1e9, "loss_first": float(losses[0]), "loss_last": float(losses[-1]),
           # the kernel pl_bench_kernel really launches for a mini-batch of <= 128 rows: the 16-row reduce-scatter sweep in bf16 (VERDICT r3:
           # the line named the 32-row kernel), the f32 sweep otherwise
           "roofline": {"bound": "mfma", "kernel": ("lstm_bwd16_rs_sweep_kernel" if B <= 128 else "lstm_bwd_rs_stream_kernel") if cfg["dtype"] == "bf16" else "lstm_bwd_sweep_f32_kernel",
                        "achieved": fl / (ms * 1e-3) / 1e12, "peak": peak, "unit": "TFLOP/s",
                        "frac": fl / (ms * 1e-3) / 1e12 / peak, "traffic": None, "avg_launch_us": ms * 1e3}}
    if dumped is not None:
        out["dumped_outputs"] = dumped
    if not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_train(cfg)
    print(json.dumps(out), flush=True)


def progress(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def plumbing_only(args, cfg):
    """The N-rank skeleton of main() with the engine cut out: what can be checked where there is no GPU."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs WORLD_SIZE={args.gpus} (got {world})")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    B, T = cfg["batch"], cfg["frames"]
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    time.sleep(0.01 * (rank + 1))          # the "steps": ranks finish at different times, the job's time is the slowest rank's
    elapsed = time.perf_counter() - t0
    cp = torch.full((B, T, 30), float(rank))
    outs = [cp]
    if world > 1:
        dist.barrier()
        tmax = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
        outs = [torch.empty_like(cp) for _ in range(world)]
        dist.all_gather(outs, cp)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"cp": torch.cat(outs)})
    if rank == 0:
        print(json.dumps({"plumbing_only": True, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": elapsed / max(1, args.steps) * 1e3, "scaling": "weak",
                          "gathered_rows": int(sum(o.shape[0] for o in outs)),
                          "gathered_ranks_ok": all(float(o[0, 0, 0]) == r for r, o in enumerate(outs))}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _uses_sweep16(hidden, batch, n_cu=256):
    """lstm_sweep16_wanted (paule_amd/csrc/lstm_persist16.hip) restated for the kernel name in the roofline object: groups of 16
    rows when all of them are resident at once, up to 128 rows or, for narrow models, up to half the chip."""
    hp, bp = -(-hidden // 32) * 32, -(-batch // 16) * 16
    p, groups = hp // 32, bp // 16
    return bp <= 16 or (groups * p <= n_cu and (bp <= 128 or groups * p <= n_cu // 2))


def source_digest():
    """Digest of the kernel sources: what profiles/traffic.json was measured on (the GPU box has no .git to ask for HEAD)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "paule_amd", "csrc")
    for fn in sorted(os.listdir(d)):
        if fn.endswith((".hip", ".h")):
            h.update(fn.encode())
            h.update(open(os.path.join(d, fn), "rb").read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="cfg3", choices=sorted(CONFIGS))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl (= RCCL, the product path); gloo only to rehearse the multi-rank plumbing with several ranks on ONE GPU")
    ap.add_argument("--device-index", type=int, default=-1, help="HIP device of this rank (default: LOCAL_RANK)")
    ap.add_argument("--strong-total", type=int, default=0,
                    help="strong scaling: this many utterances in total, split evenly over the ranks (e.g. 2048 = cfg4); "
                         "default 0 = weak scaling with the config's per-GPU batch")
    ap.add_argument("--cpu-full", action="store_true",
                    help="CPU baseline at the real configuration (all B utterances, 1 warm-up + 3 timed iterations: about a minute at "
                         "cfg3) instead of the bounded 16-utterance sample")
    ap.add_argument("--plumbing-only", action="store_true",
                    help="multi-rank plumbing without an engine (rendezvous, barrier, max-over-ranks timing, all_gather of a CP-shaped "
                         "tensor, rank-0 JSON): what tests/test_host.py runs on a machine without a GPU; prints \"plumbing_only\": true")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (final CP trajectories and loss rows; training "
                         "configs: loss and parameters) as DIR/<name>.npy, float32, at most 64 MB (a fixed sample of rows beyond that)")
    args = ap.parse_args()
    cfg = CONFIGS[args.config]
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # not under a launcher: start one rank per GPU ourselves -- as CHILD processes, before anything here touches the GPU
        # (nothing has: torch is not even imported yet), and leave with their exit code
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        progress(f"no launcher environment: starting {args.gpus} ranks: {' '.join(cmd[1:8])} ...")
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        raise SystemExit(subprocess.run(cmd, env=env).returncode)
    if args.plumbing_only:
        return plumbing_only(args, cfg)
    if cfg.get("train"):
        if args.gpus != 1:
            raise SystemExit("the training configs are single-GPU")
        return bench_train(args, cfg)

    import torch
    import torch.distributed as dist
    from paule_amd import synthetic
    from paule_amd.engine import HipPlanner

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} needs a torch.distributed launch with WORLD_SIZE={args.gpus} (got {world})")
    dev_index = local_rank if args.device_index < 0 else args.device_index
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    gloo = args.dist_backend == "gloo"
    coll = (lambda t: t.cpu()) if gloo else (lambda t: t)   # gloo rehearsal: collectives on host copies
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if gloo:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    B, T = cfg["batch"], cfg["frames"]
    if args.strong_total:
        if args.strong_total % world:
            raise SystemExit(f"--strong-total {args.strong_total} is not divisible by {world} ranks")
        B = args.strong_total // world
    # same random-init weights on every rank (same seed), different utterances per rank (weak scaling)
    wl = synthetic.make_workload(B, T, cfg["model_set"], seed=synthetic.SEED)
    if rank:
        wl_r = synthetic.make_workload(B, T, cfg["model_set"], seed=synthetic.SEED + 1000 * rank)
        wl = wl._replace(target_mel=wl_r.target_mel, target_semvec=wl_r.target_semvec, cp0=wl_r.cp0)
    tube_kw = dict(tube_models=synthetic.make_tube_models()) if cfg.get("tube") else {}
    eng = HipPlanner(wl.pred_sd, wl.emb_sd, batch=B, n_frames=T, objective=cfg["objective"], dtype=cfg["dtype"],
                     device=device, use_graph=not args.no_graph, **tube_kw)
    eng.set_targets(wl.target_mel, wl.target_semvec)
    eng.set_cp(wl.cp0)

    def barrier():
        if world > 1:
            dist.barrier()

    progress(f"engine ready ({eng.device_bytes / 2**30:.2f} GiB on device); warm-up")
    if args.warmup > 0:
        eng.step(args.warmup, return_loss=False)
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = eng.step(args.steps)                 # EXACTLY K steps
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    barrier()
    if world > 1:
        tmax = coll(torch.tensor([elapsed], dtype=torch.float64, device=device))
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())

    # the single collective of the path: gather the final CP trajectories (outside the timed loop)
    gather_ms = None
    cp = eng.get_cp()
    if world > 1:
        cpc = coll(cp)
        outs = [torch.empty_like(cpc) for _ in range(world)]
        torch.cuda.synchronize()
        tg = time.perf_counter()
        dist.all_gather(outs, cpc)
        torch.cuda.synchronize()
        gather_ms = (time.perf_counter() - tg) * 1e3
    eng.synchronize()   # surfaces device-side failures (bounded in-kernel waits) -- outside the timed region
    finite = bool(torch.isfinite(loss).all().item() and torch.isfinite(cp).all().item())
    dumped = None
    if args.dump_outputs and rank == 0:   # the final CP trajectories (all ranks') and the last step's loss rows [B, 8]
        dumped = dump_outputs(args.dump_outputs, {"cp": torch.cat([o.cpu() for o in outs]) if world > 1 else cp, "loss": loss[-1]})

    if rank == 0:
        progress(f"timed region done: {elapsed / args.steps * 1e3:.3f} ms/step")
        # weak scaling: every rank iterates its own batch of B, the job does world x steps "batch = B" iterations;
        # strong scaling: one iteration covers the whole --strong-total batch across the ranks
        it_s = (1 if args.strong_total else world) * args.steps / elapsed
        flops_it = eng.flops_per_iteration
        # dominant kernel: the LSTM backward sweep of the predictive model (one launch = T steps), or the launch-per-step
        # backward kernel when the sweeps are switched off / unsupported.  Timed with hipEvents on the engine's stream.
        swept = True
        names = ("bwd_sweep", "fwd_sweep") if swept else ("bwd", "fwd")
        roof = {}
        for name in names:
            try:
                roof[name] = eng.bench_kernel(name, "pred", reps=5 if swept else min(298, T - 2) * 2)
            except ValueError:
                swept, names = False, ("bwd", "fwd")
                break
        if not swept:
            roof = {name: eng.bench_kernel(name, "pred", reps=min(298, T - 2) * 2) for name in names}
        eng.synchronize()
        ms, fl = roof[names[0]]
        ms_f, fl_f = roof[names[1]]
        fused = None   # the fused forward launch (all forward LSTM layers + the mel head as roles of one grid), when the handle runs it
        try:
            fused = eng.bench_kernel("fused_fwd", "pred", reps=5)
            eng.synchronize()
        except ValueError:
            fused = None
        rs = os.environ.get("PAULE_HIP_BWD_MODE", "1") == "1"   # reduce-scatter form is the library default
        plan = eng.plan_info()
        fused_b = None   # the fused backward launch, when the handle's plan runs it (49 ... 128 rows by default): THE backward kernel of the timed iteration
        if plan["fused_bwd"]:
            fused_b = eng.bench_kernel("fused_bwd", "pred", reps=5)
            eng.synchronize()
        if not swept:
            kname = "lstm_bwd_step_kernel"
        elif cfg["dtype"] == "f32":
            # more 16-row groups than the chip holds at once (256 CUs / (Hp / 16) workgroups per group): the chains kernels
            hp = -(-int(eng.pred_hidden) // 32) * 32   # feature dimensions are padded to multiples of 32
            chained = -(-cfg["batch"] // 16) > 256 // (hp // 16) and os.environ.get("PAULE_HIP_F32_CHAINS", "-1") != "0" and hp in (96, 736)
            kname = "lstm_bwd_chain_f32_kernel" if chained else "lstm_bwd_sweep_f32_kernel"
        elif _uses_sweep16(int(eng.pred_hidden), cfg["batch"]) and os.environ.get("PAULE_HIP_SWEEP16", "1") != "0" and rs:
            kname = "lstm_bwd16_rs_sweep_kernel"   # the 16-row kernels (what pl_bench_kernel launches for this width and batch)
        else:
            streamed = rs and os.environ.get("PAULE_HIP_BWD_STREAM", "1") != "0" and os.environ.get("PAULE_HIP_BWD_WAVES", "8") != "4"
            kname = ("lstm_bwd_rs_stream_kernel" if streamed else "lstm_bwd_rs_sweep_kernel") if rs else "lstm_bwd_sweep_kernel"
        per_layer = None
        if fused_b is not None:   # name and rate the kernel the timed iteration runs; keep the per-layer kernel's figures beside it
            per_layer = {"kernel": kname, "avg_launch_us": ms * 1e3, "flops_per_launch": fl, "achieved": fl / (ms * 1e-3) / 1e12,
                         "note": "per-layer backward sweep of the predictive model, timed on its own (the A/B reference, PAULE_HIP_FUSED=1)"}
            kname = "fused_bwd16_kernel" if plan.get("fused_rows") == 16 else "fused_bwd_kernel"   # 16: batches of up to 16 rows (lstm_fused16.h)
            if cfg["model_set"] == "B":
                kname += "2"   # stacked predictor of another width than the embedder: the two-width kernels
            ms, fl = fused_b
        achieved = fl / (ms * 1e-3) / 1e12
        peak = PEAK_TFLOPS[cfg["dtype"]]
        # HBM bytes per launch of that kernel from the PMC passes (rocprofv3 --pmc, profiles/README.md): a measurement of ANOTHER run of
        # the same command, so it is only reported while the kernel sources are the ones it was taken on
        traffic, traffic_note = None, "no PMC pass recorded for this configuration"
        tpath = os.path.join(ROOT, "profiles", "traffic.json")
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                if tj.get("source_digest") != source_digest():
                    traffic_note = f"profiles/traffic.json was measured on other kernel sources (digest {tj.get('source_digest')}): not reported"
                else:
                    traffic = tj.get(args.config, {}).get(kname + "_bytes_per_launch")
                    traffic_note = "profiles/traffic.json (separate --pmc passes of this command, same kernel sources)" if traffic else traffic_note
            except Exception:
                traffic = None
        # algorithmic HBM bytes per utterance-iteration = CP / Adam streams + stash written once and read once
        spec = synthetic.MODEL_SETS[cfg["model_set"]]
        esz = 2 if cfg["dtype"] == "bf16" else 4
        layers = [(spec["pred"]["hidden_size"], T)] * spec["pred"]["num_lstm_layers"]
        if cfg["objective"] != "acoustic":
            layers += [(spec["emb"]["hidden_size"], T // 2)] * spec["emb"]["num_lstm_layers"]
        if cfg.get("tube"):
            layers += [(sp["hidden_size"], T) for sp in synthetic.TUBE_SPECS.values() for _ in range(sp["num_lstm_layers"])]
        bytes_utt = 6 * T * 30 * 4 + (T // 2) * 60 * esz + 2 * esz * sum(6 * hl * tl for hl, tl in layers)
        out = {
            # cfg3 is the configuration BASELINE.json's metric is quoted on: its string verbatim
            "metric": "planning iters/sec, batch=256 \u00d7 300-frame CP trajs; 1/2/4/8 MI355X" if args.config == "cfg3" and not args.strong_total
                      else f"planning iters/sec, batch={args.strong_total or B} x {T}-frame CP trajs",
            "value": it_s, "unit": "iters/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong" if args.strong_total else "weak",
            "vs_baseline": None, "dtype": cfg["dtype"], "data": "synthetic (random-init weights, random smooth targets)",
            "config": {"workload": f"{args.config}: {B} utterances/GPU x {T} CP frames, objective {cfg['objective']}, "
                                   f"model set {cfg['model_set']}", "objective": cfg["objective"],
                       "batch_per_gpu": B, "global_batch": B * world, "n_frames": T, "model_set": cfg["model_set"],
                       "parallelism": f"batch-sharded x{world}, no collective in the loop", "hip_graph": not args.no_graph},
            "utt_iters_per_s": world * B * args.steps / elapsed,
            "algorithmic_gflop_per_iter": flops_it / 1e9,
            "whole_iteration_mfma_frac": (flops_it * args.steps / elapsed) / (peak * 1e12),   # per GPU
            "algorithmic_mbyte_per_utt_iter": bytes_utt / 1e6,
            "whole_iteration_hbm_frac": (bytes_utt * B * args.steps / elapsed) / 8e12,         # per GPU, of 8 TB/s
            "finite": finite, "final_loss_mean": float(loss[-1, :, 0].mean().item()),
            "device_bytes": eng.device_bytes,
            "roofline": {"bound": "mfma", "kernel": kname, "achieved": achieved, "peak": peak,
                         "unit": "TFLOP/s", "frac": achieved / peak, "traffic": traffic, "traffic_note": traffic_note,
                         "avg_launch_us": ms * 1e3, "flops_per_launch": fl,
                         "us_per_time_step": ms * 1e3 / (T - 1) if swept else ms * 1e3,
                         "plan": plan, "per_layer_bwd_kernel": per_layer,
                         "fwd_kernel_avg_launch_us": ms_f * 1e3,
                         "fwd_kernel_achieved": fl_f / (ms_f * 1e-3) / 1e12,
                         "fused_fwd_kernel": None if fused is None else {
                             "kernel": "fused_fwd16_kernel" if plan.get("fused_rows") == 16 else ("fused_fwd2_kernel" if plan.get("fwd_per_cu") == 2 else "fused_fwd_kernel"),
                             "avg_launch_us": fused[0] * 1e3, "flops_per_launch": fused[1],
                             "achieved": fused[1] / (fused[0] * 1e-3) / 1e12, "frac": fused[1] / (fused[0] * 1e-3) / 1e12 / peak}},
        }
        if gather_ms is not None:
            out["final_cp_all_gather_ms"] = gather_ms
        if dumped is not None:
            out["dumped_outputs"] = dumped
        progress("kernel timing done; cpu baseline")
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(cfg, cfg["objective"], full=args.cpu_full)
        print(json.dumps(out), flush=True)
    if world > 1:
        barrier()   # rank 0 is still timing single kernels: nobody tears the communicator down under it
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
