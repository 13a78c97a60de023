#!/usr/bin/env python
"""bench.py -- training images/sec of the MNIST-32 CNN-VAE + GaussianPrior step on MI355X (BASELINE.json configs[1]).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One step = forward + backward + (RCCL all-reduce of the flat gradient buffer when N > 1) + Adam over one resident
synthetic batch of 1024 images per GPU (weak scaling), replayed as a hipGraph, plus the latent statistics update
(GaussianModel.update, the streaming fp64 covariance the Gaussian-W2 path consumes).  Inputs are already in HBM when
the timed region starts, and are the same from run to run.  Rank 0 prints ONE JSON line; `ms_per_step` is the wall
time of one of the K timed steps.

--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (dump_outputs), so that two builds can be
compared output for output.

A plain run sets up, warms up, times the K steps and prints the line.  --full adds these objects, each measured by
runs of its own after the timed steps (side_measurements):
  roofline      dominant kernel of the step, timed live with HIP events on the stream it runs on
  cpu_baseline  the CPU oracle (oracle/otvae_oracle.py, a port pinned to the reference by golden vectors) timed on the
                host cores of this box on a bounded sample of the same step (rank 0, N == 1 only)
  parity        relative error of the GPU step's losses vs that oracle on identical inputs (fp32, tolerance 1e-4)
and beside them the per-family table, the issue bounds of the attention stages, the eager and Lightning routes and, with
--workload sinkhorn, the OT solve alone.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PER_GPU_BATCH = 1024
# algorithmic traffic of one fused training step, MNIST test config (residual="add"), fp32
ALG_BYTES_PER_IMAGE_FWD_BWD = 1.72e6
ALG_FLOP_PER_IMAGE_FWD_BWD = 59e6
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
FP32_VALU_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: fp32 vector == fp32 MFMA peak


def host_threads() -> int:
    """Cores this process may really use (the GPU box gives a 16-core share of a much larger host)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:  # cgroup v2 quota
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:  # noqa: BLE001
        pass
    return max(1, min(n, 16))


def build_model(A, seed=0, workload="gaussian"):
    torch.manual_seed(seed)
    dec = A.CNN(128, 1, 1, 32, capacity=8, up_sample=True, residual="add")
    if workload == "sinkhorn":  # BASELINE configs[2]: deterministic encoder + entropic OT prior (eps 0.05, 50 iterations)
        enc = A.CNN(1, 128, 32, 1, capacity=8, down_sample=True, residual="add")
        return A.VAE(encoder=enc, decoder=dec, prior=A.SinkhornPrior(reg=0.05, max_iter=50, threshold=0.0))
    enc = A.CNN(1, 256, 32, 1, capacity=8, down_sample=True, residual="add")
    return A.VAE(encoder=enc, decoder=dec, prior=A.GaussianPrior(loss_coeff=0.1))


def time_sinkhorn(A, n=1024, d=128, iters=50, reps=20):
    """The OT term alone (configs[2] shapes): cost matrix + 50 log-domain Sinkhorn iterations + sum(C * pi), HIP events."""
    g = torch.Generator().manual_seed(7)
    z = torch.randn(n, d, generator=g).cuda()
    y = torch.randn(n, d, generator=g).cuda()
    prior = A.SinkhornPrior(reg=0.05, max_iter=iters, threshold=0.0)

    def solve():  # otvae_sinkhorn_prior_fwd: cost tiles + maxima, init, the solve, read-out
        with torch.no_grad():
            return prior(z, step=0, prior_samples=y)[1][0]

    for _ in range(3):
        solve()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        cost = solve()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    # per iteration: one log-sum-exp pass over the rows of Cr and one over its transposed copy
    return {"n": n, "m": n, "iterations": iters, "ms_per_solve": round(ms, 4), "us_per_iteration": round(ms * 1e3 / iters, 3),
            "exp_per_s": round(2.0 * n * n * iters / (ms * 1e-3), 1),
            "l2_resident_read_gbytes_per_s": round(2.0 * n * n * 4 * iters / (ms * 1e-3) / 1e9, 1), "ot_cost": float(cost)}


def time_eager_route(A, workload, pool, steps=20, warmup=5):
    """The same step WITHOUT the hipGraph: every operator launched from Python through torch.ops.otvae / the C ABI (what a
    Lightning loop that calls ``training_step`` + ``loss.backward()`` + the fused Adam pays per step).  Host-bound."""
    model = build_model(A, seed=1, workload=workload).cuda().train()
    tr = A.HipTrainer(model, batch_shape=tuple(pool[0].shape), use_graph=False, data_parallel=False)
    for i in range(warmup):
        tr.step(pool[i % len(pool)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        tr.step(pool[i % len(pool)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def time_lightning_route(A, workload, pool, steps=30, warmup=8):
    """The reference's own loop shape -- ``training_step`` -> ``loss.backward()`` -> a stock ``torch.optim.Adam`` (model/base.py:
    122-129, model/vae.py:148-156) -- with ``model.enable_graphed_step()``: nelbo is one autograd node that replays a captured
    forward graph and a captured backward graph (engine/graphed.py); the optimizer is torch's, untouched."""
    model = build_model(A, seed=1, workload=workload).cuda().train().enable_graphed_step()
    opt = torch.optim.Adam(model.optim_parameters(), lr=1e-3, betas=(0.9, 0.999))
    labels = torch.zeros(pool[0].shape[0], dtype=torch.long, device="cuda")

    def step(i):
        opt.zero_grad()
        out = model.training_step((pool[i % len(pool)], labels), i)
        out["loss"].backward()
        opt.step()

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def cpu_baseline(A, batch=250, steps=5, warmup=2):
    """The oracle on the host cores: same step definition (fwd + bwd + Adam), bounded sample."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import otvae_oracle as O
    from detfill import mnist_like, normal
    torch.set_num_threads(host_threads())
    model = build_model(A)
    ea = O.cnn_arch(1, 256, 32, 1, capacity=8, down_sample=True, residual="add")
    da = O.cnn_arch(128, 1, 1, 32, capacity=8, up_sample=True, residual="add")
    enc = {k: v.detach().clone().contiguous() for k, v in model.encoder.state_dict().items()}
    dec = {k: v.detach().clone().contiguous() for k, v in model.decoder.state_dict().items()}
    leaves = [v.requires_grad_(True) for d in (enc, dec) for k, v in d.items()
              if v.is_floating_point() and "running" not in k]
    m = [torch.zeros_like(v) for v in leaves]
    s = [torch.zeros_like(v) for v in leaves]
    x, eps = mnist_like(batch, 42), normal((batch, 128, 1, 1), 43)
    t0 = None
    for it in range(warmup + steps):
        if it == warmup:
            t0 = time.perf_counter()
        for v in leaves:
            v.grad = None
        r = O.vae_nelbo(x, eps, enc, dec, ea, da, loss_coeff=0.1)
        r["loss"].backward()
        with torch.no_grad():
            O.adam_step(leaves, [v.grad for v in leaves], m, s, step=it + 1)
    dt = time.perf_counter() - t0
    return {"value": round(batch * steps / dt, 2), "unit": "images/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{steps} steps (fwd+bwd+Adam) at batch {batch} after {warmup} warm-up, fp32, torch "
                      f"{torch.__version__} CPU ops, oracle/otvae_oracle.py"}


def parity_check(A, batch=PER_GPU_BATCH):
    """GPU step vs oracle on identical weights / batch / eps AT THE BENCHED BATCH: relative error of [total, recon, prior(KL)],
    of the reconstructions, and of the Sinkhorn OT loss (1024 x 1024 plan, eps 0.05, 50 iterations)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import otvae_oracle as O
    from detfill import mnist_like, normal
    model = build_model(A)
    ea = O.cnn_arch(1, 256, 32, 1, capacity=8, down_sample=True, residual="add")
    da = O.cnn_arch(128, 1, 1, 32, capacity=8, up_sample=True, residual="add")
    enc = {k: v.detach().clone().contiguous() for k, v in model.encoder.state_dict().items()}
    dec = {k: v.detach().clone().contiguous() for k, v in model.decoder.state_dict().items()}
    x, eps = mnist_like(batch, 5), normal((batch, 128, 1, 1), 6)
    with torch.no_grad():
        r = O.vae_nelbo(x, eps, enc, dec, ea, da, loss_coeff=0.1)
    want = torch.stack([r["loss"], r["recon"], r["prior"]])
    model = model.cuda().train()
    with torch.no_grad():
        loss, logs, art = model.nelbo({"samples": x.cuda(), "target": x.cuda(), "kwargs": {"eps": eps.cuda()}}, 0)
    got = model._last_out3.cpu()
    rel = ((got - want).abs() / want.abs()).tolist()
    rec = ((art["preds"].cpu() - r["preds"]).abs().max() / r["preds"].abs().max()).item()
    z, p = normal((batch, 128), 11), normal((batch, 128), 12)
    ot_cpu = O.sinkhorn_ot_loss(z, p, reg=0.05, max_iter=50, threshold=0.0).item()
    with torch.no_grad():
        ot_gpu = A.SinkhornPrior(reg=0.05, max_iter=50, threshold=0.0)(z.cuda(), step=0, prior_samples=p.cuda())[1][0].item()
    return {"loss_rel_err": max(rel), "reconstruction_rel_err": rec, "ot_loss_rel_err": abs(ot_gpu - ot_cpu) / abs(ot_cpu),
            "tolerance": 1e-4, "batch": batch}


# Issue bounds of the single-channel attention backward, in (query, key) pairs per second over 1024 SIMDs x 2.4 GHz x 64 lanes:
#   OWN ISA  -- the instruction stream the kernel actually has: 36 issue cycles per 2 pairs (2 v_exp_f32 at 8 + 5 packed FMA/MUL at 4).
#               Says how close the kernel runs to ITS OWN instructions' nominal rate (rounds 1-3 reported only this one).
#   ALGORITHM -- the fewest vector operations ANY kernel needs per pair, at the cycle table's best rates (v_exp_f32: 8 issue cycles per
#               wave-instruction; v_pk_fma_f32: 4 cycles for two FMAs).  One head channel: forward = score 1 FMA + 1 exp + value 1 FMA +
#               row sum 1 = 1 exp + 3 FMA (VERDICT r3 #2d) -> 8 + 3 * 2 = 14 cycles.  Backward: the textbook pass (recompute p, dP = go v,
#               dS = p (dP - delta), dv += p go, dk += dS q, dq += dS k) is 1 exp + 7 FMA = 22 cycles, but dq needs no pair work at all
#               when the forward keeps the per-query moments sum_s p (v - out) k (head widths <= 2; csrc/attention.hip), which leaves
#               score 1 + exp + dP 1 + dS 1 + dv 1 + dk 1 = 1 exp + 5 FMA -> 8 + 5 * 2 = 18 cycles: the fewest known, and what this
#               kernel's stream has, so for the backward the two bounds coincide and `frac` says how far the kernel is from
#               issuing them at the table's rates.
ISSUE_BOUND_TPAIRS = 1024 * 2.4e9 * 64 / 18.0 / 1e12
ALG_ISSUE_CYCLES_PER_PAIR_C1 = {"fwd": 8 + 3 * 2, "bwd": 8 + 5 * 2}
ALG_ISSUE_BOUND_TPAIRS = {k: 1024 * 2.4e9 * 64 / v / 1e12 for k, v in ALG_ISSUE_CYCLES_PER_PAIR_C1.items()}


def time_dominant_kernel(A, trainer, iters=30):
    """Average duration of the longest single launch of the step (profiles/: the AttentionBlock backward of the decoder's last
    block, T=1024 tokens, 1 head, 1 channel), launched back to back through the C ABI between two HIP events on the
    stream the kernel runs on."""
    from ot_vae_lightning_amd import functional as HF
    from ot_vae_lightning_amd import _lib as L
    lib = L.load()
    n, t, heads, c = PER_GPU_BATCH, 1024, 1, 1
    qkv = HF.as_nhwc(torch.randn(n, 3, 32, 32, device="cuda"))
    out = HF.qkv_attention(qkv, 1)                       # forward once: out and the log-sum-exp it saved
    lse = torch.empty((n, heads, t), device="cuda")
    aux = torch.empty((n, heads, t, c * c), device="cuda")  # key moments: the training path's backward uses them
    L.check(lib.otvae_attn_fwd(L.ptr(qkv), n, t, heads, c, L.ptr(out), L.ptr(lse), L.ptr(aux), L.stream()), "otvae_attn_fwd")
    g = torch.randn_like(out)
    gqkv = torch.empty_like(qkv)

    # since the end of round 3 the step runs this attention inside the one-launch AttentionBlock backward (attn_stage_bwd_kernel<1,4,true>:
    # + the two 1x1 kernels' data gradients and the BatchNorm sums): that launch is what is timed
    import ctypes as C
    x, gv = torch.randn(n, t, 1, device="cuda"), torch.empty(n, t, 1, device="cuda")
    wq, wp = torch.randn(1, 3, device="cuda"), torch.randn(1, 1, device="cuda")
    one, zero = torch.ones(4, device="cuda"), torch.zeros(4, device="cuda")
    rows_b = C.c_int(0)
    L.check(lib.otvae_attn_stage_bwd_plan(n, t, heads, c, C.byref(rows_b)), "otvae_attn_stage_bwd_plan")
    part_b = torch.empty(rows_b.value, 2, 1, device="cuda", dtype=torch.float64)

    def launch():
        L.check(lib.otvae_attn_stage_bwd(L.ptr(g), L.ptr(wp), L.ptr(wq), L.ptr(x), L.ptr(zero), L.ptr(one), L.ptr(one), L.ptr(zero), None,
                                         L.ptr(out), L.ptr(lse), L.ptr(aux), n, t, heads, c, 1.0 / c, L.ptr(gqkv), L.ptr(gv), L.ptr(part_b),
                                         L.stream()), "otvae_attn_stage_bwd")

    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    # `iters` launches captured into one hipGraph: the events then bracket kernel time only (no host launch gaps)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):  # the RCCL watchdog may poll from its own thread
        for _ in range(iters):
            launch()
    for _ in range(10):     # the set-up above left the GPU idle: bring the clocks back to the training loop's state
        graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / (4 * iters)
    # algorithmic work of this launch: reads gy, x, out, lse, the forward's key moments (1 float each for one channel), writes gqkv (3)
    # and gv (1) -> 9 floats per token; arithmetic: T*T pair evaluations per image (one dK/dV pass; dQ comes from the moments)
    tokens = n * 1024
    alg_bytes = tokens * 9 * 4
    pair_evals = n * 1024 * 1024
    # the same stage's FORWARD launch (attn_stage_fwd_kernel<1,4,true>), for the 1 exp + 3 FMA bound
    rows_f = C.c_int(0)
    L.check(lib.otvae_attn_stage_plan(n, t, heads, c, 1, C.byref(rows_f)), "otvae_attn_stage_plan")
    part_f = torch.empty(rows_f.value, 2, 1, device="cuda", dtype=torch.float64)
    y_f, res_f = torch.empty(n, t, 1, device="cuda"), torch.randn(n, t, 1, device="cuda")

    def launch_f():
        L.check(lib.otvae_attn_stage_fwd(L.ptr(x), L.ptr(one), L.ptr(zero), L.ptr(wq), L.ptr(wp), L.ptr(res_f), n, t, heads, c, 1.0 / c, None,
                                         L.ptr(out), L.ptr(lse), L.ptr(aux), L.ptr(y_f), L.ptr(part_f), L.stream()), "otvae_attn_stage_fwd")

    for _ in range(3):
        launch_f()
    torch.cuda.synchronize()
    graph_f = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_f, capture_error_mode="thread_local"):
        for _ in range(iters):
            launch_f()
    for _ in range(5):
        graph_f.replay()
    torch.cuda.synchronize()
    f0, f1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    f0.record()
    for _ in range(4):
        graph_f.replay()
    f1.record()
    torch.cuda.synchronize()
    ms_f = f0.elapsed_time(f1) / (4 * iters)
    return {"kernel": "attn_stage_bwd_kernel<1,4,true> (T=1024,H=1,C=1)", "ms": ms, "alg_bytes": alg_bytes, "pair_evals": pair_evals,
            "pmc_traffic_bytes": pmc_traffic("attn_stage_bwd_kernel<1, 4, true>"), "ms_fwd": ms_f}


# Issue model of the head-width-2 attention kernels (T = 256, 4 heads: encoder block 0 / decoder block 3), from the ISA of the
# inner loops (hipcc -S): per 16 (query, key) pairs of a lane
#   forward  (moments for dq ride along): 80 v_pk_fma_f32 + 8 v_pk_add_f32 + 8 v_mov_b32 + 16 v_exp_f32
#   backward (dk, dv; dq from the moments): 64 v_pk_fma_f32 + 8 v_pk_mul_f32 + 4 v_mov_b32 + 16 v_exp_f32
# at the cycle table's issue costs (MI355X_MICROARCH.md: 4 cycles per vector instruction, 8 per transcendental), 1024 SIMDs,
# 2.4 GHz, 64 lanes.  (Measured at 4 waves per SIMD a v_pk_fma_f32 costs 5.2-5.8, which is most of the gap.)
ATTN_C2_CYCLES_PER_16_PAIRS = {"fwd": (80 + 8 + 8) * 4 + 16 * 8, "bwd": (64 + 8 + 4) * 4 + 16 * 8}


def time_attention_c2(A, iters=20):
    """The head-width-2 attention of the 16x16 blocks at the benchmark's shape through the C ABI, 20 launches per hipGraph, HIP events on
    the launch stream; against the issue model above.  Since the end of round 3 the step runs it inside the one-launch AttentionBlock
    kernels (attn_stage_fwd/bwd_kernel<2,4,true>: BatchNorm affine + 1x1 qkv + attention + 1x1 projection + skip; backward likewise):
    those are timed and priced here -- the model still counts the (query, key) pair work only, so the stage's other phases show up as a
    lower fraction -- with the bare attention kernels (otvae_attn_fwd / _bwd) beside them as ``attention_only_ms``."""
    import ctypes as C
    from ot_vae_lightning_amd import _lib as L
    lib = L.load()
    n, t, heads, c = PER_GPU_BATCH, 256, 4, 2
    hc = heads * c
    dev = "cuda"
    qkv = torch.randn(n, t, 3 * hc, device=dev)
    out = torch.empty(n, t, hc, device=dev)
    lse = torch.empty(n, heads, t, device=dev)
    aux = torch.empty(n, heads, t, c * c, device=dev)
    g, gq = torch.randn_like(out), torch.empty_like(qkv)
    x, res, y, gv = torch.randn(n, t, hc, device=dev), torch.randn(n, t, hc, device=dev), torch.empty(n, t, hc, device=dev), torch.empty(n, t, hc, device=dev)
    wq, wp = torch.randn(hc, 3 * hc, device=dev) * 0.3, torch.randn(hc, hc, device=dev) * 0.3
    scale, shift = torch.rand(hc, device=dev) + 0.5, torch.randn(hc, device=dev) * 0.1
    mean, invstd = torch.randn(hc, device=dev) * 0.1, torch.rand(hc, device=dev) + 0.5
    rows, rows_b = C.c_int(0), C.c_int(0)
    L.check(lib.otvae_attn_stage_plan(n, t, heads, c, 1, C.byref(rows)), "plan")
    L.check(lib.otvae_attn_stage_bwd_plan(n, t, heads, c, C.byref(rows_b)), "plan")
    part = torch.empty(rows.value, 2, hc, device=dev, dtype=torch.float64)
    part_b = torch.empty(rows_b.value, 2, hc, device=dev, dtype=torch.float64)
    fns = {"fwd": lambda: L.check(lib.otvae_attn_stage_fwd(L.ptr(x), L.ptr(scale), L.ptr(shift), L.ptr(wq), L.ptr(wp), L.ptr(res), n, t, heads, c,
                                                           1.0 / c, None, L.ptr(out), L.ptr(lse), L.ptr(aux), L.ptr(y), L.ptr(part), L.stream()), "f"),
           "bwd": lambda: L.check(lib.otvae_attn_stage_bwd(L.ptr(g), L.ptr(wp), L.ptr(wq), L.ptr(x), L.ptr(mean), L.ptr(invstd), L.ptr(scale),
                                                           L.ptr(shift), None, L.ptr(out), L.ptr(lse), L.ptr(aux), n, t, heads, c, 1.0 / c,
                                                           L.ptr(gq), L.ptr(gv), L.ptr(part_b), L.stream()), "b"),
           "fwd_plain": lambda: L.check(lib.otvae_attn_fwd(L.ptr(qkv), n, t, heads, c, L.ptr(out), L.ptr(lse), L.ptr(aux), L.stream()), "f"),
           "bwd_plain": lambda: L.check(lib.otvae_attn_bwd(L.ptr(qkv), L.ptr(out), L.ptr(lse), L.ptr(g), L.ptr(aux), n, t, heads, c, L.ptr(gq),
                                                           L.stream()), "b")}
    times = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            for _ in range(iters):
                fn()
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        times[name] = e0.elapsed_time(e1) / (4 * iters)
    res_ = {}
    pairs = n * heads * t * t
    for name in ("fwd", "bwd"):
        ms = times[name]
        peak = 1024 * 2.4e9 * 64 * 16 / ATTN_C2_CYCLES_PER_16_PAIRS[name] / 1e12
        tp = pairs / ms / 1e9
        res_[name] = {"kernel": f"attn_stage_{name}_kernel<2,4,true> (T=256,H=4,C=2, width 8)", "avg_launch_ms": round(ms, 5),
                      "attention_only_ms": round(times[name + "_plain"], 5), "launches_per_step": 2, "achieved": round(tp, 3),
                      "peak": round(peak, 3), "unit": "T (query,key) pairs/s", "frac": round(tp / peak, 4)}
    return res_


FP32_MFMA_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: dense fp32 MFMA peak == fp32 vector peak
GEOM_FIELDS = ("N", "Hs", "Ws", "Cs", "up", "Ho", "Wo", "Cn", "KH", "KW", "stride", "pad")


def _axis_pairs(n_out, k, stride, pad, n_src_up):
    """(output position, tap) pairs of one axis whose input coordinate o * stride + t - pad falls inside the (up-sampled) source,
    and the taps that are in range for at least one output position (the kernel's live-tap rule, csrc/conv.hip:179-211)"""
    pairs, live = 0, 0
    for t in range(k):
        cnt = sum(1 for o in range(n_out) if 0 <= o * stride + t - pad < n_src_up)
        pairs += cnt
        live += 1 if cnt else 0
    return pairs, live


def _job_flops(job):
    """Multiply-add work of one conv job under three conventions, all as 2 x MACs:
      live     -- MACs whose input operand exists (padding contributes nothing): the ALGORITHM's work, what `roofline.frac` prices;
      executed -- MACs the kernel issues: every output position x every tap that is in range for SOME position (dead taps are dropped,
                  csrc/conv.hip:179-211; a padded position inside a live tap is multiplied by a zero-filled operand);
      padded   -- 2 * y * KH * KW * Cs, the convention of SURVEY section 8(d) and of rounds 1-3 (counts work nobody does: a 3x3 kernel
                  on a 1x1 map has one live tap of nine).
    The same three counts hold for the data- and the weight-gradient of the layer (each forward MAC has one counterpart in each)."""
    g = dict(zip(GEOM_FIELDS, job["geom"]))
    hu, wu = g["Hs"] * g["up"], g["Ws"] * g["up"]
    py, ly = _axis_pairs(g["Ho"], g["KH"], g["stride"], g["pad"], hu)
    px, lx = _axis_pairs(g["Wo"], g["KW"], g["stride"], g["pad"], wu)
    per_pos = 2 * g["N"] * g["Cs"] * g["Cn"]
    return {"live": per_pos * py * px, "executed": per_pos * g["Ho"] * g["Wo"] * ly * lx,
            "padded": per_pos * g["Ho"] * g["Wo"] * g["KH"] * g["KW"]}


def _job_algorithmic(job):
    """(bytes, flops) one conv job must move / compute at least (fp32; every operand read once, every result written once;
    the weight-gradient's split-K partials and the BatchNorm partial sums are NOT algorithmic traffic).  flops = the LIVE count of
    ``_job_flops`` (round 3 returned the padded count: VERDICT r3 weak #4)."""
    g = dict(zip(GEOM_FIELDS, job["geom"]))
    x = g["N"] * g["Hs"] * g["Ws"] * g["Cs"]
    y = g["N"] * g["Ho"] * g["Wo"] * g["Cn"]
    w = g["KH"] * g["KW"] * g["Cs"] * g["Cn"]
    flops = _job_flops(job)["live"]
    if job["kind"] == 0:      # forward: x, w -> y
        return 4 * (x + w + y), flops
    if job["kind"] == 1:      # data gradient: gy, w (, x for the ReLU mask / BatchNorm sums) -> gv
        return 4 * (y + w + x + (x if (job["relu"] or job["bn_sums"]) else 0)), flops
    return 4 * (x + y + w), flops   # weight gradient: x, gy -> gw


def time_largest_aggregate_kernel(A, workload, iters=10):
    """The MFMA kernel with the largest aggregate share of the step (profiles/r02_final_replay_kernel_stats.csv:
    ``conv_jobs_kernel<true>``, the packed launches of a ConvBlock's two branches -- forward and data gradient; 9 launches = 5.7 %
    of the step now that the weight-gradient jobs run on their own stream, 24 launches = 16 % before): the step's own
    otvae_conv_multi calls that end in that kernel are recorded from one step issued as the captured step issues it
    (functional.JOB_TRACE + otvae_conv_multi_last), re-issued on tensors of the same shapes through the C ABI into one hipGraph,
    and timed with HIP events on the launch stream."""
    import ctypes as C
    from ot_vae_lightning_amd import functional as HF
    from ot_vae_lightning_amd import _lib as L
    from ot_vae_lightning_amd.utils.synthetic import mnist_like
    lib = L.load()
    model = build_model(A, seed=2, workload=workload).cuda().train()
    tr = A.HipTrainer(model, batch_shape=(PER_GPU_BATCH, 1, 32, 32), use_graph=False, data_parallel=False)  # rank-local
    x = mnist_like(PER_GPU_BATCH, seed=77).cuda()
    tr.step(x)
    side, HF.WGRAD_SIDE_STREAM = HF.WGRAD_SIDE_STREAM, 2 if HF.WGRAD_SIDE_STREAM else 0  # the launches of the CAPTURED step
    HF.JOB_TRACE = []
    tr.step(x)
    torch.cuda.synchronize()
    trace, HF.JOB_TRACE = HF.JOB_TRACE, None
    HF.WGRAD_SIDE_STREAM = side
    calls = [c for c in trace if c["uniform_tap"] == 1 and c["packed_mask"]]
    if not calls:
        return None
    dev = "cuda"
    keep, launches = [], []
    tot_bytes = tot_flops = tot_exec = tot_padded = 0
    for c in calls:
        jobs = [j for i, j in enumerate(c["jobs"]) if c["packed_mask"] >> i & 1]
        arr = (L.ConvJob * len(jobs))()
        for jb, j in zip(arr, jobs):
            g = L.ConvGeom(*j["geom"])
            gd = dict(zip(GEOM_FIELDS, j["geom"]))
            t_x = torch.randn(gd["N"], gd["Hs"], gd["Ws"], gd["Cs"], device=dev)
            t_y = torch.randn(gd["N"], gd["Ho"], gd["Wo"], gd["Cn"], device=dev)
            t_w = torch.randn(gd["KH"] * gd["KW"] * gd["Cs"] * gd["Cn"], device=dev) * 0.05
            vec = lambda: torch.rand(gd["Cs"], device=dev) + 0.5  # noqa: E731
            jb.kind, jb.relu, jb.has_bias, jb.geom = j["kind"], j["relu"], j["has_bias"], g
            held = [t_x, t_y, t_w]
            if j["has_norm"]:
                sc, sh = vec(), vec()
                jb.scale, jb.shift = L.ptr(sc), L.ptr(sh)
                held += [sc, sh]
            if j["kind"] == L.JOB_FWD:
                jb.x, jb.w, jb.y = L.ptr(t_x), L.ptr(t_w), L.ptr(t_y)
            elif j["kind"] == L.JOB_BWD_DATA:
                gv = torch.empty_like(t_x)
                jb.gy, jb.w, jb.x, jb.gv = L.ptr(t_y), L.ptr(t_w), L.ptr(t_x), L.ptr(gv)
                held.append(gv)
                if j["bn_sums"]:
                    p_d, cp = C.c_int(0), C.c_int(0)
                    L.check(lib.otvae_conv_bwd_data_ws(C.byref(g), C.byref(p_d), C.byref(cp)), "otvae_conv_bwd_data_ws")
                    mean, invstd = vec(), vec()
                    part = torch.empty((p_d.value, 2, cp.value), device=dev, dtype=torch.float64)
                    jb.mean, jb.invstd, jb.bn_partial = L.ptr(mean), L.ptr(invstd), L.ptr(part)
                    held += [mean, invstd, part]
            else:
                p_w = C.c_int(0)
                L.check(lib.otvae_conv_bwd_weight_ws(C.byref(g), j["has_bias"], C.byref(p_w)), "otvae_conv_bwd_weight_ws")
                kk = gd["KH"] * gd["KW"] * gd["Cs"] + (1 if j["has_bias"] else 0)
                wpart = torch.empty((p_w.value, kk, gd["Cn"]), device=dev)
                gw, gb = torch.empty_like(t_w), torch.empty(gd["Cn"], device=dev)
                jb.x, jb.gy, jb.wpartial, jb.gw, jb.gb = L.ptr(t_x), L.ptr(t_y), L.ptr(wpart), L.ptr(gw), L.ptr(gb)
                jb.defer_reduce = L.DEFER_SPARSE  # as in the step: the partials are reduced by the step's batched reduction
                held += [wpart, gw, gb]
            keep.append(held)
            by, fl = _job_algorithmic(j)
            fls = _job_flops(j)
            tot_bytes += by
            tot_flops += fl
            tot_exec += fls["executed"]
            tot_padded += fls["padded"]
        launches.append((arr, len(jobs)))
    mask, ut = C.c_uint32(0), C.c_int(0)

    def issue(verify=False):
        for arr, n in launches:
            L.check(lib.otvae_conv_multi(n, arr, L.stream()), "otvae_conv_multi")
            if verify:  # every re-issued call must end in exactly the kernel being measured
                L.check(lib.otvae_conv_multi_last(C.byref(mask), C.byref(ut)), "otvae_conv_multi_last")
                assert ut.value == 1 and bin(mask.value).count("1") == n, (ut.value, mask.value, n)

    issue(verify=True)
    issue()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        for _ in range(iters):
            issue()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(4):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    n_launch = len(launches)
    ms = e0.elapsed_time(e1) / (4 * iters * n_launch)
    return {"kernel": "conv_jobs_kernel<true> (the packed forward / data-gradient jobs of a ConvBlock's two branches, implicit GEMM, fp32 MFMA 16x16x4)",
            "launches_per_step": n_launch, "ms": ms, "alg_bytes": tot_bytes / n_launch, "alg_flops": tot_flops / n_launch,
            "executed_flops": tot_exec / n_launch, "padded_flops": tot_padded / n_launch,
            "pmc_traffic_bytes": pmc_traffic("conv_jobs_kernel<true>"), "trace": trace}


ROUND_TAG = "r04"   # profiles/<ROUND_TAG>_*: the committed summaries this line's `traffic` and `families` read

# kernel families of the step (VERDICT r3 #2c: no kernel holds more than 6 % of it, so the step's roofline is decomposed by family)
FAMILIES = (("conv fwd+dgrad", ("conv_jobs_kernel", "conv_gemm_kernel", "conv_tile_kernel", "conv_small_fwd", "conv_small_dgrad")),
            ("wgrad", ("conv_wgrad_kernel", "conv_wtile_kernel", "conv_small_wgrad", "wgrad_reduce")),
            ("attention stages", ("attn_",)),
            ("BatchNorm launches", ("bn_",)),
            ("other", ()))
# (T, heads, head width) of the ten AttentionBlocks of the MNIST network, encoder then decoder
MNIST_ATTENTION = ((256, 4, 2), (64, 4, 4), (16, 8, 4), (4, 8, 8), (1, 16, 16), (4, 8, 8), (16, 8, 4), (64, 4, 4), (256, 4, 2), (1024, 1, 1))


def _family_of(kernel_name):
    k = kernel_name.replace("void ", "")
    for fam, pats in FAMILIES:
        if any(k.startswith(p_) for p_ in pats):
            return fam
    return "other"


def family_table(trace, trainer, world):
    """Per kernel family of ONE training step: launches, ms, algorithmic bytes and FLOPs (live / padded), PMC bytes -- the
    decomposition of ``step_roofline``.  Algorithmic work: convolutions from the step's own recorded jobs (``functional.JOB_TRACE``:
    every otvae_conv_multi call), the AttentionBlocks analytically (a fused stage reads x and the residual and writes y; its
    1 x 1 kernels' FLOPs are counted here because they run inside the stage kernels), BatchNorm launches hold NO algorithmic work
    (their arithmetic belongs to the neighbouring layers' passes: they are pure overhead), `other` = Adam (7 passes over the
    parameters), the loss (pred + target once), the transposed weight copies.  Launches / ms / PMC bytes come from the committed
    summaries of THIS round (profiles/<round>_final_replay_kernel_stats.csv, _pmc_per_kernel.csv: same bench command under rocprofv3)
    and are null when those were collected from other kernel sources than the tree holds."""
    import csv
    B = PER_GPU_BATCH
    alg = {fam: [0.0, 0.0, 0.0] for fam, _ in FAMILIES}   # bytes, live flops, padded flops
    for c in trace:
        for j in c["jobs"]:
            by, fl = _job_algorithmic(j)
            fam = "wgrad" if j["kind"] == 2 else "conv fwd+dgrad"
            alg[fam][0] += by
            alg[fam][1] += fl
            alg[fam][2] += _job_flops(j)["padded"]
    for t, h, c_ in MNIST_ATTENTION:
        w = h * c_
        fused = w <= 32 and t > 1
        fl = 4 * t * t * w + (2 * t * w * 3 * w + 2 * t * w * w if fused else 0)
        by = 4 * t * w * (3 if fused else 4)
        alg["attention stages"][0] += 3 * B * by      # forward + backward = 3 x forward
        alg["attention stages"][1] += 3 * B * fl
        alg["attention stages"][2] += 3 * B * fl
    n_par = trainer.pflat.numel()
    alg["other"][0] += 7 * 4 * n_par + 2 * 4 * B * 32 * 32 + 2 * 4 * trainer.wdflat.numel()
    alg["other"][1] += 12 * n_par
    alg["other"][2] += 12 * n_par
    meas = {fam: [None, None, None] for fam, _ in FAMILIES}   # launches, ms, pmc bytes
    try:
        lines = open(os.path.join(ROOT, "profiles", f"{ROUND_TAG}_final_replay_kernel_stats.csv")).read().splitlines()
        fresh = any(l.startswith("# csrc_sha256=") and l.split("=", 1)[1].strip() == csrc_digest() for l in lines[:3])
        calls = {}
        if fresh:
            for fam in meas:
                meas[fam][:2] = [0.0, 0.0]
            for row in csv.DictReader(l for l in lines if not l.startswith("#")):
                fam = _family_of(row["kernel"])
                meas[fam][0] += float(row["calls_per_step"])
                meas[fam][1] += float(row["ms_per_step"])
                calls[row["kernel"]] = float(row["calls_per_step"])
            plines = open(os.path.join(ROOT, "profiles", f"{ROUND_TAG}_pmc_per_kernel.csv")).read().splitlines()
            if plines and plines[0].startswith("# csrc_sha256=") and plines[0].split("=", 1)[1].strip() == csrc_digest():
                for fam in meas:
                    meas[fam][2] = 0.0
                for row in csv.DictReader(plines[1:]):
                    if row["kernel"] in calls:
                        meas[_family_of(row["kernel"])][2] += float(row["hbm_MB_per_launch"]) * 1048576.0 * calls[row["kernel"]]
    except OSError:
        pass
    rows = []
    for fam, _ in FAMILIES:
        by, fl, flp = alg[fam]
        n, ms, pmc_b = meas[fam]
        rows.append({"family": fam, "launches": n, "ms_per_step": None if ms is None else round(ms, 4),
                     "alg_mbytes": round(by / 1e6, 2), "alg_gflops_live": round(fl / 1e9, 3), "alg_gflops_padded": round(flp / 1e9, 3),
                     "pmc_mbytes": None if pmc_b is None else round(pmc_b / 1e6, 2),
                     "frac_of_hbm_peak": None if not ms else round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                     "frac_of_fp32_peak": None if not ms else round(fl / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4)})
    tot_b, tot_f = sum(a[0] for a in alg.values()), sum(a[1] for a in alg.values())
    return {"rows": rows, "sum_alg_gbytes": round(tot_b / 1e9, 3), "sum_alg_gflops_live": round(tot_f / 1e9, 2),
            "sum_alg_gflops_padded": round(sum(a[2] for a in alg.values()) / 1e9, 2),
            "note": "ms of the two streams add up to more than the step (the weight-gradient family runs beside the chain)"}


def csrc_digest():
    """sha256 over the kernel sources (the same function as tools/summarize_profiles.py:csrc_digest)"""
    import hashlib
    root = os.path.join(ROOT, "ot_vae_lightning_amd", "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(root)):
        if f.endswith((".hip", ".h", ".cpp")):
            h.update(f.encode())
            h.update(open(os.path.join(root, f), "rb").read())
    return h.hexdigest()


def pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` from the committed PMC summary of THIS round (profiles/<round>_pmc_per_kernel.csv, written by
    tools/summarize_profiles.py --pmc from separate rocprofv3 --pmc passes of this same command: FETCH_SIZE with the x2 gfx950
    correction + WRITE_SIZE, KiB -> bytes, as MI355X_MICROARCH.md prescribes).  None -- not a stale number -- when the summary is
    missing or was collected from other kernel sources than the tree holds now (its first line carries their digest)."""
    import csv
    path = os.path.join(ROOT, "profiles", f"{ROUND_TAG}_pmc_per_kernel.csv")
    try:
        lines = open(path).read().splitlines()
    except OSError:
        return None
    if not lines or not lines[0].startswith("# csrc_sha256=") or lines[0].split("=", 1)[1].strip() != csrc_digest():
        return None
    for row in csv.reader(lines[1:]):
        if row and row[0].strip().endswith(kernel):
            return (2.0 * float(row[2]) + float(row[4])) * 1024.0
    return None


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, trainer, latent_model, loss):
    """What the last timed step handed its caller, one ``<name>.npy`` per array in float32 (float64 where the step keeps
    float64): the loss vector [total, recon, prior], the latents, the flat parameters after Adam, the flat gradient Adam read,
    the model's floating-point buffers (BatchNorm running statistics) and the latent Gaussian statistics.  An array that would
    take the files past 64 MB in all is written as a fixed, seeded sample of its elements."""
    import numpy as np
    arrays = {"loss": loss, "latents": trainer.latents, "params": trainer.pflat, "grads": trainer.gflat,
              "model_buffers": [b for b in trainer.model.buffers() if b.is_floating_point()],
              "latent_stats": [b for b in latent_model.buffers() if b.is_floating_point()]}
    arrays = {k: v for k, v in arrays.items() if v is not None and not (isinstance(v, list) and not v)}
    os.makedirs(out_dir, exist_ok=True)
    budget = DUMP_LIMIT_BYTES
    for i, (name, t) in enumerate(arrays.items()):
        if isinstance(t, list):
            dt = torch.float64 if any(b.dtype == torch.float64 for b in t) else torch.float32
            t = torch.cat([b.detach().reshape(-1).to(dt) for b in t])
        a = t.detach().cpu()
        a = (a.double() if a.dtype == torch.float64 else a.float()).numpy()
        keep = min(a.size, budget // (len(arrays) - i) // a.itemsize)  # an equal share of what is left
        if keep < a.size:
            idx = np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        budget -= a.nbytes


def side_measurements(A, args, trainer, pool, world):
    """What ``--full`` adds to the line, each from runs of its own after the timed steps: the roofline of the kernel with the
    largest aggregate share of the step and the per-family table, the longest launch against HBM and the issue bounds, the
    head-width-2 attention stages, the Sinkhorn solve alone (``--workload sinkhorn``), and on one rank the eager and Lightning
    routes, parity with the CPU oracle and the CPU baseline."""
    line = {}
    agg = time_largest_aggregate_kernel(A, args.workload)
    try:
        longest, longest_err = time_dominant_kernel(A, trainer), None
    except Exception as e:  # noqa: BLE001  (an auxiliary measurement must not take the headline line with it)
        longest, longest_err = None, repr(e)
    if agg is not None:
        gbs = agg["alg_bytes"] / (agg["ms"] * 1e-3) / 1e9
        tfl = agg["alg_flops"] / (agg["ms"] * 1e-3) / 1e12
        tfl_exec = agg["executed_flops"] / (agg["ms"] * 1e-3) / 1e12
        tfl_pad = agg["padded_flops"] / (agg["ms"] * 1e-3) / 1e12
        # The kernel with the largest aggregate share of the step.  Its launches average ~10 MB and ~0.7 GFLOP of
        # algorithmic work: ~67 FLOP/B against a ridge at 157.3 TFLOP/s / 8 TB/s = 19.7 FLOP/B, so the fp32 MFMA roof is the
        # one that bounds it (at that peak a launch would take ~4.5 us, at the HBM peak ~1.3 us); the HBM figures ride along.
        t_mfma, t_hbm = agg["alg_flops"] / (FP32_MFMA_PEAK_TFLOPS * 1e12), agg["alg_bytes"] / (HBM_PEAK_GBS * 1e9)  # (live MACs)
        hbm = {"achieved": round(gbs, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 5)}
        # achieved / frac price the LIVE multiply-adds (operands that exist; `_job_flops`); beside them the work the kernel issues
        # (dead taps dropped, padded positions multiplied by zeros) and the padded convention of SURVEY 8(d) / rounds 1-3
        mfma = {"achieved": round(tfl, 3), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(tfl / FP32_MFMA_PEAK_TFLOPS, 5),
                "frac_live": round(tfl / FP32_MFMA_PEAK_TFLOPS, 5), "frac_executed": round(tfl_exec / FP32_MFMA_PEAK_TFLOPS, 5),
                "frac_padded": round(tfl_pad / FP32_MFMA_PEAK_TFLOPS, 5)}
        main_roof, other = (("mfma", mfma), ("hbm", hbm)) if t_mfma >= t_hbm else (("hbm", hbm), ("mfma", mfma))
        line["roofline"] = {"bound": main_roof[0], "kernel": agg["kernel"], **main_roof[1], "traffic": agg["pmc_traffic_bytes"],
                            "avg_launch_ms": round(agg["ms"], 5), "launches_per_step": agg["launches_per_step"],
                            "alg_bytes_per_launch": round(agg["alg_bytes"]), "alg_flops_per_launch": round(agg["alg_flops"]),
                            "executed_flops_per_launch": round(agg["executed_flops"]),
                            "alg_flops_padded_per_launch": round(agg["padded_flops"]),
                            other[0]: other[1]}
        try:
            line["families"] = family_table(agg["trace"], trainer, world)
        except Exception as e:  # noqa: BLE001
            line["families"] = {"error": repr(e)}
    # the longest single launch of the step (attention backward of the decoder's last block) against HBM and against the
    # bound that actually holds it: vector-instruction issue (2 v_exp_f32 at 8 cycles + 5 packed FMA/MUL at 4 per 2
    # (query, key) pairs; 1024 SIMDs at the 2.4 GHz peak clock)
    if longest is None:
        line["roofline_longest_launch"] = line["roofline_issue"] = {"error": longest_err}
    else:
        achieved = longest["alg_bytes"] / (longest["ms"] * 1e-3) / 1e9
        tp = longest["pair_evals"] / longest["ms"] / 1e9
        line["roofline_longest_launch"] = {"bound": "hbm", "kernel": longest["kernel"], "achieved": round(achieved, 2),
                                           "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                                           "traffic": longest["pmc_traffic_bytes"], "avg_launch_ms": round(longest["ms"], 4)}
        # `frac` = against the ALGORITHM's minimum (1 exp + 7 FMA per pair); `frac_own_isa` = against the kernel's own instruction
        # stream (what rounds 1-3 called frac: it cannot say whether fewer instructions would do)
        line["roofline_issue"] = {"bound": "valu_issue", "kernel": longest["kernel"], "achieved": round(tp, 3),
                                  "peak": round(ALG_ISSUE_BOUND_TPAIRS["bwd"], 3), "unit": "T (query,key) pairs/s",
                                  "frac": round(tp / ALG_ISSUE_BOUND_TPAIRS["bwd"], 4),
                                  "peak_definition": "algorithmic minimum: 1 v_exp_f32 (8 issue cycles) + 5 FMA as packed pairs (2 cycles each) per pair (dq from the forward's moments)",
                                  "peak_own_isa": round(ISSUE_BOUND_TPAIRS, 3), "frac_own_isa": round(tp / ISSUE_BOUND_TPAIRS, 4)}
        tpf = longest["pair_evals"] / longest["ms_fwd"] / 1e9
        line["roofline_issue_fwd"] = {"bound": "valu_issue", "kernel": "attn_stage_fwd_kernel<1,4,true> (T=1024,H=1,C=1)",
                                      "avg_launch_ms": round(longest["ms_fwd"], 4), "achieved": round(tpf, 3),
                                      "peak": round(ALG_ISSUE_BOUND_TPAIRS["fwd"], 3), "unit": "T (query,key) pairs/s",
                                      "frac": round(tpf / ALG_ISSUE_BOUND_TPAIRS["fwd"], 4),
                                      "peak_definition": "algorithmic minimum: 1 v_exp_f32 (8 issue cycles) + 3 FMA as packed pairs (2 cycles each) per pair"}
    try:
        line["roofline_issue_c2"] = {"bound": "valu_issue", **time_attention_c2(A)}
    except Exception as e:  # noqa: BLE001
        line["roofline_issue_c2"] = {"error": repr(e)}
    if args.workload == "sinkhorn":
        line["sinkhorn"] = time_sinkhorn(A)
    if world == 1:
        line["eager_ms_per_step"] = round(time_eager_route(A, args.workload, pool), 4)
        try:
            line["lightning_route_ms_per_step"] = round(time_lightning_route(A, args.workload, pool), 4)
        except Exception as e:  # noqa: BLE001
            line["lightning_route_ms_per_step"] = {"error": repr(e)}
        try:
            line["parity"] = parity_check(A)
        except Exception as e:  # noqa: BLE001
            line["parity"] = {"error": repr(e)}
        if not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(A)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--workload", choices=["gaussian", "sinkhorn"], default="gaussian",
                    help="gaussian = BASELINE configs[1] (the metric's configuration, default); sinkhorn = configs[2]")
    ap.add_argument("--full", action="store_true",
                    help="also the side measurements (rooflines, kernel families, eager / Lightning routes, parity, CPU baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32 / float64)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world == 1:
        raise SystemExit("launch N > 1 with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...")
    # Rehearsal of the N > 1 call sequence on a one-GPU box (OTVAE_BENCH_SHARE_GPU=1): every rank uses cuda:0 and the
    # collectives go over gloo (RCCL refuses two ranks on one device).  The line it prints is marked and is not a result.
    share_gpu = world > 1 and os.environ.get("OTVAE_BENCH_SHARE_GPU", "0") == "1"
    if share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if share_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from ot_vae_lightning_amd import build as otbuild
    if rank == 0 and not os.path.exists(otbuild.LIB):
        otbuild.build(verbose=False)
    if world > 1:
        dist.barrier()
    import ot_vae_lightning_amd as A
    from ot_vae_lightning_amd.utils.synthetic import mnist_like

    B = PER_GPU_BATCH
    model = build_model(A, workload=args.workload).cuda().train()
    A.broadcast_module(model, src=0)  # identical replicas (no-op for one rank)
    latent_model = A.GaussianTransport(128, source_cfg=dict(dtype=torch.double, reduce_on_update=False),
                                       target_cfg=dict(dtype=torch.double, reduce_on_update=False),
                                       transport_cfg=dict(make_pd=True)).cuda()
    trainer = A.HipTrainer(model, batch_shape=(B, 1, 32, 32), use_graph=not args.no_graph, latent_stats=latent_model)
    # resident synthetic data: 4 different MNIST-like batches per rank, rotated
    pool = [mnist_like(B, seed=1000 + 17 * rank + i).cuda() for i in range(4)]
    torch.cuda.synchronize()

    for i in range(args.warmup):
        trainer.step(pool[i % len(pool)])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        out = trainer.step(pool[i % len(pool)])
    t_host = time.perf_counter() - t0    # the host has ENQUEUED the K steps (graph launches, collectives); the device may lag behind
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if world > 1:
        tmax = torch.tensor([dt], device="cuda", dtype=torch.float64)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    final_loss = [float(v) for v in out.tolist()]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, trainer, latent_model, out)

    if rank == 0:
        ips = world * B * args.steps / dt
        line = {
            "metric": "training images/sec (whole node) + OT-loss rel-err vs CPU ref",
            "value": round(ips, 1), "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 4), "host_enqueue_ms_per_step": round(t_host / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": ("MNIST-32 CNN VAE (capacity 8, latent 128x1x1, residual=add) + GaussianPrior("
                                    "loss_coeff=0.1): fwd+bwd+Adam + latent Gaussian statistics update, hipGraph replay")
                       if args.workload == "gaussian" else
                       ("MNIST-32 CNN VAE (capacity 8, latent 128x1x1, residual=add) + Sinkhorn OT prior (eps=0.05, "
                        "50 iterations, 1024x1024 plan): fwd+bwd+Adam + latent Gaussian statistics update"),
                       "per_gpu_batch": B, "global_batch": world * B,
                       "parallelism": (f"dp{world}: one process per GPU, flat-gradient all-reduce over RCCL"
                                       + (", decoder half overlapped with the encoder's backward" if trainer.dp_overlap else ""))
                       if world > 1 else "single GPU"},
            "final_loss": final_loss,
            **({"rehearsal": "ranks share cuda:0, collectives over gloo: call-sequence check, not a measurement"}
               if share_gpu else {}),
            "step_roofline": {"alg_gbytes_per_s": round(ips * ALG_BYTES_PER_IMAGE_FWD_BWD / 1e9 / world, 2),
                              "frac_of_hbm_peak": round(ips / world * ALG_BYTES_PER_IMAGE_FWD_BWD / 1e9 / HBM_PEAK_GBS, 5),
                              "alg_tflops": round(ips / world * ALG_FLOP_PER_IMAGE_FWD_BWD / 1e12, 3),
                              "frac_of_fp32_peak": round(ips / world * ALG_FLOP_PER_IMAGE_FWD_BWD / 1e12 / FP32_VALU_PEAK_TFLOPS, 5)},
        }
        if args.full:
            line.update(side_measurements(A, args, trainer, pool, world))
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        # ordinary teardown: wait for the reducer's stream, drop the captured graphs, then the communicator
        trainer.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
