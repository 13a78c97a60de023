"""Sinkhorn-divergence operator and prior on one MI355X.

1. ``otvae::sinkhorn_divergence`` + ``otvae::sinkhorn_divergence_backward`` (reg 0.05, 50 iterations) at N = M = 1024, D = 128 and D = 16
   against, on the same device and the same inputs, the same divergence composed from three ``otvae::sinkhorn_prior`` forward calls and
   three ``otvae::sinkhorn_prior_backward`` calls (what a user can write without the operator; every problem is then normalised by its
   own maximum, so the value differs but the work is the same).  Both forms of the solve are timed beside them through the C entry
   point: one batch of three and three consecutive solves.  The candidates take turns inside every round (one process, device events
   around ``--iters`` back-to-back calls); median, minimum and spread (max - min) / median over the rounds, in microseconds per forward +
   backward.
2. The captured training step of the MNIST-32 CNN VAE (BASELINE configs[1] network, batch 1024) with ``SinkhornDivergencePrior()`` and
   with ``SinkhornPrior(0.05, 50)``, alternating windows of ``--steps`` steps.

Prints a table and one JSON line (``--json FILE`` also writes it).  Exits non-zero if the operator is slower than the three-call
composition by more than the run's own spread."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ot_vae_lightning_amd as A  # noqa: E402
from ot_vae_lightning_amd import _lib  # noqa: E402
from ot_vae_lightning_amd._lib import check, ptr, stream  # noqa: E402
from ot_vae_lightning_amd.utils.synthetic import mnist_like  # noqa: E402

REG, ITERS = 0.05, 50


def forward_through_the_entry_point(z, y, batched):
    """``otvae_sinkhorn_div_fwd`` with the form of the solve chosen by the caller (1: one batch of three, 0: three consecutive solves)"""
    lib = _lib.load()
    (n, d), m = z.shape, y.shape[0]
    new = lambda *shape: torch.empty(shape, device=z.device, dtype=z.dtype)  # noqa: E731
    loss, pi_zy, pi_zz = new(n), new(n, m), new(n, n)
    terms = torch.empty(3, device=z.device, dtype=torch.float64)
    iters = torch.empty(1, device=z.device, dtype=torch.int32)
    ws = torch.empty(lib.otvae_sinkhorn_div_ws(0, n, m), device=z.device, dtype=torch.uint8)
    check(lib.otvae_sinkhorn_div_fwd(0, ptr(z), ptr(y), n, m, d, REG, ITERS, 1.0, batched, ptr(ws), ptr(loss), ptr(terms), ptr(pi_zy),
                                     ptr(pi_zz), ptr(iters), stream()), "otvae_sinkhorn_div_fwd")
    return loss, terms, pi_zy, pi_zz, iters


def op_candidates(n, m, d):
    gen = torch.Generator().manual_seed(0)
    z = (1.3 * torch.randn(n, d, generator=gen) + 0.2).cuda()
    y = torch.randn(m, d, generator=gen).cuda()
    gout = torch.full((n,), 1.0 / n, device="cuda")
    gadd = torch.randn(n, d, generator=gen).cuda()
    ops = torch.ops.otvae

    def operator():
        loss, _, pi_zy, pi_zz, _ = ops.sinkhorn_divergence(z, y, REG, ITERS, 1.0)
        return loss, ops.sinkhorn_divergence_backward(gout, gadd, z, y, pi_zy, pi_zz, 1.0)

    def form(batched):
        def run():
            loss, _, pi_zy, pi_zz, _ = forward_through_the_entry_point(z, y, batched)
            return loss, ops.sinkhorn_divergence_backward(gout, gadd, z, y, pi_zy, pi_zz, 1.0)
        return run

    def three_calls():
        c_zy, p_zy, _ = ops.sinkhorn_prior(z, y, REG, ITERS, 0.0, 1.0)
        c_zz, p_zz, _ = ops.sinkhorn_prior(z, z, REG, ITERS, 0.0, 1.0)
        c_yy, _, _ = ops.sinkhorn_prior(y, y, REG, ITERS, 0.0, 1.0)
        loss = c_zy - 0.5 * c_zz - 0.5 * c_yy
        gz = ops.sinkhorn_prior_backward(gout, gadd, z, y, p_zy, 1.0)
        gz = ops.sinkhorn_prior_backward(gout, gz, z, z, p_zz, -0.5)
        return loss, ops.sinkhorn_prior_backward(gout, gz, z, z, p_zz.T.contiguous(), -0.5)

    # the forms agree before anything is timed: the two solves bit for bit, the operator with them
    a, b, c = forward_through_the_entry_point(z, y, 1), forward_through_the_entry_point(z, y, 0), ops.sinkhorn_divergence(z, y, REG, ITERS, 1.0)
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(a, b, c)), "the forms of the solve differ in their bits"
    assert int(a[4]) == ITERS and bool(torch.isfinite(a[0]).all())
    return {"sinkhorn_divergence": operator, "batch_of_three": form(1), "three_consecutive": form(0), "three_sinkhorn_prior_calls": three_calls}


def time_ops(cands, rounds, iters, warmup):
    for f in cands.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in cands}
    for _ in range(rounds):
        for name, f in cands.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                f()
            b.record()
            b.synchronize()
            us[name].append(a.elapsed_time(b) * 1e3 / iters)
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "spread": (max(v) - min(v)) / statistics.median(v)} for k, v in us.items()}


def step_times(batch, steps, warmup, windows):
    def trainer(prior):
        torch.manual_seed(0)
        enc = A.CNN(1, 128, 32, 1, capacity=8, down_sample=True, residual="add")
        dec = A.CNN(128, 1, 1, 32, capacity=8, up_sample=True, residual="add")
        model = A.VAE(encoder=enc, decoder=dec, prior=prior).cuda().train()
        return A.HipTrainer(model, batch_shape=(batch, 1, 32, 32), data_parallel=False)

    trs = {"SinkhornDivergencePrior(0.05, 50)": trainer(A.SinkhornDivergencePrior(reg=REG, max_iter=ITERS, seed=1)),
           "SinkhornPrior(0.05, 50)": trainer(A.SinkhornPrior(reg=REG, max_iter=ITERS, threshold=0.0, seed=1))}
    xs = [mnist_like(batch, seed=5 + i).cuda() for i in range(4)]
    for tr in trs.values():
        for i in range(warmup):
            tr.step(xs[i % 4])
    torch.cuda.synchronize()
    ms = {k: [] for k in trs}
    last = {}
    for _ in range(windows):
        for name, tr in trs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                out = tr.step(xs[i % 4])
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / steps * 1e3)
            last[name] = [float(v) for v in out.tolist()]
    for tr in trs.values():
        tr.close()
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "spread": (max(v) - min(v)) / statistics.median(v),
                "img_per_s": batch / statistics.median(v) * 1e3, "loss": last[k]} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sinkhorn_div_bench needs the MI355X: there is nothing to time on the host")
    n = m = 1024
    result = {"device": torch.cuda.get_device_name(0), "N": n, "M": m, "reg": REG, "max_iter": ITERS, "op": {}, "step": None}
    slower = []
    for d in (128, 16):
        r = time_ops(op_candidates(n, m, d), args.rounds, args.iters, args.warmup)
        result["op"][str(d)] = r
        print(f"forward + backward, N = M = {n}, D = {d}, reg {REG}, {ITERS} iterations  (median / min / spread over {args.rounds} rounds of "
              f"{args.iters} calls)")
        for k, v in r.items():
            print(f"    {k:28s} {v['median_us']:9.1f} us  {v['min_us']:9.1f} us  {v['spread']:6.1%}")
        ours, theirs = r["sinkhorn_divergence"], r["three_sinkhorn_prior_calls"]
        print(f"    sinkhorn_divergence vs three sinkhorn_prior calls: {theirs['median_us'] / ours['median_us']:.2f}x")
        if ours["median_us"] > theirs["median_us"] * (1.0 + max(ours["spread"], theirs["spread"])):
            slower.append(d)
    if not args.skip_step:
        s = step_times(args.batch, args.steps, args.warmup, args.windows)
        result["step"] = s
        print(f"captured step, MNIST-32 CNN VAE, batch {args.batch}  (median / min / spread over {args.windows} windows of {args.steps} steps)")
        for k, v in s.items():
            print(f"    {k:36s} {v['median_ms']:8.3f} ms  {v['min_ms']:8.3f} ms  {v['spread']:6.1%}  {v['img_per_s']:9.0f} img/s  loss {v['loss']}")
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    if slower:
        raise SystemExit(f"sinkhorn_divergence is slower than the three-call composition at D = {slower}")


if __name__ == "__main__":
    main()
