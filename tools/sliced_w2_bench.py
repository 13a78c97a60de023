"""Sliced-W2 operator and prior on one MI355X.

1. ``otvae::sliced_w2`` forward + backward at N = 1024, D = 128, L in {64, 256} against, on the same device and the same inputs,
   (a) the torch composition (normalise, two matmuls, two ``torch.sort``, scatter, matmul) and
   (b) ``otvae::sinkhorn_prior`` forward + backward (reg 0.05, 50 iterations) at the same N and D.
   The candidates take turns inside every round (one process, device events around ``--iters`` back-to-back calls); median and minimum
   over the rounds are reported in microseconds per forward + backward.
2. The captured training step of the MNIST-32 CNN VAE (BASELINE configs[1] network, batch 1024) with ``SlicedWassersteinPrior(128)`` and
   with ``SinkhornPrior(0.05, 50)``, alternating windows of ``--steps`` steps.

Prints a table and one JSON line (``--json FILE`` also writes it)."""
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
from ot_vae_lightning_amd.utils.synthetic import mnist_like  # noqa: E402


def composition(z, y, g, gout, gadd):
    """sliced W2 forward + backward out of library operators (what a user would write)"""
    n, nl = z.shape[0], g.shape[0]
    theta = g / g.norm(dim=1, keepdim=True)
    p, q = z @ theta.T, y @ theta.T
    ps, order = torch.sort(p, dim=0, stable=True)
    qs = torch.sort(q, dim=0).values
    diff = ps - qs
    loss = (diff * diff).sum() * (1.0 / (nl * n))
    r = torch.empty_like(p).scatter_(0, order, diff)
    gz = gadd + (gout.sum() * (2.0 / (nl * n))) * (r @ theta)
    return loss.expand(n), gz


def op_candidates(n, d, nl):
    gen = torch.Generator().manual_seed(0)
    z = (1.3 * torch.randn(n, d, generator=gen) + 0.2).cuda()
    y = torch.randn(n, d, generator=gen).cuda()
    g = torch.randn(nl, d, generator=gen).cuda()
    gout = torch.full((n,), 1.0 / n, device="cuda")
    gadd = torch.randn(n, d, generator=gen).cuda()

    def ours():
        loss, resid, theta = torch.ops.otvae.sliced_w2(z, y, g, 1.0)
        return loss, torch.ops.otvae.sliced_w2_backward(gout, gadd, resid, theta, 1.0)

    def torch_composition():
        return composition(z, y, g, gout, gadd)

    def sinkhorn():
        cost, pi, _ = torch.ops.otvae.sinkhorn_prior(z, y, 0.05, 50, 0.0, 1.0)
        return cost, torch.ops.otvae.sinkhorn_prior_backward(gout, gadd, z, y, pi, 1.0)

    # the two forms of the sliced distance agree before anything is timed (gout sums to 1: the same gradient)
    (la, ga), (lb, gb) = ours(), torch_composition()
    torch.cuda.synchronize()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    assert rel(la, lb) < 1e-4 and rel(ga, gb) < 1e-4, (rel(la, lb), rel(ga, gb))
    return {"sliced_w2": ours, "torch_composition": torch_composition, "sinkhorn_prior": sinkhorn}


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
    return {k: {"median_us": statistics.median(v), "min_us": min(v)} for k, v in us.items()}


def step_times(batch, steps, warmup, windows):
    def trainer(prior):
        torch.manual_seed(0)
        enc = A.CNN(1, 128, 32, 1, capacity=8, down_sample=True, residual="add")
        dec = A.CNN(128, 1, 1, 32, capacity=8, up_sample=True, residual="add")
        model = A.VAE(encoder=enc, decoder=dec, prior=prior).cuda().train()
        return A.HipTrainer(model, batch_shape=(batch, 1, 32, 32), data_parallel=False)

    trs = {"SlicedWassersteinPrior(128)": trainer(A.SlicedWassersteinPrior(n_projections=128, seed=1)),
           "SinkhornPrior(0.05, 50)": trainer(A.SinkhornPrior(reg=0.05, max_iter=50, threshold=0.0, seed=1))}
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
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "img_per_s": batch / statistics.median(v) * 1e3, "loss": last[k]}
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sliced_w2_bench needs the MI355X: there is nothing to time on the host")
    n, d = 1024, 128
    result = {"device": torch.cuda.get_device_name(0), "N": n, "D": d, "op": {}, "step": None}
    for nl in (64, 256):
        r = time_ops(op_candidates(n, d, nl), args.rounds, args.iters, args.warmup)
        result["op"][str(nl)] = r
        print(f"forward + backward, N = {n}, D = {d}, L = {nl}  (median / min over {args.rounds} rounds of {args.iters} calls)")
        for k, v in r.items():
            print(f"    {k:20s} {v['median_us']:9.1f} us  {v['min_us']:9.1f} us")
        print(f"    sliced_w2 vs torch composition: {r['torch_composition']['median_us'] / r['sliced_w2']['median_us']:.2f}x, "
              f"vs sinkhorn_prior: {r['sinkhorn_prior']['median_us'] / r['sliced_w2']['median_us']:.2f}x")
    if not args.skip_step:
        s = step_times(args.batch, args.steps, args.warmup, args.windows)
        result["step"] = s
        print(f"captured step, MNIST-32 CNN VAE, batch {args.batch}  (median / min over {args.windows} windows of {args.steps} steps)")
        for k, v in s.items():
            print(f"    {k:28s} {v['median_ms']:8.3f} ms  {v['min_ms']:8.3f} ms  {v['img_per_s']:9.0f} img/s  loss {v['loss']}")
    line = json.dumps(result)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    lost = [nl for nl, r in result["op"].items() if r["sliced_w2"]["median_us"] >= r["torch_composition"]["median_us"]]
    if lost:
        raise SystemExit(f"sliced_w2 does not beat the torch composition at L = {', '.join(lost)}")


if __name__ == "__main__":
    main()
