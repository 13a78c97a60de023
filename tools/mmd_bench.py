"""MMD operator and prior on one MI355X.

1. ``otvae::mmd_prior`` + ``otvae::mmd_prior_backward`` (imq, the seven default scales, unbiased) at N = M = 1024, D = 128 against, on
   the same device and the same inputs, the torch composition (Gram-form distances, the kernel function, autograd).  The candidates
   take turns inside every round (one process, device events around ``--iters`` back-to-back calls); median and minimum over the rounds
   are reported in microseconds per forward + backward.
2. The captured training step of the MNIST-32 CNN VAE (BASELINE configs[1] network, batch 1024) with ``MMDPrior()``, with
   ``SinkhornPrior(0.05, 50)`` and with ``SlicedWassersteinPrior(128)``, alternating windows of ``--steps`` steps.

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

SCALES = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)


def composition(z, y, gout, gadd):
    """unbiased imq MMD2 forward + backward out of library operators (what a user would write)"""
    z = z.detach().requires_grad_(True)
    n, d = z.shape
    m = y.shape[0]

    def k(a, b):
        r = ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)).clamp_min(0.0)
        out = 0.0
        for s in SCALES:
            c = 2.0 * d * s
            out = out + c / (c + r)
        return out

    kzz, kyy, kzy = k(z, z), k(y, y), k(z, y)
    loss = ((kzz.sum() - kzz.diagonal().sum()) / (n * (n - 1)) + (kyy.sum() - kyy.diagonal().sum()) / (m * (m - 1))
            - 2.0 * kzy.mean())
    lossv = loss.expand(n)
    (gz,) = torch.autograd.grad(lossv, z, gout)
    return lossv.detach(), gadd + gz


def op_candidates(n, m, d):
    gen = torch.Generator().manual_seed(0)
    z = (1.3 * torch.randn(n, d, generator=gen) + 0.2).cuda()
    y = torch.randn(m, d, generator=gen).cuda()
    gout = torch.full((n,), 1.0 / n, device="cuda")
    gadd = torch.randn(n, d, generator=gen).cuda()
    scales = list(SCALES)

    def ours():
        loss, G, _ = torch.ops.otvae.mmd_prior(z, y, 0, scales, 1.0, True, 1.0, True)
        return loss, torch.ops.otvae.mmd_prior_backward(gout, gadd, G)

    def torch_composition():
        return composition(z, y, gout, gadd)

    # the two forms agree before anything is timed (gout sums to 1: the same gradient; the composition's loss is fp32 throughout)
    la, g0 = ours()[0], torch.ops.otvae.mmd_prior(z, y, 0, scales, 1.0, True, 1.0, True)[1]
    lb, g1 = composition(z, y, gout, torch.zeros_like(gadd))
    torch.cuda.synchronize()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    assert rel(la, lb) < 1e-3 and rel(g0, g1) < 1e-3, (rel(la, lb), rel(g0, g1))
    return {"mmd_prior": ours, "torch_composition": torch_composition}


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

    trs = {"MMDPrior()": trainer(A.MMDPrior(seed=1)),
           "SinkhornPrior(0.05, 50)": trainer(A.SinkhornPrior(reg=0.05, max_iter=50, threshold=0.0, seed=1)),
           "SlicedWassersteinPrior(128)": trainer(A.SlicedWassersteinPrior(n_projections=128, seed=1))}
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
        raise SystemExit("mmd_bench needs the MI355X: there is nothing to time on the host")
    n, m, d = 1024, 1024, 128
    result = {"device": torch.cuda.get_device_name(0), "N": n, "M": m, "D": d, "op": None, "step": None}
    r = time_ops(op_candidates(n, m, d), args.rounds, args.iters, args.warmup)
    result["op"] = r
    print(f"forward + backward, N = M = {n}, D = {d}, imq, {len(SCALES)} scales  (median / min over {args.rounds} rounds of {args.iters} calls)")
    for k, v in r.items():
        print(f"    {k:20s} {v['median_us']:9.1f} us  {v['min_us']:9.1f} us")
    print(f"    mmd_prior vs torch composition: {r['torch_composition']['median_us'] / r['mmd_prior']['median_us']:.2f}x")
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
    if r["mmd_prior"]["median_us"] >= r["torch_composition"]["median_us"]:
        raise SystemExit("mmd_prior does not beat the torch composition")


if __name__ == "__main__":
    main()
