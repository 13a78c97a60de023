"""One ``KernelDistance.compute()`` (Kernel Inception Distance: the polynomial-kernel MMD^2 of S random subsets of m rows per side,
mean and std), at torchmetrics' default shape and at a small-set shape, four ways in one process on the SAME subset indices:

    compute       KernelDistance.compute(): counts read on the host, indices drawn on the device, otvae_poly_mmd_subsets
    kernel        torch.ops.otvae.poly_mmd_subsets alone (csrc/kid.hip), on the indices the metric drew last
    torch fp64    per subset: two row gathers, .double(), three GEMMs, pow, diagonal handling, sums -- the equal-precision comparison
    torch fp32    the same composition in float32 (for information: it is 1e-7 ... 1e-4 off)

Device-event timing: warm-up, then --repeats rounds; inside every round the four are run one after the other (interleaved), each
between two events; the median per variant is reported (min .. max beside it).  Achieved fp64 FLOP/s of the kernel counts the useful
work S (2 m (m + 1) / 2 + m^2) 2 D against the fp64 matrix peak.

    timeout 900 python tools/kid_bench.py [--repeats 20] [--out profiles/kid_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_MATRIX_PEAK = 78.6e12   # FLOP/s, MI355X fp64 matrix (DESIGN.md kernel table)
SHAPES = (("default", 10000, 2048, 100, 1000), ("small set", 500, 192, 100, 100))   # name, rows per side, D, subsets, subset size


def composition(real, fake, idx_real, idx_fake, gamma, coef, degree, dtype):
    vals = []
    for ir, jf in zip(idx_real, idx_fake):
        x, y = real[ir].to(dtype), fake[jf].to(dtype)
        m = x.shape[0]
        k_xx, k_yy, k_xy = ((a @ b.T * gamma + coef) ** degree for a, b in ((x, x), (y, y), (x, y)))
        within = (k_xx.sum() - torch.diagonal(k_xx).sum()) + (k_yy.sum() - torch.diagonal(k_yy).sum())
        vals.append(within / (m * (m - 1)) - 2.0 * k_xy.sum() / (m * m))
    per = torch.stack(vals)
    return per, per.mean(), per.std(unbiased=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kid_bench needs the MI355X: a CPU run says nothing about these kernels")
    if args.repeats < 20:
        raise SystemExit("at least 20 repeats")
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd.metrics import KernelDistance
    lines = [f"# one KID evaluation (degree 3, gamma 1 / D, coef 1), fp32 features, median of {args.repeats} interleaved rounds "
             "(min .. max), milliseconds",
             f"# {'shape':>28} | {'compute()':>26} | {'kernel':>26} | {'torch fp64':>26} | {'torch fp32':>26} | kernel fp64 FLOP/s "
             "(share of matrix peak) | fp64 composition / kernel | fp32 composition error"]
    for name, n, d, subsets, m in SHAPES:
        g = torch.Generator("cuda").manual_seed(d)
        real = torch.relu(torch.randn(n, d, device="cuda", generator=g) + 0.5)
        fake = torch.relu(1.1 * torch.randn(n, d, device="cuda", generator=g) + 0.4)
        metric = KernelDistance(feature_size=d, max_observations=n, subsets=subsets, subset_size=m, seed=0).cuda()
        metric.update(real, fake)
        metric.compute()
        idx_real, idx_fake, _ = metric.last_subsets
        lr, lf = idx_real.long(), idx_fake.long()
        gamma = 1.0 / d
        out = {}

        def f_compute():
            out["compute"] = metric.compute()

        def f_kernel():
            out["kernel"] = torch.ops.otvae.poly_mmd_subsets(real, fake, idx_real, idx_fake, m, 3, gamma, 1.0)

        def f_fp64():
            out["fp64"] = composition(real, fake, lr, lf, gamma, 1.0, 3, torch.float64)

        def f_fp32():
            out["fp32"] = composition(real, fake, lr, lf, gamma, 1.0, 3, torch.float32)

        fns = (f_compute, f_kernel, f_fp64, f_fp32)
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in fns]
        for _ in range(args.repeats):
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        med = [statistics.median(t) for t in times]
        cell = lambda k: f"{med[k]:8.3f} ({min(times[k]):7.3f} .. {max(times[k]):7.3f})"  # noqa: E731
        flops = subsets * (m * (m + 1) + m * m) * 2 * d
        rate = flops / (med[1] * 1e-3)
        per, _ = out["kernel"]
        per64, per32 = out["fp64"][0], out["fp32"][0]
        agree = float((per - per64).abs().max() / per64.abs().max())
        assert agree < 1e-9, agree                                    # both fp64: they differ by summation order only
        err32 = float((per32.double() - per).abs().max() / per.abs().max())
        lines.append(f"  {name + f' n={n} D={d} {subsets}x{m}':>28} | {cell(0)} | {cell(1)} | {cell(2)} | {cell(3)} | "
                     f"{rate / 1e12:6.2f} TFLOP/s ({100 * rate / FP64_MATRIX_PEAK:5.1f} %) | {med[2] / med[1]:6.2f} x | {err32:.1e}")
        if med[1] > med[2]:
            lines.append(f"# {name}: the kernel does NOT beat the fp64 composition ({med[1]:.3f} vs {med[2]:.3f} ms)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
