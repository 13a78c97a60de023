"""Precision / recall / density / coverage of two feature sets (k = 5), at the metric's default shape and at a small-set shape, in one
process on the SAME features:

    prdc          precision_recall_density_coverage: two otvae_knn_sq_radii, one otvae_manifold_counts, integer reductions in torch
    radii         torch.ops.otvae.knn_sq_radii on both sets (csrc/knn_manifold.hip: full within-set blocks, k-smallest selection)
    counts        torch.ops.otvae.manifold_counts alone (the cross block: ball memberships, minima)
    torch fp64    the equal-precision composition: Gram-form distances in row blocks, topk, comparisons
    torch fp32    the same composition in float32 (for information: its decisions can differ near a radius)
    KID 1 subset  KernelDistance.compute() with one subset of all rows: the yardstick for the shared 128 x 128 main loop (it computes
                  the lower triangles of the within-set blocks only)

Device-event timing: warm-up, then --repeats rounds; inside every round the variants run one after the other (interleaved), each
between two events; the median per variant is reported (min .. max beside it).  Useful work of prdc is 2 D (N^2 + M^2 + N M) FLOP
(no block uses symmetry), of KID 2 D (n (n + 1) + n^2), both against the fp64 matrix peak; the per-tile times compare the epilogues.

    timeout 900 python tools/prdc_bench.py [--repeats 20] [--out profiles/prdc_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_MATRIX_PEAK = 78.6e12   # FLOP/s, MI355X fp64 matrix (DESIGN.md kernel table)
SHAPES = (("default", 10000, 2048), ("small set", 500, 192))   # name, rows per side, D
K = 5
BLOCK = 2048


def composition(real, fake, k, dtype):
    real, fake = real.to(dtype), fake.to(dtype)
    nr, nf = (real * real).sum(1), (fake * fake).sum(1)

    def sq_radii(x, nx):
        out = []
        for lo in range(0, x.shape[0], BLOCK):
            d2 = (nx[lo:lo + BLOCK, None] + nx[None, :] - 2.0 * (x[lo:lo + BLOCK] @ x.T)).clamp_min_(0.0)
            rows = torch.arange(d2.shape[0], device=x.device)
            d2[rows, lo + rows] = float("inf")
            out.append(d2.topk(k, dim=1, largest=False).values[:, k - 1])
        return torch.cat(out)

    r2_real, r2_fake = sq_radii(real, nr), sq_radii(fake, nf)
    count_fake = torch.zeros(fake.shape[0], dtype=torch.int64, device=real.device)
    hit, low = [], []
    for lo in range(0, real.shape[0], BLOCK):
        d2 = (nr[lo:lo + BLOCK, None] + nf[None, :] - 2.0 * (real[lo:lo + BLOCK] @ fake.T)).clamp_min_(0.0)
        count_fake += (d2 <= r2_real[lo:lo + BLOCK, None]).sum(0)
        hit.append((d2 <= r2_fake[None, :]).any(1))
        low.append(d2.min(1).values)
    n, m = real.shape[0], fake.shape[0]
    return torch.stack([(count_fake > 0).sum() / m, torch.cat(hit).sum() / n, count_fake.sum() / (k * m),
                        (torch.cat(low) <= r2_real).sum() / n]).double()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prdc_bench needs the MI355X: a CPU run says nothing about these kernels")
    if args.repeats < 20:
        raise SystemExit("at least 20 repeats")
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd.metrics import KernelDistance, precision_recall_density_coverage
    names = ("prdc", "radii", "counts", "torch fp64", "torch fp32", "KID 1 subset")
    lines = [f"# precision / recall / density / coverage, k = {K}, fp32 features, median of {args.repeats} interleaved rounds (min .. max), "
             "milliseconds"]
    for name, n, d in SHAPES:
        g = torch.Generator("cuda").manual_seed(d)
        real = torch.relu(torch.randn(n, d, device="cuda", generator=g) + 0.5)
        fake = torch.relu(1.1 * torch.randn(n, d, device="cuda", generator=g) + 0.4)
        kid = KernelDistance(feature_size=d, max_observations=n, subsets=1, subset_size=n, seed=0).cuda()
        kid.update(real, fake)
        r2_real, r2_fake = torch.ops.otvae.knn_sq_radii(real, K), torch.ops.otvae.knn_sq_radii(fake, K)
        out = {}

        def f_prdc():
            out["prdc"] = torch.stack(precision_recall_density_coverage(real, fake, k=K))

        def f_radii():
            out["radii"] = (torch.ops.otvae.knn_sq_radii(real, K), torch.ops.otvae.knn_sq_radii(fake, K))

        def f_counts():
            out["counts"] = torch.ops.otvae.manifold_counts(real, r2_real, fake, r2_fake)

        def f_fp64():
            out["fp64"] = composition(real, fake, K, torch.float64)

        def f_fp32():
            out["fp32"] = composition(real, fake, K, torch.float32)

        def f_kid():
            out["kid"] = kid.compute()

        fns = (f_prdc, f_radii, f_counts, f_fp64, f_fp32, f_kid)
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in fns]
        for _ in range(args.repeats):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[i].append(e0.elapsed_time(e1))
        med = [statistics.median(t) for t in times]
        nt = -(-n // 128)
        flops = {"prdc": 2 * d * 3 * n * n, "radii": 2 * d * 2 * n * n, "counts": 2 * d * n * n, "KID 1 subset": 2 * d * (n * (n + 1) + n * n)}
        tiles = {"radii": 2 * nt * nt, "counts": nt * nt, "KID 1 subset": nt * (nt + 1) + nt * nt}
        lines.append(f"# {name}: {n} rows per side, D = {d}; values (prdc) {[round(v, 4) for v in out['prdc'].tolist()]}, "
                     f"fp64 composition differs by {float((out['prdc'] - out['fp64']).abs().max()):.1e}, "
                     f"fp32 composition by {float((out['prdc'] - out['fp32']).abs().max()):.1e}")
        for i, nm in enumerate(names):
            line = f"  {nm:>12} | {med[i]:9.3f} ({min(times[i]):8.3f} .. {max(times[i]):8.3f})"
            if nm in flops:
                rate = flops[nm] / (med[i] * 1e-3)
                line += f" | {rate / 1e12:6.2f} useful TFLOP/s ({100 * rate / FP64_MATRIX_PEAK:5.1f} % of the fp64 matrix peak)"
            if nm in tiles:
                line += f" | {1e3 * med[i] / tiles[nm]:7.2f} us per tile / {min(256, tiles[nm])} CUs busy"
            lines.append(line)
        lines.append(f"  torch fp64 / prdc = {med[3] / med[0]:.2f} x, torch fp32 / prdc = {med[4] / med[0]:.2f} x")
        if med[0] > med[3]:
            lines.append(f"# {name}: prdc does NOT beat the fp64 composition ({med[0]:.3f} vs {med[3]:.3f} ms)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
