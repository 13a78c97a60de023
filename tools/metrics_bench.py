"""One feature-moments update (n, sum f, sum f f^T in fp64) at B = 1024 for D in {192, 768, 2048}, three ways in one process:

    gauss_stats   otvae_gauss_stats(accumulate=1, decay<0): the latent-statistics kernel, all there was before csrc/metrics.hip
    torch         sum_xx += f.double().T @ f.double(); sum_x += f.double().sum(0); n += B      (rocBLAS fp64 + element-wise adds)
    moments       otvae_moments_accum (torch.ops.otvae.moments_accum)

Device-event timing: warm-up, then --repeats timed calls each between two events, median (and min / max); the three are
alternated inside every repeat.  Shares of peak for the new kernel: useful FLOPs = B D (D + 1) (the lower triangle, 2 per
multiply-add) over the fp64 matrix peak, and the bytes it must move (B D 4 read + D^2 8 read and written) over the HBM peak.

    timeout 600 python tools/metrics_bench.py [--repeats 30] [--out profiles/metrics_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_MATRIX_PEAK = 78.6e12   # FLOP/s, MI355X fp64 matrix (DESIGN.md kernel table)
HBM_PEAK = 8.0e12            # B/s, spec (6.29e12 measured by a float4 copy)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench needs the MI355X: a CPU run says nothing about these kernels")
    if args.repeats < 20:
        raise SystemExit("at least 20 repeats")
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import _lib
    from ot_vae_lightning_amd._lib import check, ptr, stream
    lib = _lib.load()
    b = args.batch
    lines = [f"# one moments update, B = {b}, fp32 features, median of {args.repeats} (min .. max), microseconds",
             f"# {'D':>5} | {'gauss_stats':>28} | {'torch fp64':>28} | {'moments_accum':>28} | ws bytes (x D^2*8) | fp64-MFMA share | HBM share"]
    ok = True
    for d in (192, 768, 2048):
        f = torch.randn(b, d, device="cuda", generator=torch.Generator("cuda").manual_seed(d))
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")  # noqa: E731
        st_old, st_torch, st_new = (z(1), z(d), z(d, d)), (z(1), z(d), z(d, d)), (z(1), z(d), z(d, d))
        ws_old = torch.empty(max(8, lib.otvae_gauss_stats_ws(1, b, d, 0)), device="cuda", dtype=torch.uint8)

        def old():
            check(lib.otvae_gauss_stats(0, ptr(f), 1, b, d, 0, 1, -1.0, ptr(ws_old), ptr(st_old[0]), ptr(st_old[1]), ptr(st_old[2]),
                                        stream()), "otvae_gauss_stats")

        def eager():
            fd = f.double()
            st_torch[2].addmm_(fd.T, fd)
            st_torch[1].add_(fd.sum(0))
            st_torch[0].add_(b)

        def new():
            torch.ops.otvae.moments_accum(f, *st_new)

        fns = (old, eager, new)
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        times = [[], [], []]
        for _ in range(args.repeats):
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
        med = [statistics.median(t) for t in times]
        cell = lambda k: f"{med[k]:9.1f} ({min(times[k]):8.1f} .. {max(times[k]):8.1f})"  # noqa: E731
        ws_new = lib.otvae_moments_accum_ws(b, d)
        t_new = med[2] * 1e-6
        flop_share = b * d * (d + 1) / FP64_MATRIX_PEAK / t_new
        byte_share = (b * d * 4 + 2 * d * d * 8) / HBM_PEAK / t_new
        lines.append(f"  {d:>5} | {cell(0)} | {cell(1)} | {cell(2)} | {ws_new:>10} ({ws_new / (d * d * 8):4.2f}) | "
                     f"{100 * flop_share:13.1f} % | {100 * byte_share:7.1f} %")
        # all three agree (same inputs, same number of calls)
        n_calls = args.warmup + args.repeats
        assert float(st_new[0]) == float(st_old[0]) == n_calls * b
        rel = float((st_new[2] - st_torch[2]).abs().max() / st_torch[2].abs().max())
        assert rel < 1e-12, rel
        if d >= 768 and not med[2] < med[0]:
            ok = False
            lines.append(f"# D = {d}: moments_accum is NOT below otvae_gauss_stats")
        if med[2] > med[1]:
            lines.append(f"# D = {d}: moments_accum loses to the torch column ({med[2]:.1f} vs {med[1]:.1f} us)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
