"""One ``StructuralSimilarityIndexMeasure.update`` (11 x 11 Gaussian window, data_range = 1) on fp32 image pairs of the shapes the
package's workloads produce, beside two yardsticks, in one process:

    ssim          StructuralSimilarityIndexMeasure.update                       (csrc/ssim.hip: tile launch + one-workgroup fold)
    composition   the definition in fp32 torch: stack the five maps, grouped conv2d over the valid positions, the map
                  element-wise, mean per image, two in-place adds into a state   (what a user would write without the kernel)
    sqerr         torch.ops.otvae.sqerr_accum on the same pair: it reads both tensors once, the floor for any metric of the pair

Device-event timing: warm-up, then --repeats timed calls each between two events, median (and min / max); the three are
alternated inside every repeat.  Bytes: the algorithmic 2 * itemsize * B * C * H * W (each tensor read once) over the median time.

    timeout 600 python tools/ssim_bench.py [--repeats 30] [--out profiles/ssim_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1024, 1, 32, 32), (256, 3, 32, 32), (64, 3, 64, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_bench needs the MI355X: a CPU run says nothing about these kernels")
    if args.repeats < 20:
        raise SystemExit("at least 20 repeats")
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd.metrics import PeakSignalNoiseRatio, StructuralSimilarityIndexMeasure
    from ot_vae_lightning_amd.metrics.ssim import gaussian_window
    lines = [f"# one SSIM update, fp32, 11 x 11 Gaussian window, data_range 1; median of {args.repeats} (min .. max), microseconds",
             f"# {'shape':>16} | {'ssim update':>28} | {'torch composition':>28} | {'sqerr_accum':>28} | ssim GB/s | x composition | x sqerr"]
    g1 = torch.tensor(gaussian_window(1.5), dtype=torch.float64)
    for shape in SHAPES:
        b, c, h, w = shape
        gen = torch.Generator("cuda").manual_seed(h * w + b)
        target = torch.rand(shape, device="cuda", generator=gen)
        preds = (target + 0.1 * torch.randn(shape, device="cuda", generator=gen)).clamp(0, 1)
        metric = StructuralSimilarityIndexMeasure(data_range=1.0).cuda()
        psnr = PeakSignalNoiseRatio(data_range=1.0).cuda()
        kernel = torch.outer(g1, g1).float().cuda().expand(c, 1, -1, -1).contiguous()
        state = torch.zeros(2, dtype=torch.float64, device="cuda")
        c1, c2 = 0.01 ** 2, 0.03 ** 2

        def ours():
            metric.update(preds, target)

        def composition():
            mu_p, mu_t, e_pp, e_tt, e_pt = F.conv2d(torch.cat([preds, target, preds * preds, target * target, preds * target]), kernel,
                                                    groups=c).split(b)
            s_pp, s_tt, s_pt = e_pp - mu_p * mu_p, e_tt - mu_t * mu_t, e_pt - mu_p * mu_t
            ssim = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_pp + s_tt + c2))
            state[0] += ssim.reshape(b, -1).mean(-1).double().sum()
            state[1] += b

        def floor():
            torch.ops.otvae.sqerr_accum(preds, target, psnr.sqerr_state)

        fns = (ours, composition, floor)
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
        nbytes = 2 * preds.element_size() * preds.numel()
        lines.append(f"  {'x'.join(map(str, shape)):>16} | {cell(0)} | {cell(1)} | {cell(2)} | {nbytes / (med[0] * 1e-6) / 1e9:9.1f} | "
                     f"{med[1] / med[0]:13.2f} | {med[0] / med[2]:7.2f}")
        # both routes saw the same inputs the same number of times
        n_calls = args.warmup + args.repeats
        assert float(metric.total) == float(state[1]) == n_calls * b
        rel = abs(float(metric.compute()) - float(state[0] / state[1])) / abs(float(metric.compute()))
        assert rel < 1e-4, rel
        if med[0] >= med[1]:
            lines.append(f"# {shape}: the update is NOT faster than the torch composition ({med[0]:.1f} vs {med[1]:.1f} us)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
