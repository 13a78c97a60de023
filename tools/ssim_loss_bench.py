"""Forward + backward of ``SSIMLoss`` (11 x 11 Gaussian window, data_range = 1, reduction "mean") on fp32 image pairs of the shapes the
package's workloads produce, beside the float32 torch composition's forward + backward, in one process:

    ssim loss     SSIMLoss(preds, target).backward()   (csrc/ssim.hip forward: tile launch + fold; csrc/ssim_grad.hip: one launch;
                  the few element-wise ATen kernels of 1 - x / cast / mean and their backward are inside the window)
    composition   the definition in fp32 torch: stack the five maps, grouped conv2d over the valid positions, the map element-wise,
                  mean per image, 1 - mean, .backward()                           (what a user would write without the kernel)

Device-event timing: warm-up, then --repeats timed calls each between two events, median (and min / max); the two are alternated
inside every repeat.  Bytes: the algorithmic 12 B per pixel at fp32 of the backward alone (both images read once, the gradient
written once) plus the forward's 8, i.e. 20 * B * C * H * W over the median time; the "grad GB/s" column is the 12 B per pixel over
the time of the gradient operator called on its own.

    timeout 600 python tools/ssim_loss_bench.py [--repeats 30] [--out profiles/ssim_loss_bench.txt]
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
        raise SystemExit("ssim_loss_bench needs the MI355X: a CPU run says nothing about these kernels")
    if args.repeats < 20:
        raise SystemExit("at least 20 repeats")
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import SSIMLoss
    from ot_vae_lightning_amd.metrics.ssim import gaussian_window
    lines = [f"# SSIMLoss forward + backward, fp32, 11 x 11 Gaussian window, data_range 1; median of {args.repeats} (min .. max), "
             "microseconds",
             f"# {'shape':>16} | {'ssim loss fwd + bwd':>28} | {'torch composition fwd + bwd':>28} | {'gradient operator alone':>28} | "
             "fwd+bwd GB/s | grad GB/s | x composition"]
    g1 = torch.tensor(gaussian_window(1.5), dtype=torch.float64)
    for shape in SHAPES:
        b, c, h, w = shape
        gen = torch.Generator("cuda").manual_seed(h * w + b)
        target = torch.rand(shape, device="cuda", generator=gen)
        preds = (target + 0.1 * torch.randn(shape, device="cuda", generator=gen)).clamp(0, 1).requires_grad_(True)
        loss_fn = SSIMLoss(data_range=1.0).cuda()
        o = loss_fn.options
        kernel = torch.outer(g1, g1).float().cuda().expand(c, 1, -1, -1).contiguous()
        cot = torch.full((b,), -1.0 / b, dtype=torch.float64, device="cuda")
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        grads = [None, None]

        def ours():
            preds.grad = None
            loss_fn(preds, target).backward()
            grads[0] = preds.grad

        def composition():
            preds.grad = None
            mu_p, mu_t, e_pp, e_tt, e_pt = F.conv2d(torch.cat([preds, target, preds * preds, target * target, preds * target]), kernel,
                                                    groups=c).split(b)
            s_pp, s_tt, s_pt = e_pp - mu_p * mu_p, e_tt - mu_t * mu_t, e_pt - mu_p * mu_t
            ssim = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_pp + s_tt + c2))
            (1.0 - ssim.reshape(b, -1).mean(-1)).mean().backward()
            grads[1] = preds.grad

        def grad_alone():
            torch.ops.otvae.ssim_loss_backward(cot, preds.detach(), target, o.window[0], o.window[1], o.k1, o.k2, o.range_mode, o.range_lo,
                                               o.range_hi)

        fns = (ours, composition, grad_alone)
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
        pixels = preds.numel()
        lines.append(f"  {'x'.join(map(str, shape)):>16} | {cell(0)} | {cell(1)} | {cell(2)} | {20 * pixels / (med[0] * 1e-6) / 1e9:12.1f} | "
                     f"{12 * pixels / (med[2] * 1e-6) / 1e9:9.1f} | {med[1] / med[0]:13.2f}")
        # both routes computed the same gradient
        scale = float(grads[1].abs().max())
        rel = float((grads[0] - grads[1]).abs().max()) / scale
        assert rel < 1e-3, rel
        if med[0] >= med[1]:
            lines.append(f"# {shape}: the loss is NOT faster than the torch composition ({med[0]:.1f} vs {med[1]:.1f} us)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
