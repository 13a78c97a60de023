"""Multi-scale SSIM on fp32 image pairs beside the float32 torch composition of the definition, in one process, at two shapes:

    [256, 3, 64, 64]    3 betas, sigma 1.0 (7 taps)         the reconstruction-loss shape
    [16, 3, 256, 256]   the default 5 betas, 11 x 11 window  the validation shape

    update        MultiScaleStructuralSimilarityIndexMeasure.update          (csrc/ssim.hip: one launch per scale + the fold)
    loss          MSSSIMLoss(preds, target).backward()                        (that forward, then one gradient launch per scale)
    composition   per scale: stack the five maps, grouped conv2d over the valid positions, the maps element-wise, mean per image,
                  two avg_pool2d; the product of powers; for the loss its .backward()   (what a user would write without the kernels)
    scale 0       the forward launches of ONE scale at the same shape (betas = (1.0,): tile launch + fold, no pooled output) beside
                  otvae::ssim_accum, and the first launch of the multi-scale call by difference: (2 scales) - (1 scale at H / 2)

Device-event timing: warm-up, then --repeats timed calls each between two events, median (and min / max); all routes are alternated
inside every repeat.  The spread is (max - min) / median of the repeats.

    timeout 600 python tools/ms_ssim_bench.py [--repeats 30] [--out profiles/ms_ssim_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
CASES = (((256, 3, 64, 64), 1.0, BETAS[:3]), ((16, 3, 256, 256), 1.5, BETAS))


def composition(p, t, kernel, betas):
    """the definition in the dtype of ``p``, data_range 1, normalize relu: msssim [B]"""
    b, c = p.shape[:2]
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    v = []
    for s in range(len(betas)):
        mu_p, mu_t, e_pp, e_tt, e_pt = F.conv2d(torch.cat([p, t, p * p, t * t, p * t]), kernel, groups=c).split(b)
        s_pp, s_tt, s_pt = e_pp - mu_p * mu_p, e_tt - mu_t * mu_t, e_pt - mu_p * mu_t
        cs = (2 * s_pt + c2) / (s_pp + s_tt + c2)
        if s == len(betas) - 1:
            cs = (2 * mu_p * mu_t + c1) / (mu_p * mu_p + mu_t * mu_t + c1) * cs
        v.append(cs.reshape(b, -1).mean(-1))
        if s + 1 < len(betas):
            p, t = F.avg_pool2d(p, 2), F.avg_pool2d(t, 2)
    return (torch.relu(torch.stack(v)) ** torch.tensor(betas, dtype=p.dtype, device=p.device)[:, None]).prod(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ms_ssim_bench needs the MI355X: a CPU run says nothing about these kernels")
    if args.repeats < 20:
        raise SystemExit("at least 20 repeats")
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import MSSSIMLoss, metrics
    from ot_vae_lightning_amd.metrics.ssim import gaussian_window
    names = ("update", "composition fwd", "loss fwd+bwd", "composition fwd+bwd", "1 scale", "ssim_accum", "2 scales", "1 scale at H/2")
    lines = [f"# multi-scale SSIM, fp32, data_range 1; median of {args.repeats} (min .. max) in microseconds, spread = (max - min) / median"]
    for shape, sigma, betas in CASES:
        b, c, h, w = shape
        gen = torch.Generator("cuda").manual_seed(h * w + b)
        target = torch.rand(shape, device="cuda", generator=gen)
        preds = (target + 0.1 * torch.randn(shape, device="cuda", generator=gen)).clamp(0, 1).requires_grad_(True)
        half_p, half_t = F.avg_pool2d(preds.detach(), 2), F.avg_pool2d(target, 2)
        kw = dict(sigma=sigma, data_range=1.0)
        metric = metrics.MultiScaleStructuralSimilarityIndexMeasure(betas=betas, **kw).cuda()
        one, two = (metrics.MultiScaleStructuralSimilarityIndexMeasure(betas=bt, **kw).cuda() for bt in ((1.0,), (0.5, 0.5)))
        half = metrics.MultiScaleStructuralSimilarityIndexMeasure(betas=(1.0,), **kw).cuda()
        ssim = metrics.StructuralSimilarityIndexMeasure(**kw).cuda()
        loss_fn = MSSSIMLoss(betas=betas, **kw).cuda()
        g1 = torch.tensor(gaussian_window(sigma), dtype=torch.float64)
        kernel = torch.outer(g1, g1).float().cuda().expand(c, 1, -1, -1).contiguous()
        grads, values = [None, None], [None, None]

        def update():
            metric.update(preds.detach(), target)

        def comp_fwd():
            with torch.no_grad():
                values[1] = composition(preds, target, kernel, betas)

        def loss():
            preds.grad = None
            loss_fn(preds, target).backward()
            grads[0] = preds.grad

        def comp_loss():
            preds.grad = None
            (1.0 - composition(preds, target, kernel, betas)).mean().backward()
            grads[1] = preds.grad

        fns = (update, comp_fwd, loss, comp_loss, lambda: one.update(preds.detach(), target), lambda: ssim.update(preds.detach(), target),
               lambda: two.update(preds.detach(), target), lambda: half.update(half_p, half_t))
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
                times[k].append(e0.elapsed_time(e1) * 1e3)
        med = [statistics.median(t) for t in times]
        lines.append(f"# {'x'.join(map(str, shape))}, {len(betas)} betas, sigma {sigma} ({len(g1)} taps)")
        for k, name in enumerate(names):
            lines.append(f"  {name:>20} | {med[k]:9.1f} ({min(times[k]):8.1f} .. {max(times[k]):8.1f}) | spread {(max(times[k]) - min(times[k])) / med[k]:5.2f}")
        pooled_launch = med[6] - med[7]
        lines.append(f"  update is {med[1] / med[0]:.2f} x the composition's forward, the loss {med[3] / med[2]:.2f} x the composition's forward + backward")
        lines.append(f"  one scale (tile launch + fold) / ssim_accum = {med[4] / med[5]:.2f}; the pooling launch by difference "
                     f"{pooled_launch:.1f} us = {pooled_launch / med[5]:.2f} x ssim_accum (it moves 1.25 x the bytes)")
        # both routes computed the same thing
        values[0] = metrics.multiscale_structural_similarity(preds.detach(), target, betas=betas, **kw)
        rel_v = float(((values[0] - values[1].double()).abs() / values[0].abs()).max())
        rel_g = float((grads[0] - grads[1]).abs().max()) / float(grads[1].abs().max())
        lines.append(f"  agreement with the composition: values {rel_v:.1e}, gradient {rel_g:.1e}")
        assert rel_v < 1e-3 and rel_g < 1e-3, (rel_v, rel_g)
        if med[2] >= med[3]:
            lines.append(f"# {shape}: the loss is NOT faster than the torch composition ({med[2]:.1f} vs {med[3]:.1f} us)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
