"""The definition of multi-scale SSIM in torch, shared by ``test_gpu_ms_ssim.py`` and ``test_gpu_ms_ssim_loss.py``: the truth in float64,
the "composition" a user would write in float32.  Not a test module."""
import torch
import torch.nn.functional as F

BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def windows(gaussian=True, sigma=1.5, kernel_size=11):
    from ot_vae_lightning_amd.metrics.ssim import _pair, gaussian_window
    if gaussian:
        return [torch.tensor(gaussian_window(float(s)), dtype=torch.float64) for s in _pair(sigma, "sigma")]
    return [torch.full((k,), 1.0 / k, dtype=torch.float64) for k in _pair(kernel_size, "kernel_size")]


def option_kwargs(window):
    return dict(gaussian_kernel=window.get("gaussian", True), sigma=window.get("sigma", 1.5), kernel_size=window.get("kernel_size", 11))


def definition(p, t, wh, ww, data_range, betas, normalize="relu", k1=0.01, k2=0.03, detach_pooled=False):
    """(msssim [B], v [S][B]) in the dtype of ``p``: the issue's definition, nothing else.  ``detach_pooled`` cuts the graph at the
    pooling, which leaves the scale-0 term of the gradient alone."""
    dtype = p.dtype
    t = t.to(dtype)
    b, c = p.shape[:2]
    kernel = torch.outer(wh, ww).to(dtype).expand(c, 1, -1, -1)
    v = []
    for s in range(len(betas)):
        ps, ts = p, t
        if isinstance(data_range, tuple):
            ps, ts = p.clamp(*data_range), t.clamp(*data_range)       # each scale clamps its own images ...
            rng = data_range[1] - data_range[0]
        elif data_range is None:
            rng = torch.maximum(p.max() - p.min(), t.max() - t.min())   # ... or takes its own range
        else:
            rng = data_range
        mu_p, mu_t, e_pp, e_tt, e_pt = F.conv2d(torch.cat([ps, ts, ps * ps, ts * ts, ps * ts]), kernel, groups=c).split(b)
        s_pp, s_tt, s_pt = e_pp - mu_p * mu_p, e_tt - mu_t * mu_t, e_pt - mu_p * mu_t
        c1, c2 = (k1 * rng) ** 2, (k2 * rng) ** 2
        cs = (2 * s_pt + c2) / (s_pp + s_tt + c2)
        ssim = (2 * mu_p * mu_t + c1) / (mu_p * mu_p + mu_t * mu_t + c1) * cs
        v.append((ssim if s == len(betas) - 1 else cs).reshape(b, -1).mean(-1))
        p, t = F.avg_pool2d(p, 2), F.avg_pool2d(t, 2)                   # ... and the pooling takes the unclamped values
        if detach_pooled:
            p, t = p.detach(), t.detach()
    v = torch.stack(v)
    f = torch.relu(v) if normalize == "relu" else ((v + 1) / 2 if normalize == "simple" else v)
    return (f ** torch.tensor(betas, dtype=dtype)[:, None]).prod(0), v


def pair_of(shape, rng, seed, dtype=torch.float32, lo=0.0, clamp=True):
    """``tests/test_gpu_ssim.py``'s inputs: the target uniform noise, the prediction the target plus 0.1 R Gaussian noise, clamped"""
    g = torch.Generator().manual_seed(seed)
    target = lo + rng * torch.rand(shape, generator=g, dtype=torch.float64)
    preds = target + 0.1 * rng * torch.randn(shape, generator=g, dtype=torch.float64)
    if clamp:
        preds = preds.clamp(lo, lo + rng)
    return preds.to(dtype), target.to(dtype)


def independent_pair():
    """two independent uniform images per pair: v = [[0.0587, 0.0326], [-0.0725, 0.0737], [0.2481, 0.6481]] at sigma 0.5, data_range 1,
    so image 0 is dead under ``relu`` (and NaN under ``None``) while image 1 is alive"""
    g = torch.Generator().manual_seed(3)
    t = torch.rand((2, 1, 32, 32), generator=g, dtype=torch.float64)
    p = torch.rand((2, 1, 32, 32), generator=g, dtype=torch.float64)
    return p, t


# shape, window, betas: the issue's table
CASES = [((2, 1, 32, 32), dict(sigma=0.5), BETAS[:3]),
         ((2, 3, 45, 43), dict(gaussian=False, kernel_size=(3, 5)), BETAS[:4]),
         ((2, 2, 23, 21), dict(sigma=0.5), BETAS[:3]),
         ((1, 1, 176, 177), dict(), BETAS)]
CASE_IDS = ["x".join(map(str, c[0])) for c in CASES]
