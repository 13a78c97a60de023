"""Case tables, input builders, fp64 truths, bound functions and fp32 emulations shared by ``test_step_chain_host.py`` and
``test_gpu_step_chain.py`` (no tests here): the kernels that end every training step in ``csrc/loss_optim.hip`` -- ``otvae_step_begin``,
``otvae_nelbo_fwd / _bwd``, ``otvae_copy_batched``, ``otvae_grad_clip_coef``, ``otvae_adam_step`` (step guard, state restore, folded
parameter EMA), ``otvae_ema_update`` and ``otvae_zero_words`` -- each on its own.  Pure torch / numpy on the CPU.

The truth of an operation is its plain definition in fp64 on the fp32 operands widened to fp64 (hyper-parameters included: the kernel
reads lr, b1, b2, eps as fp32).  Every bound is first-order rounding propagation through the kernel's operation order, per element,
from the truth: u = 2^-24 per fp32 rounding (division and square root are correctly rounded in this build, powf is held to its
documented 1 ulp = 2 u), times ONE margin, ``MARGIN``, for the second-order terms.  The count stands beside each bound.  Nothing
here comes from a measured HIP number.  Builders are cached per process: callers must not modify what they get."""
import functools
import math

import numpy as np
import torch

import otvae_oracle as O

U32 = 2.0 ** -24
U64 = 2.0 ** -53
MARGIN = 1.25          # over every rounding count below (the issue allows up to 2)
F32, F64 = torch.float32, torch.float64
INF, NAN = float("inf"), float("nan")
SPECIALS = (INF, -INF, NAN)
SENT = -6.25e22        # prefill of every output buffer and guard band: no kernel here produces it from these inputs
SENT_INT = -77
BAND = 64              # guard band, elements, on both sides of a buffer (a multiple of 4: the 16-byte alignment survives)

# lr, b1, b2, eps as the kernel reads them: fp32
HYPER = torch.tensor([1e-3, 0.9, 0.999, 1e-8], dtype=F32)


def hyper64(hyper=HYPER):
    return tuple(float(x) for x in hyper.double())


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn32(n, seed):
    return torch.randn(n, generator=gen(seed), dtype=F64).to(F32)


def _f64(x):
    """tensor or Python number as fp64 on the host (a Python float must not pass through torch's default fp32)"""
    return x.detach().double().cpu() if isinstance(x, torch.Tensor) else torch.tensor(x, dtype=F64)


def worst_ratio(got, truth, bound):
    """max |got - truth| / bound element-wise (a zero bound admits a zero error only; inf if anything is not finite)"""
    g, t, b = _f64(got), _f64(truth), _f64(bound)
    assert g.shape == t.shape, (g.shape, t.shape)
    if g.numel() == 0:
        return 0.0
    r = ((g - t).abs() / (b + 1e-300)).max().item()
    return r if math.isfinite(r) else INF


def rel_err(got, truth):
    """max |got - truth| / |truth| over truth != 0"""
    g, t = _f64(got), _f64(truth)
    nz = t != 0
    if not bool(nz.any()):
        return 0.0
    r = ((g[nz] - t[nz]).abs() / t[nz].abs()).max().item()
    return r if math.isfinite(r) else INF


def median_rel_err(got, truth):
    """median |got - truth| / |truth| over truth != 0: an error common to all elements (the bias corrections') shows here, one that
    a single cancellation makes does not"""
    g, t = _f64(got), _f64(truth)
    nz = t != 0
    if not bool(nz.any()):
        return 0.0
    return ((g[nz] - t[nz]).abs() / t[nz].abs()).median().item()


def bits_equal(a, b):
    """same shape and the same bit patterns (NaN equals the same NaN, -0 differs from +0)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == F32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    elif a.dtype == F64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return torch.equal(a, b)


def banded(inner, device="cpu", fill=None):
    """(whole, view): ``inner`` (a tensor, or a length for a pure output that starts from the sentinel) between two guard bands of
    BAND sentinels.  ``view`` is what the kernel is handed."""
    if isinstance(inner, int):
        inner = torch.full((inner,), SENT if fill is None else fill, dtype=F32)
    sent = SENT if inner.dtype.is_floating_point else SENT_INT
    whole = torch.full((inner.numel() + 2 * BAND,), sent, dtype=inner.dtype)
    whole[BAND:BAND + inner.numel()] = inner
    whole = whole.to(device)
    return whole, whole[BAND:BAND + inner.numel()]


def bands_intact(whole):
    w = whole.detach().cpu()
    sent = SENT if w.dtype.is_floating_point else SENT_INT
    ref = torch.full((BAND,), sent, dtype=w.dtype)
    return bits_equal(w[:BAND], ref) and bits_equal(w[-BAND:], ref)


# ======================================================================================================== 1. otvae_adam_step
# n: tail only (1, 3) / body only (4) / both (5) / under, on and over one block of 256 float4 (1023, 1024, 1025) / 4099: five blocks and
# a tail / 2 * 2^20 + 1024 + 3: the grid capped at 2048 blocks of 1024 elements, a second pass of one block, and a tail of three
ADAM_N = (1, 3, 4, 5, 1023, 1024, 1025, 4099, 2 * 2 ** 20 + 1024 + 3)
ADAM_T = (1, 2, 10, 1000, 100000)
ADAM_SCALES = (1.0, 0.5)
ADAM_GRID_CAP, ADAM_PER_BLOCK = 2048, 1024


def adam_grid(n):
    return min(-(-n // ADAM_PER_BLOCK), ADAM_GRID_CAP)


@functools.lru_cache(maxsize=None)
def adam_inputs(n, seed=0):
    """g, m, v (fp32): magnitudes log-uniform over [1e-6, 1e3], g and m signed; exact zeros in g (i % 7 == 3), in m (i % 11 == 5),
    in m and v (i % 13 == 2) and, at the LAST index where n >= 5, in all three: a fresh parameter with a zero gradient"""
    ge = gen(100 + 7 * seed + n % 9973)
    mag = lambda: 10.0 ** (torch.rand(n, generator=ge, dtype=F64) * 9.0 - 6.0)            # noqa: E731
    sign = lambda: torch.where(torch.rand(n, generator=ge) < 0.5, -1.0, 1.0).double()     # noqa: E731
    g, m, v = mag() * sign(), mag() * sign(), mag()
    i = torch.arange(n)
    g[i % 7 == 3] = 0.0
    m[i % 11 == 5] = 0.0
    both = i % 13 == 2
    m[both], v[both] = 0.0, 0.0
    if n >= 5:
        g[-1] = m[-1] = v[-1] = 0.0
    return g.to(F32), m.to(F32), v.to(F32)


@functools.lru_cache(maxsize=None)
def generic_p(n, seed=0):
    """parameters of order 1, none near zero"""
    p = randn32(n, 900 + seed)
    return torch.where(p.abs() < 0.25, p + p.sign() + (p == 0), p)


def bias_corrections(t, b1, b2):
    return 1.0 - b1 ** t, 1.0 - b2 ** t


ADAM_DEFECTS = ("t-1", "no bc2", "eps inside sqrt", "g not squared", "tail unchanged", "scale twice")


def adam_truth(g, m, v, p, s, t, hyper=HYPER, defect=None):
    """torch.optim.Adam's rule (no weight decay, no amsgrad) in fp64 on the widened fp32 operands: m', v', the update u = p - p'
    and p'.  ``defect``: one of ADAM_DEFECTS, a single wrong step of a plausible kernel."""
    lr, b1, b2, eps = hyper64(hyper)
    g, m, v, p = g.double(), m.double(), v.double(), p.double()
    gs = g * s * (s if defect == "scale twice" else 1.0)
    m2 = b1 * m + (1.0 - b1) * gs
    v2 = b2 * v + (1.0 - b2) * (gs if defect == "g not squared" else gs * gs)
    bc1, bc2 = bias_corrections(t - 1 if defect == "t-1" else t, b1, b2)
    if defect == "no bc2":
        bc2 = 1.0
    if bc1 == 0.0:      # t - 1 = 0
        upd = torch.full_like(m2, INF)
    elif defect == "eps inside sqrt":
        upd = (lr / bc1) * m2 / torch.sqrt(v2 / bc2 + eps)
    else:
        upd = (lr / bc1) * m2 / (torch.sqrt(v2) / math.sqrt(bc2) + eps)
    p2 = p - upd
    if defect == "tail unchanged" and g.numel() % 4:
        k = g.numel() - g.numel() % 4
        m2[k:], v2[k:], p2[k:], upd[k:] = m[k:], v[k:], p[k:], 0.0
    return dict(m=m2, v=v2, upd=upd, p=p2)


# ---- the rounding counts of adam_kernel (csrc/loss_optim.hip), per element --------------------------------------------------------
# gg = g * s                       1
# m' = fma(b1, m, (1 - b1) * gg)   1 - b1 is exact for b1 in [0.5, 1] (Sterbenz); the product 1, the fma 1.  With gg's: 3, each
#                                  relative to a term no larger than |b1 m| + |(1 - b1) g s| (m and g may cancel: an ABSOLUTE bound)
ADAM_M_COUNT = 3
# v' = fma(b2, v, (1 - b2) * gg * gg)   gg enters twice 2, two products 2, the fma 1: all terms >= 0, so 5 RELATIVE to v'
ADAM_V_COUNT = 5
# u = (lr / bc1) * m' / (sqrt(v') / bc2s + eps):  lr / bc1, step_size * m', sqrt, / bc2s, + eps, the final division: 6 (the errors of the
# denominator's first term weigh D / (D + eps) <= 1)
ADAM_U_COUNT = 6
# bc1 = 1 - powf(b1, t): powf within 1 ulp = 2 u of b1^t = 1 - bc1, the subtraction 1:  (1 + 2 (1 / bc1 - 1)) u relative to bc1
# bc2s = sqrtf(1 - powf(b2, t)): the same halved by the root, and the root's own rounding: (1.5 + (1 / bc2 - 1)) u
# At t = 1, powf(b, 1) = b and 1 - b are exact: bc1 carries nothing, bc2s the root's rounding alone.
# Sum for t > 1: 6 + 2.5 (half of v's 5) + 1 + 1.5 - 2 - 1 = 8, plus 2 / bc1 + 1 / bc2  -- the cancellation of the bias corrections.


def adam_rel_count(t, bc1, bc2, with_v=True):
    """the update's relative rounding count, without m's share: (c0 + c1 / bc1 + c2 / bc2) with c0 = 8, c1 = 2, c2 = 1 for t > 1,
    and 9.5 flat at t = 1.  ``with_v=False`` leaves v's 2.5 out (the chain carries v's error itself)."""
    c = ADAM_U_COUNT + (ADAM_V_COUNT / 2.0 if with_v else 0.0)
    if t == 1:
        return c + 1.0
    return c + (1.0 + 2.0 * (1.0 / bc1 - 1.0)) + (1.5 + (1.0 / bc2 - 1.0))


def adam_bounds(g, m, v, s, t, truth, hyper=HYPER, Em=0.0, Ev=0.0, es=0.0):
    """per-element bounds (m, v, upd) of ONE step from the truth.  Em, Ev: error bounds already on the incoming m and v; es: the
    absolute error bound on the scale s (all zero for a single step on exact inputs)."""
    lr, b1, b2, eps = hyper64(hyper)
    g, m, v = g.double(), m.double(), v.double()
    bc1, bc2 = bias_corrections(t, b1, b2)
    dm = b1 * Em + MARGIN * ADAM_M_COUNT * U32 * ((b1 * m).abs() + ((1.0 - b1) * g * s).abs()) + (1.0 - b1) * g.abs() * es
    dv = b2 * Ev + MARGIN * ADAM_V_COUNT * U32 * truth["v"] + 2.0 * (1.0 - b2) * g * g * abs(s) * es
    den = torch.sqrt(truth["v"]) / math.sqrt(bc2) + eps
    du = (lr / bc1) * dm / den
    if isinstance(Ev, float) and Ev == 0.0 and es == 0.0:
        du = du + MARGIN * U32 * adam_rel_count(t, bc1, bc2) * truth["upd"].abs()
    else:       # v's whole error through d u / d v = -u D / (2 v' (D + eps)), |.| <= |u| / (2 v')
        assert bool((truth["v"] > 0).all())
        du = du + MARGIN * U32 * adam_rel_count(t, bc1, bc2, with_v=False) * truth["upd"].abs() + truth["upd"].abs() * dv / (2.0 * truth["v"])
    return dict(m=dm, v=dv, upd=du)


def p_bound(truth, du):
    """the new parameter: the update's bound and the half ulp of the final subtraction"""
    return du + U32 * truth["p"].abs()


def _fma32(a, b, c):
    return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def adam_emulate(g, m, v, p, s, t, hyper=HYPER):
    """the kernel's operation order in numpy fp32 (the fma through one fp64 product and sum)"""
    f = np.float32
    lr, b1, b2, eps = (f(x) for x in hyper.tolist())
    g, m, v, p = (x.numpy() for x in (g, m, v, p))
    gg = g * f(s)
    m2 = _fma32(b1, m, (f(1) - b1) * gg)
    v2 = _fma32(b2, v, (f(1) - b2) * gg * gg)
    bc1 = f(1) - np.power(b1, f(t), dtype=f)
    bc2s = np.sqrt(f(1) - np.power(b2, f(t), dtype=f), dtype=f)
    step = lr / bc1
    upd = step * m2 / (np.sqrt(v2) / bc2s + eps)
    p2 = p - upd
    assert all(a.dtype == np.float32 for a in (m2, v2, upd, p2))
    return dict(m=torch.from_numpy(m2), v=torch.from_numpy(v2), upd=torch.from_numpy(upd), p=torch.from_numpy(p2))


# ======================================================================================================== 2. the guard matrix
GUARD_N = 5
GUARD_N_STATE = (0, 7, 1000)        # 1000 > the 256 threads of the one-block grid: the restore loop strides
GUARD_SOURCES = ("watch_loss", "norm", "host grad_scale", "device grad_scale")
GUARD_VALUES = (0.5, INF, -INF, NAN)


def guard_refuses(value):
    return not math.isfinite(value)


# ======================================================================================================== 3. the parameter EMA
EMA_DECAYS = (0.0, 0.9, 0.9999, 1.0)
EMA_T = (1, 79, 80, 81, 1000)       # (1 + t) / (10 + t) = 0.9 at t = 80: the warm-up hands over to decay 0.9 there
EMA_N = (1, 1025, 2 * 2 ** 20 + 5)  # ema_update_kernel: one element / two blocks / the grid capped at 2048 with a second pass
EMA_IN_ADAM_N = 1027                # float4 body over two blocks and a tail of three


def ema_rule(shadow, p, decay, t, off_by=0):
    """``oracle.ParamEMARef``'s rule, one update that is the t-th: d = min(decay, (1 + t) / (10 + t)) and torch's three fp32 roundings
    shadow - ((shadow - p) * (1 - d)).  ``off_by``: the warm-up evaluated that many steps off (a defect)."""
    ref = O.ParamEMARef([shadow.clone()], decay)
    ref.num_updates = t - 1 + off_by
    ref.update([p])
    return ref.shadow[0]


def ema_fixed_rule(shadow, p, decay):
    """the stand-alone kernel takes the EFFECTIVE decay: the same three roundings with 1 - decay, no warm-up"""
    tmp = shadow - p
    tmp.mul_(1.0 - decay)
    return shadow - tmp


# ======================================================================================================== 4. otvae_grad_clip_coef
# 4096 elements per part, at most 512 parts: tail only (1, 3) / one float4 (4) / under, on and over one part / capped parts whose
# blocks make a second pass, with a tail
CLIP_N = (1, 3, 4, 4095, 4096, 4097, 512 * 4096 + 4099)
CLIP_SCALES = (1.0, 0.25)
CLIP_MAX_NORM_FACTORS = (0.5, 2.0, 0.0, -1.0)     # max_norm = factor x the true norm: clipping, not clipping, report only (<= 0)
CLIP_EPS = float(np.float32(1e-6))                # the kernel's 1e-6f
CLIP_PARTS, CLIP_PER_PART = 512, 4096
# norm = (float) sqrt(sum) * s: per pair two fp32 squares and one fp32 add (2 u on a sum of non-negative terms, halved by the root: 1),
# the cast 1, the product with s 1.  The fp64 accumulation adds n 2^-53 to the sum, half of it to the root.
CLIP_NORM_COUNT = 3
# out[0] = s * (max_norm / (norm + 1e-6f)): the norm's 3, the sum 1, the division 1, the product 1.  Not clipping: s itself, exact.
CLIP_COEF_COUNT = 6
CLIP_DEFECTS = ("no 1e-6", "scale twice")


def clip_parts(n):
    return min(CLIP_PARTS, -(-n // CLIP_PER_PART))


@functools.lru_cache(maxsize=None)
def clip_gradient(n):
    """randn scaled to a norm of about 0.1: 1e-6 is then 1e-5 of the norm, far above the bound, and every square is a normal fp32"""
    return (randn32(n, 4000 + n % 9973).double() * (0.1 / math.sqrt(n))).to(F32) if n > 1 else torch.tensor([0.1], dtype=F32)


def clip_in_range(g):
    """the range in which the reported norm is accurate: every non-zero square is a normal fp32 number"""
    a = g.double().abs()
    a = a[a != 0]
    return bool(((a * a >= 2.0 ** -126) & (a * a <= float(np.finfo(np.float32).max))).all())


def clip_truth(g, s, max_norm, defect=None):
    """clip_grad_norm_'s coefficient on the mean gradient g s: (out[0], out[1]) = (s min(1, max_norm / (|g s| + 1e-6)), |g s|); with
    max_norm <= 0 the scale is s and the norm is reported only"""
    norm = math.sqrt(float((g.double() ** 2).sum())) * s
    coef = 1.0
    if max_norm > 0:
        coef = min(1.0, max_norm / (norm + (0.0 if defect == "no 1e-6" else CLIP_EPS)))
    return s * coef * (s if defect == "scale twice" else 1.0), norm


def clip_bounds(n, s, max_norm, truth):
    out0, norm = truth
    acc = n * U64 / 2.0
    clipped = max_norm > 0 and max_norm / (norm + CLIP_EPS) < 1.0
    d0 = (MARGIN * CLIP_COEF_COUNT * U32 + acc) * abs(out0) if clipped else 0.0
    return d0, (MARGIN * CLIP_NORM_COUNT * U32 + acc) * norm


def clip_emulate(g, s, max_norm):
    """the kernel's arithmetic: fp32 squares and pair sums, fp64 accumulation, fp32 from the cast on"""
    f = np.float32
    a = g.numpy()
    n4 = a.size // 4 * 4
    q = a[:n4].reshape(-1, 4)
    with np.errstate(over="ignore", invalid="ignore"):      # an overflowing square is +inf, as in the kernel
        body = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]).astype(np.float64).sum() + (q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]).astype(np.float64).sum()
        total = body + (a[n4:] * a[n4:]).astype(np.float64).sum()
    norm = f(np.sqrt(total)) * f(s)
    coef = f(max_norm) / (norm + f(1e-6))
    coef = coef if coef < f(1) else f(1)
    if not max_norm > 0:
        coef = f(1)
    return float(f(s) * coef), float(norm)


# ======================================================================================================== 5. otvae_nelbo_fwd / _bwd
# forward: 1024 elements per part, at most 256 parts -- one element / under, on, over one part / capped parts with a second pass
NELBO_FWD_NUMEL = (1, 1023, 1024, 1025, 256 * 1024 + 7)
NELBO_B = (1, 257)                  # the final kernel's 256 threads stride the prior vector: 257 gives thread 0 a second entry
NELBO_CHW = (1.0, 3072.0)
# backward: 256 elements per block, at most 2048 blocks -- one element / over one block / the capped grid with a second pass
NELBO_BWD_NUMEL = (1, 257, 2048 * 256 + 5)
NELBO_GOUT = (0.75, -1.5, 0.3125)
NELBO_PARTS, NELBO_PER_PART = 256, 1024
# recon = (float)(sum (pred - target)^2 / numel): the difference 1 -- twice in the square -- and the square 1: 3 on a sum of
# non-negative terms, the cast 1.  fp64 accumulation: numel 2^-53.
NELBO_RECON_COUNT = 4
# prior = (float)(sum prior_loss / B) / chw: the cast 1, the division 1; the fp64 sum may cancel: B 2^-53 of the mean of |prior_loss|
NELBO_PRIOR_COUNT = 2
# total = recon + prior: both errors and the sum's 1
# gpred = (2 (g0 + g1) / numel) (pred - target): the sum 1, the division 1 (2 x and (float) numel are exact), the difference 1, the product 1
NELBO_GPRED_COUNT = 4
# gprior = (g0 + g2) / (B chw): the sum 1, the product 1, the division 1
NELBO_GPRIOR_COUNT = 3
NELBO_DEFECTS = ("prior not divided by chw", "1/numel")


def nelbo_parts(numel):
    return min(NELBO_PARTS, -(-numel // NELBO_PER_PART))


@functools.lru_cache(maxsize=None)
def nelbo_inputs(numel, B):
    seed = 5000 + numel % 9973 + 17 * B
    return randn32(numel, seed), randn32(numel, seed + 1), (5.0 + 3.0 * randn32(B, seed + 2).double()).to(F32)


def nelbo_fwd_truth(pred, target, prior, chw, defect=None):
    """(total, recon, prior term) and their bounds; ``prior`` None: the prior term is exactly 0"""
    numel = pred.numel()
    recon = float(((pred.double() - target.double()) ** 2).sum()) / numel
    pr, dpr = 0.0, 0.0
    if prior is not None:
        B = prior.numel()
        pr = float(prior.double().sum()) / B / (1.0 if defect == "prior not divided by chw" else chw)
        dpr = MARGIN * NELBO_PRIOR_COUNT * U32 * abs(pr) + B * U64 * float(prior.double().abs().sum()) / B / chw
    total = recon + pr
    drecon = (MARGIN * NELBO_RECON_COUNT * U32 + numel * U64) * recon
    return (total, recon, pr), (drecon + dpr + MARGIN * U32 * abs(total), drecon, dpr)


def nelbo_bwd_truth(pred, target, B, chw, gout, defect=None):
    """(gpred, gprior) with out = {recon + prior, recon, prior}: d / d recon = g0 + g1, d / d prior = g0 + g2; ``gout`` None: (1, 0, 0)"""
    g0, g1, g2 = (1.0, 0.0, 0.0) if gout is None else (float(np.float32(x)) for x in gout)
    numel = pred.numel()
    gpred = ((1.0 if defect == "1/numel" else 2.0) * (g0 + g1) / numel) * (pred.double() - target.double())
    gprior = torch.full((B,), (g0 + g2) / (B * chw), dtype=F64)
    return (gpred, gprior), (MARGIN * NELBO_GPRED_COUNT * U32 * gpred.abs(), MARGIN * NELBO_GPRIOR_COUNT * U32 * gprior.abs())


def nelbo_fwd_emulate(pred, target, prior, chw):
    f = np.float32
    d = pred.numpy() - target.numpy()
    recon = f((d * d).astype(np.float64).sum() / pred.numel())
    pr = f(0)
    if prior is not None:
        pr = f(prior.numpy().astype(np.float64).sum() / prior.numel()) / f(chw)
    return float(recon + pr), float(recon), float(pr)


def nelbo_bwd_emulate(pred, target, B, chw, gout):
    f = np.float32
    g = (f(1), f(0), f(0)) if gout is None else tuple(f(x) for x in gout)
    k = f(2) * (g[0] + g[1]) / f(pred.numel())
    gpred = k * (pred.numpy() - target.numpy())
    gprior = np.full((B,), (g[0] + g[2]) / (f(B) * f(chw)), dtype=f)
    return torch.from_numpy(gpred), torch.from_numpy(gprior)


# ======================================================================================================== 6. otvae_copy_batched
# 32 entries per launch: one launch of one / a full launch / a full launch and one entry / two full launches and six
COPY_COUNTS = (1, 32, 33, 70)
COPY_LONGEST = 256 * 1024 + 9       # 1024 elements per block, at most 256: the capped grid, every block a second pass
COPY_CHUNK = 32
_COPY_LENGTHS = (1, 2, 255, 1, 256, 257, 1023, 1, 1025, 4097, 3, 70001)


@functools.lru_cache(maxsize=None)
def copy_layout(count):
    """lengths, source offsets and destination offsets in two flat buffers: the longest entry sits in the first launch (and in the
    second of count = 70) between length-1 entries; entries are separated by gaps of odd sizes that must stay untouched"""
    lengths = [_COPY_LENGTHS[i % len(_COPY_LENGTHS)] for i in range(count)]
    lengths[min(1, count - 1)] = COPY_LONGEST
    if count > 40:
        lengths[40] = COPY_LONGEST
    soff, doff, s, d = [], [], 3, BAND
    for i, n in enumerate(lengths):
        soff.append(s)
        doff.append(d)
        s += n + 1 + i % 3
        d += n + 5 + 2 * (i % 4)
    return lengths, soff, doff, s, d + BAND


def copy_expected(count, src):
    lengths, soff, doff, _, dtotal = copy_layout(count)
    exp = torch.full((dtotal,), SENT, dtype=F32)
    for n, so, do in zip(lengths, soff, doff):
        exp[do:do + n] = src[so:so + n]
    return exp


# ======================================================================================================== 7. otvae_step_begin / otvae_zero_words
# (n, zero_words): 1024 units of work per block (a float of the backup, a 16-byte pair of words), at most 1024 blocks of 256 threads
STEP_BEGIN_CASES = [(0, 0),                                 # the counter alone
                    (0, 2),                                 # zeroing only: one int4
                    (5, 0),                                 # backup only
                    (5, 2 * (1024 * 256 + 5)),              # the zero loop strides: 256 blocks, 262149 int4
                    (1024 * 1024 + 3, 2)]                   # the backup loop strides: 1024 blocks, 1048579 floats
STEP_BEGIN_GRID_CAP = 1024


def step_begin_grid(n, zero_words):
    work = max(n, zero_words // 2)
    return max(1, min(-(-work // 1024), STEP_BEGIN_GRID_CAP))


# ======================================================================================================== 8. the chain
CHAIN_N, CHAIN_STEPS, CHAIN_MAX_NORM, CHAIN_NAN_STEP = 4099, 5, 1.0, 2      # the third step carries a NaN
CHAIN_AMPS = (0.05, 0.001, 0.01, 0.1, 0.005)    # |g| = 64 amp: 3.2, 0.064, (NaN), 6.4, 0.32 against max_norm 1
CHAIN_N_STATE = 300


@functools.lru_cache(maxsize=None)
def chain_inputs():
    p0 = generic_p(CHAIN_N, 8)
    grads = [(CHAIN_AMPS[k] * randn32(CHAIN_N, 8100 + k).double()).to(F32) for k in range(CHAIN_STEPS)]
    grads[CHAIN_NAN_STEP][CHAIN_N // 2] = NAN
    return p0, grads


@functools.lru_cache(maxsize=None)
def chain_truth():
    """five steps of torch.optim.Adam and clip_grad_norm_ in float64 on the host, the NaN step skipped as the guard skips it -- an
    independent implementation -- with the per-step bounds accumulated alongside: after every step (p, m, v, bounds, scale, norm)"""
    p0, grads = chain_inputs()
    lr, b1, b2, eps = hyper64()
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    Ep = torch.zeros(CHAIN_N, dtype=F64)
    Em, Ev = torch.zeros_like(Ep), torch.zeros_like(Ep)
    m_prev, v_prev = torch.zeros_like(Ep), torch.zeros_like(Ep)
    steps, t = [], 0
    for k, g in enumerate(grads):
        if not bool(torch.isfinite(g).all()):
            steps.append(dict(skipped=True, t=t, p=p.detach().clone(), m=m_prev.clone(), v=v_prev.clone(), Ep=Ep.clone(),
                              Em=Em.clone(), Ev=Ev.clone()))
            continue
        t += 1
        p.grad = g.double().clone()
        norm = float(torch.nn.utils.clip_grad_norm_([p], CHAIN_MAX_NORM))
        s = min(1.0, CHAIN_MAX_NORM / (norm + 1e-6))
        p_before = p.detach().clone()
        opt.step()
        st = opt.state[p]
        truth = dict(m=st["exp_avg"].clone(), v=st["exp_avg_sq"].clone(), upd=p_before - p.detach(), p=p.detach().clone())
        # the scale's error: the clip bound, and the kernel's 1e-6f against clip_grad_norm_'s 1e-6
        d0, dnorm = clip_bounds(CHAIN_N, 1.0, CHAIN_MAX_NORM, (s, norm))
        es = d0 + (abs(CLIP_EPS - 1e-6) / norm if s < 1.0 else 0.0)
        b = adam_bounds(g, m_prev, v_prev, s, t, truth, Em=Em, Ev=Ev, es=es)
        Em, Ev = b["m"], b["v"]
        Ep = Ep + b["upd"] + U32 * truth["p"].abs()
        m_prev, v_prev = truth["m"], truth["v"]
        steps.append(dict(skipped=False, t=t, p=truth["p"], m=truth["m"], v=truth["v"], Ep=Ep.clone(), Em=Em.clone(), Ev=Ev.clone(),
                          scale=s, norm=norm, dscale=es, dnorm=dnorm))
    return steps


def chain_emulate():
    """the same chain in the kernels' fp32 arithmetic on the host"""
    p0, grads = chain_inputs()
    p, m, v = p0.clone(), torch.zeros(CHAIN_N), torch.zeros(CHAIN_N)
    out, t = [], 0
    for g in grads:
        s, norm = clip_emulate(g, 1.0, CHAIN_MAX_NORM)
        if math.isfinite(s) and math.isfinite(norm):
            t += 1
            r = adam_emulate(g, m, v, p, s, t)
            p, m, v = r["p"], r["m"], r["v"]
        out.append(dict(p=p.clone(), m=m.clone(), v=v.clone(), t=t))
    return out
