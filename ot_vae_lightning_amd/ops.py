"""PyTorch custom operators (``torch.library``) over the C ABI: the fused ops of the hot path as dispatcher-visible
``torch.ops.otvae.*`` with ``register_fake`` shape functions and ``register_autograd`` formulas, so
that an unmodified ``training_step`` / ``loss.backward()`` runs them, the profiler names them, and tracing sees opaque ops
with known output shapes.  Every forward op has a ``*_backward`` op of its own; nothing here computes outside the HIP library.

    otvae::qkv_attention            QKVAttention.forward                         networks/nets_utils.py:63-82
    otvae::qkv_attention_one_token  AttentionBlock.forward on a one-pixel map    networks/cnn.py:212-240
                                    (one token: the attention returns v)
    otvae::bn_batch_stats +         ConvLayer.forward (BN -> act -> up -> conv)  networks/cnn.py:183-192
    otvae::conv_bn_act
    otvae::gaussian_prior           GaussianPrior.encode (+ loss coefficient)    prior/gaussian.py:63-96, prior/base.py:74-78
    otvae::nelbo_loss               VAE.nelbo's reduction                        model/vae.py:158-176
    otvae::sinkhorn_prior           sq. euclidean cost -> sinkhorn_log -> <C,pi> ot/w2_utils.py:265-269,276-319
    otvae::gaussian_w2_prior        _stats -> mean_cov -> w2_gaussian            gaussian_model.py:144-157, matrix_utils.py:145-158,
                                                                                 w2_utils.py:40-80
    otvae::sliced_w2                sliced Wasserstein-2 (sort and match per     no reference class
                                    projection)
    otvae::mmd_prior                kernel two-sample (MMD) loss and its latent  no reference class
                                    gradient, one fused launch
    otvae::sinkhorn_divergence      debiased entropic OT: W(z,y) - W(z,z)/2 -    no reference class; the solve is
                                    W(y,y)/2 at one epsilon, envelope gradient   sinkhorn_log's, ot/w2_utils.py:276-319
    otvae::soft_cross_entropy       DAD.prior_loss's shifted soft-label CE       model/discrete_auto_diffuser.py:63-72
    otvae::gaussian_blur            torchvision's gaussian_blur (GaussianBlur)   tests/test_latent_transport.py:35
    otvae::ssim_loss                SSIMLoss: the per-image SSIM values [B] and  torchmetrics' ssim, differentiable
                                    their gradient for preds and target
    otvae::ms_ssim                  MSSSIMLoss: the per-image MS-SSIM values     torchmetrics' ms_ssim, differentiable
                                    [B], the scale weights and the pyramid its
                                    backward operator reads

    otvae::moments_accum           FrechetInceptionDistance.update's moments    metrics/fid.py:99-122   (in place, no gradient)
    otvae::sqerr_accum              PeakSignalNoiseRatio.update                  torchmetrics' psnr      (in place, no gradient)
    otvae::ssim_accum               StructuralSimilarityIndexMeasure.update      torchmetrics' ssim      (in place, no gradient)
    otvae::ms_ssim_accum            MultiScaleStructuralSimilarityIndexMeasure   torchmetrics' ms_ssim   (in place, no gradient)
                                    .update
    otvae::feature_append           KernelInceptionDistance.update's store     torchmetrics' kid       (in place, no gradient)
    otvae::poly_mmd_subsets         KernelInceptionDistance.compute: the MMD^2   torchmetrics' kid       (no gradient)
                                    of every random subset and their mean / std
    otvae::knn_sq_radii             PrecisionRecall.compute: k-NN ball radii     no reference class      (no gradient)
    otvae::manifold_counts          PrecisionRecall.compute: ball memberships    no reference class      (no gradient)
                                    and nearest-sample distances

The modules call these through ``functional`` (``qkv_attention``, ``gaussian_prior``, ``nelbo_loss``, the OT priors,
``soft_cross_entropy``, ``gaussian_blur``).
``ConvBlock`` runs its two branches and the training engine's in-place gradient slots through the packed variant of the
same kernels (``functional.conv_layers``); ``otvae::conv_bn_act`` is the single-layer functional form.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional, Tuple

import torch
from torch import Tensor

from . import _lib
from ._lib import check, ptr, stream

__all__ = ["OPS"]

OPS = ("qkv_attention", "bn_batch_stats", "conv_bn_act", "gaussian_prior", "nelbo_loss", "sinkhorn_prior", "gaussian_w2_prior",
       "soft_cross_entropy", "gaussian_blur", "sliced_w2", "mmd_prior", "ssim_loss", "ms_ssim", "sinkhorn_divergence")
_lib_def = torch.library.Library("otvae", "DEF")


def _nhwc(n, c, h, w, like, dtype=None):
    return torch.empty((n, h, w, c), device=like.device, dtype=dtype or like.dtype).permute(0, 3, 1, 2)


def _define(name: str, schema: str, impl, fake, tags=()):
    _lib_def.define(f"{name}{schema}", tags=tags)
    torch.library.impl(f"otvae::{name}", "CUDA")(impl)
    torch.library.register_fake(f"otvae::{name}")(fake)


def _refuse_second_derivative(op_name: str, what: str):
    """an Autograd kernel for a backward op too: differentiating it twice is refused aloud instead of returning a silent constant"""
    def refuse(ctx, *grads):
        raise NotImplementedError(f"otvae::{op_name} has no derivative of its own: the {what} is differentiable once")

    torch.library.register_autograd(f"otvae::{op_name}", refuse, setup_context=lambda ctx, inputs, output: None)


def _dense_or_none(gadd: Optional[Tensor]) -> Optional[Tensor]:
    """the optional ``gadd`` operand of the prior backward ops (the gradient reaching z through its other consumer), densely laid out"""
    return gadd.contiguous() if gadd is not None else None


# ------------------------------------------------------------------------------------------------ attention
def _attn_fwd(qkv: Tensor, heads: int, scale: float, need_aux: bool):
    from .functional import as_nhwc
    lib = _lib.load()
    qkv = as_nhwc(qkv)
    n, width, h, w = qkv.shape
    t, c = h * w, width // (3 * heads)
    out = _nhwc(n, heads * c, h, w, qkv)
    lse = torch.empty((n, heads, t), device=qkv.device, dtype=torch.float32)
    aux = torch.empty((n, heads, t, c * c) if (need_aux and c <= 2) else (0,), device=qkv.device, dtype=torch.float32)
    check(lib.otvae_attn_fwd_scaled(ptr(qkv), n, t, heads, c, float(scale), ptr(out), ptr(lse), ptr(aux) if aux.numel() else None,
                                    stream()), "otvae_attn_fwd")
    return out, lse, aux


def _attn_fwd_fake(qkv, heads, scale, need_aux):
    n, width, h, w = qkv.shape
    c = width // (3 * heads)
    return (_nhwc(n, heads * c, h, w, qkv), qkv.new_empty((n, heads, h * w)),
            qkv.new_empty((n, heads, h * w, c * c) if (need_aux and c <= 2) else (0,)))


def _attn_bwd(gout: Tensor, qkv: Tensor, out: Tensor, lse: Tensor, aux: Tensor, heads: int, scale: float):
    from .functional import as_nhwc
    lib = _lib.load()
    qkv = as_nhwc(qkv)
    n, width, h, w = qkv.shape
    t, c = h * w, width // (3 * heads)
    gout = as_nhwc(gout)
    gqkv = torch.empty_strided(qkv.shape, qkv.stride(), device=qkv.device, dtype=qkv.dtype)
    check(lib.otvae_attn_bwd_scaled(ptr(qkv), ptr(out), ptr(lse), ptr(gout), ptr(aux) if aux.numel() else None, n, t, heads, c,
                                    float(scale), ptr(gqkv), stream()), "otvae_attn_bwd")
    return gqkv


_define("qkv_attention", "(Tensor qkv, int heads, float scale, bool need_aux) -> (Tensor, Tensor, Tensor)", _attn_fwd, _attn_fwd_fake)
_define("qkv_attention_backward", "(Tensor gout, Tensor qkv, Tensor out, Tensor lse, Tensor aux, int heads, float scale) -> Tensor",
        _attn_bwd, lambda gout, qkv, out, lse, aux, heads, scale: torch.empty_strided(qkv.shape, qkv.stride(), device=qkv.device,
                                                                                      dtype=qkv.dtype))


def _attn_setup(ctx, inputs, output):
    qkv, heads, scale, _ = inputs
    out, lse, aux = output
    ctx.save_for_backward(qkv, out, lse, aux)
    ctx.cfg = (heads, scale)
    ctx.set_materialize_grads(False)  # lse / aux never carry a gradient: no zero-fill launches for them in every backward pass


def _attn_backward(ctx, gout, _glse, _gaux):
    if gout is None:
        return None, None, None, None
    qkv, out, lse, aux = ctx.saved_tensors
    return torch.ops.otvae.qkv_attention_backward(gout, qkv, out, lse, aux, *ctx.cfg), None, None, None


torch.library.register_autograd("otvae::qkv_attention", _attn_backward, setup_context=_attn_setup)


# ---- attention over ONE token (the AttentionBlock on a one-pixel map): the attention returns v, so the operator is the block's value
# projection and output projection (functional.one_token_forward / one_token_backward).  Its backward writes parameter gradients
# into the training engine's flat slots like functional.conv_layers does, so it is a Python formula and not a ``*_backward`` op.
def _attn_one_token_fwd(x: Tensor, wq: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], wp: Tensor, residual: Optional[Tensor]):
    from . import functional as HF
    return HF.one_token_forward(x, wq, gamma, beta, wp, residual, HF._ONE_TOKEN_CALL)


def _attn_one_token_fake(x, wq, gamma, beta, wp, residual):
    n, c, h, w = x.shape
    return _nhwc(n, c, h, w, x), _nhwc(n, c, h, w, x)


_define("qkv_attention_one_token", "(Tensor x, Tensor wq, Tensor? gamma, Tensor? beta, Tensor wp, Tensor? residual) -> (Tensor, Tensor)",
        _attn_one_token_fwd, _attn_one_token_fake)


def _attn_one_token_setup(ctx, inputs, output):
    from . import functional as HF
    ctx.save_for_backward(*inputs, output[1])
    ctx.call = HF._ONE_TOKEN_CALL
    ctx.set_materialize_grads(False)  # v is the block's inner tensor: nothing reads it outside


def _attn_one_token_backward(ctx, gy, _gv):
    if gy is None:
        return None, None, None, None, None, None
    from . import functional as HF
    return HF.one_token_backward(ctx.call, ctx.needs_input_grad[0], gy, *ctx.saved_tensors)


torch.library.register_autograd("otvae::qkv_attention_one_token", _attn_one_token_backward, setup_context=_attn_one_token_setup)


# ------------------------------------------------------------------------------------------------ ConvLayer
# Two ops, like aten's native_batch_norm split: ``bn_batch_stats`` (mutates the running buffers, not differentiable on its own)
# hands (mean, invstd, scale, shift) to the functional, differentiable ``conv_bn_act``, whose backward is the whole
# BatchNorm + activation + up-sampling + convolution adjoint.
def _bn_stats(x: Tensor, gamma: Tensor, beta: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor],
              num_batches_tracked: Optional[Tensor], training: bool):
    from . import functional as HF
    _lib.require_cuda(x, "BatchNorm input")
    br = HF.BNBranch(gamma, beta, running_mean, running_var, num_batches_tracked)
    if training:
        mean, invstd, (scale,), (shift,) = HF.bn_batch_stats(HF.as_nhwc(x), [br])
        return mean, invstd, scale, shift
    return HF.bn_eval_affine(br)


_define("bn_batch_stats", "(Tensor x, Tensor gamma, Tensor beta, Tensor(a!)? running_mean, Tensor(b!)? running_var, "
        "Tensor(c!)? num_batches_tracked, bool training) -> (Tensor, Tensor, Tensor, Tensor)", _bn_stats,
        lambda x, gamma, beta, rm, rv, nbt, training: tuple(x.new_empty(x.shape[1]) for _ in range(4)))


def _conv_fwd(x: Tensor, weight: Tensor, bias: Optional[Tensor], gamma: Optional[Tensor], beta: Optional[Tensor],
              mean: Optional[Tensor], invstd: Optional[Tensor], scale: Optional[Tensor], shift: Optional[Tensor],
              residual: Optional[Tensor], stride: int, pad: int, up: int, relu: bool, training: bool):
    from . import functional as HF
    _lib.require_cuda(x, "conv input")
    if x.dtype != torch.float32:
        raise TypeError("the MI355X conv path computes in fp32")
    x = HF.as_nhwc(x)
    wt = weight if HF.is_hwio(weight) else HF.hwio_weight(weight)
    has_norm = gamma is not None
    if has_norm and (mean is None or invstd is None or scale is None or shift is None):
        raise ValueError("conv_bn_act with a BatchNorm needs the (mean, invstd, scale, shift) of otvae::bn_batch_stats")
    spec = HF.ConvSpec(stride, pad, up, relu, has_norm, bias is not None, residual is not None, False)
    res = HF.as_nhwc(residual) if residual is not None else None
    (y,), _, _ = HF.conv_forward_launch(x, (spec,), (mean, invstd, [scale], [shift], training), (wt, bias, gamma, beta, res))
    return y


def _conv_fwd_fake(x, weight, bias, gamma, beta, mean, invstd, scale, shift, residual, stride, pad, up, relu, training):
    kh, kw = weight.shape[2], weight.shape[3]
    ho, wo = (x.shape[2] * up + 2 * pad - kh) // stride + 1, (x.shape[3] * up + 2 * pad - kw) // stride + 1
    return _nhwc(x.shape[0], weight.shape[0], ho, wo, x)


def _conv_bwd(gy: Tensor, x: Tensor, weight: Tensor, gamma: Optional[Tensor], mean: Optional[Tensor], invstd: Optional[Tensor],
              scale: Optional[Tensor], shift: Optional[Tensor], stride: int, pad: int, up: int, relu: bool, has_bias: bool,
              has_residual: bool, training: bool, need_dx: bool):
    from . import functional as HF
    x = HF.as_nhwc(x)
    wt = weight if HF.is_hwio(weight) else HF.hwio_weight(weight)
    has_norm = gamma is not None
    spec = HF.ConvSpec(stride, pad, up, relu, has_norm, has_bias, has_residual, False)
    g, _, _ = HF._geom(x, wt, stride, pad, up)
    bias_like = x.new_empty(weight.shape[0]) if has_bias else None
    dx, ((gw, gb, dgam, dbet, _),) = HF.conv_backward_launch(x, (wt, bias_like, gamma, gamma, None), (spec,), [g],
                                                            (mean, invstd, [scale], [shift], training), ((None, None, None, None),),
                                                            (gy,), need_dx)
    e = x.new_empty(0)
    return (dx if dx is not None else e), gw, (gb if gb is not None else e), (dgam if dgam is not None else e), \
        (dbet if dbet is not None else e)


def _conv_bwd_fake(gy, x, weight, gamma, mean, invstd, scale, shift, stride, pad, up, relu, has_bias, has_residual, training,
                   need_dx):
    e = x.new_empty(0)
    return (torch.empty_strided(x.shape, x.stride(), device=x.device, dtype=x.dtype) if need_dx else e, torch.empty_like(weight),
            x.new_empty(weight.shape[0]) if has_bias else e, x.new_empty(x.shape[1]) if gamma is not None else e,
            x.new_empty(x.shape[1]) if gamma is not None else e)


_define("conv_bn_act",
        "(Tensor x, Tensor weight, Tensor? bias, Tensor? gamma, Tensor? beta, Tensor? mean, Tensor? invstd, Tensor? scale, "
        "Tensor? shift, Tensor? residual, int stride, int pad, int up, bool relu, bool training) -> Tensor", _conv_fwd, _conv_fwd_fake)
_define("conv_bn_act_backward",
        "(Tensor gy, Tensor x, Tensor weight, Tensor? gamma, Tensor? mean, Tensor? invstd, Tensor? scale, Tensor? shift, int stride, "
        "int pad, int up, bool relu, bool has_bias, bool has_residual, bool training, bool need_dx) -> "
        "(Tensor, Tensor, Tensor, Tensor, Tensor)", _conv_bwd, _conv_bwd_fake)


def _conv_setup(ctx, inputs, output):
    x, weight, bias, gamma, beta, mean, invstd, scale, shift, residual, stride, pad, up, relu, training = inputs
    ctx.save_for_backward(x, weight, gamma, mean, invstd, scale, shift)
    ctx.cfg = (stride, pad, up, relu, bias is not None, residual is not None, training)


def _conv_backward(ctx, gy):
    x, weight, gamma, mean, invstd, scale, shift = ctx.saved_tensors
    stride, pad, up, relu, has_bias, has_res, training = ctx.cfg
    need_dx = ctx.needs_input_grad[0]
    dx, gw, gb, dgam, dbet = torch.ops.otvae.conv_bn_act_backward(gy, x, weight, gamma, mean, invstd, scale, shift, stride, pad, up,
                                                                  relu, has_bias, has_res, training, need_dx)
    none = lambda t: t if t.numel() else None  # noqa: E731
    return (none(dx) if need_dx else None, gw, none(gb), none(dgam), none(dbet), None, None, None, None, gy if has_res else None,
            None, None, None, None, None)


torch.library.register_autograd("otvae::conv_bn_act", _conv_backward, setup_context=_conv_setup)


# ------------------------------------------------------------------------------------------------ GaussianPrior
def _gp_fwd(h: Tensor, eps: Tensor, coeff: float):
    lib = _lib.load()
    b, c2, hh, ww = h.shape
    d, s = c2 // 2, hh * ww
    z = _nhwc(b, d, hh, ww, h)
    loss = torch.empty(b, device=h.device, dtype=torch.float32)
    check(lib.otvae_gaussian_prior_fwd(ptr(h), ptr(eps), None, None, None, b, s, d, float(coeff), 0, ptr(z), ptr(loss), stream()),
          "otvae_gaussian_prior_fwd")
    return z, loss


def _gp_bwd(h: Tensor, eps: Tensor, gz: Optional[Tensor], gloss: Optional[Tensor], coeff: float):
    from .functional import as_nhwc
    lib = _lib.load()
    b, c2, hh, ww = h.shape
    d, s = c2 // 2, hh * ww
    gz = as_nhwc(gz) if gz is not None else None
    gloss = gloss.contiguous() if gloss is not None else None
    gh = torch.empty_strided(h.shape, h.stride(), device=h.device, dtype=h.dtype)
    check(lib.otvae_gaussian_prior_bwd(ptr(h), ptr(eps), None, None, None, ptr(gz), ptr(gloss), b, s, d, float(coeff), 0, ptr(gh),
                                       None, None, stream()), "otvae_gaussian_prior_bwd")
    return gh


_define("gaussian_prior", "(Tensor h, Tensor eps, float coeff) -> (Tensor, Tensor)", _gp_fwd,
        lambda h, eps, coeff: (_nhwc(h.shape[0], h.shape[1] // 2, h.shape[2], h.shape[3], h), h.new_empty(h.shape[0])))
_define("gaussian_prior_backward", "(Tensor h, Tensor eps, Tensor? gz, Tensor? gloss, float coeff) -> Tensor", _gp_bwd,
        lambda h, eps, gz, gloss, coeff: torch.empty_strided(h.shape, h.stride(), device=h.device, dtype=h.dtype))


def _gp_setup(ctx, inputs, output):
    h, eps, coeff = inputs
    ctx.save_for_backward(h, eps)
    ctx.coeff = coeff
    ctx.set_materialize_grads(False)  # gz / gloss are optional arguments of the backward kernel


def _gp_backward(ctx, gz, gloss):
    if gz is None and gloss is None:
        return None, None, None
    h, eps = ctx.saved_tensors
    return torch.ops.otvae.gaussian_prior_backward(h, eps, gz, gloss, ctx.coeff), None, None


torch.library.register_autograd("otvae::gaussian_prior", _gp_backward, setup_context=_gp_setup)


# ------------------------------------------------------------------------------------------------ nelbo reduction
def _nelbo_fwd(pred: Tensor, target: Tensor, prior_loss: Optional[Tensor], chw: float):
    from .functional import PriorLane
    if PriorLane.is_open(pred.device) and PriorLane.active(pred.device):
        # the prior term is still being computed on the prior lane (functional.PriorLane): the loss vector is formed there too,
        # behind it -- the backward pass needs pred and target, not this value (ordered behind the lane's work, not the side stream's)
        return PriorLane.issue(pred.device, lambda: _nelbo_fwd_launch(pred, target, prior_loss, chw, allow_defer=False),
                               pred, target, prior_loss)
    return _nelbo_fwd_launch(pred, target, prior_loss, chw)


def _nelbo_fwd_launch(pred: Tensor, target: Tensor, prior_loss: Optional[Tensor], chw: float, allow_defer: bool = True):
    from .functional import _PendingReduce
    lib = _lib.load()
    numel = pred.numel()
    # the prior term is a mean over ITS entries: one per latent the prior saw = expansion * batch (model/vae.py:165-169), which is
    # the batch of `pred` (the mean over the replicas) only when expansion = 1
    n_prior = prior_loss.numel() if prior_loss is not None else pred.shape[0]
    if prior_loss is not None:
        prior_loss = prior_loss.contiguous()
    ws = torch.empty(lib.otvae_nelbo_ws(), device=pred.device, dtype=torch.float64)
    out = torch.empty(3, device=pred.device, dtype=torch.float32)

    def launch():
        check(lib.otvae_nelbo_fwd(ptr(pred), ptr(target), numel, ptr(prior_loss), n_prior, float(chw), ptr(ws), ptr(out), stream()),
              "otvae_nelbo_fwd")

    # inside a training engine's captured step the loss VALUE goes to the side stream with the backward pass's first weight-gradient
    # fork: the backward pass needs pred and target, not this value (functional._PendingReduce.defer_to_side)
    if not (allow_defer and _PendingReduce.defer_to_side(pred.device, launch, pred, target, prior_loss, ws, out)):
        launch()
    return out


def _nelbo_bwd(gout: Tensor, pred: Tensor, target: Tensor, n_prior: int, chw: float):
    lib = _lib.load()
    numel = pred.numel()
    gout = gout.contiguous()
    gpred = torch.empty_strided(pred.shape, pred.stride(), device=pred.device, dtype=pred.dtype)
    gprior = torch.empty(n_prior, device=pred.device, dtype=torch.float32)
    check(lib.otvae_nelbo_bwd(ptr(pred), ptr(target), numel, max(n_prior, 1), float(chw), ptr(gout), ptr(gpred),
                              ptr(gprior) if n_prior else None, stream()), "otvae_nelbo_bwd")
    return gpred, gprior


_define("nelbo_loss", "(Tensor pred, Tensor target, Tensor? prior_loss, float chw) -> Tensor", _nelbo_fwd,
        lambda pred, target, prior_loss, chw: pred.new_empty(3))
_define("nelbo_loss_backward", "(Tensor gout, Tensor pred, Tensor target, int n_prior, float chw) -> (Tensor, Tensor)", _nelbo_bwd,
        lambda gout, pred, target, n_prior, chw: (torch.empty_strided(pred.shape, pred.stride(), device=pred.device, dtype=pred.dtype),
                                                  pred.new_empty(n_prior)))


def _nelbo_setup(ctx, inputs, output):
    pred, target, prior_loss, chw = inputs
    ctx.save_for_backward(pred, target)
    ctx.cfg = (0 if prior_loss is None else prior_loss.numel(), tuple(prior_loss.shape) if prior_loss is not None else None, chw)


def _nelbo_backward(ctx, gout):
    pred, target = ctx.saved_tensors
    n_prior, pshape, chw = ctx.cfg
    gpred, gprior = torch.ops.otvae.nelbo_loss_backward(gout, pred, target, n_prior, chw)
    return gpred, None, (gprior.reshape(pshape) if n_prior else None), None


torch.library.register_autograd("otvae::nelbo_loss", _nelbo_backward, setup_context=_nelbo_setup)


# ------------------------------------------------------------------------------------------------ minibatch-OT prior
def _sk_fwd(z: Tensor, y: Tensor, reg: float, max_iter: int, threshold: float, scale: float):
    lib = _lib.load()
    _lib.require_cuda(z, "latents")
    if z.dtype not in (torch.float32, torch.float64):
        raise TypeError("SinkhornPrior computes in float32 or float64")
    z, y = z.contiguous(), y.to(z.dtype).contiguous()
    (n, d), m = z.shape, y.shape[0]
    if y.shape[1] != d:
        raise ValueError(f"prior samples have {y.shape[1]} dimensions, latents {d}")
    dt = 0 if z.dtype == torch.float32 else 1
    new = lambda *shape: torch.empty(shape, device=z.device, dtype=z.dtype)  # noqa: E731
    C, pi, u, v, cost, cmax = new(n, m), new(n, m), new(n), new(m), new(n), new(1)   # cost: one entry per sample
    ws = torch.empty(lib.otvae_sinkhorn_prior_ws(dt, n, m), device=z.device, dtype=torch.uint8)
    iters = torch.empty(1, device=z.device, dtype=torch.int32)
    check(lib.otvae_sinkhorn_prior_fwd(dt, ptr(z), ptr(y), n, m, d, float(reg), int(max_iter), float(threshold), float(scale), n,
                                       ptr(ws), ptr(C), ptr(pi), ptr(u), ptr(v), ptr(cost), ptr(cmax), ptr(iters), stream()),
          "otvae_sinkhorn_prior_fwd")
    return cost, pi, iters


def _sk_bwd(g: Tensor, gadd: Optional[Tensor], z: Tensor, y: Tensor, pi: Tensor, scale: float):
    z, y = z.contiguous(), y.to(z.dtype).contiguous()
    n, d = z.shape
    gz = torch.empty_like(z)
    gadd = _dense_or_none(gadd)
    check(_lib.load().otvae_ot_cost_grad(0 if z.dtype == torch.float32 else 1, ptr(z), ptr(y), ptr(pi), ptr(g.contiguous()), g.numel(),
                                         float(scale), ptr(gadd), n, y.shape[0], d, ptr(gz), stream()), "otvae_ot_cost_grad")
    return gz


_define("sinkhorn_prior", "(Tensor z, Tensor y, float reg, int max_iter, float threshold, float scale) -> (Tensor, Tensor, Tensor)",
        _sk_fwd, lambda z, y, reg, max_iter, threshold, scale: (z.new_empty(z.shape[0]), z.new_empty(z.shape[0], y.shape[0]),
                                                               z.new_empty(1, dtype=torch.int32)))
_define("sinkhorn_prior_backward", "(Tensor g, Tensor? gadd, Tensor z, Tensor y, Tensor pi, float scale) -> Tensor", _sk_bwd,
        lambda g, gadd, z, y, pi, scale: torch.empty_like(z))


def _sk_setup(ctx, inputs, output):
    z, y, _, _, _, scale = inputs
    ctx.save_for_backward(z, y, output[1])
    ctx.scale = scale
    ctx.set_materialize_grads(False)


def _sk_backward(ctx, g, _gpi, _giters):
    z, y, pi = ctx.saved_tensors
    if g is None:
        return None, None, None, None, None, None
    return torch.ops.otvae.sinkhorn_prior_backward(g, None, z, y, pi, ctx.scale), None, None, None, None, None


torch.library.register_autograd("otvae::sinkhorn_prior", _sk_backward, setup_context=_sk_setup)


# ------------------------------------------------------------------------------------------------ Sinkhorn divergence prior
def sinkhorn_div_check(z: Tensor, y: Tensor, reg: float, max_iter: int) -> None:
    """the refusals of ``otvae::sinkhorn_divergence``, before any kernel (also called by ``SinkhornDivergencePrior`` and
    ``ot.sinkhorn_divergence``)"""
    if z.dim() != 2 or y.dim() != 2:
        raise ValueError(f"sinkhorn_divergence takes z [N, D] and y [M, D]; got {tuple(z.shape)}, {tuple(y.shape)}")
    if y.shape[1] != z.shape[1]:
        raise ValueError(f"sinkhorn_divergence: prior samples are {tuple(y.shape)}, latents {tuple(z.shape)}: the widths D differ")
    if z.shape[0] < 1 or y.shape[0] < 1 or z.shape[1] < 1:
        raise ValueError(f"sinkhorn_divergence needs N, M, D >= 1, got N = {z.shape[0]}, M = {y.shape[0]}, D = {z.shape[1]}")
    if not float(reg) > 0:
        raise ValueError(f"sinkhorn_divergence: reg must be positive, got {reg!r}")
    if int(max_iter) < 0:
        raise ValueError(f"sinkhorn_divergence: max_iter must not be negative, got {max_iter!r}")
    if z.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"sinkhorn_divergence computes in float32 or float64, got {z.dtype} latents")
    _lib.require_cuda(z, "latents")
    _lib.require_cuda(y, "prior samples")


def _sd_fwd(z: Tensor, y: Tensor, reg: float, max_iter: int, scale: float):
    sinkhorn_div_check(z, y, reg, max_iter)
    lib = _lib.load()
    z, y = z.contiguous(), y.to(z.dtype).contiguous()
    (n, d), m = z.shape, y.shape[0]
    dt = 0 if z.dtype == torch.float32 else 1
    nbytes = lib.otvae_sinkhorn_div_ws(dt, n, m)
    if nbytes < 0:
        raise NotImplementedError(f"sinkhorn_divergence is built for N, M <= 32768, got N = {n}, M = {m}")
    new = lambda *shape: torch.empty(shape, device=z.device, dtype=z.dtype)  # noqa: E731
    loss, pi_zy, pi_zz = new(n), new(n, m), new(n, n)   # loss: one entry per sample
    terms = torch.empty(3, device=z.device, dtype=torch.float64)
    iters = torch.empty(1, device=z.device, dtype=torch.int32)
    ws = torch.empty(nbytes, device=z.device, dtype=torch.uint8)
    check(lib.otvae_sinkhorn_div_fwd(dt, ptr(z), ptr(y), n, m, d, float(reg), int(max_iter), float(scale), -1, ptr(ws), ptr(loss),
                                     ptr(terms), ptr(pi_zy), ptr(pi_zz), ptr(iters), stream()), "otvae_sinkhorn_div_fwd")
    return loss, terms, pi_zy, pi_zz, iters


def _sd_bwd(g: Tensor, gadd: Optional[Tensor], z: Tensor, y: Tensor, pi_zy: Tensor, pi_zz: Tensor, scale: float):
    z, y = z.contiguous(), y.to(z.dtype).contiguous()
    n, d = z.shape
    gz = torch.empty_like(z)
    gadd = _dense_or_none(gadd)
    check(_lib.load().otvae_sinkhorn_div_grad(0 if z.dtype == torch.float32 else 1, ptr(z), ptr(y), ptr(pi_zy.contiguous()),
                                              ptr(pi_zz.contiguous()), ptr(g.to(z.dtype).contiguous()), g.numel(), float(scale), ptr(gadd),
                                              n, y.shape[0], d, ptr(gz), stream()), "otvae_sinkhorn_div_grad")
    return gz


_define("sinkhorn_divergence", "(Tensor z, Tensor y, float reg, int max_iter, float scale) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
        _sd_fwd, lambda z, y, reg, max_iter, scale: (z.new_empty(z.shape[0]), z.new_empty(3, dtype=torch.float64),
                                                     z.new_empty(z.shape[0], y.shape[0]), z.new_empty(z.shape[0], z.shape[0]),
                                                     z.new_empty(1, dtype=torch.int32)))
_define("sinkhorn_divergence_backward", "(Tensor g, Tensor? gadd, Tensor z, Tensor y, Tensor pi_zy, Tensor pi_zz, float scale) -> Tensor",
        _sd_bwd, lambda g, gadd, z, y, pi_zy, pi_zz, scale: torch.empty_like(z))


def _sd_setup(ctx, inputs, output):
    z, y, _, _, scale = inputs
    ctx.save_for_backward(z, y, output[2], output[3])
    ctx.scale = scale
    ctx.set_materialize_grads(False)   # terms / plans / iters never carry a gradient


def _sd_backward(ctx, g, *_):
    if g is None:
        return None, None, None, None, None
    z, y, pi_zy, pi_zz = ctx.saved_tensors
    return torch.ops.otvae.sinkhorn_divergence_backward(g, None, z, y, pi_zy, pi_zz, ctx.scale), None, None, None, None


torch.library.register_autograd("otvae::sinkhorn_divergence", _sd_backward, setup_context=_sd_setup)
_refuse_second_derivative("sinkhorn_divergence_backward", "Sinkhorn divergence prior")


# ------------------------------------------------------------------------------------------------ sliced W2 prior
def _sw_fwd(z: Tensor, y: Tensor, dirs: Tensor, scale: float):
    lib = _lib.load()
    _lib.require_cuda(z, "latents")
    if z.dtype != torch.float32:
        raise NotImplementedError(f"sliced_w2 computes in float32, got {z.dtype} latents")
    if z.dim() != 2 or y.dim() != 2 or dirs.dim() != 2:
        raise ValueError(f"sliced_w2 takes z [N, D], y [N, D], dirs [L, D]; got {tuple(z.shape)}, {tuple(y.shape)}, {tuple(dirs.shape)}")
    n, d = z.shape
    if tuple(y.shape) != (n, d):
        raise ValueError(f"prior samples are {tuple(y.shape)}, latents {(n, d)}: sliced_w2 pairs sorted projections one to one")
    if dirs.shape[1] != d or dirs.shape[0] < 1:
        raise ValueError(f"projection directions are {tuple(dirs.shape)}, expected [L >= 1, {d}]")
    z, y, dirs = z.contiguous(), y.to(z.dtype).contiguous(), dirs.to(z.dtype).contiguous()
    nl = dirs.shape[0]
    nbytes = lib.otvae_sliced_w2_ws(n, nl)
    if nbytes < 0:
        raise NotImplementedError(f"sliced_w2 sorts 1 <= N <= 4096 rows per projection in LDS, got N = {n}")
    ws = torch.empty(nbytes, device=z.device, dtype=torch.uint8)
    loss = torch.empty(n, device=z.device, dtype=torch.float32)   # one entry per sample
    resid = torch.empty((nl, n), device=z.device, dtype=torch.float32)
    theta = torch.empty((nl, d), device=z.device, dtype=torch.float32)
    check(lib.otvae_sliced_w2_fwd(ptr(z), ptr(y), ptr(dirs), n, d, nl, float(scale), n, ptr(ws), ptr(theta), ptr(resid), ptr(loss),
                                  stream()), "otvae_sliced_w2_fwd")
    return loss, resid, theta


def _sw_bwd(g: Tensor, gadd: Optional[Tensor], resid: Tensor, theta: Tensor, scale: float):
    nl, n = resid.shape
    d = theta.shape[1]
    gz = torch.empty((n, d), device=resid.device, dtype=torch.float32)
    gadd = _dense_or_none(gadd)
    check(_lib.load().otvae_sliced_w2_bwd(ptr(g.float().contiguous()), ptr(gadd), ptr(resid.contiguous()), ptr(theta.contiguous()), n, d, nl,
                                          float(scale), ptr(gz), stream()), "otvae_sliced_w2_bwd")
    return gz


_define("sliced_w2", "(Tensor z, Tensor y, Tensor dirs, float scale) -> (Tensor, Tensor, Tensor)", _sw_fwd,
        lambda z, y, dirs, scale: (z.new_empty(z.shape[0]), z.new_empty(dirs.shape[0], z.shape[0]), z.new_empty(dirs.shape[0], z.shape[1])))
_define("sliced_w2_backward", "(Tensor g, Tensor? gadd, Tensor resid, Tensor theta, float scale) -> Tensor", _sw_bwd,
        lambda g, gadd, resid, theta, scale: resid.new_empty(resid.shape[1], theta.shape[1]))


def _sw_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1], output[2])
    ctx.scale = inputs[3]
    ctx.set_materialize_grads(False)   # resid / theta never carry a gradient


def _sw_backward(ctx, g, _gresid, _gtheta):
    if g is None:
        return None, None, None, None
    resid, theta = ctx.saved_tensors
    return torch.ops.otvae.sliced_w2_backward(g, None, resid, theta, ctx.scale), None, None, None


torch.library.register_autograd("otvae::sliced_w2", _sw_backward, setup_context=_sw_setup)
_refuse_second_derivative("sliced_w2_backward", "sliced W2 prior")


# ------------------------------------------------------------------------------------------------ MMD prior
MMD_KERNELS = {"imq": 0, "rbf": 1}
MMD_MAX_SCALES = 8
MMD_MAX_D = 512   # csrc/mmd.hip: the gradient accumulators of a 32-row tile stay in registers, both staged tiles in LDS


def mmd_kernel_id(kernel) -> int:
    if not isinstance(kernel, str) or kernel not in MMD_KERNELS:
        raise ValueError(f"mmd: unknown kernel {kernel!r}, expected one of {sorted(MMD_KERNELS)}")
    return MMD_KERNELS[kernel]


def mmd_check_config(scales, sigma2) -> Tuple[float, ...]:
    """the scales as a tuple of floats; ValueError for none, more than 8, a non-positive one or a non-positive sigma2"""
    try:
        scales = tuple(float(s) for s in scales)
    except TypeError:
        raise ValueError(f"mmd: scales must be a sequence of positive numbers, got {scales!r}") from None
    if not 1 <= len(scales) <= MMD_MAX_SCALES:
        raise ValueError(f"mmd: 1 to {MMD_MAX_SCALES} scales, got {len(scales)}")
    if not all(s > 0 and s == s and s != float("inf") for s in scales):
        raise ValueError(f"mmd: every scale must be positive and finite, got {scales}")
    if not (float(sigma2) > 0 and float(sigma2) != float("inf")):
        raise ValueError(f"mmd: sigma2 must be positive and finite, got {sigma2!r}")
    return scales


def mmd_check_inputs(z: Tensor, y: Tensor, unbiased: bool) -> None:
    """the shape / dtype refusals of ``otvae::mmd_prior``, before any kernel (also called by ``MMDPrior`` and ``ot.mmd2``)"""
    if z.dim() != 2 or y.dim() != 2:
        raise ValueError(f"mmd takes z [N, D] and y [M, D]; got {tuple(z.shape)}, {tuple(y.shape)}")
    if y.shape[1] != z.shape[1]:
        raise ValueError(f"mmd: prior samples are {tuple(y.shape)}, latents {tuple(z.shape)}: the widths D differ")
    least = 2 if unbiased else 1
    if z.shape[0] < least or y.shape[0] < least or z.shape[1] < 1:
        raise ValueError(f"mmd: the {'unbiased' if unbiased else 'biased'} estimator needs N, M >= {least} and D >= 1, got N = "
                         f"{z.shape[0]}, M = {y.shape[0]}, D = {z.shape[1]}")
    if z.dtype != torch.float32:
        raise NotImplementedError(f"mmd computes in float32, got {z.dtype} latents")


def _mmd_fwd(z: Tensor, y: Tensor, kernel: int, scales, sigma2: float, unbiased: bool, scale: float, need_grad: bool):
    if kernel not in (0, 1):
        raise ValueError(f"mmd: kernel id must be 0 (imq) or 1 (rbf), got {kernel}")
    scales = mmd_check_config(scales, sigma2)
    mmd_check_inputs(z, y, unbiased)
    _lib.require_cuda(z, "latents")
    lib = _lib.load()
    n, d = z.shape
    m = y.shape[0]
    nbytes = lib.otvae_mmd_ws(n, m, d)
    if nbytes < 0:
        raise NotImplementedError(f"mmd_prior is built for 1 <= D <= {MMD_MAX_D} (N D, M D below 2^31), got N = {n}, M = {m}, D = {d}")
    z, y = z.contiguous(), y.to(z.dtype).contiguous()
    ws = torch.empty(nbytes, device=z.device, dtype=torch.uint8)
    loss = torch.empty(n, device=z.device, dtype=torch.float32)   # one entry per sample
    terms = torch.empty(3, device=z.device, dtype=torch.float32)
    G = torch.empty((n if need_grad else 0, d), device=z.device, dtype=torch.float32)
    sc = (C.c_double * len(scales))(*scales)   # read by the call itself: a captured graph holds the constants by value
    check(lib.otvae_mmd_fwd(ptr(z), ptr(y), n, m, d, int(kernel), sc, len(scales), float(sigma2), int(bool(unbiased)), float(scale), n,
                            ptr(ws), ptr(loss), ptr(terms), ptr(G) if need_grad else None, stream()), "otvae_mmd_fwd")
    return loss, G, terms


def _mmd_bwd(g: Tensor, gadd: Optional[Tensor], G: Tensor):
    n, d = G.shape
    if n < 1:
        raise ValueError("mmd_prior_backward: the forward ran with need_grad=False and kept no gradient")
    gz = torch.empty((n, d), device=G.device, dtype=torch.float32)
    g = g.float().contiguous()
    gadd = _dense_or_none(gadd)
    check(_lib.load().otvae_mmd_bwd(ptr(g), g.numel(), ptr(gadd), ptr(G.contiguous()), n, d, ptr(gz), stream()), "otvae_mmd_bwd")
    return gz


_define("mmd_prior", "(Tensor z, Tensor y, int kernel, float[] scales, float sigma2, bool unbiased, float scale, bool need_grad) -> "
        "(Tensor, Tensor, Tensor)", _mmd_fwd,
        lambda z, y, kernel, scales, sigma2, unbiased, scale, need_grad: (z.new_empty(z.shape[0]),
                                                                          z.new_empty(z.shape[0] if need_grad else 0, z.shape[1]),
                                                                          z.new_empty(3)))
_define("mmd_prior_backward", "(Tensor g, Tensor? gadd, Tensor G) -> Tensor", _mmd_bwd, lambda g, gadd, G: G.new_empty(G.shape))


def _mmd_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.need_grad = inputs[7]
    ctx.set_materialize_grads(False)   # G / terms never carry a gradient


def _mmd_backward(ctx, g, _gG, _gterms):
    if g is None:
        return (None,) * 8
    if not ctx.need_grad:
        raise RuntimeError("otvae::mmd_prior ran with need_grad=False: it kept no gradient to propagate")
    (G,) = ctx.saved_tensors
    return (torch.ops.otvae.mmd_prior_backward(g, None, G),) + (None,) * 7


torch.library.register_autograd("otvae::mmd_prior", _mmd_backward, setup_context=_mmd_setup)
_refuse_second_derivative("mmd_prior_backward", "MMD prior")


# ------------------------------------------------------------------------------------------------ Gaussian W2 prior
def _w2_fwd(z: Tensor, mut: Optional[Tensor], covt: Optional[Tensor], rt: Optional[Tensor], v_init: Optional[Tensor],
            warm: Optional[Tensor], scale: float):
    from .ot import matrix_utils as MU
    lib = _lib.load()
    _lib.require_cuda(z, "latents")
    if z.dtype not in (torch.float32, torch.float64):
        raise TypeError("GaussianW2Prior takes float32 or float64 latents")
    z = z.contiguous()
    b, d = z.shape
    dev = z.device
    f64 = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float64)  # noqa: E731
    n, sx, sxx = f64(1), f64(1, d), f64(1, d, d)
    ws = torch.empty(max(8, lib.otvae_gauss_stats_ws(1, b, d, 0)), device=dev, dtype=torch.uint8)
    check(lib.otvae_gauss_stats(0 if z.dtype == torch.float32 else 1, ptr(z), 1, b, d, 0, 0, -1.0, ptr(ws), ptr(n), ptr(sx), ptr(sxx),
                                stream()), "otvae_gauss_stats")
    mu, cov = f64(1, d), f64(1, d, d)
    check(lib.otvae_mean_cov(ptr(n), ptr(sx), ptr(sxx), 1, d, 0, ptr(mu), ptr(cov), stream()), "otvae_mean_cov")
    m = cov if rt is None else MU.matmul64(MU.matmul64(rt, cov), rt)
    lam, vt = f64(1, d), f64(1, d, d)
    ews = torch.empty(lib.otvae_eigh_ws(1, d), device=dev, dtype=torch.uint8)
    if v_init is not None:  # the previous step's eigenvectors as the start basis (2-4 sweeps instead of ~9)
        g0 = f64(1, d, d)
        check(lib.otvae_eigh_fn_warm(ptr(m), ptr(v_init), ptr(warm), 1, d, 3, ptr(vt), ptr(lam), ptr(ews), ptr(g0), stream()),
              "otvae_eigh_fn_warm")
    else:
        check(lib.otvae_eigh_fn(ptr(m), 1, d, 3, ptr(vt), ptr(lam), ptr(ews), stream()), "otvae_eigh_fn")
    loss = torch.empty(b, device=dev, dtype=torch.float32)
    q = f64(d, d)
    check(lib.otvae_w2_prior_tail(ptr(mu), ptr(mut), ptr(cov), ptr(covt), ptr(lam), ptr(vt), d, float(scale), b, ptr(loss), ptr(q),
                                  stream()), "otvae_w2_prior_tail")
    return loss, mu, q, vt


def _w2_bwd(g: Tensor, gadd: Optional[Tensor], z: Tensor, mu: Tensor, q: Tensor, mut: Optional[Tensor], rt: Optional[Tensor],
            scale: float):
    from .ot import matrix_utils as MU
    lib = _lib.load()
    z = z.contiguous()
    b, d = z.shape
    w = MU.matmul64(q, q, trans_a=True)                          # M^-1/2
    if rt is not None:
        w = MU.matmul64(MU.matmul64(rt, w), rt)                  # covt^1/2 M^-1/2 covt^1/2
    gz = torch.empty_like(z)
    gadd = _dense_or_none(gadd)
    check(lib.otvae_w2_prior_bwd(0 if z.dtype == torch.float32 else 1, ptr(z), b, d, ptr(mu), ptr(mut), ptr(w),
                                 ptr(g.float().contiguous()), g.numel(), float(scale), ptr(gadd), ptr(gz), stream()),
          "otvae_w2_prior_bwd")
    return gz


_define("gaussian_w2_prior", "(Tensor z, Tensor? target_mean, Tensor? target_cov, Tensor? target_root, Tensor? v_init, Tensor? warm, "
        "float scale) -> (Tensor, Tensor, Tensor, Tensor)", _w2_fwd,
        lambda z, mut, covt, rt, v_init, warm, scale: (z.new_empty(z.shape[0], dtype=torch.float32),
                                                       z.new_empty((1, z.shape[1]), dtype=torch.float64),
                                                       z.new_empty((z.shape[1], z.shape[1]), dtype=torch.float64),
                                                       z.new_empty((1, z.shape[1], z.shape[1]), dtype=torch.float64)))
_define("gaussian_w2_prior_backward", "(Tensor g, Tensor? gadd, Tensor z, Tensor mu, Tensor q, Tensor? target_mean, "
        "Tensor? target_root, float scale) -> Tensor", _w2_bwd, lambda g, gadd, z, mu, q, mut, rt, scale: torch.empty_like(z))


def _w2_setup(ctx, inputs, output):
    z, mut, _, rt, _, _, scale = inputs
    ctx.save_for_backward(z, output[1], output[2], mut, rt)
    ctx.scale = scale
    ctx.set_materialize_grads(False)


def _w2_backward(ctx, g, _gmu, _gq, _gvt):
    z, mu, q, mut, rt = ctx.saved_tensors
    if g is None:
        return None, None, None, None, None, None, None
    return torch.ops.otvae.gaussian_w2_prior_backward(g, None, z, mu, q, mut, rt, ctx.scale), None, None, None, None, None, None


torch.library.register_autograd("otvae::gaussian_w2_prior", _w2_backward, setup_context=_w2_setup)


# ------------------------------------------------------------------------------------------------ DAD's shifted soft-label CE
def _rows_k(t: Tensor, name: str) -> Tensor:
    """[B, T, K] fp32 on the device with rows of K contiguous values (any batch / token strides: a transposed view is read in place)"""
    _lib.require_cuda(t, name)
    if t.dim() != 3 or t.dtype != torch.float32:
        raise ValueError(f"soft_cross_entropy takes float32 [B, T, K] tensors, got {name} {tuple(t.shape)} {t.dtype}")
    if t.stride(2) != 1:
        t = t.contiguous()
    return t


def _sce_fwd(logits: Tensor, probs: Tensor):
    lib = _lib.load()
    logits, probs = _rows_k(logits, "logits"), _rows_k(probs, "probs")
    if logits.shape != probs.shape:
        raise ValueError(f"soft_cross_entropy: logits {tuple(logits.shape)} and probs {tuple(probs.shape)} differ in shape")
    b, t, k = logits.shape
    loss = torch.empty(b, device=logits.device, dtype=torch.float32)
    lse = torch.empty((b, t), device=logits.device, dtype=torch.float32)
    psum = torch.empty((b, t), device=logits.device, dtype=torch.float32)
    ws = torch.empty(max(1, lib.otvae_soft_ce_ws(b, t) // 8), device=logits.device, dtype=torch.float64)
    check(lib.otvae_soft_ce_fwd(ptr(logits), logits.stride(0), logits.stride(1), ptr(probs), probs.stride(0), probs.stride(1), b, t, k,
                                ptr(loss), ptr(lse), ptr(psum), ptr(ws), stream()), "otvae_soft_ce_fwd")
    return loss, lse, psum


def _sce_bwd(gloss: Tensor, logits: Tensor, probs: Tensor, lse: Tensor, psum: Tensor, need_dlogits: bool, need_dprobs: bool):
    lib = _lib.load()
    logits, probs = _rows_k(logits, "logits"), _rows_k(probs, "probs")
    b, t, k = logits.shape
    e = logits.new_empty(0)
    dl = torch.empty((b, t, k), device=logits.device, dtype=torch.float32) if need_dlogits else None
    dp = torch.empty((b, t, k), device=logits.device, dtype=torch.float32) if need_dprobs else None
    check(lib.otvae_soft_ce_bwd(ptr(logits), logits.stride(0), logits.stride(1), ptr(probs), probs.stride(0), probs.stride(1),
                                ptr(lse.contiguous()), ptr(psum.contiguous()), ptr(gloss.float().contiguous()), b, t, k, ptr(dl), ptr(dp),
                                stream()), "otvae_soft_ce_bwd")
    return (dl if dl is not None else e), (dp if dp is not None else e)


_define("soft_cross_entropy", "(Tensor logits, Tensor probs) -> (Tensor, Tensor, Tensor)", _sce_fwd,
        lambda logits, probs: (logits.new_empty(logits.shape[0]), logits.new_empty(logits.shape[:2]), logits.new_empty(logits.shape[:2])))
_define("soft_cross_entropy_backward", "(Tensor gloss, Tensor logits, Tensor probs, Tensor lse, Tensor psum, bool need_dlogits, "
        "bool need_dprobs) -> (Tensor, Tensor)", _sce_bwd,
        lambda gloss, logits, probs, lse, psum, need_dlogits, need_dprobs: (
            logits.new_empty(tuple(logits.shape) if need_dlogits else (0,)), logits.new_empty(tuple(logits.shape) if need_dprobs else (0,))))


def _sce_setup(ctx, inputs, output):
    logits, probs = inputs
    ctx.save_for_backward(logits, probs, output[1], output[2])
    ctx.set_materialize_grads(False)  # lse / psum never carry a gradient


def _sce_backward(ctx, gloss, _glse, _gpsum):
    need_dl, need_dp = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if gloss is None or not (need_dl or need_dp):
        return None, None
    logits, probs, lse, psum = ctx.saved_tensors
    dl, dp = torch.ops.otvae.soft_cross_entropy_backward(gloss, logits, probs, lse, psum, need_dl, need_dp)
    return (dl if need_dl else None), (dp if need_dp else None)


torch.library.register_autograd("otvae::soft_cross_entropy", _sce_backward, setup_context=_sce_setup)


# ------------------------------------------------------------------------------------------------ GaussianBlur
@functools.lru_cache(maxsize=64)
def _gaussian_kernel1d(kernel_size: int, sigma: float):
    """torchvision's ``_get_gaussian_kernel1d`` in fp32 on the host, as a ctypes array for the kernel's argument block"""
    half = (kernel_size - 1) * 0.5
    x = torch.linspace(-half, half, steps=kernel_size)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return (C.c_float * kernel_size)(*(pdf / pdf.sum()).tolist())


def _blur_call(entry: str, img: Tensor, kx: int, ky: int, sx: float, sy: float) -> Tensor:
    """``img``: fp32 [C, H, W] or [N, C, H, W], NCHW-contiguous or channels-last (any other striding is made contiguous first); the
    result has the layout of the input."""
    lib = _lib.load()
    _lib.require_cuda(img, "gaussian_blur input")
    if img.dtype != torch.float32:
        raise NotImplementedError(f"gaussian_blur computes in float32, got {img.dtype}")
    if img.dim() not in (3, 4):
        raise ValueError(f"gaussian_blur takes [C, H, W] or [N, C, H, W] images, got {tuple(img.shape)}")
    x4 = img if img.dim() == 4 else img.unsqueeze(0)
    n, c, h, w = x4.shape
    if kx // 2 >= w or ky // 2 >= h:   # F.pad(mode="reflect")'s own refusal, in its words
        raise RuntimeError(f"Padding size should be less than the corresponding input dimension, but got: padding ({kx // 2}, {kx // 2}) "
                           f"at dimension 3 and ({ky // 2}, {ky // 2}) at dimension 2 of input {list(x4.shape)}")
    if x4.numel() == 0:
        return torch.empty_like(img)
    from .functional import is_nhwc
    if x4.is_contiguous():
        channels_last = 0
    elif is_nhwc(x4):
        channels_last = 1
    else:
        x4, channels_last = x4.contiguous(), 0
    out = torch.empty_strided(x4.shape, x4.stride(), device=x4.device, dtype=x4.dtype)
    check(getattr(lib, entry)(ptr(x4), n, c, h, w, channels_last, kx, ky, _gaussian_kernel1d(kx, sx), _gaussian_kernel1d(ky, sy),
                              ptr(out), stream()), entry)
    return out if img.dim() == 4 else out.squeeze(0)


def _blur_fwd(img: Tensor, kx: int, ky: int, sx: float, sy: float) -> Tensor:
    return _blur_call("otvae_gaussian_blur_fwd", img, kx, ky, sx, sy)


def _blur_bwd(gout: Tensor, kx: int, ky: int, sx: float, sy: float) -> Tensor:
    return _blur_call("otvae_gaussian_blur_bwd", gout, kx, ky, sx, sy)


def _blur_fake(img, kx, ky, sx, sy):
    from .functional import is_nhwc
    x4 = img if img.dim() == 4 else img.unsqueeze(0)
    dense = x4.is_contiguous() or is_nhwc(x4)
    return torch.empty_strided(img.shape, img.stride(), device=img.device, dtype=img.dtype) if dense else \
        torch.empty(img.shape, device=img.device, dtype=img.dtype)


_define("gaussian_blur", "(Tensor img, int kx, int ky, float sigma_x, float sigma_y) -> Tensor", _blur_fwd, _blur_fake)
_define("gaussian_blur_backward", "(Tensor gout, int kx, int ky, float sigma_x, float sigma_y) -> Tensor", _blur_bwd, _blur_fake)


def _blur_setup(ctx, inputs, output):
    ctx.cfg = inputs[1:]


def _blur_backward(ctx, gout):
    return torch.ops.otvae.gaussian_blur_backward(gout, *ctx.cfg), None, None, None, None


torch.library.register_autograd("otvae::gaussian_blur", _blur_backward, setup_context=_blur_setup)


# ------------------------------------------------------------------------------------------------ validation metrics
# In-place accumulators like ``bn_batch_stats``' running buffers: the states are mutated, nothing is returned, nothing is differentiable.
def _moments_accum(feats: Tensor, n_obs: Tensor, sum_x: Tensor, sum_xx: Tensor) -> None:
    lib = _lib.load()
    _lib.require_cuda(feats, "features")
    if feats.dim() != 2 or feats.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"moments_accum takes [B, D] float32 / float64 features, got {tuple(feats.shape)} {feats.dtype}")
    b, d = feats.shape
    if b == 0:
        return
    for name, t, shape in (("n_obs", n_obs, (1,)), ("sum_x", sum_x, (d,)), ("sum_xx", sum_xx, (d, d))):
        if t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"moments_accum: {name} must be a contiguous float64 tensor of shape {shape}, got {tuple(t.shape)} {t.dtype}")
    nbytes = lib.otvae_moments_accum_ws(b, d)
    if nbytes < 0:
        raise ValueError(f"moments_accum: feature width {d} is beyond the kernel's 2048")
    feats = feats.contiguous()
    ws = torch.empty(nbytes, device=feats.device, dtype=torch.uint8) if nbytes else None
    check(lib.otvae_moments_accum(0 if feats.dtype == torch.float32 else 1, ptr(feats), b, d, ptr(n_obs), ptr(sum_x), ptr(sum_xx), ptr(ws),
                                  stream()), "otvae_moments_accum")


def _sqerr_accum(preds: Tensor, target: Tensor, state: Tensor) -> None:
    lib = _lib.load()
    _lib.require_cuda(preds, "preds")
    if preds.shape != target.shape:
        raise ValueError(f"sqerr_accum: preds {tuple(preds.shape)} and target {tuple(target.shape)} differ in shape")
    if preds.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"sqerr_accum takes float32 / float64 tensors, got {preds.dtype}")
    if state.dtype != torch.float64 or state.numel() != lib.otvae_sqerr_state_words() or not state.is_contiguous():
        raise ValueError(f"sqerr_accum: state must be {lib.otvae_sqerr_state_words()} contiguous float64 words")
    if preds.numel() == 0:
        return
    preds, target = preds.contiguous(), target.to(preds.dtype).contiguous()
    check(lib.otvae_sqerr_accum(0 if preds.dtype == torch.float32 else 1, ptr(preds), ptr(target), preds.numel(), ptr(state), stream()),
          "otvae_sqerr_accum")


_define("moments_accum", "(Tensor feats, Tensor(a!) n_obs, Tensor(b!) sum_x, Tensor(c!) sum_xx) -> ()", _moments_accum,
        lambda feats, n_obs, sum_x, sum_xx: None)
_define("sqerr_accum", "(Tensor preds, Tensor target, Tensor(a!) state) -> ()", _sqerr_accum, lambda preds, target, state: None)


# ------------------------------------------------------------------------------------------------ Kernel Inception Distance
def _poly_mmd_subsets(real: Tensor, fake: Tensor, idx_real: Optional[Tensor], idx_fake: Optional[Tensor], subset_size: int, degree: int,
                      gamma: float, coef: float):
    """``gamma`` is the number the kernel uses (the caller resolves the default 1 / D).  Indices must lie in [0, n): they are not read
    on the host (the kernel clamps a stray one); ``metrics/kid.py`` constructs them in range."""
    lib = _lib.load()
    _lib.require_cuda(real, "real features")
    _lib.require_cuda(fake, "fake features")
    for name, t in (("real", real), ("fake", fake)):
        if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"poly_mmd_subsets: {name} must be a contiguous [n, D] float32 tensor, got {tuple(t.shape)} {t.dtype}")
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"poly_mmd_subsets: feature widths differ ({real.shape[1]} and {fake.shape[1]})")
    if (idx_real is None) != (idx_fake is None):
        raise ValueError("poly_mmd_subsets: idx_real and idx_fake come together")
    d, m = real.shape[1], int(subset_size)
    subsets = 1
    if idx_real is not None:
        for name, t in (("idx_real", idx_real), ("idx_fake", idx_fake)):
            _lib.require_cuda(t, name)
            if t.dim() != 2 or t.dtype != torch.int32 or not t.is_contiguous() or t.shape[1] != m or t.shape != idx_real.shape:
                raise ValueError(f"poly_mmd_subsets: {name} must be a contiguous [S, {m}] int32 tensor, got {tuple(t.shape)} {t.dtype}")
        subsets = idx_real.shape[0]
    if not 2 <= m <= min(real.shape[0], fake.shape[0]):
        raise ValueError("Argument `subset_size` should be smaller than the number of samples")
    if degree < 1 or subsets < 1 or d < 1 or not (gamma == gamma and coef == coef):
        raise ValueError(f"poly_mmd_subsets: bad argument (subsets {subsets}, width {d}, degree {degree}, gamma {gamma}, coef {coef})")
    nbytes = lib.otvae_poly_mmd_ws(subsets, m, d)
    if nbytes < 0 or degree > 8:
        raise NotImplementedError(f"poly_mmd_subsets: {subsets} subsets of {m} rows, width {d}, degree {degree} is beyond the kernel's "
                                  "envelope (65535 subsets, width 2048, degree 8)")
    ws = torch.empty(nbytes, device=real.device, dtype=torch.uint8)
    per_subset = torch.empty(subsets, device=real.device, dtype=torch.float64)
    stats = torch.empty(2, device=real.device, dtype=torch.float64)
    check(lib.otvae_poly_mmd_subsets(ptr(real), real.shape[0], ptr(fake), fake.shape[0], d, ptr(idx_real), ptr(idx_fake), subsets, m,
                                     int(degree), float(gamma), float(coef), ptr(ws), ptr(per_subset), ptr(stats), stream()),
          "otvae_poly_mmd_subsets")
    return per_subset, stats


def _poly_mmd_subsets_fake(real, fake, idx_real, idx_fake, subset_size, degree, gamma, coef):
    subsets = 1 if idx_real is None else idx_real.shape[0]
    return real.new_empty((subsets,), dtype=torch.float64), real.new_empty((2,), dtype=torch.float64)


def _feature_append(feats: Tensor, buf: Tensor, count: Tensor) -> None:
    lib = _lib.load()
    _lib.require_cuda(feats, "features")
    _lib.require_cuda(buf, "feature buffer")
    _lib.require_cuda(count, "count")
    if feats.dim() != 2 or feats.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"feature_append takes [B, D] float32 / float64 features, got {tuple(feats.shape)} {feats.dtype}")
    if buf.dim() != 2 or buf.dtype != torch.float32 or not buf.is_contiguous() or buf.shape[1] != feats.shape[1] or buf.shape[0] < 1:
        raise ValueError(f"feature_append: the buffer must be a contiguous [capacity, {feats.shape[1]}] float32 tensor, got "
                         f"{tuple(buf.shape)} {buf.dtype}")
    if count.dtype != torch.int64 or tuple(count.shape) != (2,) or not count.is_contiguous():
        raise ValueError(f"feature_append: count must be a contiguous int64 tensor of shape (2,), got {tuple(count.shape)} {count.dtype}")
    b, d = feats.shape
    if b == 0 or d == 0:
        return
    feats = feats.contiguous()
    check(lib.otvae_feature_append(0 if feats.dtype == torch.float32 else 1, ptr(feats), b, d, ptr(buf), buf.shape[0], ptr(count),
                                   stream()), "otvae_feature_append")


_define("poly_mmd_subsets", "(Tensor real, Tensor fake, Tensor? idx_real, Tensor? idx_fake, int subset_size, int degree, float gamma, "
        "float coef) -> (Tensor per_subset, Tensor stats)", _poly_mmd_subsets, _poly_mmd_subsets_fake)
_define("feature_append", "(Tensor feats, Tensor(a!) buf, Tensor(b!) count) -> ()", _feature_append, lambda feats, buf, count: None)


# ------------------------------------------------------------------------------------------------ k-NN manifold statistics
def _manifold_features(op: str, name: str, t: Tensor) -> None:
    _lib.require_cuda(t, f"{name} features")
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{op}: {name} must be a contiguous [n, D] float32 tensor, got {tuple(t.shape)} {t.dtype}")


def _knn_sq_radii(x: Tensor, k: int) -> Tensor:
    """``r2 [n]`` float64: the k-th smallest squared distance from each row to the OTHER rows (self excluded by index)"""
    lib = _lib.load()
    _manifold_features("knn_sq_radii", "x", x)
    n, d = x.shape
    nbytes = lib.otvae_knn_sq_radii_ws(n, d, int(k))
    if nbytes < 0:
        raise ValueError(f"knn_sq_radii: need 1 <= k <= 16, k < n <= 2^21 rows and a feature width in 1 ... 2048, got k = {k}, "
                         f"x {tuple(x.shape)}")
    ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
    r2 = torch.empty(n, device=x.device, dtype=torch.float64)
    check(lib.otvae_knn_sq_radii(ptr(x), n, d, int(k), ptr(r2), ptr(ws), stream()), "otvae_knn_sq_radii")
    return r2


def _manifold_counts(real: Tensor, r2_real: Tensor, fake: Tensor, r2_fake: Tensor):
    """``(count_fake [M] int32, hit_real [N] int32, min_real [N] float64)`` of ``otvae_manifold_counts``"""
    lib = _lib.load()
    _manifold_features("manifold_counts", "real", real)
    _manifold_features("manifold_counts", "fake", fake)
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"manifold_counts: feature widths differ ({real.shape[1]} and {fake.shape[1]})")
    for name, r, f in (("r2_real", r2_real, real), ("r2_fake", r2_fake, fake)):
        _lib.require_cuda(r, name)
        if r.dtype != torch.float64 or tuple(r.shape) != (f.shape[0],) or not r.is_contiguous():
            raise ValueError(f"manifold_counts: {name} must be a contiguous float64 tensor of shape ({f.shape[0]},), got "
                             f"{tuple(r.shape)} {r.dtype}")
    (n, d), m = real.shape, fake.shape[0]
    nbytes = lib.otvae_manifold_counts_ws(n, m, d)
    if nbytes < 0:
        raise ValueError(f"manifold_counts: need 2 <= rows <= 2^21 per side and a feature width in 1 ... 2048, got real "
                         f"{tuple(real.shape)}, fake {tuple(fake.shape)}")
    ws = torch.empty(nbytes, device=real.device, dtype=torch.uint8)
    count_fake = torch.empty(m, device=real.device, dtype=torch.int32)
    hit_real = torch.empty(n, device=real.device, dtype=torch.int32)
    min_real = torch.empty(n, device=real.device, dtype=torch.float64)
    check(lib.otvae_manifold_counts(ptr(real), ptr(r2_real), n, ptr(fake), ptr(r2_fake), m, d, ptr(count_fake), ptr(hit_real),
                                    ptr(min_real), ptr(ws), stream()), "otvae_manifold_counts")
    return count_fake, hit_real, min_real


def _manifold_counts_fake(real, r2_real, fake, r2_fake):
    return (fake.new_empty((fake.shape[0],), dtype=torch.int32), real.new_empty((real.shape[0],), dtype=torch.int32),
            real.new_empty((real.shape[0],), dtype=torch.float64))


_define("knn_sq_radii", "(Tensor x, int k) -> Tensor", _knn_sq_radii, lambda x, k: x.new_empty((x.shape[0],), dtype=torch.float64))
_define("manifold_counts", "(Tensor real, Tensor r2_real, Tensor fake, Tensor r2_fake) -> (Tensor count_fake, Tensor hit_real, "
        "Tensor min_real)", _manifold_counts, _manifold_counts_fake)

SSIM_RANGE_FIXED, SSIM_RANGE_CLAMP, SSIM_RANGE_BATCH = 0, 1, 2   # otvae_ssim_accum's range_mode


def _ssim_pair_check(name: str, preds: Tensor, target: Tensor):
    """what every SSIM entry asks of its image pair first: on the device, [B, C, H, W] of one shape, one float dtype; returns lib"""
    lib = _lib.load()
    _lib.require_cuda(preds, "preds")
    _lib.require_cuda(target, "target")
    if preds.dim() != 4 or preds.shape != target.shape:
        raise ValueError(f"{name} takes two [B, C, H, W] tensors of one shape, got {tuple(preds.shape)} and {tuple(target.shape)}")
    if preds.dtype not in (torch.float32, torch.float64) or target.dtype != preds.dtype:
        raise ValueError(f"{name} takes two float32 or two float64 tensors, got {preds.dtype} and {target.dtype}")
    return lib


def _ssim_accum(preds: Tensor, target: Tensor, win_h, win_w, k1: float, k2: float, range_mode: int, range_lo: float, range_hi: float,
                state: Tensor, per_image: Optional[Tensor]) -> None:
    """``win_h`` / ``win_w``: the window's weights per axis, float64 values of the host (they travel in the kernel's argument block)"""
    lib = _ssim_pair_check("ssim_accum", preds, target)
    if not (preds.is_contiguous() and target.is_contiguous()):
        raise ValueError("ssim_accum: preds and target must be NCHW-contiguous")
    b, c, h, w = preds.shape
    kh, kw = len(win_h), len(win_w)
    if kh % 2 == 0 or kw % 2 == 0 or h < kh or w < kw:
        raise ValueError(f"ssim_accum: a {kh} x {kw} window must be odd and fit the {h} x {w} images")
    words = lib.otvae_ssim_state_words()
    if state.dtype != torch.float64 or state.numel() != words or not state.is_contiguous():
        raise ValueError(f"ssim_accum: state must be {words} contiguous float64 words")
    if per_image is not None and (per_image.dtype != torch.float64 or tuple(per_image.shape) != (b,) or not per_image.is_contiguous()):
        raise ValueError(f"ssim_accum: per_image must be a contiguous float64 tensor of shape ({b},)")
    if range_mode not in (SSIM_RANGE_FIXED, SSIM_RANGE_CLAMP, SSIM_RANGE_BATCH):
        raise ValueError(f"ssim_accum: range_mode must be 0, 1 or 2, got {range_mode}")
    if b == 0 or c == 0:
        return
    if kh > 31 or kw > 31:
        raise NotImplementedError(f"ssim_accum: a {kh} x {kw} window is beyond the kernel's 31 taps per axis")
    nbytes = lib.otvae_ssim_ws(b, c, h, w, kh, kw)
    if nbytes < 0:
        raise NotImplementedError(f"ssim_accum: {tuple(preds.shape)} with a {kh} x {kw} window is beyond the kernel's envelope")
    ws = torch.empty(nbytes, device=preds.device, dtype=torch.uint8)
    check(lib.otvae_ssim_accum(0 if preds.dtype == torch.float32 else 1, ptr(preds), ptr(target), b, c, h, w, kh, kw,
                               (C.c_double * kh)(*win_h), (C.c_double * kw)(*win_w), float(k1), float(k2),
                               int(range_mode), float(range_lo), float(range_hi), ptr(per_image), ptr(state), ptr(ws), stream()),
          "otvae_ssim_accum")


_define("ssim_accum", "(Tensor preds, Tensor target, float[] win_h, float[] win_w, float k1, float k2, int range_mode, float range_lo, "
        "float range_hi, Tensor(a!) state, Tensor(b!)? per_image) -> ()", _ssim_accum,
        lambda preds, target, win_h, win_w, k1, k2, range_mode, range_lo, range_hi, state, per_image: None)


# ------------------------------------------------------------------------------------------------ SSIM as a loss
def _ssim_loss_check(name: str, preds: Tensor, target: Tensor, win_h, win_w, range_mode: int):
    """the refusals the forward and the backward share, before any kernel; returns (lib, b, c, h, w, kh, kw)"""
    lib = _ssim_pair_check(name, preds, target)
    b, c, h, w = preds.shape
    kh, kw = len(win_h), len(win_w)
    if kh % 2 == 0 or kw % 2 == 0 or h < kh or w < kw:
        raise ValueError(f"{name}: a {kh} x {kw} window must be odd and fit the {h} x {w} images")
    if range_mode not in (SSIM_RANGE_FIXED, SSIM_RANGE_CLAMP):
        raise ValueError(f"{name}: range_mode must be 0 (fixed) or 1 (clamp), got {range_mode}: a range taken from the batch depends on "
                         "the data, and a loss needs a fixed scale")
    if b and c and lib.otvae_ssim_grad_ws(b, c, h, w, kh, kw) < 0:
        raise NotImplementedError(f"{name}: {tuple(preds.shape)} with a {kh} x {kw} window is beyond the gradient kernel's envelope "
                                  "(15 taps per axis)")
    return lib, b, c, h, w, kh, kw


def _ssim_loss_fwd(preds: Tensor, target: Tensor, win_h, win_w, k1: float, k2: float, range_mode: int, range_lo: float,
                   range_hi: float) -> Tensor:
    """``structural_similarity``'s per-image values by the same call of ``otvae_ssim_accum``: the running sums go to a scratch state"""
    lib, b, c, _, _, _, _ = _ssim_loss_check("ssim_loss", preds, target, win_h, win_w, range_mode)
    per_image = torch.empty(b, dtype=torch.float64, device=preds.device)
    if b == 0 or c == 0:
        return per_image
    state = torch.empty(lib.otvae_ssim_state_words(), dtype=torch.float64, device=preds.device)   # written, never read
    _ssim_accum(preds.contiguous(), target.contiguous(), win_h, win_w, k1, k2, range_mode, range_lo, range_hi, state, per_image)
    return per_image


def _ssim_loss_bwd(g: Tensor, preds: Tensor, target: Tensor, win_h, win_w, k1: float, k2: float, range_mode: int, range_lo: float,
                   range_hi: float) -> Tensor:
    """d sum_b g[b] ssim_b / d preds; for ``target`` the caller exchanges the two images (the map is symmetric)"""
    lib, b, c, h, w, kh, kw = _ssim_loss_check("ssim_loss_backward", preds, target, win_h, win_w, range_mode)
    if tuple(g.shape) != (b,):
        raise ValueError(f"ssim_loss_backward: the cotangent must have shape ({b},), got {tuple(g.shape)}")
    grad = torch.empty(preds.shape, dtype=preds.dtype, device=preds.device)
    if b == 0 or c == 0:
        return grad
    g = g.to(torch.float64).contiguous()
    nbytes = lib.otvae_ssim_grad_ws(b, c, h, w, kh, kw)
    ws = torch.empty(nbytes, device=preds.device, dtype=torch.uint8) if nbytes else None
    check(lib.otvae_ssim_grad(0 if preds.dtype == torch.float32 else 1, ptr(preds.contiguous()), ptr(target.contiguous()), b, c, h, w, kh,
                              kw, (C.c_double * kh)(*win_h), (C.c_double * kw)(*win_w), float(k1), float(k2), int(range_mode),
                              float(range_lo), float(range_hi), ptr(g), ptr(grad), ptr(ws), stream()), "otvae_ssim_grad")
    return grad


_define("ssim_loss", "(Tensor preds, Tensor target, float[] win_h, float[] win_w, float k1, float k2, int range_mode, float range_lo, "
        "float range_hi) -> Tensor", _ssim_loss_fwd,
        lambda preds, target, win_h, win_w, k1, k2, range_mode, range_lo, range_hi: preds.new_empty(preds.shape[0], dtype=torch.float64))
_define("ssim_loss_backward", "(Tensor g, Tensor preds, Tensor target, float[] win_h, float[] win_w, float k1, float k2, int range_mode, "
        "float range_lo, float range_hi) -> Tensor", _ssim_loss_bwd,
        lambda g, preds, target, win_h, win_w, k1, k2, range_mode, range_lo, range_hi: preds.new_empty(preds.shape))


def _ssim_loss_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.cfg = inputs[2:]


def _ssim_loss_backward(ctx, g):
    preds, target = ctx.saved_tensors
    need_p, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    gp = torch.ops.otvae.ssim_loss_backward(g, preds, target, *ctx.cfg) if need_p else None
    gt = torch.ops.otvae.ssim_loss_backward(g, target, preds, *ctx.cfg) if need_t else None
    return (gp, gt) + (None,) * 7


torch.library.register_autograd("otvae::ssim_loss", _ssim_loss_backward, setup_context=_ssim_loss_setup)
_refuse_second_derivative("ssim_loss_backward", "SSIM loss")


# ------------------------------------------------------------------------------------------------ multi-scale SSIM
MS_SSIM_NORMALIZE = {None: 0, "relu": 1, "simple": 2}   # otvae_ms_ssim_accum's normalize
_MS_SSIM_ELEM = {torch.float32: 4, torch.float64: 8}


def _ms_ssim_check(name: str, preds: Tensor, target: Tensor, win_h, win_w, betas, max_taps: int):
    """the refusals every multi-scale entry shares, before any kernel; returns (lib, b, c, h, w, kh, kw, scales)"""
    lib = _ssim_pair_check(name, preds, target)
    if not (preds.is_contiguous() and target.is_contiguous()):
        raise ValueError(f"{name}: preds and target must be NCHW-contiguous")
    b, c, h, w = preds.shape
    kh, kw, scales = len(win_h), len(win_w), len(betas)
    if kh % 2 == 0 or kw % 2 == 0 or scales < 1:
        raise ValueError(f"{name}: a {kh} x {kw} window must be odd, and betas must not be empty")
    if kh > max_taps or kw > max_taps or scales > 8:
        raise NotImplementedError(f"{name}: {scales} scales of a {kh} x {kw} window are beyond the kernel's envelope ({max_taps} taps per "
                                  "axis, 8 scales)")
    if (h >> (scales - 1)) < kh or (w >> (scales - 1)) < kw:
        raise ValueError(f"{name}: {h} x {w} images are too small for {scales} scales of a {kh} x {kw} window: every scale must hold one "
                         f"window, so the smallest admissible size is {kh << (scales - 1)} x {kw << (scales - 1)}")
    return lib, b, c, h, w, kh, kw, scales


def _ms_ssim_run(lib, preds, target, win_h, win_w, k1, k2, range_mode, range_lo, range_hi, betas, normalize, per_image, weights, pyramid,
                 state):
    b, c, h, w = preds.shape
    kh, kw, scales = len(win_h), len(win_w), len(betas)
    nbytes = lib.otvae_ms_ssim_ws(b, c, h, w, kh, kw, scales)
    if nbytes < 0:
        raise NotImplementedError(f"ms_ssim: {tuple(preds.shape)} with {scales} scales of a {kh} x {kw} window is beyond the kernel's envelope")
    ws = torch.empty(nbytes, device=preds.device, dtype=torch.uint8)
    check(lib.otvae_ms_ssim_accum(0 if preds.dtype == torch.float32 else 1, ptr(preds), ptr(target), b, c, h, w, kh, kw,
                                  (C.c_double * kh)(*win_h), (C.c_double * kw)(*win_w), float(k1), float(k2), int(range_mode),
                                  float(range_lo), float(range_hi), scales, (C.c_double * scales)(*betas), int(normalize), ptr(per_image),
                                  ptr(weights), ptr(pyramid[0]) if scales > 1 else None, ptr(pyramid[1]) if scales > 1 else None,
                                  ptr(state), ptr(ws), stream()), "otvae_ms_ssim_accum")


def _ms_ssim_pyramid(lib, preds: Tensor, scales: int) -> Tensor:
    """[2][elements]: scales 1 .. S - 1 of preds, then of target"""
    b, c, h, w = preds.shape
    nbytes = max(0, lib.otvae_ms_ssim_pyramid(0 if preds.dtype == torch.float32 else 1, b, c, h, w, scales)) if b and c else 0
    return torch.empty((2, nbytes // _MS_SSIM_ELEM[preds.dtype]), dtype=preds.dtype, device=preds.device)


def _ms_ssim_accum(preds: Tensor, target: Tensor, win_h, win_w, k1: float, k2: float, range_mode: int, range_lo: float, range_hi: float,
                   betas, normalize: int, state: Tensor, per_image: Optional[Tensor]) -> None:
    lib, b, c, _, _, _, _, scales = _ms_ssim_check("ms_ssim_accum", preds, target, win_h, win_w, betas, 31)
    words = lib.otvae_ms_ssim_state_words()
    if state.dtype != torch.float64 or state.numel() != words or not state.is_contiguous():
        raise ValueError(f"ms_ssim_accum: state must be {words} contiguous float64 words")
    if per_image is not None and (per_image.dtype != torch.float64 or tuple(per_image.shape) != (b,) or not per_image.is_contiguous()):
        raise ValueError(f"ms_ssim_accum: per_image must be a contiguous float64 tensor of shape ({b},)")
    if range_mode not in (SSIM_RANGE_FIXED, SSIM_RANGE_CLAMP, SSIM_RANGE_BATCH) or normalize not in (0, 1, 2):
        raise ValueError(f"ms_ssim_accum: range_mode must be 0, 1 or 2 and normalize 0, 1 or 2, got {range_mode} and {normalize}")
    if b == 0 or c == 0:
        return
    _ms_ssim_run(lib, preds, target, win_h, win_w, k1, k2, range_mode, range_lo, range_hi, betas, normalize, per_image, None,
                 _ms_ssim_pyramid(lib, preds, scales), state)


_define("ms_ssim_accum", "(Tensor preds, Tensor target, float[] win_h, float[] win_w, float k1, float k2, int range_mode, float range_lo, "
        "float range_hi, float[] betas, int normalize, Tensor(a!) state, Tensor(b!)? per_image) -> ()", _ms_ssim_accum,
        lambda preds, target, win_h, win_w, k1, k2, range_mode, range_lo, range_hi, betas, normalize, state, per_image: None)


def _ms_ssim_loss_check(name, preds, target, win_h, win_w, betas, range_mode, normalize):
    out = _ms_ssim_check(name, preds, target, win_h, win_w, betas, 15)
    if range_mode not in (SSIM_RANGE_FIXED, SSIM_RANGE_CLAMP):
        raise ValueError(f"{name}: range_mode must be 0 (fixed) or 1 (clamp), got {range_mode}: a range taken from the batch depends on "
                         "the data, and a loss needs a fixed scale")
    if normalize not in (0, 1, 2):
        raise ValueError(f"{name}: normalize must be 0 (none), 1 (relu) or 2 (simple), got {normalize}")
    return out


def _ms_ssim_fwd(preds: Tensor, target: Tensor, win_h, win_w, k1: float, k2: float, range_mode: int, range_lo: float, range_hi: float,
                 betas, normalize: int):
    """(msssim [B] float64, w [S][B] float64, the pyramid [2][elements] of both images): what the backward operator needs"""
    lib, b, c, _, _, _, _, scales = _ms_ssim_loss_check("ms_ssim", preds, target, win_h, win_w, betas, range_mode, normalize)
    per_image = torch.empty(b, dtype=torch.float64, device=preds.device)
    weights = torch.empty((scales, b), dtype=torch.float64, device=preds.device)
    pyramid = _ms_ssim_pyramid(lib, preds, scales)
    if b == 0 or c == 0:
        return per_image, weights, pyramid
    state = torch.empty(lib.otvae_ms_ssim_state_words(), dtype=torch.float64, device=preds.device)   # written, never read
    _ms_ssim_run(lib, preds, target, win_h, win_w, k1, k2, range_mode, range_lo, range_hi, betas, normalize, per_image, weights, pyramid,
                 state)
    return per_image, weights, pyramid


def _ms_ssim_fwd_fake(preds, target, win_h, win_w, k1, k2, range_mode, range_lo, range_hi, betas, normalize):
    b, c, h, w = preds.shape
    n = sum(b * c * (h >> s) * (w >> s) for s in range(1, len(betas)))
    return (preds.new_empty((b,), dtype=torch.float64), preds.new_empty((len(betas), b), dtype=torch.float64), preds.new_empty((2, n)))


def _ms_ssim_bwd(g: Tensor, weights: Tensor, pyramid: Tensor, preds: Tensor, target: Tensor, swap: bool, win_h, win_w, k1: float,
                 k2: float, range_mode: int, range_lo: float, range_hi: float, betas, normalize: int) -> Tensor:
    """d sum_b g[b] msssim_b / d preds; ``swap``: ``preds`` / ``target`` arrive exchanged and so do the pyramid's two rows (the gradient for
    the forward's ``target``: every term is symmetric)"""
    lib, b, c, h, w, kh, kw, scales = _ms_ssim_loss_check("ms_ssim_backward", preds, target, win_h, win_w, betas, range_mode, normalize)
    if tuple(g.shape) != (b,) or tuple(weights.shape) != (scales, b) or weights.dtype != torch.float64:
        raise ValueError(f"ms_ssim_backward: the cotangent must have shape ({b},) and the weights ({scales}, {b}) in float64, got "
                         f"{tuple(g.shape)} and {tuple(weights.shape)}")
    grad = torch.empty(preds.shape, dtype=preds.dtype, device=preds.device)
    if b == 0 or c == 0:
        return grad
    in_dtype = 0 if preds.dtype == torch.float32 else 1
    want = lib.otvae_ms_ssim_pyramid(in_dtype, b, c, h, w, scales) // _MS_SSIM_ELEM[preds.dtype]
    if pyramid.dtype != preds.dtype or tuple(pyramid.shape) != (2, want) or not pyramid.is_contiguous():
        raise ValueError(f"ms_ssim_backward: the pyramid must be the forward's (2, {want}) tensor of {preds.dtype}")
    g = g.to(torch.float64).contiguous()
    nbytes = lib.otvae_ms_ssim_grad_ws(in_dtype, b, c, h, w, kh, kw, scales)
    if nbytes < 0:
        raise NotImplementedError(f"ms_ssim_backward: {tuple(preds.shape)} with {scales} scales of a {kh} x {kw} window is beyond the "
                                  "gradient kernel's envelope")
    ws = torch.empty(nbytes, device=preds.device, dtype=torch.uint8) if nbytes else None
    pyr_p, pyr_t = (pyramid[1], pyramid[0]) if swap else (pyramid[0], pyramid[1])
    check(lib.otvae_ms_ssim_grad(in_dtype, ptr(preds), ptr(target), ptr(pyr_p) if scales > 1 else None, ptr(pyr_t) if scales > 1 else None,
                                 b, c, h, w, kh, kw, (C.c_double * kh)(*win_h), (C.c_double * kw)(*win_w), float(k1), float(k2),
                                 int(range_mode), float(range_lo), float(range_hi), scales, ptr(g), ptr(weights.contiguous()), ptr(grad),
                                 ptr(ws), stream()), "otvae_ms_ssim_grad")
    return grad


_define("ms_ssim", "(Tensor preds, Tensor target, float[] win_h, float[] win_w, float k1, float k2, int range_mode, float range_lo, "
        "float range_hi, float[] betas, int normalize) -> (Tensor, Tensor, Tensor)", _ms_ssim_fwd, _ms_ssim_fwd_fake)
_define("ms_ssim_backward", "(Tensor g, Tensor weights, Tensor pyramid, Tensor preds, Tensor target, bool swap, float[] win_h, "
        "float[] win_w, float k1, float k2, int range_mode, float range_lo, float range_hi, float[] betas, int normalize) -> Tensor",
        _ms_ssim_bwd,
        lambda g, weights, pyramid, preds, target, swap, win_h, win_w, k1, k2, range_mode, range_lo, range_hi, betas, normalize:
        preds.new_empty(preds.shape))


def _ms_ssim_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], output[1], output[2])
    ctx.cfg = inputs[2:]
    ctx.set_materialize_grads(False)   # w and the pyramid never carry a gradient


def _ms_ssim_backward(ctx, g, _gw, _gpyr):
    if g is None:
        return (None,) * 11
    preds, target, weights, pyramid = ctx.saved_tensors
    need_p, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    gp = torch.ops.otvae.ms_ssim_backward(g, weights, pyramid, preds, target, False, *ctx.cfg) if need_p else None
    gt = torch.ops.otvae.ms_ssim_backward(g, weights, pyramid, target, preds, True, *ctx.cfg) if need_t else None
    return (gp, gt) + (None,) * 9


torch.library.register_autograd("otvae::ms_ssim", _ms_ssim_backward, setup_context=_ms_ssim_setup)
_refuse_second_derivative("ms_ssim_backward", "MS-SSIM loss")
