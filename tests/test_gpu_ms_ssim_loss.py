"""GPU: ``MSSSIMLoss`` / ``ms_ssim_loss`` / ``torch.ops.otvae.ms_ssim`` (``csrc/ssim.hip``, ``csrc/ssim_grad.hip``) against float64 autograd of the definition
(``tests/ms_ssim_definition.py``), evaluated on the CPU.

Truth and bound.  The float64 autograd gradient of ``sum_b g_b (1 - msssim_b)`` is the truth, the float32 autograd gradient of the same
function the "composition".  Per image b and elementwise, as in ``tests/test_gpu_ssim_loss.py``:
``|ours - truth| <= max(1e-4 max|truth_b|, 1.5 |composition - truth|)``.  The cotangents are distinct per image.  Every case prints our
error and the composition's.

The model tests use the small synthetic VAE of ``tests/test_gpu_ssim_loss.py`` at 32 x 32 instead of 16 x 16: three scales of the
5-tap window need 20 pixels."""
import copy
import functools

import pytest
import torch

from conftest import rel_err
from ms_ssim_definition import BETAS, CASE_IDS, CASES, definition, independent_pair, option_kwargs, pair_of, windows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd as pkg
    return pkg


def _cotangent(b, seed):
    """distinct, float32-representable, of either sign and away from 0"""
    g = torch.Generator().manual_seed(1000 + seed)
    v = 0.5 + torch.rand(b, generator=g, dtype=torch.float32) + torch.arange(b, dtype=torch.float32)
    return v * torch.where(torch.arange(b) % 2 == 0, 1.0, -1.0)


def _reference_grads(p, t, wh, ww, data_range, betas, g, dtype, normalize="relu", detach_pooled=False):
    """d sum_b g_b (1 - msssim_b) / d (p, t) by autograd of the definition in ``dtype``, as float64"""
    pd, td = p.detach().to(dtype, copy=True).requires_grad_(True), t.detach().to(dtype, copy=True).requires_grad_(True)
    loss = 1.0 - definition(pd, td, wh, ww, data_range, betas, normalize, detach_pooled=detach_pooled)[0]
    gp, gt = torch.autograd.grad((loss.double() * g.double()).sum(), [pd, td])
    return gp.double(), gt.double()


def _ours(A, p, t, g, data_range, betas, want_target=False, normalize="relu", **window):
    pc, tc = p.detach().cuda().requires_grad_(True), t.detach().cuda().requires_grad_(want_target)
    loss = A.MSSSIMLoss(data_range=data_range, betas=betas, normalize=normalize, reduction="none", **option_kwargs(window))(pc, tc)
    assert loss.dtype == p.dtype and loss.shape == (p.shape[0],)
    loss.backward(g.to(p.dtype).cuda())
    assert pc.grad.dtype == p.dtype and pc.grad.shape == p.shape
    return loss.detach(), pc.grad, (tc.grad if want_target else None)


def _assert_bound(label, ours, truth, comp):
    ours = ours.double().cpu()
    scale = truth.abs().amax(dim=(1, 2, 3), keepdim=True)
    err, cerr = (ours - truth).abs(), (comp - truth).abs()
    bound = torch.maximum(1e-4 * scale, 1.5 * cerr)
    print(f"[ms-ssim grad {label}] max|truth| {scale.flatten().tolist()}  ours err/scale {(err / scale).amax(dim=(1, 2, 3)).tolist()}  "
          f"composition err/scale {(cerr / scale).amax(dim=(1, 2, 3)).tolist()}")
    assert bool(torch.isfinite(ours).all())
    worst = float((err - bound).max())
    assert bool((err <= bound).all()), f"{label}: {int((err > bound).sum())} entries beyond the bound, the worst by {worst:.3e}"


@functools.lru_cache(maxsize=None)
def _case(case, rng, dtype):
    """inputs, cotangent and both reference gradients (for preds and target) of a case of the table, computed once"""
    shape, window, betas = CASES[case]
    p, t = pair_of(shape, rng, seed=sum(shape), dtype=dtype)
    wh, ww = windows(**window)
    g = _cotangent(shape[0], sum(shape))
    return p, t, g, _reference_grads(p, t, wh, ww, rng, betas, g, torch.float64), _reference_grads(p, t, wh, ww, rng, betas, g, torch.float32)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("rng", [1.0, 255.0])
@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_gradient_against_the_float64_definition(A, case, rng, dtype):
    _, window, betas = CASES[case]
    p, t, g, truth, comp = _case(case, rng, dtype)
    _, grad, _ = _ours(A, p, t, g, rng, betas, **window)
    _assert_bound(f"{CASE_IDS[case]} R={rng} {dtype}", grad, truth[0], comp[0])


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_target_gradient_and_symmetry(A):
    _, window, betas = CASES[1]
    p, t, g, truth, comp = _case(1, 1.0, torch.float32)
    _, gp, gt = _ours(A, p, t, g, 1.0, betas, want_target=True, **window)
    _assert_bound("preds, both inputs require a gradient", gp, truth[0], comp[0])
    _assert_bound("target", gt, truth[1], comp[1])
    _, gp_swapped, _ = _ours(A, t, p, g, 1.0, betas, **window)
    assert torch.equal(gt, gp_swapped), "grad_target is not the preds gradient of the exchanged call"


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_dropped_row_and_column_receive_the_own_scale_term_alone(A):
    """45 x 43: row 44 and column 42 are dropped by the first pooling, so nothing reaches them from the coarser scales"""
    shape, window, betas = CASES[1]
    p, t, g, truth, comp = _case(1, 1.0, torch.float32)
    wh, ww = windows(**window)
    own, _ = _reference_grads(p, t, wh, ww, 1.0, betas, g, torch.float64, detach_pooled=True)
    tiny = 1e-14 * float(truth[0].abs().max())
    assert float((own - truth[0])[:, :, 44, :].abs().max()) <= tiny and float((own - truth[0])[:, :, :, 42].abs().max()) <= tiny   # the truth has the property
    assert float((own - truth[0])[:, :, :44, :42].abs().amin()) > 0                                                     # ... and only there
    _, grad, _ = _ours(A, p, t, g, 1.0, betas, **window)
    grad = grad.double().cpu()
    bound = torch.maximum(1e-4 * truth[0].abs().amax(dim=(1, 2, 3), keepdim=True), 1.5 * (comp[0] - truth[0]).abs())
    err = (grad - own).abs()
    print(f"[ms-ssim grad dropped] row err {float(err[:, :, 44, :].max()):.3e} column err {float(err[:, :, :, 42].max()):.3e}")
    assert bool((err <= bound)[:, :, 44, :].all()) and bool((err <= bound)[:, :, :, 42].all())


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_clamp_mode_zeroes_the_own_term_and_passes_the_coarse_one(A, dtype):
    p, t = pair_of((2, 1, 41, 43), 1.0, seed=31, dtype=dtype, clamp=False)
    outside = (p < 0.2) | (p > 0.8)
    assert int(outside.sum()) > 50 and int((~outside).sum()) > 50
    wh, ww = windows(sigma=0.5)
    g = _cotangent(2, 31)
    betas = BETAS[:3]
    truth, _ = _reference_grads(p, t, wh, ww, (0.2, 0.8), betas, g, torch.float64)
    comp, _ = _reference_grads(p, t, wh, ww, (0.2, 0.8), betas, g, torch.float32)
    own, _ = _reference_grads(p, t, wh, ww, (0.2, 0.8), betas, g, torch.float64, detach_pooled=True)
    assert bool((own[outside] == 0).all())                                # the own-scale part is zero outside the interval
    pooled = torch.zeros_like(outside)
    pooled[:, :, :40, :42] = True                                         # pixels under a pooled pixel
    # ... while the coarse part arrives there -- unless the pooled pixel above is itself clamped at its scale and has nothing above it
    arrives = truth != 0
    assert float(arrives[outside & pooled].double().mean()) > 0.9 and not bool(arrives[outside & ~pooled].any())
    _, grad, _ = _ours(A, p, t, g, (0.2, 0.8), betas, sigma=0.5)
    _assert_bound(f"clamp (0.2, 0.8) {dtype}", grad, truth, comp)
    grad = grad.cpu()
    assert bool((grad[outside & ~pooled] == 0).all()), "a clamped pixel of the dropped row / column received a gradient"
    assert torch.equal((grad != 0)[outside], arrives[outside]), "the coarse gradient and ours differ in where they pass a clamped pixel"


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_dead_image_passes_no_gradient(A):
    p, t = independent_pair()
    wh, ww = windows(sigma=0.5)
    g = _cotangent(2, 3)
    betas = BETAS[:3]
    loss, grad, grad_t = _ours(A, p, t, g, 1.0, betas, want_target=True, sigma=0.5)
    assert float(loss[0]) == 1.0                                           # msssim_0 is exactly 0
    assert bool((grad[0] == 0).all()) and bool((grad_t[0] == 0).all()), "the dead image received a gradient"
    truth, truth_t = _reference_grads(p, t, wh, ww, 1.0, betas, g, torch.float64)
    comp, comp_t = _reference_grads(p, t, wh, ww, 1.0, betas, g, torch.float32)
    print(f"[ms-ssim grad dead image] torch autograd there: NaN {bool(torch.isnan(truth[0]).any())}, largest finite entry "
          f"{float(truth[0].nan_to_num(0.0).abs().max()):.3e}; ours: exactly 0")
    _assert_bound("the live image beside a dead one", grad[1:], truth[1:], comp[1:])
    _assert_bound("the live image beside a dead one, target", grad_t[1:], truth_t[1:], comp_t[1:])
    for normalize in ("simple", None):                                     # every image is alive under "simple"; None: image 1 is
        truth, _ = _reference_grads(p, t, wh, ww, 1.0, betas, g, torch.float64, normalize=normalize)
        comp, _ = _reference_grads(p, t, wh, ww, 1.0, betas, g, torch.float32, normalize=normalize)
        _, grad, _ = _ours(A, p, t, g, 1.0, betas, normalize=normalize, sigma=0.5)
        keep = slice(0, 2) if normalize == "simple" else slice(1, 2)
        _assert_bound(f"normalize={normalize}", grad[keep], truth[keep], comp[keep])


# 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_forward_bits_and_determinism(A, dtype):
    shape, window, betas = CASES[1]
    p, t = pair_of((3,) + shape[1:], 1.0, seed=61, dtype=dtype)
    g = _cotangent(3, 61)
    kw = dict(data_range=1.0, betas=betas, **option_kwargs(window))
    loss, grad, _ = _ours(A, p, t, g, 1.0, betas, **window)
    metric = A.metrics.multiscale_structural_similarity(p.cuda(), t.cuda(), **kw)
    assert torch.equal(loss, (1.0 - metric).to(dtype))
    o = A.MSSSIMLoss(**kw).options
    raw, w, pyramid = torch.ops.otvae.ms_ssim(p.cuda(), t.cuda(), o.window[0], o.window[1], o.k1, o.k2, o.range_mode, o.range_lo, o.range_hi,
                                              o.betas, o.normalize_mode)
    assert raw.dtype == torch.float64 and torch.equal(raw, metric) and w.shape == (4, 3) and pyramid.dtype == dtype
    first = torch.nn.functional.avg_pool2d(p.double(), 2)                  # the pyramid begins with the pooled preds
    assert (pyramid[0, :first.numel()].double().cpu().reshape(first.shape) - first).abs().max() <= (2.0 ** -22 if dtype == torch.float32 else 2.0 ** -51)
    for reduction, want in (("mean", loss.mean()), ("sum", loss.sum())):
        assert torch.equal(A.MSSSIMLoss(reduction=reduction, **kw)(p.cuda(), t.cuda()), want)
    assert torch.equal(A.ms_ssim_loss(p.cuda(), t.cuda(), reduction="none", **kw), loss)
    _, again, _ = _ours(A, p, t, g, 1.0, betas, **window)
    assert torch.equal(grad, again)
    _, alone, _ = _ours(A, p[1:2], t[1:2], g[1:2], 1.0, betas, **window)
    assert torch.equal(grad[1:2], alone), "image 1's gradient depends on its neighbours in the batch"
    _, moved, _ = _ours(A, p.flip(0).contiguous(), t.flip(0).contiguous(), g.flip(0), 1.0, betas, **window)
    assert torch.equal(grad, moved.flip(0)), "an image's gradient depends on where it sits in the batch"


# 7 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("window", [dict(), dict(gaussian=False, kernel_size=(3, 5))], ids=["11x11", "3x5"])
def test_one_scale_gradient_has_the_bits_of_the_ssim_gradient(A, window, dtype):
    """One scale, ``betas = (1.0,)``, no normalisation: msssim_b = pow(v, 1) and the fold's weight is 1.0 exactly, so the gradient kernel
    -- one body, ``ssg_tile_kernel`` of ``csrc/ssim_grad.hip``, for both losses -- does the SSIM gradient's arithmetic.  (The forward values
    agree to 1e-12 only: the two folds sum in different orders, ``test_gpu_ms_ssim.py::test_one_scale_is_ssim``.)"""
    p, t = pair_of((2, 2, 19, 37), 1.0, seed=97, dtype=dtype)
    g = _cotangent(2, 97).to(dtype).cuda()
    grads = []
    for loss_fn, extra in ((A.ms_ssim_loss, dict(betas=(1.0,), normalize=None)), (A.ssim_loss, {})):
        pc = p.cuda().requires_grad_(True)
        loss = loss_fn(pc, t.cuda(), data_range=1.0, reduction="none", **option_kwargs(window), **extra)
        assert bool(torch.isfinite(loss).all()) and bool((loss != 1.0).all())   # a finite non-zero msssim_b: the weight is 1.0
        loss.backward(g)
        grads.append(pc.grad)
    assert bool((grads[1] != 0).any())
    assert torch.equal(grads[0], grads[1]), f"{int((grads[0] != grads[1]).sum())} elements differ"


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(A):
    x = torch.rand(2, 1, 32, 32)
    with pytest.raises(RuntimeError):
        A.MSSSIMLoss(sigma=0.5, betas=BETAS[:3])(x, x)
    p = x.cuda().requires_grad_(True)
    loss = A.MSSSIMLoss(sigma=0.5, betas=BETAS[:3], reduction="sum")(p, x.cuda().flip(0))
    (grad,) = torch.autograd.grad(loss, p, create_graph=True)
    assert grad.requires_grad
    with pytest.raises(RuntimeError):          # (NotImplementedError is one): the backward operator has no derivative of its own
        torch.autograd.grad(grad.sum(), p)
    big = torch.rand(1, 1, 40, 40, device="cuda")
    wide = A.MSSSIMLoss(sigma=4.3, betas=(1.0,))       # 31 taps: the forward kernel has them, the gradient kernel does not
    assert wide.window_size == (31, 31)
    with pytest.raises(NotImplementedError):
        wide(big, big)                                   # refused in the forward already, as SSIMLoss does
    o = A.MSSSIMLoss(sigma=0.5, betas=BETAS[:3]).options
    xc = x.cuda()
    with pytest.raises(ValueError, match="range_mode"):
        torch.ops.otvae.ms_ssim(xc, xc, o.window[0], o.window[1], o.k1, o.k2, 2, 0.0, 0.0, o.betas, 1)
    with pytest.raises(ValueError):
        torch.ops.otvae.ms_ssim(xc, xc.double(), o.window[0], o.window[1], o.k1, o.k2, 0, 0.0, 1.0, o.betas, 1)


# 9 ------------------------------------------------------------------------------------------------------------------------------
B, IMG = 8, (1, 32, 32)


def _small_vae(A, seed=71, **kw):
    torch.manual_seed(seed)
    enc = A.CNN(1, 16, 32, 1, capacity=4, down_sample=True, residual="add")
    dec = A.CNN(8, 1, 1, 32, capacity=4, up_sample=True, residual="add")
    return A.VAE(encoder=enc, decoder=dec, prior=A.GaussianPrior(loss_coeff=0.1), **kw).cuda().train()


def _ms_ssim_vae(A, seed=71):
    return _small_vae(A, seed, ssim_loss=A.MSSSIMLoss(sigma=0.5, betas=BETAS[:3], data_range=1.0), ssim_weight=0.5)


def _batches(n=3):
    g = torch.Generator().manual_seed(81)
    xs = [torch.rand((B, *IMG), generator=g).cuda() for _ in range(n)]
    es = [torch.randn((B, 8, 1, 1), generator=g).cuda() for _ in range(n)]
    return xs, es


def test_model_logs_the_structural_term_in_recon(A):
    model = _ms_ssim_vae(A)
    assert model.ssim_weight == 0.5 and isinstance(model.ssim_loss, A.MSSSIMLoss)
    (x,), (eps,) = _batches(1)
    loss, logs, art = model.nelbo({"samples": x, "target": x, "kwargs": {"eps": eps}}, 0)
    total, recon, prior = (float(logs[f"train/loss/{k}"].detach()) for k in ("total", "recon", "prior"))
    assert float(loss.detach()) == total
    pm, xd = art["preds_mean"].detach().double().cpu(), x.double().cpu()
    wh, ww = windows(sigma=0.5)
    structural = 1.0 - definition(pm, xd, wh, ww, 1.0, BETAS[:3])[0].mean()
    want = float(((pm - xd) ** 2).mean() + 0.5 * structural)
    print(f"[ms-ssim vae] recon {recon} want {want} (structural {float(structural)}) total {total} prior {prior}")
    assert float(structural) > 0.01 and abs(recon - want) <= 1e-5 * abs(want)
    assert abs(total - recon - prior) <= 4 * 2.0 ** -23 * abs(total)
    loss.backward()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in model.optim_parameters())


def test_model_graphed_step_agrees_with_the_eager_step(A):
    xs, es = _batches()
    seen = {}
    for graphed in (False, True):
        model = _ms_ssim_vae(A)
        if graphed:
            model.enable_graphed_step()
        opt = torch.optim.Adam(model.optim_parameters(), lr=1e-3)
        model.batch_preprocess = lambda b: {"samples": b[0], "target": b[0], "kwargs": {"eps": b[1]}}
        rows = []
        for i, (x, eps) in enumerate(zip(xs, es)):
            opt.zero_grad()
            out = model.training_step((x, eps), i)
            out["loss"].backward()
            opt.step()
            rows.append(torch.stack([out[f"train/loss/{k}"].detach() for k in ("total", "recon", "prior")]).clone())
        seen[graphed] = torch.stack(rows)
        model.disable_graphed_step()
    print("[ms-ssim vae] eager:\n", seen[False].cpu(), "\ngraphed:\n", seen[True].cpu())
    assert bool(torch.isfinite(seen[False]).all()) and bool(torch.isfinite(seen[True]).all())
    assert rel_err(seen[True], seen[False]) <= 1e-5


def test_model_captured_trainer_equals_the_eager_trainer(A):
    model = _ms_ssim_vae(A)
    twin = copy.deepcopy(model)
    xs, es = _batches()
    t_graph = A.HipTrainer(model, batch_shape=(B, *IMG), use_graph=True)
    t_eager = A.HipTrainer(twin, batch_shape=(B, *IMG), use_graph=False)
    p0 = t_graph.pflat.clone()
    for x, eps in zip(xs, es):
        a, b = t_graph.step(x, eps), t_eager.step(x, eps)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (a, b)
    assert torch.equal(t_graph.pflat, t_eager.pflat) and not torch.equal(t_graph.pflat, p0)
    assert t_graph.skipped_steps == 0 and t_eager.skipped_steps == 0
    t_graph.close(); t_eager.close()
