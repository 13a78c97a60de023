"""GPU: the pass-through loss node of the minibatch priors (``prior/base.py``), once per prior (run with ``-m gpu``).

Every deterministic-encoder prior returns its latents through the node that computes its loss (an alias of z), so that the gradient
the decoder sends back is added inside the prior's backward kernel.  What that promises, at the smallest shapes that exercise it:
z_out is z's memory; loss is [N] with equal entries; the gradient through the loss alone is ``own``; through the latents alone it is
the incoming gradient itself, untouched (nothing launched, nothing added); through both it is their sum.

Bound of the sum, per element: MMD's kernel does one fp32 addition to the rounded product, so ``torch.equal``.  The other kernels
may fuse the addition into a multiply-add, so the product is not rounded on its own: one rounding of the product not taken plus one
of the sum, each at most 1 ulp of the larger operand, doubled for slack = 4 fp32 ulps of max(|w|, |own|, |w + own|)."""
import pytest
import torch

from detfill import normal

pytestmark = pytest.mark.gpu

KINDS = ["sinkhorn", "sliced", "mmd", "gaussian_w2"]


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd as pkg
    return pkg


def _case(A, kind):
    """(prior, z [N, D] on the device, the keywords that hand every draw in, w [N, D])"""
    n, d = (9, 4) if kind == "gaussian_w2" else (7, 5)
    z, w = normal((n, d), 500).cuda(), normal((n, d), 501).cuda()
    if kind == "sinkhorn":
        return A.SinkhornPrior(loss_coeff=0.5).cuda(), z, {"prior_samples": normal((n, d), 502).cuda()}, w
    if kind == "sliced":
        kw = {"prior_samples": normal((n, d), 502).cuda(), "projections": normal((3, d), 503).cuda()}
        return A.SlicedWassersteinPrior(n_projections=3, loss_coeff=0.5).cuda(), z, kw, w
    if kind == "mmd":
        return A.MMDPrior(loss_coeff=0.5).cuda(), z, {"prior_samples": normal((5, d), 502).cuda()}, w
    # evaluation mode: in training mode this prior carries its warm-start basis from call to call (the last test)
    return A.GaussianW2Prior(loss_coeff=0.5).cuda().eval(), z, {}, w


def _grad(prior, z, kw, w, through_loss, through_latents):
    zl = z.clone().requires_grad_(True)
    z_out, loss, _ = prior(zl, step=0, **kw)
    total = 0
    if through_loss:
        total = total + loss.mean()
    if through_latents:
        total = total + (z_out * w).sum()
    total.backward()
    return zl.grad


def _ulp32(x):
    """the fp32 unit in the last place at |x| (float64 tensor in, float64 out)"""
    return torch.ldexp(torch.ones_like(x), torch.frexp(x.abs().clamp_min(2.0 ** -126))[1] - 24)


@pytest.mark.parametrize("kind", KINDS)
def test_latents_leave_as_an_alias_and_the_loss_is_one_value_per_sample(A, kind):
    prior, z, kw, _ = _case(A, kind)
    zl = z.clone().requires_grad_(True)
    z_out, loss, _ = prior(zl, step=0, **kw)
    assert z_out.shape == zl.shape and z_out.data_ptr() == zl.data_ptr()
    assert loss.shape == (z.shape[0],) and bool((loss == loss[0]).all()) and bool(torch.isfinite(loss).all())
    assert loss.requires_grad and z_out.requires_grad
    # the same inputs again: the same bits; without a graph: the same bits, and nothing to differentiate
    _, again, _ = prior(zl, step=0, **kw)
    assert torch.equal(again, loss)
    with torch.no_grad():
        _, plain, _ = prior(zl, step=0, **kw)
    assert torch.equal(plain, loss) and not plain.requires_grad


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_through_loss_latents_and_both(A, kind):
    prior, z, kw, w = _case(A, kind)
    own = _grad(prior, z, kw, w, True, False)
    assert own.shape == z.shape and bool(torch.isfinite(own).all()) and float(own.abs().max()) > 0
    # only the latents were used downstream: the incoming gradient comes back as it is
    assert torch.equal(_grad(prior, z, kw, w, False, True), w)
    both = _grad(prior, z, kw, w, True, True)
    if kind == "mmd":
        assert torch.equal(both, w + own)
        return
    both, w, own = both.double().cpu(), w.double().cpu(), own.double().cpu()
    want = w + own
    excess = (both - want).abs() / _ulp32(torch.maximum(torch.maximum(w.abs(), own.abs()), want.abs()))
    print(f"{kind}: |both - (w + own)| is at most {float(excess.max()):.3f} fp32 ulps of max(|w|, |own|, |w + own|)")
    assert float(excess.max()) <= 4.0


def test_gaussian_w2_refreshes_its_warm_start_basis_behind_the_solve(A):
    """training mode: the first call solves cold and leaves its eigenvectors as the next call's start basis -- one path, eager or
    on the prior lane, with or without a graph"""
    _, z, kw, w = _case(A, "gaussian_w2")
    prior = A.GaussianW2Prior(loss_coeff=0.5).cuda().train()
    assert int(prior._warm) == 0 and prior._v_prev is None
    with torch.no_grad():
        _, first, _ = prior(z, step=0)
    assert int(prior._warm) == 1
    basis = prior._v_prev.clone()
    assert basis.shape == (1, 4, 4) and bool(torch.isfinite(basis).all()) and float(basis.abs().max()) > 0
    zl = z.clone().requires_grad_(True)
    z_out, second, _ = prior(zl, step=0)          # the warm solve, with a graph this time
    assert int(prior._warm) == 1 and bool(torch.isfinite(prior._v_prev).all()) and float(prior._v_prev.abs().max()) > 0
    assert z_out.data_ptr() == zl.data_ptr()
    # the same distance from another start basis: the fp64 solves agree to ~1e-15, the fp32 loss to its last bit or two (1.2e-7)
    assert bool(torch.isfinite(second).all()) and torch.allclose(second, first, rtol=1e-6, atol=0)
    (z_out * w).sum().backward()
    assert torch.equal(zl.grad, w)
