"""CPU: the host side of the sliced Wasserstein-2 prior -- exports, the constructor and its refusals, the refusal of host tensors, the
fake (meta) implementations' shapes and the dispatcher registration of ``otvae::sliced_w2`` / ``otvae::sliced_w2_backward`` (Autograd
and CUDA kernels, no CPU kernel).  No kernel runs here."""
import pytest
import torch

import ot_vae_lightning_amd as A
from ot_vae_lightning_amd import ops


def test_prior_and_functional_are_exported():
    from ot_vae_lightning_amd import ot, prior
    from ot_vae_lightning_amd.ot import w2_utils
    from ot_vae_lightning_amd.prior import sliced
    assert A.SlicedWassersteinPrior is prior.SlicedWassersteinPrior is sliced.SlicedWassersteinPrior
    assert issubclass(A.SlicedWassersteinPrior, A.Prior)
    assert A.sliced_w2 is ot.sliced_w2 is w2_utils.sliced_w2
    assert "sliced_w2" in w2_utils.__all__ and "sinkhorn_log" in w2_utils.__all__
    assert "sliced_w2" in ops.OPS


def test_constructor_defaults_and_contract():
    p = A.SlicedWassersteinPrior()
    assert p.n_projections == 128 and p.loss_coeff == 1.0 and p.annealing_steps == 0 and p.seed is None
    p = A.SlicedWassersteinPrior(n_projections=7, loss_coeff=0.25, annealing_steps=10, seed=3)
    assert (p.n_projections, p.loss_coeff, p.annealing_steps, p.seed) == (7, 0.25, 10, 3)
    assert p.out_size((16, 1, 1)) == (16, 1, 1)            # a deterministic encoder: the latent has the encoder's shape
    assert p.sample((5, 16), "cpu").shape == (5, 16)
    assert p.annealing(0) == 0.0 and p.annealing(10) == 1
    assert not list(p.parameters()) and not list(p.buffers())
    import inspect
    assert list(inspect.signature(p.forward).parameters) == ["x", "step", "prior_samples", "projections"]


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, None])
def test_constructor_refuses_a_bad_projection_count(bad):
    with pytest.raises(ValueError, match="n_projections"):
        A.SlicedWassersteinPrior(n_projections=bad)


def test_shape_and_dtype_refusals_come_before_any_kernel():
    p = A.SlicedWassersteinPrior(n_projections=4)
    z = torch.zeros(6, 5)
    with pytest.raises(ValueError, match="prior_samples"):
        p(z, step=0, prior_samples=torch.zeros(7, 5))           # another N
    with pytest.raises(ValueError, match="prior_samples"):
        p(z, step=0, prior_samples=torch.zeros(6, 4))           # another D
    with pytest.raises(ValueError, match="projections"):
        p(z, step=0, projections=torch.zeros(4, 6))             # not [L, D]
    with pytest.raises(ValueError, match="projections"):
        p(z, step=0, projections=torch.zeros(5))
    with pytest.raises(NotImplementedError, match="float32"):
        p(z.double(), step=0)
    with pytest.raises(NotImplementedError, match="float32"):
        p(z.half(), step=0, prior_samples=torch.zeros(6, 5), projections=torch.zeros(4, 5))
    z4 = torch.zeros(6, 5, 1, 1)                                # latents are flattened: [B, C, 1, 1] against [B, C] draws is fine ...
    with pytest.raises(RuntimeError, match="MI355X"):          # ... and gets as far as the refusal of host tensors
        p(z4, step=0, prior_samples=torch.zeros(6, 5), projections=torch.zeros(4, 5))


def test_cpu_tensors_are_refused():
    z, y, g = torch.zeros(6, 5), torch.zeros(6, 5), torch.ones(4, 5)
    with pytest.raises(RuntimeError, match="MI355X"):
        A.SlicedWassersteinPrior(4)(z, step=0)
    with pytest.raises(RuntimeError, match="MI355X"):
        A.sliced_w2(z, y, projections=g)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.otvae.sliced_w2(z, y, g, 1.0)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.otvae.sliced_w2_backward(torch.zeros(6), None, torch.zeros(4, 6), g, 1.0)


def test_functional_refuses_bad_shapes():
    with pytest.raises(RuntimeError, match="MI355X"):
        A.sliced_w2(torch.zeros(6, 5), torch.zeros(6, 5))
    z = torch.empty(6, 5, device="meta")
    for args, kw in (((z, torch.empty(7, 5, device="meta")), {}), ((z, z), {"projections": torch.empty(4, 6, device="meta")}),
                     ((z, z), {"n_projections": 0})):
        with pytest.raises(ValueError, match="sliced_w2"):
            A.sliced_w2(*args, **kw)


@pytest.mark.parametrize("n,d,nl", [(1, 4, 1), (7, 5, 3), (64, 16, 8)])
def test_fake_implementations_give_the_kernels_shapes(n, d, nl):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        z, y, g = (torch.empty(s, device="cuda") for s in ((n, d), (n, d), (nl, d)))
        loss, resid, theta = torch.ops.otvae.sliced_w2(z, y, g, 0.5)
        assert loss.shape == (n,) and resid.shape == (nl, n) and theta.shape == (nl, d)
        assert loss.dtype == resid.dtype == theta.dtype == torch.float32 and loss.device.type == "cuda"
        for gadd in (None, torch.empty((n, d), device="cuda")):
            gz = torch.ops.otvae.sliced_w2_backward(loss, gadd, resid, theta, 0.5)
            assert gz.shape == z.shape and gz.dtype == torch.float32 and gz.is_contiguous()


def test_both_ops_have_autograd_and_cuda_kernels_and_no_cpu_kernel():
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    for name in ("sliced_w2", "sliced_w2_backward"):
        op = getattr(torch.ops.otvae, name).default
        assert op._schema.name == f"otvae::{name}"
        assert has(f"otvae::{name}", "Autograd"), name
        assert has(f"otvae::{name}", "CUDA"), name
        assert not has(f"otvae::{name}", "CPU"), name
    assert str(torch.ops.otvae.sliced_w2.default._schema) == \
        "otvae::sliced_w2(Tensor z, Tensor y, Tensor dirs, float scale) -> (Tensor, Tensor, Tensor)"
    assert str(torch.ops.otvae.sliced_w2_backward.default._schema) == \
        "otvae::sliced_w2_backward(Tensor g, Tensor? gadd, Tensor resid, Tensor theta, float scale) -> Tensor"


def test_abi_rows_are_declared():
    from ot_vae_lightning_amd import _lib
    for name in ("otvae_sliced_w2_ws", "otvae_sliced_w2_fwd", "otvae_sliced_w2_bwd"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["otvae_sliced_w2_fwd"][1]) == 13 and len(_lib.SIGNATURES["otvae_sliced_w2_bwd"][1]) == 10
