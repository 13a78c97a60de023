"""CPU: the host side of the MMD prior -- exports, the constructor and its refusals, the refusal of bad shapes, dtypes and host tensors
before any kernel, the fake (meta) implementations' shapes and the dispatcher registration of ``otvae::mmd_prior`` /
``otvae::mmd_prior_backward`` (Autograd and CUDA kernels, no CPU kernel).  No kernel runs here."""
import inspect

import pytest
import torch

import ot_vae_lightning_amd as A
from ot_vae_lightning_amd import ops

SCALES = [0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0]


def test_prior_and_functional_are_exported():
    from ot_vae_lightning_amd import ot, prior
    from ot_vae_lightning_amd.ot import w2_utils
    from ot_vae_lightning_amd.prior import mmd
    assert A.MMDPrior is prior.MMDPrior is mmd.MMDPrior
    assert issubclass(A.MMDPrior, A.Prior)
    assert A.mmd2 is ot.mmd2 is w2_utils.mmd2
    assert "mmd2" in w2_utils.__all__ and "sliced_w2" in w2_utils.__all__
    assert "mmd_prior" in ops.OPS


def test_constructor_defaults_and_contract():
    p = A.MMDPrior()
    assert p.kernel == "imq" and p.scales == tuple(SCALES) and p.sigma2 == 1.0 and p.unbiased is True
    assert p.loss_coeff == 1.0 and p.annealing_steps == 0 and p.seed is None
    p = A.MMDPrior(kernel="rbf", scales=[1, 2], sigma2=2.0, unbiased=False, loss_coeff=0.25, annealing_steps=10, seed=3)
    assert (p.kernel, p.scales, p.sigma2, p.unbiased, p.loss_coeff, p.annealing_steps, p.seed) == ("rbf", (1.0, 2.0), 2.0, False, 0.25, 10, 3)
    assert p.out_size((16, 1, 1)) == (16, 1, 1)            # a deterministic encoder: the latent has the encoder's shape
    assert p.sample((5, 16), "cpu").shape == (5, 16)
    assert p.annealing(0) == 0.0 and p.annealing(10) == 1
    assert not list(p.parameters()) and not list(p.buffers())
    assert list(inspect.signature(p.forward).parameters) == ["x", "step", "prior_samples"]
    assert list(inspect.signature(A.MMDPrior.__init__).parameters) == ["self", "kernel", "scales", "sigma2", "unbiased", "loss_coeff",
                                                                       "annealing_steps", "seed"]
    assert list(inspect.signature(A.mmd2).parameters) == ["z", "y", "kernel", "scales", "sigma2", "unbiased"]


@pytest.mark.parametrize("kw", [{"kernel": "laplace"}, {"kernel": 0}, {"scales": ()}, {"scales": tuple(range(1, 10))}, {"scales": (1.0, 0.0)},
                                {"scales": (-1.0,)}, {"scales": 3.0}, {"sigma2": 0.0}, {"sigma2": -2.0}])
def test_constructor_and_functional_refuse_a_bad_configuration(kw):
    with pytest.raises(ValueError, match="mmd"):
        A.MMDPrior(**kw)
    z = torch.zeros(6, 5)
    with pytest.raises(ValueError, match="mmd"):   # host tensors: the configuration is refused first
        A.mmd2(z, z, **kw)


def test_shape_and_dtype_refusals_come_before_any_kernel():
    p = A.MMDPrior()
    z = torch.zeros(6, 5)
    with pytest.raises(ValueError, match="widths"):
        p(z, step=0, prior_samples=torch.zeros(7, 4))           # another D
    with pytest.raises(ValueError, match="prior_samples"):
        p(z, step=0, prior_samples=torch.zeros(5))
    with pytest.raises(ValueError, match="N, M >= 2"):
        p(torch.zeros(1, 5), step=0)                            # the unbiased estimator needs two latents ...
    with pytest.raises(ValueError, match="N, M >= 2"):
        p(z, step=0, prior_samples=torch.zeros(1, 5))           # ... and two draws
    with pytest.raises(ValueError, match="N, M >= 1"):
        A.MMDPrior(unbiased=False)(torch.zeros(0, 5), step=0)
    with pytest.raises(NotImplementedError, match="float32"):
        p(z.double(), step=0)
    with pytest.raises(NotImplementedError, match="float32"):
        p(z.half(), step=0, prior_samples=torch.zeros(9, 5))
    with pytest.raises(NotImplementedError, match="512"):       # the envelope, known on the host
        p(torch.zeros(4, 513), step=0)
    z4 = torch.zeros(6, 5, 1, 1)                                # latents are flattened; any M of draws is fine ...
    with pytest.raises(RuntimeError, match="MI355X"):          # ... and gets as far as the refusal of host tensors
        p(z4, step=0, prior_samples=torch.zeros(9, 5))
    with pytest.raises(RuntimeError, match="MI355X"):          # the biased estimator takes a single latent
        A.MMDPrior(unbiased=False)(torch.zeros(1, 5), step=0, prior_samples=torch.zeros(1, 5))


def test_functional_refuses_bad_shapes_and_host_tensors():
    z = torch.zeros(6, 5)
    with pytest.raises(ValueError, match="mmd"):
        A.mmd2(torch.zeros(6), z)
    with pytest.raises(ValueError, match="mmd"):
        A.mmd2(z, torch.zeros(2, 6, 5))
    with pytest.raises(ValueError, match="widths"):
        A.mmd2(z, torch.zeros(6, 4))
    with pytest.raises(ValueError, match="N, M >= 2"):
        A.mmd2(z, torch.zeros(1, 5))
    with pytest.raises(NotImplementedError, match="float32"):
        A.mmd2(z.double(), z)
    with pytest.raises(RuntimeError, match="MI355X"):
        A.mmd2(z, torch.zeros(9, 5))
    with pytest.raises(RuntimeError, match="MI355X"):
        A.MMDPrior()(z, step=0)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.otvae.mmd_prior(z, z, 0, SCALES, 1.0, True, 1.0, True)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.otvae.mmd_prior_backward(torch.zeros(6), None, z)


@pytest.mark.parametrize("n,m,d", [(2, 2, 1), (7, 5, 5), (64, 97, 16)])
def test_fake_implementations_give_the_kernels_shapes(n, m, d):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        z, y = torch.empty((n, d), device="cuda"), torch.empty((m, d), device="cuda")
        loss, G, terms = torch.ops.otvae.mmd_prior(z, y, 0, SCALES, 1.0, True, 0.5, True)
        assert loss.shape == (n,) and G.shape == (n, d) and terms.shape == (3,)
        assert loss.dtype == G.dtype == terms.dtype == torch.float32 and loss.device.type == "cuda"
        loss, G0, terms = torch.ops.otvae.mmd_prior(z, y, 1, [1.0], 2.0, False, 0.5, False)
        assert loss.shape == (n,) and G0.shape == (0, d) and terms.shape == (3,)
        for gadd in (None, torch.empty((n, d), device="cuda")):
            gz = torch.ops.otvae.mmd_prior_backward(loss, gadd, G)
            assert gz.shape == z.shape and gz.dtype == torch.float32 and gz.is_contiguous()


def test_both_ops_have_autograd_and_cuda_kernels_and_no_cpu_kernel():
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    for name in ("mmd_prior", "mmd_prior_backward"):
        op = getattr(torch.ops.otvae, name).default
        assert op._schema.name == f"otvae::{name}"
        assert has(f"otvae::{name}", "Autograd"), name
        assert has(f"otvae::{name}", "CUDA"), name
        assert not has(f"otvae::{name}", "CPU"), name
    assert str(torch.ops.otvae.mmd_prior.default._schema) == \
        "otvae::mmd_prior(Tensor z, Tensor y, int kernel, float[] scales, float sigma2, bool unbiased, float scale, bool need_grad) " \
        "-> (Tensor, Tensor, Tensor)"
    assert str(torch.ops.otvae.mmd_prior_backward.default._schema) == \
        "otvae::mmd_prior_backward(Tensor g, Tensor? gadd, Tensor G) -> Tensor"


def test_abi_rows_are_declared():
    from ot_vae_lightning_amd import _lib
    for name in ("otvae_mmd_ws", "otvae_mmd_fwd", "otvae_mmd_bwd"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["otvae_mmd_ws"][1]) == 3
    assert len(_lib.SIGNATURES["otvae_mmd_fwd"][1]) == 17 and len(_lib.SIGNATURES["otvae_mmd_bwd"][1]) == 8
