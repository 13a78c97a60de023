"""CPU: the host side of the Sinkhorn-divergence prior -- exports, the constructor and the signatures, the refusals of bad shapes,
configurations, dtypes and host tensors before any kernel, the fake (meta) implementations' shapes and dtypes, the dispatcher
registration of ``otvae::sinkhorn_divergence`` / ``otvae::sinkhorn_divergence_backward`` (Autograd and CUDA kernels, no CPU kernel) and
the three C entry points.  No kernel runs here."""
import ctypes
import inspect

import pytest
import torch

import ot_vae_lightning_amd as A
from ot_vae_lightning_amd import ops


def test_prior_and_functional_are_exported():
    from ot_vae_lightning_amd import ot, prior
    from ot_vae_lightning_amd.ot import w2_utils
    from ot_vae_lightning_amd.prior import sinkhorn_divergence as mod
    assert A.SinkhornDivergencePrior is prior.SinkhornDivergencePrior is mod.SinkhornDivergencePrior
    assert issubclass(A.SinkhornDivergencePrior, prior.MinibatchPrior) and issubclass(A.SinkhornDivergencePrior, A.Prior)
    assert A.sinkhorn_divergence is ot.sinkhorn_divergence is w2_utils.sinkhorn_divergence
    assert "sinkhorn_divergence" in w2_utils.__all__ and "mmd2" in w2_utils.__all__
    assert ops.OPS[-1] == "sinkhorn_divergence" and "otvae::sinkhorn_divergence " in ops.__doc__


def test_constructor_defaults_and_contract():
    p = A.SinkhornDivergencePrior()
    assert (p.reg, p.max_iter, p.loss_coeff, p.annealing_steps, p.seed, p.last_iters) == (0.05, 50, 1.0, 0, None, None)
    assert not hasattr(p, "threshold")
    p.raise_if_starved()                                   # nothing has run: nothing to read
    p = A.SinkhornDivergencePrior(reg=0.1, max_iter=20, loss_coeff=0.25, annealing_steps=10, seed=3)
    assert (p.reg, p.max_iter, p.loss_coeff, p.annealing_steps, p.seed) == (0.1, 20, 0.25, 10, 3)
    assert p.out_size((16, 1, 1)) == (16, 1, 1)            # a deterministic encoder: the latent has the encoder's shape
    assert p.sample((5, 16), "cpu").shape == (5, 16)
    assert p.annealing(0) == 0.0 and 0.0 < p.annealing(5) < 1.0 and p.annealing(10) == 1
    assert not list(p.parameters()) and not list(p.buffers()) and not p.state_dict()
    assert list(inspect.signature(p.forward).parameters) == ["x", "step", "prior_samples"]
    assert list(inspect.signature(A.SinkhornDivergencePrior.__init__).parameters) == ["self", "reg", "max_iter", "loss_coeff",
                                                                                      "annealing_steps", "seed"]
    sig = inspect.signature(A.sinkhorn_divergence)
    assert list(sig.parameters) == ["z", "y", "reg", "max_iter"]
    assert sig.parameters["reg"].default == 0.05 and sig.parameters["max_iter"].default == 50


@pytest.mark.parametrize("kw", [{"reg": 0.0}, {"reg": -0.05}, {"reg": float("nan")}, {"max_iter": -1}])
def test_a_bad_configuration_is_refused(kw):
    with pytest.raises(ValueError, match="sinkhorn_divergence"):
        A.SinkhornDivergencePrior(**kw)
    z = torch.zeros(6, 5)
    with pytest.raises(ValueError, match="sinkhorn_divergence"):   # host tensors: the configuration is refused first
        A.sinkhorn_divergence(z, z, **kw)
    p = A.SinkhornDivergencePrior()
    for k, v in kw.items():
        setattr(p, k, v)                                           # changed after construction: refused at the call
    with pytest.raises(ValueError, match="sinkhorn_divergence"):
        p(z, step=0, prior_samples=z)


def test_shape_and_dtype_refusals_come_before_any_kernel():
    p = A.SinkhornDivergencePrior()
    z = torch.zeros(6, 5)
    with pytest.raises(ValueError, match="widths"):
        p(z, step=0, prior_samples=torch.zeros(7, 4))           # another D
    with pytest.raises(ValueError, match="prior_samples"):
        p(z, step=0, prior_samples=torch.zeros(5))              # not 2-D
    with pytest.raises(ValueError, match="latents"):
        p(torch.zeros(6), step=0)
    with pytest.raises(ValueError, match="N, M, D >= 1"):
        p(torch.zeros(0, 5), step=0)
    with pytest.raises(ValueError, match="N, M, D >= 1"):
        p(z, step=0, prior_samples=torch.zeros(0, 5))
    with pytest.raises(TypeError, match="float32 or float64"):
        p(z.half(), step=0)
    with pytest.raises(TypeError, match="float32 or float64"):
        p(z.to(torch.bfloat16), step=0, prior_samples=torch.zeros(9, 5))
    z4 = torch.zeros(6, 5, 1, 1)                                # latents are flattened; any M of draws is fine ...
    with pytest.raises(RuntimeError, match="MI355X"):          # ... and gets as far as the refusal of host tensors
        p(z4, step=0, prior_samples=torch.zeros(9, 5))
    with pytest.raises(RuntimeError, match="MI355X"):
        p(z.double(), step=0)                                   # float64 is computed, not refused
    with pytest.raises(RuntimeError, match="MI355X"):
        p(torch.zeros(1, 1), step=0, prior_samples=torch.zeros(1, 1))   # N = M = D = 1 is a problem like any other


def test_functional_refuses_bad_shapes_and_host_tensors():
    z = torch.zeros(6, 5)
    with pytest.raises(ValueError, match="sinkhorn_divergence"):
        A.sinkhorn_divergence(torch.zeros(6), z)
    with pytest.raises(ValueError, match="sinkhorn_divergence"):
        A.sinkhorn_divergence(z, torch.zeros(2, 6, 5))
    with pytest.raises(ValueError, match="widths"):
        A.sinkhorn_divergence(z, torch.zeros(6, 4))
    with pytest.raises(TypeError, match="float32 or float64"):
        A.sinkhorn_divergence(z.half(), z.half())
    with pytest.raises(RuntimeError, match="MI355X"):
        A.sinkhorn_divergence(z, torch.zeros(9, 5))
    with pytest.raises(RuntimeError, match="MI355X"):
        A.sinkhorn_divergence(z.double(), z.double(), reg=0.5, max_iter=0)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.otvae.sinkhorn_divergence(z, z, 0.05, 50, 1.0)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.otvae.sinkhorn_divergence_backward(torch.zeros(6), None, z, z, torch.zeros(6, 6), torch.zeros(6, 6), 1.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("n,m,d", [(1, 1, 1), (7, 5, 5), (64, 97, 16)])
def test_fake_implementations_give_the_kernels_shapes(n, m, d, dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        z, y = torch.empty((n, d), device="cuda", dtype=dtype), torch.empty((m, d), device="cuda", dtype=dtype)
        loss, terms, pi_zy, pi_zz, iters = torch.ops.otvae.sinkhorn_divergence(z, y, 0.05, 50, 0.5)
        assert loss.shape == (n,) and terms.shape == (3,) and pi_zy.shape == (n, m) and pi_zz.shape == (n, n) and iters.shape == (1,)
        assert loss.dtype == pi_zy.dtype == pi_zz.dtype == dtype and terms.dtype == torch.float64 and iters.dtype == torch.int32
        assert all(t.device.type == "cuda" for t in (loss, terms, pi_zy, pi_zz, iters))
        for gadd in (None, torch.empty((n, d), device="cuda", dtype=dtype)):
            gz = torch.ops.otvae.sinkhorn_divergence_backward(loss, gadd, z, y, pi_zy, pi_zz, 0.5)
            assert gz.shape == z.shape and gz.dtype == dtype and gz.is_contiguous()


def test_both_ops_have_autograd_and_cuda_kernels_and_no_cpu_kernel():
    has = torch._C._dispatch_has_kernel_for_dispatch_key
    for name in ("sinkhorn_divergence", "sinkhorn_divergence_backward"):
        op = getattr(torch.ops.otvae, name).default
        assert op._schema.name == f"otvae::{name}"
        assert has(f"otvae::{name}", "Autograd"), name
        assert has(f"otvae::{name}", "CUDA"), name
        assert not has(f"otvae::{name}", "CPU"), name
    assert str(torch.ops.otvae.sinkhorn_divergence.default._schema) == \
        "otvae::sinkhorn_divergence(Tensor z, Tensor y, float reg, int max_iter, float scale) -> (Tensor, Tensor, Tensor, Tensor, Tensor)"
    assert str(torch.ops.otvae.sinkhorn_divergence_backward.default._schema) == \
        "otvae::sinkhorn_divergence_backward(Tensor g, Tensor? gadd, Tensor z, Tensor y, Tensor pi_zy, Tensor pi_zz, float scale) -> Tensor"


def test_the_three_entry_points_are_declared_and_exported():
    from ot_vae_lightning_amd import _lib, build
    want = {"otvae_sinkhorn_div_ws": 3, "otvae_sinkhorn_div_fwd": 17, "otvae_sinkhorn_div_grad": 14}
    for name, arity in want.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity, name
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in want:
        assert hasattr(lib, name), f"{name} is not exported"
    # the workspace size is a host function: a positive byte count inside the envelope, -1 outside it
    ws = lib.otvae_sinkhorn_div_ws
    ws.restype, ws.argtypes = ctypes.c_int64, [ctypes.c_int] * 3
    assert ws(0, 64, 64) > 0 and ws(1, 7, 5) > 0 and ws(0, 1, 1) > 0
    assert ws(0, 0, 5) == -1 and ws(0, 5, 0) == -1 and ws(2, 5, 5) == -1 and ws(0, 32769, 5) == -1
    assert ws(0, 130, 97) >= 4 * 2 * (130 * 97 + 130 * 130 + 97 * 97)     # the three cost matrices and the three plans
