"""CPU: the host side of ``SSIMLoss`` / ``ssim_loss`` -- exports, option refusals, the empty ``state_dict``, the ``VAE(ssim_loss=...)``
keyword, the two operators' registration and fake implementations, and the two C-ABI entries of the gradient kernel.  The loss has no
host path; ``tests/test_gpu_ssim_loss.py`` drives it."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports():
    import ot_vae_lightning_amd as A
    from ot_vae_lightning_amd import losses
    assert losses.__all__ == ["SSIMLoss", "ssim_loss"]
    assert A.SSIMLoss is losses.SSIMLoss and A.ssim_loss is losses.ssim_loss and A.losses is losses
    m = A.SSIMLoss()
    assert m.window_size == (11, 11) and m.reduction == "mean" and m.options.range_mode == 0 and m.options.range_hi == 1.0
    assert A.SSIMLoss(data_range=(0.25, 0.75)).options.range_mode == 1
    assert A.SSIMLoss(sigma=(1.0, 2.0)).window_size == (9, 15)
    assert A.SSIMLoss(gaussian_kernel=False, kernel_size=(3, 5)).window_size == (3, 5)
    assert "data_range=1.0" in repr(m)


def test_option_refusals():
    from ot_vae_lightning_amd import SSIMLoss, ssim_loss
    x = torch.rand(2, 1, 16, 16)
    for bad in (dict(reduction="elementwise_mean"), dict(reduction=None), dict(gaussian_kernel=False, kernel_size=8), dict(kernel_size=(11, 4)),
                dict(sigma=0.0), dict(data_range=(1.0, 0.5)), dict(data_range=(0.5, 0.5)), dict(data_range=0.0), dict(k1=-1.0)):
        with pytest.raises(ValueError):
            SSIMLoss(**bad)
        with pytest.raises(ValueError):
            ssim_loss(x, x, **bad)
    with pytest.raises(ValueError, match="data_range=None"):
        SSIMLoss(data_range=None)
    with pytest.raises(ValueError, match="fixed scale"):
        ssim_loss(x, x, data_range=None)
    m = SSIMLoss()
    for p, t in ((x[0], x[0]), (x, torch.rand(2, 1, 16, 17)), (torch.rand(1, 1, 10, 16), torch.rand(1, 1, 10, 16))):
        with pytest.raises(ValueError):
            m(p, t)
    with pytest.raises(RuntimeError):       # no CPU path: the dispatcher refuses host tensors (NotImplementedError is a RuntimeError)
        m(x, x)
    with pytest.raises(RuntimeError):
        ssim_loss(x, x)


def test_module_holds_no_state():
    from ot_vae_lightning_amd import SSIMLoss
    m = SSIMLoss(data_range=(0.0, 1.0), reduction="sum")
    assert list(m.state_dict()) == [] and list(m.parameters()) == [] and list(m.buffers()) == []


def _vae(A, **kw):
    torch.manual_seed(3)
    enc = A.CNN(1, 16, 16, 1, capacity=4, down_sample=True, residual="add")
    dec = A.CNN(8, 1, 1, 16, capacity=4, up_sample=True, residual="add")
    return A.VAE(encoder=enc, decoder=dec, prior=A.GaussianPrior(loss_coeff=0.1), **kw)


def test_vae_keyword_leaves_the_state_dict_alone():
    import ot_vae_lightning_amd as A
    bare, none, with_loss = _vae(A), _vae(A, ssim_loss=None), _vae(A, ssim_loss=A.SSIMLoss(), ssim_weight=0.5)
    assert list(bare.state_dict()) == list(none.state_dict()) == list(with_loss.state_dict())
    assert bare.ssim_loss is None and none.ssim_loss is None and with_loss.ssim_weight == 0.5
    assert not hasattr(bare, "_ssim_mask") and with_loss._ssim_mask.tolist() == [1.0, 1.0, 0.0]
    assert [n for n, _ in with_loss.named_buffers() if "ssim" in n] == ["_ssim_mask"]
    assert len(list(bare.optim_parameters())) == len(list(with_loss.optim_parameters()))
    with pytest.raises(ValueError, match="reduction"):
        _vae(A, ssim_loss=A.SSIMLoss(reduction="none"))


def test_operators_and_fake_implementations():
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "ssim_loss" in ops.OPS and "otvae::ssim_loss " in ops.__doc__
    for name in ("ssim_loss", "ssim_loss_backward"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{name}", "CUDA"), name
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{name}", "Autograd"), name
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{name}", "CPU"), name
    schema = str(torch.ops.otvae.ssim_loss.default._schema)
    assert schema.endswith("-> Tensor") and "float[] win_h" in schema and "(a!)" not in schema, schema
    win = [1.0 / 11] * 11
    p = torch.empty(5, 3, 32, 40, device="meta")
    out = torch.ops.otvae.ssim_loss(p, p, win, win, 0.01, 0.03, 0, 0.0, 1.0)
    assert out.shape == (5,) and out.dtype == torch.float64 and out.device.type == "meta"
    g = torch.empty(5, dtype=torch.float64, device="meta")
    for dtype in (torch.float32, torch.float64):
        q = p.to(dtype)
        grad = torch.ops.otvae.ssim_loss_backward(g, q, q, win, win, 0.01, 0.03, 0, 0.0, 1.0)
        assert grad.shape == q.shape and grad.dtype == dtype
    with FakeTensorMode():
        x = torch.empty(4, 1, 16, 16, device="cuda", requires_grad=True)
        loss = torch.ops.otvae.ssim_loss(x, torch.empty(4, 1, 16, 16, device="cuda"), win, win, 0.01, 0.03, 0, 0.0, 1.0)
        assert loss.shape == (4,) and loss.dtype == torch.float64 and loss.requires_grad and loss.grad_fn is not None
        gx = torch.ops.otvae.ssim_loss_backward(torch.empty(4, dtype=torch.float64, device="cuda"), x.detach(), x.detach(), win, win, 0.01,
                                                0.03, 0, 0.0, 1.0)
        assert gx.shape == x.shape and gx.dtype == torch.float32


def test_entries_in_header_binding_and_library():
    from ot_vae_lightning_amd import _lib, build
    names = ("otvae_ssim_grad", "otvae_ssim_grad_ws")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "otvae.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(otvae_[a-z0-9_]+)\s*\(", hdr))
    lib = build.build(verbose=False)
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert n in declared and n in _lib.SIGNATURES, n
        assert re.search(rf"\bT {n}\b", exported), f"{n} is not exported by {lib}"
    assert _lib.SIGNATURES["otvae_ssim_grad"][1][:16] == _lib.SIGNATURES["otvae_ssim_accum"][1][:16]   # the shared leading arguments
    handle = _lib.load()
    # one launch, everything in LDS: no workspace inside the envelope (odd windows of up to 15 taps per axis), -1 outside
    for ok in ((1, 1, 11, 11, 11, 11), (1024, 1, 32, 32, 11, 11), (2, 2, 75, 70, 3, 5), (2, 2, 40, 45, 9, 15), (1, 1, 15, 15, 15, 15),
               (3, 2, 20, 40, 1, 1)):
        assert handle.otvae_ssim_grad_ws(*ok) == 0, ok
    for refused in ((0, 1, 32, 32, 11, 11), (1, 0, 32, 32, 11, 11), (1, 1, 10, 32, 11, 11), (1, 1, 32, 10, 11, 11), (1, 1, 32, 32, 10, 11),
                    (1, 1, 32, 32, 11, 0), (1, 1, 64, 64, 17, 11), (1, 1, 64, 64, 11, 17), (1 << 30, 64, 64, 64, 11, 11)):
        assert handle.otvae_ssim_grad_ws(*refused) == -1, refused
