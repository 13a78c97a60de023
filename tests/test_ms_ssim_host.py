"""CPU: the host side of multi-scale SSIM -- the C-ABI entries in header, binding and library, the operators' registration and fake
implementations, exports, option refusals, the size rule (every scale must hold one window) and the loss's empty ``state_dict``.
There is no host path for the values; ``tests/test_gpu_ms_ssim.py`` and ``tests/test_gpu_ms_ssim_loss.py`` drive the kernels."""
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("otvae_ms_ssim_state_words", "otvae_ms_ssim_pyramid", "otvae_ms_ssim_ws", "otvae_ms_ssim_accum", "otvae_ms_ssim_grad_ws",
           "otvae_ms_ssim_grad")
BETAS3 = (0.0448, 0.2856, 0.3001)


def test_entries_in_header_binding_and_library():
    from ot_vae_lightning_amd import _lib, build
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "otvae.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(otvae_[a-z0-9_]+)\s*\(", hdr))
    lib = build.build(verbose=False)
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for n in ENTRIES:
        assert n in declared and n in _lib.SIGNATURES, n
        assert re.search(rf"\bT {n}\b", exported), f"{n} is not exported by {lib}"
    handle = _lib.load()
    assert handle.otvae_ms_ssim_state_words() == handle.otvae_ssim_state_words()
    # workspace: two doubles per (scale, plane, 16 x 32 tile of positions)
    assert handle.otvae_ms_ssim_ws(2, 3, 45, 43, 3, 5, 4) == 16 * 2 * 3 * (3 * 2 + 2 * 1 + 1 + 1)
    assert handle.otvae_ms_ssim_ws(1, 1, 11, 11, 11, 11, 1) == 16
    # pyramid: scales 1 .. S - 1 of one image tensor, odd rows / columns dropped
    assert handle.otvae_ms_ssim_pyramid(0, 2, 3, 45, 43, 4) == 4 * 6 * (22 * 21 + 11 * 10 + 5 * 5)
    assert handle.otvae_ms_ssim_pyramid(1, 2, 3, 45, 43, 1) == 0
    # gradient workspace: the largest odd and the largest even coarse scale
    assert handle.otvae_ms_ssim_grad_ws(0, 2, 3, 45, 43, 3, 5, 4) == 4 * 6 * (22 * 21 + 11 * 10)
    assert handle.otvae_ms_ssim_grad_ws(1, 1, 1, 32, 32, 5, 5, 2) == 8 * 16 * 16
    assert handle.otvae_ms_ssim_grad_ws(0, 1, 1, 11, 11, 11, 11, 1) == 0
    # refused: nine scales, a scale smaller than the window, an even window, more taps than the kernel has
    for refused in ((1, 1, 4096, 4096, 3, 3, 9), (1, 1, 32, 32, 11, 11, 3), (1, 1, 43, 44, 11, 11, 3), (1, 1, 64, 64, 4, 5, 2),
                    (0, 1, 64, 64, 5, 5, 2), (1, 1, 64, 64, 5, 5, 0), (1, 1, 256, 256, 33, 33, 2)):
        assert handle.otvae_ms_ssim_ws(*refused) == -1, refused
        assert handle.otvae_ms_ssim_grad_ws(0, *refused) == -1, refused
    assert handle.otvae_ms_ssim_ws(1, 1, 44, 44, 11, 11, 3) > 0 and handle.otvae_ms_ssim_ws(1, 1, 124, 124, 31, 31, 3) > 0
    assert handle.otvae_ms_ssim_grad_ws(0, 1, 1, 124, 124, 31, 31, 3) == -1 and handle.otvae_ms_ssim_grad_ws(0, 1, 1, 64, 64, 15, 15, 3) > 0
    assert handle.otvae_ms_ssim_pyramid(0, 1, 1, 64, 64, 9) == -1 and handle.otvae_ms_ssim_pyramid(2, 1, 1, 64, 64, 2) == -1


def test_operators_and_fake_implementations():
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "ms_ssim" in ops.OPS and "otvae::ms_ssim " in ops.__doc__ and "otvae::ms_ssim_accum " in ops.__doc__
    for name in ("ms_ssim", "ms_ssim_backward", "ms_ssim_accum"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{name}", "CUDA"), name
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{name}", "CPU"), name
    for name in ("ms_ssim", "ms_ssim_backward"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{name}", "Autograd"), name
    schema = str(torch.ops.otvae.ms_ssim_accum.default._schema)
    assert "Tensor(a!) state" in schema and "float[] betas" in schema and schema.endswith("-> ()"), schema
    win = [0.2] * 5
    p = torch.empty(5, 3, 45, 43, device="meta")
    ms, w, pyr = torch.ops.otvae.ms_ssim(p, p, win, win, 0.01, 0.03, 0, 0.0, 1.0, list(BETAS3), 1)
    assert ms.shape == (5,) and ms.dtype == torch.float64 and w.shape == (3, 5) and w.dtype == torch.float64
    assert pyr.shape == (2, 15 * (22 * 21 + 11 * 10)) and pyr.dtype == torch.float32
    for dtype in (torch.float32, torch.float64):
        q = p.to(dtype)
        grad = torch.ops.otvae.ms_ssim_backward(ms, w, pyr.to(dtype), q, q, False, win, win, 0.01, 0.03, 0, 0.0, 1.0, list(BETAS3), 1)
        assert grad.shape == q.shape and grad.dtype == dtype
    with FakeTensorMode():
        x = torch.empty(4, 1, 32, 32, device="cuda", requires_grad=True)
        ms, w, pyr = torch.ops.otvae.ms_ssim(x, torch.empty(4, 1, 32, 32, device="cuda"), win, win, 0.01, 0.03, 0, 0.0, 1.0, list(BETAS3), 1)
        assert ms.shape == (4,) and ms.requires_grad and ms.grad_fn is not None and pyr.shape == (2, 4 * (256 + 64))


def test_exports():
    import ot_vae_lightning_amd as A
    from ot_vae_lightning_amd import losses, metrics
    for name in ("MultiScaleStructuralSimilarityIndexMeasure", "multiscale_structural_similarity"):
        assert name in metrics.__all__ and hasattr(metrics, name), name
    assert A.MSSSIMLoss is losses.MSSSIMLoss and A.ms_ssim_loss is losses.ms_ssim_loss
    m = A.MSSSIMLoss()
    assert m.window_size == (11, 11) and m.reduction == "mean" and m.options.range_mode == 0 and m.options.range_hi == 1.0
    assert m.options.betas == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) and m.options.normalize == "relu"
    assert A.MSSSIMLoss(data_range=(0.25, 0.75)).options.range_mode == 1
    assert A.MSSSIMLoss(gaussian_kernel=False, kernel_size=(3, 5)).window_size == (3, 5)
    assert "normalize='relu'" in repr(m) and "data_range=1.0" in repr(m)
    metric = metrics.MultiScaleStructuralSimilarityIndexMeasure()
    assert metric.window_size == (11, 11) and metric.options.range_mode == 2 and metric.reduction == "elementwise_mean"
    assert metric.ms_ssim_state.dtype == torch.float64 and float(metric.total) == 0
    import inspect
    assert list(inspect.signature(metrics.MultiScaleStructuralSimilarityIndexMeasure.__init__).parameters)[1:10] == [
        "gaussian_kernel", "kernel_size", "sigma", "reduction", "data_range", "k1", "k2", "betas", "normalize"]


def test_option_refusals():
    from ot_vae_lightning_amd import MSSSIMLoss, ms_ssim_loss
    from ot_vae_lightning_amd.metrics import MultiScaleStructuralSimilarityIndexMeasure as Metric, multiscale_structural_similarity
    x = torch.rand(2, 1, 64, 64)
    for bad in (dict(betas=()), dict(betas=("a", "b")), dict(betas=[0.5, 0.5]), dict(betas=(1, 2)), dict(betas=0.5), dict(normalize="tanh"),
                dict(normalize=True), dict(sigma=0.0), dict(data_range=(1.0, 0.5)), dict(k1=-1.0)):
        with pytest.raises(ValueError):
            MSSSIMLoss(**bad)
        with pytest.raises(ValueError):
            ms_ssim_loss(x, x, **bad)
        with pytest.raises(ValueError):
            Metric(**bad)
        with pytest.raises(ValueError):
            multiscale_structural_similarity(x, x, **bad)
    with pytest.raises(ValueError, match="data_range=None"):
        MSSSIMLoss(data_range=None)
    with pytest.raises(ValueError, match="fixed scale"):
        ms_ssim_loss(x, x, data_range=None)
    for bad in ("elementwise_mean", None, "avg"):
        with pytest.raises(ValueError, match="reduction"):
            MSSSIMLoss(reduction=bad)
        with pytest.raises(ValueError, match="reduction"):
            ms_ssim_loss(x, x, reduction=bad)
    with pytest.raises(ValueError, match="reduction"):
        Metric(reduction="none")
    for normalize in ("relu", "simple", None):
        assert MSSSIMLoss(normalize=normalize).options.normalize_mode == {"relu": 1, "simple": 2, None: 0}[normalize]


def test_every_scale_must_hold_one_window():
    from ot_vae_lightning_amd import MSSSIMLoss
    from ot_vae_lightning_amd.metrics import MultiScaleStructuralSimilarityIndexMeasure as Metric, multiscale_structural_similarity
    x = torch.rand(2, 1, 32, 32)
    with pytest.raises(ValueError, match="44"):                         # 11 taps, 3 scales: 32 >> 2 = 8 < 11; 11 << 2 = 44
        multiscale_structural_similarity(x, x, betas=BETAS3, data_range=1.0)
    with pytest.raises(ValueError, match="44"):
        Metric(betas=BETAS3, data_range=1.0).update(x, x)
    with pytest.raises(ValueError, match="44"):
        MSSSIMLoss(betas=BETAS3)(x, x)
    # sigma 0.5 is 5 taps: 32 >> 2 = 8 holds it, so the call gets as far as the operator, which has no host kernel
    for call in (lambda: multiscale_structural_similarity(x, x, sigma=0.5, betas=BETAS3, data_range=1.0),
                 lambda: MSSSIMLoss(sigma=0.5, betas=BETAS3)(x, x)):
        with pytest.raises(RuntimeError) as info:       # (NotImplementedError is one)
            call()
        assert not isinstance(info.value, ValueError)


def test_module_holds_no_state():
    from ot_vae_lightning_amd import MSSSIMLoss
    m = MSSSIMLoss(data_range=(0.0, 1.0), reduction="sum")
    assert list(m.state_dict()) == [] and list(m.parameters()) == [] and list(m.buffers()) == []
