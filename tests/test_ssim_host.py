"""CPU: the host side of ``StructuralSimilarityIndexMeasure`` / ``structural_similarity`` -- exports, the three C-ABI entries, the
operator's registration, every constructor / shape refusal, window sizes and weights, and the metric's state (reset, clone,
collection naming, ``state_dict``, ``sync`` over gloo).  ``update`` has no host path; ``tests/test_gpu_ssim.py`` drives it."""
import math
import os
import re
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = 4 + 4 * 256


def test_exports_and_operator_registration():
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import metrics
    assert "StructuralSimilarityIndexMeasure" in metrics.__all__ and "structural_similarity" in metrics.__all__
    assert metrics.StructuralSimilarityIndexMeasure.higher_is_better is True
    # (ops.OPS lists the differentiable operators, each with a *_backward operator and an autograd kernel -- test_custom_ops_host.py;
    # the in-place accumulators sqerr_accum / moments_accum / ssim_accum have neither and are registered beside it)
    schema = str(torch.ops.otvae.ssim_accum.default._schema)
    assert "Tensor(a!) state" in schema and "Tensor(b!)? per_image" in schema and schema.endswith("-> ()"), schema
    assert torch._C._dispatch_has_kernel_for_dispatch_key("otvae::ssim_accum", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("otvae::ssim_accum", "CPU")
    x = torch.rand(2, 1, 16, 16)
    with pytest.raises((NotImplementedError, RuntimeError)):      # no CPU path: the dispatcher refuses host tensors
        metrics.structural_similarity(x, x, data_range=1.0)
    with pytest.raises((NotImplementedError, RuntimeError)):
        metrics.StructuralSimilarityIndexMeasure(data_range=1.0).update(x, x)


def test_entries_in_header_binding_and_library():
    from ot_vae_lightning_amd import _lib, build
    from ot_vae_lightning_amd.metrics import ssim
    names = ("otvae_ssim_accum", "otvae_ssim_ws", "otvae_ssim_state_words")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "otvae.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(otvae_[a-z0-9_]+)\s*\(", hdr))
    lib = build.build(verbose=False)
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert n in declared and n in _lib.SIGNATURES, n
        assert re.search(rf"\bT {n}\b", exported), f"{n} is not exported by {lib}"
    handle = _lib.load()
    assert handle.otvae_abi_version() == 2
    assert handle.otvae_ssim_state_words() == ssim._STATE_WORDS == WORDS
    # one double per (image, channel, 16 x 32 tile of window positions)
    for (b, c, h, w, kh, kw), tiles in (((1, 1, 11, 11, 11, 11), 1), ((1024, 1, 32, 32, 11, 11), 2), ((2, 2, 75, 70, 11, 11), 5 * 2),
                                        ((64, 3, 64, 64, 11, 11), 4 * 2), ((1, 1, 31, 40, 31, 31), 1), ((3, 2, 20, 40, 3, 5), 2 * 2)):
        assert handle.otvae_ssim_ws(b, c, h, w, kh, kw) == 8 * b * c * tiles, (b, c, h, w, kh, kw)
    # the layout does not depend on B: the bytes are proportional to it
    assert handle.otvae_ssim_ws(7, 3, 100, 90, 9, 15) == 7 * handle.otvae_ssim_ws(1, 3, 100, 90, 9, 15)
    for refused in ((0, 1, 32, 32, 11, 11), (1, 0, 32, 32, 11, 11), (1, 1, 10, 32, 11, 11), (1, 1, 32, 10, 11, 11), (1, 1, 32, 32, 10, 11),
                    (1, 1, 32, 32, 11, 0), (1, 1, 64, 64, 33, 11), (1, 1, 64, 64, 11, 33), (1 << 30, 64, 64, 64, 11, 11)):
        assert handle.otvae_ssim_ws(*refused) == -1, refused


def test_constructor_and_shape_refusals():
    from ot_vae_lightning_amd.metrics import StructuralSimilarityIndexMeasure as SSIM, structural_similarity
    for bad in (dict(kernel_size=10), dict(kernel_size=0), dict(kernel_size=-3), dict(kernel_size=(11, 4)), dict(gaussian_kernel=False, kernel_size=8),
                dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=(1.5, 0.0)), dict(return_full_image=True), dict(return_contrast_sensitivity=True),
                dict(reduction="mean"), dict(data_range=(1.0, 0.0)), dict(data_range=0.0)):
        with pytest.raises(ValueError):
            SSIM(**bad)
    for reduction in ("none", None):
        with pytest.raises(ValueError, match="structural_similarity"):
            SSIM(reduction=reduction)
    m = SSIM(data_range=1.0)
    x = torch.rand(2, 1, 16, 16)
    for p, t in ((x[0], x[0]), (x[:, :, :, :, None], x[:, :, :, :, None]),                 # ndim != 4
                 (x, torch.rand(2, 1, 16, 17)), (x, torch.rand(3, 1, 16, 16)),             # shape mismatch
                 (torch.rand(1, 1, 10, 16), torch.rand(1, 1, 10, 16)),                     # H < kh
                 (torch.rand(1, 1, 16, 10), torch.rand(1, 1, 16, 10))):                    # W < kw
        with pytest.raises(ValueError):
            m.update(p, t)
        with pytest.raises(ValueError):
            structural_similarity(p, t, data_range=1.0)
    with pytest.raises(ValueError):
        structural_similarity(x, x, sigma=0.0)
    with pytest.raises(ValueError):
        structural_similarity(x, x, return_full_image=True)
    # the operator's own checks come before any call into the library
    state, win = torch.zeros(WORDS, dtype=torch.float64), [1.0]
    for args in ((x[0], x[0], win, win, 0.01, 0.03, 0, 0.0, 1.0, state, None), (x, x.double(), win, win, 0.01, 0.03, 0, 0.0, 1.0, state, None)):
        with pytest.raises((ValueError, NotImplementedError, RuntimeError)):
            torch.ops.otvae.ssim_accum(*args)


def test_window_sizes_and_weights():
    from ot_vae_lightning_amd.metrics import StructuralSimilarityIndexMeasure as SSIM
    from ot_vae_lightning_amd.metrics.ssim import gaussian_window
    for sigma, size in ((1.5, (11, 11)), (1.0, (9, 9)), (2.0, (15, 15)), ((1.0, 2.0), (9, 15)), (4.3, (31, 31)), (4.5, (33, 33))):
        assert SSIM(sigma=sigma).window_size == size
    assert SSIM(sigma=1.5, kernel_size=7).window_size == (11, 11)                  # kernel_size is ignored with a Gaussian window
    assert SSIM(gaussian_kernel=False, kernel_size=7).window_size == (7, 7)
    u = SSIM(gaussian_kernel=False, kernel_size=(3, 5))
    assert u.window_size == (3, 5) and u.options.window[0] == [1 / 3] * 3 and u.options.window[1] == [1 / 5] * 5
    for sigma in (1.0, 1.5, 2.0, 4.3):
        k = 2 * int(3.5 * sigma + 0.5) + 1
        i = torch.arange(k, dtype=torch.float64)
        g = torch.exp(-(((i - (k - 1) / 2) / sigma) ** 2) / 2)
        want = g / g.sum()
        got = torch.tensor(gaussian_window(sigma), dtype=torch.float64)
        assert got.shape == want.shape and float((got - want).abs().max()) <= 4 * 2.0 ** -53
        assert abs(math.fsum(gaussian_window(sigma)) - 1.0) <= 4 * 2.0 ** -53
    m = SSIM(sigma=(1.0, 2.0))
    assert m.options.window[0] == gaussian_window(1.0) and m.options.window[1] == gaussian_window(2.0)


def test_state_reset_clone_collection_and_state_dict():
    from ot_vae_lightning_amd.metrics import MetricCollection, PeakSignalNoiseRatio, StructuralSimilarityIndexMeasure as SSIM
    m = SSIM(data_range=1.0)
    assert m.ssim_state.dtype == torch.float64 and m.ssim_state.numel() == WORDS and float(m.ssim_state.abs().sum()) == 0
    addr = m.ssim_state.data_ptr()
    m.ssim_state[:2] = torch.tensor([3.0, 4.0], dtype=torch.float64)
    m.ssim_state[100] = 7.0
    assert float(m.similarity) == 3 and float(m.total) == 4
    v = m.compute()
    assert v.dtype == torch.float64 and v.dim() == 0 and float(v) == 0.75
    s = SSIM(data_range=1.0, reduction="sum")
    s.ssim_state[:2] = torch.tensor([3.0, 4.0], dtype=torch.float64)
    assert float(s.compute()) == 3.0
    twin = m.clone()
    assert twin.ssim_state.data_ptr() != addr and torch.equal(twin.ssim_state, m.ssim_state) and twin.window_size == (11, 11)
    m.reset()
    assert m.ssim_state.data_ptr() == addr and float(m.ssim_state.abs().sum()) == 0 and float(twin.similarity) == 3
    assert list(m.state_dict()) == []
    base = MetricCollection({"psnr": PeakSignalNoiseRatio(), "ssim": SSIM()})
    val = base.clone(prefix="val/metrics/")
    assert val.keys() == ["val/metrics/psnr", "val/metrics/ssim"] and list(val.state_dict()) == []
    val["ssim"].ssim_state[:2] = torch.tensor([1.0, 2.0], dtype=torch.float64)
    assert float(base["ssim"].total) == 0 and float(val.compute()["val/metrics/ssim"]) == 0.5
    assert MetricCollection([SSIM()], prefix="p/").keys() == ["p/StructuralSimilarityIndexMeasure"]
    assert m.update_keywords() == ["preds", "target"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sync_worker(rank, world, port, q):
    try:
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        from ot_vae_lightning_amd.metrics import MetricCollection, StructuralSimilarityIndexMeasure
        coll = MetricCollection({"ssim": StructuralSimilarityIndexMeasure()}, prefix="val/metrics/")
        ssim = coll["ssim"]
        ssim.ssim_state[:2] = torch.tensor([1.5 + rank, 4.0 + rank], dtype=torch.float64)
        ssim.ssim_state[2:] = 10.0 + rank                                        # the scratch: every rank's own, never reduced
        dist.init_process_group("gloo", rank=rank, world_size=world)
        coll.sync()
        assert ssim.ssim_state[:2].tolist() == [4.0, 9.0]
        assert bool((ssim.ssim_state[2:] == 10.0 + rank).all())
        assert abs(float(coll.compute()["val/metrics/ssim"]) - 4.0 / 9.0) < 1e-15
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_sync_sums_the_two_accumulators_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, msg in res:
        assert msg == "ok", f"rank {rank}:\n{msg}"
