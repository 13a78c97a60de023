"""CPU: the interface of ``ot_vae_lightning_amd.metrics`` (collection prefixing / cloning, keyword routing, the 1000-observation
guard, reset, states outside ``state_dict``, ``sync`` over gloo) and the C ABI of the two new entries.

No fixture from the reference is used: its ``metrics/fid.py`` cannot be imported without torchmetrics, so it serves as the
specification of behaviour only.  States are pre-filled on the host here (``update`` has no host path; the GPU tests drive it)."""
import importlib.util
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


def _prefill(metric, n, seed, shift=0.0):
    """moments of n seeded feature vectors written straight into the (host) states of both sides"""
    g = torch.Generator().manual_seed(seed)
    d = metric.feature_size
    for side, off in (("real", 0.0), ("fake", shift)):
        f = torch.randn(n, d, generator=g, dtype=torch.float64) + off
        getattr(metric, f"{side}_sum").copy_(f.sum(0))
        getattr(metric, f"{side}_correlation").copy_(f.T @ f)
        getattr(metric, f"num_{side}_obs").fill_(n)


def test_collection_prefix_clone_and_items():
    from ot_vae_lightning_amd.metrics import FrechetDistance, MetricCollection, PeakSignalNoiseRatio
    base = MetricCollection({"psnr": PeakSignalNoiseRatio(data_range=1.0), "fid": FrechetDistance(8)})
    assert base.prefix is None and [k for k, _ in base.items()] == ["psnr", "fid"]
    val, test = base.clone(prefix="val/metrics/"), base.clone(prefix="test/metrics/")
    assert val.prefix == "val/metrics/" and [k for k, _ in val.items()] == ["val/metrics/psnr", "val/metrics/fid"]
    assert [k for k, _ in val.items(keep_base=True)] == ["psnr", "fid"]
    # clones share no state
    val["fid"].real_sum.add_(1.0)
    val["psnr"].sqerr_state[0] = 5.0
    assert float(test["fid"].real_sum.abs().sum()) == 0 and float(base["fid"].real_sum.abs().sum()) == 0
    assert float(test["psnr"].sum_squared_error) == 0
    assert val["fid"].real_sum.data_ptr() != test["fid"].real_sum.data_ptr()
    assert set(val.compute()) == {"val/metrics/psnr", "val/metrics/fid"}
    # a list is named by class
    assert [k for k, _ in MetricCollection([PeakSignalNoiseRatio()], prefix="p/").items()] == ["p/PeakSignalNoiseRatio"]
    with pytest.raises(ValueError):
        MetricCollection({"x": torch.nn.Identity()})


def test_collection_routes_keywords_by_update_signature():
    from ot_vae_lightning_amd.metrics import Metric, MetricCollection

    class Rec(Metric):
        def __init__(self):
            super().__init__()
            self.add_state("calls", torch.zeros(1))
            self.seen = None

    class PT(Rec):
        def update(self, preds, target):
            self.seen = ("pt", preds, target)
            self.calls += 1

    class GS(Rec):
        def update(self, generated=None, samples=None):
            self.seen = ("gs", generated, samples)
            self.calls += 1

    class Any_(Rec):
        def update(self, *a, **kw):
            self.seen = sorted(kw)
            self.calls += 1

    c = MetricCollection({"a": PT(), "b": GS(), "c": Any_()}, prefix="val/")
    c.update(samples=1, target=2, preds=3, generated=4, kwargs={})
    assert c["a"].seen == ("pt", 3, 2) and c["b"].seen == ("gs", 4, 1)
    assert c["c"].seen == ["generated", "kwargs", "preds", "samples", "target"]
    assert c(10, 20) == {}                      # forward = update; nothing is returned unless compute_on_step
    assert c["a"].seen == ("pt", 10, 20) and c["b"].seen == ("gs", 10, 20)
    assert float(c["a"].calls) == 2
    c.reset()
    assert float(c["a"].calls) == 0 and float(c["b"].calls) == 0


def test_frechet_guard_reset_and_state_dict():
    from ot_vae_lightning_amd.metrics import FrechetDistance, MetricCollection, PeakSignalNoiseRatio
    m = FrechetDistance(6)
    assert torch.isinf(m.compute()).all()                       # nothing seen
    _prefill(m, 999, 1)
    assert torch.isinf(m.compute()).all()                       # 999 per side
    _prefill(m, 1000, 1)
    m.num_fake_obs.fill_(999)
    assert torch.isinf(m.compute()).all()                       # one side short
    m.num_fake_obs.fill_(1000)
    v = m.compute()
    assert torch.isfinite(v).all() and v.dtype == torch.float64 and float(v) >= 0

    # the value is the Frechet distance of the two moment sets (LAPACK route for host-resident states)
    g = torch.Generator().manual_seed(1)
    fa = torch.randn(1000, 6, generator=g, dtype=torch.float64)
    fb = torch.randn(1000, 6, generator=g, dtype=torch.float64)
    ca, cb = torch.cov(fa.T, correction=0), torch.cov(fb.T, correction=0)
    lam = torch.linalg.eigvals(ca @ cb).real.clamp(min=0)
    want = ((fa.mean(0) - fb.mean(0)) ** 2).sum() + ca.trace() + cb.trace() - 2 * lam.sqrt().sum()
    assert abs(float(v) - float(want)) <= 1e-8 * max(1.0, abs(float(want)))

    # a pure mean shift gives |delta|^2
    _prefill(m, 2000, 3)
    m.fake_sum.copy_(m.real_sum + 2000 * 0.5)
    mu = m.real_sum / 2000
    m.fake_correlation.copy_(m.real_correlation + 2000 * (torch.outer(mu + 0.5, mu + 0.5) - torch.outer(mu, mu)))
    assert abs(float(m.compute()) - 6 * 0.25) < 1e-8

    m.reset()
    assert float(m.num_real_obs) == 0 and float(m.real_correlation.abs().sum()) == 0 and torch.isinf(m.compute()).all()

    p = PeakSignalNoiseRatio()
    addr = p.sqerr_state.data_ptr()
    p.sqerr_state[:4] = torch.tensor([4.0, 100.0, 0.0, 2.0], dtype=torch.float64)
    assert abs(float(p.compute()) - 10 * math.log10(4.0 / 0.04)) < 1e-12   # tracked range 2
    p.reset()
    assert p.sqerr_state.data_ptr() == addr and float(p.total) == 0 and float(p.min_target) == float("inf")
    assert torch.isinf(_with_state(PeakSignalNoiseRatio(data_range=1.0), [0.0, 10.0, 0.0, 1.0]).compute())   # identical tensors
    assert abs(float(_with_state(PeakSignalNoiseRatio(data_range=1.0, base=2.0), [5.0, 10.0]).compute()) - 10.0) < 1e-12

    # states and the feature network's buffers stay out of checkpoints; a model that owns a collection keeps the reference's keys
    coll = MetricCollection({"psnr": PeakSignalNoiseRatio(), "fid": FrechetDistance(4)})
    assert list(coll.state_dict()) == [] and list(m.state_dict()) == []
    import ot_vae_lightning_amd as A
    mk = lambda metrics: A.VAE(encoder=A.CNN(1, 16, 16, 1, capacity=2, down_sample=True), metrics=metrics,      # noqa: E731
                               decoder=A.CNN(8, 1, 1, 16, capacity=2, up_sample=True), prior=A.GaussianPrior(loss_coeff=0.1))
    with_m, without = mk(coll), mk(None)
    assert list(with_m.state_dict()) == list(without.state_dict())
    assert with_m.val_metrics.prefix == "val/metrics/" and with_m.monitor == "val/metrics/psnr"
    assert with_m.val_metrics["fid"].real_sum.data_ptr() != with_m.test_metrics["fid"].real_sum.data_ptr()
    # without metrics every evaluation hook returns at once
    assert without.validation_step((torch.zeros(2, 1, 16, 16), None), 0) is None and without.test_step(None, 0) is None
    assert without._compute_and_log_metric("val") is None and without._prepare_metrics("test") is None
    assert without.on_validation_epoch_end() is None and without.logged == {}


def _with_state(metric, head):
    metric.sqerr_state[:len(head)] = torch.tensor(head, dtype=torch.float64)
    return metric


def test_inception_default_needs_torchmetrics():
    from ot_vae_lightning_amd.metrics import FrechetInceptionDistance
    if importlib.util.find_spec("torchmetrics") is None:    # (where it is installed, net=None builds its Inception-v3 instead)
        with pytest.raises(ImportError, match="torchmetrics.*net="):
            FrechetInceptionDistance(net=None, feature_size=2048)
    with pytest.raises(ValueError):
        FrechetInceptionDistance(net=None, feature_size=100)
    # a network of the caller's own: eval mode, kept there, grey images tiled, to_255 conversion
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.AdaptiveAvgPool2d(1))
    fid = FrechetInceptionDistance(net=net, feature_size=4, to_255=False, data_range=(-1.0, 1.0))
    assert not fid.net.training and not fid.train().net.training
    assert fid.data_range == 2.0 and fid.data_low == -1.0
    x = torch.rand(5, 1, 8, 8)
    f = fid._extract_features(x)
    assert f.shape == (5, 4) and torch.allclose(f, net(torch.cat([x, x, x], 1)).reshape(5, 4))
    fid.to_255 = True
    seen = {}
    fid.net = type("Spy", (torch.nn.Module,), {"forward": lambda self, img: seen.setdefault("img", img).float().mean((2, 3))})()
    fid._extract_features(torch.full((2, 3, 4, 4), 0.0))
    assert seen["img"].dtype == torch.uint8 and int(seen["img"].max()) == 127      # 255 * (0 - -1) / 2


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
        from ot_vae_lightning_amd.metrics import FrechetDistance, MetricCollection, PeakSignalNoiseRatio
        coll = MetricCollection({"psnr": PeakSignalNoiseRatio(), "fid": FrechetDistance(5)}, prefix="val/metrics/")
        g = torch.Generator().manual_seed(7)
        feats = torch.randn(2 * 700, 5, generator=g, dtype=torch.float64)
        mine = feats[rank * 700:(rank + 1) * 700]
        fid, psnr = coll["fid"], coll["psnr"]
        for side in ("real", "fake"):
            getattr(fid, f"{side}_sum").copy_(mine.sum(0))
            getattr(fid, f"{side}_correlation").copy_(mine.T @ mine)
            getattr(fid, f"num_{side}_obs").fill_(700)
        psnr.sqerr_state[:4] = torch.tensor([1.0 + rank, 10.0, -1.0 - rank, 2.0 + rank], dtype=torch.float64)
        coll.sync()                                   # no process group yet: nothing happens
        assert float(fid.num_real_obs) == 700 and torch.isinf(coll.compute()["val/metrics/fid"]).all()
        dist.init_process_group("gloo", rank=rank, world_size=world)
        coll.sync()
        assert float(fid.num_real_obs) == 1400 and float(fid.num_fake_obs) == 1400
        assert torch.allclose(fid.real_sum, feats.sum(0)) and torch.allclose(fid.fake_correlation, feats.T @ feats)
        assert psnr.sqerr_state[:4].tolist() == [3.0, 20.0, -2.0, 3.0]          # sum, sum, min, max
        res = coll.compute()
        assert abs(float(res["val/metrics/fid"])) < 1e-8                        # equal streams on both sides
        assert abs(float(res["val/metrics/psnr"]) - 10 * math.log10(25.0 / (3.0 / 20.0))) < 1e-9
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_sync_sums_states_world2_gloo():
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


def test_new_entries_in_header_binding_and_library():
    from ot_vae_lightning_amd import _lib, build
    names = ("otvae_moments_accum", "otvae_moments_accum_ws", "otvae_sqerr_accum", "otvae_sqerr_state_words")
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "otvae.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(otvae_[a-z0-9_]+)\s*\(", hdr))
    lib = build.build(verbose=False)
    exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert n in declared and n in _lib.SIGNATURES, n
        assert re.search(rf"\bT {n}\b", exported), f"{n} is not exported by {lib}"
    # the workspace promise of the header: (4 D64^2 + 264 D64) * 8 bytes at most, whatever B is; none for the widest features
    handle = _lib.load()
    assert handle.otvae_sqerr_state_words() == 4 + 3 * 256
    for d in (1, 17, 64, 100, 192, 768, 1024, 1984, 1985, 2048):
        d64 = (d + 63) // 64 * 64
        for b in (1, 127, 128, 1024, 1 << 20):
            ws = handle.otvae_moments_accum_ws(b, d)
            assert 0 <= ws <= (4 * d64 * d64 + 264 * d64) * 8, (b, d, ws)
            if d >= 1024:
                assert ws < 4.2 * d * d * 8
            if d >= 1985 or b < 256:
                assert ws == 0
    assert handle.otvae_moments_accum_ws(1024, 2049) == -1 and handle.otvae_moments_accum_ws(0, 8) == -1
    # operators: mutable schemas, CUDA kernels only
    import ot_vae_lightning_amd  # noqa: F401
    for op in ("moments_accum", "sqerr_accum"):
        schema = str(getattr(torch.ops.otvae, op).default._schema)
        assert "(a!)" in schema and schema.endswith("-> ()"), schema
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{op}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{op}", "CPU")
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.otvae.moments_accum(torch.zeros(4, 3), torch.zeros(1, dtype=torch.float64), torch.zeros(3, dtype=torch.float64),
                                      torch.zeros(3, 3, dtype=torch.float64))
