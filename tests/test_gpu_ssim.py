"""GPU: ``StructuralSimilarityIndexMeasure`` / ``structural_similarity`` (``csrc/ssim.hip``) against the definition evaluated in
float64 on the CPU inside the test.

Truth and bound.  ``_definition`` is the specification as written: the five windowed means by a grouped ``conv2d`` over the valid
positions, ``sigma = E[x^2] - mu^2``, the map, its mean per image.  In float64 it is the truth; the same function in float32 is the
"composition" a user would write in torch.  Per image, under the project's evidence rule,
``|ours - truth| <= max(1e-4 |truth|, 1.5 |composition - truth|)``: 1e-4 relative is the fp32 parity contract, and where fp32
arithmetic of the formula itself cannot reach it the composition's own error says so.  The cancellation cases are held to
``1e-4 |truth|`` ALONE -- there the composition loses digits to ``E[x^2] - mu^2`` and the kernel, which forms the second moments
about a pixel of the tile, must not.  Every case prints our error and the composition's."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -23


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import metrics
    return metrics


def _windows(gaussian=True, sigma=1.5, kernel_size=11):
    from ot_vae_lightning_amd.metrics.ssim import _pair, gaussian_window
    if gaussian:
        return [torch.tensor(gaussian_window(float(s)), dtype=torch.float64) for s in _pair(sigma, "sigma")]
    return [torch.full((k,), 1.0 / k, dtype=torch.float64) for k in _pair(kernel_size, "kernel_size")]


def _definition(p, t, wh, ww, data_range, k1=0.01, k2=0.03):
    """per-image SSIM [B] in the dtype of ``p``: the issue's definition, nothing else"""
    dtype = p.dtype
    t = t.to(dtype)
    if isinstance(data_range, tuple):
        p, t = p.clamp(*data_range), t.clamp(*data_range)
        rng = data_range[1] - data_range[0]
    elif data_range is None:
        rng = torch.maximum(p.max() - p.min(), t.max() - t.min())
    else:
        rng = data_range
    b, c = p.shape[:2]
    kernel = torch.outer(wh, ww).to(dtype).expand(c, 1, -1, -1)
    mu_p, mu_t, e_pp, e_tt, e_pt = F.conv2d(torch.cat([p, t, p * p, t * t, p * t]), kernel, groups=c).split(b)
    s_pp, s_tt, s_pt = e_pp - mu_p * mu_p, e_tt - mu_t * mu_t, e_pt - mu_p * mu_t
    c1, c2 = (k1 * rng) ** 2, (k2 * rng) ** 2
    ssim = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p * mu_p + mu_t * mu_t + c1) * (s_pp + s_tt + c2))
    return ssim.reshape(b, -1).mean(-1)


def _pair_of(shape, rng, seed, dtype=torch.float32, lo=0.0):
    g = torch.Generator().manual_seed(seed)
    target = lo + rng * torch.rand(shape, generator=g, dtype=torch.float64)
    preds = (target + 0.1 * rng * torch.randn(shape, generator=g, dtype=torch.float64)).clamp(lo, lo + rng)
    return preds.to(dtype), target.to(dtype)


def _check(M, label, p, t, data_range, cancellation=False, **window):
    wh, ww = _windows(**window)
    truth = _definition(p.double(), t.double(), wh, ww, data_range)
    comp = _definition(p.float(), t.float(), wh, ww, data_range).double()
    kw = dict(gaussian_kernel=window.get("gaussian", True), sigma=window.get("sigma", 1.5), kernel_size=window.get("kernel_size", 11))
    ours = M.structural_similarity(p.cuda(), t.cuda(), data_range=data_range, **kw).cpu()
    assert ours.dtype == torch.float64 and ours.shape == truth.shape
    err, cerr = (ours - truth).abs(), (comp - truth).abs()
    bound = 1e-4 * truth.abs() if cancellation else torch.maximum(1e-4 * truth.abs(), 1.5 * cerr)
    print(f"[ssim {label}] truth {truth.tolist()}  ours err {err.max():.3e} (rel {float((err / truth.abs()).max()):.3e})  "
          f"composition err {cerr.max():.3e}  bound {bound.min():.3e}")
    assert bool((err <= bound).all()), f"{label}: err {err.tolist()} beyond {bound.tolist()}"
    return ours, truth


SHAPES = [(1, 1, 11, 11), (2, 1, 11, 12), (2, 1, 12, 11), (3, 1, 32, 32), (2, 3, 33, 47), (2, 2, 75, 70)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("rng", [1.0, 255.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_float64_definition(M, shape, rng, dtype):
    p, t = _pair_of(shape, rng, seed=sum(shape), dtype=dtype)
    _check(M, f"{shape} R={rng} {dtype}", p, t, rng)


@pytest.mark.parametrize("window", [dict(sigma=(1.0, 2.0)), dict(gaussian=False, kernel_size=7), dict(gaussian=False, kernel_size=(3, 5))],
                         ids=["sigma1x2", "uniform7", "uniform3x5"])
def test_window_options(M, window):
    p, t = _pair_of((2, 2, 20, 40), 1.0, seed=5)
    _check(M, f"{window}", p, t, 1.0, **window)


def test_data_range_pair_clamps_and_none_takes_the_batch_range(M):
    p, t = _pair_of((2, 2, 20, 40), 1.0, seed=6)      # values in [0, 1]: well outside (0.2, 0.8)
    assert float(p.min()) < 0.2 and float(p.max()) > 0.8
    _check(M, "clamp (0.2, 0.8)", p, t, (0.2, 0.8))
    for dtype in (torch.float32, torch.float64):
        p, t = _pair_of((3, 2, 33, 47), 3.0, seed=7, dtype=dtype, lo=-1.0)
        _check(M, f"data_range=None {dtype}", p, t, None)


def test_cancellation_cases_hold_the_contract_alone(M):
    g = torch.Generator().manual_seed(11)
    target = 0.98 + 0.01 * torch.rand((2, 1, 32, 32), generator=g, dtype=torch.float64)
    preds = target + 0.002 * torch.randn((2, 1, 32, 32), generator=g, dtype=torch.float64)
    _check(M, "narrow 0.98..0.99, data_range=None", preds.float(), target.float(), None, cancellation=True)
    target = 250.0 + torch.rand((2, 1, 32, 32), generator=g, dtype=torch.float64)
    preds = target + 0.2 * torch.randn((2, 1, 32, 32), generator=g, dtype=torch.float64)
    _check(M, "250..251, R=255", preds.float(), target.float(), 255.0, cancellation=True)


def test_identical_tensors_give_one(M):
    for dtype in (torch.float32, torch.float64):
        _, t = _pair_of((3, 2, 33, 47), 1.0, seed=8, dtype=dtype)
        for data_range in (1.0, None):
            v = M.structural_similarity(t.cuda(), t.clone().cuda(), data_range=data_range).cpu()
            print(f"[ssim identical {dtype} data_range={data_range}] 1 - v = {(1 - v).tolist()}")
            assert bool(((v - 1).abs() <= 4 * ULP32).all())


def test_bit_properties(M):
    p, t = _pair_of((4, 3, 33, 47), 1.0, seed=9)
    pg, tg = p.cuda(), t.cuda()
    full = M.structural_similarity(pg, tg, data_range=1.0)
    assert torch.equal(full, M.structural_similarity(pg, tg, data_range=1.0))                    # run to run
    assert torch.equal(M.structural_similarity(pg[1:3], tg[1:3], data_range=1.0), full[1:3])    # an image's value is its own
    assert torch.equal(M.structural_similarity(pg[3:], tg[3:], data_range=1.0), full[3:])
    cl_p, cl_t = pg.contiguous(memory_format=torch.channels_last), tg.contiguous(memory_format=torch.channels_last)
    assert not cl_p.is_contiguous()
    assert torch.equal(M.structural_similarity(cl_p, cl_t, data_range=1.0), full)
    big_p, big_t = torch.rand(4, 3, 40, 50, device="cuda"), torch.rand(4, 3, 40, 50, device="cuda")
    sl_p, sl_t = big_p[:, :, 3:36, 1:48], big_t[:, :, 3:36, 1:48]
    assert not sl_p.is_contiguous()
    assert torch.equal(M.structural_similarity(sl_p, sl_t, data_range=1.0),
                       M.structural_similarity(sl_p.contiguous(), sl_t.contiguous(), data_range=1.0))
    # the metric's state is the same sum on every run
    a, b = M.StructuralSimilarityIndexMeasure(data_range=1.0).cuda(), M.StructuralSimilarityIndexMeasure(data_range=1.0).cuda()
    a.update(pg, tg)
    b.update(pg, tg)
    assert torch.equal(a.ssim_state[:2], b.ssim_state[:2])


def test_accumulation_reductions_and_reset(M):
    p, t = _pair_of((6, 2, 20, 40), 1.0, seed=10)
    pg, tg = p.cuda(), t.cuda()
    per_image = M.structural_similarity(pg, tg, data_range=1.0).cpu()
    tol = 6 * 2.0 ** -53 * float(per_image.abs().sum())
    mean, total = M.StructuralSimilarityIndexMeasure(data_range=1.0).cuda(), M.StructuralSimilarityIndexMeasure(data_range=1.0, reduction="sum").cuda()
    for m in (mean, total):
        m.update(pg[:3], tg[:3])
        m.update(pg[3:], tg[3:])
        assert float(m.total) == 6
    v = mean.compute()
    assert v.dtype == torch.float64 and v.dim() == 0
    print(f"[ssim accumulate] mean {float(v)} vs {float(per_image.mean())}, sum {float(total.compute())} vs {float(per_image.sum())}, tol {tol:.3e}")
    assert abs(float(v) - float(per_image.sum()) / 6) <= tol
    assert abs(float(total.compute()) - float(per_image.sum())) <= tol
    addr = mean.ssim_state.data_ptr()
    mean.reset()
    assert mean.ssim_state.data_ptr() == addr and float(mean.total) == 0 and float(mean.similarity) == 0
    mean.update(pg[:2], tg[:2])
    assert abs(float(mean.compute()) - float(per_image[:2].sum()) / 2) <= tol and float(mean.total) == 2


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_pixel_stays_in_its_image(M, bad):
    p, t = _pair_of((3, 2, 20, 40), 1.0, seed=12)
    clean = M.structural_similarity(p.cuda(), t.cuda(), data_range=1.0).cpu()
    p[1, 1, 7, 33] = bad
    v = M.structural_similarity(p.cuda(), t.cuda(), data_range=1.0).cpu()
    assert not bool(torch.isfinite(v[1]))
    assert torch.equal(v[0], clean[0]) and torch.equal(v[2], clean[2])
    m = M.StructuralSimilarityIndexMeasure(data_range=1.0).cuda()
    m.update(p.cuda(), t.cuda())
    assert not bool(torch.isfinite(m.compute())) and float(m.total) == 3
    if bad != bad:
        assert bool(torch.isnan(v[1])) and bool(torch.isnan(m.compute()))


def test_window_envelope(M):
    with pytest.raises(NotImplementedError):      # sigma 4.5 -> 33 taps
        M.structural_similarity(torch.rand(1, 1, 40, 40, device="cuda"), torch.rand(1, 1, 40, 40, device="cuda"), sigma=4.5, data_range=1.0)
    p, t = _pair_of((1, 1, 31, 40), 1.0, seed=13)   # sigma 4.3 -> 31 taps: one row of ten positions
    _check(M, "sigma 4.3 (31 taps)", p, t, 1.0, sigma=4.3)


def test_operator_checks_come_before_the_call(M):
    from ot_vae_lightning_amd import _lib
    words = _lib.load().otvae_ssim_state_words()
    x = torch.rand(2, 1, 16, 16, device="cuda")
    state, win = torch.zeros(words, dtype=torch.float64, device="cuda"), [0.25, 0.5, 0.25]
    call = lambda p, t, st=state, per=None, wh=win: torch.ops.otvae.ssim_accum(p, t, wh, win, 0.01, 0.03, 0, 0.0, 1.0, st, per)  # noqa: E731
    for bad in ((x[0], x[0]), (x, x[:1]), (x, x.double()), (x.half(), x.half()), (x.transpose(2, 3), x.transpose(2, 3))):
        with pytest.raises(ValueError):
            call(*bad)
    for kwargs in (dict(st=state[:-1]), dict(st=state.float()), dict(per=torch.zeros(3, dtype=torch.float64, device="cuda")),
                   dict(per=torch.zeros(2, device="cuda")), dict(wh=[0.5, 0.5]), dict(wh=[1 / 17] * 17)):
        with pytest.raises(ValueError):
            call(x, x, **kwargs)
    assert float(state.abs().sum()) == 0                    # nothing ran
    per = torch.zeros(2, dtype=torch.float64, device="cuda")
    call(x, x, per=per)
    assert float(state[1]) == 2 and bool(((per - 1).abs() <= 4 * ULP32).all())


@pytest.mark.parametrize("data_range", [1.0, None], ids=["fixed", "batch"])
def test_update_replays_from_a_captured_graph(M, data_range):
    """``update`` inside a capture on a stream of the package's own (linear, no side branch), then two replays: the state is that of
    three eager calls -- which also shows that ``update`` reads nothing back to the host"""
    from ot_vae_lightning_amd import _lib
    p, t = _pair_of((8, 3, 32, 32), 1.0, seed=14)
    pg, tg = p.cuda(), t.cuda()
    eager = M.StructuralSimilarityIndexMeasure(data_range=data_range).cuda()
    for _ in range(3):
        eager.update(pg, tg)
    captured = M.StructuralSimilarityIndexMeasure(data_range=data_range).cuda()
    torch.cuda.synchronize()
    s = _lib.fresh_stream("cuda")
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        captured.update(pg, tg)
    torch.cuda.synchronize()
    captured.reset()                                                          # (whatever the capture itself left behind)
    captured.update(pg, tg)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert float(captured.total) == 3 * 8
    assert torch.equal(captured.ssim_state[:2], eager.ssim_state[:2]) and torch.equal(captured.compute(), eager.compute())
    del graph


def test_collection_with_psnr_under_a_prefix(M):
    p, t = _pair_of((4, 3, 32, 32), 1.0, seed=15)
    coll = M.MetricCollection({"psnr": M.PeakSignalNoiseRatio(), "ssim": M.StructuralSimilarityIndexMeasure(data_range=1.0)},
                              prefix="val/metrics/").cuda()
    assert coll(p.cuda(), t.cuda()) == {}
    res = coll.compute()
    assert set(res) == {"val/metrics/psnr", "val/metrics/ssim"}
    wh, ww = _windows()
    truth = float(_definition(p.double(), t.double(), wh, ww, 1.0).mean())
    assert abs(float(res["val/metrics/ssim"]) - truth) <= 1e-4 * abs(truth) and bool(torch.isfinite(res["val/metrics/psnr"]))
