"""GPU: ``MultiScaleStructuralSimilarityIndexMeasure`` / ``multiscale_structural_similarity`` (``csrc/ssim.hip``) against the
definition (``tests/ms_ssim_definition.py``) evaluated in float64 on the CPU.

Truth and bound, per image, under the evidence rule of ``tests/test_gpu_ssim.py``:
``|ours - truth| <= max(1e-4 |truth|, 1.5 |float32 composition - truth|)``; the narrow-range case is held to ``1e-4 |truth|`` ALONE.
Every case prints our error and the composition's.  The references are computed once per case and shared."""
import functools

import pytest
import torch

from ms_ssim_definition import BETAS, CASE_IDS, CASES, definition, independent_pair, option_kwargs, pair_of, windows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import metrics
    return metrics


@functools.lru_cache(maxsize=None)
def _reference(case, rng, dtype):
    shape, window, betas = CASES[case]
    p, t = pair_of(shape, rng, seed=sum(shape), dtype=dtype)
    wh, ww = windows(**window)
    truth, v = definition(p.double(), t.double(), wh, ww, rng, betas, None)
    comp, _ = definition(p.float(), t.float(), wh, ww, rng, betas, None)
    return p, t, truth, comp.double(), v


def _assert_bound(label, ours, truth, comp, cancellation=False):
    ours = ours.cpu()
    assert ours.dtype == torch.float64 and ours.shape == truth.shape
    err, cerr = (ours - truth).abs(), (comp - truth).abs()
    bound = 1e-4 * truth.abs() if cancellation else torch.maximum(1e-4 * truth.abs(), 1.5 * cerr)
    print(f"[ms-ssim {label}] truth {truth.tolist()}  ours err {err.max():.3e} (rel {float((err / truth.abs()).max()):.3e})  "
          f"composition err {cerr.max():.3e}  bound {bound.min():.3e}")
    assert bool((err <= bound).all()), f"{label}: err {err.tolist()} beyond {bound.tolist()}"


def _check(M, label, p, t, data_range, betas, normalize="relu", cancellation=False, **window):
    wh, ww = windows(**window)
    truth, _ = definition(p.double(), t.double(), wh, ww, data_range, betas, normalize)
    comp, _ = definition(p.float(), t.float(), wh, ww, data_range, betas, normalize)
    ours = M.multiscale_structural_similarity(p.cuda(), t.cuda(), data_range=data_range, betas=betas, normalize=normalize,
                                              **option_kwargs(window))
    _assert_bound(label, ours, truth, comp.double(), cancellation)
    return ours


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("rng", [1.0, 255.0])
@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_against_the_float64_definition(M, case, rng, dtype):
    _, window, betas = CASES[case]
    p, t, truth, comp, v = _reference(case, rng, dtype)
    assert float(v.min()) > 0.9                     # every scale mean is far from 0: normalize=None stays finite
    for normalize in ("relu", None):                # (the same value on these inputs)
        ours = M.multiscale_structural_similarity(p.cuda(), t.cuda(), data_range=rng, betas=betas, normalize=normalize, **option_kwargs(window))
        _assert_bound(f"{CASE_IDS[case]} R={rng} {dtype} normalize={normalize}", ours, truth, comp)


def test_one_scale_is_ssim(M):
    p, t = pair_of((1, 1, 11, 11), 1.0, seed=24)
    ours = M.multiscale_structural_similarity(p.cuda(), t.cuda(), data_range=1.0, betas=(1.0,))
    ssim = M.structural_similarity(p.cuda(), t.cuda(), data_range=1.0)
    print(f"[ms-ssim one scale] {ours.tolist()} vs ssim {ssim.tolist()}")
    assert bool(((ours - ssim).abs() <= 1e-12 * ssim.abs()).all())
    wh, ww = windows()
    truth, _ = definition(p.double(), t.double(), wh, ww, 1.0, (1.0,))
    assert bool(((ours.cpu() - truth).abs() <= 1e-4 * truth.abs()).all())


def test_normalize(M):
    p, t = independent_pair()
    wh, ww = windows(sigma=0.5)
    _, v = definition(p, t, wh, ww, 1.0, BETAS[:3], None)
    assert float(v[1, 0]) < 0 < float(v[1, 1])                       # image 0 has a negative scale mean, image 1 has none
    kw = dict(sigma=0.5, data_range=1.0, betas=BETAS[:3])
    relu = M.multiscale_structural_similarity(p.cuda(), t.cuda(), normalize="relu", **kw).cpu()
    simple = M.multiscale_structural_similarity(p.cuda(), t.cuda(), normalize="simple", **kw).cpu()
    none = M.multiscale_structural_similarity(p.cuda(), t.cuda(), normalize=None, **kw).cpu()
    print(f"[ms-ssim normalize] relu {relu.tolist()} simple {simple.tolist()} none {none.tolist()}")
    assert float(relu[0]) == 0.0 and bool(torch.isnan(none[0]))
    for got, name, want in ((relu[1:], "relu", 0.3576), (none[1:], None, 0.3576), (simple[:1], "simple", 0.6774), (simple[1:], "simple", 0.7669)):
        assert abs(float(got) - want) <= 5e-5 + 1e-4 * want, (name, got, want)      # the figures of the issue, four decimals
    truth_simple, _ = definition(p, t, wh, ww, 1.0, BETAS[:3], "simple")
    comp_simple, _ = definition(p.float(), t.float(), wh, ww, 1.0, BETAS[:3], "simple")
    _assert_bound("simple", simple, truth_simple, comp_simple.double())
    truth_relu, _ = definition(p, t, wh, ww, 1.0, BETAS[:3], "relu")
    comp_relu, _ = definition(p.float(), t.float(), wh, ww, 1.0, BETAS[:3], "relu")
    _assert_bound("relu, the live image", relu[1:], truth_relu[1:], comp_relu.double()[1:])
    _assert_bound("none, the live image", none[1:], truth_relu[1:], comp_relu.double()[1:])


def test_data_range_pair_clamps_each_scale_and_pools_unclamped(M):
    p, t = pair_of((2, 2, 41, 43), 1.0, seed=6)           # values in [0, 1]: well outside (0.2, 0.8)
    assert float(p.min()) < 0.2 and float(p.max()) > 0.8
    ours = _check(M, "clamp (0.2, 0.8)", p, t, (0.2, 0.8), BETAS[:3], sigma=0.5).cpu()
    # pooling the CLAMPED images instead is a different number, further away than the bound
    wh, ww = windows(sigma=0.5)
    truth, _ = definition(p.double(), t.double(), wh, ww, (0.2, 0.8), BETAS[:3])
    wrong, _ = definition(p.double().clamp(0.2, 0.8), t.double().clamp(0.2, 0.8), wh, ww, 0.6, BETAS[:3])
    assert bool(((wrong - truth).abs() > 10 * (ours - truth).abs()).all()) and bool(((wrong - truth).abs() > 1e-3 * truth.abs()).all())


def test_data_range_none_takes_each_scale_s_range(M):
    for dtype in (torch.float32, torch.float64):
        p, t = pair_of((3, 2, 45, 43), 3.0, seed=7, dtype=dtype, lo=-1.0)
        ours = _check(M, f"data_range=None {dtype}", p, t, None, BETAS[:3], sigma=0.5).cpu()
    wh, ww = windows(sigma=0.5)
    truth, _ = definition(p.double(), t.double(), wh, ww, None, BETAS[:3])
    r0 = float(torch.maximum(p.max() - p.min(), t.max() - t.min()))
    wrong, _ = definition(p.double(), t.double(), wh, ww, r0, BETAS[:3])          # scale 0's range at every scale
    assert bool(((wrong - truth).abs() > 10 * (ours - truth).abs()).all())


def test_narrow_range_holds_the_contract_alone(M):
    g = torch.Generator().manual_seed(11)
    target = 0.98 + 0.01 * torch.rand((2, 1, 32, 32), generator=g, dtype=torch.float64)
    preds = target + 0.002 * torch.randn((2, 1, 32, 32), generator=g, dtype=torch.float64)
    _check(M, "narrow 0.98..0.99, data_range=None", preds.float(), target.float(), None, BETAS[:3], cancellation=True, sigma=0.5)
    _check(M, "narrow 0.98..0.99, data_range=1", preds.float(), target.float(), 1.0, BETAS[:3], cancellation=True, sigma=0.5)


def test_accumulation_reductions_and_reset(M):
    p, t = pair_of((5, 2, 32, 36), 1.0, seed=10)
    pg, tg = p.cuda(), t.cuda()
    kw = dict(sigma=0.5, betas=BETAS[:3], data_range=1.0)
    per_image = M.multiscale_structural_similarity(pg, tg, **kw).cpu()
    tol = 6 * 2.0 ** -53 * float(per_image.abs().sum())
    mean = M.MultiScaleStructuralSimilarityIndexMeasure(**kw).cuda()
    total = M.MultiScaleStructuralSimilarityIndexMeasure(reduction="sum", **kw).cuda()
    for m in (mean, total):
        m.update(pg[:2], tg[:2])
        m.update(pg[2:], tg[2:])
        assert float(m.total) == 5
    v = mean.compute()
    assert v.dtype == torch.float64 and v.dim() == 0
    print(f"[ms-ssim accumulate] mean {float(v)} vs {float(per_image.mean())}, sum {float(total.compute())} vs {float(per_image.sum())}, tol {tol:.3e}")
    assert abs(float(v) - float(per_image.sum()) / 5) <= tol
    assert abs(float(total.compute()) - float(per_image.sum())) <= tol
    addr = mean.ms_ssim_state.data_ptr()
    mean.reset()
    assert mean.ms_ssim_state.data_ptr() == addr and float(mean.total) == 0 and float(mean.similarity) == 0
    mean.update(pg[:2], tg[:2])
    assert abs(float(mean.compute()) - float(per_image[:2].sum()) / 2) <= tol and float(mean.total) == 2


@pytest.mark.parametrize("case", [1, 3], ids=[CASE_IDS[1], CASE_IDS[3]])
def test_bit_properties(M, case):
    shape, window, betas = CASES[case]
    p, t = pair_of((3,) + shape[1:], 1.0, seed=9)
    pg, tg = p.cuda(), t.cuda()
    kw = dict(data_range=1.0, betas=betas, **option_kwargs(window))
    full = M.multiscale_structural_similarity(pg, tg, **kw)
    assert torch.equal(full, M.multiscale_structural_similarity(pg, tg, **kw))                      # run to run
    alone = M.multiscale_structural_similarity(pg[1:2], tg[1:2], **kw)
    assert torch.equal(alone, full[1:2])                                                             # an image's value is its own
    moved = M.multiscale_structural_similarity(pg.flip(0).contiguous(), tg.flip(0).contiguous(), **kw)
    assert torch.equal(moved, full.flip(0))                                                          # ... wherever it sits
    a, b = M.MultiScaleStructuralSimilarityIndexMeasure(**kw).cuda(), M.MultiScaleStructuralSimilarityIndexMeasure(**kw).cuda()
    a.update(pg, tg)
    b.update(pg, tg)
    assert torch.equal(a.ms_ssim_state[:2], b.ms_ssim_state[:2])


def test_refusals(M):
    x = torch.rand(1, 1, 40, 40, device="cuda")
    with pytest.raises(NotImplementedError):      # sigma 4.5 -> 33 taps
        M.multiscale_structural_similarity(x, x, sigma=4.5, data_range=1.0, betas=(1.0,))
    big = torch.empty(1, 1, 1280, 1280, device="cuda")         # 5 taps << 8: nine scales would fit
    with pytest.raises(NotImplementedError):
        M.multiscale_structural_similarity(big, big, sigma=0.5, data_range=1.0, betas=(0.1,) * 9)
    from ot_vae_lightning_amd import _lib
    words = _lib.load().otvae_ms_ssim_state_words()
    x = torch.rand(2, 1, 32, 32, device="cuda")
    state, win = torch.zeros(words, dtype=torch.float64, device="cuda"), [0.25, 0.5, 0.25]
    call = lambda p, t, st=state, per=None, wh=win, betas=(0.5, 0.5): torch.ops.otvae.ms_ssim_accum(  # noqa: E731
        p, t, wh, win, 0.01, 0.03, 0, 0.0, 1.0, list(betas), 1, st, per)
    for bad in ((x[0], x[0]), (x, x[:1]), (x, x.double()), (x.half(), x.half()), (x.transpose(2, 3), x.transpose(2, 3))):
        with pytest.raises(ValueError):
            call(*bad)
    for kwargs in (dict(st=state[:-1]), dict(st=state.float()), dict(per=torch.zeros(3, dtype=torch.float64, device="cuda")),
                   dict(wh=[0.5, 0.5]), dict(betas=()), dict(betas=(0.2,) * 5)):          # (five scales of 3 taps need 48 pixels)
        with pytest.raises(ValueError):
            call(x, x, **kwargs)
    assert float(state.abs().sum()) == 0                    # nothing ran
    per = torch.zeros(2, dtype=torch.float64, device="cuda")
    call(x, x, per=per)
    assert float(state[1]) == 2 and bool(((per - 1).abs() <= 4 * 2.0 ** -23).all())


def test_update_replays_from_a_captured_graph(M):
    """``update`` inside a capture on a stream of the package's own, then two replays: the state is that of three eager calls -- which
    also shows that ``update`` reads nothing back to the host"""
    from ot_vae_lightning_amd import _lib
    p, t = pair_of((4, 3, 32, 32), 1.0, seed=14)
    pg, tg = p.cuda(), t.cuda()
    kw = dict(sigma=0.5, betas=BETAS[:3], data_range=None)
    eager = M.MultiScaleStructuralSimilarityIndexMeasure(**kw).cuda()
    for _ in range(3):
        eager.update(pg, tg)
    captured = M.MultiScaleStructuralSimilarityIndexMeasure(**kw).cuda()
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
    assert float(captured.total) == 3 * 4
    assert torch.equal(captured.ms_ssim_state[:2], eager.ms_ssim_state[:2]) and torch.equal(captured.compute(), eager.compute())
    del graph
