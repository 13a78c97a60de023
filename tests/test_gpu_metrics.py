"""GPU: the validation metrics (``ot_vae_lightning_amd.metrics``, ``csrc/metrics.hip``) against float64 truth computed in the
test on the CPU.

No fixture from the reference is used: its ``metrics/fid.py`` cannot be imported without torchmetrics (it is the specification
of behaviour, not an oracle); every truth below is formed here in float64.

Bounds.  Moments: products of fp32 inputs are exact in fp64, and any fixed summation order of B terms obeys the recursive-
summation bound, so per entry |err_ij| <= B * 2^-53 * sum_b |f_bi f_bj| (for fp64 inputs the product's own rounding is one of the
B roundings of the fused chain); the same with |f_bi| for the feature sums; the observation count is exact.  The truth is
``f.double().T @ f.double()`` on the CPU; since that product is rounded too, entries that miss the bound against it (and a seeded
sample of the rest) are checked against exact rational arithmetic instead, with the same bound (``_check_moments``).  PSNR: the same
bound on the fp64 sum of squared differences.  Frechet distance: max(1e-8 |B|, 1.5 |A - B|) with A the ``scipy.linalg.sqrtm``
route and B the symmetric eigenvalue route, both float64 LAPACK -- evaluated per case, printed with our value."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import metrics
    return metrics


def _features(b, d, kind, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(b, d, generator=g, dtype=torch.float64)
    if kind == "offset":           # what post-ReLU pooled features look like: a large common offset plus noise
        f = 1e3 + f
    else:                          # mixed sign, a few decades of scale across the features
        f = f * torch.logspace(-2, 2, d, dtype=torch.float64)
    return f.to(dtype)


def _zero_state(d):
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")  # noqa: E731
    return z(1), z(d), z(d, d)


def _truth(f):
    fd = f.double()
    a = fd.abs()
    return fd.T @ fd, fd.sum(0), a.T @ a, a.sum(0)


def _check_moments(state, f, label, parts=1):
    n, sx, sxx = (t.cpu() for t in state)
    b = f.shape[0]
    txx, tx, axx, ax = _truth(f)
    exx, ex = (sxx - txx).abs(), (sx - tx).abs()
    bxx, bx = b * U * axx, b * U * ax
    worst_xx, worst_x = float((exx / bxx.clamp(min=1e-300)).max()), float((ex / bx.clamp(min=1e-300)).max())
    print(f"[moments {label}] n={float(n):.0f} max err/bound vs the BLAS truth: sum_xx {worst_xx:.3f}  sum_x {worst_x:.3f}")
    assert float(n) == b
    assert torch.equal(sxx, sxx.T), "sum_xx is not bit-symmetric"
    # The BLAS product is itself a rounded sum obeying the same bound, so two correct results may differ by up to twice the bound
    # (seen at B = 3: two CPU summation orders 1.26 bounds apart, each within 0.65 of the exact value).  Every entry beyond the
    # bound against BLAS -- and a seeded sample of the others -- is therefore held to the SAME bound against the exact rational
    # value of the same expression.
    fl = f.double()
    g = torch.Generator().manual_seed(b * 7919 + f.shape[1])
    over = (exx > bxx).nonzero().tolist()
    assert len(over) <= 20000, f"sum_xx: {len(over)} entries beyond the bound, max err/bound {worst_xx}"
    d = f.shape[1]
    sample = torch.randint(0, d, (16, 2), generator=g).tolist()
    cols = {}
    col = lambda j: cols.setdefault(j, [Fraction(v) for v in fl[:, j].tolist()])  # noqa: E731
    for i, j in over + sample:
        exact = sum(p * q for p, q in zip(col(i), col(j)))
        bound = Fraction(b) * Fraction(U) * sum(abs(p * q) for p, q in zip(col(i), col(j)))
        err = abs(Fraction(float(sxx[i, j])) - exact)
        assert err <= bound, f"sum_xx[{i}][{j}]: err/bound {float(err / bound) if bound else float('inf')} against the exact value"
    over_x = (ex > bx).nonzero().reshape(-1).tolist()
    for i in over_x + [s_[0] for s_ in sample]:
        exact, bound = sum(col(i)), Fraction(b) * Fraction(U) * sum(abs(p) for p in col(i))
        err = abs(Fraction(float(sx[i])) - exact)
        assert err <= bound, f"sum_x[{i}]: err/bound {float(err / bound) if bound else float('inf')} against the exact value"


@pytest.mark.parametrize("kind", ["mixed", "offset"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("b", [1, 3, 50, 1000, 1024])
@pytest.mark.parametrize("d", [1, 17, 64, 100, 192, 768, 2048])
def test_moments_accum_against_float64_truth(M, d, b, dtype, kind):
    f = _features(b, d, kind, dtype, seed=1000 * d + b)
    fg = f.cuda()
    state = _zero_state(d)
    torch.ops.otvae.moments_accum(fg, *state)
    _check_moments(state, f, f"D={d} B={b} {dtype} {kind}")
    # run-to-run identical
    again = _zero_state(d)
    torch.ops.otvae.moments_accum(fg, *again)
    assert all(torch.equal(p, q) for p, q in zip(state, again))
    # two halves of the batch meet the bound of the whole
    if b >= 2:
        halves = _zero_state(d)
        torch.ops.otvae.moments_accum(fg[:b // 2].contiguous(), *halves)
        torch.ops.otvae.moments_accum(fg[b // 2:].contiguous(), *halves)
        _check_moments(halves, f, f"D={d} B={b} {dtype} {kind} halves")


@pytest.mark.parametrize("d,b", [(100, 50), (192, 1024), (2048, 300)])
def test_moments_accum_propagates_non_finite_features(M, d, b):
    f = _features(b, d, "mixed", torch.float32, seed=5)
    f[b // 2, d // 3] = float("nan")
    f[b - 1, d - 1] = float("inf")
    state = _zero_state(d)
    torch.ops.otvae.moments_accum(f.cuda(), *state)
    n, sx, sxx = (t.cpu() for t in state)
    assert float(n) == b
    assert torch.isnan(sx[d // 3]) and torch.isinf(sx[d - 1])
    assert torch.isnan(sxx[d // 3]).all() and torch.isnan(sxx[:, d // 3]).all()
    assert not torch.isfinite(sxx[d - 1]).any() and not torch.isfinite(sxx[:, d - 1]).any()
    clean = [j for j in range(d) if j not in (d // 3, d - 1)]
    assert torch.isfinite(sxx[clean][:, clean]).all() and torch.isfinite(sx[clean]).all()


def test_moments_accum_workspace_and_arguments(M):
    from ot_vae_lightning_amd import _lib
    lib = _lib.load()
    assert lib.otvae_moments_accum_ws(1024, 2048) < 4.2 * 2048 ** 2 * 8        # the header's multiple (in fact none at this width)
    assert 0 < lib.otvae_moments_accum_ws(1024, 768) <= (4 * 768 ** 2 + 264 * 768) * 8
    state = _zero_state(8)
    with pytest.raises(ValueError):
        torch.ops.otvae.moments_accum(torch.zeros(4, 9, device="cuda"), *state)
    with pytest.raises(ValueError):
        torch.ops.otvae.moments_accum(torch.zeros(4, 8, device="cuda"), state[0], state[1], state[2].float())
    with pytest.raises(ValueError):
        torch.ops.otvae.moments_accum(torch.zeros(4, 2049, device="cuda"), *_zero_state(2049))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("d,b", [(1, 50), (17, 1000), (64, 1024), (100, 3), (192, 1024), (256, 1000)])
def test_moments_accum_agrees_with_gauss_stats(M, d, b, dtype):
    """neither kernel is the other's truth: they may differ by the sum of their two summation bounds"""
    from ot_vae_lightning_amd import _lib
    from ot_vae_lightning_amd._lib import check, ptr, stream
    lib = _lib.load()
    f = _features(b, d, "offset", dtype, seed=77 + d)
    fg = f.cuda()
    new = _zero_state(d)
    torch.ops.otvae.moments_accum(fg, *new)
    old = _zero_state(d)
    ws = torch.empty(max(8, lib.otvae_gauss_stats_ws(1, b, d, 0)), device="cuda", dtype=torch.uint8)
    check(lib.otvae_gauss_stats(0 if dtype == torch.float32 else 1, ptr(fg), 1, b, d, 0, 1, -1.0, ptr(ws), ptr(old[0]), ptr(old[1]),
                                ptr(old[2]), stream()), "otvae_gauss_stats")
    _, _, axx, ax = _truth(f)
    assert float(new[0]) == float(old[0]) == b
    dxx, dx = (new[2] - old[2]).abs().cpu(), (new[1] - old[1]).abs().cpu()
    print(f"[agreement D={d} B={b} {dtype}] max diff/bound: sum_xx {float((dxx / (2 * b * U * axx)).max()):.3f} "
          f"sum_x {float((dx / (2 * b * U * ax)).max()):.3f}")
    assert bool((dxx <= 2 * b * U * axx).all()) and bool((dx <= 2 * b * U * ax).all())


# ---------------------------------------------------------------------------------------------------------------- PSNR
@pytest.mark.parametrize("data_range", [1.0, None], ids=["given", "tracked"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_psnr_against_float64_truth(M, data_range, dtype):
    g = torch.Generator().manual_seed(3)
    metric = M.PeakSignalNoiseRatio(data_range=data_range).cuda()
    ps, ts = [], []
    for shape in ((7, 1, 32, 32), (1, 3, 5, 5), (64, 3, 33, 31)):            # three updates of different sizes
        t = torch.rand(shape, generator=g, dtype=torch.float64).to(dtype)
        p = (t.double() + 0.05 * torch.randn(shape, generator=g, dtype=torch.float64)).to(dtype)
        metric.update(p.cuda(), t.cuda())
        ps.append(p.double().reshape(-1))
        ts.append(t.double().reshape(-1))
    p, t = torch.cat(ps), torch.cat(ts)
    sq = (p - t) ** 2
    n = p.numel()
    sse = float(metric.sum_squared_error)
    print(f"[psnr {dtype} range={data_range}] sse {sse!r} truth {float(sq.sum())!r} bound {n * U * float(sq.sum()):.3e}")
    assert float(metric.total) == n
    assert abs(sse - float(sq.sum())) <= n * U * float(sq.sum())
    assert float(metric.min_target) == float(t.min()) and float(metric.max_target) == float(t.max())
    rng = 1.0 if data_range is not None else float(t.max() - t.min())
    want = 10 * math.log10(rng ** 2 / float(sq.mean()))
    got = float(metric.compute())
    print(f"[psnr {dtype} range={data_range}] ours {got!r} truth {want!r}")
    assert abs(got - want) <= (10 / math.log(10)) * (n * U + 8 * U) + 4 * U * abs(want)   # d psnr = 10 / ln 10 * d mse / mse
    metric.reset()
    assert float(metric.total) == 0 and float(metric.sum_squared_error) == 0


def test_psnr_of_identical_tensors_is_inf(M):
    metric = M.PeakSignalNoiseRatio(data_range=1.0).cuda()
    x = torch.rand(4, 3, 16, 16, device="cuda")
    metric.update(x, x.clone())
    assert float(metric.compute()) == float("inf")
    with pytest.raises(ValueError):
        metric.update(x, x[:2])


# ---------------------------------------------------------------------------------------------------------------- Frechet distance
def _stream_pair(d, n, seed):
    """two fp32 feature streams of the same family (ReLU of a random affine map of Gaussian codes), different parameters"""
    g = torch.Generator().manual_seed(seed)
    k = min(d, 96)
    out = []
    for s in range(2):
        w = torch.randn(k, d, generator=g, dtype=torch.float64) / math.sqrt(k)
        bias = 0.3 * torch.randn(d, generator=g, dtype=torch.float64) + 0.1 * s
        z = torch.randn(n, k, generator=g, dtype=torch.float64)
        noise = 0.2 * torch.randn(n, d, generator=g, dtype=torch.float64)
        out.append(torch.relu(z @ w + bias + noise).float())
    return out


def _moments64(f):
    fd = f.double()
    mu = fd.mean(0)
    return mu.numpy(), (fd.T @ fd / fd.shape[0] - torch.outer(mu, mu)).numpy()


def _fid_truths(m1, c1, m2, c2):
    import scipy.linalg
    base = float(((m1 - m2) ** 2).sum() + np.trace(c1) + np.trace(c2))
    root = scipy.linalg.sqrtm(c1 @ c2)
    a = base - 2.0 * float(np.trace(root).real)                              # what torchmetrics' _compute_fid historically did
    lam, v = np.linalg.eigh(c1)
    r1 = (v * np.sqrt(np.clip(lam, 0.0, None))) @ v.T
    inner = r1 @ c2 @ r1
    ev = np.linalg.eigh((inner + inner.T) / 2)[0]
    b = base - 2.0 * float(np.sqrt(np.clip(ev, 0.0, None)).sum())
    return a, b


@pytest.mark.parametrize("d,n", [(64, 4096), (768, 4096), (2048, 1000)])
def test_frechet_distance_against_two_lapack_routes(M, d, n):
    """Measured on one MI355X (A = sqrtm route, B = eigenvalue route, ours, tolerance max(1e-8 |B|, 1.5 |A - B|)):

        D = 64,   n = 4096: A 10.444689667774576  B 10.444689667774654  ours 10.444689667774675  tol 1.04e-07
        D = 768,  n = 4096: A 295.6758395370451   B 295.6758395370459   ours 295.6758395370415   tol 2.96e-06
        D = 2048, n = 1000: A 1154.9388107617199  B 1154.9388505974007  ours 1154.9388636630938  tol 5.98e-05

    The D = 2048 case (singular covariances) was 6.3e-2 off while the block eigensolver for 1024 < D <= 2048 stopped after 14 sweeps
    (residual 6e-9); with its budget of 28 sweeps (``EIGH_BLOCK_SWEEPS_WIDE``, gaussian_ot.hip) the residual is at its floor."""
    f1, f2 = _stream_pair(d, n, seed=d)
    metric = M.FrechetDistance(d).cuda()
    assert torch.isinf(metric.compute()).all()
    for lo in range(0, n, 1000):                                              # uneven last batch at n = 4096
        metric.update(f1[lo:lo + 1000].cuda(), f2[lo:lo + 1000].cuda())
    assert float(metric.num_real_obs) == n and float(metric.num_fake_obs) == n
    ours = float(metric.compute())
    m1, c1 = _moments64(f1)
    m2, c2 = _moments64(f2)
    a, b = _fid_truths(m1, c1, m2, c2)
    tol = max(1e-8 * abs(b), 1.5 * abs(a - b))
    print(f"[fid D={d} n={n}] A (sqrtm)    {a!r}\n[fid D={d} n={n}] B (eigh)     {b!r}\n[fid D={d} n={n}] ours         {ours!r}   "
          f"tol {tol:.3e}")
    assert abs(ours - b) <= tol and abs(ours - a) <= tol + abs(a - b)

    # equal streams on both sides: 0
    metric.reset()
    assert torch.isinf(metric.compute()).all()
    for lo in range(0, n, 1000):
        metric.update(f1[lo:lo + 1000].cuda(), f1[lo:lo + 1000].cuda())
    same = float(metric.compute())
    print(f"[fid D={d} n={n}] equal streams {same!r}")
    assert abs(same) <= tol

    # a pure mean shift delta: |delta|^2
    delta = torch.linspace(-1.0, 1.0, d, dtype=torch.float64)
    shifted = (f1.double() + delta).cuda()                                    # fp64 features: the covariance is unchanged up to round-off
    metric.reset()
    for lo in range(0, n, 1000):
        metric.update(f1[lo:lo + 1000].double().cuda(), shifted[lo:lo + 1000])
    shift = float(metric.compute())
    print(f"[fid D={d} n={n}] mean shift   {shift!r} truth {float((delta ** 2).sum())!r}")
    assert abs(shift - float((delta ** 2).sum())) <= tol


# ---------------------------------------------------------------------------------------------------------------- in the model
class _ConvPoolNet(torch.nn.Module):
    """fixed feature network built from a seeded generator: 3 x 3 convolution (as unfold + product) -> ReLU -> global average pool,
    in float64 so that the CPU truth and the device run differ by summation order only"""

    def __init__(self, width=64, seed=11):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.register_buffer("weight", torch.randn(width, 27, generator=g, dtype=torch.float64) / 3.0)
        self.register_buffer("bias", 0.1 * torch.randn(width, generator=g, dtype=torch.float64))

    def forward(self, img):
        cols = F.unfold(img.double(), 3, padding=1)                           # [B, 27, L]
        return torch.relu(self.weight @ cols + self.bias[:, None]).mean(-1)   # [B, width]


def _model(A, M, metrics):
    torch.manual_seed(0)
    enc = A.CNN(1, 16, 16, 1, capacity=4, down_sample=True, residual="add")
    dec = A.CNN(8, 1, 1, 16, capacity=4, up_sample=True, residual="add")
    return A.VAE(encoder=enc, decoder=dec, prior=A.GaussianPrior(loss_coeff=0.1), metrics=metrics).cuda().eval()


def test_validation_loop_logs_psnr_and_fid(M):
    import ot_vae_lightning_amd as A
    from ot_vae_lightning_amd.utils.synthetic import mnist_like
    net = _ConvPoolNet()
    coll = M.MetricCollection({"psnr": M.PeakSignalNoiseRatio(data_range=1.),
                               "fid": M.FrechetInceptionDistance(net=net, feature_size=64)})
    model = _model(A, M, coll)
    assert model.monitor == "val/metrics/psnr"
    images = mnist_like(1100, 5)[:, :, 8:24, 8:24].contiguous()
    model.on_validation_start()
    model.on_validation_epoch_start()
    steps, lo, i = [], 0, 0
    for size in (300, 257, 1, 400, 142):                                      # >= 1000 images in uneven batches
        out = model.validation_step((images[lo:lo + size].cuda(), None), i)
        steps.append({k: out[k].detach().double().cpu() for k in ("preds", "target", "generated", "samples")})
        lo, i = lo + size, i + 1
    assert lo == 1100
    res = model.on_validation_epoch_end()
    assert set(model.logged) == {"val/metrics/psnr", "val/metrics/fid"} and model.monitor in model.logged
    assert set(res) == set(model.logged)

    cat = {k: torch.cat([s[k] for s in steps]) for k in steps[0]}
    assert torch.equal(cat["samples"], images.double()) and cat["generated"].shape == images.shape
    sq = (cat["preds"] - cat["target"]) ** 2
    n = sq.numel()
    want_psnr = 10 * math.log10(1.0 / float(sq.mean()))
    got_psnr = float(model.logged["val/metrics/psnr"])
    print(f"[model] psnr ours {got_psnr!r} truth {want_psnr!r}")
    assert abs(got_psnr - want_psnr) <= (10 / math.log(10)) * (n * U + 8 * U) + 4 * U * abs(want_psnr)

    cpu_net = _ConvPoolNet()
    tile = lambda x: torch.cat([x, x, x], 1)  # noqa: E731
    m1, c1 = _moments64(cpu_net(tile(cat["generated"])))
    m2, c2 = _moments64(cpu_net(tile(cat["samples"])))
    a, b = _fid_truths(m1, c1, m2, c2)
    tol = max(1e-8 * abs(b), 1.5 * abs(a - b))
    got_fid = float(model.logged["val/metrics/fid"])
    print(f"[model] fid A {a!r} B {b!r} ours {got_fid!r} tol {tol:.3e}")
    assert abs(got_fid - b) <= tol

    # the collection is reset afterwards
    assert float(model.val_metrics["fid"].num_real_obs) == 0 and float(model.val_metrics["psnr"].total) == 0
    assert torch.isinf(model.val_metrics["fid"].compute()).all()
    assert float(model.test_metrics["fid"].num_real_obs) == 0                 # the test clone never saw the validation data

    # the same run without metrics logs nothing and raises nothing
    plain = _model(A, M, None)
    plain.on_validation_start()
    plain.on_validation_epoch_start()
    assert plain.validation_step((images[:64].cuda(), None), 0) is None
    assert plain.on_validation_epoch_end() is None and plain.logged == {}


def test_updates_replay_from_a_captured_graph(M):
    """``update`` of both metrics inside a capture on a stream of our own (linear, no side branch): a replay gives the state of the
    eager call -- which also shows that ``update`` reads nothing back to the host"""
    from ot_vae_lightning_amd import _lib
    g = torch.Generator().manual_seed(9)
    feats_a = torch.randn(1024, 192, generator=g).cuda()
    feats_b = torch.randn(1024, 192, generator=g).cuda().double()
    wide = torch.randn(256, 2048, generator=g).cuda()
    p, t = torch.rand(32, 3, 16, 16, generator=g).cuda(), torch.rand(32, 3, 16, 16, generator=g).cuda()

    def build():
        return M.FrechetDistance(192).cuda(), M.FrechetDistance(2048).cuda(), M.PeakSignalNoiseRatio().cuda()

    def run(fd, fw, ps):
        fd.update(feats_a, feats_b)
        fw.update(wide, None)
        ps.update(p, t)

    eager = build()
    run(*eager)
    captured = build()
    torch.cuda.synchronize()
    s = _lib.fresh_stream("cuda")
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        run(*captured)
    torch.cuda.synchronize()
    for m in captured:
        m.reset()                                                             # (whatever the capture itself left behind)
    graph.replay()
    torch.cuda.synchronize()
    for me, mc in zip(eager, captured):
        for name in me._defaults:
            a, b = getattr(me, name), getattr(mc, name)
            if name == "sqerr_state":
                a, b = a[:4], b[:4]
            assert torch.equal(a, b), name
    graph.replay()                                                            # a second replay accumulates again
    torch.cuda.synchronize()
    assert float(captured[0].num_real_obs) == 2048 and float(captured[2].total) == 2 * p.numel()
    del graph
