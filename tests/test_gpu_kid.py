"""GPU: the Kernel Inception Distance (``ot_vae_lightning_amd.metrics.kid``, ``csrc/kid.hip``) against float64 truth computed in the
test on the CPU from the estimator's formulas (the reference has no KID; torchmetrics' ``poly_kernel`` /
``maximum_mean_discrepancy`` are the specification).

Bound (derived, not fitted).  u = 2^-53, G_ij = gamma <a_i, b_j> + coef, k_ij = G_ij^degree.  The fp32 features are exact in fp64, a
D-long fp64 dot product in any order errs by at most D u sum_d |a_id b_jd|, which G^degree magnifies by degree |G|^(degree - 1) gamma;
forming G and the degree - 1 multiplications add (degree + 1) u |k_ij|:

    e_ij = degree |G_ij|^(degree - 1) gamma D u sum_d |a_id b_jd|  +  (degree + 1) u |k_ij|

and a block sum of n terms adds n u sum |k_ij|.  The three blocks are combined with the estimator's weights.  The CPU truth is rounded
under the same bound, hence ``|ours - truth| <= 2 bound``.  The bound sits orders of magnitude below the value it bounds (printed per
case); an fp32 composition misses it by 2e-7 ... 3e-4.

The kernel works on 128 x 128 tiles of the Gram blocks: m = 2 and 33 are one masked tile, 65 sits across the 64-row quarters the four
waves own, 130 has an off-diagonal tile (3 + 4 tiles), 257 three tiles per side.  D = 96 and 2048 stage the panels with 16-byte loads,
D = 1 and 70 (no multiple of 4) with 4-byte loads; 70 and 96 end in a partial chunk of 32 features."""
import math
from fractions import Fraction

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CONFIGS = [(degree, coef, gamma) for degree in (1, 2, 3) for coef in (0.0, 1.0) for gamma in (None, 0.37)]


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import metrics
    return metrics


def _features(n, d, kind, seed, shift=0.0):
    """fp32 features: "mixed" -- mixed sign, decades of scale across the features; "offset" -- 3 + noise (post-ReLU-like: every
    inner product is a large positive number, the estimator cancels heavily)"""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n, d, generator=g, dtype=torch.float64)
    if kind == "offset":
        f = 3.0 + shift + (1.0 + shift) * f
    else:
        f = (f * (1.0 + shift) + shift) * torch.logspace(-2, 2, d, dtype=torch.float64)
    return f.float()


def _pair(m, d, kind, seed):
    n_real, n_fake = max(150, m + 20), max(97, m + 7)
    return _features(n_real, d, kind, seed), _features(n_fake, d, kind, seed + 1, shift=0.25)


def _block(a, b, degree, gamma, coef, skip_diagonal):
    d = a.shape[1]
    dot, absdot = a @ b.T, a.abs() @ b.abs().T
    g = gamma * dot + coef
    k = g ** degree
    e = degree * g.abs() ** (degree - 1) * gamma * d * U * absdot + (degree + 1) * U * k.abs()
    if skip_diagonal:
        keep = ~torch.eye(a.shape[0], dtype=torch.bool)
        k, e = k * keep, e * keep
        n = a.shape[0] * (a.shape[0] - 1)
    else:
        n = a.shape[0] * b.shape[0]
    return float(k.sum()), float(e.sum() + n * U * k.abs().sum())


def _truth(x, y, degree, gamma, coef):
    """(value, bound) of one subset: x, y [m, D] float64 on the CPU"""
    m = x.shape[0]
    sxx, bxx = _block(x, x, degree, gamma, coef, True)
    syy, byy = _block(y, y, degree, gamma, coef, True)
    sxy, bxy = _block(x, y, degree, gamma, coef, False)
    return (sxx + syy) / (m * (m - 1)) - 2 * sxy / m ** 2, (bxx + byy) / (m * (m - 1)) + 2 * bxy / m ** 2


def _check_values(per, real, fake, idx_real, idx_fake, degree, gamma, coef, label):
    rd, fd = real.double(), fake.double()
    for s, got in enumerate(per.tolist()):
        want, bound = _truth(rd[idx_real[s].long()], fd[idx_fake[s].long()], degree, gamma, coef)
        err = abs(got - want)
        print(f"[kid {label} s={s}] ours {got!r} truth {want!r} err {err:.3e} 2*bound {2 * bound:.3e}")
        assert math.isfinite(got) and err <= 2 * bound, (label, s, got, want, err, bound)


def _exact_stats(values):
    fr = [Fraction(v) for v in values]
    mean = sum(fr) / len(fr)
    var = sum((v - mean) ** 2 for v in fr) / len(fr)
    return float(mean), math.sqrt(float(var))


def _check_stats(per, stats, label):
    mean, std = _exact_stats(per.tolist())
    got_mean, got_std = stats.tolist()
    print(f"[kid {label}] mean {got_mean!r} exact {mean!r}  std {got_std!r} exact {std!r}")
    assert abs(got_mean - mean) <= 4 * math.ulp(mean) and abs(got_std - std) <= 4 * math.ulp(std), (label, got_mean, mean, got_std, std)


def _subsets(M, real_g, fake_g, s, m, seed):
    out = M.kernel_distance(real_g, fake_g, subsets=s, subset_size=m, seed=seed, return_subsets=True)
    return out[3], out[4]


# ---------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("kind", ["mixed", "offset"])
@pytest.mark.parametrize("s", [1, 5])
@pytest.mark.parametrize("d", [1, 70, 96])
@pytest.mark.parametrize("m", [2, 33, 65, 130, 257])
def test_subset_mmd_against_float64_truth(M, m, d, s, kind):
    real, fake = _pair(m, d, kind, seed=1000 * m + d)
    real_g, fake_g = real.cuda(), fake.cuda()
    idx_real, idx_fake = _subsets(M, real_g, fake_g, s, m, seed=m + d)
    assert idx_real.shape == idx_fake.shape == (s, m) and idx_real.dtype == torch.int32
    ir, jf = idx_real.cpu(), idx_fake.cpu()
    for rows, n in ((ir, real.shape[0]), (jf, fake.shape[0])):
        assert int(rows.min()) >= 0 and int(rows.max()) < n and all(len(set(r.tolist())) == m for r in rows)
    for degree, coef, gamma in CONFIGS:
        gm = 1.0 / d if gamma is None else gamma
        per, stats = torch.ops.otvae.poly_mmd_subsets(real_g, fake_g, idx_real, idx_fake, m, degree, gm, coef)
        label = f"m={m} D={d} S={s} {kind} degree={degree} coef={coef} gamma={gamma}"
        _check_values(per.cpu(), real, fake, ir, jf, degree, gm, coef, label)
        _check_stats(per.cpu(), stats.cpu(), label)


@pytest.mark.parametrize("kind", ["mixed", "offset"])
def test_subset_mmd_at_the_widest_features(M, kind):
    m, d, s = 65, 2048, 2
    real, fake = _pair(m, d, kind, seed=77)
    real_g, fake_g = real.cuda(), fake.cuda()
    idx_real, idx_fake = _subsets(M, real_g, fake_g, s, m, seed=3)
    for degree, coef, gamma in ((3, 1.0, None), (2, 0.0, 0.37)):
        gm = 1.0 / d if gamma is None else gamma
        per, stats = torch.ops.otvae.poly_mmd_subsets(real_g, fake_g, idx_real, idx_fake, m, degree, gm, coef)
        label = f"m={m} D={d} S={s} {kind} degree={degree} coef={coef} gamma={gamma}"
        _check_values(per.cpu(), real, fake, idx_real.cpu(), idx_fake.cpu(), degree, gm, coef, label)
        _check_stats(per.cpu(), stats.cpu(), label)


def test_functional_forms(M):
    real, fake = _pair(65, 70, "offset", seed=5)
    real_g, fake_g = real.cuda(), fake.cuda()
    mean, std, per, idx_real, idx_fake = M.kernel_distance(real_g, fake_g, subsets=5, subset_size=65, seed=9, return_subsets=True)
    assert mean.dim() == 0 and std.dim() == 0 and mean.dtype == std.dtype == per.dtype == torch.float64 and per.shape == (5,)
    _check_values(per.cpu(), real, fake, idx_real.cpu(), idx_fake.cpu(), 3, 1.0 / 70, 1.0, "kernel_distance")
    _check_stats(per.cpu(), torch.stack([mean, std]).cpu(), "kernel_distance")
    again = M.kernel_distance(real_g, fake_g, subsets=5, subset_size=65, seed=9)
    assert torch.equal(again[0], mean) and torch.equal(again[1], std)
    # poly_mmd2: all rows of two equally sized sets, one subset, no indices
    x, y = real[:97], fake[:97]
    got = M.poly_mmd2(x.cuda(), y.cuda(), degree=2, gamma=0.37, coef=1.0)
    assert got.dim() == 0 and got.dtype == torch.float64
    rows = torch.arange(97, dtype=torch.int32)[None]
    _check_values(got.reshape(1).cpu(), x, y, rows, rows, 2, 0.37, 1.0, "poly_mmd2")
    with pytest.raises(ValueError, match="subset_size"):
        M.kernel_distance(real_g, fake_g, subsets=2, subset_size=fake.shape[0] + 1)
    with pytest.raises(NotImplementedError):
        torch.ops.otvae.poly_mmd_subsets(real_g, fake_g, None, None, 8, 9, 0.1, 1.0)
    with pytest.raises(ValueError):
        torch.ops.otvae.poly_mmd_subsets(real_g, fake_g, idx_real, None, 65, 3, 0.1, 1.0)
    with pytest.raises(ValueError):
        torch.ops.otvae.poly_mmd_subsets(real_g.double(), fake_g.double(), None, None, 8, 3, 0.1, 1.0)


# ---------------------------------------------------------------------------------------------------------------- 2. structure
@pytest.mark.parametrize("m,d", [(33, 70), (130, 96), (257, 70)])
def test_structure(M, m, d):
    real, fake = _pair(m, d, "offset", seed=m)
    real_g, fake_g = real.cuda(), fake.cuda()
    s = 4
    idx_real, idx_fake = _subsets(M, real_g, fake_g, s, m, seed=1)
    op = torch.ops.otvae.poly_mmd_subsets
    gm = 1.0 / d
    per, stats = op(real_g, fake_g, idx_real, idx_fake, m, 3, gm, 1.0)
    per2, stats2 = op(real_g, fake_g, idx_real, idx_fake, m, 3, gm, 1.0)
    assert torch.equal(per, per2) and torch.equal(stats, stats2), "two identical calls differ"
    # the estimator is symmetric in its two sides: so are the bits
    swapped, _ = op(fake_g, real_g, idx_fake, idx_real, m, 3, gm, 1.0)
    assert torch.equal(per, swapped), (per - swapped).tolist()
    # no indices == rows 0 .. m - 1 in every subset
    plain, plain_stats = op(real_g, fake_g, None, None, m, 3, gm, 1.0)
    rows = torch.arange(m, dtype=torch.int32, device="cuda").repeat(3, 1).contiguous()
    explicit, _ = op(real_g, fake_g, rows, rows, m, 3, gm, 1.0)
    assert plain.shape == (1,) and torch.equal(explicit, plain.expand(3))
    assert float(plain_stats[0]) == float(plain[0]) and float(plain_stats[1]) == 0.0
    # a subset depends on its own index rows alone: repeated elsewhere, among other subsets, it gives the same bits
    mixed_real = torch.stack([idx_real[2], idx_real[0], idx_real[2]]).contiguous()
    mixed_fake = torch.stack([idx_fake[2], idx_fake[0], idx_fake[2]]).contiguous()
    mixed, _ = op(real_g, fake_g, mixed_real, mixed_fake, m, 3, gm, 1.0)
    assert torch.equal(mixed, per[[2, 0, 2]])
    # features that do not start on a 16-byte boundary take the 4-byte staging loads (as every D that is no multiple of 4 does): the
    # products meet the matrix cores in the same order, so the bits are the same
    shifted = torch.empty(real_g.numel() + 1, device="cuda")[1:].view_as(real_g).copy_(real_g)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    assert torch.equal(op(shifted, fake_g, idx_real, idx_fake, m, 3, gm, 1.0)[0], per)
    # a stray index is clamped into the rows, never followed
    stray = idx_real.clone()
    stray[0, 0], stray[1, 1] = real.shape[0] + 5, -3
    clamped = idx_real.clone()
    clamped[0, 0], clamped[1, 1] = real.shape[0] - 1, 0
    assert torch.equal(op(real_g, fake_g, stray, idx_fake, m, 3, gm, 1.0)[0], op(real_g, fake_g, clamped, idx_fake, m, 3, gm, 1.0)[0])


# ---------------------------------------------------------------------------------------------------------------- 3. feature store
def test_feature_store_appends_and_stops_at_the_capacity():
    import ot_vae_lightning_amd  # noqa: F401
    d, cap, guard = 70, 100, 16
    g = torch.Generator().manual_seed(2)
    batches = [torch.randn(40, d, generator=g), torch.randn(40, d, generator=g, dtype=torch.float64) * 1e3, torch.randn(40, d, generator=g)]
    arena = torch.full((cap + guard, d), -7.0, device="cuda")
    buf = arena[:cap]
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    want_counts = [[40, 40], [80, 80], [100, 120]]
    for b, want in zip(batches, want_counts):
        torch.ops.otvae.feature_append(b.cuda(), buf, count)
        assert count.tolist() == want
    want = torch.cat([b.float() for b in batches])[:cap]            # the float64 batch is rounded to float32
    assert torch.equal(buf.cpu(), want)
    assert bool((arena[cap:] == -7.0).all()), "rows beyond the capacity were written"
    torch.ops.otvae.feature_append(batches[0].cuda(), buf, count)   # a full store stays as it is
    assert count.tolist() == [100, 160] and torch.equal(buf.cpu(), want) and bool((arena[cap:] == -7.0).all())
    with pytest.raises(ValueError):
        torch.ops.otvae.feature_append(batches[0][:, :8].cuda(), buf, count)
    with pytest.raises(ValueError):
        torch.ops.otvae.feature_append(batches[0].cuda(), buf, count.int())


def test_update_replays_from_a_captured_graph(M):
    """the append offset is read on the device: a captured ``update`` lands behind what earlier calls stored, on every replay"""
    from ot_vae_lightning_amd import _lib
    g = torch.Generator().manual_seed(4)
    gen_feats, smp_feats = torch.randn(24, 70, generator=g).cuda(), torch.randn(17, 70, generator=g).cuda().double()
    metric = M.KernelDistance(feature_size=70, max_observations=64, subsets=2, subset_size=8).cuda()
    addr = [getattr(metric, n).data_ptr() for n in metric._defaults]
    torch.cuda.synchronize()
    s = _lib.fresh_stream("cuda")
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metric.update(gen_feats, smp_feats)                          # warm-up: stored 24 / 17
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        metric.update(gen_feats, smp_feats)
    torch.cuda.synchronize()
    assert metric.num_real.tolist() == [24, 24] and metric.num_fake.tolist() == [17, 17]   # a capture runs nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert metric.num_real.tolist() == [64, 72] and metric.num_fake.tolist() == [51, 51]
    assert torch.equal(metric.real_features, torch.cat([gen_feats] * 3)[:64])
    assert torch.equal(metric.fake_features[:51], torch.cat([smp_feats.float()] * 3))
    assert bool((metric.fake_features[51:] == 0).all())
    assert [getattr(metric, n).data_ptr() for n in metric._defaults] == addr
    del graph


# ---------------------------------------------------------------------------------------------------------------- 4. metric class
def _fed(M, real, fake, seed, cuts=((0, 50), (50, 51), (51, None))):
    metric = M.KernelDistance(feature_size=70, max_observations=256, subsets=5, subset_size=33, seed=seed).cuda()
    for lo, hi in cuts:                                              # three uneven batches per side
        metric.update(real[lo:hi].cuda(), fake[lo:hi].cuda())
    return metric


def test_kernel_distance_metric(M):
    real, fake = _pair(33, 70, "offset", seed=21)                    # 150 and 97 rows
    metric = _fed(M, real, fake, seed=1)
    assert metric.num_real.tolist() == [150, 150] and metric.num_fake.tolist() == [97, 97]
    assert torch.equal(metric.real_features[:150].cpu(), real) and torch.equal(metric.fake_features[:97].cpu(), fake)
    mean, std = metric.compute()
    idx_real, idx_fake, per = metric.last_subsets
    assert idx_real.shape == idx_fake.shape == (5, 33)
    for rows, n in ((idx_real.cpu(), 150), (idx_fake.cpu(), 97)):
        assert int(rows.min()) >= 0 and int(rows.max()) < n and all(len(set(r.tolist())) == 33 for r in rows)
    _check_values(per.cpu(), real, fake, idx_real.cpu(), idx_fake.cpu(), 3, 1.0 / 70, 1.0, "metric")
    _check_stats(per.cpu(), torch.stack([mean, std]).cpu(), "metric")
    twin = _fed(M, real, fake, seed=1)
    tmean, tstd = twin.compute()
    assert torch.equal(tmean, mean) and torch.equal(tstd, std) and torch.equal(twin.last_subsets[0], idx_real)
    other = _fed(M, real, fake, seed=2)
    other.compute()
    assert not torch.equal(other.last_subsets[0], idx_real) and not torch.equal(other.last_subsets[1], idx_fake)
    # reset: the counts go to zero where they are
    addr = [getattr(metric, n).data_ptr() for n in metric._defaults]
    metric.reset()
    assert metric.num_real.tolist() == [0, 0] and metric.num_fake.tolist() == [0, 0]
    assert [getattr(metric, n).data_ptr() for n in metric._defaults] == addr
    with pytest.raises(ValueError, match="Argument `subset_size` should be smaller than the number of samples"):
        metric.compute()
    metric.update(real[:40].cuda(), fake[:32].cuda())                # 32 < 33 rows on one side
    with pytest.raises(ValueError, match="Argument `subset_size` should be smaller than the number of samples"):
        metric.compute()
    metric.update(None, fake[32:33].cuda())
    assert all(bool(torch.isfinite(v)) for v in metric.compute())


def test_kernel_inception_distance_in_a_collection(M):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 8 * 8, 24)).cuda()
    kid = M.KernelInceptionDistance(net=net, feature_size=24, max_observations=128, subsets=4, subset_size=20, seed=6)
    coll = M.MetricCollection({"psnr": M.PeakSignalNoiseRatio(data_range=1.0), "kid": kid}).cuda()
    coll.train()
    assert not net.training                                          # the feature network never trains
    g = torch.Generator().manual_seed(8)
    real_feats, fake_feats = [], []
    for size in (30, 1, 33):
        samples = torch.rand(size, 1, 8, 8, generator=g).cuda()
        batch = {"samples": samples, "target": samples, "preds": (samples + 0.05 * torch.rand(size, 1, 8, 8, generator=g).cuda()),
                 "generated": torch.rand(size, 1, 8, 8, generator=g).cuda() ** 2, "kwargs": {}}
        assert coll(**batch) == {}                                   # nothing computes on the step
        with torch.no_grad():
            real_feats.append(net(torch.cat([batch["generated"]] * 3, 1)))
            fake_feats.append(net(torch.cat([batch["samples"]] * 3, 1)))
    res = coll.compute()
    assert set(res) == {"psnr", "kid_mean", "kid_std"}
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in res.values())
    want = M.kernel_distance(torch.cat(real_feats), torch.cat(fake_feats), subsets=4, subset_size=20, seed=6)
    assert torch.equal(res["kid_mean"], want[0]) and torch.equal(res["kid_std"], want[1])
    assert float(res["kid_mean"]) > 0 and float(res["kid_std"]) > 0
    coll.reset()
    assert kid.num_real.tolist() == [0, 0]
