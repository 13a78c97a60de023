"""GPU: precision / recall / density / coverage (``ot_vae_lightning_amd.metrics.prdc``, ``csrc/knn_manifold.hip``) against CPU truth
(``prdc_cases``).  Every count and every radius must match EXACTLY; the inputs make that a fair demand:

  * dyadic and lattice features -- the kernel's fp64 Gram form is exact on them, the truth is int64 arithmetic;
  * float features -- the truth is the fp64 difference form; the test first ASSERTS that every decision of the truth clears four times
    the Gram form's error bound (``prdc_cases`` derives it; the smallest margin over these shapes is 1e5 times the bound), then demands
    equal counts and radii within twice the bound.

Shapes (N, M, D, k).  The kernels work on 128 x 128 tiles: (4, 5, 1, 3) is k = n - 1 and D = 1 with 4-byte loads; (33, 33, 70, 3) one
masked tile, D no multiple of 4, a partial chunk of 32 features; (65, 40, 96, 5) sits across the 64-row quarters of the waves;
(130, 97, 2048, 3) has an off-diagonal tile, 16-byte loads, the widest features; (257, 257, 96, 5) three tiles a side;
(257, 130, 2048, 16) the largest k (and the kernel variant with 16 list slots); (1025, 300, 32, 5) nine column tiles.
``otvae_knn_sq_radii`` splits the nt column tiles of a row strip over G workgroups, G the smallest minimiser of
ceil(nt G / 512) ceil(nt / G): at 1025 rows nt = G = 9, so NINE workgroups contribute candidates to one row and each sees one column
tile; at 2817 rows (``WALK_SHAPE``) nt = 23, G = 12, so eleven workgroups of every strip WALK TWO column tiles with a running k-list --
the smallest row count at which that happens (22 strips still get one workgroup per tile)."""
import pytest
import torch

import prdc_cases as C

pytestmark = pytest.mark.gpu

NAMES = ("precision", "recall", "density", "coverage")
ALL_SHAPES = C.SHAPES + [C.WALK_SHAPE]


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import metrics
    return metrics


def _ops(real, fake, k):
    real_g, fake_g = real.cuda(), fake.cuda()
    r2_real, r2_fake = torch.ops.otvae.knn_sq_radii(real_g, k), torch.ops.otvae.knn_sq_radii(fake_g, k)
    count_fake, hit_real, min_real = torch.ops.otvae.manifold_counts(real_g, r2_real, fake_g, r2_fake)
    assert r2_real.dtype == r2_fake.dtype == min_real.dtype == torch.float64
    assert count_fake.dtype == hit_real.dtype == torch.int32
    assert count_fake.shape == r2_fake.shape == (fake.shape[0],) and hit_real.shape == min_real.shape == r2_real.shape == (real.shape[0],)
    return dict(r_real=r2_real.cpu(), r_fake=r2_fake.cpu(), count_fake=count_fake.cpu(), hit_real=hit_real.cpu(), min_real=min_real.cpu())


def _assert_counts(got, t, label):
    assert torch.equal(got["count_fake"].long(), t["count_fake"]), (label, "count_fake")
    assert torch.equal(got["hit_real"].bool(), t["hit_real"]), (label, "hit_real")


def _assert_values(got, t, label):
    assert len(got) == 4
    for name, g in zip(NAMES, got):
        assert g.dtype == torch.float64 and g.dim() == 0
        assert float(g) == t[name], (label, name, float(g), t[name])


def _fed(M, case, d, cuts_real, cuts_fake, **kwargs):
    """the metric fed in uneven batches, the two sides interleaved"""
    metric = M.PrecisionRecall(feature_size=d, k=case["k"], **kwargs).cuda()
    real, fake = case["real"].cuda(), case["fake"].cuda()
    for (rl, rh), (fl, fh) in zip(cuts_real, cuts_fake):
        metric.update(generated=fake[fl:fh] if fh != fl else None, samples=real[rl:rh] if rh != rl else None)
    return metric


def _cuts(n):
    a, b = n // 3, n // 3 + 1
    return [(0, a), (a, b), (b, n)]


# ---------------------------------------------------------------------------------------------------------------- 1. exact inputs
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_dyadic_features_match_the_integer_truth_exactly(M, shape):
    n, m, d, k = shape
    case = C.dyadic(*shape)
    t = case["truth"]
    got = _ops(case["real"], case["fake"], k)
    print(f"[prdc dyadic {shape}] " + " ".join(f"{name} {t[name]:.4f}" for name in NAMES) + f" ties {case['ties']}")
    for key in ("r_real", "r_fake", "min_real"):
        assert torch.equal(got[key], t[key]), (shape, key, (got[key] - t[key]).abs().max())
    _assert_counts(got, t, shape)
    _assert_values(M.precision_recall_density_coverage(case["real"].cuda(), case["fake"].cuda(), k=k), t, shape)
    # knn_radii is the square root of the exact r2, taken on the device: HIP documents its fp64 sqrt to 1 ulp
    radii, want = M.knn_radii(case["real"].cuda(), k).cpu(), t["r_real"].sqrt()
    assert radii.dtype == torch.float64 and bool(((radii - want).abs() <= 2.0 ** -52 * want).all())
    # the metric, fed in uneven batches through otvae::feature_append
    metric = _fed(M, case, d, _cuts(n), _cuts(m), max_observations=max(n, m) + 3)
    assert metric.num_real.tolist() == [n, n] and metric.num_fake.tolist() == [m, m]
    _assert_values(metric.compute(), t, shape)


@pytest.mark.parametrize("which", ["ties", "duplicates"])
def test_lattices_closed_balls_duplicates_zero_radii(M, which):
    case = C.lattice(which)
    t, strict = case["truth"], case["strict"]
    assert case["ties"] > 200 and strict["precision"] < t["precision"] and strict["coverage"] < t["coverage"]   # the inputs decide <=
    got = _ops(case["real"], case["fake"], 3)
    for key in ("r_real", "r_fake", "min_real"):
        assert torch.equal(got[key], t[key]), (which, key)
    _assert_counts(got, t, which)
    _assert_values(M.precision_recall_density_coverage(case["real"].cuda(), case["fake"].cuda(), k=3), t, which)
    if which == "duplicates":
        assert int((got["r_real"] == 0).sum()) > 50                  # self excluded by index: a duplicate is a neighbour at 0


def test_k_equal_one(M):
    n, m, d, _ = (130, 97, 2048, 3)
    case = C.dyadic(n, m, d, 1)
    got = _ops(case["real"], case["fake"], 1)
    for key in ("r_real", "r_fake", "min_real"):
        assert torch.equal(got[key], case["truth"][key])
    _assert_counts(got, case["truth"], "k=1")
    _assert_values(M.precision_recall_density_coverage(case["real"].cuda(), case["fake"].cuda(), k=1), case["truth"], "k=1")


# ---------------------------------------------------------------------------------------------------------------- 2. float features
@pytest.mark.parametrize("shape", C.SHAPES, ids=str)
def test_float_features_equal_counts_and_radii_within_the_bound(M, shape):
    n, m, d, k = shape
    case = C.floating(*shape)
    t = case["truth"]
    print(f"[prdc float {shape}] smallest decision margin / (4 bound) = {case['margin']:.3e}")
    assert case["margin"] > 1.0, "a decision of the truth lies within the error bound: the inputs cannot demand equality"
    got = _ops(case["real"], case["fake"], k)
    for key, e in (("r_real", case["e_r_real"]), ("r_fake", case["e_r_fake"])):
        err = (got[key] - t[key]).abs()
        print(f"[prdc float {shape}] {key}: max err / (2 e) = {float((err / (2 * e)).max()):.3e}")
        assert bool((err <= 2 * e).all()), (shape, key)
    assert bool(((got["min_real"] - t["min_real"]).abs() <= 2 * case["e_min_real"]).all())
    _assert_counts(got, t, shape)
    _assert_values(M.precision_recall_density_coverage(case["real"].cuda(), case["fake"].cuda(), k=k), t, shape)


# ---------------------------------------------------------------------------------------------------------------- 3. structure
@pytest.mark.parametrize("shape", [(33, 33, 70, 3), (130, 97, 2048, 3), (1025, 300, 32, 5)], ids=str)
def test_run_to_run_and_swap_identity(M, shape):
    n, m, d, k = shape
    case = C.floating(*shape)                                        # rounding happens here: identity is not a matter of exactness
    real_g, fake_g = case["real"].cuda(), case["fake"].cuda()
    op_r, op_c = torch.ops.otvae.knn_sq_radii, torch.ops.otvae.manifold_counts
    r2_real, r2_fake = op_r(real_g, k), op_r(fake_g, k)
    assert torch.equal(op_r(real_g, k), r2_real) and torch.equal(op_r(fake_g, k), r2_fake), "two identical calls differ"
    fwd, fwd2 = op_c(real_g, r2_real, fake_g, r2_fake), op_c(real_g, r2_real, fake_g, r2_fake)
    assert all(torch.equal(a, b) for a, b in zip(fwd, fwd2)), "two identical calls differ"
    # sides exchanged: d2(a, b) keeps its bits, so memberships and minima carry over
    swp = op_c(fake_g, r2_fake, real_g, r2_real)
    assert torch.equal(swp[0] > 0, fwd[1] > 0) and torch.equal(swp[1] > 0, fwd[0] > 0)
    assert float(fwd[2].min()) == float(swp[2].min())                # the smallest cross distance, seen from either side
    a = M.precision_recall_density_coverage(real_g, fake_g, k=k)
    b = M.precision_recall_density_coverage(fake_g, real_g, k=k)
    assert torch.equal(a[0], b[1]) and torch.equal(a[1], b[0])       # precision(R, F) is recall(F, R), bit for bit
    assert all(torch.equal(x, y) for x, y in zip(a, M.precision_recall_density_coverage(real_g, fake_g, k=k)))
    if d % 4 == 0:
        # features that do not start on a 16-byte boundary take the 4-byte staging loads: the same products in the same order
        shifted = torch.empty(real_g.numel() + 1, device="cuda")[1:].view_as(real_g).copy_(real_g)
        assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
        assert torch.equal(op_r(shifted, k), r2_real)
        assert all(torch.equal(x, y) for x, y in zip(op_c(shifted, r2_real, fake_g, r2_fake), fwd))
    # float64 features are rounded to float32, as the kernel distance does
    c = M.precision_recall_density_coverage(real_g.double(), fake_g.double(), k=k)
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def test_the_group_rule_is_what_the_shapes_exercise():
    from ot_vae_lightning_amd import _lib
    lib = _lib.load()
    assert lib.otvae_knn_groups(1025) == 9 and -(-1025 // 128) == 9          # several workgroups, one column tile each
    assert lib.otvae_knn_groups(C.WALK_SHAPE[0]) == 12 and -(-C.WALK_SHAPE[0] // 128) == 23   # eleven of them walk two tiles
    assert lib.otvae_knn_groups(C.WALK_SHAPE[0] - 1) == 22                   # one row fewer: one tile each


# ---------------------------------------------------------------------------------------------------------------- 4. metric classes
def test_samples_are_the_real_and_generated_the_fake_manifold(M):
    g = torch.Generator().manual_seed(3)
    data = torch.round(64 * torch.randn(60, 2, generator=g)) / 16    # spread wide
    generated = torch.round(4 * torch.randn(40, 2, generator=g)) / 16   # a tight clump inside the data
    metric = M.PrecisionRecall(feature_size=2, max_observations=64, k=3).cuda()
    metric.update(generated=generated.cuda(), samples=data.cuda())
    assert torch.equal(metric.real_features[:60].cpu(), data) and torch.equal(metric.fake_features[:40].cpu(), generated)
    got = metric.compute()
    want = M.precision_recall_density_coverage(real=data, fake=generated, k=3)      # the host path: exact on these inputs
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want))
    assert float(got[0]) == 1.0 and float(got[1]) < 0.5
    # reset: the counts go to zero where they are; k rows or fewer on a side are refused
    addr = [getattr(metric, n).data_ptr() for n in metric._defaults]
    metric.reset()
    assert metric.num_real.tolist() == [0, 0] and [getattr(metric, n).data_ptr() for n in metric._defaults] == addr
    metric.update(generated=generated[:3].cuda(), samples=data.cuda())
    with pytest.raises(ValueError, match="more than 3 rows"):
        metric.compute()
    metric.update(generated=generated[3:4].cuda())
    assert all(bool(torch.isfinite(v)) for v in metric.compute())


def test_inception_precision_recall_in_a_collection(M):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 8 * 8, 24)).cuda()
    for p in net.parameters():
        p.requires_grad_(False)
    ipr = M.InceptionPrecisionRecall(net=net, feature_size=24, max_observations=128, k=3)
    coll = M.MetricCollection({"psnr": M.PeakSignalNoiseRatio(data_range=1.0), "pr": ipr}).cuda()
    coll.train()
    assert not net.training                                          # the feature network never trains
    g = torch.Generator().manual_seed(8)
    data_feats, gen_feats = [], []
    for size in (30, 1, 33):
        samples = torch.rand(size, 1, 8, 8, generator=g).cuda()
        batch = {"samples": samples, "target": samples, "preds": samples + 0.05 * torch.rand(size, 1, 8, 8, generator=g).cuda(),
                 "generated": torch.rand(size, 1, 8, 8, generator=g).cuda() ** 2, "kwargs": {}}
        assert coll(**batch) == {}                                   # nothing computes on the step
        with torch.no_grad():
            data_feats.append(net(torch.cat([batch["samples"]] * 3, 1)))
            gen_feats.append(net(torch.cat([batch["generated"]] * 3, 1)))
    res = coll.compute()
    assert set(res) == {"psnr", "pr_precision", "pr_recall", "pr_density", "pr_coverage"}
    feature_level = M.PrecisionRecall(feature_size=24, max_observations=128, k=3).cuda()
    feature_level.update(generated=torch.cat(gen_feats), samples=torch.cat(data_feats))
    want = feature_level.compute()
    functional = M.precision_recall_density_coverage(torch.cat(data_feats), torch.cat(gen_feats), k=3)
    for name, w, f in zip(NAMES, want, functional):
        assert torch.equal(res[f"pr_{name}"], w) and torch.equal(w, f)
    assert 0.0 < float(res["pr_recall"]) <= 1.0 and float(res["pr_density"]) > 0.0
    coll.reset()
    assert ipr.num_real.tolist() == [0, 0] and ipr.num_fake.tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def test_ops_refuse_what_lies_outside_the_envelope():
    import ot_vae_lightning_amd  # noqa: F401
    x, y = torch.zeros(8, 4, device="cuda"), torch.zeros(6, 4, device="cuda")
    r8, r6 = torch.zeros(8, device="cuda", dtype=torch.float64), torch.zeros(6, device="cuda", dtype=torch.float64)
    op_r, op_c = torch.ops.otvae.knn_sq_radii, torch.ops.otvae.manifold_counts
    for k in (0, 17, 8, -1):                                         # k outside 1 .. 16, k >= n
        with pytest.raises(ValueError):
            op_r(x, k)
    with pytest.raises(ValueError):
        op_r(torch.zeros(8, 2049, device="cuda"), 3)                 # wider than the tile's 2048
    with pytest.raises(ValueError):
        op_r(x.double(), 3)
    with pytest.raises(ValueError):
        op_r(x.t(), 3)                                               # not contiguous
    with pytest.raises(ValueError):
        op_r(x[0], 3)
    with pytest.raises(ValueError):
        op_c(x, r8, torch.zeros(6, 5, device="cuda"), r6)            # widths differ
    with pytest.raises(ValueError):
        op_c(x, r6, y, r6)                                           # one radius per row
    with pytest.raises(ValueError):
        op_c(x, r8.float(), y, r6)
    with pytest.raises(ValueError):
        op_c(x[:1], r8[:1], y, r6)                                   # a single row has no neighbour
    assert op_r(x, 7).tolist() == [0.0] * 8                          # k = n - 1 on eight copies of one point
    count, hit, low = op_c(x, r8, y, r6)
    assert count.tolist() == [8] * 6 and hit.tolist() == [1] * 8 and low.tolist() == [0.0] * 8
