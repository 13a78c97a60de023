"""CPU: the host side of precision / recall / density / coverage (``ot_vae_lightning_amd/metrics/prdc.py``) -- the fp64 torch path that
host-resident features take against the int64 truth of ``prdc_cases`` (exact: dyadic and lattice inputs), which ``update`` keyword is
which manifold, the ``compute_names`` expansion in a ``MetricCollection``, the store shared with ``KernelDistance``, refusals and the
workspace queries.  No kernel runs here."""
import warnings

import pytest
import torch

import prdc_cases as C

NAMES = ("precision", "recall", "density", "coverage")


@pytest.fixture(scope="module")
def M():
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import metrics
    return metrics


def _prefill(metric, real, fake, seen=None):
    for side, f in (("real", real), ("fake", fake)):
        getattr(metric, f"{side}_features")[:f.shape[0]] = f
        getattr(metric, f"num_{side}").copy_(torch.tensor([f.shape[0], f.shape[0] if seen is None else seen]))


def _assert_values(got, want, label):
    assert len(got) == 4
    for name, g in zip(NAMES, got):
        assert g.dtype == torch.float64 and g.dim() == 0
        assert float(g) == want[name], (label, name, float(g), want[name])


# ---------------------------------------------------------------------------------------------------------------- the host path
@pytest.mark.parametrize("shape", C.SHAPES, ids=str)
def test_host_path_matches_the_integer_truth(M, shape):
    n, m, d, k = shape
    case = C.dyadic(*shape)
    t = case["truth"]
    _assert_values(M.precision_recall_density_coverage(case["real"], case["fake"], k=k), t, shape)
    assert torch.equal(M.knn_radii(case["real"], k), t["r_real"].sqrt()) and torch.equal(M.knn_radii(case["fake"], k), t["r_fake"].sqrt())
    assert 0 < t["recall"] <= 1 and 0 < t["coverage"] <= 1 and t["density"] > 0


@pytest.mark.parametrize("which", ["ties", "duplicates"])
def test_host_path_on_the_lattices_closed_balls_and_self_by_index(M, which):
    case = C.lattice(which)
    t, strict = case["truth"], case["strict"]
    _assert_values(M.precision_recall_density_coverage(case["real"], case["fake"], k=3), t, which)
    assert torch.equal(M.knn_radii(case["real"], 3), t["r_real"].sqrt())
    # the inputs decide the rule: a strict comparison gives other values
    assert case["ties"] > 200 and strict["precision"] < t["precision"] and strict["coverage"] < t["coverage"]
    if which == "ties":
        assert round(t["precision"], 3) == 0.979 and round(t["coverage"], 3) == 0.938
        assert round(strict["precision"], 3) == 0.866 and round(strict["coverage"], 3) == 0.700
    else:
        # 130 rows over 27 points: duplicates are neighbours at distance 0 (self is excluded by index, not by value)
        assert int((t["r_real"] == 0).sum()) > 50


def test_three_point_known_answer(M):
    # real 0, 1, 3 on a line, fake 1.5 and 10, k = 1: radii 1, 1, 2 (squared 1, 1, 4) and 8.5 (squared 72.25) twice
    #   d2(real_i, fake 1.5) = 2.25, 0.25, 2.25 -> inside the balls of real 1 and real 3: count 2;  fake 10 inside none
    #   every real row is within 8.5 of fake 1.5: recall 1;  nearest fake at 2.25, 0.25, 2.25 against 1, 1, 4: coverage 2 / 3
    real, fake = torch.tensor([[0.], [1.], [3.]]), torch.tensor([[1.5], [10.]])
    assert M.knn_radii(real, 1).tolist() == [1.0, 1.0, 2.0] and M.knn_radii(fake, 1).tolist() == [8.5, 8.5]
    p, r, dens, c = M.precision_recall_density_coverage(real, fake, k=1)
    assert (float(p), float(r), float(dens), float(c)) == (0.5, 1.0, 1.0, 2 / 3)


# ---------------------------------------------------------------------------------------------------------------- the metric class
def _asymmetric_pair():
    """data spread wide, the model's samples a tight clump inside it: every generated sample lies in the data manifold (precision 1),
    hardly any data sample lies in the generated one (low recall)"""
    g = torch.Generator().manual_seed(3)
    data = torch.round(64 * torch.randn(60, 2, generator=g)) / 16
    generated = torch.round(4 * torch.randn(40, 2, generator=g)) / 16
    return data, generated


def test_samples_are_the_real_and_generated_the_fake_manifold(M, monkeypatch):
    from ot_vae_lightning_amd.metrics.features import FeatureStore

    def host_append(self, feats, side):                              # `update` has no host path: stand in for otvae::feature_append
        buf, num = getattr(self, f"{side}_features"), getattr(self, f"num_{side}")
        at = int(num[0])
        buf[at:at + feats.shape[0]] = feats
        num += feats.shape[0]

    monkeypatch.setattr(FeatureStore, "_append", host_append)
    data, generated = _asymmetric_pair()
    metric = M.PrecisionRecall(feature_size=2, max_observations=64, k=3)
    metric.update(generated=generated[:25], samples=data[:7])
    metric.update(samples=data[7:])
    metric.update(generated=generated[25:])
    assert torch.equal(metric.real_features[:60], data) and torch.equal(metric.fake_features[:40], generated)
    assert metric.num_real.tolist() == [60, 60] and metric.num_fake.tolist() == [40, 40]
    got = metric.compute()
    want = M.precision_recall_density_coverage(real=data, fake=generated, k=3)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    swapped = M.precision_recall_density_coverage(real=generated, fake=data, k=3)
    assert float(got[0]) == 1.0 and float(got[1]) < 0.5, [float(v) for v in got]
    assert float(swapped[0]) == float(got[1]) and float(swapped[1]) == float(got[0])   # precision(R, F) is recall(F, R)
    assert float(swapped[0]) != float(got[0])
    assert "samples" in M.PrecisionRecall.__doc__ and "generated" in M.PrecisionRecall.__doc__


def test_collection_logs_four_names_and_checkpoints_nothing(M):
    case = C.dyadic(33, 33, 70, 3)
    pr = M.PrecisionRecall(feature_size=70, max_observations=64, k=3)
    coll = M.MetricCollection({"pr": pr}, prefix="val/")
    _prefill(pr, case["real"], case["fake"])
    named = coll.compute()
    assert set(named) == {"val/pr_precision", "val/pr_recall", "val/pr_density", "val/pr_coverage"}
    for name in NAMES:
        assert float(named[f"val/pr_{name}"]) == case["truth"][name]
    assert M.PrecisionRecall.compute_names == NAMES and M.PrecisionRecall.higher_is_better is True
    assert M.InceptionPrecisionRecall.compute_names == NAMES
    assert pr.update_keywords() == ["generated", "samples"]
    assert len(pr.state_dict()) == 0 and len(coll.state_dict()) == 0


def test_reset_and_too_few_rows(M):
    case = C.dyadic(33, 33, 70, 3)
    metric = M.PrecisionRecall(feature_size=70, max_observations=40, k=3)
    with pytest.raises(ValueError, match="more than 3 rows"):
        metric.compute()
    _prefill(metric, case["real"], case["fake"][:3])                 # k rows on one side: one short
    with pytest.raises(ValueError, match="more than 3 rows"):
        metric.compute()
    _prefill(metric, case["real"], case["fake"][:4])
    assert all(bool(torch.isfinite(v)) for v in metric.compute())
    _prefill(metric, case["real"], case["fake"], seen=50)
    with pytest.warns(UserWarning, match="PrecisionRecall keeps the first max_observations = 40"):
        _assert_values(metric.compute(), case["truth"], "prefilled")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        metric.compute()                                             # once only
    addr = metric.num_real.data_ptr(), metric.real_features.data_ptr(), metric.fake_features.data_ptr()
    metric.reset()
    assert metric.num_real.tolist() == [0, 0] and metric.num_fake.tolist() == [0, 0]
    assert (metric.num_real.data_ptr(), metric.real_features.data_ptr(), metric.fake_features.data_ptr()) == addr
    with pytest.raises(ValueError):
        metric.compute()
    metric.sync()                                                    # no process group: nothing happens
    assert metric.real_features.shape == (40, 70)


def test_kernel_distance_still_sits_on_the_shared_store(M):
    from ot_vae_lightning_amd.metrics.features import FeatureStore
    assert issubclass(M.KernelDistance, FeatureStore) and issubclass(M.PrecisionRecall, FeatureStore)
    assert issubclass(M.KernelInceptionDistance, M.KernelDistance) and issubclass(M.InceptionPrecisionRecall, M.PrecisionRecall)
    kid = M.KernelDistance(feature_size=4, max_observations=16, subsets=2, subset_size=4)
    pr = M.PrecisionRecall(feature_size=4, max_observations=16, k=2)
    for metric in (kid, pr):
        assert list(metric._defaults) == ["real_features", "num_real", "fake_features", "num_fake"]
        assert metric.real_features.shape == (16, 4) and metric.real_features.dtype == torch.float32
        assert metric.num_fake.shape == (2,) and metric.num_fake.dtype == torch.int64
    for name in ("reset", "_append", "sync"):
        assert getattr(M.KernelDistance, name) is getattr(FeatureStore, name) is getattr(M.PrecisionRecall, name)


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kwargs", [dict(k=0), dict(k=17), dict(k=2.0), dict(k=True), dict(feature_size=0), dict(feature_size=2049),
                                    dict(max_observations=5, k=5), dict(max_observations=7.5)],
                         ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_constructor_refusals(M, kwargs):
    base = dict(feature_size=8, max_observations=16, k=3)
    base.update(kwargs)
    with pytest.raises(ValueError):
        M.PrecisionRecall(**base)
    with pytest.raises(ValueError):
        M.InceptionPrecisionRecall(net=torch.nn.Flatten(), **base)


def test_functional_refusals(M):
    x, y = torch.zeros(6, 4), torch.zeros(5, 4)
    for k in (0, 17, 2.5):
        with pytest.raises(ValueError, match="`k`"):
            M.precision_recall_density_coverage(x, y, k=k)
    with pytest.raises(ValueError):
        M.precision_recall_density_coverage(x, y, k=5)               # the smaller side holds k rows
    with pytest.raises(ValueError):
        M.precision_recall_density_coverage(x, torch.zeros(5, 3), k=2)
    with pytest.raises(ValueError):
        M.precision_recall_density_coverage(x, torch.zeros(5), k=2)
    with pytest.raises(ValueError):
        M.precision_recall_density_coverage(torch.zeros(6, 2049), torch.zeros(6, 2049), k=2)
    with pytest.raises(ValueError):
        M.knn_radii(x, k=6)
    assert M.knn_radii(x, k=5).tolist() == [0.0] * 6                 # duplicates: neighbours at distance 0


def test_ops_refuse_cpu_tensors(M):
    x = torch.zeros(8, 4)
    with pytest.raises(RuntimeError):
        torch.ops.otvae.knn_sq_radii(x, 3)
    with pytest.raises(RuntimeError):
        torch.ops.otvae.manifold_counts(x, torch.zeros(8, dtype=torch.float64), x, torch.zeros(8, dtype=torch.float64))
    metric = M.PrecisionRecall(feature_size=4, max_observations=16, k=3)
    with pytest.raises(RuntimeError):
        metric.update(x, x)


# ---------------------------------------------------------------------------------------------------------------- workspace queries
@pytest.mark.parametrize("args", [(10, 64, 0), (10, 64, 17), (5, 64, 5), (0, 64, 1), (10, 0, 3), (10, 2049, 3), ((1 << 21) + 1, 64, 3)])
def test_radii_workspace_refuses_bad_arguments(args):
    from ot_vae_lightning_amd import _lib
    assert _lib.load().otvae_knn_sq_radii_ws(*args) == -1


def test_workspace_sizes_and_the_group_rule():
    from ot_vae_lightning_amd import _lib
    lib = _lib.load()
    def rule(n):                                                     # the header's: rounds of 512 resident workgroups x tiles each
        nt = -(-n // 128)
        cap = max(1, min(nt, (1 << 25) // n))
        return min(range(1, cap + 1), key=lambda g: (-(-nt * g // 512) * -(-nt // g), g))

    for n, groups in ((4, 1), (128, 1), (257, 3), (1025, 9), (2816, 22), (2817, 12), (2945, 12), (10000, 79), (1 << 21, 1)):
        assert groups == rule(n)
        assert lib.otvae_knn_groups(n) == groups
        assert lib.otvae_knn_sq_radii_ws(n, 96, 3) == 8 * (n + groups * n * 3)
    assert lib.otvae_knn_groups(0) == -1
    for n, m in ((2, 2), (130, 97), (1025, 300)):
        ntn, ntm = -(-n // 128), -(-m // 128)
        assert lib.otvae_manifold_counts_ws(n, m, 2048) == 8 * (n + m + ntm * n) + 4 * (ntn * m + ntm * n)
    for args in ((1, 5, 8), (5, 1, 8), (5, 5, 0), (5, 5, 2049), ((1 << 21) + 1, 5, 8)):
        assert lib.otvae_manifold_counts_ws(*args) == -1
