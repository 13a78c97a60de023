"""CPU: the Kernel Inception Distance's host side (``ot_vae_lightning_amd/metrics/kid.py``) -- argument refusals, the envelope of
``otvae_poly_mmd_ws``, the fp64 torch path that host-resident states take, the ``compute_names`` expansion of ``MetricCollection``
and ``KernelDistance.sync`` over a world-2 gloo group.  No kernel runs here."""
import os
import socket
import sys
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import metrics
    return metrics


def _truth_mmd2(x, y, degree, gamma, coef):
    """the estimator of the issue, term by term in float64"""
    x, y = x.double(), y.double()
    m = x.shape[0]
    k = lambda a, b: (gamma * (a @ b.T) + coef) ** degree  # noqa: E731
    off = lambda g: g.sum() - g.diagonal().sum()  # noqa: E731
    return (off(k(x, x)) + off(k(y, y))) / (m * (m - 1)) - 2 * k(x, y).sum() / m ** 2


def _prefill(metric, real, fake, seen=None):
    for side, f in (("real", real), ("fake", fake)):
        getattr(metric, f"{side}_features")[:f.shape[0]] = f
        getattr(metric, f"num_{side}").copy_(torch.tensor([f.shape[0], f.shape[0] if seen is None else seen]))


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kwargs", [dict(subset_size=1), dict(subset_size=0), dict(degree=0), dict(degree=9), dict(degree=2.5),
                                    dict(feature_size=0), dict(feature_size=2049), dict(max_observations=999, subset_size=1000),
                                    dict(subsets=0), dict(subsets=65536), dict(gamma=0.0), dict(gamma=-1.0)],
                         ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
def test_constructor_refusals(M, kwargs):
    base = dict(feature_size=8, max_observations=16, subsets=2, subset_size=4)
    base.update(kwargs)
    with pytest.raises(ValueError):
        M.KernelDistance(**base)
    with pytest.raises(ValueError):
        M.KernelInceptionDistance(net=torch.nn.Flatten(), **base)


def test_functional_refusals(M):
    x, y = torch.zeros(6, 4), torch.zeros(5, 4)
    with pytest.raises(ValueError, match="subset_size"):
        M.kernel_distance(x, y, subsets=2, subset_size=6)           # more than the smaller side holds
    with pytest.raises(ValueError):
        M.kernel_distance(x, y, subsets=2, subset_size=1)
    with pytest.raises(ValueError):
        M.kernel_distance(x, y, subsets=2, subset_size=3, degree=9)
    with pytest.raises(ValueError):
        M.kernel_distance(x, torch.zeros(5, 3), subsets=2, subset_size=3)
    with pytest.raises(ValueError):
        M.poly_mmd2(x, y)                                            # unequal sizes
    with pytest.raises(ValueError):
        M.poly_mmd2(torch.zeros(4, 2049), torch.zeros(4, 2049))
    with pytest.raises(ValueError):
        M.poly_mmd2(x[:1], y[:1])


@pytest.mark.parametrize("args", [(0, 100, 64), (70000, 100, 64), (1, 1, 64), (1, 0, 64), (1, 100, 0), (1, 100, 2049), (-1, 100, 64),
                                  (1, 1 << 22, 64)])
def test_workspace_size_refuses_bad_arguments(args):
    from ot_vae_lightning_amd import _lib
    assert _lib.load().otvae_poly_mmd_ws(*args) == -1


def test_workspace_size_is_one_double_per_tile_and_subset():
    from ot_vae_lightning_amd import _lib
    lib = _lib.load()
    for s, m in ((1, 2), (5, 128), (5, 129), (100, 1000)):
        nt = -(-m // 128)
        assert lib.otvae_poly_mmd_ws(s, m, 2048) == s * (nt * (nt + 1) + nt * nt) * 8


def test_ops_refuse_cpu_tensors(M):
    x = torch.zeros(8, 4)
    with pytest.raises(RuntimeError):
        torch.ops.otvae.poly_mmd_subsets(x, x, None, None, 4, 3, 0.25, 1.0)
    with pytest.raises(RuntimeError):
        torch.ops.otvae.feature_append(x, torch.zeros(16, 4), torch.zeros(2, dtype=torch.int64))
    metric = M.KernelDistance(feature_size=4, max_observations=16, subsets=2, subset_size=4)
    with pytest.raises(RuntimeError):
        metric.update(x, x)                                          # `update` has no host path, like FrechetDistance's


# ---------------------------------------------------------------------------------------------------------------- the host path
def test_three_sample_known_answer(M):
    # x = (1,0), (0,1), (1,1);  y = (0,0), (1,0), (0,2);  k(a, b) = (<a, b> + 1)^2
    #   <x_i, x_j>, i < j: 0, 1, 1         -> k = 1, 4, 4    -> sum over i != j = 2 * 9  = 18
    #   <y_i, y_j>, i < j: 0, 0, 0         -> k = 1, 1, 1    -> sum over i != j = 2 * 3  = 6
    #   <x_i, y_j>: 0 1 0 / 0 0 2 / 0 1 2  -> k = 1 4 1 / 1 1 9 / 1 4 9              -> sum = 31
    #   MMD^2 = (18 + 6) / (3 * 2) - 2 * 31 / 9 = 4 - 62 / 9 = -26 / 9
    x = torch.tensor([[1., 0.], [0., 1.], [1., 1.]])
    y = torch.tensor([[0., 0.], [1., 0.], [0., 2.]])
    want = -26.0 / 9.0
    got = M.poly_mmd2(x, y, degree=2, gamma=1.0, coef=1.0)
    assert got.dtype == torch.float64 and got.dim() == 0
    assert abs(float(got) - want) <= 4 * 2.0 ** -52 * abs(want)
    metric = M.KernelDistance(feature_size=2, max_observations=3, subsets=4, subset_size=3, degree=2, gamma=1.0, coef=1.0, seed=0)
    _prefill(metric, x, y)
    mean, std = metric.compute()                                     # every subset is a permutation of all three rows
    assert abs(float(mean) - want) <= 4 * 2.0 ** -52 * abs(want) and float(std) <= 4 * 2.0 ** -52 * abs(want)
    assert mean.dtype == torch.float64 and mean.dim() == 0 and std.dim() == 0


@pytest.mark.parametrize("degree,gamma,coef", [(3, None, 1.0), (2, 0.37, 0.0), (1, None, 1.0)])
def test_host_compute_matches_the_formulas(M, degree, gamma, coef):
    g = torch.Generator().manual_seed(5)
    real, fake = 3 + torch.randn(40, 17, generator=g), 3 + 1.1 * torch.randn(31, 17, generator=g)
    metric = M.KernelDistance(feature_size=17, max_observations=64, subsets=6, subset_size=12, degree=degree, gamma=gamma, coef=coef, seed=3)
    _prefill(metric, real, fake)
    mean, std = metric.compute()
    idx_real, idx_fake, per = metric.last_subsets
    assert idx_real.shape == idx_fake.shape == (6, 12) and idx_real.dtype == torch.int32
    for rows, n in ((idx_real, 40), (idx_fake, 31)):
        assert int(rows.min()) >= 0 and int(rows.max()) < n
        assert all(len(set(r.tolist())) == 12 for r in rows)
    gm = 1.0 / 17 if gamma is None else gamma
    want = torch.stack([_truth_mmd2(real[i.long()], fake[j.long()], degree, gm, coef) for i, j in zip(idx_real, idx_fake)])
    assert torch.allclose(per, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(mean, want.mean(), rtol=1e-12, atol=1e-14) and torch.allclose(std, want.std(unbiased=False), rtol=1e-10, atol=1e-14)
    # the functional form on the same features: the same estimator (its own indices)
    fm, fs, fper, fi, fj = M.kernel_distance(real, fake, subsets=6, subset_size=12, degree=degree, gamma=gamma, coef=coef, seed=3,
                                             return_subsets=True)
    fwant = torch.stack([_truth_mmd2(real[i.long()], fake[j.long()], degree, gm, coef) for i, j in zip(fi, fj)])
    assert torch.allclose(fper, fwant, rtol=1e-12, atol=1e-12) and torch.allclose(fm, fwant.mean(), rtol=1e-12, atol=1e-14)
    # same seed, same call number: the same indices; the next call draws others
    twin = M.KernelDistance(feature_size=17, max_observations=64, subsets=6, subset_size=12, degree=degree, gamma=gamma, coef=coef, seed=3)
    _prefill(twin, real, fake)
    twin.compute()
    assert torch.equal(twin.last_subsets[0], idx_real) and torch.equal(twin.last_subsets[1], idx_fake)
    twin.compute()
    assert not torch.equal(twin.last_subsets[0], idx_real)


def test_compute_refuses_too_few_rows_and_warns_about_dropped_ones(M):
    metric = M.KernelDistance(feature_size=4, max_observations=16, subsets=2, subset_size=8)
    g = torch.Generator().manual_seed(1)
    _prefill(metric, torch.randn(8, 4, generator=g), torch.randn(7, 4, generator=g))
    with pytest.raises(ValueError, match="Argument `subset_size` should be smaller than the number of samples"):
        metric.compute()
    _prefill(metric, torch.randn(16, 4, generator=g), torch.randn(16, 4, generator=g), seen=20)
    with pytest.warns(UserWarning, match="dropped"):
        metric.compute()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        metric.compute()                                             # once only
    addr = metric.num_real.data_ptr(), metric.real_features.data_ptr()
    metric.reset()
    assert metric.num_real.tolist() == [0, 0] and metric.num_fake.tolist() == [0, 0]
    assert (metric.num_real.data_ptr(), metric.real_features.data_ptr()) == addr
    assert "real_features" not in metric.state_dict() and "num_real" not in metric.state_dict()


# ---------------------------------------------------------------------------------------------------------------- MetricCollection
def test_compute_names_expand_in_a_collection(M):
    class Const(M.Metric):
        def __init__(self, value):
            super().__init__(compute_on_step=True)
            self.value = value

        def update(self, preds=None):
            pass

        def compute(self):
            return self.value

    class Pair(Const):
        compute_names = ("mean", "std")

    plain_value = (torch.tensor(1.0), torch.tensor(2.0))             # a tuple from a metric WITHOUT the attribute stays a tuple
    coll = M.MetricCollection({"a": Const(plain_value), "kid": Pair((torch.tensor(3.0), torch.tensor(4.0)))}, prefix="val/")
    for res in (coll.compute(), coll(preds=torch.zeros(1))):
        assert set(res) == {"val/a", "val/kid_mean", "val/kid_std"}
        assert res["val/a"] is plain_value
        assert float(res["val/kid_mean"]) == 3.0 and float(res["val/kid_std"]) == 4.0
    assert M.Metric.compute_names is None and M.PeakSignalNoiseRatio.compute_names is None
    assert M.KernelDistance.compute_names == ("mean", "std")
    bad = M.MetricCollection({"kid": Pair((torch.tensor(3.0),))})
    with pytest.raises(ValueError):
        bad.compute()


# ---------------------------------------------------------------------------------------------------------------- data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_features(rank):
    g = torch.Generator().manual_seed(40 + rank)
    return torch.randn(9 + 3 * rank, 6, generator=g), 0.5 + torch.randn(7 + 5 * rank, 6, generator=g)


def _worker(rank, world, port, q):
    try:
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from ot_vae_lightning_amd import metrics as M
        metric = M.KernelDistance(feature_size=6, max_observations=16, subsets=3, subset_size=8, seed=11)
        real, fake = _rank_features(rank)
        _prefill(metric, real, fake, seen=20 if rank == 1 else None)
        metric.sync()
        parts = [_rank_features(r) for r in range(world)]
        all_real, all_fake = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
        assert metric.real_features.shape == (world * 16, 6) and metric.fake_features.shape == (world * 16, 6)
        assert metric.num_real.tolist() == [all_real.shape[0], parts[0][0].shape[0] + 20]
        assert metric.num_fake.tolist() == [all_fake.shape[0], parts[0][1].shape[0] + 20]
        assert torch.equal(metric.real_features[:all_real.shape[0]], all_real)        # rank 0's rows first
        assert torch.equal(metric.fake_features[:all_fake.shape[0]], all_fake)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mean, std = metric.compute()
        idx_real, idx_fake, per = metric.last_subsets
        want = torch.stack([_truth_mmd2(all_real[i.long()], all_fake[j.long()], 3, 1.0 / 6, 1.0) for i, j in zip(idx_real, idx_fake)])
        assert torch.allclose(per, want, rtol=1e-12, atol=1e-12)
        got = [torch.empty(2, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(got, torch.stack([mean, std]))
        assert torch.equal(got[0], got[1]), "the ranks computed different values"
        metric.reset()
        assert metric.real_features.shape == (16, 6) and metric.num_real.tolist() == [0, 0]
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_sync_gathers_the_union_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, msg in res:
        assert msg == "ok", f"rank {rank}:\n{msg}"


def test_sync_without_a_process_group_is_a_no_op(M):
    metric = M.KernelDistance(feature_size=4, max_observations=8, subsets=2, subset_size=4)
    addr = metric.real_features.data_ptr()
    metric.sync()
    assert metric.real_features.data_ptr() == addr and metric.real_features.shape == (8, 4)
