"""GPU: ``otvae::sliced_w2`` / ``SlicedWassersteinPrior`` against the definition evaluated in float64 on the CPU (run with ``-m gpu``).

    theta_l = g_l / |g_l|,  p = z theta^T,  q = y theta^T,  both sorted per column with a STABLE sort (ties: the smaller row first)
    SW = 1 / (L N) sum_l sum_k (p_l,(k) - q_l,(k))^2,   r[l, i] = p_l,i - q_l,(rank_l(i)),   d SW / d z = 2 / (L N) r^T theta

Inputs: z = 1.3 randn + 0.2, y = randn, dirs = randn from one seeded CPU generator (in this order).  Bounds: 1e-4 relative for the loss,
the residuals and the gradient (the project's fp32 contract), 1e-5 for the backward product against float64 on the kernel's own operands.

fp32 cannot rank two projections that lie within 1e-5 of each other in float64, and a swapped rank pairs the row with another q: residual
entries whose projection has another VALUE within 1e-5 in its column are left out of the entry-wise comparison (never more than 3 % of a
case; the count is printed).  With seed 0 the float64 reference leaves out 0 entries below N = 1000, 0.38 % at (1000, 16, 33), 0.45 % at
(1024, 128, 64) and 1.66 % at (4096, 8, 4)."""
import functools

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 1), (2, 4, 1), (7, 5, 3), (64, 16, 8), (1000, 16, 33), (1024, 128, 64), (4096, 8, 4)]
TIE_EPS = 1e-5


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd as pkg
    return pkg


def _inputs(n, d, nl, seed=0, duplicate_rows=False):
    gen = torch.Generator().manual_seed(seed)
    z = 1.3 * torch.randn(n, d, generator=gen) + 0.2
    y = torch.randn(n, d, generator=gen)
    g = torch.randn(nl, d, generator=gen)
    if duplicate_rows:
        z[1::2] = z[0:n - 1:2]      # rows 2k and 2k + 1 are the same vector: every projection has exact ties
    return z, y, g


def _truth(z, y, g, scale=1.0):
    """the definition in float64: loss (scalar), r [L, N], theta [L, D], d loss / d z [N, D], near [L, N] (entries fp32 cannot rank)"""
    z, y, g = z.double(), y.double(), g.double()
    theta = g / g.norm(dim=1, keepdim=True)
    p, q = z @ theta.T, y @ theta.T                                     # [N, L]
    ps, order = torch.sort(p, dim=0, stable=True)
    qs, _ = torch.sort(q, dim=0, stable=True)
    n, nl = p.shape
    loss = scale * ((ps - qs) ** 2).sum() / (nl * n)
    r = torch.empty_like(p).scatter_(0, order, ps - qs)                 # back to the original row order
    grad = (2.0 * scale / (nl * n)) * (r @ theta)
    # another VALUE of the same column within TIE_EPS: count of the window minus the count of exact copies
    pst = ps.T.contiguous()
    pt = p.T.contiguous()
    window = torch.searchsorted(pst, pt + TIE_EPS, right=True) - torch.searchsorted(pst, pt - TIE_EPS, right=False)
    copies = torch.searchsorted(pst, pt, right=True) - torch.searchsorted(pst, pt, right=False)
    near = window > copies                                              # [L, N]
    gaps = (ps[1:] - ps[:-1])
    min_gap = float(gaps[gaps > 0].min()) if n > 1 and bool((gaps > 0).any()) else float("inf")
    return {"loss": loss, "r": r.T.contiguous(), "theta": theta, "grad": grad, "near": near, "min_gap": min_gap}


@functools.lru_cache(maxsize=None)
def _case(n, d, nl, seed=0, duplicate_rows=False):
    """inputs and float64 truth of a case, computed once and shared (callers do not modify them)"""
    z, y, g = _inputs(n, d, nl, seed, duplicate_rows)
    return z, y, g, _truth(z, y, g)


@functools.lru_cache(maxsize=None)
def _device_run(n, d, nl, seed=0, duplicate_rows=False):
    z, y, g, _ = _case(n, d, nl, seed, duplicate_rows)
    zc, yc, gc = z.cuda(), y.cuda(), g.cuda()
    loss, resid, theta = torch.ops.otvae.sliced_w2(zc, yc, gc, 1.0)
    torch.cuda.synchronize()
    return zc, yc, gc, loss, resid, theta


@pytest.mark.parametrize("n,d,nl", SHAPES)
def test_loss_matches_float64_and_is_replicated_and_reproducible(A, n, d, nl):
    _, _, _, t = _case(n, d, nl)
    zc, yc, gc, loss, resid, theta = _device_run(n, d, nl)
    assert loss.shape == (n,) and resid.shape == (nl, n) and theta.shape == (nl, d)
    err = abs(float(loss[0]) - float(t["loss"])) / float(t["loss"])
    print(f"sliced_w2 loss N={n} D={d} L={nl}: {float(loss[0]):.8g} vs {float(t['loss']):.8g}, rel {err:.2e}")
    assert err <= 1e-4
    assert bool((loss == loss[0]).all()), "the loss entries differ"
    assert rel_err(theta, t["theta"]) <= 1e-6
    loss2, resid2, theta2 = torch.ops.otvae.sliced_w2(zc, yc, gc, 1.0)
    assert torch.equal(loss, loss2) and torch.equal(resid, resid2) and torch.equal(theta, theta2), "two runs differ in their bits"
    # the scale enters the loss and nothing else
    loss3, resid3, _ = torch.ops.otvae.sliced_w2(zc, yc, gc, 0.25)
    assert rel_err(loss3, 0.25 * loss) <= 1e-6 and torch.equal(resid3, resid)
    # the functional form is the same number
    assert float(A.sliced_w2(zc, yc, projections=gc)) == float(loss[0])


@pytest.mark.parametrize("n,d,nl", SHAPES)
def test_residuals_match_float64_in_original_row_order(A, n, d, nl):
    _, _, _, t = _case(n, d, nl)
    resid = _device_run(n, d, nl)[4].cpu().double()
    near = t["near"]
    share = float(near.double().mean())
    keep = ~near
    scale = float(t["r"].abs().max())
    err = float((resid - t["r"])[keep].abs().max()) / scale if bool(keep.any()) else 0.0
    print(f"sliced_w2 resid N={n} D={d} L={nl}: {int(near.sum())} of {near.numel()} entries left out ({100 * share:.2f} %), "
          f"rel {err:.2e}, smallest float64 gap {t['min_gap']:.2e}")
    assert share <= 0.03
    assert err <= 1e-4


@pytest.mark.parametrize("n,d,nl", SHAPES)
def test_backward_product_matches_float64_on_the_kernels_own_operands(A, n, d, nl):
    """separates the GEMM from the sort: gz against float64 on the residuals and directions the forward kernel itself left"""
    zc, _, _, _, resid, theta = _device_run(n, d, nl)
    gen = torch.Generator().manual_seed(5)
    gout = (torch.randint(-3, 4, (n,), generator=gen).float() / 8).cuda()          # dyadic: its sum is exact in any order
    if float(gout.sum()) == 0.0:
        gout[0] += 0.5
    gadd = torch.randn(n, d, generator=gen).cuda()
    scale = 0.7
    gz = torch.ops.otvae.sliced_w2_backward(gout, None, resid, theta, scale)
    want = (float(gout.double().sum()) * scale * 2.0 / (nl * n)) * (resid.double().T @ theta.double())
    err = rel_err(gz, want)
    print(f"sliced_w2 backward N={n} D={d} L={nl}: rel {err:.2e}")
    assert gz.shape == (n, d) and err <= 1e-5
    # gadd is added exactly: one fp32 addition to the very same product
    gz_add = torch.ops.otvae.sliced_w2_backward(gout, gadd, resid, theta, scale)
    assert torch.equal(gz_add, gadd + gz)
    # gout enters as its sum
    lumped = torch.zeros_like(gout)
    lumped[n - 1] = gout.sum()
    assert torch.equal(torch.ops.otvae.sliced_w2_backward(lumped, None, resid, theta, scale), gz)
    assert torch.equal(torch.ops.otvae.sliced_w2_backward(2 * gout, None, resid, theta, scale), 2 * gz)


@pytest.mark.parametrize("n,d,nl,seed", [(7, 5, 3, 0), (64, 16, 8, 1)])
def test_gradient_through_the_prior_matches_float64(A, n, d, nl, seed):
    """no near-ties: the smallest float64 gap between two projections of a column is 6.8e-3 at (7, 5, 3) with seed 0 and 4.4e-4 at
    (64, 16, 8) with seed 1 (1.4e-5 with seed 0), far above what fp32 resolves, so the matching is the reference's and the whole
    gradient can be compared"""
    z, y, g, t = _case(n, d, nl, seed=seed)
    print(f"sliced_w2 gradient N={n} D={d} L={nl}: smallest float64 gap {t['min_gap']:.2e}")
    assert t["min_gap"] > 1e-4 and not bool(t["near"].any())
    coeff = 0.5
    prior = A.SlicedWassersteinPrior(n_projections=nl, loss_coeff=coeff).cuda()
    zc = z.cuda().requires_grad_(True)
    z_out, loss, art = prior(zc, step=0, prior_samples=y.cuda(), projections=g.cuda())
    assert z_out.shape == zc.shape and z_out.data_ptr() == zc.data_ptr() and set(art) == {"prior_samples", "projections"}
    assert abs(float(loss.detach().mean()) - coeff * float(t["loss"])) <= 1e-4 * coeff * float(t["loss"])
    loss.mean().backward()
    err = rel_err(zc.grad, coeff * t["grad"])
    print(f"    d loss / d z: rel {err:.2e}")
    assert err <= 1e-4
    # a decoder's share arrives through the aliased latents and is added inside the backward kernel
    own = zc.grad.clone()
    zc.grad = None
    z_out, loss, _ = prior(zc, step=0, prior_samples=y.cuda(), projections=g.cuda())
    w = torch.linspace(-1, 1, n * d, device="cuda").reshape(n, d)
    (loss.mean() + (z_out * w).sum()).backward()
    assert torch.equal(zc.grad, w + own)
    # the functional form, no decoder
    z2 = z.cuda().requires_grad_(True)
    A.sliced_w2(z2, y.cuda(), projections=g.cuda()).backward()
    assert rel_err(z2.grad, t["grad"]) <= 1e-4


@pytest.mark.parametrize("n,d,nl", [(64, 16, 8), (1000, 16, 33)])
def test_exact_ties_fall_to_the_smaller_row(A, n, d, nl):
    _, _, _, t = _case(n, d, nl, seed=2, duplicate_rows=True)
    _, _, _, loss, resid, _ = _device_run(n, d, nl, seed=2, duplicate_rows=True)
    err = abs(float(loss[0]) - float(t["loss"])) / float(t["loss"])
    assert err <= 1e-4 and bool((loss == loss[0]).all())
    resid = resid.cpu().double()
    near = t["near"]
    share = float(near.double().mean())
    print(f"sliced_w2 ties N={n} D={d} L={nl}: loss rel {err:.2e}, {int(near.sum())} entries left out ({100 * share:.2f} %)")
    assert share <= 0.03
    scale = float(t["r"].abs().max())
    for l in range(nl):   # the multiset of every residual column
        keep = ~near[l]
        got, want = resid[l][keep].sort().values, t["r"][l][keep].sort().values
        assert float((got - want).abs().max()) <= 1e-4 * scale, l


def test_a_nan_latent_poisons_the_loss(A):
    z, y, g, _ = _case(64, 16, 8)
    zc = z.clone()
    zc[17, 3] = float("nan")
    loss, resid, theta = torch.ops.otvae.sliced_w2(zc.cuda(), y.cuda(), g.cuda(), 1.0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and bool(torch.isfinite(theta).all())
    zi = z.clone()
    zi[5, 0] = float("inf")
    assert bool(torch.isnan(torch.ops.otvae.sliced_w2(zi.cuda(), y.cuda(), g.cuda(), 1.0)[0]).all())


def test_opcheck(A):
    z, y, g, _ = _case(64, 16, 8)
    zc, yc, gc, loss, resid, theta = _device_run(64, 16, 8)
    torch.library.opcheck(torch.ops.otvae.sliced_w2.default, (zc.clone().requires_grad_(True), yc, gc, 0.5))
    torch.library.opcheck(torch.ops.otvae.sliced_w2_backward.default, (torch.full((64,), 1.0 / 64, device="cuda"), None, resid, theta, 0.5))
    torch.library.opcheck(torch.ops.otvae.sliced_w2_backward.default,
                          (torch.full((64,), 1.0 / 64, device="cuda"), torch.ones(64, 16, device="cuda"), resid, theta, 0.5))


def test_more_rows_than_one_workgroup_sorts_are_refused(A):
    z = torch.zeros(4097, 4, device="cuda")
    with pytest.raises(NotImplementedError, match="4096"):
        torch.ops.otvae.sliced_w2(z, z, torch.ones(2, 4, device="cuda"), 1.0)
    with pytest.raises(NotImplementedError):
        A.SlicedWassersteinPrior(2).cuda()(z, step=0)


def _small_vae(A, nl=16, seed=41):
    torch.manual_seed(seed)
    enc = A.CNN(1, 16, 16, 1, capacity=4, down_sample=True, residual="add")
    dec = A.CNN(16, 1, 1, 16, capacity=4, up_sample=True, residual="add")
    return A.VAE(encoder=enc, decoder=dec, prior=A.SlicedWassersteinPrior(n_projections=nl, loss_coeff=0.5, seed=7)).cuda().train()


def test_small_vae_trains_eagerly_and_captured(A):
    from detfill import normal
    B, nl = 64, 16
    xs = [normal((B, 1, 16, 16), 300 + i).cuda() for i in range(3)]
    ps, g = normal((B, 16), 310).cuda(), normal((nl, 16), 311).cuda()

    # the same draws handed in: the eager step and the captured one agree
    out = {}
    for graph in (False, True):
        tr = A.HipTrainer(_small_vae(A, nl), batch_shape=(B, 1, 16, 16), use_graph=graph, batch_kwargs={"prior_samples": ps, "projections": g})
        out[graph] = torch.stack([tr.step(x).clone() for x in xs])
        torch.cuda.synchronize()
        assert tr.skipped_steps == 0
        tr.close()
    print("sliced_w2 VAE [total, recon, prior] eager:\n", out[False].cpu(), "\ncaptured:\n", out[True].cpu())
    assert bool(torch.isfinite(out[False]).all()) and bool(torch.isfinite(out[True]).all())
    assert bool((out[False][:, 2] > 0).all())
    assert rel_err(out[True], out[False]) <= 1e-5

    # its own draws: fresh on every replay of the captured step (lr = 0 and one batch: only the draws change)
    tr = A.HipTrainer(_small_vae(A, nl), batch_shape=(B, 1, 16, 16), use_graph=True, lr=0.0)
    losses = torch.stack([tr.step(xs[0]).clone() for _ in range(3)])
    torch.cuda.synchronize()
    tr.close()
    assert bool(torch.isfinite(losses).all())
    assert losses[0, 1] == losses[1, 1] == losses[2, 1], "the reconstruction term moved at lr = 0"
    assert len({float(v) for v in losses[:, 2]}) == 3, f"the prior term did not change between replays: {losses[:, 2]}"


def test_enable_graphed_step_runs_the_prior(A):
    from detfill import normal
    B = 64
    model = _small_vae(A).enable_graphed_step()
    opt = torch.optim.Adam(model.optim_parameters(), lr=1e-3)
    model.batch_preprocess = lambda b: {"samples": b, "target": b, "kwargs": {}}
    seen = []
    for i in range(3):
        opt.zero_grad()
        out = model.training_step(normal((B, 1, 16, 16), 320 + i).cuda(), i)
        out["loss"].backward()
        opt.step()
        seen.append(float(out["train/loss/prior"].detach()))
    assert all(v == v and v > 0 for v in seen), seen


def test_prior_step_launches_no_aten_kernels(A):
    """prior forward + backward under the profiler: only this library's kernels (no library GEMM, no library sort, no ATen fill / copy)"""
    from torch.profiler import ProfilerActivity, profile
    z, y, g, _ = _case(1024, 128, 64)
    zc, yc, gc = z.cuda().requires_grad_(True), y.cuda(), g.cuda()
    prior = A.SlicedWassersteinPrior(n_projections=64, loss_coeff=0.5).cuda()
    gl = torch.full((1024,), 1.0 / 1024, device="cuda")

    def run():
        zc.grad = None
        _, loss, _ = prior(zc, step=0, prior_samples=yc, projections=gc)
        torch.autograd.backward(loss, grad_tensors=[gl], inputs=[zc])

    run()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        run()
        torch.cuda.synchronize()
    names = sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})
    assert names, "the profiler saw no device kernels"
    foreign = [n for n in names if "sliced_w2" not in n]
    assert not foreign, foreign
    assert any("sliced_w2_fwd" in n for n in names) and any("sliced_w2_bwd" in n for n in names)
    # the drawn path: the device generator for the samples and the directions, no ATen philox kernel
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        prior(zc, step=0)
        torch.cuda.synchronize()
    names = sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})
    assert any("normal_fill" in n for n in names) and not [n for n in names if "at::" in n or "Cijk" in n], names
