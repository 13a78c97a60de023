"""GPU: ``otvae::mmd_prior`` / ``MMDPrior`` / ``ot.mmd2`` against the definition evaluated in float64 on the CPU (run with ``-m gpu``).

    r(a, b) = |a - b|^2 from explicit differences,  C_k = 2 D sigma2 s_k
    imq: k(r) = sum_k C_k / (C_k + r)        rbf: k(r) = sum_k exp(-r / C_k)
    MMD2 = cz sum_{i != j} k(r(z_i, z_j)) + cy sum_{i != j} k(r(y_i, y_j)) - 2 / (N M) sum_{i, j} k(r(z_i, y_j))
    cz, cy = 1 / (N (N - 1)), 1 / (M (M - 1)) (unbiased) or 1 / N^2, 1 / M^2 with the diagonal in the sums (biased)

and its gradient from autograd on that float64 graph.  Inputs: z = 1.3 randn + 0.2, then y = randn, from one seeded CPU generator.
Bounds (the project's fp32 contract): loss 1e-4 relative, each term 1e-5 relative, gradient rel_err 1e-4; in the matched case
(z = randn, MMD2 about 0) |loss - truth| <= 1e-5 (Ezz + Eyy + 2 Ezy)."""
import functools

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

DEFAULT = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)
SMALL = [(2, 2, 1), (2, 3, 4), (7, 5, 5), (33, 64, 16), (130, 97, 20)]
# the larger ones, imq / unbiased alone; D = 33, 65 and 129 are one past the widths at which the kernel takes more accumulator tiles
LARGE = [(257, 256, 128), (1024, 1024, 128), (16, 16, 512), (40, 33, 33), (40, 33, 65), (40, 33, 129), (40, 33, 257)]
KID = {"imq": 0, "rbf": 1}


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd as pkg
    return pkg


def _inputs(n, m, d, seed=0, matched=False, duplicate=False):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(n, d, generator=gen)
    if not matched:
        z = 1.3 * z + 0.2
    y = torch.randn(m, d, generator=gen)
    if duplicate:
        z[1] = z[0]      # two different rows with the same vector: a pair at r = 0, not a diagonal entry
    return z, y


def _kfun(r, kernel, scales, sigma2, d):
    k = torch.zeros_like(r)
    for s in scales:
        c = 2.0 * d * sigma2 * s
        k = k + (c / (c + r) if kernel == "imq" else torch.exp(-r / c))
    return k


def _truth(z, y, kernel="imq", scales=DEFAULT, sigma2=1.0, unbiased=True):
    """the definition in float64, explicit differences, row chunks (each chunk's share of the gradient by autograd)"""
    zd, yd = z.double().requires_grad_(True), y.double()
    n, d = z.shape
    m = y.shape[0]

    def block(a, b, same, weight):
        total = 0.0
        rows = max(1, (1 << 23) // (b.shape[0] * d))
        for i0 in range(0, a.shape[0], rows):
            ai = a[i0:i0 + rows]
            r = ((ai[:, None, :] - b[None, :, :]) ** 2).sum(-1)
            k = _kfun(r, kernel, scales, sigma2, d)
            s = k.sum()
            if same and unbiased:   # the diagonal by index
                idx = torch.arange(ai.shape[0])
                s = s - k[idx, idx + i0].sum()
            part = weight * s
            if part.requires_grad:
                part.backward()
            total += float(part.detach())
        return total

    ezz = block(zd, zd, True, 1.0 / (n * (n - 1)) if unbiased else 1.0 / (n * n))
    g_zz = zd.grad.clone()
    zd.grad = None
    ezy = block(zd, yd, False, 1.0 / (n * m))
    g_zy = zd.grad.clone()
    eyy = block(yd, yd, True, 1.0 / (m * (m - 1)) if unbiased else 1.0 / (m * m))
    return {"loss": ezz + eyy - 2.0 * ezy, "terms": (ezz, eyy, ezy), "grad": g_zz - 2.0 * g_zy, "mag": ezz + eyy + 2.0 * ezy}


@functools.lru_cache(maxsize=None)
def _case(n, m, d, kernel="imq", scales=DEFAULT, unbiased=True, seed=0, matched=False, duplicate=False):
    """inputs and float64 truth of a case, computed once and shared (callers do not modify them)"""
    z, y = _inputs(n, m, d, seed, matched, duplicate)
    return z, y, _truth(z, y, kernel, scales, 1.0, unbiased)


@functools.lru_cache(maxsize=None)
def _device_run(n, m, d, kernel="imq", scales=DEFAULT, unbiased=True, seed=0, matched=False, duplicate=False):
    z, y = _inputs(n, m, d, seed, matched, duplicate)
    zc, yc = z.cuda(), y.cuda()
    loss, G, terms = torch.ops.otvae.mmd_prior(zc, yc, KID[kernel], list(scales), 1.0, unbiased, 1.0, True)
    torch.cuda.synchronize()
    return zc, yc, loss, G, terms


def _check(A, n, m, d, kernel, scales, unbiased, **kw):
    _, _, t = _case(n, m, d, kernel, scales, unbiased, **kw)
    zc, yc, loss, G, terms = _device_run(n, m, d, kernel, scales, unbiased, **kw)
    assert loss.shape == (n,) and G.shape == (n, d) and terms.shape == (3,)
    assert bool((loss == loss[0]).all()), "the loss entries differ"
    err = abs(float(loss[0]) - t["loss"]) / abs(t["loss"])
    terr = [abs(float(terms[i]) - t["terms"][i]) / abs(t["terms"][i]) for i in range(3)]
    gerr = rel_err(G, t["grad"])
    print(f"mmd N={n} M={m} D={d} {kernel} S={len(scales)} unbiased={unbiased}: loss {float(loss[0]):.8g} vs {t['loss']:.8g} rel {err:.2e} "
          f"({abs(t['loss']) / t['mag']:.2e} of the magnitude), terms rel {max(terr):.2e}, grad rel {gerr:.2e}")
    assert err <= 1e-4
    assert max(terr) <= 1e-5
    assert gerr <= 1e-4
    return zc, yc, loss, G, terms, t


@pytest.mark.parametrize("scales", [DEFAULT, (1.0,)], ids=["default", "one"])
@pytest.mark.parametrize("unbiased", [True, False], ids=["unbiased", "biased"])
@pytest.mark.parametrize("kernel", ["imq", "rbf"])
@pytest.mark.parametrize("n,m,d", SMALL)
def test_small_shapes_match_float64(A, n, m, d, kernel, unbiased, scales):
    _check(A, n, m, d, kernel, scales, unbiased)


@pytest.mark.parametrize("n,m,d", LARGE)
def test_large_shapes_match_float64_reproduce_and_scale(A, n, m, d):
    zc, yc, loss, G, terms, t = _check(A, n, m, d, "imq", DEFAULT, True)
    # a second run: the same bits
    loss2, G2, terms2 = torch.ops.otvae.mmd_prior(zc, yc, 0, list(DEFAULT), 1.0, True, 1.0, True)
    assert torch.equal(loss, loss2) and torch.equal(G, G2) and torch.equal(terms, terms2), "two runs differ in their bits"
    # the scale multiplies the loss and G and leaves the terms alone
    loss3, G3, terms3 = torch.ops.otvae.mmd_prior(zc, yc, 0, list(DEFAULT), 1.0, True, 0.25, True)
    assert rel_err(loss3, 0.25 * loss) <= 1e-6 and rel_err(G3, 0.25 * G) <= 1e-6 and torch.equal(terms3, terms)
    # need_grad=False: the same loss bits, no gradient
    loss4, G4, terms4 = torch.ops.otvae.mmd_prior(zc, yc, 0, list(DEFAULT), 1.0, True, 1.0, False)
    assert torch.equal(loss4, loss) and torch.equal(terms4, terms) and G4.shape == (0, d)
    # the functional form is the same number, and so is its gradient
    z2 = zc.clone().requires_grad_(True)
    v = A.mmd2(z2, yc)
    assert float(v.detach()) == float(loss[0])
    v.backward()
    assert rel_err(z2.grad, t["grad"]) <= 1e-4
    with torch.no_grad():
        assert float(A.mmd2(zc, yc)) == float(loss[0])


@pytest.mark.parametrize("kernel", ["imq", "rbf"])
def test_matched_samples_give_a_loss_near_zero(A, kernel):
    n, m, d = 130, 97, 20
    _, _, t = _case(n, m, d, kernel, matched=True)
    _, _, loss, G, terms = _device_run(n, m, d, kernel, matched=True)
    err = abs(float(loss[0]) - t["loss"]) / t["mag"]
    print(f"mmd matched {kernel}: loss {float(loss[0]):.6e} vs {t['loss']:.6e}, error {err:.2e} of the magnitude {t['mag']:.4g}")
    assert err <= 1e-5
    assert rel_err(G, t["grad"]) <= 1e-4


@pytest.mark.parametrize("n,m,d,seed", [(7, 5, 5, 0), (130, 97, 20, 0)])
def test_gradient_through_the_prior_and_the_decoder_share(A, n, m, d, seed):
    z, y, t = _case(n, m, d, seed=seed)
    coeff = 0.5
    prior = A.MMDPrior(loss_coeff=coeff).cuda()
    zc, yc = z.cuda().requires_grad_(True), y.cuda()
    z_out, loss, art = prior(zc, step=0, prior_samples=yc)
    assert z_out.shape == zc.shape and z_out.data_ptr() == zc.data_ptr() and set(art) == {"prior_samples", "mmd_terms"}
    assert loss.shape == (n,) and bool((loss == loss[0]).all())
    assert abs(float(loss.detach().mean()) - coeff * t["loss"]) <= 1e-4 * coeff * abs(t["loss"])
    assert rel_err(art["mmd_terms"], torch.tensor(t["terms"])) <= 1e-5
    loss.mean().backward()
    err = rel_err(zc.grad, coeff * t["grad"])
    print(f"mmd prior gradient N={n} M={m} D={d}: rel {err:.2e}")
    assert err <= 1e-4
    # a decoder's share arrives through the aliased latents and is added inside the backward kernel
    own = zc.grad.clone()
    zc.grad = None
    z_out, loss, _ = prior(zc, step=0, prior_samples=yc)
    w = torch.linspace(-1, 1, n * d, device="cuda").reshape(n, d)
    (loss.mean() + (z_out * w).sum()).backward()
    assert torch.equal(zc.grad, w + own)
    # under no_grad the prior takes the path without the gradient product: the same loss bits
    with torch.no_grad():
        _, loss_ng, art_ng = prior(zc, step=0, prior_samples=yc)
    assert torch.equal(loss_ng, loss.detach()) and not loss_ng.requires_grad


@pytest.mark.parametrize("n,m,d", [(7, 5, 5), (130, 97, 20), (1024, 1024, 128)])
def test_backward_operator_on_the_kernels_own_gradient(A, n, m, d):
    G = _device_run(n, m, d)[3]
    gen = torch.Generator().manual_seed(5)
    gout = (torch.randint(-3, 4, (n,), generator=gen).float() / 8).cuda()          # dyadic: its sum is exact in any order
    if float(gout.sum()) == 0.0:
        gout[0] += 0.5
    gadd = torch.randn(n, d, generator=gen).cuda()
    gz = torch.ops.otvae.mmd_prior_backward(gout, None, G)
    assert gz.shape == (n, d) and torch.equal(gz, float(gout.sum()) * G)
    # gadd is added exactly: one fp32 addition to the very same product
    gz_add = torch.ops.otvae.mmd_prior_backward(gout, gadd, G)
    assert torch.equal(gz_add, gadd + gz)
    # gout enters as its sum
    lumped = torch.zeros_like(gout)
    lumped[n - 1] = gout.sum()
    assert torch.equal(torch.ops.otvae.mmd_prior_backward(lumped, None, G), gz)
    assert torch.equal(torch.ops.otvae.mmd_prior_backward(2 * gout, None, G), 2 * gz)


@pytest.mark.parametrize("unbiased", [True, False], ids=["unbiased", "biased"])
@pytest.mark.parametrize("n,m,d", [(7, 5, 5), (33, 64, 16)])
def test_duplicated_rows_are_a_pair_and_the_diagonal_is_not(A, n, m, d, unbiased):
    _check(A, n, m, d, "imq", DEFAULT, unbiased, duplicate=True)


def test_one_scale_imq_by_hand(A):
    z, y = _inputs(2, 2, 1)
    c = 2.0 * 1 * 1.0 * 1.0
    r = (float(z[0, 0]) - float(z[1, 0])) ** 2
    terms = _device_run(2, 2, 1, "imq", (1.0,), True)[4]
    assert abs(float(terms[0]) - c / (c + r)) <= 1e-5 * c / (c + r)          # Ezz = (k(r01) + k(r10)) / 2
    terms_b = _device_run(2, 2, 1, "imq", (1.0,), False)[4]
    want = (2.0 * c / (c + r) + 2.0) / 4.0                                     # the biased form adds k(0) = 1 twice
    assert abs(float(terms_b[0]) - want) <= 1e-5 * want


def test_values_that_are_not_finite_poison_the_loss(A):
    z, y, _ = _case(33, 64, 16)
    args = (0, list(DEFAULT), 1.0, True, 1.0, True)
    zn = z.clone()
    zn[17, 3] = float("nan")
    zi = z.clone()
    zi[5, 0] = float("inf")
    yn = y.clone()
    yn[40, 15] = float("nan")
    for zz, yy in ((zn, y), (zi, y), (z, yn)):
        loss = torch.ops.otvae.mmd_prior(zz.cuda(), yy.cuda(), *args)[0]
        assert bool(torch.isnan(loss).all())
    assert bool(torch.isfinite(_device_run(33, 64, 16)[3]).all())


def test_the_envelope_is_refused_aloud(A):
    z = torch.zeros(4, 513, device="cuda")
    with pytest.raises(NotImplementedError, match="512"):
        torch.ops.otvae.mmd_prior(z, z, 0, list(DEFAULT), 1.0, True, 1.0, True)
    with pytest.raises(NotImplementedError, match="512"):
        A.MMDPrior().cuda()(z, step=0)
    one = torch.zeros(1, 4, device="cuda")
    with pytest.raises(ValueError, match="N, M >= 2"):
        torch.ops.otvae.mmd_prior(one, torch.zeros(3, 4, device="cuda"), 0, list(DEFAULT), 1.0, True, 1.0, True)
    loss, G, terms = torch.ops.otvae.mmd_prior(one, one, 0, list(DEFAULT), 1.0, False, 1.0, True)   # the biased form takes N = M = 1
    assert float(loss[0]) == 0.0 and float(G.abs().max()) == 0.0


def test_opcheck(A):
    zc, yc, loss, G, _ = _device_run(33, 64, 16)
    for kernel, scales, unbiased in ((0, list(DEFAULT), True), (1, [1.0], False)):
        torch.library.opcheck(torch.ops.otvae.mmd_prior.default, (zc.clone().requires_grad_(True), yc, kernel, scales, 1.0, unbiased, 0.5, True))
        torch.library.opcheck(torch.ops.otvae.mmd_prior.default, (zc, yc, kernel, scales, 1.0, unbiased, 0.5, False))
    g = torch.full((33,), 1.0 / 33, device="cuda")
    torch.library.opcheck(torch.ops.otvae.mmd_prior_backward.default, (g, None, G))
    torch.library.opcheck(torch.ops.otvae.mmd_prior_backward.default, (g, torch.ones(33, 16, device="cuda"), G))


def _small_vae(A, seed=41):
    torch.manual_seed(seed)
    enc = A.CNN(1, 16, 16, 1, capacity=4, down_sample=True, residual="add")
    dec = A.CNN(16, 1, 1, 16, capacity=4, up_sample=True, residual="add")
    return A.VAE(encoder=enc, decoder=dec, prior=A.MMDPrior(loss_coeff=0.5, seed=7)).cuda().train()


def test_small_vae_trains_eagerly_and_captured(A):
    from detfill import normal
    B = 64
    xs = [normal((B, 1, 16, 16), 300 + i).cuda() for i in range(3)]
    ps = normal((48, 16), 310).cuda()      # any M

    # the same draws handed in: the eager step and the captured one agree
    out = {}
    for graph in (False, True):
        tr = A.HipTrainer(_small_vae(A), batch_shape=(B, 1, 16, 16), use_graph=graph, batch_kwargs={"prior_samples": ps})
        out[graph] = torch.stack([tr.step(x).clone() for x in xs])
        torch.cuda.synchronize()
        assert tr.skipped_steps == 0
        tr.close()
    print("mmd VAE [total, recon, prior] eager:\n", out[False].cpu(), "\ncaptured:\n", out[True].cpu())
    assert bool(torch.isfinite(out[False]).all()) and bool(torch.isfinite(out[True]).all())
    assert bool((out[False][:, 2] > 0).all())
    assert rel_err(out[True], out[False]) <= 1e-5

    # its own draws: fresh on every replay of the captured step (lr = 0 and one batch: only the draws change)
    tr = A.HipTrainer(_small_vae(A), batch_shape=(B, 1, 16, 16), use_graph=True, lr=0.0)
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


def test_prior_step_launches_only_its_own_kernels(A):
    """prior forward + backward under the profiler: only this prior's kernels (no library GEMM, no ATen fill / copy), at most two
    launches forward and one backward"""
    from torch.profiler import ProfilerActivity, profile
    z, y = _inputs(1024, 1024, 128)
    zc, yc = z.cuda().requires_grad_(True), y.cuda()
    prior = A.MMDPrior(loss_coeff=0.5).cuda()
    gl = torch.full((1024,), 1.0 / 1024, device="cuda")

    def run():
        zc.grad = None
        _, loss, _ = prior(zc, step=0, prior_samples=yc)
        torch.autograd.backward(loss, grad_tensors=[gl], inputs=[zc])

    run()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        run()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert names, "the profiler saw no device kernels"
    foreign = [n for n in names if "mmd" not in n]
    assert not foreign, foreign
    fwd = [n for n in names if "mmd_fwd" in n or "mmd_finish" in n]
    bwd = [n for n in names if "mmd_bwd" in n]
    assert 1 <= len(fwd) <= 2 and len(bwd) == 1 and len(names) == len(fwd) + len(bwd), names
    # the drawn path: the device generator for the samples, no ATen philox kernel
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        prior(zc, step=0)
        torch.cuda.synchronize()
    names = sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})
    assert any("normal_fill" in n for n in names) and not [n for n in names if "at::" in n or "Cijk" in n], names
