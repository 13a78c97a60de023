"""GPU: the fused FiLM + activation kernels, the Fourier time features, the class / time conditioned ``AutoEncoder`` against the
reference's recorded results (tests/golden/autodiffusion.npz, written by tools/gen_golden_autodiffusion.py) and ``AutoDiffusion``
(loss, sampling loop, captured training step).

Bounds follow the evidence rule of tests/test_gpu_dad.py::vs_truth: for a quantity with a float64 truth T the bound is
max(1e-4, 1.5 x the error of the fp32 reference against T); gradients use the contracts GRAD_TOL_L2 / GRAD_TOL_MAX of
tests/test_gpu_parity.py in the same way (``grads_vs_truth`` below is ``Report.check_grads_vs_truth`` as a function)."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL32, FACTOR = 1e-4, 1.5
GRAD_TOL_L2, GRAD_TOL_MAX = 2e-3, 5e-3


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd as A_
    return A_


@pytest.fixture(scope="module")
def gold():
    return load_golden("autodiffusion.npz")


def vs_truth(name, got, ref32, truth, floor=0.0):
    t = truth.detach().double().cpu()
    scale = max(t.abs().max().item(), floor, 1e-30)
    e_hip = (got.detach().double().cpu() - t).abs().max().item() / scale
    e_ref = (ref32.detach().double().cpu() - t).abs().max().item() / scale
    tol = max(TOL32, FACTOR * e_ref)
    print(f"[autodiffusion] {name}: hip vs fp64 truth {e_hip:.3e}  reference fp32 vs truth {e_ref:.3e}  bound {tol:.3e}")
    assert math.isfinite(e_hip) and e_hip <= tol, (name, e_hip, e_ref, tol)


def grads_vs_truth(name, got, ref32, truth, names):
    """per tensor: relative L2 and max error of HIP and of the fp32 reference against the fp64 truth (denominators never below 1e-2
    of the network's gradient scale); the tensor's bound is the contract or 1.5 x the reference's own error, whichever is larger"""
    got, ref32, truth = ([t.detach().double().cpu() for t in lst] for lst in (got, ref32, truth))
    assert all(a.shape == b.shape for a, b in zip(got, truth)), "gradient lists differ in shape"
    rms_scale = max(float(b.norm()) / max(b.numel(), 1) ** 0.5 for b in truth)
    max_scale = max(float(b.abs().max()) for b in truth)
    failed, worst = [], (0.0, "")
    for a, r, b, tag in zip(got, ref32, truth, names):
        n = b.numel() ** 0.5
        d2, dm = max(float(b.norm()), 1e-2 * rms_scale * n, 1e-30), max(float(b.abs().max()), 1e-2 * max_scale, 1e-30)
        h2, hm = float((a - b).norm()) / d2, float((a - b).abs().max()) / dm
        r2, rm = float((r - b).norm()) / d2, float((r - b).abs().max()) / dm
        t2, tm = max(GRAD_TOL_L2, FACTOR * r2), max(GRAD_TOL_MAX, FACTOR * rm)
        if not (h2 <= t2 and hm <= tm and math.isfinite(h2) and math.isfinite(hm)):
            failed.append((tag, (h2, hm), (r2, rm), (t2, tm)))
        if max(h2 / t2, hm / tm) > worst[0]:
            worst = (max(h2 / t2, hm / tm), f"{tag}: hip ({h2:.2e}, {hm:.2e}) reference fp32 ({r2:.2e}, {rm:.2e}) bound ({t2:.2e}, {tm:.2e})")
    print(f"[autodiffusion] {name}: {len(got)} tensors vs fp64 truth, tightest {worst[1]}")
    assert not failed, failed


def normal(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---- otvae_film_act_fwd / _bwd ---------------------------------------------------------------------------------------------------------
# C not a multiple of 4 / HW = 1 / an HW that the launcher cuts into 18 row chunks of 64 with one row left over (N = 2: the batch alone
# does not fill the chip) and whose row lanes (256 // 3 = 85) do not divide the chunk either / C above 128 (one channel per lane, two
# chunks of 64 + 6 rows)
FILM_SHAPES = [(3, 5, 6), (2, 1, 8), (2, 1089, 12), (1, 70, 130)]
TORCH_ACT = {0: lambda v: v, 1: F.relu, 2: lambda v: F.leaky_relu(v, 0.2), 3: F.selu, 4: F.gelu, 5: F.silu}


def _film_reference(x, s, b, g, kind, dtype):
    """the definition, restated with torch operators on the host: out = act(x * s + b), gradients by autograd"""
    x, s, b = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, s, b))
    out = TORCH_ACT[kind](x * s[:, :, None, None] + b[:, :, None, None])
    out.backward(g.to(dtype))
    return out.detach(), x.grad, s.grad, b.grad


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("shape", FILM_SHAPES)
def test_film_act_forward_bits_and_backward_truth(A, shape, kind):
    HF = A.functional
    n, hw, c = shape
    x = normal((n, c, hw, 1), 11 + kind)
    s, b, g = 1.0 + 0.5 * normal((n, c), 12), 0.3 * normal((n, c), 13), normal((n, c, hw, 1), 14)
    xd = HF.as_nhwc(x.cuda()).requires_grad_(True)
    sd, bd = s.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    gd = HF.as_nhwc(g.cuda())
    out = HF.film_act(xd, sd, bd, kind)
    # forward: the same bits as the kept two-launch chain
    with torch.no_grad():
        old = HF._FilmFn.apply(xd.detach(), sd.detach(), bd.detach())
        if kind != 0:
            old = HF._BnActFn.apply(old, None, None, None, kind, (None, None))
    assert out.shape == x.shape and HF.is_nhwc(out) and torch.equal(out, old)
    gx, gs, gb = torch.autograd.grad(out, (xd, sd, bd), gd)
    ref32, truth = _film_reference(x, s, b, g, kind, torch.float32), _film_reference(x, s, b, g, kind, torch.float64)
    tag = f"film_act {shape} kind {kind}"
    vs_truth(tag + " out", out, ref32[0], truth[0])
    vs_truth(tag + " gx", gx, ref32[1], truth[1])
    vs_truth(tag + " gscale", gs, ref32[2], truth[2])
    vs_truth(tag + " gbias", gb, ref32[3], truth[3])
    # the same call again: the same bits (fixed-order fp64 sums, no floating-point atomics)
    out2 = HF.film_act(xd, sd, bd, kind)
    gx2, gs2, gb2 = torch.autograd.grad(out2, (xd, sd, bd), gd)
    assert torch.equal(out, out2) and torch.equal(gx, gx2) and torch.equal(gs, gs2) and torch.equal(gb, gb2)
    # an embedding that takes no gradient: only gx is computed, with the same bits
    out3 = HF.film_act(xd, sd.detach(), bd.detach(), kind)
    (gx3,) = torch.autograd.grad(out3, (xd,), gd)
    assert torch.equal(out3, out) and torch.equal(gx3, gx)


def test_film_act_refuses_bad_arguments(A):
    HF = A.functional
    x = torch.zeros(2, 4, 3, 3, device="cuda")
    with pytest.raises(ValueError):
        HF.film_act(x, torch.zeros(2, 5, device="cuda"), torch.zeros(2, 5, device="cuda"), 1)
    with pytest.raises(ValueError):
        HF.film_act(x, torch.zeros(2, 4, device="cuda"), torch.zeros(2, 4, device="cuda"), 6)
    with pytest.raises(RuntimeError):
        HF.film_act(x.cpu(), torch.zeros(2, 4), torch.zeros(2, 4), 1)


def test_film_layer_takes_the_fused_route(A, monkeypatch):
    """a ConvLayer with `additional_embed` issues otvae_film_act_* and no longer the two-launch chain"""
    HF = A.functional
    calls = []
    real = HF._FilmActFn.apply
    monkeypatch.setattr(HF._FilmActFn, "apply", staticmethod(lambda *a: (calls.append(a[3]), real(*a))[1]))
    monkeypatch.setattr(HF._FilmFn, "apply", staticmethod(lambda *a: pytest.fail("the unfused FiLM chain ran")))
    torch.manual_seed(0)
    layer = A.ConvLayer(6, 4, additional_embed=5, normalization="batchnorm", activation="gelu").cuda()
    y = layer(normal((2, 6, 5, 5), 1).cuda(), normal((2, 5), 2).cuda())
    y.square().mean().backward()
    assert calls == [HF.ACT_KINDS["gelu"]] and layer._embed_proj_scale.weight.grad is not None


# ---- otvae_fourier_features ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 34])
@pytest.mark.parametrize("times", [[0.0], [1.0], [0.0, 1.0, 0.5, 0.123456, 0.999, 1e-6, 0.75]])
def test_fourier_features(A, times, dim):
    t = torch.tensor(times, dtype=torch.float32)
    w = 30.0 * normal((1, dim // 2), 21 + dim)
    p32 = t.unsqueeze(-1) * w * 2 * np.pi                 # fp32, the reference's order of operations
    truth = torch.cat([torch.sin(p32.double()), torch.cos(p32.double())], dim=-1)
    ref32 = torch.cat([torch.sin(p32), torch.cos(p32)], dim=-1)
    got = A.functional.fourier_features(t.cuda(), w.cuda())
    assert got.shape == (len(times), dim) and got.dtype == torch.float32
    vs_truth(f"fourier_features N={len(times)} dim={dim} (|p| up to {float(p32.abs().max()):.0f} rad)", got, ref32, truth)
    zero = [i for i, v in enumerate(times) if v == 0.0]
    if zero:   # t = 0 exactly: sin 0, cos 1
        assert torch.equal(got[zero[0]].cpu(), torch.cat([torch.zeros(dim // 2), torch.ones(dim // 2)]))


# ---- against the reference's recorded results ----------------------------------------------------------------------------------------
def _load(module, gold, tag):
    names = [str(n) for n in gold[f"{tag}/names"]]
    module.load_state_dict({n: torch.from_numpy(gold[f"{tag}/state/{n}"]) for n in names})
    return module.cuda().train()


def _recorded_grads(gold, tag, module):
    names = [n for n, p in module.named_parameters() if p.requires_grad]
    assert sorted(names) == sorted(k[len(f"{tag}/f64/grad/"):] for k in gold.files if k.startswith(f"{tag}/f64/grad/"))
    return names, [torch.from_numpy(gold[f"{tag}/f32/grad/{n}"]) for n in names], [torch.from_numpy(gold[f"{tag}/f64/grad/{n}"]) for n in names]


def test_fourier_projection_against_the_reference(A, gold):
    gfp = _load(A.GaussianFourierProjection(8, 8), gold, "gfp")
    out = gfp(torch.from_numpy(gold["gfp/time"]).cuda())
    vs_truth("GaussianFourierProjection out", out, torch.from_numpy(gold["gfp/f32/out"]), torch.from_numpy(gold["gfp/f64/out"]))
    out.square().mean().backward()
    names, g32, g64 = _recorded_grads(gold, "gfp", gfp)
    assert "proj.2.weight" in names and "proj.4.weight" not in names     # one tensor, used twice: its gradient is the sum of both uses
    params = dict(gfp.named_parameters())
    grads_vs_truth("GaussianFourierProjection", [params[n].grad for n in names], g32, g64, names)


def test_conditioned_autoencoder_against_the_reference(A, gold):
    ae = _load(A.AutoEncoder(1, 4, 8, 2, capacity=4, num_classes=10, time_embed_dim=8, residual="add", down_up_sample=True), gold, "ae")
    x, labels, time = (torch.from_numpy(gold[f"ae/{k}"]).cuda() for k in ("x", "labels", "time"))
    h = ae.encode(x, labels, time)
    y = ae.decode(h, labels, time)
    vs_truth("AutoEncoder encode", h, torch.from_numpy(gold["ae/f32/h"]), torch.from_numpy(gold["ae/f64/h"]))
    vs_truth("AutoEncoder decode", y, torch.from_numpy(gold["ae/f32/y"]), torch.from_numpy(gold["ae/f64/y"]))
    y.square().mean().backward()
    names, g32, g64 = _recorded_grads(gold, "ae", ae)
    params = dict(ae.named_parameters())
    assert all(params[n].grad is not None for n in names), [n for n in names if params[n].grad is None]
    grads_vs_truth("AutoEncoder", [params[n].grad for n in names], g32, g64, names)


# ---- AutoDiffusion -------------------------------------------------------------------------------------------------------------------
B, IMG, LAT = 6, (1, 8, 8), (4, 2, 2)


def _model(A, seed=5, expansion=1):
    torch.manual_seed(seed)
    ae = A.AutoEncoder(1, 4, 8, 2, capacity=4, num_classes=10, time_embed_dim=8, residual="add", down_up_sample=True)
    return A.AutoDiffusion(autoencoder=ae, prior=A.GaussianPrior(loss_coeff=0.5, fixed_var=True), conditional=True,
                           expansion=expansion).cuda()


def _batch(seed=7):
    x, eps = normal((B, *IMG), seed).cuda(), normal((B, *LAT), seed + 1).cuda()
    labels = torch.tensor([3, 0, 9, 9, 1, 7]).cuda()
    time = torch.tensor([0.0, 1.0, 0.5, 0.4, 0.73, 0.55]).cuda()
    return x, eps, labels, time


def test_nelbo_is_recon_plus_beta_weighted_prior(A):
    model = _model(A).train()
    assert tuple(model.latent_size) == LAT
    x, eps, labels, time = _batch()
    loss, logs, art = model.nelbo({"samples": x, "target": x, "kwargs": {"labels": labels, "time": time, "eps": eps}}, 0)
    with torch.no_grad():   # the package's own prior on the same encodings (training mode: the batch statistics are the same)
        enc = model.autoencoder.encode(x, labels, time)
        z, prior_vec, _ = model.prior(enc, step=0, time=time, eps=eps)
        beta = 0.5 * torch.tanh(10 * (time.double() - 0.5)) + 0.5
        want_prior = (beta * prior_vec.double()).mean() / float(np.prod(IMG))
        recon = F.mse_loss(model.autoencoder.decode(z, labels, time).double(), x.double())
    assert torch.equal(art["latents"], z)
    # fp32 sums of B terms and one fp32 addition: a few units of 2^-24 each
    got = {k: float(v.detach()) for k, v in logs.items()}
    print(f"[autodiffusion] nelbo {got}  recon {float(recon):.8f}  prior {float(want_prior):.8f}")
    assert float(prior_vec.abs().max()) > 0 and float(want_prior) > 0
    assert abs(got["train/loss/recon"] - float(recon)) <= 1e-5 * float(recon)
    assert abs(got["train/loss/prior"] - float(want_prior)) <= 1e-5 * float(want_prior)
    assert abs(got["train/loss/total"] - (got["train/loss/recon"] + float(want_prior))) <= 1e-5 * got["train/loss/total"]
    loss.backward()
    params = list(model.optim_parameters())
    assert len(params) == sum(1 for p in model.autoencoder.parameters() if p.requires_grad)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params)
    assert model.autoencoder.time_embed.weight.grad is None     # the random frequencies are not trained


def test_prior_without_fixed_var_refuses_the_time(A):
    torch.manual_seed(1)
    ae = A.AutoEncoder(1, 4, 8, 2, capacity=4, time_embed_dim=8, double_encoded_features=True, down_up_sample=True)
    model = A.AutoDiffusion(autoencoder=ae, prior=A.GaussianPrior()).cuda().train()
    x = normal((B, *IMG), 3).cuda()
    with pytest.raises(NotImplementedError, match="fixed_var"):
        model.nelbo({"samples": x, "target": x, "kwargs": {"time": torch.rand(B).cuda()}}, 0)


@pytest.mark.parametrize("improved", [False, True])
def test_sample_equals_the_hand_written_loop(A, improved):
    model = _model(A).eval()
    n = model.n_steps
    labels = torch.tensor([3, 0, 9, 9, 1, 7]).cuda()
    latents = normal((B, *LAT), 31).cuda()
    noise = normal((n * (2 if improved else 1), B, *LAT), 32).cuda()
    keep = latents.clone()
    got = model.sample(B, steps=list(range(n)), improved_algorithm=improved, latents=latents, noise=noise, labels=labels)
    assert torch.equal(latents, keep) and len(got) == n
    ones, xs, k, want = torch.ones(B, device="cuda"), latents.clone(), 0, []
    with torch.no_grad():
        for s in np.linspace(1, 1 / n, n):
            x_hat = model.decode(xs, labels=labels, time=ones * s)
            if improved:
                a = model.encode(x_hat, labels=labels, time=ones * (s - 1 / n), eps=noise[k])
                b = model.encode(x_hat, labels=labels, time=ones * s, eps=noise[k + 1])
                xs, k = xs - (a - b), k + 2
            else:
                xs, k = model.encode(x_hat, labels=labels, time=ones * (s - 1 / n), eps=noise[k]), k + 1
            want.append(x_hat)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and bool(torch.isfinite(got[-1]).all())
    assert torch.equal(model.sample(B, improved_algorithm=improved, latents=latents, noise=noise, labels=labels), want[-1])
    assert float((want[0] - want[-1]).abs().max()) > 0
    # without `latents` / `noise` the prior and the device generator draw
    free = model.sample(B, improved_algorithm=improved, labels=labels)
    assert free.shape == (B, *IMG) and bool(torch.isfinite(free).all())


def test_captured_step_equals_the_eager_step(A):
    """three ``HipTrainer`` steps with ``time`` and ``labels`` resident as batch keywords: the captured graph leaves the parameters
    bit-equal to three eagerly issued steps (the FiLM sums are order-fixed, the time embedding skips its range check while capturing)"""
    model = _model(A, seed=9).train()
    twin = copy.deepcopy(model)
    x, eps, labels, time = _batch(17)
    kw = {"time": time, "labels": labels}
    t_graph = A.HipTrainer(model, batch_shape=(B, *IMG), use_graph=True, batch_kwargs=kw)
    t_eager = A.HipTrainer(twin, batch_shape=(B, *IMG), use_graph=False, batch_kwargs=kw)
    p0 = t_graph.pflat.clone()
    for i in range(3):
        time_i = (time + 0.1 * i).clamp(0, 1)
        a, b = t_graph.step(x, eps, time=time_i, labels=labels), t_eager.step(x, eps, time=time_i, labels=labels)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert torch.equal(t_graph.pflat, t_eager.pflat) and not torch.equal(t_graph.pflat, p0)
    # the shared Linear of the time embedding moved (its two gradients were added, not overwritten), the frequencies did not
    te, te0 = model.autoencoder.time_embed, _model(A, seed=9).autoencoder.time_embed
    assert not torch.equal(te.proj[2].weight, te0.proj[2].weight) and torch.equal(te.weight, te0.weight)
    t_graph.close(); t_eager.close()
