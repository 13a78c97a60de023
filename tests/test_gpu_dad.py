"""GPU: the Discrete Auto Diffuser -- ``otvae::soft_cross_entropy`` and the sampling kernels against float64 truth formed in the
test, the model against the reference's own DAD (tests/golden/dad.npz, tools/gen_dad_golden.py), and the three training routes.

Bound (the rule of ``check_vs_truth`` in tests/test_gpu_parity.py): with the float64 truth T of a quantity,
|hip - T| <= max(1e-4 * scale, 1.5 * |reference_fp32 - T|), scale = max |T|: the fp32 contract or 1.5x the error of the reference's
own fp32 composition on the same inputs.  The reference composition is evaluated here with stock torch operators; nothing in a
bound comes from the kernels under test.  For a model's parameter gradients the scale of a tensor is floored at 1 % of the largest
gradient entry of the network: a tensor whose true gradient is that small holds rounding noise of the activations on both sides."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import group, load_golden
from test_dad_host import CONFIGS, build_dad

pytestmark = pytest.mark.gpu

TOL32, FACTOR = 1e-4, 1.5


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd as A_
    return A_


def vs_truth(name, got, ref32, truth, floor=0.0):
    t = truth.detach().double().cpu()
    scale = max(t.abs().max().item(), floor, 1e-30)
    e_hip = (got.detach().double().cpu() - t).abs().max().item() / scale
    e_ref = (ref32.detach().double().cpu() - t).abs().max().item() / scale
    tol = max(TOL32, FACTOR * e_ref)
    print(f"[dad] {name}: hip vs fp64 truth {e_hip:.3e}  reference fp32 vs truth {e_ref:.3e}  bound {tol:.3e}")
    assert math.isfinite(e_hip) and e_hip <= tol, (name, e_hip, e_ref, tol)


def reference_ce(logits, probs):
    """discrete_auto_diffuser.py:63-72, as the reference writes it"""
    shift_logits, shift_labels = logits[:, :-1].contiguous(), probs[:, 1:].contiguous()
    return F.cross_entropy(shift_logits.transpose(-1, -2), shift_labels.transpose(-1, -2), reduction="none").sum(-1)


def ce_case(kind, B, T, K, seed):
    g = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn(B, T, K, generator=g)
    probs = torch.softmax(1.5 * torch.randn(B, T, K, generator=g), -1)
    if kind == "peaked":          # a row spanning +-80: the soft-max is one-hot to fp32
        logits[0, 0] = torch.linspace(-80.0, 80.0, K)[torch.randperm(K, generator=g)]
        logits[1, T - 2, :] = -80.0
        logits[1, T - 2, K // 3] = 80.0
    if kind == "unnormalised":    # label rows that do not sum to 1
        probs = probs * (0.25 + 2.0 * torch.rand(B, T, 1, generator=g))
    return logits, probs, torch.randn(B, generator=g)


CE_CASES = [("plain", 6, 4, 32), ("plain", 50, 16, 128), ("plain", 32, 64, 8192), ("strided", 7, 5, 96), ("strided", 3, 4, 33),
            ("peaked", 6, 4, 32), ("peaked", 4, 8, 8192), ("unnormalised", 50, 16, 128), ("plain", 3, 2, 1)]


@pytest.mark.parametrize("kind,B,T,K", CE_CASES)
def test_soft_cross_entropy_vs_fp64_truth(A, kind, B, T, K):
    logits, probs, gl = ce_case(kind, B, T, K, seed=B * 1000 + K)
    # float64 truth on the CPU, from the formula
    l64, p64 = logits.double().requires_grad_(True), probs.double().requires_grad_(True)
    ce64 = -(p64[:, 1:] * torch.log_softmax(l64[:, :-1], -1)).sum((-1, -2))
    (ce64 * gl.double()).sum().backward()
    # the reference's fp32 composition, stock torch
    l32, p32 = logits.cuda().requires_grad_(True), probs.cuda().requires_grad_(True)
    ce32 = reference_ce(l32, p32)
    (ce32 * gl.cuda()).sum().backward()
    # the operator
    lh, ph = logits.cuda(), probs.cuda()
    if kind == "strided":         # non-contiguous batch / token strides (every other token of a wider buffer; padded rows)
        lh = lh.repeat_interleave(2, 1)[:, ::2]
        ph = F.pad(ph, (0, 4))[..., :K]
        assert not lh.is_contiguous() and not ph.is_contiguous() and lh.stride(2) == ph.stride(2) == 1
    lh, ph = lh.requires_grad_(True), ph.requires_grad_(True)
    loss, lse, psum = torch.ops.otvae.soft_cross_entropy(lh, ph)
    assert loss.shape == (B,) and lse.shape == (B, T) and psum.shape == (B, T)
    (loss * gl.cuda()).sum().backward()
    tag = f"{kind} ({B},{T},{K})"
    vs_truth(f"{tag} loss", loss, ce32, ce64)
    vs_truth(f"{tag} dlogits", lh.grad, l32.grad, l64.grad)
    vs_truth(f"{tag} dprobs", ph.grad, p32.grad, p64.grad)
    vs_truth(f"{tag} lse", lse[:, :-1], torch.logsumexp(l32[:, :-1], -1), torch.logsumexp(l64[:, :-1], -1))
    vs_truth(f"{tag} psum", psum[:, :-1], p32[:, 1:].sum(-1), p64[:, 1:].sum(-1))
    # the structural zeros are exact
    assert torch.equal(lh.grad[:, T - 1], torch.zeros_like(lh.grad[:, T - 1]))
    assert torch.equal(ph.grad[:, 0], torch.zeros_like(ph.grad[:, 0]))
    # one output only
    only_l = torch.autograd.grad((torch.ops.otvae.soft_cross_entropy(lh, ph.detach())[0] * gl.cuda()).sum(), lh)[0]
    assert torch.equal(only_l, lh.grad)
    only_p = torch.autograd.grad((torch.ops.otvae.soft_cross_entropy(lh.detach(), ph)[0] * gl.cuda()).sum(), ph)[0]
    assert torch.equal(only_p, ph.grad)


def test_soft_cross_entropy_opcheck_and_refusals(A):
    g = torch.Generator().manual_seed(5)
    l = torch.randn(3, 4, 16, generator=g).cuda().requires_grad_(True)
    p = torch.softmax(torch.randn(3, 4, 16, generator=g), -1).cuda().requires_grad_(True)
    torch.library.opcheck(torch.ops.otvae.soft_cross_entropy.default, (l, p))
    torch.library.opcheck(torch.ops.otvae.soft_cross_entropy.default, (l.detach(), p.detach()))
    with pytest.raises(NotImplementedError):     # OTVAE_EUNSUPPORTED: a single token predicts nothing
        torch.ops.otvae.soft_cross_entropy(l[:, :1].detach(), p[:, :1].detach())
    with pytest.raises(ValueError):
        torch.ops.otvae.soft_cross_entropy(l.detach(), p[:, :3].detach())
    with pytest.raises(ValueError):
        torch.ops.otvae.soft_cross_entropy(l.detach().double(), p.detach().double())


# ------------------------------------------------------------------------------------------------ the model against the reference
def load_model(A, tag, dropout=0.0):
    g = group(load_golden("dad.npz"), tag)
    model = build_dad(**CONFIGS[tag], dropout=dropout)
    state = {k[len("state/"):]: v for k, v in g.items() if k.startswith("state/")}
    model.load_state_dict(state, strict=True)
    return model.cuda().train(), g


@pytest.mark.parametrize("tag", ["A", "B"])
def test_dad_nelbo_and_gradients_vs_reference_golden(A, tag):
    """The reference's DAD on the recorded weights, batch and draws: the sampled indices bit for bit, the three losses and every
    parameter's gradient against the reference's float64 run, bounded by the reference's float32 run (module docstring)."""
    model, g = load_model(A, tag)
    cm = model.prior.codebook_model
    cm.index_noise = g["u_index"].cuda()
    if "gumbel" in cm.training_mode:
        cm.gumbel_noise = g["gumbel"].cuda()
    x = g["x"].cuda()
    loss, logs, art = model.nelbo(model.batch_preprocess((x, torch.zeros(x.shape[0], dtype=torch.long))), 0)
    loss.backward()
    assert cm.index_noise is None
    assert torch.equal(art["indices"].cpu(), g["indices"]), "the sampled token ids must be bit-exact"
    got = torch.stack([logs["train/loss/total"], logs["train/loss/recon"], logs["train/loss/prior"]])
    for i, name in enumerate(("total", "recon", "prior")):
        vs_truth(f"{tag} loss/{name}", got[i], g["loss32"][i], g["loss64"][i])
    names = [str(n) for n in g["params"]]
    params = dict(model.named_parameters())
    biggest = max(float(g[f"grad64/{n}"].abs().max()) for n in names)
    assert biggest > 0
    ar_seen = 0
    for n in names:
        assert params[n].grad is not None, f"{n} received no gradient"
        vs_truth(f"{tag} d/d {n}", params[n].grad, g[f"grad32/{n}"], g[f"grad64/{n}"], floor=1e-2 * biggest)
        ar_seen += n.startswith("autoregressive_decoder.")
    assert ar_seen > 0
    # prior_loss itself keeps the reference's contract: the mean of (prior_loss + ce_coeff * ce)
    cm.index_noise = g["u_index"].cuda()
    if "gumbel" in cm.training_mode:
        cm.gumbel_noise = g["gumbel"].cuda()
    with torch.no_grad():
        _, pl, art = model.encode(x, return_prior_artifacts=True)
        total = model.prior_loss(pl, art)
        ce = reference_ce(model.autoregressive_decoder(art["indices"]), art["distribution"].probs)
    assert total.dim() == 0
    assert abs(float(total) - float((pl + model.hparams.ce_coeff * ce).mean())) <= 1e-5 * abs(float(total)) + 1e-7


# ------------------------------------------------------------------------------------------------ sampling
def inverse_cdf(logits64, u):
    cdf = torch.softmax(logits64, -1).cumsum(-1)
    return (cdf <= u.double().unsqueeze(-1)).sum(-1).clamp(max=logits64.shape[-1] - 1), cdf


@pytest.mark.parametrize("K", [32, 128, 8192])
def test_categorical_sample_exact(A, K):
    """Inputs whose answer is unambiguous: per row a target index whose float64 CDF interval is at least 1e-3 wide, u its midpoint.
    Every index must match."""
    from ot_vae_lightning_amd import functional as HF
    B, T, pos, col = 96, 5, 1, 2
    g = torch.Generator().manual_seed(K)
    logits = 3.0 * torch.randn(B, 3, K, generator=g)
    cdf = torch.softmax(logits[:, pos].double(), -1).cumsum(-1)
    lo = torch.cat([torch.zeros(B, 1, dtype=torch.float64), cdf[:, :-1]], 1)
    wide = (cdf - lo) >= 1e-3
    assert bool(wide.any(-1).all())
    pick = torch.multinomial(wide.float(), 1, generator=g).squeeze(1)                 # one of the wide intervals per row
    assert pick.unique().numel() > 4
    u = (0.5 * (lo + cdf)).gather(1, pick[:, None]).squeeze(1)
    ids0 = torch.randint(0, K, (B, T), generator=g)
    ids = ids0.clone().cuda()
    out = HF.categorical_sample_(ids, col, logits.cuda(), pos, u=u.float().cuda())
    assert out is ids
    assert torch.equal(ids[:, col].cpu(), pick), (ids[:, col].cpu() != pick).nonzero().flatten().tolist()
    keep = [c for c in range(T) if c != col]
    assert torch.equal(ids[:, keep].cpu(), ids0[:, keep])
    # a non-contiguous view of the logits, u = 0 and u just below 1
    view = logits.cuda().transpose(0, 1).contiguous().transpose(0, 1)
    assert not view.is_contiguous()
    HF.categorical_sample_(ids, 0, view, pos, u=u.float().cuda())
    assert torch.equal(ids[:, 0].cpu(), pick)
    first = (cdf > 0).double().argmax(-1)
    HF.categorical_sample_(ids, 1, logits.cuda(), pos, u=torch.zeros(B).cuda())
    assert torch.equal(ids[:, 1].cpu(), first)
    # drawn on the device: in range, reproducible for a key, different for the next call counter
    key = HF.new_dropout_key("cuda", seed=123)
    a, b, c = (torch.zeros(B, T, dtype=torch.int64, device="cuda") for _ in range(3))
    HF.categorical_sample_(a, 3, logits.cuda(), pos, key=key)
    HF.categorical_sample_(b, 3, logits.cuda(), pos, key=key)
    key[1:].add_(1)
    HF.categorical_sample_(c, 3, logits.cuda(), pos, key=key)
    assert torch.equal(a, b) and not torch.equal(a, c) and int(a.min()) >= 0 and int(a.max()) < K
    with pytest.raises(ValueError):
        HF.categorical_sample_(ids, T, logits.cuda(), pos, u=u.float().cuda())        # column outside the id matrix


def test_codebook_gather(A):
    from ot_vae_lightning_amd import functional as HF
    g = torch.Generator().manual_seed(9)
    cb = torch.randn(37, 12, generator=g).cuda().requires_grad_(True)
    ids = torch.randint(0, 37, (5, 7), generator=g).cuda()
    out = HF.codebook_gather(cb, ids)
    assert torch.equal(out, cb.detach()[ids])
    assert torch.equal(out, (F.one_hot(ids, 37).float() @ cb.detach()))
    w = torch.randn(5, 7, 12, generator=g).cuda()
    (out * w).sum().backward()
    want = torch.zeros(37, 12, dtype=torch.float64).index_add_(0, ids.flatten().cpu(), w.reshape(-1, 12).double().cpu())
    assert float((cb.grad.double().cpu() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_dad_sample_end_to_end(A):
    torch.manual_seed(21)
    model = build_dad().cuda().eval()
    B, T, K = 200, model.n_tokens, model.num_embeddings
    g = torch.Generator().manual_seed(22)
    init = torch.randint(0, K, (B, T), generator=g)
    noise = torch.rand(B, T - 1, generator=g)
    seen = {}
    orig = A.functional.codebook_gather

    def spy(codebook, ids):
        seen["ids"] = ids.clone()
        return orig(codebook, ids)

    A.functional.codebook_gather = spy
    try:
        with torch.no_grad():
            img1 = model.sample(B, init_indices=init, noise=noise)
            img2 = model.sample(B, init_indices=init.cuda(), noise=noise.cuda())
    finally:
        A.functional.codebook_gather = orig
    assert img1.shape == (B, 1, 8, 8) and torch.equal(img1, img2)
    ids = seen["ids"]
    assert torch.equal(ids[:, 0].cpu(), init[:, 0])
    with torch.no_grad():
        logits = model.autoregressive_decoder(ids).double().cpu()      # causal: position i does not see the later tokens
        latents = model.prior.unflatten_and_unpermute(model.prior.codebook_model.codebook.reshape(K, -1)[ids].transpose(0, 1))
        assert torch.equal(model.decode(latents), img1)
    skipped = total = 0
    for i in range(T - 1):
        want, cdf = inverse_cdf(logits[:, i], noise[:, i])
        near = ((cdf - noise[:, i].double().unsqueeze(-1)).abs().min(-1).values < 1e-4)
        ok = (ids[:, i + 1].cpu() == want) | near
        assert bool(ok.all()), (i, (~ok).nonzero().flatten().tolist())
        skipped, total = skipped + int(near.sum()), total + B
    print(f"[dad] sample: {skipped} of {total} positions within 1e-4 of a CDF boundary were left out")
    assert skipped <= 0.05 * total
    # drawn on the device: valid images, new ones on every call
    with torch.no_grad():
        a, b = model.sample(8), model.sample(8)
    assert a.shape == (8, 1, 8, 8) and bool(torch.isfinite(a).all()) and not torch.equal(a, b)
    with pytest.raises(ValueError):
        model.sample(4, noise=noise[:4, :1])


# ------------------------------------------------------------------------------------------------ training routes
def test_dad_trains_through_hiptrainer_captured_equals_eager(A):
    """Configuration A through ``HipTrainer``: one captured step equals the eagerly issued one bit for bit (same device generator
    state in front of both: the token ids and the Gumbel noise are drawn inside the step), the autoregressive decoder's parameters
    move, and twenty steps on a fixed batch lower the loss."""
    import copy
    model, g = load_model(A, "A")
    twin = copy.deepcopy(model)
    x = g["x"].cuda()
    t_graph = A.HipTrainer(model, batch_shape=tuple(x.shape), use_graph=True)
    t_eager = A.HipTrainer(twin, batch_shape=tuple(x.shape), use_graph=False)
    ar_ids = {id(p) for p in model.autoregressive_decoder.parameters()}
    assert ar_ids <= {id(p) for p in t_graph.params}
    before = [p.detach().clone() for p in model.autoregressive_decoder.parameters()]
    t_graph.capture()
    torch.cuda.manual_seed(77)
    a = t_graph.step(x).clone()
    torch.cuda.manual_seed(77)
    b = t_eager.step(x).clone()
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (a.tolist(), b.tolist())
    assert torch.equal(t_graph.pflat, t_eager.pflat)
    moved = [not torch.equal(p.detach(), q) for p, q in zip(model.autoregressive_decoder.parameters(), before)]
    assert all(moved), moved
    t_eager.close()
    torch.cuda.manual_seed(78)
    losses = [float(a[0])] + [float(t_graph.step(x)[0]) for _ in range(20)]
    print(f"[dad] train/loss/total over 21 captured steps: {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert losses[-1] < losses[0], losses
    assert t_graph.skipped_steps == 0
    t_graph.close()


def test_dad_graphed_step_gradients_equal_the_eager_route(A):
    """``enable_graphed_step()`` + ``loss.backward()`` against the eagerly issued ``nelbo`` + ``loss.backward()`` on a twin."""
    import copy
    model, g = load_model(A, "A")
    twin = copy.deepcopy(model)
    x = g["x"].cuda()
    batch = (x, torch.zeros(x.shape[0], dtype=torch.long, device="cuda"))
    model.enable_graphed_step()
    out = model.training_step(batch, 0)           # captures
    model.zero_grad(set_to_none=True)
    torch.cuda.manual_seed(91)
    out = model.training_step(batch, 0)
    out["loss"].backward()
    torch.cuda.manual_seed(91)
    ref = twin.training_step(batch, 0)
    ref["loss"].backward()
    assert torch.equal(out["loss"], ref["loss"])
    n, worst = 0, 0.0
    for (name, p), q in zip(model.named_parameters(), twin.parameters()):
        assert p.grad is not None and q.grad is not None, name
        # the same kernels on the same data in both routes; what may differ is the order in which partial sums of a weight gradient
        # are added (in-place slots against autograd's accumulation): a few fp32 roundings of the tensor's largest entry
        scale = max(float(q.grad.abs().max()), 1e-30)
        diff = float((p.grad - q.grad).abs().max())
        worst = max(worst, diff / scale)
        assert diff <= 1e-6 * scale, (name, diff, scale)
        n += name.startswith("autoregressive_decoder.")
    print(f"[dad] graphed vs eager gradients: worst relative difference {worst:.2e}")
    assert n > 0
    model.disable_graphed_step()
