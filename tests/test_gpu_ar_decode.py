"""GPU: key/value-cached incremental decoding -- ``otvae_ar_layer_step`` / ``otvae_ar_embed_step`` through ``functional``,
``AutoRegressive.decode_state`` / ``step`` and ``DAD.sample(cached=True)``.

Bound (the evidence rule of tests/test_gpu_dad.py::vs_truth): with the float64 truth T of a quantity,
|hip - T| <= max(1e-4 * max|T|, 1.5 * |ref32 - T|).  The truth is a stock ``nn.TransformerEncoder`` (post-norm, ReLU, ``batch_first``,
boolean upper-triangular mask) with an ``nn.Embedding``, learned positions, a LayerNorm and a Linear head, built here on the CPU, cast
to double and loaded from the model's ``state_dict`` (the keys are torch's); ``ref32`` is the same composition in float32.  Nothing in a
bound comes from the code under test.  The difference to the package's own full forward pass is printed for information only."""
import math

import pytest
import torch
import torch.nn as nn

from test_dad_host import build_dad

pytestmark = pytest.mark.gpu

TOL32, FACTOR = 1e-4, 1.5


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd as A_
    return A_


def vs_truth(name, got, ref32, truth):
    t = truth.detach().double().cpu()
    scale = max(t.abs().max().item(), 1e-30)
    e_hip = (got.detach().double().cpu() - t).abs().max().item() / scale
    e_ref = (ref32.detach().double().cpu() - t).abs().max().item() / scale
    tol = max(TOL32, FACTOR * e_ref)
    print(f"[ar] {name}: hip vs fp64 truth {e_hip:.3e}  reference fp32 vs truth {e_ref:.3e}  bound {tol:.3e}")
    assert math.isfinite(e_hip) and e_hip <= tol, (name, e_hip, e_ref, tol)


def causal_mask(T):
    return torch.triu(torch.ones(T, T, dtype=torch.bool), diagonal=1)


# ------------------------------------------------------------------------------------------------ 1. the layer kernel, raw
def stock_layer(D, H, F, seed, peaked=False):
    torch.manual_seed(seed)
    layer = nn.TransformerEncoderLayer(D, H, F, 0.0, batch_first=True).eval()
    with torch.no_grad():   # biases and LayerNorm affines away from their 0 / 1 initial values
        for p in (layer.self_attn.in_proj_bias, layer.self_attn.out_proj.bias, layer.norm1.bias, layer.norm2.bias):
            p.copy_(0.1 * torch.randn_like(p))
        for p in (layer.norm1.weight, layer.norm2.weight):
            p.copy_(1.0 + 0.1 * torch.randn_like(p))
        if peaked:          # scores spread over far more than 80: the soft-max is one-hot to fp32
            layer.self_attn.in_proj_weight[:2 * D] *= 12.0
    return layer


def kv_truth(layer, x, H):
    """[B, H, T, C] keys and values of the stock layer's in-projection"""
    B, T, D = x.shape
    qkv = x @ layer.self_attn.in_proj_weight.t() + layer.self_attn.in_proj_bias
    k, v = qkv[..., D:2 * D], qkv[..., 2 * D:]
    return (k.reshape(B, T, H, D // H).transpose(1, 2), v.reshape(B, T, H, D // H).transpose(1, 2)), qkv[..., :D]


def hip_layer_args(layer):
    from ot_vae_lightning_amd import functional as HF

    def lin(w):
        out = HF.new_linear_weight(w.shape[0], w.shape[1], device="cuda")
        out.copy_(w.detach())
        return out

    c = lambda t: t.detach().float().cuda().contiguous()
    at = layer.self_attn
    return dict(heads=at.num_heads, in_proj_weight=lin(at.in_proj_weight), in_proj_bias=c(at.in_proj_bias),
                out_proj_weight=lin(at.out_proj.weight), out_proj_bias=c(at.out_proj.bias), norm1_weight=c(layer.norm1.weight),
                norm1_bias=c(layer.norm1.bias), eps1=layer.norm1.eps, linear1_weight=lin(layer.linear1.weight),
                linear1_bias=c(layer.linear1.bias), linear2_weight=lin(layer.linear2.weight), linear2_bias=c(layer.linear2.bias),
                norm2_weight=c(layer.norm2.weight), norm2_bias=c(layer.norm2.bias), eps2=layer.norm2.eps)


LAYER_CASES = [(1, 16, 4, 32, 5, False), (17, 32, 2, 128, 9, False), (50, 128, 8, 512, 16, False), (3, 64, 4, 64, 70, False),
               (17, 32, 2, 128, 9, True)]


@pytest.mark.parametrize("B,D,H,F,T,peaked", LAYER_CASES)
def test_layer_step_vs_fp64_truth(A, B, D, H, F, T, peaked):
    """Every position through ``ar_layer_step`` against the full causal layer, row by row, and the caches against the true k / v.
    The caches are longer than T and NaN beyond the position being written: nothing past ``pos`` may be read."""
    from ot_vae_lightning_amd import functional as HF
    layer = stock_layer(D, H, F, seed=B * 100 + D, peaked=peaked)
    g = torch.Generator().manual_seed(D + T)
    x = torch.randn(B, T, D, generator=g)
    with torch.no_grad():
        y32 = layer(x, src_mask=causal_mask(T))
        (k32, v32), q32 = kv_truth(layer, x, H)
        l64 = stock_layer(D, H, F, seed=B * 100 + D, peaked=peaked).double()
        y64 = l64(x.double(), src_mask=causal_mask(T))
        (k64, v64), q64 = kv_truth(l64, x.double(), H)
    if peaked:
        s = torch.einsum("bthc,bshc->bhts", q64.reshape(B, T, H, -1), k64.transpose(1, 2)) / math.sqrt(D // H)
        last = s[:, :, T - 1, :]
        top2 = last.topk(2, -1).values
        assert float((top2[..., 0] - top2[..., 1]).max()) > 80.0, "the peaked case must hold a score that dominates by more than 80"
    args = hip_layer_args(layer)
    Tmax = T + 3
    kc = torch.full((B, H, Tmax, D // H), float("nan"), device="cuda")
    vc = torch.full_like(kc, float("nan"))
    xs = x.cuda()
    ys = []
    for pos in range(T):
        ys.append(HF.ar_layer_step(xs[:, pos].contiguous(), pos, kcache=kc, vcache=vc, **args))
        assert bool(torch.isnan(kc[:, :, pos + 1:]).all()) and bool(torch.isnan(vc[:, :, pos + 1:]).all())
    y = torch.stack(ys, 1)
    assert bool(torch.isfinite(y).all())
    tag = f"layer ({B},{D},{H},{F},{T}){' peaked' if peaked else ''}"
    vs_truth(f"{tag} y", y, y32, y64)
    vs_truth(f"{tag} kcache", kc[:, :, :T], k32, k64)
    vs_truth(f"{tag} vcache", vc[:, :, :T], v32, v64)
    # bit-reproducible: the last position again, on a copy of the caches
    again = HF.ar_layer_step(xs[:, T - 1].contiguous(), T - 1, kcache=kc.clone(), vcache=vc.clone(), **args)
    assert torch.equal(again, ys[-1])


def test_layer_step_refusals(A):
    from ot_vae_lightning_amd import functional as HF
    layer = stock_layer(32, 2, 64, seed=1)
    args = hip_layer_args(layer)
    x = torch.randn(3, 32).cuda()
    kc, vc = torch.zeros(3, 2, 4, 16).cuda(), torch.zeros(3, 2, 4, 16).cuda()
    HF.ar_layer_step(x, 3, kcache=kc, vcache=vc, **args)
    with pytest.raises(ValueError):                      # OTVAE_EINVAL: pos >= Tmax
        HF.ar_layer_step(x, 4, kcache=kc, vcache=vc, **args)
    with pytest.raises(ValueError):
        HF.ar_layer_step(x, 0, kcache=kc, vcache=vc[:, :, :3].contiguous(), **args)
    with pytest.raises(RuntimeError):
        HF.ar_layer_step(x.cpu(), 0, kcache=kc, vcache=vc, **args)
    with pytest.raises(RuntimeError):                    # no backward pass
        HF.ar_layer_step(x.clone().requires_grad_(True), 0, kcache=kc, vcache=vc, **args)
    # an unsupported width: OTVAE_EUNSUPPORTED -> NotImplementedError
    l24 = stock_layer(24, 2, 48, seed=2)
    with pytest.raises(NotImplementedError):
        HF.ar_layer_step(torch.randn(3, 24).cuda(), 0, kcache=torch.zeros(3, 2, 4, 12).cuda(), vcache=torch.zeros(3, 2, 4, 12).cuda(),
                         **hip_layer_args(l24))


# ------------------------------------------------------------------------------------------------ the stock composition of the model
class StockAR(nn.Module):
    """``AutoRegressive`` from stock torch modules, restricted to the input tokens (no token after them is visible under the mask)"""

    def __init__(self, K, T, D, H, F, depth):
        super().__init__()
        self.vocab_embed = nn.Embedding(K, D)
        self.pos = nn.Embedding(T, D)
        self.norm = nn.LayerNorm(D)
        self.transformer = nn.TransformerEncoder(nn.TransformerEncoderLayer(D, H, F, 0.0, batch_first=True), num_layers=depth,
                                                 enable_nested_tensor=False)
        self.head = nn.Linear(D, K)

    def forward(self, ids):
        T = ids.shape[1]
        x = self.norm(self.vocab_embed(ids) + self.pos.weight[:T])
        return self.head(self.transformer(x, mask=causal_mask(T)))


def stock_from(ar, K, T, D, H, F, depth, dtype):
    stock = StockAR(K, T, D, H, F, depth).to(dtype).eval()
    sd = {k: v.detach().cpu() for k, v in ar.state_dict().items()}
    mine = {"vocab_embed.weight": sd["vocab_embed.weight"], "pos.weight": sd["positional_embed.position_embeddings.weight"][:T],
            "norm.weight": sd["positional_embed.LayerNorm.weight"], "norm.bias": sd["positional_embed.LayerNorm.bias"],
            "head.weight": sd["head.weight"], "head.bias": sd["head.bias"]}
    mine.update({k: v for k, v in sd.items() if k.startswith("transformer.")})
    stock.load_state_dict({k: v.to(dtype) for k, v in mine.items()}, strict=True)
    return stock


def make_ar(A, K, T, D, H, F, depth, seed, n_embed_tokens=0, **extra):
    torch.manual_seed(seed)
    kw = dict(vocab_size=K, image_size=8, patch_size=4, dim=D, depth=depth, heads=H, mlp_dim=F, dropout=0.0, emb_dropout=0.0,
              n_embed_tokens=n_embed_tokens, n_input_tokens=T, output_tokens="input", patch_to_embed=False, embed_to_patch=False,
              causal_mask=True)
    kw.update(extra)
    ar = A.AutoRegressive(**kw)
    with torch.no_grad():   # every layer is a copy of one at construction: make them differ, and move the zero biases
        for p in ar.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return ar


AR_CASES = [("dad", 32, 16, 4, 32, 0), ("wide", 96, 128, 8, 512, 0), ("embed-token", 32, 16, 4, 32, 1)]


@pytest.mark.parametrize("tag,K,D,H,F,n_embed", AR_CASES)
def test_step_vs_full_forward_truth(A, tag, K, D, H, F, n_embed):
    T, depth, B = 12, 2, 19
    ar = make_ar(A, K, T, D, H, F, depth, seed=K + D, n_embed_tokens=n_embed)
    ids = torch.randint(0, K, (B, T), generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        l64 = stock_from(ar, K, T, D, H, F, depth, torch.float64)(ids)
        l32 = stock_from(ar, K, T, D, H, F, depth, torch.float32)(ids)
    ar = ar.cuda().eval()
    idc = ids.cuda()
    state = ar.decode_state(B)
    assert state.length == 0 and len(state.kcache) == depth and state.kcache[0].shape == (B, H, T, D // H)
    got = torch.stack([ar.step(idc[:, i], state) for i in range(T)], 1)
    assert state.length == T and got.shape == (B, T, K)
    vs_truth(f"step {tag}", got, l32, l64)
    with torch.no_grad():
        full = ar(idc)
    print(f"[ar] step {tag}: largest difference to the package's full forward {float((got - full).abs().max()):.3e} "
          f"(logits up to {float(full.abs().max()):.3e})")
    with pytest.raises(ValueError):
        ar.step(idc[:, 0], state)                                   # past max_tokens
    # reset + the same ids: the same logits bit for bit
    state.reset()
    again = torch.stack([ar.step(idc[:, i], state) for i in range(T)], 1)
    assert torch.equal(again, got)


def test_two_states_do_not_disturb_each_other(A):
    K, T, D, H, F, depth, B = 32, 7, 16, 4, 32, 2, 5
    ar = make_ar(A, K, T, D, H, F, depth, seed=8).cuda().eval()
    g = torch.Generator().manual_seed(4)
    a_ids, b_ids = torch.randint(0, K, (B, T), generator=g).cuda(), torch.randint(0, K, (B, T), generator=g).cuda()
    sa, sb = ar.decode_state(B), ar.decode_state(B)
    for s in (sa, sb):      # whatever the caches hold beyond the position is never read
        for t in s.kcache + s.vcache:
            t.fill_(float("nan"))
    alone = ar.decode_state(B, max_tokens=T)
    want_a = torch.stack([ar.step(a_ids[:, i], alone) for i in range(T)], 1)
    alone.reset()
    want_b = torch.stack([ar.step(b_ids[:, i], alone) for i in range(T)], 1)
    got_a, got_b = [], []
    for i in range(T):
        got_a.append(ar.step(a_ids[:, i], sa))
        got_b.append(ar.step(b_ids[:, i], sb))
    assert bool(torch.isfinite(want_a).all()) and not torch.equal(want_a, want_b)
    assert torch.equal(torch.stack(got_a, 1), want_a) and torch.equal(torch.stack(got_b, 1), want_b)
    short = ar.decode_state(B, max_tokens=2)
    ar.step(a_ids[:, 0], short), ar.step(a_ids[:, 1], short)
    with pytest.raises(ValueError):
        ar.step(a_ids[:, 2], short)


def test_decode_state_refusals_on_the_device(A):
    ar = make_ar(A, 32, 6, 24, 2, 48, 1, seed=5).cuda().eval()      # D = 24: outside the kernel's envelope
    state = ar.decode_state(3)
    with pytest.raises(NotImplementedError):
        ar.step(torch.zeros(3, dtype=torch.int64, device="cuda"), state)
    ok = make_ar(A, 32, 6, 16, 4, 32, 1, seed=5).cuda().eval()
    state = ok.decode_state(3)
    with pytest.raises(RuntimeError):
        ok.step(torch.zeros(3, dtype=torch.int64), state)            # a CPU tensor
    with pytest.raises(ValueError):
        ok.step(torch.zeros(4, dtype=torch.int64, device="cuda"), state)


# ------------------------------------------------------------------------------------------------ 5. DAD.sample(cached=True)
def build_dad16(A, K=32):
    v = dict(image_size=16, patch_size=4, dim=16, depth=1, heads=4, mlp_dim=32, channels=1, dropout=0.0, emb_dropout=0.)
    enc = A.ViT(n_embed_tokens=0, n_input_tokens=None, output_tokens="input", patch_to_embed=True, embed_to_patch=False, **v)
    dec = A.ViT(n_embed_tokens=None, n_input_tokens=enc.total_num_tokens, output_tokens="input", patch_to_embed=False,
                embed_to_patch=True, **v)
    ar = A.AutoRegressive(vocab_size=K, n_embed_tokens=0, n_input_tokens=enc.total_num_tokens, output_tokens="input",
                          patch_to_embed=False, embed_to_patch=False, causal_mask=True, **v)
    prior = A.CodebookPrior(latent_size=enc.out_size, embed_dims=(2,), loss=None, loss_coeff=1.0, annealing_steps=0,
                            mixture_cfg=dict(n_components=K, metric="euclidean", temperature=1.0, training_mode="gumbel-softmax",
                                             inference_mode="gumbel-softmax"), update_with_autograd=True)
    return A.DAD(encoder=enc, decoder=dec, autoregressive_decoder=ar, prior=prior, ce_coeff=1.0)


def inverse_cdf(logits64, u):
    cdf = torch.softmax(logits64, -1).cumsum(-1)
    return (cdf <= u.double().unsqueeze(-1)).sum(-1).clamp(max=logits64.shape[-1] - 1), cdf


def test_dad_sample_cached_end_to_end(A):
    torch.manual_seed(31)
    model = build_dad16(A)
    with torch.no_grad():   # logits with some spread: an untrained head is nearly uniform
        model.autoregressive_decoder.head.weight.mul_(4.0)
    B, T, K = 200, model.n_tokens, model.num_embeddings
    assert T == 16
    ar = model.autoregressive_decoder
    stock64 = stock_from(ar, K, T, 16, 4, 32, 1, torch.float64)
    stock32 = stock_from(ar, K, T, 16, 4, 32, 1, torch.float32)
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(32)
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
            img1 = model.sample(B, init_indices=init, noise=noise, cached=True)
            img2 = model.sample(B, init_indices=init.cuda(), noise=noise.cuda(), cached=True)
    finally:
        A.functional.codebook_gather = orig
    assert img1.shape == (B, 1, 16, 16) and torch.equal(img1, img2)
    ids = seen["ids"]
    assert torch.equal(ids[:, 0].cpu(), init[:, 0])
    with torch.no_grad():
        truth = stock64(ids.cpu())                                  # causal: position i does not see the later tokens
        ref32 = stock32(ids.cpu())
        latents = model.prior.unflatten_and_unpermute(model.prior.codebook_model.codebook.reshape(K, -1)[ids].transpose(0, 1))
        assert torch.equal(model.decode(latents), img1)
    skipped = skipped32 = total = 0
    for i in range(T - 1):
        want, cdf = inverse_cdf(truth[:, i], noise[:, i])
        near = ((cdf - noise[:, i].double().unsqueeze(-1)).abs().min(-1).values < 1e-4)
        ok = (ids[:, i + 1].cpu() == want) | near
        assert bool(ok.all()), (i, (~ok).nonzero().flatten().tolist())
        skipped, total = skipped + int(near.sum()), total + B
        skipped32 += int((inverse_cdf(ref32[:, i].double(), noise[:, i])[0] != want).sum())
    print(f"[ar] cached sample: {skipped} of {total} positions within 1e-4 of a CDF boundary were left out "
          f"(the float32 composition disagrees with the truth at {skipped32})")
    assert skipped <= 0.05 * total
    # drawn on the device: valid images, new ones on every call
    with torch.no_grad():
        a, b = model.sample(8, cached=True), model.sample(8, cached=True)
    assert a.shape == (8, 1, 16, 16) and bool(torch.isfinite(a).all()) and not torch.equal(a, b)
    # an ineligible decoder raises instead of taking the uncached route
    model.autoregressive_decoder.causal_mask = False
    with pytest.raises(NotImplementedError):
        model.sample(4, cached=True)
    model.autoregressive_decoder.causal_mask = True


def test_cached_and_uncached_samples_agree_on_build_dad(A):
    """information: the two routes of the recorded architecture on the same draws (they may differ where a uniform sits within
    rounding of a CDF boundary, which the end-to-end tests bound against the truth; here only a count is printed) -- and the
    assertion that the cached route yields valid, reproducible ids."""
    torch.manual_seed(21)
    model = build_dad().cuda().eval()
    B, T, K = 64, model.n_tokens, model.num_embeddings
    g = torch.Generator().manual_seed(22)
    init, noise = torch.randint(0, K, (B, T), generator=g), torch.rand(B, T - 1, generator=g)
    with torch.no_grad():
        a = model.sample(B, init_indices=init, noise=noise, cached=True)
        b = model.sample(B, init_indices=init, noise=noise, cached=True)
        c = model.sample(B, init_indices=init, noise=noise)
    assert torch.equal(a, b) and a.shape == c.shape and bool(torch.isfinite(a).all())
    print(f"[ar] build_dad: cached and uncached images differ in {int((a != c).flatten(1).any(1).sum())} of {B} samples")


# ------------------------------------------------------------------------------------------------ 6. launch budget
def test_step_launch_budget_and_no_aten_kernels(A):
    from torch.profiler import ProfilerActivity, profile
    from ot_vae_lightning_amd import functional as HF
    K, T, D, H, F, depth, B = 96, 8, 128, 8, 512, 2, 40
    ar = make_ar(A, K, T, D, H, F, depth, seed=6).cuda().eval()
    ids = torch.randint(0, K, (B, T), generator=torch.Generator().manual_seed(7)).cuda()
    u = torch.rand(B, generator=torch.Generator().manual_seed(8)).cuda()
    state = ar.decode_state(B)

    def run(i):
        logits = ar.step(ids[:, i], state)
        HF.categorical_sample_(ids, i + 1, logits.unsqueeze(1), 0, u=u)

    run(0)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        run(1)
        torch.cuda.synchronize()
    kernels = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    print(f"[ar] one step + one draw on a depth-{depth} decoder: {len(kernels)} kernels: {kernels}")
    assert kernels, "the profiler saw no device kernels"
    assert len(kernels) <= depth + 3, kernels
    assert sum("ar_layer_step" in n for n in kernels) == depth and sum("ar_embed_step" in n for n in kernels) == 1
    foreign = [n for n in kernels if "at::" in n or "Cijk" in n or "elementwise" in n or "Memcpy" in n or "Memset" in n]
    assert not foreign, foreign
