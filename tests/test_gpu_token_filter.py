"""GPU: temperature, top-k and top-p (nucleus) filtering in the token sampler -- ``otvae_filtered_sample`` through
``HF.categorical_sample_`` against a float64 reference of its rules formed here, and ``DAD.sample`` with the new arguments against
loops the tests run themselves.

The rules (include/otvae.h): entries ordered by (logit descending, index ascending); weights exp((l - max) / temperature) in fp64;
top-k keeps the first min(k, K) of the order; top-p keeps a survivor iff the mass of the survivors before it over their total is < p;
the draw is the inverse CDF of u over the kept entries in index order.  The scalars reach the kernel as float32, so the reference
uses their float32 values.

Nothing here is a tolerance.  Indices and kept counts must match exactly, on inputs whose answer does not depend on the last bits
of a sum, which the tests assert on the reference itself: every top-p comparison of every row is at least 1e-10 away from p (fp64
summation order moves these ratios by about 1e-12), and u is the midpoint of a CDF interval at least 1e-3 wide.

One case is not run as listed: at K = 1 the setting top_k = K - 1 would be top_k = 0, which is no legal value; it runs as
top_k = 1."""
import numpy as np
import pytest
import torch

from test_dad_host import build_dad

pytestmark = pytest.mark.gpu

B, T, POS, COL = 96, 5, 1, 2
KS = [1, 2, 33, 257, 1000, 8192, 16384]


@pytest.fixture(scope="module")
def HF():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd  # noqa: F401
    from ot_vae_lightning_amd import functional
    return functional


def f32(x):
    return float(np.float32(x))


class Row:
    """float64 reference for one [B, K] block of logits; the sort is done once and shared by every setting"""

    def __init__(self, logits):
        self.l = logits.double()
        self.K = logits.shape[-1]
        self.order = torch.sort(self.l, dim=-1, descending=True, stable=True).indices     # ties: the lower index first
        self.m = self.l.max(-1, keepdim=True).values

    def filtered(self, tau, k, p):
        """kept mask [B, K], kept count [B], normalised CDF of the kept entries in index order [B, K], top-p margin"""
        K = self.K
        w = torch.exp((self.l - self.m) / f32(tau))
        ws = w.gather(1, self.order)
        kk = K if k is None else min(k, K)
        keep = (torch.arange(K) < kk).expand_as(ws).clone()
        margin = float("inf")
        if p is not None and f32(p) < 1.0:
            surv = ws[:, :kk]
            cum = surv.cumsum(-1)
            before = torch.cat([torch.zeros(len(ws), 1, dtype=torch.float64), cum[:, :-1]], 1)
            ratio = before / cum[:, -1:]
            keep[:, :kk] &= ratio < f32(p)
            margin = float((ratio - f32(p)).abs().min())
        mask = torch.zeros_like(keep).scatter_(1, self.order, keep)
        cdf = (w * mask).cumsum(-1)
        return mask, keep.sum(-1), cdf / cdf[:, -1:], margin


def midpoints(mask, cdf, g):
    """per row one kept entry whose CDF interval is at least 1e-3 wide, and the midpoint of that interval"""
    lo = torch.cat([torch.zeros(len(cdf), 1, dtype=torch.float64), cdf[:, :-1]], 1)
    wide = ((cdf - lo) >= 1e-3) & mask
    assert bool(wide.any(-1).all()), "a row without a wide interval"
    pick = torch.multinomial(wide.float(), 1, generator=g).squeeze(1)
    return pick, (0.5 * (lo + cdf)).gather(1, pick[:, None]).squeeze(1).float()


def draw(HF, logits_gpu, ids, col, u=None, key=None, **kw):
    kept = torch.full((ids.shape[0],), -1, dtype=torch.int32, device="cuda")
    out = HF.categorical_sample_(ids, col, logits_gpu, POS, u=None if u is None else u.cuda(), key=key, kept=kept, **kw)
    assert out is ids
    return ids[:, col].cpu(), kept.cpu()


def settings(K):
    return [(1.0, None, 0.9), (0.7, 5, None), (1.3, 50, 0.5), (1.0, max(K - 1, 1), 0.999), (2.0, None, 1e-4)]


def make_logits(K, quantised):
    g = torch.Generator().manual_seed(K + 1 if quantised else K)
    logits = 3.0 * torch.randn(B, 3, K, generator=g)
    return (torch.round(2.0 * logits) / 2.0 if quantised else logits), g


def check_case(HF, logits, g, cases):
    """every id and every kept count of every setting; the untouched columns; u = 0 and u just below 1"""
    K = logits.shape[-1]
    ref = Row(logits[:, POS])
    dev = logits.cuda()
    ids0 = torch.randint(0, K, (logits.shape[0], T), generator=g)
    others = [c for c in range(T) if c != COL]
    for tau, k, p in cases:
        mask, count, cdf, margin = ref.filtered(tau, k, p)
        print(f"[filter] K = {K} (tau, k, p) = ({tau}, {k}, {p}): kept {int(count.min())} .. {int(count.max())}, top-p margin {margin:.2e}")
        assert margin >= 1e-10, (K, tau, k, p, margin)
        pick, u = midpoints(mask, cdf, g)
        ids = ids0.clone().cuda()
        got, kept = draw(HF, dev, ids, COL, u=u, temperature=tau, top_k=k, top_p=p)
        assert torch.equal(kept.long(), count), (K, tau, k, p, (kept.long() != count).nonzero().flatten().tolist())
        assert torch.equal(got, pick), (K, tau, k, p, (got != pick).nonzero().flatten().tolist())
        assert torch.equal(ids[:, others].cpu(), ids0[:, others])
        got, _ = draw(HF, dev, ids, COL, u=torch.zeros(len(u)), temperature=tau, top_k=k, top_p=p)
        # u = 0 yields the first kept entry of POSITIVE weight; here that is the lowest kept index, asserted: no kept weight is 0
        lowest = mask.long().argmax(-1)
        assert bool((cdf.gather(1, lowest[:, None]) > 0).all())
        assert torch.equal(got, lowest), (K, tau, k, p)
        got, _ = draw(HF, dev, ids, COL, u=torch.full((len(u),), f32(np.nextafter(np.float32(1), np.float32(0)))), temperature=tau,
                      top_k=k, top_p=p)
        assert bool(mask.gather(1, got[:, None]).all()), (K, tau, k, p)
    return ref, dev


@pytest.mark.parametrize("K", KS)
def test_filtered_draw_is_exact(HF, K):
    logits, g = make_logits(K, quantised=False)
    ref, dev = check_case(HF, logits, g, settings(K))
    # filters off and temperature 1 through the new entry: otvae_categorical_sample's ids bit for bit, for a u and for a key
    u = torch.rand(B, generator=g).cuda()
    key = HF.new_dropout_key("cuda", seed=5)
    a, b, c, d = (torch.zeros(B, T, dtype=torch.int64, device="cuda") for _ in range(4))
    HF.categorical_sample_(a, COL, dev, POS, u=u)
    got, kept = draw(HF, dev, b, COL, u=u, temperature=1.0, top_k=None, top_p=1.0)
    assert torch.equal(a, b) and bool((kept == K).all())
    HF.categorical_sample_(c, 3, dev, POS, key=key)
    draw(HF, dev, d, 3, key=key, top_k=K)          # top_k >= K is the same as off
    assert torch.equal(c, d)
    # a non-contiguous view of the logits
    tau, k, p = settings(K)[2]
    mask, count, cdf, _ = ref.filtered(tau, k, p)
    pick, um = midpoints(mask, cdf, g)
    view = dev.transpose(0, 1).contiguous().transpose(0, 1)
    assert not view.is_contiguous() or K == 1
    got, kept = draw(HF, view, a, 0, u=um, temperature=tau, top_k=k, top_p=p)
    assert torch.equal(got, pick) and torch.equal(kept.long(), count)


@pytest.mark.parametrize("K", KS)
def test_filtered_draw_with_tied_logits(HF, K):
    """logits quantised to halves: ties at the k-th value are certain, and so are tied maxima"""
    logits, g = make_logits(K, quantised=True)
    cases = [s for s in settings(K) if not (K == 2 and s[2] == 0.5)]     # two tied logits put the mass exactly on p = 0.5
    ref, dev = check_case(HF, logits, g, cases)
    row = logits[:, POS]
    if K >= 33:
        kth = row.sort(-1, descending=True).values[:, 4:6]
        print(f"[filter] K = {K}: {int((kth[:, 0] == kth[:, 1]).sum())} of {B} rows tie at the 5th value, "
              f"{int(((row == row.max(-1, keepdim=True).values).sum(-1) > 1).sum())} at the maximum")
        assert bool((kth[:, 0] == kth[:, 1]).any())
        assert bool(((row == row.max(-1, keepdim=True).values).sum(-1) > 1).any())
    # greedy: temperature 0, and top_k = 1 at any temperature, are the first entry of the order
    first = ref.order[:, 0]
    ids = torch.zeros(B, T, dtype=torch.int64, device="cuda")
    u = torch.rand(B, generator=g)
    for kw in (dict(temperature=0.0), dict(top_k=1), dict(temperature=0.3, top_k=1, top_p=0.5), dict(temperature=0.0, top_k=7, top_p=0.2)):
        got, kept = draw(HF, dev, ids, COL, u=u, **kw)
        assert torch.equal(got, first) and bool((kept == 1).all()), kw


def test_filtered_draw_with_masked_logits(HF):
    """-inf entries weigh nothing and are legal"""
    K = 1000
    g = torch.Generator().manual_seed(7)
    logits = 3.0 * torch.randn(B, 3, K, generator=g)
    dead = torch.rand(B, 3, K, generator=g) < 0.3
    dead[..., 0] = False
    logits[dead] = -float("inf")
    check_case(HF, logits, g, [(1.0, 40, 0.8)])


def test_device_drawn_uniforms_under_top_k(HF):
    K = 1000
    logits, g = make_logits(K, quantised=True)
    dev = logits.cuda()
    top5, _, _, _ = Row(logits[:, POS]).filtered(1.0, 5, None)
    key = HF.new_dropout_key("cuda", seed=123)
    a, b, c = (torch.zeros(B, T, dtype=torch.int64, device="cuda") for _ in range(3))
    ga, _ = draw(HF, dev, a, 3, key=key, top_k=5)
    draw(HF, dev, b, 3, key=key, top_k=5)
    key[1:].add_(1)
    gc, _ = draw(HF, dev, c, 3, key=key, top_k=5)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert bool(top5.gather(1, ga[:, None]).all()) and bool(top5.gather(1, gc[:, None]).all())


def test_envelope_and_single_row(HF):
    """a row of 16385 logits cannot be sorted in LDS: top-k / top-p refuse it, temperature alone and greedy decoding take it"""
    K, n = 16385, 8
    g = torch.Generator().manual_seed(K)
    logits = 3.0 * torch.randn(n, 3, K, generator=g)
    dev = logits.cuda()
    ids = torch.zeros(n, T, dtype=torch.int64, device="cuda")
    with pytest.raises(NotImplementedError, match="16385"):
        HF.categorical_sample_(ids, COL, dev, POS, u=torch.zeros(n).cuda(), top_k=5)
    with pytest.raises(NotImplementedError, match="16384"):
        HF.categorical_sample_(ids, COL, dev, POS, u=torch.zeros(n).cuda(), top_p=0.5)
    ref = Row(logits[:, POS])
    mask, count, cdf, _ = ref.filtered(0.7, None, None)
    pick, u = midpoints(mask, cdf, g)
    got, kept = draw(HF, dev, ids, COL, u=u, temperature=0.7)
    assert torch.equal(got, pick) and bool((kept == K).all())
    got, kept = draw(HF, dev, ids, COL, u=u, temperature=0.0)
    assert torch.equal(got, ref.order[:, 0]) and bool((kept == 1).all())
    # B = 1
    one = logits[:1, :, :1000].contiguous()
    mask, count, cdf, margin = Row(one[:, POS]).filtered(0.9, 20, 0.7)
    assert margin >= 1e-10
    pick, u = midpoints(mask, cdf, g)
    got, kept = draw(HF, one.cuda(), torch.zeros(1, T, dtype=torch.int64, device="cuda"), COL, u=u, temperature=0.9, top_k=20, top_p=0.7)
    assert torch.equal(got, pick) and torch.equal(kept.long(), count)


# ------------------------------------------------------------------------------------------------ DAD.sample
@pytest.fixture(scope="module")
def dad(HF):
    torch.manual_seed(21)
    model = build_dad().cuda().eval()
    g = torch.Generator().manual_seed(22)
    n, Tm, K = 16, model.n_tokens, model.num_embeddings
    return model, torch.randint(0, K, (n, Tm), generator=g).cuda(), torch.rand(n, Tm - 1, generator=g).cuda()


def images_of(HF, model, ids):
    codebook = model.prior.codebook_model.codebook
    latents = HF.codebook_gather(codebook.reshape(-1, codebook.shape[-1]).float(), ids).type_as(codebook)
    return model.decode(model.prior.unflatten_and_unpermute(latents.transpose(0, 1)))


def own_loop(model, init, cached, choose):
    """the sampling loop, run by the test: ``choose(i, logits [B, K])`` returns the ids of position i + 1"""
    ar, Tm = model.autoregressive_decoder, model.n_tokens
    ids = init.clone()
    state = ar.decode_state(len(ids), Tm) if cached else None
    for i in range(Tm - 1):
        logits = ar.step(ids[:, i], state) if cached else ar(ids)[:, i]
        ids[:, i + 1] = choose(i, logits.contiguous())
    return ids


def test_sample_defaults_are_todays_draws(HF, dad):
    model, init, noise = dad
    with torch.no_grad():
        for cached in (False, True):
            a = model.sample(len(init), init_indices=init, noise=noise, cached=cached)
            b = model.sample(len(init), init_indices=init, noise=noise, cached=cached, temperature=1.0, top_k=None, top_p=None)
            assert torch.equal(a, b)


@pytest.mark.parametrize("cached", [False, True])
def test_sample_greedy(HF, dad, cached):
    model, init, noise = dad

    def argmax(i, logits):
        top2 = logits.topk(2, -1).values
        assert bool((top2[:, 0] > top2[:, 1]).all()), "a tied maximum"
        return torch.argmax(logits, -1)

    with torch.no_grad():
        want = images_of(HF, model, own_loop(model, init, cached, argmax))
        a = model.sample(len(init), init_indices=init, noise=noise, cached=cached, top_k=1)
        b = model.sample(len(init), init_indices=init, cached=cached, temperature=0)
    assert torch.equal(a, b) and torch.equal(a, want)


@pytest.mark.parametrize("cached", [False, True])
def test_sample_filtered(HF, dad, cached):
    model, init, noise = dad
    kw = dict(top_k=4, top_p=0.9, temperature=0.8)

    def choose(i, logits):
        ids = torch.zeros(len(logits), 1, dtype=torch.int64, device="cuda")
        HF.categorical_sample_(ids, 0, logits.unsqueeze(1), 0, u=noise[:, i].contiguous(), **kw)
        fourth = logits.topk(4, -1).values[:, 3]
        assert bool((logits.gather(1, ids).squeeze(1) >= fourth).all())
        return ids[:, 0]

    with torch.no_grad():
        want = images_of(HF, model, own_loop(model, init, cached, choose))
        got = model.sample(len(init), init_indices=init, noise=noise, cached=cached, **kw)
        plain = model.sample(len(init), init_indices=init, noise=noise, cached=cached)
    assert torch.equal(got, want) and not torch.equal(got, plain)
