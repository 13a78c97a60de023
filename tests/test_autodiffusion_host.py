"""CPU: the host side of the class / time conditioned ``AutoEncoder``, ``GaussianFourierProjection`` and ``AutoDiffusion`` --
construction, state-dict layout against the reference's (tests/golden/autodiffusion.npz), argument checks, the sampling schedule and
the beta weighting of the prior loss.  Nothing here launches a kernel."""
import inspect
import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import load_golden

import ot_vae_lightning_amd as A

GOLD = load_golden("autodiffusion.npz")


def _ae(**kw):
    cfg = dict(capacity=4, num_classes=10, time_embed_dim=8, residual="add", down_up_sample=True)
    cfg.update(kw)
    return A.AutoEncoder(1, 4, 8, 2, **cfg)


# ---- construction --------------------------------------------------------------------------------------------------------------------
def test_conditioned_autoencoder_constructs_with_the_reference_state_dict():
    ae = _ae()
    state = ae.state_dict()
    names = [str(n) for n in GOLD["ae/names"]]
    assert list(state.keys()) == names
    for n in names:
        assert tuple(state[n].shape) == GOLD[f"ae/state/{n}"].shape, n
    for leaf in ("weight", "bias"):
        a, b = state[f"time_embed.proj.2.{leaf}"], state[f"time_embed.proj.4.{leaf}"]
        assert a.data_ptr() == b.data_ptr() and a.shape == b.shape
    assert ae.time_embed.proj[2] is ae.time_embed.proj[4]
    assert not ae.time_embed.weight.requires_grad and ae.time_embed.weight.shape == (1, 4)
    ae.load_state_dict({n: torch.from_numpy(GOLD[f"ae/state/{n}"]) for n in names})
    # (module order: class_embed, time_embed, encoder, decoder)
    assert [n for n, _ in ae.named_children()] == ["class_embed", "time_embed", "encoder", "decoder"]


def test_class_embedding_width_and_additional_embed():
    ae10, ae100 = _ae(num_classes=10), _ae(num_classes=100)
    assert ae10.class_embed.embedding_dim == 64 and ae100.class_embed.embedding_dim == 128
    first = next(m for m in ae10.encoder.modules() if isinstance(m, A.ConvLayer))
    assert first._embed_proj_scale.in_features == 64 + 8
    only_time = _ae(num_classes=None)
    assert only_time.class_embed is None
    assert next(m for m in only_time.decoder.modules() if isinstance(m, A.ConvLayer))._embed_proj_scale.in_features == 8
    only_class = _ae(time_embed_dim=None)
    assert only_class.time_embed is None
    assert next(m for m in only_class.decoder.modules() if isinstance(m, A.ConvLayer))._embed_proj_scale.in_features == 64


def test_unconditioned_autoencoder_is_unchanged():
    ae = A.AutoEncoder(1, 4, 8, 2, capacity=4, down_up_sample=True)
    assert ae.class_embed is None and ae.time_embed is None
    assert all(m._embed_proj_scale is None for m in ae.modules() if isinstance(m, A.ConvLayer))
    assert not any(k.startswith(("class_embed", "time_embed")) for k in ae.state_dict())
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert ae.embed(None, None) is None
    assert not w


def test_same_seed_gives_the_reference_initial_weights():
    """creation order and RNG draws as the reference: the recorded state was constructed under this seed"""
    torch.manual_seed(4321)
    gfp = A.GaussianFourierProjection(8, 8)
    for n in [str(n) for n in GOLD["gfp/names"]]:
        assert torch.equal(gfp.state_dict()[n], torch.from_numpy(GOLD[f"gfp/state/{n}"])), n


# ---- embed() -------------------------------------------------------------------------------------------------------------------------
class _StubTime(nn.Module):
    def forward(self, t):
        return torch.stack([t, 2 * t, 3 * t], dim=1)


def test_embed_warnings_errors_and_concatenation_order():
    plain = A.AutoEncoder(1, 4, 8, 2, capacity=4, down_up_sample=True)
    with pytest.warns(UserWarning, match="`labels` but `self.class_embed` is None"):
        assert plain.embed(labels=torch.zeros(2, dtype=torch.long)) is None
    with pytest.warns(UserWarning, match="`time` but `self.time_embed` is None"):
        assert plain.embed(time=torch.zeros(2)) is None
    ae = _ae()
    ae.time_embed = _StubTime()
    labels, time = torch.tensor([3, 0, 9]), torch.tensor([0.0, 0.5, 1.0])
    with pytest.raises(ValueError, match="labels"):
        ae.embed(None, time)
    with pytest.raises(ValueError, match="time"):
        ae.embed(labels, None)
    e = ae.embed(labels, time)
    assert e.shape == (3, 64 + 3)
    assert torch.equal(e[:, :64], ae.class_embed(labels)) and torch.equal(e[:, 64:], ae.time_embed(time))
    only_class = _ae(time_embed_dim=None)
    assert torch.equal(only_class.embed(labels), only_class.class_embed(labels))
    only_time = _ae(num_classes=None)
    only_time.time_embed = _StubTime()
    assert torch.equal(only_time.embed(time=time), only_time.time_embed(time))


def test_fourier_projection_refuses_bad_inputs():
    gfp = A.GaussianFourierProjection(8, 8)
    with pytest.raises(ValueError, match="1-dimensional"):
        gfp(torch.zeros(2, 1))
    with pytest.raises(ValueError, match=r"range \[0,1\]"):
        gfp(torch.tensor([0.5, 1.5]))
    with pytest.raises(ValueError, match=r"range \[0,1\]"):
        gfp(torch.tensor([-0.1, 0.5]))
    with pytest.raises(RuntimeError):   # a valid host tensor gets as far as the kernel's gate: there is no CPU path
        gfp(torch.tensor([0.0, 1.0]))
    assert A.GaussianFourierProjection(8, 8, trainable=True).weight.requires_grad


# ---- AutoDiffusion -------------------------------------------------------------------------------------------------------------------
def test_exports_and_signature():
    assert issubclass(A.AutoDiffusion, A.VAE) and A.AutoDiffusion.n_steps == 10
    from ot_vae_lightning_amd.model import AutoDiffusion
    assert AutoDiffusion is A.AutoDiffusion
    params = inspect.signature(A.AutoDiffusion.sample).parameters
    assert list(params) == ["self", "batch_size", "steps", "improved_algorithm", "latents", "noise", "kwargs"]
    assert params["steps"].default is None and params["improved_algorithm"].default is False
    assert params["latents"].kind is params["noise"].kind is inspect.Parameter.KEYWORD_ONLY
    assert params["latents"].default is None and params["noise"].default is None
    assert params["kwargs"].kind is inspect.Parameter.VAR_KEYWORD


class _StubAE(nn.Module):
    """pure torch: encode / decode record (name, time) and are cheap affine maps"""
    latent_size = torch.Size([2, 1, 1])

    def __init__(self, log):
        super().__init__()
        self.w = nn.Parameter(torch.tensor(0.5))
        self.log = log

    def encode(self, x, time=None):
        self.log.append(("encode", [round(float(v), 6) for v in time]))
        return x * self.w + time.reshape(-1, 1, 1, 1)

    def decode(self, z, time=None):
        self.log.append(("decode", [round(float(v), 6) for v in time]))
        return z * 2.0 - time.reshape(-1, 1, 1, 1)


class _StubPrior(nn.Module):
    """z = x + time * eps; records the time of every call and the eps it was handed"""

    def __init__(self, log):
        super().__init__()
        self.log, self.eps_seen = log, []

    def out_size(self, size):
        return torch.Size(size)

    def sample(self, shape, device, time=None):
        self.log.append(("prior.sample", [round(float(v), 6) for v in time]))
        return torch.full(shape, 0.25, device=device)

    def forward(self, x, step, time=None, eps=None):
        self.log.append(("prior", [round(float(v), 6) for v in time]))
        self.eps_seen.append(eps)
        if eps is None:
            eps = torch.zeros_like(x)
        return x + time.reshape(-1, 1, 1, 1) * eps, torch.zeros(x.shape[0]), {}


def _stub_model(expansion=1):
    log = []
    model = A.AutoDiffusion(autoencoder=_StubAE(log), prior=_StubPrior(log), expansion=expansion)
    return model, log


@pytest.mark.parametrize("improved", [False, True])
def test_sampling_schedule(improved):
    B, n = 3, A.AutoDiffusion.n_steps
    model, log = _stub_model()
    n_calls = n * (2 if improved else 1)
    noise = torch.arange(n_calls * B * 2, dtype=torch.float32).reshape(n_calls, B, 2, 1, 1)
    out = model.sample(B, improved_algorithm=improved, noise=noise)
    assert out.shape == (B, 2, 1, 1)
    # the exact sequence of calls and the time each one received
    s_values = [round(float(s), 6) for s in np.linspace(1, 1 / n, n)]
    want = [("prior.sample", [1.0] * B)]
    for s in s_values:
        want.append(("decode", [s] * B))
        lo = round(s - 1 / n, 6)
        for t in ([lo, s] if improved else [lo]):
            want += [("encode", [t] * B), ("prior", [t] * B)]
    assert [(name, [round(v, 5) for v in ts]) for name, ts in log] == [(name, [round(v, 5) for v in ts]) for name, ts in want]
    # the rows of `noise` are consumed in order, one per encode call
    seen = model.prior.eps_seen
    assert len(seen) == n_calls and all(torch.equal(e, noise[k]) for k, e in enumerate(seen))
    # a hand-written loop over the same stubs
    xs = torch.full((B, 2, 1, 1), 0.25)
    ae, k = model.autoencoder, 0
    quiet = []
    ae.log = model.prior.log = quiet
    with torch.no_grad():
        for s in np.linspace(1, 1 / n, n):
            t_hi, t_lo = torch.ones(B) * s, torch.ones(B) * (s - 1 / n)
            x_hat = ae.decode(xs, t_hi)
            if improved:
                a = ae.encode(x_hat, t_lo) + t_lo.reshape(-1, 1, 1, 1) * noise[k]
                b = ae.encode(x_hat, t_hi) + t_hi.reshape(-1, 1, 1, 1) * noise[k + 1]
                xs, k = xs - (a - b), k + 2
            else:
                xs, k = ae.encode(x_hat, t_lo) + t_lo.reshape(-1, 1, 1, 1) * noise[k], k + 1
    assert torch.equal(out, x_hat)


@pytest.mark.parametrize("improved", [False, True])
def test_sample_steps_latents_and_generation(improved):
    B = 2
    model, log = _stub_model()
    assert len(model.sample(B, steps=[0, 4, 9], improved_algorithm=improved)) == 3
    assert len(model.sample(B, steps=[], improved_algorithm=improved)) == 0
    assert len(model.sample(B, steps=[3, 10, 11], improved_algorithm=improved)) == 1   # iterations run 0 .. n_steps - 1
    # `latents` replaces the prior's draw and is left as it was
    del log[:]
    lat = torch.full((B, 2, 1, 1), 2.0)
    model.sample(B, improved_algorithm=improved, latents=lat, time=torch.zeros(B))
    assert log[0][0] == "decode" and torch.equal(lat, torch.full((B, 2, 1, 1), 2.0))
    batch = {"samples": torch.zeros(B, 2, 1, 1), "target": torch.zeros(B, 2, 1, 1), "kwargs": {"time": torch.rand(B)}}
    gen = model.generation_improved(batch) if improved else model.generation(batch)
    assert len(gen) == 9 and all(g.shape == (B, 2, 1, 1) for g in gen)
    rec = model.reconstruction(batch)
    assert len(rec) == 11 and rec[-1] is batch["target"]
    n_calls = model.n_steps * (2 if improved else 1)
    with pytest.raises(ValueError, match="noise"):
        model.sample(B, improved_algorithm=improved, noise=torch.zeros(n_calls + 1, B, 2, 1, 1))
    with pytest.raises(ValueError, match="latents"):
        model.sample(B, improved_algorithm=improved, latents=torch.zeros(B + 1, 2, 1, 1))


def test_batch_preprocess_draws_a_time_per_sample():
    model, _ = _stub_model()
    pb = model.batch_preprocess((torch.zeros(5, 2, 1, 1), torch.zeros(5, dtype=torch.long)))
    t = pb["kwargs"]["time"]
    assert t.shape == (5,) and bool((t >= 0).all()) and bool((t < 1).all()) and "labels" not in pb["kwargs"]


@pytest.mark.parametrize("expansion", [1, 2])
def test_beta_weighting_of_the_prior_loss(expansion):
    model, _ = _stub_model(expansion)
    time = torch.tensor([0.0, 0.5, 1.0])
    prior = torch.arange(1, 3 * expansion + 1, dtype=torch.float32)
    beta = 0.5 * np.tanh(10 * (np.array([0.0, 0.5, 1.0]) - 0.5)) + 0.5
    want = torch.from_numpy(np.tile(beta, expansion)).float() * prior     # `time` replicated like the latents: [t0 t1 t2 t0 t1 t2]
    got = model.per_sample_prior_loss(prior, {}, time=time, eps=None)
    assert got.shape == prior.shape and torch.allclose(got, want, rtol=1e-6, atol=1e-7)
    assert abs(float(got[1]) - 0.5 * float(prior[1])) < 1e-7 and float(got[0]) < 1e-4 * float(prior[0])
    assert torch.allclose(model.prior_loss(prior, {}, time=time), want.mean(), rtol=1e-6, atol=1e-7)
    # VAE.nelbo hands the batch's keywords to per_sample_prior_loss; VAE itself ignores them
    assert "kwargs" in inspect.signature(A.VAE.per_sample_prior_loss).parameters
    assert torch.equal(A.VAE.per_sample_prior_loss(model, prior, {}, time=time), prior)
