"""Records ``tests/golden/dad.npz`` from the reference's own ``DAD`` (model/discrete_auto_diffuser.py) on the CPU.

    python tools/gen_dad_golden.py            # needs the reference checkout (OTVAE_REFERENCE_ROOT), build container only

Two small configurations, each run in float32 (the reference as it is) and in float64 (the truth the GPU tests measure both sides
against) on the same weights, batch and random draws:

    A  the ViT of the reference's tests/test_dad.py shrunk to 8x8 images (patch 4, dim 16, depth 1, no dropout), K = 32, euclidean,
       'gumbel-softmax' assignments, loss=None, update_with_autograd=True
    B  after configs/dad/defaults.yaml: cosine similarity, loss='first_kl', the soft 'mean' mode, loss_coeff = ce_coeff = 1e-3
       (the codebook trained by autograd here too: its k-means initialisation draws from the host generator)

The random draws the prior consumes are made here and recorded: the Gumbel noise of ``F.gumbel_softmax`` (A) and one uniform per
token for ``Categorical.sample`` -- the index is the inverse CDF of that uniform under the assignment probabilities, taken in
float64; every uniform is kept at least MARGIN away from a CDF boundary so that the recorded indices do not hinge on rounding.
Data only: arrays and two lists of names."""
import os
import sys
import types

import numpy as np
import torch
import torch.distributions as D
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import as R  # noqa: E402

MARGIN = 1e-3
OUT = os.path.join(ROOT, "tests", "golden", "dad.npz")


def _reference():
    R.install()
    stand_in = types.ModuleType("ot_vae_lightning.data.torchvision_datamodule")
    stand_in.TorchvisionDatamodule = type("TorchvisionDatamodule", (), {})
    sys.modules[stand_in.__name__] = stand_in
    return R.ref("model.discrete_auto_diffuser").DAD, R.ref("prior.codebook").CodebookPrior, R.ref("networks.vit")


def _build(cfg):
    DAD, CodebookPrior, vit = _reference()
    v = dict(image_size=8, patch_size=4, dim=16, depth=cfg["depth"], heads=4, mlp_dim=32, channels=cfg["channels"], dropout=0.,
             emb_dropout=0.)
    enc = vit.ViT(n_embed_tokens=0, n_input_tokens=None, output_tokens="input", patch_to_embed=True, embed_to_patch=False, **v)
    dec = vit.ViT(n_embed_tokens=None, n_input_tokens=enc.total_num_tokens, output_tokens="input", patch_to_embed=False,
                  embed_to_patch=True, **v)
    ar = vit.AutoRegressive(vocab_size=cfg["K"], n_embed_tokens=0, n_input_tokens=enc.total_num_tokens, output_tokens="input",
                            patch_to_embed=False, embed_to_patch=False, causal_mask=True, **{**v, "depth": cfg["ar_depth"]})
    prior = CodebookPrior(latent_size=enc.out_size, embed_dims=(2,), loss=cfg["loss"], loss_coeff=cfg["loss_coeff"], annealing_steps=0,
                          mixture_cfg=dict(n_components=cfg["K"], metric=cfg["metric"], temperature=cfg["temperature"],
                                           training_mode=cfg["mode"], inference_mode=cfg["mode"]),
                          update_with_autograd=True)
    model = DAD(metrics=R._MetricCollection(), encoder=enc, decoder=dec, autoregressive_decoder=ar, prior=prior)
    model.hparams.ce_coeff = cfg["ce_coeff"]   # (the import shim's save_hyperparameters records nothing)
    return model


class _Draws:
    """Categorical.sample as the inverse CDF of recorded uniforms, and F.gumbel_softmax with recorded Gumbel noise."""

    def __init__(self, u, gumbel):
        self.u, self.gumbel, self.margin = u, gumbel, float("inf")

    def __enter__(self):
        self._sample, self._gumbel = D.Categorical.sample, F.gumbel_softmax
        draws = self

        def sample(dist, sample_shape=torch.Size()):
            cdf = dist.probs.double().cumsum(-1)
            total = cdf[..., -1:]
            target = draws.u.reshape(cdf.shape[:-1]).double().unsqueeze(-1) * total
            draws.margin = min(draws.margin, float(((cdf - target).abs() / total).min().detach()))
            return (cdf <= target).sum(-1).clamp(max=cdf.shape[-1] - 1)

        def gumbel_softmax(logits, tau=1, hard=False, eps=1e-10, dim=-1):
            y = ((logits + draws.gumbel.to(logits.dtype).reshape(logits.shape)) / tau).softmax(dim)
            if hard:
                idx = y.max(dim, keepdim=True)[1]
                return torch.zeros_like(logits).scatter_(dim, idx, 1.0) - y.detach() + y
            return y

        D.Categorical.sample, F.gumbel_softmax = sample, gumbel_softmax
        return self

    def __exit__(self, *exc):
        D.Categorical.sample, F.gumbel_softmax = self._sample, self._gumbel


def _run(model, x, u, gumbel):
    model.train()
    model.zero_grad(set_to_none=True)
    with _Draws(u, gumbel) as draws:
        loss, logs, art = model.nelbo(model.batch_preprocess((x, torch.zeros(x.shape[0], dtype=torch.long))), 0)
        loss.backward()
    losses = torch.stack([logs["train/loss/total"], logs["train/loss/recon"], logs["train/loss/prior"]]).detach()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return losses, grads, art["indices"].detach(), art["distribution"].probs.detach(), draws.margin


def _record(tag, cfg, out):
    torch.manual_seed(cfg["seed"])
    model = _build(cfg)
    B, T, K = cfg["B"], 4, cfg["K"]
    x = torch.rand(B, cfg["channels"], 8, 8)
    gumbel = -torch.empty(T, B, K).exponential_().log()
    gen = torch.Generator().manual_seed(cfg["seed"])
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for attempt in range(200):
        u = torch.rand(T, B, generator=gen)
        l32, g32, idx32, probs32, margin = _run(model, x, u, gumbel)
        if margin >= MARGIN:
            break
    else:
        raise RuntimeError("no draw keeps every uniform away from the CDF boundaries")
    model.double()
    l64, g64, idx64, _, margin64 = _run(model, x.double(), u, gumbel)
    assert torch.equal(idx32, idx64) and margin64 >= 0.5 * MARGIN, (margin, margin64)
    names = [n for n, _ in model.named_parameters()]
    out[f"{tag}/keys"] = np.array(list(state.keys()))
    out[f"{tag}/params"] = np.array(names)
    for k, v in state.items():
        out[f"{tag}/state/{k}"] = v.numpy()
    out[f"{tag}/x"], out[f"{tag}/u_index"], out[f"{tag}/gumbel"] = x.numpy(), u.numpy(), gumbel.numpy()
    out[f"{tag}/indices"], out[f"{tag}/probs"] = idx32.numpy(), probs32.numpy()
    out[f"{tag}/loss32"], out[f"{tag}/loss64"] = l32.numpy(), l64.numpy()
    for n in names:
        if n in g32:
            out[f"{tag}/grad32/{n}"], out[f"{tag}/grad64/{n}"] = g32[n].numpy(), g64[n].numpy()
    print(f"{tag}: losses {l32.tolist()} margin {margin:.2e} (fp64 {margin64:.2e}) after {attempt + 1} draw(s); "
          f"{len(g32)}/{len(names)} parameters with a gradient")


CONFIGS = {
    "A": dict(seed=11, B=6, K=32, channels=1, depth=1, ar_depth=1, metric="euclidean", temperature=1.0, mode="gumbel-softmax", loss=None,
              loss_coeff=1.0, ce_coeff=1.0),
    "B": dict(seed=12, B=5, K=32, channels=3, depth=1, ar_depth=1, metric="cosine", temperature=0.1, mode="mean", loss="first_kl",
              loss_coeff=1e-3, ce_coeff=1e-3),
}

if __name__ == "__main__":
    out = {}
    for tag, cfg in CONFIGS.items():
        _record(tag, cfg, out)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT) / 1024:.1f} KiB, {len(out)} arrays")
