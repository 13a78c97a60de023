"""CPU: the Discrete Auto Diffuser's host side -- the class and its reference contract (model/discrete_auto_diffuser.py:31-95), the
``otvae::soft_cross_entropy`` operator's registration, the C ABI of the four new entries, and the shape of ``tests/golden/dad.npz``
(recorded by tools/gen_dad_golden.py from the reference's own DAD)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import ot_vae_lightning_amd as A
from ot_vae_lightning_amd.model import DAD

ENTRIES = ("otvae_soft_ce_ws", "otvae_soft_ce_fwd", "otvae_soft_ce_bwd", "otvae_categorical_sample", "otvae_codebook_gather")


def build_dad(K=32, channels=1, metric="euclidean", temperature=1.0, mode="gumbel-softmax", loss=None, loss_coeff=1.0, ce_coeff=1.0,
              dropout=0.0):
    """the architecture of both recorded configurations (tools/gen_dad_golden.py)"""
    v = dict(image_size=8, patch_size=4, dim=16, depth=1, heads=4, mlp_dim=32, channels=channels, dropout=dropout, emb_dropout=0.)
    enc = A.ViT(n_embed_tokens=0, n_input_tokens=None, output_tokens="input", patch_to_embed=True, embed_to_patch=False, **v)
    dec = A.ViT(n_embed_tokens=None, n_input_tokens=enc.total_num_tokens, output_tokens="input", patch_to_embed=False,
                embed_to_patch=True, **v)
    ar = A.AutoRegressive(vocab_size=K, n_embed_tokens=0, n_input_tokens=enc.total_num_tokens, output_tokens="input",
                          patch_to_embed=False, embed_to_patch=False, causal_mask=True, **v)
    prior = A.CodebookPrior(latent_size=enc.out_size, embed_dims=(2,), loss=loss, loss_coeff=loss_coeff, annealing_steps=0,
                            mixture_cfg=dict(n_components=K, metric=metric, temperature=temperature, training_mode=mode,
                                             inference_mode=mode), update_with_autograd=True)
    return DAD(encoder=enc, decoder=dec, autoregressive_decoder=ar, prior=prior, ce_coeff=ce_coeff)


CONFIGS = {"A": dict(), "B": dict(channels=3, metric="cosine", temperature=0.1, mode="mean", loss="first_kl", loss_coeff=1e-3, ce_coeff=1e-3)}


def test_dad_is_exported():
    assert A.DAD is DAD and issubclass(DAD, A.VAE)
    from ot_vae_lightning_amd.model import discrete_auto_diffuser
    assert discrete_auto_diffuser.__all__ == ["DAD"]


def test_constructor_errors_and_attributes():
    m = build_dad()
    assert m.token_dims == 16 and m.n_tokens == 4 and m.num_embeddings == 32
    assert m.hparams.ce_coeff == 1.0
    assert isinstance(m.autoregressive_decoder, A.AutoRegressive)
    assert m.latent_size == torch.Size([4, 16])
    with pytest.raises(ValueError):
        DAD(decoder=m.decoder, prior=m.prior, autoregressive_decoder=m.autoregressive_decoder)
    with pytest.raises(ValueError):
        DAD(encoder=m.encoder, prior=m.prior, autoregressive_decoder=m.autoregressive_decoder)
    with pytest.raises(TypeError):
        DAD(encoder=m.encoder, decoder=m.decoder, prior=m.prior)   # keyword-only, required: as the reference


@pytest.mark.parametrize("tag", ["A", "B"])
def test_state_dict_keys_are_the_references(tag):
    g = np.load(os.path.join(GOLDEN, "dad.npz"), allow_pickle=False)
    m = build_dad(**CONFIGS[tag])
    assert list(m.state_dict().keys()) == [str(k) for k in g[f"{tag}/keys"]]
    assert [n for n, _ in m.named_parameters()] == [str(k) for k in g[f"{tag}/params"]]
    for k, v in m.state_dict().items():
        assert tuple(v.shape) == g[f"{tag}/state/{k}"].shape, k


def test_optim_parameters_contain_the_autoregressive_decoder():
    m = build_dad()
    ids = [id(p) for p in m.optim_parameters()]
    assert len(ids) == len(set(ids))
    ar = [p for p in m.autoregressive_decoder.parameters() if p.requires_grad]
    assert ar and all(id(p) in ids for p in ar)
    base = [id(p) for p in A.VAE.optim_parameters(m)]
    assert ids[:len(base)] == base and len(ids) == len(base) + len(ar)
    m.autoregressive_decoder.head.bias.requires_grad_(False)
    assert id(m.autoregressive_decoder.head.bias) not in [id(p) for p in m.optim_parameters()]
    # a plain VAE's parameters are what they were
    v = A.VAE(encoder=m.encoder, decoder=m.decoder, prior=m.prior)
    assert [id(p) for p in v.optim_parameters()] == base


def test_operator_registration_fake_and_cpu_refusal():
    from ot_vae_lightning_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert "soft_cross_entropy" in ops.OPS
    op = torch.ops.otvae.soft_cross_entropy.default
    assert str(op._schema) == "otvae::soft_cross_entropy(Tensor logits, Tensor probs) -> (Tensor, Tensor, Tensor)"
    for name in ("soft_cross_entropy", "soft_cross_entropy_backward"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{name}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"otvae::{name}", "CPU")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("otvae::soft_cross_entropy", "Autograd")
    with FakeTensorMode():
        l, p = torch.empty(6, 4, 32, device="cuda"), torch.empty(6, 4, 32, device="cuda")
        loss, lse, psum = torch.ops.otvae.soft_cross_entropy(l, p)
        assert loss.shape == (6,) and lse.shape == (6, 4) and psum.shape == (6, 4) and loss.dtype == torch.float32
        dl, dp = torch.ops.otvae.soft_cross_entropy_backward(loss, l, p, lse, psum, True, False)
        assert dl.shape == (6, 4, 32) and dp.numel() == 0
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.otvae.soft_cross_entropy(torch.zeros(2, 3, 4), torch.zeros(2, 3, 4))
    with pytest.raises(RuntimeError):
        A.functional.categorical_sample_(torch.zeros(2, 3, dtype=torch.int64), 1, torch.zeros(2, 3, 4), 0, u=torch.zeros(2))
    with pytest.raises(RuntimeError):
        A.functional.codebook_gather(torch.zeros(4, 2), torch.zeros(3, dtype=torch.int64))


def _prototypes():
    src = open(os.path.join(ROOT, "include", "otvae.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return {m.group(1): [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
            for m in re.finditer(r"\b(otvae_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)}


def test_header_loader_and_library_agree_on_the_new_entries():
    from ot_vae_lightning_amd import _lib, build
    protos = _prototypes()
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in ENTRIES:
        assert name in protos, f"{name} is not declared in include/otvae.h"
        restype, argtypes = _lib.SIGNATURES[name]
        params = protos[name]
        assert len(params) == len(argtypes), name
        for decl, at in zip(params, argtypes):
            assert ("*" in decl) == (at is ctypes.c_void_p), (name, decl)
            if "*" not in decl:
                assert (ctypes.c_int64 if decl.startswith("int64_t") else ctypes.c_int) is at, (name, decl)
        assert hasattr(lib, name), f"{name} is not exported"
    assert _lib.SIGNATURES["otvae_soft_ce_ws"][0] is ctypes.c_int64
    # host-side answers that launch nothing
    lib.otvae_soft_ce_ws.restype = ctypes.c_int64
    assert lib.otvae_soft_ce_ws(6, 4) == 6 * 3 * 8 and lib.otvae_soft_ce_ws(6, 1) == 0


def test_golden_holds_numbers_and_name_lists_only():
    path = os.path.join(GOLDEN, "dad.npz")
    assert os.path.getsize(path) < 1 << 20
    g = np.load(path, allow_pickle=False)
    for k in g.files:
        a = g[k]
        if k.endswith("/keys") or k.endswith("/params"):
            assert a.dtype.kind == "U" and a.ndim == 1 and max(len(s) for s in a) < 100, k
        else:
            assert a.dtype.kind in "fi", (k, a.dtype)
    for tag in ("A", "B"):
        assert g[f"{tag}/indices"].dtype == np.int64 and g[f"{tag}/loss32"].shape == (3,) and g[f"{tag}/loss64"].dtype == np.float64
        assert g[f"{tag}/probs"].shape == (*g[f"{tag}/indices"].shape, 32)
