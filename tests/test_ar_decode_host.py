"""CPU: the host side of key/value-cached decoding -- ``AutoRegressive.decode_state``'s eligibility rules, the refusals that need no
device, the C ABI of the two new entries, and ``DAD.sample``'s ``cached`` keyword."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
from test_dad_host import build_dad

import ot_vae_lightning_amd as A
from ot_vae_lightning_amd import functional as HF
from ot_vae_lightning_amd.networks.vit import ARDecodeState

ENTRIES = ("otvae_ar_layer_step", "otvae_ar_embed_step")


def make_ar(**extra):
    kw = dict(vocab_size=32, image_size=8, patch_size=4, dim=16, depth=2, heads=4, mlp_dim=32, dropout=0.0, emb_dropout=0.0,
              n_embed_tokens=0, n_input_tokens=6, output_tokens="input", patch_to_embed=False, embed_to_patch=False, causal_mask=True)
    kw.update(extra)
    return A.AutoRegressive(**kw)


def test_decode_state_owns_the_caches():
    ar = make_ar().eval()
    state = ar.decode_state(3)
    assert isinstance(state, ARDecodeState) and state.length == 0 and state.batch_size == 3 and state.max_tokens == 6
    assert len(state.kcache) == len(state.vcache) == 2
    for t in state.kcache + state.vcache:
        assert t.shape == (3, 4, 6, 4) and t.dtype == torch.float32 and t.is_contiguous()
    assert ar.decode_state(3, max_tokens=2).kcache[0].shape == (3, 4, 2, 4)
    state.length = 5
    assert state.reset() is state and state.length == 0
    for bad in (0, 7):
        with pytest.raises(ValueError):
            ar.decode_state(3, max_tokens=bad)
    # embed / class tokens behind the input tokens do not make a decoder ineligible
    assert make_ar(n_embed_tokens=1).eval().decode_state(2).max_tokens == 6
    assert make_ar(n_embed_tokens=1, num_classes=5).eval().decode_state(2).max_tokens == 6


def test_decode_state_refusals():
    with pytest.raises(NotImplementedError, match="causal_mask"):
        make_ar(causal_mask=False).eval().decode_state(2)
    with pytest.raises(NotImplementedError, match="preprocess_depth"):
        make_ar(preprocess_depth=1, n_embed_tokens=1).eval().decode_state(2)
    with pytest.raises(NotImplementedError, match="output_tokens"):
        make_ar(n_embed_tokens=1, output_tokens="embed").eval().decode_state(2)
    with pytest.raises(NotImplementedError, match="output_tokens"):
        make_ar(n_embed_tokens=1, output_tokens=["input", "embed"]).eval().decode_state(2)
    dropping = make_ar(dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        dropping.train().decode_state(2)
    assert dropping.eval().decode_state(2).length == 0
    assert make_ar().train().decode_state(2).length == 0          # training mode with every dropout 0 drops nothing
    with pytest.raises(NotImplementedError, match="dropout"):
        make_ar(emb_dropout=0.1).train().decode_state(2)


def test_step_refusals_without_a_device():
    ar = make_ar().eval()
    state = ar.decode_state(2)
    with pytest.raises(RuntimeError, match="MI355X"):
        ar.step(torch.zeros(2, dtype=torch.int64), state)          # CPU tensors: there is no CPU execution path
    assert state.length == 0
    state.length = state.max_tokens
    with pytest.raises(ValueError):
        ar.step(torch.zeros(2, dtype=torch.int64), state)          # past max_tokens
    state.reset()
    with pytest.raises(ValueError):
        ar.step(torch.zeros(3, dtype=torch.int64), state)          # another batch size than the state's
    with pytest.raises(RuntimeError):
        HF.ar_layer_step(torch.zeros(2, 16), 0, 4, *([torch.zeros(1)] * 6), 1e-5, *([torch.zeros(1)] * 6), 1e-5, torch.zeros(2, 4, 6, 4),
                         torch.zeros(2, 4, 6, 4))
    with pytest.raises(RuntimeError):
        HF.ar_embed_step(torch.zeros(2, dtype=torch.int64), 0, torch.zeros(32, 16), torch.zeros(6, 16), torch.ones(16), torch.zeros(16), 1e-5)


def test_existing_classes_keep_their_state_dict_keys():
    ar = make_ar()
    keys = list(ar.state_dict().keys())
    assert keys[-3:] == ["vocab_embed.weight", "head.weight", "head.bias"] and not any("cache" in k for k in keys)
    ar.eval().decode_state(2)
    assert list(ar.state_dict().keys()) == keys


def test_dad_sample_has_the_cached_keyword_off_by_default():
    sig = inspect.signature(A.DAD.sample)
    assert sig.parameters["cached"].default is False and sig.parameters["cached"].kind is inspect.Parameter.KEYWORD_ONLY
    model = build_dad().eval()
    model.autoregressive_decoder.causal_mask = False
    with pytest.raises(NotImplementedError, match="causal_mask"):   # refused before anything touches a device
        model.sample(2, cached=True)


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
        assert restype is ctypes.c_int and len(params) == len(argtypes), name
        for decl, at in zip(params, argtypes):
            assert ("*" in decl) == (at is ctypes.c_void_p), (name, decl)
            if "*" not in decl:
                want = ctypes.c_float if decl.startswith("float") else ctypes.c_int64 if decl.startswith("int64_t") else ctypes.c_int
                assert want is at, (name, decl)
        assert hasattr(lib, name), f"{name} is not exported"
    names = [p.split()[-1].lstrip("*") for p in protos["otvae_ar_layer_step"]]
    assert names == ["x", "B", "D", "H", "F", "pos", "Tmax", "w_in", "b_in", "w_out", "b_out", "ln1_g", "ln1_b", "eps1", "w1", "b1", "w2", "b2",
                     "ln2_g", "ln2_b", "eps2", "kcache", "vcache", "y", "stream"]


def test_layer_kernel_uses_fp32_mfma_and_does_not_spill():
    """Device assembly of the new source: the layer's GEMMs issue v_mfma_f32_16x16x4_f32, nothing spills to scratch."""
    import subprocess
    src = os.path.join(ROOT, "ot_vae_lightning_amd", "csrc", "ar_decode.hip")
    r = subprocess.run(["hipcc", "-x", "hip", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", "-", src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ar_decode.hip" not in r.stderr, r.stderr[-2000:]      # no diagnostics about the source itself
    assert r.stdout.count("v_mfma_f32_16x16x4_f32") >= 16
    spills = [int(x) for x in re.findall(r"\.vgpr_spill_count:\s+(\d+)", r.stdout)]
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", r.stdout)]
    assert len(spills) == 2 and max(spills) == 0 and max(scratch) == 0, (spills, scratch)
