"""CPU: the host side of the filtered token sampler -- the C ABI of ``otvae_filtered_sample`` (header, library, loader), the scalar
checks of ``HF.categorical_sample_`` and ``DAD.sample`` (raised before anything needs a device), and ``DAD.sample``'s signature."""
import ctypes
import inspect

import pytest
import torch

import ot_vae_lightning_amd as A
from ot_vae_lightning_amd.model import DAD
from test_dad_host import _prototypes, build_dad

BAD = [dict(temperature=-0.5), dict(temperature=float("nan")), dict(temperature=float("inf")), dict(temperature=None),
       dict(top_k=0), dict(top_k=-3), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.5), dict(top_p=float("nan"))]


def test_header_loader_and_library_agree_on_the_entry():
    from ot_vae_lightning_amd import _lib, build
    name = "otvae_filtered_sample"
    protos = _prototypes()
    assert name in protos, f"{name} is not declared in include/otvae.h"
    restype, argtypes = _lib.SIGNATURES[name]
    params = protos[name]
    assert restype is ctypes.c_int and len(params) == len(argtypes)
    for decl, at in zip(params, argtypes):
        want = ctypes.c_void_p if "*" in decl else {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}[decl.split()[0]]
        assert at is want, (decl, at)
    # otvae_categorical_sample's parameters, then temperature, top_k, top_p, kept; the stream stays last
    plain = protos["otvae_categorical_sample"]
    assert params[:len(plain) - 1] == plain[:-1] and params[-1] == plain[-1]
    assert [p.split()[-1].lstrip("*") for p in params[len(plain) - 1:-1]] == ["temperature", "top_k", "top_p", "kept"]
    assert hasattr(ctypes.CDLL(build.build(verbose=False)), name), f"{name} is not exported"


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_scalars_raise_before_any_device_requirement(bad):
    ids, logits, u = torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, 4), torch.zeros(2)
    with pytest.raises(ValueError, match=next(iter(bad))):
        A.functional.categorical_sample_(ids, 1, logits, 0, u=u, **bad)
    m = build_dad()
    with pytest.raises(ValueError, match=next(iter(bad))):
        m.sample(2, **bad)
    with pytest.raises(ValueError, match=next(iter(bad))):
        m.sample(2, cached=True, init_indices=torch.zeros(2, 4, dtype=torch.int64), **bad)


def test_good_scalars_reach_the_device_requirement():
    """legal settings pass the scalar checks: on CPU tensors the next gate is the device requirement"""
    ids, logits, u = torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, 4), torch.zeros(2)
    for good in (dict(), dict(temperature=0), dict(temperature=0.0, top_k=1, top_p=1.0), dict(temperature=2.5, top_k=10 ** 6, top_p=1e-6)):
        with pytest.raises(RuntimeError, match="cuda|GPU|device"):
            A.functional.categorical_sample_(ids, 1, logits, 0, u=u, **good)


def test_sample_signature():
    params = inspect.signature(DAD.sample).parameters
    for name, default in (("temperature", 1.0), ("top_k", None), ("top_p", None)):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default, name
    assert params["temperature"].default is not None and isinstance(params["temperature"].default, float)
    for name in ("init_indices", "noise", "cached"):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(A.functional.categorical_sample_).parameters
    for name, default in (("temperature", 1.0), ("top_k", None), ("top_p", None), ("kept", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
