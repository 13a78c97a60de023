"""``FilterSequential``, ``GaussianFourierProjection`` and ``QKVAttention`` with the reference's interface
(networks/nets_utils.py:10-19,22-52,55-82), executing on the MI355X kernels."""
import inspect
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from .. import functional as HF

__all__ = ["FilterSequential", "GaussianFourierProjection", "QKVAttention"]


def _accepts(module: nn.Module, name: str) -> bool:
    return name in inspect.signature(module.forward).parameters


class FilterSequential(nn.Sequential):
    """Sequential that forwards a keyword argument only to the layers whose ``forward`` declares it.
    The reference re-inspects every layer's signature on every call (nets_utils.py:15-19, utils/__init__.py:78-109);
    here the per-layer decision is cached the first time a keyword set is seen."""

    def forward(self, x, **kwargs):
        keys = tuple(sorted(kwargs))
        cache = self.__dict__.setdefault("_kw_cache", {})
        plan = cache.get(keys)
        if plan is None or len(plan) != len(self):
            plan = [tuple(k for k in keys if _accepts(layer, k)) for layer in self]
            cache[keys] = plan
        for layer, ks in zip(self, plan):
            x = layer(x, **{k: kwargs[k] for k in ks})
        return x


def _alias(p: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """The same memory as ``p`` under a tensor object of its own, without the gradient slot a training engine attached to the
    parameter: a kernel WRITES a parameter's gradient into that slot, so a parameter used twice in one pass must collect its two
    gradients through autograd (which adds them) instead."""
    a = p[...]
    wd = getattr(like, "_otvae_wd", None)   # (the engine's resident transposed copy for the data-gradient kernel is still right)
    if wd is not None:
        a._otvae_wd = wd
    return a


class GaussianFourierProjection(nn.Module):
    """Gaussian random features for encoding time steps (reference nets_utils.py:22-52): ``proj([sin(p), cos(p)])`` with
    ``p = t * weight * 2 * pi``, ``weight`` [1, dim // 2] drawn once from N(0, scale^2).

    Same construction as the reference, quirks included: ``[nn.ReLU(), nn.Linear(out_dim, out_dim)] * (n_layers - 1)`` repeats ONE
    Linear object, so ``proj.2`` and ``proj.4`` are the same module (shared weights, both keys in the state dict).

    MI355X path: the features are one launch (``otvae_fourier_features``) and every Linear is one launch of the fused 1x1 route with
    the ReLU in its prologue (``TokenLinear(relu_input=True)``): 1 + n_layers launches, no ATen kernel.  ``trainable=True`` computes the
    features with torch operators so that autograd reaches ``weight``."""

    def __init__(self, dim: int, out_dim: Optional[int] = None, n_layers: int = 3, scale: float = 30., trainable: bool = False):
        super().__init__()
        from .vit import TokenLinear
        self.dim = dim
        self.scale = scale
        self.weight = nn.Parameter(self._init_tensor, requires_grad=trainable)
        self.proj = nn.Sequential(
            TokenLinear(dim, out_dim) if out_dim is not None else nn.Identity(),
            *([nn.ReLU(), TokenLinear(out_dim, out_dim)] * (n_layers - 1))
        )

    @property
    def _init_tensor(self):
        return torch.randn(1, self.dim // 2) * self.scale

    def forward(self, input):
        if input.dim() != 1:
            raise ValueError("`input` is expected to be 1-dimensional")
        # the range check reads the device: not possible (and not wanted) while a step is being captured into a graph
        if not (input.is_cuda and torch.cuda.is_current_stream_capturing()):
            if (input < 0).any() or (input > 1).any():
                raise ValueError("`input` is expected to contain floats in the range [0,1]")
        if self.weight.requires_grad:
            x_proj = input.unsqueeze(-1) * self.weight * 2 * np.pi
            feats = torch.cat([torch.sin(x_proj), torch.cos(x_proj)], dim=-1)
        else:
            feats = HF.fourier_features(input, self.weight)
        h = feats.unsqueeze(0)   # [1, N, dim]: N tokens for the 1x1 route
        layers = list(self.proj)
        if not isinstance(layers[0], nn.Identity):
            h = layers[0](h)
        for layer in layers[2::2]:   # each behind a ReLU, which its kernel applies to what it reads
            shared = sum(1 for other in layers if other is layer) > 1
            if shared:
                h = HF.linear_tokens(h, _alias(layer.weight, layer.weight), _alias(layer.bias, layer.bias), relu_input=True)
            else:
                h = layer(h, relu_input=True)
        return h.squeeze(0)


class QKVAttention(nn.Module):
    """QKV attention over ``[N, (G,) 3*H*C, T]`` -> ``[N, G*H*C, T]`` (no mask, no residual, q and k both scaled by
    C**-0.5).  A 4-D channels-last ``[N, 3*H*C, Hs, Ws]`` tensor is accepted as well (the AttentionBlock fast path,
    no layout change)."""

    def __init__(self, n_heads):
        super().__init__()
        self.n_heads = int(n_heads)

    def forward(self, qkv):
        if qkv.dim() == 4 and HF.is_nhwc(qkv) and qkv.shape[1] % (3 * self.n_heads) == 0 and not getattr(self, "_grouped", False):
            return HF.qkv_attention(qkv, self.n_heads)
        if qkv.dim() == 3:
            qkv = qkv.unsqueeze(1)
        bs, groups, width, length = qkv.shape
        assert width % (3 * self.n_heads) == 0, \
            f"tensor width: {width} must be divisible by (3 * n_heads): {3 * self.n_heads}"
        a = HF.qkv_attention(qkv.reshape(bs * groups, width, length), self.n_heads)
        return a.reshape(bs, -1, length)
