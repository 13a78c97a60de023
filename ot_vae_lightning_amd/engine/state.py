"""What a training step writes besides what the optimizer owns: ONE enumeration for the step guard (which keeps it in one flat
range and puts it back when it refuses a step) and for every capture (which snapshots it before warm-up and restores it after)."""
from typing import List, Sequence

import torch
from torch import Tensor


def step_state(model, flat_params, latent_shape, device, latent_stats=None) -> List[Tensor]:
    """Every tensor OBJECT whose storage a training step writes besides parameters / moments / gradients: all buffers of the model
    (BatchNorm running statistics and counters, the EMA embeddings of a ConditionalGaussianPrior, GaussianW2Prior's warm-start
    flag), parameters not in ``flat_params`` (frozen ones an EMA rewrites), the dropout key counters, what modules declare through
    ``_otvae_step_state(latent_shape, device)`` (state that is not a registered buffer: GaussianW2Prior's warm-start basis) and the
    running statistics of the latent operator.  Each object once; no empty ones."""
    flat_ids = {id(p) for p in flat_params}
    ts: List[Tensor] = list(model.buffers())
    ts += [p for p in model.parameters() if id(p) not in flat_ids]
    for mod in model.modules():
        key = mod.__dict__.get("_dropout_key")
        if isinstance(key, Tensor):
            ts.append(key)
        decl = getattr(mod, "_otvae_step_state", None)
        if decl is not None:
            ts += list(decl(tuple(latent_shape), device))
    if latent_stats is not None:
        ts += list(latent_stats.buffers()) + list(latent_stats.parameters())
    seen, out = set(), []
    for t in ts:
        if t is None or id(t) in seen or t.numel() == 0:
            continue
        seen.add(id(t))
        out.append(t)
    return out


def snapshot(tensors: Sequence[Tensor]) -> List[Tensor]:
    return [t.detach().clone() for t in tensors]


def restore(tensors: Sequence[Tensor], snap: Sequence[Tensor]) -> None:
    with torch.no_grad():
        for t, v in zip(tensors, snap):
            t.copy_(v)
