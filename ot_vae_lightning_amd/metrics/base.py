"""``Metric`` and ``MetricCollection``: the slice of torchmetrics' interface that the reference's model code touches
(model/base.py:100-113,125-127,197-220), without the torchmetrics dependency.

A metric is an ``nn.Module`` whose accumulators (``add_state``) are NON-persistent buffers: they follow ``.cuda()`` / ``.to()``
with the model that owns the collection and never appear in a ``state_dict``, so a checkpoint keeps loading into the reference
and back.  ``reset()`` restores the defaults in place -- the buffers keep their addresses, which a captured ``update`` relies on.
"""
import copy
import inspect
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor

__all__ = ["Metric", "MetricCollection"]

_REDUCE_OPS = ("sum", "min", "max")
# dist_reduce_fx: one of _REDUCE_OPS for the whole state, or [(start, stop, op), ...] over a 1-D state's slices
ReduceSpec = Union[str, Sequence[Tuple[int, int, str]]]


class Metric(nn.Module):
    higher_is_better: Optional[bool] = None
    compute_names: Optional[Tuple[str, ...]] = None   # names of the values of a tuple-valued ``compute`` (``MetricCollection``)
    full_state_update: bool = False

    def __init__(self, compute_on_step: bool = False, dist_sync_on_step: bool = False, process_group: Any = None,
                 dist_sync_fn: Any = None):
        super().__init__()
        self.compute_on_step = compute_on_step
        self.dist_sync_on_step = dist_sync_on_step
        self.process_group = process_group
        self.dist_sync_fn = dist_sync_fn
        self._defaults: Dict[str, Tensor] = {}
        self._reductions: Dict[str, ReduceSpec] = {}

    # ---- states
    def add_state(self, name: str, default: Tensor, dist_reduce_fx: ReduceSpec = "sum") -> None:
        if not isinstance(default, Tensor):
            raise ValueError(f"state {name!r}: the default must be a tensor")
        spec = [(0, default.numel(), dist_reduce_fx)] if isinstance(dist_reduce_fx, str) else list(dist_reduce_fx)
        for _, _, op in spec:
            if op not in _REDUCE_OPS:
                raise ValueError(f"state {name!r}: dist_reduce_fx must be one of {_REDUCE_OPS}, got {op!r}")
        self._defaults[name] = default.detach().clone()
        self._reductions[name] = dist_reduce_fx
        self.register_buffer(name, default.detach().clone(), persistent=False)

    def reset(self) -> None:
        for name, default in self._defaults.items():
            state = getattr(self, name)
            state.copy_(default.to(state.device))

    # ---- the three calls of a run
    def update(self, *args, **kwargs) -> None:  # pragma: no cover - interface
        raise NotImplementedError

    def compute(self):  # pragma: no cover - interface
        raise NotImplementedError

    def forward(self, *args, **kwargs):
        self.update(*args, **kwargs)
        if self.compute_on_step:
            if self.dist_sync_on_step:
                self.sync(self.process_group)
            return self.compute()
        return None

    def clone(self) -> "Metric":
        return copy.deepcopy(self)

    def update_keywords(self) -> Optional[List[str]]:
        """the keyword names ``update`` declares (None: it takes ``**kwargs``, i.e. everything)"""
        params = inspect.signature(self.update).parameters.values()
        if any(p.kind is inspect.Parameter.VAR_KEYWORD for p in params):
            return None
        return [p.name for p in params if p.kind in (inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY)]

    # ---- data parallel
    def sync(self, process_group: Any = None) -> None:
        """all-reduce every state over the ranks (sum, or min / max where the state says so); nothing to do without an
        initialised ``torch.distributed`` group"""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        group = process_group if process_group is not None else self.process_group
        if dist.get_world_size(group) == 1:
            return
        ops = {"sum": dist.ReduceOp.SUM, "min": dist.ReduceOp.MIN, "max": dist.ReduceOp.MAX}
        for name, spec in self._reductions.items():
            state = getattr(self, name)
            if isinstance(spec, str):
                dist.all_reduce(state, op=ops[spec], group=group)
            else:
                flat = state.view(-1)
                for start, stop, op in spec:
                    dist.all_reduce(flat[start:stop], op=ops[op], group=group)


class MetricCollection(nn.ModuleDict):
    """``MetricCollection({"psnr": PeakSignalNoiseRatio(), "fid": FrechetInceptionDistance(...)})`` or a list of metrics (named by
    their class).  ``collection(preds, target)`` hands the positional arguments to every metric; keywords reach only the metrics whose
    ``update`` names them (a validation batch is passed whole: samples, target, preds, generated, kwargs)."""

    def __init__(self, metrics: Union[Dict[str, Metric], Iterable[Metric], Metric], prefix: Optional[str] = None):
        super().__init__()
        if isinstance(metrics, Metric):
            metrics = [metrics]
        if isinstance(metrics, dict):
            named = list(metrics.items())
        else:
            named = [(type(m).__name__, m) for m in metrics]
        for name, metric in named:
            if not isinstance(metric, Metric):
                raise ValueError(f"{name!r} is not a Metric: {type(metric).__name__}")
            if name in self._modules:
                raise ValueError(f"two metrics are named {name!r}")
            self[name] = metric
        self.prefix = self._check_prefix(prefix)

    @staticmethod
    def _check_prefix(prefix):
        if prefix is not None and not isinstance(prefix, str):
            raise ValueError(f"prefix must be a string, got {prefix!r}")
        return prefix

    def _name(self, base: str) -> str:
        return base if self.prefix is None else self.prefix + base

    def clone(self, prefix: Optional[str] = None) -> "MetricCollection":
        other = copy.deepcopy(self)
        if prefix is not None:
            other.prefix = self._check_prefix(prefix)
        return other

    def items(self, keep_base: bool = False):
        if keep_base:
            return self._modules.items()
        return [(self._name(k), m) for k, m in self._modules.items()]

    def keys(self, keep_base: bool = False):
        return [k for k, _ in self.items(keep_base)]

    @staticmethod
    def _filtered(metric: Metric, kwargs: Dict[str, Any]) -> Dict[str, Any]:
        names = metric.update_keywords()
        return kwargs if names is None else {k: v for k, v in kwargs.items() if k in names}

    def update(self, *args, **kwargs) -> None:
        for _, metric in self.items(keep_base=True):
            metric.update(*args, **self._filtered(metric, kwargs))

    def _named_results(self, res: Dict[str, Any]) -> Dict[str, Any]:
        """a metric that declares ``compute_names = ("mean", "std")`` returns a tuple, logged as ``<name>_mean`` and ``<name>_std``"""
        out = {}
        for k, v in res.items():
            names = getattr(self[k], "compute_names", None)
            if names is None:
                out[self._name(k)] = v
            else:
                if len(names) != len(v):
                    raise ValueError(f"metric {k!r} declares compute_names {tuple(names)} and returned {len(v)} values")
                out.update({self._name(f"{k}_{n}"): x for n, x in zip(names, v)})
        return out

    def forward(self, *args, **kwargs) -> Dict[str, Any]:
        res = {k: m(*args, **self._filtered(m, kwargs)) for k, m in self.items(keep_base=True)}
        return self._named_results({k: v for k, v in res.items() if v is not None})

    def compute(self) -> Dict[str, Any]:
        return self._named_results({k: m.compute() for k, m in self.items(keep_base=True)})

    def reset(self) -> None:
        for _, m in self.items(keep_base=True):
            m.reset()

    def sync(self, process_group: Any = None) -> None:
        for _, m in self.items(keep_base=True):
            m.sync(process_group)
