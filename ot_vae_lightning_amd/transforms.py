"""Image transforms on the device, and the reference's progressive-transform callback (data/progressive_callback.py:25-118).

``GaussianBlur`` keeps torchvision's constructor and call (the reference's experiments build
``GaussianBlur(5, sigma=(1.5, 1.5))``, tests/test_latent_transport.py:35); torchvision itself is not needed.  ``NOOP``, ``PgTransform``,
``PgCompose``, ``ProgressiveTransform``, ``transform_args`` and ``transform_batch_tv`` have the reference's semantics, without Lightning:
``trainer`` is any object with ``current_epoch``.

Where this differs from the reference: the transform a ``ProgressiveTransform`` installs is stored on the
module INSTANCE, keyed by the decorated method's name, and the wrapper falls back to the function's ``NOOP`` -- in the reference it is
stored on the class's function, so two models in one process share it.  ``PgCompose[t]`` composes the t-th step of every member; the
reference's own line iterates a ``PgTransform``, which never ends.
"""
import functools
import warnings
from typing import Any, Callable, Dict, Sequence, Type, Union

import torch
import torch.nn as nn
from torch import Tensor

from . import functional as HF

__all__ = ["GaussianBlur", "Compose", "NOOP", "PgTransform", "PgCompose", "ProgressiveTransform", "transform_args",
           "transform_batch_tv"]

_ACTIVE = "_otvae_active_transforms"   # instance attribute: {method name: transform}


class GaussianBlur(nn.Module):
    """``torchvision.transforms.GaussianBlur``: ``kernel_size`` an odd int or (kx, ky); ``sigma`` a float (fixed) or (min, max), from
    which one value is drawn per call -- ``torch.empty(1).uniform_(min, max).item()``, the draw torchvision makes, used for both axes.
    ``last_sigma`` is the value of the latest call.  float32 images on the device, [C, H, W] or [N, C, H, W]."""

    def __init__(self, kernel_size, sigma=(0.1, 2.0)) -> None:
        super().__init__()
        if isinstance(kernel_size, int):
            kernel_size = (kernel_size, kernel_size)
        elif isinstance(kernel_size, Sequence) and len(kernel_size) == 1:
            kernel_size = (kernel_size[0], kernel_size[0])
        if not isinstance(kernel_size, Sequence) or len(kernel_size) != 2:
            raise ValueError("Kernel size should be a tuple/list of two integers")
        for ks in kernel_size:
            if not isinstance(ks, int) or ks <= 0 or ks % 2 == 0:
                raise ValueError("Kernel size value should be an odd and positive number.")
        self.kernel_size = tuple(kernel_size)
        if isinstance(sigma, (int, float)):
            if sigma <= 0:
                raise ValueError("If sigma is a single number, it must be positive.")
            sigma = (sigma, sigma)
        elif isinstance(sigma, Sequence) and len(sigma) == 2:
            if not 0.0 < sigma[0] <= sigma[1]:
                raise ValueError("sigma values should be positive and of the form (min, max).")
        else:
            raise ValueError("sigma should be a single number or a list/tuple with length 2.")
        self.sigma = tuple(float(s) for s in sigma)
        self.last_sigma = None

    @staticmethod
    def get_params(sigma_min: float, sigma_max: float) -> float:
        return torch.empty(1).uniform_(sigma_min, sigma_max).item()

    def forward(self, img: Tensor) -> Tensor:
        sigma = self.get_params(self.sigma[0], self.sigma[1])
        self.last_sigma = sigma
        return HF.gaussian_blur(img, self.kernel_size, (sigma, sigma))

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(kernel_size={self.kernel_size}, sigma={self.sigma})"


class Compose:
    """The chain ``transforms[-1](... transforms[0](x))`` (torchvision's ``Compose``; the default ``compose_cls`` of ``PgCompose``)."""

    def __init__(self, transforms: Sequence[Callable]) -> None:
        self.transforms = list(transforms)

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.transforms})"


class NOOP:
    def __call__(self, arg):
        return arg


class PgTransform:
    """``PgTransform(cls, {'sigma': [s0, s1, ...]}, **fixed)[t]``: ``cls`` built with the t-th value of every varying keyword (the last
    one once a sequence has run out); ``NOOP`` for ``t > num_steps`` (data/progressive_callback.py:30-46)."""

    def __init__(self, transform_cls: Type, varying_kwargs: Dict[str, Sequence[Any]], **kwargs) -> None:
        self.transform_cls = transform_cls
        self.varying_kwargs = varying_kwargs
        self.kwargs = kwargs
        self.num_steps = max([len(seq) for seq in varying_kwargs.values()])

    def __getitem__(self, timestamp: int) -> Callable:
        if timestamp > self.num_steps:
            return NOOP()
        step_kwargs = {k: seq[min(len(seq) - 1, timestamp)] for k, seq in self.varying_kwargs.items()}
        return self.transform_cls(**step_kwargs, **self.kwargs)


class PgCompose:
    def __init__(self, diffused_transforms: Sequence[PgTransform], compose_cls: Any = Compose) -> None:
        self.transforms = diffused_transforms
        self.compose_cls = compose_cls

    def __getitem__(self, timestamp: int) -> Callable:
        return self.compose_cls([t[timestamp] for t in self.transforms])


def _decorated(method) -> bool:
    return callable(method) and hasattr(method, "__wrapped__") and hasattr(method.__wrapped__, "transform")


class ProgressiveTransform:
    """On the epochs named in ``schedule``, every method of the module decorated with ``transform_args`` gets
    ``transform[trainer.current_epoch]`` as its argument transform; on every other epoch the one in place stays
    (data/progressive_callback.py:58-97)."""

    def __init__(self, transform: Union[PgTransform, PgCompose], schedule: Sequence[int]) -> None:
        self.transform = transform
        self.schedule = schedule

    def on_train_epoch_start(self, trainer, pl_module) -> None:
        if trainer.current_epoch not in self.schedule:
            return
        found = False
        for func in dir(pl_module):
            try:
                method = getattr(pl_module, func)
            except Exception:   # a property that cannot be evaluated now (e.g. one that needs a trainer) is no method
                continue
            if _decorated(method):
                active = pl_module.__dict__.setdefault(_ACTIVE, {})
                active[method.__wrapped__.__name__] = self.transform[trainer.current_epoch]
                found = True
        if not found:
            warnings.warn("`ProgressiveTransform` didn't find any method of the module which should have its arguments transformed. "
                          "Use the @transform_args decorator in order to have a method affected by the callback.")


def transform_args(getter_func: Callable = lambda x: x, setter_func: Callable = lambda orig, changed: orig):
    """Decorator: ``method(self, *arg)`` is called with ``setter_func(transform(getter_func(*arg)), *arg)``.  ``transform`` is what a
    ``ProgressiveTransform`` installed on this instance for this method, else the function's own ``method.transform`` (``NOOP``)."""
    def decorator(method):
        method.transform = NOOP()

        @functools.wraps(method)
        def wrapper(self, *arg):
            transform = getattr(self, "__dict__", {}).get(_ACTIVE, {}).get(method.__name__, method.transform)
            to_transform = getter_func(*arg)
            transformed = transform(to_transform)
            new = setter_func(transformed, *arg)
            return method(self, new)
        return wrapper
    return decorator


transform_batch_tv = functools.partial(
    transform_args,
    getter_func=lambda b: b[0],
    setter_func=lambda x, b: (x, *b[1:])
)
