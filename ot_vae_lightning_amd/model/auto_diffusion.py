"""``AutoDiffusion(autoencoder=AutoEncoder(..., time_embed_dim=...), prior=GaussianPrior(fixed_var=True))``: the reference's
time-conditioned VAE (model/auto_diffusion.py:16-85).  Every training sample draws a time t ~ U[0, 1]; the autoencoder is conditioned
on it (FiLM on every ConvLayer), the prior re-parametrises with t as its temperature, and the prior's regulariser is weighted by
beta_t = 0.5 * tanh(10 * (t - 0.5)) + 0.5.  ``sample`` walks t from 1 down to 1 / n_steps, decoding and re-encoding at each step.

The prior must be built with ``fixed_var=True``: the time is its temperature (prior/gaussian.py), and this package's ``GaussianPrior``
refuses ``time`` otherwise -- with a learned variance there is no place for a temperature in the closed-form KL.

Differences from the reference, all deliberate:
  * ``sample(latents=, noise=)`` make a draw reproducible: the start of the chain and one ``eps`` per encode call;
  * the beta weighting lives in ``per_sample_prior_loss`` (the fused loss reduction takes the [B] vector); ``prior_loss`` is its mean,
    as the reference's override computes;
  * ``sample`` does not swallow a ``RuntimeError`` into an empty list, and ``FilterKwargs`` is not patched: ``VAE`` forwards every
    keyword by the callee's signature already."""
from typing import List, Optional, Union

import numpy as np
import torch
from torch import Tensor

from ..utils import Collage
from .vae import VAE

__all__ = ["AutoDiffusion"]


class AutoDiffusion(VAE):
    n_steps = int(1e1)

    def batch_preprocess(self, batch) -> VAE.Batch:
        pbatch = super().batch_preprocess(batch)
        batch_size = pbatch["samples"].size(0)
        pbatch["kwargs"]["time"] = torch.rand(batch_size, device=self.device)
        return pbatch

    def per_sample_prior_loss(self, prior_loss: Tensor, prior_artifacts, **kwargs) -> Tensor:
        """beta_t * prior_loss per (replicated) sample, t = the batch's ``time`` (auto_diffusion.py:29-32)"""
        t = self._expand(kwargs["time"])
        beta_t = 0.5 * torch.tanh(10 * (t - 0.5)) + 0.5
        return beta_t * prior_loss

    def prior_loss(self, prior_loss: Tensor, prior_artifacts, **kwargs) -> Tensor:
        return self.per_sample_prior_loss(prior_loss, prior_artifacts, **kwargs).mean()

    @VAE.postprocess
    def sample(self, batch_size: int, steps: Optional[List[int]] = None, improved_algorithm: bool = False, *,
               latents: Optional[Tensor] = None, noise: Optional[Tensor] = None, **kwargs) -> Union[Tensor, List[Tensor]]:
        """Reference auto_diffusion.py:35-59.  From xs ~ prior (or ``latents``), for s = 1, 1 - 1/n, ..., 1/n:
        ``x_hat = decode(xs, time=s)`` and then ``xs = encode(x_hat, time=s - 1/n)``, or with ``improved_algorithm``
        ``xs -= encode(x_hat, time=s - 1/n) - encode(x_hat, time=s)``.  Returns the last ``x_hat``, or with ``steps`` the list of the
        ``x_hat`` of the iterations named there.

        ``noise`` [n_encode_calls, B, *latent_size]: row k is the ``eps`` of the k-th encode call (n_steps calls, twice as many with
        ``improved_algorithm``).  ``kwargs['time']`` is used for its shape only; without it the times are [batch_size]."""
        n = self.n_steps
        n_calls = n * (2 if improved_algorithm else 1)
        if noise is not None and tuple(noise.shape) != (n_calls, batch_size, *self.latent_size):
            raise ValueError(f"`noise` must be {(n_calls, batch_size, *self.latent_size)}: one draw per encode call, "
                             f"got {tuple(noise.shape)}")
        if latents is not None and tuple(latents.shape) != (batch_size, *self.latent_size):
            raise ValueError(f"`latents` must be {(batch_size, *self.latent_size)}, got {tuple(latents.shape)}")
        x_hat, intermediate, call = None, [], 0

        def encode(x, t):
            nonlocal call
            extra = {} if noise is None else {"eps": noise[call]}
            call += 1
            return self.encode(x, **{**kwargs, **extra, "time": t}, no_preprocess_override=True)

        with torch.no_grad():
            ones = torch.ones_like(kwargs["time"]) if kwargs.get("time") is not None else torch.ones(batch_size, device=self.device)
            if latents is not None:
                xs = latents.to(self.device).clone()   # (the improved algorithm updates it in place)
            elif self.prior is not None:
                draw_kwargs = {**kwargs, "time": ones}
                with self._filter(self.prior.sample, draw_kwargs.keys()) as draw:
                    xs = draw((batch_size, *self.latent_size), device=self.device, **draw_kwargs)
            else:
                xs = torch.randn((batch_size, *self.latent_size), device=self.device)
            step_size = 1 / n
            for i, s in enumerate(np.linspace(1, step_size, n)):
                x_hat = self.decode(xs, **{**kwargs, "time": ones * s}, no_postprocess_override=True)
                if improved_algorithm:
                    xs -= encode(x_hat, ones * (s - step_size)) - encode(x_hat, ones * s)
                else:
                    xs = encode(x_hat, ones * (s - step_size))
                if steps is not None and i in steps:
                    intermediate.append(x_hat)
        return x_hat if steps is None else intermediate

    def _generation_steps(self) -> List[int]:
        return [int(i) for i in np.linspace(0, self.n_steps, 10)]   # (n_steps itself is never reached: 9 images at n_steps = 10)

    @Collage.log_method
    def reconstruction(self, batch: VAE.Batch) -> List[Tensor]:
        samples, target, kwargs = batch["samples"], batch["target"], batch["kwargs"]
        ones = torch.ones_like(kwargs["time"])
        return [self(samples, **{**kwargs, "time": ones * t}) for t in np.linspace(0, 1, 10)] + [target]

    @Collage.log_method
    def generation(self, batch: VAE.Batch) -> List[Tensor]:
        samples, kwargs = batch["samples"], batch["kwargs"]
        return self.sample(samples.size(0), steps=self._generation_steps(), improved_algorithm=False, **kwargs)

    @Collage.log_method
    def generation_improved(self, batch: VAE.Batch) -> List[Tensor]:
        samples, kwargs = batch["samples"], batch["kwargs"]
        return self.sample(samples.size(0), steps=self._generation_steps(), improved_algorithm=True, **kwargs)
