"""``DAD(encoder=, decoder=, prior=CodebookPrior, autoregressive_decoder=)``: the reference's Discrete Auto Diffuser
(model/discrete_auto_diffuser.py:31-95).  A VAE over vector-quantised tokens whose training loss adds the cross-entropy between an
autoregressive decoder's next-token logits and the codebook's assignment probabilities, and whose ``sample`` runs that decoder
token by token.

MI355X path: the cross-entropy is one fused operator (``torch.ops.otvae.soft_cross_entropy``: one pass over the two [B, T, K]
tensors, the one-token shift as index arithmetic), every step of the sampling loop is one launch that writes ``ids[:, i + 1]`` in
place (``otvae_categorical_sample``, or ``otvae_filtered_sample`` under a temperature / top-k / top-p: no host read inside the loop),
and the sampled ids are decoded by a row gather
(``otvae_codebook_gather``) instead of ``one_hot @ codebook``.

Deliberate difference from the reference: ``optim_parameters()`` also yields the autoregressive decoder's parameters.  The reference
inherits ``VAE.optim_parameters`` (model/vae.py:142-146: encoder, decoder, prior), so its own optimizer never updates the decoder
its loss trains."""
import itertools
from typing import Dict, Optional, Union

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor
from torch.distributions import Categorical

from .. import functional as HF
from ..prior.codebook import CodebookPrior
from .vae import VAE

__all__ = ["DAD"]


class DAD(VAE):
    # noinspection PyUnusedLocal
    def __init__(self, *vae_args, prior: CodebookPrior, autoregressive_decoder: nn.Module, ce_coeff: float = 1., **vae_kwargs) -> None:
        super().__init__(*vae_args, prior=prior, **vae_kwargs)
        self.hparams.ce_coeff = ce_coeff
        self.token_dims = prior.dimensionality
        self.n_tokens = int(np.prod(prior.batch_shape))
        self.num_embeddings = prior.num_embeddings
        self.autoregressive_decoder = autoregressive_decoder

    def optim_parameters(self):
        return itertools.chain(super().optim_parameters(),
                               filter(lambda p: p.requires_grad, self.autoregressive_decoder.parameters()))

    def per_sample_prior_loss(self, prior_loss: Tensor, artifacts: Dict[str, Union[Tensor, Categorical]], **kwargs) -> Tensor:
        """prior_loss[B] + ce_coeff * ce[B] (discrete_auto_diffuser.py:56-74), ce[b] = sum_t KL-style cross-entropy between the
        assignment probabilities of token t + 1 (NOT detached: the gradient reaches the encoder) and the autoregressive decoder's
        prediction from the sampled tokens <= t."""
        distributions, indices = artifacts["distribution"], artifacts["indices"]
        logits = self.autoregressive_decoder(indices.detach())
        labels = distributions.probs
        expected_shape = torch.Size([prior_loss.size(0), self.n_tokens, self.num_embeddings])
        assert labels.shape == logits.shape == expected_shape
        return prior_loss + self.hparams.ce_coeff * HF.soft_cross_entropy(logits, labels).type_as(prior_loss)

    def prior_loss(self, prior_loss: Tensor, artifacts: Dict[str, Union[Tensor, Categorical]], **kwargs) -> Tensor:
        return super().prior_loss(self.per_sample_prior_loss(prior_loss, artifacts, **kwargs), artifacts, **kwargs)

    @VAE.postprocess
    def sample(self, batch_size: int, *, init_indices: Optional[Tensor] = None, noise: Optional[Tensor] = None, cached: bool = False,
               temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None, **kwargs) -> Tensor:
        """Reference discrete_auto_diffuser.py:77-95.  ``init_indices`` (int64 [B, T], the uniformly random start; only column 0
        survives) and ``noise`` ([B, T - 1] uniforms in [0, 1): token i + 1 is the inverse CDF of ``noise[:, i]`` under the decoder's
        distribution at position i) make the draw reproducible; without them both are drawn on the device.

        ``temperature``, ``top_k`` and ``top_p`` filter the decoder's distribution at every position, in that order, inside the draw's
        one launch (``HF.categorical_sample_``): logits over ``temperature``, then the ``top_k`` most likely tokens, then of those the
        smallest set whose renormalised mass reaches ``top_p``; ``noise[:, i]`` is then the uniform of step i under the filtered
        distribution.  ``temperature=0`` (or ``top_k=1``) decodes greedily.  The defaults draw from the unfiltered distribution, as the
        reference does.  top-k / top-p need ``num_embeddings <= 16384`` (``NotImplementedError`` beyond).

        ``cached=True`` advances the decoder one token at a time on per-layer key / value caches (``AutoRegressive.decode_state`` /
        ``step``) instead of running it on the whole id matrix T - 1 times: same draws, same distribution at every position.  A decoder
        that route cannot take (``decode_state``'s rules) raises ``NotImplementedError``; there is no silent fall-back."""
        HF.check_token_filter(temperature, top_k, top_p)
        device, T = self.device, self.n_tokens
        state = None
        if cached:
            if not hasattr(self.autoregressive_decoder, "decode_state"):
                raise NotImplementedError(f"`cached=True` needs a decoder with `decode_state` / `step`, got {type(self.autoregressive_decoder).__name__}")
            state = self.autoregressive_decoder.decode_state(batch_size, T)
        if init_indices is None:
            embed_ind = torch.randint(high=self.num_embeddings, size=(batch_size, T), device=device)
        else:
            if tuple(init_indices.shape) != (batch_size, T):
                raise ValueError(f"`init_indices` must be [{batch_size}, {T}], got {tuple(init_indices.shape)}")
            embed_ind = init_indices.to(device=device, dtype=torch.int64).clone()
        key = None
        if noise is None:
            key = self.__dict__.get("_sample_key")
            if key is None or key.device != device:
                key = self.__dict__["_sample_key"] = HF.new_dropout_key(device)
            key[1:].add_(1)
        else:
            if tuple(noise.shape) != (batch_size, T - 1):
                raise ValueError(f"`noise` must be [{batch_size}, {T - 1}], got {tuple(noise.shape)}")
            noise = noise.to(device=device, dtype=torch.float32).t().contiguous()   # [T - 1, B]: one contiguous row per step
        with torch.no_grad():
            for i in range(T - 1):
                if state is not None:
                    logits, at = self.autoregressive_decoder.step(embed_ind[:, i], state).unsqueeze(1), 0
                else:
                    logits, at = self.autoregressive_decoder(embed_ind), i
                HF.categorical_sample_(embed_ind, i + 1, logits, at, u=None if noise is None else noise[i], key=key,
                                       temperature=temperature, top_k=top_k, top_p=top_p)
            codebook = self.prior.codebook_model.codebook
            latents = HF.codebook_gather(codebook.reshape(-1, codebook.shape[-1]).float(), embed_ind).type_as(codebook)
        latents = self.prior.unflatten_and_unpermute(latents.transpose(0, 1))
        return self.decode(latents, **kwargs, no_postprocess_override=True)
