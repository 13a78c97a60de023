"""Minibatch optimal-transport priors for BASELINE configs 3-4.  The reference has no such class: these
are new ``Prior`` subclasses on the reference's plug-in API whose arithmetic is the reference's own
``sinkhorn_log`` (ot/w2_utils.py:276-319) composed with a squared-euclidean cost normalised by its maximum and the
``sum(C * pi)`` read-out, exactly as ``batch_ot_gmm`` does (ot/w2_utils.py:265-269).

    loss = sum_ij C_ij pi_ij,  C_ij = |z_i - y_j|^2,  pi the (detached) entropic plan of C / max C with uniform marginals
    d loss / d z_i = 2 sum_j pi_ij (z_i - y_j)         envelope form: the plan is a constant

Forward = ``torch.ops.otvae.sinkhorn_prior`` -> ``otvae_sinkhorn_prior_fwd`` (cost tiles + tile maxima on the matrix cores, the solve,
the read-out), backward = ``otvae_ot_cost_grad`` (plan x samples on the matrix cores): no library GEMM and no ATen kernel on either side."""
from typing import Optional

import torch
from torch import Tensor

from ..ot import w2_utils as W
from .base import MinibatchPrior, Prior, _LatentLossFn

__all__ = ["SinkhornPrior"]


class SinkhornPrior(MinibatchPrior):
    """Deterministic encoder + entropic OT between the minibatch of latents and a minibatch of N(0, I) draws.
    ``forward`` returns (z, loss[B], artifacts) with loss[b] = OT cost (identical for every b so that the VAE's
    ``prior_loss.mean()`` equals it).

    The loss VALUE is the reference's own composition (``sinkhorn_log`` on C / max C, read-out sum(C * pi): ot/w2_utils.py:265-269,
    276-319).  Its GRADIENT comes in two conventions, and they are NOT close:

    * ``differentiate_plan=False`` (default, the training configuration of BASELINE configs 2-3): the envelope form -- the plan is
      a constant, d loss / d z_i = 2 sum_j pi_ij (z_i - y_j).  This is what the composition gives when the solve runs under
      ``torch.no_grad()``; it is the gradient of the converged OT cost and is cheap (one plan-times-samples product).
    * ``differentiate_plan=True``: what autograd gives for the composition of the reference's functions as written -- the
      gradient also flows through the cost normalisation and through all ``max_iter`` iterations of ``sinkhorn_log``
      (``ot.sinkhorn_log``'s backward, csrc/sinkhorn_diff.hip).  With reg = 0.05 and 50 iterations on a max-normalised cost the plan
      is far from converged and the two gradients differ by 37 % (N = 7), 93 % (N = 64), 97 % (N = 256) of the gradient's
      largest entry on the recorded problems (tests/golden/sinkhorn_autograd.npz: ``gz_full`` vs ``gz_envelope``, both from the
      reference's function).  Costs 2 max_iter + 5 extra launches per step and runs on the launch stream."""

    def __init__(self, reg: float = 0.05, max_iter: int = 50, threshold: float = 0., loss_coeff: float = 1.,
                 annealing_steps: int = 0, seed: int = None, differentiate_plan: bool = False):
        super().__init__(loss_coeff, annealing_steps)
        self.reg, self.max_iter, self.threshold = reg, max_iter, threshold
        self.seed = seed
        self.differentiate_plan = bool(differentiate_plan)
        self.last_iters = None  # device int32: iterations of the last solve (-1: the solver was starved, loss is NaN)

    def raise_if_starved(self) -> None:
        """Host check of the last solve (one device read): raises ``SinkhornSolverStarved`` if the single-launch solver gave up
        waiting for its other workgroups.  The training step itself never synchronises for this: a starved solve makes the
        loss NaN (every entry of the plan is), which is what a captured step can show; ``HipTrainer.close`` and callers that
        log losses call this."""
        if self.last_iters is not None:
            W.raise_if_solver_starved(self.last_iters)

    def _draw(self, like: Tensor) -> Tensor:
        """prior samples N(0, I) from the device-side counter-based generator: inside a captured step every replay draws
        fresh samples (the call counter lives in device memory and advances in the kernel)"""
        from .. import functional as HF
        return HF.normal_like(like, self._key(like.device), stream_id=1)

    def forward(self, x: Tensor, step: int, prior_samples: Optional[Tensor] = None) -> Prior.EncodingResults:
        return super().forward(x, step, prior_samples=prior_samples)

    def encode(self, x: Tensor, prior_samples: Optional[Tensor] = None, _scale: float = 1.0) -> Prior.EncodingResults:
        z = x
        zf = z.flatten(1)
        if prior_samples is None:
            prior_samples = self._draw(zf) if zf.dtype == torch.float32 else torch.randn_like(zf)
        if self.differentiate_plan and torch.is_grad_enabled() and zf.requires_grad:
            y = prior_samples.flatten(1).to(zf.dtype)
            n, m = zf.shape[0], y.shape[0]
            C = W.sq_euclidean_cost(zf, y)                     # differentiable (plan-times-samples kernel in its backward)
            Cn = C / C.amax()                                  # the maximum takes part in the gradient, as under autograd
            a = torch.full((n,), 1.0 / n, device=zf.device, dtype=zf.dtype)
            b = torch.full((m,), 1.0 / m, device=zf.device, dtype=zf.dtype)
            pi = W.sinkhorn_log(a, b, Cn, self.reg, self.max_iter, self.threshold)   # carries _SinkhornLogFn's backward
            loss = ((C * pi).sum() * _scale).expand(n)
            self.last_iters = None
            return z, loss, {"prior_samples": prior_samples}
        y = prior_samples.flatten(1)
        cfg, scale = (float(self.reg), int(self.max_iter), float(self.threshold)), float(_scale)

        def run():
            cost, pi, iters = torch.ops.otvae.sinkhorn_prior(zf, y, *cfg, scale)
            return cost, (zf, y, pi), (iters,)

        z_out, loss, self.last_iters = _LatentLossFn.apply(
            zf, run, lambda g, gadd, z_, y_, pi: torch.ops.otvae.sinkhorn_prior_backward(g, gadd, z_, y_, pi, scale), y)
        return z_out.view(z.shape), loss, {"prior_samples": prior_samples}
