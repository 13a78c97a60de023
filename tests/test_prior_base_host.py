"""Host: what the minibatch priors share (``prior/base.py``: ``MinibatchPrior`` and the one pass-through loss node)."""
import inspect

import pytest
import torch

import ot_vae_lightning_amd as A
from ot_vae_lightning_amd.utils import hasarg

KEYWORDS = {"SinkhornPrior": ["prior_samples"], "SlicedWassersteinPrior": ["prior_samples", "projections"],
            "MMDPrior": ["prior_samples"], "GaussianW2Prior": []}


@pytest.mark.parametrize("name", sorted(KEYWORDS))
def test_forward_names_the_keywords_the_vae_may_hand_over(name):
    """``VAE.encode`` passes a keyword on only when the prior's ``forward`` signature names it: a draw handed in must not be dropped"""
    prior = getattr(A, name)()
    assert isinstance(prior, A.MinibatchPrior) and isinstance(prior, A.Prior)
    for key in ("prior_samples", "projections", "eps", "labels"):
        assert hasarg(prior, key) == (key in KEYWORDS[name]), key
    assert prior.out_size((16, 1, 1)) == (16, 1, 1) and prior.sample((3, 16), "cpu").shape == (3, 16)
    assert "_rng_key" not in prior.state_dict() and "_rng_key" not in dict(prior.named_buffers())


def test_gaussian_w2_prior_refuses_an_unknown_keyword():
    with pytest.raises(TypeError, match="prior_samples"):
        A.GaussianW2Prior()(torch.zeros(9, 4), step=0, prior_samples=torch.zeros(9, 4))


def test_the_priors_share_one_autograd_node():
    from ot_vae_lightning_amd import prior
    nodes = {obj for mod in vars(prior).values() if inspect.ismodule(mod) for obj in vars(mod).values()
             if inspect.isclass(obj) and issubclass(obj, torch.autograd.Function) and obj.__module__.startswith(prior.__name__)}
    assert nodes == {prior.base._LatentLossFn}
