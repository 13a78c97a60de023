"""ot_vae_lightning_amd -- the training-step hot path of theoad/ot-vae-lightning, rebuilt for AMD Instinct MI355X
(gfx950): hand-written HIP kernels behind a C ABI (``include/otvae.h``, ``libotvae_hip.so``) and the reference's own
plug-in API on top (``networks.CNN``, ``prior.GaussianPrior``, ``model.VAE``, ``ot.sinkhorn_log``,
``ot.GaussianTransport`` ...).  There is no CPU execution path: see DESIGN.md."""
from . import _lib  # noqa: F401
from .networks import *  # noqa: F401,F403
from .prior import *  # noqa: F401,F403
from .model import *  # noqa: F401,F403
from .ot import *  # noqa: F401,F403
from .engine import *  # noqa: F401,F403
from . import metrics  # noqa: F401
from . import losses  # noqa: F401
from .losses import *  # noqa: F401,F403
from .losses import MSSSIMLoss, ms_ssim_loss  # noqa: F401
from . import transforms  # noqa: F401
from .transforms import *  # noqa: F401,F403
from .utils import Collage  # noqa: F401

__version__ = "0.1.0"
