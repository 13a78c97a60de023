from .base import *  # noqa: F401,F403
from .vae import *  # noqa: F401,F403
from .discrete_auto_diffuser import *  # noqa: F401,F403
from .auto_diffusion import *  # noqa: F401,F403
