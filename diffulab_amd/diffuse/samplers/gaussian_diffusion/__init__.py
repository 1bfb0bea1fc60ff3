from .ddim import DDIM
from .ddpm import DDPM
from .dpmpp_2m import DPMSolverPP2M

__all__ = ["DDIM", "DDPM", "DPMSolverPP2M"]
