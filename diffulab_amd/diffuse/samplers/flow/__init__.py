from .ab2 import AB2
from .euler import Euler
from .euler_maruyama import EulerMaruyama

__all__ = ["AB2", "Euler", "EulerMaruyama"]
