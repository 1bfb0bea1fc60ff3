"""Sampler plugin interface (reference diffuse/samplers/common.py:7-32)."""

from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Any, TypedDict

from torch import Tensor

try:
    from typing import NotRequired, Required
except ImportError:
    from typing_extensions import NotRequired, Required


class StepResult(TypedDict):
    x_prev: Required[Tensor]
    estimated_x0: Required[Tensor]
    x_prev_mean: NotRequired[Tensor]
    x_prev_std: NotRequired[Tensor]
    logprob: NotRequired[Tensor]


class Sampler(ABC):
    name: str
    # a multistep sampler (this project's) keeps one tensor of the previous step; the Gaussian loop hands it the step's host index
    multistep: bool = False

    def __init__(self) -> None:
        pass

    def reset(self) -> None:
        """forget the previous step (the loops call it once before they start); nothing to forget for a single-step sampler"""

    @abstractmethod
    def set_steps(self, *args: Any, **kwargs: Any) -> None: ...

    @abstractmethod
    def step(self, *args: Any, **kwargs: Any) -> StepResult: ...
