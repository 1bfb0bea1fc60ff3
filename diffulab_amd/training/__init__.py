from .ema import EMA
from .losses import LossFunction, RepaLoss
from .optim import FusedAdamW, FusedArenaOptimizer, FusedSGD
from .trainers import BaseTrainer, Trainer
from .utils import AverageMeter

__all__ = ["FusedAdamW", "FusedSGD", "FusedArenaOptimizer", "AverageMeter", "EMA", "BaseTrainer", "Trainer", "LossFunction", "RepaLoss"]
