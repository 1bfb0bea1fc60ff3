from .ema import EMA, PowerEMA
from .losses import LossFunction, RepaLoss
from .optim import FusedAdamW, FusedArenaOptimizer, FusedMuon, FusedSGD
from .trainers import BaseTrainer, Trainer
from .utils import AverageMeter

__all__ = ["FusedAdamW", "FusedSGD", "FusedMuon", "FusedArenaOptimizer", "AverageMeter", "EMA", "PowerEMA", "BaseTrainer", "Trainer", "LossFunction", "RepaLoss"]
