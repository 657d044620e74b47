from notorch_amd.nn.loss.loss import (
    BCE,
    MSE,
    MVE,
    XENT,
    BinaryCrossEntropy,
    BoundedMSE,
    CrossEntropy,
    Dirichlet,
    Evidential,
    MeanVarianceEstimation,
    SelfSupervisedLoss,
    TaskLossFunction,
)
from notorch_amd.nn.loss.rnc import CDist, PNorm, RankNContrastLoss, RnCRankFunction

__all__ = [
    "SelfSupervisedLoss",
    "MSE",
    "BoundedMSE",
    "MeanVarianceEstimation",
    "MVE",
    "Evidential",
    "BinaryCrossEntropy",
    "BCE",
    "CrossEntropy",
    "XENT",
    "Dirichlet",
    "TaskLossFunction",
    "RankNContrastLoss",
    "CDist",
    "PNorm",
    "RnCRankFunction",
]
