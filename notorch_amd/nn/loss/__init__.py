from notorch_amd.nn.loss.rnc import CDist, PNorm, RankNContrastLoss, RnCRankFunction

__all__ = ["RankNContrastLoss", "CDist", "PNorm", "RnCRankFunction"]
