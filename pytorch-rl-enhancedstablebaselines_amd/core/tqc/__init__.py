from core.tqc.policies import MlpPolicy, QuantileCritic, TQCPolicy
from core.tqc.tqc import TQC

__all__ = ["TQC", "TQCPolicy", "QuantileCritic", "MlpPolicy"]
