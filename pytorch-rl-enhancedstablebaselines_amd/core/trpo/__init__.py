from core.trpo.policies import MlpPolicy
from core.trpo.trpo import TRPO

__all__ = ["TRPO", "MlpPolicy"]
