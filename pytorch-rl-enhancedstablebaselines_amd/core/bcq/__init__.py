from core.bcq.bcq import BCQ
from core.bcq.policies import BCQPolicy, MlpPolicy

__all__ = ["BCQ", "BCQPolicy", "MlpPolicy"]
