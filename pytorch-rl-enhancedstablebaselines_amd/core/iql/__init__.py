from core.iql.iql import IQL
from core.iql.policies import IQLPolicy, MlpPolicy

__all__ = ["IQL", "IQLPolicy", "MlpPolicy"]
