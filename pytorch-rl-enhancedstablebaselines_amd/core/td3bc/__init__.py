from core.td3bc.policies import MlpPolicy, TD3BCPolicy
from core.td3bc.td3bc import TD3BC

__all__ = ["TD3BC", "TD3BCPolicy", "MlpPolicy"]
