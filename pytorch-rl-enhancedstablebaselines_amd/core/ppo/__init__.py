from core.ppo.policies import MlpPolicy
from core.ppo.ppo import PPO

__all__ = ["PPO", "MlpPolicy"]
