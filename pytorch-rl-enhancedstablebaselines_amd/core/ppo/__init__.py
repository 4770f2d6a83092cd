from core.ppo.policies import MlpPolicy, MultiInputPolicy
from core.ppo.ppo import PPO

__all__ = ["PPO", "MlpPolicy", "MultiInputPolicy"]
