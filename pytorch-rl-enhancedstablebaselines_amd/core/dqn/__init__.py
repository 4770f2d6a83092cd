from core.dqn.dqn import DQN
from core.dqn.policies import DQNPolicy, MlpPolicy, QNetwork

__all__ = ["DQN", "DQNPolicy", "MlpPolicy", "QNetwork"]
