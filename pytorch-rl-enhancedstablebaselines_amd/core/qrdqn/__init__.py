from core.qrdqn.policies import MlpPolicy, QRDQNPolicy, QuantileNetwork
from core.qrdqn.qrdqn import QRDQN

__all__ = ["QRDQN", "QRDQNPolicy", "MlpPolicy", "QuantileNetwork"]
