from core.a2c.a2c import A2C
from core.a2c.policies import MlpPolicy, MultiInputPolicy

__all__ = ["A2C", "MlpPolicy", "MultiInputPolicy"]
