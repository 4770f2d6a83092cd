from core.ars.ars import ARS
from core.ars.policies import ARSLinearPolicy, ARSPolicy, LinearPolicy, MlpPolicy

__all__ = ["ARS", "ARSPolicy", "ARSLinearPolicy", "MlpPolicy", "LinearPolicy"]
