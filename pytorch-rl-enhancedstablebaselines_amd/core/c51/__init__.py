from core.c51.c51 import C51
from core.c51.policies import C51Policy, CategoricalNetwork, MlpPolicy

__all__ = ["C51", "C51Policy", "MlpPolicy", "CategoricalNetwork"]
