from core.cql.cql import CQL
from core.cql.policies import CQLPolicy, MlpPolicy

__all__ = ["CQL", "CQLPolicy", "MlpPolicy"]
