"""CQL's policy is SAC's `SACPolicy` itself (same modules, same construction order, same state_dict and seeded initial weights):
`MlpPolicy` only."""
from core.sac.policies import SACPolicy

CQLPolicy = SACPolicy
MlpPolicy = SACPolicy
