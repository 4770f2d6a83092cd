"""reference: core/a2c/policies.py -- A2C's policy aliases (the CNN and dict-observation policies are out of scope)."""
from core.common.policies import ActorCriticPolicy

MlpPolicy = ActorCriticPolicy
