"""reference: core/a2c/policies.py -- A2C's policy aliases (the CNN policies are out of scope)."""
from core.common.policies import ActorCriticPolicy, MultiInputActorCriticPolicy

MlpPolicy = ActorCriticPolicy
MultiInputPolicy = MultiInputActorCriticPolicy
