from core.ppo_recurrent.buffers import RecurrentRolloutBuffer, segment_tables
from core.ppo_recurrent.policies import MlpLstmPolicy
from core.ppo_recurrent.ppo_recurrent import RecurrentPPO

__all__ = ["RecurrentPPO", "MlpLstmPolicy", "RecurrentRolloutBuffer", "segment_tables"]
