from core.her.goal_selection_strategy import GoalSelectionStrategy
from core.her.her_replay_buffer import HerReplayBuffer

__all__ = ["GoalSelectionStrategy", "HerReplayBuffer"]
