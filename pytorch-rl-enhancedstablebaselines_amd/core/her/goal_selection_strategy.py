"""reference: core/her/goal_selection_strategy.py"""
from enum import Enum


class GoalSelectionStrategy(Enum):
    """The strategies for selecting new goals when creating artificial transitions."""

    FUTURE = 0   # a goal achieved after the current step, in the same episode
    FINAL = 1    # the goal achieved at the end of the episode
    EPISODE = 2  # a goal achieved in the episode


KEY_TO_GOAL_STRATEGY = {
    "future": GoalSelectionStrategy.FUTURE,
    "final": GoalSelectionStrategy.FINAL,
    "episode": GoalSelectionStrategy.EPISODE,
}
