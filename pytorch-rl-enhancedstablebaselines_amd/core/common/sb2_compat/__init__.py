"""Optimisers kept for parity with the original (TensorFlow) stable-baselines: `RMSpropTFLike`."""
from core.common.sb2_compat.rmsprop_tf_like import RMSpropTFLike

__all__ = ["RMSpropTFLike"]
