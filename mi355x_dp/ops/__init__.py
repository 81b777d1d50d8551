"""Native gfx950 ops (HIP kernels in csrc/kernels) with autograd support."""
from .functional import (  # noqa: F401
    MixedTarget, adamw_flat_, adamw_prep_, augment, augment_mix, augment_resized, batch_norm_act, cast_bf16_, checksum, conv2d,
    cross_entropy, ema_prep_, ema_swap_, ema_update_, global_avg_pool,
    grad_sqnorm_, lamb_apply_, lamb_moments_, lamb_prep_, lamb_trust_, lars_flat_, lars_trust_, linear, max_pool2d,
    seg_sqnorm_reduce_, seg_sqnorm_units_, sgd_flat_, weight_bf16,
)
from ._lib import available as native_available  # noqa: F401
