from ._ext import ext, have_ext  # noqa: F401
from .functional import (  # noqa: F401
    batch_norm,
    compute_dtype,
    conv2d,
    cross_entropy,
    gather_augment,
    global_avg_pool,
    grad_stats,
    lars_plan,
    lars_stats,
    lars_step,
    linear,
    max_pool2d,
    scaler_update,
    sgd_step,
    sgd_step_guarded,
)
