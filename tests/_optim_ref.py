"""Float64 numpy restatement of the reference's optimizer chain (reference train.py:25-27, 215-220):

    optax.chain(clip_by_global_norm(max_norm), scale_by_adam(), additive_weight_decay(wd),
                scale_by_schedule(warmup_cosine_decay_schedule(init, peak, warmup, decay, end)))

as the package applies it (survey D9: descent; torch.optim.AdamW's order of operations, which
csrc/adamw.h documents).  The tests of the clip / schedule kernels compare against these functions;
nothing here is imported by the package."""
import math

import numpy as np


def warmup_cosine(count, init, peak, warmup_steps, decay_steps, end):
    """optax.warmup_cosine_decay_schedule at ``count`` (the number of updates already applied):
    linear_schedule(init, peak, warmup_steps) joined at warmup_steps with
    cosine_decay_schedule(peak, decay_steps - warmup_steps, alpha = end / peak)."""
    count = int(count)
    if count < warmup_steps:
        return np.float64(init) + (np.float64(peak) - np.float64(init)) * count / warmup_steps
    D = decay_steps - warmup_steps
    c = min(count - warmup_steps, D)
    alpha = np.float64(end) / np.float64(peak)
    return np.float64(peak) * ((1.0 - alpha) * 0.5 * (1.0 + math.cos(math.pi * c / D)) + alpha)


def global_norm(arrays):
    """optax.global_norm: sqrt of the sum of squares over every array, in float64."""
    return np.sqrt(sum(np.square(np.asarray(a, np.float64)).sum() for a in arrays))


def clip_scale(norm, max_norm):
    """optax.clip_by_global_norm as one factor: 1 below max_norm, max_norm / norm from max_norm on
    (a zero norm is below every positive max_norm)."""
    norm = np.float64(norm)
    return np.float64(1.0) if norm < max_norm else np.float64(max_norm) / norm


def adamw_step(p, g, m, v, t, lr, scale=1.0, b1=0.9, b2=0.999, eps=1e-8, wd=1e-4):
    """One update of the arrays p, m, v in place with the gradient g * scale, t = the update's
    number counted from 1:  p *= 1 - lr wd;  m, v moments;  p -= lr / (1 - b1^t) m / (sqrt(v / (1 - b2^t)) + eps).
    Every operation runs in p's dtype: float64 arrays give the reference, float32 arrays the
    helper's own fp32 execution (the yardstick for what fp32 rounding alone costs)."""
    f = p.dtype.type
    g = np.asarray(g, p.dtype) * f(scale)
    p *= f(1.0) - f(lr) * f(wd)
    m += (f(1.0) - f(b1)) * (g - m)
    v *= f(b2)
    v += (f(1.0) - f(b2)) * g * g
    step_size = f(lr) / (f(1.0) - f(b1) ** f(t))
    p -= step_size * (m / (np.sqrt(v) / np.sqrt(f(1.0) - f(b2) ** f(t)) + f(eps)))
