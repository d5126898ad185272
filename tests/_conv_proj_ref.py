"""Float64 reference (torch, CPU) of the CvT convolutional projection in front of its 1x1
convolution (cvt_attention.py:21-36): depthwise 3x3 convolution with Flax SAME padding, BatchNorm
in training and evaluation, the running-statistics recurrence, and the hand-written backward the
kernels implement.  ``mode="bf16"`` emulates the two compute-dtype roundings (of the conv output t
and of y) and the kernel used at the compute dtype; x and dy are taken as given (the caller passes
bf16-representable values)."""
import math

import torch
import torch.nn.functional as F


def same_pads(n, k, s):
    out = math.ceil(n / s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def rnd(x, mode):
    return x.to(torch.bfloat16).to(torch.float64) if mode == "bf16" else x


def pad(x, s):
    """x [B, H, W, C] -> zero-padded xp and the output extent."""
    (pt, pb), (pl, pr) = same_pads(x.shape[1], 3, s), same_pads(x.shape[2], 3, s)
    return F.pad(x, (0, 0, pl, pr, pt, pb)), math.ceil(x.shape[1] / s), math.ceil(x.shape[2] / s)


def conv(x, w, s):
    """Depthwise 3x3 of x [B, H, W, C] with w [3, 3, 1, C] at stride s (SAME) -> [B, Ho, Wo, C]."""
    C = x.shape[-1]
    xp, _, _ = pad(x, s)
    k = w.permute(3, 2, 0, 1)   # [C, 1, 3, 3]
    return F.conv2d(xp.permute(0, 3, 1, 2), k, stride=s, groups=C).permute(0, 2, 3, 1)


def forward(x, w, gamma, beta, s, eps, mode="f64", stats=None, round_t=True):
    """Training (stats None: biased batch statistics of the rounded t) or evaluation (stats = (mean,
    var)).  Everything float64; returns t, mu, var, r, xhat, y."""
    t = conv(x, rnd(w, mode), s)
    if round_t:
        t = rnd(t, mode)
    if stats is None:
        mu, var = t.mean((0, 1, 2)), t.var((0, 1, 2), unbiased=False)
    else:
        mu, var = stats
    r = 1.0 / torch.sqrt(var + eps)
    xh = (t - mu) * r
    return dict(t=t, mu=mu, var=var, r=r, xh=xh, y=rnd(xh * gamma + beta, mode))


def backward(x, w, gamma, fw, g, s, mode="f64"):
    """The formulas of the kernels, given the forward's dict fw and g = dL/dy."""
    N = g.shape[0] * g.shape[1] * g.shape[2]
    dbeta = g.sum((0, 1, 2))
    dgamma = (g * fw["xh"]).sum((0, 1, 2))
    dt = gamma * fw["r"] * (g - dbeta / N - fw["xh"] * dgamma / N)
    xp, Ho, Wo = pad(x, s)
    wr = rnd(w, mode)
    dw = torch.zeros_like(w)
    dxp = torch.zeros_like(xp)
    for i in range(3):
        for j in range(3):
            rows, cols = slice(i, i + s * (Ho - 1) + 1, s), slice(j, j + s * (Wo - 1) + 1, s)
            dw[i, j, 0] = (xp[:, rows, cols, :] * dt).sum((0, 1, 2))
            dxp[:, rows, cols, :] += wr[i, j, 0] * dt
    pt, pl = same_pads(x.shape[1], 3, s)[0], same_pads(x.shape[2], 3, s)[0]
    dx = dxp[:, pt:pt + x.shape[1], pl:pl + x.shape[2], :]
    return dict(dx=dx, dw=dw, dgamma=dgamma, dbeta=dbeta, dt=dt)


def running(mean, var, mu, sigma2, momentum):
    """Flax: ra = momentum * ra + (1 - momentum) * batch."""
    return momentum * mean + (1 - momentum) * mu, momentum * var + (1 - momentum) * sigma2
