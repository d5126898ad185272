"""Float64 reference (torch, CPU) of the CeiT locally-enhanced feed-forward
(models/layers/feedforwards/leff.py:9-63): BatchNorm over token rows + tanh-GELU with the hand-written
backward the kernels of csrc/bn_rows.h implement, the running-statistics recurrence, and the whole
block as plain differentiable float64 math.  ``mode="bf16"`` emulates the two compute-dtype roundings
of the kernel (z, the BatchNorm output, and y); x and dy are taken as given (the caller passes
bf16-representable values)."""
import math

import torch
import torch.nn.functional as F

GELU_B, GELU_K = math.sqrt(2.0 / math.pi), 0.044715


def same_pads(n, k, s):
    """ops.same_pads: Flax SAME padding (low, high)."""
    out = math.ceil(n / s)
    total = max((out - 1) * s + k - n, 0)
    return total // 2, total - total // 2


def rnd(x, mode):
    return x.to(torch.bfloat16).to(torch.float64) if mode == "bf16" else x


def gelu(z):
    return 0.5 * z * (1.0 + torch.tanh(GELU_B * (z + GELU_K * z ** 3)))


def dgelu(z):
    t = torch.tanh(GELU_B * (z + GELU_K * z ** 3))
    return 0.5 * (1.0 + t) + 0.5 * z * (1.0 - t * t) * GELU_B * (1.0 + 3.0 * GELU_K * z * z)


def bn_gelu_forward(x, gamma, beta, eps, mode="f64", stats=None):
    """x [N, C]: the participating rows.  Training (stats None: biased batch statistics) or evaluation
    (stats = (mean, var)).  Everything float64; returns mu, var, r, xh, z, y."""
    if stats is None:
        mu, var = x.mean(0), x.var(0, unbiased=False)
    else:
        mu, var = stats
    r = 1.0 / torch.sqrt(var + eps)
    xh = (x - mu) * r
    z = rnd(xh * gamma + beta, mode)
    return dict(mu=mu, var=var, r=r, xh=xh, z=z, y=rnd(gelu(z), mode))


def bn_gelu_backward(gamma, fw, g):
    """The formulas of the kernels, given the forward's dict fw and g = dL/dy [N, C]."""
    N = g.shape[0]
    dz = g * dgelu(fw["z"])
    dbeta = dz.sum(0)
    dgamma = (dz * fw["xh"]).sum(0)
    dx = gamma * fw["r"] * (dz - dbeta / N - fw["xh"] * dgamma / N)
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta)


def running(mean, var, mu, sigma2, momentum):
    """Flax: ra = momentum * ra + (1 - momentum) * batch."""
    return momentum * mean + (1 - momentum) * mu, momentum * var + (1 - momentum) * sigma2


PARAMS = ("Dense_0.kernel", "Dense_0.bias", "BatchNorm_0.scale", "BatchNorm_0.bias", "Conv_0.kernel", "Conv_0.bias",
          "BatchNorm_1.scale", "BatchNorm_1.bias", "Dense_1.kernel", "Dense_1.bias", "BatchNorm_2.scale",
          "BatchNorm_2.bias")


def leff_block(inputs, p, k, eps, stats=None):
    """The whole block, differentiable float64: inputs [B, 1 + L, C], p a dict over PARAMS (Flax
    layouts: Dense kernel [in, out], Conv kernel [k, k, in, out]), stats None (training) or three
    (mean, var) pairs.  Returns the output [B, 1 + L, C], the three (mu, var) of the batch and the three
    BatchNorm inputs (a caller that wants their gradients calls retain_grad on them)."""
    cls, tokens = inputs[:, :1], inputs[:, 1:]
    B, L, C = tokens.shape
    S = math.isqrt(L)
    batch, bn_in = [], []

    def bn_act(h, i):
        bn_in.append(h)
        flat = h.reshape(-1, h.shape[-1])
        if stats is None:
            mu, var = flat.mean(0), flat.var(0, unbiased=False)
        else:
            mu, var = stats[i]
        batch.append((mu.detach(), var.detach()))
        return gelu((h - mu) / torch.sqrt(var + eps) * p[f"BatchNorm_{i}.scale"] + p[f"BatchNorm_{i}.bias"])

    h = bn_act(tokens @ p["Dense_0.kernel"] + p["Dense_0.bias"], 0)
    (pt, pb), (pl, pr) = same_pads(S, k, 1), same_pads(S, k, 1)
    hp = F.pad(h.reshape(B, S, S, -1).permute(0, 3, 1, 2), (pl, pr, pt, pb))
    h = F.conv2d(hp, p["Conv_0.kernel"].permute(3, 2, 0, 1), p["Conv_0.bias"]).permute(0, 2, 3, 1).reshape(B, L, -1)
    h = bn_act(h, 1)
    h = bn_act(h @ p["Dense_1.kernel"] + p["Dense_1.bias"], 2)
    return torch.cat([cls, h], dim=1), batch, bn_in
