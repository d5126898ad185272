"""Float64 reference (torch, CPU) of the CvT model (models/cvt.py:10-171) and of its convolutional
token embedding: ``F.conv2d`` on explicitly SAME-padded input, LayerNorm, the stage blocks around the
convolutional projections of _conv_proj_ref.py, the zero-initialised head; gradients by float64
autograd.  ``mode="bf16"`` rounds where the kernels round (the staged input, the kernel at the compute
dtype, each op's output); the roundings are straight-through for autograd, so a gradient is the
float64 gradient of the rounded forward.

Parameters come as the Flax tree of ``layers.flax_params`` (nested dicts of float64 tensors), the
BatchNorm statistics as ``{module path: (mean, var)}``; a training forward returns the moved ones."""
import math

import torch
import torch.nn.functional as F

import _conv_proj_ref as P

LN_EPS = 1e-6


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.to(torch.bfloat16).to(torch.float64)

    @staticmethod
    def backward(ctx, g):
        return g


def rnd(x, mode):
    return _Round.apply(x) if mode == "bf16" else x


def same_pads(n, k, s):
    return P.same_pads(n, k, s)


def pad_same(x, k, s):
    """x [B, H, W, C] zero-padded for a k x k window at stride s (Flax SAME)."""
    (pt, pb), (pl, pr) = same_pads(x.shape[1], k, s), same_pads(x.shape[2], k, s)
    return F.pad(x, (0, 0, pl, pr, pt, pb))


def conv_tokens(x, w, b, k, s, mode="f64"):
    """x [B, H, W, Cin], w [k, k, Cin, E] (Flax), b [E] or None -> [B, Ho Wo, E]."""
    xp = pad_same(rnd(x, mode), k, s).permute(0, 3, 1, 2)
    y = F.conv2d(xp, rnd(w, mode).permute(3, 2, 0, 1), b, stride=s).permute(0, 2, 3, 1)
    return rnd(y.reshape(y.shape[0], -1, y.shape[3]), mode)


def window_matrix(x, k, s):
    """The unfold of the padded input: [B Ho Wo, k k Cin], column (ky k + kx) Cin + c."""
    B, H, W, C = x.shape
    Ho, Wo = math.ceil(H / s), math.ceil(W / s)
    xp = pad_same(x, k, s)
    taps = [xp[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s, :] for ky in range(k) for kx in range(k)]
    return torch.stack(taps, dim=3).reshape(B * Ho * Wo, k * k * C)


def window_fold(dP, shape, k, s):
    """The transpose of window_matrix: dP [B Ho Wo, k k Cin] -> [B, H, W, Cin]."""
    B, H, W, C = shape
    Ho, Wo = math.ceil(H / s), math.ceil(W / s)
    (pt, pb), (pl, pr) = same_pads(H, k, s), same_pads(W, k, s)
    dxp = torch.zeros((B, H + pt + pb, W + pl + pr, C), dtype=dP.dtype)
    d = dP.reshape(B, Ho, Wo, k, k, C)
    for ky in range(k):
        for kx in range(k):
            dxp[:, ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s, :] += d[:, :, :, ky, kx, :]
    return dxp[:, pt:pt + H, pl:pl + W, :]


def layer_norm(x, p, mode="f64"):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return rnd((x - mu) / torch.sqrt(var + LN_EPS) * p["scale"] + p["bias"], mode)


def gelu(x):   # Flax nn.gelu default: the tanh approximation
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


def zero_pad_and_reshape(x):
    b, l, c = x.shape
    S = math.isqrt(l)
    S = S if S * S == l else S + 1
    return F.pad(x, (0, 0, 0, S * S - l)).reshape(b, S, S, c)


def conv_projection(x, p, stats, stride, training, momentum, eps, mode):
    """ConvProjectionBlock (cvt_attention.py:12-40) -> (y [B, Ho, Wo, out], moved (mean, var))."""
    fw = P.forward(rnd(x, mode), p["Conv_0"]["kernel"], p["BatchNorm_0"]["scale"], p["BatchNorm_0"]["bias"], stride,
                   eps, mode, stats=None if training else stats)
    if training:
        stats = P.running(stats[0], stats[1], fw["mu"].detach(), fw["var"].detach(), momentum)
    w1 = rnd(p["Conv_1"]["kernel"].reshape(x.shape[-1], -1), mode)
    return rnd(fw["y"] @ w1, mode), stats


def attention(grid, p, stats, path, heads, training, momentum, eps, mode, new_stats):
    """CvTSelfAttentionBlock (cvt_attention.py:43-120), strides (1, 2, 2), no bias."""
    outs = []
    for i, s in enumerate((1, 2, 2)):
        name = f"ConvProjectionBlock_{i}"
        y, st = conv_projection(grid, p[name], stats[f"{path}.{name}.BatchNorm_0"], s, training, momentum, eps, mode)
        new_stats[f"{path}.{name}.BatchNorm_0"] = st
        outs.append(y.reshape(y.shape[0], -1, heads, y.shape[-1] // heads))
    q, k, v = outs
    D = q.shape[-1]
    w = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(D), dim=-1)
    o = rnd(torch.einsum("bhqk,bkhd->bqhd", w, v), mode)
    return rnd(torch.einsum("bqhd,hdo->bqo", o, rnd(p["DenseGeneral_0"]["kernel"], mode)), mode)


def dense(x, p, mode):
    return rnd(x @ rnd(p["kernel"], mode) + p["bias"], mode)


def stage_block(x, p, stats, path, heads, training, momentum, eps, mode, new_stats):
    grid = zero_pad_and_reshape(x)
    a = attention(grid, p["CvTSelfAttentionBlock_0"], stats, f"{path}.CvTSelfAttentionBlock_0", heads, training,
                  momentum, eps, mode, new_stats)
    x = a + grid.reshape(grid.shape[0], -1, grid.shape[3])
    y = layer_norm(x, p["LayerNorm_0"], mode)
    y = dense(rnd(gelu(dense(y, p["FFBlock_0"]["Dense_0"], mode)), mode), p["FFBlock_0"]["Dense_1"], mode)
    return x + y


def cvt(images, params, stats, stage_sizes, num_heads, embed_kernel_size=(7, 3, 3), embed_strides=(4, 2, 2),
        training=True, momentum=0.9, eps=1e-5, mode="f64"):
    """models/cvt.py:116-171 -> (logits [B, classes], the BatchNorm statistics after the call)."""
    x, new_stats, n = images, {}, len(stage_sizes)
    for i in range(n):
        p = params[f"Stage_{i}"]
        e = p["ConvTokenEmbedBlock_0"]
        x = conv_tokens(x, e["Conv_0"]["kernel"], e["Conv_0"]["bias"], embed_kernel_size[i], embed_strides[i], mode)
        x = layer_norm(x, e["LayerNorm_0"], mode)
        if i == n - 1:
            x = torch.cat([p["cls"].expand(x.shape[0], 1, x.shape[2]), x], dim=1)
        for j in range(stage_sizes[i]):
            x = stage_block(x, p[f"StageBlock_{j}"], stats, f"Stage_{i}.StageBlock_{j}", num_heads[i], training,
                            momentum, eps, mode, new_stats)
        if i < n - 1:
            S = math.isqrt(x.shape[1])
            x = x.reshape(x.shape[0], S, S, x.shape[2])
    head = params["Dense_0"]
    return dense(x[:, 0], head, mode), new_stats
