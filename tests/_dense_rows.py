"""One pinned ``ops.dense`` call per route and per edge of the Dense plans (ops.dense_fwd_plan /
dense_bwd_plan): the facts of the call in, the route names out.  Shared by tests/test_dense_plan_cpu.py
and, for the production widths, tests/test_routing_cpu.py.

Every expectation is read off the branch cascade of ``_Dense.forward`` / ``_Dense.backward`` that the plans
replaced (aligned contiguous operands, fp32 parameters), not off the plans' output:
  * forward: exact fp32 on sae_gemm_f32 if x and W are fp32 operands (widths % 4); else sae_gemm_nt if a
    bf16 W^T exists, I % 8 == 0 and J % 8 == 0, and GEMM_LIB is off or M <= SMALL_M; else the library;
  * dX: fp32 as the forward; else sae_gemm_nt if GEMM_LIB is off and I % 8 == 0 and J % 8 == 0; else, if the
    forward kept W^T (bf16, J % 8 != 0, M <= SMALL_M) and dY^T [J, M] is an sae_gemm_dw operand
    (M % 8 == 0, I % 8 == 0), sae_gemm_dw over the rows of dY^T and W^T; else the library;
  * dW: fp32 as the forward; else the library unless x and dY are sae_gemm_dw operands (I % 8, J % 8); one
    kernel: into its sink or a fresh buffer; several of one width % 4 == 0: one blocked launch, into the
    sinks if every block has one and they are adjacent, else into a fresh buffer (sinks of single blocks
    are left to autograd); any other blocks: one fresh [I, J], sliced, the bias sink ignored;
  * offload: a launch that writes a weight sink, and a bias sink or no bias at all.
``keep_wt`` differs from that cascade in one row on purpose: the forward used to keep W^T at any M <= SMALL_M
and the backward then found dY^T's pitch (M = 20) unusable; the plan does not keep it there."""
import torch

import sae_vision_amd.ops as ops

BF16, F32 = torch.bfloat16, torch.float32
ALL_LIB = ("lib", False), ("lib", "lib", False)

# (id, dense_facts_of_shapes arguments, GEMM_LIB, (forward route, keep_wt), (dx, dw, offload))
ROWS = [
    ("single", dict(M=256, I=64, widths=(128,)), False, ("nt", False), ("nt", "dw", False)),
    ("blocks", dict(M=256, I=64, widths=(64, 64, 64)), False, ("nt", False), ("nt", "dw_blocks", False)),
    ("blocks_adjacent_sinks", dict(M=256, I=64, widths=(64, 64, 64), sinks_w=(True, True, True), sink_b=True), False,
     ("nt", False), ("nt", "dw_blocks_sunk", True)),
    ("blocks_apart_sinks", dict(M=256, I=64, widths=(64, 64, 64), sinks_w=(True, True, True), sink_b=True,
                                adjacent=False), False, ("nt", False), ("nt", "dw_blocks", False)),
    ("blocks_some_sinks", dict(M=256, I=64, widths=(64, 64, 64), sinks_w=(True, False, True)), False,
     ("nt", False), ("nt", "dw_blocks", False)),
    ("unequal_blocks", dict(M=256, I=64, widths=(64, 32)), False, ("nt", False), ("nt", "dw_stacked", False)),
    ("unequal_blocks_sinks", dict(M=256, I=64, widths=(64, 32), sinks_w=(True, True), sink_b=True), False,
     ("nt", False), ("nt", "dw_stacked", False)),
    ("blocks_of_6", dict(M=256, I=64, widths=(6, 6, 6, 6)), False, ("nt", False), ("nt", "dw_stacked", False)),
    ("head_1000", dict(M=128, I=384, widths=(1000,)), False, ("nt", False), ("nt", "dw", False)),
    ("head_10", dict(M=24, I=64, widths=(10,)), False, ("lib", True), ("dw_t", "lib", False)),
    ("head_10_m4097", dict(M=4097, I=64, widths=(10,)), False, ("lib", False), ("lib", "lib", False)),
    ("head_10_m4104", dict(M=4104, I=64, widths=(10,)), False, ("lib", False), ("lib", "lib", False)),   # M % 8 == 0
    ("head_10_m4096", dict(M=4096, I=64, widths=(10,)), False, ("lib", True), ("dw_t", "lib", False)),
    ("head_10_m20", dict(M=20, I=64, widths=(10,)), False, ("lib", False), ("lib", "lib", False)),
    ("head_10_lib", dict(M=24, I=64, widths=(10,)), True, ("lib", True), ("dw_t", "lib", False)),
    ("in_12", dict(M=64, I=12, widths=(64,)), False, *ALL_LIB),
    ("f32", dict(M=64, I=64, widths=(64,), dtype=F32), False, ("f32", False), ("f32", "f32", False)),
    ("f32_blocks_sinks", dict(M=64, I=64, widths=(64, 32), dtype=F32, sinks_w=(True, True), sink_b=True), False,
     ("f32", False), ("f32", "f32", False)),
    ("f32_in_6", dict(M=64, I=6, widths=(64,), dtype=F32), False, *ALL_LIB),
    ("cpu", dict(M=256, I=64, widths=(128,), on_gpu=False), False, *ALL_LIB),
    ("cpu_f32", dict(M=64, I=64, widths=(64,), dtype=F32, on_gpu=False), False, *ALL_LIB),
    ("lib_m4096", dict(M=4096, I=64, widths=(64,)), True, ("nt", False), ("lib", "dw", False)),
    ("lib_m4097", dict(M=4097, I=64, widths=(64,)), True, ("lib", False), ("lib", "dw", False)),
    # the offload flag on the sunk single kernel: bias x bias sink
    ("sunk_bias_sink", dict(M=256, I=64, widths=(128,), sinks_w=(True,), sink_b=True), False,
     ("nt", False), ("nt", "dw_sunk", True)),
    ("sunk_bias_no_sink", dict(M=256, I=64, widths=(128,), sinks_w=(True,)), False,
     ("nt", False), ("nt", "dw_sunk", False)),
    ("sunk_no_bias", dict(M=256, I=64, widths=(128,), has_bias=False, sinks_w=(True,)), False,
     ("nt", False), ("nt", "dw_sunk", True)),
    ("blocks_sunk_bias_no_sink", dict(M=256, I=64, widths=(64, 64), sinks_w=(True, True)), False,
     ("nt", False), ("nt", "dw_blocks_sunk", False)),
    ("blocks_sunk_no_bias", dict(M=256, I=64, widths=(64, 64), has_bias=False, sinks_w=(True, True)), False,
     ("nt", False), ("nt", "dw_blocks_sunk", True)),
    ("unsunk_bias_sink", dict(M=256, I=64, widths=(128,), sink_b=True), False, ("nt", False), ("nt", "dw", False)),
    ("unsunk_no_bias", dict(M=256, I=64, widths=(128,), has_bias=False), False, ("nt", False), ("nt", "dw", False)),
]


def facts(kw, gemm_lib=False):
    return ops.dense_facts_of_shapes(**kw)._replace(gemm_lib=gemm_lib)
