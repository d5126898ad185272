"""One pinned call per row of gemm.hip's instance tables that ``sae_gemm_nt`` / ``sae_gemm_nt_gelu_dropout``
can launch (SAE_G8_TABLE, SAE_G8X_TABLE and the row-operand rows of SAE_NT128_TABLE), shared by the
CPU routing test (the name, through ``sae_gemm_nt_instance``) and the GPU test (the name, then the call).

Every expectation is read off the rules of ``nt_plan`` at 256 compute units (the MI355X, and what the
plan assumes without a device), not off the query's output:
  * gemm8x: K >= 768, K % 64 == 0, M >= 4096, N % 256 == 0 and (N == 768 or N % 192 != 0), never GELU';
  * gemm8: N % 192 == 0, K % 64 == 0, K >= 384, M >= 4096; GELU' only at K == 384 or as the multiply;
  * tile height (both): 224 unless 256-row tiles take fewer rows per CU -- 4100 rows are 19 tiles of 224
    or 17 of 256, so 14 tile columns (N = 2688 at 192, 3584 at 256) make 266 tiles = two rounds = 448
    rows against 238 = one round = 256, and a few columns make one round either way = 224;
  * 256 x 128 tiles (GELU family, K < 768, N % 128 == 0): when rounds x 256 x 128 < rounds x BM x 192 --
    N = 384: 17 x 3 = 51 tiles, 32 K outputs against 19 x 2 of 224 x 192 = 43 K; N = 2688: two rounds of
    32 K against one of 256 x 192 = 49 K, so the 192-wide tiles stay;
  * 128-row kernel: K % 64 != 0 the K tail; else GELU family at K >= 768 with >= 512 tiles of 256 x 128
    (M 4000: 16 x 32) the tall tile; else GELU family at K <= 384 the 32-deep stages; else 64-deep."""
from sae_vision_amd import _lib as L

NONE, GELU, DGELU, GELU_GRAD, MUL_AUX = range(5)   # SAE_EPI_*

# (M, K, N, epilogue, dropout, row name)
NT_ROWS = [
    (4096, 384, 192, NONE, 0, "g8_192_bm224_plain"),
    (4096, 384, 2688, NONE, 0, "g8_192_bm256_plain"),
    (4100, 384, 192, GELU, 0, "g8_192_bm224_gelu"),
    (4100, 384, 2688, GELU_GRAD, 0, "g8_192_bm256_gelu"),
    (4100, 384, 192, DGELU, 0, "g8_192_bm224_dgelu"),
    (4100, 768, 2688, MUL_AUX, 0, "g8_192_bm256_dgelu"),       # beyond K 384 only the multiply stays on gemm8
    (4100, 384, 192, GELU_GRAD, 1, "g8_192_bm224_gelu_drop"),
    (4100, 384, 2688, GELU_GRAD, 1, "g8_192_bm256_gelu_drop"),
    (25216, 384, 1536, GELU, 0, "g8_128_wgm4_gelu"),           # DeiT-S FF Dense_0
    (4100, 384, 384, MUL_AUX, 0, "g8_128_wgm4_dgelu"),
    (4100, 384, 384, GELU_GRAD, 1, "g8_128_wgm4_gelu_drop"),
    (4100, 768, 768, NONE, 0, "g8x_bm224_plain"),
    (4100, 768, 3584, NONE, 0, "g8x_bm256_plain"),
    (4100, 768, 768, GELU, 0, "g8x_bm224_gelu"),
    (4100, 768, 3584, GELU_GRAD, 0, "g8x_bm256_gelu"),
    (4100, 768, 768, GELU_GRAD, 1, "g8x_bm224_gelu_drop"),
    (4100, 768, 3584, GELU_GRAD, 1, "g8x_bm256_gelu_drop"),
    (130, 128, 136, NONE, 0, "nt128_k64_plain"),
    (130, 448, 136, GELU, 0, "nt128_k64_gelu"),
    (130, 448, 136, DGELU, 0, "nt128_k64_dgelu"),
    (130, 448, 136, GELU_GRAD, 1, "nt128_k64_gelu_drop"),
    (128, 128, 136, GELU, 0, "nt128_k32_gelu"),
    (130, 128, 136, MUL_AUX, 0, "nt128_k32_dgelu"),
    (130, 128, 136, GELU_GRAD, 1, "nt128_k32_gelu_drop"),
    (4000, 768, 4096, GELU, 0, "nt128_tall_gelu"),             # M < 4096 keeps it off gemm8x
    (4000, 768, 4096, DGELU, 0, "nt128_tall_dgelu"),
    (4000, 768, 4096, GELU_GRAD, 1, "nt128_tall_gelu_drop"),
    (128, 40, 64, NONE, 0, "nt128_ktail_plain"),
    (130, 40, 72, GELU_GRAD, 0, "nt128_ktail_gelu"),
    (130, 40, 72, DGELU, 0, "nt128_ktail_dgelu"),
    (130, 40, 72, GELU_GRAD, 1, "nt128_ktail_gelu_drop"),
]

# the image loaders of sae_patch_embed_fwd: chosen by layout and dtype (tests/test_gpu_patch.py), no shape reaches them
PATCH_ROWS = {"patch_nhwc_bf16", "patch_nhwc_f32", "patch_hwcn_bf16", "patch_hwcn_f32"}

# the four-value route of a row's table
ROUTE_OF_PREFIX = {"g8_": L.SAE_NT_ROUTE_GEMM8, "g8x_": L.SAE_NT_ROUTE_GEMM8X, "nt128_ktail_": L.SAE_NT_ROUTE_TILE128_KTAIL,
                   "nt128_": L.SAE_NT_ROUTE_TILE128}


def route_of(name):
    return next(r for p, r in ROUTE_OF_PREFIX.items() if name.startswith(p))


def instance(lib, M, K, N, epilogue, dropout=0):
    s = lib.sae_gemm_nt_instance(M, N, K, epilogue, dropout)
    return None if s is None else s.decode()
