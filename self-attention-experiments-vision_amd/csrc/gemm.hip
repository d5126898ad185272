// gemm.hip -- the projection entry points of the C ABI: weight gradients (gemm_dw8.h), fp32
// GEMMs (gemm_f32.h), the forward / input-gradient GEMMs (gemm_nt.h, gemm8.h) with their routing
// rule, the patch embedding (patch.h) and the weight casts.
#include <type_traits>

#include "gemm_nt.h"
#include "gemm8.h"
#include "gemm_dw.h"
#include "gemm_dw8.h"
#include "gemm_f32.h"
#include "patch.h"
#include "host.h"

using namespace sae;

namespace {

// ------------------------------------------------------------------ projection gradients
void dw_plan(int M, int I, int J, int* S, int* chunk, int slots = 512) {
  // at most `slots` workgroups = one resident round (512: 2 per CU x 256 CUs; 256 for the 8-wave
  // two-group kernel): a 513th would run alone in a second round (the old ceil() rule launched
  // 513 / 540 / 513 for the DeiT-S QKV / FF / output projections).  A smaller slot count gives
  // fewer splits, so the 512-slot plan's workspace bounds every plan's.
  const int tiles = ((I + kDwT - 1) / kDwT) * ((J + kDwT - 1) / kDwT);
  int s = slots / tiles;
  s = std::max(1, std::min(s, (M + 255) / 256));
  int c = (M + s - 1) / s;
  c = (c + kDwK - 1) / kDwK * kDwK;
  *chunk = c;
  *S = (M + c - 1) / c;
}

size_t dw_part_bytes(int S, int I, int J) { return ((size_t)S * I * J * 4 + 255) & ~(size_t)255; }

long long dw_grid(const DwArgs& a) {
  return (long long)a.S * ((a.I + kDwT - 1) / kDwT) * ((a.J + kDwT - 1) / kDwT);
}

// one gemm_dw8 launch (gemm_dw8.h; with or without the bias column sums), NG wave groups per workgroup
template <int NG> int dw8_launch(const DwArgs& a, hipStream_t st) {
  return launch("gemm_dw", a.db ? gemm_dw8_kernel<true, NG> : gemm_dw8_kernel<false, NG>, dw_grid(a), dim3(256 * NG),
                dw8_lds_bytes<NG>(), st, a);
}

// sum of the S split partials into dw (and db)
int dw_reduce(const char* name, const DwArgs& a, hipStream_t st) {
  const long long n4 = (long long)a.I * a.J / 4;
  const unsigned rb = (unsigned)std::min<long long>((n4 + kDwRedCols - 1) / kDwRedCols, 4096);
  return launch(name, gemm_dw_reduce_kernel, dim3(rb, a.db ? 2 : 1), dim3(256), 0, st, a);
}

int gemm_dw_impl(void* stream, int32_t M, int32_t I, int32_t J, const void* x, int64_t ldx, const void* dy,
                 int64_t ldy, float* dw, int64_t ldw, float* db, int32_t accumulate, void* workspace,
                 int32_t jblock) {
  if (M < 1 || I < 1 || J < 1) return fail(SAE_EINVAL, "gemm_dw: M/I/J must be >= 1 (got %d/%d/%d)", M, I, J);
  if (I % 8 || J % 8) return fail(SAE_EUNSUPPORTED, "gemm_dw: I (%d) and J (%d) must be multiples of 8", I, J);
  if (ldx < I || ldy < J || ldw < J || ldx % 8 || ldy % 8 || ldw % 4)
    return fail(SAE_EINVAL, "gemm_dw: bad leading dimensions ldx %lld ldy %lld ldw %lld", (long long)ldx,
                (long long)ldy, (long long)ldw);
  if (!x || !dy || !dw || !workspace) return fail(SAE_EINVAL, "gemm_dw: x/dy/dw/workspace must be non-NULL");
  if (!aligned16(x) || !aligned16(dy) || !aligned16(dw) || !aligned16(workspace))
    return fail(SAE_EINVAL, "gemm_dw: x, dy, dw and workspace must be 16-byte aligned");
  DwArgs a;
  memset(&a, 0, sizeof a);
  a.x = reinterpret_cast<const __bf16*>(x);
  a.dy = reinterpret_cast<const __bf16*>(dy);
  a.M = M;
  a.I = I;
  a.J = J;
  // wave groups per workgroup (gemm_dw8.h): two for small outputs (<= 64 tiles of 128 x 128: every
  // DeiT-S / CaiT projection), where half the splits still fill the chip and halve the fp32
  // partial traffic (output projection dW + reduce 34.8 -> 30.6 us); one for the larger ViT-B
  // outputs, where halving the splits would leave CUs idle (FF 139 -> 205 us)
  const int tiles = ((I + kDwT - 1) / kDwT) * ((J + kDwT - 1) / kDwT);
  const int NG = tiles <= 64 ? 2 : 1;
  dw_plan(M, I, J, &a.S, &a.chunk, 512 / NG);
  if ((long long)(a.chunk + 4 * NG * kDwK) * std::max(ldx, ldy) * 2 >= (1LL << 31))
    return fail(SAE_EUNSUPPORTED, "gemm_dw: token chunk exceeds 32-bit buffer addressing");
  a.part = reinterpret_cast<float*>(workspace);
  a.bpart = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + dw_part_bytes(a.S, I, J));
  a.dw = dw;
  a.db = db;
  a.ldx = ldx;
  a.ldy = ldy;
  a.ldw = ldw;
  a.accumulate = accumulate;
  a.jblock = jblock;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = NG == 2 ? dw8_launch<2>(a, st) : dw8_launch<1>(a, st)) return rc;
  return dw_reduce("gemm_dw_reduce", a, st);
}

// ------------------------------------------------------------------ fp32 projections
// split-K plan: more splits only while the output tiles leave the chip idle and each split keeps
// >= 1,024 of depth (the weight gradients: K = the token count); independent of `colsum` so the
// workspace bound holds for both
void f32_plan(int M, int N, int K, int* S, int* kchunk) {
  const int tiles = ((M + kF32T - 1) / kF32T) * ((N + kF32T - 1) / kF32T);
  int s = 1;
  if (tiles < 256 && K >= 2048) s = std::min((512 + tiles - 1) / tiles, K / 1024);
  s = std::max(1, std::min(s, 64));
  int c = (K + s - 1) / s;
  c = (c + kF32K - 1) / kF32K * kF32K;
  *kchunk = c;
  *S = (K + c - 1) / c;
}

// ------------------------------------------------------------ forward / input-gradient GEMMs
// one launch of the 128-row kernel: TM x 128 tiles, two LDS stage buffers of BK-deep A and B
// images; TM and BK are the operand loader's
template <int EPI, class AL> int nt_run(const char* name, hipStream_t st, const NtArgs& g) {
  const size_t lds = 2 * (NtRows<AL>::value + kNtT) * NtDepth<AL>::value * 2;
  const long long grid = (long long)((g.M + NtRows<AL>::value - 1) / NtRows<AL>::value) * ((g.N + kNtT - 1) / kNtT);
  return launch(name, gemm_nt_kernel<EPI, AL>, grid, dim3(256), lds, st, g);
}

// one persistent gemm8 launch (BM x BN tiles, one 8-wave workgroup per CU)
template <int EPI, int BN, int BK, int NS, int BM, int WGM, bool XW>
int g8_run(const char* name, hipStream_t st, const NtArgs& g, int cus) {
  const long long tiles = (long long)((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
  return launch(name, gemm8_nt_kernel<EPI, BN, BK, NS, BM, WGM, XW>, std::min<long long>(tiles, cus), dim3(512),
                g8_lds_bytes<BN, BK, NS, WGM>(), st, g);
}

// one gemm8x launch (BM x BN tiles, ping-pong wave groups, one tile per workgroup)
template <int EPI, int BN, int BM> int g8x_run(const char* name, hipStream_t st, const NtArgs& g) {
  const long long tiles = (long long)((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
  return launch(name, gemm8x_nt_kernel<EPI, BN, true, BM>, tiles, dim3(512), g8x_lds_bytes<BN, BM>(), st, g);
}

// ------------------------------------------------------------------------ instance tables
// Every instance of gemm8_nt_kernel, gemm8x_nt_kernel and gemm_nt_kernel is ONE row: the template
// parameters written once, under their names; the plan and the patch embedding name a row, never
// a tuple.  Epilogue suffixes: _plain (kEpiNone), _gelu (SAE_EPI_GELU and _GELU_GRAD), _dgelu
// (SAE_EPI_DGELU and _MUL_AUX), _gelu_drop (sae_gemm_nt_gelu_dropout).
//
// gemm8: 224 / 256 x 192 tiles on 2 x 4 waves, and 256 x 128 tiles on 4 x 2 waves (nt_plan).
// XW, plain 192-wide tiles: whole-row epilogue stores through the shared row image: QKV forward
// 32.9 -> 31.4 us, DeiT-S step -0.13 % (profiles/r06xw_g8_xw_ab.txt)
//  row name                 EPI           BN   BK  NS BM   WGM XW
#define SAE_G8_TABLE(X)                                                \
  X(g8_192_bm224_plain,      kEpiNone,     192, 64, 2, 224, 2,  true)  \
  X(g8_192_bm256_plain,      kEpiNone,     192, 64, 2, 256, 2,  true)  \
  X(g8_192_bm224_gelu,       kEpiGelu,     192, 64, 2, 224, 2,  false) \
  X(g8_192_bm256_gelu,       kEpiGelu,     192, 64, 2, 256, 2,  false) \
  X(g8_192_bm224_dgelu,      kEpiDGelu,    192, 64, 2, 224, 2,  false) \
  X(g8_192_bm256_dgelu,      kEpiDGelu,    192, 64, 2, 256, 2,  false) \
  X(g8_192_bm224_gelu_drop,  kEpiGeluDrop, 192, 64, 2, 224, 2,  false) \
  X(g8_192_bm256_gelu_drop,  kEpiGeluDrop, 192, 64, 2, 256, 2,  false) \
  X(g8_128_wgm4_gelu,        kEpiGelu,     128, 64, 2, 256, 4,  false) \
  X(g8_128_wgm4_dgelu,       kEpiDGelu,    128, 64, 2, 256, 4,  false) \
  X(g8_128_wgm4_gelu_drop,   kEpiGeluDrop, 128, 64, 2, 256, 4,  false)

// gemm8x: 224 / 256 x 256 tiles; no GELU' epilogue (g8x_route)
//  row name                 EPI           BN   BM
#define SAE_G8X_TABLE(X)                             \
  X(g8x_bm224_plain,         kEpiNone,     256, 224) \
  X(g8x_bm256_plain,         kEpiNone,     256, 256) \
  X(g8x_bm224_gelu,          kEpiGelu,     256, 224) \
  X(g8x_bm256_gelu,          kEpiGelu,     256, 256) \
  X(g8x_bm224_gelu_drop,     kEpiGeluDrop, 256, 224) \
  X(g8x_bm256_gelu_drop,     kEpiGeluDrop, 256, 256)

// The 128-row kernel by operand loader AL = NtRowAT<stage depth, tile rows, K tail>: _k64 the
// 64-deep stages, _k32 the shallow ones, _tall the 256-token tile (both for the GELU-family
// epilogues only, nt_plan), _ktail K % 64 != 0; and the four image loaders of sae_patch_embed_fwd
// (patch.h: NtPatchA<HWCN, F32>), chosen by layout and dtype.
//  row name                 EPI           AL
#define SAE_NT128_TABLE(X)                                        \
  X(nt128_k64_plain,         kEpiNone,     NtRowAT<64>)           \
  X(nt128_k64_gelu,          kEpiGelu,     NtRowAT<64>)           \
  X(nt128_k64_dgelu,         kEpiDGelu,    NtRowAT<64>)           \
  X(nt128_k64_gelu_drop,     kEpiGeluDrop, NtRowAT<64>)           \
  X(nt128_k32_gelu,          kEpiGelu,     NtRowAT<32>)           \
  X(nt128_k32_dgelu,         kEpiDGelu,    NtRowAT<32>)           \
  X(nt128_k32_gelu_drop,     kEpiGeluDrop, NtRowAT<32>)           \
  X(nt128_tall_gelu,         kEpiGelu,     NtRowAT<32, 256>)      \
  X(nt128_tall_dgelu,        kEpiDGelu,    NtRowAT<32, 256>)      \
  X(nt128_tall_gelu_drop,    kEpiGeluDrop, NtRowAT<32, 256>)      \
  X(nt128_ktail_plain,       kEpiNone,     NtRowAT<64, 128, true>) \
  X(nt128_ktail_gelu,        kEpiGelu,     NtRowAT<64, 128, true>) \
  X(nt128_ktail_dgelu,       kEpiDGelu,    NtRowAT<64, 128, true>) \
  X(nt128_ktail_gelu_drop,   kEpiGeluDrop, NtRowAT<64, 128, true>) \
  X(patch_nhwc_bf16,         kEpiNone,     NtPatchA<false, false>) \
  X(patch_nhwc_f32,          kEpiNone,     NtPatchA<false, true>)  \
  X(patch_hwcn_bf16,         kEpiNone,     NtPatchA<true, false>)  \
  X(patch_hwcn_f32,          kEpiNone,     NtPatchA<true, true>)

#define SAE_ROW(name, ...) name,
enum class Inst { SAE_G8_TABLE(SAE_ROW) SAE_G8X_TABLE(SAE_ROW) SAE_NT128_TABLE(SAE_ROW) count };
#undef SAE_ROW

const char* inst_name(Inst i) {
  switch (i) {
#define SAE_ROW(name, ...) \
  case Inst::name: return #name;
    SAE_G8_TABLE(SAE_ROW) SAE_G8X_TABLE(SAE_ROW) SAE_NT128_TABLE(SAE_ROW)
#undef SAE_ROW
    case Inst::count: break;
  }
  return nullptr;
}

// the launch of a row; `cus` bounds the persistent gemm8 grid (the other kernels: one tile per workgroup)
int run_inst(Inst i, hipStream_t st, const NtArgs& g, int cus = 0) {
  switch (i) {
#define SAE_G8(name, ...) \
  case Inst::name: return g8_run<__VA_ARGS__>(#name, st, g, cus);
#define SAE_G8X(name, ...) \
  case Inst::name: return g8x_run<__VA_ARGS__>(#name, st, g);
#define SAE_NT(name, ...) \
  case Inst::name: return nt_run<__VA_ARGS__>(#name, st, g);
    SAE_G8_TABLE(SAE_G8) SAE_G8X_TABLE(SAE_G8X) SAE_NT128_TABLE(SAE_NT)
#undef SAE_G8
#undef SAE_G8X
#undef SAE_NT
    case Inst::count: break;
  }
  return fail(SAE_EINVAL, "gemm_nt: bad instance %d", (int)i);
}

// SAE_NT_ROUTE_* of a row: its table, and for the 128-row kernel whether the loader takes a K tail
int inst_route(Inst i) {
  switch (i) {
#define SAE_G8(name, ...) \
  case Inst::name: return SAE_NT_ROUTE_GEMM8;
#define SAE_G8X(name, ...) \
  case Inst::name: return SAE_NT_ROUTE_GEMM8X;
#define SAE_NT(name, EPI, ...) \
  case Inst::name: return NtKT<__VA_ARGS__>::value ? SAE_NT_ROUTE_TILE128_KTAIL : SAE_NT_ROUTE_TILE128;
    SAE_G8_TABLE(SAE_G8) SAE_G8X_TABLE(SAE_G8X) SAE_NT128_TABLE(SAE_NT)
#undef SAE_G8
#undef SAE_G8X
#undef SAE_NT
    case Inst::count: break;
  }
  return SAE_NT_ROUTE_NONE;
}

// NtArgs.nts of a gemm8 row (0 for the other kernels, which do not read it):
// epilogue stores non-temporal except for the gelu' multiply on 2 x 4 waves (whose 96-byte row segments then
// left L2 unmerged: 77 -> 102 MB written); DeiT-S step 8.02 -> 7.96 ms with every epilogue
// non-temporal, the plain / GELU launches faster and the multiply slower (profiles/r06z_g8_nts_ab.txt).
// The multiply's aux (gelu'(h)) tile loaded non-temporal: level in isolation, DeiT-S step
// 8.01 -> 7.85 ms (profiles/r06z4_g8_aux_nt_ab.txt)
int g8_nts(Inst i) {
  switch (i) {
#define SAE_G8(name, EPI, BN, BK, NS, BM, WGM, XW)                                        \
  case Inst::name:                                                                        \
    return ((EPI != kEpiDGelu || WGM == 4) && !dev_knob("SAE_G8_NO_NTS") ? 1 : 0) |        \
           (!dev_knob("SAE_G8_NO_AUX_NT") ? 2 : 0);
    SAE_G8_TABLE(SAE_G8)
#undef SAE_G8
    default: return 0;
  }
}

// ------------------------------------------------------------------------------- the plan
// What nt_plan decides on: the call's shape and epilogue, the device's CU count and the value of
// every dev knob of the dispatch (0 in the release library).  nt_facts reads the device and the
// environment; the plan itself touches neither, so a shape plans the same with and without a device
// of the same size (no device: 256 CUs).
struct NtFacts {
  int M, N, K;
  int epilogue;   // SAE_EPI_* as passed
  bool drop;      // sae_gemm_nt_gelu_dropout: the hidden dropout rides on SAE_EPI_GELU_GRAD
  int cus;
  int no_g8, bm256, variant, no_bn128, mul192, no_mul;   // SAE_NT_NO_G8, SAE_NT_BM256, SAE_NT_VARIANT,
                                                         // SAE_G8_NO_BN128, SAE_G8_MUL192, SAE_G8_NO_MUL
};

NtFacts nt_facts(int M, int N, int K, int epilogue, bool drop) {
  return NtFacts{M, N, K, epilogue, drop, device_cus(), dev_knob("SAE_NT_NO_G8"), dev_knob("SAE_NT_BM256"),
                 dev_knob("SAE_NT_VARIANT"), dev_knob("SAE_G8_NO_BN128"), dev_knob("SAE_G8_MUL192"),
                 dev_knob("SAE_G8_NO_MUL")};
}

// tile height of a gemm8 / gemm8x launch: 224 where 256-row tiles quantize worse onto the CUs --
// cost = rounds of tiles over the CUs x rows per tile (M = 25,216 into 384 features: 198 tiles of
// 256 rows, one round on 256 CUs with 58 idle, vs 226 of 224 rows; M = 18,464 into 768: 219 vs 249)
int g8_pick_bm(const NtFacts& f, int BN) {
  if (f.bm256) return 256;
  const long long G = f.cus, tn = (f.N + BN - 1) / BN;
  auto cost = [&](int bm) { return ((((long long)f.M + bm - 1) / bm * tn + G - 1) / G) * bm; };
  return cost(224) < cost(256) ? 224 : 256;
}

// GELU forward at K < 768 (the epilogue's VALU work, which scales with the outputs, outweighs the
// reduction): 256 x 128 tiles when they put fewer outputs on the busiest CU than 224 / 256 x 192 --
// DeiT-S / CaiT-S FF Dense_0 (M 25,216 / 25,088 into 1,536): 5 rounds of 32 K outputs against 4 of
// 43 K, 68.0 -> 63.8 us same box (profiles/r05ai_g8_bn128_ab.txt; the GELU' input gradient measured
// level, so it keeps the 192-wide tiles)
bool g8_gelu_bn128(const NtFacts& f) {
  const int M = f.M, N = f.N;
  if (f.K >= 768 || N % 128 || f.no_bn128) return false;
  const long long G = f.cus;
  const int bm = g8_pick_bm(f, 192);
  const long long c192 = (((long long)(M + bm - 1) / bm * ((N + 191) / 192) + G - 1) / G) * bm * 192;
  const long long c128 = (((long long)(M + 255) / 256 * (N / 128) + G - 1) / G) * 256 * 128;
  return c128 < c192;
}

// Kernel choice for sae_gemm_nt (round 5: a rule on tile fill and reduction depth instead of the
// BASELINE shape whitelist; every width in create_model.py:6-215 routes to one of these):
//   gemm8x  (ping-pong 256 x 256 tiles): reductions K >= 768 into outputs that fill 256-wide tiles
//           but not 192-wide ones (N % 256 == 0 and N % 192 != 0: ViT-L 1024 / 4096, CvT-W24 1024),
//           plus the 768-feature outputs (ViT-B / CaiT-M output projection, QKV / Dense_0 input
//           gradients, Dense_1 forward; 0.90-0.98 of the library, profiles/r04i_g8probe.txt);
//   gemm8   (persistent 224/256 x 192 tiles): outputs that fill 192-wide tiles (N % 192 == 0) at
//           K >= 384 -- every DeiT-S / CaiT-S projection, the ViT-B wide K = 768 forwards;
//   128-row sae_gemm_nt: the rest -- small M (classifier heads, CLS rows), K < 384 (DeiT-Ti, the
//           C = 192 widths), K not a multiple of 64 (KT instances: CaiT-XXS / XS 288, CvT 368, TNT
//           inner 24 / 40 and their FF widths), the GELU' epilogue beyond K = 384 (its 256-token
//           tile), N not a multiple of 192 or 256.
// Both persistent kernels need M >= 4096 (enough tiles to fill the CUs) and K % 64 == 0.
bool g8x_route(const NtFacts& f, int epilogue) {
  const int M = f.M, N = f.N, K = f.K;
  if (epilogue == SAE_EPI_DGELU || K < 768 || K % 64 || M < 4096 || N % 256) return false;
  return N == 768 || N % 192 != 0;
}

// gemm8 (gemm8.h) or the 128-row sae_gemm_nt: tools/probe/gemm8_probe.py, profiles/r04c_g8probe.txt --
// gemm8 wins on the 384-feature outputs at every depth (DeiT-S / CaiT output projection, QKV and
// FF Dense_0 input gradients, Dense_1 forward: 412-692 -> 497-849 TF/s) and on the wide K = 768
// ViT-B forwards (QKV 2304 features 750 -> 850-900, FF Dense_0 + GELU 673-700 -> 715-729: level with
// the library's 830-960); the 128-row kernel stays on the DeiT-S wide K = 384 outputs (a tie) and
// the GELU' epilogue (gemm8 has none)
// Round 4 (224-row tiles, g8_pick_bm): also the DeiT-S / CaiT wide K = 384 outputs -- QKV forward
// 593 -> 647 TF/s, FF Dense_0 + GELU 546 -> 563, Dense_1 input gradient with GELU' 497 -> 509
// (profiles/r04k_g8probe.txt, v53 vs rel)
// Round 5: with the saved-gelu' multiply epilogue (SAE_EPI_MUL_AUX, `gp`) the GELU' epilogue no
// longer bounds the deeper ViT-B input gradient either, so gemm8 takes it at every K.
bool g8_route(const NtFacts& f, int epilogue, bool gp) {
  const int M = f.M, N = f.N, K = f.K;
  if (N % 192 || K % 64 || K < 384 || M < 4096) return false;
  return epilogue != SAE_EPI_DGELU || K == 384 || (gp && !f.no_mul);
}

// The one routing decision: sae_gemm_nt_route and sae_gemm_nt_instance report it, sae_gemm_nt,
// sae_gemm_nt_gelu_dropout launch it.  Pure: no HIP call, no pointer, no environment.  Refuses
// what no row takes.
int nt_plan(const NtFacts& f, Inst* row) {
  using I = Inst;
  const int M = f.M, N = f.N, K = f.K;
  if (M < 1 || N < 1 || K < 1) return fail(SAE_EINVAL, "gemm_nt: M/N/K must be >= 1 (got %d/%d/%d)", M, N, K);
  if (K % 8 || N % 8) return fail(SAE_EUNSUPPORTED, "gemm_nt: K (%d) and N (%d) must be multiples of 8", K, N);
  if (f.epilogue < SAE_EPI_NONE || f.epilogue > SAE_EPI_MUL_AUX)
    return fail(SAE_EINVAL, "gemm_nt: unknown epilogue %d", f.epilogue);
  if (f.drop && f.epilogue != SAE_EPI_GELU_GRAD)
    return fail(SAE_EINVAL, "gemm_nt: dropout rides on the SAE_EPI_GELU_GRAD epilogue only (got %d)", f.epilogue);
  // the gelu' forms run on the GELU / GELU' kernels with the saved operand gelu'(h) (NtArgs.gp)
  const bool gp = f.epilogue >= SAE_EPI_GELU_GRAD;
  const int epi = gp ? f.epilogue - 2 : f.epilogue;   // SAE_EPI_NONE / GELU / DGELU
  const int e = f.drop ? kEpiGeluDrop : epi;          // the rows' EPI column: plain, gelu, dgelu, gelu_drop
  if (!f.no_g8 && g8x_route(f, epi)) {
    static const I rows[2][4] = {
        {I::g8x_bm224_plain, I::g8x_bm224_gelu, I::count, I::g8x_bm224_gelu_drop},
        {I::g8x_bm256_plain, I::g8x_bm256_gelu, I::count, I::g8x_bm256_gelu_drop}};
    *row = rows[g8_pick_bm(f, 256) == 256][e];
  } else if (!f.no_g8 && g8_route(f, epi, gp)) {
    // GELU on 4 x 2 waves (64 x 64 wave tiles): whole 128-byte output lines per wave row segment --
    // writes 172 -> 155 MB (= algorithmic), 57.1 -> 54.8 us at DeiT-S (profiles/r06w4_g8_wgm4_ab.txt);
    // the gelu' multiply on the same 256 x 128 tiles and 4 x 2 waves (whole-line stores, now also
    // non-temporal): 59.5 -> 53.8 us at DeiT-S, reads 128 -> 111 MB (profiles/r06m128_g8_mul_ab.txt)
    static const I bn128[4] = {I::count, I::g8_128_wgm4_gelu, I::g8_128_wgm4_dgelu, I::g8_128_wgm4_gelu_drop};
    static const I bn192[2][4] = {
        {I::g8_192_bm224_plain, I::g8_192_bm224_gelu, I::g8_192_bm224_dgelu, I::g8_192_bm224_gelu_drop},
        {I::g8_192_bm256_plain, I::g8_192_bm256_gelu, I::g8_192_bm256_dgelu, I::g8_192_bm256_gelu_drop}};
    const bool may128 = epi == SAE_EPI_GELU || (epi == SAE_EPI_DGELU && !f.mul192);
    *row = may128 && g8_gelu_bn128(f) ? bn128[e] : bn192[g8_pick_bm(f, 192) == 256][e];
  } else {
    // [loader][EPI]: the shallow and the tall tiles have no plain row
    static const I rows[4][4] = {
        {I::nt128_k64_plain, I::nt128_k64_gelu, I::nt128_k64_dgelu, I::nt128_k64_gelu_drop},
        {I::count, I::nt128_k32_gelu, I::nt128_k32_dgelu, I::nt128_k32_gelu_drop},
        {I::count, I::nt128_tall_gelu, I::nt128_tall_dgelu, I::nt128_tall_gelu_drop},
        {I::nt128_ktail_plain, I::nt128_ktail_gelu, I::nt128_ktail_dgelu, I::nt128_ktail_gelu_drop}};
    // tile height: 256 tokens for the GELU / GELU' epilogue GEMMs at K >= 768 (the ViT-B FF block:
    // the epilogue's VALU work per output is amortised over twice the MFMA work per tile;
    // tools/nt_probe.py at M 36928 K 768 N 3072: GELU 512 -> 634, GELU' 548 -> 609 TF/s) when that
    // still gives >= 2 tiles per CU; 128 otherwise (plain GEMMs: no gain, profiles/r03n_nt_probe.txt)
    const bool fused = epi != SAE_EPI_NONE;
    bool tall = fused && K >= 768 && (long long)((M + 255) / 256) * ((N + kNtT - 1) / kNtT) >= 512;
    if (f.variant) tall = fused && f.variant == 2;
    // stage depth: the GELU / GELU' epilogue GEMMs at reduction depth <= 384 (DeiT-S / CaiT FF
    // block) run 32-deep stages (32 KiB of LDS: 3-4 workgroups per CU, so one tile's epilogue VALU
    // overlaps other tiles' MFMAs; same-box step A/B 9.19 -> 9.10 ms); deeper reductions (ViT-B,
    // K 768) and the plain GEMM keep 64-deep stages (2 workgroups per CU), which are faster there
    const bool shallow = fused && K <= 384;
    // K-tail instances (K % 8 == 0): 64-deep stages, the last one partial
    *row = rows[K % kNtK ? 3 : tall ? 2 : shallow ? 1 : 0][e];
  }
  return SAE_OK;
}

// ------------------------------------------------------------------------ patch embedding
int patch_geom(const sae_patch_desc* d, PatchGeom* g, int* M, int* K) {
  if (!d) return fail(SAE_EINVAL, "patch_embed: NULL descriptor");
  if (d->batch < 1 || d->height < 1 || d->width < 1 || d->channels < 1 || d->patch_h < 1 || d->patch_w < 1 ||
      d->embed < 1)
    return fail(SAE_EINVAL, "patch_embed: sizes must be >= 1");
  if (d->layout != SAE_LAYOUT_NHWC && d->layout != SAE_LAYOUT_HWCN)
    return fail(SAE_EINVAL, "patch_embed: unknown layout %d", d->layout);
  if (d->dtype != SAE_DTYPE_BF16 && d->dtype != SAE_DTYPE_F32)
    return fail(SAE_EINVAL, "patch_embed: unknown image dtype %d", d->dtype);
  if (d->height % d->patch_h || d->width % d->patch_w)
    return fail(SAE_EINVAL, "patch_embed: image %dx%d is not a whole number of %dx%d patches", d->height, d->width,
                d->patch_h, d->patch_w);
  const long long k = (long long)d->patch_h * d->patch_w * d->channels;
  const long long elems = (long long)d->batch * d->height * d->width * d->channels;
  const long long L = (long long)(d->height / d->patch_h) * (d->width / d->patch_w);
  if (k % kNtK || (d->patch_w * d->channels) % 8 || d->embed % 8)
    return fail(SAE_EUNSUPPORTED, "patch_embed: needs ph*pw*C %% 64 == 0, pw*C %% 8 == 0, embed %% 8 == 0 "
                "(got K %lld, pw*C %d, embed %d)", k, d->patch_w * d->channels, d->embed);
  if (d->layout == SAE_LAYOUT_HWCN && d->batch % 8)
    return fail(SAE_EUNSUPPORTED, "patch_embed: the HWCN layout needs batch %% 8 == 0 (got %d)", d->batch);
  if (elems >= (1LL << 31) || L * d->batch >= (1LL << 31))
    return fail(SAE_EUNSUPPORTED, "patch_embed: more than 2^31 image elements or tokens");
  memset(g, 0, sizeof *g);
  g->Nb = d->batch;
  g->Himg = d->height;
  g->Wimg = d->width;
  g->C = d->channels;
  g->Ph = d->patch_h;
  g->Pw = d->patch_w;
  g->gw = d->width / d->patch_w;
  g->L = (int)L;
  g->PwC = d->patch_w * d->channels;
  g->WC = d->width * d->channels;
  g->dL = FDiv::make((unsigned)L);
  g->dNb = FDiv::make((unsigned)d->batch);
  g->dgw = FDiv::make((unsigned)g->gw);
  g->dPwC = FDiv::make((unsigned)g->PwC);
  *M = (int)(L * d->batch);
  *K = (int)k;
  return 0;
}

template <bool HWCN, bool F32> int patch_dw_launch(hipStream_t st, const DwArgs& a) {
  using YL = typename std::conditional<HWCN, DwPermY, DwRow<true>>::type;
  return launch("patch_embed_dw",
                a.db ? gemm_dw_kernel<true, DwPatchX<HWCN, F32>, YL> : gemm_dw_kernel<false, DwPatchX<HWCN, F32>, YL>,
                dw_grid(a), dim3(256), 4 * kDwK * 256, st, a);
}

}  // namespace

extern "C" {

size_t sae_gemm_dw_workspace_bytes(int32_t M, int32_t I, int32_t J) {
  if (M < 1 || I < 1 || J < 1) return 0;
  int S, chunk;
  dw_plan(M, I, J, &S, &chunk);
  return dw_part_bytes(S, I, J) + (((size_t)S * J * 4 + 255) & ~(size_t)255);
}

int sae_gemm_dw(void* stream, int32_t M, int32_t I, int32_t J, const void* x, int64_t ldx, const void* dy,
                int64_t ldy, float* dw, int64_t ldw, float* db, int32_t accumulate, void* workspace) {
  return gemm_dw_impl(stream, M, I, J, x, ldx, dy, ldy, dw, ldw, db, accumulate, workspace, 0);
}

int sae_gemm_dw_blocked(void* stream, int32_t M, int32_t I, int32_t J, int32_t jblock, const void* x, int64_t ldx,
                        const void* dy, int64_t ldy, float* dw, float* db, int32_t accumulate, void* workspace) {
  if (jblock < 4 || jblock % 4 || J % jblock)
    return fail(SAE_EINVAL, "gemm_dw_blocked: jblock (%d) must be a multiple of 4 dividing J (%d)", jblock, J);
  return gemm_dw_impl(stream, M, I, J, x, ldx, dy, ldy, dw, J, db, accumulate, workspace, jblock);
}

size_t sae_gemm_f32_workspace_bytes(int32_t M, int32_t N, int32_t K) {
  if (M < 1 || N < 1 || K < 1) return 0;
  int S, c;
  f32_plan(M, N, K, &S, &c);
  return S > 1 ? (size_t)S * (M + 1) * N * 4 : 0;
}

int sae_gemm_f32(void* stream, int32_t M, int32_t N, int32_t K, const float* a, int64_t sam, int64_t sak,
                 const float* b, int64_t sbk, int64_t sbn, const float* bias, float* c, int64_t ldc,
                 float* colsum, int32_t accumulate, void* workspace) {
  if (M < 1 || N < 1 || K < 1) return fail(SAE_EINVAL, "gemm_f32: M/N/K must be >= 1 (got %d/%d/%d)", M, N, K);
  if (!a || !b || !c) return fail(SAE_EINVAL, "gemm_f32: a, b and c must be non-NULL");
  const bool ak = sak == 1, bk = sbk == 1;
  if (ak ? (sam < K || sam % 4 || K % 4) : (sam != 1 || sak < M || sak % 4 || M % 4))
    return fail(SAE_EUNSUPPORTED, "gemm_f32: A needs unit stride along k (sam >= K, K and sam multiples of 4) "
                "or along m (sak >= M, M and sak multiples of 4); got sam %lld sak %lld", (long long)sam,
                (long long)sak);
  if (bk ? (sbn < K || sbn % 4 || K % 4) : (sbn != 1 || sbk < N || sbk % 4 || N % 4))
    return fail(SAE_EUNSUPPORTED, "gemm_f32: B needs unit stride along k (sbn >= K, K and sbn multiples of 4) "
                "or along n (sbk >= N, N and sbk multiples of 4); got sbk %lld sbn %lld", (long long)sbk,
                (long long)sbn);
  if (ldc < N) return fail(SAE_EINVAL, "gemm_f32: ldc (%lld) < N (%d)", (long long)ldc, N);
  if (!aligned16(a) || !aligned16(b)) return fail(SAE_EINVAL, "gemm_f32: a and b must be 16-byte aligned");
  F32Args g;
  memset(&g, 0, sizeof g);
  g.a = a;
  g.b = b;
  g.bias = bias;
  g.c = c;
  g.colsum = colsum;
  g.sam = sam;
  g.sak = sak;
  g.sbk = sbk;
  g.sbn = sbn;
  g.ldc = ldc;
  g.M = M;
  g.N = N;
  g.K = K;
  g.accumulate = accumulate;
  f32_plan(M, N, K, &g.S, &g.kchunk);
  if (g.S > 1) {
    if (!workspace || !aligned16(workspace))
      return fail(SAE_EINVAL, "gemm_f32: this shape splits K: pass sae_gemm_f32_workspace_bytes() of 16-byte "
                  "aligned workspace");
    g.part = reinterpret_cast<float*>(workspace);
  }
  const int Mx = M + (colsum ? 1 : 0);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((Mx + kF32T - 1) / kF32T, (N + kF32T - 1) / kF32T, g.S);
  if (int rc = launch("gemm_f32",
                      ak ? (bk ? gemm_f32_kernel<true, true> : gemm_f32_kernel<true, false>)
                         : (bk ? gemm_f32_kernel<false, true> : gemm_f32_kernel<false, false>),
                      grid, dim3(256), 0, st, g))
    return rc;
  if (g.S == 1) return 0;
  const long long n = (long long)Mx * N;
  return launch("gemm_f32_reduce", gemm_f32_reduce_kernel, std::min<long long>((n + 255) / 256, 4096), dim3(256), 0, st,
                g);
}

int sae_gemm_nt_route(int32_t M, int32_t N, int32_t K, int32_t epilogue) {
  Inst row;
  return nt_plan(nt_facts(M, N, K, epilogue, false), &row) ? SAE_NT_ROUTE_NONE : inst_route(row);
}

// host-only: the row sae_gemm_nt (dropout != 0: sae_gemm_nt_gelu_dropout) launches, by name
const char* sae_gemm_nt_instance(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t dropout) {
  Inst row;
  if (nt_plan(nt_facts(M, N, K, epilogue, dropout != 0), &row)) return nullptr;
  ok();
  return inst_name(row);
}

// row `index` of the three tables, in table order (the tests hold a pin against every name)
const char* sae_gemm_nt_instance_name(int32_t index) {
  return index >= 0 && index < (int)Inst::count ? inst_name((Inst)index) : nullptr;
}

// plan, validate the operands, fill, launch.  drop != nullptr (epilogue SAE_EPI_GELU_GRAD): the
// _gelu_drop row of the kernel nt_plan routes the plain call to -- same validation, same shape
// envelope, same route
static int gemm_nt_impl(void* stream, int32_t M, int32_t N, int32_t K, const void* a, int64_t lda, const void* bt,
                        int64_t ldb, const float* bias, void* c, int64_t ldc, int32_t epilogue, const void* aux,
                        int64_t ldaux, void* c2, const DropRows* drop) {
  const NtFacts f = nt_facts(M, N, K, epilogue, drop != nullptr);
  Inst row;
  if (int rc = nt_plan(f, &row)) return rc;
  if (lda < K || ldb < K || ldc < N || lda % 8 || ldb % 8 || ldc % 8)
    return fail(SAE_EINVAL, "gemm_nt: bad leading dimensions lda %lld ldb %lld ldc %lld", (long long)lda,
                (long long)ldb, (long long)ldc);
  if (!a || !bt || !c) return fail(SAE_EINVAL, "gemm_nt: a/bt/c must be non-NULL");
  const bool gp = epilogue >= SAE_EPI_GELU_GRAD;   // the gelu' forms: the GELU / GELU' checks and kernels
  if (gp) epilogue -= 2;
  if (epilogue == SAE_EPI_GELU && !c2) return fail(SAE_EINVAL, "gemm_nt: the GELU epilogue needs c2 (pre-activation out)");
  if (epilogue == SAE_EPI_DGELU && (!aux || ldaux < N || ldaux % 8 || bias))
    return fail(SAE_EINVAL, "gemm_nt: the GELU-derivative epilogue needs aux (ldaux >= N, multiple of 8) and no bias");
  if (!aligned16(a) || !aligned16(bt) || !aligned16(c) || !aligned16(c2) || !aligned16(aux) || !aligned16(bias))
    return fail(SAE_EINVAL, "gemm_nt: a, bt, c, c2, aux and bias must be 16-byte aligned");
  if (256LL * std::max(lda, ldb) * 2 >= (1LL << 31))
    return fail(SAE_EUNSUPPORTED, "gemm_nt: a 256-row block exceeds 32-bit buffer addressing");
  NtArgs g;
  memset(&g, 0, sizeof g);
  g.a = reinterpret_cast<const __bf16*>(a);
  g.bt = reinterpret_cast<const __bf16*>(bt);
  g.bias = bias;
  g.aux = reinterpret_cast<const __bf16*>(aux);
  g.gp = gp ? 1 : 0;
  g.nts = g8_nts(row);
  g.c = reinterpret_cast<__bf16*>(c);
  g.c2 = reinterpret_cast<__bf16*>(c2);
  g.M = M;
  g.N = N;
  g.K = K;
  g.lda = lda;
  g.ldb = ldb;
  g.ldc = ldc;
  g.ldaux = ldaux;
  if (drop) g.drop = *drop;
  return run_inst(row, (hipStream_t)stream, g, f.cus);
}

int sae_gemm_nt(void* stream, int32_t M, int32_t N, int32_t K, const void* a, int64_t lda, const void* bt,
                int64_t ldb, const float* bias, void* c, int64_t ldc, int32_t epilogue, const void* aux,
                int64_t ldaux, void* c2) {
  return gemm_nt_impl(stream, M, N, K, a, lda, bt, ldb, bias, c, ldc, epilogue, aux, ldaux, c2, nullptr);
}

int sae_gemm_nt_gelu_dropout(void* stream, int32_t M, int32_t N, int32_t K, const void* a, int64_t lda,
                             const void* bt, int64_t ldb, const float* bias, void* c, int64_t ldc, void* c2,
                             float rate, const uint64_t* rng, uint32_t stream_id) {
  unsigned thr;
  if (int rc = rows_drop_check("gemm_nt_gelu_dropout", rate, rng, 1, &thr)) return rc;
  if (thr == 0) return sae_gemm_nt(stream, M, N, K, a, lda, bt, ldb, bias, c, ldc, SAE_EPI_GELU_GRAD, nullptr, 0, c2);
  const DropRows d = make_drop_rows(rng, stream_id, thr, 0, 1);
  return gemm_nt_impl(stream, M, N, K, a, lda, bt, ldb, bias, c, ldc, SAE_EPI_GELU_GRAD, nullptr, 0, c2, &d);
}

int sae_patch_embed_fwd(void* stream, const sae_patch_desc* d, const void* images, const void* wt, const float* bias,
                        void* out) {
  NtArgs g;
  memset(&g, 0, sizeof g);
  int M, K;
  if (int rc = patch_geom(d, &g.pg, &M, &K)) return rc;
  if (!images || !wt || !out) return fail(SAE_EINVAL, "patch_embed: images/wt/out must be non-NULL");
  if (!aligned16(images) || !aligned16(wt) || !aligned16(out) || !aligned16(bias))
    return fail(SAE_EINVAL, "patch_embed: images, wt, out and bias must be 16-byte aligned");
  g.pg.x = images;
  g.bt = reinterpret_cast<const __bf16*>(wt);
  g.bias = bias;
  g.c = reinterpret_cast<__bf16*>(out);
  g.M = M;
  g.N = d->embed;
  g.K = K;
  g.ldb = K;
  g.ldc = d->embed;
  static const Inst rows[2][2] = {{Inst::patch_nhwc_bf16, Inst::patch_nhwc_f32},
                                  {Inst::patch_hwcn_bf16, Inst::patch_hwcn_f32}};
  return run_inst(rows[d->layout == SAE_LAYOUT_HWCN][d->dtype == SAE_DTYPE_F32], (hipStream_t)stream, g);
}

int sae_patch_gather(void* stream, const sae_patch_desc* d, const void* images, void* patches) {
  PatchGeom g;
  int M, K;
  if (int rc = patch_geom(d, &g, &M, &K)) return rc;
  if (d->layout != SAE_LAYOUT_HWCN) return fail(SAE_EUNSUPPORTED, "patch_gather: HWCN images only");
  if (!images || !patches) return fail(SAE_EINVAL, "patch_gather: images / patches must be non-NULL");
  if (!aligned16(images) || !aligned16(patches))
    return fail(SAE_EINVAL, "patch_gather: images and patches must be 16-byte aligned");
  g.x = images;
  const dim3 grid((unsigned)g.L, (unsigned)((g.Nb + 63) / 64), (unsigned)((K / 8 + 3) / 4));
  return launch("patch_gather", d->dtype == SAE_DTYPE_F32 ? patch_gather_hwcn_kernel<true> : patch_gather_hwcn_kernel<false>,
                grid, dim3(256), 0, (hipStream_t)stream, g, reinterpret_cast<__bf16*>(patches), K);
}

size_t sae_patch_embed_bwd_workspace_bytes(const sae_patch_desc* d) {
  PatchGeom g;
  int M, K;
  if (patch_geom(d, &g, &M, &K)) return 0;
  return sae_gemm_dw_workspace_bytes(M, K, d->embed);
}

int sae_patch_embed_bwd(void* stream, const sae_patch_desc* d, const void* images, const void* dout, float* dw,
                        float* db, int32_t accumulate, void* workspace) {
  DwArgs a;
  memset(&a, 0, sizeof a);
  int M, K;
  if (int rc = patch_geom(d, &a.pg, &M, &K)) return rc;
  if (!images || !dout || !dw || !workspace)
    return fail(SAE_EINVAL, "patch_embed_bwd: images/dout/dw/workspace must be non-NULL");
  if (!aligned16(images) || !aligned16(dout) || !aligned16(dw) || !aligned16(db) || !aligned16(workspace))
    return fail(SAE_EINVAL, "patch_embed_bwd: images, dout, dw, db and workspace must be 16-byte aligned");
  const int J = d->embed;
  a.pg.x = images;
  a.dy = reinterpret_cast<const __bf16*>(dout);
  a.M = M;
  a.I = K;
  a.J = J;
  dw_plan(M, K, J, &a.S, &a.chunk);
  if ((long long)a.chunk * J * 2 >= (1LL << 31))
    return fail(SAE_EUNSUPPORTED, "patch_embed_bwd: token chunk exceeds 32-bit buffer addressing");
  a.part = reinterpret_cast<float*>(workspace);
  a.bpart = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + dw_part_bytes(a.S, K, J));
  a.dw = dw;
  a.db = db;
  a.ldy = J;
  a.ldw = J;
  a.accumulate = accumulate;
  hipStream_t st = (hipStream_t)stream;
  const bool hwcn = d->layout == SAE_LAYOUT_HWCN, f32 = d->dtype == SAE_DTYPE_F32;
  if (int rc = hwcn ? (f32 ? patch_dw_launch<true, true>(st, a) : patch_dw_launch<true, false>(st, a))
                    : (f32 ? patch_dw_launch<false, true>(st, a) : patch_dw_launch<false, false>(st, a)))
    return rc;
  return dw_reduce("patch_embed_dw_reduce", a, st);
}

int sae_weight_cast(void* stream, int32_t K, int32_t N, const float* w, void* w16, void* wt16) {
  if (K < 1 || N < 1) return fail(SAE_EINVAL, "weight_cast: K/N must be >= 1 (got %d/%d)", K, N);
  if (!w || (!w16 && !wt16)) return fail(SAE_EINVAL, "weight_cast: w and at least one output must be non-NULL");
  return launch("weight_cast", weight_cast_kernel, dim3((N + 31) / 32, (K + 31) / 32), dim3(256), 0, (hipStream_t)stream,
                w, reinterpret_cast<__bf16*>(w16), reinterpret_cast<__bf16*>(wt16), K, N);
}

int sae_weight_cast_multi(void* stream, int32_t n, const sae_weight_cast_item* items) {
  if (n < 0 || (n > 0 && !items)) return fail(SAE_EINVAL, "weight_cast_multi: bad item list");
  hipStream_t st = (hipStream_t)stream;
  for (int base = 0; base < n; base += kCastMax) {
    CastList L;
    memset(&L, 0, sizeof L);
    L.n = std::min(kCastMax, n - base);
    long long tiles = 0;
    for (int j = 0; j < L.n; ++j) {
      const sae_weight_cast_item& s = items[base + j];
      if (!s.w || s.K < 1 || s.N < 1 || (!s.w16 && !s.wt16) || s.col0 < 0 ||
          (s.w16 && s.ld16 < s.col0 + s.N) || (s.wt16 && s.ldT < s.K))
        return fail(SAE_EINVAL, "weight_cast_multi: item %d invalid (K %d N %d ld16 %d ldT %d col0 %d)", base + j,
                    s.K, s.N, s.ld16, s.ldT, s.col0);
      CastItem& c = L.it[j];
      c.w = s.w;
      c.w16 = reinterpret_cast<__bf16*>(s.w16);
      c.wt16 = reinterpret_cast<__bf16*>(s.wt16);
      c.K = s.K;
      c.N = s.N;
      c.ld16 = s.ld16;
      c.ldT = s.ldT;
      c.col0 = s.col0;
      const auto a8 = [](const void* p) { return ((uintptr_t)p & 7) == 0; };
      c.vec = s.K % 4 == 0 && s.N % 4 == 0 && s.col0 % 4 == 0 && aligned16(s.w) &&
              (!s.w16 || (s.ld16 % 4 == 0 && a8(s.w16))) && (!s.wt16 || (s.ldT % 4 == 0 && a8(s.wt16)));
      c.tiles = c.vec ? ((s.K + 63) / 64) * ((s.N + 63) / 64) : ((s.K + 31) / 32) * ((s.N + 31) / 32);
      tiles += c.tiles;
    }
    if (tiles >= (1LL << 31)) return fail(SAE_EUNSUPPORTED, "weight_cast_multi: too many tiles");
    if (int rc = launch("weight_cast_multi", weight_cast_multi_kernel, tiles, dim3(256), 0, st, L)) return rc;
  }
  return ok();
}

}  // extern "C"
