// Host-side AddressSanitizer run of the C ABI ("race detection / sanitizers":
// the reference has none; this is the host half of the plan -- GPU ASan is not available on the
// MI355X pool).  Built by tools/asan/build.sh with the host code of every unit instrumented
// (-Xarch_host -fsanitize=address); needs no GPU.  It drives every host-only code path of the ABI
// with exact-capacity heap tables, so any overrun of a caller buffer or a descriptor is caught:
//   * the AdamW chunk / tile planners (host only: they write the tables the caller allocated), on
//     random item lists, at exact capacity and one short (must refuse, not overrun);
//   * every workspace-size function over a sweep of shapes (no overflow, no negative sizes);
//   * the validation of every launcher (bad shapes, strides, alignment, NULLs): the error code and
//     sae_last_error() text, read back each time;
//   * the attention route queries against their entry points, over a sweep of descriptors.
// Launchers whose arguments pass validation would launch: with no GPU the HIP launch fails and
// the ABI reports SAE_EHIP, which is the expected outcome here (no device memory is touched).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "sae_attn.h"

static int g_checks = 0, g_fail = 0;

static void expect(bool ok, const char* what) {
  ++g_checks;
  if (!ok) {
    ++g_fail;
    std::printf("FAIL %s (last error: %s)\n", what, sae_last_error());
  }
}

// a heap block per fake pointer, so a host-side dereference would be an ASan report
static void* fake(size_t bytes = 4096) {
  void* p = nullptr;
  if (posix_memalign(&p, 256, bytes)) std::abort();
  std::memset(p, 0, bytes);
  return p;
}

static void adamw_plans(std::mt19937& rng) {
  for (int trial = 0; trial < 200; ++trial) {
    const int n = 1 + rng() % 40;
    std::vector<float*> p(n), m(n), v(n);
    std::vector<const float*> g(n);
    std::vector<int64_t> sz(n);
    int64_t need = 0;
    for (int i = 0; i < n; ++i) {
      sz[i] = 1 + rng() % 20000;
      // misaligned starts on purpose (the plan marks those chunks scalar)
      p[i] = reinterpret_cast<float*>(0x100000 + 4 * (rng() % 7) + 0x1000000LL * i);
      g[i] = p[i] + 1;
      m[i] = p[i] + 2;
      v[i] = p[i] + 3;
      need += (sz[i] + SAE_ADAMW_CHUNK - 1) / SAE_ADAMW_CHUNK;
    }
    sae_adamw_chunk* exact = new sae_adamw_chunk[need];
    int64_t got = -1;
    expect(sae_adamw_plan(n, p.data(), g.data(), m.data(), v.data(), sz.data(), exact, need, &got) == SAE_OK &&
               got == need,
           "adamw_plan at exact capacity");
    int64_t total = 0;
    for (int64_t c = 0; c < got; ++c) total += exact[c].n;
    int64_t want = 0;
    for (int i = 0; i < n; ++i) want += sz[i];
    expect(total == want, "adamw_plan covers every element once");
    delete[] exact;
    if (need > 1) {
      sae_adamw_chunk* shrt = new sae_adamw_chunk[need - 1];
      expect(sae_adamw_plan(n, p.data(), g.data(), m.data(), v.data(), sz.data(), shrt, need - 1, &got) != SAE_OK,
             "adamw_plan refuses a short table");
      delete[] shrt;
    }
  }
  for (int trial = 0; trial < 200; ++trial) {
    const int n = 1 + rng() % 12;
    std::vector<float*> p(n), m(n), v(n);
    std::vector<const float*> g(n);
    std::vector<int32_t> K(n), N(n), ld16(n), ldT(n), col0(n);
    std::vector<void*> w16(n), wt16(n);
    int64_t need = 0;
    for (int i = 0; i < n; ++i) {
      K[i] = 4 * (1 + rng() % 300);
      N[i] = 4 * (1 + rng() % 300);
      col0[i] = 4 * (rng() % 8);
      ld16[i] = N[i] + col0[i] + 4 * (rng() % 3);
      ldT[i] = K[i] + 4 * (rng() % 3);
      p[i] = reinterpret_cast<float*>(0x200000LL + 0x10000000LL * i);
      g[i] = p[i] + 0x1000000;
      m[i] = p[i] + 0x2000000;
      v[i] = p[i] + 0x3000000;
      w16[i] = rng() % 4 ? reinterpret_cast<void*>(p[i] + 0x4000000) : nullptr;
      wt16[i] = (rng() % 4 || !w16[i]) ? reinterpret_cast<void*>(p[i] + 0x5000000) : nullptr;   // >= 1 copy
      need += (int64_t)((K[i] + 63) / 64) * ((N[i] + 63) / 64);
    }
    sae_adamw_cast_tile* exact = new sae_adamw_cast_tile[need];
    int64_t got = -1;
    expect(sae_adamw_cast_plan(n, p.data(), g.data(), m.data(), v.data(), K.data(), N.data(), w16.data(),
                               ld16.data(), wt16.data(), ldT.data(), col0.data(), exact, need, &got) == SAE_OK &&
               got == need,
           "adamw_cast_plan at exact capacity");
    delete[] exact;
    sae_adamw_cast_tile* shrt = new sae_adamw_cast_tile[need - 1 > 0 ? need - 1 : 1];
    if (need > 1)
      expect(sae_adamw_cast_plan(n, p.data(), g.data(), m.data(), v.data(), K.data(), N.data(), w16.data(),
                                 ld16.data(), wt16.data(), ldT.data(), col0.data(), shrt, need - 1, &got) != SAE_OK,
             "adamw_cast_plan refuses a short table");
    delete[] shrt;
  }
  {   // an item with neither copy is refused
    float* p = reinterpret_cast<float*>(0x400000);
    const float* g = p + 4096;
    float *m = p + 8192, *v = p + 12288;
    void* none = nullptr;
    const int32_t K = 64, N = 64, ld = 64, col0 = 0;
    sae_adamw_cast_tile t[1];
    int64_t got = -1;
    expect(sae_adamw_cast_plan(1, &p, &g, &m, &v, &K, &N, &none, &ld, &none, &ld, &col0, t, 1, &got) == SAE_EINVAL,
           "adamw_cast_plan refuses an item with no bf16 copy");
  }
}

static void workspace_sizes() {
  const int dims[] = {1, 7, 64, 197, 384, 577, 1152, 3072, 25216, 100000};
  for (int a : dims)
    for (int b : dims)
      for (int c : dims) {
        expect(sae_gemm_dw_workspace_bytes(a, b, c) < ((size_t)1 << 44), "gemm_dw workspace bounded");
        expect(sae_gemm_f32_workspace_bytes(a, b, c) < ((size_t)1 << 44), "gemm_f32 workspace bounded");
        expect(sae_layernorm_bwd_workspace_bytes(a, b % 4097 + 4) < ((size_t)1 << 40), "ln workspace bounded");
      }
  sae_attn_desc d;
  for (int n : {1, 17, 197, 577, 3136})
    for (int h : {1, 6, 12, 16})
      for (int dd : {6, 10, 32, 48, 64, 128}) {
        sae_attn_desc_init(&d, 3, h, n, n, dd, SAE_DTYPE_BF16, 0.125f);
        expect(sae_attn_bwd_workspace_bytes(&d) < ((size_t)1 << 40), "attn bwd workspace bounded");
        expect(sae_th_attn_bwd_workspace_bytes(&d) < ((size_t)1 << 40), "th bwd workspace bounded");
      }
  sae_patch_desc pd = {8, 224, 224, 3, 16, 16, 384, SAE_LAYOUT_HWCN, SAE_DTYPE_F32};
  expect(sae_patch_embed_bwd_workspace_bytes(&pd) > 0, "patch workspace");
}

static void validation() {
  void *q = fake(), *k = fake(), *v = fake(), *o = fake();
  float* lse = static_cast<float*>(fake());
  sae_attn_desc d;
  sae_attn_desc_init(&d, 2, 4, 64, 64, 64, SAE_DTYPE_BF16, 0.125f);
  d.head_dim = 0;
  expect(sae_attn_fwd(nullptr, &d, q, k, v, nullptr, nullptr, o, lse) == SAE_EINVAL, "head_dim 0");
  expect(std::strlen(sae_last_error()) > 0, "error text");
  sae_attn_desc_init(&d, 2, 4, 64, 64, 256, SAE_DTYPE_BF16, 0.125f);
  expect(sae_attn_fwd(nullptr, &d, q, k, v, nullptr, nullptr, o, lse) == SAE_EUNSUPPORTED, "head_dim 256");
  sae_attn_desc_init(&d, 2, 4, 64, 64, 64, 7, 0.125f);
  expect(sae_attn_fwd(nullptr, &d, q, k, v, nullptr, nullptr, o, lse) != SAE_OK, "bad dtype");
  sae_attn_desc_init(&d, 2, 4, 64, 64, 64, SAE_DTYPE_BF16, 0.125f);
  expect(sae_attn_fwd(nullptr, &d, nullptr, k, v, nullptr, nullptr, o, lse) == SAE_EINVAL, "null q");
  expect(sae_attn_fwd(nullptr, nullptr, q, k, v, nullptr, nullptr, o, lse) == SAE_EINVAL, "null desc");
  d.flags = SAE_FLAG_RELPOS;
  d.rel_h = 3;
  d.rel_w = 5;   // 15 != seq_k
  expect(sae_attn_fwd(nullptr, &d, q, k, v, lse, lse, o, lse) != SAE_OK, "relpos grid != seq_k");
  // launches that pass validation: no GPU here, so the HIP launch must fail cleanly
  sae_attn_desc_init(&d, 1, 1, 16, 16, 64, SAE_DTYPE_BF16, 0.125f);
  const int rc = sae_attn_fwd(nullptr, &d, q, k, v, nullptr, nullptr, o, lse);
  expect(rc == SAE_OK || rc == SAE_EHIP, "valid launch without a GPU: SAE_EHIP");
  // dropout entry points: rate, rng and flags are refused on the host
  const uint64_t* rng = static_cast<const uint64_t*>(fake());
  expect(sae_attn_fwd_dropout(nullptr, &d, q, k, v, o, lse, 1.0f, rng, 0) == SAE_EINVAL, "dropout rate 1");
  expect(sae_attn_fwd_dropout(nullptr, &d, q, k, v, o, lse, 0.1f, nullptr, 0) == SAE_EINVAL, "dropout null rng");
  expect(sae_attn_bwd_dropout(nullptr, &d, q, k, v, o, lse, o, q, k, v, fake(), -0.1f, rng, 0) == SAE_EINVAL,
         "dropout rate < 0");
  d.flags = SAE_FLAG_RELPOS;
  expect(sae_attn_fwd_dropout(nullptr, &d, q, k, v, o, lse, 0.1f, rng, 0) == SAE_EUNSUPPORTED, "dropout + relpos");
  expect(sae_attn_dropout_mask(nullptr, 1, 1, 4, 4, 0.5f, nullptr, 0, static_cast<uint8_t*>(fake())) == SAE_EINVAL,
         "mask null rng");
  expect(sae_dropout_advance(nullptr, nullptr, 1) == SAE_EINVAL, "advance null rng");

  expect(sae_gemm_nt(nullptr, 128, 128, 60, q, 64, k, 64, nullptr, o, 128, SAE_EPI_NONE, nullptr, 0, nullptr) ==
             SAE_EUNSUPPORTED,
         "gemm_nt K % 64");
  expect(sae_gemm_nt(nullptr, 0, 128, 64, q, 64, k, 64, nullptr, o, 128, SAE_EPI_NONE, nullptr, 0, nullptr) ==
             SAE_EINVAL,
         "gemm_nt M 0");
  float* fa = static_cast<float*>(fake());
  expect(sae_gemm_f32(nullptr, 64, 64, 30, fa, 30, 1, fa, 64, 1, nullptr, fa, 64, nullptr, 0, nullptr) ==
             SAE_EUNSUPPORTED,
         "gemm_f32 K % 4 (k-contiguous A)");
  expect(sae_gemm_f32(nullptr, 64, 64, 32, fa, 3, 2, fa, 64, 1, nullptr, fa, 64, nullptr, 0, nullptr) ==
             SAE_EUNSUPPORTED,
         "gemm_f32 no unit stride");
  expect(sae_gemm_f32(nullptr, 64, 64, 32, fa + 1, 32, 1, fa, 64, 1, nullptr, fa, 64, nullptr, 0, nullptr) ==
             SAE_EINVAL,
         "gemm_f32 misaligned a");
  expect(sae_gemm_f32(nullptr, 64, 64, 100000, fa, 100000, 1, fa, 64, 1, nullptr, fa, 64, nullptr, 0, nullptr) ==
             SAE_EINVAL,
         "gemm_f32 split without workspace");
  expect(sae_gemm_dw(nullptr, 64, 12, 16, q, 12, k, 16, fa, 16, nullptr, 0, fake()) == SAE_EUNSUPPORTED,
         "gemm_dw I % 8");
  expect(sae_gemm_dw_blocked(nullptr, 64, 16, 24, 5, q, 16, k, 24, fa, nullptr, 0, fake()) == SAE_EINVAL,
         "gemm_dw_blocked jblock");
  std::vector<sae_weight_cast_item> items(100);
  expect(sae_weight_cast_multi(nullptr, 100, items.data()) != SAE_OK, "weight_cast_multi too many items");
  expect(sae_layernorm_fwd(nullptr, 16, 6, fa, nullptr, fa, fa, fa, q, fa, fa, 1e-6f) != SAE_OK, "layernorm C % 4");
  sae_patch_desc pd = {8, 224, 224, 3, 16, 16, 384, SAE_LAYOUT_HWCN, SAE_DTYPE_F32};
  pd.patch_h = 15;
  expect(sae_patch_embed_fwd(nullptr, &pd, q, k, nullptr, o) != SAE_OK, "patch not dividing the image");
  expect(sae_tokens_fwd(nullptr, 2, 196, 6, q, fa, fa, fa) != SAE_OK, "tokens E % 4");
  expect(sae_smoothed_ce_fwd(nullptr, 0, 1000, q, 1000, SAE_DTYPE_BF16, static_cast<const int64_t*>(fake()), 0.1f,
                             fa, fa, fa) != SAE_OK,
         "ce zero rows");
  // the mixed loss, its backward and the evaluation accumulator: every refusal on the host
  {
    const int64_t* lab = static_cast<const int64_t*>(fake());
    const int64_t* mix = static_cast<const int64_t*>(fake());
    int32_t* rank = static_cast<int32_t*>(fake());
    expect(sae_mixed_ce_fwd(nullptr, 0, 1000, q, 1000, SAE_DTYPE_BF16, lab, nullptr, nullptr, 0.1f, fa, fa, nullptr,
                            fa, nullptr) == SAE_EINVAL,
           "mixed_ce_fwd zero rows");
    expect(sae_mixed_ce_fwd(nullptr, SAE_CE_MAX_ROWS + 1, 1000, q, 1000, SAE_DTYPE_BF16, lab, nullptr, nullptr, 0.1f,
                            fa, fa, nullptr, fa, nullptr) == SAE_EINVAL,
           "mixed_ce_fwd too many rows");
    expect(sae_mixed_ce_fwd(nullptr, 8, 1000, q, 999, SAE_DTYPE_BF16, lab, nullptr, nullptr, 0.1f, fa, fa, nullptr, fa,
                            nullptr) == SAE_EINVAL,
           "mixed_ce_fwd ld < classes");
    expect(sae_mixed_ce_fwd(nullptr, 8, 1000, q, 1000, 9, lab, nullptr, nullptr, 0.1f, fa, fa, nullptr, fa, nullptr) ==
               SAE_EINVAL,
           "mixed_ce_fwd bad dtype");
    expect(sae_mixed_ce_fwd(nullptr, 8, 1000, nullptr, 1000, SAE_DTYPE_BF16, lab, nullptr, nullptr, 0.1f, fa, fa,
                            nullptr, fa, nullptr) == SAE_EINVAL,
           "mixed_ce_fwd null logits");
    expect(sae_mixed_ce_fwd(nullptr, 8, 1000, q, 1000, SAE_DTYPE_BF16, nullptr, nullptr, nullptr, 0.1f, fa, fa,
                            nullptr, fa, nullptr) == SAE_EINVAL,
           "mixed_ce_fwd null labels");
    expect(sae_mixed_ce_fwd(nullptr, 8, 1000, q, 1000, SAE_DTYPE_BF16, lab, nullptr, fa, 0.1f, fa, fa, nullptr, fa,
                            nullptr) == SAE_EINVAL,
           "mixed_ce_fwd ratio without mix_labels");
    expect(sae_mixed_ce_fwd(nullptr, 8, 1000, q, 1000, SAE_DTYPE_BF16, lab, mix, nullptr, 0.1f, fa, fa, nullptr, fa,
                            nullptr) == SAE_EINVAL,
           "mixed_ce_fwd mix_labels without ratio");
    expect(sae_mixed_ce_fwd(nullptr, 8, 1000, q, 1000, SAE_DTYPE_BF16, lab, mix, fa, 0.1f, fa, fa, rank, fa, nullptr) ==
               SAE_EINVAL,
           "mixed_ce_fwd rank without top");
    expect(sae_mixed_ce_fwd(nullptr, 8, 1000, q, 1000, SAE_DTYPE_BF16, lab, mix, fa, 0.1f, fa, fa, nullptr, nullptr,
                            nullptr) == SAE_EINVAL,
           "mixed_ce_fwd null loss");
    int rc3 = sae_mixed_ce_fwd(nullptr, 8, 1000, q, 1000, SAE_DTYPE_BF16, lab, mix, fa, 0.1f, fa, fa, rank, fa, fa);
    expect(rc3 == SAE_OK || rc3 == SAE_EHIP, "mixed_ce_fwd: valid launch without a GPU");
    expect(sae_mixed_ce_bwd(nullptr, 0, 1000, q, 1000, SAE_DTYPE_BF16, lab, nullptr, nullptr, 0.1f, fa, fa, o, 1000) ==
               SAE_EINVAL,
           "mixed_ce_bwd zero rows");
    expect(sae_mixed_ce_bwd(nullptr, 8, 1000, q, 1000, SAE_DTYPE_BF16, lab, nullptr, fa, 0.1f, fa, fa, o, 1000) ==
               SAE_EINVAL,
           "mixed_ce_bwd ratio without mix_labels");
    expect(sae_mixed_ce_bwd(nullptr, 8, 1000, q, 1000, SAE_DTYPE_BF16, lab, mix, fa, 0.1f, fa, fa, o, 999) ==
               SAE_EINVAL,
           "mixed_ce_bwd ldd < classes");
    expect(sae_mixed_ce_bwd(nullptr, 8, 1000, q, 1000, SAE_DTYPE_BF16, lab, mix, fa, 0.1f, nullptr, fa, o, 1000) ==
               SAE_EINVAL,
           "mixed_ce_bwd null lse");
    expect(sae_mixed_ce_bwd(nullptr, 8, 1000, q, 1000, SAE_DTYPE_BF16, lab, mix, fa, 0.1f, fa, fa, nullptr, 1000) ==
               SAE_EINVAL,
           "mixed_ce_bwd null dlogits");
    void* acc = fake(SAE_CE_ACCUM_BYTES);
    expect(sae_ce_accumulate(nullptr, 0, fa, rank, acc) == SAE_EINVAL, "ce_accumulate zero rows");
    expect(sae_ce_accumulate(nullptr, SAE_CE_MAX_ROWS + 1, fa, rank, acc) == SAE_EINVAL, "ce_accumulate too many rows");
    expect(sae_ce_accumulate(nullptr, 8, nullptr, rank, acc) == SAE_EINVAL, "ce_accumulate null row_loss");
    expect(sae_ce_accumulate(nullptr, 8, fa, nullptr, acc) == SAE_EINVAL, "ce_accumulate null rank");
    expect(sae_ce_accumulate(nullptr, 8, fa, rank, nullptr) == SAE_EINVAL, "ce_accumulate null acc");
    expect(sae_ce_accumulate(nullptr, 8, fa, rank, static_cast<char*>(acc) + 4) == SAE_EINVAL,
           "ce_accumulate misaligned acc");
    rc3 = sae_ce_accumulate(nullptr, 8, fa, rank, acc);
    expect(rc3 == SAE_OK || rc3 == SAE_EHIP, "ce_accumulate: valid launch without a GPU");
  }
  // clip + schedule around AdamW: every refusal on the host, the schedule read from the caller's struct only
  {
    int32_t* step = static_cast<int32_t*>(fake());
    float* hyper = static_cast<float*>(fake(16));
    void* ws = fake(sae_adamw_prepare_workspace_bytes(100000));
    sae_lr_schedule* s = new sae_lr_schedule{SAE_LR_WARMUP_COSINE, 0.f, 1e-3f, 1e-5f, 2, 10};
    expect(sae_adamw_prepare(nullptr, 100000, fa, 1.f, nullptr, step, ws, hyper) == SAE_EINVAL, "prepare null schedule");
    expect(sae_adamw_prepare(nullptr, 0, fa, 1.f, s, step, ws, hyper) == SAE_EINVAL, "prepare n 0 with buffers");
    expect(sae_adamw_prepare(nullptr, 100000, fa, 0.f, s, step, ws, hyper) == SAE_EINVAL, "prepare max_norm 0");
    expect(sae_adamw_prepare(nullptr, 100000, fa, NAN, s, step, ws, hyper) == SAE_EINVAL, "prepare max_norm NaN");
    s->decay_steps = 2;
    expect(sae_adamw_prepare(nullptr, 100000, fa, 1.f, s, step, ws, hyper) == SAE_EINVAL, "prepare decay <= warmup");
    s->decay_steps = 10;
    s->peak = 0.f;
    expect(sae_adamw_prepare(nullptr, 100000, fa, 1.f, s, step, ws, hyper) == SAE_EINVAL, "prepare peak 0");
    s->peak = 1e-3f;
    int rc2 = sae_adamw_prepare(nullptr, 100000, fa, INFINITY, s, step, ws, hyper);
    expect(rc2 == SAE_OK || rc2 == SAE_EHIP, "prepare: valid launch without a GPU");
    rc2 = sae_adamw_prepare(nullptr, 0, nullptr, INFINITY, s, step, nullptr, hyper);
    expect(rc2 == SAE_OK || rc2 == SAE_EHIP, "prepare, schedule alone: valid launch without a GPU");
    expect(sae_adamw_step_dev(nullptr, 1, nullptr, 0, nullptr, step, hyper, 0.9f, 0.999f, 1e-8f, 1e-4f) == SAE_EINVAL,
           "step_dev null chunks");
    expect(sae_adamw_step_dev(nullptr, 0, nullptr, 0, nullptr, step, nullptr, 0.9f, 0.999f, 1e-8f, 1e-4f) == SAE_EINVAL,
           "step_dev null hyper");
    delete s;
    for (int64_t n : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)SAE_ADAMW_NORM_SPAN, (int64_t)1 << 40})
      expect(sae_adamw_prepare_workspace_bytes(n) == (n < 1 ? 0 : (size_t)((n - 1) / SAE_ADAMW_NORM_SPAN + 1) * 8),
             "prepare workspace bytes");
  }
  expect(sae_abi_version() == SAE_ABI_VERSION, "abi version");
  expect(std::strlen(sae_build_info()) > 0, "build info");
}

// sae_attn_route / sae_th_attn_route name a route exactly when the matching entry point gets as far
// as the launch (SAE_EHIP without a GPU) and return NULL exactly when it refuses on the host.
static void routes_agree() {
  char* base = static_cast<char*>(fake(1 << 16));
  float *lse = static_cast<float*>(fake()), *sn = static_cast<float*>(fake()), *cs = static_cast<float*>(fake());
  float *th1 = static_cast<float*>(fake()), *th2 = static_cast<float*>(fake()), *dth1 = static_cast<float*>(fake()),
        *dth2 = static_cast<float*>(fake());
  void* ws = fake();
  const uint64_t* rng = static_cast<const uint64_t*>(fake());
  auto launched = [](int rc) { return rc == SAE_EHIP || rc == SAE_OK; };
  auto refused = [](int rc) { return rc == SAE_EINVAL || rc == SAE_EUNSUPPORTED; };
  for (int dtype : {SAE_DTYPE_F32, SAE_DTYPE_BF16})
    for (int D : {8, 10, 32, 40, 48, 64, 128})
      for (int Nq : {1, 50})
        for (int Nk : {50, 300})
          for (int H : {4, 12})
            for (int aligned : {0, 1})
              for (int form : {SAE_FORM_PLAIN, SAE_FORM_ROTARY, SAE_FORM_DROPOUT})
                for (int pass : {SAE_PASS_FWD, SAE_PASS_BWD}) {
                  sae_attn_desc d;
                  sae_attn_desc_init(&d, 2, H, Nq, Nk, D, dtype, 0.125f);
                  // one tensor off the 16-byte grid makes the call unaligned
                  void *q = base + (aligned ? 0 : 4), *k = base + 4096, *v = base + 8192, *o = base + 12288,
                       *dout = base + 16384, *dq = base + 20480, *dk = base + 24576, *dv = base + 28672;
                  int rc, rt = SAE_EUNSUPPORTED;   // talking heads has no dropout entry point
                  if (form == SAE_FORM_PLAIN) {
                    rc = pass ? sae_attn_bwd(nullptr, &d, q, k, v, o, lse, dout, nullptr, nullptr, dq, dk, dv, nullptr,
                                             nullptr, ws)
                              : sae_attn_fwd(nullptr, &d, q, k, v, nullptr, nullptr, o, lse);
                    rt = pass ? sae_th_attn_bwd(nullptr, &d, q, k, v, th1, th2, lse, dout, dq, dk, dv, dth1, dth2, ws)
                              : sae_th_attn_fwd(nullptr, &d, q, k, v, th1, th2, o, lse);
                  } else if (form == SAE_FORM_ROTARY) {
                    rc = pass ? sae_attn_bwd_rotary(nullptr, &d, q, k, v, o, lse, dout, sn, cs, dq, dk, dv, ws)
                              : sae_attn_fwd_rotary(nullptr, &d, q, k, v, sn, cs, o, lse);
                    rt = pass ? sae_th_attn_bwd_rotary(nullptr, &d, q, k, v, th1, th2, lse, dout, sn, cs, dq, dk, dv,
                                                       dth1, dth2, ws)
                              : sae_th_attn_fwd_rotary(nullptr, &d, q, k, v, th1, th2, sn, cs, o, lse);
                  } else {
                    rc = pass ? sae_attn_bwd_dropout(nullptr, &d, q, k, v, o, lse, dout, dq, dk, dv, ws, 0.5f, rng, 3)
                              : sae_attn_fwd_dropout(nullptr, &d, q, k, v, o, lse, 0.5f, rng, 3);
                  }
                  const bool ra = sae_attn_route(&d, pass, form, aligned) != nullptr;
                  expect(ra ? launched(rc) : refused(rc), "sae_attn_route agrees with the entry point");
                  const bool rh = sae_th_attn_route(&d, pass, form, aligned) != nullptr;
                  expect(rh ? launched(rt) : refused(rt), "sae_th_attn_route agrees with the entry point");
                }
  expect(sae_attn_route(nullptr, SAE_PASS_FWD, SAE_FORM_PLAIN, 1) == nullptr, "route: null desc");
  expect(sae_th_attn_route(nullptr, SAE_PASS_FWD, SAE_FORM_ROTARY, 1) == nullptr, "th route: null desc");
  sae_attn_desc d;
  sae_attn_desc_init(&d, 1, 1, 16, 16, 64, SAE_DTYPE_BF16, 0.125f);
  expect(sae_attn_route(&d, 2, SAE_FORM_PLAIN, 1) == nullptr && sae_attn_route(&d, SAE_PASS_FWD, 3, 1) == nullptr,
         "route: bad pass / form");
}

// sae_gemm_nt_instance names a row exactly when sae_gemm_nt / sae_gemm_nt_gelu_dropout get as far as
// the launch, its table agrees with sae_gemm_nt_route, and the row list ends in NULL.
static void gemm_rows_agree() {
  void *a = fake(), *bt = fake(), *c = fake(), *c2 = fake(), *aux = fake();
  const uint64_t* rng = static_cast<const uint64_t*>(fake());
  auto launched = [](int rc) { return rc == SAE_EHIP || rc == SAE_OK; };
  auto refused = [](int rc) { return rc == SAE_EINVAL || rc == SAE_EUNSUPPORTED; };
  int rows = 0;
  while (sae_gemm_nt_instance_name(rows)) ++rows;
  expect(rows == 35 && !sae_gemm_nt_instance_name(-1) && !sae_gemm_nt_instance_name(rows + 1), "gemm_nt row list");
  // the shapes tests/_gemm_rows.py pins, the training shapes, and refused ones (M 0, K 12, N 10)
  for (int M : {0, 128, 130, 4000, 4096, 4100, 18464, 25216})
    for (int K : {12, 40, 128, 384, 448, 768, 3072})
      for (int N : {10, 64, 72, 136, 192, 384, 768, 1536, 2688, 3584, 4096})
        for (int epi : {-1, SAE_EPI_NONE, SAE_EPI_GELU, SAE_EPI_DGELU, SAE_EPI_GELU_GRAD, SAE_EPI_MUL_AUX, 5})
          for (int drop : {0, 1}) {
            const char* row = sae_gemm_nt_instance(M, N, K, epi, drop);
            const bool dgelu = epi == SAE_EPI_DGELU || epi == SAE_EPI_MUL_AUX;
            int rc;
            if (drop && epi != SAE_EPI_GELU_GRAD) {
              expect(!row && std::strlen(sae_last_error()) > 0, "gemm_nt instance: dropout needs GELU_GRAD");
              continue;
            }
            if (drop)
              rc = sae_gemm_nt_gelu_dropout(nullptr, M, N, K, a, K, bt, K, nullptr, c, N, c2, 0.25f, rng, 3);
            else
              rc = sae_gemm_nt(nullptr, M, N, K, a, K, bt, K, nullptr, c, N, epi, dgelu ? aux : nullptr, dgelu ? N : 0,
                               c2);
            expect(row ? launched(rc) : refused(rc), "sae_gemm_nt_instance agrees with the entry point");
            const int route = sae_gemm_nt_route(M, N, K, epi);
            expect((row != nullptr) == (route != SAE_NT_ROUTE_NONE), "sae_gemm_nt_instance agrees with the route");
            if (row)
              expect((route == SAE_NT_ROUTE_GEMM8X) == !std::strncmp(row, "g8x_", 4) &&
                         (route == SAE_NT_ROUTE_GEMM8) == !std::strncmp(row, "g8_", 3) &&
                         (route == SAE_NT_ROUTE_TILE128_KTAIL) == !std::strncmp(row, "nt128_ktail_", 12),
                     "row name and route name the same table");
          }
}

int main() {
  std::mt19937 rng(1234);
  adamw_plans(rng);
  workspace_sizes();
  validation();
  routes_agree();
  gemm_rows_agree();
  std::printf("capi_asan: %d checks, %d failed\n", g_checks, g_fail);
  return g_fail ? 1 : 0;
}
