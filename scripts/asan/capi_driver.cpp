// Host sanitizer driver for the C ABI (include/smcdet_hip.h): the library's
// host side compiled with -Xarch_host -fsanitize=address,undefined (device
// code not built: nothing is launched) by `make asan`, run by
// tests/test_sanitizers.py without a GPU.  Every entry point is called with
// the argument errors its validation must reject (null buffers, empty or
// oversized shapes, unknown enums, inconsistent flags) and must return the
// documented negative code with a message, touching no device memory.  The MH
// sweep's launch plan (a pure host function) is checked here too, row by row.
#include <cstdio>
#include <cstring>

#include "../../include/smcdet_hip.h"
#include "../../smcdet_amd/csrc/mh_plan.h"

static int fails = 0;
#define EXPECT(expr, code)                                                         \
  do {                                                                             \
    const long long rc_ = (long long)(expr);                                       \
    if (rc_ != (code)) {                                                           \
      std::printf("FAIL %s -> %lld (want %d): %s\n", #expr, rc_, (code),           \
                  smcdet_last_error());                                            \
      ++fails;                                                                     \
    } else if (std::strlen(smcdet_last_error()) == 0 && (code) != 0) {             \
      std::printf("FAIL %s: empty error message\n", #expr);                       \
      ++fails;                                                                     \
    }                                                                              \
  } while (0)

// The MH sweep's launch plan (smcdet_amd/csrc/mh_plan.h) row by row: which
// instantiation, LDS bytes, tail and store policy each shape gets.  Every
// variant computes the same bits, so only this table sees a wrong choice.
// Unless a row says otherwise: CU count 256, rate_out present, T = 1; the
// base LDS is (images + 4) (H W + 64) 4 B.  fused: smcdet_mh_sweep_step_fused's
// answer (-1: not asked).
namespace {
using namespace smcdet;
struct PlanRow {
  const char* name;
  int model, H, W, R, N, S, T;
  uint32_t flags;
  bool tail, two_launch, rate_out, diag, psf_tab;
  MhVariant variant;
  bool geo_fixed;
  int ppl;
  size_t lds;
  MhTailMode tail_mode;
  bool write_through;
  int fused;
};
constexpr int M = SMCDET_MODEL_M71, P = SMCDET_MODEL_POISSON;
constexpr uint32_t kGen = SMCDET_MH_GENERIC_GEOMETRY, kFull = SMCDET_MH_FULL_RECOMPUTE,
                   kNoWt = SMCDET_MH_NO_WRITE_THROUGH, kNoPc = SMCDET_MH_NO_PSF_CACHE;
constexpr bool T_ = true, F_ = false;
const PlanRow kPlanRows[] = {
    // name, model H W R N S T, flags, tail two rate_out diag tab -> variant geo ppl lds tail wt fused
    {"c2", M, 32, 32, 8, 4096, 10, 1, 0, F_, F_, T_, F_, F_, kMhRV, T_, 16, 39168, kMhNoTail, T_, -1},
    {"c2 generic geometry", M, 32, 32, 8, 4096, 10, 1, kGen, F_, F_, T_, F_, F_, kMhRV, F_, 16, 39168,
     kMhNoTail, T_, -1},
    {"c2 N=4100", M, 32, 32, 8, 4100, 10, 1, 0, F_, F_, T_, F_, F_, kMhRV, T_, 16, 39168, kMhNoTail,
     F_, -1},
    {"c2 T=2", M, 32, 32, 8, 4096, 10, 2, 0, F_, F_, T_, F_, F_, kMhRV, T_, 16, 39168, kMhNoTail, F_,
     -1},
    {"c2 no rate_out", M, 32, 32, 8, 4096, 10, 1, 0, F_, F_, F_, F_, F_, kMhRV, T_, 16, 39168,
     kMhNoTail, F_, -1},
    {"c2 no write-through", M, 32, 32, 8, 4096, 10, 1, kNoWt, F_, F_, T_, F_, F_, kMhRV, T_, 16,
     39168, kMhNoTail, F_, -1},
    {"c2 tail", M, 32, 32, 8, 4096, 10, 1, 0, T_, F_, T_, F_, F_, kMhTail, F_, 16, 32772,
     kMhTailFused, F_, 1},
    {"c2 tail two-launch", M, 32, 32, 8, 4096, 10, 1, 0, T_, T_, T_, F_, F_, kMhRV, T_, 16, 39168,
     kMhTailSplit, T_, -1},
    {"c2 tail N=4094", M, 32, 32, 8, 4094, 10, 1, 0, T_, F_, T_, F_, F_, kMhRV, T_, 16, 39168,
     kMhTailSplit, T_, 0},
    {"c2 tail N=4100", M, 32, 32, 8, 4100, 10, 1, 0, T_, F_, T_, F_, F_, kMhRV, T_, 16, 39168,
     kMhTailSplit, F_, -1},
    {"32x32 R=6", M, 32, 32, 6, 4096, 10, 1, 0, F_, F_, T_, F_, F_, kMhRV, F_, 16, 39168, kMhNoTail,
     T_, -1},
    {"24x40", M, 24, 40, 8, 4096, 10, 1, 0, F_, F_, T_, F_, F_, kMhRV, F_, 16, 9 * 1024 * 4,
     kMhNoTail, T_, -1},
    {"16x16", M, 16, 16, 8, 4096, 10, 1, 0, F_, F_, T_, F_, F_, kMhRV, F_, 4, 11520, kMhNoTail, T_,
     -1},
    {"c2 full", M, 32, 32, 8, 4096, 10, 1, kFull, F_, F_, T_, F_, F_, kMhUnpaired, F_, 16, 21760,
     kMhNoTail, F_, -1},
    {"c2 full tail", M, 32, 32, 8, 4096, 10, 1, kFull, T_, F_, T_, F_, F_, kMhUnpaired, F_, 16, 21760,
     kMhTailSplit, F_, 0},
    {"8x8", M, 8, 8, 8, 4096, 10, 1, 0, F_, F_, T_, F_, F_, kMhPC, F_, 1, 12800, kMhNoTail, F_, -1},
    {"8x8 tail", M, 8, 8, 8, 4096, 10, 1, 0, T_, F_, T_, F_, F_, kMhPC, F_, 1, 12800, kMhTailSplit,
     F_, 0},
    {"8x8 S=19", M, 8, 8, 8, 4096, 19, 1, 0, F_, F_, T_, F_, F_, kMhPC, F_, 1, 22016, kMhNoTail, F_,
     -1},
    {"8x8 S=20", M, 8, 8, 8, 4096, 20, 1, 0, F_, F_, T_, F_, F_, kMhPaired, F_, 1, 2560, kMhNoTail,
     F_, -1},  // 7 (23 040 + 1024) > 160 KiB
    {"8x8 no PSF cache", M, 8, 8, 8, 4096, 10, 1, kNoPc, F_, F_, T_, F_, F_, kMhPaired, F_, 1, 2560,
     kMhNoTail, F_, -1},
    {"8x8 full", M, 8, 8, 8, 4096, 10, 1, kFull, F_, F_, T_, F_, F_, kMhUnpaired, F_, 1, 2560,
     kMhNoTail, F_, -1},
    {"poisson 8x8", P, 8, 8, 8, 4096, 10, 1, 0, F_, F_, T_, F_, F_, kMhPC, F_, 1, 13312, kMhNoTail,
     F_, -1},
    {"poisson 16x16 N=64", P, 16, 16, 8, 64, 10, 1, 0, F_, F_, T_, F_, F_, kMhPaired, F_, 4, 7680,
     kMhNoTail, T_, -1},
    {"64x64", M, 64, 64, 8, 4096, 10, 1, 0, F_, F_, T_, F_, F_, kMhPaired, F_, 0, 83200, kMhNoTail,
     F_, -1},
    {"64x64 tail", M, 64, 64, 8, 4096, 10, 1, 0, T_, F_, T_, F_, F_, kMhPaired, F_, 0, 83200,
     kMhTailSplit, F_, 0},  // 4 (83 200 + 2048) > 160 KiB
    {"128x128", M, 128, 128, 8, 4096, 10, 1, 0, F_, F_, T_, F_, F_, kMhGL, F_, 0, 0, kMhNoTail, F_,
     -1},
    {"128x128 tail", M, 128, 128, 8, 4096, 10, 1, 0, T_, F_, T_, F_, F_, kMhGL, F_, 0, 0,
     kMhTailSplit, F_, 0},
    // the diagnostic build's variants (the table: 513 float4 behind 16-B alignment)
    {"diag c2 scalar slots", M, 32, 32, 8, 4096, 10, 1, SMCDET_MH_SCALAR_SLOTS, F_, F_, T_, T_, F_,
     kMhUnpaired, F_, 16, 21760, kMhNoTail, T_, -1},
    {"diag c2 no 1/v", M, 32, 32, 8, 4096, 10, 1, SMCDET_MH_NO_RCP_CACHE, F_, F_, T_, T_, F_,
     kMhPaired, F_, 16, 21760, kMhNoTail, T_, -1},
    {"diag c2 table", M, 32, 32, 8, 4096, 10, 1, SMCDET_MH_PSF_TABLE, F_, F_, T_, T_, T_, kMhTB, F_,
     16, 21760 + 8208, kMhNoTail, T_, -1},  // with the 1/v image: 4 (47 376 + 1024) > 160 KiB
    {"diag 16x16 table", M, 16, 16, 8, 4096, 10, 1, SMCDET_MH_PSF_TABLE, F_, F_, T_, T_, T_, kMhRVTB,
     F_, 4, 11520 + 8208, kMhNoTail, T_, -1},
    {"diag 8x8 table", M, 8, 8, 8, 4096, 10, 1, SMCDET_MH_PSF_TABLE, F_, F_, T_, T_, T_, kMhPCTB, F_,
     1, 12800 + 8208, kMhNoTail, F_, -1},
};

int plan_table(const smcdet_image_model_t& base) {
  int bad = 0;
  for (const PlanRow& r : kPlanRows) {
    MhPlanIn in{};
    in.model = r.model, in.H = r.H, in.W = r.W, in.R = r.R, in.N = r.N, in.S = r.S, in.T = r.T;
    in.flags = r.flags, in.tail = r.tail, in.two_launch = r.two_launch;
    in.tail_lds = (size_t)(2 * r.N + 1) * 4;
    in.rate_out = r.rate_out, in.psf_tab = r.psf_tab, in.cu_count = 256, in.diag = r.diag;
    const MhPlan p = mh_plan(in);
    if (p.status != SMCDET_OK || p.variant != r.variant || p.geo_fixed != r.geo_fixed ||
        p.ppl != r.ppl || p.lds != r.lds || p.tail != r.tail_mode ||
        p.write_through != r.write_through) {
      std::printf("FAIL plan %s: status %d (%s) variant %d geo %d ppl %d lds %zu tail %d wt %d\n",
                  r.name, p.status, p.msg, (int)p.variant, (int)p.geo_fixed, p.ppl, p.lds,
                  (int)p.tail, (int)p.write_through);
      ++bad;
    }
    if (r.fused >= 0) {
      smcdet_image_model_t m = base;
      m.model = r.model, m.H = r.H, m.W = r.W, m.psf_radius = r.R;
      if (smcdet_mh_sweep_step_fused(&m, r.N, r.S, r.flags) != r.fused) {
        std::printf("FAIL smcdet_mh_sweep_step_fused %s: want %d\n", r.name, r.fused);
        ++bad;
      }
    }
  }
  // the errors the plan keeps (the product refuses the scalar-slots flag earlier)
  MhPlanIn in{};
  in.model = M, in.H = in.W = 128, in.R = 8, in.N = 4096, in.S = 10, in.T = 1, in.diag = true;
  in.flags = SMCDET_MH_SCALAR_SLOTS;
  const MhPlan p = mh_plan(in);
  if (p.status != SMCDET_EUNSUPPORTED ||
      std::strcmp(p.msg, "tiles above 4096 pixels: no fused step / scalar slots") != 0) {
    std::printf("FAIL plan 128x128 scalar slots: status %d (%s)\n", p.status, p.msg);
    ++bad;
  }
  return bad;
}
}  // namespace

int main() {
  std::printf("%s abi %d\n", smcdet_version(), smcdet_abi_version());
  if (smcdet_abi_version() != SMCDET_ABI_VERSION) ++fails;
  smcdet_image_model_t m{};
  m.model = SMCDET_MODEL_M71;
  m.H = m.W = 32;
  m.psf_radius = 8;
  m.background = 104.f;
  m.adu_per_nmgy = 241.f;
  float pp[6] = {1.1f, 2.1f, 2.3f, 5.2f, 0.73f, 0.51f};
  std::memcpy(m.psf_params, pp, sizeof pp);
  m.psf_norm = 12.75f;
  m.noise_additive = 1e-10f;
  m.noise_multiplicative = 1.94f;
  smcdet_prior_t p{};
  p.kind = SMCDET_PRIOR_M71;
  p.min_objects = p.max_objects = 10;
  p.loc_low = -4.f;
  p.loc_high_h = p.loc_high_w = 36.f;
  p.poisson_mean = 4.f;
  p.flux_alpha = 0.21f;
  p.flux_lower = 0.063f;
  p.flux_upper = 1804.f;
  smcdet_mh_t mh{};
  mh.num_iters = 10;
  mh.locs_stdev = 0.1f;
  mh.fluxes_stdev = 2.5f;
  float dummy[16] = {0};
  float* d = dummy;
  alignas(8) int32_t ws[4] = {0};

  EXPECT(smcdet_loglik(nullptr, d, d, d, 1, 1, 1, d, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_loglik(&m, nullptr, d, d, 1, 1, 1, d, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_loglik(&m, d, d, d, 0, 1, 1, d, nullptr), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_loglik(&m, d, d, d, 70000, 1, 1, d, nullptr), SMCDET_EUNSUPPORTED);
  smcdet_image_model_t big = m;
  big.H = big.W = 300;
  EXPECT(smcdet_loglik(&big, d, d, d, 1, 1, 1, d, nullptr), SMCDET_EUNSUPPORTED);
  big.H = big.W = 100;
  big.model = SMCDET_MODEL_POISSON;
  EXPECT(smcdet_render(&big, d, d, 1, 1, 1, d, nullptr), SMCDET_EUNSUPPORTED);
  big.model = 7;
  EXPECT(smcdet_psf_dense(&big, d, 1, 1, 1, d, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_sample_image(&m, nullptr, 4, 0, 0, d, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_log_prior(nullptr, d, d, d, 1, 1, 1, nullptr, d, nullptr), SMCDET_EINVAL);
  smcdet_prior_t bp = p;
  bp.max_objects = 2;  // < min
  EXPECT(smcdet_log_prior(&bp, d, d, d, 1, 1, 1, nullptr, d, nullptr), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_prior_sample(&p, 1, 4, 0, 0, d, nullptr, nullptr, d, d, d, nullptr),
         SMCDET_EINVAL);
  // MH sweep: null buffers, S out of range, ancestors with aliased buffers,
  // negative K, zero proposal scale, incomplete replay, large tile without rate_out
  EXPECT(smcdet_mh_sweep(&m, &p, &mh, d, d, 1, 4, 10, nullptr, d, d, d, nullptr, d, d, nullptr,
                         nullptr, 0, 0, nullptr, 0, nullptr, nullptr, ws, nullptr, nullptr,
                         nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_mh_sweep(&m, &p, &mh, d, d, 1, 4, 65, nullptr, d, d, d, nullptr, d, d, nullptr,
                         nullptr, 0, 0, nullptr, 0, nullptr, d, ws, nullptr, nullptr, nullptr),
         SMCDET_EUNSUPPORTED);
  // the accept counter is one uint64 per tile: a misaligned workspace is refused
  EXPECT(smcdet_mh_sweep(&m, &p, &mh, d, d, 1, 4, 10, nullptr, d, d, d, nullptr, d, d, nullptr,
                         nullptr, 0, 0, nullptr, 0, nullptr, d, ws + 1, nullptr, nullptr, nullptr),
         SMCDET_EINVAL);
  int64_t anc[4] = {0, 0, 0, 0};
  EXPECT(smcdet_mh_sweep(&m, &p, &mh, d, d, 1, 4, 10, anc, d, d, d, nullptr, d, d, nullptr,
                         nullptr, 0, 0, nullptr, 0, nullptr, d, ws, nullptr, nullptr, nullptr),
         SMCDET_EINVAL);
  smcdet_mh_t bad = mh;
  bad.num_iters = -1;
  EXPECT(smcdet_mh_sweep(&m, &p, &bad, d, d, 1, 4, 10, nullptr, d, d, d, nullptr, dummy + 8,
                         dummy + 12, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, d, ws, nullptr,
                         nullptr, nullptr), SMCDET_EINVAL);
  bad = mh;
  bad.locs_stdev = 0.f;
  EXPECT(smcdet_mh_sweep(&m, &p, &bad, d, d, 1, 4, 10, nullptr, d, d, d, nullptr, dummy + 8,
                         dummy + 12, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, d, ws, nullptr,
                         nullptr, nullptr), SMCDET_EINVAL);
  smcdet_mh_replay_t rp{};
  rp.comp = nullptr;
  EXPECT(smcdet_mh_sweep(&m, &p, &mh, d, d, 1, 4, 10, nullptr, d, d, d, nullptr, dummy + 8,
                         dummy + 12, nullptr, nullptr, 0, 0, &rp, 0, nullptr, d, ws, nullptr,
                         nullptr, nullptr), SMCDET_EINVAL);
  smcdet_image_model_t g = m;
  g.H = g.W = 128;
  EXPECT(smcdet_mh_sweep(&g, &p, &mh, d, d, 1, 4, 10, nullptr, d, d, d, nullptr, dummy + 8,
                         dummy + 12, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, d, ws, nullptr,
                         nullptr, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_mh_sweep_step(&m, &p, &mh, d, d, 1, 4, 10, nullptr, d, d, d, nullptr, dummy + 8,
                              dummy + 12, nullptr, nullptr, 0, 0, nullptr, 0, d, d, ws, nullptr,
                              nullptr, nullptr, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_mala_sweep(&g, &p, &mh, d, d, 1, 4, 10, nullptr, d, d, d, nullptr, d, d, nullptr,
                           nullptr, 0, 0, nullptr, 0, nullptr, d, ws, nullptr, nullptr),
         SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_temper(nullptr, d, d, 1, 4, 2.0, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_temper(d, d, d, 1, 0, 2.0, nullptr), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_temper(d, d, d, 1, 100000, 2.0, nullptr), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_update_weights(d, d, d, d, d, nullptr, d, 1, 4, nullptr), SMCDET_EINVAL);
  int64_t idx[4];
  EXPECT(smcdet_resample_index(d, 1, 4, 9, 0, 0, nullptr, idx, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_temper_reweight(d, d, d, d, d, d, d, 1, 4, 2.0, 9, 0, 0, idx, 0, nullptr, 0,
                                nullptr, nullptr, nullptr, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_gather(idx, 1, 4, 2, d, d, d, d, d, d, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_prune(nullptr, d, 1, 1, 1, 8.f, 0.25f, idx, d, d, nullptr), SMCDET_EINVAL);
  // catalog matching: null buffers, sizes, tolerances, null index with M != N, limits
  EXPECT(smcdet_match_catalogs(nullptr, d, d, ws, d, d, nullptr, 1, 1, 1, 4, 4, 0.5f, 0.5f, d, 4, d,
                               d, d, d, nullptr, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_match_catalogs(ws, d, d, ws, d, d, nullptr, 1, 1, 1, 4, 4, 0.5f, 0.5f, d, 4, d, d,
                               d, nullptr, nullptr, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_match_catalogs(ws, d, d, ws, d, d, nullptr, 0, 1, 1, 4, 4, 0.5f, 0.5f, d, 4, d, d,
                               d, d, nullptr, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_match_catalogs(ws, d, d, ws, d, d, nullptr, 1, 1, 1, 4, 4, 0.f, 0.5f, d, 4, d, d,
                               d, d, nullptr, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_match_catalogs(ws, d, d, ws, d, d, nullptr, 1, 4, 2, 4, 4, 0.5f, 0.5f, d, 4, d, d,
                               d, d, nullptr, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_match_catalogs(ws, d, d, ws, d, d, nullptr, 1, 1, 1, 65, 4, 0.5f, 0.5f, d, 4, d,
                               d, d, d, nullptr, nullptr), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_match_catalogs(ws, d, d, ws, d, d, nullptr, 1, 1, 1, 4, 65, 0.5f, 0.5f, d, 4, d,
                               d, d, d, nullptr, nullptr), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_match_catalogs(ws, d, d, ws, d, d, nullptr, 1, 1, 1, 4, 4, 0.5f, 0.5f, d, 65, d,
                               d, d, d, nullptr, nullptr), SMCDET_EUNSUPPORTED);
  // condensed catalogs: null buffers, sizes, a bad box, limits (box is a host pointer)
  const float box[4] = {-2.f, -2.f, 10.f, 10.f}, nobox[4] = {0.f, 0.f, 0.f, 8.f};
  EXPECT(smcdet_source_map(nullptr, d, d, nullptr, box, nullptr, 1, 4, 3, 4, 48, 48, d, nullptr, d,
                           nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_source_map(ws, d, d, nullptr, nullptr, nullptr, 1, 4, 3, 4, 48, 48, d, nullptr, d,
                           nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_source_map(ws, d, d, nullptr, nobox, nullptr, 1, 4, 3, 4, 48, 48, d, nullptr, d,
                           nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_source_map(ws, d, d, nullptr, box, nullptr, 1, 0, 3, 4, 48, 48, d, nullptr, d,
                           nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_source_map(ws, d, d, nullptr, box, nullptr, 1, 4, 3, 9, 48, 48, d, nullptr, d,
                           nullptr), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_source_map(ws, d, d, nullptr, box, nullptr, 1, 4, 3, 4, 2049, 48, d, nullptr, d,
                           nullptr), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_source_map(ws, d, d, nullptr, box, nullptr, 1, 1 << 30, 3, 4, 48, 48, d, nullptr,
                           d, nullptr), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_map_peaks(d, box, nullptr, 1, 48, 48, 4, 1, 2, nullptr, 20, ws, ws, d, d, nullptr),
         SMCDET_EINVAL);
  EXPECT(smcdet_map_peaks(d, box, nullptr, 1, 48, 48, 4, 1, 2, d, 0, ws, ws, d, d, nullptr),
         SMCDET_EINVAL);
  EXPECT(smcdet_map_peaks(d, box, nullptr, 1, 48, 48, 4, 1, 2, d, 65, ws, ws, d, d, nullptr),
         SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_map_peaks(d, box, nullptr, 1, 182, 182, 4, 1, 2, d, 20, ws, ws, d, d, nullptr),
         SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_map_peaks(d, box, nullptr, 1, 48, 48, 4, 9, 2, d, 20, ws, ws, d, d, nullptr),
         SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_map_peaks(d, box, nullptr, 1, 48, 48, 4, 1, 17, d, 20, ws, ws, d, d, nullptr),
         SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_seed_moments(ws, d, d, nullptr, d, 1, 4, 3, 20, nullptr, nullptr, nullptr),
         SMCDET_EINVAL);
  EXPECT(smcdet_seed_moments(ws, d, d, nullptr, d, 1, 4, 0, 20, (double*)d, nullptr, nullptr),
         SMCDET_EINVAL);
  EXPECT(smcdet_seed_moments(ws, d, d, nullptr, d, 1, 4, 3, 65, (double*)d, nullptr, nullptr),
         SMCDET_EUNSUPPORTED);
  // posterior-predictive images: every call stops before the launch (the
  // last ones at a workspace one byte short)
  EXPECT(smcdet_posterior_image_workspace(nullptr, 1, 4), SMCDET_EINVAL);
  EXPECT(smcdet_posterior_image_workspace(&m, 0, 4), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_posterior_image_workspace(&m, 70000, 4), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_posterior_image(nullptr, d, d, d, nullptr, 1, 4, 3, 0, 0, d, d, d, d, d, d, 0,
                                nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_posterior_image(&m, d, d, d, nullptr, 1, 4, 3, 0, 0, nullptr, d, d, d, d, d, 0,
                                nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_posterior_image(&m, d, d, d, nullptr, 1, 4, 3, 0, 0, d, d, d, d, d, nullptr, 0,
                                nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_posterior_image(&m, d, nullptr, d, nullptr, 1, 4, 3, 0, 0, d, d, d, d, d, d, 0,
                                nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_posterior_image(&m, nullptr, d, d, nullptr, 1, 4, 3, 0, 0, d, d, d, d, d, d, 0,
                                nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_posterior_image(&m, d, d, d, nullptr, 1, 0, 3, 0, 0, d, d, d, d, d, d, 0,
                                nullptr), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_posterior_image(&m, d, d, d, nullptr, 1, 4, -1, 0, 0, d, d, d, d, d, d, 0,
                                nullptr), SMCDET_EUNSUPPORTED);
  {
    const int64_t need = smcdet_posterior_image_workspace(&m, 3, 257);
    EXPECT(need == 8 * 3 + 16 * 3 * 9 * 1024 ? 0 : 1, 0);
    EXPECT(smcdet_posterior_image(&m, nullptr, nullptr, nullptr, d, 3, 257, 0, 0, 0, d, d, nullptr,
                                  d, d, d, need - 1, nullptr), SMCDET_EINVAL);
  }
  // calibration summaries: limits, sizes, nulls, and the host arrays (cuts, q)
  // the validation reads
  {
    const float cuts[8] = {0.f, 1.f, 2.f, 3.f, 4.f, 5.f, 6.f, __builtin_nanf("")};
    const double q[3] = {0.0, 0.5, 1.5};
    double* dd = (double*)d;
    EXPECT(smcdet_catalog_totals(ws, d, cuts, 1, 4, 3, 9, ws, d, nullptr), SMCDET_EUNSUPPORTED);
    EXPECT(smcdet_catalog_totals(ws, d, cuts, 1, 4, 65, 1, ws, d, nullptr), SMCDET_EUNSUPPORTED);
    EXPECT(smcdet_catalog_totals(ws, d, cuts, 1 << 30, 4, 3, 1, ws, d, nullptr),
           SMCDET_EUNSUPPORTED);
    EXPECT(smcdet_catalog_totals(ws, d, cuts, 0, 4, 3, 1, ws, d, nullptr), SMCDET_EINVAL);
    EXPECT(smcdet_catalog_totals(ws, d, nullptr, 1, 4, 3, 1, ws, d, nullptr), SMCDET_EINVAL);
    EXPECT(smcdet_catalog_totals(ws, d, cuts, 1, 4, 3, 8, ws, d, nullptr), SMCDET_EINVAL);  // NaN
    EXPECT(smcdet_row_summary(d, nullptr, 1, 16385, 1, q, 2, SMCDET_SUMMARY_LINEAR, d, 1, ws, dd,
                              dd, dd, d, d, d, dd, dd, nullptr), SMCDET_EUNSUPPORTED);
    EXPECT(smcdet_row_summary(d, nullptr, 1, 8, 1, q, 65, SMCDET_SUMMARY_LINEAR, d, 1, ws, dd, dd,
                              dd, d, d, d, dd, dd, nullptr), SMCDET_EUNSUPPORTED);
    EXPECT(smcdet_row_summary(d, nullptr, 1, 8, 1, q, 2, SMCDET_SUMMARY_LINEAR, d, 66, ws, dd, dd,
                              dd, d, d, d, dd, dd, nullptr), SMCDET_EUNSUPPORTED);
    EXPECT(smcdet_row_summary(d, nullptr, 1 << 20, 8, 1 << 12, q, 2, SMCDET_SUMMARY_LINEAR, d, 1,
                              ws, dd, dd, dd, d, d, d, dd, dd, nullptr), SMCDET_EUNSUPPORTED);
    EXPECT(smcdet_row_summary(d, d, 1, 8, 1, q, 2, SMCDET_SUMMARY_LINEAR, d, 1, ws, dd, dd, dd, d,
                              d, d, dd, dd, nullptr), SMCDET_EINVAL);  // linear with weights
    EXPECT(smcdet_row_summary(d, nullptr, 1, 8, 1, q, 3, SMCDET_SUMMARY_LOWER, d, 1, ws, dd, dd,
                              dd, d, d, d, dd, dd, nullptr), SMCDET_EINVAL);  // q = 1.5
    EXPECT(smcdet_row_summary(d, nullptr, 1, 8, 1, q, 2, 7, d, 1, ws, dd, dd, dd, d, d, d, dd, dd,
                              nullptr), SMCDET_EINVAL);
    EXPECT(smcdet_row_summary(d, nullptr, 1, 8, 1, q, 2, SMCDET_SUMMARY_LOWER, nullptr, 1, ws, dd,
                              dd, dd, d, d, d, dd, dd, nullptr), SMCDET_EINVAL);
    EXPECT(smcdet_row_summary(d, nullptr, 1, 0, 1, q, 2, SMCDET_SUMMARY_LOWER, d, 1, ws, dd, dd,
                              dd, d, d, d, dd, dd, nullptr), SMCDET_EINVAL);
    EXPECT(smcdet_bootstrap_means(d, 4, 257, nullptr, 0, 2, d, nullptr), SMCDET_EUNSUPPORTED);
    EXPECT(smcdet_bootstrap_means(d, 0, 3, nullptr, 0, 2, d, nullptr), SMCDET_EINVAL);
    EXPECT(smcdet_bootstrap_means(d, 4, 3, nullptr, 0, 2, nullptr, nullptr), SMCDET_EINVAL);
  }
  // convergence diagnostics: limits, sizes, nulls and the workspace requirement
  {
    double* dd = (double*)d;
#define CHAIN_STATS(R, C, M, split, lag, nrho, x, wsp, wsn)                                  \
  smcdet_chain_stats(x, R, C, M, split, lag, nrho, dd, dd, dd, dd, dd, dd, dd, ws, ws, nullptr, \
                     nullptr, d, wsp, wsn, nullptr)
    EXPECT(CHAIN_STATS(1, 33, 16, 1, 7, 0, d, nullptr, 0), SMCDET_EUNSUPPORTED);
    EXPECT(CHAIN_STATS(1, 32, 32770, 1, 7, 0, d, nullptr, 0), SMCDET_EUNSUPPORTED);
    EXPECT(CHAIN_STATS(1, 2, 16, 1, 7, 1025, d, nullptr, 0), SMCDET_EUNSUPPORTED);
    EXPECT(CHAIN_STATS(1 << 26, 32, 16, 1, 7, 0, d, nullptr, 0), SMCDET_EUNSUPPORTED);
    EXPECT(CHAIN_STATS(0, 2, 16, 1, 7, 0, d, nullptr, 0), SMCDET_EINVAL);
    EXPECT(CHAIN_STATS(1, 2, 7, 1, 7, 0, d, nullptr, 0), SMCDET_EINVAL);   // n = 3
    EXPECT(CHAIN_STATS(1, 2, 16, 1, 0, 0, d, nullptr, 0), SMCDET_EINVAL);  // max_lag
    EXPECT(CHAIN_STATS(1, 2, 16, 1, 7, -1, d, nullptr, 0), SMCDET_EINVAL);
    EXPECT(CHAIN_STATS(1, 2, 16, 1, 7, 0, nullptr, nullptr, 0), SMCDET_EINVAL);
    const int64_t cneed = smcdet_chain_stats_workspace(5, 4, 4098, 1);
    EXPECT(cneed == 5 * 16392 ? 0 : 1, 0);
    EXPECT(smcdet_chain_stats_workspace(5, 4, 4096, 1) == 0 ? 0 : 1, 0);
    EXPECT(smcdet_chain_stats_workspace(1, 33, 16, 1), SMCDET_EUNSUPPORTED);
    EXPECT(CHAIN_STATS(5, 4, 4098, 1, 7, 0, d, nullptr, 0), SMCDET_EINVAL);
    EXPECT(CHAIN_STATS(5, 4, 4098, 1, 7, 0, d, d, cneed - 1), SMCDET_EINVAL);
#undef CHAIN_STATS
  }
  // image-model fit: nulls, sizes, psf_radius, a non-finite log_theta (a host
  // array the validation reads), the workspace requirement, the 2^31-1 limits
  {
    double* dd = (double*)d;
    const uint8_t* mk = (const uint8_t*)d;
    double th[SMCDET_FIT_PARAMS] = {0};
    const int64_t fneed = SMCDET_FIT_WORKSPACE_DOUBLES(2, 17, 33);
    EXPECT(fneed == 64 * 7 + 66 * 2 * 2 * 3 ? 0 : 1, 0);
#define FIT(theta, img, lc, fl, F, H, W, D, R, out, wsp, wsn)                                   \
  smcdet_fit_objective(theta, img, mk, lc, fl, ws, F, H, W, D, R, out, dd, dd, nullptr, wsp, wsn, \
                       nullptr)
    EXPECT(FIT(nullptr, d, d, d, 2, 17, 33, 4, 8, dd, dd, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, nullptr, d, d, 2, 17, 33, 4, 8, dd, dd, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, d, nullptr, d, 2, 17, 33, 4, 8, dd, dd, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, d, d, nullptr, 2, 17, 33, 4, 8, dd, dd, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, d, d, d, 2, 17, 33, 4, 8, nullptr, dd, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, d, d, d, 2, 17, 33, 4, 8, dd, nullptr, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, d, d, d, 2, 17, 33, 4, 8, dd, dd, fneed - 1), SMCDET_EINVAL);
    EXPECT(FIT(th, d, d, d, 0, 17, 33, 4, 8, dd, dd, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, d, d, d, 2, 0, 33, 4, 8, dd, dd, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, d, d, d, 2, 17, -3, 4, 8, dd, dd, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, d, d, d, 2, 17, 33, -1, 8, dd, dd, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, d, d, d, 2, 17, 33, 4, -1, dd, dd, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, d, d, d, 2, 17, 33, 4, 65, dd, dd, fneed), SMCDET_EINVAL);
    EXPECT(FIT(th, d, d, d, 3, 32768, 32768, 4, 8, dd, dd, fneed), SMCDET_EUNSUPPORTED);
    EXPECT(FIT(th, d, d, d, 32768, 17, 33, 65536, 8, dd, dd, fneed), SMCDET_EUNSUPPORTED);
    // many tiny fields: more 16x16 blocks than one launch takes
    EXPECT(FIT(th, d, d, d, 1 << 24, 1, 1, 4, 8, dd, dd, fneed), SMCDET_EUNSUPPORTED);
    EXPECT(FIT(th, d, d, d, SMCDET_FIT_MAX_BLOCKS, 1, 1, 4, 8, dd, dd, fneed), SMCDET_EINVAL);
    th[SMCDET_FIT_PARAMS - 1] = __builtin_nan("");
    EXPECT(FIT(th, d, d, d, 2, 17, 33, 4, 8, dd, dd, fneed), SMCDET_EINVAL);
    th[SMCDET_FIT_PARAMS - 1] = -__builtin_inf();
    EXPECT(FIT(th, d, d, d, 2, 17, 33, 4, 8, dd, dd, fneed), SMCDET_EINVAL);
#undef FIT
  }
  EXPECT(smcdet_count_posterior(d, d, 0, 1, 100000, 4, 1, 4, SMCDET_RESAMPLE_SYSTEMATIC, 0, 0,
                                nullptr, nullptr, d, d, d, d, idx, d, d, d, nullptr),
         SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_mh_chain(&m, &p, &mh, d, 1, 1, 10, d, d, d, 100, 200, 1, 0, 10, 0, 0, nullptr, d,
                         d, nullptr, nullptr, nullptr), SMCDET_EINVAL);
  // aggregation: odd joint side, workspace query and requirement
  smcdet_image_model_t j = m;
  j.H = 15;
  EXPECT(smcdet_aggregate_sweep(&j, &p, &mh, 0, d, d, 1, 4, 10, nullptr, d, d, d, nullptr, d, d,
                                0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr), SMCDET_EUNSUPPORTED);
  j.H = 128;
  j.W = 64;
  const int64_t need = smcdet_aggregate_workspace(&j, 1, 4, 24);
  if (need != 4 * (2 * 128 * 64 + 3 * 24)) {
    std::printf("FAIL workspace %lld\n", (long long)need);
    ++fails;
  }
  if (smcdet_aggregate_workspace(&m, 1, 4, 10) != 0) ++fails;
  EXPECT(smcdet_aggregate_workspace(&m, 1, 4, 5000), SMCDET_EUNSUPPORTED);
  EXPECT(smcdet_aggregate_sweep(&j, &p, &mh, 0, d, d, 1, 4, 24, nullptr, d, d, d, nullptr, d, d,
                                0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr), SMCDET_EINVAL);
  EXPECT(smcdet_aggregate_temper(nullptr, d, d, 1, 1, 4, nullptr, nullptr, nullptr, 0.5, d,
                                 nullptr), SMCDET_EINVAL);
  // timing pool: refuse negative, 0 disables, empty reads
  EXPECT(smcdet_launch_timing(-1), SMCDET_EINVAL);
  EXPECT(smcdet_launch_timing(0), SMCDET_OK);
  float ms[2];
  int32_t n = -1;
  EXPECT(smcdet_launch_timing_read(ms, 2, &n), SMCDET_OK);
  EXPECT(smcdet_launch_timing_starts(ms, 2, &n), SMCDET_OK);
  if (n != 0) ++fails;
  EXPECT(smcdet_host_free(nullptr), SMCDET_OK);  // like free(NULL)
  fails += plan_table(m);
  // a diagnostic-only flag is refused before the buffers and the plan
  EXPECT(smcdet_mh_sweep(&m, &p, &mh, nullptr, d, 1, 4, 10, nullptr, d, d, d, nullptr, d, d,
                         nullptr, nullptr, 0, 0, nullptr, SMCDET_MH_SCALAR_SLOTS, nullptr, d, ws,
                         nullptr, nullptr, nullptr), SMCDET_EUNSUPPORTED);
  std::printf("capi sanitizer driver: %d failure(s)\n", fails);
  return fails ? 1 : 0;
}
