// photometry_kernel.hip — forced PSF photometry: positions held fixed, the
// image model given, the fluxes of all sources of a problem solved jointly by
// iteratively reweighted least squares, with their Cramér–Rao errors.  The
// method's definition is in include/smcdet_hip.h (smcdet_forced_photometry);
// the reference has no such code.
//
// One wavefront per problem.  Pixel p sits on lane p % 64 (one per lane up to
// 64 pixels, strided above), and everything a pixel owns -- its weight, its
// data value, its coordinates and the cached weighted column -- is in the
// wave's LDS slab at index p, read and written by that lane only.  A PSF
// column is evaluated in float32 by the render's device functions where it is
// used and is not kept: between the iterations only the weights change, and a
// column costs four hardware transcendentals against 8 bytes of LDS per pixel
// and source.  The normal matrix is packed lower-triangular float64 in the
// slab; each of its entries is one per-lane sum in ascending pixel order and
// one float64 wave reduction.  Nothing is atomic and nothing leaves the slab
// before the outputs, so a problem gives the same bits on every run, in every
// launch and behind every allocation.
#include "render.h"

namespace smcdet {
namespace {

constexpr int kMaxP = SMCDET_PHOT_MAX_SOURCES + 1;  // the sources and the background
constexpr int kPacked = kMaxP * (kMaxP + 1) / 2;    // 561
constexpr int kSmallPix = 64, kSmallWaves = 4;      // H*W <= 64: one pixel per lane
constexpr int kBigPix = SMCDET_EXTRACT_MAX_PIXELS, kBigWaves = 1;
constexpr double kPivotMin = 1e-8;  // smallest squared pivot of a unit-diagonal factor

struct PhotArgs {
  DevModel m;
  const float* images;
  const int32_t* counts;
  const float* locs;
  const float* background;
  double* fluxes;
  double* flux_err;
  double* bg_out;
  double* chi2;
  int32_t* n_pixels;
  int32_t* n_free;
  int32_t* status;
  double* cov;
  double g, na, nm;
  int32_t T, G, K, n_iter, fit_bg;
};

template <int NPIX>
struct Slab {
  double a[kPacked];  // normal matrix / information, then its factor, then the covariance
  double x[kPacked];  // inverse of the information's factor
  double rhs[kMaxP], th[kMaxP], sc[kMaxP];
  float sh[kMaxP], sw[kMaxP];  // the free sources, compacted in slot order
  int sfh[kMaxP], sfw[kMaxP];  // their window anchors
  // per pixel, owned by lane p % 64
  double w[NPIX];   // 1 / v (the information's weight at the end)
  double y[NPIX];   // the data value the linear model is fitted to
  double ci[NPIX];  // column i times the weight, while row i is formed
  int pq[NPIX];     // row << 16 | column
};
static_assert(sizeof(Slab<kSmallPix>) * kSmallWaves <= 65536, "LDS");
static_assert(sizeof(Slab<kBigPix>) * kBigWaves <= 65536, "LDS");

__device__ __forceinline__ unsigned long long ballot(bool p) {
  return __builtin_amdgcn_ballot_w64(p);
}
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }  // i >= j

// g * phi of free parameter i at the pixel pq: the normalised PSF by the
// render's float32 functions and argument (render.h add_source), zero outside
// the (2R+1)^2 window anchored at floor(loc); the background's column is 1
template <int MODEL, int NPIX>
__device__ __forceinline__ double column(const PhotArgs& a, const Slab<NPIX>& s, int i, int ns,
                                         int pq) {
  if (i >= ns) return 1.0;  // wave-uniform
  const DevModel& m = a.m;
  const float h = s.sh[i], w = s.sw[i];
  const int fh = s.sfh[i], fw = s.sfw[i];
  const int ph = pq >> 16, pw = pq & 0xffff;
  const float dh = ((float)ph + 0.5f) - h;
  const float dw = ((float)pw + 0.5f) - w;
  const float phi = psf_raw<MODEL>(m, fmaf(dh, dh, dw * dw)) * psf_scale<MODEL>(m);
  const bool in = (unsigned)(ph - fh + m.R) <= 2u * (unsigned)m.R &&
                  (unsigned)(pw - fw + m.R) <= 2u * (unsigned)m.R;
  return in ? a.g * (double)phi : 0.0;
}

// a = D^T diag(w) D over the P free parameters (packed lower triangle) and,
// with RHS, rhs = D^T diag(w) y
template <int MODEL, int NPIX, bool RHS>
__device__ __forceinline__ void normal_equations(const PhotArgs& a, Slab<NPIX>& s, int P, int ns,
                                                 int HW, int lane) {
  constexpr int PPL = NPIX / 64;
  for (int i = 0; i < P; ++i) {
    double racc = 0.0;
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      if (p < HW) {
        const double ci = column<MODEL>(a, s, i, ns, s.pq[p]) * s.w[p];
        s.ci[p] = ci;
        if (RHS) racc += ci * s.y[p];
      }
    }
    if (RHS) {
      racc = wave_sum(racc);
      if (lane == 0) s.rhs[i] = racc;
    }
    for (int j = 0; j <= i; ++j) {
      double acc = 0.0;
#pragma unroll 1
      for (int c = 0; c < PPL; ++c) {
        const int p = lane + 64 * c;
        if (p < HW) acc += s.ci[p] * column<MODEL>(a, s, j, ns, s.pq[p]);
      }
      acc = wave_sum(acc);
      if (lane == 0) s.a[tri(i, j)] = acc;
    }
  }
  wave_sync();
}

// a <- S a S with S = diag(sc), sc_i = 1 / sqrt(a_ii): a unit diagonal
__device__ __forceinline__ void scale_unit_diagonal(double* a, double* sc, int P, int lane) {
  if (lane < P) sc[lane] = 1.0 / sqrt(a[tri(lane, lane)]);
  wave_sync();
  if (lane < P) {
    const double si = sc[lane];
    for (int j = 0; j <= lane; ++j) a[tri(lane, j)] *= si * sc[j];
  }
  wave_sync();
}

// in-place Cholesky factor of the packed matrix, row i on lane i; false (and
// an unfinished factor) when a squared pivot is below kPivotMin or not a number
__device__ __forceinline__ bool cholesky(double* a, int P, int lane) {
  for (int j = 0; j < P; ++j) {
    const double d = a[tri(j, j)];
    if (ballot(!(d >= kPivotMin))) return false;
    const double l = sqrt(d);
    const bool below = lane > j && lane < P;
    double lij = 0.0;
    if (below) {
      lij = a[tri(lane, j)] / l;
      a[tri(lane, j)] = lij;
    }
    wave_sync();
    if (lane == j) a[tri(j, j)] = l;
    if (below)
      for (int k = j + 1; k <= lane; ++k) a[tri(lane, k)] -= lij * a[tri(k, j)];
    wave_sync();
  }
  return true;
}

// th <- (L L^T)^-1 th, L the packed factor
__device__ __forceinline__ void cholesky_solve(const double* L, double* th, int P, int lane) {
  for (int j = 0; j < P; ++j) {
    const double z = th[j] / L[tri(j, j)];
    wave_sync();
    if (lane == j) th[j] = z;
    if (lane > j && lane < P) th[lane] -= L[tri(lane, j)] * z;
    wave_sync();
  }
  for (int j = P - 1; j >= 0; --j) {
    const double z = th[j] / L[tri(j, j)];
    wave_sync();
    if (lane == j) th[j] = z;
    if (lane < j) th[lane] -= L[tri(j, lane)] * z;
    wave_sync();
  }
}

template <int MODEL, int NPIX, int WAVES>
__global__ __launch_bounds__(WAVES* kWave) void photometry_kernel(PhotArgs a) {
  constexpr int PPL = NPIX / 64;
  __shared__ Slab<NPIX> slabs[WAVES];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t prob = (int64_t)blockIdx.x * WAVES + wv;  // g fastest: neighbours share the image
  if (prob >= (int64_t)a.T * a.G) return;  // wave-uniform; there is no workgroup barrier below
  Slab<NPIX>& s = slabs[wv];
  const int t = (int)(prob / a.G);
  const int W = a.m.W, HW = a.m.H * a.m.W, K = a.K;
  const bool fit = a.fit_bg != 0;

  const double B = a.background ? (double)a.background[t] : (double)a.m.bg;
  const bool bad_bg = !(B > 0.0) || !(B < INFINITY);
  const double lam_floor = 0.25 * B;
  const double B_fixed = fit ? 0.0 : B;  // the part of the rate that is not D theta

  // ---- the pixels: coordinates, data, initial weights -------------------------
  const float* img = a.images + (int64_t)t * HW;
#pragma unroll 1
  for (int c = 0; c < PPL; ++c) {
    const int p = lane + 64 * c;
    if (p < HW) {
      const int i = p / W;
      const double x = (double)img[p];
      s.pq[p] = (i << 16) | (p - i * W);
      s.y[p] = x - B_fixed;
      s.w[p] = 1.0 / (a.na + a.nm * fmax(x, lam_floor));
    }
  }

  // ---- the slots: skipped, dropped or free --------------------------------------
  const int cnt = min(max(a.counts[prob], 0), K);
  float h = NAN, w = NAN;
  if (lane < cnt) {
    const float* l = a.locs + 2 * (prob * K + lane);  // (4-byte aligned: a view may start anywhere)
    h = l[0];
    w = l[1];
  }
  const bool cand = lane < cnt && isfinite(h) && isfinite(w);
  const int fh = ifloor_clamped(h), fw = ifloor_clamped(w);
  const unsigned long long cand_mask = ballot(cand);
  unsigned long long free_mask = 0;
  int ns = 0;
  for (int k = 0; k < cnt; ++k) {
    if (!((cand_mask >> k) & 1)) continue;  // wave-uniform
    const float hk = readlane(h, k), wk = readlane(w, k);
    const int fhk = readlane(fh, k), fwk = readlane(fw, k);
    if (lane == 0) {
      s.sh[ns] = hk;
      s.sw[ns] = wk;
      s.sfh[ns] = fhk;
      s.sfw[ns] = fwk;
    }
    wave_sync();
    bool any = false;
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      if (p < HW) any |= column<MODEL>(a, s, ns, ns + 1, s.pq[p]) != 0.0;
    }
    if (ballot(any)) {  // else: the next free source takes this place
      free_mask |= 1ull << k;
      ++ns;
    }
    wave_sync();
  }
  const bool is_free = (free_mask >> lane) & 1;
  const bool dropped = cand && !is_free;
  const int pidx = __builtin_popcountll(free_mask & ((1ull << lane) - 1));
  const int P = ns + (fit ? 1 : 0);
  int status = (ballot(dropped) ? 1 : 0) | (bad_bg ? 4 : 0);
  bool failed = bad_bg;

  // ---- the reweighted solve -------------------------------------------------------
  double chi = 0.0;
  for (int it = 0; it < a.n_iter && !failed; ++it) {
    normal_equations<MODEL, NPIX, true>(a, s, P, ns, HW, lane);
    scale_unit_diagonal(s.a, s.sc, P, lane);
    if (!cholesky(s.a, P, lane)) {
      failed = true;
      status |= 2;
      break;
    }
    if (lane < P) s.th[lane] = s.rhs[lane] * s.sc[lane];
    wave_sync();
    cholesky_solve(s.a, s.th, P, lane);
    if (lane < P) s.th[lane] *= s.sc[lane];
    wave_sync();
    chi = 0.0;
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      if (p < HW) {
        double lin = 0.0;
        for (int i = 0; i < P; ++i) lin += column<MODEL>(a, s, i, ns, s.pq[p]) * s.th[i];
        const double wp = 1.0 / (a.na + a.nm * fmax(lin + B_fixed, lam_floor));
        const double r = s.y[p] - lin;
        s.w[p] = wp;
        chi += r * r * wp;
      }
    }
  }
  chi = wave_sum(chi);

  // ---- the Cramér–Rao bound at the final theta and v ---------------------------------
  if (!failed) {
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      if (p < HW) {
        const double wp = s.w[p];
        s.w[p] = wp + 0.5 * a.nm * a.nm * wp * wp;
      }
    }
    normal_equations<MODEL, NPIX, false>(a, s, P, ns, HW, lane);
    scale_unit_diagonal(s.a, s.sc, P, lane);
    if (!cholesky(s.a, P, lane)) {
      failed = true;
      status |= 2;
    }
  }
  if (!failed) {
    // x = L^-1, column m on lane m; then cov = S x^T x S, row i on lane i, into a
    if (lane < P) {
      const int mcol = lane;
      s.x[tri(mcol, mcol)] = 1.0 / s.a[tri(mcol, mcol)];
      for (int i = mcol + 1; i < P; ++i) {
        double sum = 0.0;
        for (int k = mcol; k < i; ++k) sum += s.a[tri(i, k)] * s.x[tri(k, mcol)];
        s.x[tri(i, mcol)] = -sum / s.a[tri(i, i)];
      }
    }
    wave_sync();
    if (lane < P) {
      const int i = lane;
      for (int j = 0; j <= i; ++j) {
        double sum = 0.0;
        for (int k = i; k < P; ++k) sum += s.x[tri(k, i)] * s.x[tri(k, j)];
        s.a[tri(i, j)] = sum * s.sc[i] * s.sc[j];
      }
    }
    wave_sync();
  }

  // ---- outputs ----------------------------------------------------------------------------
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (lane < K) {
    double f = 0.0, e = nan;  // a skipped slot
    if (cand) {
      f = nan;
      if (is_free && !failed) {
        f = s.th[pidx];
        e = sqrt(s.a[tri(pidx, pidx)]);
      }
    }
    a.fluxes[prob * K + lane] = f;
    a.flux_err[prob * K + lane] = e;
  }
  if (lane == 0) {
    a.bg_out[prob] = failed ? nan : (fit ? s.th[ns] : B);
    a.chi2[prob] = failed ? nan : chi;
    a.n_pixels[prob] = HW;
    a.n_free[prob] = P;
    a.status[prob] = status;
  }
  if (a.cov) {
    double* cov = a.cov + prob * K * K;
    for (int q = lane; q < K * K; q += 64) {
      const int r = q / K, c = q - r * K;
      const bool ok = !failed && ((free_mask >> r) & 1) && ((free_mask >> c) & 1);
      double v = nan;
      if (ok) {
        const int ir = __builtin_popcountll(free_mask & ((1ull << r) - 1));
        const int ic = __builtin_popcountll(free_mask & ((1ull << c) - 1));
        v = s.a[tri(max(ir, ic), min(ir, ic))];
      }
      cov[q] = v;
    }
  }
}

template <int MODEL>
void launch(const PhotArgs& a, int64_t probs, hipStream_t st) {
  if (a.m.H * a.m.W <= kSmallPix) {
    const int64_t blocks = (probs + kSmallWaves - 1) / kSmallWaves;
    launch_sweep(photometry_kernel<MODEL, kSmallPix, kSmallWaves>, dim3((unsigned)blocks),
                 dim3(kSmallWaves * kWave), 0, st, a);
  } else {
    launch_sweep(photometry_kernel<MODEL, kBigPix, kBigWaves>, dim3((unsigned)probs),
                 dim3(kBigWaves * kWave), 0, st, a);
  }
}

}  // namespace
}  // namespace smcdet

extern "C" {

int smcdet_forced_photometry(const smcdet_image_model_t* model, const float* images,
                             const int32_t* counts, const float* locs, const float* background,
                             int32_t T, int32_t G, int32_t K, int32_t n_iter, uint32_t flags,
                             double* fluxes, double* flux_err, double* background_out,
                             double* chi2, int32_t* n_pixels, int32_t* n_free, int32_t* status,
                             double* cov, void* stream) {
  using namespace smcdet;
  if (int rc = validate_model(model, SMCDET_EXTRACT_MAX_PIXELS)) return rc;
  if (T < 1 || G < 1 || K < 1)
    return set_error(SMCDET_EINVAL, "forced_photometry: T=%d G=%d K=%d must be >= 1", T, G, K);
  if (K > SMCDET_PHOT_MAX_SOURCES)
    return set_error(SMCDET_EUNSUPPORTED, "forced_photometry: K=%d above %d", K,
                     SMCDET_PHOT_MAX_SOURCES);
  const int64_t probs = (int64_t)T * G;
  if (probs > 0x7fffffffll)
    return set_error(SMCDET_EUNSUPPORTED, "forced_photometry: T*G = %lld problems exceed the grid",
                     (long long)probs);
  if (n_iter < 1 || n_iter > SMCDET_PHOT_MAX_ITER)
    return set_error(SMCDET_EINVAL, "forced_photometry: n_iter=%d outside 1..%d", n_iter,
                     SMCDET_PHOT_MAX_ITER);
  if (flags & ~SMCDET_PHOT_FIT_BACKGROUND)
    return set_error(SMCDET_EINVAL, "forced_photometry: unknown flags 0x%x", flags);
  if (!images || !counts || !locs || !fluxes || !flux_err || !background_out || !chi2 ||
      !n_pixels || !n_free || !status)
    return set_error(SMCDET_EINVAL, "forced_photometry: null buffer");
  if (!background && !(model->background > 0.f && model->background < INFINITY))
    return set_error(SMCDET_EINVAL, "forced_photometry: the model's background %g is not "
                     "positive and finite", (double)model->background);
  PhotArgs a{};
  a.m = make_dev_model(*model);
  const bool m71 = model->model == SMCDET_MODEL_M71;
  a.g = (double)a.m.g;
  a.na = m71 ? (double)model->noise_additive : 0.0;
  a.nm = m71 ? (double)model->noise_multiplicative : 1.0;
  if (!(a.na >= 0.0) || !(a.nm >= 0.0) || !(a.na + a.nm > 0.0) || !(a.na + a.nm < INFINITY))
    return set_error(SMCDET_EINVAL, "forced_photometry: noise_additive=%g and "
                     "noise_multiplicative=%g do not give a positive variance", a.na, a.nm);
  if (!(a.g > 0.0) || !(a.g < INFINITY))
    return set_error(SMCDET_EINVAL, "forced_photometry: adu_per_nmgy=%g is not positive and "
                     "finite", a.g);
  a.images = images;
  a.counts = counts;
  a.locs = locs;
  a.background = background;
  a.fluxes = fluxes;
  a.flux_err = flux_err;
  a.bg_out = background_out;
  a.chi2 = chi2;
  a.n_pixels = n_pixels;
  a.n_free = n_free;
  a.status = status;
  a.cov = cov;
  a.T = T;
  a.G = G;
  a.K = K;
  a.n_iter = n_iter;
  a.fit_bg = (flags & SMCDET_PHOT_FIT_BACKGROUND) ? 1 : 0;
  if (m71)
    launch<SMCDET_MODEL_M71>(a, probs, (hipStream_t)stream);
  else
    launch<SMCDET_MODEL_POISSON>(a, probs, (hipStream_t)stream);
  return check_launch("smcdet_forced_photometry");
}

}  // extern "C"
