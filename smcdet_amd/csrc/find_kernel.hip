// find_kernel.hip — the PSF-fitting detector's two device steps: the
// significance map of an image's residual with its peaks (smcdet_psf_find),
// and one Jacobi sweep of leave-one-out position moves (smcdet_psf_recentre).
// The method's definition is in include/smcdet_hip.h; the reference has no
// such code.
//
// Both kernels keep, per pixel and in LDS, the residual r and the weight 1/v
// as float64.  A candidate's profile is evaluated where it is used, by the
// render's float32 device functions with the render's argument (render.h
// add_source), over its clipped window in ascending pixel order, widened, and
// folded into a = sum phi r / v and d = sum phi^2 / v by float64 fma: one
// thread owns one candidate, so every sum has one fixed order.  No table of the
// profile is kept: a cell centre (i + 1/2)/c is not base + phase in float32 for
// c = 3, and the fitted model has to stay the samplers' and the photometry's
// bit for bit.  Nothing is atomic (the peak bits are wave ballots), so a
// problem gives the same bits on every run and among any neighbours.
#include "render.h"

namespace smcdet {
namespace {

constexpr int kFindThreads = 256;
constexpr int kMaxK = SMCDET_PHOT_MAX_SOURCES;
constexpr int kMaxCand = 49;  // (2 * 3 + 1)^2 candidates of a move

struct FindArgs {
  DevModel m;
  const float* images;
  const float* background;
  const int32_t* counts;
  const float* locs;
  const float* fluxes;
  const float* thresh;
  const int32_t* nms;
  int32_t* counts_out;
  float* locs_out;
  float* snr_out;
  float* flux_hat;
  int32_t* n_found;
  float* map_out;
  double g, na, nm, min_sep;
  int32_t T, G, K, c, cH, cW;
};

struct MoveArgs {
  DevModel m;
  const float* images;
  const float* background;
  const int32_t* counts;
  const float* locs;
  const float* fluxes;
  float* locs_out;
  float* snr_out;
  double g, na, nm, step;
  int32_t T, G, K, half;
};

__device__ __forceinline__ unsigned long long ballot64(bool p) {
  return __builtin_amdgcn_ballot_w64(p);
}

__device__ __forceinline__ unsigned long long wave_max_key(unsigned long long v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned long long o = __shfl_xor(v, m, 64);
    v = o > v ? o : v;
  }
  return v;
}

// the float's bits as an unsigned integer of the same order (-0 as +0)
__device__ __forceinline__ uint32_t ordered_bits(float v) {
  const uint32_t b = (uint32_t)__float_as_int(v + 0.0f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the render's float32 profile of a source at (h, w) at the pixel (ph, pw)
template <int MODEL>
__device__ __forceinline__ float profile_at(const DevModel& m, float h, float w, int ph, int pw) {
  const float dh = ((float)ph + 0.5f) - h;
  const float dw = ((float)pw + 0.5f) - w;
  return psf_raw<MODEL>(m, fmaf(dh, dh, dw * dw)) * psf_scale<MODEL>(m);
}

// the same, zero outside the (2R+1)^2 window anchored at floor(loc)
template <int MODEL>
__device__ __forceinline__ double column_at(const DevModel& m, float h, float w, int ph, int pw) {
  const int fh = ifloor_clamped(h), fw = ifloor_clamped(w);
  const bool in = (unsigned)(ph - fh + m.R) <= 2u * (unsigned)m.R &&
                  (unsigned)(pw - fw + m.R) <= 2u * (unsigned)m.R;
  return in ? (double)profile_at<MODEL>(m, h, w, ph, pw) : 0.0;
}

// a = sum phi_c r / v and d = sum phi_c^2 / v of the candidate at (h, w) over
// its clipped window, pixels ascending; with BACK, r has g f phi of the
// source at (bh, bw) put back (gf = g f)
template <int MODEL, bool BACK>
__device__ __forceinline__ void correlate(const DevModel& m, const double* r, const double* iw,
                                          float h, float w, float bh, float bw, double gf,
                                          double& a_out, double& d_out) {
  const int fh = ifloor_clamped(h), fw = ifloor_clamped(w);
  const int r0 = max(fh - m.R, 0), r1 = min(fh + m.R, m.H - 1);
  const int c0 = max(fw - m.R, 0), c1 = min(fw + m.R, m.W - 1);
  double a = 0.0, d = 0.0;
  for (int ph = r0; ph <= r1; ++ph)
    for (int pw = c0; pw <= c1; ++pw) {
      const int p = ph * m.W + pw;
      const double phi = (double)profile_at<MODEL>(m, h, w, ph, pw);
      const double wp = iw[p];
      double rp = r[p];
      if (BACK) rp = fma(gf, column_at<MODEL>(m, bh, bw, ph, pw), rp);
      a = fma(phi, rp * wp, a);
      d = fma(phi, phi * wp, d);
    }
  a_out = a;
  d_out = d;
}

__device__ __forceinline__ float snr_of(double a, double d) {
  return d == 0.0 ? -INFINITY : (float)(a / sqrt(d));
}

// the parabola through (-1, sm), (0, s0), (1, sp): its vertex clamped to
// +-1/2, or 0 where a neighbour is missing or the three points are not concave
__device__ __forceinline__ double vertex(bool both, float sm, float s0, float sp) {
  if (!both) return 0.0;
  const double den = ((double)sm - 2.0 * (double)s0) + (double)sp;
  if (!(den < 0.0)) return 0.0;
  const double dl = 0.5 * ((double)sm - (double)sp) / den;
  return fmin(fmax(dl, -0.5), 0.5);
}

// r_p = x_p - B - g sum_k f_k phi_pk over the ns listed sources, slot order, and
// 1 / v_p with v_p = na + nm max(x_p, B / 4), for the pixels tid, tid + n, ...
template <int MODEL>
__device__ __forceinline__ void residual(const DevModel& m, const float* img, double B,
                                         bool bad_bg, double g, double na, double nm,
                                         const float* sh, const float* sw, const float* sf, int ns,
                                         double* r, double* iw, int tid, int nthreads) {
  const int HW = m.H * m.W;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int p = tid; p < HW; p += nthreads) {
    const int ph = p / m.W, pw = p - ph * m.W;
    const double x = (double)img[p];
    double acc = 0.0;
    for (int k = 0; k < ns; ++k)
      acc = fma((double)sf[k], column_at<MODEL>(m, sh[k], sw[k], ph, pw), acc);
    r[p] = (x - B) - g * acc;
    iw[p] = bad_bg ? nan : 1.0 / (na + nm * fmax(x, 0.25 * B));
  }
}

// LDS of psf_find_kernel: r and 1/v [HW] float64, 4 u64 of the reductions, the
// listed sources (h, w, f) [32] float each, the chosen cells [32] int32, the
// map [cells] float, the peak bits [ceil(cells / 32)] u32
constexpr size_t find_lds_bytes(int HW, int cells) {
  return (size_t)HW * 16 + 32 + 4 * kMaxK * 4 + (size_t)cells * 4 + (size_t)((cells + 31) / 32) * 4;
}

template <int MODEL>
__global__ __launch_bounds__(kFindThreads) void psf_find_kernel(FindArgs a) {
  extern __shared__ double find_lds[];
  const DevModel& m = a.m;
  const int HW = m.H * m.W, cells = a.cH * a.cW, words = (cells + 31) / 32, K = a.K;
  double* r = find_lds;
  double* iw = r + HW;
  unsigned long long* red = reinterpret_cast<unsigned long long*>(iw + HW);
  float* sh = reinterpret_cast<float*>(red + 4);
  float* sw = sh + kMaxK;
  float* sf = sw + kMaxK;
  int32_t* chosen = reinterpret_cast<int32_t*>(sf + kMaxK);
  float* s = reinterpret_cast<float*>(chosen + kMaxK);
  uint32_t* bits = reinterpret_cast<uint32_t*>(s + cells);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t prob = blockIdx.x;  // g fastest: neighbours share the image
  const int t = (int)(prob / a.G), gi = (int)(prob - (int64_t)t * a.G);

  const double B = a.background ? (double)a.background[t] : (double)m.bg;
  const bool bad_bg = !(B > 0.0) || !(B < INFINITY);
  const int n = a.counts ? min(max(a.counts[prob], 0), K) : 0;

  // ---- the listed sources that count, compacted in slot order (wave 0) ------------
  int ns = 0;
  if (wv == 0) {
    float h = NAN, w = NAN, f = NAN;
    if (lane < n) {
      h = a.locs[2 * (prob * K + lane)];
      w = a.locs[2 * (prob * K + lane) + 1];
      f = a.fluxes[prob * K + lane];
    }
    const bool counted = lane < n && isfinite(h) && isfinite(w) && isfinite(f);
    const unsigned long long mask = ballot64(counted);
    if (counted) {
      const int i = __builtin_popcountll(mask & ((1ull << lane) - 1));
      sh[i] = h;
      sw[i] = w;
      sf[i] = f;
    }
    if (lane == 0) red[0] = (unsigned long long)__builtin_popcountll(mask);
  }
  __syncthreads();
  ns = (int)red[0];

  residual<MODEL>(m, a.images + (int64_t)t * HW, B, bad_bg, a.g, a.na, a.nm, sh, sw, sf, ns, r, iw,
                  tid, kFindThreads);
  __syncthreads();

  // ---- the map: one thread per cell ----------------------------------------------------
  for (int x = tid; x < cells; x += kFindThreads) {
    const int i = x / a.cW, j = x - i * a.cW;
    const float h = (float)(((double)i + 0.5) / (double)a.c);
    const float w = (float)(((double)j + 0.5) / (double)a.c);
    double ca, cd;
    correlate<MODEL, false>(m, r, iw, h, w, 0.f, 0.f, 0.0, ca, cd);
    const float v = snr_of(ca, cd);
    s[x] = v;
    if (a.map_out) a.map_out[prob * cells + x] = v;
  }
  __syncthreads();

  // ---- the peaks: threshold, suppression, exclusion; bits by wave ballot ----------------
  const float thresh = a.thresh[gi];
  const int q = min(max(a.nms[gi], 0), 16);
  int found = 0;  // wave-uniform: the peaks of this wave's cells
  for (int base = 0; base < cells; base += kFindThreads) {
    const int x = base + tid;
    bool peak = false;
    if (x < cells) {
      const float v = s[x];
      peak = v >= thresh;
      if (peak) {
        const int i = x / a.cW, j = x - i * a.cW;
        const int i0 = max(i - q, 0), i1 = min(i + q, a.cH - 1);
        const int j0 = max(j - q, 0), j1 = min(j + q, a.cW - 1);
        for (int ii = i0; ii <= i1 && peak; ++ii)
          for (int jj = j0; jj <= j1; ++jj) {
            const int y = ii * a.cW + jj;
            const float u = s[y];
            if (y != x && !(v > u || (v == u && x < y))) peak = false;
          }
        const double ch = ((double)i + 0.5) / (double)a.c, cw = ((double)j + 0.5) / (double)a.c;
        for (int k = 0; k < ns; ++k)
          if (!(fmax(fabs(ch - (double)sh[k]), fabs(cw - (double)sw[k])) > a.min_sep))
            peak = false;
      }
    }
    const unsigned long long mask = ballot64(peak);
    found += __builtin_popcountll(mask);
    const int w0 = (base + 64 * wv) >> 5;
    if (lane == 0) {
      if (w0 < words) bits[w0] = (uint32_t)mask;
      if (w0 + 1 < words) bits[w0 + 1] = (uint32_t)(mask >> 32);
    }
  }
  if (lane == 0) red[wv] = (unsigned long long)found;
  __syncthreads();
  const int n_found = (int)(red[0] + red[1] + red[2] + red[3]);
  int n_new = min(n_found, K - n);
  __syncthreads();

  // ---- the first n_new by (snr descending, index ascending): one arg-max each ------------
  for (int o = 0; o < n_new; ++o) {  // block-uniform
    unsigned long long best = 0;
    for (int w = tid; w < words; w += kFindThreads)
      for (uint32_t mk = bits[w]; mk; mk &= mk - 1) {
        const uint32_t x = (uint32_t)w * 32u + (uint32_t)__builtin_ctz(mk);
        const unsigned long long key =
            ((unsigned long long)ordered_bits(s[x]) << 32) | (0xffffffffu - x);
        best = key > best ? key : best;
      }
    best = wave_max_key(best);
    if (lane == 0) red[wv] = best;
    __syncthreads();
    best = red[0];
    for (int w = 1; w < kFindThreads / 64; ++w) best = red[w] > best ? red[w] : best;
    if (best == 0) {  // block-uniform; no peak bit is left (cannot happen: n_new <= n_found)
      n_new = o;
      break;
    }
    const uint32_t x = 0xffffffffu - (uint32_t)(best & 0xffffffffull);
    if (tid == 0) {
      chosen[o] = (int32_t)x;
      bits[x >> 5] &= ~(1u << (x & 31));
    }
    __syncthreads();
  }

  // ---- outputs: the given slots bit for bit, the new ones refined, NaN past them ---------
  if (tid < K) {
    const int64_t o = prob * K + tid;
    float lh = NAN, lw = NAN, snr = NAN, fhat = NAN;
    if (tid < n) {
      lh = a.locs[2 * o];
      lw = a.locs[2 * o + 1];
    } else if (tid - n < n_new) {
      const int x = chosen[tid - n];
      const int i = x / a.cW, j = x - i * a.cW;
      const float s0 = s[x];
      const bool bi = i > 0 && i < a.cH - 1, bj = j > 0 && j < a.cW - 1;
      const double di = vertex(bi, bi ? s[x - a.cW] : 0.f, s0, bi ? s[x + a.cW] : 0.f);
      const double dj = vertex(bj, bj ? s[x - 1] : 0.f, s0, bj ? s[x + 1] : 0.f);
      lh = (float)((((double)i + 0.5) + di) / (double)a.c);
      lw = (float)((((double)j + 0.5) + dj) / (double)a.c);
      const float h = (float)(((double)i + 0.5) / (double)a.c);
      const float w = (float)(((double)j + 0.5) / (double)a.c);
      double ca, cd;
      correlate<MODEL, false>(m, r, iw, h, w, 0.f, 0.f, 0.0, ca, cd);
      snr = s0;
      fhat = (float)(ca / (a.g * cd));
    }
    if (tid < n) {  // (as integers: a NaN's payload is kept)
      const int32_t* li = reinterpret_cast<const int32_t*>(a.locs);
      int32_t* lo = reinterpret_cast<int32_t*>(a.locs_out);
      lo[2 * o] = li[2 * o];
      lo[2 * o + 1] = li[2 * o + 1];
    } else {
      a.locs_out[2 * o] = lh;
      a.locs_out[2 * o + 1] = lw;
    }
    a.snr_out[o] = snr;
    a.flux_hat[o] = fhat;
  }
  if (tid == 0) {
    a.counts_out[prob] = n + n_new;
    a.n_found[prob] = n_found;
  }
}

// LDS of psf_recentre_kernel: r and 1/v [HW] float64, the counted sources
// (h, w, f) [32] float each, the candidates' snr [32 * 49] float
constexpr size_t move_lds_bytes(int HW, int ns_max, int ncand) {
  return (size_t)HW * 16 + 3 * kMaxK * 4 + (size_t)ns_max * ncand * 4;
}

// One wavefront per problem: pixel p of the residual on lane p % 64, then one
// (source, candidate) pair per lane -- a tile's few sources times 25 candidates
// fill one or two passes -- then source k's arg-max and parabola on lane k.
// Only wave barriers; nothing is shared between problems.
template <int MODEL>
__global__ __launch_bounds__(kWave) void psf_recentre_kernel(MoveArgs a) {
  extern __shared__ double move_lds[];
  const DevModel& m = a.m;
  const int HW = m.H * m.W, K = a.K;
  const int side = 2 * a.half + 1, nc = side * side;
  double* r = move_lds;
  double* iw = r + HW;
  float* sh = reinterpret_cast<float*>(iw + HW);
  float* sw = sh + kMaxK;
  float* sf = sw + kMaxK;
  float* cs = sf + kMaxK;
  const int lane = threadIdx.x;
  const int64_t prob = blockIdx.x;
  const int t = (int)(prob / a.G);

  const double B = a.background ? (double)a.background[t] : (double)m.bg;
  const bool bad_bg = !(B > 0.0) || !(B < INFINITY);
  const int n = min(max(a.counts[prob], 0), K);

  float h = NAN, w = NAN, f = NAN;
  if (lane < K) {
    h = a.locs[2 * (prob * K + lane)];
    w = a.locs[2 * (prob * K + lane) + 1];
    f = a.fluxes[prob * K + lane];
  }
  const bool counted = lane < n && isfinite(h) && isfinite(w) && isfinite(f);
  const unsigned long long mask = ballot64(counted);
  const int ns = __builtin_popcountll(mask);
  const int me = __builtin_popcountll(mask & ((1ull << lane) - 1));
  if (counted) {
    sh[me] = h;
    sw[me] = w;
    sf[me] = f;
  }
  wave_sync();
  residual<MODEL>(m, a.images + (int64_t)t * HW, B, bad_bg, a.g, a.na, a.nm, sh, sw, sf, ns, r, iw,
                  lane, kWave);
  wave_sync();

  // ---- the leave-one-out snr of every candidate of every counted source ------------------
  for (int q = lane; q < ns * nc; q += kWave) {
    const int k = q / nc, cand = q - k * nc;
    const int oa = cand / side - a.half, ob = cand - (cand / side) * side - a.half;
    const float ch = (float)((double)sh[k] + (double)oa * a.step);
    const float cw = (float)((double)sw[k] + (double)ob * a.step);
    double ca, cd;
    correlate<MODEL, true>(m, r, iw, ch, cw, sh[k], sw[k], a.g * (double)sf[k], ca, cd);
    cs[q] = snr_of(ca, cd);
  }
  wave_sync();

  // ---- the move of source k on the lane that holds its slot ------------------------------
  float oh = h, ow = w, snr = NAN;
  if (counted) {
    const float* c = cs + me * nc;
    int best = 0;
    float vb = c[0];
    for (int i = 1; i < nc; ++i)
      if (c[i] > vb) {
        vb = c[i];
        best = i;
      }
    const int ia = best / side, ib = best - ia * side;
    const bool ba = ia > 0 && ia < side - 1, bb = ib > 0 && ib < side - 1;
    const double da = vertex(ba, ba ? c[best - side] : 0.f, vb, ba ? c[best + side] : 0.f);
    const double db = vertex(bb, bb ? c[best - 1] : 0.f, vb, bb ? c[best + 1] : 0.f);
    oh = (float)((double)h + ((double)(ia - a.half) + da) * a.step);
    ow = (float)((double)w + ((double)(ib - a.half) + db) * a.step);
    snr = vb;
  }
  if (lane < K) {
    const int64_t o = prob * K + lane;
    if (counted) {
      a.locs_out[2 * o] = oh;
      a.locs_out[2 * o + 1] = ow;
    } else {  // (as integers: a NaN's payload is kept)
      const int32_t* li = reinterpret_cast<const int32_t*>(a.locs);
      int32_t* lo = reinterpret_cast<int32_t*>(a.locs_out);
      lo[2 * o] = li[2 * o];
      lo[2 * o + 1] = li[2 * o + 1];
    }
    a.snr_out[o] = snr;
  }
}

// the checks the two entry points share; fills the noise model
int check_common(const char* who, const smcdet_image_model_t* model, int32_t T, int32_t G,
                 int32_t K, const float* background, double& g, double& na, double& nm,
                 DevModel& dm) {
  if (int rc = validate_model(model, SMCDET_EXTRACT_MAX_PIXELS)) return rc;
  if (T < 1 || G < 1 || K < 1)
    return set_error(SMCDET_EINVAL, "%s: T=%d G=%d K=%d must be >= 1", who, T, G, K);
  if (K > SMCDET_PHOT_MAX_SOURCES)
    return set_error(SMCDET_EUNSUPPORTED, "%s: K=%d above %d", who, K, SMCDET_PHOT_MAX_SOURCES);
  if ((int64_t)T * G > 0x7fffffffll)
    return set_error(SMCDET_EUNSUPPORTED, "%s: T*G = %lld problems exceed the grid", who,
                     (long long)T * G);
  if (!background && !(model->background > 0.f && model->background < INFINITY))
    return set_error(SMCDET_EINVAL, "%s: the model's background %g is not positive and finite",
                     who, (double)model->background);
  dm = make_dev_model(*model);
  const bool m71 = model->model == SMCDET_MODEL_M71;
  g = (double)dm.g;
  na = m71 ? (double)model->noise_additive : 0.0;
  nm = m71 ? (double)model->noise_multiplicative : 1.0;
  if (!(na >= 0.0) || !(nm >= 0.0) || !(na + nm > 0.0) || !(na + nm < INFINITY))
    return set_error(SMCDET_EINVAL, "%s: noise_additive=%g and noise_multiplicative=%g do not "
                     "give a positive variance", who, na, nm);
  if (!(g > 0.0) || !(g < INFINITY))
    return set_error(SMCDET_EINVAL, "%s: adu_per_nmgy=%g is not positive and finite", who, g);
  return SMCDET_OK;
}

}  // namespace
}  // namespace smcdet

extern "C" {

int smcdet_psf_find(const smcdet_image_model_t* model, const float* images,
                    const float* background, const int32_t* counts, const float* locs,
                    const float* fluxes, int32_t T, int32_t G, int32_t K, int32_t cells,
                    const float* thresh, const int32_t* nms_radius, double min_sep,
                    int32_t* counts_out, float* locs_out, float* snr_out, float* flux_hat,
                    int32_t* n_found, float* map_out, void* stream) {
  using namespace smcdet;
  FindArgs a{};
  if (int rc = check_common("psf_find", model, T, G, K, background, a.g, a.na, a.nm, a.m))
    return rc;
  if (cells < 1 || cells > SMCDET_FIND_MAX_CELLS_PER_PIXEL)
    return set_error(SMCDET_EINVAL, "psf_find: cells=%d outside 1..%d", cells,
                     SMCDET_FIND_MAX_CELLS_PER_PIXEL);
  if (!(min_sep >= 0.0) || !(min_sep < INFINITY))
    return set_error(SMCDET_EINVAL, "psf_find: min_sep=%g must be finite and >= 0", min_sep);
  if (!images || !thresh || !nms_radius || !counts_out || !locs_out || !snr_out || !flux_hat ||
      !n_found)
    return set_error(SMCDET_EINVAL, "psf_find: null buffer");
  if ((counts || locs || fluxes) && !(counts && locs && fluxes))
    return set_error(SMCDET_EINVAL, "psf_find: counts, locs and fluxes are given together or "
                     "all null");
  const int64_t ncell = (int64_t)cells * model->H * cells * model->W;
  if (ncell > SMCDET_FIND_MAX_CELLS)
    return set_error(SMCDET_EUNSUPPORTED, "psf_find: %lld cells above %d", (long long)ncell,
                     SMCDET_FIND_MAX_CELLS);
  a.images = images;
  a.background = background;
  a.counts = counts;
  a.locs = locs;
  a.fluxes = fluxes;
  a.thresh = thresh;
  a.nms = nms_radius;
  a.counts_out = counts_out;
  a.locs_out = locs_out;
  a.snr_out = snr_out;
  a.flux_hat = flux_hat;
  a.n_found = n_found;
  a.map_out = map_out;
  a.min_sep = min_sep;
  a.T = T;
  a.G = G;
  a.K = K;
  a.c = cells;
  a.cH = cells * model->H;
  a.cW = cells * model->W;
  const size_t lds = find_lds_bytes(model->H * model->W, (int)ncell);
  const bool m71 = model->model == SMCDET_MODEL_M71;
  const void* kern = m71 ? (const void*)psf_find_kernel<SMCDET_MODEL_M71>
                         : (const void*)psf_find_kernel<SMCDET_MODEL_POISSON>;
  if (int rc = ensure_lds(kern, lds)) return rc;
  const dim3 grid((unsigned)((int64_t)T * G)), block(kFindThreads);
  if (m71)
    launch_sweep(psf_find_kernel<SMCDET_MODEL_M71>, grid, block, lds, (hipStream_t)stream, a);
  else
    launch_sweep(psf_find_kernel<SMCDET_MODEL_POISSON>, grid, block, lds, (hipStream_t)stream, a);
  return check_launch("smcdet_psf_find");
}

int smcdet_psf_recentre(const smcdet_image_model_t* model, const float* images,
                        const float* background, const int32_t* counts, const float* locs,
                        const float* fluxes, int32_t T, int32_t G, int32_t K, int32_t half,
                        double step, float* locs_out, float* snr_out, void* stream) {
  using namespace smcdet;
  MoveArgs a{};
  if (int rc = check_common("psf_recentre", model, T, G, K, background, a.g, a.na, a.nm, a.m))
    return rc;
  if (half < 1 || half > SMCDET_FIND_MAX_HALF)
    return set_error(SMCDET_EINVAL, "psf_recentre: half=%d outside 1..%d", half,
                     SMCDET_FIND_MAX_HALF);
  if (!(step > 0.0) || !(step < INFINITY))
    return set_error(SMCDET_EINVAL, "psf_recentre: step=%g must be positive and finite", step);
  if (!images || !counts || !locs || !fluxes || !locs_out || !snr_out)
    return set_error(SMCDET_EINVAL, "psf_recentre: null buffer");
  a.images = images;
  a.background = background;
  a.counts = counts;
  a.locs = locs;
  a.fluxes = fluxes;
  a.locs_out = locs_out;
  a.snr_out = snr_out;
  a.step = step;
  a.T = T;
  a.G = G;
  a.K = K;
  a.half = half;
  const int side = 2 * half + 1;
  const size_t lds = move_lds_bytes(model->H * model->W, K, side * side);
  static_assert(move_lds_bytes(SMCDET_EXTRACT_MAX_PIXELS, kMaxK, kMaxCand) <= 65536, "LDS");
  const dim3 grid((unsigned)((int64_t)T * G)), block(kWave);
  if (model->model == SMCDET_MODEL_M71)
    launch_sweep(psf_recentre_kernel<SMCDET_MODEL_M71>, grid, block, lds, (hipStream_t)stream, a);
  else
    launch_sweep(psf_recentre_kernel<SMCDET_MODEL_POISSON>, grid, block, lds, (hipStream_t)stream,
                 a);
  return check_launch("smcdet_psf_recentre");
}

}  // extern "C"
