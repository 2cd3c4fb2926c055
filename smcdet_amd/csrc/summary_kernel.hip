// summary_kernel.hip — posterior calibration summaries: the
// per-catalog functionals, order statistics along the catalog axis and
// bootstrap row means that the count heat maps, the coverage of total flux,
// the luminosity function and the precision / recall bands are made of.
//
//   catalog_totals_kernel   256 catalogs per workgroup, staged 16 slots at a
//                           time through LDS (contiguous global reads); one
//                           thread per catalog adds its counted slots in float64
//   row_summary_kernel      one workgroup per row: order-preserving uint32 keys
//                           (NaN last; with weights the catalog index as the low
//                           word of a 64-bit key) bitonic-sorted in LDS sized to
//                           the next power of two >= N, float64 segment sums and
//                           one block scan, then one thread per quantile level
//                           or threshold
//   bootstrap_means_kernel  one workgroup per replicate: lanes across columns,
//                           wave groups across draws (one Philox call = 4 draws),
//                           float64 partial sums added through LDS in group order
//
// No float atomics: every sum has a fixed order.
#include <type_traits>

#include "device.h"

namespace smcdet {
namespace {

// ---- catalog totals ---------------------------------------------------------
constexpr int kTotThreads = 256;
constexpr int kTotSlots = 16;

struct TotArgs {
  const int32_t* counts;
  const float* fluxes;
  int32_t* n_above;
  float* flux_above;
  float cuts[SMCDET_TOTALS_MAX_CUTS];
  int64_t TN;
  int32_t S, C;
};

__global__ __launch_bounds__(kTotThreads) void catalog_totals_kernel(TotArgs a) {
  __shared__ float tile[kTotThreads][kTotSlots + 1];  // +1: a catalog per bank
  const int tid = threadIdx.x;
  const int64_t cat0 = (int64_t)blockIdx.x * kTotThreads, cat = cat0 + tid;
  const int64_t left = a.TN - cat0;
  const int ncat = left < kTotThreads ? (int)left : kTotThreads;
  const int cnt = tid < ncat ? min(max(a.counts[cat], 0), a.S) : 0;
  double sum[SMCDET_TOTALS_MAX_CUTS];
  int num[SMCDET_TOTALS_MAX_CUTS];
#pragma unroll
  for (int c = 0; c < SMCDET_TOTALS_MAX_CUTS; ++c) {
    sum[c] = 0.0;
    num[c] = 0;
  }
  for (int s0 = 0; s0 < a.S; s0 += kTotSlots) {
    const int ns = min(kTotSlots, a.S - s0);
    // 16 consecutive lanes read 16 consecutive slots of one catalog
    for (int e = tid; e < ncat * kTotSlots; e += kTotThreads) {
      const int c = e / kTotSlots, s = e % kTotSlots;
      if (s < ns) tile[c][s] = a.fluxes[(cat0 + c) * a.S + s0 + s];
    }
    __syncthreads();
    const int m = min(ns, cnt - s0);  // slots at or past the count are never read
    for (int s = 0; s < m; ++s) {
      const float f = tile[tid][s];
#pragma unroll
      for (int c = 0; c < SMCDET_TOTALS_MAX_CUTS; ++c)
        if (c < a.C && f >= a.cuts[c]) {
          ++num[c];
          sum[c] += (double)f;
        }
    }
    __syncthreads();
  }
  if (tid < ncat) {
#pragma unroll
    for (int c = 0; c < SMCDET_TOTALS_MAX_CUTS; ++c)
      if (c < a.C) {
        a.n_above[(int64_t)c * a.TN + cat] = num[c];
        a.flux_above[(int64_t)c * a.TN + cat] = (float)sum[c];
      }
  }
}

// ---- row summary ------------------------------------------------------------
constexpr int kSumMaxThreads = 1024;
constexpr int kSumMinPow2 = 64;
constexpr uint32_t kKeyNaN = 0xffffffffu;

struct SumArgs {
  const float* values;
  const float* weights;
  const float* thresholds;
  int32_t* n_valid;
  double* weight;
  double* mean;
  double* var;
  float* vmin;
  float* vmax;
  float* quantiles;
  double* below;
  double* at_or_below;
  double q[SMCDET_SUMMARY_MAX_Q];
  int32_t N, B, Q, E, P, lower;
};

// float32 -> uint32 with the same order (-inf .. -0 < +0 .. +inf), NaN last
__device__ __forceinline__ uint32_t key_of_float(float f) {
  const uint32_t u = __float_as_uint(f);
  if (f != f) return kKeyNaN;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of_key(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ uint32_t hi_word(uint32_t k) { return k; }
__device__ __forceinline__ uint32_t hi_word(uint64_t k) { return (uint32_t)(k >> 32); }

// threads of the workgroup for a sort of P = 2^k >= 64 keys: 8 keys per thread,
// 64..1024 threads
__host__ __device__ inline int summary_threads(int P) {
  const int t = P / 8;
  return t < 64 ? 64 : (t > kSumMaxThreads ? kSumMaxThreads : t);
}
// LDS: [threads] float64 inclusive weight prefixes, [24] float64 wave totals,
// [P] keys
__host__ __device__ inline size_t summary_lds_bytes(int P, bool weighted) {
  return (size_t)(summary_threads(P) + 24) * sizeof(double) + (size_t)P * (weighted ? 8 : 4);
}

// inclusive scan of v over the workgroup in thread order; *total = the sum of
// all threads, formed in the same order by every thread
__device__ __forceinline__ double block_scan(double v, double* wsum, double* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  __syncthreads();  // the previous scan's wave totals have been read
  if (lane == 63) wsum[wv] = v;
  __syncthreads();
  double off = 0.0, tot = 0.0;
  for (int w = 0; w < nw; ++w) {
    const double x = wsum[w];
    if (w < wv) off += x;
    tot += x;
  }
  *total = tot;
  return off + v;
}

template <bool W>
__global__ __launch_bounds__(kSumMaxThreads) void row_summary_kernel(SumArgs a) {
  using K = typename std::conditional<W, uint64_t, uint32_t>::type;
  extern __shared__ double summary_lds[];
  const int tid = threadIdx.x, nt = blockDim.x;
  double* incl = summary_lds;
  double* wsum = incl + nt;
  K* s = reinterpret_cast<K*>(wsum + 24);
  const int P = a.P, L = P / nt;
  const int64_t row = blockIdx.x;  // = ia * B + ib: b fastest
  const int64_t ia = row / a.B;
  const int ib = (int)(row - ia * a.B);
  const float* vals = a.values + ia * a.N * a.B + ib;
  const float* wts = W ? a.weights + ia * a.N : nullptr;

  // keys (and the catalog index as the payload) into LDS; entries past N are
  // padding that sorts with the NaNs
  int valid = 0;
  for (int i = tid; i < P; i += nt) {
    uint32_t key = kKeyNaN;
    if (i < a.N) {
      key = key_of_float(vals[(int64_t)i * a.B]);
      valid += key != kKeyNaN;
    }
    if (W)
      s[i] = (K)(((uint64_t)key << 32) | (uint32_t)i);
    else
      s[i] = (K)key;
  }
  double tot;
  block_scan((double)valid, wsum, &tot);  // (its barriers also publish the keys)
  const int nv = (int)tot;

  // bitonic sort, ascending; the 64-bit keys are all different, so the order
  // of equal values is that of their indices
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < (P >> 1); i += nt) {
        const int lo = 2 * i - (i & (j - 1)), hi = lo + j;
        const K x = s[lo], y = s[hi];
        if ((x > y) == ((lo & k) == 0)) {
          s[lo] = y;
          s[hi] = x;
        }
      }
      __syncthreads();
    }

  // this thread's contiguous sorted segment, cut at the valid entries
  const int i0 = min(tid * L, nv), i1 = min(tid * L + L, nv);
  double sw = 0.0, swv = 0.0;
  for (int i = i0; i < i1; ++i) {
    const double v = (double)float_of_key(hi_word(s[i]));
    float wf = 1.f;
    if (W) {
      // the payload has served: from here on the low word is the weight
      const uint64_t e = (uint64_t)s[i];
      wf = wts[(uint32_t)e];
      s[i] = (K)((e & 0xffffffff00000000ull) | __float_as_uint(wf));
    }
    sw += (double)wf;
    swv += (double)wf * v;
  }
  double wtot, vtot, dtot;
  const double cum = block_scan(sw, wsum, &wtot);
  incl[tid] = cum;
  block_scan(swv, wsum, &vtot);
  const double mean = vtot / wtot;  // 0 / 0 = NaN for a row without weight
  double sd = 0.0;
  for (int i = i0; i < i1; ++i) {
    const K e = s[i];
    const double d = (double)float_of_key(hi_word(e)) - mean;
    const double w = W ? (double)__uint_as_float((uint32_t)e) : 1.0;
    sd += w * d * d;
  }
  block_scan(sd, wsum, &dtot);  // (its barriers also publish incl and the weights)
  if (tid == 0) {
    const double var = dtot / wtot;
    a.n_valid[row] = nv;
    a.weight[row] = wtot;
    a.mean[row] = mean;
    a.var[row] = var < 0.0 ? 0.0 : var;  // (NaN stays NaN)
    a.vmin[row] = nv > 0 ? float_of_key(hi_word(s[0])) : NAN;
    a.vmax[row] = nv > 0 ? float_of_key(hi_word(s[nv - 1])) : NAN;
  }

  // weight of the first p sorted entries (p <= nv)
  auto mass = [&](int p) -> double {
    if (!W) return (double)p;
    const int t = p / L;
    if (t >= nt) return incl[nt - 1];
    double c = t > 0 ? incl[t - 1] : 0.0;
    for (int i = t * L; i < p; ++i) c += (double)__uint_as_float((uint32_t)s[i]);
    return c;
  };

  // one thread per quantile level
  for (int qi = tid; qi < a.Q; qi += nt) {
    const double q = a.q[qi];
    float out = NAN;
    if (nv > 0 && wtot > 0.0) {
      if (!a.lower) {
        const double pos = q * (double)(nv - 1);
        const double fl = floor(pos), g = pos - fl;
        const int lo = min((int)fl, nv - 1), hi = min(lo + 1, nv - 1);
        const double vlo = (double)float_of_key(hi_word(s[lo]));
        const double vhi = (double)float_of_key(hi_word(s[hi]));
        out = g == 0.0 ? (float)vlo : (float)(vlo + (vhi - vlo) * g);
      } else {
        const double target = q * wtot;
        int pos;
        if (!W) {
          // cumulative weights 1, 2, ...: the entries with i + 1 < target come first
          pos = (int)ceil(target) - 1;
        } else {
          // the first thread whose inclusive prefix reaches the target, then
          // the first entry of its segment that does
          int t0 = 0, t1 = nt - 1;
          while (t0 < t1) {
            const int m = (t0 + t1) >> 1;
            if (incl[m] >= target)
              t1 = m;
            else
              t0 = m + 1;
          }
          double c = t0 > 0 ? incl[t0 - 1] : 0.0;
          const int e1 = min(t0 * L + L, nv);
          pos = e1 - 1;
          for (int i = min(t0 * L, nv); i < e1; ++i) {
            c += (double)__uint_as_float((uint32_t)s[i]);
            if (c >= target) {
              pos = i;
              break;
            }
          }
        }
        pos = min(max(pos, 0), nv - 1);
        out = float_of_key(hi_word(s[pos]));
      }
    }
    a.quantiles[row * a.Q + qi] = out;
  }

  // one thread per (threshold, strict or not): a binary search of the keys
  for (int task = tid; task < 2 * a.E; task += nt) {
    const int k = task >> 1;
    const bool strict = (task & 1) == 0;
    const float e = a.thresholds[row * a.E + k];
    int p = 0;
    if (e == e) {
      // -0 == +0: "< 0" stops before the key of -0, "<= 0" runs past that of +0
      const uint32_t ke = key_of_float(e == 0.f ? (strict ? -0.f : 0.f) : e);
      int lo = 0, hi = P;  // the number of keys < ke (strict) or <= ke
      while (lo < hi) {
        const int m = (lo + hi) >> 1;
        const uint32_t km = hi_word(s[m]);
        if (strict ? km < ke : km <= ke)
          lo = m + 1;
        else
          hi = m;
      }
      p = min(lo, nv);
    }
    (strict ? a.below : a.at_or_below)[row * a.E + k] = mass(p);
  }
}

// ---- bootstrap means ----------------------------------------------------------
constexpr int kBootThreads = 256;

struct BootArgs {
  const float* values;
  const int32_t* indices;
  float* out;
  uint32_t k0, k1;
  int32_t M, D, Dp;
};

__global__ __launch_bounds__(kBootThreads) void bootstrap_means_kernel(BootArgs a) {
  __shared__ double part[kBootThreads];
  const int tid = threadIdx.x;
  const uint32_t r = blockIdx.x;
  // Dp = D rounded up to whole waves; G = 256 / Dp groups of Dp lanes share the
  // draws, four (one Philox call) at a time
  const int G = kBootThreads / a.Dp, g = tid / a.Dp, d = tid - g * a.Dp;
  const bool on = g < G && d < a.D;
  const int dd = on ? d : 0;
  const int quads = (a.M + 3) >> 2;
  const uint32_t M = (uint32_t)a.M;
  double acc = 0.0;
  if (g < G)
    for (int qd = g; qd < quads; qd += G) {
      const int j0 = 4 * qd;
      uint32_t idx[4];
      if (a.indices) {
        const int32_t* ix = a.indices + (int64_t)r * a.M + j0;
#pragma unroll
        for (int k = 0; k < 4; ++k) idx[k] = j0 + k < a.M ? (uint32_t)ix[k] : 0u;
      } else {
        const U4 u = philox4x32(r, (uint32_t)qd, 0u, kTagBoot, a.k0, a.k1);
        idx[0] = __umulhi(u.x, M);
        idx[1] = __umulhi(u.y, M);
        idx[2] = __umulhi(u.z, M);
        idx[3] = __umulhi(u.w, M);
      }
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        v[k] = j0 + k < a.M ? a.values[(int64_t)idx[k] * a.D + dd] : 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += (double)v[k];
    }
  part[tid] = on ? acc : 0.0;
  __syncthreads();
  if (tid < a.D) {
    double sum = 0.0;
    for (int gg = 0; gg < G; ++gg) sum += part[gg * a.Dp + tid];
    a.out[(int64_t)r * a.D + tid] = (float)(sum / (double)a.M);
  }
}

}  // namespace
}  // namespace smcdet

extern "C" {

int smcdet_catalog_totals(const int32_t* counts, const float* fluxes, const float* flux_cuts,
                          int32_t T, int32_t N, int32_t S, int32_t C, int32_t* n_above,
                          float* flux_above, void* stream) {
  using namespace smcdet;
  if (C > SMCDET_TOTALS_MAX_CUTS)
    return set_error(SMCDET_EUNSUPPORTED, "catalog_totals: C = %d flux cuts above %d", C,
                     SMCDET_TOTALS_MAX_CUTS);
  if (S > SMCDET_MATCH_MAX_SOURCES)
    return set_error(SMCDET_EUNSUPPORTED, "catalog_totals: S = %d slots above %d", S,
                     SMCDET_MATCH_MAX_SOURCES);
  if (T < 1 || N < 1 || S < 1 || C < 1)
    return set_error(SMCDET_EINVAL, "catalog_totals: T=%d N=%d S=%d C=%d must be >= 1", T, N, S, C);
  if ((int64_t)T * N > 0x7fffffffll)
    return set_error(SMCDET_EUNSUPPORTED, "catalog_totals: T*N = %lld catalogs exceed 2^31-1",
                     (long long)T * N);
  if (!counts || !fluxes || !flux_cuts || !n_above || !flux_above)
    return set_error(SMCDET_EINVAL, "catalog_totals: null buffer");
  TotArgs a{};
  a.counts = counts;
  a.fluxes = fluxes;
  a.n_above = n_above;
  a.flux_above = flux_above;
  for (int c = 0; c < C; ++c) {
    if (flux_cuts[c] != flux_cuts[c])
      return set_error(SMCDET_EINVAL, "catalog_totals: flux_cuts[%d] is NaN", c);
    a.cuts[c] = flux_cuts[c];
  }
  a.TN = (int64_t)T * N;
  a.S = S;
  a.C = C;
  const int64_t blocks = (a.TN + kTotThreads - 1) / kTotThreads;
  launch_sweep(catalog_totals_kernel, dim3((unsigned)blocks), dim3(kTotThreads), 0,
               (hipStream_t)stream, a);
  return check_launch("smcdet_catalog_totals");
}

int smcdet_row_summary(const float* values, const float* weights, int32_t A, int32_t N, int32_t B,
                       const double* q, int32_t Q, int32_t interpolation, const float* thresholds,
                       int32_t E, int32_t* n_valid, double* weight, double* mean, double* var,
                       float* vmin, float* vmax, float* quantiles, double* below,
                       double* at_or_below, void* stream) {
  using namespace smcdet;
  if (N > SMCDET_SUMMARY_MAX_N)
    return set_error(SMCDET_EUNSUPPORTED,
                     "row_summary: N = %d entries per row above %d (the row is sorted in LDS)", N,
                     SMCDET_SUMMARY_MAX_N);
  if (Q > SMCDET_SUMMARY_MAX_Q)
    return set_error(SMCDET_EUNSUPPORTED, "row_summary: Q = %d quantile levels above %d", Q,
                     SMCDET_SUMMARY_MAX_Q);
  if (E > SMCDET_SUMMARY_MAX_E)
    return set_error(SMCDET_EUNSUPPORTED, "row_summary: E = %d thresholds above %d", E,
                     SMCDET_SUMMARY_MAX_E);
  if (A < 1 || N < 1 || B < 1 || Q < 0 || E < 0)
    return set_error(SMCDET_EINVAL, "row_summary: A=%d N=%d B=%d must be >= 1, Q=%d E=%d >= 0", A,
                     N, B, Q, E);
  if ((int64_t)A * B > 0x7fffffffll)
    return set_error(SMCDET_EUNSUPPORTED, "row_summary: A*B = %lld rows exceed 2^31-1",
                     (long long)A * B);
  if (interpolation != SMCDET_SUMMARY_LINEAR && interpolation != SMCDET_SUMMARY_LOWER)
    return set_error(SMCDET_EINVAL, "row_summary: unknown interpolation %d", interpolation);
  if (interpolation == SMCDET_SUMMARY_LINEAR && weights)
    return set_error(SMCDET_EINVAL,
                     "row_summary: linear interpolation takes no weights (use "
                     "SMCDET_SUMMARY_LOWER)");
  if (!values || !n_valid || !weight || !mean || !var || !vmin || !vmax ||
      (Q > 0 && (!q || !quantiles)) || (E > 0 && (!thresholds || !below || !at_or_below)))
    return set_error(SMCDET_EINVAL, "row_summary: null buffer");
  SumArgs a{};
  for (int i = 0; i < Q; ++i) {
    if (!(q[i] >= 0.0 && q[i] <= 1.0))
      return set_error(SMCDET_EINVAL, "row_summary: q[%d] = %g outside [0, 1]", i, q[i]);
    a.q[i] = q[i];
  }
  int P = kSumMinPow2;
  while (P < N) P <<= 1;
  a.values = values;
  a.weights = weights;
  a.thresholds = thresholds;
  a.n_valid = n_valid;
  a.weight = weight;
  a.mean = mean;
  a.var = var;
  a.vmin = vmin;
  a.vmax = vmax;
  a.quantiles = quantiles;
  a.below = below;
  a.at_or_below = at_or_below;
  a.N = N;
  a.B = B;
  a.Q = Q;
  a.E = E;
  a.P = P;
  a.lower = interpolation == SMCDET_SUMMARY_LOWER;
  const bool weighted = weights != nullptr;
  const size_t lds = summary_lds_bytes(P, weighted);
  const int rc = ensure_lds(weighted ? (const void*)row_summary_kernel<true>
                                     : (const void*)row_summary_kernel<false>, lds);
  if (rc != SMCDET_OK) return rc;
  const dim3 grid((unsigned)((int64_t)A * B)), block(summary_threads(P));
  if (weighted)
    launch_sweep(row_summary_kernel<true>, grid, block, lds, (hipStream_t)stream, a);
  else
    launch_sweep(row_summary_kernel<false>, grid, block, lds, (hipStream_t)stream, a);
  return check_launch("smcdet_row_summary");
}

int smcdet_bootstrap_means(const float* values, int32_t M, int32_t D, const int32_t* indices,
                           uint64_t seed, int32_t Bn, float* out, void* stream) {
  using namespace smcdet;
  if (D > SMCDET_BOOT_MAX_COLUMNS)
    return set_error(SMCDET_EUNSUPPORTED, "bootstrap_means: D = %d columns above %d", D,
                     SMCDET_BOOT_MAX_COLUMNS);
  if (M < 1 || D < 1 || Bn < 1)
    return set_error(SMCDET_EINVAL, "bootstrap_means: M=%d D=%d Bn=%d must be >= 1", M, D, Bn);
  if (!values || !out) return set_error(SMCDET_EINVAL, "bootstrap_means: null buffer");
  BootArgs a{values, indices, out, (uint32_t)seed, (uint32_t)(seed >> 32), M, D,
             (D + 63) / 64 * 64};
  launch_sweep(bootstrap_means_kernel, dim3((unsigned)Bn), dim3(kBootThreads), 0,
               (hipStream_t)stream, a);
  return check_launch("smcdet_bootstrap_means");
}

}  // extern "C"
