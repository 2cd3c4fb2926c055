// predictive_kernel.hip — posterior-predictive images and model checks:
// smcdet_posterior_image, smcdet_posterior_image_workspace.
//
// Every catalog is rendered once, by one wavefront, and neither its rate image
// nor its replicate image is stored: the wave folds the rate into per-pixel
// float64 sums over catalogs (mean and variance) and into per-catalog float64
// sums over pixels (chi2, chi2_rep, flux_rep).
//
// Moments: with w~ = w / sum(w) and d = rate - background (both exact in
// float64), a workgroup accumulates (sum w~ d, sum w~ d^2) per pixel over its
// chunk of catalogs and writes them to the caller's workspace; the finish
// kernel adds the chunks of a tile in chunk order and forms
// mean = background + S1, var = max(S2 - S1^2, 0).  No atomics anywhere, every
// sum has a fixed order: the outputs are the same bits on every run.
//
// Three render paths, the ones smcdet_loglik dispatches:
//   regs  (<= 1024 pixels, S <= 64): render_regs, 1 / 4 / 16 pixels per lane,
//         the float64 accumulators in registers next to the rate;
//   lds   (<= 4096 pixels, any S): render_sources_mem into the wave's LDS
//         image; the workgroup's 256 threads then fold the four images into
//         thread-owned accumulators (16 pixels per thread);
//   chunk (M71 above 4096 pixels, S <= 64): chunk_rate, 64 pixels at a time,
//         the accumulators in the wave's own slice of the workspace.
#include <math.h>

#include <algorithm>

#include "render.h"

namespace smcdet {
namespace {

constexpr int kPredWaves = 4;
constexpr int kPredBlock = kPredWaves * kWave;
constexpr int kPredPixPerThread = kMaxLdsPixels / kPredBlock;  // lds path: 16
constexpr int kPredMaxChunks = 64;   // catalog chunks per tile
constexpr int kPredMinChunk = 32;    // catalogs per chunk (regs / lds paths)

// How the N catalogs of a tile are split: `chunks` workgroups of `chunk`
// catalogs (a multiple of the 4 waves; the last one may be ragged), `parts`
// partial-sum images per tile (one per workgroup, or one per wave on the
// chunk path) and `bound` >= parts, the number the workspace is sized for
// (non-decreasing in N, which the exact count is not).
struct PredPlan {
  int chunk, chunks, parts, bound;
};

PredPlan pred_plan(int HW, int N) {
  const bool big = HW > kMaxLdsPixels;
  const int min_chunk = big ? kPredWaves : kPredMinChunk;
  // chunk path: at most 64 MiB of per-wave partial images per tile
  const int max_chunks = big ? std::min(kPredMaxChunks, std::max(1, (1 << 20) / HW))
                             : kPredMaxChunks;
  const int cb = std::min((N + min_chunk - 1) / min_chunk, max_chunks);
  PredPlan p;
  p.chunk = kPredWaves * ((N + kPredWaves * cb - 1) / (kPredWaves * cb));
  p.chunks = (N + p.chunk - 1) / p.chunk;
  p.parts = (big ? kPredWaves : 1) * p.chunks;
  p.bound = (big ? kPredWaves : 1) * cb;
  return p;
}

int64_t pred_workspace_bytes(int HW, int T, int N) {
  return (int64_t)T * (int64_t)sizeof(double) +
         (int64_t)T * pred_plan(HW, N).bound * HW * (int64_t)sizeof(double2);
}

struct PredArgs {
  const float* img;      // [T,H,W] or null
  const float* locs;     // [T,N,S,2]
  const float* fluxes;   // [T,N,S]
  const float* weights;  // [T,N] or null
  const double* wsum;    // [T] sum of the weights (read when weights != null)
  int N, S, chunk;
  uint32_t k0, k1;
  uint64_t offset;
  float *chi2, *chi2_rep, *flux_rep;  // [T,N], each nullable
  double2* parts;                     // [T,parts,H*W] (sum w~ d, sum w~ d^2)
};

struct PixSums {
  double chi2, chi2_rep, flux_rep;
};

// the catalog's normalised weight; w / w = 1 exactly when one catalog holds
// all the weight (its variance is then exactly 0)
__device__ __forceinline__ double pred_weight(const PredArgs& a, int t, int n) {
  return a.weights ? (double)a.weights[(size_t)t * a.N + n] / a.wsum[t] : 1.0 / (double)a.N;
}

// one pixel's terms of the per-catalog sums.  The replicate is the draw
// smcdet_sample_image makes for element (t*H*W + p)*N + n of a [T,H,W,N] rate
// array at the same seed and offset: same counter, tags and arithmetic.
template <int MODEL>
__device__ __forceinline__ void pred_pixel(const DevModel& m, const PredArgs& a, float lam, float x,
                                           uint64_t elem, bool want_chi2, bool want_rep,
                                           PixSums& s) {
  // 1 / v(lam) once for both discrepancies (v_rcp_f32: one ulp)
  const float rv = fast_rcp(MODEL == SMCDET_MODEL_M71 ? fmaf(m.eta, lam, m.s0sq) : lam);
  if (want_chi2) {
    const float d = x - lam;
    s.chi2 += (double)(d * d * rv);
  }
  if (want_rep) {
    const uint64_t c = a.offset + elem;
    float xr;
    if constexpr (MODEL == SMCDET_MODEL_M71) {
      U4 r = philox4x32((uint32_t)c, (uint32_t)(c >> 32), 0u, kTagNoise, a.k0, a.k1);
      const float sd = sqrtf(fmaf(m.eta, lam, m.s0sq));
      xr = fmaf(sd, std_normal(r.x, r.y), lam);
    } else {
      xr = poisson_draw(lam, a.k0, a.k1, (uint32_t)c, (uint32_t)(c >> 32));
    }
    const float d = xr - lam;
    s.flux_rep += (double)xr;
    s.chi2_rep += (double)(d * d * rv);
  }
}

// wave sums of the per-catalog terms (float64 across the wave) and their store
__device__ __forceinline__ void pred_store(const PredArgs& a, size_t pid, const PixSums& s,
                                           bool want_chi2, bool want_rep, int lane) {
  if (want_chi2) {
    const double v = wave_sum(s.chi2);
    if (lane == 0) a.chi2[pid] = (float)v;
  }
  if (want_rep) {
    const double f = wave_sum(s.flux_rep), c = wave_sum(s.chi2_rep);
    if (lane == 0) {
      if (a.flux_rep) a.flux_rep[pid] = (float)f;
      if (a.chi2_rep) a.chi2_rep[pid] = (float)c;
    }
  }
}

__device__ __forceinline__ void load_sources(const PredArgs& a, size_t pid, int lane, float& sh,
                                             float& sw, float& sf) {
  sh = sw = sf = 0.f;
  if (lane < a.S) {
    sh = a.locs[(pid * a.S + lane) * 2 + 0];
    sw = a.locs[(pid * a.S + lane) * 2 + 1];
    sf = a.fluxes[pid * a.S + lane];
  }
}

// sum of a tile's weights, float64, fixed order: one workgroup per tile
__global__ __launch_bounds__(kPredBlock) void pred_wsum_kernel(const float* __restrict__ weights,
                                                               int N, double* __restrict__ wsum) {
  __shared__ double sh[kPredBlock];
  const float* w = weights + (size_t)blockIdx.x * N;
  double acc = 0.0;
  for (int n = threadIdx.x; n < N; n += kPredBlock) acc += (double)w[n];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = kPredBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) wsum[blockIdx.x] = sh[0];
}

// ---------------------------------------------------------------------------
// regs path: lane owns pixels 64k + lane, k < PPL, and their accumulators
// ---------------------------------------------------------------------------
template <int MODEL, int PPL>
__global__ __launch_bounds__(kPredBlock) void pred_regs_kernel(DevModel m, PredArgs a) {
  extern __shared__ double2 pred_smem[];
  const int HW = m.H * m.W;
  double2* red = pred_smem;              // [HW] cross-wave sum
  float* xs = (float*)(pred_smem + HW);  // [HW] tile image
  const int t = blockIdx.y, c = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool want_chi2 = a.chi2 != nullptr;
  const bool want_rep = a.chi2_rep != nullptr || a.flux_rep != nullptr;
  if (a.img)
    for (int p = threadIdx.x; p < HW; p += kPredBlock) xs[p] = a.img[(size_t)t * HW + p];
  __syncthreads();
  const int n0 = c * a.chunk, n1 = min(a.N, n0 + a.chunk);
  double a1[PPL], a2[PPL];
#pragma unroll
  for (int k = 0; k < PPL; ++k) a1[k] = a2[k] = 0.0;
  int n = n0 + wave;
  float sh, sw, sf;
  load_sources(a, (size_t)t * a.N + (n < n1 ? n : n0), lane, sh, sw, sf);
  for (; n < n1; n += kPredWaves) {
    const size_t pid = (size_t)t * a.N + n;
    // the next catalog's sources travel while this one renders
    float nh, nw, nf;
    load_sources(a, (size_t)t * a.N + (n + kPredWaves < n1 ? n + kPredWaves : n), lane, nh, nw,
                 nf);
    float lamk[PPL];
    render_regs<MODEL, PPL>(m, lamk, sh, sw, sf, a.S, lane);
    const double wt = pred_weight(a, t, n);
    PixSums s{0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < PPL; ++k) {
      const int p = k * kWave + lane;
      if (k * kWave < HW && p < HW) {
        const double d = (double)lamk[k] - (double)m.bg;
        const double wd = wt * d;
        a1[k] += wd;
        a2[k] = fma(wd, d, a2[k]);
        if (want_chi2 || want_rep)
          pred_pixel<MODEL>(m, a, lamk[k], want_chi2 ? xs[p] : 0.f,
                            ((uint64_t)t * HW + p) * (uint64_t)a.N + (uint64_t)n, want_chi2,
                            want_rep, s);
      }
    }
    pred_store(a, pid, s, want_chi2, want_rep, lane);
    sh = nh;
    sw = nw;
    sf = nf;
  }
  // the four waves' sums, added in wave order
  for (int w = 0; w < kPredWaves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int k = 0; k < PPL; ++k) {
        const int p = k * kWave + lane;
        if (k * kWave < HW && p < HW) {
          double2 r = make_double2(a1[k], a2[k]);
          if (w > 0) {
            r.x += red[p].x;
            r.y += red[p].y;
          }
          red[p] = r;
        }
      }
    }
    __syncthreads();
  }
  double2* out = a.parts + ((size_t)t * gridDim.x + c) * HW;
  for (int p = threadIdx.x; p < HW; p += kPredBlock) out[p] = red[p];
}

// ---------------------------------------------------------------------------
// lds path: a rate image per wave in LDS; thread owns pixels 256k + tid
// ---------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(kPredBlock) void pred_lds_kernel(DevModel m, PredArgs a) {
  extern __shared__ float pred_smem_f[];
  const int HW = m.H * m.W;
  float* xs = pred_smem_f;
  float* lams = pred_smem_f + HW;  // [4][HW]
  const int t = blockIdx.y, c = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* lam = lams + wave * HW;
  const bool want_chi2 = a.chi2 != nullptr;
  const bool want_rep = a.chi2_rep != nullptr || a.flux_rep != nullptr;
  if (a.img)
    for (int p = threadIdx.x; p < HW; p += kPredBlock) xs[p] = a.img[(size_t)t * HW + p];
  __syncthreads();
  const int n0 = c * a.chunk, n1 = min(a.N, n0 + a.chunk);
  double a1[kPredPixPerThread], a2[kPredPixPerThread];
#pragma unroll
  for (int k = 0; k < kPredPixPerThread; ++k) a1[k] = a2[k] = 0.0;
  for (int base = n0; base < n1; base += kPredWaves) {  // workgroup-uniform
    const int n = base + wave;
    if (n < n1) {
      const size_t pid = (size_t)t * a.N + n;
      render_sources_mem<MODEL>(m, lam, a.locs + pid * a.S * 2, a.fluxes + pid * a.S, a.S, lane);
      if (want_chi2 || want_rep) {
        PixSums s{0.0, 0.0, 0.0};
        for (int p = lane; p < HW; p += kWave)
          pred_pixel<MODEL>(m, a, lam[p], want_chi2 ? xs[p] : 0.f,
                            ((uint64_t)t * HW + p) * (uint64_t)a.N + (uint64_t)n, want_chi2,
                            want_rep, s);
        pred_store(a, pid, s, want_chi2, want_rep, lane);
      }
    }
    __syncthreads();
    for (int w = 0; w < kPredWaves; ++w) {
      if (base + w >= n1) break;
      const double wt = pred_weight(a, t, base + w);
      const float* lw = lams + w * HW;
#pragma unroll
      for (int k = 0; k < kPredPixPerThread; ++k) {
        const int p = k * kPredBlock + (int)threadIdx.x;
        if (k * kPredBlock < HW && p < HW) {
          const double d = (double)lw[p] - (double)m.bg;
          const double wd = wt * d;
          a1[k] += wd;
          a2[k] = fma(wd, d, a2[k]);
        }
      }
    }
    __syncthreads();
  }
  double2* out = a.parts + ((size_t)t * gridDim.x + c) * HW;
#pragma unroll
  for (int k = 0; k < kPredPixPerThread; ++k) {
    const int p = k * kPredBlock + (int)threadIdx.x;
    if (k * kPredBlock < HW && p < HW) out[p] = make_double2(a1[k], a2[k]);
  }
}

// ---------------------------------------------------------------------------
// chunk path (M71 above 4096 pixels): the tile image stays in global memory,
// the rate comes 64 pixels at a time, and each wave adds into its own partial
// image in the workspace (lane p % 64 is the only one that ever touches pixel
// p of it: plain loads and stores, program order)
// ---------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(kPredBlock) void pred_chunk_kernel(DevModel m, PredArgs a) {
  const int HW = m.H * m.W;
  const int t = blockIdx.y, c = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool want_chi2 = a.chi2 != nullptr;
  const bool want_rep = a.chi2_rep != nullptr || a.flux_rep != nullptr;
  const int n0 = c * a.chunk, n1 = min(a.N, n0 + a.chunk);
  double2* part =
      a.parts + (((size_t)t * gridDim.x + (size_t)c) * kPredWaves + (size_t)wave) * HW;
  const float* x = a.img ? a.img + (size_t)t * HW : nullptr;
  const float inv_w = 1.0f / (float)m.W;
  bool first = true;
  for (int n = n0 + wave; n < n1; n += kPredWaves) {
    const size_t pid = (size_t)t * a.N + n;
    float sh, sw, sf;
    load_sources(a, pid, lane, sh, sw, sf);
    const ChunkSrc cs = chunk_sources<MODEL>(m, sh, sw, sf, a.S, lane);
    const double wt = pred_weight(a, t, n);
    PixSums s{0.0, 0.0, 0.0};
    for (int k = 0; k * kWave < HW; ++k) {
      const int p = k * kWave + lane;
      const float lam = chunk_rate<MODEL>(m, cs, a.S, k, lane, inv_w);
      if (p < HW) {
        const double d = (double)lam - (double)m.bg;
        const double wd = wt * d;
        double2 r = make_double2(wd, wd * d);
        if (!first) {
          const double2 o = part[p];
          r.x = o.x + wd;
          r.y = fma(wd, d, o.y);
        }
        part[p] = r;
        if (want_chi2 || want_rep)
          pred_pixel<MODEL>(m, a, lam, want_chi2 ? x[p] : 0.f,
                            ((uint64_t)t * HW + p) * (uint64_t)a.N + (uint64_t)n, want_chi2,
                            want_rep, s);
      }
    }
    pred_store(a, pid, s, want_chi2, want_rep, lane);
    first = false;
  }
  if (first)  // a wave of the ragged last chunk without a catalog
    for (int p = lane; p < HW; p += kWave) part[p] = make_double2(0.0, 0.0);
}

// mean and variance from a tile's partial sums, added in chunk order
__global__ void pred_finish_kernel(const double2* __restrict__ parts, int parts_per_tile, int HW,
                                   int64_t total, float bg, float* __restrict__ mean,
                                   float* __restrict__ var) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t t = i / HW;
  const int p = (int)(i - t * HW);
  const double2* src = parts + (size_t)t * parts_per_tile * HW + p;
  double s1 = 0.0, s2 = 0.0;
  for (int q = 0; q < parts_per_tile; ++q) {
    const double2 v = src[(size_t)q * HW];
    s1 += v.x;
    s2 += v.y;
  }
  mean[i] = (float)((double)bg + s1);
  // S1^2 rounded on its own, not fused into the subtraction: a single catalog
  // leaves S2 = fl(d^2) and S1 = d, and the variance is then exactly 0
  double v;
  {
#pragma clang fp contract(off)
    const double sq = s1 * s1;
    v = s2 - sq;
  }
  var[i] = (float)(v < 0.0 ? 0.0 : v);  // (NaN, from weights that sum to 0, stays NaN)
}

int pred_validate(const smcdet_image_model_t* model, int32_t T, int32_t N) {
  const int rc = validate_model(model, kMaxGlobalPixels);
  if (rc) return rc;
  if (T <= 0 || N <= 0) return set_error(SMCDET_EUNSUPPORTED, "T=%d N=%d (need T,N>0)", T, N);
  if (T > 65535) return set_error(SMCDET_EUNSUPPORTED, "T=%d > 65535", T);
  return SMCDET_OK;
}

}  // namespace
}  // namespace smcdet

using namespace smcdet;

extern "C" {

int64_t smcdet_posterior_image_workspace(const smcdet_image_model_t* model, int32_t T,
                                         int32_t N) {
  const int rc = pred_validate(model, T, N);
  if (rc) return rc;
  return pred_workspace_bytes(model->H * model->W, T, N);
}

int smcdet_posterior_image(const smcdet_image_model_t* model, const float* tiled_image,
                           const float* locs, const float* fluxes, const float* weights,
                           int32_t T, int32_t N, int32_t S, uint64_t seed, uint64_t offset,
                           float* mean, float* var, float* chi2, float* chi2_rep,
                           float* flux_rep, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  int rc = validate_model(model, kMaxGlobalPixels);
  if (rc) return rc;
  // (S = 0: the catalog buffers are empty, never read, and may be null)
  if (!mean || !var || !workspace || (S > 0 && (!locs || !fluxes)))
    return set_error(SMCDET_EINVAL, "null buffer");
  if (chi2 && !tiled_image)
    return set_error(SMCDET_EINVAL, "chi2 needs tiled_image (it is null)");
  if (S < 0) return set_error(SMCDET_EUNSUPPORTED, "S=%d (need S>=0)", S);
  rc = pred_validate(model, T, N);
  if (rc) return rc;
  const DevModel m = make_dev_model(*model);
  const int HW = m.H * m.W;
  if (HW > kMaxLdsPixels && S > kWave)
    return set_error(SMCDET_EUNSUPPORTED, "S=%d > 64 above %d pixels", S, kMaxLdsPixels);
  const int64_t need = pred_workspace_bytes(HW, T, N);
  if (workspace_bytes < need)
    return set_error(SMCDET_EINVAL, "workspace of %lld bytes, %lld required",
                     (long long)workspace_bytes, (long long)need);
  if (((uintptr_t)workspace & 15u) != 0)
    return set_error(SMCDET_EINVAL, "workspace must be 16-byte aligned");

  hipStream_t st = (hipStream_t)stream;
  const PredPlan plan = pred_plan(HW, N);
  // workspace: the tiles' partial-sum images, then the tiles' weight sums
  PredArgs a;
  a.parts = (double2*)workspace;
  double* wsum = (double*)(a.parts + (size_t)T * plan.bound * HW);
  a.img = tiled_image;
  a.locs = locs;
  a.fluxes = fluxes;
  a.weights = weights;
  a.wsum = wsum;
  a.N = N;
  a.S = S;
  a.chunk = plan.chunk;
  a.k0 = (uint32_t)seed;
  a.k1 = (uint32_t)(seed >> 32);
  a.offset = offset;
  a.chi2 = chi2;
  a.chi2_rep = chi2_rep;
  a.flux_rep = flux_rep;
  if (weights)
    hipLaunchKernelGGL(pred_wsum_kernel, dim3(T), dim3(kPredBlock), 0, st, weights, N, wsum);
  const dim3 grid(plan.chunks, T);
  const bool m71 = m.model == SMCDET_MODEL_M71;
  if (HW > kMaxLdsPixels) {  // M71 (validate_model)
    hipLaunchKernelGGL(pred_chunk_kernel<SMCDET_MODEL_M71>, grid, dim3(kPredBlock), 0, st, m, a);
  } else if (S > kWave || HW > 1024) {
    const size_t lds = (size_t)(1 + kPredWaves) * HW * sizeof(float);
    const void* fn = m71 ? (const void*)pred_lds_kernel<SMCDET_MODEL_M71>
                         : (const void*)pred_lds_kernel<SMCDET_MODEL_POISSON>;
    rc = ensure_lds(fn, lds);
    if (rc) return rc;
    if (m71)
      hipLaunchKernelGGL(pred_lds_kernel<SMCDET_MODEL_M71>, grid, dim3(kPredBlock), lds, st, m, a);
    else
      hipLaunchKernelGGL(pred_lds_kernel<SMCDET_MODEL_POISSON>, grid, dim3(kPredBlock), lds, st,
                         m, a);
  } else {
    const size_t lds = (size_t)HW * (sizeof(double2) + sizeof(float));
    const int ppl = HW <= 64 ? 1 : (HW <= 256 ? 4 : 16);
#define SMCDET_PRED_LAUNCH(MDL, P)                                                             \
  hipLaunchKernelGGL((pred_regs_kernel<MDL, P>), grid, dim3(kPredBlock), lds, st, m, a)
    if (m71) {
      if (ppl == 1) SMCDET_PRED_LAUNCH(SMCDET_MODEL_M71, 1);
      else if (ppl == 4) SMCDET_PRED_LAUNCH(SMCDET_MODEL_M71, 4);
      else SMCDET_PRED_LAUNCH(SMCDET_MODEL_M71, 16);
    } else {
      if (ppl == 1) SMCDET_PRED_LAUNCH(SMCDET_MODEL_POISSON, 1);
      else if (ppl == 4) SMCDET_PRED_LAUNCH(SMCDET_MODEL_POISSON, 4);
      else SMCDET_PRED_LAUNCH(SMCDET_MODEL_POISSON, 16);
    }
#undef SMCDET_PRED_LAUNCH
  }
  rc = check_launch("smcdet_posterior_image");
  if (rc) return rc;
  const int64_t total = (int64_t)T * HW;
  hipLaunchKernelGGL(pred_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                     (const double2*)a.parts, plan.parts, HW, total, m.bg, mean, var);
  return check_launch("smcdet_posterior_image");
}

}  // extern "C"
