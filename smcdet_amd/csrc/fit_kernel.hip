// fit_kernel.hip — the objective of the image-model fit: the
// masked Gaussian negative log-likelihood of F calibration fields under the M71
// image model with the catalog held fixed, its gradient and its expected
// Fisher information in the logs of the ten parameters, all in float64.
//
//   fit_norm_kernel    the normaliser: seven sums of the profile's pieces over
//                      one quadrant of the (32R)^2 grid (the grid is symmetric
//                      in both axes), kFitNormBlocks workgroups, fixed strides
//   fit_pixel_kernel   a workgroup per 16 x 16 pixel block: the field's stars
//                      in LDS-staged chunks of 256, compacted in catalog order
//                      to those whose clipped window meets the block; each
//                      thread sums the same seven pieces for its pixel, forms
//                      lambda, v, its nll term, 10 gradient and 55 information
//                      terms; a fixed tree per workgroup into the workspace
//   fit_final_kernel   one workgroup per output sum: the pixel workgroups'
//                      partial sums in a fixed order
//
// The seven pieces of a profile sum X (weights f; f = 1 on the normaliser grid),
// with t1 = exp(-r2/(2 s1)), t2 = exp(-r2/(2 s2)), x = r2/(beta sp),
// t3 = (1 + x)^(-beta/2):
//   X0 = sum f t1      X1 = sum f t2      X2 = sum f t3
//   X3 = sum f t1 r2   X4 = sum f t2 r2
//   X5 = sum f t3 x/(1+x)     X6 = sum f t3 (x/(1+x) - log(1+x))
// from which sum f u and its six partials in the logs follow (fit_combine).
//
// No atomics: every sum has a fixed order.
#include <cmath>

#include "device.h"

namespace smcdet {
namespace {

constexpr int kFitP = SMCDET_FIT_PARAMS;
constexpr int kFitTerms = SMCDET_FIT_TERMS;
constexpr int kFitB = SMCDET_FIT_BLOCK;
constexpr int kFitThreads = kFitB * kFitB;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kFitNormBlocks = SMCDET_FIT_NORM_BLOCKS;
constexpr int kFitSums = SMCDET_FIT_NORM_SUMS;
static_assert(kFitTerms == 1 + kFitP + kFitP * (kFitP + 1) / 2, "nll, grad, upper triangle");
static_assert(kFitThreads == 256 && kFitWaves == 4, "16 x 16 pixels, four waves");

// exp(log_theta) and what the profile needs of it, formed once on the host
struct FitTheta {
  double g, b, p0, nm, na, bg;
  double i2s1, i2s2;  // 1 / (2 sigma1), 1 / (2 sigma2)
  double ibs;         // 1 / (beta sigmap)
  double hb;          // beta / 2
  double iz;          // 1 / (1 + b + p0)
};

struct FitArgs {
  FitTheta th;
  const float* images;
  const uint8_t* mask;
  const float* locs;
  const float* fluxes;
  const int32_t* counts;
  float* rate;
  double* norm_part;  // [kFitNormBlocks, kFitSums]
  double* part;       // [blocks, kFitTerms]
  int32_t F, H, W, D, R, nbh, nbw;
};

// the sum of v over the wave, the same bits in every lane
__device__ __forceinline__ double fit_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// X[0..6] += f * (the seven pieces at r2)
__device__ __forceinline__ void fit_pieces(const FitTheta& th, double r2, double f, double* X) {
  const double t1 = exp(-r2 * th.i2s1);
  const double t2 = exp(-r2 * th.i2s2);
  const double x = r2 * th.ibs;
  const double lq = log1p(x);
  const double t3 = exp(-th.hb * lq);
  const double xq = x / (1.0 + x);
  const double f1 = f * t1, f2 = f * t2, f3 = f * t3;
  X[0] += f1;
  X[1] += f2;
  X[2] += f3;
  X[3] += f1 * r2;
  X[4] += f2 * r2;
  X[5] += f3 * xq;
  X[6] += f3 * (xq - lq);
}

// U[0] = sum f u, U[1..6] = its partials in log sigma1, sigma2, sigmap, beta, b, p0
__device__ __forceinline__ void fit_combine(const FitTheta& th, const double* X, double* U) {
  const double u = (X[0] + th.b * X[1] + th.p0 * X[2]) * th.iz;
  U[0] = u;
  U[1] = X[3] * th.i2s1 * th.iz;
  U[2] = th.b * X[4] * th.i2s2 * th.iz;
  U[3] = th.p0 * th.hb * X[5] * th.iz;
  U[4] = th.p0 * th.hb * X[6] * th.iz;
  U[5] = th.b * (X[1] - u) * th.iz;
  U[6] = th.p0 * (X[2] - u) * th.iz;
}

__global__ __launch_bounds__(kFitThreads) void fit_norm_kernel(FitTheta th, int32_t R,
                                                               double* norm_part) {
  __shared__ double sh[kFitWaves][kFitSums];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = 16 * R;  // the quadrant's side: offsets i + 1/2, i = 0 .. 16R-1
  const int Q = n * n;
  double X[kFitSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = blockIdx.x * kFitThreads + tid; q < Q; q += kFitNormBlocks * kFitThreads) {
    const int i = q / n, j = q - i * n;
    const double a = (double)i + 0.5, c = (double)j + 0.5;
    fit_pieces(th, a * a + c * c, 1.0, X);
  }
#pragma unroll
  for (int k = 0; k < kFitSums; ++k) {
    const double s = fit_wave_sum(X[k]);
    if (lane == 0) sh[wv][k] = s;
  }
  __syncthreads();
  if (tid < kFitSums)
    norm_part[blockIdx.x * kFitSums + tid] =
        (sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid]);
}

struct FitShared {
  double h[kFitThreads], w[kFitThreads], f[kFitThreads];
  int fh[kFitThreads], fw[kFitThreads];
  double norm[kFitSums];
  double red[kFitWaves][kFitTerms];
  int wcount[kFitWaves];
};

__global__ __launch_bounds__(kFitThreads) void fit_pixel_kernel(FitArgs a) {
  __shared__ FitShared sh;
  const FitTheta& th = a.th;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int blk = blockIdx.x;
  const int bw = blk % a.nbw, bh = (blk / a.nbw) % a.nbh, fld = blk / (a.nbw * a.nbh);
  const int R = a.R;
  // the block's pixels clipped to the field (its bounding box)
  const int h0 = bh * kFitB, w0 = bw * kFitB;
  const int h1 = min(h0 + kFitB, a.H) - 1, w1 = min(w0 + kFitB, a.W) - 1;
  const int ph = h0 + (tid >> 4), pw = w0 + (tid & 15);
  const bool infield = ph <= h1 && pw <= w1;
  const int64_t pix = ((int64_t)fld * a.H + ph) * a.W + pw;
  const bool masked_in = infield && (a.mask == nullptr || a.mask[pix] != 0);
  const bool active = masked_in || (infield && a.rate != nullptr);

  // the normaliser's sums: the workgroups' partial sums in order, times the four quadrants
  if (tid < kFitSums) {
    double s = 0.0;
    for (int k = 0; k < kFitNormBlocks; ++k) s += a.norm_part[k * kFitSums + tid];
    sh.norm[tid] = 4.0 * s;
  }

  int cnt = a.D;
  if (a.counts) cnt = min(max(a.counts[fld], 0), a.D);
  const double ch = (double)ph + 0.5, cw = (double)pw + 0.5;
  double X[kFitSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int base = 0; base < cnt; base += kFitThreads) {
    // stage a chunk: one star per thread, kept if its clipped window meets the block
    const int d = base + tid;
    double sh_h = 0.0, sh_w = 0.0, sh_f = 0.0;
    int fh = 0, fw = 0;
    bool hit = false;
    if (d < cnt) {
      const int64_t s = (int64_t)fld * a.D + d;
      sh_h = (double)a.locs[2 * s];
      sh_w = (double)a.locs[2 * s + 1];
      sh_f = (double)a.fluxes[s];
      fh = (int)fmin(fmax(floor(sh_h), -1.0e6), 1.0e6);
      fw = (int)fmin(fmax(floor(sh_w), -1.0e6), 1.0e6);
      hit = fh + R >= h0 && fh - R <= h1 && fw + R >= w0 && fw - R <= w1;
    }
    const unsigned long long bal = __ballot(hit);
    const int within = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) sh.wcount[wv] = __popcll(bal);
    __syncthreads();  // (also: the previous chunk's stars have been read)
    int off = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kFitWaves; ++k) {
      if (k < wv) off += sh.wcount[k];
      total += sh.wcount[k];
    }
    if (hit) {
      const int slot = off + within;  // < kFitThreads: at most one star per thread
      sh.h[slot] = sh_h;
      sh.w[slot] = sh_w;
      sh.f[slot] = sh_f;
      sh.fh[slot] = fh;
      sh.fw[slot] = fw;
    }
    __syncthreads();
    if (active) {
      for (int s = 0; s < total; ++s) {
        const int sfh = sh.fh[s], sfw = sh.fw[s];
        if ((unsigned)(ph - sfh + R) <= 2u * (unsigned)R &&
            (unsigned)(pw - sfw + R) <= 2u * (unsigned)R) {
          const double dh = ch - sh.h[s], dw = cw - sh.w[s];
          fit_pieces(th, dh * dh + dw * dw, sh.f[s], X);
        }
      }
    }
    __syncthreads();  // wcount and the stars are rewritten by the next chunk
  }
  __syncthreads();  // sh.norm (cnt = 0 passes no barrier above)

  double T[kFitTerms];
#pragma unroll
  for (int k = 0; k < kFitTerms; ++k) T[k] = 0.0;
  if (active) {
    double Nn[kFitSums], Cc[kFitSums], U[kFitSums];
#pragma unroll
    for (int k = 0; k < kFitSums; ++k) Nn[k] = sh.norm[k];
    fit_combine(th, Nn, Cc);
    fit_combine(th, X, U);
    const double ic = 1.0 / Cc[0];
    const double S = cnt > 0 ? U[0] * ic : 0.0;  // no stars: background only, whatever C is
    const double lam = th.bg + th.g * S;
    if (a.rate) a.rate[pix] = (float)lam;
    if (masked_in) {
      // d lambda / d log theta and d v / d log theta, in the order of log_theta
      double L[kFitP], V[kFitP];
      L[0] = th.g * S;
#pragma unroll
      for (int k = 1; k < kFitSums; ++k)
        L[k] = cnt > 0 ? th.g * (U[k] - S * Cc[k]) * ic : 0.0;
      L[7] = 0.0;
      L[8] = 0.0;
      L[9] = th.bg;
      const double v = th.na + th.nm * lam;
#pragma unroll
      for (int k = 0; k < kFitP; ++k) V[k] = th.nm * L[k];
      V[7] = th.nm * lam;
      V[8] = th.na;
      const double iv = 1.0 / v;
      const double r = (double)a.images[pix] - lam;
      T[0] = 0.5 * log(6.283185307179586 * v) + 0.5 * r * r * iv;
      const double dl = -r * iv;                              // d nll / d lambda
      const double dv = 0.5 * iv - 0.5 * r * r * iv * iv;     // d nll / d v
      const double hv = 0.5 * iv * iv;
      int o = 1 + kFitP;
#pragma unroll
      for (int i = 0; i < kFitP; ++i) {
        T[1 + i] = dl * L[i] + dv * V[i];
#pragma unroll
        for (int j = i; j < kFitP; ++j) T[o++] = L[i] * L[j] * iv + V[i] * V[j] * hv;
      }
    }
  }
  // the workgroup's sums: a butterfly per wave, then the four waves in order
#pragma unroll
  for (int k = 0; k < kFitTerms; ++k) {
    const double s = fit_wave_sum(T[k]);
    if (lane == 0) sh.red[wv][k] = s;
  }
  __syncthreads();
  if (tid < kFitTerms)
    a.part[(int64_t)blk * kFitTerms + tid] =
        (sh.red[0][tid] + sh.red[1][tid]) + (sh.red[2][tid] + sh.red[3][tid]);
}

// output o of kFitTerms: nll, grad[0..9], then the information's upper triangle
// row by row; thread t sums the workgroups t, t + 256, ... in order
__global__ __launch_bounds__(kFitThreads) void fit_final_kernel(const double* part, int64_t nblk,
                                                                double* nll, double* grad,
                                                                double* information) {
  __shared__ double sh[kFitWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int o = blockIdx.x;
  double s = 0.0;
  for (int64_t k = tid; k < nblk; k += kFitThreads) s += part[k * kFitTerms + o];
  s = fit_wave_sum(s);
  if (lane == 0) sh[wv] = s;
  __syncthreads();
  if (tid != 0) return;
  const double total = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  if (o == 0) {
    nll[0] = total;
  } else if (o <= kFitP) {
    grad[o - 1] = total;
  } else {
    int i = 0, q = o - 1 - kFitP;  // q-th entry of the upper triangle
    while (q >= kFitP - i) {
      q -= kFitP - i;
      ++i;
    }
    const int j = i + q;
    information[i * kFitP + j] = total;
    information[j * kFitP + i] = total;
  }
}

}  // namespace
}  // namespace smcdet

extern "C" {

int smcdet_fit_objective(const double* log_theta, const float* images, const uint8_t* mask,
                         const float* locs, const float* fluxes, const int32_t* counts,
                         int32_t F, int32_t H, int32_t W, int32_t D, int32_t psf_radius,
                         double* nll, double* grad, double* information, float* rate,
                         double* workspace, int64_t workspace_doubles, void* stream) {
  using namespace smcdet;
  if (F < 1 || H < 1 || W < 1 || D < 0)
    return set_error(SMCDET_EINVAL, "fit_objective: F=%d H=%d W=%d must be >= 1, D=%d >= 0", F, H,
                     W, D);
  if (psf_radius < 0 || psf_radius > 64)
    return set_error(SMCDET_EINVAL, "fit_objective: psf_radius %d outside 0..64", psf_radius);
  if ((int64_t)F * H * W > 0x7fffffffll)
    return set_error(SMCDET_EUNSUPPORTED, "fit_objective: F*H*W = %lld pixels exceed 2^31-1",
                     (long long)F * H * W);
  if ((int64_t)F * D > 0x7fffffffll)
    return set_error(SMCDET_EUNSUPPORTED, "fit_objective: F*D = %lld stars exceed 2^31-1",
                     (long long)F * D);
  const int64_t nblk_check = (int64_t)F * ((H + kFitB - 1) / kFitB) * ((W + kFitB - 1) / kFitB);
  if (nblk_check > SMCDET_FIT_MAX_BLOCKS)
    return set_error(SMCDET_EUNSUPPORTED,
                     "fit_objective: %lld pixel blocks of 16x16 (per field) exceed %d",
                     (long long)nblk_check, SMCDET_FIT_MAX_BLOCKS);
  if (!log_theta || !images || !nll || !grad || !information || !workspace ||
      (D > 0 && (!locs || !fluxes)))
    return set_error(SMCDET_EINVAL, "fit_objective: null buffer");
  for (int k = 0; k < kFitP; ++k)
    if (!std::isfinite(log_theta[k]))
      return set_error(SMCDET_EINVAL, "fit_objective: log_theta[%d] = %g is not finite", k,
                       log_theta[k]);
  const int64_t need = SMCDET_FIT_WORKSPACE_DOUBLES((int64_t)F, H, W);
  if (workspace_doubles < need)
    return set_error(SMCDET_EINVAL,
                     "fit_objective: a workspace of %lld float64 is required, got %lld",
                     (long long)need, (long long)workspace_doubles);
  FitArgs a{};
  FitTheta& th = a.th;
  const double s1 = exp(log_theta[1]), s2 = exp(log_theta[2]), sp = exp(log_theta[3]);
  const double beta = exp(log_theta[4]);
  th.g = exp(log_theta[0]);
  th.b = exp(log_theta[5]);
  th.p0 = exp(log_theta[6]);
  th.nm = exp(log_theta[7]);
  th.na = exp(log_theta[8]);
  th.bg = exp(log_theta[9]);
  th.i2s1 = 1.0 / (2.0 * s1);
  th.i2s2 = 1.0 / (2.0 * s2);
  th.ibs = 1.0 / (beta * sp);
  th.hb = 0.5 * beta;
  th.iz = 1.0 / (1.0 + th.b + th.p0);
  a.images = images;
  a.mask = mask;
  a.locs = locs;
  a.fluxes = fluxes;
  a.counts = counts;
  a.rate = rate;
  a.norm_part = workspace;
  a.part = workspace + kFitNormBlocks * kFitSums;
  a.F = F;
  a.H = H;
  a.W = W;
  a.D = D;
  a.R = psf_radius;
  a.nbh = (H + kFitB - 1) / kFitB;
  a.nbw = (W + kFitB - 1) / kFitB;
  const int64_t nblk = nblk_check;  // <= SMCDET_FIT_MAX_BLOCKS: nblk * 256 threads < 2^32
  hipStream_t st = (hipStream_t)stream;
  launch_sweep(fit_norm_kernel, dim3(kFitNormBlocks), dim3(kFitThreads), 0, st, th, psf_radius,
               a.norm_part);
  launch_sweep(fit_pixel_kernel, dim3((unsigned)nblk), dim3(kFitThreads), 0, st, a);
  launch_sweep(fit_final_kernel, dim3(kFitTerms), dim3(kFitThreads), 0, st,
               (const double*)a.part, nblk, nll, grad, information);
  return check_launch("smcdet_fit_objective");
}

}  // extern "C"
