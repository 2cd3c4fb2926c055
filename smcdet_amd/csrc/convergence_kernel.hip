// convergence_kernel.hip — MCMC convergence diagnostics:
// split-R-hat, Geyer's initial-monotone-sequence ESS and the Monte Carlo
// standard error of the mean for rows of chains x [R,C,M].
//
//   chain_stats_kernel   one workgroup (8 waves) per row
//     phase 1  one wave per (split) chain: float64 mean, the centered draws
//              rounded to float32 once into LDS or the global workspace, a_j(0)
//              from the unrounded float64 differences; then W, var+ and R-hat
//     phase 2  kCsPairs lag pairs per block, one pair (rho_2k, rho_2k+1) per
//              wave: lanes stride over i with float64 accumulators, chains in
//              order, one butterfly per lag; after each block every thread
//              applies the stopping rule to the same LDS values, so the exit
//              is workgroup-uniform around the barriers
//
// No atomics: every sum has a fixed order.
#include "device.h"

namespace smcdet {
namespace {

constexpr int kCsThreads = 512;
constexpr int kCsWaves = kCsThreads / 64;
constexpr int kCsPairs = SMCDET_CHAINS_BLOCK_PAIRS;
constexpr int kCsMaxM = 2 * SMCDET_CHAINS_MAX_CHAINS;
static_assert(kCsPairs == kCsWaves, "one lag pair per wave and block");

struct CsArgs {
  const float* x;
  double* mean;
  double* W;
  double* var_plus;
  double* rhat;
  double* tau;
  double* ess;
  double* mcse;
  int32_t* n_pairs;
  int32_t* stopped;
  double* chain_mean;
  double* chain_var;
  float* rho;
  float* workspace;
  int32_t C, M, m, n, split, max_lag, num_rho;
};

// the sum of v over the wave, the same bits in every lane
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// LDS: [kCsMaxM] chain means, [kCsMaxM] a_j(0), [2 * kCsPairs] the block's
// rho, one flag; then (LDS path) the m * n centered draws
struct CsShared {
  double mu[kCsMaxM];
  double a0[kCsMaxM];
  double rho[2 * kCsPairs];
  int bad;
  int pad;
};

template <bool LDS>
__global__ __launch_bounds__(kCsThreads) void chain_stats_kernel(CsArgs a) {
  extern __shared__ double cs_lds[];
  CsShared& sh = *reinterpret_cast<CsShared*>(cs_lds);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t row = blockIdx.x;
  const int m = a.m, n = a.n;
  float* c;
  if (LDS)
    c = reinterpret_cast<float*>(cs_lds + sizeof(CsShared) / sizeof(double));
  else
    c = a.workspace + row * (int64_t)m * n;
  const float* xr = a.x + row * (int64_t)a.C * a.M;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  if (tid == 0) sh.bad = 0;
  __syncthreads();

  // ---- phase 1: per-chain means, centered draws, a_j(0) ----------------------
  for (int j = wv; j < m; j += kCsWaves) {
    const float* xc = a.split ? xr + (int64_t)(j >> 1) * a.M + ((j & 1) ? a.M - n : 0)
                              : xr + (int64_t)j * a.M;
    double s = 0.0;
    bool bad = false;
#pragma unroll 4
    for (int i = lane; i < n; i += 64) {
      const float v = xc[i];
      bad |= !(fabsf(v) <= 3.402823466e38f);  // NaN or +-inf
      s += (double)v;
    }
    if (bad) sh.bad = 1;
    const double mu = wave_sum(s) / (double)n;
    float* cc = c + (int64_t)j * n;
    double q = 0.0;
#pragma unroll 4
    for (int i = lane; i < n; i += 64) {
      const double d = (double)xc[i] - mu;
      cc[i] = (float)d;
      q += d * d;
    }
    q = wave_sum(q);
    if (lane == 0) {
      sh.mu[j] = mu;
      sh.a0[j] = q / (double)n;
    }
  }
  __syncthreads();

  // every thread forms the row's moments from the same LDS values in the same
  // order: the branches below are workgroup-uniform
  const bool bad = sh.bad != 0;
  double smu = 0.0, sa0 = 0.0;
  for (int j = 0; j < m; ++j) {
    smu += sh.mu[j];
    sa0 += sh.a0[j];
  }
  const double dn = (double)n, dm = (double)m;
  const double mean = smu / dm;
  const double W = sa0 / dm * dn / (dn - 1.0);
  double bn = 0.0;
  if (m > 1) {
    for (int j = 0; j < m; ++j) {
      const double d = sh.mu[j] - mean;
      bn += d * d;
    }
    bn /= dm - 1.0;
  }
  const double vp = W * (dn - 1.0) / dn + bn;
  const bool degenerate = bad || !(W > 0.0);

  if (a.chain_mean)
    for (int j = tid; j < m; j += kCsThreads) {
      a.chain_mean[row * m + j] = bad ? nan : sh.mu[j];
      a.chain_var[row * m + j] = bad ? nan : sh.a0[j] * dn / (dn - 1.0);
    }
  // rho past n - 1 (a degenerate row: everywhere) is NaN
  for (int t = tid; t < a.num_rho; t += kCsThreads)
    if (degenerate || t >= n) a.rho[row * a.num_rho + t] = __int_as_float(0x7fc00000);
  if (degenerate) {
    if (tid == 0) {
      a.mean[row] = bad ? nan : mean;
      a.W[row] = bad ? nan : W;
      a.var_plus[row] = bad ? nan : vp;
      a.rhat[row] = nan;
      a.tau[row] = nan;
      a.ess[row] = nan;
      a.mcse[row] = nan;
      a.n_pairs[row] = 0;
      a.stopped[row] = 0;
    }
    return;
  }

  // ---- phase 2: lag pairs in blocks, Geyer's initial monotone sequence -------
  const int lmax = min(n - 1, a.max_lag);
  const int kmax = (lmax + 1) >> 1;          // pairs k with 2k + 1 <= lmax
  const int rho_lags = min(a.num_rho, n);    // lags 0 .. rho_lags - 1 go to rho
  const double inv_mn = 1.0 / (dm * dn);
  int K = 0, stopped = 0;
  bool done = false;
  double psum = 0.0, pmin = 0.0;
  for (int k0 = 0;; k0 += kCsPairs) {
    const bool more_pairs = !done && k0 < kmax;
    if (!more_pairs && 2 * k0 >= rho_lags) break;
    const int k = k0 + wv, t0 = 2 * k, t1 = t0 + 1;
    // this wave's pair is wanted by the sum or by the rho output
    if ((more_pairs && k < kmax) || t0 < rho_lags) {
      double acc0 = 0.0, acc1 = 0.0;
      if (t0 < n) {
        const int n0 = n - t0, n1 = n - t1;  // n1 may be 0: lag t1 = n has no term
        double acc0b = 0.0, acc1b = 0.0;  // a second accumulator per lag: two FMA chains
        for (int j = 0; j < m; ++j) {
          const float* cc = c + (int64_t)j * n;
          int i = lane;
          // four strides at a time while all of them have both lags (n1 < n0): the
          // twelve loads are issued before the first FMA needs one
          for (; i + 192 < n1; i += 256) {
            float u[4], v[4], w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              u[q] = cc[i + 64 * q];
              v[q] = cc[i + 64 * q + t0];
              w[q] = cc[i + 64 * q + t1];
            }
            acc0 = fma((double)u[0], (double)v[0], acc0);
            acc1 = fma((double)u[0], (double)w[0], acc1);
            acc0b = fma((double)u[1], (double)v[1], acc0b);
            acc1b = fma((double)u[1], (double)w[1], acc1b);
            acc0 = fma((double)u[2], (double)v[2], acc0);
            acc1 = fma((double)u[2], (double)w[2], acc1);
            acc0b = fma((double)u[3], (double)v[3], acc0b);
            acc1b = fma((double)u[3], (double)w[3], acc1b);
          }
          for (; i < n0; i += 64) {
            const double u = (double)cc[i];
            acc0 = fma(u, (double)cc[i + t0], acc0);
            if (i < n1) acc1 = fma(u, (double)cc[i + t1], acc1);
          }
        }
        acc0 += acc0b;
        acc1 += acc1b;
      }
      acc0 = wave_sum(acc0);
      acc1 = wave_sum(acc1);
      if (lane == 0) {
        sh.rho[2 * wv] = t0 == 0 ? 1.0 : 1.0 - (W - acc0 * inv_mn) / vp;
        sh.rho[2 * wv + 1] = 1.0 - (W - acc1 * inv_mn) / vp;
      }
    }
    __syncthreads();
    if (tid < 2 * kCsPairs) {
      const int t = 2 * k0 + tid;
      if (t < rho_lags) a.rho[row * a.num_rho + t] = (float)sh.rho[tid];
    }
    if (!done) {
      for (int kk = 0; kk < kCsPairs; ++kk) {
        if (k0 + kk >= kmax) {  // the lags ran out
          done = true;
          break;
        }
        const double P = sh.rho[2 * kk] + sh.rho[2 * kk + 1];
        if (!(P > 0.0)) {
          done = true;
          stopped = 1;
          break;
        }
        pmin = K == 0 ? P : fmin(pmin, P);
        psum += pmin;
        ++K;
      }
    }
    __syncthreads();  // the block's rho have been read
  }

  if (tid == 0) {
    const double floor_tau = 1.0 / log10(dm * dn);
    const double tau = fmax(-1.0 + 2.0 * psum, floor_tau);
    const double ess = dm * dn / tau;
    a.mean[row] = mean;
    a.W[row] = W;
    a.var_plus[row] = vp;
    a.rhat[row] = sqrt(vp / W);
    a.tau[row] = tau;
    a.ess[row] = ess;
    a.mcse[row] = sqrt(vp / ess);
    a.n_pairs[row] = K;
    a.stopped[row] = stopped;
  }
}

// m, n of a (C, M, split) shape after the argument checks; 0 on success
int chain_shape(const char* who, int32_t R, int32_t C, int32_t M, int32_t split, int* m_out,
                int* n_out) {
  if (R < 1 || C < 1 || M < 1)
    return set_error(SMCDET_EINVAL, "%s: R=%d C=%d M=%d must be >= 1", who, R, C, M);
  if (C > SMCDET_CHAINS_MAX_CHAINS)
    return set_error(SMCDET_EUNSUPPORTED, "%s: C = %d chains above %d", who, C,
                     SMCDET_CHAINS_MAX_CHAINS);
  const int m = split ? 2 * C : C, n = split ? M / 2 : M;
  if (n < 4)
    return set_error(SMCDET_EINVAL, "%s: n = %d draws per %schain, at least 4 are needed", who, n,
                     split ? "split " : "");
  if ((int64_t)m * n > SMCDET_CHAINS_MAX_DRAWS)
    return set_error(SMCDET_EUNSUPPORTED, "%s: m*n = %lld draws per row above %d", who,
                     (long long)m * n, SMCDET_CHAINS_MAX_DRAWS);
  if ((int64_t)R * m > 0x7fffffffll)
    return set_error(SMCDET_EUNSUPPORTED, "%s: R*m = %lld chains exceed 2^31-1", who,
                     (long long)R * m);
  *m_out = m;
  *n_out = n;
  return SMCDET_OK;
}

}  // namespace
}  // namespace smcdet

extern "C" {

int64_t smcdet_chain_stats_workspace(int32_t R, int32_t C, int32_t M, int32_t split) {
  using namespace smcdet;
  int m, n;
  const int rc = chain_shape("chain_stats_workspace", R, C, M, split, &m, &n);
  if (rc != SMCDET_OK) return rc;
  return (int64_t)m * n <= SMCDET_CHAINS_LDS_DRAWS ? 0 : (int64_t)R * m * n;
}

int smcdet_chain_stats(const float* x, int32_t R, int32_t C, int32_t M, int32_t split,
                       int32_t max_lag, int32_t num_rho, double* mean, double* W,
                       double* var_plus, double* rhat, double* tau, double* ess, double* mcse,
                       int32_t* n_pairs, int32_t* stopped, double* chain_mean, double* chain_var,
                       float* rho, float* workspace, int64_t workspace_floats, void* stream) {
  using namespace smcdet;
  int m, n;
  const int rc = chain_shape("chain_stats", R, C, M, split, &m, &n);
  if (rc != SMCDET_OK) return rc;
  if (num_rho > SMCDET_CHAINS_MAX_RHO)
    return set_error(SMCDET_EUNSUPPORTED, "chain_stats: num_rho = %d autocorrelations above %d",
                     num_rho, SMCDET_CHAINS_MAX_RHO);
  if (max_lag < 1 || num_rho < 0)
    return set_error(SMCDET_EINVAL, "chain_stats: max_lag = %d must be >= 1, num_rho = %d >= 0",
                     max_lag, num_rho);
  if (!x || !mean || !W || !var_plus || !rhat || !tau || !ess || !mcse || !n_pairs || !stopped ||
      (num_rho > 0 && !rho) || (chain_mean == nullptr) != (chain_var == nullptr))
    return set_error(SMCDET_EINVAL, "chain_stats: null buffer");
  const bool lds_path = (int64_t)m * n <= SMCDET_CHAINS_LDS_DRAWS;
  const int64_t need = lds_path ? 0 : (int64_t)R * m * n;
  if (need > 0 && (!workspace || workspace_floats < need))
    return set_error(SMCDET_EINVAL,
                     "chain_stats: a workspace of %lld floats is required (m*n = %lld draws per "
                     "row above the %d kept in LDS), got %lld",
                     (long long)need, (long long)m * n, SMCDET_CHAINS_LDS_DRAWS,
                     workspace ? (long long)workspace_floats : 0ll);
  CsArgs a{};
  a.x = x;
  a.mean = mean;
  a.W = W;
  a.var_plus = var_plus;
  a.rhat = rhat;
  a.tau = tau;
  a.ess = ess;
  a.mcse = mcse;
  a.n_pairs = n_pairs;
  a.stopped = stopped;
  a.chain_mean = chain_mean;
  a.chain_var = chain_var;
  a.rho = rho;
  a.workspace = workspace;
  a.C = C;
  a.M = M;
  a.m = m;
  a.n = n;
  a.split = split != 0;
  a.max_lag = max_lag;
  a.num_rho = num_rho;
  const size_t lds = sizeof(CsShared) + (lds_path ? (size_t)m * n * sizeof(float) : 0);
  if (lds_path) {
    const int rl = ensure_lds((const void*)chain_stats_kernel<true>, lds);
    if (rl != SMCDET_OK) return rl;
    launch_sweep(chain_stats_kernel<true>, dim3((unsigned)R), dim3(kCsThreads), lds,
                 (hipStream_t)stream, a);
  } else {
    launch_sweep(chain_stats_kernel<false>, dim3((unsigned)R), dim3(kCsThreads), lds,
                 (hipStream_t)stream, a);
  }
  return check_launch("smcdet_chain_stats");
}

}  // extern "C"
