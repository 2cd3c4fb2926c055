// condense_kernel.hip — posterior catalogs condensed into detections
// (DESIGN.md §11): the posterior source-density map, the seeds read off its
// peaks, and the per-seed posterior moments once smcdet_match_catalogs has
// associated every catalog's sources with the seeds.
//
//   source_map_kernel    one workgroup per (tile, chunk of particles): sources
//                        are binned into an LDS copy of the tile's grid with
//                        ds_add_f32, then only the non-zero cells are flushed
//                        as contiguous row segments of global float adds; a
//                        grid too large for LDS adds to global memory directly
//   map_peaks_kernel     one workgroup per tile: box-smoothed map in LDS, a bit
//                        per peak of the non-maximum suppression, K rounds of
//                        block-wide arg-max on the key (value, -index)
//   seed_moments_kernel  one workgroup per tile: every lane owns one seed and a
//                        fixed stride of catalogs, accumulates in float64, and
//                        the lanes of a seed are combined in a fixed order
#include "device.h"

namespace smcdet {
namespace {

constexpr int kCondThreads = 256;
constexpr int kMapChunk = 256;           // least particles per workgroup of the map
constexpr int kMapTargetBlocks = 4096;   // workgroups the map aims for (16 per CU)
constexpr size_t kMapLdsBytes = 160 * 1024;

struct MapArgs {
  const int32_t* counts;
  const float* locs;
  const float* fluxes;
  const float* weights;
  const float* tile_boxes;
  float* count_map;
  float* flux_map;
  float* outside;
  float lo_h, lo_w;
  int32_t N, S, c, Gh, Gw, chunks, chunk_len;
};

// the counted rule of smcdet_match_catalogs (match_kernel.hip load_src)
__device__ __forceinline__ bool counted(float h, float w, float f) {
  return isfinite(h) && isfinite(w) && isfinite(f) && f > 0.f;
}

template <bool LDS>
__global__ __launch_bounds__(kCondThreads) void source_map_kernel(MapArgs a) {
  extern __shared__ float grid[];  // LDS: [cells] counts, then [cells] fluxes
  const int tid = threadIdx.x;
  const int t = blockIdx.x / a.chunks, chunk = blockIdx.x - t * a.chunks;
  const int cells = a.Gh * a.Gw;
  const int nmaps = a.flux_map ? 2 : 1;
  if (LDS) {
    for (int i = tid; i < cells * nmaps; i += kCondThreads) grid[i] = 0.f;
    __syncthreads();
  }
  const float lo_h = a.tile_boxes ? a.tile_boxes[4 * t] : a.lo_h;
  const float lo_w = a.tile_boxes ? a.tile_boxes[4 * t + 1] : a.lo_w;
  const float cf = (float)a.c, gh = (float)a.Gh, gw = (float)a.Gw;
  float* cnt = LDS ? grid : a.count_map + (int64_t)t * cells;
  float* flx = LDS ? grid + cells : (a.flux_map ? a.flux_map + (int64_t)t * cells : nullptr);

  const int64_t tn = (int64_t)t * a.N;
  const int n0 = chunk * a.chunk_len, n1 = min(n0 + a.chunk_len, a.N);
  const float2* locs = reinterpret_cast<const float2*>(a.locs) + tn * a.S;
  const float* fluxes = a.fluxes + tn * a.S;
  float out = 0.f;
  // source i = n * S + j of the tile: consecutive lanes read consecutive sources
  for (int64_t i = (int64_t)n0 * a.S + tid; i < (int64_t)n1 * a.S; i += kCondThreads) {
    const int n = (int)(i / a.S), j = (int)(i - (int64_t)n * a.S);
    if (j >= min(max(a.counts[tn + n], 0), a.S)) continue;
    const float2 hw = locs[i];
    const float f = fluxes[i];
    if (!counted(hw.x, hw.y, f)) continue;
    const float w = a.weights ? a.weights[tn + n] : 1.f;
    const float ih = floorf((hw.x - lo_h) * cf), iw = floorf((hw.y - lo_w) * cf);
    if (ih >= 0.f && ih < gh && iw >= 0.f && iw < gw) {
      const int cell = (int)ih * a.Gw + (int)iw;
      if (LDS) {
        atomicAdd(&cnt[cell], w);
        if (flx) atomicAdd(&flx[cell], w * f);
      } else {
        unsafeAtomicAdd(&cnt[cell], w);
        if (flx) unsafeAtomicAdd(&flx[cell], w * f);
      }
    } else {
      out += w;
    }
  }
  out = wave_sum(out);
  if ((tid & 63) == 0 && out != 0.f) unsafeAtomicAdd(&a.outside[t], out);
  if (LDS) {
    __syncthreads();
    // consecutive lanes flush consecutive cells: row segments of float adds
    for (int i = tid; i < cells * nmaps; i += kCondThreads) {
      const float v = grid[i];
      if (v != 0.f) {
        float* dst = i < cells ? a.count_map + (int64_t)t * cells + i
                               : a.flux_map + (int64_t)t * cells + (i - cells);
        unsafeAtomicAdd(dst, v);
      }
    }
  }
}

struct PeakArgs {
  const float* map;
  const float* tile_boxes;
  const float* min_mass;
  int32_t* n_seeds;
  int32_t* seed_cell;
  float* seed_mass;
  float* seed_locs;
  float lo_h, lo_w;
  int32_t Gh, Gw, c, q, p, K;
};

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned long long o = __shfl_xor(v, m, 64);
    v = o > v ? o : v;
  }
  return v;
}

// LDS: [4] u64 per-wave maxima, [64] int32 chosen cells, [cells] float smoothed
// map, [ceil(cells/32)] u32 peak bits
__host__ __device__ inline size_t peaks_lds_bytes(int cells) {
  return 4 * sizeof(unsigned long long) + 64 * sizeof(int32_t) + (size_t)cells * sizeof(float) +
         (size_t)((cells + 31) / 32) * sizeof(uint32_t);
}

__global__ __launch_bounds__(kCondThreads) void map_peaks_kernel(PeakArgs a) {
  extern __shared__ unsigned long long peaks_lds[];
  unsigned long long* red = peaks_lds;
  int32_t* chosen = reinterpret_cast<int32_t*>(red + 4);
  float* s = reinterpret_cast<float*>(chosen + 64);
  const int cells = a.Gh * a.Gw, words = (cells + 31) / 32;
  uint32_t* bits = reinterpret_cast<uint32_t*>(s + cells);
  const int tid = threadIdx.x, t = blockIdx.x;
  const float* map = a.map + (int64_t)t * cells;
  const float min_mass = a.min_mass[t];

  // s = box sum of the map over (2q+1)^2 cells, zero outside the grid
  for (int x = tid; x < cells; x += kCondThreads) {
    const int i = x / a.Gw, j = x - i * a.Gw;
    const int i0 = max(i - a.q, 0), i1 = min(i + a.q, a.Gh - 1);
    const int j0 = max(j - a.q, 0), j1 = min(j + a.q, a.Gw - 1);
    float v = 0.f;
    for (int ii = i0; ii <= i1; ++ii)
      for (int jj = j0; jj <= j1; ++jj) v += map[ii * a.Gw + jj];
    s[x] = v;
  }
  for (int w = tid; w < words; w += kCondThreads) bits[w] = 0u;
  __syncthreads();

  // peaks: at least min_mass and above every other cell within Chebyshev
  // distance p (equal values: the lower flat index wins)
  for (int x = tid; x < cells; x += kCondThreads) {
    const float v = s[x];
    bool peak = v >= min_mass && v > 0.f;  // an empty cell is never a peak
    if (peak) {
      const int i = x / a.Gw, j = x - i * a.Gw;
      const int i0 = max(i - a.p, 0), i1 = min(i + a.p, a.Gh - 1);
      const int j0 = max(j - a.p, 0), j1 = min(j + a.p, a.Gw - 1);
      for (int ii = i0; ii <= i1 && peak; ++ii)
        for (int jj = j0; jj <= j1; ++jj) {
          const int y = ii * a.Gw + jj;
          const float u = s[y];
          if (y != x && !(v > u || (v == u && x < y))) peak = false;
        }
    }
    if (peak) atomicOr(&bits[x >> 5], 1u << (x & 31));
  }
  __syncthreads();

  // the K largest peaks, one block-wide arg-max each on (value, -index): the
  // float bits of a positive value order as integers, so the pair packs into
  // one u64 (0 = no peak left)
  int ns = 0;
  for (; ns < a.K; ++ns) {
    unsigned long long best = 0;
    for (int w = tid; w < words; w += kCondThreads)
      for (uint32_t m = bits[w]; m; m &= m - 1) {
        const uint32_t x = (uint32_t)w * 32u + (uint32_t)__builtin_ctz(m);
        const float v = s[x];  // > 0
        const unsigned long long key =
            ((unsigned long long)(uint32_t)__float_as_int(v) << 32) | (0xffffffffu - x);
        best = key > best ? key : best;
      }
    best = wave_max_u64(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    best = red[0];
    for (int w = 1; w < kCondThreads / 64; ++w) best = red[w] > best ? red[w] : best;
    if (best == 0) break;  // block-uniform
    const uint32_t x = 0xffffffffu - (uint32_t)(best & 0xffffffffull);
    if (tid == 0) {
      chosen[ns] = (int32_t)x;
      bits[x >> 5] &= ~(1u << (x & 31));
    }
    __syncthreads();
  }
  __syncthreads();

  if (tid == 0) a.n_seeds[t] = ns;
  if (tid < a.K) {
    const int64_t o = (int64_t)t * a.K + tid;
    if (tid < ns) {
      const int x = chosen[tid];
      const int i = x / a.Gw, j = x - i * a.Gw;
      const int i0 = max(i - a.q, 0), i1 = min(i + a.q, a.Gh - 1);
      const int j0 = max(j - a.q, 0), j1 = min(j + a.q, a.Gw - 1);
      // mass-weighted centroid of the raw map over the smoothing window
      double sm = 0.0, sh = 0.0, sw = 0.0;
      for (int ii = i0; ii <= i1; ++ii)
        for (int jj = j0; jj <= j1; ++jj) {
          const double m = (double)map[ii * a.Gw + jj];
          sm += m;
          sh += m * ((double)ii + 0.5);
          sw += m * ((double)jj + 0.5);
        }
      const double lo_h = a.tile_boxes ? (double)a.tile_boxes[4 * t] : (double)a.lo_h;
      const double lo_w = a.tile_boxes ? (double)a.tile_boxes[4 * t + 1] : (double)a.lo_w;
      a.seed_cell[o] = x;
      a.seed_mass[o] = s[x];
      a.seed_locs[2 * o] = (float)(lo_h + (sh / sm) / (double)a.c);
      a.seed_locs[2 * o + 1] = (float)(lo_w + (sw / sm) / (double)a.c);
    } else {
      a.seed_cell[o] = -1;
      a.seed_mass[o] = 0.f;
      a.seed_locs[2 * o] = NAN;
      a.seed_locs[2 * o + 1] = NAN;
    }
  }
}

struct MomentArgs {
  const int32_t* match;
  const float* locs;
  const float* fluxes;
  const float* weights;
  const float* seed_locs;
  double* moments;
  float* matched_flux;
  int32_t N, S, K;
};

__global__ __launch_bounds__(kCondThreads) void seed_moments_kernel(MomentArgs a) {
  __shared__ double part[SMCDET_SEED_MOMENTS][kCondThreads];
  const int tid = threadIdx.x, t = blockIdx.x;
  // lane tid owns seed k and catalogs r, r + R, ...: consecutive lanes read
  // consecutive words of match_of_seed [N,K]
  const int R = kCondThreads / a.K, k = tid % a.K, r = tid / a.K;
  double m[SMCDET_SEED_MOMENTS];
#pragma unroll
  for (int c = 0; c < SMCDET_SEED_MOMENTS; ++c) m[c] = 0.0;
  if (r < R) {
    const int64_t tk = (int64_t)t * a.K + k;
    const double seed_h = (double)a.seed_locs[2 * tk], seed_w = (double)a.seed_locs[2 * tk + 1];
    for (int n = r; n < a.N; n += R) {
      const int64_t tn = (int64_t)t * a.N + n;
      const int slot = a.match[tn * a.K + k];
      float mf = NAN;
      if (slot >= 0 && slot < a.S) {
        const float2 hw = reinterpret_cast<const float2*>(a.locs)[tn * a.S + slot];
        mf = a.fluxes[tn * a.S + slot];
        const double w = a.weights ? (double)a.weights[tn] : 1.0;
        const double dh = (double)hw.x - seed_h, dw = (double)hw.y - seed_w;
        const double f = (double)mf, mag = 22.5 - 2.5 * log10(f);
        m[0] += w;
        m[1] += w * dh;
        m[2] += w * dw;
        m[3] += w * dh * dh;
        m[4] += w * dw * dw;
        m[5] += w * dh * dw;
        m[6] += w * f;
        m[7] += w * f * f;
        m[8] += w * mag;
        m[9] += w * mag * mag;
      }
      if (a.matched_flux) a.matched_flux[tn * a.K + k] = mf;
    }
  }
#pragma unroll
  for (int c = 0; c < SMCDET_SEED_MOMENTS; ++c) part[c][tid] = m[c];
  __syncthreads();
  // the R lanes of a seed, summed in lane order
  for (int o = tid; o < a.K * SMCDET_SEED_MOMENTS; o += kCondThreads) {
    const int kk = o / SMCDET_SEED_MOMENTS, c = o - kk * SMCDET_SEED_MOMENTS;
    double v = 0.0;
    for (int rr = 0; rr < R; ++rr) v += part[c][rr * a.K + kk];
    a.moments[((int64_t)t * a.K + kk) * SMCDET_SEED_MOMENTS + c] = v;
  }
}

// finite with lo < hi (host side)
bool box_ok(const float* b) {
  for (int i = 0; i < 4; ++i)
    if (!(b[i] - b[i] == 0.f)) return false;
  return b[2] > b[0] && b[3] > b[1];
}

}  // namespace
}  // namespace smcdet

extern "C" {

int smcdet_source_map(const int32_t* counts, const float* locs, const float* fluxes,
                      const float* weights, const float* box, const float* tile_boxes, int32_t T,
                      int32_t N, int32_t S, int32_t cells_per_pixel, int32_t Gh, int32_t Gw,
                      float* count_map, float* flux_map, float* outside, void* stream) {
  using namespace smcdet;
  if (cells_per_pixel < 1 || cells_per_pixel > SMCDET_MAP_MAX_CELLS_PER_PIXEL)
    return set_error(SMCDET_EUNSUPPORTED, "source_map: cells_per_pixel = %d outside 1..%d",
                     cells_per_pixel, SMCDET_MAP_MAX_CELLS_PER_PIXEL);
  if (Gh > SMCDET_MAP_MAX_GRID || Gw > SMCDET_MAP_MAX_GRID)
    return set_error(SMCDET_EUNSUPPORTED, "source_map: grid %dx%d above %d cells per side", Gh, Gw,
                     SMCDET_MAP_MAX_GRID);
  if (T < 1 || N < 1 || S < 1 || Gh < 1 || Gw < 1)
    return set_error(SMCDET_EINVAL, "source_map: T=%d N=%d S=%d Gh=%d Gw=%d must be >= 1", T, N, S,
                     Gh, Gw);
  if ((int64_t)N * S > 0x7fffffffll)
    return set_error(SMCDET_EUNSUPPORTED, "source_map: N*S = %lld sources per tile exceed 2^31-1",
                     (long long)N * S);
  if (!counts || !locs || !fluxes || !box || !count_map || !outside)
    return set_error(SMCDET_EINVAL, "source_map: null buffer");
  if (!tile_boxes && !box_ok(box))
    return set_error(SMCDET_EINVAL, "source_map: box (%g, %g, %g, %g) is not lo < hi, finite",
                     (double)box[0], (double)box[1], (double)box[2], (double)box[3]);
  // at least kMapChunk particles per workgroup, about kMapTargetBlocks workgroups
  const int want = (kMapTargetBlocks + T - 1) / T;
  const int per = (N + want - 1) / want, chunk_len = per > kMapChunk ? per : kMapChunk;
  const int chunks = (N + chunk_len - 1) / chunk_len;
  const int64_t blocks = (int64_t)T * chunks;
  if (blocks > 0x7fffffffll)
    return set_error(SMCDET_EUNSUPPORTED, "source_map: T*chunks = %lld exceeds the grid",
                     (long long)blocks);
  const size_t cells = (size_t)Gh * Gw;
  const size_t lds = cells * sizeof(float) * (flux_map ? 2 : 1);
  const bool in_lds = lds <= kMapLdsBytes;
  if (in_lds) {
    const int rc = ensure_lds((const void*)source_map_kernel<true>, lds);
    if (rc != SMCDET_OK) return rc;
  }
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(count_map, 0, (size_t)T * cells * sizeof(float), st) != hipSuccess ||
      hipMemsetAsync(outside, 0, (size_t)T * sizeof(float), st) != hipSuccess ||
      (flux_map &&
       hipMemsetAsync(flux_map, 0, (size_t)T * cells * sizeof(float), st) != hipSuccess))
    return set_error(SMCDET_EHIP, "source_map: hipMemsetAsync failed");
  MapArgs a{counts, locs, fluxes, weights, tile_boxes, count_map, flux_map, outside,
            box[0], box[1], N, S, cells_per_pixel, Gh, Gw, chunks, chunk_len};
  if (in_lds)
    launch_sweep(source_map_kernel<true>, dim3((unsigned)blocks), dim3(kCondThreads), lds, st, a);
  else
    launch_sweep(source_map_kernel<false>, dim3((unsigned)blocks), dim3(kCondThreads), 0, st, a);
  return check_launch("smcdet_source_map");
}

int smcdet_map_peaks(const float* map, const float* box, const float* tile_boxes, int32_t T,
                     int32_t Gh, int32_t Gw, int32_t cells_per_pixel, int32_t smooth_radius,
                     int32_t nms_radius, const float* min_mass, int32_t K, int32_t* n_seeds,
                     int32_t* seed_cell, float* seed_mass, float* seed_locs, void* stream) {
  using namespace smcdet;
  if (K > SMCDET_MATCH_MAX_SOURCES)
    return set_error(SMCDET_EUNSUPPORTED, "map_peaks: K = %d seeds above %d", K,
                     SMCDET_MATCH_MAX_SOURCES);
  if (cells_per_pixel < 1 || cells_per_pixel > SMCDET_MAP_MAX_CELLS_PER_PIXEL)
    return set_error(SMCDET_EUNSUPPORTED, "map_peaks: cells_per_pixel = %d outside 1..%d",
                     cells_per_pixel, SMCDET_MAP_MAX_CELLS_PER_PIXEL);
  if (smooth_radius < 0 || smooth_radius > SMCDET_PEAKS_MAX_SMOOTH || nms_radius < 0 ||
      nms_radius > SMCDET_PEAKS_MAX_NMS)
    return set_error(SMCDET_EUNSUPPORTED,
                     "map_peaks: smooth_radius = %d outside 0..%d or nms_radius = %d outside 0..%d",
                     smooth_radius, SMCDET_PEAKS_MAX_SMOOTH, nms_radius, SMCDET_PEAKS_MAX_NMS);
  if (T < 1 || Gh < 1 || Gw < 1 || K < 1)
    return set_error(SMCDET_EINVAL, "map_peaks: T=%d Gh=%d Gw=%d K=%d must be >= 1", T, Gh, Gw, K);
  if ((int64_t)Gh * Gw > SMCDET_PEAKS_MAX_CELLS)
    return set_error(SMCDET_EUNSUPPORTED,
                     "map_peaks: a %dx%d grid has %lld cells, above the %d whose smoothed map "
                     "fits LDS: use a smaller cells_per_pixel",
                     Gh, Gw, (long long)Gh * Gw, SMCDET_PEAKS_MAX_CELLS);
  if (!map || !box || !min_mass || !n_seeds || !seed_cell || !seed_mass || !seed_locs)
    return set_error(SMCDET_EINVAL, "map_peaks: null buffer");
  if (!tile_boxes && !box_ok(box))
    return set_error(SMCDET_EINVAL, "map_peaks: box (%g, %g, %g, %g) is not lo < hi, finite",
                     (double)box[0], (double)box[1], (double)box[2], (double)box[3]);
  const size_t lds = peaks_lds_bytes(Gh * Gw);
  const int rc = ensure_lds((const void*)map_peaks_kernel, lds);
  if (rc != SMCDET_OK) return rc;
  PeakArgs a{map, tile_boxes, min_mass, n_seeds, seed_cell, seed_mass, seed_locs,
             box[0], box[1], Gh, Gw, cells_per_pixel, smooth_radius, nms_radius, K};
  launch_sweep(map_peaks_kernel, dim3((unsigned)T), dim3(kCondThreads), lds, (hipStream_t)stream,
               a);
  return check_launch("smcdet_map_peaks");
}

int smcdet_seed_moments(const int32_t* match_of_seed, const float* locs, const float* fluxes,
                        const float* weights, const float* seed_locs, int32_t T, int32_t N,
                        int32_t S, int32_t K, double* moments, float* matched_flux,
                        void* stream) {
  using namespace smcdet;
  if (K > SMCDET_MATCH_MAX_SOURCES || S > SMCDET_MATCH_MAX_SOURCES)
    return set_error(SMCDET_EUNSUPPORTED, "seed_moments: K = %d seeds or S = %d slots above %d", K,
                     S, SMCDET_MATCH_MAX_SOURCES);
  if (T < 1 || N < 1 || S < 1 || K < 1)
    return set_error(SMCDET_EINVAL, "seed_moments: T=%d N=%d S=%d K=%d must be >= 1", T, N, S, K);
  if (!match_of_seed || !locs || !fluxes || !seed_locs || !moments)
    return set_error(SMCDET_EINVAL, "seed_moments: null buffer");
  MomentArgs a{match_of_seed, locs, fluxes, weights, seed_locs, moments, matched_flux, N, S, K};
  launch_sweep(seed_moments_kernel, dim3((unsigned)T), dim3(kCondThreads), 0, (hipStream_t)stream,
               a);
  return check_launch("smcdet_seed_moments");
}

}  // extern "C"
