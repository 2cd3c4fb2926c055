// match_kernel.hip — catalog matching for the evaluation metrics
// (smcdet/metrics.py:8-84, match_catalogs): one wavefront per (tile, sampled
// catalog) assignment problem.
//
// Both catalogs sit one source per lane.  The smaller side supplies the rows
// of a rectangular assignment problem, the larger side the columns (one per
// lane), and the shortest-augmenting-path Hungarian method assigns every row:
// the row being scanned is broadcast with v_readlane, each lane forms its own
// cost on the fly, the minimum over the unscanned columns is a DPP wave
// reduction.  Costs and duals are pairs (k, d) compared lexicographically:
// k = 1, d = 0 for a pair out of tolerance, k = 0, d = distance for one in
// tolerance.  The method only adds, subtracts and takes minima, so it runs
// unchanged over that ordered group and returns the assignment with the
// fewest out-of-tolerance pairs (= the most matches) and, among those, the
// smallest sum of matched distances; no large float penalty is involved.
#include "device.h"

namespace smcdet {
namespace {

constexpr int kMatchWaves = 4;      // problems (waves) per workgroup
constexpr int kBigK = 1 << 28;      // "no value yet" for the integer half of a pair

struct MatchArgs {
  const int32_t* true_counts;
  const float* true_locs;
  const float* true_fluxes;
  const int32_t* est_counts;
  const float* est_locs;
  const float* est_fluxes;
  const int64_t* index;
  const float* mag_bins;
  float* true_total;
  float* true_matches;
  float* est_total;
  float* est_matches;
  int32_t* match_of_true;
  int32_t T, N, M, St, Se, B;
  float locs_tol, mags_tol;
};

// 64-lane minima on DPP, as device.h's wave_max: lanes a control leaves
// without a source read the identity (INT_MAX / +inf as `old`), which lets the
// compiler fuse each step into one v_min_*_dpp
template <int CTRL>
__device__ __forceinline__ int dpp_imin(int v) {
  return __builtin_amdgcn_update_dpp(0x7fffffff, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float dpp_fmin(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(INFINITY), __float_as_int(v),
                                                    CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ int wave_min(int v) {
  v = min(v, dpp_imin<0xb1>(v));
  v = min(v, dpp_imin<0x4e>(v));
  v = min(v, dpp_imin<0x114>(v));
  v = min(v, dpp_imin<0x118>(v));
  v = min(v, dpp_imin<0x142>(v));
  v = min(v, dpp_imin<0x143>(v));
  return readlane(v, 63);
}
__device__ __forceinline__ float wave_min(float v) {
  v = fminf(v, dpp_fmin<0xb1>(v));
  v = fminf(v, dpp_fmin<0x4e>(v));
  v = fminf(v, dpp_fmin<0x114>(v));
  v = fminf(v, dpp_fmin<0x118>(v));
  v = fminf(v, dpp_fmin<0x142>(v));
  v = fminf(v, dpp_fmin<0x143>(v));
  return readlane(v, 63);
}

__device__ __forceinline__ unsigned long long ballot(bool p) {
  return __builtin_amdgcn_ballot_w64(p);
}

// value of lane `src` (per lane; any lane of the wave)
__device__ __forceinline__ int lane_gather(int v, int src) {
  return __builtin_amdgcn_ds_bpermute(src << 2, v);
}
__device__ __forceinline__ float lane_gather(float v, int src) {
  return __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v)));
}

// One source as the matching sees it: ok = finite location and finite positive
// flux (anything else is out of tolerance with everything).
struct Src {
  float x, y, mag;
  int ok;
};

// out of tolerance: the reference's strict `>` on the Euclidean distance and on
// |delta mag| (metrics.py:51-57); dist is the pair's distance
__device__ __forceinline__ bool out_of_tol(const Src& a, const Src& b, float locs_tol,
                                           float mags_tol, float& dist) {
  const float dx = a.x - b.x, dy = a.y - b.y;
  dist = sqrtf(dx * dx + dy * dy);
  return !(a.ok && b.ok) || dist > locs_tol || fabsf(a.mag - b.mag) > mags_tol;
}

__device__ __forceinline__ Src load_src(const float* locs, const float* fluxes, int lane,
                                        int count, float& mag_raw) {
  Src s{0.f, 0.f, 0.f, 0};
  mag_raw = 0.f;
  if (lane < count) {
    const float2 xy = reinterpret_cast<const float2*>(locs)[lane];  // (row h, column w)
    const float x = xy.x, y = xy.y, f = fluxes[lane];
    // utils/sdss.py convert_nmgy_to_mag; NaN for f < 0, +inf for f = 0
    mag_raw = 22.5f - 2.5f * log10f(f);
    if (isfinite(x) && isfinite(y) && isfinite(f) && f > 0.f) s = Src{x, y, mag_raw, 1};
  }
  return s;
}

__global__ __launch_bounds__(kMatchWaves* kWave) void match_kernel(MatchArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t prob = (int64_t)blockIdx.x * kMatchWaves +
                       __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (prob >= (int64_t)a.T * a.M) return;  // wave-uniform
  const int t = (int)(prob / a.M), j = (int)(prob % a.M);
  int64_t e = a.index ? a.index[prob] : (int64_t)j;
  e = e < 0 ? 0 : (e >= a.N ? (int64_t)a.N - 1 : e);  // (the callers validate the index)
  const int64_t te = (int64_t)t * a.N + e;
  const int n = min(max(a.true_counts[t], 0), a.St);
  const int m = min(max(a.est_counts[te], 0), a.Se);

  float tmag_raw, emag_raw;
  const Src ts = load_src(a.true_locs + (int64_t)t * a.St * 2, a.true_fluxes + (int64_t)t * a.St,
                          lane, n, tmag_raw);
  const Src es = load_src(a.est_locs + te * a.Se * 2, a.est_fluxes + te * a.Se, lane, m, emag_raw);

  // rows: the smaller catalog (lane = row), columns: the larger (lane = column)
  const bool rows_true = n <= m;
  const int r = rows_true ? n : m, c = rows_true ? m : n;
  const Src row = rows_true ? ts : es, col = rows_true ? es : ts;
  const bool is_col = lane < c;

  int p = -1;                // column lane: the row assigned to it
  int vk = 0, uk = 0;        // duals, (k, d) pairs: v of this lane's column, u of this lane's row
  float vd = 0.f, ud = 0.f;
  for (int i = 0; i < r; ++i) {
    int mk = kBigK, way = -1;  // per column: least reduced cost seen from the tree, and from where
    float md = 0.f;
    bool used = false, tree = lane == i;
    int j0 = -1, i0 = i;       // j0 = -1: the virtual column holding the new row i
    bool found = false;
    for (int it = 0; it <= c; ++it) {  // (each pass scans one more column: at most c + 1)
      const Src b{readlane(row.x, i0), readlane(row.y, i0), readlane(row.mag, i0),
                  readlane(row.ok, i0)};
      const int buk = readlane(uk, i0);
      const float bud = readlane(ud, i0);
      const bool open = is_col && !used;
      float dist;
      const bool oob = out_of_tol(b, col, a.locs_tol, a.mags_tol, dist);
      const int ck = (oob ? 1 : 0) - buk - vk;
      const float cd = (oob ? 0.f : dist) - bud - vd;
      if (open && (ck < mk || (ck == mk && cd < md))) {
        mk = ck;
        md = cd;
        way = j0;
      }
      // delta = lexicographic minimum over the open columns; ties: the lowest lane
      const int dk = wave_min(open ? mk : kBigK);
      const float dd = wave_min(open && mk == dk ? md : INFINITY);
      const unsigned long long at = ballot(open && mk == dk && md == dd);
      if (at == 0) break;  // (cannot happen while r <= c: an open column always exists)
      if (tree) {
        uk += dk;
        ud += dd;
      }
      if (is_col) {
        if (used) {
          vk -= dk;
          vd -= dd;
        } else {
          mk -= dk;
          md -= dd;
        }
      }
      j0 = __builtin_ctzll(at);
      const int pj = readlane(p, j0);
      if (pj < 0) {
        found = true;
        break;
      }
      used |= lane == j0;
      i0 = pj;
      tree |= lane == i0;
    }
    // augment along the alternating path back to the virtual column
    for (int it = 0; found && it <= r && j0 >= 0; ++it) {
      const int j1 = readlane(way, j0);
      const int pr = j1 >= 0 ? readlane(p, j1) : i;
      if (lane == j0) p = pr;
      j0 = j1;
    }
  }

  // an assigned pair is a match only when it is in tolerance
  const int pc = p < 0 ? 0 : p;
  const Src prow{lane_gather(row.x, pc), lane_gather(row.y, pc), lane_gather(row.mag, pc),
                 lane_gather(row.ok, pc)};
  float dist;
  const int col_match = (is_col && p >= 0 && !out_of_tol(prow, col, a.locs_tol, a.mags_tol, dist))
                            ? p : -1;
  int row_match = -1;  // row lane: its matched column
  for (unsigned long long mm = ballot(col_match >= 0); mm; mm &= mm - 1) {
    const int jc = __builtin_ctzll(mm);
    if (lane == readlane(col_match, jc)) row_match = jc;
  }
  const int true_match = rows_true ? row_match : col_match;  // est slot of this lane's true source
  const int est_match = rows_true ? col_match : row_match;

  // torch.bucketize(mag, mag_bins): the number of edges below mag (NaN: B)
  int tb = 0, eb = 0;
  for (int b = 0; b < a.B; ++b) {
    const float edge = a.mag_bins[b];
    tb += !(edge >= tmag_raw);
    eb += !(edge >= emag_raw);
  }
  float tt = 0.f, tm = 0.f, et = 0.f, em = 0.f;
  for (int b = 0; b < a.B; ++b) {
    const float c0 = (float)__builtin_popcountll(ballot(lane < n && tb == b));
    const float c1 = (float)__builtin_popcountll(ballot(lane < n && tb == b && true_match >= 0));
    const float c2 = (float)__builtin_popcountll(ballot(lane < m && eb == b));
    const float c3 = (float)__builtin_popcountll(ballot(lane < m && eb == b && est_match >= 0));
    if (lane == b) {
      tt = c0;
      tm = c1;
      et = c2;
      em = c3;
    }
  }
  if (lane < a.B) {
    const int64_t o = prob * a.B + lane;
    a.true_total[o] = tt;
    a.true_matches[o] = tm;
    a.est_total[o] = et;
    a.est_matches[o] = em;
  }
  if (a.match_of_true && lane < a.St) a.match_of_true[prob * a.St + lane] = true_match;
}

}  // namespace
}  // namespace smcdet

extern "C" {

int smcdet_match_catalogs(const int32_t* true_counts, const float* true_locs,
                          const float* true_fluxes, const int32_t* est_counts,
                          const float* est_locs, const float* est_fluxes, const int64_t* index,
                          int32_t T, int32_t N, int32_t M, int32_t St, int32_t Se, float locs_tol,
                          float mags_tol, const float* mag_bins, int32_t B, float* true_total,
                          float* true_matches, float* est_total, float* est_matches,
                          int32_t* match_of_true, void* stream) {
  using namespace smcdet;
  if (St < 1 || St > SMCDET_MATCH_MAX_SOURCES || Se < 1 || Se > SMCDET_MATCH_MAX_SOURCES)
    return set_error(SMCDET_EUNSUPPORTED, "match_catalogs: St=%d Se=%d outside 1..%d", St, Se,
                     SMCDET_MATCH_MAX_SOURCES);
  if (B < 1 || B > SMCDET_MATCH_MAX_BINS)
    return set_error(SMCDET_EUNSUPPORTED, "match_catalogs: %d magnitude bins outside 1..%d", B,
                     SMCDET_MATCH_MAX_BINS);
  if (T < 1 || N < 1 || M < 1)
    return set_error(SMCDET_EINVAL, "match_catalogs: T=%d N=%d M=%d must be >= 1", T, N, M);
  if (!(locs_tol > 0.f) || !(mags_tol > 0.f))
    return set_error(SMCDET_EINVAL, "match_catalogs: tolerances %g, %g must be positive",
                     (double)locs_tol, (double)mags_tol);
  if (!index && M != N)
    return set_error(SMCDET_EINVAL, "match_catalogs: index is null, so M = %d must equal N = %d",
                     M, N);
  if (!true_counts || !true_locs || !true_fluxes || !est_counts || !est_locs || !est_fluxes ||
      !mag_bins || !true_total || !true_matches || !est_total || !est_matches)
    return set_error(SMCDET_EINVAL, "match_catalogs: null buffer");
  const int64_t blocks = ((int64_t)T * M + kMatchWaves - 1) / kMatchWaves;
  if (blocks > 0x7fffffffll)
    return set_error(SMCDET_EUNSUPPORTED, "match_catalogs: T*M = %lld problems exceed the grid",
                     (long long)T * M);
  MatchArgs a{true_counts, true_locs, true_fluxes, est_counts, est_locs, est_fluxes, index,
              mag_bins, true_total, true_matches, est_total, est_matches, match_of_true,
              T, N, M, St, Se, B, locs_tol, mags_tol};
  launch_sweep(match_kernel, dim3((unsigned)blocks), dim3(kMatchWaves * kWave), 0,
               (hipStream_t)stream, a);
  return check_launch("smcdet_match_catalogs");
}

}  // extern "C"
