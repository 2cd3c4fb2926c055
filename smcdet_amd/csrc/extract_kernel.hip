// extract_kernel.hip — the classical baseline of the reference's experiment
// scripts (experiments/*/run_sep.py): a multi-threshold detector "after
// SExtractor / SEP", one wavefront per (image, setting) problem.  The
// algorithm is this project's own definition (include/smcdet_hip.h,
// smcdet_extract); it does not claim parity with sep.
//
// A problem lives in one per-wave LDS slab: the detection values, five int16
// label planes and the float32 threshold ladder per pixel, and after the
// deblending the float64 object table in the ladder's place.  Pixels sit on
// the lanes, pixel p on lane p % 64 (one per lane up to 64 pixels, strided
// above).  Every loop that ends on data ends on a ballot, so the trip counts
// are wave-uniform; nothing is atomic and nothing leaves the slab before the
// outputs, so a problem gives the same bits on every run and in every launch.
//
// Labelling is propagation of the smallest flat pixel index over the eight
// neighbours, in place, with one pointer jump (label <- label of label) per
// pixel and sweep; the fixed point is the component's smallest index however
// the sweeps interleave.
#include "device.h"

namespace smcdet {
namespace {

constexpr int kSmallPix = 64, kSmallObj = 32, kSmallWaves = 4;  // H*W <= 64: one pixel per lane
constexpr int kBigPix = SMCDET_EXTRACT_MAX_PIXELS, kBigObj = 512, kBigWaves = 1;

// columns of the object table
enum { cF = 0, cH, cW, cA, cChh, cCww, cChw, cAlpha, cMth, kCols };

struct ExtractArgs {
  const float* images;
  const float* background;
  const float* sigma;
  const float* thresh;
  const int32_t* minarea;
  const float* deblend_cont;
  const float* clean_param;
  int32_t* counts;
  float* locs;
  float* fluxes;
  int32_t* n_found;
  int32_t* segmap;
  int32_t T, H, W, G, nlevels, nsqrt, K;
};

// MAXOBJ >= ceil(H/2) * ceil(W/2) for every H*W <= NPIX: leaves are pairwise
// non-adjacent, so a problem cannot hold more objects
template <int NPIX, int MAXOBJ>
struct Slab {
  union {
    struct {
      double froot[NPIX];  // F_root, at the root's smallest pixel
      float thr[NPIX];     // tau_k of the pixel's root
      float q[NPIX];       // ladder ratio of the pixel's root
    } d;
    double tab[kCols][MAXOBJ];  // object statistics (after the deblending)
  } u;
  float v[NPIX];
  // label planes; their later uses are named where they change hands
  short root[NPIX], node[NPIX], lab[NPIX], obj[NPIX], flag[NPIX];
  unsigned char nb[NPIX];  // which of the 8 neighbours exist
};
static_assert(sizeof(Slab<kSmallPix, kSmallObj>) * kSmallWaves <= 65536, "LDS");
static_assert(sizeof(Slab<kBigPix, kBigObj>) * kBigWaves <= 65536, "LDS");
static_assert(2 * kSmallObj <= kSmallPix && 2 * kBigObj <= kBigPix,
              "the int16 object tables reuse label planes");

__device__ __forceinline__ unsigned long long ballot(bool p) {
  return __builtin_amdgcn_ballot_w64(p);
}
template <int CTRL>
__device__ __forceinline__ int dpp_imin(int v) {
  return __builtin_amdgcn_update_dpp(0x7fffffff, v, CTRL, 0xf, 0xf, false);
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

// neighbour d of pixel p (bit d of nb[p]): row above, same row, row below
__device__ __forceinline__ int nb_offset(int d, int W) {
  return d < 3 ? d - 1 - W : d == 3 ? -1 : d == 4 ? 1 : d - 6 + W;
}

// lab >= 0 marks the set; on return lab[p] is the smallest flat index of p's
// 8-connected component of the set
template <int PPL>
__device__ __forceinline__ void label_components(short* lab, const unsigned char* nb, int HW,
                                                 int W, int lane) {
  wave_sync();
  for (int it = 0; it < 64 * PPL + 2; ++it) {  // (a sweep that changes nothing ends it sooner)
    bool changed = false;
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      if (p < HW) {
        const int m0 = lab[p];
        if (m0 >= 0) {
          int m = m0;
          const int mask = nb[p];
#pragma unroll
          for (int d = 0; d < 8; ++d) {
            if (mask & (1 << d)) {
              const int x = lab[p + nb_offset(d, W)];
              if (x >= 0 && x < m) m = x;
            }
          }
          const int x = lab[m];  // m is a pixel of this component: lab[m] >= 0
          if (x < m) m = x;
          if (m < m0) {
            lab[p] = (short)m;
            changed = true;
          }
        }
      }
    }
    wave_sync();
    if (!ballot(changed)) break;
  }
}

// order[r] = the alive object of rank r by descending F, ties to the smaller
// smallest pixel; returns the number of alive objects.  Object o sits on lane
// o % 64.
template <int OC>
__device__ __forceinline__ int rank_objects(const double* F, const short* minidx,
                                            const short* into, short* order, int nobj, int lane) {
  double Fo[OC];
  int mo[OC], rk[OC];
  bool alive[OC];
#pragma unroll
  for (int c = 0; c < OC; ++c) {
    const int o = lane + 64 * c;
    alive[c] = o < nobj && into[o] == o;
    Fo[c] = alive[c] ? F[o] : 0.0;
    mo[c] = alive[c] ? minidx[o] : 0;
    rk[c] = 0;
  }
  for (int j = 0; j < nobj; ++j) {
    if (into[j] != j) continue;  // wave-uniform
    const double Fj = F[j];
    const int mj = minidx[j];
#pragma unroll
    for (int c = 0; c < OC; ++c) rk[c] += (Fj > Fo[c] || (Fj == Fo[c] && mj < mo[c])) ? 1 : 0;
  }
  int n = 0;
#pragma unroll
  for (int c = 0; c < OC; ++c) {
    if (alive[c]) order[min(rk[c], nobj - 1)] = (short)(lane + 64 * c);
    n += __builtin_popcountll(ballot(alive[c]));
  }
  wave_sync();
  return n;
}

template <int NPIX, int MAXOBJ, int WAVES>
__global__ __launch_bounds__(WAVES* kWave) void extract_kernel(ExtractArgs a) {
  constexpr int PPL = NPIX / 64;
  constexpr int OC = (MAXOBJ + 63) / 64;
  __shared__ Slab<NPIX, MAXOBJ> slabs[WAVES];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t prob = (int64_t)blockIdx.x * WAVES + wv;  // g fastest: neighbours share the image
  if (prob >= (int64_t)a.T * a.G) return;  // wave-uniform; there is no workgroup barrier below
  Slab<NPIX, MAXOBJ>& s = slabs[wv];
  const int t = (int)(prob / a.G), g = (int)(prob % a.G);
  const int W = a.W, HW = a.H * a.W;

  const float tau = a.thresh[g] * a.sigma[t];
  const float bg = a.background[t];
  const int minarea = a.minarea[g];
  const double cont = (double)a.deblend_cont[g];
  const double beta = (double)a.clean_param[g];
  const bool live = isfinite(tau) && tau > 0.f;

  // ---- detection values and the pixels above tau ----------------------------
  const float* img = a.images + (int64_t)t * HW;
#pragma unroll 1
  for (int c = 0; c < PPL; ++c) {
    const int p = lane + 64 * c;
    if (p < HW) {
      const float x = img[p] - bg;
      const int i = p / W, j = p - i * W;
      const bool up = i > 0, dn = i < a.H - 1, lf = j > 0, rt = j < W - 1;
      s.v[p] = x;
      s.nb[p] = (unsigned char)((up && lf) | (up << 1) | ((up && rt) << 2) | (lf << 3) | (rt << 4) |
                                ((dn && lf) << 5) | (dn << 6) | ((dn && rt) << 7));
      s.lab[p] = (live && x > tau) ? (short)p : (short)-1;  // (a NaN is above nothing)
      s.obj[p] = -1;
      s.node[p] = -1;
    }
  }
  label_components<PPL>(s.lab, s.nb, HW, W, lane);
#pragma unroll 1
  for (int c = 0; c < PPL; ++c) {
    const int p = lane + 64 * c;
    if (p < HW) s.root[p] = s.lab[p];
  }
  wave_sync();

  // ---- roots: drop the small ones, set up the ladder of the others ------------
#pragma unroll 1
  for (int c = 0; c < PPL; ++c) {
    const int p = lane + 64 * c;
    unsigned long long heads = ballot(p < HW && s.root[p] == p);
    while (heads) {
      const int r = __builtin_ctzll(heads) + 64 * c;
      heads &= heads - 1;
      int cnt = 0;
      float pk = -INFINITY;
      double F = 0.0;
#pragma unroll 1
      for (int c2 = 0; c2 < PPL; ++c2) {
        const int p2 = lane + 64 * c2;
        const bool in = p2 < HW && s.root[p2] == r;
        cnt += __builtin_popcountll(ballot(in));
        if (in) {
          const float x = s.v[p2];
          pk = fmaxf(pk, x);
          F += (double)x;
        }
      }
      pk = wave_max(pk);
      F = wave_sum(F);
      float q = pk / tau;
      for (int i = 0; i < a.nsqrt; ++i) q = sqrtf(q);
#pragma unroll 1
      for (int c2 = 0; c2 < PPL; ++c2) {
        const int p2 = lane + 64 * c2;
        if (p2 < HW && s.root[p2] == r) {
          if (cnt < minarea) {
            s.root[p2] = -1;
          } else {
            s.u.d.thr[p2] = tau;
            s.u.d.q[p2] = q;
            s.node[p2] = (short)r;
          }
        }
      }
      if (lane == 0) s.u.d.froot[r] = F;
      wave_sync();
    }
  }

  // ---- the significant tree, level by level -----------------------------------
  // node[p]: the significant node of the previous level that holds p (its
  // smallest pixel), -1 once p's node is a leaf or p fell out of the tree.
  // Nodes of one level are pairwise non-adjacent, so the components of the
  // pixels above their own root's tau_k are the children.
  for (int k = 1; k < a.nlevels; ++k) {
    bool act = false, drop = false;
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      if (p < HW) {
        const int nd = s.node[p];
        short l = -1;
        if (nd >= 0) {
          act = true;
          const float th = s.u.d.thr[p] * s.u.d.q[p];
          s.u.d.thr[p] = th;
          if (s.v[p] > th) l = (short)nd; else drop = true;
        }
        s.lab[p] = l;
      }
    }
    if (!ballot(act)) break;
    // is the component labelled h (its smallest pixel) significant at this level?
    auto significant = [&](int h) {
      double ex = 0.0;
#pragma unroll 1
      for (int c2 = 0; c2 < PPL; ++c2) {
        const int p2 = lane + 64 * c2;
        if (p2 < HW && s.lab[p2] == h) ex += (double)s.v[p2] - (double)s.u.d.thr[p2];
      }
      return wave_sum(ex) > cont * s.u.d.froot[s.root[h]];
    };
    if (!ballot(drop)) {
      // every node kept all its pixels, so each node is its own only child (lab
      // = node): no relabelling, and a child that is no longer significant
      // makes its node a leaf
      wave_sync();
#pragma unroll 1
      for (int c = 0; c < PPL; ++c) {
        const int p = lane + 64 * c;
        unsigned long long heads = ballot(p < HW && s.lab[p] == p);
        while (heads) {
          const int h = __builtin_ctzll(heads) + 64 * c;
          heads &= heads - 1;
          if (!significant(h)) {  // wave-uniform
#pragma unroll 1
            for (int c2 = 0; c2 < PPL; ++c2) {
              const int p2 = lane + 64 * c2;
              if (p2 < HW && s.lab[p2] == h) {
                s.obj[p2] = (short)h;
                s.node[p2] = -1;
              }
            }
          }
        }
      }
      wave_sync();
      continue;
    }
    // the pixel set changed: label it again
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      if (p < HW) {
        if (s.lab[p] >= 0) s.lab[p] = (short)p;
        s.flag[p] = 0;
      }
    }
    label_components<PPL>(s.lab, s.nb, HW, W, lane);
    // flag bit 0 at a child's smallest pixel: significant; bit 1 at a node's:
    // it has a significant child
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      unsigned long long heads = ballot(p < HW && s.lab[p] == p);
      while (heads) {
        const int h = __builtin_ctzll(heads) + 64 * c;
        heads &= heads - 1;
        const int parent = s.node[h];
        if (significant(h) && lane == 0) {
          s.flag[h] |= 1;
          s.flag[parent] |= 2;
        }
      }
    }
    wave_sync();
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      if (p < HW) {
        const int nd = s.node[p];
        if (nd >= 0) {
          const int cl = s.lab[p];
          if (cl >= 0 && (s.flag[cl] & 1)) {
            s.node[p] = (short)cl;
          } else {
            if (!(s.flag[nd] & 2)) s.obj[p] = (short)nd;  // no significant child: a leaf
            s.node[p] = -1;
          }
        }
      }
    }
    wave_sync();
  }
#pragma unroll 1
  for (int c = 0; c < PPL; ++c) {
    const int p = lane + 64 * c;
    if (p < HW && s.node[p] >= 0) s.obj[p] = s.node[p];  // the last level's nodes are leaves
  }
  wave_sync();

  // ---- gather: synchronous sweeps (read obj, write lab, copy back) ------------
  // A root with one leaf ends up whole under that leaf's label, which is what
  // the definition asks of a chain.
  {
    bool un = false;
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      un |= p < HW && s.root[p] >= 0 && s.obj[p] < 0;
    }
    for (int it = 0; it < NPIX && ballot(un); ++it) {
      un = false;
#pragma unroll 1
      for (int c = 0; c < PPL; ++c) {
        const int p = lane + 64 * c;
        if (p < HW) {
          int o = s.obj[p];
          if (o < 0 && s.root[p] >= 0) {
            float bv = 0.f;
            const int mask = s.nb[p];
#pragma unroll
            for (int d = 0; d < 8; ++d) {
              if (mask & (1 << d)) {
                const int pn = p + nb_offset(d, W);
                const int x = s.obj[pn];
                if (x >= 0) {
                  const float vn = s.v[pn];
                  if (o < 0 || vn > bv || (vn == bv && x < o)) {
                    bv = vn;
                    o = x;
                  }
                }
              }
            }
            un |= o < 0;
          }
          s.lab[p] = (short)o;
        }
      }
      wave_sync();
#pragma unroll 1
      for (int c = 0; c < PPL; ++c) {
        const int p = lane + 64 * c;
        if (p < HW) s.obj[p] = s.lab[p];
      }
      wave_sync();
    }
  }

  // ---- objects: number them by their leaf's smallest pixel ----------------------
  int nobj = 0;
#pragma unroll 1
  for (int c = 0; c < PPL; ++c) {
    const int p = lane + 64 * c;
    const bool head = p < HW && s.obj[p] == p;
    const unsigned long long m = ballot(head);
    if (head) s.flag[p] = (short)(nobj + __builtin_popcountll(m & ((1ull << lane) - 1)));
    nobj += __builtin_popcountll(m);
  }
  wave_sync();
#pragma unroll 1
  for (int c = 0; c < PPL; ++c) {
    const int p = lane + 64 * c;
    if (p < HW) {
      const int o = s.obj[p];
      const int id = o >= 0 ? (int)s.flag[o] : -1;
      s.node[p] = (short)(id < MAXOBJ ? id : -1);  // (id < MAXOBJ always: see Slab)
    }
  }
  nobj = min(nobj, MAXOBJ);
  wave_sync();
  // from here: node = object of the pixel, lab = its row, flag = its column;
  // root and obj hold the int16 object tables
  short* const npix = s.root;
  short* const order = s.root + MAXOBJ;
  short* const minidx = s.obj;
  short* const into = s.obj + MAXOBJ;
#pragma unroll 1
  for (int c = 0; c < PPL; ++c) {
    const int p = lane + 64 * c;
    if (p < HW) {
      const int i = p / W;
      s.lab[p] = (short)i;
      s.flag[p] = (short)(p - i * W);
    }
  }
  wave_sync();

  // ---- object statistics, float64 -------------------------------------------------
  const double U = 100.0 * 3.14159265358979323846;
  const double taud = (double)tau;
  for (int o = 0; o < nobj; ++o) {
    double F = 0.0, Sh = 0.0, Sw = 0.0, Shh = 0.0, Sww = 0.0, Shw = 0.0;
    int np = 0, mi = 0x7fff;
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      const bool in = p < HW && s.node[p] == o;
      np += __builtin_popcountll(ballot(in));
      if (in) {
        const double x = (double)s.v[p], h = s.lab[p] + 0.5, w = s.flag[p] + 0.5;
        F += x;
        Sh += x * h;
        Sw += x * w;
        Shh += x * h * h;
        Sww += x * w * w;
        Shw += x * h * w;
        mi = min(mi, p);
      }
    }
    F = wave_sum(F);
    Sh = wave_sum(Sh);
    Sw = wave_sum(Sw);
    Shh = wave_sum(Shh);
    Sww = wave_sum(Sww);
    Shw = wave_sum(Shw);
    mi = wave_min(mi);
    const double hb = Sh / F, wb = Sw / F;
    double hh = Shh / F - hb * hb, ww = Sww / F - wb * wb;
    const double hw = Shw / F - hb * wb;
    if (hh * ww - hw * hw < 1.0 / 144.0) {
      hh += 1.0 / 12.0;
      ww += 1.0 / 12.0;
    }
    const double det = hh * ww - hw * hw;
    const double hd = 0.5 * (hh - ww);
    const double aa = sqrt(0.5 * (hh + ww) + sqrt(hd * hd + hw * hw));
    double mth = 0.0, alpha = 0.0;
    if (beta > 0.0) {  // wave-uniform
      if (np >= minarea) {
        // the minarea-th largest v: v > tau > 0, so the bit patterns order as the values
        unsigned int x = 0;
        for (int bit = 30; bit >= 0; --bit) {
          const unsigned int trial = x | (1u << bit);
          int ge = 0;
#pragma unroll 1
          for (int c = 0; c < PPL; ++c) {
            const int p = lane + 64 * c;
            ge += __builtin_popcountll(
                ballot(p < HW && s.node[p] == o && __float_as_uint(s.v[p]) >= trial));
          }
          if (ge >= minarea) x = trial;
        }
        mth = (double)__uint_as_float(x) - taud;
      }
      const double amp = F / (2.0 * U);
      alpha = (pow(amp / taud, 1.0 / beta) - 1.0) * U / (double)np;
    }
    if (lane == 0) {
      s.u.tab[cF][o] = F;
      s.u.tab[cH][o] = hb;
      s.u.tab[cW][o] = wb;
      s.u.tab[cA][o] = aa;
      s.u.tab[cChh][o] = ww / det;
      s.u.tab[cCww][o] = hh / det;
      s.u.tab[cChw][o] = -2.0 * hw / det;
      s.u.tab[cAlpha][o] = alpha;
      s.u.tab[cMth][o] = mth;
      npix[o] = (short)np;
      minidx[o] = (short)mi;
      into[o] = (short)o;
    }
  }
  wave_sync();
  int nfound = rank_objects<OC>(s.u.tab[cF], minidx, into, order, nobj, lane);

  // ---- clean: every absorber is judged by its original statistics ---------------
  bool absorbed = false;
  if (beta > 0.0) {
    for (int r = 1; r < nobj; ++r) {
      const int i = order[r];
      const double hi = s.u.tab[cH][i], wi = s.u.tab[cW][i], ai = s.u.tab[cA][i];
      const double mthi = s.u.tab[cMth][i];
      int jstar = -1;
      for (int c = 0; 64 * c < r && jstar < 0; ++c) {
        const int rr = lane + 64 * c;
        bool hit = false;
        if (rr < r) {
          const int j = order[rr];
          if (into[j] == j) {
            const double dh = hi - s.u.tab[cH][j], dw = wi - s.u.tab[cW][j];
            const double sa = ai + s.u.tab[cA][j];
            const double amp = s.u.tab[cF][j] / (2.0 * U);
            if (dh * dh + dw * dw < 100.0 * sa * sa && amp > taud) {
              const double val = 1.0 + s.u.tab[cAlpha][j] * (s.u.tab[cChh][j] * dh * dh +
                                                             s.u.tab[cCww][j] * dw * dw +
                                                             s.u.tab[cChw][j] * dh * dw);
              if (val > 1.0 && val < 1e10) hit = amp * pow(val, -beta) > mthi;
            }
          }
        }
        const unsigned long long m = ballot(hit);
        if (m) jstar = order[__builtin_ctzll(m) + 64 * c];
      }
      if (jstar >= 0) {
        if (lane == 0) into[i] = (short)jstar;
        absorbed = true;
        wave_sync();
      }
    }
  }
  if (absorbed) {  // wave-uniform: the survivors' sums over their final pixel sets
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      if (p < HW && s.node[p] >= 0) s.node[p] = into[s.node[p]];
    }
    wave_sync();
    for (int o = 0; o < nobj; ++o) {
      if (into[o] != o) continue;  // wave-uniform
      double F = 0.0, Sh = 0.0, Sw = 0.0;
      int mi = 0x7fff;
#pragma unroll 1
      for (int c = 0; c < PPL; ++c) {
        const int p = lane + 64 * c;
        if (p < HW && s.node[p] == o) {
          const double x = (double)s.v[p];
          F += x;
          Sh += x * (s.lab[p] + 0.5);
          Sw += x * (s.flag[p] + 0.5);
          mi = min(mi, p);
        }
      }
      F = wave_sum(F);
      Sh = wave_sum(Sh);
      Sw = wave_sum(Sw);
      mi = wave_min(mi);
      if (lane == 0) {
        s.u.tab[cF][o] = F;
        s.u.tab[cH][o] = Sh / F;
        s.u.tab[cW][o] = Sw / F;
        minidx[o] = (short)mi;
      }
    }
    wave_sync();
    nfound = rank_objects<OC>(s.u.tab[cF], minidx, into, order, nobj, lane);
  }

  // ---- outputs ----------------------------------------------------------------------
  const int kept = min(nfound, a.K);
  if (lane == 0) {
    a.counts[prob] = kept;
    if (a.n_found) a.n_found[prob] = nfound;
  }
  if (lane < a.K) {  // K <= 64
    float f = 0.f, lh = NAN, lw = NAN;
    if (lane < kept) {
      const int o = order[lane];
      f = (float)s.u.tab[cF][o];
      lh = (float)s.u.tab[cH][o];
      lw = (float)s.u.tab[cW][o];
    }
    a.fluxes[prob * a.K + lane] = f;
    reinterpret_cast<float2*>(a.locs)[prob * a.K + lane] = make_float2(lh, lw);
  }
  if (a.segmap) {
    short* const rankof = s.lab;  // (the rows are done with)
    wave_sync();
    for (int r = lane; r < nfound; r += 64) rankof[order[r]] = (short)r;
    wave_sync();
    int32_t* seg = a.segmap + prob * HW;
#pragma unroll 1
    for (int c = 0; c < PPL; ++c) {
      const int p = lane + 64 * c;
      if (p < HW) {
        const int o = s.node[p];
        seg[p] = o >= 0 ? rankof[o] + 1 : 0;
      }
    }
  }
}

}  // namespace
}  // namespace smcdet

extern "C" {

int smcdet_extract(const float* images, const float* background, const float* sigma, int32_t T,
                   int32_t H, int32_t W, const float* thresh, const int32_t* minarea,
                   const float* deblend_cont, const float* clean_param, int32_t G,
                   int32_t deblend_nthresh, int32_t K, int32_t* counts, float* locs,
                   float* fluxes, int32_t* n_found, int32_t* segmap, void* stream) {
  using namespace smcdet;
  if (T < 1 || H < 1 || W < 1 || G < 1 || K < 1 || deblend_nthresh < 1)
    return set_error(SMCDET_EINVAL, "extract: T=%d H=%d W=%d G=%d K=%d deblend_nthresh=%d must be "
                     ">= 1", T, H, W, G, K, deblend_nthresh);
  if (!images || !background || !sigma || !thresh || !minarea || !deblend_cont || !clean_param ||
      !counts || !locs || !fluxes)
    return set_error(SMCDET_EINVAL, "extract: null buffer");
  if ((int64_t)H * W > SMCDET_EXTRACT_MAX_PIXELS)
    return set_error(SMCDET_EUNSUPPORTED, "extract: a %dx%d image has more than %d pixels", H, W,
                     SMCDET_EXTRACT_MAX_PIXELS);
  if (K > SMCDET_MATCH_MAX_SOURCES)
    return set_error(SMCDET_EUNSUPPORTED, "extract: K=%d above %d", K, SMCDET_MATCH_MAX_SOURCES);
  if (deblend_nthresh > 64 || (deblend_nthresh & (deblend_nthresh - 1)))
    return set_error(SMCDET_EUNSUPPORTED, "extract: deblend_nthresh=%d is not a power of two in "
                     "1..64", deblend_nthresh);
  const int64_t probs = (int64_t)T * G;
  if (probs > 0x7fffffffll)
    return set_error(SMCDET_EUNSUPPORTED, "extract: T*G = %lld problems exceed the grid",
                     (long long)probs);
  int nsqrt = 0;
  while ((1 << nsqrt) < deblend_nthresh) ++nsqrt;
  ExtractArgs a{images, background, sigma, thresh, minarea, deblend_cont, clean_param, counts,
                locs, fluxes, n_found, segmap, T, H, W, G, deblend_nthresh, nsqrt, K};
  if (H * W <= kSmallPix) {
    const int64_t blocks = (probs + kSmallWaves - 1) / kSmallWaves;
    launch_sweep(extract_kernel<kSmallPix, kSmallObj, kSmallWaves>, dim3((unsigned)blocks),
                 dim3(kSmallWaves * kWave), 0, (hipStream_t)stream, a);
  } else {
    launch_sweep(extract_kernel<kBigPix, kBigObj, kBigWaves>, dim3((unsigned)probs),
                 dim3(kBigWaves * kWave), 0, (hipStream_t)stream, a);
  }
  return check_launch("smcdet_extract");
}

}  // extern "C"
