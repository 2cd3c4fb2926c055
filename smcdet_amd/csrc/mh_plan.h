// mh_plan.h — what is decided before an MH sweep launch: the layout of the
// kernel's dynamic LDS and the launch plan (instantiation, LDS bytes, fused or
// split tail, store policy).  Plain C++, no device work: the
// plan is a value that a host test reads (scripts/asan/capi_driver.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/smcdet_hip.h"

#ifdef __HIP__
#define SMCDET_HD __host__ __device__
#else
#define SMCDET_HD
#endif
#ifndef SMCDET_SMALL_TILE_WAVES
#define SMCDET_SMALL_TILE_WAVES 7
#endif

namespace smcdet {
constexpr int kMhWaves = 4;            // particles (one wave each) per workgroup
constexpr int kMhPad = 64;             // dummy cells behind an image, one per lane (kWave)
constexpr int kMhMaxLdsPixels = 4096;  // larger tiles work in global memory (kMaxLdsPixels)
constexpr int kMhTailMaxN = 4096;      // the fused tail's particles per tile (kTailMaxN)
constexpr int kMhTabFloats = 4 * 513;  // the radial PSF table (kTabNodes float4)
constexpr size_t kMhLdsPerCu = 160 * 1024;

// The LDS layout in floats, HWp = H*W + kMhPad: [imgs images (M71 1, Poisson 2)]
// [kMhWaves rate images] [kMhWaves 1/v images (RV) or kMhWaves * S PSF-cache
// rows of H*W (PC)] [the PSF table, 16-byte aligned (TB)]
SMCDET_HD constexpr int mh_lds_rates(int imgs, int HWp) { return imgs * HWp; }
// a region of per-wave images: a wave's 1/v image lies this far behind its rates
SMCDET_HD constexpr int mh_lds_region(int HWp) { return kMhWaves * HWp; }
SMCDET_HD constexpr int mh_lds_cache(int imgs, int HWp) { return (imgs + kMhWaves) * HWp; }
SMCDET_HD constexpr int mh_lds_floats(int imgs, int HWp, int HW, int S, bool rv, bool pc) {
  return mh_lds_cache(imgs, HWp) + (rv ? mh_lds_region(HWp) : 0) + (pc ? kMhWaves * S * HW : 0);
}
SMCDET_HD constexpr int mh_lds_tab(int imgs, int HWp, int HW, int S, bool rv, bool pc) {
  return (mh_lds_floats(imgs, HWp, HW, S, rv, pc) + 3) & ~3;
}
constexpr size_t mh_lds_bytes(int model, int HW, int S, bool rv, bool pc, bool tab) {
  const int imgs = model == SMCDET_MODEL_POISSON ? 2 : 1, HWp = HW + kMhPad;
  return sizeof(float) * (size_t)(tab ? mh_lds_tab(imgs, HWp, HW, S, rv, pc) + kMhTabFloats
                                      : mh_lds_floats(imgs, HWp, HW, S, rv, pc));
}
// workgroups per CU (= waves per SIMD) an instantiation is built for
constexpr int mh_wg_per_cu(int ppl, bool replay, bool full) {
  return ppl == 1 ? (replay ? SMCDET_SMALL_TILE_WAVES - 1 : SMCDET_SMALL_TILE_WAVES)
                  : (full && ppl == 16 ? 2 : 4);
}

enum MhVariant {  // the instantiations by name (mh_sweep_kernel's PAIRED .. TB arguments)
  kMhGL,        // tiles above kMhMaxLdsPixels (M71): images in global memory, no LDS
  kMhPC,        // <= 64 pixels, incremental: the per-wave PSF cache, where 7 per CU fit
  kMhPaired,    // incremental, no cache (in the product: not M71 of 65..1024 pixels)
  kMhRV,        // M71, 65..1024 pixels, incremental: the per-wave 1/v image
  kMhTail,      // the fused SMC step: the tile pass in the sweep's last workgroup
  kMhUnpaired,  // full re-render; diagnostic build: scalar slots too
  kMhTB, kMhPCTB, kMhRVTB  // diagnostic build: the PSF table in LDS, alone / with PC / with RV
};
enum MhTailMode { kMhNoTail, kMhTailFused, kMhTailSplit };

struct MhPlanIn {
  int model, H, W, R;       // image model: kind, tile, psf radius
  int N, S, T;
  uint32_t flags;           // SMCDET_MH_*
  bool tail;                // a tile pass is asked for ...
  size_t tail_lds;          // ... with this LDS buffer (tile_lds_bytes(N))
  bool diag;                // the diagnostic build's variants exist
  bool replay = false, two_launch = false;  // SMCDET_SMC_TWO_LAUNCH
  bool rate_out = false;    // rate images are written back
  bool psf_tab = false;     // diagnostic build: this model has a device PSF table
  int cu_count = 0;         // compute units of the device (0: unknown)
};
struct MhPlan {
  int status = SMCDET_OK;   // or the error and its message
  const char* msg = "";
  int ppl = 0;              // pixels per lane rendered in registers: 1 / 4 / 16, 0: LDS render
  MhVariant variant = kMhPaired;
  bool geo_fixed = false;   // kMhRV with the 32x32 / R = 8 geometry compiled in
  size_t lds = 0;           // dynamic LDS bytes
  MhTailMode tail = kMhNoTail;
  bool write_through = false;
};

inline MhPlan mh_plan(const MhPlanIn& in) {
  MhPlan p;
  const bool m71 = in.model == SMCDET_MODEL_M71, full = in.flags & SMCDET_MH_FULL_RECOMPUTE;
  const bool scalar = in.diag && (in.flags & SMCDET_MH_SCALAR_SLOTS), paired = !full && !scalar;
  const bool no_pc = in.flags & SMCDET_MH_NO_PSF_CACHE;
  const long long HW = (long long)in.H * in.W;
  auto lds = [&](bool rv, bool pc, bool tab) {
    return mh_lds_bytes(in.model, (int)HW, in.S, rv, pc, tab);
  };
  if (HW > kMhMaxLdsPixels) {  // (M71 only: validate_model)
    static_assert(kMhMaxLdsPixels == 4096, "the message names it");
    if (scalar)
      return {SMCDET_EUNSUPPORTED, "tiles above 4096 pixels: no fused step / scalar slots"};
    p.variant = kMhGL;
    p.tail = in.tail ? kMhTailSplit : kMhNoTail;
    return p;
  }
  if (in.S <= kMhPad) p.ppl = HW <= 64 ? 1 : HW <= 256 ? 4 : HW <= 1024 ? 16 : 0;
  // The tail fuses into sweeps of tiles above 64 pixels whose N its one
  // instantiation takes, where 4 workgroups per CU hold the larger of the two
  // buffers; otherwise it is its own launch and the sweep is as without one.
  p.lds = lds(false, false, false);
  if (in.tail) {
    const size_t need = p.lds > in.tail_lds ? p.lds : in.tail_lds;
    const bool fusable = !(in.flags & (SMCDET_MH_FULL_RECOMPUTE | SMCDET_MH_SCALAR_SLOTS)) &&
                         in.N % kMhWaves == 0 && in.N <= kMhTailMaxN && p.ppl != 1 &&
                         4 * (need + 2048) <= kMhLdsPerCu;
    p.tail = fusable && !in.two_launch ? kMhTailFused : kMhTailSplit;
    if (p.tail == kMhTailFused) p.lds = need;
  }
  const bool fused = p.tail == kMhTailFused;
  if (fused && (!paired || p.ppl == 1)) return {SMCDET_EINVAL, "fused step: unsupported shape"};
  // Write-through rate-image stores (register-render tiles above 64 pixels)
  // where every workgroup is resident at once: all the images are then still
  // dirty in the L2 when the kernel ends.  A launch of several rounds has
  // written the earlier rounds' back by then and keeps the plain stores it was
  // measured with; the fused tail keeps its stores and fences.
  p.write_through = p.ppl > 1 && !full && !fused && in.rate_out &&
                    !(in.flags & SMCDET_MH_NO_WRITE_THROUGH) &&
                    (long long)((in.N + kMhWaves - 1) / kMhWaves) * in.T <=
                        (long long)in.cu_count * mh_wg_per_cu(p.ppl, in.replay, full);
  // The LDS-cached variants, richest first, where their workgroups per CU fit
  // the 160 KiB: the PSF cache (small tiles), the 1/v image (M71 register-render
  // tiles; 9 (H*W + 64) floats always fit), the PSF table (diagnostic build).
  auto take = [&](bool on, MhVariant v, bool rv, bool pc, bool tab, int wg_per_cu) {
    if (!on || (size_t)wg_per_cu * (lds(rv, pc, tab) + 1024) > kMhLdsPerCu) return false;
    p.variant = v;
    p.lds = lds(rv, pc, tab);
    return true;
  };
  const bool tb = in.diag && in.psf_tab && m71 && paired && !fused;
  if (p.ppl == 1 && !full) {
    constexpr int wg = SMCDET_SMALL_TILE_WAVES;
    if (take(tb && !no_pc, kMhPCTB, false, true, true, wg) ||
        take(paired && !no_pc, kMhPC, false, true, false, wg) ||
        take(tb, kMhTB, false, false, true, wg))
      return p;
  } else if (m71 && p.ppl > 1 && !full) {
    const bool rv = paired && !fused && !(in.diag && (in.flags & SMCDET_MH_NO_RCP_CACHE));
    if (take(tb && rv, kMhRVTB, true, false, true, 4) || take(tb, kMhTB, false, false, true, 4))
      return p;
    if (take(rv, kMhRV, true, false, false, 4)) {
      p.geo_fixed = p.ppl == 16 && in.H == 32 && in.W == 32 && in.R == 8 &&
                    !(in.flags & SMCDET_MH_GENERIC_GEOMETRY);
      return p;
    }
    if (!in.diag && !fused) return {SMCDET_EUNSUPPORTED, "M71 sweep: the 1/v image does not fit"};
  }
  p.variant = fused ? kMhTail : paired ? kMhPaired : kMhUnpaired;
  return p;
}
}  // namespace smcdet
