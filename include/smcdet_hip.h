/*
 * smcdet_hip.h — C ABI of the MI355X (gfx950) hot path of the smcdet SMC
 * star-detection sampler.  Plain pointers and sizes only; every buffer is a
 * caller-owned, contiguous, float32 (unless stated) device allocation on the
 * device that owns `stream`.  Every entry point is asynchronous on `stream`
 * (a hipStream_t passed as void*), never allocates, never synchronises, and
 * returns 0 on success or a negative SMCDET_E* code; smcdet_last_error()
 * then describes the failure (thread-local).
 *
 * Layout follows the reference (timwhite0/smcdet): tiles lead, then
 * particles, then sources.  T = numH*numW tiles (row-major), N particles per
 * tile, S sources per particle (= Prior.max_objects), tile H x W pixels.
 *   tiled_image [T,H,W]   locs [T,N,S,2] (row h, column w)   fluxes [T,N,S]
 *   counts [T,N] (float32, as the reference)                  per-tile [T]
 *
 * Each entry point cites the reference interface it replaces.  The
 * reference has no FFI: its "plugin" boundary is duck-typed Python objects
 * (smcdet/sampler.py:10-37); the Python package smcdet_amd keeps those
 * classes and calls this ABI through ctypes.
 */
#ifndef SMCDET_HIP_H
#define SMCDET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMCDET_ABI_VERSION 20

/* status codes */
#define SMCDET_OK 0
#define SMCDET_EINVAL -1      /* bad argument (null pointer, size, enum) */
#define SMCDET_EUNSUPPORTED -2 /* shape outside what the kernels support */
#define SMCDET_EHIP -3        /* HIP runtime error (launch/config) */

/* image models */
#define SMCDET_MODEL_M71 1     /* M71ImageModel: 3-component PSF, Gaussian noise */
#define SMCDET_MODEL_POISSON 2 /* ImageModel: Normal-pdf PSF, Poisson noise      */

/* priors */
#define SMCDET_PRIOR_M71 1    /* M71Prior: Poisson count, uniform locs, truncated-Pareto flux */
#define SMCDET_PRIOR_PARETO 2 /* ParetoStarPrior: uniform count, uniform locs, Pareto flux   */
/* StarPrior (smcdet/prior.py:125-154): uniform count, uniform locs, Normal
 * flux.  Added under SMCDET_ABI_VERSION 20 (additive: a new value of `kind`;
 * smcdet_prior_t keeps its layout, see the field reuse there).  Taken by
 * smcdet_log_prior, smcdet_prior_sample, and by smcdet_mh_sweep /
 * smcdet_mh_sweep_step / smcdet_mala_sweep with SMCDET_MODEL_POISSON (every
 * use in the reference); with SMCDET_MODEL_M71, and in smcdet_mh_chain and
 * smcdet_aggregate_sweep, it returns SMCDET_EUNSUPPORTED before any device
 * work.  A Normal flux may be <= 0: no zero-flux substitution (prior.py:151-154
 * has none) and no log(flux) in the prior term of the sweeps.
 * smcdet_prior_sample draws flux = mean + stdev * sqrt(2) * erfinv(2u' - 1)
 * with u' = min(max(u, 2^-25), 1 - 2^-24): u = 0 (which the generator can
 * return) maps to mean - 5.42 stdev, u = 1 - 2^-24 to mean + 5.29 stdev, both
 * finite. */
#define SMCDET_PRIOR_NORMAL 3

/* resampling */
#define SMCDET_RESAMPLE_MULTINOMIAL 0
#define SMCDET_RESAMPLE_SYSTEMATIC 1

/* mh flags */
#define SMCDET_MH_FULL_RECOMPUTE 1u /* re-render every source per step (reference arithmetic) */
/* draw the moved component from 0..count-1 instead of 0..S-1: a particle of
 * count s padded to S sources then moves exactly as the reference's
 * fixed-count kernel with S = s (kernel.py:35-37); count 0 never moves.
 * Used by the count-stratified sampler (CS-SMC). */
#define SMCDET_MH_COMPONENT_BY_COUNT 2u
/* independent stopping: tiles whose temperature is already 1 are not mutated
 * (their particles are only gathered through `ancestors`) */
#define SMCDET_MH_SKIP_DONE 4u

/* (no flag) A location proposal clamped onto the prior box's upper edge
 * (distributions.py:48) has log prior -inf (Uniform.log_prob(high),
 * prior.py:73) and is rejected; as in the reference, whose cached log target
 * then becomes -inf * 0 = NaN (kernel.py:125), the particle also rejects every
 * remaining proposal of that sweep. */

/* temper_reweight flags */
/* independent stopping: a tile that entered at temperature 1 keeps it (delta
 * 0), gets uniform weights, an unchanged log Z and ESS (that of its last
 * step) and identity resampling indices, so its final particles stay put
 * while the other tiles run on.
 * Without it (the reference, sampler.py:230) such tiles are resampled and
 * mutated at temperature 1 until every tile has finished. */
#define SMCDET_SMC_FREEZE_DONE 1u
/* smcdet_mh_sweep_step only: run the tile pass as its own launch right after
 * the sweep even where the shape could fuse (same results).  The default in
 * SMCsampler: on gfx950 the separate 512-thread tile kernel (~27 us at
 * N = 4096) beats the fused tail on the sweep's 256-thread workgroup (~30 us),
 * and back-to-back launches on one stream leave no gap to recover
 * (DESIGN.md §4.2). */
#define SMCDET_SMC_TWO_LAUNCH 2u
/* Flags marked "diagnostic build only" are compiled into
 * libsmcdet_hip_diag.so (make diag, -DSMCDET_DIAG) alone: the product library
 * returns SMCDET_EUNSUPPORTED for them before any device work.
 * diagnostic build only: ablations (timing only; results are NOT valid samples) */
#define SMCDET_MH_ABLATE_LIKELIHOOD 256u /* skip the delta-likelihood passes */
#define SMCDET_MH_ABLATE_PROPOSAL 512u   /* skip the truncated-normal proposal math */
/* diagnostic build only: evaluate the union window one position per lane instead of two
 * (packed arithmetic); same results up to float32 summation order */
#define SMCDET_MH_SCALAR_SLOTS 1024u
/* diagnostic: small tiles (H*W <= 64) without the per-wave PSF cache (the
 * moved source's old PSF re-evaluated each iteration); same results */
#define SMCDET_MH_NO_PSF_CACHE 2048u
/* diagnostic build only: M71 tiles of 65..1024 pixels without the per-wave 1/v image
 * (each pixel's 1/(s0^2 + eta*rate) formed per use); same results */
#define SMCDET_MH_NO_RCP_CACHE 4096u
/* diagnostic build only: M71 sweeps with the radial PSF table in LDS (the union
 * window's PSF values from a cubic table instead of exp2/log2; results differ
 * by float32 rounding of the profile, ~3e-7 relative).  Measured slower at
 * 32x32 (its LDS reads) and even at 8x8, so off by default */
#define SMCDET_MH_PSF_TABLE 8192u
/* diagnostic: M71 tiles of 16x16 .. 1024 pixels without the block form of
 * same-anchor steps (the union window's first 16 rows and columns as one
 * 16x16 block whose Gaussian PSF terms come from a rank-4 MFMA); results
 * differ by float32 rounding of the profile */
#define SMCDET_MH_NO_BLOCK 16384u
/* diagnostic: M71 32x32 tiles with psf_radius 8 through the sweep that reads
 * the tile geometry at run time (every other shape's kernel) instead of the
 * instantiation with H, W and R compiled in; same results, bit for bit
 * (DESIGN.md §4.1).  Added under SMCDET_ABI_VERSION 20 (additive: a flag bit
 * that was free; no entry point or struct changed). */
#define SMCDET_MH_GENERIC_GEOMETRY 32768u
/* diagnostic: the sweep's rate images stored with plain stores where it would
 * store them write-through (launches of one resident round of workgroups: the
 * dirty lines then wait in the L2 for the write-back at the kernel's end);
 * same results, bit for bit.  Additive: a flag bit that was
 * free; no entry point or struct changed. */
#define SMCDET_MH_NO_WRITE_THROUGH 65536u

/* Image model (smcdet/images.py:6-26 ImageModel, :105-145 M71ImageModel). */
typedef struct smcdet_image_model {
  int32_t model;          /* SMCDET_MODEL_* */
  int32_t H, W;           /* tile height / width in pixels */
  int32_t psf_radius;     /* R: (2R+1)^2 window anchored at floor(loc) */
  float background;       /* additive background (ADU) */
  float adu_per_nmgy;     /* M71 flux scale; 1 for POISSON */
  float psf_params[6];    /* M71: sigma1, sigma2, sigmap, beta, b, p0; POISSON: [0]=psf_stdev */
  float psf_norm;         /* M71 normalising constant C (images.py:122-135) */
  float noise_additive;   /* M71: variance = noise_additive + noise_multiplicative*rate */
  float noise_multiplicative;
} smcdet_image_model_t;

/* Prior (smcdet/prior.py:8-75, :78-101, :125-154, :157-189, :192-226). */
typedef struct smcdet_prior {
  int32_t kind;           /* SMCDET_PRIOR_* */
  int32_t min_objects, max_objects;
  float loc_low;          /* -pad */
  float loc_high_h;       /* H + pad */
  float loc_high_w;       /* W + pad */
  float poisson_mean;     /* M71: counts_rate*(H+2pad)*(W+2pad) */
  float flux_alpha;       /* NORMAL: unused */
  float flux_lower;       /* M71: truncated-Pareto lower; PARETO: flux_scale; NORMAL: flux_mean */
  float flux_upper;       /* M71: truncated-Pareto upper; PARETO: unused; NORMAL: flux_stdev
                           * (finite, > 0; flux_mean finite: else SMCDET_EINVAL) */
} smcdet_prior_t;

/* Single-component MH kernel (smcdet/kernel.py:7-24). */
typedef struct smcdet_mh {
  int32_t num_iters;
  float locs_stdev;
  float fluxes_stdev;
  float fluxes_min, fluxes_max;
  float locs_min_h, locs_min_w; /* = Prior.loc_prior.low  (sampler.py:36) */
  float locs_max_h, locs_max_w; /* = Prior.loc_prior.high (sampler.py:37) */
} smcdet_mh_t;

/* Optional replay of recorded draws (tests): per MH iteration k, tile t,
 * particle n: the chosen component, the two location uniforms and the flux
 * uniform of the chosen component, and the accept uniform.
 * trace_loga / trace_accept (nullable; smcdet_mh_sweep / _step only): the
 * sweep writes each decision's log alpha (float32, as the kernel evaluated
 * it) and its accept flag (0/1) at [k,t,n] -- decision-by-decision parity
 * against recorded reference decisions (kernel.py:114-116).  Iterations a
 * particle does not run (after an upper-edge freeze, or K = 0) are left
 * untouched.  Only the replay instantiation carries these stores. */
typedef struct smcdet_mh_replay {
  const int32_t* comp; /* [K,T,N]   */
  const float* uloc;   /* [K,T,N,2] */
  const float* uflux;  /* [K,T,N]   */
  const float* uacc;   /* [K,T,N]   */
  float* trace_loga;   /* [K,T,N] (nullable) */
  uint8_t* trace_accept; /* [K,T,N] (nullable) */
} smcdet_mh_replay_t;

/* "smcdet_hip <version> (gfx950) src <sha1 of the library's sources>" */
const char* smcdet_version(void);
int32_t smcdet_abi_version(void);
const char* smcdet_last_error(void);

/* Pinned, device-mapped host memory (hipHostMalloc): *host is the host
 * address, *device the address kernels use; zero-filled.  For small
 * device->host signals without a copy launch (smcdet_temper_reweight's
 * live_host).  Free with smcdet_host_free(host). */
int smcdet_host_alloc(size_t bytes, void** host, void** device);
int smcdet_host_free(void* host);

/* Per-launch kernel timing for benchmarks (no reference counterpart).  While
 * enabled, each of the next max_launches sweep launches (smcdet_mh_sweep,
 * smcdet_mh_sweep_step, smcdet_mala_sweep) is dispatched by
 * hipExtLaunchKernel with a start/stop event pair of an internal pool: the
 * events are stamped by the kernel's own dispatch, so timing adds no marker
 * packet (and no launch bubble) between kernels.  max_launches = 0 disables
 * timing and frees the pool; a new call discards earlier timings.
 * smcdet_launch_timing_read waits for the timed launches and writes the first
 * min(max, *n_out) durations in ms; *n_out = launches timed since enabling.
 * The pool is process-global and not thread-safe: enable, launch and read
 * from one host thread (bench.py does). */
int smcdet_launch_timing(int32_t max_launches);
int smcdet_launch_timing_read(float* ms, int32_t max, int32_t* n_out);
/* The same launches' start times in ms after the first timed launch's start
 * (launch-to-launch intervals: the step-time spread bench.py reports). */
int smcdet_launch_timing_starts(float* ms, int32_t max, int32_t* n_out);
/* on != 0: while timing is enabled, the per-tile temper / reweight /
 * resampling launches (smcdet_temper, smcdet_update_weights,
 * smcdet_temper_reweight and the tile pass of a two-launch
 * smcdet_mh_sweep_step) also take event pairs from the pool, in launch order
 * with the sweeps (a two-launch SMC step: sweep, then tile pass).  Off by
 * default; smcdet_launch_timing(0) turns it off. */
int smcdet_launch_timing_tiles(int32_t on);

/* ImageModel.loglikelihood / M71ImageModel.loglikelihood
 * (smcdet/images.py:85-102, :159-175): out[T,N].  Tiles up to 4096 pixels
 * (either model) stage the tile in LDS; M71 tiles up to 65536 pixels render
 * 64-pixel chunks in registers and read the tile from global memory
 * (smcdet_render likewise).  MALA, MCMC chains and aggregation sweeps keep
 * the 4096-pixel LDS budget. */
int smcdet_loglik(const smcdet_image_model_t* model, const float* tiled_image,
                  const float* locs, const float* fluxes, int32_t T, int32_t N,
                  int32_t S, float* out, void* stream);

/* rate image lambda = B + sum_j g*f_j*psf_j  (images.py:80-82, :149-154):
 * rate[T,H,W,N] (the layout the reference's ImageModel.sample produces). */
int smcdet_render(const smcdet_image_model_t* model, const float* locs,
                  const float* fluxes, int32_t T, int32_t N, int32_t S,
                  float* rate, void* stream);

/* ImageModel.psf (smcdet/images.py:28-76): dense psf[T,H,W,N,S]. */
int smcdet_psf_dense(const smcdet_image_model_t* model, const float* locs,
                     int32_t T, int32_t N, int32_t S, float* psf, void* stream);

/* Noise draw for ImageModel.sample (images.py:78-83 Poisson, :147-157
 * Normal): image[T,H,W,N] from rate[T,H,W,N] (in place allowed).  Element i
 * draws from the Philox counter offset + i, so a call at offset k repeats
 * elements k.. of the call at offset 0.  Poisson draws follow the Poisson law
 * for rates up to 1e6 (the supported ceiling: the transformed-rejection
 * candidate is float32, its acceptance test double); a rate that is zero,
 * negative or NaN gives 0. */
int smcdet_sample_image(const smcdet_image_model_t* model, const float* rate,
                        int64_t count, uint64_t seed, uint64_t offset,
                        float* image, void* stream);

/* Per-tile location boxes (every function taking `tile_boxes`): a nullable
 * [T,4] float array (lo_h, lo_w, hi_h, hi_w) that replaces the prior's
 * [-pad, H+pad) x [-pad, W+pad) for tile t -- the tiles' boxes then partition
 * the padded image (padding only on its outer edges), so the product of the
 * tiles' priors is the whole image's prior (used by tile aggregation,
 * DESIGN.md §9).  An M71 prior's Poisson count mean scales with the box
 * area.  Null: the reference's per-tile padding (prior.py:17-23). */

/* Prior.log_prob (smcdet/prior.py:67-75, :183-189, :220-226): out[T,N]. */
int smcdet_log_prior(const smcdet_prior_t* prior, const float* counts,
                     const float* locs, const float* fluxes, int32_t T,
                     int32_t N, int32_t S, const float* tile_boxes, float* out,
                     void* stream);

/* Prior.sample(stratify_by_count=True, num_catalogs_per_count=n_per_count)
 * (smcdet/prior.py:25-64, :201-217): N = (max-min+1)*n_per_count.
 * uloc [T,N,S,2] / uflux [T,N,S] replay the uniforms when non-null. */
int smcdet_prior_sample(const smcdet_prior_t* prior, int32_t T,
                        int32_t n_per_count, uint64_t seed, uint64_t offset,
                        const float* uloc, const float* uflux,
                        const float* tile_boxes, float* counts, float* locs,
                        float* fluxes, void* stream);

/* SingleComponentMH.run (smcdet/kernel.py:26-130), K = mh->num_iters
 * iterations fused in one launch.  Reads the state of particle
 * ancestors[t,n] (identity when null) from *_in and writes the mutated
 * state to *_out (in place allowed when ancestors is null).  counts_out may
 * be null.  temperature[T].  Outputs: acc_rate[T] = acceptance rate of the
 * LAST iteration (kernel.py:130); loglik_out[T,N] (nullable) = the image
 * log-likelihood of the returned state (what SMCsampler.temper recomputes,
 * sampler.py:100-102).  acc_count[2T] is an int32 workspace, 8-byte aligned,
 * that must be zero before the first call; every call leaves it zero again
 * (it holds the per-tile accept counters and workgroup tickets only while the
 * kernel runs), so one zeroed buffer serves every call on a stream.
 * rate_in / rate_out [T,N,H*W] (both nullable, ignored with
 * SMCDET_MH_FULL_RECOMPUTE): persisted per-particle rate images
 * lambda = B + sum_j g f_j psf_j.  With rate_in the sweep starts from the
 * image of particle ancestors[t,n] instead of re-rendering all S sources;
 * rate_out receives the image of the returned state (maintained
 * incrementally, float32 update rounding).  rate_in must describe *_in
 * exactly; rate_in != rate_out when ancestors is non-null.
 * Tiles above 4096 pixels (M71 model, up to 65536 = 256x256 pixels): the tile
 * image and the rate images live in global memory -- rate_in / rate_out are
 * [T,N,H*W+64] (64 dummy cells per row for masked lanes), rate_out is
 * REQUIRED (the sweep updates its rows in place; with FULL_RECOMPUTE their
 * contents afterwards are unspecified), rate_in == rate_out is allowed
 * without ancestors, and the fused step (smcdet_mh_sweep_step) runs as two
 * launches.
 * go (nullable, int32 device scalar): when *go == 0 the launch does nothing
 * (no output is written) -- lets a host enqueue the next SMC iteration before
 * it has read the loop condition (see smcdet_temper_reweight's `live`).
 * tile_boxes (nullable): per-tile location boxes in place of mh->locs_min/max.
 * Tiles wider than 256 pixels: without SMCDET_MH_FULL_RECOMPUTE,
 * 2*psf_radius + 2 + 4.8*locs_stdev must not exceed 256 (the widest window
 * that an old and a proposed position can span), else SMCDET_EUNSUPPORTED. */
int smcdet_mh_sweep(const smcdet_image_model_t* model,
                    const smcdet_prior_t* prior, const smcdet_mh_t* mh,
                    const float* tiled_image, const float* temperature,
                    int32_t T, int32_t N, int32_t S, const int64_t* ancestors,
                    const float* counts_in, const float* locs_in,
                    const float* fluxes_in, float* counts_out,
                    float* locs_out, float* fluxes_out, const float* rate_in,
                    float* rate_out, uint64_t seed,
                    uint64_t offset, const smcdet_mh_replay_t* replay,
                    uint32_t flags, float* loglik_out, float* acc_rate,
                    int32_t* acc_count, const int32_t* go,
                    const float* tile_boxes, void* stream);

/* SingleComponentMALA.run (smcdet/kernel.py:133-275), K iterations fused in
 * one launch.  Arguments as smcdet_mh_sweep; mala->locs_stdev and
 * mala->fluxes_stdev carry the step sizes (locs_step, fluxes_step,
 * kernel.py:134-145).  The gradient of log_target w.r.t. the chosen source's
 * (h, w, f) -- what torch.autograd.grad computes (kernel.py:160-166,
 * :190-197) -- is evaluated analytically in-kernel over the source's PSF
 * window.  Flags: SMCDET_MH_COMPONENT_BY_COUNT, SMCDET_MH_SKIP_DONE.
 * The replay layout is smcdet_mh_replay_t's; `go` as smcdet_mh_sweep. */
int smcdet_mala_sweep(const smcdet_image_model_t* model,
                      const smcdet_prior_t* prior, const smcdet_mh_t* mala,
                      const float* tiled_image, const float* temperature,
                      int32_t T, int32_t N, int32_t S, const int64_t* ancestors,
                      const float* counts_in, const float* locs_in,
                      const float* fluxes_in, float* counts_out,
                      float* locs_out, float* fluxes_out, const float* rate_in,
                      float* rate_out, uint64_t seed,
                      uint64_t offset, const smcdet_mh_replay_t* replay,
                      uint32_t flags, float* loglik_out, float* acc_rate,
                      int32_t* acc_count, const int32_t* go, void* stream);

/* MHsampler.run (smcdet/sampler.py:301-486): one single-component MH chain
 * per (tile, chain) at temperature 1 -- C chains per tile, T tiles (the
 * reference runs C = 1).  locs_state [T,C,S,2] / fluxes_state [T,C,S] hold
 * the chain state (the initial sample on the first call) and are updated in
 * place; iterations [k_begin, k_end) of num_samples_total - 1 run in this
 * call (chunked runs continue the same Philox streams).  Sample m is the
 * state after iteration m-1 (sample 0 = the initial state); samples
 * m >= num_samples_burnin with (m - burnin) % keep_every_k == 0 are written to
 * locs_out [T,C,M,S,2] / fluxes_out [T,C,M,S], M = ceil((total - burnin) /
 * keep), the reference's burn_thin_idx (sampler.py:339-341).  accept_out
 * [T,C,total-1] int32 (nullable): the accept flag of every iteration.
 * mh->locs_stdev / fluxes_stdev / bounds as in smcdet_mh_sweep (the
 * reference takes the flux bounds from Prior.flux_lower/flux_upper).  Replay
 * buffers: comp [total-1,T,C], uloc [total-1,T,C,2], uflux / uacc
 * [total-1,T,C].  frozen [T,C] int32 (nullable, zero before the first call):
 * a chain whose location proposal lands on the prior box's upper edge
 * rejects it and every later proposal of the run, as the reference's NaN
 * cached target does (sampler.py:522-526); the flag carries that across
 * chunked calls. */
int smcdet_mh_chain(const smcdet_image_model_t* model,
                    const smcdet_prior_t* prior, const smcdet_mh_t* mh,
                    const float* tiled_image, int32_t T, int32_t C, int32_t S,
                    const float* counts, float* locs_state, float* fluxes_state,
                    int32_t num_samples_total, int32_t num_samples_burnin,
                    int32_t keep_every_k, int32_t k_begin, int32_t k_end,
                    uint64_t seed, uint64_t offset,
                    const smcdet_mh_replay_t* replay, float* locs_out,
                    float* fluxes_out, int32_t* accept_out, int32_t* frozen,
                    void* stream);

/* SMCsampler.temper (smcdet/sampler.py:93-125) on device: per tile, delta
 * solves exp(2 LSE(delta*l) - LSE(2 delta*l)) = ess_threshold on (0, 1-tau]
 * (or delta = 1-tau when the ESS there is still above threshold).
 * temperature[T] is updated in place (float32 tau + delta); temperature_prev
 * receives the old value. */
int smcdet_temper(const float* loglik, float* temperature,
                  float* temperature_prev, int32_t T, int32_t N,
                  double ess_threshold, void* stream);

/* SMCsampler.update_weights (smcdet/sampler.py:181-196). */
int smcdet_update_weights(const float* loglik, const float* temperature,
                          const float* temperature_prev,
                          float* log_weights_unnorm, float* weights,
                          float* ess, float* log_norm_const, int32_t T,
                          int32_t N, void* stream);

/* Resampling indices (smcdet/sampler.py:127-150): systematic
 * (bucketize of (n+U)/N into cumsum(W)) or multinomial (iid).  u replays the
 * uniforms when non-null ([T] systematic, [T,N] multinomial). */
int smcdet_resample_index(const float* weights, int32_t T, int32_t N,
                          int32_t method, uint64_t seed, uint64_t offset,
                          const float* u, int64_t* idx, void* stream);

/* temper + update_weights (+ resample index when idx != null) fused: one
 * launch per SMC iteration instead of three.  flags: SMCDET_SMC_*.
 * finished_iter [T] (nullable, int32): set to `iter` when a tile's
 * temperature reaches 1 while it holds a negative value (per-tile finishing
 * iteration).  live [3] (nullable, int32, 8-byte aligned, zero before the first call): after
 * the call live[2] = the number of tiles still below temperature 1 (the
 * reference's while condition, sampler.py:230); live[0..1] are workspace and
 * left zero.  go (nullable): when *go == 0 the launch does nothing.
 * live_host (nullable, used with live): pinned, device-accessible host memory
 * (hipHostMalloc) that also receives live[2], so a host can read the count
 * once the launch has completed without enqueueing a copy. */
int smcdet_temper_reweight(const float* loglik, float* temperature,
                           float* temperature_prev, float* log_weights_unnorm,
                           float* weights, float* ess, float* log_norm_const,
                           int32_t T, int32_t N, double ess_threshold,
                           int32_t resample_method, uint64_t seed,
                           uint64_t offset, int64_t* idx, uint32_t flags,
                           int32_t* finished_iter, int32_t iter, int32_t* live,
                           const int32_t* go, int32_t* live_host, void* stream);

/* The temper / reweight / resample-index half of a fused SMC iteration
 * (smcdet_mh_sweep_step): the arguments of smcdet_temper_reweight that the
 * sweep does not already carry (its loglik_out and temperature are the
 * pass's log-likelihoods and temperatures).  resample_u [T] (nullable)
 * replays the systematic offsets (tests); multinomial draws are not
 * replayable here. */
typedef struct smcdet_smc_tail {
  float* temperature_prev;
  float* log_weights_unnorm;
  float* weights;
  float* ess;
  float* log_norm_const;
  double ess_threshold;
  int32_t resample_method;
  uint32_t flags;            /* SMCDET_SMC_* */
  uint64_t seed;
  uint64_t offset;
  int64_t* idx;              /* [T,N] next resampling indices (nullable) */
  const float* resample_u;   /* [T] systematic U replay (nullable) */
  int32_t* finished_iter;
  int32_t* live;
  int32_t* live_host;
  int32_t iter;
  int32_t reserved;
  /* (ABI 16) systematic resampling handed to the next sweep as bins instead
   * of indices: bins_out (nullable; SMCDET_BINS_FLOATS(T, N) floats) receives
   * the tile's running sum of the new weights, [T*N] (float32 roundings of the
   * float64 cumsum), then the T offsets U, then (ABI 17) per tile the 64
   * chunk-end bins of the search's first level, [T*64]: entry l is
   * bins[min((l+1)*c, N) - 1] for l < ceil(N/c), c = ceil(N/64) -- so the
   * first level reads 256 contiguous bytes per wave instead of 64 strided
   * lines.  The tile pass then skips the index search; anc_bins (nullable,
   * input) is such a buffer from the previous step, and each wave of this
   * sweep finds its own ancestor in it (idx[n] = #{i : bins[i] < (n + U)/N},
   * clamped to N - 1: the same indices, bit for bit) in place of
   * `ancestors`.  smcdet_bins_index converts a buffer to the indices. */
  const float* anc_bins;
  float* bins_out;
} smcdet_smc_tail_t;

/* One SMC iteration of SMCsampler.run (smcdet/sampler.py:221-237: resample
 * -> mutate -> temper -> update_weights, the resample being the sweep's
 * ancestor gather): smcdet_mh_sweep followed by smcdet_temper_reweight on its
 * loglik_out (required), with the same results bit for bit.  One launch: the
 * last workgroup to finish a tile runs the tile's temper / reweight / index
 * pass in the sweep's own LDS, so the pass starts the moment the tile's last
 * particle is done and the step pays one launch instead of two.  Shapes the
 * fused form does not cover (N % 4 != 0, N > 4096, tiles of <= 64 pixels,
 * SMCDET_MH_FULL_RECOMPUTE, an LDS budget that would cost occupancy) run as
 * the two launches; smcdet_mh_sweep_step_fused() reports which. */
int smcdet_mh_sweep_step(const smcdet_image_model_t* model,
                         const smcdet_prior_t* prior, const smcdet_mh_t* mh,
                         const float* tiled_image, float* temperature,
                         int32_t T, int32_t N, int32_t S,
                         const int64_t* ancestors, const float* counts_in,
                         const float* locs_in, const float* fluxes_in,
                         float* counts_out, float* locs_out, float* fluxes_out,
                         const float* rate_in, float* rate_out, uint64_t seed,
                         uint64_t offset, const smcdet_mh_replay_t* replay,
                         uint32_t flags, float* loglik_out, float* acc_rate,
                         int32_t* acc_count, const int32_t* go,
                         const float* tile_boxes, const smcdet_smc_tail_t* tail,
                         void* stream);
/* 1 when smcdet_mh_sweep_step runs these shapes as one launch, else 0. */
int smcdet_mh_sweep_step_fused(const smcdet_image_model_t* model, int32_t N,
                               int32_t S, uint32_t flags);

/* Gather of the resampled state (smcdet/sampler.py:150-169). */
/* The systematic resampling indices [T,N] of a bins buffer (the tail's
 * bins_out layout: [T*N] running sums, [T] offsets U, [T*64] first-level
 * chunk ends): idx[t,n] = #{i : bins[t,i] < (n + U_t)/N} clamped to N - 1
 * (sampler.py:141-148). */
#define SMCDET_BINS_FLOATS(T, N) ((size_t)(T) * (size_t)(N) + (size_t)(T) * 65u)
int smcdet_bins_index(const float* bins, int32_t T, int32_t N, int64_t* idx, void* stream);

int smcdet_gather(const int64_t* idx, int32_t T, int32_t N, int32_t S,
                  const float* counts_in, const float* locs_in,
                  const float* fluxes_in, float* counts_out, float* locs_out,
                  float* fluxes_out, void* stream);

/* Count-stratified SMC combination (manuscript/manuscript.tex:344-354,
 * Algorithm 2; the reference describes CS-SMC but has no code for it at HEAD).
 * Per image tile t, with NS count strata k (count s_min + k) whose fixed-count
 * samplers ran as "stratum tiles" t*NS + k of N equally weighted particles:
 *   probs[t,k] = p(s|x) = softmax_k(log_norm_const[t*NS+k] + log_count_prior[k])
 *   (log_count_prior [T,NS] per tile when lcp_per_tile != 0: tile boxes)
 *   then n_out catalogs: stratum k_n ~ probs[t,:] (systematic: u_n = (n+U)/n_out,
 *   first k with cumsum(probs) >= u_n; multinomial: iid u_n), and a uniform
 *   particle m_n = floor(v_n * N) of that stratum; idx[t,n] = k_n*N + m_n and
 *   the catalog (counts [T,NS,N], locs [T,NS,N,S,2], fluxes [T,NS,N,S]) is
 *   gathered to counts_out [T,n_out], locs_out, fluxes_out.
 * u_strata ([T] systematic / [T,n_out] multinomial) and u_pick [T,n_out]
 * replay the uniforms when non-null. */
int smcdet_count_posterior(const float* log_norm_const,
                           const float* log_count_prior, int32_t lcp_per_tile,
                           int32_t T, int32_t NS,
                           int32_t N, int32_t S, int32_t n_out,
                           int32_t resample_method, uint64_t seed,
                           uint64_t offset, const float* u_strata,
                           const float* u_pick, const float* counts_in,
                           const float* locs_in, const float* fluxes_in,
                           float* probs, int64_t* idx, float* counts_out,
                           float* locs_out, float* fluxes_out, void* stream);

/* SMCsampler.prune (smcdet/sampler.py:198-219): counts_out[T,N] int64,
 * kept sources compacted to the front in their original order. */
int smcdet_prune(const float* locs, const float* fluxes, int32_t T, int32_t N,
                 int32_t S, float tile_dim, float flux_threshold,
                 int64_t* counts_out, float* locs_out, float* fluxes_out,
                 void* stream);

/* ---- evaluation (smcdet/metrics.py:8-84, match_catalogs) ----------------- */
#define SMCDET_MATCH_MAX_SOURCES 64 /* St, Se: one source per lane */
#define SMCDET_MATCH_MAX_BINS 64    /* B: one magnitude bin per lane */

/* Matches sampled catalogs to a true catalog, tile by tile, and counts sources
 * and matches per magnitude bin.  Layouts are smcdet_prune's, kept sources
 * first:
 *   true_counts [T] int32, true_locs [T,St,2], true_fluxes [T,St]
 *   est_counts [T,N] int32, est_locs [T,N,Se,2], est_fluxes [T,N,Se]
 * (the counts are int32: cast smcdet_prune's int64 or the samplers' float32).
 * index [T,M] int64 (nullable), values in [0, N): catalog index[t,j] of tile t
 * is problem (t, j).  Null: M must equal N and problem (t, j) is catalog j.
 * Per problem, with n / m the two counts clamped to [0,St] / [0,Se] (only the
 * first n / m slots are read; padding may hold anything):
 *   mag = 22.5 - 2.5 log10(flux); a pair is in tolerance iff its Euclidean
 *   distance <= locs_tol and |delta mag| <= mags_tol (the reference's strict
 *   `>` for out of bounds, metrics.py:51-57).  The matching is the exact
 *   lexicographic optimum: the largest number of in-tolerance pairs, then the
 *   smallest sum of their distances (what the reference's cost
 *   locs_dist + oob * 1e20 intends; its float32 / float64 sums swallow the
 *   distances whenever an out-of-tolerance pair must be assigned).  Ties of
 *   the objective: one optimum, the same on every run.
 *   A source with a non-finite location or a non-finite or non-positive flux
 *   is out of tolerance with everything (the reference raises from scipy).
 * Outputs, each [T,M,B] float32 (metrics.py:67-77): a source of magnitude x
 * is counted in bin b = torch.bucketize(x, mag_bins), mag_bins[b-1] < x <=
 * mag_bins[b] (mag_bins [B] ascending; b = 0 is everything <= mag_bins[0];
 * b = B, fainter than the last edge, and a NaN magnitude are counted nowhere).
 * true_total / est_total bin all n / m sources, true_matches / est_matches
 * the matched ones.  match_of_true [T,M,St] int32 (nullable): the est slot
 * matched to true source i, or -1 (also for i >= n).
 * St, Se <= SMCDET_MATCH_MAX_SOURCES and B <= SMCDET_MATCH_MAX_BINS, else
 * SMCDET_EUNSUPPORTED before any device work; null required buffers, T, N or
 * M < 1, a non-positive tolerance, or a null index with M != N: SMCDET_EINVAL. */
int smcdet_match_catalogs(const int32_t* true_counts, const float* true_locs,
                          const float* true_fluxes, const int32_t* est_counts,
                          const float* est_locs, const float* est_fluxes,
                          const int64_t* index, int32_t T, int32_t N, int32_t M,
                          int32_t St, int32_t Se, float locs_tol, float mags_tol,
                          const float* mag_bins, int32_t B, float* true_total,
                          float* true_matches, float* est_total,
                          float* est_matches, int32_t* match_of_true,
                          void* stream);

/* ---- condensed catalogs --------------------------------- */
/* A run leaves N equally weighted (or weighted) catalogs per tile; these three
 * entry points, with smcdet_match_catalogs between the second and the third,
 * condense them into one list of detections per tile.  The reference has no
 * counterpart (its notebooks scatter-plot the sampled locations by hand).
 *
 * Layouts as smcdet_match_catalogs: counts [T,N] int32, locs [T,N,S,2],
 * fluxes [T,N,S], kept sources first; weights [T,N] (nullable: every catalog
 * weighs 1).  Source (t, n, j) is *counted* iff j < clamp(counts[t,n], 0, S),
 * both coordinates are finite and the flux is finite and > 0 -- the rule of
 * smcdet_match_catalogs; padding may hold anything, NaN included.
 * `box` is a HOST pointer to four floats (lo_h, lo_w, hi_h, hi_w), read
 * during the call: the location box every tile shares.  tile_boxes (nullable,
 * device [T,4]) replaces it per tile, as elsewhere in this header. */
#define SMCDET_MAP_MAX_CELLS_PER_PIXEL 8
#define SMCDET_MAP_MAX_GRID 2048     /* Gh, Gw of smcdet_source_map */
#define SMCDET_PEAKS_MAX_CELLS 32768 /* Gh*Gw of smcdet_map_peaks (128 KiB of LDS) */
#define SMCDET_PEAKS_MAX_SMOOTH 8    /* smooth_radius, cells */
#define SMCDET_PEAKS_MAX_NMS 16      /* nms_radius, cells */
#define SMCDET_SEED_MOMENTS 10       /* float64 sums per seed of smcdet_seed_moments */

/* Posterior source-density map on a grid of c = cells_per_pixel (1..8) cells
 * per pixel, Gh x Gw cells per tile, cell (0,0) at the box's lower corner.
 * The cell of a counted source at (h, w) is, in float32 exactly as written,
 *   ih = floorf((h - lo_h) * (float)c),  iw = floorf((w - lo_w) * (float)c),
 * and it lies in the grid iff 0 <= ih < Gh and 0 <= iw < Gw.
 *   count_map [T,Gh,Gw]           sum of the weights of the counted sources per cell
 *   flux_map  [T,Gh,Gw] nullable  sum of weight * flux (the float32 product) per cell
 *   outside   [T]                 weight of the counted sources in no cell
 * The outputs are zeroed here (memsets on `stream`) before the launch.
 * Each workgroup bins a chunk of one tile's particles into an LDS copy of the
 * grid (up to 160 KiB for the one or two maps) and flushes its non-zero cells
 * with float atomic adds; a larger grid is added to in global memory directly.
 * Reproducibility: with weights == NULL every cell of count_map and outside is
 * an integer below 2^24, hence exact and identical on every run whatever the
 * arrival order.  With weights, and for flux_map always, the float32 adds
 * arrive in an order that varies, so the last bits may differ between runs.
 * cells_per_pixel outside 1..8, Gh or Gw > SMCDET_MAP_MAX_GRID, or N*S above
 * 2^31-1: SMCDET_EUNSUPPORTED before any device work; a null required buffer,
 * a size < 1 or (without tile_boxes) a box that is not finite with lo < hi:
 * SMCDET_EINVAL. */
int smcdet_source_map(const int32_t* counts, const float* locs,
                      const float* fluxes, const float* weights,
                      const float* box, const float* tile_boxes, int32_t T,
                      int32_t N, int32_t S, int32_t cells_per_pixel, int32_t Gh,
                      int32_t Gw, float* count_map, float* flux_map,
                      float* outside, void* stream);

/* Seeds: the peaks of map [T,Gh,Gw].  With q = smooth_radius (0..8) and p =
 * nms_radius (0..16), in cells:
 *   s[i,j] = sum of map over the (2q+1)^2 window around (i,j), the map taken
 *   as zero outside the grid (float32, summed row by row);
 *   cell x is a peak iff s[x] >= min_mass[t], s[x] > 0 and, for every other
 *   cell y of the grid within Chebyshev distance p, s[x] > s[y], or s[x] ==
 *   s[y] and the flat index i*Gw + j of x is below that of y.
 * min_mass [T] is a device array.  The peaks are ordered by descending s, then
 * ascending flat index, and the first K (<= SMCDET_MATCH_MAX_SOURCES) kept:
 *   n_seeds   [T]     int32  number of seeds kept
 *   seed_cell [T,K]   int32  flat cell index; -1 past n_seeds
 *   seed_mass [T,K]          s at the peak; 0 past n_seeds
 *   seed_locs [T,K,2]        NaN past n_seeds; else the mass-weighted centroid
 *       of the raw map over the peak's (2q+1)^2 window clipped to the grid, in
 *       pixels: lo + (sum m*(i+0.5) / sum m) / c, formed in float64 and
 *       rounded once.
 * One workgroup per tile, the smoothed map in LDS: Gh*Gw above
 * SMCDET_PEAKS_MAX_CELLS is SMCDET_EUNSUPPORTED (use a smaller
 * cells_per_pixel), as are K, cells_per_pixel and the radii outside their
 * ranges; null buffers and sizes < 1 are SMCDET_EINVAL.  Deterministic. */
int smcdet_map_peaks(const float* map, const float* box,
                     const float* tile_boxes, int32_t T, int32_t Gh, int32_t Gw,
                     int32_t cells_per_pixel, int32_t smooth_radius,
                     int32_t nms_radius, const float* min_mass, int32_t K,
                     int32_t* n_seeds, int32_t* seed_cell, float* seed_mass,
                     float* seed_locs, void* stream);

/* Per-seed posterior moments.  match_of_seed [T,N,K] int32 is the
 * match_of_true output of smcdet_match_catalogs with the seeds as the true
 * catalog: the slot of catalog n matched to seed k, or -1.  seed_locs [T,K,2].
 * moments [T,K,SMCDET_SEED_MOMENTS] is FLOAT64 (double): sums over the
 * catalogs n with 0 <= match_of_seed[t,n,k] < S, w the catalog's weight (or
 * 1), every operand converted to double before any arithmetic, with
 * dh = (double)h - (double)seed_h, dw likewise, f the matched flux and
 * m = 22.5 - 2.5 log10((double)f):
 *   0 sum w      1 sum w dh    2 sum w dw    3 sum w dh^2   4 sum w dw^2
 *   5 sum w dh dw   6 sum w f   7 sum w f^2   8 sum w m     9 sum w m^2
 * matched_flux [T,N,K] float32 (nullable): the matched source's flux, NaN when
 * unmatched.  One workgroup per tile; each lane accumulates one seed over a
 * fixed stride of catalogs in float64 and the lanes of a seed are then added
 * in lane order, so the result is identical on every run.
 * K or S above SMCDET_MATCH_MAX_SOURCES: SMCDET_EUNSUPPORTED; null required
 * buffers and sizes < 1: SMCDET_EINVAL. */
int smcdet_seed_moments(const int32_t* match_of_seed, const float* locs,
                        const float* fluxes, const float* weights,
                        const float* seed_locs, int32_t T, int32_t N, int32_t S,
                        int32_t K, double* moments, float* matched_flux,
                        void* stream);

/* ---- posterior-predictive images and model checks -------- */
/* Does the fitted model reproduce the image?  From the N posterior catalogs of
 * each tile, with lambda[n,p] the rate smcdet_render defines and
 * w~[n] = weights[t,n] / sum_n weights[t,n] (weights nullable: uniform; they
 * must be >= 0 and need not be normalised; a tile whose weights sum to 0 gets
 * NaN):
 *   mean [T,H,W]  sum_n w~[n] lambda[n,p]
 *   var  [T,H,W]  sum_n w~[n] (lambda[n,p] - mean[p])^2  (population form, >= 0)
 * and per catalog, each output nullable, with v(lambda) = noise_additive +
 * noise_multiplicative * lambda (M71) or lambda (POISSON), which must be > 0:
 *   chi2     [T,N]  sum_p (x[p] - lambda)^2 / v(lambda), x = tiled_image
 *   flux_rep [T,N]  sum_p x_rep[n,p]
 *   chi2_rep [T,N]  sum_p (x_rep[n,p] - lambda)^2 / v(lambda)
 * x_rep[n,p] is the draw smcdet_sample_image makes at the same seed and offset
 * for element i = (t*H*W + p)*N + n of a [T,H,W,N] rate array (Philox counter
 * offset + i, the same tags and arithmetic), so smcdet_render followed by
 * smcdet_sample_image and a sum reproduces the two replicate outputs.
 * tiled_image is needed for chi2 only (chi2 without it: SMCDET_EINVAL).  S = 0
 * is legal (the rate is the background; locs and fluxes may then be null).
 * Neither a rate image nor a replicate is stored.  One catalog per wavefront,
 * rendered as smcdet_loglik renders it (registers up to 1024 pixels and S <=
 * 64, the per-wave LDS image up to 4096 pixels, 64-pixel chunks above); the
 * sums over catalogs are float64 sums of w~ (lambda - background) and its
 * square, the sums over pixels float64 as well; all are rounded to float32 once.
 * Determinism: each workgroup writes the partial sums of its chunk of
 * catalogs to `workspace`, a second kernel adds a tile's chunks in chunk
 * order, and no atomic is used: two calls on the same inputs give
 * bit-identical outputs, and mean / var do not depend on which of the
 * per-catalog outputs are requested.
 * workspace: caller-owned, 16-byte aligned, at least
 * smcdet_posterior_image_workspace(model, T, N) bytes (contents on entry are
 * ignored).  With C = min(ceil(N/32), 64) (above 4096 pixels:
 * C = 4 min(ceil(N/4), 64, max(1, 2^20 / (H W)))) that is 8 T + 16 T C H W;
 * the catalogs of a tile are split into ceil(N / (4 ceil(N / (4 C')))) chunks,
 * C' = C (above 4096 pixels: C / 4).  The function returns a negative SMCDET_E*
 * code for a model or shape smcdet_posterior_image refuses.
 * Limits as smcdet_loglik, all SMCDET_EUNSUPPORTED: T <= 65535, the POISSON
 * model up to 4096 pixels, S <= 64 above 4096 pixels; T, N < 1 or S < 0
 * likewise.  A null required buffer (mean, var, workspace; locs / fluxes when
 * S > 0) or a workspace smaller than required (the message names the size):
 * SMCDET_EINVAL.  Everything is checked before any device work.
 * Both entry points were added under SMCDET_ABI_VERSION 20 (purely additive:
 * no existing entry point or struct changed). */
int64_t smcdet_posterior_image_workspace(const smcdet_image_model_t* model,
                                         int32_t T, int32_t N);
int smcdet_posterior_image(const smcdet_image_model_t* model,
                           const float* tiled_image, const float* locs,
                           const float* fluxes, const float* weights, int32_t T,
                           int32_t N, int32_t S, uint64_t seed, uint64_t offset,
                           float* mean, float* var, float* chi2,
                           float* chi2_rep, float* flux_rep, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* ---- posterior calibration summaries --------------------- */
/* The three entry points below were added under SMCDET_ABI_VERSION 20 (purely
 * additive: no existing entry point or struct changed).  None uses a float
 * atomic and every reduction has a fixed order: two calls on the same inputs
 * return the same bits. */
#define SMCDET_TOTALS_MAX_CUTS 8     /* C of smcdet_catalog_totals */
#define SMCDET_SUMMARY_MAX_N 16384   /* N of smcdet_row_summary (keys + payload: 128 KiB of LDS) */
#define SMCDET_SUMMARY_MAX_Q 64      /* quantile levels per call */
#define SMCDET_SUMMARY_MAX_E 65      /* thresholds per row */
#define SMCDET_SUMMARY_LINEAR 0      /* numpy / torch "linear" quantiles (unweighted only) */
#define SMCDET_SUMMARY_LOWER 1       /* smallest value whose cumulative weight reaches q * weight */
#define SMCDET_BOOT_MAX_COLUMNS 256  /* D of smcdet_bootstrap_means */

/* Per-catalog functionals.  counts [T,N] int32, fluxes [T,N,S] (kept sources
 * first, as smcdet_match_catalogs takes them), flux_cuts: C (1..8) floats in
 * HOST memory.  With cnt = min(max(counts[t,n], 0), S):
 *   n_above    [C,T,N] int32  number of slots s < cnt with fluxes[t,n,s] >= flux_cuts[c]
 *   flux_above [C,T,N]        the sum of those fluxes, accumulated in float64 in
 *                             slot order and rounded to float32 once
 * Slots at or past cnt are never looked at, whatever they hold; a NaN inside
 * the counted slots is above no cut.  One pass over fluxes: a workgroup stages
 * 256 catalogs x 16 slots at a time through LDS so that global reads are
 * contiguous, then one thread per catalog walks its slots.
 * C > SMCDET_TOTALS_MAX_CUTS, S > SMCDET_MATCH_MAX_SOURCES or T*N above 2^31-1:
 * SMCDET_EUNSUPPORTED; sizes < 1, a null buffer or a NaN cut: SMCDET_EINVAL. */
int smcdet_catalog_totals(const int32_t* counts, const float* fluxes,
                          const float* flux_cuts, int32_t T, int32_t N, int32_t S,
                          int32_t C, int32_t* n_above, float* flux_above,
                          void* stream);

/* Order statistics along N.  values [A,N,B] float32, summarised along N: a
 * "row" is one (a, b), and every per-row output is indexed [a,b].  NaN in
 * values means "missing" and is excluded from everything.  weights [A,N]
 * (nullable: 1) are >= 0 and shared by the B rows of an a.  q: Q (0..64)
 * doubles in [0,1] in HOST memory.  thresholds [A,B,E] (device, nullable iff
 * E = 0, E <= 65).
 *   n_valid [A,B] int32     entries that are not NaN
 *   weight  [A,B] float64   sum of the weights of the valid entries (= n_valid without weights)
 *   mean    [A,B] float64   sum w v / weight
 *   var     [A,B] float64   sum w (v - mean)^2 / weight, clamped at 0
 *   vmin, vmax [A,B]        the smallest / largest valid value
 *   quantiles [A,B,Q]       (nullable iff Q = 0)
 *   below, at_or_below [A,B,E] float64 (nullable iff E = 0): the weight of the
 *       valid entries < e and <= e (float comparison: -0 == +0; a NaN threshold gives 0)
 * A row with weight == 0 (in particular n_valid == 0) gets NaN for mean, var
 * and the quantiles and 0 for the masses; vmin / vmax are NaN iff n_valid == 0.
 * SMCDET_SUMMARY_LINEAR (weights must be null): with v the valid entries in
 * ascending order, pos = q * (n_valid - 1) in float64, lo = floor(pos) and
 * g = pos - lo: v[lo] when g == 0, else v[lo] + (v[lo+1] - v[lo]) * g formed in
 * float64 from the two float32 order statistics and rounded to float32 once.
 * SMCDET_SUMMARY_LOWER: the smallest valid value whose cumulative weight, in
 * ascending order of (value, index n), is >= q * weight (that float64
 * product); q = 0 gives the minimum.
 * One workgroup per row, b fastest in the grid: the row's keys (the float32
 * mapped to an order-preserving uint32, NaN last; with weights the index n
 * rides along as the low word of a 64-bit key) are bitonic-sorted in LDS, sized
 * to the next power of two >= N; the weighted sums are float64, each thread
 * summing its contiguous sorted segment and one block scan combining them.
 * N > SMCDET_SUMMARY_MAX_N, Q > SMCDET_SUMMARY_MAX_Q, E > SMCDET_SUMMARY_MAX_E or
 * A*B above 2^31-1: SMCDET_EUNSUPPORTED; A, N, B < 1, Q or E < 0, a q outside
 * [0,1], an unknown interpolation, LINEAR with weights, or a null required
 * buffer: SMCDET_EINVAL.  Everything is checked before any device work. */
int smcdet_row_summary(const float* values, const float* weights, int32_t A,
                       int32_t N, int32_t B, const double* q, int32_t Q,
                       int32_t interpolation, const float* thresholds, int32_t E,
                       int32_t* n_valid, double* weight, double* mean,
                       double* var, float* vmin, float* vmax, float* quantiles,
                       double* below, double* at_or_below, void* stream);

/* Bootstrap row means.  values [M,D] float32 (1 <= D <= 256), out [Bn,D]:
 *   out[r,d] = (sum_j values[idx[r,j], d]) / M,  j = 0..M-1,
 * the sum and the quotient in float64, then rounded to float32.  idx is
 * indices [Bn,M] int32 when given (each in [0,M): NOT checked here), else
 *   idx[r,j] = mulhi32(x_{j mod 4}, M),  x = Philox4x32-10(counter (r, j / 4, 0,
 *   tag 0x42530000), key (seed low word, seed high word)),
 * which favours no index by more than M / 2^32 in probability.  One workgroup
 * per replicate: lanes run across D, wave groups across draws, and the groups'
 * float64 partial sums are added through LDS in group order.
 * D > SMCDET_BOOT_MAX_COLUMNS: SMCDET_EUNSUPPORTED; M, D, Bn < 1 or a null
 * buffer: SMCDET_EINVAL. */
int smcdet_bootstrap_means(const float* values, int32_t M, int32_t D,
                           const int32_t* indices, uint64_t seed, int32_t Bn,
                           float* out, void* stream);

/* ---- MCMC convergence diagnostics (added under SMCDET_ABI_VERSION 20) ------
 * Split-R-hat, effective sample size and Monte Carlo standard error of the
 * mean for chains of kept draws (Geyer 1992; Vehtari, Gelman, Simpson,
 * Carpenter & Buerkner 2021, section 3, without the tail term Stan adds to
 * tau).  The reference has no such diagnostics.  DESIGN.md §14 has the
 * definitions and the error bounds. */
#define SMCDET_CHAINS_MAX_CHAINS 32      /* C of smcdet_chain_stats (m = 2C <= 64 split chains) */
#define SMCDET_CHAINS_MAX_DRAWS 1048576  /* m * n draws of one row */
#define SMCDET_CHAINS_MAX_RHO 1024       /* num_rho */
#define SMCDET_CHAINS_LDS_DRAWS 16384    /* rows with m * n <= this keep their draws in LDS */
#define SMCDET_CHAINS_BLOCK_PAIRS 8      /* lag pairs between two tests of the stopping rule */

/* x [R,C,M] float32: R rows, C chains, M kept draws per chain.  split != 0:
 * every chain becomes two of length n = M / 2, draws [0, n) and [M - n, M)
 * (an odd M drops the middle draw, which is never read), m = 2C chains in the
 * order (chain 0 first half, chain 0 second half, chain 1 first half, ...);
 * split == 0: m = C, n = M.  n >= 4.  Per chain j, in float64:
 *   mu_j = mean of its draws,  a_j(t) = (1/n) sum_{i < n-t} (x_i - mu_j)(x_{i+t} - mu_j)
 * and per row
 *   mean = mean_j mu_j,  W = mean_j a_j(0) * n / (n - 1),
 *   B/n = sum_j (mu_j - mean)^2 / (m - 1)  (0 when m = 1),
 *   var_plus = W (n - 1) / n + B/n,  rhat = sqrt(var_plus / W),
 *   rho_t = 1 - (W - mean_j a_j(t)) / var_plus,  rho_0 := 1,
 *   P_k = rho_{2k} + rho_{2k+1} for k = 0, 1, ... while 2k + 1 <= min(n - 1, max_lag);
 *   the sum stops at the first P_k <= 0 (not included): n_pairs = K pairs kept,
 *   stopped = 1, or stopped = 0 when the lags ran out; P'_k = min(P'_{k-1}, P_k);
 *   tau = max(-1 + 2 sum_{k<K} P'_k, 1 / log10(m n)),  ess = m n / tau,
 *   mcse = sqrt(var_plus / ess).
 * Row outputs [R]: mean, W, var_plus, rhat, tau, ess, mcse float64; n_pairs,
 * stopped int32.  Optional (nullable): chain_mean, chain_var [R,m] float64
 * (mu_j and a_j(0) n / (n - 1)); rho [R,num_rho] float32 (nullable iff num_rho
 * = 0): rho_0 .. rho_{num_rho-1}, computed whether or not the sum stopped
 * earlier and whatever max_lag is, NaN for t > n - 1.
 * A row whose read draws hold a NaN or an infinity gets NaN in every float
 * output and n_pairs = stopped = 0; a row with W == 0 keeps mean, W, var_plus
 * and the chain moments and gets NaN for rhat, tau, ess, mcse and rho, n_pairs
 * = stopped = 0.  A row with W > 0 of which some chains are constant is an
 * ordinary row.
 * One workgroup (512 threads) per row.  Phase 1, one wave per chain: the
 * float64 mean, then the centered draws x_i - mu_j formed in float64 and
 * rounded to float32 once, and a_j(0) from the unrounded differences.  Phase
 * 2, SMCDET_CHAINS_BLOCK_PAIRS lag pairs at a time, one pair per wave: lanes
 * stride over i with float64 accumulators, chains in order, one butterfly over
 * the lanes per lag; after every block all threads apply the stopping rule to
 * the same values (workgroup-uniform) and the row ends or takes the next
 * block.  No atomics: the same bits on every run.  Rows with m n <=
 * SMCDET_CHAINS_LDS_DRAWS hold the centered draws in LDS (64 KiB: two
 * workgroups per CU); larger rows keep them in `workspace`, a caller-owned
 * device buffer of smcdet_chain_stats_workspace() floats (workspace_floats
 * says how many it holds; nullable when 0 are needed).
 * C > SMCDET_CHAINS_MAX_CHAINS, m n > SMCDET_CHAINS_MAX_DRAWS, num_rho >
 * SMCDET_CHAINS_MAX_RHO or R m above 2^31-1: SMCDET_EUNSUPPORTED; R, C, M < 1,
 * n < 4, max_lag < 1, num_rho < 0, a null required buffer or a workspace
 * smaller than required: SMCDET_EINVAL.  Everything is checked before any
 * device work. */
int smcdet_chain_stats(const float* x, int32_t R, int32_t C, int32_t M,
                       int32_t split, int32_t max_lag, int32_t num_rho,
                       double* mean, double* W, double* var_plus, double* rhat,
                       double* tau, double* ess, double* mcse, int32_t* n_pairs,
                       int32_t* stopped, double* chain_mean, double* chain_var,
                       float* rho, float* workspace, int64_t workspace_floats,
                       void* stream);
/* Floats of workspace smcdet_chain_stats needs for these shapes (0: the LDS
 * path runs; < 0: refused, smcdet_last_error says why). */
int64_t smcdet_chain_stats_workspace(int32_t R, int32_t C, int32_t M, int32_t split);

/* ---- source-extraction baseline (added under SMCDET_ABI_VERSION 20) --------
 * The classical detector the reference's experiment scripts compare the SMC
 * catalogs with (experiments/[name]/run_sep.py: Source Extractor through sep,
 * grid-searched for F1).  A multi-threshold detector after SExtractor / SEP;
 * the definition below is this project's own and claims no parity with sep
 * (differences: DESIGN.md §15).  The reference has no such code of its own. */
#define SMCDET_EXTRACT_MAX_PIXELS 1024 /* H*W of an image */

/* One problem is image t under setting g; T*G problems, g fastest.
 * images [T,H,W], background [T], sigma [T] float32; thresh, deblend_cont,
 * clean_param [G] float32, minarea [G] int32 (>= 1); deblend_nthresh = n, a
 * power of two in 1..64, for all settings.
 * Detection values: v = image - background[t] and tau = thresh[g] * sigma[t],
 *   one float32 operation each.  tau not finite or <= 0: no detections.  A NaN
 *   pixel is above no threshold.
 * Roots: the 8-connected components of {v > tau} with >= minarea pixels.
 * Ladder, float32, correctly rounded operations only: per root with peak p,
 *   r = p / tau, q = r after log2(n) successive sqrtf, tau_0 = tau,
 *   tau_k = tau_{k-1} * q (k = 1..n-1).
 * Significant tree: a node of level k is an 8-connected component of {pixels
 *   of its parent with v > tau_k}; the root is the node of level 0.  A node C
 *   of level k >= 1 is significant iff sum_C (v - tau_k) > deblend_cont *
 *   F_root, F_root = sum_root v, all in float64 (operands converted first, sums
 *   in any order).  Only children of significant nodes are examined.  The
 *   root's objects are the leaves: significant nodes without a significant
 *   child.  A chain gives one object, the whole root; n = 1 does not deblend.
 *   At most ceil(H/2) * ceil(W/2) objects per problem (leaves are pairwise
 *   non-adjacent).
 * Gather (roots with two or more leaves): leaves are numbered by their
 *   smallest flat pixel index i*W + j; in synchronous sweeps every unassigned
 *   root pixel with an assigned 8-neighbour takes the label of the neighbour
 *   with the largest v (ties: the smaller number), until none is unassigned.
 * Object statistics, float64, pixel (i, j) at (i + 0.5, j + 0.5): F = sum v,
 *   npix, hbar = sum v h / F, wbar likewise; hh, ww, hw the v-weighted means of
 *   squares minus the squares of means; if hh ww - hw^2 < 1/144 add 1/12 to hh
 *   and ww; d = hh ww - hw^2; a^2 = (hh + ww)/2 + sqrt(((hh - ww)/2)^2 + hw^2);
 *   c_hh = ww/d, c_ww = hh/d, c_hw = -2 hw/d; mthresh = (the minarea-th largest
 *   v of the object) - tau, 0 when npix < minarea.
 * Clean (only where clean_param[g] = beta > 0): objects in the order of
 *   descending F (ties: the smaller smallest flat pixel index of the object);
 *   from the second on, object i is absorbed by the first surviving earlier
 *   object j with, U = 100 pi, amp = F_j / (2U), dh = hbar_i - hbar_j, dw alike:
 *     dh^2 + dw^2 < 100 (a_i + a_j)^2,  amp > tau,
 *     alpha = ((amp/tau)^(1/beta) - 1) U / npix_j,
 *     val = 1 + alpha (c_hh,j dh^2 + c_ww,j dw^2 + c_hw,j dh dw),  1 < val < 1e10,
 *     amp val^(-beta) > mthresh_i,
 *   in float64, always with j's original statistics (absorbing updates
 *   nothing); i's pixels take j's label.
 * Outputs: F, hbar, wbar again over the survivors' final pixel sets; survivors
 *   in the same order (descending F, ties to the smaller smallest pixel), the
 *   first K kept; flux = F, loc = (hbar, wbar), each rounded to float32 once.
 *   counts [T,G] int32 = min(found, K); locs [T,G,K,2], NaN past the count;
 *   fluxes [T,G,K], 0 past the count: the est_* layout of
 *   smcdet_match_catalogs with N = G.  Nullable: n_found [T,G] int32, the
 *   survivors before the cap; segmap [T,G,H,W] int32, 0 or the 1-based rank of
 *   the pixel's object in the output order (ranks above K included).
 * One wavefront per problem, its working set in registers and a per-wave LDS
 * slab; H*W <= 64 puts one pixel on each lane (four problems per workgroup),
 * larger images stride the pixels over the lanes.  No atomics, no global
 * scratch: the same bits on every run and for every grouping of the settings
 * into launches.
 * H*W > SMCDET_EXTRACT_MAX_PIXELS, K > SMCDET_MATCH_MAX_SOURCES,
 * deblend_nthresh above 64 or not a power of two, T*G above 2^31-1:
 * SMCDET_EUNSUPPORTED; a null required buffer or a size below 1:
 * SMCDET_EINVAL.  Everything is checked before any device work. */
int smcdet_extract(const float* images, const float* background, const float* sigma,
                   int32_t T, int32_t H, int32_t W,
                   const float* thresh, const int32_t* minarea, const float* deblend_cont,
                   const float* clean_param, int32_t G, int32_t deblend_nthresh, int32_t K,
                   int32_t* counts, float* locs, float* fluxes,
                   int32_t* n_found, int32_t* segmap, void* stream);

/* ---- image-model fit (added under SMCDET_ABI_VERSION 20) ------------------
 * The objective of the reference's image-model fit (experiments/m71/m71.ipynb,
 * "Optimize image model parameters"): the masked Gaussian negative
 * log-likelihood of F calibration fields under the M71 image model with the
 * catalog held fixed, its gradient and its expected Fisher information in the
 * logs of the P = SMCDET_FIT_PARAMS parameters, in float64.
 * Additive: a new entry point; no struct changed. */
#define SMCDET_FIT_PARAMS 10       /* log_theta, grad; information is [P,P] */
#define SMCDET_FIT_TERMS 66        /* 1 + P + P(P+1)/2 sums per workgroup */
#define SMCDET_FIT_BLOCK 16        /* a workgroup owns 16 x 16 pixels */
#define SMCDET_FIT_NORM_BLOCKS 64  /* workgroups of the normaliser launch */
#define SMCDET_FIT_NORM_SUMS 7     /* sums each of them leaves */
#define SMCDET_FIT_MAX_BLOCKS 16777215 /* F * ceil(H/16) * ceil(W/16): one launch's threads < 2^32 */
/* float64 of workspace smcdet_fit_objective needs: the normaliser's partial
 * sums, then SMCDET_FIT_TERMS per pixel workgroup */
#define SMCDET_FIT_WORKSPACE_DOUBLES(F, H, W)                                          \
  ((int64_t)SMCDET_FIT_NORM_BLOCKS * SMCDET_FIT_NORM_SUMS +                            \
   (int64_t)SMCDET_FIT_TERMS * (F) * (((H) + SMCDET_FIT_BLOCK - 1) / SMCDET_FIT_BLOCK) * \
       (((W) + SMCDET_FIT_BLOCK - 1) / SMCDET_FIT_BLOCK))

/* log_theta (host, 10 float64): the logs of
 *   adu_per_nmgy g, sigma1, sigma2, sigmap, beta, b, p0,
 *   noise_multiplicative nm, noise_additive na, background B
 * in this order; the three sigmas are variances (images.py:137-141).
 * Model, every operation in float64 (the float32 inputs are widened exactly):
 *   u(r2) = (exp(-r2/(2 sigma1)) + b exp(-r2/(2 sigma2))
 *            + p0 (1 + r2/(beta sigmap))^(-beta/2)) / (1 + b + p0)
 *   C     = sum of u over the (32R)^2 grid of pixel-centre offsets
 *           (i + 1/2 - 16R, j + 1/2 - 16R), i, j = 0 .. 32R-1 (images.py:122-135)
 *   lambda_p = B + g sum_d f_d u(r2_pd) / C over the stars d < counts[f] whose
 *           (2R+1)^2 window anchored at floor(loc_d) holds pixel p = (ph, pw),
 *           r2_pd = (ph + 1/2 - h_d)^2 + (pw + 1/2 - w_d)^2, in catalog order
 *   v_p   = na + nm lambda_p
 *   nll   = sum over the pixels with mask != 0 of
 *           log(2 pi v_p) / 2 + (x_p - lambda_p)^2 / (2 v_p)
 *   grad[i] = d nll / d log_theta[i]
 *   information[i,j] = sum over the same pixels of
 *           lambda_i lambda_j / v + v_i v_j / (2 v^2),
 *           lambda_i = d lambda / d log_theta[i], v_i likewise (symmetric, both
 *           triangles written).
 * images [F,H,W] float32; mask [F,H,W] uint8, null = every pixel; locs [F,D,2]
 * (row h, column w) and fluxes [F,D] float32; counts [F] int32 (clamped to
 * 0..D), null = D stars in every field.  The F fields share log_theta and
 * their sums add.  D = 0 (locs and fluxes may then be null) gives the
 * background-only result.  R = 0 has an empty normaliser grid (C = 0): the
 * outputs are finite only without stars.
 * Outputs, device: nll [1], grad [10], information [10,10] float64; rate
 * [F,H,W] float32 (nullable): lambda_p of every pixel, masked ones included,
 * rounded to float32 once.  workspace: SMCDET_FIT_WORKSPACE_DOUBLES(F, H, W)
 * float64 of caller-owned device memory (workspace_doubles says how many
 * there are), every word the launches read is written by them first.
 * Three launches on `stream`, no host round trip between them: the
 * normaliser's seven sums over one quadrant of its grid (fixed strides, a
 * fixed tree per workgroup); the pixels (a workgroup per 16 x 16 block, the
 * field's stars staged through LDS 256 at a time and compacted, in catalog
 * order, to those whose clipped window meets the block; per workgroup a fixed
 * tree over its pixels into the workspace); one fixed-order sum over the
 * workgroups.  No atomics: the same bits on every run.
 * A null required buffer, F, H or W < 1, D < 0, psf_radius outside 0..64, a
 * non-finite log_theta or a workspace that is too small: SMCDET_EINVAL.
 * F*H*W or F*D above 2^31-1, or more than SMCDET_FIT_MAX_BLOCKS pixel blocks
 * (F * ceil(H/16) * ceil(W/16): many tiny fields): SMCDET_EUNSUPPORTED.
 * Everything is checked before any device work.  Non-finite locs are not
 * checked here: such a star's window is taken to miss the field (the Python
 * wrapper refuses them). */
int smcdet_fit_objective(const double* log_theta, const float* images, const uint8_t* mask,
                         const float* locs, const float* fluxes, const int32_t* counts,
                         int32_t F, int32_t H, int32_t W, int32_t D, int32_t psf_radius,
                         double* nll, double* grad, double* information, float* rate,
                         double* workspace, int64_t workspace_doubles, void* stream);

/* ---- forced PSF photometry (added under SMCDET_ABI_VERSION 20) ------------
 * Positions are held fixed and the image model is given; the fluxes of all
 * sources of a problem are solved jointly (they blend) by iteratively
 * reweighted least squares, each with its Cramér–Rao error: the crowded-field
 * baseline (DAOPHOT-style flux fitting) next to smcdet_extract, and a
 * per-detection check of condensed posterior catalogs.  Positions are never
 * fitted.  The definition below is this project's own; the reference has no
 * such code.  Additive: a new entry point; no struct changed. */
#define SMCDET_PHOT_MAX_SOURCES 32    /* K: position slots of a problem */
#define SMCDET_PHOT_MAX_ITER 16       /* n_iter */
#define SMCDET_PHOT_FIT_BACKGROUND 1u /* flags: the background is a free parameter */
/* status bits */
#define SMCDET_PHOT_DROPPED 1    /* a source's column is all zero: flux and error NaN */
#define SMCDET_PHOT_SINGULAR 2   /* a squared pivot below 1e-8: the whole problem NaN */
#define SMCDET_PHOT_BACKGROUND 4 /* background[t] is not positive and finite: as singular */

/* One problem is image t = images[t] (model->H x model->W pixels) with
 * position list g: counts [T,G] int32 (clamped to 0..K) and locs [T,G,K,2]
 * float32 (row h, column w), T*G problems, g fastest; the G lists of an image
 * share it (the layout of smcdet_extract's outputs and of a population
 * [T,N,S,2]).  background [T] float32, nullable: per-image B, else
 * model->background; B must be > 0 and finite.  g = adu_per_nmgy (1 for
 * SMCDET_MODEL_POISSON).  Variance v = na + nm * lambda with na =
 * noise_additive, nm = noise_multiplicative; SMCDET_MODEL_POISSON is taken as
 * Gaussian with v = lambda (na = 0, nm = 1), an approximation of its Poisson
 * likelihood that is good where the rates are large.
 * 1. Columns: phi_pk, the normalised PSF of source k at pixel p = (ph, pw), is
 *    non-zero only inside the (2R+1)^2 window anchored at floor(loc_k),
 *    clipped to the image; it is evaluated in float32 exactly as the render
 *    evaluates it (dh = (ph + 0.5f) - h, dw alike, r2 = fma(dh, dh, dw*dw), the
 *    profile's three hardware exponentials) and then widened.  Everything
 *    after this point is float64.
 * 2. Skipped: a slot at or past counts[t,g], and a slot whose location is not
 *    finite: flux 0, error NaN, no parameter.  Dropped: a source whose column
 *    is all zero (its window misses the image): no parameter, flux and error
 *    NaN, status bit SMCDET_PHOT_DROPPED.  The other sources, in slot order,
 *    and then the background with SMCDET_PHOT_FIT_BACKGROUND, are the P free
 *    parameters theta.
 * 3. Initial variance v_p = na + nm * max(x_p, B/4).  The floor B/4 applies to
 *    lambda_p in every later variance: a guard against non-positive
 *    variances, not a model.
 * 4. n_iter (1..SMCDET_PHOT_MAX_ITER) times: A = D^T W D, b = D^T W y with W =
 *    diag(1/v); columns D_k = g phi_k; without SMCDET_PHOT_FIT_BACKGROUND y =
 *    x - B, with it D gains a column of ones and y = x.  A is scaled to a unit
 *    diagonal (A_ij / sqrt(A_ii A_jj), b_i / sqrt(A_ii)), Cholesky-factored
 *    and solved; lambda = D theta (+ B), v = na + nm * max(lambda, B/4).  A
 *    squared pivot of the scaled factor below 1e-8 (or not a number) makes
 *    the problem singular: status bit SMCDET_PHOT_SINGULAR, and every flux and
 *    error of its free and dropped sources, its background_out and its chi2
 *    are NaN.  (Two identical positions, or positions 1e-4 px apart, are
 *    singular; a pair 0.3 px apart has pivots near 1e-2.)  Fluxes are not
 *    constrained to be non-negative.
 * 5. Outputs at the final theta and v, float64: fluxes [T,G,K] (nmgy);
 *    flux_err [T,G,K] = sqrt(diag(I^-1)), I_ij = sum_p D_pi D_pj / v_p +
 *    (nm D_pi)(nm D_pj) / (2 v_p^2), the expected Fisher information over the
 *    free parameters, inverted through the Cholesky factor of its
 *    unit-diagonal scaling (the same pivot rule); background_out [T,G], fitted
 *    or given; chi2 [T,G] = sum_p (x_p - lambda_p)^2 / v_p; n_pixels [T,G] int32
 *    = H*W; n_free [T,G] int32 = P; status [T,G] int32; cov [T,G,K,K]
 *    (nullable): the sources' block of I^-1, symmetric bit for bit, NaN in
 *    the rows and columns of slots that are not free.
 * One wavefront per problem, pixel p on lane p % 64; the normal matrix, its
 * factor and the factor's inverse are packed lower-triangular float64 in the
 * wave's LDS slab (2 x 561 for K = 32 and the background).  Every sum runs in
 * a fixed order (per lane ascending p, then one float64 wave reduction per
 * matrix entry); no atomics: the same bits on every run, in every launch and
 * behind every allocation.
 * H*W > SMCDET_EXTRACT_MAX_PIXELS, K > SMCDET_PHOT_MAX_SOURCES, psf_radius
 * outside 0..64, T*G above 2^31-1: SMCDET_EUNSUPPORTED; a null required
 * buffer, a size below 1, n_iter outside its range, unknown flags, a model
 * background that is not positive and finite when background is null, noise
 * parameters that do not give a positive variance: SMCDET_EINVAL.  Everything
 * is checked before any device work; a per-image background that is not
 * positive and finite is found on the device (SMCDET_PHOT_BACKGROUND). */
int smcdet_forced_photometry(const smcdet_image_model_t* model, const float* images,
                             const int32_t* counts, const float* locs, const float* background,
                             int32_t T, int32_t G, int32_t K, int32_t n_iter, uint32_t flags,
                             double* fluxes, double* flux_err, double* background_out,
                             double* chi2, int32_t* n_pixels, int32_t* n_free, int32_t* status,
                             double* cov, void* stream);

/* ---- PSF-fitting detector (added under SMCDET_ABI_VERSION 20) -------------
 * The finder and the position step of DAOPHOT's loop next to
 * smcdet_forced_photometry: the significance map of an image's residual with
 * the PSF as matched filter, its peaks, and leave-one-out recentring of listed
 * sources.  The definition below is this project's own; the reference has no
 * such code.  Additive: two new entry points; no struct
 * changed.
 *
 * - A problem is one image x[H,W] with one list of n ≤ K sources (`counts
 *   [T,G]`, `locs [T,G,K,2]`, `fluxes [T,G,K]` float32 nmgy).  The G lists share
 *   the image.  This is the layout of `extract_grid` and `forced_photometry`.
 *   A null list means n = 0.
 * - B is the model's background or a per-image `background [T]` > 0.  g is
 *   `adu_per_nmgy`.
 * - The Poisson `ImageModel` is taken as Gaussian with na = 0, nm = 1, g = 1,
 *   as `photometry` does.
 * - φ_pk is the render's own float32 profile: `psf_raw`·`psf_scale` of
 *   `device.h`, the argument formed as in `render.h`.  It is non-zero only in
 *   the (2R+1)² window anchored at floor(loc), clipped to the image.  It is
 *   widened to float64 before use.  Everything after is float64 with fixed
 *   summation order.
 * - Variance from the data: v_p = na + nm·max(x_p, B/4).  This is the first
 *   iteration of `smcdet_forced_photometry`, independent of the list.
 * - A listed source counts if its slot is below the count and its location and
 *   flux are finite.  Other slots are ignored: not subtracted, never moved,
 *   never excluding.
 * - Residual: r_p = x_p − B − g·Σ_k f_k φ_pk over the counted sources.
 * - For a candidate position c: a_c = Σ_p φ_pc r_p / v_p and d_c = Σ_p
 *   φ_pc² / v_p over its clipped window.
 *   - f̂_c = a_c / (g·d_c) is the ML flux of one more source at c with
 *     everything else held.
 *   - snr_c = a_c / √d_c, rounded once to float32.
 *   - A candidate inside the image always has d_c > 0.  A candidate with d_c =
 *     0 has snr −inf.
 * A candidate's position is a float32 (the float64 value below rounded once)
 * when its profile is formed.  counts are clamped to 0..K.  A per-image
 * background that is not positive and finite gives 1/v = NaN: a map of NaN, no
 * peak, no move. */
#define SMCDET_FIND_MAX_CELLS_PER_PIXEL 4 /* cells */
#define SMCDET_FIND_MAX_CELLS 16384       /* (cells H) (cells W) */
#define SMCDET_FIND_MAX_NMS 16            /* nms_radius, cells (clamped on the device) */
#define SMCDET_FIND_MAX_HALF 3            /* half: (2 half + 1)^2 candidates of a move */

/* Map and peaks.  Candidates: `cells` = c in 1..4 per pixel; the grid is cH x
 * cW = cH·cW cells and cell (i, j) sits at ((i+½)/c, (j+½)/c).  thresh [G]
 * float32 and nms_radius [G] int32 (0..16) are per setting g; min_sep >= 0 px.
 * A cell is a peak iff (1) snr >= thresh, compared in float32; (2) it beats
 * every other cell within Chebyshev distance nms_radius by the total order of
 * smcdet_map_peaks (a larger value wins, on equality the lower flat index i·cW
 * + j); (3) its centre lies more than min_sep (Chebyshev, pixels, float64)
 * from every counted source.  Refinement, per axis, with s-, s0, s+ the
 * float32 map values: if both neighbours exist and s- − 2 s0 + s+ < 0 then δ =
 * clamp(½ (s- − s+) / (s- − 2 s0 + s+), ±½), formed in float64, else δ = 0; loc
 * = centre + δ/c (evaluated as ((i+½) + δ)/c), rounded once to float32.  Peaks
 * are ordered by descending snr, then ascending flat index; n_found [T,G]
 * counts all of them and the first K − n are appended.
 * Outputs: counts_out [T,G]; locs_out [T,G,K,2]: the n given slots copied bit
 * for bit, the new ones after, NaN past the count; snr_out and flux_hat
 * [T,G,K] float32 (snr and f̂ at the peak's cell centre): NaN in given and
 * empty slots; map_out [T,G,cH,cW] float32, nullable.  No output may alias an
 * input.
 * One workgroup of 256 threads per problem: r and 1/v per pixel (float64), the
 * float32 map and the peak bits in LDS (16 H W + 4 cH cW + cH cW / 8 + 544
 * bytes: 82.5 KiB at both limits); one thread per cell forms a and d over the
 * cell's clipped window in ascending pixel order by float64 fma, the profile
 * evaluated in place; peak bits are wave ballots and the K − n selections are
 * workgroup arg-maxes.  No atomics; the same bits on every run, whatever the
 * neighbours in the launch.
 * H·W > SMCDET_EXTRACT_MAX_PIXELS, cH·cW > SMCDET_FIND_MAX_CELLS, K >
 * SMCDET_PHOT_MAX_SOURCES, psf_radius outside 0..64, T·G above 2^31-1:
 * SMCDET_EUNSUPPORTED; null required buffers (counts, locs and fluxes are
 * given together or all null), sizes < 1, cells outside 1..4, a min_sep that
 * is negative or not finite, a model background that is not positive and
 * finite when background is null, noise parameters that do not give a
 * positive variance: SMCDET_EINVAL.  Everything is checked before any device
 * work. */
int smcdet_psf_find(const smcdet_image_model_t* model, const float* images,
                    const float* background, const int32_t* counts, const float* locs,
                    const float* fluxes, int32_t T, int32_t G, int32_t K, int32_t cells,
                    const float* thresh, const int32_t* nms_radius, double min_sep,
                    int32_t* counts_out, float* locs_out, float* snr_out, float* flux_hat,
                    int32_t* n_found, float* map_out, void* stream);

/* One Jacobi sweep of position moves.  For every counted source k,
 * independently and from the launch's inputs only: r(k) = r + g·f_k phi_k(old
 * position); candidates old position + (a, b)·step with a, b in −half..half
 * (half in 1..3, step > 0; up to 49, row-major, index (a + half)(2 half + 1) +
 * b + half); snr at each from r(k) and v; the arg-max, the lowest candidate
 * index on ties; the same per-axis parabola on the candidate grid, in units of
 * step; new loc = old + (offset + δ)·step, rounded once.
 * Outputs: locs_out [T,G,K,2] and snr_out [T,G,K], the leave-one-out
 * significance at the chosen candidate.  Slots that do not count are copied
 * unchanged (bit for bit), with snr NaN.
 * One wavefront per problem: the residual's pixel p on lane p % 64, then one
 * (source, candidate) pair per lane, then source k's arg-max and parabola on
 * the lane of its slot; LDS 16 H W + 384 + 4 K (2 half + 1)^2 bytes.  No
 * atomics; the same bits on every run.
 * Limits and errors as smcdet_psf_find; half outside 1..3, a step that is not
 * positive and finite, a null buffer: SMCDET_EINVAL. */
int smcdet_psf_recentre(const smcdet_image_model_t* model, const float* images,
                        const float* background, const int32_t* counts, const float* locs,
                        const float* fluxes, int32_t T, int32_t G, int32_t K, int32_t half,
                        double step, float* locs_out, float* snr_out, void* stream);

/* ---- tile aggregation (smcdet/aggregate.py:8-593, Aggregate) ------------- */
#define SMCDET_AGG_MAX_SOURCES 4096

/* Aggregate.mutate (aggregate.py:176-187 with log_target :105-130): K =
 * mh->num_iters single-component MH iterations on joint tiles of
 * model->H x model->W pixels (T tiles, N particles, S source slots), under
 *   log p(z) + (1 - tau) * [l_c1(z_1) + l_c2(z_2)] + tau * l_p(z),
 * l_p the joint tile's image log-likelihood, l_c1 / l_c2 those of its two
 * halves along `axis` (0: h, 1: w), each rendered from the sources whose axis
 * coordinate is <= dim/2 (first half) or > dim/2 (second), the reference's
 * unjoin (aggregate.py:265-324).  The moved component is drawn from
 * 0..count-1 (slots past the count hold zero flux and never move); proposals,
 * accept rule and the upper-edge freeze as smcdet_mh_sweep.  Reads particle
 * ancestors[t,n] (identity when null) from *_in; counts_out nullable.
 * loglik_parent / loglik_children [T,N] (nullable): l_p and l_c1 + l_c2 of the
 * returned state, from a fresh render (num_iters = 0 evaluates the input
 * state).  acc_rate [T] (nullable) = acceptance rate of the last iteration,
 * with acc_count [2T] as in smcdet_mh_sweep.  Replay layout as
 * smcdet_mh_replay_t (comp must be < count).  tile_boxes (nullable): per
 * joint tile location boxes in place of mh->locs_min/max.
 * workspace (nullable): joint tiles whose image, two rate images and catalog
 * per wave do not fit LDS at 4 waves per workgroup (smcdet_aggregate_workspace
 * > 0; M71 model, up to 65536 pixels and 4096 sources) keep them in this
 * caller-owned device buffer of smcdet_aggregate_workspace() floats and read
 * the tile image from global memory. */
int smcdet_aggregate_sweep(const smcdet_image_model_t* model,
                           const smcdet_prior_t* prior, const smcdet_mh_t* mh,
                           int32_t axis, const float* tiled_image,
                           const float* temperature, int32_t T, int32_t N,
                           int32_t S, const int64_t* ancestors,
                           const float* counts_in, const float* locs_in,
                           const float* fluxes_in, float* counts_out,
                           float* locs_out, float* fluxes_out, uint64_t seed,
                           uint64_t offset, const smcdet_mh_replay_t* replay,
                           float* loglik_parent, float* loglik_children,
                           float* acc_rate, int32_t* acc_count,
                           const float* tile_boxes, float* workspace, void* stream);
/* Floats of workspace smcdet_aggregate_sweep needs for these shapes (0: the
 * LDS path runs; < 0: unsupported, smcdet_last_error says why). */
int64_t smcdet_aggregate_workspace(const smcdet_image_model_t* model, int32_t T,
                                   int32_t N, int32_t S);

/* Aggregate.temper (aggregate.py:140-174), per count group: the particles of
 * each joint tile are sorted by count and split into G segments (count
 * groups) given by seg_tile[g], seg_start[g] (first particle within the
 * tile) and seg_len[g] (device int32 arrays).  With l = loglik_parent -
 * loglik_children, delta[g] solves exp(2 LSE(delta*l) - LSE(2 delta*l)) =
 * ess_threshold_prop * seg_len[g] on (0, 1 - tau] (brentq, xtol = rtol =
 * 1e-6), or is 1 - tau when the ESS there is still above it. */
int smcdet_aggregate_temper(const float* loglik_parent,
                            const float* loglik_children,
                            const float* temperature, int32_t T, int32_t N,
                            int32_t G, const int32_t* seg_tile,
                            const int32_t* seg_start, const int32_t* seg_len,
                            double ess_threshold_prop, float* delta,
                            void* stream);

/* Aggregate.update_weights (aggregate.py:439-483) + resample_intracount
 * (:485-521) per count group, after the caller has set temperature[t] to
 * temperature_prev[t] + the minimum of the tile's delta[g] (aggregate.py:171-
 * 174).  Per segment: log_weights_unnorm = (temperature - temperature_prev) *
 * l (float32), weights_intracount = softmax within the segment,
 * log_norm_const[g] += log mean exp(log w) (in place), ess[g] = 1 / sum w^2.
 * idx [T,N] (nullable): tile-local multinomial resampling indices drawn within
 * each segment from its weights (u [T,N] replays the uniforms). */
int smcdet_aggregate_reweight(const float* loglik_parent,
                              const float* loglik_children,
                              const float* temperature,
                              const float* temperature_prev, int32_t T,
                              int32_t N, int32_t G, const int32_t* seg_tile,
                              const int32_t* seg_start, const int32_t* seg_len,
                              float* log_weights_unnorm,
                              float* weights_intracount, float* log_norm_const,
                              float* ess, uint64_t seed, uint64_t offset,
                              const float* u, int64_t* idx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMCDET_HIP_H */
