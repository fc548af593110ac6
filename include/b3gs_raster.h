/*
 * b3gs_raster.h -- C ABI of libb3gs_raster.so, the MI355X-native differentiable Gaussian
 * rasterizer that sits behind the reference's `diff_gaussian_rasterization._C` extension.
 *
 * Boundary it replaces (reference = hanl2010/Binocular3DGS; the extension's own source is an
 * un-vendored submodule, .gitmodules:1-3, so the citations are the reference's call sites):
 *   gaussian_renderer/__init__.py:36-49   GaussianRasterizationSettings  -> B3gsScene scalars/matrices
 *   gaussian_renderer/__init__.py:85-93   rasterizer(means3D=..., ...)   -> b3gs_forward()
 *   train.py:149 (total_loss.backward())  _RasterizeGaussians.backward   -> b3gs_backward()
 *   (upstream `_C.mark_visible`, unused by the reference)                -> b3gs_mark_visible()
 *
 * Rules of the ABI:
 *   - plain C: pointers, sizes, a stream handle; no torch / C++ types cross it
 *   - every pointer is a DEVICE pointer unless the name says `host_`
 *   - the caller owns all memory.  The three opaque state buffers (geometry / binning / image)
 *     are obtained through caller-supplied allocation callbacks, exactly like the upstream
 *     extension asks torch to resize three uint8 tensors; they must stay alive until
 *     b3gs_backward() for the same view has been enqueued
 *   - all work is enqueued on `stream`; b3gs_forward() blocks the calling host thread once
 *     (to read back num_rendered) -- b3gs_forward_capacity() is the sync-free variant
 *   - every function returns B3GS_OK or a negative B3gsStatus and never throws
 *   - no global mutable state: re-entrant per stream / per device (one process per GPU)
 */
#ifndef B3GS_RASTER_H
#define B3GS_RASTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define B3GS_ABI_VERSION 18
#define B3GS_TILE 16 /* 16x16-pixel tiles: the binning granularity (bit-exact with the oracle) */

typedef enum B3gsStatus {
  B3GS_OK = 0,
  B3GS_ERR_ARG = -1,      /* inconsistent arguments (exactly one of shs/colors_precomp, ...) */
  B3GS_ERR_ALLOC = -2,    /* an allocation callback returned NULL */
  B3GS_ERR_HIP = -3,      /* a HIP runtime call failed; see b3gs_last_error() */
  B3GS_ERR_CAPACITY = -4, /* b3gs_forward_capacity: binning capacity too small */
  B3GS_ERR_NO_DEVICE = -5
} B3gsStatus;

typedef void* b3gs_stream_t; /* hipStream_t */

/* Allocation callback: return a device pointer to at least `bytes` bytes, 256-byte aligned,
 * or NULL.  Mirrors the resize-a-uint8-tensor lambdas of the upstream torch binding. */
typedef char* (*b3gs_alloc_fn)(void* user, size_t bytes);

/* One view of one Gaussian cloud.  Field meaning = the 12 settings of
 * gaussian_renderer/__init__.py:36-49 plus the 8 tensors of :85-93. */
typedef struct B3gsScene {
  int32_t P;           /* number of Gaussians (< 2^24) */
  int32_t D;           /* active SH degree, 0..3 (raster_settings.sh_degree) */
  int32_t M;           /* SH coefficients per channel stored in `shs` (0 when shs == NULL) */
  int32_t W, H;        /* image_width, image_height */
  float tan_fovx, tan_fovy;
  float scale_modifier;
  int32_t prefiltered; /* reference always passes False */
  int32_t debug;       /* sync + check after every kernel */
  const float* background;     /* [3] */
  const float* means3D;        /* [P,3] */
  const float* shs;            /* [P,M,3] or NULL */
  const float* colors_precomp; /* [P,3]   or NULL  (exactly one of shs / colors_precomp) */
  const float* opacities;      /* [P,1] */
  const float* scales;         /* [P,3]   or NULL */
  const float* rotations;      /* [P,4] (w,x,y,z), used as given  or NULL */
  const float* cov3D_precomp;  /* [P,6] (xx,xy,xz,yy,yz,zz) or NULL (exactly one of cov3D / scales+rotations) */
  const float* viewmatrix;     /* [4,4] row-vector convention: [x y z 1] @ viewmatrix (scene/cameras.py:55) */
  const float* projmatrix;     /* [4,4] full projection, same convention (scene/cameras.py:57) */
  const float* campos;         /* [3] */
} B3gsScene;

/* Sizes of the opaque buffers (bytes).  geometry depends on P, image on W*H, binning on N. */
size_t b3gs_geometry_bytes(int32_t P);
size_t b3gs_image_bytes(int32_t W, int32_t H);
size_t b3gs_binning_bytes(int32_t P, int64_t num_rendered);

/* Forward: colour [3,H,W], depth [1,H,W] (= sum z a T, un-normalised), alpha [1,H,W] (= sum a T),
 * radii [P] int32 (0 = culled).  *host_num_rendered receives N (tile instances). */
int b3gs_forward(const B3gsScene* scene,
                 b3gs_alloc_fn geometry_alloc, void* geometry_user,
                 b3gs_alloc_fn binning_alloc, void* binning_user,
                 b3gs_alloc_fn image_alloc, void* image_user,
                 float* out_color, float* out_depth, float* out_alpha, int32_t* radii,
                 int32_t* host_num_rendered, b3gs_stream_t stream);

/* Sync-free forward for callers that keep persistent scratch (the build's own training step):
 * all three buffers are pre-sized by the caller; binning has room for `binning_capacity`
 * instances.  N is written to *device_num_rendered (device int32) and nothing is read back.
 * If N > binning_capacity the images are left untouched and *device_num_rendered still
 * holds the required N (caller checks it at its next natural sync and retries). */
int b3gs_forward_capacity(const B3gsScene* scene, char* geometry, char* binning, int64_t binning_capacity,
                          char* image, float* out_color, float* out_depth, float* out_alpha, int32_t* radii,
                          int32_t* device_num_rendered, b3gs_stream_t stream);

/* Backward.  Pixel gradients: dL_dcolor [3,H,W] (required), dL_ddepth / dL_dalpha [1,H,W] or NULL.
 * Outputs (all fully overwritten, culled Gaussians get zeros):
 *   dL_dmeans2D [P,3]  (x,y in the NDC-scaled units the densifier thresholds, z = 0)
 *   dL_dcolors  [P,3]  gradient of the per-Gaussian RGB (= grad of colors_precomp)
 *   dL_dopacity [P,1], dL_dmeans3D [P,3], dL_dcov3D [P,6]
 *   dL_dsh [P,M,3] (NULL if colours were precomputed), dL_dscales [P,3], dL_drotations [P,4]
 *   (NULL if cov3D was precomputed)
 * num_rendered < 0 means "read N from the image buffer" (forward_capacity path). */
int b3gs_backward(const B3gsScene* scene, int32_t num_rendered, const int32_t* radii,
                  const char* geometry, const char* binning, const char* image,
                  const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                  float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                  float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations,
                  b3gs_stream_t stream);

/* ---- fused-activation ("raw parameter") path ------------------------------------------------
 * The reference computes the rasterizer's inputs with five small PyTorch kernels per view
 * (scene/gaussian_model.py:95-115: exp, normalize, sigmoid, cat) and autograd adds five more in
 * the backward plus one gradient-accumulation add per parameter per view.  These two entry
 * points take the PRE-activation parameters, apply the activations inside the per-Gaussian
 * kernels and accumulate (+=) the gradients straight into parameter-shaped buffers (e.g. views
 * into one flat slab that is later all-reduced).  Same arithmetic, same outputs; not part of the
 * reference's extension API -- used by the build's own training step. */
typedef struct B3gsRawParams {
  const float* xyz;            /* [P,3]                                   (GaussianModel._xyz) */
  const float* features_dc;    /* [P,1,3]                                 (_features_dc) */
  const float* features_rest;  /* [P,M-1,3] (may be NULL when M == 1)     (_features_rest) */
  const float* scaling;        /* [P,3]  scales    = exp(scaling)         (_scaling) */
  const float* rotation;       /* [P,4]  rotations = normalize(rotation)  (_rotation) */
  const float* opacity;        /* [P,1]  opacity   = sigmoid(opacity)     (_opacity) */
} B3gsRawParams;
typedef struct B3gsRawGrads {  /* accumulated into (+=); same shapes as B3gsRawParams */
  float* xyz; float* features_dc; float* features_rest; float* scaling; float* rotation; float* opacity;
  /* Optional sparse-row mode of b3gs_backward_raw_accumulate[_range] with overwrite != 0 (NULL = dense; ignored by
   * every other entry point): a bitmap of ceil(P / 64) words, bit (i & 63) of word (i >> 6) = "Gaussian i received a
   * gradient from at least one view of the call".  Rows whose bit is clear are NOT stored (most Gaussians of an
   * iteration: ~80 % at the headline workload) -- their content is stale and only a consumer that reads the bitmap
   * (b3gs_adam_step with row_mask) may use the buffers.  Range calls need first % 64 == 0. */
  uint64_t* touched_rows;
} B3gsRawGrads;

/* Sync-free forward (see b3gs_forward_capacity) on raw parameters.  `view` supplies P, D, M (= total
 * SH coefficients per channel), W, H, tan_fov*, scale_modifier, prefiltered, debug, background,
 * viewmatrix, projmatrix, campos; its per-Gaussian tensor pointers are ignored. */
/* `phases`: bit 0 = per-Gaussian projection + binning (ends with the tile lists in `binning`), bit 1 =
 * blend forward (the three output images); 3 = both.  A caller rendering several views runs phase 1 of
 * each view on its own stream and then ONE b3gs_blend_forward_batch() for all of them. */
int b3gs_forward_raw(const B3gsScene* view, const B3gsRawParams* params, char* geometry, char* binning,
                     int64_t binning_capacity, char* image, float* out_color, float* out_depth, float* out_alpha,
                     int32_t* radii, int32_t* device_num_rendered, int phases, b3gs_stream_t stream);

/* The whole forward of up to 8 views of the SAME Gaussians, every stage one launch for all views:
 * the projection reads and activates each Gaussian once for all views, the radix passes / scans / emission
 * / blend take the views as blockIdx.y (a single view's pass is ~250 workgroups on 256 CUs: latency-bound).
 * depth_order_from: -1 = this view sorts its own depth keys; k = reuse view k's depth order -- valid iff
 * both view matrices have the same z row, which is what the binocular shifted cameras are (the translation is
 * along the camera x axis, utils/pose_utils.py:148-163): one depth sort per input/shifted pair.
 * Views share P, M, D, scale_modifier; W, H may differ.  phases as in b3gs_forward_raw. */
typedef struct B3gsForwardView {
  const B3gsScene* view;
  char* geometry;
  char* binning;
  int64_t binning_capacity;
  char* image;
  float* out_color;
  float* out_depth;
  float* out_alpha;
  int32_t* radii;
  int32_t* device_num_rendered;  /* N = tile instances binned (segment 1 + segment 2) */
  int32_t depth_order_from;
  /* Two-round ("termination-aware") binning.  0 < seg1_fraction < 1: only the nearest ceil(seg1_fraction * P) Gaussians
   * of the depth order -- rounded UP to a whole number of the scan's 4096-Gaussian tiles; when that reaches P (always below
   * 4097 Gaussians) the forward is binned in one round -- are binned first (segment 1 of every tile list); the blend
   * forward marks the tiles whose pixels
   * all terminated inside it (T < 1e-4: nothing behind can contribute), and the remaining Gaussians are binned into the
   * OTHER tiles only (segment 2), which are then blended again over segment 1 + segment 2.  Images, n_contrib-relative
   * gradients and the order inside every list are those of one-round binning; only the instances no pixel could have
   * reached are never emitted or sorted.  0 or >= 1: one round.  All views of a batch use views[0]'s value.
   * The `image` buffer carries a prediction from one two-round forward to the next one into the SAME buffer: the tiles
   * left unterminated are predicted open and receive their complete list in segment 1 (then nothing is left for segment
   * 2 on a settled scene).  Any buffer content is valid -- the prediction only moves work between the rounds, the
   * results do not depend on it -- but a caller that wants the saving keeps one image buffer per camera (and zeroes a
   * fresh one). */
  float seg1_fraction;
  /* ABI 6 -- overflow that cannot corrupt a step (both optional, device int32 words the caller keeps across forwards):
   * high_water    <- max(high_water, N)           by the binning kernels themselves (no extra launch);
   * overflow_flag <- 1 (sticky) when N > binning_capacity, i.e. this view was rendered from truncated tile lists.
   * b3gs_adam_step(skip_if_nonzero = overflow_flag) and B3gsDensifyStats::skip_if_nonzero then turn every step from
   * the overflowing one on into a no-op for the parameters, the Adam state and the statistics, until the host has read
   * the flag, grown the buffers and cleared it: the steps since the last check can really be repeated.
   * Bits of the word: 0 = capacity, 1 = a depth key outside the 27-bit span (depth_key_bits), 2 (ABI 7) = the second
   * binning round's persistent launch timed out at its grid barrier (its workgroups were not co-resident: a shared or
   * partitioned device) -- the repaired tiles of that forward are wrong, the step is dropped like an overflowing one and
   * the caller goes back to one round (seg1_fraction = 0); 3 (ABI 7) = a TRUSTED depth-order hint was wrong
   * (hint_trusted): the view was rendered from another view's depth order. */
  int32_t* high_water;
  int32_t* overflow_flag;
  /* 27: the caller vouches that every visible Gaussian's depth key (float bits of view z > 0.2) lies within 2^27 of the
   * bits of 0.2f, i.e. z < ~13107: the depth sort then runs three 9-bit passes instead of four 8-bit ones (same
   * permutation).  The library CHECKS it: a key outside the span raises bit 1 of *overflow_flag (required non-NULL for
   * this mode), which drops the step like a capacity overflow; the caller then falls back to 0.  0 (or 32): full sort. */
  int32_t depth_key_bits;
  /* != 0: `image` is a fresh allocation with undefined content (not the buffer of an earlier forward): nothing is read
   * from it -- neither the tile order the previous backward of a persistent buffer leaves for the next forward nor the
   * open-tile prediction (two-round binning is then off).  A caller that re-uses image buffers across forwards zeroes a
   * new one ONCE and passes 0.  All views of a batch use views[0]'s value. */
  int32_t fresh_image;
  /* ABI 7 -- depth order of an EARLIER forward, checked on the device.  depth_order_hint (may be NULL) is the geometry
   * buffer of a completed earlier b3gs_forward_raw_batch() of the same P Gaussians (same depth_key_bits) on this stream;
   * it must stay alive until this forward has run.  The projection compares every depth key of this view with the key that
   * forward stored (keys are a function of the Gaussian's position and the z row of the view matrix only: the binocular
   * partner of train.py:124-128 differs from its input view by a translation along the camera x axis, so all keys are
   * equal); any difference -- another camera, moved Gaussians, a different near-plane cull -- sets *hint_mismatch
   * (device int32, must be ZERO on entry, required when a hint is given) and this view's own depth sort runs as usual.
   * While the word stays zero the sort launches exit at once and the earlier order is adopted: same lists bit for bit,
   * ~60 us less per view at 1M Gaussians.  The answer never depends on the caller being right about the hint.
   * Only for views that sort their own keys (depth_order_from == -1). */
  const char* depth_order_hint;
  int32_t* hint_mismatch;
  /* != 0: the caller KNOWS the keys are equal (it built both view matrices and their z rows are the same bits): the depth
   * sort is not even launched (an idle launch is ~5 us on this part, nine of them per view).  Still checked: a key that
   * differs sets *hint_mismatch and raises bit 3 of *overflow_flag (required non-NULL then) -- that view was rendered from
   * a wrong depth order, the step is dropped like an overflowing one and the caller stops trusting its knowledge.
   * With depth_order_from == k - 1 (view k shares the order of the PREVIOUS view of the batch, no hint buffer involved): the
   * projection compares this view's depth keys with that view's and raises bit 3 of *overflow_flag (required non-NULL) on
   * a difference -- the same check for a pair rendered in one batch.  0: the pair is the caller's word (fused path). */
  int32_t hint_trusted;
  /* ABI 8 (may be NULL): [P] bytes <- radii > 0, render()'s `visibility_filter` (gaussian_renderer/__init__.py:99), written
   * by the projection next to the radius instead of by a compare kernel per render afterwards. */
  uint8_t* visible;
  /* ABI 10 -- which tiles a Gaussian is binned into.  0 (default): the tiles its alpha >= 1/255 footprint can reach
   * ("tight" binning: same images, shorter lists -- every list is an order-preserving subsequence of the reference's).
   * != 0: every tile of the reference's rectangle (radius = ceil(3 sigma)): point_list / ranges
   * are then the reference's bit for bit, as on the b3gs_forward() surface.  All views of a batch use views[0]'s value.
   * (Until ABI 9 this was a process-wide environment switch read inside the library.) */
  int32_t reference_binning;
} B3gsForwardView;
int b3gs_forward_raw_batch(int32_t nviews, const B3gsForwardView* views, const B3gsRawParams* params, int phases,
                           b3gs_stream_t stream);

/* Blend (per-tile alpha compositing) of up to 8 views in ONE launch each way.  One view's ~1900 tiles fill
 * the 256 CUs roughly once, so a per-view launch pays its own tail; batched, the dispatcher packs the tiles
 * of all views (MI355X, 1M Gaussians, 800x600: forward 126 us per view alone, 74 us per view batched).
 * forward: needs every view's b3gs_forward_raw(..., phases = 1) complete on a stream `stream` waits for;
 * backward: = phase 1 of b3gs_backward_raw for every view (own zeroed `scratch` each). */
typedef struct B3gsBlendView {
  const B3gsScene* view;
  const char* geometry;
  const char* binning;
  const char* image;
  float* out_color;          /* forward */
  float* out_depth;
  float* out_alpha;
  const float* dL_dcolor;    /* backward */
  const float* dL_ddepth;    /* may be NULL */
  const float* dL_dalpha;    /* may be NULL */
  float* scratch;            /* backward: b3gs_backward_scratch_floats(P) zeroed floats */
  int64_t binning_capacity;  /* the capacity `binning` was carved with in the forward (two-word instance layout: locates
                              * nothing the blend reads; kept for symmetry with B3gsForwardView) */
} B3gsBlendView;
int b3gs_blend_forward_batch(int32_t nviews, const B3gsBlendView* views, b3gs_stream_t stream);
int b3gs_blend_backward_batch(int32_t nviews, const B3gsBlendView* views, b3gs_stream_t stream);

/* Backward of b3gs_forward_raw.  `scratch` holds b3gs_backward_scratch_floats(P) floats that must be
 * ZERO on entry and are left zero on exit (persistent across views: no per-view memset).
 * dL_dmeans2D ([P,3], optional) is overwritten with the screen-space mean gradients.
 * `phases`: bit 0 = blend backward (pixel gradients -> per-Gaussian sums in `scratch`), bit 1 = per-Gaussian
 * chain rule + accumulation into `grads`; 3 = both.  Views rendered concurrently on several streams call
 * phase 1 in parallel (own scratch each) and order their phase-2 calls with stream events, because phase 2
 * read-modify-writes the shared gradient buffers without atomics. */
size_t b3gs_backward_scratch_floats(int32_t P);
int b3gs_backward_raw(const B3gsScene* view, const B3gsRawParams* params, const int32_t* radii, const char* geometry,
                      const char* binning, const char* image, const float* dL_dcolor, const float* dL_ddepth,
                      const float* dL_dalpha, float* scratch, const B3gsRawGrads* grads, float* dL_dmeans2D,
                      int phases, b3gs_stream_t stream);

/* Phase 2 for SEVERAL views in one pass over the Gaussians (at most 8 per call): parameters are read
 * once, each view contributes its phase-1 sums (read and reset), the gradients are written once --
 * `overwrite` != 0 stores them (culled-everywhere Gaussians get zeros: no zero-fill of `grads` needed),
 * 0 accumulates (+=).  Every view must have completed b3gs_backward_raw(..., phases = 1) with its OWN
 * scratch on a stream that `stream` has been made to wait for.  All views share P, M, D, scale_modifier. */
typedef struct B3gsFusedView {
  const B3gsScene* view;     /* camera fields as passed to b3gs_forward_raw */
  const int32_t* radii;
  const char* geometry;
  float* scratch;            /* that view's phase-1 sums; left zero */
  float* dL_dmeans2D;        /* optional [P,3] */
  int32_t densify_stats;     /* != 0: this view feeds the densification statistics (train.py:178-179) */
} B3gsFusedView;
/* Densification statistics of scene/gaussian_model.py:147-152,409-411 and train.py:178, updated for every
 * Gaussian visible (radii > 0) in a view with densify_stats set:
 *   xyz_gradient_accum += ||dL_dmeans2D[:2]||,  denom += 1,  max_radii2D = max(max_radii2D, radii). */
typedef struct B3gsDensifyStats {
  float* xyz_gradient_accum; /* [P,1] */
  float* denom;              /* [P,1] */
  float* max_radii2D;        /* [P]   */
  const int32_t* skip_if_nonzero;  /* ABI 6, may be NULL: device word; != 0 -> the statistics are left untouched (see
                                    * B3gsForwardView::overflow_flag) */
} B3gsDensifyStats;
int b3gs_backward_raw_accumulate(int32_t nviews, const B3gsFusedView* views, const B3gsRawParams* params,
                                 const B3gsRawGrads* grads, int32_t overwrite, const B3gsDensifyStats* stats,
                                 b3gs_stream_t stream);
/* The same for the Gaussians [first, first + count) only.  Every pointer (parameters, gradients, statistics,
 * per-view state) is still indexed by the GLOBAL Gaussian index, so a caller that keeps the gradients of a range
 * in one contiguous block passes block_base - first * row_width.  Disjoint ranges issued back to back let the
 * gradient all-reduce of one range overlap the chain rule of the next (step.ViewShardedStep, data parallel). */
int b3gs_backward_raw_accumulate_range(int32_t nviews, const B3gsFusedView* views, const B3gsRawParams* params,
                                       const B3gsRawGrads* grads, int32_t overwrite, const B3gsDensifyStats* stats,
                                       int32_t first, int32_t count, b3gs_stream_t stream);

/* ---- fused optimiser step -----------------------------------------------------------
 * Adam exactly as torch.optim.Adam (no amsgrad, no weight decay) for up to 8 parameter tensors with their
 * own learning rates in ONE launch: the reference's six parameter groups (scene/gaussian_model.py:154-167,
 * eps = 1e-15) and optimizer.step() at train.py:196-198.  `device_step` (int32 on the device, incremented
 * by the call unless bump_step_after == 0: a step issued as several calls over disjoint slices -- the pipelined
 * data-parallel tail -- bumps on the last one) keeps the bias correction replayable from a HIP graph.  opacity_decay > 0 additionally
 * applies  o <- logit(sigmoid(o) * opacity_decay)  to segment `opacity_segment` (gaussian_model.py:307-309,
 * train.py:171-173): after its update when opacity_decay_first == 0; when != 0, in the reference's order -- the
 * decay runs BEFORE optimizer.step() (train.py:171-173 vs :196-198), so the Adam update (computed from the gradient at
 * the un-decayed value) is subtracted from the decayed logit.  A segment with count == 0 may carry NULL pointers
 * (features_rest at SH degree 0). */
typedef struct B3gsAdamSegment {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t count;  /* floats */
  float lr;
  int32_t row_len;    /* floats per Gaussian row of this tensor; only read when row_mask != NULL (0 = segment not masked) */
  int32_t first_row;  /* Gaussian index of the segment's first float (a segment starts at a row boundary when masked) */
  const float* lr_dev; /* ABI 7, may be NULL: a device float that REPLACES `lr` (the position learning rate follows a
                        * schedule, train.py:83: a step replayed as a HIP graph reads it from device memory) */
} B3gsAdamSegment;
/* `row_mask` (may be NULL): the touched_rows bitmap of B3gsRawGrads.  Element e of a segment with row_len > 0 belongs to
 * Gaussian first_row + e / row_len; when that Gaussian's bit is clear the gradient is taken as 0 WITHOUT reading it
 * (moments and parameter still follow Adam: same result as a dense zero gradient, 4 of 28 bytes per float less). */
/* ABI 7: `device_step` points to B3GS_ADAM_STEP_WORDS int32 words the optimiser owns, ZERO apart from the first:
 * {step, completion counter, 64 first-level completion counters a cache line apart} -- the workgroup that finishes last
 * advances the step (no second launch); two levels because thousands of workgroups arriving at one address cost ~15 ns
 * each (85 us of the launch at 500k Gaussians).  Optimisers stepping concurrently on several streams own their words.  `skip_if_nonzero` (may be NULL): device word; when it is != 0 at launch time the call changes
 * NOTHING (parameters, moments, step counter): the update of a step rendered from truncated tile lists is dropped on the
 * device, without a host round trip (B3gsForwardView::overflow_flag). */
#define B3GS_ADAM_STEP_WORDS (2 + 64 * 32)
int b3gs_adam_step(int32_t nseg, const B3gsAdamSegment* segs, int32_t* device_step, float beta1, float beta2,
                   float eps, float opacity_decay, int32_t opacity_segment, int32_t opacity_decay_first,
                   int32_t bump_step_after, const uint64_t* row_mask, const int32_t* skip_if_nonzero,
                   b3gs_stream_t stream);

/* ---- fused loss block ----------------------------------------------------------------
 * Value and pixel gradients of the per-pair training loss of train.py:123-148 in 4 launches:
 *   total = (1-lambda_dssim) L1(image, gt) + lambda_dssim (1 - SSIM(image, gt))
 *         + L1(warp(shifted, disp) mask, gt mask) + lambda_smooth smooth(disp mask, gt)     [shifted_image != NULL]
 *         + mean(|alpha| alpha_weight)                                                      [alpha_weight  != NULL]
 * disp = focal_x (-trans_dist) / (depth + 1e-5); warp / mask = utils/graphics_utils.py:80-125; smooth =
 * utils/loss_utils.py:68-91; SSIM = utils/loss_utils.py:36-66.  alpha_weight is (1 - gt_alpha_mask) or the DTU
 * background mask (train.py:139-143).  All images are [C,H,W] fp32 device tensors.  The four gradient images are
 * OVERWRITTEN with d(total)/d(input) * grad_scale; parts (8 device floats) receives total, Ll1, ssim,
 * l1_masked, smooth, alpha_loss.  No host synchronisation: graph-capturable. */
typedef struct B3gsLossIO {
  int32_t W, H;
  const float* image;          /* [3,H,W] primary render */
  const float* depth;          /* [1,H,W] */
  const float* alpha;          /* [1,H,W] */
  const float* gt_image;       /* [3,H,W] */
  const float* shifted_image;  /* [3,H,W] or NULL */
  const float* alpha_weight;   /* [1,H,W] or NULL */
  float focal_x, trans_dist, lambda_dssim, lambda_smooth, grad_scale;
  float* dL_dimage;            /* [3,H,W] */
  float* dL_ddepth;            /* [1,H,W] */
  float* dL_dalpha;            /* [1,H,W] */
  float* dL_dshifted;          /* [3,H,W]; required iff shifted_image */
  float* parts;                /* [8] */
  /* (`workspace` below.)  ABI 7, last field of the struct: trans_dist_dev (may be NULL) -- a device float that REPLACES
   * `trans_dist` when given: the shift of the binocular partner is drawn anew every iteration (train.py:125-126), and an
   * iteration replayed as a HIP graph can only see it through device memory. */
  float* workspace;            /* b3gs_loss_workspace_floats(W, H) floats.  ABI 7: its first 512 floats (the partial-sum
                                * slots) must be ZERO before the first call with this workspace; every call leaves them zero
                                * (self-cleaning: no memset per call).  One workspace per pair in flight. */
  const float* trans_dist_dev;
} B3gsLossIO;
size_t b3gs_loss_workspace_floats(int32_t W, int32_t H);
int b3gs_binocular_loss(const B3gsLossIO* io, b3gs_stream_t stream);
/* The same for up to 8 pairs (ios[0..npairs)) with ONE launch per stage: the images of one pair are ~1900 tiles. */
int b3gs_binocular_loss_batch(int32_t npairs, const B3gsLossIO* ios, b3gs_stream_t stream);

/* ---- densify / clone / split / prune ------------------------------------------------------
 * Net effect of the reference's densify_and_prune (scene/gaussian_model.py:393-407 with :258-391) including the
 * Adam-state surgery, as: b3gs_densify_classify (per-Gaussian decisions) -> caller forms the three exclusive prefix
 * sums and their totals (the only host read-back) -> b3gs_densify_scatter (one pass writes every surviving /
 * new row of the six parameter tensors and of exp_avg / exp_avg_sq).
 * Tensor order everywhere: xyz[P,3], features_dc[P,3], features_rest[P,3(M-1)], scaling[P,3], rotation[P,4],
 * opacity[P] (raw, pre-activation).  flags[i]: bit 0 = original kept, bit 1 = clone appended, bit 2 = two split
 * children appended.  Output rows: kept originals | clones | children k=0 | children k=1, each in index order
 * (the reference's order); new rows get zero Adam state.  noise: [2,P,3] standard-normal samples addressed by
 * the ORIGINAL index (child k of Gaussian i uses noise[k][i]): the caller owns the random stream, so replicas
 * that share it stay identical.  max_screen_size <= 0: opacity rule only (what train.py passes). */
typedef struct B3gsDensifyIO {
  int32_t P, M;
  const float* param[6];
  const float* exp_avg[6];        /* all six, or all NULL */
  const float* exp_avg_sq[6];
  const float* xyz_gradient_accum; /* [P] */
  const float* denom;              /* [P] */
  float grad_threshold, min_opacity, extent, percent_dense, max_screen_size;
} B3gsDensifyIO;
int b3gs_densify_classify(const B3gsDensifyIO* io, int32_t* flags, b3gs_stream_t stream);
int b3gs_densify_scatter(const B3gsDensifyIO* io, const int32_t* flags, const int32_t* off_keep,
                         const int32_t* off_clone, const int32_t* off_split, int32_t n_keep, int32_t n_clone,
                         int32_t n_split, const float* noise, float* const* out_param, float* const* out_exp_avg,
                         float* const* out_exp_avg_sq, b3gs_stream_t stream);

/* ---- ABI 9: the statements of the training loop ONE BY ONE, behind the reference's own call signatures ------------
 * An unchanged train.py:123-198 calls l1_loss / ssim / SmoothLoss.forward / inverse_warp_images as separate statements
 * with PyTorch glue between them, then gaussians.opacity_decay(), add_densification_stats() and optimizer.step(): each
 * of them is one launch here (value forward; EVERY input gradient backward), wrapped on the python side as
 * autograd.Functions / methods with exactly the reference's signatures (binocular3dgs_amd/loss_utils.py,
 * graphics_utils.py, gaussian_model.py, optim.py).  All tensors fp32, contiguous, on the device.
 *
 * Scalar results are deterministic (per-workgroup partial sums folded in index order by the workgroup that arrives
 * last: no float atomics, no second launch).  `workspace`: b3gs_lossfn_workspace_floats(planes, H, W) floats whose
 * header (the first 2080 words: two levels of arrival counters) is ZERO before the first call; every call leaves it zero.
 * One workspace per stream. */
size_t b3gs_lossfn_workspace_floats(int64_t planes, int32_t H, int32_t W);

/* utils/loss_utils.py:18-21  l1_loss(network_output, gt, mask=None) = mean |x*mask - y*mask|.
 * x, y: [batch, channels, hw]; mask: NULL, or [batch, hw] (broadcast over the channels; a mask of x's own shape is
 * passed as channels = 1, hw = numel / batch).  out: [1].  backward: grad_out = the upstream gradient, a device scalar;
 * grad_x / grad_y / grad_mask may each be NULL (not wanted). */
int b3gs_l1_loss_forward(const float* x, const float* y, const float* mask, int64_t batch, int32_t channels, int64_t hw,
                         float* out, float* workspace, b3gs_stream_t stream);
int b3gs_l1_loss_backward(const float* x, const float* y, const float* mask, int64_t batch, int32_t channels, int64_t hw,
                          const float* grad_out, float* grad_x, float* grad_y, float* grad_mask, b3gs_stream_t stream);

/* utils/graphics_utils.py:80-125  inverse_warp_images(image [B,C,H,W], disparity [B,1,H,W], row_indices, column_indices)
 * -> [B,C,H,W]: linear interpolation between columns c + floor(d) and the next one, zero where either leaves the row.
 * zero_fill (may be NULL): a [B,C,H,W] buffer the forward fills with zeros on its way -- the grad_image of the backward,
 * which ADDS into it (bilinear scatter); grad_image / grad_disparity may each be NULL. */
int b3gs_inverse_warp_forward(const float* image, const float* disparity, int32_t B, int32_t C, int32_t H, int32_t W,
                              float* out, float* zero_fill, b3gs_stream_t stream);
int b3gs_inverse_warp_backward(const float* image, const float* disparity, const float* grad_out, int32_t B, int32_t C,
                               int32_t H, int32_t W, float* grad_image, float* grad_disparity, b3gs_stream_t stream);

/* utils/loss_utils.py:68-91  SmoothLoss.forward(disparity [B,1,H,W], image [B,C,H,W]): edge-aware first-order
 * smoothness on the interior (the reference's fixed 3x3 convolutions have no padding).  out: [1]. */
int b3gs_smooth_loss_forward(const float* disparity, const float* image, int32_t B, int32_t C, int32_t H, int32_t W,
                             float* out, float* workspace, b3gs_stream_t stream);
int b3gs_smooth_loss_backward(const float* disparity, const float* image, int32_t B, int32_t C, int32_t H, int32_t W,
                              const float* grad_out, float* grad_disparity, float* grad_image, b3gs_stream_t stream);

/* utils/loss_utils.py:36-66  ssim(img1, img2, window_size=11, size_average=True): 11x11 Gaussian window (sigma 1.5),
 * zero padding, every [H,W] plane by itself.  out: [1], or [batch] when size_average == 0.  maps (NULL: value only):
 * 5 * batch * channels * H * W floats the backward reads (the last two fifths only written when maps_for_img2 != 0,
 * i.e. when img2 wants a gradient too).  backward: grad_out [1] or [batch]; grad_img1 / grad_img2 may be NULL. */
int b3gs_ssim_forward(const float* img1, const float* img2, int32_t batch, int32_t channels, int32_t H, int32_t W,
                      int32_t size_average, float* maps, int32_t maps_for_img2, float* out, float* workspace,
                      b3gs_stream_t stream);
int b3gs_ssim_backward(const float* img1, const float* img2, const float* maps, int32_t batch, int32_t channels, int32_t H,
                       int32_t W, int32_t size_average, const float* grad_out, float* grad_img1, float* grad_img2,
                       b3gs_stream_t stream);

/* scene/gaussian_model.py:307-309  opacity_decay(factor): o <- inverse_sigmoid(sigmoid(o) * factor), in place. */
int b3gs_opacity_decay(float* opacity, int64_t count, float factor, b3gs_stream_t stream);
/* scene/gaussian_model.py:409-411  add_densification_stats: for the rows update_filter (one byte per row) selects,
 * xyz_gradient_accum += ||viewspace_grad[row, :2]|| and denom += 1.  row_stride: floats per row of viewspace_grad (3). */
int b3gs_add_densification_stats(int64_t P, const float* viewspace_grad, int64_t row_stride, const uint8_t* update_filter,
                                 float* xyz_gradient_accum, float* denom, b3gs_stream_t stream);
/* Data-parallel tail: statistics of a step staged by the chain rule (B3gsDensifyStats pointing at three zeroed [P] arrays)
 * are added to the model's once the ranks agree that nobody overflowed -- `agreed_word` (device, any 32-bit pattern: the
 * float SUM of the ranks' flags that travelled inside the first gradient range's all-reduce) == 0 -- and discarded
 * otherwise, in which case *local_overflow_flag (may be NULL) gets bit 0 set.  The staging arrays are left zero. */
int b3gs_apply_staged_densify_stats(int64_t P, float* staged_accum, float* staged_denom, float* staged_max_radii,
                                    float* xyz_gradient_accum, float* denom, float* max_radii2D, const int32_t* agreed_word,
                                    int32_t* local_overflow_flag, b3gs_stream_t stream);
/* train.py:196-198 optimizer.step() for an optimiser that keeps torch.optim.Adam's state layout: b3gs_adam_step with the
 * step number given by the host (1-based, the value of state["step"] after its increment); no decay, no row mask. */
int b3gs_adam_step_at(int32_t nseg, const B3gsAdamSegment* segs, int32_t step, float beta1, float beta2, float eps,
                      b3gs_stream_t stream);

/* ---- ABI 11: image metrics of held-out views (binocular3dgs_amd/evaluate.py) -----------------------------------------
 * The per-view sums behind train.py:226-261 (training_report: clamp to [0,1], mean L1, mean of per-channel PSNRs) and
 * metrics.py:37-124 over the PNGs of render.py (8-bit round trip, DTU mask composite, masked PSNR, SSIM).  Per view and
 * element: both images are clamped to [0,1] (mode bit B3GS_METRIC_CLAMP) and/or quantised to
 * uint8(clamp(x*255 + 0.5, 0, 255)) / 255 (bit B3GS_METRIC_QUANTIZE, torchvision's save_image + to_tensor), then
 * composited with the mask as x*m + (1 - m) (mask NULL: unchanged), then d = image - gt.
 * out[v, 2C + 2] (fp64): sum |d| per channel, sum d^2 per channel, sum d^2 over the elements with m == 1 exactly (all
 * channels pooled; every element when mask is NULL), the number of those elements.
 * prepared_image / prepared_gt (both NULL or both set): [C,H,W] each, the composited pair -- with one [nviews,C,H,W]
 * tensor per side, b3gs_ssim_forward(batch = nviews, size_average = 0) gives the per-view SSIM of metrics.py.
 * One partial-sum launch per 32 views (all views of an evaluation batch in one) and one fold in fixed order: no float
 * atomics, every sum in fp64, the same bits from call to call.  All images fp32, contiguous, [C,H,W]; 1 <= C <= 4.
 * workspace: b3gs_image_metrics_workspace_bytes(nviews, C, H, W) bytes, no initial content needed. */
#define B3GS_METRIC_CLAMP 1
#define B3GS_METRIC_QUANTIZE 2
typedef struct B3gsMetricView {
  const float* image;     /* [C,H,W] */
  const float* gt;        /* [C,H,W] */
  const float* mask;      /* NULL, [1,H,W] (broadcast over the channels) or [C,H,W]; may be fractional */
  int32_t mask_channels;  /* 1 or C (ignored when mask is NULL) */
  float* prepared_image;  /* NULL or [C,H,W] */
  float* prepared_gt;     /* NULL or [C,H,W] */
} B3gsMetricView;
size_t b3gs_image_metrics_workspace_bytes(int32_t nviews, int32_t C, int32_t H, int32_t W);
int b3gs_image_metrics_batch(int32_t nviews, const B3gsMetricView* views, int32_t C, int32_t H, int32_t W, int32_t mode,
                             double* out, void* workspace, b3gs_stream_t stream);

/* ---- ABI 12: frames of a rendered path (binocular3dgs_amd/frames.py) --------------------------------------------------
 * The three uint8 images spiral.py:101-131 writes per frame, bit for bit, with torchvision's quantiser
 * q(x) = uint8(clamp(x*255 + 0.5, 0, 255)):
 *   rgb_out   [H,W,3]  q(rgb), fp32
 *   gray_out  [H,W,3]  v = 1 - (1 - (depth - min) / (max - min)) * alpha (fp32, that op order, min / max over all H*W
 *                      pixels of the view), q(v) in all three channels
 *   cmap_out  [H,W,3]  visualize_cmap(v, ones, turbo, percentile, curve -log(x + 1e-6)): lo / hi are the weighted
 *                      percentiles 50 -/+ percentile/2 of v (np.interp on the exact order statistics), widened by the fp32
 *                      epsilon; the value is curved in fp32, lo / hi in fp64, normalised in fp64, clipped, NaN -> 0, LUT
 *                      index int(x*256) with 256 -> 255; the pixel is lut[index] (lut: 256 x 3 bytes on the device).
 * Empty view (max == min: the reference divides 0 by 0): gray 0 and cmap lut[0] everywhere, bounds NaN.
 * depth must be finite.  Any of the three outputs may be NULL (skipped); rgb may be NULL when rgb_out is, depth / alpha
 * when gray_out and cmap_out are (and bounds_out is NULL).
 * bounds_out: NULL or device double[nviews * 2]: the percentile bounds lo_auto, hi_auto of every view (before the
 * epsilon and the curve).
 * Exact and deterministic: min / max by comparison, the order statistics by an exact radix select (11/11/10 bits, integer
 * atomics on histograms only).  8 launches per call whatever nviews; the host reads nothing.
 * 1 <= nviews <= 8, 1 <= H*W <= 2^24 (the reference's fp32 cumulative weights are exact integers there).
 * workspace: b3gs_frames_workspace_bytes(nviews, H, W) bytes, no initial content needed. */
#define B3GS_MAX_FRAME_VIEWS 8
typedef struct B3gsFrameView {
  const float* rgb;    /* [3,H,W] */
  const float* depth;  /* [1,H,W] */
  const float* alpha;  /* [1,H,W] */
  uint8_t* rgb_out;    /* NULL or [H,W,3] */
  uint8_t* gray_out;   /* NULL or [H,W,3] */
  uint8_t* cmap_out;   /* NULL or [H,W,3] */
} B3gsFrameView;
size_t b3gs_frames_workspace_bytes(int32_t nviews, int32_t H, int32_t W);
int b3gs_encode_frames_batch(int32_t nviews, const B3gsFrameView* views, int32_t H, int32_t W, double percentile,
                             const uint8_t* lut, void* workspace, double* bounds_out, b3gs_stream_t stream);

/* ---- ABI 13: ground-truth preparation of dataset images (binocular3dgs_amd/ground_truth.py) ----------------------------
 * From the uint8 source image at its own size to the tensors the training loop reads, bit for bit what the reference
 * computes on the host (utils/general_utils.py:22-28 PILtoTorch, utils/camera_utils.py:22-57 loadCam,
 * scene/cameras.py:40-47, train.py:110-120), for up to 8 views of one output W x H per call:
 *   1. PIL.Image.resize((W, H)) with its default filter, 8 bits per channel: per axis whose size changes, a pass
 *      clip8((2^21 + sum_j pixel[first + j] * K[j]) >> 22) with the taps of a host-built table; horizontal pass first, stored
 *      as uint8; RGBA is premultiplied before (c' = ((t >> 8) + t) >> 8, t = c*a + 128) and un-premultiplied after
 *      (a in {0, 255}: c', else min(255, 255*c' / a)); both sizes unchanged: the source as it is.
 *   2. / 255 (the correctly rounded fp32 division).  C = 4: alpha = a / 255; with white_background
 *      image = image * alpha + (1 - alpha) (three roundings, no FMA).  clamp(0, 1).  C = 4: image *= alpha.
 *   3. dtu_threshold > 0: bg_mask[y, x] = AND over rows max(0, y-49)..y of (max over channels of image < dtu_threshold).
 * A table is device int32 [2 + ks][out], row-major: row 0 = first source index of every output index, row 1 = its tap
 * count (<= ks), rows 2.. = the taps with 22 fractional bits (0 beyond the count).  tab_x / tab_y is NULL exactly when
 * Ws == W / Hs == H.  The caller guarantees 255 * sum|K| < 2^31 per output index (int32 accumulators); source indices are
 * clamped on the device, so a wrong table gives wrong pixels, never an access outside the buffers.
 * Outputs (float32, device, 16-byte aligned): image [3,H,W] ([1,H,W] when C = 1), alpha [1,H,W] (C = 4 only, else ignored),
 * bg_mask [1,H,W] (needed when dtu_threshold > 0).  src is 16-byte aligned.
 * At most 3 launches per call (horizontal pass only when a view needs it, mask only when asked); the host reads nothing.
 * workspace: b3gs_gt_workspace_bytes(nviews, views, H, W) bytes (the horizontal passes' intermediates), 256-byte aligned,
 * no initial content needed. */
#define B3GS_MAX_GT_VIEWS 8
typedef struct B3gsGtView {
  const uint8_t* src;    /* [Hs, Ws, C] */
  int32_t Hs, Ws, C;     /* C in {1, 3, 4} */
  const int32_t* tab_x;  /* [2 + ks_x][W] or NULL */
  const int32_t* tab_y;  /* [2 + ks_y][H] or NULL */
  int32_t ks_x, ks_y;
  float* image;
  float* alpha;
  float* bg_mask;
} B3gsGtView;
size_t b3gs_gt_workspace_bytes(int32_t nviews, const B3gsGtView* views, int32_t H, int32_t W);
int b3gs_prepare_gt_batch(int32_t nviews, const B3gsGtView* views, int32_t H, int32_t W, int32_t white_background,
                          float dtu_threshold, void* workspace, b3gs_stream_t stream);

/* ---- the matcher cloud (ABI 14; binocular3dgs_amd/matcher_cloud.py) ---------------------------
 * What the reference's submodules/dense_matcher/triangulate.py does once the matcher has produced its keypoints: DLT
 * triangulation with the reprojection and frame filters and the colour lookup (lines 165-219), the DTU background sheet
 * (221-238) and one round of the photo-consistency growth loop (264-379).  All pointers are device pointers unless said
 * otherwise; nothing reads the device.  workspace: b3gs_cloud_workspace_bytes(n) bytes, 256-byte aligned, n = matches /
 * pixels / candidates of the call.
 *
 * b3gs_triangulate_matches: one view pair.  proj_ref / proj_src [3,4], intrinsic [3,3], w2c_ref / w2c_src [4,4], kp [N,2],
 * image uint8 [H,W,3]; points [N,3] and colors [N,3] receive the kept matches densely in input order, *count their number.
 * b3gs_background_sheet: inv_intrinsic_t = inverse(intrinsic^T) [3,3], c2w [4,4]; for every pixel whose largest channel is
 * >= 254 the world point of `depth` (pixel order), colour 255; outputs sized H*W.
 * b3gs_cloud_grow_round: see B3gsCloudGrow.  At most two launches (three when `init` counts the starting cloud first). */
size_t b3gs_cloud_workspace_bytes(int64_t n);
int b3gs_triangulate_matches(int32_t N, const float* proj_ref, const float* proj_src, const float* intrinsic,
                             const float* w2c_ref, const float* w2c_src, const float* kp_ref, const float* kp_src,
                             const uint8_t* image, int32_t W, int32_t H, float reproj_threshold, float* points,
                             uint8_t* colors, int32_t* count, void* workspace, b3gs_stream_t stream);
int b3gs_background_sheet(const uint8_t* image, int32_t W, int32_t H, const float* inv_intrinsic_t, const float* c2w,
                          float depth, float* points, uint8_t* colors, int32_t* count, void* workspace,
                          b3gs_stream_t stream);
#define B3GS_CLOUD_MAX_VIEWS 16
typedef struct B3gsCloudGrow {
  int32_t W, H, n_views;          /* the selected views, 2..16 of them */
  int32_t ref, src;               /* this round's two views (slots into the arrays below), ref != src */
  int32_t n_seeds, n_samples;     /* candidates = n_seeds * n_samples, candidate (i, j) = points[seed_idx[i]] + noise[i,j] * alpha */
  int32_t n_start;                /* length of the cloud before growth: seed indices lie below it */
  int32_t h_patch_size;           /* 5 (an 11x11 window); anything else is refused */
  int32_t init;                   /* non-zero: zero the grids and count points[0, n_start) into them first */
  float fx, fy, cx, cy, alpha, ssim_threshold;
  const uint8_t* images;          /* [n_views, H, W, 3] */
  const float* w2c;               /* [n_views, 4, 4] */
  const float* window;            /* [121] */
  const int32_t* seed_idx;        /* [n_seeds] */
  const float* noise;             /* [n_seeds, n_samples, 3] */
  float* points;                  /* [capacity, 3] */
  float* colors;                  /* [capacity, 3], 0..255 as float32 */
  int32_t capacity;
  int32_t* length;                /* device word: points in the cloud; keeps counting past `capacity` (nothing is written there) */
  int32_t* overflow;              /* device word: set when a point did not fit, or when a grid margin was violated (bit 1) */
  int32_t* grids;                 /* [n_views, H + 2, W + 2] points of the cloud per rounded pixel, one cell of margin */
  void* workspace;
  float* debug_ssim;              /* [candidates] or NULL: mean SSIM of every live candidate (0 for the others) */
  uint8_t* debug_mask;            /* [candidates] or NULL: patch_mask */
} B3gsCloudGrow;
int b3gs_cloud_grow_round(const B3gsCloudGrow* io, b3gs_stream_t stream);

/* ---- the plane-sweep stereo matcher (ABI 15; binocular3dgs_amd/sweep_matcher.py) ---------------
 * Keypoint matches of one calibrated view pair {a, b}, both directions in one call, without a network: per node of the
 * reference view (pixels 3 + i stride, row-major) the best of D fronto-parallel inverse-depth hypotheses by the ZNCC of the
 * 7x7 gray patches, a uniqueness test, a parabola refinement, a left/right check against the other direction's node map and
 * an ordered compaction.  Five launches; nothing reads the device, nothing synchronises.  Direction 0 is a -> b, 1 is b -> a.
 * nodes = ((W - 7) / stride + 1) * ((H - 7) / stride + 1); every output holds `nodes` rows per direction, so nothing overflows.
 * workspace: b3gs_sweep_workspace_bytes(W, H, D, stride) bytes (0: bad sizes), 256-byte aligned. */
typedef struct B3gsSweepPair {
  int32_t W, H, D, stride;
  int32_t radius;                 /* 3 (a 7x7 patch); anything else is refused */
  float near, far;                /* 0 < near < far: the depth range the hypotheses span */
  float inv_far, step;            /* invd[k] = inv_far + step * k, as float32 of the float64 values */
  float min_score, margin, min_var, cyc_steps;
  const uint8_t* image_a;         /* [H, W, 3] */
  const uint8_t* image_b;
  const float* homographies;      /* [2, D, 3, 3]: pixel of the direction's reference view -> pixel of the other view, plane k */
  const float* proj;              /* [2, 12]: K R K^-1 (9, row-major) and K t (3) of the direction: q ~ M p + (K t) invd */
  float* kp_source;               /* [2, nodes, 2] the kept nodes (x, y), in node order */
  float* kp_target;               /* [2, nodes, 2] their correspondences in the other view */
  float* score;                   /* [2, nodes]    their ZNCC */
  int32_t* count;                 /* [2] device words: kept matches per direction */
  float* node_invd;               /* [2, nodes] the node map: refined inverse depth, -1 = none */
  float* node_score;              /* [2, nodes] best valid score (0: no valid hypothesis) */
  int32_t* node_k;                /* [2, nodes] best valid hypothesis (-1: none) */
  void* workspace;
} B3gsSweepPair;
size_t b3gs_sweep_workspace_bytes(int32_t W, int32_t H, int32_t D, int32_t stride);
int b3gs_sweep_match_pair(const B3gsSweepPair* io, b3gs_stream_t stream);

/* ---- baseline JPEG of rendered frames (ABI 16; binocular3dgs_amd/frames.py) ---------------------
 * The entropy-coded scan of a baseline sequential JPEG of up to B3GS_MAX_FRAME_VIEWS uint8 [H,W,3] images of one W x H (what
 * the frame encoder of ABI 12 writes): YCbCr 4:2:0, 8 bit, one interleaved scan (Y00 Y01 Y10 Y11 Cb Cr per 16 x 16 MCU, MCUs
 * row by row), the Annex K "typical" Huffman tables, no restart markers, 0xFF stuffed with 0x00, the last byte filled with
 * 1-bits.  Header (SOI .. SOS) and EOI are the same for every frame of a (W, H, tables): the caller puts them around the scan.
 * Integer arithmetic throughout (tests/jpeg_ref.py restates it; the bytes agree):
 *   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16,
 *   Cr = (32768 R - 27439 G - 5329 B + 8421375) >> 16; edges replicated to whole MCUs; chroma = (sum of 2 x 2 + bias) >> 2 with
 *   bias 1, 2, 1, 2, .. along a row; the 13-bit Loeffler-Ligtenberg-Moschytz DCT of sample - 128 (rows, then columns, scaled
 *   by 8); coefficient = sign(c) * ((|c| + 4 q) / (8 q)).
 * images: HOST array of nviews device pointers.  qtables: device uint16[128], the luminance then the chrominance table,
 * row-major, entries 1..255.  Frame i goes to out + i * capacity and its byte count to lengths[i] (device); a frame whose scan
 * is longer than `capacity` is not written at all (no byte of `out` changes for it) and reports -1: the bound is about 10
 * bytes per pixel.  Six launches whatever nviews; nothing reads the device, nothing synchronises; capturable in a graph.
 * 1 <= nviews <= 8, 1 <= W, H <= 65535, capacity >= 1.
 * workspace: b3gs_jpeg_workspace_bytes(nviews, H, W) bytes (0: bad sizes), 256-byte aligned, no initial content needed. */
size_t b3gs_jpeg_workspace_bytes(int32_t nviews, int32_t H, int32_t W);
int b3gs_jpeg_encode_batch(int32_t nviews, const uint8_t* const* images, int32_t H, int32_t W, const uint16_t* qtables,
                           uint8_t* out, int64_t capacity, int64_t* lengths, void* workspace, b3gs_stream_t stream);

/* ---- a triangle mesh of a trained scene (ABI 17; binocular3dgs_amd/mesh.py) ---------------------
 * TSDF fusion of rendered depth into a voxel volume, and marching tetrahedra over it.  tests/mesh_ref.py restates every
 * statement in numpy float32; the volume, the vertices and the faces agree bit for bit.
 *
 * The volume: nx x ny x nz voxels, x fastest; the centre of voxel (i, j, k) is origin + (i + 0.5, j + 0.5, k + 0.5) * voxel.
 * Per voxel tsdf (float32, in units of the truncation, <= 1), weight (float32, the number of views that reached it) and
 * rgb (3 x float32, interleaved).  1 <= nx, ny, nz <= B3GS_MAX_TSDF_DIM.
 *
 * b3gs_tsdf_integrate_batch: 1..B3GS_MAX_TSDF_VIEWS views of one W x H (W * H <= 2^30).  One thread owns one voxel and walks
 * the views in index order (no atomics: the result does not depend on scheduling).  Per view, one correctly rounded float32
 * operation per statement:
 *   c = (rot[3r] * px + rot[3r + 1] * py) + rot[3r + 2] * pz + trans[r]        the centre in the camera (r = 0, 1, 2)
 *   skipped unless c.z > near
 *   u = fx * (c.x / c.z) + (0.5 W - 0.5), v likewise with fy and H             the project's pixel of a point (preprocess.hip:
 *   pixel = (rint(u), rint(v)), skipped outside the image                      ((ndc + 1) S - 1) / 2: centres at integers)
 *   skipped unless alpha[pixel] >= alpha_min;  d = depth[pixel] / alpha[pixel]
 *       (the renderer's depth is the alpha-weighted sum of the camera-space z of the Gaussians blended into the pixel --
 *        render.hip accumulates record.depth * alpha * T, and preprocess.hip stores the view-space z there -- so depth / alpha
 *        is their mean z: the same axis as c.z, no ray-length conversion)
 *   sdf = d - c.z, skipped unless sdf >= -truncation;  val = min(1, sdf / truncation)
 *   tsdf = (tsdf * w + val) / (w + 1), the three colour channels likewise, then w = w + 1
 * truncation > 0, near >= 0, alpha_min > 0, voxel > 0.
 *
 * b3gs_mesh_count / b3gs_mesh_emit: marching tetrahedra.  Every cell (the cube between 8 voxel centres) is cut into the six
 * tetrahedra around its diagonal (0,0,0)-(1,1,1): for the axis permutation (a, b, c), in lexicographic order, the corners
 * 0, e_a, e_a + e_b, (1,1,1).  A cell is valid when its 8 corners have weight >= min_weight; a corner is inside when
 * tsdf < 0 (exactly 0 is outside; zero-area triangles that follow are kept).  A vertex lives on one of the 7 edges its
 * lower-index end owns -- slots x, y, z, xy, xz, yz, xyz -- and exists exactly when the edge changes sign and lies in a valid
 * cell.  Vertex ids are the exclusive scan of the existing slots in (voxel linear index, slot) order, triangles come in (cell
 * linear index, tetrahedron, table) order: one fixed output whatever the launch geometry.  position = p0 + t (p1 - p0),
 * t = d0 / (d0 - d1), p0 the lower-index end; colour = uint8(rint(min(max((c0 + t (c1 - c0)) * 255, 0), 255))).  Triangles
 * are wound so that the normal points to the positive (free-space) side.
 * count writes the per-voxel slot masks and per-cell triangle counts, their block sums and, at the START of the workspace,
 * two int64 totals {vertices, triangles}: the only words the host reads.  emit(nverts, ntris) then fills vertices
 * [nverts, 3], colours [nverts, 3] and faces [ntris, 3]; totals beyond INT32_MAX are B3GS_ERR_ARG, and no write goes past the
 * counts it was given.  Nothing synchronises; both are capturable in a graph.
 * workspace: b3gs_mesh_workspace_bytes(nx, ny, nz) bytes (0: bad sizes; 6 bytes per voxel), 256-byte aligned. */
#define B3GS_MAX_TSDF_VIEWS 8
#define B3GS_MAX_TSDF_DIM 1024
typedef struct B3gsTsdfVolume {
  int32_t nx, ny, nz;
  float origin[3];
  float voxel;
  float* tsdf;                    /* [nz, ny, nx] */
  float* weight;                  /* [nz, ny, nx] */
  float* rgb;                     /* [nz, ny, nx, 3] */
} B3gsTsdfVolume;
typedef struct B3gsTsdfView {
  const float* depth;             /* [H, W] the renderer's depth */
  const float* alpha;             /* [H, W] */
  const float* colour;            /* [3, H, W] */
  float rot[9];                   /* world -> camera rotation, row-major */
  float trans[3];                 /* world -> camera translation */
  float fx, fy;                   /* focal lengths in pixels */
} B3gsTsdfView;
int b3gs_tsdf_integrate_batch(const B3gsTsdfVolume* volume, int32_t nviews, const B3gsTsdfView* views, int32_t W, int32_t H,
                              float truncation, float near, float alpha_min, b3gs_stream_t stream);
size_t b3gs_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int b3gs_mesh_count(const B3gsTsdfVolume* volume, float min_weight, void* workspace, b3gs_stream_t stream);
int b3gs_mesh_emit(const B3gsTsdfVolume* volume, void* workspace, int64_t nverts, int64_t ntris, float* vertices,
                   uint8_t* colours, int32_t* faces, b3gs_stream_t stream);

/* ---- cleaning and scoring an extracted mesh (ABI 18; binocular3dgs_amd/mesh_tools.py) -----------
 * Integer work, minima over sets and single correctly rounded float32 operations: tests/meshtools_ref.py restates every
 * statement in numpy, and everything below except the fp64 means agrees bit for bit.  Nothing synchronises or reads the
 * device; every call is capturable in a graph.  Every workspace is 256-byte aligned; a size function returns 0 for bad sizes.
 *
 * b3gs_mesh_components: faces int32 [F, 3] over vertices 0 .. V-1.  Two vertices are connected when one triangle names
 * both (a repeated index is legal).  labels[v] = the smallest vertex index of v's component; tri_count[r] = the triangles of
 * the component whose label is r, 0 at every index that is not a label; a vertex no triangle names is its own component
 * with 0 triangles.  A triangle with an index outside 0 .. V-1 connects nothing and is counted nowhere.  Lock-free
 * union-find, one thread per triangle edge; four launches, no thread waits for another.
 *
 * b3gs_mesh_clean_count / _emit: a component survives when tri_count >= max(*threshold, 1) (threshold: ONE int32 on the
 * device).  A vertex is kept when its component survives (so it has a triangle), a triangle when its component survives.
 * New vertex ids are the exclusive scan of the kept flags; kept vertices, colours and triangles keep their order and winding.
 * count leaves three int64 at the START of the workspace: {vertices kept, triangles kept, triangles with an index outside
 * 0 .. V-1}; emit(nverts, ntris) fills out_vertices [nverts, 3], out_colours [nverts, 3], out_faces [ntris, 3] and writes
 * nothing past those counts.  emit takes the arguments of count again and the same workspace.
 *
 * b3gs_mesh_sample_count / _emit: points = the V vertices in order, then per triangle (p0, p1, p2), in triangle order:
 *   e1 = p1 - p0, e2 = p2 - p0                                              per component
 *   |e| = sqrt((e.x e.x + e.y e.y) + e.z e.z)
 *   n1 = floor(|e1| / spacing), n2 = floor(|e2| / spacing)                  both < 2^15, else the triangle is counted as an error
 *   for i = 0 .. n1, for j = 0 .. n2, without (0, 0), where i (n2+1) + j (n1+1) < (n1+1)(n2+1)   (integers)
 *     point = (p0 + (i / (n1+1)) e1) + (j / (n2+1)) e2                      i / (n1+1) and j / (n2+1) are float32 divisions
 * count leaves three int64 at the start of the workspace: {lattice points (without the V vertices), triangles past the 2^15
 * limit, triangles with an index outside 0 .. V-1}; emit(npoints) writes points [V + npoints, 3].  spacing > 0;
 * V + npoints <= 2^31 - 1.
 *
 * b3gs_nearest_grid / _query: out[i] = min(max_dist, sqrt(min_j d2(a_i, b_j))), d = a - b per component,
 * d2 = (d.x d.x + d.y d.y) + d.z d.z, all float32: the float32 brute force, bit for bit.  grid sorts b (Nb >= 1 points)
 * into a uniform grid whose origin, edge and dimensions are computed on the device and left at the start of the workspace as
 * {float origin[3], float edge, int32 dim[3], int32 shells}; the edge is the largest of cbrt(box volume / (8 Nb)) (square
 * root / quotient when the box is flat along one / two axes), max_dist / 16 and extent / 1000, widened until the grid has at
 * most 1024 cells per axis and min(max(8 Nb, 4096), 2^24) cells.  query walks shells of cells outward from the query's cell
 * and stops at the first shell that provably holds nothing nearer than the best so far or max_dist (csrc/meshtools.hip states
 * the bound); at most `shells` <= 17 shells.  max_dist > 0 and finite; the coordinates are finite.
 *
 * b3gs_nearest_query_index (added for binocular3dgs_amd/edit.py: register): the same walk over the same workspace; besides
 * out it writes index [Na] int32, the index into b of the nearest point, among equal float32 d2 the smallest index, and -1
 * when sqrt(min_j d2) > max_dist (nothing lies within max_dist; out is max_dist there).
 *
 * b3gs_cloud_score: out[0] = the fp64 sum of dist[i] over the points with mask[i] != 0 (mask NULL: all), out[1] = their
 * number, out[2] = the number of them with dist[i] < tau.  Per-workgroup fp64 partials, folded in index order by one wave:
 * the same bits on every call. */
int b3gs_mesh_components(int32_t V, int64_t F, const int32_t* faces, int32_t* labels, int32_t* tri_count, b3gs_stream_t stream);
size_t b3gs_mesh_clean_workspace_bytes(int64_t V, int64_t F);
int b3gs_mesh_clean_count(int32_t V, int64_t F, const int32_t* faces, const int32_t* labels, const int32_t* tri_count,
                          const int32_t* threshold, void* workspace, b3gs_stream_t stream);
int b3gs_mesh_clean_emit(int32_t V, int64_t F, const float* vertices, const uint8_t* colours, const int32_t* faces,
                         const int32_t* labels, const int32_t* tri_count, const int32_t* threshold, void* workspace,
                         int64_t nverts, int64_t ntris, float* out_vertices, uint8_t* out_colours, int32_t* out_faces,
                         b3gs_stream_t stream);
size_t b3gs_mesh_sample_workspace_bytes(int64_t F);
int b3gs_mesh_sample_count(int32_t V, int64_t F, const float* vertices, const int32_t* faces, float spacing, void* workspace,
                           b3gs_stream_t stream);
int b3gs_mesh_sample_emit(int32_t V, int64_t F, const float* vertices, const int32_t* faces, float spacing, void* workspace,
                          int64_t npoints, float* points, b3gs_stream_t stream);
size_t b3gs_nearest_workspace_bytes(int64_t Nb);
int b3gs_nearest_grid(int64_t Nb, const float* b, float max_dist, void* workspace, b3gs_stream_t stream);
int b3gs_nearest_query(int64_t Na, const float* a, int64_t Nb, float max_dist, const void* workspace, float* out,
                       b3gs_stream_t stream);
int b3gs_nearest_query_index(int64_t Na, const float* a, int64_t Nb, float max_dist, const void* workspace, float* out,
                             int32_t* index, b3gs_stream_t stream);
size_t b3gs_cloud_score_workspace_bytes(int64_t N);
int b3gs_cloud_score(int64_t N, const float* dist, const uint8_t* mask, float tau, double* out, void* workspace,
                     b3gs_stream_t stream);

/* ---- simplifying an extracted mesh: quadric vertex clustering (ABI 18, added entry points; binocular3dgs_amd/mesh_tools.py, INTEGRATION.md
 * section 14) ------------------------------------------------------------------------------------------------------------------
 * Three entry points ADDED to ABI 18: no existing declaration, struct or meaning changes, so the number stays (a binding of
 * ABI 18 keeps working against this library, and tests/test_meshtools_cpu.py pins it).
 * A Rossignac-Borrel grid with Lindstrom's quadric-optimal representatives.  Integer work, stable sorts, ordered scans, single
 * correctly rounded float32 operations, and fp64 statements that ONE thread per cluster executes in one fixed order:
 * tests/simplify_ref.py restates every statement in numpy and every output agrees bit for bit.  Nothing synchronises or reads
 * the device; the workspace is 256-byte aligned, b3gs_mesh_simplify_workspace_bytes(V, F) bytes (0 for bad sizes; about
 * 80 bytes per triangle and 50 per vertex).  V <= 2^31 - 1, 3 F <= 2^31 - 1, cell > 0 and finite.
 *
 * 1. grid      o = the per-axis float32 minimum of the V vertices (computed on the device)
 *              c_a = floor((x_a - o_a) / cell)            two rounded float32 operations, then the floor, per axis
 *              key = (c_z << 20) | (c_y << 10) | c_x       a c_a outside 0 .. 1023 (or NaN) is counted as an error, not clamped
 * 2. clusters  the vertices are sorted stably by key; the cluster id of a vertex is the rank of its key among the distinct
 *              keys, ascending; the members of a cluster are in vertex-index order
 * 3. faces     (a, b, c) = the cluster ids of the corners; two equal ids: the face is degenerate and dropped.  Among the
 *              faces with the same unordered {a, b, c} the one with the smallest face index survives, whatever the winding of
 *              the others (a stable sort by max, then by mid, then by min, the three orders composed, and a boundary pass).
 *              Survivors come out in input face order with the input's corner order.
 * 4. vertices  a cluster survives when a surviving face names it; new ids are the ranks among the survivors, in cluster
 *              order.  A mesh that collapses completely gives nverts = ntris = 0 and no error.
 * 5. colour    per channel (2 sum + n) / (2 n) in integers over the n members
 * 6. mean      m = (the fp64 sum of the member positions, in member order) / n, per axis;  position = float32(m)
 * 7. quadric   ONE THREAD PER CLUSTER k walks, in face-index order, the input faces with at least one corner in k (a face
 *              once, even with two or three corners in k; the faces step 3 drops included): the (cluster, face) incidence
 *              list is built on the device and sorted stably by cluster.  In fp64 from the float32 coordinates, m kept in fp64,
 *              one operation per statement:
 *                u = p1 - p0, v = p2 - p0;  n = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x);  q = p0 - m
 *                d = (n_x q_x + n_y q_y) + n_z q_z
 *                A00 += n_x n_x, A01 += n_x n_y, A02 += n_x n_z, A11 += n_y n_y, A12 += n_y n_z, A22 += n_z n_z
 *                r0 += d n_x, r1 += d n_y, r2 += d n_z
 *              lambda = 1e-3 ((A00 + A11) + A22);  lambda == 0: y = 0.  Otherwise (A + lambda I) y = r by Cholesky:
 *                a00 = A00 + lambda, a11 = A11 + lambda, a22 = A22 + lambda
 *                l00 = sqrt(a00), l10 = A01 / l00, l20 = A02 / l00
 *                l11 = sqrt(a11 - l10 l10), l21 = (A12 - l20 l10) / l11, l22 = sqrt((a22 - l20 l20) - l21 l21)
 *                z0 = r0 / l00, z1 = (r1 - l10 z0) / l11, z2 = ((r2 - l20 z0) - l21 z1) / l22
 *                y2 = z2 / l22, y1 = (z1 - l21 y2) / l11, y0 = ((z0 - l10 y1) - l20 y2) / l00
 *              max |y_a| > cell, or a y_a that is not finite: y = 0.  position = float32(m + y), per axis.
 * 8. the translation unit is compiled with -ffp-contract=off; no floating-point atomic anywhere.
 *
 * count leaves nine int64 at the START of the workspace: {vertices out, triangles out, triangles with an index outside
 * 0 .. V-1, vertices with a coordinate that is not finite, vertices outside the 1024 cells of an axis, clusters, degenerate
 * triangles, duplicate triangles, the float32 bits of the largest box edge}.  A caller reads them once, treats words 2 .. 4 as
 * errors, and calls emit(nverts, ntris) with the arguments of count and the same workspace; emit fills out_vertices
 * [nverts, 3], out_colours [nverts, 3], out_faces [ntris, 3], writes nothing past those counts (which are at most V and F,
 * so they fit int32) and may be called again, e.g. once per placement. */
#define B3GS_SIMPLIFY_QUADRIC 0
#define B3GS_SIMPLIFY_MEAN 1
size_t b3gs_mesh_simplify_workspace_bytes(int64_t V, int64_t F);
int b3gs_mesh_simplify_count(int32_t V, int64_t F, const float* vertices, const int32_t* faces, float cell, void* workspace,
                             b3gs_stream_t stream);
int b3gs_mesh_simplify_emit(int32_t V, int64_t F, const float* vertices, const uint8_t* colours, const int32_t* faces, float cell,
                            int32_t placement, void* workspace, int64_t nverts, int64_t ntris, float* out_vertices,
                            uint8_t* out_colours, int32_t* out_faces, b3gs_stream_t stream);

/* ---- rendering an extracted mesh: a triangle rasterizer (ABI 18, added entry points; binocular3dgs_amd/mesh_render.py, INTEGRATION.md
 * section 15) ------------------------------------------------------------------------------------------------------------------
 * Three entry points ADDED to ABI 18: no existing declaration, struct or meaning changes, so the number stays.
 * Up to B3GS_MAX_MESH_VIEWS views of one W x H of one mesh (vertices float32 [V, 3], colours uint8 [V, 3], faces int32 [F, 3]):
 * per pixel the nearest triangle and its depth.  Membership is 64-bit integer work, every float statement is one correctly
 * rounded operation (the translation unit is compiled with -ffp-contract=off), the visibility buffer is a minimum over a set:
 * tests/meshraster_ref.py restates every statement in numpy and every output agrees bit for bit, whatever the launch geometry
 * and whichever path took a triangle.  Nothing synchronises or reads the device; both calls are capturable in a graph.
 * cameras: HOST float32 [nviews, 14] rows of (world -> camera rotation, 9 row-major; translation, 3; fx, fy in pixels), read
 * during the call.  1 <= nviews <= 8, 1 <= W, H <= B3GS_MAX_MESH_IMAGE, V and F <= 2^31 - 1.
 *
 * 1. vertex    p_r = ((rot[3r] x + rot[3r+1] y) + rot[3r+2] z) + trans[r], r = 0, 1, 2          camera space, float32
 *              sx = fx * (p_0 / p_2) + (0.5 W - 0.5),  sy = fy * (p_1 / p_2) + (0.5 H - 0.5)      pixel centres at integers
 *              X = (int) rint(sx * 256), Y likewise (half to even): 8 sub-pixel bits
 * 2. rejected  a vertex is good when p_2 > 0.2 (the renderer's near plane), p_2 is finite and |rint(sx * 256)|,
 *              |rint(sy * 256)| < 2^22 (a NaN anywhere fails one of these).  A triangle with a vertex that is not good, or
 *              with an index outside 0 .. V-1, is rejected: not clipped, not drawn, counted.  counts (device int32 [9], zeroed
 *              by the call): [v] = triangles rejected in view v, [8] = triangles with an index outside 0 .. V-1 (once, not per
 *              view; they are part of every [v] too).
 * 3. coverage  A = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0), the doubled area (int64); A = 0 covers nothing; A > 0 is
 *              clockwise as seen (y points down): the normal (p1 - p0) x (p2 - p0) points away, and cull_backface drops it.
 *              With s = sign(A): for k = 0, 1, 2, p = k + 1, q = k + 2 (mod 3), (dx, dy) = s (X_q - X_p, Y_q - Y_p),
 *                E_k(i, j) = dx (256 j - Y_p) - dy (256 i - X_p)                                   int64, below 2^48
 *              Pixel (i, j) is covered when, for every k, E_k > 0, or E_k = 0 and the edge is a top or a left one:
 *              dy < 0, or dy = 0 and dx > 0.  Two triangles that share an edge walk it in opposite directions, so a pixel
 *              centre on it belongs to exactly one of them.  Both windings cover.
 * 4. depth     b_k = (float)((double)E_k / (double)(s A)),  w_k = b_k * (1 / p_2 of vertex k),
 *              iz = (w_0 + w_1) + w_2,  z = 1 / iz: the perspective-correct camera-space z (the `d` of section 12)
 * 5. buffer    one uint64 per pixel and view, all ones = empty; a covered pixel takes the minimum of
 *              (float bits of z << 32) | triangle index: the nearest z, among equal z the smallest index.  Integer atomics.
 * 6. paths     the clamped box of a triangle is i = max(ceil(min X / 256), 0) .. min(floor(max X / 256), W - 1), j likewise;
 *              box = its pixel count.  box <= small_box: the lane that set the triangle up walks it; box <= wave_box: one
 *              wave, in 8 x 8 pixel blocks from the box's corner, a block skipped when some E_k is below its bound at the block
 *              corner where it is largest; beyond: one workgroup of 16 waves.  The two lists are compacted in triangle order by
 *              the ordered scan.  small_box, wave_box < 0: the defaults B3GS_MESH_SMALL_BOX, B3GS_MESH_WAVE_BOX; any values
 *              give the same output (0, 2^31 - 1: everything through one wave each; 0, 0: one workgroup each).
 * 7. resolve   a second call with the same cameras, mesh and workspace; thread = pixel.  The winner's E_k, b_k, w_k and z
 *              again from the same integers.  triangle_id int32 [n, H, W] (-1: empty), depth float32 [n, 1, H, W] = z (0),
 *              alpha float32 [n, 1, H, W] = 1 (0), colour float32 [n, 3, H, W] (bg, device float32 [3]; NULL: 0):
 *                B3GS_MESH_SHADE_COLOUR  (((w_0 c_0 + w_1 c_1) + w_2 c_2) * z) / 255 per channel, c the uint8 vertex colours
 *                B3GS_MESH_SHADE_NORMAL  u = p1 - p0, v = p2 - p0 (camera space, statement 1 again),
 *                                        n = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x),
 *                                        l = sqrt((n_x n_x + n_y n_y) + n_z n_z) (correctly rounded), n / l per component (0
 *                                        when l is 0 or not finite), negated when A > 0, then (n + 1) * 0.5
 *              face_pixels int32 [F]: + 1 per pixel the triangle wins (an integer atomic; it accumulates until the caller
 *              zeroes it).  Every output pointer may be NULL.
 * workspace: b3gs_mesh_raster_workspace_bytes(nviews, V, F, W, H) bytes (0: bad sizes; 16 bytes per view and vertex, 8 per view
 * and pixel, 9 per view and triangle), 256-byte aligned, no initial content needed. */
#define B3GS_MAX_MESH_VIEWS 8
#define B3GS_MAX_MESH_IMAGE 16384
#define B3GS_MESH_SMALL_BOX 32
#define B3GS_MESH_WAVE_BOX 4096
#define B3GS_MESH_SHADE_COLOUR 0
#define B3GS_MESH_SHADE_NORMAL 1
size_t b3gs_mesh_raster_workspace_bytes(int32_t nviews, int64_t V, int64_t F, int32_t W, int32_t H);
int b3gs_mesh_raster_batch(int32_t nviews, const float* cameras, int32_t W, int32_t H, int32_t V, int64_t F, const float* vertices,
                           const int32_t* faces, int32_t cull_backface, int32_t small_box, int32_t wave_box, void* workspace,
                           int32_t* counts, b3gs_stream_t stream);
int b3gs_mesh_resolve_batch(int32_t nviews, const float* cameras, int32_t W, int32_t H, int32_t V, int64_t F, const float* vertices,
                            const uint8_t* colours, const int32_t* faces, const void* workspace, const float* bg, int32_t shading,
                            int32_t* triangle_id, float* depth, float* alpha, float* colour, int32_t* face_pixels,
                            b3gs_stream_t stream);

/* ---- texturing an extracted mesh: atlas bake and textured resolve (ABI 18, added entry points; binocular3dgs_amd/mesh_texture.py,
 * INTEGRATION.md section 16) -------------------------------------------------------------------------------------------------
 * Four entry points ADDED to ABI 18: no existing declaration, struct or meaning changes, so the number stays.
 * Every triangle owns a patch of one atlas, texture uint8 [Ht, Wt, 3]; a texel is a point of its triangle's plane, coloured
 * from up to B3GS_MAX_MESH_VIEWS pictures per call.  Integer layout, single correctly rounded float32 operations (the
 * translation unit is compiled with -ffp-contract=off), no float atomic and no sum across threads: tests/texture_ref.py restates
 * every statement in numpy and every output agrees bit for bit, whatever the launch geometry.  Nothing synchronises or reads
 * the device; the three calls are capturable in a graph.  cameras, W, H, V, F, vertices, faces: as for b3gs_mesh_raster_batch;
 * F >= 1.
 *
 * 1. atlas     cell parameter n, 4 <= n <= 256; a cell is (n + 1) x n texels, local indices i = 0 .. n, j = 0 .. n - 1.
 *              cpr = Wt / (n + 1) cells per row (integer division, >= 1); cell c = f / 2 of triangle f sits at column c % cpr,
 *              row c / cpr: its texel (i, j) is texel (x0 + i, y0 + j) of the atlas, x0 = (c % cpr)(n + 1), y0 = (c / cpr) n.
 *              Ht = n ceil(ceil(F / 2) / cpr) = b3gs_mesh_texture_atlas_height(F, n, Wt) (0: no such atlas); Wt, Ht <= 16384.
 *              The even triangle 2c owns the texels with i + j <= n - 1, the odd one 2c + 1 those with i + j >= n: n (n + 1) / 2
 *              each, every texel of the cell once.  The odd half is the even half under i -> n - i, j -> n - 1 - j; (i, j)
 *              below are the indices in the EVEN frame.  A texel in no cell (x >= cpr (n + 1)) or of a triangle >= F is unowned.
 *              In texel-centre coordinates (the centre of atlas texel (x, y) is (x, y)) the corners of vertices 0, 1, 2 are
 *              (x0, y0), (x0 + n - 2, y0), (x0, y0 + n - 2) for the even triangle, and for the odd one
 *              (x0 + n, y0 + n - 1), (x0 + 2, y0 + n - 1), (x0 + n, y0 + 1).
 *              Why the legs are n - 2: a bilinear fetch at (u, v) reads texels floor(u), floor(u) + 1 by floor(v), floor(v) + 1,
 *              the upper ones with weight 0 when u (v) is whole.  In the even frame u, v >= 0 and u + v <= n - 2.  With both
 *              fractions positive, floor(u) + floor(v) < u + v <= n - 2 is a whole number, so <= n - 3, and the largest index sum
 *              read is n - 1.  With one fraction positive, say u's, floor(u) + v < n - 2, so <= n - 3, and the texels read have
 *              sums <= n - 2.  With none, one texel of sum <= n - 2.  Every texel with a weight is owned; legs of n - 1 would
 *              reach sum n, the other triangle's.  The odd half is the point reflection, which maps such footprints onto each other.
 *              The owned texels outside the UV triangle (the gutter) are baked like the others, so there is no dilation pass.
 * 2. texel     b_1 = i / (n - 2), b_2 = j / (n - 2), b_0 = (1 - b_1) - b_2            (negative in the gutter: extrapolation)
 *              q = (b_0 v0 + b_1 v1) + b_2 v2 per axis, the point of the triangle's plane
 *              e1 = v1 - v0, e2 = v2 - v0, m = (e1_y e2_z - e1_z e2_y, e1_z e2_x - e1_x e2_z, e1_x e2_y - e1_y e2_x),
 *              l = sqrt((m_x m_x + m_y m_y) + m_z m_z) (correctly rounded); l = 0 or not finite: the texel takes no view;
 *              N = m / l per component
 * 3. accumulate, thread = texel, for the views v = 0 .. nviews - 1 in order (triangle_id int32 [n, H, W], depth float32
 *    [n, 1, H, W]: the outputs of b3gs_mesh_resolve_batch for the same cameras and mesh; images float32 [n, 3, H, W]):
 *              p, sx, sy: statement 1 of the mesh rasterizer applied to q
 *              the view is skipped unless p_2 > 0.2, p_2 is finite, 0 <= sx <= W - 1 and 0 <= sy <= H - 1 (a NaN fails one)
 *              (i, j) = (rint(sx), rint(sy)), half to even; tid, d = triangle_id, depth there
 *              visible when tid < 0, or tid = f, or p_2 <= d + slack (one rounded sum); otherwise skipped
 * 4. weight    C = -((rot[a] t_0 + rot[3 + a] t_1) + rot[6 + a] t_2), a = 0, 1, 2: the camera centre, float32 on the host
 *              g = C - q, gl = sqrt((g_x g_x + g_y g_y) + g_z g_z); gl = 0 or not finite: skipped
 *              c = ((N_x g_x + N_y g_y) + N_z g_z) / gl; two_sided: c = |c|; c <= 0 (or NaN): skipped;  w = c c
 * 5. sample    x0 = floor(sx), fx = sx - x0, gx = 1 - fx, x1 = min(x0 + 1, W - 1); y likewise.  Per channel with
 *              I the image plane: top = gx I[y0][x0] + fx I[y0][x1], bot = gx I[y1][x0] + fx I[y1][x1], s = gy top + fy bot
 * 6. sum       accum[texel] = (A_r + w s_r, A_g + w s_g, A_b + w s_b, A_w + w): accum float32 [Ht, Wt, 4], 16-byte aligned, read
 *              once, carried through the views, written once; the caller zeroes it before the first call and may call again with
 *              further views.  Unowned texels and the texels of a triangle with an index outside 0 .. V-1 are not touched;
 *              bad_faces (device int32 [1], zeroed by the call) counts those triangles, once each.  A vertex that is not
 *              finite gives l, p or gl that is not finite: weight 0.
 * 7. fetch     the bilinear fetch of statement 5 applies to the atlas as well (W, H -> Wt, Ht; I = the uint8 texel as float).
 * 8. finalize, thread = texel.  byte(r) = (uint8) rint(255 min(max(r, 0), 1)) (a NaN gives 0).  An owned texel with A_w > 0:
 *              byte(A_ch / A_w) per channel.  An owned texel with A_w = 0: with c_k = max(b_k, 0), S = (c_0 + c_1) + c_2,
 *              c_k = c_k / S and C the uint8 vertex colours, byte((((c_0 C_0 + c_1 C_1) + c_2 C_2)) / 255) per channel; 0 when
 *              colours is NULL or the triangle has an index outside 0 .. V-1.  Unowned texels: 0.
 *              coverage (device int32 [2], zeroed by the call): [0] = owned texels with A_w > 0, [1] = owned texels.
 * 9. resolve   b3gs_mesh_resolve_batch (statement 7 there) with the same workspace, the same E_k, b_k, w_k, z, triangle_id,
 *              depth, alpha and face_pixels; the colour of a covered pixel is, with (U_k, V_k) the corners of its triangle,
 *              u = ((w_0 U_0 + w_1 U_1) + w_2 U_2) * z, v likewise, u = min(max(u, 0), Wt - 1), v = min(max(v, 0), Ht - 1),
 *              then statement 7's fetch per channel, divided by 255.  Empty pixels take bg. */
#define B3GS_TEXTURE_MIN_CELL 4
#define B3GS_TEXTURE_MAX_CELL 256
#define B3GS_MAX_ATLAS_SIDE 16384
int32_t b3gs_mesh_texture_atlas_height(int64_t F, int32_t cell, int32_t Wt);
int b3gs_mesh_texture_accumulate_batch(int32_t nviews, const float* cameras, int32_t W, int32_t H, int32_t V, int64_t F,
                                       const float* vertices, const int32_t* faces, int32_t cell, int32_t Wt, int32_t Ht,
                                       const int32_t* triangle_id, const float* depth, const float* images, float slack,
                                       int32_t two_sided, float* accum, int32_t* bad_faces, b3gs_stream_t stream);
int b3gs_mesh_texture_finalize(int32_t V, int64_t F, const uint8_t* colours, const int32_t* faces, int32_t cell, int32_t Wt, int32_t Ht,
                               const float* accum, uint8_t* texture, int32_t* coverage, b3gs_stream_t stream);
int b3gs_mesh_resolve_textured_batch(int32_t nviews, const float* cameras, int32_t W, int32_t H, int32_t V, int64_t F,
                                     const float* vertices, const int32_t* faces, const void* workspace, const float* bg,
                                     const uint8_t* texture, int32_t cell, int32_t Wt, int32_t Ht, int32_t* triangle_id, float* depth,
                                     float* alpha, float* colour, int32_t* face_pixels, b3gs_stream_t stream);

/* ---- smoothing an extracted mesh: vertex adjacency, Taubin filter, vertex normals, shaded resolve (ABI 18, added entry points;
 * binocular3dgs_amd/mesh_tools.py, mesh_render.py) --------------------------------------------------
 * Six entry points ADDED to ABI 18: no existing declaration, struct or meaning changes, so the number stays.
 * Integer work, stable sorts, ordered scans, and fp64 / float32 statements of one correctly rounded operation each that ONE
 * thread per vertex (or pixel) executes in one fixed order: tests/meshsmooth_ref.py restates every statement in numpy and every
 * output agrees bit for bit.  The translation unit is compiled with -ffp-contract=off; no floating-point atomic anywhere.
 * Nothing synchronises or reads the device: every call is capturable in a graph.  The workspace is 256-byte aligned,
 * b3gs_mesh_adjacency_workspace_bytes(V, F) bytes (0 for bad sizes; about 130 bytes per triangle and 50 per vertex), needs no
 * initial content, and is what build fills and smooth / vertex_normals read: it stays valid while the faces are unchanged.
 * V <= 2^31 - 1, 6 F <= 2^31 - 1.
 *
 * a. validity  a face with an index outside 0 .. V-1 is bad: counted, and it contributes nothing anywhere.  A vertex with a
 *              coordinate that is not finite is counted (by build, smooth and vertex_normals alike, each for the vertices it
 *              is given: word 1 below describes the latest call).  Every kernel still runs to its end; with such vertices the
 *              positions and normals are unspecified.
 * b. pairs     every good face (a, b, c) gives the ordered pairs (a,b), (b,a), (b,c), (c,b), (c,a), (a,c); a pair with equal
 *              ends is dropped.  The pairs are sorted stably by second, then by first, the two orders composed; head flags and
 *              the ordered scan give the distinct pairs.  The neighbours of vertex i are the seconds of its distinct pairs,
 *              ascending: CSR, offsets int32 [V + 1] and indices int32 [<= 6 F].
 * c. edges     a distinct pair with first < second is an undirected edge; m, the length of its run in the sorted list, is the
 *              number of good faces that contain it (a face listed twice counts twice, and a degenerate face (a, a, b) names
 *              its one edge twice).  m = 1: boundary, m = 2: interior,
 *              m > 2: non-manifold.  A vertex is pinned-eligible when it is an end of an edge with m != 2, isolated when its
 *              neighbour list is empty.
 * d. incidence each good face gives three (corner, face) slots, a vertex named twice by the face one; sorted stably by vertex:
 *              the faces of a vertex in face-index order.
 * e. totals    eight int64 at the START of the workspace: {bad faces, vertices that are not finite, distinct undirected edges,
 *              boundary edges, non-manifold edges, pinned-eligible vertices, isolated vertices, good faces}.
 * f. step      with factor k, thread = vertex i with neighbours j_0 < j_1 < .. (deg of them), per axis, fp64 from float32:
 *                s = 0;  s += (double) x_j  for j ascending;  m = s / (double) deg;  d = m - (double) x_i;  t = k * d
 *                x'_i = (float)((double) x_i + t)
 *              An isolated vertex is copied, and with pin_boundary so is a pinned-eligible one.  Jacobi: a step reads one
 *              buffer and writes the other.  iterations = n: steps 0 .. 2n - 1, the even ones with k = lambda, the odd ones
 *              with k = mu; mu = 0 skips the odd ones (a Laplacian filter of n steps); n = 0 copies.  0 < lambda <= 1, and mu = 0
 *              or mu < -lambda (Taubin); n <= 2^20.  out_vertices may be the input.
 * g. normals   thread = vertex, over its incident faces in face-index order, fp64 from float32, one operation per statement:
 *                u = p1 - p0, v = p2 - p0;  n = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x);  N += n per component
 *              l = sqrt((N_x N_x + N_y N_y) + N_z N_z);  normal = (float)(N_a / l) per component, (0, 0, 0) when l is 0 or not
 *              finite.  Area weights only.
 * h. shaded    b3gs_mesh_resolve_batch (statement 7 of the rasterizer) with the same cameras, faces and workspace, the same E_k,
 *              b_k, w_k, z, triangle_id, depth, alpha and face_pixels; normals float32 [V, 3].  The colour of a covered pixel, in
 *              float32, with n_k the normals of the winner's corners:
 *                g_a = ((w_0 n_0a + w_1 n_1a) + w_2 n_2a) * z                                     world space, a = x, y, z
 *                c_r = (rot[3r] g_x + rot[3r+1] g_y) + rot[3r+2] g_z                              camera space
 *                l = sqrt((c_x c_x + c_y c_y) + c_z c_z) (correctly rounded);  c = c / l per component (0 when l is 0 or not
 *                finite), negated when the winner has A > 0
 *                B3GS_MESH_SHADE_SMOOTH  (c + 1) * 0.5 per component
 *                B3GS_MESH_SHADE_LIT     t = max(-c_z, 0);  v = 0.85 t;  v = v + 0.15: a grey headlight, on the three channels
 *              Empty pixels take bg.
 * b3gs_mesh_adjacency_layout: the byte offsets in the workspace of {neighbour offsets int32 [V + 1], neighbour indices int32 [6 F],
 * incidence ranges (first, one past last) uint32 [V, 2], incident faces int32 [3 F], pinned-eligible mask uint8 [V]}, for callers
 * that read the lists (the tests do). */
#define B3GS_MESH_SHADE_SMOOTH 2
#define B3GS_MESH_SHADE_LIT 3
size_t b3gs_mesh_adjacency_workspace_bytes(int64_t V, int64_t F);
int b3gs_mesh_adjacency_layout(int64_t V, int64_t F, size_t* offsets);
int b3gs_mesh_adjacency_build(int32_t V, int64_t F, const float* vertices, const int32_t* faces, void* workspace,
                              b3gs_stream_t stream);
int b3gs_mesh_smooth(int32_t V, int64_t F, const float* vertices, void* workspace, int32_t iterations, double lambda, double mu,
                     int32_t pin_boundary, float* out_vertices, b3gs_stream_t stream);
int b3gs_mesh_vertex_normals(int32_t V, int64_t F, const float* vertices, const int32_t* faces, void* workspace, float* normals,
                             b3gs_stream_t stream);
int b3gs_mesh_resolve_shaded_batch(int32_t nviews, const float* cameras, int32_t W, int32_t H, int32_t V, int64_t F,
                                   const float* normals, const int32_t* faces, const void* workspace, const float* bg, int32_t mode,
                                   int32_t* triangle_id, float* depth, float* alpha, float* colour, int32_t* face_pixels,
                                   b3gs_stream_t stream);

/* ---- LPIPS (VGG16, version 0.1) of held-out views (ABI 18, added entry points; binocular3dgs_amd/lpips.py, evaluate.py,
 * INTEGRATION.md section 18) --------------------------------------------------------------------------------------------------
 * Three entry points ADDED to ABI 18: no existing declaration, struct or meaning changes, so the number stays.
 * The third number of the reference's metrics.py:103-117, lpips(render, gt, net_type='vgg'), from weights the caller brings:
 * nothing is fetched.  Images are the project's planar float32 [n,3,H,W]; every pointer is a device pointer except `weights`
 * and `feats` themselves, which are host structures of device pointers.  Nothing synchronises or reads the device.
 *
 * network   VGG16 `features` up to relu5_3: 3x3 convolutions (stride 1, zero padding 1, bias, ReLU) of widths
 *             64, 64 | 128, 128 | 256, 256, 256 | 512, 512, 512 | 512, 512, 512
 *           with a 2x2 stride-2 max-pool in floor mode between the groups (an odd last row or column is dropped) and none
 *           after the fifth.  Tap l = 0..4 is the output of the last ReLU of group l: C_l = 64, 128, 256, 512, 512 channels of
 *           H_l x W_l = floor(H / 2^l) x floor(W / 2^l) pixels.
 * input     x^ = (x - shift_c) / scale_c in float32, an IEEE division; with normalize != 0, x is 2 x - 1 first (two roundings).
 *           The zero padding of the first convolution is zero AFTER this step.
 * conv      implicit GEMM on v_mfma_f32_32x32x2_f32: float32 operands and accumulation.  Per output and per chunk of four input
 *           channels (the first convolution: its three) one k-ordered fmaf chain from 0, k = 9 c + 3 ky + kx ascending (c the
 *           input channel, (ky, kx) the tap at offset (ky - 1, kx - 1)); the chunk sums are added in chunk order from 0, then
 *           the bias, then max(., 0).
 * weights   conv_w[i]: convolution i's [Cout, Cin, 3, 3] weights repacked as [K', Cout] with row k = 9 c + 3 ky + kx, where
 *           K' = 9 Cin, but 28 for the first convolution (Cin = 3): its row 27 is zero.  conv_b[i]: [Cout].  lin[l]: [C_l],
 *           the LPIPS package's lin<l>.model.1.weight.  shift / scale: the six input constants (-.030, -.088, -.188 and
 *           .458, .448, .450 in the reference).
 * tap       per pixel of a tapped layer, in fp64 from the float32 features f (image x of the pair) and g (image y):
 *             nx = sqrt(sum_c f_c^2) + 1e-10, ny likewise;  d_c = f_c / nx - g_c / ny;  t = sum_c lin_c d_c^2   (c ascending)
 *           summed over the layer's pixels in fp64 -- per-workgroup partials in one fixed tree, folded in index order, no
 *           floating-point atomic -- and divided by H_l W_l: out[pair, l].  LPIPS of a pair is the sum of its five terms.
 *           A pair's terms have the same bits alone and at any position of a batch; identical images give exactly 0.
 * limits    1 <= npairs (nimages) <= B3GS_LPIPS_MAX_PAIRS per call; H, W >= B3GS_LPIPS_MIN_SIDE (below it the fifth layer is
 *           empty); H W <= 2^24.  Anything else: B3GS_ERR_ARG with a message, nothing launched.
 * workspace b3gs_lpips_workspace_bytes(npairs, H, W) bytes (0 for sizes outside the limits), 256-byte aligned, no initial
 *           content needed: two activation buffers of 2 npairs * 64 * H * W floats, and the tap partials.
 *           b3gs_lpips_features takes b3gs_lpips_workspace_bytes(nimages, H, W).
 * b3gs_lpips_batch     out: double [npairs, 5], the per-layer means.
 * b3gs_lpips_features  feats[l]: float32 [nimages, C_l, H_l, W_l], the five tap feature maps before normalisation. */
#define B3GS_LPIPS_CONVS 13
#define B3GS_LPIPS_TAPS 5
#define B3GS_LPIPS_MAX_PAIRS 8
#define B3GS_LPIPS_MIN_SIDE 16
typedef struct B3gsLpipsWeights {
  const float* conv_w[B3GS_LPIPS_CONVS];
  const float* conv_b[B3GS_LPIPS_CONVS];
  const float* lin[B3GS_LPIPS_TAPS];
  float shift[3];
  float scale[3];
} B3gsLpipsWeights;
size_t b3gs_lpips_workspace_bytes(int32_t npairs, int32_t H, int32_t W);
int b3gs_lpips_batch(int32_t npairs, const float* x, const float* y, int32_t H, int32_t W, const B3gsLpipsWeights* weights,
                     int32_t normalize, double* out, void* workspace, b3gs_stream_t stream);
int b3gs_lpips_features(int32_t nimages, const float* x, int32_t H, int32_t W, const B3gsLpipsWeights* weights, int32_t normalize,
                        float* const* feats, void* workspace, b3gs_stream_t stream);

/* ---- per-Gaussian render contribution (added to ABI 18) ------------------------------------------------
 * A second walk of the tile lists that a finished forward left on the device (b3gs_forward_raw[_batch] with the blend, or
 * b3gs_blend_forward_batch): per pixel the list the blend backward walks -- segment 1 followed by segment 2 -- over the
 * positions below that pixel's n_contrib (clamped to the list length), transmittance T restarted from 1.  An entry is
 * blended exactly where the forward blended it (not power > 0, alpha = min(0.99, opacity exp(power)) >= 1/255, evaluated by
 * the forward's own device function); the saturation stop is not evaluated again, n_contrib ends the walk in front of the
 * stopping entry.  Every blended (pixel, entry) has the weight w = alpha * T, T the transmittance in front of the entry; the
 * alpha image of the forward is the sum of w over a pixel's entries.
 *
 * Four arrays of [P], shared by all views of a call and ACCUMULATED INTO (the caller zeroes them):
 *   weight_q32  sum of rint(w * 2^32) over the counted pixels.  The product is exact in float32; the conversion rounds to
 *               nearest, ties to even (it only rounds where w < 2^-9); 64-bit integer adds.  weight = weight_q32 / 2^32.
 *   hits        number of (view, pixel) the Gaussian was blended into
 *   wmax_bits   float32 bits of the largest w (w >= 0, so unsigned order is float order); unsigned max
 *   dominant    number of (view, pixel) at which it has the largest w of the pixel; ties go to the first in list order
 * Nothing but integer adds and max reaches memory: the results do not depend on any order, a view gives the same bits
 * alone and at any position of a batch, and two calls give the same bits.  The 32-bit counters wrap after 2^32 pixels:
 * fold and zero them between calls (8 views of 16k x 16k still fit one call).
 * pixel_mask: [H*W] bytes, nonzero = count the pixel; NULL = every pixel.  Pixels outside W x H never count.
 * The call reads geometry / binning / image and writes only the four arrays.  All views share P.  1..8 views per call;
 * arguments are checked before the first HIP call (B3GS_ERR_ARG). */
typedef struct B3gsContribView {
  const B3gsScene* view;         /* P, W, H are read */
  const char* geometry;          /* as left by b3gs_forward_raw[_batch] + the blend forward of this view */
  const char* binning;
  const char* image;
  const uint8_t* pixel_mask;     /* [H*W], nonzero = count this pixel; NULL = every pixel */
} B3gsContribView;
typedef struct B3gsContribOut {  /* [P] each, shared by all views of the call, accumulated into; the caller zeroes */
  uint64_t* weight_q32;          /* sum over counted pixels of rint(w * 2^32), w = alpha * T (T before the blend) */
  uint32_t* hits;                /* number of (view, pixel) the Gaussian was blended into */
  uint32_t* wmax_bits;           /* bits of the largest float32 w (w >= 0: unsigned order = float order) */
  uint32_t* dominant;            /* number of (view, pixel) where it has the largest w; ties: first in list order */
} B3gsContribOut;
int b3gs_blend_contribution_batch(int32_t nviews, const B3gsContribView* views, const B3gsContribOut* out, b3gs_stream_t stream);

/* ---- per-pixel geometry maps (added to ABI 18) ----------------------------------------------------------
 * The same second walk of a finished forward's tile lists (above: positions below the pixel's n_contrib, T restarted from 1,
 * an entry blended exactly where the forward blended it, w = alpha * T with T the transmittance in front of the entry),
 * reduced per PIXEL.  With d the camera-space depth of an entry's render record, five planes of [H*W] words per view:
 *
 *   median_depth  float32  d of the last blended entry whose T BEFORE the blend was > 0.5: the entry at which T crosses one
 *                          half, or the last blended entry when T never gets there (a pixel of alpha < 0.5); 0 when nothing
 *                          was blended.  A copy of the record's float, no arithmetic.
 *   depth_m1      float32  sum of w d   in list order, acc = fmaf(d, w, acc): the forward's statement of its depth image
 *   depth_m2      float32  sum of w d d in list order, acc = fmaf(w * d, d, acc)
 *   dominant      int32    Gaussian index of the largest w; ties: the first in list order; -1 when nothing was blended
 *   count         int32    number of blended entries
 *
 * Any plane pointer may be NULL: that plane is not written.  Every pixel inside W x H writes every other plane, so the planes
 * need no initial content.  The entry that saturates a pixel (T (1 - alpha) < 1e-4) stops it WITHOUT being blended and is in
 * none of the planes.  No atomics and no reduction across pixels: a view's planes are the same bits whatever else the call
 * holds.  The call reads geometry / binning / image and writes only the planes.  All views share P (P == 0: nothing is
 * done), sizes may differ.  1..8 views per call; arguments are checked before the first HIP call (B3GS_ERR_ARG). */
typedef struct B3gsPixelMapView {
  const B3gsScene* view;         /* P, W, H are read */
  const char* geometry;          /* as left by b3gs_forward_raw[_batch] + the blend forward of this view */
  const char* binning;
  const char* image;
  float* median_depth;           /* [H*W] each; NULL = not wanted */
  float* depth_m1;
  float* depth_m2;
  int32_t* dominant;
  int32_t* count;
} B3gsPixelMapView;
int b3gs_blend_pixel_maps_batch(int32_t nviews, const B3gsPixelMapView* views, b3gs_stream_t stream);

/* ---- segmentation from 2D label planes (added to ABI 18; binocular3dgs_amd/segment.py, csrc/segment.hip) ----------
 * Two more reductions of the same second walk of a finished forward's tile lists (above: positions below the pixel's
 * n_contrib, T restarted from 1, an entry blended exactly where the forward blended it, w = alpha * T with T the
 * transmittance in front of the entry).  Labels are bytes 0 .. nlabels - 1, 1 <= nlabels <= B3GS_MAX_LABELS; a byte
 * >= nlabels means "no label" (255 is the conventional spelling).
 *
 * b3gs_label_votes_batch: every pixel gives the weight it received from a Gaussian to the label the pixel carries.
 *   labels     per view, [H*W] bytes, required.  A pixel whose byte is >= nlabels is not walked; pixels outside W x H never count.
 *   votes_q32  uint64 [P * nlabels], row-major [P][nlabels], shared by all views of the call and ACCUMULATED INTO (the caller
 *              zeroes it).  votes_q32[g][l] = the sum of rint(w * 2^32) over the blended (view, pixel, entry) of Gaussian g at
 *              the pixels labelled l -- the weight_q32 of b3gs_blend_contribution_batch under pixel_mask = (labels == l), the
 *              same bits, for every l in one walk.  The product is exact in float32; the conversion rounds to nearest, ties to
 *              even; 64-bit integer adds.  votes = votes_q32 / 2^32.
 *   Nothing but integer adds reaches memory: the bits do not depend on the order of waves, tiles, views or calls.
 *
 * b3gs_label_render_batch: the inverse direction, a label map of per-Gaussian labels.
 *   gaussian_label  [P] bytes, shared by all views.  A Gaussian whose byte is >= nlabels adds to no sum.
 *   For each label l, S_l = the float32 sum, in list order, of w over the pixel's blended entries whose Gaussian carries l
 *   (S_l = S_l + w, one rounding per entry).  Two planes of [H*W] per view, both required:
 *   label   uint8    the smallest l that holds the largest S_l when that S_l > 0, otherwise 255
 *   weight  float32  that S_l, or 0
 *   Pixels that walk nothing (n_contrib == 0) get 255 and 0; every pixel inside W x H is written, the planes need no initial
 *   content.  No atomics and no reduction across pixels: a view's planes are the same bits alone and at any position of a batch.
 *
 * Both calls read geometry / binning / image and write only their outputs; neither reads anything back to the host.  All
 * views share P (P == 0: nothing is done), sizes may differ.  1..8 views per call; arguments are checked before the first
 * HIP call (B3GS_ERR_ARG). */
#define B3GS_MAX_LABELS 16
typedef struct B3gsLabelVoteView {
  const B3gsScene* view;         /* P, W, H are read */
  const char* geometry;          /* as left by b3gs_forward_raw[_batch] + the blend forward of this view */
  const char* binning;
  const char* image;
  const uint8_t* labels;         /* [H*W], the label of every pixel; a byte >= nlabels: the pixel votes for nothing */
} B3gsLabelVoteView;
typedef struct B3gsLabelRenderView {
  const B3gsScene* view;         /* P, W, H are read */
  const char* geometry;
  const char* binning;
  const char* image;
  uint8_t* label;                /* [H*W] out */
  float* weight;                 /* [H*W] out */
} B3gsLabelRenderView;
int b3gs_label_votes_batch(int32_t nviews, const B3gsLabelVoteView* views, int32_t nlabels, uint64_t* votes_q32,
                           b3gs_stream_t stream);
int b3gs_label_render_batch(int32_t nviews, const B3gsLabelRenderView* views, int32_t nlabels, const uint8_t* gaussian_label,
                            b3gs_stream_t stream);

/* ---- feature fields (added to ABI 18; binocular3dgs_amd/features.py, csrc/features.hip) --------------------------
 * The general continuous pair on the same second walk of a finished forward's tile lists (above: positions below the pixel's
 * n_contrib, T restarted from 1, an entry blended exactly where the forward blended it, w = alpha * T with T the transmittance
 * in front of the entry): a C-channel float field per Gaussian blended into [C, H, W] maps, and the adjoint that sums [C, H, W]
 * maps back onto the Gaussians.  1 <= C <= B3GS_MAX_FEATURE_CHANNELS; channels are processed 8 at a time.
 *
 * b3gs_feature_render_batch: out[c][pixel] = the float32 sum, in list order, of w f[g][c] over the pixel's blended entries,
 *   acc = fmaf(f, w, acc) from 0 -- the forward's statement of its colour planes; there is NO background term.
 *   gaussian_features  float32 [P * C], row-major [P][C], shared by all views.
 *   out                per view, float32 [C * H * W], required.  Every pixel inside W x H writes its C words (0 where nothing
 *                      was blended): the planes need no initial content.  No atomics and no reduction across pixels: a view's
 *                      planes are the same bits alone and at any position of a batch, and channel c of a call with C channels
 *                      holds the bits of that channel rendered alone.
 *
 * b3gs_feature_lift_batch: sums_q32[g][c] += the sum over the blended (view, pixel, entry) of Gaussian g of
 *   rint(float32(w * Fn) * 2^32),  Fn = min(1, max(-1, maps[c][pixel] / scale[c]))  (an IEEE float32 division).
 *   maps        per view, float32 [C * H * W], required; finite values.
 *   pixel_mask  per view, [H*W] bytes, nonzero = count the pixel; NULL = every pixel (b3gs_blend_contribution_batch's).
 *   scale       float32 [C] in HOST memory, every entry finite and > 0 (checked: B3GS_ERR_ARG); it travels in the kernel
 *               arguments.  |Fn| <= 1 keeps |w Fn| 2^32 below 2^32: choose scale[c] >= max |maps[c]| to lose nothing.
 *   sums_q32    int64 [P * C], row-major [P][C], shared by all views and ACCUMULATED INTO (the caller zeroes it);
 *               sum of w F = scale[c] * sums_q32[g][c] / 2^32.
 *   weight_q32  uint64 [P] or NULL, accumulated into: the weight_q32 of b3gs_blend_contribution_batch under the same masks,
 *               the same bits.  For maps[c] = scale[c] at the counted pixels, sums_q32[.][c] is that integer too.
 *   The product w * Fn is exact to one float32 rounding and its scaling by 2^32 is exact; the conversion rounds to nearest,
 *   ties to even.  Nothing but 64-bit integer adds reaches memory: the bits do not depend on the order of waves, tiles, views,
 *   batches or calls.
 *
 * Both calls read geometry / binning / image and write only their outputs; neither reads anything back to the host.  All
 * views share P (P == 0: nothing is done), sizes may differ.  1..8 views per call; arguments are checked before the first
 * HIP call (B3GS_ERR_ARG). */
#define B3GS_MAX_FEATURE_CHANNELS 256
typedef struct B3gsFeatureRenderView {
  const B3gsScene* view;         /* P, W, H are read */
  const char* geometry;          /* as left by b3gs_forward_raw[_batch] + the blend forward of this view */
  const char* binning;
  const char* image;
  float* out;                    /* [C*H*W] out */
} B3gsFeatureRenderView;
typedef struct B3gsFeatureLiftView {
  const B3gsScene* view;         /* P, W, H are read */
  const char* geometry;
  const char* binning;
  const char* image;
  const float* maps;             /* [C*H*W] */
  const uint8_t* pixel_mask;     /* [H*W], nonzero = count this pixel; NULL = every pixel */
} B3gsFeatureLiftView;
int b3gs_feature_render_batch(int32_t nviews, const B3gsFeatureRenderView* views, int32_t C, const float* gaussian_features,
                              b3gs_stream_t stream);
int b3gs_feature_lift_batch(int32_t nviews, const B3gsFeatureLiftView* views, int32_t C, const float* scale, int64_t* sums_q32,
                            uint64_t* weight_q32, b3gs_stream_t stream);

/* ---- weighted k-means codebooks (added to ABI 18; binocular3dgs_amd/compress.py, csrc/kmeans.hip) ---------------
 * Lloyd's algorithm over N rows x [N,D] (float32) with K codes [K,D] and optional row weights w [N] (float32, not negative;
 * NULL = 1), entirely on the stream: no host read.  1 <= D <= 64, 1 <= K <= 65536, N >= 0 (N == 0: returns B3GS_OK and does
 * nothing).  NaN and Inf inputs are undefined.
 *
 * Assignment:  h_k = float32(0.5 sum_d c_kd^2), summed in fp64 with d ascending; the score of (n, k) is the float32 chain
 *   a_0 = -h_k, a_{d+1} = fmaf(x_nd, c_kd, a_d), d = 0 .. D-1 (the exact-f32 MFMA); codes[n] = the smallest k whose a_D is
 *   largest, i.e. the nearest code up to the rounding of that chain.
 * Update:  c_k = float32(sum w_n x_n / sum w_n) over the rows with code k; sums in fp64 in a fixed order: the members of a
 *   code in row order, cut into chunks of 256 members, each chunk summed from 0 in member order, the chunk sums added from 0
 *   in chunk order.  No floating-point atomic.  A code with no member or with sum w == 0 keeps its centroid.
 * b3gs_kmeans runs assignment 0, then `iters` times (update, assignment): the returned codes belong to the returned codebook.
 *   codebook  in: the initial codes, out: the final ones        counts [K]: members of the final assignment
 *   distortion [iters + 1]: sum_n w_n |x_n - c_code(n)|^2 of assignment i, fp64 throughout, folded in a fixed order
 *   (csrc/kmeans.hip states it; tests/kmeans_ref.py reproduces it).
 * workspace: b3gs_kmeans_workspace_bytes(N, D, K) bytes (0 for sizes outside the limits), 256-byte aligned, no initial content;
 *   both calls take the same size.  Arguments are checked before the first HIP call (B3GS_ERR_ARG). */
size_t b3gs_kmeans_workspace_bytes(int32_t N, int32_t D, int32_t K);
int b3gs_kmeans_assign(int32_t N, int32_t D, int32_t K, const float* x, const float* codebook, int32_t* codes, void* workspace,
                       b3gs_stream_t stream);
int b3gs_kmeans(int32_t N, int32_t D, int32_t K, int32_t iters, const float* x, const float* weights, float* codebook,
                int32_t* codes, int32_t* counts, double* distortion, void* workspace, b3gs_stream_t stream);

/* ---- undistorting a COLMAP dataset (added to ABI 18; binocular3dgs_amd/undistort.py, csrc/undistort.hip) -------------
 * Camera models with lens distortion, by COLMAP's model id and parameter order: 2 SIMPLE_RADIAL (f, cx, cy, k), 3 RADIAL
 * (f, cx, cy, k1, k2), 4 OPENCV (fx, fy, cx, cy, k1, k2, p1, p2), 5 OPENCV_FISHEYE (fx, fy, cx, cy, k1..k4), 6 FULL_OPENCV
 * (fx, fy, cx, cy, k1, k2, p1, p2, k3..k6), 8 SIMPLE_RADIAL_FISHEYE (f, cx, cy, k), 9 RADIAL_FISHEYE (f, cx, cy, k1, k2).
 * Any other id, or n_params that does not belong to the id, is B3GS_ERR_ARG.  The B3gsCameraModel is host memory; every other
 * pointer is a device pointer unless said otherwise.  Pixel coordinates have their origin at the top-left corner of the image
 * and pixel centres at +0.5 (COLMAP's convention).  All arithmetic on coordinates is fp64; distort() on normalised coordinates
 * is one fixed sequence of operations per model (csrc/undistort.hip states it, tests/undistort_ref.py repeats it in numpy):
 * the same bits for the four models without a transcendental (2, 3, 4, 6).  One launch per call, no atomics, no host read;
 * arguments are checked before the first HIP call.
 *
 * b3gs_camera_points: n points xy [n,2] -> out [n,2].  inverse == 0: u = (x - cx) / fx, distort, x' = fx u' + cx.
 *   inverse != 0: the point whose distortion is xy, by Newton's iteration on (u, v) from the distorted point: the 2x2 Jacobian
 *   from forward differences of distort() with h = 1e-6 max(1, |coordinate|), at most 50 iterations, converged when the squared
 *   step is below 1e-22, given up when the Jacobian of an iterate has no positive determinant and trace (the iterate is
 *   behind the fold-over of the distortion) or is not finite; converged [n] (needed when inverse != 0, else optional) receives
 *   1 or 0.  A point that did not converge (it is not the image of a point in front of the fold-over) comes back unchanged.
 * b3gs_undistort_map: for every pixel (i, j) of an output pinhole W x H with focal lengths fx, fy and the principal point at
 *   (W/2, H/2): u = ((i + 0.5) - W/2) / fx, distort, x = (fx_cam u' + cx_cam) - 0.5, X = floor(x * 256 + 0.5) clamped to
 *   [-2^30, 2^30], -2^30 when not finite; map [H,W,2] int32 = (X, Y): the source position of the output pixel's centre with
 *   pixel centres at integers and 8 fractional bits.  map is 8-byte aligned.
 * b3gs_remap_batch: up to 8 uint8 sources [Hs,Ws,C] of one size, C in {1, 3, 4}, through one map [H,W,2] into out[i] [H,W,C]:
 *   x0 = X >> 8, ax = X & 255 (the same for y); the taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), each index
 *   clamped to the image, with the weights (256 - ax | ax) * (256 - ay | ay); out = (sum w p + 32768) >> 16 per channel.
 *   valid [H,W] uint8 = 255 where -128 <= X < 256 Ws - 128 and -128 <= Y < 256 Hs - 128 (the sample centre lies inside the
 *   source), else 0, and there out is 0 in every channel.  src / out are HOST arrays of nviews device pointers; src[i] is
 *   4-byte aligned.  Every output pixel owns its bytes; a wrong map gives wrong pixels, never an access outside the buffers. */
#define B3GS_MAX_REMAP_VIEWS 8
typedef struct B3gsCameraModel {
  int32_t model;         /* COLMAP's model id */
  int32_t width, height; /* the image size the parameters belong to */
  int32_t n_params;
  double params[12];
} B3gsCameraModel;
int b3gs_camera_points(const B3gsCameraModel* cam, int32_t inverse, int64_t n, const double* xy, double* out, uint8_t* converged,
                       b3gs_stream_t stream);
int b3gs_undistort_map(const B3gsCameraModel* cam, int32_t W, int32_t H, double fx, double fy, int32_t* map, b3gs_stream_t stream);
int b3gs_remap_batch(int32_t nviews, const uint8_t* const* src, int32_t Hs, int32_t Ws, int32_t C, const int32_t* map, int32_t H,
                     int32_t W, uint8_t* const* out, uint8_t* valid, b3gs_stream_t stream);

/* ---- editing a trained model (added to ABI 18; binocular3dgs_amd/edit.py, csrc/edit.hip) ----
 * A similarity is x' = s R x + t, s > 0, R a proper rotation.  B3gsSimilarity is HOST memory, all doubles: R row-major, t, s,
 * ln_s = log(s), q = the unit quaternion of R as (w, x, y, z), and the rotation matrices D1 [3x3], D2 [5x5], D3 [7x7]
 * (row-major) of the real spherical harmonics of bands 1..3 in the basis and sign convention of csrc/preprocess.hip:
 * Y_l(d)^T D_l = Y_l(R^T d)^T for every unit d (binocular3dgs_amd/edit.py: sh_rotation_matrices).  The library trusts the
 * caller that these belong together; it checks that every entry is finite and s > 0.
 * Every statement below is fp64 in the operation order written, products and sums rounded one by one (no fused multiply-add),
 * float32 inputs widened exactly, ONE rounding to float32 at the store: tests/edit_ref.py repeats it in numpy, same bits.
 *
 * b3gs_transform_points: out_i = s * ((R_i0 x + R_i1 y) + R_i2 z) + t_i for N points [N,3]; out may be in.
 * b3gs_transform_gaussians: P Gaussians, raw parameters, features_rest [P, (sh_degree+1)^2 - 1, 3], sh_degree 0..3
 *   (sh_degree 0: both features_rest pointers are ignored):
 *     xyz'       as b3gs_transform_points
 *     rotation'  = q (x) rotation, the Hamilton product in (w, x, y, z) order on the raw, un-normalised parameter r:
 *                  w' = ((qw rw - qx rx) - qy ry) - qz rz      x' = ((qw rx + qx rw) + qy rz) - qz ry
 *                  y' = ((qw ry - qx rz) + qy rw) + qz rx      z' = ((qw rz + qx ry) - qy rx) + qz rw     (the norm is kept)
 *     scaling'   = scaling + ln_s, on the raw log parameter
 *     features_rest'[band l, m, c] = (..((D_l[m][0] f[0] + D_l[m][1] f[1]) + D_l[m][2] f[2]) + ..), f[k] = features_rest[band l, k, c]
 *   features_dc and opacity do not change and are not arguments.  Every Gaussian owns its output rows and a workgroup reads
 *   its rows before it writes them: each out_* may be its input.  No atomics, no host read; P = 0 is a no-op.
 *   Under the identity similarity every finite value keeps its bits, except that a -0.0 may come back as +0.0 (x + 0.0 and
 *   0.0 * y + x are +0.0 for x = -0.0); a row of zeros stays a row of zeros.  Non-finite values propagate as IEEE has them.
 * b3gs_select_gaussians: keep[i] = 1 when Gaussian i passes every test enabled in flags, else 0; seen[i] = the number of views
 *   that see it (0 when B3GS_SELECT_VIEWS is off).  A disabled test reads nothing (its pointers may be NULL).
 *     BOX      p_k = ((M_k0 x + M_k1 y) + M_k2 z) + M_k3 with box = M [3x4] row-major world-to-box; |p_k| <= half[k] for k = 0..2
 *     SPHERE   d = x - centre; (dx dx + dy dy) + dz dz <= r2
 *     OPACITY  opacity_raw >= logit_min            (a float32 compare on the raw parameter: no transcendental on the device)
 *     SCALE    max_k scaling_raw[k] <= log_max_scale   (float32)
 *     VIEWS    cameras: DEVICE doubles [nviews][19] = [3x4 world-to-view row-major | fx fy cx cy W H near], nviews <= 64.  A view
 *              sees the Gaussian when, with (X, Y, Z) = the rows applied as in BOX, Z > near, u = (fx X) / Z + cx has
 *              0 <= u < W, v = (fy Y) / Z + cy has 0 <= v < H and, when masks (DEVICE uint8 [nviews][mask_h][mask_w]) is not
 *              NULL, masks[view][floor(v)][floor(u)] != 0 (a texel outside the plane, when W > mask_w or H > mask_h, counts
 *              as 0).  Kept when seen >= min_views.
 *   A Gaussian with a non-finite coordinate fails BOX, SPHERE and every view.  No atomics, no host read; P = 0 is a no-op.
 * b3gs_similarity_sums: over the pairs i < N with 0 <= index[i] < Nb, dist[i] <= gate (float32) and mask[i] != 0 (mask NULL:
 *   all), with a~ = a_i - origin_a and b~ = b[index[i]] - origin_b in fp64, out[18] = {n, sum a~ (3), sum b~ (3),
 *   sum ((a~x a~x + a~y a~y) + a~z a~z), sum b~ a~^T (9, row-major: b~_r a~_c), sum ((b~x b~x + b~y b~y) + b~z b~z)}.  The
 *   18th sum is what the residual of a similarity fit needs besides the other 17 (var b): one launch gives the fit AND its rms.  origin_a / origin_b are HOST doubles [3].
 *   Thread t of workgroup g (256 threads, nb = clamp(ceil(N / 2048), 1, 256) workgroups) adds i = 256 g + t, + 256 nb, .. in
 *   order; the per-workgroup partials and their fold by one wave are those of b3gs_cloud_score: the same bits on every call.
 *   No floating-point atomic.  workspace: b3gs_similarity_sums_workspace_bytes(N) bytes, no initial content. */
#define B3GS_SELECT_BOX 1
#define B3GS_SELECT_SPHERE 2
#define B3GS_SELECT_OPACITY 4
#define B3GS_SELECT_SCALE 8
#define B3GS_SELECT_VIEWS 16
#define B3GS_MAX_SELECT_VIEWS 64
typedef struct B3gsSimilarity {
  double R[9], t[3], s, ln_s, q[4], D1[9], D2[25], D3[49];
} B3gsSimilarity;
typedef struct B3gsSelect {
  int32_t flags;       /* B3GS_SELECT_* */
  int32_t nviews, min_views, mask_h, mask_w;
  float logit_min, log_max_scale;
  double box[12], half[3], centre[3], r2;
  const double* cameras;
  const uint8_t* masks;
} B3gsSelect;
int b3gs_transform_points(int64_t N, const float* in, const B3gsSimilarity* xf, float* out, b3gs_stream_t stream);
int b3gs_transform_gaussians(int32_t P, int32_t sh_degree, const float* xyz, const float* rotation, const float* scaling,
                             const float* features_rest, const B3gsSimilarity* xf, float* out_xyz, float* out_rotation,
                             float* out_scaling, float* out_features_rest, b3gs_stream_t stream);
int b3gs_select_gaussians(int32_t P, const float* xyz, const float* opacity_raw, const float* scaling_raw, const B3gsSelect* sel,
                          uint8_t* keep, int32_t* seen, b3gs_stream_t stream);
size_t b3gs_similarity_sums_workspace_bytes(int64_t N);
int b3gs_similarity_sums(int64_t N, const float* a, int64_t Nb, const float* b, const int32_t* index, const float* dist, float gate,
                         const uint8_t* mask, const double* origin_a, const double* origin_b, double* out, void* workspace,
                         b3gs_stream_t stream);

/* ---- the camera pose gradient from the per-Gaussian gradients (added to ABI 18; csrc/pose.hip) ----
 * A render from a moved camera is the render of the inversely moved scene, so the gradient of a loss with respect to a rigid
 * motion is a linear reduction of the gradients the backward already wrote.  For each of nviews <= 8 views (one launch, all
 * views share the parameters), with mu = xyz, q = rotation (raw, (w, x, y, z)), f = features_rest [P, (sh_degree+1)^2 - 1, 3]
 * and g_mu, g_q, g_f their gradients for that view, over the rows i < P with skip[view][i] == 0 (skip NULL, or skip[view] NULL:
 * all rows; a skipped row is not read):
 *   out[view] = {tau_x, tau_y, tau_z, f_x, f_y, f_z}: the gradient with respect to a world-frame twist (omega, t) of the SCENE
 *   about `pivot` c (x -> c + exp(omega) (x - c) + t); the camera's gradient is its negative.  Per row, fp64 in the operation
 *   order written, products and sums rounded one by one (no fused multiply-add), float32 inputs widened exactly:
 *     d = mu - c
 *     cross_x = d_y g_z - d_z g_y      cross_y = d_z g_x - d_x g_z      cross_z = d_x g_y - d_y g_x            (g = g_mu)
 *     h_x = ((g_x q_w - g_w q_x) + g_z q_y) - g_y q_z       = <g_q, e_x (x) q>, the Hamilton product with the pure unit e_x
 *     h_y = ((g_y q_w - g_w q_y) + g_x q_z) - g_z q_x       h_z = ((g_z q_w - g_w q_z) + g_y q_x) - g_x q_y    (g = g_q)
 *     s_x = s_y = s_z = 0; for band l = 1 .. sh_degree, for channel c = 0, 1, 2, with f[k] = f[band l, k, c], g[k] likewise
 *     of g_f, each statement "s, a, j, m" below in order is  s = s + a * (g[j] * f[m] - g[m] * f[j])  (the entry G_l[j][m] = a
 *     of the antisymmetric generator of the band rotation about that axis, d/dtheta D_l(exp(theta e_k)) at 0, and its mirror):
 *       band 1:  s_x 1 0 1;  s_y 1 1 2;  s_z 1 0 2
 *       band 2:  s_x 1 0 3;  s_x r3 1 2;  s_x 1 1 4;  s_y -1 0 1;  s_y r3 2 3;  s_y 1 3 4;  s_z 2 0 4;  s_z 1 1 3
 *       band 3:  s_x r6/2 0 5;  s_x r10/2 1 4;  s_x r6/2 1 6;  s_x r6 2 3;  s_x r10/2 2 5;  s_y -r6/2 0 1;  s_y -r10/2 1 2;
 *                s_y r6 3 4;  s_y r10/2 4 5;  s_y r6/2 5 6;  s_z 3 0 6;  s_z 2 1 5;  s_z 1 2 4
 *       r3 = 1.7320508075688772, r6 = 2.4494897427831779, r6/2 = 1.2247448713915890, r10/2 = 1.5811388300841898
 *     tau_k += (cross_k + 0.5 * h_k) + s_k          f_k += g_mu_k
 *   Thread t of workgroup g (256 threads, nb = clamp(ceil(P / 1024), 1, 1024) workgroups per view) adds the rows i = 256 g + t,
 *   + 256 nb, .. in order, each of the six sums starting from +0; the per-workgroup partials and their fold by one wave are
 *   those of b3gs_similarity_sums: the same bits on every call.  No floating-point atomic, no host read.
 *   sh_degree 0 reads neither features_rest pointer.  P = 0 writes zeros (no pointer but pivot and out is read).  Non-finite
 *   inputs propagate as IEEE has them.  B3GS_ERR_ARG before the first HIP call: nviews outside 1 .. 8, sh_degree outside
 *   0 .. 3, P < 0, a non-finite pivot, a NULL required pointer.
 *   grad_xyz / grad_rotation / grad_features_rest / skip are HOST arrays of nviews DEVICE pointers, pivot is HOST double[3], out
 *   is DEVICE double[nviews][6]; workspace: b3gs_pose_gradient_workspace_bytes(P, nviews) bytes, no initial content. */
#define B3GS_MAX_POSE_VIEWS 8
size_t b3gs_pose_gradient_workspace_bytes(int32_t P, int32_t nviews);
int b3gs_pose_gradient(int32_t P, int32_t sh_degree, int32_t nviews, const float* xyz, const float* rotation,
                       const float* features_rest, const float* const* grad_xyz, const float* const* grad_rotation,
                       const float* const* grad_features_rest, const uint8_t* const* skip, const double* pivot, double* out,
                       void* workspace, b3gs_stream_t stream);

/* ---- merging Gaussians: moment-matched levels of detail (added to ABI 18; csrc/lod.hip, binocular3dgs_amd/lod.py, INTEGRATION.md
 * section 26) ------------------------------------------------------------------------------------------------------------------
 * Three entry points ADDED to ABI 18: no existing declaration, struct or meaning changes, so the number stays.
 * The mergeable Gaussians of one grid cell are replaced by the ONE Gaussian with the mass-weighted mean and covariance of their
 * mixture.  The inputs are ACTIVATED float32 values: positions [P,3], scales [P,3] > 0, quaternions [P,4] (w, x, y, z; any
 * non-zero norm), opacities [P] in (0, 1), features_dc [P,3], features_rest [P, K, 3] with K in {0, 3, 8, 15} coefficients
 * per channel, an optional float64 weights [P] >= 0 (NULL: none), a float32 cell > 0.  P < 2^24.  No exp, log or sigmoid runs
 * here: only + - * / sqrt and comparisons, in fp64 unless stated, every statement ONE operation (the translation unit is
 * compiled with -ffp-contract=off), one thread per output in one fixed order: tests/lod_ref.py restates every statement and
 * every output agrees bit for bit.  No floating-point atomic, no vendor library, no host read.
 *
 * 1. box        o = the per-axis float32 minimum of the positions.  A row (Gaussian) with a value that is not finite in ANY
 *               input is counted, once.  c_a = floor((x_a - o_a) / cell): two rounded float32 operations, then the floor.  A
 *               c_a outside 0 .. 1023 (or NaN) is counted, not clamped.  key = (c_z << 20) | (c_y << 10) | c_x.
 * 2. mergeable  max(s_0, s_1, s_2) <= cell, compared in float32.  A Gaussian that is not mergeable passes through untouched.
 * 3. clusters   the mergeable Gaussians of one key, in index order (a stable sort by key).
 * 4. order      output rows: the clusters in ascending key order, then the pass-throughs in index order.  A cluster of one
 *               member and every pass-through is a copy of its input words, bit for bit (the quaternion as given).
 * 5. a cluster of n >= 2 members i (in order) makes one Gaussian:
 *      v_i = (s_0 s_1) s_2,  a_i = alpha_i v_i,  A = sum a_i,  W = sum w_i a_i        (each sum from +0, one addition per member)
 *      m_i = w_i a_i and M = W when weights are given and W != 0; otherwise m_i = a_i and M = A
 *      S_a = sum m_i x_ia;  mu_a = S_a / M
 *      per member: n = sqrt(((w w + x x) + y y) + z z) of its quaternion, (w, x, y, z) each / n,
 *        R = [1 - 2 (y y + z z), 2 (x y - w z), 2 (x z + w y);  2 (x y + w z), 1 - 2 (x x + z z), 2 (y z - w x);
 *             2 (x z - w y), 2 (y z + w x), 1 - 2 (x x + y y)],   u_k = s_k s_k,   d_a = x_ia - mu_a,
 *        cov_ab = ((R_a0 u_0) R_b0 + (R_a1 u_1) R_b1) + (R_a2 u_2) R_b2
 *        C_ab = C_ab + m_i (cov_ab + d_a d_b)          for the six entries 00, 01, 02, 11, 12, 22
 *      Sigma_ab = C_ab / M
 *      eigen-decomposition: cyclic Jacobi, V = I, B3GS_MERGE_JACOBI_SWEEPS sweeps over (p, q) = (0,1), (0,2), (1,2); a
 *        rotation is skipped when a_pq == 0, else with r the third index
 *          theta = (a_qq - a_pp) / (2 a_pq);  t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta theta + 1))
 *          c = 1 / sqrt(t t + 1);  s = t c;  tau = t a_pq;  a_pp = a_pp - tau;  a_qq = a_qq + tau;  a_pq = 0
 *          (a_rp, a_rq) = (c a_rp - s a_rq, s a_rp + c a_rq);  per row k of V: (v_kp, v_kq) = (c v_kp - s v_kq, s v_kp + c v_kq)
 *        lambda = the diagonal, sorted descending with its columns of V by insertion (strict >: ties keep column order);
 *        det V = (v00 (v11 v22 - v12 v21) - v01 (v10 v22 - v12 v20)) + v02 (v10 v21 - v11 v20) < 0: the third column is negated
 *      floor: f = z z with z the smallest float32 scale of any member; lambda_k < f: lambda_k = f.  s'_k = sqrt(lambda_k)
 *      quaternion of V by Shepperd's branches, T = (v00 + v11) + v22:
 *        T > 0:                     g = 2 sqrt(T + 1):                  (g / 4, (v21 - v12) / g, (v02 - v20) / g, (v10 - v01) / g)
 *        else v00 > v11, v00 > v22: g = 2 sqrt(((1 + v00) - v11) - v22): ((v21 - v12) / g, g / 4, (v01 + v10) / g, (v02 + v20) / g)
 *        else v11 > v22:            g = 2 sqrt(((1 + v11) - v00) - v22): ((v02 - v20) / g, (v01 + v10) / g, g / 4, (v12 + v21) / g)
 *        else:                      g = 2 sqrt(((1 + v22) - v00) - v11): ((v10 - v01) / g, (v02 + v20) / g, (v12 + v21) / g, g / 4)
 *        (g / 4 is 0.25 g), divided by its norm as above, all four negated when w < 0
 *      opacity: alpha' = A / ((s'_0 s'_1) s'_2), clamped to [1 / 255, 0.99]: the mass sum a_i is preserved where the clamp
 *        does not bite; unlike m_i it does not use the weights
 *      colour: every channel f of features_dc and features_rest: (sum m_i f_i) / M, from +0, members in order
 *      every output is rounded once to float32.
 *    The sweep count is the smallest at which tests/lod_ref.py agrees with numpy.linalg.eigh to 1e-13 (relative to the largest
 *    eigenvalue, eigenvalues and V diag(lambda) V^T) on 10^5 random and degenerate symmetric 3 x 3 matrices.
 *
 * count leaves int64 words at the START of the workspace: {clusters, pass-throughs, merged members (members of clusters with
 * n >= 2), rows that are not finite, rows beyond the 1024 cells of an axis}, then two more {output rows = clusters +
 * pass-throughs, the float32 bits of the largest box edge}.  The caller reads them ONCE and hands the first five to emit as a
 * HOST array; emit fails with B3GS_ERR_ARG and the count in b3gs_last_error() when either error word is not zero, otherwise
 * fills the outputs ([rows, ..]), cluster_of [P] (the output row of every input) and members [rows] (the member count of
 * every output row), and writes nothing past `rows` rows.  emit takes the arguments of count and the same workspace
 * (256-byte aligned, b3gs_gaussian_merge_workspace_bytes(P, K) bytes, about 70 bytes per Gaussian; 0 for bad sizes).
 * A cluster may have any number of members (one thread walks them). */
#define B3GS_MERGE_JACOBI_SWEEPS 4
size_t b3gs_gaussian_merge_workspace_bytes(int64_t P, int32_t K);
int b3gs_gaussian_merge_count(int32_t P, int32_t K, const float* positions, const float* scales, const float* quaternions,
                              const float* opacities, const float* features_dc, const float* features_rest, const double* weights,
                              float cell, void* workspace, b3gs_stream_t stream);
int b3gs_gaussian_merge_emit(int32_t P, int32_t K, const float* positions, const float* scales, const float* quaternions,
                             const float* opacities, const float* features_dc, const float* features_rest, const double* weights,
                             float cell, void* workspace, const int64_t* totals, float* out_positions, float* out_scales,
                             float* out_quaternions, float* out_opacities, float* out_features_dc, float* out_features_rest,
                             int32_t* cluster_of, int32_t* members, b3gs_stream_t stream);

/* ---- screened Poisson surface reconstruction (added to ABI 18; csrc/poisson.hip, binocular3dgs_amd/poisson.py, INTEGRATION.md
 * section 27) ---------------------------------------------------------------------------------------------------------------
 * Eight entry points ADDED to ABI 18: no existing declaration, struct or meaning changes, so the number stays.
 * Oriented samples -> one smooth function over the node grid of a B3gsTsdfVolume (nodes at the voxel centres, x fastest) whose
 * level set b3gs_mesh_count / b3gs_mesh_emit extract unchanged.  float32 unless stated, every statement ONE correctly rounded
 * operation of + - * / sqrt in the order written (the library is built with -ffp-contract=off), one thread per output word,
 * sums across threads as fixed-order fp64 folds: no floating-point atomic, no vendor library, and one result whatever the launch
 * geometry.  tests/poisson_ref.py restates every statement in numpy; every output agrees bit for bit.
 *
 * 1. b3gs_oriented_points_batch / _emit: 1..8 views (B3gsTsdfView) of one W x H, W * H <= 2^27.  Pixel (px, py) of a view
 *    qualifies when px % stride == 0 and py % stride == 0, 1 <= px <= W - 2, 1 <= py <= H - 2, and alpha >= alpha_min at the
 *    pixel and at (px - 1, py), (px + 1, py), (px, py - 1), (px, py + 1).  z = depth / alpha at each of the five (the renderer's
 *    mean depth, as b3gs_tsdf_integrate_batch defines it), or z = depth as given when `median` != 0.
 *      rejected unless |z_n - z| <= rel_jump * z for the four neighbours n
 *      P(q) = (((qx - (0.5 W - 0.5)) / fx) * z_q, ((qy - (0.5 H - 0.5)) / fy) * z_q, z_q)
 *      a = P(px + 1, py) - P(px - 1, py);  b = P(px, py + 1) - P(px, py - 1);  n = b x a, n_0 = b_1 a_2 - b_2 a_1 and cyclic:
 *      the side that faces the camera
 *      |n| = sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2), rejected unless > 0;  |P| likewise
 *      c = (0 - ((n_0 P_0 + n_1 P_1) + n_2 P_2)) / (|n| |P|), rejected unless c > min_cos
 *      u = n / |n|;  position_k = (rot[k] t_0 + rot[3 + k] t_1) + rot[6 + k] t_2 with t = P - trans (R^T (P - t));
 *      normal_k likewise from u;  weight = c;  colour = the pixel's three colour words
 *    The accepted pixels are compacted in (view, py, px) order.  batch leaves their number as ONE int64 at the start of the
 *    workspace (b3gs_oriented_points_workspace_bytes, 0 for bad sizes; 256-byte aligned): the only word the host reads; emit,
 *    with the same arguments and workspace, fills points [n, 3], normals [n, 3], weights [n], colours [n, 3] and writes nothing
 *    past n rows.
 * 2. b3gs_poisson_splat: per sample and axis a, c = (x_a - origin_a) / voxel - 0.5, base = floor(c), f = c - base.  A sample
 *    whose base is outside 0 .. n_a - 2 on any axis (its 8 surrounding nodes are not all in the grid; NaN included) is dropped
 *    and counted.  The others are sorted by the key (base_z ny + base_y) nx + base_x with the stable radix sort: the members of a
 *    cell stay in sample order.  One thread per node visits its 8 cells (node - (dx, dy, dz)) for dz, dy, dx in {0, 1}, dx
 *    fastest, and every member in order:  t_a = d_a ? f_a : 1 - f_a;  t = (t_x t_y) t_z;  in fp64 wt = w t (exact),
 *    D = D + wt, V_a = V_a + wt n_a;  the four sums start at +0 and are rounded once to float32: density [n], vector [3, n].
 * 3. b = 0 - 0.5 (((Vx(i+1) - Vx(i-1)) + (Vy(j+1) - Vy(j-1))) + (Vz(k+1) - Vz(k-1))), a value beyond the grid is 0.
 *    A x = (((x_c - x(i-1)) + (x_c - x(i+1))) + ((x_c - x(j-1)) + (x_c - x(j+1)))) + ((x_c - x(k-1)) + (x_c - x(k+1)))
 *          + (screen D_c) x_c, a neighbour beyond the grid is the node itself (Neumann).  b3gs_poisson_apply: out = A x.
 *    A is symmetric positive definite when screen > 0 and some D > 0.
 * 4. b3gs_poisson_solve: conjugate gradients from x = 0, r = p = b, `iters` iterations of TWO launches, no host read.
 *    x, r, p, Ap are float32; a dot product u.v: q_i = (double)u_i (double)v_i (exact); one partial per 256 consecutive nodes
 *    (missing nodes are +0): per 64 the xor butterfly 32, 16, .., 1, then (s_0 + s_1) + (s_2 + s_3); the partials are folded by
 *    one wave: lane l adds l, l + 64, .. in order from +0, then the butterfly.  All of that in fp64.
 *      rr = bb = b.b;  thr = (tol tol) bb (fp64);  done when rr <= thr or no sample survived the splat (status bit 0)
 *      per iteration, unless done:  p = r + bf p (from the second iteration on);  pAp = p.Ap;  pAp == 0: done;
 *        alpha = rr / pAp, af = (float)alpha;  x = x + af p;  r = r - af Ap;  rn = r.r;  beta = rn / rr, bf = (float)beta;
 *        rr = rn;  iterations = iterations + 1;  done when rn <= thr
 *    Once done, later launches return without writing.  The partial of a chunk of 256 nodes does not depend on the workgroup
 *    that made it; the LAST workgroup of a launch to finish folds them (an arrival counter; nobody waits), so max_blocks (0: at
 *    most 2048 workgroups, each walking chunks b, b + grid, ..) changes no bit.  Also written: rhs [n] = b.
 *    The workspace begins with int64 words {dropped samples, samples, status, iterations, done} and the doubles {rr, bb}: the
 *    caller reads them once.  screen <= 0 is B3GS_ERR_ARG.
 * 5. b3gs_poisson_volume: iso = (float)(sum(D x) / sum(D)), the two sums as dot products above;  tsdf = x - iso (normals point
 *    to free space: positive outside);  weight = D summed over the (2 spread + 1)^3 box of nodes clipped to the grid, one axis
 *    after the other (x, y, z), each in index order from +0;  rgb = 0.
 * workspace: b3gs_poisson_workspace_bytes(nx, ny, nz, nsamples) bytes (0 for bad sizes; about 32 bytes per node and 36 per
 * sample), 256-byte aligned.  ORDER: b3gs_poisson_splat needs no initial content and writes the head words {dropped samples,
 * samples}; b3gs_poisson_solve READS those two words (the status bit "no sample survived"), so it takes the workspace the splat
 * of the same grid wrote, after it on the stream -- on any other bytes its status and stop flag are undefined.
 * b3gs_poisson_volume reads nothing of the head and only uses the node arrays as scratch (the solver's state is lost).
 * b3gs_poisson_apply takes no workspace. */
size_t b3gs_oriented_points_workspace_bytes(int32_t nviews, int32_t W, int32_t H);
int b3gs_oriented_points_batch(int32_t nviews, const B3gsTsdfView* views, int32_t W, int32_t H, int32_t stride, float alpha_min,
                               float rel_jump, float min_cos, int32_t median, void* workspace, b3gs_stream_t stream);
int b3gs_oriented_points_emit(int32_t nviews, const B3gsTsdfView* views, int32_t W, int32_t H, int32_t stride, float alpha_min,
                              float rel_jump, float min_cos, int32_t median, void* workspace, int64_t npoints, float* points,
                              float* normals, float* weights, float* colours, b3gs_stream_t stream);
size_t b3gs_poisson_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, int64_t nsamples);
int b3gs_poisson_splat(const B3gsTsdfVolume* grid, int64_t nsamples, const float* points, const float* normals, const float* weights,
                       float* density, float* vector, void* workspace, b3gs_stream_t stream);
int b3gs_poisson_apply(const B3gsTsdfVolume* grid, const float* density, float screen, const float* x, float* out, b3gs_stream_t stream);
int b3gs_poisson_solve(const B3gsTsdfVolume* grid, const float* density, const float* vector, float screen, int32_t iters, float tol,
                       int32_t max_blocks, float* rhs, float* x, void* workspace, b3gs_stream_t stream);
int b3gs_poisson_volume(const B3gsTsdfVolume* volume, const float* density, const float* x, int32_t spread, void* workspace,
                        b3gs_stream_t stream);

/* ---- fixed-budget training: MCMC relocation and position noise (added to ABI 18; csrc/mcmc.hip, binocular3dgs_amd/mcmc.py,
 * INTEGRATION.md section 29) ------------------------------------------------------------------------------------------------
 * Five entry points ADDED to ABI 18: no existing declaration, struct or meaning changes, so the number stays.
 * tests/mcmc_ref.py restates every rule below in numpy / Python integers.
 *
 * 1. Random numbers: Philox4x32-10 (Salmon et al., SC 2011).  One round of counter c[4] under key k[2]:
 *      p0 = 0xD2511F53 * c[0], p1 = 0xCD9E8D57 * c[2]  (64-bit products)
 *      c = { hi(p1) ^ c[1] ^ k[0], lo(p1), hi(p0) ^ c[3] ^ k[1], lo(p0) };  ten rounds, and between two rounds
 *      k[0] += 0x9E3779B9, k[1] += 0xBB67AE85.
 *    The key is the 64-bit seed (k[0] its low word), the counter is (index, offset, stream_id, 0); one counter gives one BLOCK
 *    of four words w0..w3.
 *      B3GS_RANDOM_U32     element e of the output is word e % 4 of the block with index e / 4
 *      B3GS_RANDOM_NORMAL  element e (float32) comes from the block with index e / 4 and its word pair (w0, w1) when
 *                          e % 4 < 2, else (w2, w3); with (a, b) that pair, in fp64: u1 = (a + 0.5) 2^-32, u2 = (b + 0.5) 2^-32,
 *                          r = sqrt(-2 log(u1)); an even e takes r cos(2 pi u2), an odd e r sin(2 pi u2), rounded ONCE to float32
 *                          (u1 > 0: the logarithm is finite)
 *      a 64-bit draw       (relocation) of index j is w0 | w1 << 32 of the block with index j
 *    b3gs_mcmc_random fills out[n] (0 <= n <= 2^32) with uint32 or float32 words.
 * 2. b3gs_mcmc_noise: per row i of the raw parameters, in float32, every statement one rounded operation in the order written:
 *      q = rotation_i / sqrt(((w w + x x) + y y) + z z);  R the rotation matrix of q as build_rotation states it;
 *      v_k = exp(scaling_ik)^2;  t_k = ((R_0k n_0 + R_1k n_1) + R_2k n_2) v_k;  d_j = (R_j0 t_0 + R_j1 t_1) + R_j2 t_2  (= Sigma n)
 *      o = 1 / (1 + exp(-opacity_i));  g = 1 / (1 + exp(100 (o - 0.005)));  xyz_ij = xyz_ij + (d_j g) (noise_lr lr_xyz)
 *    n = normals[3 i + k] when `normals` is given, else element 3 i + k of B3GS_RANDOM_NORMAL for (seed, stream_id 0,
 *    offset = iteration), made in registers.  lr_xyz_dev (one float on the device) replaces lr_xyz when it is not NULL.
 *    No atomics, no row reads another row.
 * 3. b3gs_mcmc_relocate, in place on the six raw parameter tensors of P rows (rows [P_old, P) are the APPENDED ones of a growth
 *    step, P_old == P: none).  No host read; `workspace` holds b3gs_mcmc_workspace_bytes(P) bytes (0 for bad sizes), 256-byte
 *    aligned, no initial content.
 *      classify  o_i = 1 / (1 + exp(-(double)opacity_i)) in fp64.  Row i is DEAD when o_i <= (double)min_opacity or i >= P_old;
 *                its weight is q_i = dead ? 0 : (uint32)(o_i 2^24).
 *      scans     rank_i = the dead rows in front of i;  W_i = q_0 + .. + q_i as uint64;  total = W_(P-1).
 *      sample    the dead row of rank j takes the 64-bit draw u of (seed, stream_id 1, offset, index j) -- or draws[j] when
 *                `draws` is given -- and t = (u * total) >> 64; src_i = the first row s with W_s > t (alive, never a zero-weight
 *                row); count_s += 1.  total == 0: nothing is written at all and bit 0 of the status word is set.
 *      correct   every alive row with count > 0, in fp64, each statement one operation in the order written:
 *                N = min(count + 1, n_max);  o' = 1 - pow(1 - o, 1 / N);  p_1 = o', p_(k+1) = p_k o';
 *                denom = sum over i = 1..N, inside it k = 0..i-1, of +- (C(i-1, k) p_(k+1)) / sqrt(k + 1), added for even k and
 *                subtracted for odd k, from +0;  for each axis s' = (exp((double)scaling) o) / denom;
 *                o' clamped to [min_opacity, 1 - 2^-24];  stored (float)log(o' / (1 - o')) and (float)log(s').
 *      apply     a dead row with a source copies xyz, rotation, features_dc and features_rest from it bit for bit and takes the
 *                source's corrected opacity and scaling; the source takes them too.  The Adam moments (when given: all twelve
 *                pointers of exp_avg / exp_avg_sq, or none) of every row WRITTEN, sources and destinations, become zero.
 *    b3gs_mcmc_views: where src (int32 [P], -1: not relocated), count (int32 [P]), rank (int32 [P]), W (uint64 [P]) and the head
 *    words (int64: total, dead rows, status) of the last call lie inside the workspace. */
#define B3GS_RANDOM_U32 0
#define B3GS_RANDOM_NORMAL 1
#define B3GS_MCMC_MAX_N 51
typedef struct B3gsMcmcIO {
  int32_t P, P_old;
  int32_t K;                 /* floats of one features_rest row (0: none; features_dc rows hold 3) */
  int32_t n_max;             /* 1 .. B3GS_MCMC_MAX_N */
  float min_opacity;         /* in (0, 1) */
  uint32_t offset;
  uint64_t seed;
  float* param[6];           /* xyz, features_dc, features_rest, scaling, rotation, opacity */
  float* exp_avg[6];
  float* exp_avg_sq[6];
  const uint64_t* draws;     /* NULL, or [P] injected draws by dead rank (tests) */
} B3gsMcmcIO;
typedef struct B3gsMcmcViews {
  const int32_t* src;
  const int32_t* count;
  const int32_t* rank;
  const uint64_t* weight_scan;
  const int64_t* head;       /* [3] total weight, dead rows, status (bit 0: nothing alive, no-op) */
} B3gsMcmcViews;
int b3gs_mcmc_random(int64_t n, uint64_t seed, uint32_t stream_id, uint32_t offset, int32_t kind, void* out, b3gs_stream_t stream);
int b3gs_mcmc_noise(int32_t P, const float* scaling, const float* rotation, const float* opacity, float* xyz, const float* normals,
                    uint64_t seed, uint32_t iteration, float noise_lr, float lr_xyz, const float* lr_xyz_dev, b3gs_stream_t stream);
size_t b3gs_mcmc_workspace_bytes(int32_t P);
int b3gs_mcmc_relocate(const B3gsMcmcIO* io, void* workspace, b3gs_stream_t stream);
int b3gs_mcmc_views(int32_t P, void* workspace, B3gsMcmcViews* out);

/* ---- depth priors: Pearson depth loss and prior preparation (added to ABI 18; csrc/depthprior.hip,
 * binocular3dgs_amd/depth_prior.py) --------------------------------------------------------------
 * Three entry points ADDED to ABI 18: no existing declaration, struct or meaning changes, so the number stays.
 * tests/depth_prior_ref.py restates every rule below in numpy float64.
 *
 * 1. b3gs_depth_prior_loss_batch: per view the scale- and shift-invariant loss
 *      L = w_global (1 - rho_image) + w_local mean over the counted patches of (1 - rho_patch)
 *    between the rendered depth D and a prior P, and dL/dD.  All arithmetic is fp64, only + - * / sqrt, every statement one
 *    rounded operation in the order written.  Pixel i (row-major) is USED iff mask_i != 0 and alpha_i >= alpha_min.
 *      B3GS_DEPTH_PRIOR_DEPTH      x = D,               t' = 1
 *      B3GS_DEPTH_PRIOR_DISPARITY  x = 1 / (D + 1e-5),  t' = 0 - x x
 *    with y = P; the six quantities of a pixel are q = (1, x, y, x x, y y, x y), all zero for a pixel that is not used.
 *    The TREE of 256 values v[0..255]: the xor butterfly per group of 64 (d = 32, 16, .., 1: v[l] = v[l] + v[l ^ d]), then
 *    (g0 + g1) + (g2 + g3) of the four group results.
 *      image sums  block b holds pixels 256 b .. 256 b + 255; its partial is the TREE of their q.  The sum is the FOLD of the
 *                  partials: s[l] = the partials l, l + 64, .. added in that order to +0, then the butterfly of s[0..63].
 *      patch sums  patches of `patch` x `patch` pixels on the grid with origin (-ox, -oy); (ox, oy) = offset_dev[0..1], each
 *                  clamped to [0, patch - 1], (0, 0) when offset_dev is NULL.  Patch (i, j), 0 <= i < gx = ceil(W / patch) + 1,
 *                  0 <= j < gy = ceil(H / patch) + 1, has the local pixels k = 0 .. patch^2 - 1 at x = i patch - ox + k % patch,
 *                  y = j patch - oy + k / patch (outside the image: not used).  v[t] = q of k = t, t + 256, .. added in that
 *                  order to +0; the sum is the TREE of v.
 *      a set       with sums (n, Sx, Sy, Sxx, Syy, Sxy):  cxx = Sxx - (Sx Sx) / n, cyy = Syy - (Sy Sy) / n, cxy = Sxy - (Sx Sy) / n.
 *                  SKIPPED when n < min_valid, or not cxx > 0, or not cyy > 0: term 0, gradient 0, not counted.  Otherwise
 *                  den = sqrt(cxx cyy), rho = cxy / den, mx = Sx / n, my = Sy / n, term = 1 - rho, and for a used pixel
 *                  g = (0 - ((y - my) / den - (rho (x - mx)) / cxx)) t'.
 *      local mean  the FOLD over the patches in index order j gx + i of (term, counted ? 1 : 0); mean = sum / count, 0 if none.
 *      gradient    dL_ddepth_i = (float)(w_global g_image + (w_local g_patch) / count), each g 0 where it does not apply.
 *      parts       [L, 1 - rho_image, local mean, n_used, patches counted, rho_image, a, b], L = w_global term + w_local mean;
 *                  a = cxy / cyy, b = mx - a my: the least-squares fit D ~ a P + b (x ~ a P + b in disparity mode); an image
 *                  that is skipped reports rho_image = a = b = 0.
 *    Two launches for all views of the call (sums with the folds done by the last workgroup of a view to arrive; gradient), no
 *    host read, no allocation, no floating-point atomic.  `workspace`: b3gs_depth_prior_workspace_bytes(W, H, patch) bytes (0
 *    for bad sizes), 256-byte aligned, ZERO before its first use; a call leaves it ready for the next one (the arrival counter
 *    at its head resets itself).  1 <= n_views <= 8, 1 <= W, H and W H <= 2^24, patch 0 (no local term; w_local is then taken
 *    as 0) or 8 .. 256, min_valid >= 2; anything else is B3GS_ERR_ARG before the first HIP call.
 * 2. b3gs_resize_depth_batch: a prior of any size -> the training size, float32.  Per output pixel (x, y), in float32:
 *      sx = fma(x + 0.5, (float)Wsrc / (float)W, -0.5), x0 = floor(sx), fx = sx - x0; the same for y;
 *      w00 = (1 - fx)(1 - fy), w01 = fx (1 - fy), w10 = (1 - fx) fy, w11 = fx fy  (first index: row);
 *      taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), clamped into the source;
 *      v = fma(w11, p11, fma(w10, p10, fma(w01, p01, w00 p00))), a tap of weight 0 entering as 0.
 *    A source pixel is valid iff it is finite and > 0 (and, with src_mask, its mask byte != 0); an output pixel is valid iff
 *    every tap of non-zero weight is: then prior = v, mask = 1, else prior = 0, mask = 0.  Equal sizes copy the valid pixels
 *    bit for bit.  One launch for all views. */
#define B3GS_DEPTH_PRIOR_DEPTH 0
#define B3GS_DEPTH_PRIOR_DISPARITY 1
#define B3GS_DEPTH_PRIOR_MAX_VIEWS 8
typedef struct B3gsDepthPriorIO {
  int32_t W, H;
  const float* depth;          /* [H, W] rendered depth */
  const float* alpha;          /* [H, W] rendered alpha */
  const float* prior;          /* [H, W] */
  const uint8_t* mask;         /* [H, W] validity of the prior */
  int32_t mode;                /* B3GS_DEPTH_PRIOR_DEPTH / _DISPARITY */
  int32_t patch;               /* 0, or 8 .. 256 */
  int32_t min_valid;           /* >= 2 */
  float alpha_min;
  double w_global, w_local;
  const int32_t* offset_dev;   /* NULL, or 2 words on the device: (ox, oy) */
  float* dL_ddepth;            /* [H, W], every word written */
  double* parts;               /* [8] on the device */
  void* workspace;
} B3gsDepthPriorIO;
typedef struct B3gsDepthResizeIO {
  int32_t Wsrc, Hsrc, W, H;
  const float* src;            /* [Hsrc, Wsrc] */
  const uint8_t* src_mask;     /* NULL, or [Hsrc, Wsrc] */
  float* prior;                /* [H, W] */
  uint8_t* mask;               /* [H, W] */
} B3gsDepthResizeIO;
size_t b3gs_depth_prior_workspace_bytes(int32_t W, int32_t H, int32_t patch);
int b3gs_depth_prior_loss_batch(int32_t n_views, const B3gsDepthPriorIO* io, b3gs_stream_t stream);
int b3gs_resize_depth_batch(int32_t n_views, const B3gsDepthResizeIO* io, b3gs_stream_t stream);

/* ---- per-image exposure compensation (added to ABI 18; csrc/exposure.hip, binocular3dgs_amd/exposure.py, INTEGRATION.md
 * section 31) --------------------------------------------------------------------------------------------------------------
 * Five entry points ADDED to ABI 18: no existing declaration, struct or meaning changes, so the number stays.
 * tests/exposure_ref.py restates every rule below in numpy float64.
 *
 * The transform of an image x = (r, g, b) [3, H, W] by a matrix A [3, 4] (12 floats, row-major; row c = [a_c0 a_c1 a_c2 t_c]):
 *      out_c = t_c + a_c0 r + a_c1 g + a_c2 b,  c = 0, 1, 2;  no clamp;  the identity is [I | 0].
 * All arithmetic is fp64, only + - * / sqrt, every statement one rounded operation in the order written; a float32 result is
 * rounded once.  A plane names its matrix as 12 floats (row_dev NULL), or as a table [V, 12] and a device word *row_dev: the
 * kernels read the word (clamped to [0, V - 1]), so a captured launch follows it.
 * The TREE of 256 values, and the FOLD of partials, are those of the depth-prior section above: the xor butterfly per group of
 * 64 and (g0 + g1) + (g2 + g3); s[l] = the partials l, l + 64, .. added in that order to +0, then the butterfly of s[0..63].
 * Block b of a plane holds pixels 256 b .. 256 b + 255 (row-major); a pixel outside the image, or not used, enters as +0.
 *
 * 1. b3gs_exposure_apply: out_c = (float)(((t_c + a_c0 r) + a_c1 g) + a_c2 b).  One launch for up to 8 planes of any sizes.
 *    `g_out`, `G` and `workspace` are not read.
 * 2. b3gs_exposure_backward: `out` receives g_in_k = (float)((A[0][k] g0 + A[1][k] g1) + A[2][k] g2), g = g_out; and
 *      G[c][k] = sum over the pixels of g_c x_k (k < 3),  G[c][3] = sum of g_c
 *    as the TREE per block and the FOLD of a plane's partials.  Planes SHARE a matrix when they name the same `A` and the same
 *    `row_dev`; they must then name the same `G`, and get ONE combined G: the folds of the planes added in plane order to +0
 *    (a trainer's input view and its shifted partner are such a pair: their sum is never formed in float32).  `G`: 12 doubles
 *    followed by their 12 float32 roundings (144 bytes), written by the last workgroup of the group to arrive.  One launch.
 * 3. b3gs_exposure_fit: per plane, over the pixels with mask != 0 (all when mask is NULL), with x = (r, g, b, 1) of the
 *    render and y = the ground truth,
 *      S = sum x x^T  (its 10 unique entries in the order rr rg rb r gg gb g bb b n),  B[c][i] = sum x_i y_c,
 *    TREE and FOLD as above; `sums` = [n, the 10 of S, the 12 of B] (23 doubles; n is S's last entry).  Then S a_c = B[c]:
 *      for j = 0..3:  d = S[j][j] - L[j][0]^2 - .. - L[j][j-1]^2 (left to right);  L[j][j] = sqrt(d);
 *                     for i > j:  L[i][j] = (S[i][j] - L[i][0] L[j][0] - .. - L[i][j-1] L[j][j-1]) / L[j][j]
 *      y_i = (B[c][i] - L[i][0] y_0 - .. ) / L[i][i], i = 0..3;   a_i = (y_i - L[i+1][i] a_{i+1} - .. - L[3][i] a_3) / L[i][i], i = 3..0
 *    and A[c] = (float)(a_0, a_1, a_2, a_3).  DEGENERATE: n < 16, or a pivot d that is not > 2^-40 trace(S), trace =
 *    ((rr + gg) + bb) + n: then A is the identity and *flag = 1; otherwise *flag = 0.  One launch, no host read.
 * 4. b3gs_exposure_adam: Adam on ONE row of the table, row = *row_dev (outside [0, V): nothing happens), one launch of 12
 *    lanes.  prods [V, 2] holds the running products beta1^t, beta2^t of every row (1 before its first step), steps [V] its t:
 *      p1 = prods[row][0] beta1, p2 = prods[row][1] beta2 (stored back), steps[row] += 1,
 *      m = beta1 m + (1 - beta1) g,  v = beta2 v + ((1 - beta2) g) g  (stored as float32),
 *      x = (float)(x - (lr (m / (1 - p1))) / (sqrt(v) / sqrt(1 - p2) + eps))
 *    with g = grad[k] (12 doubles: a G), lr = *lr_dev, m and v the unrounded values.  Only the named row moves: the rows of
 *    views that were not drawn do not drift on their momentum.  While *skip_if_nonzero != 0 (NULL: never) the launch returns
 *    at once -- the sticky capacity word that b3gs_adam_step obeys.
 * `workspace`: b3gs_exposure_workspace_bytes(W, H) bytes (0 for sizes that are refused: 1 <= W, H and W H <= 2^24), 256-byte
 * aligned, one per plane, ZERO before its first use; a call leaves it ready for the next one (the arrival counters at its head
 * reset themselves).  Bad arguments are B3GS_ERR_ARG before the first HIP call. */
#define B3GS_EXPOSURE_MAX_PLANES 8
typedef struct B3gsExposurePlane {
  int32_t W, H;
  const float* in;             /* [3, H, W] */
  const float* g_out;          /* backward: [3, H, W] */
  float* out;                  /* apply: the transformed image; backward: g_in; [3, H, W], every word written */
  const float* A;              /* 12 floats, or the table [V, 12] when row_dev is given */
  const int32_t* row_dev;      /* NULL, or one word on the device */
  int32_t V;                   /* rows of the table */
  double* G;                   /* backward: 12 doubles + 12 floats on the device */
  void* workspace;             /* backward */
} B3gsExposurePlane;
typedef struct B3gsExposureFitIO {
  int32_t W, H;
  const float* render;         /* [3, H, W] */
  const float* gt;             /* [3, H, W] */
  const uint8_t* mask;         /* NULL, or [H, W] */
  float* A;                    /* [12] on the device */
  double* sums;                /* [23] on the device */
  int32_t* flag;               /* one word on the device */
  void* workspace;
} B3gsExposureFitIO;
size_t b3gs_exposure_workspace_bytes(int32_t W, int32_t H);
int b3gs_exposure_apply(int32_t n_planes, const B3gsExposurePlane* io, b3gs_stream_t stream);
int b3gs_exposure_backward(int32_t n_planes, const B3gsExposurePlane* io, b3gs_stream_t stream);
int b3gs_exposure_fit(int32_t n_planes, const B3gsExposureFitIO* io, b3gs_stream_t stream);
int b3gs_exposure_adam(int32_t V, float* table, float* exp_avg, float* exp_avg_sq, int32_t* steps, double* prods,
                       const int32_t* row_dev, const double* grad, const float* lr_dev, double beta1, double beta2, double eps,
                       const int32_t* skip_if_nonzero, b3gs_stream_t stream);

/* ---- normal priors: depth-derived normals and their loss (added to ABI 18; csrc/normalprior.hip,
 * binocular3dgs_amd/normal_prior.py) -------------------------------------------------------------
 * Four entry points ADDED to ABI 18: no existing declaration, struct or meaning changes, so the number stays.
 * tests/normal_prior_ref.py restates every rule below in numpy float64.
 *
 * All arithmetic is fp64, only + - * / sqrt (and |.|, which is exact), every statement one rounded operation in the order
 * written, no fma.  Inputs are float32 planes; every output plane is rounded to float32 once.
 * 1. The depth-derived normal of pixel (x, y), axes x right, y down, z forward, centred pinhole:
 *      usable   u(x, y) iff alpha >= alpha_min (compared in float32; alpha_min > 0)
 *      z        = depth / alpha                      (the render is not normalised)
 *      ray      rx = ((2 (x + 0.5)) / W - 1) tanfovx,  ry = ((2 (y + 0.5)) / H - 1) tanfovy,  rz = 1
 *      point    p = (z rx, z ry, z)
 *      tangents tx = p(x + 1, y) - p(x - 1, y),  ty = p(x, y + 1) - p(x, y - 1)      (1 <= x <= W - 2, 1 <= y <= H - 2)
 *      c        = cross(ty, tx) = (ty_y tx_z - ty_z tx_y,  ty_z tx_x - ty_x tx_z,  ty_x tx_y - ty_y tx_x)
 *                 (a fronto-parallel surface: c points at the camera, c_z < 0)
 *      cc = (c_x c_x + c_y c_y) + c_z c_z,  s = sqrt(cc),  n = c / s
 *      valid    v(x, y) iff the pixel is interior, u holds at it and at its four axis neighbours, cc > 0 and cc < +inf, and the
 *               target's mask byte is non-zero (no mask: every byte counts as 1).  Elsewhere n = 0 and valid = 0.
 * 2. b3gs_normal_prior_loss_batch: against a unit target plane t (float32 [3, H, W], camera frame), with N = #valid
 *      per valid pixel   dot = (n_x t_x + n_y t_y) + n_z t_z,  a = 1 - dot,  b = (|n_x - t_x| + |n_y - t_y|) + |n_z - t_z|
 *      block sums        block k holds pixels 256 k .. 256 k + 255 (row-major); its three sums (count, a, b; 0 for a pixel that
 *                        is not valid) are the TREE of section "depth priors"; the image sums are the FOLD of the block sums.
 *      parts             cos_term = S_a / N, l1_term = S_b / N, L = w_cos cos_term + w_l1 l1_term;
 *                        parts = [L, cos_term, l1_term, N, 1 - cos_term (the mean n.t), 0]; N == 0: all six are 0.
 *      adjoint of n      h_k = w_l1 sgn(n_k - t_k) - w_cos t_k  (sgn(0) = 0); UNSCALED: 1 / N enters last
 *      through n = c/s   d = (n_x h_x + n_y h_y) + n_z h_z,  e_k = (h_k - n_k d) / s
 *      tangent adjoints  g_ty = cross(tx, e),  g_tx = cross(e, ty)  (the component order of c above); 0 where not valid
 *      gather, pixel q   g_p(q) = ((g_tx(x - 1, y) - g_tx(x + 1, y)) + g_ty(x, y - 1)) - g_ty(x, y + 1) per component, a term whose
 *                        centre lies outside the image entering as 0
 *      g_z = ((g_p_x rx + g_p_y ry) + g_p_z) (1 / N)           (1 / N read from device memory; 0 when N == 0)
 *      dL_ddepth = (float)(g_z / alpha),  dL_dalpha = (float)((0 - g_z z) / alpha);  both 0 where u(q) does not hold
 *    Two launches for all views of the call: (1) thread = pixel: n, validity, the block sums, the tangent adjoints into the
 *    workspace (48 bytes per pixel), the FOLD by the last workgroup of a view to arrive, which also writes parts and 1 / N and
 *    resets the arrival counter; (2) the gather.  No host read, no allocation, no floating-point atomic.  `normals` / `valid`:
 *    NULL, or planes that receive n and v.  `mask` may be NULL.  `workspace`: b3gs_normal_prior_workspace_bytes(W, H) bytes (0
 *    for sizes outside 1 <= W, H, W H <= 2^24), 256-byte aligned, ZERO before its first use; a call leaves it ready for the
 *    next.  Its float64 words: [0] the counter, [8] 1 / N, [32 + 3 k ..] the sums of block k.
 * 3. b3gs_depth_normals_batch: rule 1 alone, one launch.
 * 4. b3gs_resize_normals_batch: a prior [3, Hsrc, Wsrc] of any size -> the training size.  Taps, weights and the float32 fma
 *    chain per component are those of b3gs_resize_depth_batch.  A source pixel is good iff its three components are finite (and,
 *    with src_mask, its byte != 0).  In fp64 from the three float32 results: l = (v_x v_x + v_y v_y) + v_z v_z; the output pixel
 *    is valid iff every tap of non-zero weight is good and l >= 1/4: then n = (float)(v / sqrt(l)), mask = 1; else n = 0, mask = 0.
 * Every entry point checks its arguments before the first HIP call: B3GS_ERR_ARG with a message for NULL pointers, n_views
 * outside 1 .. 8, bad sizes, alpha_min <= 0 or NaN, NaN weights, tanfov <= 0 or NaN, a misaligned workspace. */
#define B3GS_NORMAL_PRIOR_MAX_VIEWS 8
typedef struct B3gsNormalPriorIO {
  int32_t W, H;
  const float* depth;          /* [H, W] rendered depth */
  const float* alpha;          /* [H, W] rendered alpha */
  const float* target;         /* [3, H, W] unit normals, camera frame */
  const uint8_t* mask;         /* NULL, or [H, W] validity of the target */
  float alpha_min;             /* > 0 */
  double tanfovx, tanfovy;     /* > 0 */
  double w_cos, w_l1;
  float* dL_ddepth;            /* [H, W], every word written */
  float* dL_dalpha;            /* [H, W], every word written */
  float* normals;              /* NULL, or [3, H, W] */
  uint8_t* valid;              /* NULL, or [H, W] */
  double* parts;               /* [6] on the device */
  void* workspace;
} B3gsNormalPriorIO;
typedef struct B3gsDepthNormalsIO {
  int32_t W, H;
  const float* depth;          /* [H, W] */
  const float* alpha;          /* [H, W] */
  const uint8_t* mask;         /* NULL, or [H, W] */
  float alpha_min;
  double tanfovx, tanfovy;
  float* normals;              /* [3, H, W] */
  uint8_t* valid;              /* [H, W] */
} B3gsDepthNormalsIO;
typedef struct B3gsNormalResizeIO {
  int32_t Wsrc, Hsrc, W, H;
  const float* src;            /* [3, Hsrc, Wsrc] */
  const uint8_t* src_mask;     /* NULL, or [Hsrc, Wsrc] */
  float* normals;              /* [3, H, W] */
  uint8_t* mask;               /* [H, W] */
} B3gsNormalResizeIO;
size_t b3gs_normal_prior_workspace_bytes(int32_t W, int32_t H);
int b3gs_normal_prior_loss_batch(int32_t n_views, const B3gsNormalPriorIO* io, b3gs_stream_t stream);
int b3gs_depth_normals_batch(int32_t n_views, const B3gsDepthNormalsIO* io, b3gs_stream_t stream);
int b3gs_resize_normals_batch(int32_t n_views, const B3gsNormalResizeIO* io, b3gs_stream_t stream);

/* ---- scale initialisation -------------------------------------------------------------
 * mean_dist2[i] = mean squared distance from point i to its 3 nearest OTHER points: the distCUDA2 of the
 * reference's simple-knn extension (scene/gaussian_model.py:134: scales = log(sqrt(max(dist2, 1e-7)))).
 * Exact; points [P,3] and mean_dist2 [P] on the device; workspace = b3gs_knn_workspace_bytes(P) bytes. */
size_t b3gs_knn_workspace_bytes(int32_t P);
int b3gs_knn_mean_dist2(int32_t P, const float* points, float* mean_dist2, char* workspace, b3gs_stream_t stream);

/* Frustum test only: present[i] = 1 if Gaussian i passes the near-plane cull (view z > 0.2). */
int b3gs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                      uint8_t* present, b3gs_stream_t stream);

/* Read-only views into the opaque buffers, for parity tests (tile/bin indices must be
 * bit-exact with the oracle).  Pointers are device pointers inside the caller's buffers. */
typedef struct B3gsDebugViews {
  const uint32_t* tiles_touched; /* [P] */
  const float* depths;           /* [P] */
  const float* records;          /* [P,16] x,y,cxx,cxy,cyy,opacity,r,g,b,depth,ext_x,ext_y, 4 pad (zero: written so that a slot is one unmasked 64-byte store) */
  const uint32_t* point_list;    /* [N] one word per instance, tile-major, depth-sorted: the Gaussian index, or
                                  *     (tile << packed_idx_bits) | index when packed_idx_bits >= 0 */
  const uint32_t* tile_ids;      /* [N] tile id per sorted instance; NULL when the words are packed */
  const uint32_t* ranges;        /* [tiles,2] begin, end; an EMPTY tile holds (0xFFFFFFFF, 0) */
  const float* final_T;          /* [H*W] */
  const uint32_t* n_contrib;     /* [H*W] */
  int32_t packed_idx_bits;       /* >= 0 whenever bits(P) + bits(tiles) <= 32 (e.g. <= 2M Gaussians at 800x600) */
  const uint32_t* counts;        /* [3] N1 (segment 1 / the only segment), V, N2 (segment 2 of a two-round forward, else stale) */
  const uint32_t* point_list2;   /* segment 2 of the tile lists: N2 entries starting at element counts[0] (= N1) of this array (it is
                                  * point_list: segment 2 sits behind segment 1); tile ids likewise at tile_ids + N1 */
  const uint32_t* ranges2;       /* [tiles,2] segment 2 ranges; EMPTY = (0xFFFFFFFF, 0) */
} B3gsDebugViews;
int b3gs_debug_views(int32_t P, int32_t W, int32_t H, int64_t num_rendered, const char* geometry,
                     const char* binning, const char* image, B3gsDebugViews* out);

/* Parity hook (ABI 9): the accessors of scene/gaussian_model.py:95-115 exactly as the raw-parameter kernels evaluate them
 * -- exp(_scaling) [P,3], F.normalize(_rotation) [P,4], sigmoid(_opacity) [P] -- so that a test can hold them against the
 * torch operators bit for bit (integer radii on the raw-parameter path depend on it). */
int b3gs_debug_activations(int32_t P, const B3gsRawParams* raw, float* scales, float* rotations, float* opacity,
                           b3gs_stream_t stream);

/* Per-stage timing hook (thread-local): when non-NULL, b3gs_forward/backward record HIP events
 * around every stage on `stream` WITHOUT synchronising.  After the caller has synchronised the
 * stream, b3gs_timing_collect() adds the elapsed milliseconds of every parked stage to the sink
 * and returns the number of stages resolved (at most 4096 may be parked).  Used by bench.py for
 * the roofline figure; never set in production. */
typedef struct B3gsKernelTimes {
  double preprocess_ms, sort_ms, render_fwd_ms, render_bwd_ms, preprocess_bwd_ms;
  int64_t calls;
} B3gsKernelTimes;
void b3gs_set_timing(B3gsKernelTimes* sink);
int b3gs_timing_collect(void);

const char* b3gs_last_error(void); /* thread-local message of the last failure */
int b3gs_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* B3GS_RASTER_H */
