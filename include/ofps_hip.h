/*
 * ofps_hip.h -- C ABI of libofps_hip.so, the MI355X (gfx950) backend for the OFPS flow hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  A Rust cdylib
 * shim implements the reference's plugin traits on top of these calls:
 *
 *   ofps_hip_sad_flow*      -> Decoder::process_frame          (ofps/src/decoder.rs:45-73); output
 *                              record convention of av-decoder   (av-decoder/src/lib.rs:404-419)
 *   ofps_hip_densify*       -> MotionFieldDensifier::add_vector + MotionField::from
 *                                                               (ofps/src/motion_field.rs:133-190,297-308)
 *   ofps_hip_densify_to_entries -> cv-decoder's downsample stage (cv-decoder/src/lib.rs:244-291)
 *   ofps_hip_detect*        -> Detector::detect_motion          (ofps/src/detection.rs:11,
 *                                                               block-motion-detector/src/lib.rs:49-118)
 *   ofps_hip_almeida*       -> Estimator::estimate              (ofps/src/estimator.rs:19-24,
 *                                                               almeida-estimator/src/lib.rs:100-251)
 *
 * A MotionEntry is 4 consecutive f32 [pos.x, pos.y, motion.x, motion.y] (decoder.rs:40-42), the
 * same record the reference's .mvec files hold (motion-extract/src/main.rs:23-35).
 *
 * Conventions
 *   - every call returns 0 on success or a negative OFPS_HIP_E* code; ofps_hip_last_error(ctx)
 *     returns a human-readable message for the last failure on that context.
 *   - one context per plugin instance; calls on one context must be serialised by the caller
 *     (plugins are Send, not Sync: ofps/src/plugins/mod.rs:244,261,278); different contexts may
 *     be used concurrently from different host threads.
 *   - the library never frees or retains caller memory; all outputs are caller-allocated.
 *   - "*_dev" entry points take device pointers (hipMalloc'd on the context's device), enqueue
 *     on the context's stream and return without synchronising; host-pointer entry points
 *     copy in/out and synchronise before returning.
 *   - there is no CPU fallback: without a usable gfx950 device ofps_hip_init fails.
 */
#ifndef OFPS_HIP_H
#define OFPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFPS_HIP_API_VERSION 2

enum {
    OFPS_HIP_OK = 0,
    OFPS_HIP_EINVAL = -1,      /* bad argument (message says which) */
    OFPS_HIP_EDEVICE = -2,     /* HIP runtime error / no device */
    OFPS_HIP_EUNSUPPORTED = -3, /* parameter combination has no kernel */
    OFPS_HIP_ENOMEM = -4
};

typedef struct ofps_hip_ctx ofps_hip_ctx;

/* ---- context ---- */
int  ofps_hip_api_version(void);
int  ofps_hip_device_count(void);
int  ofps_hip_init(int device, ofps_hip_ctx** out);
void ofps_hip_destroy(ofps_hip_ctx* ctx);
const char* ofps_hip_last_error(const ofps_hip_ctx* ctx);   /* ctx may be NULL: last init error */
/* Run on a caller-owned hipStream_t (e.g. torch's current stream).  NULL is a valid handle: HIP's
 * default stream.  ofps_hip_use_own_stream() goes back to the stream the context created. */
int   ofps_hip_set_stream(ofps_hip_ctx* ctx, void* hip_stream);
int   ofps_hip_use_own_stream(ofps_hip_ctx* ctx);
void* ofps_hip_get_stream(ofps_hip_ctx* ctx);
int   ofps_hip_sync(ofps_hip_ctx* ctx);
/* Diagnostic / A-B switches (table in INTEGRATION.md).  `name` is the switch's environment-variable name, e.g.
 * "OFPS_HIP_ALMEIDA_HIER"; value NULL or "" restores the default.  ofps_hip_init reads the same variables from the
 * environment ONCE; no other entry point looks at the environment.  The fault injectors
 * (OFPS_HIP_ALMEIDA_TEST_FAULT, OFPS_HIP_LK_TEST_FALL, OFPS_HIP_LK_TEST_WAIT_BUDGET, OFPS_HIP_LK_TEST_ORDER) exist only in libofps_hip_testhooks.so (built with
 * -DOFPS_HIP_TEST_HOOKS, used by the parity tests), can only be armed through this call, and are refused with
 * OFPS_HIP_EUNSUPPORTED by the product library. */
int   ofps_hip_set_option(ofps_hip_ctx* ctx, const char* name, const char* value);
int   ofps_hip_has_test_hooks(void);                         /* 1 in libofps_hip_testhooks.so, 0 in libofps_hip.so */

/* ---- device memory plumbing for hosts without their own HIP binding ---- */
int ofps_hip_malloc(ofps_hip_ctx* ctx, size_t bytes, void** dptr);
int ofps_hip_free(ofps_hip_ctx* ctx, void* dptr);
/* page-locked host memory for frame buffers (H2D by DMA, no staging copy); plain malloc'ed buffers work everywhere too */
int ofps_hip_host_alloc(ofps_hip_ctx* ctx, size_t bytes, void** hptr);
int ofps_hip_host_free(ofps_hip_ctx* ctx, void* hptr);
int ofps_hip_memcpy_h2d(ofps_hip_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int ofps_hip_memcpy_d2h(ofps_hip_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);

/* ---- timing helper: HIP events on the context's stream (bench.py roofline leg) ---- */
int ofps_hip_timer_start(ofps_hip_ctx* ctx);
int ofps_hip_timer_stop(ofps_hip_ctx* ctx, float* elapsed_ms);   /* synchronises on the stop event */

/* ---- N1: full-search SAD block matcher ("hip_sad" Decoder) ----
 * Blocks on a block x block lattice from (0,0), full blocks only; candidates (dx,dy) in
 * [-range,range]^2 whose block lies inside the frame; winner = min of
 * (SAD, dx*dx+dy*dy, dy+range, dx+range); entry = (pos = (centre+d)/(W,H), motion = -d/(W,H)).
 * Motion beyond `range`: the search levels, N1h below.
 * Supported: block in {8,16} with range in {8,12,16,20,24,28,32} and 16-byte aligned rows run on the packed-SAD strip
 * kernel (the same geometries with rows only 4-byte aligned: the per-block packed kernel); any other block <= 64,
 * range <= 64 runs on the generic kernel (correctness path, ~30x slower).  stride % 4 == 0. */
size_t ofps_hip_sad_block_count(int W, int H, int block);
/* Search strategy of ofps_hip_sad_flow*: both return the spec's winner bit for bit.
 * EXHAUSTIVE evaluates every candidate (content-independent run time, the default).
 * PRUNED (partial-distortion elimination) computes the SAD over 4 of the 16 block rows for every candidate -- a lower
 * bound of the full SAD -- and evaluates in full only the candidates whose bound does not exceed the exact SAD of the
 * minimum-bound candidate; run time depends on the content (faster on smooth camera motion with little noise, slower
 * where there is nothing to prune); 16x16 blocks, range 16 only -- other geometries ignore the mode. */
enum { OFPS_HIP_SAD_EXHAUSTIVE = 0, OFPS_HIP_SAD_PRUNED = 1 };
int ofps_hip_set_sad_mode(ofps_hip_ctx* ctx, int mode);
/* Diagnostics: how many strips of the last PRUNED call overflowed their survivor lists and were redone by the
 * exhaustive kernel (synchronises the stream). */
int ofps_hip_sad_pruned_overflow_strips(ofps_hip_ctx* ctx, uint32_t* count);
/* ---- N1q: quarter-pel vectors (AVMotionVector.motion_scale = 4, H.264's; av-decoder/src/lib.rs:412-417 divides by it) ----
 * scale 1 (the default): the full-pel vectors above, byte for byte.  scale 4: every ofps_hip_sad_flow* call and every
 * ofps_hip_push_frame* search is followed by a refinement launch around each block's integer winner (dx,dy), unchanged:
 *   candidates D = (4*dx + fx, 4*dy + fy), fx, fy in [-3,3], in quarter-pel units; valid when every sample position of
 *   the block lies inside the frame: 0 <= 4*x0 + Dx and 4*(x0 + B - 1) + Dx <= 4*(W - 1), the same in y (f = 0 always is);
 *   cost = sum |cur - ref_q| over the block, ref_q = the previous frame at quarter-pel positions by H.264's luma
 *   interpolation (ITU-T H.264 8.4.2.2.1), taps outside the frame edge-replicated:
 *     half-pel in one direction: b1 = E - 5F + 20G + 20H - 5I + J over the six nearest integer samples of the row (the
 *       column for h1), b = clip255((b1 + 16) >> 5); half-pel in both: j1 = the same taps over the unrounded b1 of six
 *       rows, j = clip255((j1 + 512) >> 10);
 *     quarter-pel: (p + q + 1) >> 1 of two samples of the half-pel grid (integer samples included): fx odd, fy even: the
 *       left and right neighbours; fx even, fy odd: the upper and lower; both odd: of the four surrounding half-grid
 *       points the two that are half-pel in exactly one direction (H.264's e, g, p, r);
 *   winner = min of (SAD, Dx*Dx + Dy*Dy, Dy + 4*range + 3, Dx + 4*range + 3), lexicographic (a flat block keeps D = 4*d);
 *   entry: pos.x = ((float)(4*cx + Dx) * 0.25f) * nx, motion.x = ((float)Dx / 4.0f) * (-nx), cx = x0 + B/2,
 *   nx = 1.0f / (float)W; y alike.  out_best holds (Dx, Dy, SAD) in quarter-pel units while the scale is 4.
 * Build-defined like N1 (no encoder's search is anybody's contract: parity with FFmpeg's vectors is unpinned by
 * construction); all-integer, bit-exact against the NumPy restatement tests/indep_sad_qpel.py.  Any scale other than
 * 1 or 4 is OFPS_HIP_EINVAL.  The option OFPS_HIP_SAD_MOTION_SCALE (environment / ofps_hip_set_option) sets the same field. */
int ofps_hip_set_sad_motion_scale(ofps_hip_ctx* ctx, int scale);
int ofps_hip_get_sad_motion_scale(ofps_hip_ctx* ctx);
int ofps_hip_sad_flow(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur,
                      int W, int H, int stride, int block, int range,
                      float* out_entries /* 4*nblk */, int32_t* out_best /* 3*nblk (dx,dy,sad); with motion scale 4: (Dx,Dy,SAD) in quarter-pel units; or NULL */,
                      size_t* n_out);
/* Batched, device-resident: n_frames luma frames at d_frames + k*frame_pitch (bytes).
 * ref_mode 0: pairs (k, k+1); ref_mode 1: pairs (0, k+1) (shared key frame).  n_frames-1 pairs.
 * d_out_entries: [(n_frames-1) * nblk * 4] f32; d_out_best: [(n_frames-1) * nblk * 3] i32 or NULL. */
int ofps_hip_sad_flow_dev(ofps_hip_ctx* ctx, const void* d_frames, int n_frames,
                          int W, int H, int stride, size_t frame_pitch, int ref_mode,
                          int block, int range, void* d_out_entries, void* d_out_best);

/* ---- N1g: hip_sad's contrast gate -- a block that tells nothing yields no record (csrc/sad_gate.hip) ----
 * av-decoder, whose record convention hip_sad copies, yields a vector only for the blocks the encoder chose to predict
 * (av-decoder/src/lib.rs:396-419); the dense decoders drop the pixels outside cv-decoder's contrast mask.  The gate is hip_sad's form of
 * both.  Build-defined, like N1 and N1q.  The contrast gate of a frame pair (prev, cur) with lattice `block` = B:
 *   M = cv-decoder's contrast mask of the CURRENT frame's luma: exactly what ofps_hip_contrast_mask(cur) returns;
 *   count(bx, by) = the number of set pixels of M inside [bx*B, bx*B + B) x [by*B, by*B + B).  Only full lattice blocks are counted, as in
 *     ofps_hip_sad_block_count; mask pixels in the ragged right / bottom margin belong to no block;
 *   a block is KEPT iff count >= min_pixels, min_pixels in [1, B*B];
 *   the kept blocks' records keep raster order (block row outer, block column inner): the ungated order with the dropped ones removed.
 *     The records themselves are the ungated ones bit for bit, quarter-pel refined or not; out_best triples are compacted the same way.
 * Gate value 0 = off, the default: every entry point then uses the launches, streams and bytes of a build without the gate.  A negative
 * value is OFPS_HIP_EINVAL at the setter; a value > B*B for the block size of a call is OFPS_HIP_EINVAL at that call.  The option
 * OFPS_HIP_SAD_GATE (environment / ofps_hip_set_option) sets the same field.
 * ofps_hip_block_contrast[_dev]: the counts alone, uint32 per block in raster order, any block <= 64, any stride >= W; they equal the
 *   per-block sums of ofps_hip_contrast_mask's output (the kernel runs the mask's arithmetic and never writes the pixel mask).
 * With the gate on:
 *   ofps_hip_sad_flow: *n_out = the kept count; out_entries / out_best hold the kept records first (capacity nblk, as without the gate;
 *     what lies behind the kept ones is unspecified).
 *   ofps_hip_push_frame[_async] / ofps_hip_frame_wait: the count stays on the device -- the keep flags are made beside the search on a
 *     second stream, one compaction launch behind it, and estimator, compensation (mode 1) and detector read the count from device memory
 *     (launches sized from the capacity nblk).  n_vectors = the kept count; have_vectors stays 1 for every frame that ran a search, also
 *     with 0 kept (Ok(true) with an empty list: av-decoder on an all-intra frame); out_entries receives the kept records first.  The
 *     detector's result equals ofps_hip_detect on the kept records bit for bit, the quaternion ofps_hip_almeida's to the solver's parity
 *     bound (2e-6, as for the dense decoders' fused form below).  Fewer than 3 kept records -> identity, with either solver (the
 *     reference's rule for RANSAC inliers, almeida-estimator/src/lib.rs:246-250); none kept -> no motion.  A ticket follows the gate the
 *     context has when it is pushed.
 * ofps_hip_sad_flow_gated_dev: one pair of device frames with an explicit min_pixels in [1, B*B] (the context's gate is not looked at);
 *   d_out_entries / d_out_best have capacity nblk, d_out_count is one uint32 in device memory; enqueues only.
 * The batched forms: ofps_hip_sad_flow_dev and ofps_hip_multi_sad_flow / _run_resident / _fetch ignore the gate and always produce nblk
 * records per pair; ofps_hip_push_frames_async and the ofps_hip_multi_* workers' pushes do so unless the batch filter switch is on (N1b
 * below, which also holds the filtered sibling of ofps_hip_sad_flow_dev).  Out of scope: a second criterion on the SAD surface
 * (best against second best) is not part of this (the forward-backward check, N1c below, is the second criterion this build has). */
int ofps_hip_block_contrast(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride, int block, uint32_t* out_counts /* nblk */);
int ofps_hip_block_contrast_dev(ofps_hip_ctx* ctx, const void* d_luma, int W, int H, int stride, int block, void* d_out_counts);
int ofps_hip_set_sad_gate(ofps_hip_ctx* ctx, int min_pixels);   /* 0 = off (default) */
int ofps_hip_get_sad_gate(ofps_hip_ctx* ctx);
int ofps_hip_sad_flow_gated_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block, int range,
                                int min_pixels, void* d_out_entries, void* d_out_best /* or NULL */, void* d_out_count /* one uint32 */);

/* ---- N1c: hip_sad's forward-backward consistency check -- a winner that does not come back yields no record (csrc/sad_consistency.hip) ----
 * The round-trip test of flow and stereo pipelines: search forward, search backward, drop what does not return.  It drops what the contrast
 * gate keeps: blocks whose content left the frame or was occluded, repeated texture, noise that trips the mask's threshold, the block column
 * the mask's dilation carries across a texture edge.  Build-defined, like N1, N1q and N1g.  For a frame pair (prev, cur), lattice `block`
 * = B, nbx = W / B, nby = H / B:
 *   F[k] = (dx, dy): the forward winner of block k -- what ofps_hip_sad_flow(prev, cur) reports in out_best at motion scale 1: the block of
 *     cur at (x0, y0) matched prev at (x0 + dx, y0 + dy);
 *   G[k'] = (ex, ey): the winner of the same search with the frames exchanged, sad(prev := cur, cur := prev), same block and range;
 *   the partner of block k = (bx, by): cx = bx*B + B/2 + dx, cy = by*B + B/2 + dy (the integer numerators of the record's pos; never
 *     negative: the matched block lies inside the frame); bx' = min(cx / B, nbx - 1), by' = min(cy / B, nby - 1), integer division (the
 *     clamp catches centres in the ragged right / bottom margin); k' = by'*nbx + bx';
 *   residual(k) = max(|dx + ex|, |dy + ey|) with (ex, ey) = G[k']: an integer in [0, 2*range];
 *   a block is KEPT iff residual < limit, limit in [1, 129]: 1 = an exact round trip.  A limit above 2*range + 1 is valid and keeps every block.
 *   The check always uses the INTEGER winners of both directions: at motion scale 4 the backward search is never refined and the forward
 *     refinement is unchanged.
 *   Kept records and out_best triples keep raster order and are the unchecked call's records and triples bit for bit, quarter-pel or not.
 *   With the contrast gate (N1g) on as well a block is kept iff both criteria keep it: one compaction, one count.
 * Limit 0 = off, the default: every entry point then uses the launches, streams and bytes of a build without the check.  Negative values and
 * values above 129 are OFPS_HIP_EINVAL at the setter.  The option OFPS_HIP_SAD_CONSISTENCY (environment / ofps_hip_set_option) sets the
 * same field.
 * The check says nothing about a clean flat block: both directions return 0 and the round trip is exact -- that is the contrast gate's job.
 * ofps_hip_sad_consistency[_dev]: residuals and / or keep bytes from two arrays of (dx, dy, sad) triples in integer units (only dx and dy are
 *   read), limit in [1, 129]; either output may be NULL.  The triples are the caller's responsibility: |d| above 64 gives an unspecified
 *   flag, never an access out of bounds (k' is clamped on both sides).  The _dev form enqueues only.
 * With the context's limit > 0:
 *   ofps_hip_sad_flow: *n_out = the kept count, the kept records first (capacity nblk, as for the gate); the contrast gate is applied as well
 *     when it is on.
 *   ofps_hip_push_frame[_async] / ofps_hip_frame_wait: the gate's path with one more producer of keep flags -- the backward search runs on the
 *     two resident frames right behind the forward one on the compute stream, then (behind the join with the contrast flags, if any) the
 *     check, ONE compaction and the count in device memory; estimator, compensation (mode 1) and detector in their device-count forms.
 *     n_vectors = the kept count; have_vectors stays 1 for every frame that ran a search; fewer than 3 kept -> identity, none -> no motion,
 *     as N1g documents them.  A ticket follows the limit the context has when it is pushed.
 * ofps_hip_sad_flow_checked_dev: one pair of device frames with an explicit min_pixels (0 = no contrast gate, else [1, B*B]) and limit in
 *   [1, 129] (the context's values are not looked at); capacities and count as ofps_hip_sad_flow_gated_dev; enqueues only.
 * In PRUNED mode ofps_hip_sad_pruned_overflow_strips then reports the backward search, the last one of the call.
 * The batched forms, as for N1g: ofps_hip_sad_flow_dev and ofps_hip_multi_sad_flow / _run_resident / _fetch ignore the limit and always
 * produce nblk records per pair; ofps_hip_push_frames_async and the ofps_hip_multi_* workers' pushes follow it with the batch filter
 * switch on (N1b below). */
int ofps_hip_sad_consistency(ofps_hip_ctx* ctx, const int32_t* fwd_best, const int32_t* bwd_best, int W, int H, int block, int limit,
                             uint32_t* out_residual /* nblk or NULL */, uint8_t* out_keep /* nblk or NULL */);
int ofps_hip_sad_consistency_dev(ofps_hip_ctx* ctx, const void* d_fwd_best, const void* d_bwd_best, int W, int H, int block, int limit,
                                 void* d_out_residual /* or NULL */, void* d_out_keep /* or NULL */);
int ofps_hip_set_sad_consistency(ofps_hip_ctx* ctx, int limit);   /* 0 = off (default) */
int ofps_hip_get_sad_consistency(ofps_hip_ctx* ctx);
int ofps_hip_sad_flow_checked_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block, int range,
                                  int min_pixels /* 0 = no contrast gate */, int limit /* >= 1 */, void* d_out_entries,
                                  void* d_out_best /* or NULL */, void* d_out_count /* one uint32 */);

/* ---- N1v: hip_sad's median test -- a winner that disagrees with its neighbours yields no record (csrc/sad_median.hip) ----
 * The median test of vector-field post-processing (the outlier test of PIV and of every encoder's vector smoothing): a vector is compared
 * with the median of its neighbours' and dropped when it lies far from it.  It drops what gate (N1g) and check (N1c) keep: a clean, textured,
 * round-trip-consistent match at the wrong place -- repeated texture on which both directions lock onto the same alias, a block clipped by
 * the frame edge, the ring of blocks the mask's dilation carries across a texture edge.  Build-defined, like N1g and N1c; all-integer, so
 * bit-exact on every device.  For a frame pair, lattice `block` = B, nbx = W / B, nby = H / B:
 *   F[k] = (dx, dy): the INTEGER forward winner of block k, as N1c uses it: at motion scale 4 the winner in front of the quarter-pel
 *     refinement, with search levels (N1h) the level-0 winner;
 *   keep_in[k]: what the other criteria say: contrast gate AND consistency check, whichever are on; neither on: all ones;
 *   N(k) for k = (bx, by): the blocks (bx + i, by + j), i, j in {-1, 0, 1}, not both 0, that lie inside the lattice and have keep_in = 1;
 *     n = |N(k)|;
 *   per component c in {x, y}: the neighbours' d_c sorted ascending into s[0..n-1]; the doubled median M_c = s[(n-1) >> 1] + s[n >> 1]: twice
 *     the middle value for odd n, the sum of the two middle values for even n -- component-wise and in half-pixels, nothing is ever rounded;
 *   r2(k) = max(|2*dx - M_x|, |2*dy - M_y|) for n >= 1, r2(k) = 0 for n = 0: an integer in half-pixels;
 *   a block is KEPT iff keep_in[k] and r2(k) < 2*limit, limit in [1, 255]: at limit 1 the vector lies less than one pixel from the
 *     neighbours' median.  A block with no kept neighbour is kept: nothing contradicts it.
 *   One pass: every verdict reads the INCOMING flags of its neighbours, never another block's verdict of this test; nothing is iterated.
 *   Kept records and out_best triples keep raster order and are the unfiltered call's records and triples bit for bit, quarter-pel or not.
 * Limit 0 = off, the default: every entry point then uses the launches, streams, scratch and bytes of a build without the test.  Negative
 * values and values above 255 are OFPS_HIP_EINVAL at the setter.  The option OFPS_HIP_SAD_MEDIAN (environment / ofps_hip_set_option) sets
 * the same field.
 * ofps_hip_sad_median[_dev]: the test alone on caller-held (dx, dy, sad) triples in integer units (only dx and dy are read), limit in
 *   [1, 255]; keep_in: one byte per block (non-zero = kept) or NULL = all ones; either output may be NULL; out_residual2 = r2, saturated at
 *   2^32 - 1.  Any |d| gives a defined flag and never an access out of bounds.  The _dev form enqueues only; its d_out_keep may not be
 *   d_keep_in (OFPS_HIP_EINVAL): a verdict reads its neighbours' incoming flags.
 * With the context's limit > 0:
 *   ofps_hip_sad_flow: *n_out = the kept count, the kept records first (capacity nblk, as for the gate); gate and check are applied as well
 *     when they are on.
 *   ofps_hip_push_frame[_async] / ofps_hip_frame_wait: the gate's path with a third producer of keep flags -- on the compute stream, behind
 *     the check's flags (if any): the median flags, read from those and written to an array of their own, then ONE compaction and the count
 *     in device memory; no host synchronisation is added.  n_vectors = the kept count; have_vectors stays 1 for every frame that ran a
 *     search; fewer than 3 kept -> identity, none -> no motion, as N1g documents them.  A ticket follows the limit the context has when it
 *     is pushed.
 * ofps_hip_sad_flow_median_dev: one pair of device frames with explicit values -- min_pixels (0 = no contrast gate, else [1, B*B]), limit
 *   (0 = no consistency check, else [1, 129]), median_limit in [1, 255]; the context's three fields are not looked at; capacities and count as
 *   ofps_hip_sad_flow_checked_dev; enqueues only.
 * The batched forms, as for N1g / N1c: ofps_hip_sad_flow_dev and ofps_hip_multi_sad_flow / _run_resident / _fetch ignore the limit and
 * always produce nblk records per pair; ofps_hip_push_frames_async and the ofps_hip_multi_* workers' pushes follow it with the batch
 * filter switch on (N1b below).  Out of scope: replacing an outlier by the median (it would need a re-scored SAD and a moved record position); a
 * normalised (fluctuation-scaled) threshold; the dense decoders. */
int ofps_hip_sad_median(ofps_hip_ctx* ctx, const int32_t* best, const uint8_t* keep_in /* nblk or NULL = all ones */, int W, int H, int block,
                        int limit, uint32_t* out_residual2 /* nblk or NULL */, uint8_t* out_keep /* nblk or NULL */);
int ofps_hip_sad_median_dev(ofps_hip_ctx* ctx, const void* d_best, const void* d_keep_in /* or NULL */, int W, int H, int block, int limit,
                            void* d_out_residual2 /* or NULL */, void* d_out_keep /* or NULL */);
int ofps_hip_set_sad_median(ofps_hip_ctx* ctx, int limit);   /* 0 = off (default) */
int ofps_hip_get_sad_median(ofps_hip_ctx* ctx);
int ofps_hip_sad_flow_median_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block, int range,
                                 int min_pixels /* 0 = no contrast gate */, int limit /* 0 = no consistency check */, int median_limit /* >= 1 */,
                                 void* d_out_entries, void* d_out_best /* or NULL */, void* d_out_count /* one uint32 */);

/* ---- N1b: gate, check and median test in the batched forms (csrc/sad_gate.hip, csrc/pipeline.hip) ----
 * The three criteria above over a whole batch of pairs, with a number of launches that does not depend on the number of pairs: contrast
 * counts + keep flags, consistency flags, median flags and the compaction are one launch each over the batch (the item in a grid
 * dimension), the compaction segmented -- one workgroup scans one item, one path for every nblk -- with one count per item; neighbour and
 * partner indices never cross an item boundary.
 * ofps_hip_sad_flow_filtered_dev: frames and pairs as ofps_hip_sad_flow_dev, in both ref_modes (ref_mode 1: the current frame of pair k is
 *   frame k + 1 -- the gate reads it, the backward search goes from it to the key frame).  min_pixels (0 = no contrast gate, else [1, B*B]),
 *   limit (0 = no consistency check, else [1, 129]) and median (0 = no median test, else [1, 255]) are explicit, the context's three fields
 *   are not looked at; all three 0 is OFPS_HIP_EINVAL.  Everything else of the context applies as to any search: motion scale 4, search
 *   levels and predictors, mean removal (the gate reads the raw frames), PRUNED.  Item k's slot -- d_out_entries + k*nblk records,
 *   d_out_best + k*nblk triples -- and d_out_counts[k] are bit for bit what ofps_hip_sad_flow_median_dev (_checked_dev / _gated_dev where
 *   the later criteria are 0) returns for that pair with the same three values: the kept records and triples first, in raster order; the
 *   rest of the slot is unspecified, nothing is written outside it.  Enqueues only: no host synchronisation, no read-back.
 * ofps_hip_set_sad_batch_filter: 0 (default) = ofps_hip_push_frames_async and the ofps_hip_multi_* workers' pushes ignore the context's
 *   gate, limit and median limit, as they always have, and enqueue what a build without this section enqueues; 1 = a ticket pushed while at
 *   least one of the three is on runs the filtered batched search and the tail's device-count forms with one count per item:
 *   ofps_hip_frames_wait fills out[j].n_vectors with item j's kept count (it travels in the ticket's page-locked block in the one read-back;
 *   nothing is synchronised between push and wait), have_vectors stays 1 for every frame that ran a search, also with 0 kept, out_entries
 *   holds the kept records first in slot j.  Records and counts of item j equal a single ofps_hip_push_frame of that frame with the same
 *   settings bit for bit, the detector's result likewise, the quaternion to 2e-6; fewer than 3 kept -> identity with either solver, none
 *   kept -> no motion.  A ticket follows the settings the context has when it is pushed.  Detect-compensation mode 1 works where it does
 *   without the switch (not in the multi-device workers).  Any value but 0 / 1 is OFPS_HIP_EINVAL.  The option OFPS_HIP_SAD_BATCH_FILTER
 *   (environment / ofps_hip_set_option) sets the same field; the multi-device workers read it from the environment at their init, as they
 *   read OFPS_HIP_SAD_GATE, so ofps_hip_multi_push_frames_async follows it, n_vectors and records in frame order as ever.
 * Still ignoring all three: ofps_hip_sad_flow_dev (its filtered sibling is the call above), ofps_hip_multi_sad_flow / _run_resident / _fetch. */
int ofps_hip_sad_flow_filtered_dev(ofps_hip_ctx* ctx, const void* d_frames, int n_frames, int W, int H, int stride, size_t frame_pitch,
                                   int ref_mode, int block, int range, int min_pixels, int limit, int median,
                                   void* d_out_entries /* pairs * nblk * 4 f32 */, void* d_out_best /* pairs * nblk * 3 i32, or NULL */,
                                   void* d_out_counts /* pairs uint32 */);
int ofps_hip_set_sad_batch_filter(ofps_hip_ctx* ctx, int on);   /* 0 = the batched forms ignore gate, check and median test (default) */
int ofps_hip_get_sad_batch_filter(ofps_hip_ctx* ctx);

/* ---- N1i: hip_sad's intra test and scene-cut rule -- a block that matches nothing yields no record (csrc/sad_intra.hip) ----
 * A block whose content has no counterpart in the previous frame -- a scene cut, uncovered background, an object that appears, a flash --
 * still has a best match among the search's candidates, and N1 reports it as a normal record.  An encoder's mode decision compares the
 * match's cost with the cost of coding the block from itself; the decoder this build mirrors yields no vector for such a block and none on
 * an intra frame (av-decoder/src/lib.rs:396-419).  Build-defined, like N1g, N1c and N1v; all-integer, so bit-exact on every device.  For a
 * frame pair, lattice `block` = B in [1, 64], nbx = W / B, nby = H / B, full blocks only:
 *   A(k), the activity of block k of the RAW current frame: S = the sum of its n = B*B pixels p, m = (S + n/2) / n (integer division: the
 *     mean rounded half up), A(k) = the sum of |p - m|: a uint32, at most 522,240 (B = 64, half 0 and half 255).  The contrast gate (N1g)
 *     reads the raw frame as well; with mean removal (N1m) on, the SAD below is the filtered frames' and A stays the raw frame's;
 *   SAD(k): the SAD of the INTEGER forward winner of block k, the triple N1c and N1v read: in front of the quarter-pel refinement at
 *     motion scale 4, the level-0 winner with search levels (N1h);
 *   ratio q in [1, 255], in sixteenths: block k is INTRA iff 16 * SAD(k) >= q * A(k), evaluated in 64-bit signed arithmetic whatever the
 *     triple holds.  Equality is intra; a flat block (A = 0, SAD = 0) is intra.  q = 16 is the encoder's literal rule; uncorrelated content
 *     wins at SAD ~ A, so useful values lie below it;
 *   flags: keep(k) = gate(k) AND NOT intra(k), gate(k) the contrast gate's flag (gate off: all ones).  The consistency check ANDs its flag
 *     onto that, the median test reads the result as its incoming flags (gate AND NOT intra AND check).  One compaction, one count;
 *   scene cut, P in [0, 100] percent: n_cand = the number of blocks of the pair with gate(k) = 1, n_intra = the number of those that are
 *     intra (check and median test do not enter).  With P > 0 the pair is a CUT iff 100 * n_intra >= P * n_cand -- so n_cand = 0 is a cut --
 *     and a cut pair yields zero records: n_vectors = 0, have_vectors as before; estimator and detector take their paths for fewer than 3
 *     and for no records (identity, no motion: N1g).  P has no effect while q = 0; setting it then is accepted;
 *   Kept records and out_best triples keep raster order and are the unfiltered call's records and triples bit for bit, quarter-pel or not.
 * q = 0 = off, the default: every entry point then uses the launches, streams, scratch and bytes of a build without the test.  Values
 * outside [0, 255] (q) and [0, 100] (P) are OFPS_HIP_EINVAL at the setters.  The options OFPS_HIP_SAD_INTRA and OFPS_HIP_SAD_CUT
 * (environment / ofps_hip_set_option) set the same fields.
 * ofps_hip_block_activity[_dev]: A alone, uint32 per block in raster order, any block in [1, 64], any stride >= W.  Every pixel is read once;
 *   no address outside the frame is formed: the ragged right and bottom margins belong to no block.  The _dev form enqueues only.
 * ofps_hip_sad_intra[_dev]: verdict and cut alone on caller-held data: (dx, dy, sad) triples (only the SAD is read, as a signed 32-bit
 *   number), activities, keep_in (one byte per block, non-zero = gate(k) = 1, or NULL = all ones), ratio in [1, 255], cut in [0, 100] ->
 *   out_keep (keep(k), all zero for a cut; the _dev form's may be d_keep_in) and, unless NULL, out_counts = [n_cand, n_intra].  The _dev
 *   form enqueues only.
 * With the context's q > 0:
 *   ofps_hip_sad_flow: *n_out = the kept count, the kept records first (capacity nblk, as for the gate); gate, check and median test are
 *     applied as well when they are on.
 *   ofps_hip_push_frame[_async] / ofps_hip_frame_wait: the gate's path with one more producer of keep flags -- the activities of the current
 *     frame are made beside the search on the second stream (with the contrast count, if the gate is on); on the compute stream behind the
 *     search and the join: the verdicts and the pair's two counters, [check, median test,] [the cut rule's veto, one launch, only with
 *     P > 0,] then ONE compaction and the count in device memory; no host synchronisation is added.  n_vectors = the
 *     kept count, 0 for a cut; have_vectors stays 1 for every frame that ran a search.  A ticket follows the values the context has when it
 *     is pushed.
 * ofps_hip_sad_flow_intra_dev: ofps_hip_sad_flow_filtered_dev's shape (frames, pairs, both ref_modes, slots and counts) with two more
 *   explicit values: intra in [1, 255] and cut in [0, 100]; min_pixels, limit and median may all be 0; the context's five fields are not
 *   looked at.  Everything else of the context applies as to any search: motion scale 4, search levels and predictors, mean removal, PRUNED.
 * The batched forms, as for N1g / N1c / N1v: ofps_hip_sad_flow_dev and ofps_hip_multi_sad_flow / _run_resident / _fetch ignore both fields
 * and always produce nblk records per pair, and so do the explicit-argument forms _gated_dev, _checked_dev, _median_dev and _filtered_dev;
 * ofps_hip_push_frames_async and the ofps_hip_multi_* workers' pushes follow them with the batch filter switch on (N1b).  Out of scope:
 * replacing an intra block's vector; an activity on the filtered frame; reporting the cut through ofps_hip_frame_result (its layout is
 * ABI); the dense decoders. */
int ofps_hip_block_activity(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride, int block, uint32_t* out_activity /* nblk */);
int ofps_hip_block_activity_dev(ofps_hip_ctx* ctx, const void* d_luma, int W, int H, int stride, int block, void* d_out_activity);
int ofps_hip_sad_intra(ofps_hip_ctx* ctx, const int32_t* best, const uint32_t* activity, const uint8_t* keep_in /* nblk or NULL = all ones */,
                       int W, int H, int block, int ratio, int cut, uint8_t* out_keep /* nblk */, uint32_t* out_counts /* [n_cand, n_intra] or NULL */);
int ofps_hip_sad_intra_dev(ofps_hip_ctx* ctx, const void* d_best, const void* d_activity, const void* d_keep_in /* or NULL */, int W, int H,
                           int block, int ratio, int cut, void* d_out_keep, void* d_out_counts /* two uint32, or NULL */);
int ofps_hip_set_sad_intra(ofps_hip_ctx* ctx, int ratio);    /* sixteenths; 0 = off (default) */
int ofps_hip_get_sad_intra(ofps_hip_ctx* ctx);
int ofps_hip_set_sad_cut(ofps_hip_ctx* ctx, int percent);    /* 0 = off (default); no effect while the intra ratio is 0 */
int ofps_hip_get_sad_cut(ofps_hip_ctx* ctx);
int ofps_hip_sad_flow_intra_dev(ofps_hip_ctx* ctx, const void* d_frames, int n_frames, int W, int H, int stride, size_t frame_pitch,
                                int ref_mode, int block, int range, int min_pixels, int limit, int median, int intra /* >= 1 */, int cut,
                                void* d_out_entries /* pairs * nblk * 4 f32 */, void* d_out_best /* pairs * nblk * 3 i32, or NULL */,
                                void* d_out_counts /* pairs uint32 */);

/* ---- N1s: hip_sad's split blocks -- a block that holds two motions yields its four sub-blocks' vectors (csrc/sad_split.hip) ----
 * A lattice block that straddles a motion boundary has no right vector: its winner belongs to one side, to neither, or to whatever fits the
 * mixture, and every criterion above can only drop it.  The encoders whose vectors av-decoder reads split such a macroblock into
 * partitions, and the decoder yields one record per partition (av-decoder/src/lib.rs:396-419).  Build-defined, like N1, N1q, N1g ... N1p;
 * all-integer, so bit-exact on every device.  For a frame pair (prev, cur), lattice `block` = B, sub-block side b = B / 2, `threshold` = T
 * in [1, 4080]:
 *   frames: the ones the integer search read -- the mean-removed copies with N1m on; with search levels (N1h) the step acts on level 0;
 *   parents: the integer winners (dx, dy, SAD) of the context's search, one per lattice block, after every other setting of the context
 *     (PRUNED, levels, predictors, mean removal); R0 = ofps_hip_sad_reach(range, levels);
 *   sub-block s in {0, 1, 2, 3} of block (bx, by), raster order: at (sx0, sy0) = (bx*B + (s & 1)*b, by*B + (s >> 1)*b);
 *   predictor list, in this order: the winner of (bx, by); the winners of (bx - 1, by), (bx + 1, by), (bx, by - 1), (bx, by + 1), those that
 *     exist in the lattice (a neighbour's keep flag is not looked at); (0, 0).  Predictors are not doubled.  Each is clamped on its own for
 *     this sub-block: px = clamp(px, -sx0, W - b - sx0), py alike; the block's own winner is never changed by the clamp;
 *   candidates d = p + e over all predictors p and e in [-3, 3]^2, valid iff 0 <= sx0 + dx <= W - b and the same in y;
 *   cost = sum |cur - prev displaced by d| over the b x b sub-block;
 *   winner = min of (SAD, dx*dx + dy*dy, dy + R0 + 3, dx + R0 + 3), lexicographic: a total order on d, so duplicate predictors and candidates
 *     cannot change it (the kernel drops duplicate predictors);
 *   consequence: the parent's winner is a valid candidate of each of its sub-blocks, so sum_s SAD_s <= SAD_parent and
 *     gain = SAD_parent - sum_s SAD_s >= 0;
 *   rule: a block is SPLIT iff 16 * gain >= T * B * B (64-bit signed): T counts sixteenths of a grey level per pixel of the block, as the
 *     intra test's ratio counts sixteenths;
 *   records: an unsplit kept block yields its one N1 record, bit for bit; a split kept block yields four records in sub-block order in its
 *     place, by N1's float expressions with the sub-block's centre (sx0 + b/2, sy0 + b/2) and d_s; a block dropped by gate, check, median
 *     test, intra test or cut rule yields nothing -- those criteria read the parents and are unchanged.  Block raster order; the count is
 *     variable, between kept and 4 * kept.
 * OFPS_HIP_EINVAL: B odd or b < 4 (B < 8); R0 + 3 > 127; T outside [0, 4080] at the setter and at the option OFPS_HIP_SAD_SPLIT
 * (environment / ofps_hip_set_option), outside [1, 4080] at the explicit calls.  With motion scale 4 and T > 0 a search call returns
 * OFPS_HIP_EUNSUPPORTED: quarter-pel sub-block vectors are a later step.  T = 0 = off, the default: every entry point then uses the
 * launches, streams, scratch and bytes of a build without this section.
 * ofps_hip_sad_record_capacity(ctx, W, H, block): the records out_entries must hold for a search call of this context: nblk with T = 0,
 *   4 * nblk with T > 0.
 * ofps_hip_sad_split[_dev]: the step alone on caller-held data, as ofps_hip_sad_refine is: best = the nblk parent triples (a predictor is
 *   clamped to the frame whatever they hold: no access out of bounds), keep = one byte per block (non-zero = kept) or NULL = all ones,
 *   reach = R0 in [0, 124] ->
 *   out_sub_best: the four sub-blocks' (dx, dy, SAD), 12 int32 per block, for every kept block whether split or not (zeros for the others);
 *   out_split: one byte per block; out_entries (or NULL): the raw slots, 4 records per block, slot 4 * blk + s; out_slot_flags (or NULL):
 *   one byte per slot -- an unsplit kept block fills slot 0 alone, with its N1 record, a split one all four, a block that is not kept none;
 *   a slot whose flag is 0 holds zeros.  An ordered compaction of the slots by their flags is the record stream above.  The _dev form
 *   enqueues only; the packed kernels need 4-byte aligned rows (other rows take the byte-wise form).
 * ofps_hip_sad_flow_split_dev: one pair in device memory: search + the three explicit criteria (min_pixels, limit, median; 0 = off each;
 *   the context's own criteria and T are not looked at) + split with T in [1, 4080] + ONE compaction + the count on the device:
 *   d_out_entries holds 4 * nblk records, d_out_count one uint32.  Enqueues only.
 * With the context's T > 0:
 *   ofps_hip_sad_flow: *n_out = the record count, out_entries has capacity 4 * nblk; out_best stays the PARENTS' triples, nblk of them,
 *     compacted by the keep flags as before.
 *   ofps_hip_push_frame[_async] / ofps_hip_frame_wait: the filtered path with the split step between the flags and the one compaction, on
 *     the compute stream; out_entries has capacity 4 * nblk, n_vectors = the record count, detector and estimator read the split stream
 *     through their device-count forms; no host synchronisation is added, and a ticket follows the T the context has when it is pushed.
 * Ignoring T, as they first ignored the gate (a later step): the batched and multi-device forms -- ofps_hip_sad_flow_dev, _gated_dev,
 * _checked_dev, _median_dev, _filtered_dev, _intra_dev, ofps_hip_push_frames_async, ofps_hip_multi_* -- which always produce at most nblk
 * records per pair, and the dense decoders. */
int ofps_hip_set_sad_split(ofps_hip_ctx* ctx, int threshold);   /* sixteenths; 0 = off (default) */
int ofps_hip_get_sad_split(ofps_hip_ctx* ctx);
size_t ofps_hip_sad_record_capacity(ofps_hip_ctx* ctx, int W, int H, int block);
int ofps_hip_sad_split(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int block,
                       const int32_t* best /* 3 * nblk */, const uint8_t* keep /* nblk or NULL = all ones */, int reach, int threshold,
                       int32_t* out_sub_best /* 12 * nblk */, uint8_t* out_split /* nblk */, float* out_entries /* 16 * nblk or NULL */,
                       uint8_t* out_slot_flags /* 4 * nblk or NULL */);
int ofps_hip_sad_split_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block, const void* d_best,
                           const void* d_keep /* or NULL */, int reach, int threshold, void* d_out_sub_best, void* d_out_split,
                           void* d_out_entries /* or NULL */, void* d_out_slot_flags /* or NULL */);
int ofps_hip_sad_flow_split_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block, int range,
                                int min_pixels, int limit, int median, int threshold, void* d_out_entries /* 4 * nblk * 4 f32 */,
                                void* d_out_count /* one uint32 */);

/* ---- N1h: hip_sad's search levels -- coarse-to-fine search for motion beyond the search range (csrc/sad_hier.hip) ----
 * The plain search cannot return a vector that was never a candidate: range 16 at 1080p ends at about one degree of camera rotation per
 * frame.  With levels = L in {2, 3} the search runs on the frames halved L - 1 times and every finer level repairs the doubled vectors in a
 * small window, as the hierarchical searches of the encoders do whose vectors av-decoder consumes.  Build-defined, like N1, N1q, N1g and
 * N1c.  For a frame pair (prev, cur), lattice `block` = B, `range` = R:
 *   pyramid: level 0 is the frame; level l+1 has W_{l+1} = W_l >> 1, H_{l+1} = H_l >> 1 and pixel (x, y) = (a + b + c + d + 2) >> 2 of the
 *     2 x 2 quad at (2x, 2y) of level l (a last odd column or row is unused): what ofps_hip_sad_down2 returns;
 *   top: T = the N1 winners of the plain search (block B, range R) on the level L-1 pair: exactly what ofps_hip_sad_flow returns for those two
 *     images at levels 1 (the kernel selection and the PRUNED mode apply to it as they do to any plain search);
 *   reach: R_{L-1} = R, R_l = 2 * R_{l+1} + 3;
 *   refinement, for l = L-2 down to 0, on the level-l lattice (nbx_l = W_l / B, nby_l = H_l / B, full blocks from (0, 0)); for the block
 *     (bx, by) at (x0, y0) = (bx*B, by*B): what ofps_hip_sad_refine returns:
 *       parent = (min(bx >> 1, nbx_{l+1} - 1), min(by >> 1, nby_{l+1} - 1)) of the level l+1 lattice;
 *       predictor p = 2 * the parent's winner, clamped so that the block lies inside the frame: px = clamp(px, -x0, W_l - B - x0), py alike
 *         (zero is always inside: the clamp never enlarges |p|);
 *       candidates d = p + e, e in [-3, 3]^2, valid iff 0 <= x0 + dx <= W_l - B and the same in y (e = 0 always is);
 *       cost = sum |cur_l - prev_l| over the block, prev_l displaced by d;
 *       winner = min of (SAD, dx*dx + dy*dy, dy + R_l, dx + R_l), lexicographic, d the total displacement;
 *   output: the level-0 winners (dx, dy, SAD) and their records in N1's convention, one per lattice block in raster order.
 * levels 1 = off, the default: every entry point then uses the launches, streams and bytes of a build without this section.  levels outside
 * {1, 2, 3} is OFPS_HIP_EINVAL at the setter.  A call is OFPS_HIP_EINVAL when the top level has no full block (W >> (L-1) < B or
 * H >> (L-1) < B) or when R_0 > 127 (the 10-bit fields of the quarter-pel key: 8 * R_0 + 6 <= 1023): levels 2 takes range <= 62, levels 3
 * range <= 29; the top search keeps N1's limits on block and range.  The option OFPS_HIP_SAD_LEVELS (environment / ofps_hip_set_option) sets
 * the same field.  ofps_hip_sad_reach(range, levels) = R_0, or a negative value when (range, levels) is invalid.
 * Every search of the context follows it: ofps_hip_sad_flow, ofps_hip_sad_flow_dev (both ref modes), ofps_hip_sad_flow_gated_dev /
 * _checked_dev, ofps_hip_push_frame[_async], ofps_hip_push_frames_async and the ofps_hip_multi_* workers (through the environment option).
 * Composition: quarter-pel (N1q) refines the level-0 winners, with R_0 where its key has `range`; the consistency check (N1c) runs both
 * directions over the same levels, its limits stay [1, 129] and "a limit above 2*range + 1 keeps every block" holds with R_0 for `range`; the
 * contrast gate (N1g) is untouched.  The refinement radius 3 is a constant of the build.
 * ofps_hip_sad_down2[_dev]: one frame, W, H >= 2, stride >= W -> (W >> 1) x (H >> 1) bytes, dst_stride >= W >> 1.
 * ofps_hip_sad_refine[_dev]: one refinement step of one pair: parent_best = the nbx_parent x nby_parent triples (dx, dy, sad) of the coarser
 *   lattice (only dx, dy are read), reach = R_l in [0, 127] for the key; out_best: nblk triples; out_entries: nblk records or NULL.  The
 *   triples are the caller's responsibility: a predictor is clamped to the frame whatever they hold (no access out of bounds), the winner is
 *   the definition's while every |d| <= 508.  The _dev forms enqueue only; their frames' rows must be 4-byte aligned (stride % 4 == 0). */
int ofps_hip_set_sad_levels(ofps_hip_ctx* ctx, int levels);   /* 1 = off (default) */
int ofps_hip_get_sad_levels(ofps_hip_ctx* ctx);
int ofps_hip_sad_reach(int range, int levels);
int ofps_hip_sad_down2(ofps_hip_ctx* ctx, const uint8_t* src, int W, int H, int stride, uint8_t* dst /* (H >> 1) rows of dst_stride bytes */, int dst_stride);
int ofps_hip_sad_down2_dev(ofps_hip_ctx* ctx, const void* d_src, int W, int H, int stride, void* d_dst, int dst_stride);
int ofps_hip_sad_refine(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int block,
                        const int32_t* parent_best /* 3 * nbx_parent * nby_parent */, int nbx_parent, int nby_parent, int reach,
                        int32_t* out_best /* 3 * nblk */, float* out_entries /* 4 * nblk or NULL */);
int ofps_hip_sad_refine_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block,
                            const void* d_parent_best, int nbx_parent, int nby_parent, int reach, void* d_out_best, void* d_out_entries /* or NULL */);

/* ---- N1p: neighbour and zero predictors for the search levels (csrc/sad_hier.hip) ----
 * Under N1h a refined block has one predictor, its parent's doubled winner: where that parent straddles a motion boundary, sits on low
 * texture in the box-filtered image, or had its match clipped by the frame edge, the +-3 window around it cannot return to the true
 * vector.  With sad_predictors = OFPS_HIP_SAD_PRED_NEIGHBOURS a block tries several predictors, as hierarchical encoder searches do, and
 * only the refinement paragraph of N1h changes.  Build-defined, all-integer, off by default.  For the block (bx, by) at (x0, y0) of level l:
 *   parent (qx, qy) = (min(bx >> 1, nbx_{l+1} - 1), min(by >> 1, nby_{l+1} - 1)), as in N1h;
 *   predictor list, in this order: 2 * the winner of parent (qx, qy); 2 * the winners of (qx - 1, qy), (qx + 1, qy), (qx, qy - 1),
 *     (qx, qy + 1), for those that exist in the parent lattice; (0, 0);
 *   each predictor is clamped on its own, after the doubling, with N1h's clamp: px = clamp(px, -x0, W_l - B - x0), py alike;
 *   candidates: the multiset of d = p + e over all predictors p and e in [-3, 3]^2, valid iff the displaced block lies inside the frame;
 *   cost and winner as in N1h: min of (SAD, dx*dx + dy*dy, dy + R_l, dx + R_l).  The key is a total order on d, so duplicate candidates and
 *     duplicate predictors cannot change the winner (the kernel drops duplicate predictors).
 * The pyramid, the top search, the reach R_l = 2 * R_{l+1} + 3 (every candidate still has |d| <= R_l: the neighbours' winners obey the
 * parent's bound and zero is inside), the EINVAL conditions and the output convention are N1h's.  OFPS_HIP_SAD_PRED_PARENT (0, the default)
 * is N1h as it stands: the launches and bytes of a build without this section.  Any other mode is OFPS_HIP_EINVAL at the setter, at the
 * option OFPS_HIP_SAD_PREDICTORS (environment / ofps_hip_set_option; the ofps_hip_multi_* workers follow it) and at
 * ofps_hip_sad_refine_pred[_dev].  At levels 1 the field is stored and has no effect.  Every search that follows `levels` follows it, and
 * the consistency check (N1c) runs both directions in the same mode.
 * ofps_hip_sad_refine_pred[_dev]: ofps_hip_sad_refine[_dev] with the predictor mode as an argument (mode 0 is that call). */
#define OFPS_HIP_SAD_PRED_PARENT 0
#define OFPS_HIP_SAD_PRED_NEIGHBOURS 1
int ofps_hip_set_sad_predictors(ofps_hip_ctx* ctx, int mode);   /* 0 = parent only (default) */
int ofps_hip_get_sad_predictors(ofps_hip_ctx* ctx);
int ofps_hip_sad_refine_pred(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int block,
                             const int32_t* parent_best /* 3 * nbx_parent * nby_parent */, int nbx_parent, int nby_parent, int reach,
                             int predictors, int32_t* out_best /* 3 * nblk */, float* out_entries /* 4 * nblk or NULL */);
int ofps_hip_sad_refine_pred_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block,
                                 const void* d_parent_best, int nbx_parent, int nby_parent, int reach, int predictors, void* d_out_best,
                                 void* d_out_entries /* or NULL */);

/* ---- N1m: hip_sad's mean removal -- a search that does not see a brightness change between the two frames (csrc/sad_prefilter.hip) ----
 * N1 compares raw luma: an exposure step, a flickering lamp or a passing cloud moves every block's SAD minimum away from the true vector, and
 * no later filter repairs it.  With sad_prefilter = r in [1, 16] every search of the context runs on the filtered pair F(prev), F(cur), the
 * prefilter of every stereo and block matcher.  Build-defined, like N1q / N1g / N1c / N1h; all-integer, so bit-exact on every device.  For a
 * frame v of W x H:
 *   window k = 2r + 1, n = k * k;
 *   S(x, y) = sum of v(clamp(x + i, 0, W - 1), clamp(y + j, 0, H - 1)) over i, j in [-r, r]: a replicated border; a frame smaller than the
 *     window is valid;
 *   m = (S + (n >> 1)) / n, integer division;
 *   F(x, y) = clamp(v(x, y) - m + 128, 0, 255): what ofps_hip_sad_prefilter returns.
 * Every search means: the plain and the PRUNED search; the search levels (N1h: the pyramid is built from F, not from the raw frames) and
 * their neighbour predictors (N1p); the quarter-pel refinement (N1q), which interpolates F; both directions of the consistency check (N1c).
 * The SAD field of the out_best triples is then the SAD of the FILTERED blocks (quarter-pel: of the interpolated filtered block).  The
 * contrast gate (N1g) keeps counting mask pixels of the UNFILTERED current frame.  Positions, the record convention, the reach and every
 * existing OFPS_HIP_EINVAL condition are unchanged.  It follows: ofps_hip_sad_flow, ofps_hip_sad_flow_dev (both ref modes; consecutive pairs
 * of one sequence are filtered once over n_frames frames, a shared key frame once), ofps_hip_sad_flow_gated_dev / _checked_dev,
 * ofps_hip_push_frame[_async], ofps_hip_push_frames_async and the ofps_hip_multi_* workers (through the environment option).  No filtered
 * frame is kept across searches: the two searches of the consistency check each filter their own pair.
 * 0 = off, the default: every entry point then uses the launches, streams, scratch and bytes of a build without this section.  A radius
 * outside [0, 16] is OFPS_HIP_EINVAL at the setter and at the option OFPS_HIP_SAD_PREFILTER (environment / ofps_hip_set_option), with the
 * value in the message.  The dense decoders (hip_lk, hip_flow) are not touched.
 * ofps_hip_sad_prefilter[_dev]: the filter alone on one frame, radius in [1, 16], W, H >= 1, stride >= W, dst_stride >= W; bytes of a dst row
 *   behind W are not written.  The _dev form enqueues only and takes any alignment (4-byte aligned rows are the fast path). */
int ofps_hip_set_sad_prefilter(ofps_hip_ctx* ctx, int radius);   /* 0 = off (default) */
int ofps_hip_get_sad_prefilter(ofps_hip_ctx* ctx);
int ofps_hip_sad_prefilter(ofps_hip_ctx* ctx, const uint8_t* src, int W, int H, int stride, int radius, uint8_t* dst /* H rows of dst_stride bytes */, int dst_stride);
int ofps_hip_sad_prefilter_dev(ofps_hip_ctx* ctx, const void* d_src, int W, int H, int stride, int radius, void* d_dst, int dst_stride);

/* ---- N2: dense per-pixel flow, pyramidal Lucas-Kanade ("hip_lk" Decoder) ----
 * The reference's only per-pixel flow is OpenCV's Farneback inside cv-decoder (cv-decoder/src/lib.rs:188-199); this
 * is a build-defined algorithm (oracle/ofps_oracle.c:orc_lk_flow) with cv-decoder's conventions: prev(x,y) ~
 * cur(x+u,y+v); records pos = ((x+.5)/W,(y+.5)/H), motion = flow/(W,H) in raster order (:239-243,262-269).
 * levels in [1,8] (cfg3: 3), radius in [1,15] (window (2r+1)^2), iters >= 1 Gauss-Newton steps per level.
 * out_flow: 2*W*H f32 (u,v) or NULL; out_entries: 4*W*H f32 or NULL (at least one of them). */
int ofps_hip_lk_flow(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride,
                     int levels, int radius, int iters, float* out_flow, float* out_entries);
/* Revision of the build-defined N2 arithmetic this library was compiled with: 2 = fused multiply-adds in the bilinear
 * sample, the residual sums and the structure tensor (the default), 1 = separate multiply and add (-DOFPS_LK_SPEC_FMA=0,
 * A/B builds).  The oracle exports the same number (orc_lk_spec_revision); the parity tests assert they agree. */
int ofps_hip_lk_spec_revision(void);
/* The flow runs its whole pyramid as ONE launch in which a tile waits for its parent tile of the coarser level to publish its flows.
 * Forward progress does not depend on how the device schedules the launch: a tile whose parent has not published within 0.3 ms computes the
 * missing ancestors itself (a tile's flows are a pure function of the frames: computed twice they are written twice with the same bits), so
 * every workgroup finishes in bounded time in any dispatch order, with any number of resident workgroups, on a CU-masked stream -- and no
 * flow is ever made from an unfinished parent.  Diagnostics (synchronises): how many tiles a waiting child computed since the flag buffer
 * was last allocated -- 0 on a whole device with an in-order dispatcher; a non-zero count costs time, never bits.  OFPS_HIP_LK_SERIAL=1 runs
 * one launch per pyramid level instead (A/B runs). */
int ofps_hip_lk_helped_tiles(ofps_hip_ctx* ctx, uint64_t* count);
/* ---- cv-decoder's frame front-end (cv-decoder/src/lib.rs:98-135): capped grid, resize(INTER_LINEAR), cvt_color(BGR2GRAY) ----
 * OpenCV's 8-bit arithmetic restated integer for integer (oracle/frontend_oracle.c names the sources; "parity unpinned": OpenCV is not vendored
 * by the reference): 11-bit bilinear coefficients with half-pixel centres, the horizontal edge rule, the uchar vertical pass
 * (((b0*(D0>>4))>>16) + ((b1*(D1>>4))>>16) + 2) >> 2, exact 2 x 2 reductions as the area mean; gray = (B*1868 + G*9617 + R*4899 + 8192) >> 14. */
enum { OFPS_HIP_FMT_LUMA = 0, OFPS_HIP_FMT_BGR = 1 /* VideoCapture's frames */, OFPS_HIP_FMT_RGBA = 2 /* ofps::RGBA's byte order */, OFPS_HIP_FMT_BGRA = 3 };
int ofps_hip_frame_channels(int fmt);                                            /* bytes per pixel: 1, 3, 4, 4; 0 = unknown format */
int ofps_hip_cv_grid(int W, int H, int max_w, int max_h, int* gw, int* gh);      /* :98-121 with aspect_ratio_scale (1, 1) */
/* resize keeping the channels: src H rows of W pixels of `fmt`, `stride` bytes apart -> dst dh x dw x channels, dense */
int ofps_hip_resize_linear(ofps_hip_ctx* ctx, const uint8_t* src, int W, int H, int stride, int fmt, uint8_t* dst, int dw, int dh);
int ofps_hip_resize_linear_dev(ofps_hip_ctx* ctx, const void* d_src, int W, int H, int stride, int fmt, void* d_dst, int dw, int dh);
/* what cv-decoder's read loop leaves in `self.gray` for one frame: [reduced != 0: resize to the capped grid ->] gray.  out_gray: *out_w x *out_h
 * dense bytes (capacity W * H is always enough). */
int ofps_hip_cv_frontend(ofps_hip_ctx* ctx, const uint8_t* frame, int W, int H, int stride, int fmt, int reduced, int max_w, int max_h,
                         uint8_t* out_gray, int* out_w, int* out_h);
int ofps_hip_cv_frontend_dev(ofps_hip_ctx* ctx, const void* d_frame, int W, int H, int stride, int fmt, int reduced, int max_w, int max_h,
                             void* d_out_gray, int* out_w, int* out_h);
/* cv-decoder's contrast mask (cv-decoder/src/lib.rs:203-237): Sobel(gray, CV_32F, 1, 1, ksize 5) -> threshold(> 20)
 * -> dilate(MORPH_ELLIPSE 11x11); a pixel contributes a record only where the mask is set (:253-257).  Restated
 * from OpenCV's published definitions (oracle/ofps_oracle.c:orc_contrast_mask; "parity unpinned": OpenCV is not
 * vendored by the reference).  out_mask: W*H bytes, 1 = keep. */
int ofps_hip_contrast_mask(ofps_hip_ctx* ctx, const uint8_t* gray, int W, int H, int stride, uint8_t* out_mask);
int ofps_hip_contrast_mask_dev(ofps_hip_ctx* ctx, const void* d_gray, int W, int H, int stride, void* d_out_mask);

/* ofps_hip_lk_decode / _lk_push_frame / _lk_push_frame_async flags */
#define OFPS_HIP_LK_CONTRAST_MASK 1u /* drop records of pixels outside the contrast mask of `cur` (the reference's
                                        Farneback path always masks, :203-237,253-257) */
#define OFPS_HIP_LK_FULLRES_RECORDS 2u /* an output form of this build, NOT a cv-decoder mode: one record per (unmasked) pixel of the
                                        full-resolution flow in raster order, no down-sampling -- the 2.07 M records of BASELINE
                                        configs[2] that feed ofps_hip_densify_raster_dev / ofps_hip_almeida_dev directly
                                        (API version 1 called this bit OFPS_HIP_LK_PER_PIXEL and mislabelled it "Process Fullres = false") */
#define OFPS_HIP_FLOW_FARNEBACK   4u /* the flow is Farneback's (ofps_hip_farneback_flow: levels = pyramid levels, winsize = 2 * radius + 1,
                                        iters = iterations, poly_n 7, poly_sigma 1.5) instead of the iterative Lucas-Kanade: "hip_flow".
                                        With this flag levels and radius may be 0 (no layer above the frame; a 1 x 1 window), as they may
                                        in ofps_hip_farneback_flow; winsize <= 15 means radius <= 7 */
#define OFPS_HIP_FLOW_USE_PREVIOUS 8u /* with OFPS_HIP_FLOW_FARNEBACK, stream forms: the flow of the stream's previous pair is this pair's initial
                                        flow -- OPTFLOW_USE_INITIAL_FLOW exactly as cv-decoder sets it from its second pair on
                                        (cv-decoder/src/lib.rs:161-165: `self.flow` persists between process_frame calls).  A stream's first
                                        pair (and ofps_hip_lk_decode, a pair on its own) starts from zero flow, like cv-decoder's first. */
#define OFPS_HIP_LK_REDUCED      16u /* cv-decoder's "Process Fullres" = false (cv-decoder/src/lib.rs:124-133,274-276): every frame is resized
                                        (imgproc::resize, INTER_LINEAR) to the (max_w, max_h)-capped grid of :98-121 BEFORE the colour
                                        conversion, mask and flow -- which therefore run on the ~150 x 84 frame -- and every unmasked
                                        pixel of that REDUCED frame is one record at ((x+.5)/gw, (y+.5)/gh) in raster order; no densifier.
                                        Excludes OFPS_HIP_LK_FULLRES_RECORDS. */
#define OFPS_HIP_FLOW_SPARSE     32u /* "hip_klt" (N3 below) in place of the flow, mask and output stage: levels, radius and iters mean L, w and K;
                                        out_w x out_h is the cell lattice of the frames the tracker reads and the capacity its slot count;
                                        max_w / max_h are ignored unless OFPS_HIP_LK_REDUCED is set.  Frame formats, OFPS_HIP_LK_REDUCED,
                                        the two tickets in flight, ofps_hip_lk_reset and the fused forms stay as they are; a ticket follows
                                        the ofps_hip_set_klt values the context has when it is pushed.  Excludes OFPS_HIP_LK_CONTRAST_MASK,
                                        OFPS_HIP_LK_FULLRES_RECORDS, OFPS_HIP_FLOW_FARNEBACK and OFPS_HIP_FLOW_USE_PREVIOUS
                                        (OFPS_HIP_EINVAL before anything is uploaded) */
/* The frames' pixel format, bits 8-9 of `flags` (one of the OFPS_HIP_FMT_* values below shifted left by 8; 0 = 8-bit luma, this build's
 * raw-stream input).  With a colour format `stride` is the row pitch in BYTES (>= W * channels) and every frame goes through
 * cvt_color(.., COLOR_BGR2GRAY)'s integer formula (cv-decoder/src/lib.rs:135) behind its upload -- after the resize when
 * OFPS_HIP_LK_REDUCED is set, as in the reference. */
#define OFPS_HIP_FRAME_FORMAT(fmt) ((unsigned)(fmt) << 8)
#define OFPS_HIP_FRAME_FORMAT_MASK 0x300u
/* (csrc/dense_decoder.hip)  One Decoder::process_frame of a "hip_lk" plugin (cv-decoder/src/lib.rs:82-294): flow -> per-pixel records
 * [-> contrast mask] -> down-sampled through the densifier to the (max_w, max_h)-capped grid of :98-121 (defaults
 * 150 x 150 -> 150 x 84 at 16:9) -> one record per visited cell in (x, y)-sorted order.  out_entries capacity:
 * 4 * min(max_w,W) * min(max_h,H) floats (4 * W * H with OFPS_HIP_LK_FULLRES_RECORDS).  out_w/out_h: the record grid (with
 * OFPS_HIP_LK_REDUCED also the size of the frames the flow ran on). */
int ofps_hip_lk_decode(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride,
                       int levels, int radius, int iters, int max_w, int max_h, unsigned flags,
                       float* out_entries, size_t* n_out, int* out_w, int* out_h);
/* The same for a STREAM of frames (cv-decoder keeps its previous gray frame and starts emitting with the second one,
 * cv-decoder/src/lib.rs:142-158): `frame` is uploaded once and is the next call's previous frame.  *have_vectors = 0 for
 * the first frame of a stream -- after ofps_hip_init, ofps_hip_lk_reset or a change of W/H.  The stream's two frames
 * live in device slots of their own: no other entry point of the context disturbs them. */
int ofps_hip_lk_push_frame(ofps_hip_ctx* ctx, const uint8_t* frame, int W, int H, int stride,
                           int levels, int radius, int iters, int max_w, int max_h, unsigned flags,
                           float* out_entries, size_t* n_out, int* out_w, int* out_h, int* have_vectors);
/* The same iteration split in two for read-ahead callers (cv-decoder's loop, cv-decoder/src/lib.rs:82-158, run one frame
 * ahead on a decoder thread as ofps-suite/src/app/tracking/worker.rs:165-226 does): push_frame_async returns once the frame's
 * H2D copy (on a copy stream when another ticket is in flight), the flow of (previous frame, this frame) and the output
 * stage are enqueued; the stage's last kernel writes the records and their count straight into the ticket's page-locked
 * block.  ofps_hip_lk_frame_wait(ticket) blocks until they are there and copies them to out_entries.  Up to 2 tickets in
 * flight: the upload of frame k+1 overlaps the flow of pair (k-1, k), and the host collects pair k-1's records meanwhile.
 * `frame` must stay valid until its ticket is collected (page-locked memory: ofps_hip_host_alloc; pageable memory makes the
 * copy synchronous).  ofps_hip_lk_push_frame == push_frame_async + frame_wait, bit for bit; both forms share one stream
 * of frames.  out_entries capacity as for ofps_hip_lk_decode. */
int ofps_hip_lk_push_frame_async(ofps_hip_ctx* ctx, const uint8_t* frame, int W, int H, int stride,
                                 int levels, int radius, int iters, int max_w, int max_h, unsigned flags, int* ticket);
int ofps_hip_lk_frame_wait(ofps_hip_ctx* ctx, int ticket, float* out_entries, size_t* n_out, int* out_w, int* out_h,
                           int* have_vectors);
int ofps_hip_lk_reset(ofps_hip_ctx* ctx);                  /* waits for tickets in flight; the next frame starts a new stream (zero initial flow) */
/* The same, but the stream's last flow stays the next pair's initial flow (OFPS_HIP_FLOW_USE_PREVIOUS): what a decoder calls when it skipped
 * frames and pushes the pair's first frame again -- cv-decoder's `self.flow` persists across skipped reads (cv-decoder/src/lib.rs:92-142,161-165). */
int ofps_hip_lk_rewind(ofps_hip_ctx* ctx);
int ofps_hip_lk_flow_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride,
                         int levels, int radius, int iters, void* d_out_flow, void* d_out_entries);
/* The same with a starting flow for the COARSEST pyramid level (d_init_flow: 2 f32 per pixel of that level, whose size is
 * W, H halved -- rounding up -- levels - 1 times; NULL = zero = ofps_hip_lk_flow_dev): a temporal prior, e.g. the previous
 * pair's flow reduced to that level -- the role of OPTFLOW_USE_INITIAL_FLOW in the call cv-decoder makes with flags 0
 * (cv-decoder/src/lib.rs:188-199).  Spec: oracle/ofps_oracle.c:orc_lk_flow_init. */
int ofps_hip_lk_flow_init_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride,
                              int levels, int radius, int iters, const void* d_init_flow, void* d_out_flow,
                              void* d_out_entries);

/* ---- N2 in the reference's own algorithm family: Farneback's polynomial-expansion flow as cv-decoder calls it
 * (cv-decoder/src/lib.rs:188-199: pyr_scale 0.5, levels 5, winsize 13, iterations 3, poly_n 7, poly_sigma 1.5; pyr_scale is fixed at 0.5).
 * The arithmetic the reference runs is OpenCV's (not part of the reference tree: PARITY UNPINNED); this is the published algorithm in the
 * form calcOpticalFlowFarneback gives it (flags = 0: box window), precision per stage as in OpenCV's CPU path -- DESIGN.md "N2b".
 * out_flow: 2*W*H f32 (dx, dy) per pixel of `prev` (prev(x,y) ~ cur(x+dx, y+dy)) or NULL; out_entries: 4*W*H f32 records or NULL (at least
 * one).  init_flow: NULL, or a 2*W*H flow to start from (OPTFLOW_USE_INITIAL_FLOW: cv-decoder passes its previous result).
 * winsize odd <= 15, poly_n <= 15, at most 6 + 1 pyramid layers of blur taps (levels <= 6 at any size): else OFPS_HIP_EUNSUPPORTED.
 * OFPS_HIP_FLOW_FARNEBACK in the `flags` of ofps_hip_lk_decode / _lk_push_frame / _lk_push_frame_async selects this flow for the
 * decoder entry points (levels = pyramid levels, winsize = 2 * radius + 1, iters = iterations; poly_n 7, poly_sigma 1.5). */
int ofps_hip_farneback_flow(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int levels, int winsize,
                            int iters, int poly_n, float poly_sigma, const float* init_flow, float* out_flow, float* out_entries);
int ofps_hip_farneback_flow_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int levels, int winsize,
                                int iters, int poly_n, float poly_sigma, const void* d_init_flow, void* d_out_flow, void* d_out_entries);
/* In the stream forms (ofps_hip_lk_push_frame[_async] with OFPS_HIP_FLOW_FARNEBACK) a pair's second frame is the next pair's first: its
 * pyramid and polynomial expansion are kept on the device and only the new frame goes through them (same results, bit for bit).
 * Diagnostics: how many calls of this context found the first frame's expansion already there. */
int ofps_hip_flow_cache_hits(ofps_hip_ctx* ctx, uint64_t* count);
/* ---- N3: sparse Lucas-Kanade on per-cell corner features ("hip_klt" Decoder; csrc/klt.hip) ----
 * Between hip_sad's block vectors and the dense flows: sub-pixel vectors at one well-chosen point per lattice cell.  Build-defined (the
 * reference has no counterpart; its report names sparse optical flow as future work).  Every sum over pixels is an exact integer and the
 * few f64 operations are scalar and in a fixed order, so the result does not depend on a reduction order: bit-exact against the NumPy
 * restatement tests/indep_klt.py.  Integers are signed 64-bit unless a smaller range is stated.
 * Settings of the context (ofps_hip_set_klt): cell C in {8, 16, 32} (16), score_radius r in [1, 3] (2), min_score in [1, 2^31 - 1] (1),
 *   min_eig e in [1, 65535] (1), max_residual R in [0, 4080], 0 = off (0).  Per call: levels L in [1, 6], radius w in [1, 7], iters K in
 *   [1, 30]; window side n = 2w + 1.  Frames: 8-bit luma, W x H with W >> (L - 1) >= 8 and H >> (L - 1) >= 8, stride >= W.  Anything else is
 *   OFPS_HIP_EINVAL.
 * Features (in prev): gradients = the 3 x 3 Sobel pair on integers (gx = right - left, gy = lower - upper, weights 1 2 1); a pixel is
 *   admissible iff r + 1 <= x <= W - r - 2 and the same in y; a, b, c = the sums of gx*gx, gx*gy, gy*gy over its (2r + 1)^2 window;
 *   D = (a - c)^2 + 4 b^2; score = a + c - ceil(sqrt(D)), the root exact.  The lattice has ceil(W / C) x ceil(H / C) cells from (0, 0), the
 *   slot index is raster order.  A cell's feature = its admissible pixel of largest score, ties to the smallest y, then the smallest x; a
 *   cell with no admissible pixel, or whose best score is below min_score, has none (status 1).
 * Pyramid: both frames' levels are ofps_hip_sad_down2's (N1h), as they are.
 * Sampling: positions are integers in 1/256 pixel, q = 256 i + f per axis (i = q >> 8, arithmetic); S(img, q) = (the sum of weight * pixel
 *   + 128) >> 8 over the four pixels (i, i + 1) x (j, j + 1), weights (256 - fx)(256 - fy), fx (256 - fy), (256 - fx) fy, fx fy, pixel indices
 *   clamped into the level's frame: no sample is ever refused; values carry 8 fractional bits.
 * Tracking the feature (x, y): dq = (0, 0); for l = L - 1 .. 0:
 *   centre cq = (((2x + 1) * 128) >> l) - 128, y alike;
 *   template I = S(prev_l, cq + 256 (i, j)), i, j in [-w - 1, w + 1]; Ix = I(i + 1, j) - I(i - 1, j), Iy alike, on the n x n interior;
 *     A11, A12, A22 = the sums of Ix*Ix, Ix*Iy, Iy*Iy;
 *   flat test: T = e * n * n * 262144; in f64 X = (double)(A11 - T), Y = (double)(A22 - T), Z = (double)A12; the feature is flat (status 2)
 *     unless X * Y >= Z * Z and X + Y >= 0;  det = (double)A11 * (double)A22 - Z * Z; det <= 0 is flat as well;
 *   up to K iterations: the feature has left the frame (status 3) unless 0 <= 256 x + dqx * 2^l <= 256 (W - 1) and the same in y (tested at
 *     level-0 scale); J = S(cur_l, cq + dq + 256 (i, j)) on the n x n window; b1 = sum (J - I) Ix, b2 = sum (J - I) Iy; in f64, in this order:
 *     num_x = (double)A22 * (double)b1 - Z * (double)b2, u_x = (-512.0 * num_x) / det; u_y alike with (double)A11 * (double)b2 - Z * (double)b1;
 *     uq = clamp(rint(u), -256 w, 256 w), round half even; dq += uq; stop when uq = (0, 0);
 *   if l > 0: dq = 2 dq.
 *   After level 0 the frame test once more, then res = sum |J - I| at the final dq; with R > 0, res > 16 R n n is a residual loss (status 4);
 *   otherwise the feature is kept (status 0).  Statuses 1, 2 and 3 report dq = (0, 0) and res = 0; status 4 reports its dq and res.
 * Records (cv-decoder's convention, as N2): pos = ((x + 0.5f) / W, (y + 0.5f) / H), motion = (((float)dqx / 256.0f) / W,
 *   ((float)dqy / 256.0f) / H), f32 divisions; the kept slots' records come first, in slot order, and their count is made on the device.
 * ofps_hip_klt_features[_dev]: one frame -> int32 (x, y, score) per slot, (-1, -1, 0) = no feature.
 * ofps_hip_klt_track[_dev]: the pair, n caller-given points as int32 (x, y) -> int32 (dqx, dqy, res, status) per point; min_eig and
 *   max_residual are the context's.  A point outside the frame: OFPS_HIP_EINVAL in the host form, status 3 in the _dev form (no access
 *   out of bounds).
 * ofps_hip_klt_flow[_dev]: the pair -> records (capacity: the slot count), their count (_dev: one uint32 in device memory) and, unless
 *   NULL, the raw slots: int32 (x, y, score, dqx, dqy, status) per slot, (-1, -1, 0, 0, 0, 1) for a cell without a feature.  Statuses: 0 kept,
 *   1 no feature, 2 flat, 3 left the frame, 4 residual loss, 5 did not return (N3f), 6 intra and 7 cut (N3i); 4 to 7 report their dq.
 * The _dev forms enqueue on the context's stream and synchronise nothing.  OFPS_HIP_FLOW_SPARSE (above) runs the same chain inside the
 * dense decoders' stream and fused forms. */
int ofps_hip_set_klt(ofps_hip_ctx* ctx, int cell, int score_radius, int min_score, int min_eig, int max_residual);
int ofps_hip_get_klt(ofps_hip_ctx* ctx, int32_t* cell, int32_t* score_radius, int32_t* min_score, int32_t* min_eig, int32_t* max_residual);   /* any may be NULL */
size_t ofps_hip_klt_slot_count(int W, int H, int cell);      /* ceil(W / cell) * ceil(H / cell); 0 for an invalid cell */
int ofps_hip_klt_features(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride, int32_t* out_triples /* 3 * slots */);
int ofps_hip_klt_features_dev(ofps_hip_ctx* ctx, const void* d_luma, int W, int H, int stride, void* d_out_triples);
int ofps_hip_klt_track(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, const int32_t* points /* 2 * n */,
                       size_t n, int levels, int radius, int iters, int32_t* out_quads /* 4 * n */);
int ofps_hip_klt_track_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, const void* d_points, size_t n,
                           int levels, int radius, int iters, void* d_out_quads);
int ofps_hip_klt_flow(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int levels, int radius, int iters,
                      float* out_entries /* 4 * slots */, uint32_t* n_out, int32_t* out_slots /* 6 * slots, or NULL */);
int ofps_hip_klt_flow_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int levels, int radius, int iters,
                          void* d_out_entries, void* d_out_count /* one uint32 */, void* d_out_slots /* or NULL */);

/* ---- N3m: hip_klt with mean removal: tracking that ignores a brightness offset between the frames (csrc/klt.hip) ----
 * Build-defined, off by default.  N3's step solves A u = -sum (J - I) grad I on raw grey levels: an offset o between the frames adds
 * o * sum grad I to the right-hand side and o per pixel to the residual.  A setting of the context, mean_removal in {0, 1}
 * (ofps_hip_set_klt_mean_removal; option and environment variable OFPS_HIP_KLT_MEAN_REMOVAL).  With 0 every entry point enqueues the
 * kernels it enqueues without this row.  With 1 tracking a feature differs from N3 in three places, and in nothing else; N = n * n:
 *   per level, after the template: sx = sum Ix, sy = sum Iy over the n x n interior; A11 = N * sum Ix*Ix - sx * sx,
 *     A12 = N * sum Ix*Iy - sx * sy, A22 = N * sum Iy*Iy - sy * sy; T = e * N * N * 262144; the flat test, det, X, Y and Z as in N3 on
 *     these values;
 *   per iteration: d = J - I on the window, sd = sum d; b1 = N * sum d*Ix - sd * sx, b2 = N * sum d*Iy - sd * sy; the f64 lines of N3
 *     (num_x, u_x = (-512.0 * num_x) / det, ..., rint, clamp) unchanged and in the same order.  This is the normal equation of the model
 *     "shift plus one unknown offset" with the offset eliminated; the common factor N cancels;
 *   residual, at the final dq: sd = sum d; m = floor((2 sd + N) / (2 N)), floor towards minus infinity; res = sum |d - m|; the loss test
 *     res > 16 R N is unchanged.
 * Number range: all integers are signed 64-bit.  With |Ix| <= 130,560, |d| <= 65,280 and N <= 225 every quantity stays below 9e14, so
 * the conversions to f64 are exact.
 * Consequences.  If no pixel of cur + o clips, on level 0 and on the pyramid's levels, S gives exactly J + 256 o, d shifts by 256 o and
 * b1, b2 and res do not change: the slots of (prev, cur + o) equal those of (prev, cur) bit for bit.  A window whose gradient is constant
 * (a ramp) has centred A = 0 and is status 2: shift and offset cannot be told apart there, so small windows on smooth content are flat
 * with mean removal where they are not without.
 * Every entry point that tracks follows the setting, with no new argument: ofps_hip_klt_track[_dev], _flow[_dev], _flow_batch[_dev],
 * OFPS_HIP_FLOW_SPARSE in the dense decoders' stream and fused forms, ofps_hip_push_frames_async and the multi-device workers' pushes
 * with the batch decoder at KLT (the workers' contexts read the environment variable at ofps_hip_init, as they read N3b's).
 * ofps_hip_klt_features[_dev] does not change: the score is built from gradients.  Bit-exact against the restatement
 * tests/indep_klt_zm.py.  A value other than 0 | 1 is OFPS_HIP_EINVAL and the setting stays as it was.  Additive: OFPS_HIP_API_VERSION
 * stays. */
int ofps_hip_set_klt_mean_removal(ofps_hip_ctx* ctx, int on);
int ofps_hip_get_klt_mean_removal(ofps_hip_ctx* ctx);        /* 0 | 1; OFPS_HIP_EINVAL for a NULL context */

/* ---- N3f: hip_klt's forward-backward check: a track that does not return to its feature is dropped (csrc/klt.hip) ----
 * Build-defined, off by default; hip_klt's counterpart of hip_sad's consistency check (N1c).  N3's only test of a finished track is the
 * optional residual limit: a track that converged on content that was repainted or uncovered between the frames, that lies beyond the
 * pyramid's reach or across a motion boundary is kept with full weight.  A setting of the context, fb_limit F in [0, 4096], in units of
 * 1/256 pixel (ofps_hip_set_klt_fb; option and environment variable OFPS_HIP_KLT_FB).  With F = 0 every entry point enqueues the kernels,
 * streams and bytes it enqueues without this row.  With F > 0 a slot whose forward track ends with status 0 and displacement dq runs a
 * backward pass:
 *   it starts at P = (256 x + dqx, 256 y + dqy), which the forward pass's final frame test has put inside the frame;
 *   it is N3's tracking with prev and cur exchanged, started at P: the template is sampled from cur_l; the level's centre is
 *     cq = ((P + 128) >> l) - 128 per axis, arithmetic shift (for P = 256 x this is N3's (((2x + 1) * 128) >> l) - 128); the frame test is on
 *     P + bq * 2^l against [0, 256 (W - 1)] and [0, 256 (H - 1)]; everything else is N3's text with the same L, w, K, min_eig and
 *     max_residual, and with N3m on the same mean-removal lines.  It yields (bqx, bqy, bres, bstatus);
 *   the round-trip distance is e = max(|dqx + bqx|, |dqy + bqy|), N1c's measure;
 *   the slot is kept iff bstatus == 0 and e < F; otherwise its status is 5, "did not return", which reports the forward dq and res, as
 *     status 4 does, and yields no record.  F = 1 is an exact round trip.
 * Statuses 1 to 4 are the forward pass's and are unchanged; kept records are, bit for bit, the records of the same slots without the
 * check.  On the device the backward pass runs inside the track launch, in the wave that finished the forward pass: no second launch, no
 * intermediate array, no launch count that depends on the number of pairs.
 * Every entry point that tracks follows the setting, with no new argument: ofps_hip_klt_track[_dev], _flow[_dev], _flow_batch[_dev] in
 * chain and key mode, OFPS_HIP_FLOW_SPARSE in the dense decoders' stream and fused forms, ofps_hip_push_frames_async and the multi-device
 * workers' pushes with the batch decoder at KLT (the workers' contexts read the environment variable at ofps_hip_init).
 * ofps_hip_klt_features[_dev] does not change.  A negative value or one above 4096 is OFPS_HIP_EINVAL and the setting stays as it was.
 * ofps_hip_klt_track_q[_dev]: the stage the check is built from.  ofps_hip_klt_track[_dev]'s signature with points as int32 (Px, Py) in
 * 1/256 pixel; one direction, from prev into cur as given, started at P as above, with the context's min_eig, max_residual and mean
 * removal; it never applies the check.  A point outside [0, 256 (W - 1)] x [0, 256 (H - 1)] is OFPS_HIP_EINVAL in the host form and
 * status 3 in the _dev form, with no access out of bounds.  At P = 256 (x, y) it answers what ofps_hip_klt_track answers at (x, y) with
 * the check off.  Bit-exact against the restatement tests/indep_klt_fb.py.  Additive: OFPS_HIP_API_VERSION stays. */
int ofps_hip_set_klt_fb(ofps_hip_ctx* ctx, int limit);
int ofps_hip_get_klt_fb(ofps_hip_ctx* ctx);                  /* [0, 4096]; OFPS_HIP_EINVAL for a NULL context */
int ofps_hip_klt_track_q(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, const int32_t* points /* 2 * n */,
                         size_t n, int levels, int radius, int iters, int32_t* out_quads /* 4 * n */);
int ofps_hip_klt_track_q_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, const void* d_points, size_t n,
                             int levels, int radius, int iters, void* d_out_quads);

/* ---- N3p: hip_klt with motion prediction: a track starts from the previous pair's flow (csrc/klt.hip, csrc/dense_decoder.hip) ----
 * Build-defined, off by default; hip_klt's counterpart of hip_sad's neighbour predictors (N1p) and of OFPS_HIP_FLOW_USE_PREVIOUS.  N3 starts
 * every track at dq = (0, 0), so the pyramid has to reach the whole motion of the pair; started from the previous pair's flow it has to
 * reach the CHANGE of motion between two pairs.
 * Guess.  A track may start from a guess g = (gx, gy), int32, in 1/256 pixel at level 0:
 *   N3's line "dq = (0, 0)" becomes dq = (gx >> (L - 1), gy >> (L - 1)), arithmetic shift (-1 >> 1 = -1; L = 1 is no shift);
 *   the guess is replaced by (0, 0) if |gx| or |gy| exceeds 2^23 (8,388,608);
 *   it is replaced by (0, 0) too if the start fails N3's frame test: 256 x + dqx * 2^(L - 1) outside [0, 256 (W - 1)] or
 *     256 y + dqy * 2^(L - 1) outside [0, 256 (H - 1)] (in a pass that starts at a position P, N3f's backward pass: P + ...);
 *   everything after that line is N3's text, N3m's where mean removal is on.  The reported dq is the whole displacement, guess included;
 *   statuses 1, 2 and 3 report zeros as before.  A guess of (0, 0) gives N3's answer bit for bit.
 * With N3f on, the backward pass starts at P = 256 (x, y) + dq as before, with the guess (-gx, -gy): the negation first, then the three
 *   rules above.  (Not the forward result: that would start the backward pass on the feature and weaken the check.)
 * Predictor.  The guess of lattice slot (cx, cy) is made from the raw slots of the previous pair on the same lattice, int32
 *   (x, y, score, dqx, dqy, status) per slot as ofps_hip_klt_flow writes them.  The candidates are the slot itself and its left, right,
 *   upper and lower lattice neighbours, those that lie inside the lattice and have status 0; slots of status 1 to 5 are not used.  With
 *   none the guess is (0, 0); with k of them it is, per component, the element of index (k - 1) / 2 (integer division) of the k values
 *   sorted ascending: the median, the lower middle for an even k.  All-integer.
 * Setting of the context, prediction in {0, 1} (ofps_hip_set_klt_prediction; option and environment variable OFPS_HIP_KLT_PREDICTION).
 *   Any other value is OFPS_HIP_EINVAL and the setting stays as it was.  With 0 every entry point enqueues the launches and bytes it
 *   enqueues without this row.  Only the stream forms below read it.
 * ofps_hip_klt_predict[_dev]: the previous pair's slots (6 * slots int32) and W, H, cell -> int32 (gx, gy) per slot: the predictor alone.
 * ofps_hip_klt_track_from[_dev]: ofps_hip_klt_track[_dev] with one guess per point, `guesses` (2 * n int32).  It follows the context's
 *   min_eig, max_residual, mean removal and fb_limit and does not read the prediction setting.  A guess beyond +-2^23 is OFPS_HIP_EINVAL
 *   in the host form and (0, 0) in the _dev form.
 * ofps_hip_klt_flow_from[_dev]: ofps_hip_klt_flow[_dev] with `prev_slots` (6 * slots int32, or NULL).  With NULL it is ofps_hip_klt_flow,
 *   bit for bit and launch for launch; otherwise every feature starts from its slot's predicted guess (the predictor runs inside the track
 *   launch).  The caller passes one call's out_slots to the next.  It does not read the setting either.  In the _dev form d_prev_slots
 *   and d_out_slots must not overlap (the track reads neighbours' previous slots while it writes its own: two buffers, alternating);
 *   overlapping arrays are OFPS_HIP_EINVAL.  The host form copies prev_slots first: there the two may be one array.
 * OFPS_HIP_FLOW_SPARSE in the dense decoders' stream and fused forms (ofps_hip_lk_push_frame*, ofps_hip_lk_push_frame_fused[_async], full
 *   resolution and reduced, every frame format): with the setting on the stream keeps the last pair's raw slots on the device (two buffers
 *   per stream that alternate by pair) and the track of pair k reads the slots of pair k - 1: records, counts, island and quaternion are
 *   those of a chain of ofps_hip_klt_flow_from calls on the frames the tracker reads.  The slots are forgotten on ofps_hip_lk_reset and
 *   ofps_hip_lk_rewind, on the stream's first pair, and on any change of geometry, format, mode, cell or flags.  A pair pushed with the
 *   setting off writes no slots, so its successor starts from zero: the setting may be switched in mid-stream.
 * The batch form ofps_hip_klt_flow_batch[_dev] and ofps_hip_push_frames_async IGNORE the setting while N3pb's switch (below) is 0, its
 *   default, and return the bytes they return without it: item k's guess depends on item k - 1's result, which serialises the one track
 *   launch N3b exists for, so that is asked for separately.  The multi-device workers IGNORE the setting and N3pb's switch always.
 *   ofps_hip_klt_track[_dev], _track_q[_dev], _flow[_dev] and ofps_hip_lk_decode start from (0, 0) as before.
 * Bit-exact against the restatement tests/indep_klt_pred.py.  Additive: OFPS_HIP_API_VERSION stays. */
int ofps_hip_set_klt_prediction(ofps_hip_ctx* ctx, int on);
int ofps_hip_get_klt_prediction(ofps_hip_ctx* ctx);          /* 0 | 1; OFPS_HIP_EINVAL for a NULL context */
int ofps_hip_klt_predict(ofps_hip_ctx* ctx, const int32_t* prev_slots /* 6 * slots */, int W, int H, int cell, int32_t* out_guesses /* 2 * slots */);
int ofps_hip_klt_predict_dev(ofps_hip_ctx* ctx, const void* d_prev_slots, int W, int H, int cell, void* d_out_guesses);
int ofps_hip_klt_track_from(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, const int32_t* points /* 2 * n */,
                            const int32_t* guesses /* 2 * n */, size_t n, int levels, int radius, int iters, int32_t* out_quads /* 4 * n */);
int ofps_hip_klt_track_from_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, const void* d_points,
                                const void* d_guesses, size_t n, int levels, int radius, int iters, void* d_out_quads);
int ofps_hip_klt_flow_from(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int levels, int radius, int iters,
                           const int32_t* prev_slots /* 6 * slots, or NULL */, float* out_entries, uint32_t* n_out, int32_t* out_slots /* or NULL */);
int ofps_hip_klt_flow_from_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int levels, int radius, int iters,
                               const void* d_prev_slots, void* d_out_entries, void* d_out_count, void* d_out_slots);

/* ---- N3b: hip_klt on a batch of pairs, and in the batched stream forms (csrc/klt.hip, csrc/pipeline.hip) ----
 * Nothing about the arithmetic is new.  Item k of a sequence of n_frames >= 2 frames, frame_pitch >= stride * H bytes apart, is the pair
 * (k, k + 1) with ref_mode 0 and (0, k + 1) with ref_mode 1; pairs = n_frames - 1.  Per item the kept records (kept slots first, in slot
 * order), their count and the raw slots equal ofps_hip_klt_flow on that pair with the context's settings, bit for bit.  Item k's records
 * lead item k's slot of ofps_hip_klt_slot_count(W, H, cell) records; what lies at and behind its count is unspecified (the host form
 * leaves it untouched); counts[k] is a uint32.  pairs * slots < 2^31.  The number of launches does not depend on pairs: one score launch
 * over the distinct previous frames, one halving per level over the distinct frames, one track launch of pairs * slots waves, one segmented
 * compaction (one workgroup per item).  Refused with OFPS_HIP_EINVAL before anything is enqueued or uploaded: what ofps_hip_klt_flow
 * refuses, n_frames < 2, a ref_mode other than 0 | 1, frame_pitch < stride * H.  The _dev form enqueues on the context's stream and
 * synchronises nothing.
 *
 * ofps_hip_set_batch_decoder: what ofps_hip_push_frames_async and the ofps_hip_multi_push_frames_async workers' pushes search with.
 * OFPS_HIP_BATCH_DECODER_SAD (default): hip_sad, exactly as without this switch; levels, radius and iters are not read.
 * OFPS_HIP_BATCH_DECODER_KLT: hip_klt with these levels, window radius and iterations (defaults 4, 7, 10) and the ofps_hip_set_klt values
 * the context has at the push.  Then params->block and params->range are ignored; a frame's record capacity is the slot count and
 * out_entries holds n * 4 * slots floats; frame j's n_vectors is its kept count, made on the device and read back behind the quaternions;
 * detector, estimator, islands and compensation read the counts on the device, nothing is read back between push and wait; a least-squares
 * fit of too few records is the identity, as in the fused sparse form of the dense decoders' stream; the stream's first frame, a geometry
 * change and ofps_hip_reset_frames behave as with hip_sad; a frame the decoder refuses (N3) is OFPS_HIP_EINVAL before the upload.  Only
 * luma frames.  Bounds against six ofps_hip_lk_push_frame_fused calls with OFPS_HIP_FLOW_SPARSE: records, counts and detector results
 * equal bit for bit, the quaternion to 2e-6; frame j's RANSAC seed is params->seed + j.  ofps_hip_multi_sad_flow, _stage_frames,
 * _run_resident and _fetch stay hip_sad.  The multi-device workers' contexts take the switch and the settings from the environment at
 * ofps_hip_init alone: OFPS_HIP_BATCH_DECODER, OFPS_HIP_KLT_LEVELS, OFPS_HIP_KLT_RADIUS, OFPS_HIP_KLT_ITERS, OFPS_HIP_KLT_CELL,
 * OFPS_HIP_KLT_SCORE_RADIUS, OFPS_HIP_KLT_MIN_SCORE, OFPS_HIP_KLT_MIN_EIG, OFPS_HIP_KLT_MAX_RESIDUAL (all ofps_hip_set_option names too).
 * Additive: OFPS_HIP_API_VERSION stays. */
int ofps_hip_klt_flow_batch(ofps_hip_ctx* ctx, const uint8_t* frames, int n_frames, int W, int H, int stride, size_t frame_pitch, int ref_mode,
                            int levels, int radius, int iters, float* out_entries /* pairs * 4 * slots */, uint32_t* out_counts /* pairs */,
                            int32_t* out_slots /* pairs * 6 * slots, or NULL */);
int ofps_hip_klt_flow_batch_dev(ofps_hip_ctx* ctx, const void* d_frames, int n_frames, int W, int H, int stride, size_t frame_pitch, int ref_mode,
                                int levels, int radius, int iters, void* d_out_entries /* pairs * slots float4 */,
                                void* d_out_counts /* pairs uint32 */, void* d_out_slots /* pairs * 6 * slots int32, or NULL */);
enum { OFPS_HIP_BATCH_DECODER_SAD = 0, OFPS_HIP_BATCH_DECODER_KLT = 1 };
int ofps_hip_set_batch_decoder(ofps_hip_ctx* ctx, int decoder, int levels, int radius, int iters);   /* levels, radius, iters: read only for KLT */
int ofps_hip_get_batch_decoder(ofps_hip_ctx* ctx, int32_t* decoder, int32_t* levels, int32_t* radius, int32_t* iters);   /* any may be NULL */

/* ---- N3pb: motion prediction in the batch form and the batched stream: a chained batch (csrc/klt.hip, csrc/pipeline.hip) ----
 * Build-defined, off by default.  Nothing about the arithmetic of N3, N3m, N3f or N3p changes.  A CHAINED batch: item k starts every track
 * from the guess that N3p's predictor makes from item k - 1's raw slots; item 0 starts from the guesses made from `prev_slots`, from (0, 0)
 * where there are none.  This holds in both ref_modes; with ref_mode 1 (pairs (0, k + 1)) the features, and so the lattice's slots, are the
 * same for all items, so every item only has to reach the increment of a displacement that grows with k.  With N3f on, the backward pass
 * starts from the negated guess, as in N3p.  Per item, records, count and raw slots equal a chain of ofps_hip_klt_flow_from calls on the
 * item's pair, each given the slots of the call before, bit for bit.
 * On the device only the track step serialises: the score launch, the one halving per level and the segmented compaction stay one launch
 * each for the whole batch; the track step is `pairs` launches on the context's stream, one item each, launch k reading the slots launch
 * k - 1 wrote (in the caller's slot array, or in scratch when the caller takes no slots).  Stream order is the only dependency between
 * items, and no launch reads the array it writes.
 * ofps_hip_klt_flow_batch_from[_dev]: ofps_hip_klt_flow_batch[_dev] with one more trailing argument, `prev_slots` (6 * slots int32, or
 *   NULL).  Always chained; it reads neither prediction setting, as ofps_hip_klt_flow_from does not.  It refuses what _flow_batch refuses.
 *   In the _dev form d_prev_slots must not share a byte with d_out_slots (pairs * 6 * slots int32): OFPS_HIP_EINVAL.  The host form copies
 *   prev_slots first: there it may lie inside out_slots.
 * Switch of the context, batch_prediction in {0, 1} (ofps_hip_set_klt_batch_prediction; option and environment variable
 *   OFPS_HIP_KLT_BATCH_PREDICTION).  Any other value is OFPS_HIP_EINVAL and the setting stays as it was.  With the switch AND N3p's
 *   prediction setting both 1, ofps_hip_klt_flow_batch[_dev] is ofps_hip_klt_flow_batch_from[_dev] with NULL, and
 *   ofps_hip_push_frames_async with the batch decoder at KLT chains within a ticket and ACROSS tickets: the stream keeps the raw slots of
 *   its newest pair on the device (two buffers that alternate by ticket, so a ticket of one frame never reads what it writes; written and
 *   read on the compute stream alone), and the next ticket's first item starts from them.  Frame j's records, kept count, island and
 *   quaternion then do not depend on how the frames were cut into tickets, and equal those of the sparse one-pair stream with N3p's
 *   setting on (records and counts bit for bit, the rest within N3b's bounds).  The slots are forgotten on the stream's first frame, on a
 *   change of geometry or cell, on ofps_hip_reset_frames, and by any ticket pushed with either setting at 0 or with the search as decoder:
 *   such a ticket enqueues exactly what it enqueues without this row and leaves no slots, so its successor starts from zero.  The
 *   settings may be switched in mid-stream.  With either at 0 every batched form enqueues the launches and bytes it enqueues without this
 *   row.
 * The multi-device workers (ofps_hip_multi_push_frames_async) ignore both settings: a worker sees every n-th batch, so its first item has
 *   no predecessor on its device, and an answer must not depend on the number of devices.
 * Bit-exact against the restatement tests/indep_klt_batch_pred.py.  Additive: OFPS_HIP_API_VERSION stays. */
int ofps_hip_set_klt_batch_prediction(ofps_hip_ctx* ctx, int on);
int ofps_hip_get_klt_batch_prediction(ofps_hip_ctx* ctx);    /* 0 | 1; OFPS_HIP_EINVAL for a NULL context */
int ofps_hip_klt_flow_batch_from(ofps_hip_ctx* ctx, const uint8_t* frames, int n_frames, int W, int H, int stride, size_t frame_pitch, int ref_mode,
                                 int levels, int radius, int iters, float* out_entries /* pairs * 4 * slots */, uint32_t* out_counts /* pairs */,
                                 int32_t* out_slots /* pairs * 6 * slots, or NULL */, const int32_t* prev_slots /* 6 * slots, or NULL */);
int ofps_hip_klt_flow_batch_from_dev(ofps_hip_ctx* ctx, const void* d_frames, int n_frames, int W, int H, int stride, size_t frame_pitch,
                                     int ref_mode, int levels, int radius, int iters, void* d_out_entries, void* d_out_counts,
                                     void* d_out_slots /* or NULL */, const void* d_prev_slots /* or NULL */);

/* ---- N3i: hip_klt's intra test and scene-cut rule: a track that found nothing that belongs to it is dropped (csrc/klt_intra.hip) ----
 * Build-defined, off by default; hip_klt's counterpart of hip_sad's intra test (N1i).  A pyramidal tracker started on content that has no
 * counterpart in the other frame -- across a scene cut, on uncovered background, on an object that appears, beyond the pyramid's reach --
 * still converges somewhere inside its reach and is reported with status 0 and full weight; N3's only guard is max_residual, an absolute
 * grey-level limit that has to be tuned to the texture.  This test compares the residual the track reports with the window's own activity.
 * All arithmetic is integer.  It applies to a pair tracked with the context's KLT settings and the call's L, w, K; n = 2w + 1, N = n * n.
 * Activity A(k) of a slot with feature (x, y): the n x n window of the RAW level-0 previous frame centred on (x, y), pixel indices clamped
 *   into the frame as N3's sampling clamps them; S = sum p, m = (S + N / 2) / N (integer division), A = sum |p - m|: a uint32, at most
 *   225 * 255.  A is 1/256 of sum |Ic - 256 m| over the level-0 template's interior, so 256 A is in res's unit.  The key-frame form
 *   (ref_mode 1) takes the window from the key frame.
 * Residual res(k): the forward pass's residual exactly as the slot reports it: with N3m on the residual around the window's mean difference,
 *   with N3f on the forward pass's.
 * Candidates: cand(k) iff the slot's final status is 0, 4 or 5, the statuses that report a residual.
 * Intra: ratio q in [1, 255], in sixteenths; intra(k) iff cand(k) and 16 * res(k) >= q * 256 * A(k), compared in signed 64-bit arithmetic;
 *   equality is intra, so A = 0 with res = 0 is intra.
 * Status 6, "intra": a slot with status 0 that is intra gets status 6; it reports its dq, as status 4 does, and yields no record.  Statuses 4
 *   and 5 stay as they are (earlier tests win).  Kept records are, bit for bit, the records of the same slots with the test off.
 * Scene cut: P in [0, 100] percent; n_cand and n_intra are counted over the pair, the candidates of status 4 and 5 included.  With P > 0 the
 *   pair is a CUT iff 100 * n_intra >= P * n_cand (so n_cand = 0 is a cut): it yields zero records and every status 0 that is left becomes
 *   status 7, "cut".  P has no effect while q = 0; setting it then is accepted.
 * Prediction (N3p, N3pb) needs no new rule: the predictor reads status 0 only, and statuses 6 and 7 stand in the raw slots before the next
 *   pair's or item's track launch reads them: after a cut every guess is (0, 0).  In a chained batch item k's verdict and cut are enqueued
 *   behind item k's track launch and in front of item k + 1's.
 * Settings of the context: intra q in [0, 255], 0 = off (ofps_hip_set_klt_intra; option and environment variable OFPS_HIP_KLT_INTRA) and cut P
 *   in [0, 100], 0 = off (ofps_hip_set_klt_cut; OFPS_HIP_KLT_CUT).  A value outside its range is OFPS_HIP_EINVAL and the setting stays as it
 *   was.  With q = 0 every entry point enqueues the launches, scratch and bytes it enqueues without this row.  With q > 0 the test runs in
 *   launches of its own between the track launch and the compaction: one verdict launch (a chained batch: one per item) and, with P > 0, one
 *   cut launch behind it; the track kernels are the ones that run without it.  No host synchronisation is added.
 * Every form that runs the decoder follows the two settings, with no new argument: ofps_hip_klt_flow[_dev] and _flow_from[_dev],
 *   _flow_batch[_dev] and _flow_batch_from[_dev] in both ref_modes, OFPS_HIP_FLOW_SPARSE in the dense decoders' stream and fused forms (a cut
 *   frame has n_vectors 0: the estimator answers the identity and the detector no motion, as for any frame without records),
 *   ofps_hip_push_frames_async with the batch decoder at KLT, and the multi-device workers, whose contexts read the two variables at
 *   ofps_hip_init.  ofps_hip_klt_track*[_dev] are stages and never apply the test.
 * ofps_hip_klt_activity[_dev]: one frame, n points as int32 (x, y), radius w in [1, 7] -> uint32 A per point.  A point outside the frame is
 *   OFPS_HIP_EINVAL in the host form and A = 0 in the _dev form, with no access out of bounds.
 * ofps_hip_klt_intra[_dev]: verdict and cut on caller-held data: n quads (dqx, dqy, res, status) as ofps_hip_klt_track writes them, n
 *   activities, ratio in [1, 255], cut in [0, 100] -> int32 statuses (6 and 7 as above) and, unless NULL, [n_cand, n_intra] as uint32.
 * Bit-exact against the restatement tests/indep_klt_intra.py.  Additive: OFPS_HIP_API_VERSION stays. */
int ofps_hip_set_klt_intra(ofps_hip_ctx* ctx, int ratio);
int ofps_hip_get_klt_intra(ofps_hip_ctx* ctx);               /* [0, 255]; OFPS_HIP_EINVAL for a NULL context */
int ofps_hip_set_klt_cut(ofps_hip_ctx* ctx, int percent);
int ofps_hip_get_klt_cut(ofps_hip_ctx* ctx);                 /* [0, 100]; OFPS_HIP_EINVAL for a NULL context */
int ofps_hip_klt_activity(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride, const int32_t* points /* 2 * n */, size_t n, int radius,
                          uint32_t* out_activity /* n */);
int ofps_hip_klt_activity_dev(ofps_hip_ctx* ctx, const void* d_luma, int W, int H, int stride, const void* d_points, size_t n, int radius,
                              void* d_out_activity);
int ofps_hip_klt_intra(ofps_hip_ctx* ctx, const int32_t* quads /* 4 * n */, const uint32_t* activity /* n */, size_t n, int ratio, int cut,
                       int32_t* out_status /* n */, uint32_t* out_counts /* 2, or NULL */);
int ofps_hip_klt_intra_dev(ofps_hip_ctx* ctx, const void* d_quads, const void* d_activity, size_t n, int ratio, int cut, void* d_out_status,
                           void* d_out_counts /* or NULL */);

/* ---- A1-A4: MotionFieldDensifier ---- */
int ofps_hip_densify(ofps_hip_ctx* ctx, const float* entries, size_t n, int w, int h,
                     float* out_field /* 2*w*h, cell (x,y) at 2*(y*w+x) */,
                     uint32_t* out_cells /* 2*n (x,y) per entry, or NULL */);
/* add_vector_weighted (ofps/src/motion_field.rs:164-178): entry i is inserted with weights[i]: counts += w,
 * sum = motion * w + sum, in input order; ofps_hip_densify is the weights == 1 case (add_vector, :188-190). */
int ofps_hip_densify_weighted(ofps_hip_ctx* ctx, const float* entries, const float* weights, size_t n, int w, int h,
                              float* out_field /* 2*w*h */, uint32_t* out_cells /* 2*n or NULL */);
/* batch items of n_per_item entries each (contiguous); outputs per item. */
int ofps_hip_densify_dev(ofps_hip_ctx* ctx, const void* d_entries, size_t n_per_item, int batch,
                         int w, int h, void* d_out_field, void* d_out_cells /* or NULL */);
/* The same fields for a PER-PIXEL producer (cv-decoder/src/lib.rs:239-291): d_entries holds W*H records in raster order
 * whose positions are ((x+.5)/W, (y+.5)/H) -- what ofps_hip_lk_flow_dev writes -- and d_mask (W*H bytes, or NULL) selects
 * the records that are inserted (cv-decoder's contrast mask, :251-276).  A cell's records are then a rectangle of pixels
 * in raster order, which is their input order: one launch, no sort, the same bits as ofps_hip_densify_dev on the
 * (compacted) records.  verify != 0 checks the precondition on the device first (blocking) and fails with
 * OFPS_HIP_EINVAL when a record is not where the lattice puts it; without it a violated precondition gives an
 * unspecified field. */
int ofps_hip_densify_raster_dev(ofps_hip_ctx* ctx, const void* d_entries, const void* d_mask /* or NULL */, int W, int H,
                                int w, int h, void* d_out_field /* 2*w*h floats */, int verify);
int ofps_hip_densify_to_entries(ofps_hip_ctx* ctx, const float* entries, size_t n, int w, int h,
                                float* out_entries /* capacity 4*w*h */, size_t* n_out);

/* new_densifier + add_vector (all entries) + interpolate_empty_cells + from_densifier: the sequence of
 * flow-extract/src/main.rs:74-83 (ofps/src/motion_field.rs:193-294).  Sequential by definition. */
int ofps_hip_densify_interpolated(ofps_hip_ctx* ctx, const float* entries, size_t n, int w, int h, float* out_field);

/* ---- A5: BlockMotionDetection::detect_motion ("hip_block_motion" Detector) ---- */
int ofps_hip_block_dim(float min_size, size_t subdivide);
int ofps_hip_detect(ofps_hip_ctx* ctx, const float* entries, size_t n,
                    float min_size, size_t subdivide, float target_motion,
                    int* has_motion, size_t* area, int* dim, float* out_field /* 2*dim*dim */);
/* per item result record: int32[4] = {has_motion, area, dim, 0}; field 2*dim*dim f32 per item. */
int ofps_hip_detect_dev(ofps_hip_ctx* ctx, const void* d_entries, size_t n_per_item, int batch,
                        float min_size, size_t subdivide, float target_motion,
                        void* d_out_result, void* d_out_field);

/* ---- A5i: every moving island, not the largest alone (csrc/detect.hip; build-defined, off by default) ----
 * A5 answers "is there an island of at least min_size, and which cells does the largest cover" -- the reference's detect_motion, which
 * stays as it is.  The labelling behind it knows every 8-connected component; this extension hands them out.  Build-defined: the
 * reference has no counterpart, the definition below is this library's.
 * Inputs: those of ofps_hip_detect plus max_islands = K in [1, 6400] (6400: the most components a 160 x 160 grid holds).
 *   dim = ofps_hip_block_dim(min_size, subdivide), cells = dim * dim; f = the densified field, the detector's own densify call;
 *   cell i = y * dim + x is lit iff sqrtf(f.x * f.x + f.y * f.y) >= target_motion (the detector's expression, no contraction);
 *   a component is an 8-connected set of lit cells; its seed is its smallest cell index, its area its cell count; it qualifies iff
 *   (float)area / (float)cells >= min_size (the detector's test);
 *   the islands are the qualifying components ordered by area descending, then seed ascending -- a total order.  Island 0 is the
 *   detector's winner (strict >, first in raster order).  Listed: ranks 0 .. min(n_islands, K) - 1.
 * Outputs:
 *   counts, int32[4]: n_islands (all qualifying components, also beyond K), n_components (all, any size), dim, n_listed;
 *   table, int32[8] per listed island in rank order: seed, area, x0, y0, x1, y1, sum_x, sum_y -- the inclusive bounding box in cells and
 *     the integer sums of the cells' x and y; the centroid in frame coordinates is ((sum_x / area) + 0.5) / dim, the caller's to compute.
 *     Rows at and behind n_listed are unspecified;
 *   labels (optional), uint16 per cell: the rank of the cell's island if it is listed, else 0xFFFF;
 *   field (optional), 2 f32 per cell: f[i] where cell i belongs to a listed island and is not that island's seed, else (0, 0) -- the
 *     reference never copies a seed cell (block-motion-detector/src/lib.rs:79-102) and every island keeps that rule, so with K = 1 the
 *     field equals ofps_hip_detect's out_field bit for bit, with or without motion.
 * Everything but the field is integer and order-independent (integer atomics and owned writes), no float is summed: bit-exact by
 * construction.  Always: has_motion == (n_islands >= 1) and area == table[0].area.
 * ofps_hip_detect_islands_dev: item j reads n_per_item records at j * n_per_item, as ofps_hip_detect_dev does; counts 4 int32, table
 * 8 * max_islands int32, labels dim * dim uint16 and field 2 * dim * dim f32 per item; enqueues and returns.
 * K outside [1, 6400] and dim outside [1, 160]: OFPS_HIP_EINVAL.  out_labels is uint16_t[dim * dim] (typed void*).
 *
 * The fused per-frame entry points -- ofps_hip_push_frame[_async], ofps_hip_push_frames_async, ofps_hip_lk_push_frame_fused[_async] --
 * follow the context's max_islands (ofps_hip_set_detect_islands; the option OFPS_HIP_DETECT_ISLANDS sets the same field; 0 = off, the
 * default: every entry point enqueues exactly what a build without this extension enqueues).  A ticket follows the value the context
 * had when it was pushed.  With K > 0 and run_detector set, the tail computes counts, table and labels behind the detector, on its
 * stream, from the records the detector reads (detect-compensation mode 1: the compensated records; device-side counts: the first
 * d_n[j] records): one launch and one copy into a page-locked block of the ticket, no host synchronisation between push and wait.  The
 * wait copies them into memory the context owns -- a later push cannot disturb them -- and ofps_hip_frame_islands returns those of
 * `item` of the most recently collected fused ticket: item 0 for the single-frame forms, 0 .. n - 1 after ofps_hip_frames_wait.  A frame
 * that yielded no vectors (a stream's first) has n_islands = n_components = 0.  OFPS_HIP_EINVAL: the ticket was pushed with K = 0 or
 * without the detector; item out of range; capacity (in records) < n_listed.  ofps_hip_frame_result and the fused out_field do not
 * change: out_field stays the largest island's.
 * Out of scope: the worker contexts of ofps_hip_multi_* ignore max_islands. */
int ofps_hip_detect_islands(ofps_hip_ctx* ctx, const float* entries, size_t n, float min_size, size_t subdivide, float target_motion,
                            int max_islands, int32_t out_counts[4], int32_t* out_table /* 8*max_islands */,
                            void* out_labels /* uint16 x dim*dim, or NULL */, float* out_field /* 2*dim*dim or NULL */);
int ofps_hip_detect_islands_dev(ofps_hip_ctx* ctx, const void* d_entries, size_t n_per_item, int batch, float min_size, size_t subdivide,
                                float target_motion, int max_islands, void* d_out_counts /* batch*4 */,
                                void* d_out_table /* batch*max_islands*8 */, void* d_out_labels /* or NULL */, void* d_out_field /* or NULL */);
int ofps_hip_set_detect_islands(ofps_hip_ctx* ctx, int max_islands);   /* 0 = off (default); option OFPS_HIP_DETECT_ISLANDS */
int ofps_hip_get_detect_islands(ofps_hip_ctx* ctx);
int ofps_hip_frame_islands(ofps_hip_ctx* ctx, int item, int32_t out_counts[4], int32_t* out_table, int capacity /* records */,
                           void* out_labels /* uint16 x dim*dim, or NULL */);

/* ---- A5t: island tracks -- follow the islands across frames (csrc/detect_tracks.hip; build-defined, off by default) ----
 * A5i ranks the islands of one frame by area; rank is not identity.  This step gives every listed island an id that survives rank
 * swaps and short gaps, an age, a hit count and the integer sums of its cells' motion.  Build-defined: the reference has a temporal rule
 * for the frame as a whole only (ofps-suite/src/app/detection.rs:195-212); the definition below is this library's.  All integer.
 * Parameters: max_tracks = T in [1, 256]; reach in [0, 4] cells (Chebyshev); max_gap = G in [0, 255] frames.
 * Input per frame: A5i's counts, table and labels for max_islands = K (the rows are matched by rank: the table is taken and not read);
 *   optionally cells, the densified field, 2 f32 per cell (the detector's own densify).
 * State: ofps_hip_island_tracker_bytes(dim, T) bytes, opaque to callers, 4-byte aligned; all-zero bytes are a fresh tracker.  It holds a
 *   step counter t, the count of ids handed out (the first id is 1; ids are never reused), per slot s < T (id, born, hits, last) with id 0
 *   = free, and per cell an owner (a slot or none) and gone, the frames since that owner was confirmed there.  Every byte of the state
 *   after a step is a function of the inputs: freed slots and cleared cells are written back to zero.  Layout: int32 t, handed, 0, 0; 4
 *   int32 per slot; uint16 owner per cell (slot + 1, 0 = none), padded to 16 bytes; uint8 gone per cell, padded to 16 bytes.  Ids stay
 *   below 2^31: a tracker that has handed out 2^31 - 1 ids is to be zeroed.
 * One step, with n = min(n_listed, T); only ranks r < n take part:
 *   1. t += 1.
 *   2. Overlap: for r < n and every live slot s, O[r][s] = the number of ordered pairs (c, c') with labels[c] == r, owner[c'] == s and
 *      max(|x - x'|, |y - y'|) <= reach, both cells inside the grid.  A pair count, nothing de-duplicated: at most 25,600 * 81.
 *   3. Match, in rank order r = 0 .. n - 1: among the live slots not yet claimed in this step with O[r][s] >= 1 take the largest O, ties
 *      to the smaller id; claim it, hits += 1, last = t.  If there is none: take the lowest-index free slot, id = the next id, born = t,
 *      hits = 1, last = t, claim it.  If there is no free slot either, the island is untracked in this frame.
 *   4. Paint: every cell of a tracked island gets owner = its slot and gone = 0.  Every other cell that has an owner -- cells of
 *      untracked islands and of islands at rank >= n among them -- gets gone += 1, and loses its owner (gone = 0) when gone > G.
 *   5. Expire: a live slot with t - last > G is freed (all four words zero) behind the matching; rule 4 has cleared its cells already.
 * Output per item:
 *   track_counts, int32[4]: rows = n, n_tracked = the rows with id != 0, n_live = the slots alive after the step, t;
 *   tracks, int32[8] per rank r < n, in rank order beside A5i's table row r: id (0 = untracked), slot (-1 = untracked), age = t - born + 1,
 *     hits (age and hits are 0 for an untracked row), sum_mx low and high word, sum_my low and high word.  Rows at and behind n are
 *     unspecified.  sum_mx and sum_my are the int64 sums of q(cells[c].x) and q(cells[c].y) over the cells labelled r, q(v) = the
 *     nearest-even integer of clamp(v, -64, 64) * 2^24 (exact in f32: one rintf of an exact value), q(NaN) = 0; both are 0 when cells
 *     is NULL.  The island's mean motion is sum / area / 2^24, the caller's to compute.
 * Consequences: a split leaves the id with the larger piece (the lower rank claims first); a merge keeps the id of the previous island
 * with the larger pair count; an island that vanishes for at most G frames comes back under its id with hits not advanced, after G + 1
 * frames under a new one.
 * ofps_hip_track_islands_dev steps `batch` items in order through one state, in one launch: item j reads counts at 4 j, labels at
 * dim * dim * j, cells at 2 * dim * dim * j and writes track_counts at 4 j and tracks at 8 * max_tracks * j; it only enqueues.
 * ofps_hip_detect_tracks runs densify, A5i and the steps for `batch` frames of n_per_item records each from host memory; the state
 * travels in and out, so 12 frames in one call, in 12 calls or cut 5 + 7 give the same rows and the same state bytes.
 * OFPS_HIP_EINVAL, before anything is enqueued: T, reach, G or K outside their ranges; dim outside [1, 160]; a NULL state.
 *
 * The fused entry points follow ofps_hip_set_detect_tracks (options OFPS_HIP_DETECT_TRACKS, OFPS_HIP_DETECT_TRACK_REACH,
 * OFPS_HIP_DETECT_TRACK_GAP; T = 0 is off and the default, reach 1 and gap 2 are the other defaults).  A ticket pushed with run_detector,
 * K > 0 and T > 0 takes one step per item that yielded vectors, behind the islands launch on its stream, on the island list and the field
 * the detector read (detect-compensation mode 1: motion relative to the camera); its rows travel in the ticket's page-locked block behind
 * every item's A5i block and ofps_hip_frame_tracks returns them, with ofps_hip_frame_islands' rules (capacity in rows).  An item without
 * vectors (a stream's first frame) takes no step: its track_counts are zero.  An item with vectors and no islands takes a step with n = 0.
 * Each of the three stream forms -- ofps_hip_push_frame[_async], ofps_hip_push_frames_async, ofps_hip_lk_push_frame_fused[_async] --
 * owns one state in context scratch; it starts from zeros after that form's reset, at the first frame of a stream, and when dim, T,
 * reach or G differ from the push before (a push with T = 0 or K = 0 among them).  Frame k's step runs behind frame k - 1's by stream
 * order; a batch ticket steps its items in frame order, so a frame's rows do not depend on how the frames were cut into tickets.  With
 * T = 0 or K = 0 nothing is enqueued, reserved or copied.  The worker contexts of ofps_hip_multi_* ignore the setting. */
size_t ofps_hip_island_tracker_bytes(int dim, int max_tracks);     /* 0: dim or max_tracks out of range */
int ofps_hip_track_islands_dev(ofps_hip_ctx* ctx, const void* d_counts /* batch*4 */, const void* d_table /* batch*max_islands*8 */,
                               const void* d_labels /* uint16 x batch*dim*dim */, const void* d_cells /* f32 x batch*2*dim*dim, or NULL */,
                               int dim, int max_islands, int batch, int max_tracks, int reach, int max_gap, void* d_state,
                               void* d_out_track_counts /* batch*4 */, void* d_out_tracks /* batch*max_tracks*8 */);
int ofps_hip_detect_tracks(ofps_hip_ctx* ctx, const float* entries, size_t n_per_item, int batch, float min_size, size_t subdivide,
                           float target_motion, int max_islands, int max_tracks, int reach, int max_gap, void* state /* in and out */,
                           int32_t* out_counts /* batch*4 */, int32_t* out_table /* batch*max_islands*8 */,
                           void* out_labels /* uint16 x batch*dim*dim, or NULL */, int32_t* out_track_counts /* batch*4 */,
                           int32_t* out_tracks /* batch*max_tracks*8 */);
int ofps_hip_set_detect_tracks(ofps_hip_ctx* ctx, int max_tracks, int reach, int max_gap);   /* max_tracks 0 = off (default) */
int ofps_hip_get_detect_tracks(ofps_hip_ctx* ctx, int* max_tracks, int* reach, int* max_gap);
int ofps_hip_frame_tracks(ofps_hip_ctx* ctx, int item, int32_t out_track_counts[4], int32_t* out_tracks, int capacity /* rows */);

/* ---- A6-A12: Almeida estimator ("hip_almeida" Estimator) ----
 * out_quat = (w,i,j,k) of the returned UnitQuaternion; out_tr = translation (always 0,
 * almeida-estimator/src/lib.rs:120).  seed drives the counter-based RANSAC sampler (the reference draws from
 * thread_rng): callers should advance it per call -- a constant seed samples the same positions every frame -- and
 * in a batched call item b uses seed + b.  Fields of more than 65,536 vectors (per-pixel records) are solved with
 * reciprocal-multiply quotients instead of IEEE division and fused multiply-adds (<= 1 ulp per operation; quaternion
 * within 2e-6 of the exact path).  Like the reference's estimator (singular system -> zero step,
 * almeida-estimator/src/lib.rs:181-185; < 3 inliers -> identity, :246-250) no entry point ever returns NaN: a cluster
 * launch whose workgroups were not all resident (another process holding CUs) finishes the solve inside the same
 * launch after its bounded wait (~0.3 s), on every entry point incl. the device-pointer and per-frame ones;
 * ofps_hip_almeida_recoveries counts how often that happened on this context (diagnostics; synchronises). */
int ofps_hip_almeida(ofps_hip_ctx* ctx, const float* entries, size_t n,
                     float aspect, float fov_y_deg, int use_ransac, size_t num_iters,
                     float inlier_deg, size_t num_samples, uint64_t seed,
                     float out_quat[4], float out_tr[3]);
int ofps_hip_almeida_dev(ofps_hip_ctx* ctx, const void* d_entries, size_t n_per_item, int batch,
                         float aspect, float fov_y_deg, int use_ransac, size_t num_iters,
                         float inlier_deg, size_t num_samples, uint64_t seed,
                         void* d_out_quat /* 4 f32 per item */);
int ofps_hip_almeida_recoveries(ofps_hip_ctx* ctx, uint64_t* count);

/* ---- A6c: camera compensation -- what moves relative to the camera (csrc/compensate.hip) ----
 * The residual of the reference's RANSAC inlier test, vec - camera.delta(pos, fit.inverse().to_homogeneous())
 * (almeida-estimator/src/lib.rs:224-231; delta: ofps/src/camera.rs:115-117), as an output.  Per record, in f32 without contraction:
 *   M = to_homogeneous(inverse(q)), q = (w,i,j,k) as ofps_hip_almeida returns it (oracle/ofps_oracle.c: orc_quat_inverse,
 *       orc_quat_to_homogeneous);
 *   d = camera.delta(pos, M), camera = (aspect, fov_y_deg) as for ofps_hip_almeida;
 *   out.pos = pos, the same bits; out.motion = motion - d.
 * ONE regime: the exact delta with IEEE divisions at every record count -- the estimator's reciprocal-quotient regime above 65,536
 * records has no counterpart here, a record's result does not depend on how many records there are.  n == 0 is valid; out_entries may
 * be entries (in place).  The _dev form takes `batch` items of n_per_item records and ONE quaternion per item from DEVICE memory
 * (4 f32 each -- what ofps_hip_almeida_dev wrote, no host copy or synchronisation in between), enqueues and returns.
 *
 * Detect-compensation mode of the fused per-frame entry points -- ofps_hip_push_frame[_async], ofps_hip_push_frames_async,
 * ofps_hip_lk_push_frame_fused[_async]; the option OFPS_HIP_DETECT_COMPENSATE (environment / ofps_hip_set_option) sets the same field:
 *   0 (the default): the detector reads the decoder's raw records -- the launches, streams and bytes of a build without this stage;
 *   1: when a ticket runs detector AND estimator, its detector reads that frame's records compensated with that frame's quaternion
 *      (LSQ or RANSAC as the parameters say, camera = the parameters' aspect / fov_y_deg): has_motion, area, dim and out_field describe
 *      the compensated field and equal ofps_hip_detect(ofps_hip_compensate(out_entries, quat)) bit for bit.  The vectors handed back in
 *      out_entries stay the raw decoder records and the quaternion is unchanged, both bit for bit.  The detector's chain then runs
 *      BEHIND the estimator and one compensation launch instead of beside the estimator.  A ticket whose estimator does not run has
 *      the raw detector, with no compensation launch and no error: camera.delta(pos, identity) is not exactly zero in f32, so
 *      "compensated with the identity" is NOT the definition.  A ticket follows the mode the context has when it is pushed.
 *   Any other value is OFPS_HIP_EINVAL.  ofps_hip_frame_params / ofps_hip_frame_result are unchanged (API version 2).
 * Out of scope: the worker contexts of ofps_hip_multi_* (always mode 0, also with the variable in the environment), the Python
 * plugins (ofps_amd/plugins.py) and the C++ host loops (ofps_amd/host) keep the default. */
int ofps_hip_compensate(ofps_hip_ctx* ctx, const float* entries, size_t n, float aspect, float fov_y_deg,
                        const float quat[4], float* out_entries /* 4*n */);
int ofps_hip_compensate_dev(ofps_hip_ctx* ctx, const void* d_entries, size_t n_per_item, int batch,
                            float aspect, float fov_y_deg, const void* d_quat /* 4 f32 per item, device memory */,
                            void* d_out_entries /* may equal d_entries */);
int ofps_hip_set_detect_compensation(ofps_hip_ctx* ctx, int mode);
int ofps_hip_get_detect_compensation(ofps_hip_ctx* ctx);

/* ---- fused per-frame path (live streams): decoder -> detector + estimator, vectors stay on the device ----
 * One call per arriving luma frame = one iteration of the reference's worker loops
 * (ofps-suite/src/app/detection.rs:111-148, tracking/worker.rs:328-361).  The context keeps the previous
 * frames on the device (a ring of three slots); the first frame after ofps_hip_init / ofps_hip_reset_frames / a geometry change
 * yields have_vectors = 0 (Decoder::process_frame -> Ok(false)). */
typedef struct {
    int block, range;                                   /* hip_sad */
    int run_detector;                                   /* hip_block_motion */
    float min_size; size_t subdivide; float target_motion;
    int run_estimator;                                  /* hip_almeida */
    float aspect, fov_y_deg; int use_ransac; size_t num_iters; float inlier_deg; size_t num_samples; uint64_t seed;
} ofps_hip_frame_params;
typedef struct {
    int have_vectors; size_t n_vectors;
    int has_motion; size_t area; int dim;               /* detector: Some((area, field dim x dim)) / None */
    float quat[4];                                      /* estimator: (w,i,j,k); identity when not run */
} ofps_hip_frame_result;
int ofps_hip_reset_frames(ofps_hip_ctx* ctx);
/* upload a frame as the stream's newest frame without computing anything: the frames `Decoder::process_frame` reads
 * past when called with `skip_frames > 0` (ofps/src/decoder.rs:47-60; cv-decoder/src/lib.rs:92-142 loops `cnt <= skip`) */
int ofps_hip_stage_frame(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride);
int ofps_hip_push_frame(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride,
                        const ofps_hip_frame_params* params, ofps_hip_frame_result* out,
                        float* out_entries /* 4*nblk or NULL */, float* out_field /* 2*dim*dim or NULL */);
/* The same iteration split in two for read-ahead callers (the reference decodes on its own thread into a double
 * buffer, ofps-suite/src/app/tracking/worker.rs:165-226): push_frame_async returns once the frame's H2D copy (on a
 * copy stream), its search and its tail are enqueued; ofps_hip_frame_wait(ticket) blocks until that frame's results
 * are on the host and fills `out`.  Up to 2 tickets may be in flight, so the upload of frame k+1 overlaps the search of
 * pair (k-1, k); tickets must be collected in order before a third push.  `luma`, `out_entries` and `out_field` must
 * stay valid until the wait returns; use ofps_hip_host_alloc'ed (page-locked) buffers -- pageable memory turns the
 * copies synchronous.  ofps_hip_push_frame == push_frame_async + frame_wait, bit for bit. */
int ofps_hip_push_frame_async(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride,
                              const ofps_hip_frame_params* params, float* out_entries /* 4*nblk or NULL */,
                              float* out_field /* 2*dim*dim or NULL */, int* ticket);
int ofps_hip_frame_wait(ofps_hip_ctx* ctx, int ticket, ofps_hip_frame_result* out);
/* The dense decoders ("hip_lk", "hip_flow") in the same shape: one ticket = frame -> records -> island + quaternion, the records and their
 * COUNT staying on the device between the decoder and its tail (the count of a dense decoder -- mask survivors, visited cells -- is only
 * known there: detector and estimator read it from device memory, every launch is sized from the records' capacity, nothing is read back
 * or synchronised between push and wait).  Arguments up to `flags` as for ofps_hip_lk_push_frame_async; `tail` is the
 * ofps_hip_frame_params of ofps_hip_push_frame with `block` / `range` ignored.  The wait fills `out` (n_vectors = the record count; a
 * stream's first frame: have_vectors = 0, identity, no motion), copies the records to out_entries (capacity as for ofps_hip_lk_decode)
 * and the island's field to out_field when given, and returns the record grid in out_w / out_h.  These calls and
 * ofps_hip_lk_push_frame[_async] are ONE stream of frames -- same ring (2 tickets in flight), same ofps_hip_lk_reset / _rewind, same kept
 * Farneback expansion and OFPS_HIP_FLOW_USE_PREVIOUS flow -- and may be mixed freely: ofps_hip_lk_frame_wait collects a fused ticket (the
 * tail's results are dropped), the fused wait a plain one (identity, no motion).  The records are bit for bit the plain form's; the
 * detector's result equals ofps_hip_detect on them bit for bit, the quaternion ofps_hip_almeida's to the solver's parity bound (2e-6
 * least squares: the launch partitions the capacity, not the count -- another fixed summation order; RANSAC draws the same samples).
 * OFPS_HIP_LK_FULLRES_RECORDS has no fused form (OFPS_HIP_EUNSUPPORTED): ofps_hip_lk_flow_dev -> ofps_hip_almeida_dev is that chain. */
int ofps_hip_lk_push_frame_fused_async(ofps_hip_ctx* ctx, const uint8_t* frame, int W, int H, int stride,
                                       int levels, int radius, int iters, int max_w, int max_h, unsigned flags,
                                       const ofps_hip_frame_params* tail, int* ticket);
int ofps_hip_lk_frame_fused_wait(ofps_hip_ctx* ctx, int ticket, ofps_hip_frame_result* out, float* out_entries /* or NULL */,
                                 float* out_field /* 2*dim*dim or NULL */, int* out_w, int* out_h);
int ofps_hip_lk_push_frame_fused(ofps_hip_ctx* ctx, const uint8_t* frame, int W, int H, int stride,
                                 int levels, int radius, int iters, int max_w, int max_h, unsigned flags,
                                 const ofps_hip_frame_params* tail, ofps_hip_frame_result* out, float* out_entries /* or NULL */,
                                 float* out_field /* 2*dim*dim or NULL */, int* out_w, int* out_h);
/* Batched read-ahead form: n consecutive frames of a stream per ticket (a decoder running n frames ahead).  `frames` holds
 * them frame_pitch bytes apart; ONE upload, one search launch over the batch's pairs, one detector chain and one
 * estimator launch over the batch, one read-back: a handful of HIP calls per batch instead of ~9 per frame.  Frame j is
 * paired with the stream's previous frame (the last frame of the previous batch for j = 0; the very first frame of a
 * stream yields have_vectors = 0).  Vectors and detector results equal n single pushes bit for bit; the quaternions agree
 * to the solver's parity bound (2e-6: a batch is solved by one launch over its items, a lone frame by the cluster solver --
 * two fixed summation orders), frame j's RANSAC seed = params->seed + j.  out_entries (n * nblk * 4 floats, or NULL) receives every frame's vectors at j * nblk * 4.  Up to 2 batches in
 * flight; `frames` / `out_entries` must stay valid until ofps_hip_frames_wait(ticket) returns, which fills out[0..n-1].
 * The batched stream is separate from the single-frame calls' (its own previous frame); ofps_hip_reset_frames resets both. */
int ofps_hip_push_frames_async(ofps_hip_ctx* ctx, const uint8_t* frames, int n, int W, int H, int stride, size_t frame_pitch,
                               const ofps_hip_frame_params* params, float* out_entries /* n*4*nblk or NULL */, int* ticket);
int ofps_hip_frames_wait(ofps_hip_ctx* ctx, int ticket, ofps_hip_frame_result* out /* n entries */);

/* ---- one host process, several GPUs: frame pairs are independent units, so a batch is split into
 * contiguous pair ranges, one worker thread + one context + one stream per entry of `devices` (an entry may repeat: the
 * workers are then independent contexts on one GPU).  No collective on the data path; in key mode (ref_mode 1: pair k =
 * frames 0, k+1) the key frame is uploaded once and fanned out device to device (hipMemcpyPeerAsync, xGMI point to
 * point).  Results come back in pair order.  The reference's counterpart is its worker-thread model
 * (ofps-suite/src/app/tracking/worker.rs:251-260,347-352); it has no multi-GPU code of its own. ---- */
/* Per-item checksum of device-resident data (records, fields): d_out_u64[item] = wrapping sum of the item's bytes read
 * as u64 words -- what a host gathers across GPUs instead of the records when it only needs to confirm them.  Enqueues on
 * the context's stream; bytes_per_item % 8 == 0. */
int ofps_hip_checksum_dev(ofps_hip_ctx* ctx, const void* d_data, size_t bytes_per_item, int batch, void* d_out_u64);
typedef struct ofps_hip_multi ofps_hip_multi;
int  ofps_hip_multi_init(const int* devices, int n, ofps_hip_multi** out);
void ofps_hip_multi_destroy(ofps_hip_multi* m);
const char* ofps_hip_multi_last_error(const ofps_hip_multi* m);       /* m may be NULL: last init error */
int  ofps_hip_multi_worker_count(const ofps_hip_multi* m);
/* How the shared key frame of ref_mode 1 reaches the workers' devices: 0 = hipMemcpyPeerAsync from the first worker's copy (the default),
 * 1 = ONE ncclBroadcast over an RCCL communicator of the workers' devices (xGMI) -- chosen at ofps_hip_multi_init when the environment
 * has OFPS_HIP_MULTI_RCCL=1, the devices are distinct and librccl.so can be dlopen'ed (the library does not link it).  *broadcasts (may
 * be NULL): key frames that went through ncclBroadcast so far. */
int  ofps_hip_multi_fanout(const ofps_hip_multi* m, uint64_t* broadcasts);
/* The partition, as pure functions (no device needed): worker k of n gets pairs [first, first + count) -- the first
 * n_pairs % n workers one more -- and keeps frames [first_frame, first_frame + n_frames) resident: count + 1 frames in
 * pair mode (one halo frame shared with the next worker), count frames in key mode (frame 0 arrives by the fan-out). */
void ofps_hip_multi_pair_range(size_t n_pairs, int n_workers, int k, size_t* first, size_t* count);
void ofps_hip_multi_frame_range(size_t n_pairs, int n_workers, int k, int ref_mode, size_t* first_frame, size_t* n_frames);
/* Host frames in (n_frames luma frames at frames + k * frame_pitch), vectors out in pair order:
 * out_entries [(n_frames - 1) * nblk * 4] f32.  = stage_frames + run_resident(1 step) + fetch. */
int ofps_hip_multi_sad_flow(ofps_hip_multi* m, const uint8_t* frames, int n_frames, int W, int H, int stride,
                            size_t frame_pitch, int ref_mode, int block, int range, float* out_entries);
/* The same in three parts, for callers that search a resident batch repeatedly (bench.py --launcher threads): upload and
 * partition; `steps` searches of every worker's resident pairs back to back (returns when all workers are through); copy
 * the last results back in pair order. */
int ofps_hip_multi_stage_frames(ofps_hip_multi* m, const uint8_t* frames, int n_frames, int W, int H, int stride,
                                size_t frame_pitch, int ref_mode);
int ofps_hip_multi_run_resident(ofps_hip_multi* m, int block, int range, int steps,
                                float* worker_ms /* NULL, or one entry per worker: HIP-event time of its `steps` launches */);
int ofps_hip_multi_fetch(ofps_hip_multi* m, int block, float* out_entries);     /* results of the LAST run of the staged batch, same block size */
/* The dispatcher's entry points are serialised among themselves (one lock per handle): several host threads may share a handle,
 * they just do not overlap inside it (ofps_hip_multi_frames_wait blocks outside the lock). */

/* A STREAM of frames over several devices: the multi-device form of ofps_hip_push_frames_async / ofps_hip_frames_wait (same
 * parameters, same results per frame).  Batch g of n consecutive frames goes to worker g % n_workers together with the one frame
 * in front of it (kept by the dispatcher in page-locked memory), through that worker's two-ticket batched read-ahead: upload on
 * a copy stream, one search launch, detector and estimator over the batch, results read back by kernel.  Up to 2 * n_workers
 * batches in flight; ofps_hip_multi_frames_wait(ticket) fills out[0..n-1] -- frame order is batch order.  `frames` and
 * `out_entries` must stay valid until the wait returns; batches in pageable memory are copied into a worker's page-locked
 * staging on that worker's thread.  Vectors and detector results equal the single-context stream's bit for bit, quaternions
 * too for equal batch sizes (one launch per batch either way).  The reference's counterpart: the decoder thread + double
 * buffer and the estimator fan-out of ofps-suite/src/app/tracking/worker.rs:165-226,347-361. */
int ofps_hip_multi_push_frames_async(ofps_hip_multi* m, const uint8_t* frames, int n, int W, int H, int stride, size_t frame_pitch,
                                     const ofps_hip_frame_params* params, float* out_entries /* n*4*nblk or NULL */, int* ticket);
int ofps_hip_multi_frames_wait(ofps_hip_multi* m, int ticket, ofps_hip_frame_result* out /* n entries */);
int ofps_hip_multi_reset_frames(ofps_hip_multi* m);
/* The dealing, as a pure function (no device needed): batch g of a stream -> the worker that takes it, the halo buffer that
 * holds the frame in front of it, and the ticket slot it occupies (at most two batches in flight per worker). */
void ofps_hip_multi_stream_plan(long batch, int n_workers, int* worker, int* halo_slot, int* ticket_slot);

#ifdef __cplusplus
}
#endif
#endif
