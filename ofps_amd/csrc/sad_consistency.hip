// sad_consistency.hip -- hip_sad's forward-backward consistency check (include/ofps_hip.h N1c): a lattice block yields a record only when
// the search in the other direction, started where its own winner points, comes back -- the round-trip test of flow and stereo pipelines.
// It drops what the contrast gate (sad_gate.hip) keeps: content that left the frame or was occluded, repeated texture, noise winners.
//
// Nothing here searches.  The backward winners are ofps::sad_pairs_device over SadFrames::swapped() (the search kernels of sad.hip are the
// parent's, untouched); this file holds what is behind the two searches:
// sad_consistency_kernel: one lane per block of one item (blockIdx.y; one pair is item 0): F[k] -> partner block k' -> G[k'] -> residual = max(|dx + ex|, |dy + ey|) -> keep byte.
//   12 + 12 bytes read per block (the gather hits the 12 bytes of a near neighbour: |d| <= 64 px is at most 8 blocks away), 1-5 written.
// The keep bytes feed the ordered compactions the gate already uses (mask.hip, compact_best_kernel): one compaction, one count.
//
// The two hazards of running a second search in one context (docs/history/20_sad_consistency.md):
//   motion scale 4: sad_pairs_device refines in place.  The backward call passes integer_only (no refinement, no S_SAD_QBEST); the forward
//     call passes d_int_best = S_CONS_FWD, where the integer winners are written and stay while the refinement writes elsewhere.
//   context scratch (S_SAD_QBEST, the pruned mode's S_SAD_LIST): both searches are enqueued on ctx->stream, the backward one right behind
//     the forward one, so the slots are reused in stream order and never shared.
#include "common.hpp"

namespace ofps {

// fwd / bwd: (dx, dy, sad) triples in integer pixels, only dx and dy are read.  keep_in (optional, may alias out_keep: a lane reads and
// writes its own byte only) is ANDed in.  Garbage winners (|d| > 64) give an unspecified flag: k' is clamped on both sides.
__device__ __forceinline__ void sad_consistency_block(const int* __restrict__ fwd, const int* __restrict__ bwd, int nbx, int nby, int B, int limit,
                                                      const uint8_t* keep_in, uint32_t* __restrict__ out_residual, uint8_t* out_keep) {
    const uint32_t nblk = (uint32_t)nbx * (uint32_t)nby;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= nblk) return;
    const int bx = (int)(k % (uint32_t)nbx), by = (int)(k / (uint32_t)nbx);
    const int dx = fwd[3 * (size_t)k], dy = fwd[3 * (size_t)k + 1];
    // the integer numerators of the record's pos: the centre of the matched block of the other frame
    // (64-bit sums: whatever the triples hold, nothing wraps; clamped into the lattice's pixels BEFORE the division, which is then a 32-bit one:
    // min(cx / B, nbx - 1) == min(cx, nbx * B - 1) / B for cx >= 0.  The upper clamp is what catches centres in the ragged right / bottom margin)
    const long long cx = (long long)bx * B + B / 2 + dx, cy = (long long)by * B + B / 2 + dy;
    const long long mx = (long long)nbx * B - 1, my = (long long)nby * B - 1;
    const uint32_t px = (uint32_t)(cx < 0 ? 0 : cx > mx ? mx : cx) / (uint32_t)B;
    const uint32_t py = (uint32_t)(cy < 0 ? 0 : cy > my ? my : cy) / (uint32_t)B;
    const size_t kp = (size_t)py * nbx + px;
    const int ex = bwd[3 * kp], ey = bwd[3 * kp + 1];
    const long long rx = (long long)dx + ex, ry = (long long)dy + ey;
    const unsigned long long ax = (unsigned long long)(rx < 0 ? -rx : rx), ay = (unsigned long long)(ry < 0 ? -ry : ry);
    const uint32_t res = (uint32_t)(ax > ay ? ax : ay);
    if (out_residual) out_residual[k] = res;
    if (out_keep) {
        bool keep = res < (uint32_t)limit;
        if (keep_in) keep = keep && keep_in[k] != 0;
        out_keep[k] = keep ? 1 : 0;
    }
}

// blockIdx.y is the item, every array nbx * nby elements per item.  The partner block is clamped into the item's own lattice
__global__ __launch_bounds__(256) void sad_consistency_kernel(const int* __restrict__ fwd, const int* __restrict__ bwd, int nbx, int nby, int B,
                                                              int limit, const uint8_t* keep_in, uint32_t* __restrict__ out_residual,
                                                              uint8_t* out_keep) {
    const size_t at = (size_t)blockIdx.y * ((size_t)nbx * nby);
    sad_consistency_block(fwd + 3 * at, bwd + 3 * at, nbx, nby, B, limit, keep_in ? keep_in + at : nullptr, out_residual ? out_residual + at : nullptr,
                          out_keep ? out_keep + at : nullptr);
}

int sad_consistency_check(ofps_hip_ctx* ctx, int block, int limit, const char* who) {
    OFPS_REQUIRE(ctx, block >= 1 && block <= 64, "%s: block=%d outside [1,64]", who, block);
    OFPS_REQUIRE(ctx, limit >= 1 && limit <= kSadConsistencyMax, "%s: consistency limit %d outside [1, %d]", who, limit, kSadConsistencyMax);
    return OFPS_HIP_OK;
}

int sad_consistency_flags_device(ofps_hip_ctx* ctx, const int* d_fwd_best, const int* d_bwd_best, int W, int H, int block, int limit,
                                 const uint8_t* d_keep_in, uint32_t* d_out_residual, uint8_t* d_out_keep, hipStream_t st, int items) {
    const int rc = sad_consistency_check(ctx, block, limit, "sad_consistency");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1, "sad_consistency: bad geometry W=%d H=%d", W, H);
    const int nbx = W / block, nby = H / block;
    if (nbx == 0 || nby == 0) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, (long long)nbx * nby < (1ll << 31), "sad_consistency: too many blocks");
    OFPS_REQUIRE(ctx, items >= 1 && items <= 65535, "sad_consistency: %d items", items);
    const size_t nblk = (size_t)nbx * nby;
    hipLaunchKernelGGL(sad_consistency_kernel, dim3((unsigned)((nblk + 255) / 256), (unsigned)items), dim3(256), 0, st, d_fwd_best, d_bwd_best, nbx,
                       nby, block, limit, d_keep_in, d_out_residual, d_out_keep);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

}  // namespace ofps

extern "C" {

int ofps_hip_sad_consistency_dev(ofps_hip_ctx* ctx, const void* d_fwd_best, const void* d_bwd_best, int W, int H, int block, int limit,
                                 void* d_out_residual, void* d_out_keep) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_fwd_best && d_bwd_best, "sad_consistency_dev: null device pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::sad_consistency_flags_device(ctx, static_cast<const int*>(d_fwd_best), static_cast<const int*>(d_bwd_best), W, H, block, limit,
                                              nullptr, static_cast<uint32_t*>(d_out_residual), static_cast<uint8_t*>(d_out_keep), ctx->stream);
}

int ofps_hip_sad_consistency(ofps_hip_ctx* ctx, const int32_t* fwd_best, const int32_t* bwd_best, int W, int H, int block, int limit,
                             uint32_t* out_residual, uint8_t* out_keep) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, fwd_best && bwd_best, "sad_consistency: null host pointer");
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1, "sad_consistency: bad geometry W=%d H=%d", W, H);
    int rc = ofps::sad_consistency_check(ctx, block, limit, "sad_consistency");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nblk = ofps_hip_sad_block_count(W, H, block);
    if (!nblk) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, nblk < (size_t(1) << 31), "sad_consistency: too many blocks");
    // [forward triples][backward triples] | [residuals][keep bytes]
    const size_t tri = nblk * 3 * sizeof(int32_t);
    auto* d_in = static_cast<char*>(ofps::scratch(ctx, ofps::S_CONS_FWD, 2 * tri));
    auto* d_flags = static_cast<char*>(ofps::scratch(ctx, ofps::S_GATE_FLAGS, ofps::gate_flags_bytes(nblk)));
    if (!d_in || !d_flags) return OFPS_HIP_ENOMEM;
    uint32_t* d_res = ofps::gate_counts(d_flags);
    uint8_t* d_keep = ofps::gate_keep(d_flags, nblk);
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_in, fwd_best, tri, hipMemcpyHostToDevice, ctx->stream));
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_in + tri, bwd_best, tri, hipMemcpyHostToDevice, ctx->stream));
    rc = ofps::sad_consistency_flags_device(ctx, reinterpret_cast<const int*>(d_in), reinterpret_cast<const int*>(d_in + tri), W, H, block, limit,
                                            nullptr, out_residual ? d_res : nullptr, out_keep ? d_keep : nullptr, ctx->stream);
    if (rc != OFPS_HIP_OK) return rc;
    if (out_residual) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_residual, d_res, nblk * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out_keep) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_keep, d_keep, nblk, hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_set_sad_consistency(ofps_hip_ctx* ctx, int limit) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, limit >= 0 && limit <= ofps::kSadConsistencyMax, "set_sad_consistency: %d outside [0, %d]", limit, ofps::kSadConsistencyMax);
    ctx->opt.sad_consistency = limit;
    return OFPS_HIP_OK;
}

int ofps_hip_get_sad_consistency(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.sad_consistency : OFPS_HIP_EINVAL; }

int ofps_hip_sad_flow_checked_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block, int range,
                                  int min_pixels, int limit, void* d_out_entries, void* d_out_best, void* d_out_count) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_prev && d_cur && d_out_entries && d_out_count, "sad_flow_checked_dev: null device pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = ofps::sad_consistency_check(ctx, block, limit, "sad_flow");           // (the filter itself takes 0 for "no check")
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_REQUIRE(ctx, min_pixels >= 0, "sad_flow: contrast gate %d is negative", min_pixels);
    return ofps::sad_flow_filtered_device(ctx, {static_cast<const uint8_t*>(d_prev), static_cast<const uint8_t*>(d_cur), 0, 0, W, H, stride}, 1, block,
                                          range, {min_pixels, limit}, static_cast<float4*>(d_out_entries), static_cast<int*>(d_out_best),
                                          static_cast<uint32_t*>(d_out_count), "sad_flow");
}

}  // extern "C"
