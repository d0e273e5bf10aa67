// sad_median.hip -- hip_sad's median test (include/ofps_hip.h N1v): a lattice block yields a record only when its integer winner lies
// within `limit` pixels of the component-wise median of its kept lattice neighbours' winners -- the outlier test of vector-field
// post-processing.  It drops what the contrast gate (sad_gate.hip) and the consistency check (sad_consistency.hip) keep: a clean, textured,
// round-trip-consistent match at the wrong place (repeated texture, a block clipped by the frame edge, the mask's dilation ring).
//
// Nothing here searches.  This file holds what is behind the search[es] and the other criteria's flags:
// sad_median_kernel: one lane per block of one item (blockIdx.y; one pair is item 0): up to 8 neighbours' (dx, dy) and incoming keep bytes -> two sorts of 8 in registers -> the two middle
//   order statistics per component -> residual in half-pixels -> keep byte.  At most 8 * (8 + 1) + 8 + 1 bytes read per block (neighbouring
//   lanes read the same lines), 1-5 written.  A latency-sized launch: no LDS, no tiling.
// One pass: every verdict reads the INCOMING flags of its neighbours, so the outgoing flags are another array (SadFilter: S_MED_KEEP).
#include "common.hpp"

#include <climits>

namespace ofps {

namespace {
__device__ __forceinline__ void cswap(int& a, int& b) { const int lo = min(a, b); b = max(a, b); a = lo; }

// ascending, 19 compare-exchanges in 6 layers (the optimal network for 8 inputs)
__device__ __forceinline__ void sort8(int (&s)[8]) {
    cswap(s[0], s[2]); cswap(s[1], s[3]); cswap(s[4], s[6]); cswap(s[5], s[7]);
    cswap(s[0], s[4]); cswap(s[1], s[5]); cswap(s[2], s[6]); cswap(s[3], s[7]);
    cswap(s[0], s[1]); cswap(s[2], s[3]); cswap(s[4], s[5]); cswap(s[6], s[7]);
    cswap(s[2], s[4]); cswap(s[3], s[5]);
    cswap(s[1], s[4]); cswap(s[3], s[6]);
    cswap(s[1], s[2]); cswap(s[3], s[4]); cswap(s[5], s[6]);
}

// |2 * d - (s[(n - 1) >> 1] + s[n >> 1])|, n in [1, 8]; 64-bit: whatever the triples hold, nothing wraps
__device__ __forceinline__ unsigned long long half_pel_distance(const int (&s)[8], int n, int d) {
    const int ia = (n - 1) >> 1, ib = n >> 1;
    int a = s[0], b = s[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) { a = i == ia ? s[i] : a; b = i == ib ? s[i] : b; }
    const long long r = 2ll * d - ((long long)a + b);
    return (unsigned long long)(r < 0 ? -r : r);
}
}  // namespace

// best: (dx, dy, sad) triples in integer pixels, only dx and dy are read.  keep_in (optional: absent = all ones) must NOT alias out_keep: a
// lane reads its neighbours' bytes.  An unkept or off-lattice neighbour sorts to the end as INT_MAX -- a kept winner that holds INT_MAX
// itself ties with it, and a tie leaves the first n sorted values what they are.  The residual saturates at 2^32 - 1.
__device__ __forceinline__ void sad_median_block(const int* __restrict__ best, const uint8_t* __restrict__ keep_in, int nbx, int nby,
                                                 uint32_t limit2, uint32_t* __restrict__ out_residual2, uint8_t* __restrict__ out_keep) {
    const uint32_t nblk = (uint32_t)nbx * (uint32_t)nby;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= nblk) return;
    const int bx = (int)(k % (uint32_t)nbx), by = (int)(k / (uint32_t)nbx);
    int sx[8], sy[8], n = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int q = j < 4 ? j : j + 1;                    // the 3 x 3 window in raster order without its centre
        const int x = bx + q % 3 - 1, y = by + q / 3 - 1;
        bool valid = x >= 0 && x < nbx && y >= 0 && y < nby;
        size_t kn = 0;
        if (valid) {                                        // the index exists only inside the lattice
            kn = (size_t)y * nbx + x;
            if (keep_in) valid = keep_in[kn] != 0;
        }
        sx[j] = valid ? best[3 * kn] : INT_MAX;
        sy[j] = valid ? best[3 * kn + 1] : INT_MAX;
        n += valid ? 1 : 0;
    }
    sort8(sx); sort8(sy);
    uint32_t r2 = 0;                                        // no kept neighbour: nothing contradicts the block
    if (n > 0) {
        const unsigned long long rx = half_pel_distance(sx, n, best[3 * (size_t)k]), ry = half_pel_distance(sy, n, best[3 * (size_t)k + 1]);
        const unsigned long long r = rx > ry ? rx : ry;
        r2 = r > 0xffffffffull ? 0xffffffffu : (uint32_t)r;
    }
    if (out_residual2) out_residual2[k] = r2;
    if (out_keep) out_keep[k] = r2 < limit2 && (!keep_in || keep_in[k] != 0) ? 1 : 0;
}

// blockIdx.y is the item, every array nbx * nby elements per item.  A neighbour index is formed inside the item's own lattice (x in [0, nbx),
// y in [0, nby)) and never reaches another item's blocks
__global__ __launch_bounds__(256) void sad_median_kernel(const int* __restrict__ best, const uint8_t* __restrict__ keep_in, int nbx, int nby,
                                                         uint32_t limit2, uint32_t* __restrict__ out_residual2, uint8_t* __restrict__ out_keep) {
    const size_t at = (size_t)blockIdx.y * ((size_t)nbx * nby);
    sad_median_block(best + 3 * at, keep_in ? keep_in + at : nullptr, nbx, nby, limit2, out_residual2 ? out_residual2 + at : nullptr,
                     out_keep ? out_keep + at : nullptr);
}

int sad_median_check(ofps_hip_ctx* ctx, int block, int limit, const char* who) {
    OFPS_REQUIRE(ctx, block >= 1 && block <= 64, "%s: block=%d outside [1,64]", who, block);
    OFPS_REQUIRE(ctx, limit >= 1 && limit <= kSadMedianMax, "%s: median limit %d outside [1, %d]", who, limit, kSadMedianMax);
    return OFPS_HIP_OK;
}

int sad_median_flags_device(ofps_hip_ctx* ctx, const int* d_best, const uint8_t* d_keep_in, int W, int H, int block, int limit,
                            uint32_t* d_out_residual2, uint8_t* d_out_keep, hipStream_t st, int items) {
    const int rc = sad_median_check(ctx, block, limit, "sad_median");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1, "sad_median: bad geometry W=%d H=%d", W, H);
    OFPS_REQUIRE(ctx, !d_keep_in || d_keep_in != d_out_keep, "sad_median: the outgoing flags may not alias the incoming ones");
    const int nbx = W / block, nby = H / block;
    if (nbx == 0 || nby == 0) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, (long long)nbx * nby < (1ll << 31), "sad_median: too many blocks");
    OFPS_REQUIRE(ctx, items >= 1 && items <= 65535, "sad_median: %d items", items);
    const size_t nblk = (size_t)nbx * nby;
    hipLaunchKernelGGL(sad_median_kernel, dim3((unsigned)((nblk + 255) / 256), (unsigned)items), dim3(256), 0, st, d_best, d_keep_in, nbx, nby,
                       2u * (uint32_t)limit, d_out_residual2, d_out_keep);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

}  // namespace ofps

extern "C" {

int ofps_hip_sad_median_dev(ofps_hip_ctx* ctx, const void* d_best, const void* d_keep_in, int W, int H, int block, int limit,
                            void* d_out_residual2, void* d_out_keep) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_best, "sad_median_dev: null device pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::sad_median_flags_device(ctx, static_cast<const int*>(d_best), static_cast<const uint8_t*>(d_keep_in), W, H, block, limit,
                                         static_cast<uint32_t*>(d_out_residual2), static_cast<uint8_t*>(d_out_keep), ctx->stream);
}

int ofps_hip_sad_median(ofps_hip_ctx* ctx, const int32_t* best, const uint8_t* keep_in, int W, int H, int block, int limit,
                        uint32_t* out_residual2, uint8_t* out_keep) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, best, "sad_median: null host pointer");
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1, "sad_median: bad geometry W=%d H=%d", W, H);
    int rc = ofps::sad_median_check(ctx, block, limit, "sad_median");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nblk = ofps_hip_sad_block_count(W, H, block);
    if (!nblk) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, nblk < (size_t(1) << 31), "sad_median: too many blocks");
    // [triples][incoming flags] | [residuals][keep bytes]
    const size_t tri = nblk * 3 * sizeof(int32_t);
    auto* d_in = static_cast<char*>(ofps::scratch(ctx, ofps::S_CONS_FWD, tri + nblk));
    auto* d_flags = static_cast<char*>(ofps::scratch(ctx, ofps::S_GATE_FLAGS, ofps::gate_flags_bytes(nblk)));
    if (!d_in || !d_flags) return OFPS_HIP_ENOMEM;
    uint32_t* d_res = ofps::gate_counts(d_flags);
    uint8_t* d_keep = ofps::gate_keep(d_flags, nblk);
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_in, best, tri, hipMemcpyHostToDevice, ctx->stream));
    if (keep_in) OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_in + tri, keep_in, nblk, hipMemcpyHostToDevice, ctx->stream));
    rc = ofps::sad_median_flags_device(ctx, reinterpret_cast<const int*>(d_in), keep_in ? reinterpret_cast<const uint8_t*>(d_in + tri) : nullptr, W, H,
                                       block, limit, out_residual2 ? d_res : nullptr, out_keep ? d_keep : nullptr, ctx->stream);
    if (rc != OFPS_HIP_OK) return rc;
    if (out_residual2) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_residual2, d_res, nblk * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out_keep) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_keep, d_keep, nblk, hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_set_sad_median(ofps_hip_ctx* ctx, int limit) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, limit >= 0 && limit <= ofps::kSadMedianMax, "set_sad_median: %d outside [0, %d]", limit, ofps::kSadMedianMax);
    ctx->opt.sad_median = limit;
    return OFPS_HIP_OK;
}

int ofps_hip_get_sad_median(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.sad_median : OFPS_HIP_EINVAL; }

int ofps_hip_sad_flow_median_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block, int range,
                                 int min_pixels, int limit, int median_limit, void* d_out_entries, void* d_out_best, void* d_out_count) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_prev && d_cur && d_out_entries && d_out_count, "sad_flow_median_dev: null device pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = ofps::sad_median_check(ctx, block, median_limit, "sad_flow");          // (the filter itself takes 0 for "no median test")
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_REQUIRE(ctx, min_pixels >= 0, "sad_flow: contrast gate %d is negative", min_pixels);
    OFPS_REQUIRE(ctx, limit >= 0, "sad_flow: consistency limit %d is negative", limit);
    return ofps::sad_flow_filtered_device(ctx, {static_cast<const uint8_t*>(d_prev), static_cast<const uint8_t*>(d_cur), 0, 0, W, H, stride}, 1, block,
                                          range, {min_pixels, limit, median_limit}, static_cast<float4*>(d_out_entries), static_cast<int*>(d_out_best),
                                          static_cast<uint32_t*>(d_out_count), "sad_flow");
}

}  // extern "C"
