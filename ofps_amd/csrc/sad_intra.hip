// sad_intra.hip -- hip_sad's intra test and scene-cut rule (include/ofps_hip.h N1i): a lattice block whose best match costs no less than
// coding the block from itself yields no record -- the encoder's mode decision, with a ratio -- and a frame pair most of whose blocks say so
// yields none at all.  It drops what no other criterion can: content with no counterpart in the previous frame (a scene cut, uncovered
// background, an object that appears, a flash), for which the search still returns the best of its bad matches as a normal record.
//
// Nothing here searches.  This file holds:
// block_activity_kernel: A(k) = sum |p - m| over block k of the RAW current frame, m the block's rounded mean.  Every pixel is read from
//   memory once and both passes -- the sum, then the deviation from m -- run from registers through the packed-byte SAD instruction: the sum
//   as SAD against 0, the deviation as SAD against m replicated into four bytes.
//   Block 8 and 16 (lattice path): a wave covers a 64 x 16 pixel tile whose origin lies on the lattice, a lane 16 bytes of one row (one
//   16-byte load, two 8-byte loads or dword loads, as the alignment of base, stride and pitch allows; bytes otherwise); the rows of a block
//   are summed over the lanes that hold them; one writer per block, plain stores.
//   Any other block size <= 64: one wave per block, a lane holds every 64th pixel of the block packed four to a register; bytes that are no
//   pixel are 0, add nothing to the sum and m each to the deviation, which their number takes off again.
//   Neither path forms an address outside the lattice's pixels: the ragged right and bottom margins belong to no block.
// sad_intra_kernel: a lane takes four blocks of one item (blockIdx.y): SAD of the integer forward winner, activity, incoming flag -> flag, and
//   the item's two counters (candidates, intra among them), summed in LDS and added by one pair of integer atomics per workgroup of 1,024
//   blocks (one per wave cost 40 us at 129,600 blocks: 4,050 atomics on two addresses): the result does not depend on the order.
// sad_cut_kernel: an item whose counters say "cut" loses all its flags, in front of the compaction.  Launched only when the cut rule is on.
#include "common.hpp"

namespace ofps {

namespace {
constexpr int AT_W = 256, AT_H = 16;                        // the lattice path's workgroup tile: four waves side by side, 64 x 16 pixels each

// bytes [0, 8) at p as two dwords.  ALIGN: what p is known to be a multiple of
template <int ALIGN>
__device__ __forceinline__ uint2 load8(const uint8_t* __restrict__ p) {
    if (ALIGN >= 8) return *reinterpret_cast<const uint2*>(p);
    if (ALIGN == 4) { const uint32_t* q = reinterpret_cast<const uint32_t*>(p); return make_uint2(q[0], q[1]); }
    uint32_t a = 0, b = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) { a |= (uint32_t)p[i] << (8 * i); b |= (uint32_t)p[4 + i] << (8 * i); }
    return make_uint2(a, b);
}

// the sum over the lanes that differ in the bits lo .. hi (powers of two) of their number; every lane gets it
__device__ __forceinline__ uint32_t lanes_sum(uint32_t v, int lo, int hi) {
    for (int d = lo; d <= hi; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

__device__ __forceinline__ uint32_t sad2(uint2 d, uint32_t ref, uint32_t acc) {
    return __builtin_amdgcn_sad_u8(d.y, ref, __builtin_amdgcn_sad_u8(d.x, ref, acc));
}
}  // namespace

// blockIdx.z is the item, its frame `pitch` bytes behind the previous item's, its activities nbx * nby behind.  B in {8, 16}.
// Lane l of a wave: row l >> 2 of the tile, bytes [16 * (l & 3), + 16) of it: two halves of 8.  A half is read iff it lies inside the lattice's
// pixels (x + 8 <= nbx * B, y < nby * B), which lie inside the frame.  B = 16: both halves or neither
template <int B, int ALIGN>
__global__ __launch_bounds__(256) void block_activity_kernel(const uint8_t* __restrict__ gray, size_t pitch, int stride, int nbx, int nby,
                                                             uint32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * AT_W + wave * 64 + (lane & 3) * 16, y = blockIdx.y * AT_H + (lane >> 2);
    const size_t item = blockIdx.z;
    const bool row = y < nby * B, v0 = row && x + 8 <= nbx * B, v1 = row && x + 16 <= nbx * B;
    uint2 h0 = make_uint2(0, 0), h1 = make_uint2(0, 0);
    if (v0) {
        const uint8_t* p = gray + item * pitch + (size_t)y * stride + x;
        if (ALIGN == 16 && v1) { const uint4 q = *reinterpret_cast<const uint4*>(p); h0 = make_uint2(q.x, q.y); h1 = make_uint2(q.z, q.w); }
        else { h0 = load8<ALIGN>(p); if (v1) h1 = load8<ALIGN>(p + 8); }
    }
    out += item * (size_t)nbx * nby;
    if (B == 16) {                                            // the block's 16 rows: the lanes with this lane's l & 3
        const uint32_t S = lanes_sum(sad2(h1, 0, sad2(h0, 0, 0)), 4, 32);
        const uint32_t m = ((S + 128) >> 8) * 0x01010101u;
        const uint32_t A = lanes_sum(sad2(h1, m, sad2(h0, m, 0)), 4, 32);
        if (lane < 4 && v1) out[(size_t)(y >> 4) * nbx + (x >> 4)] = A;
    } else {                                                  // two blocks per lane, 8 rows each: the lanes with this lane's l & 3 and l >> 5
        const uint32_t S0 = lanes_sum(sad2(h0, 0, 0), 4, 16), S1 = lanes_sum(sad2(h1, 0, 0), 4, 16);
        const uint32_t m0 = ((S0 + 32) >> 6) * 0x01010101u, m1 = ((S1 + 32) >> 6) * 0x01010101u;
        const uint32_t A0 = lanes_sum(sad2(h0, m0, 0), 4, 16), A1 = lanes_sum(sad2(h1, m1, 0), 4, 16);
        if ((lane & 28) == 0) {
            uint32_t* o = out + (size_t)(y >> 3) * nbx + (x >> 3);
            if (v0) o[0] = A0;
            if (v1) o[1] = A1;
        }
    }
}

// blockIdx.y is the item; wave w of workgroup g: block 4 * g + w.  Pixel i of the block's n = block^2, row-major, lives in lane i & 63, byte
// (i >> 6) & 3 of register i >> 8
__global__ __launch_bounds__(256) void block_activity_any_kernel(const uint8_t* __restrict__ gray, size_t pitch, int stride, int block, int nbx, int nby,
                                                                 uint32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const uint32_t nblk = (uint32_t)nbx * (uint32_t)nby, k = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (k >= nblk) return;                                    // (the whole wave)
    const size_t item = blockIdx.y;
    const int bx = (int)(k % (uint32_t)nbx), by = (int)(k / (uint32_t)nbx), n = block * block;
    const uint8_t* p = gray + item * pitch + (size_t)by * block * stride + (size_t)bx * block;
    uint32_t px[16], S = 0, A = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = (4 * j + b) * 64 + lane;
            if (i < n) { const int yy = i / block, xx = i - yy * block; w |= (uint32_t)p[(size_t)yy * stride + xx] << (8 * b); }
        }
        px[j] = w;
        S = __builtin_amdgcn_sad_u8(w, 0, S);
    }
    S = lanes_sum(S, 1, 32);
    const uint32_t m = (S + (uint32_t)(n >> 1)) / (uint32_t)n;
    // against m in all 64 bytes of the lane; a byte that holds no pixel is 0 and adds |0 - m| = m: taken off again by their number
    const uint32_t mrep = m * 0x01010101u, held = lane < n ? (uint32_t)(n - lane + 63) >> 6 : 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) A = __builtin_amdgcn_sad_u8(px[j], mrep, A);
    A = lanes_sum(A - (64u - held) * m, 1, 32);
    if (lane == 0) out[item * (size_t)nblk + k] = A;
}

// best: (dx, dy, sad) triples, only the SAD is read, as a signed 32-bit number.  keep_in (optional: absent = all ones) may be out_keep.
// counts (optional): [candidates, intra candidates] of the item, zero before the launch
constexpr uint32_t kIntraPerGroup = 1024;                   // blocks per workgroup: four per lane, 256 apart
__global__ __launch_bounds__(256) void sad_intra_kernel(const int* __restrict__ best, const uint32_t* __restrict__ activity, const uint8_t* keep_in,
                                                        uint32_t nblk, uint32_t ratio, uint8_t* out_keep, uint32_t* __restrict__ counts) {
    __shared__ uint32_t group[2];
    const size_t at = (size_t)blockIdx.y * nblk;
    if (threadIdx.x < 2) group[threadIdx.x] = 0;
    __syncthreads();
    uint32_t nc = 0, ni = 0;
#pragma unroll
    for (uint32_t j = 0; j < kIntraPerGroup / 256u; ++j) {
        const uint32_t k = blockIdx.x * kIntraPerGroup + j * 256u + threadIdx.x;
        bool cand = false, intra = false;
        if (k < nblk) {
            cand = !keep_in || keep_in[at + k] != 0;
            intra = 16ll * (long long)best[3 * (at + k) + 2] >= (long long)ratio * (long long)activity[at + k];
            out_keep[at + k] = cand && !intra ? 1 : 0;
        }
        nc += (uint32_t)__popcll(__ballot(cand)); ni += (uint32_t)__popcll(__ballot(cand && intra));
    }
    if (!counts) return;                                      // (the whole grid)
    if ((threadIdx.x & 63) == 0) { atomicAdd(&group[0], nc); atomicAdd(&group[1], ni); }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (group[0]) atomicAdd(&counts[2 * (size_t)blockIdx.y], group[0]);
        if (group[1]) atomicAdd(&counts[2 * (size_t)blockIdx.y + 1], group[1]);
    }
}

// an item is a cut iff 100 * n_intra >= cut * n_cand (no candidate: a cut): its flags are cleared
__global__ __launch_bounds__(256) void sad_cut_kernel(const uint32_t* __restrict__ counts, uint32_t nblk, uint32_t cut, uint8_t* __restrict__ flags) {
    const uint32_t* c = counts + 2 * (size_t)blockIdx.y;
    if (100ull * c[1] < (unsigned long long)cut * c[0]) return;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < nblk) flags[(size_t)blockIdx.y * nblk + k] = 0;
}

int sad_intra_check(ofps_hip_ctx* ctx, int block, int ratio, int cut, const char* who) {
    OFPS_REQUIRE(ctx, block >= 1 && block <= 64, "%s: block=%d outside [1,64]", who, block);
    OFPS_REQUIRE(ctx, ratio >= 1 && ratio <= kSadIntraMax, "%s: intra ratio %d outside [1, %d]", who, ratio, kSadIntraMax);
    OFPS_REQUIRE(ctx, cut >= 0 && cut <= kSadCutMax, "%s: scene cut %d outside [0, %d]", who, cut, kSadCutMax);
    return OFPS_HIP_OK;
}

namespace {
template <int B>
void launch_activity(int align, dim3 grid, hipStream_t st, const uint8_t* d_luma, size_t pitch, int stride, int nbx, int nby, uint32_t* d_out) {
    if (align == 16) hipLaunchKernelGGL((block_activity_kernel<B, 16>), grid, dim3(256), 0, st, d_luma, pitch, stride, nbx, nby, d_out);
    else if (align == 8) hipLaunchKernelGGL((block_activity_kernel<B, 8>), grid, dim3(256), 0, st, d_luma, pitch, stride, nbx, nby, d_out);
    else if (align == 4) hipLaunchKernelGGL((block_activity_kernel<B, 4>), grid, dim3(256), 0, st, d_luma, pitch, stride, nbx, nby, d_out);
    else hipLaunchKernelGGL((block_activity_kernel<B, 1>), grid, dim3(256), 0, st, d_luma, pitch, stride, nbx, nby, d_out);
}
}  // namespace

// frame k lies k * pitch bytes behind d_luma, its activities k * nblk behind d_out; one launch over all `items`
int block_activity_device(ofps_hip_ctx* ctx, const uint8_t* d_luma, size_t pitch, int items, int W, int H, int stride, int block, uint32_t* d_out,
                          hipStream_t st) {
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1 && stride >= W, "block_activity: bad geometry W=%d H=%d stride=%d", W, H, stride);
    OFPS_REQUIRE(ctx, block >= 1 && block <= 64, "block_activity: block=%d outside [1,64]", block);
    OFPS_REQUIRE(ctx, items >= 1 && items <= 65535, "block_activity: %d items", items);
    const int nbx = W / block, nby = H / block;
    if (nbx == 0 || nby == 0) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, (long long)nbx * nby * items < (1ll << 31), "block_activity: too many blocks");
    if (block == 8 || block == 16) {
        // every load address is base + item * pitch + y * stride + a multiple of 8 (of 16 for the 16-byte load)
        const size_t bits = reinterpret_cast<size_t>(d_luma) | (size_t)stride | (items > 1 ? pitch : 0);
        const int align = bits % 16 == 0 ? 16 : bits % 8 == 0 ? 8 : bits % 4 == 0 ? 4 : 1;
        const dim3 grid((nbx * block + AT_W - 1) / AT_W, (nby * block + AT_H - 1) / AT_H, items);
        if (block == 16) launch_activity<16>(align, grid, st, d_luma, pitch, stride, nbx, nby, d_out);
        else launch_activity<8>(align, grid, st, d_luma, pitch, stride, nbx, nby, d_out);
    } else {
        const size_t nblk = (size_t)nbx * nby;
        hipLaunchKernelGGL(block_activity_any_kernel, dim3((unsigned)((nblk + 3) / 4), (unsigned)items), dim3(256), 0, st, d_luma, pitch, stride, block,
                           nbx, nby, d_out);
    }
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

int sad_intra_flags_device(ofps_hip_ctx* ctx, const int* d_best, const uint32_t* d_activity, const uint8_t* d_keep_in, int W, int H, int block,
                           int ratio, uint8_t* d_out_keep, uint32_t* d_counts, hipStream_t st, int items, bool zero_counts) {
    const int rc = sad_intra_check(ctx, block, ratio, 0, "sad_intra");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1, "sad_intra: bad geometry W=%d H=%d", W, H);
    OFPS_REQUIRE(ctx, items >= 1 && items <= 65535, "sad_intra: %d items", items);
    if (d_counts && zero_counts) OFPS_HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, (size_t)items * 2 * sizeof(uint32_t), st));
    const int nbx = W / block, nby = H / block;
    if (nbx == 0 || nby == 0) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, (long long)nbx * nby < (1ll << 31), "sad_intra: too many blocks");
    const size_t nblk = (size_t)nbx * nby;
    hipLaunchKernelGGL(sad_intra_kernel, dim3((unsigned)((nblk + kIntraPerGroup - 1) / kIntraPerGroup), (unsigned)items), dim3(256), 0, st, d_best, d_activity, d_keep_in,
                       (uint32_t)nblk, (uint32_t)ratio, d_out_keep, d_counts);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

int sad_cut_device(ofps_hip_ctx* ctx, const uint32_t* d_counts, size_t nblk, int cut, uint8_t* d_flags, hipStream_t st, int items) {
    if (cut <= 0 || nblk == 0) return OFPS_HIP_OK;
    hipLaunchKernelGGL(sad_cut_kernel, dim3((unsigned)((nblk + 255) / 256), (unsigned)items), dim3(256), 0, st, d_counts, (uint32_t)nblk, (uint32_t)cut,
                       d_flags);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

}  // namespace ofps

extern "C" {

int ofps_hip_block_activity_dev(ofps_hip_ctx* ctx, const void* d_luma, int W, int H, int stride, int block, void* d_out_activity) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_luma && d_out_activity, "block_activity_dev: null device pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::block_activity_device(ctx, static_cast<const uint8_t*>(d_luma), 0, 1, W, H, stride, block, static_cast<uint32_t*>(d_out_activity),
                                       ctx->stream);
}

int ofps_hip_block_activity(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride, int block, uint32_t* out_activity) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, luma && out_activity, "block_activity: null host pointer");
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1 && stride >= W, "block_activity: bad geometry W=%d H=%d stride=%d", W, H, stride);
    OFPS_REQUIRE(ctx, block >= 1 && block <= 64, "block_activity: block=%d outside [1,64]", block);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nblk = ofps_hip_sad_block_count(W, H, block);
    if (!nblk) return OFPS_HIP_OK;
    const int dstride = (W + 15) & ~15;                       // repacked: any host stride is accepted, every row is aligned
    auto* d_gray = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, (size_t)dstride * H));
    auto* d_act = static_cast<uint32_t*>(ofps::scratch(ctx, ofps::S_INTRA, nblk * sizeof(uint32_t)));
    if (!d_gray || !d_act) return OFPS_HIP_ENOMEM;
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_gray, dstride, luma, stride, W, H, ctx->stream));
    const int rc = ofps::block_activity_device(ctx, d_gray, 0, 1, W, H, dstride, block, d_act, ctx->stream);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_activity, d_act, nblk * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_sad_intra_dev(ofps_hip_ctx* ctx, const void* d_best, const void* d_activity, const void* d_keep_in, int W, int H, int block, int ratio,
                           int cut, void* d_out_keep, void* d_out_counts) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_best && d_activity && d_out_keep, "sad_intra_dev: null device pointer");
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1, "sad_intra_dev: bad geometry W=%d H=%d", W, H);
    int rc = ofps::sad_intra_check(ctx, block, ratio, cut, "sad_intra_dev");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto* d_counts = static_cast<uint32_t*>(d_out_counts);
    if (!d_counts && cut > 0) {                               // the cut rule reads the counters whether the caller wants them or not
        d_counts = static_cast<uint32_t*>(ofps::scratch(ctx, ofps::S_RESULT, 2 * sizeof(uint32_t)));
        if (!d_counts) return OFPS_HIP_ENOMEM;
    }
    rc = ofps::sad_intra_flags_device(ctx, static_cast<const int*>(d_best), static_cast<const uint32_t*>(d_activity),
                                      static_cast<const uint8_t*>(d_keep_in), W, H, block, ratio, static_cast<uint8_t*>(d_out_keep), d_counts, ctx->stream);
    if (rc != OFPS_HIP_OK) return rc;
    return ofps::sad_cut_device(ctx, d_counts, ofps_hip_sad_block_count(W, H, block), cut, static_cast<uint8_t*>(d_out_keep), ctx->stream);
}

int ofps_hip_sad_intra(ofps_hip_ctx* ctx, const int32_t* best, const uint32_t* activity, const uint8_t* keep_in, int W, int H, int block, int ratio,
                       int cut, uint8_t* out_keep, uint32_t* out_counts) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, best && activity && out_keep, "sad_intra: null host pointer");
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1, "sad_intra: bad geometry W=%d H=%d", W, H);
    int rc = ofps::sad_intra_check(ctx, block, ratio, cut, "sad_intra");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nblk = ofps_hip_sad_block_count(W, H, block);
    if (out_counts) out_counts[0] = out_counts[1] = 0;
    if (!nblk) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, nblk < (size_t(1) << 31), "sad_intra: too many blocks");
    // [triples][activities][incoming flags] | [counters][keep bytes]
    const size_t tri = nblk * 3 * sizeof(int32_t), act = nblk * sizeof(uint32_t);
    auto* d_in = static_cast<char*>(ofps::scratch(ctx, ofps::S_CONS_FWD, tri + act + nblk));
    auto* d_flags = static_cast<char*>(ofps::scratch(ctx, ofps::S_GATE_FLAGS, ofps::gate_flags_bytes(nblk)));
    if (!d_in || !d_flags) return OFPS_HIP_ENOMEM;
    uint32_t* d_counts = ofps::gate_counts(d_flags);
    uint8_t* d_keep = ofps::gate_keep(d_flags, nblk);
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_in, best, tri, hipMemcpyHostToDevice, ctx->stream));
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_in + tri, activity, act, hipMemcpyHostToDevice, ctx->stream));
    if (keep_in) OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_in + tri + act, keep_in, nblk, hipMemcpyHostToDevice, ctx->stream));
    rc = ofps::sad_intra_flags_device(ctx, reinterpret_cast<const int*>(d_in), reinterpret_cast<const uint32_t*>(d_in + tri),
                                      keep_in ? reinterpret_cast<const uint8_t*>(d_in + tri + act) : nullptr, W, H, block, ratio, d_keep, d_counts,
                                      ctx->stream);
    if (rc == OFPS_HIP_OK) rc = ofps::sad_cut_device(ctx, d_counts, nblk, cut, d_keep, ctx->stream);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_keep, d_keep, nblk, hipMemcpyDeviceToHost, ctx->stream));
    if (out_counts) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_counts, d_counts, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_set_sad_intra(ofps_hip_ctx* ctx, int ratio) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, ratio >= 0 && ratio <= ofps::kSadIntraMax, "set_sad_intra: %d outside [0, %d]", ratio, ofps::kSadIntraMax);
    ctx->opt.sad_intra = ratio;
    return OFPS_HIP_OK;
}

int ofps_hip_get_sad_intra(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.sad_intra : OFPS_HIP_EINVAL; }

int ofps_hip_set_sad_cut(ofps_hip_ctx* ctx, int percent) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, percent >= 0 && percent <= ofps::kSadCutMax, "set_sad_cut: %d outside [0, %d]", percent, ofps::kSadCutMax);
    ctx->opt.sad_cut = percent;
    return OFPS_HIP_OK;
}

int ofps_hip_get_sad_cut(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.sad_cut : OFPS_HIP_EINVAL; }

int ofps_hip_sad_flow_intra_dev(ofps_hip_ctx* ctx, const void* d_frames, int n_frames, int W, int H, int stride, size_t frame_pitch, int ref_mode,
                                int block, int range, int min_pixels, int limit, int median, int intra, int cut, void* d_out_entries,
                                void* d_out_best, void* d_out_counts) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_frames && d_out_entries && d_out_counts, "sad_flow_intra_dev: null device pointer");
    OFPS_REQUIRE(ctx, n_frames >= 2, "sad_flow_intra_dev: need at least 2 frames (got %d)", n_frames);
    OFPS_REQUIRE(ctx, W > 0 && H > 0 && stride >= W, "sad_flow_intra_dev: bad geometry W=%d H=%d stride=%d", W, H, stride);
    OFPS_REQUIRE(ctx, frame_pitch >= (size_t)stride * (size_t)H, "sad_flow_intra_dev: frame_pitch smaller than a frame");
    OFPS_REQUIRE(ctx, ref_mode == 0 || ref_mode == 1, "sad_flow_intra_dev: ref_mode must be 0 or 1");
    OFPS_REQUIRE(ctx, min_pixels >= 0, "sad_flow_intra_dev: contrast gate %d is negative", min_pixels);
    OFPS_REQUIRE(ctx, limit >= 0, "sad_flow_intra_dev: consistency limit %d is negative", limit);
    OFPS_REQUIRE(ctx, median >= 0, "sad_flow_intra_dev: median limit %d is negative", median);
    const int rc = ofps::sad_intra_check(ctx, block, intra, cut, "sad_flow_intra_dev");       // (the filter itself takes 0 for "no intra test")
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::sad_flow_filtered_device(ctx, ofps::SadFrames::sequence(static_cast<const uint8_t*>(d_frames), frame_pitch, ref_mode, W, H, stride),
                                          n_frames - 1, block, range, {min_pixels, limit, median, intra, cut}, static_cast<float4*>(d_out_entries),
                                          static_cast<int*>(d_out_best), static_cast<uint32_t*>(d_out_counts), "sad_flow_intra_dev");
}

}  // extern "C"
