// sad_prefilter.hip -- hip_sad's mean removal (include/ofps_hip.h N1m): F = clamp(v - box mean + 128) of every frame a search reads, so that
// the SAD no longer sees a brightness change between the two frames.  Kernel + the driver sad_pairs_device calls in front of its launches.
//
// sad_prefilter_kernel: one workgroup (256 threads) = a 128 x 32 tile of one frame (grid z), three steps through the LDS:
//   1. stage  the tile and its halo, rows [y0 - r, y0 + 32 + r) x ten 16-byte chunks that cover columns [x0 - r, x0 + 128 + r), every coordinate
//             clamped to the frame BEFORE the address is formed (the replicated border).  A chunk that lies inside the row is one 16-byte load
//             when the source rows are 16-byte aligned, else four dwords (rows 4-byte aligned), else clamped byte loads.  A thread issues all
//             its loads (at most three chunks) before it stores the first to the LDS.
//   2. rows   thread = four adjacent row sums of one staged row: the window's bytes come as dwords, and v_dot4_u32_u8 with a 0/1 byte mask adds
//             the bytes that belong to each of the four windows.  The masks depend on r alone: the host makes them, the scalar unit reads them.
//             32 lanes read 32 consecutive dwords (no bank conflict at any row pitch) and store 32 x 8 bytes of 16-bit sums (k * 255 <= 8415).
//   3. cols   thread = four adjacent pixels of four consecutive rows: the k + 3 rows of sums they need are read once (ds_read_b64: the 32 lanes
//             of a row cover the 64 banks exactly).  The k - 3 rows all four outputs share are added once; the three rows above and below
//             them are combined as packed 16-bit pairs (three rows stay below 2^16).  Mean by multiplier, subtract, clamp, one dword store.
// The division S' / n, S' = S + (n >> 1) < 2^19, is umulhi(S', M) with M = ceil(2^32 / n) = (2^32 + e) / n, 0 <= e < n <= 1089:
// S' * M / 2^32 = S' / n + S' * e / (n * 2^32), and the second term is below 1 / n because S' * e < 2^19 * 2^11 < 2^32 -- it never carries the
// quotient over (tests/test_sad_prefilter_cpu.py walks every S' of every radius).
#include "common.hpp"

namespace {

constexpr int kTileW = 128, kTileH = 32;                 // output pixels per workgroup
constexpr int kRowsPerThread = 4;                        // step 3: 32 x 8 threads, four rows each
constexpr int kMaxR = 16;
constexpr int kChunks = 10;                              // 16-byte chunks per staged row: (sh + 128 + 2r + 15) / 16 with sh = -r mod 16 is 10 for every r in [1, 16]
constexpr int kRawDw = 4 * kChunks;                      // staged dwords per row
constexpr int kRawRows = kTileH + 2 * kMaxR;             // 64
constexpr int kMaxWindowDw = 10;                         // dwords a thread's four windows touch at most: (3 + 33 + 3 + 3) / 4

struct PrefilterParams {
    const uint8_t* src; uint8_t* dst;
    size_t src_pitch, dst_pitch;          // between frames, bytes
    int src_stride, dst_stride;
    int W, H;
    int r, k;                             // radius, window 2r + 1
    uint32_t half_n, mul;                 // n >> 1, ceil(2^32 / n)
    int src_vec, dst_vec;                 // source rows: 16 | 4 | 1-byte aligned; destination rows 4-byte aligned or not
    uint32_t mask[kMaxWindowDw][4];       // [i][q]: byte c of dword i of a thread's window is 1 where q <= 4i + c - (sh & 3) < q + k
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// four bytes of a row from column x on, columns clamped to [0, W): one load where they lie inside the row and the rows are dword aligned
__device__ __forceinline__ uint32_t load4(const uint8_t* line, int x, int W, bool vec4) {
    if (vec4 && x >= 0 && x + 3 < W) return *reinterpret_cast<const uint32_t*>(line + x);
    return (uint32_t)line[clampi(x, 0, W - 1)] | ((uint32_t)line[clampi(x + 1, 0, W - 1)] << 8) |
           ((uint32_t)line[clampi(x + 2, 0, W - 1)] << 16) | ((uint32_t)line[clampi(x + 3, 0, W - 1)] << 24);
}

__device__ __forceinline__ uint2 add2(uint2 a, uint2 b) { return make_uint2(a.x + b.x, a.y + b.y); }    // packed 16-bit pairs that cannot carry

__global__ __launch_bounds__(256) void sad_prefilter_kernel(const PrefilterParams p) {
    __shared__ uint4 raw[kRawRows * kChunks];                    // 10,240 bytes
    __shared__ uint2 sums[kRawRows * (kTileW / 4)];              // 16-bit row sums, four per entry: 16,384 bytes
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const uint8_t* src = p.src + (size_t)blockIdx.z * p.src_pitch;
    uint8_t* dst = p.dst + (size_t)blockIdx.z * p.dst_pitch;
    const int r = p.r, k = p.k, W = p.W, H = p.H;
    const int sh = (16 - (r & 15)) & 15;                         // x0 - r - sh is a multiple of 16: staged chunks are aligned source chunks
    const int xa = x0 - r - sh;                                  // column of the first staged byte (may be negative)
    const int nrows = kTileH + 2 * r;

    // 1. stage: loads first, stores behind them
    uint4 v[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int it = tid + 256 * u;
        if (it < nrows * kChunks) {
            const int row = it / kChunks, c = it - row * kChunks;
            const uint8_t* line = src + (uint32_t)clampi(y0 - r + row, 0, H - 1) * (uint32_t)p.src_stride;
            const int x = xa + 16 * c;
            if (p.src_vec == 16 && x >= 0 && x + 15 < W) v[u] = *reinterpret_cast<const uint4*>(line + x);
            else {
                const bool vec4 = p.src_vec >= 4;
                v[u] = make_uint4(load4(line, x, W, vec4), load4(line, x + 4, W, vec4), load4(line, x + 8, W, vec4), load4(line, x + 12, W, vec4));
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int it = tid + 256 * u;
        if (it < nrows * kChunks) raw[it] = v[u];
    }
    __syncthreads();

    // 2. row sums: a thread's windows start at staged byte 4 * tx + sh and span k + 3 bytes
    const uint32_t* raw_dw = reinterpret_cast<const uint32_t*>(raw);
    const int wdw = ((sh & 3) + k + 3 + 3) >> 2;                 // dwords a thread's four windows touch
    for (int it = tid; it < nrows * (kTileW / 4); it += 256) {
        const uint32_t* in = raw_dw + (it >> 5) * kRawDw + (it & 31) + (sh >> 2);
        uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
#pragma unroll
        for (int i = 0; i < kMaxWindowDw; ++i) {                 // unrolled: the masks stay in scalar registers, the bound is a uniform branch
            if (i < wdw) {
                const uint32_t d = in[i];
                s0 = __builtin_amdgcn_udot4(d, p.mask[i][0], s0, false);
                s1 = __builtin_amdgcn_udot4(d, p.mask[i][1], s1, false);
                s2 = __builtin_amdgcn_udot4(d, p.mask[i][2], s2, false);
                s3 = __builtin_amdgcn_udot4(d, p.mask[i][3], s3, false);
            }
        }
        sums[it] = make_uint2(s0 | (s1 << 16), s2 | (s3 << 16));
    }
    __syncthreads();

    // 3. column sums of output rows 0 .. 3 of the thread; staged sum row j (relative to the thread's first) belongs to output row o iff
    //    o <= j < o + k: rows 3 .. k - 1 to all four, rows 0 .. 2 (e) and k .. k + 2 (t) to some
    const int tx = tid & 31, ty = tid >> 5;
    const int x = x0 + 4 * tx;
    if (x >= W) return;                                          // (no barrier below)
    const uint2* col = sums + (ty * kRowsPerThread) * (kTileW / 4) + tx;
    const uint2 e0 = col[0], e1 = col[kTileW / 4], e2 = col[2 * (kTileW / 4)];
    const uint2 t0 = col[k * (kTileW / 4)], t1 = col[(k + 1) * (kTileW / 4)], t2 = col[(k + 2) * (kTileW / 4)];
    uint32_t common[4] = {p.half_n, p.half_n, p.half_n, p.half_n};
    for (int j = kRowsPerThread - 1; j < k; ++j) {
        const uint2 s = col[j * (kTileW / 4)];
        common[0] += s.x & 0xFFFFu; common[1] += s.x >> 16; common[2] += s.y & 0xFFFFu; common[3] += s.y >> 16;
    }
    const uint2 e12 = add2(e1, e2), t01 = add2(t0, t1);
    const uint2 edge[kRowsPerThread] = {add2(e12, e0), add2(e12, t0), add2(e2, t01), add2(t01, t2)};     // three rows each: < 2^16 per half
    const int centre = (sh + r) >> 2;                            // sh + r is a multiple of 4: the pixels' own dword
#pragma unroll
    for (int o = 0; o < kRowsPerThread; ++o) {
        const int yl = ty * kRowsPerThread + o, y = y0 + yl;
        if (y >= H) break;
        const uint32_t px = raw_dw[(yl + r) * kRawDw + tx + centre];
        const uint32_t sq[4] = {common[0] + (edge[o].x & 0xFFFFu), common[1] + (edge[o].x >> 16), common[2] + (edge[o].y & 0xFFFFu),
                                common[3] + (edge[o].y >> 16)};
        uint32_t out = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = (int)__umulhi(sq[q], p.mul);
            out |= (uint32_t)clampi((int)((px >> (8 * q)) & 0xFFu) - m + 128, 0, 255) << (8 * q);
        }
        uint8_t* o_ptr = dst + (uint32_t)y * (uint32_t)p.dst_stride + x;
        if (p.dst_vec && x + 3 < W) *reinterpret_cast<uint32_t*>(o_ptr) = out;
        else
            for (int q = 0; q < 4 && x + q < W; ++q) o_ptr[q] = (uint8_t)(out >> (8 * q));
    }
}

int prefilter_check(ofps_hip_ctx* ctx, const void* src, const void* dst, int W, int H, int stride, int radius, int dst_stride) {
    OFPS_REQUIRE(ctx, src && dst, "sad_prefilter: null pointer");
    OFPS_REQUIRE(ctx, radius >= 1 && radius <= kMaxR, "sad_prefilter: radius=%d outside [1,%d]", radius, kMaxR);
    OFPS_REQUIRE(ctx, W > 0 && H > 0 && stride >= W && dst_stride >= W, "sad_prefilter: bad geometry W=%d H=%d stride=%d dst_stride=%d", W, H, stride,
                 dst_stride);
    return OFPS_HIP_OK;
}

}  // namespace

namespace ofps {

// `frames` frames of W x H at src + k*src_pitch -> their mean-removed forms at dst + k*dst_pitch, on ctx->stream
int sad_prefilter_device(ofps_hip_ctx* ctx, const uint8_t* src, size_t src_pitch, int W, int H, int src_stride, uint8_t* dst, size_t dst_pitch,
                         int dst_stride, long long frames, int radius) {
    PrefilterParams p{};
    p.src_pitch = src_pitch; p.dst_pitch = dst_pitch; p.src_stride = src_stride; p.dst_stride = dst_stride;
    p.W = W; p.H = H; p.r = radius; p.k = 2 * radius + 1;
    const uint32_t n = (uint32_t)(p.k * p.k);
    p.half_n = n >> 1;
    p.mul = (uint32_t)(((1ull << 32) + n - 1) / n);
    auto aligned = [&](size_t a) { return (uintptr_t)src % a == 0 && src_pitch % a == 0 && (size_t)src_stride % a == 0; };
    p.src_vec = aligned(16) ? 16 : (aligned(4) ? 4 : 1);
    p.dst_vec = (uintptr_t)dst % 4 == 0 && dst_pitch % 4 == 0 && dst_stride % 4 == 0;
    const int sh4 = ((16 - (radius & 15)) & 15) & 3;             // the kernel's window offset inside its first dword
    for (int i = 0; i < kMaxWindowDw; ++i)
        for (int q = 0; q < 4; ++q)
            for (int c = 0; c < 4; ++c) {
                const int j = 4 * i + c - sh4;
                if (j >= q && j < q + p.k) p.mask[i][q] |= 1u << (8 * c);
            }
    OFPS_REQUIRE(ctx, (long long)src_stride * H < (1ll << 31) && (long long)dst_stride * H < (1ll << 31), "sad_prefilter: frame too large");
    const unsigned gx = (unsigned)((W + kTileW - 1) / kTileW), gy = (unsigned)((H + kTileH - 1) / kTileH);
    OFPS_REQUIRE(ctx, gy <= 65535, "sad_prefilter: grid too large");
    for (long long f = 0; f < frames; f += 65535) {              // grid z is the frame
        const long long nz = frames - f < 65535 ? frames - f : 65535;
        p.src = src + (size_t)f * src_pitch; p.dst = dst + (size_t)f * dst_pitch;
        hipLaunchKernelGGL(sad_prefilter_kernel, dim3(gx, gy, (unsigned)nz), dim3(256), 0, ctx->stream, p);
    }
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// Called by sad_pairs_device in front of its launches when the context's sad_prefilter > 0: the two frame sets are filtered into S_SAD_PREF and
// *filtered describes them there (64-byte rows, so the search behind it takes the strip kernel whatever the caller's alignment was).  What
// is filtered and where it lands: SadFrames::sets -- a chain once over pairs + 1 frames, a set with pitch 0 as one frame.  S_SAD_PREF is
// written and read on ctx->stream only, anew by every search, which that stream orders.
int sad_prefilter_pairs_device(ofps_hip_ctx* ctx, int radius, const SadFrames& f, int pairs, SadFrames* filtered) {
    const SadFrames::Sets sets = f.sets(pairs);
    const int fstride = ofps::padded_stride(f.W);
    const size_t fpitch = (size_t)fstride * f.H;
    auto* buf = static_cast<uint8_t*>(scratch(ctx, S_SAD_PREF, (size_t)(sets.nprev + sets.ncur) * fpitch));
    if (!buf) return OFPS_HIP_ENOMEM;
    int rc = sad_prefilter_device(ctx, f.prev_base, f.prev_pitch, f.W, f.H, f.stride, buf, fpitch, fstride, sets.nprev, radius);
    if (rc == OFPS_HIP_OK && !sets.chain)
        rc = sad_prefilter_device(ctx, f.cur_base, f.cur_pitch, f.W, f.H, f.stride, buf + (size_t)sets.cur_first() * fpitch, fpitch, fstride, sets.ncur, radius);
    if (rc == OFPS_HIP_OK) *filtered = sets.in(buf, fpitch, f.W, f.H, fstride);
    return rc;
}

}  // namespace ofps

extern "C" {

int ofps_hip_set_sad_prefilter(ofps_hip_ctx* ctx, int radius) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, radius >= 0 && radius <= ofps::kSadPrefilterMax, "set_sad_prefilter: %d outside [0, %d]", radius, ofps::kSadPrefilterMax);
    ctx->opt.sad_prefilter = radius;
    return OFPS_HIP_OK;
}

int ofps_hip_get_sad_prefilter(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.sad_prefilter : OFPS_HIP_EINVAL; }

int ofps_hip_sad_prefilter_dev(ofps_hip_ctx* ctx, const void* d_src, int W, int H, int stride, int radius, void* d_dst, int dst_stride) {
    if (!ctx) return OFPS_HIP_EINVAL;
    const int rc = prefilter_check(ctx, d_src, d_dst, W, H, stride, radius, dst_stride);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::sad_prefilter_device(ctx, static_cast<const uint8_t*>(d_src), 0, W, H, stride, static_cast<uint8_t*>(d_dst), 0, dst_stride, 1, radius);
}

int ofps_hip_sad_prefilter(ofps_hip_ctx* ctx, const uint8_t* src, int W, int H, int stride, int radius, uint8_t* dst, int dst_stride) {
    if (!ctx) return OFPS_HIP_EINVAL;
    int rc = prefilter_check(ctx, src, dst, W, H, stride, radius, dst_stride);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int ds = ofps::padded_stride(W);                       // both sides repacked to 64-byte rows, so any host stride is accepted
    auto* d_src = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, (size_t)ds * H));
    auto* d_dst = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_SAD_PREF, (size_t)ds * H));
    if (!d_src || !d_dst) return OFPS_HIP_ENOMEM;
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_src, ds, src, stride, W, H, ctx->stream));
    rc = ofps::sad_prefilter_device(ctx, d_src, 0, W, H, ds, d_dst, 0, ds, 1, radius);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpy2DAsync(dst, dst_stride, d_dst, ds, W, H, hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

}  // extern "C"
