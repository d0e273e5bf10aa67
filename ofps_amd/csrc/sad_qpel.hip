// sad_qpel.hip -- N1q: quarter-pel refinement of the SAD block matcher's integer winners (motion_scale 4).
//
// Spec: include/ofps_hip.h / DESIGN.md "N1q".  For every block the 49 displacements D = 4*d + f, f in [-3,3]^2 (quarter-pel
// units) around the integer winner d are compared on SAD against the previous frame sampled with H.264's luma interpolation
// (ITU-T H.264 8.4.2.2.1: six-tap half-pel samples, bilinear quarter-pel samples, frame edges replicated); the winner is the
// minimum of (SAD, Dx^2+Dy^2, Dy+4R+3, Dx+4R+3).  All-integer arithmetic: bit-exact against tests/indep_sad_qpel.py.
//
// Kernel shape (sad_qpel_kernel): one wave per block, the waves of a workgroup are independent (no workgroup barrier).
//   0. the (B+6)^2 integer window around the winner -> LDS, coordinates clamped to the frame (= edge replication); the
//      block of the current frame -> LDS;
//   1. b1 = the unrounded horizontal six-tap sums of every window row (int16: |b1| <= 10,710);
//   2. the half-pel grid of the window, (2B+3)^2 samples: integer samples, b = clip((b1+16)>>5), h the same down the columns,
//      j = clip((six taps down the b1 columns + 512) >> 10).  It is stored de-interleaved by the parity of its x coordinate,
//      so the samples that four horizontally adjacent pixels of one candidate need are four adjacent bytes;
//   3. lane = candidate (49 of 64 lanes).  Every quarter-pel sample is (p + q + 1) >> 1 of two half-grid samples whose offsets
//      from the pixel depend on f only (p = q on the half grid itself), so a lane walks the block with two fixed offsets:
//      per row B/4+1 dwords of each, v_alignbyte to the lane's byte phase, the rounded byte average of four samples at
//      once ((p|q) - (((p^q)>>1) & 0x7f7f7f7f)), v_sad_u8 against the row of the current block (a broadcast LDS read);
//   4. the 64-bit key's minimum over the wave (xor butterfly); lane 0 writes the record.
// Block sizes 8 and 16 are templates (packed path); any other block <= 64 runs the same phases with a byte-wise phase 3.
#include "common.hpp"

namespace {

struct QpelParams {
    const uint8_t* prev_base;   // pair k: prev = prev_base + k*prev_pitch, cur = cur_base + k*cur_pitch
    const uint8_t* cur_base;
    size_t prev_pitch, cur_pitch;
    int W, H, stride;
    int nbx, nby, B, R;
    long long total;            // blocks of the whole batch
    float nx, ny;
    float4* out_entries;
    const int* in_best;         // integer winners (dx, dy, sad) of the search
    int* out_best;              // (Dx, Dy, SAD) in quarter-pel units; may be null, may alias in_best
};

// LDS layout of one wave, in bytes
__host__ __device__ constexpr int q_iw(int B) { return B + 6; }                  // side of the integer window
__host__ __device__ constexpr int q_hw(int B) { return B + 1; }                  // half-pel columns of b1
__host__ __device__ constexpr int q_ps(int B) { return (B + 4 + 3) & ~3; }       // bytes of one parity plane's row (packed reads run to B+3)
__host__ __device__ constexpr int q_rows(int B) { return 2 * B + 3; }            // rows of the half-pel grid
__host__ __device__ constexpr int q_off_b1(int B) { return (q_iw(B) * q_iw(B) + 3) & ~3; }
__host__ __device__ constexpr int q_off_hg(int B) { return q_off_b1(B) + ((q_iw(B) * q_hw(B) * 2 + 3) & ~3); }
__host__ __device__ constexpr int q_off_cur(int B) { return q_off_hg(B) + q_rows(B) * 2 * q_ps(B); }
__host__ __device__ constexpr int q_wave_bytes(int B) { return (q_off_cur(B) + ((B * B + 3) & ~3) + 15) & ~15; }
static_assert(q_wave_bytes(64) <= 64 * 1024, "the generic form keeps one wave's planes in the default LDS allocation");

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int mask) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = __shfl_xor(lo, mask, 64);
    hi = __shfl_xor(hi, mask, 64);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint8_t clip255(int v) { return (uint8_t)clampi(v, 0, 255); }

template <typename T>
__device__ __forceinline__ int tap6(const T* s, int step) {
    return (int)s[0] - 5 * (int)s[step] + 20 * (int)s[2 * step] + 20 * (int)s[3 * step] - 5 * (int)s[4 * step] + (int)s[5 * step];
}

// half-grid offsets (in half-pel units, relative to the pixel) of the two samples a quarter-pel phase averages
__device__ __forceinline__ void phase_offsets(int fx, int fy, int& pox, int& poy, int& qox, int& qoy) {
    const bool ox = fx & 1, oy = fy & 1;
    if (!ox && !oy) { pox = qox = fx >> 1; poy = qoy = fy >> 1; }
    else if (ox && !oy) { pox = (fx - 1) >> 1; qox = (fx + 1) >> 1; poy = qoy = fy >> 1; }
    else if (!ox) { pox = qox = fx >> 1; poy = (fy - 1) >> 1; qoy = (fy + 1) >> 1; }
    else {
        // of the four surrounding half-grid points the two that are half-pel in exactly one direction: the diagonal whose
        // coordinates have an odd sum (H.264's e, g, p, r)
        const int xa = (fx - 1) >> 1, ya = (fy - 1) >> 1;
        if ((xa + ya) & 1) { pox = xa; poy = ya; qox = xa + 1; qoy = ya + 1; }
        else { pox = xa + 1; poy = ya; qox = xa; qoy = ya + 1; }
    }
}

template <int BT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void sad_qpel_kernel(const QpelParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t q_lds[];
    const int B = BT ? BT : p.B;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const long long k = (long long)blockIdx.x * WAVES + wave;
    if (k >= p.total) return;
    const int per_pair = p.nbx * p.nby;
    const int pair = (int)(k / per_pair);
    const int rem = (int)(k - (long long)pair * per_pair);
    const int by = rem / p.nbx, bx = rem - by * p.nbx;
    const int x0 = bx * B, y0 = by * B;
    const uint8_t* __restrict__ prev = p.prev_base + (size_t)pair * p.prev_pitch;
    const uint8_t* __restrict__ cur = p.cur_base + (size_t)pair * p.cur_pitch;
    const int dx = __builtin_amdgcn_readfirstlane(p.in_best[3 * k + 0]);
    const int dy = __builtin_amdgcn_readfirstlane(p.in_best[3 * k + 1]);

    uint8_t* win = q_lds + (size_t)wave * q_wave_bytes(B);
    int16_t* b1 = reinterpret_cast<int16_t*>(win + q_off_b1(B));
    uint8_t* hg = win + q_off_hg(B);
    uint8_t* cl = win + q_off_cur(B);
    const int IW = q_iw(B), HW = q_hw(B), PS = q_ps(B);

    // ---- 0. integer window (clamped = edge-replicated) and the current block
    for (int i = lane; i < IW * IW; i += 64) {
        const int wy = i / IW, wx = i - wy * IW;
        const int gx = clampi(x0 + dx - 3 + wx, 0, p.W - 1), gy = clampi(y0 + dy - 3 + wy, 0, p.H - 1);
        win[i] = prev[(size_t)gy * p.stride + gx];
    }
    if constexpr (BT != 0) {
        constexpr int BW = BT / 4;
        for (int i = lane; i < BT * BW; i += 64) {
            const int y = i / BW, q = i - y * BW;
            reinterpret_cast<uint32_t*>(cl)[i] = *reinterpret_cast<const uint32_t*>(cur + (size_t)(y0 + y) * p.stride + x0 + 4 * q);
        }
    } else {
        for (int i = lane; i < B * B; i += 64) {
            const int y = i / B, x = i - y * B;
            cl[i] = cur[(size_t)(y0 + y) * p.stride + x0 + x];
        }
    }
    wave_sync();

    // ---- 1. b1[wy][hx]: six taps over window columns hx .. hx+5 (the half sample between window columns hx+2 and hx+3)
    for (int i = lane; i < IW * HW; i += 64) {
        const int wy = i / HW, hx = i - wy * HW;
        b1[i] = (int16_t)tap6(win + wy * IW + hx, 1);
    }
    wave_sync();

    // ---- 2. half-pel grid, index (Y2, X2) in [0, 2B+2]^2 = half-pel position (Y2 - 2, X2 - 2) from the displaced block's origin;
    // row Y2 holds two planes: even X2 (B+2 samples), then odd X2 (B+1 samples)
    {
        const int NE = B + 2, NO = B + 1;
        auto at = [&](int Y2, int X2) -> uint8_t& { return hg[(Y2 * 2 + (X2 & 1)) * PS + (X2 >> 1)]; };
        for (int i = lane; i < NE * NE; i += 64) {                   // integer samples
            const int iy = i / NE, ix = i - iy * NE;
            at(2 * iy, 2 * ix) = win[(iy + 2) * IW + ix + 2];
        }
        for (int i = lane; i < NE * NO; i += 64) {                   // b: half-pel in x
            const int iy = i / NO, ix = i - iy * NO;
            at(2 * iy, 2 * ix + 1) = clip255(((int)b1[(iy + 2) * HW + ix] + 16) >> 5);
        }
        for (int i = lane; i < NO * NE; i += 64) {                   // h: half-pel in y
            const int iy = i / NE, ix = i - iy * NE;
            at(2 * iy + 1, 2 * ix) = clip255((tap6(win + iy * IW + ix + 2, IW) + 16) >> 5);
        }
        for (int i = lane; i < NO * NO; i += 64) {                   // j: half-pel in both, from the unrounded b1
            const int iy = i / NO, ix = i - iy * NO;
            at(2 * iy + 1, 2 * ix + 1) = clip255((tap6(b1 + iy * HW + ix, HW) + 512) >> 10);
        }
    }
    wave_sync();

    // ---- 3. lane = candidate
    const int cand = lane < 49 ? lane : 48;
    const int fy = cand / 7 - 3, fx = cand - (cand / 7) * 7 - 3;
    int pox, poy, qox, qoy;
    phase_offsets(fx, fy, pox, poy, qox, qoy);
    const int prow = ((poy + 2) * 2 + (pox & 1)) * PS, qrow = ((qoy + 2) * 2 + (qox & 1)) * PS;    // plane row of pixel row 0
    const int pk = (pox + 2) >> 1, qk = (qox + 2) >> 1;                                              // byte of pixel column 0
    uint32_t sad = 0;
    if constexpr (BT != 0) {
        constexpr int BW = BT / 4;
        const uint32_t* pp = reinterpret_cast<const uint32_t*>(hg + prow);
        const uint32_t* qp = reinterpret_cast<const uint32_t*>(hg + qrow);
        const uint32_t* cp = reinterpret_cast<const uint32_t*>(cl);
        const int RS = PS;                                            // dwords between pixel rows: two grid rows of two planes
#pragma unroll
        for (int y = 0; y < BT; ++y) {
            uint32_t a[BW + 1], b[BW + 1];
#pragma unroll
            for (int g = 0; g <= BW; ++g) { a[g] = pp[y * RS + g]; b[g] = qp[y * RS + g]; }
#pragma unroll
            for (int g = 0; g < BW; ++g) {
                const uint32_t pa = __builtin_amdgcn_alignbyte(a[g + 1], a[g], (uint32_t)pk);
                const uint32_t qb = __builtin_amdgcn_alignbyte(b[g + 1], b[g], (uint32_t)qk);
                const uint32_t avg = (pa | qb) - (((pa ^ qb) >> 1) & 0x7F7F7F7Fu);     // (p + q + 1) >> 1, four bytes at once
                sad = __builtin_amdgcn_sad_u8(avg, cp[y * BW + g], sad);
            }
        }
    } else {
        const uint8_t* pp = hg + prow + pk;
        const uint8_t* qp = hg + qrow + qk;
        for (int y = 0; y < B; ++y)
            for (int x = 0; x < B; ++x) {
                const int s = ((int)pp[y * 4 * PS + x] + (int)qp[y * 4 * PS + x] + 1) >> 1;
                const int d = (int)cl[y * B + x] - s;
                sad += (uint32_t)(d < 0 ? -d : d);
            }
    }

    // ---- 4. key = (SAD, Dx^2 + Dy^2, Dy + 4R + 3, Dx + 4R + 3): 24 + 20 + 10 + 10 bits (B <= 64, R <= 127)
    const int Dx = 4 * dx + fx, Dy = 4 * dy + fy;
    const bool valid = lane < 49 && 4 * x0 + Dx >= 0 && 4 * (x0 + B - 1) + Dx <= 4 * (p.W - 1) && 4 * y0 + Dy >= 0 &&
                       4 * (y0 + B - 1) + Dy <= 4 * (p.H - 1);
    const int bias = 4 * p.R + 3;
    unsigned long long best = ~0ull;
    if (valid)
        best = ((unsigned long long)sad << 40) | ((unsigned long long)(uint32_t)(Dx * Dx + Dy * Dy) << 20) |
               ((unsigned long long)(uint32_t)(Dy + bias) << 10) | (unsigned long long)(uint32_t)(Dx + bias);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = shfl_xor_u64(best, m);
        best = o < best ? o : best;
    }
    if (lane == 0) {
        const int bsad = (int)(best >> 40);
        const int bDy = (int)((best >> 10) & 1023) - bias, bDx = (int)(best & 1023) - bias;
        const int cx = x0 + B / 2, cy = y0 + B / 2;
        float4 e;
        e.x = ((float)(4 * cx + bDx) * 0.25f) * p.nx;
        e.y = ((float)(4 * cy + bDy) * 0.25f) * p.ny;
        e.z = ((float)bDx / 4.0f) * (-p.nx);
        e.w = ((float)bDy / 4.0f) * (-p.ny);
        p.out_entries[k] = e;
        if (p.out_best) {
            p.out_best[3 * k + 0] = bDx;
            p.out_best[3 * k + 1] = bDy;
            p.out_best[3 * k + 2] = bsad;
        }
    }
}

template <int BT, int WAVES>
void launch_qpel(const QpelParams& p, hipStream_t s) {
    const unsigned nwg = (unsigned)((p.total + WAVES - 1) / WAVES);
    hipLaunchKernelGGL((sad_qpel_kernel<BT, WAVES>), dim3(nwg), dim3(64 * WAVES), (size_t)WAVES * q_wave_bytes(p.B), s, p);
}

}  // namespace

namespace ofps {
// Enqueued by sad_pairs_device behind the integer search when the context's motion scale is 4.  d_in_best: the search's
// (dx, dy, sad); d_out_best: null, or where (Dx, Dy, SAD) go (may be d_in_best itself).
int sad_qpel_refine_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int block, int range, void* d_entries, const void* d_in_best,
                           void* d_out_best) {
    OFPS_REQUIRE(ctx, block >= 1 && block <= 64 && range >= 0 && range <= kSadHierMaxReach, "sad_qpel: block=%d range=%d outside [1,64]/[0,127]",
                 block, range);                 // range above 64: the reach of a search over levels (sad_hier.hip); the key's fields hold 8 * 127 + 6
    OFPS_REQUIRE(ctx, d_entries && d_in_best, "sad_qpel: null device pointer");
    QpelParams p{};
    p.prev_base = f.prev_base; p.cur_base = f.cur_base;
    p.prev_pitch = f.prev_pitch; p.cur_pitch = f.cur_pitch;
    p.W = f.W; p.H = f.H; p.stride = f.stride;
    p.nbx = f.W / block; p.nby = f.H / block; p.B = block; p.R = range;
    p.total = (long long)p.nbx * p.nby * pairs;
    p.nx = 1.0f / (float)f.W; p.ny = 1.0f / (float)f.H;
    p.out_entries = static_cast<float4*>(d_entries);
    p.in_best = static_cast<const int*>(d_in_best);
    p.out_best = static_cast<int*>(d_out_best);
    if (p.total <= 0) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, p.total < (1ll << 31), "sad_qpel: grid too large");
    // the packed forms read the current block by dwords: rows 4-byte aligned (sad_pairs_device requires it)
    if (block == 16) launch_qpel<16, 4>(p, ctx->stream);
    else if (block == 8) launch_qpel<8, 4>(p, ctx->stream);
    else launch_qpel<0, 1>(p, ctx->stream);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}
}  // namespace ofps

extern "C" {

int ofps_hip_set_sad_motion_scale(ofps_hip_ctx* ctx, int scale) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, scale == 1 || scale == 4, "set_sad_motion_scale: %d is not 1 (full-pel) or 4 (quarter-pel)", scale);
    ctx->opt.sad_motion_scale = scale;
    return OFPS_HIP_OK;
}

int ofps_hip_get_sad_motion_scale(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.sad_motion_scale : OFPS_HIP_EINVAL; }

}  // extern "C"
