// sad_hier.hip -- N1h: hip_sad's search levels.  Coarse-to-fine search for motion beyond the search range.
//
// Spec: include/ofps_hip.h / DESIGN.md "N1h".  The frames are halved levels - 1 times (2 x 2 box, rounded), the plain search (sad.hip, its
// kernels unchanged) runs on the top pair, and every finer level repairs the doubled winners of its parent lattice in a +-3 window:
// 49 candidates per block against (2R + 1)^2.  All-integer, bit-exact against tests/indep_sad_hier.py.
//
// sad_down2_kernel: one thread = four output pixels of one frame of the batch: two 8-byte row loads, one dword store when the rows are
//   8-byte aligned (every level the driver makes is), bytes otherwise (ofps_hip_sad_down2 takes any stride).
// sad_hier_refine_kernel: the shape of sad_qpel_kernel without its interpolation: one wave per block, the waves of a workgroup independent.
//   0. parent winner -> predictor, clamped to the frame (wave-uniform); the (B+6)^2 window of prev around it and the B^2 block of cur -> LDS.
//      Window positions outside the frame belong to invalid candidates only: their loads are clamped to the frame;
//   1. lane = candidate (49 of 64 lanes): B rows of B/4 + 1 window dwords, v_alignbyte to the lane's byte phase, v_sad_u8 against the row of
//      the current block (a broadcast LDS read).  The window's row pitch is B + 8 bytes: the 14 distinct dwords the lanes of one read touch
//      -- 7 rows x 2 dword columns, 6 (B 16) or 4 (B 8) dwords apart -- lie on 14 different banks;
//   2. the 64-bit key's minimum over the wave (xor butterfly); lane 0 writes the triple and, at level 0, the record.
// Block sizes 8 and 16 are templates (packed path); any other block <= 64 runs the same phases byte-wise.
#include "common.hpp"

namespace {

using ofps::SadFrames;

struct RefineParams {
    SadFrames f;                    // one level of one search's two frame sets
    int nbx, nby, B;                // this level's lattice
    int pnbx, pnby;                 // the parent lattice
    long long total;                // blocks of the whole batch
    float nx, ny;
    const int* parent_best;         // (dx, dy, sad) per parent block, pair after pair
    int* out_best;                  // (dx, dy, sad) per block; may be null at level 0
    float4* out_entries;            // level 0 only: the records in N1's convention; else null
};

struct Down2Params {
    const uint8_t* src; uint8_t* dst;
    size_t src_pitch, dst_pitch;    // between the frames of the batch
    int src_stride, dst_stride;
    int Wo, Ho, cols4;              // the output's size; cols4 = ceil(Wo / 4) threads per row
    long long total;                // threads with work: frames * Ho * cols4
    int vec;                        // rows of both sides are aligned for the 8-byte loads and the dword store
};

__host__ __device__ constexpr int h_ws(int B) { return B + 8; }                    // bytes of one window row (B + 6 used; packed reads run to B + 8)
__host__ __device__ constexpr int h_off_cur(int B) { return ((B + 6) * h_ws(B) + 3) & ~3; }
__host__ __device__ constexpr int h_wave_bytes(int B) { return (h_off_cur(B) + ((B * B + 3) & ~3) + 15) & ~15; }
static_assert(h_wave_bytes(64) <= 16 * 1024, "one wave's window and block");

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

__global__ __launch_bounds__(256) void sad_down2_kernel(const Down2Params p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.total) return;
    const long long row = t / p.cols4;                      // (frame, y)
    const int x = (int)(t - row * p.cols4) * 4;
    const long long frame = row / p.Ho;
    const int y = (int)(row - frame * p.Ho);
    const uint8_t* __restrict__ s0 = p.src + (size_t)frame * p.src_pitch + (size_t)(2 * y) * p.src_stride + 2 * x;
    const uint8_t* __restrict__ s1 = s0 + p.src_stride;
    uint8_t* __restrict__ d = p.dst + (size_t)frame * p.dst_pitch + (size_t)y * p.dst_stride + x;
    if (p.vec && x + 4 <= p.Wo) {                            // source columns 2x .. 2x + 7 <= 2 * Wo - 1 < W
        const uint2 a = *reinterpret_cast<const uint2*>(s0), b = *reinterpret_cast<const uint2*>(s1);
        // per 16-bit lane: the sum of a row's two bytes (<= 510); two rows + 2 <= 1022, >> 2 in place
        const uint32_t lo = (a.x & 0x00FF00FFu) + ((a.x >> 8) & 0x00FF00FFu) + (b.x & 0x00FF00FFu) + ((b.x >> 8) & 0x00FF00FFu) + 0x00020002u;
        const uint32_t hi = (a.y & 0x00FF00FFu) + ((a.y >> 8) & 0x00FF00FFu) + (b.y & 0x00FF00FFu) + ((b.y >> 8) & 0x00FF00FFu) + 0x00020002u;
        const uint32_t l2 = (lo >> 2) & 0x00FF00FFu, h2 = (hi >> 2) & 0x00FF00FFu;
        *reinterpret_cast<uint32_t*>(d) = (l2 & 0xFFu) | ((l2 >> 8) & 0xFF00u) | ((h2 & 0xFFu) << 16) | ((h2 >> 16) << 24);
    } else {
        for (int i = 0; i < 4 && x + i < p.Wo; ++i)
            d[i] = (uint8_t)(((int)s0[2 * i] + (int)s0[2 * i + 1] + (int)s1[2 * i] + (int)s1[2 * i + 1] + 2) >> 2);
    }
}

template <int BT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void sad_hier_refine_kernel(const RefineParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t h_lds[];
    constexpr int E = ofps::kSadHierRefine, N = 2 * E + 1;
    static_assert(N * N <= 64 && E == 3, "lane = candidate; the window's margins and row pitch are written for radius 3");
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
    const uint8_t* __restrict__ prev = p.f.prev_base + (size_t)pair * p.f.prev_pitch;
    const uint8_t* __restrict__ cur = p.f.cur_base + (size_t)pair * p.f.cur_pitch;
    const int W = p.f.W, H = p.f.H, stride = p.f.stride;

    // ---- 0. predictor: twice the parent's winner, clamped so that the block lies inside the frame
    const int pbx = min(bx >> 1, p.pnbx - 1), pby = min(by >> 1, p.pnby - 1);
    const size_t pk = ((size_t)pair * p.pnby + pby) * p.pnbx + pbx;
    // (the doubling cannot overflow for any triple whose clamp below matters: saturate first)
    const int qx = clampi(__builtin_amdgcn_readfirstlane(p.parent_best[3 * pk + 0]), -(1 << 20), 1 << 20);
    const int qy = clampi(__builtin_amdgcn_readfirstlane(p.parent_best[3 * pk + 1]), -(1 << 20), 1 << 20);
    const int px = clampi(2 * qx, -x0, W - B - x0), py = clampi(2 * qy, -y0, H - B - y0);

    uint8_t* win = h_lds + (size_t)wave * h_wave_bytes(B);
    uint8_t* cl = win + h_off_cur(B);
    const int IW = B + 2 * E, WS = h_ws(B);
    for (int i = lane; i < IW * IW; i += 64) {
        const int wy = i / IW, wx = i - wy * IW;
        const int gx = clampi(x0 + px - E + wx, 0, W - 1), gy = clampi(y0 + py - E + wy, 0, H - 1);
        win[wy * WS + wx] = prev[(size_t)gy * stride + gx];
    }
    if constexpr (BT != 0) {
        constexpr int BW = BT / 4;
        // the packed reads run two bytes past the window's B + 6 columns: they are shifted out again, but LDS that was never written would
        // make the kernel's reads depend on what ran before it
        for (int i = lane; i < IW; i += 64) { win[i * WS + IW] = 0; win[i * WS + IW + 1] = 0; }
        for (int i = lane; i < BT * BW; i += 64) {
            const int y = i / BW, q = i - y * BW;
            reinterpret_cast<uint32_t*>(cl)[i] = *reinterpret_cast<const uint32_t*>(cur + (size_t)(y0 + y) * stride + x0 + 4 * q);
        }
    } else {
        for (int i = lane; i < B * B; i += 64) {
            const int y = i / B, x = i - y * B;
            cl[i] = cur[(size_t)(y0 + y) * stride + x0 + x];
        }
    }
    wave_sync();

    // ---- 1. lane = candidate
    const int cand = lane < N * N ? lane : N * N - 1;
    const int ey = cand / N - E, ex = cand - (cand / N) * N - E;
    uint32_t sad = 0;
    if constexpr (BT != 0) {
        constexpr int BW = BT / 4, WSD = h_ws(BT) / 4;
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(win) + (ey + E) * WSD + ((ex + E) >> 2);
        const uint32_t* cp = reinterpret_cast<const uint32_t*>(cl);
        const uint32_t ph = (uint32_t)(ex + E) & 3u;
#pragma unroll
        for (int y = 0; y < BT; ++y) {
            uint32_t a[BW + 1];
#pragma unroll
            for (int g = 0; g <= BW; ++g) a[g] = wp[y * WSD + g];
#pragma unroll
            for (int g = 0; g < BW; ++g) sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(a[g + 1], a[g], ph), cp[y * BW + g], sad);
        }
    } else {
        const uint8_t* wp = win + (ey + E) * WS + (ex + E);
        for (int y = 0; y < B; ++y)
            for (int x = 0; x < B; ++x) {
                const int d = (int)cl[y * B + x] - (int)wp[y * WS + x];
                sad += (uint32_t)(d < 0 ? -d : d);
            }
    }

    // ---- 2. key = (SAD, dx^2 + dy^2, dy + R_l, dx + R_l) in 24 + 20 + 10 + 10 bits.  The bias of the last two fields does not change the
    // order, so the fields carry + 512 whatever R_l is: exact for every |d| <= 508 (the searches' own |d| <= R_l <= 127)
    const int dx = px + ex, dy = py + ey;
    const bool valid = lane < N * N && x0 + dx >= 0 && x0 + dx <= W - B && y0 + dy >= 0 && y0 + dy <= H - B;
    unsigned long long best = ~0ull;
    if (valid)
        best = ((unsigned long long)sad << 40) | ((unsigned long long)((uint32_t)(dx * dx + dy * dy) & 0xFFFFFu) << 20) |
               ((unsigned long long)((uint32_t)(dy + 512) & 1023u) << 10) | (unsigned long long)((uint32_t)(dx + 512) & 1023u);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = shfl_xor_u64(best, m);
        best = o < best ? o : best;
    }
    if (lane == 0) {
        const int bsad = (int)(best >> 40);
        const int bdy = (int)((best >> 10) & 1023) - 512, bdx = (int)(best & 1023) - 512;
        if (p.out_best) {
            p.out_best[3 * k + 0] = bdx;
            p.out_best[3 * k + 1] = bdy;
            p.out_best[3 * k + 2] = bsad;
        }
        if (p.out_entries) {
            float4 e;
            e.x = (float)(x0 + B / 2 + bdx) * p.nx;
            e.y = (float)(y0 + B / 2 + bdy) * p.ny;
            e.z = ((float)bdx / 1.0f) * (-p.nx);
            e.w = ((float)bdy / 1.0f) * (-p.ny);
            p.out_entries[k] = e;
        }
    }
}

// N1p: the refinement with neighbour and zero predictors.  The phases of sad_hier_refine_kernel, with up to kSadHierPredictors windows:
//   0. the triples of the parent, its four lattice neighbours (those that exist) and zero -> doubled, each clamped like the one predictor
//      above; a predictor equal to an earlier one is dropped (all wave-uniform, so is every branch on it).  Packed path: the windows of all
//      distinct predictors go to LDS slots of their own -- every load is issued before the first value is stored -- and the current block is
//      staged once.  Generic path (a window reaches 9 KB): one slot, predictor after predictor;
//   1. lane = candidate of each distinct predictor in turn; the lane keeps the minimum of its keys;
//   2. one butterfly over the wave.  The key is a total order on d, so dropping duplicates cannot change the winner.
// The two properties of the kernel above hold per window: positions outside the frame belong to invalid candidates only and their loads are
// clamped to the frame; the two pad bytes per row are written before the packed reads touch them.
constexpr int kPred = ofps::kSadHierPredictors;
__host__ __device__ constexpr int hp_wave_bytes(int B, bool packed) {
    return packed ? (kPred * h_off_cur(B) + ((B * B + 3) & ~3) + 15) & ~15 : h_wave_bytes(B);
}

template <int BT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void sad_hier_refine_pred_kernel(const RefineParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t h_lds[];
    constexpr int E = ofps::kSadHierRefine, N = 2 * E + 1;
    static_assert(N * N <= 64 && E == 3 && kPred == 6, "lane = candidate; parent + four neighbours + zero");
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
    const uint8_t* __restrict__ prev = p.f.prev_base + (size_t)pair * p.f.prev_pitch;
    const uint8_t* __restrict__ cur = p.f.cur_base + (size_t)pair * p.f.cur_pitch;
    const int W = p.f.W, H = p.f.H, stride = p.f.stride;

    // ---- 0. predictors.  A neighbour outside the parent lattice reads the parent's own triple and is dropped
    const int pbx = min(bx >> 1, p.pnbx - 1), pby = min(by >> 1, p.pnby - 1);
    const int* __restrict__ pb = p.parent_best + (size_t)pair * p.pnby * p.pnbx * 3;
    const int ox[kPred - 1] = {0, -1, 1, 0, 0}, oy[kPred - 1] = {0, 0, 0, -1, 1};
    int rx[kPred - 1], ry[kPred - 1];
    bool use[kPred];
#pragma unroll
    for (int w = 0; w < kPred - 1; ++w) {
        const int nx = pbx + ox[w], ny = pby + oy[w];
        use[w] = nx >= 0 && nx < p.pnbx && ny >= 0 && ny < p.pnby;
        const size_t pk = use[w] ? (size_t)ny * p.pnbx + nx : (size_t)pby * p.pnbx + pbx;
        rx[w] = pb[3 * pk + 0];
        ry[w] = pb[3 * pk + 1];
    }
    int px[kPred], py[kPred];
#pragma unroll
    for (int w = 0; w < kPred; ++w) {
        // (the doubling cannot overflow for any triple whose clamp below matters: saturate first)
        const int qx = w < kPred - 1 ? clampi(__builtin_amdgcn_readfirstlane(rx[w]), -(1 << 20), 1 << 20) : 0;
        const int qy = w < kPred - 1 ? clampi(__builtin_amdgcn_readfirstlane(ry[w]), -(1 << 20), 1 << 20) : 0;
        px[w] = clampi(2 * qx, -x0, W - B - x0);
        py[w] = clampi(2 * qy, -y0, H - B - y0);
        if (w == kPred - 1) use[w] = true;
#pragma unroll
        for (int j = 0; j < w; ++j) use[w] = use[w] && !(use[j] && px[j] == px[w] && py[j] == py[w]);
    }

    const int IW = B + 2 * E, WS = h_ws(B);
    uint8_t* base = h_lds + (size_t)wave * hp_wave_bytes(B, BT != 0);
    uint8_t* cl = base + (BT ? kPred : 1) * h_off_cur(B);
    if constexpr (BT != 0) {
        constexpr int BW = BT / 4, IWT = BT + 2 * E, PER = (IWT * IWT + 63) / 64;
        uint8_t v[kPred][PER];
#pragma unroll
        for (int w = 0; w < kPred; ++w)
            if (use[w]) {
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    const int i = min(lane + 64 * j, IWT * IWT - 1);
                    const int wy = i / IWT, wx = i - wy * IWT;
                    const int gx = clampi(x0 + px[w] - E + wx, 0, W - 1), gy = clampi(y0 + py[w] - E + wy, 0, H - 1);
                    v[w][j] = prev[(size_t)gy * stride + gx];
                }
            }
        for (int i = lane; i < BT * BW; i += 64) {
            const int y = i / BW, q = i - y * BW;
            reinterpret_cast<uint32_t*>(cl)[i] = *reinterpret_cast<const uint32_t*>(cur + (size_t)(y0 + y) * stride + x0 + 4 * q);
        }
#pragma unroll
        for (int w = 0; w < kPred; ++w)
            if (use[w]) {
                uint8_t* win = base + w * h_off_cur(BT);
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    const int i = min(lane + 64 * j, IWT * IWT - 1);     // (the last step's spare lanes write the last byte again)
                    const int wy = i / IWT, wx = i - wy * IWT;
                    win[wy * WS + wx] = v[w][j];
                }
                // the packed reads run two bytes past the window's B + 6 columns: written before they are read, as above
                for (int i = lane; i < IWT; i += 64) { win[i * WS + IWT] = 0; win[i * WS + IWT + 1] = 0; }
            }
        wave_sync();
    } else {
        for (int i = lane; i < B * B; i += 64) {
            const int y = i / B, x = i - y * B;
            cl[i] = cur[(size_t)(y0 + y) * stride + x0 + x];
        }
    }

    // ---- 1. lane = candidate, predictor after predictor
    const int cand = lane < N * N ? lane : N * N - 1;
    const int ey = cand / N - E, ex = cand - (cand / N) * N - E;
    unsigned long long best = ~0ull;
#pragma unroll
    for (int w = 0; w < kPred; ++w) {
        if (!use[w]) continue;
        uint32_t sad = 0;
        if constexpr (BT != 0) {
            constexpr int BW = BT / 4, WSD = h_ws(BT) / 4;
            const uint32_t* wp = reinterpret_cast<const uint32_t*>(base + w * h_off_cur(BT)) + (ey + E) * WSD + ((ex + E) >> 2);
            const uint32_t* cp = reinterpret_cast<const uint32_t*>(cl);
            const uint32_t ph = (uint32_t)(ex + E) & 3u;
#pragma unroll
            for (int y = 0; y < BT; ++y) {
                uint32_t a[BW + 1];
#pragma unroll
                for (int g = 0; g <= BW; ++g) a[g] = wp[y * WSD + g];
#pragma unroll
                for (int g = 0; g < BW; ++g) sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(a[g + 1], a[g], ph), cp[y * BW + g], sad);
            }
        } else {
            wave_sync();                                     // the window before this one has been read by every lane
            for (int i = lane; i < IW * IW; i += 64) {
                const int wy = i / IW, wx = i - wy * IW;
                const int gx = clampi(x0 + px[w] - E + wx, 0, W - 1), gy = clampi(y0 + py[w] - E + wy, 0, H - 1);
                base[wy * WS + wx] = prev[(size_t)gy * stride + gx];
            }
            wave_sync();
            const uint8_t* wp = base + (ey + E) * WS + (ex + E);
            for (int y = 0; y < B; ++y)
                for (int x = 0; x < B; ++x) {
                    const int d = (int)cl[y * B + x] - (int)wp[y * WS + x];
                    sad += (uint32_t)(d < 0 ? -d : d);
                }
        }
        // the key of sad_hier_refine_kernel
        const int dx = px[w] + ex, dy = py[w] + ey;
        const bool valid = lane < N * N && x0 + dx >= 0 && x0 + dx <= W - B && y0 + dy >= 0 && y0 + dy <= H - B;
        if (valid) {
            const unsigned long long key = ((unsigned long long)sad << 40) | ((unsigned long long)((uint32_t)(dx * dx + dy * dy) & 0xFFFFFu) << 20) |
                                           ((unsigned long long)((uint32_t)(dy + 512) & 1023u) << 10) | (unsigned long long)((uint32_t)(dx + 512) & 1023u);
            best = key < best ? key : best;
        }
    }

    // ---- 2. the minimum over the wave
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = shfl_xor_u64(best, m);
        best = o < best ? o : best;
    }
    if (lane == 0) {
        const int bsad = (int)(best >> 40);
        const int bdy = (int)((best >> 10) & 1023) - 512, bdx = (int)(best & 1023) - 512;
        if (p.out_best) {
            p.out_best[3 * k + 0] = bdx;
            p.out_best[3 * k + 1] = bdy;
            p.out_best[3 * k + 2] = bsad;
        }
        if (p.out_entries) {
            float4 e;
            e.x = (float)(x0 + B / 2 + bdx) * p.nx;
            e.y = (float)(y0 + B / 2 + bdy) * p.ny;
            e.z = ((float)bdx / 1.0f) * (-p.nx);
            e.w = ((float)bdy / 1.0f) * (-p.ny);
            p.out_entries[k] = e;
        }
    }
}

template <int BT, int WAVES>
void launch_refine(const RefineParams& p, hipStream_t s) {
    const unsigned nwg = (unsigned)((p.total + WAVES - 1) / WAVES);
    hipLaunchKernelGGL((sad_hier_refine_kernel<BT, WAVES>), dim3(nwg), dim3(64 * WAVES), (size_t)WAVES * h_wave_bytes(p.B), s, p);
}

template <int BT, int WAVES>
void launch_refine_pred(const RefineParams& p, hipStream_t s) {
    const unsigned nwg = (unsigned)((p.total + WAVES - 1) / WAVES);
    hipLaunchKernelGGL((sad_hier_refine_pred_kernel<BT, WAVES>), dim3(nwg), dim3(64 * WAVES), (size_t)WAVES * hp_wave_bytes(p.B, BT != 0), s, p);
}

// `frames` frames of W x H at src + k*src_pitch -> (W >> 1) x (H >> 1) at dst + k*dst_pitch
int down2_device(ofps_hip_ctx* ctx, const uint8_t* src, size_t src_pitch, int W, int H, int src_stride, uint8_t* dst, size_t dst_pitch, int dst_stride,
                 long long frames) {
    Down2Params p{};
    p.src = src; p.dst = dst; p.src_pitch = src_pitch; p.dst_pitch = dst_pitch;
    p.src_stride = src_stride; p.dst_stride = dst_stride;
    p.Wo = W >> 1; p.Ho = H >> 1; p.cols4 = (p.Wo + 3) / 4;
    p.total = frames * p.Ho * p.cols4;
    p.vec = (uintptr_t)src % 8 == 0 && src_pitch % 8 == 0 && src_stride % 8 == 0 && (uintptr_t)dst % 4 == 0 && dst_pitch % 4 == 0 && dst_stride % 4 == 0;
    if (p.total <= 0) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, (p.total + 255) / 256 < (1ll << 31), "sad_down2: grid too large");
    hipLaunchKernelGGL(sad_down2_kernel, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, ctx->stream, p);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// (the level's reach R_l biases the last two fields of the definition's key and so never changes its order: the kernel does not need it)
// predictors: OFPS_HIP_SAD_PRED_PARENT the kernel above alone, OFPS_HIP_SAD_PRED_NEIGHBOURS sad_hier_refine_pred_kernel (N1p)
int refine_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int block, const int* d_parent, int pnbx, int pnby, int predictors,
                  int* d_out_best, float4* d_out_entries) {
    RefineParams p{};
    p.f = f;
    p.nbx = f.W / block; p.nby = f.H / block; p.B = block;
    p.pnbx = pnbx; p.pnby = pnby;
    p.total = (long long)p.nbx * p.nby * pairs;
    p.nx = 1.0f / (float)f.W; p.ny = 1.0f / (float)f.H;
    p.parent_best = d_parent; p.out_best = d_out_best; p.out_entries = d_out_entries;
    if (p.total <= 0) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, p.total < (1ll << 31), "sad_refine: grid too large");
    // the packed forms read the current block by dwords: rows 4-byte aligned (every caller requires it)
    if (predictors == OFPS_HIP_SAD_PRED_NEIGHBOURS) {
        if (block == 16) launch_refine_pred<16, 4>(p, ctx->stream);
        else if (block == 8) launch_refine_pred<8, 4>(p, ctx->stream);
        else launch_refine_pred<0, 1>(p, ctx->stream);
    } else if (block == 16) launch_refine<16, 4>(p, ctx->stream);
    else if (block == 8) launch_refine<8, 4>(p, ctx->stream);
    else launch_refine<0, 1>(p, ctx->stream);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

int refine_check(ofps_hip_ctx* ctx, const void* prev, const void* cur, const void* parent, const void* out_best, int W, int H, int stride, int block,
                 int pnbx, int pnby, int reach, int predictors) {
    OFPS_REQUIRE(ctx, predictors == OFPS_HIP_SAD_PRED_PARENT || predictors == OFPS_HIP_SAD_PRED_NEIGHBOURS, "sad_refine: predictors=%d is not 0|1",
                 predictors);
    OFPS_REQUIRE(ctx, prev && cur && parent && out_best, "sad_refine: null pointer");
    OFPS_REQUIRE(ctx, W > 0 && H > 0 && stride >= W, "sad_refine: bad geometry W=%d H=%d stride=%d", W, H, stride);
    OFPS_REQUIRE(ctx, block >= 1 && block <= 64, "sad_refine: block=%d outside [1,64]", block);
    OFPS_REQUIRE(ctx, pnbx >= 1 && pnby >= 1, "sad_refine: parent lattice %d x %d is empty", pnbx, pnby);
    OFPS_REQUIRE(ctx, reach >= 0 && reach <= ofps::kSadHierMaxReach, "sad_refine: reach=%d outside [0,%d]", reach, ofps::kSadHierMaxReach);
    return OFPS_HIP_OK;
}

}  // namespace

namespace ofps {

// `frames` frames -> their halved forms, on ctx->stream: the levels hip_klt's pyramid is made of (klt.hip)
int sad_down2_frames_device(ofps_hip_ctx* ctx, const uint8_t* src, size_t src_pitch, int W, int H, int src_stride, uint8_t* dst, size_t dst_pitch,
                            int dst_stride, long long frames) {
    return down2_device(ctx, src, src_pitch, W, H, src_stride, dst, dst_pitch, dst_stride, frames);
}

int sad_hier_reach(int range, int levels) {
    if (range < 0 || range > 64 || levels < 1 || levels > 3) return -1;
    int r = range;
    for (int l = 1; l < levels; ++l) r = 2 * r + kSadHierRefine;
    return r <= kSadHierMaxReach ? r : -1;
}

int sad_hier_check(ofps_hip_ctx* ctx, int W, int H, int block, int range, int levels) {
    OFPS_REQUIRE(ctx, levels >= 1 && levels <= 3, "sad_flow: levels=%d is not 1|2|3", levels);
    int r = range;
    for (int l = 1; l < levels; ++l) r = 2 * r + kSadHierRefine;
    OFPS_REQUIRE(ctx, r <= kSadHierMaxReach, "sad_flow: range=%d with levels=%d reaches %d, above %d", range, levels, r, kSadHierMaxReach);
    OFPS_REQUIRE(ctx, (W >> (levels - 1)) >= block && (H >> (levels - 1)) >= block,
                 "sad_flow: a %d x %d frame halved %d times holds no %d x %d block (levels=%d)", W, H, levels - 1, block, block, levels);
    return OFPS_HIP_OK;
}

// Called by sad_pairs_device in place of the plain search's launches when the context's levels > 1.  Pyramids and the winners of the levels
// above 0 live in S_HIER_*: written and read on ctx->stream only, by this search alone -- the next search (the consistency check's backward
// one, the next ticket's) is ordered behind it by that stream.
int sad_hier_pairs_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int block, int range, int levels, int predictors, void* d_out_entries,
                          void* d_out_best) {
    int rc = sad_hier_check(ctx, f.W, f.H, block, range, levels);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_REQUIRE(ctx, levels > 1 && pairs >= 1 && d_out_entries, "sad_flow: levels=%d pairs=%d is no search over levels", levels, pairs);
    // the frames to halve: a chain once, not as two sets (SadFrames::sets); every level above 0 has the shape of level 0
    const SadFrames::Sets sets = f.sets(pairs);
    SadFrames lv[3];
    size_t pyr_off[3] = {0, 0, 0}, best_off[3] = {0, 0, 0}, pyr_bytes = 0, best_bytes = 0;
    lv[0] = f;
    for (int l = 1; l < levels; ++l) {                       // the geometry; the bases follow the reservation
        lv[l].W = lv[l - 1].W >> 1; lv[l].H = lv[l - 1].H >> 1;
        lv[l].stride = ofps::padded_stride(lv[l].W);         // 64-byte rows, so 16-byte frame pitches: the top search gets the strip kernel
        pyr_off[l] = pyr_bytes; pyr_bytes += (size_t)(sets.nprev + sets.ncur) * lv[l].stride * lv[l].H;
        best_off[l] = best_bytes;
        best_bytes += (((size_t)pairs * (lv[l].W / block) * (lv[l].H / block) * 3 * sizeof(int)) + 255) & ~size_t(255);
    }
    const int top = levels - 1;
    const size_t top_blocks = (size_t)pairs * (lv[top].W / block) * (lv[top].H / block);
    auto* pyr = static_cast<uint8_t*>(scratch(ctx, S_HIER_PYR, pyr_bytes));
    auto* bestbuf = static_cast<char*>(scratch(ctx, S_HIER_BEST, best_bytes));
    auto* top_ent = scratch(ctx, S_HIER_ENT, top_blocks * sizeof(float4));
    if (!pyr || !bestbuf || !top_ent) return OFPS_HIP_ENOMEM;
    for (int l = 1; l < levels; ++l) {
        uint8_t* dp = pyr + pyr_off[l];
        const size_t pitch = (size_t)lv[l].stride * lv[l].H;
        lv[l] = sets.in(dp, pitch, lv[l].W, lv[l].H, lv[l].stride);
        const SadFrames& s = lv[l - 1];
        rc = down2_device(ctx, s.prev_base, s.prev_pitch, s.W, s.H, s.stride, dp, pitch, lv[l].stride, sets.nprev);
        if (rc == OFPS_HIP_OK && !sets.chain)
            rc = down2_device(ctx, s.cur_base, s.cur_pitch, s.W, s.H, s.stride, dp + (size_t)sets.cur_first() * pitch, pitch, lv[l].stride, sets.ncur);
        if (rc != OFPS_HIP_OK) return rc;
    }
    // top: the plain search, never sad_pairs_device -- no quarter-pel refinement of the top winners, no way back here
    int* parent = reinterpret_cast<int*>(bestbuf + best_off[top]);
    rc = sad_search_device(ctx, lv[top], pairs, block, range, top_ent, parent);
    if (rc != OFPS_HIP_OK) return rc;
    for (int l = top - 1; l >= 0; --l) {
        int* out = l == 0 ? static_cast<int*>(d_out_best) : reinterpret_cast<int*>(bestbuf + best_off[l]);
        rc = refine_device(ctx, lv[l], pairs, block, parent, lv[l + 1].W / block, lv[l + 1].H / block, predictors, out,
                           l == 0 ? static_cast<float4*>(d_out_entries) : nullptr);
        if (rc != OFPS_HIP_OK) return rc;
        parent = out;
    }
    return OFPS_HIP_OK;
}

}  // namespace ofps

extern "C" {

int ofps_hip_set_sad_levels(ofps_hip_ctx* ctx, int levels) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, levels >= 1 && levels <= 3, "set_sad_levels: %d is not 1, 2 or 3", levels);
    ctx->opt.sad_levels = levels;
    return OFPS_HIP_OK;
}

int ofps_hip_get_sad_levels(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.sad_levels : OFPS_HIP_EINVAL; }

int ofps_hip_set_sad_predictors(ofps_hip_ctx* ctx, int mode) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, mode == OFPS_HIP_SAD_PRED_PARENT || mode == OFPS_HIP_SAD_PRED_NEIGHBOURS, "set_sad_predictors: %d is not 0 or 1", mode);
    ctx->opt.sad_predictors = mode;
    return OFPS_HIP_OK;
}

int ofps_hip_get_sad_predictors(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.sad_predictors : OFPS_HIP_EINVAL; }

int ofps_hip_sad_reach(int range, int levels) {
    const int r = ofps::sad_hier_reach(range, levels);
    return r < 0 ? OFPS_HIP_EINVAL : r;
}

int ofps_hip_sad_down2_dev(ofps_hip_ctx* ctx, const void* d_src, int W, int H, int stride, void* d_dst, int dst_stride) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_src && d_dst, "sad_down2: null device pointer");
    OFPS_REQUIRE(ctx, W >= 2 && H >= 2 && stride >= W && dst_stride >= (W >> 1), "sad_down2: bad geometry W=%d H=%d stride=%d dst_stride=%d", W, H,
                 stride, dst_stride);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return down2_device(ctx, static_cast<const uint8_t*>(d_src), 0, W, H, stride, static_cast<uint8_t*>(d_dst), 0, dst_stride, 1);
}

int ofps_hip_sad_down2(ofps_hip_ctx* ctx, const uint8_t* src, int W, int H, int stride, uint8_t* dst, int dst_stride) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, src && dst, "sad_down2: null host pointer");
    OFPS_REQUIRE(ctx, W >= 2 && H >= 2 && stride >= W && dst_stride >= (W >> 1), "sad_down2: bad geometry W=%d H=%d stride=%d dst_stride=%d", W, H,
                 stride, dst_stride);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int Wo = W >> 1, Ho = H >> 1, ss = ofps::padded_stride(W), ds = ofps::padded_stride(Wo);
    auto* d_src = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, (size_t)ss * H));
    auto* d_dst = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_HIER_PYR, (size_t)ds * Ho));
    if (!d_src || !d_dst) return OFPS_HIP_ENOMEM;
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_src, ss, src, stride, W, H, ctx->stream));
    const int rc = down2_device(ctx, d_src, 0, W, H, ss, d_dst, 0, ds, 1);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpy2DAsync(dst, dst_stride, d_dst, ds, Wo, Ho, hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_sad_refine_pred_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block,
                                 const void* d_parent_best, int nbx_parent, int nby_parent, int reach, int predictors, void* d_out_best,
                                 void* d_out_entries) {
    if (!ctx) return OFPS_HIP_EINVAL;
    const int rc = refine_check(ctx, d_prev, d_cur, d_parent_best, d_out_best, W, H, stride, block, nbx_parent, nby_parent, reach, predictors);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_REQUIRE(ctx, stride % 4 == 0 && ((uintptr_t)d_prev % 4) == 0 && ((uintptr_t)d_cur % 4) == 0,
                 "sad_refine: rows must be 4-byte aligned (stride=%d)", stride);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const SadFrames f{static_cast<const uint8_t*>(d_prev), static_cast<const uint8_t*>(d_cur), 0, 0, W, H, stride};
    return refine_device(ctx, f, 1, block, static_cast<const int*>(d_parent_best), nbx_parent, nby_parent, predictors, static_cast<int*>(d_out_best),
                         static_cast<float4*>(d_out_entries));
}

int ofps_hip_sad_refine_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block,
                            const void* d_parent_best, int nbx_parent, int nby_parent, int reach, void* d_out_best, void* d_out_entries) {
    return ofps_hip_sad_refine_pred_dev(ctx, d_prev, d_cur, W, H, stride, block, d_parent_best, nbx_parent, nby_parent, reach,
                                        OFPS_HIP_SAD_PRED_PARENT, d_out_best, d_out_entries);
}

int ofps_hip_sad_refine_pred(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int block,
                             const int32_t* parent_best, int nbx_parent, int nby_parent, int reach, int predictors, int32_t* out_best,
                             float* out_entries) {
    if (!ctx) return OFPS_HIP_EINVAL;
    int rc = refine_check(ctx, prev, cur, parent_best, out_best, W, H, stride, block, nbx_parent, nby_parent, reach, predictors);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // repack to a 64-byte-multiple device stride so any host stride is accepted (as ofps_hip_sad_flow does)
    const int dstride = ofps::padded_stride(W);
    const size_t pitch = (size_t)dstride * H, nblk = ofps_hip_sad_block_count(W, H, block), npar = (size_t)nbx_parent * nby_parent;
    auto* d_frames = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, 2 * pitch));
    auto* d_ent = static_cast<float*>(ofps::scratch(ctx, ofps::S_ENTRIES, nblk * 4 * sizeof(float)));
    auto* d_best = static_cast<int32_t*>(ofps::scratch(ctx, ofps::S_BEST, nblk * 3 * sizeof(int32_t)));
    auto* d_par = static_cast<int32_t*>(ofps::scratch(ctx, ofps::S_HIER_BEST, npar * 3 * sizeof(int32_t)));
    if (!d_frames || !d_ent || !d_best || !d_par) return OFPS_HIP_ENOMEM;
    if (!nblk) return OFPS_HIP_OK;
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_frames, dstride, prev, stride, W, H, ctx->stream));
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_frames + pitch, dstride, cur, stride, W, H, ctx->stream));
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_par, parent_best, npar * 3 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    rc = ofps_hip_sad_refine_pred_dev(ctx, d_frames, d_frames + pitch, W, H, dstride, block, d_par, nbx_parent, nby_parent, reach, predictors, d_best,
                                      out_entries ? d_ent : nullptr);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_best, d_best, nblk * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out_entries) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_entries, d_ent, nblk * 4 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_sad_refine(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int block,
                        const int32_t* parent_best, int nbx_parent, int nby_parent, int reach, int32_t* out_best, float* out_entries) {
    return ofps_hip_sad_refine_pred(ctx, prev, cur, W, H, stride, block, parent_best, nbx_parent, nby_parent, reach, OFPS_HIP_SAD_PRED_PARENT,
                                    out_best, out_entries);
}

}  // extern "C"
