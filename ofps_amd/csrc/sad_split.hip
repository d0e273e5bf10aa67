// sad_split.hip -- N1s: hip_sad's split step.  A block that holds two motions yields its four sub-blocks' vectors.
//
// Spec: include/ofps_hip.h / DESIGN.md "N1s".  For every kept lattice block the four b x b sub-blocks (b = B / 2) are searched in +-3
// windows around the block's own winner, its four lattice neighbours' winners and zero; the block is SPLIT iff the four sub-block SADs
// together lie at least T/16 grey levels per pixel below the block's own.  All-integer, bit-exact against tests/indep_sad_split.py.
//
// sad_split_kernel: the shape of sad_hier_refine_pred_kernel (sad_hier.hip): one wave per block, the waves of a workgroup independent.
//   0. the keep flag (0: the wave writes its block's empty slots and is done), the five triples and zero -> predictors (wave-uniform);
//   1. one (B+6)^2 window of prev per distinct predictor, at the predictor clamped for the BLOCK.  It covers the +-3 windows of all four
//      sub-blocks whatever their own clamps do: a sub-block's clamp moves a predictor by at most b towards the block's, so sub-block s
//      reads the window at the offset (s & 1) * b + px_s - px_B in [0, b] (y alike).  Packed form (B 16 and 8, 4-byte aligned rows): the
//      windows of all distinct predictors go to LDS slots of their own -- every load is issued before the first value is stored -- and
//      the current block is staged once; lane = candidate e; per predictor and sub-block b rows of b/4 + 1 window dwords, v_alignbyte
//      to the lane's byte phase, v_sad_u8 against the row of the current sub-block.  Byte-wise form (any other even B <= 64, unaligned
//      rows): one LDS slot, predictor after predictor;
//   2. one 64-bit key butterfly per sub-block; lanes 0..3 apply the rule and store their sub-block's triple, raw slot and slot flag.
// The two properties of the refinement kernels hold per window: positions outside the frame belong to invalid candidates only and their
// loads are clamped to the frame; the two pad bytes per row are written before the packed reads touch them.
#include "common.hpp"

namespace {

using ofps::SadFrames;

struct SplitParams {
    SadFrames f;                    // the pair the integer search read
    int nbx, nby, B, T;
    int total;                      // blocks
    float nx, ny;
    const int* best;                // (dx, dy, sad) per block: the parents
    const uint8_t* keep;            // or null: all ones
    int* sub_best;                  // 12 i32 per block
    uint8_t* split;                 // u8 per block
    float4* raw;                    // 4 records per block, or null
    uint8_t* slot_flags;            // 4 u8 per block, or null
};

constexpr int E = 3, N = 2 * E + 1, kPred = 6;
static_assert(N * N <= 64, "lane = candidate");

__host__ __device__ constexpr int s_ws(int B) { return B + 8; }                     // bytes of one window row (B + 6 used; packed reads run to B + 8)
__host__ __device__ constexpr int s_win(int B) { return ((B + 6) * s_ws(B) + 3) & ~3; }
__host__ __device__ constexpr int s_wave_bytes(int B, bool packed) { return ((packed ? kPred : 1) * s_win(B) + ((B * B + 3) & ~3) + 15) & ~15; }
static_assert(s_wave_bytes(64, false) <= 16 * 1024 && 4 * s_wave_bytes(16, true) <= 16 * 1024, "a workgroup's windows and blocks");

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

// the key of the refinement kernels: (SAD, dx^2 + dy^2, dy + 512, dx + 512) in 24 + 20 + 10 + 10 bits; the bias of the last two fields does
// not change the order, so + 512 stands for the definition's R0 + 3 (|d| <= R0 + 3 <= 127)
__device__ __forceinline__ unsigned long long split_key(uint32_t sad, int dx, int dy) {
    return ((unsigned long long)sad << 40) | ((unsigned long long)((uint32_t)(dx * dx + dy * dy) & 0xFFFFFu) << 20) |
           ((unsigned long long)((uint32_t)(dy + 512) & 1023u) << 10) | (unsigned long long)((uint32_t)(dx + 512) & 1023u);
}

template <int BT, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void sad_split_kernel(const SplitParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_lds[];
    const int B = BT ? BT : p.B, b = B >> 1;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * WAVES + wave;
    if (k >= p.total) return;
    const int by = k / p.nbx, bx = k - by * p.nbx;
    const int x0 = bx * B, y0 = by * B;
    const uint8_t* __restrict__ prev = p.f.prev_base;
    const uint8_t* __restrict__ cur = p.f.cur_base;
    const int W = p.f.W, H = p.f.H, stride = p.f.stride;

    // ---- 0. a block that is not kept does no work: no split, no slot
    const int kept = p.keep ? __builtin_amdgcn_readfirstlane((int)p.keep[k]) : 1;
    if (!kept) {
        if (lane < 12) p.sub_best[12 * (size_t)k + lane] = 0;
        if (lane < 4 && p.raw) p.raw[4 * (size_t)k + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < 4 && p.slot_flags) p.slot_flags[4 * (size_t)k + lane] = 0;
        if (lane == 0) p.split[k] = 0;
        return;
    }

    // the predictors.  A neighbour outside the lattice reads the block's own triple and is dropped
    const int ox[kPred - 1] = {0, -1, 1, 0, 0}, oy[kPred - 1] = {0, 0, 0, -1, 1};
    int qx[kPred], qy[kPred];
    bool has[kPred];                                           // the predictor exists
#pragma unroll
    for (int w = 0; w < kPred - 1; ++w) {
        const int nx = bx + ox[w], ny = by + oy[w];
        has[w] = nx >= 0 && nx < p.nbx && ny >= 0 && ny < p.nby;
        const size_t pk = has[w] ? (size_t)ny * p.nbx + nx : (size_t)k;
        // whatever the triples hold, a predictor ends inside the frame: saturate first so that no sum below overflows
        qx[w] = clampi(__builtin_amdgcn_readfirstlane(p.best[3 * pk + 0]), -(1 << 20), 1 << 20);
        qy[w] = clampi(__builtin_amdgcn_readfirstlane(p.best[3 * pk + 1]), -(1 << 20), 1 << 20);
    }
    qx[kPred - 1] = 0; qy[kPred - 1] = 0; has[kPred - 1] = true;
    // the unsplit block's record is N1's of the triple as it stands (in 64 bits: whatever it holds)
    const long long pdx = __builtin_amdgcn_readfirstlane(p.best[3 * (size_t)k + 0]), pdy = __builtin_amdgcn_readfirstlane(p.best[3 * (size_t)k + 1]);
    const int psad = __builtin_amdgcn_readfirstlane(p.best[3 * (size_t)k + 2]);

    const int WS = s_ws(B);
    uint8_t* base = s_lds + (size_t)wave * s_wave_bytes(B, BT != 0);
    uint8_t* cl = base + (BT ? kPred : 1) * s_win(B);
    const int cand = lane < N * N ? lane : N * N - 1;
    const int ey = cand / N - E, ex = cand - (cand / N) * N - E;
    unsigned long long best[4] = {~0ull, ~0ull, ~0ull, ~0ull};

    // ---- 1. the window of predictor w lies at the predictor clamped for the BLOCK.  A predictor equal to an earlier one is dropped
    int bxp[kPred], byp[kPred];
    bool use[kPred];
#pragma unroll
    for (int w = 0; w < kPred; ++w) {
        bxp[w] = clampi(qx[w], -x0, W - B - x0);
        byp[w] = clampi(qy[w], -y0, H - B - y0);
        use[w] = has[w];
#pragma unroll
        for (int j = 0; j < w; ++j) use[w] = use[w] && !(use[j] && qx[j] == qx[w] && qy[j] == qy[w]);
    }
    const int IW = B + 2 * E;

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
                    const int gx = clampi(x0 + bxp[w] - E + wx, 0, W - 1), gy = clampi(y0 + byp[w] - E + wy, 0, H - 1);
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
                uint8_t* win = base + w * s_win(BT);
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    const int i = min(lane + 64 * j, IWT * IWT - 1);     // (the last step's spare lanes write the last byte again)
                    const int wy = i / IWT, wx = i - wy * IWT;
                    win[wy * WS + wx] = v[w][j];
                }
                // the packed reads run two bytes past the window's B + 6 columns: written before they are read
                for (int i = lane; i < IWT; i += 64) { win[i * WS + IWT] = 0; win[i * WS + IWT + 1] = 0; }
            }
        wave_sync();
    } else {
        for (int i = lane; i < B * B; i += 64) {
            const int y = i / B, x = i - y * B;
            cl[i] = cur[(size_t)(y0 + y) * stride + x0 + x];
        }
    }

#pragma unroll
    for (int w = 0; w < kPred; ++w) {
        if (!use[w]) continue;
        if constexpr (BT == 0) {
            wave_sync();                                     // the window before this one has been read by every lane (the first: cl is written)
            for (int i = lane; i < IW * IW; i += 64) {
                const int wy = i / IW, wx = i - wy * IW;
                const int gx = clampi(x0 + bxp[w] - E + wx, 0, W - 1), gy = clampi(y0 + byp[w] - E + wy, 0, H - 1);
                base[wy * WS + wx] = prev[(size_t)gy * stride + gx];
            }
            wave_sync();
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int sxo = (s & 1) * b, syo = (s >> 1) * b;
            const int sx0 = x0 + sxo, sy0 = y0 + syo;
            // this sub-block's own clamp of the predictor, and where its +-3 window begins inside the block's: offsets in [0, b]
            const int px = clampi(qx[w], -sx0, W - b - sx0), py = clampi(qy[w], -sy0, H - b - sy0);
            const int offx = sxo + px - bxp[w], offy = syo + py - byp[w];
            uint32_t sad = 0;
            if constexpr (BT != 0) {
                constexpr int BW = BT / 4, bw = BT / 8, bt = BT / 2, WSD = s_ws(BT) / 4;
                const int col = offx + ex + E;               // window byte of the candidate's first column: 0 .. b + 6
                const uint32_t* wp = reinterpret_cast<const uint32_t*>(base + w * s_win(BT)) + (offy + ey + E) * WSD + (col >> 2);
                const uint32_t* cp = reinterpret_cast<const uint32_t*>(cl) + syo * BW + (sxo >> 2);
                const uint32_t ph = (uint32_t)col & 3u;
#pragma unroll
                for (int y = 0; y < bt; ++y) {
                    uint32_t a[bw + 1];
#pragma unroll
                    for (int g = 0; g <= bw; ++g) a[g] = wp[y * WSD + g];
#pragma unroll
                    for (int g = 0; g < bw; ++g) sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(a[g + 1], a[g], ph), cp[y * BW + g], sad);
                }
            } else {
                const uint8_t* wp = base + (offy + ey + E) * WS + (offx + ex + E);
                const uint8_t* cp = cl + syo * B + sxo;
                for (int y = 0; y < b; ++y)
                    for (int x = 0; x < b; ++x) {
                        const int d = (int)cp[y * B + x] - (int)wp[y * WS + x];
                        sad += (uint32_t)(d < 0 ? -d : d);
                    }
            }
            const int dx = px + ex, dy = py + ey;
            const bool valid = lane < N * N && sx0 + dx >= 0 && sx0 + dx <= W - b && sy0 + dy >= 0 && sy0 + dy <= H - b;
            if (valid) {
                const unsigned long long key = split_key(sad, dx, dy);
                best[s] = key < best[s] ? key : best[s];
            }
        }
    }

    // ---- 2. the minimum over the wave, per sub-block (d = 0 is a valid candidate of every sub-block: no key stays empty)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long o = shfl_xor_u64(best[s], m);
            best[s] = o < best[s] ? o : best[s];
        }
    }
    long long sum = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) sum += (long long)(best[s] >> 40);
    const bool split = 16ll * ((long long)psad - sum) >= (long long)p.T * B * B;
    if (lane < 4) {
        const int s = lane;
        const unsigned long long key = s == 0 ? best[0] : (s == 1 ? best[1] : (s == 2 ? best[2] : best[3]));
        const int ssad = (int)(key >> 40);
        const int sdy = (int)((key >> 10) & 1023) - 512, sdx = (int)(key & 1023) - 512;
        int* sb = p.sub_best + 12 * (size_t)k + 3 * s;
        sb[0] = sdx; sb[1] = sdy; sb[2] = ssad;
        const bool flag = split || s == 0;
        if (p.slot_flags) p.slot_flags[4 * (size_t)k + s] = flag ? 1 : 0;
        if (p.raw) {
            // N1's record (sad.hip: write_block_result), of the sub-block's centre and vector or, unsplit, of the block's
            const int cx = split ? x0 + (s & 1) * b + b / 2 : x0 + B / 2, cy = split ? y0 + (s >> 1) * b + b / 2 : y0 + B / 2;
            const long long dx = split ? sdx : pdx, dy = split ? sdy : pdy;
            float4 e;
            e.x = (float)(cx + dx) * p.nx;
            e.y = (float)(cy + dy) * p.ny;
            e.z = ((float)dx / 1.0f) * (-p.nx);
            e.w = ((float)dy / 1.0f) * (-p.ny);
            p.raw[4 * (size_t)k + s] = flag ? e : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (s == 0) p.split[k] = split ? 1 : 0;
    }
}

template <int BT, int WAVES>
void launch_split(const SplitParams& p, hipStream_t s) {
    const unsigned nwg = (unsigned)((p.total + WAVES - 1) / WAVES);
    hipLaunchKernelGGL((sad_split_kernel<BT, WAVES>), dim3(nwg), dim3(64 * WAVES), (size_t)WAVES * s_wave_bytes(p.B, BT != 0), s, p);
}

}  // namespace

namespace ofps {

int sad_split_check(ofps_hip_ctx* ctx, int block, int reach, int threshold, const char* who) {
    OFPS_REQUIRE(ctx, block >= 8 && block <= 64 && block % 2 == 0, "%s: split blocks need an even block in [8, 64] (sub-block side >= 4), got %d", who, block);
    OFPS_REQUIRE(ctx, reach >= 0 && reach + kSadHierRefine <= kSadHierMaxReach, "%s: split blocks: reach %d + %d above %d", who, reach, kSadHierRefine,
                 kSadHierMaxReach);
    OFPS_REQUIRE(ctx, threshold >= 1 && threshold <= kSadSplitMax, "%s: split threshold %d outside [1, %d]", who, threshold, kSadSplitMax);
    return OFPS_HIP_OK;
}

int sad_split_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int block, int reach, int threshold, const int* d_best, const uint8_t* d_keep,
                     int* d_sub_best, uint8_t* d_split, float4* d_raw, uint8_t* d_slot_flags) {
    const int rc = sad_split_check(ctx, block, reach, threshold, "sad_split");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_REQUIRE(ctx, pairs == 1, "sad_split: %d pairs (one pair at a time)", pairs);
    OFPS_REQUIRE(ctx, f.W > 0 && f.H > 0 && f.stride >= f.W, "sad_split: bad geometry W=%d H=%d stride=%d", f.W, f.H, f.stride);
    OFPS_REQUIRE(ctx, f.prev_base && f.cur_base && d_best && d_sub_best && d_split, "sad_split: null pointer");
    SplitParams p{};
    p.f = f;
    p.nbx = f.W / block; p.nby = f.H / block; p.B = block; p.T = threshold;
    const long long total = (long long)p.nbx * p.nby;
    if (total <= 0) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, total < (1ll << 29), "sad_split: grid too large");
    p.total = (int)total;
    p.nx = 1.0f / (float)f.W; p.ny = 1.0f / (float)f.H;
    p.best = d_best; p.keep = d_keep; p.sub_best = d_sub_best; p.split = d_split; p.raw = d_raw; p.slot_flags = d_slot_flags;
    // the packed forms read the current block by dwords: rows 4-byte aligned, else the byte-wise form
    const bool aligned = f.stride % 4 == 0 && (uintptr_t)f.cur_base % 4 == 0;
    if (block == 16 && aligned) launch_split<16, 4>(p, ctx->stream);
    else if (block == 8 && aligned) launch_split<8, 4>(p, ctx->stream);
    else launch_split<0, 1>(p, ctx->stream);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

}  // namespace ofps

extern "C" {

int ofps_hip_set_sad_split(ofps_hip_ctx* ctx, int threshold) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, threshold >= 0 && threshold <= ofps::kSadSplitMax, "set_sad_split: %d outside [0, %d]", threshold, ofps::kSadSplitMax);
    ctx->opt.sad_split = threshold;
    return OFPS_HIP_OK;
}

int ofps_hip_get_sad_split(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.sad_split : OFPS_HIP_EINVAL; }

size_t ofps_hip_sad_record_capacity(ofps_hip_ctx* ctx, int W, int H, int block) {
    const size_t nblk = ofps_hip_sad_block_count(W, H, block);
    return ctx && ctx->opt.sad_split > 0 ? 4 * nblk : nblk;
}

int ofps_hip_sad_split_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block, const void* d_best,
                           const void* d_keep, int reach, int threshold, void* d_out_sub_best, void* d_out_split, void* d_out_entries,
                           void* d_out_slot_flags) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_prev && d_cur && d_best && d_out_sub_best && d_out_split, "sad_split_dev: null device pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ofps::SadFrames f{static_cast<const uint8_t*>(d_prev), static_cast<const uint8_t*>(d_cur), 0, 0, W, H, stride};
    return ofps::sad_split_device(ctx, f, 1, block, reach, threshold, static_cast<const int*>(d_best), static_cast<const uint8_t*>(d_keep),
                                  static_cast<int*>(d_out_sub_best), static_cast<uint8_t*>(d_out_split), static_cast<float4*>(d_out_entries),
                                  static_cast<uint8_t*>(d_out_slot_flags));
}

int ofps_hip_sad_split(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int block, const int32_t* best,
                       const uint8_t* keep, int reach, int threshold, int32_t* out_sub_best, uint8_t* out_split, float* out_entries,
                       uint8_t* out_slot_flags) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, prev && cur && best && out_sub_best && out_split, "sad_split: null host pointer");
    OFPS_REQUIRE(ctx, W > 0 && H > 0 && stride >= W, "sad_split: bad geometry W=%d H=%d stride=%d", W, H, stride);
    int rc = ofps::sad_split_check(ctx, block, reach, threshold, "sad_split");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // repack to a 64-byte-multiple device stride so any host stride is accepted (as ofps_hip_sad_flow does)
    const int dstride = ofps::padded_stride(W);
    const size_t pitch = (size_t)dstride * H, nblk = ofps_hip_sad_block_count(W, H, block);
    if (!nblk) return OFPS_HIP_OK;
    const size_t keep_bytes = (nblk + 15) & ~size_t(15);
    auto* d_frames = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, 2 * pitch));
    auto* d_best = static_cast<int32_t*>(ofps::scratch(ctx, ofps::S_BEST, nblk * 3 * sizeof(int32_t)));
    auto* d_keep = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_MASK, keep_bytes));
    auto* d_work = static_cast<char*>(ofps::scratch(ctx, ofps::S_SPLIT, ofps::sad_split_bytes(nblk)));
    if (!d_frames || !d_best || !d_keep || !d_work) return OFPS_HIP_ENOMEM;
    auto* d_raw = reinterpret_cast<float4*>(d_work);
    auto* d_sub = reinterpret_cast<int*>(d_work + nblk * 4 * sizeof(float4));
    auto* d_slot = reinterpret_cast<uint8_t*>(d_sub + 12 * nblk);
    auto* d_split = d_slot + 4 * nblk;
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_frames, dstride, prev, stride, W, H, ctx->stream));
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_frames + pitch, dstride, cur, stride, W, H, ctx->stream));
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_best, best, nblk * 3 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (keep) OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_keep, keep, nblk, hipMemcpyHostToDevice, ctx->stream));
    rc = ofps_hip_sad_split_dev(ctx, d_frames, d_frames + pitch, W, H, dstride, block, d_best, keep ? d_keep : nullptr, reach, threshold, d_sub, d_split,
                                out_entries ? d_raw : nullptr, out_slot_flags ? d_slot : nullptr);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_sub_best, d_sub, nblk * 12 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_split, d_split, nblk, hipMemcpyDeviceToHost, ctx->stream));
    if (out_entries) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_entries, d_raw, nblk * 16 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (out_slot_flags) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_slot_flags, d_slot, nblk * 4, hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_sad_flow_split_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block, int range,
                                int min_pixels, int limit, int median, int threshold, void* d_out_entries, void* d_out_count) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_prev && d_cur && d_out_entries && d_out_count, "sad_flow_split_dev: null device pointer");
    OFPS_REQUIRE(ctx, min_pixels >= 0 && limit >= 0 && median >= 0, "sad_flow_split_dev: negative criterion (gate %d, limit %d, median %d)", min_pixels,
                 limit, median);
    OFPS_REQUIRE(ctx, threshold >= 1 && threshold <= ofps::kSadSplitMax, "sad_flow_split_dev: split threshold %d outside [1, %d]", threshold,
                 ofps::kSadSplitMax);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::sad_flow_filtered_device(ctx, {static_cast<const uint8_t*>(d_prev), static_cast<const uint8_t*>(d_cur), 0, 0, W, H, stride}, 1, block,
                                          range, {min_pixels, limit, median, /*intra=*/0, /*cut=*/0, threshold}, static_cast<float4*>(d_out_entries), nullptr,
                                          static_cast<uint32_t*>(d_out_count), "sad_flow_split_dev");
}

}  // extern "C"
