// klt.hip -- hip_klt (include/ofps_hip.h N3): one corner feature per lattice cell of the previous frame, tracked into the current
// frame by a pyramidal Lucas-Kanade iteration.  Every sum over pixels is an integer; the handful of f64 operations per iteration are
// scalar, in the definition's order and computed by every lane alike (the build compiles with -ffp-contract=off).
//
// klt_score_kernel: one workgroup = one cell.  The cell's pixels and an r + 1 halo are staged in LDS; a horizontal pass makes the
//   (2r + 1)-column sums of gx*gx, gx*gy, gy*gy for the cell's columns over the cell's rows and r rows above and below, the Sobel
//   values of the walked columns held in registers; a vertical pass sums 2r + 1 of those rows per pixel.  The cell's winner is the
//   maximum of one 64-bit key, score << 32 | ~local index: a total order, so the reduction's order cannot change it.
// klt_track_kernel: one wave = one slot, the lanes over the n * n <= 225 window pixels (four per lane), the (n + 2)^2 template samples
//   of a level in LDS, the template's gradients in registers; A11, A12, A22, b1, b2 and the residual are 64-bit integer sums reduced
//   across the wave by a butterfly, so every lane holds them and takes the same branches.  All levels in one launch.
// klt_track_zm_kernel: the same body with mean removal (N3m): per level sx = sum Ix and sy = sum Iy are reduced beside the three products
//   (both in one 64-bit butterfly, a word each) and every lane's gradients become the centred N Ix - sx, N Iy - sy (below 6e7: int32), so
//   the iteration's two sums are N3m's b1 and b2 as they are -- one more reduction per level, none per iteration --, and the residual takes a
//   32-bit one more for the mean of d.
// klt_track_*fb_kernel: the same body with the forward-backward check (N3f): the wave whose forward pass ends with status 0 runs the pass
//   once more right behind it, from P = 256 (x, y) + dq and with the two frames' pointers exchanged, on the same LDS template rows and in the
//   same registers, and keeps the slot iff that pass is kept too and comes back to within F / 256 pixel; status 5 otherwise.
// klt_track_q_kernel, klt_track_q_zm_kernel: one direction from points given in 1/256 pixel, the stage the check is built from.
// klt_track_pred*_kernel: the one-pair kernels with motion prediction (N3p): a pass starts from the slot's guess -- given by the caller, or made
//   by klt_predict_slot from the previous pair's raw slots in front of the wave's first level -- in place of dq = (0, 0), N3f's backward pass
//   from its negation.  klt_predict_kernel: the predictor alone, a lane per slot.
// klt_track_batch_pred*_kernel: the batch kernels with motion prediction (N3pb): ONE item of a batch per launch, its slots' guesses predicted from
//   the raw slots the launch of the item before has written.  The launches follow one another on the context's stream, which is all that orders
//   them: no wave waits for another.
//
// The host side holds each step once.  klt_track_launch: THE track launch, the kernel picked from a [check][mean removal] table of the launch's
//   parameter struct.  klt_track_settings: the part of KltTrackParams that comes from the context and the call.  klt_pyramid_device: the levels of
//   a SadFrames' distinct frames; the one-pair forms hand it their two frames as a batch of one pair.  KltWork: S_KLT_WORK's layout.
//   ofps::klt_flow_device(KltFlowCall): THE driver -- score, pyramid, track, (N3i) verdict and cut, compaction -- of the one-pair form, the batch
//   form and the chained batch, which differ in the score and the track launch alone.  KltHostIo, klt_host_read: S_KLT_HOST's layout and the
//   read-back of the host-pointer flow forms.
#include "common.hpp"

#include <cmath>

namespace {

using namespace ofps;

constexpr int kKltTemplate = (2 * kKltMaxRadius + 3) * (2 * kKltMaxRadius + 3);       // 17 x 17 samples
constexpr int kKltTemplatePitch = (kKltTemplate + 3) & ~3;
constexpr int kKltTrackWaves = 4;

enum { KLT_KEPT = 0, KLT_NONE = 1, KLT_FLAT = 2, KLT_LEFT = 3, KLT_RESIDUAL = 4, KLT_NO_RETURN = 5 };

// how klt_track_body starts and ends: N3 from a pixel; N3 and N3f's backward pass behind it; one pass from a 1/256-pixel position (the stage form)
enum { KLT_MODE_PIXEL = 0, KLT_MODE_FB = 1, KLT_MODE_Q = 2 };

struct KltLevels {
    const uint8_t* prev[kKltMaxLevels];
    const uint8_t* cur[kKltMaxLevels];
    int W[kKltMaxLevels], H[kKltMaxLevels], stride[kKltMaxLevels];
};

struct KltTrackParams {
    KltLevels lv;
    int L, w, K, min_eig, max_residual;
    const int* pts;                      // n points, pt_stride ints apart: (x, y[, score])
    int pt_stride, from_features, n;     // from_features: the points are the score kernel's triples, x < 0 = no feature (status 1)
    int fb_limit;                        // N3f: F in 1/256 pixel, read by the FB kernels alone (it lies where the struct had padding)
    int* out_quad;                       // 4 per slot or null
    int* out_slots;                      // 6 per slot or null
    float4* out_rec;                     // the slot's record (zeros unless kept) or null
    uint8_t* out_flag;                   // 1 = kept; beside out_rec
};

// the batch form's track launch (N3b): slot s belongs to item s / slots_per_item, whose frames of level l lie item * pitch[l] behind the
// level's base (a pitch of 0: one frame for every item); shared_features: one set of triples, of the key frame, for every item
struct KltTrackBatchParams {
    KltTrackParams t;
    size_t prev_pitch[kKltMaxLevels], cur_pitch[kKltMaxLevels];
    int slots_per_item, shared_features;
};

// N3p's track launch: where slot s starts from.  `guesses`: 2 ints per slot, the stage form; else `prev_slots`: the previous pair's raw slots
// on the nx x ny lattice whose slot s this is, the guess made from them by klt_predict_slot.  (A wrapper, as the batch form's: KltTrackParams
// keeps its size, so no kernel argument of the other kernels moves.)
struct KltTrackPredParams {
    KltTrackParams t;
    const int* guesses;
    const int* prev_slots;
    int nx, ny;
};

// N3pb's track launch: the slots first_slot .. t.n - 1 of the batch, ONE item's.  Where they start from: the guesses klt_predict_slot makes from
// `prev_slots`, the raw slots of the item before on the item's nx x ny lattice (null: every guess is (0, 0)).  Never the array the launch writes
struct KltTrackBatchPredParams {
    KltTrackBatchParams b;
    const int* prev_slots;
    int first_slot, nx, ny;
};

constexpr int kKltMaxGuess = 1 << 23;                        // N3p: a guess beyond it, per component, is (0, 0)

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

__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int m = 1; m < 64; m <<= 1) v += (long long)shfl_xor_u64((unsigned long long)v, m);
    return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    for (int m = 1; m < 64; m <<= 1) { const unsigned long long o = shfl_xor_u64(v, m); v = o > v ? o : v; }
    return v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ceil(sqrt(D)), exact: the f64 root is a first guess, the integer loops make it the floor whatever its last bit was
__device__ __forceinline__ unsigned long long ceil_sqrt_u64(unsigned long long D) {
    unsigned long long s = (unsigned long long)sqrt((double)D);
    while (s * s > D) --s;
    while ((s + 1) * (s + 1) <= D) ++s;
    return s + (s * s < D ? 1 : 0);
}

// one workgroup's cell of one frame; `out`: that frame's triples
template <int C>
__device__ __forceinline__ void klt_score_body(const uint8_t* __restrict__ img, int W, int H, int stride, int r, int min_score, int* __restrict__ out) {
    constexpr int T = C * C < 256 ? C * C : 256;
    constexpr int PWMAX = C + 2 * (kKltMaxScoreRadius + 1), HRMAX = C + 2 * kKltMaxScoreRadius;
    __shared__ uint8_t P[PWMAX * PWMAX];
    __shared__ int Hs[3][HRMAX * C];
    __shared__ unsigned long long wkey[T / 64];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * C, y0 = blockIdx.y * C;
    const int PW = C + 2 * (r + 1), HR = C + 2 * r;
    // pixels outside the frame are replicated: they reach only pixels that are not admissible
    for (int idx = tid; idx < PW * PW; idx += T) {
        const int py = idx / PW, px = idx - py * PW;
        const int gx = clampi(x0 - (r + 1) + px, 0, W - 1), gy = clampi(y0 - (r + 1) + py, 0, H - 1);
        P[idx] = img[(size_t)gy * stride + gx];
    }
    __syncthreads();
    // row hy of Hs is frame row y0 - r + hy = P row hy + 1; the window of column lx covers P columns lx + 1 .. lx + 2r + 1
    for (int idx = tid; idx < HR * C; idx += T) {
        const int hy = idx / C, lx = idx - hy * C;
        const uint8_t* row = &P[(hy + 1) * PW + lx];
        // column c of the walk: s = top + 2 mid + bottom (gx = s[c + 1] - s[c - 1]), d = bottom - top (gy = d[c - 1] + 2 d[c] + d[c + 1])
        int s0 = (int)row[-PW] + 2 * (int)row[0] + (int)row[PW], d0 = (int)row[PW] - (int)row[-PW];
        int s1 = (int)row[1 - PW] + 2 * (int)row[1] + (int)row[1 + PW], d1 = (int)row[1 + PW] - (int)row[1 - PW];
        int a = 0, b = 0, c = 0;
        for (int i = 0; i <= 2 * r; ++i) {
            const uint8_t* q = row + i + 2;
            const int s2 = (int)q[-PW] + 2 * (int)q[0] + (int)q[PW], d2 = (int)q[PW] - (int)q[-PW];
            const int gx = s2 - s0, gy = d0 + 2 * d1 + d2;
            a += gx * gx; b += gx * gy; c += gy * gy;
            s0 = s1; d0 = d1; s1 = s2; d1 = d2;
        }
        Hs[0][idx] = a; Hs[1][idx] = b; Hs[2][idx] = c;
    }
    __syncthreads();
    unsigned long long key = 0;
    for (int idx = tid; idx < C * C; idx += T) {
        const int ly = idx / C, lx = idx - ly * C;
        const int x = x0 + lx, y = y0 + ly;
        if (x < r + 1 || x > W - r - 2 || y < r + 1 || y > H - r - 2) continue;
        long long a = 0, b = 0, c = 0;
        for (int j = 0; j <= 2 * r; ++j) {
            const int h = (ly + j) * C + lx;
            a += Hs[0][h]; b += Hs[1][h]; c += Hs[2][h];
        }
        const unsigned long long D = (unsigned long long)((a - c) * (a - c)) + 4ull * (unsigned long long)(b * b);
        const long long score = a + c - (long long)ceil_sqrt_u64(D);
        const unsigned long long k = ((unsigned long long)score << 32) | (unsigned long long)(~(unsigned)idx);
        key = k > key ? k : key;
    }
    key = wave_max_u64(key);
    if ((tid & 63) == 0) wkey[tid >> 6] = key;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < T / 64; ++k) key = wkey[k] > key ? wkey[k] : key;
        int* o = out + 3 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        const long long score = (long long)(key >> 32);
        if (key != 0 && score >= (long long)min_score) {
            const int idx = (int)(~(unsigned)key);
            o[0] = x0 + idx % C; o[1] = y0 + idx / C; o[2] = (int)score;
        } else {
            o[0] = -1; o[1] = -1; o[2] = 0;
        }
    }
}

template <int C>
__global__ __launch_bounds__(C * C < 256 ? C * C : 256) void klt_score_kernel(const uint8_t* __restrict__ img, int W, int H, int stride, int r,
                                                                              int min_score, int* __restrict__ out) {
    klt_score_body<C>(img, W, H, stride, r, min_score, out);
}

// N3b: frame blockIdx.z lies frame_pitch bytes further, its triples 3 * slots ints further
template <int C>
__global__ __launch_bounds__(C * C < 256 ? C * C : 256) void klt_score_batch_kernel(const uint8_t* __restrict__ img, size_t frame_pitch, int W, int H,
                                                                                    int stride, int r, int min_score, int* __restrict__ out) {
    klt_score_body<C>(img + (size_t)blockIdx.z * frame_pitch, W, H, stride, r, min_score,
                      out + 3 * (size_t)blockIdx.z * ((size_t)gridDim.x * gridDim.y));
}

// S(img, q): bilinear sample at a 1/256-pixel position, pixel indices clamped into the frame, 8 fractional bits
__device__ __forceinline__ int klt_sample(const uint8_t* __restrict__ img, int W, int H, int stride, int qx, int qy) {
    const int ix = qx >> 8, iy = qy >> 8, fx = qx & 255, fy = qy & 255;
    const int xa = clampi(ix, 0, W - 1), xb = clampi(ix + 1, 0, W - 1);
    const uint8_t* ra = img + (size_t)clampi(iy, 0, H - 1) * stride;
    const uint8_t* rb = img + (size_t)clampi(iy + 1, 0, H - 1) * stride;
    const int s = (256 - fx) * (256 - fy) * (int)ra[xa] + fx * (256 - fy) * (int)ra[xb] + (256 - fx) * fy * (int)rb[xa] + fx * fy * (int)rb[xb];
    return (s + 128) >> 8;
}

// what one lane stores for a slot: statuses 1, 2 and 3 report dq = (0, 0) and res = 0; status 5 (FB alone) the forward pass's, as status 4
template <bool FB = false>
__device__ __forceinline__ void klt_store(const KltTrackParams& p, long long slot, int x, int y, int score, int dqx, int dqy, long long res, int status) {
    if (status != KLT_KEPT && status != KLT_RESIDUAL && !(FB && status == KLT_NO_RETURN)) { dqx = 0; dqy = 0; res = 0; }
    if (p.out_quad) {
        int* o = p.out_quad + 4 * (size_t)slot;
        o[0] = dqx; o[1] = dqy; o[2] = (int)res; o[3] = status;
    }
    if (p.out_slots) {
        int* o = p.out_slots + 6 * (size_t)slot;
        o[0] = status == KLT_NONE ? -1 : x; o[1] = status == KLT_NONE ? -1 : y; o[2] = status == KLT_NONE ? 0 : score;
        o[3] = dqx; o[4] = dqy; o[5] = status;
    }
    if (p.out_rec) {
        const float W0 = (float)p.lv.W[0], H0 = (float)p.lv.H[0];
        float4 rec = make_float4(0.f, 0.f, 0.f, 0.f);
        if (status == KLT_KEPT) rec = make_float4(((float)x + 0.5f) / W0, ((float)y + 0.5f) / H0, ((float)dqx / 256.0f) / W0, ((float)dqy / 256.0f) / H0);
        p.out_rec[slot] = rec;
        p.out_flag[slot] = status == KLT_KEPT ? 1 : 0;
    }
}

// N3f's kernels alone (where FB is true): a value, or a test, that is the same in every lane, told to the compiler, so that the branch on it is
// a scalar one and needs no saved exec mask -- with the second pass around the first the scalar registers run out otherwise.  Elsewhere the
// value as it is: the constant condition is folded before any instruction is chosen, so the plain kernels keep theirs
#define KLT_UNIFORM(v) (FB ? __builtin_amdgcn_readfirstlane(v) : (v))
#define KLT_UNIFORM_TEST(c) (FB ? __builtin_amdgcn_readfirstlane((int)(c)) != 0 : (c))

// level l of the slot's frame: the previous frame's, or with `second` the current frame's
template <bool BATCH>
__device__ __forceinline__ const uint8_t* klt_level(const KltTrackParams& p, const KltTrackBatchParams* b, size_t item, int l, bool second) {
    // the arrays are chosen, not the loaded values: where `second` is not a constant (N3f's kernels) one pointer and one pitch are loaded
    const uint8_t* const* base = second ? p.lv.cur : p.lv.prev;
    if constexpr (BATCH) return base[l] + item * (second ? b->cur_pitch : b->prev_pitch)[l];
    else return base[l];
}

__device__ __forceinline__ void klt_cmpx(int& a, int& b) { const int lo = a < b ? a : b, hi = a < b ? b : a; a = lo; b = hi; }

// N3p's predictor: the guess of lattice slot (cx, cy) from the previous pair's raw slots, 6 ints each -- the slot and its left, right, upper and
// lower neighbours, those inside the lattice with status 0; per component the element (k - 1) / 2 of the k values in ascending order, (0, 0)
// with none.  The missing candidates sort behind the others as INT_MAX (a value that is INT_MAX itself answers the same either way)
__device__ __forceinline__ void klt_predict_slot(const int* __restrict__ prev_slots, int nx, int ny, int cx, int cy, int& gx, int& gy) {
    const int ox[5] = {0, -1, 1, 0, 0}, oy[5] = {0, 0, 0, -1, 1};
    int vx[5], vy[5], k = 0;
    for (int c = 0; c < 5; ++c) {
        const int x = cx + ox[c], y = cy + oy[c];
        vx[c] = vy[c] = 0x7fffffff;
        if (x >= 0 && x < nx && y >= 0 && y < ny) {
            const int* s = prev_slots + 6 * ((size_t)y * nx + x);
            if (s[5] == KLT_KEPT) { vx[c] = s[3]; vy[c] = s[4]; ++k; }
        }
    }
    // five values in ascending order by nine compare-exchanges
    klt_cmpx(vx[0], vx[1]); klt_cmpx(vx[3], vx[4]); klt_cmpx(vx[2], vx[4]); klt_cmpx(vx[2], vx[3]); klt_cmpx(vx[0], vx[3]);
    klt_cmpx(vx[0], vx[2]); klt_cmpx(vx[1], vx[4]); klt_cmpx(vx[1], vx[3]); klt_cmpx(vx[1], vx[2]);
    klt_cmpx(vy[0], vy[1]); klt_cmpx(vy[3], vy[4]); klt_cmpx(vy[2], vy[4]); klt_cmpx(vy[2], vy[3]); klt_cmpx(vy[0], vy[3]);
    klt_cmpx(vy[0], vy[2]); klt_cmpx(vy[1], vy[4]); klt_cmpx(vy[1], vy[3]); klt_cmpx(vy[1], vy[2]);
    const int mid = (k - 1) >> 1;
    gx = k == 0 ? 0 : (mid == 0 ? vx[0] : (mid == 1 ? vx[1] : vx[2]));
    gy = k == 0 ? 0 : (mid == 0 ? vy[0] : (mid == 1 ? vy[1] : vy[2]));
}

// one wave's slot.  BATCH: the slot's item picks the frames (b: the launch's pitches) and, with shared features, its triple; the outputs are
// indexed by the slot either way.  Everything behind the pointers is one text for both kernels.  ZM: mean removal (N3m); the lines it adds
// are compiled into its own kernels alone.  MODE: KLT_MODE_PIXEL is N3 as it was, from the pixel (x, y), and compiles to the instructions it
// had.  The other two start a pass at a position P in 1/256 pixel -- the level's centre ((P + 128) >> l) - 128 and the frame test on
// P + dq * 2^l, which for P = 256 (x, y) are N3's values --: KLT_MODE_Q reads P from the points and runs one pass; KLT_MODE_FB (N3f) runs N3's
// pass from 256 (x, y) and, where it ends with status 0, a second pass from P = 256 (x, y) + dq with prev and cur exchanged.  PRED (N3p): a
// pass starts from the slot's guess g (the backward pass from -g) in place of dq = (0, 0); g is one value per wave, read or predicted once
// and held in scalar registers.  Its lines are compiled into its own kernels alone.  BATCH and PRED (N3pb): the launch's first wave is slot
// c->first_slot of the batch, and the guess is predicted from c->prev_slots at the slot's place within its item
template <bool BATCH, bool ZM, int MODE = KLT_MODE_PIXEL, bool PRED = false>
__device__ __forceinline__ void klt_track_body(const KltTrackParams& p, const KltTrackBatchParams* b, int* tmpl, const KltTrackPredParams* g = nullptr,
                                               const KltTrackBatchPredParams* c = nullptr) {
    constexpr bool FB = MODE == KLT_MODE_FB, AT_Q = MODE != KLT_MODE_PIXEL;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long slot = (long long)blockIdx.x * kKltTrackWaves + wave + (BATCH && PRED ? c->first_slot : 0);
    if (slot >= p.n) return;                                  // the whole wave
    int* I = tmpl + wave * kKltTemplatePitch;
    size_t item = 0;
    long long pt_slot = slot;
    if constexpr (BATCH) {                                    // slot < 2^31; the item is the same for the wave's lanes: a scalar
        item = (size_t)__builtin_amdgcn_readfirstlane((int)slot / b->slots_per_item);
        if (b->shared_features) pt_slot = slot - (long long)item * b->slots_per_item;
    }
    const int* pt = p.pts + (size_t)pt_slot * p.pt_stride;
    const int x = KLT_UNIFORM(pt[0]), y = KLT_UNIFORM(pt[1]), score = KLT_UNIFORM(p.from_features ? pt[2] : 0);      // KLT_MODE_Q: (Px, Py) in 1/256 pixel
    const int W0 = p.lv.W[0], H0 = p.lv.H[0];
    const int w = p.w, n = 2 * w + 1, n2 = n * n, m = n + 2;
    int status = KLT_KEPT, dqx = 0, dqy = 0;
    long long res = 0;
    if (p.from_features && x < 0) status = KLT_NONE;
    else if (MODE == KLT_MODE_Q ? (x < 0 || x > 256 * (W0 - 1) || y < 0 || y > 256 * (H0 - 1)) : (x < 0 || x >= W0 || y < 0 || y >= H0)) status = KLT_LEFT;
    if (status != KLT_KEPT) {                                 // no feature, or a point outside the frame: the wave leaves at once
        if (lane == 0) klt_store<FB>(p, slot, x, y, score, 0, 0, 0, status);
        return;
    }
    // the lane's window pixels lane + 64 k: their offsets from the window centre, and the template's value and gradients there
    int pi[4], pj[4], ix[4], iy[4], ic[4];
    for (int k = 0; k < 4; ++k) {
        const int q = lane + 64 * k;
        pj[k] = q / n; pi[k] = q - pj[k] * n;
        ix[k] = iy[k] = ic[k] = 0;
    }
    int px = MODE == KLT_MODE_Q ? x : 256 * x, py = MODE == KLT_MODE_Q ? y : 256 * y;      // the pass's start (read with AT_Q alone)
    int gx = 0, gy = 0;                                       // PRED: the slot's guess, 1/256 pixel at level 0
    if constexpr (PRED && BATCH) {
        // the wave's lattice cell, the slot's place within its item, as a scalar
        const int s = __builtin_amdgcn_readfirstlane((int)slot - (int)item * b->slots_per_item);
        if (c->prev_slots) klt_predict_slot(c->prev_slots, c->nx, c->ny, s % c->nx, s / c->nx, gx, gy);
        gx = __builtin_amdgcn_readfirstlane(gx); gy = __builtin_amdgcn_readfirstlane(gy);
        if (gx < -kKltMaxGuess || gx > kKltMaxGuess || gy < -kKltMaxGuess || gy > kKltMaxGuess) { gx = 0; gy = 0; }
        // with the second pass around the first, and the item's pitches beside it, two scalars that live through both passes are two more than
        // the scalar registers hold: the guess waits in the wave's template row, behind the 17 x 17 samples, and each pass reads it back
        // (every lane stores the same two words: a test on the lane here would be kept, as a mask in two scalar registers, for the store at the end)
        if constexpr (FB) { I[kKltTemplate] = gx; I[kKltTemplate + 1] = gy; }
    } else if constexpr (PRED) {
        const int s = __builtin_amdgcn_readfirstlane((int)slot);      // the wave's slot as a scalar: what is read below is read once per wave
        if (g->guesses) { gx = g->guesses[2 * (size_t)s]; gy = g->guesses[2 * (size_t)s + 1]; }
        else klt_predict_slot(g->prev_slots, g->nx, g->ny, s % g->nx, s / g->nx, gx, gy);
        gx = __builtin_amdgcn_readfirstlane(gx); gy = __builtin_amdgcn_readfirstlane(gy);
        if (gx < -kKltMaxGuess || gx > kKltMaxGuess || gy < -kKltMaxGuess || gy > kKltMaxGuess) { gx = 0; gy = 0; }
    }
    int fdqx = 0, fdqy = 0;                                   // FB: the forward pass's answer while the backward pass runs
    long long fres = 0;
    // one pass from (x, y) or, with AT_Q, from (px, py).  FB comes here a second time, with `back`: the two frames change places.  (A jump and
    // not a loop around the pass: a loop of one round changes the instructions the plain kernels are compiled to.)
    bool back = false;                                        // wave-uniform
another_pass: __attribute__((unused));
    {
    int cqx = 0, cqy = 0;
    if constexpr (PRED) {
        // dq = g >> (L - 1) (the backward pass: -g), unless N3's frame test fails on the start: then (0, 0).  |g| <= 2^23 and a start inside the
        // frame: every dq of the pass stays an int as it does without a guess
        const int sh = p.L - 1;
        if constexpr (BATCH && FB) {
            wave_sync();
            gx = __builtin_amdgcn_readfirstlane(I[kKltTemplate]); gy = __builtin_amdgcn_readfirstlane(I[kKltTemplate + 1]);
        }
        const int sx = (back ? -gx : gx) >> sh, sy = (back ? -gy : gy) >> sh;
        const long long fx = (AT_Q ? (long long)px : 256ll * x) + (long long)sx * (1ll << sh), fy = (AT_Q ? (long long)py : 256ll * y) + (long long)sy * (1ll << sh);
        const bool out = __builtin_amdgcn_readfirstlane((int)(fx < 0 || fx > 256ll * (W0 - 1) || fy < 0 || fy > 256ll * (H0 - 1))) != 0;
        dqx = out ? 0 : sx; dqy = out ? 0 : sy;
    }
    for (int l = p.L - 1; l >= 0 && KLT_UNIFORM(status) == KLT_KEPT; --l) {
        const uint8_t* __restrict__ prev = klt_level<BATCH>(p, b, item, l, back);
        const uint8_t* __restrict__ cur = klt_level<BATCH>(p, b, item, l, !back);
        const int Wl = p.lv.W[l], Hl = p.lv.H[l], sl = p.lv.stride[l];
        if constexpr (AT_Q) {
            cqx = ((px + 128) >> l) - 128;
            cqy = ((py + 128) >> l) - 128;
        } else {
            cqx = (((2 * x + 1) * 128) >> l) - 128;
            cqy = (((2 * y + 1) * 128) >> l) - 128;
        }
        wave_sync();                                          // the previous level's template has been read
        for (int idx = lane; idx < m * m; idx += 64) {
            const int j = idx / m, i = idx - j * m;
            I[idx] = klt_sample(prev, Wl, Hl, sl, cqx + 256 * (i - w - 1), cqy + 256 * (j - w - 1));
        }
        wave_sync();
        long long a11 = 0, a12 = 0, a22 = 0;
        for (int k = 0; k < 4; ++k) {
            if (lane + 64 * k < n2) {
                const int c = (pj[k] + 1) * m + pi[k] + 1;
                ix[k] = I[c + 1] - I[c - 1]; iy[k] = I[c + m] - I[c - m]; ic[k] = I[c];
                a11 += (long long)ix[k] * ix[k]; a12 += (long long)ix[k] * iy[k]; a22 += (long long)iy[k] * iy[k];
            }
        }
        a11 = wave_sum_i64(a11); a12 = wave_sum_i64(a12); a22 = wave_sum_i64(a22);
        const long long T = (long long)p.min_eig * n2 * 262144ll * (ZM ? n2 : 1);
        if constexpr (ZM) {
            // N3m: A of the model "shift plus one offset", the offset eliminated; every term stays below 9e14.  From here on ix, iy hold the
            // centred gradients, whose products with d sum to N3m's b1, b2
            // sx and sy stay below 3e7 in magnitude, so both go through ONE 64-bit reduction, sx in the upper word: the sum's lower word is sy
            long long sxy = 0;
            for (int k = 0; k < 4; ++k) sxy += (long long)ix[k] * 4294967296ll + iy[k];      // (0 where the lane has no pixel)
            sxy = wave_sum_i64(sxy);
            const int sy = (int)(unsigned)(unsigned long long)sxy;
            const int sx = (int)((sxy - sy) / 4294967296ll);
            a11 = n2 * a11 - (long long)sx * sx; a12 = n2 * a12 - (long long)sx * sy; a22 = n2 * a22 - (long long)sy * sy;
            for (int k = 0; k < 4; ++k) {
                if (lane + 64 * k < n2) { ix[k] = n2 * ix[k] - sx; iy[k] = n2 * iy[k] - sy; }
            }
        }
        const double X = (double)(a11 - T), Y = (double)(a22 - T), Z = (double)a12;
        const double xy = X * Y, zz = Z * Z;
        if (KLT_UNIFORM_TEST(!(xy >= zz && X + Y >= 0.0))) { status = KLT_FLAT; break; }
        const double A11 = (double)a11, A22 = (double)a22;
        const double det = A11 * A22 - zz;
        if (KLT_UNIFORM_TEST(det <= 0.0)) { status = KLT_FLAT; break; }
        const double lim = 256.0 * w;
        for (int it = 0; it < p.K; ++it) {
            const long long fx = (AT_Q ? (long long)px : 256ll * x) + (long long)dqx * (1ll << l), fy = (AT_Q ? (long long)py : 256ll * y) + (long long)dqy * (1ll << l);
            if (KLT_UNIFORM_TEST(fx < 0 || fx > 256ll * (W0 - 1) || fy < 0 || fy > 256ll * (H0 - 1))) { status = KLT_LEFT; break; }
            long long b1 = 0, b2 = 0;
            for (int k = 0; k < 4; ++k) {
                if (lane + 64 * k < n2) {
                    const int d = klt_sample(cur, Wl, Hl, sl, cqx + dqx + 256 * (pi[k] - w), cqy + dqy + 256 * (pj[k] - w)) - ic[k];
                    b1 += (long long)d * ix[k]; b2 += (long long)d * iy[k];
                }
            }
            b1 = wave_sum_i64(b1); b2 = wave_sum_i64(b2);
            const double B1 = (double)b1, B2 = (double)b2;
            const double t1 = A22 * B1, t2 = Z * B2, t3 = A11 * B2, t4 = Z * B1;
            const double num_x = t1 - t2, num_y = t3 - t4;
            const double ux = (-512.0 * num_x) / det, uy = (-512.0 * num_y) / det;
            const int uqx = (int)rint(fmin(fmax(ux, -lim), lim)), uqy = (int)rint(fmin(fmax(uy, -lim), lim));
            dqx += uqx; dqy += uqy;
            if (KLT_UNIFORM(uqx) == 0 && KLT_UNIFORM(uqy) == 0) break;
        }
        if (KLT_UNIFORM(status) != KLT_KEPT) break;
        if (l > 0) { dqx *= 2; dqy *= 2; }
    }
    if (KLT_UNIFORM(status) == KLT_KEPT) {
        const long long fx = (AT_Q ? (long long)px : 256ll * x) + dqx, fy = (AT_Q ? (long long)py : 256ll * y) + dqy;
        if (fx < 0 || fx > 256ll * (W0 - 1) || fy < 0 || fy > 256ll * (H0 - 1)) status = KLT_LEFT;
    }
    if (KLT_UNIFORM(status) == KLT_KEPT) {
        const uint8_t* __restrict__ cur0 = klt_level<BATCH>(p, b, item, 0, !back);
        long long sum = 0;
        if constexpr (ZM) {
            // N3m: the residual around the window's mean difference m = floor((2 sd + N) / (2 N)), |m| <= 65,280
            int d[4], sd = 0;                                     // |sd| <= 225 * 65,280: a 32-bit reduction
            for (int k = 0; k < 4; ++k) {
                d[k] = 0;
                if (lane + 64 * k < n2) {
                    d[k] = klt_sample(cur0, W0, H0, p.lv.stride[0], cqx + dqx + 256 * (pi[k] - w), cqy + dqy + 256 * (pj[k] - w)) - ic[k];
                    sd += d[k];
                }
            }
            sd = wave_sum_i32(sd);
            const int num = 2 * sd + n2, den = 2 * n2;
            const int mean = num / den - (num % den < 0 ? 1 : 0);
            for (int k = 0; k < 4; ++k) {
                if (lane + 64 * k < n2) { const int e = d[k] - mean; sum += e < 0 ? -e : e; }
            }
        } else {
            for (int k = 0; k < 4; ++k) {
                if (lane + 64 * k < n2) {
                    const int d = klt_sample(cur0, W0, H0, p.lv.stride[0], cqx + dqx + 256 * (pi[k] - w), cqy + dqy + 256 * (pj[k] - w)) - ic[k];
                    sum += d < 0 ? -d : d;
                }
            }
        }
        res = wave_sum_i64(sum);
        if (p.max_residual > 0 && res > 16ll * p.max_residual * n2) status = KLT_RESIDUAL;
    }
    }
    if constexpr (FB) {
        // N3f: the kernel holds the pass's text once.  Every value here is the same in all lanes: the wave takes one way.  The forward pass's
        // final frame test has put P inside the frame, and a kept |dq| is below 256 * 32768, so everything fits an int
        if (!back) {
            // a forward pass that fails leaves as it does without the check.  The test and the new start are scalars, so that `back`, what it
            // selects and the levels' centres stay in scalar registers: 92 / 94 vector registers, five waves per SIMD as the plain kernels
            if (__builtin_amdgcn_readfirstlane(status) == KLT_KEPT) {
                fdqx = dqx; fdqy = dqy; fres = res;
                px = __builtin_amdgcn_readfirstlane(px + dqx); py = __builtin_amdgcn_readfirstlane(py + dqy);
                dqx = 0; dqy = 0; res = 0;
                back = true;
                goto another_pass;
            }
        } else {
            const int ex = fdqx + dqx, ey = fdqy + dqy;
            const int ax = ex < 0 ? -ex : ex, ay = ey < 0 ? -ey : ey;
            status = (status == KLT_KEPT && (ax > ay ? ax : ay) < p.fb_limit) ? KLT_KEPT : KLT_NO_RETURN;
            dqx = fdqx; dqy = fdqy; res = fres;
        }
    }
    if (lane == 0) klt_store<FB>(p, slot, x, y, score, dqx, dqy, res, status);
}

#undef KLT_UNIFORM
#undef KLT_UNIFORM_TEST

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_kernel(const KltTrackParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<false, false>(p, nullptr, tmpl);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_batch_kernel(const KltTrackBatchParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<true, false>(p.t, &p, tmpl);
}

// N3m: the two kernels of a context whose mean_removal is 1
__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_zm_kernel(const KltTrackParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<false, true>(p, nullptr, tmpl);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_batch_zm_kernel(const KltTrackBatchParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<true, true>(p.t, &p, tmpl);
}

// N3f: the four kernels of a context whose fb_limit is above 0, and the two of the stage form ofps_hip_klt_track_q
__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_fb_kernel(const KltTrackParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<false, false, KLT_MODE_FB>(p, nullptr, tmpl);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_batch_fb_kernel(const KltTrackBatchParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<true, false, KLT_MODE_FB>(p.t, &p, tmpl);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_zm_fb_kernel(const KltTrackParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<false, true, KLT_MODE_FB>(p, nullptr, tmpl);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_batch_zm_fb_kernel(const KltTrackBatchParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<true, true, KLT_MODE_FB>(p.t, &p, tmpl);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_q_kernel(const KltTrackParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<false, false, KLT_MODE_Q>(p, nullptr, tmpl);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_q_zm_kernel(const KltTrackParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<false, true, KLT_MODE_Q>(p, nullptr, tmpl);
}

// N3p: the four one-pair kernels whose tracks start from a guess, and the predictor's stage form (a lane per slot)
__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_pred_kernel(const KltTrackPredParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<false, false, KLT_MODE_PIXEL, true>(p.t, nullptr, tmpl, &p);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_pred_zm_kernel(const KltTrackPredParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<false, true, KLT_MODE_PIXEL, true>(p.t, nullptr, tmpl, &p);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_pred_fb_kernel(const KltTrackPredParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<false, false, KLT_MODE_FB, true>(p.t, nullptr, tmpl, &p);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_pred_zm_fb_kernel(const KltTrackPredParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<false, true, KLT_MODE_FB, true>(p.t, nullptr, tmpl, &p);
}

// N3pb: the four batch kernels whose launch is one item, started from the item before
__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_batch_pred_kernel(const KltTrackBatchPredParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<true, false, KLT_MODE_PIXEL, true>(p.b.t, &p.b, tmpl, nullptr, &p);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_batch_pred_zm_kernel(const KltTrackBatchPredParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<true, true, KLT_MODE_PIXEL, true>(p.b.t, &p.b, tmpl, nullptr, &p);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_batch_pred_fb_kernel(const KltTrackBatchPredParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<true, false, KLT_MODE_FB, true>(p.b.t, &p.b, tmpl, nullptr, &p);
}

__global__ __launch_bounds__(64 * kKltTrackWaves) void klt_track_batch_pred_zm_fb_kernel(const KltTrackBatchPredParams p) {
    __shared__ int tmpl[kKltTrackWaves * kKltTemplatePitch];
    klt_track_body<true, true, KLT_MODE_FB, true>(p.b.t, &p.b, tmpl, nullptr, &p);
}

__global__ __launch_bounds__(256) void klt_predict_kernel(const int* __restrict__ prev_slots, int nx, int ny, int* __restrict__ out) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= (long long)nx * ny) return;
    int gx, gy;
    klt_predict_slot(prev_slots, nx, ny, (int)(s % nx), (int)(s / nx), gx, gy);
    out[2 * s] = gx; out[2 * s + 1] = gy;
}

struct KltSettings { int cell, r, min_score, min_eig, max_residual; };

KltSettings klt_settings(const ofps_hip_ctx* ctx) {
    return {ctx->opt.klt_cell, ctx->opt.klt_score_radius, ctx->opt.klt_min_score, ctx->opt.klt_min_eig, ctx->opt.klt_max_residual};
}

int klt_check_settings(ofps_hip_ctx* ctx, int cell, int r, int min_score, int min_eig, int max_residual, const char* who) {
    OFPS_REQUIRE(ctx, cell == 8 || cell == 16 || cell == 32, "%s: cell %d is not 8|16|32", who, cell);
    OFPS_REQUIRE(ctx, r >= 1 && r <= kKltMaxScoreRadius, "%s: score_radius %d outside [1, %d]", who, r, kKltMaxScoreRadius);
    OFPS_REQUIRE(ctx, min_score >= 1, "%s: min_score %d outside [1, 2^31 - 1]", who, min_score);
    OFPS_REQUIRE(ctx, min_eig >= 1 && min_eig <= kKltMaxMinEig, "%s: min_eig %d outside [1, 65535]", who, min_eig);
    OFPS_REQUIRE(ctx, max_residual >= 0 && max_residual <= kKltMaxResidual, "%s: max_residual %d outside [0, 4080]", who, max_residual);
    return OFPS_HIP_OK;
}

int klt_check_frame(ofps_hip_ctx* ctx, int W, int H, int stride, int levels, const char* who) {
    OFPS_REQUIRE(ctx, levels >= 1 && levels <= kKltMaxLevels, "%s: levels %d outside [1, %d]", who, levels, kKltMaxLevels);
    OFPS_REQUIRE(ctx, W >= 8 && H >= 8 && W <= 32768 && H <= 32768 && stride >= W, "%s: bad geometry W=%d H=%d stride=%d", who, W, H, stride);
    OFPS_REQUIRE(ctx, (W >> (levels - 1)) >= 8 && (H >> (levels - 1)) >= 8, "%s: a %d x %d frame has no %d levels of at least 8 x 8", who, W, H,
                 levels);
    return OFPS_HIP_OK;
}

inline size_t klt_slots(int W, int H, int cell) { return klt_lattice(W, H, cell).slots(); }
inline size_t pad16(size_t b) { return (b + 15) & ~size_t(15); }

// the two arrays of raw slots of a call with prediction: a wave reads its neighbours' previous slots while other waves, and in a batch later the
// other items, write theirs, so the two must not share a byte
int klt_check_apart(ofps_hip_ctx* ctx, const void* d_prev_slots, size_t prev_bytes, const void* d_out_slots, size_t out_bytes, const char* who) {
    const char* a = static_cast<const char*>(d_prev_slots);
    const char* b = static_cast<const char*>(d_out_slots);
    OFPS_REQUIRE(ctx, !a || !b || a + prev_bytes <= b || b + out_bytes <= a, "%s: d_prev_slots and d_out_slots overlap", who);
    return OFPS_HIP_OK;
}

int klt_features_device(ofps_hip_ctx* ctx, const uint8_t* d_img, int W, int H, int stride, const KltSettings& s, int* d_out) {
    const KltLattice lat = klt_lattice(W, H, s.cell);
    const dim3 grid(lat.nx, lat.ny);
    if (s.cell == 8) hipLaunchKernelGGL(klt_score_kernel<8>, grid, dim3(64), 0, ctx->stream, d_img, W, H, stride, s.r, s.min_score, d_out);
    else if (s.cell == 16) hipLaunchKernelGGL(klt_score_kernel<16>, grid, dim3(256), 0, ctx->stream, d_img, W, H, stride, s.r, s.min_score, d_out);
    else hipLaunchKernelGGL(klt_score_kernel<32>, grid, dim3(256), 0, ctx->stream, d_img, W, H, stride, s.r, s.min_score, d_out);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// The track kernels of one parameter struct, [N3f's check on][N3m's mean removal on], and THE track launch: `waves` slots, four to a workgroup,
// the kernel the context's two settings pick.  The stage form ofps_hip_klt_track_q runs one direction whatever the check's setting is: its
// table holds the same row twice
template <class P> using KltTrackKernels = void (*const[2][2])(P);
constexpr KltTrackKernels<KltTrackParams> kKltTrack = {{klt_track_kernel, klt_track_zm_kernel}, {klt_track_fb_kernel, klt_track_zm_fb_kernel}};
constexpr KltTrackKernels<KltTrackParams> kKltTrackQ = {{klt_track_q_kernel, klt_track_q_zm_kernel}, {klt_track_q_kernel, klt_track_q_zm_kernel}};
constexpr KltTrackKernels<KltTrackPredParams> kKltTrackPred = {{klt_track_pred_kernel, klt_track_pred_zm_kernel},
                                                               {klt_track_pred_fb_kernel, klt_track_pred_zm_fb_kernel}};
constexpr KltTrackKernels<KltTrackBatchParams> kKltTrackBatch = {{klt_track_batch_kernel, klt_track_batch_zm_kernel},
                                                                 {klt_track_batch_fb_kernel, klt_track_batch_zm_fb_kernel}};
constexpr KltTrackKernels<KltTrackBatchPredParams> kKltTrackBatchPred = {{klt_track_batch_pred_kernel, klt_track_batch_pred_zm_kernel},
                                                                         {klt_track_batch_pred_fb_kernel, klt_track_batch_pred_zm_fb_kernel}};

template <class P>
int klt_track_launch(ofps_hip_ctx* ctx, KltTrackKernels<P>& kernels, long long waves, const P& p) {
    if (waves <= 0) return OFPS_HIP_OK;
    const dim3 grid((unsigned)((waves + kKltTrackWaves - 1) / kKltTrackWaves));
    hipLaunchKernelGGL(kernels[ctx->opt.klt_fb > 0][ctx->opt.klt_mean_removal != 0], grid, dim3(64 * kKltTrackWaves), 0, ctx->stream, p);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// what every track launch takes from the context and the call; the callers add the levels, the points and the outputs.  fb_limit (N3f) is above 0
// exactly when the launch picks the FB kernels, which alone read it
void klt_track_settings(const ofps_hip_ctx* ctx, int levels, int radius, int iters, KltTrackParams* p) {
    p->L = levels; p->w = radius; p->K = iters; p->min_eig = ctx->opt.klt_min_eig; p->max_residual = ctx->opt.klt_max_residual;
    p->fb_limit = ctx->opt.klt_fb;
}

int klt_predict_device(ofps_hip_ctx* ctx, const int* d_prev_slots, int W, int H, int cell, int* d_out) {
    const KltLattice lat = klt_lattice(W, H, cell);
    const int nx = lat.nx, ny = lat.ny;
    const size_t ns = lat.slots();
    hipLaunchKernelGGL(klt_predict_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, ctx->stream, d_prev_slots, nx, ny, d_out);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// ---- N3b: the batch form's three steps, each one launch (the pyramid: one per level) whatever the number of pairs
// `frames` frames `pitch` bytes apart -> their triples, 3 * slots ints apart
int klt_features_batch_device(ofps_hip_ctx* ctx, const uint8_t* d_img, size_t pitch, int frames, int W, int H, int stride, const KltSettings& s,
                              int* d_out) {
    OFPS_REQUIRE(ctx, frames >= 1 && frames <= 65535, "klt_flow_batch: %d frames to score (at most 65535)", frames);
    const KltLattice lat = klt_lattice(W, H, s.cell);
    const dim3 grid(lat.nx, lat.ny, frames);
    if (s.cell == 8) hipLaunchKernelGGL(klt_score_batch_kernel<8>, grid, dim3(64), 0, ctx->stream, d_img, pitch, W, H, stride, s.r, s.min_score, d_out);
    else if (s.cell == 16) hipLaunchKernelGGL(klt_score_batch_kernel<16>, grid, dim3(256), 0, ctx->stream, d_img, pitch, W, H, stride, s.r, s.min_score, d_out);
    else hipLaunchKernelGGL(klt_score_batch_kernel<32>, grid, dim3(256), 0, ctx->stream, d_img, pitch, W, H, stride, s.r, s.min_score, d_out);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// the levels above 0 of the distinct frames of `pairs` pairs in S_KLT_PYR -> b->t.lv (the levels' bases) and the levels' pitches.  A chain
// (consecutive pairs of one sequence) or a key frame followed by its current frames is one run of frames: one halving per level; two unrelated
// sets take two.  One pair of two frames anywhere (both pitches 0, pairs = 1) is two sets of one frame: two halvings per level, cur's copy one
// frame behind prev's -- the one-pair forms' pyramid, whose kernels read b->t.lv and no pitch
int klt_pyramid_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int levels, KltTrackBatchParams* b) {
    KltLevels* lv = &b->t.lv;
    const SadFrames::Sets sets = f.sets(pairs);
    const bool key_run = !sets.chain && !sets.prev_many && sets.cur_many && f.cur_base == f.prev_base + f.cur_pitch;      // frames 0, 1 .. pairs of one sequence
    const long long total = sets.nprev + sets.ncur;
    size_t off[kKltMaxLevels] = {}, bytes = 0;
    lv->prev[0] = f.prev_base; lv->cur[0] = f.cur_base; lv->W[0] = f.W; lv->H[0] = f.H; lv->stride[0] = f.stride;
    b->prev_pitch[0] = f.prev_pitch; b->cur_pitch[0] = f.cur_pitch;
    for (int l = 1; l < kKltMaxLevels; ++l) {
        lv->prev[l] = lv->cur[l] = nullptr;
        lv->W[l] = lv->H[l] = lv->stride[l] = 0;
        b->prev_pitch[l] = b->cur_pitch[l] = 0;
        if (l >= levels) continue;
        lv->W[l] = lv->W[l - 1] >> 1; lv->H[l] = lv->H[l - 1] >> 1;
        lv->stride[l] = ofps::padded_stride(lv->W[l]);
        off[l] = bytes; bytes += (size_t)total * lv->stride[l] * lv->H[l];
    }
    if (levels == 1) return OFPS_HIP_OK;
    auto* pyr = static_cast<uint8_t*>(scratch(ctx, S_KLT_PYR, bytes));
    if (!pyr) return OFPS_HIP_ENOMEM;
    for (int l = 1; l < levels; ++l) {
        const size_t pitch = (size_t)lv->stride[l] * lv->H[l];
        uint8_t* dp = pyr + off[l];
        uint8_t* dc = dp + (size_t)sets.cur_first() * pitch;
        const int Wp = lv->W[l - 1], Hp = lv->H[l - 1], sp = lv->stride[l - 1];
        int rc;
        if (sets.chain) rc = sad_down2_frames_device(ctx, lv->prev[l - 1], b->prev_pitch[l - 1], Wp, Hp, sp, dp, pitch, lv->stride[l], sets.nprev);
        else if (key_run) rc = sad_down2_frames_device(ctx, lv->prev[l - 1], b->cur_pitch[l - 1], Wp, Hp, sp, dp, pitch, lv->stride[l], total);
        else {
            rc = sad_down2_frames_device(ctx, lv->prev[l - 1], b->prev_pitch[l - 1], Wp, Hp, sp, dp, pitch, lv->stride[l], sets.nprev);
            if (rc == OFPS_HIP_OK) rc = sad_down2_frames_device(ctx, lv->cur[l - 1], b->cur_pitch[l - 1], Wp, Hp, sp, dc, pitch, lv->stride[l], sets.ncur);
        }
        if (rc != OFPS_HIP_OK) return rc;
        lv->prev[l] = dp; lv->cur[l] = dc;
        b->prev_pitch[l] = sets.prev_many ? pitch : 0; b->cur_pitch[l] = sets.cur_many ? pitch : 0;
    }
    return OFPS_HIP_OK;
}

// N3pb: `pairs` launches, one item each, in item order on ctx->stream.  Item k writes its raw slots where the caller wants them (b.t.out_slots,
// item-major: the caller's array, or S_KLT_WORK's), the last item into d_last_slots if that is given; item k + 1 reads them there.  Item 0 reads
// d_prev_slots (null: zero guesses).  No launch reads the array it writes: the items' slots are ns apart, and the callers keep d_prev_slots
// and d_last_slots apart from each other and from the rest
// intra (N3i, optional): item k's verdict and cut are enqueued behind its track launch
int klt_track_chained_launch(ofps_hip_ctx* ctx, const KltTrackBatchParams& b, int pairs, KltLattice lat, const int* d_prev_slots, int* d_last_slots,
                             const KltIntraCall* intra) {
    const int ns = b.slots_per_item;
    int* const all = b.t.out_slots;                           // 6 ints per slot of the batch
    const int* prev = d_prev_slots;
    for (int k = 0; k < pairs; ++k) {
        KltTrackBatchPredParams f{b, prev, k * ns, lat.nx, lat.ny};
        f.b.t.n = (k + 1) * ns;
        int* mine = all + 6 * (size_t)k * ns;
        if (k == pairs - 1 && d_last_slots) {
            // the kernel stores at 6 * slot behind out_slots, slot counted from the batch's first: this item's slots land in d_last_slots
            mine = d_last_slots;
            f.b.t.out_slots = reinterpret_cast<int*>(reinterpret_cast<uintptr_t>(d_last_slots) - 6 * (size_t)k * ns * sizeof(int));
        }
        int rc = klt_track_launch(ctx, kKltTrackBatchPred, ns, f);
        // N3i: statuses 6 and 7 stand in `mine` before the next launch's predictor reads it
        if (rc == OFPS_HIP_OK && intra) rc = klt_intra_device(ctx, *intra, k, 1, f.b.t.out_slots);
        if (rc != OFPS_HIP_OK) return rc;
        prev = mine;
    }
    return OFPS_HIP_OK;
}

int klt_check_sequence(ofps_hip_ctx* ctx, int n_frames, int H, int stride, size_t frame_pitch, int ref_mode, const char* who) {
    OFPS_REQUIRE(ctx, n_frames >= 2 && n_frames <= 65536, "%s: n_frames %d outside [2, 65536]", who, n_frames);
    OFPS_REQUIRE(ctx, ref_mode == 0 || ref_mode == 1, "%s: ref_mode %d is not 0|1", who, ref_mode);
    OFPS_REQUIRE(ctx, frame_pitch >= (size_t)stride * H, "%s: frame_pitch %zu is below stride * H = %zu", who, frame_pitch, (size_t)stride * H);
    return OFPS_HIP_OK;
}

// S_KLT_WORK of one run, every part on a multiple of 16 bytes: [triples of the `scored` distinct prev frames][raw records, pairs x slots]
// [keep flags, pairs x slots]; own_slots (a chained batch whose caller takes no slots): [raw slots, 6 i32 per slot of the batch], dead behind the
// last track launch; intra (N3i): [the tracks' quads, 4 i32 per slot of the batch][candidate and intra counters, 2 x u32 per item]
struct KltWork {
    int* feat; float4* raw; uint8_t* flag;
    int* slots; int* quad; uint32_t* cnt;                     // null where the run has none
    bool make(ofps_hip_ctx* ctx, int pairs, int scored, size_t ns, bool own_slots, bool intra) {
        const size_t total = (size_t)pairs * ns;
        const size_t o_raw = pad16((size_t)scored * ns * 3 * sizeof(int)), o_flag = o_raw + total * sizeof(float4), o_slots = o_flag + pad16(total);
        const size_t end_slots = o_slots + (own_slots ? total * 6 * sizeof(int) : 0);
        const size_t o_quad = pad16(end_slots), o_cnt = o_quad + total * 4 * sizeof(int);
        auto* work = static_cast<char*>(scratch(ctx, S_KLT_WORK, intra ? o_cnt + pad16((size_t)pairs * 2 * sizeof(uint32_t)) : end_slots));
        if (!work) return false;
        feat = reinterpret_cast<int*>(work); raw = reinterpret_cast<float4*>(work + o_raw); flag = reinterpret_cast<uint8_t*>(work + o_flag);
        slots = own_slots ? reinterpret_cast<int*>(work + o_slots) : nullptr;
        quad = intra ? reinterpret_cast<int*>(work + o_quad) : nullptr;
        cnt = intra ? reinterpret_cast<uint32_t*>(work + o_cnt) : nullptr;
        return true;
    }
};

}  // namespace

namespace ofps {

// what every call of the decoder refuses, the stage forms and the dense decoders' stream forms alike
int klt_check_call(ofps_hip_ctx* ctx, int W, int H, int stride, int levels, int radius, int iters, const char* who) {
    const int rc = klt_check_frame(ctx, W, H, stride, levels, who);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_REQUIRE(ctx, radius >= 1 && radius <= kKltMaxRadius, "%s: radius %d outside [1, %d]", who, radius, kKltMaxRadius);
    OFPS_REQUIRE(ctx, iters >= 1 && iters <= kKltMaxIters, "%s: iters %d outside [1, %d]", who, iters, kKltMaxIters);
    return OFPS_HIP_OK;
}

// THE driver of every flow form (common.hpp: KltFlowCall).  Both scratch slots are written and read on ctx->stream alone and are dead behind the
// compaction, so two tickets of the batched stream share them; scratch() waits for that stream before it frees a slot it has to grow, which is
// all the order they need.  One pair of the one-pair form is the batch form at pairs = 1 in everything but the kernels: the two branch where
// those differ, the score launch and the track launch, and nowhere else
int klt_flow_device(ofps_hip_ctx* ctx, const KltFlowCall& c) {
    const SadFrames& f = c.f;
    const KltSettings s = klt_settings(ctx);
    const KltLattice lat = klt_lattice(f.W, f.H, s.cell);
    const size_t ns = lat.slots();
    const int pairs = c.pairs;
    OFPS_REQUIRE(ctx, pairs >= 1 && (unsigned long long)pairs * ns < (1ull << 31), "klt_flow_batch: %d pairs of %zu slots (pairs * slots must stay below 2^31)",
                 pairs, ns);
    const int scored = f.prev_pitch ? pairs : 1;              // the distinct prev frames
    const int intra = ctx->opt.klt_intra;
    KltWork w;
    if (!w.make(ctx, pairs, scored, ns, c.chained && !c.d_slots, intra > 0)) return OFPS_HIP_ENOMEM;
    int* const d_slots = w.slots ? w.slots : c.d_slots;
    int rc = c.batch ? klt_features_batch_device(ctx, f.prev_base, f.prev_pitch, scored, f.W, f.H, f.stride, s, w.feat)
                     : klt_features_device(ctx, f.prev_base, f.W, f.H, f.stride, s, w.feat);
    if (rc != OFPS_HIP_OK) return rc;
    KltTrackBatchParams b{};
    rc = klt_pyramid_device(ctx, f, pairs, c.levels, &b);
    if (rc != OFPS_HIP_OK) return rc;
    KltTrackParams& p = b.t;
    klt_track_settings(ctx, c.levels, c.radius, c.iters, &p);
    p.pts = w.feat; p.pt_stride = 3; p.from_features = 1; p.n = (int)(pairs * ns);
    p.out_quad = w.quad; p.out_slots = d_slots; p.out_rec = w.raw; p.out_flag = w.flag;
    b.slots_per_item = (int)ns; b.shared_features = f.prev_pitch ? 0 : 1;
    // N3i: the verdict, and the cut, rewrite flags and statuses in front of the compaction -- and of the track launch that reads these raw slots
    // next on this stream: the next pair's, or in a chained batch item k + 1's, so there item k's verdict goes right behind item k's launch
    KltIntraCall ic{};
    if (intra > 0) {
        OFPS_HIP_TRY(ctx, hipMemsetAsync(w.cnt, 0, (size_t)pairs * 2 * sizeof(uint32_t), ctx->stream));
        ic = KltIntraCall{f.prev_base, f.prev_pitch, f.W, f.H, f.stride, c.radius, (int)ns, w.feat, f.prev_pitch ? ns * 3 : 0, w.quad, w.flag, w.cnt,
                          intra, ctx->opt.klt_cut};
    }
    if (c.chained) rc = klt_track_chained_launch(ctx, b, pairs, lat, c.d_prev_slots, c.d_last_slots, intra > 0 ? &ic : nullptr);
    else {
        if (c.batch) rc = klt_track_launch(ctx, kKltTrackBatch, p.n, b);
        // N3p: the predictor runs inside the track kernel, in front of the wave's first level: no launch and no array of guesses between the two
        else if (c.d_prev_slots) rc = klt_track_launch(ctx, kKltTrackPred, p.n, KltTrackPredParams{p, nullptr, c.d_prev_slots, lat.nx, lat.ny});
        else rc = klt_track_launch(ctx, kKltTrack, p.n, p);
        if (rc == OFPS_HIP_OK && intra > 0) rc = klt_intra_device(ctx, ic, 0, pairs, d_slots);
    }
    if (rc != OFPS_HIP_OK) return rc;
    // one workgroup per item is right for a batch; ONE pair through it would scan a 4K frame's 129,600 slots on one compute unit (measured:
    // 5 % of the pair's time), so a batch of one pair keeps the one-pair form's compactions, as SadFilter::finish does (sad_gate.hip)
    if (pairs == 1) return ns <= kCompactSmallMax ? compact_small_device(ctx, w.raw, w.flag, ns, c.d_out, c.d_counts) : compact_entries_device(ctx, w.raw, w.flag, ns, c.d_out, c.d_counts);
    return compact_items_device(ctx, w.raw, w.flag, ns, pairs, c.d_out, c.d_counts);
}

int klt_flow_device(ofps_hip_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_cur, int W, int H, int stride, int levels, int radius, int iters,
                    float4* d_out, uint32_t* d_count, int* d_slots, const int* d_prev_slots) {
    return klt_flow_device(ctx, KltFlowCall{SadFrames{d_prev, d_cur, 0, 0, W, H, stride}, 1, levels, radius, iters, d_out, d_count, d_slots, false, false,
                                            d_prev_slots, nullptr});
}

}  // namespace ofps

extern "C" {

int ofps_hip_set_klt(ofps_hip_ctx* ctx, int cell, int score_radius, int min_score, int min_eig, int max_residual) {
    if (!ctx) return OFPS_HIP_EINVAL;
    const int rc = klt_check_settings(ctx, cell, score_radius, min_score, min_eig, max_residual, "set_klt");
    if (rc != OFPS_HIP_OK) return rc;
    ctx->opt.klt_cell = cell; ctx->opt.klt_score_radius = score_radius; ctx->opt.klt_min_score = min_score;
    ctx->opt.klt_min_eig = min_eig; ctx->opt.klt_max_residual = max_residual;
    return OFPS_HIP_OK;
}

int ofps_hip_get_klt(ofps_hip_ctx* ctx, int32_t* cell, int32_t* score_radius, int32_t* min_score, int32_t* min_eig, int32_t* max_residual) {
    if (!ctx) return OFPS_HIP_EINVAL;
    if (cell) *cell = ctx->opt.klt_cell;
    if (score_radius) *score_radius = ctx->opt.klt_score_radius;
    if (min_score) *min_score = ctx->opt.klt_min_score;
    if (min_eig) *min_eig = ctx->opt.klt_min_eig;
    if (max_residual) *max_residual = ctx->opt.klt_max_residual;
    return OFPS_HIP_OK;
}

int ofps_hip_set_klt_mean_removal(ofps_hip_ctx* ctx, int on) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, on == 0 || on == 1, "set_klt_mean_removal: %d is not 0|1", on);
    ctx->opt.klt_mean_removal = on;
    return OFPS_HIP_OK;
}

int ofps_hip_get_klt_mean_removal(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.klt_mean_removal : OFPS_HIP_EINVAL; }

int ofps_hip_set_klt_fb(ofps_hip_ctx* ctx, int limit) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, limit >= 0 && limit <= kKltMaxFb, "set_klt_fb: limit %d outside [0, %d]", limit, kKltMaxFb);
    ctx->opt.klt_fb = limit;
    return OFPS_HIP_OK;
}

int ofps_hip_get_klt_fb(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.klt_fb : OFPS_HIP_EINVAL; }

int ofps_hip_set_klt_prediction(ofps_hip_ctx* ctx, int on) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, on == 0 || on == 1, "set_klt_prediction: %d is not 0|1", on);
    ctx->opt.klt_prediction = on;
    return OFPS_HIP_OK;
}

int ofps_hip_get_klt_prediction(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.klt_prediction : OFPS_HIP_EINVAL; }

int ofps_hip_set_klt_batch_prediction(ofps_hip_ctx* ctx, int on) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, on == 0 || on == 1, "set_klt_batch_prediction: %d is not 0|1", on);
    ctx->opt.klt_batch_prediction = on;
    return OFPS_HIP_OK;
}

int ofps_hip_get_klt_batch_prediction(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.klt_batch_prediction : OFPS_HIP_EINVAL; }

size_t ofps_hip_klt_slot_count(int W, int H, int cell) {
    if (W < 1 || H < 1 || (cell != 8 && cell != 16 && cell != 32)) return 0;
    return klt_slots(W, H, cell);
}

int ofps_hip_klt_features_dev(ofps_hip_ctx* ctx, const void* d_luma, int W, int H, int stride, void* d_out_triples) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_luma && d_out_triples, "klt_features: null device pointer");
    const int rc = klt_check_frame(ctx, W, H, stride, 1, "klt_features");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return klt_features_device(ctx, static_cast<const uint8_t*>(d_luma), W, H, stride, klt_settings(ctx), static_cast<int*>(d_out_triples));
}

int ofps_hip_klt_features(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride, int32_t* out_triples) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, luma && out_triples, "klt_features: null host pointer");
    int rc = klt_check_frame(ctx, W, H, stride, 1, "klt_features");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const KltSettings s = klt_settings(ctx);
    const size_t ns = klt_slots(W, H, s.cell);
    const int ss = ofps::padded_stride(W);
    auto* d_img = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, (size_t)ss * H));
    auto* d_out = static_cast<int*>(ofps::scratch(ctx, ofps::S_KLT_HOST, ns * 3 * sizeof(int)));
    if (!d_img || !d_out) return OFPS_HIP_ENOMEM;
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_img, ss, luma, stride, W, H, ctx->stream));
    rc = klt_features_device(ctx, d_img, W, H, ss, s, d_out);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_triples, d_out, ns * 3 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

// ofps_hip_klt_track_dev and, with at_q, ofps_hip_klt_track_q_dev (N3f's stage form: the points are positions in 1/256 pixel)
static int klt_track_dev_impl(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, const void* d_points, size_t n,
                              int levels, int radius, int iters, void* d_out_quads, bool at_q, const void* d_guesses = nullptr) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_prev && d_cur && (n == 0 || (d_points && d_out_quads)), "klt_track: null device pointer");
    OFPS_REQUIRE(ctx, n < (1ull << 28), "klt_track: too many points");
    int rc = klt_check_call(ctx, W, H, stride, levels, radius, iters, "klt_track");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n == 0) return OFPS_HIP_OK;
    KltTrackBatchParams b{};                                  // the two frames as a batch of one pair; the one-pair kernels take b.t
    rc = klt_pyramid_device(ctx, ofps::SadFrames{static_cast<const uint8_t*>(d_prev), static_cast<const uint8_t*>(d_cur), 0, 0, W, H, stride}, 1, levels, &b);
    if (rc != OFPS_HIP_OK) return rc;
    KltTrackParams& p = b.t;
    klt_track_settings(ctx, levels, radius, iters, &p);
    p.pts = static_cast<const int*>(d_points); p.pt_stride = 2; p.from_features = 0; p.n = (int)n;
    p.out_quad = static_cast<int*>(d_out_quads);
    if (d_guesses) return klt_track_launch(ctx, kKltTrackPred, p.n, KltTrackPredParams{p, static_cast<const int*>(d_guesses), nullptr, 0, 0});
    return klt_track_launch(ctx, at_q ? kKltTrackQ : kKltTrack, p.n, p);
}

static int klt_track_host_impl(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, const int32_t* points, size_t n,
                               int levels, int radius, int iters, int32_t* out_quads, bool at_q, const int32_t* guesses = nullptr) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, prev && cur && (n == 0 || (points && out_quads)), "klt_track: null host pointer");
    OFPS_REQUIRE(ctx, n < (1ull << 28), "klt_track: too many points");
    int rc = klt_check_call(ctx, W, H, stride, levels, radius, iters, "klt_track");
    if (rc != OFPS_HIP_OK) return rc;
    const int xmax = at_q ? 256 * (W - 1) : W - 1, ymax = at_q ? 256 * (H - 1) : H - 1;
    for (size_t k = 0; k < n; ++k)
        OFPS_REQUIRE(ctx, points[2 * k] >= 0 && points[2 * k] <= xmax && points[2 * k + 1] >= 0 && points[2 * k + 1] <= ymax,
                     "klt_track: point %zu = (%d, %d) lies outside the %d x %d frame", k, points[2 * k], points[2 * k + 1], W, H);
    for (size_t k = 0; guesses && k < n; ++k)
        OFPS_REQUIRE(ctx, guesses[2 * k] >= -kKltMaxGuess && guesses[2 * k] <= kKltMaxGuess && guesses[2 * k + 1] >= -kKltMaxGuess && guesses[2 * k + 1] <= kKltMaxGuess,
                     "klt_track_from: guess %zu = (%d, %d) lies beyond +-2^23", k, guesses[2 * k], guesses[2 * k + 1]);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n == 0) return OFPS_HIP_OK;
    const int ss = ofps::padded_stride(W);
    const size_t fb = (size_t)ss * H, o_quad = pad16(n * 2 * sizeof(int)), o_guess = o_quad + n * 4 * sizeof(int);
    auto* d_fr = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, 2 * fb));
    auto* d_io = static_cast<char*>(ofps::scratch(ctx, ofps::S_KLT_HOST, o_guess + (guesses ? n * 2 * sizeof(int) : 0)));
    if (!d_fr || !d_io) return OFPS_HIP_ENOMEM;
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_fr, ss, prev, stride, W, H, ctx->stream));
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_fr + fb, ss, cur, stride, W, H, ctx->stream));
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_io, points, n * 2 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (guesses) OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_io + o_guess, guesses, n * 2 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    rc = klt_track_dev_impl(ctx, d_fr, d_fr + fb, W, H, ss, d_io, n, levels, radius, iters, d_io + o_quad, at_q, guesses ? d_io + o_guess : nullptr);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_quads, d_io + o_quad, n * 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_klt_track_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, const void* d_points, size_t n,
                           int levels, int radius, int iters, void* d_out_quads) {
    return klt_track_dev_impl(ctx, d_prev, d_cur, W, H, stride, d_points, n, levels, radius, iters, d_out_quads, false);
}

int ofps_hip_klt_track(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, const int32_t* points, size_t n,
                       int levels, int radius, int iters, int32_t* out_quads) {
    return klt_track_host_impl(ctx, prev, cur, W, H, stride, points, n, levels, radius, iters, out_quads, false);
}

int ofps_hip_klt_track_from_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, const void* d_points,
                                const void* d_guesses, size_t n, int levels, int radius, int iters, void* d_out_quads) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, n == 0 || d_guesses, "klt_track_from: null device pointer");
    return klt_track_dev_impl(ctx, d_prev, d_cur, W, H, stride, d_points, n, levels, radius, iters, d_out_quads, false, d_guesses);
}

int ofps_hip_klt_track_from(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, const int32_t* points,
                            const int32_t* guesses, size_t n, int levels, int radius, int iters, int32_t* out_quads) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, n == 0 || guesses, "klt_track_from: null host pointer");
    return klt_track_host_impl(ctx, prev, cur, W, H, stride, points, n, levels, radius, iters, out_quads, false, guesses);
}

int ofps_hip_klt_predict_dev(ofps_hip_ctx* ctx, const void* d_prev_slots, int W, int H, int cell, void* d_out_guesses) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_prev_slots && d_out_guesses, "klt_predict: null device pointer");
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1 && W <= 32768 && H <= 32768 && (cell == 8 || cell == 16 || cell == 32), "klt_predict: bad lattice W=%d H=%d cell=%d", W, H, cell);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return klt_predict_device(ctx, static_cast<const int*>(d_prev_slots), W, H, cell, static_cast<int*>(d_out_guesses));
}

int ofps_hip_klt_predict(ofps_hip_ctx* ctx, const int32_t* prev_slots, int W, int H, int cell, int32_t* out_guesses) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, prev_slots && out_guesses, "klt_predict: null host pointer");
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1 && W <= 32768 && H <= 32768 && (cell == 8 || cell == 16 || cell == 32), "klt_predict: bad lattice W=%d H=%d cell=%d", W, H, cell);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ns = klt_slots(W, H, cell), o_out = pad16(ns * 6 * sizeof(int));
    auto* d_io = static_cast<char*>(ofps::scratch(ctx, ofps::S_KLT_HOST, o_out + ns * 2 * sizeof(int)));
    if (!d_io) return OFPS_HIP_ENOMEM;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_io, prev_slots, ns * 6 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    const int rc = klt_predict_device(ctx, reinterpret_cast<const int*>(d_io), W, H, cell, reinterpret_cast<int*>(d_io + o_out));
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_guesses, d_io + o_out, ns * 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_klt_track_q_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, const void* d_points, size_t n,
                             int levels, int radius, int iters, void* d_out_quads) {
    return klt_track_dev_impl(ctx, d_prev, d_cur, W, H, stride, d_points, n, levels, radius, iters, d_out_quads, true);
}

int ofps_hip_klt_track_q(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, const int32_t* points, size_t n,
                         int levels, int radius, int iters, int32_t* out_quads) {
    return klt_track_host_impl(ctx, prev, cur, W, H, stride, points, n, levels, radius, iters, out_quads, true);
}

int ofps_hip_klt_flow_from_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int levels, int radius, int iters,
                               const void* d_prev_slots, void* d_out_entries, void* d_out_count, void* d_out_slots) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_prev && d_cur && d_out_entries && d_out_count, "klt_flow: null device pointer");
    int rc = klt_check_call(ctx, W, H, stride, levels, radius, iters, "klt_flow");
    if (rc != OFPS_HIP_OK) return rc;
    const size_t slot_bytes = klt_slots(W, H, ctx->opt.klt_cell) * 6 * sizeof(int);
    rc = klt_check_apart(ctx, d_prev_slots, slot_bytes, d_out_slots, slot_bytes, "klt_flow_from");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::klt_flow_device(ctx, static_cast<const uint8_t*>(d_prev), static_cast<const uint8_t*>(d_cur), W, H, stride, levels, radius, iters,
                                 static_cast<float4*>(d_out_entries), static_cast<uint32_t*>(d_out_count), static_cast<int*>(d_out_slots),
                                 static_cast<const int*>(d_prev_slots));
}

int ofps_hip_klt_flow_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int levels, int radius, int iters,
                          void* d_out_entries, void* d_out_count, void* d_out_slots) {
    return ofps_hip_klt_flow_from_dev(ctx, d_prev, d_cur, W, H, stride, levels, radius, iters, nullptr, d_out_entries, d_out_count, d_out_slots);
}

// S_KLT_HOST of the host-pointer flow forms: [records, pairs x slots][counts, a u32 per item][raw slots, 6 i32 per slot of the batch]; with_prev:
// [the previous pair's raw slots, one item's].  d: null if the scratch slot could not be had
struct KltHostIo {
    size_t o_count, o_slots, o_prev;
    char* d;
    KltHostIo(ofps_hip_ctx* ctx, int pairs, size_t ns, bool with_prev)
        : o_count((size_t)pairs * ns * sizeof(float4)), o_slots(o_count + pad16((size_t)pairs * sizeof(uint32_t))),
          o_prev(o_slots + (size_t)pairs * ns * 6 * sizeof(int)),
          d(static_cast<char*>(ofps::scratch(ctx, ofps::S_KLT_HOST, o_prev + (with_prev ? ns * 6 * sizeof(int) : 0)))) {}
    float4* entries() const { return reinterpret_cast<float4*>(d); }
    uint32_t* counts() const { return reinterpret_cast<uint32_t*>(d + o_count); }
    int* slots() const { return reinterpret_cast<int*>(d + o_slots); }
    int* prev_slots() const { return reinterpret_cast<int*>(d + o_prev); }
};

// what a finished run hands back: the counts, the raw slots (optional), then each item's kept records alone -- what lies behind them in the item's
// slot is unspecified.  Waits for the stream
static int klt_host_read(ofps_hip_ctx* ctx, const KltHostIo& io, int pairs, size_t ns, const char* who, float* out_entries, uint32_t* out_counts,
                         int32_t* out_slots) {
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_counts, io.counts(), (size_t)pairs * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out_slots) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_slots, io.slots(), (size_t)pairs * ns * 6 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < pairs; ++k) {
        if (out_counts[k] > ns) return ofps::set_error(ctx, OFPS_HIP_EDEVICE, "%s: the device counted %u records in %zu slots", who, out_counts[k], ns);
        if (out_counts[k])
            OFPS_HIP_TRY(ctx, hipMemcpy(out_entries + (size_t)k * ns * 4, io.entries() + (size_t)k * ns, (size_t)out_counts[k] * sizeof(float4), hipMemcpyDeviceToHost));
    }
    return OFPS_HIP_OK;
}

int ofps_hip_klt_flow_from(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int levels, int radius, int iters,
                           const int32_t* prev_slots, float* out_entries, uint32_t* n_out, int32_t* out_slots) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, prev && cur && out_entries && n_out, "klt_flow: null host pointer");
    int rc = klt_check_call(ctx, W, H, stride, levels, radius, iters, "klt_flow");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t ns = klt_slots(W, H, ctx->opt.klt_cell);
    const int ss = ofps::padded_stride(W);
    const size_t fb = (size_t)ss * H;
    auto* d_fr = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, 2 * fb));
    const KltHostIo io(ctx, 1, ns, prev_slots != nullptr);
    if (!d_fr || !io.d) return OFPS_HIP_ENOMEM;
    if (prev_slots) OFPS_HIP_TRY(ctx, hipMemcpyAsync(io.prev_slots(), prev_slots, ns * 6 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_fr, ss, prev, stride, W, H, ctx->stream));
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_fr + fb, ss, cur, stride, W, H, ctx->stream));
    rc = ofps::klt_flow_device(ctx, d_fr, d_fr + fb, W, H, ss, levels, radius, iters, io.entries(), io.counts(), out_slots ? io.slots() : nullptr,
                               prev_slots ? io.prev_slots() : nullptr);
    uint32_t count = 0;                                       // n_out is written on success alone
    if (rc == OFPS_HIP_OK) rc = klt_host_read(ctx, io, 1, ns, "klt_flow", out_entries, &count, out_slots);
    if (rc == OFPS_HIP_OK) *n_out = count;
    return rc;
}

int ofps_hip_klt_flow(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int levels, int radius, int iters,
                      float* out_entries, uint32_t* n_out, int32_t* out_slots) {
    return ofps_hip_klt_flow_from(ctx, prev, cur, W, H, stride, levels, radius, iters, nullptr, out_entries, n_out, out_slots);
}

// ofps_hip_klt_flow_batch_dev and, with `chained`, ofps_hip_klt_flow_batch_from_dev (N3pb)
static int klt_flow_batch_dev_impl(ofps_hip_ctx* ctx, const void* d_frames, int n_frames, int W, int H, int stride, size_t frame_pitch, int ref_mode,
                                   int levels, int radius, int iters, void* d_out_entries, void* d_out_counts, void* d_out_slots, bool chained,
                                   const void* d_prev_slots) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_frames && d_out_entries && d_out_counts, "klt_flow_batch: null device pointer");
    int rc = klt_check_call(ctx, W, H, stride, levels, radius, iters, "klt_flow_batch");
    if (rc == OFPS_HIP_OK) rc = klt_check_sequence(ctx, n_frames, H, stride, frame_pitch, ref_mode, "klt_flow_batch");
    if (rc != OFPS_HIP_OK) return rc;
    const size_t slot_bytes = klt_slots(W, H, ctx->opt.klt_cell) * 6 * sizeof(int);
    rc = klt_check_apart(ctx, d_prev_slots, slot_bytes, d_out_slots, (size_t)(n_frames - 1) * slot_bytes, "klt_flow_batch_from");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const ofps::SadFrames f = ofps::SadFrames::sequence(static_cast<const uint8_t*>(d_frames), frame_pitch, ref_mode, W, H, stride);
    return ofps::klt_flow_device(ctx, ofps::KltFlowCall{f, n_frames - 1, levels, radius, iters, static_cast<float4*>(d_out_entries),
                                                        static_cast<uint32_t*>(d_out_counts), static_cast<int*>(d_out_slots), true, chained,
                                                        static_cast<const int*>(d_prev_slots), nullptr});
}

// N3pb's switch: the plain batch entry points chain iff the context has both prediction settings on
static bool klt_batch_chained(const ofps_hip_ctx* ctx) { return ctx->opt.klt_prediction && ctx->opt.klt_batch_prediction; }

int ofps_hip_klt_flow_batch_dev(ofps_hip_ctx* ctx, const void* d_frames, int n_frames, int W, int H, int stride, size_t frame_pitch, int ref_mode,
                                int levels, int radius, int iters, void* d_out_entries, void* d_out_counts, void* d_out_slots) {
    if (!ctx) return OFPS_HIP_EINVAL;
    return klt_flow_batch_dev_impl(ctx, d_frames, n_frames, W, H, stride, frame_pitch, ref_mode, levels, radius, iters, d_out_entries, d_out_counts,
                                   d_out_slots, klt_batch_chained(ctx), nullptr);
}

int ofps_hip_klt_flow_batch_from_dev(ofps_hip_ctx* ctx, const void* d_frames, int n_frames, int W, int H, int stride, size_t frame_pitch, int ref_mode,
                                     int levels, int radius, int iters, void* d_out_entries, void* d_out_counts, void* d_out_slots,
                                     const void* d_prev_slots) {
    return klt_flow_batch_dev_impl(ctx, d_frames, n_frames, W, H, stride, frame_pitch, ref_mode, levels, radius, iters, d_out_entries, d_out_counts,
                                   d_out_slots, true, d_prev_slots);
}

// ofps_hip_klt_flow_batch and, with `chained`, ofps_hip_klt_flow_batch_from (N3pb): prev_slots is copied to the device first, so it may be out_slots
static int klt_flow_batch_host_impl(ofps_hip_ctx* ctx, const uint8_t* frames, int n_frames, int W, int H, int stride, size_t frame_pitch, int ref_mode,
                                    int levels, int radius, int iters, float* out_entries, uint32_t* out_counts, int32_t* out_slots, bool chained,
                                    const int32_t* prev_slots) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, frames && out_entries && out_counts, "klt_flow_batch: null host pointer");
    int rc = klt_check_call(ctx, W, H, stride, levels, radius, iters, "klt_flow_batch");
    if (rc == OFPS_HIP_OK) rc = klt_check_sequence(ctx, n_frames, H, stride, frame_pitch, ref_mode, "klt_flow_batch");
    if (rc != OFPS_HIP_OK) return rc;
    const int pairs = n_frames - 1;
    const size_t ns = klt_slots(W, H, ctx->opt.klt_cell);
    OFPS_REQUIRE(ctx, (unsigned long long)pairs * ns < (1ull << 31), "klt_flow_batch: %d pairs of %zu slots (pairs * slots must stay below 2^31)", pairs, ns);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int ss = ofps::padded_stride(W);
    const size_t fb = (size_t)ss * H;
    auto* d_fr = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, (size_t)n_frames * fb));
    const KltHostIo io(ctx, pairs, ns, prev_slots != nullptr);
    if (!d_fr || !io.d) return OFPS_HIP_ENOMEM;
    if (prev_slots) OFPS_HIP_TRY(ctx, hipMemcpyAsync(io.prev_slots(), prev_slots, ns * 6 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    for (int k = 0; k < n_frames; ++k)
        OFPS_HIP_TRY(ctx, ofps::upload_rows(d_fr + (size_t)k * fb, ss, frames + (size_t)k * frame_pitch, stride, W, H, ctx->stream));
    rc = ofps::klt_flow_device(ctx, ofps::KltFlowCall{ofps::SadFrames::sequence(d_fr, fb, ref_mode, W, H, ss), pairs, levels, radius, iters, io.entries(),
                                                      io.counts(), out_slots ? io.slots() : nullptr, true, chained,
                                                      prev_slots ? io.prev_slots() : nullptr, nullptr});
    if (rc != OFPS_HIP_OK) return rc;
    return klt_host_read(ctx, io, pairs, ns, "klt_flow_batch", out_entries, out_counts, out_slots);
}

int ofps_hip_klt_flow_batch(ofps_hip_ctx* ctx, const uint8_t* frames, int n_frames, int W, int H, int stride, size_t frame_pitch, int ref_mode,
                            int levels, int radius, int iters, float* out_entries, uint32_t* out_counts, int32_t* out_slots) {
    if (!ctx) return OFPS_HIP_EINVAL;
    return klt_flow_batch_host_impl(ctx, frames, n_frames, W, H, stride, frame_pitch, ref_mode, levels, radius, iters, out_entries, out_counts, out_slots,
                                    klt_batch_chained(ctx), nullptr);
}

int ofps_hip_klt_flow_batch_from(ofps_hip_ctx* ctx, const uint8_t* frames, int n_frames, int W, int H, int stride, size_t frame_pitch, int ref_mode,
                                 int levels, int radius, int iters, float* out_entries, uint32_t* out_counts, int32_t* out_slots,
                                 const int32_t* prev_slots) {
    return klt_flow_batch_host_impl(ctx, frames, n_frames, W, H, stride, frame_pitch, ref_mode, levels, radius, iters, out_entries, out_counts, out_slots,
                                    true, prev_slots);
}

int ofps_hip_set_batch_decoder(ofps_hip_ctx* ctx, int decoder, int levels, int radius, int iters) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, decoder == OFPS_HIP_BATCH_DECODER_SAD || decoder == OFPS_HIP_BATCH_DECODER_KLT, "set_batch_decoder: decoder %d is not 0|1", decoder);
    if (decoder == OFPS_HIP_BATCH_DECODER_KLT) {
        OFPS_REQUIRE(ctx, levels >= 1 && levels <= kKltMaxLevels, "set_batch_decoder: levels %d outside [1, %d]", levels, kKltMaxLevels);
        OFPS_REQUIRE(ctx, radius >= 1 && radius <= kKltMaxRadius, "set_batch_decoder: radius %d outside [1, %d]", radius, kKltMaxRadius);
        OFPS_REQUIRE(ctx, iters >= 1 && iters <= kKltMaxIters, "set_batch_decoder: iters %d outside [1, %d]", iters, kKltMaxIters);
        ctx->opt.klt_levels = levels; ctx->opt.klt_radius = radius; ctx->opt.klt_iters = iters;
    }
    ctx->opt.batch_decoder = decoder;
    return OFPS_HIP_OK;
}

int ofps_hip_get_batch_decoder(ofps_hip_ctx* ctx, int32_t* decoder, int32_t* levels, int32_t* radius, int32_t* iters) {
    if (!ctx) return OFPS_HIP_EINVAL;
    if (decoder) *decoder = ctx->opt.batch_decoder;
    if (levels) *levels = ctx->opt.klt_levels;
    if (radius) *radius = ctx->opt.klt_radius;
    if (iters) *iters = ctx->opt.klt_iters;
    return OFPS_HIP_OK;
}

}  // extern "C"
