// klt_intra.hip -- hip_klt's intra test and scene-cut rule (include/ofps_hip.h N3i): a kept track whose residual costs no less than coding the
// window from itself yields no record, and a pair most of whose candidates say so yields none at all.  hip_sad's N1i (sad_intra.hip) restated
// for the sparse decoder: it drops what no other test of a finished track can -- a track that converged on content with no counterpart (a scene
// cut, uncovered background, an object that appears, motion beyond the pyramid's reach).
//
// Nothing here tracks: the residual is the one the track launch reports.  This file holds:
// klt_activity_kernel: A(k) = sum |p - m| over the n x n window of the RAW level-0 previous frame around slot k's feature, m the window's rounded
//   mean, pixel indices clamped into the frame (no address outside it is formed, at any stride).  SIXTEEN LANES PER SLOT, four slots per wave:
//   lane i < n of a slot's sixteen holds COLUMN i of the window, its n <= 15 bytes packed into four registers.  A 225-byte window fills 16
//   lanes x 16 bytes to 88 %, as well as 64 lanes x 4 bytes would, but a wave then answers four slots and the two sums cross four lanes' bits
//   and not six (they stay inside a row of sixteen lanes).  The loads are bytes: a window row starts at any address, is 3 .. 15 bytes long
//   and is clamped at the frame's edges per pixel, so no wider load is both aligned and inside the frame; with a column per lane the n loads
//   of a lane walk DOWN the window, so one load instruction reads n adjacent bytes of one image row per slot -- four short runs per wave.
//   (A row per lane, the first form, had every load instruction touch 4 n different image rows: 12.1 us at 8,160 slots and 92.5 us at
//   129,600, measured; docs/history/42_klt_intra.md.)
//   Every window pixel is read once; both passes -- the sum, then the deviation from m -- run from registers through the packed-byte SAD
//   instruction: the sum as SAD against 0, the deviation as SAD against m in four bytes; a byte that holds no pixel is 0 and adds m to the
//   deviation, which the lane takes off again.  With VERDICT the same body reads the slot's quad first (a slot that is no candidate loads no
//   pixel), decides 16 res >= q 256 A in 64 bits, clears the keep flag and writes status 6 where slots exist, and adds to the item's two
//   counters: ballots per wave, summed in LDS, one pair of integer atomics per workgroup of 64 slots (the result does not depend on the order).
//   The item comes from the grid (blockIdx.y).
// klt_cut_kernel: an item whose counters say "cut" loses its flags, its statuses 0 become 7.  Launched only when the cut rule is on.
// klt_intra_verdict_kernel: verdict on caller-held quads and activities, a lane per entry (the stage form ofps_hip_klt_intra).
#include "common.hpp"

namespace ofps {

namespace {

enum { KLT_KEPT = 0, KLT_RESIDUAL = 4, KLT_NO_RETURN = 5, KLT_INTRA = 6, KLT_CUT = 7 };

constexpr int kIntraGroupSlots = 64;                        // slots per workgroup: four passes of sixteen (256 threads, 16 lanes per slot)

struct KltIntraParams {
    KltIntraCall c;
    int item0;
    int pt_stride;                                          // ints between two points: 3 (feature triples) or 2 (the stage form)
    uint32_t* out_activity;                                 // the stage form: A per point; else null
    int* slots;                                             // raw slots, 6 ints each, or null
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the sum over the sixteen lanes that share this lane's bits 4 and 5; every lane gets it
__device__ __forceinline__ uint32_t sum16(uint32_t v) {
    for (int d = 1; d <= 8; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

__device__ __forceinline__ bool klt_candidate(int status) { return status == KLT_KEPT || status == KLT_RESIDUAL || status == KLT_NO_RETURN; }

// N3i's comparison: 64-bit signed, equality is intra
__device__ __forceinline__ bool klt_is_intra(int res, uint32_t A, uint32_t ratio) {
    return 16ll * (long long)res >= (long long)ratio * 256ll * (long long)A;
}

template <bool VERDICT>
__global__ __launch_bounds__(256) void klt_activity_kernel(const KltIntraParams p) {
    __shared__ uint32_t group[2];
    const KltIntraCall& c = p.c;
    const int lane = threadIdx.x & 15, sub = threadIdx.x >> 4;
    const size_t item = (size_t)p.item0 + blockIdx.y;
    const uint8_t* __restrict__ img = c.frames + item * c.frame_pitch;
    const int* __restrict__ pts = c.feat + item * c.feat_pitch;
    const size_t at = item * (size_t)c.ns;
    const int n = 2 * c.w + 1;
    const uint32_t N = (uint32_t)(n * n);
    if (VERDICT) {
        if (threadIdx.x < 2) group[threadIdx.x] = 0;
        __syncthreads();
    }
    uint32_t nc = 0, ni = 0;
#pragma unroll
    for (int pass = 0; pass < kIntraGroupSlots / 16; ++pass) {
        const long long k = (long long)blockIdx.x * kIntraGroupSlots + pass * 16 + sub;
        const bool live = k < c.ns;
        int x = -1, y = -1, res = 0, status = KLT_KEPT;
        if (live) {
            const int* pt = pts + (size_t)k * p.pt_stride;
            x = pt[0]; y = pt[1];
            if (VERDICT) { const int* q = c.quads + 4 * (at + (size_t)k); res = q[2]; status = q[3]; }
        }
        const bool cand = live && (!VERDICT || klt_candidate(status));
        // a point outside the frame (the stage form's _dev entry alone: a feature lies inside) has A = 0 and loads nothing
        const bool col = cand && x >= 0 && x < c.W && y >= 0 && y < c.H && lane < n;
        uint32_t r[4] = {0, 0, 0, 0};
        if (col) {
            const uint8_t* __restrict__ column = img + clampi(x - c.w + lane, 0, c.W - 1);
#pragma unroll
            for (int j = 0; j < 2 * kKltMaxRadius + 1; ++j)
                if (j < n) r[j >> 2] |= (uint32_t)column[(size_t)clampi(y - c.w + j, 0, c.H - 1) * c.stride] << (8 * (j & 3));
        }
        uint32_t S = 0, A = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) S = __builtin_amdgcn_sad_u8(r[j], 0, S);
        S = sum16(S);
        const uint32_t m = (S + (N >> 1)) / N;
        const uint32_t mrep = m * 0x01010101u;
#pragma unroll
        for (int j = 0; j < 4; ++j) A = __builtin_amdgcn_sad_u8(r[j], mrep, A);
        // the lane's 16 bytes hold n pixels (none in a lane without a column): every other byte is 0 and has added m
        A = sum16(A - (16u - (col ? (uint32_t)n : 0u)) * m);
        const bool first = lane == 0 && live;
        if (first && p.out_activity) p.out_activity[at + (size_t)k] = A;
        if (VERDICT) {
            const bool intra = cand && klt_is_intra(res, A, (uint32_t)c.ratio);
            if (first && intra && status == KLT_KEPT) {
                c.flags[at + (size_t)k] = 0;
                if (p.slots) p.slots[6 * (at + (size_t)k) + 5] = KLT_INTRA;
            }
            nc += (uint32_t)__popcll(__ballot(first && cand)); ni += (uint32_t)__popcll(__ballot(first && intra));
        }
    }
    if (VERDICT) {
        if ((threadIdx.x & 63) == 0) { atomicAdd(&group[0], nc); atomicAdd(&group[1], ni); }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (group[0]) atomicAdd(&c.counts[2 * item], group[0]);
            if (group[1]) atomicAdd(&c.counts[2 * item + 1], group[1]);
        }
    }
}

// item item0 + blockIdx.y is a cut iff 100 * n_intra >= cut * n_cand (no candidate: a cut): what is still kept -- its flag where there are flags,
// its status 0 otherwise -- loses the flag and becomes status 7.  st (optional): the entries' statuses, st_stride ints apart
__global__ __launch_bounds__(256) void klt_cut_kernel(const uint32_t* __restrict__ counts, int item0, uint32_t ns, uint32_t cut, uint8_t* flags, int* st,
                                                      int st_stride) {
    const size_t item = (size_t)item0 + blockIdx.y;
    const uint32_t* c = counts + 2 * item;
    if (100ull * c[1] < (unsigned long long)cut * c[0]) return;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= ns) return;
    const size_t idx = item * ns + k;
    const bool kept = flags ? flags[idx] != 0 : st[idx * (size_t)st_stride] == KLT_KEPT;
    if (!kept) return;
    if (flags) flags[idx] = 0;
    if (st) st[idx * (size_t)st_stride] = KLT_CUT;
}

// the stage form: entry k's quad (dqx, dqy, res, status) and activity -> its status after the intra test; counts: [candidates, intra], zero before
__global__ __launch_bounds__(256) void klt_intra_verdict_kernel(const int* __restrict__ quads, const uint32_t* __restrict__ activity, uint32_t n, uint32_t ratio,
                                                                int* __restrict__ out_status, uint32_t* __restrict__ counts) {
    __shared__ uint32_t group[2];
    if (threadIdx.x < 2) group[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    bool cand = false, intra = false;
    if (k < n) {
        const int res = quads[4 * (size_t)k + 2], status = quads[4 * (size_t)k + 3];
        cand = klt_candidate(status);
        intra = cand && klt_is_intra(res, activity[k], ratio);
        out_status[k] = status == KLT_KEPT && intra ? (int)KLT_INTRA : status;
    }
    const uint32_t nc = (uint32_t)__popcll(__ballot(cand)), ni = (uint32_t)__popcll(__ballot(intra));
    if ((threadIdx.x & 63) == 0) { atomicAdd(&group[0], nc); atomicAdd(&group[1], ni); }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (group[0]) atomicAdd(&counts[0], group[0]);
        if (group[1]) atomicAdd(&counts[1], group[1]);
    }
}

int klt_cut_launch(ofps_hip_ctx* ctx, const uint32_t* d_counts, int item0, int items, size_t ns, int cut, uint8_t* d_flags, int* d_st, int st_stride) {
    if (cut <= 0 || ns == 0 || items <= 0) return OFPS_HIP_OK;
    hipLaunchKernelGGL(klt_cut_kernel, dim3((unsigned)((ns + 255) / 256), (unsigned)items), dim3(256), 0, ctx->stream, d_counts, item0, (uint32_t)ns,
                       (uint32_t)cut, d_flags, d_st, st_stride);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

int klt_intra_check(ofps_hip_ctx* ctx, int ratio, int cut, const char* who) {
    OFPS_REQUIRE(ctx, ratio >= 1 && ratio <= kKltIntraMax, "%s: intra ratio %d outside [1, %d]", who, ratio, kKltIntraMax);
    OFPS_REQUIRE(ctx, cut >= 0 && cut <= kKltCutMax, "%s: scene cut %d outside [0, %d]", who, cut, kKltCutMax);
    return OFPS_HIP_OK;
}

int klt_activity_check(ofps_hip_ctx* ctx, int W, int H, int stride, size_t n, int radius, const char* who) {
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1 && W <= 32768 && H <= 32768 && stride >= W, "%s: bad geometry W=%d H=%d stride=%d", who, W, H, stride);
    OFPS_REQUIRE(ctx, radius >= 1 && radius <= kKltMaxRadius, "%s: radius %d outside [1, %d]", who, radius, kKltMaxRadius);
    OFPS_REQUIRE(ctx, n < (1ull << 28), "%s: too many points", who);
    return OFPS_HIP_OK;
}

// the stage form: n points (x, y) of one frame -> their activities
int klt_activity_device(ofps_hip_ctx* ctx, const uint8_t* d_luma, int W, int H, int stride, const int* d_points, size_t n, int radius, uint32_t* d_out) {
    if (n == 0) return OFPS_HIP_OK;
    KltIntraParams p{};
    p.c.frames = d_luma; p.c.W = W; p.c.H = H; p.c.stride = stride; p.c.w = radius; p.c.ns = (int)n; p.c.feat = d_points;
    p.pt_stride = 2; p.out_activity = d_out;
    hipLaunchKernelGGL(klt_activity_kernel<false>, dim3((unsigned)((n + kIntraGroupSlots - 1) / kIntraGroupSlots)), dim3(256), 0, ctx->stream, p);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// the stage form: verdict and cut on n quads and activities -> statuses, and the two counters in d_counts (never null here)
int klt_intra_stage_device(ofps_hip_ctx* ctx, const int* d_quads, const uint32_t* d_activity, size_t n, int ratio, int cut, int* d_out_status,
                           uint32_t* d_counts) {
    OFPS_HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, 2 * sizeof(uint32_t), ctx->stream));
    if (n) {
        hipLaunchKernelGGL(klt_intra_verdict_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_quads, d_activity, (uint32_t)n,
                           (uint32_t)ratio, d_out_status, d_counts);
        OFPS_HIP_TRY(ctx, hipGetLastError());
    }
    return klt_cut_launch(ctx, d_counts, 0, 1, n, cut, nullptr, d_out_status, 1);
}

}  // namespace

int klt_intra_device(ofps_hip_ctx* ctx, const KltIntraCall& c, int item0, int items, int* d_slots) {
    if (c.ns <= 0 || items <= 0) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, items <= 65535, "klt_intra: %d items in one launch (at most 65535)", items);
    KltIntraParams p{};
    p.c = c; p.item0 = item0; p.pt_stride = 3; p.out_activity = nullptr; p.slots = d_slots;
    hipLaunchKernelGGL(klt_activity_kernel<true>, dim3((unsigned)((c.ns + kIntraGroupSlots - 1) / kIntraGroupSlots), (unsigned)items), dim3(256), 0,
                       ctx->stream, p);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return klt_cut_launch(ctx, c.counts, item0, items, (size_t)c.ns, c.cut, c.flags, d_slots ? d_slots + 5 : nullptr, 6);
}

}  // namespace ofps

extern "C" {

int ofps_hip_set_klt_intra(ofps_hip_ctx* ctx, int ratio) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, ratio >= 0 && ratio <= ofps::kKltIntraMax, "set_klt_intra: %d outside [0, %d]", ratio, ofps::kKltIntraMax);
    ctx->opt.klt_intra = ratio;
    return OFPS_HIP_OK;
}

int ofps_hip_get_klt_intra(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.klt_intra : OFPS_HIP_EINVAL; }

int ofps_hip_set_klt_cut(ofps_hip_ctx* ctx, int percent) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, percent >= 0 && percent <= ofps::kKltCutMax, "set_klt_cut: %d outside [0, %d]", percent, ofps::kKltCutMax);
    ctx->opt.klt_cut = percent;
    return OFPS_HIP_OK;
}

int ofps_hip_get_klt_cut(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.klt_cut : OFPS_HIP_EINVAL; }

int ofps_hip_klt_activity_dev(ofps_hip_ctx* ctx, const void* d_luma, int W, int H, int stride, const void* d_points, size_t n, int radius,
                              void* d_out_activity) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_luma && (n == 0 || (d_points && d_out_activity)), "klt_activity: null device pointer");
    const int rc = ofps::klt_activity_check(ctx, W, H, stride, n, radius, "klt_activity");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::klt_activity_device(ctx, static_cast<const uint8_t*>(d_luma), W, H, stride, static_cast<const int*>(d_points), n, radius,
                                     static_cast<uint32_t*>(d_out_activity));
}

int ofps_hip_klt_activity(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride, const int32_t* points, size_t n, int radius,
                          uint32_t* out_activity) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, luma && (n == 0 || (points && out_activity)), "klt_activity: null host pointer");
    int rc = ofps::klt_activity_check(ctx, W, H, stride, n, radius, "klt_activity");
    if (rc != OFPS_HIP_OK) return rc;
    for (size_t k = 0; k < n; ++k)
        OFPS_REQUIRE(ctx, points[2 * k] >= 0 && points[2 * k] < W && points[2 * k + 1] >= 0 && points[2 * k + 1] < H,
                     "klt_activity: point %zu = (%d, %d) lies outside the %d x %d frame", k, points[2 * k], points[2 * k + 1], W, H);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n == 0) return OFPS_HIP_OK;
    const int ss = ofps::padded_stride(W);
    const size_t o_out = (n * 2 * sizeof(int) + 15) & ~size_t(15);
    auto* d_img = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, (size_t)ss * H));
    auto* d_io = static_cast<char*>(ofps::scratch(ctx, ofps::S_KLT_HOST, o_out + n * sizeof(uint32_t)));
    if (!d_img || !d_io) return OFPS_HIP_ENOMEM;
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_img, ss, luma, stride, W, H, ctx->stream));
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_io, points, n * 2 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    rc = ofps::klt_activity_device(ctx, d_img, W, H, ss, reinterpret_cast<const int*>(d_io), n, radius, reinterpret_cast<uint32_t*>(d_io + o_out));
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_activity, d_io + o_out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_klt_intra_dev(ofps_hip_ctx* ctx, const void* d_quads, const void* d_activity, size_t n, int ratio, int cut, void* d_out_status,
                           void* d_out_counts) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, n == 0 || (d_quads && d_activity && d_out_status), "klt_intra: null device pointer");
    OFPS_REQUIRE(ctx, n < (1ull << 28), "klt_intra: too many entries");
    const int rc = ofps::klt_intra_check(ctx, ratio, cut, "klt_intra");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto* d_counts = static_cast<uint32_t*>(d_out_counts);
    if (!d_counts) {                                          // the cut rule reads the counters whether the caller wants them or not
        d_counts = static_cast<uint32_t*>(ofps::scratch(ctx, ofps::S_RESULT, 2 * sizeof(uint32_t)));
        if (!d_counts) return OFPS_HIP_ENOMEM;
    }
    return ofps::klt_intra_stage_device(ctx, static_cast<const int*>(d_quads), static_cast<const uint32_t*>(d_activity), n, ratio, cut,
                                        static_cast<int*>(d_out_status), d_counts);
}

int ofps_hip_klt_intra(ofps_hip_ctx* ctx, const int32_t* quads, const uint32_t* activity, size_t n, int ratio, int cut, int32_t* out_status,
                       uint32_t* out_counts) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, n == 0 || (quads && activity && out_status), "klt_intra: null host pointer");
    OFPS_REQUIRE(ctx, n < (1ull << 28), "klt_intra: too many entries");
    int rc = ofps::klt_intra_check(ctx, ratio, cut, "klt_intra");
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // [quads][activities][statuses][counters]
    const size_t o_act = n * 4 * sizeof(int), o_st = o_act + n * sizeof(uint32_t), o_cnt = (o_st + n * sizeof(int) + 15) & ~size_t(15);
    auto* d_io = static_cast<char*>(ofps::scratch(ctx, ofps::S_KLT_HOST, o_cnt + 2 * sizeof(uint32_t)));
    if (!d_io) return OFPS_HIP_ENOMEM;
    if (n) {
        OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_io, quads, n * 4 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_io + o_act, activity, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    rc = ofps::klt_intra_stage_device(ctx, reinterpret_cast<const int*>(d_io), reinterpret_cast<const uint32_t*>(d_io + o_act), n, ratio, cut,
                                      reinterpret_cast<int*>(d_io + o_st), reinterpret_cast<uint32_t*>(d_io + o_cnt));
    if (rc != OFPS_HIP_OK) return rc;
    if (n) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_status, d_io + o_st, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (out_counts) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_counts, d_io + o_cnt, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

}  // extern "C"
