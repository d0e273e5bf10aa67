// detect.hip -- A5: BlockMotionDetection::detect_motion on gfx950
// (block-motion-detector/src/lib.rs:49-118; trait ofps/src/detection.rs:11).
//
// densify (densify.hip, exact input-order sums) -> one workgroup per item:
//   * map[cell] = |m| >= target_motion                                  (lib.rs:63-68)
//   * 8-connected components by min-label propagation with pointer jumping in LDS; the label of
//     a component is its smallest cell index = the raster-scan seed of the reference's flood
//     fill (lib.rs:74-76)
//   * area per label with LDS integer atomics; winner = max (area, earliest seed): the
//     reference keeps the first island under a strict `>` (lib.rs:106-109)
//   * output = winner's cells except its seed cell, which the reference never copies
//     (lib.rs:79-102); Some iff area / dim^2 >= min_size                (lib.rs:114-118)
// Everything integer is order-independent, so area and membership are bit-exact by construction.
#include "common.hpp"

#include <cstdlib>

namespace ofps {

// dynamic LDS: area[cells] (u32) then label[cells] (u16; every cell is owned by one thread, so
// labels need no atomics).  160x160 cells -> 150 KiB, inside the 160 KiB of one CU.
__global__ __launch_bounds__(1024) void detect_kernel(const float2* __restrict__ field, int dim, float target_motion,
                                                      float min_size, int* __restrict__ out_result,
                                                      float2* __restrict__ out_field) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    __shared__ unsigned long long best_key;
    const int cells = dim * dim;
    uint32_t* area = lds;
    uint16_t* label = reinterpret_cast<uint16_t*>(lds + cells);
    const size_t item = blockIdx.x;
    const float2* f = field + item * cells;
    const uint32_t NONE = 0xFFFFu;

    for (int i = threadIdx.x; i < cells; i += 1024) {
        const float2 m = f[i];
        const float mag = sqrtf(m.x * m.x + m.y * m.y);                 // Vector2::magnitude
        label[i] = (uint16_t)((mag >= target_motion) ? (uint32_t)i : NONE);
        area[i] = 0;
    }
    if (threadIdx.x == 0) best_key = 0;
    __syncthreads();

    for (;;) {
        int changed = 0;
        for (int i = threadIdx.x; i < cells; i += 1024) {
            uint32_t l = label[i];
            if (l == NONE) continue;
            const int x = i % dim, y = i / dim;
            uint32_t m = l;
#pragma unroll
            for (int oy = -1; oy <= 1; ++oy)
#pragma unroll
                for (int ox = -1; ox <= 1; ++ox) {
                    const int nx = x + ox, ny = y + oy;
                    if (nx < 0 || nx >= dim || ny < 0 || ny >= dim) continue;
                    const uint32_t nl = label[ny * dim + nx];
                    if (nl != NONE) m = min(m, nl);
                }
            const uint32_t root = label[m];                              // pointer jump (root <= m)
            if (root != NONE) m = min(m, root);
            if (m < l) { label[i] = (uint16_t)m; changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
    }

    for (int i = threadIdx.x; i < cells; i += 1024) {
        const uint32_t l = label[i];
        if (l != NONE) atomicAdd(&area[l], 1u);
    }
    __syncthreads();
    // winner: max area, ties -> smallest seed index
    unsigned long long k = 0;
    for (int i = threadIdx.x; i < cells; i += 1024) {
        const uint32_t a = area[i];
        if (a) {
            const unsigned long long key = ((unsigned long long)a << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i);
            k = key > k ? key : k;
        }
    }
    if (k) atomicMax(&best_key, k);
    __syncthreads();
    const unsigned long long bk = best_key;
    const uint32_t barea = (uint32_t)(bk >> 32);
    const uint32_t seed = 0xFFFFFFFFu - (uint32_t)(bk & 0xFFFFFFFFu);
    const bool some = bk != 0 && ((float)barea / (float)cells >= min_size);
    float2* o = out_field + item * cells;
    for (int i = threadIdx.x; i < cells; i += 1024) {
        const bool in = some && label[i] == seed && (uint32_t)i != seed;
        o[i] = in ? f[i] : make_float2(0.0f, 0.0f);
    }
    if (threadIdx.x == 0) {
        out_result[4 * item + 0] = some ? 1 : 0;
        out_result[4 * item + 1] = some ? (int)barea : 0;
        out_result[4 * item + 2] = dim;
        out_result[4 * item + 3] = 0;
    }
}

// ---- A5i: every qualifying island, not the largest alone (include/ofps_hip.h).  One workgroup per item, like detect_kernel, and the same
// labelling: min-label propagation with pointer jumping, areas by LDS integer atomics.  Then
//   * every root with an area is a component; the qualifying ones' keys (area << 32 | ~seed, detect_kernel's winner key) go to scratch in
//     any order -- the key order is total, so the sort below does not care -- and the area array is dead
//   * the keys come back into the area array's LDS and are sorted descending by a bitonic network: rank r = the r-th key.  At most
//     ceil(dim / 2)^2 components exist (two lit cells of one 2 x 2 block touch), 6,400 at dim 160: 8,192 keys, 64 KiB
//   * the listed ranks' seeds and areas go to the table, rank[seed] to scratch, and the keys are dead
//   * one pass over the cells: label -> rank -> labels and field out, box and sums into per-rank accumulators by integer atomicMin /
//     atomicMax / atomicAdd -- the first `acc_rows` ranks in the LDS the keys held, the rest straight in the table (an island behind rank r
//     has at most cells / (r + 1) cells).  A wave whose listed cells are all of one island -- every wave inside a large island -- reduces
//     in registers first and issues six atomics, not 384.
// LDS: label[cells] (u16) then max(area[cells] u32, keys[P] u64, accumulators): 150 KiB at dim 160, what detect_kernel takes.  No float is
// summed and every integer result is independent of the order of the atomics: bit-exact by construction.
__device__ inline int wave_min(int v) { for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ inline int wave_max(int v) { for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }
__device__ inline int wave_sum(int v) { for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o); return v; }

struct IslandsOut {                      // item j's outputs lie j * stride elements behind the base; labels / field may be null
    int* counts; size_t counts_stride;
    int* table; size_t table_stride;
    uint16_t* labels; size_t labels_stride;
    float2* field;                       // cells per item
};

__global__ __launch_bounds__(1024) void islands_kernel(const float2* __restrict__ field, int dim, float target_motion, float min_size, int K,
                                                       int P, int acc_rows, char* __restrict__ work, size_t work_stride, IslandsOut o) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    __shared__ int n_comp, n_qual;
    const int cells = dim * dim;
    const int tid = threadIdx.x;
    uint16_t* label = reinterpret_cast<uint16_t*>(lds);
    uint32_t* region = lds + ((cells * 2 + 15) / 16) * 4;
    uint32_t* area = region;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(region);
    int* acc = reinterpret_cast<int*>(region);
    const size_t item = blockIdx.x;
    const float2* f = field + item * cells;
    unsigned long long* gkeys = reinterpret_cast<unsigned long long*>(work + item * work_stride);
    uint16_t* grank = reinterpret_cast<uint16_t*>(work + item * work_stride + (size_t)P * sizeof(unsigned long long));
    int* counts = o.counts + item * o.counts_stride;
    int* table = o.table + item * o.table_stride;
    const uint32_t NONE = 0xFFFFu;

    for (int i = tid; i < cells; i += 1024) {
        const float2 m = f[i];
        const float mag = sqrtf(m.x * m.x + m.y * m.y);
        label[i] = (uint16_t)((mag >= target_motion) ? (uint32_t)i : NONE);
        area[i] = 0;
    }
    if (tid == 0) { n_comp = 0; n_qual = 0; }
    __syncthreads();

    for (;;) {
        int changed = 0;
        for (int i = tid; i < cells; i += 1024) {
            uint32_t l = label[i];
            if (l == NONE) continue;
            const int x = i % dim, y = i / dim;
            uint32_t m = l;
#pragma unroll
            for (int oy = -1; oy <= 1; ++oy)
#pragma unroll
                for (int ox = -1; ox <= 1; ++ox) {
                    const int nx = x + ox, ny = y + oy;
                    if (nx < 0 || nx >= dim || ny < 0 || ny >= dim) continue;
                    const uint32_t nl = label[ny * dim + nx];
                    if (nl != NONE) m = min(m, nl);
                }
            const uint32_t root = label[m];
            if (root != NONE) m = min(m, root);
            if (m < l) { label[i] = (uint16_t)m; changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
    }

    for (int i = tid; i < cells; i += 1024) {
        const uint32_t l = label[i];
        if (l != NONE) atomicAdd(&area[l], 1u);
    }
    __syncthreads();
    // components and qualifying roots; every root's rank starts as "not listed"
    for (int i = tid; i < cells; i += 1024) {
        const uint32_t a = area[i];
        if (!a) continue;
        atomicAdd(&n_comp, 1);
        grank[i] = (uint16_t)NONE;
        if ((float)a / (float)cells >= min_size) {
            const int q = atomicAdd(&n_qual, 1);
            if (q < P) gkeys[q] = ((unsigned long long)a << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i);
        }
    }
    __syncthreads();                                                     // (the area array is dead from here)
    const int nq = min(n_qual, P);
    int Pn = 2;
    while (Pn < nq) Pn <<= 1;
    for (int t = tid; t < Pn; t += 1024) keys[t] = t < nq ? gkeys[t] : 0ull;
    __syncthreads();
    for (int k = 2; k <= Pn; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (Pn >> 1); t += 1024) {
                const int lo = ((t / j) * 2 * j) + (t % j), hi = lo + j;
                const unsigned long long a = keys[lo], b = keys[hi];
                const bool desc = (lo & k) == 0;
                if (desc ? a < b : a > b) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
    const int n_listed = min(nq, K);
    const int n_acc = min(n_listed, acc_rows);
    for (int r = tid; r < n_listed; r += 1024) {
        const unsigned long long key = keys[r];
        const uint32_t seed = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu);
        int* row = table + (size_t)r * 8;
        row[0] = (int)seed;
        row[1] = (int)(key >> 32);
        if (r >= n_acc) { row[2] = 0x7FFFFFFF; row[3] = 0x7FFFFFFF; row[4] = -1; row[5] = -1; row[6] = 0; row[7] = 0; }
        grank[seed] = (uint16_t)r;
    }
    __threadfence();
    __syncthreads();                                                     // (the keys are dead from here)
    for (int t = tid; t < n_acc * 6; t += 1024) {
        const int c = t % 6;
        acc[t] = c < 2 ? 0x7FFFFFFF : (c < 4 ? -1 : 0);
    }
    __syncthreads();

    uint16_t* ol = o.labels ? o.labels + item * o.labels_stride : nullptr;
    float2* of = o.field ? o.field + item * cells : nullptr;
    for (int base = 0; base < cells; base += 1024) {                     // every wave whole: the reductions below read all 64 lanes
        const int i = base + tid;
        uint32_t l = NONE, r = NONE;
        if (i < cells) {
            l = label[i];
            if (l != NONE) r = grank[l];
            if (ol) ol[i] = (uint16_t)r;
            if (of) of[i] = (r != NONE && (uint32_t)i != l) ? f[i] : make_float2(0.0f, 0.0f);
        }
        const bool listed = r != NONE;
        const unsigned long long mask = __ballot(listed);
        if (!mask) continue;
        const int x = listed ? i % dim : 0, y = listed ? i / dim : 0;
        const uint32_t r0 = (uint32_t)__shfl((int)r, __ffsll((long long)mask) - 1);
        if (__all(!listed || r == r0)) {
            const int x0 = wave_min(listed ? x : 0x7FFFFFFF), y0 = wave_min(listed ? y : 0x7FFFFFFF);
            const int x1 = wave_max(listed ? x : -1), y1 = wave_max(listed ? y : -1);
            const int sx = wave_sum(x), sy = wave_sum(y);
            if ((tid & 63) == 0) {
                int* row = (int)r0 < n_acc ? acc + r0 * 6 : table + (size_t)r0 * 8 + 2;
                atomicMin(row + 0, x0); atomicMin(row + 1, y0); atomicMax(row + 2, x1); atomicMax(row + 3, y1);
                atomicAdd(row + 4, sx); atomicAdd(row + 5, sy);
            }
        } else if (listed) {
            int* row = (int)r < n_acc ? acc + r * 6 : table + (size_t)r * 8 + 2;
            atomicMin(row + 0, x); atomicMin(row + 1, y); atomicMax(row + 2, x); atomicMax(row + 3, y);
            atomicAdd(row + 4, x); atomicAdd(row + 5, y);
        }
    }
    __syncthreads();
    for (int t = tid; t < n_acc * 6; t += 1024) table[(size_t)(t / 6) * 8 + 2 + t % 6] = acc[t];
    if (tid == 0) {
        counts[0] = n_qual;
        counts[1] = n_comp;
        counts[2] = dim;
        counts[3] = n_listed;
    }
}

static int block_dim_host(float min_size, size_t subdivide) {          // lib.rs:53-54, f32 throughout
    const float block_width = sqrtf(min_size) / (float)subdivide;
    const float d = ceilf(1.0f / block_width);
    if (!(d > 0.0f)) return 0;
    if (d > 1.0e9f) return 1000000000;
    return (int)d;
}

// d_n (optional): the entry counts on the device, one per item -- n is the capacity and the stride of every item (densify.hip)
int detect_device(ofps_hip_ctx* ctx, const float4* d_entries, size_t n, int batch, float min_size, size_t subdivide,
                  float target_motion, int* d_result, float2* d_out_field, int* out_dim, const uint32_t* d_n) {
    const int dim = block_dim_host(min_size, subdivide);
    if (out_dim) *out_dim = dim;
    OFPS_REQUIRE(ctx, dim >= 1 && dim <= 160, "detect: block_dim %d outside [1,160] (min_size=%g subdivide=%zu)", dim,
                 (double)min_size, subdivide);
    const size_t cells = (size_t)dim * dim;
    auto* d_field = static_cast<float2*>(scratch(ctx, S_FIELD, cells * batch * sizeof(float2)));
    if (!d_field) return OFPS_HIP_ENOMEM;
    int rc = densify_device(ctx, d_entries, n, batch, dim, dim, d_field, nullptr, nullptr, nullptr, d_n);
    if (rc != OFPS_HIP_OK) return rc;
    const size_t lds = cells * sizeof(uint32_t) + ((cells * sizeof(uint16_t) + 15) & ~size_t(15));
    if (lds > 48 * 1024)
        OFPS_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(detect_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(detect_kernel, dim3(batch), dim3(1024), lds, ctx->stream, d_field, dim, target_motion, min_size,
                       d_result, d_out_field);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// A5i: the islands of `batch` densified fields of dim x dim cells, on ctx->stream
static int islands_field_device(ofps_hip_ctx* ctx, const float2* d_field, int dim, int batch, float min_size, float target_motion, int K,
                                const IslandsOut& o) {
    const size_t cells = (size_t)dim * dim;
    const size_t max_roots = (size_t)((dim + 1) / 2) * ((dim + 1) / 2);
    size_t P = 2;
    while (P < max_roots) P <<= 1;
    const size_t lab_bytes = (cells * sizeof(uint16_t) + 15) & ~size_t(15);
    size_t region = cells * sizeof(uint32_t);
    if (region < P * sizeof(unsigned long long)) region = P * sizeof(unsigned long long);
    size_t acc_rows = region / (6 * sizeof(int));
    if (acc_rows > (size_t)K) acc_rows = (size_t)K;
    const size_t lds = lab_bytes + ((region + 15) & ~size_t(15));
    const size_t work_stride = P * sizeof(unsigned long long) + lab_bytes;
    auto* d_work = static_cast<char*>(scratch(ctx, S_ISL_WORK, work_stride * batch));
    if (!d_work) return OFPS_HIP_ENOMEM;
    if (lds > 48 * 1024)
        OFPS_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(islands_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(islands_kernel, dim3(batch), dim3(1024), lds, ctx->stream, d_field, dim, target_motion, min_size, K, (int)P, (int)acc_rows,
                       d_work, work_stride, o);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// densify as the detector does -> islands
static int detect_islands_device(ofps_hip_ctx* ctx, const float4* d_entries, size_t n, int batch, float min_size, size_t subdivide,
                                 float target_motion, int K, const IslandsOut& o) {
    const int dim = block_dim_host(min_size, subdivide);
    OFPS_REQUIRE(ctx, dim >= 1 && dim <= kMaxDetectDim, "detect_islands: block_dim %d outside [1,160] (min_size=%g subdivide=%zu)", dim, (double)min_size,
                 subdivide);
    OFPS_REQUIRE(ctx, K >= 1 && K <= kMaxIslands, "detect_islands: max_islands %d outside [1, %d]", K, kMaxIslands);
    const size_t cells = (size_t)dim * dim;
    auto* d_field = static_cast<float2*>(scratch(ctx, S_FIELD, cells * batch * sizeof(float2)));
    if (!d_field) return OFPS_HIP_ENOMEM;
    const int rc = densify_device(ctx, d_entries, n, batch, dim, dim, d_field, nullptr, nullptr, nullptr, nullptr);
    if (rc != OFPS_HIP_OK) return rc;
    return islands_field_device(ctx, d_field, dim, batch, min_size, target_motion, K, o);
}

// `items` blocks `bytes` apart, each led by [counts][table][labels]; bytes 0: islands_block_bytes(K, dim), nothing behind them
static IslandsOut islands_blocks(char* base, int K, int dim, size_t bytes = 0) {
    if (!bytes) bytes = islands_block_bytes(K, dim);
    return {reinterpret_cast<int*>(base), bytes / 4, reinterpret_cast<int*>(base + 16), bytes / 4,
            reinterpret_cast<uint16_t*>(base + 16 + (size_t)K * 32), bytes / 2, nullptr};
}

int detect_islands_blocks_device(ofps_hip_ctx* ctx, const float4* d_entries, size_t n, int batch, float min_size, size_t subdivide, float target_motion,
                                 int K, char* d_blocks, size_t stride) {
    const int dim = block_dim_host(min_size, subdivide);
    OFPS_REQUIRE(ctx, dim >= 1 && dim <= kMaxDetectDim, "detect_islands: block_dim %d outside [1,160]", dim);
    return detect_islands_device(ctx, d_entries, n, batch, min_size, subdivide, target_motion, K, islands_blocks(d_blocks, K, dim, stride));
}

void islands_ticket_arm(ofps_hip_ctx* ctx, IslandsTicket* isl, const ofps_hip_frame_params* prm, int items, int form, bool restart) {
    const int dim = prm->run_detector ? block_dim_host(prm->min_size, prm->subdivide) : 0;
    isl->K = dim >= 1 && dim <= kMaxDetectDim ? ctx->opt.detect_islands : 0;
    isl->items = items; isl->first = items; isl->dim = dim;
    tracks_ticket_arm(ctx, isl, form, restart);                          // A5t
}

int islands_ticket_device(ofps_hip_ctx* ctx, int batch, int dim, float min_size, float target_motion, IslandsTicket* isl) {
    const size_t bytes = ticket_block_bytes(isl->K, dim, isl->T);
    int rc = host_block_reserve(ctx, &isl->pinned, &isl->cap, bytes * isl->items);
    if (rc != OFPS_HIP_OK) return rc;
    auto* d_blocks = static_cast<char*>(scratch(ctx, S_ISL_OUT, bytes * batch));
    if (!d_blocks) return OFPS_HIP_ENOMEM;
    // detect_device has just densified these records into S_FIELD, on this stream
    rc = islands_field_device(ctx, static_cast<const float2*>(ctx->scratch[S_FIELD].p), dim, batch, min_size, target_motion, isl->K,
                              islands_blocks(d_blocks, isl->K, dim, bytes));
    // A5t: a ticket armed with max_tracks > 0 steps its form's tracker through these items, behind the islands kernel on this stream
    if (rc == OFPS_HIP_OK && isl->T > 0) rc = tracks_ticket_device(ctx, isl, batch, dim, d_blocks, bytes);
    if (rc != OFPS_HIP_OK) return rc;
    isl->first = isl->items - batch; isl->dim = dim;
    return read_back_device(ctx, static_cast<char*>(isl->pinned) + bytes * isl->first, d_blocks, bytes * batch, ctx->stream);
}

int islands_collect(ofps_hip_ctx* ctx, const IslandsTicket& isl) {
    auto& last = ctx->isl_last;
    last.K = 0;
    if (isl.K <= 0) return OFPS_HIP_OK;
    const size_t bytes = ticket_block_bytes(isl.K, isl.dim, isl.T), total = bytes * isl.items;
    if (last.cap < total) {
        free(last.data);
        last.cap = 0;
        last.data = static_cast<char*>(malloc(total));
        if (!last.data) return set_error(ctx, OFPS_HIP_ENOMEM, "frame islands: out of host memory (%zu bytes)", total);
        last.cap = total;
    }
    for (int j = 0; j < isl.items; ++j) {
        char* dst = last.data + bytes * j;
        if (j >= isl.first) { memcpy(dst, static_cast<const char*>(isl.pinned) + bytes * j, bytes); continue; }
        memset(dst, 0, bytes);                                          // no vectors, no islands
        reinterpret_cast<int*>(dst)[2] = isl.dim;
        memset(dst + 16 + (size_t)isl.K * 32, 0xFF, (size_t)isl.dim * isl.dim * sizeof(uint16_t));
    }
    last.K = isl.K; last.items = isl.items; last.dim = isl.dim; last.T = isl.T;
    return OFPS_HIP_OK;
}

}  // namespace ofps

extern "C" {

int ofps_hip_block_dim(float min_size, size_t subdivide) { return ofps::block_dim_host(min_size, subdivide); }

int ofps_hip_detect_dev(ofps_hip_ctx* ctx, const void* d_entries, size_t n_per_item, int batch, float min_size,
                        size_t subdivide, float target_motion, void* d_out_result, void* d_out_field) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_out_result && d_out_field && (d_entries || n_per_item == 0), "detect: null device pointer");
    OFPS_REQUIRE(ctx, batch >= 1, "detect: batch must be >= 1");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::detect_device(ctx, static_cast<const float4*>(d_entries), n_per_item, batch, min_size, subdivide,
                               target_motion, static_cast<int*>(d_out_result), static_cast<float2*>(d_out_field), nullptr);
}

int ofps_hip_detect(ofps_hip_ctx* ctx, const float* entries, size_t n, float min_size, size_t subdivide,
                    float target_motion, int* has_motion, size_t* area, int* dim, float* out_field) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, has_motion && area && dim && out_field && (entries || n == 0), "detect: null host pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int d = ofps::block_dim_host(min_size, subdivide);
    OFPS_REQUIRE(ctx, d >= 1 && d <= 160, "detect: block_dim %d outside [1,160]", d);
    const size_t cells = (size_t)d * d;
    auto* d_ent = static_cast<float4*>(ofps::scratch(ctx, ofps::S_ENTRIES, n * sizeof(float4)));
    auto* d_res = static_cast<int*>(ofps::scratch(ctx, ofps::S_RESULT, 4 * sizeof(int)));
    auto* d_out = static_cast<float2*>(ofps::scratch(ctx, ofps::S_BEST, cells * sizeof(float2)));
    if (!d_ent || !d_res || !d_out) return OFPS_HIP_ENOMEM;
    if (n) OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_ent, entries, n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    int rc = ofps::detect_device(ctx, d_ent, n, 1, min_size, subdivide, target_motion, d_res, d_out, nullptr);
    if (rc != OFPS_HIP_OK) return rc;
    int res[4] = {0, 0, 0, 0};
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(res, d_res, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_field, d_out, cells * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *has_motion = res[0];
    *area = (size_t)res[1];
    *dim = res[2];
    return OFPS_HIP_OK;
}

int ofps_hip_detect_islands_dev(ofps_hip_ctx* ctx, const void* d_entries, size_t n_per_item, int batch, float min_size, size_t subdivide,
                                float target_motion, int max_islands, void* d_out_counts, void* d_out_table, void* d_out_labels,
                                void* d_out_field) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_out_counts && d_out_table && (d_entries || n_per_item == 0), "detect_islands: null device pointer");
    OFPS_REQUIRE(ctx, batch >= 1, "detect_islands: batch must be >= 1");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int d = ofps::block_dim_host(min_size, subdivide);
    const size_t cells = d >= 1 && d <= ofps::kMaxDetectDim ? (size_t)d * d : 0;     // (a bad grid is refused below)
    const ofps::IslandsOut o{static_cast<int*>(d_out_counts), 4, static_cast<int*>(d_out_table), (size_t)(max_islands > 0 ? max_islands : 0) * 8,
                             static_cast<uint16_t*>(d_out_labels), cells, static_cast<float2*>(d_out_field)};
    return ofps::detect_islands_device(ctx, static_cast<const float4*>(d_entries), n_per_item, batch, min_size, subdivide, target_motion,
                                       max_islands, o);
}

int ofps_hip_detect_islands(ofps_hip_ctx* ctx, const float* entries, size_t n, float min_size, size_t subdivide, float target_motion,
                            int max_islands, int32_t out_counts[4], int32_t* out_table, void* out_labels, float* out_field) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, out_counts && out_table && (entries || n == 0), "detect_islands: null host pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int d = ofps::block_dim_host(min_size, subdivide);
    OFPS_REQUIRE(ctx, d >= 1 && d <= ofps::kMaxDetectDim, "detect_islands: block_dim %d outside [1,160]", d);
    OFPS_REQUIRE(ctx, max_islands >= 1 && max_islands <= ofps::kMaxIslands, "detect_islands: max_islands %d outside [1, %d]", max_islands, ofps::kMaxIslands);
    const size_t cells = (size_t)d * d, bytes = ofps::islands_block_bytes(max_islands, d);
    auto* d_ent = static_cast<float4*>(ofps::scratch(ctx, ofps::S_ENTRIES, n * sizeof(float4)));
    auto* d_blk = static_cast<char*>(ofps::scratch(ctx, ofps::S_ISL_OUT, bytes));
    auto* d_out = out_field ? static_cast<float2*>(ofps::scratch(ctx, ofps::S_BEST, cells * sizeof(float2))) : nullptr;
    if (!d_ent || !d_blk || (out_field && !d_out)) return OFPS_HIP_ENOMEM;
    if (n) OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_ent, entries, n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    ofps::IslandsOut o = ofps::islands_blocks(d_blk, max_islands, d);
    o.field = d_out;
    int rc = ofps::detect_islands_device(ctx, d_ent, n, 1, min_size, subdivide, target_motion, max_islands, o);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_counts, d_blk, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // only the listed rows travel
    const int n_listed = out_counts[3] < 0 ? 0 : (out_counts[3] > max_islands ? max_islands : out_counts[3]);
    if (n_listed) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_table, d_blk + 16, (size_t)n_listed * 32, hipMemcpyDeviceToHost, ctx->stream));
    if (out_labels) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_labels, d_blk + 16 + (size_t)max_islands * 32, cells * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    if (out_field) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_field, d_out, cells * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_set_detect_islands(ofps_hip_ctx* ctx, int max_islands) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, max_islands >= 0 && max_islands <= ofps::kMaxIslands, "set_detect_islands: %d outside [0, %d] (0 = off)", max_islands, ofps::kMaxIslands);
    ctx->opt.detect_islands = max_islands;
    return OFPS_HIP_OK;
}

int ofps_hip_get_detect_islands(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.detect_islands : OFPS_HIP_EINVAL; }

int ofps_hip_frame_islands(ofps_hip_ctx* ctx, int item, int32_t out_counts[4], int32_t* out_table, int capacity, void* out_labels) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, out_counts && (out_table || capacity <= 0), "frame_islands: null pointer");
    const auto& last = ctx->isl_last;
    OFPS_REQUIRE(ctx, last.K > 0, "frame_islands: the last collected ticket was pushed with max_islands 0 or without the detector");
    OFPS_REQUIRE(ctx, item >= 0 && item < last.items, "frame_islands: item %d outside [0, %d)", item, last.items);
    const char* blk = last.data + ofps::ticket_block_bytes(last.K, last.dim, last.T) * item;
    int32_t counts[4];
    memcpy(counts, blk, sizeof(counts));
    OFPS_REQUIRE(ctx, capacity >= counts[3], "frame_islands: capacity %d is below the %d listed islands", capacity, counts[3]);
    memcpy(out_counts, counts, sizeof(counts));
    if (counts[3] > 0) memcpy(out_table, blk + 16, (size_t)counts[3] * 32);
    if (out_labels) memcpy(out_labels, blk + 16 + (size_t)last.K * 32, (size_t)last.dim * last.dim * sizeof(uint16_t));
    return OFPS_HIP_OK;
}

}  // extern "C"
