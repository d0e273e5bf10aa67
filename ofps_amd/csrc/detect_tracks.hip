// detect_tracks.hip -- A5t: island tracks (include/ofps_hip.h).  A small all-integer tracker behind the islands kernel (detect.hip, A5i): it
// follows the listed islands of one frame sequence across frames and gives every one an id that is never reused, an age, a hit count and the
// integer sums of its cells' quantised motion.  Build-defined and off by default, as A5i is.
//
// One workgroup of 1,024 threads per sequence; the items of a call are stepped in order INSIDE the launch, because step j reads step j - 1's
// state -- the state then crosses device memory once per launch and not once per item, and a batch ticket is one launch whatever its length.
// LDS holds the state for the whole launch: the owner map (u16 per cell: slot + 1, 0 = none), the gone map (u8 per cell), the slot table.  One
// step:
//   * motion: one pass over the cells, q(x) and q(y) into per-rank int64 accumulators by LDS atomics; a wave whose listed cells all belong to
//     one rank -- every wave inside a large island -- reduces in registers first
//   * overlap: the matrix O[r][s] does not fit beside the maps at T = 256 (256 KiB), so it is built `rows` ranks at a time (64 KiB), one pass
//     over the cells per block of ranks.  A lane sums its (2 reach + 1)^2 window in a register for the first owner it meets -- inside a
//     footprint the only one -- and issues an atomic at once only for a cell of another owner; a wave whose lanes all end with one (rank,
//     owner) pair reduces before lane 0 issues ONE atomic.  One island over its own footprint at reach 4 is then 400 LDS atomics, not 2 M
//   * match: wave 0 alone, the block's ranks in order: a 64-bit key (O, ~id, slot) per candidate slot, four slots a lane, a butterfly max;
//     every slot's entry is read and written by the one lane that owns it, so the rounds need no barrier
//   * paint, expire, rows out.
// Everything is integer and independent of the order of the atomics; the one float operation is q.
#include "common.hpp"

namespace ofps {

namespace {

constexpr uint32_t kNone = 0xFFFFu;
constexpr int kTrackHeader = 16;         // state: [t, next_id - 1, 0, 0] int32, then 4 int32 per slot, then the owner and the gone map

__host__ __device__ inline uint32_t pad16(uint32_t b) { return (b + 15u) & ~15u; }

struct TrackLayout {                     // the state's bytes and the kernel's dynamic LDS, the same offsets on both sides
    uint32_t slots, owner, gone, bytes;  // state (device or host memory); 32 bits: all of it is below 160 KiB, and the kernel keeps them in scalar registers
    uint32_t l_owner, l_gone, l_over, l_slot, l_msum, l_row, lds;
    int rows;                            // ranks per overlap block
};

__host__ __device__ inline TrackLayout track_layout(int dim, int T) {
    const uint32_t cells = (uint32_t)(dim * dim);
    TrackLayout L;
    L.slots = kTrackHeader;
    L.owner = L.slots + (uint32_t)T * 16;
    L.gone = L.owner + pad16(cells * 2);
    L.bytes = L.gone + pad16(cells);
    int rows = 16384 / T;                // 64 KiB of u32
    L.rows = rows < T ? rows : T;
    L.l_owner = 0;
    L.l_gone = pad16(cells * 2);
    L.l_over = L.l_gone + pad16(cells);
    L.l_slot = L.l_over + pad16((uint32_t)(L.rows * T) * 4);
    L.l_msum = L.l_slot + (uint32_t)T * 16;
    L.l_row = L.l_msum + (uint32_t)T * 16;
    L.lds = L.l_row + pad16((uint32_t)T * 4);
    return L;
}

// item j's inputs and outputs lie j * stride elements behind the base; cells may be null
struct TracksIO {                        // (strides of 32 bits: a block is below 1 MiB)
    const int* counts; const uint16_t* labels; const float2* cells; int* out_counts; int* out_tracks;
    uint32_t counts_stride, labels_stride, cells_stride, out_counts_stride, out_tracks_stride;
};

__device__ inline int q24(float v) {                                      // A5t's q: exact product, one rounding to nearest even
    if (v != v) return 0;
    v = fminf(fmaxf(v, -64.0f), 64.0f);
    return (int)rintf(v * 16777216.0f);
}
__device__ inline int wsum(int v) { for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ inline long long wsum64(long long v) {
    for (int o = 32; o; o >>= 1) {
        const int lo = __shfl_xor((int)(uint32_t)(unsigned long long)v, o), hi = __shfl_xor((int)((unsigned long long)v >> 32), o);
        v += (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
    }
    return v;
}
__device__ inline unsigned long long wmax64(unsigned long long v) {
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(v >> 32), o);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}
__device__ inline int wmin(int v) { for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }

}  // namespace

__global__ __launch_bounds__(1024) void island_tracks_kernel(TracksIO io, int dim, int batch, int T, int reach, int G,
                                                             char* __restrict__ state) {
    extern __shared__ __attribute__((aligned(16))) unsigned char trk_lds[];
    const TrackLayout L = track_layout(dim, T);
    const int cells = dim * dim;
    const int tid = threadIdx.x, lane = tid & 63;
    uint16_t* owner = reinterpret_cast<uint16_t*>(trk_lds + L.l_owner);
    uint8_t* gone = trk_lds + L.l_gone;
    uint32_t* over = reinterpret_cast<uint32_t*>(trk_lds + L.l_over);
    int* slot = reinterpret_cast<int*>(trk_lds + L.l_slot);              // id, born, hits, last
    unsigned long long* msum = reinterpret_cast<unsigned long long*>(trk_lds + L.l_msum);
    int* rowslot = reinterpret_cast<int*>(trk_lds + L.l_row);

    {
        const uint16_t* g_owner = reinterpret_cast<const uint16_t*>(state + L.owner);
        const uint8_t* g_gone = reinterpret_cast<const uint8_t*>(state + L.gone);
        const int* g_slot = reinterpret_cast<const int*>(state + L.slots);
        for (int i = tid; i < cells; i += 1024) { owner[i] = g_owner[i]; gone[i] = g_gone[i]; }
        for (int i = tid; i < 4 * T; i += 1024) slot[i] = g_slot[i];
    }
    int t = reinterpret_cast<const int*>(state)[0];
    int handed = reinterpret_cast<const int*>(state)[1];                 // ids handed out so far: the next one is handed + 1 (wave 0 keeps it)
    __syncthreads();

    for (int j = 0; j < batch; ++j) {
        const int* counts = io.counts + (size_t)j * io.counts_stride;
        const uint16_t* labels = io.labels + (size_t)j * io.labels_stride;
        const float2* f = io.cells ? io.cells + (size_t)j * io.cells_stride : nullptr;
        int n = counts[3];
        n = n < 0 ? 0 : n;
        n = n > T ? T : n;                                               // (n_listed <= K by A5i; every index below is bounded by T)
        t += 1;

        for (int i = tid; i < 2 * n; i += 1024) msum[i] = 0ull;
        for (int i = tid; i < n; i += 1024) rowslot[i] = -1;
        __syncthreads();

        // ---- motion sums
        if (f && n > 0)
            for (int base = 0; base < cells; base += 1024) {             // every wave whole: the reductions read all 64 lanes
                const int i = base + tid;
                uint32_t l = kNone;
                if (i < cells) l = labels[i];
                const bool act = l < (uint32_t)n;
                const unsigned long long mask = __ballot(act);
                if (!mask) continue;
                int qx = 0, qy = 0;
                if (act) { const float2 m = f[i]; qx = q24(m.x); qy = q24(m.y); }
                const uint32_t l0 = (uint32_t)__shfl((int)l, __ffsll((long long)mask) - 1);
                if (__all(!act || l == l0)) {
                    const long long sx = wsum64(qx), sy = wsum64(qy);
                    if (lane == 0) { atomicAdd(&msum[2 * l0], (unsigned long long)sx); atomicAdd(&msum[2 * l0 + 1], (unsigned long long)sy); }
                } else if (act) {
                    atomicAdd(&msum[2 * l], (unsigned long long)(long long)qx);
                    atomicAdd(&msum[2 * l + 1], (unsigned long long)(long long)qy);
                }
            }

        // ---- overlap and match, a block of ranks at a time
        unsigned claimed = 0;                                            // wave 0: bit k = slot lane + 64 k was claimed in this step
        for (int b0 = 0; b0 < n; b0 += L.rows) {
            const int nb = min(L.rows, n - b0);
            for (int i = tid; i < nb * T; i += 1024) over[i] = 0;
            __syncthreads();
            for (int base = 0; base < cells; base += 1024) {
                const int i = base + tid;
                uint32_t l = kNone;
                if (i < cells) l = labels[i];
                const bool act = l >= (uint32_t)b0 && l < (uint32_t)(b0 + nb);
                if (!__ballot(act)) continue;
                int s0 = -1, c0 = 0;
                if (act) {
                    uint32_t* row = over + (size_t)(l - b0) * T;
                    const int x = i % dim, y = i / dim;
                    const int y_lo = max(y - reach, 0), y_hi = min(y + reach, dim - 1);
                    const int x_lo = max(x - reach, 0), x_hi = min(x + reach, dim - 1);
                    for (int yy = y_lo; yy <= y_hi; ++yy)
                        for (int xx = x_lo; xx <= x_hi; ++xx) {
                            const int ow = owner[yy * dim + xx];
                            if (ow == 0 || ow > T) continue;
                            if (s0 < 0) s0 = ow - 1;
                            if (ow - 1 == s0) c0 += 1;
                            else atomicAdd(&row[ow - 1], 1u);
                        }
                }
                const bool has = s0 >= 0;
                const unsigned long long mask = __ballot(has);
                if (!mask) continue;
                const int key = has ? (int)((l - b0) * (uint32_t)T + (uint32_t)s0) : -1;
                const int key0 = __shfl(key, __ffsll((long long)mask) - 1);
                if (__all(!has || key == key0)) {
                    const int sum = wsum(has ? c0 : 0);
                    if (lane == 0) atomicAdd(&over[key0], (uint32_t)sum);
                } else if (has) {
                    atomicAdd(&over[key], (uint32_t)c0);
                }
            }
            __syncthreads();
            if (tid < 64) {
                for (int rr = 0; rr < nb; ++rr) {
                    const uint32_t* row = over + (size_t)rr * T;
                    unsigned long long best = 0;
                    int free_slot = 0x7FFFFFFF;
#pragma unroll 1
                    for (int k = 0; k < 4; ++k) {
                        const int s = lane + 64 * k;
                        if (s >= T) break;
                        const int id = slot[4 * s];
                        if (id == 0) { free_slot = min(free_slot, s); continue; }
                        if (claimed & (1u << k)) continue;
                        const uint32_t o = row[s];
                        if (!o) continue;
                        const unsigned long long key = ((unsigned long long)o << 40) | ((unsigned long long)(uint32_t)(0x7FFFFFFF - id) << 8) | (unsigned)s;
                        best = key > best ? key : best;
                    }
                    best = wmax64(best);
                    int s = -1;
                    if (best) {
                        s = (int)(best & 0xFFu);
                        if ((s & 63) == lane) { slot[4 * s + 2] += 1; slot[4 * s + 3] = t; claimed |= 1u << (s >> 6); }
                    } else {
                        const int fs = wmin(free_slot);
                        if (fs < T) {
                            s = fs;
                            handed += 1;
                            if ((s & 63) == lane) {
                                slot[4 * s] = handed; slot[4 * s + 1] = t; slot[4 * s + 2] = 1; slot[4 * s + 3] = t;
                                claimed |= 1u << (s >> 6);
                            }
                        }
                    }
                    if (lane == 0) rowslot[b0 + rr] = s;
                }
            }
            __syncthreads();
        }

        // ---- paint
        for (int i = tid; i < cells; i += 1024) {
            const uint32_t l = labels[i];
            const int s = l < (uint32_t)n ? rowslot[l] : -1;
            if (s >= 0) { owner[i] = (uint16_t)(s + 1); gone[i] = 0; }
            else if (owner[i]) {
                const int g = (int)gone[i] + 1;
                if (g > G) { owner[i] = 0; gone[i] = 0; }
                else gone[i] = (uint8_t)g;
            }
        }
        // ---- rows out (a slot matched in this step has last == t: it is not freed below)
        int* out = io.out_tracks + (size_t)j * io.out_tracks_stride;
        for (int r = tid; r < n; r += 1024) {
            const int s = rowslot[r];
            const unsigned long long mx = msum[2 * r], my = msum[2 * r + 1];
            int* row = out + (size_t)r * 8;
            row[0] = s >= 0 ? slot[4 * s] : 0;
            row[1] = s;
            row[2] = s >= 0 ? t - slot[4 * s + 1] + 1 : 0;
            row[3] = s >= 0 ? slot[4 * s + 2] : 0;
            row[4] = (int)(uint32_t)mx; row[5] = (int)(uint32_t)(mx >> 32);
            row[6] = (int)(uint32_t)my; row[7] = (int)(uint32_t)(my >> 32);
        }
        const int n_tracked = __syncthreads_count(tid < n && rowslot[tid] >= 0);
        // ---- expire
        if (tid < T && slot[4 * tid] != 0 && t - slot[4 * tid + 3] > G) {
            slot[4 * tid] = 0; slot[4 * tid + 1] = 0; slot[4 * tid + 2] = 0; slot[4 * tid + 3] = 0;
        }
        const int n_live = __syncthreads_count(tid < T && slot[4 * tid] != 0);
        if (tid == 0) {
            int* oc = io.out_counts + (size_t)j * io.out_counts_stride;
            oc[0] = n; oc[1] = n_tracked; oc[2] = n_live; oc[3] = t;
        }
    }

    uint16_t* g_owner = reinterpret_cast<uint16_t*>(state + L.owner);
    uint8_t* g_gone = reinterpret_cast<uint8_t*>(state + L.gone);
    int* g_slot = reinterpret_cast<int*>(state + L.slots);
    int* g_head = reinterpret_cast<int*>(state);
    for (int i = tid; i < cells; i += 1024) { g_owner[i] = owner[i]; g_gone[i] = gone[i]; }
    for (int i = tid; i < 4 * T; i += 1024) g_slot[i] = slot[i];
    if (tid == 0) { g_head[0] = t; g_head[1] = handed; g_head[2] = 0; g_head[3] = 0; }
}

static int tracks_check(ofps_hip_ctx* ctx, const char* who, int dim, int K, int T, int reach, int G) {
    OFPS_REQUIRE(ctx, dim >= 1 && dim <= kMaxDetectDim, "%s: dim %d outside [1, %d]", who, dim, kMaxDetectDim);
    OFPS_REQUIRE(ctx, K >= 1 && K <= kMaxIslands, "%s: max_islands %d outside [1, %d]", who, K, kMaxIslands);
    OFPS_REQUIRE(ctx, T >= 1 && T <= kMaxTracks, "%s: max_tracks %d outside [1, %d]", who, T, kMaxTracks);
    OFPS_REQUIRE(ctx, reach >= 0 && reach <= kMaxTrackReach, "%s: reach %d outside [0, %d]", who, reach, kMaxTrackReach);
    OFPS_REQUIRE(ctx, G >= 0 && G <= kMaxTrackGap, "%s: max_gap %d outside [0, %d]", who, G, kMaxTrackGap);
    return OFPS_HIP_OK;
}

// `batch` steps through one state, in order, in one launch on ctx->stream (the arguments have been checked)
static int tracks_device(ofps_hip_ctx* ctx, const TracksIO& io, int dim, int K, int batch, int T, int reach, int G, char* d_state) {
    const TrackLayout L = track_layout(dim, T);
    if (L.lds > 48 * 1024)
        OFPS_HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(island_tracks_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds));
    hipLaunchKernelGGL(island_tracks_kernel, dim3(1), dim3(1024), L.lds, ctx->stream, io, dim, batch, T, reach, G, d_state);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// the blocks of a ticket or of the host-pointer form: [A5i block][track_counts][tracks], `stride` bytes apart; the field in S_FIELD
static TracksIO tracks_of_blocks(ofps_hip_ctx* ctx, char* d_blocks, size_t stride, int K, int dim, int T) {
    char* trk = d_blocks + islands_block_bytes(K, dim);
    const uint32_t s4 = (uint32_t)(stride / 4);
    return {reinterpret_cast<const int*>(d_blocks), reinterpret_cast<const uint16_t*>(d_blocks + 16 + (size_t)K * 32),
            static_cast<const float2*>(ctx->scratch[S_FIELD].p), reinterpret_cast<int*>(trk), reinterpret_cast<int*>(trk + 16),
            s4, (uint32_t)(stride / 2), (uint32_t)(dim * dim), s4, s4};
}

void tracks_ticket_arm(ofps_hip_ctx* ctx, IslandsTicket* isl, int form, bool restart) {
    const auto& o = ctx->opt;
    isl->form = form;
    isl->T = form >= 0 && isl->K > 0 ? o.detect_tracks : 0;
    isl->reach = o.detect_track_reach; isl->gap = o.detect_track_gap;
    // a push without tracks, or the first frame of a stream, forgets the form's state: the next step starts from zeros
    if (form >= 0 && (isl->T == 0 || restart)) ctx->trk[form].live = false;
}

int tracks_ticket_device(ofps_hip_ctx* ctx, IslandsTicket* isl, int batch, int dim, char* d_blocks, size_t stride) {
    auto& f = ctx->trk[isl->form];
    const int T = isl->T;
    const size_t bytes = track_layout(dim, T).bytes;
    auto* d_state = static_cast<char*>(scratch(ctx, S_TRK_STATE + isl->form, bytes));
    if (!d_state) return OFPS_HIP_ENOMEM;
    const uint64_t gen = ctx->scratch[S_TRK_STATE + isl->form].gen;
    if (!f.live || f.T != T || f.reach != isl->reach || f.gap != isl->gap || f.dim != dim || f.gen != gen)
        OFPS_HIP_TRY(ctx, hipMemsetAsync(d_state, 0, bytes, ctx->stream));
    f.live = true; f.T = T; f.reach = isl->reach; f.gap = isl->gap; f.dim = dim; f.gen = gen;
    return tracks_device(ctx, tracks_of_blocks(ctx, d_blocks, stride, isl->K, dim, T), dim, isl->K, batch, T, isl->reach, isl->gap, d_state);
}

}  // namespace ofps

extern "C" {

size_t ofps_hip_island_tracker_bytes(int dim, int max_tracks) {
    if (dim < 1 || dim > ofps::kMaxDetectDim || max_tracks < 1 || max_tracks > ofps::kMaxTracks) return 0;
    return ofps::track_layout(dim, max_tracks).bytes;
}

int ofps_hip_track_islands_dev(ofps_hip_ctx* ctx, const void* d_counts, const void* d_table, const void* d_labels, const void* d_cells, int dim,
                               int max_islands, int batch, int max_tracks, int reach, int max_gap, void* d_state, void* d_out_track_counts,
                               void* d_out_tracks) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_counts && d_table && d_labels && d_out_track_counts && d_out_tracks, "track_islands: null device pointer");
    OFPS_REQUIRE(ctx, d_state, "track_islands: null state");
    OFPS_REQUIRE(ctx, ((uintptr_t)d_state & 3) == 0, "track_islands: the state is not 4-byte aligned");
    OFPS_REQUIRE(ctx, batch >= 1, "track_islands: batch must be >= 1");
    const int rc = ofps::tracks_check(ctx, "track_islands", dim, max_islands, max_tracks, reach, max_gap);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t cells = (uint32_t)(dim * dim);
    const ofps::TracksIO io{static_cast<const int*>(d_counts), static_cast<const uint16_t*>(d_labels), static_cast<const float2*>(d_cells),
                            static_cast<int*>(d_out_track_counts), static_cast<int*>(d_out_tracks), 4, cells, cells, 4, (uint32_t)max_tracks * 8};
    return ofps::tracks_device(ctx, io, dim, max_islands, batch, max_tracks, reach, max_gap, static_cast<char*>(d_state));
}

int ofps_hip_detect_tracks(ofps_hip_ctx* ctx, const float* entries, size_t n_per_item, int batch, float min_size, size_t subdivide, float target_motion,
                           int max_islands, int max_tracks, int reach, int max_gap, void* state, int32_t* out_counts, int32_t* out_table,
                           void* out_labels, int32_t* out_track_counts, int32_t* out_tracks) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, out_counts && out_table && out_track_counts && out_tracks && (entries || n_per_item == 0), "detect_tracks: null host pointer");
    OFPS_REQUIRE(ctx, state, "detect_tracks: null state");
    OFPS_REQUIRE(ctx, batch >= 1, "detect_tracks: batch must be >= 1");
    const int d = ofps_hip_block_dim(min_size, subdivide);
    int rc = ofps::tracks_check(ctx, "detect_tracks", d, max_islands, max_tracks, reach, max_gap);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int K = max_islands, T = max_tracks;
    const size_t cells = (size_t)d * d, isl_bytes = ofps::islands_block_bytes(K, d), stride = isl_bytes + ofps::track_block_bytes(T);
    const size_t st_bytes = ofps::track_layout(d, T).bytes, n_all = n_per_item * (size_t)batch;
    auto* d_ent = static_cast<float4*>(ofps::scratch(ctx, ofps::S_ENTRIES, n_all * sizeof(float4)));
    auto* d_blk = static_cast<char*>(ofps::scratch(ctx, ofps::S_ISL_OUT, stride * batch));
    auto* d_state = static_cast<char*>(ofps::scratch(ctx, ofps::S_TRK_HOST, st_bytes));
    if (!d_ent || !d_blk || !d_state) return OFPS_HIP_ENOMEM;
    hipStream_t s = ctx->stream;
    if (n_all) OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_ent, entries, n_all * sizeof(float4), hipMemcpyHostToDevice, s));
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_state, state, st_bytes, hipMemcpyHostToDevice, s));
    rc = ofps::detect_islands_blocks_device(ctx, d_ent, n_per_item, batch, min_size, subdivide, target_motion, K, d_blk, stride);
    if (rc != OFPS_HIP_OK) return rc;
    rc = ofps::tracks_device(ctx, ofps::tracks_of_blocks(ctx, d_blk, stride, K, d, T), d, K, batch, T, reach, max_gap, d_state);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(state, d_state, st_bytes, hipMemcpyDeviceToHost, s));
    // every item's rows travel whole: the rows at and behind n_listed / rows are unspecified
    for (int j = 0; j < batch; ++j) {
        const char* b = d_blk + stride * j;
        OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_counts + 4 * j, b, 16, hipMemcpyDeviceToHost, s));
        OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_table + (size_t)8 * K * j, b + 16, (size_t)K * 32, hipMemcpyDeviceToHost, s));
        if (out_labels)
            OFPS_HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint16_t*>(out_labels) + cells * j, b + 16 + (size_t)K * 32, cells * 2, hipMemcpyDeviceToHost, s));
        OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_track_counts + 4 * j, b + isl_bytes, 16, hipMemcpyDeviceToHost, s));
        OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_tracks + (size_t)8 * T * j, b + isl_bytes + 16, (size_t)T * 32, hipMemcpyDeviceToHost, s));
    }
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(s));
    return OFPS_HIP_OK;
}

int ofps_hip_set_detect_tracks(ofps_hip_ctx* ctx, int max_tracks, int reach, int max_gap) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, max_tracks >= 0 && max_tracks <= ofps::kMaxTracks, "set_detect_tracks: max_tracks %d outside [0, %d] (0 = off)", max_tracks, ofps::kMaxTracks);
    OFPS_REQUIRE(ctx, reach >= 0 && reach <= ofps::kMaxTrackReach, "set_detect_tracks: reach %d outside [0, %d]", reach, ofps::kMaxTrackReach);
    OFPS_REQUIRE(ctx, max_gap >= 0 && max_gap <= ofps::kMaxTrackGap, "set_detect_tracks: max_gap %d outside [0, %d]", max_gap, ofps::kMaxTrackGap);
    ctx->opt.detect_tracks = max_tracks; ctx->opt.detect_track_reach = reach; ctx->opt.detect_track_gap = max_gap;
    return OFPS_HIP_OK;
}

int ofps_hip_get_detect_tracks(ofps_hip_ctx* ctx, int* max_tracks, int* reach, int* max_gap) {
    if (!ctx) return OFPS_HIP_EINVAL;
    if (max_tracks) *max_tracks = ctx->opt.detect_tracks;
    if (reach) *reach = ctx->opt.detect_track_reach;
    if (max_gap) *max_gap = ctx->opt.detect_track_gap;
    return OFPS_HIP_OK;
}

int ofps_hip_frame_tracks(ofps_hip_ctx* ctx, int item, int32_t out_track_counts[4], int32_t* out_tracks, int capacity) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, out_track_counts && (out_tracks || capacity <= 0), "frame_tracks: null pointer");
    const auto& last = ctx->isl_last;
    OFPS_REQUIRE(ctx, last.K > 0 && last.T > 0, "frame_tracks: the last collected ticket was pushed with max_tracks 0, max_islands 0 or without the detector");
    OFPS_REQUIRE(ctx, item >= 0 && item < last.items, "frame_tracks: item %d outside [0, %d)", item, last.items);
    const size_t isl_bytes = ofps::islands_block_bytes(last.K, last.dim);
    const char* blk = last.data + (isl_bytes + ofps::track_block_bytes(last.T)) * item + isl_bytes;
    int32_t counts[4];
    memcpy(counts, blk, sizeof(counts));
    OFPS_REQUIRE(ctx, capacity >= counts[0], "frame_tracks: capacity %d is below the %d rows", capacity, counts[0]);
    memcpy(out_track_counts, counts, sizeof(counts));
    if (counts[0] > 0) memcpy(out_tracks, blk + 16, (size_t)counts[0] * 32);
    return OFPS_HIP_OK;
}

}  // extern "C"
