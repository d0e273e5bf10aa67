// common.hpp -- context object and error plumbing shared by the libofps_hip.so translation units.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/ofps_hip.h"

namespace ofps {

int set_error(ofps_hip_ctx* ctx, int code, const char* fmt, ...);

// The streaming front doors (pipeline.hip, dense_decoder.hip, multi.hip) number their tickets 0, 1, 2, ... and keep the newest N in a
// ring; the caller sees the low 31 bits of the number.
inline int ticket_id(long number) { return (int)(number & 0x7FFFFFFF); }
// the number of the ticket with this id among the newest `n` handed out (numbers next - n .. next - 1), or -1
inline long ticket_number(long next, int n, int id) {
    for (long k = next - 1; k >= 0 && k >= next - n; --k) if (ticket_id(k) == id) return k;
    return -1;
}

// Ticket: { bool pending; hipEvent_t done; ... }.  pending: pushed, not yet collected; done: everything of the ticket, read-backs included.
template <class Ticket, int N>
struct TicketRing {
    Ticket entry[N]; long next = 0;      // next: the number the next push gets
    Ticket& at(long number) { return entry[number % N]; }
    Ticket* find(int id) { const long k = ticket_number(next, N, id); return k < 0 ? nullptr : &at(k); }
    bool any_pending(const Ticket* but = nullptr) const { for (const Ticket& t : entry) if (t.pending && &t != but) return true; return false; }
    bool other_pending() const { return any_pending(&entry[next % N]); }     // ... but the one the next push would take
    hipError_t drain(bool forget = true) {       // waits for everything in flight [and marks it collected]
        for (Ticket& t : entry) {
            const hipError_t e = t.pending && t.done ? hipEventSynchronize(t.done) : hipSuccess;
            if (e != hipSuccess) return e;
            if (forget) t.pending = false;
        }
        return hipSuccess;
    }
    // a wait entry point's ticket: in flight and not yet collected -- else nullptr, the error set in that entry point's own words
    Ticket* claim(ofps_hip_ctx* ctx, int id, const char* who, const char* collected) {
        Ticket* t = find(id);
        if (!t) set_error(ctx, OFPS_HIP_EINVAL, "%s: ticket %d is not in flight", who, id);
        else if (!t->pending) { set_error(ctx, OFPS_HIP_EINVAL, "%s: ticket %d %s collected", who, id, collected); t = nullptr; }
        return t;
    }
    int commit() { at(next).pending = true; return ticket_id(next++); }      // the LAST thing a push does: one that failed half-way changed nothing here
};

// What a fused ticket answers per frame, as the detector's and the estimator's last kernels store it (tail.hip).  The per-frame SAD
// ticket (pipeline.hip: PipeOut) and the dense decoders' ticket (dense_decoder.hip: behind the records) hold one; a batch ticket holds
// a BatchBlock.
struct TailRecord {
    int result[4];                       // has_motion, area, dim, 0
    float quat[4];                       // (w, i, j, k)
};
static_assert(sizeof(TailRecord) == 32 && offsetof(TailRecord, quat) == 16 && sizeof(TailRecord::quat) == sizeof(float4), "result record layout");
// A batch ticket's result block of n frames: [n results][n quaternions][n kept counts, only when the ticket is `counted`: the batch filter
// or hip_klt].  The same layout in the push's device scratch and in the ticket's page-locked memory; nobody else spells it
constexpr size_t kBatchResult = sizeof(TailRecord::result);
static_assert(kBatchResult + sizeof(TailRecord::quat) == sizeof(TailRecord), "batch block layout");
struct BatchBlock {
    size_t n; bool counted;
    constexpr size_t quat_at() const { return n * kBatchResult; }
    constexpr size_t kept_at() const { return n * sizeof(TailRecord); }
    constexpr size_t bytes() const { return kept_at() + (counted ? n * sizeof(uint32_t) : 0); }
    int* result(char* base, size_t j) const { return reinterpret_cast<int*>(base) + 4 * j; }
    float4* quat(char* base, size_t j) const { return reinterpret_cast<float4*>(base + quat_at()) + j; }
    uint32_t* kept(char* base) const { return counted ? reinterpret_cast<uint32_t*>(base + kept_at()) : nullptr; }      // word j: frame j's
};
static_assert(BatchBlock{1, false}.bytes() == 32 && BatchBlock{1, true}.bytes() == 36 && BatchBlock{5, true}.bytes() == 5 * 32 + 5 * 4, "batch block size");
static_assert(BatchBlock{1, false}.quat_at() == 16 && BatchBlock{1, true}.quat_at() == 16 && BatchBlock{5, true}.quat_at() == 5 * 16, "batch block quaternions");
static_assert(BatchBlock{1, false}.kept_at() == 32 && BatchBlock{1, true}.kept_at() == 32 && BatchBlock{5, true}.kept_at() == 5 * 32, "batch block counts");
// A dense decoder's result block: [count, pad x 3][records x max_records] and, behind a fused ticket's records, [TailRecord][detector field
// dim x dim].  The ticket's page-locked memory, ofps_hip_lk_decode's, and (plain) the fused push's device copy of the records; nobody else
// spells it.  result / quat / field: null when the block is not fused
struct DenseBlock {
    size_t max_records; bool fused; int dim;
    static constexpr size_t kHeader = 16;
    constexpr size_t tail_at() const { return kHeader + max_records * sizeof(float4); }
    constexpr size_t bytes() const { return tail_at() + (fused ? sizeof(TailRecord) + (size_t)dim * dim * sizeof(float2) : 0); }
    uint32_t* count(char* base) const { return reinterpret_cast<uint32_t*>(base); }
    float4* records(char* base) const { return reinterpret_cast<float4*>(base + kHeader); }
    int* result(char* base) const { return fused ? reinterpret_cast<int*>(base + tail_at() + offsetof(TailRecord, result)) : nullptr; }
    float4* quat(char* base) const { return fused ? reinterpret_cast<float4*>(base + tail_at() + offsetof(TailRecord, quat)) : nullptr; }
    float2* field(char* base) const { return fused ? reinterpret_cast<float2*>(base + tail_at() + sizeof(TailRecord)) : nullptr; }
};
static_assert(DenseBlock::kHeader % sizeof(float4) == 0 && sizeof(TailRecord) % sizeof(float4) == 0, "records, quaternion and field stay 16-byte aligned");
static_assert(DenseBlock{312, false, 0}.bytes() == 16 + 312 * 16 && DenseBlock{312, false, 0}.tail_at() == 16 + 312 * 16, "dense block, plain");
static_assert(DenseBlock{312, true, 14}.bytes() == 16 + 312 * 16 + 32 + 14 * 14 * 8 && DenseBlock{312, true, 14}.tail_at() == 16 + 312 * 16, "dense block, fused");
static_assert(DenseBlock{12600, true, 23}.bytes() == 16 + 12600 * 16 + 32 + 23 * 23 * 8 && DenseBlock{12600, true, 23}.tail_at() == 16 + 12600 * 16, "dense block, fused and reduced");
// What every fused wait answers: zeros and the identity quaternion, then what the ticket has.  n_vectors: already clamped by the caller;
// result (int[4]) / quat (float[4]): null for a stage that did not run or a frame without vectors; they need no alignment
inline void fill_frame_result(ofps_hip_frame_result* out, int have_vectors, size_t n_vectors, const void* result, const void* quat) {
    memset(out, 0, sizeof(*out));
    out->quat[0] = 1.0f;
    out->have_vectors = have_vectors;
    out->n_vectors = n_vectors;
    if (result) {
        int res[4];
        memcpy(res, result, sizeof(res));
        out->has_motion = res[0]; out->area = (size_t)res[1]; out->dim = res[2];
    }
    if (quat) memcpy(out->quat, quat, sizeof(out->quat));
}
inline int padded_stride(int W) { return (W + 63) & ~63; }     // the device rows of every repacked frame: 64-byte multiples, so any host stride is accepted
constexpr int kMaxDetectDim = 160;       // the detector's field is at most 160 x 160 vectors
constexpr size_t kMaxFieldBytes = (size_t)kMaxDetectDim * kMaxDetectDim * sizeof(float2);

inline void destroy(hipEvent_t e) { if (e) (void)hipEventDestroy(e); }
inline void destroy(hipStream_t s) { if (s) (void)hipStreamDestroy(s); }
inline void free_host(void* p) { if (p) (void)hipHostFree(p); }

// A5i (detect.hip): what a fused ticket pushed with max_islands = K > 0 and the detector on carries beside its result block.  One block
// per item: [counts, int32 x 4][table, int32 x 8 x K][labels, u16 x dim x dim, padded to 16 bytes], made in device scratch by the islands
// kernel and copied to `pinned` behind it, on the stream the detector ran on.  Items in front of `first` yielded no vectors (a stream's
// first frame): nothing was enqueued for them, their islands are none.  K == 0: the ticket has no islands
constexpr int kMaxIslands = 6400;        // the most 8-connected components a 160 x 160 grid holds
inline size_t islands_block_bytes(int K, int dim) { return 16 + (size_t)K * 32 + (((size_t)dim * dim * sizeof(uint16_t) + 15) & ~size_t(15)); }
struct IslandsTicket {
    void* pinned = nullptr; size_t cap = 0;
    int K = 0, items = 0, first = 0, dim = 0;
    int T = 0, reach = 0, gap = 0, form = -1;     // A5t: the context's track settings at this push and the stream form whose state it steps
    void release() { free_host(pinned); }
};
// A5t (detect_tracks.hip): a ticket pushed with max_tracks = T > 0 as well carries [track_counts, int32 x 4][tracks, int32 x 8 x T] behind every
// item's A5i block, whose layout does not change.  Each of the three stream forms owns one tracker state in context scratch (S_TRK_STATE +
// form); `live` says that the state continues the settings and the grid below -- anything else starts from zeros (one memset in front of the
// step, on its stream).  Steps of one form run in stream order: the detector's chain of ticket k + 1 lies behind ticket k's on whichever of
// the two streams it runs (tail.hip: the side stream is forked behind and joined into the compute stream by every push)
constexpr int kMaxTracks = 256, kMaxTrackReach = 4, kMaxTrackGap = 255;
enum TrackFormId { TRK_PIPE = 0, TRK_BATCH = 1, TRK_DENSE = 2, kTrackForms = 3 };
inline size_t track_block_bytes(int T) { return T > 0 ? 16 + (size_t)T * 32 : 0; }
inline size_t ticket_block_bytes(int K, int dim, int T) { return islands_block_bytes(K, dim) + track_block_bytes(T); }
struct TrackForm { bool live = false; int T = 0, reach = 0, gap = 0, dim = 0; uint64_t gen = 0; };

// Farneback's state across calls (farneback.hip).  hip_flow in the stream forms: the pyramid + polynomial expansion of a pair's second
// frame is the next pair's first, and the NEW frame's is made on the upload's stream beside the previous pair's flow.  Frames of the
// stream carry ids (never reused); `cache.id[i]` is the frame whose expansion planes are in R slot i of the S_FB_WORK allocation of
// generation `gen`, made with these parameters.
struct FarnebackState {
    static constexpr int kSlots = 3;     // expansion-plane slots per layer: the frames of two pairs in flight (k - 1, k, k + 1)
    struct Cache {
        uint64_t id[kSlots] = {0, 0, 0}; // the stream frame whose planes a slot holds (0 = none)
        int W = 0, H = 0, K = 0, poly_n = 0;
        double poly_sigma = 0;
        uint64_t gen = 0;
    } cache;
    hipEvent_t prep_done = nullptr;      // the last pyramid + expansion of this context (its T / I temporaries are shared; prepares may run on two streams)
    bool prep_recorded = false;          // a prepare has been enqueued (on prep_stream) since the context was made
    hipStream_t prep_stream = nullptr;
    hipStream_t prep_synced = nullptr;   // a stream that has been ordered behind the latest prepare by its caller (the stream forms' `uploaded` event)
    uint64_t cache_hits = 0;             // (tests: how many calls skipped the first frame's pyramid + expansion)
    struct PrevFlow { bool valid = false; int W = 0, H = 0; uint64_t id = 0, gen = 0; } prev_flow;     // S_FB_FLOW holds the flow of the pair whose second frame has this id
    void release() { destroy(prep_done); }
};

// ---- the three streaming front doors' state: a ring of device frame slots, two tickets in flight, the new frame uploaded on a copy stream
// beside the previous ticket's work.  release(): for ofps_hip_destroy; sync_side_streams(): before the context moves to another compute stream.
// per-frame SAD pipeline (pipeline.hip: ofps_hip_push_frame[_async] / ofps_hip_frame_wait): frame k lives in slot k % 3 of S_PIPE_FRAMES
struct PipeStream {
    static constexpr int kSlots = 3, kTickets = 2;
    int w = 0, h = 0;
    long frames = 0;                     // frames pushed since the last reset
    hipStream_t copy_stream = nullptr;
    hipStream_t aux_stream = nullptr;    // the detector runs here beside the estimator (both read the same vectors)
    hipEvent_t fork = nullptr, join = nullptr;
    hipEvent_t uploaded[kSlots] = {};    // H2D of the frame in this slot finished (recorded on the copy stream)
    hipEvent_t slot_read[kSlots] = {};   // last search that reads this slot finished (recorded on the compute stream)
    bool slot_read_valid[kSlots] = {};
    bool uploaded_on_compute[kSlots] = {};   // the upload was enqueued on the compute stream (ordered by it)
    struct Ticket {
        bool pending = false; hipEvent_t done = nullptr;
        void* pinned = nullptr;          // page-locked PipeOut block for the result read-back
        int have_vectors = 0, run_detector = 0, run_estimator = 0;
        int gated = 0;                   // pushed with the contrast gate or the consistency check on: n_vectors is the kept count in the page-locked block
        size_t n_vectors = 0;
        IslandsTicket isl;               // A5i
    };
    hipEvent_t gate_done = nullptr;      // contrast gate and intra test (sad_gate.hip): the keep flags and activities of the newest frame, made on aux_stream beside the search (created with the first gated push)
    TicketRing<Ticket, kTickets> ring;
    void release() {
        for (auto& t : ring.entry) { free_host(t.pinned); destroy(t.done); t.isl.release(); }
        for (int k = 0; k < kSlots; ++k) { destroy(uploaded[k]); destroy(slot_read[k]); }
        destroy(copy_stream); destroy(aux_stream); destroy(fork); destroy(join); destroy(gate_done);
    }
    hipError_t sync_side_streams() {
        const hipError_t e = copy_stream ? hipStreamSynchronize(copy_stream) : hipSuccess;
        return e == hipSuccess && aux_stream ? hipStreamSynchronize(aux_stream) : e;
    }
};

// batched form of the same pipeline (ofps_hip_push_frames_async / ofps_hip_frames_wait): n frames per ticket, ONE upload, ONE search
// launch over the batch's pairs, ONE read-back.  Two batch buffers of (capacity + 1) frames alternate in S_BATCH_FRAMES: slot 0 holds the
// last frame of the previous batch (the first pair's previous frame).  Its stream of frames is separate from the single-frame calls';
// its uploads run on the per-frame pipeline's copy stream.
struct BatchStream {
    static constexpr int kTickets = 2;
    int w = 0, h = 0;
    void* last_frame = nullptr;          // device address of the newest frame of the batched stream
    // N3pb (both prediction settings 1, the KLT decoder): the raw slots of the newest frame's pair lie in half `half` of S_KLT_BATCH_PRED; the
    // next ticket's first item starts from them if it is chained too, on the same lattice and the same allocation.  The halves alternate by
    // ticket: a ticket of one frame reads one and writes the other.  Written and read on the compute stream alone
    struct KltPred { bool valid = false; int half = 0, w = 0, h = 0, cell = 0; uint64_t gen = 0; } klt_pred;
    struct Ticket {
        bool pending = false;
        hipEvent_t done = nullptr, uploaded = nullptr, prev_copied = nullptr;
        bool prev_copied_valid = false;
        void* pinned = nullptr; size_t pinned_cap = 0;       // a BatchBlock of n frames
        int n = 0, first_has_prev = 0, run_detector = 0, run_estimator = 0;
        int filtered = 0;                // pushed with the batch filter switch and a criterion on, or with hip_klt, and with a pair to run: the block's kept counts are n_vectors
        size_t n_vectors = 0;
        IslandsTicket isl;               // A5i
    };
    TicketRing<Ticket, kTickets> ring;
    void release() { for (auto& t : ring.entry) { free_host(t.pinned); destroy(t.done); destroy(t.uploaded); destroy(t.prev_copied); t.isl.release(); } }
};

// dense decoders, hip_lk and hip_flow (dense_decoder.hip: ofps_hip_lk_push_frame[_async] / ofps_hip_lk_frame_wait): frame k lives in
// slot k % 3 of S_LK_FRAMES; each ticket has a page-locked block (DenseBlock) that its last kernels write directly
struct DenseStream {
    static constexpr int kSlots = 3, kTickets = 2;
    int w = 0, h = 0;                    // the arriving frames' size
    int fw = 0, fh = 0, fmt = 0;         // the size of the frames in the ring (reduced with OFPS_HIP_LK_REDUCED) and the arriving frames' format
    long frames = 0;
    uint64_t frames_gen = 0;             // generation of the S_LK_FRAMES allocation the count refers to
    bool fb_params_valid = false; int fb_levels = 0, fb_radius = 0;     // the hip_flow stream's last Farneback parameters (a change with a ticket in flight is refused)
    uint64_t frame_serial = 0;           // frames of the stream carry ids (FarnebackState::cache); the id of the frame in each slot
    uint64_t slot_id[kSlots] = {0, 0, 0};
    // N3p (OFPS_HIP_FLOW_SPARSE with klt_prediction 1): the last pair's raw slots lie in half `pair & 1` of S_KLT_PRED; the pair that follows
    // reads them if nothing of what they were made under has changed
    struct KltPred { bool valid = false; long pair = 0; int fw = 0, fh = 0, cell = 0; unsigned flags = 0; uint64_t gen = 0; } klt_pred;
    hipStream_t copy_stream = nullptr;
    struct Ticket {
        bool pending = false;
        hipEvent_t done = nullptr, uploaded = nullptr;
        void* pinned = nullptr; size_t pinned_cap = 0;       // a DenseBlock of {max_records, fused, dim}
        int have_vectors = 0, gw = 0, gh = 0;
        size_t max_records = 0;
        // fused form (ofps_hip_lk_push_frame_fused[_async]): the tail's results sit behind the records
        int fused = 0, run_detector = 0, run_estimator = 0, dim = 0;
        IslandsTicket isl;               // A5i
    };
    TicketRing<Ticket, kTickets> ring;
    void* decode_pinned = nullptr; size_t decode_pinned_cap = 0;     // ofps_hip_lk_decode's block: a pair's records + their count (one wait)
    void release() {
        free_host(decode_pinned);
        for (auto& t : ring.entry) { free_host(t.pinned); destroy(t.done); destroy(t.uploaded); t.isl.release(); }
        destroy(copy_stream);
    }
    hipError_t sync_side_streams() { return copy_stream ? hipStreamSynchronize(copy_stream) : hipSuccess; }
};

}  // namespace ofps

struct ofps_hip_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;        // the stream work is enqueued on (own or caller's)
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    int num_cus = 0;
    int stream_cus = 0;                  // compute units `stream` may use (hipExtStreamGetCUMask; a caller's stream may carry a CU mask)
    int sad_mode = OFPS_HIP_SAD_EXHAUSTIVE;
    char err[512] = {0};

    // Diagnostic / A-B switches (INTEGRATION.md lists them).  Read from the environment ONCE, in ofps_hip_init; a live
    // context changes them through ofps_hip_set_option.  No entry point reads the environment after that.
    struct Options {
        int sad_force_block = 0;         // OFPS_HIP_SAD_KERNEL=block
        int densify_no_small = 0;        // OFPS_HIP_DENSIFY_NO_SMALL
        int almeida_path = 0;            // OFPS_HIP_ALMEIDA_PATH: 0 default, 1 step, 2 wg, 3 cluster
        int almeida_ept = 0;             // OFPS_HIP_ALMEIDA_EPT: 0 = cost model, else 1/2/4/8
        int almeida_block = 0;           // OFPS_HIP_ALMEIDA_BLOCK: 0 = 1024, else 256/1024
        int almeida_hier = 1;            // OFPS_HIP_ALMEIDA_HIER: 0 never, 1 when it pays, 2 always
        int almeida_fast = -1;           // OFPS_HIP_ALMEIDA_FAST: -1 by size, 0 exact, 1 folded
        int almeida_one_xcd = 1;         // OFPS_HIP_ALMEIDA_ONE_XCD: 0 never, 1 small clusters run on one XCD and exchange through its L2 (almeida.hip)
        int almeida_prof = 0;            // OFPS_HIP_ALMEIDA_PROF
        int lk_prof = 0;                 // OFPS_HIP_LK_PROF
        int fb_prepare_ahead = 1;        // OFPS_HIP_FB_PREPARE_AHEAD: a hip_flow stream's new frame is expanded on the upload's stream when it is pushed (0: inside the pair's flow, round 5's order)
        int lk_serial = 0;               // OFPS_HIP_LK_SERIAL: one launch per pyramid level instead of one for the pyramid
        int sad_motion_scale = 1;        // OFPS_HIP_SAD_MOTION_SCALE / ofps_hip_set_sad_motion_scale: 1 full-pel vectors, 4 quarter-pel refinement (sad_qpel.hip)
        int detect_compensate = 0;       // OFPS_HIP_DETECT_COMPENSATE / ofps_hip_set_detect_compensation: 0 the fused entry points' detector reads the raw vectors, 1 the vectors compensated with the frame's own quaternion (compensate.hip)
        int sad_gate = 0;                // OFPS_HIP_SAD_GATE / ofps_hip_set_sad_gate: 0 one record per lattice block, N >= 1 only blocks with at least N contrast-mask pixels of the current frame (sad_gate.hip)
        int sad_consistency = 0;         // OFPS_HIP_SAD_CONSISTENCY / ofps_hip_set_sad_consistency: 0 off, N in [1, 129] only blocks whose forward-backward residual is below N (sad_consistency.hip)
        int sad_levels = 1;              // OFPS_HIP_SAD_LEVELS / ofps_hip_set_sad_levels: 1 the plain search, 2 | 3 coarse-to-fine: the search runs on the frames halved levels - 1 times, a +-3 refinement per finer level (sad_hier.hip)
        int sad_predictors = 0;          // OFPS_HIP_SAD_PREDICTORS / ofps_hip_set_sad_predictors: 0 a refined block's one predictor is its parent's winner, 1 the parent's, its four lattice neighbours' and zero (sad_hier.hip, N1p); no effect at levels 1
        int sad_median = 0;              // OFPS_HIP_SAD_MEDIAN / ofps_hip_set_sad_median: 0 off, N in [1, 255] only blocks whose integer winner lies less than N pixels from the median of their kept lattice neighbours' (sad_median.hip, N1v)
        int sad_intra = 0;               // OFPS_HIP_SAD_INTRA / ofps_hip_set_sad_intra: 0 off, q in [1, 255] (sixteenths) only blocks whose integer winner's SAD lies below q/16 of the block's activity in the raw current frame (sad_intra.hip, N1i)
        int sad_cut = 0;                 // OFPS_HIP_SAD_CUT / ofps_hip_set_sad_cut: 0 off, P in [1, 100] a pair with at least P percent of its gated blocks intra yields no record; no effect while sad_intra is 0 (sad_intra.hip, N1i)
        int sad_split = 0;               // OFPS_HIP_SAD_SPLIT / ofps_hip_set_sad_split: 0 one record per kept block, T in [1, 4080] (sixteenths of a grey level per pixel) a kept block whose four sub-blocks together match better by at least T yields their four records (sad_split.hip, N1s)
        int sad_batch_filter = 0;        // OFPS_HIP_SAD_BATCH_FILTER / ofps_hip_set_sad_batch_filter: 0 the batched stream forms (ofps_hip_push_frames_async, the ofps_hip_multi_* workers' pushes) ignore gate, check and median test, 1 they follow them (include/ofps_hip.h N1b)
        int sad_prefilter = 0;           // OFPS_HIP_SAD_PREFILTER / ofps_hip_set_sad_prefilter: 0 the searches read the frames as they are, r in [1, 16] their mean-removed forms, box radius r (sad_prefilter.hip, N1m)
        // OFPS_HIP_DETECT_TRACKS, OFPS_HIP_DETECT_TRACK_REACH, OFPS_HIP_DETECT_TRACK_GAP / ofps_hip_set_detect_tracks: T = 0 off, T in [1, 256] a ticket
        // that lists islands follows them across frames as well, with this reach in cells [0, 4] and this gap in frames [0, 255] (detect_tracks.hip, A5t)
        int detect_tracks = 0, detect_track_reach = 1, detect_track_gap = 2;
        int detect_islands = 0;          // OFPS_HIP_DETECT_ISLANDS / ofps_hip_set_detect_islands: 0 the fused entry points' detector answers for the largest island alone, K in [1, 6400] a ticket that runs the detector lists up to K islands as well (detect.hip, A5i)
        // ofps_hip_set_klt: hip_klt's lattice cell (8 | 16 | 32), score window radius [1, 3], smallest score of a feature, smallest eigenvalue of
        // a template's structure tensor per pixel [1, 65535], residual limit in sixteenths of a grey level per pixel (0 = off) (klt.hip, N3)
        int klt_cell = 16, klt_score_radius = 2, klt_min_score = 1, klt_min_eig = 1, klt_max_residual = 0;
        // ofps_hip_set_klt_mean_removal: 1 = hip_klt tracks under the model "shift plus one brightness offset" (include/ofps_hip.h N3m)
        int klt_mean_removal = 0;
        // ofps_hip_set_klt_fb: hip_klt's forward-backward check, the round-trip limit F in 1/256 pixel, 0 = off (include/ofps_hip.h N3f)
        int klt_fb = 0;
        // ofps_hip_set_klt_prediction: 1 = the sparse stream forms start a pair's tracks from the previous pair's flow (include/ofps_hip.h N3p)
        int klt_prediction = 0;
        // OFPS_HIP_KLT_BATCH_PREDICTION / ofps_hip_set_klt_batch_prediction: 1 = with klt_prediction 1 as well, the batch form and the batched stream
        // (not the ofps_hip_multi_* workers) chain their items: each starts from the item before (include/ofps_hip.h N3pb)
        int klt_batch_prediction = 0;
        // OFPS_HIP_KLT_INTRA / ofps_hip_set_klt_intra: 0 off, q in [1, 255] (sixteenths) a kept track whose residual reaches q/16 of its window's
        // activity in the raw previous frame becomes status 6 and yields no record (klt_intra.hip, N3i)
        int klt_intra = 0;
        // OFPS_HIP_KLT_CUT / ofps_hip_set_klt_cut: 0 off, P in [1, 100] a pair with at least P percent of its candidates intra yields no record
        // (status 7); no effect while klt_intra is 0 (klt_intra.hip, N3i)
        int klt_cut = 0;
        // OFPS_HIP_BATCH_DECODER / ofps_hip_set_batch_decoder: 0 the batched stream forms (ofps_hip_push_frames_async, the ofps_hip_multi_* workers'
        // pushes) search with hip_sad, 1 they run hip_klt with these levels, window radius and iterations (include/ofps_hip.h N3b)
        int batch_decoder = 0, klt_levels = 4, klt_radius = 7, klt_iters = 10;
        int multi_rccl = 0;              // OFPS_HIP_MULTI_RCCL: ofps_hip_multi_init fans the shared key frame out by ncclBroadcast (multi.hip)
        // fault injectors: only builds with -DOFPS_HIP_TEST_HOOKS (libofps_hip_testhooks.so) can set them, and only
        // through ofps_hip_set_option -- never from the environment
        int test_almeida_fault = 0;      // OFPS_HIP_ALMEIDA_TEST_FAULT: workgroup (value - 1) withholds its step-3 granule
        int test_lk_fall = -1;           // OFPS_HIP_LK_TEST_FALL: every other tile hands over at this step
        int test_lk_wait_budget = 0;     // OFPS_HIP_LK_TEST_WAIT_BUDGET: 100 MHz ticks a tile waits for its parent's flag before it computes its ancestors itself (0 = the product's budget)
        int test_lk_order = 0;           // OFPS_HIP_LK_TEST_ORDER: the one-launch pyramid's blocks take their positions 1: in reverse, 2: permuted, after random delays
    } opt;

    ofps::PipeStream pipe;
    ofps::BatchStream batch;
    ofps::DenseStream dense;
    ofps::FarnebackState fb;
    // A5i: the islands of the most recently collected fused ticket, in host memory the context owns (detect.hip: islands_collect): `items`
    // blocks of islands_block_bytes(K, dim).  K == 0: that ticket had none
    struct IslandsLast { char* data = nullptr; size_t cap = 0; int K = 0, items = 0, dim = 0, T = 0; } isl_last;      // T > 0: A5t's rows behind every block
    ofps::TrackForm trk[ofps::kTrackForms];      // A5t: what each stream form's tracker state in S_TRK_STATE + form continues
    uint32_t lk_epoch = 0;               // lk_levels_kernel: tag of the last launch in the tile flags (S_LK_FLAGS)
    uint64_t lk_flags_gen = 0;           // generation of the flag buffer the tags refer to

    // cluster Almeida solver (almeida.hip): granule exchange buffer state.  Tags are unique per call (tag base advances
    // by 32 per launch), so the buffer is zeroed only when (re)allocated or when the 32-bit tag space wraps.
    uint32_t gran_tag_base = 0;
    uint64_t gran_zeroed_gen = 0;        // generation (Scratch::gen) of the allocation the zeroing was done for

    // grow-only device scratch owned by the context (staging for host-pointer entry points and
    // kernel workspaces); never shrinks, freed in ofps_hip_destroy.
    struct Scratch { void* p = nullptr; size_t cap = 0; uint64_t gen = 0; };   // gen: bumped by every (re)allocation of the slot
    static constexpr int kNumScratch = 66;
    Scratch scratch[kNumScratch];
};

namespace ofps {

enum ScratchSlot {
    S_FRAMES = 0, S_ENTRIES, S_BEST, S_FIELD, S_CELLS, S_WORK0, S_WORK1, S_WORK2, S_WORK3, S_RESULT,
    S_QUAT, S_WORK4, S_PIPE_FRAMES, S_PIPE_ENTRIES, S_PIPE_OUT, S_MASK, S_ENTRIES2, S_GRAN, S_SAD_LIST,
    // the estimator's own workspaces: it may run beside the detector (pipeline.hip), so the two share no slot
    S_ALM_PART, S_ALM_STATE, S_ALM_HYP, S_ALM_COUNTS, S_ALM_SEL, S_ALM_SELN, S_ALM_PROF, S_ALM_RECOVER,
    S_LK_FRAMES, S_BATCH_FRAMES, S_BATCH_ENTRIES, S_BATCH_OUT, S_BATCH_FIELD,
    // the one-launch LK pyramid's tile flags + helped-tile counter: they carry state ACROSS calls (epoch tags, never cleared), so the slot
    // is nobody else's (round 4: they sat in S_WORK3, which the densifier's per-cell tables also use -- a decode call wiped the counter,
    // and a begin[] value equal to a later launch's epoch would have read as "parent tile done")
    S_LK_FLAGS,
    S_FB_WORK,              // farneback.hip: blur / image / expansion / flow planes of one pair
    S_FB_FLOW,              // hip_flow streams with OFPS_HIP_FLOW_USE_PREVIOUS: the last pair's flow (the next pair's initial flow)
    S_XMAJOR,               // densify.hip, raster producers: the field + visited flag in (x, y)-sorted cell order (the record order)
    S_LK_MASKS,             // dense decoders, stream forms: one contrast mask per ticket in flight (made on the upload's stream, beside the previous pair's flow)
    S_SAD_QBEST,            // sad_qpel.hip: the integer winners when the caller of a quarter-pel search passes no out_best
    S_FE_RAW,               // frontend.hip: the frames as they arrive (colour and / or full size) when the decoder resizes / converts them: one per ticket in flight
    S_FE_RAW_PAIR,          // ... of the stateless calls (ofps_hip_lk_decode, ofps_hip_cv_frontend, ofps_hip_resize_linear): never the stream's staging, whose
                            // upload + front-end may still be running on the upload stream when such a call comes in
    S_DENSE_REC,            // dense decoders, fused stream form: [count, pad x 3][records] of the newest pair, in device memory for the detector + estimator
    S_GATE_RAW,             // hip_sad's contrast gate (sad_gate.hip): the search's one-record-per-block output, in front of the compaction
    S_GATE_BEST,            // ... and its (dx, dy, SAD) triples
    S_GATE_FLAGS,           // ... [counts, u32 per block][kept count, 16 bytes][keep flags, u8 per block], one per ticket in flight in the fused path
    S_COMP,                 // detect-compensation mode 1 (tail.hip): [quaternion per item][compensated records] -- the detector's input; the slots the
                            // record copy and the estimator read are never overwritten.  Written and read on the compute stream only
    S_CONS_FWD,             // hip_sad's consistency check (sad_consistency.hip): the forward search's integer winners, kept through a quarter-pel refinement
    S_CONS_BWD,             // ... the backward search's integer winners
    S_CONS_BWD_ENT,         // ... and its records, which nobody reads (the search kernels always write them).  All three: compute stream only
    S_HIER_PYR,             // hip_sad's search levels (sad_hier.hip): the halved frames of one search's two frame sets, every level above 0
    S_HIER_BEST,            // ... the winners of every level above 0
    S_HIER_ENT,             // ... and the top search's records, which nobody reads.  All three: compute stream only, written anew by every search
    S_SAD_PREF,             // hip_sad's mean removal (sad_prefilter.hip): the filtered frames of one search's two frame sets.  Compute stream only, written anew by every search
    S_MED_KEEP,             // hip_sad's median test (sad_median.hip): the outgoing keep flags, u8 per block, one per ticket in flight in the fused path (the incoming ones stay in S_GATE_FLAGS)
    S_INTRA,                // hip_sad's intra test (sad_intra.hip): [activity, u32 per block][candidate and intra counters, 2 x u32 per item], one per ticket in flight in the fused path
    S_ISL_WORK,             // the islands kernel (detect.hip, A5i): per item [qualifying roots' keys, u64][rank of every root, u16 per cell]
    S_ISL_OUT,              // ... and the blocks of a fused ticket or a host-pointer call ([counts][table][labels] per item), copied out behind the kernel on its stream
    S_SPLIT,                // hip_sad's split step (sad_split.hip, N1s): [raw slots, 4 records per block][sub triples, 12 i32 per block][slot flags, 4 u8 per block][split flags, u8 per block].  Compute stream only, written anew by every search
    S_KLT_PYR,              // hip_klt (klt.hip, N3): both frames' pyramid levels above 0.  Compute stream only, written anew by every call
    S_KLT_WORK,             // ... [features, 3 i32 per slot][raw records per slot][keep flags, u8 per slot], in front of the compaction
    S_KLT_HOST,             // ... the host-pointer forms' device-side inputs and outputs
    S_KLT_PRED,             // N3p: the sparse stream's raw slots of the last two pairs, 6 i32 per slot each.  Compute stream only
    S_KLT_BATCH_PRED,       // N3pb: the batched stream's raw slots of the last item of the last two chained tickets, 6 i32 per slot each.  Compute stream only
    S_TRK_STATE,            // A5t (detect_tracks.hip): the tracker state of the per-frame stream form, ...
    S_TRK_STATE_BATCH,      // ... of the batched form
    S_TRK_STATE_DENSE,      // ... and of the dense decoders' fused form (S_TRK_STATE + TrackFormId).  Each carries state ACROSS pushes: nobody else's slot
    S_TRK_HOST              // ... and the state of one ofps_hip_detect_tracks call, between its upload and its read-back
};
static_assert(S_TRK_HOST < ofps_hip_ctx::kNumScratch, "scratch table too small");

// Page-locked blocks that kernels write directly and the host reads after an event (ticket result blocks, ofps_hip_host_alloc):
// fine-grained host memory, asked for explicitly.  A/B builds (tools/read_ahead_bisect.sh) override the two constants with -D.
#ifndef OFPS_HIP_HOST_BLOCK_FLAGS
#define OFPS_HIP_HOST_BLOCK_FLAGS hipHostMallocCoherent
#endif
#ifndef OFPS_HIP_HOST_USER_FLAGS
#define OFPS_HIP_HOST_USER_FLAGS hipHostMallocCoherent
#endif
#ifndef OFPS_HIP_FRAME_WAIT_SPIN_US
#define OFPS_HIP_FRAME_WAIT_SPIN_US 500
#endif

int check_hip(ofps_hip_ctx* ctx, hipError_t e, const char* what);
// returns nullptr (and sets the error) on failure
void* scratch(ofps_hip_ctx* ctx, int slot, size_t bytes);

// ---- device-side stage entry points shared between translation units (all enqueue on ctx->stream)
// The two frame sets of one search: pair k reads prev_base + k*prev_pitch and cur_base + k*cur_pitch; a set with pitch 0 is one frame that
// every pair reads.  `pairs` travels beside it.  The refine kernels take one by value (sad_hier.hip: RefineParams): the member order is layout.
struct SadFrames {
    const uint8_t* prev_base;
    const uint8_t* cur_base;
    size_t prev_pitch, cur_pitch;
    int W, H, stride;
    // the n_frames - 1 pairs of a frame sequence: ref_mode 0 (k, k + 1), ref_mode 1 (0, k + 1).  The current frame of pair k is frame k + 1 in both
    static SadFrames sequence(const uint8_t* frames, size_t frame_pitch, int ref_mode, int W, int H, int stride) {
        return {frames, frames + frame_pitch, ref_mode ? 0 : frame_pitch, frame_pitch, W, H, stride};
    }
    SadFrames swapped() const { return {cur_base, prev_base, cur_pitch, prev_pitch, W, H, stride}; }       // the backward search's sets
    // What a stage that copies the sets of `pairs` pairs (mean removal, the levels' halving) has to copy, and where the copies lie.  Consecutive
    // pairs of one sequence (cur = prev + one frame) are a chain: pairs + 1 frames copied once, all counted in nprev; else two sets
    struct Sets {
        bool chain, prev_many, cur_many;
        long long nprev, ncur;
        long long cur_first() const { return chain ? 1 : nprev; }      // where the copies of cur begin: one frame behind prev for a chain, else behind the nprev frames
        // the same sets inside `buf`, frames `pitch` apart; a pitch of 0 stays 0
        SadFrames in(const uint8_t* buf, size_t pitch, int W, int H, int stride) const {
            return {buf, buf + (size_t)cur_first() * pitch, prev_many ? pitch : 0, cur_many ? pitch : 0, W, H, stride};
        }
    };
    Sets sets(int pairs) const {
        const bool chain = prev_pitch != 0 && prev_pitch == cur_pitch && cur_base == prev_base + prev_pitch;
        return {chain, prev_pitch != 0, cur_pitch != 0, chain ? (long long)pairs + 1 : (prev_pitch ? pairs : 1), chain ? 0 : (cur_pitch ? pairs : 1)};
    }
};
// integer_only: no quarter-pel refinement whatever the context's motion scale (the consistency check's backward search).
// d_int_best (motion scale 4 only): the integer winners are written here, not to S_SAD_QBEST / d_out_best, and are still there behind the
// refinement, which then writes its triples to d_out_best (or nowhere)
int sad_pairs_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int block, int range, void* d_out_entries, void* d_out_best,
                     bool integer_only = false, void* d_int_best = nullptr);
// the plain integer search alone (N1): what sad_pairs_device runs at one search level, and the top search of sad_hier_pairs_device
int sad_search_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int block, int range, void* d_out_entries, void* d_out_best);
// sad_hier.hip (include/ofps_hip.h N1h): the integer winners of a search over `levels` > 1 levels; never refines to quarter-pel and never
// looks at the context's levels or predictor mode, so it cannot come back to itself through the top search.  d_out_best may be null
constexpr int kSadHierRefine = 3;                           // the refinement's radius: 49 candidates in a 64-lane wave
constexpr int kSadHierPredictors = 6;                       // N1p: parent, four lattice neighbours, zero
constexpr int kSadHierMaxReach = 127;                       // 8 * reach + 6 <= 1023: the quarter-pel key's 10-bit fields
int sad_hier_reach(int range, int levels);                  // R_0, or -1
int sad_hier_check(ofps_hip_ctx* ctx, int W, int H, int block, int range, int levels);
int sad_hier_pairs_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int block, int range, int levels, int predictors, void* d_out_entries,
                          void* d_out_best);
// one pyramid step (what ofps_hip_sad_down2_dev enqueues for one frame), W x H -> (W >> 1) x (H >> 1), of `frames` frames src_pitch bytes apart,
// their halved forms dst_pitch apart, in one launch
int sad_down2_frames_device(ofps_hip_ctx* ctx, const uint8_t* src, size_t src_pitch, int W, int H, int src_stride, uint8_t* dst, size_t dst_pitch,
                            int dst_stride, long long frames);
// klt.hip (include/ofps_hip.h N3): hip_klt with the context's settings.  The decoder's limits on one call: levels, radius, iters, a frame of
// 8 .. 32768 pixels a side whose top level is at least 8 x 8, stride >= W -- what klt_check_call refuses, for every form of the decoder
constexpr int kKltMaxLevels = 6, kKltMaxRadius = 7, kKltMaxIters = 30, kKltMaxScoreRadius = 3, kKltMaxMinEig = 65535, kKltMaxResidual = 4080, kKltMaxFb = 4096;
int klt_check_call(ofps_hip_ctx* ctx, int W, int H, int stride, int levels, int radius, int iters, const char* who);
struct KltLattice { int nx, ny; size_t slots() const { return (size_t)nx * ny; } };      // a partial cell at the right and lower edge counts
inline KltLattice klt_lattice(int W, int H, int cell) { return {(W + cell - 1) / cell, (H + cell - 1) / cell}; }
// One run of the decoder over `pairs` pairs of `f`: score -> pyramid -> track -> (N3i) verdict and cut -> the ordered compaction, enqueued on
// ctx->stream only.  d_out: pairs x slots records, item k's kept records lead slot k; d_counts: pairs counts in device memory; d_slots
// (optional): 6 int32 per slot, item-major.  S_KLT_PYR and S_KLT_WORK are dead behind the compaction: the batched stream's tickets share them.
// batch = false: the one-pair kernels (pairs is 1); d_prev_slots (N3p, optional): the previous pair's raw slots, every feature starts from its
// slot's predicted guess.  batch = true (N3b): item k = the one-pair run on that pair, bit for bit, in a number of launches that does not depend
// on `pairs`.  chained (N3pb, batch only): the track step is `pairs` launches, one item each, in stream order; item k starts from item k - 1's raw
// slots, item 0 from d_prev_slots (null: from zero); d_last_slots (optional): the last item's raw slots go there and not into d_slots; neither
// it nor d_prev_slots may share a byte with d_slots or with each other
struct KltFlowCall {
    SadFrames f;
    int pairs, levels, radius, iters;
    float4* d_out; uint32_t* d_counts; int* d_slots;
    bool batch, chained;
    const int* d_prev_slots; int* d_last_slots;
};
int klt_flow_device(ofps_hip_ctx* ctx, const KltFlowCall& c);
// ... the one-pair form on two device frames: the set {d_prev, d_cur, pitches 0}
int klt_flow_device(ofps_hip_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_cur, int W, int H, int stride, int levels, int radius, int iters,
                    float4* d_out, uint32_t* d_count, int* d_slots, const int* d_prev_slots = nullptr);
// klt_intra.hip (include/ofps_hip.h N3i): hip_klt's intra test and scene-cut rule, between the track launch and the compaction.  What the
// driver hands over: the level-0 previous frames (pitch 0: one key frame for every item), the feature triples (pitch 0: one set), the
// tracks' quads, the keep flags the track launch wrote and the items' counters [candidates, intra], all but the frames and triples item-major,
// `ns` entries per item
constexpr int kKltIntraMax = 255, kKltCutMax = 100;
struct KltIntraCall {
    const uint8_t* frames; size_t frame_pitch;
    int W, H, stride, w, ns;
    const int* feat; size_t feat_pitch;          // 3 ints per slot; feat_pitch in ints
    const int* quads;                            // 4 ints per slot
    uint8_t* flags;
    uint32_t* counts;                            // 2 per item, zero before the first verdict launch
    int ratio, cut;
};
// verdict, and with c.cut > 0 the cut, for the items item0 .. item0 + items - 1, enqueued on ctx->stream.  d_slots (optional): the raw slots,
// 6 ints per slot, indexed as the flags are; statuses 6 and 7 are written there
int klt_intra_device(ofps_hip_ctx* ctx, const KltIntraCall& c, int item0, int items, int* d_slots);
// sad_prefilter.hip (include/ofps_hip.h N1m): F = clamp(v - box mean + 128), radius in [1, kSadPrefilterMax]
constexpr int kSadPrefilterMax = 16;
int sad_prefilter_device(ofps_hip_ctx* ctx, const uint8_t* src, size_t src_pitch, int W, int H, int src_stride, uint8_t* dst, size_t dst_pitch,
                         int dst_stride, long long frames, int radius);
// a search's two frame sets -> S_SAD_PREF; *filtered: the filtered frames, in the shape of `f`
int sad_prefilter_pairs_device(ofps_hip_ctx* ctx, int radius, const SadFrames& f, int pairs, SadFrames* filtered);
int sad_qpel_refine_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int block, int range, void* d_entries, const void* d_in_best,
                           void* d_out_best);
// d_n (densify_device, densify_device_raw, detect_device; optional): the entry counts live in device memory, one per item -- n is the capacity
// and the stride of every item, the first min(d_n[item], n) entries of an item count, and nothing about the launches depends on the counts
int densify_device(ofps_hip_ctx* ctx, const float4* d_entries, size_t n, int batch, int w, int h, float2* d_field,
                   uint32_t* d_cells, uint32_t** out_begin, uint32_t** out_end, const uint32_t* d_n = nullptr);
int densify_device_raw(ofps_hip_ctx* ctx, const float4* d_entries, size_t n, int batch, int w, int h, float2* d_field,
                       uint32_t* d_cells, uint32_t** out_begin, uint32_t** out_end, float2* d_sum, float* d_cnt,
                       const float* d_weights, const uint32_t* d_n = nullptr);
int densify_entries_device(ofps_hip_ctx* ctx, const float4* d_entries, size_t n, int w, int h, float2* d_field,
                           float4* d_out_entries, uint32_t* d_count);
int densify_raster_device(ofps_hip_ctx* ctx, const float4* d_entries, const uint8_t* d_mask, int W, int H, int w, int h,
                          float2* d_field, uint32_t** out_begin, uint32_t** out_end, float4* d_xmajor = nullptr);
int densify_raster_entries_device(ofps_hip_ctx* ctx, const float4* d_entries, const uint8_t* d_mask, int W, int H, int w, int h,
                                  float2* d_field, float4* d_out_entries, uint32_t* d_count);
// frontend.hip: cv-decoder's capped grid (cv-decoder/src/lib.rs:98-121) and its per-frame [resize ->] gray step (:124-135)
int frame_format_channels(int fmt);
void cv_grid(int W, int H, int max_w, int max_h, int* gw, int* gh);
int frontend_device(ofps_hip_ctx* ctx, const uint8_t* d_src, int W, int H, int stride, int fmt, bool to_gray, uint8_t* d_dst, int dw, int dh,
                    hipStream_t st = nullptr);
int contrast_mask_device(ofps_hip_ctx* ctx, const uint8_t* d_gray, int W, int H, int stride, uint8_t* d_mask, hipStream_t st = nullptr);   // st: nullptr = ctx->stream
int compact_entries_device(ofps_hip_ctx* ctx, const float4* d_in, const uint8_t* d_mask, size_t n, float4* d_out,
                           uint32_t* d_count);
constexpr size_t kCompactSmallMax = 32768;          // record sets up to this size are compacted by one workgroup, straight to their destination (mask.hip)
int compact_small_device(ofps_hip_ctx* ctx, const float4* d_in, const uint8_t* d_mask, size_t n, float4* d_out, uint32_t* d_count);
int detect_device(ofps_hip_ctx* ctx, const float4* d_entries, size_t n, int batch, float min_size, size_t subdivide,
                  float target_motion, int* d_result, float2* d_out_field, int* out_dim, const uint32_t* d_n = nullptr);
int farneback_flow_device(ofps_hip_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_cur, int W, int H, int stride, int levels, int winsize,
                          int iters, int poly_n, double poly_sigma, const float2* d_init, float2* d_flow, float4* d_entries,
                          uint64_t prev_id = 0, uint64_t cur_id = 0);     // ids != 0: frames of a stream (FarnebackState::cache)
void farneback_mark_ordered(ofps_hip_ctx* ctx, hipStream_t s);
int farneback_prepare_device(ofps_hip_ctx* ctx, const uint8_t* d_img, int W, int H, int stride, int levels, int winsize, int poly_n, double poly_sigma,
                             uint64_t id, hipStream_t st);          // a stream frame's pyramid + expansion ahead of its pair's flow, on stream st
int farneback_check_params(ofps_hip_ctx* ctx, int W, int H, int levels, int winsize, int poly_n);       // what farneback_flow_device would refuse, without running it
void cluster_gate_context_created(int device);      // almeida.hip: the cluster launches' per-device gate counts the contexts alive on a device
void cluster_gate_context_destroyed(int device);
int almeida_device(ofps_hip_ctx* ctx, const float4* d_entries, size_t n, int batch, float aspect, float fov_y_deg,
                   int use_ransac, size_t num_iters, float inlier_deg, size_t num_samples, uint64_t seed, float4* d_quat);
// `batch` problems of n_max records each whose record counts live in device memory: item j's estimate over its first min(d_n[j], n_max)
// records; every launch is sized from n_max.  One problem may take any solver, a batch the one-workgroup solver (n_max <= 8192) or the
// launch-per-step one.  lsq_min_n: the least-squares fit of fewer records than this is the identity (RANSAC has its own rule: fewer than 3 inliers)
int almeida_device_n(ofps_hip_ctx* ctx, const float4* d_entries, size_t n_max, const uint32_t* d_n, float aspect, float fov_y_deg,
                     int use_ransac, size_t num_iters, float inlier_deg, size_t num_samples, uint64_t seed, float4* d_quat,
                     uint32_t lsq_min_n = 0, int batch = 1);

// sad_gate.hip: hip_sad's contrast gate.  The flags buffer of a frame: [counts][kept count][keep flags]; of a batch of `items` frames:
// [items x nblk counts][items kept counts][items x nblk keep flags], item-major
inline size_t gate_kept_bytes(size_t items) { return (items * sizeof(uint32_t) + 15) & ~size_t(15); }
inline size_t gate_flags_bytes(size_t nblk, size_t items = 1) {
    return ((items * nblk * sizeof(uint32_t) + 15) & ~size_t(15)) + gate_kept_bytes(items) + ((items * nblk + 15) & ~size_t(15));
}
inline uint32_t* gate_counts(char* flags) { return reinterpret_cast<uint32_t*>(flags); }
inline uint32_t* gate_kept(char* flags, size_t nblk, size_t items = 1) {
    return reinterpret_cast<uint32_t*>(flags + ((items * nblk * sizeof(uint32_t) + 15) & ~size_t(15)));
}
inline uint8_t* gate_keep(char* flags, size_t nblk, size_t items = 1) { return reinterpret_cast<uint8_t*>(gate_kept(flags, nblk, items)) + gate_kept_bytes(items); }

// the segmented ordered compaction (compact_items_kernel): item k's records with a non-zero flag -> the head of slot k of d_out, their number ->
// d_counts[k]; every array holds items x n, item-major; one workgroup per item, one launch, on ctx->stream.  d_out may not alias d_in
int compact_items_device(ofps_hip_ctx* ctx, const float4* d_in, const uint8_t* d_flags, size_t n, int items, float4* d_out, uint32_t* d_counts);

// sad_consistency.hip: hip_sad's forward-backward consistency check (include/ofps_hip.h N1c)
constexpr int kSadConsistencyMax = 129;                     // 2 * 64 + 1: above every residual of the largest search range
int sad_consistency_check(ofps_hip_ctx* ctx, int block, int limit, const char* who);        // limit in [1, 129]
// residual and / or keep byte per block from the two directions' integer winners, on stream st; d_keep_in (optional, may be d_out_keep) is ANDed in.
// Every array holds items x nblk, item-major; one launch, no partner block outside its item
int sad_consistency_flags_device(ofps_hip_ctx* ctx, const int* d_fwd_best, const int* d_bwd_best, int W, int H, int block, int limit,
                                 const uint8_t* d_keep_in, uint32_t* d_out_residual, uint8_t* d_out_keep, hipStream_t st, int items = 1);

// sad_median.hip: hip_sad's median test (include/ofps_hip.h N1v)
constexpr int kSadMedianMax = 255;
int sad_median_check(ofps_hip_ctx* ctx, int block, int limit, const char* who);             // limit in [1, 255]
// doubled residual and / or keep byte per block from the integer winners, on stream st; d_keep_in (optional: absent = all ones) is ANDed in
// and may NOT be d_out_keep: a verdict reads its neighbours' incoming flags.  Every array holds items x nblk, item-major; one launch, no
// neighbour outside its item
int sad_median_flags_device(ofps_hip_ctx* ctx, const int* d_best, const uint8_t* d_keep_in, int W, int H, int block, int limit,
                            uint32_t* d_out_residual2, uint8_t* d_out_keep, hipStream_t st, int items = 1);

// sad_intra.hip: hip_sad's intra test and scene-cut rule (include/ofps_hip.h N1i)
constexpr int kSadIntraMax = 255, kSadCutMax = 100;
int sad_intra_check(ofps_hip_ctx* ctx, int block, int ratio, int cut, const char* who);     // ratio in [1, 255], cut in [0, 100]
// A(k) of every block of `items` frames `pitch` bytes apart, u32 per block, item-major, on stream st; one launch
int block_activity_device(ofps_hip_ctx* ctx, const uint8_t* d_luma, size_t pitch, int items, int W, int H, int stride, int block, uint32_t* d_out,
                          hipStream_t st);
// keep byte per block = incoming flag (d_keep_in: optional, absent = all ones, may be d_out_keep) AND NOT intra, from the integer winners' SADs
// and the activities; d_counts (optional): [candidates, intra candidates] per item, zeroed here unless the caller has (zero_counts).  Every
// array holds items x nblk, item-major
int sad_intra_flags_device(ofps_hip_ctx* ctx, const int* d_best, const uint32_t* d_activity, const uint8_t* d_keep_in, int W, int H, int block,
                           int ratio, uint8_t* d_out_keep, uint32_t* d_counts, hipStream_t st, int items = 1, bool zero_counts = true);
// cut > 0: the flags of every item whose counters say 100 * intra >= cut * candidates are cleared; one launch.  cut == 0: nothing
int sad_cut_device(ofps_hip_ctx* ctx, const uint32_t* d_counts, size_t nblk, int cut, uint8_t* d_flags, hipStream_t st, int items = 1);

// sad_split.hip: hip_sad's split step (include/ofps_hip.h N1s)
constexpr int kSadSplitMax = 4080;                          // sixteenths: 255 grey levels per pixel
int sad_split_check(ofps_hip_ctx* ctx, int block, int reach, int threshold, const char* who);       // block even in [8, 64], reach + 3 <= 127, threshold in [1, 4080]
inline size_t sad_split_bytes(size_t nblk) { return nblk * (4 * sizeof(float4) + 12 * sizeof(int) + 4 + 1); }
// One pair of `f` (the frames the integer search read), on ctx->stream, one launch: per block with a non-zero keep flag (d_keep: optional,
// absent = all ones) the four sub-blocks' winners -> d_sub_best (12 i32 per block), the verdict -> d_split (u8 per block), and, unless null,
// the raw slots 4 * blk + s -> d_raw (records) and d_slot_flags (u8): an unsplit kept block fills slot 0 with its N1 record, a split one all
// four, a block that is not kept none; slots whose flag is 0 hold zeros
int sad_split_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int block, int reach, int threshold, const int* d_best, const uint8_t* d_keep,
                     int* d_sub_best, uint8_t* d_split, float4* d_raw, uint8_t* d_slot_flags);

// sad_gate.hip: the filtered search of `pairs` pairs -- search [+ backward search] -> keep flags -> ordered compaction -> count on the device --
// in the steps every caller takes: plan, reserve, search, [contrast_flags,] finish.  sad_flow_filtered_device runs them all on ctx->stream; the
// fused per-frame path (pipeline.hip) makes the contrast flags and the activities on its auxiliary stream, beside the search.  Every per-block array holds pairs x nblk, item-major,
// and every step is one launch whatever `pairs`.  With gate == 0, limit == 0 and median == 0 search() is the plain search into d_out and no
// other step reserves or enqueues anything; the same holds for intra == 0 (cut alone does nothing).
// SadCriteria: the six settings of a filtered search as one value, every one 0 = off.  The context's are of(ctx->opt); an explicit-argument
// entry point writes out the ones it takes and leaves the rest 0
struct SadCriteria {
    int gate = 0, limit = 0, median = 0; // the contrast gate's min_pixels, the consistency check's limit, the median test's limit
    int intra = 0, cut = 0;              // the intra test's ratio in sixteenths; the scene-cut rule's percentage, no effect while intra == 0
    int split = 0;                       // the split step's threshold in sixteenths (N1s); one pair only
    static SadCriteria of(const ofps_hip_ctx::Options& o) { return {o.sad_gate, o.sad_consistency, o.sad_median, o.sad_intra, o.sad_cut, o.sad_split}; }
    SadCriteria without_split() const { return {gate, limit, median, intra, cut, 0}; }      // the batched forms take none
    bool criteria() const { return gate > 0 || limit > 0 || median > 0 || intra > 0; }         // something drops blocks
    bool on() const { return criteria() || split > 0; }   // the record count is variable and lives on the device
    bool winners() const { return limit > 0 || median > 0 || intra > 0 || split > 0; }       // all four read the forward search's INTEGER winners, whatever the motion scale
};
struct SadFilter : SadCriteria {
    SadFrames fr;                        // plan() and reserve() read the geometry alone: the bases may be filled in behind them (pipeline.hip)
    int pairs, block, range;
    bool want_triples;                   // the caller takes the kept records' (dx, dy, SAD) triples as well
    static SadFilter make(const SadFrames& fr, int pairs, int block, int range, const SadCriteria& c, bool want_triples) {     // the one way to make one
        return {c, fr, pairs, block, range, want_triples};
    }
    size_t nblk = 0;                     // per pair
    float4* d_raw = nullptr;             // S_GATE_RAW: the search's one record per block, in front of the compaction
    char* d_flags = nullptr;             // S_GATE_FLAGS, this ticket's block: [counts][kept count][keep flags]
    int *d_fwd = nullptr, *d_bwd = nullptr;      // S_CONS_FWD (limit > 0 or median > 0), S_CONS_BWD (limit > 0): the two directions' integer winners
    float4* d_bwd_ent = nullptr;         // S_CONS_BWD_ENT
    int* d_triples = nullptr;            // the triples that belong to d_raw: S_GATE_BEST, or d_fwd itself (integer winners kept, motion scale 1)
    uint8_t* d_med_keep = nullptr;       // S_MED_KEEP, this ticket's block: the median test's outgoing flags (median > 0)
    uint32_t *d_act = nullptr, *d_intra_counts = nullptr;       // S_INTRA, this ticket's block: the current frames' activities and the items' two counters (intra > 0)
    int* d_sub_best = nullptr;           // S_SPLIT (split > 0): the raw slots' records (d_split_raw), the sub-blocks' triples, slot flags and split flags
    float4* d_split_raw = nullptr;
    uint8_t *d_slot_flags = nullptr, *d_split = nullptr;
    size_t total() const { return (size_t)pairs * nblk; }
    size_t capacity() const { return split > 0 ? 4 * nblk : nblk; }       // records d_out must hold, per pair
    uint32_t* kept() const { return on() ? gate_kept(d_flags, nblk, pairs) : nullptr; }
    uint8_t* keep() const { return gate_keep(d_flags, nblk, pairs); }       // the incoming flags: contrast gate AND NOT intra AND consistency check
    int plan(ofps_hip_ctx* ctx, const char* who);         // validation, every text led by `who`; nothing is reserved or enqueued
    // the scratch slots; S_GATE_FLAGS / S_MED_KEEP hold `tickets` blocks, this plan's is number `tix`.  May reallocate: behind whatever drains the slots' readers
    int reserve(ofps_hip_ctx* ctx, int tix = 0, int tickets = 1);
    int search(ofps_hip_ctx* ctx, float4* d_out);         // on ctx->stream; d_out: the unfiltered search's records.  The backward search reads fr.swapped()
    // what depends on the current frames alone, on stream st: gate > 0: contrast counts and keep flags; intra > 0: activities, and the counters zeroed
    int contrast_flags(ofps_hip_ctx* ctx, hipStream_t st);
    // on ctx->stream behind search and contrast_flags: [intra flags and counters, the gate's ANDed in in place ->] [consistency flags, those
    // ANDed in in place ->] [median flags read from those, into d_med_keep ->] [the cut rule's veto on the final flags ->] [the split step: raw
    // slots and slot flags of the kept blocks ->] kept records [and triples] in raster order -> count.  d_out and d_out_best hold pairs slots of nblk, item k's kept ones
    // lead slot k; d_count holds pairs counts.  split > 0: d_out holds capacity() records, d_out_best stays the parents' nblk triples
    int finish(ofps_hip_ctx* ctx, float4* d_out, int* d_out_best, uint32_t* d_count);               // d_out may not alias d_raw
    int finish_split(ofps_hip_ctx* ctx, const uint8_t* flags, float4* d_out, int* d_out_best, uint32_t* d_count);     // finish()'s last step with split > 0
};
// the five steps on ctx->stream, the launch count independent of `pairs`; `who` leads every error text, tix / tickets: SadFilter::reserve
int sad_flow_filtered_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int block, int range, const SadCriteria& c, float4* d_out,
                             int* d_out_best, uint32_t* d_counts, const char* who, int tix = 0, int tickets = 1);

// compensate.hip: out = (pos, motion - camera.delta(pos, to_homogeneous(inverse(quat[item])))) per record, batch items of n records; the quaternions
// are read on the device.  d_n (optional): the record counts in device memory, one per item, n the capacity.  d_out may equal d_entries.
// d_quat_echo (optional): the quaternions are stored there as well (a ticket's result block)
int compensate_device(ofps_hip_ctx* ctx, const float4* d_entries, size_t n, int batch, const uint32_t* d_n, float aspect, float fov_y_deg,
                      const float4* d_quat, float4* d_out, float4* d_quat_echo);

// tail.hip: estimator -> [compensation ->] detector over `batch` items of n records, the one tail of every fused entry point.
// TailSide: the detector's chain runs on `stream` beside the estimator -- forked on `fork_on` (recorded on the compute stream here unless it
// `recorded` a point there already), joined through `join`.  Only when both stages run and nothing is compensated.
struct TailSide { hipStream_t stream; hipEvent_t fork_on; bool recorded; hipEvent_t join; };
// d_n (optional): the record counts live in device memory, d_n[j] item j's, n is the capacity and the stride of every item, and the
// estimator takes its device-count form (lsq_min_n: almeida_device_n).  seed0: item 0's seed, item j gets seed0 + j.  may_compensate: the context's detect-compensation mode
// counts here.  d_result [batch][4], d_quat [batch], d_field: device memory or a ticket's device-addressable block.  -> *out_dim (optional)
// isl (optional; the ticket's, with K = the context's max_islands at this push, 0 = off): behind the detector, on its stream, the islands of
// the field it read -> the ticket's page-locked blocks, items isl->first .. isl->first + batch - 1 (detect.hip).  Nothing is enqueued with K == 0
int frame_tail_device(ofps_hip_ctx* ctx, const float4* d_rec, size_t n, int batch, const uint32_t* d_n, uint32_t lsq_min_n,
                      const ofps_hip_frame_params* prm, uint64_t seed0, bool may_compensate, int* d_result, float4* d_quat, float2* d_field,
                      const TailSide* side, int* out_dim, IslandsTicket* isl = nullptr);
// detect.hip, A5i.  A push arms its ticket: K = the context's max_islands when the detector runs and its grid is valid, else 0; `items` frames
// form (A5t): the stream form that pushes, -1 = a ticket without tracks; restart: the ticket holds the first frame of a stream
void islands_ticket_arm(ofps_hip_ctx* ctx, IslandsTicket* isl, const ofps_hip_frame_params* prm, int items, int form = -1, bool restart = false);
// densify as the detector does -> the islands of `batch` items into blocks `stride` bytes apart, each led by its A5i block
int detect_islands_blocks_device(ofps_hip_ctx* ctx, const float4* d_entries, size_t n, int batch, float min_size, size_t subdivide, float target_motion,
                                 int K, char* d_blocks, size_t stride);
// detect_tracks.hip, A5t.  The arm step's part: T, reach and gap of the context at this push; T == 0 or a restart forget the form's state
void tracks_ticket_arm(ofps_hip_ctx* ctx, IslandsTicket* isl, int form, bool restart);
// `batch` steps in item order through the form's state, one launch on ctx->stream behind the islands kernel that filled the blocks
int tracks_ticket_device(ofps_hip_ctx* ctx, IslandsTicket* isl, int batch, int dim, char* d_blocks, size_t stride);
// the islands of the `batch` fields detect_device has just left in S_FIELD, on ctx->stream -> isl->pinned, items isl->first ..
int islands_ticket_device(ofps_hip_ctx* ctx, int batch, int dim, float min_size, float target_motion, IslandsTicket* isl);
// a fused wait: the collected ticket's blocks -> the context's own host memory (what ofps_hip_frame_islands answers from)
int islands_collect(ofps_hip_ctx* ctx, const IslandsTicket& isl);

// ---- transfers (transfer.hip)
bool device_address_of(const void* host_ptr, void** dev_ptr);        // the device address of page-locked host memory, or false for pageable memory
// device -> host: by a copy KERNEL when the destination is page-locked (device-addressable), by hipMemcpyAsync otherwise.  bytes % 4 == 0.
int read_back_device(ofps_hip_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes, hipStream_t s);
int copy_words_device(ofps_hip_ctx* ctx, void* dst, const void* src, size_t words, unsigned blocks, hipStream_t s);     // that kernel, `blocks` workgroups
// dense bytes, host -> device on stream s; by_kernel: through the upload kernel when the source is page-locked (else the DMA engine)
int upload_dense_device(ofps_hip_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s, bool by_kernel);
// a page-locked block that kernels write and the host reads after an event, of at least `bytes`; grows, never shrinks
int host_block_reserve(ofps_hip_ctx* ctx, void** p, size_t* cap, size_t bytes);

// lk.hip: the iterative LK flow of a pair of device frames (d_flow and / or d_entries; d_init: the initial flow or null)
int lk_flow_device(ofps_hip_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_cur, int W, int H, int stride, int levels, int radius, int iters,
                   float2* d_flow, float4* d_entries, const float2* d_init = nullptr);

// the batched read-ahead push with the previous frame supplied by the caller (pipeline.hip; multi.hip deals batches to workers)
int push_frames_impl(ofps_hip_ctx* ctx, const uint8_t* frames, int n, int W, int H, int stride, size_t frame_pitch,
                     const ofps_hip_frame_params* prm, float* out_entries, int* ticket, int halo_mode, const uint8_t* halo, int halo_stride);

// rows of `width` bytes, host -> device; one linear copy when both sides are dense (the 2-D path is slower)
inline hipError_t upload_rows(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                              hipStream_t stream) {
    if (dpitch == width && spitch == width) return hipMemcpyAsync(dst, src, width * height, hipMemcpyHostToDevice, stream);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice, stream);
}

#define OFPS_HIP_TRY(ctx, expr)                                          \
    do {                                                                 \
        hipError_t _e = (expr);                                          \
        if (_e != hipSuccess) return ofps::check_hip((ctx), _e, #expr);  \
    } while (0)

#define OFPS_REQUIRE(ctx, cond, ...)                                              \
    do {                                                                          \
        if (!(cond)) return ofps::set_error((ctx), OFPS_HIP_EINVAL, __VA_ARGS__);  \
    } while (0)

}  // namespace ofps
