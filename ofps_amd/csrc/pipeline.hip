// pipeline.hip -- the fused per-frame path (BASELINE configs[4]: live stream, SAD decoder + block-motion
// detector + Almeida estimator per frame).  One ticket per arriving frame reproduces one iteration of the
// reference's worker loops -- decoder.process_frame -> detector.detect_motion
// (ofps-suite/src/app/detection.rs:111-148) and -> estimator.estimate
// (ofps-suite/src/app/tracking/worker.rs:328-361) -- without the motion vectors leaving the device:
//   H2D of the new luma frame into the free slot of a three-slot device ring, on a COPY stream
//   -> (compute stream, after the copy's event) SAD search between the two newest slots
//   -> detect + estimate on the device-resident vectors
//   -> one small D2H (result record, quaternion; vectors / field only when the caller asks for them).
// ofps_hip_push_frame_async returns once that is enqueued; ofps_hip_frame_wait collects a ticket.  With two tickets in
// flight the upload of frame k+1 overlaps the search of pair (k-1, k) -- what the reference's read-ahead decoder thread
// does on the host (ofps-suite/src/app/tracking/worker.rs:165-226).  ofps_hip_push_frame = push_async + wait.
#include "common.hpp"

#include <chrono>

namespace {
using ofps::PipeStream;
using ofps::TailRecord;
struct PipeOut {                 // a ticket's result block: page-locked, and in device scratch at the head of its kPipeOutBytes
    TailRecord r;
    uint32_t kept[4];            // contrast gate, consistency check, median test or intra test on: the kept record count (sad_gate.hip); not read back, not looked at, with all off
};
constexpr size_t kPipeOutPlain = offsetof(PipeOut, kept);       // what a ticket without the gate reads back
constexpr size_t kPipeField = 4096;                             // the detector's field in the device copy, behind the block
constexpr size_t kPipeOutBytes = kPipeField + ofps::kMaxFieldBytes;
static_assert(offsetof(PipeOut, r) == 0 && kPipeOutPlain == sizeof(TailRecord) && sizeof(PipeOut) == 48 && sizeof(PipeOut) <= kPipeField, "PipeOut layout");
constexpr int kSlots = PipeStream::kSlots, kTickets = PipeStream::kTickets;

#ifndef OFPS_HIP_UPLOAD_KERNEL_SINGLE
#define OFPS_HIP_UPLOAD_KERNEL_SINGLE 0          // A/B (tools/upload_ab.sh): the single-frame form through the upload kernel as well (transfer.hip)
#endif

int pipe_setup(ofps_hip_ctx* ctx) {
    if (ctx->pipe.copy_stream) return OFPS_HIP_OK;
    OFPS_HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->pipe.copy_stream, hipStreamNonBlocking));
    OFPS_HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->pipe.aux_stream, hipStreamNonBlocking));
    OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pipe.fork, hipEventDisableTiming));
    OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pipe.join, hipEventDisableTiming));
    for (int k = 0; k < kSlots; ++k) {
        OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pipe.uploaded[k], hipEventDisableTiming));
        OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pipe.slot_read[k], hipEventDisableTiming));
    }
    for (auto& t : ctx->pipe.ring.entry) {
        OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
        // kernels store the result record straight into this block: fine-grained, like every result block (transfer.hip: host_block_reserve)
        OFPS_HIP_TRY(ctx, hipHostMalloc(&t.pinned, sizeof(PipeOut), OFPS_HIP_HOST_BLOCK_FLAGS));
    }
    return OFPS_HIP_OK;
}

// Waits for every ticket still in flight and forgets the stream position (geometry change / reset).
int pipe_drain(ofps_hip_ctx* ctx) {
    OFPS_HIP_TRY(ctx, ctx->pipe.ring.drain());
    if (ctx->pipe.copy_stream) OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->pipe.copy_stream));
    ctx->pipe.frames = 0;
    for (bool& v : ctx->pipe.slot_read_valid) v = false;
    return OFPS_HIP_OK;
}

// Enqueues the H2D of one luma frame as frame number ctx->pipe.frames (slot = number % 3).  With another ticket in
// flight the copy goes to the copy stream, so that it overlaps that ticket's search; a lone frame is copied on the
// compute stream itself (no cross-stream events on the latency path of the synchronous call: 0.10 vs 0.17 ms per
// 1080p frame).
int pipe_upload(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride, bool overlap, uint8_t** slots_out,
                size_t* pitch_out, int* dstride_out) {
    int rc = pipe_setup(ctx);
    if (rc != OFPS_HIP_OK) return rc;
    const int dstride = ofps::padded_stride(W);
    const size_t pitch = (size_t)dstride * H;
    if (W != ctx->pipe.w || H != ctx->pipe.h) {            // geometry change restarts the stream (decoder.rs:66-72)
        rc = pipe_drain(ctx);
        if (rc != OFPS_HIP_OK) return rc;
        ctx->pipe.w = W; ctx->pipe.h = H;
    }
    auto* slots = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_PIPE_FRAMES, kSlots * pitch));
    if (!slots) return OFPS_HIP_ENOMEM;
    const int slot = (int)(ctx->pipe.frames % kSlots);
    hipStream_t up = overlap ? ctx->pipe.copy_stream : ctx->stream;
    // the slot's previous tenant (frame number - 3) may still be read by the search of ticket number - 2
    if (overlap && ctx->pipe.slot_read_valid[slot]) OFPS_HIP_TRY(ctx, hipStreamWaitEvent(up, ctx->pipe.slot_read[slot], 0));
    if (dstride == W && stride == W) {
        rc = ofps::upload_dense_device(ctx, slots + (size_t)slot * pitch, luma, pitch, up, OFPS_HIP_UPLOAD_KERNEL_SINGLE != 0);
        if (rc != OFPS_HIP_OK) return rc;
    } else {
        OFPS_HIP_TRY(ctx, ofps::upload_rows(slots + (size_t)slot * pitch, dstride, luma, stride, W, H, up));
    }
    if (overlap) OFPS_HIP_TRY(ctx, hipEventRecord(ctx->pipe.uploaded[slot], up));
    ctx->pipe.uploaded_on_compute[slot] = !overlap;       // ... in which case the compute stream never has to wait for it
    ctx->pipe.frames += 1;
    *slots_out = slots; *pitch_out = pitch; *dstride_out = dstride;
    return OFPS_HIP_OK;
}

// One ofps_hip_push_frame_async call, step by step.  Every step enqueues or returns an error; none touches the ring (commit does, last).
struct Push {
    ofps_hip_ctx* ctx;
    const ofps_hip_frame_params* prm;
    ofps::SadFilter f;                   // contrast gate, consistency check, median test, intra test and cut rule as the context has them at this push; all 0: the plain search.
                                         // Made with the geometry alone -- claim() refuses before anything is uploaded -- upload() fills in the pair's frames
    PipeStream::Ticket* t = nullptr;
    int tix = 0;
    long frame_no = 0;                   // the frame this push uploads
    int cur_slot = 0, prev_slot = 0;
    bool cur_by_event = false;           // this frame's upload ran on the copy stream and has an event of its own
    float4* d_ent = nullptr;             // this ticket's records: what the caller gets
    char* d_out = nullptr;               // ... and its kPipeOutBytes
    PipeOut* out = nullptr;              // where the tail stores result and quaternion: the ticket's page-locked block, or d_out
    int dim = 0;

    int claim() {
        const long tno = ctx->pipe.ring.next;
        t = &ctx->pipe.ring.at(tno);
        tix = (int)(tno % kTickets);
        OFPS_REQUIRE(ctx, !t->pending, "push_frame_async: ticket %ld has not been collected (at most %d frames in flight)", tno - kTickets, kTickets);
        ofps::islands_ticket_arm(ctx, &t->isl, prm, 1, ofps::TRK_PIPE);     // A5i, A5t: the ticket follows the context's max_islands and max_tracks at this push
        return f.plan(ctx, "push_frame_async");
    }

    // The H2D of the frame, and the compute stream behind the uploads of both frames of the pair: the previous frame's was waited for by the
    // previous ticket (or by the stage_frame that made it), this frame's by its event.  Uploads made on the compute stream itself are ordered
    // by the stream; one wait per upload is enough
    int upload(const uint8_t* luma, int stride) {
        PipeStream& ps = ctx->pipe;
        uint8_t* slots; size_t pitch; int dstride;
        const int rc = pipe_upload(ctx, luma, f.fr.W, f.fr.H, stride, /*overlap=*/ps.ring.other_pending(), &slots, &pitch, &dstride);
        if (rc != OFPS_HIP_OK) return rc;
        frame_no = ps.frames - 1;
        if (frame_no == 0) ctx->trk[ofps::TRK_PIPE].live = false;      // A5t: a stream's first frame forgets the tracks of the one before
        cur_slot = (int)(frame_no % kSlots); prev_slot = (int)((frame_no + kSlots - 1) % kSlots);
        f.fr.cur_base = slots + (size_t)cur_slot * pitch; f.fr.prev_base = slots + (size_t)prev_slot * pitch;
        cur_by_event = !ps.uploaded_on_compute[cur_slot];
        for (int slot : {prev_slot, cur_slot}) {
            if (ps.uploaded_on_compute[slot] || (frame_no == 0 && slot == prev_slot)) continue;
            OFPS_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ps.uploaded[slot], 0));
            ps.uploaded_on_compute[slot] = true;
        }
        return OFPS_HIP_OK;
    }

    // The search of pair (prev, cur) -> the [kept] records in d_ent [and their count in device memory, f.kept()].  Gate or intra test on: the
    // contrast flags and the activities depend on the new frame only -- they are made on the auxiliary stream, forked on that frame's upload,
    // beside the search (never in front
    // of it on the compute stream).  Check on: both searches read prev_slot, so its event is recorded behind both.
    int search() {
        PipeStream& ps = ctx->pipe;
        hipStream_t s = ctx->stream;
        d_ent = static_cast<float4*>(ofps::scratch(ctx, ofps::S_PIPE_ENTRIES, kTickets * f.capacity() * sizeof(float4)));
        d_out = static_cast<char*>(ofps::scratch(ctx, ofps::S_PIPE_OUT, kTickets * kPipeOutBytes));
        if (!d_ent || !d_out) return OFPS_HIP_ENOMEM;
        d_ent += (size_t)tix * f.capacity(); d_out += (size_t)tix * kPipeOutBytes;
        int rc = f.reserve(ctx, tix, kTickets);          // S_GATE_FLAGS per ticket: the detector may still read ticket k's count while ticket k + 1 compacts
        if (rc != OFPS_HIP_OK) return rc;
        if (f.gate > 0 || f.intra > 0) {
            if (!ps.gate_done) OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&ps.gate_done, hipEventDisableTiming));
            // fork on the upload: its own event when it ran on the copy stream (the flags are then made beside the previous ticket's tail as
            // well), else the compute stream's position, which is right behind the upload
            if (!cur_by_event) OFPS_HIP_TRY(ctx, hipEventRecord(ps.fork, s));
            OFPS_HIP_TRY(ctx, hipStreamWaitEvent(ps.aux_stream, cur_by_event ? ps.uploaded[cur_slot] : ps.fork, 0));
            rc = f.contrast_flags(ctx, ps.aux_stream);
            if (rc != OFPS_HIP_OK) return rc;
            OFPS_HIP_TRY(ctx, hipEventRecord(ps.gate_done, ps.aux_stream));
        }
        rc = f.search(ctx, d_ent);
        if (rc != OFPS_HIP_OK) return rc;
        // the older slot may be overwritten once this search is through; the same event forks the unfiltered tail's detector
        // (one barrier packet between the search and the estimator instead of two)
        OFPS_HIP_TRY(ctx, hipEventRecord(ps.slot_read[prev_slot], s));
        ps.slot_read_valid[prev_slot] = true;
        if (f.gate > 0 || f.intra > 0) OFPS_HIP_TRY(ctx, hipStreamWaitEvent(s, ps.gate_done, 0));
        return f.finish(ctx, d_ent, nullptr, f.kept());
    }

    // The 32 bytes the caller waits for (island result, quaternion) are written by the detector's and the estimator's last kernels STRAIGHT
    // into the ticket's page-locked block -- it is device-addressable, each is one thread's store at the end of a kernel -- instead of into
    // device scratch and from there by a copy launch behind the join: that launch and the gap in front of it were 14 us of a 170 us frame
    // (rocprofv3 kernel trace, tools/trace_stream.sh).  Filtered: the tail's device-count forms, fewer than 3 kept records -> identity, and
    // the detector's stream starts behind the compaction, not behind the search.
    int tail() {
        PipeStream& ps = ctx->pipe;
        void* mapped = nullptr;
        out = ofps::device_address_of(t->pinned, &mapped) ? static_cast<PipeOut*>(mapped) : reinterpret_cast<PipeOut*>(d_out);
        const ofps::TailSide side{ps.aux_stream, f.on() ? ps.fork : ps.slot_read[prev_slot], /*recorded=*/!f.on(), ps.join};
        return ofps::frame_tail_device(ctx, d_ent, f.capacity(), 1, f.kept(), /*lsq_min_n=*/3, prm, prm->seed, /*may_compensate=*/true, out->r.result,
                                       reinterpret_cast<float4*>(out->r.quat), reinterpret_cast<float2*>(d_out + kPipeField), &side, &dim, &t->isl);
    }

    int read_back(float* out_entries, float* out_field) {
        hipStream_t s = ctx->stream;
        int rc = OFPS_HIP_OK;
        if ((prm->run_detector || prm->run_estimator) && out == reinterpret_cast<PipeOut*>(d_out)) rc = ofps::read_back_device(ctx, t->pinned, d_out, kPipeOutPlain, s);
        if (rc == OFPS_HIP_OK && f.on())                             // the kept count travels in the ticket's page-locked block
            rc = ofps::read_back_device(ctx, static_cast<PipeOut*>(t->pinned)->kept, f.kept(), sizeof(uint32_t), s);
        if (rc == OFPS_HIP_OK && out_entries && f.nblk) rc = ofps::read_back_device(ctx, out_entries, d_ent, f.capacity() * sizeof(float4), s);
        if (rc == OFPS_HIP_OK && out_field && prm->run_detector)
            rc = ofps::read_back_device(ctx, out_field, d_out + kPipeField, (size_t)dim * dim * sizeof(float2), s);
        return rc;
    }

    int commit(int* ticket) {
        OFPS_HIP_TRY(ctx, hipEventRecord(t->done, ctx->stream));
        t->have_vectors = frame_no > 0; t->n_vectors = frame_no > 0 ? f.capacity() : 0; t->gated = frame_no > 0 && f.on();
        t->run_detector = prm->run_detector; t->run_estimator = prm->run_estimator;
        *ticket = ctx->pipe.ring.commit();
        return OFPS_HIP_OK;
    }
};
}  // namespace

extern "C" {

int ofps_hip_reset_frames(ofps_hip_ctx* ctx) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    OFPS_HIP_TRY(ctx, ctx->batch.ring.drain());
    ctx->batch.last_frame = nullptr;
    ctx->batch.klt_pred.valid = false;
    ctx->trk[ofps::TRK_PIPE].live = false; ctx->trk[ofps::TRK_BATCH].live = false;       // A5t: both forms' tracks start anew
    return pipe_drain(ctx);
}

int ofps_hip_stage_frame(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, luma, "stage_frame: null pointer");
    OFPS_REQUIRE(ctx, W > 0 && H > 0 && stride >= W, "stage_frame: bad geometry W=%d H=%d stride=%d", W, H, stride);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint8_t* slots; size_t pitch; int dstride;
    int rc = pipe_upload(ctx, luma, W, H, stride, /*overlap=*/false, &slots, &pitch, &dstride);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));             // the caller may reuse `luma` right away
    return OFPS_HIP_OK;
}

int ofps_hip_push_frame_async(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride,
                              const ofps_hip_frame_params* prm, float* out_entries, float* out_field, int* ticket) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, luma && prm && ticket, "push_frame_async: null pointer");
    OFPS_REQUIRE(ctx, W > 0 && H > 0 && stride >= W, "push_frame_async: bad geometry W=%d H=%d stride=%d", W, H, stride);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = pipe_setup(ctx);
    if (rc != OFPS_HIP_OK) return rc;
    Push p{ctx, prm, ofps::SadFilter::make({nullptr, nullptr, 0, 0, W, H, ofps::padded_stride(W)}, 1, prm->block, prm->range, ofps::SadCriteria::of(ctx->opt),
                                           /*want_triples=*/false)};
    rc = p.claim();                                     // refused before anything is uploaded
    if (rc == OFPS_HIP_OK) rc = p.upload(luma, stride);
    if (rc == OFPS_HIP_OK && p.frame_no > 0) {          // (the first frame of a stream: Ok(false), no vectors yet)
        rc = p.search();
        if (rc == OFPS_HIP_OK) rc = p.tail();
        if (rc == OFPS_HIP_OK) rc = p.read_back(out_entries, out_field);
    }
    return rc == OFPS_HIP_OK ? p.commit(ticket) : rc;
}

int ofps_hip_frame_wait(ofps_hip_ctx* ctx, int ticket, ofps_hip_frame_result* out) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, out, "frame_wait: null pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto* t = ctx->pipe.ring.claim(ctx, ticket, "frame_wait", "was already");
    if (!t) return OFPS_HIP_EINVAL;
    // a per-frame result is tens of microseconds away: poll first (hipEventSynchronize may put the thread to sleep, and a
    // wake-up costs more than the whole frame -- 0.23 vs 0.06 ms per frame measured inside a process that initialised
    // torch's runtime), then block
    {
        const auto t0 = std::chrono::steady_clock::now();
        hipError_t q;
        while ((q = hipEventQuery(t->done)) == hipErrorNotReady) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(OFPS_HIP_FRAME_WAIT_SPIN_US)) break;
        }
        if (q != hipSuccess) {
            if (q != hipErrorNotReady) OFPS_HIP_TRY(ctx, q);
            (void)hipGetLastError();
            OFPS_HIP_TRY(ctx, hipEventSynchronize(t->done));
        }
    }
    t->pending = false;
    const auto* host = static_cast<const PipeOut*>(t->pinned);
    const bool has = t->have_vectors != 0;
    ofps::fill_frame_result(out, t->have_vectors, has && t->gated && host->kept[0] < t->n_vectors ? host->kept[0] : t->n_vectors,
                            has && t->run_detector ? host->r.result : nullptr, has && t->run_estimator ? host->r.quat : nullptr);
    return ofps::islands_collect(ctx, t->isl);
}

}  // extern "C"

// ---- batched read-ahead form: n consecutive frames of the stream per ticket.  What a decoder that runs n frames ahead
// (ofps-suite/src/app/tracking/worker.rs:165-226 decodes into a buffer on its own thread) hands over in one go: ONE H2D of the
// n frames (contiguous at frame_pitch), one search launch over the batch's pairs, one detector chain and one estimator
// launch over the batch, one read-back -- a handful of HIP calls per BATCH instead of ~9 per frame, which is what kept
// the single-frame loop 20 % under the PCIe ceiling.  Frame j of the batch is pair (previous frame of the stream, frame
// j); the previous frame of frame 0 is the last frame of the previous batch, kept in slot 0 of the other batch buffer.
// The push is BatchPush's steps in the order claim -> reserve -> upload -> [decode -> tail -> read_back] -> commit, as the per-frame
// form's is Push's; the ticket's result block is a BatchBlock (common.hpp).
namespace ofps {
namespace {
// One push_frames_impl call, step by step.  Every step enqueues or returns an error; none touches the ring (commit does, last), and none
// but commit writes the ticket, with two exceptions where they always were: prev_copied_valid in front of the copy, the islands arming at
// the end of upload(), in front of the tail that takes it.  claim() refuses before anything is uploaded.  The settings are the context's at this push:
//   klt      -- the batch decoder switch (include/ofps_hip.h N3b): hip_klt in place of the search; the slot count takes the block count's
//               place in every size, the kept counts travel where the batch filter's do
//   filtered -- the batch filter switch (N1b) with a criterion on: the filtered batched search and the tail's per-item device counts
//   chained  -- N3pb, both prediction settings on: the ticket's items are chained, item 0 behind the last item of the ticket before.  That
//               item's raw slots wait in one half of S_KLT_BATCH_PRED (d_pred_in), this ticket's last item writes the other (d_pred_out).
//               Any other ticket -- a setting off, the search, a multi-device worker's (halo_mode 1: a worker sees every n-th batch, its first
//               item has no predecessor there) -- leaves no slots behind: its successor starts from zero
// With all three off nothing differs from the plain batched search.
struct BatchPush {
    ofps_hip_ctx* ctx;
    const ofps_hip_frame_params* prm;
    const uint8_t* frames; int n, W, H, stride; size_t frame_pitch;
    int halo_mode; const uint8_t* halo; int halo_stride;
    static constexpr int kTickets = BatchStream::kTickets;
    int dstride = 0; size_t pitch = 0;   // the frames on the device
    long tno = 0; BatchStream::Ticket* t = nullptr; int tix = 0;
    bool klt = false, filtered = false, chained = false;
    size_t nblk = 0;                     // records per frame: blocks, or hip_klt's slots
    SadCriteria crit;                    // filtered: what the search follows (no split: the batched forms take none)
    BatchBlock blk{0, false};
    const int* d_pred_in = nullptr; int* d_pred_out = nullptr; int pred_half = 0;
    uint8_t* buf = nullptr;              // this ticket's batch buffer: [slot 0 = previous frame][n frames]
    float4* d_ent = nullptr; char* d_out = nullptr;      // this ticket's records and its block
    bool has_prev = false;
    int first = 0, pairs = 0;            // pairs (slot j, slot j + 1), j = first .. n - 1: the stream's very first frame has no pair
    float4* ent0() const { return d_ent + (size_t)first * nblk; }
    uint32_t* d_cnt() const { return blk.counted ? blk.kept(d_out) + first : nullptr; }     // item j's count is word j behind the quaternions

    int claim() {
        tno = ctx->batch.ring.next;
        t = &ctx->batch.ring.at(tno);
        OFPS_REQUIRE(ctx, !t->pending, "push_frames_async: ticket %ld has not been collected (at most %d batches in flight)",
                     tno - kTickets, kTickets);
        if (!t->done) {
            OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&t->done, hipEventDisableTiming));
            OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&t->uploaded, hipEventDisableTiming));
            OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&t->prev_copied, hipEventDisableTiming));
        }
        if (W != ctx->batch.w || H != ctx->batch.h) {              // geometry change restarts the stream
            OFPS_HIP_TRY(ctx, ctx->batch.ring.drain());
            ctx->batch.w = W; ctx->batch.h = H; ctx->batch.last_frame = nullptr;
            ctx->batch.klt_pred.valid = false;
        }
        dstride = padded_stride(W);
        pitch = (size_t)dstride * H;
        tix = (int)(tno % kTickets);
        const auto& o = ctx->opt;
        klt = o.batch_decoder == OFPS_HIP_BATCH_DECODER_KLT;
        if (klt) {                                                   // a frame the decoder refuses is refused here
            const int rc = klt_check_call(ctx, W, H, dstride, o.klt_levels, o.klt_radius, o.klt_iters, "push_frames_async");
            if (rc != OFPS_HIP_OK) return rc;
            OFPS_REQUIRE(ctx, (unsigned long long)n * ofps_hip_klt_slot_count(W, H, o.klt_cell) < (1ull << 31), "push_frames_async: %d frames of %zu slots", n,
                         ofps_hip_klt_slot_count(W, H, o.klt_cell));
        }
        nblk = klt ? ofps_hip_klt_slot_count(W, H, o.klt_cell) : ofps_hip_sad_block_count(W, H, prm->block);
        BatchStream::KltPred& kp = ctx->batch.klt_pred;
        chained = klt && !halo_mode && o.klt_prediction && o.klt_batch_prediction;
        if (chained) {
            const size_t half = (nblk * 6 * sizeof(int) + 255) & ~(size_t)255;
            auto* d_pred = static_cast<char*>(scratch(ctx, S_KLT_BATCH_PRED, 2 * half));
            if (!d_pred) return OFPS_HIP_ENOMEM;
            if (kp.valid && ctx->batch.last_frame && kp.w == W && kp.h == H && kp.cell == o.klt_cell && kp.gen == ctx->scratch[S_KLT_BATCH_PRED].gen)
                d_pred_in = reinterpret_cast<const int*>(d_pred + (size_t)kp.half * half);
            else kp.half = 0;
            d_pred_out = reinterpret_cast<int*>(d_pred + (size_t)(kp.half ^ 1) * half);
        }
        pred_half = kp.half ^ 1;
        crit = SadCriteria::of(o).without_split();
        filtered = !klt && o.sad_batch_filter && crit.criteria();
        blk = {(size_t)n, filtered || klt};
        return filtered ? SadFilter::make({nullptr, nullptr, 0, 0, W, H, dstride}, 1, prm->block, prm->range, crit, /*want_triples=*/false).plan(ctx, "push_frames_async")
                        : OFPS_HIP_OK;
    }

    // capacity: both buffers and the per-ticket outputs are sized for the largest batch seen (grow-only; growing waits for work in flight)
    int reserve() {
        const size_t cap_frames = (size_t)n + 1;
        auto& fs = ctx->scratch[S_BATCH_FRAMES];
        size_t per_buf = fs.cap / kTickets / (pitch ? pitch : 1);
        if (per_buf < cap_frames) {
            OFPS_HIP_TRY(ctx, ctx->batch.ring.drain(/*forget=*/false));
            // the newest frame of the stream lives in the old allocation: keep a copy
            void* keep = nullptr;
            if (ctx->batch.last_frame) {
                OFPS_HIP_TRY(ctx, hipMalloc(&keep, pitch));
                OFPS_HIP_TRY(ctx, hipMemcpyAsync(keep, ctx->batch.last_frame, pitch, hipMemcpyDeviceToDevice, ctx->stream));
                OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            }
            auto* nb = static_cast<uint8_t*>(scratch(ctx, S_BATCH_FRAMES, kTickets * cap_frames * pitch));
            if (!nb) { if (keep) (void)hipFree(keep); return OFPS_HIP_ENOMEM; }
            per_buf = cap_frames;
            if (keep) {
                // parked in the LAST slot of the buffer this ticket does not use: nothing writes there before it is consumed
                uint8_t* park = nb + ((size_t)(tix ^ 1) * per_buf + (per_buf - 1)) * pitch;
                OFPS_HIP_TRY(ctx, hipMemcpyAsync(park, keep, pitch, hipMemcpyDeviceToDevice, ctx->stream));
                OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
                (void)hipFree(keep);
                ctx->batch.last_frame = park;
            }
        }
        buf = static_cast<uint8_t*>(fs.p) + (size_t)tix * per_buf * pitch;
        auto* d_ent_all = static_cast<float4*>(scratch(ctx, S_BATCH_ENTRIES, kTickets * (size_t)n * nblk * sizeof(float4)));
        auto* d_out_all = static_cast<char*>(scratch(ctx, S_BATCH_OUT, kTickets * blk.bytes()));
        if (!d_ent_all || !d_out_all) return OFPS_HIP_ENOMEM;
        d_ent = d_ent_all + (size_t)tix * (ctx->scratch[S_BATCH_ENTRIES].cap / kTickets / sizeof(float4));
        d_out = d_out_all + (size_t)tix * (ctx->scratch[S_BATCH_OUT].cap / kTickets);
        return host_block_reserve(ctx, &t->pinned, &t->pinned_cap, blk.bytes());
    }

    // copy stream: the n frames in one transfer (the buffer's previous tenant, ticket tno - 2, has been collected: its work is done);
    // compute stream: the previous frame into slot 0, then the wait for the transfer
    int upload() {
        hipStream_t s = ctx->stream, up = ctx->pipe.copy_stream;
        // the other ticket's copy of ITS previous frame reads slot n of this buffer's previous tenant: wait for it
        auto& other = ctx->batch.ring.at(tno + 1);
        if (other.pending && other.prev_copied_valid) OFPS_HIP_TRY(ctx, hipStreamWaitEvent(up, other.prev_copied, 0));
        if (frame_pitch == (size_t)W * H && stride == W && dstride == W) {
            const int rc = upload_dense_device(ctx, buf + pitch, frames, (size_t)n * pitch, up, true);                        // the whole batch
            if (rc != OFPS_HIP_OK) return rc;
        } else {
            for (int j = 0; j < n; ++j)
                OFPS_HIP_TRY(ctx, upload_rows(buf + (size_t)(j + 1) * pitch, dstride, frames + (size_t)j * frame_pitch, stride, W, H, up));
        }
        if (halo_mode && halo) OFPS_HIP_TRY(ctx, upload_rows(buf, dstride, halo, halo_stride ? halo_stride : stride, W, H, up));       // the caller's previous frame into slot 0
        OFPS_HIP_TRY(ctx, hipEventRecord(t->uploaded, up));
        has_prev = halo_mode ? halo != nullptr : ctx->batch.last_frame != nullptr;
        t->prev_copied_valid = false;
        if (has_prev && !halo_mode) {
            // by a copy KERNEL, not hipMemcpyAsync: the runtime may hand a device-to-device copy to the SDMA engine that is busy with the
            // NEXT batch's 33 MB upload, and then this 2 MB copy -- and the search behind it -- waits 0.1-0.6 ms for that upload (transfer.hip)
            const int rc = copy_words_device(ctx, buf, ctx->batch.last_frame, pitch / 4, 256, s);
            if (rc != OFPS_HIP_OK) return rc;
            OFPS_HIP_TRY(ctx, hipEventRecord(t->prev_copied, s));
            t->prev_copied_valid = true;
        }
        OFPS_HIP_TRY(ctx, hipStreamWaitEvent(s, t->uploaded, 0));
        first = has_prev ? 0 : 1;
        pairs = n - first;
        // what holds whether or not a pair follows: no slots to chain from until decode() says so, and the ticket's islands
        ctx->batch.klt_pred.valid = false;
        if (halo_mode) t->isl.K = 0;                                 // the multi-device workers list no islands (include/ofps_hip.h A5i)
        else islands_ticket_arm(ctx, &t->isl, prm, n, TRK_BATCH, /*restart=*/!has_prev);
        return OFPS_HIP_OK;
    }

    // the one choice among the three decoders, on the compute stream: item j's [kept] records lead its slot of the record buffer [, its count
    // is d_cnt()[j]; searches, flags and the compaction run in front of the tail that reads the counts there]
    int decode() {
        const auto& o = ctx->opt;
        const SadFrames fr = SadFrames::sequence(buf + (size_t)first * pitch, pitch, /*ref_mode=*/0, W, H, dstride);
        if (klt) {
            const int rc = klt_flow_device(ctx, KltFlowCall{fr, pairs, o.klt_levels, o.klt_radius, o.klt_iters, ent0(), d_cnt(), nullptr, true, chained, d_pred_in, d_pred_out});
            if (rc == OFPS_HIP_OK && chained) ctx->batch.klt_pred = {true, pred_half, W, H, o.klt_cell, ctx->scratch[S_KLT_BATCH_PRED].gen};
            return rc;
        }
        if (filtered) return sad_flow_filtered_device(ctx, fr, pairs, prm->block, prm->range, crit, ent0(), nullptr, d_cnt(), "push_frames_async", tix, kTickets);
        return sad_pairs_device(ctx, fr, pairs, prm->block, prm->range, ent0(), nullptr);
    }

    // one estimator launch, [one compensation launch,] one detector chain over the batch, item j seeded seed + j.  The multi-device
    // dispatcher's worker contexts (halo_mode 1) keep the raw detector whatever their detect-compensation mode.  filtered: the tail's
    // device-count forms with one count per item; fewer than 3 kept -> identity, as in the filtered per-frame path
    int tail() {
        float2* d_field = nullptr;
        if (prm->run_detector) {
            d_field = static_cast<float2*>(scratch(ctx, S_BATCH_FIELD, (size_t)pairs * kMaxFieldBytes));   // its own slot: the densifier works in S_WORK*
            if (!d_field) return OFPS_HIP_ENOMEM;
        }
        return frame_tail_device(ctx, ent0(), nblk, pairs, d_cnt(), filtered ? 3 : 0, prm, prm->seed + (uint64_t)first, /*may_compensate=*/!halo_mode,
                                 blk.result(d_out, first), blk.quat(d_out, first), d_field, nullptr, nullptr, &t->isl);
    }

    int read_back(float* out_entries) {
        hipStream_t s = ctx->stream;
        int rc = OFPS_HIP_OK;
        if (blk.counted || prm->run_detector || prm->run_estimator) rc = read_back_device(ctx, t->pinned, d_out, blk.bytes(), s);     // (the kept counts travel in this read-back)
        if (rc == OFPS_HIP_OK && out_entries) rc = read_back_device(ctx, out_entries + (size_t)first * nblk * 4, ent0(), (size_t)pairs * nblk * sizeof(float4), s);
        return rc;
    }

    int commit(int* ticket) {
        OFPS_HIP_TRY(ctx, hipEventRecord(t->done, ctx->stream));
        ctx->batch.last_frame = buf + (size_t)n * pitch;
        t->n = n; t->first_has_prev = has_prev ? 1 : 0; t->run_detector = prm->run_detector; t->run_estimator = prm->run_estimator; t->n_vectors = nblk;
        t->filtered = blk.counted && pairs > 0;
        *ticket = ctx->batch.ring.commit();
        return OFPS_HIP_OK;
    }
};
}  // namespace

// halo_mode 0: frame 0 of the batch is paired with the context's own previous frame (ofps_hip_push_frames_async).
// halo_mode 1: the caller supplies the previous frame (`halo`, host memory, rows `halo_stride` bytes apart; 0 = `stride`) or says there is none
// (halo == nullptr: the very first frame of a stream) -- the multi-device dispatcher's form (multi.hip): a worker sees every
// n_workers-th batch of a stream, so the frame in front of its batch is not the last one IT saw.
int push_frames_impl(ofps_hip_ctx* ctx, const uint8_t* frames, int n, int W, int H, int stride, size_t frame_pitch,
                     const ofps_hip_frame_params* prm, float* out_entries, int* ticket, int halo_mode, const uint8_t* halo, int halo_stride) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, frames && prm && ticket && n >= 1 && n <= 4096, "push_frames_async: bad arguments (n=%d)", n);
    OFPS_REQUIRE(ctx, W > 0 && H > 0 && stride >= W && frame_pitch >= (size_t)stride * H, "push_frames_async: bad geometry W=%d H=%d stride=%d", W, H, stride);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = pipe_setup(ctx);
    if (rc != OFPS_HIP_OK) return rc;
    BatchPush p{ctx, prm, frames, n, W, H, stride, frame_pitch, halo_mode, halo, halo_stride};
    rc = p.claim();                                     // refused before anything is uploaded
    if (rc == OFPS_HIP_OK) rc = p.reserve();
    if (rc == OFPS_HIP_OK) rc = p.upload();
    if (rc == OFPS_HIP_OK && p.pairs > 0) {
        rc = p.decode();
        if (rc == OFPS_HIP_OK) rc = p.tail();
        if (rc == OFPS_HIP_OK) rc = p.read_back(out_entries);
    }
    return rc == OFPS_HIP_OK ? p.commit(ticket) : rc;
}
}  // namespace ofps

extern "C" {

int ofps_hip_push_frames_async(ofps_hip_ctx* ctx, const uint8_t* frames, int n, int W, int H, int stride, size_t frame_pitch,
                               const ofps_hip_frame_params* prm, float* out_entries, int* ticket) {
    return ofps::push_frames_impl(ctx, frames, n, W, H, stride, frame_pitch, prm, out_entries, ticket, 0, nullptr, 0);
}

int ofps_hip_frames_wait(ofps_hip_ctx* ctx, int ticket, ofps_hip_frame_result* out /* n of them */) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, out, "frames_wait: null pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto* t = ctx->batch.ring.claim(ctx, ticket, "frames_wait", "was already");
    if (!t) return OFPS_HIP_EINVAL;
    OFPS_HIP_TRY(ctx, hipEventSynchronize(t->done));
    t->pending = false;
    const ofps::BatchBlock blk{(size_t)t->n, t->filtered != 0};
    char* base = static_cast<char*>(t->pinned);
    const uint32_t* kept = blk.kept(base);
    for (int j = 0; j < t->n; ++j) {
        const bool has = j > 0 || t->first_has_prev;
        ofps::fill_frame_result(&out[j], has ? 1 : 0, !has ? 0 : kept && kept[j] < t->n_vectors ? kept[j] : t->n_vectors,
                                has && t->run_detector ? blk.result(base, j) : nullptr, has && t->run_estimator ? blk.quat(base, j) : nullptr);
    }
    return ofps::islands_collect(ctx, t->isl);
}

int ofps_hip_push_frame(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride,
                        const ofps_hip_frame_params* prm, ofps_hip_frame_result* out, float* out_entries,
                        float* out_field) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, luma && prm && out, "push_frame: null pointer");
    int ticket = 0;
    int rc = ofps_hip_push_frame_async(ctx, luma, W, H, stride, prm, out_entries, out_field, &ticket);
    if (rc != OFPS_HIP_OK) return rc;
    return ofps_hip_frame_wait(ctx, ticket, out);
}

}  // extern "C"
