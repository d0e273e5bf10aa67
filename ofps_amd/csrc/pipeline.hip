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
struct PipeOut {                 // layout of the pinned read-back block
    int result[4];               // has_motion, area, dim, 0
    float quat[4];
    uint32_t kept[4];            // contrast gate or consistency check on: the kept record count (sad_gate.hip, sad_consistency.hip); not read back, not looked at, with both off
};
constexpr size_t kPipeOutPlain = offsetof(PipeOut, kept);       // what a ticket without the gate reads back
constexpr int kSlots = ofps::PipeStream::kSlots;

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
    const int dstride = (W + 63) & ~63;
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
}  // namespace

extern "C" {

int ofps_hip_reset_frames(ofps_hip_ctx* ctx) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    OFPS_HIP_TRY(ctx, ctx->batch.ring.drain());
    ctx->batch.last_frame = nullptr;
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
    constexpr int kTickets = ofps::PipeStream::kTickets;
    const long tno = ctx->pipe.ring.next;
    auto& t = ctx->pipe.ring.at(tno);
    OFPS_REQUIRE(ctx, !t.pending, "push_frame_async: ticket %ld has not been collected (at most %d frames in flight)",
                 tno - kTickets, kTickets);
    // contrast gate (sad_gate.hip; the gate is the context's at this push): 0 = every launch, stream and byte below is the ungated build's
    const int gate = ctx->opt.sad_gate;
    if (gate > 0) {
        rc = ofps::sad_gate_check(ctx, prm->block, gate, "push_frame_async");
        if (rc != OFPS_HIP_OK) return rc;
    }
    // consistency check (sad_consistency.hip; the limit is the context's at this push): one more producer of keep flags on the gate's path.
    // `filtered`: either criterion is on; with only the gate on, everything enqueued below is what it was before the check existed
    const int limit = ctx->opt.sad_consistency;
    if (limit > 0) {
        rc = ofps::sad_consistency_check(ctx, prm->block, limit, "push_frame_async");
        if (rc != OFPS_HIP_OK) return rc;
    }
    const bool filtered = gate > 0 || limit > 0;
    hipStream_t s = ctx->stream;
    uint8_t* slots; size_t pitch; int dstride;
    const bool overlap = ctx->pipe.ring.other_pending();               // the other ticket is in flight
    rc = pipe_upload(ctx, luma, W, H, stride, overlap, &slots, &pitch, &dstride);
    if (rc != OFPS_HIP_OK) return rc;
    const long frame_no = ctx->pipe.frames - 1;                       // the frame just enqueued
    const int cur_slot = (int)(frame_no % kSlots);
    t.have_vectors = 0; t.n_vectors = 0; t.run_detector = prm->run_detector; t.run_estimator = prm->run_estimator; t.gated = 0;
    const size_t nblk = ofps_hip_sad_block_count(W, H, prm->block);
    if (frame_no == 0) {                                             // first frame of a stream: Ok(false), no vectors yet
        if (!ctx->pipe.uploaded_on_compute[cur_slot]) {
            OFPS_HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->pipe.uploaded[cur_slot], 0));
            ctx->pipe.uploaded_on_compute[cur_slot] = true;
        }
        OFPS_HIP_TRY(ctx, hipEventRecord(t.done, s));
        *ticket = ctx->pipe.ring.commit();
        return OFPS_HIP_OK;
    }
    const int prev_slot = (int)((frame_no - 1) % kSlots);
    const int tix = (int)(tno % kTickets);
    auto* d_ent_all = static_cast<float4*>(ofps::scratch(ctx, ofps::S_PIPE_ENTRIES, kTickets * nblk * sizeof(float4)));
    constexpr size_t kOutBytes = 4096 + (size_t)160 * 160 * sizeof(float2);
    auto* d_out_all = static_cast<char*>(ofps::scratch(ctx, ofps::S_PIPE_OUT, kTickets * kOutBytes));
    if (!d_ent_all || !d_out_all) return OFPS_HIP_ENOMEM;
    float4* d_ent = d_ent_all + (size_t)tix * nblk;
    char* d_out = d_out_all + (size_t)tix * kOutBytes;
    // the search needs both frames on the device: the previous frame's upload was waited for by the previous ticket
    // (or by the stage_frame that made it), this frame's by the event
    // (uploads made on the compute stream itself are ordered by the stream; one wait per upload is enough)
    const bool cur_by_event = !ctx->pipe.uploaded_on_compute[cur_slot];      // this frame's upload is on the copy stream and has an event of its own
    for (int slot : {prev_slot, cur_slot}) {
        if (!ctx->pipe.uploaded_on_compute[slot]) {
            OFPS_HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->pipe.uploaded[slot], 0));
            ctx->pipe.uploaded_on_compute[slot] = true;
        }
    }
    // gate on: the keep flags depend on the new frame only -- they are made on the auxiliary stream, forked on that frame's upload, beside
    // the search (never in front of it on the compute stream); the search writes one record per block into the gate's own slot and the
    // compaction behind the join leaves the kept records, in raster order, in d_ent and their count in device memory (d_kept)
    float4* d_raw = d_ent;
    char* d_flags = nullptr;
    uint32_t* d_kept = nullptr;
    if (filtered) {
        const size_t fbytes = ofps::gate_flags_bytes(nblk);
        d_raw = static_cast<float4*>(ofps::scratch(ctx, ofps::S_GATE_RAW, nblk * sizeof(float4)));
        auto* d_flags_all = static_cast<char*>(ofps::scratch(ctx, ofps::S_GATE_FLAGS, kTickets * fbytes));
        if (!d_raw || !d_flags_all) return OFPS_HIP_ENOMEM;
        d_flags = d_flags_all + (size_t)tix * fbytes;
        d_kept = ofps::gate_kept(d_flags, nblk);
    }
    if (gate > 0) {
        if (!ctx->pipe.gate_done) OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->pipe.gate_done, hipEventDisableTiming));
        // fork on the upload: its own event when it ran on the copy stream (the flags are then made beside the previous ticket's tail as
        // well), else the compute stream's position, which is right behind the upload
        if (cur_by_event) {
            OFPS_HIP_TRY(ctx, hipStreamWaitEvent(ctx->pipe.aux_stream, ctx->pipe.uploaded[cur_slot], 0));
        } else {
            OFPS_HIP_TRY(ctx, hipEventRecord(ctx->pipe.fork, s));
            OFPS_HIP_TRY(ctx, hipStreamWaitEvent(ctx->pipe.aux_stream, ctx->pipe.fork, 0));
        }
        rc = ofps::sad_gate_flags_device(ctx, slots + (size_t)cur_slot * pitch, W, H, dstride, prm->block, gate, ofps::gate_counts(d_flags),
                                         ofps::gate_keep(d_flags, nblk), ctx->pipe.aux_stream);
        if (rc != OFPS_HIP_OK) return rc;
        OFPS_HIP_TRY(ctx, hipEventRecord(ctx->pipe.gate_done, ctx->pipe.aux_stream));
    }
    // check on: the forward search keeps its integer winners, the backward search runs on the same two resident slots right behind it on the
    // compute stream (one context's searches share scratch: never two at once) -- both read prev_slot, so its event is recorded behind both
    const int *d_fwd = nullptr, *d_bwd = nullptr;
    if (limit > 0)
        rc = ofps::sad_consistency_searches_device(ctx, slots + (size_t)prev_slot * pitch, slots + (size_t)cur_slot * pitch, W, H, dstride,
                                                   prm->block, prm->range, d_raw, false, &d_fwd, &d_bwd, nullptr);
    else
        rc = ofps::sad_pairs_device(ctx, slots + (size_t)prev_slot * pitch, 0, slots + (size_t)cur_slot * pitch, 0, 1, W, H, dstride,
                                    prm->block, prm->range, d_raw, nullptr);
    if (rc != OFPS_HIP_OK) return rc;
    // the older slot may be overwritten once this search is through; the same event forks the detector's stream below
    // (one barrier packet between the search and the estimator instead of two)
    OFPS_HIP_TRY(ctx, hipEventRecord(ctx->pipe.slot_read[prev_slot], s));
    ctx->pipe.slot_read_valid[prev_slot] = true;
    t.have_vectors = 1; t.n_vectors = nblk; t.gated = filtered;
    if (filtered) {
        if (gate > 0) OFPS_HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->pipe.gate_done, 0));
        if (limit > 0) {                                         // behind the join: the contrast flags, when there are any, are ANDed in in place
            uint8_t* d_keep = ofps::gate_keep(d_flags, nblk);
            rc = ofps::sad_consistency_flags_device(ctx, d_fwd, d_bwd, W, H, prm->block, limit, gate > 0 ? d_keep : nullptr, nullptr, d_keep, s);
            if (rc != OFPS_HIP_OK) return rc;
        }
        rc = ofps::sad_gate_compact_device(ctx, d_raw, nullptr, ofps::gate_keep(d_flags, nblk), nblk, d_ent, nullptr, d_kept);
        if (rc != OFPS_HIP_OK) return rc;
    }

    int dim = 0;
    int* d_res = reinterpret_cast<int*>(d_out);
    float4* d_quat = reinterpret_cast<float4*>(d_out + 16);
    float2* d_field = reinterpret_cast<float2*>(d_out + 4096);
    // The 32 bytes the caller waits for (island result, quaternion) are written by the detector's and the estimator's last
    // kernels STRAIGHT into the ticket's page-locked block -- it is device-addressable, each is one thread's store at the
    // end of a kernel -- instead of into device scratch and from there by a copy launch behind the join: that launch and
    // the gap in front of it were 14 us of a 170 us frame (rocprofv3 kernel trace, tools/trace_stream.sh).
    void* mapped_out = nullptr;
    const bool direct = ofps::device_address_of(t.pinned, &mapped_out);
    if (direct) {
        d_res = reinterpret_cast<int*>(static_cast<char*>(mapped_out) + offsetof(PipeOut, result));
        d_quat = reinterpret_cast<float4*>(static_cast<char*>(mapped_out) + offsetof(PipeOut, quat));
    }
    // detector and estimator read the same device-resident vectors and share no workspace: with both enabled the
    // detector's chain of small launches runs on an auxiliary stream beside the estimator (fork after the search, join
    // before the read-back) instead of in front of it
    // detect-compensation mode 1 (compensate.hip; the mode is the context's at this push): the detector reads this frame's vectors
    // compensated with this frame's quaternion, so its chain cannot run beside the estimator -- estimator, compensation and detector are
    // enqueued on the compute stream in that order.  The estimator writes the quaternion to device memory (the compensation launch reads it
    // there and passes it on to the ticket's block); the compensated records have a slot of their own: d_ent is what the caller gets.
    const bool compensate = ctx->opt.detect_compensate == 1 && prm->run_detector && prm->run_estimator;
    const bool fork = prm->run_detector && prm->run_estimator && !compensate;
    if (fork && filtered) {                                      // the detector's stream starts behind the compaction, not behind the search
        OFPS_HIP_TRY(ctx, hipEventRecord(ctx->pipe.fork, s));
        OFPS_HIP_TRY(ctx, hipStreamWaitEvent(ctx->pipe.aux_stream, ctx->pipe.fork, 0));
    } else if (fork) OFPS_HIP_TRY(ctx, hipStreamWaitEvent(ctx->pipe.aux_stream, ctx->pipe.slot_read[prev_slot], 0));
    // gate or check on: estimator, compensation and detector in their device-count forms -- every launch sized from the capacity nblk, the first
    // *d_kept records count; fewer than 3 kept records -> identity (both solvers), none -> no motion
    auto estimate = [&](float4* d_q) {
        return filtered ? ofps::almeida_device_n(ctx, d_ent, nblk, d_kept, prm->aspect, prm->fov_y_deg, prm->use_ransac, prm->num_iters,
                                                 prm->inlier_deg, prm->num_samples, prm->seed, d_q, /*lsq_min_n=*/3)
                        : ofps::almeida_device(ctx, d_ent, nblk, 1, prm->aspect, prm->fov_y_deg, prm->use_ransac, prm->num_iters,
                                               prm->inlier_deg, prm->num_samples, prm->seed, d_q);
    };
    const float4* d_det_in = d_ent;
    if (compensate) {
        auto* d_comp = static_cast<float4*>(ofps::scratch(ctx, ofps::S_COMP, nblk * sizeof(float4)));
        if (!d_comp) return OFPS_HIP_ENOMEM;
        float4* d_quat_dev = reinterpret_cast<float4*>(d_out + 16);
        rc = estimate(d_quat_dev);
        if (rc != OFPS_HIP_OK) return rc;
        rc = ofps::compensate_device(ctx, d_ent, nblk, 1, d_kept, prm->aspect, prm->fov_y_deg, d_quat_dev, d_comp, direct ? d_quat : nullptr);
        if (rc != OFPS_HIP_OK) return rc;
        d_det_in = d_comp;
    }
    // the estimator is enqueued first: it is the long pole (0.1 ms of dependent steps against the detector's seven small
    // launches), and whatever is enqueued second starts a host-enqueue time later
    if (prm->run_estimator && !compensate) {
        rc = estimate(d_quat);
        if (rc != OFPS_HIP_OK) return rc;
    }
    if (prm->run_detector) {
        if (fork) ctx->stream = ctx->pipe.aux_stream;           // the stage entry points enqueue on ctx->stream
        rc = ofps::detect_device(ctx, d_det_in, nblk, 1, prm->min_size, prm->subdivide, prm->target_motion, d_res, d_field, &dim, d_kept);
        if (fork) {
            ctx->stream = s;
            if (rc == OFPS_HIP_OK) OFPS_HIP_TRY(ctx, hipEventRecord(ctx->pipe.join, ctx->pipe.aux_stream));
        }
        if (rc != OFPS_HIP_OK) return rc;
    }
    if (fork) OFPS_HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->pipe.join, 0));
    if ((prm->run_detector || prm->run_estimator) && !direct) {
        rc = ofps::read_back_device(ctx, t.pinned, d_out, kPipeOutPlain, s);
        if (rc != OFPS_HIP_OK) return rc;
    }
    if (filtered) {                                              // the kept count travels in the ticket's page-locked block
        rc = ofps::read_back_device(ctx, static_cast<char*>(t.pinned) + offsetof(PipeOut, kept), d_kept, sizeof(uint32_t), s);
        if (rc != OFPS_HIP_OK) return rc;
    }
    if (out_entries && nblk) {
        rc = ofps::read_back_device(ctx, out_entries, d_ent, nblk * sizeof(float4), s);
        if (rc != OFPS_HIP_OK) return rc;
    }
    if (out_field && prm->run_detector) {
        rc = ofps::read_back_device(ctx, out_field, d_field, (size_t)dim * dim * sizeof(float2), s);
        if (rc != OFPS_HIP_OK) return rc;
    }
    OFPS_HIP_TRY(ctx, hipEventRecord(t.done, s));
    *ticket = ctx->pipe.ring.commit();
    return OFPS_HIP_OK;
}

int ofps_hip_frame_wait(ofps_hip_ctx* ctx, int ticket, ofps_hip_frame_result* out) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, out, "frame_wait: null pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto* t = ctx->pipe.ring.find(ticket);
    OFPS_REQUIRE(ctx, t, "frame_wait: ticket %d is not in flight", ticket);
    OFPS_REQUIRE(ctx, t->pending, "frame_wait: ticket %d was already collected", ticket);
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
    memset(out, 0, sizeof(*out));
    out->quat[0] = 1.0f;
    out->have_vectors = t->have_vectors;
    out->n_vectors = t->n_vectors;
    if (t->have_vectors) {
        const auto* host = static_cast<const PipeOut*>(t->pinned);
        if (t->gated) out->n_vectors = host->kept[0] < t->n_vectors ? host->kept[0] : t->n_vectors;
        if (t->run_detector) {
            out->has_motion = host->result[0];
            out->area = (size_t)host->result[1];
            out->dim = host->result[2];
        }
        if (t->run_estimator) memcpy(out->quat, host->quat, sizeof(out->quat));
    }
    return OFPS_HIP_OK;
}

// ---- batched read-ahead form: n consecutive frames of the stream per ticket.  What a decoder that runs n frames ahead
// (ofps-suite/src/app/tracking/worker.rs:165-226 decodes into a buffer on its own thread) hands over in one go: ONE H2D of the
// n frames (contiguous at frame_pitch), one search launch over the batch's pairs, one detector chain and one estimator
// launch over the batch, one read-back -- a handful of HIP calls per BATCH instead of ~9 per frame, which is what kept
// the single-frame loop 20 % under the PCIe ceiling.  Frame j of the batch is pair (previous frame of the stream, frame
// j); the previous frame of frame 0 is the last frame of the previous batch, kept in slot 0 of the other batch buffer.
}  // extern "C"

namespace ofps {
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
    constexpr int kTickets = BatchStream::kTickets;
    const long tno = ctx->batch.ring.next;
    auto& t = ctx->batch.ring.at(tno);
    OFPS_REQUIRE(ctx, !t.pending, "push_frames_async: ticket %ld has not been collected (at most %d batches in flight)",
                 tno - kTickets, kTickets);
    if (!t.done) {
        OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
        OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&t.uploaded, hipEventDisableTiming));
        OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&t.prev_copied, hipEventDisableTiming));
    }
    if (W != ctx->batch.w || H != ctx->batch.h) {              // geometry change restarts the stream
        OFPS_HIP_TRY(ctx, ctx->batch.ring.drain());
        ctx->batch.w = W; ctx->batch.h = H; ctx->batch.last_frame = nullptr;
    }
    const int dstride = (W + 63) & ~63;
    const size_t pitch = (size_t)dstride * H;
    const size_t nblk = ofps_hip_sad_block_count(W, H, prm->block);
    const int tix = (int)(tno % kTickets);
    // capacity: both buffers and the per-ticket outputs are sized for the largest batch seen (grow-only; growing waits
    // for work in flight)
    constexpr size_t kOutBytes = 32;                             // {result[4], quat[4]} per frame
    const size_t cap_frames = (size_t)n + 1;
    auto& fs = ctx->scratch[ofps::S_BATCH_FRAMES];
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
        auto* nb = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_BATCH_FRAMES, kTickets * cap_frames * pitch));
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
    auto* bufs = static_cast<uint8_t*>(fs.p);
    uint8_t* buf = bufs + (size_t)tix * per_buf * pitch;        // [slot 0 = previous frame][n frames]
    auto* d_ent_all = static_cast<float4*>(ofps::scratch(ctx, ofps::S_BATCH_ENTRIES, kTickets * (size_t)n * nblk * sizeof(float4)));
    auto* d_out_all = static_cast<char*>(ofps::scratch(ctx, ofps::S_BATCH_OUT, kTickets * (size_t)n * kOutBytes));
    if (!d_ent_all || !d_out_all) return OFPS_HIP_ENOMEM;
    const size_t ent_per_ticket = ctx->scratch[ofps::S_BATCH_ENTRIES].cap / kTickets / sizeof(float4);
    const size_t out_per_ticket = ctx->scratch[ofps::S_BATCH_OUT].cap / kTickets;
    float4* d_ent = d_ent_all + (size_t)tix * ent_per_ticket;
    char* d_out = d_out_all + (size_t)tix * out_per_ticket;
    rc = host_block_reserve(ctx, &t.pinned, &t.pinned_cap, (size_t)n * kOutBytes);
    if (rc != OFPS_HIP_OK) return rc;
    hipStream_t s = ctx->stream, up = ctx->pipe.copy_stream;
    // ---- copy stream: the n frames in one transfer (the buffer's previous tenant, ticket tno - 2, has been collected:
    // its work is done); compute stream: the previous frame into slot 0
    // the other ticket's copy of ITS previous frame reads slot n of this buffer's previous tenant: wait for it
    auto& other = ctx->batch.ring.at(tno + 1);
    if (other.pending && other.prev_copied_valid) OFPS_HIP_TRY(ctx, hipStreamWaitEvent(up, other.prev_copied, 0));
    if (frame_pitch == (size_t)W * H && stride == W && dstride == W) {
        rc = upload_dense_device(ctx, buf + pitch, frames, (size_t)n * pitch, up, true);                                       // the whole batch
        if (rc != OFPS_HIP_OK) return rc;
    } else {
        for (int j = 0; j < n; ++j)
            OFPS_HIP_TRY(ctx, ofps::upload_rows(buf + (size_t)(j + 1) * pitch, dstride, frames + (size_t)j * frame_pitch, stride, W, H, up));
    }
    if (halo_mode && halo) OFPS_HIP_TRY(ctx, ofps::upload_rows(buf, dstride, halo, halo_stride ? halo_stride : stride, W, H, up));       // the caller's previous frame into slot 0
    OFPS_HIP_TRY(ctx, hipEventRecord(t.uploaded, up));
    const bool has_prev = halo_mode ? halo != nullptr : ctx->batch.last_frame != nullptr;
    t.prev_copied_valid = false;
    if (has_prev && !halo_mode) {
        // by a copy KERNEL, not hipMemcpyAsync: the runtime may hand a device-to-device copy to the SDMA engine that is busy with the
        // NEXT batch's 33 MB upload, and then this 2 MB copy -- and the search behind it -- waits 0.1-0.6 ms for that upload (transfer.hip)
        rc = copy_words_device(ctx, buf, ctx->batch.last_frame, pitch / 4, 256, s);
        if (rc != OFPS_HIP_OK) return rc;
        OFPS_HIP_TRY(ctx, hipEventRecord(t.prev_copied, s));
        t.prev_copied_valid = true;
    }
    OFPS_HIP_TRY(ctx, hipStreamWaitEvent(s, t.uploaded, 0));
    // ---- compute stream: pairs (slot j, slot j + 1), j = first .. n - 1
    const int first = has_prev ? 0 : 1;                           // the stream's very first frame has no pair
    const int pairs = n - first;
    t.n = n; t.first_has_prev = has_prev ? 1 : 0; t.run_detector = prm->run_detector; t.run_estimator = prm->run_estimator; t.n_vectors = nblk;
    if (pairs > 0) {
        float4* ent0 = d_ent + (size_t)first * nblk;
        rc = ofps::sad_pairs_device(ctx, buf + (size_t)first * pitch, pitch, buf + (size_t)(first + 1) * pitch, pitch, pairs, W, H, dstride,
                                    prm->block, prm->range, ent0, nullptr);
        if (rc != OFPS_HIP_OK) return rc;
        int* d_res = reinterpret_cast<int*>(d_out);                                 // [n][4]
        float4* d_quat = reinterpret_cast<float4*>(d_out + (size_t)n * 16);          // [n]
        if (prm->run_estimator) {
            rc = ofps::almeida_device(ctx, ent0, nblk, pairs, prm->aspect, prm->fov_y_deg, prm->use_ransac, prm->num_iters, prm->inlier_deg,
                                      prm->num_samples, prm->seed + (uint64_t)first, d_quat + first);
            if (rc != OFPS_HIP_OK) return rc;
        }
        if (prm->run_detector) {
            int dim = 0;
            auto* d_field = static_cast<float2*>(ofps::scratch(ctx, ofps::S_BATCH_FIELD, (size_t)pairs * 160 * 160 * sizeof(float2)));   // its own slot: the densifier works in S_WORK*
            if (!d_field) return OFPS_HIP_ENOMEM;
            // detect-compensation mode 1: ONE compensation launch over the batch, item j with the quaternion the estimator's launch above left
            // for it in device memory, into a slot of its own; then the batched detector chain as it is.  The multi-device dispatcher's
            // worker contexts (halo_mode 1) keep the raw detector.
            const float4* det_in = ent0;
            if (ctx->opt.detect_compensate == 1 && prm->run_estimator && !halo_mode) {
                auto* d_comp = static_cast<float4*>(ofps::scratch(ctx, ofps::S_COMP, (size_t)pairs * nblk * sizeof(float4)));
                if (!d_comp) return OFPS_HIP_ENOMEM;
                rc = ofps::compensate_device(ctx, ent0, nblk, pairs, nullptr, prm->aspect, prm->fov_y_deg, d_quat + first, d_comp, nullptr);
                if (rc != OFPS_HIP_OK) return rc;
                det_in = d_comp;
            }
            rc = ofps::detect_device(ctx, det_in, nblk, pairs, prm->min_size, prm->subdivide, prm->target_motion, d_res + 4 * first, d_field, &dim);
            if (rc != OFPS_HIP_OK) return rc;
        }
        if (prm->run_detector || prm->run_estimator) {
            rc = ofps::read_back_device(ctx, t.pinned, d_out, (size_t)n * kOutBytes, s);
            if (rc != OFPS_HIP_OK) return rc;
        }
        if (out_entries) {
            rc = ofps::read_back_device(ctx, out_entries + (size_t)first * nblk * 4, ent0, (size_t)pairs * nblk * sizeof(float4), s);
            if (rc != OFPS_HIP_OK) return rc;
        }
    }
    OFPS_HIP_TRY(ctx, hipEventRecord(t.done, s));
    ctx->batch.last_frame = buf + (size_t)n * pitch;
    *ticket = ctx->batch.ring.commit();
    return OFPS_HIP_OK;
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
    auto* t = ctx->batch.ring.find(ticket);
    OFPS_REQUIRE(ctx, t, "frames_wait: ticket %d is not in flight", ticket);
    OFPS_REQUIRE(ctx, t->pending, "frames_wait: ticket %d was already collected", ticket);
    OFPS_HIP_TRY(ctx, hipEventSynchronize(t->done));
    t->pending = false;
    const auto* res = static_cast<const int*>(t->pinned);
    const auto* quat = reinterpret_cast<const float*>(static_cast<const char*>(t->pinned) + (size_t)t->n * 16);
    for (int j = 0; j < t->n; ++j) {
        ofps_hip_frame_result& o = out[j];
        memset(&o, 0, sizeof(o));
        o.quat[0] = 1.0f;
        const bool has = j > 0 || t->first_has_prev;
        o.have_vectors = has ? 1 : 0;
        o.n_vectors = has ? t->n_vectors : 0;
        if (!has) continue;
        if (t->run_detector) { o.has_motion = res[4 * j]; o.area = (size_t)res[4 * j + 1]; o.dim = res[4 * j + 2]; }
        if (t->run_estimator) memcpy(o.quat, quat + 4 * j, sizeof(o.quat));
    }
    return OFPS_HIP_OK;
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
