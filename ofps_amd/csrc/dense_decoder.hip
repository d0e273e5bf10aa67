// dense_decoder.hip -- the dense decoders ("hip_lk" and "hip_flow", full-resolution and reduced) as a stage chain and as a read-ahead stream
// (ofps_hip_lk_decode / ofps_hip_lk_push_frame[_async] / ofps_hip_lk_frame_wait; state: common.hpp DenseStream), and the same stream with the
// detector and the estimator behind the decoder in the same ticket (ofps_hip_lk_push_frame_fused[_async] / ofps_hip_lk_frame_fused_wait).
// No flow kernel lives here.
//
// The body of a Decoder::process_frame (cv-decoder/src/lib.rs:82-294): dense flow (lk.hip, or farneback.hip with OFPS_HIP_FLOW_FARNEBACK),
// per-pixel records, optionally filtered by the contrast mask of :203-237 (OFPS_HIP_LK_CONTRAST_MASK, computed on `cur` like the
// reference's `self.gray`), then either down-sampled through the densifier to the (max_w, max_h)-capped grid of
// :98-121 with one record per visited cell in BTreeSet<(x,y)> order ("Process Fullres" = true, the default), or -- with
// OFPS_HIP_LK_REDUCED, "Process Fullres" = false -- computed on frames resized to that grid first (frontend.hip) and returned per pixel
// of the reduced frame in raster order (the `mf.push` branch, :274-276).  Only the final records leave the device.
#include "common.hpp"

namespace {

struct DenseGrid {              // what a process_frame returns for this geometry / these flags
    int gw = 0, gh = 0;         // the record grid
    int fw = 0, fh = 0;         // the frames the mask and the flow run on: W x H, or the record grid itself with OFPS_HIP_LK_REDUCED
    bool per_pixel = false;     // one record per (unmasked) pixel of the fw x fh frames (OFPS_HIP_LK_FULLRES_RECORDS, OFPS_HIP_LK_REDUCED)
    bool use_mask = false;
    bool farneback = false;     // OFPS_HIP_FLOW_FARNEBACK: the flow is farneback.hip's (the "hip_flow" decoder), not the iterative LK
    bool use_previous = false;  // OFPS_HIP_FLOW_USE_PREVIOUS: the stream's previous flow is the initial flow (cv-decoder/src/lib.rs:161-165)
    bool reduced = false;       // OFPS_HIP_LK_REDUCED: cv-decoder's "Process Fullres" = false (:124-133,274-276)
    bool sparse = false;        // OFPS_HIP_FLOW_SPARSE: hip_klt (klt.hip) in place of flow, mask and output stage; the record grid is its cell lattice
    int fmt = OFPS_HIP_FMT_LUMA, cn = 1;      // the arriving frames' pixel format (bits 8-9 of the flags)
    bool frontend = false;      // the arriving frames are resized and / or converted behind their upload (frontend.hip)
    size_t raw_row = 0;         // bytes per row of the staged arriving frame (W * cn rounded up to 4)
    size_t max_records = 0;     // capacity the records need
};

constexpr unsigned kDenseFlagBits = OFPS_HIP_LK_CONTRAST_MASK | OFPS_HIP_LK_FULLRES_RECORDS | OFPS_HIP_FLOW_FARNEBACK | OFPS_HIP_FLOW_USE_PREVIOUS |
                                 OFPS_HIP_LK_REDUCED | OFPS_HIP_FLOW_SPARSE | OFPS_HIP_FRAME_FORMAT_MASK;
// max_w / max_h are not looked at by hip_klt on full-size frames
inline bool dense_cap_ok(unsigned flags, int max_w, int max_h) {
    return ((flags & OFPS_HIP_FLOW_SPARSE) && !(flags & OFPS_HIP_LK_REDUCED)) || (max_w >= 1 && max_h >= 1);
}

// hip_klt has no mask, no per-pixel records and no flow to carry over: refused in front of every other test of the flags
int dense_sparse_flags(ofps_hip_ctx* ctx, unsigned flags, const char* who) {
    constexpr unsigned excluded = OFPS_HIP_LK_CONTRAST_MASK | OFPS_HIP_LK_FULLRES_RECORDS | OFPS_HIP_FLOW_FARNEBACK | OFPS_HIP_FLOW_USE_PREVIOUS;
    OFPS_REQUIRE(ctx, !(flags & OFPS_HIP_FLOW_SPARSE) || !(flags & excluded),
                 "%s: OFPS_HIP_FLOW_SPARSE excludes OFPS_HIP_LK_CONTRAST_MASK, OFPS_HIP_LK_FULLRES_RECORDS, OFPS_HIP_FLOW_FARNEBACK and "
                 "OFPS_HIP_FLOW_USE_PREVIOUS (flags 0x%x)", who, flags);
    return OFPS_HIP_OK;
}

int dense_grid_of(ofps_hip_ctx* ctx, int W, int H, int stride, int max_w, int max_h, unsigned flags, int levels, int radius, int iters, const char* who,
                  DenseGrid* g) {
    g->use_mask = flags & OFPS_HIP_LK_CONTRAST_MASK;
    g->farneback = flags & OFPS_HIP_FLOW_FARNEBACK;
    g->use_previous = flags & OFPS_HIP_FLOW_USE_PREVIOUS;
    g->reduced = flags & OFPS_HIP_LK_REDUCED;
    const bool fullres_records = flags & OFPS_HIP_LK_FULLRES_RECORDS;
    g->fmt = (int)((flags & OFPS_HIP_FRAME_FORMAT_MASK) >> 8);
    g->cn = ofps::frame_format_channels(g->fmt);
    g->sparse = flags & OFPS_HIP_FLOW_SPARSE;
    if (g->sparse) {
        const int rc = dense_sparse_flags(ctx, flags, who);
        if (rc != OFPS_HIP_OK) return rc;
        OFPS_REQUIRE(ctx, stride >= W * g->cn, "dense decoder: stride %d < %d bytes per row (%d x %d channels)", stride, W * g->cn, W, g->cn);
        g->fw = W; g->fh = H;
        if (g->reduced) {
            ofps::cv_grid(W, H, max_w, max_h, &g->fw, &g->fh);
            OFPS_REQUIRE(ctx, g->fw >= 1 && g->fh >= 1, "dense decoder: the capped grid of %dx%d under (%d, %d) is empty", W, H, max_w, max_h);
        }
        const int rc_klt = ofps::klt_check_call(ctx, g->fw, g->fh, g->fw, levels, radius, iters, who);       // the frames the tracker reads, rows dense
        if (rc_klt != OFPS_HIP_OK) return rc_klt;
        const ofps::KltLattice lat = ofps::klt_lattice(g->fw, g->fh, ctx->opt.klt_cell);
        g->gw = lat.nx; g->gh = lat.ny;
        g->max_records = lat.slots();
        g->frontend = g->reduced || g->fmt != OFPS_HIP_FMT_LUMA;
        g->raw_row = ((size_t)W * g->cn + 3) & ~(size_t)3;
        return OFPS_HIP_OK;
    }
    OFPS_REQUIRE(ctx, !g->use_previous || g->farneback, "OFPS_HIP_FLOW_USE_PREVIOUS without OFPS_HIP_FLOW_FARNEBACK (the iterative LK has no initial flow across pairs)");
    OFPS_REQUIRE(ctx, !(g->reduced && fullres_records), "OFPS_HIP_LK_REDUCED with OFPS_HIP_LK_FULLRES_RECORDS: the reduced mode has no full-resolution flow");
    OFPS_REQUIRE(ctx, stride >= W * g->cn, "dense decoder: stride %d < %d bytes per row (%d x %d channels)", stride, W * g->cn, W, g->cn);
    int gw = 0, gh = 0;
    ofps::cv_grid(W, H, max_w, max_h, &gw, &gh);            // cv-decoder/src/lib.rs:98-121 with aspect_ratio_scale = (1, 1)
    g->per_pixel = fullres_records || g->reduced;
    if (g->reduced) OFPS_REQUIRE(ctx, gw >= 1 && gh >= 1, "dense decoder: the capped grid of %dx%d under (%d, %d) is empty", W, H, max_w, max_h);
    else if (!fullres_records) OFPS_REQUIRE(ctx, gw >= 1 && gh >= 1 && (size_t)gw * gh <= 65536, "lk_decode: field %dx%d unsupported", gw, gh);
    g->fw = g->reduced ? gw : W; g->fh = g->reduced ? gh : H;
    g->gw = fullres_records ? W : gw; g->gh = fullres_records ? H : gh;
    g->max_records = (size_t)g->gw * g->gh;
    g->frontend = g->reduced || g->fmt != OFPS_HIP_FMT_LUMA;
    g->raw_row = ((size_t)W * g->cn + 3) & ~(size_t)3;
    // The flow's own parameter limits, checked where a stream's FIRST frame is pushed (it runs no flow) and before any upload: a stream must not
    // accept a frame and then fail every later one.  Farneback: winsize = 2 radius + 1 <= 15, and the layers of the fw x fh frames.
    // (Farneback's levels count the layers ABOVE the frame and its window is 2 radius + 1: 0 is a value of both -- the frame alone, the pixel alone)
    const int lowest = g->farneback ? 0 : 1;
    OFPS_REQUIRE(ctx, levels >= lowest && levels <= 8 && radius >= lowest && radius <= 15 && iters >= 1 && iters <= 64,
                 "%s: levels=%d radius=%d iters=%d out of range", who, levels, radius, iters);
    return g->farneback ? ofps::farneback_check_params(ctx, g->fw, g->fh, levels, 2 * radius + 1, 7) : OFPS_HIP_OK;
}

// the arriving frame (host memory) -> the fw x fh luma frame the flow reads, on stream `up`: a plain upload, or upload into `d_raw` + front-end
int dense_upload_frame(ofps_hip_ctx* ctx, const DenseGrid& g, const uint8_t* frame, int W, int H, int stride, uint8_t* d_raw, uint8_t* d_dst, hipStream_t up) {
    if (!g.frontend) {
        OFPS_HIP_TRY(ctx, ofps::upload_rows(d_dst, W, frame, stride, W, H, up));
        return OFPS_HIP_OK;
    }
    // A strongly reduced frame needs two of every H / fh source rows (168 of 1080 at the default cap): when the caller's frame is page-locked
    // -- device-addressable -- the front-end gathers them straight from host memory (~1 MB over PCIe instead of the 6.2 MB of a 1080p BGR
    // frame; the pixels of a row are 38 bytes apart, so the touched rows cross whole) and nothing is staged.  The frame must stay valid until
    // the ticket is collected, which the read-ahead form asks for anyway (include/ofps_hip.h).
    void* mapped = nullptr;
    if (g.reduced && g.fh * 3 <= H && ofps::device_address_of(frame, &mapped))
        return ofps::frontend_device(ctx, static_cast<const uint8_t*>(mapped), W, H, stride, g.fmt, true, d_dst, g.fw, g.fh, up);
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_raw, g.raw_row, frame, stride, (size_t)W * g.cn, H, up));
    return ofps::frontend_device(ctx, d_raw, W, H, (int)g.raw_row, g.fmt, true, d_dst, g.fw, g.fh, up);
}

// records 0 .. *d_count - 1 (or n_max when d_count is null) to a device-addressable destination, the count to cnt_dst
__global__ __launch_bounds__(256) void dense_copy_records_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                              const uint32_t* __restrict__ d_count, size_t n_max, uint32_t* __restrict__ cnt_dst) {
    size_t n = d_count ? (size_t)*d_count : n_max;
    if (n > n_max) n = n_max;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
    if (cnt_dst && blockIdx.x == 0 && threadIdx.x == 0) *cnt_dst = (uint32_t)n;
}

// One pair of a process_frame, as dense_enqueue_frame takes it
struct DenseFrameCall {
    const uint8_t* d_prev; const uint8_t* d_cur;      // the fw x fh frames on the device, rows dense
    uint64_t prev_id, cur_id;                         // the stream's frame ids (farneback.hip, OFPS_HIP_FLOW_USE_PREVIOUS); 0: a pair outside a stream
    int W, H;
    int levels, radius, iters;
    const DenseGrid& g;
    float4* rec_dst; uint32_t* cnt_dst;               // device scratch, or the device address of a page-locked block
    bool in_place;                                    // fused form: the caller reads the records where they lie -- a compaction's own output is not copied to rec_dst at all
    const uint8_t* d_mask_ready;                      // stream forms: the mask made ahead on the upload's stream, or null
    int* klt_slots; const int* klt_prev_slots;        // N3p: the pair's raw slots are kept in klt_slots, its tracks start from klt_prev_slots' flow
};
// ... and what it answers: where the records and their count lie in DEVICE memory -- rec_dst / cnt_dst, or (in_place) the compaction's own output
struct DenseRecords {
    int rc; const float4* rec; const uint32_t* cnt;
    DenseRecords(int rc_, const float4* rec_ = nullptr, const uint32_t* cnt_ = nullptr) : rc(rc_), rec(rec_), cnt(cnt_) {}
};

// Enqueues everything of a process_frame that follows the uploads on ctx->stream: flow [-> contrast mask] -> output stage.
// The record count lands at cnt_dst and the records at rec_dst -- device scratch, or the device address of a page-locked
// block (the kernels store there directly: no read-back launch of their own).
DenseRecords dense_enqueue_frame(ofps_hip_ctx* ctx, const DenseFrameCall& c) {
    const auto [d_prev, d_cur, prev_id, cur_id, W, H, levels, radius, iters, g, rec_dst, cnt_dst, in_place, d_mask_ready, klt_slots, klt_prev_slots] = c;
    // hip_klt: features, pyramid, track, flags, the ordered compaction and the count, straight to rec_dst / cnt_dst
    if (g.sparse) return {ofps::klt_flow_device(ctx, d_prev, d_cur, W, H, W, levels, radius, iters, rec_dst, cnt_dst, klt_slots, klt_prev_slots), rec_dst, cnt_dst};
    const size_t px = (size_t)W * H, cells = g.per_pixel ? 1 : (size_t)g.gw * g.gh;
    auto* d_ent = static_cast<float4*>(ofps::scratch(ctx, ofps::S_ENTRIES, px * sizeof(float4)));
    auto* d_field = static_cast<float2*>(ofps::scratch(ctx, ofps::S_FIELD, cells * sizeof(float2)));
    auto* d_cnt = static_cast<uint32_t*>(ofps::scratch(ctx, ofps::S_RESULT, 16));
    if (!d_ent || !d_field || !d_cnt) return OFPS_HIP_ENOMEM;
    int rc;
    if (g.farneback) {
        // cv-decoder's call (cv-decoder/src/lib.rs:188-199): levels = pyramid levels, winsize = 2 * radius + 1, iters = iterations,
        // poly_n 7, poly_sigma 1.5.  prev_id / cur_id: the
        // stream's frame ids -- the first frame's pyramid + expansion are the previous call's (farneback.hip)
        // OFPS_HIP_FLOW_USE_PREVIOUS: the flow of the pair that ended with this pair's first frame is the initial flow, and this pair's flow is
        // kept for the next one (read by the coarsest layer's first kernel, written by the last kernel of the call: one buffer)
        float2* d_keep = nullptr;
        const float2* d_init = nullptr;
        ofps::FarnebackState::PrevFlow& pf = ctx->fb.prev_flow;
        if (g.use_previous && cur_id != 0) {
            d_keep = static_cast<float2*>(ofps::scratch(ctx, ofps::S_FB_FLOW, px * sizeof(float2)));
            if (!d_keep) return OFPS_HIP_ENOMEM;
            // (the stream's LAST flow, whichever frames it related: cv-decoder's self.flow persists across skipped reads, cv-decoder/src/lib.rs:161-165;
            // ofps_hip_lk_reset and a geometry change forget it, ofps_hip_lk_rewind does not)
            if (pf.valid && pf.W == W && pf.H == H && pf.gen == ctx->scratch[ofps::S_FB_FLOW].gen) d_init = d_keep;
        }
        if (d_keep) pf.valid = false;               // (until this call has enqueued everything; a call that keeps nothing leaves the buffer alone)
        rc = ofps::farneback_flow_device(ctx, d_prev, d_cur, W, H, W, levels, 2 * radius + 1, iters, 7, 1.5, d_init, d_keep, d_ent, prev_id, cur_id);
        if (rc != OFPS_HIP_OK) return rc;
        if (d_keep) { pf.valid = true; pf.id = cur_id; pf.W = W; pf.H = H; pf.gen = ctx->scratch[ofps::S_FB_FLOW].gen; }
    } else {
        rc = ofps::lk_flow_device(ctx, d_prev, d_cur, W, H, W, levels, radius, iters, nullptr, d_ent, nullptr);
        if (rc != OFPS_HIP_OK) return rc;
    }
    const uint8_t* d_mask = d_mask_ready;          // (stream forms: made on the upload's stream already, beside the previous pair's flow)
    if (g.use_mask && !d_mask) {
        auto* m = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_MASK, px));
        if (!m) return OFPS_HIP_ENOMEM;
        rc = ofps::contrast_mask_device(ctx, d_cur, W, H, W, m);
        if (rc != OFPS_HIP_OK) return rc;
        d_mask = m;
    }
    if (g.per_pixel) {
        const float4* d_rec = d_ent;
        const uint32_t* d_n = nullptr;
        if (g.use_mask && px <= ofps::kCompactSmallMax)      // a reduced frame's records: one single-workgroup launch, straight into the block
            return {ofps::compact_small_device(ctx, d_ent, d_mask, px, rec_dst, cnt_dst), rec_dst, cnt_dst};
        if (g.use_mask) {                                  // the masked records themselves: order-preserving compaction
            auto* d_ent2 = static_cast<float4*>(ofps::scratch(ctx, ofps::S_ENTRIES2, px * sizeof(float4)));
            if (!d_ent2) return OFPS_HIP_ENOMEM;
            rc = ofps::compact_entries_device(ctx, d_ent, d_mask, px, d_ent2, d_cnt + 1);
            if (rc != OFPS_HIP_OK) return rc;
            d_rec = d_ent2; d_n = d_cnt + 1;
            if (in_place) return {OFPS_HIP_OK, d_ent2, d_cnt + 1};      // (the caller's one copy fills the block from here)
        }
        hipLaunchKernelGGL(dense_copy_records_kernel, dim3(1024), dim3(256), 0, ctx->stream, d_rec, rec_dst, d_n, px, cnt_dst);
        OFPS_HIP_TRY(ctx, hipGetLastError());
        return {OFPS_HIP_OK, rec_dst, cnt_dst};
    }
    // down-sampled output (cv-decoder/src/lib.rs:244-291): the records are this call's own per-pixel lattice, so the
    // densifier walks each cell's rectangle of pixels (masked ones skipped in place) instead of sorting 2 M records
    return {ofps::densify_raster_entries_device(ctx, d_ent, d_mask, W, H, g.gw, g.gh, d_field, rec_dst, cnt_dst), rec_dst, cnt_dst};
}

// count + records of a finished block -> the caller's buffer
void dense_collect(void* pinned, size_t max_records, float* out_entries, size_t* n_out) {
    const ofps::DenseBlock blk{max_records, false, 0};
    char* base = static_cast<char*>(pinned);
    uint32_t cnt = 0;
    memcpy(&cnt, blk.count(base), sizeof(cnt));
    if (cnt > max_records) cnt = (uint32_t)max_records;
    if (cnt) memcpy(out_entries, blk.records(base), (size_t)cnt * sizeof(float4));
    *n_out = cnt;
}

int dense_stream_setup(ofps_hip_ctx* ctx) {
    ofps::DenseStream& ds = ctx->dense;
    if (ds.copy_stream) return OFPS_HIP_OK;
    OFPS_HIP_TRY(ctx, hipStreamCreateWithFlags(&ds.copy_stream, hipStreamNonBlocking));
    for (auto& t : ds.ring.entry) {
        OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&t.done, hipEventDisableTiming));
        OFPS_HIP_TRY(ctx, hipEventCreateWithFlags(&t.uploaded, hipEventDisableTiming));
    }
    return OFPS_HIP_OK;
}

// waits for every ticket in flight and forgets the stream position (reset / geometry change / reallocation of the ring)
int dense_stream_drain(ofps_hip_ctx* ctx) {
    OFPS_HIP_TRY(ctx, ctx->dense.ring.drain());
    OFPS_HIP_TRY(ctx, ctx->dense.sync_side_streams());
    ctx->dense.frames = 0;
    ctx->dense.klt_pred.valid = false;
    return OFPS_HIP_OK;
}

// One dense_push call, step by step: claim -> reserve -> upload -> [decode -> tail] -> commit, the names of pipeline.hip's Push and BatchPush.
// Every step enqueues or returns an error; none touches the ring (commit does, last), and none but commit writes the ticket, with one exception
// where it always was: t.isl, armed at the end of upload() in front of the tail that takes it.  claim() refuses before anything is uploaded.
// There is no read_back step: the kernels store into the ticket's block (its device address), the fused form's copy launch included.
// prm == nullptr: ofps_hip_lk_push_frame_async, the records go straight to the ticket's block.
// prm != nullptr: ofps_hip_lk_push_frame_fused_async -- the records and their count are kept in device memory (S_DENSE_REC), copied to
// the block from there, and the detector and / or the estimator run on them behind the decoder, the count staying on the device.
// Everything of a ticket is enqueued on the compute stream: ticket k's tail has read the records (and detect_device's / almeida's workspaces
// are free again) before ticket k + 1's output stage writes them -- stream order is the join, no per-ticket copy of the tail's inputs.
struct DensePush {
    ofps_hip_ctx* ctx;
    const uint8_t* frame; int W, H, stride, levels, radius, iters, max_w, max_h; unsigned flags;
    const ofps_hip_frame_params* prm; int dim;           // dim: the detector's field, 0 when it does not run
    const char* who;
    static constexpr int kSlots = ofps::DenseStream::kSlots, kTickets = ofps::DenseStream::kTickets;
    ofps::DenseStream& ds = ctx->dense;
    hipStream_t s = ctx->stream;
    const long tno = ds.ring.next;
    ofps::DenseStream::Ticket& t = ds.ring.at(tno);
    DenseGrid g;
    size_t px = 0, raw_bytes = 0;        // the ring holds the frames the flow reads (reduced / converted)
    bool other_pending = false;
    uint8_t* d_frames = nullptr; uint8_t* d_raw_all = nullptr;
    int slot = 0;
    const uint8_t* d_mask_ready = nullptr;
    long frames_after = 0;
    ofps::DenseBlock blk{0, false, 0};   // the ticket's block ...
    char* base = nullptr;                // ... and its device address
    const float4* d_rec = nullptr;       // the records and their count in device memory: what the fused form's copy and tail read
    const uint32_t* d_cnt = nullptr;

    int claim() {
        // (a stream's first frame runs no flow: the flow's parameters -- Farneback's own limits included -- are refused here, not one frame later)
        int rc = dense_grid_of(ctx, W, H, stride, max_w, max_h, flags, levels, radius, iters, who, &g);
        if (rc != OFPS_HIP_OK) return rc;
        OFPS_REQUIRE(ctx, !t.pending, "%s: ticket %ld has not been collected (at most %d frames in flight)", who,
                     tno - kTickets, kTickets);
        px = (size_t)g.fw * g.fh; raw_bytes = g.raw_row * (size_t)H;
        // A new geometry restarts the stream and may reallocate the ring.  With a ticket in flight that would throw its records away
        // (draining marks it collected: the caller's later lk_frame_wait would fail with "already collected"): refused, like the
        // multi-device form does -- collect first, or ofps_hip_lk_reset.
        other_pending = ds.ring.other_pending();
        // (so does a change of the front-end -- "Process Fullres" flipped, another pixel format: the ring's frames are the other mode's; cv-decoder
        // returns Ok(false) for that frame because gray and old_gray differ in size, cv-decoder/src/lib.rs:156-158)
        const bool restart = ds.w != W || ds.h != H || ds.fw != g.fw || ds.fh != g.fh || ds.fmt != g.fmt ||
                             ctx->scratch[ofps::S_LK_FRAMES].cap < kSlots * px ||
                             (g.frontend && ctx->scratch[ofps::S_FE_RAW].cap < kTickets * raw_bytes);
        OFPS_REQUIRE(ctx, !(restart && other_pending), "%s: geometry change %dx%d -> %dx%d with a ticket in flight "
                     "(collect it with ofps_hip_lk_frame_wait first)", who, ds.w, ds.h, W, H);
        // hip_flow expands a new frame ahead of its pair, into the plane slot of the oldest frame of THIS parameter set: other Farneback parameters
        // re-plan the workspace (other layers), which a flow still in flight would be reading -- refused like a geometry change
        const bool fb_params_changed = g.farneback && ds.fb_params_valid && (ds.fb_levels != levels || ds.fb_radius != radius);
        OFPS_REQUIRE(ctx, !(fb_params_changed && other_pending), "%s: Farneback parameters changed (levels %d -> %d, radius %d -> %d) with a "
                     "ticket in flight (collect it with ofps_hip_lk_frame_wait first)", who, ds.fb_levels, levels, ds.fb_radius, radius);
        if (g.farneback) { ds.fb_params_valid = true; ds.fb_levels = levels; ds.fb_radius = radius; }
        if (restart) {
            rc = dense_stream_drain(ctx);
            if (rc != OFPS_HIP_OK) return rc;
            ds.w = W; ds.h = H; ds.fw = g.fw; ds.fh = g.fh; ds.fmt = g.fmt;
            ctx->fb.prev_flow.valid = false;
        }
        return OFPS_HIP_OK;
    }

    // only these two scratch() calls: a reallocation synchronises, so none may move across an enqueue
    int reserve() {
        // the stream's frames have slots of their own: no other entry point (lk_decode, lk_flow, sad_flow, contrast_mask stage
        // their frames in S_FRAMES) can overwrite or reallocate a previous frame behind the stream's back.  Three slots: frame
        // k + 1 is uploaded (copy stream) into the slot of frame k - 2, whose last reader -- ticket k - 1 -- has been collected
        // by the time a third push is accepted.
        d_frames = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_LK_FRAMES, kSlots * px));
        // the arriving frame of a stream with a front-end is staged per ticket in flight (the ticket's upload + front-end run on one stream; the
        // buffer's previous user, ticket tno - 2, has been collected)
        d_raw_all = g.frontend ? static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FE_RAW, kTickets * raw_bytes)) : nullptr;
        if (!d_frames || (g.frontend && !d_raw_all)) return OFPS_HIP_ENOMEM;
        if (ds.frames_gen != ctx->scratch[ofps::S_LK_FRAMES].gen) {         // (re)allocated: whatever was there is gone
            ds.frames_gen = ctx->scratch[ofps::S_LK_FRAMES].gen;
            ds.frames = 0;
        }
        return OFPS_HIP_OK;
    }

    int upload() {
        // with another ticket in flight the upload goes to the copy stream and overlaps that ticket's flow; a lone frame is
        // copied on the compute stream itself (no cross-stream event on the latency path of the synchronous call)
        const bool overlap = other_pending;
        slot = (int)(ds.frames % kSlots);
        hipStream_t up = overlap ? ds.copy_stream : s;
        ds.slot_id[slot] = ++ds.frame_serial;               // (a new id for whatever is in the slot now, also if the push fails below)
        int rc = dense_upload_frame(ctx, g, frame, W, H, stride, d_raw_all ? d_raw_all + (size_t)(tno % kTickets) * raw_bytes : nullptr,
                                    d_frames + (size_t)slot * px, up);
        if (rc != OFPS_HIP_OK) return rc;
        // cv-decoder's contrast mask depends on the new frame only: it is made right behind the upload, on the upload's stream -- with
        // another ticket in flight that is beside that ticket's flow instead of after this one's (one mask buffer per ticket in flight)
        if (g.use_mask && ds.frames + 1 >= 2) {
            auto* masks = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_LK_MASKS, (size_t)kTickets * px));
            if (!masks) return OFPS_HIP_ENOMEM;
            uint8_t* m = masks + (size_t)(tno % kTickets) * px;
            rc = ofps::contrast_mask_device(ctx, d_frames + (size_t)slot * px, g.fw, g.fh, g.fw, m, up);
            if (rc != OFPS_HIP_OK) return rc;
            d_mask_ready = m;
        }
        // hip_flow: the new frame's pyramid + polynomial expansion depend on that frame only, like the mask: made here, behind the upload on the
        // upload's stream -- with another ticket in flight beside that ticket's flow, whose coarse layers (a chain of dependent round trips) leave
        // most of the device idle (farneback.hip: farneback_prepare_device; the pair's flow below finds the planes by the frame's id)
        if (g.farneback && ctx->opt.fb_prepare_ahead) {
            rc = ofps::farneback_prepare_device(ctx, d_frames + (size_t)slot * px, g.fw, g.fh, g.fw, levels, 2 * radius + 1, 7, 1.5, ds.slot_id[slot], up);
            if (rc != OFPS_HIP_OK) return rc;
        }
        if (overlap) {
            OFPS_HIP_TRY(ctx, hipEventRecord(t.uploaded, up));
            OFPS_HIP_TRY(ctx, hipStreamWaitEvent(s, t.uploaded, 0));       // everything of this ticket on the compute stream comes after the upload
            if (g.farneback) ofps::farneback_mark_ordered(ctx, s);         // ... the new frame's pyramid + expansion included
        }
        // the stream position and the ticket change only once everything is enqueued: a failure below leaves both as they were (the
        // frame's slot is simply uploaded again by the next push) -- ADVICE r4
        frames_after = ds.frames + 1;
        // ... but for what holds whether or not a pair follows, the ticket's islands
        if (prm) ofps::islands_ticket_arm(ctx, &t.isl, prm, 1, ofps::TRK_DENSE, /*restart=*/frames_after < 2);     // A5i, A5t: the ticket follows the context's max_islands and max_tracks at this push
        else t.isl.K = 0;
        return OFPS_HIP_OK;
    }

    // the pair (frame k - 1, frame k) -> the records and their count in the ticket's block; fused: in device memory (d_rec, d_cnt) and from there,
    // by one copy launch in front of the tail, in the block
    int decode() {
        blk = {g.max_records, prm != nullptr, dim};
        int rc = ofps::host_block_reserve(ctx, &t.pinned, &t.pinned_cap, blk.bytes());
        if (rc != OFPS_HIP_OK) return rc;
        void* mapped = nullptr;
        OFPS_REQUIRE(ctx, ofps::device_address_of(t.pinned, &mapped), "%s: page-locked block is not device-addressable", who);
        base = static_cast<char*>(mapped);
        const int prev_slot = (int)((frames_after - 2) % kSlots);
        float4* rec_dst = blk.records(base);
        uint32_t* cnt_dst = blk.count(base);
        if (prm) {
            // the tail reads records and count from DEVICE memory, not back over PCIe: the output stage stores there, and one copy kernel
            // (bounded by the count it reads on the device) fills the block
            const ofps::DenseBlock dev{g.max_records, false, 0};
            char* d_rec_blk = static_cast<char*>(ofps::scratch(ctx, ofps::S_DENSE_REC, dev.bytes()));
            if (!d_rec_blk) return OFPS_HIP_ENOMEM;
            rec_dst = dev.records(d_rec_blk);
            cnt_dst = dev.count(d_rec_blk);
        }
        // N3p: with the setting on the stream keeps each pair's raw slots, two buffers that alternate by pair (per stream, not per ticket: the
        // track launches of two tickets in flight run on the one compute stream, in order).  Pair k reads pair k - 1's if that pair wrote them
        // on this lattice under these flags; a pair pushed with the setting off writes none, so its successor starts from zero
        ofps::DenseStream::KltPred& kp = ds.klt_pred;
        int* klt_slots = nullptr;
        const int* klt_prev_slots = nullptr;
        const bool predict = g.sparse && ctx->opt.klt_prediction;
        if (predict) {
            const size_t half = (g.max_records * 6 * sizeof(int) + 255) & ~(size_t)255;
            auto* d_pred = static_cast<char*>(ofps::scratch(ctx, ofps::S_KLT_PRED, 2 * half));
            if (!d_pred) return OFPS_HIP_ENOMEM;
            const uint64_t gen = ctx->scratch[ofps::S_KLT_PRED].gen;
            if (kp.valid && kp.pair == frames_after - 1 && kp.fw == g.fw && kp.fh == g.fh && kp.cell == ctx->opt.klt_cell && kp.flags == flags && kp.gen == gen)
                klt_prev_slots = reinterpret_cast<const int*>(d_pred + (size_t)(kp.pair & 1) * half);
            klt_slots = reinterpret_cast<int*>(d_pred + (size_t)(frames_after & 1) * half);
        }
        kp.valid = false;                                    // (until this pair has enqueued everything)
        const DenseRecords at = dense_enqueue_frame(ctx, {d_frames + (size_t)prev_slot * px, d_frames + (size_t)slot * px, ds.slot_id[prev_slot], ds.slot_id[slot],
                                                          g.fw, g.fh, levels, radius, iters, g, rec_dst, cnt_dst, /*in_place=*/prm != nullptr, d_mask_ready,
                                                          klt_slots, klt_prev_slots});
        if (at.rc != OFPS_HIP_OK) return at.rc;
        if (predict) kp = {true, frames_after, g.fw, g.fh, ctx->opt.klt_cell, flags, ctx->scratch[ofps::S_KLT_PRED].gen};
        d_rec = at.rec; d_cnt = at.cnt;
        if (prm) {
            const unsigned copy_blocks = (unsigned)((g.max_records + 255) / 256 < 1024 ? (g.max_records + 255) / 256 : 1024);
            hipLaunchKernelGGL(dense_copy_records_kernel, dim3(copy_blocks ? copy_blocks : 1), dim3(256), 0, s, d_rec,
                               blk.records(base), d_cnt, g.max_records, blk.count(base));
            OFPS_HIP_TRY(ctx, hipGetLastError());
        }
        return OFPS_HIP_OK;
    }

    // the 32 bytes the caller waits for -- island result, quaternion -- and the island's field are stored by the detector's and the
    // estimator's last kernels straight into the ticket's block, as pipeline.hip does.  The tail (tail.hip) in its device-count form,
    // sized from the capacity, on this one stream; with detect-compensation 1 its detector reads compensated records in a slot of
    // their own: d_rec is what decode()'s copy reads
    int tail() {
        return ofps::frame_tail_device(ctx, d_rec, g.max_records, 1, d_cnt, /*lsq_min_n=*/0, prm, prm->seed, /*may_compensate=*/true,
                                       blk.result(base), blk.quat(base), blk.field(base), nullptr, nullptr, &t.isl);
    }

    int commit(int* ticket) {
        OFPS_HIP_TRY(ctx, hipEventRecord(t.done, s));
        ds.frames = frames_after;
        t.have_vectors = frames_after >= 2; t.gw = g.gw; t.gh = g.gh; t.max_records = g.max_records;       // cv-decoder/src/lib.rs:156-158: flow needs two frames
        t.fused = prm ? 1 : 0; t.run_detector = prm ? prm->run_detector : 0; t.run_estimator = prm ? prm->run_estimator : 0;
        t.dim = dim;
        *ticket = ds.ring.commit();
        return OFPS_HIP_OK;
    }
};

// One frame of the dense decoders' stream, ofps_hip_lk_push_frame[_fused][_async]: the refusals that need no stream, then DensePush's steps
int dense_push(ofps_hip_ctx* ctx, const uint8_t* frame, int W, int H, int stride, int levels, int radius, int iters, int max_w, int max_h,
               unsigned flags, const ofps_hip_frame_params* tail, int* ticket, const char* who) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, frame && ticket, "%s: null pointer", who);
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1 && dense_cap_ok(flags, max_w, max_h), "%s: bad geometry", who);
    OFPS_REQUIRE(ctx, (flags & ~kDenseFlagBits) == 0, "%s: unknown flags 0x%x", who, flags);
    if (const int rc_sparse = dense_sparse_flags(ctx, flags, who)) return rc_sparse;
    int dim = 0;
    if (tail) {
        // refused before anything is uploaded, the stream's first frame (which runs no tail) included
        if (flags & OFPS_HIP_LK_FULLRES_RECORDS)
            return ofps::set_error(ctx, OFPS_HIP_EUNSUPPORTED, "%s: OFPS_HIP_LK_FULLRES_RECORDS has no fused form (ofps_hip_lk_flow_dev -> "
                                   "ofps_hip_almeida_dev / ofps_hip_densify_raster_dev is that chain, with a count the host knows)", who);
        if (tail->run_detector) {
            dim = ofps_hip_block_dim(tail->min_size, tail->subdivide);
            OFPS_REQUIRE(ctx, dim >= 1 && dim <= ofps::kMaxDetectDim, "%s: detector block_dim %d outside [1,160] (min_size=%g subdivide=%zu)", who, dim,
                         (double)tail->min_size, tail->subdivide);
        }
        if (tail->run_estimator) {
            OFPS_REQUIRE(ctx, tail->aspect > 0.0f && tail->fov_y_deg > 0.0f && tail->fov_y_deg < 180.0f, "%s: bad camera (aspect=%g fov_y=%g)", who,
                         (double)tail->aspect, (double)tail->fov_y_deg);
            OFPS_REQUIRE(ctx, !tail->use_ransac || (tail->num_iters >= 1 && tail->num_iters <= 65535 && tail->num_samples >= 1),
                         "%s: ransac iters %zu / samples %zu out of range", who, tail->num_iters, tail->num_samples);
        }
    }
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = dense_stream_setup(ctx);
    if (rc != OFPS_HIP_OK) return rc;
    DensePush p{ctx, frame, W, H, stride, levels, radius, iters, max_w, max_h, flags, tail, dim, who};
    rc = p.claim();                                     // refused before anything is uploaded
    if (rc == OFPS_HIP_OK) rc = p.reserve();
    if (rc == OFPS_HIP_OK) rc = p.upload();
    if (rc == OFPS_HIP_OK && p.frames_after >= 2) {     // cv-decoder/src/lib.rs:156-158: flow needs two frames
        rc = p.decode();
        if (rc == OFPS_HIP_OK && tail) rc = p.tail();
    }
    return rc == OFPS_HIP_OK ? p.commit(ticket) : rc;
}

}  // namespace

extern "C" {

int ofps_hip_lk_decode(ofps_hip_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int W, int H, int stride, int levels,
                       int radius, int iters, int max_w, int max_h, unsigned flags, float* out_entries, size_t* n_out,
                       int* out_w, int* out_h) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, prev && cur && out_entries && n_out, "lk_decode: null host pointer");
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1 && dense_cap_ok(flags, max_w, max_h), "lk_decode: bad geometry");
    OFPS_REQUIRE(ctx, (flags & ~kDenseFlagBits) == 0, "lk_decode: unknown flags 0x%x", flags);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    DenseGrid g;
    int rc = dense_grid_of(ctx, W, H, stride, max_w, max_h, flags, levels, radius, iters, "lk_decode", &g);
    if (rc != OFPS_HIP_OK) return rc;
    const size_t px = (size_t)g.fw * g.fh, raw_bytes = g.raw_row * (size_t)H;
    auto* d_frames = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, 2 * px));
    auto* d_raw = g.frontend ? static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FE_RAW_PAIR, 2 * raw_bytes)) : nullptr;
    if (!d_frames || (g.frontend && !d_raw)) return OFPS_HIP_ENOMEM;
    rc = dense_upload_frame(ctx, g, prev, W, H, stride, d_raw, d_frames, ctx->stream);
    if (rc != OFPS_HIP_OK) return rc;
    rc = dense_upload_frame(ctx, g, cur, W, H, stride, d_raw ? d_raw + raw_bytes : nullptr, d_frames + px, ctx->stream);
    if (rc != OFPS_HIP_OK) return rc;
    // the count and the records come back in ONE page-locked block and one wait; only the visited cells' records reach the
    // caller's buffer
    const ofps::DenseBlock blk{g.max_records, false, 0};
    rc = ofps::host_block_reserve(ctx, &ctx->dense.decode_pinned, &ctx->dense.decode_pinned_cap, blk.bytes());
    if (rc != OFPS_HIP_OK) return rc;
    void* mapped = nullptr;
    OFPS_REQUIRE(ctx, ofps::device_address_of(ctx->dense.decode_pinned, &mapped), "lk_decode: page-locked block is not device-addressable");
    char* base = static_cast<char*>(mapped);
    rc = dense_enqueue_frame(ctx, {d_frames, d_frames + px, 0, 0, g.fw, g.fh, levels, radius, iters, g, blk.records(base), blk.count(base), /*in_place=*/false,
                                   nullptr, nullptr, nullptr}).rc;
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    dense_collect(ctx->dense.decode_pinned, g.max_records, out_entries, n_out);
    if (out_w) *out_w = g.gw;
    if (out_h) *out_h = g.gh;
    return OFPS_HIP_OK;
}

int ofps_hip_lk_push_frame_async(ofps_hip_ctx* ctx, const uint8_t* frame, int W, int H, int stride, int levels, int radius, int iters,
                                 int max_w, int max_h, unsigned flags, int* ticket) {
    return dense_push(ctx, frame, W, H, stride, levels, radius, iters, max_w, max_h, flags, nullptr, ticket, "lk_push_frame_async");
}

int ofps_hip_lk_frame_wait(ofps_hip_ctx* ctx, int ticket, float* out_entries, size_t* n_out, int* out_w, int* out_h, int* have_vectors) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, out_entries && n_out && have_vectors, "lk_frame_wait: null pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto* t = ctx->dense.ring.claim(ctx, ticket, "lk_frame_wait", "has already been");
    if (!t) return OFPS_HIP_EINVAL;
    OFPS_HIP_TRY(ctx, hipEventSynchronize(t->done));
    t->pending = false;
    *n_out = 0;
    *have_vectors = t->have_vectors;
    if (out_w) *out_w = t->gw;
    if (out_h) *out_h = t->gh;
    if (t->have_vectors) dense_collect(t->pinned, t->max_records, out_entries, n_out);
    return OFPS_HIP_OK;
}

int ofps_hip_lk_push_frame(ofps_hip_ctx* ctx, const uint8_t* frame, int W, int H, int stride, int levels, int radius, int iters,
                           int max_w, int max_h, unsigned flags, float* out_entries, size_t* n_out, int* out_w, int* out_h,
                           int* have_vectors) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, frame && out_entries && n_out && have_vectors, "lk_push_frame: null host pointer");
    OFPS_REQUIRE(ctx, !ctx->dense.ring.any_pending(), "lk_push_frame: a read-ahead ticket is in flight (collect it with ofps_hip_lk_frame_wait first)");
    int ticket = 0;
    const int rc = ofps_hip_lk_push_frame_async(ctx, frame, W, H, stride, levels, radius, iters, max_w, max_h, flags, &ticket);
    if (rc != OFPS_HIP_OK) return rc;
    return ofps_hip_lk_frame_wait(ctx, ticket, out_entries, n_out, out_w, out_h, have_vectors);     // the caller may reuse `frame` right away
}

int ofps_hip_lk_push_frame_fused_async(ofps_hip_ctx* ctx, const uint8_t* frame, int W, int H, int stride, int levels, int radius, int iters,
                                       int max_w, int max_h, unsigned flags, const ofps_hip_frame_params* tail, int* ticket) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, tail, "lk_push_frame_fused_async: null parameters");
    return dense_push(ctx, frame, W, H, stride, levels, radius, iters, max_w, max_h, flags, tail, ticket, "lk_push_frame_fused_async");
}

int ofps_hip_lk_frame_fused_wait(ofps_hip_ctx* ctx, int ticket, ofps_hip_frame_result* out, float* out_entries, float* out_field, int* out_w,
                                 int* out_h) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, out, "lk_frame_fused_wait: null pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto* t = ctx->dense.ring.claim(ctx, ticket, "lk_frame_fused_wait", "has already been");
    if (!t) return OFPS_HIP_EINVAL;
    OFPS_HIP_TRY(ctx, hipEventSynchronize(t->done));
    t->pending = false;
    // identity / no motion: a stream's first frame, a plain ticket, a stage that did not run
    const ofps::DenseBlock blk{t->max_records, t->have_vectors && t->fused, t->dim};
    char* base = static_cast<char*>(t->pinned);
    uint32_t cnt = 0;
    if (t->have_vectors) memcpy(&cnt, blk.count(base), sizeof(cnt));
    if (cnt > t->max_records) cnt = (uint32_t)t->max_records;
    ofps::fill_frame_result(out, t->have_vectors, cnt, t->run_detector ? blk.result(base) : nullptr, t->run_estimator ? blk.quat(base) : nullptr);
    if (out_w) *out_w = t->gw;
    if (out_h) *out_h = t->gh;
    const int isl_rc = ofps::islands_collect(ctx, t->isl);             // (a plain ticket: none)
    if (isl_rc != OFPS_HIP_OK) return isl_rc;
    if (out_entries && cnt) memcpy(out_entries, blk.records(base), (size_t)cnt * sizeof(float4));
    if (blk.fused && t->run_detector && out_field) memcpy(out_field, blk.field(base), (size_t)t->dim * t->dim * sizeof(float2));
    return OFPS_HIP_OK;
}

int ofps_hip_lk_push_frame_fused(ofps_hip_ctx* ctx, const uint8_t* frame, int W, int H, int stride, int levels, int radius, int iters,
                                 int max_w, int max_h, unsigned flags, const ofps_hip_frame_params* tail, ofps_hip_frame_result* out,
                                 float* out_entries, float* out_field, int* out_w, int* out_h) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, frame && tail && out, "lk_push_frame_fused: null pointer");
    OFPS_REQUIRE(ctx, !ctx->dense.ring.any_pending(), "lk_push_frame_fused: a read-ahead ticket is in flight (collect it with ofps_hip_lk_frame_fused_wait first)");
    int ticket = 0;
    const int rc = dense_push(ctx, frame, W, H, stride, levels, radius, iters, max_w, max_h, flags, tail, &ticket, "lk_push_frame_fused");
    if (rc != OFPS_HIP_OK) return rc;
    return ofps_hip_lk_frame_fused_wait(ctx, ticket, out, out_entries, out_field, out_w, out_h);     // the caller may reuse `frame` right away
}

int ofps_hip_lk_reset(ofps_hip_ctx* ctx) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->fb.prev_flow.valid = false;                       // a new stream starts from zero flow, like a new CvDecoder
    ctx->trk[ofps::TRK_DENSE].live = false;                // ... and from no tracks (A5t)
    return dense_stream_drain(ctx);
}

int ofps_hip_lk_rewind(ofps_hip_ctx* ctx) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return dense_stream_drain(ctx);                           // the frames are forgotten, the kept flow (OFPS_HIP_FLOW_USE_PREVIOUS) is not
}

}  // extern "C"
