// tail.hip -- the tail of every fused entry point: estimator -> [compensation ->] detector on device-resident records, the results stored by
// the stages' last kernels where the caller says (a ticket's device-addressable block, or scratch it reads back).  The per-frame SAD path
// (pipeline.hip: one item, the count on the host or -- filtered -- on the device, the detector beside the estimator), its batched form
// (n items, their counts on the host or -- filtered -- one per item on the device; the multi-device workers among them) and the dense decoders' fused form (dense_decoder.hip: the count on the device) differ in
// the arguments alone.  No kernel lives here.
#include "common.hpp"

namespace ofps {

int frame_tail_device(ofps_hip_ctx* ctx, const float4* d_rec, size_t n, int batch, const uint32_t* d_n, uint32_t lsq_min_n,
                      const ofps_hip_frame_params* prm, uint64_t seed0, bool may_compensate, int* d_result, float4* d_quat, float2* d_field,
                      const TailSide* side, int* out_dim, IslandsTicket* isl) {
    const bool both = prm->run_detector && prm->run_estimator;
    // detect-compensation mode 1 (compensate.hip; the mode is the context's at this push): the detector reads the vectors compensated with the
    // frame's own quaternion, so its chain cannot run beside the estimator -- estimator, compensation and detector are enqueued on the compute
    // stream in that order.  The estimator writes the quaternions to the head of S_COMP; the compensation launch reads them there, passes
    // them on to d_quat and leaves the compensated records behind them: d_rec is what the caller hands out.
    const bool compensate = may_compensate && ctx->opt.detect_compensate == 1 && both;
    // detector and estimator read the same records and share no workspace: the detector's chain of small launches runs on the side stream.
    // The estimator is enqueued first: it is the long pole (0.1 ms of dependent steps), and whatever is enqueued second starts a host-enqueue
    // time later
    const bool fork = side && both && !compensate;
    hipStream_t s = ctx->stream;
    if (fork) {
        if (!side->recorded) OFPS_HIP_TRY(ctx, hipEventRecord(side->fork_on, s));
        OFPS_HIP_TRY(ctx, hipStreamWaitEvent(side->stream, side->fork_on, 0));
    }
    float4* d_comp = nullptr;
    if (compensate) {
        d_comp = static_cast<float4*>(scratch(ctx, S_COMP, (size_t)batch * (1 + n) * sizeof(float4)));
        if (!d_comp) return OFPS_HIP_ENOMEM;
    }
    float4* d_q = compensate ? d_comp : d_quat;
    int rc = OFPS_HIP_OK;
    // device-side counts: every launch is sized from the capacity n, the first d_n[j] records of item j count
    if (prm->run_estimator)
        rc = d_n ? almeida_device_n(ctx, d_rec, n, d_n, prm->aspect, prm->fov_y_deg, prm->use_ransac, prm->num_iters, prm->inlier_deg,
                                    prm->num_samples, seed0, d_q, lsq_min_n, batch)
                 : almeida_device(ctx, d_rec, n, batch, prm->aspect, prm->fov_y_deg, prm->use_ransac, prm->num_iters, prm->inlier_deg,
                                  prm->num_samples, seed0, d_q);
    if (rc == OFPS_HIP_OK && compensate) rc = compensate_device(ctx, d_rec, n, batch, d_n, prm->aspect, prm->fov_y_deg, d_q, d_comp + batch, d_quat);
    if (rc != OFPS_HIP_OK || !prm->run_detector) return rc;
    if (fork) ctx->stream = side->stream;                         // the stage entry points enqueue on ctx->stream
    int dim = 0;
    rc = detect_device(ctx, compensate ? d_comp + batch : d_rec, n, batch, prm->min_size, prm->subdivide, prm->target_motion, d_result, d_field,
                       &dim, d_n);
    if (out_dim) *out_dim = dim;
    // A5i: a ticket armed with max_islands > 0 lists the islands of the field the detector has just read, behind it on its stream: one launch
    // and one copy to the ticket's page-locked blocks, inside the fork.  Nothing here with max_islands 0
    if (rc == OFPS_HIP_OK && isl && isl->K > 0) rc = islands_ticket_device(ctx, batch, dim, prm->min_size, prm->target_motion, isl);
    ctx->stream = s;
    if (rc != OFPS_HIP_OK || !fork) return rc;
    OFPS_HIP_TRY(ctx, hipEventRecord(side->join, side->stream));
    OFPS_HIP_TRY(ctx, hipStreamWaitEvent(s, side->join, 0));
    return OFPS_HIP_OK;
}

}  // namespace ofps
