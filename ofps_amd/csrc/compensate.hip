// compensate.hip -- camera compensation of motion records: what moves relative to the camera.
//
// The residual of the reference's RANSAC inlier test (almeida-estimator/src/lib.rs:224-231),
//     vec - camera.delta(pos, fit.inverse().to_homogeneous())          (ofps/src/camera.rs:115-117)
// as an OUTPUT: per record, in f32 without contraction,
//     M = to_homogeneous(inverse(q))      oracle/ofps_oracle.c: orc_quat_inverse, orc_quat_to_homogeneous
//     d = camera.delta(pos, M)            camera.hpp: cam_delta, the exact form pinned to the oracle's operation order
//     out.pos = pos (the same bits), out.motion = motion - d
// ONE regime: cam_delta with IEEE divisions at every record count (the estimator's reciprocal-quotient regime above 65,536
// records has no counterpart here), so a record's result does not depend on how many records there are.
//
// The quaternion is read from DEVICE memory -- the estimator's launch wrote it there, nothing is read back or synchronised in
// between -- one per item; the rotation matrix is formed once per workgroup, ahead of its loop, and kept in scalar registers.
// One record per lane: one 16-byte load, one 16-byte store, grid-stride.  In place (out == in) is fine: a lane reads its record
// before it writes it and touches no other.
//
// The fused per-frame entry points (pipeline.hip, dense_decoder.hip) run it between the estimator and the detector when the
// context's detect-compensation mode is 1 (ofps_hip_set_detect_compensation): the detector then answers for the compensated field.
#include "common.hpp"
#include "camera.hpp"

namespace ofps {

constexpr int kCompThreads = 256;
constexpr unsigned kCompMaxBlocks = 2048;        // per item; the loop strides over the rest

// n_dev != nullptr: the record counts live in device memory, one per item (the dense decoders' tail, the filtered SAD tails), n is the
// capacity the grid was sized from and the stride of every item.
// quat_echo != nullptr: the item's quaternion is also stored there (a ticket's page-locked result block: the estimator wrote to device
// memory so that this kernel reads it from there).
__global__ __launch_bounds__(kCompThreads) void compensate_kernel(const float4* in, size_t n, const uint32_t* __restrict__ n_dev, Camera cam,
                                                                  const float4* __restrict__ quat, float4* out, float4* __restrict__ quat_echo) {
    const size_t item = blockIdx.y;
    size_t cnt = n;
    if (n_dev) { const uint32_t c = n_dev[item]; cnt = c < n ? c : n; }
    const float4 qv = quat[item];                                        // (w, i, j, k)
    const Quat inv = {qv.x, -qv.y, -qv.z, -qv.w};                        // orc_quat_inverse
    const Mat3 M = mat3_uniform(quat_to_mat3(inv));                      // orc_quat_to_homogeneous, 3 x 3 part
    if (quat_echo && blockIdx.x == 0 && threadIdx.x == 0) quat_echo[item] = qv;
    const float4* src = in + item * n;
    float4* dst = out + item * n;
    const size_t step = (size_t)gridDim.x * kCompThreads;
    for (size_t i = (size_t)blockIdx.x * kCompThreads + threadIdx.x; i < cnt; i += step) {
        float4 e = src[i];
        const float2 d = cam_delta(cam, e.x, e.y, M);
        e.z = e.z - d.x;
        e.w = e.w - d.y;
        dst[i] = e;
    }
}

int compensate_device(ofps_hip_ctx* ctx, const float4* d_entries, size_t n, int batch, const uint32_t* d_n, float aspect, float fov_y_deg,
                      const float4* d_quat, float4* d_out, float4* d_quat_echo) {
    OFPS_REQUIRE(ctx, batch >= 1 && batch <= 65535, "compensate: batch %d out of range", batch);
    OFPS_REQUIRE(ctx, n < (1ull << 31), "compensate: too many entries");
    OFPS_REQUIRE(ctx, aspect > 0.0f && fov_y_deg > 0.0f && fov_y_deg < 180.0f, "compensate: bad camera (aspect=%g fov_y=%g)",
                 (double)aspect, (double)fov_y_deg);
    const Camera cam = camera_new(aspect, fov_y_deg);
    size_t blocks = (n + kCompThreads - 1) / kCompThreads;
    if (blocks > kCompMaxBlocks) blocks = kCompMaxBlocks;
    if (blocks < 1) blocks = 1;                                          // n == 0: one workgroup per item still echoes the quaternion
    hipLaunchKernelGGL(compensate_kernel, dim3((unsigned)blocks, (unsigned)batch), dim3(kCompThreads), 0, ctx->stream, d_entries, n, d_n, cam,
                       d_quat, d_out, d_quat_echo);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

}  // namespace ofps

extern "C" {

int ofps_hip_set_detect_compensation(ofps_hip_ctx* ctx, int mode) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, mode == 0 || mode == 1, "set_detect_compensation: %d is not 0 (raw vectors) or 1 (camera-compensated vectors)", mode);
    ctx->opt.detect_compensate = mode;
    return OFPS_HIP_OK;
}

int ofps_hip_get_detect_compensation(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.detect_compensate : OFPS_HIP_EINVAL; }

int ofps_hip_compensate_dev(ofps_hip_ctx* ctx, const void* d_entries, size_t n_per_item, int batch, float aspect, float fov_y_deg,
                            const void* d_quat, void* d_out_entries) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_quat && ((d_entries && d_out_entries) || n_per_item == 0), "compensate: null device pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::compensate_device(ctx, static_cast<const float4*>(d_entries), n_per_item, batch, nullptr, aspect, fov_y_deg,
                                   static_cast<const float4*>(d_quat), static_cast<float4*>(d_out_entries), nullptr);
}

int ofps_hip_compensate(ofps_hip_ctx* ctx, const float* entries, size_t n, float aspect, float fov_y_deg, const float quat[4],
                        float* out_entries) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, quat && ((entries && out_entries) || n == 0), "compensate: null host pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto* d_ent = static_cast<float4*>(ofps::scratch(ctx, ofps::S_ENTRIES, n * sizeof(float4)));
    auto* d_q = static_cast<float4*>(ofps::scratch(ctx, ofps::S_QUAT, sizeof(float4)));
    if (!d_ent || !d_q) return OFPS_HIP_ENOMEM;
    if (n) OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_ent, entries, n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_q, quat, sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    const int rc = ofps::compensate_device(ctx, d_ent, n, 1, nullptr, aspect, fov_y_deg, d_q, d_ent, nullptr);     // in place
    if (rc != OFPS_HIP_OK) return rc;
    if (n) OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_entries, d_ent, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

}  // extern "C"
