// camera.hpp -- StandardCamera::delta and the quaternion -> rotation-matrix code shared by the estimator (almeida.hip) and the
// compensation stage (compensate.hip).  Every function is pinned to the oracle's operation order (oracle/ofps_oracle.c:
// orc_camera_new, orc_camera_delta, orc_quat_to_homogeneous): no operation or order may change here.  Compiled with -ffp-contract=off.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace ofps {

struct Camera {            // same fields as the oracle's orc_camera (camera.rs:26-35)
    float aspect, fov_y;
    float m00, m11, m22, m23;
    float r00, r11, r32, r33;
};

static float to_radians_host(float deg) {
    const float k = 3.14159265358979323846264338327950288f / 180.0f;
    return deg * k;
}

static Camera camera_new(float aspect, float fov_y_deg) {   // Perspective3::new + inverse
    Camera c;
    const float zn = 0.1f, zf = 10.0f;
    const float fovy = to_radians_host(fov_y_deg);
    c.aspect = aspect; c.fov_y = fov_y_deg;
    c.m11 = 1.0f / tanf(fovy / 2.0f);
    c.m00 = c.m11 / aspect;
    c.m22 = (zf + zn) / (zn - zf);
    c.m23 = zf * zn * 2.0f / (zn - zf);
    c.r00 = 1.0f / c.m00;
    c.r11 = 1.0f / c.m11;
    c.r32 = 1.0f / c.m23;
    c.r33 = c.m22 * c.r32;
    return c;
}

struct Mat3 { float m[9]; };   // row-major 3x3 rotation

// camera.rs:115-117 (rotate - coords), closed form; see the header of almeida.hip.
__device__ __forceinline__ float2 cam_delta(const Camera& c, float px, float py, const Mat3& R) {
    const float cx = px * 2.0f - 1.0f, cy = py * 2.0f - 1.0f;
    const float n0 = c.r32 + c.r33;
    const float wx = ((-c.r00) * cx) / n0;
    const float wy = -1.0f / n0;
    const float wz = (c.r11 * cy) / n0;
    const float rx = (R.m[0] * wx + R.m[1] * wy) + R.m[2] * wz;
    const float ry = (R.m[3] * wx + R.m[4] * wy) + R.m[5] * wz;
    const float rz = (R.m[6] * wx + R.m[7] * wy) + R.m[8] * wz;
    const float qx = -rx, qy = rz, qz = ry;                   // view: (-x, z, y)
    const float inv = -1.0f / qz;
    const float sx = c.m00 * qx * inv;
    const float sy = c.m11 * qy * inv;
    const float sz = (c.m22 * qz + c.m23) * inv;
    const float ox = (sx / sz + 1.0f) * 0.5f;                 // camera.rs:77: divide by NDC z
    const float oy = (sy / sz + 1.0f) * 0.5f;
    return make_float2(ox - px, oy - py);
}

struct alignas(16) Quat { float w, i, j, k; };      // (16-byte aligned: one ds_read_b128 / global dwordx4 per quaternion)

__device__ __forceinline__ Mat3 quat_to_mat3(const Quat& q) {                    // to_homogeneous, 3x3 part
    const float w = q.w, i = q.i, j = q.j, k = q.k;
    const float ww = w * w, ii = i * i, jj = j * j, kk = k * k;
    const float ij = i * j * 2.0f, wk = w * k * 2.0f, wj = w * j * 2.0f;
    const float ik = i * k * 2.0f, jk = j * k * 2.0f, wi = w * i * 2.0f;
    Mat3 r;
    r.m[0] = ww + ii - jj - kk; r.m[1] = ij - wk;           r.m[2] = wj + ik;
    r.m[3] = wk + ij;           r.m[4] = ww - ii + jj - kk; r.m[5] = jk - wi;
    r.m[6] = ik - wj;           r.m[7] = wi + jk;           r.m[8] = ww - ii - jj + kk;
    return r;
}

// A wave-uniform matrix moved to scalar registers (v_readfirstlane): nine VGPRs less per matrix in kernels whose
// per-record state fills the register file; VALU instructions read the element as their scalar operand.
__device__ __forceinline__ Mat3 mat3_uniform(const Mat3& a) {
    Mat3 r;
#pragma unroll
    for (int k = 0; k < 9; ++k) r.m[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.m[k])));
    return r;
}

}  // namespace ofps
