// transfer.hip -- host <-> device transfers of the streaming front doors (pipeline.hip, dense_decoder.hip, multi.hip): the copy kernels
// that stand in for the DMA engines where those get in each other's way, and the page-locked blocks kernels write results into.
#include "common.hpp"

namespace {
// Device -> page-locked host memory by a kernel (the destination is device-addressable) instead of hipMemcpyAsync: a
// D2H copy sits in the same in-order DMA queue as the NEXT frame's H2D and -- because it has to wait for this frame's
// search -- held that upload back until the search was over (rocprofv3 memory-copy trace, ROCm 7.2 runtime): no overlap
// at all.  The copy kernel runs on the compute stream, where it belongs.
__global__ __launch_bounds__(256) void copy_words_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, size_t n_words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

// Host -> device by a copy KERNEL reading the page-locked source over PCIe: the batched read-ahead form's upload (round 5).
// hipMemcpyAsync binds a stream to whichever SDMA engine is free at its first copy, and the engines are not equally fast for 33 MB copies:
// the batched form ran at 0.0385 ms per 1080p frame in most processes and 0.046 in the rest.  A 16-workgroup copy kernel on the copy stream
// sustains the link rate in every process (0.0389), leaves the CUs to the search beside it (64 workgroups: 0.043, 128: 0.046) and makes small
// batches faster.  The single-frame form keeps the DMA engine: a lone 2 MB frame is on the latency path and crosses faster that way (0.0545
// against 0.0628 / 0.0558 with 16 / 32 workgroups).  profiles/r05/batched_bimodal.txt; A/B builds: tools/upload_ab.sh (-DOFPS_HIP_UPLOAD_WGS=n).
#ifndef OFPS_HIP_UPLOAD_WGS
#define OFPS_HIP_UPLOAD_WGS 16
#endif
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void upload_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, size_t n16) {
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {                // four 16-byte reads in flight per lane
        const u32x4 a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + stride);
        const u32x4 c = __builtin_nontemporal_load(src + i + 2 * stride), d = __builtin_nontemporal_load(src + i + 3 * stride);
        dst[i] = a; dst[i + stride] = b; dst[i + 2 * stride] = c; dst[i + 3 * stride] = d;
    }
    for (; i < n16; i += stride) dst[i] = __builtin_nontemporal_load(src + i);
}

}  // namespace

namespace ofps {

bool device_address_of(const void* host_ptr, void** dev_ptr) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, host_ptr) != hipSuccess) { (void)hipGetLastError(); return false; }   // pageable memory
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return false;
    *dev_ptr = a.devicePointer;
    return true;
}

int upload_dense_device(ofps_hip_ctx* ctx, void* dst, const void* src, size_t bytes, hipStream_t s, bool by_kernel) {
    void* mapped = nullptr;
    if (by_kernel && OFPS_HIP_UPLOAD_WGS > 0 && bytes % 16 == 0 && ((uintptr_t)dst % 16) == 0 && ((uintptr_t)src % 16) == 0 && device_address_of(src, &mapped)) {
        hipLaunchKernelGGL(upload_kernel, dim3(OFPS_HIP_UPLOAD_WGS), dim3(256), 0, s, static_cast<const u32x4*>(mapped), static_cast<u32x4*>(dst),
                           bytes / 16);
        OFPS_HIP_TRY(ctx, hipGetLastError());
        return OFPS_HIP_OK;
    }
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    return OFPS_HIP_OK;
}

int copy_words_device(ofps_hip_ctx* ctx, void* dst, const void* src, size_t words, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL(copy_words_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, s, static_cast<const uint32_t*>(src), static_cast<uint32_t*>(dst), words);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

int read_back_device(ofps_hip_ctx* ctx, void* host_dst, const void* dev_src, size_t bytes, hipStream_t s) {
    void* mapped = nullptr;
    if (device_address_of(host_dst, &mapped)) {
        const size_t words = bytes / 4;
        return copy_words_device(ctx, mapped, dev_src, words, (unsigned)((words + 255) / 256 < 64 ? (words + 255) / 256 : 64), s);
    }
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, s));
    return OFPS_HIP_OK;
}

// Kernels store into the block and the host reads it after a hipEventDisableTiming event (no release-to-system fence of its own): it must be
// FINE-GRAINED host memory whatever HIP_HOST_COHERENT or a future runtime default says -- asked for explicitly.  A block that
// grows is freed: its last ticket has been collected by then, and the compute stream is idle before it goes.
int host_block_reserve(ofps_hip_ctx* ctx, void** p, size_t* cap, size_t bytes) {
    if (*cap >= bytes) return OFPS_HIP_OK;
    if (*p) { OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); OFPS_HIP_TRY(ctx, hipHostFree(*p)); *p = nullptr; *cap = 0; }
    OFPS_HIP_TRY(ctx, hipHostMalloc(p, bytes, OFPS_HIP_HOST_BLOCK_FLAGS));
    *cap = bytes;
    return OFPS_HIP_OK;
}

}  // namespace ofps
