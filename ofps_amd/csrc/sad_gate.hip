// sad_gate.hip -- hip_sad's contrast gate (include/ofps_hip.h N1g): a lattice block whose pixels hold fewer than `min_pixels` set pixels
// of cv-decoder's contrast mask of the CURRENT frame yields no record -- what av-decoder does with a block the encoder did not predict
// (av-decoder/src/lib.rs:396-419) and what the dense decoders do per pixel (mask.hip).
//
// block_contrast_kernel: the mask's arithmetic (mask_tile.hpp: 64x16 tile, halo 7, reflect-101, separable Sobel, threshold, ballot-packed
// rows, ellipse by 128-bit window extraction) WITHOUT the pixel mask: each wave ballots its dilated rows into 16 row masks of the tile,
// and the row masks are popcounted per lattice block.  HBM traffic: the mask kernel's reads, 4 bytes per BLOCK written instead of one
// per pixel.  For block 8 and 16 the tile origin lies on the lattice and a block lies in one tile: one writer per count, plain stores.
// Any other block size <= 64: a block straddles tiles, the partial counts are added with atomicAdd to a zeroed buffer (integer sums: the
// result does not depend on the order).
// block_keep_kernel: count >= min_pixels -> one byte per block, the flag the ordered compactions of mask.hip take.
// compact_best_kernel: the (dx, dy, SAD) triples compacted by the same flags in the same order.
// Every kernel but the compactions takes the item (the pair of a batch, include/ofps_hip.h N1b) from a grid dimension or sees the batch as one
// array: one launch per step whatever the number of pairs, and one pair is item 0.
// compact_items_kernel: a batch's compaction, segmented: one workgroup per item, records + triples + one count per item.
//
// Host side: ofps::SadFilter (common.hpp), the one filtered search of hip_sad -- this gate, the consistency check (sad_consistency.hip),
// the median test (sad_median.hip) and / or the intra test (sad_intra.hip) in front of one compaction and one device-side count -- for the
// one-pair entry points, the fused per-frame path and, over `pairs` pairs at once, ofps_hip_sad_flow_filtered_dev and the batched stream forms (pipeline.hip).
#include "common.hpp"
#include "mask_tile.hpp"

namespace ofps {

// one workgroup's tile of one frame
__device__ __forceinline__ void block_contrast_tile(const uint8_t* __restrict__ gray, int W, int H, int stride, int block, int nbx, int nby,
                                                    int lattice, uint32_t* __restrict__ counts) {
    __shared__ uint8_t g[MG_H][MG_W + 2];
    __shared__ short hx[MG_H][MS_W + 2];
    __shared__ unsigned long long rowbits[MS_H][2];          // thresholded window, one bit per column
    __shared__ unsigned long long drow[MT_H];                // the tile's mask rows, one bit per column (pixels outside the frame: 0)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * MT_W, y0 = blockIdx.y * MT_H;
    mask_tile_rowbits(gray, W, H, stride, x0, y0, g, hx, rowbits);
#pragma unroll
    for (int k = 0; k < MT_H / 4; ++k) {
        const int ly = wave + 4 * k;
        const bool m = mask_tile_dilated(rowbits, lane, ly);
        const unsigned long long bal = __ballot(m && x0 + lane < W && y0 + ly < H);
        if (lane == 0) drow[ly] = bal;
    }
    __syncthreads();
    // thread j: the j-th block column that meets the tile, clipped to the tile: bits [lo, hi) of every row mask
    if (tid >= MT_W) return;
    const int bx = x0 / block + tid;
    if (bx >= nbx) return;
    const int lo = max(bx * block, x0) - x0, hi = min(bx * block + block, x0 + MT_W) - x0;
    if (lo >= MT_W) return;
    const unsigned long long seg = hi - lo == 64 ? ~0ull : ((1ull << (hi - lo)) - 1ull);
    uint32_t c = 0;
    int by = y0 / block;
    for (int r = 0; r < MT_H; ++r) {
        const int b = (y0 + r) / block;
        if (b != by) {                                        // a block row ends inside the tile
            if (lattice) counts[(size_t)by * nbx + bx] = c; else if (c) atomicAdd(&counts[(size_t)by * nbx + bx], c);
            c = 0; by = b;
        }
        if (by >= nby) return;                                // the ragged bottom margin belongs to no block
        c += (uint32_t)__popcll((drow[r] >> lo) & seg);
    }
    // lattice: MT_H is a multiple of the block size, the last block row ends with the tile
    if (lattice) counts[(size_t)by * nbx + bx] = c; else if (c) atomicAdd(&counts[(size_t)by * nbx + bx], c);
}

// blockIdx.z is the item, its frame `pitch` bytes behind the previous item's, its counts nbx * nby behind
__global__ __launch_bounds__(256) void block_contrast_kernel(const uint8_t* __restrict__ gray, size_t pitch, int W, int H, int stride, int block,
                                                             int nbx, int nby, int lattice, uint32_t* __restrict__ counts) {
    const size_t item = blockIdx.z;
    block_contrast_tile(gray + item * pitch, W, H, stride, block, nbx, nby, lattice, counts + item * (size_t)nbx * nby);
}

__global__ __launch_bounds__(256) void block_keep_kernel(const uint32_t* __restrict__ counts, uint32_t n, uint32_t min_pixels,
                                                         uint8_t* __restrict__ keep) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keep[i] = counts[i] >= min_pixels ? 1 : 0;
}

// compact_small_kernel's scheme (mask.hip) for 12-byte triples, any n: one workgroup, 1,024 triples per round
__global__ __launch_bounds__(1024) void compact_best_kernel(const int* __restrict__ in, const uint8_t* __restrict__ keep_flags, uint32_t n,
                                                            int* __restrict__ out) {
    __shared__ uint32_t wtot[16];
    __shared__ uint32_t base_sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base_sh = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < n; i0 += 1024) {
        const uint32_t i = i0 + tid;
        const bool keep = i < n && keep_flags[i];
        int v0 = 0, v1 = 0, v2 = 0;
        if (keep) { v0 = in[3 * (size_t)i]; v1 = in[3 * (size_t)i + 1]; v2 = in[3 * (size_t)i + 2]; }
        const unsigned long long bal = __ballot(keep);
        const uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = base_sh;
        for (int k = 0; k < wave; ++k) off += wtot[k];
        if (keep) { int* o = out + 3 * (size_t)(off + rank); o[0] = v0; o[1] = v1; o[2] = v2; }
        __syncthreads();
        if (tid == 0) { uint32_t t = 0; for (int k = 0; k < 16; ++k) t += wtot[k]; base_sh += t; }
        __syncthreads();
    }
}

// The segmented ordered compaction of the batched filtered search: workgroup `item` scans its own n flags with the scheme above -- one path
// for every n -- and writes its kept records [and triples] to the head of its own n-record slot and their number to counts[item].
__global__ __launch_bounds__(1024) void compact_items_kernel(const float4* __restrict__ in, const int* __restrict__ in_best,
                                                             const uint8_t* __restrict__ keep_flags, uint32_t n, float4* __restrict__ out,
                                                             int* __restrict__ out_best, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wtot[16];
    __shared__ uint32_t base_sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t item = blockIdx.x, i_base = item * n;
    in += i_base; out += i_base; keep_flags += i_base;
    const bool triples = in_best && out_best;
    if (triples) { in_best += 3 * i_base; out_best += 3 * i_base; }
    if (tid == 0) base_sh = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < n; i0 += 1024) {
        const uint32_t i = i0 + tid;
        const bool keep = i < n && keep_flags[i];
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        int v0 = 0, v1 = 0, v2 = 0;
        if (keep) {
            v = in[i];
            if (triples) { v0 = in_best[3 * (size_t)i]; v1 = in_best[3 * (size_t)i + 1]; v2 = in_best[3 * (size_t)i + 2]; }
        }
        const unsigned long long bal = __ballot(keep);
        const uint32_t rank = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = base_sh;
        for (int k = 0; k < wave; ++k) off += wtot[k];
        if (keep) {                                           // off + rank <= i: inside the item's slot
            out[off + rank] = v;
            if (triples) { int* o = out_best + 3 * (size_t)(off + rank); o[0] = v0; o[1] = v1; o[2] = v2; }
        }
        __syncthreads();
        if (tid == 0) { uint32_t t = 0; for (int k = 0; k < 16; ++k) t += wtot[k]; base_sh += t; }
        __syncthreads();
    }
    if (tid == 0) counts[item] = base_sh;
}

// frame k lies k * pitch bytes behind d_luma, its counts k * nblk behind d_counts; one launch over all `items`
int block_contrast_device(ofps_hip_ctx* ctx, const uint8_t* d_luma, size_t pitch, int items, int W, int H, int stride, int block, uint32_t* d_counts,
                          hipStream_t st) {
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1 && stride >= W, "block_contrast: bad geometry W=%d H=%d stride=%d", W, H, stride);
    OFPS_REQUIRE(ctx, block >= 1 && block <= 64, "block_contrast: block=%d outside [1,64]", block);
    OFPS_REQUIRE(ctx, items >= 1 && items <= 65535, "block_contrast: %d items", items);
    const int nbx = W / block, nby = H / block;
    if (nbx == 0 || nby == 0) return OFPS_HIP_OK;
    OFPS_REQUIRE(ctx, (long long)nbx * nby * items < (1ll << 31), "block_contrast: too many blocks");
    const int lattice = block == 8 || block == 16;
    if (!lattice) OFPS_HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, (size_t)items * nbx * nby * sizeof(uint32_t), st));
    hipLaunchKernelGGL(block_contrast_kernel, dim3((W + MT_W - 1) / MT_W, (H + MT_H - 1) / MT_H, items), dim3(256), 0, st, d_luma, pitch, W, H, stride,
                       block, nbx, nby, lattice, d_counts);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

static int sad_gate_check(ofps_hip_ctx* ctx, int block, int min_pixels, const char* who) {          // min_pixels in [1, block * block]
    OFPS_REQUIRE(ctx, block >= 1 && block <= 64, "%s: block=%d outside [1,64]", who, block);
    OFPS_REQUIRE(ctx, min_pixels >= 1 && min_pixels <= block * block, "%s: contrast gate %d outside [1, %d] for block %d", who, min_pixels,
                 block * block, block);
    return OFPS_HIP_OK;
}

// compact_items_kernel for a caller outside this file (klt.hip's batch form): records alone, no triples
int compact_items_device(ofps_hip_ctx* ctx, const float4* d_in, const uint8_t* d_flags, size_t n, int items, float4* d_out, uint32_t* d_counts) {
    OFPS_REQUIRE(ctx, items >= 1 && n < (1ull << 32), "compact_items: %d items of %zu records", items, n);
    hipLaunchKernelGGL(compact_items_kernel, dim3((unsigned)items), dim3(1024), 0, ctx->stream, d_in, nullptr, d_flags, (uint32_t)n, d_out, nullptr,
                       d_counts);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// ---- SadFilter (common.hpp): the steps of the filtered search
int SadFilter::plan(ofps_hip_ctx* ctx, const char* who) {
    int rc = limit > 0 ? sad_consistency_check(ctx, block, limit, who) : OFPS_HIP_OK;
    if (rc == OFPS_HIP_OK && gate > 0) rc = sad_gate_check(ctx, block, gate, who);
    if (rc == OFPS_HIP_OK && median > 0) rc = sad_median_check(ctx, block, median, who);
    if (rc == OFPS_HIP_OK && intra > 0) rc = sad_intra_check(ctx, block, intra, cut, who);
    if (rc == OFPS_HIP_OK && intra == 0 && (cut < 0 || cut > kSadCutMax)) rc = set_error(ctx, OFPS_HIP_EINVAL, "%s: scene cut %d outside [0, %d]", who, cut, kSadCutMax);
    if (rc != OFPS_HIP_OK) return rc;
    if (split > 0) {                                          // N1s: one pair, integer vectors, the sub-blocks' candidates inside the key's fields
        const int reach = sad_hier_reach(range, ctx->opt.sad_levels);
        if ((rc = sad_split_check(ctx, block, reach < 0 ? kSadHierMaxReach + 1 : reach, split, who)) != OFPS_HIP_OK) return rc;
        OFPS_REQUIRE(ctx, pairs == 1, "%s: split blocks take one pair at a time (%d pairs)", who, pairs);
        if (ctx->opt.sad_motion_scale == 4)
            return set_error(ctx, OFPS_HIP_EUNSUPPORTED, "%s: split blocks (threshold %d) have no quarter-pel form: motion scale 4 needs threshold 0", who, split);
    } else if (split < 0) return set_error(ctx, OFPS_HIP_EINVAL, "%s: split threshold %d is negative", who, split);
    OFPS_REQUIRE(ctx, fr.W > 0 && fr.H > 0 && fr.stride >= fr.W, "%s: bad geometry W=%d H=%d stride=%d", who, fr.W, fr.H, fr.stride);
    OFPS_REQUIRE(ctx, pairs >= 1 && pairs <= 65535, "%s: %d pairs outside [1, 65535]", who, pairs);
    nblk = ofps_hip_sad_block_count(fr.W, fr.H, block);
    OFPS_REQUIRE(ctx, pairs == 1 || total() < (size_t(1) << 31), "%s: too many blocks (%d pairs of %zu)", who, pairs, nblk);
    return OFPS_HIP_OK;
}

int SadFilter::reserve(ofps_hip_ctx* ctx, int tix, int tickets) {
    if (!on()) return OFPS_HIP_OK;
    const size_t fbytes = gate_flags_bytes(nblk, pairs), tri = total() * 3 * sizeof(int);
    d_raw = static_cast<float4*>(scratch(ctx, S_GATE_RAW, total() * sizeof(float4)));
    auto* flags = static_cast<char*>(scratch(ctx, S_GATE_FLAGS, tickets * fbytes));
    if (!d_raw || !flags) return OFPS_HIP_ENOMEM;
    d_flags = flags + tix * fbytes;
    if (winners()) {
        d_fwd = static_cast<int*>(scratch(ctx, S_CONS_FWD, tri));
        if (!d_fwd) return OFPS_HIP_ENOMEM;
    }
    if (limit > 0) {
        d_bwd = static_cast<int*>(scratch(ctx, S_CONS_BWD, tri));
        d_bwd_ent = static_cast<float4*>(scratch(ctx, S_CONS_BWD_ENT, total() * sizeof(float4)));     // the search kernels always write records
        if (!d_bwd || !d_bwd_ent) return OFPS_HIP_ENOMEM;
    }
    if (median > 0) {
        const size_t mbytes = (total() + 15) & ~size_t(15);
        auto* mk = static_cast<uint8_t*>(scratch(ctx, S_MED_KEEP, tickets * mbytes));
        if (!mk) return OFPS_HIP_ENOMEM;
        d_med_keep = mk + tix * mbytes;
    }
    if (intra > 0) {
        const size_t abytes = (total() * sizeof(uint32_t) + 15) & ~size_t(15), ibytes = abytes + (((size_t)pairs * 2 * sizeof(uint32_t) + 15) & ~size_t(15));
        auto* ia = static_cast<char*>(scratch(ctx, S_INTRA, tickets * ibytes));
        if (!ia) return OFPS_HIP_ENOMEM;
        d_act = reinterpret_cast<uint32_t*>(ia + tix * ibytes);
        d_intra_counts = reinterpret_cast<uint32_t*>(ia + tix * ibytes + abytes);
    }
    if (split > 0 && nblk) {
        auto* sp = static_cast<char*>(scratch(ctx, S_SPLIT, sad_split_bytes(nblk)));
        if (!sp) return OFPS_HIP_ENOMEM;
        d_split_raw = reinterpret_cast<float4*>(sp);
        d_sub_best = reinterpret_cast<int*>(sp + nblk * 4 * sizeof(float4));
        d_slot_flags = reinterpret_cast<uint8_t*>(d_sub_best + 12 * nblk);
        d_split = d_slot_flags + 4 * nblk;
    }
    // the records' triples: the forward search's integer winners themselves when they are kept and nothing refines them
    if (want_triples) d_triples = winners() && ctx->opt.sad_motion_scale != 4 ? d_fwd : static_cast<int*>(scratch(ctx, S_GATE_BEST, tri));
    return want_triples && !d_triples ? OFPS_HIP_ENOMEM : OFPS_HIP_OK;
}

int SadFilter::search(ofps_hip_ctx* ctx, float4* d_out) {
    if (!winners()) return sad_pairs_device(ctx, fr, pairs, block, range, on() ? d_raw : d_out, d_triples);
    // check or median test on (the two hazards: sad_consistency.hip): the forward search leaves its integer winners in d_fwd whatever the motion scale -- at
    // scale 4 as d_int_best, the refinement then writes d_triples or nothing -- and the backward search, integer only, runs right behind it
    const bool qpel = ctx->opt.sad_motion_scale == 4;
    const int rc = sad_pairs_device(ctx, fr, pairs, block, range, d_raw, qpel ? d_triples : d_fwd, /*integer_only=*/false, qpel ? d_fwd : nullptr);
    if (rc != OFPS_HIP_OK || limit == 0) return rc;
    return sad_pairs_device(ctx, fr.swapped(), pairs, block, range, d_bwd_ent, d_bwd, /*integer_only=*/true);
}

int SadFilter::contrast_flags(ofps_hip_ctx* ctx, hipStream_t st) {
    if (!nblk) return OFPS_HIP_OK;
    if (intra > 0) {                                          // the intra test's share: the raw current frames' activities, the counters at zero
        const int rc = block_activity_device(ctx, fr.cur_base, fr.cur_pitch, pairs, fr.W, fr.H, fr.stride, block, d_act, st);
        if (rc != OFPS_HIP_OK) return rc;
        OFPS_HIP_TRY(ctx, hipMemsetAsync(d_intra_counts, 0, (size_t)pairs * 2 * sizeof(uint32_t), st));
    }
    if (gate <= 0) return OFPS_HIP_OK;
    const int rc = block_contrast_device(ctx, fr.cur_base, fr.cur_pitch, pairs, fr.W, fr.H, fr.stride, block, gate_counts(d_flags), st);
    if (rc != OFPS_HIP_OK) return rc;
    // a flag depends on its own count alone: the batch's pairs * nblk counts are one array to this kernel
    hipLaunchKernelGGL(block_keep_kernel, dim3((unsigned)((total() + 255) / 256)), dim3(256), 0, st, gate_counts(d_flags), (uint32_t)total(), (uint32_t)gate, keep());
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

int SadFilter::finish(ofps_hip_ctx* ctx, float4* d_out, int* d_out_best, uint32_t* d_count) {
    if (!on()) return OFPS_HIP_OK;
    int rc = OFPS_HIP_OK;
    // the intra test: the forward winners' SADs against the activities contrast_flags() made of the RAW current frames (as the gate reads
    // them), the verdict ANDed onto the gate's flags
    if (intra > 0 && nblk) {
        rc = sad_intra_flags_device(ctx, d_fwd, d_act, gate > 0 ? keep() : nullptr, fr.W, fr.H, block, intra, keep(), d_intra_counts, ctx->stream, pairs,
                                    /*zero_counts=*/false);
        if (rc != OFPS_HIP_OK) return rc;
    }
    if (limit > 0)
        rc = sad_consistency_flags_device(ctx, d_fwd, d_bwd, fr.W, fr.H, block, limit, gate > 0 || intra > 0 ? keep() : nullptr, nullptr, keep(), ctx->stream, pairs);
    if (rc != OFPS_HIP_OK) return rc;
    // one pass: the median test reads the other criteria's flags (none on: all ones) and writes its own array
    if (median > 0)
        rc = sad_median_flags_device(ctx, d_fwd, gate > 0 || limit > 0 || intra > 0 ? keep() : nullptr, fr.W, fr.H, block, median, nullptr, d_med_keep, ctx->stream, pairs);
    if (rc != OFPS_HIP_OK) return rc;
    if (nblk == 0) {
        OFPS_HIP_TRY(ctx, hipMemsetAsync(d_count, 0, pairs * sizeof(uint32_t), ctx->stream));
        return OFPS_HIP_OK;
    }
    uint8_t* flags = median > 0 ? d_med_keep : keep();
    // a cut item loses every flag: gate and intra verdicts alone decide that, whatever check and median test said since
    if (intra > 0 && (rc = sad_cut_device(ctx, d_intra_counts, nblk, cut, flags, ctx->stream, pairs)) != OFPS_HIP_OK) return rc;
    if (split > 0) return finish_split(ctx, criteria() ? flags : nullptr, d_out, d_out_best, d_count);
    // The compaction is the one step that keeps a path per shape.  compact_items_kernel runs ONE workgroup per item whatever nblk: right for a
    // batch of small lattices, but one pair through it would scan a 4K frame's 129,600 blocks on one compute unit, and in one launch where the
    // paths below take up to three.  That would change speed and launch count; the one-pair path stays on the grid-wide compactions of mask.hip
    if (pairs > 1) {                                          // records, triples and counts[item] in one launch
        hipLaunchKernelGGL(compact_items_kernel, dim3((unsigned)pairs), dim3(1024), 0, ctx->stream, d_raw, d_out_best ? d_triples : nullptr, flags,
                           (uint32_t)nblk, d_out, d_out_best, d_count);
        OFPS_HIP_TRY(ctx, hipGetLastError());
        return OFPS_HIP_OK;
    }
    rc = nblk <= kCompactSmallMax ? compact_small_device(ctx, d_raw, flags, nblk, d_out, d_count)
                                  : compact_entries_device(ctx, d_raw, flags, nblk, d_out, d_count);
    if (rc != OFPS_HIP_OK) return rc;
    if (d_out_best) {
        hipLaunchKernelGGL(compact_best_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_triples, flags, (uint32_t)nblk, d_out_best);
        OFPS_HIP_TRY(ctx, hipGetLastError());
    }
    return OFPS_HIP_OK;
}

// N1s behind the criteria's final flags (null: every block is kept): the split step over the frames the integer search read -> raw slots
// 4 * blk + s and their flags -> the one compaction, over 4 * nblk slots: block raster order, a split block's four records in sub-block
// order, the count on the device.  The cut rule's veto has cleared the flags by now.  d_out_best: the PARENTS' triples of the kept blocks
int SadFilter::finish_split(ofps_hip_ctx* ctx, const uint8_t* flags, float4* d_out, int* d_out_best, uint32_t* d_count) {
    // mean removal: the search filtered its pair into scratch that, with the check on, the backward search has since rewritten; the step
    // filters the pair itself either way (one more filter pass, only with both settings on)
    SadFrames s = fr;
    int rc = OFPS_HIP_OK;
    if (ctx->opt.sad_prefilter > 0 && (rc = sad_prefilter_pairs_device(ctx, ctx->opt.sad_prefilter, fr, 1, &s)) != OFPS_HIP_OK) return rc;
    rc = sad_split_device(ctx, s, 1, block, sad_hier_reach(range, ctx->opt.sad_levels), split, d_fwd, flags, d_sub_best, d_split, d_split_raw, d_slot_flags);
    if (rc != OFPS_HIP_OK) return rc;
    // (four slots per block: a 1080p frame's 32,160 slots are past the size one workgroup scans well; the grid-wide compaction takes over earlier)
    rc = 4 * nblk <= kCompactSmallMax / 4 ? compact_small_device(ctx, d_split_raw, d_slot_flags, 4 * nblk, d_out, d_count)
                                          : compact_entries_device(ctx, d_split_raw, d_slot_flags, 4 * nblk, d_out, d_count);
    if (rc != OFPS_HIP_OK || !d_out_best) return rc;
    if (!flags) {
        OFPS_HIP_TRY(ctx, hipMemcpyAsync(d_out_best, d_triples, nblk * 3 * sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
        return OFPS_HIP_OK;
    }
    hipLaunchKernelGGL(compact_best_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_triples, flags, (uint32_t)nblk, d_out_best);
    OFPS_HIP_TRY(ctx, hipGetLastError());
    return OFPS_HIP_OK;
}

// `pairs` pairs of `f`, everything on ctx->stream: search[es], [contrast flags and / or activities of the current frames,] [the intra test's flags,] [the check's flags,] [the median test's
// flags,] one compaction, one count per pair.  Item k's kept records [and triples] lead its nblk-record slot of d_out [d_out_best], d_counts[k]
// is their number
int sad_flow_filtered_device(ofps_hip_ctx* ctx, const SadFrames& f, int pairs, int block, int range, const SadCriteria& c, float4* d_out,
                             int* d_out_best, uint32_t* d_counts, const char* who, int tix, int tickets) {
    SadFilter flt = SadFilter::make(f, pairs, block, range, c, d_out_best != nullptr);
    int rc = flt.plan(ctx, who);
    if (rc == OFPS_HIP_OK) rc = flt.reserve(ctx, tix, tickets);
    if (rc == OFPS_HIP_OK) rc = flt.search(ctx, d_out);
    if (rc == OFPS_HIP_OK) rc = flt.contrast_flags(ctx, ctx->stream);
    return rc == OFPS_HIP_OK ? flt.finish(ctx, d_out, d_out_best, d_counts) : rc;
}

}  // namespace ofps

extern "C" {

int ofps_hip_sad_flow_filtered_dev(ofps_hip_ctx* ctx, const void* d_frames, int n_frames, int W, int H, int stride, size_t frame_pitch, int ref_mode,
                                   int block, int range, int min_pixels, int limit, int median, void* d_out_entries, void* d_out_best,
                                   void* d_out_counts) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_frames && d_out_entries && d_out_counts, "sad_flow_filtered_dev: null device pointer");
    OFPS_REQUIRE(ctx, n_frames >= 2, "sad_flow_filtered_dev: need at least 2 frames (got %d)", n_frames);
    OFPS_REQUIRE(ctx, W > 0 && H > 0 && stride >= W, "sad_flow_filtered_dev: bad geometry W=%d H=%d stride=%d", W, H, stride);
    OFPS_REQUIRE(ctx, frame_pitch >= (size_t)stride * (size_t)H, "sad_flow_filtered_dev: frame_pitch smaller than a frame");
    OFPS_REQUIRE(ctx, ref_mode == 0 || ref_mode == 1, "sad_flow_filtered_dev: ref_mode must be 0 or 1");
    OFPS_REQUIRE(ctx, min_pixels >= 0, "sad_flow_filtered_dev: contrast gate %d is negative", min_pixels);
    OFPS_REQUIRE(ctx, limit >= 0, "sad_flow_filtered_dev: consistency limit %d is negative", limit);
    OFPS_REQUIRE(ctx, median >= 0, "sad_flow_filtered_dev: median limit %d is negative", median);
    OFPS_REQUIRE(ctx, min_pixels > 0 || limit > 0 || median > 0,
                 "sad_flow_filtered_dev: contrast gate, consistency limit and median limit are all 0 (the unfiltered form is ofps_hip_sad_flow_dev)");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::sad_flow_filtered_device(ctx, ofps::SadFrames::sequence(static_cast<const uint8_t*>(d_frames), frame_pitch, ref_mode, W, H, stride),
                                          n_frames - 1, block, range, {min_pixels, limit, median}, static_cast<float4*>(d_out_entries),
                                          static_cast<int*>(d_out_best), static_cast<uint32_t*>(d_out_counts), "sad_flow_filtered_dev");
}

int ofps_hip_block_contrast_dev(ofps_hip_ctx* ctx, const void* d_luma, int W, int H, int stride, int block, void* d_out_counts) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_luma && d_out_counts, "block_contrast_dev: null device pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ofps::block_contrast_device(ctx, static_cast<const uint8_t*>(d_luma), 0, 1, W, H, stride, block, static_cast<uint32_t*>(d_out_counts), ctx->stream);
}

int ofps_hip_block_contrast(ofps_hip_ctx* ctx, const uint8_t* luma, int W, int H, int stride, int block, uint32_t* out_counts) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, luma && out_counts, "block_contrast: null host pointer");
    OFPS_REQUIRE(ctx, W >= 1 && H >= 1 && stride >= W, "block_contrast: bad geometry W=%d H=%d stride=%d", W, H, stride);
    OFPS_REQUIRE(ctx, block >= 1 && block <= 64, "block_contrast: block=%d outside [1,64]", block);
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nblk = ofps_hip_sad_block_count(W, H, block);
    if (!nblk) return OFPS_HIP_OK;
    auto* d_gray = static_cast<uint8_t*>(ofps::scratch(ctx, ofps::S_FRAMES, (size_t)W * H));
    auto* d_flags = static_cast<char*>(ofps::scratch(ctx, ofps::S_GATE_FLAGS, ofps::gate_flags_bytes(nblk)));
    if (!d_gray || !d_flags) return OFPS_HIP_ENOMEM;
    OFPS_HIP_TRY(ctx, ofps::upload_rows(d_gray, W, luma, stride, W, H, ctx->stream));
    const int rc = ofps::block_contrast_device(ctx, d_gray, 0, 1, W, H, W, block, ofps::gate_counts(d_flags), ctx->stream);
    if (rc != OFPS_HIP_OK) return rc;
    OFPS_HIP_TRY(ctx, hipMemcpyAsync(out_counts, ofps::gate_counts(d_flags), nblk * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    OFPS_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OFPS_HIP_OK;
}

int ofps_hip_set_sad_gate(ofps_hip_ctx* ctx, int min_pixels) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, min_pixels >= 0, "set_sad_gate: %d is negative", min_pixels);
    ctx->opt.sad_gate = min_pixels;
    return OFPS_HIP_OK;
}

int ofps_hip_get_sad_gate(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.sad_gate : OFPS_HIP_EINVAL; }

int ofps_hip_set_sad_batch_filter(ofps_hip_ctx* ctx, int on) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, on == 0 || on == 1, "set_sad_batch_filter: %d is not 0|1", on);
    ctx->opt.sad_batch_filter = on;
    return OFPS_HIP_OK;
}

int ofps_hip_get_sad_batch_filter(ofps_hip_ctx* ctx) { return ctx ? ctx->opt.sad_batch_filter : OFPS_HIP_EINVAL; }

int ofps_hip_sad_flow_gated_dev(ofps_hip_ctx* ctx, const void* d_prev, const void* d_cur, int W, int H, int stride, int block, int range,
                                int min_pixels, void* d_out_entries, void* d_out_best, void* d_out_count) {
    if (!ctx) return OFPS_HIP_EINVAL;
    OFPS_REQUIRE(ctx, d_prev && d_cur && d_out_entries && d_out_count, "sad_flow_gated_dev: null device pointer");
    OFPS_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = ofps::sad_gate_check(ctx, block, min_pixels, "sad_flow");             // (the filter itself takes 0 for "no gate")
    if (rc != OFPS_HIP_OK) return rc;
    return ofps::sad_flow_filtered_device(ctx, {static_cast<const uint8_t*>(d_prev), static_cast<const uint8_t*>(d_cur), 0, 0, W, H, stride}, 1, block,
                                          range, {min_pixels}, static_cast<float4*>(d_out_entries), static_cast<int*>(d_out_best),
                                          static_cast<uint32_t*>(d_out_count), "sad_flow");
}

}  // extern "C"
