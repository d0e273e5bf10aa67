"""Thin Python front-end over the C ABI (include/ofps_hip.h): context handling plus numpy and
device-pointer call wrappers.  All compute happens in libofps_hip.so; nothing here has a CPU path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import OfpsHipError


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class HipContext:
    """One ofps_hip_ctx (one per plugin instance, ofps/src/plugins/mod.rs:244-278 'Send, not Sync')."""

    def __init__(self, device: int = 0, test_hooks: bool = False):
        # test_hooks: bind libofps_hip_testhooks.so (fault injectors compiled in) instead of the product library
        self._lib = _lib.load_test_hooks() if test_hooks else _lib.load()
        h = C.c_void_p()
        rc = self._lib.ofps_hip_init(device, C.byref(h))
        if rc != 0:
            raise OfpsHipError(rc, (self._lib.ofps_hip_last_error(None) or b"").decode())
        self._h = h
        self.device = device
        self._pinned = []

    def close(self):
        if getattr(self, "_h", None):
            for p in getattr(self, "_pinned", []):
                self._lib.ofps_hip_host_free(self._h, C.c_void_p(p))
            self._pinned = []
            self._lib.ofps_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise OfpsHipError(rc, (self._lib.ofps_hip_last_error(self._h) or b"").decode())

    # ---- plumbing
    def set_stream(self, stream_ptr: int):
        """Enqueue on a caller-owned hipStream_t; 0 is HIP's default stream (torch's default)."""
        self._check(self._lib.ofps_hip_set_stream(self._h, C.c_void_p(stream_ptr)))

    def use_own_stream(self):
        self._check(self._lib.ofps_hip_use_own_stream(self._h))

    def use_torch_stream(self):
        import torch
        self.set_stream(torch.cuda.current_stream().cuda_stream)

    def sync(self):
        self._check(self._lib.ofps_hip_sync(self._h))

    def set_option(self, name: str, value=None):
        """Diagnostic / A-B switch by its environment-variable name; None restores the default."""
        v = None if value is None else str(value).encode()
        self._check(self._lib.ofps_hip_set_option(self._h, name.encode(), v))

    def almeida_recoveries(self) -> int:
        n = C.c_uint64(0)
        self._check(self._lib.ofps_hip_almeida_recoveries(self._h, C.byref(n)))
        return int(n.value)

    # device memory for hosts without a HIP binding of their own (what the Rust shim uses for resident chains)
    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p(0)
        self._check(self._lib.ofps_hip_malloc(self._h, nbytes, C.byref(p)))
        return int(p.value)

    def free(self, dptr: int):
        self._check(self._lib.ofps_hip_free(self._h, C.c_void_p(dptr)))

    def memcpy_h2d(self, dptr: int, host: np.ndarray):
        a = np.ascontiguousarray(host)
        self._check(self._lib.ofps_hip_memcpy_h2d(self._h, C.c_void_p(dptr), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def memcpy_d2h(self, host: np.ndarray, dptr: int):
        assert host.flags["C_CONTIGUOUS"]
        self._check(self._lib.ofps_hip_memcpy_d2h(self._h, host.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), host.nbytes))

    def get_stream(self) -> int:
        return int(self._lib.ofps_hip_get_stream(self._h) or 0)

    def timer_start(self):
        self._check(self._lib.ofps_hip_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_float(0)
        self._check(self._lib.ofps_hip_timer_stop(self._h, C.byref(ms)))
        return float(ms.value)

    # ---- N1
    SAD_EXHAUSTIVE, SAD_PRUNED = 0, 1

    def set_sad_mode(self, mode: int):
        """0 = exhaustive (default), 1 = exact search with partial-distortion elimination (content-dependent run time)."""
        self._check(self._lib.ofps_hip_set_sad_mode(self._h, mode))

    def set_sad_motion_scale(self, scale: int):
        """1 = full-pel vectors (default); 4 = quarter-pel refinement of every block's integer winner (H.264's motion_scale)."""
        self._check(self._lib.ofps_hip_set_sad_motion_scale(self._h, scale))

    def get_sad_motion_scale(self) -> int:
        return int(self._lib.ofps_hip_get_sad_motion_scale(self._h))

    def set_sad_gate(self, min_pixels: int):
        """hip_sad's contrast gate (include/ofps_hip.h N1g): 0 = one record per lattice block (default); N >= 1 = only the blocks that hold
        at least N set pixels of the current frame's contrast mask yield a record (sad_flow, push_frame[_async])."""
        self._check(self._lib.ofps_hip_set_sad_gate(self._h, min_pixels))

    def get_sad_gate(self) -> int:
        return int(self._lib.ofps_hip_get_sad_gate(self._h))

    def block_contrast(self, luma: np.ndarray, block: int, stride: int | None = None) -> np.ndarray:
        """Set pixels of the contrast mask of `luma` per full lattice block -> uint32 [H // block, W // block].  stride: as for contrast_mask."""
        if stride is None:
            g = np.ascontiguousarray(luma, np.uint8)
            stride = g.shape[1]
        else:
            g = luma
            assert g.dtype == np.uint8 and g.ndim == 2 and (g.shape[0] == 1 or g.strides[0] == stride) and g.strides[1] == 1
        H, W = g.shape
        out = np.zeros((H // block, W // block), np.uint32)
        buf = out if out.size else np.zeros(1, np.uint32)
        self._check(self._lib.ofps_hip_block_contrast(self._h, C.cast(C.c_void_p(g.ctypes.data), C.POINTER(C.c_uint8)), W, H, stride, block,
                                                      buf.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def block_contrast_dev(self, d_luma: int, W: int, H: int, stride: int, block: int, d_out_counts: int):
        self._check(self._lib.ofps_hip_block_contrast_dev(self._h, C.c_void_p(d_luma), W, H, stride, block, C.c_void_p(d_out_counts)))

    def sad_flow_gated_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, block: int, search_range: int, min_pixels: int,
                           d_out_entries: int, d_out_best: int | None, d_out_count: int):
        """One pair of device frames through the contrast gate: the kept records first (capacity nblk), their count in *d_out_count (u32).
        Enqueue only."""
        self._check(self._lib.ofps_hip_sad_flow_gated_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, block, search_range,
                                                          min_pixels, C.c_void_p(d_out_entries), C.c_void_p(d_out_best or 0),
                                                          C.c_void_p(d_out_count)))

    def set_sad_consistency(self, limit: int):
        """hip_sad's forward-backward consistency check (include/ofps_hip.h N1c): 0 = off (default); N in [1, 129] = only the blocks whose
        round-trip residual max(|dx + ex|, |dy + ey|) is below N yield a record (sad_flow, push_frame[_async]); 1 = an exact round trip."""
        self._check(self._lib.ofps_hip_set_sad_consistency(self._h, limit))

    def get_sad_consistency(self) -> int:
        return int(self._lib.ofps_hip_get_sad_consistency(self._h))

    def sad_consistency(self, fwd_best: np.ndarray, bwd_best: np.ndarray, W: int, H: int, block: int, limit: int, want_residual=True,
                        want_keep=True):
        """The check alone on two [nblk, 3] arrays of (dx, dy, sad) integer winners (forward, backward) -> (residual uint32 [nblk] or None,
        keep uint8 [nblk] or None)."""
        f = np.ascontiguousarray(fwd_best, np.int32); b = np.ascontiguousarray(bwd_best, np.int32)
        nb = int(self._lib.ofps_hip_sad_block_count(W, H, block))
        assert f.shape == b.shape == (nb, 3)
        res = np.zeros(max(nb, 1), np.uint32) if want_residual else None
        keep = np.zeros(max(nb, 1), np.uint8) if want_keep else None
        i32 = C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_sad_consistency(self._h, f.ctypes.data_as(i32), b.ctypes.data_as(i32), W, H, block, limit,
                                                       res.ctypes.data_as(C.POINTER(C.c_uint32)) if want_residual else None,
                                                       keep.ctypes.data_as(C.POINTER(C.c_uint8)) if want_keep else None))
        return (res[:nb] if want_residual else None), (keep[:nb] if want_keep else None)

    def sad_consistency_dev(self, d_fwd_best: int, d_bwd_best: int, W: int, H: int, block: int, limit: int, d_out_residual: int | None,
                            d_out_keep: int | None):
        self._check(self._lib.ofps_hip_sad_consistency_dev(self._h, C.c_void_p(d_fwd_best), C.c_void_p(d_bwd_best), W, H, block, limit,
                                                           C.c_void_p(d_out_residual or 0), C.c_void_p(d_out_keep or 0)))

    def sad_flow_checked_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, block: int, search_range: int, min_pixels: int,
                             limit: int, d_out_entries: int, d_out_best: int | None, d_out_count: int):
        """One pair of device frames through the consistency check (and the contrast gate when min_pixels > 0): the kept records first
        (capacity nblk), their count in *d_out_count (u32).  Enqueue only."""
        self._check(self._lib.ofps_hip_sad_flow_checked_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, block, search_range,
                                                            min_pixels, limit, C.c_void_p(d_out_entries), C.c_void_p(d_out_best or 0),
                                                            C.c_void_p(d_out_count)))

    def set_sad_median(self, limit: int):
        """hip_sad's median test (include/ofps_hip.h N1v): 0 = off (default); N in [1, 255] = only the blocks whose integer winner lies
        less than N pixels (Chebyshev, in half-pixel steps) from the component-wise median of their kept lattice neighbours' winners yield
        a record (sad_flow, push_frame[_async])."""
        self._check(self._lib.ofps_hip_set_sad_median(self._h, limit))

    def get_sad_median(self) -> int:
        return int(self._lib.ofps_hip_get_sad_median(self._h))

    def sad_median(self, best: np.ndarray, keep_in: np.ndarray | None, W: int, H: int, block: int, limit: int, want_residual=True,
                   want_keep=True):
        """The test alone on a [nblk, 3] array of (dx, dy, sad) integer winners and the other criteria's keep bytes (None = all ones)
        -> (doubled residual uint32 [nblk] or None, keep uint8 [nblk] or None)."""
        b = np.ascontiguousarray(best, np.int32)
        nb = int(self._lib.ofps_hip_sad_block_count(W, H, block))
        assert b.shape == (nb, 3)
        k = None if keep_in is None else np.ascontiguousarray(keep_in, np.uint8)
        assert k is None or k.shape == (nb,)
        res = np.zeros(max(nb, 1), np.uint32) if want_residual else None
        keep = np.zeros(max(nb, 1), np.uint8) if want_keep else None
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.ofps_hip_sad_median(self._h, b.ctypes.data_as(C.POINTER(C.c_int32)), None if k is None else k.ctypes.data_as(u8),
                                                  W, H, block, limit, res.ctypes.data_as(C.POINTER(C.c_uint32)) if want_residual else None,
                                                  keep.ctypes.data_as(u8) if want_keep else None))
        return (res[:nb] if want_residual else None), (keep[:nb] if want_keep else None)

    def sad_median_dev(self, d_best: int, d_keep_in: int | None, W: int, H: int, block: int, limit: int, d_out_residual2: int | None,
                       d_out_keep: int | None):
        self._check(self._lib.ofps_hip_sad_median_dev(self._h, C.c_void_p(d_best), C.c_void_p(d_keep_in or 0), W, H, block, limit,
                                                      C.c_void_p(d_out_residual2 or 0), C.c_void_p(d_out_keep or 0)))

    def sad_flow_median_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, block: int, search_range: int, min_pixels: int,
                            limit: int, median_limit: int, d_out_entries: int, d_out_best: int | None, d_out_count: int):
        """One pair of device frames through the median test (the contrast gate when min_pixels > 0, the consistency check when limit > 0):
        the kept records first (capacity nblk), their count in *d_out_count (u32).  Enqueue only."""
        self._check(self._lib.ofps_hip_sad_flow_median_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, block, search_range,
                                                           min_pixels, limit, median_limit, C.c_void_p(d_out_entries),
                                                           C.c_void_p(d_out_best or 0), C.c_void_p(d_out_count)))

    def sad_flow_filtered_dev(self, d_frames: int, n_frames: int, W: int, H: int, stride: int, frame_pitch: int, ref_mode: int, block: int,
                              search_range: int, min_pixels: int, limit: int, median: int, d_out_entries: int, d_out_best: int | None,
                              d_out_counts: int):
        """The batched search of sad_flow_dev through contrast gate, consistency check and / or median test with explicit values (include/
        ofps_hip.h N1b): item k's kept records [and triples] first in its nblk-sized slot, its count in d_out_counts[k] (u32).  Enqueue only."""
        self._check(self._lib.ofps_hip_sad_flow_filtered_dev(self._h, C.c_void_p(d_frames), n_frames, W, H, stride, frame_pitch, ref_mode, block,
                                                             search_range, min_pixels, limit, median, C.c_void_p(d_out_entries),
                                                             C.c_void_p(d_out_best or 0), C.c_void_p(d_out_counts)))

    def set_sad_batch_filter(self, on: int):
        """0 = push_frames_async and the multi-device workers' pushes ignore gate, check and median test (default); 1 = they follow the
        context's three settings: frames_wait's n_vectors is the kept count per frame, the kept records lead each frame's slot."""
        self._check(self._lib.ofps_hip_set_sad_batch_filter(self._h, int(on)))

    def get_sad_batch_filter(self) -> int:
        return int(self._lib.ofps_hip_get_sad_batch_filter(self._h))

    def set_sad_intra(self, ratio: int):
        """hip_sad's intra test (include/ofps_hip.h N1i): 0 = off (default); q in [1, 255] (sixteenths) = a block whose integer winner's SAD
        reaches q/16 of the block's activity in the raw current frame (16 * SAD >= q * A) yields no record (sad_flow, push_frame[_async])."""
        self._check(self._lib.ofps_hip_set_sad_intra(self._h, ratio))

    def get_sad_intra(self) -> int:
        return int(self._lib.ofps_hip_get_sad_intra(self._h))

    def set_sad_cut(self, percent: int):
        """hip_sad's scene-cut rule (N1i): 0 = off (default); P in [1, 100] = a pair with at least P percent of its gated blocks intra yields
        no record at all.  No effect while the intra ratio is 0."""
        self._check(self._lib.ofps_hip_set_sad_cut(self._h, percent))

    def get_sad_cut(self) -> int:
        return int(self._lib.ofps_hip_get_sad_cut(self._h))

    def block_activity(self, luma: np.ndarray, block: int, stride: int | None = None) -> np.ndarray:
        """Sum of |pixel - rounded block mean| per full lattice block of `luma` -> uint32 [H // block, W // block].  stride: as for
        block_contrast."""
        if stride is None:
            g = np.ascontiguousarray(luma, np.uint8)
            stride = g.shape[1]
        else:
            g = luma
            assert g.dtype == np.uint8 and g.ndim == 2 and (g.shape[0] == 1 or g.strides[0] == stride) and g.strides[1] == 1
        H, W = g.shape
        out = np.zeros((H // block, W // block), np.uint32)
        buf = out if out.size else np.zeros(1, np.uint32)
        self._check(self._lib.ofps_hip_block_activity(self._h, C.cast(C.c_void_p(g.ctypes.data), C.POINTER(C.c_uint8)), W, H, stride, block,
                                                      buf.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def block_activity_dev(self, d_luma: int, W: int, H: int, stride: int, block: int, d_out_activity: int):
        self._check(self._lib.ofps_hip_block_activity_dev(self._h, C.c_void_p(d_luma), W, H, stride, block, C.c_void_p(d_out_activity)))

    def sad_intra(self, best: np.ndarray, activity: np.ndarray, keep_in: np.ndarray | None, W: int, H: int, block: int, ratio: int, cut: int = 0,
                  want_counts=True):
        """Verdict and cut rule alone on a [nblk, 3] array of (dx, dy, sad) integer winners, the blocks' activities and the gate's keep
        bytes (None = all ones) -> (keep uint8 [nblk], [n_cand, n_intra] uint32 or None)."""
        b = np.ascontiguousarray(best, np.int32)
        nb = int(self._lib.ofps_hip_sad_block_count(W, H, block))
        a = np.ascontiguousarray(activity, np.uint32).reshape(-1)
        assert b.shape == (nb, 3) and a.shape == (nb,)
        k = None if keep_in is None else np.ascontiguousarray(keep_in, np.uint8)
        assert k is None or k.shape == (nb,)
        keep = np.zeros(max(nb, 1), np.uint8)
        counts = np.zeros(2, np.uint32) if want_counts else None
        u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
        self._check(self._lib.ofps_hip_sad_intra(self._h, b.ctypes.data_as(C.POINTER(C.c_int32)), a.ctypes.data_as(u32),
                                                 None if k is None else k.ctypes.data_as(u8), W, H, block, ratio, cut, keep.ctypes.data_as(u8),
                                                 counts.ctypes.data_as(u32) if want_counts else None))
        return keep[:nb], counts

    def sad_intra_dev(self, d_best: int, d_activity: int, d_keep_in: int | None, W: int, H: int, block: int, ratio: int, cut: int,
                      d_out_keep: int, d_out_counts: int | None):
        self._check(self._lib.ofps_hip_sad_intra_dev(self._h, C.c_void_p(d_best), C.c_void_p(d_activity), C.c_void_p(d_keep_in or 0), W, H, block,
                                                     ratio, cut, C.c_void_p(d_out_keep), C.c_void_p(d_out_counts or 0)))

    def sad_flow_intra_dev(self, d_frames: int, n_frames: int, W: int, H: int, stride: int, frame_pitch: int, ref_mode: int, block: int,
                           search_range: int, min_pixels: int, limit: int, median: int, intra: int, cut: int, d_out_entries: int,
                           d_out_best: int | None, d_out_counts: int):
        """sad_flow_filtered_dev with the intra test (intra in [1, 255]) and the cut rule (cut in [0, 100]) as two more explicit values
        (include/ofps_hip.h N1i); min_pixels, limit and median may all be 0.  Enqueue only."""
        self._check(self._lib.ofps_hip_sad_flow_intra_dev(self._h, C.c_void_p(d_frames), n_frames, W, H, stride, frame_pitch, ref_mode, block,
                                                          search_range, min_pixels, limit, median, intra, cut, C.c_void_p(d_out_entries),
                                                          C.c_void_p(d_out_best or 0), C.c_void_p(d_out_counts)))

    def set_sad_split(self, threshold: int):
        """hip_sad's split blocks (include/ofps_hip.h N1s): 0 = off (default); T in [1, 4080] (sixteenths of a grey level per pixel) = a kept
        block whose four sub-blocks together match better than the block by at least T yields their four records in its place (sad_flow,
        push_frame[_async]); the record buffers then hold sad_record_capacity() = 4 * nblk records."""
        self._check(self._lib.ofps_hip_set_sad_split(self._h, threshold))

    def get_sad_split(self) -> int:
        return int(self._lib.ofps_hip_get_sad_split(self._h))

    def sad_record_capacity(self, W: int, H: int, block: int) -> int:
        """The records a search call of this context may return: nblk, 4 * nblk with split blocks on."""
        if "ofps_hip_sad_record_capacity" not in _lib.PROTOTYPES:      # a tool's --lib run against a build from before N1s: one record per block
            return int(self._lib.ofps_hip_sad_block_count(W, H, block))
        return int(self._lib.ofps_hip_sad_record_capacity(self._h, W, H, block))

    def sad_split(self, prev: np.ndarray, cur: np.ndarray, block: int, best: np.ndarray, keep: np.ndarray | None, reach: int, threshold: int,
                  want_entries=True, stride: int | None = None) -> dict:
        """The split step alone on a [nblk, 3] array of parent (dx, dy, sad) triples and keep bytes (None = all ones) -> dict(sub_best int32
        [nblk, 4, 3], split uint8 [nblk], entries float32 [nblk, 4, 4] | None, slot_flags uint8 [nblk, 4] | None).  stride: None, or the row
        pitch in bytes of both frames (views of wider buffers)."""
        if stride is None:
            prev = np.ascontiguousarray(prev, np.uint8); cur = np.ascontiguousarray(cur, np.uint8)
            stride = prev.shape[1]
        else:
            for g in (prev, cur):
                assert g.dtype == np.uint8 and g.ndim == 2 and (g.shape[0] == 1 or g.strides[0] == stride) and g.strides[1] == 1
        assert prev.shape == cur.shape and prev.ndim == 2
        H, W = prev.shape
        nb = int(self._lib.ofps_hip_sad_block_count(W, H, block))
        b = np.ascontiguousarray(best, np.int32)
        k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        assert b.shape == (nb, 3) and (k is None or k.shape == (nb,))
        sub = np.zeros((max(nb, 1), 4, 3), np.int32)
        split = np.zeros(max(nb, 1), np.uint8)
        ent = np.zeros((max(nb, 1), 4, 4), np.float32) if want_entries else None
        slot = np.zeros((max(nb, 1), 4), np.uint8) if want_entries else None
        u8, i32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_sad_split(self._h, C.cast(C.c_void_p(prev.ctypes.data), u8), C.cast(C.c_void_p(cur.ctypes.data), u8), W, H,
                                                 stride, block, b.ctypes.data_as(i32), None if k is None else k.ctypes.data_as(u8), reach, threshold,
                                                 sub.ctypes.data_as(i32), split.ctypes.data_as(u8), _fp(ent) if want_entries else None,
                                                 slot.ctypes.data_as(u8) if want_entries else None))
        return {"sub_best": sub[:nb], "split": split[:nb], "entries": ent[:nb] if want_entries else None,
                "slot_flags": slot[:nb] if want_entries else None}

    def sad_split_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, block: int, d_best: int, d_keep: int | None, reach: int,
                      threshold: int, d_out_sub_best: int, d_out_split: int, d_out_entries: int | None = None, d_out_slot_flags: int | None = None):
        self._check(self._lib.ofps_hip_sad_split_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, block, C.c_void_p(d_best),
                                                     C.c_void_p(d_keep or 0), reach, threshold, C.c_void_p(d_out_sub_best), C.c_void_p(d_out_split),
                                                     C.c_void_p(d_out_entries or 0), C.c_void_p(d_out_slot_flags or 0)))

    def sad_flow_split_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, block: int, search_range: int, min_pixels: int, limit: int,
                           median: int, threshold: int, d_out_entries: int, d_out_count: int):
        """One pair in device memory: search + gate / check / median test (0 = off each) + split blocks (threshold in [1, 4080]) + one
        compaction; d_out_entries holds 4 * nblk records, d_out_count one uint32.  Enqueue only."""
        self._check(self._lib.ofps_hip_sad_flow_split_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, block, search_range,
                                                          min_pixels, limit, median, threshold, C.c_void_p(d_out_entries), C.c_void_p(d_out_count)))

    def set_sad_levels(self, levels: int):
        """hip_sad's search levels (include/ofps_hip.h N1h): 1 = the plain search (default); 2 | 3 = the search runs on the frames halved
        levels - 1 times and every finer level repairs the doubled vectors in a +-3 window: reach 2 * range + 3, 4 * range + 9."""
        self._check(self._lib.ofps_hip_set_sad_levels(self._h, levels))

    def get_sad_levels(self) -> int:
        return int(self._lib.ofps_hip_get_sad_levels(self._h))

    def sad_reach(self, search_range: int, levels: int) -> int:
        """The largest |dx|, |dy| a search of `search_range` over `levels` levels can return (R_0); ValueError when the pair is invalid."""
        r = int(self._lib.ofps_hip_sad_reach(search_range, levels))
        if r < 0:
            raise ValueError(f"range {search_range} with levels {levels} is no valid search")
        return r

    def sad_down2(self, img: np.ndarray, stride: int | None = None) -> np.ndarray:
        """One pyramid step: [H, W] u8 -> [H >> 1, W >> 1], (a + b + c + d + 2) >> 2 of every 2 x 2 quad.  stride: None, or the row pitch in
        bytes of `img` (a view of a wider buffer)."""
        if stride is None:
            g = np.ascontiguousarray(img, np.uint8)
            stride = g.shape[1]
        else:
            g = img
            assert g.dtype == np.uint8 and g.ndim == 2 and (g.shape[0] == 1 or g.strides[0] == stride) and g.strides[1] == 1
        H, W = g.shape
        out = np.zeros((H >> 1, W >> 1), np.uint8)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.ofps_hip_sad_down2(self._h, C.cast(C.c_void_p(g.ctypes.data), u8), W, H, stride,
                                                 C.cast(C.c_void_p((out if out.size else np.zeros(1, np.uint8)).ctypes.data), u8), max(W >> 1, 1)))
        return out

    def sad_down2_dev(self, d_src: int, W: int, H: int, stride: int, d_dst: int, dst_stride: int):
        self._check(self._lib.ofps_hip_sad_down2_dev(self._h, C.c_void_p(d_src), W, H, stride, C.c_void_p(d_dst), dst_stride))

    def sad_refine(self, prev: np.ndarray, cur: np.ndarray, block: int, parent_best: np.ndarray, reach: int, want_entries=False):
        """One refinement step of the search levels: parent_best [nby_parent, nbx_parent, 3] = the coarser lattice's (dx, dy, sad) ->
        triples [nblk, 3] (and records [nblk, 4])."""
        prev = np.ascontiguousarray(prev, np.uint8); cur = np.ascontiguousarray(cur, np.uint8)
        par = np.ascontiguousarray(parent_best, np.int32)
        assert prev.shape == cur.shape and prev.ndim == 2 and par.ndim == 3 and par.shape[2] == 3
        H, W = prev.shape
        nb = int(self._lib.ofps_hip_sad_block_count(W, H, block))
        best = np.zeros((max(nb, 1), 3), np.int32)
        ent = np.zeros((max(nb, 1), 4), np.float32)
        u8 = C.POINTER(C.c_uint8); i32 = C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_sad_refine(self._h, prev.ctypes.data_as(u8), cur.ctypes.data_as(u8), W, H, W, block, par.ctypes.data_as(i32),
                                                  par.shape[1], par.shape[0], reach, best.ctypes.data_as(i32), _fp(ent) if want_entries else None))
        return (best[:nb], ent[:nb]) if want_entries else best[:nb]

    def sad_refine_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, block: int, d_parent_best: int, nbx_parent: int,
                       nby_parent: int, reach: int, d_out_best: int, d_out_entries: int | None = None):
        self._check(self._lib.ofps_hip_sad_refine_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, block, C.c_void_p(d_parent_best),
                                                      nbx_parent, nby_parent, reach, C.c_void_p(d_out_best), C.c_void_p(d_out_entries or 0)))

    SAD_PRED_PARENT, SAD_PRED_NEIGHBOURS = 0, 1

    def set_sad_predictors(self, mode: int):
        """The predictors of a refined block of the search levels (include/ofps_hip.h N1p): 0 = its parent's winner alone (default);
        1 = the parent's, its four lattice neighbours' and zero, each repaired in its own +-3 window.  No effect at levels 1."""
        self._check(self._lib.ofps_hip_set_sad_predictors(self._h, mode))

    def get_sad_predictors(self) -> int:
        return int(self._lib.ofps_hip_get_sad_predictors(self._h))

    def sad_refine_pred(self, prev: np.ndarray, cur: np.ndarray, block: int, parent_best: np.ndarray, reach: int, predictors: int, want_entries=False):
        """sad_refine with the predictor mode as an argument (0 is sad_refine)."""
        prev = np.ascontiguousarray(prev, np.uint8); cur = np.ascontiguousarray(cur, np.uint8)
        par = np.ascontiguousarray(parent_best, np.int32)
        assert prev.shape == cur.shape and prev.ndim == 2 and par.ndim == 3 and par.shape[2] == 3
        H, W = prev.shape
        nb = int(self._lib.ofps_hip_sad_block_count(W, H, block))
        best = np.zeros((max(nb, 1), 3), np.int32)
        ent = np.zeros((max(nb, 1), 4), np.float32)
        u8 = C.POINTER(C.c_uint8); i32 = C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_sad_refine_pred(self._h, prev.ctypes.data_as(u8), cur.ctypes.data_as(u8), W, H, W, block,
                                                       par.ctypes.data_as(i32), par.shape[1], par.shape[0], reach, predictors,
                                                       best.ctypes.data_as(i32), _fp(ent) if want_entries else None))
        return (best[:nb], ent[:nb]) if want_entries else best[:nb]

    def sad_refine_pred_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, block: int, d_parent_best: int, nbx_parent: int,
                            nby_parent: int, reach: int, predictors: int, d_out_best: int, d_out_entries: int | None = None):
        self._check(self._lib.ofps_hip_sad_refine_pred_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, block,
                                                           C.c_void_p(d_parent_best), nbx_parent, nby_parent, reach, predictors,
                                                           C.c_void_p(d_out_best), C.c_void_p(d_out_entries or 0)))

    def set_sad_prefilter(self, radius: int):
        """hip_sad's mean removal (include/ofps_hip.h N1m): 0 = off (default); r in [1, 16] = every search of the context runs on
        clamp(v - box mean of radius r + 128) of both frames, so a brightness change between them no longer moves the SAD minimum."""
        self._check(self._lib.ofps_hip_set_sad_prefilter(self._h, radius))

    def get_sad_prefilter(self) -> int:
        return int(self._lib.ofps_hip_get_sad_prefilter(self._h))

    def sad_prefilter(self, img: np.ndarray, radius: int, stride: int | None = None) -> np.ndarray:
        """The filter alone: [H, W] u8 -> [H, W] u8.  stride: None, or the row pitch in bytes of `img` (a view of a wider buffer)."""
        if stride is None:
            g = np.ascontiguousarray(img, np.uint8)
            stride = g.shape[1]
        else:
            g = img
            assert g.dtype == np.uint8 and g.ndim == 2 and (g.shape[0] == 1 or g.strides[0] == stride) and g.strides[1] == 1
        H, W = g.shape
        out = np.zeros((H, W), np.uint8)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.ofps_hip_sad_prefilter(self._h, C.cast(C.c_void_p(g.ctypes.data), u8), W, H, stride, radius,
                                                     C.cast(C.c_void_p(out.ctypes.data), u8), W))
        return out

    def sad_prefilter_dev(self, d_src: int, W: int, H: int, stride: int, radius: int, d_dst: int, dst_stride: int):
        self._check(self._lib.ofps_hip_sad_prefilter_dev(self._h, C.c_void_p(d_src), W, H, stride, radius, C.c_void_p(d_dst), dst_stride))

    def sad_pruned_overflow_strips(self) -> int:
        n = C.c_uint32(0)
        self._check(self._lib.ofps_hip_sad_pruned_overflow_strips(self._h, C.byref(n)))
        return int(n.value)

    def sad_flow(self, prev: np.ndarray, cur: np.ndarray, block: int, search_range: int, want_best=False):
        """-> records [n, 4] (and (dx, dy, SAD) triples [m, 3]): n = m = one per lattice block, or the kept blocks with the contrast gate and / or
        the consistency check on.  With split blocks on (N1s) n lies between kept and 4 * kept and the triples stay the kept PARENTS', m = kept
        (their number is not returned by the library: m = nblk unless a criterion drops blocks, when the caller counts them)"""
        prev = np.ascontiguousarray(prev, np.uint8); cur = np.ascontiguousarray(cur, np.uint8)
        assert prev.shape == cur.shape and prev.ndim == 2
        H, W = prev.shape
        nb = int(self._lib.ofps_hip_sad_block_count(W, H, block))
        cap = self.sad_record_capacity(W, H, block)
        if cap != nb:
            ent = np.zeros((max(cap, 1), 4), np.float32)
            best = np.zeros((max(nb, 1), 3), np.int32)
            n_out = C.c_size_t(0)
            self._check(self._lib.ofps_hip_sad_flow(self._h, prev.ctypes.data_as(C.POINTER(C.c_uint8)), cur.ctypes.data_as(C.POINTER(C.c_uint8)), W, H, W,
                                                    block, search_range, _fp(ent), best.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n_out)))
            n = int(n_out.value)
            assert n <= cap
            return (ent[:n], best[:nb]) if want_best else ent[:n]
        ent = np.zeros((max(nb, 1), 4), np.float32)
        best = np.zeros((max(nb, 1), 3), np.int32)
        n_out = C.c_size_t(0)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.ofps_hip_sad_flow(self._h, prev.ctypes.data_as(u8), cur.ctypes.data_as(u8), W, H, W,
                                                block, search_range, _fp(ent),
                                                best.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n_out)))
        n = int(n_out.value)
        assert n <= nb
        return (ent[:n], best[:n]) if want_best else ent[:n]

    def sad_flow_dev(self, d_frames: int, n_frames: int, W: int, H: int, stride: int, frame_pitch: int, ref_mode: int,
                     block: int, search_range: int, d_out_entries: int, d_out_best: int | None = None):
        self._check(self._lib.ofps_hip_sad_flow_dev(self._h, C.c_void_p(d_frames), n_frames, W, H, stride, frame_pitch,
                                                    ref_mode, block, search_range, C.c_void_p(d_out_entries),
                                                    C.c_void_p(d_out_best or 0)))

    # ---- N2
    def lk_flow(self, prev: np.ndarray, cur: np.ndarray, levels=3, radius=4, iters=3, want_entries=False):
        prev = np.ascontiguousarray(prev, np.uint8); cur = np.ascontiguousarray(cur, np.uint8)
        H, W = prev.shape
        flow = np.zeros((H, W, 2), np.float32)
        ent = np.zeros((H * W, 4), np.float32) if want_entries else None
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.ofps_hip_lk_flow(self._h, prev.ctypes.data_as(u8), cur.ctypes.data_as(u8), W, H, W, levels, radius,
                                               iters, _fp(flow), _fp(ent) if want_entries else None))
        return (flow, ent) if want_entries else flow

    def farneback_flow(self, prev: np.ndarray, cur: np.ndarray, levels=5, winsize=13, iters=3, poly_n=7, poly_sigma=1.5, init=None,
                       want_entries=False):
        """Farneback's dense flow with cv-decoder's arguments as defaults (cv-decoder/src/lib.rs:188-199) -> flow[H, W, 2]
        (dx, dy): prev(x, y) ~ cur(x + dx, y + dy) [, records[H*W, 4]].  init: None or a [H, W, 2] flow to start from."""
        prev = np.ascontiguousarray(prev, np.uint8); cur = np.ascontiguousarray(cur, np.uint8)
        H, W = prev.shape
        flow = np.zeros((H, W, 2), np.float32)
        ent = np.zeros((H * W, 4), np.float32) if want_entries else None
        ini = None if init is None else np.ascontiguousarray(init, np.float32).reshape(H, W, 2)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.ofps_hip_farneback_flow(self._h, prev.ctypes.data_as(u8), cur.ctypes.data_as(u8), W, H, W, levels, winsize, iters,
                                                      poly_n, poly_sigma, _fp(ini) if ini is not None else None, _fp(flow),
                                                      _fp(ent) if want_entries else None))
        return (flow, ent) if want_entries else flow

    def farneback_flow_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, levels=5, winsize=13, iters=3, poly_n=7,
                           poly_sigma=1.5, d_init: int | None = None, d_out_flow: int | None = None, d_out_entries: int | None = None):
        self._check(self._lib.ofps_hip_farneback_flow_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, levels, winsize, iters,
                                                          poly_n, poly_sigma, C.c_void_p(d_init or 0), C.c_void_p(d_out_flow or 0),
                                                          C.c_void_p(d_out_entries or 0)))

    def lk_spec_revision(self) -> int:
        return int(self._lib.ofps_hip_lk_spec_revision())

    def lk_helped_tiles(self) -> int:
        """Tiles of the one-launch pyramid flow that a waiting child computed itself on this context (0 on an in-order dispatcher; costs
        time, never bits; diagnostics, synchronises)."""
        n = C.c_uint64(0)
        self._check(self._lib.ofps_hip_lk_helped_tiles(self._h, C.byref(n)))
        return int(n.value)

    def flow_cache_hits(self) -> int:
        """hip_flow stream forms: calls of this context that found their first frame's pyramid + expansion already on the device."""
        n = C.c_uint64(0)
        self._check(self._lib.ofps_hip_flow_cache_hits(self._h, C.byref(n)))
        return int(n.value)

    def lk_flow_init(self, prev: np.ndarray, cur: np.ndarray, levels, radius, iters, init: np.ndarray):
        """ofps_hip_lk_flow_init_dev through library-owned device buffers: `init` [h_L, w_L, 2] is the coarsest level's
        starting flow.  -> flow[H, W, 2]."""
        prev = np.ascontiguousarray(prev, np.uint8); cur = np.ascontiguousarray(cur, np.uint8)
        init = np.ascontiguousarray(init, np.float32)
        H, W = prev.shape
        flow = np.zeros((H, W, 2), np.float32)
        bufs = [self.malloc(prev.nbytes), self.malloc(cur.nbytes), self.malloc(init.nbytes), self.malloc(flow.nbytes)]
        try:
            self.memcpy_h2d(bufs[0], prev); self.memcpy_h2d(bufs[1], cur); self.memcpy_h2d(bufs[2], init)
            self._check(self._lib.ofps_hip_lk_flow_init_dev(self._h, C.c_void_p(bufs[0]), C.c_void_p(bufs[1]), W, H, W, levels, radius,
                                                            iters, C.c_void_p(bufs[2]), C.c_void_p(bufs[3]), C.c_void_p(0)))
            self.memcpy_d2h(flow, bufs[3])
        finally:
            for b in bufs:
                self.free(b)
        return flow

    # ---- N3: hip_klt, sparse Lucas-Kanade on per-cell corner features
    KLT_KEPT, KLT_NO_FEATURE, KLT_FLAT, KLT_LEFT_FRAME, KLT_RESIDUAL = 0, 1, 2, 3, 4

    def set_klt(self, cell: int = 16, score_radius: int = 2, min_score: int = 1, min_eig: int = 1, max_residual: int = 0):
        """hip_klt's settings (include/ofps_hip.h N3): lattice cell 8 | 16 | 32, score window radius [1, 3], smallest score of a feature,
        smallest eigenvalue of a template's structure tensor per pixel [1, 65535], residual limit in sixteenths of a grey level per pixel
        [0, 4080] (0 = off)."""
        self._check(self._lib.ofps_hip_set_klt(self._h, cell, score_radius, min_score, min_eig, max_residual))

    def get_klt(self) -> dict:
        v = [C.c_int32(0) for _ in range(5)]
        self._check(self._lib.ofps_hip_get_klt(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("cell", "score_radius", "min_score", "min_eig", "max_residual"), (int(x.value) for x in v)))

    def set_klt_mean_removal(self, on: int):
        """1: every hip_klt form of this context tracks under the model "shift plus one brightness offset" and measures the residual around
        the window's mean difference (include/ofps_hip.h N3m); 0 (default): N3 as it is."""
        self._check(self._lib.ofps_hip_set_klt_mean_removal(self._h, int(on)))

    def get_klt_mean_removal(self) -> int:
        return int(self._lib.ofps_hip_get_klt_mean_removal(self._h))

    def set_klt_fb(self, limit: int):
        """hip_klt's forward-backward check (include/ofps_hip.h N3f): limit F in [0, 4096] in 1/256 pixel; a kept track is followed back from
        where it ended and dropped (status 5) unless that pass is kept too and returns to within F of the feature.  0 (default): off."""
        self._check(self._lib.ofps_hip_set_klt_fb(self._h, int(limit)))

    def get_klt_fb(self) -> int:
        return int(self._lib.ofps_hip_get_klt_fb(self._h))

    def klt_slot_count(self, W: int, H: int, cell: int | None = None) -> int:
        return int(self._lib.ofps_hip_klt_slot_count(W, H, self.get_klt()["cell"] if cell is None else cell))

    @staticmethod
    def _luma_view(img: np.ndarray, stride: int | None):
        if stride is None:
            g = np.ascontiguousarray(img, np.uint8)
            return g, g.shape[1]
        assert img.dtype == np.uint8 and img.ndim == 2 and (img.shape[0] == 1 or img.strides[0] == stride) and img.strides[1] == 1
        return img, stride

    def klt_features(self, luma: np.ndarray, stride: int | None = None) -> np.ndarray:
        """-> int32 [slots, 3]: (x, y, score) of every lattice cell's corner feature, (-1, -1, 0) for a cell without one.  stride: None, or
        the row pitch in bytes of `luma` (a view of a wider buffer)."""
        g, stride = self._luma_view(luma, stride)
        H, W = g.shape
        out = np.zeros((max(self.klt_slot_count(W, H), 1), 3), np.int32)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.ofps_hip_klt_features(self._h, C.cast(C.c_void_p(g.ctypes.data), u8), W, H, stride,
                                                    out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out[:self.klt_slot_count(W, H)]

    def klt_features_dev(self, d_luma: int, W: int, H: int, stride: int, d_out_triples: int):
        self._check(self._lib.ofps_hip_klt_features_dev(self._h, C.c_void_p(d_luma), W, H, stride, C.c_void_p(d_out_triples)))

    def klt_track(self, prev: np.ndarray, cur: np.ndarray, points: np.ndarray, levels: int, radius: int, iters: int,
                  stride: int | None = None) -> np.ndarray:
        """points int [n, 2] (x, y) inside the frame -> int32 [n, 4]: (dqx, dqy, res, status), dq in 1/256 pixel"""
        p, stride = self._luma_view(prev, stride)
        c, stride_c = self._luma_view(cur, stride)
        assert p.shape == c.shape and stride == stride_c
        H, W = p.shape
        pts = np.ascontiguousarray(points, np.int32).reshape(-1, 2)
        out = np.zeros((max(len(pts), 1), 4), np.int32)
        u8, i32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_klt_track(self._h, C.cast(C.c_void_p(p.ctypes.data), u8), C.cast(C.c_void_p(c.ctypes.data), u8), W, H,
                                                 stride, pts.ctypes.data_as(i32) if len(pts) else None, len(pts), levels, radius, iters,
                                                 out.ctypes.data_as(i32)))
        return out[:len(pts)]

    def klt_track_q(self, prev: np.ndarray, cur: np.ndarray, points: np.ndarray, levels: int, radius: int, iters: int,
                    stride: int | None = None) -> np.ndarray:
        """N3f's stage form: points int [n, 2] (Px, Py) in 1/256 pixel inside the frame -> int32 [n, 4]: (dqx, dqy, res, status); one direction,
        from prev into cur, never checked"""
        p, stride = self._luma_view(prev, stride)
        c, stride_c = self._luma_view(cur, stride)
        assert p.shape == c.shape and stride == stride_c
        H, W = p.shape
        pts = np.ascontiguousarray(points, np.int32).reshape(-1, 2)
        out = np.zeros((max(len(pts), 1), 4), np.int32)
        u8, i32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_klt_track_q(self._h, C.cast(C.c_void_p(p.ctypes.data), u8), C.cast(C.c_void_p(c.ctypes.data), u8), W, H,
                                                   stride, pts.ctypes.data_as(i32) if len(pts) else None, len(pts), levels, radius, iters,
                                                   out.ctypes.data_as(i32)))
        return out[:len(pts)]

    def klt_track_q_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, d_points: int, n: int, levels: int, radius: int, iters: int,
                        d_out_quads: int):
        """Enqueue only; a position outside the frame comes back with status 3."""
        self._check(self._lib.ofps_hip_klt_track_q_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, C.c_void_p(d_points), n,
                                                       levels, radius, iters, C.c_void_p(d_out_quads)))

    def klt_track_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, d_points: int, n: int, levels: int, radius: int, iters: int,
                      d_out_quads: int):
        """Enqueue only; a point outside the frame comes back with status 3."""
        self._check(self._lib.ofps_hip_klt_track_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, C.c_void_p(d_points), n,
                                                     levels, radius, iters, C.c_void_p(d_out_quads)))

    def klt_flow(self, prev: np.ndarray, cur: np.ndarray, levels: int, radius: int, iters: int, want_slots=False, stride: int | None = None):
        """-> entries float32 [count, 4] (the kept features' records, in slot order) [, slots int32 [slots, 6]: (x, y, score, dqx, dqy, status)]"""
        p, stride = self._luma_view(prev, stride)
        c, stride_c = self._luma_view(cur, stride)
        assert p.shape == c.shape and stride == stride_c
        H, W = p.shape
        ns = self.klt_slot_count(W, H)
        ent = np.zeros((max(ns, 1), 4), np.float32)
        slots = np.zeros((max(ns, 1), 6), np.int32) if want_slots else None
        n = C.c_uint32(0)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.ofps_hip_klt_flow(self._h, C.cast(C.c_void_p(p.ctypes.data), u8), C.cast(C.c_void_p(c.ctypes.data), u8), W, H,
                                                stride, levels, radius, iters, _fp(ent), C.byref(n),
                                                slots.ctypes.data_as(C.POINTER(C.c_int32)) if want_slots else None))
        return (ent[:n.value], slots[:ns]) if want_slots else ent[:n.value]

    def klt_flow_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, levels: int, radius: int, iters: int, d_out_entries: int,
                     d_out_count: int, d_out_slots: int | None = None):
        """Enqueue only: d_out_entries holds klt_slot_count records, d_out_count one uint32, d_out_slots (optional) 6 int32 per slot."""
        self._check(self._lib.ofps_hip_klt_flow_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, levels, radius, iters,
                                                    C.c_void_p(d_out_entries), C.c_void_p(d_out_count), C.c_void_p(d_out_slots or 0)))

    # ---- N3p: hip_klt with motion prediction
    def set_klt_prediction(self, on: int):
        """1: the sparse stream forms (OFPS_HIP_FLOW_SPARSE) start every pair's tracks from the previous pair's flow (include/ofps_hip.h N3p);
        0 (default): every track starts from zero.  The batch forms and the stage forms do not read it."""
        self._check(self._lib.ofps_hip_set_klt_prediction(self._h, int(on)))

    def get_klt_prediction(self) -> int:
        return int(self._lib.ofps_hip_get_klt_prediction(self._h))

    def klt_predict(self, prev_slots: np.ndarray, W: int, H: int, cell: int | None = None) -> np.ndarray:
        """The predictor alone: the previous pair's raw slots int32 [slots, 6] on the W x H lattice -> int32 [slots, 2], the guess (gx, gy) of
        every slot in 1/256 pixel"""
        cell = self.get_klt()["cell"] if cell is None else cell
        ns = self.klt_slot_count(W, H, cell)
        ps = np.ascontiguousarray(prev_slots, np.int32).reshape(-1, 6)
        assert len(ps) == ns
        out = np.zeros((max(ns, 1), 2), np.int32)
        i32 = C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_klt_predict(self._h, ps.ctypes.data_as(i32), W, H, cell, out.ctypes.data_as(i32)))
        return out[:ns]

    def klt_predict_dev(self, d_prev_slots: int, W: int, H: int, cell: int, d_out_guesses: int):
        self._check(self._lib.ofps_hip_klt_predict_dev(self._h, C.c_void_p(d_prev_slots), W, H, cell, C.c_void_p(d_out_guesses)))

    def klt_track_from(self, prev: np.ndarray, cur: np.ndarray, points: np.ndarray, guesses: np.ndarray, levels: int, radius: int, iters: int,
                       stride: int | None = None) -> np.ndarray:
        """klt_track with one guess per point: guesses int [n, 2] (gx, gy) in 1/256 pixel, within +-2^23 -> int32 [n, 4]: (dqx, dqy, res,
        status), dq the whole displacement"""
        p, stride = self._luma_view(prev, stride)
        c, stride_c = self._luma_view(cur, stride)
        assert p.shape == c.shape and stride == stride_c
        H, W = p.shape
        pts = np.ascontiguousarray(points, np.int32).reshape(-1, 2)
        gs = np.ascontiguousarray(guesses, np.int32).reshape(-1, 2)
        assert len(gs) == len(pts)
        out = np.zeros((max(len(pts), 1), 4), np.int32)
        u8, i32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_klt_track_from(self._h, C.cast(C.c_void_p(p.ctypes.data), u8), C.cast(C.c_void_p(c.ctypes.data), u8), W, H,
                                                      stride, pts.ctypes.data_as(i32) if len(pts) else None,
                                                      gs.ctypes.data_as(i32) if len(pts) else None, len(pts), levels, radius, iters,
                                                      out.ctypes.data_as(i32)))
        return out[:len(pts)]

    def klt_track_from_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, d_points: int, d_guesses: int, n: int, levels: int,
                           radius: int, iters: int, d_out_quads: int):
        """Enqueue only; a point outside the frame comes back with status 3, a guess beyond +-2^23 counts as (0, 0)."""
        self._check(self._lib.ofps_hip_klt_track_from_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, C.c_void_p(d_points),
                                                          C.c_void_p(d_guesses), n, levels, radius, iters, C.c_void_p(d_out_quads)))

    def klt_flow_from(self, prev: np.ndarray, cur: np.ndarray, levels: int, radius: int, iters: int, prev_slots: np.ndarray | None = None,
                      want_slots=True, stride: int | None = None):
        """klt_flow whose features start from the guesses predicted from prev_slots (the previous call's slots; None: from zero).
        -> entries float32 [count, 4] [, slots int32 [slots, 6]]"""
        p, stride = self._luma_view(prev, stride)
        c, stride_c = self._luma_view(cur, stride)
        assert p.shape == c.shape and stride == stride_c
        H, W = p.shape
        ns = self.klt_slot_count(W, H)
        ent = np.zeros((max(ns, 1), 4), np.float32)
        slots = np.zeros((max(ns, 1), 6), np.int32) if want_slots else None
        ps = None
        if prev_slots is not None:
            ps = np.ascontiguousarray(prev_slots, np.int32).reshape(-1, 6)
            assert len(ps) == ns
        n = C.c_uint32(0)
        u8, i32 = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_klt_flow_from(self._h, C.cast(C.c_void_p(p.ctypes.data), u8), C.cast(C.c_void_p(c.ctypes.data), u8), W, H,
                                                     stride, levels, radius, iters, ps.ctypes.data_as(i32) if ps is not None else None,
                                                     _fp(ent), C.byref(n), slots.ctypes.data_as(i32) if want_slots else None))
        return (ent[:n.value], slots[:ns]) if want_slots else ent[:n.value]

    def klt_flow_from_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, levels: int, radius: int, iters: int,
                          d_prev_slots: int | None, d_out_entries: int, d_out_count: int, d_out_slots: int | None = None):
        """Enqueue only: klt_flow_dev with the previous pair's slots in device memory (None: klt_flow_dev itself)."""
        self._check(self._lib.ofps_hip_klt_flow_from_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, levels, radius, iters,
                                                         C.c_void_p(d_prev_slots or 0), C.c_void_p(d_out_entries), C.c_void_p(d_out_count),
                                                         C.c_void_p(d_out_slots or 0)))

    # ---- N3b: hip_klt on a batch of pairs, and as the batched stream forms' decoder
    BATCH_DECODER_SAD, BATCH_DECODER_KLT = 0, 1

    def klt_flow_batch(self, frames: np.ndarray, levels: int, radius: int, iters: int, ref_mode: int = 0, want_slots=False):
        """frames uint8 [n_frames, H, W] (a view with padded rows and frames further apart is passed as it is); item k = the pair (k, k + 1),
        or (0, k + 1) with ref_mode 1 -> (entries float32 [pairs, slots, 4], counts uint32 [pairs][, slots int32 [pairs, slots, 6]]).  Item k's
        kept records are entries[k, :counts[k]]; the rows behind them are not written."""
        assert frames.dtype == np.uint8 and frames.ndim == 3
        n, H, W = frames.shape
        pitch, stride, unit = frames.strides
        assert unit == 1 and stride >= W, "frames: rows must be byte-contiguous"
        pairs, ns = max(n - 1, 0), self.klt_slot_count(W, H)
        ent = np.zeros((max(pairs, 1), max(ns, 1), 4), np.float32)
        counts = np.zeros(max(pairs, 1), np.uint32)
        slots = np.zeros((max(pairs, 1), max(ns, 1), 6), np.int32) if want_slots else None
        self._check(self._lib.ofps_hip_klt_flow_batch(self._h, C.cast(C.c_void_p(frames.ctypes.data), C.POINTER(C.c_uint8)), n, W, H, stride,
                                                      pitch if n > 1 else stride * H, ref_mode, levels, radius, iters, _fp(ent),
                                                      counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                      slots.ctypes.data_as(C.POINTER(C.c_int32)) if want_slots else None))
        return (ent[:pairs], counts[:pairs], slots[:pairs]) if want_slots else (ent[:pairs], counts[:pairs])

    def klt_flow_batch_dev(self, d_frames: int, n_frames: int, W: int, H: int, stride: int, frame_pitch: int, ref_mode: int, levels: int,
                           radius: int, iters: int, d_out_entries: int, d_out_counts: int, d_out_slots: int | None = None):
        """Enqueue only: d_out_entries holds pairs x klt_slot_count records, d_out_counts pairs uint32, d_out_slots (optional) 6 int32 per slot."""
        self._check(self._lib.ofps_hip_klt_flow_batch_dev(self._h, C.c_void_p(d_frames), n_frames, W, H, stride, frame_pitch, ref_mode, levels,
                                                          radius, iters, C.c_void_p(d_out_entries), C.c_void_p(d_out_counts),
                                                          C.c_void_p(d_out_slots or 0)))

    # ---- N3pb: motion prediction in the batch form and the batched stream
    def set_klt_batch_prediction(self, on: int):
        """1, with set_klt_prediction(1) as well: klt_flow_batch[_dev] and push_frames_async with the batch decoder at KLT chain their items,
        each started from the item before, across tickets too (include/ofps_hip.h N3pb); 0 (default): they ignore the prediction setting."""
        self._check(self._lib.ofps_hip_set_klt_batch_prediction(self._h, int(on)))

    def get_klt_batch_prediction(self) -> int:
        return int(self._lib.ofps_hip_get_klt_batch_prediction(self._h))

    def klt_flow_batch_from(self, frames: np.ndarray, levels: int, radius: int, iters: int, ref_mode: int = 0, prev_slots: np.ndarray | None = None,
                            want_slots=True):
        """klt_flow_batch, chained: item k starts from the guesses predicted from item k - 1's slots, item 0 from prev_slots' (int32
        [slots, 6]; None: from zero).  Reads neither prediction setting.  -> (entries, counts[, slots]) as klt_flow_batch"""
        assert frames.dtype == np.uint8 and frames.ndim == 3
        n, H, W = frames.shape
        pitch, stride, unit = frames.strides
        assert unit == 1 and stride >= W, "frames: rows must be byte-contiguous"
        pairs, ns = max(n - 1, 0), self.klt_slot_count(W, H)
        ent = np.zeros((max(pairs, 1), max(ns, 1), 4), np.float32)
        counts = np.zeros(max(pairs, 1), np.uint32)
        slots = np.zeros((max(pairs, 1), max(ns, 1), 6), np.int32) if want_slots else None
        ps = None
        if prev_slots is not None:
            ps = np.ascontiguousarray(prev_slots, np.int32).reshape(-1, 6)
            assert len(ps) == ns
        i32 = C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_klt_flow_batch_from(self._h, C.cast(C.c_void_p(frames.ctypes.data), C.POINTER(C.c_uint8)), n, W, H, stride,
                                                           pitch if n > 1 else stride * H, ref_mode, levels, radius, iters, _fp(ent),
                                                           counts.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                           slots.ctypes.data_as(i32) if want_slots else None,
                                                           ps.ctypes.data_as(i32) if ps is not None else None))
        return (ent[:pairs], counts[:pairs], slots[:pairs]) if want_slots else (ent[:pairs], counts[:pairs])

    def klt_flow_batch_from_dev(self, d_frames: int, n_frames: int, W: int, H: int, stride: int, frame_pitch: int, ref_mode: int, levels: int,
                                radius: int, iters: int, d_out_entries: int, d_out_counts: int, d_out_slots: int | None = None,
                                d_prev_slots: int | None = None):
        """Enqueue only: klt_flow_batch_dev, chained, with the slots item 0 starts from in device memory (None: from zero); they must not overlap
        d_out_slots."""
        self._check(self._lib.ofps_hip_klt_flow_batch_from_dev(self._h, C.c_void_p(d_frames), n_frames, W, H, stride, frame_pitch, ref_mode, levels,
                                                               radius, iters, C.c_void_p(d_out_entries), C.c_void_p(d_out_counts),
                                                               C.c_void_p(d_out_slots or 0), C.c_void_p(d_prev_slots or 0)))

    # ---- N3i: hip_klt's intra test and scene-cut rule
    def set_klt_intra(self, ratio: int):
        """hip_klt's intra test (include/ofps_hip.h N3i): 0 = off (default); q in [1, 255] (sixteenths) = a kept track whose residual reaches
        q/16 of its window's activity in the raw previous frame (16 * res >= q * 256 * A) becomes status 6 and yields no record, in every form
        that runs the decoder."""
        self._check(self._lib.ofps_hip_set_klt_intra(self._h, int(ratio)))

    def get_klt_intra(self) -> int:
        return int(self._lib.ofps_hip_get_klt_intra(self._h))

    def set_klt_cut(self, percent: int):
        """hip_klt's scene-cut rule (N3i): 0 = off (default); P in [1, 100] = a pair with at least P percent of its candidates intra yields no
        record at all, its statuses 0 become 7.  No effect while the intra ratio is 0."""
        self._check(self._lib.ofps_hip_set_klt_cut(self._h, int(percent)))

    def get_klt_cut(self) -> int:
        return int(self._lib.ofps_hip_get_klt_cut(self._h))

    def klt_activity(self, luma: np.ndarray, points: np.ndarray, radius: int, stride: int | None = None) -> np.ndarray:
        """points int [n, 2] (x, y) inside the frame -> uint32 [n]: sum |p - rounded window mean| over each point's (2 radius + 1)^2 window,
        pixel indices clamped into the frame"""
        g, stride = self._luma_view(luma, stride)
        H, W = g.shape
        pts = np.ascontiguousarray(points, np.int32).reshape(-1, 2)
        out = np.zeros(max(len(pts), 1), np.uint32)
        self._check(self._lib.ofps_hip_klt_activity(self._h, C.cast(C.c_void_p(g.ctypes.data), C.POINTER(C.c_uint8)), W, H, stride,
                                                    pts.ctypes.data_as(C.POINTER(C.c_int32)) if len(pts) else None, len(pts), radius,
                                                    out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out[:len(pts)]

    def klt_activity_dev(self, d_luma: int, W: int, H: int, stride: int, d_points: int, n: int, radius: int, d_out_activity: int):
        """Enqueue only; a point outside the frame comes back with A = 0."""
        self._check(self._lib.ofps_hip_klt_activity_dev(self._h, C.c_void_p(d_luma), W, H, stride, C.c_void_p(d_points), n, radius,
                                                        C.c_void_p(d_out_activity)))

    def klt_intra(self, quads: np.ndarray, activity: np.ndarray, ratio: int, cut: int = 0, want_counts=True):
        """Verdict and cut rule alone on [n, 4] quads (dqx, dqy, res, status) and the points' activities -> (statuses int32 [n],
        [n_cand, n_intra] uint32 or None)."""
        q = np.ascontiguousarray(quads, np.int32).reshape(-1, 4)
        a = np.ascontiguousarray(activity, np.uint32).reshape(-1)
        assert len(q) == len(a)
        st = np.zeros(max(len(q), 1), np.int32)
        counts = np.zeros(2, np.uint32) if want_counts else None
        i32, u32 = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        self._check(self._lib.ofps_hip_klt_intra(self._h, q.ctypes.data_as(i32) if len(q) else None, a.ctypes.data_as(u32) if len(q) else None, len(q),
                                                 ratio, cut, st.ctypes.data_as(i32), counts.ctypes.data_as(u32) if want_counts else None))
        return st[:len(q)], counts

    def klt_intra_dev(self, d_quads: int, d_activity: int, n: int, ratio: int, cut: int, d_out_status: int, d_out_counts: int | None = None):
        self._check(self._lib.ofps_hip_klt_intra_dev(self._h, C.c_void_p(d_quads), C.c_void_p(d_activity), n, ratio, cut, C.c_void_p(d_out_status),
                                                     C.c_void_p(d_out_counts or 0)))

    def set_batch_decoder(self, decoder: int = 0, levels: int = 4, radius: int = 7, iters: int = 10):
        """What push_frames_async searches with: BATCH_DECODER_SAD (default), or BATCH_DECODER_KLT with these levels, window radius and
        iterations and the set_klt values (include/ofps_hip.h N3b)."""
        self._check(self._lib.ofps_hip_set_batch_decoder(self._h, decoder, levels, radius, iters))

    def get_batch_decoder(self) -> dict:
        v = [C.c_int32(0) for _ in range(4)]
        self._check(self._lib.ofps_hip_get_batch_decoder(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("decoder", "levels", "radius", "iters"), (int(x.value) for x in v)))

    def batch_record_capacity(self, W: int, H: int, block: int = 16) -> int:
        """records per frame of push_frames_async's out_entries: the slot count with the batch decoder at KLT, else the block count"""
        if self.get_batch_decoder()["decoder"] == self.BATCH_DECODER_KLT:
            return self.klt_slot_count(W, H)
        return int(self._lib.ofps_hip_sad_block_count(W, H, block))

    LK_CONTRAST_MASK, LK_FULLRES_RECORDS, FLOW_FARNEBACK, FLOW_USE_PREVIOUS, LK_REDUCED = 1, 2, 4, 8, 16
    FLOW_SPARSE = 32            # hip_klt (include/ofps_hip.h N3) in place of flow, mask and output stage; levels / radius / iters = L / w / K
    FMT_LUMA, FMT_BGR, FMT_RGBA, FMT_BGRA = 0, 1, 2, 3

    def _lk_flags(self, contrast_mask, fullres_records, farneback, use_previous, reduced, fmt, sparse=False) -> int:
        return ((self.FLOW_SPARSE if sparse else 0) | (self.LK_CONTRAST_MASK if contrast_mask else 0) | (self.LK_FULLRES_RECORDS if fullres_records else 0) |
                (self.FLOW_FARNEBACK if farneback else 0) | (self.FLOW_USE_PREVIOUS if use_previous else 0) |
                (self.LK_REDUCED if reduced else 0) | (int(fmt) << 8))

    def _frame_geometry(self, frame: np.ndarray, fmt: int):
        """-> (W, H, row pitch in bytes) of a C-contiguous u8 frame [H, W] (luma) or [H, W, channels]"""
        cn = int(self._lib.ofps_hip_frame_channels(int(fmt)))
        if cn == 0:
            raise ValueError(f"unknown frame format {fmt}")
        if (frame.ndim == 2 and cn != 1) or (frame.ndim == 3 and frame.shape[2] != cn) or frame.ndim not in (2, 3):
            raise ValueError(f"frame of shape {frame.shape} is not a format-{fmt} frame ({cn} bytes per pixel)")
        H, W = frame.shape[:2]
        return W, H, W * cn

    def _lk_capacity(self, W, H, max_w, max_h, fullres_records, reduced=False, sparse=False) -> int:
        if sparse:                                            # hip_klt: the slot count of the frames the tracker reads
            fw, fh = self.cv_grid(W, H, max_w, max_h) if reduced else (W, H)
            return max(self.klt_slot_count(fw, fh), 1)
        return W * H if fullres_records else min(max_w, W) * min(max_h, H)

    def cv_grid(self, W: int, H: int, max_w: int = 150, max_h: int = 150):
        """cv-decoder/src/lib.rs:98-121: the capped record grid (and the size "Process Fullres" = false resizes the frames to)."""
        gw = C.c_int(0); gh = C.c_int(0)
        rc = self._lib.ofps_hip_cv_grid(W, H, max_w, max_h, C.byref(gw), C.byref(gh))
        if rc != 0:
            raise ValueError("ofps_hip_cv_grid: bad arguments")
        return gw.value, gh.value

    def resize_linear(self, img: np.ndarray, dw: int, dh: int, fmt: int = 0) -> np.ndarray:
        """imgproc::resize(.., INTER_LINEAR) of an 8-bit frame, channels kept (cv-decoder/src/lib.rs:124-133)."""
        img = np.ascontiguousarray(img, np.uint8)
        W, H, pitch = self._frame_geometry(img, fmt)
        out = np.zeros((dh, dw) + img.shape[2:], np.uint8)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.ofps_hip_resize_linear(self._h, img.ctypes.data_as(u8), W, H, pitch, int(fmt), out.ctypes.data_as(u8), dw, dh))
        return out

    def cv_frontend(self, frame: np.ndarray, fmt: int = 0, reduced: bool = False, max_w: int = 150, max_h: int = 150) -> np.ndarray:
        """[resize to the capped grid ->] gray: what cv-decoder leaves in `self.gray` for one frame (cv-decoder/src/lib.rs:98-135)."""
        frame = np.ascontiguousarray(frame, np.uint8)
        W, H, pitch = self._frame_geometry(frame, fmt)
        out = np.zeros(W * H, np.uint8)
        ow = C.c_int(0); oh = C.c_int(0)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.ofps_hip_cv_frontend(self._h, frame.ctypes.data_as(u8), W, H, pitch, int(fmt), int(bool(reduced)), max_w, max_h,
                                                   out.ctypes.data_as(u8), C.byref(ow), C.byref(oh)))
        return out[:ow.value * oh.value].reshape(oh.value, ow.value).copy()

    def cv_frontend_dev(self, d_frame: int, W: int, H: int, stride: int, fmt: int, reduced: bool, max_w: int, max_h: int, d_out_gray: int):
        ow = C.c_int(0); oh = C.c_int(0)
        self._check(self._lib.ofps_hip_cv_frontend_dev(self._h, C.c_void_p(d_frame), W, H, stride, int(fmt), int(bool(reduced)), max_w, max_h,
                                                       C.c_void_p(d_out_gray), C.byref(ow), C.byref(oh)))
        return ow.value, oh.value

    def lk_decode(self, prev: np.ndarray, cur: np.ndarray, levels=3, radius=4, iters=3, max_w=150, max_h=150, farneback=False, use_previous=False,
                  contrast_mask=False, fullres_records=False, reduced=False, fmt=0, *, sparse=False):
        """-> (entries[n,4], (grid_w, grid_h)): what a hip_lk Decoder appends per frame (cv-decoder/src/lib.rs:82-294).
        reduced: cv-decoder's "Process Fullres" = false; fmt: the frames' pixel format (FMT_*; colour frames are [H, W, channels])."""
        prev = np.ascontiguousarray(prev, np.uint8); cur = np.ascontiguousarray(cur, np.uint8)
        assert prev.shape == cur.shape
        W, H, pitch = self._frame_geometry(prev, fmt)
        out = np.zeros((self._lk_capacity(W, H, max_w, max_h, fullres_records, reduced, sparse), 4), np.float32)
        n = C.c_size_t(0); gw = C.c_int(0); gh = C.c_int(0)
        u8 = C.POINTER(C.c_uint8)
        flags = self._lk_flags(contrast_mask, fullres_records, farneback, use_previous, reduced, fmt, sparse)
        self._check(self._lib.ofps_hip_lk_decode(self._h, prev.ctypes.data_as(u8), cur.ctypes.data_as(u8), W, H, pitch, levels, radius,
                                                 iters, max_w, max_h, flags, _fp(out), C.byref(n), C.byref(gw), C.byref(gh)))
        return out[:n.value].copy(), (gw.value, gh.value)

    def lk_push_frame(self, frame: np.ndarray, levels=3, radius=4, iters=3, max_w=150, max_h=150, contrast_mask=False,
                      fullres_records=False, farneback=False, use_previous=False, reduced=False, fmt=0, *, sparse=False):
        """Stream form of lk_decode: the frame is uploaded once and is the next call's previous frame.
        -> None for the first frame of a stream, else (entries[n,4], (grid_w, grid_h))."""
        frame = np.ascontiguousarray(frame, np.uint8)
        W, H, pitch = self._frame_geometry(frame, fmt)
        out = np.zeros((self._lk_capacity(W, H, max_w, max_h, fullres_records, reduced, sparse), 4), np.float32)
        n = C.c_size_t(0); gw = C.c_int(0); gh = C.c_int(0); have = C.c_int(0)
        flags = self._lk_flags(contrast_mask, fullres_records, farneback, use_previous, reduced, fmt, sparse)
        self._check(self._lib.ofps_hip_lk_push_frame(self._h, frame.ctypes.data_as(C.POINTER(C.c_uint8)), W, H, pitch, levels, radius,
                                                     iters, max_w, max_h, flags, _fp(out), C.byref(n), C.byref(gw), C.byref(gh),
                                                     C.byref(have)))
        if not have.value:
            return None
        return out[:n.value].copy(), (gw.value, gh.value)

    def lk_push_frame_async(self, frame: np.ndarray, levels=3, radius=4, iters=3, max_w=150, max_h=150, contrast_mask=False,
                            fullres_records=False, farneback=False, use_previous=False, reduced=False, fmt=0, *, sparse=False) -> int:
        """Read-ahead form: returns a ticket once the upload, the flow and the output stage are enqueued.  `frame` must be
        C-contiguous u8 and stay alive (ideally page-locked: pinned_frame) until lk_frame_wait(ticket)."""
        assert frame.dtype == np.uint8 and frame.flags["C_CONTIGUOUS"]
        W, H, pitch = self._frame_geometry(frame, fmt)
        flags = self._lk_flags(contrast_mask, fullres_records, farneback, use_previous, reduced, fmt, sparse)
        t = C.c_int(0)
        self._check(self._lib.ofps_hip_lk_push_frame_async(self._h, frame.ctypes.data_as(C.POINTER(C.c_uint8)), W, H, pitch, levels, radius,
                                                           iters, max_w, max_h, flags, C.byref(t)))
        self._lk_cap = getattr(self, "_lk_cap", {})
        self._lk_cap[t.value] = self._lk_capacity(W, H, max_w, max_h, fullres_records, reduced, sparse)
        return t.value

    def lk_frame_wait(self, ticket: int, out: np.ndarray | None = None):
        """-> None for the first frame of a stream, else (entries[n,4], (grid_w, grid_h)).  `out`: a caller buffer of the
        capacity lk_decode documents (the result is then a view of it)."""
        cap = getattr(self, "_lk_cap", {}).pop(ticket, 1)    # an unknown ticket: the library says so
        getattr(self, "_lk_dim", {}).pop(ticket, None)       # (a fused ticket collected here: its tail is dropped)
        if out is None:
            out = np.zeros((cap, 4), np.float32)
        assert out.dtype == np.float32 and out.size >= 4 * cap and out.flags["C_CONTIGUOUS"]
        n = C.c_size_t(0); gw = C.c_int(0); gh = C.c_int(0); have = C.c_int(0)
        self._check(self._lib.ofps_hip_lk_frame_wait(self._h, ticket, _fp(out), C.byref(n), C.byref(gw), C.byref(gh), C.byref(have)))
        if not have.value:
            return None
        return out.reshape(-1, 4)[:n.value], (gw.value, gh.value)

    # ---- the dense decoders with detector + estimator behind them in the same ticket (ofps_hip_lk_push_frame_fused[_async])
    def _fused_result(self, res, ent, fld, grid, islands=False):
        have = bool(res.have_vectors)
        n = int(res.n_vectors)
        motion = (int(res.area), fld) if res.has_motion else None
        out = {"have_vectors": have, "n_vectors": n, "motion": motion, "quat": np.array(list(res.quat), np.float32),
               "entries": ent[:n] if (ent is not None and have) else None, "grid": grid}
        if islands:
            out["islands"] = self.frame_islands(0)
        if islands == 2:
            out["tracks"] = self.frame_tracks(0)
        return out

    def lk_push_frame_fused_async(self, frame: np.ndarray, levels=3, radius=4, iters=3, max_w=150, max_h=150, contrast_mask=False,
                                  farneback=False, use_previous=False, reduced=False, fmt=0, fullres_records=False, detector=True,
                                  min_size=0.05, subdivide=3, target_motion=0.003, estimator=True, aspect=16 / 9, fov_y_deg=39.6 * 9 / 16,
                                  use_ransac=False, num_iters=200, inlier_deg=0.05, num_samples=1000, seed=0, *, sparse=False) -> int:
        """Read-ahead form of lk_push_frame_fused: -> ticket once upload, flow, output stage, detector and estimator are enqueued.
        `frame` as for lk_push_frame_async; collect with lk_frame_fused_wait (or lk_frame_wait: the records alone)."""
        assert frame.dtype == np.uint8 and frame.flags["C_CONTIGUOUS"]
        W, H, pitch = self._frame_geometry(frame, fmt)
        flags = self._lk_flags(contrast_mask, fullres_records, farneback, use_previous, reduced, fmt, sparse)
        prm = self._frame_params(0, 0, detector, min_size, subdivide, target_motion, estimator, aspect, fov_y_deg, use_ransac, num_iters,
                                 inlier_deg, num_samples, seed)
        t = C.c_int(0)
        self._check(self._lib.ofps_hip_lk_push_frame_fused_async(self._h, frame.ctypes.data_as(C.POINTER(C.c_uint8)), W, H, pitch, levels,
                                                                 radius, iters, max_w, max_h, flags, C.byref(prm), C.byref(t)))
        self._lk_cap = getattr(self, "_lk_cap", {})
        self._lk_cap[t.value] = self._lk_capacity(W, H, max_w, max_h, fullres_records, reduced, sparse)
        self._lk_dim = getattr(self, "_lk_dim", {})
        self._lk_dim[t.value] = self.block_dim(min_size, subdivide) if detector else 0
        self._lk_isl = getattr(self, "_lk_isl", {})
        self._lk_isl[t.value] = self._ticket_islands(detector)
        return t.value

    def lk_frame_fused_wait(self, ticket: int, want_entries=True, want_field=True) -> dict:
        """-> dict(have_vectors, n_vectors, motion=None|(area, field|None), quat, entries|None, grid): push_frame's shape plus the record
        grid.  A ticket of the plain lk_push_frame_async comes back with the identity and no motion."""
        cap = getattr(self, "_lk_cap", {}).pop(ticket, 1)
        dim = getattr(self, "_lk_dim", {}).pop(ticket, 0)
        ent = np.zeros((cap, 4), np.float32) if want_entries else None
        fld = np.zeros((dim, dim, 2), np.float32) if (want_field and dim) else None
        res = _lib.FrameResult(); gw = C.c_int(0); gh = C.c_int(0)
        self._check(self._lib.ofps_hip_lk_frame_fused_wait(self._h, ticket, C.byref(res), _fp(ent) if ent is not None else None,
                                                           _fp(fld) if fld is not None else None, C.byref(gw), C.byref(gh)))
        return self._fused_result(res, ent, fld, (gw.value, gh.value), getattr(self, "_lk_isl", {}).pop(ticket, False))

    def lk_push_frame_fused(self, frame: np.ndarray, levels=3, radius=4, iters=3, max_w=150, max_h=150, contrast_mask=False,
                            farneback=False, use_previous=False, reduced=False, fmt=0, fullres_records=False, detector=True, min_size=0.05,
                            subdivide=3, target_motion=0.003, estimator=True, aspect=16 / 9, fov_y_deg=39.6 * 9 / 16, use_ransac=False,
                            num_iters=200, inlier_deg=0.05, num_samples=1000, seed=0, want_entries=True, want_field=True, *, sparse=False) -> dict:
        """One frame of a hip_lk / hip_flow stream -> records -> island + rotation in one call, the records staying on the device in
        between (ofps_hip_lk_push_frame_fused).  The same stream of frames as lk_push_frame."""
        frame = np.ascontiguousarray(frame, np.uint8)
        W, H, pitch = self._frame_geometry(frame, fmt)
        flags = self._lk_flags(contrast_mask, fullres_records, farneback, use_previous, reduced, fmt, sparse)
        prm = self._frame_params(0, 0, detector, min_size, subdivide, target_motion, estimator, aspect, fov_y_deg, use_ransac, num_iters,
                                 inlier_deg, num_samples, seed)
        dim = self.block_dim(min_size, subdivide) if detector else 0
        ent = np.zeros((self._lk_capacity(W, H, max_w, max_h, fullres_records, reduced, sparse), 4), np.float32) if want_entries else None
        fld = np.zeros((dim, dim, 2), np.float32) if (want_field and dim) else None
        res = _lib.FrameResult(); gw = C.c_int(0); gh = C.c_int(0)
        self._check(self._lib.ofps_hip_lk_push_frame_fused(self._h, frame.ctypes.data_as(C.POINTER(C.c_uint8)), W, H, pitch, levels, radius,
                                                           iters, max_w, max_h, flags, C.byref(prm), C.byref(res),
                                                           _fp(ent) if ent is not None else None, _fp(fld) if fld is not None else None,
                                                           C.byref(gw), C.byref(gh)))
        return self._fused_result(res, ent, fld, (gw.value, gh.value), self._ticket_islands(detector))

    def lk_reset(self):
        self._check(self._lib.ofps_hip_lk_reset(self._h))

    def lk_rewind(self):
        """forget the stream's frames, keep its last flow as the next pair's initial flow (a decoder that skipped frames)"""
        self._check(self._lib.ofps_hip_lk_rewind(self._h))

    def contrast_mask(self, gray: np.ndarray, stride: int | None = None) -> np.ndarray:
        """cv-decoder's Sobel/threshold/dilate mask (cv-decoder/src/lib.rs:203-237) -> u8[H, W], 1 = keep (dense: W bytes per row).
        stride: `gray` is a u8 view [H, W] whose rows lie `stride` >= W bytes apart (e.g. buf[:, :W]); it is passed as it is."""
        if stride is None:
            g = np.ascontiguousarray(gray, np.uint8)
            stride = g.shape[1]
        else:
            g = gray
            assert g.dtype == np.uint8 and g.ndim == 2 and (g.shape[0] == 1 or g.strides[0] == stride) and g.strides[1] == 1
        H, W = g.shape
        out = np.zeros((H, W), np.uint8)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._lib.ofps_hip_contrast_mask(self._h, C.cast(C.c_void_p(g.ctypes.data), u8), W, H, stride, out.ctypes.data_as(u8)))
        return out

    def contrast_mask_dev(self, d_gray: int, W: int, H: int, stride: int, d_out_mask: int):
        self._check(self._lib.ofps_hip_contrast_mask_dev(self._h, C.c_void_p(d_gray), W, H, stride, C.c_void_p(d_out_mask)))

    def lk_flow_dev(self, d_prev: int, d_cur: int, W: int, H: int, stride: int, levels: int, radius: int, iters: int,
                    d_out_flow: int | None, d_out_entries: int | None):
        self._check(self._lib.ofps_hip_lk_flow_dev(self._h, C.c_void_p(d_prev), C.c_void_p(d_cur), W, H, stride, levels, radius,
                                                   iters, C.c_void_p(d_out_flow or 0), C.c_void_p(d_out_entries or 0)))

    # ---- A1-A4
    def densify(self, entries, w: int, h: int, want_cells=False):
        e = np.ascontiguousarray(entries, np.float32).reshape(-1, 4)
        n = e.shape[0]
        field = np.zeros((h, w, 2), np.float32)
        cells = np.zeros((max(n, 1), 2), np.uint32) if want_cells else None
        self._check(self._lib.ofps_hip_densify(self._h, _fp(e), n, w, h, _fp(field),
                                               cells.ctypes.data_as(C.POINTER(C.c_uint32)) if want_cells else None))
        return (field, cells[:n]) if want_cells else field

    def densify_weighted(self, entries, weights, w: int, h: int, want_cells=False):
        """add_vector_weighted for every entry (motion_field.rs:164-178)."""
        e = np.ascontiguousarray(entries, np.float32).reshape(-1, 4)
        wg = np.ascontiguousarray(weights, np.float32).reshape(-1)
        assert wg.shape[0] == e.shape[0]
        field = np.zeros((h, w, 2), np.float32)
        cells = np.zeros((max(e.shape[0], 1), 2), np.uint32) if want_cells else None
        self._check(self._lib.ofps_hip_densify_weighted(self._h, _fp(e), _fp(wg), e.shape[0], w, h, _fp(field),
                                                        cells.ctypes.data_as(C.POINTER(C.c_uint32)) if want_cells else None))
        return (field, cells[:e.shape[0]]) if want_cells else field

    def densify_dev(self, d_entries: int, n_per_item: int, batch: int, w: int, h: int, d_out_field: int,
                    d_out_cells: int | None = None):
        self._check(self._lib.ofps_hip_densify_dev(self._h, C.c_void_p(d_entries), n_per_item, batch, w, h,
                                                   C.c_void_p(d_out_field), C.c_void_p(d_out_cells or 0)))


    def densify_raster_dev(self, d_entries: int, d_mask: int | None, W: int, H: int, w: int, h: int, d_out_field: int,
                           verify: bool = False):
        """Densify of a per-pixel raster producer's records (cv-decoder/src/lib.rs:239-291): one launch, no sort."""
        self._check(self._lib.ofps_hip_densify_raster_dev(self._h, C.c_void_p(d_entries), C.c_void_p(d_mask or 0), W, H, w, h,
                                                          C.c_void_p(d_out_field), 1 if verify else 0))

    def densify_to_entries(self, entries, w: int, h: int) -> np.ndarray:
        e = np.ascontiguousarray(entries, np.float32).reshape(-1, 4)
        out = np.zeros((w * h, 4), np.float32)
        n_out = C.c_size_t(0)
        self._check(self._lib.ofps_hip_densify_to_entries(self._h, _fp(e), e.shape[0], w, h, _fp(out), C.byref(n_out)))
        return out[:n_out.value].copy()

    def densify_interpolated(self, entries, w: int, h: int) -> np.ndarray:
        e = np.ascontiguousarray(entries, np.float32).reshape(-1, 4)
        field = np.zeros((h, w, 2), np.float32)
        self._check(self._lib.ofps_hip_densify_interpolated(self._h, _fp(e), e.shape[0], w, h, _fp(field)))
        return field

    # ---- A5
    def block_dim(self, min_size: float, subdivide: int) -> int:
        return int(self._lib.ofps_hip_block_dim(min_size, subdivide))

    def detect(self, entries, min_size=0.05, subdivide=3, target_motion=0.003):
        e = np.ascontiguousarray(entries, np.float32).reshape(-1, 4)
        dim = self.block_dim(min_size, subdivide)
        field = np.zeros((max(dim, 1), max(dim, 1), 2), np.float32)
        has = C.c_int(0); area = C.c_size_t(0); odim = C.c_int(0)
        self._check(self._lib.ofps_hip_detect(self._h, _fp(e), e.shape[0], min_size, subdivide, target_motion,
                                              C.byref(has), C.byref(area), C.byref(odim), _fp(field)))
        return (int(area.value), field) if has.value else None

    def detect_dev(self, d_entries: int, n_per_item: int, batch: int, min_size: float, subdivide: int,
                   target_motion: float, d_out_result: int, d_out_field: int):
        self._check(self._lib.ofps_hip_detect_dev(self._h, C.c_void_p(d_entries), n_per_item, batch, min_size, subdivide,
                                                  target_motion, C.c_void_p(d_out_result), C.c_void_p(d_out_field)))

    # ---- A5i: every qualifying island (include/ofps_hip.h; csrc/detect.hip)
    @staticmethod
    def island_centroids(table: np.ndarray, dim: int) -> np.ndarray:
        """table [n, 8] -> [n, 2] centroids in frame coordinates: ((sum / area) + 0.5) / dim"""
        t = np.asarray(table, np.float64).reshape(-1, 8)
        return (t[:, 6:8] / np.maximum(t[:, 1:2], 1) + 0.5) / max(dim, 1)

    def detect_islands(self, entries, min_size=0.05, subdivide=3, target_motion=0.003, max_islands=16, want_labels=True, want_field=True) -> dict:
        """-> dict(n_islands, n_components, dim, n_listed, table int32 [n_listed, 8] = seed, area, x0, y0, x1, y1, sum_x, sum_y in rank
        order, labels uint16 [dim, dim] | None (0xFFFF = not listed), field f32 [dim, dim, 2] | None: the listed islands' cells but their seeds)"""
        e = np.ascontiguousarray(entries, np.float32).reshape(-1, 4)
        dim = max(self.block_dim(min_size, subdivide), 1)
        counts = np.zeros(4, np.int32)
        table = np.zeros((max(int(max_islands), 1), 8), np.int32)
        labels = np.zeros((dim, dim), np.uint16) if want_labels else None
        field = np.zeros((dim, dim, 2), np.float32) if want_field else None
        i32 = C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_detect_islands(self._h, _fp(e), e.shape[0], min_size, subdivide, target_motion, int(max_islands),
                                                      counts.ctypes.data_as(i32), table.ctypes.data_as(i32),
                                                      C.c_void_p(labels.ctypes.data) if want_labels else None, _fp(field) if want_field else None))
        return {"n_islands": int(counts[0]), "n_components": int(counts[1]), "dim": int(counts[2]), "n_listed": int(counts[3]),
                "table": table[:int(counts[3])].copy(), "labels": labels, "field": field}

    def detect_islands_dev(self, d_entries: int, n_per_item: int, batch: int, min_size: float, subdivide: int, target_motion: float,
                           max_islands: int, d_out_counts: int, d_out_table: int, d_out_labels: int | None = None, d_out_field: int | None = None):
        """Device form: per item counts int32[4], table int32[8 * max_islands], labels uint16[dim * dim], field f32[2 * dim * dim].  Enqueue only."""
        self._check(self._lib.ofps_hip_detect_islands_dev(self._h, C.c_void_p(d_entries), n_per_item, batch, min_size, subdivide, target_motion,
                                                          int(max_islands), C.c_void_p(d_out_counts), C.c_void_p(d_out_table),
                                                          C.c_void_p(d_out_labels or 0), C.c_void_p(d_out_field or 0)))

    def set_detect_islands(self, max_islands: int):
        """0 = off (default); K in [1, 6400]: a fused ticket that runs the detector lists up to K islands, read with frame_islands"""
        self._check(self._lib.ofps_hip_set_detect_islands(self._h, int(max_islands)))

    def get_detect_islands(self) -> int:
        return int(self._lib.ofps_hip_get_detect_islands(self._h))

    def frame_islands(self, item: int = 0, want_labels=True) -> dict:
        """The islands of `item` of the most recently collected fused ticket (pushed with max_islands > 0 and the detector on)"""
        counts = np.zeros(4, np.int32)
        if getattr(self, "_isl_buf", None) is None:                      # sized for the largest answer, made once
            self._isl_buf = (np.zeros((6400, 8), np.int32), np.zeros(160 * 160, np.uint16))
        table, labels = self._isl_buf[0], (self._isl_buf[1] if want_labels else None)
        i32 = C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_frame_islands(self._h, int(item), counts.ctypes.data_as(i32), table.ctypes.data_as(i32), table.shape[0],
                                                     C.c_void_p(labels.ctypes.data) if want_labels else None))
        dim = int(counts[2])
        return {"n_islands": int(counts[0]), "n_components": int(counts[1]), "dim": dim, "n_listed": int(counts[3]),
                "table": table[:int(counts[3])].copy(), "labels": labels[:dim * dim].reshape(dim, dim).copy() if want_labels else None}

    def _ticket_islands(self, detector) -> int:
        """whether a ticket pushed now will carry islands (1) and tracks as well (2): the context's max_islands and max_tracks at the push count"""
        if not (bool(detector) and self.get_detect_islands() > 0):
            return 0
        return 2 if self.get_detect_tracks()["max_tracks"] > 0 else 1

    # ---- A5t: island tracks (include/ofps_hip.h; csrc/detect_tracks.hip)
    @staticmethod
    def _tracks_dict(counts, rows) -> dict:
        n = int(counts[0])
        rows = np.ascontiguousarray(rows[:n], np.int32)
        sums = rows[:, 4:8].copy().view(np.int64).reshape(n, 2)
        return {"rows": n, "n_tracked": int(counts[1]), "n_live": int(counts[2]), "t": int(counts[3]), "id": rows[:, 0].copy(), "slot": rows[:, 1].copy(),
                "age": rows[:, 2].copy(), "hits": rows[:, 3].copy(), "sum_motion": sums, "table": rows.copy()}

    @staticmethod
    def track_motion(tracks: dict, areas) -> np.ndarray:
        """[n, 2] mean motion of the rows' islands: sum / area / 2^24 (areas: A5i's table column 1)"""
        a = np.maximum(np.asarray(areas, np.float64).reshape(-1, 1)[:tracks["rows"]], 1)
        return tracks["sum_motion"].astype(np.float64) / a / float(1 << 24)

    def island_tracker_bytes(self, dim: int, max_tracks: int) -> int:
        """the size of a tracker state; zeros are a fresh tracker.  0: dim or max_tracks out of range"""
        return int(self._lib.ofps_hip_island_tracker_bytes(int(dim), int(max_tracks)))

    def track_islands_dev(self, d_counts: int, d_table: int, d_labels: int, d_cells: int | None, dim: int, max_islands: int, batch: int,
                          max_tracks: int, reach: int, max_gap: int, d_state: int, d_out_track_counts: int, d_out_tracks: int):
        """Device form: `batch` items stepped in order through one state, one launch.  Per item counts int32[4], table int32[8 * max_islands],
        labels uint16[dim * dim], cells f32[2 * dim * dim] | None -> track_counts int32[4], tracks int32[8 * max_tracks].  Enqueue only."""
        self._check(self._lib.ofps_hip_track_islands_dev(self._h, C.c_void_p(d_counts), C.c_void_p(d_table), C.c_void_p(d_labels), C.c_void_p(d_cells or 0),
                                                         int(dim), int(max_islands), int(batch), int(max_tracks), int(reach), int(max_gap),
                                                         C.c_void_p(d_state or 0), C.c_void_p(d_out_track_counts), C.c_void_p(d_out_tracks)))

    def detect_tracks(self, frames, min_size=0.05, subdivide=3, target_motion=0.003, max_islands=16, max_tracks=16, reach=1, max_gap=2,
                      state: np.ndarray | None = None) -> tuple:
        """frames: [batch, n, 4] records, one frame sequence -> (list of dict(islands=..., tracks=...) per frame, state).  state: the uint8 array a
        call before returned, or None for a fresh tracker; it is updated in place and returned"""
        e = np.ascontiguousarray(frames, np.float32)
        e = e.reshape(1, -1, 4) if e.ndim == 2 else e
        batch, n = e.shape[0], e.shape[1]
        dim = max(self.block_dim(min_size, subdivide), 1)
        K, T = max(int(max_islands), 1), max(int(max_tracks), 1)
        if state is None:
            state = np.zeros(max(self.island_tracker_bytes(dim, max_tracks), 16), np.uint8)
        assert state.dtype == np.uint8 and state.flags["C_CONTIGUOUS"]
        counts, table = np.zeros((batch, 4), np.int32), np.zeros((batch, K, 8), np.int32)
        labels = np.zeros((batch, dim, dim), np.uint16)
        tcounts, rows = np.zeros((batch, 4), np.int32), np.zeros((batch, T, 8), np.int32)
        i32 = C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_detect_tracks(self._h, _fp(e), n, batch, min_size, subdivide, target_motion, int(max_islands), int(max_tracks),
                                                     int(reach), int(max_gap), C.c_void_p(state.ctypes.data), counts.ctypes.data_as(i32),
                                                     table.ctypes.data_as(i32), C.c_void_p(labels.ctypes.data), tcounts.ctypes.data_as(i32),
                                                     rows.ctypes.data_as(i32)))
        out = []
        for j in range(batch):
            c = counts[j]
            isl = {"n_islands": int(c[0]), "n_components": int(c[1]), "dim": int(c[2]), "n_listed": int(c[3]), "table": table[j, :int(c[3])].copy(),
                   "labels": labels[j].copy()}
            out.append({"islands": isl, "tracks": self._tracks_dict(tcounts[j], rows[j])})
        return out, state

    def set_detect_tracks(self, max_tracks: int, reach: int = 1, max_gap: int = 2):
        """max_tracks 0 = off (default); T in [1, 256]: a fused ticket that lists islands follows them across frames, read with frame_tracks"""
        self._check(self._lib.ofps_hip_set_detect_tracks(self._h, int(max_tracks), int(reach), int(max_gap)))

    def get_detect_tracks(self) -> dict:
        t, r, g = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._lib.ofps_hip_get_detect_tracks(self._h, C.byref(t), C.byref(r), C.byref(g)))
        return {"max_tracks": t.value, "reach": r.value, "max_gap": g.value}

    def frame_tracks(self, item: int = 0) -> dict:
        """The tracks of `item` of the most recently collected fused ticket (pushed with max_islands > 0, max_tracks > 0 and the detector on)"""
        counts = np.zeros(4, np.int32)
        if getattr(self, "_trk_buf", None) is None:
            self._trk_buf = np.zeros((256, 8), np.int32)
        i32 = C.POINTER(C.c_int32)
        self._check(self._lib.ofps_hip_frame_tracks(self._h, int(item), counts.ctypes.data_as(i32), self._trk_buf.ctypes.data_as(i32), 256))
        return self._tracks_dict(counts, self._trk_buf)

    # ---- A6-A12
    def almeida(self, entries, aspect: float, fov_y_deg: float, use_ransac=False, num_iters=200, inlier_deg=0.05,
                num_samples=1000, seed=0):
        e = np.ascontiguousarray(entries, np.float32).reshape(-1, 4)
        q = np.zeros(4, np.float32); tr = np.zeros(3, np.float32)
        self._check(self._lib.ofps_hip_almeida(self._h, _fp(e), e.shape[0], aspect, fov_y_deg, int(use_ransac),
                                               num_iters, inlier_deg, num_samples, seed, _fp(q), _fp(tr)))
        return q, tr

    def almeida_dev(self, d_entries: int, n_per_item: int, batch: int, aspect: float, fov_y_deg: float,
                    use_ransac: bool, num_iters: int, inlier_deg: float, num_samples: int, seed: int, d_out_quat: int):
        self._check(self._lib.ofps_hip_almeida_dev(self._h, C.c_void_p(d_entries), n_per_item, batch, aspect, fov_y_deg,
                                                   int(use_ransac), num_iters, inlier_deg, num_samples, seed,
                                                   C.c_void_p(d_out_quat)))

    # ---- A6c: camera compensation (include/ofps_hip.h; csrc/compensate.hip)
    def compensate(self, entries, aspect: float, fov_y_deg: float, quat) -> np.ndarray:
        """records [n, 4] and the estimator's quaternion (w, i, j, k) -> [n, 4]: pos as it is, motion - camera.delta(pos, inverse(quat))"""
        e = np.ascontiguousarray(entries, np.float32).reshape(-1, 4)
        q = np.ascontiguousarray(quat, np.float32).reshape(4)
        out = np.zeros((max(e.shape[0], 1), 4), np.float32)
        self._check(self._lib.ofps_hip_compensate(self._h, _fp(e), e.shape[0], aspect, fov_y_deg, _fp(q), _fp(out)))
        return out[:e.shape[0]]

    def compensate_dev(self, d_entries: int, n_per_item: int, batch: int, aspect: float, fov_y_deg: float, d_quat: int, d_out_entries: int):
        """Device form: one quaternion per item in device memory (what almeida_dev wrote); d_out_entries may be d_entries.  Enqueue only."""
        self._check(self._lib.ofps_hip_compensate_dev(self._h, C.c_void_p(d_entries), n_per_item, batch, aspect, fov_y_deg,
                                                      C.c_void_p(d_quat), C.c_void_p(d_out_entries)))

    def set_detect_compensation(self, mode: int):
        """0 = the fused entry points' detector reads the raw vectors (default); 1 = the vectors compensated with the frame's own quaternion
        when detector and estimator both run: "what moves relative to the camera"."""
        self._check(self._lib.ofps_hip_set_detect_compensation(self._h, mode))

    def get_detect_compensation(self) -> int:
        return int(self._lib.ofps_hip_get_detect_compensation(self._h))

    def checksum_dev(self, d_data: int, bytes_per_item: int, batch: int, d_out_u64: int):
        """Per-item wrapping u64 sum of device-resident data (ofps_hip_checksum_dev); enqueue only."""
        self._check(self._lib.ofps_hip_checksum_dev(self._h, C.c_void_p(d_data), bytes_per_item, batch, C.c_void_p(d_out_u64)))

    # ---- fused per-frame path
    def reset_frames(self):
        self._check(self._lib.ofps_hip_reset_frames(self._h))

    def stage_frame(self, luma: np.ndarray):
        """Upload a frame as the stream's newest frame without computing anything (a Decoder's skipped frames)."""
        luma = np.ascontiguousarray(luma, np.uint8)
        H, W = luma.shape
        self._check(self._lib.ofps_hip_stage_frame(self._h, luma.ctypes.data_as(C.POINTER(C.c_uint8)), W, H, W))

    def pinned_frame(self, height: int, width: int) -> np.ndarray:
        """uint8[height, width] in page-locked host memory (freed with the context): frames written into it cross
        PCIe by DMA without a staging copy."""
        p = C.c_void_p(0)
        self._check(self._lib.ofps_hip_host_alloc(self._h, height * width, C.byref(p)))
        self._pinned.append(p.value)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(height, width))

    def free_pinned(self, buf: np.ndarray):
        """Releases a buffer returned by pinned_frame / pinned_array before the context is closed."""
        p = buf.ctypes.data
        if p in self._pinned:
            self._pinned.remove(p)
            self._check(self._lib.ofps_hip_host_free(self._h, C.c_void_p(p)))

    def pinned_array(self, shape, dtype=np.float32) -> np.ndarray:
        """Page-locked host array (results of push_frame_async land in it by DMA)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p(0)
        self._check(self._lib.ofps_hip_host_alloc(self._h, max(n, 16), C.byref(p)))
        self._pinned.append(p.value)
        return np.frombuffer((C.c_uint8 * max(n, 16)).from_address(p.value), dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def _frame_params(self, block, search_range, detector, min_size, subdivide, target_motion, estimator, aspect, fov_y_deg,
                      use_ransac, num_iters, inlier_deg, num_samples, seed):
        return _lib.FrameParams(block, search_range, int(detector), min_size, subdivide, target_motion, int(estimator),
                                aspect, fov_y_deg, int(use_ransac), num_iters, inlier_deg, num_samples, seed)

    def push_frame_async(self, luma: np.ndarray, block=16, search_range=16, detector=True, min_size=0.05, subdivide=3,
                         target_motion=0.003, estimator=True, aspect=16 / 9, fov_y_deg=39.6 * 9 / 16, use_ransac=False,
                         num_iters=200, inlier_deg=0.05, num_samples=1000, seed=0, out_entries: np.ndarray | None = None,
                         out_field: np.ndarray | None = None) -> int:
        """Enqueues one frame (ofps_hip_push_frame_async) -> ticket.  `luma`, `out_entries` and `out_field` must stay alive
        and untouched until frame_wait(ticket) returns; at most two tickets in flight."""
        assert luma.dtype == np.uint8 and luma.ndim == 2 and luma.flags["C_CONTIGUOUS"]
        H, W = luma.shape
        prm = self._frame_params(block, search_range, detector, min_size, subdivide, target_motion, estimator, aspect, fov_y_deg,
                                 use_ransac, num_iters, inlier_deg, num_samples, seed)
        t = C.c_int(0)
        self._check(self._lib.ofps_hip_push_frame_async(self._h, luma.ctypes.data_as(C.POINTER(C.c_uint8)), W, H, W, C.byref(prm),
                                                        _fp(out_entries) if out_entries is not None else None,
                                                        _fp(out_field) if out_field is not None else None, C.byref(t)))
        self._pipe_isl = getattr(self, "_pipe_isl", {})
        self._pipe_isl[int(t.value)] = self._ticket_islands(detector)
        return int(t.value)

    def push_frames_async(self, frames: np.ndarray, block=16, search_range=16, detector=True, min_size=0.05, subdivide=3,
                          target_motion=0.003, estimator=True, aspect=16 / 9, fov_y_deg=39.6 * 9 / 16, use_ransac=False,
                          num_iters=200, inlier_deg=0.05, num_samples=1000, seed=0, out_entries: np.ndarray | None = None) -> int:
        """Batched form (ofps_hip_push_frames_async): frames uint8 [n, H, W] contiguous -> ticket; keep `frames` and
        `out_entries` ([n, nblk, 4] float32; with the batch decoder at KLT [n, slots, 4]: batch_record_capacity) alive until frames_wait(ticket)."""
        assert frames.dtype == np.uint8 and frames.ndim == 3 and frames.flags["C_CONTIGUOUS"]
        n, H, W = frames.shape
        if out_entries is not None and self.get_batch_decoder()["decoder"] == self.BATCH_DECODER_KLT:
            assert out_entries.size >= n * self.klt_slot_count(W, H) * 4, "out_entries: n * slots records with the batch decoder at KLT"
        prm = self._frame_params(block, search_range, detector, min_size, subdivide, target_motion, estimator, aspect, fov_y_deg,
                                 use_ransac, num_iters, inlier_deg, num_samples, seed)
        t = C.c_int(0)
        self._check(self._lib.ofps_hip_push_frames_async(self._h, frames.ctypes.data_as(C.POINTER(C.c_uint8)), n, W, H, W, W * H, C.byref(prm),
                                                         _fp(out_entries) if out_entries is not None else None, C.byref(t)))
        self._batch_n = getattr(self, "_batch_n", {})
        self._batch_n[t.value] = n
        self._batch_isl = getattr(self, "_batch_isl", {})
        self._batch_isl[t.value] = self._ticket_islands(detector)
        return t.value

    def frames_wait(self, ticket: int) -> list:
        n = self._batch_n.pop(ticket)
        res = (_lib.FrameResult * n)()
        self._check(self._lib.ofps_hip_frames_wait(self._h, ticket, res))
        out = [{"have_vectors": bool(r.have_vectors), "n_vectors": int(r.n_vectors),
                "motion": (int(r.area), int(r.dim)) if r.has_motion else None, "quat": np.array(list(r.quat), np.float32)} for r in res]
        islands = getattr(self, "_batch_isl", {}).pop(ticket, 0)
        if islands:
            for j, o in enumerate(out):
                o["islands"] = self.frame_islands(j)
                if islands == 2:
                    o["tracks"] = self.frame_tracks(j)
        return out

    def frame_wait(self, ticket: int) -> dict:
        res = _lib.FrameResult()
        self._check(self._lib.ofps_hip_frame_wait(self._h, ticket, C.byref(res)))
        out = {"have_vectors": bool(res.have_vectors), "n_vectors": int(res.n_vectors),
               "motion": (int(res.area), int(res.dim)) if res.has_motion else None, "quat": np.array(list(res.quat), np.float32)}
        islands = getattr(self, "_pipe_isl", {}).pop(ticket, 0)
        if islands:
            out["islands"] = self.frame_islands(0)
        if islands == 2:
            out["tracks"] = self.frame_tracks(0)
        return out

    def push_frame(self, luma: np.ndarray, block=16, search_range=16, detector=True, min_size=0.05, subdivide=3,
                   target_motion=0.003, estimator=True, aspect=16 / 9, fov_y_deg=39.6 * 9 / 16, use_ransac=False,
                   num_iters=200, inlier_deg=0.05, num_samples=1000, seed=0, want_entries=False, want_field=False):
        """-> dict(have_vectors, n_vectors, motion=None|(area, field|None), quat, entries|None)"""
        luma = np.ascontiguousarray(luma, np.uint8)
        H, W = luma.shape
        prm = _lib.FrameParams(block, search_range, int(detector), min_size, subdivide, target_motion, int(estimator),
                               aspect, fov_y_deg, int(use_ransac), num_iters, inlier_deg, num_samples, seed)
        res = _lib.FrameResult()
        islands = self._ticket_islands(detector)
        nb = self.sad_record_capacity(W, H, block) if want_entries else 0      # 4 * nblk with split blocks on (N1s)
        ent = np.zeros((max(nb, 1), 4), np.float32) if want_entries else None
        dim = self.block_dim(min_size, subdivide)
        fld = np.zeros((dim, dim, 2), np.float32) if want_field else None
        self._check(self._lib.ofps_hip_push_frame(self._h, luma.ctypes.data_as(C.POINTER(C.c_uint8)), W, H, W, C.byref(prm),
                                                  C.byref(res), _fp(ent) if want_entries else None,
                                                  _fp(fld) if want_field else None))
        motion = (int(res.area), fld) if res.has_motion else None
        out = {"have_vectors": bool(res.have_vectors), "n_vectors": int(res.n_vectors), "motion": motion,
               "quat": np.array(list(res.quat), np.float32),
               "entries": ent[:min(nb, int(res.n_vectors))] if (want_entries and res.have_vectors) else None}      # (the kept records with the contrast gate on)
        if islands:
            out["islands"] = self.frame_islands(0)
        if islands == 2:
            out["tracks"] = self.frame_tracks(0)
        return out


def device_count() -> int:
    return int(_lib.load().ofps_hip_device_count())


class MultiDevice:
    """In-process multi-device dispatcher (include/ofps_hip.h: ofps_hip_multi_*): one worker thread + one context per entry
    of `devices` (entries may repeat), frame pairs split into contiguous ranges, results in pair order.  The workers' contexts read their
    options from the environment when the dispatcher is made and nowhere else: with the batch decoder at KLT, OFPS_HIP_KLT_INTRA and
    OFPS_HIP_KLT_CUT (include/ofps_hip.h N3i) among them."""

    def __init__(self, devices):
        self._lib = _lib.load()
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = self._lib.ofps_hip_multi_init(devs, len(devices), C.byref(h))
        if rc != 0:
            raise OfpsHipError(rc, (self._lib.ofps_hip_multi_last_error(None) or b"").decode())
        self._h = h
        self.devices = list(devices)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ofps_hip_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise OfpsHipError(rc, (self._lib.ofps_hip_multi_last_error(self._h) or b"").decode())

    @staticmethod
    def pair_range(n_pairs: int, n_workers: int, k: int):
        f, c = C.c_size_t(0), C.c_size_t(0)
        _lib.load().ofps_hip_multi_pair_range(n_pairs, n_workers, k, C.byref(f), C.byref(c))
        return int(f.value), int(c.value)

    @staticmethod
    def frame_range(n_pairs: int, n_workers: int, k: int, ref_mode: int):
        f, c = C.c_size_t(0), C.c_size_t(0)
        _lib.load().ofps_hip_multi_frame_range(n_pairs, n_workers, k, ref_mode, C.byref(f), C.byref(c))
        return int(f.value), int(c.value)

    @staticmethod
    def stream_plan(batch: int, n_workers: int):
        """-> (worker, halo_slot, ticket_slot) of batch number `batch` of a stream (pure function, no device needed)."""
        w, h, t = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.load().ofps_hip_multi_stream_plan(batch, n_workers, C.byref(w), C.byref(h), C.byref(t))
        return int(w.value), int(h.value), int(t.value)

    @staticmethod
    def batch_record_capacity(W: int, H: int, block: int = 16) -> int:
        """records per frame of push_frames_async's out_entries.  The workers' contexts take the batch decoder from the environment at their
        init (OFPS_HIP_BATCH_DECODER, OFPS_HIP_KLT_CELL): the slot count with KLT, else the block count"""
        lib = _lib.load()
        if os.environ.get("OFPS_HIP_BATCH_DECODER") == "1":
            cell = os.environ.get("OFPS_HIP_KLT_CELL", "16")
            return int(lib.ofps_hip_klt_slot_count(W, H, int(cell) if cell in ("8", "16", "32") else 16))
        return int(lib.ofps_hip_sad_block_count(W, H, block))

    def push_frames_async(self, frames: np.ndarray, block=16, search_range=16, detector=True, min_size=0.05, subdivide=3,
                          target_motion=0.003, estimator=True, aspect=16 / 9, fov_y_deg=39.6 * 9 / 16, use_ransac=False,
                          num_iters=200, inlier_deg=0.05, num_samples=1000, seed=0, out_entries: np.ndarray | None = None) -> int:
        """One batch of consecutive frames of the stream (uint8 [n, H, W] contiguous) -> ticket; keep `frames` and `out_entries`
        ([n, nblk, 4] float32) alive until frames_wait(ticket).  Batches are dealt to the workers round-robin.  A view with
        padded rows (unit stride along x, rows `stride` >= W bytes apart, frames `stride * H` or more apart) is passed as it is."""
        assert frames.dtype == np.uint8 and frames.ndim == 3
        n, H, W = frames.shape
        pitch, stride, unit = frames.strides
        assert unit == 1 and stride >= W and (n == 1 or pitch >= stride * H), "frames: rows must be byte-contiguous"
        if out_entries is not None:
            assert out_entries.size >= n * self.batch_record_capacity(W, H, block) * 4, "out_entries: n * batch_record_capacity records"
        prm = _lib.FrameParams(block, search_range, int(detector), min_size, subdivide, target_motion, int(estimator),
                               aspect, fov_y_deg, int(use_ransac), num_iters, inlier_deg, num_samples, seed)
        t = C.c_int(0)
        self._check(self._lib.ofps_hip_multi_push_frames_async(self._h, C.cast(C.c_void_p(frames.ctypes.data), C.POINTER(C.c_uint8)), n, W, H, stride,
                                                               max(pitch, stride * H), C.byref(prm),
                                                               _fp(out_entries) if out_entries is not None else None, C.byref(t)))
        self._batch_n = getattr(self, "_batch_n", {})
        self._batch_n[t.value] = n
        return t.value

    def frames_wait(self, ticket: int) -> list:
        n = getattr(self, "_batch_n", {}).pop(ticket, 1)
        res = (_lib.FrameResult * n)()
        self._check(self._lib.ofps_hip_multi_frames_wait(self._h, ticket, res))
        return [{"have_vectors": bool(r.have_vectors), "n_vectors": int(r.n_vectors),
                 "motion": (int(r.area), int(r.dim)) if r.has_motion else None, "quat": np.array(list(r.quat), np.float32)} for r in res]

    def reset_frames(self):
        self._check(self._lib.ofps_hip_multi_reset_frames(self._h))

    def sad_flow(self, frames: np.ndarray, block: int, search_range: int, ref_mode: int = 0) -> np.ndarray:
        """frames: uint8 [n_frames, H, stride>=W is the array's row pitch] -> entries [n_frames-1, nblk, 4]."""
        frames = np.ascontiguousarray(frames, np.uint8)
        n, H, W = frames.shape
        nb = int(self._lib.ofps_hip_sad_block_count(W, H, block))
        out = np.zeros((max(n - 1, 0), nb, 4), np.float32)
        self._check(self._lib.ofps_hip_multi_sad_flow(self._h, frames.ctypes.data_as(C.POINTER(C.c_uint8)), n, W, H, W, W * H, ref_mode,
                                                      block, search_range, _fp(out)))
        return out

    def stage_frames(self, frames: np.ndarray, ref_mode: int = 0):
        frames = np.ascontiguousarray(frames, np.uint8)
        n, H, W = frames.shape
        self._geom = (n, H, W)
        self._check(self._lib.ofps_hip_multi_stage_frames(self._h, frames.ctypes.data_as(C.POINTER(C.c_uint8)), n, W, H, W, W * H, ref_mode))

    def run_resident(self, block: int, search_range: int, steps: int = 1, timed: bool = False):
        """-> None, or with timed=True the per-worker HIP-event milliseconds of the `steps` launches."""
        ms = np.zeros(len(self.devices), np.float32) if timed else None
        self._check(self._lib.ofps_hip_multi_run_resident(self._h, block, search_range, steps, _fp(ms) if timed else None))
        return ms

    def fetch(self, block: int) -> np.ndarray:
        n, H, W = self._geom
        nb = int(self._lib.ofps_hip_sad_block_count(W, H, block))
        out = np.zeros((max(n - 1, 0), nb, 4), np.float32)
        self._check(self._lib.ofps_hip_multi_fetch(self._h, block, _fp(out)))
        return out
