"""hip_klt (include/ofps_hip.h N3): what the definition itself does, asserted of the NumPy restatement alone, and the three
statements of the new entry points.  No GPU."""
import os
import re

import numpy as np
import pytest

import ffi_parse
import indep_klt as ik
import klt_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KLT_SYMBOLS = ["ofps_hip_set_klt", "ofps_hip_get_klt", "ofps_hip_klt_slot_count", "ofps_hip_klt_features", "ofps_hip_klt_features_dev",
               "ofps_hip_klt_track", "ofps_hip_klt_track_dev", "ofps_hip_klt_flow", "ofps_hip_klt_flow_dev"]


def _errors(W, H, shift, out):
    s = out["slots"]
    kept = s[:, 5] == ik.ST_KEPT
    tx, ty = kc.warp_truth(W, H, shift, s[kept, 0], s[kept, 1])
    err = np.hypot(s[kept, 3] / 256.0 - tx, s[kept, 4] / 256.0 - ty)
    return kept, err


@pytest.fixture(scope="module")
def big_pair():
    return kc.warp_pair(320, 192, (5.3, -4.6))


def test_pyramid_tracks_a_camera_warp(big_pair):
    prev, cur = big_pair
    out = ik.flow(prev, cur, 4, 7, 10)
    have = out["slots"][:, 5] != ik.ST_NONE
    kept, err = _errors(320, 192, (5.3, -4.6), out)
    print("features", have.sum(), "kept", kept.sum(), "within 0.25 px", (err <= 0.25).mean(), "median", np.median(err))
    assert have.sum() == 240
    assert kept.sum() >= 0.85 * have.sum()
    assert (err <= 0.25).mean() >= 0.95


def test_one_level_cannot_follow_that_motion(big_pair):
    prev, cur = big_pair
    out = ik.flow(prev, cur, 1, 7, 10)
    s = out["slots"]
    have = s[:, 5] != ik.ST_NONE
    kept, err = _errors(320, 192, (5.3, -4.6), out)
    print("kept", kept.sum(), "within 0.25 px", (err <= 0.25).sum())
    assert (err <= 0.25).sum() < 0.20 * have.sum()


def test_small_pair_every_feature_kept():
    prev, cur = kc.warp_pair(96, 64, (1.3, -0.6))
    out = ik.flow(prev, cur, 2, 4, 10)
    kept, err = _errors(96, 64, (1.3, -0.6), out)
    print("kept", kept.sum(), "worst", err.max())
    assert len(out["slots"]) == 24 and kept.all()
    assert err.max() <= 0.15


def test_region_interiors_recover_the_planted_integer_shift():
    prev, cur = kc.luma_pair()
    out = ik.flow(prev, cur, 3, 7, 10)
    shifts = kc.luma_region_shift()
    s = out["slots"]
    worst, n = 0.0, 0
    for x, y, _, dqx, dqy, st in s:
        if st != ik.ST_KEPT:
            continue
        lx, ly = x % 64, y % 64
        if min(lx, ly, 63 - lx, 63 - ly) < 14:
            continue
        sx, sy = shifts[y // 64, x // 64]
        worst = max(worst, float(np.hypot(dqx / 256.0 - sx, dqy / 256.0 - sy)))
        n += 1
    print("interior features", n, "worst", worst)
    assert n >= 12
    assert worst <= 0.2


def test_flat_frame_has_no_feature():
    prev, cur = kc.flat_pair()
    out = ik.flow(prev, cur, 2, 4, 10)
    assert (out["slots"][:, 5] == ik.ST_NONE).all() and out["count"] == 0
    assert (out["features"] == (-1, -1, 0)).all()


def test_edge_case_loses_features_through_the_frame_edge():
    prev, cur = kc.edge_pair()
    st = ik.flow(prev, cur, 3, 4, 10)["slots"][:, 5]
    assert (st == ik.ST_LEFT).sum() >= 1 and (st == ik.ST_KEPT).sum() >= 1


def test_repainted_region_is_lost_by_its_residual():
    prev, cur = kc.repaint_pair()
    st = ik.flow(prev, cur, 2, 4, 10, max_residual=160)["slots"][:, 5]
    assert (st == ik.ST_RESIDUAL).sum() >= 1 and (st == ik.ST_KEPT).sum() >= 1
    off = ik.flow(prev, cur, 2, 4, 10, max_residual=0)["slots"][:, 5]
    assert (off == ik.ST_RESIDUAL).sum() == 0


def test_partial_cells_and_the_unused_odd_column():
    prev, cur = kc.warp_pair(97, 65, (1.3, -0.6))
    assert ik.slot_grid(97, 65, 16) == (7, 5)
    out = ik.flow(prev, cur, 2, 4, 10)
    s = out["slots"]
    assert len(s) == 35
    last = s[6::7]                                           # the one-pixel-wide last column of cells: x = 96 is not admissible
    assert (last[:, 5] == ik.ST_NONE).all()
    assert ik.pyramid(prev, 2)[1].shape == (32, 48)


def test_header_ctypes_table_and_rust_block_declare_the_new_entry_points():
    hdr = ffi_parse.header_signatures()
    rs = ffi_parse.rust_signatures()
    from ofps_amd import _lib
    for name in KLT_SYMBOLS:
        assert name in hdr, name + " is not in include/ofps_hip.h"
        assert name in _lib.PROTOTYPES, name + " is not in ofps_amd/_lib.py"
        assert name in rs, name + " is not in INTEGRATION.md's Rust block"
        ret, args = hdr[name]
        res, cargs = _lib.PROTOTYPES[name]
        assert len(args) == len(cargs) == len(rs[name][1]), name
        for a, c, r in zip(args, cargs, rs[name][1]):
            assert ffi_parse.same_class(a, ffi_parse.ctypes_class(c), lp64=True), (name, a, c)
            assert ffi_parse.same_class(a, r), (name, a, r)
            if isinstance(a, tuple):
                assert a[2] in ("u8", "i32", "u32", "f32", "void", "ctx"), (name, a)
    text = open(os.path.join(ROOT, "include", "ofps_hip.h")).read()
    assert re.search(r"#define\s+OFPS_HIP_FLOW_SPARSE\s+32u", text)
    assert re.search(r"#define\s+OFPS_HIP_API_VERSION\s+2\b", text)
    from ofps_amd.runtime import HipContext
    assert HipContext.FLOW_SPARSE == 32
    assert "OFPS_HIP_FLOW_SPARSE" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
