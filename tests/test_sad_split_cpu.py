"""CPU: hip_sad's split blocks (include/ofps_hip.h N1s).  What the definition promises, held against the restatement
tests/indep_sad_split.py alone on the cases of tests/sad_split_cases.py, and the three statements of the new entry points (header, ctypes
table, the Rust block of INTEGRATION.md)."""
import numpy as np
import pytest

import ffi_parse
import indep_sad_split as isp
import sad_split_cases as sc

NEW_ENTRY_POINTS = ("ofps_hip_set_sad_split", "ofps_hip_get_sad_split", "ofps_hip_sad_record_capacity", "ofps_hip_sad_split",
                    "ofps_hip_sad_split_dev", "ofps_hip_sad_flow_split_dev")


@pytest.mark.parametrize("with_keep", (False, True))
@pytest.mark.parametrize("T", sc.THRESHOLDS)
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_gain_is_never_negative_and_the_count_follows_the_flags(name, T, with_keep):
    e = sc.expect(name, T, with_keep)
    best = sc.parents(name)
    keep = sc.keep_pattern(len(best)) != 0 if with_keep else np.ones(len(best), bool)
    sums = e["sub_best"][:, :, 2].astype(np.int64).sum(axis=1)
    assert (sums[keep] <= best[keep, 2]).all()                       # the parent's winner is a candidate of each of its sub-blocks
    assert not e["split"][~keep].any() and not e["slot_flags"][~keep].any() and not e["sub_best"][~keep].any()
    assert len(isp.records(e)) == int(keep.sum()) + 3 * int(e["split"].sum())
    gain = best[:, 2].astype(np.int64) - sums
    W, H, B, _ = sc.geometry(name)
    np.testing.assert_array_equal(e["split"] != 0, keep & (16 * gain >= T * B * B))
    # the sub-blocks' winners do not depend on the threshold
    np.testing.assert_array_equal(e["sub_best"], sc.expect(name, sc.THRESHOLDS[0], with_keep)["sub_best"])


def test_noise_only_pair_never_splits_at_the_largest_threshold():
    import indep_sad_prefilter as ipf
    e = sc.expect("noise_only", 4080)
    assert not e["split"].any()
    W, H, B, _ = sc.geometry("noise_only")
    plain = ipf.entries(sc.parents("noise_only"), B, W, H)
    np.testing.assert_array_equal(isp.records(e).view(np.uint32), np.ascontiguousarray(plain, np.float32).view(np.uint32))


@pytest.mark.parametrize("T", sc.THRESHOLDS)
def test_flat_frame_never_splits(T):
    e = sc.expect("flat", T)
    assert not e["split"].any() and not e["sub_best"].any()          # every sub-block: d = 0 with SAD 0
    assert (sc.parents("flat") == 0).all()


def test_boundary_scene_recovers_both_vectors():
    name, boundary = "boundary24", 24
    e = sc.expect(name, 1)
    W, H, B, _ = sc.geometry(name)
    under, want = sc.true_vectors(name, boundary)
    assert under.sum() >= 40                                          # 48 sub-blocks, the right region's bottom row has no valid true vector
    np.testing.assert_array_equal(e["sub_best"][:, :, :2][under], want[under])
    assert (e["sub_best"][:, :, 2][under] == 0).all()
    nbx = W // B
    straddling = np.array([(k % nbx) * B < boundary < (k % nbx) * B + B for k in range(len(e["split"]))])
    assert straddling.sum() == H // B
    assert (16 * sc.parents(name)[straddling, 2].astype(np.int64) >= B * B).all()      # the precondition: the parents do not fit
    assert e["split"][straddling].all()


def test_every_path_of_the_kernel_has_a_case():
    """distinct predictors: one (flat) up to several; a sub-block whose clamp differs from its sibling's (the corner scenes)"""
    assert (sc.expect("flat", 1)["n_pred"] == 1).all()
    assert sc.expect("boundary24", 1)["n_pred"].max() >= 3
    for name in ("corner_minus", "corner_plus"):
        prev, cur = sc.pair(name)
        W, H, B, R = sc.geometry(name)
        best = sc.parents(name)
        nbx, nby, b = W // B, H // B, B // 2
        differs = 0
        for k in range(nbx * nby):
            lists = [isp.predictors(best, nbx, nby, k % nbx, k // nbx, (k % nbx) * B + (s & 1) * b, (k // nbx) * B + (s >> 1) * b, b, W, H)
                     for s in range(4)]
            differs += any(l != lists[0] for l in lists[1:])
        assert differs >= 2, name
        assert (np.abs(best[:, :2]) == 8).all(axis=1).any(), name       # winners of +-8


def test_wild_parents_stay_inside_the_frame():
    prev, cur = sc.pair("boundary24")
    W, H, B, R = sc.geometry("boundary24")
    best = sc.wild_parents((W // B) * (H // B))
    e = isp.split_step(prev, cur, B, best, None, R, 16)
    b = B // 2
    for k in range(len(best)):
        for s in range(4):
            sx0, sy0 = (k % (W // B)) * B + (s & 1) * b, (k // (W // B)) * B + (s >> 1) * b
            dx, dy = e["sub_best"][k, s, :2]
            assert 0 <= sx0 + dx <= W - b and 0 <= sy0 + dy <= H - b


def test_validity_of_parameters():
    assert isp.is_valid(16, 16, 1) and isp.is_valid(8, 124, 4080) and isp.is_valid(64, 0, 1)
    assert not isp.is_valid(15, 16, 1) and not isp.is_valid(6, 16, 1) and not isp.is_valid(16, 125, 1)
    assert not isp.is_valid(16, 16, 0) and not isp.is_valid(16, 16, 4081)


def test_header_ctypes_and_rust_declare_the_entry_points():
    from ofps_amd import _lib
    hdr, rs = ffi_parse.header_signatures(), ffi_parse.rust_signatures()
    for name in NEW_ENTRY_POINTS:
        assert name in hdr, f"{name} is not declared in include/ofps_hip.h"
        assert name in rs, f"{name} is not declared in INTEGRATION.md's extern block"
        assert name in _lib.PROTOTYPES, f"{name} has no ctypes row"
        ret, args = hdr[name]
        rret, rargs = rs[name]
        assert ffi_parse.same_class(ret, rret) and len(args) == len(rargs) and all(ffi_parse.same_class(a, r) for a, r in zip(args, rargs)), name
        cres, cargs = _lib.PROTOTYPES[name]
        assert ffi_parse.same_class(ret, ffi_parse.ctypes_class(cres), lp64=True) and len(args) == len(cargs), name
        assert all(ffi_parse.same_class(a, ffi_parse.ctypes_class(c), ignore_const=True, lp64=True) for a, c in zip(args, cargs)), name
