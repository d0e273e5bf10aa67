"""CPU: the island list's plain-Python restatement (tests/indep_detect_islands.py) against scipy's labelling and against the detector's
oracle, the literals of tests/detect_islands_cases.py, and the three statements of the C ABI (include/ofps_hip.h A5i)."""
import numpy as np
import pytest
from scipy import ndimage

import detect_cases as dc
import detect_islands_cases as ic
import indep_detect_islands as indep
import oracle

F = np.float32
ENTRY_POINTS = ("ofps_hip_detect_islands", "ofps_hip_detect_islands_dev", "ofps_hip_set_detect_islands", "ofps_hip_get_detect_islands",
                "ofps_hip_frame_islands")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_the_two_families_keep_the_side():
    for d in ic.SIDES:
        if d >= 4:
            m, s = ic.pair_area2(d)
            assert oracle.block_dim(m, s) == d
            assert F(2) / F(d * d) >= F(m) and not (F(1) / F(d * d) >= F(m)), d
    for d in ic.EQUAL_SIDES:
        m, s = ic.pair_area1(d)
        assert oracle.block_dim(m, s) == d
        assert F(1) / F(d * d) >= F(m), d
    assert oracle.block_dim(float(F(1.0 / 14 ** 2)), 1) == 15             # why side 14 is not in the equality family
    for c in ic.ALL_CASES:
        assert oracle.block_dim(c.params["min_size"], c.params["subdivide"]) == c.side, c.name
    assert {c.side for c in ic.CASES} == set(ic.SIDES)


@pytest.mark.parametrize("case", ic.ALL_CASES + dc.ALL_CASES, ids=lambda c: c.name)
def test_components_equal_scipy_label(case):
    ref = ic.reference(case.make(), case.params)
    lit = indep.lit_map(ref.field, case.params["target_motion"])
    lab, n = ndimage.label(lit, structure=np.ones((3, 3), int))
    assert n == ref.n_components, case.name
    assert ((lab > 0) == (ref.root >= 0)).all()
    # the same partition: every scipy label maps to one root and back
    pairs = set(zip(lab[lit].tolist(), ref.root[lit].tolist()))
    assert len(pairs) == n and len({p[0] for p in pairs}) == n and len({p[1] for p in pairs}) == n, case.name
    # a root is its component's smallest cell index, and the table says what numpy says of the cells
    d = ref.dim
    idx = np.arange(d * d).reshape(d, d)
    for row in ref.table[:64]:
        m = ref.root == row[0]
        ys, xs = np.nonzero(m)
        assert idx[m].min() == row[0] and m.sum() == row[1], case.name
        assert row[2:].tolist() == [xs.min(), ys.min(), xs.max(), ys.max(), xs.sum(), ys.sum()], case.name
    areas = ref.table[:, 1].astype(np.int64)
    assert (np.diff(areas) <= 0).all()
    same = np.diff(areas) == 0
    assert (np.diff(ref.table[:, 0])[same] > 0).all(), "ties are ordered by seed"


@pytest.mark.parametrize("case", ic.ALL_CASES + dc.ALL_CASES, ids=lambda c: c.name)
def test_island_0_and_the_k1_field_equal_the_detector(case):
    e = case.make()
    ref = ic.reference(e, case.params)
    counts, table, labels, field = indep.listed(ref, 1)
    has_o, area_o, field_o = dc.expected(e, case.params)                  # oracle.detect_motion
    assert has_o == (ref.n_islands >= 1), case.name
    if has_o:
        assert table[0, 1] == area_o, case.name
    np.testing.assert_array_equal(_bits(field), _bits(field_o), err_msg=case.name)
    assert counts.tolist() == [ref.n_islands, ref.n_components, case.side, min(ref.n_islands, 1)]
    assert ((labels == 0) | (labels == indep.NOT_LISTED)).all()


@pytest.mark.parametrize("case", [c for c in ic.ALL_CASES if c.n_islands is not None], ids=lambda c: c.name)
def test_literals(case):
    ref = ic.reference(case.make(), case.params)
    assert (ref.n_islands, ref.n_components) == (case.n_islands, case.n_components), case.name


def test_the_named_properties():
    ref = ic.reference(ic.BY_NAME["lattice-160-a1"].make(), ic.BY_NAME["lattice-160-a1"].params)
    assert ref.n_islands == 6400 and (ref.table[:, 1] == 1).all() and (np.diff(ref.table[:, 0]) > 0).all()
    ref = ic.reference(ic.BY_NAME["dominoes-160-a2"].make(), ic.BY_NAME["dominoes-160-a2"].params)
    assert ref.n_components == 4320 and ref.n_islands == 4240 and (ref.table[:, 1] == 2).all()
    ref = ic.reference(ic.BY_NAME["dominoes-160-a1"].make(), ic.BY_NAME["dominoes-160-a1"].params)
    assert ref.n_islands == 4320 and (ref.table[:4240, 1] == 2).all() and (ref.table[4240:, 1] == 1).all()      # mixed, each tier tied
    ref = ic.reference(ic.BY_NAME["all_on-160-a2"].make(), ic.BY_NAME["all_on-160-a2"].params)
    assert ref.table.tolist() == [[0, 25600, 0, 0, 159, 159, 25600 * 159 // 2, 25600 * 159 // 2]]
    ref = ic.reference(ic.BY_NAME["spirals_extra-33-a2"].make(), ic.BY_NAME["spirals_extra-33-a2"].params)
    assert ref.table[0, 1] == ref.table[1, 1] + 1 and ref.table[0, 0] > ref.table[1, 0]      # the later spiral wins by a cell
    ref = ic.reference(ic.BY_NAME["spirals-33-a2"].make(), ic.BY_NAME["spirals-33-a2"].params)
    assert ref.table[0, 1] == ref.table[1, 1] and ref.table[0, 0] == 0                       # equal areas: the earlier seed
    for c in ic.CASES:
        if c.name.startswith("k1024") and c.side >= 64:                                      # (side 33 holds one block)
            r = ic.reference(c.make(), c.params)
            assert r.n_islands >= 2 and len(set(r.table[:, 1].tolist())) >= 2, c.name        # mixed areas
    # truncation: K below n_islands leaves cells of the islands behind K unlisted
    ref = ic.reference(ic.BY_NAME["dominoes-17-a2"].make(), ic.BY_NAME["dominoes-17-a2"].params)
    counts, table, labels, field = indep.listed(ref, 2)
    assert counts.tolist() == [ref.n_islands, ref.n_components, 17, 2] and len(table) == 2
    assert (labels == 0).sum() == 2 and (labels == 1).sum() == 2 and (labels == indep.NOT_LISTED).sum() == 17 * 17 - 4
    assert ic.k_values(5) == [1, 2, 4, 5, 6, 6400] and ic.k_values(0) == [1, 2, 6400] and ic.k_values(6400) == [1, 2, 6399, 6400]


def test_fused_frames_move_what_they_say():
    f = ic.frames()
    assert f.shape == (5, ic.FH, ic.FW) and oracle.block_dim(ic.FUSED["min_size"], ic.FUSED["subdivide"]) == 15
    assert (f[0, :8] == f[4, :8]).all() and (f[0, 16:40, 8:40] == f[2, 16:40, 12:44]).all() and (f[0, 56:80, 96:120] == f[2, 56:80, 90:114]).all()
    det = {k: ic.FUSED[k] for k in ("min_size", "subdivide", "target_motion")}
    for k in (1, 2, 3):                                                   # both rectangles are islands of the oracle's vectors
        r = oracle.sad_flow(f[k - 1], f[k], ic.BLOCK, ic.RANGE)
        isl = indep.islands(np.asarray(r[0] if isinstance(r, tuple) else r, F), **det)
        assert isl.n_islands == 2 and isl.n_components == 2, k


# ---- the ABI: header, ctypes table and the Rust block declare the five entry points ------------------------------------------------------
def test_the_five_entry_points_are_declared_three_times():
    import ffi_parse as fp
    from ofps_amd import _lib
    hdr, rs = fp.header_signatures(), fp.rust_signatures()
    for name in ENTRY_POINTS:
        assert name in hdr, f"{name}: not in include/ofps_hip.h"
        assert name in _lib.PROTOTYPES, f"{name}: not in ofps_amd/_lib.py"
        assert name in rs, f"{name}: not in INTEGRATION.md's extern block"
        assert len(hdr[name][1]) == len(_lib.PROTOTYPES[name][1]) == len(rs[name][1]), name
    assert len(hdr["ofps_hip_detect_islands"][1]) == 11 and len(hdr["ofps_hip_detect_islands_dev"][1]) == 12
    assert len(hdr["ofps_hip_frame_islands"][1]) == 6 and len(hdr["ofps_hip_set_detect_islands"][1]) == 2
    text = open(fp.os.path.join(fp.ROOT, "include", "ofps_hip.h")).read()
    assert "A5i" in text and "build-defined" in text[text.index("A5i"):text.index("A5i") + 600].lower()
    assert _lib.load().ofps_hip_api_version() == 2
