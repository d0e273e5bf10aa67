"""The cases of tests/dense_output_cases.py have the properties they are named for -- on the CPU, on the oracle mask alone.  This is what
keeps tests/test_dense_output_stage_gpu.py from passing vacuously: a "nothing survives" frame that kept a pixel, or a "two scan rounds"
frame with one tile, would make the GPU comparison say nothing about the path it is there for."""
import numpy as np
import pytest

import dense_output_cases as dc
import oracle
from oracle import np_oracle

# survivors of the oracle mask per case (W, H, shape); (a) is 0 and (b) is W * H by assertion below
SURVIVORS = {
    (217, 151, "c"): 20148, (217, 151, "g"): 6622, (256, 128, "c"): 18454, (256, 128, "g"): 5619,
    (99, 331, "c"): 22706, (99, 331, "d"): 84, (99, 331, "e"): 84, (99, 331, "f"): 993, (99, 331, "g"): 14530,
    (256, 132, "c"): 19052, (256, 132, "g"): 5795, (333, 101, "c"): 20146, (333, 101, "g"): 4432,
    (1024, 1024, "c"): 526596, (1024, 1024, "d"): 84, (1024, 1024, "e"): 84, (1024, 1024, "f"): 3178, (1024, 1024, "g"): 44977,
    (1024, 1025, "c"): 526699, (1024, 1025, "d"): 84, (1024, 1025, "e"): 84, (1024, 1025, "f"): 3178, (1024, 1025, "g"): 45021,
    (1920, 1080, "c"): 1044430, (1920, 1080, "d"): 84, (1920, 1080, "e"): 84, (1920, 1080, "f"): 3333, (1920, 1080, "g"): 47420,
    (2048, 1025, "c"): 1071109, (2048, 1025, "d"): 84, (2048, 1025, "e"): 84, (2048, 1025, "f"): 3178, (2048, 1025, "g"): 44974,
}


def test_literal_footprint_spot_values():
    """one interior impulse on 40 x 40: 4 * 5 = 20 passes nothing; 6 passes the two weight-4 taps; 21 passes all eight"""
    for a, want in ((5, 0), (6, 119), (10, 119), (11, 155), (20, 155), (21, 163)):
        for s in (a, -a):
            assert int(dc.impulse_mask(40, 40, [(20, 20, s)]).sum()) == want, s
    assert [len(dc.impulse_taps(a)) for a in dc.AMPLITUDES] == [0, 2, 2, 6, 6, 8]
    # the two signs answer in different quadrants
    assert not np.array_equal(dc.impulse_mask(40, 40, [(20, 20, 6)]), dc.impulse_mask(40, 40, [(20, 20, -6)]))


@pytest.mark.parametrize("a", dc.SIGNED_AMPLITUDES)
def test_literal_footprints_equal_both_oracles(a):
    """interior impulses around the mask tile seams, and at the closest distance to a border the literal builder accepts"""
    W, H = dc.SEAM_W, dc.SEAM_H
    m = dc.REFLECT_MARGIN
    places = list(zip(dc.SEAM_YS, dc.SEAM_XS)) + [(dc.SEAM_YS[k], dc.SEAM_XS[-1 - k]) for k in range(0, 28, 3)]
    places += [(m, m), (m, W - 1 - m), (H - 1 - m, m), (H - 1 - m, W - 1 - m), (m, 100), (30, m)]
    for y, x in places:
        g = dc.impulse_frame(W, H, [(y, x, a)])
        want = dc.impulse_mask(W, H, [(y, x, a)])
        np.testing.assert_array_equal(oracle.contrast_mask(g), want, err_msg=f"impulse {a} at {(y, x)}")
        np.testing.assert_array_equal(np_oracle.contrast_mask(g), want, err_msg=f"impulse {a} at {(y, x)}")


def test_sparse_impulses_footprint():
    for W, H in ((99, 331), (1024, 1024)):
        imp = dc.sparse_impulses(W, H)
        assert len(imp) >= 6 and all(b[0] - a[0] >= 40 for a, b in zip(imp, imp[1:]))
        np.testing.assert_array_equal(oracle.contrast_mask(dc.impulse_frame(W, H, imp)), dc.impulse_mask(W, H, imp))


@pytest.mark.parametrize("a", (6, -11, 21))
def test_border_impulses_both_oracles_agree(a):
    """near a border BORDER_REFLECT_101 folds the impulse back into the window: no literal footprint, the two restatements check each other;
    and the folding matters (some placement's mask differs from the interior footprint moved there)"""
    W, H = dc.BORDER_W, dc.BORDER_H
    places = dc.border_placements()
    assert len(places) == 4 * 49 + 28
    sums = set()
    for y, x in places:
        g = dc.impulse_frame(W, H, [(y, x, a)])
        m = oracle.contrast_mask(g)
        np.testing.assert_array_equal(m, np_oracle.contrast_mask(g), err_msg=f"impulse {a} at {(y, x)}")
        sums.add(int(m.sum()))
    assert len(sums) > 4


def test_mask_geometry_list_keeps_every_width_and_height():
    assert {W for W, _ in dc.MASK_GEOMETRIES} == set(dc.MASK_WS) and {H for _, H in dc.MASK_GEOMETRIES} == set(dc.MASK_HS)
    assert 140 <= len(dc.MASK_GEOMETRIES) <= 170
    assert dc.mask_content("checker", 9, 7).max() == 255 and not oracle.contrast_mask(dc.mask_content("constant", 9, 7)).any()
    assert oracle.contrast_mask(dc.mask_content("checker", 64, 16)).all()


def test_compaction_geometries_are_what_the_table_says():
    n = [W * H for W, H in dc.COMPACT_GEOMETRIES]
    assert n == [32767, 32768, 32769, 33792, 33633, 1048576, 1049600, 2073600, 2099200]
    assert n[0] % 4 != 0 and n[0] <= dc.SMALL_MAX == n[1] < n[2] and n[2] % 4 == 1
    tiles = [-(-k // dc.CT) for k in n]
    assert tiles[3:] == [33, 33, 1024, 1025, 2025, 2050] and n[3] % dc.CT == 0 and n[4] % dc.CT != 0
    assert [-(-t // 1024) for t in tiles[5:]] == [1, 2, 2, 3]            # rounds of the scan's carry loop
    assert len(dc.COMPACT_CASES) == 4 * 9 + 3 * 5


@pytest.mark.parametrize("W,H,shape", dc.COMPACT_CASES)
def test_compaction_case_has_its_shape(W, H, shape):
    m = dc.oracle_mask(W, H, shape)
    n, k = W * H, int(m.sum())
    idx = np.flatnonzero(m.reshape(-1))
    tc = dc.tile_counts(m)
    assert len(tc) == -(-n // dc.CT) and int(tc.sum()) == k
    print(f"survivors {W}x{H} ({shape}): {k} of {n}")
    if shape == "a":
        assert k == 0
        return
    if shape == "b":
        assert k == n
        return
    assert 0 < k < n
    assert SURVIVORS[(W, H, shape)] == k
    if shape == "c":
        assert 0.25 < k / n < 0.75
    elif shape == "d":
        # the first rows' first columns: the head of tile 0 (and of the tiles the next nine rows start in), nothing else
        assert idx.max() < dc.CORNER_BOX * W and (idx % W).max() < dc.CORNER_BOX and tc[0] > 0
        assert not tc[-(-dc.CORNER_BOX * W // dc.CT):].any()
        if W <= 102:
            assert idx.max() < dc.CT and not tc[1:].any()                 # all of it among the first 1,024 records
    elif shape == "e":
        assert idx.min() >= n - dc.CORNER_BOX * W and (idx % W).min() >= W - dc.CORNER_BOX and tc[-1] > 0
        assert not tc[:(n - dc.CORNER_BOX * W) // dc.CT].any()
        assert idx.max() >= n - 1 - 4 * W                                  # reaches the ragged / last tile's end rows
    elif shape == "f":
        some = np.flatnonzero(tc)
        gaps = np.diff(some)
        assert (gaps > 1).sum() >= 4                                       # empty tiles between tiles with survivors, several times
        assert tc[0] == 0 or W * 10 > dc.CT                                # (the first impulse sits at row 20)
    elif shape == "g":
        rows = m.reshape(H, W)
        assert rows.any(axis=1).all()                                      # survivors in every row ...
        assert 30 <= rows.sum(axis=1).min() and rows.sum(axis=1).max() <= 44   # ... only around the band
        if W % 64:                                                         # (a width of whole waves keeps the band in the same lanes)
            first = [int(np.flatnonzero(r)[0] + y * W) % 64 for y, r in enumerate(rows[:40])]
            assert len(set(first)) > 4                                     # lane positions differ from row to row


def test_reduced_cases_straddle_the_single_workgroup_limit():
    px = {}
    for W, H, cap in dc.REDUCED_CASES:
        gw, gh = oracle.cv_grid(W, H, cap, cap)
        px[(W, H, cap)] = gw * gh
    assert px == dc.REDUCED_PIXELS
    assert px[(960, 540, 241)] == 32535 <= dc.SMALL_MAX < 32912 == px[(960, 540, 242)] and px[(400, 400, 200)] == 40000


def test_stream_frames_give_very_different_counts():
    """consecutive tickets of the stream tests: everything, nothing, a few hundred, about half"""
    for W, H in ((480, 270), (1920, 1080), (256, 128)):
        n = W * H
        k = {kind: int(oracle.contrast_mask(dc.stream_frame(W, H, kind)).sum()) for kind in dc.STREAM_KINDS}
        print(f"stream frames {W}x{H}: {k}")
        assert k["flat"] == 0 and k["noise"] == n and k["impulse"] == 163 + 155 and 0.25 * n < k["texture"] < 0.75 * n
    assert dc.stream_kinds(8) == ["noise", "flat", "impulse", "texture"] * 2
