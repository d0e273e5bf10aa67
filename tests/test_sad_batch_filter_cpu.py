"""CPU: the cases of tests/sad_batch_filter_cases.py tell the batched filtered forms (include/ofps_hip.h N1b) from their absence and from
their likely bugs -- asserted of the restatements alone -- and the three new symbols are declared where a caller looks for them."""
import os
import re

import numpy as np

import sad_batch_filter_cases as bc
import sad_consistency_cases as cc
import sad_gate_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ofps_hip_sad_flow_filtered_dev", "ofps_hip_set_sad_batch_filter", "ofps_hip_get_sad_batch_filter")


def _keep(frames, ref_mode, crit):
    return [bc.keep_of(p, c, gc.BLOCK, gc.RANGE, *crit) for p, c in bc.pairs_of(frames, ref_mode)]


def test_the_three_pairs_keep_different_counts_under_the_check():
    """a kernel that reads counts[0] (or flags of item 0) for every item is caught"""
    keep = _keep(gc.frames(), 0, (0, bc.LIMIT, 0))
    assert [int(k.sum()) for k in keep] == [cc.FRAMES_KEPT[k] for k in (1, 2, 3)] == [118, 114, 116]
    for k in (1, 2, 3):
        np.testing.assert_array_equal(keep[k - 1], cc.frame_keep(k))


def test_equal_counts_under_gate_and_check_and_what_tells_those_items_apart():
    """Under gate + check items 1 and 2 keep 110 blocks each.  They were expected to keep different sets; they keep the SAME 110 blocks
    (the texture moves by the same step in every frame, and the gate drops the noise side where the pairs differ).  So this combination
    tells item 0 from the others and nothing more; items 1 and 2 are told apart by the check alone and by every combination with the
    median test, which the GPU tests run as well -- asserted here."""
    keep = _keep(gc.frames(), 0, (bc.GATE, bc.LIMIT, 0))
    assert [int(k.sum()) for k in keep] == [cc.FRAMES_KEPT_WITH_GATE[k] for k in (1, 2, 3)] == [111, 110, 110]
    assert not np.array_equal(keep[0], keep[1])
    assert np.array_equal(keep[1], keep[2])              # the same count AND the same blocks
    for crit in ((0, bc.LIMIT, 0), (0, 0, bc.MEDIAN), (0, bc.LIMIT, bc.MEDIAN)):
        k = _keep(gc.frames(), 0, crit)
        assert not np.array_equal(k[1], k[2]), crit


def test_every_combination_of_criteria_filters_and_differs_per_item():
    f = gc.frames()
    seen = {}
    for crit in bc.CRITERIA:
        for ref_mode in (0, 1):
            keep = _keep(f, ref_mode, crit)
            counts = [int(k.sum()) for k in keep]
            assert all(0 < c < gc.NBLK for c in counts), (crit, ref_mode, counts)
            # the gate keeps the same 156 blocks of every frame, and what it keeps the other two criteria mostly pass: gate alone and all
            # three together keep one set in every item of this clip -- the scan lattice below is where every combination differs per item
            if crit not in ((bc.GATE, 0, 0), (bc.GATE, bc.LIMIT, bc.MEDIAN)):
                assert any(not np.array_equal(keep[0], k) for k in keep[1:]), (crit, ref_mode)
            seen[(crit, ref_mode)] = np.concatenate(keep)
    # no two combinations keep the same blocks: a criterion that is silently skipped is caught
    keys = list(seen)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            if a[1] == b[1]:
                assert not np.array_equal(seen[a], seen[b]), (a, b)
    # the key-frame mode pairs other frames: from the second pair on, other flags (the gate alone reads the current frame only)
    for crit in bc.CRITERIA:
        if crit[1] or crit[2]:
            assert not np.array_equal(seen[(crit, 0)], seen[(crit, 1)]), crit


def test_the_median_test_reads_the_other_criterias_flags():
    """gate + median is not gate AND median-alone: the median is taken over the gate's kept neighbours"""
    p, c = bc.pairs_of(gc.frames(), 0)[1]
    both = bc.keep_of(p, c, gc.BLOCK, gc.RANGE, bc.GATE, 0, bc.MEDIAN)
    apart = bc.keep_of(p, c, gc.BLOCK, gc.RANGE, bc.GATE, 0, 0) & bc.keep_of(p, c, gc.BLOCK, gc.RANGE, 0, 0, bc.MEDIAN)
    assert not np.array_equal(both, apart)


def test_mixed_batch_has_items_with_none_two_some_and_all_kept():
    f = bc.mixed_frames()
    keep = _keep(f, 0, (gc.TWO_BLOCK_GATE, 0, 0))
    counts = [int(k.sum()) for k in keep]
    assert counts[0] == 0 and counts[1] == bc.MIXED_KEPT_2 and 2 < counts[2] < gc.NBLK and counts[3] == gc.NBLK, counts
    assert list(np.flatnonzero(keep[1])) == [4 * 20 + 4, 4 * 20 + 5]
    # the stream's batch [textured, flat, two-block, textured]: an item with 0 and an item with 2 kept in front of a normal one
    assert np.array_equal(f[:4], np.stack([gc.frames()[0], gc.flat_frame(), gc.two_block_frame(), gc.frames()[0]]))


def test_scan_lattices_span_rounds_and_are_no_multiple_of_64():
    assert bc.SCAN_NBLK == 41 * 33 == 1353 and bc.SCAN_NBLK > 1024 and bc.SCAN_NBLK % 64
    assert bc.SCAN3_NBLK == 63 * 49 == 3087 and 3 * 1024 < bc.SCAN3_NBLK < 4 * 1024 and bc.SCAN3_NBLK % 64
    for frames in (bc.scan_frames(), bc.scan3_frames()):
        for crit in bc.CRITERIA:
            keep = [bc.keep_of(p, c, bc.SCAN_B, bc.SCAN_R, *crit) for p, c in bc.pairs_of(frames, 0)]
            n = len(keep[0])
            for k in keep:
                assert 0 < int(k.sum()) < n
                assert k[:1024].any() and not k[:1024].all() and k[1024:].any() and not k[1024:].all()      # both sides of a round's edge
            assert len({int(k.sum()) for k in keep}) == len(keep), crit                  # every item another count, under every combination


def test_big_lattice_is_past_the_one_workgroup_solver():
    assert bc.BIG_NBLK == 91 * 91 == 8281 > 8192
    f = bc.big_frames()
    keep = [bc.keep_of(p, c, bc.BIG_B, bc.BIG_R, bc.GATE, 0, bc.MEDIAN) for p, c in bc.pairs_of(f, 0)]
    counts = [int(k.sum()) for k in keep]
    assert all(3 <= c < bc.BIG_NBLK for c in counts) and len(set(counts)) > 1, counts


def test_header_and_ctypes_table_declare_the_new_symbols():
    from ofps_amd import _lib
    text = open(os.path.join(ROOT, "include", "ofps_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ofps_hip_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, name + " is not declared in include/ofps_hip.h"
        assert name in _lib.PROTOTYPES, name + " is not in ofps_amd/_lib.py's table"
    assert len(_lib.PROTOTYPES["ofps_hip_sad_flow_filtered_dev"][1]) == 16
    from ofps_amd.runtime import HipContext
    for m in ("sad_flow_filtered_dev", "set_sad_batch_filter", "get_sad_batch_filter"):
        assert callable(getattr(HipContext, m, None)), m


def test_mean_removal_with_levels_keeps_some_blocks_of_every_item():
    """the premise of the GPU suite's "prefilter4-levels2" mode, from the restatements alone: winners of the search over 2 levels on the
    mean-removed frames (radius 4), forward and backward, through the criteria on the RAW frames (the gate reads the unfiltered current
    frame) -- every item keeps some blocks and drops some, in both ref_modes, under all three criteria and under the median test alone"""
    import indep_sad_hier as ih
    import indep_sad_prefilter as ip
    f = gc.frames()
    filtered = [ip.prefilter(x, 4) for x in f]
    for ref_mode in (0, 1):
        counts = {(bc.GATE, bc.LIMIT, bc.MEDIAN): [], (0, 0, bc.MEDIAN): []}
        for k in range(len(f) - 1):
            a, b = (0 if ref_mode else k), k + 1
            F = ih.search(filtered[a], filtered[b], gc.BLOCK, gc.RANGE, 2, top=ip.full_search)[1]
            G = ih.search(filtered[b], filtered[a], gc.BLOCK, gc.RANGE, 2, top=ip.full_search)[1]
            for crit, got in counts.items():
                got.append(int(bc.keep_of(f[a], f[b], gc.BLOCK, gc.RANGE, *crit, F=F, G=G).sum()))
        print(f"ref_mode {ref_mode}: {counts}")
        for crit, got in counts.items():
            assert gc.NBLK == 240 and all(0 < n < gc.NBLK for n in got), (ref_mode, crit, got)
