"""CPU: the inputs of tests/sad_gate_cases.py separate gate-on from gate-off in the oracle chain, before any GPU runs, and the restatement
of the per-block count agrees with a loop-written one.  Nothing here touches the library under test."""
import numpy as np

import oracle
import sad_gate_cases as gc


def test_block_counts_agree_with_the_loop_written_count():
    for kind, (W, H), block in (("noise", (65, 17), 8), ("half_flat", (80, 48), 16), ("impulse", (100, 60), 12)):
        f = gc.content(kind, W, H)
        a, b = gc.block_counts(f, block), gc.block_counts_loops(f, block)
        assert a.shape == (H // block, W // block) and a.dtype == np.uint32
        np.testing.assert_array_equal(a, b, err_msg=f"{kind} {W}x{H} block {block}")
    assert gc.block_counts(gc.content("constant", 64, 16), 8).sum() == 0
    assert (gc.block_counts(gc.content("noise", 128, 32), 16) == 256).all()          # noise: the dilated mask covers every block


def test_kernel_contents_exercise_both_outcomes():
    """over the kernel test's contents some blocks are kept and some dropped at every threshold it uses"""
    f = gc.content("half_flat", 128, 32)
    for block in gc.LATTICE_BLOCKS:
        c = gc.block_counts(f, block)
        for mp in (1, block * block // 2, block * block):
            keep = c >= mp
            assert keep.any() and not keep.all(), (block, mp)
    imp = gc.block_counts(gc.content("impulse", 128, 32), 16)
    assert 0 < imp.sum() < 128 * 32                       # the impulse's dilated neighbourhood straddles the corner of four tiles
    assert (imp > 0).sum() >= 2


def test_half_flat_pair_thresholds():
    prev, cur = gc.half_flat_pair()
    for block in gc.LATTICE_BLOCKS:
        nblk = (gc.PAIR_W // block) * (gc.PAIR_H // block)
        kept = [int(gc.keep_flags(cur, block, mp).sum()) for mp in (1, block * block // 2, block * block)]
        assert nblk > kept[0] >= kept[1] >= kept[2] >= 3, (block, kept)
        assert kept[0] > kept[2]                          # the block column the dilation reaches into separates the thresholds
    assert gc.keep_flags(gc.content("noise", gc.PAIR_W, gc.PAIR_H), 16, 256).all()   # "all kept"
    assert not gc.keep_flags(gc.content("constant", gc.PAIR_W, gc.PAIR_H), 16, 1).any()  # "none kept"


def test_planted_pair_separates_gate_on_from_gate_off():
    f = gc.frames()
    assert f.shape == (gc.N_FRAMES, gc.FRAME_H, gc.FRAME_W)
    cam = oracle.camera(*gc.FRAME_CAM)
    for k in range(1, gc.N_FRAMES):
        ent, best = gc.frame_vectors(k)
        keep = gc.frame_keep(k)
        kept = int(keep.sum())
        assert 3 <= kept < gc.NBLK, f"frame {k}: kept {kept}"
        dropped_moving = int(((best[~keep, 0] != 0) | (best[~keep, 1] != 0)).sum())
        assert dropped_moving >= 1, f"frame {k}: every dropped block has a zero vector"
        flat = np.arange(gc.NBLK) % (gc.FRAME_W // gc.BLOCK) >= gc.SPLIT // gc.BLOCK + 1
        assert not keep[flat].any() and ((best[flat, 0] != 0) | (best[flat, 1] != 0)).any()      # non-zero winners on the flat side
        a0 = gc.area_of(oracle.detect_motion(ent, **gc.FRAME_DETECTOR))
        a1 = gc.area_of(oracle.detect_motion(gc.gate_filter(ent, keep), **gc.FRAME_DETECTOR))
        q0 = oracle.solve_ypr_given(ent, cam)
        q1 = oracle.solve_ypr_given(gc.gate_filter(ent, keep), cam)
        print(f"frame {k}: kept {kept}/{gc.NBLK}, dropped with a non-zero vector {dropped_moving}, area {a0} -> {a1}, lsq {q0} -> {q1}")
        assert a0 != a1, f"frame {k}: the detector cannot tell the gate from its absence"
        assert np.abs(q0 - q1).max() > 1e-4, f"frame {k}: the estimator cannot tell the gate from its absence"


def test_flat_and_two_block_frames():
    assert not gc.keep_flags(gc.flat_frame(), gc.BLOCK, 1).any()
    keep = gc.keep_flags(gc.two_block_frame(), gc.BLOCK, gc.TWO_BLOCK_GATE)
    nbx = gc.FRAME_W // gc.BLOCK
    assert sorted(np.flatnonzero(keep)) == [4 * nbx + 4, 4 * nbx + 5]
