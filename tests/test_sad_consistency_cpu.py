"""CPU: the inputs of tests/sad_consistency_cases.py separate check-on from check-off in the oracle chain, before any GPU runs, and the
array-indexed restatement of the residual agrees with a loop-written one.  Nothing here touches the library under test."""
import numpy as np

import oracle
import sad_consistency_cases as cc
import sad_gate_cases as gc


def test_array_form_and_loop_form_agree():
    for name, block, rng in (("half_flat", 8, gc.PAIR_RANGE), ("half_flat", 16, gc.PAIR_RANGE), ("frames1", gc.BLOCK, gc.RANGE),
                             ("generic", cc.GENERIC_BLOCK, cc.GENERIC_RANGE), ("pruned", cc.PRUNED_BLOCK, cc.PRUNED_RANGE)):
        prev, cur, ent, F, G = cc.pair_vectors(name, block, rng)
        H, W = cur.shape
        r = cc.residual(F, G, W, H, block)
        assert r.dtype == np.uint32 and r.shape == ((W // block) * (H // block),) and r.max() <= 2 * rng, name
        np.testing.assert_array_equal(r, cc.residual_loops(F, G, W, H, block), err_msg=f"{name} block {block}")
    for B in cc.KERNEL_BLOCKS:
        for nbx, nby in cc.KERNEL_LATTICES:
            W, H, F, G = cc.synthetic_winners(nbx, nby, B)
            np.testing.assert_array_equal(cc.residual(F, G, W, H, B), cc.residual_loops(F, G, W, H, B), err_msg=f"synthetic {nbx}x{nby} block {B}")


def test_synthetic_winners_reach_the_edges_and_the_thresholds():
    """what the kernel test relies on: vectors at every frame edge, residuals of limit - 1 and limit for limits 1 and 2, the largest
    residual of the domain (128 = limit 129's limit - 1; 129 itself needs |d| > 64, outside the standalone form's domain), and blocks
    that share a partner"""
    for B in cc.KERNEL_BLOCKS:
        W, H, F, G = cc.synthetic_winners(20, 12, B)
        assert np.abs(F[:, :2]).max() <= 64 and np.abs(G[:, :2]).max() <= 64
        k = np.arange(240)
        x0, y0 = (k % 20) * B, (k // 20) * B
        assert (x0 + F[:, 0] >= 0).all() and (x0 + F[:, 0] + B <= W).all() and (y0 + F[:, 1] >= 0).all() and (y0 + F[:, 1] + B <= H).all()
        for edge in (x0 + F[:, 0] == 0, x0 + F[:, 0] + B == W, y0 + F[:, 1] == 0, y0 + F[:, 1] + B == H):
            assert (edge & ((F[:, 0] != 0) | (F[:, 1] != 0))).sum() >= 3
        r = cc.residual(F, G, W, H, B)
        for v in (0, 1, 2, 128):
            assert (r == v).any(), (B, v)
        assert len(np.unique(cc.partner(F, W, H, B))) < 240
    W, H, B, F, G, want = cc.ragged_winners()
    nbx, nby = W // B, H // B
    assert (((np.arange(2) % nbx) * B + B // 2 + F[:, 0]) // B).tolist() == [nbx, nbx]            # only the clamp keeps these inside the lattice
    assert ((B // 2 + F[:, 1]) // B).tolist() == [nby, nby]
    np.testing.assert_array_equal(cc.residual(F, G, W, H, B), want)
    np.testing.assert_array_equal(cc.residual_loops(F, G, W, H, B), want)


def test_half_flat_pair_counts_are_the_pinned_literals():
    for block in gc.LATTICE_BLOCKS:
        prev, cur, ent, F, G = cc.pair_vectors("half_flat", block)
        keep = cc.keep_flags(F, G, gc.PAIR_W, gc.PAIR_H, block, cc.LIMIT)
        gate = gc.keep_flags(cur, block, 1)
        assert int(keep.sum()) == cc.HALF_FLAT_KEPT[block]
        assert int((keep & gate).sum()) == cc.HALF_FLAT_KEPT_WITH_GATE[block] < min(int(keep.sum()), int(gate.sum()))
        assert cc.keep_flags(F, G, gc.PAIR_W, gc.PAIR_H, block, 2 * gc.PAIR_RANGE + 1).all()
    for name, block, rng in (("generic", cc.GENERIC_BLOCK, cc.GENERIC_RANGE), ("pruned", cc.PRUNED_BLOCK, cc.PRUNED_RANGE)):
        prev, cur, ent, F, G = cc.pair_vectors(name, block, rng)
        keep = cc.keep_flags(F, G, cur.shape[1], cur.shape[0], block, cc.LIMIT)
        assert 3 <= keep.sum() < len(keep), name                                         # both outcomes occur


def test_planted_stream_separates_check_on_from_check_off():
    """The conditions the issue sets on frames() at limit 1, the pinned counts, and the margins the GPU test needs.
    Margins: the fused path's quaternion is held to 2e-6 (LSQ) of ofps_hip_almeida on the same records, so a checked-against-unchecked
    difference above 1e-4 -- 50 bounds -- cannot be mistaken; the oracle's own differences are 7e-4 and more.  The detector's area is an
    integer compared bit for bit: any difference shows; the oracle's are 36 cells and more, 10 is asked for."""
    cam = oracle.camera(*gc.FRAME_CAM)
    tex = np.arange(gc.NBLK) % (gc.FRAME_W // gc.BLOCK) < cc.TEXTURE_COLUMNS
    assert tex.sum() == 144
    for k in range(1, gc.N_FRAMES):
        ent, F = gc.frame_vectors(k)
        keep = cc.frame_keep(k)
        moving = (F[:, 0] != 0) | (F[:, 1] != 0)
        n_noise, n_tex, n_dropped_moving = int(keep[~tex].sum()), int(keep[tex].sum()), int((moving & ~keep).sum())
        assert int(keep.sum()) == cc.FRAMES_KEPT[k]
        assert n_noise <= 12 and n_tex >= 100 and n_dropped_moving >= 80, (k, n_noise, n_tex, n_dropped_moving)
        assert cc.frame_keep(k, cc.KEEP_ALL).all() and cc.KEEP_ALL == 17
        gate = gc.frame_keep(k)
        both = cc.frame_keep(k, cc.LIMIT, gc.GATE)
        assert int(both.sum()) == cc.FRAMES_KEPT_WITH_GATE[k] < min(int(keep.sum()), int(gate.sum()))
        assert (keep & ~gate).any() and (gate & ~keep).any()                             # neither criterion contains the other
        a0 = gc.area_of(oracle.detect_motion(ent, **gc.FRAME_DETECTOR))
        q0 = oracle.solve_ypr_given(ent, cam)
        for what, kp in (("check", keep), ("check + gate", both)):
            a1 = gc.area_of(oracle.detect_motion(cc.check_filter(ent, kp), **gc.FRAME_DETECTOR))
            q1 = oracle.solve_ypr_given(cc.check_filter(ent, kp), cam)
            print(f"frame {k} {what}: kept {int(kp.sum())}/{gc.NBLK} (noise side {n_noise}, texture side {n_tex}, dropped with a non-zero vector "
                  f"{n_dropped_moving}), area {a0} -> {a1}, lsq {q0} -> {q1}")
            assert abs(a0 - a1) >= 10, f"frame {k} {what}: the detector cannot tell the check from its absence"
            assert np.abs(q0 - q1).max() > 1e-4, f"frame {k} {what}: the estimator cannot tell the check from its absence"


def test_flat_frame_round_trips_exactly():
    """a clean flat block is the contrast gate's business: both directions return 0 and the check keeps all 240"""
    flat = gc.flat_frame()
    F2 = np.asarray(oracle.sad_flow(flat, flat, gc.BLOCK, gc.RANGE)[1])
    assert not F2[:, :2].any() and cc.keep_flags(F2, F2, gc.FRAME_W, gc.FRAME_H, gc.BLOCK, cc.LIMIT).all()
    assert not gc.keep_flags(flat, gc.BLOCK, gc.GATE).any()
