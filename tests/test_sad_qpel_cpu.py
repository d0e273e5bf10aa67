"""CPU tests of N1q's NumPy restatement (tests/indep_sad_qpel.py) against hand-derived literals: the H.264 six-tap filter,
its rounding and saturation, the quarter-pel averages of every fractional phase, edge replication, and the refinement's
own rules (validity, total order, records).  The GPU tests hold the HIP kernel to this restatement bit for bit."""
import os

import numpy as np
import pytest

import oracle
from ofps_amd import synth

import indep_sad_qpel as iq
import sad_qpel_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sad_qpel.npz")


def _rows(row, n=8):
    return np.tile(np.asarray(row, np.uint8), (n, 1))


def test_six_tap_impulse_response():
    imp = np.zeros((1, 12), np.int64); imp[0, 5] = 1
    np.testing.assert_array_equal(iq._tap6(imp, 1)[0], [0, 0, 1, -5, 20, 20, -5, 1, 0, 0, 0])
    # an impulse of 32: b1 = 32 w, b = clip((32 w + 16) >> 5) = clip(w): the negative taps saturate at 0
    row = np.zeros(12, np.uint8); row[5] = 32
    hg = iq.half_plane(_rows(row))
    np.testing.assert_array_equal(hg[0, 1::2], [0, 0, 1, 0, 20, 20, 0, 1, 0, 0, 0])
    np.testing.assert_array_equal(hg[0, 0::2], row)                           # integer samples untouched
    # the same down a column
    hg = iq.half_plane(_rows(row).T.copy())
    np.testing.assert_array_equal(hg[1::2, 0], [0, 0, 1, 0, 20, 20, 0, 1, 0, 0, 0])


def test_half_pel_rounding():
    # impulse 16: b1 = 16 w -> (16 + 16) >> 5 = 1, (320 + 16) >> 5 = 10 (10.5 rounds down: the +16 is the only rounding),
    # (-80 + 16) >> 5 = -2 -> 0
    row = np.zeros(12, np.uint8); row[5] = 16
    np.testing.assert_array_equal(iq.half_plane(_rows(row))[0, 1::2], [0, 0, 1, 0, 10, 10, 0, 1, 0, 0, 0])
    # impulse 4: (80 + 16) >> 5 = 3, (4 + 16) >> 5 = 0
    row[5] = 4
    np.testing.assert_array_equal(iq.half_plane(_rows(row))[0, 1::2], [0, 0, 0, 0, 3, 3, 0, 0, 0, 0, 0])
    # a constant frame is a fixed point: (32 v + 16) >> 5 = v, (1024 v + 512) >> 10 = v
    for v in (0, 1, 77, 254, 255):
        assert (iq.quarter_plane(np.full((7, 9), v, np.uint8)) == v).all()


def test_saturation_at_0_and_255():
    # step 0 -> 255 between columns 3 and 4
    row = np.array([0, 0, 0, 0, 255, 255, 255, 255, 255, 255], np.uint8)
    b = iq.half_plane(_rows(row))[0, 1::2]
    assert b[2] == 0          # taps (0,0,0,0,255,255): (-5 + 1) * 255 = -1020 -> 0
    assert b[3] == 128        # taps (0,0,0,255,255,255): 16 * 255 = 4080, (4080 + 16) >> 5 = 128
    assert b[4] == 255        # taps (0,0,255,255,255,255): 36 * 255 = 9180, (9180 + 16) >> 5 = 287 -> 255
    # j saturates through the UNROUNDED b1: a 2-D step corner
    img = np.zeros((10, 10), np.uint8); img[4:, 4:] = 255
    hg = iq.half_plane(img)
    assert hg[2 * 4 + 1, 2 * 4 + 1] == 255          # 36 * 36 * 255 = 330480, (330480 + 512) >> 10 = 323 -> 255
    assert hg[2 * 3 + 1, 2 * 3 + 1] == 64           # 16 * 16 * 255 = 65280, (65280 + 512) >> 10 = 64
    assert hg[2 * 2 + 1, 2 * 2 + 1] == 4            # (-4) * (-4) * 255 = 4080, (4080 + 512) >> 10 = 4
    assert hg[2 * 2 + 1, 2 * 4 + 1] == 0            # (-4) * 36 * 255 < 0 -> 0


def test_binary_frames_take_both_clip_branches_of_b_h_and_j():
    """The sweeps' `binary` kind (only 0 and 255) drives every half-pel formula past both clip limits: shown on the UNCLIPPED
    intermediates, so the GPU sweep that replays those frames provably runs clip255's two branches in b, h and j."""
    a = cases.frames(64, 64, 64, 64, 1000, "binary")[0].astype(np.int64)
    b1, h1 = iq._tap6(a, 1), iq._tap6(a, 0)
    j1 = iq._tap6(b1, 0)
    assert b1.max() <= 10710 and b1.min() >= -2550                 # (1 + 20 + 20 + 1) * 255 and -(5 + 5) * 255: int16 holds b1
    for name, v in (("b", (b1 + 16) >> 5), ("h", (h1 + 16) >> 5), ("j", (j1 + 512) >> 10)):
        assert (v < 0).any() and (v > 255).any(), name
        assert v.min() < -30 and v.max() > 300, name               # well past the limits, not by a rounding step
    hg = iq.half_plane(a.astype(np.uint8))
    assert hg.min() == 0 and hg.max() == 255


def test_linear_ramp_is_reproduced_exactly():
    # a = 10 + 4x + 8y: the six taps sum to 32 with first moment 16, so b = a + 2, h = a + 4, j = a + 6 and every quarter
    # sample is 10 + X + 2Y exactly (X, Y in quarter pels), away from the replicated edges (2 samples before, 3 after)
    H, W = 16, 24
    yy, xx = np.mgrid[0:H, 0:W]
    q = iq.quarter_plane((10 + 4 * xx + 8 * yy).astype(np.uint8))
    Y, X = np.mgrid[0:q.shape[0], 0:q.shape[1]]
    inner = (slice(8, 4 * (H - 1) - 12 + 1), slice(8, 4 * (W - 1) - 12 + 1))
    np.testing.assert_array_equal(q[inner], (10 + X + 2 * Y)[inner])


def test_edge_replication_at_all_four_borders():
    n = 10
    row = np.zeros(n, np.uint8); row[0] = 32
    # left: taps for the half sample between 0 and 1 read columns (-2,-1,0 -> 0), 1, 2, 3: (1 - 5 + 20) * 32 -> 16;
    # between 1 and 2: (1 - 5) * 32 -> 0; between 2 and 3: 1 * 32 -> 1
    np.testing.assert_array_equal(iq.half_plane(_rows(row))[0, 1::2][:4], [16, 0, 1, 0])
    np.testing.assert_array_equal(iq.half_plane(_rows(row).T.copy())[1::2, 0][:4], [16, 0, 1, 0])       # top
    row = np.zeros(n, np.uint8); row[-1] = 32
    # right: between n-2 and n-1 reads n-4, n-3, n-2, then n-1 three times: (20 - 5 + 1) * 32 -> 16; before it (-5 + 1) -> 0; then 1
    np.testing.assert_array_equal(iq.half_plane(_rows(row))[0, 1::2][-4:], [0, 1, 0, 16])
    np.testing.assert_array_equal(iq.half_plane(_rows(row).T.copy())[1::2, 0][-4:], [0, 1, 0, 16])      # bottom


def test_all_fifteen_fractional_phases_on_a_hand_worked_patch():
    """One impulse G = 64 at (3, 3).  H.264's letters around G (8.4.2.2.1, figure 8-4): b = h = (20 * 64 + 16) >> 5 = 40,
    j = (20 * 20 * 64 + 512) >> 10 = 25, m = s = 0 (the column / row next to G is empty); a = (G + b + 1) >> 1 = 52,
    c = (H + b + 1) >> 1 = 20, e = (b + h + 1) >> 1 = 40, f = (b + j + 1) >> 1 = 33, g = (b + m + 1) >> 1 = 20,
    k = (j + m + 1) >> 1 = 13, r = (m + s + 1) >> 1 = 0, and d, n, i, p, q by symmetry.  Rows fy = 0..3, columns fx = 0..3."""
    img = np.zeros((8, 8), np.uint8); img[3, 3] = 64
    q = iq.quarter_plane(img)
    np.testing.assert_array_equal(q[12:16, 12:16], [[64, 52, 40, 20],
                                                    [52, 40, 33, 20],
                                                    [40, 33, 25, 13],
                                                    [20, 20, 13, 0]])
    # the pixel LEFT of the impulse (its H is the impulse): G = 0, b = 40, h = 0, j = 25, m = 40, s = 0 -- asymmetric, so
    # g = (b + m + 1) >> 1 = 40 and p = (h + s + 1) >> 1 = 0 cannot be swapped unnoticed
    np.testing.assert_array_equal(q[12:16, 8:12], [[0, 20, 40, 52],
                                                   [0, 20, 33, 40],
                                                   [0, 13, 25, 33],
                                                   [0, 0, 13, 20]])
    # and the pixel ABOVE it: the transpose
    np.testing.assert_array_equal(q[8:12, 12:16], np.array([[0, 20, 40, 52], [0, 20, 33, 40], [0, 13, 25, 33], [0, 0, 13, 20]]).T)


def _h264_sample(img, X, Y):
    """ITU-T H.264 8.4.2.2.1 letter by letter for one quarter-pel position: scalar, nothing shared with the restatement"""
    H, W = img.shape
    px = lambda x, y: int(img[min(max(y, 0), H - 1), min(max(x, 0), W - 1)])
    t6 = lambda v: v[0] - 5 * v[1] + 20 * v[2] + 20 * v[3] - 5 * v[4] + v[5]
    c1 = lambda v: min(max((v + 16) >> 5, 0), 255)
    xi, yi, xf, yf = X >> 2, Y >> 2, X & 3, Y & 3
    b1 = lambda x, y: t6([px(x + k, y) for k in range(-2, 4)])            # between (x, y) and (x+1, y)
    h1 = lambda x, y: t6([px(x, y + k) for k in range(-2, 4)])            # between (x, y) and (x, y+1)
    G, Hh, M = px(xi, yi), px(xi + 1, yi), px(xi, yi + 1)
    b, h = c1(b1(xi, yi)), c1(h1(xi, yi))
    s, m = c1(b1(xi, yi + 1)), c1(h1(xi + 1, yi))
    j = min(max((t6([b1(xi, yi + k) for k in range(-2, 4)]) + 512) >> 10, 0), 255)
    avg = lambda p, q: (p + q + 1) >> 1
    table = {(0, 0): G, (1, 0): avg(G, b), (2, 0): b, (3, 0): avg(Hh, b),
             (0, 1): avg(G, h), (1, 1): avg(b, h), (2, 1): avg(b, j), (3, 1): avg(b, m),
             (0, 2): h, (1, 2): avg(h, j), (2, 2): j, (3, 2): avg(j, m),
             (0, 3): avg(M, h), (1, 3): avg(h, s), (2, 3): avg(j, s), (3, 3): avg(m, s)}
    return table[(xf, yf)]


def test_quarter_plane_equals_the_standards_table_on_noise():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (9, 11)).astype(np.uint8)
    q = iq.quarter_plane(img)
    assert q.shape == (4 * 8 + 1, 4 * 10 + 1)
    for Y in range(q.shape[0]):
        for X in range(q.shape[1]):
            assert q[Y, X] == _h264_sample(img, X, Y), (X, Y)


CASES = [(96, 64, 16, 8, "seq"), (64, 48, 8, 8, "seq"), (60, 48, 12, 5, "seq"), (100, 70, 16, 16, "random"), (64, 64, 32, 4, "seq")]


def _frames(W, H, R, kind):
    if kind == "random":
        return synth.random_luma(2, W, H, seed=7)
    return synth.luma_sequence(2, W, H, max_step=min(R, 3), seed=synth.SEED0 + W + H)


@pytest.mark.parametrize("W,H,B,R,kind", CASES)
def test_refinement_rules(W, H, B, R, kind):
    fr = _frames(W, H, R, kind)
    ent_i, best_i = oracle.sad_flow(fr[0], fr[1], B, R)
    ent, best = iq.refine(fr[0], fr[1], B, R, best_i)
    # refined SAD <= integer SAD for every block (f = 0 is always a candidate), the winner within +-3 of 4 d
    assert (best[:, 2] <= best_i[:, 2]).all()
    assert (np.abs(best[:, :2] - 4 * best_i[:, :2]) <= 3).all()
    # every sample of the winning block inside the frame
    nbx = W // B
    x0 = (np.arange(len(best)) % nbx) * B; y0 = (np.arange(len(best)) // nbx) * B
    assert (4 * x0 + best[:, 0] >= 0).all() and (4 * (x0 + B - 1) + best[:, 0] <= 4 * (W - 1)).all()
    assert (4 * y0 + best[:, 1] >= 0).all() and (4 * (y0 + B - 1) + best[:, 1] <= 4 * (H - 1)).all()
    # a block whose winner stayed on the integer grid has the full-pel record's position and motion (x 0.25 and / 4 are exact)
    same = (best[:, :2] == 4 * best_i[:, :2]).all(axis=1)
    np.testing.assert_array_equal(ent[same].view(np.uint32), ent_i[same].view(np.uint32))
    np.testing.assert_array_equal(best[same, 2], best_i[same, 2])


def test_f_zero_reproduces_the_integer_search_sad():
    fr = _frames(96, 64, 8, "seq")
    _, best_i = oracle.sad_flow(fr[0], fr[1], 16, 8)
    q = iq.quarter_plane(fr[0])
    for k, (dx, dy, sad) in enumerate(best_i):
        x0, y0 = (k % 6) * 16, (k // 6) * 16
        ref = q[4 * (y0 + dy):4 * (y0 + dy + 16):4, 4 * (x0 + dx):4 * (x0 + dx + 16):4].astype(int)
        assert np.abs(fr[1][y0:y0 + 16, x0:x0 + 16].astype(int) - ref).sum() == sad


def test_flat_frame_keeps_the_integer_winner():
    fr = np.full((2, 48, 64), 77, np.uint8)
    _, best_i = oracle.sad_flow(fr[0], fr[1], 16, 8)
    _, best = iq.refine(fr[0], fr[1], 16, 8, best_i)
    np.testing.assert_array_equal(best[:, :2], 4 * best_i[:, :2])              # every candidate ties at 0: the smallest |D| wins
    assert (best == 0).all()


@pytest.mark.parametrize("D0", [(5, -7), (-2, 3), (1, 0), (-6, -5)])
def test_known_quarter_pel_shift_is_recovered(D0):
    """cur = prev rendered at a quarter-pel offset with the same interpolation: the candidate D0 has SAD 0, the least possible."""
    W, H, B, R = 160, 96, 16, 8
    prev = synth.luma_sequence(1, W, H, max_step=0, seed=91)[0]
    q = iq.quarter_plane(prev)
    Y, X = np.mgrid[0:H, 0:W]
    cur = q[np.clip(4 * Y + D0[1], 0, q.shape[0] - 1), np.clip(4 * X + D0[0], 0, q.shape[1] - 1)]
    _, best_i = oracle.sad_flow(prev, cur, B, R)
    _, best = iq.refine(prev, cur, B, R, best_i)
    nbx, nby = W // B, H // B
    interior = np.array([0 < k % nbx < nbx - 1 and 0 < k // nbx < nby - 1 for k in range(nbx * nby)])
    reach = (np.abs(4 * best_i[:, :2] - np.array(D0)) <= 3).all(axis=1)        # D0 is among the 49 candidates of the block
    assert (reach & interior).sum() >= 0.9 * interior.sum()
    np.testing.assert_array_equal(best[reach & interior, 2], 0)
    np.testing.assert_array_equal(best[reach & interior, :2], np.tile(D0, ((reach & interior).sum(), 1)))


def test_sweep_refine_equals_the_plain_tuple_minimum_and_the_sweep_covers_the_domain():
    """The whole accepted domain (blocks 1..64, ranges 0..64, frames from 1x1, five kinds of content; tests/sad_qpel_cases.py)
    through oracle.sad_flow -> refine: the packed-key winner == Python's min over (SAD, Dx^2 + Dy^2, Dy, Dx) tuples, and the
    refinement's rules hold.  Then the coverage conditions over the whole run, from the restatement's output alone: the GPU
    sweeps replay these examples (and assert the same conditions), so they cannot be vacuous."""
    obs = []

    @cases.sweep
    def run(case):
        w, h, b, r, _, _ = case
        fr = cases.frames(*case)
        _, best_i = oracle.sad_flow(fr[0], fr[1], b, r)
        ent, best = iq.refine(fr[0], fr[1], b, r, best_i)
        ent_t, best_t, n_valid = iq.refine_by_tuples(fr[0], fr[1], b, r, best_i)
        assert len(best) == (w // b) * (h // b)
        np.testing.assert_array_equal(best, best_t)
        np.testing.assert_array_equal(ent.view(np.uint32), ent_t.view(np.uint32))
        obs.append(cases.observe(case, best, n_valid))
        if not len(best):
            return
        assert (best[:, 2] <= best_i[:, 2]).all()                              # f = 0 is always a candidate
        assert (np.abs(best[:, :2] - 4 * best_i[:, :2]) <= 3).all()
        nbx = w // b
        x0 = (np.arange(len(best)) % nbx) * b; y0 = (np.arange(len(best)) // nbx) * b
        assert (4 * x0 + best[:, 0] >= 0).all() and (4 * (x0 + b - 1) + best[:, 0] <= 4 * (w - 1)).all()
        assert (4 * y0 + best[:, 1] >= 0).all() and (4 * (y0 + b - 1) + best[:, 1] <= 4 * (h - 1)).all()
        assert (n_valid >= 1).all() and (n_valid <= 49).all()
        # at f = 0 the quarter plane gives the integer search's SAD
        q = iq.quarter_plane(fr[0]).astype(np.int64)
        yy, xx = np.meshgrid(np.arange(b), np.arange(b), indexing="ij")
        ref = q[4 * (y0 + best_i[:, 1])[:, None, None] + 4 * yy, 4 * (x0 + best_i[:, 0])[:, None, None] + 4 * xx]
        cblk = fr[1][y0[:, None, None] + yy, x0[:, None, None] + xx].astype(np.int64)
        np.testing.assert_array_equal(np.abs(cblk - ref).sum(axis=(1, 2)), best_i[:, 2])

    run()
    cases.coverage(obs)                                                        # prints the measured values (pytest -s)


def test_records_follow_the_spec_formula():
    best = np.array([[5, -7, 0], [-3, 2, 9]], np.int32)
    e = iq.entries(best, 16, 32, 16)
    f = np.float32
    assert e[0, 0] == f(f(4 * 8 + 5) * f(0.25)) * (f(1) / f(32)) and e[0, 2] == f(f(5) / f(4)) * -(f(1) / f(32))
    assert e[1, 0] == f(f(4 * 24 - 3) * f(0.25)) * (f(1) / f(32)) and e[1, 3] == f(f(2) / f(4)) * -(f(1) / f(16))
    assert e[0, 1] == f(f(4 * 8 - 7) * f(0.25)) * (f(1) / f(16))


def test_golden_fixture_is_what_the_restatement_gives():
    g = np.load(GOLDEN)
    for name in ("a", "b", "c"):
        W, H, B, R = (int(v) for v in g[f"{name}_geom"])
        fr = g[f"{name}_frames"]
        _, best_i = oracle.sad_flow(fr[0], fr[1], B, R)
        np.testing.assert_array_equal(best_i, g[f"{name}_best_int"])
        ent, best = iq.refine(fr[0], fr[1], B, R, best_i)
        np.testing.assert_array_equal(best, g[f"{name}_best"])
        np.testing.assert_array_equal(ent.view(np.uint32), g[f"{name}_entries"].view(np.uint32))
        assert (best[:, :2] != 4 * best_i[:, :2]).any()                        # the fixture exercises fractional winners
