"""No GPU: every case of tests/almeida_domain_cases.py has the property it is listed for, on the CPU oracle -- sentinels that matter at
100 x the parity bound while the summation order does not, RANSAC cases whose winner is pinned and cannot be flipped by f32 rounding,
all-inlier cases whose refit set is known without the oracle's RANSAC routine -- and the chooser literals are the chooser's."""
import numpy as np
import pytest

import almeida_domain_cases as dc
import indep_ransac as ir
import oracle
from ofps_amd import synth


def _d(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _sentinel_matters(s, idx, what):
    """dropping the sentinel record, and counting it twice, each move the oracle by >= EFFECT_MIN"""
    q = dc.solve(s)
    assert np.isfinite(q).all(), what
    drop = _d(dc.solve(np.delete(s, idx, 0)), q)
    twice = _d(dc.solve(np.concatenate([s, s[idx:idx + 1]])), q)
    assert drop >= dc.EFFECT_MIN and twice >= dc.EFFECT_MIN, (what, drop, twice)
    return q


def _order_does_not(s, q, what, seed=5, perms=2):
    rng = np.random.default_rng(seed)
    for _ in range(perms):
        assert _d(dc.solve(s[rng.permutation(len(s))]), q) <= dc.PERM_MAX, what


@pytest.mark.parametrize("case", dc.LSQ_COUNTS, ids=lambda c: c.name)
def test_lsq_sentinels_matter_and_the_order_does_not(case):
    e = dc.field(case.n)
    assert e.shape == (case.n, 4)
    assert len(case.idx) <= 6 and case.idx == dc.sentinel_indices(case.n, case.per_wg, case.nblk)[:len(case.idx)]
    # +4.0, doubled until the sentinel matters enough; 2^-4 for the fields of three and four records, where a record four screens
    # off drives the oracle itself to rotations near 180 degrees and its answer moves by 0.9 under a permutation
    assert case.mag in ((0.0,) if not case.idx else (0.0625,) if case.n < 16 else (4.0, 8.0, 16.0, 32.0, 64.0))
    for k, idx in enumerate(case.idx):
        s = dc.sentinel(e, idx, case.mag)
        assert _d(s[idx, 2:], e[idx, 2:] + np.float32(case.mag)) == 0 and np.array_equal(np.delete(s, idx, 0), np.delete(e, idx, 0))
        q = _sentinel_matters(s, idx, (case.name, idx))
        assert np.array_equal(q, dc.lsq_expected(case, idx))
        if k == 0: _order_does_not(s, q, (case.name, idx))
    if not case.idx:                                        # one record: a singular system with one summation order -- the identity
        assert case.n == 1 and np.array_equal(dc.solve(e), np.array([1, 0, 0, 0], np.float32))


def test_lsq_table_covers_the_issue_s_counts():
    by = lambda pre: sorted(c.n for c in dc.LSQ_COUNTS if c.name.startswith(pre))
    assert by("wg_") == [3, 4, 63, 64, 65, 1023, 1024, 1025, 1535, 1536]
    assert by("wgf_") == [2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192]
    assert by("cl_") == [1537, 8040, 16383, 16384, 16385, 32768, 32769, 65535, 65536, 65537, 66000]
    assert by("cl1024x") == sorted(k * e * 1024 + d for e in (1, 2, 4) for k in (1, 3) for d in (-1, 1))
    assert by("step_") == [1, 3, 1023, 1025, 8193, 65536, 65537, 73729]
    assert max(c.n for c in dc.LSQ_COUNTS) == 73729


@pytest.mark.parametrize("case", dc.LSQ_COUNTS, ids=lambda c: c.name)
def test_chooser_literals(case):
    block, ept = (1024, case.ept) if (case.force == "cluster") else (0, 0)
    assert dc.chooser(case.n, case.force, block, ept) == (case.path, case.block, case.ept, case.per_wg, case.nblk)
    assert dc.options(case) == ({} if case.force is None else {"OFPS_HIP_ALMEIDA_PATH": case.force} if case.force != "cluster" else
                                {"OFPS_HIP_ALMEIDA_PATH": "cluster", "OFPS_HIP_ALMEIDA_BLOCK": 1024, "OFPS_HIP_ALMEIDA_EPT": case.ept})


def test_chooser_thresholds():
    """the places where the chooser changes its mind, as the issue lists them"""
    assert dc.chooser(1536)[0] == "wg" and dc.chooser(1537) == ("cluster", 256, 1, 256, 7)          # the first cluster launch
    assert dc.chooser(16384)[2] == 1 and dc.chooser(16385)[2] == 2 and dc.chooser(32768)[2] == 2 and dc.chooser(32769)[2] == 4
    assert dc.chooser(16384)[4] == 64 and dc.chooser(32768)[4] == 64 and dc.chooser(65536)[4] == 64  # the one-XCD limit
    assert dc.chooser(65536)[1] == 256 and dc.chooser(65537)[1] == 1024                              # the dense 1024-thread form
    assert dc.chooser(73729, "step") == ("step", 1024, 8, 8192, 10) and 73729 == 9 * 8192 + 1


@pytest.mark.parametrize("case", dc.BATCHES, ids=lambda c: c.name)
def test_batch_items_differ_and_their_sentinels_matter(case):
    B = dc.batch_size(case)
    assert B * case.n <= 2_000_000 and case.n <= 73729
    path, block, ept, per_wg, nblk = dc.chooser(case.n, case.force, 0, case.force_ept, B)
    assert (path, block, ept, per_wg, nblk) == (case.path, case.block, case.ept, case.per_wg, case.nblk)
    if path == "cluster":
        assert dc.CUS // nblk == case.per_launch
        if case.batch is None: assert B == case.per_launch + 2                  # a full launch, then one of two items
    if case.name == "step_100x9000": assert nblk < -(-case.n // 1024)           # the cap: the strided loop runs more than once
    idx = [dc.item_index(case, b, B) for b in range(B)]
    assert len(set(idx)) == B and all(0 <= i < case.n for i in idx)
    quats = [oracle.quat_from_euler(*np.radians(dc.item_euler(b)).astype(np.float32)) for b in range(B)]
    for a in range(B):
        for b in range(a + 1, B):
            assert synth.quat_angle_deg(quats[a], quats[b]) >= 0.3, (a, b)
    for b in range(B):
        s = dc.sentinel(dc.item_field(case, b), idx[b], case.mag)
        q = _sentinel_matters(s, idx[b], (case.name, b))
        assert np.array_equal(q, dc.batch_expected(case, b, B))
        if b == 0: _order_does_not(s, q, (case.name, b))


# ---- RANSAC ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.RANSAC_SELECTION, ids=lambda c: c.name)
def test_selection_literals_hold_and_cannot_flip(case):
    e = dc.sel_field(case)
    m = dc.sel_mask(case)
    assert e.shape == (dc.SEL_N, 4) and int(m.sum()) == {"even_odd": 96, "split60": 116, "keep": 18}[case.kind]
    r = ir.run(e, dc.ASPECT, dc.FOV, case.seed, case.iters, dc.SEL_DEG, dc.SEL_N)
    assert r.robust(), case.name
    assert r.winner == case.winner and (r.hyps[r.winner].count if r.winner >= 0 else 0) == case.count
    q, inl = oracle.solve_ypr_ransac(e, dc.cam(), case.iters, dc.SEL_DEG, dc.SEL_N, case.seed, want_inliers=True)
    assert len(inl) == case.count
    if case.winner < 0:
        assert np.array_equal(q, np.array([1, 0, 0, 0], np.float32))
        return
    # the oracle's inliers are the winner's population, in the winner's sample order
    h = r.hyps[case.winner]
    pure = m[list(h.drawn)]
    assert (pure.all() and case.pop == "A") or (not pure.any() and case.pop == "B")
    want = [int(i) for i in h.sampled if m[i] == (case.pop == "A")]
    assert inl.tolist() == want
    # ... and no earlier hypothesis reaches the count; the first one that does is the winner
    c = r.counts
    assert (c[:case.winner] < case.count).all() and c.max() == case.count
    if case.kind != "keep":
        other = "B" if case.pop == "A" else "A"
        assert synth.quat_angle_deg(q, dc.sel_pop_answer(case.pop)) < 0.01
        assert synth.quat_angle_deg(q, dc.sel_pop_answer(other)) > 1.0           # the populations' answers are 1.13 degrees apart
        assert _d(q, dc.sel_pop_answer(other)) > 50 * dc.RANSAC_BOUND


def test_selection_table_covers_the_issue_s_list():
    s = {c.name: c for c in dc.RANSAC_SELECTION}
    assert s["B_then_A"].pop == "B" and s["A_then_B"].pop == "A"
    assert (s["last_quad_16"].winner, s["last_quad_16"].iters, s["last_quad_17"].winner, s["last_quad_17"].iters) == (15, 16, 15, 17)
    assert (s["first_quad_17"].winner, s["first_quad_17"].iters) == (16, 17)
    assert any(c.winner == c.iters - 1 for c in dc.RANSAC_SELECTION)
    assert s["none_4"].winner == -1 and s["split60"].count == 116
    assert s["late_1025"].iters == 1025 and s["late_1025"].winner >= 1024 and s["late_2049"].iters == 2049 and s["late_2049"].winner > 1024


@pytest.mark.parametrize("case", dc.RANSAC_ALL_INLIERS, ids=lambda c: "%dx%d" % (c.n, c.ns))
def test_all_inlier_cases(case):
    ns = min(case.ns, case.n)
    s = dc.all_sampled(case)
    assert len(set(s.tolist())) == ns                                           # the sampler is a permutation: no record twice
    mag = dc.all_mag(ns)
    assert 2 * (mag + 1) ** 2 < np.radians(dc.ALL_DEG) ** 2 / 16               # the sentinel stays an inlier, far below the band
    runs = (None,) + dc.all_positions(case) + (("unsampled",) if dc.all_unsampled(case) is not None else ())
    assert "unsampled" in runs or case.n <= 5 or ns == case.n
    q_plain = None
    for pos in runs:
        f, refit = dc.all_field(case, pos)
        q = dc.solve(refit)
        q_o, inl = oracle.solve_ypr_ransac(f, dc.cam(), dc.ALL_ITERS, dc.ALL_DEG, case.ns, dc.ALL_SEED, want_inliers=True)
        assert np.array_equal(inl, s), (case, pos)                              # every sampled record, in sample order
        assert _d(q, q_o) <= dc.BOUND, (case, pos)
        if pos is None: q_plain = q
        elif pos == "unsampled": assert np.array_equal(q, q_plain)               # it is not in the refit set: it does not matter
        else:
            assert np.array_equal(refit[pos], dc.sentinel(dc.field(case.n), int(s[pos]), mag)[int(s[pos])])
            _sentinel_matters(refit, pos, (case, pos))
            if pos == 0 and ns > 3: _order_does_not(refit, q, (case, pos))


@pytest.mark.parametrize("case", [c for c in dc.RANSAC_PARAMS if c.identity is not False], ids=lambda c: c.name)
def test_param_cases_that_hinge_on_a_count_of_three(case):
    """samples 1 .. 4 and the tiny threshold: whether the best count reaches three decides between a solve and the identity, so the
    decision must not be one that f32 rounding can flip"""
    e = dc.par_field(case)
    r = ir.run(e, dc.ASPECT, dc.FOV, case.seed, case.iters, case.deg, case.ns)
    best = int(r.counts.max())
    q = dc.par_expected(case)
    if case.identity:
        assert best < 3 and all(int((h.r2 < ir.BAND * r.thr2).sum()) < 3 for h in r.hyps)      # not even the band's records make three
        assert np.array_equal(q, np.array([1, 0, 0, 0], np.float32))
    else:
        assert best >= 3 and r.robust()
        assert not np.array_equal(q, np.array([1, 0, 0, 0], np.float32))


def test_param_table_covers_the_issue_s_list():
    assert sorted(c.iters for c in dc.RANSAC_PARAMS if c.name.startswith("iters_")) == [1, 15, 16, 17, 1023, 1024, 1025, 65535]
    big = next(c for c in dc.RANSAC_PARAMS if c.iters == 65535)
    assert (big.w * big.h, big.ns) == (64, 64)
    assert sorted(c.ns for c in dc.RANSAC_PARAMS if c.name.startswith("samples_")) == [1, 2, 3, 4]
    for c in dc.RANSAC_PARAMS:
        e = dc.par_field(c)
        assert e.shape == (c.w * c.h, 4)
        if c.identity is False:                             # the plain parity cases have something to compare: not the identity
            assert not np.array_equal(dc.par_expected(c), np.array([1, 0, 0, 0], np.float32)), c.name


def test_refusal_table_covers_the_issue_s_list():
    names = {r.name for r in dc.REFUSALS}
    assert {"batch_0", "batch_65536", "aspect_0", "aspect_neg", "fov_0", "fov_180", "fov_nan", "iters_0", "iters_65536", "samples_0",
            "null_entries", "null_output"} <= names
    assert all(r.text.startswith("almeida: ") and r.form in ("dev", "host", "both") for r in dc.REFUSALS)
