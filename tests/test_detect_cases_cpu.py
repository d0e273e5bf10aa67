"""No GPU: every case of tests/detect_cases.py has the property it is named for, on the C oracle and on np_oracle.detect_motion (scipy's
labelling: independent in form of the C oracle's flood fill) -- the two agree bit for bit on outcome, area and field over the whole list --
and the literals the cases carry (area, Some / None, seed cell) are what both compute.  tests/test_detect_domain_gpu.py runs the same
cases on the device; a case that lost its property would let that file pass vacuously."""
import numpy as np
import pytest
from scipy import ndimage

import detect_cases as dc
import oracle
from oracle import np_oracle

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


_islands = {}


def islands(case):
    """the on-map from the C oracle's densified field, labelled 8-connected -> (labels [d, d], areas, first cell per island, field)"""
    if case.name not in _islands:
        d = case.side
        f = oracle.densify(case.make(), d, d)
        with np.errstate(invalid="ignore", over="ignore"):
            mask = dc.mag_separate(f) >= F(case.params["target_motion"])
        lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))
        areas = np.bincount(lab.ravel(), minlength=n + 1)[1:]
        first = np.full(n + 1, d * d)
        np.minimum.at(first, lab.ravel(), np.arange(d * d))
        _islands[case.name] = (lab, areas, first[1:], f)
    return _islands[case.name]


def winner(case):
    lab, areas, first, _ = islands(case)
    if len(areas) == 0:
        return 0, None, None
    k = max(range(len(areas)), key=lambda j: (areas[j], -first[j]))
    return int(areas[k]), int(first[k]), lab == k + 1


# ------------------------------------------------------------------------------------------------------------------------------- the grid
def test_grid_reaches_the_sides_where_the_code_changes_behaviour():
    sides = tuple(oracle.block_dim(*p) for p in dc.GRID)
    assert sides == dc.GRID_SIDES == tuple(np_oracle.block_dim(*p) for p in dc.GRID)
    assert set(dc.REQUIRED_SIDES) <= set(sides) and {129, 159} <= set(sides)
    assert all(0.01 <= m <= 1.0 and 1 <= s <= 16 for m, s in dc.GRID)                   # plugins.py: the property ranges
    assert oracle.block_dim(*dc.SIDE_161) == 161 and dc.SIDE_161[0] < 0.01
    for d in dc.GRID_SIDES:                              # the LDS the detector asks for: 4 B + 2 B per cell, the second part rounded to 16
        lds = 4 * d * d + ((2 * d * d + 15) & ~15)
        assert (lds > 48 * 1024) == (d >= 91)


def test_block_dim_of_the_library_over_the_whole_property_range():
    from ofps_amd import _lib
    lib = _lib.load()                                    # loads without a GPU (tests/test_cabi.py)
    reached = set()
    for s in range(1, 17):
        for k in range(10, 1001):
            m = k / 1000.0
            d = lib.ofps_hip_block_dim(m, s)
            assert d == oracle.block_dim(m, s) == np_oracle.block_dim(m, s), (m, s)
            reached.add(d)
    assert 1 <= min(reached) and max(reached) == 160
    assert set(dc.REQUIRED_SIDES) <= reached


def test_block_dim_of_degenerate_arguments_is_outside_the_accepted_sides():
    from ofps_amd import _lib
    lib = _lib.load()
    assert lib.ofps_hip_block_dim(0.05, 0) == 0          # 1 / (sqrt(m) / 0) = 0
    assert lib.ofps_hip_block_dim(-0.05, 3) == 0         # sqrt of a negative: NaN -> 0
    assert lib.ofps_hip_block_dim(float("nan"), 3) == 0
    assert lib.ofps_hip_block_dim(1e-9, 1) == 31623 > 160
    assert lib.ofps_hip_block_dim(*dc.SIDE_161) == 161


# ---------------------------------------------------------------------------------------------------------------------------- the entry maker
@pytest.mark.parametrize("d", dc.GRID_SIDES)
def test_entries_land_in_the_chosen_cells(d):
    on = dc.all_on(d)
    e = dc.entries(d, on, background=False)
    assert e.dtype == F and e.shape == (d * d, 4)
    assert ((e[:, :2] > 0) & (e[:, :2] < 1)).all()       # strictly inside: the all-component clamp leaves them alone
    x, y = np_oracle.cell_index(e, d, d)
    assert [tuple(c) for c in np.stack([x, y], 1)] == on
    _, cells = oracle.densify(e, d, d, want_cells=True)
    assert [tuple(c) for c in cells] == on
    # still background: one record in every cell that is not lit, behind the lit ones
    lit = dc.antidiagonal(d)
    e = dc.entries(d, lit, counts=3)
    assert len(e) == 3 * d + d * d - d and (e[:3 * d, 2] == F(dc.MOVE[0])).all() and (e[3 * d:, 2:] == 0).all()
    x, y = np_oracle.cell_index(e, d, d)
    assert sorted(set(zip(x[3 * d:], y[3 * d:]))) == sorted(set(on) - set(lit))


# ------------------------------------------------------------------------------------------------------------------------------ every case
@pytest.mark.parametrize("case", dc.ALL_CASES, ids=lambda c: c.name)
def test_case_has_its_literals_on_both_oracles(case):
    d, e = case.side, case.make()
    assert oracle.block_dim(case.params["min_size"], case.params["subdivide"]) == d and 1 <= d <= 160
    area, seed, member = winner(case)
    assert (area, seed) == (case.area, case.seed)
    some = bool(area) and bool(F(area) / F(d * d) >= F(case.params["min_size"]))
    assert some == case.some
    has, area_o, field_o = dc.expected(e, case.params)
    assert has == case.some and area_o == (case.area if case.some else 0)
    want = np.zeros((d, d, 2), F)
    if some:
        member = member.copy()
        member.ravel()[seed] = False                     # the seed is never copied
        want[member] = islands(case)[3][member]
    np.testing.assert_array_equal(_bits(field_o), _bits(want))
    with np.errstate(invalid="ignore"):
        r = np_oracle.detect_motion(e, **case.params)    # the second oracle: same outcome, area and bits
    assert (r is not None) == has
    if has:
        assert r[0] == area_o
        np.testing.assert_array_equal(_bits(r[1]), _bits(field_o))


def _case(name):
    return dc.BY_NAME[name]


def test_shapes_are_what_they_are_named_for():
    for c in dc.SHAPES:
        shape, d = c.name.rsplit("-", 1)[0], c.side
        lab, areas, first, _ = islands(c)
        n = len(areas)
        if shape in ("antidiagonal", "diagonal"):
            assert n == 1 and areas[0] == d
            on = np.argwhere(lab > 0)                      # one cell thick: no two cells share an edge, so only diagonal steps join them
            assert not any((abs(a - b).sum() == 1) for a in on for b in on) if d <= 33 else True
            assert all((x + y == d - 1) if shape == "antidiagonal" else (x == y) for y, x in on)
        elif shape.startswith("corner_blobs"):
            assert n == 1 and ndimage.label(lab > 0)[1] == 2                             # 4-connected: two
            if shape.endswith("anti"):
                a = min(d // 2, 3)
                assert lab[a - 1, a] and lab[a, a - 1] and not lab[a - 1, a - 1] and not lab[a, a]
        elif shape in ("serpentine", "last_first"):
            assert n == 1 and ndimage.label(lab > 0)[1] == 1                             # joined through edges alone
            if shape == "last_first":                    # cell 0 touches column 0 only; cells 2 .. d - 2 of row 0 are reached from the far corner
                assert lab[0, 0] and lab[1, 0] and not lab[0, 1] and not lab[1, 1] and lab[0, 2:].all() and not lab[1, 1:d - 1].any()
            else:                                        # one path: every odd row holds one cell
                assert all((lab[y] > 0).sum() == (d if y % 2 == 0 else 1) for y in range(d))
        elif shape == "spirals":
            assert n == 2 and areas[0] == areas[1] and sorted(first) == [0, 2 * d]
        elif shape == "spirals_extra":
            assert n == 2 and sorted(first) == [0, 2 * d] and areas[list(first).index(2 * d)] == areas[list(first).index(0)] + 1
        elif shape == "lattice":
            assert n == ((d + 1) // 2) ** 2 and (areas == 1).all()
            assert not dc.expected(c.make(), c.params)[2].any()                           # Some or None: nothing is returned
        elif shape == "block_lattice":
            assert n == 25 and (areas == 256).all()
        elif shape == "all_on":
            assert n == 1 and areas[0] == d * d and len(c.make()) == d * d               # no still record anywhere
        elif shape == "nothing":
            assert n == 0 and len(c.make()) == d * d
        elif shape in ("one_cell", "side"):
            assert n == 1 and areas[0] == 1
            assert not dc.expected(c.make(), c.params)[2].any()
        elif shape == "k1024_blocks":
            K = (d * d - 1) // 1024
            flat = lab.ravel()                           # the island of a multiple holds cells on both sides of it
            assert n == K and all(flat[1024 * k] and flat[1024 * k - d] == flat[1024 * k] == flat[1024 * k + 1] for k in range(1, K + 1))
            assert len(set(lab.ravel()[[1024 * k for k in range(1, K + 1)]])) == K       # one island per multiple
            if K > 2:
                assert c.seed not in (first.min(), first.max())                          # the winner is neither the first nor the last
        elif shape == "far_edge_lines":
            assert n == 2 and sorted(areas) == [d - 3, d - 2] and (lab[:d - 3, d - 1] > 0).all() and (lab[d - 1, :d - 2] > 0).all()
        else:
            raise AssertionError(shape)
    names = {c.name.rsplit("-", 1)[0] for c in dc.SHAPES}
    assert names == {"antidiagonal", "diagonal", "corner_blobs", "corner_blobs_anti", "serpentine", "last_first", "spirals", "spirals_extra", "lattice",
                     "block_lattice", "all_on", "nothing", "one_cell", "side", "k1024_blocks", "far_edge_lines"}
    assert {True, False} == {c.some for c in dc.SHAPES}
    assert _case("serpentine-160").area == 12880 and _case("side-1").side == 1
    assert {c.side for c in dc.SHAPES if c.name.startswith(("k1024", "far_edge"))} >= {33, 64, 65, 160}


def test_area_equality_is_exact_in_f32():
    assert len(dc.AREA_EQUALITY) == 16
    for m, s, a in dc.AREA_EQUALITY_PAIRS:
        d = oracle.block_dim(m, s)
        assert F(a) / F(d * d) == F(m) and not (F(a - 1) / F(d * d) >= F(m))
        some, none = _case(f"equal-{m}-{s}-some"), _case(f"equal-{m}-{s}-none")
        assert (some.some, some.area, none.some, none.area) == (True, a, False, a - 1)


def test_magnitude_edge_targets_fall_on_opposite_sides():
    for d in dc.BRIDGE_GEOMETRY:
        at, above = _case(f"edge-{d}-at"), _case(f"edge-{d}-above")
        np.testing.assert_array_equal(at.make(), above.make())
        mag = dc.mag_separate(dc.bridge_value(d, at.make()))
        t_at, t_above = F(at.params["target_motion"]), F(above.params["target_motion"])
        assert t_at == mag < t_above == np.nextafter(mag, F(np.inf))
        assert float(t_at) == at.params["target_motion"] and float(t_above) == above.params["target_motion"]   # the f32 value itself is passed
        assert mag >= t_at and not mag >= t_above
        assert at.area > above.area and at.seed != above.seed                          # the split changes the winner
        assert F(dc.TARGET) < mag < dc.mag_separate(F(dc.STRONG))                      # no other cell is near the threshold
    assert len(dc.CONTRACTION) >= 3
    flips = set()
    for c in dc.CONTRACTION:
        v = dc.bridge_value(c.side, c.make())
        sep, (fa, fb) = dc.mag_separate(v), dc.mag_fused(v)
        assert sep != fa and sep != fb and fa == fb, c.name                            # the two evaluations differ, whichever product is fused
        assert abs(int(sep.view(np.uint32)) - int(fa.view(np.uint32))) == 1            # ... by an ulp
        t = F(c.params["target_motion"])
        assert t == max(sep, fa) and float(t) == c.params["target_motion"]
        assert (sep >= t) != (fa >= t)                                                 # a contracted build flips the cell
        flips.add(bool(sep >= t))
    assert flips == {True, False}


def test_special_values_are_special():
    for d in dc.SPECIAL_SIDES:
        wl, hh = dc.BRIDGE_GEOMETRY[d]
        f = islands(_case(f"nan-{d}"))[3]
        lab = islands(_case(f"nan-{d}"))[0]
        for x, y in ((wl, 0), (wl + 2, 1), (0, 1)):      # NaN means (the last one from +inf + -inf): off
            assert np.isnan(f[y, x]).any() and not lab[y, x]
        assert len(islands(_case(f"nan-{d}"))[1]) == 2
        got = dc.expected(_case(f"inf-{d}").make(), _case(f"inf-{d}").params)[2]
        assert got[0, wl, 0] == np.inf and got[1, wl + 2, 1] == -np.inf and got[1, 0, 0] == -np.inf and got[1, 0, 1] == np.inf
        for name in (f"negzero-target0-{d}", f"negzero-negative-target-{d}"):
            c = _case(name)
            got = dc.expected(c.make(), c.params)[2]
            assert c.params["target_motion"] <= 0 and len(c.make()) < d * d              # empty cells are on as well
            for x, y in ((1, 1), (d - 2, d - 2)):
                assert _bits(got[y, x]).tolist() == [0x80000000, 0]
            assert _bits(got[1, 2]).tolist() == [0x80000000, 0x80000000]
            moving = {(x, y) for x, y in dc.all_on(d) if (x + y) % 3 == 0} - {(0, 0), (1, 1), (2, 1), (d - 2, d - 2)}   # (the seed is not copied)
            assert (got[..., 0] != 0).sum() == len(moving) and all(got[y, x, 0] > F(dc.TARGET) for x, y in moving)
        c = _case(f"piles-{d}")
        e = c.make()
        odd = ~(np.isfinite(e[:, :2]).all(1) & (e[:, :2] > 0).all(1) & (e[:, :2] < 1).all(1))
        assert odd.sum() == 16 and np.isnan(e[odd, :2]).any() and np.isinf(e[odd, :2]).any()
        x, y = np_oracle.cell_index(e, d, d)
        assert set(zip(x[odd], y[odd])) == {(0, 0), (d - 1, d - 1)}
        assert not ((x[~odd] == 0) & (y[~odd] == 0)).any() and not ((x[~odd] == d - 1) & (y[~odd] == d - 1)).any()   # lit by those records alone
        lab = islands(c)[0]
        assert lab[0, 0] and lab[d - 1, d - 1] == lab[d - hh, d - wl - 1] != lab[0, 0]


def test_densify_switch_sits_on_both_sides_of_the_thresholds():
    got = {(c.side, len(c.make())) for c in dc.DENSIFY_SWITCH}
    assert got == {(16, 8191), (16, 8192), (16, 8193), (17, 1), (17, 8192)}              # 256 cells | 289; 8,192 records | 8,193
    for c in dc.DENSIFY_SWITCH:
        lab, areas, _, f = islands(c)
        if len(c.make()) > 1:
            assert len(c.make()) // c.side ** 2 >= 28                                    # dozens of records per cell
            on = (lab > 0).mean()
            assert 0.25 < on < 0.75                                                      # the means hover around the threshold
            # ... closely enough for the order of the f32 sums to matter: a mean from f64 sums gives another field
            e = c.make().astype(np.float64)
            x, y = np_oracle.cell_index(c.make(), c.side, c.side)
            s = np.zeros((c.side, c.side, 2)); n = np.zeros((c.side, c.side))
            np.add.at(s, (y, x), e[:, 2:]); np.add.at(n, (y, x), 1)
            assert (_bits((s / n[..., None]).astype(F)) != _bits(f)).any()


def test_batches():
    assert sorted(b.make().shape[0] for b in dc.BATCHES) == [2, 2, 3, 3, 3, 3, 3, 7]
    assert {b.side for b in dc.BATCHES} == {14, 17, 33, 160}
    for b in dc.BATCHES:
        items = b.make()
        assert items.dtype == F and items.ndim == 3 and items.shape[2] == 4
        assert oracle.block_dim(b.params["min_size"], b.params["subdivide"]) == b.side
        res = [dc.expected(np.ascontiguousarray(e), b.params) for e in items]
        if items.shape[1] == 0:
            assert b.name == "batch-17x3-empty" and not any(r[0] for r in res)
            continue
        assert items.shape[1] == (b.side ** 2 if "many" not in b.name else (9000 if b.side == 33 else 3000))
        assert len({r[1] for r in res}) == len(res)                                      # every item another area: a mixed-up item shows
    for name in ("batch-14x3", "batch-17x7", "batch-33x3"):                              # nothing on between two items with motion
        res = [dc.expected(np.ascontiguousarray(e), dc.BATCH_BY_NAME[name].params) for e in dc.BATCH_BY_NAME[name].make()[:3]]
        assert res[0][0] and not res[1][0] and res[2][0]
    assert dc.expected(np.ascontiguousarray(dc.BATCH_BY_NAME["batch-17x7"].make()[3]), dc.BATCH_BY_NAME["batch-17x7"].params)[1] == 17 * 17
    assert dc.expected(np.ascontiguousarray(dc.BATCH_BY_NAME["batch-160x2"].make()[1]), dc.BATCH_BY_NAME["batch-160x2"].params)[1] == 160 * 160
