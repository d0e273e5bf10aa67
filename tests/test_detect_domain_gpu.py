"""-m gpu: the block-motion detector (ofps_amd/csrc/detect.hip, fed by densify.hip) over its whole grid and parameter domain, on the cases
of tests/detect_cases.py against the CPU oracle: outcome, area, membership, the field's bits and the returned side.  Every output is an
integer or a copied float, so every comparison is bit equality.  tests/test_detect_cases_cpu.py proves on the CPU that each case has the
property it is named for and that both oracles agree on it."""
import json
import os
import subprocess
import sys

import ctypes as C
import numpy as np
import pytest

import detect_cases as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
GUARD = 64


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _detect_raw(ctx, e, prm):
    """ofps_hip_detect itself -> (has, area, dim, field): also what it writes when the answer is None, and the side it reports"""
    e = np.ascontiguousarray(e, np.float32).reshape(-1, 4)
    d = ctx.block_dim(prm["min_size"], prm["subdivide"])
    field = np.full((d, d, 2), 7.0, np.float32)          # every cell must be written
    has, area, dim = C.c_int(-1), C.c_size_t(12345), C.c_int(-1)
    ctx._check(ctx._lib.ofps_hip_detect(ctx._h, e.ctypes.data_as(C.POINTER(C.c_float)), e.shape[0], prm["min_size"], prm["subdivide"],
                                        prm["target_motion"], C.byref(has), C.byref(area), C.byref(dim), field.ctypes.data_as(C.POINTER(C.c_float))))
    return has.value, int(area.value), dim.value, field


def _check(ctx, e, prm, side, what):
    has_o, area_o, field_o = dc.expected(e, prm)
    has, area, dim, field = _detect_raw(ctx, e, prm)
    assert dim == side == ctx.block_dim(prm["min_size"], prm["subdivide"]), what
    assert has == int(has_o), what                                                        # has-motion
    assert area == area_o, what                                                           # area: exact
    np.testing.assert_array_equal((field != 0).any(-1), (field_o != 0).any(-1), err_msg=what + ": membership")
    np.testing.assert_array_equal(_bits(field), _bits(field_o), err_msg=what + ": field bits")
    r = ctx.detect(e, **prm)                                                              # the wrapper every plugin goes through
    assert (r is not None) == has_o, what
    if r is not None:
        assert r[0] == area_o and r[1].shape == (side, side, 2), what
        np.testing.assert_array_equal(_bits(r[1]), _bits(field_o), err_msg=what + ": ctx.detect")


def _check_case(ctx, c):
    has_o, area_o, field_o = dc.expected(c.make(), c.params)
    assert has_o == c.some and area_o == (c.area if c.some else 0)                        # the literals (pinned on the CPU)
    _check(ctx, c.make(), c.params, c.side, c.name)


@pytest.mark.parametrize("case", dc.SHAPES, ids=lambda c: c.name)
def test_shapes(ctx, case):
    _check_case(ctx, case)


@pytest.mark.parametrize("case", dc.AREA_EQUALITY, ids=lambda c: c.name)
def test_area_over_cells_equal_to_min_size(ctx, case):
    _check_case(ctx, case)


@pytest.mark.parametrize("case", dc.MAGNITUDE_EDGE, ids=lambda c: c.name)
def test_magnitude_equal_to_target_motion(ctx, case):
    """the contract-* cases flip under a build that fuses x * x + y * y (ofps_amd/build.py: -ffp-contract=off)"""
    _check_case(ctx, case)


@pytest.mark.parametrize("case", dc.SPECIAL_VALUES, ids=lambda c: c.name)
def test_special_values(ctx, case):
    _check_case(ctx, case)


@pytest.mark.parametrize("case", dc.DENSIFY_SWITCH, ids=lambda c: c.name)
def test_densify_switch(ctx, case):
    _check_case(ctx, case)


SMALL_SIDES = tuple(c for c in dc.ALL_CASES if c.side <= 16)


def test_small_grids_through_the_general_densifier(ctx):
    """OFPS_HIP_DENSIFY_NO_SMALL sends the grids of at most 256 cells through the six-kernel path (one sort pass) as well"""
    ctx.set_option("OFPS_HIP_DENSIFY_NO_SMALL", 1)
    try:
        for c in SMALL_SIDES:
            _check_case(ctx, c)
    finally:
        ctx.set_option("OFPS_HIP_DENSIFY_NO_SMALL", None)


# --------------------------------------------------------------------------------------------------------------- ofps_hip_detect_dev, batched
def _detect_dev(ctx, items, prm, side, torch_stream):
    """-> (out_result [batch, 4] i32, out_field [batch, side, side, 2] f32); 64 guard words behind each output"""
    import torch
    batch, n = items.shape[:2]
    cells = side * side
    d_ent = torch.from_numpy(np.ascontiguousarray(items).reshape(-1)).cuda() if n else torch.zeros(GUARD, dtype=torch.float32, device="cuda")
    d_res = torch.full((4 * batch + GUARD,), -7, dtype=torch.int32, device="cuda")
    d_fld = torch.full((2 * cells * batch + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if torch_stream:
        ctx.use_torch_stream()
    try:
        ctx.detect_dev(d_ent.data_ptr(), n, batch, prm["min_size"], prm["subdivide"], prm["target_motion"], d_res.data_ptr(), d_fld.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
    finally:
        if torch_stream:
            ctx.use_own_stream()
    res, fld = d_res.cpu().numpy(), d_fld.cpu().numpy()
    assert (res[4 * batch:] == -7).all() and (fld[2 * cells * batch:] == -7.0).all(), "guard words"
    return res[:4 * batch].reshape(batch, 4), fld[:2 * cells * batch].reshape(batch, side, side, 2)


def _check_batch(ctx, b, torch_stream):
    items = b.make()
    res, fld = _detect_dev(ctx, items, b.params, b.side, torch_stream)
    for i in range(items.shape[0]):
        e = np.ascontiguousarray(items[i])
        what = f"{b.name} item {i}{' torch stream' if torch_stream else ''}"
        has_o, area_o, field_o = dc.expected(e, b.params)
        assert res[i].tolist() == [int(has_o), area_o, b.side, 0], what
        np.testing.assert_array_equal(_bits(fld[i]), _bits(field_o), err_msg=what + ": field against the oracle")
        alone = ctx.detect(e, **b.params)                                                 # ... and the item alone
        assert (alone is not None) == bool(res[i, 0]), what
        if alone is None:
            assert not _bits(fld[i]).any(), what
        else:
            assert alone[0] == res[i, 1], what
            np.testing.assert_array_equal(_bits(fld[i]), _bits(alone[1]), err_msg=what + ": field against ctx.detect of the item alone")


@pytest.mark.parametrize("torch_stream", (False, True), ids=["own-stream", "torch-stream"])
@pytest.mark.parametrize("b", dc.BATCHES, ids=lambda b: b.name)
def test_detect_dev_batches(ctx, b, torch_stream):
    _check_batch(ctx, b, torch_stream)


# ------------------------------------------------------------------------------------------------------------------- one context, in a row
def test_nothing_is_left_over_from_the_previous_call():
    """scratch buffers are re-used from call to call: a large grid, a tiny one, a large one, a batch, one cell, then the two grids on either
    side of the 48 KiB of dynamic LDS -- each against the oracle, on one fresh context"""
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    try:
        for step in ("all_on-160", "nothing-3", "serpentine-160", "batch-17x7", "side-1", "serpentine-91", "serpentine-90", "nothing-160", "all_on-2"):
            if step in dc.BATCH_BY_NAME:
                _check_batch(c, dc.BATCH_BY_NAME[step], False)
            else:
                _check_case(c, dc.BY_NAME[step])
    finally:
        c.close()


def test_first_grid_above_48_kib_of_lds_in_a_fresh_process():
    """the LDS limit, once raised by a large grid, stays raised for the process: only a process whose FIRST grid is 91 x 91 shows that the
    limit is raised there (tests/detect_fresh_process_child.py).  Where the runtime admits any LDS size without the attribute (ROCm 7.2 on
    gfx950 does: docs/history/29) this is no more than the cases themselves in a process of their own."""
    names = ["serpentine-91", "serpentine-90", "all_on-91", "serpentine-160"]
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "detect_fresh_process_child.py")] + names, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = [json.loads(line) for line in p.stdout.strip().splitlines() if line.startswith("{")]
    assert [o["name"] for o in out] == names
    for o in out:
        c = dc.BY_NAME[o["name"]]
        has_o, area_o, field_o = dc.expected(c.make(), c.params)
        assert (o["has"], o["area"], o["side"]) == (has_o, area_o, c.side), o["name"]
        np.testing.assert_array_equal(np.array(o["field"], np.uint32), _bits(field_o).reshape(-1), err_msg=o["name"])


# ---------------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(ctx):
    import torch
    from ofps_amd.runtime import OfpsHipError
    good = dc.BY_NAME["edge-17-above"]
    e = good.make()

    def refused(call, word):
        with pytest.raises(OfpsHipError) as ei:
            call()
        assert ei.value.code == EINVAL
        text = ctx._lib.ofps_hip_last_error(ctx._h).decode()
        assert word in text and text in str(ei.value), text                               # an error text, and the one the exception carries
        _check_case(ctx, good)                                                            # the next valid call answers correctly

    assert ctx.block_dim(*dc.SIDE_161) == 161
    refused(lambda: ctx.detect(e, dc.SIDE_161[0], dc.SIDE_161[1], dc.TARGET), "161")
    refused(lambda: ctx.detect(e, 0.05, 0, dc.TARGET), "block_dim 0")
    refused(lambda: ctx.detect(e, float("nan"), 3, dc.TARGET), "block_dim 0")
    refused(lambda: ctx.detect(e, -0.05, 3, dc.TARGET), "block_dim 0")
    d_ent = torch.from_numpy(e).cuda()
    d_res = torch.full((4 + GUARD,), -7, dtype=torch.int32, device="cuda")
    d_fld = torch.full((2 * 161 * 161 + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    args = (d_res.data_ptr(), d_fld.data_ptr())
    refused(lambda: ctx.detect_dev(d_ent.data_ptr(), len(e), 0, good.params["min_size"], good.params["subdivide"], dc.TARGET, *args), "batch")
    refused(lambda: ctx.detect_dev(d_ent.data_ptr(), len(e), -1, good.params["min_size"], good.params["subdivide"], dc.TARGET, *args), "batch")
    refused(lambda: ctx.detect_dev(d_ent.data_ptr(), len(e), 1, dc.SIDE_161[0], dc.SIDE_161[1], dc.TARGET, *args), "161")
    refused(lambda: ctx.detect_dev(d_ent.data_ptr(), len(e), 1, 0.05, 0, dc.TARGET, *args), "block_dim 0")
    ctx.sync()
    assert (d_res.cpu().numpy() == -7).all() and (d_fld.cpu().numpy() == -7.0).all()      # refused before anything was enqueued
