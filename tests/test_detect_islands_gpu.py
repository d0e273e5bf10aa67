"""-m gpu: the island list of the block-motion detector (include/ofps_hip.h A5i; ofps_amd/csrc/detect.hip) through the C ABI, on the cases
of tests/detect_islands_cases.py against the plain-Python restatement tests/indep_detect_islands.py (proved on the CPU by
tests/test_detect_islands_cpu.py).  Counts, table rows below n_listed, labels and the field's bits: everything is compared exactly."""
import ctypes as C

import numpy as np
import pytest

import detect_cases as dc
import detect_islands_cases as ic
import indep_detect_islands as indep

pytestmark = pytest.mark.gpu
EINVAL = -1
GUARD = 64
I32P = C.POINTER(C.c_int32)
F32P = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _islands_raw(ctx, e, prm, K, want_labels=True, want_field=True):
    """ofps_hip_detect_islands itself, guard words behind every output -> (counts [4], table [K, 8], labels [d, d] | None, field | None)"""
    e = np.ascontiguousarray(e, np.float32).reshape(-1, 4)
    d = ctx.block_dim(prm["min_size"], prm["subdivide"])
    counts = np.full(4 + GUARD, -7, np.int32)
    table = np.full(8 * K + GUARD, -7, np.int32)
    labels = np.full(d * d + GUARD, 0x7777, np.uint16)
    field = np.full(2 * d * d + GUARD, 7.0, np.float32)
    ctx._check(ctx._lib.ofps_hip_detect_islands(ctx._h, e.ctypes.data_as(F32P), e.shape[0], prm["min_size"], prm["subdivide"], prm["target_motion"], K,
                                                counts.ctypes.data_as(I32P), table.ctypes.data_as(I32P),
                                                C.c_void_p(labels.ctypes.data) if want_labels else None,
                                                field.ctypes.data_as(F32P) if want_field else None))
    assert (counts[4:] == -7).all() and (table[8 * K:] == -7).all() and (labels[d * d:] == 0x7777).all() and (field[2 * d * d:] == 7.0).all(), "guard words"
    if not want_labels:
        assert (labels == 0x7777).all()
    if not want_field:
        assert (field == 7.0).all()
    return (counts[:4].copy(), table[:8 * K].reshape(K, 8), labels[:d * d].reshape(d, d) if want_labels else None,
            field[:2 * d * d].reshape(d, d, 2) if want_field else None)


def _same(got, want, what):
    counts, table, labels, field = got
    w_counts, w_table, w_labels, w_field = want
    assert counts.tolist() == w_counts.tolist(), what
    n = int(w_counts[3])
    np.testing.assert_array_equal(table[:n], w_table[:n], err_msg=what + ": table")
    if labels is not None:
        np.testing.assert_array_equal(labels, w_labels, err_msg=what + ": labels")
    if field is not None:
        np.testing.assert_array_equal(_bits(field), _bits(w_field), err_msg=what + ": field bits")


def _detect_raw(ctx, e, prm):
    e = np.ascontiguousarray(e, np.float32).reshape(-1, 4)
    d = ctx.block_dim(prm["min_size"], prm["subdivide"])
    field = np.full((d, d, 2), 7.0, np.float32)
    has, area, dim = C.c_int(-1), C.c_size_t(12345), C.c_int(-1)
    ctx._check(ctx._lib.ofps_hip_detect(ctx._h, e.ctypes.data_as(F32P), e.shape[0], prm["min_size"], prm["subdivide"], prm["target_motion"],
                                        C.byref(has), C.byref(area), C.byref(dim), field.ctypes.data_as(F32P)))
    return has.value, int(area.value), dim.value, field


def _check_k1_against_the_detector(ctx, e, prm, what):
    counts, table, labels, field = _islands_raw(ctx, e, prm, 1)
    has, area, dim, dfield = _detect_raw(ctx, e, prm)
    assert has == int(counts[0] >= 1) and dim == counts[2], what
    if has:
        assert area == table[0, 1], what
    np.testing.assert_array_equal(_bits(field), _bits(dfield), err_msg=what + ": the K = 1 field against ofps_hip_detect's")


def _check_case(ctx, c, full_k):
    e, prm = c.make(), c.params
    assert ctx.block_dim(prm["min_size"], prm["subdivide"]) == c.side, c.name
    ref = ic.reference(e, prm)
    if c.n_islands is not None:
        assert (ref.n_islands, ref.n_components) == (c.n_islands, c.n_components), c.name
    for K in (ic.k_values(ref.n_islands) if full_k else (1, 16)):
        _same(_islands_raw(ctx, e, prm, K), indep.listed(ref, K), f"{c.name} K={K}")
    _check_k1_against_the_detector(ctx, e, prm, c.name)


@pytest.mark.parametrize("case", ic.CASES, ids=lambda c: c.name)
def test_shapes(ctx, case):
    _check_case(ctx, case, full_k=True)


@pytest.mark.parametrize("case", ic.AREA_EQUALITY, ids=lambda c: c.name)
def test_one_island_at_the_bound_beside_one_a_cell_smaller(ctx, case):
    _check_case(ctx, case, full_k=True)


@pytest.mark.parametrize("case", ic.MAGNITUDE_EDGE, ids=lambda c: c.name)
def test_cells_at_the_threshold(ctx, case):
    _check_case(ctx, case, full_k=True)


def test_k1_equals_the_detector_on_every_detector_case(ctx):
    for c in dc.ALL_CASES:
        _check_k1_against_the_detector(ctx, c.make(), c.params, c.name)


def test_wrapper_and_null_outputs(ctx):
    c = ic.BY_NAME["k1024_blocks-64-a2"]
    e, prm = c.make(), c.params
    ref = ic.reference(e, prm)
    want = indep.listed(ref, 2)
    for labels, field in ((False, True), (True, False), (False, False)):
        _same(_islands_raw(ctx, e, prm, 2, want_labels=labels, want_field=field), want, f"labels={labels} field={field}")
    r = ctx.detect_islands(e, max_islands=2, **prm)
    assert (r["n_islands"], r["n_components"], r["dim"], r["n_listed"]) == tuple(want[0].tolist()) and r["table"].shape == (2, 8)
    _same((want[0], r["table"], r["labels"], r["field"]), want, "ctx.detect_islands")
    cen = ctx.island_centroids(r["table"], r["dim"])
    np.testing.assert_allclose(cen, (r["table"][:, 6:8] / r["table"][:, 1:2] + 0.5) / 64)


# ------------------------------------------------------------------------------------------------------- ofps_hip_detect_islands_dev, batched
@pytest.mark.parametrize("K", (1, 3, 6400))
@pytest.mark.parametrize("b", [dc.BATCH_BY_NAME[n] for n in ("batch-14x3", "batch-17x7", "batch-33x3", "batch-160x2", "batch-17x3-empty")], ids=lambda b: b.name)
def test_detect_islands_dev_batches(ctx, b, K):
    import torch
    items = b.make()
    batch, n = items.shape[:2]
    d, cells = b.side, b.side * b.side
    prm = b.params
    d_ent = torch.from_numpy(np.ascontiguousarray(items).reshape(-1)).cuda() if n else torch.zeros(GUARD, dtype=torch.float32, device="cuda")
    d_cnt = torch.full((4 * batch + GUARD,), -7, dtype=torch.int32, device="cuda")
    d_tab = torch.full((8 * K * batch + GUARD,), -7, dtype=torch.int32, device="cuda")
    d_lab = torch.full((cells * batch + GUARD,), 0x7777, dtype=torch.int16, device="cuda")
    d_fld = torch.full((2 * cells * batch + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.detect_islands_dev(d_ent.data_ptr(), n, batch, prm["min_size"], prm["subdivide"], prm["target_motion"], K, d_cnt.data_ptr(), d_tab.data_ptr(),
                           d_lab.data_ptr(), d_fld.data_ptr())
    ctx.sync()
    cnt, tab, lab, fld = d_cnt.cpu().numpy(), d_tab.cpu().numpy(), d_lab.cpu().numpy().view(np.uint16), d_fld.cpu().numpy()
    assert (cnt[4 * batch:] == -7).all() and (tab[8 * K * batch:] == -7).all() and (lab[cells * batch:] == 0x7777).all() and \
        (fld[2 * cells * batch:] == -7.0).all(), "guard words"
    for j in range(batch):
        e = np.ascontiguousarray(items[j])
        got = (cnt[4 * j:4 * j + 4], tab[8 * K * j:8 * K * (j + 1)].reshape(K, 8), lab[cells * j:cells * (j + 1)].reshape(d, d),
               fld[2 * cells * j:2 * cells * (j + 1)].reshape(d, d, 2))
        _same(got, indep.listed(ic.reference(e, prm), K), f"{b.name} item {j} K={K}: against the restatement")
        _same(got, _islands_raw(ctx, e, prm, K), f"{b.name} item {j} K={K}: against the item alone")
    # labels and field are optional in the device form as well
    d_cnt2 = torch.full_like(d_cnt, -7)
    d_tab2 = torch.full_like(d_tab, -7)
    torch.cuda.synchronize()
    ctx.detect_islands_dev(d_ent.data_ptr(), n, batch, prm["min_size"], prm["subdivide"], prm["target_motion"], K, d_cnt2.data_ptr(), d_tab2.data_ptr())
    ctx.sync()
    np.testing.assert_array_equal(d_cnt2.cpu().numpy(), cnt)
    for j in range(batch):
        nl = cnt[4 * j + 3]
        np.testing.assert_array_equal(d_tab2.cpu().numpy()[8 * K * j:8 * K * j + 8 * nl], tab[8 * K * j:8 * K * j + 8 * nl])


# ------------------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    from ofps_amd.runtime import OfpsHipError
    c = ic.BY_NAME["dominoes-17-a2"]
    e, prm = c.make(), c.params

    def refused(call, word):
        with pytest.raises(OfpsHipError) as ei:
            call()
        assert ei.value.code == EINVAL and word in str(ei.value), str(ei.value)

    refused(lambda: _islands_raw(ctx, e, prm, 0), "max_islands")
    refused(lambda: ctx.detect_islands(e, max_islands=6401, **prm), "max_islands")
    refused(lambda: ctx.detect_islands(e, dc.SIDE_161[0], dc.SIDE_161[1], dc.TARGET, max_islands=4), "161")
    refused(lambda: ctx.set_detect_islands(-1), "set_detect_islands")
    refused(lambda: ctx.set_detect_islands(6401), "set_detect_islands")
    assert ctx.get_detect_islands() == 0
    ctx.set_option("OFPS_HIP_DETECT_ISLANDS", 5)                             # the option table sets the same field
    assert ctx.get_detect_islands() == 5
    with pytest.raises(OfpsHipError):
        ctx.set_option("OFPS_HIP_DETECT_ISLANDS", 6401)
    ctx.set_option("OFPS_HIP_DETECT_ISLANDS", None)
    assert ctx.get_detect_islands() == 0
    _check_case(ctx, c, full_k=False)                                       # the context still answers
    # a ticket pushed with K = 0 has no islands
    ctx.reset_frames()
    f = ic.frames()
    for k in range(2):
        r = ctx.push_frame(f[k], **ic.FUSED)
        assert "islands" not in r
    refused(lambda: ctx.frame_islands(0), "max_islands 0")


# ------------------------------------------------------------------------------------------------------------------------ the fused forms
NBLK = (ic.FW // ic.BLOCK) * (ic.FH // ic.BLOCK)
DET = {k: ic.FUSED[k] for k in ("min_size", "subdivide", "target_motion")}


def _same_islands(ctx, isl, entries, K, what, field=None):
    """a ticket's islands against ofps_hip_detect_islands on the ticket's records"""
    want = _islands_raw(ctx, entries, DET, K)
    _same((np.array([isl["n_islands"], isl["n_components"], isl["dim"], isl["n_listed"]], np.int32), isl["table"], isl["labels"], None), want, what)
    if field is not None:                                                   # the fused out_field stays the largest island's: the K = 1 field
        np.testing.assert_array_equal(_bits(field), _bits(_islands_raw(ctx, entries, DET, 1)[3]), err_msg=what + ": out_field")
    return want


def _sync_pushes(ctx, n, K, **kw):
    ctx.reset_frames()
    ctx.set_detect_islands(K)
    try:
        return [ctx.push_frame(ic.frames()[k], want_entries=True, want_field=True, **ic.FUSED, **kw) for k in range(n)]
    finally:
        ctx.set_detect_islands(0)


def test_push_frame_sync_and_async(ctx):
    K = 16
    out = _sync_pushes(ctx, 4, K)
    assert not out[0]["have_vectors"] and out[0]["islands"]["n_islands"] == 0 and out[0]["islands"]["n_components"] == 0
    assert out[0]["islands"]["dim"] == 15 and out[0]["islands"]["n_listed"] == 0 and (out[0]["islands"]["labels"] == 0xFFFF).all()
    for k in range(1, 4):
        r = out[k]
        assert r["have_vectors"] and r["n_vectors"] == NBLK
        want = _same_islands(ctx, r["islands"], r["entries"], K, f"push_frame {k}", field=r["motion"][1] if r["motion"] else np.zeros((15, 15, 2), np.float32))
        assert r["motion"] is not None and r["motion"][0] == r["islands"]["table"][0, 1]
        assert want[0][0] >= 2, "both planted rectangles are islands"
    # the same stream with two tickets in flight
    ctx.reset_frames()
    ctx.set_detect_islands(K)
    try:
        pins = [ctx.pinned_frame(ic.FH, ic.FW) for _ in range(3)]
        ents = [ctx.pinned_array((NBLK, 4)) for _ in range(2)]
        flds = [ctx.pinned_array((15, 15, 2)) for _ in range(2)]
        tickets = []

        def collect(k):
            r = ctx.frame_wait(tickets[k])
            if k == 0:
                assert r["islands"]["n_components"] == 0
                return
            _same_islands(ctx, r["islands"], ents[k % 2].copy(), K, f"async {k}", field=flds[k % 2].copy())
            np.testing.assert_array_equal(r["islands"]["table"], out[k]["islands"]["table"])
            np.testing.assert_array_equal(r["islands"]["labels"], out[k]["islands"]["labels"])
            assert r["motion"][0] == r["islands"]["table"][0, 1]

        for k in range(4):
            if k >= 2:
                collect(k - 2)
            np.copyto(pins[k % 3], ic.frames()[k])
            tickets.append(ctx.push_frame_async(pins[k % 3], out_entries=ents[k % 2], out_field=flds[k % 2], **ic.FUSED))
        collect(2)
        collect(3)
        for p in pins + ents + flds:
            ctx.free_pinned(p)
    finally:
        ctx.set_detect_islands(0)


def test_frame_islands_capacity_and_item(ctx):
    from ofps_amd import _lib
    out = _sync_pushes(ctx, 2, 16)
    n = out[1]["islands"]["n_listed"]
    assert n >= 2
    counts = np.zeros(4, np.int32)
    table = np.full(8 * n + GUARD, -7, np.int32)
    lib = _lib.load()
    assert lib.ofps_hip_frame_islands(ctx._h, 0, counts.ctypes.data_as(I32P), table.ctypes.data_as(I32P), n - 1, None) == EINVAL
    assert lib.ofps_hip_frame_islands(ctx._h, 1, counts.ctypes.data_as(I32P), table.ctypes.data_as(I32P), n, None) == EINVAL
    assert lib.ofps_hip_frame_islands(ctx._h, -1, counts.ctypes.data_as(I32P), table.ctypes.data_as(I32P), n, None) == EINVAL
    assert (table == -7).all()
    assert lib.ofps_hip_frame_islands(ctx._h, 0, counts.ctypes.data_as(I32P), table.ctypes.data_as(I32P), n, None) == 0
    np.testing.assert_array_equal(table[:8 * n].reshape(n, 8), out[1]["islands"]["table"])
    assert (table[8 * n:] == -7).all()


def _batched(ctx, K, n=3):
    ctx.reset_frames()
    ctx.set_detect_islands(K)
    try:
        buf = ctx.pinned_array((n, ic.FH, ic.FW), np.uint8)
        ent = ctx.pinned_array((n, NBLK, 4))
        np.copyto(buf, ic.frames()[:n])
        res = ctx.frames_wait(ctx.push_frames_async(buf, out_entries=ent, **ic.FUSED))
        e = ent.copy()
        ctx.free_pinned(buf)
        ctx.free_pinned(ent)
        return res, e
    finally:
        ctx.set_detect_islands(0)


def test_push_frames_async_items_equal_the_single_pushes(ctx):
    K = 16
    single = _sync_pushes(ctx, 3, K)
    res, ent = _batched(ctx, K)
    assert not res[0]["have_vectors"] and res[0]["islands"]["n_components"] == 0 and res[0]["islands"]["dim"] == 15
    for j in (1, 2):
        _same_islands(ctx, res[j]["islands"], ent[j], K, f"batched item {j}")
        for key in ("n_islands", "n_components", "dim", "n_listed"):
            assert res[j]["islands"][key] == single[j]["islands"][key]
        np.testing.assert_array_equal(res[j]["islands"]["table"], single[j]["islands"]["table"])
        np.testing.assert_array_equal(res[j]["islands"]["labels"], single[j]["islands"]["labels"])
        assert res[j]["motion"][0] == res[j]["islands"]["table"][0, 1]


def test_filtered_ticket_lists_the_kept_records_islands(ctx):
    K = 16
    ctx.set_sad_batch_filter(1)
    ctx.set_sad_gate(1)
    try:
        res, ent = _batched(ctx, K)
        single = _sync_pushes(ctx, 3, K)
    finally:
        ctx.set_sad_gate(0)
        ctx.set_sad_batch_filter(0)
    for j in (1, 2):
        n = res[j]["n_vectors"]
        print(f"filtered item {j}: kept {n} of {NBLK}")
        assert 0 < n < NBLK, "the gate drops the flat band's blocks"
        _same_islands(ctx, res[j]["islands"], ent[j][:n], K, f"filtered batched item {j}")
        assert single[j]["n_vectors"] == n
        _same_islands(ctx, single[j]["islands"], single[j]["entries"], K, f"filtered push_frame {j}")


def test_lk_push_frame_fused_hip_flow_reduced(ctx):
    import dense_fused_cases as fc
    import oracle
    K = 8
    kw = dict(levels=fc.FB[0], radius=fc.FB[1], iters=fc.FB[2], max_w=150, max_h=150, contrast_mask=True, reduced=True, farneback=True, fmt=oracle.FMT_BGR)
    det = fc.DETECTOR
    ctx.lk_reset()
    ctx.set_detect_islands(K)
    try:
        out = [ctx.lk_push_frame_fused(fc.bgr_of(fc.frame(k)), estimator=False, **kw, **det) for k in ("move0", "move1")]
    finally:
        ctx.set_detect_islands(0)
        ctx.lk_reset()
    assert not out[0]["have_vectors"] and out[0]["islands"]["n_components"] == 0
    r = out[1]
    assert r["have_vectors"] and r["n_vectors"] > 0
    want = _islands_raw(ctx, r["entries"], det, K)
    isl = r["islands"]
    _same((np.array([isl["n_islands"], isl["n_components"], isl["dim"], isl["n_listed"]], np.int32), isl["table"], isl["labels"], None), want, "hip_flow fused")
    assert r["motion"] is not None and r["motion"][0] == isl["table"][0, 1]
    np.testing.assert_array_equal(_bits(r["motion"][1]), _bits(_islands_raw(ctx, r["entries"], det, 1)[3]))


def test_compensation_mode_1_is_self_consistent(ctx):
    """the quaternion's 2e-6 bound makes a comparison against host-compensated records inexact at the threshold: only what is exact"""
    ctx.set_detect_compensation(1)
    try:
        out = _sync_pushes(ctx, 3, 16, estimator=True)
    finally:
        ctx.set_detect_compensation(0)
    for k in (1, 2):
        r = out[k]
        isl = r["islands"]
        assert (r["motion"] is not None) == (isl["n_islands"] >= 1)
        fld = np.zeros((15, 15, 2), np.float32)
        if r["motion"] is not None:
            assert r["motion"][0] == isl["table"][0, 1]
            fld = r["motion"][1]
        # the K = 1 field = out_field: island 0's cells but its seed carry the field, nothing else does
        member = (isl["labels"] == 0) & (np.arange(225).reshape(15, 15) != (isl["table"][0, 0] if isl["n_listed"] else -1))
        assert not _bits(fld)[~member].any()
        assert (isl["labels"] == 0).sum() == (isl["table"][0, 1] if isl["n_listed"] else 0)


def test_k16_k0_k16_on_one_context(ctx):
    ctx.reset_frames()
    f = ic.frames()
    ctx.push_frame(f[0], **ic.FUSED)
    got = []
    try:
        for k, K in ((1, 16), (2, 0), (3, 16)):
            ctx.set_detect_islands(K)
            got.append(ctx.push_frame(f[k], want_entries=True, **ic.FUSED))
            if K == 0:
                from ofps_amd.runtime import OfpsHipError
                with pytest.raises(OfpsHipError):
                    ctx.frame_islands(0)
    finally:
        ctx.set_detect_islands(0)
    ref = _sync_pushes(ctx, 4, 16)
    assert "islands" not in got[1]
    for g, k in ((got[0], 1), (got[2], 3)):
        np.testing.assert_array_equal(g["islands"]["table"], ref[k]["islands"]["table"])
        np.testing.assert_array_equal(g["islands"]["labels"], ref[k]["islands"]["labels"])
    # the middle ticket answers what a context without the extension answers
    np.testing.assert_array_equal(_bits(got[1]["entries"]), _bits(ref[2]["entries"]))
    assert got[1]["motion"][0] == ref[2]["motion"][0]
