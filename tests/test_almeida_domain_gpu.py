"""-m gpu: hip_almeida (ofps_amd/csrc/almeida.hip) over its record-count, batch and RANSAC parameter domain, on the cases of
tests/almeida_domain_cases.py against the CPU oracle.  Every least-squares input carries a sentinel record whose loss or double count
moves the oracle's answer by >= 100 x the 2e-6 parity bound (tests/test_almeida_domain_cpu.py proves it, and that the summation order
moves it by a tenth of the bound at most), so a kernel that drops its last record, reads one past the end or folds a partial sum twice
fails here.  The RANSAC cases pin WHICH hypothesis wins and WHICH records are refitted, in which order."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import almeida_domain_cases as dc
import oracle
from ofps_amd import synth

pytestmark = pytest.mark.gpu
EINVAL = -1
GUARD = 64
PATTERN = 0x7FC0BEEF                        # a NaN with a payload: neither a quaternion nor anything a kernel computes
IDENT = np.array([1, 0, 0, 0], np.float32)


@pytest.fixture(scope="module")
def ctx():
    from ofps_amd.runtime import HipContext
    c = HipContext(0)
    yield c
    c.close()


@contextlib.contextmanager
def _options(ctx, opts):
    try:
        for k, v in opts.items(): ctx.set_option(k, v)
        yield
    finally:
        for k in ("OFPS_HIP_ALMEIDA_PATH", "OFPS_HIP_ALMEIDA_BLOCK", "OFPS_HIP_ALMEIDA_EPT"): ctx.set_option(k, None)


@contextlib.contextmanager
def _stream(ctx, which):
    """which = "own": the context's stream, waited for through the context; "torch": torch's current stream"""
    import torch
    if which == "torch": ctx.use_torch_stream()
    try:
        yield
        if which == "torch": torch.cuda.synchronize()
        else: ctx.sync()
    finally:
        if which == "torch": ctx.use_own_stream()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _close(q, q_o, bound, what):
    assert np.isfinite(q).all(), what
    d = float(np.abs(np.asarray(q, np.float64) - np.asarray(q_o, np.float64)).max())
    assert d <= bound, (what, d, q, q_o)


def _out(slots):
    """slots quaternions + GUARD words of device memory, all PATTERN"""
    import torch
    return torch.full((slots * 4 + GUARD,), PATTERN, dtype=torch.int32, device="cuda")


def _read(out, batch, what=""):
    """the first batch quaternions; everything behind them -- later slots, guard words -- must be untouched"""
    a = out.cpu().numpy()
    assert (a[batch * 4:] == PATTERN).all(), what + ": written behind the batch's quaternions"
    return a[:batch * 4].view(np.float32).reshape(batch, 4).copy()


def _dev(ctx, items, batch_slots=None, which="own", ransac=False, iters=0, deg=0.05, ns=0, seed=0):
    """ofps_hip_almeida_dev on a stack of items [batch, n, 4] -> [batch, 4]; the output buffer has two slots more than the batch"""
    import torch
    items = np.array(items, np.float32, copy=True, order="C")
    batch, n = items.shape[0], items.shape[1]
    d = torch.from_numpy(items).cuda()
    out = _out(batch + 2 if batch_slots is None else batch_slots)
    torch.cuda.synchronize()
    with _stream(ctx, which):
        ctx.almeida_dev(d.data_ptr(), n, batch, dc.ASPECT, dc.FOV, ransac, iters, deg, ns, seed, out.data_ptr())
    return _read(out, batch)


# ---- least squares: record counts and paths --------------------------------------------------------------------------------------------
def _lsq_runs(case):
    e = dc.field(case.n)
    if not case.idx: return [(None, e, dc.solve(e))]
    return [(idx, dc.sentinel(e, idx, case.mag), dc.lsq_expected(case, idx)) for idx in case.idx]


@pytest.mark.parametrize("case", dc.LSQ_COUNTS, ids=lambda c: c.name)
def test_lsq_counts(ctx, case):
    rec0 = ctx.almeida_recoveries()
    with _options(ctx, dc.options(case)):
        for idx, s, q_o in _lsq_runs(case):
            q, tr = ctx.almeida(s, dc.ASPECT, dc.FOV, use_ransac=False)
            _close(q, q_o, dc.BOUND, (case.name, idx))
            assert not tr.any()
    assert ctx.almeida_recoveries() == rec0                  # every workgroup of a cluster launch was there


def test_lsq_counts_on_torch_stream(ctx):
    """the whole table once more through the device form on torch's stream, the first sentinel of every case"""
    rec0 = ctx.almeida_recoveries()
    for case in dc.LSQ_COUNTS:
        idx, s, q_o = _lsq_runs(case)[0]
        with _options(ctx, dc.options(case)):
            q = _dev(ctx, s[None], which="torch")
        _close(q[0], q_o, dc.BOUND, (case.name, idx))
    assert ctx.almeida_recoveries() == rec0


def test_lsq_paths_agree(ctx):
    """the same records through the path the library picks and through every forced one: within the bound of each other"""
    by_n = {}
    for c in dc.LSQ_COUNTS: by_n.setdefault(c.n, []).append(c)
    groups = {n: cs for n, cs in by_n.items() if len(cs) > 1}
    assert set(groups) >= {3, 1023, 1025, 2047, 2049, 4095, 4097, 65536, 65537}
    for n, cs in groups.items():
        assert len({c.path for c in cs}) > 1 and len({(c.mag, c.idx[0], c.idx[1]) for c in cs}) == 1
        for idx in cs[0].idx[:2]:
            s = dc.sentinel(dc.field(n), idx, cs[0].mag)
            qs = []
            for c in cs:
                with _options(ctx, dc.options(c)):
                    qs.append(ctx.almeida(s, dc.ASPECT, dc.FOV, use_ransac=False)[0])
            for q in qs[1:]: _close(q, qs[0], dc.BOUND, (n, idx, [c.name for c in cs]))


# ---- batches ---------------------------------------------------------------------------------------------------------------------------------
def _batch_size(case):
    import torch
    if case.batch is not None: return case.batch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nblk = dc.chooser(case.n, case.force, 0, case.force_ept, 1, cus)[4]       # 8 records per thread are forced: the batch does not move it
    return cus // nblk + 2


@pytest.mark.parametrize("which", ["own", "torch"])
@pytest.mark.parametrize("case", dc.BATCHES, ids=lambda c: c.name)
def test_batches(ctx, case, which):
    B = _batch_size(case)
    assert B * case.n <= 2_000_000
    items = np.stack([dc.sentinel(dc.item_field(case, b), dc.item_index(case, b, B), case.mag) for b in range(B)])
    rec0 = ctx.almeida_recoveries()
    with _options(ctx, dc.options(case)):
        q = _dev(ctx, items, which=which)                    # (two untouched slots and the guard words behind the batch: _read)
    for b in range(B): _close(q[b], dc.batch_expected(case, b, B), dc.BOUND, (case.name, b))
    assert ctx.almeida_recoveries() == rec0


# ---- RANSAC ------------------------------------------------------------------------------------------------------------------------------
def _sel_check(case, q):
    e = dc.sel_field(case)
    q_o = oracle.solve_ypr_ransac(e, dc.cam(), case.iters, dc.SEL_DEG, dc.SEL_N, case.seed)
    _close(q, q_o, dc.RANSAC_BOUND, case.name)
    if case.winner < 0: assert np.array_equal(_bits(q), _bits(IDENT)), case.name
    elif case.kind != "keep":
        other = "B" if case.pop == "A" else "A"
        assert synth.quat_angle_deg(q, dc.sel_pop_answer(other)) > 0.5, case.name
        assert synth.quat_angle_deg(q, dc.sel_pop_answer(case.pop)) < 0.05, case.name


@pytest.mark.parametrize("case", dc.RANSAC_SELECTION, ids=lambda c: c.name)
def test_ransac_selection(ctx, case):
    q, _ = ctx.almeida(dc.sel_field(case), dc.ASPECT, dc.FOV, use_ransac=True, num_iters=case.iters, inlier_deg=dc.SEL_DEG,
                       num_samples=dc.SEL_N, seed=case.seed)
    _sel_check(case, q)


def test_ransac_selection_on_torch_stream(ctx):
    for case in dc.RANSAC_SELECTION:
        q = _dev(ctx, dc.sel_field(case)[None], which="torch", ransac=True, iters=case.iters, deg=dc.SEL_DEG, ns=dc.SEL_N, seed=case.seed)
        _sel_check(case, q[0])


def _all_runs(case):
    return (None,) + dc.all_positions(case) + (("unsampled",) if dc.all_unsampled(case) is not None else ())


@pytest.mark.parametrize("case", dc.RANSAC_ALL_INLIERS, ids=lambda c: "%dx%d" % (c.n, c.ns))
def test_ransac_all_inliers(ctx, case):
    """every record an inlier: the refit set is iteration 0's samples in sample order, and the answer is the LSQ of exactly that set"""
    for pos in _all_runs(case):
        f, refit = dc.all_field(case, pos)
        q, _ = ctx.almeida(f, dc.ASPECT, dc.FOV, use_ransac=True, num_iters=dc.ALL_ITERS, inlier_deg=dc.ALL_DEG, num_samples=case.ns,
                           seed=dc.ALL_SEED)
        _close(q, dc.solve(refit), dc.BOUND, (case, pos))


def test_ransac_all_inliers_on_torch_stream(ctx):
    for case in dc.RANSAC_ALL_INLIERS:
        pos = _all_runs(case)[-1]
        f, refit = dc.all_field(case, pos)
        q = _dev(ctx, f[None], which="torch", ransac=True, iters=dc.ALL_ITERS, deg=dc.ALL_DEG, ns=case.ns, seed=dc.ALL_SEED)
        _close(q[0], dc.solve(refit), dc.BOUND, (case, pos))


def _par_check(case, q):
    q_o = dc.par_expected(case)
    _close(q, q_o, dc.RANSAC_BOUND, case.name)
    if case.identity:
        assert np.array_equal(q_o, IDENT) and np.array_equal(_bits(q), _bits(IDENT)), case.name      # bits 1, 0, 0, 0
    else:
        assert not np.array_equal(q_o, IDENT) and not np.array_equal(q, IDENT), case.name


@pytest.mark.parametrize("case", dc.RANSAC_PARAMS, ids=lambda c: c.name)
def test_ransac_params(ctx, case):
    q, _ = ctx.almeida(dc.par_field(case), dc.ASPECT, dc.FOV, use_ransac=True, num_iters=case.iters, inlier_deg=case.deg,
                       num_samples=case.ns, seed=case.seed)
    _par_check(case, q)


def test_ransac_params_on_torch_stream(ctx):
    for case in dc.RANSAC_PARAMS:
        q = _dev(ctx, dc.par_field(case)[None], which="torch", ransac=True, iters=case.iters, deg=case.deg, ns=case.ns, seed=case.seed)
        _par_check(case, q[0])


@pytest.mark.parametrize("iters,ns", [(17, 600), (50, 1025)])
def test_ransac_batch_items_draw_with_their_own_seed(ctx, iters, ns):
    """ofps_hip_almeida_dev with seed S: item b is the host call on item b's records with seed S + b -- the same kernels on the same
    numbers, so the same bits -- and within the RANSAC bound of the oracle with that seed"""
    S = dc.BATCH_SEED
    fields = [dc.outlier_field(40, 30, dc.item_euler(b), synth.SEED0 + 300 + b) for b in range(4)]
    q = _dev(ctx, np.stack(fields), ransac=True, iters=iters, deg=0.05, ns=ns, seed=S)
    for b in range(4):
        q_h, _ = ctx.almeida(fields[b], dc.ASPECT, dc.FOV, use_ransac=True, num_iters=iters, inlier_deg=0.05, num_samples=ns, seed=S + b)
        assert np.array_equal(_bits(q[b]), _bits(q_h)), b
        _close(q[b], oracle.solve_ypr_ransac(fields[b], dc.cam(), iters, 0.05, ns, S + b), dc.RANSAC_BOUND, b)
    assert len({_bits(x).tobytes() for x in q}) == 4


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def _refused(ctx, form, change, text):
    import torch
    from ofps_amd.runtime import OfpsHipError
    e = np.array(dc.outlier_field(30, 20), np.float32, copy=True, order="C")
    a = dict(entries=e, batch=1, aspect=dc.ASPECT, fov=dc.FOV, iters=10, samples=100, out=True)
    a.update(change)
    if form == "dev":
        d = torch.from_numpy(e).cuda()
        out = _out(1)
        with pytest.raises(OfpsHipError) as err:
            ctx._check(ctx._lib.ofps_hip_almeida_dev(ctx._h, C.c_void_p(d.data_ptr() if a["entries"] is not None else None), e.shape[0], a["batch"],
                                                     a["aspect"], a["fov"], 1, a["iters"], 0.05, a["samples"], 1,
                                                     C.c_void_p(out.data_ptr() if a["out"] else None)))
        ctx.sync()
        assert (out.cpu().numpy() == PATTERN).all(), "a refused call wrote to its output"
    else:
        q = np.full(4, 7.0, np.float32); tr = np.full(3, 7.0, np.float32)
        fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        with pytest.raises(OfpsHipError) as err:
            ctx._check(ctx._lib.ofps_hip_almeida(ctx._h, fp(e) if a["entries"] is not None else None, e.shape[0], a["aspect"], a["fov"], 1, a["iters"],
                                                 0.05, a["samples"], 1, fp(q) if a["out"] else None, fp(tr)))
        assert (q == 7.0).all() and (tr == 7.0).all(), "a refused call wrote to its output"
    assert err.value.code == EINVAL and text in str(err.value), (str(err.value), text)


@pytest.mark.parametrize("case", dc.REFUSALS, ids=lambda r: r.name)
def test_refusals(ctx, case):
    for form in (("dev", "host") if case.form == "both" else (case.form,)):
        if "batch" in case.change and form == "host": continue
        _refused(ctx, form, case.change, case.text)
    # the context is as good as before
    c = dc.lsq_case("cl_1537")
    q, _ = ctx.almeida(dc.sentinel(dc.field(c.n), c.idx[0], c.mag), dc.ASPECT, dc.FOV, use_ransac=False)
    _close(q, dc.lsq_expected(c, c.idx[0]), dc.BOUND, case.name)


# ---- a sequence of unlike calls on one context ----------------------------------------------------------------------------------------
def _sequence_calls():
    big, one_xcd, batch = dc.lsq_case("cl_66000"), dc.lsq_case("cl_1537"), dc.BATCHES[0]
    B = batch.batch
    items = np.stack([dc.sentinel(dc.item_field(batch, b), dc.item_index(batch, b, B), batch.mag) for b in range(B)])
    host = lambda e, **kw: (lambda c: c.almeida(e, dc.ASPECT, dc.FOV, **kw)[0])
    return [("66000 dense", host(dc.sentinel(dc.field(big.n), big.idx[1], big.mag), use_ransac=False)),
            ("3", host(dc.field(3), use_ransac=False)),
            ("8040 ransac, 16000 samples", host(dc.outlier_field(120, 67), use_ransac=True, num_iters=50, inlier_deg=0.05, num_samples=16000, seed=9)),
            ("1537", host(dc.sentinel(dc.field(one_xcd.n), one_xcd.idx[1], one_xcd.mag), use_ransac=False)),
            ("7 x 600", lambda c: _dev(c, items))]


def test_sequence_of_unlike_calls_is_what_each_call_returns_alone():
    """scratch buffers regrow and shrink in use, hypotheses, counts and selections of an earlier call stay behind in them: each call of
    the sequence must return the bits it returns as the first call of a fresh context"""
    from ofps_amd.runtime import HipContext
    calls = _sequence_calls()
    c = HipContext(0)
    try:
        got = [f(c) for _, f in calls]
        assert c.almeida_recoveries() == 0
    finally:
        c.close()
    for (name, f), q in zip(calls, got):
        c = HipContext(0)
        try:
            alone = f(c)
        finally:
            c.close()
        assert np.isfinite(q).all() and np.array_equal(_bits(q), _bits(alone)), name
