"""Case tables and builders for the whole-domain tests of hip_almeida (ofps_amd/csrc/almeida.hip): CPU only, no GPU call in here.
tests/test_almeida_domain_cpu.py proves on the oracle that every case has the property it is listed for and that every literal below
holds; tests/test_almeida_domain_gpu.py runs the cases through the library.

Why sentinels: the least-squares parity bound (2e-6 on the quaternion) is wider than what one ordinary record contributes to a smooth
field, so a kernel that loses its last record, reads one past the end or folds a partial sum twice stays inside it.  sentinel() raises
ONE record's motion until that record alone moves the oracle's answer by >= 2e-4 (100 x the bound) when it is dropped or counted
twice, while the order in which the records are summed still moves it by < 2e-7."""
import functools
from collections import namedtuple

import numpy as np

import oracle
from ofps_amd import synth

ASPECT, FOV = 16 / 9, 22.275
BOUND = 2e-6                 # least-squares parity bound (tests/test_gpu_parity.py, tests/test_reference_vectors_gpu.py)
RANSAC_BOUND = 1e-4          # RANSAC parity bound (same files)
EFFECT_MIN = 2e-4            # what dropping or doubling a sentinel must do to the oracle: 100 x BOUND
PERM_MAX = 2e-7              # what permuting the records may do to it: BOUND / 10
CUS = 256                    # the chooser literals below are for a 256-CU device (MI355X)
ORACLE_THREADS = 8           # oracle.solve_ypr_given(threads=...) returns the same bits as one thread


def cam():
    return oracle.camera(ASPECT, FOV)


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def field(n, euler=(0.5, 0.3, -0.2), seed=synth.SEED0 + 3):
    """the first n records of the smallest ~16:9 raster w x h >= n of synth.rotation_field (read-only, shared)"""
    w = max(int(np.ceil(np.sqrt(n * 16 / 9))), 1)
    h = max(-(-n // w), 1)
    return _ro(synth.rotation_field(w, h, euler_deg=euler, seed=seed)[:n].copy())


def sentinel(e, idx, mag):
    """copy of e with mag added to both motion components of record idx"""
    s = np.array(e, np.float32, copy=True)
    s[idx, 2:4] += np.float32(mag)
    return s


def solve(e):
    return oracle.solve_ypr_given(e, cam(), threads=ORACLE_THREADS if len(e) >= 4096 else 1)


@functools.lru_cache(maxsize=None)
def lsq_expected(case, idx):
    """the oracle's quaternion of case's field with its sentinel at idx (computed once, shared by every test)"""
    return _ro(solve(sentinel(field(case.n), idx, case.mag)))


# ---- the path chooser (lsq_device / lsq_cluster / lsq_stepped of almeida.hip) restated for one host-count problem ------------------
def chooser(n, path=None, block=0, ept=0, batch=1, cus=CUS):
    """-> (path, block, ept, per_wg, nblk): which solver a call with n records per item takes, its workgroup width, records per thread,
    records per workgroup and workgroups per item.  path / block / ept restate OFPS_HIP_ALMEIDA_PATH / _BLOCK / _EPT."""
    def stepped():
        per = 8192 if n > 65536 else 1024
        nb = max(min(-(-n // per), (2 * cus + batch - 1) // batch), 1)
        return ("step", 1024, per // 1024, per, nb)
    wg_path, cluster, cmin = n <= 8192, True, (1536 if batch == 1 else 8192)
    if path == "step": wg_path = cluster = False
    if path == "wg": cluster = False
    if path == "cluster": cmin = 0
    if cluster and n > cmin and n > 0:
        dense = n > 65536
        emax = 8 if dense else 4
        e_, best = emax, 1e30
        for e in (1, 2, 4, 8):
            if e > emax: continue
            nb = -(-n // (e * 1024))
            if nb < 1 or nb > 256 or nb > cus: continue
            per = cus // nb
            cost = ((batch + per - 1) // per) * (0.11 + 0.004 * e + 0.00001 * nb + (0.006 if nb >= 65 else 0.0))
            if cost < best: best, e_ = cost, e
        blk = 1024
        e256 = 1 if n <= 16384 else (2 if n <= 32768 else 4)
        if not dense:
            nb256 = -(-n // (e256 * 256))
            if nb256 <= 64 and nb256 * batch <= cus: blk = 256
        if block: blk = block
        if blk == 256: e_ = e256
        if ept: e_ = min(ept, emax)
        per_wg = e_ * blk
        nb = -(-n // per_wg)
        if 1 <= nb <= 256 and nb <= cus: return ("cluster", blk, e_, per_wg, nb)
    if wg_path:
        e_ = 1 if n <= 1024 else (2 if n <= 2048 else (4 if n <= 4096 else 8))
        return ("wg", 1024, e_, e_ * 1024, 1)
    return stepped()


def sentinel_indices(n, per_wg, nblk):
    """at most six of {0, n - 1, per_wg - 1, per_wg, (nblk - 1) per_wg, 1023, 1024, n - 2} inside [0, n), in that order of preference"""
    out = []
    for i in (0, n - 1, per_wg - 1, per_wg, (nblk - 1) * per_wg, 1023, 1024, n - 2):
        if 0 <= i < n and i not in out: out.append(i)
    return tuple(out[:6])


def options(case):
    """the option settings that reach the case's path (all reset by the caller afterwards)"""
    o = {}
    if case.force: o["OFPS_HIP_ALMEIDA_PATH"] = case.force
    if case.force == "cluster" and case.block == 1024:
        o["OFPS_HIP_ALMEIDA_BLOCK"] = 1024; o["OFPS_HIP_ALMEIDA_EPT"] = case.ept
    if getattr(case, "force_ept", 0): o["OFPS_HIP_ALMEIDA_EPT"] = case.force_ept
    return o


# name, records, forced path (None: the library chooses), then what the chooser makes of it on 256 CUs -- path, workgroup width,
# records per thread, records per workgroup, workgroups -- the sentinel's magnitude and where it is put (one run per index)
Lsq = namedtuple("Lsq", "name n force path block ept per_wg nblk mag idx")
LSQ_COUNTS = (
    Lsq("wg_3", 3, None, "wg", 1024, 1, 1024, 1, 0.0625, (0, 2, 1)),
    Lsq("wg_4", 4, None, "wg", 1024, 1, 1024, 1, 0.0625, (0, 3, 2)),
    Lsq("wg_63", 63, None, "wg", 1024, 1, 1024, 1, 4.0, (0, 62, 61)),
    Lsq("wg_64", 64, None, "wg", 1024, 1, 1024, 1, 4.0, (0, 63, 62)),
    Lsq("wg_65", 65, None, "wg", 1024, 1, 1024, 1, 4.0, (0, 64, 63)),
    Lsq("wg_1023", 1023, None, "wg", 1024, 1, 1024, 1, 4.0, (0, 1022, 1021)),
    Lsq("wg_1024", 1024, None, "wg", 1024, 1, 1024, 1, 4.0, (0, 1023, 1022)),
    Lsq("wg_1025", 1025, None, "wg", 1024, 2, 2048, 1, 4.0, (0, 1024, 1023)),
    Lsq("wg_1535", 1535, None, "wg", 1024, 2, 2048, 1, 4.0, (0, 1534, 1023, 1024, 1533)),
    Lsq("wg_1536", 1536, None, "wg", 1024, 2, 2048, 1, 4.0, (0, 1535, 1023, 1024, 1534)),
    Lsq("wgf_2047", 2047, "wg", "wg", 1024, 2, 2048, 1, 4.0, (0, 2046, 1023, 1024, 2045)),
    Lsq("wgf_2048", 2048, "wg", "wg", 1024, 2, 2048, 1, 4.0, (0, 2047, 1023, 1024, 2046)),
    Lsq("wgf_2049", 2049, "wg", "wg", 1024, 4, 4096, 1, 4.0, (0, 2048, 1023, 1024, 2047)),
    Lsq("wgf_4095", 4095, "wg", "wg", 1024, 4, 4096, 1, 4.0, (0, 4094, 1023, 1024, 4093)),
    Lsq("wgf_4096", 4096, "wg", "wg", 1024, 4, 4096, 1, 4.0, (0, 4095, 1023, 1024, 4094)),
    Lsq("wgf_4097", 4097, "wg", "wg", 1024, 8, 8192, 1, 4.0, (0, 4096, 1023, 1024, 4095)),
    Lsq("wgf_8191", 8191, "wg", "wg", 1024, 8, 8192, 1, 8.0, (0, 8190, 1023, 1024, 8189)),
    Lsq("wgf_8192", 8192, "wg", "wg", 1024, 8, 8192, 1, 8.0, (0, 8191, 1023, 1024, 8190)),
    Lsq("cl_1537", 1537, None, "cluster", 256, 1, 256, 7, 4.0, (0, 1536, 255, 256, 1023, 1024)),
    Lsq("cl_8040", 8040, None, "cluster", 256, 1, 256, 32, 4.0, (0, 8039, 255, 256, 7936, 1023)),
    Lsq("cl_16383", 16383, None, "cluster", 256, 1, 256, 64, 8.0, (0, 16382, 255, 256, 16128, 1023)),
    Lsq("cl_16384", 16384, None, "cluster", 256, 1, 256, 64, 8.0, (0, 16383, 255, 256, 16128, 1023)),
    Lsq("cl_16385", 16385, None, "cluster", 256, 2, 512, 33, 8.0, (0, 16384, 511, 512, 1023, 1024)),
    Lsq("cl_32768", 32768, None, "cluster", 256, 2, 512, 64, 32.0, (0, 32767, 511, 512, 32256, 1023)),
    Lsq("cl_32769", 32769, None, "cluster", 256, 4, 1024, 33, 32.0, (0, 32768, 1023, 1024, 32767)),
    Lsq("cl_65535", 65535, None, "cluster", 256, 4, 1024, 64, 64.0, (0, 65534, 1023, 1024, 64512, 65533)),
    Lsq("cl_65536", 65536, None, "cluster", 256, 4, 1024, 64, 64.0, (0, 65535, 1023, 1024, 64512, 65534)),
    Lsq("cl_65537", 65537, None, "cluster", 1024, 2, 2048, 33, 64.0, (0, 65536, 2047, 2048, 1023, 1024)),
    Lsq("cl_66000", 66000, None, "cluster", 1024, 2, 2048, 33, 32.0, (0, 65999, 2047, 2048, 65536, 1023)),
    Lsq("cl1024x1_1023", 1023, "cluster", "cluster", 1024, 1, 1024, 1, 4.0, (0, 1022, 1021)),
    Lsq("cl1024x1_1025", 1025, "cluster", "cluster", 1024, 1, 1024, 2, 4.0, (0, 1024, 1023)),
    Lsq("cl1024x1_3071", 3071, "cluster", "cluster", 1024, 1, 1024, 3, 4.0, (0, 3070, 1023, 1024, 2048, 3069)),
    Lsq("cl1024x1_3073", 3073, "cluster", "cluster", 1024, 1, 1024, 4, 4.0, (0, 3072, 1023, 1024, 3071)),
    Lsq("cl1024x2_2047", 2047, "cluster", "cluster", 1024, 2, 2048, 1, 4.0, (0, 2046, 1023, 1024, 2045)),
    Lsq("cl1024x2_2049", 2049, "cluster", "cluster", 1024, 2, 2048, 2, 4.0, (0, 2048, 2047, 1023, 1024)),
    Lsq("cl1024x2_6143", 6143, "cluster", "cluster", 1024, 2, 2048, 3, 4.0, (0, 6142, 2047, 2048, 4096, 1023)),
    Lsq("cl1024x2_6145", 6145, "cluster", "cluster", 1024, 2, 2048, 4, 4.0, (0, 6144, 2047, 2048, 1023, 1024)),
    Lsq("cl1024x4_4095", 4095, "cluster", "cluster", 1024, 4, 4096, 1, 4.0, (0, 4094, 1023, 1024, 4093)),
    Lsq("cl1024x4_4097", 4097, "cluster", "cluster", 1024, 4, 4096, 2, 4.0, (0, 4096, 4095, 1023, 1024)),
    Lsq("cl1024x4_12287", 12287, "cluster", "cluster", 1024, 4, 4096, 3, 8.0, (0, 12286, 4095, 4096, 8192, 1023)),
    Lsq("cl1024x4_12289", 12289, "cluster", "cluster", 1024, 4, 4096, 4, 4.0, (0, 12288, 4095, 4096, 1023, 1024)),
    Lsq("step_1", 1, "step", "step", 1024, 1, 1024, 1, 0.0, ()),
    Lsq("step_3", 3, "step", "step", 1024, 1, 1024, 1, 0.0625, (0, 2, 1)),
    Lsq("step_1023", 1023, "step", "step", 1024, 1, 1024, 1, 4.0, (0, 1022, 1021)),
    Lsq("step_1025", 1025, "step", "step", 1024, 1, 1024, 2, 4.0, (0, 1024, 1023)),
    Lsq("step_8193", 8193, "step", "step", 1024, 1, 1024, 9, 8.0, (0, 8192, 1023, 1024, 8191)),
    Lsq("step_65536", 65536, "step", "step", 1024, 1, 1024, 64, 64.0, (0, 65535, 1023, 1024, 64512, 65534)),
    Lsq("step_65537", 65537, "step", "step", 1024, 8, 8192, 9, 64.0, (0, 65536, 8191, 8192, 1023, 1024)),
    Lsq("step_73729", 73729, "step", "step", 1024, 8, 8192, 10, 32.0, (0, 73728, 8191, 8192, 1023, 1024)),
)


def lsq_case(name):
    return next(c for c in LSQ_COUNTS if c.name == name)


# ---- batches (ofps_hip_almeida_dev) ---------------------------------------------------------------------------------------------------
# Every item has a rotation of its own on a 0.35 degree grid of Euler angles (>= 0.3 degrees from every other item's, asserted on the
# CPU) and its sentinel at an index of its own: an item written to the wrong slot, or read at the wrong stride, is a gross error.
# batch None: num_cus // nblk + 2 items, so that the library's loop over launches makes a full one and then one of two items (30 on 256
# CUs; the GPU test reads the CU count).  force_ept: 66,000 records take 8 records per thread only when told to (for 30 items the cost
# model picks 4, two launches of 15); 8 is what makes one launch hold num_cus // 9 items.
Batch = namedtuple("Batch", "name n batch force force_ept path block ept per_wg nblk per_launch mag")
BATCHES = (
    Batch("7x600", 600, 7, None, 0, "wg", 1024, 1, 1024, 1, 0, 4.0),
    Batch("3x1025", 1025, 3, None, 0, "wg", 1024, 2, 2048, 1, 0, 4.0),
    Batch("2x8192", 8192, 2, None, 0, "wg", 1024, 8, 8192, 1, 0, 8.0),
    Batch("3x9000", 9000, 3, None, 0, "cluster", 256, 1, 256, 36, 7, 8.0),
    Batch("b0_66000", 66000, None, None, 8, "cluster", 1024, 8, 8192, 9, 28, 64.0),
    Batch("step_100x9000", 9000, 100, "step", 0, "step", 1024, 1, 1024, 6, 0, 8.0),
)


def batch_size(case, cus=CUS):
    return case.batch if case.batch is not None else cus // case.nblk + 2


def item_euler(b):
    """item b's rotation: a point of a 5 x 5 x 4 grid of (roll, pitch, yaw) at 0.35 degrees spacing"""
    return (0.35 * (b % 5) - 0.7, 0.35 * ((b // 5) % 5) - 0.7, 0.35 * (b // 25) - 0.5)


def item_index(case, b, batch):
    """item b's sentinel: the case's boundary records first, then one place per item spread over the field"""
    special = sentinel_indices(case.n, case.per_wg, case.nblk)
    if b < len(special): return special[b]
    return (b * (case.n // batch) + 17) % case.n


def item_field(case, b):
    return field(case.n, item_euler(b), synth.SEED0 + 200 + b)


@functools.lru_cache(maxsize=None)
def batch_expected(case, b, batch):
    return _ro(solve(sentinel(item_field(case, b), item_index(case, b, batch), case.mag)))


# ---- RANSAC: which hypothesis wins ---------------------------------------------------------------------------------------------------------
# 192 records (a 16 x 12 raster, no noise), num_samples = n, inlier_deg = 0.05.  Kinds:
#   even_odd   even indices from a roll of 0.8 degrees (population A), odd ones from a pitch of -0.8 degrees (B): every hypothesis drawn
#              from three records of one population counts exactly that population, 96; the first such hypothesis wins
#   split60    indices with i % 5 < 3 are A (116 records), the others B (76): the count decides, not the order
#   keep       the listed 18 records are A, every other record is a gross outlier (0.15 .. 0.35 of the screen off A's motion): the
#              records were picked so that exactly ONE hypothesis of the run draws three of them -- the winner, wherever we want it
# Robustness (asserted on the CPU with tests/indep_ransac.py): no hypothesis that ties with the winner has a sampled record whose squared
# residual is within a factor 4 of the squared threshold, and the winner leads every other hypothesis by more than the number of that
# hypothesis's records inside that band -- the device's cosf / atanf cannot flip the decision.
SEL_N, SEL_DEG = 192, 0.05
POP_EULER = {"A": (0.8, 0.0, 0.0), "B": (0.0, -0.8, 0.0)}
Sel = namedtuple("Sel", "name kind keep seed iters winner pop count why")
KEEP_1025 = (4, 10, 19, 25, 60, 63, 79, 80, 85, 87, 98, 103, 104, 135, 136, 144, 158, 168)
KEEP_2049 = (44, 51, 53, 54, 68, 69, 78, 93, 101, 123, 124, 127, 137, 165, 171, 173, 183, 189)
RANSAC_SELECTION = (
    Sel("B_then_A", "even_odd", None, 0, 16, 2, "B", 96, "pure hypotheses at 2 (B), 4 (A), 6, 9 (B), 15 (A): the first wins, not the last"),
    Sel("A_then_B", "even_odd", None, 2, 16, 1, "A", 96, "pure hypotheses at 1 (A), 3, 5, 11 (B)"),
    Sel("last_quad_16", "even_odd", None, 3, 16, 15, "B", 96, "the winner is the last quad of the first wave and the very last iteration"),
    Sel("last_quad_17", "even_odd", None, 3, 17, 15, "B", 96, "16, the first quad of the second wave, is pure A and ties: the earlier one wins"),
    Sel("first_quad_17", "even_odd", None, 763, 17, 16, "B", 96, "the only pure hypothesis is the first quad of the second wave, a wave with one live quad"),
    Sel("none_4", "even_odd", None, 29, 4, -1, None, 0, "no pure hypothesis and nothing counted at all: the identity"),
    Sel("split60", "split60", None, 3, 32, 6, "A", 116, "B's first pure hypothesis (4, 76 inliers) comes before A's (6, 116)"),
    Sel("late_1025", "keep", KEEP_1025, 5, 1025, 1024, "A", 18, "the winner is the selection kernel's second pass over the keys"),
    Sel("late_2049", "keep", KEEP_2049, 6, 2049, 1700, "A", 18, "1,700 = thread 676's second key"),
)


@functools.lru_cache(maxsize=None)
def pop_field(pop):
    return _ro(synth.rotation_field(16, 12, sigma=0.0, euler_deg=POP_EULER[pop]))


def sel_mask(case):
    """True where the record belongs to population A"""
    i = np.arange(SEL_N)
    if case.kind == "even_odd": return i % 2 == 0
    if case.kind == "split60": return i % 5 < 3
    m = np.zeros(SEL_N, bool); m[list(case.keep)] = True
    return m


def sel_field(case):
    m = sel_mask(case)
    if case.kind != "keep":
        return np.where(m[:, None], pop_field("A"), pop_field("B")).astype(np.float32)
    e = np.array(pop_field("A"), np.float32, copy=True)
    u, v = synth._gauss(SEL_N, synth.SEED0 + 31), synth._gauss(SEL_N, synth.SEED0 + 32)
    off = np.stack([np.where(u >= 0, 1.0, -1.0) * (0.15 + 0.1 * np.minimum(np.abs(u), 2.0)),
                    np.where(v >= 0, 1.0, -1.0) * (0.15 + 0.1 * np.minimum(np.abs(v), 2.0))], 1)
    e[~m, 2:] += off[~m].astype(np.float32)
    return e


def sel_pop_answer(pop):
    """what the estimator answers for a field of one population alone"""
    return solve(pop_field(pop))


# ---- RANSAC: every record an inlier ----------------------------------------------------------------------------------------------------
# inlier_deg = 1e4: the squared threshold is ~3e4, every record is an inlier of every hypothesis, iteration 0 wins, and the refit set is
# the sampled records of iteration 0 in sample order -- so the expected quaternion is oracle.solve_ypr_given of that set at the LSQ bound,
# without the oracle's RANSAC routine.  Sentinels (|mag|^2 far below the threshold) go on sampled positions j; "unsampled" puts one on
# a record that is not sampled (ns < n), which must not matter.
ALL_DEG, ALL_SEED, ALL_ITERS = 1e4, 11, 3
AllIn = namedtuple("AllIn", "n ns why")
RANSAC_ALL_INLIERS = (
    AllIn(3, 3, ""), AllIn(5, 3, "the sampler's cycle walk"), AllIn(17, 16, ""), AllIn(1025, 1024, "one compaction round exactly"),
    AllIn(1025, 1025, "a second round of one sample"), AllIn(1025, 5000, "num_samples clamped to n"), AllIn(4000, 2049, "three rounds"),
    AllIn(9000, 8192, "the largest refit of the one-workgroup solver"), AllIn(9000, 8193, "refit above 8,192: one read-back, then the cluster solver"),
    AllIn(20000, 16000, "the plugin's maximum"),
)


def all_mag(ns):
    """+4.0 as for the least-squares cases, doubled where the refit set is large enough to need it; 2^-4 below 64 records (see
    LSQ_COUNTS' smallest cases)"""
    return 0.0625 if ns < 64 else (4.0 if ns < 4096 else (8.0 if ns < 10000 else 16.0))


@functools.lru_cache(maxsize=None)
def all_sampled(case):
    ns = min(case.ns, case.n)
    return _ro(np.array([oracle.sample_index(ALL_SEED, 0, 1, j, case.n) for j in range(ns)], np.int64))


def all_positions(case):
    """sampled positions that carry a sentinel (one run each)"""
    ns = min(case.ns, case.n)
    out = []
    for j in (0, ns - 1, 1023, 1024, 2047, 2048):
        if 0 <= j < ns and j not in out: out.append(j)
    return tuple(out)


def all_unsampled(case):
    """a record that iteration 0 does not sample and no iteration draws for its fit, or None when there is none"""
    if min(case.ns, case.n) >= case.n: return None
    taken = set(all_sampled(case).tolist())
    for it in range(ALL_ITERS): taken |= {oracle.sample_index(ALL_SEED, it, 0, j, case.n) for j in range(3)}
    return next((i for i in range(case.n) if i not in taken), None)


def all_field(case, pos):
    """pos: a sampled position, "unsampled", or None for the plain field -> (records, the refit set in sample order)"""
    e = field(case.n)
    s = all_sampled(case)
    if pos == "unsampled": e = sentinel(e, all_unsampled(case), all_mag(min(case.ns, case.n)))
    elif pos is not None: e = sentinel(e, int(s[pos]), all_mag(min(case.ns, case.n)))
    return e, e[s]


# ---- RANSAC: parameter edges -----------------------------------------------------------------------------------------------------------
# one population with 30 % gross outliers against oracle.solve_ypr_ransac at RANSAC_BOUND
@functools.lru_cache(maxsize=None)
def outlier_field(w, h, euler=(0.5, 0.3, -0.2), seed=synth.SEED0 + 3, sigma=2e-4):
    return _ro(synth.rotation_field(w, h, euler_deg=euler, seed=seed, sigma=sigma, outlier_frac=0.3))


Par = namedtuple("Par", "name w h sigma iters deg ns seed identity")
RANSAC_PARAMS = (
    # (seed 27: its one hypothesis has 420 inliers; seed 21's first good hypothesis is the eighth)
    Par("iters_1", 30, 20, 2e-4, 1, 0.05, 600, 27, False), Par("iters_15", 30, 20, 2e-4, 15, 0.05, 600, 21, False),
    Par("iters_16", 30, 20, 2e-4, 16, 0.05, 600, 21, False), Par("iters_17", 30, 20, 2e-4, 17, 0.05, 600, 21, False),
    Par("iters_1023", 30, 20, 2e-4, 1023, 0.05, 600, 21, False), Par("iters_1024", 30, 20, 2e-4, 1024, 0.05, 600, 21, False),
    Par("iters_1025", 30, 20, 2e-4, 1025, 0.05, 600, 21, False), Par("iters_65535", 8, 8, 2e-4, 65535, 0.05, 64, 21, False),
    # fewer than three samples can never give three inliers: the identity, bits 1, 0, 0, 0
    Par("samples_1", 30, 20, 2e-4, 50, 0.05, 1, 21, True), Par("samples_2", 30, 20, 2e-4, 50, 0.05, 2, 21, True),
    Par("samples_3", 30, 20, 0.0, 50, 0.05, 3, 0, None), Par("samples_4", 30, 20, 0.0, 50, 0.05, 4, 0, None),
    # a threshold nothing meets: the best count stays below three (asserted on the CPU, with an empty band): the identity
    Par("deg_tiny", 30, 20, 2e-4, 20, 1e-6, 600, 21, True),
)
BATCH_SEED = 100             # ofps_hip_almeida_dev with seed S: item b draws with S + b, i.e. equals the host call with seed S + b


def par_field(case):
    return outlier_field(case.w, case.h, sigma=case.sigma)


@functools.lru_cache(maxsize=None)
def par_expected(case):
    return oracle.solve_ypr_ransac(par_field(case), cam(), case.iters, case.deg, case.ns, case.seed, threads=ORACLE_THREADS if case.iters > 2000 else 1)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
# what to change in a valid call (600 records, batch 1, ASPECT, FOV, RANSAC with 10 iterations and 100 samples) and the message
Refusal = namedtuple("Refusal", "name form change text")
REFUSALS = (
    Refusal("batch_0", "dev", dict(batch=0), "almeida: batch 0 out of range"),
    Refusal("batch_65536", "dev", dict(batch=65536), "almeida: batch 65536 out of range"),
    Refusal("aspect_0", "both", dict(aspect=0.0), "almeida: bad camera (aspect=0 fov_y=22.275)"),
    Refusal("aspect_neg", "both", dict(aspect=-1.0), "almeida: bad camera (aspect=-1 fov_y=22.275)"),
    Refusal("fov_0", "both", dict(fov=0.0), "almeida: bad camera (aspect=1.77778 fov_y=0)"),
    Refusal("fov_180", "both", dict(fov=180.0), "almeida: bad camera (aspect=1.77778 fov_y=180)"),
    Refusal("fov_nan", "both", dict(fov=float("nan")), "almeida: bad camera (aspect=1.77778 fov_y=nan)"),
    Refusal("iters_0", "both", dict(iters=0), "almeida: ransac iters 0 out of range"),
    Refusal("iters_65536", "both", dict(iters=65536), "almeida: ransac iters 65536 out of range"),
    Refusal("samples_0", "both", dict(samples=0), "almeida: ransac samples must be >= 1"),
    Refusal("null_entries", "dev", dict(entries=None), "almeida: null device pointer"),
    Refusal("null_entries_host", "host", dict(entries=None), "almeida: null host pointer"),
    Refusal("null_output", "dev", dict(out=None), "almeida: null device pointer"),
    Refusal("null_output_host", "host", dict(out=None), "almeida: null host pointer"),
)
