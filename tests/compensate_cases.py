"""Cases for the camera-compensation stage (ofps_hip_compensate[_dev]) and the compensated detector of the fused per-frame entry points
(ofps_hip_set_detect_compensation(ctx, 1)).  CPU only: numpy and the CPU oracle -- never the library under test.

The expected values are the oracle's own chain: the residual of the RANSAC inlier test (almeida-estimator/src/lib.rs:224-231),
    out.motion = motion - camera.delta(pos, to_homogeneous(inverse(q)))          (ofps/src/camera.rs:115-117)
as a loop over oracle.camera_delta.  tests/test_compensate_cpu.py pins that these inputs can tell the feature from its absence;
tests/test_compensate_gpu.py runs them."""
from functools import lru_cache

import numpy as np

import oracle

CAM = (16 / 9, 22.275)                                   # the planted field's camera
DETECTOR = dict(min_size=0.05, subdivide=3, target_motion=0.003)             # the detector's defaults: a 14 x 14 field, 196 cells
CELLS = 14 * 14
RANSAC = dict(num_iters=200, inlier_deg=0.05, num_samples=1000)
SEED = 5

# ---- the planted field: a 40 x 22 lattice (the block centres of 640 x 360 luma, 16 x 16 blocks) under a camera rotation, plus an island
LATTICE = (40, 22)
PLANTED_DEG = dict(yaw=0.5, pitch=0.2, roll=0.1)
ISLAND = dict(x0=24, y0=7, w=9, h=5, motion=(0.01, 0.0))         # lattice points [x0, x0 + w) x [y0, y0 + h).  The final geometry: 9 x 5 holds for RANSAC (14 cells) and LSQ (10 cells) here; at y0 = 6 the rectangle straddles fewer cell rows and LSQ leaves 9 cells, under min_size

# ---- the frames of the fused hip_sad cases: 320 x 192 luma, block 16, range 8 -> 20 x 12 = 240 vectors
FRAME_W, FRAME_H, BLOCK, RANGE = 320, 192, 16, 8
FRAME_CAM = (FRAME_W / FRAME_H, 22.275)
N_FRAMES = 6                                             # the stream forms push the first STREAM_FRAMES; the batched form two tickets of three
STREAM_FRAMES = 4
GLOBAL_STEP = (3, 2)                                     # px per frame, the whole content
PATCH_EXTRA = (4, 0)                                     # ... the patch, on top of that
PATCH = dict(x0=176, y0=48, size=64)
# The detector of the frame cases: 12 rows of vectors cannot fill the 14 rows of the default field (two rows of cells stay empty and cut
# every island in three), so the field is 9 x 9 (subdivide 2: ceil(1 / (sqrt(0.05) / 2)) = 9) -- every cell holds at least two vectors.
FRAME_DETECTOR = dict(min_size=0.05, subdivide=2, target_motion=0.003)
FRAME_CELLS = 9 * 9
FRAME_RANSAC = dict(num_iters=100, inlier_deg=0.05, num_samples=240)

RECORD_COUNTS = (0, 1, 63, 64, 65, 880, 8040, 70000)     # 70,000: above the estimator's 65,536 switch to reciprocal quotients


def quat_conj(q):
    q = np.asarray(q, np.float32)
    return np.array([q[0], -q[1], -q[2], -q[3]], np.float32)          # oracle/ofps_oracle.c:orc_quat_inverse


def compensate_oracle(entries, cam, q):
    """entries [n, 4], cam = oracle.camera(..), q = (w, i, j, k) as the estimator returns it -> [n, 4]: pos as it is, motion - delta"""
    e = np.ascontiguousarray(entries, np.float32).reshape(-1, 4)
    m = oracle.quat_to_homogeneous(quat_conj(q))
    out = e.copy()
    for k in range(len(e)):
        d = oracle.camera_delta(cam, e[k, :2], m)
        out[k, 2] = e[k, 2] - d[0]                       # f32 - f32
        out[k, 3] = e[k, 3] - d[1]
    return out


def planted_quat():
    """the POINT rotation the field is planted with; the estimator's answer to that field is its inverse (lib.rs:199)"""
    r = np.float32(np.pi / 180)
    return oracle.quat_from_euler(np.float32(PLANTED_DEG["roll"]) * r, np.float32(PLANTED_DEG["pitch"]) * r, np.float32(PLANTED_DEG["yaw"]) * r)


@lru_cache(maxsize=1)
def planted_field():
    """-> [880, 4] read-only: motion = camera.delta(pos, planted rotation), + ISLAND['motion'] inside the island"""
    cam = oracle.camera(*CAM)
    m = oracle.quat_to_homogeneous(planted_quat())
    w, h = LATTICE
    e = np.zeros((w * h, 4), np.float32)
    for y in range(h):
        for x in range(w):
            p = np.array([(x + 0.5) / w, (y + 0.5) / h], np.float32)
            d = oracle.camera_delta(cam, p, m)
            inside = ISLAND["x0"] <= x < ISLAND["x0"] + ISLAND["w"] and ISLAND["y0"] <= y < ISLAND["y0"] + ISLAND["h"]
            e[y * w + x] = (p[0], p[1], d[0] + np.float32(ISLAND["motion"][0] if inside else 0), d[1] + np.float32(ISLAND["motion"][1] if inside else 0))
    e.setflags(write=False)
    return e


def random_records(n, seed=0):
    """positions anywhere in the frame, motions up to a few percent of it"""
    rng = np.random.default_rng(1000 + seed)
    e = np.empty((n, 4), np.float32)
    e[:, :2] = rng.random((n, 2), np.float32)
    e[:, 2:] = (rng.random((n, 2), np.float32) - 0.5) * 0.06
    return e


def random_quat(seed=0):
    """a unit quaternion a degree or so from the identity (what an estimator hands back), f32"""
    rng = np.random.default_rng(2000 + seed)
    a = (rng.random(3) - 0.5) * np.float32(0.04)
    return oracle.quat_from_euler(np.float32(a[0]), np.float32(a[1]), np.float32(a[2]))


@lru_cache(maxsize=1)
def _content():
    from ofps_amd import synth
    margin = 48
    c = synth.random_luma(1, FRAME_W + 2 * margin, FRAME_H + 2 * margin, seed=31)[0].astype(np.float32)
    k = np.ones(7, np.float32) / 7
    for _ in range(2):
        for axis in (0, 1):
            c = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), axis, c)
    bg = ((c - c.min()) / (c.max() - c.min()) * 255).astype(np.uint8)
    s = PATCH["size"]
    obj = np.ascontiguousarray(bg[:s, :s][::-1, ::-1])            # another piece of the same texture, turned round
    return bg, obj, margin


@lru_cache(maxsize=1)
def frames():
    """-> uint8 [6, 192, 320] read-only: the content moves by GLOBAL_STEP per frame, the patch by GLOBAL_STEP + PATCH_EXTRA"""
    bg, obj, margin = _content()
    out = np.zeros((N_FRAMES, FRAME_H, FRAME_W), np.uint8)
    s = PATCH["size"]
    for k in range(N_FRAMES):
        oy, ox = margin - GLOBAL_STEP[1] * k, margin - GLOBAL_STEP[0] * k
        out[k] = bg[oy:oy + FRAME_H, ox:ox + FRAME_W]
        py = PATCH["y0"] + (GLOBAL_STEP[1] + PATCH_EXTRA[1]) * k
        px = PATCH["x0"] + (GLOBAL_STEP[0] + PATCH_EXTRA[0]) * k
        out[k, py:py + s, px:px + s] = obj
    out.setflags(write=False)
    return out


@lru_cache(maxsize=8)
def frame_vectors(k):
    """the oracle's SAD vectors of pair (k - 1, k) -> [240, 4] read-only"""
    f = frames()
    ent, _ = oracle.sad_flow(f[k - 1], f[k], BLOCK, RANGE)
    ent = np.ascontiguousarray(ent, np.float32)
    ent.setflags(write=False)
    return ent


@lru_cache(maxsize=32)
def _expected(kind, n, seed):
    e = planted_field() if kind == "planted" else random_records(n, seed)
    q = random_quat(seed)
    out = compensate_oracle(e, oracle.camera(*CAM), q)
    out.setflags(write=False)
    return e, q, out


def expected_case(kind, n, seed=0):
    """-> (records [n, 4], quaternion, the oracle's compensated records), computed once per process"""
    return _expected(kind, int(n), int(seed))


def oracle_quat(entries, cam_args, use_ransac, ransac=None, seed=SEED):
    cam = oracle.camera(*cam_args)
    if use_ransac:
        return np.asarray(oracle.solve_ypr_ransac(entries, cam, seed=seed, **(ransac or RANSAC)), np.float32)
    return np.asarray(oracle.solve_ypr_given(entries, cam), np.float32)


def area_of(det):
    return 0 if det is None else det[0]
