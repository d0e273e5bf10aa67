"""The Almeida estimator's RANSAC loop (almeida-estimator/src/lib.rs:202-251) restated in numpy float64 on tests/indep_model.py's
generic 4x4 camera: per hypothesis the three drawn records, the 30 damped steps of the three-sample solve (lib.rs:123-200, the
epsilon-prototype Jacobian taken once at the identity), the squared inlier residual of every sampled record, the inlier count, and how
many sampled records lie within a factor 4 of the squared threshold -- the band in which the device's f32 cosf / atanf could decide
differently.  Only the sampler (oracle.sample_index: it DEFINES which records are drawn) is shared with the oracle.

This is the tool that picks tests/almeida_domain_cases.py's selection cases and proves them robust; it is NOT a second oracle for
quaternions (its rotations are float64, the estimator's are float32)."""
from dataclasses import dataclass

import numpy as np
from scipy.spatial.transform import Rotation

import indep_model as im
import oracle

EPS = 0.001 * np.pi / 180.0                                             # lib.rs:28
STEPS = 30                                                              # ceil(15 / ALPHA), lib.rs:132
BAND = 4.0


class Cam:
    """indep_model's camera with its matrices made once"""

    def __init__(self, aspect, fov_y_deg):
        self.aspect, self.fov = float(aspect), float(fov_y_deg)
        self.P = im.perspective(self.aspect, np.radians(self.fov))
        self.fy = 0.5 / np.tan(np.radians(self.fov) / 2.0)              # camera.rs:121-122
        self.fx = self.fy / self.aspect

    def world(self, pos):
        return im.unproject(self.P, pos, im.VIEW.T)

    def delta_w(self, pos, world, R3):                                  # camera.rs:89-117 on points already unprojected
        return im.project(self.P, im.transform_point(im.rot4(R3), world), im.VIEW) - pos

    def delta(self, pos, R3):
        return self.delta_w(pos, self.world(pos), R3)

    def residual2(self, e, R3):
        """lib.rs:229-236: squared length of (motion - delta) * cos(point_angle(pos + delta))"""
        pos, mot = e[:, :2], e[:, 2:]
        d = self.delta(pos, R3)
        ang = np.arctan((pos + d - 0.5) / np.array([self.fx, self.fy]))
        v = (mot - d) * np.cos(ang)
        return (v * v).sum(1)


def _step_rot(m):
    """lib.rs:189-193: pitch * roll * yaw of one step's angles (nalgebra from_euler_angles(roll, pitch, yaw) = scipy extrinsic xyz)"""
    roll = Rotation.from_euler("xyz", [0.0, m[0], 0.0])
    pitch = Rotation.from_euler("xyz", [m[1], 0.0, 0.0])
    yaw = Rotation.from_euler("xyz", [0.0, 0.0, -m[2]])
    return pitch * roll * yaw


def solve(e, cam: Cam):
    """lib.rs:123-200 on the records e -> the 3x3 matrix of the accumulated rotation (what RANSAC tests its samples with, lib.rs:224;
    the estimator's answer is its inverse)"""
    e = np.asarray(e, np.float64).reshape(-1, 4)
    pos, mot = e[:, :2], e[:, 2:]
    w = cam.world(pos)
    J = np.stack([cam.delta_w(pos, w, im.euler_rot3(0.0, EPS, 0.0)).ravel(),          # lib.rs:30-42
                  cam.delta_w(pos, w, im.euler_rot3(EPS, 0.0, 0.0)).ravel(),
                  cam.delta_w(pos, w, im.euler_rot3(0.0, 0.0, -EPS)).ravel()], 1)
    A = J.T @ J
    rot = Rotation.identity()
    for it in range(STEPS):
        alpha = 1.0 if it == STEPS - 1 else 0.5
        r = (mot - cam.delta_w(pos, w, rot.as_matrix())).ravel()
        try:
            m = np.linalg.solve(A, J.T @ r)
        except np.linalg.LinAlgError:
            m = np.zeros(3)                                             # lib.rs:181-183
        rot = rot * _step_rot(m * EPS * alpha)
    return rot.as_matrix()


@dataclass
class Hyp:
    it: int
    drawn: tuple          # the three records of the fit (stream 0)
    sampled: np.ndarray   # the records tested (stream 1), in sample order
    r2: np.ndarray        # their squared residuals
    count: int
    band: int             # sampled records with thr2 / 4 < r2 < 4 thr2


@dataclass
class Run:
    hyps: list
    winner: int           # first hypothesis with the largest count (strict > in lib.rs:243); -1 when every count is 0
    thr2: float

    @property
    def counts(self):
        return np.array([h.count for h in self.hyps])

    def robust(self):
        """True when no f32 rounding of a residual can change the winner: every hypothesis that ties with the winner has an empty
        band, and the winner leads every other hypothesis by more than that hypothesis's band."""
        if self.winner < 0:
            return all(h.band == 0 for h in self.hyps)
        best = self.hyps[self.winner].count
        for h in self.hyps:
            if h.count == best:
                if h.band != 0: return False
            elif best - h.count <= h.band: return False
        return True


def drawn(seed, it, n):
    return tuple(oracle.sample_index(seed, it, 0, j, n) for j in range(min(n, 3)))


def sampled(seed, it, n, ns):
    return np.array([oracle.sample_index(seed, it, 1, j, n) for j in range(min(ns, n))], np.int64)


def run(e, aspect, fov_y_deg, seed, iters, inlier_deg, num_samples) -> Run:
    e = np.asarray(e, np.float64).reshape(-1, 4)
    n = e.shape[0]
    cam = Cam(aspect, fov_y_deg)
    thr2 = float(np.radians(inlier_deg)) ** 2
    hyps, best, winner = [], 0, -1
    for it in range(iters):
        d3 = drawn(seed, it, n)
        R = solve(e[list(d3)], cam)
        s = sampled(seed, it, n, num_samples)
        r2 = cam.residual2(e[s], R)
        h = Hyp(it, d3, s, r2, int((r2 <= thr2).sum()), int(((r2 > thr2 / BAND) & (r2 < thr2 * BAND)).sum()))
        hyps.append(h)
        if h.count > best: best, winner = h.count, it
    return Run(hyps, winner, thr2)
