"""A plain-Python restatement of the island tracks (include/ofps_hip.h A5t), on top of tests/indep_detect_islands.py -- written from the
definition, not from the kernel: the pair counts come from shifted whole-grid comparisons, one per window offset, the match is a loop over
Python lists, nothing is reduced by waves or built a block of ranks at a time.  The state is kept as Python objects and serialised to the
header's byte layout on demand.  Test infrastructure only."""
import struct

import numpy as np

import indep_detect_islands as indep

F = np.float32
MAX_TRACKS, MAX_REACH, MAX_GAP = 256, 4, 255
NOT_LISTED = indep.NOT_LISTED


def q(v):
    """the nearest-even integer of clamp(v, -64, 64) * 2^24; NaN -> 0.  The product is exact in f32"""
    v = F(v)
    if np.isnan(v):
        return 0
    c = F(min(max(v, F(-64.0)), F(64.0)))
    return int(np.rint(F(c * F(16777216.0))))


def q_array(a):
    """q over an f32 array -> int64"""
    a = np.asarray(a, F)
    nan = np.isnan(a)
    c = np.clip(np.where(nan, F(0), a), F(-64.0), F(64.0)).astype(F)
    return np.where(nan, 0, np.rint((c * F(16777216.0)).astype(F))).astype(np.int64)


def _pad16(n):
    return (n + 15) & ~15


def state_size(dim, T):
    return 16 + 16 * T + _pad16(2 * dim * dim) + _pad16(dim * dim)


class Tracker:
    """one tracker: step() takes one frame's island list and returns (track_counts [4], rows [n, 8]) as int32 arrays"""

    def __init__(self, dim, T, reach, G, state=None):
        assert 1 <= dim <= 160 and 1 <= T <= MAX_TRACKS and 0 <= reach <= MAX_REACH and 0 <= G <= MAX_GAP
        self.dim, self.T, self.reach, self.G = dim, T, reach, G
        self.t, self.handed = 0, 0
        self.slots = [[0, 0, 0, 0] for _ in range(T)]                    # id, born, hits, last
        self.owner = np.full((dim, dim), -1, np.int64)                   # a slot or -1
        self.gone = np.zeros((dim, dim), np.int64)
        self.freed_ids = set()                                           # (for the property tests; not part of the state)
        if state is not None:
            self._load(bytes(state))

    # ---- the byte layout of include/ofps_hip.h
    def _load(self, b):
        d, T = self.dim, self.T
        assert len(b) == state_size(d, T)
        self.t, self.handed, z0, z1 = struct.unpack_from("<4i", b, 0)
        assert z0 == 0 and z1 == 0
        self.slots = [list(struct.unpack_from("<4i", b, 16 + 16 * s)) for s in range(T)]
        off = 16 + 16 * T
        self.owner = np.frombuffer(b, np.uint16, d * d, off).astype(np.int64).reshape(d, d) - 1
        off += _pad16(2 * d * d)
        self.gone = np.frombuffer(b, np.uint8, d * d, off).astype(np.int64).reshape(d, d)

    def state(self):
        d, T = self.dim, self.T
        out = bytearray(state_size(d, T))
        struct.pack_into("<4i", out, 0, self.t, self.handed, 0, 0)
        for s in range(T):
            struct.pack_into("<4i", out, 16 + 16 * s, *self.slots[s])
        off = 16 + 16 * T
        out[off:off + 2 * d * d] = (self.owner + 1).astype(np.uint16).tobytes()
        off += _pad16(2 * d * d)
        out[off:off + d * d] = self.gone.astype(np.uint8).tobytes()
        return bytes(out)

    # ---- one step
    def overlap(self, labels, n):
        """O[r][s], the ordered pairs (c, c') with labels[c] == r < n, owner[c'] == s, Chebyshev distance <= reach, both in the grid"""
        d, T, R = self.dim, self.T, self.reach
        O = np.zeros((n, T), np.int64)
        if n == 0:
            return O
        lab = np.asarray(labels, np.int64).reshape(d, d)
        for oy in range(-R, R + 1):
            for ox in range(-R, R + 1):
                # c = (x, y), c' = (x + ox, y + oy): the part of the grid where both exist
                ys, ye, xs, xe = max(0, -oy), min(d, d - oy), max(0, -ox), min(d, d - ox)
                if ys >= ye or xs >= xe:
                    continue
                a = lab[ys:ye, xs:xe]
                b = self.owner[ys + oy:ye + oy, xs + ox:xe + ox]
                m = (a < n) & (b >= 0)
                if m.any():
                    np.add.at(O, (a[m], b[m]), 1)
        return O

    def step(self, labels, n_listed, cells=None):
        d, T, G = self.dim, self.T, self.G
        lab = np.asarray(labels, np.int64).reshape(d, d)
        n = min(int(n_listed), T)
        self.t += 1
        t = self.t
        O = self.overlap(lab, n)
        claimed = [False] * T
        rowslot = []
        for r in range(n):
            best = None
            for s in range(T):
                sid = self.slots[s][0]
                if sid == 0 or claimed[s] or O[r][s] < 1:
                    continue
                if best is None or (O[r][s], -sid) > (O[r][best], -self.slots[best][0]):
                    best = s
            if best is not None:
                claimed[best] = True
                self.slots[best][2] += 1
                self.slots[best][3] = t
                rowslot.append(best)
                continue
            free = [s for s in range(T) if self.slots[s][0] == 0 and not claimed[s]]
            if free:
                s = free[0]
                self.handed += 1
                self.slots[s] = [self.handed, t, 1, t]
                claimed[s] = True
                rowslot.append(s)
            else:
                rowslot.append(-1)
        # paint
        slot_of = np.full(NOT_LISTED + 1, -1, np.int64)
        slot_of[:n] = rowslot
        painted = slot_of[np.minimum(lab, NOT_LISTED)]
        tracked = painted >= 0
        other = ~tracked & (self.owner >= 0)
        self.gone = np.where(tracked, 0, np.where(other, self.gone + 1, self.gone))
        self.owner = np.where(tracked, painted, self.owner)
        clear = other & (self.gone > G)
        self.owner = np.where(clear, -1, self.owner)
        self.gone = np.where(clear, 0, self.gone)
        # rows (a slot matched in this step is not freed below)
        rows = np.zeros((n, 8), np.int32)
        for r in range(n):
            s = rowslot[r]
            sx = sy = 0
            if cells is not None:
                c = np.asarray(cells, F).reshape(d, d, 2)[lab == r]
                sx, sy = int(q_array(c[:, 0]).sum()), int(q_array(c[:, 1]).sum())
            ident, born, hits, _ = self.slots[s] if s >= 0 else (0, 0, 0, 0)
            words = struct.unpack("<4i", struct.pack("<2q", sx, sy))
            rows[r] = (ident, s, t - born + 1 if s >= 0 else 0, hits) + words
        # expire
        for s in range(T):
            if self.slots[s][0] != 0 and t - self.slots[s][3] > G:
                self.freed_ids.add(self.slots[s][0])
                self.slots[s] = [0, 0, 0, 0]
        n_live = sum(1 for s in self.slots if s[0] != 0)
        counts = np.array([n, sum(1 for s in rowslot if s >= 0), n_live, t], np.int32)
        return counts, rows


def sums_of(rows):
    """rows [n, 8] int32 -> (sum_mx, sum_my) int64 arrays"""
    w = np.ascontiguousarray(rows[:, 4:8], np.int32).view(np.int64)
    return w[:, 0], w[:, 1]


def run(frames, prm, K, T, reach, G, state=None, with_cells=True):
    """frames: one record array per frame -> ([(counts, table, labels, track_counts, rows), ...], state bytes): densify, A5i and one step
    per frame, what ofps_hip_detect_tracks does"""
    out, trk = [], None
    for e in frames:
        isl = indep.islands(e, **prm)
        counts, table, labels, _ = indep.listed(isl, K)
        if trk is None:
            trk = Tracker(isl.dim, T, reach, G, state)
        tc, rows = trk.step(labels, counts[3], isl.field if with_cells else None)
        out.append((counts, table, labels, tc, rows))
    return out, trk.state()
