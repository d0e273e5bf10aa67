"""hip_klt's intra test and scene-cut rule (include/ofps_hip.h, row N3i) restated in plain NumPy and Python integers, laid over the existing
restatements: tests/indep_klt_pred.py's flow_from (which is N3, N3m, N3f and N3p in one function) and tests/indep_klt_batch_pred.py's item
order.  The activity, the verdict, the cut and the status rewrite are written from the header's text; every value is a Python int, so the
64-bit comparison cannot wrap.  No code is shared with the library.  Test infrastructure only."""
import numpy as np

import indep_klt_batch_pred as ibp
import indep_klt_pred as ip
from indep_klt import ST_KEPT, ST_RESIDUAL, record
from indep_klt_fb import ST_NO_RETURN

ST_INTRA, ST_CUT = 6, 7
CANDIDATES = (ST_KEPT, ST_RESIDUAL, ST_NO_RETURN)


def activity_point(img, x, y, w):
    """A of the (2w + 1)^2 window of img centred on (x, y), pixel indices clamped into the frame -> (A, m)"""
    H, W = img.shape
    n = 2 * w + 1
    N = n * n
    px = [int(img[min(max(y + j, 0), H - 1), min(max(x + i, 0), W - 1)]) for j in range(-w, w + 1) for i in range(-w, w + 1)]
    m = (sum(px) + N // 2) // N
    return sum(abs(p - m) for p in px), m


def activity(img, points, w):
    """points int [n, 2] (x, y) -> uint32 [n]; a point outside the frame has A = 0 (the _dev stage form's answer)"""
    H, W = img.shape
    pts = np.asarray(points, np.int64).reshape(-1, 2)
    return np.array([activity_point(img, int(x), int(y), w)[0] if 0 <= x < W and 0 <= y < H else 0 for x, y in pts], np.uint32)


def is_intra(res, A, q):
    return 16 * int(res) >= int(q) * 256 * int(A)


def is_cut(n_cand, n_intra, P):
    return P > 0 and 100 * int(n_intra) >= int(P) * int(n_cand)


def verdict(quads, activities, q, P=0):
    """quads int [n, 4] (dqx, dqy, res, status), activities [n] (any non-negative integers) -> (statuses int32 [n], [n_cand, n_intra], cut)"""
    qd = np.asarray(quads).reshape(-1, 4)
    st = np.array([int(s) for s in qd[:, 3]], np.int32)
    n_cand = n_intra = 0
    for k in range(len(qd)):
        if int(qd[k, 3]) not in CANDIDATES:
            continue
        n_cand += 1
        if is_intra(qd[k, 2], activities[k], q):
            n_intra += 1
            if st[k] == ST_KEPT:
                st[k] = ST_INTRA
    cut = is_cut(n_cand, n_intra, P)
    if cut:
        st[st == ST_KEPT] = ST_CUT
    return st, np.array([n_cand, n_intra], np.uint32), cut


def apply(ans, prev, w, q, P=0):
    """one pair's unfiltered answer (flow_from's dict) -> the answer with the test at (q, P); prev: the frame the features lie in.  q = 0:
    the answer as it is"""
    if q <= 0:
        return dict(ans, counts=None, cut=False, activity=None)
    H, W = prev.shape
    slots = ans["slots"].copy()
    A = np.zeros(len(slots), np.uint32)
    for k, s in enumerate(slots):
        if int(s[5]) in CANDIDATES:
            A[k] = activity_point(prev, int(s[0]), int(s[1]), w)[0]
    quads = np.stack([slots[:, 3], slots[:, 4], ans["residuals"], slots[:, 5]], 1)
    st, counts, cut = verdict(quads, A, q, P)
    slots[:, 5] = st
    rec = [record(int(s[0]), int(s[1]), int(s[3]), int(s[4]), W, H) for s in slots if s[5] == ST_KEPT]
    records = np.array(rec, np.float32).reshape(-1, 4)
    return dict(ans, slots=slots, records=records, count=len(records), counts=counts, cut=cut, activity=A)


def flow_from(prev, cur, levels, w, iters, prev_slots=None, q=0, P=0, **kw):
    """ofps_hip_klt_flow_from with the context's intra ratio q and cut P; kw: indep_klt_pred.flow_from's settings"""
    return apply(ip.flow_from(prev, cur, levels, w, iters, prev_slots, **kw), prev, w, q, P)


def flow_chain(frames, levels, w, iters, q=0, P=0, predict_on=True, **kw):
    """the pairs (frames[k], frames[k + 1]) in order, each started from the FILTERED slots of the one before"""
    out, prev_slots = [], None
    for a, b in zip(frames[:-1], frames[1:]):
        out.append(flow_from(a, b, levels, w, iters, prev_slots if predict_on else None, q, P, **kw))
        prev_slots = out[-1]["slots"]
    return out


def flow_batch(frames, levels, w, iters, ref_mode=0, q=0, P=0, chained=False, prev_slots=None, **kw):
    """the items of a sequence (indep_klt_batch_pred.pairs_of); chained: item k starts from item k - 1's FILTERED slots"""
    out = []
    for a, b in ibp.pairs_of(frames, ref_mode):
        out.append(flow_from(a, b, levels, w, iters, prev_slots if chained else None, q, P, **kw))
        prev_slots = out[-1]["slots"]
    return out
