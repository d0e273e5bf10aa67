"""hip_klt's chained batch (include/ofps_hip.h, row N3pb) restated on top of tests/indep_klt_pred.py's flow_from: the items of a frame sequence
in order, each started from the guesses the predictor makes from the slots of the item before, the first from the caller's slots or from
zero.  Written from the header's text.  No code is shared with the library.  Test infrastructure only."""
import indep_klt_pred as ip


def pairs_of(frames, ref_mode):
    """item k of a sequence: (k, k + 1) with ref_mode 0, (0, k + 1) with ref_mode 1"""
    if ref_mode not in (0, 1):
        raise ValueError(ref_mode)
    return [(frames[0] if ref_mode else frames[k], frames[k + 1]) for k in range(len(frames) - 1)]


def flow_batch_from(frames, levels, w, iters, ref_mode=0, prev_slots=None, chained=True, **kw):
    """-> the list of flow_from's answers, one per item.  chained False: every item from zero (the batch form without the row)"""
    out = []
    for a, b in pairs_of(frames, ref_mode):
        out.append(ip.flow_from(a, b, levels, w, iters, prev_slots if chained else None, **kw))
        prev_slots = out[-1]["slots"]
    return out
