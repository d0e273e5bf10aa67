"""The case generator of the hip_sad property sweeps (tests/test_sad_qpel_cpu.py on the CPU, tests/test_sad_qpel_properties_gpu.py
on the GPU): geometries over the whole accepted block / range domain, frames down to 1x1, five kinds of content.

One strategy, one list of explicit corners and one fixed seed, so the CPU test and the GPU tests walk the same examples; the
coverage conditions (coverage()) are computed from the CPU chain's output alone and asserted by both, so neither sweep can pass
on inputs that never reach the places it is there for."""
import numpy as np
from hypothesis import HealthCheck, example, given, seed, settings, strategies as st

import indep_sad_qpel as iq

BLOCKS = [1, 2, 3, 4, 5, 7, 8, 12, 16, 24, 32, 48, 64]
RANGES = [0, 1, 3, 4, 8, 16, 20, 32, 33, 48, 64]
KINDS = ["noise", "binary", "coarse", "flat", "subpel"]
MAX_EXAMPLES = 150

# corners that must not depend on the draw: (w, h, b, r), each with binary and noise content
CORNERS = [(64, 64, 64, 64),       # one block of the largest size at the largest range: 20-bit SADs, the largest LDS footprint
           (130, 70, 64, 64),
           (1, 1, 1, 0),           # one sample: f = 0 is the only valid candidate
           (3, 2, 1, 3),
           (7, 5, 2, 4),
           (9, 9, 3, 64),          # range far beyond the frame
           (20, 9, 8, 0),          # range 0 at scale 4: a pure sub-pel search; H < B + 6
           (16, 16, 16, 16),       # W == B == H: one block, the window clamps on all four sides
           (21, 21, 16, 48),
           (150, 100, 16, 48),     # generic search + templated refinement at a large range
           (150, 100, 8, 64),
           (150, 100, 4, 4),       # thousands of winners on noise: the rounding constants of b, h and j each decide some of them
           (149, 99, 5, 8),
           (68, 98, 5, 64)]        # like (150, 100, 8, 64): winners with Dy + 4R + 3 >= 512, the tenth bit of the key's Dy field


@st.composite
def cases(draw):
    """-> (w, h, b, r, seed, kind).  The block is drawn first; for three quarters of the mass the frame is then drawn to hold at least one
    block (with w <= 150 and h <= 100 a free draw leaves nearly every block above 32 with an empty grid), for the last quarter it is
    free, so empty grids and frames narrower than a block stay in."""
    b, r = draw(st.sampled_from(BLOCKS)), draw(st.sampled_from(RANGES))
    lo = b if draw(st.integers(0, 3)) else 1
    w, h = draw(st.integers(lo, 150)), draw(st.integers(lo, 100))
    # flat frames cannot have a fractional winner: they get a tenth of the mass, the other four kinds share the rest
    kind = "flat" if draw(st.integers(0, 9)) == 9 else draw(st.sampled_from([k for k in KINDS if k != "flat"]))
    return (w, h, b, r, draw(st.integers(0, 2**31 - 1)), kind)


def sweep(fn):
    """@given over cases() + the corners, derandomised with one fixed seed (derandomize alone seeds from the test function, and
    the CPU and GPU sweeps are different functions).  The test takes the case as its argument `case`."""
    for k, (w, h, b, r) in enumerate(reversed(CORNERS)):
        for kind in ("noise", "binary"):
            fn = example(case=(w, h, b, r, 1000 + k, kind))(fn)
    fn = given(case=cases())(fn)
    fn = seed(20261016)(fn)
    return settings(max_examples=MAX_EXAMPLES, deadline=None, derandomize=True, database=None,
                    suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow, HealthCheck.data_too_large])(fn)


def frames(w, h, b, r, seed, kind):
    """-> uint8 [2, h, w]: previous and current frame"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        fr = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    elif kind == "binary":                                   # saturated two-level content: every six-tap sum near a clip limit
        fr = (rng.integers(0, 2, (2, h, w), dtype=np.uint8) * 255).astype(np.uint8)
    elif kind == "coarse":                                   # 4-level content shifted by a random vector inside the range
        base = (rng.integers(0, 4, (h + 128, w + 128), dtype=np.uint8) * 64).astype(np.uint8)
        dx, dy = int(rng.integers(-r, r + 1)), int(rng.integers(-r, r + 1))
        fr = np.stack([base[64:64 + h, 64:64 + w], base[64 + dy:64 + dy + h, 64 + dx:64 + dx + w]])
    elif kind == "flat":
        fr = np.full((2, h, w), int(rng.integers(0, 256)), np.uint8)
    else:                                                    # subpel: frame 1 = frame 0 rendered a random quarter-pel offset away, + noise
        cells = rng.integers(0, 256, ((h + 3) // 4 + 1, (w + 3) // 4 + 1)).astype(np.int32)
        prev = np.repeat(np.repeat(cells, 4, axis=0), 4, axis=1)[:h, :w] // 2 + rng.integers(0, 128, (h, w))
        prev = prev.astype(np.uint8)
        q = iq.quarter_plane(prev)
        m = min(4 * r + 3, 11)
        Dx, Dy = int(rng.integers(-m, m + 1)), int(rng.integers(-m, m + 1))
        Y, X = np.mgrid[0:h, 0:w]
        cur = q[np.clip(4 * Y + Dy, 0, q.shape[0] - 1), np.clip(4 * X + Dx, 0, q.shape[1] - 1)].astype(np.int32)
        cur += rng.integers(-2, 3, cur.shape)
        fr = np.stack([prev, np.clip(cur, 0, 255).astype(np.uint8)])
    return np.ascontiguousarray(fr)


def observe(case, best_q, n_valid):
    """what coverage() needs of one example: from the case and the restatement's winners (Dx, Dy, SAD) / valid-candidate counts"""
    w, h, b, r, _, kind = case
    frac = ((np.asarray(best_q)[:, :2] % 4) != 0).any(axis=1) if len(best_q) else np.zeros(0, bool)
    return dict(w=w, h=h, b=b, r=r, kind=kind, blocks=len(best_q), frac_blocks=int(frac.sum()), clipped_blocks=int((np.asarray(n_valid) < 49).sum()))


def coverage(obs, verbose=True):
    """The coverage conditions of the sweep over a whole run; -> the measured values.  Conditions on the inputs, not measurements:
    a sweep that meets them has run the large and the tiny blocks, the ranges past the strip table, frames smaller than the
    refinement's window, fractional winners and clipped candidate sets.  The counts are over examples that have blocks."""
    n = len(obs)
    nonempty = [o for o in obs if o["blocks"]]
    blocks = sum(o["blocks"] for o in obs)
    got = {
        "examples": n,
        "nonempty_share": len(nonempty) / n,
        "frac_example_share": sum(o["frac_blocks"] > 0 for o in obs) / n,
        "frac_block_share": sum(o["frac_blocks"] for o in obs) / max(blocks, 1),
        "clipped_example_share": sum(o["clipped_blocks"] > 0 for o in obs) / n,
        "small_frames": sum(o["w"] < o["b"] + 6 or o["h"] < o["b"] + 6 for o in nonempty),
        "b_ge_48": sum(o["b"] >= 48 for o in nonempty),
        "r_ge_33": sum(o["r"] >= 33 for o in nonempty),
        "b_le_3": sum(o["b"] <= 3 for o in nonempty),
    }
    if verbose:
        print("[sad_qpel sweep coverage] " + "  ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in got.items()))
    assert got["nonempty_share"] >= 0.50, got
    assert got["frac_example_share"] >= 0.40 and got["frac_block_share"] >= 0.10, got
    assert got["clipped_example_share"] >= 0.50, got
    assert got["small_frames"] >= 15, got
    assert got["b_ge_48"] >= 5 and got["r_ge_33"] >= 5 and got["b_le_3"] >= 5, got
    return got
