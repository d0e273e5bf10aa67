#!/usr/bin/env python3
"""The program for a `rocprofv3 --kernel-trace` listing of hip_klt's host paths, and the bytes they return: for a change that must move
neither.  Frames of 128 x 96 (tests/klt_batch_cases.py, tests/klt_intra_cases.py), levels 2, radius 4, 10 iterations, cell 16, under the
settings off / N3m / N3f 64 / N3m + N3f / intra 8 with cut 50:
  pair      ofps_hip_klt_flow_dev, _flow_from_dev, _track_dev, _track_q_dev and _track_from_dev on the repainted pair (intra: and the cut pair);
  batch     ofps_hip_klt_flow_batch_dev in both ref_modes, and _flow_batch_from_dev with and without d_prev_slots, on the six-frame sequence
            (intra: the four frames around a cut);
  host      ofps_hip_klt_flow, _flow_from, _flow_batch and _flow_batch_from, settings off and N3m + N3f;
  stream    six fused sparse calls of the dense decoders' stream with prediction on, and the batched stream at KLT cut into two tickets with
            both prediction settings on.
Prints one line per case with the SHA-256 of everything the case returned; --out writes the lines to a file.
  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/klt_dispatch_driver.py [--lib <libofps_hip.so>] [--out <file>]
  python tools/klt_dispatch_driver.py --list <dir>      the (kernel name, grid, workgroup) of every launch under <dir> in dispatch order"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

from sad_dispatch_driver import listing

L, W_, K = 2, 4, 10                                          # levels, radius, iterations
SETTINGS = (("off", 0, 0, 0, 0), ("n3m", 1, 0, 0, 0), ("n3f64", 0, 64, 0, 0), ("n3m n3f64", 1, 64, 0, 0), ("intra8 cut50", 0, 0, 8, 50))
SEED = 77


def main():
    if "--list" in sys.argv:
        return listing(sys.argv[sys.argv.index("--list") + 1])
    if "--lib" in sys.argv:
        from ofps_amd import _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import numpy as np

    import klt_batch_cases as bc
    import klt_cases as kc
    import klt_intra_cases as ic
    from ofps_amd.runtime import HipContext

    ctx = HipContext(0)
    lines = []

    def done(case, parts):
        h = hashlib.sha256()
        for p in parts:
            h.update(np.ascontiguousarray(p).tobytes())
        lines.append(f"{case:44s} {h.hexdigest()}")

    def apply(zm, fb, q, cut):
        ctx.set_klt_mean_removal(zm); ctx.set_klt_fb(fb); ctx.set_klt_intra(q); ctx.set_klt_cut(cut)

    def up(a):
        a = np.ascontiguousarray(a)
        d = ctx.malloc(a.nbytes)
        ctx.memcpy_h2d(d, a)
        return d

    def down(d, shape, dtype):
        host = np.zeros(shape, dtype)
        ctx.memcpy_d2h(host, d)
        return host

    def flow_pair(d_prev, d_cur, W, H, ns, d_prev_slots):
        d_rec, d_cnt, d_slots = up(np.zeros((ns, 4), np.float32)), up(np.zeros(1, np.uint32)), up(np.zeros((ns, 6), np.int32))
        if d_prev_slots is None:
            ctx.klt_flow_dev(d_prev, d_cur, W, H, W, L, W_, K, d_rec, d_cnt, d_slots)
        else:
            ctx.klt_flow_from_dev(d_prev, d_cur, W, H, W, L, W_, K, d_prev_slots, d_rec, d_cnt, d_slots)
        ctx.sync()
        cnt, slots = down(d_cnt, 1, np.uint32), down(d_slots, (ns, 6), np.int32)
        rec = down(d_rec, (ns, 4), np.float32)[:cnt[0]]
        for d in (d_rec, d_cnt, d_slots):
            ctx.free(d)
        return [cnt, rec, slots]

    def track(d_prev, d_cur, W, H, pts, form, guesses=None):
        n = len(pts)
        d_pts, d_out = up(pts), up(np.zeros((n, 4), np.int32))
        d_g = up(guesses) if guesses is not None else None
        if form == "q":
            ctx.klt_track_q_dev(d_prev, d_cur, W, H, W, d_pts, n, L, W_, K, d_out)
        elif form == "from":
            ctx.klt_track_from_dev(d_prev, d_cur, W, H, W, d_pts, d_g, n, L, W_, K, d_out)
        else:
            ctx.klt_track_dev(d_prev, d_cur, W, H, W, d_pts, n, L, W_, K, d_out)
        ctx.sync()
        out = down(d_out, (n, 4), np.int32)
        for d in (d_pts, d_out, d_g):
            if d is not None:
                ctx.free(d)
        return [out]

    def flow_batch(d_frames, n, W, H, ns, ref_mode, chained, d_prev_slots=None):
        pairs = n - 1
        d_rec, d_cnt, d_slots = up(np.zeros((pairs, ns, 4), np.float32)), up(np.zeros(pairs, np.uint32)), up(np.zeros((pairs, ns, 6), np.int32))
        if chained:
            ctx.klt_flow_batch_from_dev(d_frames, n, W, H, W, W * H, ref_mode, L, W_, K, d_rec, d_cnt, d_slots, d_prev_slots)
        else:
            ctx.klt_flow_batch_dev(d_frames, n, W, H, W, W * H, ref_mode, L, W_, K, d_rec, d_cnt, d_slots)
        ctx.sync()
        cnt, slots, rec = down(d_cnt, pairs, np.uint32), down(d_slots, (pairs, ns, 6), np.int32), down(d_rec, (pairs, ns, 4), np.float32)
        for d in (d_rec, d_cnt, d_slots):
            ctx.free(d)
        return [cnt, slots] + [rec[k, :cnt[k]] for k in range(pairs)]

    seq = bc.sequence(bc.SMALL)
    for name, zm, fb, q, cut in SETTINGS:
        apply(zm, fb, q, cut)
        pairs = [("repaint", kc.repaint_pair())] + ([("cut", ic.cut_pair())] if q else [])
        for pname, (prev, cur) in pairs:
            H, W = prev.shape
            ns = ctx.klt_slot_count(W, H)
            d_prev, d_cur = up(prev), up(cur)
            first = flow_pair(d_prev, d_cur, W, H, ns, None)
            done(f"pair {pname} flow_dev {name}", first)
            d_ps = up(first[2])
            done(f"pair {pname} flow_from_dev {name}", flow_pair(d_prev, d_cur, W, H, ns, d_ps))
            ctx.free(d_ps)
            pts = np.ascontiguousarray(first[2][first[2][:, 5] != 1][:, :2])
            done(f"pair {pname} track_dev {name}", track(d_prev, d_cur, W, H, pts, "pixel"))
            done(f"pair {pname} track_q_dev {name}", track(d_prev, d_cur, W, H, pts * 256 + 77, "q"))
            done(f"pair {pname} track_from_dev {name}", track(d_prev, d_cur, W, H, pts, "from", np.full_like(pts, 300)))
            ctx.free(d_prev); ctx.free(d_cur)
        frames = ic.cut_sequence() if q else seq
        n, H, W = frames.shape
        ns = ctx.klt_slot_count(W, H)
        d_frames = up(frames)
        for ref_mode in (0, 1):
            plain = flow_batch(d_frames, n, W, H, ns, ref_mode, False)
            done(f"batch ref_mode {ref_mode} {name}", plain)
            done(f"batch ref_mode {ref_mode} chained from zero {name}", flow_batch(d_frames, n, W, H, ns, ref_mode, True))
            d_ps = up(plain[1][0])
            done(f"batch ref_mode {ref_mode} chained from slots {name}", flow_batch(d_frames, n, W, H, ns, ref_mode, True, d_ps))
            ctx.free(d_ps)
        ctx.free(d_frames)

    for name, zm, fb, q, cut in (SETTINGS[0], SETTINGS[3]):
        apply(zm, fb, q, cut)
        prev, cur = kc.repaint_pair()
        ent, slots = ctx.klt_flow(prev, cur, L, W_, K, want_slots=True)
        done(f"host flow {name}", [ent, slots])
        done(f"host flow_from {name}", list(ctx.klt_flow_from(prev, cur, L, W_, K, slots)))
        ent, cnt, bslots = ctx.klt_flow_batch(seq, L, W_, K, 0, want_slots=True)
        done(f"host flow_batch {name}", [cnt, bslots] + [ent[k, :cnt[k]] for k in range(len(cnt))])
        ent, cnt, bslots = ctx.klt_flow_batch_from(seq, L, W_, K, 0, slots)
        done(f"host flow_batch_from {name}", [cnt, bslots] + [ent[k, :cnt[k]] for k in range(len(cnt))])
    apply(0, 0, 0, 0)

    def result_bytes(r, entries):
        have = r["have_vectors"]
        return [np.array([have, r["n_vectors"]], np.int64), r["quat"], entries[:r["n_vectors"]] if have else np.zeros(0)]

    ctx.set_klt_prediction(1)
    ctx.lk_reset()
    parts = []
    for j, f in enumerate(seq):
        r = ctx.lk_push_frame_fused(np.ascontiguousarray(f), L, W_, K, sparse=True, seed=SEED + j)
        parts += result_bytes(r, r["entries"] if r["have_vectors"] else None)
    done("stream fused sparse prediction", parts)
    ctx.lk_reset()

    ctx.set_klt_batch_prediction(1)
    ctx.set_batch_decoder(ctx.BATCH_DECODER_KLT, L, W_, K)
    ctx.reset_frames()
    n, H, W = seq.shape
    cap = ctx.batch_record_capacity(W, H)
    parts = []
    for start in (0, 3):
        batch = np.ascontiguousarray(seq[start:start + 3])
        ent = np.zeros((3, cap, 4), np.float32)
        for j, r in enumerate(ctx.frames_wait(ctx.push_frames_async(batch, seed=SEED + start, out_entries=ent))):
            parts += result_bytes(r, ent[j])
    done("stream batched two tickets chained", parts)
    ctx.reset_frames()
    ctx.set_batch_decoder(ctx.BATCH_DECODER_SAD)
    ctx.set_klt_prediction(0); ctx.set_klt_batch_prediction(0)
    ctx.close()
    print("\n".join(lines))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
