#!/usr/bin/env python3
"""The program for a `rocprofv3 --kernel-trace` listing of hip_sad's host paths, and the bytes they return: for a change that must move
neither.  The four 320 x 192 frames of tests/sad_gate_cases.py, block 16, range 8, detector + least-squares estimator:
  push      four ofps_hip_push_frame calls with all criteria off, gate 1, limit 1, median 2, and all three with motion scale 4 + levels 2 +
            mean removal 4;
  batch     the same frames as one ofps_hip_push_frames_async ticket, batch filter switch on, all three criteria;
  stream    the batched stream cut 1 + 2 + 1 (the buffers grow, the previous frame is parked): plain, one ticket at a time and two in flight;
            batch filter switch on with all three criteria plus intra 8 / cut 50;
  multi     one MultiDevice([0]) stream of two batches of two, the workers' halo mode;
  sad_flow  ofps_hip_sad_flow on frames 1 and 2 under gate 1, limit 1, median 2, intra 8 and split 16, each alone;
  filtered  ofps_hip_sad_flow_filtered_dev with all three criteria in both ref_modes.
Prints one line per case with the SHA-256 of everything the case returned; --out writes the lines to a file.
  rocprofv3 --kernel-trace [--memory-copy-trace] --output-format csv [json] -d <dir> -- python tools/sad_dispatch_driver.py [--lib <libofps_hip.so>] [--out <file>]
  python tools/sad_dispatch_driver.py --list <dir>      the (kernel name, grid, workgroup) of every launch under <dir> in dispatch order, the
                                                        `_items_kernel` forms of an older build named as their one-pair kernels; then, when the
                                                        run traced them, the runtime's copies in start order, by direction and size"""
import csv
import glob
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def listing(directory):
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("(anonymous namespace)::", "")).replace("void ", "")
        for step in ("block_contrast", "sad_consistency", "sad_median"):
            name = name.replace(step + "_items_kernel", step + "_kernel")
        print(f"{name:44s} grid {r['Grid_Size_X']:>8s} {r['Grid_Size_Y']:>5s} {r['Grid_Size_Z']:>5s}  wg {r['Workgroup_Size_X']:>4s}")
    # --memory-copy-trace: the copies the runtime's engines made, in start order, by direction and size.  The CSV has no size column; the
    # JSON output of the same run (--output-format csv json) has, in records that carry "bytes" beside their timestamps
    sizes = {}
    for f in glob.glob(os.path.join(directory, "**", "*results.json"), recursive=True):
        def walk(node):
            if isinstance(node, dict):
                if "bytes" in node and "start_timestamp" in node:
                    sizes[int(node["start_timestamp"])] = int(node["bytes"])
                for v in node.values():
                    walk(v)
            elif isinstance(node, list):
                for v in node:
                    walk(v)
        walk(json.load(open(f)))
    copies = []
    for f in glob.glob(os.path.join(directory, "**", "*memory_copy_trace.csv"), recursive=True):
        copies += list(csv.DictReader(open(f)))
    copies.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in copies:
        print(f"copy {r['Direction'].replace('MEMORY_COPY_', ''):44s} bytes {sizes.get(int(r['Start_Timestamp']), '?')}")


def main():
    if "--list" in sys.argv:
        return listing(sys.argv[sys.argv.index("--list") + 1])
    if "--lib" in sys.argv:
        from ofps_amd import _lib
        _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    import numpy as np
    import torch

    import sad_gate_cases as gc
    from ofps_amd.runtime import HipContext

    f = np.ascontiguousarray(gc.frames())
    n, H, W = f.shape
    B, R, NBLK = gc.BLOCK, gc.RANGE, gc.NBLK
    prm = dict(block=B, search_range=R, aspect=gc.FRAME_CAM[0], fov_y_deg=gc.FRAME_CAM[1], seed=gc.SEED, **gc.FRAME_DETECTOR)
    ctx = HipContext(0)
    lines = []

    def done(case, parts):
        h = hashlib.sha256()
        for p in parts:
            h.update(np.ascontiguousarray(p).tobytes())
        lines.append(f"{case:28s} {h.hexdigest()}")

    def result_bytes(r, entries):
        area = -1 if r["motion"] is None else r["motion"][0]
        return [np.array([r["have_vectors"], r["n_vectors"], area], np.int64), r["quat"], entries[:r["n_vectors"]] if r["have_vectors"] else np.zeros(0)]

    def settings(gate=0, limit=0, median=0, scale=1, levels=1, prefilter=0, batch_filter=0):
        ctx.set_sad_gate(gate); ctx.set_sad_consistency(limit); ctx.set_sad_median(median); ctx.set_sad_motion_scale(scale)
        ctx.set_sad_levels(levels); ctx.set_sad_prefilter(prefilter); ctx.set_sad_batch_filter(batch_filter)

    for case, kw in (("push off", {}), ("push gate1", dict(gate=1)), ("push limit1", dict(limit=1)), ("push median2", dict(median=2)),
                     ("push all scale4 levels2 pre4", dict(gate=1, limit=1, median=2, scale=4, levels=2, prefilter=4))):
        settings(**kw)
        ctx.reset_frames()
        parts = []
        for frame in f:
            r = ctx.push_frame(frame, want_entries=True, **prm)
            parts += result_bytes(r, r["entries"] if r["entries"] is not None else np.zeros(0))
        done(case, parts)

    settings(gate=1, limit=1, median=2, batch_filter=1)
    ctx.reset_frames()
    buf, ent = ctx.pinned_array((n, H, W), np.uint8), ctx.pinned_array((n, NBLK, 4))
    np.copyto(buf, f); ent[:] = 0
    res = ctx.frames_wait(ctx.push_frames_async(buf, out_entries=ent, **prm))
    done("batch all three", [p for j, r in enumerate(res) for p in result_bytes(r, ent[j])])
    ctx.reset_frames()
    ctx.free_pinned(buf); ctx.free_pinned(ent)
    settings()

    # the batched stream cut 1 + 2 + 1: the batch buffers grow at the second ticket and the stream's previous frame is parked
    def stream(pusher, sizes, in_flight):
        parts, pending, start = [], [], 0

        def collect():
            t, e, _ = pending.pop(0)
            for j, r in enumerate(pusher.frames_wait(t)):
                parts.extend(result_bytes(r, e[j]))
        for size in sizes:
            if len(pending) >= in_flight:
                collect()
            batch, e = np.ascontiguousarray(f[start:start + size]), np.zeros((size, NBLK, 4), np.float32)
            pending.append((pusher.push_frames_async(batch, out_entries=e, **dict(prm, seed=gc.SEED + start)), e, batch))
            start += size
        while pending:
            collect()
        pusher.reset_frames()
        return parts

    done("stream 1+2+1 plain", stream(ctx, (1, 2, 1), 1))
    done("stream 1+2+1 plain in flight", stream(ctx, (1, 2, 1), 2))
    settings(gate=1, limit=1, median=2, batch_filter=1)
    ctx.set_sad_intra(8); ctx.set_sad_cut(50)
    done("stream 1+2+1 all intra8 cut50", stream(ctx, (1, 2, 1), 1))
    ctx.set_sad_intra(0); ctx.set_sad_cut(0)
    settings()
    # the multi-device workers' pushes (halo mode).  ONE worker, so that the listing is deterministic: two workers' launches interleave as
    # their threads run
    from ofps_amd.runtime import MultiDevice
    md = MultiDevice([0])
    done("multi one worker 2+2", stream(md, (2, 2), 2))
    md.close()

    # ofps_hip_sad_flow with the context's criteria, one at a time, and under split
    for case, apply in (("gate1", lambda v: ctx.set_sad_gate(v and 1)), ("limit1", lambda v: ctx.set_sad_consistency(v and 1)),
                        ("median2", lambda v: ctx.set_sad_median(v and 2)), ("intra8", lambda v: ctx.set_sad_intra(v and 8)),
                        ("split16", lambda v: ctx.set_sad_split(v and 16))):
        apply(1)
        done(f"sad_flow {case}", list(ctx.sad_flow(f[1], f[2], B, R, want_best=True)))
        apply(0)

    d_frames = torch.from_numpy(f).cuda()
    for ref_mode in (0, 1):
        d_ent = torch.zeros(((n - 1) * NBLK, 4), dtype=torch.float32, device="cuda")
        d_best = torch.zeros(((n - 1) * NBLK, 3), dtype=torch.int32, device="cuda")
        d_cnt = torch.zeros((n - 1,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.sad_flow_filtered_dev(d_frames.data_ptr(), n, W, H, W, W * H, ref_mode, B, R, 1, 1, 2, d_ent.data_ptr(), d_best.data_ptr(), d_cnt.data_ptr())
        ctx.sync()
        cnt = d_cnt.cpu().numpy()
        ent_h, best_h = d_ent.cpu().numpy().reshape(n - 1, NBLK, 4), d_best.cpu().numpy().reshape(n - 1, NBLK, 3)
        done(f"filtered ref_mode {ref_mode}", [cnt] + [a[k, :cnt[k]] for k in range(n - 1) for a in (ent_h, best_h)])
    ctx.close()
    print("\n".join(lines))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
