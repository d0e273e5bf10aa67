#!/usr/bin/env python3
"""Device time of the island tracks' step (include/ofps_hip.h A5t) beside the islands step, with the harness and protocol of
tools/detect_islands_time.py: one sample is 200 calls back to back between two HIP events on the context's stream, divided by 200 -- the
time per call of a saturated queue, launch overhead included, not a kernel time; median of 7 samples behind 2 warm-up samples, every sample
kept.  The tracker's inputs (counts, table, labels, the densified field) are made once by ofps_hip_detect_islands_dev and ofps_hip_densify_dev;
a call is ofps_hip_track_islands_dev alone, one item, on a state that has seen the same frame before (every island over its own footprint).
The islands step of the same grid is measured beside it as detect_islands_time.py does: densify + islands_kernel minus densify alone.
  dim 14   8,040 records (a 1080p frame's 16 x 16 blocks), the plugin's default grid, K = 16, T = 16, reach 1
  dim 160  the 6,400-island lattice, K = 6400, T = 256, reach 1
  dim 160  one island covering the grid, K = 16, T = 16, reach 4 (the atomics' worst case) and reach 0
  python tools/island_tracks_time.py [--out run.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import detect_islands_time as dit  # noqa: E402
from ofps_amd.runtime import HipContext  # noqa: E402

TARGET = dit.TARGET


def samples_ms(ctx, call, reps=7, warm=2, burst=dit.BURST):
    ts = []
    for it in range(warm + reps):
        ctx.sync(); ctx.timer_start()
        for _ in range(burst):
            call()
        ms = ctx.timer_stop() / burst
        if it >= warm:
            ts.append(round(ms, 5))
    row = dit._row(ts)
    row["samples_ms"] = ts
    return row


def full_records(d):
    e = dit.lattice_records(d)
    e[:, 2] = 0.01
    return e


def rows(ctx, name, e, min_size, subdivide, K, T, reaches, gap=2):
    d = ctx.block_dim(min_size, subdivide)
    n = e.shape[0]
    d_ent = torch.from_numpy(e.reshape(-1)).cuda()
    d_cells = torch.zeros(2 * d * d, dtype=torch.float32, device="cuda")
    d_fld = torch.zeros(2 * d * d, dtype=torch.float32, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_tab = torch.zeros(8 * K, dtype=torch.int32, device="cuda")
    d_lab = torch.zeros(d * d, dtype=torch.int16, device="cuda")
    d_tc = torch.zeros(4, dtype=torch.int32, device="cuda")
    d_rows = torch.zeros(8 * T, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out = {"dim": d, "records": n, "K": K, "T": T}
    out["densify"] = samples_ms(ctx, lambda: ctx.densify_dev(d_ent.data_ptr(), n, 1, d, d, d_cells.data_ptr()))
    out["densify_islands"] = samples_ms(ctx, lambda: ctx.detect_islands_dev(d_ent.data_ptr(), n, 1, min_size, subdivide, TARGET, K, d_cnt.data_ptr(),
                                                                            d_tab.data_ptr(), d_lab.data_ptr(), d_fld.data_ptr()))
    out["islands_step_us"] = round((out["densify_islands"]["median_ms"] - out["densify"]["median_ms"]) * 1e3, 2)
    ctx.sync()
    out["counts"] = d_cnt.cpu().numpy().tolist()
    for reach in reaches:
        d_state = torch.zeros(ctx.island_tracker_bytes(d, T), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        row = samples_ms(ctx, lambda: ctx.track_islands_dev(d_cnt.data_ptr(), d_tab.data_ptr(), d_lab.data_ptr(), d_cells.data_ptr(), d, K, 1, T, reach, gap,
                                                            d_state.data_ptr(), d_tc.data_ptr(), d_rows.data_ptr()))
        ctx.sync()
        row["tracks_step_us"] = round(row["median_ms"] * 1e3, 2)
        row["track_counts"] = d_tc.cpu().numpy().tolist()
        out[f"tracks_reach{reach}"] = row
    return {name: out}


def main():
    ctx = HipContext(0)
    res = {}
    rng = np.random.default_rng(5)
    e14 = np.empty((8040, 4), np.float32)
    e14[:, :2] = rng.uniform(0.001, 0.999, (8040, 2))
    e14[:, 2:] = rng.normal(0.003, 0.002, (8040, 2))
    unit = float(np.float32(1.0 / 160 ** 2))
    res.update(rows(ctx, "dim14_8040_records", e14, 0.05, 3, 16, 16, (1,)))
    res.update(rows(ctx, "dim160_lattice_6400_islands", dit.lattice_records(160), unit, 1, 6400, 256, (1,)))
    res.update(rows(ctx, "dim160_one_island", full_records(160), unit, 1, 16, 16, (4, 0)))
    text = json.dumps(res, indent=1)
    print(text)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
