"""-m gpu: the island tracks (include/ofps_hip.h A5t) in the layers above the C ABI: the Python plugin's and the C++ host detector's
"Max tracks", "Track reach" and "Track gap" properties and the tool's --islands-csv columns.  Expectations come from the restatement
tests/indep_island_tracks.py."""
import csv
import io
import json
import subprocess

import numpy as np
import pytest

import indep_island_tracks as indep
import island_track_cases as tc
from ofps_amd import build as hip_build
from ofps_amd import mvec

pytestmark = pytest.mark.gpu
TOOL = hip_build.TOOL
DET = {k: tc.FUSED[k] for k in ("min_size", "subdivide", "target_motion")}
K, T, REACH, GAP = 4, 4, 1, 2


def _records():
    """the oracle's vectors of the fused frames: an empty first frame, then nine pairs"""
    import oracle
    f = tc.frames()
    return [np.zeros((0, 4), np.float32)] + [np.asarray(oracle.sad_flow(f[k - 1], f[k], tc.BLOCK, tc.RANGE)[0], np.float32) for k in range(1, tc.N_FUSED)]


def test_python_plugin_tracks():
    from ofps_amd.plugins import HipBlockMotionDetection
    det = HipBlockMotionDetection()
    assert len(det.props()) == 3 and det.tracks() is None
    assert det.set_prop("Max islands", K)
    assert det.ext_props() == [("Max islands", "usize", K, 0, 256), ("Max tracks", "usize", 0, 0, 256), ("Track reach", "usize", 1, 0, 4),
                               ("Track gap", "usize", 2, 0, 255)]
    assert len(det.props()) == 3, "props() stays the reference's surface"
    det.min_size, det.subdivide, det.target_motion = DET["min_size"], DET["subdivide"], DET["target_motion"]
    rec = _records()
    det.detect_motion(rec[1])
    assert det.tracks() is None, "Max tracks 0: no tracks"
    assert det.set_prop("Max tracks", T) and det.set_prop("Track reach", REACH) and det.set_prop("Track gap", 300) and det.track_gap == 255
    det.set_prop("Track gap", GAP)
    want, _ = indep.run(rec[1:], DET, K, T, REACH, GAP)
    for e, w in zip(rec[1:], want):
        det.detect_motion(e)
        trk = det.tracks()
        assert [trk["rows"], trk["n_tracked"], trk["n_live"], trk["t"]] == w[3].tolist()
        np.testing.assert_array_equal(trk["table"], w[4])
        np.testing.assert_array_equal(det.last_islands, w[1])
        mean = det.ctx.track_motion(trk, det.last_islands[:, 1])
        sx, sy = indep.sums_of(w[4])
        np.testing.assert_allclose(mean[:, 0], sx / w[1][:trk["rows"], 1] / 2.0 ** 24)
    # a changed property starts the tracker anew
    det.set_prop("Track reach", REACH + 1)
    det.detect_motion(rec[1])
    assert det.tracks()["t"] == 1
    det.ctx.close()


def _config(clip, max_tracks):
    props = {"Min size": {"Float": {"val": DET["min_size"], "min": 0.01, "max": 1.0}},
             "Subdivisions": {"Usize": {"val": DET["subdivide"], "min": 1, "max": 16}},
             "Target motion": {"Float": {"val": DET["target_motion"], "min": 0.0001, "max": 0.1}},
             "Max islands": {"Usize": {"val": K, "min": 0, "max": 256}},
             "Max tracks": {"Usize": {"val": max_tracks, "min": 0, "max": 256}},
             "Track reach": {"Usize": {"val": REACH, "min": 0, "max": 4}},
             "Track gap": {"Usize": {"val": GAP, "min": 0, "max": 255}}}
    cfg = {"decoder": [{"selected_plugin": "mvec", "arg": "@ARG@", "extra": False}, True],
           "detector": [{"selected_plugin": "hip_block_motion", "arg": "", "extra": None}, True],
           "settings": {"worker": {"decoder_properties": {}, "realtime_processing": False, "detector_properties": props},
                        "overlay_mf": False, "max_frame_gap": 3, "min_frames": 1,
                        "draw_perf_stats": {"summary_window": False, "graph_window": False}}}
    return json.dumps(cfg).replace("@ARG@", str(clip))


def test_tool_islands_csv_with_tracks(tmp_path):
    if not hip_build.os.path.exists(TOOL):
        hip_build.build_host()
    rec = _records()
    buf = io.BytesIO()
    for fr in rec:
        mvec.write_frame(buf, fr)
    clip = tmp_path / "clip.mvec"
    clip.write_bytes(buf.getvalue())
    cfg = tmp_path / "cfg.json"
    cfg.write_text(_config(clip, T))
    out = tmp_path / "islands.csv"
    p = subprocess.run([TOOL, "detect", "--config", str(cfg), "--islands-csv", str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["frames"] == tc.N_FUSED and res["detector_properties"]["Max tracks"] == T and res["detector_properties"]["Track gap"] == GAP
    rows = list(csv.reader(out.open()))
    assert rows[0] == ["frame", "rank", "seed", "area", "x0", "y0", "x1", "y1", "cx", "cy", "id", "age", "hits", "mx", "my"]
    # the host's detector steps on every frame it is handed, the empty first one included
    want = []
    got_frames, _ = indep.run(rec, DET, K, T, REACH, GAP)
    for k, w in enumerate(got_frames):
        sx, sy = indep.sums_of(w[4])
        for r in range(int(w[0][3])):
            tr = w[4][r] if r < w[3][0] else [0, -1, 0, 0]
            area = int(w[1][r, 1])
            want.append(([k, r] + w[1][r, :6].tolist(), [int(tr[0]), int(tr[2]), int(tr[3])],
                         [int(sx[r]) / area / 2.0 ** 24 if r < w[3][0] else 0.0, int(sy[r]) / area / 2.0 ** 24 if r < w[3][0] else 0.0]))
    assert len(rows) - 1 == len(want) >= 12
    for got, (isl, trk, mean) in zip(rows[1:], want):
        assert [int(v) for v in got[:8]] == isl and [int(v) for v in got[10:13]] == trk, got
        assert abs(float(got[13]) - mean[0]) < 1e-7 and abs(float(got[14]) - mean[1]) < 1e-7
    ids = sorted({int(r[10]) for r in rows[1:]})
    assert ids == [1, 2, 3], "two tracks, and a third id after the crossing"
    # "Max tracks" 0: the columns of the island list alone
    cfg.write_text(_config(clip, 0))
    p = subprocess.run([TOOL, "detect", "--config", str(cfg), "--islands-csv", str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert list(csv.reader(out.open()))[0] == ["frame", "rank", "seed", "area", "x0", "y0", "x1", "y1", "cx", "cy"]
