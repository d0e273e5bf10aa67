"""-m gpu: the island list (include/ofps_hip.h A5i) in the layers above the C ABI: the Python plugin's and the C++ host detector's
"Max islands" property and the tool's --islands-csv.  Expectations come from the restatement tests/indep_detect_islands.py."""
import csv
import io
import json
import subprocess

import numpy as np
import pytest

import detect_islands_cases as ic
import indep_detect_islands as indep
from ofps_amd import build as hip_build
from ofps_amd import mvec

pytestmark = pytest.mark.gpu
TOOL = hip_build.TOOL


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_python_plugin_max_islands():
    from ofps_amd.plugins import HipBlockMotionDetection
    det = HipBlockMotionDetection()
    assert det.ext_props() == [("Max islands", "usize", 0, 0, 256)] and len(det.props()) == 3
    c = ic.BY_NAME["k1024_blocks-64-a2"]
    e, prm = c.make(), c.params
    det.min_size, det.subdivide, det.target_motion = prm["min_size"], prm["subdivide"], prm["target_motion"]
    plain = det.detect_motion(e)                                          # 0: what it calls today
    assert det.last_islands is None
    ref = ic.reference(e, prm)
    assert det.set_prop("Max islands", 2) and det.max_islands == 2
    counts, table, labels, field = indep.listed(ref, 2)
    area, mf = det.detect_motion(e)
    assert area == table[0, 1] == plain[0]
    np.testing.assert_array_equal(det.last_islands, table)
    np.testing.assert_array_equal(_bits(mf.vf), _bits(field))      # the union of both islands
    nothing = ic.BY_NAME["lattice-17-a2"]                                 # components, no island
    det.min_size, det.subdivide = nothing.params["min_size"], nothing.params["subdivide"]
    assert det.detect_motion(nothing.make()) is None and det.last_islands.shape == (0, 8)
    det.ctx.close()


def _config(clip, max_islands):
    """a saved MotionDetectionConfig as serde writes it (tests/test_host_layer.py: SAVED_CONFIG)"""
    props = {"Min size": {"Float": {"val": ic.FUSED["min_size"], "min": 0.01, "max": 1.0}},
             "Subdivisions": {"Usize": {"val": ic.FUSED["subdivide"], "min": 1, "max": 16}},
             "Target motion": {"Float": {"val": ic.FUSED["target_motion"], "min": 0.0001, "max": 0.1}}}
    cfg = {"decoder": [{"selected_plugin": "mvec", "arg": "@ARG@", "extra": False}, True],
           "detector": [{"selected_plugin": "hip_block_motion", "arg": "", "extra": None}, True],
           "settings": {"worker": {"decoder_properties": {}, "realtime_processing": False, "detector_properties": props},
                        "overlay_mf": False, "max_frame_gap": 3, "min_frames": 1,
                        "draw_perf_stats": {"summary_window": False, "graph_window": False}}}
    if max_islands is not None:
        props["Max islands"] = {"Usize": {"val": max_islands, "min": 0, "max": 256}}
    return json.dumps(cfg).replace("@ARG@", str(clip))


def test_tool_islands_csv(tmp_path):
    import oracle
    if not hip_build.os.path.exists(TOOL):
        hip_build.build_host()
    f = ic.frames()
    frames = [np.zeros((0, 4), np.float32)] + [oracle.sad_flow(f[k - 1], f[k], ic.BLOCK, ic.RANGE)[0] for k in range(1, 4)]
    buf = io.BytesIO()
    for fr in frames:
        mvec.write_frame(buf, fr)
    clip = tmp_path / "clip.mvec"
    clip.write_bytes(buf.getvalue())
    cfg = tmp_path / "cfg.json"
    cfg.write_text(_config(clip, 4))
    out = tmp_path / "islands.csv"
    p = subprocess.run([TOOL, "detect", "--config", str(cfg), "--islands-csv", str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["frames"] == 4 and res["detector_properties"]["Max islands"] == 4
    rows = list(csv.reader(out.open()))
    assert rows[0] == ["frame", "rank", "seed", "area", "x0", "y0", "x1", "y1", "cx", "cy"]
    want = []
    det = {k: ic.FUSED[k] for k in ("min_size", "subdivide", "target_motion")}
    for k, e in enumerate(frames):
        isl = indep.islands(e, **det)
        for r, row in enumerate(isl.table[:4]):
            want.append([k, r] + row[:6].tolist() + [(row[6] / row[1] + 0.5) / isl.dim, (row[7] / row[1] + 0.5) / isl.dim])
    assert len(rows) - 1 == len(want) >= 6                                # two islands in each of three frames
    for got, w in zip(rows[1:], want):
        assert [int(v) for v in got[:8]] == w[:8]
        assert abs(float(got[8]) - w[8]) < 1e-6 and abs(float(got[9]) - w[9]) < 1e-6
    # "Max islands" 0 or absent: refused
    for k in (0, None):
        cfg.write_text(_config(clip, k))
        p = subprocess.run([TOOL, "detect", "--config", str(cfg), "--islands-csv", str(out)], capture_output=True, text=True)
        assert p.returncode != 0 and "Max islands" in p.stderr
