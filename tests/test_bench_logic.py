"""`bench.py --gpus N` launches N ranks and shards the work: the launch / sharding / gather / reduce
logic runs here under gloo with a stubbed step (`--stub`: no GPU, marked data='stub'); the GPU step itself is covered
by the -m gpu tests and by the driver's own bench runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _run(*argv, env=None, timeout=300):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "LOCAL_WORLD_SIZE"):
        e.pop(k, None)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=timeout, env=e)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, (json.loads(lines[-1]) if lines else None)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("key", [False, True])
def test_strong_plan_partitions_the_batch(world, key):
    P, G = 13, 4
    seen = []
    for r in range(world):
        pl = bench.shard_plan("strong", P, G, world, r, key)
        walk = pl["walk"]
        assert len(walk) == P + 1 and max(walk) <= G and all(abs(int(walk[i + 1]) - int(walk[i])) == 1 for i in range(P))
        seen += list(range(pl["first"], pl["first"] + pl["count"]))
        ids = pl["frame_ids"]
        if pl["count"] == 0:
            assert ids == []
            continue
        if key:      # slot 0 = key frame, then the `cur` frame of each of the rank's pairs
            assert ids == [int(walk[0])] + [int(walk[k + 1]) for k in range(pl["first"], pl["first"] + pl["count"])]
        else:        # consecutive pairs: count + 1 frames, one halo frame shared with the next rank
            assert ids == [int(walk[k]) for k in range(pl["first"], pl["first"] + pl["count"] + 1)]
        assert pl["seed_rank"] == 0
    assert seen == list(range(P))


def test_weak_plan_gives_every_rank_its_own_full_batch():
    for r in range(4):
        pl = bench.shard_plan("weak", 8, 8, 4, r, False)
        assert (pl["first"], pl["count"], pl["seed_rank"]) == (0, 8, r) and len(pl["frame_ids"]) == 9


def test_time_steps_runs_exactly_w_plus_k_steps_inside_the_brackets():
    log = []
    bench.time_steps(lambda: log.append("s"), 5, 2, lambda: log.append("y"), lambda: log.append("b"))
    assert log == ["s"] * 2 + ["y", "b", "y"] + ["s"] * 5 + ["y", "b", "y"]


def test_gpus_2_self_launches_two_ranks_strong():
    p, d = _run("--gpus", "2", "--stub", "--scaling", "strong", "--pairs", "5", "--steps", "2", "--warmup", "1", "--full")
    assert p.returncode == 0, p.stderr[-2000:]
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["scaling"] == "strong" and d["data"] == "stub"
    assert d["config"]["pairs_per_rank"] == [3, 2] and d["config"]["pairs_per_step"] == 5
    assert d["parity_check"]["ok"] is True and d["parity_check"]["gathered_checksum_of_last_pair_matches_oracle"] is True


def test_gpus_2_key_frame_broadcast_reaches_every_rank():
    p, d = _run("--gpus", "2", "--stub", "--scaling", "strong", "--pairs", "4", "--ref-mode", "key", "--steps", "1", "--warmup", "1", "--full")
    assert p.returncode == 0, p.stderr[-2000:]
    # the stubbed step folds the key frame's bytes into every pair's checksum: true only if the broadcast delivered them
    assert d["parity_check"]["gathered_checksum_of_last_pair_matches_oracle"] is True and d["ranks_seen"] == 2
    assert "broadcast" in d["config"]["parallelism"]


def test_gpus_2_weak_reports_whole_job_pairs():
    p, d = _run("--gpus", "2", "--stub", "--pairs", "6", "--steps", "1", "--warmup", "0")
    assert p.returncode == 0, p.stderr[-2000:]
    assert d["scaling"] == "weak" and d["config"]["pairs_per_rank"] == [6, 6] and d["config"]["pairs_per_step"] == 12


def test_a_skipping_rank_cannot_hide_another_ranks_mismatch_and_a_mismatch_fails_the_run():
    """Mismatches and skips are reduced separately; any mismatch makes the process exit non-zero (a driver that looks
    only at the return code and `value` must not accept wrong vectors)."""
    p, d = _run("--gpus", "2", "--stub", "--pairs", "4", "--steps", "1", "--warmup", "0", "--stub-parity", "skip,0", "--full")
    assert p.returncode != 0 and "PARITY MISMATCH" in p.stderr
    assert d["parity_check"]["ok"] is False and d["parity_check"]["ranks_skipped"] == 1 and d["parity_check"]["ranks_checked"] == 1
    p, d = _run("--gpus", "2", "--stub", "--pairs", "4", "--steps", "1", "--warmup", "0", "--stub-parity", "skip,1", "--full")
    assert p.returncode == 0 and d["parity_check"]["ok"] is True and d["parity_check"]["ranks_skipped"] == 1
    p, d = _run("--gpus", "2", "--stub", "--pairs", "4", "--steps", "1", "--warmup", "0", "--stub-parity", "skip,skip", "--full")
    assert p.returncode == 0 and d["parity_check"]["ok"] is None and d["parity_check"]["ranks_skipped"] == 2


def test_world_size_must_match_gpus():
    # a launcher that started 1 rank while --gpus says 2: fail loudly instead of measuring one GPU and printing n_gpus=1
    p, d = _run("--gpus", "2", "--stub", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode != 0 and d is None and "--gpus 2" in p.stderr


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p, d = _run("--steps", "1", "--warmup", "0")
    assert p.returncode != 0 and d is None and "no CPU fallback" in p.stderr
    p, d = _run("--gpus", "2", "--steps", "1")
    assert p.returncode != 0 and d is None and "GPU" in p.stderr


# ---- the performance gate (tools/perf_gate.py)

def _gate():
    import importlib.util
    spec = importlib.util.spec_from_file_location("perf_gate", os.path.join(ROOT, "tools", "perf_gate.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_perf_gate_would_have_caught_round_4s_read_ahead_leg():
    """Round 4's committed line went out with the read-ahead loop three times slower than the synchronous call (a 40 ms
    garbage-collector pause inside a one-shot timing) and the batched form at 0.79 of the PCIe ceiling measured in the same
    run: the in-run relations of the gate fail on exactly those two."""
    import json
    g = _gate()
    line = json.load(open(os.path.join(ROOT, "profiles", "r04", "bench_n1.json")))
    rows = {name: ok for name, ok, _ in g.gate(line, line, 0.05)}
    assert rows["read-ahead <= synchronous (Python loop)"] is False
    assert rows["batched read-ahead >= 0.87 x PCIe ceiling of this run"] is False
    assert rows["headline Mvectors/s (cfg2)"] and rows["cfg4 Mvectors/s"] and rows["parity_check.ok"]


def test_perf_gate_is_one_sided_and_tolerant():
    import copy
    import json
    g = _gate()
    assert g.DEFAULT_BASELINE.endswith(os.path.join("profiles", "r05", "bench_n1.json"))      # the PREVIOUS round's committed line, not a refreshed copy
    base = json.load(open(g.DEFAULT_BASELINE))
    base = base.get("parsed", base)
    line = copy.deepcopy(base)
    line["value"] = base["value"] * 0.96                       # 4 % slower: inside the tolerance
    line["cfg3_chain"]["almeida_ms"] = base["cfg3_chain"]["almeida_ms"] * 1.06      # 6 % slower at 5 %: fails
    line["cfg4"]["Mvectors_per_s"] = base["cfg4"]["Mvectors_per_s"] * 1.30    # faster never fails
    line["cfg3_chain"]["per_content"]["pm3"]["lk_ms"] = base["cfg3_chain"]["per_content"]["pm3"]["lk_ms"] * 1.12   # 12 % slower: fails (this row: 10 %, its own spread over processes and boxes is 7-9 %)
    line["cfg3_chain"]["per_content"]["pm16"]["lk_ms"] = base["cfg3_chain"]["per_content"]["pm16"]["lk_ms"] * 1.04  # 4 %: passes
    # cfg5: the new line carries three processes' p50s (the best one is gated), the round-5 baseline only its single p50; 15 %
    line["cfg5_stream"]["process_level"] = {"lsq": {"p50_min": base["cfg5_stream"]["latency_ms"]["p50"] * 1.14, "p50_median_of_processes": 9.9},
                                            "ransac": {"p50_min": base["cfg5_stream"]["ransac"]["latency_ms"]["p50"] * 1.16, "p50_median_of_processes": 0.1}}
    rows = {name: ok for name, ok, _ in g.gate(line, base, 0.05)}
    assert rows["headline Mvectors/s (cfg2)"] and rows["cfg4 Mvectors/s"] and rows["LK flow ms, +-16 px content"]
    assert rows["LK flow ms, +-3 px content"] is False and rows["Almeida cluster solve ms (2.07 M records)"] is False
    assert rows["cfg5 p50 ms (LSQ), best of 3 processes"] is True and rows["cfg5 p50 ms (RANSAC), best of 3 processes"] is False
    line["cfg4"]["parity_check"]["ok"] = False                 # a parity failure is a gate failure
    rows = {name: ok for name, ok, _ in g.gate(line, base, 0.05)}
    assert rows["cfg4.parity_check.ok"] is False


def test_perf_gate_uses_the_baseline_builds_sample_median_for_noisy_rows():
    """round 6: the round-5 BUILD re-measured twelve times with the gate's protocol; a cfg3 row is gated (5 %; the +-3 px LK row 10 %) against the median of those
    samples, not against the single (low) draw the committed line holds -- and nothing of round 6 is in the sample file"""
    import copy
    import json
    g = _gate()
    base = json.load(open(g.DEFAULT_BASELINE)); base = base.get("parsed", base)
    samples = json.load(open(g.BASELINE_SAMPLES))
    row = samples["rows"]["cfg3_chain.per_content.pm3.lk_ms"]
    assert len(row["samples"]) == 12 and row["min"] <= row["committed_r05_line"] <= row["max"] and row["committed_r05_line"] < row["median"]
    line = copy.deepcopy(base)
    line["cfg3_chain"]["per_content"]["pm3"]["lk_ms"] = round(row["median"] * 1.09, 4)       # 9 % over the build's median (11 % over the committed draw); the row's window is 10 %
    rows = {name: ok for name, ok, _ in g.gate(line, base, 0.05, samples)}
    assert rows["LK flow ms, +-3 px content"] is True
    assert {name: ok for name, ok, _ in g.gate(line, base, 0.05)}["LK flow ms, +-3 px content"] is False       # without the samples: the single draw
    line["cfg3_chain"]["per_content"]["pm3"]["lk_ms"] = round(row["median"] * 1.12, 4)
    assert {name: ok for name, ok, _ in g.gate(line, base, 0.05, samples)}["LK flow ms, +-3 px content"] is False


def test_quiet_gc_counts_what_still_runs_and_restores_the_collector():
    import gc
    from bench_legs import QuietGC, median_min_max
    before = gc.get_freeze_count()
    with QuietGC() as q:
        assert gc.get_freeze_count() > before
        junk = [[i] for i in range(5000)]                      # young objects are still collected
        gc.collect(0)
        del junk
    s = q.summary()
    assert s["collections"] >= 1 and s["oldest_generation"] is not None
    assert gc.get_freeze_count() == 0 and q._cb not in gc.callbacks
    assert median_min_max([3.0, 1.0, 2.0, 10.0, 2.5]) == {"median": 2.5, "min": 1.0, "max": 10.0, "repeats": 5}


def test_plain_run_times_exactly_the_steps_asked_for_and_dumps_the_last_steps_outputs(tmp_path):
    """A run without --full: the line carries no parity or roofline object; --dump-outputs writes what the last timed step
    computed (the stub's per-pair table), the same on every run."""
    for sub in ("a", "b"):
        p, d = _run("--stub", "--pairs", "6", "--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path / sub))
        assert p.returncode == 0, p.stderr[-2000:]
        assert d["steps"] == 4 and d["warmup"] == 2 and d["ms_per_step"] >= 0 and "parity_check" not in d and "roofline" not in d
    a = np.load(tmp_path / "a" / "checksum.npy")
    assert a.dtype == np.float64 and a.shape == (6, 2) and np.array_equal(a, np.load(tmp_path / "b" / "checksum.npy"))
    assert np.array_equal(a.astype(np.uint32).view(np.int64).reshape(-1), np.arange(6) * 1000)
