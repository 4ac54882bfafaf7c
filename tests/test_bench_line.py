"""bench.py's stdout contract: ONE JSON line of at most 6 KB that carries the contract's scalars,
`roofline`, `cpu_baseline` and `config.workload`; everything else goes to bench_extra.json. The input here is the
largest full record a run has produced (round 5's 21.7 KB line, profiles/r05zz_bench_steps20.json): such records come
from `bench.py --full`. A plain run's line and its `--dump-outputs` arrays are checked on the GPU at the end."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _full_record():
    with open(os.path.join(ROOT, "profiles", "r05zz_bench_steps20.json")) as fh:
        return json.load(fh)


def test_line_is_small_and_complete():
    line = bench.compact_line(_full_record())
    assert "\n" not in line
    assert len(line.encode()) < bench.LINE_LIMIT <= 6144
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "extra"):
        assert k in d, k
    assert d["config"]["workload"].startswith("Llama-2-7B int4")
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = d["cpu_baseline"]
    assert c["value"] > 0 and c["kind"] in ("port", "reference") and c["cores"] >= 1 and len(c["sample"]) <= 120
    assert d["parity"]["greedy_tokens_equal"] is True and d["parity"]["decode_logits_max_abs"] < 1e-3
    assert 0.0 < d["prefill"]["mfma_frac"] < 1.0


def test_line_never_exceeds_the_limit_whatever_the_record_holds():
    rec = _full_record()
    rec["configs_summary"] = "x" * 5000
    rec["note"] = "y" * 5000
    line = bench.compact_line(rec)
    assert len(line.encode()) <= bench.LINE_LIMIT
    d = json.loads(line)
    assert "roofline" in d and "cpu_baseline" in d and d["value"] > 0


def test_emit_writes_the_full_record_beside_the_line(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    rec = _full_record()
    bench.emit(rec)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and json.loads(out[0])["extra"] == bench.EXTRA_FILE
    with open(tmp_path / bench.EXTRA_FILE) as fh:
        full = json.load(fh)
    assert len(full["extra_configs"]) == len(rec["extra_configs"]) and "launch_modes" in full


def test_traffic_comes_from_the_latest_counter_pass(tmp_path, monkeypatch):
    """Visit names sort like spreadsheet columns (r06k < r06z < r06aa < r06ab), not as plain strings."""
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    os.makedirs(tmp_path / "profiles")
    for name, b in (("r05z", 1.0), ("r06k", 2.0), ("r06ab", 3.0), ("r06aa", 4.0)):
        with open(tmp_path / "profiles" / (name + "_pmc_traffic.json"), "w") as fh:
            json.dump({"hbm_bytes_per_launch": b, "command": "c"}, fh)
    t = bench.read_traffic()
    assert t["source"] == "profiles/r06ab_pmc_traffic.json" and t["bytes"] == 3.0 and t["measured_in_this_run"] is False


def test_full_and_dump_outputs_are_options():
    """`--full` (everything beside the headline) and `--dump-outputs DIR` are parsed before any GPU work."""
    import subprocess

    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-500:]
    assert "--full" in res.stdout and "--dump-outputs" in res.stdout


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs_twice(tmp_path):
    """A plain run (no --full) prints the contract's scalars and nothing that needs a run of its own; `--dump-outputs`
    writes the last timed step's logits and the timed steps' greedy tokens (the last one is the logits' argmax), and
    two runs with the same arguments write the same arrays."""
    import subprocess

    import numpy as np

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "7b", "--steps", "5",
           "--warmup", "2", "--layers", "2", "--condition-ms", "20"]
    got = []
    for run in ("a", "b"):
        res = subprocess.run(cmd + ["--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600,
                             cwd=ROOT)
        assert res.returncode == 0, res.stderr[-3000:]
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, res.stdout[-2000:]
        d = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert k in d, k
        assert d["steps"] == 5 and d["warmup"] == 2 and d["value"] > 0
        assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1.0
        for k in ("roofline", "cpu_baseline", "prefill", "parity", "value_128_steps"):
            assert k not in d, k
        logits, tokens = np.load(tmp_path / run / "logits.npy"), np.load(tmp_path / run / "tokens.npy")
        assert logits.dtype == np.float32 and logits.shape == (32000,) and np.isfinite(logits).all()
        assert tokens.dtype == np.float64 and tokens.shape == (5,) and int(tokens[-1]) == int(logits.argmax())
        got.append((logits, tokens))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
