"""GPU: bench.py's two modes at a small size.  A plain run prints the headline line alone (no roofline, latency, config 3 / 5
or CPU baseline); --full adds those fields and every one of them is measured.  The headline fields mean the same in both."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--docs", "2000000", "--queries", "256", "--query-file", "768", "--warmup", "1", "--steps", "2"]
HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config", "strata",
            "strata_run", "setup_s", "host_ms_per_step", "footprint")


def run_bench(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def test_bench_plain_and_full():
    plain = run_bench(SMALL)
    full = run_bench(SMALL + ["--full", "--config5-docs", "2000000", "--cpu-seconds", "1", "--latency-samples", "12"])
    for d, is_full in ((plain, False), (full, True)):
        assert all(k in d for k in HEADLINE), sorted(set(HEADLINE) - set(d))
        assert d["full"] is is_full
        assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 2 and d["warmup"] == 1
        assert sorted(d["strata"]) == ["cc", "sc", "ss"] and all(s["scan_ms"] > 0 for s in d["strata"].values())
    for k in ("metric", "unit", "higher_is_better", "dtype", "config", "strata_run"):
        assert plain[k] == full[k], k

    assert plain["roofline"] is None and plain["p50_latency_ms"] is None and plain["cpu_baseline"] is None
    assert "config3" not in plain and "config5" not in plain

    rf = full["roofline"]
    assert rf["achieved"] > 0 and rf["algo_bytes_per_launch"] > 0 and rf["launch_ms"] > 0
    assert full["p50_latency_ms"] > 0 and full["p95_latency_ms"] >= full["p50_latency_ms"]
    assert full["config3"]["ok"] == 256 and full["config3"]["queries_per_s"] > 0
    assert "error" not in full["config5"] and full["config5"]["ok"] == 1024
    assert full["cpu_baseline"]["value"] > 0
