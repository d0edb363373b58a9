"""bench.py end to end on the GPU box: the last stdout line is the compact, parsable headline record, of a `--full` run
and of a plain one."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_stdout_last_line_parses_and_is_small(tmp_path):
    det = tmp_path / "details.json"
    env = dict(os.environ, VS_BENCH_DETAILS=str(det))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--quick", "--no-other-configs"],
                       capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(p.stdout) < 8000 and len(lines[-1]) < 4096
    d = json.loads(lines[-1])
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["value"] > 1e6 and d["config"]["per_gpu_batch"] == 32 and d["config"]["t_mel"] == 1024, lines[-1]
    r = d["roofline"]
    assert r["bound"] == "mfma" and 0 < r["frac"] < 1 and r["kernel"].startswith(("conv_ktap_kernel", "conv_split_kernel")) and r["avg_launch_ms"] > 0, r
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["items"] == 1 and c["of_items"] == 32 and c["seconds"] > 0 and c["cores"] >= 1, c
    assert d["waveform_max_abs_err"] <= 1e-4 and d["flow_logdet_rel_err"] <= 1e-4, (d["waveform_max_abs_err"], d["flow_logdet_rel_err"])
    assert d["fp32_mfma_engine"]["ms_per_step"] > d["ms_per_step"], (d["fp32_mfma_engine"], d["ms_per_step"])
    full = json.loads(det.read_text())
    assert "all_instances" in full["headline"]["roofline"] and full["headline"]["value"] == pytest.approx(d["value"], rel=1e-4)


PLAIN_OVERHEAD_SECONDS = 30.0      # what a plain run may spend outside its warm-up and timed steps


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone_and_is_lean(tmp_path):
    """without --full: warm-up, the timed steps, ONE line with the headline keys; none of the legs that take runs or CPU time of their own, no details
    file; whole process (start to exit, first-step set-up included) less the steps themselves within PLAIN_OVERHEAD_SECONDS"""
    det = tmp_path / "details.json"
    env = dict(os.environ, VS_BENCH_DETAILS=str(det))
    steps, warmup = 3, 2
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       capture_output=True, text=True, env=env, timeout=900)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1 and len(lines[0]) < 4096, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"].startswith("audio samples/sec") and d["unit"] == "audio samples/s" and d["higher_is_better"] is True and d["dtype"].startswith("f32")
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup and d["config"]["per_gpu_batch"] == 32 and d["config"]["t_mel"] == 1024
    assert d["value"] > 1e6 and d["value"] == pytest.approx(32 * 1024 * 256 / (d["ms_per_step"] * 1e-3), rel=1e-4)
    for key in ("roofline", "cpu_baseline", "cpu_baseline_torch", "waveform_max_abs_err", "flow_logdet_rel_err", "fp32_mfma_engine", "split_bf16x6_engine",
                "single_stream", "details"):
        assert key not in d, key
    assert not det.exists()
    overhead = wall - (steps + warmup) * d["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.1f} s in all, {overhead:.1f} s outside its {steps + warmup} steps of {d['ms_per_step']:.1f} ms")
    assert overhead <= PLAIN_OVERHEAD_SECONDS, (wall, d["ms_per_step"])
