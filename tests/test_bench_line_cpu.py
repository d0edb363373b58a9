"""bench.py's stdout contract: the LAST line is one JSON object < 4 KB carrying the headline record with `roofline` and
`cpu_baseline`; everything bulky goes to bench_details.json.  (The driver keeps only the last ~8 KB of stdout: round 3's 22 KB line was
truncated and the headline went unmeasured.)"""
import json
import os

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _full_r03():
    return json.load(open(os.path.join(ROOT, "profiles", "r03_f_full_bench_line.json")))


def test_final_line_is_compact_and_complete():
    full = _full_r03()
    line = bench.compact_line(full, "split3", "bench_details.json")
    assert "\n" not in line and len(line) < bench.MAX_LINE_BYTES == 4096
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "cpu_baseline", "waveform_max_abs_err", "flow_logdet_rel_err", "fp32_mfma_engine"):
        assert key in d, key
    assert "model" not in d["config"] and d["config"]["workload"].startswith("VISinger synthesis")
    r = d["roofline"]
    for key in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_ms", "step"):
        assert key in r, key
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-5 and abs(r["step"]["frac"] - r["step"]["achieved"] / r["step"]["peak"]) < 1e-5
    assert abs(d["value"] - full["value"]) <= 1e-5 * full["value"] and abs(d["ms_per_step"] - full["ms_per_step"]) <= 1e-5 * full["ms_per_step"]
    assert set(d["fp32_mfma_engine"]) >= {"value", "ms_per_step"}
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] >= 1


def test_whole_default_stdout_fits_the_driver_capture():
    """the default run prints one compact line per other BASELINE config (2, 3, 5), then the headline line: together < 8 000 bytes"""
    full = _full_r03()
    lines = [bench.compact_line(full["other_configs"][c], "bf16" if c == "5" else "split3") for c in "235"]
    lines.append(bench.compact_line(full, "split3", "bench_details.json"))
    assert all(len(x) < 4096 for x in lines) and sum(len(x) + 1 for x in lines) < 8000
    assert json.loads(lines[1])["config"]["baseline_config"] == 3 and json.loads(lines[2])["ms_per_step"] > 0


def test_oversized_fields_cannot_push_the_line_past_the_limit():
    full = _full_r03()
    full["config"]["workload"] = "x" * 5000
    full["dtype"] = "y" * 5000
    full["cpu_baseline"]["sample"] = "z" * 5000
    full["roofline"]["traffic_source"] = "recorded: " + "w" * 300 + " (long tail " + "v" * 5000
    line = bench.compact_line(full, None, "bench_details.json")
    assert len(line) < 4096 and json.loads(line)["roofline"]["frac"] > 0


def test_traffic_is_keyed_by_workload():
    """a config-2 line must not show the headline batch's bytes"""
    dom = "conv_split_kernel<1, 8, 4, 1, 3>"
    assert bench.pmc_traffic(dom, bench.HEADLINE_WORKLOAD) is not None
    assert bench.pmc_traffic(dom, bench.workload_key(2, 8, 512, 192, 256, "f32")) is None
    assert bench.workload_key(0, 32, 1024, 192, 256, "f32") == bench.HEADLINE_WORKLOAD
    prof = {dom: dict(launches=10, flops=1e12, bytes=1e9, ms=5.0), "noted_site": dict(launches=3, flops=1e11, bytes=0.0, ms=0.0)}
    r = bench.roofline_from_profile(prof, 0.01, 1, bench.workload_key(2, 8, 512, 192, 256, "f32"))
    assert r["traffic"] is None and r["mfma_executed"] is None and "noted_site" not in r["all_instances"]      # (and no ZeroDivisionError)
    r = bench.roofline_from_profile(prof, 0.01, 1, bench.HEADLINE_WORKLOAD)
    assert r["traffic"] > 0 and r["traffic_over_algorithmic"] == r["traffic"] / 1e8


def test_dump_outputs_is_bounded_and_reproducible(tmp_path):
    """--dump-outputs: every returned array as <name>.npy in float32 / float64, at most 64 MB in all; a larger output becomes the same seeded
    sample in every run (what lets two builds be compared output for output)"""
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(3)
    small = {"wav_out": torch.randn(4, 1000, generator=g), "f0_pred": torch.randn(4, 10, 2, generator=g).double(), "ids": torch.arange(5),
             "loss": 1.25, "absent": None}
    bench.dump_outputs(small, str(tmp_path / "s"))
    got = {p.stem: np.load(p) for p in (tmp_path / "s").glob("*.npy")}
    assert set(got) == {"wav_out", "f0_pred", "ids", "loss"}
    assert got["wav_out"].dtype == np.float32 and np.array_equal(got["wav_out"], small["wav_out"].numpy())
    assert got["f0_pred"].dtype == np.float64 and got["ids"].dtype == np.float64 and float(got["loss"]) == 1.25
    big = {"wav_out": torch.randn(20, 1 << 20, generator=g)}        # 80 MB of float32
    for d in ("a", "b"):
        bench.dump_outputs(big, str(tmp_path / d))
    a, b = np.load(tmp_path / "a" / "wav_out.npy"), np.load(tmp_path / "b" / "wav_out.npy")
    assert np.array_equal(a, b) and (tmp_path / "a" / "wav_out.npy").stat().st_size <= bench.DUMP_BUDGET_BYTES
    assert a.size > 0.75 * bench.DUMP_BUDGET_BYTES / 4 and np.isin(a[:1000], big["wav_out"].numpy().reshape(-1)).all()


def test_full_is_an_option_and_off_by_default(monkeypatch):
    """a plain command line asks for the headline figure alone; --full switches the other legs on, and the flags that trim them stay accepted"""
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "2"])
    a = bench.parse_args()
    assert a.full is False and (a.gpus, a.steps, a.warmup, a.streams, a.math, a.batch, a.frames) == (1, 4, 2, 2, "split3", 32, 1024)
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--quick", "--no-other-configs", "--no-cpu-baseline"])
    a = bench.parse_args()
    assert a.full is True and a.quick and a.no_other_configs and a.no_cpu_baseline
    assert bench.has_kernel_records(None, 1) and not bench.has_kernel_records(None, 2) and bench.has_kernel_records({"dt": 1.0}, 2)


def test_a_line_without_the_full_legs_is_still_the_headline_record():
    """a plain run's record has no roofline / cpu_baseline / details: the compact line carries the contract keys and nothing invented"""
    full = _full_r03()
    plain = {k: v for k, v in full.items() if k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                                                    "vs_baseline", "dtype", "data", "config")}
    d = json.loads(bench.compact_line(plain, "split3", None))
    assert d["value"] == json.loads(bench.compact_line(full, "split3", None))["value"] and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert d["dtype"] == bench.SHORT_DTYPE["split3"] and not {"roofline", "cpu_baseline", "details", "fp32_mfma_engine"} & set(d)
