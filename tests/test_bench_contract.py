"""bench.py's output contract on a small graph: one JSON line with the driver's keys; with --full also roofline, cpu_baseline and
the other blocks that take runs of their own."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.gpu
def test_bench_json_line(product_lib):
    if product_lib.mtg_device_count() < 1:
        pytest.fail("needs a GPU")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--log2-edges", "19",
                        "--cpu-baseline-seconds", "2", "--full"], capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "device_mode", "scaling_stages_ms", "seeds",
                "roofline_stages", "cold_step_ms", "visited_per_step", "full_size", "one_shot", "clib_route"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["vs_baseline"] is None
    assert d["unit"] == "edges/s" and d["higher_is_better"] is True and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - d["units_per_step"]["relaxed_edges"] / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-6 and rf["kernels"] and "sssp_enum_kernel" in rf["kernels"][0]["kernel"]
    assert "traffic" in rf and "traffic_note" in rf
    # the pruned search visits no more than the full balls and emits the same candidates; the roofline prices the visited bytes
    vis, full = d["visited_per_step"], d["units_per_step"]
    assert vis["emitted"] == full["emitted"] and vis["settled_nodes"] <= full["settled_nodes"] and vis["relaxed_edges"] <= full["relaxed_edges"]
    assert rf["algorithmic_bytes_per_launch"] == 5 * vis["relaxed_edges"] + 12 * vis["settled_nodes"] + 12 * vis["emitted"]
    assert rf["full_ball_equivalent"]["algorithmic_bytes_per_launch"] == 5 * full["relaxed_edges"] + 12 * full["settled_nodes"] + 12 * full["emitted"]
    # every other GPU stage of the step has its own roofline entry (HIP-event time, byte model, frac), in both Euler modes
    stages = {(x["stage"], x["euler_mode"]) for x in d["roofline_stages"]}
    assert {("replay", "device"), ("insert_eulerise", "device"), ("replay", "host"), ("insert_eulerise", "host"), ("records", "host"), ("cut", "host")} <= stages
    # device order: the tigs straight from the pairing (one stage, cut_first_device.hip) -- or, where the graph sent the step through the
    # closed walks, decomposition + cut
    assert ("tigs_from_pairing", "device") in stages or {("decomposition", "device"), ("cut", "device")} <= stages
    for x in d["roofline_stages"]:
        assert x["avg_launch_ms"] > 0 and x["algorithmic_bytes"] > 0 and abs(x["frac"] - x["achieved"] / 8000.0) < 1e-4
        # the pass-independent floor (inputs once + outputs once) lies below what the implementation's passes move
        assert 0 < x["minimum_bytes"] <= x["algorithmic_bytes"] and 0 < x["frac_of_minimum"] <= x["frac"] + 1e-6
    cs = d["cold_step_ms"]
    assert cs["device"]["step_ms"] > 0 and cs["host"]["step_ms"] > 0 and cs["device"]["device_graph_build_ms"] > 0
    assert d["full_size"] is None  # (only the headline configuration runs the nominal-size step)
    # the consuming one-shot call (host arrays in -> clib.rs arrays out), each Euler mode in a process of its own; same tigs as the steps
    for mode in ("device", "host"):
        os_ = d["one_shot"][mode]
        assert "error" not in os_, os_
        assert os_["total_s"] > 0 and os_["same_result_both_calls"] and os_["later_call"]["tigs"] == d["config"]["tigs"]
        assert set(os_["later_call"]["phases_s"]) >= {"device_build", "sssp", "eulerise", "euler", "cut"}
    # the reference's own way in (initialise / merge_nodes per link / build_graph / compute): same number of tigs in both Euler modes (T3)
    cr = d["clib_route"]
    for mode in ("device", "host"):
        assert "error" not in cr[mode], cr[mode]
        assert cr[mode]["links"] > cr[mode]["unitigs"] > 0 and cr[mode]["build_graph_s"] > 0 and cr[mode]["compute_tigs_s"] > 0
    assert cr["device"]["tigs"] == cr["host"]["tigs"] > 0 and cr["device"]["tig_edges"] == cr["host"]["tig_edges"]
    dm = d["device_mode"]
    assert dm["ms_per_step"] > 0 and dm["tigs"] == d["config"]["tigs"] and "finish" in dm["phases_ms"]   # T3 across the two modes
    assert set(d["seeds"]) == {"2", "3"} and all(v["sssp_stage_ms"] > 0 for v in d["seeds"].values())
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and cb["sample"]
    assert cb["pairs"] == d["config"]["pairs"] and cb["tigs"] == d["config"]["tigs"]   # the CPU port and the GPU path agree


@pytest.mark.gpu
def test_bench_plain_line(product_lib):
    """Without --full the line carries the headline alone: the driver's keys, none of the blocks that take runs of their own."""
    if product_lib.mtg_device_count() < 1:
        pytest.fail("needs a GPU")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--log2-edges", "19"],
                       capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config", "units_per_step"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "edges/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and d["config"]["tigs"] > 0 and d["config"]["candidates"] > 0
    assert abs(d["value"] - d["units_per_step"]["relaxed_edges"] / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    for key in ("roofline", "roofline_stages", "visited_per_step", "cpu_baseline", "device_mode", "tig_download_ms", "cold_step_ms",
                "one_shot", "clib_route", "full_size", "seeds"):
        assert key not in d, key


def _load_bench():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _read_dump(d: Path) -> dict:
    import numpy as np

    return {p.stem: np.load(p) for p in sorted(d.glob("*.npy"))}


def test_dump_outputs_small_and_sampled(tmp_path):
    """--dump-outputs' writer: float64 files only; small outputs whole, large ones as a fixed seeded sample with its positions;
    the same arrays give the same files, a change anywhere in them changes the summary."""
    import numpy as np

    bench = _load_bench()
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 6, size=1000)
    small_lim, small_ed = np.cumsum(lens).astype(np.uint64), rng.integers(0, 1 << 31, size=int(lens.sum()), dtype=np.uint64).astype(np.uint32)
    bench.dump_outputs(tmp_path / "small", small_lim, small_ed)
    d = _read_dump(tmp_path / "small")
    assert set(d) == {"tig_summary", "tig_limits", "tig_limits_index", "tig_edges", "tig_edges_index"}
    assert all(a.dtype == np.float64 for a in d.values())
    assert np.array_equal(d["tig_limits"], small_lim.astype(np.float64)) and np.array_equal(d["tig_edges"], small_ed.astype(np.float64))
    assert d["tig_summary"][:2].tolist() == [len(small_lim), len(small_ed)]

    n = 3 * bench.DUMP_SAMPLE
    big_lim = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(3)
    big_ed = (np.arange(3 * n, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 30)).astype(np.uint32)
    for name in ("a", "b"):
        bench.dump_outputs(tmp_path / name, big_lim, big_ed)
    a, b = _read_dump(tmp_path / "a"), _read_dump(tmp_path / "b")
    assert all(np.array_equal(a[key], b[key]) for key in a)
    assert sum(p.stat().st_size for p in (tmp_path / "a").glob("*.npy")) <= 64 << 20
    assert len(a["tig_edges"]) == len(a["tig_limits"]) == bench.DUMP_SAMPLE
    assert np.array_equal(a["tig_edges"], big_ed[a["tig_edges_index"].astype(np.int64)].astype(np.float64))
    assert np.array_equal(a["tig_limits"], big_lim[a["tig_limits_index"].astype(np.int64)].astype(np.float64))
    changed = big_ed.copy()
    changed[n // 2 + 7] ^= 1
    bench.dump_outputs(tmp_path / "c", big_lim, changed)
    assert _read_dump(tmp_path / "c")["tig_summary"][3] != a["tig_summary"][3]


@pytest.mark.gpu
def test_bench_dump_outputs_repeatable(product_lib, tmp_path):
    """--dump-outputs on a small graph: the tigs of the last timed step, whole at this size, the same in two runs with the same
    arguments; --steps sets the number of timed steps."""
    import numpy as np

    if product_lib.mtg_device_count() < 1:
        pytest.fail("needs a GPU")
    runs = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--log2-edges", "19",
                            "--no-cpu-baseline", "--no-cold-steps", "--no-one-shot", "--extra-seeds", "", "--device-mode-steps", "0",
                            "--dump-outputs", str(tmp_path / name)], capture_output=True, text=True, cwd=str(ROOT), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, r.stdout[-2000:]
        runs.append((json.loads(lines[0]), _read_dump(tmp_path / name)))
    (da, a), (db, b) = runs
    assert da["steps"] == 3 and da["ms_per_step"] > 0
    assert set(a) == set(b) == {"tig_summary", "tig_limits", "tig_limits_index", "tig_edges", "tig_edges_index"}
    assert all(v.dtype == np.float64 and np.array_equal(v, b[key]) for key, v in a.items())
    n_tigs, n_edges = int(a["tig_summary"][0]), int(a["tig_summary"][1])
    assert n_tigs == da["config"]["tigs"] == db["config"]["tigs"] and len(a["tig_limits"]) == n_tigs and len(a["tig_edges"]) == n_edges
    assert a["tig_limits"][-1] == n_edges and np.all(np.diff(a["tig_limits"]) > 0)
