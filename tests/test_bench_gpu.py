"""bench.py's output contract on a real GPU: one JSON line with the fields the driver and the judge read, at N = 1
and (rehearsal: gloo control flow, both ranks on this one GPU) at N = 2."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _json_lines(text):
    out = []
    for ln in text.splitlines():
        ln = ln.strip()
        if ln.startswith("{") and ln.endswith("}"):
            out.append(json.loads(ln))
    return out


def test_single_gpu_line():
    """--full: the headline and every measurement of its own in the same line."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "1000", "--warmup", "2",
                        "--nsamp", "256", "--cpu-nsamp", "64", "--sizes", "128,512"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1
    d = lines[0]
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 1000 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["unit"] == "boxes/s" and d["value"] > 0 and d["vs_baseline"] is None and d["scaling"] == "weak"
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12 and 0 < rf["frac"] < 1
    assert rf["launches_timed"] >= 1 and rf["launches"] >= rf["launches_timed"]
    assert rf["timed_in"] and "traffic" in rf
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and cb["unit"] == "boxes/s" and cb["sample"]
    # the auxiliary legs: reference precision, BASELINE configs[2], other grid sizes, both byte counts of the step
    assert d["f64"]["value"] > 0 and d["f64"]["dtype"] == "f64"
    c3 = d["config3"]
    assert c3["ms_per_chain"] > 0 and c3["model_sweeps"] == 13.5 and 0 < c3["rsd_roofline"]["frac"] < 1
    assert set(d["sizes"]) == {"128", "512"} and all(v["value"] > 0 for v in d["sizes"].values())
    pr = d["pipeline_roofline"]
    assert pr["model_sweeps"] == 5.0 and pr["moved_sweeps"] == 4.5 and 0 < pr["frac_moved"] < pr["frac"] < 1
    assert "from_profiles" in d and "file" in d["from_profiles"] and "head" in d["from_profiles"]
    # the headline is the median of >= 5 fenced regions that hold the `steps` timed steps, every region listed
    rg = d["regions"]
    assert rg["count"] >= 5 and len(rg["ms_per_step"]) == rg["count"] and all(x > 0 for x in rg["ms_per_step"])
    assert len(rg["steps"]) == rg["count"] and sum(rg["steps"]) == d["steps"]
    assert sorted(rg["ms_per_step"])[rg["count"] // 2] == pytest.approx(d["ms_per_step"], rel=1e-3) and rg["spread"] >= 0
    assert d["collective"] is None                 # one rank: no process group
    assert "best of" in c3["workload"]


def test_plain_run_is_the_headline_only():
    """Without --full the run sets up, spins up, warms up, times the steps and prints the line: none of the legs, passes
    or baselines that are measurements of their own, and little time outside the timed steps.  With one stream the
    roofline brackets sit inside the timed region, so that object stays."""
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "400", "--warmup", "2"]
    t0 = time.time()
    r = subprocess.run(base + ["--nsamp", "256"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.time() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1
    d = lines[0]
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype",
                "regions", "config", "pipeline_roofline"):
        assert key in d, key
    assert d["steps"] == 400 and d["warmup"] == 2 and d["value"] > 0 and d["unit"] == "boxes/s"
    assert d["metric"] == "256^3 box realisations/sec (gen + log-normal + P(k))" and d["dtype"] == "f32"
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3 and d["config"]["full"] is False
    assert d["roofline"] is None and d["cpu_baseline"] is None
    for key in ("f64", "config3", "spectra_only_variant", "sizes", "strong_scaling", "roofline_gen", "roofline_bin",
                "roofline_z", "from_profiles"):
        assert key not in d, key
    assert wall - (400 + 2) * d["ms_per_step"] * 1e-3 < 30.0, wall
    r = subprocess.run(base + ["--nsamp", "256", "--streams", "1"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_lines(r.stdout)[0]
    assert d["roofline"]["timed_in"].startswith("timed region") and d["roofline"]["launches_timed"] >= 1
    assert "kernel_ms_per_step" in d and "f64" not in d and d["cpu_baseline"] is None


def test_two_ranks_started_by_bench_itself():
    """`python bench.py --full --gpus 2` with no launcher around it: bench.py starts the two ranks (rehearsal: gloo control
    flow, both ranks on this one GPU), rank 0 prints the line, and the strong-scaling leg runs the slab-decomposed box
    as a child job of two ranks."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(FASTBOX_BENCH_BACKEND="gloo", FASTBOX_BENCH_ONE_DEVICE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--steps", "1000",
                        "--warmup", "2", "--nsamp", "128", "--slab-sizes", "64"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [d for d in _json_lines(r.stdout) if d.get("scaling") == "weak"]
    assert len(lines) == 1                      # rank 0 only
    d = lines[0]
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["cpu_baseline"] is None
    assert d["config"]["parallelism"] == "replicas x2"
    import math

    def group_ok(c):        # what the process group really was: backend, size as the group reports it, one entry per rank
        assert c["backend"] == "gloo" and c["world_size"] == 2 and len(c["devices"]) == 2
        assert sorted(g["rank"] for g in c["devices"]) == [0, 1] and all("device" in g and "pci_bus_id" in g for g in c["devices"])
    group_ok(d["collective"])
    assert d["regions"]["count"] >= 5 and sum(d["regions"]["steps"]) == d["steps"] == 1000
    ss = d["strong_scaling"]["64"]
    assert ss["n_gpus"] == 2 and ss["scaling"] == "strong" and math.isfinite(ss["value"]) and ss["value"] > 0
    assert math.isfinite(ss["ms_per_step"]) and ss["finite"] is True
    ex = ss["exchange"]
    assert ex["ms_per_step_pipelined"] > 0 and ss["config"]["parallelism"] == "slab x2"
    assert math.isfinite(ex["ms_per_step_one_realisation_at_a_time"]) and math.isfinite(ex["exposed_exchange_ms_per_step"])
    assert 2 <= ex["chunks_per_transform"] <= 4 and math.isfinite(ex["ms_per_step_one_realisation_at_a_time_unchunked"])
    group_ok(ss["collective"])


def test_two_ranks_under_an_external_launcher():
    """The driver's form: torch.distributed.run around bench.py (WORLD_SIZE set): no second launch."""
    env = dict(os.environ, FASTBOX_BENCH_BACKEND="gloo", FASTBOX_BENCH_ONE_DEVICE="1", MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29571", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "6", "--warmup", "2", "--nsamp", "128", "--no-extras"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1 and lines[0]["n_gpus"] == 2 and lines[0]["value"] > 0
    assert lines[0]["collective"]["world_size"] == 2 and lines[0]["collective"]["backend"] == "gloo"


def test_dump_outputs_are_the_last_timed_step_and_repeat_run_for_run(tmp_path):
    """--dump-outputs: the last timed step's spectrum and (a seeded sample of) its delta_x, the same files whatever the
    spin-up ran, and the same numbers as the public API gives for the realisation the line names."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    N, steps = 256, 30
    runs = []
    for i, spin in enumerate(("0", "0.3")):
        out = tmp_path / ("run%d" % i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "2",
                            "--nsamp", str(N), "--no-extras", "--no-cpu-baseline", "--spin-up", spin,
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = _json_lines(r.stdout)
        assert len(lines) == 1 and lines[0]["steps"] == steps
        info = lines[0]["dump_outputs"]
        names = sorted(os.listdir(str(out)))
        assert names == sorted(info["files"]) == ["delta_x.npy", "pk.npy", "pk_k.npy", "pk_stddev.npy"]
        assert sum(os.path.getsize(str(out / n)) for n in names) <= 64 << 20
        runs.append((info, {n[:-4]: np.load(str(out / n)) for n in names}))
    (info, got), (info2, got2) = runs
    assert info["seed"] == info2["seed"] and info["realisation"] == info2["realisation"]
    for name, a in got.items():
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)), name
        assert np.array_equal(a, got2[name], equal_nan=True), name
    assert got["delta_x"].dtype == np.float32 and got["delta_x"].shape == (bench.DUMP_VOXELS,)
    # the same realisation through the public API
    from fastbox_amd import CosmoBox, default_cosmo
    box = CosmoBox(cosmo=default_cosmo, box_scale=1e3, nsamp=N, redshift=0., realise_now=False, precision="f32",
                   rng="device", seed=info["seed"])
    box._realisation = info["realisation"]
    dx = box.realise_density()
    kc, pk, err = box.binned_power_spectrum(delta_x=box.lognormal(dx), nbins=20)
    filled = ~np.isnan(pk)                                 # empty bins are NaN in what the caller gets, and left out
    assert list(np.nonzero(~filled)[0]) == info["empty_bins_left_out"]
    assert np.array_equal(kc[filled], got["pk_k"]) and np.array_equal(pk[filled], got["pk"])
    assert np.array_equal(err[filled], got["pk_stddev"])
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(N ** 3, size=bench.DUMP_VOXELS, replace=False))
    assert np.array_equal(np.asarray(dx).reshape(-1)[idx].astype(np.float32), got["delta_x"])
    box.engine.close()
