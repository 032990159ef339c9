"""bench.py --dump-outputs: what the last timed iteration computed, as DIR/<name>.npy within a size budget; and the plain run's line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_write_outputs_budget(tmp_path):
    import bench
    rng = np.random.default_rng(3)
    outs = {"out": rng.standard_normal((4, 2, 64, 64)).astype(np.float32), "mu": rng.standard_normal(5000).astype(np.float32),
            "losses": np.array([1.0, 2.0, 3.0]), "count": np.arange(10, dtype=np.int32)}
    # under the budget: every array as it is, anything else than float32 / float64 as float32
    bench.write_outputs(outs, str(tmp_path / "a"))
    for k, v in outs.items():
        a = np.load(tmp_path / "a" / (k + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.shape == v.shape and np.array_equal(a, v)
    # over the budget: the largest array becomes a fixed, seeded sample of its elements — the same one on every call
    budget = 40000
    b1 = bench.write_outputs(outs, str(tmp_path / "b"), budget=budget)
    b2 = bench.write_outputs(outs, str(tmp_path / "c"), budget=budget)
    assert sum(a.nbytes for a in b1.values()) <= budget
    assert 0 < b1["out"].size < outs["out"].size and np.array_equal(b1["out"], b2["out"])
    assert np.isin(b1["out"], outs["out"]).all()
    assert np.array_equal(np.load(tmp_path / "b" / "out.npy"), b1["out"])
    assert np.array_equal(np.load(tmp_path / "b" / "mu.npy"), outs["mu"])


def test_tilings_table_covers_the_configs():
    """Every BASELINE config's plan (at its samples per launch) has its tilings in the committed table: the benchmark never searches,
    so two runs with the same arguments compute the same sums in the same order."""
    import bench
    from mfvi_dip_mia_amd.engine import INP_NET
    from mfvi_dip_mia_amd.program import skip_program
    table = json.load(open(bench.TILINGS))
    for name, cfg in bench.CONFIGS.items():
        kw = dict(INP_NET) if cfg["task"] == "inp" else {}
        prog = skip_program(cfg["size"], cfg["size"], cfg["input_depth"], {"ct": 1, "inp": 4}.get(cfg["task"], 2), **kw)[0]
        n_conv = sum(o["type"] == 1 for o in prog.ops)
        entry = table.get(bench.plan_signature(prog, cfg.get("spl", cfg["k"])))
        assert entry is not None, name
        assert len(entry["tunes"]) == n_conv and all(len(t) == 3 for t in entry["tunes"].values()), name


def test_profile_all_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--profile-all"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--full" in r.stderr


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "cfg1", "--steps", "3", "--warmup", "1", "--dump-outputs", out_dir]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path):
    d1, d2 = str(tmp_path / "one"), str(tmp_path / "two")
    res = _plain_run(d1)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["config"]["tilings"] == "table"
    assert abs(res["value"] - 4 * 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]          # cfg1: K = 4 MC passes per step
    for key in ("roofline", "fwd_only_mc_passes_per_sec", "unfused_gpu_baseline", "cpu_baseline"):
        assert key not in res                                                          # --full only
    a = {k: np.load(os.path.join(d1, k + ".npy")) for k in ("out", "mu", "rho", "bn", "grads", "losses")}
    assert a["out"].shape == (4, 2, 128, 128) and a["out"].dtype == np.float32
    assert a["mu"].shape == a["rho"].shape and a["grads"].size == a["mu"].size + a["rho"].size + a["bn"].size
    assert np.allclose(a["losses"], [res["final_nll"], res["final_kl"], res["final_loss"]], rtol=1e-12, atol=0)
    assert all(np.isfinite(v).all() for v in a.values())
    # the same arguments: the same inputs and the same tilings, so the same outputs
    _plain_run(d2)
    for k, v in a.items():
        w = np.load(os.path.join(d2, k + ".npy"))
        assert w.shape == v.shape, k
        assert np.abs(w - v).max() <= 1e-6 * max(np.abs(v).max(), 1e-30), k


@pytest.mark.gpu
def test_plan_signature_is_the_tune_cache_key(tmp_path):
    """bench.plan_signature files a plan under the key program.Plan.autotune writes to its cache."""
    import bench
    from mfvi_dip_mia_amd.engine import ElboEngine
    eng = ElboEngine(128, 128, task="den", K=4, autotune=False)
    cache = str(tmp_path / "tunes.json")
    eng.plan.autotune(eng.mu, eng.rho, eng.bn, eng.z0, eng.chunk, cache=cache)
    saved = json.load(open(cache))
    assert saved["sig"] == bench.plan_signature(eng.prog, eng.chunk)
    assert saved["tunes"] == bench.plan_tilings(eng.plan)
