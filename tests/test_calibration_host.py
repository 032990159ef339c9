"""CPU checks of the calibration feature: the uceloss golden agrees with its float64 restatement, the C ABI
declares and binds the mfvi_uce_* entry points, and the runner refuses --calibration for the method without uncertainty maps before
anything touches the GPU."""
import os
import re

import numpy as np
import pytest

import uce_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UCE_SYMBOLS = ["mfvi_uce_bins", "mfvi_uce_minmax", "mfvi_uce_ring_inputs", "mfvi_uce_scratch_bytes", "mfvi_uce_value"]


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_golden_matches_float64_restatement(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "uce.npz"))
    err, unc, bounds = g[tag + "_err"], g[tag + "_unc"], g[tag + "_bounds"]
    assert bounds.dtype == np.float32 and bounds.shape == (int(g["n_bins"]) + 1,)
    r = R.restate(err, unc, bounds)
    assert np.array_equal(r["count"], g[tag + "_count"])
    tol = R.tolerance(g[tag + "_ref_dev"])
    for j, o in enumerate(g["outliers"]):
        prop, e_b, u_b, uce = (g["%s_%s_o%d" % (tag, k, j)] for k in ("prop", "err", "unc", "uce"))
        assert np.array_equal(np.rint(prop.astype(np.float64) * r["n"]).astype(np.int64), r["count"])       # counts are exact
        k = R.kept(r, o)
        assert e_b.shape == u_b.shape == (int(k.sum()),) and prop.shape == (int(g["n_bins"]),) and uce.shape == (1,)
        assert np.abs(e_b - r["mean_err"][k]).max() <= tol * R.mean_scale(r)
        assert np.abs(u_b - r["mean_unc"][k]).max() <= tol * R.mean_scale(r)
        assert abs(float(uce[0]) - R.uce(r, o)) <= tol * R.uce_scale(r)
        assert abs(R.uce(r, o) - float(g["%s_uce64_o%d" % (tag, j)])) <= 1e-12 * R.uce_scale(r)


def test_golden_exercises_the_quirks(golden_dir):
    g = np.load(os.path.join(golden_dir, "uce.npz"))
    empty = dropped = False
    for tag in "abc":
        unc = g[tag + "_unc"].reshape(-1)
        count = g[tag + "_count"]
        if np.isnan(g[tag + "_range"]).all():        # range None: every pixel but the minimum is in a bin
            assert count.sum() == unc.size - int((unc == unc.min()).sum())
        else:
            assert count.sum() < unc.size
        empty |= bool((count == 0).any())
        dropped |= len(g[tag + "_err_o1"]) < int((count > 0).sum())
    assert empty and dropped
    assert {g[t + "_unc"].size % 4 == 0 for t in "abc"} == {True, False}       # both load paths of the kernels


def test_golden_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "uce.npz")) <= 200 * 1024


def test_abi_declares_and_binds_the_uce_entry_points():
    from mfvi_dip_mia_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mfvi_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = sorted(s for s in set(re.findall(r"\b(mfvi_[a-z0-9_]+)\s*\(", txt)) if s.startswith("mfvi_uce_"))
    assert declared == UCE_SYMBOLS
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("mfvi_uce_")) == UCE_SYMBOLS
    assert re.search(r"#define\s+MFVI_UCE_MAX_BINS\s+%d\b" % _lib.UCE_MAX_BINS, txt)


def _no_gpu():
    raise AssertionError("the library was loaded before the arguments were checked")


def test_calibration_rejected_for_dip_on_the_command_line(monkeypatch, capsys):
    from mfvi_dip_mia_amd import _lib, runner
    monkeypatch.setattr(_lib, "lib", _no_gpu)
    cfg = os.path.join(ROOT, "configs", "dip_den.json")
    with pytest.raises(SystemExit) as e:
        runner.main(["--task", "denoising", "--bayes", "dip", "--config", cfg, "--calibration"])
    assert e.value.code == 2
    assert "--calibration" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        runner.main(["--task", "denoising", "--bayes", "mfvi", "--config", os.path.join(ROOT, "configs", "mfvi_den.json"), "--calibration",
                     "--calibration-bins", "1000"])
    assert e.value.code == 2


def test_calibration_rejected_by_the_runner_functions(monkeypatch):
    from mfvi_dip_mia_amd import _lib, runner
    monkeypatch.setattr(_lib, "lib", _no_gpu)
    with pytest.raises(ValueError, match="uncertainty maps"):
        runner.run_den_dip(imsize=(32, 32), num_iter=1, save=False, calibration=True)
    with pytest.raises(ValueError, match="uncertainty maps"):
        runner.run_inp_dip(imsize=(32, 32), num_iter=1, save=False, calibration=True)
    with pytest.raises(ValueError, match="calibration_bins"):
        runner.run_den_mfvi(imsize=(32, 32), num_iter=1, save=False, calibration=True, calibration_bins=0)


def test_cpu_tensors_and_mismatched_sizes_are_rejected(monkeypatch):
    import torch
    from mfvi_dip_mia_amd import _lib
    from mfvi_dip_mia_amd.calibration import uceloss, host_bounds
    monkeypatch.setattr(_lib, "lib", _no_gpu)
    with pytest.raises(NotImplementedError):
        uceloss(torch.ones(8), torch.ones(8))
    b = host_bounds(0.25, 1.0, 15)
    assert b.dtype == torch.float32 and torch.equal(b, torch.linspace(0.25, 1.0, 16))
