"""Host-side logic of the batched posterior predictive: the chunk / group planner, what predict() of the batch classes
and --batch-predict-samples refuse before the library is loaded, the new symbols of the C ABI."""
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"mfvi_plan_set_fits_sample_stride": 2, "mfvi_predictive_acc_doubles_fits": 4, "mfvi_predictive_accumulate_fits": 13,
               "mfvi_predictive_finalize_fits": 18}


@pytest.fixture()
def no_library(monkeypatch):
    """Loading the HIP library is an error for the duration of the test."""
    import mfvi_dip_mia_amd as M

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(M._lib, "lib", boom)
    return M


def test_header_and_ctypes_table_have_the_new_symbols():
    import mfvi_dip_mia_amd as M
    src = open(os.path.join(ROOT, "include", "mfvi_hip.h")).read()
    declared = set(re.findall(r"\b(mfvi_[a-z0-9_]+)\s*\(", src))
    for name, n in NEW_SYMBOLS.items():
        assert name in declared, name
        assert name in M._lib.SIGNATURES, name
        assert len(M._lib.SIGNATURES[name][1]) == n, name
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, src).group(1)
        assert len(decl.split(",")) == n, (name, decl)                        # the header's argument count is the table's
    assert re.search(r"#define\s+MFVI_ABI_VERSION\s+6\b", src)                  # additions only
    assert M._lib.SIGNATURES["mfvi_predictive_acc_doubles_fits"][0] is M._lib.SIGNATURES["mfvi_predictive_acc_doubles"][0]      # int64 both
    assert hasattr(M.program.Plan, "set_fits_sample_stride")
    for cls in (M.FitBatch, M.CtVolume, M.InpaintBatch, M.SiblingBatch):
        assert callable(getattr(cls, "predict")), cls


def test_planner_chunks_and_groups(no_library):
    from mfvi_dip_mia_amd.batchpredict import plan_chunks
    assert plan_chunks(3, 7, 3, 3) == [(0, 3, 0, 3), (0, 3, 1, 3), (0, 3, 2, 1)]                      # N not a multiple of S: a last chunk of 1
    assert plan_chunks(3, 7, 2, 3) == [(0, 2, 0, 3), (0, 2, 1, 3), (0, 2, 2, 1), (2, 1, 0, 3), (2, 1, 1, 3), (2, 1, 2, 1)]      # F not a multiple of G
    assert plan_chunks(4, 6, 2, 3) == [(0, 2, 0, 3), (0, 2, 1, 3), (2, 2, 0, 3), (2, 2, 1, 3)]
    assert plan_chunks(1, 2, 1, 64) == [(0, 1, 0, 2)]                                                # a chunk larger than N
    assert plan_chunks(5, 4, 5, 1) == [(0, 5, c, 1) for c in range(4)]
    for F, N, G, S in ((16, 64, 16, 4), (7, 13, 3, 5), (3, 2, 1, 1)):
        calls = plan_chunks(F, N, G, S)
        for f in range(F):      # every fit draws every sample 0 .. N-1 exactly once, in increasing order
            ks = [c * S + s for g0, g, c, n_use in calls if g0 <= f < g0 + g for s in range(n_use)]
            assert ks == list(range(N)), (F, N, G, S, f)
        assert all(1 <= n_use <= S and 1 <= g <= G for _, g, _, n_use in calls)


def owner(**kw):
    d = dict(F=3, H=32, W=32, task="den")
    d.update(kw)
    d.setdefault("n_rows", d["F"])                     # the rows of a batch are its F fits, except on a CtVolume
    return types.SimpleNamespace(**d)


def test_predict_arguments_are_checked_without_the_library(no_library):
    from mfvi_dip_mia_amd import batchpredict as B
    from mfvi_dip_mia_amd.predictive import DEFAULT_STEP
    gt = np.zeros((32, 32), np.float32)
    assert B.check_args(owner(), 7) == (7, 7, 3, DEFAULT_STEP, None, None)
    assert B.check_args(owner(F=16), 64)[1:3] == (4, 16)                                             # S = 64 // G: at most 64 samples in the workspace
    assert B.check_args(owner(F=2, D=16, S=32, n_rows=16, H=32, W=32, task="ct"), 64)[1:3] == (32, 2)                       # CtVolume: D slices, G = its slices per launch
    assert B.check_args(owner(F=100), 7)[1] == 1
    assert B.check_args(owner(), 7, target=gt, chunk=3, fits_per_call=2, step=5, calibration=True) == (7, 3, 2, 5, {}, "shared")
    assert B.check_args(owner(), 7, target=np.zeros((1, 32, 32)))[5] == "shared"
    assert B.check_args(owner(), 7, target=np.zeros((3, 32, 32)))[5] == "per_fit"
    assert B.check_args(owner(), 7, target=np.zeros((3, 1, 32, 32)))[5] == "per_fit"
    assert B.check_args(owner(task="inp", F=2), 7, target=np.zeros((3, 32, 32)))[5] == "shared"
    assert B.check_args(owner(task="inp", F=2), 7, target=np.zeros((2, 3, 32, 32)), calibration=dict(n_bins=5))[4:] == (dict(n_bins=5), "per_fit")
    assert B.check_args(owner(method="mcd"), 4)[0] == 4
    for kw, msg in ((dict(n_samples=1), "at least 2 samples"),
                    (dict(n_samples=0), "at least 2 samples"),
                    (dict(n_samples=7, chunk=0), "chunk=0"),
                    (dict(n_samples=7, chunk=-2), "chunk=-2"),
                    (dict(n_samples=7, fits_per_call=0), "fits_per_call=0 outside 1..3"),
                    (dict(n_samples=7, fits_per_call=4), "fits_per_call=4 outside 1..3"),
                    (dict(n_samples=7, step=-1), "32-bit"),
                    (dict(n_samples=7, step=2 ** 32), "32-bit"),
                    (dict(n_samples=7, target=np.zeros((32, 31))), "target of shape"),
                    (dict(n_samples=7, target=np.zeros((2, 32, 32))), "target of shape"),
                    (dict(n_samples=7, target=np.zeros((3, 3, 32, 32))), "target of shape"),
                    (dict(n_samples=7, calibration=True), "pass target"),
                    (dict(n_samples=7, calibration=dict(n_bins=5)), "pass target"),
                    (dict(n_samples=7, target=gt, calibration=dict(bins=5)), "n_bins and range"),
                    (dict(n_samples=7, chunk=65536), "below 65536")):
        with pytest.raises(ValueError, match=msg):
            B.check_args(owner(), **kw)
        with pytest.raises(ValueError, match=msg):                            # and predict_fits raises it before anything else
            B.predict_fits(owner(), **kw)
    with pytest.raises(ValueError, match="target of shape"):
        B.check_args(owner(task="inp"), 7, target=gt)                          # inpainting: [3, H, W]
    with pytest.raises(ValueError, match="deterministic"):
        B.predict_fits(owner(method="dip"), 4)
    with pytest.raises(NotImplementedError, match="iterates"):
        B.predict_fits(owner(method="sgld"), 4)


def test_batch_constructors_still_refuse_before_the_library(no_library):
    M = no_library
    with pytest.raises(ValueError):
        M.FitBatch(32, 32, 2, lr=[1e-3])
    with pytest.raises(ValueError):
        M.CtVolume(32, 3, slices_per_launch=0)
    with pytest.raises(ValueError):
        M.InpaintBatch(32, 32, 2, K=0)
    with pytest.raises(ValueError):
        M.SiblingBatch(32, 32, 2, "mcd", dropout_p=1.0)
    with pytest.raises(NotImplementedError):
        M.SiblingBatch(32, 32, 2, "mcd", task="ct")


@pytest.mark.parametrize("config,extra,msg", [
    ("mfvi_den.json", ["--batch-predict-samples", "4"], "they need --fits-per-launch, --ct-volume, --inpaint-fits or --sibling-fits"),
    ("mfvi_den.json", ["--batch-calibration"], "they need --fits-per-launch, --ct-volume, --inpaint-fits or --sibling-fits"),
    ("mfvi_den.json", ["--batch-predict-samples", "4", "--predict-samples", "4"], "they need --fits-per-launch"),
    ("mfvi_den.json", ["--fits-per-launch", "3", "--batch-predict-samples", "1"], "--batch-predict-samples 1: 0 (off) or at least 2"),
    ("mfvi_den.json", ["--fits-per-launch", "3", "--batch-predict-samples", "-3"], "--batch-predict-samples -3: 0 (off) or at least 2"),
    ("mfvi_den.json", ["--fits-per-launch", "3", "--batch-calibration"], "--batch-calibration calibrates the posterior predictive maps"),
    ("mfvi_den.json", ["--fits-per-launch", "3", "--batch-predict-samples", "4", "--batch-calibration", "--calibration-bins", "0"], "--calibration-bins 0 outside"),
    ("mfvi_den.json", ["--fits-per-launch", "3", "--batch-predict-samples", "4", "--predict-samples", "4"], "--fits-per-launch does not combine with --predict-samples"),
    ("mcd_den.json", ["--bayes", "dip", "--sibling-fits", "3", "--batch-predict-samples", "4"], "need a posterior to draw from (--bayes mcd), not dip"),
    ("mcd_den.json", ["--bayes", "sgld", "--sibling-fits", "3", "--batch-predict-samples", "4", "--batch-calibration"], "need a posterior to draw from (--bayes mcd), not sgld"),
    ("mcd_den.json", ["--bayes", "mcd", "--sibling-fits", "3", "--batch-predict-samples", "1"], "--batch-predict-samples 1: 0 (off) or at least 2")])
def test_argparse_refusals_without_the_library(no_library, tmp_path, capsys, config, extra, msg):
    M = no_library
    cfg = os.path.join(ROOT, "configs", config)
    with pytest.raises(SystemExit) as e:
        M.runner.main(["--config", cfg, "--save-path", str(tmp_path)] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert msg in " ".join(err.split()), err                                   # (argparse wraps its message: compare with the whitespace folded)
    assert os.listdir(str(tmp_path)) == []


def test_batch_runners_check_their_predict_arguments(no_library):
    from mfvi_dip_mia_amd import runner
    with pytest.raises(ValueError, match="at least 2 draws"):
        runner.run_fit_batch("den", [], batch_predict_samples=1)
    with pytest.raises(ValueError, match="batch_predict_samples >= 2"):
        runner.run_ct_volume("phantom:2", 1e-6, 0.05, batch_calibration_bins=5)
    with pytest.raises(ValueError, match="only MC dropout"):
        runner.run_sibling_batch("den", "dip", [], batch_predict_samples=4)
