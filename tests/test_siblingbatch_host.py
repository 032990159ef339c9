"""Host-side logic of the batched DIP / MC-dropout / SGLD fits: what SiblingBatch and --sibling-fits refuse before the
library is loaded, per-fit hyper-parameters, the new symbols of the C ABI."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"mfvi_plan_set_fits_points": 2, "mfvi_plan_set_fit_dropout": 3, "mfvi_mse_channel_fits": 14, "mfvi_sibling_update_fits": 17,
               "mfvi_add_normal_fits": 12}


@pytest.fixture()
def no_library(monkeypatch):
    """Loading the HIP library is an error for the duration of the test."""
    import mfvi_dip_mia_amd as M

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(M._lib, "lib", boom)
    return M


def test_check_args_refusals_and_hyper_parameters(no_library):
    from mfvi_dip_mia_amd import siblingbatch as SB
    lrs, wds, ps, gammas = SB.check_args(32, 32, 2, "mcd", "den", 2, 1e-3, [0.0, 1e-4], [0.1, 0.3], 0.9, "per_fit")
    assert (lrs, wds, ps, gammas) == ([1e-3, 1e-3], [0.0, 1e-4], [0.1, 0.3], [1.0, 1.0])      # no scheduler outside SGLD: a constant rate
    lrs, wds, ps, gammas = SB.check_args(32, 32, 2, "sgld", "sr", 1, [1e-3, 2e-3], 0.5, 0.3, [0.99, 0.999], "shared")
    assert (lrs, wds, ps, gammas) == ([1e-3, 2e-3], [0.5, 0.5], [0.0, 0.0], [0.99, 0.999])    # no dropout outside MC dropout
    assert SB.check_args(32, 32, 3, "dip", "den", 1, 1e-3, 0.0, 0.3, 0.996, "per_fit")[2:] == ([0.0] * 3, [1.0] * 3)
    ok = (32, 32, 2, "mcd", "den", 1, 1e-3, 0.0, 0.3, 0.996, "per_fit")

    def with_(**kw):
        names = ("H", "W", "n_fits", "method", "task", "K", "lr", "weight_decay", "dropout_p", "gamma", "init")
        d = dict(zip(names, ok)); d.update(kw)
        return tuple(d[k] for k in names)
    for args, msg in ((with_(method="mfvi"), "method 'mfvi'"),
                      (with_(task="deblur"), "task 'deblur'"),
                      (with_(H=30), "multiples of 4"),
                      (with_(n_fits=0), "at least 1 each"),
                      (with_(K=0), "at least 1 each"),
                      (with_(n_fits=256, K=256), "n_fits \\* K < 65536"),
                      (with_(lr=[1e-3] * 3), "lr: 3 values for 2 fits"),
                      (with_(weight_decay=[0.0]), "weight_decay: 1 values for 2 fits"),
                      (with_(dropout_p=[0.1, 0.2, 0.3]), "dropout_p: 3 values for 2 fits"),
                      (with_(gamma=[0.9]), "gamma: 1 values for 2 fits"),
                      (with_(lr=0.0), "lr must be > 0"),
                      (with_(weight_decay=-1e-4), "weight_decay >= 0"),
                      (with_(dropout_p=1.0), "dropout_p outside"),
                      (with_(dropout_p=[0.1, -0.1]), "dropout_p outside"),
                      (with_(gamma=0.0), "gamma outside"),
                      (with_(gamma=1.5), "gamma outside"),
                      (with_(init="zeros"), "init")):
        with pytest.raises(ValueError, match=msg):
            SB.check_args(*args)
    for task in ("ct", "inp"):
        with pytest.raises(NotImplementedError, match="denoising and super-resolution"):
            SB.check_args(*with_(task=task))
    with pytest.raises(NotImplementedError, match="float32"):
        SB.check_args(*ok, param_dtype="bf16")


def test_constructor_refusals_come_before_the_library(no_library):
    M = no_library
    assert M.SiblingBatch is M.siblingbatch.SiblingBatch and "SiblingBatch" in M.api.__all__
    for kw in (dict(lr=[1e-3]), dict(init="zeros"), dict(K=0), dict(lr=0.0), dict(dropout_p=1.0), dict(gamma=2.0)):
        with pytest.raises(ValueError):
            M.SiblingBatch(32, 32, 2, "mcd", **kw)
    with pytest.raises(ValueError):
        M.SiblingBatch(32, 32, 2, "vi")
    with pytest.raises(ValueError):
        M.SiblingBatch(32, 32, 2, "dip", task="sr", sr_factor=5)
    for task in ("ct", "inp"):
        with pytest.raises(NotImplementedError):
            M.SiblingBatch(32, 32, 2, "sgld", task=task)
    with pytest.raises(NotImplementedError):
        M.SiblingBatch(32, 32, 2, "dip", param_dtype="bf16")


@pytest.mark.parametrize("extra,msg", [
    (["--bayes", "mfvi"], "--sibling-fits batches the DIP, MC-dropout and SGLD fits"),
    (["--bayes", "mcd", "--task", "ct"], "--sibling-fits serves denoising and super-resolution, not ct"),
    (["--bayes", "sgld", "--task", "inpainting"], "--sibling-fits serves denoising and super-resolution, not inpainting"),
    (["--bayes", "mcd", "--fits-per-launch", "4"], "--sibling-fits does not combine with --fits-per-launch"),
    (["--bayes", "mcd", "--inpaint-fits", "4"], "--sibling-fits does not combine with --inpaint-fits"),
    (["--bayes", "dip", "--ct-volume", "phantom:4"], "--sibling-fits does not combine with --ct-volume"),
    (["--bayes", "mcd", "--predict-samples", "8"], "--sibling-fits does not combine with --predict-samples"),
    (["--bayes", "sgld", "--calibration"], "--sibling-fits does not combine with --calibration"),
    (["--bayes", "mcd", "--param-dtype", "bf16"], "--sibling-fits takes float32 parameters (--param-dtype f32)"),
    (["--bayes", "mcd", "--sibling-fits", "-2"], "--sibling-fits -2: 0 (off) or the number of fits per launch")])
def test_argparse_refusals_without_the_library(no_library, tmp_path, capsys, extra, msg):
    M = no_library
    cfg = os.path.join(ROOT, "configs", "mcd_den.json")
    with pytest.raises(SystemExit) as e:
        M.runner.main(["--config", cfg, "--save-path", str(tmp_path), "--sibling-fits", "4"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert msg in " ".join(err.split()), err                                   # (argparse wraps its message: compare with the whitespace folded)
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("bayes", ["mcd", "sgld"])
def test_fits_per_launch_still_refuses_the_siblings(no_library, tmp_path, capsys, bayes):
    M = no_library
    with pytest.raises(SystemExit) as e:
        M.runner.main(["--config", os.path.join(ROOT, "configs", "%s_den.json" % bayes), "--save-path", str(tmp_path), "--bayes", bayes, "--fits-per-launch", "4"])
    assert e.value.code == 2 and "mean-field VI" in capsys.readouterr().err
    assert os.listdir(str(tmp_path)) == []


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
    decl = re.search(r"\bmfvi_plan_set_fits\s*\(([^;]*)\)\s*;", src).group(1)
    assert len(decl.split(",")) == 4 and len(M._lib.SIGNATURES["mfvi_plan_set_fits"][1]) == 4
    assert re.search(r"typedef struct \{ double lr, gamma; float weight_decay, lr_floor; \} mfvi_sibling_hyper;", src)
    assert "sibling_fits.hip" in M._build.SOURCES and os.path.exists(os.path.join(ROOT, "mfvi-dip-mia_amd", "csrc", "sibling_fits.hip"))


def test_sibling_runners_publish_their_defaults():
    """run_sibling_batch fills what a job leaves out from the single-fit runner's defaults (the reference's keyword defaults)."""
    from mfvi_dip_mia_amd import runner
    assert runner.run_den_mcd.defaults == dict(dropout_p=0.3, weight_decay=3e-4)
    assert runner.run_sr_sgld.defaults == dict(imsize=(512, 512), input_depth=32, gamma=0.996, weight_decay=1e-4)
    assert runner.run_den_dip.defaults == {}
