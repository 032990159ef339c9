"""Host-side logic of the batched fits: the grouping of jobs into batches, per-fit hyper-parameters, what the
command line and the constructor refuse before the library is loaded, and the new symbols of the C ABI."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mfvi_plan_set_fits", "mfvi_perturb_input_fits", "mfvi_gaussian_nll_fits", "mfvi_elbo_update_fits_scratch_bytes",
               "mfvi_elbo_update_fits", "mfvi_ema_fits"]


@pytest.fixture()
def no_library(monkeypatch):
    """Loading the HIP library is an error for the duration of the test."""
    import mfvi_dip_mia_amd as M

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(M._lib, "lib", boom)
    return M


def test_grouping_mixed_shapes_order_and_sizes():
    from mfvi_dip_mia_amd.fanout import group_jobs
    a, b = ("den", (32, 32), 8, 20, 1), ("den", (64, 64), 8, 20, 1)
    assert group_jobs([a] * 4, 3) == [[0, 1, 2], [3]]                          # a second batch of one
    assert group_jobs([a] * 4, 16) == [[0, 1, 2, 3]]                           # N larger than the job count
    assert group_jobs([a, b, a, a, b, a, a], 3) == [[0, 2, 3], [1, 4], [5, 6]]  # mixed shapes never share a batch; order preserved
    assert group_jobs([a, ("sr",) + a[1:], a[:4] + (2,)], 8) == [[0], [1], [2]]  # task and K split batches too
    assert group_jobs([], 4) == []
    assert group_jobs([a, a], 1) == [[0], [1]]
    got = group_jobs([a, b] * 5, 4)
    assert sorted(i for g in got for i in g) == list(range(10)) and all(g == sorted(g) for g in got)
    assert [g[0] for g in got] == sorted(g[0] for g in got)
    with pytest.raises(ValueError):
        group_jobs([a], 0)


def test_scalar_and_sequence_hyper_parameters(no_library):
    from mfvi_dip_mia_amd import fitbatch as FB
    import numpy as np
    assert FB.per_fit(0.5, 3, "temp") == [0.5, 0.5, 0.5]
    assert FB.per_fit([1, 2, 3], 3, "lr") == [1.0, 2.0, 3.0]
    assert FB.per_fit(np.array([1e-6, 2e-6]), 2, "temp") == [1e-6, 2e-6]
    with pytest.raises(ValueError, match="sigma: 2 values for 3 fits"):
        FB.per_fit([1, 2], 3, "sigma")
    # the engine's rule, per fit: float32(sqrt(temp) * sigma + 1e-6)
    ps = FB.prior_sigmas([1e-6, 4e-6], [0.05, 0.1])
    assert ps == [float(np.float32(1e-3 * 0.05 + 1e-6)), float(np.float32(2e-3 * 0.1 + 1e-6))]
    temps, sigmas, lrs = FB.check_args(32, 32, 2, "den", 1, 1e-6, [0.1, 0.2], 1e-3, "per_fit")
    assert temps == [1e-6, 1e-6] and sigmas == [0.1, 0.2] and lrs == [1e-3, 1e-3]


def test_constructor_refusals_come_before_the_library(no_library):
    M = no_library
    for task in ("ct", "inp"):
        with pytest.raises(NotImplementedError):
            M.FitBatch(32, 32, 2, task=task)
    for kw in (dict(task="deblur"), dict(temp=[1.0, 2.0, 3.0]), dict(lr=[1e-3]), dict(sigma=[0.1] * 3), dict(init="zeros"), dict(K=0),
               dict(lr=0.0), dict(task="sr", sr_factor=5)):
        with pytest.raises(ValueError):
            M.FitBatch(32, 32, 2, **kw)
    with pytest.raises(ValueError):
        M.FitBatch(30, 32, 2)
    with pytest.raises(ValueError):
        M.FitBatch(32, 32, 0)


@pytest.mark.parametrize("extra,msg", [(["--bayes", "mcd"], "mean-field VI"), (["--bayes", "sgld"], "mean-field VI"), (["--task", "ct"], "denoising and super-resolution"),
                                       (["--task", "inpainting"], "denoising and super-resolution"), (["--param-dtype", "bf16"], "float32"),
                                       (["--predict-samples", "8"], "predict-samples"), (["--calibration"], "calibration"),
                                       (["--fits-per-launch", "-2"], "fits-per-launch")])
def test_argparse_refusals_without_the_library(no_library, tmp_path, capsys, extra, msg):
    M = no_library
    cfg = os.path.join(ROOT, "configs", "mfvi_den.json")
    with pytest.raises(SystemExit) as e:
        M.runner.main(["--config", cfg, "--save-path", str(tmp_path), "--fits-per-launch", "4"] + extra)
    assert e.value.code == 2
    assert msg in capsys.readouterr().err
    assert os.listdir(str(tmp_path)) == []


def test_header_and_ctypes_table_have_the_new_symbols():
    import mfvi_dip_mia_amd as M
    src = open(os.path.join(ROOT, "include", "mfvi_hip.h")).read()
    declared = set(re.findall(r"\b(mfvi_[a-z0-9_]+)\s*\(", src))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in M._lib.SIGNATURES, name
    assert "mfvi_fit_hyper" in src and re.search(r"#define\s+MFVI_ERR_FITS_UNSUPPORTED\s+\(-5\)", src)
    assert M._lib.ERR_FITS_UNSUPPORTED == -5
    assert re.search(r"#define\s+MFVI_ABI_VERSION\s+6\b", src)                  # additions only
    n_args = {"mfvi_plan_set_fits": 4, "mfvi_perturb_input_fits": 9, "mfvi_gaussian_nll_fits": 12, "mfvi_elbo_update_fits_scratch_bytes": 1,
              "mfvi_elbo_update_fits": 19, "mfvi_ema_fits": 10}
    for name, n in n_args.items():
        assert len(M._lib.SIGNATURES[name][1]) == n, name
    from mfvi_dip_mia_amd import _build
    assert "fits.hip" in _build.SOURCES
