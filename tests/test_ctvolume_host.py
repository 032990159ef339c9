"""Host-side logic of the CT volume: the group arithmetic, what the constructor and the command line refuse before the
library is loaded, the new symbols of the C ABI, and that FitBatch keeps refusing CT."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"mfvi_radon_mse_fits_scratch_bytes": 4, "mfvi_radon_mse_fits": 13}


@pytest.fixture()
def no_library(monkeypatch):
    """Loading the HIP library is an error for the duration of the test."""
    import mfvi_dip_mia_amd as M

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(M._lib, "lib", boom)
    return M


def test_ctvolume_is_exported():
    import mfvi_dip_mia_amd as M
    from mfvi_dip_mia_amd import ctvolume
    assert M.CtVolume is ctvolume.CtVolume and "CtVolume" in M.api.__all__
    assert callable(M.runner.run_ct_volume)


def test_group_arithmetic():
    """(first slice, slices, k0, fit0, samples) per group: rows start at slice g F, eps at global sample g F K, the perturbation at sample g F."""
    from mfvi_dip_mia_amd.ctvolume import groups
    assert groups(5, 2, 1) == [(0, 2, 0, 0, 2), (2, 2, 2, 2, 2), (4, 1, 4, 4, 1)]              # groups of 2, 2, 1
    assert groups(5, 2, 3) == [(0, 2, 0, 0, 6), (2, 2, 6, 2, 6), (4, 1, 12, 4, 3)]             # the tail: fewer samples, still a multiple of K
    assert groups(5, 5, 2) == [(0, 5, 0, 0, 10)]
    assert groups(4, 2, 1) == [(0, 2, 0, 0, 2), (2, 2, 2, 2, 2)]                               # no empty tail group
    assert groups(1, 1, 4) == [(0, 1, 0, 0, 4)]
    for D, F, K in ((32, 16, 1), (7, 3, 2), (100, 16, 1)):
        g = groups(D, F, K)
        assert [x[0] for x in g] == list(range(0, D, F)) and sum(x[1] for x in g) == D
        assert all(k0 == d0 * K and fit0 == d0 and n == nd * K and 1 <= nd <= F for d0, nd, k0, fit0, n in g)
    for bad in ((0, 1, 1), (3, 0, 1), (3, 1, 0)):
        with pytest.raises(ValueError):
            groups(*bad)


def test_check_args_values(no_library):
    from mfvi_dip_mia_amd import ctvolume as V
    S, F, temps, sigmas, lrs, theta = V.check_args(32, 5, 2, 1, 1e-6, [0.1, 0.2, 0.3, 0.4, 0.5], 1e-3, None, "per_fit")
    assert (S, F) == (32, 2) and temps == [1e-6] * 5 and sigmas == [0.1, 0.2, 0.3, 0.4, 0.5] and lrs == [1e-3] * 5
    assert theta == [float(t) for t in range(0, 180, 4)] and len(theta) == 45                # bayesian_optimization.py:545
    assert V.check_args((32, 32), 3, None, 2, 1.0, 0.1, 1e-3, [0.0, 90.0], "shared")[:2] == (32, 3)      # all slices in one launch set
    assert V.check_args(32, 3, 16, 2, 1.0, 0.1, 1e-3, [0.0], "per_fit")[1] == 3                  # F = min(slices_per_launch, n_slices)


def test_constructor_refusals_come_before_the_library(no_library):
    M = no_library
    for args, kw in ((((32, 48), 3), {}),                                # not square
                     ((30, 3), {}),                                       # S not a multiple of 4
                     ((32, 0), {}), ((32, 3), dict(K=0)),
                     ((32, 70000), {}),
                     ((32, 4096), dict(K=16)),                            # F K = 65536
                     ((32, 40000), dict(slices_per_launch=32768, K=2)),
                     ((32, 3), dict(slices_per_launch=0)),
                     ((32, 3), dict(temp=[1.0, 2.0])), ((32, 3), dict(sigma=[0.1] * 4)), ((32, 3), dict(lr=[1e-3])),
                     ((32, 3), dict(lr=0.0)), ((32, 3), dict(temp=-1.0)),
                     ((32, 3), dict(theta_deg=[])),
                     ((32, 3), dict(init="zeros"))):
        with pytest.raises(ValueError):
            M.CtVolume(*args, **kw)


def test_fitbatch_still_refuses_ct(no_library):
    M = no_library
    for task in ("ct", "inp"):
        with pytest.raises(NotImplementedError):
            M.FitBatch(32, 32, 2, task=task)


VOL = ["--task", "ct", "--ct-volume", "phantom:3"]


@pytest.mark.parametrize("argv,msg", [(VOL + ["--bayes", "mcd"], "--task ct --bayes mfvi"), (VOL + ["--bayes", "dip"], "--task ct --bayes mfvi"),
                                      (["--task", "denoising", "--ct-volume", "phantom:3"], "--task ct --bayes mfvi"),
                                      (["--ct-volume", "phantom:3"], "--task ct --bayes mfvi"),
                                      (VOL + ["--param-dtype", "bf16"], "float32"),
                                      (VOL + ["--fits-per-launch", "4"], "--fits-per-launch"),
                                      (VOL + ["--predict-samples", "8"], "--predict-samples"),
                                      (VOL + ["--calibration"], "--calibration"),
                                      (VOL + ["--bo-rounds", "2"], "--bo-rounds"),
                                      (VOL + ["--slices-per-launch", "0"], "--slices-per-launch"),
                                      (["--task", "ct", "--slices-per-launch", "2"], "--slices-per-launch"),
                                      (["--task", "ct", "--ct-volume", "phantom:0"], "phantom:D"),
                                      (["--task", "ct", "--ct-volume", "phantom:x"], "phantom:D"),
                                      (["--task", "ct", "--ct-volume", "stack.png"], ".npy")])
def test_argparse_refusals_without_the_library(no_library, tmp_path, capsys, argv, msg):
    M = no_library
    cfg = os.path.join(ROOT, "configs", "mfvi_ct.json")
    with pytest.raises(SystemExit) as e:
        M.runner.main(["--config", cfg, "--save-path", str(tmp_path)] + argv)
    assert e.value.code == 2
    assert msg in capsys.readouterr().err
    assert os.listdir(str(tmp_path)) == []


def test_fits_per_launch_still_refuses_ct(no_library, tmp_path, capsys):
    M = no_library
    with pytest.raises(SystemExit):
        M.runner.main(["--config", os.path.join(ROOT, "configs", "mfvi_ct.json"), "--save-path", str(tmp_path), "--task", "ct", "--fits-per-launch", "4"])
    assert "denoising and super-resolution" in capsys.readouterr().err and os.listdir(str(tmp_path)) == []


def test_parse_ct_volume():
    from mfvi_dip_mia_amd.runner import parse_ct_volume
    assert parse_ct_volume("phantom:12") == ("phantom", 12) and parse_ct_volume("a/b/stack.npy") == ("npy", "a/b/stack.npy")
    for bad in ("phantom", "phantom:", "phantom:-1", "stack.npz", ""):
        with pytest.raises(ValueError):
            parse_ct_volume(bad)


def test_header_and_ctypes_table_have_the_new_symbols():
    import mfvi_dip_mia_amd as M
    src = open(os.path.join(ROOT, "include", "mfvi_hip.h")).read()
    declared = set(re.findall(r"\b(mfvi_[a-z0-9_]+)\s*\(", src))
    for name, n in NEW_SYMBOLS.items():
        assert name in declared, name
        assert name in M._lib.SIGNATURES and len(M._lib.SIGNATURES[name][1]) == n, name
    assert M._lib.SIGNATURES["mfvi_radon_mse_fits_scratch_bytes"][0] is M._lib.SIGNATURES["mfvi_elbo_update_fits_scratch_bytes"][0]      # int64
    assert re.search(r"#define\s+MFVI_ABI_VERSION\s+6\b", src)                  # additions only
    from mfvi_dip_mia_amd import _build
    assert "radon_fits.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "radon_rows.h"))
    # the row loop exists once: both entry points call the header's
    for f in ("radon_planes.hip", "radon_fits.hip"):
        text = open(os.path.join(_build.CSRC, f)).read()
        assert "project_rows<PAIR>" in text and "floor(ix)" not in text, f
