"""Host-side checks of the forward direction of the KL term: the float64 restatement against the reference's
recorded values and autograd gradients (tests/golden/kl_forward.npz, scripts/make_golden_kl.py), the reference's own float32 error, the
new symbols of the C ABI, and what the engine, the batches and the CLI refuse before the library is loaded."""
import contextlib
import io
import os
import re

import numpy as np
import pytest

import kl_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"mfvi_kl_typed": 8, "mfvi_kl_backward_typed": 10, "mfvi_elbo_update_typed": 18, "mfvi_elbo_update_guarded_typed": 20,
               "mfvi_elbo_update_bf16_typed": 21, "mfvi_elbo_update_fits_typed": 20}
# the tolerances of the project's KL tests (tests/test_gpu_parity.py:308, 311): value 1e-6 relative, gradients relerr < 1e-5
TOL_VALUE, TOL_GRAD = 1e-6, 1e-5


@pytest.fixture(scope="module")
def gold(golden_dir):
    path = os.path.join(golden_dir, "kl_forward.npz")
    assert os.path.getsize(path) <= 200 * 1024
    return np.load(path, allow_pickle=False)


@pytest.fixture()
def no_library(monkeypatch):
    """Loading the HIP library is an error for the duration of the test."""
    import mfvi_dip_mia_amd as M

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(M._lib, "lib", boom)
    return M


def test_layer_cases_are_what_the_issue_sets(gold):
    assert list(R.LAYER_CASES) == ["c1", "c2", "c3", "c4", "c5"] and (R.N_W, R.N_B) == (1031, 7)
    for name, (sigma, m0, _) in R.LAYER_CASES.items():
        mu, rho = R.case_inputs(gold, name)
        assert mu.dtype == rho.dtype == np.float32 and mu.shape == rho.shape == (R.N_W + R.N_B,)
        assert gold[name + "_prior"].dtype == np.float32
        assert gold[name + "_prior"][0] == np.float32(m0) and gold[name + "_prior"][1] == np.float32(sigma + 1e-6)      # modules/module.py:38
    assert abs(float(gold["c2_prior"][1]) - 1.011e-6) < 1e-9 and gold["c3_prior"][0] == 0.25
    rho4 = gold["c4_rho"]
    assert (rho4 == 15.0).sum() == 3 and (rho4 == -20.0).sum() == 3 and 1.5 < rho4.std() < 3.5      # both softplus tails


def test_restatement_matches_the_reference_in_float64(gold):
    for name in ("c1", "c2", "c3", "c4"):
        mu, rho = R.case_inputs(gold, name)
        m0, s0 = (float(v) for v in gold[name + "_prior"])
        v, dm, dr = R.kl_forward(mu, rho, m0, s0)
        assert abs(v - float(gold[name + "_kl64"])) <= 1e-12 * abs(float(gold[name + "_kl64"])), name
        assert R.relerr(dm, gold[name + "_dmu64"]) <= 1e-12 and R.relerr(dr, gold[name + "_drho64"]) <= 1e-12, name
    # the net case: the float64 sum over the layers, from the stored tensors
    keys = [str(k) for k in gold["net_keys"]]
    tot = 0.0
    for i in range(0, len(keys), 2):
        assert keys[i].endswith("_mu") and keys[i + 1] == keys[i][:-2] + "rho"
        tot += R.kl_forward(gold["net_p%d" % i].ravel(), gold["net_p%d" % (i + 1)].ravel(), *(float(v) for v in gold["net_prior"]))[0]
    assert abs(tot - float(gold["net_kl64"])) <= 1e-12 * tot


def test_reference_float32_sits_inside_the_tolerances(gold):
    for name in ("c1", "c2", "c3", "c4"):
        v64 = float(gold[name + "_kl64"])
        assert abs(float(gold[name + "_kl"]) - v64) <= TOL_VALUE * abs(v64), name
        assert R.relerr(gold[name + "_dmu"], gold[name + "_dmu64"]) < TOL_GRAD and R.relerr(gold[name + "_drho"], gold[name + "_drho64"]) < TOL_GRAD, name
    # an arbitrary non-'reverse' string is the forward direction (modules/module.py:76-80): bit for bit case 1
    for k in ("_kl", "_dmu", "_drho"):
        assert np.array_equal(gold["c5" + k], gold["c1" + k])
    assert abs(float(gold["net_kl"]) - float(gold["net_kl64"])) <= TOL_VALUE * float(gold["net_kl64"])
    assert abs(float(gold["net_layer_kl"].astype(np.float64).sum()) - float(gold["net_kl64"])) <= TOL_VALUE * float(gold["net_kl64"])
    assert len(gold["net_layers"]) == len(gold["net_layer_kl"]) == 11


def test_the_two_directions_differ_and_agree_where_they_must():
    rng = np.random.default_rng(0)
    mu, rho = 0.1 * rng.standard_normal(50), -3.0 + rng.standard_normal(50)
    f, r = R.kl_forward(mu, rho, 0.0, 0.1), R.kl_reverse(mu, rho, 0.0, 0.1)
    assert f[0] > 0 and r[0] > 0 and abs(f[0] - r[0]) > 1e-3 * r[0]
    # posterior = prior: both are zero with zero gradients
    s0 = 0.1
    rho0 = np.full(4, np.log(np.expm1(s0)))
    for fn in (R.kl_forward, R.kl_reverse):
        v, dm, dr = fn(np.zeros(4), rho0, 0.0, s0)
        assert abs(v) < 1e-12 and np.abs(dm).max() < 1e-12 and np.abs(dr).max() < 1e-12
    # central differences of the forward value
    h = 1e-6
    for i in (0, 7, 49):
        e = np.zeros(50); e[i] = h
        assert abs((R.kl_forward(mu + e, rho, 0.0, 0.1)[0] - R.kl_forward(mu - e, rho, 0.0, 0.1)[0]) / (2 * h) - f[1][i]) < 1e-5 * max(1.0, abs(f[1][i]))
        assert abs((R.kl_forward(mu, rho + e, 0.0, 0.1)[0] - R.kl_forward(mu, rho - e, 0.0, 0.1)[0]) / (2 * h) - f[2][i]) < 1e-5 * max(1.0, abs(f[2][i]))


def test_header_and_ctypes_agree_on_the_new_symbols():
    import mfvi_dip_mia_amd as M
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mfvi_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+MFVI_ABI_VERSION\s+6\b", txt)          # additions only
    assert re.search(r"#define\s+MFVI_KL_REVERSE\s+0\b", txt) and re.search(r"#define\s+MFVI_KL_FORWARD\s+1\b", txt)
    assert (M._lib.KL_REVERSE, M._lib.KL_FORWARD) == (0, 1) and M.rowbatch.KL_TYPES == ("reverse", "forward")
    for name, n_args in NEW_SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(M._lib.SIGNATURES[name][1]), name
        twin = name[:-len("_typed")]
        assert len(M._lib.SIGNATURES[twin][1]) == n_args - 1, name      # the twin's arguments and the direction


def test_library_exports_the_new_symbols():
    import ctypes
    import mfvi_dip_mia_amd as M
    M.build()
    lib = ctypes.CDLL(M._lib.LIB_PATH)
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    assert M._lib.lib().mfvi_abi_version() == 6


def test_check_kl_type():
    from mfvi_dip_mia_amd.rowbatch import check_kl_type
    assert check_kl_type("reverse") == "reverse" and check_kl_type("forward") == "forward"
    assert check_kl_type("forward", 3) == ["forward"] * 3 and check_kl_type(("forward", "reverse", "forward"), 3) == ["forward", "reverse", "forward"]
    assert check_kl_type(np.asarray(["reverse", "forward"]), 2) == ["reverse", "forward"]
    for bad in ("sideways", "fwd", "", None, 1):
        with pytest.raises(ValueError, match="kl_type"):
            check_kl_type(bad)
    with pytest.raises(ValueError, match="2 values for 3 fits"):
        check_kl_type(["forward", "reverse"], 3)
    with pytest.raises(ValueError, match="kl_type"):
        check_kl_type(["forward", "reverse"])
    with pytest.raises(ValueError, match="'sideways'"):
        check_kl_type(["forward", "sideways"], 2)


def test_refusals_come_before_the_library(no_library):
    M = no_library
    from mfvi_dip_mia_amd.engine import ElboEngine, SiblingEngine
    from mfvi_dip_mia_amd import runner
    with pytest.raises(ValueError, match="kl_type='sideways'"):
        ElboEngine(32, 32, kl_type="sideways")
    with pytest.raises(ValueError, match="kl_type"):
        ElboEngine(32, 32, task="ct", kl_type=["forward", "reverse"])
    with pytest.raises(TypeError, match="kl_type"):
        SiblingEngine(32, 32, method="dip", kl_type="forward")            # no KL term, no such argument
    for make in (lambda **kw: M.FitBatch(32, 32, 3, **kw), lambda **kw: M.CtVolume(32, 3, **kw), lambda **kw: M.InpaintBatch(192, 192, 3, **kw)):
        with pytest.raises(ValueError, match="kl_type='sideways'"):
            make(kl_type="sideways")
        with pytest.raises(ValueError, match="kl_type: 2 values for 3 fits"):
            make(kl_type=["forward", "reverse"])
        with pytest.raises(ValueError, match="kl_type='sideways'"):
            make(kl_type=["forward", "reverse", "sideways"])
    with pytest.raises(TypeError):
        M.SiblingBatch(32, 32, 3, "dip", kl_type="forward")
    # the runners: refused before a run directory exists
    for fn, kw in ((runner.run_den_mfvi, dict(kl_type="sideways")), (runner.run_ct_mfvi, dict(kl_type="fwd")), (runner.run_inp_mfvi, dict(kl_type="sideways")),
                   (runner.run_den_dip, dict(kl_type="forward")), (runner.run_sr_sgld, dict(kl_type="forward")), (runner.run_inp_mcd, dict(kl_type="forward"))):
        with pytest.raises(ValueError, match="kl_type"):
            fn(save_path="/nonexistent/never/made", **kw)


@pytest.mark.parametrize("tail, msg", [
    (("--kl-type", "forward", "--bayes", "dip"), "--kl-type forward chooses the direction of mean-field VI's KL term (--bayes mfvi); dip has no KL term"),
    (("--kl-type", "forward", "--bayes", "mcd", "--task", "ct"), "mcd has no KL term"),
    (("--kl-type", "forward", "--bayes", "sgld", "--sibling-fits", "2"), "sgld has no KL term"),
    (("--kl-type", "sideways"), "invalid choice: 'sideways'"),
    # every older refusal is reported first
    (("--kl-type", "forward", "--bayes", "dip", "--predict-samples", "4"), "--predict-samples needs a posterior to draw from"),
    (("--kl-type", "forward", "--bayes", "dip", "--tv-weight", "-0.1"), "--tv-weight -0.1: finite and >= 0"),
])
def test_cli_refusals(tmp_path, no_library, tail, msg):
    from mfvi_dip_mia_amd import runner
    err = io.StringIO()
    with pytest.raises(SystemExit) as e, contextlib.redirect_stderr(err):
        runner.main(["--config", "unused.json", "--save-path", str(tmp_path)] + list(tail))
    assert e.value.code == 2 and msg in " ".join(err.getvalue().split()), err.getvalue()
    assert os.listdir(str(tmp_path)) == []


def test_cli_accepts_the_flag(tmp_path, no_library, monkeypatch):
    from mfvi_dip_mia_amd import runner

    class Accepted(Exception):
        pass

    def accepted(*a, **k):
        raise Accepted
    monkeypatch.setattr(runner, "load_config", accepted)
    for tail in (("--kl-type", "forward", "--bayes", "mfvi"), ("--kl-type", "forward"), ("--kl-type", "reverse", "--bayes", "dip"),
                 ("--kl-type", "forward", "--fits-per-launch", "2"), ("--task", "ct", "--kl-type", "forward", "--ct-volume", "phantom:2"),
                 ("--task", "inpainting", "--kl-type", "forward", "--inpaint-fits", "2")):
        with pytest.raises(Accepted):
            runner.main(["--config", "unused.json", "--save-path", str(tmp_path)] + list(tail))
    assert os.listdir(str(tmp_path)) == []
