"""Host-side checks of the total-variation term: the float64 restatement against the reference's recorded values
and autograd gradients (tests/golden/tv.npz, scripts/make_golden_tv.py), the two new symbols of the C ABI, and what the engines, the
batches, the drop-in and the CLI refuse before the library is loaded."""
import contextlib
import io
import os
import re

import numpy as np
import pytest

import tv_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"mfvi_tv_term_scratch_bytes": 4, "mfvi_tv_term": 16}


def golden_cases(golden_dir):
    """[(name, x, beta, val32, val64, grad64)] of tests/golden/tv.npz."""
    g = np.load(os.path.join(golden_dir, "tv.npz"))
    out = []
    for name in g["cases"]:
        shape, beta = str(name).split("_b")
        out.append((str(name), g["x_" + shape], float(beta), float(g[name + "_val32"]), float(g[name + "_val64"]), g[name + "_grad64"]))
    return out, g


@pytest.fixture()
def no_library(monkeypatch):
    """Loading the HIP library is an error for the duration of the test."""
    import mfvi_dip_mia_amd as M

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(M._lib, "lib", boom)
    return M


def test_restatement_matches_the_reference(golden_dir):
    cases, g = golden_cases(golden_dir)
    assert len(cases) == 11 and os.path.getsize(os.path.join(golden_dir, "tv.npz")) <= 200 * 1024
    assert {c[1].shape for c in cases} == {(1, 1, 2, 2), (1, 1, 1, 8), (1, 1, 8, 1), (2, 3, 5, 7), (3, 1, 17, 65), (1, 2, 33, 130), (1, 2, 32, 40)}
    assert sorted(c[2] for c in cases if c[1].shape in ((2, 3, 5, 7), (1, 2, 32, 40))) == [0.5, 0.5, 0.75, 0.75, 1.0, 1.0]
    for name, x, beta, _, v64, g64 in cases:
        assert not R.zero_cells_touch(x).any(), name                     # seeded, no ties
        v, gr = R.tv_value(x, beta), R.tv_grad(x, beta)
        if x.shape[2] == 1 or x.shape[3] == 1:
            assert v == 0.0 and v64 == 0.0 and not gr.any() and not g64.any(), name
            continue
        assert abs(v - v64) <= 1e-12 * abs(v64), (name, v, v64)
        assert np.abs(gr - g64).max() <= 1e-12 * np.abs(g64).max(), (name, np.abs(gr - g64).max())
        assert gr[..., -1, -1].any() == False, name                      # noqa: E712  (the corner pixel touches no cell)
        assert np.allclose(R.tv_planes(x, beta).sum(), v, rtol=1e-14)


def test_restatement_on_the_flat_patch(golden_dir):
    """A cell with dh = dw = 0: the reference's gradient is NaN on the three pixels that touch it; the restatement uses g = 0 there."""
    _, g = golden_cases(golden_dir)
    x, nan = g["flat_x"], g["flat_nan"]
    assert x.shape == (1, 1, 5, 7) and nan.sum() == 3
    assert np.array_equal(R.zero_cells_touch(x), nan)
    gr = R.tv_grad(x, 0.5)
    assert np.isfinite(gr).all()
    assert abs(R.tv_value(x, 0.5) - float(g["flat_val64"])) <= 1e-12 * float(g["flat_val64"])      # the value is unaffected
    # outside the mask the rule changes nothing: the same gradient as the unguarded formula (central differences of the fp64 value)
    h = 1e-6
    for idx in ((0, 0, 0, 0), (0, 0, 3, 3), (0, 0, 4, 6), (0, 0, 0, 2)):
        assert not nan[idx]
        xp, xm = x.astype(np.float64), x.astype(np.float64)
        xp[idx] += h; xm[idx] -= h
        assert abs((R.tv_value(xp) - R.tv_value(xm)) / (2 * h) - gr[idx]) < 1e-6


def test_header_and_ctypes_agree_on_the_new_symbols():
    import mfvi_dip_mia_amd as M
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mfvi_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+MFVI_ABI_VERSION\s+6\b", txt)          # additions only
    for name, n_args in NEW_SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(M._lib.SIGNATURES[name][1]), name
    assert "tv.hip" in M._build.SOURCES and os.path.exists(os.path.join(M._build.CSRC, "tv.hip"))
    assert "tv_loss" in M.api.__all__ and M.tv_loss is M.tv.tv_loss


def test_library_exports_the_new_symbols():
    import ctypes
    import mfvi_dip_mia_amd as M
    M.build()
    lib = ctypes.CDLL(M._lib.LIB_PATH)
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    assert M._lib.lib().mfvi_abi_version() == 6


def test_check_tv():
    from mfvi_dip_mia_amd.tv import check_tv
    assert check_tv(0.0, 0.5) == (0.0, 0.5) and check_tv(0.25, 1, "ct") == (0.25, 1.0)
    assert check_tv(0.1, 0.75, "den", n=3) == ([0.1] * 3, 0.75) and check_tv([0, 1, 2], 0.5, "sr", n=3) == ([0.0, 1.0, 2.0], 0.5)
    assert check_tv(0.0, 0.5, "inp") == (0.0, 0.5)                       # off is off for every task
    for w in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tv_weight"):
            check_tv(w, 0.5)
    for b in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tv_beta"):
            check_tv(0.1, b)
    with pytest.raises(ValueError, match="2 values for 3 fits"):
        check_tv([0.1, 0.2], 0.5, n=3)
    with pytest.raises(ValueError, match="inp"):
        check_tv(0.1, 0.5, "inp")


def test_refusals_come_before_the_library(no_library):
    M = no_library
    import torch
    from mfvi_dip_mia_amd.engine import ElboEngine, SiblingEngine
    from mfvi_dip_mia_amd import runner
    for kw in (dict(tv_weight=-1.0), dict(tv_weight=float("nan")), dict(tv_weight=float("inf")), dict(tv_weight=0.1, tv_beta=0.0),
               dict(tv_weight=0.1, tv_beta=-1.0), dict(tv_weight=0.1, task="inp")):
        with pytest.raises(ValueError, match="tv_"):
            ElboEngine(32, 32, **kw)
        with pytest.raises(ValueError, match="tv_"):
            SiblingEngine(32, 32, method="dip", **kw)
    for kw in (dict(tv_weight=-1.0), dict(tv_weight=[0.1, 0.2]), dict(tv_weight=[0.0, 0.1, float("inf")]), dict(tv_weight=0.1, tv_beta=0.0)):
        with pytest.raises(ValueError, match="tv_"):
            M.FitBatch(32, 32, 3, **kw)
        with pytest.raises(ValueError, match="tv_"):
            M.CtVolume(32, 3, **kw)
        with pytest.raises(ValueError, match="tv_"):
            M.SiblingBatch(32, 32, 3, "dip", **kw)
    with pytest.raises(TypeError):
        M.InpaintBatch(32, 32, 2, tv_weight=0.1)                        # the inpainting batch has no such keyword
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(NotImplementedError, match="CUDA float32"):
        M.tv_loss(x)
    with pytest.raises(NotImplementedError, match="CUDA float32"):
        M.tv_loss(x.double(), 1.0)
    # the runners: refused before a run directory exists
    for fn, kw in ((runner.run_den_mfvi, dict(tv_weight=-0.1)), (runner.run_sr_dip, dict(tv_weight=0.1, tv_beta=0.0)),
                   (runner.run_ct_mcd, dict(tv_weight=float("nan"))), (runner.run_inp_mfvi, dict(tv_weight=0.1)),
                   (runner.run_inp_dip, dict(tv_weight=0.1))):
        with pytest.raises(ValueError, match="tv_"):
            fn(save_path="/nonexistent/never/made", **kw)
    with pytest.raises(ValueError, match="tv_"):
        runner.run_inpaint_batch([dict(img=np.zeros((3, 32, 32), np.float32), temp=1e-6, sigma=0.01, tv_weight=0.1)], save=False)


@pytest.mark.parametrize("tail, msg", [
    (("--tv-weight", "-0.1"), "--tv-weight -0.1: finite and >= 0"),
    (("--tv-weight", "nan"), "--tv-weight nan: finite and >= 0"),
    (("--tv-weight", "0.1", "--tv-beta", "0"), "--tv-beta 0.0: finite and > 0"),
    (("--tv-beta", "-1"), "--tv-beta -1.0: finite and > 0"),
    (("--task", "inpainting", "--tv-weight", "0.1"), "does not combine with --task inpainting"),
    (("--task", "inpainting", "--inpaint-fits", "2", "--tv-weight", "0.1"), "does not combine with --task inpainting"),
    # every older refusal is reported first
    (("--tv-weight", "-0.1", "--predict-samples", "1"), "--predict-samples 1: 0 (off) or at least 2"),
    (("--tv-weight", "-0.1", "--fits-per-launch", "2", "--calibration"), "--fits-per-launch does not combine with --calibration"),
])
def test_cli_refusals(tmp_path, no_library, tail, msg):
    from mfvi_dip_mia_amd import runner
    err = io.StringIO()
    with pytest.raises(SystemExit) as e, contextlib.redirect_stderr(err):
        runner.main(["--config", "unused.json", "--save-path", str(tmp_path)] + list(tail))
    assert e.value.code == 2 and msg in " ".join(err.getvalue().split()), err.getvalue()
    assert os.listdir(str(tmp_path)) == []


def test_cli_accepts_the_flags(tmp_path, no_library, monkeypatch):
    from mfvi_dip_mia_amd import runner

    class Accepted(Exception):
        pass

    def accepted(*a, **k):
        raise Accepted
    monkeypatch.setattr(runner, "load_config", accepted)
    for tail in (("--tv-weight", "0.05"), ("--tv-weight", "0.05", "--tv-beta", "1"), ("--task", "ct", "--tv-weight", "1e-3", "--ct-volume", "phantom:2"),
                 ("--task", "inpainting", "--tv-weight", "0"), ("--bayes", "sgld", "--sibling-fits", "2", "--tv-weight", "0.1")):
        with pytest.raises(Accepted):
            runner.main(["--config", "unused.json", "--save-path", str(tmp_path)] + list(tail))
    assert os.listdir(str(tmp_path)) == []
