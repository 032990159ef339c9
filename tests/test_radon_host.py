"""CPU checks of the FastRadonTransform drop-in: the public name and the C ABI rows, the constructor's buffers
against the reference's (tests/golden/radon_dropin.npz, scripts/make_radon_golden.py), every refusal before the library loads, and the
float64 centre-rotation restatement (tests/radon_restatement.py) against the reference module's forward and autograd and against the
oracle."""
import os
import re

import numpy as np
import pytest

import radon_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADON_SYMBOLS = ["mfvi_radon_project", "mfvi_radon_backproject"]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "radon_dropin.npz"))


def _no_gpu():
    raise AssertionError("the library was loaded before the arguments were checked")


# ---- the public name and the ABI ---------------------------------------------------------------------------------------------------
def test_name_is_exported_without_loading_the_library(monkeypatch):
    import mfvi_dip_mia_amd as M
    from mfvi_dip_mia_amd import _lib
    monkeypatch.setattr(_lib, "lib", _no_gpu)
    assert "FastRadonTransform" in M.api.__all__
    from mfvi_dip_mia_amd import FastRadonTransform
    import torch
    assert issubclass(FastRadonTransform, torch.nn.Module)
    assert FastRadonTransform is M.FastRadonTransform                              # one class, built once


def test_abi_declares_and_binds_the_entry_points():
    from mfvi_dip_mia_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mfvi_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mfvi_[a-z0-9_]+)\s*\(", txt))
    assert set(RADON_SYMBOLS) <= declared and set(RADON_SYMBOLS) <= set(_lib.SIGNATURES)
    assert all(len(_lib.SIGNATURES[s][1]) == 7 for s in RADON_SYMBOLS)
    assert {"mfvi_radon_forward", "mfvi_radon_adjoint", "mfvi_radon_mse"} <= declared             # the engine's entry points stay
    assert re.search(r"#define\s+MFVI_ABI_VERSION\s+6\b", txt)
    from mfvi_dip_mia_amd import _build
    assert "radon_planes.hip" in _build.SOURCES and os.path.exists(os.path.join(_build.CSRC, "radon_planes.hip"))


# ---- constructor -------------------------------------------------------------------------------------------------------------------
def test_constructor_buffers_are_the_references(golden, monkeypatch):
    import torch
    from mfvi_dip_mia_amd import _lib, FastRadonTransform
    monkeypatch.setattr(_lib, "lib", _no_gpu)
    case = next(c for c in R.CASES if c[0] == R.CTOR_CASE)
    _, S, C, _ = case
    deg = R.theta_of(case)
    fr = FastRadonTransform((1, C, S, S), torch.from_numpy(deg.copy()))
    for k in ("theta", "ts", "tc", "z", "trans"):
        got = getattr(fr, k).numpy()
        assert got.dtype == np.float32 and got.shape == golden["ctor_" + k].shape, k
        assert np.abs(got - golden["ctor_" + k]).max() <= 2.0 ** -23, k                            # fp32 sin / cos of the same fp32 radians
    assert fr.trans.shape == (deg.size, 2, 3)
    assert np.array_equal(fr.theta_deg.numpy(), deg)
    keys = list(fr.state_dict().keys())
    assert keys == ["theta", "ts", "tc", "z", "trans"]                                             # the degrees are not persistent
    assert "grid" not in dict(fr.named_buffers()) and not hasattr(fr, "grid")                      # the documented difference
    # the default: 180 angles, one per degree
    fr = FastRadonTransform(torch.Size((1, 1, 33, 33)))
    assert fr.theta.shape == (180,) and np.array_equal(fr.theta_deg.numpy(), np.arange(180, dtype=np.float32))
    assert np.abs(fr.theta.numpy() - np.deg2rad(np.arange(180.0))).max() < 3e-7


def test_refusals_come_before_the_library(monkeypatch):
    import torch
    from mfvi_dip_mia_amd import _lib, FastRadonTransform
    monkeypatch.setattr(_lib, "lib", _no_gpu)
    for size in ((1, 1, 32, 24), (1, 1, 24, 32), (32, 32), (1, 1, 0, 0)):
        with pytest.raises(ValueError, match="square"):
            FastRadonTransform(size)
    fr = FastRadonTransform((1, 1, 16, 16), torch.tensor([0.0, 30.0]))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        fr(torch.zeros(1, 1, 16, 16))
    with pytest.raises(NotImplementedError, match="no CPU path"):
        fr(torch.zeros(1, 1, 16, 16, dtype=torch.float64))
    # dtype and size are judged on CUDA tensors, which this test cannot make: a stand-in with a CUDA tensor's attributes walks the
    # same checks (tests/test_gpu_radon_dropin.py repeats them on real tensors)
    class OnCuda:
        is_cuda = True

        def __init__(self, dtype, shape):
            self.dtype, self.shape = dtype, shape

        def dim(self):
            return len(self.shape)
    with pytest.raises(NotImplementedError, match="float32"):
        fr.forward(OnCuda(torch.float64, (1, 1, 16, 16)))
    with pytest.raises(NotImplementedError, match="float32"):
        fr.forward(OnCuda(torch.float16, (1, 1, 16, 16)))
    for shape in ((1, 1, 16, 20), (1, 1, 20, 16), (1, 1, 32, 32), (1, 16, 16)):
        with pytest.raises(ValueError, match="expects"):
            fr.forward(OnCuda(torch.float32, shape))


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c[0])
def test_restatement_matches_the_reference_module(golden, case):
    """relerr < 5e-5: the bound tests/test_oracle_golden.py holds the oracle to against the same module."""
    name, S, C, _ = case
    theta = R.theta_of(case)
    assert np.array_equal(golden[name + "_theta_deg"], theta)
    x, y, gy, gx = (golden[name + k] for k in ("_x", "_y", "_gy", "_gx"))
    assert x.shape == (1, C, S, S) and y.shape == gy.shape == (1, C, theta.size, S) and gx.shape == x.shape
    ef, ea = R.relerr(R.forward64(x, theta), y), R.relerr(R.adjoint64(gy, theta, S), gx)
    print("%s: forward %.2e gradient %.2e" % (name, ef, ea))
    assert ef < 5e-5 and ea < 5e-5


def test_restatement_matches_the_micro_golden(golden_dir):
    from oracle import oracle as O
    g = np.load(os.path.join(golden_dir, "micro.npz"))
    theta = np.arange(0, 180., 4., dtype=np.float32)
    img = O.phantom(64, 64, 11)
    s = R.forward64(img, theta)
    assert R.relerr(s, g["radon64_sino"]) < 5e-5
    rr = O.normal_fill(11, 2, 5, 0, 0, s.size).reshape(s.shape)
    assert R.relerr(R.adjoint64(rr, theta, 64), g["radon64_adj"]) < 5e-5
    lhs, rhs = float((s * rr).sum()), float((R.adjoint64(rr, theta, 64) * img).sum())
    assert abs(lhs - rhs) < 1e-12 * abs(lhs)                                       # one set of float64 weights: a transpose to rounding


def test_restatement_equals_the_oracle():
    """S = 33, T = 180: both are float64 arithmetic on the same float32 (c, s), rounded once."""
    from oracle import oracle as O
    theta = np.arange(180.0, dtype=np.float32)
    img = O.phantom(33, 33, 5)
    sref = O.radon_fwd(img, theta)
    assert R.relerr(R.forward64(img, theta), sref) < 1e-6
    r = O.normal_fill(5, 2, 1, 0, 0, sref.size).reshape(sref.shape)
    assert R.relerr(R.adjoint64(r, theta, 33), O.radon_adj(r, theta, 33, 33)) < 1e-6


def test_golden_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "radon_dropin.npz")) <= 512 * 1024
