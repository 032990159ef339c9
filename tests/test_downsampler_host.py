"""CPU checks of the anti-aliasing downsampler: lanczos_taps against the reference's 2-D kernels, the float64
A-matrix restatement of the operator (kept here; tests/test_gpu_downsampler.py imports it) against the reference module's forward and
autograd (tests/golden/downsampler.npz, scripts/make_downsampler_golden.py), the C ABI rows, and every refusal before the library loads."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (kind, factor, H, W): the cases of the golden file.  8 x 12 and 8 x 8: every output pixel clamps on both sides (P = 6 / 10 exceed half
# the map); 32 x 20: non-square with P = 10; 16 x 24 f8: T = 32; 72 x 136: several tiles in both directions (forward and adjoint)
CASES = [("lanczos2", 4, 8, 12), ("lanczos3", 4, 8, 8), ("lanczos3", 4, 32, 20), ("lanczos2", 8, 16, 24), ("lanczos3", 2, 72, 136),
         ("lanczos2", 4, 72, 136)]
N, C = 3, 2
DS_SYMBOLS = ["mfvi_downsample", "mfvi_downsample_adjoint", "mfvi_gaussian_nll_filtered"]


def tag(case):
    return "%s_f%d_%dx%d" % case


# ---- the float64 restatement ------------------------------------------------------------------------------------------------------
def taps64(kind, f):
    a = {"lanczos2": 2, "lanczos3": 3}[kind]
    T = 2 * a * f
    d = np.abs(np.arange(T) + 0.5 - T / 2.0) / f
    L = a * np.sin(np.pi * d) * np.sin(np.pi * d / a) / (np.pi ** 2 * d ** 2)
    return L / L.sum()


def a_matrix(k1, f, n):
    """A [n/f x n]: A[y][clamp(y f + i - P, 0, n - 1)] += k1[i], P = (T - f) / 2 (replication pad + stride-f correlation)."""
    T = len(k1)
    P = (T - f) // 2
    A = np.zeros((n // f, n))
    for y in range(n // f):
        for i in range(T):
            A[y, min(max(y * f + i - P, 0), n - 1)] += k1[i]
    return A


def forward64(x, kind, f):
    k1 = taps64(kind, f)
    H, W = x.shape[-2:]
    return np.einsum("yh,...hw,xw->...yx", a_matrix(k1, f, H), np.asarray(x, np.float64), a_matrix(k1, f, W))


def adjoint64(g, kind, f, H, W):
    k1 = taps64(kind, f)
    return np.einsum("yh,...yx,xw->...hw", a_matrix(k1, f, H), np.asarray(g, np.float64), a_matrix(k1, f, W))


def nll64(out, target, kind, f, grad_scale=1.0):
    """sum_i gaussian_nll(D(out_i)[0], D(out_i)[1], target) (s clamped to +-20, mean over the low-resolution pixels) and
    grad_scale * d nll_i / d out_i, for out [n][2][H][W]."""
    H, W = out.shape[-2:]
    lr = forward64(out, kind, f)
    m, sraw = lr[:, 0], lr[:, 1]
    s = np.clip(sraw, -20.0, 20.0)
    e, df, npix = np.exp(s), np.asarray(target, np.float64)[None] - m, m[0].size
    total = float((e * df * df - s).sum() / npix)
    glr = np.stack([-2.0 * e * df, np.where(np.abs(sraw) <= 20.0, e * df * df - 1.0, 0.0)], axis=1) * (grad_scale / npix)
    return total, adjoint64(glr, kind, f, H, W)


def tolerance(kind, f, scale):
    """4 T 2^-24 (sum |k1|)^2 max|input|: twice the worst-case rounding of a two-pass fp32 separable sum of T taps."""
    k1 = taps64(kind, f)
    return 4.0 * len(k1) * 2.0 ** -24 * np.abs(k1).sum() ** 2 * float(scale)


@pytest.fixture(scope="module")
def golden(golden_dir):
    import mfvi_dip_mia_amd.downsampler      # noqa: F401  (the fixtures belong to the feature)
    return np.load(os.path.join(golden_dir, "downsampler.npz"))


def golden_case(g, case):
    t = tag(case)
    return dict(kernel=g[t + "_kernel"], x=g[t + "_x_u8"].astype(np.float32) / np.float32(255.0), y=g[t + "_y"], gy=g[t + "_gy"], gx=g[t + "_gx"])


# ---- taps and geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=tag)
def test_taps_match_the_reference_kernel(golden, case):
    from mfvi_dip_mia_amd.downsampler import lanczos_taps, pad_width
    kind, f, H, W = case
    k1 = lanczos_taps(kind, f)
    a = int(kind[-1])
    assert k1.dtype == np.float64 and k1.shape == (2 * a * f,)
    assert np.abs(np.outer(k1, k1) - golden[tag(case) + "_kernel"]).max() <= 1e-12
    assert abs(k1.sum() - 1.0) <= 4e-16 and np.abs(k1 - taps64(kind, f)).max() <= 1e-15
    assert lanczos_taps(kind, f, np.float32).dtype == np.float32
    P = pad_width(kind, f)
    assert P == (len(k1) - f) // 2 and 2 * P == len(k1) - f
    assert (H + 2 * P - len(k1)) // f + 1 == H // f and (W + 2 * P - len(k1)) // f + 1 == W // f       # the convolution's output size
    assert golden[tag(case) + "_y"].shape == (N, C, H // f, W // f)


@pytest.mark.parametrize("case", CASES, ids=tag)
def test_restatement_matches_the_reference_module(golden, case):
    kind, f, H, W = case
    c = golden_case(golden, case)
    assert c["x"].shape == (N, C, H, W) and c["x"].min() >= 0.0 and c["x"].max() <= 1.0
    assert np.abs(forward64(c["x"], kind, f) - c["y"]).max() <= 1e-6
    assert np.abs(adjoint64(c["gy"], kind, f, H, W) - c["gx"]).max() <= 1e-6
    A = a_matrix(taps64(kind, f), f, H)
    assert np.abs(A.sum(axis=1) - 1.0).max() <= 1e-14                       # every low-resolution pixel is a weighted mean
    if min(H, W) <= 12:
        assert (np.count_nonzero(A[:, 0]) == H // f) and (np.count_nonzero(A[:, -1]) == H // f)      # every row clamps on both sides


def test_golden_is_small_and_the_gpu_tolerance_is_tight(golden, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "downsampler.npz")) <= 1024 * 1024
    tols = [tolerance(k, f, 1.0) for k, f, _, _ in CASES]
    assert 4e-6 <= min(tols) and max(tols) <= 1.2e-5


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_entry_points():
    from mfvi_dip_mia_amd import _lib
    txt = open(os.path.join(ROOT, "include", "mfvi_hip.h")).read()
    assert "models/downsampler.py:6-136" in txt
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mfvi_[a-z0-9_]+)\s*\(", txt))
    assert set(DS_SYMBOLS) <= declared and set(DS_SYMBOLS) <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["mfvi_downsample"][1]) == 10 and len(_lib.SIGNATURES["mfvi_gaussian_nll_filtered"][1]) == 13
    assert re.search(r"#define\s+MFVI_ABI_VERSION\s+6\b", txt)


# ---- refusals, all before the library is loaded --------------------------------------------------------------------------------------
def _no_gpu():
    raise AssertionError("the library was loaded before the arguments were checked")


def test_taps_refuse_what_the_operator_is_not_defined_for():
    from mfvi_dip_mia_amd.downsampler import lanczos_taps, check_geometry
    for f in (1, 3, 5, 6, 16):
        with pytest.raises(ValueError, match="factor"):
            lanczos_taps("lanczos2", f)
    with pytest.raises(ValueError, match="lanczos"):
        lanczos_taps("bicubic", 4)
    with pytest.raises(ValueError, match="divide"):
        check_geometry("lanczos2", 4, 30, 32)
    with pytest.raises(ValueError, match="divide"):
        check_geometry("lanczos3", 8, 32, 36)


def test_module_refusals(monkeypatch):
    import torch
    from mfvi_dip_mia_amd import _lib, Downsampler
    monkeypatch.setattr(_lib, "lib", _no_gpu)
    for kind in ("gauss12", "gauss1sq2", "gauss", "box"):
        with pytest.raises(NotImplementedError, match=kind):
            Downsampler(1, 4, kind)
    with pytest.raises(NotImplementedError, match="phase"):
        Downsampler(1, 4, "lanczos2", phase=0)
    with pytest.raises(NotImplementedError, match="preserve_size"):
        Downsampler(1, 4, "lanczos2", phase=0.5, preserve_size=False)
    for f in (1, 3):
        with pytest.raises(ValueError, match="factor"):
            Downsampler(1, f, "lanczos2")
    d = Downsampler(2, 4, "lanczos3", 0.5, None, None, None, True)            # the reference's positional order
    assert d.kernel.shape == (24, 24) and abs(d.kernel.sum() - 1.0) < 1e-14
    with pytest.raises(NotImplementedError, match="CPU"):
        d(torch.zeros(1, 2, 8, 8))


def test_engine_and_runner_refusals(monkeypatch):
    from mfvi_dip_mia_amd import _lib, runner
    from mfvi_dip_mia_amd.engine import ElboEngine, SiblingEngine
    monkeypatch.setattr(_lib, "lib", _no_gpu)
    with pytest.raises(ValueError, match="downsampler"):
        ElboEngine(32, 32, task="sr", downsampler="bicubic")
    with pytest.raises(ValueError, match="downsampler"):
        ElboEngine(32, 32, task="den", downsampler="lanczos2")
    with pytest.raises(ValueError, match="factor"):
        ElboEngine(32, 32, task="sr", sr_factor=3, downsampler="lanczos2")
    with pytest.raises(ValueError, match="divide"):
        ElboEngine(32, 36, task="sr", sr_factor=8, downsampler="lanczos3")
    with pytest.raises(ValueError, match="downsampler"):
        SiblingEngine(32, 32, method="dip", task="sr", downsampler="lanczos2")
    with pytest.raises(ValueError, match="downsampler"):
        runner.run_sr_mfvi(imsize=(32, 32), num_iter=1, save=False, downsampler="box")
    with pytest.raises(ValueError, match="downsampler"):
        runner.run_sr_dip(imsize=(32, 32), num_iter=1, save=False, downsampler="lanczos2")
    with pytest.raises(ValueError, match="downsampler"):
        runner.run_den_mfvi(imsize=(32, 32), num_iter=1, save=False, downsampler="lanczos2")


def test_command_line_refusals(monkeypatch, capsys):
    from mfvi_dip_mia_amd import _lib, runner
    monkeypatch.setattr(_lib, "lib", _no_gpu)
    sr, den = os.path.join(ROOT, "configs", "mfvi_sr.json"), os.path.join(ROOT, "configs", "mfvi_den.json")
    with pytest.raises(SystemExit) as e:
        runner.main(["--task", "denoising", "--bayes", "mfvi", "--config", den, "--sr-downsampler", "lanczos2"])
    assert e.value.code == 2 and "belongs to --task super-resolution" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        runner.main(["--task", "super-resolution", "--bayes", "mfvi", "--config", sr, "--sr-downsampler", "lanczos2", "--fits-per-launch", "4"])
    assert e.value.code == 2 and "does not combine with --fits-per-launch" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        runner.main(["--task", "super-resolution", "--bayes", "mfvi", "--config", sr, "--sr-downsampler", "bicubic"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err
