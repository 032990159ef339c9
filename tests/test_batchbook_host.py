"""Host-side logic of the batched bookkeeping: the new symbols of the C ABI, the public name, what the command line,
InpaintBatch.track and the BatchBook constructor refuse before the library is loaded."""
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ARGS = {"mfvi_bookkeep_fits": 15, "mfvi_pair_metrics_scratch_bytes": 3, "mfvi_pair_metrics": 12}


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
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n in N_ARGS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert m, name
        assert len(m.group(1).split(",")) == n, name                              # the header's argument count ...
        assert name in M._lib.SIGNATURES and len(M._lib.SIGNATURES[name][1]) == n, name      # ... is the ctypes table's
    assert re.search(r"#define\s+MFVI_ABI_VERSION\s+6\b", src)                    # additions only
    from mfvi_dip_mia_amd import _build
    assert "metrics_fits.hip" in _build.SOURCES
    assert os.path.exists(os.path.join(_build.CSRC, "metrics_fits.hip"))


def test_batchbook_is_public():
    import mfvi_dip_mia_amd as M
    from mfvi_dip_mia_amd import api
    assert "BatchBook" in api.__all__
    assert M.BatchBook is api.BatchBook
    for cls in (M.FitBatch, M.SiblingBatch, M.CtVolume):
        assert callable(cls.track) and callable(cls.metrics) and cls._book is None


@pytest.mark.parametrize("extra", [[], ["--inpaint-fits", "2", "--task", "inpainting"], ["--predict-samples", "4"], ["--bayes", "dip"]])
def test_batch_bookkeeping_needs_a_batch_flag(no_library, tmp_path, capsys, extra):
    M = no_library
    cfg = os.path.join(ROOT, "configs", "mfvi_den.json")
    with pytest.raises(SystemExit) as e:
        M.runner.main(["--config", cfg, "--save-path", str(tmp_path), "--batch-bookkeeping"] + extra)
    assert e.value.code == 2
    assert "--batch-bookkeeping" in capsys.readouterr().err
    assert os.listdir(str(tmp_path)) == []


def test_inpaint_batch_is_not_tracked(no_library):
    M = no_library
    ib = object.__new__(M.InpaintBatch)                # the class alone: no GPU state
    with pytest.raises(NotImplementedError):
        ib.track(np.zeros((3, 32, 32), np.float32), 10)
    with pytest.raises(NotImplementedError):
        M.BatchBook(ib, 10, np.zeros((32, 32), np.float32))


def test_wrong_shapes_are_refused_before_the_library(no_library):
    M = no_library
    H, W, F = 32, 40, 3
    den = types.SimpleNamespace(task="den", n_rows=F, C=2, F=F, H=H, W=W, sr_factor=4)
    sr = types.SimpleNamespace(task="sr", n_rows=F, C=2, F=F, H=H, W=W, sr_factor=4)
    ct = types.SimpleNamespace(task="ct", n_rows=F, C=1, H=H, W=H, groups=[(0, 2, 0, 0, 2)], D=F, S=H)
    ok, okF = np.zeros((H, W), np.float32), np.zeros((F, H, W), np.float32)
    for gt in (np.zeros((W, H)), np.zeros((F + 1, H, W)), np.zeros((F, H, W, 1)), np.zeros((H,))):
        with pytest.raises(ValueError, match="ground truth"):
            M.BatchBook(den, 5, gt, noisy=okF)
    for noisy in (np.zeros((W, H)), np.zeros((F - 1, H, W)), np.zeros((F, H // 4, W // 4))):
        with pytest.raises(ValueError, match="noisy"):
            M.BatchBook(den, 5, ok, noisy=noisy)
    with pytest.raises(ValueError, match="noisy"):
        M.BatchBook(den, 5, okF)                        # denoising needs its noisy reference
    with pytest.raises(ValueError, match="noisy"):
        M.BatchBook(sr, 5, okF, noisy=okF)              # the sr reference is gt[..., ::f, ::f]
    with pytest.raises(ValueError, match="ground truth"):
        M.BatchBook(ct, 5, np.zeros((F, H, W)))         # slices are S x S
    with pytest.raises(ValueError):
        M.BatchBook(den, 0, ok, noisy=ok)
    for b in (den, sr, ct):
        assert getattr(b, "_book", None) is None        # a refused book is not attached
    from mfvi_dip_mia_amd.batchbook import check_maps
    g, n = check_maps("den", F, H, W, ok, okF)
    assert g.shape == n.shape == (F, H, W) and g.dtype == n.dtype == np.float32 and g.flags.c_contiguous
