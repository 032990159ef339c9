"""Host-side logic of the batched inpainting fits: what InpaintBatch and --inpaint-fits refuse before the library is
loaded, per-fit hyper-parameters, the new symbols of the C ABI, and the scratch mask the runner draws for a job without one."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"mfvi_gaussian_nll_inpainting_fits": 14, "mfvi_ema_inpainting_fits": 9, "mfvi_masked_sq_err_fits": 13}


@pytest.fixture()
def no_library(monkeypatch):
    """Loading the HIP library is an error for the duration of the test."""
    import mfvi_dip_mia_amd as M

    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(M._lib, "lib", boom)
    return M


def test_check_args_refusals_and_hyper_parameters(no_library):
    from mfvi_dip_mia_amd import inpaintbatch as IB
    temps, sigmas, lrs = IB.check_args(256, 320, 2, 1, 1e-6, [0.1, 0.2], 2e-3, "per_fit")
    assert temps == [1e-6, 1e-6] and sigmas == [0.1, 0.2] and lrs == [2e-3, 2e-3]
    assert IB.pyramid(256, 320, 6) == [(128, 160), (64, 80), (32, 40), (16, 20), (8, 10), (4, 5)]      # the reference's deep widths 10 and 5
    small = dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(0, 0, 0))
    assert IB.check_args(24, 40, 3, 2, [1, 2, 3], 0.1, [1e-3] * 3, "shared", small)[0] == [1.0, 2.0, 3.0]
    # an odd map above the deepest level passes where the scale below it has a skip branch: its Concat crops the up-sampled branch to the
    # skip branch (models/common.py:31-41), and the program the constructor would build maps H x W to H x W
    skips = dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4))
    assert IB.pyramid(24, 44, 3) == [(12, 22), (6, 11), (3, 6)]
    IB.check_args(24, 44, 2, 1, 1.0, 0.1, 1e-3, "per_fit", skips)
    from mfvi_dip_mia_amd.program import skip_program
    P, zin, zout, _ = skip_program(24, 44, 8, 4, **dict(IB.inp_net(), **skips))
    assert (P.tensors[zout]["H"], P.tensors[zout]["W"]) == (24, 44)
    with pytest.raises(ValueError, match="only the deepest map may be odd"):
        IB.check_args(24, 44, 2, 1, 1.0, 0.1, 1e-3, "per_fit", dict(skips, ns=(4, 4, 0)))
    for args, msg in (((30, 32, 2, 1, 1.0, 0.1, 1e-3, "per_fit"), "multiples of 4"),
                      ((256, 322, 2, 1, 1.0, 0.1, 1e-3, "per_fit"), "multiples of 4"),
                      ((64, 64, 2, 1, 1.0, 0.1, 1e-3, "per_fit"), "at least 3 on a side"),          # six scales: 64 -> 1
                      ((128, 256, 2, 1, 1.0, 0.1, 1e-3, "per_fit"), "at least 3 on a side"),         # 128 -> 2
                      ((24, 40, 2, 1, 1.0, 0.1, 1e-3, "per_fit", dict(small, nd=(8, 16, 16, 16), nu=(8, 16, 16, 16), ns=(0, 0, 0, 0))), "only the deepest map may be odd"),
                      ((192, 192, 0, 1, 1.0, 0.1, 1e-3, "per_fit"), "at least 1 each"),
                      ((192, 192, 2, 0, 1.0, 0.1, 1e-3, "per_fit"), "at least 1 each"),
                      ((192, 192, 256, 256, 1.0, 0.1, 1e-3, "per_fit"), "n_fits \\* K < 65536"),
                      ((192, 192, 2, 1, [1.0, 2.0, 3.0], 0.1, 1e-3, "per_fit"), "temp: 3 values for 2 fits"),
                      ((192, 192, 2, 1, 1.0, [0.1], 1e-3, "per_fit"), "sigma: 1 values for 2 fits"),
                      ((192, 192, 2, 1, 1.0, 0.1, [1e-3] * 3, "per_fit"), "lr: 3 values for 2 fits"),
                      ((192, 192, 2, 1, 1.0, 0.1, 0.0, "per_fit"), "lr > 0"),
                      ((192, 192, 2, 1, -1.0, 0.1, 1e-3, "per_fit"), ">= 0"),
                      ((192, 192, 2, 1, 1.0, 0.1, 1e-3, "zeros"), "init")):
        with pytest.raises(ValueError, match=msg):
            IB.check_args(*args)


def test_constructor_refusals_come_before_the_library(no_library):
    M = no_library
    assert M.InpaintBatch is M.inpaintbatch.InpaintBatch and "InpaintBatch" in M.api.__all__
    for kw in (dict(temp=[1.0, 2.0, 3.0]), dict(lr=[1e-3]), dict(init="zeros"), dict(K=0), dict(lr=0.0)):
        with pytest.raises(ValueError):
            M.InpaintBatch(192, 192, 2, **kw)
    with pytest.raises(ValueError):
        M.InpaintBatch(190, 192, 2)
    with pytest.raises(ValueError):
        M.InpaintBatch(64, 64, 2)
    with pytest.raises(ValueError):
        M.InpaintBatch(192, 192, 0)
    with pytest.raises(NotImplementedError):                                   # FitBatch keeps its refusal of the task
        M.FitBatch(32, 32, 2, task="inp")


@pytest.mark.parametrize("extra,msg", [
    (["--task", "denoising"], "--inpaint-fits batches mean-field VI inpainting fits (--task inpainting --bayes mfvi), not --task denoising --bayes mfvi"),
    (["--task", "ct"], "--inpaint-fits batches mean-field VI inpainting fits (--task inpainting --bayes mfvi), not --task ct --bayes mfvi"),
    (["--task", "inpainting", "--bayes", "mcd"], "--inpaint-fits batches mean-field VI inpainting fits (--task inpainting --bayes mfvi), not --task inpainting --bayes mcd"),
    (["--task", "inpainting", "--bayes", "dip"], "--inpaint-fits batches mean-field VI inpainting fits (--task inpainting --bayes mfvi), not --task inpainting --bayes dip"),
    (["--task", "inpainting", "--param-dtype", "bf16"], "--inpaint-fits takes float32 parameters (--param-dtype f32)"),
    (["--task", "inpainting", "--fits-per-launch", "4"], "--inpaint-fits does not combine with --fits-per-launch"),
    (["--task", "ct", "--ct-volume", "phantom:4"], "--inpaint-fits does not combine with --ct-volume"),
    (["--task", "inpainting", "--ct-volume", "phantom:4"], "--inpaint-fits does not combine with --ct-volume"),
    (["--task", "inpainting", "--predict-samples", "8"], "--inpaint-fits does not combine with --predict-samples"),
    (["--task", "inpainting", "--calibration"], "--inpaint-fits does not combine with --calibration"),
    (["--task", "inpainting", "--inpaint-fits", "-2"], "--inpaint-fits -2: 0 (off) or the number of fits per launch")])
def test_argparse_refusals_without_the_library(no_library, tmp_path, capsys, extra, msg):
    M = no_library
    cfg = os.path.join(ROOT, "configs", "mfvi_inp.json")
    with pytest.raises(SystemExit) as e:
        M.runner.main(["--config", cfg, "--save-path", str(tmp_path), "--inpaint-fits", "4"] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert msg in " ".join(err.split()), err                                   # (argparse wraps its message: compare with the whitespace folded)
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
    m = re.search(r"#define\s+MFVI_MASKED_SQ_ERR_BLOCKS\s+(\d+)", src)
    assert m and int(m.group(1)) == M._lib.MASKED_SQ_ERR_BLOCKS


def test_scratch_mask_is_what_run_inp_mfvi_drew_inline():
    """The twelve lines run_inp_mfvi held before the helper existed, restated: the same seed must give the same mask."""
    from mfvi_dip_mia_amd import runner
    for H, W, seed in ((32, 32, 42), (24, 40, 7), (64, 96, 1)):
        rng = np.random.default_rng(seed)
        mask = np.ones((1, H, W), np.float32)
        for _ in range(24):
            y, x = rng.integers(0, H), rng.integers(0, W)
            for _ in range(H):
                mask[0, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 0
                y = int(np.clip(y + rng.integers(-1, 2), 0, H - 1)); x = int(np.clip(x + rng.integers(-1, 2), 0, W - 1))
        got = runner.scratch_mask(H, W, seed)
        assert got.dtype == np.float32 and got.shape == (1, H, W) and np.array_equal(got, mask)
        assert 0.0 < 1.0 - got.mean() < 1.0
    assert not np.array_equal(runner.scratch_mask(32, 32, 1), runner.scratch_mask(32, 32, 2))
