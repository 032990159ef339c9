"""CPU checks of the posterior predictive feature: the uncert_regression_gal golden agrees with a numpy restatement of the statistics
(DESIGN.md section 11), and the runner refuses --predict-samples for methods without a posterior before anything touches the GPU."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gal_numpy(x):
    """uncert_regression_gal restated in float64: x [N, C, H, W], the last channel a variance."""
    x = x.astype(np.float64)
    ale = x[:, -1].mean(0)
    epi = x[:, :-1].var(0, ddof=1).mean(0)
    return ale, epi, ale + epi


@pytest.mark.parametrize("tag", ["c2", "c4"])
def test_golden_matches_numpy_restatement(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "predictive_gal.npz"))
    x = g[tag + "_x"]
    N, C, H, W = x.shape
    ale, epi, unc = gal_numpy(x)
    for name, ref in (("ale", ale), ("epi", epi), ("uncert", unc)):
        got = g["%s_%s" % (tag, name)]
        assert got.shape == (1, 1, H, W)
        assert np.abs(got[0, 0] - ref).max() <= 1e-5 * np.abs(ref).max(), name
    for red, f in (("mean", np.mean), ("sum", np.sum)):
        want = np.array([f(ale), f(epi), f(unc)])
        assert np.allclose(g["%s_%s" % (tag, red)], want, rtol=1e-5, atol=0), red


def test_golden_is_small(golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "predictive_gal.npz")) <= 200 * 1024


@pytest.mark.parametrize("bayes", ["dip", "sgld"])
def test_predict_samples_rejected_for_methods_without_posterior(monkeypatch, capsys, bayes):
    from mfvi_dip_mia_amd import _lib, runner

    def no_gpu():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_gpu)
    cfg = os.path.join(ROOT, "configs", "%s_den.json" % bayes)
    with pytest.raises(SystemExit) as e:
        runner.main(["--task", "denoising", "--bayes", bayes, "--config", cfg, "--predict-samples", "8"])
    assert e.value.code == 2
    assert "--predict-samples" in capsys.readouterr().err


def test_predict_samples_rejected_by_the_runner_functions(monkeypatch):
    from mfvi_dip_mia_amd import _lib, runner

    def no_gpu():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_gpu)
    with pytest.raises(ValueError, match="posterior"):
        runner.run_den_dip(imsize=(32, 32), num_iter=1, save=False, predict_samples=4)
    with pytest.raises(ValueError, match="posterior"):
        runner.run_inp_sgld(imsize=(32, 32), num_iter=1, save=False, predict_samples=4)
    with pytest.raises(ValueError, match="at least 2"):
        runner.run_den_mfvi(imsize=(32, 32), num_iter=1, save=False, predict_samples=1)


def test_predictive_modes_and_layout():
    from mfvi_dip_mia_amd import predictive as P
    assert P.image_channels(2, "logprec") == (1, True) and P.image_channels(4, "inp") == (3, True)
    assert P.image_channels(5, "raw") == (4, True) and P.image_channels(1, "mean_only") == (1, False)
    assert [P.default_mode(c) for c in (1, 2, 4)] == ["mean_only", "logprec", "inp"]
    with pytest.raises(ValueError):
        P.default_mode(3)
    with pytest.raises(ValueError):
        P.mode_code("logvar")
    assert P.DEFAULT_STEP == 2 ** 31
