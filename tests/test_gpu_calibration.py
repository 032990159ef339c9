"""Uncertainty calibration on the GPU: the mfvi_uce_* kernels against a float64 numpy restatement of uceloss, the
uceloss drop-in against the reference's outputs (tests/golden/uce.npz), ElboEngine.predict(calibration=...) against the restatement on the
maps it returns, and the runner's calibration.npz.

Tolerances.  Against the restatement with the SAME boundaries the bin of every element is decided by the same float32 comparisons, so counts
are equal as integers, the fp64 sums agree to summation order (1e-12 relative) and an fp32 output is the restated value rounded once (1 ulp).
Against the reference golden the rule is tests/uce_restatement.py tolerance(): max(4 x the reference's own deviation from float64 recorded
in the golden, 4 fp32 ulp), per-bin means relative to the largest mean, uce relative to sum_k prop_k max(unc_k, err_k)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import note_margin as _note
import uce_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))
PRED_KEYS = {"mean", "epi", "ale", "total", "err2", "mse_mc", "n", "step"}
NPZ_KEYS = ("bounds", "count", "prop_in_bin", "err_in_bin", "uncert_in_bin", "uce", "uce_1e-4", "U")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    assert torch.cuda.is_available(), "these tests need the GPU"
    M_._lib.lib()
    return M_


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "uce.npz"))


def rel(a, b, scale, kind):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (kind, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), kind
    k = ~np.isnan(b)
    v = float(np.abs(a[k] - b[k]).max() / scale) if k.any() else 0.0
    _note(v, kind)
    return v


def ulps(got, want64, kind):
    """The largest distance of the fp32 array `got` from float32(want64), in units of the fp32 spacing at want64 (NaN must match NaN)."""
    got = np.asarray(got); want64 = np.asarray(want64, np.float64)
    assert got.dtype == np.float32 and got.shape == want64.shape, (kind, got.dtype, got.shape, want64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), kind
    k = ~np.isnan(want64)
    if not k.any():
        return 0.0
    w32 = want64[k].astype(np.float32)
    d = np.abs(got[k].astype(np.float64) - w32.astype(np.float64)) / np.spacing(np.maximum(np.abs(w32), np.float32(1e-30))).astype(np.float64)
    v = float(d.max())
    _note(v * R.FP32_ULP, kind + " (ulp as relative)")
    return v


def uce_from_fp32(c, outlier):
    """The kernel's formula on ITS fp32 per-bin outputs, in float64 and bin order."""
    prop, e, u = (host(c[k]).astype(np.float64) for k in ("prop", "err_in_bin", "unc_in_bin"))
    s = 0.0
    for k in range(prop.size):
        if prop[k] > outlier:
            s += abs(u[k] - e[k]) * prop[k]
    return s


def check_against_restatement(c, r, what):
    """Calibration dict `c` (device tensors) against restate() with the same boundaries."""
    assert c["count"].dtype == torch.int64 and np.array_equal(host(c["count"]), r["count"]), what
    assert int(c["n"]) == r["n"], what
    for k, want in (("sum_err", r["sum_err"]), ("sum_unc", r["sum_unc"])):
        assert c[k].dtype == torch.float64
        assert rel(host(c[k]), want, max(np.abs(want).max(), 1e-300), "fp64 " + k) <= 1e-12, (what, k)
    pop = r["count"] > 0
    mean_e, mean_u = host(c["sum_err"]) / np.where(pop, r["count"], 1), host(c["sum_unc"]) / np.where(pop, r["count"], 1)
    assert rel(mean_e[pop], r["mean_err"][pop], np.abs(r["mean_err"][pop]).max(), "fp64 mean err") <= 1e-12, what
    assert rel(mean_u[pop], r["mean_unc"][pop], np.abs(r["mean_unc"][pop]).max(), "fp64 mean unc") <= 1e-12, what
    assert np.array_equal(host(c["prop"]), r["prop32"]), what                      # count / n rounded once: exact
    assert ulps(host(c["err_in_bin"]), r["mean_err"], "err_in_bin") <= 1, what
    assert ulps(host(c["unc_in_bin"]), r["mean_unc"], "unc_in_bin") <= 1, what
    assert ulps(host(c["unc_mean"]).reshape(1), np.array([r["unc_mean"]]), "unc_mean") <= 1, what
    for o in (0.0, 1e-4):
        u = c.uce(o)
        assert u.shape == (1,) and u.dtype == torch.float32 and u.is_cuda
        assert np.array_equal(host(c.kept(o)), R.kept(r, o)), (what, o)
        assert ulps(host(u), np.array([uce_from_fp32(c, o)]), "uce") <= 1, (what, o)
        assert rel(host(u), [R.uce(r, o)], R.uce_scale(r), "uce vs fp64") <= 4 * R.FP32_ULP, (what, o)


# ---- 1. kernels vs float64 numpy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_kernels_vs_numpy_on_golden_inputs(M, golden, tag):
    from mfvi_dip_mia_amd.calibration import calibration
    err, unc, bounds = golden[tag + "_err"], golden[tag + "_unc"], golden[tag + "_bounds"]
    assert (unc.size % 4 == 0) == (tag == "a")                                     # a: 16-byte loads; b, c: the scalar tail
    r = R.restate(err, unc, bounds)
    assert np.array_equal(r["count"], golden[tag + "_count"])
    c1 = calibration(dev(err), dev(unc), n_bins=int(golden["n_bins"]), bounds=bounds)
    check_against_restatement(c1, r, tag)
    assert np.array_equal(host(c1["bounds"]), bounds)
    c2 = calibration(dev(err), dev(unc), n_bins=int(golden["n_bins"]), bounds=bounds)
    for k in ("count", "sum_err", "sum_unc", "prop", "err_in_bin", "unc_in_bin", "unc_mean"):
        assert host(c1[k]).tobytes() == host(c2[k]).tobytes(), (tag, k)             # bitwise, NaN included
    assert host(c1.uce(1e-4)).tobytes() == host(c2.uce(1e-4)).tobytes()


@pytest.mark.parametrize("n,n_bins", [(1 << 20, 15), (300001, 200), (4 * 256 * 256 + 2, 256), (5, 1), (64, 64)])
def test_kernels_many_blocks_and_bins(M, n, n_bins):
    """More than one iteration per block (n > 256 blocks x 1024), bins owned by every lane slot (n_bins up to the limit of 256), an
    unaligned view (the scalar path on n % 4 == 0), and the elements that belong to no bin: NaN, below / on the lowest boundary, above
    the highest."""
    from mfvi_dip_mia_amd.calibration import calibration, minmax
    rng = np.random.default_rng(n + n_bins)
    unc = np.exp(rng.normal(-5.0, 0.6, size=n)).astype(np.float32)
    err = (unc * rng.chisquare(1, size=n)).astype(np.float32)
    if n > 100:
        unc[[3, n // 2, n - 1]] = np.nan
        unc[7] = np.inf; unc[11] = -1.0
    lo, hi = minmax(dev(unc))
    fin = unc[np.isfinite(unc)]
    assert lo == float(fin.min()) and hi == float(np.nanmax(unc))                   # exact; NaN ignored
    lo, hi = float(np.quantile(fin, 0.01)), float(np.quantile(fin, 0.995))         # elements on both sides of the range
    bounds = torch.linspace(lo, hi, n_bins + 1).numpy()
    if n > 100:
        unc[13] = bounds[0]; unc[17] = bounds[-1]; unc[19] = bounds[n_bins // 2]     # on the lowest boundary: no bin; on an upper one: that bin
    r = R.restate(err, unc, bounds)
    assert n <= 100 or r["count"].sum() < np.isfinite(unc).sum()
    good = np.isfinite(unc)
    r["unc_mean"] = np.nan if not good.all() else r["unc_mean"]                     # a NaN element makes the mean NaN, as uncerts.mean() does
    c = calibration(dev(err), dev(unc), n_bins=n_bins, bounds=bounds)
    check_against_restatement(c, r, (n, n_bins))
    if n % 4 == 0:                                                                  # the same data at a 4-byte offset: scalar loads
        buf_e, buf_u = torch.empty(n + 1, device="cuda"), torch.empty(n + 1, device="cuda")
        buf_e[1:] = dev(err); buf_u[1:] = dev(unc)
        c2 = calibration(buf_e[1:], buf_u[1:], n_bins=n_bins, bounds=bounds)
        assert np.array_equal(host(c2["count"]), r["count"])
        assert host(c2["sum_err"]).tobytes() == host(c["sum_err"]).tobytes()        # same grouping of elements, same order: same bits


def test_ring_inputs_kernel(M):
    from mfvi_dip_mia_amd.calibration import ring_inputs
    rng = np.random.default_rng(5)
    S, C, H, W = 7, 3, 19, 23
    rec = rng.uniform(0, 1, size=(S, C, H, W)).astype(np.float32); gt = rng.uniform(0, 1, size=(C, H, W)).astype(np.float32)
    epi = rng.uniform(0, 1e-3, size=(C, H, W)).astype(np.float32); ale = rng.uniform(0, 1e-2, size=(1, H, W)).astype(np.float32)
    for mask in (None, (rng.uniform(size=(1, H, W)) > 0.2).astype(np.float32), (rng.uniform(size=(C, H, W)) > 0.2).astype(np.float32)):
        e, u = ring_inputs(rec, gt, epi, ale, mask)
        want = ((rec.astype(np.float64) - gt) ** 2).mean(axis=0) * (1.0 if mask is None else mask)
        assert e.shape == (C, H, W) and u.shape == (C, H, W)
        assert ulps(host(e), want, "errvar") <= 1
        assert np.array_equal(host(u), epi + ale)                                   # one fp32 addition
    e, u = ring_inputs(rec[:, :1], gt[:1], epi[:1], None, None)                      # CT: no aleatoric map
    assert np.array_equal(host(u), epi[:1])


# ---- 2. the drop-in vs the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_uceloss_vs_reference(M, golden, tag):
    from mfvi_dip_mia_amd.calibration import calibration
    err, unc = golden[tag + "_err"], golden[tag + "_unc"]
    rng_ = None if np.isnan(golden[tag + "_range"]).all() else tuple(float(v) for v in golden[tag + "_range"])
    n_bins = int(golden["n_bins"])
    r = R.restate(err, unc, golden[tag + "_bounds"])
    tol = R.tolerance(golden[tag + "_ref_dev"])
    # the boundaries: min / max kernel + host linspace == what the reference computed on the CPU, bit for bit
    assert np.array_equal(host(calibration(dev(err), dev(unc), n_bins=n_bins, range=rng_)["bounds"]), golden[tag + "_bounds"])
    for j, o in enumerate(golden["outliers"]):
        uce, e_b, u_b, prop = M.uceloss(dev(err), dev(unc), n_bins=n_bins, outlier=float(o), range=rng_)
        want = {k: golden["%s_%s_o%d" % (tag, k, j)] for k in ("uce", "err", "unc", "prop")}
        assert all(t.is_cuda and t.dtype == torch.float32 for t in (uce, e_b, u_b, prop))
        assert uce.shape == (1,) and prop.shape == (n_bins,)
        assert e_b.shape == want["err"].shape and u_b.shape == want["unc"].shape     # the kept bins only
        assert np.array_equal(host(prop), want["prop"])
        assert rel(host(e_b), want["err"], R.mean_scale(r), "err_in_bin vs reference") <= tol
        assert rel(host(u_b), want["unc"], R.mean_scale(r), "avg_uncert_in_bin vs reference") <= tol
        assert rel(host(uce), want["uce"], R.uce_scale(r), "uce vs reference") <= tol


def test_uceloss_rejections(M):
    from mfvi_dip_mia_amd import _lib as L
    from mfvi_dip_mia_amd.calibration import calibration
    x = torch.rand(3, 8, 8)
    with pytest.raises(NotImplementedError):
        M.uceloss(x, x)
    with pytest.raises(NotImplementedError):
        M.uceloss(x.cuda(), x)
    with pytest.raises(ValueError, match="elements"):
        M.uceloss(x.cuda(), x.cuda()[:2])
    with pytest.raises(ValueError, match="n_bins"):
        M.uceloss(x.cuda(), x.cuda(), n_bins=257)
    with pytest.raises(ValueError, match="decrease"):
        calibration(x.cuda(), x.cuda(), n_bins=2, bounds=[0.0, 0.5, 0.25])
    # the C entry points bound n_bins themselves
    lib = L.lib()
    assert lib.mfvi_uce_scratch_bytes(100, 257) < 0 and b"n_bins" in lib.mfvi_last_error()
    assert lib.mfvi_uce_scratch_bytes(100, 0) < 0
    d = x.cuda().view(-1)
    assert lib.mfvi_uce_bins(L.ptr(d), L.ptr(d), d.numel(), L.ptr(d), 257, L.ptr(d), L.ptr(d), L.ptr(d), L.ptr(d), L.ptr(d), L.ptr(d), L.ptr(d),
                             L.stream_ptr()) < 0
    assert lib.mfvi_uce_value(L.ptr(d), L.ptr(d), L.ptr(d), 257, ctypes.c_double(0.0), L.ptr(d), L.stream_ptr()) < 0
    # a flat map has no populated bin: every element equals the lowest boundary
    c = calibration(torch.ones(64, device="cuda"), torch.full((64,), 0.5, device="cuda"))
    assert int(c["count"].sum()) == 0 and float(c.uce(0.0)) == 0.0 and bool(torch.isnan(c["err_in_bin"]).all())


# ---- 3. the engines -------------------------------------------------------------------------------------------------------------------------
def _small_fit(M, method="mfvi"):
    from oracle import oracle as O
    H = W = 32; seed = 3
    kw = dict(task="den", K=2, input_depth=8, seed=seed, lr=1e-3, net_kwargs=SMALL, autotune=False)
    if method == "mfvi":
        eng = M.engine.ElboEngine(H, W, temp=5.7e-7, sigma=1.5e-5, **kw)
    else:
        eng = M.engine.SiblingEngine(H, W, method=method, dropout_p=0.3, **kw)
    gt = O.phantom(H, W, seed)
    eng.set_target(dev(O.noisy(gt, 0.1, seed)))
    for _ in range(5):
        eng.step()
    return eng, gt


def _check_predict_calibration(r, n_bins, rng_, what):
    c = r["calibration"]
    total, mse = host(r["total"]), host(r["mse_mc"])
    lo, hi = (float(total.min()), float(total.max())) if rng_ is None else rng_
    bounds = torch.linspace(lo, hi, n_bins + 1).numpy()
    assert np.array_equal(host(c["bounds"]), bounds), what
    rs = R.restate(mse, total, bounds)
    assert rs["count"].sum() > 0.9 * total.size or rng_ is not None
    check_against_restatement(c, rs, what)


@pytest.mark.parametrize("method", ["mfvi", "mcd"])
def test_engine_predict_calibration(M, method):
    eng, gt = _small_fit(M, method)
    N = 12
    plain = eng.predict(N, target=dev(gt))
    assert set(plain) == PRED_KEYS                                                  # without the argument: the result dict as it was
    assert set(eng.predict(N, target=dev(gt), calibration=None)) == PRED_KEYS
    r = eng.predict(N, target=dev(gt), calibration=True)
    assert set(r) == PRED_KEYS | {"calibration"}
    for k in ("mean", "total", "mse_mc"):
        assert np.array_equal(host(r[k]), host(plain[k])), k                        # the maps themselves are untouched
    _check_predict_calibration(r, 15, None, method)
    hi = float(np.quantile(host(plain["total"]), 0.9))
    r = eng.predict(N, target=dev(gt), calibration=dict(n_bins=40, range=(0.0, hi)))
    assert r["calibration"]["prop"].shape == (40,)
    _check_predict_calibration(r, 40, (0.0, hi), method + " range")
    with pytest.raises(ValueError, match="target"):
        eng.predict(N, calibration=True)
    with pytest.raises(ValueError, match="n_bins"):
        eng.predict(N, target=dev(gt), calibration=dict(bins=3))


# ---- 4. the runner --------------------------------------------------------------------------------------------------------------------------
def _ring_restatement(res, gt, n_bins, mask=None):
    S = min(25, res["recons"].shape[0])
    rec = res["recons"][-S:]                                                        # float64 arrays of fp32 values
    errvar = ((rec - gt) ** 2).mean(axis=0) * (1.0 if mask is None else mask)
    unc = res["uncerts"][-1].astype(np.float32) + res["uncerts_ale"][-1].astype(np.float32)
    bounds = torch.linspace(float(unc.min()), float(unc.max()), n_bins + 1).numpy()
    return R.restate(errvar.astype(np.float32), unc, bounds), bounds, unc


def _check_ring(z, res, gt, n_bins):
    r, bounds, unc = _ring_restatement(res, gt, n_bins)
    assert int(z["n_bins"]) == n_bins
    for k in NPZ_KEYS:
        want = {"bounds": (n_bins + 1,), "uce": (1,), "uce_1e-4": (1,), "U": ()}.get(k, (n_bins,))
        assert z["ring_" + k].shape == want, (k, z["ring_" + k].shape)
    assert np.array_equal(z["ring_bounds"], bounds)
    assert np.array_equal(z["ring_count"], r["count"]) and z["ring_count"].dtype == np.int64
    assert r["count"].sum() == unc.size - int((unc == unc.min()).sum())             # the minimum pixel(s) in no bin
    assert np.array_equal(z["ring_prop_in_bin"], r["prop32"])
    assert ulps(z["ring_uncert_in_bin"], r["mean_unc"], "ring unc_in_bin") <= 1
    # errvar is rounded to fp32 once from an fp64 sum whose order differs from numpy's: an element may round the other way (1 ulp),
    # and the per-bin mean is rounded once more
    assert rel(z["ring_err_in_bin"], r["mean_err"], R.mean_scale(r), "ring err_in_bin") <= 2 * R.FP32_ULP
    for key, o in (("ring_uce", 0.0), ("ring_uce_1e-4", 1e-4)):
        assert rel(z[key], [R.uce(r, o)], R.uce_scale(r), key) <= 4 * R.FP32_ULP
    # U = sqrt(unc_mean): the fp32 mean (1 ulp) through an fp32 square root (1 ulp)
    assert ulps(z["ring_U"].reshape(1), np.array([np.sqrt(np.float32(r["unc_mean"]))], np.float64), "ring U") <= 2


def test_runner_writes_calibration_npz(M, tmp_path, monkeypatch):
    monkeypatch.setenv("MFVI_TUNE_CACHE", str(tmp_path / "tune.json"))
    kw = dict(img="phantom", imsize=(64, 64), num_iter=8, lr=1e-3, temp=5.7e-7, sigma=1.5e-5, input_depth=8, seed=1, show_every=2, save=True,
              net_kwargs=SMALL)

    def fit(sub, fn=M.runner.run_den_mfvi, **extra):
        d = tmp_path / sub
        d.mkdir()
        r = fn(save_path=str(d), **dict(kw, **extra))
        return r, np.load(os.path.join(r["run_dir"], "save.npz"), allow_pickle=True)

    ra, a = fit("a")
    assert sorted(os.listdir(ra["run_dir"])) == ["locals.txt", "save.npz"] and "calibration" not in ra
    assert set(a.files) == {"img_gt", "img_noisy", "mse_noisy", "mse_gt", "recons", "uncerts", "uncerts_ale", "psnrs", "ssims"}
    rc, c = fit("c", calibration=True)
    assert sorted(os.listdir(rc["run_dir"])) == ["calibration.npz", "locals.txt", "save.npz"] and set(c.files) == set(a.files)
    names = lambda res: [ln.split(" = ")[0] for ln in open(os.path.join(res["run_dir"], "locals.txt")).read().splitlines()]
    assert names(rc) == names(ra)                                                   # locals.txt: the same entries
    z = np.load(os.path.join(rc["run_dir"], "calibration.npz"))
    assert sorted(z.files) == sorted(["ring_" + k for k in NPZ_KEYS] + ["n_bins"])
    gt = a["img_gt"].astype(np.float64)                                             # (1, H, W)
    _check_ring(z, rc, gt, 15)
    for k in z.files:
        assert np.array_equal(z[k], rc["calibration"][k], equal_nan=True), k
    # with posterior predictive sampling: the pred_ block; predictive.npz keeps its keys
    rp, p = fit("p", calibration=True, calibration_bins=10, predict_samples=16)
    assert sorted(os.listdir(rp["run_dir"])) == ["calibration.npz", "locals.txt", "predictive.npz", "save.npz"]
    zp = np.load(os.path.join(rp["run_dir"], "predictive.npz"))
    assert sorted(zp.files) == sorted(["mean", "epi", "ale", "total", "err2", "mse_mc", "n_samples", "step"])
    assert set(rp["predictive"]) == set(zp.files)
    z = np.load(os.path.join(rp["run_dir"], "calibration.npz"))
    assert sorted(z.files) == sorted([s + k for s in ("ring_", "pred_") for k in NPZ_KEYS] + ["n_bins"])
    _check_ring(z, rp, gt, 10)
    bounds = torch.linspace(float(zp["total"].min()), float(zp["total"].max()), 11).numpy()
    r = R.restate(zp["mse_mc"], zp["total"], bounds)
    assert np.array_equal(z["pred_bounds"], bounds) and np.array_equal(z["pred_count"], r["count"])
    assert np.array_equal(z["pred_prop_in_bin"], r["prop32"])
    assert ulps(z["pred_err_in_bin"], r["mean_err"], "pred err_in_bin") <= 1 and ulps(z["pred_uncert_in_bin"], r["mean_unc"], "pred unc_in_bin") <= 1
    assert rel(z["pred_uce"], [R.uce(r, 0.0)], R.uce_scale(r), "pred_uce") <= 4 * R.FP32_ULP
    assert rel(z["pred_uce_1e-4"], [R.uce(r, 1e-4)], R.uce_scale(r), "pred_uce_1e-4") <= 4 * R.FP32_ULP


def test_runner_calibration_ct_and_sgld(M, tmp_path, monkeypatch):
    monkeypatch.setenv("MFVI_TUNE_CACHE", str(tmp_path / "tune.json"))
    r = M.runner.run_ct_mfvi(img="phantom", imsize=(32, 32), num_iter=6, lr=1e-3, temp=2.2e-10, sigma=1.7e-7, input_depth=8, seed=1, show_every=2,
                             save=True, save_path=str(tmp_path), K=1, net_kwargs=SMALL, calibration=True)
    s = np.load(os.path.join(r["run_dir"], "save.npz"), allow_pickle=True)
    assert set(s.files) == {"img_gt", "img_radon", "mse_noisy", "mse_gt", "recons", "uncerts", "uncerts_ale", "psnrs", "ssims"}
    z = np.load(os.path.join(r["run_dir"], "calibration.npz"))
    assert sorted(z.files) == sorted(["ring_" + k for k in NPZ_KEYS] + ["n_bins"])
    _check_ring(z, r, s["img_gt"][0].astype(np.float64), 15)                         # (1, 1, H, W) -> (1, H, W)
    r = M.runner.run_den_sgld(img="phantom", imsize=(64, 64), num_iter=4, lr=1e-3, input_depth=8, seed=1, show_every=2, save=False,
                              net_kwargs=SMALL, calibration=True)
    assert r["run_dir"] is None and r["calibration"]["ring_count"].shape == (15,)
    _check_ring(r["calibration"], r, M.runner.phantom(64, 64, 1)[None].astype(np.float64), 15)
