"""Posterior predictive sampling: the accumulate / finalize kernels against numpy fp64 and across chunkings, the
uncert_regression_gal drop-in against the reference's outputs, ElboEngine.predict against the oracle and against the plan's own forward
outputs, training left undisturbed, the MC-dropout / bf16 / rejection paths, two K-sharded ranks, the runner's predictive.npz and
MeanFieldVI.predictive."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import note_margin as _note

from oracle import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))
STEP = 2 ** 31
KEYS = ("mean", "epi", "ale", "total", "err2", "mse_mc")


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    _v = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
    _note(_v, 'relerr')
    return _v


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return None if t is None else t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    assert torch.cuda.is_available(), "these tests need the GPU"
    M_._lib.lib()
    return M_


def stats_numpy(y, mode, ref=None, clip=False):
    """DESIGN.md section 11 in float64 from the fp32 draws y [N, C, H, W]."""
    y = y.astype(np.float64)
    N = y.shape[0]
    if mode == "raw":
        m, a = y[:, :-1], y[:, -1]
    elif mode == "logprec":
        m, a = y[:, :1], np.exp(-y[:, 1])
    elif mode == "inp":
        m, a = 1.0 / (1.0 + np.exp(-y[:, :3])), np.exp(-y[:, 3])
    else:
        m, a = y[:, :1], None
    if clip:
        m = np.clip(m, 0, 1); a = None if a is None else np.clip(a, 0, 1)
    r = dict(mean=m.mean(0), epi=np.maximum(m.var(0, ddof=1).mean(0), 0))
    r["ale"] = None if a is None else a.mean(0)
    r["total"] = r["epi"] + (0 if a is None else r["ale"])
    if ref is not None:
        r["err2"] = ((r["mean"] - ref) ** 2).mean(0)
        r["mse_mc"] = r["err2"] + (N - 1) / N * r["epi"]
    else:
        r["err2"] = r["mse_mc"] = None
    return r


def check_maps(got, want, tol, what=""):
    for k in KEYS:
        if want.get(k) is None:
            assert got[k] is None, (what, k)
            continue
        g = host(got[k]) if torch.is_tensor(got[k]) else got[k]
        assert g.shape == want[k].shape, (what, k, g.shape, want[k].shape)
        e = relerr(g, want[k])
        assert e < tol.get(k, tol["*"]), (what, k, e)


def synth(N, C, H, W, seed):
    rng = np.random.default_rng(seed)
    y = rng.normal(0.5, 0.4, size=(1, C, H, W)) + rng.normal(scale=0.15, size=(N, C, H, W))      # some values outside [0, 1]: clip acts
    return y.astype(np.float32)


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(35, 45), (24, 32)])          # H*W odd (scalar loads) and a multiple of 4 (16-byte loads)
@pytest.mark.parametrize("mode,C", [("raw", 3), ("logprec", 2), ("inp", 4), ("mean_only", 1)])
@pytest.mark.parametrize("clip", [False, True])
def test_accumulate_finalize_vs_numpy_any_chunking(M, hw, mode, C, clip):
    from mfvi_dip_mia_amd.predictive import Accumulator, image_channels
    H, W = hw
    N = 37
    y = synth(N, C, H, W, seed=C + 10 * clip)
    cimg = image_channels(C, mode)[0]
    ref = np.random.default_rng(5).uniform(0, 1, size=(cimg, H, W)).astype(np.float32)
    yd = dev(y)
    results = []
    for chunk in (1, 5, 16, 37):
        acc = Accumulator(C, H, W, mode)
        for c0 in range(0, N, chunk):
            n = min(chunk, N - c0)
            acc.add(yd[c0:c0 + n], n, clip)
        r = acc.finalize(N, dev(ref))
        results.append({k: host(v) for k, v in r.items()})
    base = results[0]
    for r in results[1:]:                                       # bit-identical for every chunking
        for k in list(KEYS) + ["sums"]:
            assert (base[k] is None and r[k] is None) or np.array_equal(base[k], r[k]), k
    want = stats_numpy(y, mode, ref, clip)
    check_maps(base, want, {"*": 2e-6}, mode)
    if want["ale"] is not None:
        assert relerr(base["sums"][0], want["ale"].astype(np.float32).sum()) < 2e-6
    assert relerr(base["sums"][1], want["epi"].astype(np.float32).sum()) < 2e-6


def test_accumulator_rejects_bad_arguments(M):
    from mfvi_dip_mia_amd.predictive import Accumulator
    with pytest.raises(ValueError):
        Accumulator(3, 8, 8, "logprec")
    acc = Accumulator(2, 8, 8, "logprec")
    acc.add(torch.zeros((1, 2, 8, 8), device="cuda"), 1)
    with pytest.raises(ValueError, match="at least 2"):
        acc.finalize()
    with pytest.raises(ValueError):
        acc.add(torch.zeros((1, 2, 8, 9), device="cuda"), 1)


# ---- 2. drop-in ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["c2", "c4"])
def test_uncert_regression_gal_vs_reference(M, golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "predictive_gal.npz"))
    x = g[tag + "_x"]
    imgs = [dev(x[k:k + 1]) for k in range(x.shape[0])]
    for red in ("mean", "sum"):
        got = M.uncert_regression_gal(imgs, red)
        assert isinstance(got, tuple) and all(isinstance(v, float) for v in got)
        assert relerr(np.array(got), g["%s_%s" % (tag, red)]) < 1e-5, red
    ale, epi, unc = M.uncert_regression_gal(imgs, "none")
    for t, k in ((ale, "ale"), (epi, "epi"), (unc, "uncert")):
        assert t.shape == (1, 1) + x.shape[2:] and not t.requires_grad
        assert relerr(host(t), g["%s_%s" % (tag, k)]) < 1e-5, k
    with pytest.raises(NotImplementedError):
        M.uncert_regression_gal([torch.from_numpy(x[k:k + 1]) for k in range(2)])
    with pytest.raises(NotImplementedError):
        M.uncert_regression_gal([dev(x[k:k + 1, -1:]) for k in range(2)])


# ---- 3. engine vs the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", ["den", "sr", "ct"])
def test_engine_predict_vs_oracle(M, task):
    H = W = 32; N, seed = 6, 4
    n_out = 1 if task == "ct" else 2
    eng = M.engine.ElboEngine(H, W, task=task, K=2, input_depth=8, seed=seed, net_kwargs=SMALL, autotune=False)
    onet = O.make_net(H, W, input_depth=8, n_out=n_out, **SMALL)
    gt = O.phantom(H, W, seed)
    r = eng.predict(N, target=torch.from_numpy(gt))
    assert r["n"] == N and r["step"] == STEP
    mu, rho, bn, z0 = (host(t) for t in (eng.mu, eng.rho, eng.bn, eng.z0))
    outs = []
    for k in range(N):
        o, tape = O.net_forward(onet, mu, rho, bn, z0, seed, STEP, k)
        tape.free(); outs.append(o)
    want = stats_numpy(np.stack(outs), "mean_only" if task == "ct" else "logprec", gt[None])
    # forward parity is 2e-5 per output (tests/test_gpu_parity.py); a variance of draws amplifies it by max|y| / spread
    check_maps(r, want, {"*": 5e-5, "epi": 1e-3, "total": 1e-3, "mse_mc": 1e-3}, task)


# ---- 4. engine vs the same plan's per-chunk outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [16, 8])
def test_engine_predict_vs_plan_outputs(M, chunk):
    H = W = 64; N, seed = 40, 3
    eng = M.engine.ElboEngine(H, W, task="den", K=1, input_depth=8, seed=seed, net_kwargs=dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4)),
                              autotune=False)
    gt = O.phantom(H, W, seed)
    r1 = eng.predict(N, target=dev(gt), chunk=chunk)
    r1 = {k: host(v) if torch.is_tensor(v) else v for k, v in r1.items()}
    plan, _ = eng._pred_plan(chunk)
    outs = []
    for c0 in range(0, N, chunk):
        n = min(chunk, N - c0)
        outs.append(host(plan.forward(eng.mu, eng.rho, eng.bn, eng.z0, seed, STEP, c0, n))[:n])
    want = stats_numpy(np.concatenate(outs), "logprec", gt[None])
    check_maps(r1, want, {"*": 2e-6, "epi": 2e-5, "total": 2e-5, "mse_mc": 2e-5}, chunk)
    r2 = eng.predict(N, target=dev(gt), chunk=chunk)
    for k in KEYS:
        assert relerr(host(r2[k]), r1[k]) < 1e-6, k
    assert not np.array_equal(r1["mean"], host(eng.predict(N, target=dev(gt), chunk=chunk, step=5)["mean"]))     # another step, other draws


# ---- 5. training undisturbed -----------------------------------------------------------------------------------------------------------
def _state(eng):
    torch.cuda.synchronize()
    return np.concatenate([host(eng.params), host(eng.m), host(eng.v), np.array(eng.losses(), np.float32)])


def _distance(a, b):
    return float(np.abs(a.astype(np.float64) - b).max())


@pytest.mark.parametrize("device_step", [False, True])
def test_predict_leaves_training_undisturbed(M, device_step):
    H = W = 32; seed = 6

    def fresh():
        e = M.engine.ElboEngine(H, W, task="den", K=2, input_depth=8, seed=seed, temp=5.7e-7, sigma=1.5e-5, lr=1e-3, net_kwargs=SMALL,
                                autotune=False)
        e.set_target(dev(O.noisy(O.phantom(H, W, seed), 0.1, seed)))
        if device_step:
            e.enable_device_step()
        return e

    def plain(e):
        for _ in range(3):
            e.step()
        return _state(e)

    def interleaved(e):
        e.step(); e.predict(4); e.step(); e.predict(5, chunk=1); e.step()
        return _state(e)

    if device_step:                      # init_params() does not reset the device counter: fresh engines
        a, b, c = plain(fresh()), plain(fresh()), interleaved(fresh())
    else:
        eng = fresh()
        a = plain(eng); eng.init_params(); b = plain(eng); eng.init_params(); c = interleaved(eng)
    assert _distance(c, a) <= _distance(b, a), (_distance(c, a), _distance(b, a))


# ---- 6. MC dropout, bf16, rejections ------------------------------------------------------------------------------------------------------
def test_mcd_predict_vs_oracle(M):
    from mfvi_dip_mia_amd.engine import SiblingEngine
    H = W = 32; seed, N, p = 5, 6, 0.3
    net_kw = dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4))
    eng = SiblingEngine(H, W, method="mcd", task="den", K=1, input_depth=8, seed=seed, dropout_p=p, net_kwargs=net_kw, autotune=False)
    onet = O.make_net(H, W, input_depth=8, n_out=2, drop_down=p, drop_up=p, **net_kw)
    tgt = O.noisy(O.phantom(H, W, seed), 0.1, seed)
    r = eng.predict(N)
    ref = O.sibling_grad(onet, host(eng.mu), host(eng.bn), host(eng.z0), tgt, loss="gnll", seed=seed, step=STEP, K=N, want_out=True)
    want = stats_numpy(ref["out"], "logprec")
    assert want["epi"].max() > 1e-6                                        # the masks differ between draws
    check_maps(r, want, {"*": 5e-5, "epi": 1e-3, "total": 1e-3}, "mcd")


def test_bf16_engine_predict_vs_plan_outputs(M):
    H = W = 128; N, seed, chunk = 12, 2, 8
    eng = M.engine.ElboEngine(H, W, task="den", K=2, input_depth=8, seed=seed, net_kwargs=dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4)),
                              autotune=False, param_dtype="bf16")
    r = eng.predict(N, chunk=chunk)
    plan, _ = eng._pred_plan(chunk)
    outs = [host(plan.forward(eng.mu, eng.rho, eng.bn, eng.z0, seed, STEP, c0, min(chunk, N - c0)))[:min(chunk, N - c0)] for c0 in range(0, N, chunk)]
    check_maps(r, stats_numpy(np.concatenate(outs), "logprec"), {"*": 2e-6, "epi": 2e-5, "total": 2e-5}, "bf16")


def test_predict_rejections(M):
    from mfvi_dip_mia_amd.engine import SiblingEngine
    kw = dict(task="den", K=1, input_depth=8, seed=1, net_kwargs=SMALL, autotune=False)
    with pytest.raises(ValueError, match="no posterior"):
        SiblingEngine(32, 32, method="dip", **kw).predict(4)
    with pytest.raises(NotImplementedError):
        SiblingEngine(32, 32, method="sgld", **kw).predict(4)
    eng = M.engine.ElboEngine(32, 32, **kw)
    with pytest.raises(ValueError, match="at least 2"):
        eng.predict(1)


# ---- 7. two ranks ----------------------------------------------------------------------------------------------------------------------
def test_predict_two_ranks_equal_single_rank(M, tmp_path):
    world, N = 2, 24
    out = str(tmp_path / "pred_ranks.npz")
    port = str(31500 + (os.getpid() % 2000))
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "predict_rank_worker.py"), str(r), str(world), port, out, str(N)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    z = np.load(out)
    assert z["identical"].all()
    from predict_rank_worker import make_engine
    eng, gt = make_engine(0, 1)
    r = eng.predict(N, target=dev(gt), chunk=N // world)          # the ranks' launches: 12 draws each
    for k in KEYS:
        assert relerr(z[k], host(r[k])) < 1e-6, k


# ---- 8. runner ---------------------------------------------------------------------------------------------------------------------------
def test_runner_writes_predictive_npz(M, tmp_path, monkeypatch):
    monkeypatch.setenv("MFVI_TUNE_CACHE", str(tmp_path / "tune.json"))
    # (the runner crops to a multiple of 32: 64 x 64 with the two-scale net is the tiny fit)
    kw = dict(img="phantom", imsize=(64, 64), num_iter=5, lr=1e-3, temp=5.7e-7, sigma=1.5e-5, input_depth=8, seed=1, show_every=2, save=True,
              net_kwargs=SMALL)

    def fit(sub, **extra):
        d = tmp_path / sub
        d.mkdir()
        r = M.runner.run_den_mfvi(save_path=str(d), **kw, **extra)
        return r, np.load(os.path.join(r["run_dir"], "save.npz"), allow_pickle=True)

    ra, a = fit("a")
    rb, b = fit("b")
    rp, p = fit("p", predict_samples=16)
    H, W = rp["recons"].shape[-2:]
    z = np.load(os.path.join(rp["run_dir"], "predictive.npz"))
    assert sorted(z.files) == sorted(["mean", "epi", "ale", "total", "err2", "mse_mc", "n_samples", "step"])
    assert z["mean"].shape == (1, H, W) and all(z[k].shape == (H, W) for k in ("epi", "ale", "total", "err2", "mse_mc"))
    assert int(z["n_samples"]) == 16 and int(z["step"]) == STEP
    assert np.array_equal(rp["predictive"]["mean"], z["mean"])
    assert not os.path.exists(os.path.join(ra["run_dir"], "predictive.npz")) and "predictive" not in ra
    assert sorted(a.files) == sorted(p.files)

    def same(x, y, z, what):
        # the spread of two plain fits; the metric sums are fp64 atomics, so that spread may be a last bit (seen: 1.8e-15 on a PSNR of
        # 12 against 3.6e-15 for the third fit): a floor of 1e-13 relative.  Interference (a reused eps, an overwritten slab) is O(1).
        x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
        if not x.size:
            return
        spread = max(np.abs(x - y).max(), 1e-13 * np.abs(x).max())
        assert np.abs(z - x).max() <= spread, what

    for k in a.files:
        if a[k].dtype != object:
            same(a[k], b[k], p[k], k)
        else:                                                               # the dict-of-'mfvi' object arrays
            va, vb, vp = a[k].item(), b[k].item(), p[k].item()
            assert sorted(va) == sorted(vp)
            for m in va:
                same(va[m], vb[m], vp[m], (k, m))


# ---- 9. MeanFieldVI.predictive -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reparam", ["", "local"])
def test_meanfieldvi_predictive(M, reparam):
    device = torch.device('cuda')
    mk = lambda: M.get_net(8, 'skip', 'reflection', skip_n33d=[8, 16], skip_n33u=[8, 16], skip_n11=4, num_scales=2, n_channels=2, upsample_mode='bilinear')
    torch.manual_seed(0)
    net = M.MeanFieldVI(mk(), prior={'mu': 0.0, 'sigma': 0.05}, device=device, reparam=reparam, seed=3, n_samples=4, autotune=False)
    torch.manual_seed(0)
    twin = M.MeanFieldVI(mk(), prior={'mu': 0.0, 'sigma': 0.05}, device=device, reparam=reparam, seed=3, n_samples=4, autotune=False)
    x = torch.rand(1, 8, 16, 16, device=device) * 0.1
    net(x); twin(x)                                         # one training forward each: _step 1, running statistics updated once
    step0 = net._step
    o_old = net(x)
    twin(x)
    N = 10
    gt = torch.rand(1, 16, 16, device=device)
    r = net.predictive(x, N, target=gt)
    assert net._step == step0 + 1 and r["n"] == N and r["step"] == STEP
    # the module plan's own outputs: launches of n_samples with consecutive k0
    plan = net._plan_for(8, 16, 16, 4)
    mu, rho, bn = net._blocks()
    outs = [host(plan.forward(mu, rho, bn, x[0].contiguous(), net.seed, STEP, k0, min(4, N - k0)))[:min(4, N - k0)] for k0 in range(0, N, 4)]
    check_maps(r, stats_numpy(np.concatenate(outs), "logprec", host(gt)), {"*": 2e-6, "epi": 2e-5, "total": 2e-5, "mse_mc": 2e-5}, reparam)
    with pytest.raises(RuntimeError, match="no longer the latest"):
        o_old.sum().backward()
    # the running statistics moved by the training forwards only, as the twin's did (up to the forward's run-to-run rounding)
    for b, c in zip(net._bn, twin._bn):
        assert relerr(host(b.running_mean), host(c.running_mean)) < 1e-6 and relerr(host(b.running_var), host(c.running_var)) < 1e-6
        assert int(b.num_batches_tracked) == int(c.num_batches_tracked)
    assert relerr(host(net(x)), host(twin(x))) < 1e-6         # the next training forward draws what it would have drawn
    r2 = net.predictive(x, N, target=gt, mode="raw")
    assert r2["mean"].shape == (1, 16, 16)
