"""The CT volume: the per-fit Radon data term against mfvi_radon_mse per fit and a float64 sum over mfvi_radon_project,
CtVolume against the oracle per slice, the independence from the grouping, slice 0 against the standalone CT engine, NaN isolation,
to_engine, set_volume and the runner's --ct-volume.

Net: the SMALL net of test_gpu_runner.py at 32x32, input depth 8, one output channel.  Kernel shapes: S = 1 (the four-load instance), 2 (the
smallest pair), 40 (one strip, partly live), 65 (a second strip with one live lane), with 3 and 45 angles.  As in test_gpu_fitbatch.py every
parity test first writes distinct BatchNorm parameters per slice: at initialisation all slices have gamma = 1, beta = 0."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))
THETA45 = np.arange(0, 180., 4., dtype=np.float32)
THETA3 = np.array([0.0, 33.5, 120.0], np.float32)


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    assert torch.cuda.is_available()
    M_._lib.lib()
    return M_


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def bn_values(prog, seed, f):
    """gamma = 1 + 0.2 u, beta = 0.1 u, u ~ U[0,1) seeded per slice."""
    u = O.uniform_fill(seed, 7, f, 0, prog.n_bn).astype(np.float32)
    bn = np.zeros(prog.n_bn, np.float32)
    for b in prog.bns:
        o, c = b["off"], b["C"]
        bn[o:o + c] = 1.0 + 0.2 * u[o:o + c]
        bn[o + c:o + 2 * c] = 0.1 * u[o + c:o + 2 * c]
    return bn


def write_bn(vol, seed):
    for d in range(vol.D):
        vol.fit(d)["bn"].copy_(dev(bn_values(vol.prog, seed, d)))


def _hyper(D):
    """temp, sigma, lr per slice.  temp from 1e-4 up: at the 1e-6 of the denoising tests temp * KL is 0.4 % of a CT data term (a sum over rays,
    ~18 here) and another slice's hyper-parameters would move the loss by less than the test needs to tell them apart; at 1e-4 it is a third.
    lr from 1e-3 DOWN: the first Adam step moves every parameter by its lr, a gradient at rounding level may take the other sign, and the
    bound on the largest parameter error (2.5e-3 per step) is the one the engine's test uses at lr = 1e-3."""
    return [1e-4 * 2 ** d for d in range(D)], [0.05 * 2 ** d for d in range(D)], [1e-3 / 2 ** d for d in range(D)]


def sinograms(S, D, seed, theta=THETA45):
    """One sinogram per slice, each of its own phantom."""
    return np.stack([O.radon_fwd(O.phantom(S, S, seed + d), theta) for d in range(D)]).astype(np.float32)


def volume(M, D, spl, K, seed, S=32, sinos=None):
    temps, sigmas, lrs = _hyper(D)
    vol = M.CtVolume(S, D, slices_per_launch=spl, K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
    write_bn(vol, seed)
    vol.set_sinograms(torch.from_numpy(sinograms(S, D, seed) if sinos is None else sinos))
    return vol


# ---- 1. kernel level -----------------------------------------------------------------------------------------------------------------------
def mse_fits(M, out, sinos, stride, theta, F, K, S, T, scale, scratch, dout, mse):
    L = M._lib
    return L.lib().mfvi_radon_mse_fits(L.ptr(out), L.ptr(sinos), stride, L.ptr(theta), F, K, S, T, scale, L.ptr(scratch), None if dout is None else L.ptr(dout),
                                       L.ptr(mse), L.stream_ptr())


def kernel_inputs(M, S, T, F, K, seed=17):
    n = F * K
    theta = THETA45 if T == 45 else THETA3
    out = dev((0.3 + 0.5 * O.normal_fill(seed, 2, 0, 0, 0, n * S * S)).reshape(n, 1, S, S).astype(np.float32))
    stride = T * S + 5                                                   # sinograms further apart than they are long
    sinos = np.zeros((F, stride), np.float32)
    sinos[:, :T * S] = (0.3 * S * O.uniform_fill(seed, 1, 0, 0, F * T * S)).reshape(F, T * S)      # distinct per fit, of a ray sum's size
    nbytes = M._lib.lib().mfvi_radon_mse_fits_scratch_bytes(F, K, S, T)
    assert nbytes == n * T * ((S + 63) // 64) * 8 + n * T * S * 4
    return out, dev(sinos), stride, dev(theta), torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("T", [3, 45])
@pytest.mark.parametrize("S", [1, 2, 40, 65])
def test_radon_mse_fits_against_single_fit(M, S, T):
    """F = 3 fits x K = 2 samples, distinct sinograms per fit.  Residual planes and dout against mfvi_radon_mse per fit at 4e-5 (two kernels,
    each within 2e-5 of the oracle: the bound of tests/test_gpu_radon_dropin.py); mse[f] against a float64 sum over mfvi_radon_project's
    output at 2e-6 (the bound of test_gaussian_nll_fits_against_single_fit)."""
    L = M._lib
    lib, sp = L.lib(), L.stream_ptr()
    F, K, scale = 3, 2, 0.5
    n = F * K
    out, sinos, stride, theta, scratch = kernel_inputs(M, S, T, F, K)
    proj = torch.empty((n, T, S), device="cuda")
    L.check(lib.mfvi_radon_project(L.ptr(out), L.ptr(theta), n, S, T, L.ptr(proj), sp))
    proj_before = host(proj).copy()
    dout = torch.full_like(out, 7.0); mse = torch.zeros(F, dtype=torch.float64, device="cuda")
    L.check(mse_fits(M, out, sinos, stride, theta, F, K, S, T, scale, scratch, dout, mse))
    resid = host(scratch[n * T * ((S + 63) // 64) * 8:].view(torch.float32)).reshape(n, T, S)
    sino_h = host(sinos)[:, :T * S].reshape(F, T, S)
    for f in range(F):
        s1 = torch.empty(K * T * S, device="cuda"); d1 = torch.full((K, 1, S, S), 7.0, device="cuda")
        a1 = torch.zeros(1, dtype=torch.float64, device="cuda")
        L.check(lib.mfvi_radon_mse(L.ptr(out[f * K:]), L.ptr(sinos[f]), L.ptr(theta), K, S, S, T, scale, L.ptr(s1), L.ptr(d1), L.ptr(a1), sp))
        er, ed = relerr(resid[f * K:(f + 1) * K], host(s1).reshape(K, T, S)), relerr(host(dout[f * K:(f + 1) * K]), host(d1))
        want = sum(np.mean((proj_before[f * K + k].astype(np.float64) - sino_h[f]) ** 2) for k in range(K))
        em = abs(float(mse[f]) - want) / want
        print("S=%d T=%d fit %d: residual %.2e dout %.2e mse %.2e (%.9g, single-fit entry point %.9g)" % (S, T, f, er, ed, em, float(mse[f]), float(a1[0])))
        assert er < 4e-5 and ed < 4e-5, (f, er, ed)
        assert em < 2e-6, (f, float(mse[f]), want)
    # accumulates (+=), and with dout = NULL writes no gradient
    first, d_first = host(mse).copy(), host(dout).copy()
    L.check(mse_fits(M, out, sinos, stride, theta, F, K, S, T, scale, scratch, None, mse))
    assert np.allclose(host(mse), 2 * first, rtol=1e-12, atol=0) and np.array_equal(host(dout), d_first)
    # the shared row loop did not drift: mfvi_radon_project gives the bits it gave before the epilogue kernel ran
    L.check(lib.mfvi_radon_project(L.ptr(out), L.ptr(theta), n, S, T, L.ptr(proj), sp))
    assert np.array_equal(host(proj), proj_before)


@pytest.mark.parametrize("F", [1, 3])
def test_radon_mse_fits_is_bit_identical_from_call_to_call(M, F):
    K, S, T = 2, 65, 45
    out, sinos, stride, theta, _ = kernel_inputs(M, S, T, F, K, seed=29)
    runs = []
    for _ in range(2):
        scratch = torch.zeros(M._lib.lib().mfvi_radon_mse_fits_scratch_bytes(F, K, S, T), dtype=torch.uint8, device="cuda")
        dout = torch.zeros_like(out); mse = torch.zeros(F, dtype=torch.float64, device="cuda")
        M._lib.check(mse_fits(M, out, sinos, stride, theta, F, K, S, T, 1.0 / K, scratch, dout, mse))
        runs.append([host(x).copy() for x in (dout, mse, scratch)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert np.all(runs[0][1] > 0)


def test_radon_mse_fits_argument_errors(M):
    lib = M._lib.lib()
    F, K, S, T = 2, 2, 8, 3
    out, sinos, stride, theta, scratch = kernel_inputs(M, S, T, F, K)
    dout = torch.full_like(out, 7.0); mse = torch.zeros(F, dtype=torch.float64, device="cuda")
    ok = dict(out=out, sinos=sinos, stride=stride, theta=theta, F=F, K=K, S=S, T=T, scale=1.0, scratch=scratch, dout=dout, mse=mse)

    for change in (dict(out=None), dict(sinos=None), dict(theta=None), dict(scratch=None), dict(mse=None), dict(F=0), dict(K=0), dict(F=32768, K=2),
                   dict(S=0), dict(S=32769), dict(T=0), dict(T=32769), dict(stride=T * S - 1), dict(scratch=scratch[4:])):
        a = dict(ok, **change)
        p = lambda t: None if t is None else M._lib.ptr(t)
        rc = lib.mfvi_radon_mse_fits(p(a["out"]), p(a["sinos"]), a["stride"], p(a["theta"]), a["F"], a["K"], a["S"], a["T"], a["scale"], p(a["scratch"]),
                                     p(a["dout"]), p(a["mse"]), M._lib.stream_ptr())
        assert rc == -1 and b"radon_mse_fits" in lib.mfvi_last_error(), change
    for bad in ((0, 1, 8, 3), (1, 0, 8, 3), (32768, 2, 8, 3), (1, 1, 0, 3), (1, 1, 8, 0), (1, 1, 32769, 3), (1, 1, 8, 32769)):
        assert lib.mfvi_radon_mse_fits_scratch_bytes(*bad) == -1, bad
    torch.cuda.synchronize()
    assert float(mse.abs().sum()) == 0.0 and bool((dout == 7.0).all())       # refused before any launch
    assert lib.mfvi_abi_version() == 6


# ---- 2. against the oracle -------------------------------------------------------------------------------------------------------------------
def test_volume_steps_match_oracle_per_slice(M):
    """Three iterations of D = 3 slices with K = 2, every slice with its own temp, sigma, lr, sinogram, BN parameters: each slice against the
    oracle under the bounds of test_batch_steps_match_oracle_per_fit (loss 2e-4 relative, parameters max 2.5e-3 (it + 1), mean 5e-5 (it + 1),
    re-anchored after every step).  Those two are bounds for lr = 1e-3 (2.5 lr and lr / 20 per step); a slice with a smaller lr is held to
    them scaled by lr / 1e-3, never to more than the figures above."""
    S, D, K, seed = 32, 3, 2, 4
    temps, sigmas, lrs = _hyper(D)
    sino = sinograms(S, D, seed)
    vol = volume(M, D, None, K, seed, sinos=sino)
    onet = O.make_net(S, S, input_depth=8, n_out=1, **SMALL)
    n = vol.n_vi
    p0 = host(vol.params); z0 = host(vol.z0)
    p = p0.copy()
    m = np.zeros_like(p); v = np.zeros_like(p)

    def oracle(d, it, sino_of=None, bn_of=None, k_of=None, hyper_of=None):
        sf, bf, kf, hf = (d if x is None else x for x in (sino_of, bn_of, k_of, hyper_of))
        z = z0[d] + 0.1 * O.normal_fill(seed, 1, 0, d, it, z0[d].size).reshape(z0[d].shape)
        return O.elbo_grad(onet, p[d, :n], p[d, n:2 * n], p[bf, 2 * n:], z, sino[sf], task=2, theta_deg=THETA45, seed=seed, step=it, k0=kf * K, K=K, K_total=K,
                           temp=temps[hf], prior_sigma=vol.prior_sigma[hf])

    # the test's own discriminating power, on the CPU: the oracle given ANOTHER slice's sinogram, gamma / beta, eps indices or hyper-parameters
    # must miss the right answer by more than 100 x the bound it is compared under (loss: 2e-4 relative; a gradient: 2e-4 of its largest value)
    right = oracle(0, 0)
    for kind, wrong in (("sinogram", oracle(0, 0, sino_of=1)), ("bn", oracle(0, 0, bn_of=1)), ("eps", oracle(0, 0, k_of=1)), ("hyper", oracle(0, 0, hyper_of=1))):
        dl = abs(wrong["loss"] - right["loss"]) / abs(right["loss"])
        dg = relerr(wrong["dmu"], right["dmu"])
        print("wrong %s moves the loss by %.2e, dmu by %.2e" % (kind, dl, dg))
        assert max(dl, dg) > 100 * 2e-4, (kind, dl, dg)
    for it in range(3):
        vol.step()
        nll, kl, loss = vol.losses()
        pn = host(vol.params)
        for d in range(D):
            r = oracle(d, it)
            print("slice %d it %d: loss %.6f / %.6f" % (d, it, loss[d], r["loss"]))
            assert abs(loss[d] - r["loss"]) < 2e-4 * max(abs(r["loss"]), 1e-3), (d, it, loss[d], r["loss"])
            O.adam(p[d], np.concatenate([r["dmu"], r["drho"], r["dbn"]]), m[d], v[d], lrs[d], it + 1)
            e = np.abs(pn[d] - p[d])
            print("    params max %.2e mean %.2e" % (e.max(), e.mean()))
            assert lrs[d] <= 1e-3
            assert e.max() < 2.5 * lrs[d] * (it + 1) and e.mean() < 5e-2 * lrs[d] * (it + 1), (d, it, e.max(), e.mean())
        p = pn.copy()                                  # re-anchor: Adam amplifies rounding noise of near-zero gradients
    assert not vol.dead.any()


# ---- 3. the class ----------------------------------------------------------------------------------------------------------------------------
def test_groups_do_not_matter(M):
    """D = 5 slices in groups of 2, 2, 1 and in one group: the same per-slice gradients (2e-4) and data terms (1e-5 relative), the bounds of
    test_fit0_is_the_standalone_engine -- the same arithmetic, only the fp64 BN atomics reorder."""
    D, K, seed = 5, 2, 9
    a, b = volume(M, D, 2, K, seed), volume(M, D, 5, K, seed)
    assert [g[1] for g in a.groups] == [2, 2, 1] and [g[1] for g in b.groups] == [5]
    assert torch.equal(a.params, b.params) and torch.equal(a.z0, b.z0)
    a.grad_only(0); b.grad_only(0)
    ga, gb, na, nb = host(a.grads), host(b.grads), host(a.nll_acc), host(b.nll_acc)
    assert len({float(x) for x in nb}) == D                                 # five different slices
    nv = a.n_vi
    for d in range(D):
        for name, sl in (("dmu", slice(0, nv)), ("drho", slice(nv, 2 * nv)), ("dbn", slice(2 * nv, None))):
            e = relerr(ga[d, sl], gb[d, sl])
            print("slice %d %s %.2e" % (d, name, e))
            assert e < 2e-4 and np.abs(gb[d, sl]).max() > 0, (d, name, e)
        assert abs(na[d] - nb[d]) < 1e-5 * abs(nb[d]), (d, na[d], nb[d])


def test_slice0_is_the_standalone_ct_engine(M):
    S, K, seed = 32, 2, 9
    temps, sigmas, lrs = _hyper(3)
    vol = volume(M, 3, None, K, seed)                                        # one group: vol.z[0] is slice 0's perturbed input afterwards
    eng = M.engine.ElboEngine(S, S, task="ct", K=K, input_depth=8, temp=temps[0], sigma=sigmas[0], lr=lrs[0], seed=seed, net_kwargs=SMALL, autotune=False)
    assert torch.equal(vol.z0[0], eng.z0) and vol.prior_sigma[0] == eng.prior_sigma and torch.equal(vol.theta, eng.theta)
    nv = vol.n_vi
    assert torch.equal(vol.fit(0)["params"][:2 * nv], eng.params[:2 * nv])   # bit-equal initial mu, rho (BN was rewritten per slice above)
    eng.bn.copy_(vol.fit(0)["bn"]); eng.set_target(vol.sinos[0].clone())
    vol.grad_only(0); eng.grad_only(0, with_kl=False)
    assert torch.equal(vol.z[0], eng.z)
    g, ge = host(vol.fit(0)["grads"]), host(eng.grads[:eng.n_params])
    for name, sl in (("dmu", slice(0, nv)), ("drho", slice(nv, 2 * nv)), ("dbn", slice(2 * nv, None))):
        e = relerr(g[sl], ge[sl])
        print("%s %.2e" % (name, e))
        assert e < 2e-4, (name, e)
    a, b = float(vol.nll_acc[0]), float(eng.acc[0])
    assert abs(a - b) < 1e-5 * abs(b), (a, b)


def test_nan_slice_is_isolated(M):
    D, K, seed = 3, 2, 12
    sino = sinograms(32, D, seed)
    bad = sino.copy(); bad[1, 5, 7] = np.nan
    clean, vol = volume(M, D, 2, K, seed, sinos=sino), volume(M, D, 2, K, seed, sinos=bad)      # slices 0 and 1 share a launch set
    clean.grad_only(0); vol.grad_only(0)
    for d in (0, 2):
        assert relerr(host(vol.fit(d)["grads"]), host(clean.fit(d)["grads"])) < 2e-4, d
    before = [host(x).copy() for x in (vol.params, vol.m, vol.v)]
    vol.step(); vol.step()
    assert list(vol.dead) == [0, 1, 0]
    after = [host(x) for x in (vol.params, vol.m, vol.v)]
    for a, b in zip(before, after):
        assert np.array_equal(a[1], b[1])                                  # the dead slice: parameters and moments bit-equal to before
        for d in (0, 2):
            assert np.isfinite(b[d]).all()
    for d in (0, 2):
        assert not np.array_equal(before[0][d], after[0][d])
    assert np.isnan(vol.losses()[0][1]) and np.isfinite(vol.losses()[2][[0, 2]]).all()


def test_to_engine_exports_any_slice(M):
    S, D, K, seed = 32, 3, 1, 21
    temps, sigmas, lrs = _hyper(D)
    vol = volume(M, D, 2, K, seed)
    for _ in range(3):
        vol.step()
    snap = [host(x).copy() for x in (vol.params, vol.m, vol.v, vol.ema)]
    eng = vol.to_engine(2)
    assert eng.task == "ct" and np.array_equal(host(eng.params), snap[0][2]) and np.array_equal(host(eng.m), snap[1][2]) and np.array_equal(host(eng.v), snap[2][2])
    assert eng.t == vol.t == 3 and int(eng.t_applied[0]) == 3 and torch.equal(eng.z0, vol.z0[2])
    assert torch.equal(eng.theta, vol.theta) and torch.equal(eng.target, vol.sinos[2])
    assert (eng.temp, eng.lr, eng.prior_sigma) == (temps[2], lrs[2], vol.prior_sigma[2])
    eng.step()                                                              # the exported slice runs on alone
    assert np.isfinite(eng.losses()[2]) and not np.array_equal(host(eng.params), snap[0][2])
    for a, b in zip(snap, (vol.params, vol.m, vol.v, vol.ema)):
        assert np.array_equal(a, host(b))                                  # the volume is untouched
    gt = np.stack([O.phantom(S, S, seed + d) for d in range(D)])
    ps = vol.psnr(gt)
    assert ps.shape == (D,) and np.isfinite(ps).all()
    assert abs(ps[1] - O.psnr(gt[1], np.clip(snap[3][1, 0], 0, 1))) < 1e-3
    assert tuple(vol.recon().shape) == (D, S, S)
    with pytest.raises(ValueError):
        vol.to_engine(3)


def test_set_volume_is_the_plane_projection(M):
    L = M._lib
    S, D = 32, 3
    vol = M.CtVolume(S, D, slices_per_launch=2, input_depth=8, theta_deg=THETA3.tolist(), net_kwargs=SMALL, autotune=False)
    gt = np.stack([O.phantom(S, S, 5 + d) for d in range(D)])
    vol.set_volume(gt)
    want = torch.empty((D, 3, S), device="cuda")
    L.check(L.lib().mfvi_radon_project(L.ptr(dev(gt)), L.ptr(dev(THETA3)), D, S, 3, L.ptr(want), L.stream_ptr()))
    assert torch.equal(vol.sinos, want)
    assert max(relerr(host(vol.sinos[d]), O.radon_fwd(gt[d], THETA3)) for d in range(D)) < 2e-5      # and it is the oracle's operator
    with pytest.raises(ValueError):
        vol.set_volume(gt[:2])
    with pytest.raises(ValueError):
        vol.set_sinograms(np.zeros((D, 4, S), np.float32))


# ---- 4. runner -------------------------------------------------------------------------------------------------------------------------------
def test_runner_ct_volume(M, tmp_path, capsys):
    cfg = dict(bo_params=dict(temp=dict(candidates=[1e-6]), sigma=dict(candidates=[0.05, 0.1])),
               run_params=dict(num_iter=20, lr=1e-3, seed=1, input_depth=8, show_every=5, plot=False, save=True, net_kwargs=SMALL, autotune=False,
                               save_path=str(tmp_path / "logs")))
    path = str(tmp_path / "cfg.json")
    json.dump(cfg, open(path, "w"))
    res = M.runner.main(["--task", "ct", "--config", path, "--imsize", "32", "--ct-volume", "phantom:3", "--slices-per-launch", "2"])
    assert [(j["temp"], j["sigma"]) for _, j, _ in res] == [(1e-6, 0.05), (1e-6, 0.1)] and all(np.isfinite(y) for _, _, y in res)
    assert "mean PSNR" in capsys.readouterr().out
    dirs = sorted(os.listdir(str(tmp_path / "logs")))
    assert len(dirs) == 2
    for d in dirs:
        z = np.load(os.path.join(str(tmp_path / "logs"), d, "volume.npz"))
        assert set(z.files) == {"theta", "sinograms", "temp", "sigma", "lr", "prior_sigma", "K", "seed", "num_iter", "slices_per_launch", "iterations",
                                "psnr_gt_sm", "nll", "kl", "recon", "dead"}
        assert list(z["iterations"]) == [0, 5, 10, 15, 20] and int(z["slices_per_launch"]) == 2
        assert z["theta"].shape == (45,) and z["sinograms"].shape == (3, 45, 32) and len(z["temp"]) == 3
        assert z["psnr_gt_sm"].shape == z["nll"].shape == z["kl"].shape == (5, 3) and z["recon"].shape == (3, 32, 32) and not z["dead"].any()
        for k in ("psnr_gt_sm", "nll", "kl", "recon", "sinograms"):
            assert np.isfinite(z[k]).all(), k
        assert z["recon"].min() >= 0.0 and z["recon"].max() <= 1.0
