"""GPU tests of the anti-aliasing downsampler: mfvi_downsample / mfvi_downsample_adjoint and the Downsampler module
against the float64 restatement (tests/test_downsampler_host.py) and the reference's outputs (tests/golden/downsampler.npz), the fused
mfvi_gaussian_nll_filtered against the restatement and against Downsampler -> gaussian_nll under autograd, ElboEngine(task="sr",
downsampler=...) and run_sr_mfvi(downsampler=...).  Every case is a few launches on maps of at most 72 x 136."""
import os

import numpy as np
import pytest

import test_downsampler_host as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))          # the two-scale net of tests/test_gpu_runner.py
NLL_CASES = [R.CASES[0], R.CASES[2], R.CASES[4], R.CASES[5]]       # 8 x 12, 32 x 20, 72 x 136 (f 2 and f 4)


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    assert torch.cuda.is_available(), "these tests need the GPU"
    M_._lib.lib()
    return M_


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "downsampler.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _taps(M, kind, f):
    from mfvi_dip_mia_amd.downsampler import c_taps
    return c_taps(kind, f)


# ---- forward and adjoint ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.tag)
def test_forward_and_adjoint(M, golden, case):
    """tol = 4 T 2^-24 (sum |k1|)^2 max|input| (twice the worst-case rounding of a two-pass fp32 separable sum; 5e-6 ... 1.1e-5 per unit
    input) for the forward against the restatement and the reference's output, the same with max|gradient| for the adjoint; the dot
    test within tol_fwd sum|g| + tol_adj sum|x|; the adjoint bit-identical across two calls."""
    kind, f, H, W = case
    L, lib = M._lib, M._lib.lib()
    c = R.golden_case(golden, case)
    x, gy = c["x"], c["gy"]
    tol_f, tol_a = R.tolerance(kind, f, np.abs(x).max()), R.tolerance(kind, f, np.abs(gy).max())
    taps, T = _taps(M, kind, f)
    d_x, d_g = dev(x), dev(gy)
    y = torch.full((R.N, R.C, H // f, W // f), 7.0, device="cuda"); gx = torch.full((R.N, R.C, H, W), 7.0, device="cuda"); gx2 = torch.full_like(gx, -7.0)
    L.check(lib.mfvi_downsample(L.ptr(d_x), R.N, R.C, H, W, f, taps, T, L.ptr(y), L.stream_ptr()))
    L.check(lib.mfvi_downsample_adjoint(L.ptr(d_g), R.N, R.C, H, W, f, taps, T, L.ptr(gx), L.stream_ptr()))
    L.check(lib.mfvi_downsample_adjoint(L.ptr(d_g), R.N, R.C, H, W, f, taps, T, L.ptr(gx2), L.stream_ptr()))
    y_h, gx_h = host(y), host(gx)
    e = dict(fwd64=np.abs(y_h - R.forward64(x, kind, f)).max(), fwd_ref=np.abs(y_h - c["y"]).max(),
             adj64=np.abs(gx_h - R.adjoint64(gy, kind, f, H, W)).max(), adj_ref=np.abs(gx_h - c["gx"]).max())
    dot = abs(float((y_h.astype(np.float64) * gy).sum()) - float((x.astype(np.float64) * gx_h).sum()))
    print("%s: tol_fwd %.2e tol_adj %.2e errors %s dot %.2e (bound %.2e)" % (R.tag(case), tol_f, tol_a, {k: "%.2e" % v for k, v in e.items()}, dot,
                                                                             tol_f * np.abs(gy).sum() + tol_a * np.abs(x).sum()))
    assert e["fwd64"] <= tol_f and e["fwd_ref"] <= tol_f
    assert e["adj64"] <= tol_a and e["adj_ref"] <= tol_a
    assert dot <= tol_f * np.abs(gy).sum() + tol_a * np.abs(x).sum()
    assert torch.equal(gx, gx2)
    # the drop-in module: the same kernels under autograd, with the reference's call shape
    mod = M.Downsampler(R.C, f, kind, phase=0.5, preserve_size=True)
    assert np.abs(mod.kernel - c["kernel"]).max() <= 1e-12
    xt = d_x.clone().requires_grad_(True)
    ym = mod(xt)
    (ym * d_g).sum().backward()
    assert torch.equal(ym.detach(), y) and torch.equal(xt.grad, gx)


def test_entry_points_refuse_bad_arguments(M):
    L, lib = M._lib, M._lib.lib()
    taps, T = _taps(M, "lanczos2", 4)
    x = torch.zeros((1, 1, 8, 12), device="cuda"); y = torch.zeros((1, 1, 2, 3), device="cuda")
    for H, W, f, nt in ((8, 12, 3, T), (8, 12, 1, T), (8, 10, 4, T), (8, 12, 4, 49), (8, 12, 4, 15), (8, 12, 4, 2)):
        assert lib.mfvi_downsample(L.ptr(x), 1, 1, H, W, f, taps, nt, L.ptr(y), L.stream_ptr()) == -1
        assert lib.mfvi_downsample_adjoint(L.ptr(y), 1, 1, H, W, f, taps, nt, L.ptr(x), L.stream_ptr()) == -1
        assert b"downsample" in lib.mfvi_last_error()
    with pytest.raises(ValueError, match="divide"):
        M.Downsampler(1, 4, "lanczos2")(torch.zeros((1, 1, 8, 10), device="cuda"))
    with pytest.raises(ValueError, match="n_planes"):
        M.Downsampler(2, 4, "lanczos2")(x)


# ---- the fused data term ---------------------------------------------------------------------------------------------------------------
def nll_inputs(case, golden):
    """out [3][2][H][W]: channel 0 the golden image input, channel 1 a seeded N(0, 1) log-precision; sample 1 carries a block of -25 and
    sample 2 a block of +25 in channel 1 (both clamp arms; on the 8 x 12 map the blocks are the whole plane); the target is the projected
    ground truth of sample 0 plus noise."""
    kind, f, H, W = case
    rng = np.random.default_rng(77 + H)
    out = np.empty((R.N, 2, H, W), np.float32)
    out[:, 0] = R.golden_case(golden, case)["x"][:, 0]
    out[:, 1] = rng.standard_normal((R.N, H, W)).astype(np.float32)
    bh, bw = (H, W) if H <= 8 else (H // 2, W // 2)
    out[1, 1, :bh, :bw] = -25.0
    out[2, 1, H - bh:, W - bw:] = 25.0
    target = (R.forward64(out[0, 0], kind, f) + 0.05 * rng.standard_normal((H // f, W // f))).astype(np.float32)
    return out, target


@pytest.mark.parametrize("case", NLL_CASES, ids=R.tag)
def test_fused_nll(M, golden, case):
    """nll_sum and dout against the float64 restatement under the bounds of the nearest-SR check of mfvi_gaussian_nll
    (tests/test_gpu_parity.py: 1e-5 of the value, 1e-5 of the largest gradient; here per sample, which is stricter: the +25 sample's
    gradients are e^20 times the others'); nll_sum accumulates and dout is optional; dout is bit-identical across two calls and equals
    Downsampler -> gaussian_nll under autograd."""
    kind, f, H, W = case
    L, lib = M._lib, M._lib.lib()
    out, target = nll_inputs(case, golden)
    gs = 0.5
    taps, T = _taps(M, kind, f)
    d_o, d_t = dev(out), dev(target)
    scratch = torch.empty(R.N * 2 * (H // f) * (W // f), device="cuda")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    dout = torch.full_like(d_o, 7.0); dout2 = torch.full_like(d_o, -7.0)
    call = lambda o, n, d, a: L.check(lib.mfvi_gaussian_nll_filtered(L.ptr(o), L.ptr(d_t), n, H, W, f, taps, T, gs, L.ptr(scratch), L.ptr(d) if d is not None
                                                                     else None, L.ptr(a), L.stream_ptr()))
    call(d_o, R.N, dout, acc)
    total = float(acc)
    acc1 = torch.zeros(1, dtype=torch.float64, device="cuda")
    call(d_o, 1, None, acc1)                   # the first sample alone (the +25 sample dominates the total), no gradient
    first = float(acc1)
    call(d_o, 1, None, acc1)                   # nll_sum accumulates
    assert abs(float(acc1) - 2 * first) <= 1e-12 * abs(first)
    acc2 = torch.zeros(1, dtype=torch.float64, device="cuda")
    call(d_o, R.N, dout2, acc2)
    ref_total, ref_d = R.nll64(out, target, kind, f, gs)
    ref_first, _ = R.nll64(out[:1], target, kind, f, gs)
    errs = [relerr(host(dout)[k], ref_d[k]) for k in range(R.N)]
    print("%s: nll %.9g (ref %.9g, rel %.2e), first sample rel %.2e, dout rel per sample %s" %
          (R.tag(case), total, ref_total, abs(total - ref_total) / abs(ref_total), abs(first - ref_first) / abs(ref_first), ["%.2e" % v for v in errs]))
    assert abs(total - ref_total) < 1e-5 * abs(ref_total)
    assert abs(first - ref_first) < 1e-5 * abs(ref_first)
    assert max(errs) < 1e-5
    assert torch.equal(dout, dout2)
    # the composition of the two drop-ins, sample by sample (gaussian_nll acts on one image)
    mod = M.Downsampler(2, f, kind)
    xt = d_o.clone().requires_grad_(True)
    loss = 0.0
    for k in range(R.N):
        lr = mod(xt[k:k + 1])
        loss = loss + M.gaussian_nll(lr[:, :1], lr[:, 1:], d_t[None, None])
    (gs * loss).backward()
    assert abs(float(loss.detach()) - total) < 1e-5 * abs(total)
    assert max(relerr(host(xt.grad)[k], host(dout)[k]) for k in range(R.N)) < 1e-5


# ---- engine ----------------------------------------------------------------------------------------------------------------------------
def _sr_engine(M, **kw):
    return M.engine.ElboEngine(32, 32, task="sr", K=2, input_depth=8, temp=4.381719802264805e-07, sigma=4.9e-08, lr=1e-3, seed=4, sr_factor=4,
                               net_kwargs=SMALL, **kw)


def test_engine_lanczos_data_term(M):
    from oracle import oracle as O
    eng = _sr_engine(M, downsampler="lanczos2")
    gt = O.phantom(32, 32, 4)
    target = R.forward64(gt, "lanczos2", 4).astype(np.float32)
    eng.set_target(torch.from_numpy(target))
    eng.grad_only(0, with_kl=False)
    out, dout = host(eng.out), host(eng.dout)
    ref_total, ref_d = R.nll64(out, target, "lanczos2", 4, 1.0 / eng.K)
    assert abs(float(eng.acc[0]) - ref_total) < 1e-5 * abs(ref_total)
    assert max(relerr(dout[k], ref_d[k]) for k in range(eng.K)) < 1e-5
    assert np.count_nonzero(dout) == dout.size                                  # dense: every high-resolution pixel receives a data gradient
    # the parameter gradients are the plan's backward pass of exactly that dout (fixed summation order: bit-equal)
    dmu, drho, dbn = torch.zeros_like(eng.dmu), torch.zeros_like(eng.drho), torch.zeros_like(eng.dbn)
    eng.plan.backward(eng.mu, eng.rho, eng.bn, eng.z, eng.seed, 0, 0, eng.K, eng.dout, dmu, drho, dbn, True)
    assert torch.equal(dmu, eng.dmu) and torch.equal(drho, eng.drho) and torch.equal(dbn, eng.dbn)
    assert float(dmu.abs().max()) > 0
    # the fit descends on D(gt)
    eng.step(); first = eng.losses()[0]
    for _ in range(29):
        eng.step()
    last = eng.losses()[0]
    print("lanczos2 SR fit: nll %.5f -> %.5f over 30 steps" % (first, last))
    assert np.isfinite(last) and last < first


def test_engine_nearest_is_the_default_path(M):
    from oracle import oracle as O
    target = torch.from_numpy(np.ascontiguousarray(O.phantom(32, 32, 4)[::4, ::4]))
    grads = []
    for kw in (dict(), dict(downsampler="nearest")):
        eng = _sr_engine(M, autotune=False, **kw)
        assert eng.downsampler == "nearest" and not hasattr(eng, "ds_scratch")
        eng.set_target(target)
        eng.grad_only(0)
        grads.append((eng.grads.clone(), eng.dout.clone(), float(eng.acc[0])))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1]) and grads[0][2] == grads[1][2]


# ---- runner ----------------------------------------------------------------------------------------------------------------------------
def test_runner_lanczos(M, tmp_path):
    from oracle import oracle as O
    kw = dict(img="phantom", imsize=(64, 64), num_iter=3, lr=1e-3, temp=4.4e-7, sigma=4.9e-8, input_depth=8, seed=2, show_every=2, save=True,
              save_path=str(tmp_path), K=2, net_kwargs=SMALL)
    r = M.runner.run_sr_mfvi(downsampler="lanczos2", **kw)
    rn = M.runner.run_sr_mfvi(**kw)
    z, zn = (np.load(os.path.join(x["run_dir"], "save.npz"), allow_pickle=True) for x in (r, rn))
    assert set(z.files) == set(zn.files) == {"img_hr", "img_lr", "mse_noisy", "mse_gt", "recons", "uncerts", "uncerts_ale", "psnrs", "ssims"}
    assert all(z[k].shape == zn[k].shape for k in ("img_hr", "img_lr")) and z["psnrs"].flat[0]["mfvi"].shape == (4, 3)
    assert np.isfinite(r["psnrs"]).all() and np.isfinite(r["ssims"]).all()
    gt = z["img_hr"][0]
    gt_lr = R.forward64(gt, "lanczos2", 4)
    assert np.abs(z["img_lr"] - gt_lr).max() <= R.tolerance("lanczos2", 4, 1.0)             # the target is D(ground truth)
    assert np.array_equal(zn["img_lr"], gt[::4, ::4])
    # psnr_lr = PSNR(D(gt), D(clip(out))): iteration 0 from the stored snapshot (the EMA starts at the output), the last from the engine's output
    psnr = lambda a, b: 10.0 * np.log10(1.0 / np.mean((np.asarray(a, np.float64) - b) ** 2))
    rec0 = z["recons"].flat[0]["mfvi"][0, 0].astype(np.float32)
    assert abs(psnr(gt_lr, R.forward64(rec0, "lanczos2", 4)) - r["psnrs"][0, 0]) < 1e-3
    last = np.clip(host(r["engine"].out)[:, 0].mean(axis=0), 0.0, 1.0)
    assert abs(psnr(gt_lr, R.forward64(last, "lanczos2", 4)) - r["psnrs"][-1, 0]) < 1e-3
    assert abs(O.ssim(gt_lr.astype(np.float32), R.forward64(last, "lanczos2", 4).astype(np.float32)) - r["ssims"][-1, 0]) < 1e-4
    txt = open(os.path.join(r["run_dir"], "locals.txt")).read()
    assert "downsampler = lanczos2" in txt and "downsampler = nearest" in open(os.path.join(rn["run_dir"], "locals.txt")).read()
    # the command-line switch and the config key reach the same runner
    import json
    cfg = json.load(open(os.path.join(R.ROOT, "configs", "mfvi_sr.json")))
    cfg["run_params"].update(imsize=[64, 64], num_iter=1, input_depth=8, show_every=1, save_path=str(tmp_path / "cli"), downsampler="lanczos3")
    cfg["run_params"].pop("devices", None)
    for k in cfg["bo_params"]:
        cfg["bo_params"][k]["candidates"] = cfg["bo_params"][k]["candidates"][:1]
    path = str(tmp_path / "sr.json")
    json.dump(cfg, open(path, "w"))
    (rc,) = M.runner.main(["--task", "super-resolution", "--bayes", "mfvi", "--config", path, "--sr-downsampler", "lanczos2"])
    assert rc["engine"].downsampler == "lanczos2"
    (rc,) = M.runner.main(["--task", "super-resolution", "--bayes", "mfvi", "--config", path])
    assert rc["engine"].downsampler == "lanczos3"
