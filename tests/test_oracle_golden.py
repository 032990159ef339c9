"""Pins the CPU oracle (oracle/mfvi_oracle.c) against golden vectors produced by the
reference's own modules (oracle/make_golden.py).  CPU only."""
import os

import numpy as np
import pytest

from oracle import oracle as O

RTOL = 2e-5   # oracle accumulates in double, the reference in fp32


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)


def test_philox_kat():
    # Random123 known-answer vectors for philox4x32_10
    assert [hex(v) for v in O.philox([0, 0, 0, 0], [0, 0])] == ['0x6627e8d5', '0xe169c58d', '0xbc57ac4c', '0x9b00dbd8']
    assert [hex(v) for v in O.philox([0xffffffff] * 4, [0xffffffff] * 2)] == ['0x408f276d', '0x41c83b0e', '0xa20bc7c6', '0x6d5451fd']
    assert [hex(v) for v in O.philox([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])] == \
        ['0xd16cfe09', '0x94fdcceb', '0x5001e420', '0x24126ea1']


def test_normal_statistics():
    from scipy import stats
    z = O.normal_fill(123, 0, 5, 2, 9, 1 << 20).astype(np.float64)
    assert abs(z.mean()) < 4e-3 and abs(z.std() - 1) < 3e-3
    assert abs(stats.skew(z)) < 1e-2 and abs(stats.kurtosis(z)) < 2e-2
    assert stats.kstest(z[:200000], 'norm').pvalue > 1e-3
    # streams are distinct and reproducible
    assert not np.array_equal(O.eps(1, 0, 0, 3, 0, 64), O.eps(1, 0, 1, 3, 0, 64))
    assert np.array_equal(O.eps(1, 0, 0, 3, 0, 64), O.eps(1, 0, 0, 3, 0, 64))
    assert np.array_equal(O.eps(1, 0, 0, 3, 0, 64)[:10], O.eps(1, 0, 0, 3, 0, 10))
    u = O.uniform_fill(5, 0, 0, 0, 1 << 18)
    assert u.min() >= 0 and u.max() < 1 and abs(u.mean() - 0.5) < 3e-3


def test_single_layers(golden_dir):
    g = load(golden_dir, "layers")
    for ci in range(int(g["n_cases"])):
        cin, cout, k, stride, H, W = [int(v) for v in g[f"case{ci}_shape"]]
        seed = 100 + ci; nw = cout * cin * k * k
        mu = 0.1 * O.normal_fill(seed, 2, 0, 0, 0, nw + cout); rho = -3 + 0.1 * O.normal_fill(seed, 2, 1, 0, 0, nw + cout)
        x = O.normal_fill(seed, 2, 2, 0, 0, cin * H * W).reshape(cin, H, W)
        ew = O.eps(seed, 5, 2, 0, 0, nw); eb = O.eps(seed, 5, 2, 0, 1, cout)
        w = O.reparam(mu[:nw], rho[:nw], ew).reshape(cout, cin, k, k); b = O.reparam(mu[nw:], rho[nw:], eb)
        y = O.conv_fwd(x, w, b, stride)
        assert relerr(y, g[f"case{ci}_y"]) < RTOL, ci
        dy = O.normal_fill(seed, 2, 3, 0, 0, y.size).reshape(y.shape)
        dx, dw, db = O.conv_bwd(x, w, stride, dy)
        sig = 1 / (1 + np.exp(-rho.astype(np.float64)))
        assert relerr(dx, g[f"case{ci}_dx"]) < RTOL, ci
        assert relerr(dw, g[f"case{ci}_dWmu"]) < RTOL, ci
        assert relerr(dw.ravel() * ew * sig[:nw], g[f"case{ci}_dWrho"].ravel()) < RTOL, ci
        assert relerr(db, g[f"case{ci}_dbmu"]) < RTOL, ci
        assert relerr(db * eb * sig[nw:], g[f"case{ci}_dbrho"]) < RTOL, ci


def test_micro(golden_dir):
    g = load(golden_dir, "micro")
    x = O.normal_fill(7, 2, 0, 0, 0, 6 * 10 * 12).reshape(6, 10, 12) * 1.7 + 0.4
    gam = 1 + 0.1 * O.normal_fill(7, 2, 1, 0, 0, 6); bet = 0.1 * O.normal_fill(7, 2, 2, 0, 0, 6)
    ybn, m, r = O.bn_fwd(x, gam, bet)
    y = O.upsample2_fwd(O.lrelu_fwd(ybn))
    assert relerr(y, g["bn_y"]) < RTOL
    dy = O.normal_fill(7, 2, 3, 0, 0, y.size).reshape(y.shape)
    da = O.upsample2_bwd(dy)
    dbn = np.where(ybn > 0, da, 0.2 * da).astype(np.float32)
    dx, dg, db = O.bn_bwd(x, gam, m, r, dbn)
    assert relerr(dx, g["bn_dx"]) < RTOL and relerr(dg, g["bn_dgamma"]) < RTOL and relerr(db, g["bn_dbeta"]) < RTOL
    o = O.normal_fill(8, 2, 0, 0, 0, 2 * 32 * 32).reshape(2, 32, 32).copy(); o[1, 0, :4] = [25.0, -25.0, 20.0, -20.0]
    t = O.uniform_fill(8, 1, 0, 0, 32 * 32).reshape(32, 32)
    v, dmu, ds = O.gaussian_nll(o[0], o[1], t, want_grad=True)
    assert abs(v - float(g["nll"])) < RTOL * abs(float(g["nll"]))
    assert relerr(np.stack([dmu, ds]), g["nll_dout"]) < RTOL
    a = O.phantom(48, 40, 3); b = O.noisy(a, 0.1, 3)
    assert abs(O.psnr(a, b) - float(g["psnr"])) < 1e-4
    assert abs(O.ssim(a, b) - float(g["ssim"])) < 1e-5
    mu = 0.1 * O.normal_fill(9, 2, 0, 0, 0, 40); rho = -3 + 0.5 * O.normal_fill(9, 2, 1, 0, 0, 40)
    klv, dmu, drho = O.kl(mu, rho, np.float32(0.05 + 1e-6), scale=1.0, want_grad=True)
    assert abs(klv - float(g["kl"])) < RTOL * abs(float(g["kl"]))
    assert relerr(dmu, g["kl_dmu"]) < RTOL and relerr(drho, g["kl_drho"]) < RTOL
    theta = np.arange(0, 180., 4., dtype=np.float32)
    img = O.phantom(64, 64, 11)
    s = O.radon_fwd(img, theta)
    assert relerr(s, g["radon64_sino"]) < 5e-5
    rr = O.normal_fill(11, 2, 5, 0, 0, s.size).reshape(s.shape)
    assert relerr(O.radon_adj(rr, theta, 64, 64), g["radon64_adj"]) < 5e-5
    img = O.phantom(256, 256, 11); s = O.radon_fwd(img, theta)
    assert abs(s.astype(np.float64).sum() - float(g["radon256_sino_sum"])) < 1e-5 * abs(float(g["radon256_sino_sum"]))
    st = max(1, s.size // 4096)
    assert relerr(s.ravel()[::st][:4096], g["radon256_sino_s"]) < 5e-5
    p = O.normal_fill(12, 2, 0, 0, 0, 64).copy(); m_ = np.zeros(64, np.float32); v_ = np.zeros(64, np.float32)
    for t_ in range(3):
        O.adam(p, O.normal_fill(12, 2, 1 + t_, 0, 0, 64).copy(), m_, v_, 1e-3, t_ + 1)
    assert relerr(p, g["adam_p"]) < 1e-6


def _golden_params(net, seed):
    mu, rho, bnp = O.init_params(net, seed)
    conv, bn, n_vi, n_bnp = O.net_table(net)
    gg = O.normal_fill(seed, 2, 7, 0, 0, n_bnp)
    for c, off in bn:
        bnp[off:off + c] = 1.0 + 0.1 * gg[off:off + c]; bnp[off + c:off + 2 * c] = 0.1 * gg[off + c:off + 2 * c]
    return mu, rho, bnp


NETS = {
    "small_den_k2": (dict(H=32, W=32, input_depth=8, n_out=2, nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4)), 0),
    "small_sr_k1": (dict(H=32, W=32, input_depth=8, n_out=2, nd=(8, 16), nu=(8, 16), ns=(4, 4)), 1),
    "small_ct_k1": (dict(H=32, W=32, input_depth=8, n_out=1, nd=(8, 16), nu=(8, 16), ns=(4, 4)), 2),
    "full_den_64_k1": (dict(H=64, W=64), 0),
    "full_den_128_k1": (dict(H=128, W=128), 0),
    # BASELINE configs[1] / [2] / [3] nets at 256^2 (strided fixtures) and the bf16-parameter twin of the 128^2 den net (configs[4])
    "full_den_256_k1": (dict(H=256, W=256), 0),
    "full_sr256_d32_k1": (dict(H=256, W=256, input_depth=32), 1),
    "full_ct_256_k1": (dict(H=256, W=256, n_out=1), 2),
    "full_den_128_k1_bf16": (dict(H=128, W=128), 0),
    # sides not divisible by 2^n_scales: Concat's centre-crop (models/common.py:29-41) at the deepest scale, in both dimensions
    "crop_den_36x44_k1": (dict(H=36, W=44, input_depth=8, n_out=2, nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4)), 0),
}


def _strided(a, n=4096):
    a = np.asarray(a).ravel(); st = max(1, a.size // n)
    return a[::st][:n]


@pytest.mark.parametrize("name", list(NETS))
def test_net_elbo_grad(golden_dir, name):
    g = load(golden_dir, name)
    kw, task = NETS[name]
    net = O.make_net(**kw)
    seed, K = int(g["seed"]), int(g["K"])
    mu, rho, bnp = _golden_params(net, seed)
    if name.endswith("_bf16"):
        mu, rho = O.bf16_round(mu), O.bf16_round(rho)          # the values a bf16 parameter store holds
    H, W = net.H, net.W
    z = (0.1 * O.uniform_fill(seed, 0, 0, 0, net.input_depth * H * W)).reshape(net.input_depth, H, W)
    img = O.phantom(H, W, seed); tgt = O.noisy(img, 0.1, seed)
    theta = None
    if task == 1:
        tgt = np.ascontiguousarray(tgt[::4, ::4])
    if task == 2:
        theta = np.arange(0, 180., 4., dtype=np.float32)
        tgt = O.radon_fwd(img, theta)
        assert relerr(tgt, g["sino_target"]) < 5e-5
    r = O.elbo_grad(net, mu, rho, bnp, z, tgt, task=task, factor=4, theta_deg=theta, seed=seed, step=int(g["step"]), K=K,
                    temp=float(g["temp"]), prior_sigma=float(g["prior_sigma"]), want_out=True)
    assert relerr(r["out"], g["out"]) < RTOL
    assert abs(r["nll"] - float(g["nll"])) < 3e-5 * abs(float(g["nll"]))
    assert abs(r["kl"] - float(g["kl"])) < 1e-6 * abs(float(g["kl"]))
    assert abs(r["loss"] - float(g["loss"])) < 3e-5 * abs(float(g["loss"]))
    # gradient tolerance vs the float64 twin.  SR at 256^2 back-propagates through 1/16 of the pixels and CT through a 45-angle sinogram:
    # one LeakyReLU-kink flip weighs more there (the fp32 REFERENCE itself is 7e-3 / 1.4e-4 off its float64 twin on these two)
    gt = {"full_sr256_d32_k1": 6e-4, "full_ct_256_k1": 3e-4}.get(name, 5e-5)
    if "dmu" in g.files:
        assert relerr(r["dmu"], g["dmu"]) < gt and relerr(r["drho"], g["drho"]) < gt
        assert relerr(r["dbn"], g["dbn"]) < gt
    else:
        # Full 26-layer net: the fp32 reference's own gradients are only accurate to ~1e-3 (deepest BN
        # normalises over (H/32)^2 pixels), so the tight pin is the SAME reference code run in float64
        # (keys *_f64); the fp32 run is checked at its measured noise floor.
        conv, _, _, _ = O.net_table(net)
        ds_ = r["dmu"][::max(1, r["dmu"].size // 4096)][:4096]; rs_ = r["drho"][::max(1, r["drho"].size // 4096)][:4096]
        ln = np.array([np.linalg.norm(r["dmu"][int(c[4]):int(c[5]) + int(c[1])]) for c in conv])
        assert relerr(ds_, g["dmu_s_f64"]) < gt and relerr(rs_, g["drho_s_f64"]) < gt
        assert relerr(ln, g["dmu_layer_norm_f64"]) < gt and relerr(r["dbn"], g["dbn_f64"]) < gt
        if "out_f64" in g.files:
            assert relerr(r["out"], g["out_f64"]) < 1e-5
        else:
            assert relerr(_strided(r["out"], 16384), g["out_s_f64"]) < 1e-5
        ft = 1.5e-2 if name == "full_sr256_d32_k1" else 5e-3
        assert relerr(ds_, g["dmu_s"]) < ft and relerr(rs_, g["drho_s"]) < ft and relerr(r["dbn"], g["dbn"]) < ft
    # per-layer KL (VIModule._kl) and the RNG-free eval anchor
    conv, _, _, _ = O.net_table(net)
    pl = [O.kl(mu[int(c[4]):int(c[5]) + int(c[1])], rho[int(c[4]):int(c[5]) + int(c[1])], float(g["prior_sigma"])) for c in conv]
    assert relerr(pl, g["per_layer_kl"]) < 1e-6
    out_eval, tape = O.net_forward(net, mu, rho, bnp, z, seed, 0, 0, sample_weights=False)
    tape.free()
    if "out_eval" in g.files:
        assert relerr(out_eval, g["out_eval"]) < RTOL
    else:
        assert relerr(_strided(out_eval, 16384), g["out_eval_s"]) < RTOL


@pytest.mark.parametrize("lay", ["fitted", "pruned"])
def test_net_grad_away_from_the_initial_posterior(golden_dir, lay):
    """tests/golden/posterior_range.npz (oracle/make_golden.py, golden_posterior): the reference's float64 autograd on three_scale_32 at a
    fitted (rho ~ -13.8) and a pruned (a quarter of the weights at rho = -200, mu = 0) posterior, data term only -- at small_den_k2's
    tolerances, and drho once more through q = drho / sigmoid(rho) per layer (tests/posterior_cases.py), which the fitted weights do not
    hide behind the few largest entries."""
    import posterior_cases as PC
    import mfvi_dip_mia_amd as M
    g = load(golden_dir, "posterior_range")
    kw = PC.NETS["three_scale_32"]
    net = O.make_net(**kw)
    seed, K, step = int(g["seed"]), int(g["K"]), int(g["step"])
    P, zin, out_id, _ = M.skip_program(**kw)
    mu, rho, bnp = PC.net_params(P, lay, seed)
    assert np.array_equal(mu, g[lay + "_mu"]) and np.array_equal(rho, g[lay + "_rho"])          # the layout is the one the reference ran
    z = PC.net_input(kw, seed)
    tgt = O.noisy(O.phantom(net.H, net.W, seed), 0.1, seed)
    r = O.elbo_grad(net, mu, rho, bnp, z, tgt, task=0, seed=seed, step=step, K=K, with_kl=False, want_out=True)
    assert relerr(r["out"], g[lay + "_out"]) < RTOL
    assert abs(r["nll"] - float(g[lay + "_nll"])) < 3e-5 * abs(float(g[lay + "_nll"]))
    assert relerr(r["dmu"], g[lay + "_dmu"]) < 5e-5 and relerr(r["drho"], g[lay + "_drho"]) < 5e-5 and relerr(r["dbn"], g[lay + "_dbn"]) < 5e-5
    worst, rows = PC.layer_q_err(r["drho"], PC.q_of(g[lay + "_drho"], rho), rho, P.layers)
    assert worst < 5e-5, rows
    pruned = rho == np.float32(PC.PRUNED_RHO)
    assert pruned.any() == (lay == "pruned") and np.all(np.abs(g[lay + "_drho"][pruned]) < 1e-30) and np.all(np.abs(r["drho"][pruned]) < 1e-30)
    assert np.isfinite(g[lay + "_drho"]).all()


@pytest.mark.parametrize("name", ["traj_small_k1", "traj_small_k2"])
def test_trajectory(golden_dir, name):
    """N steps of the loop bayesian_optimization.py:1360-1372 (torch AdamW in the golden run)."""
    g = load(golden_dir, name)
    net = O.make_net(32, 32, input_depth=8, n_out=2, nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4))
    seed, K, steps, lr = int(g["seed"]), int(g["K"]), int(g["steps"]), float(g["lr"])
    mu, rho, bnp = _golden_params(net, seed)
    H, W = net.H, net.W
    z0 = (0.1 * O.uniform_fill(seed, 0, 0, 0, net.input_depth * H * W)).reshape(net.input_depth, H, W)
    tgt = O.noisy(O.phantom(H, W, seed), 0.1, seed)
    p = np.concatenate([mu, rho, bnp]); m = np.zeros_like(p); v = np.zeros_like(p)
    n_vi = mu.size
    for it in range(steps):
        z = z0 + 0.1 * O.normal_fill(seed, 1, 0, 0, it, z0.size).reshape(z0.shape)
        r = O.elbo_grad(net, p[:n_vi], p[n_vi:2 * n_vi], p[2 * n_vi:], z, tgt, seed=seed, step=it, K=K,
                        temp=float(g["temp"]), prior_sigma=float(g["prior_sigma"]))
        assert abs(r["loss"] - g["loss"][it]) < 2e-4 * max(1.0, abs(g["loss"][it])), (it, r["loss"], g["loss"][it])
        grad = np.concatenate([r["dmu"], r["drho"], r["dbn"]])
        O.adam(p, grad, m, v, lr, it + 1)
    # Adam normalises by sqrt(v): elements with near-zero gradients move by ~lr whatever the fp32 noise says,
    # so parameters are compared to within one step (lr = 1e-3 absolute); the loss trajectory above is tight.
    assert np.abs(p[:n_vi] - g["mu"]).max() < 1e-3 and np.abs(p[n_vi:2 * n_vi] - g["rho"]).max() < 1e-3
    assert np.abs(p[:n_vi] - g["mu"]).mean() < 2e-6


def test_inpainting_ops(golden_dir):
    """The ops only the inpainting variant uses (5x5 Conv2dRT, nearest upsampling, sigmoid + masked NLL) against the
    reference's own modules (oracle/make_golden.py::golden_inpainting)."""
    g = load(golden_dir, "inpainting")
    for ci in range(2):
        cin, cout, k, stride, H, W = [int(v) for v in g[f"conv{ci}_shape"]]
        seed = 300 + ci; nw = cout * cin * k * k
        mu = 0.1 * O.normal_fill(seed, 2, 0, 0, 0, nw + cout); rho = -3 + 0.1 * O.normal_fill(seed, 2, 1, 0, 0, nw + cout)
        x = O.normal_fill(seed, 2, 2, 0, 0, cin * H * W).reshape(cin, H, W)
        ew = O.eps(seed, 5, 2, 0, 0, nw); eb = O.eps(seed, 5, 2, 0, 1, cout)
        w = O.reparam(mu[:nw], rho[:nw], ew).reshape(cout, cin, k, k); b = O.reparam(mu[nw:], rho[nw:], eb)
        y = O.conv_fwd(x, w, b, stride)
        assert relerr(y, g[f"conv{ci}_y"]) < RTOL, ci
        dy = O.normal_fill(seed, 2, 3, 0, 0, y.size).reshape(y.shape)
        dx, dw, db = O.conv_bwd(x, w, stride, dy)
        sig = 1 / (1 + np.exp(-rho.astype(np.float64)))
        assert relerr(dx, g[f"conv{ci}_dx"]) < RTOL, ci
        assert relerr(np.concatenate([dw.ravel(), db]), g[f"conv{ci}_dmu"]) < RTOL, ci
        assert relerr(np.concatenate([dw.ravel() * ew * sig[:nw], db * eb * sig[nw:]]), g[f"conv{ci}_drho"]) < RTOL, ci
    x = O.normal_fill(310, 2, 0, 0, 0, 3 * 5 * 7).reshape(3, 5, 7)
    assert np.array_equal(O.upsample2_nearest_fwd(x), g["up_y"])
    dy = O.normal_fill(310, 2, 1, 0, 0, 3 * 10 * 14).reshape(3, 10, 14)
    assert relerr(O.upsample2_nearest_bwd(dy), g["up_dx"]) < 1e-6
    H, W = 12, 20
    o = (2.0 * O.normal_fill(311, 2, 0, 0, 0, 4 * H * W)).reshape(4, H, W).copy(); o[3, 0, :4] = [25.0, -30.0, 19.9, 0.0]
    tgt = O.uniform_fill(311, 1, 0, 0, 3 * H * W).reshape(3, H, W)
    for mc in (1, 3):
        mask = (O.uniform_fill(311, 2 + mc, 0, 0, mc * H * W).reshape(mc, H, W) > 0.3).astype(np.float32)
        v, d = O.gaussian_nll_inp(o, tgt, mask, want_grad=True)
        assert abs(v - float(g[f"nll_mask{mc}"])) < 2e-5 * abs(float(g[f"nll_mask{mc}"]))
        assert relerr(d, g[f"nll_mask{mc}_dout"]) < RTOL


SIB_NET = dict(input_depth=8, n_out=2, nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4))


def oracle_sibling_traj(g, method, on_step0=None):
    """The siblings' loop restated with the oracle: [add_noise] -> forward (w = mu, Dropout2d masks from the spec) -> MSE / NLL ->
    backward -> AdamW(wd) [-> ExponentialLR].  Returns (losses, mu, bn)."""
    H, W, steps, seed, lr0 = int(g["H"]), int(g["W"]), int(g["steps"]), int(g["seed"]), float(g["lr"])
    p_drop, wd, gamma = float(g[method + "_p"]), float(g[method + "_wd"]), float(g[method + "_gamma"])
    net = O.make_net(H, W, drop_down=p_drop, drop_up=p_drop, **SIB_NET)
    conv, _, n_vi, n_bnp = O.net_table(net)
    mu, _, bnp = _golden_params(net, seed)
    z0 = (0.1 * O.uniform_fill(seed, 0, 0, 0, net.input_depth * H * W)).reshape(net.input_depth, H, W)
    tgt = O.noisy(O.phantom(H, W, seed), 0.1, seed)
    m1, v1, m2, v2 = np.zeros_like(mu), np.zeros_like(mu), np.zeros_like(bnp), np.zeros_like(bnp)
    lr = lr0; losses = []
    for it in range(steps):
        if method == "sgld":
            for lid, c in enumerate(conv):
                n_w = int(c[0] * c[1] * c[2] * c[2]); w_off = int(c[4])
                mu[w_off:w_off + n_w] = mu[w_off:w_off + n_w] + O.normal_fill(seed, 4, lid, 0, it, n_w) * np.float32(2 * lr0)
        z = z0 + 0.1 * O.normal_fill(seed, 1, 0, 0, it, z0.size).reshape(z0.shape)
        r = O.sibling_grad(net, mu, bnp, z, tgt, loss="gnll" if method == "mcd" else "mse0", seed=seed, step=it, want_out=True)
        if it == 0 and on_step0:
            on_step0(r)
        losses.append(r["loss"])
        O.adamw(mu, r["dmu"], m1, v1, lr, it + 1, wd); O.adamw(bnp, r["dbn"], m2, v2, lr, it + 1, wd)
        if method == "sgld" and lr > 1e-8:
            lr *= gamma
    return np.array(losses), mu, bnp


@pytest.mark.parametrize("method", ["dip", "mcd", "sgld"])
def test_siblings(golden_dir, method):
    """DIP / MC-dropout / SGLD (bayesian_optimization.py:1064-1237, 1447-1860) against the reference's skip() net with plain
    nn.Conv2d (and its own nn.Dropout2d layers), torch AdamW(weight_decay) + ExponentialLR."""
    g = load(golden_dir, "siblings")

    def first(r):
        assert relerr(r["out"][0], g[method + "_out0"]) < RTOL
        assert relerr(r["dmu"], g[method + "_dmu0"]) < 1e-4 and relerr(r["dbn"], g[method + "_dbn0"]) < 1e-4
    losses, mu, bnp = oracle_sibling_traj(g, method, first)
    assert np.abs(losses - g[method + "_loss"]).max() < 2e-4 * np.abs(g[method + "_loss"]).max(), (losses, g[method + "_loss"])
    # Adam moves an element whose gradient is at the fp32 noise floor by up to lr per step in either direction: the maximum is
    # bounded by steps * lr, the mean stays tight (as in test_trajectory)
    bound = int(g["steps"]) * float(g["lr"])
    assert np.abs(mu - g[method + "_mu"]).max() < bound and np.abs(mu - g[method + "_mu"]).mean() < 2e-6
    assert np.abs(bnp - g[method + "_bn"]).max() < bound


def test_dropout_mask_spec():
    d = O.dropout_mask(5, 3, 1, 7, 0.3, 4096)
    assert set(np.unique(d)) == {np.float32(0.0), np.float32(1.0) / (np.float32(1.0) - np.float32(0.3))}
    assert abs((d == 0).mean() - 0.3) < 0.03
    assert not np.array_equal(d, O.dropout_mask(5, 3, 2, 7, 0.3, 4096))      # keyed by the sample
    assert not np.array_equal(d, O.dropout_mask(5, 4, 1, 7, 0.3, 4096))      # ... and the step


def test_inp_dip_loss(golden_dir):
    """run_inp_dip's masked MSE on the sigmoid output (bayesian_optimization.py:2824-2826), 1- and 3-channel masks."""
    g = load(golden_dir, "inp_dip_loss")
    for mc in (1, 3):
        v, d = O.mse_sigmoid_masked(g["out%d" % mc], g["img%d" % mc], g["mask%d" % mc], 1.0, want_grad=True)
        assert abs(v - float(g["loss%d" % mc])) < 1e-6 * abs(float(g["loss%d" % mc]))
        assert relerr(d, g["grad%d" % mc]) < 1e-5 and np.all(d[3] == 0)


def _bookkeeping_case(g, task):
    """(Bookkeeper, per-iteration raw outputs [n_it][1][C][H][W]) of one golden bookkeeping case."""
    if task.startswith("inp"):
        H, W, C = [int(v) for v in g["inp_shape"]]; seed = 64; mc = int(task[3:])
        img = np.stack([O.phantom(H, W, seed + c) for c in range(3)])
        mask = (O.uniform_fill(seed, 2 + mc, 0, 0, mc * H * W).reshape(mc, H, W) > 0.3).astype(np.float32)
        bk = O.Bookkeeper("inp", H, W, img, mask=mask)
        raws = [O.bookkeeping_raw("inp", seed, i, img, 4)[None] for i in range(int(g["n_it"]))]
        return bk, raws
    H, W, C = [int(v) for v in g[task + "_shape"]]; seed = dict(den=61, sr=62, ct=63)[task]
    img = O.phantom(H, W, seed)
    bk = O.Bookkeeper(task, H, W, img, noisy=O.noisy(img, 0.1, seed))
    return bk, [O.bookkeeping_raw(task, seed, i, img, C)[None] for i in range(int(g["n_it"]))]


@pytest.mark.parametrize("task", ["den", "sr", "ct", "inp1", "inp3"])
def test_bookkeeping(golden_dir, task):
    """The oracle's restatement of the runners' bookkeeping (EMA 0.99, clips, 25-slot rings, unbiased var, LR metrics of the SR
    runner, masked metrics of the inpainting runner) against the reference's torch ops / PSNR / SSIM (bookkeeping.npz)."""
    g = load(golden_dir, "bookkeeping")
    bk, raws = _bookkeeping_case(g, task)
    M = g[task + "_metrics"]
    for i, raw in enumerate(raws):
        row = bk.step(raw)
        assert relerr(row, M[i]) < 5e-5, (task, i, row, M[i])
        if i in (10, 27):
            var, ale, recon = bk.snapshot()
            assert relerr(var, g["%s_var%d" % (task, i)]) < 2e-5
            assert relerr(recon, g["%s_recon%d" % (task, i)]) < 1e-6
            if task != "ct":
                assert relerr(ale, g["%s_ale%d" % (task, i)]) < 1e-6
    assert relerr(bk.ema, g[task + "_ema"]) < 1e-6


def test_lrt_layers(golden_dir):
    """The oracle's Conv2dLRT (local reparameterisation in activation space, oracle.lrt_conv) against the reference's own layer."""
    g = load(golden_dir, "lrt")
    for ci in range(int(g["n_cases"])):
        cin, cout, k, stride, H, W = [int(v) for v in g[f"case{ci}_shape"]]
        seed = 400 + ci
        nw = cout * cin * k * k
        mu = 0.1 * O.normal_fill(seed, 2, 0, 0, 0, nw + cout); rho = -3 + 0.5 * O.normal_fill(seed, 2, 1, 0, 0, nw + cout)
        x = O.normal_fill(seed, 2, 2, 0, 0, cin * H * W).reshape(cin, H, W)
        yg = g[f"case{ci}_y"]
        eps = O.lrt_eps(seed, 5, 2, 0, yg.size)
        dy = O.normal_fill(seed, 2, 3, 0, 0, yg.size).reshape(yg.shape)
        y, dx, dwm, dwr, dbm, dbr = O.lrt_conv(x, mu[:nw].reshape(cout, cin, k, k), rho[:nw].reshape(cout, cin, k, k), mu[nw:], rho[nw:], eps, stride, dy)
        assert relerr(y, yg) < RTOL and relerr(dx, g[f"case{ci}_dx"]) < RTOL, ci
        assert relerr(np.r_[dwm.ravel(), dbm], g[f"case{ci}_dmu"]) < RTOL and relerr(np.r_[dwr.ravel(), dbr], g[f"case{ci}_drho"]) < 5e-5, ci
        assert relerr(O.conv_fwd(x, mu[:nw].reshape(cout, cin, k, k), mu[nw:], stride), g[f"case{ci}_y_eval"]) < RTOL
    assert set(g["net_layer_types"]) == {"Conv2dLRT"}
