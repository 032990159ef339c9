"""Batched DIP / MC-dropout / SGLD fits: the plan's points mode and per-fit dropout against single-fit passes,
SiblingBatch against the oracle per fit, fit 0 against the standalone SiblingEngine, the three per-fit kernels against the entry points
they generalise, NaN isolation, the refusals, to_engine and the runner's --sibling-fits.

Net A, Net B, their tilings (pin_net_b) and the per-fit BatchNorm values are those of tests/test_gpu_fitbatch.py.  Every parity test first
writes distinct BatchNorm parameters per fit: at initialisation all fits have gamma = 1, beta = 0 and an indexing error would be invisible."""
import json
import math
import os

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_fitbatch import NET_B, SMALL, _ulp_diff, bn_values, dev, families, host, pin_net_b, relerr, write_bn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GEN_NET = dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4))      # at 40 x 40: maps 20, 10 and 5 wide -- the last two on the generic kernels
FAM_GENERIC = 0


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    assert torch.cuda.is_available()
    M_._lib.lib()
    return M_


def sibling_init(prog, seed, f):
    """nn.Conv2d's kaiming-uniform init as SiblingEngine draws it: U(-b, b), b = 1 / sqrt(fan_in), stream 16 + layer, sample f."""
    mu = np.zeros(prog.n_vi, np.float32)
    for lid, lay in enumerate(prog.layers):
        b = 1.0 / math.sqrt(lay["cin"] * lay["k"] * lay["k"])
        n = lay["cout"] * lay["cin"] * lay["k"] * lay["k"] + (lay["cout"] if lay["b_off"] >= 0 else 0)
        mu[lay["w_off"]:lay["w_off"] + n] = -b + 2.0 * b * O.uniform_fill(seed, 16 + lid, f, 0, n)
    return mu


def _rows(P, F, seed, stride, depth, H, W):
    nv, n_params = P.n_vi, 2 * P.n_vi + P.n_bn
    rows = np.zeros((F, stride), np.float32)
    for f in range(F):
        rows[f, :nv] = 0.1 * O.normal_fill(seed, 2, 0, f, 0, nv)
        rows[f, nv:2 * nv] = -3.0 + 0.1 * O.normal_fill(seed, 2, 1, f, 0, nv)      # never read: the weights are mu
        rows[f, 2 * nv:n_params] = bn_values(P, seed, f)
    z = np.stack([0.1 * O.uniform_fill(seed, 0, f, 0, depth * H * W).reshape(depth, H, W) for f in range(F)]).astype(np.float32)
    return rows, z


def _compare_with_single_fit(P, pf, ps, F, S, rows, z, stride, H, W, seed, step, tag):
    """One fits-mode forward + backward of pf (w = mu) against F single-fit passes of ps with sample_weights=False, k0 = f S.  Bounds: the
    project's for this comparison (tests/test_gpu_fitbatch.py): outputs 1e-5, dmu and dbn 2e-4 relative to the largest reference value."""
    n, nv = F * S, P.n_vi
    n_params = 2 * nv + P.n_bn
    dout = (O.normal_fill(seed, 2, 3, 0, 0, n * 2 * H * W).reshape(n, 2, H, W) / (H * W)).astype(np.float32)
    d_rows, d_z, d_dout = dev(rows), dev(z), dev(dout)
    g = torch.zeros((F, stride), device="cuda")
    out = pf.forward(d_rows[0, :nv], d_rows[0, nv:], d_rows[0, 2 * nv:], d_z, seed, step, 0, n, False)
    pf.backward(d_rows[0, :nv], d_rows[0, nv:], d_rows[0, 2 * nv:], d_z, seed, step, 0, n, d_dout, g[0, :nv], g[0, nv:], g[0, 2 * nv:], False)
    out, g = host(out), host(g)
    assert np.all(g[:, nv:2 * nv] == 0.0), "the RHO block of a gradient row is not touched"
    assert np.all(g[:, n_params:] == 0.0), "nothing is written between the rows"
    for f in range(F):
        r = d_rows[f]
        gs = torch.zeros(n_params, device="cuda")
        o = ps[f].forward(r[:nv], r[nv:2 * nv], r[2 * nv:n_params], d_z[f], seed, step, f * S, S, False)
        ps[f].backward(r[:nv], r[nv:2 * nv], r[2 * nv:n_params], d_z[f], seed, step, f * S, S, d_dout[f * S:(f + 1) * S].contiguous(), gs[:nv], gs[nv:2 * nv],
                       gs[2 * nv:], False)
        o, gs = host(o), host(gs)
        e = relerr(out[f * S:(f + 1) * S], o)
        print("%s F=%d S=%d fit %d: out %.2e" % (tag, F, S, f, e))
        assert e < 1e-5, (tag, f, e)
        for name, a, b in (("dmu", g[f, :nv], gs[:nv]), ("dbn", g[f, 2 * nv:n_params], gs[2 * nv:])):
            e = relerr(a, b)
            print("    %s %.2e" % (name, e))
            assert e < 2e-4, (tag, f, name, e)
    return out


# ---- 1. points mode ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,S", [(4, 1), (3, 2)])
def test_points_mode_matches_single_fit_passes(M, F, S):
    """Net B with the tilings of pin_net_b on both sides.  A single-fit w = mu pass draws nothing, so it has no slab and no bf16x6 weight
    pieces: its 36 -> 16 layer runs the fp32 row-phase kernel where the points-mode pass runs bf16x6, and the activations of the two sides
    differ in their last bits.  An element within those bits of LeakyReLU's kink then takes the other slope on one side, and one such element
    under a large output gradient sets the max-norm error of the whole comparison.  That is a property of the data, not of either pass: seed
    31 of tests/test_gpu_fitbatch.py has such an element in fit 2 (dmu 6.6e-3 at F, S = 4, 1 and 4.1e-4 at 3, 2; every tensor of that sample is
    within 2e-5 of the single-fit pass when both sides run the same kernels); seeds 32 .. 38 have none (all within the bounds)."""
    H = W = 64; seed, step = 32, 5
    P, zin, zout, _ = M.skip_program(H, W, 16, 2, **NET_B)
    stride = (2 * P.n_vi + P.n_bn + 3) // 4 * 4 + 8                       # rows further apart than they are long
    rows, z = _rows(P, F, seed, stride, 16, H, W)
    pf = P.compile(zin, zout, F * S); pin_net_b(M, pf); pf.set_fits(S, stride, stride); pf.set_fits_points(True)
    ps = P.compile(zin, zout, S); pin_net_b(M, ps)
    _compare_with_single_fit(P, pf, [ps] * F, F, S, rows, z, stride, H, W, seed, step, "net B")
    fam = families(M, pf)
    assert {2, 3, 4} <= fam, "row-phase, bf16x6 and one-stage kernels must each serve an op of the points-mode pass: %s" % (fam,)


@pytest.mark.parametrize("F,S", [(4, 1), (3, 2)])
def test_points_mode_on_the_generic_kernels(M, F, S):
    H = W = 40; seed, step = 32, 3
    P, zin, zout, _ = M.skip_program(H, W, 8, 2, **GEN_NET)
    stride = (2 * P.n_vi + P.n_bn + 3) // 4 * 4 + 8
    rows, z = _rows(P, F, seed, stride, 8, H, W)
    pf = P.compile(zin, zout, F * S); pf.set_fits(S, stride, stride); pf.set_fits_points(True)
    ps = P.compile(zin, zout, S)
    _compare_with_single_fit(P, pf, [ps] * F, F, S, rows, z, stride, H, W, seed, step, "generic")
    fam = families(M, pf)
    assert FAM_GENERIC in fam and any(x > 0 for x in fam), fam


# ---- 2. per-fit dropout ---------------------------------------------------------------------------------------------------------------------
def test_per_fit_dropout_matches_single_fit_plans(M):
    H = W = 32; F, S, seed, step = 3, 2, 33, 4
    ps_ = (0.1, 0.3, 0.5)
    P, zin, zout, _ = M.skip_program(H, W, 8, 2, drop_down=max(ps_), drop_up=max(ps_), **SMALL)
    nv, n_params = P.n_vi, 2 * P.n_vi + P.n_bn
    stride = (n_params + 3) // 4 * 4 + 8
    rows, z = _rows(P, F, seed, stride, 8, H, W)
    # the test's own discriminating power, on the CPU: the oracle for fit 0 with fit 1's p misses the right gradient by > 100 x the bound
    tgt = O.noisy(O.phantom(H, W, seed), 0.1, seed)
    grads = []
    for p in ps_[:2]:
        net = O.make_net(H, W, input_depth=8, n_out=2, drop_down=p, drop_up=p, **SMALL)
        grads.append(O.sibling_grad(net, rows[0, :nv], rows[0, 2 * nv:n_params], z[0], tgt, loss="gnll", seed=seed, step=step, k0=0, K=S)["dmu"])
    d = relerr(grads[1], grads[0])
    print("fit 1's p in fit 0's oracle moves dmu by %.2e" % d)
    assert d > 100 * 2e-4, d
    pf = P.compile(zin, zout, F * S); pf.set_fits(S, stride, stride); pf.set_fits_points(True); pf.set_fit_dropout(ps_)
    singles = []
    for p in ps_:
        Q, qi, qo, _ = M.skip_program(H, W, 8, 2, drop_down=p, drop_up=p, **SMALL)
        assert (Q.n_vi, Q.n_bn) == (P.n_vi, P.n_bn)
        singles.append(Q.compile(qi, qo, S))
    out = _compare_with_single_fit(P, pf, singles, F, S, rows, z, stride, H, W, seed, step, "dropout")
    assert np.abs(out[0] - out[1]).max() > 1e-3                            # different masks per sample
    # a fit whose p equals the plan's own: bit-equal to a pass without per-fit probabilities
    d_rows, d_z = dev(rows), dev(z)
    pf.set_fit_dropout(None)
    plain = host(pf.forward(d_rows[0, :nv], d_rows[0, nv:], d_rows[0, 2 * nv:], d_z, seed, step, 0, F * S, False))
    assert np.array_equal(out[2 * S:3 * S], plain[2 * S:3 * S])
    assert not np.array_equal(out[:S], plain[:S])
    # p = 0: factors of 1 -- the net without dropout
    pf.set_fit_dropout([0.0, 0.0, 0.0])
    none = host(pf.forward(d_rows[0, :nv], d_rows[0, nv:], d_rows[0, 2 * nv:], d_z, seed, step, 0, F * S, False))
    Q, qi, qo, _ = M.skip_program(H, W, 8, 2, **SMALL)
    q = Q.compile(qi, qo, S)
    o = host(q.forward(d_rows[1, :nv], d_rows[1, nv:2 * nv], d_rows[1, 2 * nv:n_params], d_z[1], seed, step, S, S, False))
    assert relerr(none[S:2 * S], o) < 1e-5


# ---- 3. against the oracle ------------------------------------------------------------------------------------------------------------------
LRS, WDS, PS, GAMMAS = [1e-3, 5e-4, 7.5e-4], [0.0, 1.0, 2.0], [0.1, 0.3, 0.5], [0.9, 0.99, 0.999]


def _batch(M, method, task, F=3, K=None, seed=4, **kw):
    K = (2 if method == "mcd" else 1) if K is None else K
    return M.SiblingBatch(32, 32, F, method, task=task, K=K, input_depth=8, lr=LRS[:F], weight_decay=WDS[:F], dropout_p=PS[:F], gamma=GAMMAS[:F],
                          seed=seed, net_kwargs=SMALL, autotune=False, **kw)


def _targets(task, F, seed, H=32, W=32):
    tg = []
    for f in range(F):
        img = O.phantom(H, W, seed + f)
        tg.append(O.noisy(img, 0.1, seed + f) if task == "den" else np.ascontiguousarray(img[::4, ::4]))
    return np.stack(tg).astype(np.float32)


@pytest.mark.parametrize("method,task", [("dip", "den"), ("mcd", "den"), ("mcd", "sr"), ("sgld", "den"), ("sgld", "sr")])
def test_batch_steps_match_oracle_per_fit(M, method, task):
    """Three iterations of F = 3 fits, every fit with its own lr, weight decay, p or gamma, target and BN parameters: each fit against
    O.sibling_grad and O.adamw under the bounds tests/test_gpu_siblings.py applies to one engine -- loss and gradients against the oracle
    (den: 2e-5 and 2e-4; sr: 5e-5 and 3e-4), the AdamW update against O.adamw on the same gradient (2e-6 absolute, its bound for
    mfvi_adamw_step: Adam divides by the gradient's magnitude, so the update of a noise-floor gradient is not a function of the oracle's
    gradient to any useful bound, and the two comparisons are made one after the other) -- re-anchored after every step."""
    H = W = 32; F, seed = 3, 4
    sb = _batch(M, method, task)
    K, n = sb.K, sb.n_vi
    lb, gb = (2e-5, 2e-4) if task == "den" else (5e-5, 3e-4)
    loss = "mse0" if sb.mse_image else "gnll"
    tg = _targets(task, F, seed)
    sb.set_targets(torch.from_numpy(tg))
    p0, z0 = host(sb.params), host(sb.z0)
    for f in range(F):                                                     # initial values: sample f of the kaiming-uniform and z0 streams
        assert np.abs(p0[f, :n] - sibling_init(sb.prog, seed, f)).max() < 1e-7
        assert np.all(p0[f, n:2 * n] == 0.0)
        assert np.abs(z0[f].ravel() - 0.1 * O.uniform_fill(seed, 0, f, 0, z0[f].size)).max() < 1e-8
    assert not np.array_equal(p0[0], p0[1]) and not np.array_equal(z0[0], z0[1])
    write_bn(sb, seed)
    p = host(sb.params).copy()
    m = np.zeros_like(p); v = np.zeros_like(p)
    nets = [O.make_net(H, W, input_depth=8, n_out=2, drop_down=sb.dropout_ps[f], drop_up=sb.dropout_ps[f], **SMALL) for f in range(F)]
    lr = list(LRS)

    def noise(f, it, mu):
        mu = mu.copy()
        if method == "sgld":
            std = np.float32(sb.param_noise_sigma * LRS[f])
            for lid, lay in enumerate(sb.prog.layers):
                cnt = lay["cout"] * lay["cin"] * lay["k"] * lay["k"]
                mu[lay["w_off"]:lay["w_off"] + cnt] += std * O.normal_fill(seed, 4, lid, f, it, cnt)
        return mu

    def oracle(f, it, mu):
        z = z0[f] + 0.1 * O.normal_fill(seed, 1, 0, f, it, z0[f].size).reshape(z0[f].shape)
        return O.sibling_grad(nets[f], mu, p[f, 2 * n:], z, tg[f], loss=loss, seed=seed, step=it, k0=f * K, K=K, factor=4 if task == "sr" else 1)

    def update(f, it, mu, r, lr_f, wd_f):
        q, mm, vv = p[f].copy(), m[f].copy(), v[f].copy()
        q[:n] = mu
        for lo, hi, g_ in ((0, n, r["dmu"]), (2 * n, q.size, r["dbn"])):
            a, b, c = q[lo:hi].copy(), mm[lo:hi].copy(), vv[lo:hi].copy()
            O.adamw(a, np.asarray(g_, np.float32), b, c, float(np.float32(lr_f)), it + 1, wd_f)
            q[lo:hi], mm[lo:hi], vv[lo:hi] = a, b, c
        return q, mm, vv

    # the test's own discriminating power, on the CPU: with ANOTHER fit's weight decay or lr the update of fit 0 moves a parameter by more
    # than 100 x the bound the update is compared under
    mu0 = noise(0, 0, p[0, :n]); r0 = oracle(0, 0, mu0)
    right = update(0, 0, mu0, r0, LRS[0], WDS[0])[0]
    for kind, wrong in (("weight decay", update(0, 0, mu0, r0, LRS[0], WDS[1])[0]), ("lr", update(0, 0, mu0, r0, LRS[1], WDS[0])[0])):
        d = float(np.abs(wrong - right).max())
        print("%s/%s: fit 1's %s moves a parameter of fit 0 by %.2e" % (method, task, kind, d))
        assert d > 100 * 2e-6, (kind, d)
    for it in range(3):
        sb.step()
        losses = sb.losses()
        pn, gn = host(sb.params), host(sb.grads)
        for f in range(F):
            mu = noise(f, it, p[f, :n])
            r = oracle(f, it, mu)
            eg, eb = relerr(gn[f, :n], r["dmu"]), relerr(gn[f, 2 * n:], r["dbn"])
            q, m[f], v[f] = update(f, it, mu, dict(dmu=gn[f, :n], dbn=gn[f, 2 * n:]), lr[f], WDS[f])      # O.adamw on the gradient just compared
            d = np.abs(pn[f] - q)
            print("%s/%s fit %d it %d: loss %.6f / %.6f, dmu %.2e dbn %.2e, update max %.2e" % (method, task, f, it, losses[f], r["loss"], eg, eb, d.max()))
            assert abs(losses[f] - r["loss"]) < lb * abs(r["loss"]), (f, it, losses[f], r["loss"])
            assert eg < gb and eb < gb, (f, it, eg, eb)
            assert d.max() < 2e-6, (f, it, d.max())
            assert np.abs(host(sb.m)[f] - m[f]).max() < 2e-6 and np.abs(host(sb.v)[f] - v[f]).max() < 2e-6
            assert np.all(pn[f, n:2 * n] == 0.0) and np.all(gn[f, n:2 * n] == 0.0)
            if method == "sgld" and lr[f] > 1e-8:
                lr[f] *= GAMMAS[f]
        p = pn.copy()                                  # re-anchor: Adam amplifies rounding noise of near-zero gradients
        m, v = host(sb.m).copy(), host(sb.v).copy()
    assert not sb.dead.any()
    assert np.array_equal(sb.lrs(), np.asarray(lr, np.float64))


# ---- 4. fit 0 is the standalone engine ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["dip", "mcd", "sgld"])
def test_fit0_is_the_standalone_sibling_engine(M, method):
    H = W = 32; seed = 9
    sb = _batch(M, method, "den", seed=seed)
    eng = M.engine.SiblingEngine(H, W, method=method, task="den", K=sb.K, input_depth=8, lr=LRS[0], weight_decay=WDS[0], dropout_p=PS[0], gamma=GAMMAS[0],
                                 seed=seed, net_kwargs=SMALL, autotune=False)
    assert torch.equal(sb.fit(0)["params"], eng.params) and torch.equal(sb.z0[0], eng.z0)          # bit-equal initial values and input
    write_bn(sb, seed); eng.bn.copy_(sb.fit(0)["bn"])
    tg = _targets("den", 3, seed)
    sb.set_targets(torch.from_numpy(tg)); eng.set_target(torch.from_numpy(tg[0]))
    if method == "sgld":
        sb.add_noise(0); eng.add_noise(0)
        assert torch.equal(sb.fit(0)["mu"], eng.mu)
        assert not torch.equal(sb.fit(1)["mu"] - sb.fit(0)["mu"], torch.zeros_like(eng.mu))
    sb.grad_only(0); eng.grad_only(0, with_kl=False)
    assert torch.equal(sb.z[0], eng.z)
    g, ge = host(sb.fit(0)["grads"]), host(eng.grads[:eng.n_params])
    nv = sb.n_vi
    for name, sl in (("dmu", slice(0, nv)), ("dbn", slice(2 * nv, None))):
        e = relerr(g[sl], ge[sl])
        print("%s %s %.2e" % (method, name, e))
        assert e < 2e-4, (name, e)
    a, b = float(sb.loss_acc[0]), float(eng.acc[0])
    assert abs(a - b) < 1e-5 * abs(b), (a, b)
    sb.init_params(); eng.init_params(); eng.lr = eng.lr0
    for _ in range(5):
        sb.step(); eng.step()
    assert np.float32(sb.lrs()[0]) == np.float32(eng.lr)
    assert (method == "sgld") == (sb.lrs()[0] != LRS[0])


# ---- 5. kernel level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,factor", [(7, 9, 1), (8, 12, 4), (8, 8, 1)])
def test_mse_channel_fits_against_single_fit(M, H, W, factor):
    lib, sp, p_ = M._lib.lib(), M._lib.stream_ptr(), M._lib.ptr
    F, S, Cc, seed = 3, 2, 2, 17
    h, w = H // factor, W // factor
    out = dev((0.5 * O.normal_fill(seed, 2, 0, 0, 0, F * S * Cc * H * W)).reshape(F * S, Cc, H, W).astype(np.float32))
    tg = dev(O.uniform_fill(seed, 1, 0, 0, F * h * w).reshape(F, h, w).astype(np.float32))
    for ch in range(Cc):
        dout = torch.full_like(out, 7.0); acc = torch.zeros(F, dtype=torch.float64, device="cuda")
        M._lib.check(lib.mfvi_mse_channel_fits(p_(out), p_(tg), h * w, F, S, Cc, H, W, ch, factor, 0.5, p_(dout), p_(acc), sp))
        for f in range(F):
            d1 = torch.full((S, Cc, H, W), 7.0, device="cuda"); a1 = torch.zeros(1, dtype=torch.float64, device="cuda")
            M._lib.check(lib.mfvi_mse_channel(p_(out[f * S:]), p_(tg[f]), S, Cc, H, W, ch, factor, 0.5, p_(d1), p_(a1), sp))
            assert abs(float(acc[f]) - float(a1[0])) < 2e-6 * abs(float(a1[0])), (ch, f)
            assert relerr(host(dout[f * S:(f + 1) * S]), host(d1)) < 2e-6, (ch, f)
        first = host(acc).copy()
        # accumulates (+=), dout = NULL; two calls are bit-identical
        M._lib.check(lib.mfvi_mse_channel_fits(p_(out), p_(tg), h * w, F, S, Cc, H, W, ch, factor, 0.5, None, p_(acc), sp))
        assert np.array_equal(host(acc), first + first)
    rc = lib.mfvi_mse_channel_fits(p_(out), p_(tg), h * w - 1, F, S, Cc, H, W, 0, factor, 0.5, None, p_(acc), sp)
    assert rc == -1 and b"mse_channel_fits" in lib.mfvi_last_error()


def _hyper(M, lrs, gammas, wds, floor=1e-8):
    dt = np.dtype([("lr", "<f8"), ("gamma", "<f8"), ("weight_decay", "<f4"), ("lr_floor", "<f4")])
    h = np.zeros(len(lrs), dt)
    h["lr"], h["gamma"], h["weight_decay"], h["lr_floor"] = lrs, gammas, wds, floor
    return dev(h.view(np.uint8)), dt


def test_sibling_update_fits_against_adamw_step(M):
    lib, sp, p_ = M._lib.lib(), M._lib.stream_ptr(), M._lib.ptr
    F, nv, nb, seed, t = 3, 1003, 37, 23, 4
    n = 2 * nv + nb
    stride, gstride = n + 5, n + 2
    lrs, wds = [1e-3, 2e-3, 3e-3], [0.0, 0.05, 0.5]

    def rows(s, sc, width):
        r = np.zeros((F, width), np.float32)
        r[:, :] = (sc * O.normal_fill(seed, 2, s, 0, 0, F * width)).reshape(F, width)      # the gaps and the RHO block hold values too
        return r
    p0, g0, m0 = rows(0, 0.1, stride), rows(1, 1e-2, gstride), rows(2, 1e-3, stride)
    v0 = np.abs(rows(3, 1e-4, stride))
    loss = torch.tensor([0.3, 0.4, 0.5], dtype=torch.float64, device="cuda")
    runs = []
    for _ in range(2):
        hyper, dt = _hyper(M, lrs, [1.0] * F, wds)
        P, G, Mo, V = dev(p0), dev(g0), dev(m0), dev(v0)
        dead = torch.zeros(F, dtype=torch.int32, device="cuda")
        M._lib.check(lib.mfvi_sibling_update_fits(p_(P), p_(G), p_(Mo), p_(V), nv, nb, stride, gstride, F, p_(hyper), 0.9, 0.999, 1e-8, t, p_(loss), p_(dead), sp))
        runs.append([host(x) for x in (P, G, Mo, V, dead, hyper)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)                                        # two calls bit-identical
    P, G, Mo, V, dead, hy = runs[0]
    assert not dead.any() and np.array_equal(hy.view(dt)["lr"], np.asarray(lrs))      # gamma = 1: a constant rate
    assert np.array_equal(G, g0)
    for A, a0 in ((P, p0), (Mo, m0), (V, v0)):                             # the RHO block and the gaps: bit-untouched
        assert np.array_equal(A[:, nv:2 * nv], a0[:, nv:2 * nv]) and np.array_equal(A[:, n:], a0[:, n:])
    for f in range(F):
        for lo, hi in ((0, nv), (2 * nv, n)):
            p1, g1, m1, v1 = dev(p0[f, lo:hi]), dev(g0[f, lo:hi]), dev(m0[f, lo:hi]), dev(v0[f, lo:hi])
            M._lib.check(lib.mfvi_adamw_step(p_(p1), p_(g1), p_(m1), p_(v1), hi - lo, lrs[f], 0.9, 0.999, 1e-8, t, wds[f], sp))
            for name, a, b in (("params", P[f, lo:hi], p1), ("m", Mo[f, lo:hi], m1), ("v", V[f, lo:hi], v1)):
                assert _ulp_diff(a, host(b)) <= 1, (f, lo, name, _ulp_diff(a, host(b)))
    assert not np.array_equal(P[0, :nv], p0[0, :nv])


def test_sibling_update_fits_lr_decay(M):
    lib, sp, p_ = M._lib.lib(), M._lib.stream_ptr(), M._lib.ptr
    F, nv, nb = 3, 64, 8
    n = 2 * nv + nb
    hyper, dt = _hyper(M, [1.5e-8, 4e-3, 1e-3], [0.5, 0.9995, 0.5], [0.0, 0.0, 0.0])
    P = dev(0.1 * O.normal_fill(1, 2, 0, 0, 0, F * n).reshape(F, n)); G = dev(1e-2 * O.normal_fill(1, 2, 1, 0, 0, F * n).reshape(F, n))
    Mo, V = torch.zeros_like(P), torch.zeros_like(P)
    loss = torch.tensor([0.3, 0.4, float("nan")], dtype=torch.float64, device="cuda")
    dead = torch.zeros(F, dtype=torch.int32, device="cuda")
    p_before = host(P).copy()
    want1 = 4e-3
    for t in range(1, 7):
        M._lib.check(lib.mfvi_sibling_update_fits(p_(P), p_(G), p_(Mo), p_(V), nv, nb, n, n, F, p_(hyper), 0.9, 0.999, 1e-8, t, p_(loss), p_(dead), sp))
        want1 *= 0.9995
        lr = host(hyper).view(dt)["lr"]
        assert lr[0] == 1.5e-8 * 0.5                                       # decays once to 7.5e-9, below the floor, and stops
        assert lr[1] == want1                                              # the Python double product chain, exactly
        assert lr[2] == 1e-3                                               # a dead fit's lr does not move
    assert list(host(dead)) == [0, 0, 1]
    assert np.array_equal(host(P)[2], p_before[2]) and not np.array_equal(host(P)[1], p_before[1])
    assert float(Mo[2].abs().max()) == 0.0 and float(V[2].abs().max()) == 0.0


def test_add_normal_fits_bits(M):
    lib, sp, p_ = M._lib.lib(), M._lib.stream_ptr(), M._lib.ptr
    F, seed, step, fit0 = 3, 77, 6, 2
    offs, ns = [8, 1100], [1001, 36]                                        # not adjacent: [8, 1009) and [1100, 1136)
    stride = 1200
    x0 = (0.1 * O.normal_fill(seed, 2, 0, 0, 0, F * stride)).reshape(F, stride).astype(np.float32)
    std = np.asarray([6e-4, 2e-3, 4e-3], np.float32)
    d_off, d_n, d_std = dev(np.asarray(offs, np.int64)), dev(np.asarray(ns, np.int64)), dev(std)
    dead = torch.zeros(F, dtype=torch.int32, device="cuda")
    x = dev(x0)
    M._lib.check(lib.mfvi_add_normal_fits(p_(x), stride, F, fit0, p_(d_off), p_(d_n), 2, seed, step, p_(d_std), p_(dead), sp))
    xh = host(x)
    want = x0.copy()
    for f in range(F):
        for l, (o, n) in enumerate(zip(offs, ns)):
            e = O.normal_fill(seed, 4, l, fit0 + f, step, n)
            # one fused multiply-add: exact product and sum in float64, rounded once
            want[f, o:o + n] = (x0[f, o:o + n].astype(np.float64) + np.float64(std[f]) * e.astype(np.float64)).astype(np.float32)
    assert np.array_equal(xh, want)                                        # the listed ranges, and everything outside them bit-untouched
    # fit 0 with fit0 = 0 is mfvi_add_normal per layer; a dead fit is skipped
    x = dev(x0); dead[1] = 1
    M._lib.check(lib.mfvi_add_normal_fits(p_(x), stride, F, 0, p_(d_off), p_(d_n), 2, seed, step, p_(d_std), p_(dead), sp))
    one = dev(x0[0])
    for l, (o, n) in enumerate(zip(offs, ns)):
        M._lib.check(lib.mfvi_add_normal(p_(one[o:]), seed, l, step, n, float(std[0]), sp))
    assert torch.equal(x[0], one)
    assert np.array_equal(host(x[1]), x0[1]) and not np.array_equal(host(x[2]), x0[2])


# ---- 6. NaN isolation -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["mcd", "sgld"])
def test_nan_fit_is_isolated(M, method):
    F, seed = 3, 12
    tg = _targets("den", F, seed)
    bad = tg.copy(); bad[1, 5, 7] = np.nan
    sbs = []
    for t in (tg, bad):
        sb = _batch(M, method, "den", seed=seed)
        write_bn(sb, seed); sb.set_targets(torch.from_numpy(t)); sb.grad_only(0)
        sbs.append(sb)
    clean, sb = sbs
    for f in (0, 2):
        assert relerr(host(sb.fit(f)["grads"]), host(clean.fit(f)["grads"])) < 2e-4, f
    before = [host(x).copy() for x in (sb.params, sb.m, sb.v)]
    lr_before = sb.lrs()
    sb.step(); sb.step()
    assert list(sb.dead) == [0, 1, 0]
    after = [host(x) for x in (sb.params, sb.m, sb.v)]
    for a, b in zip(before, after):
        assert np.array_equal(a[1], b[1])                                  # the dead fit: parameters and moments bit-equal to before, no noise added
        for f in (0, 2):
            assert np.isfinite(b[f]).all()
    for f in (0, 2):
        assert not np.array_equal(before[0][f], after[0][f])
    assert sb.lrs()[1] == lr_before[1] == LRS[1]
    if method == "sgld":
        assert sb.lrs()[0] != lr_before[0]
    assert np.isnan(sb.losses()[1]) and np.isfinite(sb.losses()[[0, 2]]).all()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(M):
    lib = M._lib.lib()
    UNS = M._lib.ERR_FITS_UNSUPPORTED

    def plan(**kw):
        P, zin, zout, _ = M.skip_program(32, 32, 8, 2, **dict(SMALL, **kw))
        return P, P.compile(zin, zout, 4)

    P, pl = plan(lrt=True)
    assert lib.mfvi_plan_set_fits_points(pl.handle, 1) == UNS and "local-reparameterisation" in lib.mfvi_last_error().decode()
    with pytest.raises(NotImplementedError):
        pl.set_fits_points(True)
    P, pl = plan(); M._lib.check(lib.mfvi_plan_set_param_dtype(pl.handle, M._lib.PARAM_BF16))
    assert lib.mfvi_plan_set_fits_points(pl.handle, 1) == UNS and "bf16 parameter storage" in lib.mfvi_last_error().decode()
    P, pl = plan(drop_down=0.3, drop_up=0.3)
    for bad in ([0.1, 1.0], [0.1, -0.1], [float("nan"), 0.1]):
        with pytest.raises(M._lib.MfviError, match="outside"):
            pl.set_fit_dropout(bad)
    import ctypes as C
    one = (C.c_float * 1)(0.1)
    assert lib.mfvi_plan_set_fit_dropout(pl.handle, one, 0) == -1 and "n_fits = 0" in lib.mfvi_last_error().decode()
    n = 2 * P.n_vi + P.n_bn
    stride = (n + 3) // 4 * 4
    pl.set_fits(2, stride, stride); pl.set_fits_points(True)
    pl.set_fit_dropout([0.1, 0.2, 0.3])                                     # three fits; the pass below has two
    rows = torch.zeros((2, stride), device="cuda")
    z = torch.zeros((2, 8, 32, 32), device="cuda")
    with pytest.raises(M._lib.MfviError, match="3 probabilities, this pass has 2 fits"):
        pl.forward(rows[0, :P.n_vi], rows[0, P.n_vi:], rows[0, 2 * P.n_vi:], z, 1, 0, 0, 4, sample_weights=False)
    pl.set_fit_dropout(None); pl.set_fits_points(False)
    with pytest.raises(NotImplementedError, match="sample_weights = 0"):    # off again: today's refusal
        pl.forward(rows[0, :P.n_vi], rows[0, P.n_vi:], rows[0, 2 * P.n_vi:], z, 1, 0, 0, 4, sample_weights=False)
    for task in ("ct", "inp"):
        with pytest.raises(NotImplementedError):
            M.SiblingBatch(32, 32, 2, "dip", task=task)
    with pytest.raises(ValueError, match="method"):
        M.SiblingBatch(32, 32, 2, "mfvi")


# ---- 8. to_engine and the runner ------------------------------------------------------------------------------------------------------------
def test_to_engine_exports_any_fit(M):
    H = W = 32; F, seed = 3, 21
    sb = _batch(M, "mcd", "den", seed=seed)
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)])
    sb.set_targets(torch.from_numpy(np.stack([O.noisy(g, 0.1, seed) for g in gt]).astype(np.float32)))
    for _ in range(3):
        sb.step()
    snap = [host(x).copy() for x in (sb.params, sb.m, sb.v, sb.ema)]
    eng = sb.to_engine(2)
    assert np.array_equal(host(eng.params), snap[0][2]) and np.array_equal(host(eng.m), snap[1][2]) and np.array_equal(host(eng.v), snap[2][2])
    assert eng.t == sb.t == 3 and torch.equal(eng.z0, sb.z0[2]) and torch.equal(eng.target, sb.targets[2])
    assert (eng.lr, eng.lr0, eng.weight_decay, eng.method) == (sb.lrs()[2], LRS[2], WDS[2], "mcd")
    assert eng.prog.tensors[sb.names[0]["d1"]]["drop_p"] == PS[2]
    r = eng.predict(4, target=torch.from_numpy(gt[2]))
    for k in ("mean", "epi", "ale", "total"):
        assert tuple(r[k].shape[-2:]) == (H, W) and torch.isfinite(r[k]).all(), k
    eng.step()
    for a, b in zip(snap, (sb.params, sb.m, sb.v, sb.ema)):
        assert np.array_equal(a, host(b))                                  # the batch is untouched
    ps = sb.psnr(gt)
    assert ps.shape == (F,) and np.isfinite(ps).all()
    with pytest.raises(ValueError):
        sb.to_engine(3)


def test_runner_sibling_fits(M, tmp_path, capsys):
    cfg = dict(bo_params=dict(dropout_p=dict(candidates=[0.1, 0.3]), weight_decay=dict(candidates=[0.0, 1e-4])),
               run_params=dict(img="phantom", num_iter=20, lr=1e-3, seed=1, p_sigma=0.1, input_depth=8, show_every=5, plot=False, save=True,
                               net_kwargs=SMALL, save_path=str(tmp_path / "logs")))
    path = str(tmp_path / "cfg.json")
    json.dump(cfg, open(path, "w"))
    res = M.runner.main(["--task", "denoising", "--bayes", "mcd", "--config", path, "--imsize", "32", "--sibling-fits", "3"])
    assert [i for i, _, _ in res] == [0, 1, 2, 3] and all(np.isfinite(y) for _, _, y in res)           # the table has four rows
    assert [(j["dropout_p"], j["weight_decay"]) for _, j, _ in res] == [(0.1, 0.0), (0.1, 1e-4), (0.3, 0.0), (0.3, 1e-4)]
    assert "4 fits in 2 batches of up to 3" in capsys.readouterr().out
    sizes = []
    for d in sorted(os.listdir(str(tmp_path / "logs"))):
        z = np.load(os.path.join(str(tmp_path / "logs"), d, "batch.npz"))
        assert set(z.files) == {"method", "task", "lr", "weight_decay", "dropout_p", "gamma", "K", "seed", "num_iter", "iterations", "psnr_gt_sm", "loss",
                                "recon", "dead"}
        Fb = len(z["lr"]); sizes.append(Fb)
        assert str(z["method"]) == "mcd" and str(z["task"]) == "den"
        assert list(z["iterations"]) == [0, 5, 10, 15, 20]
        assert z["psnr_gt_sm"].shape == z["loss"].shape == (5, Fb) and z["recon"].shape == (Fb, 32, 32) and not z["dead"].any()
        assert z["dropout_p"].shape == z["weight_decay"].shape == z["gamma"].shape == (Fb,)
        assert np.isfinite(z["psnr_gt_sm"]).all() and z["recon"].min() >= 0.0 and z["recon"].max() <= 1.0
    assert sorted(sizes) == [1, 3]
