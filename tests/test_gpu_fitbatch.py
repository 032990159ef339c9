"""Batched independent fits: the plan's fits mode against single-fit passes of the same plan type, FitBatch against
the oracle per fit, fit 0 against the standalone engine, the four batched kernels against the single-fit entry points they generalise,
NaN isolation, what the mode refuses, to_engine, and the runner's --fits-per-launch.

Net A: the SMALL net of test_gpu_runner.py at 32x32, input depth 8.  Net B: nd = nu = (16, 32, 64), ns = (4, 4, 4) at 64x64, input depth
16 -- the smallest net whose layers reach every kernel family (36 -> 16 on a 64-wide map: bf16x6 forward, backward-weight and strip-resident
backward-data; 68 -> 32 on a 32-wide map: row-phase; 3x3 layers on 16- and 8-wide maps: one-stage; the 1x1 kernels).
Every parity test first writes distinct BatchNorm parameters per fit (gamma = 1 + 0.2 u, beta = 0.1 u): at initialisation all fits have
gamma = 1, beta = 0 and an indexing error would be invisible."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))
NET_B = dict(nd=(16, 32, 64), nu=(16, 32, 64), ns=(4, 4, 4))
X6, SM = 1 << 25, 1 | 1 << 26


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
    """gamma = 1 + 0.2 u, beta = 0.1 u, u ~ U[0,1) seeded per fit."""
    u = O.uniform_fill(seed, 7, f, 0, prog.n_bn).astype(np.float32)
    bn = np.zeros(prog.n_bn, np.float32)
    for b in prog.bns:
        o, c = b["off"], b["C"]
        bn[o:o + c] = 1.0 + 0.2 * u[o:o + c]
        bn[o + c:o + 2 * c] = 0.1 * u[o + c:o + 2 * c]
    return bn


def write_bn(fb, seed):
    for f in range(fb.F):
        fb.fit(f)["bn"].copy_(dev(bn_values(fb.prog, seed, f)))


def pin_net_b(M, plan):
    """The tilings the heuristic would not pick, as tests/test_gpu_bwd_x6.py sets them: bf16x6 forward and strip-resident backward-data on the
    36 -> 16 layer of the 64-wide map, the one-stage kernels on the 3x3 layers of the 16- / 8-wide maps and on a 1x1 layer."""
    lib, T, ops = M._lib.lib(), plan.prog.tensors, plan.prog.ops
    for i, o in enumerate(ops):
        if o["type"] != M._lib.OP_CONV:
            continue
        cin, cout, w = T[o["in0"]]["C"], T[o["out"]]["C"], T[o["out"]]["W"]
        if o["ksize"] == 3 and o["stride"] == 1 and (cin, cout, w) == (36, 16, 64):
            M._lib.check(lib.mfvi_plan_set_tune(plan.handle, i, 0, 1 | 8 << 8 | 1 << 16 | X6))
            M._lib.check(lib.mfvi_plan_set_tune(plan.handle, i, 1, 2 | 8 << 8 | 1 << 16 | X6))
        if o["ksize"] == 3 and o["stride"] == 1 and w in (8, 16) and T[o["in0"]]["W"] == w and cin <= 144:
            M._lib.check(lib.mfvi_plan_set_tune(plan.handle, i, 0, SM))
            M._lib.check(lib.mfvi_plan_set_tune(plan.handle, i, 1, SM))
        if o["ksize"] == 1 and (cin, cout, w) == (64, 64, 16):
            M._lib.check(lib.mfvi_plan_set_tune(plan.handle, i, 0, SM))


def families(M, plan):
    lib = M._lib.lib()
    return {lib.mfvi_plan_last_kernel(plan.handle, i, w) for i, o in enumerate(plan.prog.ops) if o["type"] == M._lib.OP_CONV for w in range(3)}


# ---- 1. plan parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,S", [(4, 1), (3, 2)])
def test_plan_fits_mode_matches_single_fit_passes(M, F, S):
    """One forward + backward in fits mode against F calls of the same plan type in single-fit mode with fit f's parameters and input,
    k0 = f S, n = S, the same tilings.  Bounds: the project's for 'same arithmetic, only the fp64 BN atomics reorder'
    (tests/test_gpu_fullsize.py): outputs 1e-5, gradients 2e-4 relative to the largest reference value."""
    H = W = 64; seed, step = 31, 5
    P, zin, zout, _ = M.skip_program(H, W, 16, 2, **NET_B)
    n, nv, nb = F * S, P.n_vi, P.n_bn
    n_params = 2 * nv + nb
    stride = (n_params + 3) // 4 * 4 + 8                                  # rows further apart than they are long
    rows = np.zeros((F, stride), np.float32)
    for f in range(F):
        rows[f, :nv] = 0.1 * O.normal_fill(seed, 2, 0, f, 0, nv)
        rows[f, nv:2 * nv] = -3.0 + 0.1 * O.normal_fill(seed, 2, 1, f, 0, nv)
        rows[f, 2 * nv:n_params] = bn_values(P, seed, f)
    z = np.stack([0.1 * O.uniform_fill(seed, 0, f, 0, 16 * H * W).reshape(16, H, W) for f in range(F)]).astype(np.float32)
    dout = (O.normal_fill(seed, 2, 3, 0, 0, n * 2 * H * W).reshape(n, 2, H, W) / (H * W)).astype(np.float32)
    d_rows, d_z, d_dout = dev(rows), dev(z), dev(dout)
    pf = P.compile(zin, zout, n); pin_net_b(M, pf); pf.set_fits(S, stride, stride)
    g = torch.zeros((F, stride), device="cuda")
    out = pf.forward(d_rows[0, :nv], d_rows[0, nv:], d_rows[0, 2 * nv:], d_z, seed, step, 0, n)
    pf.backward(d_rows[0, :nv], d_rows[0, nv:], d_rows[0, 2 * nv:], d_z, seed, step, 0, n, d_dout, g[0, :nv], g[0, nv:], g[0, 2 * nv:])
    fam = families(M, pf)
    assert {2, 3, 4} <= fam, "row-phase, bf16x6 and one-stage kernels must each serve an op of the fits-mode pass: %s" % (fam,)
    out, g = host(out), host(g)
    assert np.all(g[:, n_params:] == 0.0)                                  # nothing is written between the rows
    ps = P.compile(zin, zout, S); pin_net_b(M, ps)
    for f in range(F):
        r = d_rows[f]
        gs = torch.zeros(n_params, device="cuda")
        o = ps.forward(r[:nv], r[nv:2 * nv], r[2 * nv:n_params], d_z[f], seed, step, f * S, S)
        ps.backward(r[:nv], r[nv:2 * nv], r[2 * nv:n_params], d_z[f], seed, step, f * S, S, d_dout[f * S:(f + 1) * S].contiguous(), gs[:nv], gs[nv:2 * nv], gs[2 * nv:])
        o, gs = host(o), host(gs)
        e = relerr(out[f * S:(f + 1) * S], o)
        print("F=%d S=%d fit %d: out %.2e" % (F, S, f, e))
        assert e < 1e-5, (f, e)
        for name, a, b in (("dmu", g[f, :nv], gs[:nv]), ("drho", g[f, nv:2 * nv], gs[nv:2 * nv]), ("dbn", g[f, 2 * nv:n_params], gs[2 * nv:])):
            e = relerr(a, b)
            print("    %s %.2e" % (name, e))
            assert e < 2e-4, (f, name, e)


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------------------------
def _hyper(F):
    return [1e-6 * 2 ** f for f in range(F)], [0.05 * 2 ** f for f in range(F)], [1e-3 * (f + 1) for f in range(F)]


@pytest.mark.parametrize("task", ["den", "sr"])
def test_batch_steps_match_oracle_per_fit(M, task):
    """Three iterations of F = 3 fits with K = 2, every fit with its own temp, sigma, lr, target, BN parameters: each fit against the oracle
    under the bounds of test_engine_steps_match_oracle (loss 2e-4 relative, parameters max 2.5e-3 (it + 1), mean 5e-5 (it + 1), re-anchored
    after every step)."""
    H = W = 32; F, K, seed = 3, 2, 4
    temps, sigmas, lrs = _hyper(F)
    fb = M.FitBatch(H, W, F, task=task, K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
    onet = O.make_net(H, W, input_depth=8, n_out=2, **SMALL)
    tid = {"den": 0, "sr": 1}[task]
    tg = []
    for f in range(F):
        img = O.phantom(H, W, seed + f)
        tg.append(O.noisy(img, 0.1, seed + f) if task == "den" else np.ascontiguousarray(img[::4, ::4]))
    tg = np.stack(tg).astype(np.float32)
    fb.set_targets(torch.from_numpy(tg))
    n = fb.n_vi
    # initial values: samples f of the INIT and z0 streams (bit-equal eps; a + b eps is one fma on the device, two roundings in numpy)
    p0 = host(fb.params); z0 = host(fb.z0)
    for f in range(F):
        assert np.abs(p0[f, :n] - 0.1 * O.normal_fill(seed, 2, 0, f, 0, n)).max() < 1e-7
        assert np.abs(p0[f, n:2 * n] - (-3.0 + 0.1 * O.normal_fill(seed, 2, 1, f, 0, n))).max() < 5e-7
        assert np.abs(z0[f].ravel() - 0.1 * O.uniform_fill(seed, 0, f, 0, z0[f].size)).max() < 1e-8
    assert not np.array_equal(p0[0], p0[1]) and not np.array_equal(z0[0], z0[1])
    write_bn(fb, seed)
    p = host(fb.params).copy()
    m = np.zeros_like(p); v = np.zeros_like(p)

    def oracle(f, it, bn_of=None, k_of=None, hyper_of=None):
        bf, kf, hf = (f if x is None else x for x in (bn_of, k_of, hyper_of))
        z = z0[f] + 0.1 * O.normal_fill(seed, 1, 0, f, it, z0[f].size).reshape(z0[f].shape)
        return O.elbo_grad(onet, p[f, :n], p[f, n:2 * n], p[bf, 2 * n:], z, tg[f], task=tid, factor=4, seed=seed, step=it, k0=kf * K, K=K, K_total=K,
                           temp=temps[hf], prior_sigma=fb.prior_sigma[hf])

    # the test's own discriminating power, on the CPU: the oracle given ANOTHER fit's gamma / beta, eps indices or hyper-parameters must miss
    # the right answer by more than 100 x the bound it is compared under (loss: 2e-4 relative; a gradient: 2e-4 of its largest value)
    right = oracle(0, 0)
    for kind, wrong in (("bn", oracle(0, 0, bn_of=1)), ("eps", oracle(0, 0, k_of=1)), ("hyper", oracle(0, 0, hyper_of=1))):
        dl = abs(wrong["loss"] - right["loss"]) / abs(right["loss"])
        dg = relerr(wrong["dmu"], right["dmu"])
        print("%s: wrong %s moves the loss by %.2e, dmu by %.2e" % (task, kind, dl, dg))
        assert max(dl, dg) > 100 * 2e-4, (kind, dl, dg)
    for it in range(3):
        fb.step()
        nll, kl, loss = fb.losses()
        pn = host(fb.params)
        for f in range(F):
            r = oracle(f, it)
            assert abs(loss[f] - r["loss"]) < 2e-4 * max(abs(r["loss"]), 1e-3), (task, f, it, loss[f], r["loss"])
            O.adam(p[f], np.concatenate([r["dmu"], r["drho"], r["dbn"]]), m[f], v[f], lrs[f], it + 1)
            d = np.abs(pn[f] - p[f])
            print("%s fit %d it %d: loss %.6f / %.6f, params max %.2e mean %.2e" % (task, f, it, loss[f], r["loss"], d.max(), d.mean()))
            assert d.max() < 2.5e-3 * (it + 1) and d.mean() < 5e-5 * (it + 1), (task, f, it, d.max(), d.mean())
        p = pn.copy()                                  # re-anchor: Adam amplifies rounding noise of near-zero gradients
    assert not fb.dead.any()


# ---- 3. fit 0 is the standalone engine ------------------------------------------------------------------------------------------------------
def test_fit0_is_the_standalone_engine(M):
    H = W = 32; K, seed = 2, 9
    temps, sigmas, lrs = _hyper(3)
    fb = M.FitBatch(H, W, 3, task="den", K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
    eng = M.engine.ElboEngine(H, W, task="den", K=K, input_depth=8, temp=temps[0], sigma=sigmas[0], lr=lrs[0], seed=seed, net_kwargs=SMALL, autotune=False)
    assert torch.equal(fb.fit(0)["params"], eng.params) and torch.equal(fb.z0[0], eng.z0)          # bit-equal initial values and input
    assert fb.prior_sigma[0] == eng.prior_sigma
    write_bn(fb, seed); eng.bn.copy_(fb.fit(0)["bn"])
    tg = np.stack([O.noisy(O.phantom(H, W, seed + f), 0.1, seed + f) for f in range(3)]).astype(np.float32)
    fb.set_targets(torch.from_numpy(tg)); eng.set_target(torch.from_numpy(tg[0]))
    fb.grad_only(0); eng.grad_only(0, with_kl=False)
    assert torch.equal(fb.z[0], eng.z)
    g, ge = host(fb.fit(0)["grads"]), host(eng.grads[:eng.n_params])
    nv = fb.n_vi
    for name, sl in (("dmu", slice(0, nv)), ("drho", slice(nv, 2 * nv)), ("dbn", slice(2 * nv, None))):
        e = relerr(g[sl], ge[sl])
        print("%s %.2e" % (name, e))
        assert e < 2e-4, (name, e)
    a, b = float(fb.nll_acc[0]), float(eng.acc[0])
    assert abs(a - b) < 1e-5 * abs(b), (a, b)


# ---- 4. kernel level ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,factor", [(7, 9, 1), (8, 12, 4), (8, 8, 1)])
def test_gaussian_nll_fits_against_single_fit(M, H, W, factor):
    """Odd F; factor 1 and 4; H W (and the target size) not a multiple of 4; the float4 path (8 x 8).  2e-6: the project's single-kernel bound."""
    lib, sp = M._lib.lib(), M._lib.stream_ptr()
    F, S, seed = 3, 2, 17
    h, w = H // factor, W // factor
    out = dev((0.5 * O.normal_fill(seed, 2, 0, 0, 0, F * S * 2 * H * W)).reshape(F * S, 2, H, W).astype(np.float32))
    tg = dev(O.uniform_fill(seed, 1, 0, 0, F * h * w).reshape(F, h, w).astype(np.float32))
    dout = torch.full_like(out, 7.0); nll = torch.zeros(F, dtype=torch.float64, device="cuda")
    M._lib.check(lib.mfvi_gaussian_nll_fits(M._lib.ptr(out), M._lib.ptr(tg), h * w, F, S, H, W, factor, 0.5, M._lib.ptr(dout), M._lib.ptr(nll), sp))
    for f in range(F):
        d1 = torch.full((S, 2, H, W), 7.0, device="cuda"); n1 = torch.zeros(1, dtype=torch.float64, device="cuda")
        M._lib.check(lib.mfvi_gaussian_nll(M._lib.ptr(out[f * S:]), M._lib.ptr(tg[f]), S, H, W, factor, 0.5, M._lib.ptr(d1), M._lib.ptr(n1), sp))
        assert abs(float(nll[f]) - float(n1[0])) < 2e-6 * abs(float(n1[0])), f
        assert relerr(host(dout[f * S:(f + 1) * S]), host(d1)) < 2e-6, f
    first = host(nll).copy()
    # accumulates (+=), like the single-fit entry point
    M._lib.check(lib.mfvi_gaussian_nll_fits(M._lib.ptr(out), M._lib.ptr(tg), h * w, F, S, H, W, factor, 0.5, None, M._lib.ptr(nll), sp))
    assert np.allclose(host(nll), 2 * first, rtol=1e-12, atol=0)
    rc = lib.mfvi_gaussian_nll_fits(M._lib.ptr(out), M._lib.ptr(tg), h * w - 1, F, S, H, W, factor, 0.5, None, M._lib.ptr(nll), sp)
    assert rc == -1 and b"gaussian_nll_fits" in lib.mfvi_last_error()


def _ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64); b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a); b = np.where(b < 0, -(b & 0x7fffffff), b)
    return int(np.abs(a - b).max())


def test_elbo_update_fits_against_single_fit(M):
    lib, sp, p_ = M._lib.lib(), M._lib.stream_ptr(), M._lib.ptr
    F, nv, nb, seed, t = 3, 1003, 37, 23, 4                                # n_vi, n_bn not multiples of the block or of 4
    n = 2 * nv + nb
    stride, gstride = n + 5, n + 2
    temps, sigmas, lrs = _hyper(F)
    ps = [float(np.float32(np.sqrt(a) * b + 1e-6)) for a, b in zip(temps, sigmas)]

    def rows(s, lo, sc, width):
        r = np.zeros((F, width), np.float32)
        r[:, :n] = (lo + sc * O.normal_fill(seed, 2, s, 0, 0, F * n)).reshape(F, n)
        return r
    p0 = rows(0, 0.0, 0.1, stride); p0[:, nv:2 * nv] -= 3.0
    g0, m0 = rows(1, 0.0, 1e-2, gstride), rows(2, 0.0, 1e-3, stride)
    v0 = np.abs(rows(3, 0.0, 1e-4, stride))
    hyper = dev(np.array([[0.0, ps[f], temps[f], lrs[f]] for f in range(F)], np.float32))
    nll = torch.tensor([0.3, 0.4, 0.5], dtype=torch.float64, device="cuda")
    scratch = torch.zeros(lib.mfvi_elbo_update_fits_scratch_bytes(F), dtype=torch.uint8, device="cuda")
    assert lib.mfvi_elbo_update_fits_scratch_bytes(0) == -1
    runs = []
    for _ in range(2):
        P, G, Mo, V = dev(p0), dev(g0), dev(m0), dev(v0)
        kl = torch.zeros(F, dtype=torch.float64, device="cuda"); dead = torch.zeros(F, dtype=torch.int32, device="cuda")
        M._lib.check(lib.mfvi_elbo_update_fits(p_(P), p_(G), p_(Mo), p_(V), nv, nb, stride, gstride, F, p_(hyper), 0.9, 0.999, 1e-8, t, p_(nll), p_(dead),
                                               p_(kl), p_(scratch), sp))
        runs.append([host(x) for x in (P, G, Mo, V, kl, dead)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)                                        # two calls bit-identical
    P, G, Mo, V, kl, dead = runs[0]
    assert not dead.any()
    assert np.array_equal(P[:, n:], p0[:, n:]) and np.array_equal(G[:, n:], g0[:, n:])      # nothing written between the rows
    s1 = torch.zeros(lib.mfvi_elbo_update_scratch_bytes(), dtype=torch.uint8, device="cuda")
    for f in range(F):
        p1, g1, m1, v1 = dev(p0[f, :n]), dev(g0[f, :n]), dev(m0[f, :n]), dev(v0[f, :n])
        k1 = torch.zeros(1, dtype=torch.float64, device="cuda")
        M._lib.check(lib.mfvi_elbo_update(p_(p1), p_(g1), p_(m1), p_(v1), nv, nb, 0.0, ps[f], temps[f], lrs[f], 0.9, 0.999, 1e-8, t, p_(k1), p_(s1), sp))
        for name, a, b in (("params", P[f, :n], p1), ("m", Mo[f, :n], m1), ("v", V[f, :n], v1), ("grads", G[f, :n], g1)):
            assert _ulp_diff(a, host(b)) <= 1, (f, name)
        assert abs(kl[f] - float(k1[0])) <= 1e-12 * abs(float(k1[0])), (f, kl[f], float(k1[0]))
    assert not np.array_equal(P[0, :n], p0[0, :n])


def test_perturb_input_fits_bits(M):
    lib, sp, p_ = M._lib.lib(), M._lib.stream_ptr(), M._lib.ptr
    F, npf, seed, step, fit0, std = 3, 8 * 11 * 13 + 3, 77, 6, 2, 0.1     # a size that is not a multiple of the Philox block
    z0 = dev(0.1 * O.uniform_fill(seed, 0, 0, 0, F * npf).reshape(F, npf).astype(np.float32))
    z = torch.zeros_like(z0)
    M._lib.check(lib.mfvi_perturb_input_fits(p_(z0), seed, step, npf, F, fit0, std, p_(z), sp))
    zh, z0h = host(z), host(z0)
    for f in range(F):
        e = torch.zeros(npf, device="cuda")
        M._lib.check(lib.mfvi_normal_fill(seed, 1, 0, fit0 + f, step, npf, 0.0, 1.0, p_(e), sp))        # the N(0,1) of sample fit0 + f
        # z0 + std * N as mfvi_perturb_input forms it: one fused multiply-add (exact product and sum in float64, rounded once)
        want = (z0h[f].astype(np.float64) + np.float64(np.float32(std)) * host(e).astype(np.float64)).astype(np.float32)
        assert np.array_equal(zh[f], want), f
    # fit 0 of a batch that starts at sample 0 IS mfvi_perturb_input
    M._lib.check(lib.mfvi_perturb_input_fits(p_(z0), seed, step, npf, F, 0, std, p_(z), sp))
    one = torch.zeros(npf, device="cuda")
    M._lib.check(lib.mfvi_perturb_input(p_(z0), seed, step, npf, std, p_(one), sp))
    assert torch.equal(z[0], one)


def test_ema_fits_against_float64_restatement(M):
    lib, sp, p_ = M._lib.lib(), M._lib.stream_ptr(), M._lib.ptr
    F, S, H, W, seed, w = 3, 2, 7, 9, 5, 0.99
    ema = torch.full((F, 2, H, W), 123.0, device="cuda")                  # the first update copies
    ref = None
    for it in range(3):
        o = (0.5 * O.normal_fill(seed, 2, 0, 0, it, F * S * 2 * H * W)).reshape(F, S, 2, H, W).astype(np.float32)
        M._lib.check(lib.mfvi_ema_fits(p_(dev(o.reshape(F * S, 2, H, W))), F, S, 2, H, W, p_(ema), w, int(it == 0), sp))
        o64 = o.astype(np.float64)
        cur = np.stack([o64[:, :, 0].mean(axis=1), np.exp(-o64[:, :, 1]).mean(axis=1)], axis=1)
        ref = cur if it == 0 else ref * np.float64(np.float32(w)) + cur * (1.0 - np.float64(np.float32(w)))
        assert relerr(host(ema), ref) < 2e-6, it
    # one fit of the batch is the EMA part of mfvi_bookkeep
    e1 = torch.zeros((2, H, W), device="cuda"); scratch = [torch.zeros((H, W), device="cuda") for _ in range(3)]
    M._lib.check(lib.mfvi_bookkeep(p_(dev(o[1])), S, 2, H, W, p_(e1), w, 1, p_(scratch[0]), p_(scratch[1]), p_(scratch[2]), None, None, sp))
    e2 = torch.zeros((F, 2, H, W), device="cuda")
    M._lib.check(lib.mfvi_ema_fits(p_(dev(o.reshape(F * S, 2, H, W))), F, S, 2, H, W, p_(e2), w, 1, sp))
    assert torch.equal(e2[1], e1)


# ---- 5. isolation and refusals -------------------------------------------------------------------------------------------------------------
def test_nan_fit_is_isolated(M):
    H = W = 32; F, K, seed = 3, 2, 12
    temps, sigmas, lrs = _hyper(F)
    tg = np.stack([O.noisy(O.phantom(H, W, seed + f), 0.1, seed + f) for f in range(F)]).astype(np.float32)
    bad = tg.copy(); bad[1, 5, 7] = np.nan
    fbs = []
    for t in (tg, bad):
        fb = M.FitBatch(H, W, F, task="den", K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
        write_bn(fb, seed); fb.set_targets(torch.from_numpy(t)); fb.grad_only(0)
        fbs.append(fb)
    clean, fb = fbs
    for f in (0, 2):
        assert relerr(host(fb.fit(f)["grads"]), host(clean.fit(f)["grads"])) < 2e-4, f
    before = [host(x).copy() for x in (fb.params, fb.m, fb.v)]
    fb.step(); fb.step()
    assert list(fb.dead) == [0, 1, 0]
    after = [host(x) for x in (fb.params, fb.m, fb.v)]
    for a, b in zip(before, after):
        assert np.array_equal(a[1], b[1])                                  # the dead fit: parameters and moments bit-equal to before
        for f in (0, 2):
            assert np.isfinite(b[f]).all()
    for f in (0, 2):
        assert not np.array_equal(before[0][f], after[0][f])
    assert np.isnan(fb.losses()[0][1]) and np.isfinite(fb.losses()[2][[0, 2]]).all()


def test_fits_mode_refusals(M):
    """Argument checks that return before any launch: a negative status and a message each, NotImplementedError from Python."""
    lib = M._lib.lib()
    UNS = M._lib.ERR_FITS_UNSUPPORTED

    def plan(depth=8, **kw):
        P, zin, zout, _ = M.skip_program(32, 32, depth, 2, **dict(SMALL, **kw))
        return P, P.compile(zin, zout, 4)

    def refused(pl, what):
        rc = lib.mfvi_plan_set_fits(pl.handle, 1, 4 * ((2 * pl.prog.n_vi + pl.prog.n_bn + 3) // 4), 2 * pl.prog.n_vi + pl.prog.n_bn)
        msg = lib.mfvi_last_error().decode()
        assert rc == UNS and what in msg, (rc, msg)
        with pytest.raises(NotImplementedError, match="fits mode"):
            pl.set_fits(1, 4 * ((2 * pl.prog.n_vi + pl.prog.n_bn + 3) // 4), 2 * pl.prog.n_vi + pl.prog.n_bn)

    P, pl = plan(); M._lib.check(lib.mfvi_plan_set_param_dtype(pl.handle, M._lib.PARAM_BF16)); refused(pl, "bf16 parameter storage")
    P, pl = plan(lrt=True); refused(pl, "local-reparameterisation")
    P, pl = plan(); running = torch.ones(P.n_bn, device="cuda"); M._lib.check(lib.mfvi_plan_set_bn_eval(pl.handle, M._lib.ptr(running))); refused(pl, "BatchNorm eval mode")
    P, pl = plan(); op, _ = pl.choose_grad_split(0.5); pl.grad_split(op, torch.cuda.Stream()); refused(pl, "gradient split")
    P, pl = plan(); cnt = torch.zeros(1, dtype=torch.int32, device="cuda"); M._lib.check(lib.mfvi_plan_set_step_source(pl.handle, M._lib.ptr(cnt))); refused(pl, "device step source")
    P, pl = plan(depth=6); refused(pl, "outside the sampling table")
    # switched on, then asked for what it does not serve: the pass refuses
    P, pl = plan()
    n = 2 * P.n_vi + P.n_bn
    stride = (n + 3) // 4 * 4
    assert lib.mfvi_plan_set_fits(pl.handle, 1, -4, stride) == -1 and "negative stride" in lib.mfvi_last_error().decode()
    assert lib.mfvi_plan_set_fits(pl.handle, 5, stride, stride) == -1
    pl.set_fits(2, stride, stride)
    rows = torch.zeros((2, stride), device="cuda"); rows[:, P.n_vi:2 * P.n_vi] = -3.0
    z = torch.zeros((2, 8, 32, 32), device="cuda")
    with pytest.raises(NotImplementedError, match="sample_weights = 0"):
        pl.forward(rows[0, :P.n_vi], rows[0, P.n_vi:], rows[0, 2 * P.n_vi:], z, 1, 0, 0, 4, sample_weights=False)
    with pytest.raises(M._lib.MfviError, match="multiple of the 2 samples per fit"):
        pl.forward(rows[0, :P.n_vi], rows[0, P.n_vi:], rows[0, 2 * P.n_vi:], z[:1], 1, 0, 0, 3)
    M._lib.check(lib.mfvi_plan_set_bn_eval(pl.handle, M._lib.ptr(torch.ones(P.n_bn, device="cuda"))))
    with pytest.raises(NotImplementedError, match="BatchNorm eval mode"):
        pl.forward(rows[0, :P.n_vi], rows[0, P.n_vi:], rows[0, 2 * P.n_vi:], z, 1, 0, 0, 4)
    M._lib.check(lib.mfvi_plan_set_bn_eval(pl.handle, None))
    with pytest.raises(NotImplementedError, match="autotune"):
        pl.autotune(rows[0, :P.n_vi], rows[0, P.n_vi:], rows[0, 2 * P.n_vi:], z[0], 4)
    pl.set_fits(0)                                                          # off again: the single-fit path as before
    out = pl.forward(rows[0, :P.n_vi], rows[0, P.n_vi:2 * P.n_vi], rows[0, 2 * P.n_vi:n], z[0], 1, 0, 0, 4)
    assert torch.isfinite(out).all()


# ---- 6. to_engine ---------------------------------------------------------------------------------------------------------------------------
def test_to_engine_exports_any_fit(M):
    H = W = 32; F, K, seed = 3, 1, 21
    temps, sigmas, lrs = _hyper(F)
    fb = M.FitBatch(H, W, F, task="den", K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)])
    fb.set_targets(torch.from_numpy(np.stack([O.noisy(g, 0.1, seed) for g in gt]).astype(np.float32)))
    for _ in range(3):
        fb.step()
    snap = [host(x).copy() for x in (fb.params, fb.m, fb.v, fb.ema)]
    eng = fb.to_engine(2)
    assert np.array_equal(host(eng.params), snap[0][2]) and np.array_equal(host(eng.m), snap[1][2]) and np.array_equal(host(eng.v), snap[2][2])
    assert eng.t == fb.t == 3 and int(eng.t_applied[0]) == 3 and torch.equal(eng.z0, fb.z0[2])
    assert (eng.temp, eng.lr, eng.prior_sigma) == (temps[2], lrs[2], fb.prior_sigma[2])
    r = eng.predict(4, target=torch.from_numpy(gt[2]))
    for k in ("mean", "epi", "ale", "total"):
        assert tuple(r[k].shape[-2:]) == (H, W) and torch.isfinite(r[k]).all(), k
    eng.step()                                                              # the exported fit runs on alone
    for a, b in zip(snap, (fb.params, fb.m, fb.v, fb.ema)):
        assert np.array_equal(a, host(b))                                  # the batch is untouched
    ps = fb.psnr(gt)
    assert ps.shape == (F,) and np.isfinite(ps).all()
    assert abs(ps[1] - O.psnr(gt[1], np.clip(snap[3][1, 0], 0, 1))) < 1e-3
    with pytest.raises(ValueError):
        fb.to_engine(3)


# ---- 7. runner ------------------------------------------------------------------------------------------------------------------------------
def test_runner_fits_per_launch(M, tmp_path, capsys):
    cfg = dict(bo_params=dict(temp=dict(candidates=[1e-6, 2e-6]), sigma=dict(candidates=[0.05, 0.1])),
               run_params=dict(img="phantom", num_iter=20, lr=1e-3, seed=1, p_sigma=0.1, input_depth=8, show_every=5, plot=False, save=True,
                               net_kwargs=SMALL, save_path=str(tmp_path / "logs")))
    path = str(tmp_path / "cfg.json")
    json.dump(cfg, open(path, "w"))
    res = M.runner.main(["--task", "denoising", "--config", path, "--imsize", "32", "--fits-per-launch", "3"])
    assert [i for i, _, _ in res] == [0, 1, 2, 3] and all(np.isfinite(y) for _, _, y in res)           # the table has four rows
    assert [(j["temp"], j["sigma"]) for _, j, _ in res] == [(1e-6, 0.05), (1e-6, 0.1), (2e-6, 0.05), (2e-6, 0.1)]
    text = capsys.readouterr().out
    assert "4 fits in 2 batches of up to 3" in text and text.count("e-0") >= 0
    dirs = sorted(os.listdir(str(tmp_path / "logs")))
    sizes = []
    for d in dirs:
        z = np.load(os.path.join(str(tmp_path / "logs"), d, "batch.npz"))
        assert set(z.files) == {"task", "temp", "sigma", "lr", "prior_sigma", "K", "seed", "num_iter", "iterations", "psnr_gt_sm", "nll", "kl", "recon", "dead"}
        Fb = len(z["temp"]); sizes.append(Fb)
        assert list(z["iterations"]) == [0, 5, 10, 15, 20]
        assert z["psnr_gt_sm"].shape == z["nll"].shape == z["kl"].shape == (5, Fb) and z["recon"].shape == (Fb, 32, 32) and not z["dead"].any()
        assert np.isfinite(z["psnr_gt_sm"]).all() and z["recon"].min() >= 0.0 and z["recon"].max() <= 1.0
    assert sorted(sizes) == [1, 3]                                          # a second batch of one fit is formed
