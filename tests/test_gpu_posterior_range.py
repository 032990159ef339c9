"""Parity of the reparameterised convolution path away from the initial posterior: rho where a fit ends (-13.8),
over the whole range softplus_fast / softplus_f / sigmoid_f see (-104 ... 50), and on pruned weights (rho = -200, mu = 0).

1. the draw weight by weight: a convolution of unit impulses returns the sampled weights, compared per element with mu + softplus64(rho) eps
   on every forward kernel family (tests/posterior_cases.py: layouts, bound, impulse plans; tests/test_posterior_cases_host.py checks them);
2. backward of a single convolution: y, dx, dmu at the tolerances of test_single_conv_fwd_bwd, drho through q = drho / sigmoid64(rho) per
   layer -- max |a - b| / max |b| over a tensor whose sigmoid(rho) spans decades sees the few largest entries only;
3. local-reparameterisation layers; 4. whole hour-glass nets at a fitted and a pruned posterior, also against the reference's own float64
   autograd (tests/golden/posterior_range.npz).
Run on an MI355X with `pytest -m gpu`."""
import os

import numpy as np
import pytest

from conftest import note_margin as _note

from oracle import oracle as O
import posterior_cases as PC
from test_gpu_parity import M, dev, host, relerr      # noqa: F401  (M is a fixture)
from test_gpu_fitbatch import pin_net_b

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, STEP, K0 = 4100, 5, 3
SEEN = {0: set(), 1: set(), 2: set()}          # pass -> kernel families observed by the tests of this file, in file order


def note_as(tag, value, what):
    """note_margin under '<test id>{tag}' (no blanks in tag): one line per rho band and draw in the margins file, not one per test."""
    cur = os.environ.get("PYTEST_CURRENT_TEST", "?")
    os.environ["PYTEST_CURRENT_TEST"] = cur.split(" ")[0] + "{" + tag + "}"
    try:
        _note(value, what)
    finally:
        os.environ["PYTEST_CURRENT_TEST"] = cur


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def conv_plan(M, shape, n, tunes=(0, 0, 0), lrt=False, param_dtype="f32"):
    cin, cout, k, stride, H, W = shape
    P = M.Program()
    zin = P.tensor(cin, H, W)
    out = P.tensor(cout, *P.conv_out_hw(zin, k, stride))
    P.conv(zin, out, k, stride, lrt=lrt)
    plan = P.compile(zin, out, max_samples=n, param_dtype=param_dtype)
    for which, t in enumerate(tunes):
        if t:
            M._lib.check(M._lib.lib().mfvi_plan_set_tune(plan.handle, 0, which, t))
    return P, plan


def family(M, plan, which, op=0):
    f = M._lib.lib().mfvi_plan_last_kernel(plan.handle, op, which)
    SEEN[which].add(f)
    return f


def params_dev(mu, rho, bf16):
    if bf16:
        return dev(mu).bfloat16(), dev(rho).bfloat16()
    return dev(mu), dev(rho)


# ---- 1. the draw, weight by weight ---------------------------------------------------------------------------------------------------------
def check_draw(got, mu, rho, eps, kind, exact_above_20):
    """got, mu, rho, eps: flat arrays of one sample.  The bound of posterior_cases.draw_bound per element, the exact statements, the margins."""
    got64 = got.astype(np.float64)
    assert np.isfinite(got64).all()
    err = np.abs(got64 - PC.w64(mu, rho, eps)); bound = PC.draw_bound(mu, rho, eps)
    band = PC.band_of(rho)
    live = PC.softplus64(rho) * np.abs(eps.astype(np.float64)) > 2.0 ** -100
    for b, (label, _, _) in enumerate(PC.BANDS):
        sel = (band == b) & live & (mu == 0)
        if sel.any():          # with mu = 0 the draw carries one rounding: (got - w64) / (softplus eps) is the device softplus' own error
            note_as("%s:%s" % (kind, label), float(np.max(err[sel] / (PC.softplus64(rho[sel]) * np.abs(eps[sel].astype(np.float64))))), "softplus rel err")
    bad = err > bound
    assert not bad.any(), "%s draw: %d elements beyond the bound, worst at rho = %r: |got - w64| = %.3e, bound %.3e" % (
        kind, bad.sum(), float(rho[np.argmax(err / bound)]), float(err[np.argmax(err / bound)]), float(bound[np.argmax(err / bound)]))
    low = rho < -87
    assert np.all((got64[low] - mu[low]) * eps[low] >= 0)                              # softplus is not negative
    pr = rho == np.float32(PC.PRUNED_RHO)
    assert np.array_equal(bits(got[pr]), bits(mu[pr])), "a pruned weight does not sample as mu"
    if exact_above_20:          # softplus(rho > 20) IS rho (torch's threshold): with mu = 0 the draw is the correctly rounded product
        hi = (rho > 20) & (mu == 0)
        assert np.array_equal(bits(got[hi]), bits((rho[hi].astype(np.float64) * eps[hi].astype(np.float64)).astype(np.float32)))


@pytest.mark.parametrize("lay", ["ladder", "broad", "pruned"])
@pytest.mark.parametrize("name,bf16", [(nm, False) for nm in PC.DRAW_CASES] + [(nm, True) for nm in PC.BF16_CASES])
def test_draw_weight_by_weight(M, name, bf16, lay):
    """Unit impulses in distinct input channels: y[co, y0 + p - ky, x0 + p - kx] is weight [co, ci, ky, kx] itself, every other product
    is with an exact 0 (on the bf16x6 kernels too: the three pieces of 1.0 are 1, 0, 0), the bias is pruned.  n = 2 samples, k0 = 3."""
    shape, tune = PC.DRAW_CASES[name]
    cin, cout, k, stride, H, W = shape
    n, nw = 2, cout * cin * k * k
    layers = PC.single_layer(cin, cout, k)
    P, plan = conv_plan(M, shape, n, (tune, 0, 0), param_dtype="bf16" if bf16 else "f32")
    passes = PC.impulse_plan(cin, k, stride, H, W)
    xs = [dev(p[0]) for p in passes]
    bn = torch.zeros(1, device="cuda")
    kind = "inkernel" if PC.FWD_FAMILY[name] == 0 else "slab"
    eps = [O.eps(SEED, STEP, K0 + i, 0, 0, nw) for i in range(n)]
    shifts = PC.ladder_shifts(nw) if lay in ("ladder", "broad") else [0]
    for shift in shifts:
        mu, rho = PC.layout(lay, nw + cout, SEED, shift=shift, layers=layers, dead=PC.dead_channels(layers) if lay == "pruned" else ())
        mu[nw:] = 0.0; rho[nw:] = PC.PRUNED_RHO
        if bf16:
            mu, rho = O.bf16_round(mu), O.bf16_round(rho)
        d_mu, d_rho = params_dev(mu, rho, bf16)
        outs = [host(plan.forward(d_mu, d_rho, bn, x, SEED, STEP, K0, n)) for x in xs]
        fam = family(M, plan, 0)
        for i in range(n):
            w, seen = PC.gather_weights(passes, [o[i] for o in outs], cin, cout, k)
            assert np.all(seen == 1)
            check_draw(w.ravel(), mu[:nw], rho[:nw], eps[i], kind, exact_above_20=True)
        if shift == 0:          # eval branch: w = mu, bit for bit
            outs = [host(plan.forward(d_mu, d_rho, bn, x, SEED, STEP, K0, 1, sample_weights=False)) for x in xs]
            w, _ = PC.gather_weights(passes, [o[0] for o in outs], cin, cout, k)
            assert np.array_equal(bits(w.ravel()), bits(mu[:nw]))
    print("%s %s bf16=%d: forward family %d, %d shifts x %d passes" % (name, lay, bf16, fam, len(shifts), len(passes)))
    assert fam == PC.FWD_FAMILY[name], "forward ran on family %d, not %d" % (fam, PC.FWD_FAMILY[name])


@pytest.mark.parametrize("lay", ["ladder", "broad", "pruned"])
@pytest.mark.parametrize("name", list(PC.DRAW_CASES))
def test_bias_draw(M, name, lay):
    """Zero input, every weight pruned: each output pixel of channel co is the sampled bias (softplus_f, the libm-grade one)."""
    shape, tune = PC.DRAW_CASES[name]
    cin, cout, k, stride, H, W = shape
    n, nw = 2, cout * cin * k * k
    P, plan = conv_plan(M, shape, n, (tune, 0, 0))
    x = torch.zeros((cin, H, W), device="cuda"); bn = torch.zeros(1, device="cuda")
    eps = [O.eps(SEED, STEP, K0 + i, 0, 1, cout) for i in range(n)]
    for shift in (range(0, PC.N_LADDER, cout) if lay == "ladder" else [0]):
        mu = np.zeros(nw + cout, np.float32); rho = np.full(nw + cout, PC.PRUNED_RHO, np.float32)
        if lay == "ladder":
            rho[nw:] = PC.LADDER[(np.arange(cout) + shift) % PC.N_LADDER]
        else:
            m_, r_ = PC.layout(lay, nw + cout, SEED)
            mu[nw:] = m_[nw:]; rho[nw:] = r_[nw:]
            if lay == "pruned":
                mu[nw] = 0.0; rho[nw] = PC.PRUNED_RHO
        y = host(plan.forward(dev(mu), dev(rho), bn, x, SEED, STEP, K0, n))
        assert np.array_equal(bits(y), bits(np.broadcast_to(y[:, :, :1, :1], y.shape))), "a pruned weight contributes to the output"
        for i in range(n):
            check_draw(y[i, :, 0, 0], mu[nw:], rho[nw:], eps[i], "bias", exact_above_20=True)
    y0 = host(plan.forward(dev(mu), dev(rho), bn, x, SEED, STEP, K0, 1, sample_weights=False))
    assert np.array_equal(bits(y0[0, :, 0, 0]), bits(mu[nw:]))
    family(M, plan, 0)


# ---- 2. backward of a single convolution ---------------------------------------------------------------------------------------------------
enc = lambda a, b, c: a | b << 8 | c << 16      # noqa: E731
# name -> (shape, (forward, backward-data, backward-weight tiling), the families the three passes must run on)
BWD_CASES = {
    "generic_5x3": ((5, 3, 3, 1, 33, 47), (0, 0, 0), (0, 0, 0)),
    "inkernel_16x16": ((16, 16, 3, 1, 16, 16), (PC.GENERIC, 0, PC.GENERIC), (0, 2, 0)),
    "mfma_s2": ((16, 16, 3, 2, 16, 16), (0, 0, 0), (1, 1, 1)),
    "mfma_5x5": ((8, 12, 5, 1, 12, 16), (0, 0, 0), (1, 1, 1)),
    "rowphase_16x16": ((16, 16, 3, 1, 16, 16), (0, 0, 0), (2, 2, 1)),
    # (the bf16x6 backward-data kernels run the fold of a BatchNorm'ed input in their epilogue: a layer fed by the plan's input stays on the
    # row-phase kernel; test_nets_at_a_fitted_and_a_pruned_posterior pins both of their forms inside the hour-glass)
    "x6_fwd_bww": ((36, 16, 3, 1, 64, 64), (PC.X6_FWD, 0, enc(1, 11, 1)), (3, 2, 3)),
    "rowphase_split": ((36, 16, 3, 1, 64, 64), (0, 0, enc(2, 10, 1)), (2, 2, 1)),
    "mfma_w4": ((36, 16, 3, 1, 64, 64), (enc(1, 8, 1), enc(1, 8, 1), enc(1, 4, 1)), (1, 1, 1)),
    "small_128": ((128, 128, 3, 1, 8, 8), (PC.SM, PC.SM, 0), (4, 4, 1)),
    "small_1x1": ((64, 64, 1, 1, 16, 16), (PC.SM, PC.SM, 0), (4, 4, 1)),
    "stream_1x1": ((16, 4, 1, 1, 8, 8), (PC.ST, 0, 0), (6, 1, 1)),
}
# fp32 flushes a sigmoid below 2^-126 (rho < -87.3) to zero or keeps a few bits of it: there drho = q sigmoid(rho) is held to an absolute
# 2^-125 per unit of q, not to a relative bound
TINY = 2.0 ** -125


def conv_reference(shape, mu, rho, x, dy, seed, step, k0, n):
    """O.conv_fwd / O.conv_bwd on the weights rounded from the float64 statement; gradients summed in float64.  -> y [n], dx [n], dmu, q."""
    cin, cout, k, stride, H, W = shape
    nw = cout * cin * k * k
    ys, dxs = [], []
    dmu = np.zeros(nw + cout); q = np.zeros(nw + cout)
    for i in range(n):
        ew = O.eps(seed, step, k0 + i, 0, 0, nw); eb = O.eps(seed, step, k0 + i, 0, 1, cout)
        w = PC.w64(mu[:nw], rho[:nw], ew).astype(np.float32).reshape(cout, cin, k, k); b = PC.w64(mu[nw:], rho[nw:], eb).astype(np.float32)
        ys.append(O.conv_fwd(x, w, b, stride))
        dx, dw, db = O.conv_bwd(x, w, stride, dy[i])
        dxs.append(dx)
        g = np.r_[dw.ravel(), db]
        dmu += g; q += g * np.r_[ew, eb].astype(np.float64)
    return ys, dxs, dmu, q


def check_drho(drho, q_ref, rho, layers, tol, what):
    """q per layer over rho >= -60; below: finite, drho = q sigmoid64(rho) to tol of the layer's scale plus the flush of a denormal sigmoid;
    exactly 0 on a pruned weight."""
    assert np.isfinite(drho).all(), what
    worst, rows = PC.layer_q_err(drho, q_ref, rho, layers)
    for i, tag, e, share in rows:
        note_as("q:%s" % tag, e, "q rel err")
        assert e < tol, (what, i, tag, e)
    assert min(PC.layer_shares(rho, layers)) >= 0.70, what
    low = rho < PC.RATIO_FLOOR
    sig = PC.sigmoid64(rho[low])
    top = max(np.abs(q_ref).max(), 1e-300)
    assert np.all(np.abs(drho[low].astype(np.float64) - q_ref[low] * sig) <= tol * top * sig + TINY * np.maximum(1.0, np.abs(q_ref[low]))), what
    assert np.all(drho[rho == np.float32(PC.PRUNED_RHO)] == 0.0), what
    return worst


def run_conv(plan, mu, rho, x, dy, seed, step, k0, n, bf16=False):
    d_mu, d_rho = params_dev(mu, rho, bf16)
    bn = torch.zeros(1, device="cuda")
    d_x = dev(x)
    y = plan.forward(d_mu, d_rho, bn, d_x, seed, step, k0, n)
    dmu = torch.zeros(mu.size, device="cuda"); drho = torch.zeros(mu.size, device="cuda"); dbn = torch.zeros(1, device="cuda")
    dz = torch.empty((n,) + x.shape, device="cuda")
    plan.backward(d_mu, d_rho, bn, d_x, seed, step, k0, n, dev(dy), dmu, drho, dbn, dz=dz)
    return host(y), host(dz), host(dmu), host(drho)


@pytest.mark.parametrize("name", list(BWD_CASES))
def test_single_conv_backward_wide_rho(M, name):
    """test_single_conv_fwd_bwd's inputs and tolerances for y (2e-6), dx (5e-6) and dmu (2e-5) at the fitted, broad and pruned layouts;
    q = drho / sigmoid64(rho) per layer at 2e-5; dmu bit-identical between two layouts that differ in rho only (dW does not depend on the
    weights) wherever backward-weight is deterministic (every family but the generic one, which accumulates with atomics)."""
    shape, tunes, want = BWD_CASES[name]
    cin, cout, k, stride, H, W = shape
    n, nw = 2, cout * cin * k * k
    seed = 1000 + cin + cout
    layers = PC.single_layer(cin, cout, k)
    P, plan = conv_plan(M, shape, n, tunes)
    x = O.normal_fill(seed, 2, 2, 0, 0, cin * H * W).reshape(cin, H, W)
    Ho, Wo = P.conv_out_hw(0, k, stride)
    dy = O.normal_fill(seed, 2, 3, 0, 0, n * cout * Ho * Wo).reshape(n, cout, Ho, Wo)
    dmus, ran = {}, set()
    for lay in ("fitted", "broad", "pruned"):
        mu, rho = PC.layout(lay, nw + cout, seed, layers=layers, dead=PC.dead_channels(layers) if lay == "pruned" else ())
        ys, dxs, r_dmu, q_ref = conv_reference(shape, mu, rho, x, dy, seed, STEP, K0, n)
        y, dz, dmu, drho = run_conv(plan, mu, rho, x, dy, seed, STEP, K0, n)
        fams = tuple(family(M, plan, w) for w in range(3))
        print("%s %s: families %s" % (name, lay, fams))
        for i in range(n):
            assert relerr(y[i], ys[i]) < 2e-6, ("fwd", lay, i)
            assert relerr(dz[i], dxs[i]) < 5e-6, ("dx", lay, i)
        assert relerr(dmu, r_dmu) < 2e-5, lay
        e = check_drho(drho, q_ref, rho, layers, 2e-5, (name, lay))
        note_as("q:bww-family-%d" % fams[2], e, "q rel err")
        dmus[lay] = dmu; ran.add(fams)
    assert ran == {want}, "passes ran on families %s, not %s" % (ran, want)
    if want[2] != 0:
        assert np.array_equal(bits(dmus["fitted"]), bits(dmus["broad"])), "dmu depends on rho"


@pytest.mark.parametrize("n", [1, 5, 19])
@pytest.mark.parametrize("name", ["mfma_s2", "generic_5x3"])
def test_sample_counts_beyond_one_trip(M, name, n):
    """n = 19: grad_finalize_kernel's sample loop (stride 16) takes its second trip, sample_weights_kernel (4 samples per thread) a fifth
    group; n = 5: a partial second group; n = 1.  Same tolerances."""
    shape, tunes, want = BWD_CASES[name]
    cin, cout, k, stride, H, W = shape
    nw = cout * cin * k * k
    seed = 2000 + cin + cout + n
    layers = PC.single_layer(cin, cout, k)
    P, plan = conv_plan(M, shape, n, tunes)
    x = O.normal_fill(seed, 2, 2, 0, 0, cin * H * W).reshape(cin, H, W)
    Ho, Wo = P.conv_out_hw(0, k, stride)
    dy = O.normal_fill(seed, 2, 3, 0, 0, n * cout * Ho * Wo).reshape(n, cout, Ho, Wo)
    for lay in ("broad", "pruned"):
        mu, rho = PC.layout(lay, nw + cout, seed, layers=layers)
        ys, dxs, r_dmu, q_ref = conv_reference(shape, mu, rho, x, dy, seed, STEP, K0, n)
        y, dz, dmu, drho = run_conv(plan, mu, rho, x, dy, seed, STEP, K0, n)
        assert tuple(family(M, plan, w) for w in range(3)) == want
        for i in range(n):
            assert relerr(y[i], ys[i]) < 2e-6, ("fwd", lay, i)
            assert relerr(dz[i], dxs[i]) < 5e-6, ("dx", lay, i)
        assert relerr(dmu, r_dmu) < 2e-5, lay
        check_drho(drho, q_ref, rho, layers, 2e-5, (name, lay, n))


# ---- 3. local reparameterisation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", ["fitted", "pruned"])
@pytest.mark.parametrize("shape", [(36, 16, 3, 1, 8, 8), (16, 4, 1, 1, 12, 12)])
def test_lrt_layer_at_a_fitted_and_a_pruned_posterior(M, shape, lay):
    """Conv2dLRT (tests/test_gpu_lrt.py's shapes and tolerances) against O.lrt_conv, rho restricted to [-8, 1]: below, sqrt(1e-16 + .)
    dominates the variance and the gradient is ill-conditioned in the reference too.  drho / (2 softplus64 sigmoid64) per layer at 6e-5."""
    cin, cout, k, stride, H, W = shape
    n, nw, seed, k0 = 2, cout * cin * k * k, 4300 + cin, 1
    layers = PC.single_layer(cin, cout, k)
    mu, rho = PC.layout(lay, nw + cout, seed, layers=layers, rho_span=(-8.0, 1.0))
    P, plan = conv_plan(M, shape, n, lrt=True)
    x = O.normal_fill(seed, 2, 2, 0, 0, cin * H * W).reshape(cin, H, W)
    Ho, Wo = P.conv_out_hw(0, k, stride)
    dy = O.normal_fill(seed, 2, 3, 0, 0, n * cout * Ho * Wo).reshape(n, cout, Ho, Wo)
    y, dz, dmu, drho = run_conv(plan, mu, rho, x, dy, seed, STEP, k0, n)
    r_dmu = np.zeros(nw + cout); r_ds = np.zeros(nw + cout)
    sp, sg = PC.softplus64(rho), PC.sigmoid64(rho)
    for i in range(n):
        yr, dx, dwm, dwr, dbm, dbr = O.lrt_conv(x, mu[:nw].reshape(cout, cin, k, k), rho[:nw].reshape(cout, cin, k, k), mu[nw:], rho[nw:],
                                                O.lrt_eps(seed, STEP, k0 + i, 0, cout * Ho * Wo), stride, dy[i])
        assert relerr(y[i], yr) < 2e-5, ("y", i)
        assert relerr(dz[i], dx) < 2e-5, ("dx", i)
        r_dmu += np.r_[dwm.ravel(), dbm]; r_ds += np.r_[dwr.ravel(), dbr]
    assert relerr(dmu, r_dmu) < 3e-5
    live = rho != np.float32(PC.PRUNED_RHO)
    assert np.all(drho[~live] == 0.0) and np.isfinite(drho).all()
    for tag, a, b in (("w", 0, nw), ("b", nw, nw + cout)):
        m = live[a:b]
        if not m.any():
            continue
        o32 = O.softplus(rho[a:b][m]).astype(np.float64)          # the oracle's own fp32 softplus and float64 sigmoid, divided out again
        ref = r_ds[a:b][m] / (2.0 * o32 * sg[a:b][m])
        got = drho[a:b][m].astype(np.float64) / (2.0 * sp[a:b][m] * sg[a:b][m])
        e = float(np.abs(got - ref).max() / np.abs(ref).max())
        note_as("lrt-q:%s" % tag, e, "q rel err")
        assert e < 6e-5, (tag, e)


# ---- 4. whole hour-glass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,lay,x6_bwd", [k + (PC.X6_BWD_STRIP,) for k in PC.NET_SEEDS] + [("net_b_64", "fitted", PC.X6_BWD)])
def test_nets_at_a_fitted_and_a_pruned_posterior(M, net, lay, x6_bwd):
    """test_small_nets_fwd_bwd's reference and tolerances (out 2e-5; dz, dmu, dbn 2e-4) with n = 3, k0 = 2; drho through q per layer at 2e-4.
    net_b_64 under pin_net_b: bf16x6 forward and backward-data (strip-resident; once with the strips reloaded) on its 36 -> 16 layer, the
    one-stage kernels on the 8- / 16-wide maps, a narrow 1x1 formed inside a fold."""
    kw = PC.NETS[net]
    seed, step, k0, n = PC.NET_SEEDS[(net, lay)], PC.NET_STEP, PC.NET_K0, PC.NET_N
    onet = O.make_net(**kw)
    P, zin, out_id, names = M.skip_program(**kw)
    mu, rho, bnp = PC.net_params(P, lay, seed)
    z = PC.net_input(kw, seed)
    plan = P.compile(zin, out_id, max_samples=n)
    if net == "net_b_64":
        pin_net_b(M, plan)
        (x6_op,) = [i for i, o in enumerate(P.ops) if o["type"] == M._lib.OP_CONV and o["ksize"] == 3 and o["stride"] == 1
                    and (P.tensors[o["in0"]]["C"], P.tensors[o["out"]]["C"], P.tensors[o["out"]]["W"]) == (36, 16, 64)]
        M._lib.check(M._lib.lib().mfvi_plan_set_tune(plan.handle, x6_op, 1, x6_bwd))
    d_mu, d_rho, d_bn, d_z = dev(mu), dev(rho), dev(bnp), dev(z)
    out = plan.forward(d_mu, d_rho, d_bn, d_z, seed, step, k0, n)
    dout = O.normal_fill(seed, 2, 9, 0, 0, out.numel()).reshape(tuple(out.shape))
    dmu = torch.zeros_like(d_mu); drho = torch.zeros_like(d_rho); dbn = torch.zeros_like(d_bn)
    dz = torch.empty((n,) + z.shape, device="cuda")
    plan.backward(d_mu, d_rho, d_bn, d_z, seed, step, k0, n, dev(dout), dmu, drho, dbn, dz=dz)
    fams = [{family(M, plan, w, op=i) for i, o in enumerate(P.ops) if o["type"] == M._lib.OP_CONV} for w in range(3)]
    print("%s %s: families %s" % (net, lay, fams))
    if net == "net_b_64":
        assert {1, 2, 3, 4} <= fams[0] and {1, 2, 3, 4, 5} <= fams[1] and {1, 3} <= fams[2], fams
        assert [M._lib.lib().mfvi_plan_last_kernel(plan.handle, x6_op, w) for w in range(3)] == [3, 3, 3]
    oh = host(out)
    r_dmu = np.zeros(P.n_vi); r_drho = np.zeros(P.n_vi); r_dbn = np.zeros(P.n_bn)
    for i in range(n):
        ref, tape = O.net_forward(onet, mu, rho, bnp, z, seed, step, k0 + i)
        assert relerr(oh[i], ref) < 2e-5, ("out", i)
        a, b, c_, dzr = tape.backward(dout[i], P.n_vi, P.n_bn, want_dz=True)
        r_dmu += a; r_drho += b; r_dbn += c_
        assert relerr(host(dz)[i], dzr) < 2e-4, ("dz", i)
        tape.free()
    assert relerr(host(dmu), r_dmu) < 2e-4
    assert relerr(host(dbn), r_dbn) < 2e-4
    g_rho = host(drho)
    assert np.isfinite(g_rho).all() and np.all(g_rho[rho == np.float32(PC.PRUNED_RHO)] == 0.0)
    worst, rows = PC.layer_q_err(g_rho, PC.q_of(r_drho, rho), rho, P.layers)
    for i, tag, e, share in rows:
        note_as("q:%s" % tag, e, "q rel err")
        assert e < 2e-4, (i, tag, e, share)
    assert min(PC.layer_shares(rho, P.layers)) >= 0.70


@pytest.mark.parametrize("lay", ["fitted", "pruned"])
def test_three_scale_net_against_the_reference_at_a_fitted_posterior(M, golden_dir, lay):
    """The reference's own MeanFieldVI autograd in float64 (oracle/make_golden.py, golden_posterior) on three_scale_32, K = 2, den data term
    without the KL term: output, NLL and gradients at test_small_golden_elbo_grad's tolerances, drho through q per layer."""
    g = np.load(os.path.join(golden_dir, "posterior_range.npz"), allow_pickle=False)
    kw = PC.NETS["three_scale_32"]
    seed, K, step = int(g["seed"]), int(g["K"]), int(g["step"])
    P, zin, out_id, _ = M.skip_program(**kw)
    mu, rho, bnp = PC.net_params(P, lay, seed)
    assert np.array_equal(mu, g[lay + "_mu"]) and np.array_equal(rho, g[lay + "_rho"])
    H, W = kw["H"], kw["W"]
    plan = P.compile(zin, out_id, max_samples=K)
    L = M._lib
    d_mu, d_rho, d_bn, d_z = dev(mu), dev(rho), dev(bnp), dev(PC.net_input(kw, seed))
    d_t = dev(O.noisy(O.phantom(H, W, seed), 0.1, seed))
    out = plan.forward(d_mu, d_rho, d_bn, d_z, seed, step, 0, K)
    assert relerr(host(out), g[lay + "_out"]) < 1e-4
    lossv = torch.zeros(1, dtype=torch.float64, device="cuda"); dout = torch.empty_like(out)
    L.check(L.lib().mfvi_gaussian_nll(L.ptr(out), L.ptr(d_t), K, H, W, 1, 1.0 / K, L.ptr(dout), L.ptr(lossv), L.stream_ptr()))
    # the NLL is a mean of terms of both signs (here -0.03 and -0.004): 1e-4 of the terms' size, not of what is left of them
    m_, s_ = g[lay + "_out"][:, 0].astype(np.float64), g[lay + "_out"][:, 1].astype(np.float64)
    scale = float(np.mean(np.exp(s_) * (m_ - host(d_t)) ** 2) + np.mean(np.abs(s_)))          # mean(exp(s) (t - m)^2 - s), s = out[:, 1]
    assert abs(float(lossv) / K - float(g[lay + "_nll"])) < 1e-4 * max(abs(float(g[lay + "_nll"])), scale)
    dmu = torch.zeros_like(d_mu); drho = torch.zeros_like(d_rho); dbn = torch.zeros_like(d_bn)
    plan.backward(d_mu, d_rho, d_bn, d_z, seed, step, 0, K, dout, dmu, drho, dbn)
    assert relerr(host(dmu), g[lay + "_dmu"]) < 3e-4 and relerr(host(dbn), g[lay + "_dbn"]) < 3e-4
    assert relerr(host(drho), g[lay + "_drho"]) < 3e-4
    worst, rows = PC.layer_q_err(host(drho), PC.q_of(g[lay + "_drho"], rho), rho, P.layers)
    for i, tag, e, share in rows:
        note_as("q:%s" % tag, e, "q rel err")
        assert e < 3e-4, (i, tag, e, share)
    assert min(PC.layer_shares(rho, P.layers)) >= 0.70
    assert np.all(host(drho)[rho == np.float32(PC.PRUNED_RHO)] == 0.0)


# ---- the kernel families this file ran on --------------------------------------------------------------------------------------------------
FILE_TESTS = {"test_draw_weight_by_weight", "test_bias_draw", "test_single_conv_backward_wide_rho", "test_sample_counts_beyond_one_trip",
              "test_nets_at_a_fitted_and_a_pruned_posterior"}
RAN = set()


@pytest.fixture(autouse=True)
def _ran(request):
    RAN.add(request.node.originalname)


def test_every_family_was_observed(M):
    """Last in the file.  The cases name, and their tests assert, families that cover the forward on all six forward families (0 - 4 and 6),
    5 in the backward-data slot of the hour-glass (all seven between them), backward-data on the generic, fp32 matrix-core, bf16x6 and
    one-stage kernels, backward-weight on the generic, fp32 matrix-core and bf16x6 kernels; when the file ran as a whole, that is also
    what mfvi_plan_last_kernel reported."""
    assert set(PC.FWD_FAMILY.values()) >= {0, 1, 2, 3, 4, 6}
    assert {w[1] for _, _, w in BWD_CASES.values()} >= {0, 1, 2, 4} and {w[2] for _, _, w in BWD_CASES.values()} >= {0, 1, 3}          # (3, 5: the hour-glass)
    if FILE_TESTS <= RAN:
        assert SEEN[0] >= {0, 1, 2, 3, 4, 6} and SEEN[0] | SEEN[1] | SEEN[2] >= set(range(7)), SEEN
        assert SEEN[1] >= {0, 1, 3, 4, 5} and SEEN[2] >= {0, 1, 3}, SEEN
