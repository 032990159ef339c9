"""Batched inpainting fits: the generic fp32 convolution kernels in the plan's fits mode against single-fit passes of
the same plan type, the three per-fit inpainting kernels against the single-fit entry points / the oracle / float64 numpy, InpaintBatch
against the standalone engine and against a float64 PyTorch restatement per fit, NaN isolation, to_engine, the reference's 320 x 256 shape,
and the runner's --inpaint-fits.

The small net throughout: nd = nu = (8, 16, 16), no skip branches, 5x5 down filters, nearest up-sampling, input depth 8, 4 outputs, at
H x W = 24 x 40 -- maps 12 x 20, 6 x 10 and 3 x 5: the first level stays on the matrix cores, the two deeper ones (widths 10 and 5, the deep
widths of the reference's 320-wide images) go to the generic kernels; non-square, so a swapped H / W shows.
Every parity test writes distinct BatchNorm parameters per fit: at initialisation all fits have gamma = 1, beta = 0 and an indexing error
would be invisible."""
import json
import os

import numpy as np
import pytest

from conftest import note_margin as _note

from oracle import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INP_SMALL = dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(0, 0, 0), fd=5, fu=3, need1x1_up=False, upsample_mode="nearest")
NET_KW = dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(0, 0, 0))                  # what InpaintBatch / ElboEngine(task="inp") take on top of INP_NET
SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))
H0, W0 = 24, 40
FAM_GENERIC = 0
TUNE_GENERIC = 1 << 27                                                      # MFVI_TUNE_GENERIC: the in-kernel-eps tiling of a layer


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
    v = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
    _note(v, "relerr")
    return v


def moved(a, b):
    """relerr for the tests' own discriminating-power checks: not a parity margin, so not put on record."""
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


def write_bn(ib, seed):
    for f in range(ib.F):
        ib.fit(f)["bn"].copy_(dev(bn_values(ib.prog, seed, f)))


def families(M, plan, which):
    lib = M._lib.lib()
    return {lib.mfvi_plan_last_kernel(plan.handle, i, which) for i, o in enumerate(plan.prog.ops) if o["type"] == M._lib.OP_CONV}


def narrow_ops(M, plan):
    """The convolutions whose input map is no multiple of 4 wide: the matrix-core forward kernels decline them."""
    T = plan.prog.tensors
    return [i for i, o in enumerate(plan.prog.ops) if o["type"] == M._lib.OP_CONV and T[o["in0"]]["W"] % 4]


def pin_generic_weight_gradient(M, plan):
    """The matrix-core backward-weight kernels serve narrow maps too (their 4-wave variant stages scalars), so the heuristic never sends a
    layer of the sampling table to the generic weight-gradient kernel: the in-kernel-eps tiling (bit 27) does, set AFTER the mode is on."""
    for i in narrow_ops(M, plan):
        M._lib.check(M._lib.lib().mfvi_plan_set_tune(plan.handle, i, 2, TUNE_GENERIC))


def check_families(M, plan, weight_gradient_pinned=False):
    """Family 0 (generic) and a matrix-core family each served an op of the forward and the backward-data pass (and of the backward-weight
    pass where the test pinned it): the convolutions on maps no multiple of 4 wide report family 0, those on wider maps a matrix-core family."""
    T, lib, wide = plan.prog.tensors, M._lib.lib(), 0
    narrow = narrow_ops(M, plan)
    assert narrow
    for which in range(3 if weight_gradient_pinned else 2):
        fam = families(M, plan, which)
        assert FAM_GENERIC in fam and any(x > 0 for x in fam), (which, fam)
    assert any(x > 0 for x in families(M, plan, 2))
    for i, o in enumerate(plan.prog.ops):
        if o["type"] != M._lib.OP_CONV:
            continue
        f0, f2 = lib.mfvi_plan_last_kernel(plan.handle, i, 0), lib.mfvi_plan_last_kernel(plan.handle, i, 2)
        if i in narrow:
            assert f0 == FAM_GENERIC and (f2 == FAM_GENERIC) == weight_gradient_pinned, (i, f0, f2)
        elif T[o["out"]]["W"] % 4 == 0:
            wide += 1
            assert f0 > 0 and f2 > 0, (i, f0, f2)
    assert wide > 0


def _hyper(F):
    return [1e-6 * 2 ** f for f in range(F)], [0.05 * 2 ** f for f in range(F)], [1e-3 * (f + 1) for f in range(F)]


def images_and_masks(F, H, W, seed, mask_channels=1):
    img = np.stack([np.stack([O.phantom(H, W, seed + 10 * f + c) for c in range(3)]) for f in range(F)]).astype(np.float32)
    # a different share of known pixels per fit (0.8, 0.55, 0.3, ...): another fit's mask then moves the data term and its gradient visibly
    u = O.uniform_fill(seed, 5, 0, 0, F * mask_channels * H * W).reshape(F, mask_channels, H, W)
    mask = np.stack([(u[f] > min(0.2 + 0.25 * f, 0.9)).astype(np.float32) for f in range(F)])
    return img, mask


# ---- 1. plan parity with generic layers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,S", [(4, 1), (3, 2)])
@pytest.mark.parametrize("net", ["inp", "small"])
def test_plan_fits_mode_with_generic_layers_matches_single_fit_passes(M, net, F, S):
    """One forward + backward in fits mode against F single-fit calls of the same plan type with fit f's row and input, k0 = f S, n = S.
    Bounds as test_plan_fits_mode_matches_single_fit_passes: outputs 1e-5, gradients 2e-4 relative to the largest reference value (the
    arithmetic per fit is the same; the fp64 BN atomics and the generic kernels' fp32 weight-gradient atomics reorder)."""
    seed, step = 31, 5
    if net == "inp":
        H, W, depth, n_out = H0, W0, 8, 4
        P, zin, zout, _ = M.skip_program(H, W, depth, n_out, **INP_SMALL)
    else:
        H, W, depth, n_out = 24, 24, 8, 2                                  # maps 24, 12, 6: concat, bilinear and a generic level
        P, zin, zout, _ = M.skip_program(H, W, depth, n_out, **SMALL)
    n, nv, nb = F * S, P.n_vi, P.n_bn
    n_params = 2 * nv + nb
    stride = (n_params + 3) // 4 * 4 + 8                                  # rows further apart than they are long ...
    gstride = stride + 12                                                 # ... and the gradient rows another distance apart: a swapped stride shows
    rows = np.zeros((F, stride), np.float32)
    for f in range(F):
        rows[f, :nv] = 0.1 * O.normal_fill(seed, 2, 0, f, 0, nv)
        rows[f, nv:2 * nv] = -3.0 + 0.1 * O.normal_fill(seed, 2, 1, f, 0, nv)
        rows[f, 2 * nv:n_params] = bn_values(P, seed, f)
    z = np.stack([0.1 * O.uniform_fill(seed, 0, f, 0, depth * H * W).reshape(depth, H, W) for f in range(F)]).astype(np.float32)
    dout = (O.normal_fill(seed, 2, 3, 0, 0, n * n_out * H * W).reshape(n, n_out, H, W) / (H * W)).astype(np.float32)
    d_rows, d_z, d_dout = dev(rows), dev(z), dev(dout)
    pf = P.compile(zin, zout, n); pf.set_fits(S, stride, gstride); pin_generic_weight_gradient(M, pf)
    g = torch.zeros((F, gstride), device="cuda")
    out = pf.forward(d_rows[0, :nv], d_rows[0, nv:], d_rows[0, 2 * nv:], d_z, seed, step, 0, n)
    pf.backward(d_rows[0, :nv], d_rows[0, nv:], d_rows[0, 2 * nv:], d_z, seed, step, 0, n, d_dout, g[0, :nv], g[0, nv:], g[0, 2 * nv:])
    check_families(M, pf, weight_gradient_pinned=True)
    out, g = host(out), host(g)
    assert np.all(g[:, n_params:] == 0.0)                                  # nothing is written between the rows
    ps = P.compile(zin, zout, S); pin_generic_weight_gradient(M, ps)

    def single(f, row_of=None, k_of=None):
        r = d_rows[f if row_of is None else row_of]
        k0 = (f if k_of is None else k_of) * S
        gs = torch.zeros(n_params, device="cuda")
        o = ps.forward(r[:nv], r[nv:2 * nv], r[2 * nv:n_params], d_z[f], seed, step, k0, S)
        ps.backward(r[:nv], r[nv:2 * nv], r[2 * nv:n_params], d_z[f], seed, step, k0, S, d_dout[f * S:(f + 1) * S].contiguous(), gs[:nv], gs[nv:2 * nv], gs[2 * nv:])
        return host(o), host(gs)

    # the test's own discriminating power: the single-fit pass with another fit's row, or with another fit's k0, misses by > 100 x the bound
    o_ok, g_ok = single(0)
    for kind, (o_w, g_w) in (("row", single(0, row_of=1)), ("k0", single(0, k_of=1))):
        eo, eg = moved(o_w, o_ok), moved(g_w[:nv], g_ok[:nv])
        print("%s F=%d S=%d: wrong %s moves the output by %.2e, dmu by %.2e" % (net, F, S, kind, eo, eg))
        assert eo > 100 * 1e-5 and eg > 100 * 2e-4, (kind, eo, eg)
    for f in range(F):
        o, gs = (o_ok, g_ok) if f == 0 else single(f)
        e = relerr(out[f * S:(f + 1) * S], o)
        print("%s F=%d S=%d fit %d: out %.2e" % (net, F, S, f, e))
        assert e < 1e-5, (f, e)
        for name, a, b in (("dmu", g[f, :nv], gs[:nv]), ("drho", g[f, nv:2 * nv], gs[nv:2 * nv]), ("dbn", g[f, 2 * nv:n_params], gs[2 * nv:])):
            e = relerr(a, b)
            print("    %s %.2e" % (name, e))
            assert e < 2e-4, (f, name, e)


# ---- 2. mfvi_gaussian_nll_inpainting_fits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mc", [1, 3])
@pytest.mark.parametrize("H,W", [(7, 9), (12, 20)])
def test_gaussian_nll_inpainting_fits(M, H, W, mc):
    lib, sp, p_ = M._lib.lib(), M._lib.stream_ptr(), M._lib.ptr
    F, S, seed = 3, 2, 17
    out_h = (2.0 * O.normal_fill(seed, 2, 0, 0, 0, F * S * 4 * H * W)).reshape(F * S, 4, H, W).astype(np.float32)
    out_h[0, 3, 0, :4] = [25.0, -30.0, 19.9, 0.0]; out_h[3, 3, 1, :3] = [25.0, -30.0, 19.9]        # the clamp branches, in two fits
    tg_h = O.uniform_fill(seed, 1, 0, 0, F * 3 * H * W).reshape(F, 3, H, W).astype(np.float32)
    mk_h = (O.uniform_fill(seed, 2, 0, 0, F * mc * H * W).reshape(F, mc, H, W) > 0.3).astype(np.float32)
    # the exp(20) pixels carry most of their fit's sum: known in their own fit's mask, unknown in the mask of the fit they are confused with below
    mk_h[0, :, 0, :4] = 1.0; mk_h[1, :, 0, :4] = 0.0; mk_h[1, :, 1, :3] = 1.0; mk_h[2, :, 1, :3] = 0.0
    out, tg, mk = dev(out_h), dev(tg_h), dev(mk_h)
    dout = torch.full_like(out, 7.0); nll = torch.zeros(F, dtype=torch.float64, device="cuda")
    M._lib.check(lib.mfvi_gaussian_nll_inpainting_fits(p_(out), p_(tg), 3 * H * W, p_(mk), mc * H * W, mc, F, S, H, W, 0.5, p_(dout), p_(nll), sp))
    nll_h, dout_h = host(nll), host(dout)
    for f in range(F):
        d1 = torch.full((S, 4, H, W), 7.0, device="cuda"); n1 = torch.zeros(1, dtype=torch.float64, device="cuda")
        M._lib.check(lib.mfvi_gaussian_nll_inpainting(p_(out[f * S:]), p_(tg[f]), p_(mk[f]), mc, S, H, W, 0.5, p_(d1), p_(n1), sp))
        assert np.array_equal(dout_h[f * S:(f + 1) * S], host(d1)), f                 # shared per-pixel code: bit-equal
        assert abs(nll_h[f] - float(n1[0])) < 2e-6 * abs(float(n1[0])), f
        ref = [O.gaussian_nll_inp(out_h[f * S + k], tg_h[f], mk_h[f], scale=0.5, want_grad=True) for k in range(S)]
        want = sum(r[0] for r in ref)
        assert abs(nll_h[f] - want) < 1e-5 * abs(want), (f, nll_h[f], want)
        for k in range(S):
            assert relerr(dout_h[f * S + k], ref[k][1]) < 5e-6, (f, k)
        # fit f scored against fit g's mask or target misses by more than 100 x the bound, loss and gradient
        g_ = (f + 1) % F
        for kind, t_, m_ in (("target", tg_h[g_], mk_h[f]), ("mask", tg_h[f], mk_h[g_])):
            wrong = [O.gaussian_nll_inp(out_h[f * S + k], t_, m_, scale=0.5, want_grad=True) for k in range(S)]
            dl = abs(sum(r[0] for r in wrong) - want) / abs(want)
            dg = moved(wrong[0][1], ref[0][1])
            print("H=%d W=%d mc=%d fit %d: wrong %s moves the loss by %.2e, dout by %.2e" % (H, W, mc, f, kind, dl, dg))
            assert dg > 100 * 5e-6 and dl > 100 * 1e-5, (kind, f, dl, dg)
    # one mask shared by every fit (mask_stride 0), loss only, accumulating (+=)
    n2 = torch.zeros(F, dtype=torch.float64, device="cuda")
    for _ in range(2):
        M._lib.check(lib.mfvi_gaussian_nll_inpainting_fits(p_(out), p_(tg), 3 * H * W, p_(mk[1]), 0, mc, F, S, H, W, 0.5, None, p_(n2), sp))
    assert abs(float(n2[1]) - 2 * nll_h[1]) < 2e-6 * abs(2 * nll_h[1])
    want0 = sum(O.gaussian_nll_inp(out_h[k], tg_h[0], mk_h[1], scale=0.5) for k in range(S))
    assert abs(float(n2[0]) - 2 * want0) < 1e-5 * abs(2 * want0)
    rc = lib.mfvi_gaussian_nll_inpainting_fits(p_(out), p_(tg), 3 * H * W - 1, p_(mk), mc * H * W, mc, F, S, H, W, 0.5, None, p_(n2), sp)
    assert rc == -1 and b"gaussian_nll_inpainting_fits" in lib.mfvi_last_error()
    rc = lib.mfvi_gaussian_nll_inpainting_fits(p_(out), p_(tg), 3 * H * W, p_(mk), mc * H * W, 2, F, S, H, W, 0.5, None, p_(n2), sp)
    assert rc == -1


# ---- 3. mfvi_ema_inpainting_fits -------------------------------------------------------------------------------------------------------------
def test_ema_inpainting_fits_against_float64_restatement(M):
    lib, sp, p_ = M._lib.lib(), M._lib.stream_ptr(), M._lib.ptr
    F, S, H, W, seed, w = 3, 2, 7, 9, 5, 0.99
    ema = torch.full((F, 4, H, W), 123.0, device="cuda")                  # the first update copies
    ref = None
    for it in range(2):
        o = (1.5 * O.normal_fill(seed, 2, 0, 0, it, F * S * 4 * H * W)).reshape(F, S, 4, H, W).astype(np.float32)
        M._lib.check(lib.mfvi_ema_inpainting_fits(p_(dev(o.reshape(F * S, 4, H, W))), F, S, H, W, p_(ema), w, int(it == 0), sp))
        o64 = o.astype(np.float64)
        cur = np.concatenate([(1.0 / (1.0 + np.exp(-o64[:, :, :3]))).mean(axis=1), np.exp(-o64[:, :, 3:]).mean(axis=1)], axis=1)
        ref = cur if it == 0 else ref * np.float64(np.float32(w)) + cur * (1.0 - np.float64(np.float32(w)))
        assert relerr(host(ema), ref) < 2e-6, it
    # one fit of the batch is the EMA part of mfvi_bookkeep_inpainting
    e1 = torch.zeros((4, H, W), device="cuda")
    s3 = [torch.zeros((3, H, W), device="cuda") for _ in range(5)]; s1 = torch.zeros((H, W), device="cuda")
    img = torch.zeros((3, H, W), device="cuda"); mk = torch.ones((1, H, W), device="cuda")
    M._lib.check(lib.mfvi_bookkeep_inpainting(p_(dev(o[1])), S, H, W, p_(img), p_(mk), 1, p_(e1), w, 1, p_(s3[0]), p_(s1), p_(s3[1]), p_(s3[2]), p_(s3[3]),
                                              p_(s3[4]), None, None, sp))
    e2 = torch.zeros((F, 4, H, W), device="cuda")
    M._lib.check(lib.mfvi_ema_inpainting_fits(p_(dev(o.reshape(F * S, 4, H, W))), F, S, H, W, p_(e2), w, 1, sp))
    assert torch.equal(e2[1], e1)


# ---- 4. mfvi_masked_sq_err_fits --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,mc", [(7, 9, 1), (7, 9, 3), (48, 72, 1), (48, 72, 3)])
def test_masked_sq_err_fits(M, H, W, mc):
    """Against float64 numpy at 1e-6 relative (an fp32 clip and product per element, fp64 accumulation: a few fp32 ulp of relative error per
    term); two calls bit-identical; 48 x 72: 3 H W / 256 = 40.5 -> 41 blocks per fit."""
    lib, sp, p_ = M._lib.lib(), M._lib.stream_ptr(), M._lib.ptr
    F, seed = 3, 29
    HW = H * W
    ema_h = (0.5 + 0.6 * O.normal_fill(seed, 2, 0, 0, 0, F * 4 * HW)).reshape(F, 4, H, W).astype(np.float32)       # values below 0 and above 1: the clip matters
    img_h = O.uniform_fill(seed, 1, 0, 0, F * 3 * HW).reshape(F, 3, H, W).astype(np.float32)
    mk_h = (O.uniform_fill(seed, 2, 0, 0, F * mc * HW).reshape(F, mc, H, W) > 0.3).astype(np.float32)
    ema, img, mk = dev(ema_h), dev(img_h), dev(mk_h)
    scratch = torch.zeros(F * M._lib.MASKED_SQ_ERR_BLOCKS, dtype=torch.float64, device="cuda")
    runs = []
    for _ in range(2):
        acc = torch.full((F,), -1.0, dtype=torch.float64, device="cuda")           # overwritten, not accumulated
        M._lib.check(lib.mfvi_masked_sq_err_fits(p_(ema), 4 * HW, p_(img), 3 * HW, p_(mk), mc * HW, mc, F, H, W, p_(acc), p_(scratch), sp))
        runs.append(host(acc))
    assert np.array_equal(runs[0], runs[1])
    e64, i64, m64 = ema_h.astype(np.float64), img_h.astype(np.float64), mk_h.astype(np.float64)
    want = ((np.clip(e64[:, :3], 0, 1) * m64 - i64 * m64) ** 2).sum(axis=(1, 2, 3))
    for f in range(F):
        assert abs(runs[0][f] - want[f]) < 1e-6 * want[f], (f, runs[0][f], want[f])
    wrong = ((np.clip(e64[:, :3], 0, 1) * np.roll(m64, 1, axis=0) - i64 * np.roll(m64, 1, axis=0)) ** 2).sum(axis=(1, 2, 3))
    assert np.all(np.abs(wrong - want) > 100 * 1e-6 * want)                        # another fit's mask would show
    # one shared mask: stride 0
    acc = torch.zeros(F, dtype=torch.float64, device="cuda")
    M._lib.check(lib.mfvi_masked_sq_err_fits(p_(ema), 4 * HW, p_(img), 3 * HW, p_(mk[2]), 0, mc, F, H, W, p_(acc), p_(scratch), sp))
    want2 = ((np.clip(e64[:, :3], 0, 1) * m64[2] - i64 * m64[2]) ** 2).sum(axis=(1, 2, 3))
    assert np.all(np.abs(host(acc) - want2) < 1e-6 * want2)
    assert lib.mfvi_masked_sq_err_fits(p_(ema), 3 * HW - 1, p_(img), 3 * HW, p_(mk), mc * HW, mc, F, H, W, p_(acc), p_(scratch), sp) == -1
    assert b"masked_sq_err_fits" in lib.mfvi_last_error()


# ---- 5. fit 0 is the standalone engine ---------------------------------------------------------------------------------------------------------
def test_fit0_is_the_standalone_inpainting_engine(M):
    H, W, K, seed = H0, W0, 2, 9
    temps, sigmas, lrs = _hyper(3)
    ib = M.InpaintBatch(H, W, 3, K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=NET_KW, autotune=False)
    eng = M.engine.ElboEngine(H, W, task="inp", K=K, input_depth=8, temp=temps[0], sigma=sigmas[0], lr=lrs[0], seed=seed, net_kwargs=NET_KW, autotune=False)
    assert torch.equal(ib.fit(0)["params"], eng.params) and torch.equal(ib.z0[0], eng.z0)          # bit-equal initial values and input
    assert not torch.equal(ib.fit(1)["params"], eng.params) and not torch.equal(ib.z0[1], eng.z0)
    assert ib.prior_sigma[0] == eng.prior_sigma
    write_bn(ib, seed); eng.bn.copy_(ib.fit(0)["bn"])
    img, mask = images_and_masks(3, H, W, seed)
    ib.set_targets(torch.from_numpy(img), torch.from_numpy(mask)); eng.set_target(torch.from_numpy(img[0]), torch.from_numpy(mask[0]))
    ib.grad_only(0); eng.grad_only(0, with_kl=False)
    check_families(M, ib.plan)
    assert torch.equal(ib.z[0], eng.z)
    g, ge = host(ib.fit(0)["grads"]), host(eng.grads[:eng.n_params])
    nv = ib.n_vi
    for name, sl in (("dmu", slice(0, nv)), ("drho", slice(nv, 2 * nv)), ("dbn", slice(2 * nv, None))):
        e = relerr(g[sl], ge[sl])
        print("%s %.2e" % (name, e))
        assert e < 2e-4, (name, e)
    a, b = float(ib.nll_acc[0]), float(eng.acc[0])
    assert abs(a - b) < 1e-5 * abs(b), (a, b)


# ---- 6. every fit against a float64 restatement ------------------------------------------------------------------------------------------------
def test_every_fit_against_float64_restatement(M):
    """F = 3, K = 2, distinct temp / sigma / lr / image / mask / gamma, beta.  grad_only(0) of each fit against the float64 interpreter of the
    layer program with the oracle's eps and the torch masked NLL (bounds of tests/test_gpu_inpainting.py for this net family: outputs 5e-5,
    gradients 5e-4), then three step()s against float64 KL gradient + Adam on the restatement's gradients, re-anchored after every step
    (bounds of test_batch_steps_match_oracle_per_fit: loss 2e-4 relative, parameters max 2.5e-3 (it + 1), mean 5e-5 (it + 1)).  The standalone
    ElboEngine(task="inp") runs fit 0's state against the same restatement beside the batch; the deviations of both are printed and noted."""
    import inp_restatement as R
    H, W, F, K, seed = H0, W0, 3, 2, 4
    temps, sigmas, lrs = _hyper(F)
    ib = M.InpaintBatch(H, W, F, K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=NET_KW, autotune=False)
    write_bn(ib, seed)
    img, mask = images_and_masks(F, H, W, seed)
    ib.set_targets(torch.from_numpy(img), torch.from_numpy(mask))
    P, zin, zout, nv, npar = ib.prog, ib.zin, ib.zout, ib.n_vi, ib.n_params
    p = host(ib.params).astype(np.float64)
    z0 = host(ib.z0)

    def z_of(f, it):
        return z0[f].astype(np.float64) + np.float64(np.float32(0.1)) * O.normal_fill(seed, 1, 0, f, it, z0[f].size).reshape(z0[f].shape).astype(np.float64)

    def restate(f, it, mask_of=None, bn_of=None, k_of=None):
        mf, bf, kf = (f if x is None else x for x in (mask_of, bn_of, k_of))
        row = p[f].copy()
        row[2 * nv:] = p[bf, 2 * nv:]
        return R.inp_grad(P, zin, zout, row, z_of(f, it), img[f], mask[mf], seed, it, kf * K, K)

    def total(r, row, f, hyper_of=None):
        hf = f if hyper_of is None else hyper_of
        kl, dkl = R.kl_and_grad(row, nv, ib.prior_sigma[hf])
        return r["nll"] + temps[hf] * kl, r["grad"] + temps[hf] * dkl

    # the test's own discriminating power, on the CPU: the restatement given ANOTHER fit's mask, gamma / beta, eps index or hyper-parameters
    # misses the right answer by more than 100 x the bound it is compared under
    right = restate(0, 0); l_right, g_right = total(right, p[0], 0)
    for kind, wrong in (("mask", restate(0, 0, mask_of=1)), ("bn", restate(0, 0, bn_of=1)), ("eps", restate(0, 0, k_of=1))):
        # each compared quantity over its own bound (outputs 5e-5, gradients 5e-4, data term 2e-4): the worst of them must exceed 100
        miss = dict(out=moved(wrong["out"], right["out"]) / 5e-5, dmu=moved(wrong["grad"][:nv], right["grad"][:nv]) / 5e-4,
                    drho=moved(wrong["grad"][nv:2 * nv], right["grad"][nv:2 * nv]) / 5e-4, dbn=moved(wrong["grad"][2 * nv:], right["grad"][2 * nv:]) / 5e-4,
                    nll=abs(wrong["nll"] - right["nll"]) / abs(right["nll"]) / 2e-4)
        print("wrong %s misses by (multiples of the bound): %s" % (kind, {k: round(v, 1) for k, v in miss.items()}))
        assert max(miss.values()) > 100, (kind, miss)
        assert kind == "mask" or miss["out"] > 100, (kind, miss)                 # (the mask does not enter the net's output)
    l_w, g_w = total(right, p[0], 0, hyper_of=1)
    assert abs(l_w - l_right) / abs(l_right) > 100 * 2e-4 or moved(g_w[:2 * nv], g_right[:2 * nv]) > 100 * 5e-4

    ib.grad_only(0)
    out, g = host(ib.out), host(ib.grads)
    for f in range(F):
        r = right if f == 0 else restate(f, 0)
        eo = relerr(out[f * K:(f + 1) * K], r["out"])
        print("fit %d: out %.2e" % (f, eo))
        assert eo < 5e-5, (f, eo)
        for name, sl in (("dmu", slice(0, nv)), ("drho", slice(nv, 2 * nv)), ("dbn", slice(2 * nv, npar))):
            e = relerr(g[f, sl], r["grad"][sl])
            print("    %s %.2e" % (name, e))
            assert e < 5e-4, (f, name, e)
        assert abs(float(ib.nll_acc[f]) / K - r["nll"]) < 2e-4 * abs(r["nll"]), f

    # three steps; the standalone engine on fit 0's state beside the batch
    eng = M.engine.ElboEngine(H, W, task="inp", K=K, input_depth=8, temp=temps[0], sigma=sigmas[0], lr=lrs[0], seed=seed, net_kwargs=NET_KW, autotune=False)
    eng.params.copy_(ib.fit(0)["params"]); eng.set_target(torch.from_numpy(img[0]), torch.from_numpy(mask[0]))
    assert torch.equal(eng.z0, ib.z0[0])
    m = np.zeros_like(p); v = np.zeros_like(p)
    worst = dict(batch=[0.0, 0.0, 0.0], engine=[0.0, 0.0, 0.0])         # loss (relative), parameter max / (it + 1), parameter mean / (it + 1)
    for it in range(3):
        ib.step(); eng.step()
        nll, kl, loss = ib.losses()
        pn = host(ib.params).astype(np.float64)
        for f in range(F):
            r = R.inp_grad(P, zin, zout, p[f], z_of(f, it), img[f], mask[f], seed, it, f * K, K)
            l_ref, g_ref = total(r, p[f], f)
            q = p[f].copy()
            R.adam64(q, g_ref, m[f], v[f], lrs[f], it + 1)
            d = np.abs(pn[f] - q)
            dl = abs(loss[f] - l_ref) / max(abs(l_ref), 1e-3)
            print("fit %d it %d: loss %.6f / %.6f (%.2e), params max %.2e mean %.2e" % (f, it, loss[f], l_ref, dl, d.max(), d.mean()))
            worst["batch"] = [max(a, b) for a, b in zip(worst["batch"], (dl, d.max() / (it + 1), d.mean() / (it + 1)))]
            if f == 0:
                de = np.abs(host(eng.params).astype(np.float64) - q)
                le = abs(eng.losses()[2] - l_ref) / max(abs(l_ref), 1e-3)
                print("    standalone engine: loss %.2e, params max %.2e mean %.2e" % (le, de.max(), de.mean()))
                worst["engine"] = [max(a, b) for a, b in zip(worst["engine"], (le, de.max() / (it + 1), de.mean() / (it + 1)))]
            assert dl < 2e-4, (f, it, loss[f], l_ref)
            assert d.max() < 2.5e-3 * (it + 1) and d.mean() < 5e-5 * (it + 1), (f, it, d.max(), d.mean())
        p = pn.copy()                                  # re-anchor: Adam amplifies rounding noise of near-zero gradients
        eng.params.copy_(ib.fit(0)["params"]); eng.m.copy_(ib.fit(0)["m"]); eng.v.copy_(ib.fit(0)["v"])
    for who in ("batch", "engine"):
        for name, val in zip(("loss", "params_max_per_it", "params_mean_per_it"), worst[who]):
            _note(val, "%s %s" % (who, name))
    print("worst deviations (loss rel, params max / (it+1), params mean / (it+1)): batch %s, standalone engine %s" % (worst["batch"], worst["engine"]))
    assert not ib.dead.any()


# ---- 7. isolation and export -------------------------------------------------------------------------------------------------------------------
def test_nan_fit_is_isolated_and_to_engine_exports(M):
    H, W, F, K, seed = H0, W0, 3, 2, 12
    temps, sigmas, lrs = _hyper(F)
    img, mask = images_and_masks(F, H, W, seed)
    bad = img.copy(); bad[1, 2, 5, 7] = np.nan; mask[1, 0, 5, 7] = 1.0          # a known pixel: the NaN reaches the data term
    ibs = []
    for t in (img, bad):
        ib = M.InpaintBatch(H, W, F, K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=NET_KW, autotune=False)
        write_bn(ib, seed); ib.set_targets(torch.from_numpy(t), torch.from_numpy(mask)); ib.grad_only(0)
        ibs.append(ib)
    clean, ib = ibs
    for f in (0, 2):
        assert relerr(host(ib.fit(f)["grads"]), host(clean.fit(f)["grads"])) < 2e-4, f
    before = [host(x).copy() for x in (ib.params, ib.m, ib.v)]
    ib.step(); ib.step(); clean.step(); clean.step()
    assert list(ib.dead) == [0, 1, 0] and not clean.dead.any()
    after = [host(x) for x in (ib.params, ib.m, ib.v)]
    for a, b in zip(before, after):
        assert np.array_equal(a[1], b[1])                                  # the dead fit: parameters and moments bit-equal to before
        for f in (0, 2):
            assert np.isfinite(b[f]).all()
    pc = host(clean.params)
    for f in (0, 2):
        assert not np.array_equal(before[0][f], after[0][f])
        # the other fits: as in the run without the NaN, after two Adam steps on gradients equal to 2e-4 (above): the mean bound of the stepping
        # tests, 5e-5 per step (two unrelated runs differ by about lr per step, 20 to 60 times as much; a max bound below 2 lr cannot be had
        # from Adam on near-zero gradients, and one above it says nothing)
        d = np.abs(after[0][f] - pc[f])
        print("fit %d: parameters against the run without the NaN: max %.2e mean %.2e" % (f, d.max(), d.mean()))
        assert d.mean() < 5e-5 * 2, (f, d.max(), d.mean())
    assert np.isnan(ib.losses()[0][1]) and np.isfinite(ib.losses()[2][[0, 2]]).all()
    # export
    snap = [host(x).copy() for x in (clean.params, clean.m, clean.v, clean.ema)]
    eng = clean.to_engine(2)
    assert np.array_equal(host(eng.params), snap[0][2]) and np.array_equal(host(eng.m), snap[1][2]) and np.array_equal(host(eng.v), snap[2][2])
    assert eng.t == clean.t == 2 and int(eng.t_applied[0]) == 2 and torch.equal(eng.z0, clean.z0[2])
    assert torch.equal(eng.target, clean.images[2]) and torch.equal(eng.mask, clean.masks[2]) and eng.task == "inp"
    assert (eng.temp, eng.lr, eng.prior_sigma) == (temps[2], lrs[2], clean.prior_sigma[2])
    r = eng.predict(4, target=torch.from_numpy(img[2]))
    for k in ("mean", "epi", "ale", "total"):
        assert tuple(r[k].shape[-2:]) == (H, W) and torch.isfinite(r[k]).all(), k
    for a, b in zip(snap, (clean.params, clean.m, clean.v, clean.ema)):
        assert np.array_equal(a, host(b))                                  # the batch is untouched
    rec, ale = host(clean.recon()), host(clean.ale())
    assert rec.shape == (F, 3, H, W) and ale.shape == (F, H, W) and rec.min() >= 0 and rec.max() <= 1 and ale.min() >= 0 and ale.max() <= 1
    ps = clean.psnr(img)
    assert ps.shape == (F,) and np.isfinite(ps).all()
    want = 10 * np.log10(1.0 / np.mean((rec[1].astype(np.float64) * mask[1] - img[1].astype(np.float64) * mask[1]) ** 2))
    assert abs(ps[1] - want) < 1e-4, (ps[1], want)
    with pytest.raises(ValueError):
        clean.to_engine(3)


# ---- 8. the reference's shape -------------------------------------------------------------------------------------------------------------------
def test_reference_shape_runs_on_generic_and_matrix_core_kernels(M):
    """320 x 256 images of the reference (H = 256, W = 320), default net and depth: maps 160 .. 10, 5 wide.  Nothing is compared numerically."""
    H, W = 256, 320
    ib = M.InpaintBatch(H, W, 2, K=1, temp=[1e-6, 2e-6], sigma=[0.05, 0.1], seed=3, autotune=False)
    assert len(ib.prog.layers) == 19 and tuple(ib.out.shape) == (2, 4, H, W)
    img = np.stack([np.stack([O.phantom(H, W, 3 + f + c) for c in range(3)]) for f in range(2)]).astype(np.float32)
    mask = (O.uniform_fill(3, 5, 0, 0, H * W).reshape(1, H, W) > 0.3).astype(np.float32)
    ib.set_targets(torch.from_numpy(img), torch.from_numpy(mask))            # one mask shared by both fits
    for _ in range(2):
        ib.step()
    nll, kl, loss = ib.losses()
    assert np.isfinite(nll).all() and np.isfinite(kl).all() and np.isfinite(loss).all() and not ib.dead.any()
    check_families(M, ib.plan)
    assert np.isfinite(ib.psnr(img[0])).all()


# ---- 9. runner ------------------------------------------------------------------------------------------------------------------------------------
def test_runner_inpaint_fits(M, tmp_path, capsys):
    H, W = H0, W0
    img = np.stack([O.phantom(H, W, 1 + c) for c in range(3)]).astype(np.float32)
    # the batch function on arrays at the non-square size of the other tests (generic levels) ...
    jobs = [dict(img=img, temp=t, sigma=0.05) for t in (1e-6, 2e-6)]
    own = (O.uniform_fill(9, 5, 0, 0, H * W).reshape(1, H, W) > 0.25).astype(np.float32)      # run_params' mask reaches the jobs that carry none
    r = M.runner.run_inpaint_batch(jobs, mask=own, num_iter=20, lr=2e-3, seed=1, input_depth=8, show_every=5, save=True, net_kwargs=NET_KW,
                                   save_path=str(tmp_path / "direct"), autotune=False)
    assert len(r["psnr"]) == 2 and all(np.isfinite(r["psnr"]))
    # ... and the command line: phantom images of the --imsize square, the two candidates of the config as one batch
    cfg = dict(bo_params=dict(temp=dict(candidates=[1e-6, 2e-6]), sigma=dict(candidates=[0.05])),
               run_params=dict(img="phantom", num_iter=20, lr=2e-3, seed=1, input_depth=8, show_every=5, plot=False, save=True, net_kwargs=NET_KW,
                               save_path=str(tmp_path / "logs")))
    path = str(tmp_path / "cfg.json")
    json.dump(cfg, open(path, "w"))
    res = M.runner.main(["--task", "inpainting", "--config", path, "--imsize", "32", "--inpaint-fits", "4"])
    assert [i for i, _, _ in res] == [0, 1] and all(np.isfinite(y) for _, _, y in res)                 # the table has one row per fit
    assert [(j["temp"], j["sigma"]) for _, j, _ in res] == [(1e-6, 0.05), (2e-6, 0.05)]
    assert "2 fits in 1 batches of up to 4" in capsys.readouterr().out
    for root, F, (h, w), image in ((str(tmp_path / "logs"), 2, (32, 32), None), (str(tmp_path / "direct"), 2, (H, W), img)):
        dirs = os.listdir(root)
        assert len(dirs) == 1
        z = np.load(os.path.join(root, dirs[0], "batch.npz"))
        assert set(z.files) == {"task", "temp", "sigma", "lr", "prior_sigma", "K", "seed", "num_iter", "iterations", "psnr_gt_sm", "nll", "kl", "recon", "dead",
                                "mask", "ale"}
        assert str(z["task"]) == "inp" and list(z["iterations"]) == [0, 5, 10, 15, 20]
        assert z["psnr_gt_sm"].shape == z["nll"].shape == z["kl"].shape == (5, F) and not z["dead"].any()
        assert z["recon"].shape == (F, 3, h, w) and z["ale"].shape == (F, h, w) and z["mask"].shape == (F, 1, h, w)
        assert np.isfinite(z["psnr_gt_sm"]).all() and z["recon"].min() >= 0.0 and z["recon"].max() <= 1.0
        if image is None:
            image = np.stack([M.runner._load_image("phantom", (h, w), 1 + c) for c in range(3)]).astype(np.float32)
        assert np.array_equal(z["mask"][0], M.runner.scratch_mask(h, w, 1) if root.endswith("logs") else own) and np.array_equal(z["mask"][1], z["mask"][0])
        # psnr_gt_sm[-1] is InpaintBatch.psnr of the saved reconstruction: recomputed from recon, mask and the image
        ib = M.InpaintBatch(h, w, F, K=1, input_depth=8, net_kwargs=NET_KW, autotune=False)
        ib.set_targets(torch.from_numpy(np.stack([image] * F)), torch.from_numpy(z["mask"]))
        ib.ema[:, :3].copy_(torch.from_numpy(z["recon"]))
        again = ib.psnr(image)
        assert np.abs(again - z["psnr_gt_sm"][-1]).max() < 1e-4, (again, z["psnr_gt_sm"][-1])
