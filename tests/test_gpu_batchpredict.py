"""Batched posterior predictive: the fits kernels of csrc/predictive.hip bit for bit against the single-fit entry
points and against a numpy restatement of uncert_regression_gal, the plan's sample stride against single-fit forwards, predict() of the
four batch classes against to_engine(f).predict(), state left alone, a dead fit, and the runner's predictive_batch.npz."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))
NET_B = dict(nd=(16, 32, 64), nu=(16, 32, 64), ns=(4, 4, 4))
INP_KW = dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(0, 0, 0))
X6, SM = 1 << 25, 1 | 1 << 26
MODES = [("raw", 3), ("logprec", 2), ("inp", 4), ("mean_only", 1)]
MAPS = ("mean", "epi", "ale", "total", "err2", "mse_mc")
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    assert torch.cuda.is_available()
    M_._lib.lib()
    return M_


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def bn_values(prog, seed, f):
    """gamma = 1 + 0.2 u, beta = 0.1 u, u ~ U[0,1) seeded per fit (at initialisation every fit has gamma = 1, beta = 0)."""
    u = O.uniform_fill(seed, 7, f, 0, prog.n_bn).astype(np.float32)
    bn = np.zeros(prog.n_bn, np.float32)
    for b in prog.bns:
        o, c = b["off"], b["C"]
        bn[o:o + c] = 1.0 + 0.2 * u[o:o + c]
        bn[o + c:o + 2 * c] = 0.1 * u[o + c:o + 2 * c]
    return bn


def write_bn(batch, seed):
    for f in range(batch.params.shape[0]):
        batch.fit(f)["bn"].copy_(dev(bn_values(batch.prog, seed, f)))


# ---- 1. kernels ------------------------------------------------------------------------------------------------------------------------------
def synth(n, C, H, W, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(0.5, 0.4, size=(1, C, H, W)) + rng.normal(scale=0.15, size=(n, C, H, W))).astype(np.float32)      # some values outside [0, 1]


def fits_stats(M, calls, F, S, C, H, W, mode, clip, N, ref, ref_stride, pad=24):
    """calls: [(out [F * S, C, H, W] device tensor, n_use)] -> (dict of host maps stacked over the fits, sums [F, 4]); asserts that the words
    between the accumulator rows keep their sentinel."""
    from mfvi_dip_mia_amd.predictive import image_channels, mode_code
    L, lib = M._lib, M._lib.lib()
    code = mode_code(mode)
    cimg, has_ale = image_channels(C, mode)
    need = lib.mfvi_predictive_acc_doubles_fits(C, H, W, code)
    assert need == lib.mfvi_predictive_acc_doubles(C, H, W, code) + 256          # the state part first, then one more word per finalize block
    stride = need + pad
    acc = torch.full((F, stride), SENTINEL, dtype=torch.float64, device="cuda")
    for i, (y, n_use) in enumerate(calls):
        L.check(lib.mfvi_predictive_accumulate_fits(L.ptr(y), F, S, n_use, C, H, W, code, int(clip), int(i == 0), L.ptr(acc), stride, L.stream_ptr()))
    t = {k: torch.full((F, cimg if k == "mean" else 1, H, W), SENTINEL, dtype=torch.float32, device="cuda") for k in MAPS}
    sums = torch.full((F, 4), SENTINEL, dtype=torch.float64, device="cuda")
    L.check(lib.mfvi_predictive_finalize_fits(L.ptr(acc), stride, F, N, C, H, W, code, L.ptr(ref), ref_stride, L.ptr(t["mean"]), L.ptr(t["epi"]),
                                              L.ptr(t["ale"]) if has_ale else None, L.ptr(t["total"]), L.ptr(t["err2"]) if ref is not None else None,
                                              L.ptr(t["mse_mc"]) if ref is not None else None, L.ptr(sums), L.stream_ptr()))
    assert bool((acc[:, need:] == SENTINEL).all()), "words between the accumulator rows were written"
    got = {k: host(v) for k, v in t.items()}
    if not has_ale:
        assert (got["ale"] == SENTINEL).all()
    if ref is None:
        assert (got["err2"] == SENTINEL).all() and (got["mse_mc"] == SENTINEL).all()
    return got, host(sums)


def single_stats(M, draws, C, H, W, mode, clip, ref):
    """The single-fit entry points on one fit's draws [N, C, H, W] (one call)."""
    from mfvi_dip_mia_amd.predictive import Accumulator
    acc = Accumulator(C, H, W, mode)
    acc.add(draws, draws.shape[0], clip)
    return {k: host(v) for k, v in acc.finalize(draws.shape[0], ref).items()}


KERNEL_CASES = {                    # (H, W), S, [n_use per call]
    "scalar": ((5, 7), 11, [11]),                 # H * W odd: scalar loads; 11 samples: one load group of 8 and a partial one
    "vector-partial": ((8, 16), 5, [3]),          # 16-byte loads; a partial chunk, the samples n_use .. S - 1 hold NaN
    "vector-two-calls": ((8, 16), 5, [5, 3]),     # first = 1 then first = 0 against ONE single-fit call over the concatenation
}


@pytest.mark.parametrize("case", sorted(KERNEL_CASES))
@pytest.mark.parametrize("mode,C", MODES)
@pytest.mark.parametrize("clip", [False, True])
def test_fits_kernels_bit_equal_single_fit(M, case, mode, C, clip):
    from mfvi_dip_mia_amd.predictive import image_channels
    (H, W), S, uses = KERNEL_CASES[case]
    F = 3
    cimg, has_ale = image_channels(C, mode)
    ys = []
    for i, n_use in enumerate(uses):
        y = synth(F * S, C, H, W, seed=17 * C + 3 * i + clip).reshape(F, S, C, H, W)
        y[:, n_use:] = np.nan                                                  # must not be read
        ys.append(y)
    calls = [(dev(y.reshape(F * S, C, H, W)), n_use) for y, n_use in zip(ys, uses)]
    draws = [dev(np.concatenate([y[f, :n_use] for y, n_use in zip(ys, uses)])) for f in range(F)]
    N = sum(uses)
    refs = np.random.default_rng(5).uniform(0, 1, size=(F, cimg, H, W)).astype(np.float32)
    d_refs = dev(refs)
    for kind in ("none", "shared", "per_fit"):
        ref, ref_stride = {"none": (None, 0), "shared": (d_refs[1], 0), "per_fit": (d_refs, cimg * H * W)}[kind]
        got, sums = fits_stats(M, calls, F, S, C, H, W, mode, clip, N, ref, ref_stride)
        for f in range(F):
            want = single_stats(M, draws[f], C, H, W, mode, clip, None if kind == "none" else (d_refs[1] if kind == "shared" else d_refs[f]))
            for k in MAPS:
                if want[k] is None:
                    continue
                assert np.isfinite(want[k]).all(), (kind, f, k)
                assert np.array_equal(got[k][f].reshape(want[k].shape), want[k]), (kind, f, k)
            assert np.array_equal(sums[f, :3], want["sums"]), (kind, f, sums[f], want["sums"])
            if kind == "none":
                assert sums[f, 3] == 0.0
            else:
                s = got["err2"][f].astype(np.float64).sum()
                assert abs(sums[f, 3] - s) <= 1e-12 * abs(s), (kind, f, sums[f, 3], s)
    again, sums2 = fits_stats(M, calls, F, S, C, H, W, mode, clip, N, d_refs, cimg * H * W)      # bit-identical from call to call
    assert all(np.array_equal(again[k], got[k]) for k in MAPS) and np.array_equal(sums2, sums)


def gal_numpy(img_list, reduction):
    """BayTorch/inference/utils.py:11-24 uncert_regression_gal, line by line in float64 numpy."""
    x = np.concatenate(img_list, axis=0).astype(np.float64)                   # torch.cat(img_list, dim=0)
    mean = x[:, :-1].mean(axis=0, keepdims=True)
    ale = x[:, -1:].mean(axis=0, keepdims=True)
    epi = x[:, :-1].var(axis=0, ddof=1, keepdims=True)                          # torch.var: unbiased
    epi = epi.mean(axis=1, keepdims=True)
    uncert = ale + epi
    if reduction == "mean":
        return ale.mean(), epi.mean(), uncert.mean()
    if reduction == "sum":
        return ale.sum(), epi.sum(), uncert.sum()
    return ale, epi, uncert, mean


def test_fits_kernels_vs_uncert_regression_gal_restatement(M):
    """The scalar case in mode raw (the reference's input: the last channel already a variance) against the fp64 restatement, under the
    bounds tests/test_gpu_predictive.py holds the single-fit kernels to: 2e-6 relative on every map and on the sums."""
    (H, W), S, _ = KERNEL_CASES["scalar"]
    F, C = 3, 3
    y = synth(F * S, C, H, W, seed=91)
    got, sums = fits_stats(M, [(dev(y), S)], F, S, C, H, W, "raw", False, S, None, 0)
    for f in range(F):
        imgs = [y[f * S + k:f * S + k + 1] for k in range(S)]
        ale, epi, unc, mean = gal_numpy(imgs, "none")
        for k, want in (("ale", ale), ("epi", epi), ("total", unc)):
            e = relerr(got[k][f], want[0])
            print("fit %d %s: %.2e" % (f, k, e))
            assert e < 2e-6, (f, k, e)
        assert relerr(got["mean"][f], mean[0]) < 2e-6
        for red, scale in (("sum", 1.0), ("mean", 1.0 / (H * W))):
            e = relerr(sums[f, :3] * scale, np.array(gal_numpy(imgs, red)))
            assert e < 2e-6, (f, red, e)


def test_fits_kernels_refuse_bad_arguments(M):
    L, lib = M._lib, M._lib.lib()
    assert lib.mfvi_predictive_acc_doubles_fits(3, 8, 8, L.PRED_LOGPREC) == -1
    need = lib.mfvi_predictive_acc_doubles_fits(2, 8, 8, L.PRED_LOGPREC)
    y = torch.zeros((6, 2, 8, 8), device="cuda"); acc = torch.zeros((3, need), dtype=torch.float64, device="cuda")
    sp = L.stream_ptr()
    for F, S, n_use, stride in ((3, 2, 3, need), (3, 2, 0, need), (0, 2, 1, need), (3, 2, 2, need - 1), (65536, 1, 1, need), (256, 256, 1, need)):
        assert lib.mfvi_predictive_accumulate_fits(L.ptr(y), F, S, n_use, 2, 8, 8, L.PRED_LOGPREC, 0, 1, L.ptr(acc), stride, sp) == -1, (F, S, n_use, stride)
        assert b"predictive_accumulate_fits" in lib.mfvi_last_error()
    m = torch.zeros((3, 8, 8), device="cuda"); s4 = torch.zeros((3, 4), dtype=torch.float64, device="cuda")
    p = L.ptr(m)
    for F, N, stride, rs, ale in ((3, 1, need, 0, p), (0, 2, need, 0, p), (3, 2, need - 1, 0, p), (3, 2, need, 63, p), (3, 2, need, 0, None)):
        assert lib.mfvi_predictive_finalize_fits(L.ptr(acc), stride, F, N, 2, 8, 8, L.PRED_LOGPREC, p, rs, p, p, ale, p, p, p, L.ptr(s4), sp) == -1, (F, N, stride, rs)
        assert b"predictive_finalize_fits" in lib.mfvi_last_error()


# ---- 2. plan: the sample stride ----------------------------------------------------------------------------------------------------------------
def pin_net_b(M, plan):
    """The pinned tilings of tests/test_gpu_fitbatch.py::test_plan_fits_mode_matches_single_fit_passes."""
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


def net_b_rows(M, F, seed, **net):
    H = W = 64
    kw = dict(NET_B); kw.update(net)
    P, zin, zout, _ = M.skip_program(H, W, 16, 2, **kw)
    nv = P.n_vi
    n_params = 2 * nv + P.n_bn
    stride = (n_params + 3) // 4 * 4 + 8
    rows = np.zeros((F, stride), np.float32)
    for f in range(F):
        rows[f, :nv] = 0.1 * O.normal_fill(seed, 2, 0, f, 0, nv)
        rows[f, nv:2 * nv] = -3.0 + 0.1 * O.normal_fill(seed, 2, 1, f, 0, nv)
        rows[f, 2 * nv:n_params] = bn_values(P, seed, f)
    z = np.stack([0.1 * O.uniform_fill(seed, 0, f, 0, 16 * H * W).reshape(16, H, W) for f in range(F)]).astype(np.float32)
    return P, zin, zout, nv, n_params, stride, dev(rows), dev(z)


@pytest.mark.parametrize("S", [3, 5])
def test_sample_stride_matches_single_fit_forwards(M, S):
    """out[f * S + s] of a fits-mode forward at k0 = 2 against the single-fit forward of fit f at k0 = 2 + f * stride, n = S, for the strides
    0, 7 and the default (S); bound: relerr < 1e-5 as test_plan_fits_mode_matches_single_fit_passes."""
    F, seed, step, k0 = 3, 31, 5, 2
    P, zin, zout, nv, n_params, stride, rows, z = net_b_rows(M, F, seed)
    ps = P.compile(zin, zout, S); pin_net_b(M, ps)

    def single(f, k):
        r = rows[f]
        return host(ps.forward(r[:nv], r[nv:2 * nv], r[2 * nv:n_params], z[f], seed, step, k, S))
    want = {ks: [single(f, k0 + f * ks) for f in range(F)] for ks in (0, 7, S)}
    for f in range(1, F):      # another fit's sample indices are a different answer by far more than the bound
        e = relerr(want[0][f], want[S][f])
        print("S=%d fit %d: stride 0 against default indices %.2e" % (S, f, e))
        assert e > 100 * 1e-5, (f, e)
    pf = P.compile(zin, zout, F * S); pin_net_b(M, pf); pf.set_fits(S, stride, stride)
    for ks in (S, 0, 7, None):      # None: a set_fits call restores the default
        if ks is None:
            pf.set_fits(S, stride, stride)
        elif ks != S:
            pf.set_fits_sample_stride(ks)
        out = host(pf.forward(rows[0, :nv], rows[0, nv:], rows[0, 2 * nv:], z, seed, step, k0, F * S))
        for f in range(F):
            e = relerr(out[f * S:(f + 1) * S], want[S if ks is None else ks][f])
            print("S=%d stride %s fit %d: %.2e" % (S, ks, f, e))
            assert e < 1e-5, (ks, f, e)


@pytest.mark.parametrize("S", [3, 5])
def test_sample_stride_mc_dropout(M, S):
    """Point weights with per-fit Dropout2d probabilities and stride 0: every fit draws the masks of the samples k0 .. k0 + S - 1, as a
    single-fit plan built with that fit's p does."""
    F, seed, step, k0 = 3, 33, 6, 2
    ps_fit = [0.1, 0.3, 0.0]
    P, zin, zout, nv, n_params, stride, rows, z = net_b_rows(M, F, seed, drop_down=0.3, drop_up=0.3)
    pf = P.compile(zin, zout, F * S); pin_net_b(M, pf)
    pf.set_fits(S, stride, stride); pf.set_fits_points(True); pf.set_fit_dropout(ps_fit); pf.set_fits_sample_stride(0)
    out = host(pf.forward(rows[0, :nv], rows[0, nv:], rows[0, 2 * nv:], z, seed, step, k0, F * S, False))
    for f in range(F):
        Q, qi, qo, nv_q, _, _, _, _ = net_b_rows(M, 1, seed, drop_down=ps_fit[f], drop_up=ps_fit[f])
        assert nv_q == nv
        q = Q.compile(qi, qo, S); pin_net_b(M, q)
        r = rows[f]
        o = host(q.forward(r[:nv], r[nv:2 * nv], r[2 * nv:n_params], z[f], seed, step, k0, S, False))
        e = relerr(out[f * S:(f + 1) * S], o)
        print("S=%d fit %d p=%.1f: %.2e" % (S, f, ps_fit[f], e))
        assert e < 1e-5, (f, e)
        if ps_fit[f] > 0:
            assert not np.array_equal(o[0], o[1])                              # the masks differ from sample to sample


def test_sample_stride_refusals(M):
    """Each refused before any launch: a status and a message, the output and gradient buffers untouched."""
    L, lib = M._lib, M._lib.lib()
    F, S, seed = 2, 2, 3
    P, zin, zout, nv, n_params, stride, rows, z = net_b_rows(M, F, seed)
    pf = P.compile(zin, zout, F * S)
    assert lib.mfvi_plan_set_fits_sample_stride(pf.handle, 0) == -1 and b"not in fits mode" in lib.mfvi_last_error()
    with pytest.raises(L.MfviError):
        pf.set_fits_sample_stride(0)
    pf.set_fits(S, stride, stride)
    assert lib.mfvi_plan_set_fits_sample_stride(pf.handle, -1) == -1 and b"negative" in lib.mfvi_last_error()
    assert lib.mfvi_plan_set_fits_sample_stride(None, 0) == -1
    pf.set_fits_sample_stride(0)
    out = pf.forward(rows[0, :nv], rows[0, nv:], rows[0, 2 * nv:], z, seed, 0, 0, F * S)
    dout = torch.ones_like(out)
    g = torch.full((F, stride), SENTINEL, device="cuda")
    ws = pf.workspace.clone()
    with pytest.raises(NotImplementedError, match="forward passes only"):
        pf.backward(rows[0, :nv], rows[0, nv:], rows[0, 2 * nv:], z, seed, 0, 0, F * S, dout, g[0, :nv], g[0, nv:], g[0, 2 * nv:])
    assert bool((g == SENTINEL).all()) and torch.equal(ws, pf.workspace)
    pf.set_fits_sample_stride(S)                                               # the default by value: backward is served again
    g.zero_()
    pf.backward(rows[0, :nv], rows[0, nv:], rows[0, 2 * nv:], z, seed, 0, 0, F * S, dout, g[0, :nv], g[0, nv:], g[0, 2 * nv:])
    pf.set_fits_sample_stride(0); pf.set_fits(S, stride, stride)               # set_fits restores it
    pf.backward(rows[0, :nv], rows[0, nv:], rows[0, 2 * nv:], z, seed, 0, 0, F * S, dout, g[0, :nv], g[0, nv:], g[0, 2 * nv:])
    assert bool(torch.isfinite(g).all())


# ---- 3. predict() of the batch classes against to_engine(f).predict() -------------------------------------------------------------------------
def _hyper(F):
    return [1e-6 * 2 ** f for f in range(F)], [0.05 * 2 ** f for f in range(F)], [1e-3 * (f + 1) for f in range(F)]


def raw_draws_max(eng, N, chunk):
    """max |y| over the N raw outputs eng.predict(N, chunk=chunk) reduces (the same plan, counters and input)."""
    from mfvi_dip_mia_amd.predictive import DEFAULT_STEP
    plan, out = eng._pred_plan(chunk)
    m = 0.0
    for c0 in range(0, N, chunk):
        n = min(chunk, N - c0)
        plan.forward(eng.mu, eng.rho, eng.bn, eng.z0, eng.seed, DEFAULT_STEP, c0, n, eng.sample_weights, out)
        m = max(m, float(out[:n].abs().max()))
    return m


def map_bounds(ref, delta):
    """Per-pixel bounds on |batched - single| for every map, from raw outputs that differ by at most delta = 1e-5 max|y_ref| (the project's
    bound for the same arithmetic in another order; the transforms id, sigmoid and exp(-y) on [0, 1]-scale values do not amplify it):
      mean   2 delta
      ale    2 delta ale_ref + 1e-7
      epi    6 delta sqrt(epi_ref) + 8 delta^2        the unbiased variance of N >= 2 values each moved by at most delta: with d_k the moves,
                                                      |var' - var| <= 2 sqrt(var) sqrt(N/(N-1)) 2 delta + N/(N-1) 4 delta^2, N/(N-1) <= 2
      total  ale + epi
      err2   4 delta sqrt(err2_ref) + 4 delta^2       (a + d)^2 - a^2 with |d| <= 2 delta, a^2 = err2 (mean over channels: Cauchy-Schwarz)
      mse_mc err2 + epi"""
    b = dict(mean=np.full_like(ref["mean"], 2 * delta, dtype=np.float64))
    b["epi"] = 6 * delta * np.sqrt(ref["epi"].astype(np.float64)) + 8 * delta ** 2
    if ref["ale"] is not None:
        b["ale"] = 2 * delta * ref["ale"].astype(np.float64) + 1e-7
    b["total"] = b["epi"] + (b["ale"] if ref["ale"] is not None else 0.0)
    if ref["err2"] is not None:
        b["err2"] = 4 * delta * np.sqrt(ref["err2"].astype(np.float64)) + 4 * delta ** 2
        b["mse_mc"] = b["err2"] + b["epi"]
    return b


def check_against_engines(batch, r, N, chunk, targets, what, calibration=None, refs=None):
    """Every fit's maps of r against batch.to_engine(f, autotune=False).predict(N, target, chunk); -> the single-fit results (reusable)."""
    F = r["mean"].shape[0]
    refs = refs or []
    for f in range(F):
        if len(refs) <= f:
            eng = batch.to_engine(f, autotune=False)
            s = eng.predict(N, target=None if targets is None else targets[f], chunk=chunk, calibration=calibration)
            s = {k: (host(v) if torch.is_tensor(v) else v) for k, v in s.items()}
            s["delta"] = 1e-5 * raw_draws_max(eng, N, chunk)
            refs.append(s)
        s = refs[f]
        bounds = map_bounds(s, s["delta"])
        for k in MAPS:
            if s[k] is None:
                assert r[k] is None, (what, k)
                continue
            got = host(r[k][f]).reshape(s[k].shape)
            d = np.abs(got.astype(np.float64) - s[k])
            worst = float((d / bounds[k]).max())
            print("%s fit %d %-6s max |diff| %.2e, largest diff / bound %.3f" % (what, f, k, d.max(), worst))
            assert worst <= 1.0, (what, f, k, worst)
        assert r["n"] == s["n"] == N and r["step"] == s["step"]
    return refs


def check_calibration_counts(r, refs, n_bins):
    """Equal bin counts, except where a pixel's total lies within its bound of a bin edge (it may fall either side); at most 1 % of the pixels
    may be excused that way, a cap the single-fit reference alone decides."""
    for f, s in enumerate(refs):
        c, cs = r["calibration"][f], s["calibration"]
        edges = host(cs["bounds"]).astype(np.float64)
        tol = map_bounds(s, s["delta"])["total"].reshape(-1) + np.abs(edges).max() * 2.0 ** -23      # (+ the edges' own fp32 rounding)
        tot = s["total"].astype(np.float64).reshape(-1)
        near = (np.abs(tot[:, None] - edges[None, :]) <= tol[:, None]).any(axis=1)
        print("calibration fit %d: %d of %d pixels within their bound of a bin edge" % (f, near.sum(), near.size))
        assert near.sum() <= 0.01 * near.size, (f, int(near.sum()))
        moved = np.abs(host(c["count"]) - host(cs["count"])).sum()
        assert moved <= 2 * near.sum(), (f, host(c["count"]), host(cs["count"]))
        assert host(c["count"]).shape == (n_bins,) and int(c["n"]) == int(cs["n"])


@pytest.fixture(scope="module")
def den_batch(M):
    """32x32 denoising, F = 3, K = 1, distinct temp / sigma / lr and BatchNorm parameters, two steps; with the single-fit references."""
    H = W = 32; F, seed = 3, 6
    temps, sigmas, lrs = _hyper(F)
    fb = M.FitBatch(H, W, F, task="den", K=1, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
    write_bn(fb, seed)
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)]).astype(np.float32)
    fb.set_targets(torch.from_numpy(np.stack([O.noisy(g, 0.1, seed + f) for f, g in enumerate(gt)]).astype(np.float32)))
    fb.step(); fb.step()
    return fb, torch.from_numpy(gt), []


def test_fitbatch_predict_matches_engines(M, den_batch):
    fb, gt, refs = den_batch
    N = 7
    r = fb.predict(N, target=gt, chunk=3, calibration=dict(n_bins=5))
    assert tuple(r["mean"].shape) == (3, 1, 32, 32) and all(tuple(r[k].shape) == (3, 32, 32) for k in MAPS[1:])
    refs.extend(check_against_engines(fb, r, N, 3, gt, "den", calibration=dict(n_bins=5)))
    check_calibration_counts(r, refs, 5)
    assert list(r["dead"]) == [0, 0, 0]
    psnr = 10 * np.log10(1.0 / host(r["err2"]).astype(np.float64).mean(axis=(1, 2)))
    assert relerr(r["psnr_mean"], psnr) < 1e-9
    for kw in (dict(chunk=3, fits_per_call=2), dict(chunk=7), dict()):
        check_against_engines(fb, fb.predict(N, target=gt, **kw), N, 3, gt, "den %s" % (kw,), refs=refs)
    a, b = fb.predict(N, target=gt, chunk=3), fb.predict(N, target=gt, chunk=3)
    assert all(torch.equal(a[k], b[k]) for k in MAPS) and all(torch.equal(a[k], r[k]) for k in MAPS)
    shared = fb.predict(N, target=gt[1], chunk=3)                              # one ground truth for all fits
    assert torch.equal(shared["err2"][1], r["err2"][1]) and torch.equal(shared["mean"], r["mean"]) and not torch.equal(shared["err2"][0], r["err2"][0])
    none = fb.predict(N, chunk=3)
    assert none["err2"] is None and none["mse_mc"] is None and none["psnr_mean"] is None and torch.equal(none["total"], r["total"])


def test_predict_leaves_the_batch_alone(M, den_batch):
    """A predict between two steps: the second step's losses and parameters are those of a run without it."""
    fb, gt, _ = den_batch
    H = W = 32; F, seed = 3, 6
    temps, sigmas, lrs = _hyper(F)
    runs = []
    for with_predict in (False, True):
        b = M.FitBatch(H, W, F, task="den", K=1, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
        write_bn(b, seed); b.set_targets(fb.targets.clone())
        b.step()
        if with_predict:
            b.recon()                                                          # (waits for the side stream's EMA of the step)
            snap = [host(x).copy() for x in (b.params, b.m, b.v, b.out, b.ema)]
            b.predict(5, target=gt, chunk=2, calibration=True)
            assert all(np.array_equal(s, host(x)) for s, x in zip(snap, (b.params, b.m, b.v, b.out, b.ema))) and b.t == 1
        b.step()
        runs.append((b.losses(), host(b.params).copy()))
    for x, y in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(x, y)
    assert np.array_equal(runs[0][1], runs[1][1])


def test_fitbatch_sr_predict_matches_engines(M):
    H = W = 32; F, seed, N = 3, 8, 7
    temps, sigmas, lrs = _hyper(F)
    fb = M.FitBatch(H, W, F, task="sr", K=1, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, sr_factor=4, net_kwargs=SMALL, autotune=False)
    write_bn(fb, seed)
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)]).astype(np.float32)
    fb.set_targets(torch.from_numpy(np.ascontiguousarray(gt[:, ::4, ::4])))
    fb.step(); fb.step()
    check_against_engines(fb, fb.predict(N, target=torch.from_numpy(gt), chunk=3), N, 3, torch.from_numpy(gt), "sr")


def test_ctvolume_predict_matches_engines(M):
    S, D, seed, N = 32, 3, 9, 7
    temps, sigmas, lrs = _hyper(D)
    vol = M.CtVolume(S, D, slices_per_launch=2, K=1, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
    write_bn(vol, seed)
    gt = np.stack([O.phantom(S, S, seed + d) for d in range(D)]).astype(np.float32)
    vol.set_volume(torch.from_numpy(gt))
    vol.step(); vol.step()
    r = vol.predict(N, target=torch.from_numpy(gt), chunk=3)                   # groups of 2 and 1 slices
    assert r["ale"] is None and torch.equal(r["total"], r["epi"]) and tuple(r["mean"].shape) == (D, 1, S, S)
    refs = check_against_engines(vol, r, N, 3, torch.from_numpy(gt), "ct")
    check_against_engines(vol, vol.predict(N, target=torch.from_numpy(gt), chunk=3, fits_per_call=3), N, 3, torch.from_numpy(gt), "ct G=3", refs=refs)


@pytest.mark.parametrize("hw", [(32, 32), (24, 40)])      # 24 x 40: the deep maps are 10 and 5 wide, their layers draw eps inside the generic kernels
def test_inpaintbatch_predict_matches_engines(M, hw):
    H, W = hw
    F, seed, N = 2, 10, 7
    temps, sigmas, lrs = _hyper(F)
    ib = M.InpaintBatch(H, W, F, K=1, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=INP_KW, autotune=False)
    write_bn(ib, seed)
    img = np.stack([np.stack([O.phantom(H, W, seed + 3 * f + c) for c in range(3)]) for f in range(F)]).astype(np.float32)
    mask = (np.random.default_rng(seed).uniform(size=(F, 1, H, W)) > 0.3).astype(np.float32)
    ib.set_targets(torch.from_numpy(img), torch.from_numpy(mask))
    ib.step(); ib.step()
    r = ib.predict(N, target=torch.from_numpy(img), chunk=3)
    assert tuple(r["mean"].shape) == (F, 3, H, W) and tuple(r["ale"].shape) == (F, H, W)
    plan = ib._predict_plans[(F, 3)][0]
    fam = {M._lib.lib().mfvi_plan_last_kernel(plan.handle, i, 0) for i, o in enumerate(plan.prog.ops) if o["type"] == M._lib.OP_CONV}
    assert (0 in fam) == (W == 40) and any(x > 0 for x in fam), fam             # family 0: the generic kernels
    check_against_engines(ib, r, N, 3, torch.from_numpy(img), "inp %dx%d" % hw)
    shared = ib.predict(N, target=torch.from_numpy(img[1]), chunk=3)           # [3, H, W]: shared
    assert torch.equal(shared["err2"][1], r["err2"][1])


def test_siblingbatch_predict_matches_engines(M):
    H = W = 32; F, seed, N = 3, 11, 7
    kw = dict(task="den", K=1, input_depth=8, lr=[1e-3, 5e-4, 7.5e-4], weight_decay=[0.0, 1.0, 2.0], seed=seed, net_kwargs=SMALL, autotune=False)
    sb = M.SiblingBatch(H, W, F, "mcd", dropout_p=[0.1, 0.3, 0.5], **kw)
    write_bn(sb, seed)
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)]).astype(np.float32)
    tg = torch.from_numpy(np.stack([O.noisy(g, 0.1, seed + f) for f, g in enumerate(gt)]).astype(np.float32))
    sb.set_targets(tg)
    sb.step(); sb.step()
    r = sb.predict(N, target=torch.from_numpy(gt), chunk=3)
    refs = check_against_engines(sb, r, N, 3, torch.from_numpy(gt), "mcd")
    check_against_engines(sb, sb.predict(N, target=torch.from_numpy(gt), chunk=2, fits_per_call=2), N, 3, torch.from_numpy(gt), "mcd G=2", refs=refs)
    assert float(r["epi"].min()) >= 0 and float(r["epi"].max()) > 0          # the masks move the output
    with pytest.raises(ValueError, match="deterministic"):
        M.SiblingBatch(H, W, 2, "dip", **dict(kw, lr=1e-3, weight_decay=0.0)).predict(4)
    with pytest.raises(NotImplementedError, match="iterates"):
        M.SiblingBatch(H, W, 2, "sgld", **dict(kw, lr=1e-3, weight_decay=0.0)).predict(4)


def test_dead_fit_is_predicted_and_flagged(M):
    """The recipe of test_nan_fit_is_isolated: fit 1 meets a NaN target and freezes.  It is flagged and still predicted (finite maps from its
    frozen parameters), and every fit's maps -- the live ones beside a dead neighbour included -- are their stand-alone engine's, under the
    bounds of the other comparisons.  (Two separately trained batches are not compared bit for bit: the fp64 BatchNorm atomics of training
    reorder from run to run.)"""
    H = W = 32; F, K, seed = 3, 2, 12
    temps, sigmas, lrs = _hyper(F)
    gt = np.stack([O.phantom(H, W, seed + f) for f in range(F)]).astype(np.float32)
    bad = np.stack([O.noisy(g, 0.1, seed + f) for f, g in enumerate(gt)]).astype(np.float32)
    bad[1, 5, 7] = np.nan
    fb = M.FitBatch(H, W, F, task="den", K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
    write_bn(fb, seed); fb.set_targets(torch.from_numpy(bad))
    frozen = host(fb.fit(1)["params"]).copy()
    fb.step(); fb.step()
    r = fb.predict(5, target=torch.from_numpy(gt), chunk=2)
    assert list(r["dead"]) == [0, 1, 0] and np.array_equal(host(fb.fit(1)["params"]), frozen)
    assert all(bool(torch.isfinite(r[k]).all()) for k in MAPS) and np.isfinite(r["psnr_mean"]).all()
    check_against_engines(fb, r, 5, 2, torch.from_numpy(gt), "dead")
    # the live fits' maps do not depend on what the row of fit 1 holds: the same rows 0 and 2 beside a live neighbour, bit for bit
    other = M.FitBatch(H, W, F, task="den", K=K, input_depth=8, temp=temps, sigma=sigmas, lr=lrs, seed=seed, net_kwargs=SMALL, autotune=False)
    other.params.copy_(fb.params); other.fit(1)["params"].copy_(fb.fit(0)["params"])
    assert torch.equal(other.z0, fb.z0)
    ro = other.predict(5, target=torch.from_numpy(gt), chunk=2)
    for f in (0, 2):
        assert all(torch.equal(ro[k][f], r[k][f]) for k in MAPS), f
    assert not torch.equal(ro["mean"][1], r["mean"][1]) and list(ro["dead"]) == [0, 0, 0]


# ---- 4. runner ---------------------------------------------------------------------------------------------------------------------------------
def test_runner_batch_predict_fits_per_launch(M, tmp_path):
    cfg = dict(bo_params=dict(temp=dict(candidates=[1e-6, 2e-6, 4e-6]), sigma=dict(candidates=[0.05])),
               run_params=dict(img="phantom", num_iter=2, lr=1e-3, seed=1, p_sigma=0.1, input_depth=8, show_every=5, plot=False, save=True,
                               net_kwargs=SMALL, autotune=False, save_path=str(tmp_path / "logs")))
    path = str(tmp_path / "cfg.json")
    json.dump(cfg, open(path, "w"))
    res = M.runner.main(["--task", "denoising", "--config", path, "--imsize", "32", "--fits-per-launch", "3", "--batch-predict-samples", "4",
                         "--batch-calibration", "--calibration-bins", "5"])
    assert len(res) == 3
    (d,) = os.listdir(str(tmp_path / "logs"))
    run = os.path.join(str(tmp_path / "logs"), d)
    assert sorted(os.listdir(run)) == ["batch.npz", "calibration_batch.npz", "predictive_batch.npz"]
    z = np.load(os.path.join(run, "predictive_batch.npz"))
    assert set(z.files) == {"mean", "epi", "ale", "total", "err2", "mse_mc", "psnr_mean", "n", "step", "dead"}
    assert z["mean"].shape == (3, 1, 32, 32) and all(z[k].shape == (3, 32, 32) for k in ("epi", "ale", "total", "err2", "mse_mc"))
    assert z["psnr_mean"].shape == (3,) and int(z["n"]) == 4 and int(z["step"]) == 2 ** 31 and list(z["dead"]) == [0, 0, 0]
    assert all(np.isfinite(z[k]).all() for k in z.files)
    c = np.load(os.path.join(run, "calibration_batch.npz"))
    assert set(c.files) == {"pred_" + k for k in ("bounds", "count", "prop_in_bin", "err_in_bin", "uncert_in_bin", "uce", "uce_1e-4", "U")}
    assert c["pred_bounds"].shape == (3, 6) and c["pred_count"].shape == (3, 5) and c["pred_uce"].reshape(3, -1).shape == (3, 1)


def test_runner_batch_predict_ct_volume(M, tmp_path):
    cfg = dict(bo_params=dict(temp=dict(candidates=[1e-6]), sigma=dict(candidates=[0.05])),
               run_params=dict(num_iter=2, lr=1e-3, seed=1, input_depth=8, show_every=5, plot=False, save=True, net_kwargs=SMALL, autotune=False,
                               save_path=str(tmp_path / "logs")))
    path = str(tmp_path / "cfg.json")
    json.dump(cfg, open(path, "w"))
    M.runner.main(["--task", "ct", "--config", path, "--imsize", "32", "--ct-volume", "phantom:3", "--slices-per-launch", "2", "--batch-predict-samples", "4"])
    (d,) = os.listdir(str(tmp_path / "logs"))
    run = os.path.join(str(tmp_path / "logs"), d)
    assert sorted(os.listdir(run)) == ["predictive_batch.npz", "volume.npz"]
    z = np.load(os.path.join(run, "predictive_batch.npz"))
    assert set(z.files) == {"mean", "epi", "total", "err2", "mse_mc", "psnr_mean", "n", "step", "dead"}      # CT: no aleatoric map
    assert z["mean"].shape == (3, 1, 32, 32) and z["epi"].shape == (3, 32, 32) and np.array_equal(z["epi"], z["total"])
    assert int(z["n"]) == 4 and list(z["dead"]) == [0, 0, 0] and np.isfinite(z["psnr_mean"]).all()
