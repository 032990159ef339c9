"""The total-variation term on the GPU: mfvi_tv_term against the float64 restatement (tests/tv_restatement.py) on
every case of tests/golden/tv.npz, its call-level properties, the drop-in tv_loss, the term inside ElboEngine / SiblingEngine (eager,
device-resident and replayed from a graph), inside FitBatch / CtVolume / SiblingBatch, and in the runners' artefacts.

Tolerance 1e-5 (value: relative; gradient: against its largest magnitude): the bar tests/test_gpu_downsampler.py holds the Lanczos data
term's dout to against its float64 restatement -- per cell a handful of fp32 operations and one rsqrt / powf, sums in fp64."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tv_restatement as R
from conftest import note_margin
from oracle import oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 1e-5
SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))          # the two-scale net of tests/test_gpu_downsampler.py
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M
    M._lib.lib()
    return M


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "tv.npz"))
    cases = []
    for name in g["cases"]:
        shape, beta = str(name).split("_b")
        cases.append((str(name), g["x_" + shape], float(beta), float(g[name + "_val32"])))
    return cases, g


def relerr(got, want, what):
    """max |got - want| / max |want| (absolute where the reference is all zero), on record in the parity-margins file."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    e = float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)) if want.any() else float(np.abs(got).max())
    note_margin(e, what)
    return e


def term(M, out, n_fits, S, channel=0, beta=0.5, weight=None, stride=0, grad_scale=1.0, accumulate=0, dout="new", tv="new", scratch="new"):
    """One mfvi_tv_term call -> (rc, dout, tv); "new": a zero-filled buffer, None: NULL."""
    L = M._lib
    n, C, H, W = out.shape
    if weight is None:
        weight = torch.ones(1, device="cuda")
    if isinstance(dout, str):
        dout = torch.zeros_like(out)
    if isinstance(tv, str):
        tv = torch.zeros(n_fits, dtype=torch.float64, device="cuda")
    if isinstance(scratch, str):
        scratch = torch.empty(max(L.lib().mfvi_tv_term_scratch_bytes(n_fits, S, H, W), 8), dtype=torch.uint8, device="cuda")
    rc = L.lib().mfvi_tv_term(L.ptr(out), n_fits, S, C, H, W, channel, beta, L.ptr(weight), stride, grad_scale, accumulate, L.ptr(dout), L.ptr(tv),
                              L.ptr(scratch), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, dout, tv


def host(t):
    return t.detach().cpu().numpy()


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------------------------------
def test_tv_term_matches_the_restatement_on_every_golden_case(M, golden):
    cases, g = golden
    assert len(cases) == 11
    for name, x, beta, val32 in cases:
        N, C, H, W = x.shape
        xd = torch.from_numpy(x).cuda().view(N * C, 1, H, W)            # the drop-in's shape of a call: n_fits = N C, S = 1, C = 1
        rc, dout, tv = term(M, xd, N * C, 1, beta=beta)
        assert rc == 0, M._lib.lib().mfvi_last_error()
        want_v, want_g = R.tv_planes(x, beta).reshape(-1), R.tv_grad(x, beta).reshape(N * C, 1, H, W)
        ev, eg = relerr(host(tv), want_v, "tv value"), relerr(host(dout), want_g, "tv gradient")
        e32 = abs(host(tv).sum() - val32) / max(abs(val32), 1e-30) if val32 else abs(host(tv).sum())
        print("%-22s value %.2e  gradient %.2e  against the reference's fp32 value %.2e" % (name, ev, eg, e32))
        assert ev < TOL and eg < TOL and e32 < TOL, name
        assert not host(dout)[:, 0, -1, -1].any(), name                 # the corner pixel touches no cell
        # the same planes as ONE fit of N C samples, a two-channel layout with the term on channel 1
        two = torch.full((N * C, 2, H, W), 7.0, device="cuda")
        two[:, 1] = xd[:, 0]
        rc, d2, tv2 = term(M, two, 1, N * C, channel=1, beta=beta)
        assert rc == 0
        assert relerr(host(tv2), [want_v.sum()], "tv value") < TOL and torch.equal(d2[:, 1], dout[:, 0]) and not d2[:, 0].any()


def test_tv_term_on_a_flat_patch_is_finite(M, golden):
    _, g = golden
    x = g["flat_x"]
    xd = torch.from_numpy(x).cuda()
    rc, dout, tv = term(M, xd, 1, 1)
    assert rc == 0
    d, want = host(dout), R.tv_grad(x, 0.5)
    assert np.isfinite(d).all() and g["flat_nan"].sum() == 3
    assert not d[want == 0.0].any()
    assert relerr(d, want, "tv gradient") < TOL and relerr(host(tv), [R.tv_value(x, 0.5)], "tv value") < TOL
    assert abs(host(tv)[0] - float(g["flat_val32"])) < TOL * float(g["flat_val32"])
    flat = torch.full((2, 1, 9, 12), 0.25, device="cuda")              # every cell is a zero cell
    for beta in (0.5, 0.75, 1.0, 1.5):
        rc, dout, tv = term(M, flat, 2, 1, beta=beta)
        assert rc == 0 and not dout.any() and not tv.any()


# ---- 2. properties ---------------------------------------------------------------------------------------------------------------------------
def _samples(n, C, H, W, seed):
    return torch.from_numpy(np.random.default_rng(seed).random((n, C, H, W), np.float32)).cuda()


def test_two_calls_are_bit_identical(M):
    out = _samples(6, 2, 33, 130, 1)
    for beta in (0.5, 0.75):
        _, d1, t1 = term(M, out, 3, 2, beta=beta)
        _, d2, t2 = term(M, out, 3, 2, beta=beta)
        assert torch.equal(d1, d2) and (host(t1) == host(t2)).all() and t1.all()
    # tv accumulates: a second call on the same buffer doubles it
    _, _, t3 = term(M, out, 3, 2, tv=t1.clone())
    _, _, t0 = term(M, out, 3, 2)
    assert np.allclose(host(t3), host(t1) + host(t0), rtol=1e-15)


def test_accumulate_and_the_other_channels(M):
    out = _samples(4, 2, 17, 65, 2)
    pattern = _samples(4, 2, 17, 65, 3) - 0.5
    w = torch.tensor([0.7], device="cuda")
    _, g, _ = term(M, out, 2, 2, channel=1, weight=w, grad_scale=0.5)
    assert not g[:, 0].any() and g[:, 1].any()
    assert relerr(host(g[:, 1]), 0.5 * np.float32(0.7) * R.tv_grad(host(out[:, 1])), "tv gradient") < TOL
    _, acc, _ = term(M, out, 2, 2, channel=1, weight=w, grad_scale=0.5, accumulate=1, dout=pattern.clone())
    assert torch.equal(acc[:, 0], pattern[:, 0])                        # untouched
    assert torch.equal(acc[:, 1], pattern[:, 1] + g[:, 1])
    _, over, _ = term(M, out, 2, 2, channel=1, weight=w, grad_scale=0.5, accumulate=0, dout=pattern.clone())
    assert torch.equal(over[:, 0], pattern[:, 0]) and torch.equal(over[:, 1], g[:, 1])


def test_weight_stride(M):
    out = _samples(6, 1, 32, 40, 4)
    ws = torch.tensor([0.5, 2.0, 0.0], device="cuda")
    _, per, tv_per = term(M, out, 3, 2, weight=ws, stride=1)
    _, one, tv_one = term(M, out, 3, 2, weight=ws, stride=0)            # weight[0] for all
    base = term(M, out, 3, 2)[1]
    assert torch.equal(one, base * 0.5) and torch.equal(tv_one, tv_per)  # the value is unweighted
    assert torch.equal(per[:2], base[:2] * 0.5) and torch.equal(per[2:4], base[2:4] * 2.0) and not per[4:].any()
    # accumulate with a weight of exactly 0 leaves that fit's dout alone, to the bit (even where the samples are not finite)
    bad = out.clone(); bad[4:] = float("nan")
    pattern = _samples(6, 1, 32, 40, 5)
    _, acc, _ = term(M, bad, 3, 2, weight=ws, stride=1, accumulate=1, dout=pattern.clone())
    assert torch.equal(acc[4:], pattern[4:]) and torch.equal(acc[:4], pattern[:4] + per[:4])


def test_a_nan_stays_in_its_fit(M):
    out = _samples(6, 2, 17, 65, 6)
    bad = out.clone(); bad[2:4, 0] = float("nan")
    _, d0, t0 = term(M, out, 3, 2)
    _, d1, t1 = term(M, bad, 3, 2)
    assert torch.equal(d1[:2], d0[:2]) and torch.equal(d1[4:], d0[4:])
    assert host(t1)[0] == host(t0)[0] and host(t1)[2] == host(t0)[2]
    assert np.isnan(host(t1)[1]) and torch.isnan(d1[2:4, 0]).any()


def test_null_outputs(M):
    out = _samples(4, 1, 33, 130, 7)
    _, d0, t0 = term(M, out, 2, 2)
    rc, _, t1 = term(M, out, 2, 2, dout=None)
    assert rc == 0 and torch.equal(t1, t0)
    rc, d1, _ = term(M, out, 2, 2, tv=None)
    assert rc == 0 and torch.equal(d1, d0)


def test_refusals(M):
    L = M._lib
    out = _samples(4, 2, 8, 12, 8)
    w = torch.ones(2, device="cuda")
    sentinel = torch.full_like(out, 123.0)
    ok = dict(n_fits=2, S=2, channel=0, beta=0.5, weight=w, stride=1)
    bad = [dict(null_weight=True), dict(scratch=None), dict(dout=None, tv=None), dict(n_fits=0), dict(S=0), dict(n_fits=256, S=256), dict(channel=-1),
           dict(channel=2), dict(beta=0.0), dict(beta=-0.5), dict(beta=float("nan")), dict(beta=float("inf")), dict(stride=2), dict(stride=-1)]
    for kw in bad:
        a = dict(ok); a.update(kw)
        d = None if "dout" in kw else sentinel.clone()
        wgt = None if a.pop("null_weight", False) else w
        tvb = a.pop("tv", "new")
        sc = a.pop("scratch", "new")
        n, C, H, W = out.shape
        scratch = torch.empty(4096, dtype=torch.uint8, device="cuda") if sc == "new" else None
        tv = torch.zeros(2, dtype=torch.float64, device="cuda") if tvb == "new" else None
        rc = L.lib().mfvi_tv_term(L.ptr(out), a["n_fits"], a["S"], C, H, W, a["channel"], a["beta"], L.ptr(wgt), a["stride"], 1.0, 0, L.ptr(d), L.ptr(tv),
                                  L.ptr(scratch), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -1 and b"tv_term" in L.lib().mfvi_last_error(), kw
        assert d is None or torch.equal(d, sentinel), kw
        assert tv is None or not tv.any(), kw
    for H, W in ((0, 8), (8, 0)):
        rc = L.lib().mfvi_tv_term(L.ptr(out), 1, 1, 1, H, W, 0, 0.5, L.ptr(w), 0, 1.0, 0, L.ptr(sentinel), None, L.ptr(w), L.stream_ptr())
        assert rc == -1 and L.lib().mfvi_tv_term_scratch_bytes(1, 1, H, W) == 0
    rc = L.lib().mfvi_tv_term(None, 1, 1, 1, 8, 8, 0, 0.5, L.ptr(w), 0, 1.0, 0, L.ptr(sentinel), None, L.ptr(w), L.stream_ptr())
    assert rc == -1
    assert L.lib().mfvi_tv_term_scratch_bytes(0, 1, 8, 8) == 0 and L.lib().mfvi_tv_term_scratch_bytes(256, 256, 8, 8) == 0
    assert L.lib().mfvi_tv_term_scratch_bytes(2, 3, 33, 130) == 2 * 3 * 3 * 3 * 8          # one double per 16 x 64 tile and sample
    torch.cuda.synchronize()
    assert torch.equal(sentinel, torch.full_like(out, 123.0))


# ---- 3. the drop-in ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 32, 40)])
def test_tv_loss_drop_in(M, golden, shape):
    cases, _ = golden
    x = next(c[1] for c in cases if c[1].shape == shape)
    for beta in (0.5, 0.75, 1.0):
        t = torch.from_numpy(x).cuda().requires_grad_(True)
        v = M.tv_loss(t, beta)
        assert v.dim() == 0 and v.dtype == torch.float32 and v.requires_grad
        assert relerr([float(v.detach())], [R.tv_value(x, beta)], "tv value") < TOL
        (3 * v).backward()
        assert relerr(host(t.grad), 3 * R.tv_grad(x, beta), "tv gradient") < TOL
    t = torch.from_numpy(x).cuda().requires_grad_(True)
    v = M.tv_loss(t)                                                     # beta defaults to 0.5
    assert relerr([float(v.detach())], [R.tv_value(x, 0.5)], "tv value") < TOL
    nc = torch.from_numpy(x).cuda().transpose(2, 3)                     # a non-contiguous view is the tensor it shows
    assert relerr([float(M.tv_loss(nc))], [R.tv_value(host(nc), 0.5)], "tv value") < TOL
    with pytest.raises(NotImplementedError):
        M.tv_loss(t.detach().double())
    with pytest.raises(ValueError):
        M.tv_loss(t.detach()[0])
    with pytest.raises(ValueError):
        M.tv_loss(t.detach(), 0.0)


# ---- 4. the engines ---------------------------------------------------------------------------------------------------------------------------
def _target(task, S, seed):
    img = O.phantom(S, S, seed)
    if task == "ct":
        return O.radon_fwd(img, np.arange(0, 180., 4., dtype=np.float32))
    if task == "sr":
        return np.ascontiguousarray(img[::4, ::4])
    return O.noisy(img, 0.1, seed)


def _engine(M, task, K=2, S=32, cls=None, **kw):
    cls = cls or M.engine.ElboEngine
    eng = cls(S, S, task=task, K=K, input_depth=8, lr=1e-3, seed=5, net_kwargs=SMALL, autotune=False, **dict(dict(temp=1e-6, sigma=0.05), **kw))
    eng.set_target(torch.from_numpy(_target(task, S, 5)))
    return eng


@pytest.mark.parametrize("task", ["den", "sr", "ct"])
def test_engine_dout_is_the_data_term_plus_the_tv_gradient(M, task):
    w, K = 0.03, 2
    off, on = _engine(M, task, K), _engine(M, task, K, tv_weight=w)
    off.grad_only(0, with_kl=False); on.grad_only(0, with_kl=False)
    torch.cuda.synchronize()
    assert torch.equal(on.out, off.out)
    img = host(on.out[:, 0])
    want = host(off.dout).astype(np.float64)
    want[:, 0] += np.float32(w) / K * R.tv_grad(img)
    assert relerr(host(on.dout)[:, 0], want[:, 0], "dout with tv") < TOL
    if on.out.shape[1] > 1:
        assert torch.equal(on.dout[:, 1:], off.dout[:, 1:])             # the log-precision channel is untouched
    assert abs(on.tv() - R.tv_planes(img).mean()) < TOL * R.tv_planes(img).mean()
    assert off.tv() == 0.0
    assert abs(on.losses()[0] - off.losses()[0]) <= 1e-12 * abs(off.losses()[0])      # losses() keeps its meaning (the NLL is an fp64 sum by atomic adds: equal to the last bits)
    # the parameter gradients are plan.backward of that dout, bit for bit
    g = torch.zeros_like(on.grads)
    nv = on.n_vi
    on.plan.backward(on.mu, on.rho, on.bn, on.z, on.seed, 0, 0, K, on.dout, g[:nv], g[nv:2 * nv], g[2 * nv:on.n_params], True)
    torch.cuda.synchronize()
    assert torch.equal(g[:on.n_params], on.grads[:on.n_params]) and not torch.equal(on.grads, off.grads)


def test_engine_with_zero_weight_is_the_engine_without_the_term(M):
    a, b = _engine(M, "den"), _engine(M, "den", tv_weight=0.0, tv_beta=0.5)
    assert b._tv is None
    for e in (a, b):
        e.grad_only(0, with_kl=False)
    torch.cuda.synchronize()
    assert torch.equal(a.grads, b.grads) and torch.equal(a.dout, b.dout) and torch.equal(a.acc, b.acc)
    a.step(); b.step()
    assert torch.equal(a.params, b.params)


def test_engine_chunks_add_up(M):
    """samples_per_launch < K: the term runs once per chunk and the += into the accumulator makes the chunks add up."""
    one, two = _engine(M, "den", K=4, tv_weight=0.02), _engine(M, "den", K=4, tv_weight=0.02, samples_per_launch=2)
    one.grad_only(0, with_kl=False); two.grad_only(0, with_kl=False)
    assert abs(one.tv() - two.tv()) < 1e-12 * one.tv()
    assert relerr(host(two.grads), host(one.grads), "grads in chunks") < 1e-4


def test_engine_thirty_steps(M):
    w = 0.02
    on, off = _engine(M, "den", tv_weight=w), _engine(M, "den")
    obj = []
    for i in range(30):
        on.step(); off.step()
        if i in (0, 29):
            nll, kl, loss = on.losses()
            assert np.isfinite([nll, kl, loss, on.tv()]).all()
            obj.append(nll + w * on.tv())
    assert obj[1] < obj[0]
    tv_off = float(R.tv_planes(host(off.out[:, 0])).mean())
    print("TV of the output after 30 steps: %.4f with tv_weight %g, %.4f without" % (on.tv(), w, tv_off))


def test_sibling_engine_takes_the_term(M):
    eng = _engine(M, "den", K=1, cls=M.engine.SiblingEngine, method="dip", tv_weight=0.05)
    off = _engine(M, "den", K=1, cls=M.engine.SiblingEngine, method="dip")
    eng.grad_only(0, with_kl=False); off.grad_only(0, with_kl=False)
    img = host(eng.out[:, 0])
    want = host(off.dout).astype(np.float64)
    want[:, 0] += np.float32(0.05) * R.tv_grad(img)
    assert relerr(host(eng.dout)[:, 0], want[:, 0], "dout with tv") < TOL and abs(eng.tv() - R.tv_value(img)) < TOL * R.tv_value(img)
    eng.step()
    assert np.isfinite(eng.losses()).all()


# ---- 5. device-resident iteration and graph replay --------------------------------------------------------------------------------------------
def test_device_step_and_graph_replay_are_bit_identical_with_tv(M):
    """tests/test_gpu_graph.py's ("den", 2) case with the term on: its launches depend on no host value."""
    def make():
        from mfvi_dip_mia_amd.engine import ElboEngine
        S = 64
        eng = ElboEngine(S, S, task="den", K=2, input_depth=8, temp=5.7e-7, sigma=1.5e-5, lr=1e-3, seed=11,
                         net_kwargs=dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4)), autotune=False, tv_weight=0.02)
        eng.set_target(torch.from_numpy(O.noisy(O.phantom(S, S, 11), 0.1, 11)))
        return eng
    n = 9
    ref = make()
    for _ in range(n):
        ref.step()
    dev = make().enable_device_step()
    for _ in range(n):
        dev.step()
    assert int(dev.step_dev) == n and torch.equal(dev.params, ref.params) and torch.equal(dev.m, ref.m) and torch.equal(dev.v, ref.v)
    gr = make().enable_graph(warmup=3)
    for _ in range(n - 3):
        gr.step()
    torch.cuda.synchronize()
    assert int(gr.step_dev) == n
    assert torch.equal(gr.params, ref.params) and torch.equal(gr.m, ref.m) and torch.equal(gr.v, ref.v)
    assert gr.tv() == ref.tv() and ref.tv() > 0.0                       # (a fixed-order sum: equal to the bit)


# ---- 6. batches -------------------------------------------------------------------------------------------------------------------------------
def _fitbatch(M, **kw):
    fb = M.FitBatch(32, 32, 3, task="den", K=2, input_depth=8, temp=[1e-6, 2e-6, 4e-6], sigma=0.05, lr=1e-3, seed=3, net_kwargs=SMALL, autotune=False, **kw)
    fb.set_targets(torch.from_numpy(np.stack([O.noisy(O.phantom(32, 32, 3 + f), 0.1, 3 + f) for f in range(3)])))
    return fb


def test_fitbatch_per_fit_weights(M):
    ws, K = [0.0, 0.02, 0.05], 2
    off, on = _fitbatch(M), _fitbatch(M, tv_weight=ws)
    assert off._tv is None and not off.tv().any()
    off.grad_only(0); on.grad_only(0)
    torch.cuda.synchronize()
    assert torch.equal(on.out, off.out)
    assert torch.equal(on.dout[:K], off.dout[:K]) and torch.equal(on.grads[0], off.grads[0])      # fit 0 of weight 0: bit-equal
    assert torch.equal(on.nll_acc, off.nll_acc)
    img = host(on.out[:, 0])
    want = host(off.dout).astype(np.float64)
    for f in range(3):
        want[f * K:(f + 1) * K, 0] += np.float32(ws[f]) / K * R.tv_grad(img[f * K:(f + 1) * K])
    assert relerr(host(on.dout)[:, 0], want[:, 0], "dout with tv") < TOL and torch.equal(on.dout[:, 1], off.dout[:, 1])
    assert not torch.equal(on.grads[1], off.grads[1]) and not torch.equal(on.grads[2], off.grads[2])
    assert relerr(on.tv(), R.tv_planes(img).reshape(3, K).mean(1), "tv value") < TOL
    eng = on.to_engine(2)
    assert eng.tv_weight == ws[2] and eng.tv_beta == 0.5 and on.to_engine(0)._tv is None
    on.step()
    assert np.isfinite(on.losses()[2]).all() and not on.dead.any()


def test_ctvolume_weights_follow_the_group_offset(M):
    ws, S, D = [0.01, 0.03, 0.09], 32, 3
    sinos = np.stack([_target("ct", S, 20 + d) for d in range(D)]).astype(np.float32)

    def make(**kw):
        vol = M.CtVolume(S, D, slices_per_launch=2, K=1, input_depth=8, temp=1e-4, sigma=0.05, lr=1e-3, seed=9, net_kwargs=SMALL, autotune=False, **kw)
        vol.set_sinograms(torch.from_numpy(sinos))
        return vol
    off, on = make(), make(tv_weight=ws)
    assert len(on.groups) == 2
    seen = {}
    for vol, tag in ((off, "off"), (on, "on")):      # the groups share out / dout: record them per group, behind each group's data term
        orig = vol.plan.backward
        def spy(*a, _vol=vol, _tag=tag, _orig=orig, **k):
            n = a[7]
            seen.setdefault(_tag, []).append((host(_vol.out[:n]).copy(), host(_vol.dout[:n]).copy()))
            return _orig(*a, **k)
        vol.plan.backward = spy
        vol.grad_only(0)
        torch.cuda.synchronize()
    tv = on.tv()
    row = 0
    for (out_off, dout_off), (out_on, dout_on) in zip(seen["off"], seen["on"]):
        assert np.array_equal(out_on, out_off)
        for i in range(out_on.shape[0]):
            want = dout_off[i, 0].astype(np.float64) + np.float32(ws[row]) * R.tv_grad(out_on[i, 0])
            assert relerr(dout_on[i, 0], want, "dout with tv") < TOL, row
            inc = np.abs(dout_on[i, 0] - dout_off[i, 0]).max() / np.abs(R.tv_grad(out_on[i, 0])).max()
            assert abs(inc / ws[row] - 1.0) < 1e-2, (row, inc)            # each slice's increment carries its OWN weight
            assert abs(tv[row] - R.tv_value(out_on[i, 0])) < TOL * tv[row]
            row += 1
    assert row == D and on.to_engine(1).tv_weight == ws[1]


def test_siblingbatch_takes_the_term(M):
    w = 0.04
    sb = M.SiblingBatch(32, 32, 2, "dip", task="den", K=1, input_depth=8, lr=1e-3, seed=4, net_kwargs=SMALL, autotune=False, tv_weight=w)
    sb.set_targets(torch.from_numpy(np.stack([O.noisy(O.phantom(32, 32, 4 + f), 0.1, 4 + f) for f in range(2)])))
    sb.step()
    torch.cuda.synchronize()
    assert np.isfinite(sb.losses()).all() and not sb.dead.any() and torch.isfinite(sb.params).all()
    assert relerr(sb.tv(), R.tv_planes(host(sb.out[:, 0])), "tv value") < TOL
    assert sb.to_engine(1).tv_weight == w


# ---- 7. runners -------------------------------------------------------------------------------------------------------------------------------
def test_runner_artifacts_with_and_without_the_term(M, tmp_path):
    kw = dict(img="phantom", imsize=(64, 64), num_iter=3, lr=1e-3, temp=1e-6, sigma=0.05, input_depth=8, seed=1, show_every=2, save=True, K=1,
              net_kwargs=SMALL)
    on = M.runner.run_den_mfvi(tv_weight=0.02, save_path=str(tmp_path / "on"), **kw)
    off = M.runner.run_den_mfvi(save_path=str(tmp_path / "off"), **kw)
    keys = {"img_gt", "img_noisy", "mse_noisy", "mse_gt", "recons", "uncerts", "uncerts_ale", "psnrs", "ssims"}
    assert set(np.load(os.path.join(on["run_dir"], "save.npz"), allow_pickle=True).files) == keys
    assert set(np.load(os.path.join(off["run_dir"], "save.npz"), allow_pickle=True).files) == keys
    assert sorted(os.listdir(on["run_dir"])) == sorted(os.listdir(off["run_dir"]))
    text_on, text_off = (open(os.path.join(r["run_dir"], "locals.txt")).read() for r in (on, off))
    assert "tv_weight" in text_on and "tv_beta" in text_on and "tv_" not in text_off
    assert on["engine"].tv_weight == 0.02 and on["engine"].tv() > 0.0 and off["engine"]._tv is None
    assert not np.array_equal(on["psnrs"], off["psnrs"]) and np.isfinite(on["psnrs"]).all()


def test_run_fit_batch_records_the_term(M, tmp_path):
    jobs = [dict(img="phantom", temp=1e-6, sigma=0.05), dict(img="phantom", temp=2e-6, sigma=0.05, tv_weight=0.03)]
    kw = dict(imsize=(32, 32), num_iter=4, lr=1e-3, input_depth=8, seed=1, show_every=2, K=1, net_kwargs=SMALL, autotune=False)
    base = {"task", "temp", "sigma", "lr", "prior_sigma", "K", "seed", "num_iter", "iterations", "psnr_gt_sm", "nll", "kl", "recon", "dead"}
    r = M.runner.run_fit_batch("den", jobs, save_path=str(tmp_path / "on"), **kw)
    z = np.load(os.path.join(r["run_dir"], "batch.npz"))
    assert set(z.files) == base | {"tv_weight", "tv_beta", "tv"}
    assert list(z["tv_weight"]) == [0.0, 0.03] and z["tv"].shape == z["nll"].shape == (3, 2) and (z["tv"] > 0).all() and float(z["tv_beta"]) == 0.5
    r = M.runner.run_fit_batch("den", [dict(j, tv_weight=0.0) for j in jobs], save_path=str(tmp_path / "off"), **kw)
    assert set(np.load(os.path.join(r["run_dir"], "batch.npz")).files) == base
    r = M.runner.run_fit_batch("den", jobs[:1], tv_weight=0.01, save_path=str(tmp_path / "wide"), **kw)      # the run-wide value
    assert list(np.load(os.path.join(r["run_dir"], "batch.npz"))["tv_weight"]) == [0.01]


# ---- 8. K sharded over two ranks --------------------------------------------------------------------------------------------------------------
def test_tv_rides_the_exchange_on_two_ranks(M, tmp_path):
    """In the manner of tests/test_gpu_multirank.py (fresh child processes, gloo, one GPU): tv() on both ranks is the single-rank value."""
    out = str(tmp_path / "tv_ranks")
    port = str(31500 + os.getpid() % 2000)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "tv_rank_worker.py"), str(r), "2", port, out], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    logs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    from tv_rank_worker import make_engine
    eng = make_engine(0, 1)
    eng.grad_only(0, with_kl=False)
    z = [np.load("%s_%d.npz" % (out, r)) for r in range(2)]
    assert float(z[0]["tv"]) == float(z[1]["tv"]) and int(z[0]["k_local"]) == 2
    assert abs(float(z[0]["tv"]) - eng.tv()) < 1e-6 * eng.tv()          # the sum rides the all-reduce as a float
    assert np.allclose(z[0]["nll"], eng.losses()[0], rtol=2e-6)
