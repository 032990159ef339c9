"""The forward direction of the KL term, KL(posterior || prior), on the GPU: the typed entry points against the
reference's recorded values (tests/golden/kl_forward.npz) and the float64 restatement (tests/kl_restatement.py), the reverse direction
through the typed entries against the untyped twins bit for bit, fused against unfused, the bf16 update against its host emulation, the
per-fit update against the single-fit one, and the direction through ElboEngine, the row batches, the drop-in MeanFieldVI and the runner.

Tolerances are the project's own for the reverse direction: value 1e-6 relative and gradients relerr < 1e-5 (tests/test_gpu_parity.py:308,
311), fused against unfused as tests/test_gpu_siblings.py:187-190, per-fit against single-fit <= 1 ulp with KL 1e-12 relative
(tests/test_gpu_fitbatch.py:282-283), the bf16 update as tests/test_gpu_bf16.py:142-154."""
import json
import os
import re

import numpy as np
import pytest

from conftest import note_margin as _note

import kl_restatement as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SMALL = dict(nd=(8, 16), nu=(8, 16), ns=(4, 4))
INP_KW = dict(nd=(8, 16, 16), nu=(8, 16, 16), ns=(0, 0, 0))
REV, FWD = 0, 1
TOL_VALUE, TOL_GRAD = 1e-6, 1e-5
PRIOR01 = dict(temp=1e-4, sigma=10.0)      # sqrt(temp) * sigma + 1e-6: a prior scale of ~0.1


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    assert torch.cuda.is_available()
    M_._lib.lib()
    return M_


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "kl_forward.npz"), allow_pickle=False)


def relerr(a, b, what="relerr"):
    v = R.relerr(a, b)
    _note(v, what)
    return v


def relval(a, b, what="kl value"):
    v = abs(float(a) - float(b)) / abs(float(b))
    _note(v, what)
    return v


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64); b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a); b = np.where(b < 0, -(b & 0x7fffffff), b)
    return int(np.abs(a - b).max())


def _kl(M, mu, rho, m0, s0, kt=FWD):
    L = M._lib
    out = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")      # overwritten, not accumulated
    L.check(L.lib().mfvi_kl_typed(L.ptr(mu), L.ptr(rho), mu.numel(), m0, s0, kt, L.ptr(out), L.stream_ptr()))
    return float(out)


def _kl_bwd(M, mu, rho, m0, s0, scale, dmu, drho, kt=FWD):
    L = M._lib
    L.check(L.lib().mfvi_kl_backward_typed(L.ptr(mu), L.ptr(rho), mu.numel(), m0, s0, scale, kt, L.ptr(dmu), L.ptr(drho), L.stream_ptr()))


# ---- 1. the unfused pair ------------------------------------------------------------------------------------------------------------------------
def test_unfused_pair_against_the_golden_and_the_restatement(M, gold):
    scale, sentinel = 0.37, 0.25
    for name in R.LAYER_CASES:
        mu, rho = R.case_inputs(gold, name)
        m0, s0 = (float(v) for v in gold[name + "_prior"])
        ref = "c1" if name == "c5" else name
        v64, dm64, dr64 = float(gold[ref + "_kl64"]), gold[ref + "_dmu64"], gold[ref + "_drho64"]
        rv, rdm, rdr = R.kl_forward(mu, rho, m0, s0)
        d_mu, d_rho = dev(mu), dev(rho)
        got = _kl(M, d_mu, d_rho, m0, s0)
        assert relval(got, v64) < TOL_VALUE and relval(got, rv) < TOL_VALUE and relval(got, float(gold[name + "_kl"])) < TOL_VALUE, name
        dmu = torch.full_like(d_mu, sentinel); drho = torch.full_like(d_rho, sentinel)      # += is what is checked
        _kl_bwd(M, d_mu, d_rho, m0, s0, scale, dmu, drho)
        for g, w64, wr in ((dmu, dm64, rdm), (drho, dr64, rdr)):
            assert relerr(host(g), sentinel + scale * w64) < TOL_GRAD and relerr(host(g), sentinel + scale * wr) < TOL_GRAD, name
        one = torch.zeros_like(d_mu); one_r = torch.zeros_like(d_rho)
        _kl_bwd(M, d_mu, d_rho, m0, s0, 1.0, one, one_r)
        assert relerr(host(one), gold[name + "_dmu"]) < TOL_GRAD and relerr(host(one_r), gold[name + "_drho"]) < TOL_GRAD, name
        # the gradient kernel has no reduction: two calls are bit-identical, as the reverse kernel's are; so is the value of a one-block call
        again = torch.zeros_like(d_mu); again_r = torch.zeros_like(d_rho)
        _kl_bwd(M, d_mu, d_rho, m0, s0, 1.0, again, again_r)
        assert torch.equal(one, again) and torch.equal(one_r, again_r)
        assert _kl(M, d_mu[:R.N_B], d_rho[:R.N_B], m0, s0) == _kl(M, d_mu[:R.N_B], d_rho[:R.N_B], m0, s0)


def _net_flat(gold):
    """The golden net's tensors as flat (mu, rho) with the layer slices [(name, lo, hi)], layer after layer: W | bias."""
    keys = [str(k) for k in gold["net_keys"]]
    mu, rho, slices, lo = [], [], [], 0
    layers = [str(k) for k in gold["net_layers"]]
    for name in layers:
        n = 0
        for part in ("W", "bias"):
            k = "%s.%s_mu" % (name, part)
            if k in keys:
                mu.append(gold["net_p%d" % keys.index(k)].ravel()); rho.append(gold["net_p%d" % keys.index("%s.%s_rho" % (name, part))].ravel())
                n += mu[-1].size
        slices.append((name, lo, lo + n)); lo += n
    return np.concatenate(mu), np.concatenate(rho), slices


def test_unfused_pair_on_the_flat_net_and_a_large_block(M, gold):
    mu, rho, slices = _net_flat(gold)
    m0, s0 = (float(v) for v in gold["net_prior"])
    d_mu, d_rho = dev(mu), dev(rho)
    assert len(slices) == 11 and slices[-1][2] == mu.size
    for (name, lo, hi), want in zip(slices, gold["net_layer_kl"]):
        got = _kl(M, d_mu[lo:hi], d_rho[lo:hi], m0, s0)
        assert relval(got, R.kl_forward(mu[lo:hi], rho[lo:hi], m0, s0)[0]) < TOL_VALUE and relval(got, float(want)) < TOL_VALUE, name
    tot = _kl(M, d_mu, d_rho, m0, s0)
    assert relval(tot, float(gold["net_kl64"])) < TOL_VALUE and relval(tot, float(gold["net_kl"])) < TOL_VALUE
    # more than one grid stride, the inputs of test_losses_kl_adam_metrics_radon
    n = 100003
    mu = 0.1 * O.normal_fill(9, 2, 0, 0, 0, n); rho = -3 + 0.5 * O.normal_fill(9, 2, 1, 0, 0, n)
    s0 = float(np.float32(1.0109e-6))
    rv, rdm, rdr = R.kl_forward(mu, rho, 0.0, s0)
    d_mu, d_rho = dev(mu), dev(rho)
    assert relval(_kl(M, d_mu, d_rho, 0.0, s0), rv) < TOL_VALUE
    dmu = torch.zeros(n, device="cuda"); drho = torch.zeros(n, device="cuda")
    _kl_bwd(M, d_mu, d_rho, 0.0, s0, 0.37, dmu, drho)
    assert relerr(host(dmu), 0.37 * rdm) < TOL_GRAD and relerr(host(drho), 0.37 * rdr) < TOL_GRAD


def test_typed_entries_refuse_before_any_launch(M):
    L = M._lib; lib, sp = L.lib(), L.stream_ptr()
    x = torch.zeros(8, device="cuda"); k = torch.zeros(1, dtype=torch.float64, device="cuda")
    sc = torch.zeros(lib.mfvi_elbo_update_scratch_bytes(), dtype=torch.uint8, device="cuda")
    for kt, s0, n, why in ((2, 0.1, 4, b"kl_type"), (-1, 0.1, 4, b"kl_type"), (FWD, 0.0, 4, b"prior_sigma"), (REV, float("inf"), 4, b"prior_sigma"),
                           (FWD, float("nan"), 4, b"prior_sigma"), (FWD, 1e-20, 4, b"normal float32"), (FWD, 0.1, 0, b"n < 1")):
        assert lib.mfvi_kl_typed(L.ptr(x), L.ptr(x), n, 0.0, s0, kt, L.ptr(k), sp) == -1 and why in lib.mfvi_last_error(), (kt, s0, n)
        assert lib.mfvi_kl_backward_typed(L.ptr(x), L.ptr(x), n, 0.0, s0, 1.0, kt, L.ptr(x), L.ptr(x), sp) == -1 and why in lib.mfvi_last_error()
    assert lib.mfvi_kl_typed(None, L.ptr(x), 4, 0.0, 0.1, FWD, L.ptr(k), sp) == -1
    for kt, s0 in ((2, 0.1), (FWD, 1e-20), (FWD, -1.0)):
        assert lib.mfvi_elbo_update_typed(L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), 2, 4, 0.0, s0, 1.0, kt, 1e-3, 0.9, 0.999, 1e-8, 1, L.ptr(k), L.ptr(sc), sp) == -1
        assert lib.mfvi_elbo_update_guarded_typed(L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), 2, 4, 0.0, s0, 1.0, kt, 1e-3, 0.9, 0.999, 1e-8, L.ptr(x), None, None,
                                                  L.ptr(k), L.ptr(sc), sp) == -1
        assert lib.mfvi_elbo_update_bf16_typed(L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), 2, 0, 0.0, s0, 1.0, kt, 1e-3, 0.9, 0.999, 1e-8, 1, 3,
                                               L.ptr(k), L.ptr(sc), sp) == -1
    assert lib.mfvi_elbo_update_typed(L.ptr(x), L.ptr(x), L.ptr(x), L.ptr(x), 2, 4, 0.0, 0.1, 1.0, FWD, 1e-3, 0.9, 0.999, 1e-8, 0, L.ptr(k), L.ptr(sc), sp) == -1
    assert not x.any() and float(k) == 0.0


# ---- 2. the reverse direction through the typed entries: the untyped twins, bit for bit ------------------------------------------------------
def _update_inputs(nv, nb, seed):
    n = 2 * nv + nb
    p = np.concatenate([0.1 * O.normal_fill(seed, 2, 0, 0, 0, nv), -3 + 0.1 * O.normal_fill(seed, 2, 1, 0, 0, nv), 1 + 0.1 * O.normal_fill(seed, 2, 2, 0, 0, nb)])
    g = 1e-3 * O.normal_fill(seed, 2, 3, 0, 0, n)
    m = 1e-3 * O.normal_fill(seed, 2, 4, 0, 0, n); v = np.abs(1e-4 * O.normal_fill(seed, 2, 5, 0, 0, n))
    return [a.astype(np.float32) for a in (p, g, m, v)]


def test_reverse_through_the_typed_entries_is_the_untyped_entry(M):
    L = M._lib; lib, sp, p_ = L.lib(), L.stream_ptr(), L.ptr
    nv, nb, seed = 1003, 37, 5
    n = 2 * nv + nb
    p0, g0, m0, v0 = _update_inputs(nv, nb, seed)
    ps, temp, lr = 0.05, 3e-4, 1e-3
    sc = torch.zeros(lib.mfvi_elbo_update_scratch_bytes(), dtype=torch.uint8, device="cuda")
    # mfvi_kl adds its blocks' sums by atomics: one block (n <= 256) is the call whose value is defined to the bit
    mu, rho = dev(p0[:200]), dev(p0[nv:nv + 200])
    a = torch.zeros(1, dtype=torch.float64, device="cuda")
    L.check(lib.mfvi_kl(p_(mu), p_(rho), 200, 0.0, ps, p_(a), sp))
    assert float(a) == _kl(M, mu, rho, 0.0, ps, REV)
    mu, rho = dev(p0[:nv]), dev(p0[nv:2 * nv])
    ga, gb = dev(g0[:2 * nv]), dev(g0[:2 * nv])
    L.check(lib.mfvi_kl_backward(p_(mu), p_(rho), nv, 0.0, ps, temp, p_(ga), p_(ga[nv:]), sp))
    _kl_bwd(M, mu, rho, 0.0, ps, temp, gb[:nv], gb[nv:], REV)
    assert torch.equal(ga, gb) and not torch.equal(ga, dev(g0[:2 * nv]))

    def both(call_a, call_b, make):
        sa, sb = make(), make()
        call_a(sa); call_b(sb)
        for x, y in zip(sa, sb):      # every output and every input, bit for bit (the bf16 words as integers; an input may be the NaN data term)
            x, y = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t for t in (x, y))
            assert np.array_equal(host(x), host(y), equal_nan=True)
        return sa
    state = lambda: [dev(p0), dev(g0), dev(m0), dev(v0), torch.zeros(1, dtype=torch.float64, device="cuda")]
    s = both(lambda s: L.check(lib.mfvi_elbo_update(p_(s[0]), p_(s[1]), p_(s[2]), p_(s[3]), nv, nb, 0.0, ps, temp, lr, 0.9, 0.999, 1e-8, 3, p_(s[4]), p_(sc), sp)),
             lambda s: L.check(lib.mfvi_elbo_update_typed(p_(s[0]), p_(s[1]), p_(s[2]), p_(s[3]), nv, nb, 0.0, ps, temp, REV, lr, 0.9, 0.999, 1e-8, 3, p_(s[4]), p_(sc), sp)),
             state)
    assert not torch.equal(s[0], dev(p0)) and float(s[4]) > 0
    for nan in (False, True):
        gstate = lambda: state() + [torch.full((1,), 2, dtype=torch.int32, device="cuda"), torch.tensor([float("nan") if nan else 0.3], dtype=torch.float64, device="cuda")]
        s = both(lambda s: L.check(lib.mfvi_elbo_update_guarded(p_(s[0]), p_(s[1]), p_(s[2]), p_(s[3]), nv, nb, 0.0, ps, temp, lr, 0.9, 0.999, 1e-8, p_(s[5]), p_(s[6]),
                                                                None, p_(s[4]), p_(sc), sp)),
                 lambda s: L.check(lib.mfvi_elbo_update_guarded_typed(p_(s[0]), p_(s[1]), p_(s[2]), p_(s[3]), nv, nb, 0.0, ps, temp, REV, lr, 0.9, 0.999, 1e-8, p_(s[5]),
                                                                      p_(s[6]), None, p_(s[4]), p_(sc), sp)), gstate)
        assert int(s[5]) == (2 if nan else 3) and torch.equal(s[0], dev(p0)) == nan
    pad = (nv + 7) // 8 * 8

    def bstate():
        b16 = torch.zeros(2 * pad, dtype=torch.bfloat16, device="cuda")
        b16[:nv].copy_(dev(O.bf16_round(p0[:nv]))); b16[pad:pad + nv].copy_(dev(O.bf16_round(p0[nv:2 * nv])))
        return [b16, dev(p0[2 * nv:]), dev(g0), dev(m0), dev(v0), torch.zeros(1, dtype=torch.float64, device="cuda")]
    s = both(lambda s: L.check(lib.mfvi_elbo_update_bf16(p_(s[0]), p_(s[0][pad:]), p_(s[1]), p_(s[2]), p_(s[3]), p_(s[4]), nv, nb, 0.0, ps, temp, lr, 0.9, 0.999, 1e-8,
                                                         2, 17, p_(s[5]), p_(sc), sp)),
             lambda s: L.check(lib.mfvi_elbo_update_bf16_typed(p_(s[0]), p_(s[0][pad:]), p_(s[1]), p_(s[2]), p_(s[3]), p_(s[4]), nv, nb, 0.0, ps, temp, REV, lr, 0.9, 0.999,
                                                               1e-8, 2, 17, p_(s[5]), p_(sc), sp)), bstate)
    assert float(s[5]) > 0
    F = 3
    hyper = dev(np.array([[0.0, 0.05 * (f + 1), 1e-4 * (f + 1), 1e-3] for f in range(F)], np.float32))
    fsc = torch.zeros(lib.mfvi_elbo_update_fits_scratch_bytes(F), dtype=torch.uint8, device="cuda")
    rows = lambda a: dev(np.stack([np.roll(a, f) if a is not p0 else a + np.float32(0.01 * f) for f in range(F)]))
    fstate = lambda: [rows(p0), rows(g0), rows(m0), rows(v0), torch.zeros(F, dtype=torch.float64, device="cuda"), torch.zeros(F, dtype=torch.int32, device="cuda"),
                      torch.tensor([0.3, float("nan"), 0.5], dtype=torch.float64, device="cuda")]
    s = both(lambda s: L.check(lib.mfvi_elbo_update_fits(p_(s[0]), p_(s[1]), p_(s[2]), p_(s[3]), nv, nb, n, n, F, p_(hyper), 0.9, 0.999, 1e-8, 2, p_(s[6]), p_(s[5]),
                                                         p_(s[4]), p_(fsc), sp)),
             lambda s: L.check(lib.mfvi_elbo_update_fits_typed(p_(s[0]), p_(s[1]), p_(s[2]), p_(s[3]), nv, nb, n, n, F, p_(hyper), None, 0.9, 0.999, 1e-8, 2, p_(s[6]),
                                                               p_(s[5]), p_(s[4]), p_(fsc), sp)), fstate)
    assert host(s[5]).tolist() == [0, 1, 0]


# ---- 3. fused forward = unfused forward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,temp", [(0.1, 1e-4), (1.0000110e-06, 5.6e-7)])
def test_fused_forward_update_equals_kl_plus_adam(M, ps, temp):
    """The structure of test_fused_elbo_update_equals_kl_plus_adam (tests/test_gpu_siblings.py), its tolerances, the forward direction; then
    the guarded entry (device counter), and a NaN data term: nothing but kl_out is written.

    The KL check, 1e-10 relative (a different fp64 summation order and nothing else), is made where it is defined: the fused KL against the
    unfused KL of the SAME parameters, at every t.  That test's own form compares the KL of the two trajectories, whose parameters it allows
    to differ by 1e-6 (the compiler's fma contraction in the two Adam kernels; measured here: a few float32 ulp from t = 2 on).  The reverse
    KL of that test is ~3e6 and hides such a difference; the forward KL here is ~850 with d kl / d mu = d / s0^2 ~ 10, and the two
    trajectories' KL measured 1.7e-10 (prior scale 0.1) and 1.2e-10 (1e-6) apart at t = 2, all of it the parameters' difference.  So the
    trajectories' KL is held to 1e-10 plus the first-order effect of the parameter difference actually present, sum |dkl/dp| |dp| from the
    float64 restatement: exactly that test's 1e-10 at t = 1, where the parameters are the same."""
    L = M._lib; lib, sp, p_ = L.lib(), L.stream_ptr(), L.ptr
    nv, nb = 1003, 37
    n = 2 * nv + nb
    p0n, g0n, _, _ = _update_inputs(nv, nb, 3)
    p0, g0 = dev(p0n), dev(g0n)
    sc = torch.zeros(lib.mfvi_elbo_update_scratch_bytes(), dtype=torch.uint8, device="cuda")
    close = lambda a, b: float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())
    for guarded in (False, True):
        pa, ga, ma, va = p0.clone(), g0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        pb, gb, mb, vb = p0.clone(), g0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        kla = torch.zeros(1, dtype=torch.float64, device="cuda")
        t_dev = torch.zeros(1, dtype=torch.int32, device="cuda"); loss_d = torch.tensor([0.25], dtype=torch.float64, device="cuda")
        for t in (1, 2, 3):
            ga.copy_(g0); gb.copy_(g0)
            before_a, before_b = pa.clone(), host(pb).astype(np.float64)
            if guarded:
                L.check(lib.mfvi_elbo_update_guarded_typed(p_(pa), p_(ga), p_(ma), p_(va), nv, nb, 0.0, ps, temp, FWD, 1e-3, 0.9, 0.999, 1e-8, p_(t_dev), p_(loss_d), None,
                                                           p_(kla), p_(sc), sp))
                assert int(t_dev) == t
            else:
                L.check(lib.mfvi_elbo_update_typed(p_(pa), p_(ga), p_(ma), p_(va), nv, nb, 0.0, ps, temp, FWD, 1e-3, 0.9, 0.999, 1e-8, t, p_(kla), p_(sc), sp))
            klb = _kl(M, pb[:nv], pb[nv:2 * nv], 0.0, ps)
            if t == 1:
                assert relval(klb, R.kl_forward(p0n[:nv], p0n[nv:2 * nv], 0.0, ps)[0]) < TOL_VALUE
            _kl_bwd(M, pb[:nv], pb[nv:2 * nv], 0.0, ps, temp, gb[:nv], gb[nv:2 * nv])
            L.check(lib.mfvi_adam_step(p_(pb), p_(gb), p_(mb), p_(vb), n, 1e-3, 0.9, 0.999, 1e-8, t, sp))
            assert close(ga, gb) and close(ma, mb) and close(va, vb), (guarded, t)
            assert float((pa - pb).abs().max()) < 1e-6, (guarded, t)
            assert relval(float(kla), _kl(M, before_a[:nv], before_a[nv:2 * nv], 0.0, ps), "fused kl against unfused, same parameters") < 1e-10, (guarded, t)
            dp = np.abs(host(before_a).astype(np.float64) - before_b)
            _, dkm, dkr = R.kl_forward(before_b[:nv], before_b[nv:2 * nv], 0.0, float(np.float32(ps)))
            first_order = float((np.abs(dkm) * dp[:nv]).sum() + (np.abs(dkr) * dp[nv:2 * nv]).sum())
            assert (t > 1 or first_order == 0.0) and abs(float(kla) - klb) <= 1e-10 * abs(klb) + 1.01 * first_order, (guarded, t, float(kla), klb, first_order)
    # NaN in the data term: parameters, moments and the counter stay, the KL of the parameters is still reported
    snap = [x.clone() for x in (pa, ma, va)]
    ga.copy_(g0); loss_d.fill_(float("nan")); kla.zero_()
    L.check(lib.mfvi_elbo_update_guarded_typed(p_(pa), p_(ga), p_(ma), p_(va), nv, nb, 0.0, ps, temp, FWD, 1e-3, 0.9, 0.999, 1e-8, p_(t_dev), p_(loss_d), None,
                                               p_(kla), p_(sc), sp))
    assert all(torch.equal(a, b) for a, b in zip(snap, (pa, ma, va))) and torch.equal(ga, g0) and int(t_dev) == 3
    assert relval(float(kla), _kl(M, pa[:nv], pa[nv:2 * nv], 0.0, ps), "fused kl against unfused") < 1e-10


# ---- 4. bf16 -----------------------------------------------------------------------------------------------------------------------------------
def test_bf16_forward_update_against_host_emulation(M):
    """test_bf16_update_against_oracle (tests/test_gpu_bf16.py) with the forward term: float32 arithmetic on the values the bf16 words
    denote (here: the float64 restatement rounded to float32), stochastic rounding from RNG domain 6; that test's tolerances."""
    L = M._lib; lib = L.lib()
    n_vi, n_bn, seed = 1003, 37, 17
    mu = O.bf16_round(0.1 * O.normal_fill(seed, 2, 0, 0, 0, n_vi)); rho = O.bf16_round(-3 + 0.1 * O.normal_fill(seed, 2, 1, 0, 0, n_vi))
    bn = (1 + 0.1 * O.normal_fill(seed, 2, 2, 0, 0, n_bn)).astype(np.float32)
    pad = (n_vi + 7) // 8 * 8
    b16 = torch.zeros(2 * pad, dtype=torch.bfloat16, device="cuda"); b_mu, b_rho = b16[:n_vi], b16[pad:pad + n_vi]
    b_mu.copy_(dev(mu)); b_rho.copy_(dev(rho)); d_bn = dev(bn)
    assert np.array_equal(host(b_mu.float()), mu) and np.array_equal(host(b_rho.float()), rho)
    m = torch.zeros(2 * n_vi + n_bn, device="cuda"); v = torch.zeros_like(m)
    scratch = torch.zeros(lib.mfvi_elbo_update_scratch_bytes(), dtype=torch.uint8, device="cuda")
    kl = torch.zeros(1, dtype=torch.float64, device="cuda")
    prior_sigma, temp, lr = 0.05, 3e-4, 1e-3
    om_bits, or_bits = O.bf16_bits(mu), O.bf16_bits(rho)
    om = np.zeros(2 * n_vi + n_bn, np.float32); ov = np.zeros_like(om); obn = bn.copy()
    moved = 0
    for t in range(1, 4):
        g = (1e-3 * O.normal_fill(seed, 2, 10 + t, 0, 0, 2 * n_vi + n_bn)).astype(np.float32)
        d_g = dev(g)
        L.check(lib.mfvi_elbo_update_bf16_typed(L.ptr(b_mu), L.ptr(b_rho), L.ptr(d_bn), L.ptr(d_g), L.ptr(m), L.ptr(v), n_vi, n_bn, 0.0, prior_sigma, temp, FWD, lr,
                                                0.9, 0.999, 1e-8, t, seed, L.ptr(kl), L.ptr(scratch), L.stream_ptr()))
        fmu, frho = O.bf16_from_bits(om_bits), O.bf16_from_bits(or_bits)
        okl, dkm, dkr = R.kl_forward(fmu, frho, 0.0, float(np.float32(prior_sigma)))
        gg = g.copy(); gg[:n_vi] += (np.float32(temp) * dkm).astype(np.float32); gg[n_vi:2 * n_vi] += (np.float32(temp) * dkr).astype(np.float32)
        assert relval(float(kl), okl) < 1e-6
        assert relerr(host(d_g), gg) < 2e-6                              # grads += temp * dKL, written back
        before = om_bits.copy()
        O.adam_bf16_sr(om_bits, np.ascontiguousarray(gg[:n_vi]), om[:n_vi], ov[:n_vi], lr, t, seed, 0)
        O.adam_bf16_sr(or_bits, np.ascontiguousarray(gg[n_vi:2 * n_vi]), om[n_vi:2 * n_vi], ov[n_vi:2 * n_vi], lr, t, seed, 1)
        O.adam(obn, np.ascontiguousarray(gg[2 * n_vi:]), om[2 * n_vi:], ov[2 * n_vi:], lr, t)
        moved += int((before != om_bits).sum())
        for dev_t, bits in ((b_mu, om_bits), (b_rho, or_bits)):
            got = dev_t.view(torch.int16).cpu().numpy().view(np.uint16)
            diff = np.abs(got.astype(np.int64) - bits.astype(np.int64))
            assert diff.max() <= 1 and (diff != 0).mean() < 2e-3, (t, diff.max(), (diff != 0).mean())
            bits[:] = got                                                 # re-anchor on the device's rounding decisions
        assert relerr(host(m), om) < 1e-6 and relerr(host(v), ov) < 1e-6 and relerr(host(d_bn), obn) < 1e-6
    assert moved > 0.3 * n_vi


# ---- 5. the per-fit update -----------------------------------------------------------------------------------------------------------------------
def test_elbo_update_fits_typed_against_single_fit(M):
    """test_elbo_update_fits_against_single_fit (tests/test_gpu_fitbatch.py) with the directions (forward, reverse, forward): its strides, sizes
    and tolerances; then a NaN row, and a row whose direction is no direction."""
    lib, sp, p_ = M._lib.lib(), M._lib.stream_ptr(), M._lib.ptr
    F, nv, nb, seed, t = 3, 1003, 37, 23, 4
    n = 2 * nv + nb
    stride, gstride = n + 5, n + 2
    temps, sigmas, lrs = [1e-4 * 2 ** f for f in range(F)], [5.0 * 2 ** f for f in range(F)], [1e-3 * (f + 1) for f in range(F)]
    ps = [float(np.float32(np.sqrt(a) * b + 1e-6)) for a, b in zip(temps, sigmas)]
    kts = [FWD, REV, FWD]

    def rows(s, lo, sc, width):
        r = np.zeros((F, width), np.float32)
        r[:, :n] = (lo + sc * O.normal_fill(seed, 2, s, 0, 0, F * n)).reshape(F, n)
        return r
    p0 = rows(0, 0.0, 0.1, stride); p0[:, nv:2 * nv] -= 3.0
    g0, m0 = rows(1, 0.0, 1e-2, gstride), rows(2, 0.0, 1e-3, stride)
    v0 = np.abs(rows(3, 0.0, 1e-4, stride))
    hyper = dev(np.array([[0.0, ps[f], temps[f], lrs[f]] for f in range(F)], np.float32))
    scratch = torch.zeros(lib.mfvi_elbo_update_fits_scratch_bytes(F), dtype=torch.uint8, device="cuda")

    def run(kl_types, nll):
        P, G, Mo, V = dev(p0), dev(g0), dev(m0), dev(v0)
        kl = torch.full((F,), -1.0, dtype=torch.float64, device="cuda"); dead = torch.zeros(F, dtype=torch.int32, device="cuda")
        d_kt, d_nll = dev(np.asarray(kl_types, np.int32)), dev(np.asarray(nll, np.float64))
        M._lib.check(lib.mfvi_elbo_update_fits_typed(p_(P), p_(G), p_(Mo), p_(V), nv, nb, stride, gstride, F, p_(hyper), p_(d_kt), 0.9, 0.999, 1e-8, t, p_(d_nll),
                                                     p_(dead), p_(kl), p_(scratch), sp))
        return [host(x) for x in (P, G, Mo, V, kl, dead)]
    runs = [run(kts, [0.3, 0.4, 0.5]) for _ in range(2)]
    for a, b in zip(*runs):
        assert np.array_equal(a, b)                                        # two calls bit-identical
    P, G, Mo, V, kl, dead = runs[0]
    assert not dead.any()
    assert np.array_equal(P[:, n:], p0[:, n:]) and np.array_equal(G[:, n:], g0[:, n:])      # nothing written between the rows
    s1 = torch.zeros(lib.mfvi_elbo_update_scratch_bytes(), dtype=torch.uint8, device="cuda")
    single = []
    for f in range(F):
        p1, g1, m1, v1 = dev(p0[f, :n]), dev(g0[f, :n]), dev(m0[f, :n]), dev(v0[f, :n])
        k1 = torch.zeros(1, dtype=torch.float64, device="cuda")
        M._lib.check(lib.mfvi_elbo_update_typed(p_(p1), p_(g1), p_(m1), p_(v1), nv, nb, 0.0, ps[f], temps[f], kts[f], lrs[f], 0.9, 0.999, 1e-8, t, p_(k1), p_(s1), sp))
        single.append([host(x) for x in (p1, g1, m1, v1)] + [float(k1)])
        for name, a, b in (("params", P[f, :n], p1), ("m", Mo[f, :n], m1), ("v", V[f, :n], v1), ("grads", G[f, :n], g1)):
            assert _ulp_diff(a, host(b)) <= 1, (f, name)
        assert relval(kl[f], float(k1), "per-fit kl against single-fit") <= 1e-12, f
        want = R.KL["forward" if kts[f] else "reverse"](p0[f, :nv], p0[f, nv:2 * nv], 0.0, ps[f])[0]
        assert relval(kl[f], want) < TOL_VALUE, f                         # each row in ITS direction
    assert abs(R.kl_forward(p0[1, :nv], p0[1, nv:2 * nv], 0.0, ps[1])[0] / kl[1] - 1.0) > 1e-2      # (the other direction would miss by far)
    # a NaN data term freezes its row and marks it dead; the others are what they were
    Pn, Gn, Mn, Vn, kln, deadn = run(kts, [0.3, float("nan"), 0.5])
    assert deadn.tolist() == [0, 1, 0] and kln[1] == kl[1]
    assert np.array_equal(Pn[1], p0[1]) and np.array_equal(Mn[1], m0[1]) and np.array_equal(Vn[1], v0[1]) and np.array_equal(Gn[1], g0[1])
    for f in (0, 2):
        assert np.array_equal(Pn[f], P[f]) and np.array_equal(Mn[f], Mo[f]) and np.array_equal(Vn[f], V[f]) and kln[f] == kl[f]
    # a direction outside {0, 1} cannot be refused on the host: the row is dead and untouched, its kl_out included
    Pb, Gb, Mb, Vb, klb, deadb = run([FWD, REV, 7], [0.3, 0.4, 0.5])
    assert deadb.tolist() == [0, 0, 1] and klb[2] == -1.0
    assert np.array_equal(Pb[2], p0[2]) and np.array_equal(Mb[2], m0[2]) and np.array_equal(Vb[2], v0[2]) and np.array_equal(Gb[2], g0[2])
    for f in (0, 1):
        assert np.array_equal(Pb[f], P[f]) and klb[f] == kl[f]


# ---- 6. the engine -------------------------------------------------------------------------------------------------------------------------------
def _target(task, S, seed):
    img = O.phantom(S, S, seed)
    if task == "ct":
        return O.radon_fwd(img, np.arange(0, 180., 4., dtype=np.float32))
    return O.noisy(img, 0.1, seed)


def _engine(M, task="den", S=32, K=2, seed=11, **kw):
    kw = dict(PRIOR01, **kw)
    eng = M.engine.ElboEngine(S, S, task=task, K=K, input_depth=8, lr=1e-3, seed=seed, net_kwargs=SMALL, autotune=False, **kw)
    eng.set_target(torch.from_numpy(_target(task, S, seed)))
    return eng


@pytest.mark.parametrize("task,dtype", [("den", "f32"), ("ct", "f32"), ("den", "bf16")])
def test_engine_step_is_grad_only_plus_the_unfused_forward_pair(M, task, dtype):
    L = M._lib; lib, sp, p_ = L.lib(), L.stream_ptr(), L.ptr
    a, b = _engine(M, task, kl_type="forward", param_dtype=dtype), _engine(M, task, kl_type="forward", param_dtype=dtype)
    assert a.kl_type == "forward" and abs(a.prior_sigma - 0.1) < 1e-4
    mu0, rho0, _ = (host(x).copy() for x in a.params_f32())
    a.step()
    b.grad_only(0, with_kl=False)
    mu, rho, bn = b.params_f32()
    p32 = torch.cat([mu, rho, bn]).contiguous()
    nv, n = b.n_vi, b.n_params
    klb = _kl(M, p32[:nv], p32[nv:2 * nv], 0.0, b.prior_sigma)
    _kl_bwd(M, p32[:nv], p32[nv:2 * nv], 0.0, b.prior_sigma, b.temp, b.dmu, b.drho)
    L.check(lib.mfvi_adam_step(p_(p32), p_(b.grads), p_(b.m), p_(b.v), n, b.lr, 0.9, 0.999, 1e-8, 1, sp))
    close = lambda x, y: float((x - y).abs().max()) <= 1e-6 * float(y.abs().max())
    assert close(a.grads[:n], b.grads[:n]) and close(a.m, b.m) and close(a.v, b.v)
    got = torch.cat(a.params_f32())
    if dtype == "bf16":      # stochastic rounding returns one of the two bf16 neighbours of the float32 update: within one bf16 ulp, 2^-7 |x|
        assert bool(((got[:2 * nv] - p32[:2 * nv]).abs() <= 2.0 ** -7 * p32[:2 * nv].abs()).all())
        assert float((got[2 * nv:] - p32[2 * nv:]).abs().max()) < 1e-6
    else:
        assert float((got - p32).abs().max()) < 1e-6
    want = R.kl_forward(mu0, rho0, 0.0, a.prior_sigma)[0]
    assert relval(a.losses()[1], want) < TOL_VALUE and relval(klb, want) < TOL_VALUE
    assert abs(R.kl_reverse(mu0, rho0, 0.0, a.prior_sigma)[0] / want - 1.0) > 1e-2
    # grad_only(with_kl=True), the K-sharded path's KL: the same direction
    b2 = _engine(M, task, kl_type="forward", param_dtype=dtype)
    b2.grad_only(0)
    assert relval(b2.losses()[1], want) < TOL_VALUE and close(b2.grads[:n], b.grads[:n])


@pytest.mark.parametrize("task", ["den", "ct"])
def test_device_step_and_graph_replay_are_bit_identical_forward(M, task):
    """tests/test_gpu_graph.py with kl_type='forward': the direction is a by-value launch argument, nothing of the capture changes."""
    n = 3
    ref = _engine(M, task, kl_type="forward")
    for _ in range(n):
        ref.step()
    dv = _engine(M, task, kl_type="forward").enable_device_step()
    for _ in range(n):
        dv.step()
    assert int(dv.step_dev) == n and int(dv.t_applied) == n
    assert torch.equal(dv.params, ref.params) and torch.equal(dv.m, ref.m) and torch.equal(dv.v, ref.v)
    gr = _engine(M, task, kl_type="forward").enable_graph(warmup=1)
    assert gr._graph is not None and gr.t == 1
    for _ in range(n - 1):
        gr.step()
    torch.cuda.synchronize()
    assert int(gr.step_dev) == n
    assert torch.equal(gr.params, ref.params) and torch.equal(gr.m, ref.m) and torch.equal(gr.v, ref.v)
    assert abs(gr.losses()[1] - ref.losses()[1]) <= 1e-12 * ref.losses()[1] and abs(dv.losses()[1] - ref.losses()[1]) <= 1e-12 * ref.losses()[1]
    rev = _engine(M, task)
    for _ in range(n):
        rev.step()
    assert not torch.equal(rev.params, ref.params)


@pytest.mark.parametrize("task,dtype", [("den", "f32"), ("ct", "f32"), ("den", "bf16")])
def test_reverse_engine_is_the_engine_without_the_argument(M, task, dtype):
    a, b = _engine(M, task, kl_type="reverse", param_dtype=dtype), _engine(M, task, param_dtype=dtype)
    assert a.kl_type == b.kl_type == "reverse"
    for _ in range(2):
        a.step(); b.step()
    for x, y in zip(a.params_f32(), b.params_f32()):
        assert torch.equal(x, y)
    assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and a.losses()[1] == b.losses()[1]


# ---- 7. the batches ------------------------------------------------------------------------------------------------------------------------------
def _row_engines_follow(M, batch, make_engine, kts):
    """Two steps of the batch; beside it, per row, the standalone engine of the row's direction under the row's RNG identity: eps of the global
    samples f K .. (its k0), and the row's perturbed input in place of its own draw (a standalone engine owns sample 0 of the INPUT stream;
    row 0's own draw is checked to be the batch's).  Each step starts from the row's state; bounds as the batch tests hold a row to an
    engine / the oracle: gradients 2e-4 of the largest, KL 1e-10, parameters max 2.5e-3, mean 5e-5 per step."""
    K, nv = batch.K, batch.n_vi
    engines = []
    for f, kt in enumerate(kts):
        eng = make_engine(f)
        assert eng.kl_type == kt == batch.kl_types[f] and eng.prior_sigma == batch.prior_sigma[f]
        engines.append(eng)
    for it in range(2):
        start = [{k: v.clone() for k, v in batch.fit(f).items() if k in ("params", "m", "v")} for f in range(len(kts))]
        batch.step()
        nll, kl, _ = batch.losses()
        for f, eng in enumerate(engines):
            eng.params.copy_(start[f]["params"]); eng.m.copy_(start[f]["m"]); eng.v.copy_(start[f]["v"])
            eng.t = it; eng.t_applied.fill_(it); eng.k0 = f * K
            if f == 0 and it == 0:
                eng.z0.copy_(batch.z0[0])
                eng._perturb(0)
                assert torch.equal(eng.z, batch.z[0])
            eng._perturb = lambda step, _e=eng, _f=f: _e.z.copy_(batch.z[_f])
            eng.step()
            row = batch.fit(f)
            g, ge = host(row["grads"]), host(eng.grads[:eng.n_params])
            for name, sl in (("dmu", slice(0, nv)), ("drho", slice(nv, 2 * nv)), ("dbn", slice(2 * nv, None))):
                assert relerr(g[sl], ge[sl], "row against engine " + name) < 2e-4, (f, it, name)
            assert relval(kl[f], eng.losses()[1], "row kl against engine") < 1e-10, (f, it)
            assert relval(nll[f], eng.losses()[0], "row nll against engine") < 1e-5, (f, it)
            d = (row["params"] - eng.params).abs()
            assert float(d.max()) < 2.5e-3 and float(d.mean()) < 5e-5, (f, it, float(d.max()), float(d.mean()))
            want = R.KL[kts[f]](host(start[f]["params"][:nv]), host(start[f]["params"][nv:2 * nv]), 0.0, batch.prior_sigma[f])[0]
            assert relval(kl[f], want) < TOL_VALUE, (f, it)
    assert not batch.dead.any()
    for f, kt in enumerate(kts):
        assert batch.to_engine(f).kl_type == kt


def test_fitbatch_mixed_directions(M):
    kts, F, K, seed = ["forward", "reverse", "forward"], 3, 2, 9
    temps, sigmas = [1e-4, 2e-4, 4e-4], 10.0
    tg = np.stack([O.noisy(O.phantom(32, 32, seed + f), 0.1, seed + f) for f in range(F)]).astype(np.float32)

    def make(**kw):
        fb = M.FitBatch(32, 32, F, task="den", K=K, input_depth=8, temp=temps, sigma=sigmas, lr=1e-3, seed=seed, net_kwargs=SMALL, autotune=False, **kw)
        fb.set_targets(torch.from_numpy(tg))
        return fb
    fb = make(kl_type=kts)
    assert fb.kl_types == kts and fb._kl_dev is not None and fb._kl_dev.tolist() == [1, 0, 1]

    def engine(f):
        eng = M.engine.ElboEngine(32, 32, task="den", K=K, input_depth=8, temp=temps[f], sigma=sigmas, lr=1e-3, seed=seed, net_kwargs=SMALL, autotune=False, kl_type=kts[f])
        eng.set_target(torch.from_numpy(tg[f]))
        return eng
    _row_engines_follow(M, fb, engine, kts)
    # all reverse, named or not: the untyped update, nothing allocated, the same bits
    a, b = make(kl_type="reverse"), make()
    assert a._kl_dev is None and b._kl_dev is None and a.kl_types == b.kl_types == ["reverse"] * F
    for _ in range(2):
        a.step(); b.step()
    assert torch.equal(a.params, b.params) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and torch.equal(a.kl, b.kl)
    # row 1 (reverse) of the mixed batch is row 1 of the all-reverse batch: a row's direction is its own
    c = make(kl_type=kts)
    for _ in range(2):
        c.step()
    assert float((c.params[1] - b.params[1]).abs().max()) < 1e-6 and not torch.equal(c.params[0], b.params[0])      # (far below one Adam step)


def test_ctvolume_mixed_directions(M):
    kts, S, D, K, seed = ["forward", "reverse"], 32, 2, 1, 9
    sinos = np.stack([_target("ct", S, 20 + d) for d in range(D)]).astype(np.float32)
    vol = M.CtVolume(S, D, K=K, input_depth=8, lr=1e-3, seed=seed, net_kwargs=SMALL, autotune=False, kl_type=kts, **PRIOR01)
    vol.set_sinograms(torch.from_numpy(sinos))
    assert len(vol.groups) == 1 and vol.kl_types == kts

    def engine(d):
        eng = M.engine.ElboEngine(S, S, task="ct", K=K, input_depth=8, lr=1e-3, seed=seed, net_kwargs=SMALL, autotune=False, kl_type=kts[d], **PRIOR01)
        eng.set_target(torch.from_numpy(sinos[d]))
        return eng
    _row_engines_follow(M, vol, engine, kts)
    assert M.CtVolume(S, D, K=K, input_depth=8, seed=seed, net_kwargs=SMALL, autotune=False, kl_type="reverse")._kl_dev is None


def test_inpaintbatch_mixed_directions(M):
    kts, H, W, F, K, seed = ["reverse", "forward"], 24, 40, 2, 2, 13
    img = np.stack([np.stack([O.phantom(H, W, seed + 3 * f + c) for c in range(3)]) for f in range(F)]).astype(np.float32)
    mask = (np.stack([O.uniform_fill(seed, 9, f, 0, H * W).reshape(1, H, W) for f in range(F)]) > 0.2).astype(np.float32)
    ib = M.InpaintBatch(H, W, F, K=K, input_depth=8, lr=1e-3, seed=seed, net_kwargs=INP_KW, autotune=False, kl_type=kts, **PRIOR01)
    ib.set_targets(torch.from_numpy(img), torch.from_numpy(mask))
    assert ib.kl_types == kts

    def engine(f):
        eng = M.engine.ElboEngine(H, W, task="inp", K=K, input_depth=8, lr=1e-3, seed=seed, net_kwargs=INP_KW, autotune=False, kl_type=kts[f], **PRIOR01)
        eng.set_target(torch.from_numpy(img[f]), torch.from_numpy(mask[f]))
        return eng
    _row_engines_follow(M, ib, engine, kts)
    assert M.InpaintBatch(H, W, F, K=K, input_depth=8, seed=seed, net_kwargs=INP_KW, autotune=False, kl_type="reverse")._kl_dev is None


# ---- 8. the drop-in ------------------------------------------------------------------------------------------------------------------------------
def _dropin(M, gold, kl_type, reparam="", flat=False):
    net = M.get_net(8, 'skip', 'reflection', skip_n33d=[8, 16], skip_n33u=[8, 16], skip_n11=4, num_scales=2, n_channels=2, upsample_mode='bilinear')
    net = M.MeanFieldVI(net, prior={'mu': 0, 'sigma': 0.1}, kl_type=kl_type, reparam=reparam, device=torch.device('cuda'), seed=3, autotune=False,
                        flat_parameters=flat)
    sd = {str(k): torch.from_numpy(gold["net_p%d" % i]) for i, k in enumerate(gold["net_keys"])}
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(".W_" not in k and ".bias_" not in k for k in missing)
    return net


@pytest.mark.parametrize("flat", [False, True])
def test_dropin_forward_kl_and_its_gradients(M, gold, flat):
    net = _dropin(M, gold, "forward", flat=flat)
    layers = [(k, m) for k, m in net.named_modules() if isinstance(m, M.bayes.Conv2dRT)]
    assert [k for k, _ in layers] == [str(k) for k in gold["net_layers"]] and all(m.kl_type == "forward" for _, m in layers)
    for (k, m), want in zip(layers, gold["net_layer_kl"]):
        assert relval(float(m._kl), float(want), "layer _kl") < TOL_VALUE, k
    kl = net.kl()
    assert kl.shape == (1,) and kl.dtype == torch.float32
    assert relval(float(kl), float(gold["net_kl"])) < TOL_VALUE and relval(float(kl), float(gold["net_kl64"])) < TOL_VALUE
    (0.5 * kl).backward()
    m0, s0 = (float(v) for v in gold["net_prior"])
    flat_g = next(net.parameters()).grad if flat else None
    for k, m in layers:
        for part, off, n in (("W", m._w_off, m.W_mu.numel()), ("bias", m._b_off, m.out_channels if m._has_bias else 0)):
            if not n:
                continue
            pm, pr = getattr(m, part + "_mu"), getattr(m, part + "_rho")
            _, dm, dr = R.kl_forward(host(pm).ravel(), host(pr).ravel(), m0, s0)
            gm, gr = (flat_g[off:off + n], flat_g[net.n_vi + off:net.n_vi + off + n]) if flat else (pm.grad.reshape(-1), pr.grad.reshape(-1))
            assert relerr(host(gm), 0.5 * dm) < TOL_GRAD and relerr(host(gr), 0.5 * dr) < TOL_GRAD, (k, part)
    if flat:
        assert not flat_g[2 * net.n_vi:].any()


def test_dropin_any_other_string_is_forward_and_local_reparam_takes_the_same_kl(M, gold):
    fwd = float(_dropin(M, gold, "forward").kl())
    other = _dropin(M, gold, "fwd")
    same = lambda a, b: abs(a - b) <= 1e-6 * abs(b)      # (the unfused sum adds its blocks by atomics: not defined to the last bit)
    assert same(float(other.kl()), fwd) and all(m.kl_type == "fwd" for m in other.modules() if isinstance(m, M.bayes.Conv2dRT))
    lrt = _dropin(M, gold, "forward", reparam="local")
    assert same(float(lrt.kl()), fwd) and all(isinstance(m, M.bayes.Conv2dLRT) for m in lrt._vi)
    rev = _dropin(M, gold, "reverse")
    mu, rho, _ = _net_flat(gold)
    assert relval(float(rev.kl()), R.kl_reverse(mu, rho, *(float(v) for v in gold["net_prior"]))[0]) < TOL_VALUE
    assert abs(float(rev.kl()) / fwd - 1.0) > 1e-2
    with pytest.raises(NotImplementedError):      # the other refusals stay
        M.MeanFieldVI(M.get_net(8, 'skip', 'reflection', skip_n33d=[8, 16], skip_n33u=[8, 16], skip_n11=4, num_scales=2, n_channels=2, upsample_mode='bilinear'),
                      prior={'mu': 0, 'sigma': 0.1, 'pi': 0.5}, kl_type="forward", device=torch.device('cuda'), reparam='')


# ---- 9. the runner -------------------------------------------------------------------------------------------------------------------------------
def test_runner_kl_type_forward(M, tmp_path, capsys):
    temp, sigma = 1e-4, 10.0
    cfg = dict(bo_params=dict(temp=dict(candidates=[temp]), sigma=dict(candidates=[sigma])),
               run_params=dict(img="phantom", num_iter=4, lr=1e-3, seed=1, p_sigma=0.1, input_depth=8, show_every=2, plot=False, save=True,
                               net_kwargs=SMALL, save_path=str(tmp_path / "logs")))
    path = str(tmp_path / "cfg.json")
    json.dump(cfg, open(path, "w"))
    out = M.runner.main(["--task", "denoising", "--config", path, "--imsize", "32", "--kl-type", "forward"])
    text = capsys.readouterr().out
    assert len(out) == 1 and out[0]["engine"].kl_type == "forward" and os.path.exists(os.path.join(out[0]["run_dir"], "save.npz"))
    assert "kl_type" in open(os.path.join(out[0]["run_dir"], "locals.txt")).read()
    kl0 = float(re.search(r"iter\s+0\s+loss\s+\S+\s+nll\s+\S+\s+kl\s+(\S+)", text).group(1))      # printed with five digits
    init = M.engine.ElboEngine(32, 32, task="den", K=1, input_depth=8, temp=temp, sigma=sigma, lr=1e-3, seed=1, net_kwargs=SMALL, autotune=False)
    mu, rho = host(init.mu), host(init.rho)
    want = R.kl_forward(mu, rho, 0.0, init.prior_sigma)[0]
    assert abs(kl0 - want) <= 1e-4 * want and abs(R.kl_reverse(mu, rho, 0.0, init.prior_sigma)[0] - want) > 1e-2 * want
    # the config's run_params.kl_type is read too
    cfg["run_params"]["kl_type"] = "forward"
    json.dump(cfg, open(path, "w"))
    out = M.runner.main(["--task", "denoising", "--config", path, "--imsize", "32", "--num-iter", "1"])
    assert out[0]["engine"].kl_type == "forward"
    capsys.readouterr()


def test_runner_batches_record_the_directions(M, tmp_path, capsys):
    base = {"task", "temp", "sigma", "lr", "prior_sigma", "K", "seed", "num_iter", "iterations", "psnr_gt_sm", "nll", "kl", "recon", "dead"}
    cfg = dict(bo_params=dict(temp=dict(candidates=[1e-4, 2e-4]), sigma=dict(candidates=[10.0])),
               run_params=dict(img="phantom", num_iter=4, lr=1e-3, seed=1, p_sigma=0.1, input_depth=8, show_every=2, plot=False, save=True,
                               net_kwargs=SMALL, save_path=str(tmp_path / "logs")))
    path = str(tmp_path / "cfg.json")
    json.dump(cfg, open(path, "w"))
    res = M.runner.main(["--task", "denoising", "--config", path, "--imsize", "32", "--fits-per-launch", "2", "--kl-type", "forward"])
    capsys.readouterr()
    assert len(res) == 2
    (d,) = os.listdir(str(tmp_path / "logs"))
    z = np.load(os.path.join(str(tmp_path / "logs"), d, "batch.npz"), allow_pickle=False)
    assert set(z.files) == base | {"kl_type"} and z["kl_type"].tolist() == ["forward", "forward"]
    # per-job directions in one batch: the same image under both, one set of launches
    jobs = [dict(img="phantom", temp=1e-4, sigma=10.0, kl_type="forward"), dict(img="phantom", temp=1e-4, sigma=10.0)]
    kw = dict(imsize=(32, 32), num_iter=4, lr=1e-3, input_depth=8, seed=1, show_every=2, K=1, net_kwargs=SMALL, autotune=False)
    r = M.runner.run_fit_batch("den", jobs, save_path=str(tmp_path / "mixed"), **kw)
    z = np.load(os.path.join(r["run_dir"], "batch.npz"), allow_pickle=False)
    assert set(z.files) == base | {"kl_type"} and z["kl_type"].tolist() == ["forward", "reverse"] and r["batch"].kl_types == ["forward", "reverse"]
    fb = r["batch"]
    p = host(fb.params)      # init='shared': both fits started from the same parameters, so iteration 0's KL is that of one point in both directions
    assert z["kl"].shape == (3, 2) and abs(z["kl"][0, 0] / z["kl"][0, 1] - 1.0) > 1e-2 and not np.array_equal(p[0], p[1])
    r = M.runner.run_fit_batch("den", [dict(j, kl_type="reverse") for j in jobs], save_path=str(tmp_path / "rev"), **kw)
    assert set(np.load(os.path.join(r["run_dir"], "batch.npz")).files) == base
    r = M.runner.run_ct_volume("phantom:2", 1e-4, 10.0, imsize=(32, 32), num_iter=2, input_depth=8, seed=1, show_every=2, net_kwargs=SMALL, autotune=False,
                               kl_type=["reverse", "forward"], save_path=str(tmp_path / "vol"))
    assert np.load(os.path.join(r["run_dir"], "volume.npz"), allow_pickle=False)["kl_type"].tolist() == ["reverse", "forward"]
