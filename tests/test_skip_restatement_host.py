"""The float64 statement of the hour-glass (tests/skip_restatement.py) against the C oracle, on the CPU: it must agree with the oracle on
every net of the suite before the GPU tests lean on it, and the tolerances those tests derive from it must be able to see an indexing or
border-weight error of the concat."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import note_margin as _note      # noqa: E402
from oracle import oracle as O      # noqa: E402
import oddmap_cases as C      # noqa: E402
import oracle_program      # noqa: E402
from skip_restatement import SkipNet64, relerr as _relerr      # noqa: E402
from test_gpu_parity import NET_CASES, NET_SEEDS      # noqa: E402


def relerr(a, b):
    v = _relerr(a, b)
    _note(v, "relerr")
    return v


def _program(kw):
    import mfvi_dip_mia_amd as M
    return M.skip_program(**kw)


ALL_NETS = dict(NET_CASES, **{"concat_" + k: v[0] for k, v in C.CONCAT_CASES.items()})


@pytest.mark.parametrize("name", list(ALL_NETS))
def test_layout_is_the_programs(name):
    """The statement counts its own parameter offsets; they are the ones Program assigns."""
    kw = ALL_NETS[name]
    P, _, _, _ = _program(kw)
    net = SkipNet64(**kw)
    assert (net.n_vi, net.n_bn) == (P.n_vi, P.n_bn)
    assert [(l["cin"], l["cout"], l["k"], l["stride"], l["w_off"], l["b_off"]) for l in net.layers] == \
           [(l["cin"], l["cout"], l["k"], l["stride"], l["w_off"], l["b_off"]) for l in P.layers]
    assert [(b["C"], b["off"]) for b in net.bns] == [(b["C"], b["off"]) for b in P.bns]


def test_oracle_program_is_net_forward():
    """The op-by-op evaluation on the oracle's primitives repeats oracle.net_forward / tape.backward call for call on a net both express."""
    kw = NET_CASES["crop_two_scale_35x45"]
    seed, step, sample = 77, 9, 2
    P, zin, out_id, names = _program(kw)
    mu, rho, bnp, z, dout = C.net_inputs(kw, seed, P, n=1)
    net = O.make_net(**kw)
    ref, tape = O.net_forward(net, mu, rho, bnp, z, seed, step, sample)
    a, b, c_, dzr = tape.backward(dout[0], P.n_vi, P.n_bn, want_dz=True)
    cat = tape.cat(1)
    tape.free()
    got = oracle_program.run(P, zin, out_id, mu, rho, bnp, z, seed, step, sample, dout[0])
    assert np.array_equal(got["out"], ref) and np.array_equal(got["dz"], dzr)
    assert np.array_equal(got["raw"][names[1]["cat"]].ravel(), cat)
    assert _relerr(got["dmu"], a) < 1e-12 and _relerr(got["drho"], b) < 1e-12 and _relerr(got["dbn"], c_) < 1e-12


@pytest.mark.parametrize("name", list(NET_CASES))
def test_agrees_with_the_oracle_on_the_suites_nets(name):
    """Output, dz, dmu, drho, dbn of every NET_CASES entry, with the inputs and the tolerances of test_small_nets_fwd_bwd."""
    kw = NET_CASES[name]
    seed, step, k0, n = NET_SEEDS.get(name, 77), 9, 2, 3
    P, zin, out_id, _ = _program(kw)
    mu, rho, bnp, z, dout = C.net_inputs(kw, seed, P, n=n)
    onet, net = O.make_net(**kw), SkipNet64(**kw)
    tot_o = [np.zeros(P.n_vi), np.zeros(P.n_vi), np.zeros(P.n_bn)]; tot_r = [np.zeros(P.n_vi), np.zeros(P.n_vi), np.zeros(P.n_bn)]
    for i in range(n):
        out, tape = O.net_forward(onet, mu, rho, bnp, z, seed, step, k0 + i)
        a, b, c_, dz = tape.backward(dout[i], P.n_vi, P.n_bn, want_dz=True)
        tape.free()
        r = net.run(mu, rho, bnp, z, seed, step, k0 + i, dout[i])
        assert relerr(out, r["out"]) < C.OUT_TOL, ("out", i)
        assert relerr(dz, r["dz"]) < C.GRAD_TOL, ("dz", i)
        for t, v in zip(tot_o, (a, b, c_)):
            t += v
        for t, q in zip(tot_r, ("dmu", "drho", "dbn")):
            t += r[q]
    for o, r, q in zip(tot_o, tot_r, ("dmu", "drho", "dbn")):
        assert relerr(o, r) < C.GRAD_TOL, q


@pytest.mark.parametrize("name", list(C.CONCAT_CASES))
def test_agrees_with_the_oracle_on_the_concat_cases(name):
    """Every quantity the GPU test compares: e32, the oracle's distance to the statement, is within the suite's tolerance for it.  Where
    oracle.net_forward expresses the net (bilinear, with a skip branch) it is the oracle; elsewhere its primitives op by op."""
    kw, seed = C.CONCAT_CASES[name]
    ref = C.concat_reference(name)
    for q, e in sorted(ref["e32"].items()):
        _note(e, "e32 " + q)
        print("%s e32 %-6s %.2e" % (name, q, e))
        assert e < C.cap(q), q
    if kw.get("upsample_mode", "bilinear") == "bilinear" and kw["ns"][0]:
        mu, rho, bnp, z, dout = ref["inputs"]
        P, onet = ref["P"], O.make_net(**kw)
        tot = [np.zeros(P.n_vi), np.zeros(P.n_vi), np.zeros(P.n_bn)]
        for i in range(C.N):
            out, tape = O.net_forward(onet, mu, rho, bnp, z, seed, C.STEP, C.K0 + i)
            grads = tape.backward(dout[i], P.n_vi, P.n_bn, want_dz=True)
            tape.free()
            assert relerr(out, ref["ref"][i]["out"]) < C.OUT_TOL and relerr(grads[3], ref["ref"][i]["dz"]) < C.GRAD_TOL
            for t, v in zip(tot, grads[:3]):
                t += v
        for t, q in zip(tot, ("dmu", "drho", "dbn")):
            assert relerr(t, ref["tot"][q]) < C.GRAD_TOL, q


@pytest.mark.parametrize("name", list(C.CONCAT_CASES) + ["crop_two_scale_35x48", "crop_three_scale_35x132", "crop_two_scale_21x99"])
def test_new_cases_are_well_conditioned(name):
    """The inputs leave the comparison to the kernels (oddmap_cases.KINK / OFF_CENTRE): no BN output under a LeakyReLU within 2e-6 of its
    tensor's scale of zero, in any sample; in the concat cases, which are held to a few 1e-6, no channel whose mean is more than 4 standard
    deviations.  (The nets of test_small_nets_fwd_bwd keep that test's all-positive input and its tolerances.)"""
    if name in C.CONCAT_CASES:
        ref = C.concat_reference(name)
        conds = [C.conditioning(ref["P"], o) for o in ref["ora"]]
    else:
        kw, seed = NET_CASES[name], NET_SEEDS.get(name, 77)
        P, zin, out_id, _ = _program(kw)
        mu, rho, bnp, z, _d = C.net_inputs(kw, seed, P, n=3)
        conds = [C.conditioning(P, oracle_program.run(P, zin, out_id, mu, rho, bnp, z, seed, 9, 2 + i)) for i in range(3)]
    kink, off = min(c[0] for c in conds), max(c[1] for c in conds)
    print("%s: nearest BN output to the kink %.2e of the scale, largest |mean| / std %.1f" % (name, kink, off))
    assert kink >= C.KINK
    assert name not in C.CONCAT_CASES or off <= C.OFF_CENTRE


@pytest.mark.parametrize("name", list(C.CONCAT_CASES))
def test_tolerances_see_a_wrong_concat(name):
    """Three wrong statements of the concat: (a) the crop drops the FIRST row / column (cases with a crop), (b) align_corners=True (bilinear
    cases), (c) the up-sampled branch shifted by one low-res column.  Each differs from the true statement by at least 10x the tolerance
    the GPU test applies, in the concat tensor and in the gradient of the up-sampled branch."""
    kw, seed = C.CONCAT_CASES[name]
    ref = C.concat_reference(name)
    mu, rho, bnp, z, dout = ref["inputs"]
    wrongs = ["shift"]
    if kw.get("upsample_mode", "bilinear") == "bilinear":
        wrongs.append("align_corners")
    if kw["ns"][0] and (kw["H"] % 2 or kw["W"] % 2):
        wrongs.append("crop_first")
    true = ref["ref"][0]
    for wrong in wrongs:
        bad = ref["net"].run(mu, rho, bnp, z, seed, C.STEP, C.K0, dout[0], wrong=wrong)
        for q, a, b in (("cat", bad["cat"][0], true["cat"][0]), ("g_deep", bad["g_deep"][0], true["g_deep"][0])):
            d, t = _relerr(a, b), C.tol(ref["e32"][q], C.cap(q))
            print("%s %-13s %-6s differs by %.2e, tolerance %.2e" % (name, wrong, q, d, t))
            assert d >= 10 * t, (wrong, q, d, t)
