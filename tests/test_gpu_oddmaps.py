"""Odd-sized maps on the fast kernels: the concat / up-sample kernels at every switch of their launchers, and the
matrix-core convolutions with an odd number of rows, against the float64 statement of tests/skip_restatement.py.

Tolerance of every comparison with the float64 statement: tol = max(4 * e32, 2e-6), capped by the tolerance test_small_nets_fwd_bwd applies
to the quantity.  e32 is the distance of the C oracle (fp32 on the host) to the statement: oracle and GPU are two fp32 evaluations with
different summation orders, so their errors against float64 have the same size, and the factor 4 covers the spread between orders; 2e-6 is
the tightest tolerance the suite holds an fp32 kernel to (test_single_conv_fwd_bwd, forward).  Nothing of it comes from the kernels."""
import numpy as np
import pytest

from conftest import note_margin as _note

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle as O      # noqa: E402
import oddmap_cases as C      # noqa: E402
import oracle_program      # noqa: E402
import skip_restatement as S      # noqa: E402
from inp_restatement import torch_program      # noqa: E402
from test_gpu_parity import M, dev, host      # noqa: E402,F401  (M is a fixture)


def hold(dist, e32, cap, what):
    """Assert a GPU distance under the tolerance rule; both figures go on record."""
    t = C.tol(e32, cap)
    _note(e32, "e32 %s" % (what,)); _note(dist, "gpu %s" % (what,))
    print("%-28s gpu %.2e   e32 %.2e   tol %.2e" % (what, dist, e32, t))
    assert dist < t, (what, dist, e32, t)


@pytest.mark.parametrize("name", list(C.CONCAT_CASES))
def test_concat_upsample_at_the_switches(M, name):
    """One-scale nets whose concat reaches one branch of launch_concat_up_fwd / launch_concat_up_bwd each (the table in oddmap_cases.py):
    the raw concat tensor, its BN sums, the gradients at the concat tensor and at its two inputs, and the net end to end."""
    ref = C.concat_reference(name)
    P, names, e = ref["P"], ref["names"][0], ref["e32"]
    kw, seed = C.CONCAT_CASES[name]
    mu, rho, bnp, z, dout = ref["inputs"]
    n = C.N
    plan = P.compile(ref["zin"], ref["out_id"], max_samples=n)
    d_mu, d_rho, d_bn, d_z = dev(mu), dev(rho), dev(bnp), dev(z)
    out = host(plan.forward(d_mu, d_rho, d_bn, d_z, seed, C.STEP, C.K0, n))
    cats = [host(plan.read_tensor(names["cat"], i, 0)) for i in range(n)]
    sums = [host(plan.read_tensor(names["cat"], i, 2)) for i in range(n)]
    dmu = torch.zeros_like(d_mu); drho = torch.zeros_like(d_rho); dbn = torch.zeros_like(d_bn)
    dz = torch.empty((n,) + z.shape, device="cuda")
    plan.backward(d_mu, d_rho, d_bn, d_z, seed, C.STEP, C.K0, n, dev(dout), dmu, drho, dbn, dz=dz)
    dz = host(dz)
    for i in range(n):
        r = ref["ref"][i]
        hold(S.relerr(cats[i], r["cat"][0]), e["cat"], C.cap("cat"), "cat[%d]" % i)
        hold(C.stat_err(sums[i], r["sums"][0], r["cat"][0]), e["sums"], C.cap("sums"), "sums[%d]" % i)
        for q, tid in (("g_cat", names["cat"]), ("g_skip", names["skip"]), ("g_deep", names["d2"])):
            if tid is not None:
                hold(S.relerr(host(plan.read_tensor(tid, i, 1)), r[q][0]), e[q], C.cap(q), "%s[%d]" % (q, i))
        hold(S.relerr(out[i], r["out"]), e["out"], C.cap("out"), "out[%d]" % i)
        hold(S.relerr(dz[i], r["dz"]), e["dz"], C.cap("dz"), "dz[%d]" % i)
    for q, got in (("dmu", dmu), ("drho", drho), ("dbn", dbn)):
        hold(S.relerr(host(got), ref["tot"][q]), e[q], C.cap(q), q)


def _families(M, plan, op):
    lib = M._lib.lib()
    return lib.mfvi_plan_last_kernel(plan.handle, op, 0), lib.mfvi_plan_last_kernel(plan.handle, op, 1)


@pytest.mark.parametrize("case", C.CONV_CASES, ids=lambda c: "-".join(map(str, c)))
def test_conv_odd_rows_on_the_matrix_cores(M, case):
    """Single layers as in test_single_conv_fwd_bwd, against conv2d behind a reflection pad in float64; the kernel families prove that the
    matrix-core kernels served them: forward 1 / 2 where W % 4 == 0 (else the generic kernel, 0), backward-data nonzero everywhere."""
    cin, cout, k, stride, H, W = case
    seed, step, k0, n = 1000 + cin + cout, 5, 3, 2
    P = M.Program()
    zin = P.tensor(cin, H, W)
    out = P.tensor(cout, *P.conv_out_hw(zin, k, stride))
    P.conv(zin, out, k, stride)
    plan = P.compile(zin, out, max_samples=n)
    nw = cout * cin * k * k
    mu = 0.1 * O.normal_fill(seed, 2, 0, 0, 0, nw + cout); rho = -3 + 0.1 * O.normal_fill(seed, 2, 1, 0, 0, nw + cout)
    x = O.normal_fill(seed, 2, 2, 0, 0, cin * H * W).reshape(cin, H, W)
    d_mu, d_rho, d_x = dev(mu), dev(rho), dev(x)
    bn = torch.zeros(1, device="cuda")
    y = plan.forward(d_mu, d_rho, bn, d_x, seed, step, k0, n)
    dy = O.normal_fill(seed, 2, 3, 0, 0, n * y[0].numel()).reshape(tuple(y.shape))
    dmu = torch.zeros_like(d_mu); drho = torch.zeros_like(d_rho); dbn = torch.zeros(1, device="cuda")
    dz = torch.empty((n, cin, H, W), device="cuda")
    plan.backward(d_mu, d_rho, bn, d_x, seed, step, k0, n, dev(dy), dmu, drho, dbn, dz=dz)
    fwd, bwd = _families(M, plan, 0)
    print("%s: kernel family forward %d, backward-data %d" % (case, fwd, bwd))
    assert (fwd in (1, 2)) if W % 4 == 0 else fwd == 0, ("forward family", fwd)
    assert bwd != 0, "backward-data ran on the generic kernel"
    yh, dzh = host(y), host(dz)
    mu64, rho64 = torch.tensor(mu.astype(np.float64)), torch.tensor(rho.astype(np.float64))
    sig = 1 / (1 + np.exp(-rho.astype(np.float64)))
    lay = dict(cin=cin, cout=cout, k=k, w_off=0, b_off=nw)
    tot = dict(r_dmu=np.zeros(nw + cout), r_drho=np.zeros(nw + cout), o_dmu=np.zeros(nw + cout), o_drho=np.zeros(nw + cout))
    for i in range(n):
        ew = O.eps(seed, step, k0 + i, 0, 0, nw).astype(np.float64); eb = O.eps(seed, step, k0 + i, 0, 1, cout).astype(np.float64)
        w64, b64 = S.sampled(mu64, rho64, lay, seed, step, k0 + i, 0)
        r_y, r_dx, r_dw, r_db = S.conv_case64(x, w64.numpy(), b64.numpy(), stride, dy[i])
        w = O.reparam(mu[:nw], rho[:nw], ew).reshape(cout, cin, k, k); b = O.reparam(mu[nw:], rho[nw:], eb)
        o_dx, o_dw, o_db = O.conv_bwd(x, w, stride, dy[i])
        hold(S.relerr(yh[i], r_y), S.relerr(O.conv_fwd(x, w, b, stride), r_y), C.OUT_TOL, "fwd[%d]" % i)
        hold(S.relerr(dzh[i], r_dx), S.relerr(o_dx, r_dx), C.GRAD_TOL, "dx[%d]" % i)
        for pre, dw, db in (("r_", r_dw, r_db), ("o_", o_dw, o_db)):
            tot[pre + "dmu"][:nw] += dw.ravel(); tot[pre + "dmu"][nw:] += db
            tot[pre + "drho"][:nw] += dw.ravel() * ew * sig[:nw]; tot[pre + "drho"][nw:] += db * eb * sig[nw:]
    hold(S.relerr(host(dmu), tot["r_dmu"]), S.relerr(tot["o_dmu"], tot["r_dmu"]), C.GRAD_TOL, "dmu")
    hold(S.relerr(host(drho), tot["r_drho"]), S.relerr(tot["o_drho"], tot["r_drho"]), C.GRAD_TOL, "drho")


@pytest.mark.parametrize("shape", [(16, 16, 1, 9, 12), (16, 8, 2, 9, 12), (16, 16, 1, 35, 48), (16, 8, 2, 35, 48)], ids=lambda c: "-".join(map(str, c)))
def test_conv_odd_rows_behind_a_batchnorm(M, shape):
    """The 3x3 layers between BatchNorms (1x1 -> BN + act -> 3x3 at stride 1 / 2 -> BN + act -> 1x1, the chain of _conv_bn_plan): backward-data
    normalises its gradient on load and, at stride 1, folds in its epilogue.  Reference: the float64 interpreter of layer programs
    (tests/inp_restatement.py), e32 from the oracle's primitives op by op."""
    cin, cout, stride, H, W = shape
    n, seed, step, k0 = 2, 77, 3, 1
    P = M.Program()
    zin = P.tensor(cin, H, W)
    x = P.tensor(cin, H, W); P.conv(zin, x, 1, 1); P.set_bn(x, act=True)
    y = P.tensor(cout, *P.conv_out_hw(x, 3, stride)); P.conv(x, y, 3, stride); P.set_bn(y, act=True)
    out = P.tensor(2, P.tensors[y]["H"], P.tensors[y]["W"]); P.conv(y, out, 1, 1)
    plan = P.compile(zin, out, n)
    mu, rho, bnp = C.params(P, seed)
    z = O.normal_fill(seed, 2, 2, 0, 0, cin * H * W).reshape(cin, H, W)
    oshape = (n, 2, P.tensors[out]["H"], P.tensors[out]["W"])
    dout = O.normal_fill(seed, 2, 3, 0, 0, int(np.prod(oshape))).reshape(oshape)
    d_mu, d_rho, d_bn, d_z = dev(mu), dev(rho), dev(bnp), dev(z)
    o = host(plan.forward(d_mu, d_rho, d_bn, d_z, seed, step, k0, n))
    dmu = torch.zeros_like(d_mu); drho = torch.zeros_like(d_rho); dbn = torch.zeros_like(d_bn)
    dz = torch.empty((n, cin, H, W), device="cuda")
    plan.backward(d_mu, d_rho, d_bn, d_z, seed, step, k0, n, dev(dout), dmu, drho, dbn, dz=dz)
    fwd, bwd = _families(M, plan, 1)
    print("%s: kernel family forward %d, backward-data %d" % (shape, fwd, bwd))
    assert fwd in (1, 2) and bwd != 0, ("kernel families of the 3x3 layer", fwd, bwd)
    dz = host(dz)
    tot_r = [0.0, 0.0, 0.0]; tot_o = [0.0, 0.0, 0.0]
    for i in range(n):
        lv = [torch.tensor(np.asarray(a, np.float64), requires_grad=True) for a in (mu, rho, bnp, z)]
        r = torch_program(P, zin, out, lv[0], lv[1], lv[2], lv[3], seed, step, k0 + i)
        (r * torch.tensor(dout[i].astype(np.float64))).sum().backward()
        oc = oracle_program.run(P, zin, out, mu, rho, bnp, z, seed, step, k0 + i, dout[i])
        hold(S.relerr(o[i], r.detach().numpy()), S.relerr(oc["out"], r.detach().numpy()), C.OUT_TOL, "out[%d]" % i)
        hold(S.relerr(dz[i], lv[3].grad.numpy()), S.relerr(oc["dz"], lv[3].grad.numpy()), C.GRAD_TOL, "dz[%d]" % i)
        for j, q in enumerate(("dmu", "drho", "dbn")):
            tot_r[j] = tot_r[j] + lv[j].grad.numpy(); tot_o[j] = tot_o[j] + oc[q]
    for j, (q, got) in enumerate((("dmu", dmu), ("drho", drho), ("dbn", dbn))):
        hold(S.relerr(host(got), tot_r[j]), S.relerr(tot_o[j], tot_r[j]), C.GRAD_TOL, q)
