"""The plan executor's fork / join paths (csrc/plan_forward.hip, csrc/plan_backward.hip, vocabulary in csrc/plan_internal.h) give the same
results and route every convolution to the same kernel family whichever of them a pass takes: events on the kernels' packets (default),
no side stream, plain event records (per-kernel profiling, capture mode), and the gradient split on a caller's stream.  Net: the smallest
hour-glass of test_gpu_skipfuse.py — skip-branch convolutions that fork in the forward, a convolution that reads the net input, fused-fold
layers, the skip convolution inside the fold, concats.  Reference: the oracle's tape, as there (models/skip.py:58-134)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_parity import M, dev, host, relerr, _net_params      # noqa: F401  (M is a fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KW = dict(H=32, W=32, input_depth=8, n_out=2, nd=(16, 32), nu=(16, 32), ns=(4, 4))
SEED, STEP, K0, N = 83, 2, 1, 2
MODES = ["default", "no_side", "profile", "capture", "split"]


def _run(M, R, mode, want_dz):
    """forward, backward, forward, backward on a fresh plan (the forward forks only once a backward has created the side stream);
    -> out, dmu, drho, dbn, dz of the second iteration and the kernel-family table."""
    P, zin, out_id, _ = M.skip_program(KW["H"], KW["W"], KW["input_depth"], KW["n_out"], KW["nd"], KW["nu"], KW["ns"])
    plan = P.compile(zin, out_id, max_samples=N)
    lib = M._lib.lib()
    split = None
    if mode == "no_side":
        plan.side_stream(False)
    elif mode == "profile":
        plan.profile(1)
    elif mode == "capture":
        M._lib.check(lib.mfvi_plan_set_capture_mode(plan.handle, 1))
    elif mode == "split":
        split = torch.cuda.Stream()
        op, _off = plan.choose_grad_split(0.5)      # (parameter offsets grow with the op index: every conv op owns a tail)
        plan.grad_split(op, split)
    d_mu, d_rho, d_bn, d_z, d_dout = dev(R["mu"]), dev(R["rho"]), dev(R["bnp"]), dev(R["z"]), dev(R["dout"])
    for _it in range(2):
        out = plan.forward(d_mu, d_rho, d_bn, d_z, SEED, STEP, K0, N)
        dmu = torch.zeros_like(d_mu); drho = torch.zeros_like(d_rho); dbn = torch.zeros_like(d_bn)
        dz = torch.zeros((N,) + R["z"].shape, device="cuda") if want_dz else None
        plan.backward(d_mu, d_rho, d_bn, d_z, SEED, STEP, K0, N, d_dout, dmu, drho, dbn, dz=dz)
        if split is not None:
            torch.cuda.current_stream().wait_stream(split)
        if mode == "profile":
            assert plan.profile_read()
    torch.cuda.synchronize()
    # (without dz the convolutions that read the net input run no backward-data: that slot is not compared)
    fam = {(i, w): lib.mfvi_plan_last_kernel(plan.handle, i, w) for i, o in enumerate(P.ops) if o["type"] == 1 for w in range(3)
           if want_dz or not (w == 1 and o["in0"] == zin)}
    return dict(out=host(out), dmu=host(dmu), drho=host(drho), dbn=host(dbn), dz=None if dz is None else host(dz), fam=fam)


@pytest.fixture(scope="module")
def R(M):
    """Inputs, the oracle's results (computed once, read-only) and the default mode's kernel-family tables."""
    net = O.make_net(**KW)
    mu, rho, bnp = _net_params(net, SEED)
    conv, bn, n_vi, n_bnp = O.net_table(net)
    z = (0.1 * O.uniform_fill(SEED, 0, 0, 0, net.input_depth * net.H * net.W)).reshape(net.input_depth, net.H, net.W)
    dout = O.normal_fill(SEED, 2, 9, 0, 0, N * KW["n_out"] * KW["H"] * KW["W"]).reshape(N, KW["n_out"], KW["H"], KW["W"])
    r = dict(mu=mu, rho=rho, bnp=bnp, z=z, dout=dout, out=[], dz=[], dmu=np.zeros(n_vi), drho=np.zeros(n_vi), dbn=np.zeros(n_bnp))
    for i in range(N):
        ref, tape = O.net_forward(net, mu, rho, bnp, z, SEED, STEP, K0 + i)
        a, b, c_, dzr = tape.backward(dout[i], n_vi, n_bnp, want_dz=True)
        r["dmu"] += a; r["drho"] += b; r["dbn"] += c_
        r["out"].append(np.array(ref)); r["dz"].append(np.array(dzr))
        tape.free()
    r["fam"] = {want_dz: _run(M, r, "default", want_dz)["fam"] for want_dz in (False, True)}
    return r


@pytest.mark.parametrize("want_dz", [False, True], ids=["nodz", "dz"])
@pytest.mark.parametrize("mode", MODES)
def test_schedule_modes_agree(M, R, mode, want_dz):
    g = _run(M, R, mode, want_dz)
    for i in range(N):
        assert relerr(g["out"][i], R["out"][i].reshape(g["out"][i].shape)) < 2e-4, ("out", i)
        if want_dz:
            assert relerr(g["dz"][i], R["dz"][i]) < 2e-4, ("dz", i)
    assert relerr(g["dmu"], R["dmu"]) < 2e-4
    assert relerr(g["drho"], R["drho"]) < 2e-4
    assert relerr(g["dbn"], R["dbn"]) < 2e-4
    assert g["fam"] == R["fam"][want_dz], (mode, g["fam"], R["fam"][want_dz])


def test_rejected_program_leaves_no_plan(M):
    """mfvi_plan_create on a program that fails validation (a tensor with three consumers) answers an error and a null plan; a valid
    create afterwards works."""
    L = M._lib
    from mfvi_dip_mia_amd.program import Program
    P = Program()
    x = P.tensor(4, 8, 8)
    a = P.tensor(4, 8, 8, bn=True, act=True); b = P.tensor(4, 8, 8, bn=True, act=True); c = P.tensor(4, 8, 8)
    for t in (a, b, c):
        P.conv(x, t, 3, 1)
    td = (L.TensorDesc * len(P.tensors))(*[L.TensorDesc(**t) for t in P.tensors])
    od = (L.OpDesc * len(P.ops))(*[L.OpDesc(**o) for o in P.ops])
    h = C.c_void_p(1)
    rc = L.lib().mfvi_plan_create(td, len(P.tensors), od, len(P.ops), x, c, P.n_vi, P.n_bn, 1, C.byref(h))
    assert rc != 0 and not h.value
    assert b"3 consumers" in L.lib().mfvi_last_error()
    Q, zin, out_id, _ = M.skip_program(KW["H"], KW["W"], KW["input_depth"], KW["n_out"], KW["nd"], KW["nu"], KW["ns"])
    plan = Q.compile(zin, out_id, max_samples=1)
    mu = torch.zeros(Q.n_vi, device="cuda"); rho = torch.full((Q.n_vi,), -5.0, device="cuda")
    bn = torch.ones(Q.n_bn, device="cuda"); z = torch.zeros(KW["input_depth"], KW["H"], KW["W"], device="cuda")
    out = plan.forward(mu, rho, bn, z, 1, 0, 0, 1)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
