"""GPU tests of the FastRadonTransform drop-in: mfvi_radon_project / mfvi_radon_backproject against the oracle, the
reference's outputs (tests/golden/radon_dropin.npz, micro.npz) and the engine's kernels (mfvi_radon_forward / mfvi_radon_adjoint), the
dot test, bit-identity, and the module in the loop the reference's CT runner writes (bayesian_optimization.py:545-582).  Every case is a
few launches; the largest plane is 256 x 256 with 45 angles."""
import os

import numpy as np
import pytest

from conftest import note_margin as _note

import radon_restatement as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

THETA45 = np.arange(0, 180., 4., dtype=np.float32)
KERNEL_CASES = [c[0] for c in R.CASES] + ["micro64", "plane256", "six40"]


@pytest.fixture(scope="module")
def M():
    import mfvi_dip_mia_amd as M_
    assert torch.cuda.is_available(), "these tests need the GPU"
    M_._lib.lib()
    return M_


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "radon_dropin.npz"))


def relerr(a, b):
    _v = R.relerr(a, b)
    _note(_v, 'relerr')
    return _v


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def project(M, x, theta):
    """mfvi_radon_project on x [n][S][S] (device) -> [n][T][S], the output pre-filled so that an unwritten element shows."""
    L = M._lib
    n, S = x.shape[0], x.shape[-1]
    y = torch.full((n, theta.numel(), S), 7.0, device="cuda")
    L.check(L.lib().mfvi_radon_project(L.ptr(x), L.ptr(theta), n, S, theta.numel(), L.ptr(y), L.stream_ptr()))
    return y


def backproject(M, g, theta):
    L = M._lib
    n, T, S = g.shape
    d = torch.full((n, S, S), -7.0, device="cuda")
    L.check(L.lib().mfvi_radon_backproject(L.ptr(g), L.ptr(theta), n, S, T, L.ptr(d), L.stream_ptr()))
    return d


_INPUTS = {}


def inputs(name, golden, golden_dir):
    """(x [n][S][S], theta [T], gy [n][T][S], oracle sino, oracle adjoint, golden sino or None, golden adjoint or None); computed once."""
    if name in _INPUTS:
        return _INPUTS[name]
    gs = ga = None
    if name == "micro64":                                # the inputs of radon64_sino / radon64_adj (oracle/make_golden.py)
        g = np.load(os.path.join(golden_dir, "micro.npz"))
        x, theta = O.phantom(64, 64, 11)[None], THETA45
        gy = O.normal_fill(11, 2, 5, 0, 0, theta.size * 64).reshape(1, theta.size, 64)
        gs, ga = g["radon64_sino"][None], g["radon64_adj"][None]
    elif name == "plane256":                             # the operating point of the CT loop: one plane, 45 angles
        x, theta = O.phantom(256, 256, 11)[None], THETA45
        gy = O.normal_fill(11, 2, 5, 0, 0, theta.size * 256).reshape(1, theta.size, 256)
    elif name == "six40":                                # more planes than one, a strip that is no multiple of 64
        x, theta = np.stack([O.noisy(O.phantom(40, 40, 20 + p), 0.1, p) for p in range(6)]), THETA45
        gy = O.normal_fill(13, 2, 5, 0, 0, 6 * theta.size * 40).reshape(6, theta.size, 40)
    else:
        theta = golden[name + "_theta_deg"]
        x, gy, gs, ga = golden[name + "_x"][0], golden[name + "_gy"][0], golden[name + "_y"][0], golden[name + "_gx"][0]
    x, gy = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(gy, np.float32)
    S = x.shape[-1]
    so = np.stack([O.radon_fwd(p, theta) for p in x])
    ao = np.stack([O.radon_adj(p, theta, S, S) for p in gy])
    _INPUTS[name] = (x, theta, gy, so, ao, gs, ga)
    return _INPUTS[name]


# ---- kernels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KERNEL_CASES)
def test_kernel_parity(M, golden, golden_dir, name):
    """Per plane against the oracle at relerr < 2e-5 (the bound of the engine's kernels, tests/test_gpu_parity.py), against the reference's
    outputs at < 5e-5, against the engine's kernels on the same inputs at < 4e-5 (two kernels, each within 2e-5 of the oracle)."""
    L = M._lib
    x, theta, gy, so, ao, gs, ga = inputs(name, golden, golden_dir)
    n, S, T = x.shape[0], x.shape[-1], theta.size
    d_x, d_th, d_g = dev(x), dev(theta), dev(gy)
    y, d = host(project(M, d_x, d_th)), host(backproject(M, d_g, d_th))
    y_old = torch.empty((n, T, S), device="cuda"); d_old = torch.empty((n, S, S), device="cuda")
    L.check(L.lib().mfvi_radon_forward(L.ptr(d_x), L.ptr(d_th), n, S, S, T, L.ptr(y_old), L.stream_ptr()))
    L.check(L.lib().mfvi_radon_adjoint(L.ptr(d_g), L.ptr(d_th), n, S, S, T, L.ptr(d_old), L.stream_ptr()))
    e = dict(fwd_oracle=max(relerr(y[p], so[p]) for p in range(n)), adj_oracle=max(relerr(d[p], ao[p]) for p in range(n)),
             fwd_old=max(relerr(y[p], host(y_old)[p]) for p in range(n)), adj_old=max(relerr(d[p], host(d_old)[p]) for p in range(n)))
    if gs is not None:
        e.update(fwd_golden=max(relerr(y[p], gs[p]) for p in range(n)), adj_golden=max(relerr(d[p], ga[p]) for p in range(n)))
    print("%s: n=%d S=%d T=%d %s" % (name, n, S, T, {k: "%.2e" % v for k, v in e.items()}))
    assert e["fwd_oracle"] < 2e-5 and e["adj_oracle"] < 2e-5
    assert e["fwd_old"] < 4e-5 and e["adj_old"] < 4e-5
    if gs is not None:
        assert e["fwd_golden"] < 5e-5 and e["adj_golden"] < 5e-5


@pytest.mark.parametrize("name", ["micro64", "odd33"])
def test_dot(M, golden, golden_dir, name):
    """<A x, y> = <x, A^T y> within 1e-5 relative (the engine's bound), at 64 x 64 with 45 angles and 33 x 33 with 180."""
    x, theta, gy, *_ = inputs(name, golden, golden_dir)
    assert (x.shape[-1], theta.size) == {"micro64": (64, 45), "odd33": (33, 180)}[name]
    d_th = dev(theta)
    y, d = host(project(M, dev(x), d_th)), host(backproject(M, dev(gy), d_th))
    lhs, rhs = float((y.astype(np.float64) * gy).sum()), float((d.astype(np.float64) * x).sum())
    print("%s: <Ax, y> %.9g  <x, A^T y> %.9g  rel %.2e" % (name, lhs, rhs, abs(lhs - rhs) / abs(lhs)))
    assert abs(lhs - rhs) < 1e-5 * abs(lhs)


@pytest.mark.parametrize("name", ["plane256", "six40"])
def test_bit_identity(M, golden, golden_dir, name):
    """Two calls agree bit for bit, at n = 1 (rows and angles split over the waves of a block) and n = 6."""
    x, theta, gy, *_ = inputs(name, golden, golden_dir)
    assert x.shape[0] == {"plane256": 1, "six40": 6}[name]
    d_x, d_th, d_g = dev(x), dev(theta), dev(gy)
    y1, y2 = project(M, d_x, d_th), project(M, d_x, d_th)
    b1, b2 = backproject(M, d_g, d_th), backproject(M, d_g, d_th)
    assert torch.equal(y1, y2) and torch.equal(b1, b2)
    assert float(y1.abs().max()) > 0 and float(b1.abs().max()) > 0


def test_zero_padding(M):
    """An image of ones at 45 degrees, S = 8: the chord of a ray shortens towards the detector's edges, and what lies outside the image
    is zero.  Against the oracle at its bound; the centre bins see more than the edge bins and no bin sees more than S."""
    x = np.ones((1, 8, 8), np.float32)
    theta = np.array([45.0], np.float32)
    y = host(project(M, dev(x), dev(theta)))[0, 0]
    ref = O.radon_fwd(x[0], theta)[0]
    print("ones at 45 degrees:", np.round(y, 4))
    assert relerr(y, ref) < 2e-5
    assert y[0] < y[3] and y[7] < y[4] and y.max() <= 8.0 + 1e-5 and y.min() >= 0.0
    assert abs(y[0] - ref[0]) < 2e-5 * ref.max() and abs(y[7] - ref[7]) < 2e-5 * ref.max()


@pytest.mark.parametrize("S", [1, 2, 65])
def test_sizes_that_take_another_path(M, S):
    """S = 1: no pair of x-neighbours exists (the single-load kernel); S = 2: the smallest paired load; S = 65: a second strip with one
    live lane, rows split over two waves.  Against the oracle at its bound, and a transpose."""
    theta = np.array([0.0, 30.0, 90.0, 137.0, 270.0], np.float32)
    x = O.uniform_fill(40 + S, 0, 0, 0, S * S).reshape(1, S, S)
    gy = O.normal_fill(40 + S, 2, 1, 0, 0, theta.size * S).reshape(1, theta.size, S)
    d_th = dev(theta)
    y, d = host(project(M, dev(x), d_th)), host(backproject(M, dev(gy), d_th))
    ef, ea = relerr(y[0], O.radon_fwd(x[0], theta)), relerr(d[0], O.radon_adj(gy[0], theta, S, S))
    lhs, rhs = float((y.astype(np.float64) * gy).sum()), float((d.astype(np.float64) * x).sum())
    print("S=%d: forward %.2e adjoint %.2e dot %.2e" % (S, ef, ea, abs(lhs - rhs) / abs(lhs)))
    assert ef < 2e-5 and ea < 2e-5 and abs(lhs - rhs) < 1e-5 * abs(lhs)


def test_entry_points_refuse_bad_arguments(M):
    L, lib = M._lib, M._lib.lib()
    z = torch.zeros(64, device="cuda")
    for fn, who in ((lib.mfvi_radon_project, b"radon_project"), (lib.mfvi_radon_backproject, b"radon_backproject")):
        for (a, th, n, S, T, o) in ((None, z, 1, 4, 2, z), (z, None, 1, 4, 2, z), (z, z, 1, 4, 2, None), (z, z, 0, 4, 2, z), (z, z, 1, 0, 2, z),
                                     (z, z, 1, 4, 0, z), (z, z, -3, 4, 2, z), (z, z, 65536, 4, 2, z)):
            rc = fn(L.ptr(a), L.ptr(th), n, S, T, L.ptr(o), L.stream_ptr())
            assert rc < 0 and who in lib.mfvi_last_error(), (who, n, S, T)
        with pytest.raises(L.MfviError, match="radon"):
            L.check(fn(L.ptr(z), L.ptr(z), 0, 4, 2, L.ptr(z), L.stream_ptr()))
    torch.cuda.synchronize()


# ---- the module ------------------------------------------------------------------------------------------------------------------------
def test_module_forward_and_autograd(M, golden, golden_dir):
    x, theta, gy, so, ao, *_ = inputs("six40", golden, golden_dir)
    S, T = 40, theta.size
    fr = M.FastRadonTransform((2, 3, S, S), torch.from_numpy(theta))             # built on the CPU, as a user may
    with pytest.raises(ValueError, match="move the module"):
        fr(dev(x).reshape(2, 3, S, S))
    fr = fr.to("cuda")
    assert fr.theta_deg.is_cuda and fr.trans.is_cuda and "grid" not in dict(fr.named_buffers())
    xt = dev(x).reshape(2, 3, S, S).requires_grad_(True)
    r = dev(gy).reshape(2, 3, T, S)
    y = fr(xt)
    assert y.shape == (2, 3, T, S) and y.dtype == torch.float32 and y.requires_grad
    assert torch.equal(y.detach().reshape(6, T, S), project(M, dev(x), fr.theta_deg))
    (y * r).sum().backward()
    assert xt.grad.shape == xt.shape and torch.equal(xt.grad.reshape(6, S, S), backproject(M, dev(gy), fr.theta_deg))
    # a non-contiguous input (and a non-contiguous upstream gradient) are made contiguous
    xp = dev(np.ascontiguousarray(x.transpose(0, 2, 1))).reshape(2, 3, S, S).transpose(2, 3).requires_grad_(True)
    assert not xp.is_contiguous()
    yp = fr(xp)
    assert torch.equal(yp.detach(), y.detach())
    rp = dev(np.ascontiguousarray(gy.transpose(0, 2, 1))).reshape(2, 3, S, T).transpose(2, 3)
    (yp * rp).sum().backward()
    assert torch.equal(xp.grad, xt.grad)
    # theta given on the device, as the reference's runner does (bayesian_optimization.py:545-546); no_grad output carries no graph
    fr2 = M.FastRadonTransform(xt.size(), torch.arange(0, 180., step=4.).to("cuda"))
    with torch.no_grad():
        y2 = fr2(xt)
    assert not y2.requires_grad and torch.equal(y2, y.detach())
    # refusals on real tensors
    with pytest.raises(NotImplementedError, match="no CPU path"):
        fr(torch.zeros(1, 1, S, S))
    with pytest.raises(NotImplementedError, match="float32"):
        fr(torch.zeros(1, 1, S, S, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="expects"):
        fr(torch.zeros(1, 1, S, S + 8, device="cuda"))
    # once-differentiable
    xq = dev(x[:1]).reshape(1, 1, S, S).requires_grad_(True)
    wq = torch.ones((1, 1, T, S), device="cuda", requires_grad=True)              # an upstream gradient that itself asks for a graph
    (gq,) = torch.autograd.grad((fr(xq) * wq).sum(), xq, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gq.sum().backward()


def test_the_references_line_matches_the_fused_data_term(M):
    """mse_loss(fr(out), sino).backward() (bayesian_optimization.py:576) against mfvi_radon_mse's dout on the same inputs, out
    [2, 1, 32, 32], grad_scale = 1 / K: two gradients, each through kernels within 2e-5 of the oracle -> 4e-5."""
    L = M._lib
    K, S = 2, 32
    theta = THETA45
    T = theta.size
    out_np = np.stack([O.noisy(O.phantom(S, S, 3 + k), 0.1, k) for k in range(K)])[:, None]
    sino_np = O.radon_fwd(O.phantom(S, S, 3), theta)
    fr = M.FastRadonTransform((1, 1, S, S), torch.from_numpy(theta)).to("cuda")
    out = dev(out_np).requires_grad_(True)
    sino = dev(sino_np)[None, None]
    # the engine's data term is the sum over the K samples of each sample's own mean; the module's line, sample by sample
    loss = sum(torch.nn.functional.mse_loss(fr(out[k:k + 1]), sino) for k in range(K)) / K
    loss.backward()
    d_th = dev(theta)
    scratch = torch.empty(K * T * S, device="cuda"); dout = torch.empty((K, 1, S, S), device="cuda")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    L.check(L.lib().mfvi_radon_mse(L.ptr(out.detach()), L.ptr(sino), L.ptr(d_th), K, S, S, T, 1.0 / K, L.ptr(scratch), L.ptr(dout), L.ptr(acc), L.stream_ptr()))
    e = relerr(host(out.grad), host(dout))
    loss_v = float(loss.detach())
    print("mse line: loss %.9g (fused %.9g), gradient relerr %.2e" % (loss_v, float(acc) / K, e))
    assert e < 4e-5
    assert abs(loss_v - float(acc) / K) < 1e-5 * abs(float(acc) / K)
    # the batch as the module's extension takes it: K samples in one call, the mean over all of them
    out2 = dev(out_np).requires_grad_(True)
    torch.nn.functional.mse_loss(fr(out2), sino.expand(K, 1, T, S)).backward()
    assert relerr(host(out2.grad), host(dout)) < 4e-5


@pytest.mark.parametrize("K", [1, 2])
def test_the_ct_loop(M, K):
    """run_ct_mfvi's loop (bayesian_optimization.py:568-582) on the drop-in names: get_net(..., n_channels=1) -> MeanFieldVI ->
    mse_loss(forward_radon(out), img_radon) + temp * kl -> AdamW, 30 iterations at 32 x 32; the data term of the last five iterations is
    below that of the first five.  (Three scales: the reference's five need at least 64 x 64 under reflection padding.)  n_samples = 2
    hands the module two samples as its batch; the sinogram broadcasts."""
    S, device = 32, torch.device("cuda")
    temp, sigma = 4.4e-7, 4.9e-8
    img = torch.from_numpy(O.phantom(S, S, 7))[None, None].to(device)
    net = M.get_net(8, 'skip', 'reflection', skip_n33d=[8, 16, 16], skip_n33u=[8, 16, 16], skip_n11=4, num_scales=3, n_channels=1,
                    upsample_mode='bilinear')
    net = M.MeanFieldVI(net, prior={'mu': 0.0, 'sigma': np.sqrt(temp) * sigma}, replace_layers='all', device=device, reparam='', seed=2,
                        n_samples=K, autotune=False)
    theta = torch.arange(0, 180., step=4.).to(device)
    forward_radon = M.FastRadonTransform(img.size(), theta)
    img_radon = forward_radon(img).to(device).detach()
    assert img_radon.shape == (1, 1, 45, S)
    net_input = (0.1 * torch.from_numpy(O.uniform_fill(2, 0, 0, 0, 8 * S * S)).reshape(1, 8, S, S)).to(device)
    optimizer = torch.optim.AdamW(net.parameters(), lr=1e-2, weight_decay=0)
    data = []
    for i in range(30):
        optimizer.zero_grad()
        out = net(net_input)
        assert out.shape == (K, 1, S, S)
        nll = torch.nn.functional.mse_loss(forward_radon(out), img_radon.expand(K, -1, -1, -1))
        kl = net.kl()
        loss = nll + temp * kl
        loss.backward()
        if not torch.isnan(loss):
            optimizer.step()
        data.append(nll.detach())
    data = torch.stack(data).cpu().numpy()
    print("CT loop K=%d: data term %.5f -> %.5f" % (K, data[:5].mean(), data[-5:].mean()))
    assert np.isfinite(data).all() and data[-5:].mean() < data[:5].mean()
