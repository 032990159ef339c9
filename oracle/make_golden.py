"""Generate golden vectors by running the REFERENCE's own modules (imported from
/root/reference, which exists only in the build container) with eps injected from the
build's RNG spec.  Output: tests/golden/*.npz (data only: inputs are regenerated from seeds,
expected outputs are stored).  Run:  python oracle/make_golden.py

Test infrastructure; never shipped in the product path and never run on the GPU box.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from oracle import oracle as O  # noqa: E402


def import_reference():
    # in-process empty stubs for packages the reference imports but never uses on this path
    for m in ["torchvision", "torchvision.transforms", "skimage", "skimage.metrics"]:
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.modules["skimage.metrics"].peak_signal_noise_ratio = None
    sys.path.insert(0, REF)
    import BayTorch.freq_to_bayes as f2b
    import BayTorch.modules.module as vimod
    import models
    import models.skip  # noqa: F401
    mskip = sys.modules['models.skip']   # models/__init__ rebinds the name `skip` to the function
    import radon.radon as radon
    import utils.bayesian_utils as bu
    import utils.common_utils as cu
    return dict(f2b=f2b, vimod=vimod, models=models, mskip=mskip, radon=radon, bu=bu, cu=cu)


R = import_reference()
torch.set_num_threads(8)


class EpsInjector:
    """Replaces VIModule.rsample (modules/module.py:82-85) by a version that consumes eps
    produced by the build's RNG spec, in call order (weight then bias per layer)."""

    def __init__(self):
        self.queue = []
        self.orig = R["vimod"].VIModule.rsample

    def __enter__(self):
        q = self.queue

        def rsample(mu, sigma):
            e = q.pop(0)
            assert e.shape == mu.shape, (e.shape, mu.shape)
            return mu + e * sigma
        R["vimod"].VIModule.rsample = staticmethod(rsample)
        return self

    def __exit__(self, *a):
        R["vimod"].VIModule.rsample = self.orig

    def load(self, layers, seed, step, sample):
        self.queue.clear()
        for lid, m in enumerate(layers):
            self.queue.append(torch.from_numpy(O.eps(seed, step, sample, lid, 0, m.W_mu.numel()).reshape(tuple(m.W_mu.shape))))
            self.queue.append(torch.from_numpy(O.eps(seed, step, sample, lid, 1, m.bias_mu.numel())))


def vi_layers(net):
    return [m for m in net.modules() if hasattr(m, "W_mu")]


def bn_layers(net):
    return [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]


def load_flat(net, mu, rho, bnp, conv_tbl, bn_tbl):
    with torch.no_grad():
        for m, row in zip(vi_layers(net), conv_tbl):
            cin, cout, k, stride, w_off, b_off = [int(v) for v in row]
            assert tuple(m.W_mu.shape) == (cout, cin, k, k), (tuple(m.W_mu.shape), row)
            n = cout * cin * k * k
            m.W_mu.copy_(torch.from_numpy(mu[w_off:w_off + n].reshape(cout, cin, k, k)))
            m.W_rho.copy_(torch.from_numpy(rho[w_off:w_off + n].reshape(cout, cin, k, k)))
            m.bias_mu.copy_(torch.from_numpy(mu[b_off:b_off + cout]))
            m.bias_rho.copy_(torch.from_numpy(rho[b_off:b_off + cout]))
        for m, (c, off) in zip(bn_layers(net), bn_tbl):
            c, off = int(c), int(off)
            assert m.num_features == c
            m.weight.copy_(torch.from_numpy(bnp[off:off + c]))
            m.bias.copy_(torch.from_numpy(bnp[off + c:off + 2 * c]))


def flat_grads(net, conv_tbl, bn_tbl, n_vi, n_bnp):
    dmu = np.zeros(n_vi, np.float64); drho = np.zeros(n_vi, np.float64); dbn = np.zeros(n_bnp, np.float64)
    for m, row in zip(vi_layers(net), conv_tbl):
        cin, cout, k, stride, w_off, b_off = [int(v) for v in row]
        n = cout * cin * k * k
        dmu[w_off:w_off + n] = m.W_mu.grad.numpy().ravel(); drho[w_off:w_off + n] = m.W_rho.grad.numpy().ravel()
        dmu[b_off:b_off + cout] = m.bias_mu.grad.numpy(); drho[b_off:b_off + cout] = m.bias_rho.grad.numpy()
    for m, (c, off) in zip(bn_layers(net), bn_tbl):
        c, off = int(c), int(off)
        dbn[off:off + c] = m.weight.grad.numpy(); dbn[off + c:off + 2 * c] = m.bias.grad.numpy()
    return dmu, drho, dbn


def build_ref_net(onet, prior_sigma_raw):
    """get_net(...)+MeanFieldVI exactly as bayesian_optimization.py:1318-1342 but with the
    channel lists of `onet` (so small nets can be pinned too)."""
    n = onet.n_scales
    net = R["mskip"].skip(onet.input_depth, onet.n_out,
                          num_channels_down=[onet.nd[i] for i in range(n)],
                          num_channels_up=[onet.nu[i] for i in range(n)],
                          num_channels_skip=[onet.ns[i] for i in range(n)],
                          upsample_mode='bilinear', downsample_mode='stride',
                          need_sigmoid=False, need_bias=True, pad='reflection', act_fun='LeakyReLU',
                          dropout_mode_down='None', dropout_mode_up='None', dropout_mode_skip='None', dropout_mode_output='None')
    net = R["f2b"].MeanFieldVI(net, prior={'mu': 0.0, 'sigma': prior_sigma_raw}, replace_layers='all', reparam='')
    return net


def test_params(onet, seed):
    mu, rho, bnp = O.init_params(onet, seed)
    conv, bn, n_vi, n_bnp = O.net_table(onet)
    g = O.normal_fill(seed, 2, 7, 0, 0, n_bnp)
    for c, off in bn:     # non-trivial affine: gamma = 1 + 0.1 n, beta = 0.1 n
        bnp[off:off + c] = 1.0 + 0.1 * g[off:off + c]
        bnp[off + c:off + 2 * c] = 0.1 * g[off + c:off + 2 * c]
    return mu, rho, bnp


def strided(a, n=4096):
    a = np.asarray(a).ravel()
    step = max(1, a.size // n)
    return a[::step][:n].copy()


DEN = dict(temp=5.656911698337764e-07, sigma=1.4616642493692077e-05)   # test_configs/mfvi_den.json:5,9
SR = dict(temp=4.381719802264805e-07, sigma=4.9e-08)                   # test_configs/mfvi_sr.json
CT = dict(temp=2.2e-10, sigma=1.7e-7)                                  # test_configs/mfvi_ct.json


def golden_net(name, onet, seed, K, task="den", full_arrays=True, dtype=torch.float32, save=True, compact=False, bf16=False, params=None, with_kl=True):
    """params: (mu, rho, bn) float32 blocks in the flat layout instead of test_params(onet, seed); with_kl=False leaves temp * kl out of the
    backward pass (the data term's gradients alone: at rho = -200 the KL gradient is of the order 1 / softplus(rho)^3).
    compact: the float64 twin's output and the eval-mode output are stored strided (the 256^2 fixtures stay small).
    bf16: mu / rho are rounded to bfloat16 (round-to-nearest-even, O.bf16_round == torch's .bfloat16().float()) before they are loaded
    into the reference's MeanFieldVI — the values a bf16 parameter store holds (BASELINE configs[4])."""
    cfg = dict(den=DEN, sr=SR, ct=CT)[task]
    temp = cfg["temp"]; prior_raw = float(np.sqrt(temp) * cfg["sigma"])
    conv, bn, n_vi, n_bnp = O.net_table(onet)
    mu, rho, bnp = test_params(onet, seed) if params is None else params
    if bf16:
        assert np.array_equal(O.bf16_round(mu), torch.from_numpy(mu).bfloat16().float().numpy())
        mu, rho = O.bf16_round(mu), O.bf16_round(rho)
    net = build_ref_net(onet, prior_raw)
    load_flat(net, mu, rho, bnp, conv, bn)
    net = net.to(dtype)      # float64 run of the same reference code = noise-free anchor for the gradients
    layers = vi_layers(net)
    H, W = onet.H, onet.W
    z = (0.1 * O.uniform_fill(seed, 0, 0, 0, onet.input_depth * H * W)).reshape(1, onet.input_depth, H, W)
    img = O.phantom(H, W, seed); tgt = O.noisy(img, 0.1, seed)
    zt = torch.from_numpy(z).to(dtype)
    res = {}
    theta = None
    if task == "ct":
        theta = torch.arange(0, 180., step=4.)
        fr = R["radon"].FastRadonTransform((1, 1, H, W), theta)
        sino_t = fr(torch.from_numpy(img)[None, None]).detach()
        res["sino_target"] = sino_t.numpy()[0, 0]
        if dtype != torch.float32:      # the float64 twin: same fp32 sinogram target, transform and loss in float64
            fr = fr.to(dtype); sino_t = sino_t.to(dtype)
    net.zero_grad()
    outs = []; nll_sum = 0.0
    with EpsInjector() as inj:
        for k in range(K):
            inj.load(layers, seed, 3, k)
            inj.queue[:] = [e.to(dtype) for e in inj.queue]
            out = net(zt)
            if task == "den":
                nll = R["bu"].gaussian_nll(out[:, :1], out[:, 1:], torch.from_numpy(tgt)[None, None].to(dtype))
            elif task == "sr":
                lr_t = torch.from_numpy(np.ascontiguousarray(tgt[::4, ::4]))[None, None]
                out_lr = torch.nn.functional.interpolate(out, scale_factor=0.25, mode='nearest', recompute_scale_factor=False)
                nll = R["bu"].gaussian_nll(out_lr[:, :1], out_lr[:, 1:], lr_t)
            else:
                nll = torch.nn.functional.mse_loss(fr(out), sino_t)
            (nll / K).backward()
            nll_sum += float(nll) / K
            outs.append(out.detach().numpy()[0].copy())
        kl = net.kl()
        if with_kl:
            (temp * kl).backward()
    per_layer_kl = np.array([float(m._kl) for m in layers], np.float64)
    dmu, drho, dbn = flat_grads(net, conv, bn, n_vi, n_bnp)
    res.update(dict(seed=seed, K=K, step=3, temp=temp, prior_sigma=np.float32(prior_raw + 1e-6), H=H, W=W,
                    nll=nll_sum, kl=float(kl), loss=nll_sum + temp * float(kl), per_layer_kl=per_layer_kl,
                    out=np.stack(outs)))
    if full_arrays:
        res.update(dmu=dmu, drho=drho, dbn=dbn)
    else:
        res.update(dmu_s=strided(dmu), drho_s=strided(drho), dbn=dbn,
                   dmu_layer_norm=np.array([np.linalg.norm(dmu[int(r[4]):int(r[5]) + int(r[1])]) for r in conv]),
                   drho_layer_norm=np.array([np.linalg.norm(drho[int(r[4]):int(r[5]) + int(r[1])]) for r in conv]),
                   dmu_sum=float(dmu.astype(np.float64).sum()), drho_sum=float(drho.astype(np.float64).sum()))
    # eval anchor: RT layers in eval (w = mu), BN still in training mode -> RNG-free forward
    for m in layers:
        m.training = False
    with torch.no_grad():
        res["out_eval"] = net(zt).numpy()[0]
    for m in layers:
        m.training = True
    res["state_dict_keys"] = np.array(list(net.state_dict().keys()))
    res["layer_names"] = np.array([n for n, m in net.named_modules() if hasattr(m, "W_mu")])
    if not save:
        return res
    if name.startswith("full"):
        r64 = golden_net(name, onet, seed, K, task, full_arrays=False, dtype=torch.float64, save=False, bf16=bf16)
        for kname in ("dmu_s", "drho_s", "dbn", "dmu_layer_norm", "drho_layer_norm", "out", "nll"):
            res[kname + "_f64"] = np.asarray(r64[kname], np.float64)
        if compact:
            res["out_s_f64"] = strided(res.pop("out_f64"), 16384); res["out_eval_s"] = strided(res.pop("out_eval"), 16384)
            res["out"] = res["out"].astype(np.float32)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **res)
    print(name, "nll", nll_sum, "kl", float(kl), "out", res["out"].shape, "|dmu|", np.linalg.norm(dmu), "|drho|", np.linalg.norm(drho))


def golden_posterior():
    """The reference's own MeanFieldVI autograd in float64 away from the initial posterior: three_scale_32, den data
    term, K = 2, at the `fitted` and `pruned` layouts of tests/posterior_cases.py (rho ~ -13.8; a quarter of the weights at rho = -200,
    mu = 0).  Pins the float64 statement of tests/posterior_cases.py to the reference, not to this project's reading of it."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import posterior_cases as PC
    from mfvi_dip_mia_amd.program import skip_program            # pure-Python layer program (offsets of the flat layout)
    kw = PC.NETS["three_scale_32"]
    onet = O.make_net(**kw)
    P, _, _, _ = skip_program(**kw)
    seed, K = PC.NET_SEEDS[("three_scale_32", "fitted")], 2
    assert PC.NET_SEEDS[("three_scale_32", "pruned")] == seed
    res = dict(seed=np.int64(seed), K=np.int64(K), step=np.int64(3))
    for lay in ("fitted", "pruned"):
        mu, rho, bnp = PC.net_params(P, lay, seed)
        r = golden_net("posterior_" + lay, onet, seed, K, task="den", dtype=torch.float64, save=False, params=(mu, rho, bnp), with_kl=False)
        assert int(r["step"]) == 3
        res.update({lay + "_out": r["out"].astype(np.float32), lay + "_nll": np.float64(r["nll"]), lay + "_mu": mu, lay + "_rho": rho,
                    lay + "_dmu": r["dmu"].astype(np.float32), lay + "_drho": r["drho"].astype(np.float32), lay + "_dbn": r["dbn"].astype(np.float32)})
        print("posterior", lay, "nll", r["nll"], "|dmu|", np.linalg.norm(r["dmu"]), "|drho|", np.linalg.norm(r["drho"]))
    np.savez_compressed(os.path.join(GOLD, "posterior_range.npz"), **res)


def golden_traj(name, onet, seed, K, steps, lr=1e-3):
    """N optimizer steps of the reference loop (bayesian_optimization.py:1360-1372) with torch AdamW."""
    temp = DEN["temp"]; prior_raw = float(np.sqrt(temp) * DEN["sigma"])
    conv, bn, n_vi, n_bnp = O.net_table(onet)
    mu, rho, bnp = test_params(onet, seed)
    net = build_ref_net(onet, prior_raw); load_flat(net, mu, rho, bnp, conv, bn)
    layers = vi_layers(net)
    H, W = onet.H, onet.W
    z0 = (0.1 * O.uniform_fill(seed, 0, 0, 0, onet.input_depth * H * W)).reshape(1, onet.input_depth, H, W)
    tgt = torch.from_numpy(O.noisy(O.phantom(H, W, seed), 0.1, seed))[None, None]
    opt = torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=0)
    losses, nlls, kls = [], [], []
    with EpsInjector() as inj:
        for it in range(steps):
            opt.zero_grad()
            zn = O.normal_fill(seed, 1, 0, 0, it, z0.size).reshape(z0.shape)      # DOMAIN_INPUT, step = it
            zt = torch.from_numpy(z0 + 0.1 * zn)
            nll_sum = 0.0
            for k in range(K):
                inj.load(layers, seed, it, k)
                out = net(zt)
                nll = R["bu"].gaussian_nll(out[:, :1], out[:, 1:], tgt)
                (nll / K).backward(); nll_sum += float(nll) / K
            kl = net.kl(); (temp * kl).backward()
            opt.step()
            losses.append(nll_sum + temp * float(kl)); nlls.append(nll_sum); kls.append(float(kl))
    # final params
    fmu = np.zeros(n_vi, np.float32); frho = np.zeros(n_vi, np.float32); fbn = np.zeros(n_bnp, np.float32)
    for m, row in zip(layers, conv):
        cin, cout, k, stride, w_off, b_off = [int(v) for v in row]; n = cout * cin * k * k
        fmu[w_off:w_off + n] = m.W_mu.detach().numpy().ravel(); frho[w_off:w_off + n] = m.W_rho.detach().numpy().ravel()
        fmu[b_off:b_off + cout] = m.bias_mu.detach().numpy(); frho[b_off:b_off + cout] = m.bias_rho.detach().numpy()
    for m, (c, off) in zip(bn_layers(net), bn):
        c, off = int(c), int(off)
        fbn[off:off + c] = m.weight.detach().numpy(); fbn[off + c:off + 2 * c] = m.bias.detach().numpy()
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), seed=seed, K=K, steps=steps, lr=lr, temp=temp,
                        prior_sigma=np.float32(prior_raw + 1e-6), H=H, W=W,
                        loss=np.array(losses), nll=np.array(nlls), kl=np.array(kls), mu=fmu, rho=frho, bn=fbn)
    print(name, "loss", losses)


def golden_fitcurve(name, size, seed, steps, every=10, lr=1e-3):
    """Fit QUALITY, not one step: the reference's denoising loop (bayesian_optimization.py:1356-1406 — MeanFieldVI + skip + gaussian_nll +
    temp * net.kl() + torch.optim.AdamW, K = 1, exp_weight 0.99 smoothing, its own peak_signal_noise_ratio) for `steps` iterations on the
    full 26-layer net at size x size, with eps and the input perturbation injected from the build's RNG spec and the parameters the
    engine starts from (O.init_params: mu ~ N(0, 0.1), rho ~ N(-3, 0.1), gamma 1, beta 0).  Stored every `every` iterations: ELBO, NLL,
    KL, PSNR(gt, out), PSNR(gt, out_avg) — once run in float32 (what the reference does) and once in float64 (the reference code on
    double tensors): the gap between the two curves is the band inside which any float32 implementation can be expected to land."""
    temp = DEN["temp"]; prior_raw = float(np.sqrt(temp) * DEN["sigma"])
    onet = O.make_net(size, size)
    conv, bn, n_vi, n_bnp = O.net_table(onet)
    H = W = size
    z0 = (0.1 * O.uniform_fill(seed, 0, 0, 0, onet.input_depth * H * W)).reshape(1, onet.input_depth, H, W)
    gt_np = O.phantom(H, W, seed); noisy_np = O.noisy(gt_np, 0.1, seed)
    res = {}
    for tag, dt in (("", torch.float32), ("_f64", torch.float64)):
        mu, rho, bnp = O.init_params(onet, seed)
        net = build_ref_net(onet, prior_raw); load_flat(net, mu, rho, bnp, conv, bn)
        net = net.to(dt)
        layers = vi_layers(net)
        tgt = torch.from_numpy(noisy_np)[None, None].to(dt); gt = torch.from_numpy(gt_np)[None, None].to(dt)
        opt = torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=0)
        out_avg = None
        rows = []
        with EpsInjector() as inj:
            for it in range(steps):
                opt.zero_grad()
                zn = O.normal_fill(seed, 1, 0, 0, it, z0.size).reshape(z0.shape)
                zt = torch.from_numpy(z0 + 0.1 * zn).to(dt)
                inj.load(layers, seed, it, 0)
                inj.queue[:] = [e.to(dt) for e in inj.queue]
                out = net(zt)
                nll = R["bu"].gaussian_nll(out[:, :1], out[:, 1:], tgt)
                kl = net.kl()
                loss = nll + temp * kl
                loss.backward(); opt.step()
                with torch.no_grad():
                    out[:, 1:] = torch.exp(-out[:, 1:])
                out_avg = out.detach() if out_avg is None else out_avg * 0.99 + out.detach() * 0.01
                if it % every == 0 or it == steps - 1:
                    with torch.no_grad():
                        psnr_gt = R["cu"].peak_signal_noise_ratio(gt, out.detach()[:, :1].clip(0, 1))
                        psnr_sm = R["cu"].peak_signal_noise_ratio(gt, out_avg.detach()[:, :1].clip(0, 1))
                    rows.append((it, float(loss), float(nll), float(kl), psnr_gt, psnr_sm))
        res["curve" + tag] = np.array(rows, np.float64)
        print(name, tag or "_f32", "last:", rows[-1])
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), seed=seed, steps=steps, every=every, lr=lr, temp=temp, sigma=DEN["sigma"],
                        prior_sigma=np.float32(prior_raw + 1e-6), size=size, columns=np.array(["it", "elbo", "nll", "kl", "psnr_gt", "psnr_gt_sm"]), **res)


def golden_layers():
    """Single Conv2dRT (ReflectionPad2d + conv, models/common.py:100-135) fwd/bwd with injected eps."""
    from models.common import conv as ref_conv
    cases = [(16, 4, 1, 1, 12, 12), (16, 16, 3, 2, 16, 16), (16, 16, 3, 1, 10, 14), (36, 16, 3, 1, 8, 8),
             (8, 32, 3, 2, 12, 20), (32, 2, 1, 1, 6, 6), (132, 8, 3, 1, 8, 8)]
    res = {}
    for ci, (cin, cout, k, stride, H, W) in enumerate(cases):
        seq = ref_conv(cin, cout, k, stride, bias=True, pad='reflection')
        net = R["f2b"].MeanFieldVI(seq, prior={'mu': 0.0, 'sigma': 0.1}, replace_layers='all', reparam='')
        m = vi_layers(net)[0]
        seed = 100 + ci
        nw = cout * cin * k * k
        mu = 0.1 * O.normal_fill(seed, 2, 0, 0, 0, nw + cout); rho = -3 + 0.1 * O.normal_fill(seed, 2, 1, 0, 0, nw + cout)
        with torch.no_grad():
            m.W_mu.copy_(torch.from_numpy(mu[:nw].reshape(cout, cin, k, k))); m.W_rho.copy_(torch.from_numpy(rho[:nw].reshape(cout, cin, k, k)))
            m.bias_mu.copy_(torch.from_numpy(mu[nw:])); m.bias_rho.copy_(torch.from_numpy(rho[nw:]))
        x = torch.from_numpy(O.normal_fill(seed, 2, 2, 0, 0, cin * H * W).reshape(1, cin, H, W)).requires_grad_(True)
        with EpsInjector() as inj:
            inj.load([m], seed, 5, 2)
            y = net(x)
        dy = torch.from_numpy(O.normal_fill(seed, 2, 3, 0, 0, y.numel()).reshape(y.shape))
        y.backward(dy)
        res[f"case{ci}_shape"] = np.array([cin, cout, k, stride, H, W])
        res[f"case{ci}_y"] = y.detach().numpy()[0]
        res[f"case{ci}_dx"] = x.grad.numpy()[0]
        res[f"case{ci}_dWmu"] = m.W_mu.grad.numpy(); res[f"case{ci}_dWrho"] = m.W_rho.grad.numpy()
        res[f"case{ci}_dbmu"] = m.bias_mu.grad.numpy(); res[f"case{ci}_dbrho"] = m.bias_rho.grad.numpy()
    res["n_cases"] = len(cases)
    np.savez_compressed(os.path.join(GOLD, "layers.npz"), **res)
    print("layers ok")


def golden_micro():
    res = {}
    # BN train-mode N=1 (models/common.py:96-97) + LeakyReLU(0.2) + Upsample bilinear x2 (models/skip.py:102)
    x = O.normal_fill(7, 2, 0, 0, 0, 6 * 10 * 12).reshape(1, 6, 10, 12) * 1.7 + 0.4
    g = 1 + 0.1 * O.normal_fill(7, 2, 1, 0, 0, 6); b = 0.1 * O.normal_fill(7, 2, 2, 0, 0, 6)
    bnm = R["models"].skip.__globals__["bn"](6)
    with torch.no_grad():
        bnm.weight.copy_(torch.from_numpy(g)); bnm.bias.copy_(torch.from_numpy(b))
    xt = torch.from_numpy(x.copy()).requires_grad_(True)
    act = R["models"].skip.__globals__["act"]('LeakyReLU')
    up = torch.nn.Upsample(scale_factor=2, mode='bilinear')
    y = up(act(bnm(xt)))
    dy = torch.from_numpy(O.normal_fill(7, 2, 3, 0, 0, y.numel()).reshape(y.shape))
    y.backward(dy)
    res.update(bn_y=y.detach().numpy()[0], bn_dx=xt.grad.numpy()[0], bn_dgamma=bnm.weight.grad.numpy(), bn_dbeta=bnm.bias.grad.numpy())
    # gaussian_nll (utils/bayesian_utils.py:29-32) incl. clamped entries
    o = O.normal_fill(8, 2, 0, 0, 0, 2 * 32 * 32).reshape(1, 2, 32, 32).copy()
    o[0, 1, 0, :4] = [25.0, -25.0, 20.0, -20.0]
    t = O.uniform_fill(8, 1, 0, 0, 32 * 32).reshape(1, 1, 32, 32)
    ot = torch.from_numpy(o).requires_grad_(True)
    nll = R["bu"].gaussian_nll(ot[:, :1], ot[:, 1:], torch.from_numpy(t)); nll.backward()
    res.update(nll=float(nll), nll_dout=ot.grad.numpy()[0])
    # PSNR / SSIM (utils/common_utils.py:297-353)
    a = O.phantom(48, 40, 3); bb = O.noisy(a, 0.1, 3)
    res.update(psnr=R["cu"].peak_signal_noise_ratio(torch.from_numpy(a)[None, None], torch.from_numpy(bb)[None, None]),
               ssim=R["cu"].structural_similarity(torch.from_numpy(a)[None, None], torch.from_numpy(bb)[None, None]))
    # get_noise stats are not pinned (torch RNG); KL closed form (modules/module.py:64-80)
    lay = R["vimod"].VIModule(None, (5, 7), (5,), prior={'mu': 0.0, 'sigma': 0.05})
    mu = 0.1 * O.normal_fill(9, 2, 0, 0, 0, 40); rho = -3 + 0.5 * O.normal_fill(9, 2, 1, 0, 0, 40)
    with torch.no_grad():
        lay.W_mu.copy_(torch.from_numpy(mu[:35].reshape(5, 7))); lay.W_rho.copy_(torch.from_numpy(rho[:35].reshape(5, 7)))
        lay.bias_mu.copy_(torch.from_numpy(mu[35:])); lay.bias_rho.copy_(torch.from_numpy(rho[35:]))
    klv = lay._kl; klv.backward()
    res.update(kl=float(klv), kl_dmu=np.concatenate([lay.W_mu.grad.numpy().ravel(), lay.bias_mu.grad.numpy()]),
               kl_drho=np.concatenate([lay.W_rho.grad.numpy().ravel(), lay.bias_rho.grad.numpy()]))
    # Radon (radon/radon.py:23-55) fwd + adjoint
    for (H, tag) in [(64, "64"), (256, "256")]:
        img = O.phantom(H, H, 11)
        theta = torch.arange(0, 180., step=4.)
        fr = R["radon"].FastRadonTransform((1, 1, H, H), theta)
        it = torch.from_numpy(img)[None, None].requires_grad_(True)
        s = fr(it)
        r = torch.from_numpy(O.normal_fill(11, 2, 5, 0, 0, s.numel()).reshape(s.shape))
        (s * r).sum().backward()
        if H == 64:
            res.update(radon64_sino=s.detach().numpy()[0, 0], radon64_adj=it.grad.numpy()[0, 0])
        else:
            res.update(radon256_sino_s=strided(s.detach().numpy()), radon256_adj_s=strided(it.grad.numpy()),
                       radon256_sino_sum=float(s.sum()), radon256_adj_sum=float(it.grad.sum()))
    # AdamW(lr, wd=0) 3 steps on a small vector
    p = torch.from_numpy(O.normal_fill(12, 2, 0, 0, 0, 64).copy()).requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=0)
    for t_ in range(3):
        opt.zero_grad(); p.grad = torch.from_numpy(O.normal_fill(12, 2, 1 + t_, 0, 0, 64).copy()); opt.step()
    res.update(adam_p=p.detach().numpy())
    np.savez_compressed(os.path.join(GOLD, "micro.npz"), **res)
    print("micro ok")



def golden_inpainting():
    """The inpainting MFVI variant (bayesian_optimization.py:2892-3114): its three ops that the den/SR/CT nets do not have, and
    the reference's own skip() built with the runner's options (no skip branches, 5x5 down filters, nearest upsampling,
    need1x1_up=False, 4 outputs) at 3 scales, wrapped in MeanFieldVI, with the sigmoid + masked NLL of the runner."""
    from models.common import conv as ref_conv
    from mfvi_dip_mia_amd.program import skip_program            # pure-Python layer program (offsets of the flat layout)
    res = {}
    # (1) Conv2dRT with 5x5 filters, reflection pad 2, stride 1 and 2
    for ci, (cin, cout, k, stride, H, W) in enumerate([(8, 12, 5, 1, 12, 16), (16, 16, 5, 2, 20, 20)]):
        seq = ref_conv(cin, cout, k, stride, bias=True, pad='reflection')
        net = R["f2b"].MeanFieldVI(seq, prior={'mu': 0.0, 'sigma': 0.1}, replace_layers='all', reparam='')
        m = vi_layers(net)[0]
        seed = 300 + ci
        nw = cout * cin * k * k
        mu = 0.1 * O.normal_fill(seed, 2, 0, 0, 0, nw + cout); rho = -3 + 0.1 * O.normal_fill(seed, 2, 1, 0, 0, nw + cout)
        with torch.no_grad():
            m.W_mu.copy_(torch.from_numpy(mu[:nw].reshape(cout, cin, k, k))); m.W_rho.copy_(torch.from_numpy(rho[:nw].reshape(cout, cin, k, k)))
            m.bias_mu.copy_(torch.from_numpy(mu[nw:])); m.bias_rho.copy_(torch.from_numpy(rho[nw:]))
        x = torch.from_numpy(O.normal_fill(seed, 2, 2, 0, 0, cin * H * W).reshape(1, cin, H, W)).requires_grad_(True)
        with EpsInjector() as inj:
            inj.load([m], seed, 5, 2)
            y = net(x)
        dy = torch.from_numpy(O.normal_fill(seed, 2, 3, 0, 0, y.numel()).reshape(y.shape))
        y.backward(dy)
        res[f"conv{ci}_shape"] = np.array([cin, cout, k, stride, H, W])
        res[f"conv{ci}_y"] = y.detach().numpy()[0]; res[f"conv{ci}_dx"] = x.grad.numpy()[0]
        res[f"conv{ci}_dmu"] = np.concatenate([m.W_mu.grad.numpy().ravel(), m.bias_mu.grad.numpy()])
        res[f"conv{ci}_drho"] = np.concatenate([m.W_rho.grad.numpy().ravel(), m.bias_rho.grad.numpy()])
    # (2) nn.Upsample(scale_factor=2, mode='nearest') (models/skip.py:102)
    x = torch.from_numpy(O.normal_fill(310, 2, 0, 0, 0, 3 * 5 * 7).reshape(1, 3, 5, 7)).requires_grad_(True)
    y = torch.nn.Upsample(scale_factor=2, mode='nearest')(x)
    dy = torch.from_numpy(O.normal_fill(310, 2, 1, 0, 0, y.numel()).reshape(y.shape)); y.backward(dy)
    res.update(up_y=y.detach().numpy()[0], up_dx=x.grad.numpy()[0])
    # (3) out_pred = out[:, :3].sigmoid(); gaussian_nll_inpainting(out_pred, out[:, 3:], img, mask) (bayesian_optimization.py:3033-3036)
    H, W = 12, 20
    o = (2.0 * O.normal_fill(311, 2, 0, 0, 0, 4 * H * W)).reshape(1, 4, H, W).copy(); o[0, 3, 0, :4] = [25.0, -30.0, 19.9, 0.0]
    tgt = O.uniform_fill(311, 1, 0, 0, 3 * H * W).reshape(1, 3, H, W)
    for mc in (1, 3):
        mask = (O.uniform_fill(311, 2 + mc, 0, 0, mc * H * W).reshape(1, mc, H, W) > 0.3).astype(np.float32)
        ot = torch.from_numpy(o.copy()).requires_grad_(True)
        nll = R["bu"].gaussian_nll_inpainting(ot[:, :3].sigmoid(), ot[:, 3:], torch.from_numpy(tgt), torch.from_numpy(mask)); nll.backward()
        res[f"nll_mask{mc}"] = float(nll); res[f"nll_mask{mc}_dout"] = ot.grad.numpy()[0]
    # (4) the reference's skip() with the inpainting runner's options, 3 scales, 24x24, K=1
    H = W = 24
    nd = nu = [8, 16, 16]
    net = R["mskip"].skip(8, num_output_channels=4, pad='reflection', num_channels_down=nd, num_channels_up=nu, num_channels_skip=[0, 0, 0],
                          filter_size_down=5, filter_size_up=3, filter_skip_size=1, need1x1_up=False, upsample_mode='nearest',
                          dropout_mode_down='None', dropout_mode_up='None', dropout_mode_skip='None', dropout_mode_output='None', need_sigmoid=False)
    net = R["f2b"].MeanFieldVI(net, prior={'mu': 0.0, 'sigma': 0.1}, replace_layers='all', reparam='')
    P, zin, zout, _ = skip_program(H, W, input_depth=8, n_out=4, nd=nd, nu=nu, ns=(0, 0, 0), fd=5, fu=3, need1x1_up=False, upsample_mode="nearest")
    layers = vi_layers(net); bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(layers) == len(P.layers) and len(bns) == len(P.bns), (len(layers), len(P.layers), len(bns), len(P.bns))
    seed = 21
    mu = 0.1 * O.normal_fill(seed, 2, 0, 0, 0, P.n_vi); rho = -3 + 0.1 * O.normal_fill(seed, 2, 1, 0, 0, P.n_vi)
    g = O.normal_fill(seed, 2, 7, 0, 0, P.n_bn); bn = np.zeros(P.n_bn, np.float32)
    with torch.no_grad():
        for m, l in zip(layers, P.layers):
            assert tuple(m.W_mu.shape) == (l["cout"], l["cin"], l["k"], l["k"]), (m.W_mu.shape, l)
            nw = m.W_mu.numel()
            m.W_mu.copy_(torch.from_numpy(mu[l["w_off"]:l["w_off"] + nw].reshape(m.W_mu.shape))); m.W_rho.copy_(torch.from_numpy(rho[l["w_off"]:l["w_off"] + nw].reshape(m.W_mu.shape)))
            m.bias_mu.copy_(torch.from_numpy(mu[l["b_off"]:l["b_off"] + l["cout"]])); m.bias_rho.copy_(torch.from_numpy(rho[l["b_off"]:l["b_off"] + l["cout"]]))
        for m, b in zip(bns, P.bns):
            c, off = b["C"], b["off"]
            assert m.num_features == c
            bn[off:off + c] = 1.0 + 0.1 * g[off:off + c]; bn[off + c:off + 2 * c] = 0.1 * g[off + c:off + 2 * c]
            m.weight.copy_(torch.from_numpy(bn[off:off + c])); m.bias.copy_(torch.from_numpy(bn[off + c:off + 2 * c]))
    net.train()
    z = torch.from_numpy(O.normal_fill(seed, 2, 2, 0, 0, 8 * H * W).reshape(1, 8, H, W)).requires_grad_(True)
    tgt = O.uniform_fill(312, 1, 0, 0, 3 * H * W).reshape(1, 3, H, W)
    mask = (O.uniform_fill(312, 2, 0, 0, H * W).reshape(1, 1, H, W) > 0.25).astype(np.float32)
    with EpsInjector() as inj:
        inj.load(layers, seed, 4, 0)
        out = net(z)
    nll = R["bu"].gaussian_nll_inpainting(out[:, :3].sigmoid(), out[:, 3:], torch.from_numpy(tgt), torch.from_numpy(mask))
    nll.backward()
    dmu = np.zeros(P.n_vi, np.float32); drho = np.zeros(P.n_vi, np.float32); dbn = np.zeros(P.n_bn, np.float32)
    for m, l in zip(layers, P.layers):
        nw = m.W_mu.numel()
        dmu[l["w_off"]:l["w_off"] + nw] = m.W_mu.grad.numpy().ravel(); drho[l["w_off"]:l["w_off"] + nw] = m.W_rho.grad.numpy().ravel()
        dmu[l["b_off"]:l["b_off"] + l["cout"]] = m.bias_mu.grad.numpy(); drho[l["b_off"]:l["b_off"] + l["cout"]] = m.bias_rho.grad.numpy()
    for m, b in zip(bns, P.bns):
        c, off = b["C"], b["off"]
        dbn[off:off + c] = m.weight.grad.numpy(); dbn[off + c:off + 2 * c] = m.bias.grad.numpy()
    res.update(net_out=out.detach().numpy()[0], net_nll=float(nll), net_dmu=dmu, net_drho=drho, net_dbn=dbn, net_dz=z.grad.numpy()[0],
               net_keys=np.array([k for k in net.state_dict().keys()]))
    np.savez_compressed(os.path.join(GOLD, "inpainting.npz"), **res)
    print("inpainting ok: nll", float(nll), "layers", len(layers))


def golden_siblings():
    """The non-Bayesian siblings on the reference's own skip() net with plain nn.Conv2d:
    DIP (bayesian_optimization.py:1064-1237), MC dropout (:1447-1655, the reference's conv() builds the nn.Dropout2d layers;
    masks injected from RNG domain 5) and SGLD (:1658-1860; add_noise :166-170 restated with noise injected from RNG domain 4),
    torch AdamW(weight_decay) and ExponentialLR.  Three optimizer steps each; first-step output / gradients and the
    final parameters are stored."""
    import torch.nn.functional as F
    onet_args = dict(input_depth=8, n_out=2, nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4))
    H = W = 32; steps = 3; seed = 41; lr = 3e-4
    res = dict(H=H, W=W, steps=steps, seed=seed, lr=lr)
    for method, p_drop, wd, gamma in (("dip", 0.0, 0.0, 1.0), ("mcd", 0.3, 3e-4, 1.0), ("sgld", 0.0, 5e-8, 0.996)):
        onet = O.make_net(H, W, drop_down=p_drop, drop_up=p_drop, **onet_args)
        conv, bn, n_vi, n_bnp = O.net_table(onet)
        mu, _, bnp = test_params(onet, seed)
        mode = '2d' if p_drop else 'None'
        n = onet.n_scales
        net = R["mskip"].skip(onet.input_depth, onet.n_out, num_channels_down=[onet.nd[i] for i in range(n)],
                              num_channels_up=[onet.nu[i] for i in range(n)], num_channels_skip=[onet.ns[i] for i in range(n)],
                              upsample_mode='bilinear', downsample_mode='stride', need_sigmoid=False, need_bias=True, pad='reflection',
                              act_fun='LeakyReLU', dropout_mode_down=mode, dropout_p_down=p_drop, dropout_mode_up=mode, dropout_p_up=p_drop,
                              dropout_mode_skip='None', dropout_mode_output='None')
        convs = [m for m in net.modules() if isinstance(m, torch.nn.Conv2d)]
        assert len(convs) == len(conv)
        with torch.no_grad():
            for m, row in zip(convs, conv):
                cin, cout, k, stride, w_off, b_off = [int(v) for v in row]
                m.weight.copy_(torch.from_numpy(mu[w_off:w_off + cout * cin * k * k].reshape(cout, cin, k, k)))
                m.bias.copy_(torch.from_numpy(mu[b_off:b_off + cout]))
            for m, (c, off) in zip(bn_layers(net), bn):
                c, off = int(c), int(off)
                m.weight.copy_(torch.from_numpy(bnp[off:off + c])); m.bias.copy_(torch.from_numpy(bnp[off + c:off + 2 * c]))
        state = dict(layer=-1, step=0)
        for lid, m in enumerate(convs):
            m.register_forward_pre_hook(lambda mod, inp, lid=lid: state.__setitem__("layer", lid))

        def dropout2d(x, p=0.5, training=True, inplace=False):
            assert training and x.shape[0] == 1
            d = O.dropout_mask(seed, state["step"], 0, state["layer"], p, x.shape[1])
            return x * torch.from_numpy(d)[None, :, None, None]
        orig = F.dropout2d; F.dropout2d = dropout2d
        try:
            z0 = (0.1 * O.uniform_fill(seed, 0, 0, 0, onet.input_depth * H * W)).reshape(1, onet.input_depth, H, W)
            tgt = torch.from_numpy(O.noisy(O.phantom(H, W, seed), 0.1, seed))[None, None]
            opt = torch.optim.AdamW(net.parameters(), lr=lr, weight_decay=wd)
            sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=gamma) if method == "sgld" else None
            losses = []
            for it in range(steps):
                state["step"] = it
                opt.zero_grad()
                if method == "sgld":          # add_noise(net, 2, LR): 4-D parameters only, noise * sigma * lr0
                    for lid, m in enumerate(convs):
                        nz = O.normal_fill(seed, 4, lid, 0, it, m.weight.numel()).reshape(tuple(m.weight.shape))
                        m.weight.data = m.weight.data + torch.from_numpy(nz) * 2 * lr
                zn = O.normal_fill(seed, 1, 0, 0, it, z0.size).reshape(z0.shape)
                out = net(torch.from_numpy(z0 + 0.1 * zn))
                if method == "mcd":
                    loss = R["bu"].gaussian_nll(out[:, :1], out[:, 1:], tgt)
                else:
                    loss = F.mse_loss(out[:, :1], tgt)
                loss.backward()
                if it == 0:
                    g_mu = np.zeros(n_vi, np.float32); g_bn = np.zeros(n_bnp, np.float32)
                    for m, row in zip(convs, conv):
                        cin, cout, k, stride, w_off, b_off = [int(v) for v in row]
                        g_mu[w_off:w_off + cout * cin * k * k] = m.weight.grad.numpy().ravel(); g_mu[b_off:b_off + cout] = m.bias.grad.numpy()
                    for m, (c, off) in zip(bn_layers(net), bn):
                        c, off = int(c), int(off)
                        g_bn[off:off + c] = m.weight.grad.numpy(); g_bn[off + c:off + 2 * c] = m.bias.grad.numpy()
                    res[method + "_out0"] = out.detach().numpy()[0].copy(); res[method + "_dmu0"] = g_mu; res[method + "_dbn0"] = g_bn
                opt.step()
                if sched is not None and sched.get_last_lr()[0] > 1e-8:
                    sched.step()
                losses.append(float(loss))
        finally:
            F.dropout2d = orig
        f_mu = np.zeros(n_vi, np.float32); f_bn = np.zeros(n_bnp, np.float32)
        for m, row in zip(convs, conv):
            cin, cout, k, stride, w_off, b_off = [int(v) for v in row]
            f_mu[w_off:w_off + cout * cin * k * k] = m.weight.detach().numpy().ravel(); f_mu[b_off:b_off + cout] = m.bias.detach().numpy()
        for m, (c, off) in zip(bn_layers(net), bn):
            c, off = int(c), int(off)
            f_bn[off:off + c] = m.weight.detach().numpy(); f_bn[off + c:off + 2 * c] = m.bias.detach().numpy()
        res.update({method + "_loss": np.array(losses), method + "_mu": f_mu, method + "_bn": f_bn, method + "_wd": wd,
                    method + "_gamma": gamma, method + "_p": p_drop})
        print("sibling", method, "losses", losses)
    np.savez_compressed(os.path.join(GOLD, "siblings.npz"), **res)


def golden_inp_dip_loss():
    """run_inp_dip's data term (bayesian_optimization.py:2822-2826), torch ops as the reference writes them, with a 1- and a 3-channel mask."""
    import torch.nn.functional as F
    H, W = 12, 20
    res = {}
    for mc in (1, 3):
        out = torch.from_numpy(O.normal_fill(50 + mc, 2, 1, 0, 0, 4 * H * W).reshape(1, 4, H, W).copy()).requires_grad_(True)
        img = torch.from_numpy(O.uniform_fill(50 + mc, 2, 0, 0, 3 * H * W).reshape(1, 3, H, W).copy())
        mask = torch.from_numpy((O.uniform_fill(50 + mc, 3, 0, 0, mc * H * W) > 0.3).astype(np.float32).reshape(1, mc, H, W))
        out_pred = out[:, :3].sigmoid()
        loss = F.mse_loss(out_pred * mask, img * mask)
        loss.backward()
        res.update({"out%d" % mc: out.detach().numpy()[0], "img%d" % mc: img.numpy()[0], "mask%d" % mc: mask.numpy()[0],
                    "loss%d" % mc: float(loss), "grad%d" % mc: out.grad.numpy()[0]})
    np.savez_compressed(os.path.join(GOLD, "inp_dip_loss.npz"), **res)
    print("inp dip loss", res["loss1"], res["loss3"])


def golden_bookkeeping():
    """The runners' per-iteration bookkeeping with torch ops in the reference's order and the reference's own PSNR / SSIM
    (utils/common_utils.py:297-353; bayesian_optimization.py itself is not importable: cv2 / gpytorch):
      den  bayesian_optimization.py:1374-1416   (2 channels, noisy + gt metrics)
      sr   :2190-2236                           (metrics of the low-resolution projection in column 0)
      ct   :584-626                             (1 channel, no aleatoric map)
      inp  :3039-3090                           (sigmoid colour channels, masked PSNR / SSIM)
    Inputs are synthetic raw network outputs regenerated from seeds by the tests; 28 iterations > 25 ring slots, so the ring
    wraps, and the snapshot at iteration 10 sees the ring's still-zero slots like the reference's torch.var over all 25."""
    psnr, ssim = R["cu"].peak_signal_noise_ratio, R["cu"].structural_similarity
    mse = torch.nn.MSELoss()
    n_it, w, mc_iter = 28, 0.99, 25
    res = dict(n_it=n_it, snap=np.array([10, 27]))
    for task, (H, W, C) in dict(den=(32, 40, 2), sr=(32, 48, 2), ct=(24, 32, 1)).items():
        seed = dict(den=61, sr=62, ct=63)[task]
        img = O.phantom(H, W, seed); noisy = O.noisy(img, 0.1, seed)
        img_t = torch.from_numpy(img)[None, None]; noisy_t = torch.from_numpy(noisy)[None, None]
        down = lambda x: torch.nn.functional.interpolate(x, scale_factor=0.25, mode='nearest', recompute_scale_factor=False)
        small_t = down(img_t)
        ring_epi = torch.zeros((mc_iter, H, W)); ring_ale = torch.zeros((mc_iter, H, W))
        out_avg = None
        M = np.zeros((n_it, 8)); snaps = {}
        for i in range(n_it):
            raw = bookkeeping_raw(task, seed, i, img, C)
            out = torch.from_numpy(raw.copy())[None]
            out_lr = down(out)
            if C > 1:
                out[:, 1:] = torch.exp(-out[:, 1:])
            out_avg = out.detach() if out_avg is None else out_avg * w + out.detach() * (1 - w)
            _out = out[:, :1].clip(0, 1); _out_avg = out_avg[:, :1].clip(0, 1)
            ring_epi[i % mc_iter] = _out[0]
            if C > 1:
                ring_ale[i % mc_iter] = out[:, 1:].clip(0, 1)[0]
            if task == "den":
                M[i] = [mse(out_avg[:, :1], noisy_t).item(), mse(out_avg[:, :1], img_t).item(),
                        psnr(noisy_t, _out), psnr(img_t, _out), psnr(img_t, _out_avg), ssim(noisy_t, _out), ssim(img_t, _out), ssim(img_t, _out_avg)]
            elif task == "sr":
                _out_lr = out_lr[:, :1].clip(0, 1)
                M[i] = [mse(down(out_avg)[:, :1], small_t).item(), mse(out_avg[:, :1], img_t).item(),
                        psnr(small_t, _out_lr), psnr(img_t, _out), psnr(img_t, _out_avg), ssim(small_t, _out_lr), ssim(img_t, _out), ssim(img_t, _out_avg)]
            else:
                m0 = mse(out_avg[:, :1], img_t).item(); p0 = psnr(img_t, _out); s0 = ssim(img_t, _out)
                M[i] = [m0, m0, p0, p0, psnr(img_t, _out_avg), s0, s0, ssim(img_t, _out_avg)]
            if i in (10, 27):
                snaps[i] = (torch.var(ring_epi, dim=0).numpy().copy(), torch.mean(ring_ale, dim=0).numpy().copy(), _out_avg[0, 0].numpy().copy())
        res.update({task + "_metrics": M, task + "_ema": out_avg[0].numpy(), task + "_shape": np.array([H, W, C])})
        for i, (v, a, r) in snaps.items():
            res.update({"%s_var%d" % (task, i): v, "%s_ale%d" % (task, i): a, "%s_recon%d" % (task, i): r})
    # inpainting
    H, W, seed = 24, 32, 64
    img = np.stack([O.phantom(H, W, seed + c) for c in range(3)])
    img_t = torch.from_numpy(img)[None]
    for mc in (1, 3):
        mask = (O.uniform_fill(seed, 2 + mc, 0, 0, mc * H * W).reshape(1, mc, H, W) > 0.3).astype(np.float32)
        mask_t = torch.from_numpy(mask)
        ring_epi = torch.zeros((mc_iter, 3, H, W)); ring_ale = torch.zeros((mc_iter, H, W))
        out_avg = None; M = np.zeros((n_it, 8)); snaps = {}
        for i in range(n_it):
            raw = bookkeeping_raw("inp", seed, i, img, 4)
            out = torch.from_numpy(raw.copy())[None]
            out_pred = out[:, :3].sigmoid()
            out[:, :3] = out_pred
            out[:, 3:] = torch.exp(-out[:, 3:])
            out_avg = out.detach() if out_avg is None else out_avg * w + out.detach() * (1 - w)
            _out = out[:, :3].clip(0, 1); _out_avg = out_avg[:, :3].clip(0, 1); _out_ale = out[:, 3:].clip(0, 1)
            ring_epi[i % mc_iter] = _out[0]; ring_ale[i % mc_iter] = _out_ale[0]
            m0 = mse(out_avg[:, :3], img_t).item()
            M[i] = [m0, m0, psnr(img_t, _out), psnr(img_t * mask_t, _out * mask_t), psnr(img_t * mask_t, _out_avg * mask_t),
                    ssim(img_t, _out), ssim(img_t * mask_t, _out * mask_t), ssim(img_t * mask_t, _out_avg * mask_t)]
            if i in (10, 27):
                snaps[i] = (torch.var(ring_epi, dim=0).numpy().copy(), torch.mean(ring_ale, dim=0).numpy().copy(), _out_avg[0].numpy().copy())
        res.update({"inp%d_metrics" % mc: M, "inp%d_ema" % mc: out_avg[0].numpy(), "inp_shape": np.array([H, W, 4])})
        for i, (v, a, r) in snaps.items():
            res.update({"inp%d_var%d" % (mc, i): v, "inp%d_ale%d" % (mc, i): a, "inp%d_recon%d" % (mc, i): r})
    np.savez_compressed(os.path.join(GOLD, "bookkeeping.npz"), **res)
    print("bookkeeping ok: den psnr_gt_sm[-1] %.4f, inp1 psnr %.4f" % (res["den_metrics"][-1, 4], res["inp1_metrics"][-1, 4]))


def bookkeeping_raw(task, seed, i, img, C):
    """Synthetic raw network output of iteration i, regenerated identically by tests/test_gpu_bookkeeping.py (oracle.bookkeeping_raw)."""
    return O.bookkeeping_raw(task, seed, i, img, C)


def golden_lrt():
    """Local reparameterisation: the reference's own Conv2dLRT layers (MeanFieldVI(reparam='local'),
    BayTorch/modules/reparam_layers.py:39-72) with eps injected in OUTPUT space from RNG domain 7 (stream = layer, element j of
    [Cout][Ho][Wo]): single layers forward / backward, and a 2-scale den net with K = 2."""
    from models.common import conv as ref_conv
    res = {}
    cases = [(16, 4, 1, 1, 12, 12), (16, 16, 3, 2, 16, 16), (36, 16, 3, 1, 8, 8), (8, 12, 5, 1, 12, 16), (7, 5, 3, 1, 9, 11)]
    for ci, (cin, cout, k, stride, H, W) in enumerate(cases):
        seq = ref_conv(cin, cout, k, stride, bias=True, pad='reflection')
        net = R["f2b"].MeanFieldVI(seq, prior={'mu': 0.0, 'sigma': 0.1}, replace_layers='all', reparam='local')
        m = vi_layers(net)[0]
        assert type(m).__name__ == "Conv2dLRT"
        seed = 400 + ci
        nw = cout * cin * k * k
        mu = 0.1 * O.normal_fill(seed, 2, 0, 0, 0, nw + cout); rho = -3 + 0.5 * O.normal_fill(seed, 2, 1, 0, 0, nw + cout)
        with torch.no_grad():
            m.W_mu.copy_(torch.from_numpy(mu[:nw].reshape(cout, cin, k, k))); m.W_rho.copy_(torch.from_numpy(rho[:nw].reshape(cout, cin, k, k)))
            m.bias_mu.copy_(torch.from_numpy(mu[nw:])); m.bias_rho.copy_(torch.from_numpy(rho[nw:]))
        x = torch.from_numpy(O.normal_fill(seed, 2, 2, 0, 0, cin * H * W).reshape(1, cin, H, W)).requires_grad_(True)
        with EpsInjector() as inj:
            Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
            inj.queue[:] = [torch.from_numpy(O.normal_fill(seed, 7, 0, 2, 5, cout * Ho * Wo).reshape(1, cout, Ho, Wo))]      # layer 0, sample 2, step 5
            y = net(x)
        dy = torch.from_numpy(O.normal_fill(seed, 2, 3, 0, 0, y.numel()).reshape(y.shape))
        y.backward(dy)
        res[f"case{ci}_shape"] = np.array([cin, cout, k, stride, H, W])
        res[f"case{ci}_y"] = y.detach().numpy()[0]; res[f"case{ci}_dx"] = x.grad.numpy()[0]
        res[f"case{ci}_dmu"] = np.concatenate([m.W_mu.grad.numpy().ravel(), m.bias_mu.grad.numpy()])
        res[f"case{ci}_drho"] = np.concatenate([m.W_rho.grad.numpy().ravel(), m.bias_rho.grad.numpy()])
        net.eval()
        with torch.no_grad():
            res[f"case{ci}_y_eval"] = net(x).numpy()[0]
    res["n_cases"] = len(cases)
    # 2-scale den net, K = 2, reference loop (gaussian_nll + temp * kl)
    onet = O.make_net(32, 32, input_depth=8, n_out=2, nd=(8, 16), nu=(8, 16), ns=(4, 4))
    temp = DEN["temp"]; prior_raw = float(np.sqrt(temp) * DEN["sigma"])
    conv, bn, n_vi, n_bnp = O.net_table(onet)
    seed, K, step = 25, 2, 3
    mu, rho, bnp = test_params(onet, seed)
    n = onet.n_scales
    net = R["mskip"].skip(onet.input_depth, onet.n_out, num_channels_down=[onet.nd[i] for i in range(n)], num_channels_up=[onet.nu[i] for i in range(n)],
                          num_channels_skip=[onet.ns[i] for i in range(n)], upsample_mode='bilinear', downsample_mode='stride', need_sigmoid=False,
                          need_bias=True, pad='reflection', act_fun='LeakyReLU', dropout_mode_down='None', dropout_mode_up='None',
                          dropout_mode_skip='None', dropout_mode_output='None')
    net = R["f2b"].MeanFieldVI(net, prior={'mu': 0.0, 'sigma': prior_raw}, replace_layers='all', reparam='local')
    load_flat(net, mu, rho, bnp, conv, bn)
    layers = vi_layers(net)
    H = W = 32
    z = (0.1 * O.uniform_fill(seed, 0, 0, 0, onet.input_depth * H * W)).reshape(1, onet.input_depth, H, W)
    tgt = torch.from_numpy(O.noisy(O.phantom(H, W, seed), 0.1, seed))[None, None]
    # output sizes of the layers in call order (conv table: cin, cout, k, stride, w_off, b_off) — recorded by a dry forward
    shapes = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: shapes.append(tuple(out.shape))) for m in layers]
    net.eval()
    with torch.no_grad():
        net(torch.from_numpy(z))
    for h in hooks:
        h.remove()
    net.train(); net.zero_grad()
    outs = []; nll_sum = 0.0
    with EpsInjector() as inj:
        for kk in range(K):
            inj.queue[:] = [torch.from_numpy(O.normal_fill(seed, 7, lid, kk, step, int(np.prod(sh))).reshape(sh)) for lid, sh in enumerate(shapes)]
            out = net(torch.from_numpy(z))
            nll = R["bu"].gaussian_nll(out[:, :1], out[:, 1:], tgt)
            (nll / K).backward(); nll_sum += float(nll) / K
            outs.append(out.detach().numpy()[0].copy())
        kl = net.kl(); (temp * kl).backward()
    dmu, drho, dbn = flat_grads(net, conv, bn, n_vi, n_bnp)
    res.update(net_seed=seed, net_K=K, net_step=step, net_temp=temp, net_prior_sigma=np.float32(prior_raw + 1e-6), net_out=np.stack(outs), net_nll=nll_sum,
               net_kl=float(kl), net_dmu=dmu, net_drho=drho, net_dbn=dbn,
               net_layer_types=np.array([type(m).__name__ for m in layers]), net_keys=np.array(list(net.state_dict().keys())))
    np.savez_compressed(os.path.join(GOLD, "lrt.npz"), **res)
    print("lrt ok: net nll", nll_sum, "kl", float(kl), "|dmu|", np.linalg.norm(dmu), "|drho|", np.linalg.norm(drho))


if __name__ == "__main__":
    os.makedirs(GOLD, exist_ok=True)
    if "--fullsize" in sys.argv:        # BASELINE configs 2-4 at 256^2 (strided) + the bf16-parameter twin of the 128^2 den net
        golden_net("full_den_256_k1", O.make_net(256, 256), seed=1, K=1, task="den", full_arrays=False, compact=True)
        golden_net("full_sr256_d32_k1", O.make_net(256, 256, input_depth=32), seed=2, K=1, task="sr", full_arrays=False, compact=True)
        golden_net("full_ct_256_k1", O.make_net(256, 256, n_out=1), seed=1, K=1, task="ct", full_arrays=False, compact=True)
        golden_net("full_den_128_k1_bf16", O.make_net(128, 128), seed=1, K=1, task="den", full_arrays=False, bf16=True)
        sys.exit(0)
    if "--lrt" in sys.argv:
        golden_lrt(); sys.exit(0)
    if "--posterior" in sys.argv:
        golden_posterior(); sys.exit(0)
    if "--crop" in sys.argv:            # sides not divisible by 2^n_scales: Concat's centre-crop (models/common.py:29-41) at the deepest scale, both dims
        golden_net("crop_den_36x44_k1", O.make_net(36, 44, input_depth=8, n_out=2, nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4)), seed=31, K=1, task="den",
                   full_arrays=True)
        sys.exit(0)
    if "--bookkeeping" in sys.argv:
        golden_bookkeeping(); sys.exit(0)
    if "--inp-dip" in sys.argv:
        golden_inp_dip_loss(); sys.exit(0)
    if "--fitcurve" in sys.argv:          # minutes of CPU: the reference's loop for 400 / 100 iterations, float32 and float64
        golden_fitcurve("fitcurve_den_64", 64, seed=1, steps=400)
        golden_fitcurve("fitcurve_den_128", 128, seed=1, steps=100)
        sys.exit(0)
    if "--siblings" in sys.argv:
        golden_siblings(); sys.exit(0)
    if "--inpainting" in sys.argv:       # only the inpainting fixtures (the others are unchanged)
        golden_inpainting(); sys.exit(0)
    golden_layers()
    golden_micro()
    small = O.make_net(32, 32, input_depth=8, n_out=2, nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4))
    golden_net("small_den_k2", small, seed=21, K=2, task="den", full_arrays=True)
    golden_net("small_sr_k1", O.make_net(32, 32, input_depth=8, n_out=2, nd=(8, 16), nu=(8, 16), ns=(4, 4)), seed=22, K=1, task="sr")
    golden_net("small_ct_k1", O.make_net(32, 32, input_depth=8, n_out=1, nd=(8, 16), nu=(8, 16), ns=(4, 4)), seed=23, K=1, task="ct")
    golden_net("full_den_64_k1", O.make_net(64, 64), seed=1, K=1, task="den", full_arrays=False)
    golden_net("full_den_128_k1", O.make_net(128, 128), seed=1, K=1, task="den", full_arrays=False)
    golden_traj("traj_small_k1", small, seed=31, K=1, steps=4)
    golden_traj("traj_small_k2", small, seed=32, K=2, steps=3)
    golden_inpainting()
    golden_siblings()
    golden_inp_dip_loss()
    golden_bookkeeping()
    golden_lrt()
    golden_posterior()
