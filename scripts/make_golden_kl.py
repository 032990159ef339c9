"""Writes tests/golden/kl_forward.npz: the reference's KL term in the forward direction, KL(posterior || prior), evaluated by its own
VIModule(..., kl_type='forward') (BayTorch/modules/module.py:9-80) and MeanFieldVI(..., kl_type='forward', reparam='')
(BayTorch/freq_to_bayes.py:9-48) in float32 on the CPU, loaded from a checkout at generation time (torchvision / skimage, which `models`
imports and this path never uses, are empty in-process stub modules).  Beside every float32 result: the float64 value and autograd gradients
of the same torch expression, kl_divergence(Normal(mu, softplus(rho)), Normal(m0, s0)).sum(), with s0 the layer's float32 prior scale.

usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_kl.py <reference checkout> [out.npz]

Layer cases (tests/kl_restatement.py LAYER_CASES; weight size 1031, bias size 7), keys per case <c>:
  <c>_mu, <c>_rho        float32 [1038]: W_mu | bias_mu and W_rho | bias_rho, each distinct array once (kl_restatement.INPUTS: c2 and c5 read
                         c1's, c4 reads c1's mu)
  <c>_prior              float32 [2]: the prior's loc and its effective scale, float32(sigma + 1e-6)
  <c>_kl, <c>_dmu, <c>_drho          the module's _kl (float32) and its autograd gradients (float32 [1038])
  <c>_kl64, <c>_dmu64, <c>_drho64    the same in float64 (not for c5, which must equal c1)
Net case, the two-scale net of tests/test_gpu_dropin.py with prior sigma 0.1:
  net_keys               the state_dict keys of the W_mu / W_rho / bias_mu / bias_rho tensors, in order
  net_p<i>               float32: tensor i of that list
  net_layers, net_layer_kl   the names of the VI layers in modules() order and each one's _kl (float32)
  net_kl                 net.kl() (float32), net_kl64 the float64 sum over all layers
  net_prior              float32 [2] as above"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "kl_forward.npz")
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    for m in ("torchvision", "torchvision.transforms", "skimage", "skimage.metrics"):
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.modules["skimage.metrics"].peak_signal_noise_ratio = None
    sys.path.insert(0, ref)
    import torch
    from torch.distributions.kl import kl_divergence
    from torch.distributions.normal import Normal
    from torch.nn.functional import softplus
    import kl_restatement as R
    from BayTorch.freq_to_bayes import MeanFieldVI
    from BayTorch.modules.module import VIModule
    import models

    def f64(mu, rho, m0, s0):
        m = torch.from_numpy(mu).double().requires_grad_(True)
        r = torch.from_numpy(rho).double().requires_grad_(True)
        kl = kl_divergence(Normal(m, softplus(r)), Normal(torch.tensor(float(m0), dtype=torch.float64), torch.tensor(float(s0), dtype=torch.float64))).sum()
        kl.backward()
        return kl.item(), m.grad.numpy(), r.grad.numpy()

    res = {}
    n = R.N_W + R.N_B
    for ci, (name, (sigma, m0, kl_type)) in enumerate(R.LAYER_CASES.items()):
        rng = np.random.default_rng(3000 + ci)
        own_mu, own_rho = (m0 + 0.1 * rng.standard_normal(n)).astype(np.float32), (-3.0 + (2.0 if name == "c4" else 0.1) * rng.standard_normal(n)).astype(np.float32)
        if name == "c4":      # both softplus tails, in the weight and in the bias block
            own_rho[[3, 500, R.N_W + 2]] = 15.0
            own_rho[[4, 777, R.N_W + 5]] = -20.0
        if R.INPUTS[name][0] == name:
            res[name + "_mu"] = own_mu
        if R.INPUTS[name][1] == name:
            res[name + "_rho"] = own_rho
        mu, rho = R.case_inputs(res, name)
        mod = VIModule(None, (R.N_W,), (R.N_B,), prior={"mu": m0, "sigma": sigma}, kl_type=kl_type)
        with torch.no_grad():
            mod.W_mu.copy_(torch.from_numpy(mu[:R.N_W])); mod.bias_mu.copy_(torch.from_numpy(mu[R.N_W:]))
            mod.W_rho.copy_(torch.from_numpy(rho[:R.N_W])); mod.bias_rho.copy_(torch.from_numpy(rho[R.N_W:]))
        kl = mod._kl
        kl.backward()
        prior = np.array([float(mod.prior.loc), float(mod.prior.scale)], np.float32)
        assert mod.prior.scale.dtype == torch.float32
        dmu = np.concatenate([mod.W_mu.grad.numpy(), mod.bias_mu.grad.numpy()]).astype(np.float32)
        drho = np.concatenate([mod.W_rho.grad.numpy(), mod.bias_rho.grad.numpy()]).astype(np.float32)
        res[name + "_prior"], res[name + "_kl"], res[name + "_dmu"], res[name + "_drho"] = prior, np.float32(kl.item()), dmu, drho
        k64, dm64, dr64 = f64(mu, rho, prior[0], prior[1])
        dev = (abs(kl.item() - k64) / abs(k64), R.relerr(dmu, dm64), R.relerr(drho, dr64))
        print("%s: scale %.6e  kl %.6e  float32 against float64: value %.2e, dmu %.2e, drho %.2e" % ((name, prior[1], k64) + dev))
        if name != "c5":
            res[name + "_kl64"], res[name + "_dmu64"], res[name + "_drho64"] = np.float64(k64), dm64, dr64
    torch.manual_seed(7)
    net = models.get_net(8, "skip", "reflection", skip_n33d=[8, 16], skip_n33u=[8, 16], skip_n11=4, num_scales=2, n_channels=2, upsample_mode="bilinear")
    net = MeanFieldVI(net, prior={"mu": 0, "sigma": 0.1}, kl_type="forward", reparam="")
    layers = [(k, m) for k, m in net.named_modules() if isinstance(m, VIModule)]
    keys = [k for k in net.state_dict() if k.rsplit(".", 1)[-1] in ("W_mu", "W_rho", "bias_mu", "bias_rho")]
    res["net_keys"] = np.asarray(keys)
    for i, k in enumerate(keys):
        res["net_p%d" % i] = net.state_dict()[k].numpy().astype(np.float32)
    res["net_layers"] = np.asarray([k for k, _ in layers])
    res["net_layer_kl"] = np.asarray([m._kl.item() for _, m in layers], np.float32)
    res["net_kl"] = np.float32(net.kl().item())
    s0 = layers[0][1].prior.scale
    res["net_prior"] = np.array([0.0, float(s0)], np.float32)
    tot = 0.0
    for _, m in layers:
        mu = np.concatenate([m.W_mu.detach().numpy().ravel(), m.bias_mu.detach().numpy().ravel()] if m.bias_mu is not None else [m.W_mu.detach().numpy().ravel()])
        rho = np.concatenate([m.W_rho.detach().numpy().ravel(), m.bias_rho.detach().numpy().ravel()] if m.bias_rho is not None else [m.W_rho.detach().numpy().ravel()])
        tot += f64(mu, rho, 0.0, float(s0))[0]
    res["net_kl64"] = np.float64(tot)
    print("net: %d VI layers, %d tensors, kl %.6e (float32 against float64: %.2e)" % (len(layers), len(keys), tot, abs(float(res["net_kl"]) - tot) / tot))
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 200 * 1024


if __name__ == "__main__":
    main()
