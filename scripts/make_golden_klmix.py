"""Writes tests/golden/kl_mixture.npz: the reference's Monte-Carlo KL term against a scale-mixture prior, evaluated by its own
VIModule(..., prior={'mu', 'sigma', 'pi'}, kl_type='forward') (BayTorch/modules/module.py:32-35, 64-80; distributions/distributions.py:6-35)
and MeanFieldVI(..., kl_type='forward', reparam='') in float32 on the CPU, loaded from a checkout at generation time (stub modules as in
scripts/make_golden_kl.py).  The reference draws eps inside _kl (Normal.rsample, W then bias); the draw is injected without patching
anything: torch.manual_seed(S) before _kl, and torch.manual_seed(S) again followed by torch.empty(shape).normal_() per tensor in the same
order reproduces it.  Beside every float32 result: the float64 value and autograd gradients of the same expression at that eps
(log-sum-exp form), and the float32 numpy emulation of the kernels' statement (tests/klmix_restatement.py emulate32) with its error.

usage:  PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_klmix.py <reference checkout> [out.npz]

Layer cases (klmix_restatement.CASES; weight size 1031, bias size 7), shared inputs once:
  mu, eps                float32 [1038]: W | bias; eps is the draw of seed EPS_SEED
  rho_lo, rho_hi         float32 [1038]: rho ~ N(-3, 0.1), the first 300 entries linspace(-12, 1.5) / linspace(-12, 6)
keys per case <c>:
  <c>_prior              float32 [3, J]: pi, component means, the FINAL scales (the module's own float32 prior.scale)
  <c>_kl64, <c>_dmu64, <c>_drho64    float64 value and autograd gradients
  <c>_emu_kl, <c>_emu_err            the emulation's value, and its errors [value relative, dmu relerr, drho relerr] against float64
  <c>_kl, <c>_dmu, <c>_drho          reference-finite cases only: the module's _kl (float32) and its autograd gradients (recorded, not
                                     compared: autograd forms d/dmu as eps/s - eps/s + ..., the cancellation leaves float32 noise)
A reference-finite case whose reference value is not finite is refused; for the others the reference's own value is printed.
Net case, MeanFieldVI(..., kl_type='forward', reparam='') on the two-scale net of tests/test_gpu_dropin.py (the parameters of
tests/golden/kl_forward.npz: same seed, same construction) with prior m3:
  net_prior              float32 [3, J] as above
  net_eps                float32 [9434]: the draw net.kl() used, flat, layer after layer W | bias
  net_kl                 net.kl() (float32); net_kl64, net_layer_kl64: float64 at that draw"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS_SEED = 1234


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "kl_mixture.npz")
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    for m in ("torchvision", "torchvision.transforms", "skimage", "skimage.metrics"):
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.modules["skimage.metrics"].peak_signal_noise_ratio = None
    sys.path.insert(0, ref)
    import warnings
    import torch
    from torch.nn.functional import softplus
    import klmix_restatement as R
    from BayTorch.freq_to_bayes import MeanFieldVI
    from BayTorch.modules.module import VIModule
    import models
    warnings.filterwarnings("ignore", message="To copy construct from a tensor")

    def f64(mu, rho, eps, prior):
        """float64 value and autograd gradients of log q(w) - log p(w) at w = mu + s eps, the mixture through torch.logsumexp."""
        # (log q through Normal.log_prob would leave the cancellation noise of eps/s - eps/s, ~1e-10 of the largest entry at rho = -12, in d/dmu)
        m = torch.from_numpy(np.asarray(mu, np.float64)).requires_grad_(True)
        r = torch.from_numpy(np.asarray(rho, np.float64)).requires_grad_(True)
        e = torch.from_numpy(np.asarray(eps, np.float64))
        pi, loc, sc = (torch.from_numpy(np.asarray(x, np.float64))[:, None] for x in prior)
        s = softplus(r)
        w = m + s * e
        lq = -0.5 * e * e - torch.log(s) - 0.5 * np.log(2.0 * np.pi)      # Normal(m, s).log_prob(w) at w = m + s e: written so, autograd does not form eps/s - eps/s
        lp = torch.logsumexp(torch.log(pi) + torch.distributions.Normal(loc, sc).log_prob(w[None, :]), dim=0)
        kl = (lq - lp).sum()
        kl.backward()
        return kl.item(), m.grad.numpy(), r.grad.numpy()

    def draw(shapes):
        torch.manual_seed(EPS_SEED)
        return [torch.empty(s).normal_().numpy().ravel() for s in shapes]

    res = {}
    n = R.N_W + R.N_B
    rng = np.random.default_rng(4000)
    res["mu"] = (0.1 * rng.standard_normal(n)).astype(np.float32)
    res["rho_lo"], res["rho_hi"] = R.case_rho(np.random.default_rng(4001), n, 1.5), R.case_rho(np.random.default_rng(4001), n, 6.0)
    res["eps"] = np.concatenate(draw([(R.N_W,), (R.N_B,)])).astype(np.float32)
    for name, (pi, sigma, loc, rho_hi, finite) in R.CASES.items():
        mu, rho, eps = res["mu"], res["rho_lo" if rho_hi == 1.5 else "rho_hi"], res["eps"]
        mod = VIModule(None, (R.N_W,), (R.N_B,), prior={"mu": list(loc), "sigma": np.asarray(sigma, np.float32), "pi": list(pi)}, kl_type="forward")
        with torch.no_grad():
            mod.W_mu.copy_(torch.from_numpy(mu[:R.N_W])); mod.bias_mu.copy_(torch.from_numpy(mu[R.N_W:]))
            mod.W_rho.copy_(torch.from_numpy(rho[:R.N_W])); mod.bias_rho.copy_(torch.from_numpy(rho[R.N_W:]))
        assert mod.prior.scale.dtype == torch.float32 and mod.prior.pi.dtype == torch.float32 and mod.prior.loc.dtype == torch.float32
        prior = np.stack([mod.prior.pi.numpy(), mod.prior.loc.numpy(), mod.prior.scale.numpy()]).astype(np.float32)
        assert np.array_equal(prior[2], R.final_scales(sigma))
        torch.manual_seed(EPS_SEED)
        kl = mod._kl
        ref_kl = float(kl.item())
        k64, dm64, dr64 = f64(mu, rho, eps, prior)
        ek, edm, edr = R.emulate32(mu, rho, eps, *prior)
        err = np.array([abs(ek - k64) / abs(k64), R.relerr(edm, dm64), R.relerr(edr, dr64)])
        rk, rdm, rdr = R.kl_mixture(mu, rho, eps, *prior)
        assert abs(rk - k64) <= 1e-12 * abs(k64) and R.relerr(rdm, dm64) < 1e-12 and R.relerr(rdr, dr64) < 1e-12, name
        res[name + "_prior"], res[name + "_kl64"], res[name + "_dmu64"], res[name + "_drho64"] = prior, np.float64(k64), dm64, dr64
        res[name + "_emu_kl"], res[name + "_emu_err"] = np.float64(ek), err
        line = "%-4s J=%d  kl64 %.9e  emulation: value %.2e, dmu %.2e, drho %.2e  reference float32: " % (name, len(pi), k64, err[0], err[1], err[2])
        if finite:
            if not np.isfinite(ref_kl):
                raise SystemExit("case %s is listed reference-finite but the reference's value is %r" % (name, ref_kl))
            kl.backward()
            dmu = np.concatenate([mod.W_mu.grad.numpy(), mod.bias_mu.grad.numpy()]).astype(np.float32)
            drho = np.concatenate([mod.W_rho.grad.numpy(), mod.bias_rho.grad.numpy()]).astype(np.float32)
            res[name + "_kl"], res[name + "_dmu"], res[name + "_drho"] = np.float32(ref_kl), dmu, drho
            line += "value %.2e, dmu %.2e, drho %.2e" % (abs(ref_kl - k64) / abs(k64), R.relerr(dmu, dm64), R.relerr(drho, dr64))
        else:
            line += "%r (restatement only)" % ref_kl
        print(line)

    # the net: same seed and construction as scripts/make_golden_kl.py, so the parameters are those of kl_forward.npz.  MeanFieldVI.kl
    # (freq_to_bayes.py:43-48) asks hasattr(layer, '_kl') before it reads layer._kl: the property runs twice per layer and the first
    # draw is thrown away, so the value comes from every SECOND draw of the generator
    pi, sigma, loc = R.PRIORS["m3"]
    torch.manual_seed(7)
    net = models.get_net(8, "skip", "reflection", skip_n33d=[8, 16], skip_n33u=[8, 16], skip_n11=4, num_scales=2, n_channels=2, upsample_mode="bilinear")
    net = MeanFieldVI(net, prior={"mu": list(loc), "sigma": np.asarray(sigma, np.float32), "pi": list(pi)}, kl_type="forward", reparam="")
    fwd = np.load(os.path.join(ROOT, "tests", "golden", "kl_forward.npz"))
    keys = [k for k in net.state_dict() if k.rsplit(".", 1)[-1] in ("W_mu", "W_rho", "bias_mu", "bias_rho")]
    assert keys == [str(k) for k in fwd["net_keys"]]
    for i, k in enumerate(keys):
        assert np.array_equal(net.state_dict()[k].numpy(), fwd["net_p%d" % i]), k
    layers = [(k, m) for k, m in net.named_modules() if isinstance(m, VIModule)]
    assert [k for k, _ in layers] == [str(k) for k in fwd["net_layers"]]
    torch.manual_seed(EPS_SEED)
    net_kl = float(net.kl().item())
    if not np.isfinite(net_kl):
        raise SystemExit("the net's reference value is %r" % net_kl)
    prior = np.stack([layers[0][1].prior.pi.numpy(), layers[0][1].prior.loc.numpy(), layers[0][1].prior.scale.numpy()]).astype(np.float32)
    torch.manual_seed(EPS_SEED)
    eps, layer_kl = [], []
    for _, m in layers:
        parts = [(m.W_mu, m.W_rho)] + ([(m.bias_mu, m.bias_rho)] if m.bias_mu is not None else [])
        [torch.empty(a.shape).normal_() for a, _ in parts]                       # the draw of hasattr
        e = np.concatenate([torch.empty(a.shape).normal_().numpy().ravel() for a, _ in parts])
        mu = np.concatenate([a.detach().numpy().ravel() for a, _ in parts]); rho = np.concatenate([b.detach().numpy().ravel() for _, b in parts])
        eps.append(e); layer_kl.append(f64(mu, rho, e, prior)[0])
    tot = float(np.sum(layer_kl))
    res["net_prior"], res["net_eps"] = prior, np.concatenate(eps).astype(np.float32)
    res["net_layer_kl64"], res["net_kl"], res["net_kl64"] = np.asarray(layer_kl, np.float64), np.float32(net_kl), np.float64(tot)
    print("net: %d VI layers, %d weights, kl %.9e (reference float32 against float64: %.2e)" % (len(layers), res["net_eps"].size, tot, abs(net_kl - tot) / abs(tot)))
    assert abs(net_kl - tot) < 1e-6 * abs(tot)
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 400 * 1024


if __name__ == "__main__":
    main()
