"""Writes tests/golden/prune_ffg.npz: the reference's global SNR pruning, evaluated by its own MeanFieldVI(net, reparam='') and
prune_weights_ffg(net, 'percentage', amount=a) (BayTorch/inference/utils.py:104-166) in float32 on the CPU, loaded from a checkout at
generation time (stub modules as in scripts/make_golden_kl.py), a fresh net per amount.

usage:  PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python scripts/make_golden_prune.py <reference checkout> [out.npz]

The net is the two-scale net of tests/test_gpu_dropin.py (every layer has a bias: the reference crashes on a layer without one).  The seed
is the first from SEED0 on at which, for every amount and both groups (all W, all biases), the float64 SNRs of the k-th and the (k+1)-th
smallest element differ by more than 1e-4 relative: a last-ulp difference between two float32 softplus implementations (about 1e-7) then
cannot move an element across the threshold, and the expected result is exact mask equality.

keys:
  seed, amounts          the seed found, float64 [3]
  layers                 names of the Bayesian layers in module order
  mu<i>, rho<i>          float32, flat: layer i's W | bias (the seeded parameters, the same for every amount)
  snr64_<i>              float64 |mu| / softplus(rho) of the same elements
  a<j>_W<i>, a<j>_b<i>   uint8, flat: the reference's W_mu_mask / bias_mu_mask of layer i after pruning with amounts[j]
  a<j>_k                 int64 [2]: int(amount * n) per group"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMOUNTS = (0.1, 0.5, 0.9)
SEED0, MIN_GAP = 7, 1e-4


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "prune_ffg.npz")
    sys.dont_write_bytecode = True
    os.environ.setdefault("MPLBACKEND", "Agg")
    for m in ("torchvision", "torchvision.transforms", "skimage", "skimage.metrics"):
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.modules["skimage.metrics"].peak_signal_noise_ratio = None
    sys.path.insert(0, ref)
    import warnings
    import torch
    from BayTorch.freq_to_bayes import MeanFieldVI
    from BayTorch.modules.module import VIModule
    from BayTorch.inference.utils import prune_weights_ffg
    import models
    warnings.filterwarnings("ignore")

    def make(seed):
        torch.manual_seed(seed)
        net = models.get_net(8, "skip", "reflection", skip_n33d=[8, 16], skip_n33u=[8, 16], skip_n11=4, num_scales=2, n_channels=2, upsample_mode="bilinear")
        net = MeanFieldVI(net, reparam="")
        return net, [(k, m) for k, m in net.named_modules() if isinstance(m, VIModule)]

    def snr64(layers):
        w, b = [], []
        for _, m in layers:
            for dst, mu, rho in ((w, m.W_mu, m.W_rho), (b, m.bias_mu, m.bias_rho)):
                r = rho.detach().double()
                dst.append((mu.detach().double().abs() / torch.nn.functional.softplus(r)).numpy().ravel())
        return w, b

    def gaps_ok(layers):
        for group in snr64(layers):
            s = np.sort(np.concatenate(group))
            for a in AMOUNTS:
                k = int(a * s.size)
                if 0 < k < s.size and not (s[k] - s[k - 1]) > MIN_GAP * s[k]:
                    return False
        return True

    seed = SEED0
    while True:
        net, layers = make(seed)
        assert all(m.bias_mu is not None for _, m in layers)
        if gaps_ok(layers):
            break
        seed += 1
        if seed > SEED0 + 500:
            raise SystemExit("no seed with separated thresholds")
    res = dict(seed=np.int64(seed), amounts=np.asarray(AMOUNTS, np.float64), layers=np.array([k for k, _ in layers]))
    w64, b64 = snr64(layers)
    for i, (_, m) in enumerate(layers):
        res["mu%d" % i] = np.concatenate([m.W_mu.detach().numpy().ravel(), m.bias_mu.detach().numpy().ravel()]).astype(np.float32)
        res["rho%d" % i] = np.concatenate([m.W_rho.detach().numpy().ravel(), m.bias_rho.detach().numpy().ravel()]).astype(np.float32)
        res["snr64_%d" % i] = np.concatenate([w64[i], b64[i]])
    n = [sum(x.size for x in w64), sum(x.size for x in b64)]
    for j, a in enumerate(AMOUNTS):
        net, layers = make(seed)                                       # a fresh net per amount: the reference's second pass takes log(0)
        for i, (_, m) in enumerate(layers):
            assert np.array_equal(res["mu%d" % i][:m.W_mu.numel()], m.W_mu.detach().numpy().ravel())
        prune_weights_ffg(net, "percentage", amount=a)
        ks = [int(a * x) for x in n]
        got = [0, 0]
        for i, (_, m) in enumerate(layers):
            wm, bm = m.W_mu_mask.numpy().ravel(), m.bias_mu_mask.numpy().ravel()
            assert set(np.unique(wm)) <= {0.0, 1.0} and np.array_equal(wm, m.W_rho_mask.numpy().ravel()) and np.array_equal(bm, m.bias_rho_mask.numpy().ravel())
            res["a%d_W%d" % (j, i)], res["a%d_b%d" % (j, i)] = wm.astype(np.uint8), bm.astype(np.uint8)
            got[0] += int((wm == 0).sum()); got[1] += int((bm == 0).sum())
        assert got == ks, (a, got, ks)
        res["a%d_k" % j] = np.asarray(ks, np.int64)
        # the masks are those of a stable argsort of the float32 SNR, per group
        for g, key in ((0, "W"), (1, "b")):
            mu = np.concatenate([(res["mu%d" % i][:m.W_mu.numel()] if g == 0 else res["mu%d" % i][m.W_mu.numel():]) for i, (_, m) in enumerate(layers)])
            rho = np.concatenate([(res["rho%d" % i][:m.W_mu.numel()] if g == 0 else res["rho%d" % i][m.W_mu.numel():]) for i, (_, m) in enumerate(layers)])
            snr = (torch.from_numpy(mu).abs() / torch.nn.functional.softplus(torch.from_numpy(rho))).numpy()
            want = np.ones(snr.size, np.uint8)
            want[np.argsort(snr, kind="stable")[:ks[g]]] = 0
            assert np.array_equal(want, np.concatenate([res["a%d_%s%d" % (j, key, i)] for i in range(len(layers))])), (a, key)
        print("amount %.1f: pruned %d of %d weights, %d of %d biases" % (a, got[0], n[0], got[1], n[1]))
    np.savez_compressed(out, **res)                                    # data only: plain arrays, loadable with allow_pickle=False
    np.load(out, allow_pickle=False)["layers"]
    print("seed %d; wrote %s, %d bytes" % (seed, out, os.path.getsize(out)))
    assert os.path.getsize(out) <= 400 * 1024


if __name__ == "__main__":
    main()
