"""Float64 numpy restatement of the two directions of the KL term between the mean-field posterior N(mu, softplus(rho)^2) and the prior
N(m0, s0^2), per (mu, rho) pair, with both derivatives (BayTorch/modules/module.py:64-80 evaluates torch's kl_divergence of two Normals):

    reverse  ('reverse', the reference's default)  KL(prior || posterior) = log(s / s0) + (s0^2 + d^2) / (2 s^2) - 1/2
    forward  (any other kl_type)                   KL(posterior || prior) = log(s0 / s) + (s^2 + d^2) / (2 s0^2) - 1/2

with s = softplus(rho), d = mu - m0.  The tests of the forward direction compare the kernels, and the golden file
tests/golden/kl_forward.npz written from the reference itself, against these."""
import numpy as np


def softplus(rho):
    rho = np.asarray(rho, np.float64)
    return np.where(rho > 20.0, rho, np.log1p(np.exp(np.minimum(rho, 20.0))))      # torch's softplus (threshold 20)


def sigmoid(rho):
    return 1.0 / (1.0 + np.exp(-np.asarray(rho, np.float64)))


def kl_forward(mu, rho, m0, s0):
    """-> (sum of the terms, d/dmu [n], d/drho [n]), everything float64."""
    mu, rho, m0, s0 = np.asarray(mu, np.float64), np.asarray(rho, np.float64), float(m0), float(s0)
    s, d = softplus(rho), mu - m0
    terms = np.log(s0) - np.log(s) + (s * s + d * d) / (2.0 * s0 * s0) - 0.5
    return float(terms.sum()), d / (s0 * s0), (s / (s0 * s0) - 1.0 / s) * sigmoid(rho)


def kl_reverse(mu, rho, m0, s0):
    """-> (sum of the terms, d/dmu [n], d/drho [n]), everything float64."""
    mu, rho, m0, s0 = np.asarray(mu, np.float64), np.asarray(rho, np.float64), float(m0), float(s0)
    s, d = softplus(rho), mu - m0
    terms = np.log(s) - np.log(s0) + (s0 * s0 + d * d) / (2.0 * s * s) - 0.5
    return float(terms.sum()), d / (s * s), (1.0 / s - (s0 * s0 + d * d) / (s * s * s)) * sigmoid(rho)


KL = {"forward": kl_forward, "reverse": kl_reverse}


def relerr(a, b):
    """max |a - b| relative to the largest |b| (the measure of tests/test_gpu_parity.py)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# the layer cases of tests/golden/kl_forward.npz (scripts/make_golden_kl.py): name -> (prior sigma, prior mu, kl_type handed to the reference)
N_W, N_B = 1031, 7      # weight and bias size of every layer case: no multiple of 4 or 256
DEN_SIGMA = float(np.sqrt(5.656911698337764e-07) * 1.4616642493692077e-05)      # the den config's sqrt(temp) * sigma: scale ~ 1.011e-6
LAYER_CASES = {"c1": (0.1, 0.0, "forward"), "c2": (DEN_SIGMA, 0.0, "forward"), "c3": (0.05, 0.25, "forward"), "c4": (0.1, 0.0, "forward"),
               "c5": (0.1, 0.0, "fwd")}
# the file stores every distinct input once: the case whose <case>_mu / <case>_rho a case reads (c2 and c5 differ from c1 in the prior and
# the kl_type string only; c4 draws its own rho, with both softplus tails)
INPUTS = {"c1": ("c1", "c1"), "c2": ("c1", "c1"), "c3": ("c3", "c3"), "c4": ("c1", "c4"), "c5": ("c1", "c1")}


def case_inputs(gold, name):
    """(mu, rho) float32 [N_W + N_B] of a layer case from the loaded golden file."""
    m, r = INPUTS[name]
    return gold[m + "_mu"], gold[r + "_rho"]
