"""Float64 numpy restatement of the Monte-Carlo KL term between the mean-field posterior N(mu, softplus(rho)^2) and a scale-mixture prior
sum_j pi_j N(m_j, sigma_j^2), per (mu, rho, eps) triple with both derivatives.  The reference evaluates, with
kl_type != 'reverse', mc_kl_divergence(posterior, mixture) (BayTorch/distributions/distributions.py:30-35) at ONE draw w = mu + s eps:

    term = log N(w; mu, s) - log sum_j pi_j N(w; m_j, sigma_j)
         = (-eps^2 / 2 - log s) - L,      L = logsumexp_j a_j,      a_j = log pi_j - log sigma_j - (w - m_j)^2 / (2 sigma_j^2)
    d term / d mu = G,      d term / d rho = (G eps - 1 / s) sigmoid(rho),      G = sum_j r_j (w - m_j) / sigma_j^2,      r_j = exp(a_j - L)

(the two 1/2 log 2 pi cancel; the pi are used as given).  emulate32 is the same statement in float32 numpy, operation by operation as the
kernels round it: its distance from float64 is what the gradient bounds of tests/test_gpu_klmix.py are derived from."""
import numpy as np

from kl_restatement import relerr, sigmoid, softplus      # noqa: F401 (relerr is used by the tests through this module)


def kl_mixture(mu, rho, eps, pi, m, sigma):
    """-> (sum of the terms, d/dmu [n], d/drho [n]), everything float64; sigma: the final scales."""
    mu, rho, eps = (np.asarray(x, np.float64) for x in (mu, rho, eps))
    pi, m, sigma = (np.asarray(x, np.float64).reshape(-1, 1) for x in (pi, m, sigma))
    s = softplus(rho)
    w = mu + s * eps
    d = w[None, :] - m
    a = np.log(pi) - np.log(sigma) - d * d / (2.0 * sigma * sigma)
    mx = a.max(axis=0)
    e = np.exp(a - mx)
    se = e.sum(axis=0)
    L = mx + np.log(se)
    G = (e * d / (sigma * sigma)).sum(axis=0) / se
    terms = (-0.5 * eps * eps - np.log(s)) - L
    return float(terms.sum()), G, (G * eps - 1.0 / s) * sigmoid(rho)


def emulate32(mu, rho, eps, pi, m, sigma):
    """The statement in float32, every operation rounded on its own (kl_mixture_terms, csrc/iter_ops.h); the terms added in float64."""
    f = np.float32
    mu, rho, eps = (np.asarray(x, f) for x in (mu, rho, eps))
    pi, m, sigma = (np.asarray(x, f) for x in (pi, m, sigma))
    with np.errstate(over="ignore"):
        s = np.where(rho > f(20), rho, np.log1p(np.exp(rho))).astype(f)
    w = mu + s * eps
    c = np.log(pi) - np.log(sigma)
    iv = f(1) / (sigma * sigma)
    d = [w - m[j] for j in range(len(pi))]
    a = [c[j] - (d[j] * d[j]) * (f(0.5) * iv[j]) for j in range(len(pi))]
    mx = np.maximum.reduce(a)
    se, ge = np.zeros_like(w), np.zeros_like(w)
    for j in range(len(pi)):
        e = np.exp(a[j] - mx)
        se = se + e
        ge = ge + e * (d[j] * iv[j])
    G = ge / se
    L = mx + np.log(se)
    sg = f(1) / (f(1) + np.exp(-rho))
    terms = (f(-0.5) * (eps * eps) - np.log(s)).astype(np.float64) - L.astype(np.float64)
    assert G.dtype == f and L.dtype == f and s.dtype == f
    return float(terms.sum()), G, (G * eps - f(1) / s) * sg


# the layer cases of tests/golden/kl_mixture.npz (scripts/make_golden_klmix.py): name -> (pi, sigma as handed to the reference, component means,
# the largest rho of the linspace head, whether the reference's own float32 value is finite and recorded)
N_W, N_B = 1031, 7      # weight and bias size of every layer case: no multiple of 4 or 256
PRIORS = {
    "m1": ((.5, .5), (1.0, 0.0025), (0.0, 0.0)),
    "m2": ((.75, .25), (0.8, 0.01), (0.25, 0.0)),
    "m3": ((.2, .5, .3), (0.5, 0.05, 2.0), (0.0, .1, -.1)),
    "m4": ((1.0,), (1.0,), (0.0,)),
    "m5": ((.3, .3, .2, .2), (1.0, .1, .01, 3.0), (0.0, 0.0, .5, -.5)),
}
CASES = {name: (pi, sg, m, 1.5, True) for name, (pi, sg, m) in PRIORS.items()}
CASES.update({name + "w": (pi, sg, m, 6.0, False) for name, (pi, sg, m) in PRIORS.items()})      # the same priors with rho up to 6
CASES["n1"] = ((.5, .5), (1e-3, 1e-5), (0.0, 0.0), 1.5, False)
CASES["n2"] = ((.5, .5), (1.011e-6, 1e-4), (0.0, 0.0), 1.5, False)                                # the runners' scale
REFERENCE_FINITE = [c for c, v in CASES.items() if v[4]]


def final_scales(sigma):
    """prior['sigma'] + 1e-6 as a float32 tensor (BayTorch/modules/module.py:34)."""
    return (np.asarray(sigma, np.float32) + np.float32(1e-6)).astype(np.float32)


def case_rho(rng, n, rho_hi):
    """rho ~ N(-3, 0.1) with the first 300 entries linspace(-12, rho_hi)."""
    rho = (-3.0 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    rho[:300] = np.linspace(-12.0, rho_hi, 300).astype(np.float32)
    return rho


def grad_bound(gold, name, which):
    """The gradient bound of a case (relative to the largest entry of the float64 gradient): max(1e-5, 4 x the recorded error of the float32
    numpy emulation); the factor 4 covers the device's expf / logf, a few ulp looser than numpy's."""
    return max(1e-5, 4.0 * float(gold["%s_emu_err" % name][{"dmu": 1, "drho": 2}[which]]))
