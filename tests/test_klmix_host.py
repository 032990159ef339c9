"""The scale-mixture prior without a GPU: check_prior_mixture, the layout of mfvi_mixture_prior, the float64 restatement
against the golden file written from the reference (scripts/make_golden_klmix.py), and the statement's own identities."""
import ctypes
import os
import re

import numpy as np
import pytest

import klmix_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "kl_mixture.npz"), allow_pickle=False)


def _inputs(gold, name):
    return gold["mu"], gold["rho_lo" if R.CASES[name][3] == 1.5 else "rho_hi"], gold["eps"]


def test_check_prior_mixture_accepts_and_refuses():
    from mfvi_dip_mia_amd.rowbatch import check_prior_mixture
    assert check_prior_mixture(None) is None
    pm = check_prior_mixture({"pi": [0.5, 0.5], "sigma": np.array([1.0, 0.0025])})
    assert pm["mu"] == [0.0, 0.0] and pm["pi"] == [0.5, 0.5] and pm["sigma"] == [1.0, 0.0025]
    assert pm["scale"] == [float(np.float32(1.0 + 1e-6)), float(np.float32(0.0025 + 1e-6))]      # module.py:34, rounded to float32
    pm = check_prior_mixture({"pi": (1.0,), "sigma": (0.0,), "mu": (0.25,)})                     # sigma 0 is the scale 1e-6
    assert pm["scale"] == [float(np.float32(1e-6))] and pm["mu"] == [0.25]
    assert len(check_prior_mixture({"pi": [.3, .3, .2, .2], "sigma": [1, .1, .01, 3], "mu": [0, 0, .5, -.5]})["pi"]) == 4
    assert check_prior_mixture({"pi": [2.0, 3.0], "sigma": [1.0, 2.0]})["pi"] == [2.0, 3.0]      # the pi are used as given, not normalised
    torch = pytest.importorskip("torch")
    assert check_prior_mixture({"pi": torch.tensor([.5, .5]), "sigma": torch.tensor([1.0, 0.1])})["sigma"] == [1.0, float(np.float32(0.1))]
    for bad in ({"pi": [], "sigma": []}, {"pi": [.2] * 5, "sigma": [1.0] * 5}, {"pi": [.5, .5], "sigma": [1.0]}, {"pi": [.5, .5], "sigma": [1.0, 1.0], "mu": [0.0]},
                {"pi": 0.5, "sigma": [1.0]}, {"pi": [0.5], "sigma": 1.0}, {"pi": [0.5], "sigma": [1.0], "mu": 0.0}, {"sigma": [1.0]}, {"pi": [1.0]},
                {"pi": [1.0], "sigma": [1.0], "weights": [1.0]}, [0.5, 1.0], "mixture",
                {"pi": [0.0, 1.0], "sigma": [1.0, 1.0]}, {"pi": [-0.5, 1.5], "sigma": [1.0, 1.0]}, {"pi": [float("nan")], "sigma": [1.0]}, {"pi": [float("inf")], "sigma": [1.0]},
                {"pi": [1.0], "sigma": [-1.0]}, {"pi": [1.0], "sigma": [-1e-6]}, {"pi": [1.0], "sigma": [float("inf")]}, {"pi": [1.0], "sigma": [float("nan")]},
                {"pi": [1.0], "sigma": [1e20]}, {"pi": [1.0], "sigma": [1.0], "mu": [float("inf")]}, {"pi": [1.0], "sigma": [1.0], "mu": [float("nan")]},
                {"pi": [1e-50], "sigma": [1.0]}, {"pi": ["a"], "sigma": [1.0]}):
        with pytest.raises(ValueError):
            check_prior_mixture(bad)


def test_struct_layout_is_the_headers():
    from mfvi_dip_mia_amd import _lib as L
    from mfvi_dip_mia_amd.rowbatch import check_prior_mixture, mixture_struct
    S = L.MixturePrior
    assert ctypes.sizeof(S) == 52 and L.MIXTURE_MAX == 4
    assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == [("n", 0, 4), ("pi", 4, 16), ("mu", 20, 16), ("sigma", 36, 16)]
    text = open(os.path.join(ROOT, "include", "mfvi_hip.h")).read()
    assert re.search(r"#define MFVI_MIXTURE_MAX 4\b", text)
    assert re.search(r"typedef struct \{ int32_t n; float pi\[MFVI_MIXTURE_MAX\], mu\[MFVI_MIXTURE_MAX\], sigma\[MFVI_MIXTURE_MAX\]; \} mfvi_mixture_prior;", text)
    assert re.search(r"DOMAIN_KLMC = 8\b", open(os.path.join(ROOT, "mfvi-dip-mia_amd", "csrc", "common.h")).read()) and L.DOMAIN_KLMC == 8
    for name in ("mfvi_kl_mixture", "mfvi_kl_mixture_backward", "mfvi_elbo_update_mixture", "mfvi_elbo_update_guarded_mixture", "mfvi_elbo_update_fits_mixture"):
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == len(L.SIGNATURES[name][1]), name
    s = mixture_struct(check_prior_mixture({"pi": [.75, .25], "sigma": [0.8, 0.01], "mu": [0.25, 0.0]}))
    assert s.n == 2 and list(s.pi) == [0.75, 0.25, 0.0, 0.0] and list(s.mu) == [0.25, 0.0, 0.0, 0.0]
    assert list(s.sigma)[:2] == [float(np.float32(0.8 + 1e-6)), float(np.float32(0.01 + 1e-6))]
    z = mixture_struct(None)
    assert z.n == 0 and bytes(z) == bytes(52)


def test_restatement_against_the_golden(gold):
    assert set(R.REFERENCE_FINITE) == {"m1", "m2", "m3", "m4", "m5"} and len(R.CASES) == 12
    for name, (pi, sigma, loc, _, finite) in R.CASES.items():
        mu, rho, eps = _inputs(gold, name)
        assert mu.size == R.N_W + R.N_B
        prior = gold[name + "_prior"]
        assert np.array_equal(prior[0], np.asarray(pi, np.float32)) and np.array_equal(prior[1], np.asarray(loc, np.float32))
        assert np.array_equal(prior[2], R.final_scales(sigma))
        v, dm, dr = R.kl_mixture(mu, rho, eps, *prior)
        assert abs(v - float(gold[name + "_kl64"])) <= 1e-12 * abs(float(gold[name + "_kl64"])), name
        assert R.relerr(dm, gold[name + "_dmu64"]) < 1e-12 and R.relerr(dr, gold[name + "_drho64"]) < 1e-12, name
        # the emulation is what the file says it is, and is within the value tolerance of float64
        ev, edm, edr = R.emulate32(mu, rho, eps, *prior)
        assert ev == float(gold[name + "_emu_kl"]) and abs(ev - v) < 1e-6 * abs(v), name
        err = gold[name + "_emu_err"]
        assert np.allclose([R.relerr(edm, dm), R.relerr(edr, dr)], err[1:], rtol=1e-6, atol=0), name
        assert R.grad_bound(gold, name, "dmu") == max(1e-5, 4 * err[1]) and R.grad_bound(gold, name, "drho") == max(1e-5, 4 * err[2])
        assert (name + "_kl" in gold.files) == finite
        if finite:      # the reference's own float32 value is a witness of the value (its gradients are recorded, not compared)
            assert np.isfinite(gold[name + "_kl"]) and abs(float(gold[name + "_kl"]) - v) < 1e-6 * abs(v), name
    assert np.array_equal(gold["rho_lo"][300:], gold["rho_hi"][300:]) and gold["rho_hi"][:300].max() == 6.0 and gold["rho_lo"][:300].min() == -12.0


def test_one_component_is_two_equal_halves(gold):
    mu, rho, eps = _inputs(gold, "m4")
    one = R.kl_mixture(mu, rho, eps, [1.0], [0.1], [0.7])
    two = R.kl_mixture(mu, rho, eps, [0.5, 0.5], [0.1, 0.1], [0.7, 0.7])
    assert abs(one[0] - two[0]) <= 1e-13 * abs(one[0]) and R.relerr(two[1], one[1]) < 1e-13 and R.relerr(two[2], one[2]) < 1e-13
    e1 = R.emulate32(mu, rho, eps, [1.0], [0.1], [0.7]); e2 = R.emulate32(mu, rho, eps, [0.5, 0.5], [0.1, 0.1], [0.7, 0.7])
    assert abs(e1[0] - e2[0]) <= 1e-6 * abs(e1[0]) and R.relerr(e2[1], e1[1]) < 1e-6 and R.relerr(e2[2], e1[2]) < 1e-6
    # J = 1 is a Gaussian prior: the expectation of the term over eps is the forward KL; one draw per weight scatters around it
    import kl_restatement as K
    rng = np.random.default_rng(5)
    draws = np.mean([R.kl_mixture(mu, rho, rng.standard_normal(mu.size), [1.0], [0.1], [0.7])[0] for _ in range(200)])
    exact = K.kl_forward(mu, rho, 0.1, 0.7)[0]
    assert abs(draws - exact) < 0.01 * abs(exact)


def test_restatement_stays_finite_where_a_literal_sum_underflows(gold):
    mu, rho, eps = _inputs(gold, "n2")
    prior = gold["n2_prior"]
    v, dm, dr = R.kl_mixture(mu, rho, eps, *prior)
    assert np.isfinite(v) and np.isfinite(dm).all() and np.isfinite(dr).all()
    ev, edm, edr = R.emulate32(mu, rho, eps, *prior)
    assert np.isfinite(ev) and np.isfinite(edm).all() and np.isfinite(edr).all()
    w = mu.astype(np.float64) + K_softplus(rho) * eps
    with np.errstate(divide="ignore"):
        literal = np.log(sum(p * np.exp(-0.5 * ((w - m) / s) ** 2, dtype=np.float32) for p, m, s in zip(*prior.astype(np.float64))))
    assert np.isinf(literal).any()


def K_softplus(rho):
    return R.softplus(rho)
