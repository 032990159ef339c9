"""The cases behind tests/golden/kl_update_bits.npz: every entry point that forms a KL term, on seeded host inputs, at
the smallest shapes that take each way its loops can go.  record(M) runs them on whatever library the package loaded and returns

  digests   name -> sha256 of the raw bytes of one output array      (every fused update, every unfused gradient)
  exact     name -> float64, held bitwise                            (unfused sums of ONE block: no atomic ordering involved)
  close     name -> float64, held to CLOSE_RTOL                      (unfused sums of several blocks: they end in a double atomicAdd across
                                                                       blocks, so their last bits may depend on block arrival order)

scripts/make_golden_klbits.py writes the three tables, tests/test_gpu_kl_bits.py compares a fresh record() with them.  Inputs come from
numpy.random.default_rng(SEED) in a fixed order of draws: adding a case at the end leaves the earlier ones as they are."""
import ctypes
import hashlib

import numpy as np

SEED = 20261021
REV, FWD = 0, 1
CLOSE_RTOL = 1e-10                      # the bound of the unfused-vs-fused checks of tests/test_gpu_kl.py
B1, B2, EPS, LR, TEMP = 0.9, 0.999, 1e-8, 1e-3, 1e-3
M0, S0 = 0.05, 0.3
MIX = dict(pi=(0.5, 0.5), mu=(0.0, 0.1), sigma=(1.0, 0.0025))      # J = 2, spike and slab
KEY = dict(seed=77, sample=1, step=4)
# (n_vi, n_bn): five blocks, a tail that is no multiple of 4, BN shorter than VI / the grid sized by the BN block, one partial quad
SMALL = [(1027, 37), (3, 300)]
# the grid cap (2048 blocks) and a second trip of the grid-stride loop
BIG = (2048 * 256 + 259, 0)
N_GRAD, I0, N_ONE_BLOCK = 1027, 5, 200


def _sha(t):
    a = t.detach().cpu()
    if a.dtype.is_floating_point and a.element_size() == 2:
        a = a.view(__import__("torch").int16)
    return hashlib.sha256(np.ascontiguousarray(a.numpy()).tobytes()).digest()


def _block(rng, n_vi, n_bn, rows=1):
    """params [MU | RHO | BN], grads, m, v of `rows` fits, float32 on the host."""
    n = 2 * n_vi + n_bn
    p = np.concatenate([rng.normal(0.0, 0.1, (rows, n_vi)), rng.normal(-3.0, 0.5, (rows, n_vi)), rng.normal(1.0, 0.1, (rows, n_bn))], axis=1)
    g = rng.normal(0.0, 1e-2, (rows, n))
    m = rng.normal(0.0, 1e-3, (rows, n))
    v = np.abs(rng.normal(0.0, 1e-6, (rows, n)))
    return [np.ascontiguousarray(a, np.float32) for a in (p, g, m, v)]


def _mixture(L, spec=MIX, n=None):
    s = L.MixturePrior()
    s.n = len(spec["pi"]) if n is None else n
    for j in range(len(spec["pi"])):
        s.pi[j], s.mu[j], s.sigma[j] = spec["pi"][j], spec["mu"][j], spec["sigma"][j]
    return s


def record(M):
    import torch
    L = M._lib
    lib, sp = L.lib(), L.stream_ptr()
    rng = np.random.default_rng(SEED)
    digests, exact, close = {}, {}, {}
    dev = lambda a: torch.from_numpy(a).cuda()
    mix = _mixture(L)
    key = (KEY["seed"], KEY["sample"], KEY["step"], None)

    def put(case, **arrays):
        for k, t in arrays.items():
            digests[case + "/" + k] = _sha(t)

    # ---- single-fit fused updates: host t and guarded (device counter 2; a finite and a NaN data term), float32 and bf16
    def single(case, host, n_vi, n_bn, call, guarded=None):
        p, g, m, v = (dev(a[0]) for a in host)
        kl = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
        scratch = torch.zeros(lib.mfvi_elbo_update_scratch_bytes(), dtype=torch.uint8, device="cuda")
        out = dict(params=p, grads=g, m=m, v=v, kl=kl)
        if guarded is None:
            step = (3,)                                                   # update number t from the host
        else:
            out["t_applied"] = torch.full((1,), 2, dtype=torch.int32, device="cuda")
            loss = torch.full((1,), guarded, dtype=torch.float64, device="cuda")
            step = (L.ptr(out["t_applied"]), L.ptr(loss), None)           # t_applied, loss_d, loss_f
        L.check(call((L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n_vi, n_bn), step, (L.ptr(kl), L.ptr(scratch), sp)))
        torch.cuda.synchronize()
        put(case, **out)

    hyper = (LR, B1, B2, EPS)
    gauss = (M0, S0, TEMP)
    # per prior: the entry with t from the host, the guarded entry; a = the block, s = the step source, z = (kl_out, scratch, stream)
    priors = {
        "rev": (lambda a, s, z: lib.mfvi_elbo_update(*a, *gauss, *hyper, *s, *z),
                lambda a, s, z: lib.mfvi_elbo_update_guarded(*a, *gauss, *hyper, *s, *z)),
        "typed_rev": (lambda a, s, z: lib.mfvi_elbo_update_typed(*a, *gauss, REV, *hyper, *s, *z),
                      lambda a, s, z: lib.mfvi_elbo_update_guarded_typed(*a, *gauss, REV, *hyper, *s, *z)),
        "fwd": (lambda a, s, z: lib.mfvi_elbo_update_typed(*a, *gauss, FWD, *hyper, *s, *z),
                lambda a, s, z: lib.mfvi_elbo_update_guarded_typed(*a, *gauss, FWD, *hyper, *s, *z)),
        "mix": (lambda a, s, z: lib.mfvi_elbo_update_mixture(*a, ctypes.byref(mix), TEMP, *hyper, *s, *key, *z),
                lambda a, s, z: lib.mfvi_elbo_update_guarded_mixture(*a, ctypes.byref(mix), TEMP, *hyper, *s, *key, *z)),
    }
    for n_vi, n_bn in SMALL:
        host = _block(rng, n_vi, n_bn)
        for name, (plain, guarded) in priors.items():
            tag = "%s/%dx%d" % (name, n_vi, n_bn)
            single("update/" + tag, host, n_vi, n_bn, plain)
            single("guarded_finite/" + tag, host, n_vi, n_bn, guarded, guarded=1.25)
            single("guarded_nan/" + tag, host, n_vi, n_bn, guarded, guarded=float("nan"))
        for name, kt in (("rev", None), ("typed_rev", REV), ("fwd", FWD)):
            p, g, m, v = (dev(a[0]) for a in host)
            mu, rho, bn = p[:n_vi].bfloat16(), p[n_vi:2 * n_vi].bfloat16(), p[2 * n_vi:].clone()
            kl = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
            scratch = torch.zeros(lib.mfvi_elbo_update_scratch_bytes(), dtype=torch.uint8, device="cuda")
            head = (L.ptr(mu), L.ptr(rho), L.ptr(bn), L.ptr(g), L.ptr(m), L.ptr(v), n_vi, n_bn, M0, S0, TEMP)
            tail = (*hyper, 3, KEY["seed"], L.ptr(kl), L.ptr(scratch), sp)
            L.check(lib.mfvi_elbo_update_bf16(*head, *tail) if kt is None else lib.mfvi_elbo_update_bf16_typed(*head, kt, *tail))
            torch.cuda.synchronize()
            put("bf16/%s/%dx%d" % (name, n_vi, n_bn), mu=mu, rho=rho, bn=bn, grads=g, m=m, v=v, kl=kl)

    # ---- per-fit fused updates: F = 3, per-row hyper-parameters, one NaN-nll row (once row 0, once row 1); typed: row 2 has direction 7;
    # mixture: row 0 a mixture, row 1 the n == 0 entry (its Gaussian prior, forward), row 2 a faulty prior (a sigma of 0)
    def fits(case, host, n_vi, n_bn, F, entry, nan_row, kl_type=None, table=None):
        p, g, m, v = (dev(a) for a in host)
        stride = 2 * n_vi + n_bn
        hyp = dev(np.array([[M0 * (f + 1), S0 * (1 + 0.5 * f), TEMP * 2 ** f, LR * (1 + f)] for f in range(F)], np.float32))
        nll = np.arange(1.0, F + 1.0)
        if nan_row is not None:
            nll[nan_row] = np.nan
        nll = dev(nll)
        dead = torch.zeros(F, dtype=torch.int32, device="cuda")
        kl = torch.full((F,), 7.0, dtype=torch.float64, device="cuda")
        scratch = torch.zeros(lib.mfvi_elbo_update_fits_scratch_bytes(F), dtype=torch.uint8, device="cuda")
        kt = None if kl_type is None else torch.tensor(kl_type, dtype=torch.int32, device="cuda")
        tab = None if table is None else torch.frombuffer(bytearray(b"".join(bytes(s) for s in table)), dtype=torch.uint8).cuda()
        head = (L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n_vi, n_bn, stride, stride, F, L.ptr(hyp))
        tail = (B1, B2, EPS, 3, L.ptr(nll), L.ptr(dead), L.ptr(kl), L.ptr(scratch), sp)
        if entry == "fits":
            L.check(lib.mfvi_elbo_update_fits(*head, *tail))
        elif entry == "typed":
            L.check(lib.mfvi_elbo_update_fits_typed(*head, L.ptr(kt), *tail))
        else:
            L.check(lib.mfvi_elbo_update_fits_mixture(*head, L.ptr(kt), L.ptr(tab), KEY["seed"], 0, KEY["step"], None, *tail))
        torch.cuda.synchronize()
        put(case, params=p, grads=g, m=m, v=v, kl=kl, dead=dead)

    faulty = _mixture(L, dict(pi=(0.5, 0.5), mu=(0.0, 0.0), sigma=(1.0, 0.0)))
    table = [mix, _mixture(L, n=0), faulty]
    for n_vi, n_bn in SMALL:
        host = _block(rng, n_vi, n_bn, rows=3)
        for nan_row in (0, 1):
            tag = "%dx%d/nan%d" % (n_vi, n_bn, nan_row)
            fits("fits/" + tag, host, n_vi, n_bn, 3, "fits", nan_row)
            fits("fits_typed/" + tag, host, n_vi, n_bn, 3, "typed", nan_row, kl_type=[FWD, REV, 7])
            fits("fits_mixture/" + tag, host, n_vi, n_bn, 3, "mixture", nan_row, kl_type=[REV, FWD, REV], table=table)
        fits("fits_mixture_nodir/%dx%d" % (n_vi, n_bn), host, n_vi, n_bn, 3, "mixture", 1, table=table)      # NULL direction table: every row reverse

    # ---- the grid cap and the second trip of the grid-stride loop (digests only)
    n_vi, n_bn = BIG
    host = _block(rng, n_vi, n_bn)
    for name in ("rev", "fwd", "mix"):
        single("update/%s/big" % name, host, n_vi, n_bn, priors[name][0])
    host = _block(rng, n_vi, n_bn, rows=2)
    fits("fits/big", host, n_vi, n_bn, 2, "fits", None)
    fits("fits_mixture/big", host, n_vi, n_bn, 2, "mixture", None, kl_type=[FWD, REV], table=[_mixture(L, n=0), mix])

    # ---- unfused gradients (added into dmu / drho) and sums
    def pair(n):
        return dev(rng.normal(0.0, 0.1, n).astype(np.float32)), dev(rng.normal(-3.0, 0.5, n).astype(np.float32))

    mu, rho = pair(N_GRAD)
    eps = dev(rng.normal(0.0, 1.0, N_GRAD).astype(np.float32))
    d0 = [rng.normal(0.0, 1e-2, N_GRAD).astype(np.float32) for _ in range(2)]
    grads = {
        "rev": lambda dm, dr: lib.mfvi_kl_backward(L.ptr(mu), L.ptr(rho), N_GRAD, M0, S0, 0.37, L.ptr(dm), L.ptr(dr), sp),
        "typed_rev": lambda dm, dr: lib.mfvi_kl_backward_typed(L.ptr(mu), L.ptr(rho), N_GRAD, M0, S0, 0.37, REV, L.ptr(dm), L.ptr(dr), sp),
        "fwd": lambda dm, dr: lib.mfvi_kl_backward_typed(L.ptr(mu), L.ptr(rho), N_GRAD, M0, S0, 0.37, FWD, L.ptr(dm), L.ptr(dr), sp),
        "mix_drawn": lambda dm, dr: lib.mfvi_kl_mixture_backward(L.ptr(mu), L.ptr(rho), N_GRAD, I0, ctypes.byref(mix), None, *key[:3], 0.37, L.ptr(dm), L.ptr(dr), sp),
        "mix_eps": lambda dm, dr: lib.mfvi_kl_mixture_backward(L.ptr(mu), L.ptr(rho), N_GRAD, I0, ctypes.byref(mix), L.ptr(eps), *key[:3], 0.37, L.ptr(dm), L.ptr(dr), sp),
    }
    for name, call in grads.items():
        dm, dr = dev(d0[0]), dev(d0[1])
        L.check(call(dm, dr))
        torch.cuda.synchronize()
        put("kl_backward/" + name, dmu=dm, drho=dr)

    def sums(table, n):
        a, b, e = mu[:n], rho[:n], eps[:n]
        out = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
        calls = {
            "rev": lambda: lib.mfvi_kl(L.ptr(a), L.ptr(b), n, M0, S0, L.ptr(out), sp),
            "typed_rev": lambda: lib.mfvi_kl_typed(L.ptr(a), L.ptr(b), n, M0, S0, REV, L.ptr(out), sp),
            "fwd": lambda: lib.mfvi_kl_typed(L.ptr(a), L.ptr(b), n, M0, S0, FWD, L.ptr(out), sp),
            "mix_drawn": lambda: lib.mfvi_kl_mixture(L.ptr(a), L.ptr(b), n, I0, ctypes.byref(mix), None, *key[:3], L.ptr(out), sp),
            "mix_eps": lambda: lib.mfvi_kl_mixture(L.ptr(a), L.ptr(b), n, I0, ctypes.byref(mix), L.ptr(e), *key[:3], L.ptr(out), sp),
        }
        for name, call in calls.items():
            L.check(call())
            table["kl/%s/%d" % (name, n)] = float(out.cpu()[0])

    sums(exact, N_ONE_BLOCK)
    sums(close, N_GRAD)
    return digests, exact, close
