"""Cases and host-side references of the odd-map tests, shared by tests/test_skip_restatement_host.py and
tests/test_gpu_oddmaps.py.  A helper, not a test module.

Every case is evaluated twice on the host: in float64 by tests/skip_restatement.py (the reference) and in fp32 by the C oracle's primitives
(tests/oracle_program.py).  The distance between the two, e32, sizes the tolerance a GPU result is held to: tol = max(4 * e32, 2e-6), never
above the tolerance test_small_nets_fwd_bwd applies to that quantity."""
import functools

import numpy as np

from oracle import oracle as O
import oracle_program
from skip_restatement import SkipNet64, relerr

OUT_TOL, LAYER_TOL, GRAD_TOL, FLOOR = 2e-5, 1e-5, 2e-4, 2e-6      # test_small_nets_fwd_bwd's tolerances; the tightest tolerance an fp32 kernel is held to
N, K0, STEP = 2, 1, 9

ONE = dict(input_depth=4, n_out=2, nd=(8,), nu=(8,), ns=(4,))
# name -> (skip_program arguments, seed).  b = the low-res branch, ceil(H/2) x ceil(W/2).  The comment names the branch of launch_concat_up_fwd
# (csrc/elementwise.hip: tiled for W % 4 == 0 && W >= 128, float4 for W % 4 == 0, else scalar) and of launch_concat_up_bwd (tile 16x64 for
# b.W >= 48, 32x32 for b.W >= 24, else 16x16; float2 pairs for an even W, else element loads) that the case reaches.  The seed is the first from
# 77 on at which the case is well conditioned with room to spare (conditioning() below; the host test holds every case to KINK / OFF_CENTRE).
CONCAT_CASES = {
    "9x12": (dict(H=9, W=12, **ONE), 77),            # b 5x6: float4 forward, last row cropped; 16x16 tile, pairs
    "35x48": (dict(H=35, W=48, **ONE), 84),          # b 18x24: float4 forward, row crop; 32x32 tile, pairs
    "27x51": (dict(H=27, W=51, **ONE), 84),          # b 14x26: scalar forward, row + column crop; 32x32 tile, element loads (ok == 2 / single)
    "67x52": (dict(H=67, W=52, **ONE), 93),          # b 34x26: float4 forward, row crop; 32x32 tile, two tile rows (32 + 2), pairs
    "21x99": (dict(H=21, W=99, **ONE), 77),          # b 11x50: scalar forward, row + column crop; 16x64 tile, element loads
    "35x132": (dict(H=35, W=132, **ONE), 108),        # b 18x66: tiled forward, tiles 64 + 2 wide and 8 + 8 + 2 high, row crop; 16x64 tiles 64 + 2 and 16 + 2, pairs
    "34x130": (dict(H=34, W=130, **ONE), 117),        # b 17x65: scalar forward (W % 4 == 2), no crop; 16x64 tile, pairs, last tile one column wide
    "20x136": (dict(H=20, W=136, **ONE), 81),        # b 10x68: tiled forward, ragged tiles (64 + 4, 8 + 2), no crop; 16x64 tile
    # mode='nearest' through the same three forward kernels and three backward tiles
    "9x12_nearest": (dict(H=9, W=12, upsample_mode="nearest", **ONE), 77),
    "21x99_nearest": (dict(H=21, W=99, upsample_mode="nearest", **ONE), 83),
    "35x132_nearest": (dict(H=35, W=132, upsample_mode="nearest", **ONE), 117),
    # no skip branch (has_a = 0): a plain up-sampling, no Concat and so no crop
    "10x12_noskip": (dict(H=10, W=12, **dict(ONE, ns=(0,))), 77),        # b 5x6: float4 forward; 16x16 tile
    "22x100_noskip": (dict(H=22, W=100, **dict(ONE, ns=(0,))), 77),      # b 11x50: float4 forward; 16x64 tile
    "36x132_noskip": (dict(H=36, W=132, **dict(ONE, ns=(0,))), 93),      # b 18x66: tiled forward; 16x64 tiles 64 + 2 and 16 + 2
}

# cin, cout, k, stride, H, W: odd maps on the matrix-core path (forward_mfma / backward_data_mfma, csrc/conv_dispatch.hip)
CONV_CASES = [
    (16, 8, 3, 2, 9, 12),        # stride-2 forward with 9 rows; Wo = 6: zero-stuffed backward-data
    (16, 8, 3, 2, 9, 16),        # Wo = 8: phase-decomposed backward-data, row phases of 5 and 4 rows
    (16, 8, 3, 2, 9, 15),        # W = 4j + 3: the forward falls to the generic kernel (W % 4 != 0), backward-data stays on the phase kernel (Wo = 8)
    (16, 8, 3, 2, 35, 48),       # several tiles, Wo = 24: phase
    (16, 8, 3, 2, 35, 44),       # Wo = 22: zero-stuffed
    (16, 16, 5, 2, 9, 12),       # 5x5 stride 2, Wo = 6
    (16, 16, 5, 2, 21, 28),      # 5x5 stride 2, Wo = 14, several row tiles
    (16, 16, 3, 1, 9, 12),       # 3x3 stride 1: rows 1 and H - 2 = 7 take the reflected taps
    (36, 16, 3, 1, 35, 48),      # 36 = 2 * 16 + 4 input channels, several tiles, last tile row ragged
    (16, 16, 5, 1, 9, 12),       # 5x5 stride 1
    (16, 4, 1, 1, 9, 12),        # 1x1
]


def params(P, seed):
    """mu ~ N(0, 0.1^2), rho ~ N(-3, 0.1^2), BN gamma = 1 + 0.1 g, beta = 0.1 g: test_gpu_parity._net_params from the program's own layout."""
    mu = (0.1 * O.normal_fill(seed, 2, 0, 0, 0, P.n_vi)).astype(np.float32)
    rho = (-3.0 + 0.1 * O.normal_fill(seed, 2, 1, 0, 0, P.n_vi)).astype(np.float32)
    g = O.normal_fill(seed, 2, 7, 0, 0, P.n_bn); bnp = np.zeros(P.n_bn, np.float32)
    for b in P.bns:
        c, off = b["C"], b["off"]
        bnp[off:off + c] = 1.0 + 0.1 * g[off:off + c]; bnp[off + c:off + 2 * c] = 0.1 * g[off + c:off + 2 * c]
    return mu, rho, bnp


def net_inputs(kw, seed, P, n=N, centred=False):
    """Parameters, net input and output gradients of n samples.  z is test_small_nets_fwd_bwd's 0.1 * U[0, 1), or, centred, N(0, 1): the 1x1 and
    3x3 convolutions of an all-positive input give channels whose mean is tens of standard deviations (see conditioning())."""
    mu, rho, bnp = params(P, seed)
    nz = kw["input_depth"] * kw["H"] * kw["W"]
    z = (O.normal_fill(seed, 2, 2, 0, 0, nz) if centred else 0.1 * O.uniform_fill(seed, 0, 0, 0, nz)).reshape(kw["input_depth"], kw["H"], kw["W"])
    oh, ow = P.tensors[len(P.tensors) - 1]["H"], P.tensors[len(P.tensors) - 1]["W"]
    dout = O.normal_fill(seed, 2, 9, 0, 0, n * kw["n_out"] * oh * ow).reshape(n, kw["n_out"], oh, ow)
    return mu, rho, bnp, z, dout


def stat_err(sums, ref_sums, ref_cat):
    """Distance of BN sums [C][2]: sum / HW against the tensor's max, sum of squares / HW against its max squared."""
    hw = ref_cat[0].size; top = np.abs(ref_cat).max()
    d = np.abs(np.asarray(sums, np.float64) - ref_sums) / hw
    return float(max(d[:, 0].max() / top, d[:, 1].max() / top ** 2))


def tol(e32, cap):
    return min(max(4.0 * e32, FLOOR), cap)


# Two ways in which inputs, not kernels, decide a comparison of two fp32 evaluations:
# KINK: a BN output within rounding of zero takes LeakyReLU's slope 1 in one evaluation and 0.2 in the other, and train-mode BN backward
#   spreads that pixel's gradient over its channel.  Two fp32 evaluations of a tensor differ by up to FLOOR of its scale; a case keeps every
#   BN output that feeds a LeakyReLU that far from zero.  (A net of 10^5 activations has one within 1e-6 of zero at most seeds.)
# OFF_CENTRE: the kernels form a channel's variance as E[x^2] - m^2 from fp32 squares (rounding 6e-8 each), which costs a factor 1 + (m / s)^2
#   of precision where the oracle's two-pass variance loses none; at |m| / s <= 4 that is 17 * 6e-8 = 1e-6 of the variance, 5e-7 of the BN
#   output: inside FLOOR.  Beyond it the oracle's e32 no longer sizes the GPU's error.
KINK, OFF_CENTRE = FLOOR, 4.0


def conditioning(P, oc):
    """Of one oracle_program.run result: (the smallest |BN output| / max |BN output| over the tensors with a LeakyReLU, the largest
    |mean| / std over the channels of the tensors with a BatchNorm)."""
    kink, off = np.inf, 0.0
    for t, ybn in oc["bn_out"].items():
        if P.tensors[t]["has_act"]:
            kink = min(kink, float(np.abs(ybn).min() / np.abs(ybn).max()))
        hw = ybn[0].size
        m = oc["sums"][t][:, 0] / hw
        off = max(off, float(np.abs(m / np.sqrt(oc["sums"][t][:, 1] / hw - m * m)).max()))
    return kink, off


@functools.lru_cache(maxsize=None)
def concat_reference(name):
    """Host-side evaluation of CONCAT_CASES[name] -> dict(P, zin, out_id, names, inputs, ref (float64, a list per sample), ora (fp32 oracle,
    a list per sample), tot (float64 dmu / drho / dbn summed over the samples), e32 {quantity: the oracle's distance to the float64 statement}).
    Computed once and shared; callers must not modify it."""
    import mfvi_dip_mia_amd as M
    kw, seed = CONCAT_CASES[name]
    P, zin, out_id, names = M.skip_program(**kw)
    net = SkipNet64(**kw)
    mu, rho, bnp, z, dout = net_inputs(kw, seed, P, centred=True)
    ref = [net.run(mu, rho, bnp, z, seed, STEP, K0 + i, dout[i]) for i in range(N)]
    ora = [oracle_program.run(P, zin, out_id, mu, rho, bnp, z, seed, STEP, K0 + i, dout[i]) for i in range(N)]
    t = names[0]
    e = {}
    worst = lambda f: max(f(r, o) for r, o in zip(ref, ora))
    e["out"] = worst(lambda r, o: relerr(o["out"], r["out"]))
    e["dz"] = worst(lambda r, o: relerr(o["dz"], r["dz"]))
    e["cat"] = worst(lambda r, o: relerr(o["raw"][t["cat"]], r["cat"][0]))
    e["sums"] = worst(lambda r, o: stat_err(o["sums"][t["cat"]], r["sums"][0], r["cat"][0]))
    e["g_cat"] = worst(lambda r, o: relerr(o["g"][t["cat"]], r["g_cat"][0]))
    e["g_deep"] = worst(lambda r, o: relerr(o["g"][t["d2"]], r["g_deep"][0]))
    if t["skip"] is not None:
        e["g_skip"] = worst(lambda r, o: relerr(o["g"][t["skip"]], r["g_skip"][0]))
    tot = {q: sum(r[q] for r in ref) for q in ("dmu", "drho", "dbn")}
    for q in tot:
        e[q] = relerr(sum(o[q] for o in ora), tot[q])
    return dict(P=P, zin=zin, out_id=out_id, names=names, net=net, inputs=(mu, rho, bnp, z, dout), ref=ref, ora=ora, tot=tot, e32=e)


def cap(q):
    """test_small_nets_fwd_bwd's tolerance for quantity q: 2e-5 on the output, 1e-5 on a layer's raw tensor and on its BN mean, 2e-4 on gradients."""
    return OUT_TOL if q == "out" else LAYER_TOL if q in ("cat", "sums") else GRAD_TOL
