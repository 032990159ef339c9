"""Posterior layouts away from the initial one, and the float64 statement of the reparameterised draw and of its chain rule (DESIGN.md
section 29), shared by tests/test_posterior_cases_host.py, tests/test_gpu_posterior_range.py and oracle/make_golden.py.  A helper, not a
test module.

Every other conv-path test draws rho = -3 + 0.1 N (at most +-0.5 N): softplus_fast runs in one branch and sigmoid(rho) is nearly constant.
The layouts here put rho where a fit ends (-13.8: softplus(rho) ~ 1e-6, the den config's prior scale), where softplus_fast changes branch,
where expf underflows, and on pruned weights (rho = -200, mu = 0; csrc/prune.hip).

    fitted   rho = clip(-13.8 + N, -20, -6)                                    mu = 0.1 N
    broad    one run of LADDER in three, the rest clip(-3 + 2 N, -30, 20)       mu = 0.1 N
    ladder   LADDER cycled over the block                                       mu = 0
    pruned   fitted, one weight of every aligned quad at rho = -200, mu = 0     (and the output channels named in `dead`)

LADDER has 217 values, an odd count: cycled over a block whose layers start at multiples of 4, value v sits at flat index t with
t % 217 == v, and the four t below 868 with that residue have four different t & 3 -- every value at every position of a quad.  A layer
shorter than 868 weights sees the rest through `shift` (ladder_shifts), which moves the cycle by multiples of 4."""
import numpy as np

from oracle import oracle as O
from kl_restatement import sigmoid as sigmoid64, softplus as softplus64      # noqa: F401  (torch's softplus, threshold 20, in float64)

PRUNED_RHO = -200.0          # MFVI_PRUNED_RHO (csrc/common.h)
RATIO_FLOOR = -60.0          # drho / sigmoid(rho) is compared where rho >= this: sigmoid(-60) = 8.8e-27 is a normal float32 with room to spare


def _ladder():
    c = np.float32(np.log(0.06))                      # softplus_fast's series / log switch: e < 0.06
    lo = c if float(c) <= np.log(0.06) else np.nextafter(c, np.float32(-np.inf))
    hi = np.nextafter(lo, np.float32(np.inf))
    edge = [np.nextafter(lo, np.float32(-np.inf)), lo, hi, np.nextafter(hi, np.float32(np.inf))]
    v = np.concatenate([np.linspace(-30.0, 20.0, 201), np.asarray(edge, np.float64),
                        [19.9, 20.0, float(np.nextafter(np.float32(20.0), np.float32(np.inf))), 25.0, 50.0],
                        [-45.0, -60.0, -87.0, -88.0, -104.0],
                        [89.0, 120.0]])          # past the overflow of expf: finite only through softplus' x > 20 branch
    return v.astype(np.float32)


LADDER = _ladder()
N_LADDER = LADDER.size                                # 217
assert N_LADDER == 217 and N_LADDER % 2 == 1
BROAD_PERIOD = 3 * N_LADDER                           # 651 = 3 (mod 4): the ladder runs of `broad` start at every position of a quad in turn
LAYOUTS = ("fitted", "broad", "ladder", "pruned")


def ladder_shifts(n):
    """Shifts (multiples of 4) under which a block of n elements sees t = j + shift over all of [0, 4 * 217)."""
    step = max(4, n // 4 * 4) if n >= 4 else 4
    return list(range(0, 4 * N_LADDER, step))


def pruned_mask(n, layers=None, dead=()):
    """One element of every aligned quad of 4 flat indices, at a position hashed from the quad's index: pruned and live weights share every
    quad, filter row and output channel, and any run of whole quads holds exactly a quarter.  dead: (layer index, output channel) pairs
    whose weights and bias are pruned altogether."""
    j = np.arange(n, dtype=np.uint64)
    q = j >> np.uint64(2)
    pos = ((q * np.uint64(2654435761)) >> np.uint64(15)) & np.uint64(3)
    m = (j & np.uint64(3)) == pos
    for li, co in dead:
        l = layers[li]
        per = l["cin"] * l["k"] * l["k"]
        m[l["w_off"] + co * per:l["w_off"] + (co + 1) * per] = True
        m[l["b_off"] + co] = True
    return m


def layout(name, n, seed, shift=0, layers=None, dead=(), rho_span=None):
    """-> (mu, rho) float32 [n].  rho_span = (lo, hi): the live rho of `fitted` / `pruned`, [-20, -6], mapped affinely onto [lo, hi] (the LRT
    cases: -13.8 +- 1 becomes -4 +- 0.64 on [-8, 1])."""
    g_mu = 0.1 * O.normal_fill(seed, 2, 0, 0, 0, n)
    g = O.normal_fill(seed, 2, 1, 0, 0, n).astype(np.float64)
    t = np.arange(n) + int(shift)
    fitted = np.clip(-13.8 + 1.0 * g, -20.0, -6.0)
    if rho_span is not None:
        fitted = rho_span[0] + (rho_span[1] - rho_span[0]) * (fitted + 20.0) / 14.0
    if name == "fitted":
        mu, rho = g_mu, fitted
    elif name == "broad":
        on = (t // N_LADDER) % 3 == 0
        mu, rho = g_mu, np.where(on, LADDER[t % N_LADDER].astype(np.float64), np.clip(-3.0 + 2.0 * g, -30.0, 20.0))
    elif name == "ladder":
        mu, rho = np.zeros(n), LADDER[t % N_LADDER]
    elif name == "pruned":
        m = pruned_mask(n, layers, dead)
        mu, rho = np.where(m, 0.0, g_mu), np.where(m, PRUNED_RHO, fitted)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(mu, np.float32), np.ascontiguousarray(rho, np.float32)


def single_layer(cin, cout, k):
    """The layer table of a one-convolution program (Program.conv: weights, then the bias)."""
    nw = cout * cin * k * k
    return [dict(cin=cin, cout=cout, k=k, w_off=0, b_off=nw)]


def dead_channels(layers):
    """The last output channel of every layer wide enough that one channel stays a small share of it (Cout >= 32: at most 1/32 on top of
    the pruned quarter).  A BatchNorm behind a constant channel has rstd = eps^-1/2 = 316, and that channel alone would set the scale of
    the max-normalised dmu comparison: the whole-net cases name no dead channel."""
    return tuple((i, l["cout"] - 1) for i, l in enumerate(layers) if l["cout"] >= 32)


# ---- the float64 statement -------------------------------------------------------------------------------------------------------------
def w64(mu, rho, eps):
    """w = mu + softplus(rho) * eps (BayTorch/modules/reparam_layers.py:26-37, modules/module.py:82-85)."""
    return np.asarray(mu, np.float64) + softplus64(rho) * np.asarray(eps, np.float64)


def q_of(drho, rho):
    """drho / sigmoid(rho) = sum_k dW_k eps_k: what is left of the chain rule once the factor that spans 87 decades is divided out."""
    return np.asarray(drho, np.float64) / sigmoid64(rho)


BANDS = (("[-30,-20)", -30.0, -20.0), ("[-20,20]", -20.0, 20.0), ("(20,120]", 20.0, 120.0), ("[-87,-30)", -87.0, -30.0))


def band_of(rho):
    """Index into BANDS per element, -1 below -87."""
    r = np.asarray(rho, np.float64)
    b = np.full(r.shape, -1)
    b[(r >= -87.0) & (r < -30.0)] = 3
    b[(r >= -30.0) & (r < -20.0)] = 0
    b[(r >= -20.0) & (r <= 20.0)] = 1
    b[r > 20.0] = 2
    return b


def draw_T(rho):
    """Relative error allowed to the device softplus: 3e-6 on [-30, 20] and above (csrc/common.h's claim for softplus_fast; x > 20 returns x),
    |rho| 2^-23 on [-87, -30) (twice the rounding of the argument rho * log2(e) of a hardware exp2), nothing relative below -87."""
    r = np.asarray(rho, np.float64)
    return np.where(r >= -30.0, 3e-6, np.where(r >= -87.0, np.abs(r) * 2.0 ** -23, 0.0))


def draw_bound(mu, rho, eps):
    """|got - w64| <= 2^-23 |w64| + T(rho) softplus64(rho) |eps| + 2^-125, per element."""
    w = w64(mu, rho, eps)
    return 2.0 ** -23 * np.abs(w) + draw_T(rho) * softplus64(rho) * np.abs(np.asarray(eps, np.float64)) + 2.0 ** -125


def softplus_err(got, mu, rho, eps):
    """Relative error of the softplus the device used, from one draw: |got - w64| / (softplus64 |eps|); meaningful where mu = 0 (one rounding)."""
    e = np.abs(np.asarray(eps, np.float64))
    return np.abs(np.asarray(got, np.float64) - w64(mu, rho, eps)) / np.maximum(softplus64(rho) * e, 1e-300)


# ---- unit-impulse plans: a convolution of impulses returns the sampled weights themselves -----------------------------------------------
def impulse_plan(cin, k, stride, H, W):
    """-> list of passes; a pass is (x [cin, H, W] float32 of unit impulses, ci, ky, kx, yo, xo): output element [co, yo[i], xo[i]] of the pass
    is weight [co, ci[i], ky[i], kx[i]] and nothing else.  Impulses sit in distinct input channels, 2 (k // 2) from the border (reflection
    padding folds no second tap onto them) and k + 1 apart (their footprints do not meet); at stride 2 an impulse sees the taps of its own
    parity only, so a channel takes four passes."""
    p = k // 2
    m = 2 * p
    sp = k + 1
    passes = []
    parities = [(0, 0)] if stride == 1 else [(a, b) for a in (0, 1) for b in (0, 1)]
    for py, px in parities:
        step = sp + sp % 2 if stride == 2 else sp                # an even step keeps the parity
        y_0 = m + ((py - m) % 2 if stride == 2 else 0); x_0 = m + ((px - m) % 2 if stride == 2 else 0)
        pos = [(y, x) for y in range(y_0, H - m, step) for x in range(x_0, W - m, step)]
        assert pos, "map too small for an impulse"
        for c0 in range(0, cin, len(pos)):
            x = np.zeros((cin, H, W), np.float32)
            ci, ky, kx, yo, xo = [], [], [], [], []
            for c, (y0, x0) in zip(range(c0, min(cin, c0 + len(pos))), pos):
                x[c, y0, x0] = 1.0
                for a in range(k):
                    for b in range(k):
                        ty, tx = y0 + p - a, x0 + p - b          # stride * (output index)
                        if ty % stride or tx % stride:
                            continue
                        ci.append(c); ky.append(a); kx.append(b); yo.append(ty // stride); xo.append(tx // stride)
            passes.append((x, np.array(ci), np.array(ky), np.array(kx), np.array(yo), np.array(xo)))
    return passes


def gather_weights(passes, outs, cin, cout, k):
    """outs[i]: output [cout, Ho, Wo] of pass i -> (w [cout, cin, k, k], times each weight was observed [cin, k, k])."""
    w = np.zeros((cout, cin, k, k), outs[0].dtype); seen = np.zeros((cin, k, k), np.int64)
    for (x, ci, ky, kx, yo, xo), y in zip(passes, outs):
        w[:, ci, ky, kx] = y[:, yo, xo]
        np.add.at(seen, (ci, ky, kx), 1)
    return w, seen


# ---- the cases of tests/test_gpu_posterior_range.py --------------------------------------------------------------------------------------
X6, SM, GENERIC, ST = 1 << 25, 1 | 1 << 26, 1 << 27, 1 | 1 << 28
X6_FWD = 1 | 8 << 8 | 1 << 16 | X6                    # the forward tiling tests/test_gpu_fitbatch.py::pin_net_b gives the 36 -> 16 layer
X6_BWD_STRIP = 2 | 8 << 8 | 1 << 16 | X6              # its strip-resident backward-data
X6_BWD = 2 | 8 << 8 | X6                              # bf16x6 backward-data, strips reloaded
# name -> (cin, cout, k, stride, H, W), forward tiling
DRAW_CASES = {
    "generic_5x3": ((5, 3, 3, 1, 33, 47), 0),
    "inkernel_16x16": ((16, 16, 3, 1, 16, 16), GENERIC),
    "mfma_s2": ((16, 16, 3, 2, 16, 16), 0),
    "mfma_5x5": ((8, 12, 5, 1, 12, 16), 0),
    "rowphase_16x16": ((16, 16, 3, 1, 16, 16), 0),
    "x6_36x16": ((36, 16, 3, 1, 64, 64), X6_FWD),
    "small_128": ((128, 128, 3, 1, 8, 8), SM),
    "small_1x1": ((64, 64, 1, 1, 16, 16), SM),
    "stream_1x1": ((16, 4, 1, 1, 8, 8), ST),
}
FWD_FAMILY = {"generic_5x3": 0, "inkernel_16x16": 0, "mfma_s2": 1, "mfma_5x5": 1, "rowphase_16x16": 2, "x6_36x16": 3, "small_128": 4,
              "small_1x1": 4, "stream_1x1": 6}
BF16_CASES = ("rowphase_16x16", "small_1x1")

# Whole-net cases: the NET_B net of tests/test_gpu_fitbatch.py at 64 x 64 (pinned tilings: families 0 - 4 in one plan) and three_scale_32 of
# tests/test_gpu_parity.py on the heuristic tilings.  name -> skip_program arguments
NETS = {
    "net_b_64": dict(H=64, W=64, input_depth=16, n_out=2, nd=(16, 32, 64), nu=(16, 32, 64), ns=(4, 4, 4)),
    "three_scale_32": dict(H=32, W=32, input_depth=8, n_out=2, nd=(8, 16, 16), nu=(8, 16, 16), ns=(4, 4, 4)),
}
NET_STEP, NET_K0, NET_N = 9, 2, 3
KINK = 2e-6
# (net, layout) -> the first seed from 77 on at which every BatchNorm output under a LeakyReLU is at least KINK of its tensor's scale from
# zero in the oracle's forward, in every sample (tests/test_posterior_cases_host.py asserts the distance).  The 64 x 64 net has 3e5
# such outputs and most seeds put one of them closer: 129 and 1067 are the first that do not.  three_scale_32 shares one seed between its
# layouts and with tests/golden/posterior_range.npz (step 3, samples 0 and 1): 79 is the first that serves all four
NET_SEEDS = {("net_b_64", "fitted"): 129, ("net_b_64", "pruned"): 1067, ("three_scale_32", "fitted"): 79, ("three_scale_32", "pruned"): 79}


def net_params(P, name, seed):
    """mu / rho of layout `name` over the program's flat block, BatchNorm parameters as tests/test_gpu_parity.py::_net_params."""
    mu, rho = layout(name, P.n_vi, seed, layers=P.layers)
    g = O.normal_fill(seed, 2, 7, 0, 0, P.n_bn); bnp = np.zeros(P.n_bn, np.float32)
    for b in P.bns:
        c, off = b["C"], b["off"]
        bnp[off:off + c] = 1.0 + 0.1 * g[off:off + c]; bnp[off + c:off + 2 * c] = 0.1 * g[off + c:off + 2 * c]
    return mu, rho, bnp


def net_input(kw, seed):
    return (0.1 * O.uniform_fill(seed, 0, 0, 0, kw["input_depth"] * kw["H"] * kw["W"])).reshape(kw["input_depth"], kw["H"], kw["W"])


def layer_q_err(drho, q_ref, rho, layers):
    """Per layer, weights and bias apart: max |drho / sigmoid64(rho) - q_ref| over the elements with rho >= RATIO_FLOOR, relative to the
    layer's largest |q_ref| (a bias in front of a BatchNorm has a gradient of exactly zero: only the layer gives it a scale).
    -> (worst, [(layer, 'w' | 'b', error, share compared)])."""
    rows = []
    for i, l in enumerate(layers):
        nw = l["cout"] * l["cin"] * l["k"] * l["k"]
        top = max(np.abs(q_ref[l["w_off"]:l["w_off"] + nw]).max(), np.abs(q_ref[l["b_off"]:l["b_off"] + l["cout"]]).max(), 1e-300)
        for tag, a, b in (("w", l["w_off"], l["w_off"] + nw), ("b", l["b_off"], l["b_off"] + l["cout"])):
            r = np.asarray(rho[a:b], np.float64); keep = r >= RATIO_FLOOR
            if not keep.any():
                continue
            q = q_of(np.asarray(drho[a:b], np.float64)[keep], r[keep])
            rows.append((i, tag, float(np.abs(q - q_ref[a:b][keep]).max() / top), float(keep.mean())))
    return max(r[2] for r in rows), rows


def layer_shares(rho, layers):
    """Per layer (weights and bias together): the share of elements with rho >= RATIO_FLOOR, which a ratio check covers."""
    return [float((np.asarray(rho[l["w_off"]:l["b_off"] + l["cout"]]) >= RATIO_FLOOR).mean()) for l in layers]
