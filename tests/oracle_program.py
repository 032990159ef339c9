"""A layer program run on the C oracle's fp32 primitives, op by op (oracle/oracle.py: conv_fwd, bn_fwd, lrelu_fwd, upsample2_*_fwd and their
adjoints): the fp32 CPU evaluation of programs that oracle.net_forward cannot express (nearest up-sampling, no skip branch, conv chains), with
every intermediate tensor and gradient at hand.  On the nets net_forward does express it performs the same calls in the same order
(tests/test_skip_restatement_host.py holds the two equal).  A helper, not a test module."""
import numpy as np

from oracle import oracle as O

f32 = np.float32


def run(P, zin, out_id, mu, rho, bn, z, seed, step, sample, dout=None):
    """One MC sample.  -> dict(out, raw {tid: raw tensor}, sums {tid: [C][2] float64 sum / sum of squares of the raw tensor}, bn_out {tid: BN
    output before the LeakyReLU}) and, for a given dout, dmu, drho (float64 [n_vi]), dbn (float64 [n_bn]), dz and g {tid: gradient wrt the
    tensor's BN output}."""
    mu, rho, bn = np.asarray(mu, f32), np.asarray(rho, f32), np.asarray(bn, f32)
    raw = {zin: np.ascontiguousarray(z, f32)}
    seen = {}          # tid -> (BN output, mean, rstd, activated view)
    wts = {}           # op index -> sampled (w, eps_w, eps_b)

    def view(t):
        d = P.tensors[t]
        if not d["has_bn"]:
            return raw[t]
        if t not in seen:
            c, off = d["C"], d["bn_off"]
            ybn, m, r = O.bn_fwd(raw[t], bn[off:off + c], bn[off + c:off + 2 * c], d["eps"])
            seen[t] = (ybn, m, r, O.lrelu_fwd(ybn, d["slope"]) if d["has_act"] else ybn)
        return seen[t][3]

    for i, op in enumerate(P.ops):
        if op["type"] == 1:
            lay = P.layers[op["layer_id"]]
            cin, cout, k = lay["cin"], lay["cout"], lay["k"]
            nw, wo, bo = cout * cin * k * k, lay["w_off"], lay["b_off"]
            ew = O.eps(seed, step, sample, op["layer_id"], 0, nw); eb = O.eps(seed, step, sample, op["layer_id"], 1, cout)
            w = O.reparam(mu[wo:wo + nw], rho[wo:wo + nw], ew).reshape(cout, cin, k, k)
            wts[i] = (w, ew, eb)
            raw[op["out"]] = O.conv_fwd(view(op["in0"]), w, O.reparam(mu[bo:bo + cout], rho[bo:bo + cout], eb), lay["stride"])
        else:
            d = P.tensors[op["out"]]
            up = (O.upsample2_nearest_fwd if op["up_mode"] == 1 else O.upsample2_fwd)(view(op["in1"]))[:, :d["H"], :d["W"]]
            raw[op["out"]] = np.ascontiguousarray(up if op["in0"] < 0 else np.concatenate([view(op["in0"]), up], 0))
    res = dict(out=raw[out_id], raw=raw)
    res["sums"] = {t: np.stack([a.astype(np.float64).sum(axis=(1, 2)), (a.astype(np.float64) ** 2).sum(axis=(1, 2))], 1) for t, a in raw.items()}
    res["bn_out"] = {t: v[0] for t, v in seen.items()}
    if dout is None:
        return res
    dmu = np.zeros(P.n_vi); drho = np.zeros(P.n_vi); dbn = np.zeros(max(P.n_bn, 1))
    gv = {out_id: np.ascontiguousarray(dout, f32)}          # gradient wrt a tensor's view, summed over its consumers
    g = {}

    def add(t, d):
        gv[t] = d if t not in gv else gv[t] + d

    sig = 1.0 / (1.0 + np.exp(-rho.astype(np.float64)))
    for i in reversed(range(len(P.ops))):
        op = P.ops[i]
        t, d = op["out"], P.tensors[op["out"]]
        gr = gv[t]
        if d["has_bn"]:
            ybn, m, r, _ = seen[t]
            gb = np.where(ybn > 0, gr, f32(d["slope"]) * gr).astype(f32) if d["has_act"] else gr
            g[t] = gb
            c, off = d["C"], d["bn_off"]
            gr, dg, db = O.bn_bwd(raw[t], bn[off:off + c], m, r, gb)
            dbn[off:off + c] += dg; dbn[off + c:off + 2 * c] += db
        if op["type"] == 1:
            lay = P.layers[op["layer_id"]]
            cin, cout, k = lay["cin"], lay["cout"], lay["k"]
            nw, wo, bo = cout * cin * k * k, lay["w_off"], lay["b_off"]
            w, ew, eb = wts[i]
            dx, dw, db = O.conv_bwd(view(op["in0"]), w, lay["stride"], gr)
            dmu[wo:wo + nw] += dw.ravel(); dmu[bo:bo + cout] += db
            drho[wo:wo + nw] += dw.ravel() * ew * sig[wo:wo + nw]; drho[bo:bo + cout] += db * eb * sig[bo:bo + cout]
            add(op["in0"], dx)
        else:
            ca = 0 if op["in0"] < 0 else P.tensors[op["in0"]]["C"]
            if ca:
                add(op["in0"], np.ascontiguousarray(gr[:ca]))
            b = P.tensors[op["in1"]]
            full = np.zeros((b["C"], 2 * b["H"], 2 * b["W"]), f32)          # adjoint of the crop: the dropped row / column gets no gradient
            full[:, :d["H"], :d["W"]] = gr[ca:]
            add(op["in1"], (O.upsample2_nearest_bwd if op["up_mode"] == 1 else O.upsample2_bwd)(full))
    res.update(dmu=dmu, drho=drho, dbn=dbn[:P.n_bn], dz=gv[zin], g=g)
    return res
