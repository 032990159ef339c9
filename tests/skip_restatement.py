"""Float64 torch statement of the skip() hour-glass that skip_program(...) lays out, written from its formulas and
differentiated by autograd.  A helper, not a test module.

Per scale i, on an input x [C][h][w] (module order, which is also the order of the flat parameter layout):
    s   = act(BN(conv_fs,1(x)))                         only if ns[i] > 0
    d   = act(BN(conv_fd,1(act(BN(conv_fd,2(x))))))     ceil(h/2) x ceil(w/2)
    d   = scale i+1 applied to d                        unless i is the deepest scale
    u   = Upsample x2 (d)                               bilinear with align_corners=False, or nearest
    cat = [s, u[:, :h, :w]]                             Concat drops the LAST row / column of u where h / w is odd; without s: cat = u
    top = act(BN(conv_1,1(act(BN(conv_fu,1(BN(cat)))))))       the 1x1 pair only with need1x1_up
and out = conv_1,1(top of scale 0).  conv_k,s = reflection pad k // 2, then conv2d at stride s, with w = mu + softplus(rho) * eps and
eps = oracle.eps(seed, step, sample, layer, tensor, n) (tensor 0: weight, 1: bias).  BN = train-mode BatchNorm over the one sample
(biased variance, eps 1e-5), act = LeakyReLU(0.2).  Parameters come in the flat mu | rho | bn layout that Program assigns: per layer
the weight then the bias, per BatchNorm gamma then beta, both in module order."""
import numpy as np
import torch

from oracle import oracle as O

F = torch.nn.functional

WRONG = ("crop_first", "align_corners", "shift")      # deliberately wrong variants of the concat, for the sensitivity checks


def relerr(a, b):
    """The project's relative error: max |a - b| / max |b|."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def conv64(x, w, b, stride):
    """Reflection pad k // 2, then conv2d: x [Cin][H][W], w [Cout][Cin][k][k], b [Cout] -> [Cout][Ho][Wo]."""
    k = w.shape[-1]
    x = x[None]
    if k > 1:
        x = F.pad(x, (k // 2,) * 4, mode="reflect")
    return F.conv2d(x, w, b, stride=stride)[0]


def bn64(x, gamma, beta, eps=1e-5):
    """Train-mode BatchNorm of one sample: per channel over H x W, biased variance."""
    m = x.mean(dim=(1, 2), keepdim=True)
    v = ((x - m) ** 2).mean(dim=(1, 2), keepdim=True)
    return (x - m) / torch.sqrt(v + eps) * gamma[:, None, None] + beta[:, None, None]


def act64(x, slope=0.2):
    return torch.where(x > 0, x, slope * x)


def upsample64(x, mode="bilinear", align_corners=False):
    if mode == "nearest":
        return F.interpolate(x[None], scale_factor=2, mode="nearest")[0]
    return F.interpolate(x[None], scale_factor=2, mode="bilinear", align_corners=align_corners)[0]


def sampled(mu, rho, lay, seed, step, sample, lid):
    """w [Cout][Cin][k][k], b [Cout] of layer `lid` (a dict of cin, cout, k, w_off, b_off) for one MC sample."""
    cin, cout, k = lay["cin"], lay["cout"], lay["k"]
    nw = cout * cin * k * k
    ew = torch.from_numpy(O.eps(seed, step, sample, lid, 0, nw).astype(np.float64))
    eb = torch.from_numpy(O.eps(seed, step, sample, lid, 1, cout).astype(np.float64))
    wo, bo = lay["w_off"], lay["b_off"]
    w = (mu[wo:wo + nw] + F.softplus(rho[wo:wo + nw]) * ew).reshape(cout, cin, k, k)
    return w, mu[bo:bo + cout] + F.softplus(rho[bo:bo + cout]) * eb


class SkipNet64:
    """The hour-glass with the parameters of skip_program.  .layers / .bns / .n_vi / .n_bn restate the flat layout (compare P.layers, P.bns);
    .scales[i] names the layers and BatchNorms of scale i."""

    def __init__(self, H, W, input_depth=16, n_out=2, nd=(16, 32, 64, 128, 128), nu=(16, 32, 64, 128, 128), ns=(4, 4, 4, 4, 4),
                 fd=3, fu=3, fs=1, need1x1_up=True, upsample_mode="bilinear"):
        self.H, self.W, self.input_depth, self.n_out = H, W, input_depth, n_out
        self.nd, self.nu, self.ns, self.fd, self.fu, self.fs = tuple(nd), tuple(nu), tuple(ns), fd, fu, fs
        self.need1x1_up, self.mode = need1x1_up, upsample_mode
        self.layers, self.bns, self.n_vi, self.n_bn = [], [], 0, 0
        self.scales = [None] * len(nd)
        self._layout(0, input_depth)
        self.final = self._conv(nu[0], n_out, 1, 1, bn=False)[0]

    def _conv(self, cin, cout, k, stride, bn=True):
        w_off = self.n_vi
        self.n_vi += cout * cin * k * k + cout
        self.layers.append(dict(cin=cin, cout=cout, k=k, stride=stride, w_off=w_off, b_off=self.n_vi - cout))
        return len(self.layers) - 1, (self._bn(cout) if bn else None)

    def _bn(self, c):
        self.bns.append(dict(C=c, off=self.n_bn))
        self.n_bn += 2 * c
        return len(self.bns) - 1

    def _layout(self, i, cin):
        s = dict(skip=self._conv(cin, self.ns[i], self.fs, 1) if self.ns[i] else None)
        s["d1"] = self._conv(cin, self.nd[i], self.fd, 2)
        s["d2"] = self._conv(self.nd[i], self.nd[i], self.fd, 1)
        kk = self.nd[i]
        if i < len(self.nd) - 1:
            self._layout(i + 1, self.nd[i]); kk = self.nu[i + 1]
        s["cat_bn"] = self._bn(self.ns[i] + kk)
        s["up"] = self._conv(self.ns[i] + kk, self.nu[i], self.fu, 1)
        s["up1"] = self._conv(self.nu[i], self.nu[i], 1, 1) if self.need1x1_up else None
        self.scales[i] = s

    def forward(self, mu, rho, bn, z, seed, step, sample, wrong=None):
        """One MC sample on float64 tensors -> (out, taps); taps[i] holds, for scale i, the raw concat tensor `cat`, its BN output `cat_bn`
        and the BN outputs (before the LeakyReLU) of the two concat inputs, `skip_bn` (None without a skip branch) and `deep_bn`.
        wrong: one of WRONG, applied at every concat."""
        assert wrong is None or wrong in WRONG
        taps = [None] * len(self.nd)

        def norm(x, bid):
            c, off = self.bns[bid]["C"], self.bns[bid]["off"]
            return bn64(x, bn[off:off + c], bn[off + c:off + 2 * c])

        def block(x, ids):
            lid, bid = ids
            w, b = sampled(mu, rho, self.layers[lid], seed, step, sample, lid)
            h = norm(conv64(x, w, b, self.layers[lid]["stride"]), bid)
            return act64(h), h

        def scale(i, x):
            s, (h, w) = self.scales[i], x.shape[1:]
            sk, sk_bn = block(x, s["skip"]) if s["skip"] else (None, None)
            deep, deep_bn = block(block(x, s["d1"])[0], s["d2"])
            if i < len(self.nd) - 1:
                deep, deep_bn = scale(i + 1, deep)
            src = torch.roll(deep, 1, dims=-1) if wrong == "shift" else deep
            up = upsample64(src, self.mode, align_corners=(wrong == "align_corners"))
            if sk is not None:
                r0, c0 = (up.shape[1] - h, up.shape[2] - w) if wrong == "crop_first" else (0, 0)
                cat = torch.cat([sk, up[:, r0:r0 + h, c0:c0 + w]], 0)
            else:
                cat = up
            cat_bn = norm(cat, s["cat_bn"])
            taps[i] = dict(cat=cat, cat_bn=cat_bn, skip_bn=sk_bn, deep_bn=deep_bn)
            top, top_bn = block(cat_bn, s["up"])
            if s["up1"]:
                top, top_bn = block(top, s["up1"])
            return top, top_bn

        top, _ = scale(0, z)
        w, b = sampled(mu, rho, self.layers[self.final], seed, step, sample, self.final)
        return conv64(top, w, b, 1), taps

    def run(self, mu, rho, bn, z, seed, step, sample, dout=None, wrong=None):
        """numpy in, numpy float64 out: dict(out, cat[i], sums[i] ([C][2]: per-channel sum and sum of squares of cat[i])) and, for a given
        dout (the gradient of a scalar loss wrt out), dmu, drho, dbn, dz and per scale g_cat[i], g_skip[i], g_deep[i]: the gradients wrt the
        BN outputs of the concat tensor and of its two inputs."""
        t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=dout is not None)
        mu, rho, bn, z = t(mu), t(rho), t(bn), t(z)
        out, taps = self.forward(mu, rho, bn, z, seed, step, sample, wrong)
        n = lambda a: None if a is None else a.detach().numpy().copy()
        cats = [tp["cat"].detach() for tp in taps]
        r = dict(out=n(out), cat=[n(c) for c in cats], sums=[np.stack([n(c.sum(dim=(1, 2))), n((c * c).sum(dim=(1, 2)))], 1) for c in cats])
        if dout is None:
            return r
        kept = [[tp[k] for k in ("cat_bn", "skip_bn", "deep_bn")] for tp in taps]
        for ks in kept:
            for a in ks:
                if a is not None:
                    a.retain_grad()
        (out * torch.tensor(np.asarray(dout, np.float64))).sum().backward()
        g = lambda a: None if a is None else a.grad.numpy().copy()
        r.update(dmu=g(mu), drho=g(rho), dbn=g(bn), dz=g(z), g_cat=[g(ks[0]) for ks in kept], g_skip=[g(ks[1]) for ks in kept],
                 g_deep=[g(ks[2]) for ks in kept])
        return r


def conv_case64(x, w, b, stride, dy=None):
    """One convolution in float64: y, or (y, dx, dw, db) for a given dy."""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=dy is not None)
    wt = torch.tensor(np.asarray(w, np.float64), requires_grad=dy is not None)
    bt = torch.tensor(np.asarray(b, np.float64), requires_grad=dy is not None)
    y = conv64(xt, wt, bt, stride)
    if dy is None:
        return y.detach().numpy()
    (y * torch.tensor(np.asarray(dy, np.float64))).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), wt.grad.numpy(), bt.grad.numpy()
