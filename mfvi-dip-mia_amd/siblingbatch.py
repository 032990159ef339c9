"""Many independent DIP / MC-dropout / SGLD fits advanced by ONE iteration of launches.

The reference sweeps dropout_p x weight_decay (MC dropout) and gamma x weight_decay (SGLD) as one process per candidate, each a chain of
small K = 1 launches (bayesian_optimization.py:1447-1655, 1658-1860, 3715-3718).  A SiblingBatch of F fits with K samples each is one plan
of F * K samples in fits mode with point weights (mfvi_plan_set_fits_points: w = mu of the sample's fit) and, for MC dropout, one Dropout2d
probability per fit (mfvi_plan_set_fit_dropout).  One iteration is

    mu[f] += sigma * lr0[f] * N(0,1) on the conv weights   SGLD only; RNG domain SGLD, stream layer, sample f   (mfvi_add_normal_fits)
    z[f]   = z0[f] + 0.1 * N(0,1)                          RNG domain INPUT, sample f                           (rowbatch.py: the perturbation)
    out    = net(z), w = mu                                dropout masks of global sample f * K + k             (mfvi_forward, points mode)
    loss[f]                                                MSE on channel 0 (dip, sgld den) / Gaussian NLL      (mfvi_mse_channel_fits / mfvi_gaussian_nll_fits)
    grads                                                                                                        (mfvi_backward, points mode)
    AdamW with lr[f], weight_decay[f]; lr[f] *= gamma[f]                                                         (mfvi_sibling_update_fits)
    ema[f]                                                 on a second stream beside the backward pass          (mfvi_ema_fits)

whatever F is.  RNG identity: fit f owns the global samples f * K .. f * K + K - 1 (dropout masks) and sample f of every per-fit stream
(initialisation, z0, input perturbation, SGLD noise), so fit 0 of a batch is the standalone SiblingEngine(seed)."""
import math

from . import _lib as L
from .rowbatch import TASKS, RowBatch, per_fit

METHODS = ("dip", "mcd", "sgld")
LR_FLOOR = 1e-8         # ExponentialLR steps while the rate is above it (bayesian_optimization.py:1784-1785)


def check_args(H, W, n_fits, method, task, K, lr, weight_decay, dropout_p, gamma, init, param_dtype="f32"):
    """Everything that can be refused without the library; -> (lrs, weight_decays, dropout_ps, gammas), one value per fit."""
    if method not in METHODS:
        raise ValueError("method %r: 'dip', 'mcd' or 'sgld'" % (method,))
    if task in ("ct", "inp"):
        raise NotImplementedError("SiblingBatch serves denoising and super-resolution; the data terms of task %r are not batched" % (task,))
    if task not in TASKS:
        raise ValueError("task %r: 'den' or 'sr'" % (task,))
    if param_dtype != "f32":
        raise NotImplementedError("SiblingBatch takes float32 parameters, not %r" % (param_dtype,))
    if int(n_fits) < 1 or int(K) < 1 or int(n_fits) * int(K) > 65535:
        raise ValueError("n_fits=%r, K=%r: at least 1 each, n_fits * K < 65536" % (n_fits, K))
    if H < 1 or W < 1 or H % 4 or W % 4:
        raise ValueError("H=%r, W=%r: multiples of 4 (the input-scale layers run on the matrix-core kernels)" % (H, W))
    if init not in ("per_fit", "shared"):
        raise ValueError("init %r: 'per_fit' or 'shared'" % (init,))
    lrs, wds = per_fit(lr, n_fits, "lr"), per_fit(weight_decay, n_fits, "weight_decay")
    ps, gammas = per_fit(dropout_p, n_fits, "dropout_p"), per_fit(gamma, n_fits, "gamma")
    if any(not r > 0.0 for r in lrs) or any(not w >= 0.0 for w in wds):
        raise ValueError("lr must be > 0 and weight_decay >= 0 for every fit")
    if any(not 0.0 <= p < 1.0 for p in ps):
        raise ValueError("dropout_p outside [0, 1)")
    if any(not 0.0 < g <= 1.0 for g in gammas):
        raise ValueError("gamma outside (0, 1]")
    if method != "mcd":
        ps = [0.0] * int(n_fits)
    if method != "sgld":
        gammas = [1.0] * int(n_fits)      # a constant rate: lr * 1.0 == lr
    return lrs, wds, ps, gammas


class SiblingBatch(RowBatch):
    """The one-group RowBatch with point weights: rowbatch.py runs the iteration; here are the per-fit dropout, lr schedule and weight
    decay, SGLD's noise, the MSE-or-NLL data term, AdamW and the engine of one fit."""
    sample_weights = False      # w = mu of the sample's fit
    targets = None

    def __init__(self, H, W, n_fits, method, task="den", K=1, input_depth=16, lr=1e-3, weight_decay=0.0, dropout_p=0.3, gamma=0.996,
                 param_noise_sigma=2.0, seed=1, sr_factor=4, net_kwargs=None, init="per_fit", autotune=True, param_dtype="f32", tv_weight=0.0,
                 tv_beta=0.5):
        self.lr0s, self.weight_decays, self.dropout_ps, self.gammas = check_args(H, W, n_fits, method, task, K, lr, weight_decay, dropout_p, gamma,
                                                                                 init, param_dtype)
        if task == "sr" and (sr_factor < 1 or H % sr_factor or W % sr_factor):
            raise ValueError("sr_factor %r does not divide %dx%d" % (sr_factor, H, W))
        from .tv import check_tv
        self.tv_weights, self.tv_beta = check_tv(tv_weight, tv_beta, task, n=int(n_fits))      # a scalar, or one weight per fit
        self.method, self.task, self.F, self.sr_factor = method, task, int(n_fits), int(sr_factor)
        self.param_noise_sigma = float(param_noise_sigma)
        self.net_kwargs = dict(net_kwargs or {})
        nk = dict(self.net_kwargs)
        self.plan_p = max(self.dropout_ps)                           # the plan's ops carry dropout at max(p); set_fit_dropout supplies each fit's own
        if method == "mcd":
            nk.update(drop_down=self.plan_p, drop_up=self.plan_p)
        self.mse_image = method == "dip" or (method == "sgld" and task == "den")      # F.mse_loss(out[:, :1], target), else the Gaussian NLL
        self._allocate(n_fits, n_fits, K, H, W, 2, input_depth, nk, seed, init, autotune)
        self.plan.set_fits_points(True)
        if method == "mcd" and self.plan_p > 0.0:
            self.plan.set_fit_dropout(self.dropout_ps)

    def _alloc_own(self):
        import numpy as np
        torch, F = self.torch, self.F
        self.loss_acc = self.nll_acc                                 # the float64 loss accumulators behind the gradient rows
        self._hyper_dtype = np.dtype([("lr", "<f8"), ("gamma", "<f8"), ("weight_decay", "<f4"), ("lr_floor", "<f4")])      # mfvi_sibling_hyper
        self.hyper = torch.zeros(F * self._hyper_dtype.itemsize, dtype=torch.uint8, device="cuda")
        self.noise_std = torch.tensor([self.param_noise_sigma * r for r in self.lr0s], dtype=torch.float32, device="cuda")    # add_noise keeps the initial rate
        lay = [(l["w_off"], l["cout"] * l["cin"] * l["k"] * l["k"]) for l in self.prog.layers]                                 # the 4-D parameters only
        self.layer_off = torch.tensor([o for o, _ in lay], dtype=torch.int64, device="cuda")
        self.layer_n = torch.tensor([n for _, n in lay], dtype=torch.int64, device="cuda")

    def _write_hyper(self, lrs):
        import numpy as np
        h = np.zeros(self.F, self._hyper_dtype)
        h["lr"], h["gamma"], h["weight_decay"], h["lr_floor"] = lrs, self.gammas, self.weight_decays, LR_FLOOR
        self.hyper.copy_(self.torch.from_numpy(h.view(np.uint8)))

    def lrs(self):
        """[F] float64: every fit's current learning rate (lr0 * gamma^steps while above the floor) -- forces a device sync."""
        return self.hyper.cpu().numpy().view(self._hyper_dtype)["lr"].copy()

    def _fill_row(self, f):
        """mu and z0 of fit f as SiblingEngine.init_params fills them, with sample f of the UNIFORM streams (rho stays the unused zero block)."""
        lib, sp = L.lib(), L.stream_ptr()
        mu = self._pbuf[f]
        for lid, lay in enumerate(self.prog.layers):
            bound = 1.0 / math.sqrt(lay["cin"] * lay["k"] * lay["k"])
            cnt = lay["cout"] * lay["cin"] * lay["k"] * lay["k"] + (lay["cout"] if lay["b_off"] >= 0 else 0)
            L.check(lib.mfvi_uniform_fill_range(self.seed, 16 + lid, f, 0, cnt, -bound, bound, L.ptr(mu[lay["w_off"]:]), sp))
        L.check(lib.mfvi_uniform_fill(self.seed, 0, f, 0, self.z0[f].numel(), 0.1, L.ptr(self.z0[f]), sp))

    def _after_init(self):
        self._write_hyper(self.lr0s)
        self._mark_bad_targets()

    def _mark_bad_targets(self):
        """Every pixel of a target enters its fit's data term, so a fit whose target is not finite can never have a finite loss: it is dead
        before its first iteration (and before SGLD's first noise launch would change its parameters).  On the device, no sync."""
        if self.targets is not None:
            self.dead_dev |= (~self.torch.isfinite(self.targets).flatten(1).all(dim=1)).to(self.torch.int32)

    def set_targets(self, targets):
        """den: the noisy images [F, H, W]; sr: the low-resolution images [F, H / f, W / f]."""
        t = self.torch.as_tensor(targets)
        f = self.sr_factor if self.task == "sr" else 1
        if tuple(t.shape) != (self.F, self.H // f, self.W // f):
            raise ValueError("targets of shape %s, expected %s" % (tuple(t.shape), (self.F, self.H // f, self.W // f)))
        self.targets = t.contiguous().float().cuda()
        self._mark_bad_targets()

    def add_noise(self, step=None):
        """SGLD's add_noise on the conv weights of every live fit: std = param_noise_sigma * lr0[f], one launch."""
        step = self.t if step is None else int(step)
        L.check(L.lib().mfvi_add_normal_fits(L.ptr(self._pbuf), self.stride, self.F, 0, L.ptr(self.layer_off), L.ptr(self.layer_n), self.layer_n.numel(),
                                             self.seed, step, L.ptr(self.noise_std), L.ptr(self.dead_dev), L.stream_ptr()))

    def _require_targets(self):
        if self.targets is None:
            raise ValueError("set_targets first")

    def _data_term(self, d0, nd, out, dout):      # one group: d0 = 0, nd = F
        lib, sp = L.lib(), L.stream_ptr()
        f = self.sr_factor if self.task == "sr" else 1
        if self.mse_image:
            L.check(lib.mfvi_mse_channel_fits(L.ptr(out), L.ptr(self.targets), self.targets[0].numel(), nd, self.K, 2, self.H, self.W, 0, f, 1.0 / self.K,
                                              L.ptr(dout), L.ptr(self.loss_acc), sp))
        else:
            L.check(lib.mfvi_gaussian_nll_fits(L.ptr(out), L.ptr(self.targets), self.targets[0].numel(), nd, self.K, self.H, self.W, f, 1.0 / self.K,
                                               L.ptr(dout), L.ptr(self.loss_acc), sp))

    def _pre_step(self):
        if self.method == "sgld":
            self.add_noise(self.t)

    def _update(self):
        """AdamW with lr[f], weight_decay[f]; lr[f] *= gamma[f].  A dead fit keeps its lr too."""
        L.check(L.lib().mfvi_sibling_update_fits(L.ptr(self._pbuf), L.ptr(self._grows), L.ptr(self._mbuf), L.ptr(self._vbuf), self.n_vi, self.n_bn, self.stride,
                                                 self.stride, self.F, L.ptr(self.hyper), 0.9, 0.999, 1e-8, self.t, L.ptr(self.loss_acc), L.ptr(self.dead_dev),
                                                 L.stream_ptr()))

    def losses(self):
        """[F]: the data term of the last step (mean over the fit's K samples) -- forces a device sync."""
        return self.loss_acc.cpu().numpy() / self.K

    def _make_engine(self, f, autotune):
        from .engine import SiblingEngine
        eng = SiblingEngine(self.H, self.W, method=self.method, task=self.task, weight_decay=self.weight_decays[f], dropout_p=self.dropout_ps[f],
                            gamma=self.gammas[f], param_noise_sigma=self.param_noise_sigma, net_kwargs=self.net_kwargs, K=self.K,
                            input_depth=self.input_depth, lr=self.lr0s[f], seed=self.seed, sr_factor=self.sr_factor, autotune=autotune, **self._tv_kw(f))
        eng.lr = float(self.lrs()[f]); eng.lr0 = self.lr0s[f]        # the copy continues the fit's schedule
        return eng

    def _hand_target(self, eng, f):
        if self.targets is not None:
            eng.set_target(self.targets[f].clone())
