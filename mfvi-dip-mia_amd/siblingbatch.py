"""Many independent DIP / MC-dropout / SGLD fits advanced by ONE iteration of launches.

The reference sweeps dropout_p x weight_decay (MC dropout) and gamma x weight_decay (SGLD) as one process per candidate, each a chain of
small K = 1 launches (bayesian_optimization.py:1447-1655, 1658-1860, 3715-3718).  A SiblingBatch of F fits with K samples each is one plan
of F * K samples in fits mode with point weights (mfvi_plan_set_fits_points: w = mu of the sample's fit) and, for MC dropout, one Dropout2d
probability per fit (mfvi_plan_set_fit_dropout).  One iteration is

    mu[f] += sigma * lr0[f] * N(0,1) on the conv weights   SGLD only; RNG domain SGLD, stream layer, sample f   (mfvi_add_normal_fits)
    z[f]   = z0[f] + 0.1 * N(0,1)                          RNG domain INPUT, sample f                           (mfvi_perturb_input_fits)
    out    = net(z), w = mu                                dropout masks of global sample f * K + k             (mfvi_forward, points mode)
    loss[f]                                                MSE on channel 0 (dip, sgld den) / Gaussian NLL      (mfvi_mse_channel_fits / mfvi_gaussian_nll_fits)
    grads                                                                                                        (mfvi_backward, points mode)
    AdamW with lr[f], weight_decay[f]; lr[f] *= gamma[f]                                                         (mfvi_sibling_update_fits)
    ema[f]                                                 on a second stream beside the backward pass          (mfvi_ema_fits)

whatever F is.  RNG identity: fit f owns the global samples f * K .. f * K + K - 1 (dropout masks) and sample f of every per-fit stream
(initialisation, z0, input perturbation, SGLD noise), so fit 0 of a batch is the standalone SiblingEngine(seed)."""
import math

from . import _lib as L
from .fitbatch import EXP_WEIGHT, TASKS, per_fit
from .program import skip_program

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


class SiblingBatch:
    _book = None            # a BatchBook once track()ed

    def __init__(self, H, W, n_fits, method, task="den", K=1, input_depth=16, lr=1e-3, weight_decay=0.0, dropout_p=0.3, gamma=0.996,
                 param_noise_sigma=2.0, seed=1, sr_factor=4, net_kwargs=None, init="per_fit", autotune=True, param_dtype="f32"):
        self.lr0s, self.weight_decays, self.dropout_ps, self.gammas = check_args(H, W, n_fits, method, task, K, lr, weight_decay, dropout_p, gamma,
                                                                                 init, param_dtype)
        if task == "sr" and (sr_factor < 1 or H % sr_factor or W % sr_factor):
            raise ValueError("sr_factor %r does not divide %dx%d" % (sr_factor, H, W))
        import numpy as np
        import torch
        self.torch = torch
        self.method, self.task, self.F, self.K, self.H, self.W = method, task, int(n_fits), int(K), H, W
        self.seed, self.sr_factor, self.input_depth, self.init = int(seed), int(sr_factor), int(input_depth), init
        self.param_noise_sigma = float(param_noise_sigma)
        self.net_kwargs = dict(net_kwargs or {})
        nk = dict(self.net_kwargs)
        self.plan_p = max(self.dropout_ps)                           # the plan's ops carry dropout at max(p); set_fit_dropout supplies each fit's own
        if method == "mcd":
            nk.update(drop_down=self.plan_p, drop_up=self.plan_p)
        self.prog, self.zin, self.zout, self.names = skip_program(H, W, input_depth, 2, **nk)
        F, K, P = self.F, self.K, self.prog
        self.n = F * K
        self.plan = P.compile(self.zin, self.zout, self.n)
        self.n_vi, self.n_bn = P.n_vi, P.n_bn
        self.n_params = 2 * P.n_vi + P.n_bn
        self.stride = (self.n_params + 3) // 4 * 4                   # row stride of params / m / v / grads, as FitBatch
        dev = "cuda"
        self._pbuf = torch.zeros((F, self.stride), dtype=torch.float32, device=dev)
        self._mbuf = torch.zeros_like(self._pbuf); self._vbuf = torch.zeros_like(self._pbuf)
        self.params, self.m, self.v = self._pbuf[:, :self.n_params], self._mbuf[:, :self.n_params], self._vbuf[:, :self.n_params]
        # gradients and the float64 loss accumulators in ONE allocation: one fill launch clears both per iteration
        self._gbuf = torch.zeros(4 * F * self.stride + 8 * F, dtype=torch.uint8, device=dev)
        self._grows = self._gbuf[:4 * F * self.stride].view(torch.float32).view(F, self.stride)
        self.grads = self._grows[:, :self.n_params]
        self.loss_acc = self._gbuf[4 * F * self.stride:].view(torch.float64)
        self.dead_dev = torch.zeros(F, dtype=torch.int32, device=dev)
        self._hyper_dtype = np.dtype([("lr", "<f8"), ("gamma", "<f8"), ("weight_decay", "<f4"), ("lr_floor", "<f4")])      # mfvi_sibling_hyper
        self.hyper = torch.zeros(F * self._hyper_dtype.itemsize, dtype=torch.uint8, device=dev)
        self.noise_std = torch.tensor([self.param_noise_sigma * r for r in self.lr0s], dtype=torch.float32, device=dev)    # add_noise keeps the initial rate
        lay = [(l["w_off"], l["cout"] * l["cin"] * l["k"] * l["k"]) for l in P.layers]                                      # the 4-D parameters only
        self.layer_off = torch.tensor([o for o, _ in lay], dtype=torch.int64, device=dev)
        self.layer_n = torch.tensor([n for _, n in lay], dtype=torch.int64, device=dev)
        self.z0 = torch.empty((F, input_depth, H, W), dtype=torch.float32, device=dev)
        self.z = torch.empty_like(self.z0)
        self.out = torch.empty((self.n, 2, H, W), dtype=torch.float32, device=dev)
        self.dout = torch.empty_like(self.out)
        self.ema = torch.zeros((F, 2, H, W), dtype=torch.float32, device=dev)
        self.targets = None
        self.t = 0
        self._ema_n = 0
        self._side = None; self._ema_done = None
        self.mse_image = method == "dip" or (method == "sgld" and task == "den")      # F.mse_loss(out[:, :1], target), else the Gaussian NLL
        self.init_params()
        if autotune:                     # before the mode is switched on (tilings do not depend on it), with fit 0's parameters and input
            f0 = self.fit(0)
            self.plan.autotune(f0["mu"], f0["rho"], f0["bn"], self.z0[0], self.n)
        self.plan.set_fits(K, self.stride, self.stride)
        self.plan.set_fits_points(True)
        if method == "mcd" and self.plan_p > 0.0:
            self.plan.set_fit_dropout(self.dropout_ps)

    # -------------------------------------------------------------------------------------------
    def fit(self, f):
        """Views of fit f: dict(mu, rho, bn, params, m, v, grads, z0, ema).  rho is the unused (zero) RHO block."""
        n = self.n_vi
        p = self._pbuf[f]
        return dict(mu=p[:n], rho=p[n:2 * n], bn=p[2 * n:self.n_params], params=p[:self.n_params], m=self._mbuf[f, :self.n_params],
                    v=self._vbuf[f, :self.n_params], grads=self._grows[f, :self.n_params], z0=self.z0[f], ema=self.ema[f])

    def _write_hyper(self, lrs):
        import numpy as np
        h = np.zeros(self.F, self._hyper_dtype)
        h["lr"], h["gamma"], h["weight_decay"], h["lr_floor"] = lrs, self.gammas, self.weight_decays, LR_FLOOR
        self.hyper.copy_(self.torch.from_numpy(h.view(np.uint8)))

    def lrs(self):
        """[F] float64: every fit's current learning rate (lr0 * gamma^steps while above the floor) -- forces a device sync."""
        return self.hyper.cpu().numpy().view(self._hyper_dtype)["lr"].copy()

    def init_params(self):
        """Per fit f as SiblingEngine.init_params with sample f of the UNIFORM streams (init='shared': every fit starts from fit 0's)."""
        lib, sp = L.lib(), L.stream_ptr()
        n = self.n_vi
        self._pbuf.zero_()
        for f in range(self.F if self.init == "per_fit" else 1):
            mu = self._pbuf[f]
            for lid, lay in enumerate(self.prog.layers):
                bound = 1.0 / math.sqrt(lay["cin"] * lay["k"] * lay["k"])
                cnt = lay["cout"] * lay["cin"] * lay["k"] * lay["k"] + (lay["cout"] if lay["b_off"] >= 0 else 0)
                L.check(lib.mfvi_uniform_fill_range(self.seed, 16 + lid, f, 0, cnt, -bound, bound, L.ptr(mu[lay["w_off"]:]), sp))
            L.check(lib.mfvi_uniform_fill(self.seed, 0, f, 0, self.z0[f].numel(), 0.1, L.ptr(self.z0[f]), sp))
        for b in self.prog.bns:
            self._pbuf[:, 2 * n + b["off"]:2 * n + b["off"] + b["C"]] = 1.0
        if self.init == "shared":
            self._pbuf[1:] = self._pbuf[:1]; self.z0[1:] = self.z0[:1]
        self._mbuf.zero_(); self._vbuf.zero_(); self.dead_dev.zero_(); self.t = 0; self._ema_n = 0
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

    # -------------------------------------------------------------------------------------------
    def _wait_ema(self):
        if self._ema_done is not None:
            self.torch.cuda.current_stream().wait_event(self._ema_done)

    def _ema(self):
        """The smoothed outputs of every fit from self.out, on a second stream behind the forward and beside the backward pass."""
        t = self.torch
        if self._side is None:
            self._side = t.cuda.Stream(); self._ema_done = t.cuda.Event()
        ready = t.cuda.Event(); ready.record(t.cuda.current_stream())
        with t.cuda.stream(self._side):
            self._side.wait_event(ready)
            if self._book is None:
                L.check(L.lib().mfvi_ema_fits(L.ptr(self.out), self.F, self.K, 2, self.H, self.W, L.ptr(self.ema), EXP_WEIGHT, int(self._ema_n == 0),
                                              L.stream_ptr()))
            else:                        # the same EMA from mfvi_bookkeep_fits, and the iteration's records (batchbook.BatchBook)
                self._book.iteration(self.out, self.K, self._ema_n == 0)
            self._ema_done.record(self._side)
        self._ema_n += 1

    def track(self, gt, num_iter, noisy=None):
        """Record what the single-fit runner records per iteration, for every fit -> the BatchBook; step() then
        runs its iteration where the EMA runs."""
        from .batchbook import BatchBook
        return BatchBook(self, num_iter, gt, noisy)

    def metrics(self, gt):
        """dict(psnr=[F], ssim=[F]) of recon() against the ground truth ([H, W] shared, or [F, H, W]), one mfvi_pair_metrics call."""
        from .batchbook import recon_metrics
        return recon_metrics(self, gt)

    def add_noise(self, step=None):
        """SGLD's add_noise on the conv weights of every live fit: std = param_noise_sigma * lr0[f], one launch."""
        step = self.t if step is None else int(step)
        L.check(L.lib().mfvi_add_normal_fits(L.ptr(self._pbuf), self.stride, self.F, 0, L.ptr(self.layer_off), L.ptr(self.layer_n), self.layer_n.numel(),
                                             self.seed, step, L.ptr(self.noise_std), L.ptr(self.dead_dev), L.stream_ptr()))

    def grad_only(self, step=None, perturb=True, ema=False):
        """Everything of one iteration except the noise and the update: grads [F, n_params] and loss_acc [F] hold the result."""
        if self.targets is None:
            raise ValueError("set_targets first")
        lib, sp = L.lib(), L.stream_ptr()
        step = self.t if step is None else int(step)
        F, K = self.F, self.K
        self._gbuf.zero_()
        zsrc = self.z0
        if perturb:
            L.check(lib.mfvi_perturb_input_fits(L.ptr(self.z0), self.seed, step, self.z0[0].numel(), F, 0, 0.1, L.ptr(self.z), sp))
            zsrc = self.z
        self._wait_ema()                 # the previous iteration's EMA has read self.out
        p0 = self._pbuf[0]
        mu, rho, bn = p0[:self.n_vi], p0[self.n_vi:], p0[2 * self.n_vi:]
        g0 = self._grows[0]
        self.plan.forward(mu, rho, bn, zsrc, self.seed, step, 0, self.n, False, self.out)
        f = self.sr_factor if self.task == "sr" else 1
        if self.mse_image:
            L.check(lib.mfvi_mse_channel_fits(L.ptr(self.out), L.ptr(self.targets), self.targets[0].numel(), F, K, 2, self.H, self.W, 0, f, 1.0 / K,
                                              L.ptr(self.dout), L.ptr(self.loss_acc), sp))
        else:
            L.check(lib.mfvi_gaussian_nll_fits(L.ptr(self.out), L.ptr(self.targets), self.targets[0].numel(), F, K, self.H, self.W, f, 1.0 / K,
                                               L.ptr(self.dout), L.ptr(self.loss_acc), sp))
        if ema:
            self._ema()
        self.plan.backward(mu, rho, bn, zsrc, self.seed, step, 0, self.n, self.dout, g0[:self.n_vi], g0[self.n_vi:], g0[2 * self.n_vi:], False)

    def step(self):
        """One iteration of every fit.  A fit whose data term is not finite keeps its parameters, moments and lr and is marked dead."""
        lib, sp = L.lib(), L.stream_ptr()
        if self.method == "sgld":
            self.add_noise(self.t)
        self.grad_only(self.t, ema=True)
        self.t += 1
        L.check(lib.mfvi_sibling_update_fits(L.ptr(self._pbuf), L.ptr(self._grows), L.ptr(self._mbuf), L.ptr(self._vbuf), self.n_vi, self.n_bn, self.stride,
                                             self.stride, self.F, L.ptr(self.hyper), 0.9, 0.999, 1e-8, self.t, L.ptr(self.loss_acc), L.ptr(self.dead_dev), sp))

    # -------------------------------------------------------------------------------------------
    def losses(self):
        """[F]: the data term of the last step (mean over the fit's K samples) -- forces a device sync."""
        return self.loss_acc.cpu().numpy() / self.K

    @property
    def dead(self):
        """[F] int32: 1 for a fit that met a non-finite data term (sticky; its parameters stopped there)."""
        return self.dead_dev.cpu().numpy()

    def recon(self):
        """clip(ema[:, 0], 0, 1) [F, H, W]: the smoothed reconstruction of every fit."""
        self._wait_ema()
        return self.ema[:, 0].clamp(0.0, 1.0).contiguous()

    def psnr(self, gt):
        """[F]: PSNR of clip(ema[:, 0], 0, 1) against the ground truth ([H, W] shared, or [F, H, W]): the psnr_gt_sm the reference returns to
        its search (bayesian_optimization.py:1220-1223, :1237)."""
        import numpy as np
        torch, lib, sp = self.torch, L.lib(), L.stream_ptr()
        g = torch.as_tensor(gt).float().cuda()
        if g.dim() == 2:
            g = g[None].expand(self.F, -1, -1)
        if tuple(g.shape) != (self.F, self.H, self.W):
            raise ValueError("ground truth of shape %s, expected %s" % (tuple(g.shape), (self.F, self.H, self.W)))
        g = g.contiguous()
        rec = self.recon()
        acc = torch.zeros(self.F, dtype=torch.float64, device="cuda")
        for f in range(self.F):
            L.check(lib.mfvi_sq_err_sum(L.ptr(g[f]), L.ptr(rec[f]), self.H * self.W, L.ptr(acc[f:]), sp))
        mse = acc.cpu().numpy() / float(self.H * self.W)
        with np.errstate(divide="ignore"):
            return 10.0 * np.log10(1.0 / mse)

    def predict(self, n_samples, target=None, clip=False, step=None, chunk=None, fits_per_call=None, calibration=None):
        """Posterior predictive maps of every fit at once (batchpredict.predict_fits): per fit what
        to_engine(f).predict(n_samples, ...) returns, stacked, from one set of launches per chunk of draws instead of one chain per fit."""
        from .batchpredict import predict_fits
        return predict_fits(self, n_samples, target=target, clip=clip, step=step, chunk=chunk, fits_per_call=fits_per_call, calibration=calibration)

    def to_engine(self, f, autotune=False):
        """A SiblingEngine holding copies of fit f's parameters, Adam moments, step count, current lr, lr0, dropout_p, input and target:
        predict() (MC dropout) and the single-fit runner then work on any fit of a batch.  (Continued alone it draws the dropout masks of
        the global samples 0 .. K - 1 and sample 0 of the noise streams, not fit f's.)"""
        from .engine import SiblingEngine
        if not 0 <= f < self.F:
            raise ValueError("fit %r outside 0..%d" % (f, self.F - 1))
        eng = SiblingEngine(self.H, self.W, method=self.method, task=self.task, weight_decay=self.weight_decays[f], dropout_p=self.dropout_ps[f],
                            gamma=self.gammas[f], param_noise_sigma=self.param_noise_sigma, net_kwargs=self.net_kwargs, K=self.K,
                            input_depth=self.input_depth, lr=self.lr0s[f], seed=self.seed, sr_factor=self.sr_factor, autotune=autotune)
        v = self.fit(f)
        eng.params.copy_(v["params"]); eng.m.copy_(v["m"]); eng.v.copy_(v["v"]); eng.z0.copy_(v["z0"])
        eng.t = self.t; eng.t_applied.fill_(self.t)
        eng.lr = float(self.lrs()[f]); eng.lr0 = self.lr0s[f]
        if self.targets is not None:
            eng.set_target(self.targets[f].clone())
        return eng
