"""The slices of a sparse-view CT volume fitted in one set of launches.

The reference fits a CT stack as one run_ct_mfvi process per slice (bayesian_optimization.py:442-648), each iteration a chain of small
K = 1 launches.  A CtVolume of D slices holds one parameter / moment / gradient row per slice, laid out as FitBatch lays out its rows, and
ONE plan of F * K samples in fits mode (F = slices_per_launch).  The slices advance in groups of F through that plan and its workspace --
a stack of 100 slices does not fit one launch set's activations --, the last group with what is left.  One iteration of group g is

    z[d]   = z0[d] + 0.1 * N(0,1)                 RNG domain INPUT, sample d          (mfvi_perturb_input_fits, fit0 = g F)
    out    = net(z)                                eps of global sample d * K + k      (mfvi_forward, fits mode, k0 = g F K)
    nll[d] = 1/K sum_k mean((R out[d, k] - sino[d])^2)                                 (mfvi_radon_mse_fits)
    ema[d]                                         on a second stream beside the backward pass (mfvi_ema_fits, C = 1)
    grads                                                                              (mfvi_backward, fits mode)

and one mfvi_elbo_update_fits over all D rows closes the iteration (KL[d], Adam with temp[d], prior_sigma[d], lr[d]).  RNG identity: slice d
owns the global eps samples d * K .. d * K + K - 1 and sample d of the INIT, z0 and perturbation streams whatever slices_per_launch is, so
slice 0 is ElboEngine(S, S, task="ct", seed, K)."""
from . import _lib as L
from .fitbatch import EXP_WEIGHT, per_fit, prior_sigmas
from .program import skip_program

MAX_LAUNCH = 65535      # samples of one launch, and rows of one update launch (a grid dimension)


def groups(n_slices, slices_per_launch, K):
    """The launch groups of a volume, a pure function: [(first slice, slices, k0, fit0, samples)] -- group g starts at slice g F, draws eps
    from global sample k0 = g F K on, perturbs with the INPUT samples fit0 = g F .., and the last group holds what is left."""
    D, F, K = int(n_slices), int(slices_per_launch), int(K)
    if D < 1 or F < 1 or K < 1:
        raise ValueError("n_slices=%r, slices_per_launch=%r, K=%r: at least 1 each" % (n_slices, slices_per_launch, K))
    return [(d0, min(F, D - d0), d0 * K, d0, min(F, D - d0) * K) for d0 in range(0, D, F)]


def check_args(S, n_slices, slices_per_launch, K, temp, sigma, lr, theta_deg, init):
    """Everything that can be refused without the library; -> (S, F, temps, sigmas, lrs, theta list)."""
    try:
        H, W = S
    except TypeError:
        H = W = S
    if H != W:
        raise ValueError("size %r: the Radon operator takes square slices" % (S,))
    H = int(H)
    if H < 1 or H % 4:
        raise ValueError("S=%r: a multiple of 4 (the input-scale layers run on the matrix-core kernels)" % (S,))
    if int(n_slices) < 1 or int(n_slices) > MAX_LAUNCH:
        raise ValueError("n_slices=%r: 1 .. %d" % (n_slices, MAX_LAUNCH))
    if int(K) < 1:
        raise ValueError("K=%r: at least 1" % (K,))
    if slices_per_launch is not None and int(slices_per_launch) < 1:
        raise ValueError("slices_per_launch=%r: None (all slices) or at least 1" % (slices_per_launch,))
    D = int(n_slices)
    F = min(int(slices_per_launch) if slices_per_launch else D, D)
    if F * int(K) > MAX_LAUNCH:
        raise ValueError("slices_per_launch * K = %d * %d: below 65536 samples per launch" % (F, K))
    if init not in ("per_fit", "shared"):
        raise ValueError("init %r: 'per_fit' or 'shared'" % (init,))
    temps, sigmas, lrs = per_fit(temp, D, "temp"), per_fit(sigma, D, "sigma"), per_fit(lr, D, "lr")
    if any(not t >= 0.0 for t in temps) or any(not s >= 0.0 for s in sigmas) or any(not r > 0.0 for r in lrs):
        raise ValueError("temp and sigma must be >= 0 and lr > 0 for every slice")
    theta = [float(t) for t in (range(0, 180, 4) if theta_deg is None else theta_deg)]      # bayesian_optimization.py:545
    if not theta or len(theta) > 32768:
        raise ValueError("theta_deg: 1 .. 32768 angles, got %d" % len(theta))
    return H, F, temps, sigmas, lrs, theta


class CtVolume:
    _book = None            # a BatchBook once track()ed

    def __init__(self, S, n_slices, slices_per_launch=None, K=1, input_depth=16, temp=1.0, sigma=0.1, lr=1e-3, theta_deg=None, seed=1,
                 net_kwargs=None, init="per_fit", autotune=True):
        self.S, self.F, self.temps, self.sigmas, self.lrs, self.theta_list = check_args(S, n_slices, slices_per_launch, K, temp, sigma, lr,
                                                                                        theta_deg, init)
        import numpy as np
        import torch
        self.torch = torch
        S = self.S
        self.D, self.K, self.T = int(n_slices), int(K), len(self.theta_list)
        self.seed, self.input_depth, self.init = int(seed), int(input_depth), init
        self.net_kwargs = dict(net_kwargs or {})
        self.prior_sigma = prior_sigmas(self.temps, self.sigmas)
        self.groups = groups(self.D, self.F, self.K)
        self.prog, self.zin, self.zout, self.names = skip_program(S, S, input_depth, 1, **self.net_kwargs)      # the CT net: n_channels = 1
        D, F, K, P = self.D, self.F, self.K, self.prog
        self.n = F * K
        self.plan = P.compile(self.zin, self.zout, self.n)
        self.n_vi, self.n_bn = P.n_vi, P.n_bn
        self.n_params = 2 * P.n_vi + P.n_bn
        self.stride = (self.n_params + 3) // 4 * 4                   # as FitBatch: every slice's MU block 16-byte aligned
        dev = "cuda"
        self._pbuf = torch.zeros((D, self.stride), dtype=torch.float32, device=dev)
        self._mbuf = torch.zeros_like(self._pbuf); self._vbuf = torch.zeros_like(self._pbuf)
        self.params, self.m, self.v = self._pbuf[:, :self.n_params], self._mbuf[:, :self.n_params], self._vbuf[:, :self.n_params]
        # gradients and the float64 data-term accumulators of ALL slices in one allocation: one fill launch clears both per iteration
        self._gbuf = torch.zeros(4 * D * self.stride + 8 * D, dtype=torch.uint8, device=dev)
        self._grows = self._gbuf[:4 * D * self.stride].view(torch.float32).view(D, self.stride)
        self.grads = self._grows[:, :self.n_params]
        self.nll_acc = self._gbuf[4 * D * self.stride:].view(torch.float64)
        self.kl = torch.zeros(D, dtype=torch.float64, device=dev)
        self.dead_dev = torch.zeros(D, dtype=torch.int32, device=dev)
        self.hyper = torch.tensor(np.array([[0.0, ps, t, r] for ps, t, r in zip(self.prior_sigma, self.temps, self.lrs)], np.float32), device=dev)   # mfvi_fit_hyper[D]
        self.theta = torch.tensor(self.theta_list, dtype=torch.float32, device=dev)
        self.z0 = torch.empty((D, input_depth, S, S), dtype=torch.float32, device=dev)
        # what one group needs, shared by the groups like the plan's workspace
        self.z = torch.empty((F, input_depth, S, S), dtype=torch.float32, device=dev)
        self.out = torch.empty((self.n, 1, S, S), dtype=torch.float32, device=dev)
        self.dout = torch.empty_like(self.out)
        self.ct_scratch = torch.empty(L.lib().mfvi_radon_mse_fits_scratch_bytes(F, K, S, self.T), dtype=torch.uint8, device=dev)
        self.ema = torch.zeros((D, 1, S, S), dtype=torch.float32, device=dev)
        self.upd_scratch = torch.zeros(L.lib().mfvi_elbo_update_fits_scratch_bytes(D), dtype=torch.uint8, device=dev)
        self.sinos = None
        self.t = 0
        self._ema_n = 0                  # EMA updates so far (the first one copies)
        self._side = None; self._ema_done = None
        self.init_params()
        if autotune:                     # before the mode is switched on (tilings do not depend on it), with slice 0's parameters and input
            f0 = self.fit(0)
            self.plan.autotune(f0["mu"], f0["rho"], f0["bn"], self.z0[0], self.n)
        self.plan.set_fits(K, self.stride, self.stride)

    # -------------------------------------------------------------------------------------------
    def fit(self, d):
        """Views of slice d: dict(mu, rho, bn, params, m, v, grads, z0, ema)."""
        n = self.n_vi
        p = self._pbuf[d]
        return dict(mu=p[:n], rho=p[n:2 * n], bn=p[2 * n:self.n_params], params=p[:self.n_params], m=self._mbuf[d, :self.n_params],
                    v=self._vbuf[d, :self.n_params], grads=self._grows[d, :self.n_params], z0=self.z0[d], ema=self.ema[d])

    def init_params(self):
        """Per slice d as ElboEngine.init_params with sample d of the INIT / z0 streams (init='shared': every slice starts from slice 0's)."""
        lib, sp = L.lib(), L.stream_ptr()
        n = self.n_vi
        self._pbuf.zero_()
        for d in range(self.D if self.init == "per_fit" else 1):
            p = self._pbuf[d]
            L.check(lib.mfvi_normal_fill(self.seed, L.DOMAIN_INIT, 0, d, 0, n, 0.0, 0.1, L.ptr(p), sp))
            L.check(lib.mfvi_normal_fill(self.seed, L.DOMAIN_INIT, 1, d, 0, n, -3.0, 0.1, L.ptr(p[n:]), sp))
            L.check(lib.mfvi_uniform_fill(self.seed, 0, d, 0, self.z0[d].numel(), 0.1, L.ptr(self.z0[d]), sp))
        for b in self.prog.bns:
            self._pbuf[:, 2 * n + b["off"]:2 * n + b["off"] + b["C"]] = 1.0
        if self.init == "shared":
            self._pbuf[1:] = self._pbuf[:1]; self.z0[1:] = self.z0[:1]
        self._mbuf.zero_(); self._vbuf.zero_(); self.dead_dev.zero_(); self.t = 0; self._ema_n = 0

    def set_sinograms(self, sinos):
        """The measured sinograms [D, T, S], one per slice."""
        s = self.torch.as_tensor(sinos)
        if tuple(s.shape) != (self.D, self.T, self.S):
            raise ValueError("sinograms of shape %s, expected %s" % (tuple(s.shape), (self.D, self.T, self.S)))
        self.sinos = s.contiguous().float().cuda()

    def set_volume(self, volume):
        """The sinograms of a ground-truth stack [D, S, S] by mfvi_radon_project, as the reference makes img_radon
        (bayesian_optimization.py:547)."""
        torch = self.torch
        v = torch.as_tensor(volume)
        if tuple(v.shape) != (self.D, self.S, self.S):
            raise ValueError("volume of shape %s, expected %s" % (tuple(v.shape), (self.D, self.S, self.S)))
        v = v.contiguous().float().cuda()
        sinos = torch.empty((self.D, self.T, self.S), dtype=torch.float32, device="cuda")
        L.check(L.lib().mfvi_radon_project(L.ptr(v), L.ptr(self.theta), self.D, self.S, self.T, L.ptr(sinos), L.stream_ptr()))
        self.sinos = sinos

    # -------------------------------------------------------------------------------------------
    def _wait_ema(self):
        if self._ema_done is not None:
            self.torch.cuda.current_stream().wait_event(self._ema_done)

    def _ema(self, d0, nd):
        """The smoothed outputs of the group's slices from self.out, on a second stream behind the forward and beside the backward pass."""
        t = self.torch
        if self._side is None:
            self._side = t.cuda.Stream(); self._ema_done = t.cuda.Event()
        ready = t.cuda.Event(); ready.record(t.cuda.current_stream())
        with t.cuda.stream(self._side):
            self._side.wait_event(ready)
            if self._book is None:
                L.check(L.lib().mfvi_ema_fits(L.ptr(self.out), nd, self.K, 1, self.S, self.S, L.ptr(self.ema[d0:]), EXP_WEIGHT, int(self._ema_n == 0),
                                              L.stream_ptr()))
            else:                        # the same EMA from mfvi_bookkeep_fits; behind the last group, the iteration's records of every slice
                self._book.group(self.out, d0, nd, self.K, self._ema_n == 0)
                if d0 + nd == self.D:
                    self._book.finish()
            self._ema_done.record(self._side)

    def track(self, gt, num_iter, noisy=None):
        """Record what the single-fit CT runner records per iteration, for every slice -> the BatchBook; step() then
        runs its iteration where the EMA runs.  gt: the stack [D, S, S] (or one [S, S] slice for all); noisy stays None (both
        'corrupted' columns of the CT runner are against the ground truth)."""
        from .batchbook import BatchBook
        return BatchBook(self, num_iter, gt, noisy)

    def metrics(self, gt):
        """dict(psnr=[D], ssim=[D]) of recon() against the ground truth ([S, S] shared, or [D, S, S]), one mfvi_pair_metrics call."""
        from .batchbook import recon_metrics
        return recon_metrics(self, gt)

    def grad_only(self, step=None, perturb=True, ema=False):
        """Everything of one iteration except the update, group by group: grads [D, n_params] and nll_acc [D] hold the result (no KL term)."""
        if self.sinos is None:
            raise ValueError("set_sinograms or set_volume first")
        lib, sp = L.lib(), L.stream_ptr()
        step = self.t if step is None else int(step)
        K, S, nv = self.K, self.S, self.n_vi
        self._gbuf.zero_()
        for d0, nd, k0, fit0, n in self.groups:
            zsrc = self.z0[d0:d0 + nd]
            if perturb:
                zsrc = self.z[:nd]
                L.check(lib.mfvi_perturb_input_fits(L.ptr(self.z0[d0:]), self.seed, step, self.z0[0].numel(), nd, fit0, 0.1, L.ptr(zsrc), sp))
            self._wait_ema()             # the EMA of the previous group (or iteration) has read self.out
            p, g = self._pbuf[d0], self._grows[d0]
            mu, rho, bn = p[:nv], p[nv:], p[2 * nv:]
            out, dout = self.out[:n], self.dout[:n]
            self.plan.forward(mu, rho, bn, zsrc, self.seed, step, k0, n, True, out)
            L.check(lib.mfvi_radon_mse_fits(L.ptr(out), L.ptr(self.sinos[d0:]), self.T * S, L.ptr(self.theta), nd, K, S, self.T, 1.0 / K,
                                            L.ptr(self.ct_scratch), L.ptr(dout), L.ptr(self.nll_acc[d0:]), sp))
            if ema:
                self._ema(d0, nd)
            self.plan.backward(mu, rho, bn, zsrc, self.seed, step, k0, n, dout, g[:nv], g[nv:], g[2 * nv:], True)
        if ema:
            self._ema_n += 1

    def step(self):
        """One ELBO iteration of every slice.  A slice whose data term is not finite keeps its parameters and moments and is marked dead
        (sticky); the reference instead skips that one update (`if not torch.isnan(loss)`, bayesian_optimization.py:581-582)."""
        lib, sp = L.lib(), L.stream_ptr()
        self.grad_only(self.t, ema=True)
        self.t += 1
        L.check(lib.mfvi_elbo_update_fits(L.ptr(self._pbuf), L.ptr(self._grows), L.ptr(self._mbuf), L.ptr(self._vbuf), self.n_vi, self.n_bn, self.stride,
                                          self.stride, self.D, L.ptr(self.hyper), 0.9, 0.999, 1e-8, self.t, L.ptr(self.nll_acc), L.ptr(self.dead_dev),
                                          L.ptr(self.kl), L.ptr(self.upd_scratch), sp))

    # -------------------------------------------------------------------------------------------
    def losses(self):
        """(nll[D], kl[D], loss[D]) of the last step (kl: of the parameters that step started from) -- forces a device sync.
        After grad_only alone kl is stale: the KL term is part of the update launch."""
        import numpy as np
        nll = self.nll_acc.cpu().numpy() / self.K
        kl = self.kl.cpu().numpy()
        return nll, kl, nll + np.asarray(self.temps) * kl

    @property
    def dead(self):
        """[D] int32: 1 for a slice that met a non-finite data term (sticky; its parameters stopped there)."""
        return self.dead_dev.cpu().numpy()

    def recon(self):
        """clip(ema[:, 0], 0, 1) [D, S, S]: the smoothed reconstruction of the volume."""
        self._wait_ema()
        return self.ema[:, 0].clamp(0.0, 1.0).contiguous()

    def psnr(self, gt):
        """[D]: PSNR of the smoothed reconstruction against the ground-truth stack [D, S, S] -- per slice the psnr_gt_sm the reference returns."""
        import numpy as np
        torch, lib, sp = self.torch, L.lib(), L.stream_ptr()
        g = torch.as_tensor(gt).float().cuda()
        if tuple(g.shape) != (self.D, self.S, self.S):
            raise ValueError("ground truth of shape %s, expected %s" % (tuple(g.shape), (self.D, self.S, self.S)))
        g = g.contiguous()
        rec = self.recon()
        acc = torch.zeros(self.D, dtype=torch.float64, device="cuda")
        for d in range(self.D):
            L.check(lib.mfvi_sq_err_sum(L.ptr(g[d]), L.ptr(rec[d]), self.S * self.S, L.ptr(acc[d:]), sp))
        mse = acc.cpu().numpy() / float(self.S * self.S)
        with np.errstate(divide="ignore"):
            return 10.0 * np.log10(1.0 / mse)

    def predict(self, n_samples, target=None, clip=False, step=None, chunk=None, fits_per_call=None, calibration=None):
        """Posterior predictive maps of every slice at once (batchpredict.predict_fits): per slice what
        to_engine(d).predict(n_samples, ...) returns, stacked, from one set of launches per chunk of draws instead of one chain per slice."""
        from .batchpredict import predict_fits
        return predict_fits(self, n_samples, target=target, clip=clip, step=step, chunk=chunk, fits_per_call=fits_per_call, calibration=calibration)

    def to_engine(self, d, autotune=False):
        """A CT ElboEngine holding copies of slice d's parameters, Adam moments, step count, input, angles and sinogram: predict() and
        calibration work on any slice of a volume.  (Continued alone it draws eps of the global samples 0 .. K - 1, not d * K ..)"""
        from .engine import ElboEngine
        if not 0 <= d < self.D:
            raise ValueError("slice %r outside 0..%d" % (d, self.D - 1))
        eng = ElboEngine(self.S, self.S, task="ct", K=self.K, input_depth=self.input_depth, temp=self.temps[d], sigma=self.sigmas[d],
                         lr=self.lrs[d], seed=self.seed, theta_deg=self.theta_list, net_kwargs=self.net_kwargs, autotune=autotune)
        v = self.fit(d)
        eng.params.copy_(v["params"]); eng.m.copy_(v["m"]); eng.v.copy_(v["v"]); eng.z0.copy_(v["z0"])
        eng.t = self.t; eng.t_applied.fill_(self.t)
        if self.sinos is not None:
            eng.set_target(self.sinos[d].clone())
        return eng
