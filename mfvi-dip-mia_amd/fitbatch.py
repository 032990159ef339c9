"""Many independent MFVI fits advanced by ONE iteration of launches.

The reference runs its (temp, sigma) candidates and the slices of a volume as one process per fit, each a chain of small K = 1
launches that leave most of an MI355X idle (bayesian_optimization.py:3760-3775, :1360-1372).  A FitBatch of F fits with K samples
each is one plan of F * K samples in fits mode (mfvi_plan_set_fits): sample i belongs to fit i // K, reads that fit's mu / rho / BN
block and input, and its gradient is reduced into that fit's row.  One iteration is the one-group iteration of rowbatch.py (perturb,
forward, data term, EMA on a second stream beside the backward pass, backward, then KL and Adam with temp[f], prior_sigma[f], lr[f]) with

    nll[f] = 1/K sum_k NLL(out[f, k], target[f])                                       (mfvi_gaussian_nll_fits)

as its data term, whatever F is.  RNG identity: fit f owns the global samples f * K .. f * K + K - 1 of eps and sample f of the INIT, z0 and input
perturbation domains, so fit 0 of a batch is the standalone ElboEngine(seed, K)."""
from . import _lib as L
from .rowbatch import EXP_WEIGHT, TASKS, ElboRowBatch, check_kl_type, check_prior_mixtures, per_fit, prior_sigmas      # (re-exported: the helpers' home is rowbatch.py)


def check_args(H, W, n_fits, task, K, temp, sigma, lr, init):
    """Everything that can be refused without the library; -> (temps, sigmas, lrs)."""
    if task in ("ct", "inp"):
        raise NotImplementedError("FitBatch serves denoising and super-resolution; the data terms of task %r are not batched" % (task,))
    if task not in TASKS:
        raise ValueError("task %r: 'den' or 'sr'" % (task,))
    if int(n_fits) < 1 or int(K) < 1 or int(n_fits) * int(K) > 65535:
        raise ValueError("n_fits=%r, K=%r: at least 1 each, n_fits * K < 65536" % (n_fits, K))
    if H < 1 or W < 1 or H % 4 or W % 4:
        raise ValueError("H=%r, W=%r: multiples of 4 (the input-scale layers run on the matrix-core kernels)" % (H, W))
    if init not in ("per_fit", "shared"):
        raise ValueError("init %r: 'per_fit' or 'shared'" % (init,))
    temps, sigmas, lrs = per_fit(temp, n_fits, "temp"), per_fit(sigma, n_fits, "sigma"), per_fit(lr, n_fits, "lr")
    if any(not t >= 0.0 for t in temps) or any(not s >= 0.0 for s in sigmas) or any(not r > 0.0 for r in lrs):
        raise ValueError("temp and sigma must be >= 0 and lr > 0 for every fit")
    return temps, sigmas, lrs


class FitBatch(ElboRowBatch):
    """The one-group ElboRowBatch of denoising / super-resolution fits: rowbatch.py runs the iteration; here are the targets, the data term
    and the engine of one fit."""
    targets = None

    def __init__(self, H, W, n_fits, task="den", K=1, input_depth=16, temp=1.0, sigma=0.1, lr=1e-3, seed=1, sr_factor=4, net_kwargs=None,
                 init="per_fit", autotune=True, tv_weight=0.0, tv_beta=0.5, kl_type="reverse", prior_mixture=None):
        self.temps, self.sigmas, self.lrs = check_args(H, W, n_fits, task, K, temp, sigma, lr, init)
        self.kl_types = check_kl_type(kl_type, int(n_fits))      # a name, or one per fit: one batch can run both directions on one image
        self.prior_mixtures = check_prior_mixtures(prior_mixture, self.kl_types)      # None, one scale-mixture prior, or one per fit (None: a Gaussian row)
        from .tv import check_tv
        self.tv_weights, self.tv_beta = check_tv(tv_weight, tv_beta, task, n=int(n_fits))      # a scalar, or one weight per fit
        if task == "sr" and (sr_factor < 1 or H % sr_factor or W % sr_factor):
            raise ValueError("sr_factor %r does not divide %dx%d" % (sr_factor, H, W))
        self.task, self.F, self.sr_factor = task, int(n_fits), int(sr_factor)
        self.net_kwargs = dict(net_kwargs or {})
        self._allocate(n_fits, n_fits, K, H, W, 2, input_depth, self.net_kwargs, seed, init, autotune)

    def set_targets(self, targets):
        """den: the noisy images [F, H, W]; sr: the low-resolution images [F, H / f, W / f]."""
        t = self.torch.as_tensor(targets)
        f = self.sr_factor if self.task == "sr" else 1
        if tuple(t.shape) != (self.F, self.H // f, self.W // f):
            raise ValueError("targets of shape %s, expected %s" % (tuple(t.shape), (self.F, self.H // f, self.W // f)))
        self.targets = t.contiguous().float().cuda()

    def _require_targets(self):
        if self.targets is None:
            raise ValueError("set_targets first")

    def _data_term(self, d0, nd, out, dout):      # one group: d0 = 0, nd = F
        L.check(L.lib().mfvi_gaussian_nll_fits(L.ptr(out), L.ptr(self.targets), self.targets[0].numel(), nd, self.K, self.H, self.W,
                                               self.sr_factor if self.task == "sr" else 1, 1.0 / self.K, L.ptr(dout), L.ptr(self.nll_acc),
                                               L.stream_ptr()))

    def _make_engine(self, f, autotune):
        from .engine import ElboEngine
        return ElboEngine(self.H, self.W, task=self.task, K=self.K, input_depth=self.input_depth, temp=self.temps[f], sigma=self.sigmas[f],
                          lr=self.lrs[f], seed=self.seed, sr_factor=self.sr_factor, net_kwargs=self.net_kwargs, autotune=autotune, **self._tv_kw(f), **self._kl_kw(f))

    def _hand_target(self, eng, f):
        if self.targets is not None:
            eng.set_target(self.targets[f].clone())
