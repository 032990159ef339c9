"""Total-variation regulariser on the HIP kernel mfvi_tv_term.

    TV_beta(x) = sum over the cells (i < H-1, j < W-1) of (dh^2 + dw^2)^beta,   dh = x[i][j+1] - x[i][j],   dw = x[i+1][j] - x[i][j]

per plane, a sum (utils/sr_utils.py:84-94 tv_loss).  One departure: where a cell has dh = dw = 0 and beta < 1 the gradient factor is 0
here, where the reference's autograd returns NaN (inf * 0).  tv_loss is the drop-in; check_tv / TvTerm are what the engines and the
batches share."""
import math

from . import _lib as L

MAX_PLANES = 65535      # planes of one mfvi_tv_term call (a grid dimension)


def check_tv(tv_weight, tv_beta, task=None, n=None, name="tv_weight"):
    """Everything that can be refused without the library -> (weights, beta): a float (n None) or a list of n floats, and the float beta."""
    from .rowbatch import per_fit
    ws = per_fit(tv_weight, 1 if n is None else n, name)
    if n is None and len(ws) != 1:
        raise ValueError("%s: one value, got %d" % (name, len(ws)))
    if any(not (w >= 0.0 and math.isfinite(w)) for w in ws):
        raise ValueError("%s=%r: finite and >= 0" % (name, tv_weight))
    beta = float(tv_beta)
    if not (beta > 0.0 and math.isfinite(beta)):
        raise ValueError("tv_beta=%r: finite and > 0" % (tv_beta,))
    if task == "inp" and any(w > 0.0 for w in ws):
        raise ValueError("%s > 0 with task 'inp': the total-variation term is built for den / sr / ct (the inpainting colour channels "
                         "pass a sigmoid)" % name)
    return (ws[0] if n is None else ws), beta


class TvTerm:
    """The device state of the term for n_fits rows whose launches hold at most max_fits rows of S samples: the weights [n_fits] (float32),
    the accumulators [n_fits] (float64, `acc`: a caller's buffer that its own fill clears, or one allocated here) and the scratch."""

    def __init__(self, weights, beta, max_fits, S, H, W, acc=None):
        import torch
        self.beta = float(beta)
        self.weight = torch.tensor([float(w) for w in weights], dtype=torch.float32, device="cuda")
        self.acc = torch.zeros(len(weights), dtype=torch.float64, device="cuda") if acc is None else acc
        self.scratch = torch.empty(L.lib().mfvi_tv_term_scratch_bytes(int(max_fits), int(S), H, W), dtype=torch.uint8, device="cuda")

    def add(self, out, dout, d0, nd, S, grad_scale):
        """dout[:, 0] += grad_scale * weight[d0 + f] * dTV/dout[:, 0] and acc[d0 + f] += sum of TV over fit f's S samples, f < nd."""
        n, C, H, W = out.shape
        L.check(L.lib().mfvi_tv_term(L.ptr(out), nd, S, C, H, W, 0, self.beta, L.ptr(self.weight[d0:]), 1, grad_scale, 1, L.ptr(dout),
                                     L.ptr(self.acc[d0:]), L.ptr(self.scratch), L.stream_ptr()))


_fn = None


def _function():
    global _fn
    if _fn is not None:
        return _fn
    import torch

    class _TvLoss(torch.autograd.Function):
        """Value and gradient from mfvi_tv_term with n_fits = N * C planes, S = 1; the backward passes the upstream gradient as the
        device weight (stride 0): no host sync inside autograd."""

        @staticmethod
        def forward(ctx, x, beta):
            xc = x.contiguous()
            N, C, H, W = xc.shape
            acc = torch.zeros(N * C, dtype=torch.float64, device=xc.device)
            one = torch.ones(1, dtype=torch.float32, device=xc.device)
            lib, sp = L.lib(), L.stream_ptr()
            for p0 in range(0, N * C, MAX_PLANES):
                n = min(MAX_PLANES, N * C - p0)
                scratch = torch.empty(lib.mfvi_tv_term_scratch_bytes(n, 1, H, W), dtype=torch.uint8, device=xc.device)
                L.check(lib.mfvi_tv_term(L.ptr(xc.view(-1)[p0 * H * W:]), n, 1, 1, H, W, 0, beta, L.ptr(one), 0, 1.0, 0, None, L.ptr(acc[p0:]),
                                         L.ptr(scratch), sp))
            ctx.save_for_backward(xc)
            ctx.beta = beta
            return acc.sum().float()

        @staticmethod
        def backward(ctx, g):
            xc, = ctx.saved_tensors
            N, C, H, W = xc.shape
            gw = g.reshape(1).contiguous().float()
            dx = torch.empty_like(xc)
            lib, sp = L.lib(), L.stream_ptr()
            for p0 in range(0, N * C, MAX_PLANES):
                n = min(MAX_PLANES, N * C - p0)
                scratch = torch.empty(max(lib.mfvi_tv_term_scratch_bytes(n, 1, H, W), 8), dtype=torch.uint8, device=xc.device)
                L.check(lib.mfvi_tv_term(L.ptr(xc.view(-1)[p0 * H * W:]), n, 1, 1, H, W, 0, ctx.beta, L.ptr(gw), 0, 1.0, 0,
                                         L.ptr(dx.view(-1)[p0 * H * W:]), None, L.ptr(scratch), sp))
            return dx, None

    _fn = _TvLoss
    return _fn


def tv_loss(x, beta=0.5):
    """Drop-in for utils/sr_utils.py:84-94 on the HIP kernel: x a CUDA float32 [N, C, H, W] tensor -> the 0-dim differentiable sum over
    all planes of TV_beta."""
    import torch
    if not isinstance(x, torch.Tensor):
        raise TypeError("tv_loss: a torch tensor, got %s" % type(x).__name__)
    if not x.is_cuda or x.dtype != torch.float32:
        raise NotImplementedError("tv_loss runs on CUDA float32 tensors only (got %s on %s); there is no CPU path" % (x.dtype, x.device))
    if x.dim() != 4:
        raise ValueError("tv_loss: a [N, C, H, W] tensor, got shape %s" % (tuple(x.shape),))
    beta = float(beta)
    if not (beta > 0.0 and math.isfinite(beta)):
        raise ValueError("beta=%r: finite and > 0" % (beta,))
    if x.numel() == 0:
        raise ValueError("tv_loss: an empty tensor of shape %s" % (tuple(x.shape),))
    with torch.cuda.device(x.device):
        return _function().apply(x, beta)
