"""The anti-aliasing downsampler of deep-image-prior super-resolution (models/downsampler.py:6-136) on the HIP kernels of
csrc/downsample.hip.

Downsampler(n_planes, factor, 'lanczos2' | 'lanczos3', phase=0.5, preserve_size=True) is ReplicationPad2d(P) followed by a stride-`factor`
convolution of every plane with a normalised 2-D Lanczos kernel.  At half phase that kernel is the outer product of T = 2 a factor 1-D taps
(a = 2 or 3), so the operator is separable: lr = A_H . hr . A_W^T with A_N[y][clamp(y * factor + i - P, 0, N - 1)] += k1[i],
P = (T - factor) / 2.  lanczos_taps is a pure host function; the module and the engine's data term call mfvi_downsample /
mfvi_downsample_adjoint / mfvi_gaussian_nll_filtered."""
import ctypes

import numpy as np

SUPPORT = {"lanczos2": 2, "lanczos3": 3}       # models/downsampler.py:15-23
FACTORS = (2, 4, 8)                            # P = (T - factor) / 2 is an integer for even factors only
_OTHER_KERNELS = ("gauss12", "gauss1sq2", "lanczos", "gauss", "box")


def check_geometry(kernel_type, factor, H=None, W=None):
    """ValueError for what the operator is not defined (or not built) for: names, odd factors, sizes the factor does not divide."""
    if kernel_type not in SUPPORT:
        raise ValueError("downsampler %r: 'lanczos2' or 'lanczos3'" % (kernel_type,))
    if factor not in FACTORS:
        raise ValueError("downsampler factor %r: 2, 4 or 8 (the replication pad (T - factor) / 2 of the half-phase kernel is an integer "
                         "only for an even factor)" % (factor,))
    if H is not None and (H < factor or W < factor or H % factor or W % factor):
        raise ValueError("downsampler: the factor %d does not divide the map %d x %d" % (factor, H, W))


def lanczos_taps(kernel_type, factor, dtype=np.float64):
    """The T = 2 a factor 1-D taps k1 of the half-phase Lanczos kernel (get_kernel, models/downsampler.py:102-134): d_i = |i + 0.5 - T/2| /
    factor, L_i = a sin(pi d_i) sin(pi d_i / a) / (pi^2 d_i^2), k1 = L / sum(L); outer(k1, k1) is the reference's 2-D kernel."""
    check_geometry(kernel_type, factor)
    a = SUPPORT[kernel_type]
    T = 2 * a * factor
    d = np.abs(np.arange(T, dtype=np.float64) + 0.5 - T / 2.0) / factor          # never 0 at half phase
    L = a * np.sin(np.pi * d) * np.sin(np.pi * d / a) / (np.pi * np.pi * d * d)
    return (L / L.sum()).astype(dtype)


def pad_width(kernel_type, factor):
    """P of ReplicationPad2d(P) (models/downsampler.py:55-62, even kernel size)."""
    return (2 * SUPPORT[kernel_type] * factor - factor) // 2


def c_taps(kernel_type, factor):
    """(ctypes float array, n_taps): the host pointer the mfvi_downsample* entry points take."""
    k = lanczos_taps(kernel_type, factor, np.float32)
    return (ctypes.c_float * len(k))(*k.tolist()), len(k)


def downsample(x, kernel_type, factor, taps=None, out=None):
    """D(x) for a CUDA float32 tensor [..., H, W] (leading dimensions are planes) on mfvi_downsample."""
    import torch
    from . import _lib as L
    H, W = x.shape[-2:]
    check_geometry(kernel_type, factor, H, W)
    arr, T = taps or c_taps(kernel_type, factor)
    x = x.contiguous()
    planes = x.numel() // (H * W)
    if out is None:
        out = torch.empty(x.shape[:-2] + (H // factor, W // factor), dtype=torch.float32, device=x.device)
    L.check(L.lib().mfvi_downsample(L.ptr(x), 1, planes, H, W, factor, arr, T, L.ptr(out), L.stream_ptr()))
    return out


def _module():
    import torch
    from torch import nn
    from . import _lib as L

    class _DownsampleFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, mod):
            N, C, H, W = x.shape
            f = mod.factor
            ctx.mod, ctx.shape = mod, (N, C, H, W)
            y = torch.empty((N, C, H // f, W // f), dtype=torch.float32, device=x.device)
            L.check(L.lib().mfvi_downsample(L.ptr(x), N, C, H, W, f, mod._taps, mod._n_taps, L.ptr(y), L.stream_ptr()))
            return y

        @staticmethod
        def backward(ctx, gy):
            N, C, H, W = ctx.shape
            mod = ctx.mod
            gy = gy.contiguous().float()
            gx = torch.empty((N, C, H, W), dtype=torch.float32, device=gy.device)
            L.check(L.lib().mfvi_downsample_adjoint(L.ptr(gy), N, C, H, W, mod.factor, mod._taps, mod._n_taps, L.ptr(gx), L.stream_ptr()))
            return gx, None

    class Downsampler(nn.Module):
        """models/downsampler.py:6-72 with the reference's constructor arguments; built: 'lanczos2' / 'lanczos3', phase=0.5,
        preserve_size=True, on (N, C, H, W) CUDA tensors with C == n_planes.  .kernel is the 2-D numpy kernel, as the reference exposes it."""

        def __init__(self, n_planes, factor, kernel_type, phase=0.5, kernel_width=None, support=None, sigma=None, preserve_size=True):
            super().__init__()
            if kernel_type in _OTHER_KERNELS:
                raise NotImplementedError("Downsampler kernel_type=%r is not built: 'lanczos2' and 'lanczos3' are" % (kernel_type,))
            if phase not in (0, 0.5):
                raise ValueError("phase should be 0 or 0.5")                        # models/downsampler.py:13
            check_geometry(kernel_type, factor)
            if phase != 0.5:
                raise NotImplementedError("Downsampler phase=0 (the odd-sized kernel) is not built: phase=0.5 is")
            if not preserve_size:
                raise NotImplementedError("Downsampler preserve_size=False (no replication pad) is not built: preserve_size=True is")
            self.n_planes, self.factor, self.kernel_type, self.preserve_size = int(n_planes), int(factor), kernel_type, True
            k1 = lanczos_taps(kernel_type, factor)
            self.kernel = np.outer(k1, k1)
            self._taps, self._n_taps = c_taps(kernel_type, factor)

        def forward(self, input):
            if not input.is_cuda:
                raise NotImplementedError("Downsampler runs on the HIP kernels: CPU tensors are not built (there is no CPU fallback)")
            if input.dim() != 4 or input.shape[1] != self.n_planes:
                raise ValueError("Downsampler(n_planes=%d) expects (N, %d, H, W), got %s" % (self.n_planes, self.n_planes, tuple(input.shape)))
            check_geometry(self.kernel_type, self.factor, input.shape[2], input.shape[3])
            return _DownsampleFn.apply(input.contiguous().float(), self)

    return Downsampler


def __getattr__(name):          # the module class needs torch.nn: built on first use, lanczos_taps stays importable without it
    if name == "Downsampler":
        cls = _module()
        globals()["Downsampler"] = cls
        return cls
    raise AttributeError(name)
