"""The Radon transform of the CT runners (radon/radon.py:4-55) on the HIP kernels of csrc/radon_planes.hip.

FastRadonTransform(image_size, theta=None) is the reference's module with the reference's constructor: a square image, theta in degrees
(None: torch.arange(180.)).  The reference's affine_grid + grid_sample(bilinear, zeros, align_corners=False) + sum over rows is a rotation
about the image centre, so the kernels recompute the sample positions from theta and the [T, S, S, 2] `grid` buffer of the reference is
never built; the small buffers (theta in radians, ts, tc, z, trans) are registered with the reference's names and values.  forward takes
[B, C, S, S] (the reference's expand admits B = 1 only; here every (b, c) plane is projected) and returns [B, C, T, S]; autograd's
backward is mfvi_radon_backproject of the upstream gradient."""


def radon_project(x, theta_deg, out=None):
    """sino [..., T, S] of a CUDA float32 tensor [..., S, S] (leading dimensions are planes) on mfvi_radon_project; theta_deg: CUDA float32 [T]."""
    import torch
    from . import _lib as L
    S, T = x.shape[-1], theta_deg.numel()
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape[:-2] + (T, S), dtype=torch.float32, device=x.device)
    L.check(L.lib().mfvi_radon_project(L.ptr(x), L.ptr(theta_deg), x.numel() // (S * S), S, T, L.ptr(out), L.stream_ptr()))
    return out


def radon_backproject(g, theta_deg, out=None):
    """The transpose: dimg [..., S, S] of a CUDA float32 tensor [..., T, S] on mfvi_radon_backproject."""
    import torch
    from . import _lib as L
    T, S = g.shape[-2:]
    g = g.contiguous()
    if out is None:
        out = torch.empty(g.shape[:-2] + (S, S), dtype=torch.float32, device=g.device)
    L.check(L.lib().mfvi_radon_backproject(L.ptr(g), L.ptr(theta_deg), g.numel() // (T * S), S, T, L.ptr(out), L.stream_ptr()))
    return out


def _module():
    import torch
    from torch import nn
    from torch.autograd.function import once_differentiable

    class _RadonFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, theta_deg):
            ctx.theta_deg = theta_deg
            return radon_project(x, theta_deg)

        @staticmethod
        @once_differentiable
        def backward(ctx, gy):
            return radon_backproject(gy.contiguous().float(), ctx.theta_deg), None

    class FastRadonTransform(nn.Module):
        """radon/radon.py:4-55 with the reference's constructor arguments, on (B, C, S, S) CUDA float32 tensors.  Not registered: `grid`."""

        def __init__(self, image_size, theta=None):
            super().__init__()
            image_size = tuple(int(v) for v in image_size)
            if len(image_size) != 4 or image_size[-2] != image_size[-1] or image_size[-1] < 1:
                raise ValueError("FastRadonTransform: image_size is (B, C, S, S) with a square image, got %s" % (image_size,))
            self.image_size = image_size
            deg = torch.arange(180.) if theta is None else torch.as_tensor(theta).detach().to(torch.float32).reshape(-1)
            if deg.numel() < 1:
                raise ValueError("FastRadonTransform: theta is empty")
            rad = torch.deg2rad(deg)
            ts, tc = torch.sin(rad), torch.cos(rad)
            z = torch.zeros_like(tc)
            self.register_buffer("theta", rad)
            self.register_buffer("ts", ts)
            self.register_buffer("tc", tc)
            self.register_buffer("z", z)
            self.register_buffer("trans", torch.stack((tc, -ts, z, ts, tc, z), dim=1).reshape(deg.numel(), 2, 3))
            self.register_buffer("theta_deg", deg.clone().contiguous(), persistent=False)         # what the kernels take

        def forward(self, image):
            if not image.is_cuda:
                raise NotImplementedError("FastRadonTransform runs on the HIP kernels: CPU tensors are not built (there is no CPU path)")
            if image.dtype != torch.float32:
                raise NotImplementedError("FastRadonTransform is built for float32 images, got %s" % (image.dtype,))
            if image.dim() != 4 or tuple(image.shape[-2:]) != self.image_size[-2:]:
                raise ValueError("FastRadonTransform(image_size=%s) expects (B, C, %d, %d), got %s"
                                 % (self.image_size, self.image_size[-2], self.image_size[-1], tuple(image.shape)))
            if self.theta_deg.device != image.device:
                raise ValueError("FastRadonTransform: the module is on %s and the image on %s (move the module with .to(device))"
                                 % (self.theta_deg.device, image.device))
            return _RadonFn.apply(image.contiguous(), self.theta_deg)

    return FastRadonTransform


def __getattr__(name):          # the module class needs torch.nn: built on first use
    if name == "FastRadonTransform":
        cls = _module()
        globals()["FastRadonTransform"] = cls
        return cls
    raise AttributeError(name)
