"""radon/radon.py:23-55 (FastRadonTransform) restated in float64 numpy as a rotation about the image centre, shared
by the Radon drop-in tests and scripts/make_radon_golden.py.

With m = (S - 1) / 2, th = float32(theta_deg) * float32(pi / 180), c = float32(cos(th)), s = float32(sin(th)), detector bin j and row i
sample the image at ix = c (j - m) - s (i - m) + m, iy = s (j - m) + c (i - m) + m, bilinear with zero padding, and
sino[t][j] = sum_i sample(ix, iy).  The angle is rounded to float32 exactly where the reference rounds it; everything after is float64."""
import numpy as np

# (name, S, C, theta in degrees or None for the reference's default arange(180.)): the cases of tests/golden/radon_dropin.npz
CASES = [
    ("lattice8", 8, 1, (0.0, 45.0, 90.0)),                           # lattice angles: samples land on integers
    ("odd33", 33, 1, None),                                          # odd size: the centre is a pixel; the default 180 angles
    ("wide20", 20, 1, (-30.0, 10.0, 200.0)),                         # angles outside [0, 180)
    ("planes40", 40, 3, tuple(np.arange(0.0, 180.0, 4.0))),          # several planes, a strip that is no multiple of 64
]
CTOR_CASE = "wide20"                                                 # the case whose constructor buffers are recorded


def theta_of(case):
    th = case[3]
    return np.arange(180.0, dtype=np.float32) if th is None else np.asarray(th, np.float32)


def relerr(a, b):
    """The project's relative error: max |a - b| / max |b|."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def rotation(theta_deg):
    """(c, s) float64 [T]: cos and sin of the float32 angle, each rounded once to float32."""
    th = np.asarray(theta_deg, np.float32).reshape(-1) * np.float32(0.017453292519943295)
    th = th.astype(np.float32).astype(np.float64)
    return np.cos(th).astype(np.float32).astype(np.float64), np.sin(th).astype(np.float32).astype(np.float64)


def _samples(S, c, s):
    """For one angle: the four neighbours (flat index into the zero-padded (S + 2)^2 image) and weights of every sample, each [4][S][S]
    indexed [neighbour][row i][bin j]."""
    m = (S - 1) / 2.0
    i, j = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    ix = c * (j - m) - s * (i - m) + m
    iy = s * (j - m) + c * (i - m) + m
    x0, y0 = np.floor(ix), np.floor(iy)
    lx, ly = ix - x0, iy - y0
    idx, w = [], []
    for dy, wy in ((0, 1.0 - ly), (1, ly)):
        for dx, wx in ((0, 1.0 - lx), (1, lx)):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < S) & (yy >= 0) & (yy < S)
            idx.append(np.where(ok, (yy + 1) * (S + 2) + xx + 1, 0).astype(np.int64))        # 0: a padding pixel
            w.append(np.where(ok, wx * wy, 0.0))
    return np.stack(idx), np.stack(w)


def forward64(img, theta_deg):
    """img [..., S, S] -> sino float64 [..., T, S]."""
    img = np.asarray(img, np.float64)
    S = img.shape[-1]
    assert img.shape[-2] == S
    planes = img.reshape(-1, S, S)
    pad = np.zeros((planes.shape[0], S + 2, S + 2))
    pad[:, 1:-1, 1:-1] = planes
    pad = pad.reshape(planes.shape[0], -1)
    c, s = rotation(theta_deg)
    out = np.empty((planes.shape[0], c.size, S))
    for t in range(c.size):
        idx, w = _samples(S, c[t], s[t])
        out[:, t] = (pad[:, idx] * w).sum(axis=(1, 2))
    return out.reshape(img.shape[:-2] + (c.size, S))


def adjoint64(dsino, theta_deg, S):
    """dsino [..., T, S] -> dimg float64 [..., S, S]: the transpose of forward64 (what autograd returns for the image)."""
    dsino = np.asarray(dsino, np.float64)
    c, s = rotation(theta_deg)
    assert dsino.shape[-2:] == (c.size, S)
    planes = dsino.reshape(-1, c.size, S)
    acc = np.zeros((planes.shape[0], (S + 2) * (S + 2)))
    for t in range(c.size):
        idx, w = _samples(S, c[t], s[t])
        for p in range(planes.shape[0]):
            np.add.at(acc[p], idx.ravel(), (w * planes[p, t][None, None, :]).ravel())
    acc = acc.reshape(-1, S + 2, S + 2)[:, 1:-1, 1:-1]
    return acc.reshape(dsino.shape[:-2] + (S, S))
