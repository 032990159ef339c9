"""Float64 numpy statement of the total-variation term, written from its formula.

Per plane x[H][W] and every cell (i, j), i < H-1, j < W-1:
    dh = x[i][j+1] - x[i][j]      dw = x[i+1][j] - x[i][j]      u = dh^2 + dw^2
    TV_beta(x) = sum over the cells of u^beta
    dTV/dx[i][j] = g(i,j) (-dh(i,j) - dw(i,j)) + g(i,j-1) dh(i,j-1) + g(i-1,j) dw(i-1,j),      g = 2 beta u^(beta-1)
with g = 0 where u == 0 (for beta < 1 the formula's own value there is inf, and the product with the zero difference NaN).  H == 1 or
W == 1: no cell, value 0 and a zero gradient."""
import numpy as np


def cells(x):
    """dh, dw, u of every cell of the planes x[..., H, W] (float64), each [..., H-1, W-1]."""
    x = np.asarray(x, np.float64)
    c = x[..., :-1, :-1]
    dh = x[..., :-1, 1:] - c
    dw = x[..., 1:, :-1] - c
    return dh, dw, dh * dh + dw * dw


def tv_planes(x, beta=0.5):
    """TV_beta of every plane of x[..., H, W] -> [...] float64."""
    _, _, u = cells(x)
    return np.power(u, float(beta)).sum(axis=(-2, -1))


def tv_value(x, beta=0.5):
    """The sum over all planes: what tv_loss(x, beta) returns."""
    return float(tv_planes(x, beta).sum())


def tv_grad(x, beta=0.5):
    """d tv_value / dx, the shape of x, float64."""
    x = np.asarray(x, np.float64)
    beta = float(beta)
    dh, dw, u = cells(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = 2.0 * beta * np.power(u, beta - 1.0)
    g = np.where(u == 0.0, 0.0, g)
    grad = np.zeros_like(x)
    grad[..., :-1, :-1] += g * (-dh - dw)      # the cell's own pixel (i, j)
    grad[..., :-1, 1:] += g * dh               # its right neighbour (i, j+1): cell (i, j-1) seen from that pixel
    grad[..., 1:, :-1] += g * dw               # its lower neighbour (i+1, j): cell (i-1, j) seen from that pixel
    return grad


def zero_cells_touch(x):
    """Boolean mask, the shape of x: the pixels that touch a cell with u == 0 (where the unguarded formula gives NaN for beta < 1)."""
    x = np.asarray(x, np.float64)
    _, _, u = cells(x)
    z = u == 0.0
    m = np.zeros(x.shape, bool)
    m[..., :-1, :-1] |= z
    m[..., :-1, 1:] |= z
    m[..., 1:, :-1] |= z
    return m
