"""float64 PyTorch restatement of one inpainting ELBO iteration, shared by the InpaintBatch tests: the interpreter of a layer program with
the oracle's eps (autograd through w = mu + softplus(rho) * eps, train-mode BatchNorm, LeakyReLU, reflection pad, F.interpolate), the
masked Gaussian NLL with the sigmoid on the colour channels, the KL term of the update kernel and Adam.  A helper, not a test module."""
import numpy as np
import torch

from oracle import oracle as O

F = torch.nn.functional


def torch_program(P, zin, out_id, mu, rho, bn, z, seed, step, sample):
    """One MC sample of the layer program in float64; mu / rho / bn / z are (leaf) tensors, eps is the oracle's for global sample `sample`."""
    vals = {zin: z}

    def view(t):
        x, d = vals[t], P.tensors[t]
        if d["has_bn"]:
            c, off = d["C"], d["bn_off"]
            x = F.batch_norm(x[None], None, None, bn[off:off + c], bn[off + c:off + 2 * c], True, 0.0, d["eps"])[0]
        if d["has_act"]:
            x = F.leaky_relu(x, d["slope"])
        return x

    for op in P.ops:
        if op["type"] == 1:
            lay = P.layers[op["layer_id"]]
            cin, cout, k = lay["cin"], lay["cout"], lay["k"]
            nw = cout * cin * k * k
            ew = torch.from_numpy(O.eps(seed, step, sample, op["layer_id"], 0, nw).astype(np.float64))
            eb = torch.from_numpy(O.eps(seed, step, sample, op["layer_id"], 1, cout).astype(np.float64))
            w = (mu[lay["w_off"]:lay["w_off"] + nw] + F.softplus(rho[lay["w_off"]:lay["w_off"] + nw]) * ew).reshape(cout, cin, k, k)
            b = mu[lay["b_off"]:lay["b_off"] + cout] + F.softplus(rho[lay["b_off"]:lay["b_off"] + cout]) * eb
            x = view(op["in0"])[None]
            if k > 1:
                x = F.pad(x, (k // 2,) * 4, mode="reflect")
            vals[op["out"]] = F.conv2d(x, w, b, stride=lay["stride"])[0]
        else:
            mode = "nearest" if op["up_mode"] == 1 else "bilinear"
            up = F.interpolate(view(op["in1"])[None], scale_factor=2, mode=mode, **({} if mode == "nearest" else {"align_corners": False}))[0]
            vals[op["out"]] = up if op["in0"] < 0 else torch.cat([view(op["in0"]), up], 0)
    return vals[out_id]


def torch_inp_nll(out4, target, mask):
    mu = torch.sigmoid(out4[:3]); s = torch.clamp(out4[3:], -20, 20)
    return ((torch.exp(s) * (target - mu) ** 2 - s) * mask).mean()


def inp_grad(P, zin, zout, params, z, image, mask, seed, step, k0, K):
    """Data term of one fit: nll = 1/K sum_k NLL(net(z; eps of global sample k0 + k)) and its gradient wrt the flat row [MU | RHO | BN].
    -> dict(nll, grad [n_params] float64, out [K, 4, H, W] float64)."""
    nv = P.n_vi
    p = torch.tensor(np.asarray(params, np.float64), requires_grad=True)
    zt = torch.tensor(np.asarray(z, np.float64))
    tg, mk = torch.tensor(np.asarray(image, np.float64)), torch.tensor(np.asarray(mask, np.float64))
    outs = [torch_program(P, zin, zout, p[:nv], p[nv:2 * nv], p[2 * nv:], zt, seed, step, k0 + k) for k in range(K)]
    nll = sum(torch_inp_nll(o, tg, mk) for o in outs) / K
    nll.backward()
    return dict(nll=float(nll.detach()), grad=p.grad.numpy().copy(), out=np.stack([o.detach().numpy() for o in outs]))


def kl_and_grad(params, n_vi, prior_sigma, prior_mu=0.0):
    """The KL term as the update kernel sums it, sum log(s / s0) + (s0^2 + (mu - m0)^2) / (2 s^2) - 1/2 with s = softplus(rho), and its
    gradient wrt [MU | RHO] (zeros for the BN block), in float64."""
    p = torch.tensor(np.asarray(params, np.float64), requires_grad=True)
    mu, s = p[:n_vi], F.softplus(p[n_vi:2 * n_vi])
    s0 = float(np.float32(prior_sigma))
    kl = (torch.log(s) - np.log(s0) + (s0 * s0 + (mu - prior_mu) ** 2) / (2 * s * s) - 0.5).sum()
    kl.backward()
    return float(kl.detach()), p.grad.numpy().copy()


def adam64(p, g, m, v, lr, t, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update in float64, in place on p / m / v; t is 1-based."""
    m *= b1; m += (1 - b1) * g
    v *= b2; v += (1 - b2) * g * g
    p -= lr / (1 - b1 ** t) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
