"""What the Radon pair costs per call, engine's kernels against the drop-in's.

One process, one GPU.  Per shape (n planes, S x S, T angles) four calls on the same seeded inputs: mfvi_radon_forward / mfvi_radon_adjoint
("old", csrc/radon.hip) and mfvi_radon_project / mfvi_radon_backproject ("new", csrc/radon_planes.hip).  Every shape is warmed, the outputs
of old and new are compared (relerr, which must stay under 4e-5), then the calls are timed in windows that end in a device synchronise, old
and new alternating, two windows per variant, each at least 0.2 s.  Reported per variant: the minimum of its two windows as us per call,
and the spread between them (|a - b| / min) — the yardstick a difference between old and new is read against.  bytes and samples are what
the shape implies (image read or written once, sinogram written or read once; one bilinear sample per plane, angle, row and bin).
Writes profiles/radon_rate.json.

The host clock around a window sees launches as well as kernels; the kernel times themselves come from a trace, in a run of its own:
`rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/radon_rate.py --only new` (or with --trace-calls N: N calls per variant and
shape, old and new, nothing timed and no file written, which keeps the trace small).

usage: python scripts/radon_rate.py [--only new|old] [--window 0.25] [--trace-calls N] [--out profiles/radon_rate.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1, 256, 45), (1, 256, 180), (16, 256, 45), (1, 512, 45)]              # (n, S, T)


def implied(n, S, T):
    return dict(samples=n * T * S * S, image_bytes=4 * n * S * S, sinogram_bytes=4 * n * T * S, theta_bytes=4 * T,
                bytes=4 * (n * S * S + n * T * S + T))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("old", "new"), default=None)
    ap.add_argument("--window", type=float, default=0.25, help="seconds a timed window aims at (at least 0.2 is enforced)")
    ap.add_argument("--trace-calls", type=int, default=0, help="under rocprofv3: this many calls per variant and shape, no timing, no file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radon_rate.json"))
    a = ap.parse_args()
    import torch
    from mfvi_dip_mia_amd import _lib as L
    if not torch.cuda.is_available():
        sys.exit("radon_rate.py measures on the GPU; there is none")
    lib = L.lib()

    def window(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def timed(fn, iters):
        """One window of at least 0.2 s: (seconds per call, iterations used)."""
        while True:
            dt = window(fn, iters)
            if dt >= 0.2:
                return dt / iters, iters
            iters = int(iters * max(2.0, 0.3 / max(dt, 1e-6))) + 1

    res = dict(device=torch.cuda.get_device_name(0), window_s=max(a.window, 0.2), only=a.only, shapes=[])
    for n, S, T in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(1000 + n + S + T)
        img = torch.rand((n, S, S), generator=g).cuda()
        dsn = torch.randn((n, T, S), generator=g).cuda()
        th = torch.linspace(0.0, 180.0, T + 1)[:T].contiguous().cuda()
        sino = {k: torch.empty((n, T, S), device="cuda") for k in ("old", "new")}
        dimg = {k: torch.empty((n, S, S), device="cuda") for k in ("old", "new")}
        st = L.stream_ptr()
        p_img, p_dsn, p_th = L.ptr(img), L.ptr(dsn), L.ptr(th)         # pointers once: the windows time launches, not attribute look-ups
        p_so, p_sn, p_do, p_dn = L.ptr(sino["old"]), L.ptr(sino["new"]), L.ptr(dimg["old"]), L.ptr(dimg["new"])
        calls = {
            ("project", "old"): lambda: L.check(lib.mfvi_radon_forward(p_img, p_th, n, S, S, T, p_so, st)),
            ("project", "new"): lambda: L.check(lib.mfvi_radon_project(p_img, p_th, n, S, T, p_sn, st)),
            ("backproject", "old"): lambda: L.check(lib.mfvi_radon_adjoint(p_dsn, p_th, n, S, S, T, p_do, st)),
            ("backproject", "new"): lambda: L.check(lib.mfvi_radon_backproject(p_dsn, p_th, n, S, T, p_dn, st)),
        }
        if a.only:
            calls = {k: v for k, v in calls.items() if k[1] == a.only}
        iters = {}
        for key, fn in calls.items():                      # warm every shape and size the windows
            window(fn, 5)
            per = window(fn, 20) / 20
            iters[key] = max(20, int(max(a.window, 0.2) * 1.15 / per) + 1)
        row = dict(n=n, S=S, T=T, **implied(n, S, T))
        if not a.only:                                     # faster and different is not faster
            rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
            row["relerr_new_vs_old"] = dict(project=rel(sino["new"], sino["old"]), backproject=rel(dimg["new"], dimg["old"]))
            assert max(row["relerr_new_vs_old"].values()) < 4e-5, row
        if a.trace_calls:                                  # the kernel-trace run: a fixed number of calls, nothing timed or written
            for fn in calls.values():
                window(fn, a.trace_calls)
            continue
        secs = {key: [] for key in calls}
        for _ in range(2):
            for key, fn in calls.items():                  # project old, project new, backproject old, backproject new; twice
                per, iters[key] = timed(fn, iters[key])
                secs[key].append(per)
        for op in ("project", "backproject"):
            r = {}
            for var in ("old", "new"):
                if (op, var) in secs:
                    w = secs[(op, var)]
                    r[var] = dict(us_per_call=min(w) * 1e6, windows_us=[v * 1e6 for v in w], spread=abs(w[0] - w[1]) / min(w),
                                  calls_per_window=iters[(op, var)])
            if len(r) == 2:
                r["old_over_new"] = r["old"]["us_per_call"] / r["new"]["us_per_call"]
                r["spread"] = max(r["old"]["spread"], r["new"]["spread"])
                r["new_no_slower_beyond_spread"] = bool(r["new"]["us_per_call"] <= r["old"]["us_per_call"] * (1.0 + r["spread"]))
            row[op] = r
        res["shapes"].append(row)
        print(json.dumps(row))
    if a.trace_calls:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
