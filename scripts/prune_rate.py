"""Times the SNR pruning path at the cfg2 net (n_vi = 1 035 446): keys + select + apply for 1 row (an ElboEngine) and for 16 rows (a
FitBatch), against the same selection stated with torch.sort on the same GPU (the baseline, not the code under test), and
predict(64, prune=0.5) against predict(64).  Run in a fresh process; per case `warmup` untimed repetitions, then `windows` windows of `reps`
repetitions between two events; the median window and the spread (min, max) are reported per repetition.

usage:  python scripts/prune_rate.py [out.json]      (default profiles/prune_rate.json)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, warmup=5, windows=7, reps=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record(); b.synchronize()
        ms.append(a.elapsed_time(b) / reps)
    ms.sort()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], windows=windows, reps=reps)


def torch_statement(torch, rows_buf, n_vi, idx, ks, out):
    """The same selection with torch: keys, a stable sort per row and group, the mask, the pruned copy."""
    R = rows_buf.shape[0]
    mu, rho = rows_buf[:, :n_vi], rows_buf[:, n_vi:2 * n_vi]
    keys = mu.abs() / torch.nn.functional.softplus(rho)
    mask = torch.ones((R, n_vi), dtype=torch.bool, device=rows_buf.device)
    for g in (0, 1):
        order = torch.sort(keys[:, idx[g]], dim=1, stable=True).indices
        for r in range(R):
            mask[r, idx[g][order[r, :ks[r][g]]]] = False
    out.copy_(rows_buf)
    out[:, :n_vi][~mask] = 0.0
    out[:, n_vi:2 * n_vi][~mask] = -200.0
    return out


def main():
    import numpy as np
    import torch
    import mfvi_dip_mia_amd as M
    from mfvi_dip_mia_amd import prune as P
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "prune_rate.json")
    res = dict(device=torch.cuda.get_device_name(0))
    eng = M.engine.ElboEngine(256, 256, K=2, input_depth=16, autotune=False, seed=1)
    res["n_vi"] = eng.n_vi
    sel = eng._snr_select()

    def lib_one(amounts=(0.5,)):
        sel.select(eng.params, list(amounts)); sel.apply(eng.params)
    res["rows1_library"] = timed(torch, lib_one)
    idx = [torch.from_numpy(np.concatenate([np.arange(o, o + c) for o, c, gg in sel.segs if gg == g])).cuda() for g in (0, 1)]
    buf1, out1 = eng.params[None], torch.empty_like(eng.params)[None]
    ks1 = [[P.k_of(0.5, n) for n in sel.n_group]]
    res["rows1_torch_sort"] = timed(torch, lambda: torch_statement(torch, buf1, eng.n_vi, idx, ks1, out1), windows=5, reps=3)
    lib_one()
    torch_statement(torch, buf1, eng.n_vi, idx, ks1, out1)
    res["rows1_equal"] = bool(torch.equal(sel.pruned[:eng.n_params], out1[0]))
    res["predict64"] = timed(torch, lambda: eng.predict(64), warmup=2, windows=5, reps=2)
    res["predict64_prune0.5"] = timed(torch, lambda: eng.predict(64, prune=0.5), warmup=2, windows=5, reps=2)
    del eng, sel
    F = 16
    fb = M.FitBatch(256, 256, F, task="den", K=1, input_depth=16, temp=[1e-6] * F, sigma=[0.05] * F, lr=[1e-3] * F, seed=1, autotune=False)
    bsel = fb._snr_select()
    amounts = [0.05 * (f + 1) for f in range(F)]

    def lib_rows():
        bsel.select(fb._pbuf, amounts); bsel.apply(fb._pbuf)
    res["rows16_library"] = timed(torch, lib_rows)
    ks = [[P.k_of(a, n) for n in bsel.n_group] for a in amounts]
    out = torch.empty_like(fb._pbuf)
    res["rows16_torch_sort"] = timed(torch, lambda: torch_statement(torch, fb._pbuf, fb.n_vi, idx, ks, out), windows=3, reps=1, warmup=1)
    lib_rows()
    torch_statement(torch, fb._pbuf, fb.n_vi, idx, ks, out)
    res["rows16_equal"] = bool(torch.equal(bsel.pruned.view(F, fb.stride)[:, :fb.n_params], out[:, :fb.n_params]))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
