"""Signal-to-noise pruning of a fitted posterior: BayTorch/inference/utils.py:104-166 (L1UnstructuredFFG,
prune_weights_ffg) restated on the flat parameter rows.  A weight is ranked by |mu| / softplus(rho); per row the `amount` share of the
convolution weights and, separately, of the biases with the lowest rank become exactly zero with zero variance in a COPY of the rows.  The
keys, the exact k-th-smallest selection and the copy are kernels of csrc/prune.hip; nothing here touches a fit's own parameters.

Everything up to SnrSelect is host arithmetic and refuses its arguments without the library."""
from . import _lib as L

GROUP_W, GROUP_B = 0, 1
GROUP_NAMES = ("weight", "bias")
HIST_BINS = 64                      # bins of the runner's SNR histogram ...
HIST_LOG10_RANGE = (-4.0, 4.0)      # ... over log10(snr), under- and overflow counted apart


def check_amount(amount, n_rows=None, name="prune"):
    """A share in [0, 1] (n_rows None -> float), or a scalar / one value per row (-> list of n_rows floats).  Anything else: ValueError."""
    import math
    try:
        vals = [float(v) for v in amount]
        scalar = False
    except TypeError:
        try:
            vals, scalar = [float(amount)], True
        except (TypeError, ValueError):
            raise ValueError("%s=%r: a share in [0, 1]" % (name, amount))
    except ValueError:
        raise ValueError("%s=%r: shares in [0, 1]" % (name, amount))
    if n_rows is None:
        if not scalar:
            raise ValueError("%s=%r: one share in [0, 1] for one fit" % (name, amount))
    elif scalar:
        vals = vals * int(n_rows)
    elif len(vals) != int(n_rows):
        raise ValueError("%s: %d values for %d rows (a scalar, or one value per row)" % (name, len(vals), n_rows))
    for v in vals:
        if math.isnan(v) or not 0.0 <= v <= 1.0:
            raise ValueError("%s=%r: a share outside [0, 1]" % (name, amount))
    return vals[0] if n_rows is None else vals


def k_of(amount, n):
    """Weights to prune: the reference's truncation int(amount * n) in double precision (inference/utils.py:120)."""
    return int(float(amount) * n)


def layer_spans(prog):
    """Per layer of the program its [(offset, count, group)]: the weights (group 0) and, where the layer has one, the bias (group 1)."""
    spans = []
    for lay in prog.layers:
        one = [(int(lay["w_off"]), lay["cout"] * lay["cin"] * lay["k"] * lay["k"], GROUP_W)]
        if lay["b_off"] >= 0:
            one.append((int(lay["b_off"]), int(lay["cout"]), GROUP_B))
        spans.append(one)
    return spans


def segment_table(prog):
    """[(offset, count, group)] of every layer of the program (or of a list of per-layer spans), sorted by offset."""
    return sorted(s for one in (layer_spans(prog) if hasattr(prog, "layers") else prog) for s in one)


def check_segments(segs, n_vi):
    """The table mfvi_snr_select takes: sorted, disjoint, inside [0, n_vi), groups 0 / 1, at most MFVI_PRUNE_MAX_SEGMENTS entries."""
    if len(segs) > L.PRUNE_MAX_SEGMENTS:
        raise ValueError("%d segments: at most %d" % (len(segs), L.PRUNE_MAX_SEGMENTS))
    end = 0
    for off, cnt, g in segs:
        if g not in (GROUP_W, GROUP_B) or cnt < 0 or off < end or off + cnt > n_vi:
            raise ValueError("segment (%d, %d, %d): sorted, disjoint, inside 0..%d, group 0 or 1" % (off, cnt, g, n_vi))
        end = off + cnt
    return segs


def group_sizes(segs):
    n = [0, 0]
    for _, cnt, g in segs:
        n[g] += cnt
    return n


def pack_segments(segs):
    """bytes of mfvi_prune_segment[len(segs)]."""
    return b"".join(bytes(L.PruneSegment(off, cnt, g, 0)) for off, cnt, g in segs)


def layer_names(prog):
    return ["layer%d" % i for i in range(len(prog.layers))]


def check_engine(eng):
    """What ElboEngine.predict(prune=) / snr() / prune_mask() refuse, from attributes alone."""
    if getattr(eng, "method", None) is not None:
        raise TypeError("SNR pruning ranks a posterior N(mu, softplus(rho)^2): the point-weight siblings (method %r) have no rho" % (eng.method,))
    if getattr(eng, "param_dtype", "f32") == "bf16":
        raise NotImplementedError("SNR pruning with param_dtype='bf16' is not built: the kernels read float32 parameter rows")
    if getattr(eng, "world", 1) > 1:
        raise NotImplementedError("SNR pruning with world_size > 1 is not built (sharded prediction under pruning)")


def check_batch(batch):
    """What RowBatch.predict(prune=) / snr() / prune_mask() refuse, from attributes alone."""
    if getattr(batch, "method", None) is not None or not getattr(batch, "sample_weights", True):
        raise TypeError("SNR pruning ranks a posterior N(mu, softplus(rho)^2): the point-weight sibling batches have no rho")


def hist_bounds(n_bins=HIST_BINS, log10_range=HIST_LOG10_RANGE):
    """(edges_log10 float64 [n_bins + 1], float32 boundaries in key space): the comparison happens on the float32 values."""
    import numpy as np
    if not 1 <= int(n_bins) <= L.SNR_MAX_BINS:
        raise ValueError("n_bins=%r outside 1..%d" % (n_bins, L.SNR_MAX_BINS))
    lo, hi = float(log10_range[0]), float(log10_range[1])
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("log10_range=%r: two finite increasing numbers" % (log10_range,))
    edges = np.linspace(lo, hi, int(n_bins) + 1)
    return edges, np.float32(10.0) ** edges.astype(np.float32)


class SnrSelect:
    """Keys, mask and scratch of `rows` parameter rows of one network (spans: layer_spans(prog), or the same list built from a module tree),
    allocated once per owner."""

    def __init__(self, torch, spans, n_vi, rows, stride, row_floats):
        self.torch, self.spans, self.rows, self.stride, self.row_floats = torch, spans, int(rows), int(stride), int(row_floats)
        self.n_vi = int(n_vi)
        if self.n_vi >= 2 ** 31:
            raise ValueError("n_vi=%d: below 2**31" % self.n_vi)
        self.segs = check_segments(segment_table(spans), self.n_vi)
        self.n_group = group_sizes(self.segs)
        lib = L.lib()
        dev, R = "cuda", self.rows
        self.keys = torch.empty((R, self.n_vi), dtype=torch.float32, device=dev)
        self.mask = torch.empty((R, self.n_vi), dtype=torch.uint8, device=dev)
        self.segs_dev = torch.frombuffer(bytearray(pack_segments(self.segs) or b"\0" * 24), dtype=torch.uint8).to(dev)
        nb = int(lib.mfvi_snr_select_scratch_bytes(R))
        if nb < 0:
            raise L.MfviError(lib.mfvi_last_error().decode())
        self.scratch = torch.empty(nb // 8 + 1, dtype=torch.int64, device=dev)
        self.k_dev = torch.zeros((R, 2), dtype=torch.int64, device=dev)
        self.thr = torch.zeros((R, 2), dtype=torch.int32, device=dev)
        self.ties = torch.zeros((R, 2), dtype=torch.int64, device=dev)
        self.pruned = None          # the pruned clone of the rows, on first apply()

    def compute_keys(self, rows_buf):
        """keys [rows, n_vi] of the parameter rows (a tensor whose row r starts stride floats behind row r - 1)."""
        L.check(L.lib().mfvi_snr_keys(L.ptr(rows_buf), self.rows, self.stride, self.n_vi, L.ptr(self.keys), L.stream_ptr()))
        return self.keys

    def select(self, rows_buf, amounts):
        """Keys and selection for one share per row -> k [rows][2] (host ints); mask / thr / ties are filled on the device."""
        import numpy as np
        ks = [[k_of(a, n) for n in self.n_group] for a in amounts]
        self.compute_keys(rows_buf)
        self.k_dev.copy_(self.torch.from_numpy(np.asarray(ks, np.int64).reshape(self.rows, 2)))
        L.check(L.lib().mfvi_snr_select(L.ptr(self.keys), self.rows, self.n_vi, L.ptr(self.segs_dev), len(self.segs), L.ptr(self.k_dev), L.ptr(self.mask),
                                        L.ptr(self.thr), L.ptr(self.ties), L.ptr(self.scratch), L.stream_ptr()))
        return ks

    def apply(self, rows_buf):
        """The pruned clone of the rows under the current mask (same stride; allocated once, rewritten whole every time)."""
        if self.pruned is None:
            self.pruned = self.torch.zeros(self.rows * self.stride, dtype=self.torch.float32, device="cuda")
        L.check(L.lib().mfvi_prune_apply(L.ptr(rows_buf), L.ptr(self.pruned), L.ptr(self.mask), self.rows, self.stride, self.n_vi, self.row_floats,
                                         L.stream_ptr()))
        return self.pruned

    def info(self, ks, amounts, with_mask=True):
        """Per row dict(amount, k [2], n [2], threshold [2] (float32 keys; NaN where nothing is pruned), ties [2], layer_sparsity [n_layers],
        mask [n_vi] uint8 with 0 = pruned).  The per-layer counts are torch sums over the layers' segments; one host sync."""
        import numpy as np
        torch = self.torch
        thr = self.thr.cpu().numpy().view(np.uint32)
        ties = self.ties.cpu().numpy()
        kept = torch.stack([sum(self.mask[:, off:off + cnt].sum(dim=1, dtype=torch.int64) for off, cnt, _ in one)
                            for one in self.spans]).cpu().numpy()                # [n_layers, rows]
        sizes = np.array([sum(c for _, c, _ in one) for one in self.spans], np.int64)
        out = []
        for r in range(self.rows):
            k = np.asarray(ks[r], np.int64)
            t = thr[r].view(np.float32).copy()
            t[k == 0] = np.nan
            d = dict(amount=float(amounts[r]), k=k, n=np.asarray(self.n_group, np.int64), threshold=t, ties=ties[r].copy(),
                     layer_sparsity=(sizes - kept[:, r]) / np.maximum(sizes, 1).astype(np.float64), layer_pruned=sizes - kept[:, r])
            if with_mask:
                d["mask"] = self.mask[r].clone()
            out.append(d)
        return out


def snr_histogram(sel, n_bins=HIST_BINS, log10_range=HIST_LOG10_RANGE):
    """Histogram of the CURRENT keys of a SnrSelect -> (counts int64 [rows, 2, n_bins + 2] on the host, edges_log10 [n_bins + 1]): slot 0 the
    underflow, slot n_bins + 1 the overflow (NaN keys included), slot s the keys with bounds[s - 1] <= key < bounds[s]."""
    edges, bounds = hist_bounds(n_bins, log10_range)
    torch = sel.torch
    b = torch.from_numpy(bounds).cuda()
    counts = torch.empty((sel.rows, 2, int(n_bins) + 2), dtype=torch.int64, device="cuda")
    L.check(L.lib().mfvi_snr_histogram(L.ptr(sel.keys), sel.rows, sel.n_vi, L.ptr(sel.segs_dev), len(sel.segs), L.ptr(b), int(n_bins), L.ptr(counts),
                                       L.stream_ptr()))
    return counts.cpu().numpy(), edges


def owner_select(owner, rows, stride, row_floats):
    """The owner's SnrSelect, allocated on first use."""
    sel = owner.__dict__.get("_snr_state")
    if sel is None:
        sel = owner.__dict__["_snr_state"] = SnrSelect(owner.torch, layer_spans(owner.prog), owner.prog.n_vi, rows, stride, row_floats)
    return sel
