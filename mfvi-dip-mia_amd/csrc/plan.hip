// Host side of libmfvi_hip: the layer-program planner/executor behind mfvi_plan_* / mfvi_forward /
// mfvi_backward (include/mfvi_hip.h).  It validates the fused-op program emitted by the Python front-end
// (which walks the reference's module tree: models/skip.py:58-134), lays the activations, gradients and
// BN statistics out in one caller-provided workspace, and issues the kernels on the caller's stream.
#include "plan_internal.h"

#include <cstdarg>

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}

bool fail(const char* fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return false;
}

const PlanSwitches& switches()
{
    static const PlanSwitches s = [] {
        auto on = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };      // default on, "0..." switches off
        auto num = [](const char* name, long long dflt) { const char* e = getenv(name); return e ? atoll(e) : dflt; };
        return PlanSwitches{on("MFVI_FOLD_FUSION"), on("MFVI_FOLD_FUSION3"), num("MFVI_FWD_FORK", 16384), on("MFVI_FORK_ON_PACKET"),
                            on("MFVI_SIDE_STREAM"), num("MFVI_SIDE_MAXPIX", 1LL << 40), on("MFVI_SIDE_PRIO"), on("MFVI_FUSE_SKIP_BWD")};
    }();
    return s;
}

bool check_call(const mfvi_plan* p, int n_samples, const void* ws)
{
    if (!p) return fail("null plan");
    if (!ws) return fail("null workspace");
    if (n_samples < 1 || n_samples > p->max_samples) return fail("n_samples %d outside 1..%d", n_samples, p->max_samples);
    return true;
}

// Fits mode runs on the sampled-weight slab alone: whatever reads ONE mu / rho / bn for all samples, or reduces over all of them, is refused
// rather than served with fit 0's parameters.
int fits_refusal(const mfvi_plan* p, const char* who)
{
    const char* what = nullptr;
    if (p->param_dtype == MFVI_PARAM_BF16) what = "bf16 parameter storage";
    else if (p->n_lrt) what = "local-reparameterisation layers";
    else if (p->bn_eval) what = "BatchNorm eval mode";
    else if (p->split_op >= 0) what = "a gradient split";
    else if (p->step_dev) what = "a device step source";
    else if (p->n_generic > 0 || p->n_samp < 1) what = "layers outside the sampling table (input channels and weight offsets must be multiples of 4)";
    else if (!use_mfma()) what = "MFVI_DISABLE_MFMA (the generic kernels read one mu / rho)";
    if (!what) return 0;
    set_error("%s: fits mode (mfvi_plan_set_fits) does not serve %s", who, what);
    return MFVI_ERR_FITS_UNSUPPORTED;
}

namespace {

inline long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

// the program is well-formed: shapes, offsets, program order = execution order, the consumer patterns the kernels serve
bool validate_program(mfvi_plan& p, const mfvi_tensor_desc* td, int n_t, const mfvi_op_desc* od, int n_ops)
{
    if (n_t < 2 || n_ops < 1) return fail("plan: need >= 2 tensors and >= 1 op");
    if (p.input < 0 || p.input >= n_t || p.output < 0 || p.output >= n_t || p.input == p.output)
        return fail("plan: bad input/output tensor ids %d/%d", p.input, p.output);
    if (p.max_samples < 1) return fail("plan: max_samples must be >= 1");
    p.t.resize(n_t); p.ops.resize(n_ops);
    for (int i = 0; i < n_t; ++i) {
        TensorInfo& ti = p.t[i]; ti.d = td[i];
        if (ti.d.C < 1 || ti.d.H < 1 || ti.d.W < 1 || ti.d.C > MFVI_MAX_C) return fail("plan: tensor %d has bad shape (%d,%d,%d)", i, ti.d.C, ti.d.H, ti.d.W);
        if (ti.d.has_act && !ti.d.has_bn) return fail("plan: tensor %d: activation without BatchNorm is not part of the skip() family", i);
        if (ti.d.has_bn && (ti.d.bn_off < 0 || ti.d.bn_off + 2LL * ti.d.C > p.n_bn)) return fail("plan: tensor %d: bn_off out of range", i);
        if (!(ti.d.drop_p >= 0.f && ti.d.drop_p < 1.f)) return fail("plan: tensor %d: dropout probability %g outside [0, 1)", i, (double)ti.d.drop_p);
        if (ti.d.has_act && !(ti.d.slope >= 0.f && ti.d.slope <= 1.f)) return fail("plan: tensor %d: LeakyReLU slope %g outside [0, 1] (the kernels form it as max(v, slope * v))", i, (double)ti.d.slope);
        if (ti.d.drop_p > 0.f && !ti.d.has_bn) return fail("plan: tensor %d: Dropout2d without a following BatchNorm is not part of the skip() family", i);
        ti.numel = (long long)ti.d.C * ti.d.H * ti.d.W;
    }
    if (p.t[p.input].d.has_bn) return fail("plan: the input tensor cannot carry a BatchNorm");
    if (p.t[p.output].d.has_bn) return fail("plan: the output tensor must be raw (no BatchNorm/activation)");
    for (int i = 0; i < n_ops; ++i) {
        OpInfo& o = p.ops[i]; o.d = od[i];
        const mfvi_op_desc& d = o.d;
        if (d.out < 0 || d.out >= n_t || d.out == p.input) return fail("plan: op %d: bad output tensor", i);
        if (p.t[d.out].producer >= 0) return fail("plan: tensor %d produced twice", d.out);
        p.t[d.out].producer = i;
        if (d.type == MFVI_OP_CONV || d.type == MFVI_OP_CONV_LRT) {
            if (d.in0 < 0 || d.in0 >= n_t) return fail("plan: op %d: bad input tensor", i);
            if (d.type == MFVI_OP_CONV_LRT) { ++p.n_lrt; if (d.b_off < 0) return fail("plan: op %d: a local-reparameterisation layer needs its bias (skip() builds every conv with one)", i); }
            const TensorInfo& x = p.t[d.in0]; const TensorInfo& y = p.t[d.out];
            if (!(((d.ksize == 3 || d.ksize == 5) && (d.stride == 1 || d.stride == 2)) || (d.ksize == 1 && d.stride == 1)))
                return fail("plan: op %d: conv ksize %d stride %d not supported (3x3 / 5x5 s1/s2, 1x1 s1)", i, d.ksize, d.stride);
            const int P = d.ksize / 2;
            const int Ho = (x.d.H + 2 * P - d.ksize) / d.stride + 1, Wo = (x.d.W + 2 * P - d.ksize) / d.stride + 1;
            if (Ho != y.d.H || Wo != y.d.W) return fail("plan: op %d: output spatial size (%d,%d) != expected (%d,%d)", i, y.d.H, y.d.W, Ho, Wo);
            if (P > 0 && (x.d.H <= P || x.d.W <= P)) return fail("plan: op %d: reflection padding %d needs H,W > %d", i, P, P);
            const long long nw = (long long)y.d.C * x.d.C * d.ksize * d.ksize;
            if (d.w_off < 0 || d.w_off + nw > p.n_vi) return fail("plan: op %d: w_off out of range", i);
            if (d.b_off >= 0 && d.b_off + y.d.C > p.n_vi) return fail("plan: op %d: b_off out of range", i);
            if (d.layer_id < 0 || d.layer_id >= (1 << 22)) return fail("plan: op %d: bad layer_id", i);
            o.g = ConvGeom{x.d.C, y.d.C, x.d.H, x.d.W, Ho, Wo, d.ksize, d.stride, d.w_off, d.b_off, d.layer_id};
            p.t[d.in0].consumers.push_back(i);
        } else if (d.type == MFVI_OP_CONCAT_UP) {
            if (d.in1 < 0 || d.in1 >= n_t || d.in0 >= n_t) return fail("plan: op %d: bad input tensors", i);
            if (d.up_mode != MFVI_UP_BILINEAR && d.up_mode != MFVI_UP_NEAREST) return fail("plan: op %d: unknown upsampling mode %d (bilinear, nearest)", i, d.up_mode);
            const TensorInfo& b = p.t[d.in1]; const TensorInfo& y = p.t[d.out];
            int Ca = 0;
            if (d.in0 >= 0) {
                const TensorInfo& a = p.t[d.in0]; Ca = a.d.C;
                // Concat centre-crops to the smaller input (models/common.py:31-41).  In skip() the up-sampled branch is 2*ceil(H/2) against
                // the skip branch's H, so the crop offset (size - target) / 2 is 0 and at most its last row / column is dropped.
                if (2 * b.d.H < a.d.H || 2 * b.d.H - a.d.H > 1 || 2 * b.d.W < a.d.W || 2 * b.d.W - a.d.W > 1)
                    return fail("plan: op %d: concat inputs %dx%d vs 2*%dx%d: only the crop of the up-sampled branch by one row / column is built", i, a.d.H, a.d.W, b.d.H, b.d.W);
                if (d.in0 == p.input) return fail("plan: op %d: the net input cannot feed a concat", i);
                p.t[d.in0].consumers.push_back(i);
            }
            if (d.in1 == p.input) return fail("plan: op %d: the net input cannot feed an upsample", i);
            const int cH = d.in0 >= 0 ? p.t[d.in0].d.H : 2 * b.d.H, cW = d.in0 >= 0 ? p.t[d.in0].d.W : 2 * b.d.W;
            if (y.d.C != Ca + b.d.C || y.d.H != cH || y.d.W != cW) return fail("plan: op %d: concat output shape mismatch", i);
            p.t[d.in1].consumers.push_back(i);
        } else return fail("plan: op %d: unknown type %d", i, d.type);
        // inputs must already be produced (program order = execution order)
        const int ins[2] = {d.in0, d.type == MFVI_OP_CONCAT_UP ? d.in1 : -1};
        for (int q = 0; q < 2; ++q)
            if (ins[q] >= 0 && ins[q] != p.input && (p.t[ins[q]].producer < 0 || p.t[ins[q]].producer >= i))
                return fail("plan: op %d reads tensor %d before it is produced", i, ins[q]);
    }
    for (int i = 0; i < n_t; ++i) {
        if (p.t[i].d.drop_p > 0.f && (p.t[i].producer < 0 || p.ops[p.t[i].producer].d.type == MFVI_OP_CONCAT_UP))
            return fail("plan: tensor %d: Dropout2d must follow a convolution", i);
        if (i != p.input && p.t[i].producer < 0) return fail("plan: tensor %d is never produced", i);
        if (i != p.output && p.t[i].consumers.empty()) return fail("plan: tensor %d is never consumed", i);
        if (i == p.output && !p.t[i].consumers.empty()) return fail("plan: the output tensor has consumers");
        bool cat = false;
        for (int c : p.t[i].consumers) cat |= p.ops[c].d.type == MFVI_OP_CONCAT_UP;
        if (p.n_lrt && p.t[i].d.drop_p > 0.f) return fail("plan: Dropout2d and local-reparameterisation layers are not combined by any runner");
        if (cat && p.t[i].consumers.size() != 1) return fail("plan: tensor %d feeds a concat and something else", i);
        if (p.t[i].consumers.size() > 2) return fail("plan: tensor %d has %d consumers (max 2)", i, (int)p.t[i].consumers.size());
    }
    return true;
}

// workspace offsets of every tensor, scratch and table; the device tables that do not change afterwards
bool layout_workspace(mfvi_plan& p)
{
    const int n_t = (int)p.t.size();
    long long sd = 0;
    std::vector<BnGradEntry> table;
    for (int i = 0; i < n_t; ++i)
        if (p.t[i].d.has_bn) {
            p.t[i].stats_off = sd; sd += (long long)p.max_samples * p.t[i].d.C * 2;
            BnGradEntry e; e.bsums_off = p.t[i].stats_off; e.bn_off = p.t[i].d.bn_off; e.C = p.t[i].d.C; e.hw = p.t[i].d.H * p.t[i].d.W;
            table.push_back(e); if (p.t[i].d.C > p.max_c) p.max_c = p.t[i].d.C;
        }
    p.stats_doubles = align_up(sd, 32);
    p.float_base = 2 * p.stats_doubles * (long long)sizeof(double);
    long long fo = 0;
    auto take = [&](long long n) { const long long o = fo; fo += align_up(n, 64); return o; };
    for (int i = 0; i < n_t; ++i) {
        if (i != p.input && i != p.output) p.t[i].act_off = take(p.t[i].numel * p.max_samples);
        if (i != p.output && i != p.input) p.t[i].ga_off = take(p.t[i].numel * p.max_samples);
    }
    std::vector<DropEntry> drops;
    for (int i = 0; i < n_t; ++i)
        if (p.t[i].d.drop_p > 0.f) {
            p.t[i].drop_off = take((long long)p.t[i].d.C * p.max_samples);
            DropEntry e{}; e.drop_off = p.t[i].drop_off; e.C = p.t[i].d.C; e.layer_id = p.ops[p.t[i].producer].d.layer_id; e.p = p.t[i].d.drop_p;
            drops.push_back(e);
        }
    p.n_drop = (int)drops.size();
    if (p.n_drop) {
        hipError_t e = hipMalloc((void**)&p.drop_dev, sizeof(DropEntry) * drops.size());
        if (e == hipSuccess) e = hipMemcpy(p.drop_dev, drops.data(), sizeof(DropEntry) * drops.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail("plan: dropout table setup failed: %s", hipGetErrorString(e));
    }
    long long shared_scratch = 0;
    for (auto& o : p.ops)
        if (o.d.type != MFVI_OP_CONCAT_UP) {
            const bool lrt = o.d.type == MFVI_OP_CONV_LRT;
            const long long n = o.padded_per_sample() * p.max_samples;
            if (p.t[o.d.in0].consumers.size() > 1) { o.scratch_off = take(n); if (lrt) o.scratch2_off = take(n); }       // live until the fold of in0
            else if ((lrt ? 2 : 1) * n > shared_scratch) shared_scratch = (lrt ? 2 : 1) * n;
            if (lrt) {
                const long long no = (long long)o.g.Cout * o.g.Ho * o.g.Wo * p.max_samples;
                o.s2_off = take(no);
                if (no > p.lrt_tmp_n) p.lrt_tmp_n = no;
            }
        }
    const long long shared_off = take(shared_scratch);
    for (auto& o : p.ops)
        if (o.d.type != MFVI_OP_CONCAT_UP && o.scratch_off < 0) {
            o.scratch_off = shared_off;
            if (o.d.type == MFVI_OP_CONV_LRT) o.scratch2_off = shared_off + o.padded_per_sample() * p.max_samples;
        }
    if (p.n_lrt) { p.sig2_off = take(p.n_vi); p.dsig2_off = take(p.n_vi); p.lrt_tmp_off = take(p.lrt_tmp_n); }
    // weights of the MFMA-served layers are sampled once per pass into [max_samples][n_vi]
    std::vector<SampleEntry> samp;
    for (auto& o : p.ops)      // (LRT layers draw nothing in weight space: their convolutions read mu and softplus(rho)^2)
        if ((o.in_slab = o.d.type == MFVI_OP_CONV && !(o.g.Cin & 3) && !(o.g.w_off & 3) && o.g.Cin <= MFVI_MAX_C && o.g.Cout <= MFVI_MAX_C)) {
            SampleEntry e{};
            e.w_off = o.g.w_off; e.b_off = o.g.b_off; e.n_w = (int)o.n_weights(); e.n_b = o.n_bias();
            e.layer_id = o.g.layer_id; e.first_block = p.samp_blocks;
            p.samp_blocks += quads_to_blocks(e.n_w, e.n_b, SAMPLE_QUADS);
            samp.push_back(e);
        }
    p.n_samp = (int)samp.size();
    for (auto& o : p.ops) if (o.d.type != MFVI_OP_CONCAT_UP) ++p.n_generic;
    p.n_generic -= p.n_samp;
    if (p.n_generic > 0) p.p32_off = take(2 * p.n_vi);
    if (p.n_samp) {
        p.wsamp_off = take(p.n_vi * p.max_samples);
        hipError_t e = hipMalloc((void**)&p.samp_dev, sizeof(SampleEntry) * samp.size());
        if (e == hipSuccess) e = hipMemcpy(p.samp_dev, samp.data(), sizeof(SampleEntry) * samp.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail("plan: sampling table setup failed: %s", hipGetErrorString(e));
    }
    // partial-dW slabs: up to ~4M floats per layer, at least one pixel strip
    for (auto& o : p.ops)
        if (o.d.type != MFVI_OP_CONCAT_UP) {
            ++p.n_conv;
            o.part_stride = o.n_weights() + (o.g.b_off >= 0 ? align_up(o.g.Cout, 4) : 0);
            const long long ms = (4LL << 20) / (o.part_stride * p.max_samples);
            o.max_strips = (int)(ms < 1 ? 1 : (ms > 64 ? 64 : ms));
            o.part_off = take(o.part_stride * p.max_samples * o.max_strips);
            if (o.d.type == MFVI_OP_CONV) { const long long xf = x6_fwd_scratch_floats(o.g, p.max_samples); if (xf > 0) o.x6w_off = take(xf); }
            if (o.d.type == MFVI_OP_CONV && o.d.in0 != p.input && p.t[o.d.in0].consumers.size() == 1) {      // (the fused-fold path: the conv's input feeds nothing else)
                const long long xb = x6_bwd_scratch_floats(o.g, p.max_samples); if (xb > 0) o.x6bw_off = take(xb); }
        }
    p.total_bytes = p.float_base + fo * (long long)sizeof(float);
    if (p.n_conv) {      // one allocation: whole pass | early group | late group of a gradient split
        const hipError_t e = hipMalloc((void**)&p.fin[0].dev, sizeof(GradFinEntry) * p.n_conv * 3);
        if (e != hipSuccess) return fail("plan: hipMalloc of the gradient table failed: %s", hipGetErrorString(e));
        p.fin[1].dev = p.fin[0].dev + p.n_conv; p.fin[2].dev = p.fin[0].dev + 2 * p.n_conv;
    }
    p.n_entries = (int)table.size();
    if (p.n_entries) {
        hipError_t e = hipMalloc((void**)&p.table_dev, sizeof(BnGradEntry) * table.size());
        if (e != hipSuccess) return fail("plan: hipMalloc of the BN table failed: %s", hipGetErrorString(e));
        e = hipMemcpy(p.table_dev, table.data(), sizeof(BnGradEntry) * table.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail("plan: hipMemcpy of the BN table failed: %s", hipGetErrorString(e));
    }
    return true;
}

}  // namespace

// ---- what mfvi_forward, mfvi_backward and mfvi_plan_autotune share of a pass ----
int pass_setup(PassSetup& S, bool expand, uint64_t seed, uint32_t step, uint32_t k0)
{
    mfvi_plan* plan = S.plan;
    S.bf16 = plan->param_dtype == MFVI_PARAM_BF16;
    if (S.bf16 && !use_mfma()) { set_error("%s: bf16 parameters need the MFMA path (MFVI_DISABLE_MFMA is set)", S.who); return -1; }
    if (S.bf16 && (((uintptr_t)S.mu_v | (uintptr_t)S.rho_v) & 7)) { set_error("%s: bf16 mu / rho must be 8-byte aligned", S.who); return -1; }
    // float32 view of mu / rho for the generic kernels: the caller's arrays, or their expansion when the parameters are stored in bf16
    if (!S.bf16) { S.mu = static_cast<const float*>(S.mu_v); S.rho = static_cast<const float*>(S.rho_v); }
    else if (expand && plan->n_generic > 0) {
        float* dst = S.c.farena() + plan->p32_off;
        int rc = launch_expand_bf16(S.mu_v, plan->n_vi, dst, S.st);
        if (!rc) rc = launch_expand_bf16(S.rho_v, plan->n_vi, dst + plan->n_vi, S.st);
        if (rc) { set_error("%s: bf16 expansion failed: %s", S.who, hipGetErrorString((hipError_t)rc)); return rc; }
        S.mu = dst; S.rho = dst + plan->n_vi;
    }
    S.presample = use_mfma() && (S.sample_weights || S.bf16) && plan->n_samp > 0;
    S.key = base_key(seed, step, k0, plan->step_dev);
    S.W = ConvWeights{S.presample ? S.c.wsamp() : S.mu, (S.presample && S.sample_weights) ? plan->n_vi : 0, S.mu, S.rho, S.key, S.sample_weights};
    if (plan->fit_s) {
        // F = n_samples / fit_s fits in one pass: sample i is sample i % fit_s of fit i / fit_s and uses eps of global sample k0 + i
        // (k0 + (i / fit_s) * fit_kstride + i % fit_s after mfvi_plan_set_fits_sample_stride)
        if (int rc = fits_refusal(plan, S.who)) return rc;
        if (!S.sample_weights && !plan->fit_points) { set_error("%s: fits mode (mfvi_plan_set_fits) does not serve sample_weights = 0", S.who); return MFVI_ERR_FITS_UNSUPPORTED; }
        if (S.n_samples % plan->fit_s) { set_error("%s: n_samples %d is not a multiple of the %d samples per fit", S.who, S.n_samples, plan->fit_s); return -1; }
        S.c.fit_s = plan->fit_s; S.c.gamma_fstride = plan->fit_pstride; S.c.z_sstride = plan->t[plan->input].numel;
        if (plan->fit_s > 1) {      // z[n_fits][Cin][H][W] once per sample
            float* zr = S.c.farena() + plan->zrep_off;
            const int rc = launch_replicate_input(S.c.z, plan->t[plan->input].numel, plan->fit_s, S.n_samples, zr, S.st);
            if (rc) { set_error("%s: fits mode: the copy of the net input per sample failed (its size must be a multiple of 4 floats, z 16-byte aligned): %s", S.who, hipGetErrorString((hipError_t)rc)); return rc > 0 ? rc : -1; }
            S.c.z = zr;
        }
        // a layer the matrix-core kernels decline (a map not a multiple of 4 wide) runs on the generic kernels: fit 0's mu / rho plus the strides,
        // sample k reads and accumulates at fit k / fit_s (every layer is in the sampling table here: fits_refusal)
        // points mode (sample_weights = 0 with mfvi_plan_set_fits_points): the same rows hold each sample's fit's mu, the generic kernels read w = mu
        S.points = !S.sample_weights; S.presample = true;
        if (!plan->fit_drop.empty() && plan->n_drop && (int)plan->fit_drop.size() != S.n_samples / plan->fit_s) {
            set_error("%s: mfvi_plan_set_fit_dropout gave %d probabilities, this pass has %d fits", S.who, (int)plan->fit_drop.size(), S.n_samples / plan->fit_s); return -1; }
        S.W = ConvWeights{S.c.wsamp(), plan->n_vi, S.mu, S.rho, S.key, S.sample_weights, FitGeom{plan->fit_s, plan->fit_pstride, plan->fit_gstride, plan->fit_kdelta()}};
    }
    return 0;
}

namespace {

bool split_entry(const ConvGeom& g, long long off, X6SplitEntry* e) { return x6_split_entry(g, off, e); }
bool split_entry(const ConvGeom& g, long long off, X6BSplitEntry* e) { return x6b_split_entry(g, off, e); }
int split_units(const X6SplitEntry& e) { return e.units; }
int split_units(const X6BSplitEntry& e) { return e.units + e.rem_units; }
int launch_split_all(const X6SplitEntry* t, int n, int nb, const float* w, long long ws, int nk, float* a, hipStream_t st) { return launch_x6_split_all(t, n, nb, w, ws, nk, a, st); }
int launch_split_all(const X6BSplitEntry* t, int n, int nb, const float* w, long long ws, int nk, float* a, hipStream_t st) { return launch_x6b_split_all(t, n, nb, w, ws, nk, a, st); }

template <typename E> int split_pieces(PassSetup& S, DeviceTable<E>& T, int pass, const float* dz)
{
    mfvi_plan* plan = S.plan;
    std::vector<E> tab; int nb = 0;
    for (auto& o : plan->ops) {
        const long long off = pass == 0 ? o.x6w_off : o.x6bw_off;
        if (o.d.type != MFVI_OP_CONV || off < 0 || !(o.g.tune[pass] & MFVI_TUNE_X6) || (pass == 1 && !S.c.need_dx(o, dz))) continue;
        E e; if (!split_entry(o.g, off, &e)) continue;
        e.first_block = nb; nb += (split_units(e) + 255) / 256; tab.push_back(e);
    }
    if (tab.empty()) return 0;
    const hipError_t e = T.upload_if_changed(tab, plan->ops.size(), S.st);
    if (e != hipSuccess) { set_error("%s: weight-piece table setup failed: %s", S.who, hipGetErrorString(e)); return (int)e; }
    const int rc = launch_split_all(T.dev, (int)tab.size(), nb, S.c.wsamp(), S.slab_rows() ? plan->n_vi : 0, S.slab_rows() ? S.n_samples : 1, S.c.farena(), S.st);
    if (rc) set_error("%s: weight-piece launch failed: %s", S.who, hipGetErrorString((hipError_t)rc));
    S.x6_ready = rc == 0;
    return rc;
}

}  // namespace

int split_weight_pieces(PassSetup& S, int pass, const float* dz)
{
    S.x6_ready = false;
    if (!S.presample) return 0;
    return pass == 0 ? split_pieces(S, S.plan->x6, pass, dz) : split_pieces(S, S.plan->x6b, pass, dz);
}

extern "C" {

int mfvi_plan_create(const mfvi_tensor_desc* tensors, int n_tensors, const mfvi_op_desc* ops, int n_ops, int input_tensor,
                     int output_tensor, int64_t n_vi, int64_t n_bn, int max_samples, mfvi_plan** plan)
{
    if (!tensors || !ops || !plan) { set_error("plan_create: null argument"); return -1; }
    mfvi_plan* p = new mfvi_plan();
    p->input = input_tensor; p->output = output_tensor; p->n_vi = n_vi; p->n_bn = n_bn; p->max_samples = max_samples;
    if (!validate_program(*p, tensors, n_tensors, ops, n_ops) || !layout_workspace(*p)) { mfvi_plan_destroy(p); *plan = nullptr; return -1; }
    *plan = p;
    return 0;
}

void mfvi_plan_destroy(mfvi_plan* plan)
{
    if (!plan) return;
    for (auto& r : plan->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : plan->free_events) (void)hipEventDestroy(e);
    if (plan->table_dev) (void)hipFree(plan->table_dev);
    if (plan->fin[0].dev) (void)hipFree(plan->fin[0].dev);
    if (plan->x6.dev) (void)hipFree(plan->x6.dev);
    if (plan->x6b.dev) (void)hipFree(plan->x6b.dev);
    if (plan->samp_dev) (void)hipFree(plan->samp_dev);
    if (plan->drop_dev) (void)hipFree(plan->drop_dev);
    if (plan->fit_drop_dev) (void)hipFree(plan->fit_drop_dev);
    for (auto e : plan->fork_events.ev) (void)hipEventDestroy(e);
    for (auto e : plan->fwd_events.ev) (void)hipEventDestroy(e);
    if (plan->join_event) (void)hipEventDestroy(plan->join_event);
    for (auto e : plan->split_ev) if (e) (void)hipEventDestroy(e);
    if (plan->side) (void)hipStreamDestroy(plan->side);
    delete plan;
}

int64_t mfvi_plan_workspace_bytes(const mfvi_plan* plan) { return plan ? plan->total_bytes : -1; }

int mfvi_plan_set_side_stream(mfvi_plan* plan, int enabled)
{
    if (!plan) { set_error("set_side_stream: null plan"); return -1; }
    plan->side_enabled = enabled != 0;
    return 0;
}

int mfvi_plan_grad_split_offset(const mfvi_plan* plan, int first_op, int64_t* offset)
{
    if (!plan || !offset || first_op < 0 || first_op >= (int)plan->ops.size()) { set_error("grad_split_offset: bad arguments"); return -1; }
    if (plan->n_lrt) { set_error("grad_split_offset: plans with local-reparameterisation layers reduce d rho in one pass at the end"); return -1; }
    long long lo = plan->n_vi, head_end = 0;
    for (int i = 0; i < (int)plan->ops.size(); ++i) {
        const OpInfo& o = plan->ops[i];
        if (o.d.type != MFVI_OP_CONV) continue;
        const long long a = o.g.b_off >= 0 ? std::min<long long>(o.g.w_off, o.g.b_off) : o.g.w_off;
        const long long b = std::max<long long>(o.g.w_off + o.n_weights(), o.g.b_off >= 0 ? o.g.b_off + o.g.Cout : 0);
        if (i >= first_op) lo = std::min(lo, a); else head_end = std::max(head_end, b);
    }
    if (head_end > lo) { set_error("grad_split_offset: the parameters of the ops >= %d are not a tail of the flat layout", first_op); return -1; }
    *offset = lo;
    return 0;
}

int mfvi_plan_set_grad_split(mfvi_plan* plan, int first_op, void* comm_stream)
{
    if (!plan) { set_error("set_grad_split: null plan"); return -1; }
    if (first_op < 0) { plan->split_op = -1; plan->split_stream = nullptr; return 0; }
    int64_t off = 0;
    if (mfvi_plan_grad_split_offset(plan, first_op, &off)) return -1;
    for (auto& e : plan->split_ev)
        if (!e) { const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming); if (rc != hipSuccess) { set_error("set_grad_split: event creation failed: %s", hipGetErrorString(rc)); return (int)rc; } }
    plan->split_op = first_op; plan->split_stream = (hipStream_t)comm_stream;
    return 0;
}

int mfvi_plan_set_fits(mfvi_plan* plan, int samples_per_fit, int64_t param_stride, int64_t grad_stride)
{
    if (!plan) { set_error("set_fits: null plan"); return -1; }
    plan->samp_n = 0;
    if (samples_per_fit == 0) { plan->fit_s = 0; plan->fit_pstride = plan->fit_gstride = plan->fit_kstride = 0; return 0; }
    const long long n_params = 2 * plan->n_vi + plan->n_bn;
    if (samples_per_fit < 0 || samples_per_fit > plan->max_samples || param_stride < 0 || grad_stride < 0) {
        set_error("set_fits: samples_per_fit %d outside 0..%d, or a negative stride (%lld, %lld; %lld parameters per fit)",
                  samples_per_fit, plan->max_samples, (long long)param_stride, (long long)grad_stride, n_params); return -1; }
    if (int rc = fits_refusal(plan, "set_fits")) return rc;
    if (samples_per_fit > 1 && plan->zrep_off < 0) {      // room for the net input once per sample, behind everything laid out so far
        const long long n = plan->t[plan->input].numel * plan->max_samples;
        plan->zrep_off = (plan->total_bytes - plan->float_base) / (long long)sizeof(float);
        plan->total_bytes += align_up(n, 64) * (long long)sizeof(float);
    }
    // in-kernel-eps tilings (bit 27) route a layer to the generic kernels, which read one mu / rho: back to the heuristic for those
    for (auto& o : plan->ops)
        if (o.d.type == MFVI_OP_CONV) for (int& t : o.g.tune) if (t & MFVI_TUNE_GENERIC) t = 0;
    plan->fit_s = samples_per_fit; plan->fit_pstride = param_stride; plan->fit_gstride = grad_stride;
    plan->fit_kstride = samples_per_fit;      // sample i draws eps of global sample k0 + i
    return 0;
}

int mfvi_plan_set_fits_sample_stride(mfvi_plan* plan, int64_t stride)
{
    if (!plan) { set_error("set_fits_sample_stride: null plan"); return -1; }
    if (!plan->fit_s) { set_error("set_fits_sample_stride: the plan is not in fits mode (call mfvi_plan_set_fits first; it also restores the default stride)"); return -1; }
    if (stride < 0) { set_error("set_fits_sample_stride: negative stride %lld", (long long)stride); return -1; }
    plan->fit_kstride = stride; plan->samp_n = 0;
    return 0;
}

int mfvi_plan_set_fits_points(mfvi_plan* plan, int enabled)
{
    if (!plan) { set_error("set_fits_points: null plan"); return -1; }
    if (enabled) if (int rc = fits_refusal(plan, "set_fits_points")) return rc;
    plan->fit_points = enabled != 0; plan->samp_n = 0;
    return 0;
}

int mfvi_plan_set_fit_dropout(mfvi_plan* plan, const float* p, int n_fits)
{
    if (!plan) { set_error("set_fit_dropout: null plan"); return -1; }
    if (!p || n_fits == 0) {
        if (p) { set_error("set_fit_dropout: n_fits = 0 with a non-null array (NULL, 0 clears the per-fit probabilities)"); return -1; }
        plan->fit_drop.clear(); return 0;
    }
    if (n_fits < 0 || n_fits > plan->max_samples) { set_error("set_fit_dropout: n_fits %d outside 1..%d", n_fits, plan->max_samples); return -1; }
    for (int f = 0; f < n_fits; ++f)
        if (!(p[f] >= 0.f && p[f] < 1.f)) { set_error("set_fit_dropout: fit %d: dropout probability %g outside [0, 1)", f, (double)p[f]); return -1; }
    if (!plan->fit_drop_dev) {
        const hipError_t e = hipMalloc((void**)&plan->fit_drop_dev, sizeof(float) * plan->max_samples);
        if (e != hipSuccess) { plan->fit_drop_dev = nullptr; set_error("set_fit_dropout: hipMalloc failed: %s", hipGetErrorString(e)); return (int)e; }
    }
    const hipError_t e = hipMemcpy(plan->fit_drop_dev, p, sizeof(float) * n_fits, hipMemcpyHostToDevice);      // (synchronous: p is the caller's)
    if (e != hipSuccess) { set_error("set_fit_dropout: copy failed: %s", hipGetErrorString(e)); return (int)e; }
    plan->fit_drop.assign(p, p + n_fits);
    return 0;
}

int mfvi_plan_set_step_source(mfvi_plan* plan, const int32_t* step_dev)
{
    if (!plan) { set_error("set_step_source: null plan"); return -1; }
    plan->step_dev = step_dev; plan->samp_n = 0;
    return 0;
}

int mfvi_plan_set_capture_mode(mfvi_plan* plan, int enabled)
{
    if (!plan) { set_error("set_capture_mode: null plan"); return -1; }
    plan->capture_mode = enabled != 0;
    return 0;
}

int mfvi_plan_set_param_dtype(mfvi_plan* plan, int dtype)
{
    if (!plan || (dtype != MFVI_PARAM_F32 && dtype != MFVI_PARAM_BF16)) { set_error("set_param_dtype: bad arguments"); return -1; }
    plan->param_dtype = dtype; plan->samp_n = 0;
    return 0;
}

int mfvi_plan_set_bn_eval(mfvi_plan* plan, const float* running)
{
    if (!plan) { set_error("set_bn_eval: null plan"); return -1; }
    plan->bn_eval = running;
    return 0;
}

int mfvi_plan_bn_update_running(const mfvi_plan* plan, const void* workspace, int n_samples, float momentum, float* running, void* stream)
{
    if (!plan || !workspace || !running || n_samples < 1 || n_samples > plan->max_samples || !(momentum >= 0.f && momentum <= 1.f)) {
        set_error("bn_update_running: bad arguments"); return -1; }
    if (plan->bn_eval) { set_error("bn_update_running: the plan is in BatchNorm eval mode (no batch statistics were formed)"); return -1; }
    if (plan->fit_s) { set_error("bn_update_running: fits mode (mfvi_plan_set_fits) does not serve running statistics (one block for all samples)"); return MFVI_ERR_FITS_UNSUPPORTED; }
    const int rc = launch_bn_update_running(plan->table_dev, plan->n_entries, plan->max_c, (const double*)workspace, n_samples, momentum, running, (hipStream_t)stream);
    if (rc) set_error("bn_update_running: %s", hipGetErrorString((hipError_t)rc));
    return rc;
}

int mfvi_plan_set_dropout(mfvi_plan* plan, int enabled)
{
    if (!plan) { set_error("set_dropout: null plan"); return -1; }
    plan->dropout_on = enabled != 0;
    return 0;
}


int mfvi_plan_read_tensor(const mfvi_plan* plan, const void* workspace, int tensor_id, int sample, int which, void* dst, void* stream)
{
    if (!plan || !workspace || !dst) { set_error("read_tensor: null argument"); return -1; }
    if (tensor_id < 0 || tensor_id >= (int)plan->t.size() || tensor_id == plan->input || tensor_id == plan->output) {
        set_error("read_tensor: tensor %d is not a workspace tensor", tensor_id); return -1; }
    if (sample < 0 || sample >= plan->max_samples) { set_error("read_tensor: bad sample"); return -1; }
    const TensorInfo& t = plan->t[tensor_id];
    const char* ws = (const char*)workspace;
    const void* src; size_t bytes;
    if (which == 0 || which == 1) {
        const float* base = (const float*)(ws + plan->float_base) + (which == 0 ? t.act_off : t.ga_off);
        src = base + (long long)sample * t.numel; bytes = sizeof(float) * t.numel;
    } else if (which == 2 || which == 3) {
        if (!t.d.has_bn) { set_error("read_tensor: tensor %d has no BatchNorm", tensor_id); return -1; }
        const double* base = (const double*)ws + (which == 3 ? plan->stats_doubles : 0) + t.stats_off;
        src = base + (long long)sample * t.d.C * 2; bytes = sizeof(double) * t.d.C * 2;
    } else { set_error("read_tensor: bad selector %d", which); return -1; }
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) { set_error("read_tensor: %s", hipGetErrorString(e)); return (int)e; }
    return 0;
}

int mfvi_plan_profile(mfvi_plan* plan, int mode, int op, int pass)
{
    if (!plan || mode < 0 || mode > 2) { set_error("plan_profile: bad arguments"); return -1; }
    plan->prof_mode = mode; plan->prof_op = op; plan->prof_pass = pass;
    return 0;
}

int mfvi_plan_profile_read(mfvi_plan* plan, int capacity, int* n_records, int* ops, int* passes, float* ms)
{
    if (!plan || capacity < 0 || !n_records) { set_error("plan_profile_read: bad arguments"); return -1; }
    int n = 0;
    for (auto& r : plan->recs) {
        float t = 0.f;
        hipError_t e = hipEventSynchronize(r.b);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, r.a, r.b);
        if (e != hipSuccess) { set_error("plan_profile_read: %s", hipGetErrorString(e)); return (int)e; }
        if (n < capacity) { ops[n] = r.op; passes[n] = r.pass; ms[n] = t; }
        ++n;
        plan->free_events.push_back(r.a); plan->free_events.push_back(r.b);
    }
    plan->recs.clear();
    *n_records = n;      /* may exceed capacity: only the first `capacity` were written */
    return 0;
}

int mfvi_plan_last_kernel(const mfvi_plan* plan, int op, int which)
{
    if (!plan || op < 0 || op >= (int)plan->ops.size() || which < 0 || which > 2 || plan->ops[op].d.type != MFVI_OP_CONV) return -1;
    return plan->ops[op].family[which];
}

int mfvi_plan_get_tune(const mfvi_plan* plan, int op, int which)
{
    if (!plan || op < 0 || op >= (int)plan->ops.size() || which < 0 || which > 2 || plan->ops[op].d.type != MFVI_OP_CONV) return -1;
    return plan->ops[op].g.tune[which];
}

int mfvi_plan_set_tune(mfvi_plan* plan, int op, int which, int tune)
{
    if (!plan || op < 0 || op >= (int)plan->ops.size() || which < 0 || which > 2 || tune < 0 || plan->ops[op].d.type != MFVI_OP_CONV) {
        set_error("plan_set_tune: bad arguments"); return -1; }
    plan->ops[op].g.tune[which] = tune;
    return 0;
}

const char* mfvi_last_error(void) { return g_err; }
int mfvi_abi_version(void) { return MFVI_ABI_VERSION; }

}  // extern "C"
