// Internals shared by the plan sources: plan.hip (types, validation, layout, setters), plan_forward.hip, plan_backward.hip, plan_autotune.hip.
#pragma once
#include "common.h"
#include "../../include/mfvi_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <vector>

struct TensorInfo {
    mfvi_tensor_desc d;
    long long numel = 0;
    long long act_off = -1, ga_off = -1;       // floats, from the float arena base
    long long stats_off = -1;                  // doubles, inside the fwd-stats block (same offset in the bsums block)
    long long drop_off = -1;                   // floats: Dropout2d factors [max_samples][C] (drop_p > 0 only)
    int producer = -1;
    std::vector<int> consumers;                // op indices, forward order
};

// blocks of `quads` weight quads that cover n_w weights and n_b biases (sampling and grad_finalize kernels)
inline int quads_to_blocks(int n_w, int n_b, int quads) { return ((n_w >> 2) + ((n_b + 3) >> 2) + quads - 1) / quads; }

struct OpInfo {
    mfvi_op_desc d;
    ConvGeom g;
    long long scratch_off = -1;                // floats: padded input-gradient scratch of this conv
    long long scratch2_off = -1, s2_off = -1;  // LRT: padded scratch of the variance convolution's input gradient; s2 = conv(v^2, sigma^2) kept for the backward
    long long part_off = -1, part_stride = 0;  // floats: partial-dW slabs of the MFMA backward-weight kernel [strip][sample][stride]
    int max_strips = 0;
    long long x6w_off = -1;                    // floats: split weight pieces of the bf16x6 forward (conv_x6.hip), -1: shape not served
    long long x6bw_off = -1;                   // floats: split weight pieces of the bf16x6 backward-data (conv_bwd_x6.hip), -1: shape not served
    bool in_slab = false;                      // its weights are drawn once per pass into the sampled-weight slab (the MFMA-served layers)
    mutable int family[3] = {0, 0, 0};         // kernel family of the last forward / backward-data / backward-weight launch (mfvi_plan_last_kernel)
    long long n_weights() const { return (long long)g.Cout * g.Cin * g.ks * g.ks; }
    int n_bias() const { return g.b_off >= 0 ? g.Cout : 0; }
    long long padded_per_sample() const { const int P = g.ks / 2; return (long long)g.Cin * (g.H + 2 * P) * (g.W + 2 * P); }      // the padded input gradient
};

// Untimed events handed out in order during a pass and reused by the next one
struct EventPool {
    std::vector<hipEvent_t> ev; size_t used = 0;
    void reset() { used = 0; }
    hipError_t next(hipEvent_t* e)
    {
        if (used == ev.size()) { hipEvent_t n; const hipError_t rc = hipEventCreateWithFlags(&n, hipEventDisableTiming); if (rc != hipSuccess) return rc; ev.push_back(n); }
        *e = ev[used++]; return hipSuccess;
    }
};

// An event that should ride on the dispatch packet of a launch (Launch::stop) where that launch goes through mfvi_launch: armed on the op's
// Launch right before the op's last kernel, settled behind it.  sent == false afterwards (a launcher that took a plain hipLaunchKernelGGL, or
// riding is off): the event is recorded the ordinary way (record_unless_sent).  Off in capture mode (fork / join as plain records in a HIP
// graph), with per-kernel profiling (mode 1 brackets every launch with its own events) and with MFVI_FORK_ON_PACKET=0.
struct PacketEvent {
    bool on_packet; hipEvent_t ev = nullptr; bool sent = false;
    void arm(Launch& L, hipEvent_t e) { ev = e; sent = false; L.stop = on_packet ? e : nullptr; }
    void settle(Launch& L) { sent = on_packet && ev && L.stop == nullptr; L.stop = nullptr; }
    void clear() { ev = nullptr; sent = false; }
};
inline hipError_t record_unless_sent(hipEvent_t ev, hipStream_t s, bool sent) { return sent ? hipSuccess : hipEventRecord(ev, s); }
// work enqueued on `to` from here on runs behind everything enqueued on `from` so far
inline hipError_t fork(hipStream_t from, hipStream_t to, hipEvent_t ev, bool already_sent = false)
{
    const hipError_t e = record_unless_sent(ev, from, already_sent);
    return e != hipSuccess ? e : hipStreamWaitEvent(to, ev, 0);
}

// A small device table with the host copy of its last upload: uploaded again only when it differs (tilings change only when the plan is
// (re)tuned, so each table is uploaded once in steady state).
template <typename E> struct DeviceTable {
    E* dev = nullptr; std::vector<E> uploaded;
    bool holds(const std::vector<E>& tab) const { return tab.size() == uploaded.size() && memcmp(tab.data(), uploaded.data(), sizeof(E) * tab.size()) == 0; }
    hipError_t upload_if_changed(const std::vector<E>& tab, size_t capacity, hipStream_t st)
    {
        hipError_t e = hipSuccess;
        if (!dev) e = hipMalloc((void**)&dev, sizeof(E) * capacity);
        if (e != hipSuccess || holds(tab)) return e;
        // the previous upload may still be reading the vector about to be reassigned (pageable source of an async copy)
        if (!uploaded.empty()) (void)hipStreamSynchronize(st);
        uploaded = tab;      // (copied from the plan-owned vector: it outlives the asynchronous copy, the caller's may not)
        e = hipMemcpyAsync(dev, uploaded.data(), sizeof(E) * tab.size(), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) uploaded.clear();
        return e;
    }
};

struct mfvi_plan {
    std::vector<TensorInfo> t;
    std::vector<OpInfo> ops;
    int input = -1, output = -1, max_samples = 0;
    long long n_vi = 0, n_bn = 0;
    long long stats_doubles = 0;               // per block (fwd stats | bsums), for max_samples
    const void* bsums_clean_ws = nullptr;      // workspace whose BN-backward sums the last forward zeroed (one memset for both blocks) with no backward since
    long long float_base = 0;                  // byte offset of the float arena
    long long total_bytes = 0;
    BnGradEntry* table_dev = nullptr; int n_entries = 0, max_c = 1;
    SampleEntry* samp_dev = nullptr; int n_samp = 0, samp_blocks = 0;    // layers whose weights are drawn once per pass
    long long wsamp_off = -1;                  // floats: sampled weights [max_samples][n_vi]
    DeviceTable<X6SplitEntry> x6;              // table of the bf16x6 forward layers' weight split (conv_x6.hip)
    DeviceTable<X6BSplitEntry> x6b;            // the same for the bf16x6 backward-data layers (conv_bwd_x6.hip)
    int param_dtype = MFVI_PARAM_F32;          // storage of mu / rho handed to forward / backward (MFVI_PARAM_BF16: bf16_t arrays)
    const int32_t* step_dev = nullptr;         // device-resident step counter (mfvi_plan_set_step_source): the `step` argument of forward / backward is an offset to it
    bool capture_mode = false;                 // the calls are being captured into a HIP graph: fork / join events as plain records (no events on kernel packets)
    int n_generic = 0;                         // conv layers outside the sampling table (served by the generic fp32 kernels)
    long long p32_off = -1;                    // floats: [mu | rho] expanded to float32 for those kernels when mu / rho are bf16
    const float* bn_eval = nullptr;            // BatchNorm in eval mode: running statistics used by mfvi_forward (nullptr: batch statistics)
    // fits mode (mfvi_plan_set_fits): the samples of a call are n_samples / fit_s independent fits of fit_s samples each;
    // mu / rho / bn of fit j lie j * fit_pstride floats behind the pointers of the call, its gradients j * fit_gstride.  0: one fit (off)
    int fit_s = 0; long long fit_pstride = 0, fit_gstride = 0;
    // fits mode: the eps / dropout sample index of fit j's draw s is k0 + j * fit_kstride + s (mfvi_plan_set_fits_sample_stride).
    // mfvi_plan_set_fits puts it back to fit_s, which is k0 + i for sample i; any other value serves forward passes only
    long long fit_kstride = 0;
    uint32_t fit_kdelta() const { return (uint32_t)(fit_kstride - fit_s); }      // what the kernels add per fit (fit_sample_index)
    // fits mode with point weights (mfvi_plan_set_fits_points): a sample_weights = 0 pass writes every sample's slab row with
    // its fit's mu and runs on those rows like a sampled pass.  Off (the default): fits mode refuses sample_weights = 0
    bool fit_points = false;
    // fits mode: Dropout2d probability per fit (mfvi_plan_set_fit_dropout); empty: every fit draws with the tensors' own drop_p
    std::vector<float> fit_drop; float* fit_drop_dev = nullptr;
    long long zrep_off = -1;                   // floats: the net input once per SAMPLE [max_samples][Cin][H][W] (fit_s > 1: the kernels address it by sample)
    int n_lrt = 0;                             // local-reparameterisation layers
    long long sig2_off = -1, dsig2_off = -1;   // floats [n_vi] each: softplus(rho)^2 of this pass / gradient wrt it
    long long lrt_tmp_off = -1, lrt_tmp_n = 0; // floats: mean-convolution output (forward) / ds2 (backward) of the LRT layer in flight
    // identity of the draw currently held in the sampled-weight slab (set by forward, reused by the matching backward)
    const void* samp_mu = nullptr; const void* samp_rho = nullptr; const void* samp_ws = nullptr;
    uint64_t samp_seed = 0; uint32_t samp_step = 0, samp_k0 = 0; int samp_n = 0;      // samp_n: +n a draw for n samples, -n w = mu (one row; n rows in a points pass of fits mode)
    DropEntry* drop_dev = nullptr; int n_drop = 0; bool dropout_on = true;   // Dropout2d layers (MC-dropout sibling)
    // Backward-weight launches are off the critical path of the backward pass (only grad_finalize needs them): they run on a side
    // stream of the plan, forked per layer behind the event that marks "dy of this layer is final" and joined before grad_finalize,
    // so they fill the CUs the latency-bound backward-data / fold kernels of the small maps leave idle.
    hipStream_t side = nullptr; EventPool fork_events; hipEvent_t join_event = nullptr; bool side_enabled = true;
    EventPool fwd_events;                      // forward pass: skip-branch convolutions beside the down path (MFVI_FWD_FORK)
    // Tables of the layers whose partial dW slabs grad_finalize reduces.
    // Gradient split for an overlapped exchange (mfvi_plan_set_grad_split): the backward pass reduces the weight gradients of the ops
    // >= split_op on split_stream as soon as their backward-weight kernels have been enqueued, the rest at the end as before.
    int split_op = -1; hipStream_t split_stream = nullptr; hipEvent_t split_ev[2] = {nullptr, nullptr}; int n_conv = 0;
    // three tables, each with its own device slot (one allocation: fin[0].dev + {0, 1, 2} * n_conv) and cached host copy: the whole pass (no
    // split), the early group of a split pass, the late group of a split pass.  An engine that splits only the LAST launch of an iteration
    // (K_local > samples per launch) alternates between "whole" and "early + late": with one slot shared by "whole" and "late" the cache
    // missed twice per iteration, and the reassigned host vector was the source of a copy still in flight.
    enum { FIN_WHOLE = 0, FIN_EARLY = 1, FIN_LATE = 2 };
    DeviceTable<GradFinEntry> fin[3];
    // optional per-kernel timing with HIP events on the caller's stream (bench.py's roofline leg)
    struct Rec { int op, pass; hipEvent_t a, b; };
    int prof_mode = 0, prof_op = -1, prof_pass = -1;      // 0 off, 1 every kernel, 2 only (prof_op, prof_pass)
    std::vector<Rec> recs;
    std::vector<hipEvent_t> free_events;
    bool split_active(hipStream_t st) const { return split_op >= 0 && split_stream && split_stream != st; }
};

// The plan-side environment switches, each read once per process.
struct PlanSwitches {
    // MFVI_FOLD_FUSION=0: 1x1 backward-data always goes through the padded-gradient scratch + finalize_dx (A/B and parity cross-checks)
    bool fold_fusion;
    // MFVI_FOLD_FUSION3=0: 3x3 stride-1 backward-data keeps the padded-gradient scratch + finalize_dx (A/B and parity cross-checks)
    bool fold_fusion3;
    // MFVI_FWD_FORK: a skip-branch convolution (its only consumer is a later concat) on a map of up to this many pixels (default 128 x 128;
    // 0 = never) runs on the plan's side stream beside the down path of its scale and is joined in front of that concat: at those sizes both
    // are latency-bound launches that leave most of the chip idle (with the events on the kernels' packets: 3.306 ms per iteration without,
    // 3.282 / 3.274 / 3.279 with the maps up to 64^2 / 128^2 / 256^2).  The side stream exists once a backward pass has run.
    long long fwd_fork;
    // MFVI_FORK_ON_PACKET=0: fork / join events always by hipEventRecord, never on a kernel's packet (PacketEvent)
    bool fork_on_packet;
    // MFVI_SIDE_STREAM=0: the backward-weight kernels on the caller's stream like everything else
    bool side_stream;
    // MFVI_SIDE_MAXPIX: layers with more output pixels per sample keep their backward-weight on the caller's stream (a kernel that
    // fills the chip by itself gains nothing from sharing it, and its launch duration stays meaningful for the roofline)
    long long side_maxpix;
    // MFVI_SIDE_PRIO=0: the side stream at the default priority instead of the lowest (the caller's stream carries the critical path, the
    // side stream only fills what it leaves idle)
    bool side_low_prio;
    // MFVI_FUSE_SKIP_BWD=0: the narrow 1x1 skip convolution keeps a backward-data launch of its own instead of being formed inside the
    // fold of the tensor it shares (A/B, parity cross-checks)
    bool fuse_skip_bwd;
};
const PlanSwitches& switches();

bool fail(const char* fmt, ...);      // sets the error string, returns false
bool check_call(const mfvi_plan* p, int n_samples, const void* ws);
// fits mode: what it does not serve in the plan's current state (message set), else nullptr-equivalent 0.  One predicate for mfvi_plan_set_fits and every pass
int fits_refusal(const mfvi_plan* p, const char* who);

enum { PASS_FWD = 0, PASS_BWD_WEIGHT = 1, PASS_BWD_DATA = 2, PASS_FINALIZE = 3, PASS_CONCAT_BWD = 4, PASS_GRAD_FINALIZE = 5, PASS_SAMPLE = 6 };

struct ProfScope {
    mfvi_plan* p; hipStream_t st; bool on; hipEvent_t a, b; int op, pass;
    ProfScope(mfvi_plan* p_, int op_, int pass_, hipStream_t st_) : p(p_), st(st_), on(false), op(op_), pass(pass_)
    {
        on = p->prof_mode == 1 || (p->prof_mode == 2 && p->prof_op == op && p->prof_pass == pass);
        if (!on) return;
        auto get = [&]() { hipEvent_t e; if (!p->free_events.empty()) { e = p->free_events.back(); p->free_events.pop_back(); } else (void)hipEventCreate(&e); return e; };
        a = get(); b = get();
        (void)hipEventRecord(a, st);
    }
    ~ProfScope() { if (on) { (void)hipEventRecord(b, st); p->recs.push_back({op, pass, a, b}); } }
};

struct Ctx {
    const mfvi_plan& p; char* ws; const float* bn; const float* z; int n;
    int fit_s = 0; long long gamma_fstride = 0, z_sstride = 0;      // fits mode (set by pass_setup): per-fit BatchNorm parameters, one net input per sample
    double* fstats() const { return (double*)ws; }
    double* bsums() const { return (double*)ws + p.stats_doubles; }
    float* farena() const { return (float*)(ws + p.float_base); }
    float* wsamp() const { return p.wsamp_off >= 0 ? farena() + p.wsamp_off : nullptr; }
    TView view(int i, const float* out_ptr = nullptr) const
    {
        const TensorInfo& t = p.t[i]; TView v;
        if (i == p.input) { v.data = z; v.sstride = z_sstride; }
        else if (i == p.output) { v.data = out_ptr; v.sstride = t.numel; }
        else { v.data = farena() + t.act_off; v.sstride = t.numel; }
        v.C = t.d.C; v.H = t.d.H; v.W = t.d.W;
        v.stats = t.d.has_bn ? fstats() + t.stats_off : nullptr;
        v.gamma = t.d.has_bn ? bn + t.d.bn_off : nullptr;
        v.eps = t.d.eps; v.slope = t.d.slope; v.act = t.d.has_act;
        v.drop = (t.drop_off >= 0 && p.dropout_on) ? farena() + t.drop_off : nullptr;
        v.fit_s = fit_s; v.gamma_fstride = gamma_fstride;
        return v;
    }
    GView gview(int i, const float* dout) const
    {
        const TensorInfo& t = p.t[i]; GView g;
        g.ga = (i == p.output) ? dout : farena() + t.ga_off; g.gstride = t.numel;
        g.y = (i == p.output) ? nullptr : farena() + t.act_off; g.ystride = t.numel;
        g.C = t.d.C; g.H = t.d.H; g.W = t.d.W;
        g.stats = t.d.has_bn ? fstats() + t.stats_off : nullptr;
        g.bsums = t.d.has_bn ? bsums() + t.stats_off : nullptr;
        g.gamma = t.d.has_bn ? bn + t.d.bn_off : nullptr;
        g.eps = t.d.eps;
        g.drop = (t.drop_off >= 0 && p.dropout_on) ? farena() + t.drop_off : nullptr;
        g.fit_s = fit_s; g.gamma_fstride = gamma_fstride;
        return g;
    }
    double* bsums_of(int tid) const { return p.t[tid].d.has_bn ? bsums() + p.t[tid].stats_off : nullptr; }      // BN-backward sums of a tensor
    float* grad_of(int tid, float* dz) const { return tid == p.input ? dz : farena() + p.t[tid].ga_off; }          // where its gradient goes
    bool need_dx(const OpInfo& o, const float* dz) const { return o.d.in0 != p.input || dz != nullptr; }          // a conv of the net input: only when dz is asked for
    OutDesc out_desc(const OpInfo& o, float* out, bool with_stats = true) const      // raw output of a forward op (+ its BN statistics to accumulate)
    {
        const TensorInfo& y = p.t[o.d.out]; OutDesc od;
        od.data = (o.d.out == p.output) ? out : farena() + y.act_off; od.sstride = y.numel;
        od.stats = (y.d.has_bn && with_stats) ? fstats() + y.stats_off : nullptr;
        return od;
    }
    FoldFuse fold_fuse(const OpInfo& o, float* dz) const      // the fold of the conv's input tensor, for a backward-data kernel that does it itself
    {
        FoldFuse ff; ff.x = view(o.d.in0); ff.ga = grad_of(o.d.in0, dz); ff.ga_sstride = p.t[o.d.in0].numel; ff.bsums = bsums_of(o.d.in0);
        return ff;
    }
};

// What forward, backward and the autotuner share of a pass: the checked arguments, the float32 view of the parameters, the weights as the
// conv dispatch wants them, the bf16x6 weight pieces.
struct PassSetup {
    mfvi_plan* plan; const char* who; hipStream_t st; Ctx c;
    const void* mu_v; const void* rho_v; int n_samples, sample_weights;
    bool bf16;
    const float* mu = nullptr; const float* rho = nullptr;      // float32 view of mu / rho for the generic kernels (nullptr: bf16 parameters, no generic layer)
    // MFMA-served layers: every weight drawn once per (layer, sample) into the slab; without sampling the kernels read mu (stride 0)
    // (bf16 parameters: the slab also serves w = mu, as one float32 copy shared by all samples)
    bool presample = false;
    bool points = false;        // fits mode, sample_weights = 0 (mfvi_plan_set_fits_points): the slab holds one row per sample, each its fit's mu
    bool slab_rows() const { return sample_weights || points; }      // one slab row per sample (else one row, w = mu, shared by all samples)
    RngKey key; ConvWeights W;
    bool x6_ready = false;      // a pass-wide launch split the weight pieces of this pass's bf16x6 layers (split_weight_pieces)
};
// expand: launch the float32 expansion of bf16 parameters for the generic layers (else mu = rho = nullptr for a bf16 plan).  <> 0: error set
int pass_setup(PassSetup& S, bool expand, uint64_t seed, uint32_t step, uint32_t k0);
// Weight pieces of the layers whose forward (pass 0) / backward-data (pass 1; dz as given to mfvi_backward) runs on a bf16x6 kernel with the
// tilings of this pass: one launch behind the draw for all of them; sets S.x6_ready
int split_weight_pieces(PassSetup& S, int pass, const float* dz);

// conv2d(reflection_pad(view), w, b) with EXPLICIT float32 weights (w_base + g.w_off, bias at w_base + g.b_off), no sampling: the two
// convolutions of a local-reparameterisation layer.  MFMA kernel when the shape is served, else the generic one (w = "mu", eval branch).
inline ConvWeights plain_weights(const float* w_base) { return ConvWeights{w_base, 0, w_base, w_base, RngKey{}, 0}; }

// The conv's input feeds nothing else: backward-data with the fold in its epilogue (no scratch round trip, no finalize_dx launch; 3x3 stride-1
// layers compute on the un-padded domain with the reflection adjoint on the pixel operand).  One predicate for mfvi_backward and the autotuner
inline bool fused_fold(const mfvi_plan& p, const OpInfo& o, bool need_dx)
{
    return need_dx && (o.g.ks == 1 || (o.g.ks == 3 && o.g.stride == 1 && switches().fold_fusion3)) && p.t[o.d.in0].consumers.size() == 1 && use_mfma() && switches().fold_fusion;
}

inline RngKey base_key(uint64_t seed, uint32_t step, uint32_t k0, const int32_t* step_dev = nullptr)
{
    RngKey k; k.k0 = (uint32_t)seed; k.k1 = (uint32_t)(seed >> 32); k.stream = 0; k.sample = k0; k.step = step; k.step_dev = step_dev; return k;
}
