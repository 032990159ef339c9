// mfvi_backward: the backward pass of a plan (include/mfvi_hip.h) — the ops last to first on the caller's stream, their backward-weight
// kernels forked onto the plan's side stream, the partial weight gradients reduced at the end (or, with a gradient split, in two groups).
#include "plan_internal.h"

namespace {

struct Backward {
    PassSetup S; const float* dout; float* dmu; float* drho; float* dbn; float* dz;
    hipStream_t side = nullptr;            // stream of the forked backward-weight kernels; == S.st: everything on the caller's stream
    // The fork event of the NEXT op's backward-weight kernel rides on the packet of this op's last launch on the caller's stream, the join
    // event on the side stream's last launch (the backward-weight kernel of the last op that forks)
    PacketEvent next_fork{false}, join{false};
    int last_fork_op = -1;
    std::vector<GradFinEntry> fin;         // layers whose dW went to partial slabs in this pass and is not reduced yet
    bool bn_done = false;                  // the BatchNorm parameter gradients went out with the last grad_finalize launch

    // Op j's backward-weight kernel goes to the side stream.  Not the layers that read the network input (unless dz is asked for): they have
    // no backward-data, so their backward-weight kernel is all the caller's stream would do for them and it runs there — at the end of the
    // pass the side stream is still working off the last layers' kernels while the caller's stream would sit idle (a ~100 us tail of three
    // serial launches otherwise).  Nor the layers above MFVI_SIDE_MAXPIX (PlanSwitches::side_maxpix)
    bool will_fork(int j) const
    {
        if (j < 0 || side == S.st || S.plan->ops[j].d.type != MFVI_OP_CONV) return false;
        const OpInfo& oj = S.plan->ops[j];
        return S.c.need_dx(oj, dz) && (long long)oj.g.Ho * oj.g.Wo <= switches().side_maxpix;
    }
    // right before the LAST launch of op i on the caller's stream: the fork event of op i - 1 rides on it
    int arm(Launch& L, int i)
    {
        L.stop = nullptr; next_fork.sent = false;
        if (!next_fork.on_packet || !will_fork(i - 1)) return 0;
        const hipError_t e = next_fork.ev ? hipSuccess : S.plan->fork_events.next(&next_fork.ev);
        if (e != hipSuccess) { set_error("backward: event creation failed: %s", hipGetErrorString(e)); return -1; }
        next_fork.arm(L, next_fork.ev);
        return 0;
    }
    void settle(Launch& L) { next_fork.settle(L); }      // behind that launch: sent (the event is on the kernel's packet) or not
};

// Everything in front of the last op: cleared sums, the weights of this pass, the bf16x6 weight pieces, the side stream
int begin_backward(Backward& B, void* workspace, uint64_t seed, uint32_t step, uint32_t k0)
{
    PassSetup& S = B.S; mfvi_plan* plan = S.plan; const Ctx& c = S.c; hipStream_t st = S.st;
    if (plan->stats_doubles && plan->bsums_clean_ws != workspace) {      // a second backward after one forward (gradients accumulate): the sums start from zero again
        hipError_t e = hipMemsetAsync(c.bsums(), 0, sizeof(double) * plan->stats_doubles, st);
        if (e != hipSuccess) { set_error("backward: memset failed: %s", hipGetErrorString(e)); return (int)e; }
    }
    plan->bsums_clean_ws = nullptr;
    if (plan->n_lrt && S.sample_weights) {
        if (!S.rho) { set_error("backward: local-reparameterisation layers take float32 parameters"); return -1; }
        hipError_t e = hipMemsetAsync(c.farena() + plan->dsig2_off, 0, sizeof(float) * plan->n_vi, st);
        if (e != hipSuccess) { set_error("backward: memset failed: %s", hipGetErrorString(e)); return (int)e; }
    }
    // the weights of this pass: the slab still holds them when the preceding forward was this very pass (same parameter
    // buffers, counters, sample range and workspace); otherwise they are re-drawn from the same counters
    const bool held = plan->samp_mu == S.mu_v && plan->samp_rho == S.rho_v && plan->samp_ws == workspace && plan->samp_seed == seed &&
                      plan->samp_step == step && plan->samp_k0 == k0 && plan->samp_n == (S.sample_weights ? S.n_samples : -S.n_samples);
    if (S.presample && !held) {
        ProfScope ps(plan, -1, PASS_SAMPLE, st);
        const int rc = launch_sample_weights(plan->samp_dev, plan->n_samp, plan->samp_blocks, S.mu_v, S.rho_v, S.key, S.slab_rows() ? S.n_samples : 1, c.wsamp(),
                                             plan->n_vi, st, S.bf16, S.sample_weights, nullptr, 0, plan->fit_s, plan->fit_pstride);
        if (rc) { set_error("backward: sample_weights launch failed: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    }
    // one use per draw: the parameters are updated in place in the same buffers, so a later backward with the same counters (a second
    // backward through a retained graph, a caller re-using a step index after an optimizer step) must re-draw from what mu / rho hold now
    plan->samp_n = 0;
    const int rc = split_weight_pieces(S, 1, B.dz);
    if (rc) return rc;
    B.side = st;
    if (switches().side_stream && plan->side_enabled) {
        if (!plan->side) {
            int prio_least = 0, prio_greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
            hipError_t e = hipStreamCreateWithPriority(&plan->side, hipStreamNonBlocking, switches().side_low_prio ? prio_least : 0);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&plan->join_event, hipEventDisableTiming);
            if (e != hipSuccess) { set_error("backward: side stream setup failed: %s", hipGetErrorString(e)); return (int)e; }
        }
        B.side = plan->side;
    }
    plan->fork_events.reset();
    B.next_fork.on_packet = B.join.on_packet = switches().fork_on_packet && !plan->capture_mode && plan->prof_mode != 1;
    for (int j = 0; j < (int)plan->ops.size(); ++j) if (B.will_fork(j)) { B.last_fork_op = j; break; }
    return 0;
}

// Gradient wrt tensor `tid` once every consumer has written its padded input gradient: reflection-pad adjoint fold, sum over the
// consumers (an LRT consumer contributes two sources, the variance branch with the factor 2 * view(x)), LeakyReLU', BN-backward sums.
// inline_op >= 0: that consumer (a narrow 1x1 convolution) wrote no padded gradient — its backward-data is formed inside the fold from its
// output gradient gy1 and its weights in the slab (launch_finalize_dx_inline1x1)
int fold_consumers(const Backward& B, int tid, int op_index, Launch& L, int inline_op = -1, const GView* gy1 = nullptr)
{
    const PassSetup& S = B.S; const Ctx& c = S.c; mfvi_plan* plan = S.plan;
    const TensorInfo& x = plan->t[tid];
    FoldSrc srcs[MAX_FOLD_SRC]; int ns = 0;
    for (int ci : x.consumers) {
        if (ci == inline_op) continue;
        const OpInfo& co = plan->ops[ci];
        srcs[ns++] = FoldSrc{c.farena() + co.scratch_off, co.padded_per_sample(), co.g.ks / 2, 0};
        if (co.d.type == MFVI_OP_CONV_LRT && S.sample_weights) srcs[ns++] = FoldSrc{c.farena() + co.scratch2_off, co.padded_per_sample(), co.g.ks / 2, 1};
    }
    ProfScope ps(plan, op_index, PASS_FINALIZE, L.st);
    if (inline_op >= 0) {
        if (ns != 1) return CONV_NOT_SERVED;
        const OpInfo& io = plan->ops[inline_op];
        return launch_finalize_dx_inline1x1(srcs[0], *gy1, S.W.w + io.g.w_off, S.W.wstride, io.g.Cout, c.view(tid), c.grad_of(tid, B.dz), x.numel, c.bsums_of(tid), S.n_samples, L);
    }
    return launch_finalize_dx(srcs, ns, c.view(tid), c.grad_of(tid, B.dz), x.numel, c.bsums_of(tid), S.n_samples, L);
}

// reduction of the partial dW slabs of the layers collected in B.fin into dmu / drho, on stream fs through the table `slot` of the plan
int finalize_grads(Backward& B, hipStream_t fs, int slot, bool with_bn = false)
{
    const PassSetup& S = B.S; mfvi_plan* plan = S.plan; std::vector<GradFinEntry>& fin = B.fin;
    if (fin.empty()) return 0;
    // longest blocks first: a block's work grows with the number of pixel strips of its layer
    std::stable_sort(fin.begin(), fin.end(), [](const GradFinEntry& a, const GradFinEntry& b) { return a.strips > b.strips; });
    int fin_blocks = 0;
    for (auto& e : fin) { e.first_block = fin_blocks; fin_blocks += quads_to_blocks(e.n_w, e.n_b, GRAD_FIN_QUADS); }
    ProfScope ps(plan, -1, PASS_GRAD_FINALIZE, fs);
    DeviceTable<GradFinEntry>& T = plan->fin[slot];
    if (!T.holds(fin) && getenv("MFVI_DEBUG_FIN")) for (auto& e : fin) fprintf(stderr, "fin layer %d n_w %d strips %d first_block %d\n", e.layer_id, e.n_w, e.strips, e.first_block);
    const hipError_t e = T.upload_if_changed(fin, plan->n_conv, fs);
    if (e != hipSuccess) { set_error("backward: gradient table upload failed: %s", hipGetErrorString(e)); return (int)e; }
    const int rc = launch_grad_finalize(T.dev, (int)fin.size(), fin_blocks, S.c.farena(), S.rho_v, S.key, S.sample_weights, S.n_samples, B.dmu, B.drho, fs, S.bf16,
                                        with_bn ? plan->table_dev : nullptr, with_bn ? plan->n_entries : 0, S.c.bsums(), B.dbn, plan->fit_s, plan->fit_pstride,
                                        plan->fit_gstride);
    if (rc) { set_error("backward: grad_finalize launch failed: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    if (with_bn && plan->n_entries) B.bn_done = true;
    fin.clear();
    return 0;
}

// Gradient split: every kernel that writes a weight gradient of the ops >= split_op (partial slabs on the side stream, generic kernels'
// atomics on either stream) has been enqueued; the exchange stream waits for them and reduces that group now
int reduce_early_group(Backward& B)
{
    mfvi_plan* plan = B.S.plan;
    hipError_t e = fork(B.S.st, plan->split_stream, plan->split_ev[0]);
    if (e == hipSuccess && B.side != B.S.st) e = fork(B.side, plan->split_stream, plan->split_ev[1]);
    if (e != hipSuccess) { set_error("backward: gradient split failed: %s", hipGetErrorString(e)); return (int)e; }
    return finalize_grads(B, plan->split_stream, mfvi_plan::FIN_EARLY);
}

// autograd of LRTLayer.forward: d act_mu = dy, d act_var = dy * eps / (2 std); the two convolutions' weight gradients go to
// d mu and (through sigma^2 = softplus(rho)^2) to d rho; their input gradients meet in the fold, the variance branch with
// the factor 2 * view(x) of its x**2 operand.  Caller's stream throughout (an alternative estimator, not the hot path).
int backward_lrt(Backward& B, int i, const OpInfo& o, Launch& L)
{
    const PassSetup& S = B.S; const Ctx& c = S.c; mfvi_plan* plan = S.plan; hipStream_t st = S.st; const int n_samples = S.n_samples;
    const GView gy = c.gview(o.d.out, B.dout);
    const TView xin = c.view(o.d.in0);
    const TensorInfo& yt = plan->t[o.d.out];
    const long long per = o.padded_per_sample();
    const bool need_dx = c.need_dx(o, B.dz);
    if (!S.mu) { set_error("backward: local-reparameterisation layers take float32 parameters"); return -1; }
    RngKey none{};
    int rc;
    { ProfScope ps(plan, i, PASS_BWD_WEIGHT, st);
      rc = launch_conv_bwd_weight(xin, gy, o.g, S.rho, none, 0, B.dmu, B.drho, n_samples, st); }          // d mu, d mu_b
    if (!rc && need_dx) { ProfScope ps(plan, i, PASS_BWD_DATA, st);
      rc = conv_backward_data(L, gy, o.g, plain_weights(S.mu), c.farena() + o.scratch_off, per, n_samples); }
    if (!rc && S.sample_weights) {
        float* ds2 = c.farena() + plan->lrt_tmp_off;
        rc = launch_lrt_ds2(gy, c.farena() + o.s2_off, yt.numel, S.key, o.g.layer_id, ds2, n_samples, st);
        GView g2{}; g2.ga = ds2; g2.gstride = yt.numel; g2.y = nullptr; g2.ystride = 0; g2.C = yt.d.C; g2.H = yt.d.H; g2.W = yt.d.W;
        g2.stats = nullptr; g2.bsums = nullptr; g2.gamma = nullptr; g2.eps = 0.f; g2.drop = nullptr;
        TView v2 = xin; v2.act |= MFVI_ACT_SQUARE;
        float* dsig2 = c.farena() + plan->dsig2_off;
        if (!rc) { ProfScope ps(plan, i, PASS_BWD_WEIGHT, st);
          rc = launch_conv_bwd_weight(v2, g2, o.g, S.rho, none, 0, dsig2, dsig2, n_samples, st); }    // d sigma^2 (weights and bias variance)
        if (!rc && need_dx) { ProfScope ps(plan, i, PASS_BWD_DATA, st);
          rc = conv_backward_data(L, g2, o.g, plain_weights(c.farena() + plan->sig2_off), c.farena() + o.scratch2_off, per, n_samples); }
    }
    if (!rc && need_dx && plan->t[o.d.in0].consumers.front() == i) rc = fold_consumers(B, o.d.in0, i, L);
    return rc;
}

// The backward-weight kernel of op i, forked onto the side stream behind everything it reads (dy, BN-backward sums: final at this point of
// the caller's stream); a kernel that wrote partial slabs enters B.fin
int backward_weight(Backward& B, int i, const OpInfo& o, const TView& xin, const GView& gy)
{
    const PassSetup& S = B.S; mfvi_plan* plan = S.plan; hipStream_t st = S.st;
    const bool forks = B.will_fork(i);
    if (forks) {
        hipEvent_t ev = B.next_fork.ev;      // already on the previous launch's packet when that was sent
        hipError_t e = ev ? hipSuccess : plan->fork_events.next(&ev);
        if (e != hipSuccess) { set_error("backward: event creation failed: %s", hipGetErrorString(e)); return -1; }
        e = fork(st, B.side, ev, B.next_fork.sent);
        if (e != hipSuccess) { set_error("backward: fork failed: %s", hipGetErrorString(e)); return -1; }
    }
    B.next_fork.clear();
    Launch Lw{forks ? B.side : st};
    ProfScope ps(plan, i, PASS_BWD_WEIGHT, Lw.st);
    const bool last = forks && i == B.last_fork_op;
    if (last) B.join.arm(Lw, plan->join_event);
    int strips = 0;
    const int rc = conv_backward_weight(Lw, xin, gy, o.g, S.W, BwwPart{S.c.farena() + o.part_off, o.part_stride, o.max_strips}, &strips, B.dmu, B.drho, S.n_samples);
    o.family[2] = Lw.family;
    if (last) B.join.settle(Lw);
    if (rc == 0 && Lw.family != FAM_GENERIC) {      // the gradient went to partial slabs: grad_finalize reduces them
        GradFinEntry e{};
        e.w_off = o.g.w_off; e.b_off = o.g.b_off; e.part_off = o.part_off; e.stride = o.part_stride;
        e.n_w = (int)o.n_weights(); e.n_b = o.n_bias(); e.strips = strips; e.layer_id = o.g.layer_id;
        B.fin.push_back(e);
    }
    return rc;
}

// Backward-data with the fold in its epilogue (fused_fold).  *folded: done; else (declined) the un-fused route follows
int backward_data_fused_fold(Backward& B, int i, const OpInfo& o, Launch& L, const GView& gy, bool* folded)
{
    const PassSetup& S = B.S;
    const FoldFuse ff = S.c.fold_fuse(o, B.dz);
    ProfScope ps(S.plan, i, PASS_BWD_DATA, S.st);
    if (B.arm(L, i)) return -1;
    if (S.presample && o.x6bw_off >= 0) { L.x6_scratch = S.c.farena() + o.x6bw_off; L.x6_ready = S.x6_ready; }
    const int rc = conv_backward_data(L, gy, o.g, S.W, nullptr, 0, S.n_samples, &ff);
    B.settle(L);
    if (rc == 0) { *folded = true; o.family[1] = L.family; }
    return conv_declined(rc) ? 0 : rc;
}

// The tensor's other consumer has written its padded gradient and this one is a narrow 1x1 convolution (the 4-channel skip branch of a
// down-path tensor): no launch of its own — its backward-data is formed inside the fold (elementwise.hip, finalize_dx_vec1_kernel)
bool skip_in_fold(const Backward& B, const OpInfo& o)
{
    const PassSetup& S = B.S; const TensorInfo& x = S.plan->t[o.d.in0];
    return switches().fuse_skip_bwd && o.g.ks == 1 && o.g.stride == 1 && o.g.Cout <= 8 && x.consumers.size() == 2 &&
           S.plan->ops[x.consumers.back()].d.type == MFVI_OP_CONV && use_mfma() &&
           (S.presample ? o.in_slab : (!S.sample_weights && S.mu != nullptr));      // (its weights are in the slab, or w = mu)
}
int backward_data_in_fold(Backward& B, int i, const OpInfo& o, Launch& L, const GView& gy, bool* folded)
{
    ProfScope ps(B.S.plan, i, PASS_BWD_DATA, B.S.st);      // (booked on the op's backward-data slot: the fold now holds both)
    if (B.arm(L, i)) return -1;
    const int rc = fold_consumers(B, o.d.in0, i, L, i, &gy);
    B.settle(L);
    if (rc == 0) { *folded = true; o.family[1] = FAM_FOLD_SKIP; }
    return rc == CONV_NOT_SERVED ? 0 : rc;
}

// Backward-data into the padded-gradient scratch; the last consumer of the input tensor to run (the first in program order) folds
int backward_data_plain(Backward& B, int i, const OpInfo& o, Launch& L, const GView& gy, bool fold_here)
{
    const PassSetup& S = B.S;
    int rc;
    { ProfScope ps(S.plan, i, PASS_BWD_DATA, S.st);
      if (!fold_here && B.arm(L, i)) return -1;      // no fold behind it: this is the op's last launch on the caller's stream
      rc = conv_backward_data(L, gy, o.g, S.W, S.c.farena() + o.scratch_off, o.padded_per_sample(), S.n_samples);
      o.family[1] = L.family;
      if (!fold_here) B.settle(L); }
    if (rc || !fold_here) return rc;
    if (B.arm(L, i)) return -1;      // all consumers of in0 have run: fold + act' + BN sums
    rc = fold_consumers(B, o.d.in0, i, L);
    B.settle(L);
    return rc;
}

int backward_conv(Backward& B, int i, const OpInfo& o, Launch& L)
{
    const Ctx& c = B.S.c;
    const GView gy = c.gview(o.d.out, B.dout);
    int rc = backward_weight(B, i, o, c.view(o.d.in0), gy);
    if (rc || !c.need_dx(o, B.dz)) return rc;
    const bool fold_here = B.S.plan->t[o.d.in0].consumers.front() == i;
    bool folded = false;
    if (fused_fold(*B.S.plan, o, true)) rc = backward_data_fused_fold(B, i, o, L, gy, &folded);
    if (!rc && !folded && fold_here && skip_in_fold(B, o)) rc = backward_data_in_fold(B, i, o, L, gy, &folded);
    if (!rc && !folded) rc = backward_data_plain(B, i, o, L, gy, fold_here);
    return rc;
}

int backward_concat(Backward& B, int i, const OpInfo& o, Launch& L)
{
    const Ctx& c = B.S.c; const mfvi_plan& p = *B.S.plan;
    TView a; float* ga_a = nullptr; long long sa = 0;
    if (o.d.in0 >= 0) { a = c.view(o.d.in0); ga_a = c.grad_of(o.d.in0, nullptr); sa = p.t[o.d.in0].numel; }
    ProfScope ps(B.S.plan, i, PASS_CONCAT_BWD, B.S.st);
    if (B.arm(L, i)) return -1;
    const int rc = launch_concat_up_bwd(c.gview(o.d.out, B.dout), o.d.in0 >= 0 ? &a : nullptr, ga_a, sa, o.d.in0 >= 0 ? c.bsums_of(o.d.in0) : nullptr, c.view(o.d.in1),
                                        c.grad_of(o.d.in1, nullptr), p.t[o.d.in1].numel, c.bsums_of(o.d.in1), o.d.up_mode == MFVI_UP_NEAREST, B.S.n_samples, L);
    B.settle(L);
    return rc;
}

}  // namespace

extern "C" int mfvi_backward(mfvi_plan* plan, const void* mu_v, const void* rho_v, const float* bn, const float* z, uint64_t seed, uint32_t step,
                             uint32_t k0, int n_samples, int sample_weights, void* workspace, const float* dout, float* dmu, float* drho,
                             float* dbn, float* dz, void* stream)
{
    if (!check_call(plan, n_samples, workspace)) return -1;
    if (!mu_v || !rho_v || !z || !dout || !dmu || !drho || (plan->n_bn > 0 && (!bn || !dbn))) { set_error("backward: null pointer argument"); return -1; }
    if (plan->bn_eval) { set_error("backward: BatchNorm is in eval mode (mfvi_plan_set_bn_eval); the kernels implement the training-mode backward only"); return -1; }
    if (plan->fit_s && plan->fit_kstride != plan->fit_s) {      // (the gradient reduction re-derives eps of sample k0 + i)
        set_error("backward: fits mode with a sample stride of %lld (mfvi_plan_set_fits_sample_stride) serves forward passes only; the default is the %d samples per fit",
                  plan->fit_kstride, plan->fit_s);
        return MFVI_ERR_FITS_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    Backward B{PassSetup{plan, "backward", st, Ctx{*plan, (char*)workspace, bn, z, n_samples}, mu_v, rho_v, n_samples, sample_weights}, dout, dmu, drho, dbn, dz};
    int rc = pass_setup(B.S, true, seed, step, k0);
    if (!rc) rc = begin_backward(B, workspace, seed, step, k0);
    if (rc) return rc;
    for (int i = (int)plan->ops.size() - 1; i >= 0; --i) {
        const OpInfo& o = plan->ops[i];
        Launch L{st};      // this op's launches on the caller's stream
        rc = o.d.type == MFVI_OP_CONV_LRT ? backward_lrt(B, i, o, L) : o.d.type == MFVI_OP_CONV ? backward_conv(B, i, o, L) : backward_concat(B, i, o, L);
        if (rc > 0) set_error("backward: op %d launch failed: %s", i, hipGetErrorString((hipError_t)rc));
        if (!rc && i == plan->split_op && plan->split_active(st)) rc = reduce_early_group(B);
        if (rc) {
            if (B.side != st) (void)hipStreamSynchronize(B.side);   // leave no side-stream work behind a failed call
            return rc;
        }
    }
    if (B.side != st) {        // join: grad_finalize (and the caller) see every partial slab / accumulated gradient
        const hipError_t e = fork(B.side, st, plan->join_event, B.join.sent);
        if (e != hipSuccess) { set_error("backward: join failed: %s", hipGetErrorString(e)); return (int)e; }
    }
    // The rest (or all) of the layers: the late group of a split pass has its own table slot.  The BatchNorm parameter gradients ride on
    // this launch: every fold that feeds the BN-backward sums ran on `st` in front of it.  (Not with local-reparameterisation layers: their
    // d rho kernel in between touches neither, but keeps the old order for its tests)
    rc = finalize_grads(B, st, plan->split_active(st) ? mfvi_plan::FIN_LATE : mfvi_plan::FIN_WHOLE, plan->n_entries > 0 && plan->n_lrt == 0);
    if (rc) return rc;
    if (plan->n_lrt && sample_weights) {      // d rho += d sigma^2 * 2 softplus(rho) sigmoid(rho)
        rc = launch_lrt_drho(B.S.c.farena() + plan->dsig2_off, B.S.rho, plan->n_vi, drho, st);
        if (rc) { set_error("backward: lrt_drho launch failed: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    }
    if (plan->n_entries && !B.bn_done) {
        rc = launch_bn_param_grads(plan->table_dev, plan->n_entries, plan->max_c, B.S.c.bsums(), n_samples, dbn, st, plan->fit_s, plan->fit_gstride);
        if (rc) { set_error("backward: bn_param_grads launch failed: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    }
    return 0;
}
