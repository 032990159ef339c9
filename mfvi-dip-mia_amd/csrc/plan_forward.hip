// mfvi_forward: the forward pass of a plan (include/mfvi_hip.h) — the draws in front of it, then the ops in program order, the skip-branch
// convolutions of the small maps forked onto the plan's side stream.
#include "plan_internal.h"

namespace {

struct Forward {
    PassSetup S; float* out;
    // A skip-branch convolution (its only consumer is a later concat) on a map of up to MFVI_FWD_FORK pixels runs on the side stream
    // (PlanSwitches::fwd_fork) and is joined in front of that concat
    bool forks(size_t j) const
    {
        const mfvi_plan& p = *S.plan;
        if (j >= p.ops.size()) return false;
        const OpInfo& oj = p.ops[j]; const TensorInfo& yj = p.t[oj.d.out];
        return switches().fwd_fork > 0 && p.side && p.side_enabled && oj.d.type == MFVI_OP_CONV && use_mfma() && (long long)oj.g.Ho * oj.g.Wo <= switches().fwd_fork &&
               yj.consumers.size() == 1 && yj.consumers.front() > (int)j + 1 && p.ops[yj.consumers.front()].d.type == MFVI_OP_CONCAT_UP;
    }
};

// Everything in front of the first op: cleared statistics, eval-mode BatchNorm, the draws of this pass (weights, Dropout2d factors), the
// bf16x6 weight pieces
int begin_forward(Forward& F, void* workspace, uint64_t seed, uint32_t step, uint32_t k0)
{
    PassSetup& S = F.S; mfvi_plan* plan = S.plan; const Ctx& c = S.c; hipStream_t st = S.st;
    // The forward statistics and (adjacent) the BN-backward sums of the backward pass that follows start every pass from zero.  With a weight
    // draw in front of the pass the draw's kernel clears them with its own threads (round 4: the memset was a dependent 6 us launch at the
    // head of every iteration); eval-mode BatchNorm fills the statistics in front of the draw and keeps the memset.
    const bool zero_in_draw = plan->stats_doubles && S.presample && !(plan->bn_eval && plan->n_entries);
    if (plan->stats_doubles) {
        if (!zero_in_draw) {
            hipError_t e = hipMemsetAsync(c.fstats(), 0, sizeof(double) * 2 * plan->stats_doubles, st);
            if (e != hipSuccess) { set_error("forward: memset failed: %s", hipGetErrorString(e)); return (int)e; }
        }
        plan->bsums_clean_ws = workspace;
    }
    if (plan->bn_eval && plan->n_entries) {   // nn.BatchNorm2d in eval mode: the running statistics stand in for every sample's batch sums
        const int rc = launch_bn_eval_fill(plan->table_dev, plan->n_entries, plan->max_c, c.fstats(), S.n_samples, plan->bn_eval, st);
        if (rc) { set_error("forward: bn_eval_fill launch failed: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    }
    if (plan->n_lrt && S.sample_weights) {      // weights of the variance convolutions of this pass
        if (!S.rho) { set_error("forward: local-reparameterisation layers take float32 parameters"); return -1; }
        const int rc = launch_lrt_sigma2(S.rho, plan->n_vi, c.farena() + plan->sig2_off, st);
        if (rc) { set_error("forward: sigma^2 launch failed: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    }
    if (S.presample) {
        ProfScope ps(plan, -1, PASS_SAMPLE, st);
        const int rc = launch_sample_weights(plan->samp_dev, plan->n_samp, plan->samp_blocks, S.mu_v, S.rho_v, S.key, S.slab_rows() ? S.n_samples : 1, c.wsamp(),
                                             plan->n_vi, st, S.bf16, S.sample_weights, zero_in_draw ? c.fstats() : nullptr, zero_in_draw ? 2 * plan->stats_doubles : 0,
                                             plan->fit_s, plan->fit_pstride, plan->fit_kdelta());
        if (rc) { set_error("forward: sample_weights launch failed: %s", hipGetErrorString((hipError_t)rc)); return rc; }
        plan->samp_mu = S.mu_v; plan->samp_rho = S.rho_v; plan->samp_ws = workspace; plan->samp_seed = seed; plan->samp_step = step; plan->samp_k0 = k0;
        plan->samp_n = S.sample_weights ? S.n_samples : -S.n_samples;
    }
    if (plan->n_drop && plan->dropout_on) {      // Dropout2d factors of this pass; the backward reads them from the workspace
        const int rc = launch_dropout_masks(plan->drop_dev, plan->n_drop, S.key, S.n_samples, c.farena(), st, plan->fit_s && !plan->fit_drop.empty() ? plan->fit_drop_dev : nullptr, plan->fit_s,
                                            plan->fit_kdelta());
        if (rc) { set_error("forward: dropout mask launch failed: %s", hipGetErrorString((hipError_t)rc)); return rc; }
    }
    return split_weight_pieces(S, 0, nullptr);
}

// LRTLayer.forward (reparam_layers.py:59-72): act_mu = conv(v, mu, mu_b); training: + sqrt(1e-16 + conv(v^2, sigma^2, sigma_b^2)) * eps
int forward_lrt(const Forward& F, const OpInfo& o, Launch& L)
{
    const PassSetup& S = F.S; const Ctx& c = S.c; const mfvi_plan& p = *S.plan;
    const TensorInfo& y = p.t[o.d.out];
    const OutDesc od = c.out_desc(o, F.out, !p.bn_eval);
    if (!S.mu) { set_error("forward: local-reparameterisation layers take float32 parameters"); return -1; }
    if (!S.sample_weights) return conv_forward(L, c.view(o.d.in0), o.g, plain_weights(S.mu), od, S.n_samples);
    OutDesc oa; oa.data = c.farena() + p.lrt_tmp_off; oa.sstride = y.numel; oa.stats = nullptr;
    OutDesc os; os.data = c.farena() + o.s2_off; os.sstride = y.numel; os.stats = nullptr;
    TView v2 = c.view(o.d.in0); v2.act |= MFVI_ACT_SQUARE;
    int rc = conv_forward(L, c.view(o.d.in0), o.g, plain_weights(S.mu), oa, S.n_samples);
    if (!rc) rc = conv_forward(L, v2, o.g, plain_weights(c.farena() + p.sig2_off), os, S.n_samples);
    if (!rc) rc = launch_lrt_combine(oa.data, os.data, y.numel, y.d.C, (long long)y.d.H * y.d.W, S.key, o.g.layer_id, od, S.n_samples, L.st);
    return rc;
}

int forward_conv(const Forward& F, const OpInfo& o, Launch& L)
{
    const PassSetup& S = F.S;
    if (S.presample && o.x6w_off >= 0) { L.x6_scratch = S.c.farena() + o.x6w_off; L.x6_ready = S.x6_ready; }
    const int rc = conv_forward(L, S.c.view(o.d.in0), o.g, S.W, S.c.out_desc(o, F.out, !S.plan->bn_eval), S.n_samples);
    o.family[0] = L.family;
    return rc;
}

int forward_concat(const Forward& F, const OpInfo& o, Launch& L)
{
    const PassSetup& S = F.S;
    TView a; if (o.d.in0 >= 0) a = S.c.view(o.d.in0);
    return launch_concat_up_fwd(o.d.in0 >= 0 ? &a : nullptr, S.c.view(o.d.in1), S.c.out_desc(o, F.out, !S.plan->bn_eval), o.d.up_mode == MFVI_UP_NEAREST, S.n_samples, L.st);
}

}  // namespace

extern "C" int mfvi_forward(mfvi_plan* plan, const void* mu_v, const void* rho_v, const float* bn, const float* z, uint64_t seed, uint32_t step,
                            uint32_t k0, int n_samples, int sample_weights, void* workspace, float* out, void* stream)
{
    if (!check_call(plan, n_samples, workspace)) return -1;
    if (!mu_v || !rho_v || !z || !out || (plan->n_bn > 0 && !bn)) { set_error("forward: null pointer argument"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    Forward F{PassSetup{plan, "forward", st, Ctx{*plan, (char*)workspace, bn, z, n_samples}, mu_v, rho_v, n_samples, sample_weights}, out};
    int rc = pass_setup(F.S, true, seed, step, k0);
    if (!rc) rc = begin_forward(F, workspace, seed, step, k0);
    if (rc) return rc;
    // Events on the kernels' own packets where the launch goes through mfvi_launch (as in mfvi_backward): the fork event of op i + 1 on op i's
    // last launch, the join event on the forked launch itself.
    const bool on_packet = switches().fork_on_packet && !plan->capture_mode && plan->prof_mode != 1;
    PacketEvent next_fork{on_packet}, join{on_packet};
    EventPool& pool = plan->fwd_events; pool.reset();
    std::vector<hipEvent_t> join_at(plan->ops.size(), nullptr);      // per op: the completion event of a forked producer of its input
    const char* what = "fork";
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < plan->ops.size(); ++i) {
        const OpInfo& o = plan->ops[i];
        if (join_at[i]) { what = "join"; e = hipStreamWaitEvent(st, join_at[i], 0); if (e != hipSuccess) break; what = "fork"; }
        const bool forked = F.forks(i);
        hipEvent_t ev = next_fork.ev;      // reserved on the previous launch (sent there, or recorded here if that launch took another path)
        if (forked) { if (!ev) e = pool.next(&ev); if (e == hipSuccess) e = fork(st, plan->side, ev, next_fork.sent); if (e != hipSuccess) break; }
        next_fork.clear();
        Launch L{forked ? plan->side : st};      // this op's launches: its stream, the event riding on them, its bf16x6 weight pieces
        if (forked) { e = pool.next(&ev); if (e != hipSuccess) break; join.arm(L, ev); }      // its completion event rides on its own launch
        else if (on_packet && o.d.type != MFVI_OP_CONV_LRT && F.forks(i + 1)) { e = pool.next(&ev); if (e != hipSuccess) break; next_fork.arm(L, ev); }
        {
            ProfScope ps(plan, (int)i, PASS_FWD, L.st);
            rc = o.d.type == MFVI_OP_CONV_LRT ? forward_lrt(F, o, L) : o.d.type == MFVI_OP_CONV ? forward_conv(F, o, L) : forward_concat(F, o, L);
        }
        if (rc) { if (rc > 0) set_error("forward: op %d launch failed: %s", (int)i, hipGetErrorString((hipError_t)rc)); break; }
        if (forked) {      // its completion event, waited for in front of the consumer
            join.settle(L);
            e = record_unless_sent(join.ev, L.st, join.sent); if (e != hipSuccess) break;
            join_at[plan->t[o.d.out].consumers.front()] = join.ev;
        } else next_fork.settle(L);
    }
    if (e != hipSuccess) { set_error("forward: %s failed: %s", what, hipGetErrorString(e)); rc = (int)e; }
    // forked skip-branch work may still be writing activations / BN statistics: join it before handing the buffers back
    if (rc && plan->side) (void)hipStreamSynchronize(plan->side);
    return rc;
}
