// mfvi_plan_autotune: times the valid tilings of every convolution of a plan on this device and keeps the fastest (include/mfvi_hip.h).
#include "plan_internal.h"

namespace {

// Candidate tilings of op `o` for pass `which`, in the order they are timed (ties go to the first):
//   fwd / bwd-data (mf, th, T) = fragments x tile rows x tiles per block;
//   bwd-weight (nb, waves, target/256) = input tiles per block x waves x block-count target
// in_kernel_eps: the layer is small enough for the generic kernels that draw eps themselves (MFVI_TUNE_GENERIC)
std::vector<int> tune_candidates(const OpInfo& o, int which, int n_samples, bool in_kernel_eps)
{
    std::vector<int> cands;
    if (which < 2) {
        for (int th : {8, 16, 8 | 128, 16 | 128, 4 | 128, 2 | 128}) for (int mf = 1; mf <= 4; ++mf) for (int T = 1; T <= 8; T *= 2) cands.push_back(mf | th << 8 | T << 16);
        // backward-data of the 4 + 16n-channel concat layers: the last 4 output channels on the 4x4x1 matrix instruction (th bit 64)
        if (which == 1 && (o.g.Cin & 15) == 4) for (int mf : {1, 2, 4}) for (int T = 1; T <= 8; T *= 2) cands.push_back(mf | (8 | 64) << 8 | T << 16);
        // row-phase kernels (conv_rp.hip) for 3x3 stride-1 layers on maps whose width is a multiple of 64:
        // (mf, rows per wave, 4 extra channels on the 4x4x1 instruction, tiles per block); -3 = not valid for the shape
        if (o.g.ks == 3 && o.g.stride == 1 && ((o.g.W & 63) == 0 || o.g.W == 32 || o.g.W == 16) && rp_default_tune(o.g, which, n_samples))
            for (int mf : {1, 2, 4}) for (int r : {1, 2, 4}) for (int rem = 0; rem <= ((which == 1 && (o.g.Cin & 15) == 4) ? 1 : 0); ++rem)
                for (int T = 1; T <= 8; T *= 2) cands.push_back(mf | r << 8 | rem << 12 | T << 16 | MFVI_TUNE_RP);
        if (o.g.ks == 3 && o.g.stride == 1 && o.g.W == 16 && rp_default_tune(o.g, which, n_samples))      // 16-wide maps: 2 / 4 k-steps per stage
            for (int mf : {1, 2}) for (int ks : {2, 4}) for (int rem = 0; rem <= ((which == 1 && (o.g.Cin & 15) == 4) ? 1 : 0); ++rem)
                cands.push_back(mf | 1 << 8 | rem << 12 | ks << 13 | 1 << 16 | MFVI_TUNE_RP);
        // small-map forward (conv_small.hip): one stage, the block's whole reduction in LDS
        if (which <= 1 && o.g.ks == 3 && o.g.stride == 1 && o.g.W <= 16) cands.push_back(1 | MFVI_TUNE_SM);
        // streaming forward of the narrow 1x1 layers (conv_1x1.hip, conv1_stream_kernel): at most 32 output channels
        if (which == 0 && o.g.ks == 1 && o.g.stride == 1 && o.g.Cout <= 32 && (o.g.Cin & 3) == 0 && o.g.Cin <= 64 && (((long long)o.g.H * o.g.W) & 63) == 0)
            cands.push_back(1 | MFVI_TUNE_ST);
        // one-stage 1x1 kernel (conv_1x1.hip): the `up` 1x1 layers of 32 ... 128 channels; same tune bit
        if (which <= 1 && o.g.ks == 1 && o.g.stride == 1 && (o.g.Cin & 15) == 0 && (o.g.Cout & 15) == 0 && o.g.Cin <= 128 && o.g.Cout <= 128
            && (((long long)o.g.H * o.g.W) & 63) == 0) cands.push_back(1 | MFVI_TUNE_SM);
        // bf16x6 forward (conv_x6.hip): output fragments per block, 8 output rows per block
        if (which == 0 && o.x6w_off >= 0) for (int mf : {1, 2}) for (int T = 1; T <= 16; T *= 2) cands.push_back(mf | 8 << 8 | T << 16 | MFVI_TUNE_X6);
        if (which == 0 && o.x6w_off >= 0 && (o.g.Cin & 31) == 4) for (int T = 1; T <= 16; T *= 2) cands.push_back(1 | 8 << 8 | 1 << 12 | T << 16 | MFVI_TUNE_X6);      // remainder plane on the last group's pass
        // bf16x6 backward-data with the fold (conv_bwd_x6.hip): strips per block; rows per strip follow the output-channel count
        if (which == 1 && o.x6bw_off >= 0) for (int T : {1, 2, 4, 8, 16, 32}) cands.push_back(T | (o.g.Cout == 16 ? 8 : o.g.Cout == 32 ? 4 : 2) << 8 | MFVI_TUNE_X6);
        if (which == 1 && o.x6bw_off >= 0 && x6s_shape_ok(o.g)) for (int T : {2, 4, 8, 16, 32}) cands.push_back(T | 8 << 8 | 1 << 16 | MFVI_TUNE_X6);      // strip-resident form (conv_bwd_x6s.hip)
    }
    else {
        for (int nb = 1; nb <= 3; ++nb) for (int nw : {4, 8, 9}) for (int tb = 1; tb <= 8; tb *= 2) cands.push_back(nb | nw << 8 | tb << 16);
        for (int tb = 1; tb <= 8; tb *= 2) cands.push_back(2 | 10 << 8 | tb << 16);      // fragment-split variant (3x3 stride 1, full-width tiles)
        if (o.g.ks == 3 && o.g.stride == 1 && (o.g.W & 31) == 0)                         // bf16x6 kernel (conv_bww_x6.hip)
            for (int cof = 1; cof <= 2; ++cof) for (int tb = 1; tb <= 4; tb *= 2) cands.push_back(cof | 11 << 8 | tb << 16);
    }
    if (in_kernel_eps && which != 1) cands.push_back(MFVI_TUNE_GENERIC);      // (backward-data: the fused fold of the matrix-core path is not what the generic kernel replaces)
    return cands;
}

struct TuneBuffers { float* out; float* dout; float* dmu; float* drho; };

// What mfvi_forward / mfvi_backward launch for the tiling in o.g.tune[which], through the same dispatch, except: the layer splits its own bf16x6
// weight pieces (x6_ready stays false: timed with the layer), and only an in-kernel-eps candidate reaches the generic kernels
int launch_tuned(const PassSetup& S, const OpInfo& o, int which, const TuneBuffers& b, int* strips_used)
{
    const Ctx& c = S.c;
    Launch L{S.st};
    const bool generic = (o.g.tune[which] & MFVI_TUNE_GENERIC) != 0;
    const TView xin = c.view(o.d.in0);
    if (which == 0) {
        if (o.x6w_off >= 0) L.x6_scratch = c.farena() + o.x6w_off;
        return conv_forward(L, xin, o.g, S.W, c.out_desc(o, b.out), S.n_samples, generic);
    }
    const GView gy = c.gview(o.d.out, b.dout);
    if (which == 2)
        return conv_backward_weight(L, xin, gy, o.g, S.W, BwwPart{c.farena() + o.part_off, o.part_stride, o.max_strips}, strips_used, b.dmu, b.drho, S.n_samples, generic);
    if (fused_fold(*S.plan, o, c.need_dx(o, nullptr))) {      // (it accumulates into the BN-backward sums: contents undefined afterwards)
        const FoldFuse ff = c.fold_fuse(o, nullptr);
        if (o.x6bw_off >= 0) L.x6_scratch = c.farena() + o.x6bw_off;
        const int r2 = conv_backward_data(L, gy, o.g, S.W, nullptr, 0, S.n_samples, &ff);
        if (r2 != CONV_NOT_SERVED) return r2;
    }
    return conv_backward_data(L, gy, o.g, S.W, c.farena() + o.scratch_off, o.padded_per_sample(), S.n_samples, nullptr, generic);
}

}  // namespace

extern "C" int mfvi_plan_autotune(mfvi_plan* plan, const void* mu, const void* rho, const float* bn, const float* z, int n_samples,
                                  void* workspace, float* out_scratch, float* grad_scratch, void* stream)
{
    if (!check_call(plan, n_samples, workspace)) return -1;
    if (!mu || !rho || !z || !out_scratch || !grad_scratch || (plan->n_bn > 0 && !bn)) { set_error("autotune: null pointer argument"); return -1; }
    if (plan->fit_s) { set_error("autotune: run it before mfvi_plan_set_fits switches fits mode on (the tilings do not depend on the mode)"); return MFVI_ERR_FITS_UNSUPPORTED; }
    { const char* e = getenv("MFVI_AUTOTUNE"); if ((e && e[0] == '0') || !use_mfma()) return 0; }
    hipStream_t st = (hipStream_t)stream;
    const long long n_out = plan->t[plan->output].numel * n_samples;
    const TuneBuffers b{out_scratch, out_scratch + n_out, grad_scratch, grad_scratch + plan->n_vi};
    float* dbn = b.drho + plan->n_vi;
    // every tensor, statistic and gradient the kernels read holds finite data: one real forward + backward
    int rc = mfvi_forward(plan, mu, rho, bn, z, 1, 0, 0, n_samples, 1, workspace, b.out, stream);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(b.dout, b.out, sizeof(float) * n_out, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(grad_scratch, 0, sizeof(float) * (2 * plan->n_vi + plan->n_bn), st);
    if (e != hipSuccess) { set_error("autotune: %s", hipGetErrorString(e)); return (int)e; }
    rc = mfvi_backward(plan, mu, rho, bn, z, 1, 0, 0, n_samples, 1, workspace, b.dout, b.dmu, b.drho, dbn, nullptr, stream);
    if (rc) return rc;
    // a cold GPU ramps its clocks over the first ~100 ms of work: candidates timed during the ramp would look slow and the
    // choice would depend on their order, so run the real passes until the device has been busy for a while
    for (int warm = 0; warm < 24 && !rc; ++warm) {
        rc = mfvi_forward(plan, mu, rho, bn, z, 1, 0, 0, n_samples, 1, workspace, b.out, stream);
        if (!rc) rc = mfvi_backward(plan, mu, rho, bn, z, 1, 0, 0, n_samples, 1, workspace, b.dout, b.dmu, b.drho, dbn, nullptr, stream);
    }
    if (rc) return rc;
    // the pass those launches belong to: the slab holds its draw; bf16 parameters are not expanded (the in-kernel-eps candidates, which
    // alone would read the float32 view, are offered to float32 plans only)
    PassSetup S{plan, "autotune", st, Ctx{*plan, (char*)workspace, bn, z, n_samples}, mu, rho, n_samples, 1};
    rc = pass_setup(S, false, 1, 0, 0);
    if (rc) return rc;
    S.W = ConvWeights{S.c.wsamp(), plan->n_vi, S.mu, S.rho, base_key(1, 0, 0), 1};
    hipEvent_t ea, eb;
    if (hipEventCreate(&ea) != hipSuccess || hipEventCreate(&eb) != hipSuccess) { set_error("autotune: hipEventCreate failed"); return -1; }
    const int reps = 6;
    for (size_t i = 0; i < plan->ops.size(); ++i) {
        OpInfo& o = plan->ops[i];
        if (o.d.type != MFVI_OP_CONV) continue;
        for (int which = 0; which < 3; ++which) {
            if (which == 1 && o.d.in0 == plan->input) continue;
            int strips_used = 0;
            int best = 0; float best_ms = 1e30f;
            for (int cand : tune_candidates(o, which, n_samples, S.mu && o.n_weights() <= MFVI_INKERNEL_MAX_W)) {
                o.g.tune[which] = cand;
                rc = launch_tuned(S, o, which, b, &strips_used);      // warm-up
                if (rc == CONV_NOT_SERVED) break;                // no candidate will serve this op and pass
                if (rc == CONV_BAD_TILING) continue;
                if (rc) { set_error("autotune: op %d launch failed: %s", (int)i, rc > 0 ? hipGetErrorString((hipError_t)rc) : "bad arguments"); goto done; }
                float ms = 1e30f;
                for (int trial = 0; trial < 3 && !rc; ++trial) {      // best of three timings of `reps` launches: the choice must not flip on noise
                    (void)hipEventRecord(ea, st);
                    for (int r = 0; r < reps && !rc; ++r) rc = launch_tuned(S, o, which, b, &strips_used);
                    (void)hipEventRecord(eb, st);
                    float t_ms = 0.f;
                    e = hipEventSynchronize(eb);
                    if (e == hipSuccess) e = hipEventElapsedTime(&t_ms, ea, eb);
                    if (e != hipSuccess) break;
                    if (t_ms < ms) ms = t_ms;
                }
                if (rc || e != hipSuccess) { set_error("autotune: op %d timing failed: %s", (int)i, hipGetErrorString(rc ? (hipError_t)rc : e)); rc = rc ? rc : (int)e; goto done; }
                // backward-weight: every extra pixel strip is one more slab grad_finalize has to read (~2 TB/s there)
                if (which == 2) ms += reps * (float)((double)strips_used * n_samples * o.part_stride * 4.0 / 2.0e12 * 1e3);
                if (ms < best_ms) { best_ms = ms; best = cand; }
            }
            o.g.tune[which] = best;
            rc = 0;
        }
    }
done:
    plan->bsums_clean_ws = nullptr;      // the timed launches accumulated into the BN-backward sums
    (void)hipEventDestroy(ea); (void)hipEventDestroy(eb);
    if (rc) for (auto& o : plan->ops) { o.g.tune[0] = 0; o.g.tune[1] = 0; o.g.tune[2] = 0; }
    return rc;
}
