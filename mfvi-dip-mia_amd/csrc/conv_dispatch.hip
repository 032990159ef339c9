// The one path from the plan to a convolution kernel (common.h: conv_forward, conv_backward_data, conv_backward_weight): picks the kernel family
// of a (layer, pass) from the layer's tiling word and the shape, for mfvi_forward / mfvi_backward and for mfvi_plan_autotune's candidates alike.
#include "common.h"
#include "../../include/mfvi_hip.h"
#include <cstdlib>

bool use_mfma()
{
    static const bool on = [] { const char* e = getenv("MFVI_DISABLE_MFMA"); return !(e && e[0] == '1'); }();
    return on;
}

namespace {

// an explicit tiling of the plan / autotuner answers for itself: "shape not served" by the family it names is "tiling not valid"
inline int own_answer(int rc) { return rc == CONV_NOT_SERVED ? CONV_BAD_TILING : rc; }

// the layer's fp32 default where the plan holds no tiling (or the tiling's family cannot run in this call): row-phase where it serves the shape
inline int default_tune(const ConvGeom& g, int mode, int n_samples) { return env_tune() ? 0 : rp_default_tune(g, mode, n_samples); }

int forward_mfma(Launch& L, const TView& in, const ConvGeom& g, const float* w, long long wstride, OutDesc out, int n_samples)
{
    if (g.Cin > MFVI_MAX_C || (g.Cin & 3) || (g.w_off & 3)) return CONV_NOT_SERVED;      // Philox blocks must tile every weight row
    if (g.tune[0] & MFVI_TUNE_GENERIC) return CONV_NOT_SERVED;                           // in-kernel eps: the generic kernel draws and convolves in one launch
    if ((long long)g.Cout * g.Ho * g.Wo >= (1LL << 31)) return CONV_NOT_SERVED;          // the epilogue uses 32-bit element offsets per sample
    // aligned float4 staging: image rows, sample strides and the base pointer must be multiples of 4 floats
    if ((g.W & 3) || g.W < 4 || (in.sstride & 3) || ((uintptr_t)in.data & 15)) return CONV_NOT_SERVED;
    // streaming 1x1, one-stage and bf16x6 kernels: only as an explicit tiling of the plan / autotuner
    int tn = g.tune[0] ? g.tune[0] : default_tune(g, 0, n_samples);
    if (tn & MFVI_TUNE_ST) return own_answer(launch_conv1_fwd_stream(in, g, w, wstride, out, n_samples, L));
    if (tn & MFVI_TUNE_SM) return own_answer(g.ks == 1 ? launch_conv1_fwd_small(in, g, w, wstride, out, n_samples, L) : launch_conv_fwd_small(in, g, w, wstride, out, n_samples, L));
    if (tn & MFVI_TUNE_X6) {
        const int rc = launch_conv_fwd_x6(in, g, w, wstride, out, tn & (MFVI_TUNE_X6 - 1), n_samples, L);
        if (rc != CONV_NOT_SERVED) return rc;
        // no scratch for the weight pieces in this call (w = mu of the eval branch, sample_weights = 0: the plan hands the scratch over
        // only behind a weight draw): the layer's fp32 default, not the generic kernels
        tn = default_tune(g, 0, n_samples);
    }
    if (tn & MFVI_TUNE_RP) {
        const int rc = launch_conv_fwd_rp(in, g, w, wstride, out, tn & (MFVI_TUNE_RP - 1), n_samples, L);
        if (g.tune[0] & MFVI_TUNE_RP) return own_answer(rc);
        if (!conv_declined(rc)) return rc;      // (a heuristic tiling the shape does not admit: the round-2 tiles below)
    }
    return launch_conv_fwd_mfma(in, g, w, wstride, out, n_samples, L);
}

int backward_data_mfma(Launch& L, const GView& gy, const ConvGeom& g, const float* w, long long wstride, float* dxp, long long dxp_sstride, int n_samples,
                       const FoldFuse* fuse)
{
    if (g.Cout > MFVI_MAX_C || (g.stride != 1 && !(g.stride == 2 && g.ks >= 3)) || (g.Cin & 3) || (g.w_off & 3)) return CONV_NOT_SERVED;
    if (g.tune[1] & MFVI_TUNE_GENERIC) return CONV_NOT_SERVED;
    if ((long long)g.Cin * (g.H + 4) * (g.W + 4) >= (1LL << 31)) return CONV_NOT_SERVED;   // 32-bit element offsets per sample
    // aligned float4 (stride 2: float2) staging of the gradient and of the conv output it is normalised with
    const int wa = g.stride == 2 ? 1 : 3;
    if ((g.Wo & wa) || g.Wo < (wa + 1) || (gy.gstride & wa) || ((uintptr_t)gy.ga & 15) || (gy.y && ((gy.ystride & wa) || ((uintptr_t)gy.y & 15)))) return CONV_NOT_SERVED;
    if (!fuse) return launch_conv_bwd_data_mfma(gy, g, w, wstride, dxp, dxp_sstride, n_samples, L);
    // the fold runs in the epilogue: aligned float4 rows of the input tensor and of its gradient
    if (!(g.ks == 1 || (g.ks == 3 && g.stride == 1)) || !fuse->ga || (g.W & 3) || (fuse->ga_sstride & 3) || ((uintptr_t)fuse->ga & 15)) return CONV_NOT_SERVED;
    if (fuse->bsums && ((fuse->x.sstride & 3) || ((uintptr_t)fuse->x.data & 15))) return CONV_NOT_SERVED;
    if (g.ks == 3 && (g.H < 4 || g.W < 4)) return CONV_NOT_SERVED;      // rows 1 and H-2 (columns 1 and W-2) must be distinct, interior lines
    if (g.ks == 1) {      // one-stage 1x1 kernel: only as an explicit tiling of the plan / autotuner
        if (g.tune[1] & MFVI_TUNE_SM) return own_answer(launch_conv1_bwd_data_small(gy, g, w, wstride, n_samples, L, *fuse));
        return launch_conv_bwd_data_mfma(gy, g, w, wstride, nullptr, 0, n_samples, L, fuse);
    }
    int tn = g.tune[1] ? g.tune[1] : default_tune(g, 1, n_samples);
    bool own = g.tune[1] != 0;      // a row-phase tiling of the plan answers for itself
    if (tn & MFVI_TUNE_X6) {        // bf16x6 and one-stage kernels: only as an explicit tiling of the plan / autotuner
        const int rc = launch_conv_bwd_data_x6(gy, g, w, wstride, tn & (MFVI_TUNE_X6 - 1), n_samples, L, *fuse);
        if (rc != CONV_NOT_SERVED) return rc;
        // no scratch for the weight pieces in this call (w = mu without a weight draw): the layer's fp32 default
        tn = default_tune(g, 1, n_samples); own = false;
    } else if (tn & MFVI_TUNE_SM) return own_answer(launch_conv_bwd_data_small(gy, g, w, wstride, n_samples, L, *fuse));
    if (tn & MFVI_TUNE_RP) {
        const int rc = launch_conv_bwd_data_rp(gy, g, w, wstride, tn & (MFVI_TUNE_RP - 1), n_samples, L, *fuse);
        if (own) return own_answer(rc);
        if (!conv_declined(rc)) return rc;      // (heuristic tiling not valid for this shape: the round-2 tiles below)
    }
    return launch_conv_bwd_data_mfma(gy, g, w, wstride, nullptr, 0, n_samples, L, fuse);
}

int backward_weight_mfma(Launch& L, const TView& in, const GView& gy, const ConvGeom& g, BwwPart part, int* strips_used, int n_samples)
{
    if (!part.base || part.max_strips < 1 || (g.Cin & 3) || (g.w_off & 3)) return CONV_NOT_SERVED;
    if (g.tune[2] & MFVI_TUNE_GENERIC) return CONV_NOT_SERVED;                           // in-kernel eps: the generic kernel accumulates d mu / d rho itself
    const int cfg = g.tune[2] ? g.tune[2] : env_tune_w();
    if (!cfg) {
        // heuristic: the bf16x6 kernel where it serves the shape and measured ahead of the fp32 ones (3x3 stride 1, >= 32 input channels, maps a
        // multiple of 32 wide: profiles/r03_x6_layers.txt)
        static const bool x6_on = [] { const char* e = getenv("MFVI_X6"); return !(e && e[0] == '0'); }();
        if (x6_on && g.ks == 3 && g.stride == 1 && !(g.W & 31) && !(g.H & 1) && g.H >= 4 && g.Cin >= 32 && ((g.Cin & 15) == 0 || (g.Cin & 15) == 4)) {
            const int rc = launch_conv_bwd_weight_x6(in, gy, g, part, strips_used, g.Cout >= 32 ? 2 : 1, 256, n_samples, L);
            if (!conv_declined(rc)) return rc;
        }
    }
    if (((cfg >> 8) & 255) == 11)      // bf16x6 kernel as an explicit tiling: output fragments per block | 11 << 8 | (target blocks / 256) << 16
        return launch_conv_bwd_weight_x6(in, gy, g, part, strips_used, cfg & 255, ((cfg >> 16) & 255) * 256, n_samples, L);
    return launch_conv_bwd_weight_mfma(in, gy, g, part, strips_used, cfg, n_samples, L);
}

// the matrix-core path declined: true = run the generic fp32 kernel (which bf16 parameters do not reach: *rc = -1)
bool to_generic(Launch& L, const ConvGeom& g, const ConvWeights& W, const char* pass, bool generic_fallback, int* rc)
{
    if (!conv_declined(*rc) || !generic_fallback) return false;
    if (W.mu) { L.family = FAM_GENERIC; return true; }      // (fits mode too: the kernels find a sample's fit through W.fit)
    set_error("%s: conv layer %d needs the generic fp32 kernels, which bf16 parameters reach only for layers outside the sampling table (use H, W multiples of 4)", pass, g.layer_id);
    *rc = -1; return false;
}

}  // namespace

int conv_forward(Launch& L, const TView& in, const ConvGeom& g, const ConvWeights& W, OutDesc out, int n_samples, bool generic_fallback)
{
    int rc = use_mfma() ? forward_mfma(L, in, g, W.w, W.wstride, out, n_samples) : CONV_NOT_SERVED;
    if (to_generic(L, g, W, "forward", generic_fallback, &rc)) rc = launch_conv_fwd(in, g, W.mu, W.rho, W.key, W.sample_weights, out, n_samples, L.st, W.fit);
    return rc;
}

int conv_backward_data(Launch& L, const GView& gy, const ConvGeom& g, const ConvWeights& W, float* dxp, long long dxp_sstride, int n_samples,
                       const FoldFuse* fuse, bool generic_fallback)
{
    int rc = use_mfma() ? backward_data_mfma(L, gy, g, W.w, W.wstride, dxp, dxp_sstride, n_samples, fuse) : CONV_NOT_SERVED;
    if (to_generic(L, g, W, "backward-data", generic_fallback && !fuse, &rc))
        rc = launch_conv_bwd_data(gy, g, W.mu, W.rho, W.key, W.sample_weights, dxp, dxp_sstride, n_samples, L.st, W.fit);
    return rc;
}

int conv_backward_weight(Launch& L, const TView& in, const GView& gy, const ConvGeom& g, const ConvWeights& W, BwwPart part, int* strips_used,
                         float* dmu, float* drho, int n_samples, bool generic_fallback)
{
    int rc = use_mfma() ? backward_weight_mfma(L, in, gy, g, part, strips_used, n_samples) : CONV_NOT_SERVED;
    if (to_generic(L, g, W, "backward-weight", generic_fallback, &rc)) rc = launch_conv_bwd_weight(in, gy, g, W.rho, W.key, W.sample_weights, dmu, drho, n_samples, L.st, W.fit);
    return rc;
}
