// The element-wise passes of one ELBO iteration for MANY independent fits in one launch each (mfvi_plan_set_fits is
// the plan side): input perturbation, Gaussian NLL, KL + AdamW, smoothed outputs, and for inpainting (section 17) the masked 4-channel NLL,
// the smoothed sigmoid colours and the masked squared error of the metric.  Grid y = fit (or sample); the per-thread bodies are the
// single-fit kernels' own (iter_ops.h), so a fit of a batch computes what mfvi_perturb_input / mfvi_gaussian_nll / mfvi_elbo_update /
// mfvi_bookkeep / mfvi_gaussian_nll_inpainting / mfvi_bookkeep_inpainting compute for it alone.  The reference runs one process per fit instead (bayesian_optimization.py:3760-3775).
#include "common.h"
#include "iter_ops.h"
#include "../../include/mfvi_hip.h"

namespace {

__global__ __launch_bounds__(256) void perturb_fits_kernel(RngKey key, long long n, float std, const float* __restrict__ z0, float* __restrict__ z)
{
    key.sample += blockIdx.y;      // fit f: sample fit0 + f of RNG domain INPUT
    normal_fill_share(key, n, 0.f, std, z0 + (long long)blockIdx.y * n, z + (long long)blockIdx.y * n);
}

template <bool VEC>
__global__ __launch_bounds__(256) void gaussian_nll_fits_kernel(const float* __restrict__ out, const float* __restrict__ targets, long long target_stride,
                                                                int S, int H, int W, int f, float grad_scale, float* __restrict__ dout,
                                                                double* __restrict__ nll)
{
    __shared__ double s_red[8];
    const int k = blockIdx.y, fit = k / S;
    const long long HW = (long long)H * W;
    const float* __restrict__ o = out + (long long)k * 2 * HW;
    const float* __restrict__ t = targets + (long long)fit * target_stride;
    float* __restrict__ d = dout ? dout + (long long)k * 2 * HW : nullptr;
    const double v = VEC ? gnll_sample_vec(o, t, HW, grad_scale, d) : gnll_sample(o, t, H, W, f, grad_scale, d);
    block_atomic_add(v, nll + fit, s_red);
}

// ---- KL + AdamW of every fit: one kernel pair in three instantiations, so that a batch pays only for what its rows use.
//   <TYPED, MIX> = <0, 0>  every row reverse against its Gaussian prior (mfvi_elbo_update_fits)
//                  <1, 0>  the direction of every row's term from kl_type, read once per block: block-uniform, no branch inside the element loop
//                  <1, 1>  and every row's prior table entry: n == 0 runs the Gaussian prior in the row's direction as <1, 0>; n in
//                          1..MFVI_MIXTURE_MAX the Monte-Carlo mixture term with sample sample0 + fit of the draw's stream (kl_type may be NULL: reverse)
// What row `fit` runs -> false for a direction or an entry the single-fit entries would refuse, which can only be met here: the fit's blocks
// write nothing and its finish block marks it dead.
template <bool TYPED, bool MIX>
__device__ __forceinline__ bool fit_row(const int32_t* __restrict__ kl_type, const mfvi_mixture_prior* __restrict__ mix_tab, int fit, int& kt, mfvi_mixture_prior& mix)
{
    kt = TYPED && kl_type ? kl_type[fit] : MFVI_KL_REVERSE;
    if (MIX) mix = mix_tab[fit]; else mix.n = 0;
    return mix.n == 0 ? (kt == MFVI_KL_REVERSE || kt == MFVI_KL_FORWARD) : mix_prior_fault(mix) == MIX_OK;
}
template <bool TYPED, bool MIX>
__global__ __launch_bounds__(256) void elbo_update_fits_kernel(float* __restrict__ params, float* __restrict__ grads, float* __restrict__ m, float* __restrict__ v,
                                                               long long n_vi, long long n_bn, long long param_stride, long long grad_stride,
                                                               const mfvi_fit_hyper* __restrict__ hyper, const int32_t* __restrict__ kl_type,
                                                               const mfvi_mixture_prior* __restrict__ mix_tab, RngKey key, float b1, float b2, float eps,
                                                               double bc1, float inv_sqrt_bc2, const double* __restrict__ nll,
                                                               const int32_t* __restrict__ dead, double* __restrict__ partial)
{
    __shared__ double s_red[8];
    const int fit = blockIdx.y;
    int kt; mfvi_mixture_prior mix;
    if (!fit_row<TYPED, MIX>(kl_type, mix_tab, fit, kt, mix)) return;
    const mfvi_fit_hyper h = hyper[fit];
    // a fit whose data term is not finite (or that died earlier) keeps parameters and moments; its KL is still reported
    const bool skip = dead[fit] != 0 || !isfinite(nll[fit]);
    const long long po = (long long)fit * param_stride;
    const AdamStep adam{params + po, m + po, v + po, b1, b2, eps, (float)((double)h.lr / bc1), inv_sqrt_bc2};
    float* __restrict__ g = grads + (long long)fit * grad_stride;
    const GaussPrior prior{h.prior_mu, h.prior_sigma};
    double acc;
    if (MIX && mix.n != 0) {
        key = key_now(key);
        key.sample += (uint32_t)fit;
        acc = elbo_update_share_quads(KlMixture(mix, key), g, n_vi, n_bn, h.temp, adam, skip);
    } else if (TYPED && kt == MFVI_KL_FORWARD)
        acc = elbo_update_share(KlForward(prior), g, n_vi, n_bn, h.temp, adam, skip);
    else
        acc = elbo_update_share(KlReverse(prior), g, n_vi, n_bn, h.temp, adam, skip);
    const double tot = block_sum_d(acc, s_red);
    if (threadIdx.x == 0) partial[(long long)fit * ELBO_UPDATE_MAX_BLOCKS + blockIdx.x] = tot;
}
// one block per fit: its partials in block order (the order of elbo_update_finish_kernel), and the sticky dead flag
template <bool TYPED, bool MIX>
__global__ __launch_bounds__(256) void elbo_update_fits_finish_kernel(const double* __restrict__ partial, int n_blocks, const double* __restrict__ nll,
                                                                      const int32_t* __restrict__ kl_type, const mfvi_mixture_prior* __restrict__ mix_tab,
                                                                      int32_t* __restrict__ dead, double* __restrict__ kl_out)
{
    __shared__ double s_red[8];
    const int fit = blockIdx.x;
    int kt; mfvi_mixture_prior mix;
    if (!fit_row<TYPED, MIX>(kl_type, mix_tab, fit, kt, mix)) { if (threadIdx.x == 0) dead[fit] = 1; return; }
    double t = 0;
    for (int b = threadIdx.x; b < n_blocks; b += 256) t += partial[(long long)fit * ELBO_UPDATE_MAX_BLOCKS + b];
    t = block_sum_d(t, s_red);
    if (threadIdx.x == 0) { kl_out[fit] = t; if (!isfinite(nll[fit])) dead[fit] = 1; }
}

__global__ __launch_bounds__(256) void ema_fits_kernel(const float* __restrict__ out, int S, int C, long long HW, float* __restrict__ ema, float w, int first)
{
    const float* __restrict__ o = out + (long long)blockIdx.y * S * C * HW;
    float* __restrict__ e = ema + (long long)blockIdx.y * C * HW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)gridDim.x * 256) {
        float mean, ale;
        (void)sample_means_ema(o, S, C, HW, i, e, w, first, mean, ale);
    }
}

// ---- inpainting (4 outputs: 3 colours through the sigmoid + one log-precision channel, a mask per fit) ----
__global__ __launch_bounds__(256) void gaussian_nll_inp_fits_kernel(const float* __restrict__ out, const float* __restrict__ targets, long long target_stride,
                                                                    const float* __restrict__ masks, long long mask_stride, int mask_channels, int S,
                                                                    long long HW, float grad_scale, float* __restrict__ dout, double* __restrict__ nll)
{
    __shared__ double s_red[8];
    const int k = blockIdx.y, fit = k / S;
    const double v = gnll_inp_sample(out + (long long)k * 4 * HW, targets + (long long)fit * target_stride, masks + (long long)fit * mask_stride, mask_channels, HW,
                                     grad_scale, dout ? dout + (long long)k * 4 * HW : nullptr);
    block_atomic_add(v, nll + fit, s_red);
}

__global__ __launch_bounds__(256) void ema_inp_fits_kernel(const float* __restrict__ out, int S, long long HW, float* __restrict__ ema, float w, int first)
{
    const float* __restrict__ o = out + (long long)blockIdx.y * S * 4 * HW;
    float* __restrict__ e = ema + (long long)blockIdx.y * 4 * HW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)gridDim.x * 256) {
        float a, m[3], e0[3];
        sample_means_ema_inp(o, S, HW, i, e, w, first, m, e0, a);
    }
}

// sum over [3][HW] of (clip(ema, 0, 1) * mask - img * mask)^2 of fit blockIdx.y: this block's partial, in a fixed order
__global__ __launch_bounds__(256) void masked_sq_err_fits_kernel(const float* __restrict__ ema, long long ema_stride, const float* __restrict__ img, long long img_stride,
                                                                 const float* __restrict__ masks, long long mask_stride, int mask_channels, long long HW,
                                                                 double* __restrict__ partial)
{
    __shared__ double s_red[8];
    const int fit = blockIdx.y;
    const float* __restrict__ e = ema + (long long)fit * ema_stride;
    const float* __restrict__ g = img + (long long)fit * img_stride;
    const float* __restrict__ mk = masks + (long long)fit * mask_stride;
    double acc = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < 3 * HW; i += (long long)gridDim.x * 256) {
        const float m = mk[mask_channels == 3 ? i : i % HW];
        const float d = fminf(fmaxf(e[i], 0.f), 1.f) * m - g[i] * m;
        acc += (double)d * (double)d;
    }
    const double tot = block_sum_d(acc, s_red);
    if (threadIdx.x == 0) partial[(long long)fit * MFVI_MASKED_SQ_ERR_BLOCKS + blockIdx.x] = tot;
}
// one block per fit: its partials in block order
__global__ __launch_bounds__(64) void masked_sq_err_fits_finish_kernel(const double* __restrict__ partial, int n_blocks, double* __restrict__ acc)
{
    if (threadIdx.x == 0) {
        double t = 0;
        for (int b = 0; b < n_blocks; ++b) t += partial[(long long)blockIdx.x * MFVI_MASKED_SQ_ERR_BLOCKS + b];
        acc[blockIdx.x] = t;
    }
}

// the argument check of the three mfvi_elbo_update_fits* entries (`entry` names the caller in the message) and their two launches
template <bool TYPED, bool MIX>
int launch_elbo_update_fits(const char* entry, float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, int64_t param_stride, int64_t grad_stride,
                            int n_fits, const mfvi_fit_hyper* hyper_dev, const int32_t* kl_type_dev, const mfvi_mixture_prior* mix_dev, RngKey key, float beta1,
                            float beta2, float eps, int t, const double* nll, int32_t* dead, double* kl_out, void* scratch, void* stream)
{
    if (!params || !grads || !m || !v || !hyper_dev || !nll || !dead || !kl_out || !scratch || n_vi < 0 || n_bn < 0 || t < 1 || n_fits < 1 || n_fits > 65535 ||
        param_stride < 2 * n_vi + n_bn || grad_stride < 2 * n_vi + n_bn || (MIX && n_vi > ((int64_t)1 << 34))) {      // a Philox block index is a 32-bit word
        set_error("%s: bad arguments (t is 1-based, strides >= 2 n_vi + n_bn, scratch of mfvi_elbo_update_fits_scratch_bytes(n_fits) bytes)", entry); return -1; }
    const double bc1 = 1.0 - pow((double)beta1, t), bc2 = 1.0 - pow((double)beta2, t);
    const long long work = n_vi > n_bn ? n_vi : n_bn;      // as mfvi_elbo_update: the same blocks per fit
    const int nb = nblocks(work, ELBO_UPDATE_MAX_BLOCKS);
    hipLaunchKernelGGL((elbo_update_fits_kernel<TYPED, MIX>), dim3(nb, n_fits), dim3(256), 0, (hipStream_t)stream, params, grads, m, v, (long long)n_vi, (long long)n_bn,
                       (long long)param_stride, (long long)grad_stride, hyper_dev, kl_type_dev, mix_dev, key, beta1, beta2, eps, bc1, (float)(1.0 / sqrt(bc2)), nll,
                       (const int32_t*)dead, (double*)scratch);
    hipLaunchKernelGGL((elbo_update_fits_finish_kernel<TYPED, MIX>), dim3(n_fits), dim3(256), 0, (hipStream_t)stream, (const double*)scratch, nb, nll, kl_type_dev, mix_dev,
                       dead, kl_out);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int mfvi_perturb_input_fits(const float* z0, uint64_t seed, uint32_t step, int64_t n_per_fit, int n_fits, uint32_t fit0, float std, float* z, void* stream)
{
    if (!z0 || !z || n_per_fit < 1 || n_fits < 1 || n_fits > 65535) { set_error("perturb_input_fits: bad arguments (n_per_fit=%lld n_fits=%d)", (long long)n_per_fit, n_fits); return -1; }
    RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.stream = (uint32_t)DOMAIN_INPUT << 24; key.sample = fit0; key.step = step; key.step_dev = nullptr;
    hipLaunchKernelGGL(perturb_fits_kernel, dim3(nblocks((n_per_fit + 3) / 4), n_fits), dim3(256), 0, (hipStream_t)stream, key, (long long)n_per_fit, std, z0, z);
    return (int)hipGetLastError();
}

int mfvi_gaussian_nll_fits(const float* out, const float* targets, int64_t target_stride, int n_fits, int S, int H, int W, int factor, float grad_scale,
                           float* dout, double* nll, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!out || !targets || !nll || n_fits < 1 || S < 1 || (long long)n_fits * S > 65535 || factor < 1 || H < 1 || W < 1 || H % factor || W % factor ||
        target_stride < (int64_t)(H / factor) * (W / factor)) {
        set_error("gaussian_nll_fits: bad arguments (n_fits=%d S=%d H=%d W=%d factor=%d target_stride=%lld)", n_fits, S, H, W, factor, (long long)target_stride); return -1; }
    const int n = n_fits * S;
    if (dout && factor > 1) { hipError_t e = hipMemsetAsync(dout, 0, sizeof(float) * (size_t)n * 2 * H * W, st); if (e) return (int)e; }
    const long long npix = (long long)(H / factor) * (W / factor);
    if (factor == 1 && (W & 3) == 0 && !(target_stride & 3) && !(((uintptr_t)out | (uintptr_t)targets | (uintptr_t)dout) & 15))
        hipLaunchKernelGGL(gaussian_nll_fits_kernel<true>, dim3(nblocks(npix / 4, 16), n), dim3(256), 0, st, out, targets, (long long)target_stride, S, H, W, 1, grad_scale, dout, nll);
    else
        hipLaunchKernelGGL(gaussian_nll_fits_kernel<false>, dim3(nblocks(npix, 16), n), dim3(256), 0, st, out, targets, (long long)target_stride, S, H, W, factor, grad_scale, dout, nll);
    return (int)hipGetLastError();
}

int64_t mfvi_elbo_update_fits_scratch_bytes(int n_fits) { return n_fits < 1 ? -1 : (int64_t)n_fits * ELBO_UPDATE_MAX_BLOCKS * (int64_t)sizeof(double); }

int mfvi_elbo_update_fits(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, int64_t param_stride, int64_t grad_stride, int n_fits,
                          const mfvi_fit_hyper* hyper_dev, float beta1, float beta2, float eps, int t, const double* nll, int32_t* dead, double* kl_out,
                          void* scratch, void* stream)
{
    return launch_elbo_update_fits<false, false>("elbo_update_fits", params, grads, m, v, n_vi, n_bn, param_stride, grad_stride, n_fits, hyper_dev, nullptr, nullptr,
                                                 RngKey{}, beta1, beta2, eps, t, nll, dead, kl_out, scratch, stream);
}

int mfvi_elbo_update_fits_typed(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, int64_t param_stride, int64_t grad_stride, int n_fits,
                                const mfvi_fit_hyper* hyper_dev, const int32_t* kl_type_dev, float beta1, float beta2, float eps, int t, const double* nll,
                                int32_t* dead, double* kl_out, void* scratch, void* stream)
{
    if (!kl_type_dev)      // all reverse: the entry above, as it is
        return mfvi_elbo_update_fits(params, grads, m, v, n_vi, n_bn, param_stride, grad_stride, n_fits, hyper_dev, beta1, beta2, eps, t, nll, dead, kl_out, scratch,
                                     stream);
    return launch_elbo_update_fits<true, false>("elbo_update_fits_typed", params, grads, m, v, n_vi, n_bn, param_stride, grad_stride, n_fits, hyper_dev, kl_type_dev,
                                                nullptr, RngKey{}, beta1, beta2, eps, t, nll, dead, kl_out, scratch, stream);
}

int mfvi_elbo_update_fits_mixture(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, int64_t param_stride, int64_t grad_stride,
                                  int n_fits, const mfvi_fit_hyper* hyper_dev, const int32_t* kl_type_dev, const mfvi_mixture_prior* mix_dev, uint64_t seed,
                                  uint32_t sample0, uint32_t step, const int32_t* step_dev, float beta1, float beta2, float eps, int t, const double* nll,
                                  int32_t* dead, double* kl_out, void* scratch, void* stream)
{
    if (!mix_dev)          // no row has a mixture: the entry above, as it is
        return mfvi_elbo_update_fits_typed(params, grads, m, v, n_vi, n_bn, param_stride, grad_stride, n_fits, hyper_dev, kl_type_dev, beta1, beta2, eps, t, nll, dead,
                                           kl_out, scratch, stream);
    return launch_elbo_update_fits<true, true>("elbo_update_fits_mixture", params, grads, m, v, n_vi, n_bn, param_stride, grad_stride, n_fits, hyper_dev, kl_type_dev,
                                               mix_dev, klmc_key(seed, sample0, step, step_dev), beta1, beta2, eps, t, nll, dead, kl_out, scratch, stream);
}

int mfvi_ema_fits(const float* out, int n_fits, int S, int C, int H, int W, float* ema, float weight, int first, void* stream)
{
    if (!out || !ema || n_fits < 1 || n_fits > 65535 || S < 1 || C < 1 || C > 2 || H < 1 || W < 1) { set_error("ema_fits: bad arguments"); return -1; }
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(ema_fits_kernel, dim3(nblocks(HW, 256), n_fits), dim3(256), 0, (hipStream_t)stream, out, S, C, HW, ema, weight, first);
    return (int)hipGetLastError();
}

int mfvi_gaussian_nll_inpainting_fits(const float* out, const float* targets, int64_t target_stride, const float* masks, int64_t mask_stride, int mask_channels,
                                      int n_fits, int S, int H, int W, float grad_scale, float* dout, double* nll, void* stream)
{
    const long long HW = (long long)H * W;
    if (!out || !targets || !masks || !nll || n_fits < 1 || S < 1 || (long long)n_fits * S > 65535 || H < 1 || W < 1 || (mask_channels != 1 && mask_channels != 3) ||
        target_stride < 3 * HW || (mask_stride != 0 && mask_stride < mask_channels * HW)) {
        set_error("gaussian_nll_inpainting_fits: bad arguments (n_fits=%d S=%d H=%d W=%d mask_channels=%d target_stride=%lld mask_stride=%lld)", n_fits, S, H, W,
                  mask_channels, (long long)target_stride, (long long)mask_stride); return -1; }
    hipLaunchKernelGGL(gaussian_nll_inp_fits_kernel, dim3(nblocks(HW, 16), n_fits * S), dim3(256), 0, (hipStream_t)stream, out, targets, (long long)target_stride, masks,
                       (long long)mask_stride, mask_channels, S, HW, grad_scale, dout, nll);
    return (int)hipGetLastError();
}

int mfvi_ema_inpainting_fits(const float* out, int n_fits, int S, int H, int W, float* ema, float weight, int first, void* stream)
{
    if (!out || !ema || n_fits < 1 || n_fits > 65535 || S < 1 || H < 1 || W < 1) { set_error("ema_inpainting_fits: bad arguments"); return -1; }
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(ema_inp_fits_kernel, dim3(nblocks(HW, 256), n_fits), dim3(256), 0, (hipStream_t)stream, out, S, HW, ema, weight, first);
    return (int)hipGetLastError();
}

int mfvi_masked_sq_err_fits(const float* ema, int64_t ema_stride, const float* img, int64_t img_stride, const float* masks, int64_t mask_stride, int mask_channels,
                            int n_fits, int H, int W, double* acc, void* scratch, void* stream)
{
    const long long HW = (long long)H * W;
    if (!ema || !img || !masks || !acc || !scratch || n_fits < 1 || n_fits > 65535 || H < 1 || W < 1 || (mask_channels != 1 && mask_channels != 3) ||
        ema_stride < 3 * HW || img_stride < 3 * HW || (mask_stride != 0 && mask_stride < mask_channels * HW)) {
        set_error("masked_sq_err_fits: bad arguments (n_fits=%d H=%d W=%d mask_channels=%d; strides >= 3 H W, scratch of n_fits * MFVI_MASKED_SQ_ERR_BLOCKS doubles)",
                  n_fits, H, W, mask_channels); return -1; }
    const int nb = nblocks(3 * HW, MFVI_MASKED_SQ_ERR_BLOCKS);
    hipLaunchKernelGGL(masked_sq_err_fits_kernel, dim3(nb, n_fits), dim3(256), 0, (hipStream_t)stream, ema, (long long)ema_stride, img, (long long)img_stride, masks,
                       (long long)mask_stride, mask_channels, HW, (double*)scratch);
    hipLaunchKernelGGL(masked_sq_err_fits_finish_kernel, dim3(n_fits), dim3(64), 0, (hipStream_t)stream, (const double*)scratch, nb, acc);
    return (int)hipGetLastError();
}

}  // extern "C"
