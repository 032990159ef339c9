// The element-wise passes of one iteration of the non-Bayesian siblings (plain deep image prior, MC dropout, SGLD) for MANY independent fits
// in one launch each (the plan side is mfvi_plan_set_fits_points / mfvi_plan_set_fit_dropout): the one-channel MSE, AdamW
// with decoupled weight decay and a per-fit ExponentialLR, SGLD's parameter noise.  Per fit they compute what mfvi_mse_channel /
// mfvi_adamw_step / mfvi_add_normal compute for it alone.  Reductions are fp64 sums in a fixed order, nothing uses a floating-point atomic.
// The reference runs one process per candidate instead (bayesian_optimization.py:1064-1237, 1447-1655, 1658-1860).
#include "common.h"
#include "iter_ops.h"
#include "../../include/mfvi_hip.h"

namespace {

constexpr int NOISE_BLOCKS = 64;      // blocks per (layer, fit) of the noise launch: grid-stride over the layer's Philox blocks

// One block per fit: its S samples one after the other, the pixels strided over the block's threads -- the per-pixel code of mse_channel_kernel
__global__ __launch_bounds__(1024) void mse_channel_fits_kernel(const float* __restrict__ out, const float* __restrict__ targets, long long target_stride,
                                                                int S, int C, int H, int W, int channel, int f, float grad_scale,
                                                                float* __restrict__ dout, double* __restrict__ mse_acc)
{
    __shared__ double s_red[32];
    const int fit = blockIdx.x;
    const long long HW = (long long)H * W;
    const int w = W / f; const long long n = (long long)(H / f) * w;
    const float* __restrict__ target = targets + (long long)fit * target_stride;
    const float gs = grad_scale * 2.f / (float)n;
    double acc = 0;
    for (int s = 0; s < S; ++s) {
        const long long k = (long long)fit * S + s;
        const float* __restrict__ o = out + k * C * HW;
        float* __restrict__ d = dout ? dout + k * C * HW : nullptr;
        for (long long i = threadIdx.x; i < HW; i += blockDim.x) {
            const int y = (int)(i / W), x = (int)(i - (long long)y * W);
            float g = 0.f;
            if (y % f == 0 && x % f == 0 && y / f < H / f && x / f < w) {
                const float df = o[channel * HW + i] - target[(long long)(y / f) * w + x / f];
                acc += (double)(df * df); g = gs * df;
            }
            if (d) for (int c = 0; c < C; ++c) d[c * HW + i] = c == channel ? g : 0.f;
        }
    }
    // lanes of a wave, then the waves in order: the same order on every call
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += s_red[i];
        mse_acc[fit] += t / (double)n;
    }
}

// grid y = fit.  The per-element arithmetic of adam_kernel (losses.hip) with the host-side scalars of mfvi_adamw_step formed per fit
__global__ __launch_bounds__(256) void sibling_update_fits_kernel(float* __restrict__ params, const float* __restrict__ grads, float* __restrict__ m,
                                                                  float* __restrict__ v, long long n_vi, long long n_bn, long long param_stride,
                                                                  long long grad_stride, const mfvi_sibling_hyper* __restrict__ hyper, float b1, float b2,
                                                                  float eps, double bc1, float inv_sqrt_bc2, const double* __restrict__ loss_acc,
                                                                  const int32_t* __restrict__ dead)
{
    const int fit = blockIdx.y;
    if (dead[fit] != 0 || !isfinite(loss_acc[fit])) return;      // (uniform per block)
    const mfvi_sibling_hyper h = hyper[fit];
    const float lr = (float)h.lr;                                 // the float32 a caller of mfvi_adamw_step hands over
    const float step_size = (float)((double)lr / bc1);
    const float decay = __fsub_rn(1.0f, __fmul_rn(lr, h.weight_decay));      // two roundings, as the host forms it
    const long long po = (long long)fit * param_stride, go = (long long)fit * grad_stride;
    float* __restrict__ p = params + po; const float* __restrict__ g = grads + go;
    float* __restrict__ mm = m + po; float* __restrict__ vv = v + po;
    const long long n = n_vi + n_bn;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n; q += (long long)gridDim.x * 256) {
        const long long i = q < n_vi ? q : q + n_vi;              // MU block, then the BN block behind RHO
        const float gi = g[i];
        const float mi = b1 * mm[i] + (1.f - b1) * gi;
        const float vi = b2 * vv[i] + (1.f - b2) * gi * gi;
        mm[i] = mi; vv[i] = vi;
        p[i] = p[i] * decay - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
    }
}
// one block behind the update (stream order: no block of the update reads an lr written here): the sticky dead flags, then the decay of
// every live fit's lr, in fp64
__global__ __launch_bounds__(256) void sibling_update_fits_tail_kernel(mfvi_sibling_hyper* __restrict__ hyper, int n_fits, const double* __restrict__ loss_acc,
                                                                       int32_t* __restrict__ dead)
{
    for (int f = threadIdx.x; f < n_fits; f += 256) {
        if (!isfinite(loss_acc[f])) dead[f] = 1;
        if (dead[f] != 0) continue;
        const double lr = hyper[f].lr;
        if (lr > (double)hyper[f].lr_floor) hyper[f].lr = lr * hyper[f].gamma;
    }
}

// grid: x = blocks over the layer, y = layer, z = fit
__global__ __launch_bounds__(256) void add_normal_fits_kernel(float* __restrict__ params, long long param_stride, const int64_t* __restrict__ layer_off,
                                                              const int64_t* __restrict__ layer_n, RngKey key, const float* __restrict__ std,
                                                              const int32_t* __restrict__ dead)
{
    const int fit = blockIdx.z, layer = blockIdx.y;
    if (dead && dead[fit] != 0) return;
    key.stream = ((uint32_t)DOMAIN_SGLD << 24) | (uint32_t)layer;
    key.sample += (uint32_t)fit;
    const long long n = layer_n[layer];
    float* __restrict__ x = params + (long long)fit * param_stride + layer_off[layer];
    const float sd = std[fit];
    const long long nblk = (n + 3) >> 2;
    for (long long blk = (long long)blockIdx.x * 256 + threadIdx.x; blk < nblk; blk += (long long)gridDim.x * 256) {
        float z[4]; spec_normal4(key, (uint32_t)blk, z);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const long long j = blk * 4 + l;
            if (j < n) x[j] = __builtin_fmaf(sd, z[l], x[j]);
        }
    }
}

}  // namespace

extern "C" {

int mfvi_mse_channel_fits(const float* out, const float* targets, int64_t target_stride, int n_fits, int S, int C, int H, int W, int channel, int factor,
                          float grad_scale, float* dout, double* mse_acc, void* stream)
{
    if (!out || !targets || !mse_acc || n_fits < 1 || S < 1 || (long long)n_fits * S > 65535 || C < 1 || channel < 0 || channel >= C || H < 1 || W < 1 ||
        factor < 1 || H / factor < 1 || W / factor < 1) {
        set_error("mse_channel_fits: bad arguments (n_fits=%d S=%d C=%d H=%d W=%d channel=%d factor=%d)", n_fits, S, C, H, W, channel, factor); return -1; }
    if (target_stride < (int64_t)(H / factor) * (W / factor)) {
        set_error("mse_channel_fits: target_stride %lld is shorter than a target of %d x %d", (long long)target_stride, H / factor, W / factor); return -1; }
    hipLaunchKernelGGL(mse_channel_fits_kernel, dim3(n_fits), dim3(1024), 0, (hipStream_t)stream, out, targets, (long long)target_stride, S, C, H, W, channel,
                       factor, grad_scale, dout, mse_acc);
    return (int)hipGetLastError();
}

int mfvi_sibling_update_fits(float* params, float* grads, float* m, float* v, int64_t n_vi, int64_t n_bn, int64_t param_stride, int64_t grad_stride,
                             int n_fits, mfvi_sibling_hyper* hyper_dev, float beta1, float beta2, float eps, int t, const double* loss_acc, int32_t* dead,
                             void* stream)
{
    if (!params || !grads || !m || !v || !hyper_dev || !loss_acc || !dead || n_vi < 0 || n_bn < 0 || t < 1 || n_fits < 1 || n_fits > 65535 ||
        param_stride < 2 * n_vi + n_bn || grad_stride < 2 * n_vi + n_bn) {
        set_error("sibling_update_fits: bad arguments (t is 1-based, strides >= 2 n_vi + n_bn)"); return -1; }
    const double bc1 = 1.0 - pow((double)beta1, t), bc2 = 1.0 - pow((double)beta2, t);
    long long nb = (n_vi + n_bn + 255) / 256; nb = nb < 1 ? 1 : (nb > 2048 ? 2048 : nb);
    hipLaunchKernelGGL(sibling_update_fits_kernel, dim3((unsigned)nb, n_fits), dim3(256), 0, (hipStream_t)stream, params, (const float*)grads, m, v, (long long)n_vi,
                       (long long)n_bn, (long long)param_stride, (long long)grad_stride, (const mfvi_sibling_hyper*)hyper_dev, beta1, beta2, eps, bc1,
                       (float)(1.0 / sqrt(bc2)), loss_acc, (const int32_t*)dead);
    hipLaunchKernelGGL(sibling_update_fits_tail_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hyper_dev, n_fits, loss_acc, dead);
    return (int)hipGetLastError();
}

int mfvi_add_normal_fits(float* params, int64_t param_stride, int n_fits, uint32_t fit0, const int64_t* layer_off, const int64_t* layer_n, int n_layers,
                         uint64_t seed, uint32_t step, const float* std, const int32_t* dead, void* stream)
{
    if (!params || !layer_off || !layer_n || !std || param_stride < 0 || n_fits < 1 || n_fits > 65535 || n_layers < 0 || n_layers > 65535) {
        set_error("add_normal_fits: bad arguments (n_fits=%d n_layers=%d)", n_fits, n_layers); return -1; }
    if (n_layers == 0) return 0;
    RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.stream = (uint32_t)DOMAIN_SGLD << 24; key.sample = fit0; key.step = step; key.step_dev = nullptr;
    hipLaunchKernelGGL(add_normal_fits_kernel, dim3(NOISE_BLOCKS, n_layers, n_fits), dim3(256), 0, (hipStream_t)stream, params, (long long)param_stride, layer_off,
                       layer_n, key, std, dead);
    return (int)hipGetLastError();
}

}  // extern "C"
