// Posterior predictive statistics over N forward draws of the fitted net (BayTorch/inference/utils.py:11-24 uncert_regression_gal,
// the per-pixel quantities of the evaluation notebooks' uceloss inputs): the draws arrive in chunks out[n][C][H][W] (as mfvi_forward
// writes them), each chunk folds into a per-pixel fp64 accumulator, and one finalize pass turns the sums into the fp32 maps.
//
// Accumulator (doubles): [ sum m (Cimg*HW) | sum m^2 (Cimg*HW) | sum a (HW, absent in MEAN_ONLY) | 3 * PRED_FIN_BLOCKS finalize partials ]
// Every accumulator word is owned by ONE thread of the accumulate kernel, which adds the chunk's samples to it in increasing k: the
// summation order of every pixel is sample 0, 1, ..., N-1 whatever the chunking, so the maps are bit-identical for any chunking of the
// same per-sample outputs.  No atomics; the scalar reductions of the finalize pass run in a fixed order too (block sums, then one block
// over the partials).
#include "common.h"
#include "../../include/mfvi_hip.h"

namespace {

constexpr int PRED_ACC_THREADS = 64;        // one wave per block: at 256^2 one channel plane is 256 blocks, enough to cover the device
constexpr int PRED_KB = 8;                  // samples whose loads are issued together before they are summed (in order); 16 (one round
                                            // of loads per chunk of 16) measured 12.1 us per launch at 256^2, 8: 10.0-10.9 us
constexpr int PRED_FIN_THREADS = 256;
constexpr int PRED_FIN_BLOCKS = 256;        // finalize grid cap: the partials region of the accumulator holds 3 doubles per block

enum { TR_ID = 0, TR_SIGMOID = 1, TR_EXPNEG = 2 };

struct PredLayout {
    int cimg, has_ale, y_mean0, y_ale, tr_mean, tr_ale;     // image channels, aleatoric map?, first mean channel of y, ale channel of y
};

bool pred_layout(int C, int mode, PredLayout& L)
{
    switch (mode) {
    case MFVI_PRED_RAW:       if (C < 2) return false; L = {C - 1, 1, 0, C - 1, TR_ID, TR_ID}; return true;
    case MFVI_PRED_LOGPREC:   if (C != 2) return false; L = {1, 1, 0, 1, TR_ID, TR_EXPNEG}; return true;
    case MFVI_PRED_INP:       if (C != 4) return false; L = {3, 1, 0, 3, TR_SIGMOID, TR_EXPNEG}; return true;
    case MFVI_PRED_MEAN_ONLY: if (C != 1) return false; L = {1, 0, 0, -1, TR_ID, TR_ID}; return true;
    default: return false;
    }
}

__device__ __forceinline__ float pred_tr(float y, int tr, int clip)
{
    float v = tr == TR_SIGMOID ? sigmoid_f(y) : (tr == TR_EXPNEG ? expf(-y) : y);
    return clip ? fminf(fmaxf(v, 0.f), 1.f) : v;
}

// grid (ceil(HW / (4 * 64)), Cimg + has_ale).  blockIdx.y < Cimg: image channel c -> sum m, sum m^2 of that channel; the last row: sum a.
// Each thread owns 4 consecutive pixels of one plane.  VEC: 16-byte loads (HW % 4 == 0 and a 16-byte aligned chunk); otherwise scalar
// loads of the same 4 pixels with a bounds check on the tail.  The thread's work is one function for the single-fit kernel and the one with
// the fit as grid z (as iter_ops.h serves fits.hip): the same arithmetic in the same order, so the two agree bit for bit.
template <bool VEC>
__device__ __forceinline__ void pred_accumulate_thread(const float* __restrict__ out, int n, int C, long long HW, const PredLayout& lay, int clip,
                                                       int first, double* __restrict__ acc)
{
    const long long p0 = ((long long)blockIdx.x * PRED_ACC_THREADS + threadIdx.x) * 4;
    if (p0 >= HW) return;
    const int row = blockIdx.y;
    const bool is_ale = row >= lay.cimg;
    const int ych = is_ale ? lay.y_ale : lay.y_mean0 + row;
    const int tr = is_ale ? lay.tr_ale : lay.tr_mean;
    const long long sstride = (long long)C * HW;
    const float* __restrict__ src = out + (long long)ych * HW + p0;
    const int np = (int)(HW - p0 < 4 ? HW - p0 : 4);
    double* __restrict__ s_dst = is_ale ? acc + 2LL * lay.cimg * HW + p0 : acc + (long long)row * HW + p0;
    double* __restrict__ q_dst = acc + (long long)(lay.cimg + row) * HW + p0;        // not used for the ale row
    double s[4], q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s[j] = (first || j >= np) ? 0.0 : s_dst[j];
        q[j] = (first || j >= np || is_ale) ? 0.0 : q_dst[j];
    }
    for (int k0 = 0; k0 < n; k0 += PRED_KB) {
        float4 v[PRED_KB];
#pragma unroll
        for (int b = 0; b < PRED_KB; ++b) {
            v[b] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 + b < n) {
                const float* sp = src + (long long)(k0 + b) * sstride;
                if (VEC) v[b] = *reinterpret_cast<const float4*>(sp);
                else {
                    v[b].x = sp[0];
                    if (np > 1) v[b].y = sp[1];
                    if (np > 2) v[b].z = sp[2];
                    if (np > 3) v[b].w = sp[3];
                }
            }
        }
#pragma unroll
        for (int b = 0; b < PRED_KB; ++b) {
            if (k0 + b < n) {
                const float e[4] = {v[b].x, v[b].y, v[b].z, v[b].w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double m = (double)pred_tr(e[j], tr, clip);
                    s[j] += m;
                    q[j] += m * m;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < np) {
            s_dst[j] = s[j];
            if (!is_ale) q_dst[j] = q[j];
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(PRED_ACC_THREADS) void pred_accumulate_kernel(const float* __restrict__ out, int n, int C, long long HW,
                                                                           PredLayout lay, int clip, int first, double* __restrict__ acc)
{
    pred_accumulate_thread<VEC>(out, n, C, HW, lay, clip, first, acc);
}

// grid z = fit: fit f folds its first n_use samples out[f * S ..] into its own accumulator row
template <bool VEC>
__global__ __launch_bounds__(PRED_ACC_THREADS) void pred_accumulate_fits_kernel(const float* __restrict__ out, int S, int n_use, int C, long long HW,
                                                                                PredLayout lay, int clip, int first, double* __restrict__ acc,
                                                                                long long acc_stride)
{
    const long long f = blockIdx.z;
    pred_accumulate_thread<VEC>(out + f * S * C * HW, n_use, C, HW, lay, clip, first, acc + f * acc_stride);
}

// per pixel: mean[c] = S/N, epi = mean_c max-clamped unbiased variance, ale = A/N, total = ale + epi, and with a ground truth
// err2 = mean_c (mean[c] - g[c])^2, mse_mc = err2 + (N-1)/N * epi.  Per-block fp64 partials of sum ale / sum epi / sum total.
// The thread's pixels, shared by the single-fit kernel and the one with the fit as grid y; sa / se / st / sr: the thread's sums of the
// stored ale / epi / total / err2 values.
__device__ __forceinline__ void pred_finalize_thread(const double* __restrict__ acc, int N, long long HW, const PredLayout& lay,
                                                     const float* __restrict__ ref, float* __restrict__ mean, float* __restrict__ epi,
                                                     float* __restrict__ ale, float* __restrict__ total, float* __restrict__ err2,
                                                     float* __restrict__ mse_mc, double& sa, double& se, double& st, double& sr)
{
    const double inv_n = 1.0 / N, inv_n1 = 1.0 / (N - 1);
    const double* __restrict__ S = acc;
    const double* __restrict__ Q = acc + (long long)lay.cimg * HW;
    const double* __restrict__ A = acc + 2LL * lay.cimg * HW;
    for (long long p = (long long)blockIdx.x * PRED_FIN_THREADS + threadIdx.x; p < HW; p += (long long)gridDim.x * PRED_FIN_THREADS) {
        double var = 0, e2 = 0;
        for (int c = 0; c < lay.cimg; ++c) {
            const double s = S[c * HW + p], q = Q[c * HW + p];
            const double mu = s * inv_n;
            var += (q - s * mu) * inv_n1;
            const float mf = (float)mu;
            mean[c * HW + p] = mf;
            if (ref) { const double d = (double)mf - (double)ref[c * HW + p]; e2 += d * d; }
        }
        double ep = var / lay.cimg;
        ep = ep > 0.0 ? ep : 0.0;
        const float epf = (float)ep;
        epi[p] = epf;
        float tf = epf;
        if (lay.has_ale) {
            const float af = (float)(A[p] * inv_n);
            ale[p] = af;
            tf = (float)((double)af + (double)epf);
            sa += af;
        }
        total[p] = tf;
        se += epf; st += tf;
        if (ref) {
            const double e2m = e2 / lay.cimg;
            if (err2) err2[p] = (float)e2m;
            if (mse_mc) mse_mc[p] = (float)(e2m + (double)(N - 1) * inv_n * (double)epf);
            sr += (float)e2m;
        }
    }
}

__global__ __launch_bounds__(PRED_FIN_THREADS) void pred_finalize_kernel(const double* __restrict__ acc, int N, long long HW, PredLayout lay,
                                                                         const float* __restrict__ ref, float* __restrict__ mean,
                                                                         float* __restrict__ epi, float* __restrict__ ale,
                                                                         float* __restrict__ total, float* __restrict__ err2,
                                                                         float* __restrict__ mse_mc, double* __restrict__ partials)
{
    __shared__ double s_red[PRED_FIN_THREADS / 64];
    double sa = 0, se = 0, st = 0, sr = 0;
    pred_finalize_thread(acc, N, HW, lay, ref, mean, epi, ale, total, err2, mse_mc, sa, se, st, sr);
    const double ba = block_sum_d(sa, s_red);
    const double be = block_sum_d(se, s_red);
    const double bt = block_sum_d(st, s_red);
    if (threadIdx.x == 0) { partials[3 * blockIdx.x] = ba; partials[3 * blockIdx.x + 1] = be; partials[3 * blockIdx.x + 2] = bt; }
}

// grid (blocks, fit): fit f's maps from its accumulator row; its partials hold a fourth word per block, the sum of err2
__global__ __launch_bounds__(PRED_FIN_THREADS) void pred_finalize_fits_kernel(double* acc, long long acc_stride, int N, long long HW,
                                                                              PredLayout lay, const float* __restrict__ ref, long long ref_stride,
                                                                              float* __restrict__ mean, float* __restrict__ epi,
                                                                              float* __restrict__ ale, float* __restrict__ total,
                                                                              float* __restrict__ err2, float* __restrict__ mse_mc, long long state)
{
    __shared__ double s_red[PRED_FIN_THREADS / 64];
    const long long f = blockIdx.y;
    double* __restrict__ partials = acc + f * acc_stride + state;      // behind the words the threads read
    double sa = 0, se = 0, st = 0, sr = 0;
    pred_finalize_thread(acc + f * acc_stride, N, HW, lay, ref ? ref + f * ref_stride : nullptr, mean + f * lay.cimg * HW, epi + f * HW,
                         ale ? ale + f * HW : nullptr, total + f * HW, err2 ? err2 + f * HW : nullptr, mse_mc ? mse_mc + f * HW : nullptr, sa, se, st, sr);
    const double ba = block_sum_d(sa, s_red);
    const double be = block_sum_d(se, s_red);
    const double bt = block_sum_d(st, s_red);
    const double br = block_sum_d(sr, s_red);
    if (threadIdx.x == 0) { partials[4 * blockIdx.x] = ba; partials[4 * blockIdx.x + 1] = be; partials[4 * blockIdx.x + 2] = bt; partials[4 * blockIdx.x + 3] = br; }
}

// one block: sums[j] = sum over the finalize blocks of partials[NS b + j], strided per thread then one block sum (a fixed order)
template <int NS>
__device__ __forceinline__ void pred_sums_block(const double* __restrict__ partials, int nb, double* __restrict__ sums, double* s_red)
{
    for (int j = 0; j < NS; ++j) {
        double v = 0;
        for (int b = threadIdx.x; b < nb; b += PRED_FIN_THREADS) v += partials[NS * b + j];
        const double t = block_sum_d(v, s_red);
        if (threadIdx.x == 0) sums[j] = t;
    }
}

__global__ __launch_bounds__(PRED_FIN_THREADS) void pred_sums_kernel(const double* __restrict__ partials, int nb, double* __restrict__ sums)
{
    __shared__ double s_red[PRED_FIN_THREADS / 64];
    pred_sums_block<3>(partials, nb, sums, s_red);
}

// one block per fit: sums[f][0..3] from that fit's partials
__global__ __launch_bounds__(PRED_FIN_THREADS) void pred_sums_fits_kernel(const double* __restrict__ acc, long long acc_stride, long long state, int nb,
                                                                          double* __restrict__ sums)
{
    __shared__ double s_red[PRED_FIN_THREADS / 64];
    pred_sums_block<4>(acc + (long long)blockIdx.x * acc_stride + state, nb, sums + 4 * blockIdx.x, s_red);
}

inline int fin_blocks(long long HW)
{
    long long b = (HW + PRED_FIN_THREADS - 1) / PRED_FIN_THREADS;
    return (int)(b < 1 ? 1 : (b > PRED_FIN_BLOCKS ? PRED_FIN_BLOCKS : b));
}

}  // namespace

extern "C" {

int64_t mfvi_predictive_acc_doubles(int C, int H, int W, int mode)
{
    PredLayout lay;
    if (H < 1 || W < 1 || !pred_layout(C, mode, lay)) { set_error("predictive_acc_doubles: C=%d mode=%d H=%d W=%d not valid", C, mode, H, W); return -1; }
    const long long HW = (long long)H * W;
    return (2LL * lay.cimg + lay.has_ale) * HW + 3LL * PRED_FIN_BLOCKS;
}

int mfvi_predictive_accumulate(const float* out, int n, int C, int H, int W, int mode, int clip, int first, double* acc, void* stream)
{
    PredLayout lay;
    if (!out || !acc || n < 1 || H < 1 || W < 1 || !pred_layout(C, mode, lay)) {
        set_error("predictive_accumulate: bad arguments (n=%d C=%d mode=%d H=%d W=%d)", n, C, mode, H, W); return -1;
    }
    const long long HW = (long long)H * W;
    const dim3 grid((unsigned)((HW + 4 * PRED_ACC_THREADS - 1) / (4 * PRED_ACC_THREADS)), (unsigned)(lay.cimg + lay.has_ale));
    const bool vec = (HW & 3) == 0 && ((uintptr_t)out & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(pred_accumulate_kernel<true>, grid, dim3(PRED_ACC_THREADS), 0, st, out, n, C, HW, lay, clip, first, acc);
    else hipLaunchKernelGGL(pred_accumulate_kernel<false>, grid, dim3(PRED_ACC_THREADS), 0, st, out, n, C, HW, lay, clip, first, acc);
    return (int)hipGetLastError();
}

int mfvi_predictive_finalize(double* acc, int n_total, int C, int H, int W, int mode, const float* ref, float* mean, float* epi, float* ale,
                             float* total, float* err2, float* mse_mc, double* sums, void* stream)
{
    PredLayout lay;
    if (!acc || !mean || !epi || !total || !sums || H < 1 || W < 1 || !pred_layout(C, mode, lay) || (lay.has_ale && !ale)) {
        set_error("predictive_finalize: bad arguments (C=%d mode=%d H=%d W=%d)", C, mode, H, W); return -1;
    }
    if (n_total < 2) { set_error("predictive_finalize: %d samples; the unbiased variance needs at least 2", n_total); return -1; }
    const long long HW = (long long)H * W;
    const int nb = fin_blocks(HW);
    double* partials = acc + (2LL * lay.cimg + lay.has_ale) * HW;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pred_finalize_kernel, dim3(nb), dim3(PRED_FIN_THREADS), 0, st, acc, n_total, HW, lay, ref, mean, epi,
                       lay.has_ale ? ale : nullptr, total, ref ? err2 : nullptr, ref ? mse_mc : nullptr, partials);
    hipError_t e = hipGetLastError(); if (e) return (int)e;
    hipLaunchKernelGGL(pred_sums_kernel, dim3(1), dim3(PRED_FIN_THREADS), 0, st, partials, nb, sums);
    return (int)hipGetLastError();
}

int64_t mfvi_predictive_acc_doubles_fits(int C, int H, int W, int mode)
{
    PredLayout lay;
    if (H < 1 || W < 1 || !pred_layout(C, mode, lay)) { set_error("predictive_acc_doubles_fits: C=%d mode=%d H=%d W=%d not valid", C, mode, H, W); return -1; }
    const long long HW = (long long)H * W;
    return (2LL * lay.cimg + lay.has_ale) * HW + 4LL * PRED_FIN_BLOCKS;
}

int mfvi_predictive_accumulate_fits(const float* out, int n_fits, int S, int n_use, int C, int H, int W, int mode, int clip, int first,
                                    double* acc, int64_t acc_stride, void* stream)
{
    PredLayout lay;
    if (!out || !acc || H < 1 || W < 1 || !pred_layout(C, mode, lay)) {
        set_error("predictive_accumulate_fits: bad arguments (C=%d mode=%d H=%d W=%d)", C, mode, H, W); return -1;
    }
    if (n_fits < 1 || S < 1 || n_fits > 65535 || (long long)n_fits * S > 65535 || n_use < 1 || n_use > S) {
        set_error("predictive_accumulate_fits: n_fits=%d, S=%d, n_use=%d: at least 1 each, n_fits and n_fits * S below 65536, n_use <= S", n_fits, S, n_use); return -1;
    }
    const long long HW = (long long)H * W;
    if (acc_stride < (2LL * lay.cimg + lay.has_ale) * HW + 4LL * PRED_FIN_BLOCKS) {
        set_error("predictive_accumulate_fits: acc_stride %lld below the %lld doubles of one fit (mfvi_predictive_acc_doubles_fits)", (long long)acc_stride,
                  (2LL * lay.cimg + lay.has_ale) * HW + 4LL * PRED_FIN_BLOCKS); return -1;
    }
    const dim3 grid((unsigned)((HW + 4 * PRED_ACC_THREADS - 1) / (4 * PRED_ACC_THREADS)), (unsigned)(lay.cimg + lay.has_ale), (unsigned)n_fits);
    // every fit's slice of out starts 16-byte aligned: out itself and the S * C * HW floats between two fits
    const bool vec = (HW & 3) == 0 && ((uintptr_t)out & 15) == 0 && (((long long)S * C * HW) & 3) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(pred_accumulate_fits_kernel<true>, grid, dim3(PRED_ACC_THREADS), 0, st, out, S, n_use, C, HW, lay, clip, first, acc, (long long)acc_stride);
    else hipLaunchKernelGGL(pred_accumulate_fits_kernel<false>, grid, dim3(PRED_ACC_THREADS), 0, st, out, S, n_use, C, HW, lay, clip, first, acc, (long long)acc_stride);
    return (int)hipGetLastError();
}

int mfvi_predictive_finalize_fits(double* acc, int64_t acc_stride, int n_fits, int n_total, int C, int H, int W, int mode, const float* ref,
                                  int64_t ref_stride, float* mean, float* epi, float* ale, float* total, float* err2, float* mse_mc, double* sums,
                                  void* stream)
{
    PredLayout lay;
    if (!acc || !mean || !epi || !total || !sums || H < 1 || W < 1 || !pred_layout(C, mode, lay) || (lay.has_ale && !ale)) {
        set_error("predictive_finalize_fits: bad arguments (C=%d mode=%d H=%d W=%d)", C, mode, H, W); return -1;
    }
    if (n_fits < 1 || n_fits > 65535) { set_error("predictive_finalize_fits: n_fits %d outside 1..65535", n_fits); return -1; }
    if (n_total < 2) { set_error("predictive_finalize_fits: %d samples; the unbiased variance needs at least 2", n_total); return -1; }
    const long long HW = (long long)H * W, state = (2LL * lay.cimg + lay.has_ale) * HW;
    if (acc_stride < state + 4LL * PRED_FIN_BLOCKS) {
        set_error("predictive_finalize_fits: acc_stride %lld below the %lld doubles of one fit (mfvi_predictive_acc_doubles_fits)", (long long)acc_stride,
                  state + 4LL * PRED_FIN_BLOCKS); return -1;
    }
    if (ref && ref_stride != 0 && ref_stride < lay.cimg * HW) {
        set_error("predictive_finalize_fits: ref_stride %lld: 0 (one ground truth for all fits) or at least the %lld floats of one", (long long)ref_stride, lay.cimg * HW); return -1;
    }
    const int nb = fin_blocks(HW);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pred_finalize_fits_kernel, dim3(nb, n_fits), dim3(PRED_FIN_THREADS), 0, st, acc, (long long)acc_stride, n_total, HW, lay, ref,
                       (long long)ref_stride, mean, epi, lay.has_ale ? ale : nullptr, total, ref ? err2 : nullptr, ref ? mse_mc : nullptr, state);
    hipError_t e = hipGetLastError(); if (e) return (int)e;
    hipLaunchKernelGGL(pred_sums_fits_kernel, dim3(n_fits), dim3(PRED_FIN_THREADS), 0, st, acc, (long long)acc_stride, state, nb, sums);
    return (int)hipGetLastError();
}

}  // extern "C"
