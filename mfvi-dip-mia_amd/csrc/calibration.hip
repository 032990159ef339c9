// Uncertainty calibration (utils/uce.py uceloss, the "UCE" cells of the evaluation notebooks): per-bin statistics of an
// error map against an uncertainty map for GIVEN bin boundaries b[0..n_bins], the scalar UCE over them, the exact min / max of a map (for
// callers that pass no range) and the notebooks' recipe for the runner's ring maps.
//
// Bin rule: element i belongs to the bin k with unc[i] > b[k] && unc[i] <= b[k+1], found by a binary search of comparisons over the
// boundaries (never by arithmetic on (unc - lo) / width, which places edge values differently).  An element equal to b[0], outside
// [b[0], b[n_bins]] or NaN belongs to no bin and still counts in the denominator n -- uceloss's own behaviour (gt on the lowest boundary).
//
// Reproducibility: no floating-point atomics.  Each wave folds its 256 elements per iteration into per-bin wave sums (masked shuffles, fp64;
// lane k % 64 owns bin k), a block adds its waves in wave order, every block writes one record of partials, and one thread per bin adds
// the records in block order.  The grid depends on n alone, so two calls on the same inputs are bit-identical.
#include "common.h"
#include "../../include/mfvi_hip.h"

namespace {

constexpr int UCE_THREADS = 256;
constexpr int UCE_WAVES = UCE_THREADS / 64;
constexpr int UCE_MAX_BLOCKS = 256;
constexpr int UCE_MAX_BINS = MFVI_UCE_MAX_BINS;
constexpr int UCE_SLOTS = UCE_MAX_BINS / 64;        // bins owned by one lane

inline int uce_blocks(long long n)
{
    const long long per_block = 4LL * UCE_THREADS;
    long long b = (n + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > UCE_MAX_BLOCKS ? UCE_MAX_BLOCKS : b));
}

// words (8 bytes each) of one block's record: [n_bins] sum err | [n_bins] sum unc | [n_bins] count (int64) | sum unc over all elements
__host__ __device__ inline long long record_words(int n_bins) { return 3LL * n_bins + 1; }

// the bin of u, or -1: j = the smallest index with u <= b[j] (n_bins + 1 when there is none: u above the range, or NaN);
// j == 0 is u <= b[0], outside the half-open lowest bin
__device__ __forceinline__ int find_bin(float u, const float* b, int n_bins)
{
    int lo = 0, hi = n_bins + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u <= b[mid]) hi = mid; else lo = mid + 1;
    }
    return (lo == 0 || lo > n_bins) ? -1 : lo - 1;
}

// Each thread takes 4 consecutive elements per iteration (group g = base + threadIdx.x of a block-uniform base).  VEC: 16-byte loads
// (n % 4 == 0 and 16-byte aligned pointers); otherwise scalar loads of the same 4 elements with a bounds check on the tail.
template <bool VEC>
__global__ __launch_bounds__(UCE_THREADS) void uce_partial_kernel(const float* __restrict__ err, const float* __restrict__ unc, long long n,
                                                                  const float* __restrict__ bounds, int n_bins, double* __restrict__ scratch)
{
    __shared__ float s_b[UCE_MAX_BINS + 1];
    __shared__ double s_e[UCE_WAVES][UCE_MAX_BINS], s_u[UCE_WAVES][UCE_MAX_BINS];
    __shared__ long long s_c[UCE_WAVES][UCE_MAX_BINS];
    __shared__ double s_red[UCE_WAVES];
    for (int i = threadIdx.x; i <= n_bins; i += UCE_THREADS) s_b[i] = bounds[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc_e[UCE_SLOTS], acc_u[UCE_SLOTS], tot = 0.0;
    long long acc_c[UCE_SLOTS];
#pragma unroll
    for (int s = 0; s < UCE_SLOTS; ++s) { acc_e[s] = 0.0; acc_u[s] = 0.0; acc_c[s] = 0; }
    const long long groups = (n + 3) >> 2;
    for (long long base = (long long)blockIdx.x * UCE_THREADS; base < groups; base += (long long)gridDim.x * UCE_THREADS) {
        const long long p0 = (base + threadIdx.x) * 4;
        const int np = p0 >= n ? 0 : (int)(n - p0 < 4 ? n - p0 : 4);
        float e[4] = {0.f, 0.f, 0.f, 0.f}, u[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            if (np) {
                const float4 ev = *reinterpret_cast<const float4*>(err + p0), uv = *reinterpret_cast<const float4*>(unc + p0);
                e[0] = ev.x; e[1] = ev.y; e[2] = ev.z; e[3] = ev.w;
                u[0] = uv.x; u[1] = uv.y; u[2] = uv.z; u[3] = uv.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (j < np) { e[j] = err[p0 + j]; u[j] = unc[p0 + j]; }
        }
        int bin[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bin[j] = j < np ? find_bin(u[j], s_b, n_bins) : -1;
            if (j < np) tot += (double)u[j];
        }
        for (int k = 0; k < n_bins; ++k) {                   // k, and every branch on it, is uniform over the wave
            double se = 0.0, su = 0.0;
            int c = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = bin[j] == k;
                se += in ? (double)e[j] : 0.0;
                su += in ? (double)u[j] : 0.0;
                c += __popcll(__ballot(in));
            }
            if (c == 0) continue;
            se = wave_sum_d(se);
            su = wave_sum_d(su);
#pragma unroll
            for (int s = 0; s < UCE_SLOTS; ++s)
                if ((k >> 6) == s && lane == (k & 63)) { acc_e[s] += se; acc_u[s] += su; acc_c[s] += c; }
        }
    }
#pragma unroll
    for (int s = 0; s < UCE_SLOTS; ++s) {
        const int k = s * 64 + lane;
        if (k < n_bins) { s_e[wave][k] = acc_e[s]; s_u[wave][k] = acc_u[s]; s_c[wave][k] = acc_c[s]; }
    }
    const double btot = block_sum_d(tot, s_red);             // its barriers also publish s_e / s_u / s_c
    double* __restrict__ rec = scratch + (long long)blockIdx.x * record_words(n_bins);
    long long* __restrict__ rec_c = reinterpret_cast<long long*>(rec + 2LL * n_bins);
    for (int k = threadIdx.x; k < n_bins; k += UCE_THREADS) {
        double be = 0.0, bu = 0.0;
        long long bc = 0;
#pragma unroll
        for (int w = 0; w < UCE_WAVES; ++w) { be += s_e[w][k]; bu += s_u[w][k]; bc += s_c[w][k]; }
        rec[k] = be; rec[n_bins + k] = bu; rec_c[k] = bc;
    }
    if (threadIdx.x == 0) rec[3LL * n_bins] = btot;
}

// one block; thread k < n_bins adds bin k's partials in block order and writes the bin's outputs, thread n_bins the sum over all elements.
// count[n_bins] = n.  sums: [n_bins] sum err | [n_bins] sum unc | sum unc over all elements (the fp64 values the fp32 outputs round).
__global__ __launch_bounds__(UCE_THREADS) void uce_final_kernel(const double* __restrict__ scratch, int nb, long long n, int n_bins,
                                                                long long* __restrict__ count, double* __restrict__ sums,
                                                                float* __restrict__ prop, float* __restrict__ err_in_bin,
                                                                float* __restrict__ unc_in_bin, float* __restrict__ unc_mean)
{
    const long long words = record_words(n_bins);
    for (int k = threadIdx.x; k <= n_bins; k += UCE_THREADS) {
        if (k == n_bins) {
            double t = 0.0;
            for (int b = 0; b < nb; ++b) t += scratch[b * words + 3LL * n_bins];
            sums[2 * n_bins] = t;
            unc_mean[0] = (float)(t / (double)n);
            count[n_bins] = n;
            continue;
        }
        double se = 0.0, su = 0.0;
        long long c = 0;
        for (int b = 0; b < nb; ++b) {
            const double* rec = scratch + b * words;
            se += rec[k]; su += rec[n_bins + k];
            c += reinterpret_cast<const long long*>(rec + 2LL * n_bins)[k];
        }
        count[k] = c; sums[k] = se; sums[n_bins + k] = su;
        prop[k] = (float)((double)c / (double)n);
        const float nanf_ = __builtin_nanf("");
        err_in_bin[k] = c ? (float)(se / (double)c) : nanf_;
        unc_in_bin[k] = c ? (float)(su / (double)c) : nanf_;
    }
}

// uce = sum over the bins with prop > outlier of |unc_in_bin - err_in_bin| * prop, in bin order (fp64 over the fp32 values, rounded once)
__global__ void uce_value_kernel(const float* __restrict__ prop, const float* __restrict__ err_in_bin, const float* __restrict__ unc_in_bin,
                                 int n_bins, double outlier, float* __restrict__ uce)
{
    if (threadIdx.x || blockIdx.x) return;
    double s = 0.0;
    for (int k = 0; k < n_bins; ++k)
        if ((double)prop[k] > outlier) s += fabs((double)unc_in_bin[k] - (double)err_in_bin[k]) * (double)prop[k];
    uce[0] = (float)s;
}

__device__ __forceinline__ void minmax_fold(float v, float& mn, float& mx)
{
    if (v == v) { mn = fminf(mn, v); mx = fmaxf(mx, v); }      // NaN is ignored
}

__device__ __forceinline__ void minmax_block(float& mn, float& mx, float* red)      // result valid in thread 0
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o, 64)); mx = fmaxf(mx, __shfl_xor(mx, o, 64)); }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[2 * w] = mn; red[2 * w + 1] = mx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 0; i < UCE_WAVES; ++i) { mn = fminf(mn, red[2 * i]); mx = fmaxf(mx, red[2 * i + 1]); }
}

template <bool VEC>
__global__ __launch_bounds__(UCE_THREADS) void uce_minmax_partial_kernel(const float* __restrict__ x, long long n, float* __restrict__ part)
{
    __shared__ float s_red[2 * UCE_WAVES];
    float mn = INFINITY, mx = -INFINITY;
    const long long groups = (n + 3) >> 2;
    for (long long g = (long long)blockIdx.x * UCE_THREADS + threadIdx.x; g < groups; g += (long long)gridDim.x * UCE_THREADS) {
        const long long p0 = g * 4;
        if (VEC) {
            const float4 v = *reinterpret_cast<const float4*>(x + p0);
            minmax_fold(v.x, mn, mx); minmax_fold(v.y, mn, mx); minmax_fold(v.z, mn, mx); minmax_fold(v.w, mn, mx);
        } else {
            for (long long p = p0; p < p0 + 4 && p < n; ++p) minmax_fold(x[p], mn, mx);
        }
    }
    minmax_block(mn, mx, s_red);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = mn; part[2 * blockIdx.x + 1] = mx; }
}

__global__ __launch_bounds__(UCE_THREADS) void uce_minmax_final_kernel(const float* __restrict__ part, int nb, float* __restrict__ out)
{
    __shared__ float s_red[2 * UCE_WAVES];
    float mn = INFINITY, mx = -INFINITY;
    for (int b = threadIdx.x; b < nb; b += UCE_THREADS) { mn = fminf(mn, part[2 * b]); mx = fmaxf(mx, part[2 * b + 1]); }
    minmax_block(mn, mx, s_red);
    if (threadIdx.x == 0) { out[0] = mn; out[1] = mx; }
}

// the notebooks' inputs from the runner's arrays: err[i] = mean over the S snapshots of (rec[s][i] - gt[i])^2 (fp64, rounded once),
// times mask[i % mask_len] when there is a mask; unc[i] = epi[i] + ale[i % ale_len] (fp32, as the notebooks add the two maps)
__global__ __launch_bounds__(UCE_THREADS) void uce_ring_inputs_kernel(const float* __restrict__ rec, int S, long long n,
                                                                      const float* __restrict__ gt, const float* __restrict__ mask,
                                                                      long long mask_len, const float* __restrict__ epi,
                                                                      const float* __restrict__ ale, long long ale_len,
                                                                      float* __restrict__ err, float* __restrict__ unc)
{
    for (long long i = (long long)blockIdx.x * UCE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * UCE_THREADS) {
        const double g = (double)gt[i];
        double s = 0.0;
        for (int k = 0; k < S; ++k) { const double d = (double)rec[k * n + i] - g; s += d * d; }
        s /= (double)S;
        if (mask) s *= (double)mask[i % mask_len];
        err[i] = (float)s;
        unc[i] = ale ? epi[i] + ale[i % ale_len] : epi[i];
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int64_t mfvi_uce_scratch_bytes(int64_t n, int n_bins)
{
    if (n < 1 || n_bins < 1 || n_bins > UCE_MAX_BINS) {
        set_error("uce_scratch_bytes: n=%lld n_bins=%d not valid (1 <= n_bins <= %d)", (long long)n, n_bins, UCE_MAX_BINS); return -1;
    }
    return (int64_t)uce_blocks(n) * record_words(n_bins) * 8;
}

int mfvi_uce_minmax(const float* unc, int64_t n, float* minmax, void* scratch, void* stream)
{
    if (!unc || !minmax || !scratch || n < 1) { set_error("uce_minmax: bad arguments (n=%lld)", (long long)n); return -1; }
    const int nb = uce_blocks(n);                    // 2 floats per block: within the scratch of any n_bins >= 1
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)scratch;
    if ((n & 3) == 0 && aligned16(unc)) hipLaunchKernelGGL(uce_minmax_partial_kernel<true>, dim3(nb), dim3(UCE_THREADS), 0, st, unc, (long long)n, part);
    else hipLaunchKernelGGL(uce_minmax_partial_kernel<false>, dim3(nb), dim3(UCE_THREADS), 0, st, unc, (long long)n, part);
    hipError_t e = hipGetLastError(); if (e) return (int)e;
    hipLaunchKernelGGL(uce_minmax_final_kernel, dim3(1), dim3(UCE_THREADS), 0, st, part, nb, minmax);
    return (int)hipGetLastError();
}

int mfvi_uce_bins(const float* err, const float* unc, int64_t n, const float* bounds, int n_bins, void* scratch, int64_t* count, double* sums,
                  float* prop, float* err_in_bin, float* unc_in_bin, float* unc_mean, void* stream)
{
    if (n_bins < 1 || n_bins > UCE_MAX_BINS) { set_error("uce_bins: n_bins=%d outside 1..%d", n_bins, UCE_MAX_BINS); return -2; }
    if (!err || !unc || !bounds || !scratch || !count || !sums || !prop || !err_in_bin || !unc_in_bin || !unc_mean || n < 1) {
        set_error("uce_bins: bad arguments (n=%lld)", (long long)n); return -1;
    }
    const int nb = uce_blocks(n);
    hipStream_t st = (hipStream_t)stream;
    double* rec = (double*)scratch;
    if ((n & 3) == 0 && aligned16(err) && aligned16(unc))
        hipLaunchKernelGGL(uce_partial_kernel<true>, dim3(nb), dim3(UCE_THREADS), 0, st, err, unc, (long long)n, bounds, n_bins, rec);
    else
        hipLaunchKernelGGL(uce_partial_kernel<false>, dim3(nb), dim3(UCE_THREADS), 0, st, err, unc, (long long)n, bounds, n_bins, rec);
    hipError_t e = hipGetLastError(); if (e) return (int)e;
    hipLaunchKernelGGL(uce_final_kernel, dim3(1), dim3(UCE_THREADS), 0, st, rec, nb, (long long)n, n_bins, (long long*)count, sums, prop, err_in_bin,
                       unc_in_bin, unc_mean);
    return (int)hipGetLastError();
}

int mfvi_uce_value(const float* prop, const float* err_in_bin, const float* unc_in_bin, int n_bins, double outlier, float* uce, void* stream)
{
    if (n_bins < 1 || n_bins > UCE_MAX_BINS) { set_error("uce_value: n_bins=%d outside 1..%d", n_bins, UCE_MAX_BINS); return -2; }
    if (!prop || !err_in_bin || !unc_in_bin || !uce) { set_error("uce_value: bad arguments"); return -1; }
    hipLaunchKernelGGL(uce_value_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, prop, err_in_bin, unc_in_bin, n_bins, outlier, uce);
    return (int)hipGetLastError();
}

int mfvi_uce_ring_inputs(const float* rec, int S, int64_t n, const float* gt, const float* mask, int64_t mask_len, const float* epi,
                         const float* ale, int64_t ale_len, float* err, float* unc, void* stream)
{
    if (!rec || !gt || !epi || !err || !unc || S < 1 || n < 1 || (mask && (mask_len < 1 || n % mask_len)) || (ale && (ale_len < 1 || n % ale_len))) {
        set_error("uce_ring_inputs: bad arguments (S=%d n=%lld mask_len=%lld ale_len=%lld)", S, (long long)n, (long long)mask_len, (long long)ale_len);
        return -1;
    }
    long long nb = (n + UCE_THREADS - 1) / UCE_THREADS;
    if (nb > 4096) nb = 4096;
    hipLaunchKernelGGL(uce_ring_inputs_kernel, dim3((unsigned)nb), dim3(UCE_THREADS), 0, (hipStream_t)stream, rec, S, (long long)n, gt, mask,
                       (long long)mask_len, epi, ale, (long long)ale_len, err, unc);
    return (int)hipGetLastError();
}

}  // extern "C"
