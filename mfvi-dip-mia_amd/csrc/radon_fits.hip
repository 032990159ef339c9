// K7c — the Radon MSE data term of MANY independent CT fits in three launches, whatever their number: what
// mfvi_radon_mse computes for one fit (bayesian_optimization.py:576, radon/radon.py:49-53) in the accumulation contract of
// mfvi_gaussian_nll_fits, on the plane kernels of radon_planes.hip.
//   1. project + residual : the row loop of mfvi_radon_project (radon_rows.h: the same block ownership, clip, fp64 coordinates and
//                           accumulator, wave-order combine).  Where that kernel writes the ray sum, wave 0 here subtracts the bin of the
//                           fit's sinogram, writes grad_scale * 2 d / (T S) into the residual plane and reduces (double)(d * d) over
//                           its live lanes by a fixed butterfly into ONE fp64 partial per block.
//   2. finish             : one block per fit adds the fit's S_per_fit * T * strips partials in a fixed order, divides by T S and adds
//                           into mse[fit].
//   3. mfvi_radon_backproject of the residual planes into dout, as it is.
// No floating-point atomics anywhere: bit-identical from call to call (the double atomicAdd of mfvi_radon_mse is not).
#include "common.h"
#include "radon_rows.h"
#include "../../include/mfvi_hip.h"

namespace {

using namespace radon_rows;

template <bool PAIR>
__global__ __launch_bounds__(64 * MAX_WAVES) void radon_residual_kernel(const float* __restrict__ img, const float* __restrict__ theta, int S,
                                                                         int T, int strips, int chunk, const float* __restrict__ sinos,
                                                                         long long sino_stride, int S_per_fit, float grad_scale,
                                                                         float* __restrict__ resid, double* __restrict__ partials)
{
    __shared__ double part[MAX_WAVES][64];
    Ray r;
    const double tot = project_rows<PAIR>(img, theta, S, strips, chunk, part, r);
    if (threadIdx.x < 64) {                                                          // wave 0, all 64 lanes: the butterfly needs them
        const bool live = r.j < S;
        // straight line: the sinogram bin unconditionally at a clamped index, a lane past the detector contributes zero by select
        const float* __restrict__ sf = sinos + (long long)(r.k / S_per_fit) * sino_stride + (long long)r.t * S;
        const float d = (float)tot - sf[min(r.j, S - 1)];
        if (live) resid[((long long)r.k * T + r.t) * S + r.j] = grad_scale * 2.f * d / (float)((long long)T * S);      // as mse_grad_kernel (radon.hip)
        const double q = wave_sum_d(live ? (double)(d * d) : 0.0);
        if (threadIdx.x == 0) partials[(long long)r.k * T * strips + blockIdx.x] = q;
    }
}

// one block per fit: thread i adds partials i, i + 256, ... in index order, the 256 sums meet in block_sum_d's fixed order
__global__ __launch_bounds__(256) void radon_mse_finish_kernel(const double* __restrict__ partials, long long per_fit, double n_per, double* __restrict__ mse)
{
    __shared__ double s_red[8];
    const double* __restrict__ p = partials + (long long)blockIdx.x * per_fit;
    double t = 0;
    for (long long i = threadIdx.x; i < per_fit; i += 256) t += p[i];
    t = block_sum_d(t, s_red);
    if (threadIdx.x == 0) mse[blockIdx.x] += t / n_per;
}

bool shapes_ok(int n_fits, int S_per_fit, int S, int T)
{
    return n_fits >= 1 && S_per_fit >= 1 && (long long)n_fits * S_per_fit <= 65535 && S >= 1 && S <= 32768 && T >= 1 && T <= 32768;
}
inline long long partial_bytes(int n, int S, int T) { return (long long)n * T * ((S + 63) / 64) * (long long)sizeof(double); }

}  // namespace

extern "C" {

int64_t mfvi_radon_mse_fits_scratch_bytes(int n_fits, int S_per_fit, int S, int T)
{
    if (!shapes_ok(n_fits, S_per_fit, S, T)) return -1;
    const int n = n_fits * S_per_fit;
    return (int64_t)(partial_bytes(n, S, T) + (long long)n * T * S * (long long)sizeof(float));      // [partials fp64 | residual planes fp32]
}

int mfvi_radon_mse_fits(const float* out, const float* sinos, int64_t sino_stride, const float* theta_deg, int n_fits, int S_per_fit, int S, int T,
                        float grad_scale, void* scratch, float* dout, double* mse, void* stream)
{
    if (!out || !sinos || !theta_deg || !scratch || !mse) { set_error("radon_mse_fits: null tensor (only dout may be NULL)"); return -1; }
    if (!shapes_ok(n_fits, S_per_fit, S, T)) {
        set_error("radon_mse_fits: bad shape n_fits=%d S_per_fit=%d S=%d T=%d (1 <= n_fits * S_per_fit <= 65535 planes, 1 <= S, T <= 32768)", n_fits,
                  S_per_fit, S, T); return -1; }
    if (sino_stride < (int64_t)T * S) { set_error("radon_mse_fits: sino_stride=%lld below T * S = %lld", (long long)sino_stride, (long long)T * S); return -1; }
    if ((uintptr_t)scratch & 7) { set_error("radon_mse_fits: scratch must be 8-byte aligned (it starts with fp64 partial sums)"); return -1; }
    hipStream_t st = (hipStream_t)stream;
    const int n = n_fits * S_per_fit;
    const Split sp = project_split(n, S, T);                                         // the split of mfvi_radon_project for n planes
    double* partials = (double*)scratch;
    float* resid = (float*)((char*)scratch + partial_bytes(n, S, T));
    if (S >= 2)
        hipLaunchKernelGGL(radon_residual_kernel<true>, dim3((unsigned)(T * sp.strips), n), dim3(64 * sp.nw), 0, st, out, theta_deg, S, T, sp.strips,
                           sp.chunk, sinos, (long long)sino_stride, S_per_fit, grad_scale, resid, partials);
    else
        hipLaunchKernelGGL(radon_residual_kernel<false>, dim3((unsigned)(T * sp.strips), n), dim3(64 * sp.nw), 0, st, out, theta_deg, S, T, sp.strips,
                           sp.chunk, sinos, (long long)sino_stride, S_per_fit, grad_scale, resid, partials);
    hipLaunchKernelGGL(radon_mse_finish_kernel, dim3(n_fits), dim3(256), 0, st, (const double*)partials, (long long)S_per_fit * T * sp.strips,
                       (double)T * (double)S, mse);
    const int rc = (int)hipGetLastError(); if (rc) return rc;
    if (dout) return mfvi_radon_backproject(resid, theta_deg, n, S, T, dout, stream);
    return 0;
}

}  // extern "C"
