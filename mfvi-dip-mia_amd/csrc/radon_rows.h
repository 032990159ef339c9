// The row loop of the plane Radon projection, shared by radon_planes.hip (mfvi_radon_project: the ray sum is the output) and
// radon_fits.hip (mfvi_radon_mse_fits: the ray sum meets a residual epilogue), the way iter_ops.h serves fits.hip: one body, so both
// entry points form the same fp64 ray sums in the same order.  DESIGN.md sections 15 and 16.
#pragma once
#include "common.h"

namespace radon_rows {

constexpr float DEG2RAD = 0.017453292519943295f;      // torch.deg2rad in fp32 (radon/radon.py:31)
constexpr int MAX_WAVES = 16;                         // waves of a block (1024 threads)
constexpr int TARGET_WAVES = 8192;                    // 256 CUs x 32 waves: the split factor fills the chip from the shapes alone

// rows i with -1 < d + k (i - m) < S (the only rows whose bilinear footprint can meet the image along this coordinate), widened by a row
// on both sides and intersected into [lo, hi): a superset, the rows added contribute exactly zero
__device__ __forceinline__ void clip_rows(double d, double k, double m, int S, double& lo, double& hi)
{
    if (fabs(k) < 1e-9) {                              // the coordinate moves by < 1e-9 S over the rows: all of them or none
        if (!(d > -1.5 && d < (double)S + 0.5)) { lo = (double)S; hi = 0.0; }
        return;
    }
    const double u1 = (-1.0 - d) / k, u2 = ((double)S - d) / k;
    lo = fmax(lo, floor(fmin(u1, u2) + m));
    hi = fmin(hi, ceil(fmax(u1, u2) + m) + 1.0);
}

struct __attribute__((packed, aligned(4))) Pair { float a, b; };         // two neighbours of a row in one 8-byte load (dword-aligned)

// What a block's position means: angle t, strip of 64 bins, plane k, this lane's bin j
struct Ray { int t, strip, k, j; };

// The ray sums of one block (plane blockIdx.y, angle and strip from blockIdx.x): every wave sums its chunk of rows, the partial sums meet in
// `part` and wave 0 adds them in wave order.  Returns the sum of bin ray.j in the lanes of wave 0 (0 in the other waves).  A lane with
// j >= S walks the wave's rows too and returns a number that means nothing: the caller selects on ray.j < S.  Contains a __syncthreads:
// every thread of the block calls it.
// PAIR (S >= 2): the two x-neighbours of a sample come from one load at clamp(x0, 0, S - 2) and are told apart by selects
template <bool PAIR>
__device__ __forceinline__ double project_rows(const float* __restrict__ img, const float* __restrict__ theta, int S, int strips, int chunk,
                                               double (*part)[64], Ray& ray)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int t = blockIdx.x / strips, strip = blockIdx.x - t * strips, k = blockIdx.y;
    const int j = strip * 64 + lane;
    ray.t = t; ray.strip = strip; ray.k = k; ray.j = j;
    const float th = theta[t] * DEG2RAD;
    const double c = (double)cosf(th), s = (double)sinf(th), m = 0.5 * (double)(S - 1);
    const double a = c * ((double)j - m) + m, b = s * ((double)j - m) + m;          // the sample of row i = m
    double lo_d = 0.0, hi_d = (double)S;
    clip_rows(a, -s, m, S, lo_d, hi_d);
    clip_rows(b, c, m, S, lo_d, hi_d);
    int lo = (int)fmin(fmax(lo_d, 0.0), (double)S), hi = (int)fmin(fmax(hi_d, 0.0), (double)S);
    if (j >= S) { lo = S; hi = 0; }                                                  // lanes past the detector decide nothing
    for (int o = 32; o; o >>= 1) { lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); }
    lo = __builtin_amdgcn_readfirstlane(max(lo, wave * chunk));
    hi = __builtin_amdgcn_readfirstlane(min(hi, min(S, (wave + 1) * chunk)));
    const float* __restrict__ im = img + (long long)k * S * S;
    double ix = a - s * ((double)lo - m), iy = b + c * ((double)lo - m);
    double acc = 0;
#pragma unroll 4
    for (int i = lo; i < hi; ++i) {
        const double fx = floor(ix), fy = floor(iy);
        const int x0 = (int)fx, y0 = (int)fy;
        const float lx = (float)(ix - fx), ly = (float)(iy - fy);
        // straight line: unconditional loads at clamped indices, weights of out-of-image neighbours zeroed
        const float wx0 = (x0 >= 0 && x0 < S) ? 1.f - lx : 0.f, wx1 = (x0 >= -1 && x0 < S - 1) ? lx : 0.f;
        const float wy0 = (y0 >= 0 && y0 < S) ? 1.f - ly : 0.f, wy1 = (y0 >= -1 && y0 < S - 1) ? ly : 0.f;
        const int ra = min(max(y0, 0), S - 1) * S, rb = min(max(y0 + 1, 0), S - 1) * S;
        float v00, v01, v10, v11;
        if constexpr (PAIR) {
            const int xl = min(max(x0, 0), S - 2);                                   // x0 = -1 / S - 1: the valid neighbour is the other half
            const Pair pa = *reinterpret_cast<const Pair*>(im + ra + xl), pb = *reinterpret_cast<const Pair*>(im + rb + xl);
            v00 = x0 > xl ? pa.b : pa.a; v01 = x0 < xl ? pa.a : pa.b;
            v10 = x0 > xl ? pb.b : pb.a; v11 = x0 < xl ? pb.a : pb.b;
        } else {
            const int xa = min(max(x0, 0), S - 1), xb = min(max(x0 + 1, 0), S - 1);
            v00 = im[ra + xa]; v01 = im[ra + xb]; v10 = im[rb + xa]; v11 = im[rb + xb];
        }
        acc += (double)(wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11));
        ix -= s; iy += c;
    }
    part[wave][lane] = acc;
    __syncthreads();
    double tot = 0;
    if (wave == 0) {
        tot = part[0][lane];
        for (int w = 1; w < nw; ++w) tot += part[w][lane];
    }
    return tot;
}

// waves per block: the smallest power of two that brings `units` blocks to TARGET_WAVES waves, at most MAX_WAVES and at most `cap`
inline int split_factor(long long units, int cap)
{
    int nw = 1;
    while (nw < MAX_WAVES && nw * 2 <= cap && units * nw < TARGET_WAVES) nw *= 2;
    return nw;
}

// the launch shape of a projection of n planes: strips of 64 bins, waves per block (a wave keeps at least 8 rows), rows per wave
struct Split { int strips, nw, chunk; };
inline Split project_split(int n, int S, int T)
{
    Split sp;
    sp.strips = (S + 63) / 64;
    sp.nw = split_factor((long long)n * T * sp.strips, (S + 7) / 8);
    sp.chunk = (S + sp.nw - 1) / sp.nw;
    return sp;
}

}  // namespace radon_rows
