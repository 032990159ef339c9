// The per-iteration bookkeeping of the runner loop (bayesian_optimization.py:1374-1406, :2190-2236, :584-626) for MANY fits in one set of
// launches: the EMA / clip / ring-slot pass per fit (mfvi_bookkeep_fits, the per-pixel code of mfvi_bookkeep) and the
// squared-error and SSIM sums of n_pairs image pairs (mfvi_pair_metrics).  The SSIM of structural_similarity (utils/common_utils.py:308-351)
// is a separable 11-tap filter of five moment planes on an LDS tile; every sum is fp64 in a fixed order, with no floating-point atomics.
#include "common.h"
#include "iter_ops.h"
#include "../../include/mfvi_hip.h"

namespace {

// grid (pixels, fit): bookkeep_kernel's body (losses.hip) on fit blockIdx.y; the map buffers are [n_fits][HW]
__global__ __launch_bounds__(256) void bookkeep_fits_kernel(const float* __restrict__ out, int S, int C, long long HW, float* __restrict__ ema, float w, int first,
                                                            float* __restrict__ out_clip, float* __restrict__ avg_clip, float* __restrict__ ale_clip,
                                                            float* __restrict__ ring_epi, float* __restrict__ ring_ale)
{
    const float* __restrict__ o = out + (long long)blockIdx.y * S * C * HW;
    float* __restrict__ e = ema + (long long)blockIdx.y * C * HW;
    const long long off = (long long)blockIdx.y * HW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < HW; i += (long long)gridDim.x * 256) {
        float m, a;
        const float e0 = sample_means_ema(o, S, C, HW, i, e, w, first, m, a);
        const float mc = fminf(fmaxf(m, 0.f), 1.f), ac = fminf(fmaxf(a, 0.f), 1.f);
        out_clip[off + i] = mc; avg_clip[off + i] = fminf(fmaxf(e0, 0.f), 1.f);
        if (ring_epi) ring_epi[off + i] = mc;
        if (C > 1) { ale_clip[off + i] = ac; if (ring_ale) ring_ale[off + i] = ac; }
    }
}

// ---- pair metrics -------------------------------------------------------------------------------------------------------------------
// One block owns a TH x TW tile of one pair.  LDS:
//   s_in[2][IH][IP]   x and y with the 5-pixel halo, zeros outside the image (the zero padding of the reference's conv2d)
//   s_h [5][IH][HP]   the horizontally filtered moment planes x, y, x^2, y^2, xy
// Row pitches (bank rules of ds_read_b128 / ds_write_b128 / ds_read_b32 on gfx950):
//   * the horizontal pass reads 14 consecutive floats per lane as three ds_read_b128 and a ds_read_b64 (bank = dword % 64, conflicts inside the 16-lane groups
//     {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same + 32).  h_lane() deals the 16 column groups of ONE row to each of those lane groups,
//     so a group's 16 addresses are 16 consecutive 16-byte slots of one row = 64 distinct banks whatever the pitch; IP only has to keep the
//     rows 16-byte aligned and hold column 4 * 15 + 15: IP = 76.
//   * its ds_write_b128 (bank = dword % 32, groups of 8 consecutive lanes) then has lanes 0-3 on one row and lanes 4-7 on the next with the
//     same columns 0-15: HP = 80 = 16 (mod 32) puts the second row's 16 dwords on the other half of the banks.
//   * the vertical pass (ds_read2_b32 of two rows) and the staging stores (ds_write_b32) have consecutive lanes on consecutive dwords.
constexpr int TH = 16, TW = 64, HALO = 5, IH = TH + 2 * HALO, IW = TW + 2 * HALO, IP = 76, HP = 80;
constexpr int STAGE_ITERS = (IH * IW + 255) / 256;
static_assert(IP % 4 == 0 && IP >= TW + 12 && HP % 4 == 0 && HP >= TW, "LDS row pitches");
static_assert((2 * IH * IP + 5 * IH * HP) * 4 + 64 <= 64 * 1024, "static LDS within 64 KB: two blocks per CU");

struct PairWin { float g[11]; };

// lane -> (row within the wave's four rows, column group 0..15) of the horizontal pass: each ds_read_b128 lane group gets one row
__device__ __forceinline__ void h_lane(int lane, int& row, int& g)
{
    const int l5 = lane & 31;
    const bool a = l5 < 4 || (l5 >= 12 && l5 < 16) || (l5 >= 20 && l5 < 28);
    g = a ? (l5 < 4 ? l5 : (l5 < 16 ? l5 - 8 : l5 - 12)) : (l5 < 12 ? l5 - 4 : (l5 < 20 ? l5 - 8 : l5 - 16));
    row = (lane >> 5) * 2 + (a ? 0 : 1);
}

template <bool SSIM>
__global__ __launch_bounds__(256) void pair_metrics_kernel(const float* __restrict__ x, long long x_stride, const float* __restrict__ y, long long y_stride,
                                                           int H, int W, int tiles_x, PairWin win, double* __restrict__ partial)
{
    __shared__ double s_red[8];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int r0 = ty * TH, c0 = tx * TW;
    const float* __restrict__ xp = x + (long long)blockIdx.y * x_stride;
    const float* __restrict__ yp = y + (long long)blockIdx.y * y_stride;
    // this thread's output pixels: column c0 + (tid & 63), rows r0 + 4 * (tid >> 6) + 0..3
    const int oc = tid & 63, orow = (tid >> 6) * 4;
    double acc_sq = 0, acc_ss = 0;

    if constexpr (!SSIM) {
        // the same pixels in the same order as the SSIM variant, so slot 0 does not depend on want_ssim.  Clamped address + select: no
        // branch around a load, and no address outside the image
        float d[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = r0 + orow + k, c = c0 + oc;
            const long long p = (long long)min(r, H - 1) * W + min(c, W - 1);
            const float dv = xp[p] - yp[p];
            d[k] = (r < H && c < W) ? dv : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) acc_sq += (double)(d[k] * d[k]);
    } else {
        __shared__ __align__(16) float s_in[2][IH][IP];
        __shared__ __align__(16) float s_h[5][IH][HP];
        // ---- stage x and y with the halo: STAGE_ITERS straight-line rounds of clamped loads, out-of-image positions become 0 without a read
        // of their own (the clamped address is inside the image)
        float vx[STAGE_ITERS], vy[STAGE_ITERS];
#pragma unroll
        for (int it = 0; it < STAGE_ITERS; ++it) {
            const int e = min(it * 256 + tid, IH * IW - 1);
            const int j = e / IW, i = e - j * IW;
            const int r = r0 - HALO + j, c = c0 - HALO + i;
            const bool in = r >= 0 && r < H && c >= 0 && c < W;
            const long long p = (long long)min(max(r, 0), H - 1) * W + min(max(c, 0), W - 1);
            const float a = xp[p], b = yp[p];
            vx[it] = in ? a : 0.f; vy[it] = in ? b : 0.f;
        }
#pragma unroll
        for (int it = 0; it < STAGE_ITERS; ++it) {      // the clamped tail of the last round rewrites element IH * IW - 1 with its own value
            const int e = min(it * 256 + tid, IH * IW - 1);
            const int j = e / IW, i = e - j * IW;
            s_in[0][j][i] = vx[it]; s_in[1][j][i] = vy[it];
        }
        __syncthreads();
        // ---- horizontal pass: a work item is 4 consecutive columns of one staged row; a wave takes 4 rows per round
        int hrow, hg; h_lane(tid & 63, hrow, hg);
#pragma unroll
        for (int rnd = 0; rnd < (IH + 15) / 16; ++rnd) {
            const int j = (rnd * 4 + (tid >> 6)) * 4 + hrow;
            if (j < IH) {
                float a[16], b[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 av = *reinterpret_cast<const float4*>(&s_in[0][j][4 * hg + 4 * q]);
                    const float4 bv = *reinterpret_cast<const float4*>(&s_in[1][j][4 * hg + 4 * q]);
                    a[4 * q] = av.x; a[4 * q + 1] = av.y; a[4 * q + 2] = av.z; a[4 * q + 3] = av.w;
                    b[4 * q] = bv.x; b[4 * q + 1] = bv.y; b[4 * q + 2] = bv.z; b[4 * q + 3] = bv.w;
                }
                // the values are final in their registers: without this the SLP vectoriser re-reads the row from LDS as unaligned pairs
                // (ds_read2_b32 at a lane stride of 4 dwords: 4-way bank conflicts) to feed packed multiplies
#pragma unroll
                for (int c = 0; c < 14; ++c) { asm volatile("" : "+v"(a[c])); asm volatile("" : "+v"(b[c])); }
                float h[5][4];
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    float m1 = 0, m2 = 0, s11 = 0, s22 = 0, s12 = 0;
#pragma unroll
                    for (int k = 0; k < 11; ++k) {      // columns 14 and 15 of the 16 read are never used
                        const float wv = win.g[k], p = a[o + k], q = b[o + k];
                        m1 += wv * p; m2 += wv * q; s11 += wv * (p * p); s22 += wv * (q * q); s12 += wv * (p * q);
                    }
                    h[0][o] = m1; h[1][o] = m2; h[2][o] = s11; h[3][o] = s22; h[4][o] = s12;
                }
#pragma unroll
                for (int pl = 0; pl < 5; ++pl)
                    *reinterpret_cast<float4*>(&s_h[pl][j][4 * hg]) = make_float4(h[pl][0], h[pl][1], h[pl][2], h[pl][3]);
            }
        }
        __syncthreads();
        // ---- vertical pass: 4 vertically consecutive outputs per thread from 14 rows of the five planes
        float v[5][4];
#pragma unroll
        for (int pl = 0; pl < 5; ++pl)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[pl][k] = 0.f;
#pragma unroll
        for (int jj = 0; jj < 14; ++jj) {
            float t[5];
#pragma unroll
            for (int pl = 0; pl < 5; ++pl) t[pl] = s_h[pl][orow + jj][oc];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (jj - k >= 0 && jj - k < 11) {       // compile-time after unrolling: output k takes rows k .. k + 10 in ascending order
                    const float wv = win.g[jj - k];
#pragma unroll
                    for (int pl = 0; pl < 5; ++pl) v[pl][k] += wv * t[pl];
                }
            }
        }
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float m1 = v[0][k], m2 = v[1][k];
            const float v1 = v[2][k] - m1 * m1, v2 = v[3][k] - m2 * m2, v12 = v[4][k] - m1 * m2;
            const float ss = ((2.f * m1 * m2 + C1) * (2.f * v12 + C2)) / ((m1 * m1 + m2 * m2 + C1) * (v1 + v2 + C2));
            const float dv = s_in[0][orow + k + HALO][oc + HALO] - s_in[1][orow + k + HALO][oc + HALO];
            if (r0 + orow + k < H && c0 + oc < W) { acc_sq += (double)(dv * dv); acc_ss += (double)ss; }
        }
    }
    const double bsq = block_sum_d(acc_sq, s_red);
    double* __restrict__ slot = partial + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    if (SSIM) {
        const double bss = block_sum_d(acc_ss, s_red);
        if (tid == 0) slot[1] = bss;
    }
    if (tid == 0) slot[0] = bsq;
}

// one block per pair: thread i adds the tile partials i, i + 256, ... in index order, the 256 sums meet in block_sum_d's fixed order
__global__ __launch_bounds__(256) void pair_metrics_finish_kernel(const double* __restrict__ partial, int n_tiles, int want_ssim, double* __restrict__ sums,
                                                                  long long sums_stride)
{
    __shared__ double s_red[8];
    const double* __restrict__ p = partial + (long long)blockIdx.x * n_tiles * 2;
    double a = 0, b = 0;
    for (int t = threadIdx.x; t < n_tiles; t += 256) { a += p[2 * t]; if (want_ssim) b += p[2 * t + 1]; }
    a = block_sum_d(a, s_red);
    b = block_sum_d(b, s_red);
    if (threadIdx.x == 0) {
        sums[(long long)blockIdx.x * sums_stride] = a;
        if (want_ssim) sums[(long long)blockIdx.x * sums_stride + 1] = b;
    }
}

inline long long n_tiles_of(int H, int W) { return (long long)((H + TH - 1) / TH) * ((W + TW - 1) / TW); }

}  // namespace

extern "C" {

int mfvi_bookkeep_fits(const float* out, int n_fits, int S, int C, int H, int W, float* ema, float weight, int first, float* out_clip, float* avg_clip,
                       float* ale_clip, float* ring_epi, float* ring_ale, void* stream)
{
    if (!out || !ema || !out_clip || !avg_clip || (C > 1 && !ale_clip) || n_fits < 1 || n_fits > 65535 || S < 1 || C < 1 || C > 2 || H < 1 || W < 1) {
        set_error("bookkeep_fits: bad arguments (n_fits=%d S=%d C=%d H=%d W=%d; ale_clip is required for C = 2)", n_fits, S, C, H, W); return -1; }
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(bookkeep_fits_kernel, dim3(nblocks(HW, 256), n_fits), dim3(256), 0, (hipStream_t)stream, out, S, C, HW, ema, weight, first, out_clip,
                       avg_clip, ale_clip, ring_epi, ring_ale);
    return (int)hipGetLastError();
}

size_t mfvi_pair_metrics_scratch_bytes(int n_pairs, int H, int W)
{
    if (n_pairs < 1 || n_pairs > 65535 || H < 1 || W < 1) return 0;
    return (size_t)n_pairs * (size_t)n_tiles_of(H, W) * 2 * sizeof(double);
}

int mfvi_pair_metrics(const float* x, int64_t x_stride, const float* y, int64_t y_stride, int n_pairs, int H, int W, int want_ssim, void* scratch,
                      double* sums, int64_t sums_stride, void* stream)
{
    const long long HW = (long long)H * W;
    if (!x || !y || !sums || !scratch || n_pairs < 1 || n_pairs > 65535 || H < 1 || W < 1 || (x_stride != 0 && x_stride < HW) ||
        (y_stride != 0 && y_stride < HW) || sums_stride < (want_ssim ? 2 : 1) || n_tiles_of(H, W) > 0x7fffffffLL) {
        set_error("pair_metrics: bad arguments (n_pairs=%d in 1..65535, H=%d W=%d, x_stride=%lld y_stride=%lld 0 or >= H W, sums_stride=%lld, scratch of "
                  "mfvi_pair_metrics_scratch_bytes(n_pairs, H, W) bytes)", n_pairs, H, W, (long long)x_stride, (long long)y_stride, (long long)sums_stride);
        return -1; }
    const int tiles_x = (W + TW - 1) / TW, n_tiles = (int)n_tiles_of(H, W);
    hipStream_t st = (hipStream_t)stream;
    if (want_ssim) {
        PairWin win; float s = 0.f;      // as mfvi_ssim_sum builds its window
        for (int i = 0; i < 11; ++i) { win.g[i] = expf(-(float)((i - 5) * (i - 5)) / (2.f * 1.5f * 1.5f)); s += win.g[i]; }
        for (int i = 0; i < 11; ++i) win.g[i] /= s;
        hipLaunchKernelGGL(pair_metrics_kernel<true>, dim3(n_tiles, n_pairs), dim3(256), 0, st, x, (long long)x_stride, y, (long long)y_stride, H, W, tiles_x,
                           win, (double*)scratch);
    } else {
        PairWin win = {};
        hipLaunchKernelGGL(pair_metrics_kernel<false>, dim3(n_tiles, n_pairs), dim3(256), 0, st, x, (long long)x_stride, y, (long long)y_stride, H, W, tiles_x,
                           win, (double*)scratch);
    }
    hipLaunchKernelGGL(pair_metrics_finish_kernel, dim3(n_pairs), dim3(256), 0, st, (const double*)scratch, n_tiles, want_ssim ? 1 : 0, sums,
                       (long long)sums_stride);
    return (int)hipGetLastError();
}

}  // extern "C"
