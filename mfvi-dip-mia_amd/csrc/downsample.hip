// Anti-aliased super-resolution data term: the Lanczos downsampler of models/downsampler.py:6-136 (half phase, preserve_size) as a
// separable banded operator per plane, lr = A_H . hr . A_W^T with A[y][clamp(y*f + i - P, 0, N-1)] += k1[i], P = (T - f) / 2 the
// ReplicationPad2d width, its adjoint as a gather, and gaussian_nll (utils/bayesian_utils.py:29-32) of the
// projected output as bayesian_optimization.py:2182-2185 forms it.
#include "common.h"
#include "iter_ops.h"
#include <algorithm>
#include "../../include/mfvi_hip.h"

namespace {

constexpr int DS_MAX_TAPS = 48;
constexpr int DS_CORE_H = 32, DS_CORE_W = 64;      // high-resolution core of one tile: (32 / f) x (64 / f) low-resolution pixels

// the 1-D taps by value (as SsimWin travels): k, and for the two border pixels of a line the folded weights of the replication pad:
// pre[j] = sum_{i < j} k[i] (every tap that clamps to pixel 0), suf[j] = sum_{i >= j} k[i] (pixel N - 1); summed in fp64 on the host
struct DsTaps { float k[DS_MAX_TAPS]; float pre[DS_MAX_TAPS + 1]; float suf[DS_MAX_TAPS + 1]; };

// f is 2, 4 or 8 (lf = log2 f): divisions by f are arithmetic shifts, which floor for negative numerators too
__device__ __forceinline__ int ceil_div(int a, int f, int lf) { return (a + f - 1) >> lf; }

// The TY x TX low-resolution pixels from (ty0, tx0) of ONE plane -> s_lr[yy * TX + xx].  The tile with its halo ((TY-1) f + T rows,
// (TX-1) f + T columns) is staged once, every load unconditional with a clamped index (which IS the replication pad), eight loads of a
// thread requested before the first is stored; row pass into s_tmp (transposed), column pass into s_lr.  Odd LDS pitches: the row pass
// walks the tile's rows across lanes, the column pass the columns of s_tmp.  Pixels of a partial tile beyond the map are computed from
// clamped (valid) loads and never stored by the caller.
__device__ __forceinline__ void ds_filter_tile(const float* __restrict__ src, int H, int W, int f, int lf, int T, int ty0, int tx0, int TY, int TX,
                                               const float* s_k, float* s_tile, float* s_tmp, float* s_lr)
{
    constexpr int U = 8;
    const int P = (T - f) / 2, ltx = 6 - lf;      // TX = 64 / f
    const int rows = (TY - 1) * f + T, cols = (TX - 1) * f + T, pitch = cols | 1, tp = rows | 1;
    const int y0 = ty0 * f - P, x0 = tx0 * f - P;
    const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
    for (int c0 = 0; c0 < cols; c0 += 64) {
        const int c = c0 + lx, gx = min(max(x0 + c, 0), W - 1);
        for (int r0 = ly; r0 < rows; r0 += 4 * U) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = src[(long long)min(max(y0 + r0 + 4 * u, 0), H - 1) * W + gx];
#pragma unroll
            for (int u = 0; u < U; ++u) if (r0 + 4 * u < rows && c < cols) s_tile[(r0 + 4 * u) * pitch + c] = v[u];
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < rows * TX; j += 256) {
        const int x = j / rows, r = j - x * rows;
        const float* p = s_tile + r * pitch + x * f;
        float a = 0.f;
        for (int i = 0; i < T; ++i) a = fmaf(s_k[i], p[i], a);
        s_tmp[x * tp + r] = a;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < TY * TX; j += 256) {
        const int y = j >> ltx, x = j & (TX - 1);
        const float* p = s_tmp + x * tp + y * f;
        float a = 0.f;
        for (int i = 0; i < T; ++i) a = fmaf(s_k[i], p[i], a);
        s_lr[j] = a;
    }
    __syncthreads();
}

// dynamic LDS of the two forward kernels: [taps 48][lr 2 * TY * TX][tmp TX * (rows | 1)][tile rows * (cols | 1)]
inline size_t ds_forward_lds(int f, int T)
{
    const int TY = DS_CORE_H / f, TX = DS_CORE_W / f, rows = (TY - 1) * f + T, cols = (TX - 1) * f + T;
    return sizeof(float) * (size_t)(DS_MAX_TAPS + 2 * TY * TX + TX * (rows | 1) + rows * (cols | 1));
}

// grid (tiles, C, n): plane = sample * C + channel
__global__ __launch_bounds__(256) void downsample_kernel(const float* __restrict__ src, int H, int W, int f, int lf, int T, DsTaps taps, float* __restrict__ dst)
{
    extern __shared__ float ds_smem[];
    const int h = H / f, w = W / f, TY = DS_CORE_H / f, TX = DS_CORE_W / f, rows = (TY - 1) * f + T;
    float* s_k = ds_smem; float* s_lr = s_k + DS_MAX_TAPS; float* s_tmp = s_lr + 2 * TY * TX; float* s_tile = s_tmp + TX * (rows | 1);
    if ((int)threadIdx.x < T) s_k[threadIdx.x] = taps.k[threadIdx.x];
    const int tiles_x = (w + TX - 1) / TX;
    const int ty0 = ((int)blockIdx.x / tiles_x) * TY, tx0 = ((int)blockIdx.x % tiles_x) * TX;
    const long long plane = (long long)blockIdx.z * gridDim.y + blockIdx.y;
    ds_filter_tile(src + plane * H * W, H, W, f, lf, T, ty0, tx0, TY, TX, s_k, s_tile, s_tmp, s_lr);
    float* __restrict__ d = dst + plane * h * w;
    for (int j = threadIdx.x; j < TY * TX; j += 256) {
        const int y = ty0 + (j >> (6 - lf)), x = tx0 + (j & (TX - 1));
        if (y < h && x < w) d[(long long)y * w + x] = s_lr[j];
    }
}

// grid (blocks per sample, n): a block walks tiles b, b + gridDim.x, ... of its sample — both channels of a tile, then the NLL and the
// low-resolution gradient glr[n][2][h][w] (already times grad_scale / (h w)) of its pixels; one fp64 atomic per block (as gaussian_nll_kernel)
__global__ __launch_bounds__(256) void gnll_filtered_kernel(const float* __restrict__ out, const float* __restrict__ target, int H, int W, int f, int lf, int T,
                                                            DsTaps taps, float grad_scale, float* __restrict__ glr, double* __restrict__ nll_sum)
{
    extern __shared__ float ds_smem[];
    __shared__ double s_red[8];
    const int h = H / f, w = W / f, TY = DS_CORE_H / f, TX = DS_CORE_W / f, rows = (TY - 1) * f + T;
    float* s_k = ds_smem; float* s_lr = s_k + DS_MAX_TAPS; float* s_tmp = s_lr + 2 * TY * TX; float* s_tile = s_tmp + TX * (rows | 1);
    if ((int)threadIdx.x < T) s_k[threadIdx.x] = taps.k[threadIdx.x];
    const int tiles_x = (w + TX - 1) / TX, tiles = tiles_x * ((h + TY - 1) / TY);
    const long long HW = (long long)H * W, hw = (long long)h * w;
    const float* __restrict__ o = out + (long long)blockIdx.y * 2 * HW;
    float* __restrict__ g = glr ? glr + (long long)blockIdx.y * 2 * hw : nullptr;
    const float nf = (float)hw;
    double acc = 0;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int ty0 = (t / tiles_x) * TY, tx0 = (t % tiles_x) * TX;
        ds_filter_tile(o, H, W, f, lf, T, ty0, tx0, TY, TX, s_k, s_tile, s_tmp, s_lr);
        ds_filter_tile(o + HW, H, W, f, lf, T, ty0, tx0, TY, TX, s_k, s_tile, s_tmp, s_lr + TY * TX);
        for (int j = threadIdx.x; j < TY * TX; j += 256) {
            const int y = ty0 + (j >> (6 - lf)), x = tx0 + (j & (TX - 1));
            if (y >= h || x >= w) continue;
            const long long p = (long long)y * w + x;
            const float m = s_lr[j], sraw = s_lr[TY * TX + j];
            const float s = fminf(fmaxf(sraw, -20.f), 20.f);
            const bool inside = (sraw >= -20.f) && (sraw <= 20.f);
            const float df = target[p] - m, e = expf(s);
            acc += (double)(e * df * df - s);
            if (g) {
                g[p] = grad_scale * (-2.f * e * df) / nf;
                g[hw + p] = inside ? grad_scale * (e * df * df - 1.f) / nf : 0.f;
            }
        }      // (the next tile's column pass writes s_lr two barriers further on)
    }
    block_atomic_add(acc / (double)hw, nll_sum, s_red);
}

// dsrc = A_H^T . g . A_W as a GATHER, grid (tiles of 32 x 64 high-resolution pixels, C, n): the low-resolution gradients that reach the
// tile are staged (rows ylo..yhi, columns xlo..xhi; at most LY x LX), pass 1 folds the columns (s_t[yy][X]), pass 2 the rows.  A pixel
// inside a line takes tap i = X + P - x f of low-resolution pixel x; pixels 0 and N - 1 take the folded weights of the replication pad.
// No atomics, one fixed summation order per pixel: bit-identical from call to call.
__global__ __launch_bounds__(256) void downsample_adjoint_kernel(const float* __restrict__ g, int H, int W, int f, int lf, int T, DsTaps taps, int LY, int LX,
                                                                 float* __restrict__ dsrc)
{
    extern __shared__ float ds_smem[];
    const int h = H / f, w = W / f, P = (T - f) / 2;
    float* s_k = ds_smem; float* s_pre = s_k + DS_MAX_TAPS; float* s_suf = s_pre + DS_MAX_TAPS + 1;
    float* s_g = s_suf + DS_MAX_TAPS + 1; float* s_t = s_g + LY * LX;
    for (int i = threadIdx.x; i <= T; i += 256) { if (i < T) s_k[i] = taps.k[i]; s_pre[i] = taps.pre[i]; s_suf[i] = taps.suf[i]; }
    const int tiles_x = (W + DS_CORE_W - 1) / DS_CORE_W;
    const int Y0 = ((int)blockIdx.x / tiles_x) * DS_CORE_H, X0 = ((int)blockIdx.x % tiles_x) * DS_CORE_W;
    const int Y1 = min(Y0 + DS_CORE_H - 1, H - 1), X1 = min(X0 + DS_CORE_W - 1, W - 1);
    const long long plane = (long long)blockIdx.z * gridDim.y + blockIdx.y;
    const int ylo = max(0, ceil_div(Y0 + P - T + 1, f, lf)), yhi = min(h - 1, (Y1 + P) >> lf), ny = min(yhi - ylo + 1, LY);
    const int xlo = max(0, ceil_div(X0 + P - T + 1, f, lf)), xhi = min(w - 1, (X1 + P) >> lf), nx = min(xhi - xlo + 1, LX);
    const float* __restrict__ gp = g + plane * h * w;
    for (int j = threadIdx.x; j < ny * nx; j += 256) {
        const int yy = j / nx, xx = j - yy * nx;
        s_g[yy * LX + xx] = gp[(long long)(ylo + yy) * w + xlo + xx];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < ny * DS_CORE_W; j += 256) {
        const int Xl = j & (DS_CORE_W - 1), yy = j >> 6, X = min(X0 + Xl, W - 1);
        const int xa = max(xlo, ceil_div(X + P - T + 1, f, lf)), xb = min(xlo + nx - 1, (X + P) >> lf);
        const float* wt = X == 0 ? s_pre + 1 : (X == W - 1 ? s_suf : s_k);
        float a = 0.f;
        for (int x = xa; x <= xb; ++x) a = fmaf(wt[X + P - x * f], s_g[yy * LX + x - xlo], a);
        s_t[j] = a;
    }
    __syncthreads();
    float* __restrict__ d = dsrc + plane * H * W;
    for (int j = threadIdx.x; j < DS_CORE_H * DS_CORE_W; j += 256) {
        const int Xl = j & (DS_CORE_W - 1), Y = Y0 + (j >> 6), X = X0 + Xl;
        if (Y >= H || X >= W) continue;
        const int ya = max(ylo, ceil_div(Y + P - T + 1, f, lf)), yb = min(ylo + ny - 1, (Y + P) >> lf);
        const float* wt = Y == 0 ? s_pre + 1 : (Y == H - 1 ? s_suf : s_k);
        float a = 0.f;
        for (int y = ya; y <= yb; ++y) a = fmaf(wt[Y + P - y * f], s_t[(y - ylo) * DS_CORE_W + Xl], a);
        d[(long long)Y * W + X] = a;
    }
}

inline int ds_log2(int f) { return f == 2 ? 1 : (f == 4 ? 2 : 3); }

// shape / tap checks shared by the three entry points; fills the by-value tap block
int ds_prepare(const char* who, int n, int C, int H, int W, int factor, const float* taps, int n_taps, DsTaps& t)
{
    if (n < 1 || n > 65535 || C < 1 || C > 65535 || (factor != 2 && factor != 4 && factor != 8) || H < factor || W < factor || H % factor || W % factor) {
        set_error("%s: bad shape n=%d C=%d H=%d W=%d factor=%d (factor 2, 4 or 8 dividing H and W; n, C <= 65535)", who, n, C, H, W, factor); return -1; }
    if (!taps || n_taps < factor || n_taps > DS_MAX_TAPS || ((n_taps - factor) & 1)) {
        set_error("%s: bad taps (n_taps=%d: factor <= n_taps <= %d, n_taps - factor even)", who, n_taps, DS_MAX_TAPS); return -1; }
    double run = 0;
    for (int i = 0; i < DS_MAX_TAPS; ++i) t.k[i] = i < n_taps ? taps[i] : 0.f;
    for (int i = 0; i <= DS_MAX_TAPS; ++i) { t.pre[i] = (float)run; if (i < n_taps) run += (double)taps[i]; }
    run = 0;
    for (int i = DS_MAX_TAPS; i >= 0; --i) { if (i < n_taps) run += (double)taps[i]; t.suf[i] = (float)run; }
    return 0;
}

int launch_adjoint(const float* ddst, int n, int C, int H, int W, int f, int T, const DsTaps& t, float* dsrc, hipStream_t st)
{
    // at most floor((core - 1 + T - 1) / f) + 1 low-resolution lines reach the core's lines
    const int LY = (DS_CORE_H + T - 2) / f + 1, LX = (DS_CORE_W + T - 2) / f + 1;
    const size_t lds = sizeof(float) * (size_t)(DS_MAX_TAPS + 2 * (DS_MAX_TAPS + 1) + LY * LX + LY * DS_CORE_W);
    const int tiles = ((H + DS_CORE_H - 1) / DS_CORE_H) * ((W + DS_CORE_W - 1) / DS_CORE_W);
    hipLaunchKernelGGL(downsample_adjoint_kernel, dim3(tiles, C, n), dim3(256), lds, st, ddst, H, W, f, ds_log2(f), T, t, LY, LX, dsrc);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int mfvi_downsample(const float* src, int n, int C, int H, int W, int factor, const float* taps, int n_taps, float* dst, void* stream)
{
    DsTaps t;
    if (!src || !dst) { set_error("downsample: null tensor"); return -1; }
    if (int rc = ds_prepare("downsample", n, C, H, W, factor, taps, n_taps, t)) return rc;
    const int TY = DS_CORE_H / factor, TX = DS_CORE_W / factor, h = H / factor, w = W / factor;
    const int tiles = ((h + TY - 1) / TY) * ((w + TX - 1) / TX);
    hipLaunchKernelGGL(downsample_kernel, dim3(tiles, C, n), dim3(256), ds_forward_lds(factor, n_taps), (hipStream_t)stream, src, H, W, factor, ds_log2(factor), n_taps, t, dst);
    return (int)hipGetLastError();
}

int mfvi_downsample_adjoint(const float* ddst, int n, int C, int H, int W, int factor, const float* taps, int n_taps, float* dsrc, void* stream)
{
    DsTaps t;
    if (!ddst || !dsrc) { set_error("downsample_adjoint: null tensor"); return -1; }
    if (int rc = ds_prepare("downsample_adjoint", n, C, H, W, factor, taps, n_taps, t)) return rc;
    return launch_adjoint(ddst, n, C, H, W, factor, n_taps, t, dsrc, (hipStream_t)stream);
}

int mfvi_gaussian_nll_filtered(const float* out, const float* target, int n, int H, int W, int factor, const float* taps, int n_taps, float grad_scale,
                               float* scratch, float* dout, double* nll_sum, void* stream)
{
    DsTaps t;
    hipStream_t st = (hipStream_t)stream;
    if (!out || !target || !nll_sum || (dout && !scratch)) { set_error("gaussian_nll_filtered: null tensor (dout needs scratch)"); return -1; }
    if (int rc = ds_prepare("gaussian_nll_filtered", n, 2, H, W, factor, taps, n_taps, t)) return rc;
    const int TY = DS_CORE_H / factor, TX = DS_CORE_W / factor, h = H / factor, w = W / factor;
    const int tiles = ((h + TY - 1) / TY) * ((w + TX - 1) / TX);
    // every block ends in one fp64 atomic on the same address (losses.hip): a block takes several tiles once the launch fills the chip
    const int per_sample = std::min(tiles, std::max(16, 1024 / n));
    hipLaunchKernelGGL(gnll_filtered_kernel, dim3(per_sample, n), dim3(256), ds_forward_lds(factor, n_taps), st, out, target, H, W, factor, ds_log2(factor), n_taps, t,
                       grad_scale, dout ? scratch : nullptr, nll_sum);
    if (hipError_t e = hipGetLastError()) return (int)e;
    return dout ? launch_adjoint(scratch, n, 2, H, W, factor, n_taps, t, dout, st) : 0;
}

}  // extern "C"
