// Total-variation regulariser (utils/sr_utils.py:84-94 tv_loss): value and gradient of
//     TV_beta(x) = sum over the cells (i < H-1, j < W-1) of u^beta,   u = dh^2 + dw^2,   dh = x[i][j+1] - x[i][j],   dw = x[i+1][j] - x[i][j]
// for one channel of n_fits * S samples.  The gradient of a pixel is a GATHER over the three cells it touches, always in the order
//     cell (i, j):    g (-dh - dw)       cell (i, j-1):    g dh       cell (i-1, j):    g dw           g = 2 beta u^(beta - 1)
// so it needs no atomics and is bit-identical from call to call.  g = 0 where u == 0 and beta < 1 (the reference's autograd returns
// inf * 0 = NaN there; the value is unaffected).  The value goes through one fp64 partial per block and a second launch with one block
// per fit that adds the partials in index order: no floating-point atomics.
//
// One block owns a 16 x 64 tile of one plane; a lane owns four consecutive pixels of a row and reads the 3 x 6 neighbourhood (row
// above, own row, row below; one column left, one right) through the cache -- the rows of a wave are four 256-byte runs.  Borders are
// clamped addresses plus selects: there is no branch around a load, and no address leaves the plane, so a NaN stays in its fit.
#include <cmath>
#include "common.h"
#include "../../include/mfvi_hip.h"

namespace {

constexpr int TH = 16, TW = 64;
enum { BETA_HALF = 0, BETA_ONE = 1, BETA_ANY = 2 };

// u -> (u^beta, 2 beta u^(beta - 1)), with g = 0 at u == 0 for beta < 1
template <int MODE>
__device__ __forceinline__ void cell_terms(float u, float beta, float& val, float& g)
{
    if constexpr (MODE == BETA_HALF) {
        const float r = rsqrtf(u);
        g = u == 0.f ? 0.f : r;                          // 2 * 0.5 * u^(-1/2)
        val = sqrtf(u);
    } else if constexpr (MODE == BETA_ONE) {
        g = 2.f; val = u;
    } else {
        const float p = 2.f * beta * powf(u, beta - 1.f);
        g = (u == 0.f && beta < 1.f) ? 0.f : p;
        val = powf(u, beta);
    }
}

// columns c - 1 .. c + 4 of one row into v[0..5]; every address is inside the row
template <bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ row, int c, int W, float v[6])
{
    if constexpr (VEC) {      // W % 4 == 0, c % 4 == 0, c <= W - 4, 16-byte aligned rows
        const float4 q = *reinterpret_cast<const float4*>(row + c);
        v[1] = q.x; v[2] = q.y; v[3] = q.z; v[4] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k + 1] = row[min(c + k, W - 1)];
    }
    v[0] = row[max(c - 1, 0)];
    v[5] = row[min(c + 4, W - 1)];
}

// grid (tiles of a plane, plane); plane p = sample p of `out`, fit p / S
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void tv_term_kernel(const float* __restrict__ out, int S, int C, int H, int W, int channel, int tiles_x, float beta,
                                                      const float* __restrict__ weight, int weight_stride, float grad_scale, int accumulate,
                                                      float* __restrict__ dout, double* __restrict__ partial)
{
    __shared__ double s_red[8];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int r = ty * TH + (tid >> 4);                 // this lane's row, and the first of its four columns
    const int c = tx * TW + (tid & 15) * 4;
    const long long plane = ((long long)blockIdx.y * C + channel) * H * W;
    const float* __restrict__ x = out + plane;
    const int cl = VEC ? min(c, W - 4) : c;             // VEC: a lane past the row reads the row's last quad (and is masked below)
    const int rz = min(r, H - 1);
    float m[6], z[6], p[6];
    load_row<VEC>(x + (long long)max(rz - 1, 0) * W, cl, W, m);
    load_row<VEC>(x + (long long)rz * W, cl, W, z);
    load_row<VEC>(x + (long long)min(rz + 1, H - 1) * W, cl, W, p);

    // cells of row r at columns c - 1 .. c + 3 (index q = column - c + 1) and of row r - 1 at columns c .. c + 3
    float g0[5], dh0[5], dw0[5], v0[5], g1[4], dw1[4];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        dh0[q] = z[q + 1] - z[q]; dw0[q] = p[q] - z[q];
        cell_terms<MODE>(dh0[q] * dh0[q] + dw0[q] * dw0[q], beta, v0[q], g0[q]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float dh = m[k + 2] - m[k + 1]; float v;
        dw1[k] = z[k + 1] - m[k + 1];
        cell_terms<MODE>(dh * dh + dw1[k] * dw1[k], beta, v, g1[k]);
    }
    float grad[4];
    double acc = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = c + k;
        const bool in = r < H && j < W;
        const bool cellA = in && r < H - 1 && j < W - 1, cellB = in && r < H - 1 && j >= 1, cellC = in && r >= 1 && j < W - 1;
        const float a = cellA ? g0[k + 1] * (-dh0[k + 1] - dw0[k + 1]) : 0.f;
        const float b = cellB ? g0[k] * dh0[k] : 0.f;
        const float d = cellC ? g1[k] * dw1[k] : 0.f;
        grad[k] = (a + b) + d;
        acc += (double)(cellA ? v0[k + 1] : 0.f);
    }
    const float coef = dout ? grad_scale * weight[(long long)(blockIdx.y / S) * weight_stride] : 0.f;
    if (dout && !(accumulate && coef == 0.f)) {         // a fit of weight 0 among weighted ones keeps its dout to the bit (block-uniform)
#pragma clang fp contract(off)                          // product, then sum: accumulate = 1 is bit for bit the preset plus what accumulate = 0 writes
        float* __restrict__ drow = dout + plane + (long long)rz * W;
        if (VEC) {
            if (r < H && c < W) {
                float4* dp = reinterpret_cast<float4*>(drow + c);
                float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
                if (accumulate) o = *dp;
                o.x += coef * grad[0]; o.y += coef * grad[1]; o.z += coef * grad[2]; o.w += coef * grad[3];
                *dp = o;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (r < H && c + k < W) drow[c + k] = (accumulate ? drow[c + k] : 0.f) + coef * grad[k];
        }
    }
    if (partial) {
        const double b = block_sum_d(acc, s_red);
        if (tid == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = b;
    }
}

// one block per fit: thread i adds the fit's partials i, i + 256, ... in index order, the 256 sums meet in block_sum_d's fixed order
__global__ __launch_bounds__(256) void tv_finish_kernel(const double* __restrict__ partial, long long n_per_fit, double* __restrict__ tv)
{
    __shared__ double s_red[8];
    const double* __restrict__ p = partial + (long long)blockIdx.x * n_per_fit;
    double a = 0;
    for (long long t = threadIdx.x; t < n_per_fit; t += 256) a += p[t];
    a = block_sum_d(a, s_red);
    if (threadIdx.x == 0) tv[blockIdx.x] += a;
}

inline long long n_tiles_of(int H, int W) { return (long long)((H + TH - 1) / TH) * ((W + TW - 1) / TW); }

inline bool shape_ok(int n_fits, int S, int H, int W)
{
    return n_fits >= 1 && S >= 1 && (long long)n_fits * S <= 65535 && H >= 1 && W >= 1 && n_tiles_of(H, W) <= 0x7fffffffLL;
}

template <int MODE>
void launch(bool vec, dim3 grid, hipStream_t st, const float* out, int S, int C, int H, int W, int channel, int tiles_x, float beta, const float* weight,
            int weight_stride, float grad_scale, int accumulate, float* dout, double* partial)
{
    if (vec)
        hipLaunchKernelGGL((tv_term_kernel<MODE, true>), grid, dim3(256), 0, st, out, S, C, H, W, channel, tiles_x, beta, weight, weight_stride, grad_scale,
                           accumulate, dout, partial);
    else
        hipLaunchKernelGGL((tv_term_kernel<MODE, false>), grid, dim3(256), 0, st, out, S, C, H, W, channel, tiles_x, beta, weight, weight_stride, grad_scale,
                           accumulate, dout, partial);
}

}  // namespace

extern "C" {

size_t mfvi_tv_term_scratch_bytes(int n_fits, int S, int H, int W)
{
    if (!shape_ok(n_fits, S, H, W)) return 0;
    return (size_t)n_fits * (size_t)S * (size_t)n_tiles_of(H, W) * sizeof(double);
}

int mfvi_tv_term(const float* out, int n_fits, int S, int C, int H, int W, int channel, float beta, const float* weight, int weight_stride,
                 float grad_scale, int accumulate, float* dout, double* tv, void* scratch, void* stream)
{
    if (!out || !weight || !scratch || (!dout && !tv) || !shape_ok(n_fits, S, H, W) || C < 1 || channel < 0 || channel >= C || !(beta > 0.f) ||
        !std::isfinite(beta) || (weight_stride != 0 && weight_stride != 1)) {
        set_error("tv_term: bad arguments (out, weight and scratch non-null, dout or tv non-null, n_fits=%d S=%d with n_fits * S in 1..65535, C=%d, "
                  "channel=%d in 0..C-1, H=%d W=%d >= 1, beta=%g > 0 and finite, weight_stride=%d 0 or 1; scratch of "
                  "mfvi_tv_term_scratch_bytes(n_fits, S, H, W) bytes)", n_fits, S, C, channel, H, W, (double)beta, weight_stride);
        return -1; }
    const int tiles_x = (W + TW - 1) / TW, n_tiles = (int)n_tiles_of(H, W);
    const bool vec = W % 4 == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)dout & 15) == 0;
    const dim3 grid(n_tiles, n_fits * S);
    hipStream_t st = (hipStream_t)stream;
    double* partial = tv ? (double*)scratch : nullptr;
    if (beta == 0.5f)
        launch<BETA_HALF>(vec, grid, st, out, S, C, H, W, channel, tiles_x, beta, weight, weight_stride, grad_scale, accumulate, dout, partial);
    else if (beta == 1.f)
        launch<BETA_ONE>(vec, grid, st, out, S, C, H, W, channel, tiles_x, beta, weight, weight_stride, grad_scale, accumulate, dout, partial);
    else
        launch<BETA_ANY>(vec, grid, st, out, S, C, H, W, channel, tiles_x, beta, weight, weight_stride, grad_scale, accumulate, dout, partial);
    if (tv)
        hipLaunchKernelGGL(tv_finish_kernel, dim3(n_fits), dim3(256), 0, st, (const double*)scratch, (long long)S * n_tiles, tv);
    return (int)hipGetLastError();
}

}  // extern "C"
