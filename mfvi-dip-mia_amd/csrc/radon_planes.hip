// K7b — the Radon pair of the drop-in FastRadonTransform (radon.py): parallel-reduction kernels for the operating
// point of the reference's loop, one plane at a time between the net's forward and backward.  The operator is that of radon.hip
// (radon/radon.py:23-55), restated as a rotation about the image centre m = (S - 1) / 2: detector bin j, row i sample the image at
//     ix = c (j - m) - s (i - m) + m,   iy = s (j - m) + c (i - m) + m          (c, s = cosf / sinf of the fp32 angle, as radon.hip)
// bilinear, zero padding; sino[t][j] = sum_i sample(ix, iy).
// project     : a block owns (plane, angle, strip of 64 bins); lanes are adjacent bins, the block's waves split the rows [0, S) in equal
//               chunks, each wave clips its chunk to the rows where the strip's rays meet the image, and the per-wave partial sums are
//               combined through LDS in wave order.  Coordinates advance by (-s, c) per row in fp64 from a base computed once.
//               No branch in the row loop: loads at clamped indices (the two x-neighbours of a row as one 8-byte load), weights of
//               out-of-image neighbours zeroed by selects.
// backproject : a gather, no atomics.  A block owns (plane, 8 x 8 pixels); its waves split the angles, (c, s) of the angles are computed
//               once per block into LDS, and the partial sums are combined through LDS in wave order.  Per angle only the 3 x 3 samples
//               around rint(R^T (x - m, y - m) + m) can touch the pixel (a rotation is an isometry); the centre candidate's forward position
//               is recomputed in fp64 (so the weights are the forward's: an exact transpose), its 8 neighbours by fp32 rotated unit offsets.
// Both are bit-identical from call to call: the split and the summation order depend on the shapes only.
#include "common.h"
#include "../../include/mfvi_hip.h"

namespace {

constexpr float DEG2RAD = 0.017453292519943295f;      // torch.deg2rad in fp32 (radon/radon.py:31)
constexpr int MAX_WAVES = 16;                         // waves of a block (1024 threads)
constexpr int TARGET_WAVES = 8192;                    // 256 CUs x 32 waves: the split factor fills the chip from the shapes alone
constexpr int ANGLE_TILE = 256;                       // angles whose (c, s) sit in LDS at a time (backproject)

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

// PAIR (S >= 2): the two x-neighbours of a sample come from one load at clamp(x0, 0, S - 2) and are told apart by selects
template <bool PAIR>
__global__ __launch_bounds__(64 * MAX_WAVES) void radon_project_kernel(const float* __restrict__ img, const float* __restrict__ theta, int S,
                                                                        int T, int strips, int chunk, float* __restrict__ sino)
{
    __shared__ double part[MAX_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int t = blockIdx.x / strips, strip = blockIdx.x - t * strips, k = blockIdx.y;
    const int j = strip * 64 + lane;
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
    if (wave == 0 && j < S) {
        double tot = part[0][lane];
        for (int w = 1; w < nw; ++w) tot += part[w][lane];
        sino[((long long)k * T + t) * S + j] = (float)tot;
    }
}

__global__ __launch_bounds__(64 * MAX_WAVES) void radon_backproject_kernel(const float* __restrict__ dsino, const float* __restrict__ theta,
                                                                            int S, int T, int tiles, float* __restrict__ dimg)
{
    __shared__ float2 cs[ANGLE_TILE];
    __shared__ double part[MAX_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int ty = blockIdx.x / tiles, tx = blockIdx.x - ty * tiles, k = blockIdx.y;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const double m = 0.5 * (double)(S - 1), dx = (double)x - m, dy = (double)y - m;
    const float* __restrict__ ds = dsino + (long long)k * T * S;
    double acc = 0;
    for (int t0 = 0; t0 < T; t0 += ANGLE_TILE) {
        const int nt = min(ANGLE_TILE, T - t0);
        __syncthreads();                                                             // the previous tile has been consumed
        for (int q = threadIdx.x; q < nt; q += blockDim.x) {
            const float th = theta[t0 + q] * DEG2RAD;
            cs[q] = make_float2(cosf(th), sinf(th));
        }
        __syncthreads();
#pragma unroll 2
        for (int q = wave; q < nt; q += nw) {
            const float cf = cs[q].x, sf = cs[q].y;
            const double c = (double)cf, s = (double)sf;
            const double jr = rint(c * dx + s * dy + m), ir = rint(c * dy - s * dx + m);       // the sample nearest to the pixel
            const int jc = (int)jr, ic = (int)ir;
            // straight line: the three bins of the neighbourhood, unconditionally at clamped indices, ahead of the weights
            const float* __restrict__ row = ds + (t0 + q) * S;
            float g[3];
#pragma unroll
            for (int dj = -1; dj <= 1; ++dj) g[dj + 1] = row[min(max(jc + dj, 0), S - 1)];
            const float ox = (float)(c * (jr - m) - s * (ir - m) - dx);                          // its forward position minus the pixel
            const float oy = (float)(s * (jr - m) + c * (ir - m) - dy);
            float val = 0.f;
#pragma unroll
            for (int dj = -1; dj <= 1; ++dj) {
                float wsum = 0.f;
#pragma unroll
                for (int di = -1; di <= 1; ++di) {
                    const float wx = fmaxf(1.f - fabsf(ox + cf * (float)dj - sf * (float)di), 0.f);
                    const float wy = fmaxf(1.f - fabsf(oy + sf * (float)dj + cf * (float)di), 0.f);
                    const int i = ic + di;
                    wsum += (i >= 0 && i < S) ? wx * wy : 0.f;
                }
                const int j = jc + dj;
                val += ((j >= 0 && j < S) ? wsum : 0.f) * g[dj + 1];
            }
            acc += (double)val;
        }
    }
    part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && x < S && y < S) {
        double tot = part[0][lane];
        for (int w = 1; w < nw; ++w) tot += part[w][lane];
        dimg[(long long)k * S * S + y * S + x] = (float)tot;
    }
}

// waves per block: the smallest power of two that brings `units` blocks to TARGET_WAVES waves, at most MAX_WAVES and at most `cap`
int split_factor(long long units, int cap)
{
    int nw = 1;
    while (nw < MAX_WAVES && nw * 2 <= cap && units * nw < TARGET_WAVES) nw *= 2;
    return nw;
}

int check(const char* who, const void* a, const void* b, const void* c, int n, int S, int T)
{
    if (!a || !b || !c) { set_error("%s: null tensor", who); return -1; }
    if (n < 1 || n > 65535 || S < 1 || S > 32768 || T < 1 || T > 32768) {
        set_error("%s: bad shape n=%d S=%d T=%d (1 <= n <= 65535 planes, 1 <= S, T <= 32768)", who, n, S, T); return -1; }
    return 0;
}

}  // namespace

extern "C" {

int mfvi_radon_project(const float* img, const float* theta_deg, int n, int S, int T, float* sino, void* stream)
{
    if (check("radon_project", img, theta_deg, sino, n, S, T)) return -1;
    const int strips = (S + 63) / 64;
    const int nw = split_factor((long long)n * T * strips, (S + 7) / 8);             // a wave keeps at least 8 rows
    const int chunk = (S + nw - 1) / nw;
    if (S >= 2)
        hipLaunchKernelGGL(radon_project_kernel<true>, dim3((unsigned)(T * strips), n), dim3(64 * nw), 0, (hipStream_t)stream, img, theta_deg,
                           S, T, strips, chunk, sino);
    else
        hipLaunchKernelGGL(radon_project_kernel<false>, dim3((unsigned)(T * strips), n), dim3(64 * nw), 0, (hipStream_t)stream, img, theta_deg,
                           S, T, strips, chunk, sino);
    return (int)hipGetLastError();
}

int mfvi_radon_backproject(const float* dsino, const float* theta_deg, int n, int S, int T, float* dimg, void* stream)
{
    if (check("radon_backproject", dsino, theta_deg, dimg, n, S, T)) return -1;
    const int tiles = (S + 7) / 8;
    const int nw = split_factor((long long)n * tiles * tiles, T);                    // a wave keeps at least one angle
    hipLaunchKernelGGL(radon_backproject_kernel, dim3((unsigned)(tiles * tiles), n), dim3(64 * nw), 0, (hipStream_t)stream, dsino, theta_deg,
                       S, T, tiles, dimg);
    return (int)hipGetLastError();
}

}  // extern "C"
