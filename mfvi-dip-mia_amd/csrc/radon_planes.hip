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
#include "radon_rows.h"
#include "../../include/mfvi_hip.h"

namespace {

using namespace radon_rows;                           // DEG2RAD, MAX_WAVES, split_factor and the project kernel's row loop (shared with radon_fits.hip)
constexpr int ANGLE_TILE = 256;                       // angles whose (c, s) sit in LDS at a time (backproject)

template <bool PAIR>
__global__ __launch_bounds__(64 * MAX_WAVES) void radon_project_kernel(const float* __restrict__ img, const float* __restrict__ theta, int S,
                                                                        int T, int strips, int chunk, float* __restrict__ sino)
{
    __shared__ double part[MAX_WAVES][64];
    Ray r;
    const double tot = project_rows<PAIR>(img, theta, S, strips, chunk, part, r);
    if (threadIdx.x < 64 && r.j < S) sino[((long long)r.k * T + r.t) * S + r.j] = (float)tot;
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
    const Split sp = project_split(n, S, T);
    const int strips = sp.strips, nw = sp.nw, chunk = sp.chunk;
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
