// Signal-to-noise pruning of a fitted posterior (BayTorch/inference/utils.py:104-166 L1UnstructuredFFG / prune_weights_ffg, the SNR
// histograms of BayTorch/visualize): the keys |mu| / softplus(rho), an exact k-th-smallest selection over them per
// parameter row and per group (0 = the convolution weights, 1 = the biases, the reference's separate W_* / bias_* calls), the pruned copy of
// the parameter rows, and the histogram of the keys.
//
// Order: unsigned compare of bits(key) & 0x7fffffff, ties by ascending flat index.  Keys are >= 0, so this is the order of the floats with
// NaN (mu = 0 over sigma = 0, or a NaN parameter) above +inf -- the order of a stable argsort of the reference's log(snr)
// (inference/utils.py:116-123, 139-142).
//
// Selection: an MSB-first radix select over the 31 key bits in four digits (8, 8, 8, 7 bits).  Per digit every block counts the keys that
// still match the chosen prefix in an LDS histogram and flushes it with integer atomics; one thread per (row, group) then picks the digit
// that holds rank k and clears the histogram.  After the last digit the prefix is the k-th smallest key (the threshold) and the remaining
// rank is the number of keys EQUAL to it that are pruned: those with the lowest indices.  The final two launches give every block one
// contiguous range of the row: the first counts the range's keys equal to the threshold, the second adds the counts of the blocks in front
// of it (integers, any order), ranks the equal keys of its range by a ballot prefix in index order, and writes the mask.  Only integer
// atomics, no "last block" handshake, no host round-trip: bit-identical from call to call.
//
// Bounds: a kernel indexes memory by (row, j) with j < n_vi only; the segment table is used for comparisons against j, never as an index,
// and k is clamped to the group's size on the device.  A table that is not sorted gives a wrong answer, not a stray access.
#include "common.h"
#include "iter_ops.h"
#include "../../include/mfvi_hip.h"

namespace {

constexpr int PR_THREADS = 256;
constexpr int PR_WAVES = PR_THREADS / 64;
constexpr int PR_MAX_BLOCKS = 2048;                  // blocks per row (iter_ops.h nblocks' cap)
constexpr int PR_GROUPS = MFVI_PRUNE_GROUPS;
constexpr int PR_MAX_SEG = MFVI_PRUNE_MAX_SEGMENTS;
constexpr int PR_DIGITS = 4;
constexpr int PR_BINS = 256;
constexpr int PR_MAX_HBINS = MFVI_SNR_MAX_BINS;

__host__ __device__ inline int digit_shift(int pass) { return pass == 0 ? 23 : pass == 1 ? 15 : pass == 2 ? 7 : 0; }
__host__ __device__ inline int digit_mask(int pass) { return pass == 3 ? 127 : 255; }

struct SelState { long long k_rem; unsigned prefix; unsigned pad; };

// scratch of mfvi_snr_select: [rows][2][256] uint32 digit histogram | [rows][2] SelState | [rows][2][PR_MAX_BLOCKS] uint32 equal counts
inline long long hist_words(int rows) { return (long long)rows * PR_GROUPS * PR_BINS; }
inline long long state_off_bytes(int rows) { return hist_words(rows) * 4; }
inline long long cnt_off_bytes(int rows) { return state_off_bytes(rows) + (long long)rows * PR_GROUPS * (long long)sizeof(SelState); }
inline long long total_bytes(int rows) { return cnt_off_bytes(rows) + (long long)rows * PR_GROUPS * PR_MAX_BLOCKS * 4; }

// the segment table in LDS: [s_lo[i], s_hi[i]) clamped to [0, n_vi], group s_g[i] (-1: neither group)
struct SegLds { int lo[PR_MAX_SEG], hi[PR_MAX_SEG], g[PR_MAX_SEG]; };

__device__ __forceinline__ void load_segments(SegLds& S, const mfvi_prune_segment* __restrict__ segs, int n_seg, int n_vi)
{
    for (int i = threadIdx.x; i < n_seg; i += PR_THREADS) {
        long long lo = segs[i].offset, c = segs[i].count;
        lo = lo < 0 ? 0 : (lo > n_vi ? n_vi : lo);
        c = c < 0 ? 0 : (c > n_vi ? n_vi : c);
        long long hi = lo + c;
        if (hi > n_vi) hi = n_vi;
        const int g = segs[i].group;
        S.lo[i] = (int)lo; S.hi[i] = (int)hi; S.g[i] = (g == 0 || g == 1) ? g : -1;
    }
    __syncthreads();
}

// group of element j, or -1: the last segment that starts at or before j (the table is sorted by offset), if j lies inside it
__device__ __forceinline__ int group_of(const SegLds& S, int n_seg, int j)
{
    int lo = 0, hi = n_seg;                       // first segment with S.lo > j
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (S.lo[mid] <= j) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return -1;
    return j < S.hi[lo - 1] ? S.g[lo - 1] : -1;
}

__device__ __forceinline__ unsigned key_bits(float k) { return __float_as_uint(k) & 0x7fffffffu; }

// key[row][j] = |mu| / softplus(rho): one IEEE division (inference/utils.py:116-118 ranks by the log of this ratio; the order is the same)
__global__ __launch_bounds__(PR_THREADS) void snr_keys_kernel(const float* __restrict__ params, long long stride, int n_vi, float* __restrict__ keys)
{
    const float* __restrict__ p = params + (long long)blockIdx.y * stride;
    float* __restrict__ k = keys + (long long)blockIdx.y * n_vi;
    for (long long j = (long long)blockIdx.x * PR_THREADS + threadIdx.x; j < n_vi; j += (long long)gridDim.x * PR_THREADS)
        k[j] = fabsf(p[j]) / softplus_f(p[(long long)n_vi + j]);
}

__global__ __launch_bounds__(PR_THREADS) void select_init_kernel(const long long* __restrict__ k, int pairs, unsigned* __restrict__ hist, SelState* __restrict__ st)
{
    const long long n = (long long)pairs * PR_BINS;
    for (long long i = (long long)blockIdx.x * PR_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * PR_THREADS) hist[i] = 0u;
    for (long long i = (long long)blockIdx.x * PR_THREADS + threadIdx.x; i < pairs; i += (long long)gridDim.x * PR_THREADS) {
        const long long v = k[i];
        st[i].k_rem = v < 0 ? 0 : v; st[i].prefix = 0u; st[i].pad = 0u;
    }
}

__global__ __launch_bounds__(PR_THREADS) void select_hist_kernel(const float* __restrict__ keys, int n_vi, const mfvi_prune_segment* __restrict__ segs, int n_seg,
                                                                 int pass, const SelState* __restrict__ st, unsigned* __restrict__ hist)
{
    __shared__ SegLds S;
    __shared__ unsigned s_h[PR_GROUPS][PR_BINS];
    const int row = blockIdx.y;
    for (int i = threadIdx.x; i < PR_GROUPS * PR_BINS; i += PR_THREADS) (&s_h[0][0])[i] = 0u;
    load_segments(S, segs, n_seg, n_vi);                              // its barrier also publishes s_h
    const int shift = digit_shift(pass), dmask = digit_mask(pass);
    const int up = pass == 0 ? 31 : digit_shift(pass - 1);            // the bits above this digit: must equal the prefix chosen so far
    const unsigned pre[PR_GROUPS] = {st[row * PR_GROUPS].prefix >> up, st[row * PR_GROUPS + 1].prefix >> up};
    const float* __restrict__ k = keys + (long long)row * n_vi;
    for (long long j = (long long)blockIdx.x * PR_THREADS + threadIdx.x; j < n_vi; j += (long long)gridDim.x * PR_THREADS) {
        const int g = group_of(S, n_seg, (int)j);
        if (g < 0) continue;
        const unsigned b = key_bits(k[j]);
        if ((b >> up) == pre[g]) atomicAdd(&s_h[g][(b >> shift) & dmask], 1u);
    }
    __syncthreads();
    unsigned* __restrict__ h = hist + (long long)row * PR_GROUPS * PR_BINS;
    for (int i = threadIdx.x; i < PR_GROUPS * PR_BINS; i += PR_THREADS) {
        const unsigned c = (&s_h[0][0])[i];
        if (c) atomicAdd(&h[i], c);
    }
}

// one thread per (row, group): the digit that holds rank k_rem (1-based) among the keys matching the prefix; clears the histogram for the
// next digit.  Pass 0 sees the whole group: k is clamped to its size there.  After the last digit: threshold and tie count.
__global__ void select_pick_kernel(int pairs, int pass, unsigned* __restrict__ hist, SelState* __restrict__ st, unsigned* __restrict__ thr,
                                   long long* __restrict__ ties)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pairs) return;
    unsigned* h = hist + (long long)i * PR_BINS;
    long long k = st[i].k_rem;
    if (pass == 0) {
        long long total = 0;
        for (int d = 0; d < PR_BINS; ++d) total += h[d];
        if (k > total) k = total;
    }
    unsigned prefix = st[i].prefix;
    if (k > 0) {
        long long cum = 0;
        int d = 0;
        for (; d < digit_mask(pass); ++d) {                           // the last digit takes what is left
            if (cum + h[d] >= k) break;
            cum += h[d];
        }
        k -= cum;
        prefix |= (unsigned)d << digit_shift(pass);
    }
    for (int d = 0; d < PR_BINS; ++d) h[d] = 0u;
    st[i].k_rem = k; st[i].prefix = prefix;
    if (pass == PR_DIGITS - 1) { thr[i] = k > 0 ? prefix : 0u; ties[i] = k; }
}

// the contiguous range of block b: [b * chunk, (b + 1) * chunk) cut at n_vi, chunk a multiple of the block size
__device__ __forceinline__ void block_range(int n_vi, long long& j0, long long& j1)
{
    long long chunk = ((long long)n_vi + gridDim.x - 1) / gridDim.x;
    chunk = (chunk + PR_THREADS - 1) / PR_THREADS * PR_THREADS;
    j0 = (long long)blockIdx.x * chunk;
    j1 = j0 + chunk;
    if (j0 > n_vi) j0 = n_vi;
    if (j1 > n_vi) j1 = n_vi;
}

__global__ __launch_bounds__(PR_THREADS) void select_count_kernel(const float* __restrict__ keys, int n_vi, const mfvi_prune_segment* __restrict__ segs, int n_seg,
                                                                  const SelState* __restrict__ st, unsigned* __restrict__ cnt)
{
    __shared__ SegLds S;
    __shared__ unsigned s_c[PR_GROUPS];
    const int row = blockIdx.y;
    if (threadIdx.x < PR_GROUPS) s_c[threadIdx.x] = 0u;
    load_segments(S, segs, n_seg, n_vi);
    const unsigned thr[PR_GROUPS] = {st[row * PR_GROUPS].prefix, st[row * PR_GROUPS + 1].prefix};
    const float* __restrict__ k = keys + (long long)row * n_vi;
    long long j0, j1;
    block_range(n_vi, j0, j1);
    unsigned c[PR_GROUPS] = {0u, 0u};
    for (long long j = j0 + threadIdx.x; j < j1; j += PR_THREADS) {
        const int g = group_of(S, n_seg, (int)j);
        if (g >= 0 && key_bits(k[j]) == thr[g]) ++c[g];
    }
#pragma unroll
    for (int g = 0; g < PR_GROUPS; ++g)
        if (c[g]) atomicAdd(&s_c[g], c[g]);
    __syncthreads();
    if (threadIdx.x < PR_GROUPS) cnt[((long long)row * PR_GROUPS + threadIdx.x) * PR_MAX_BLOCKS + blockIdx.x] = s_c[threadIdx.x];
}

__global__ __launch_bounds__(PR_THREADS) void select_mark_kernel(const float* __restrict__ keys, int n_vi, const mfvi_prune_segment* __restrict__ segs, int n_seg,
                                                                 const SelState* __restrict__ st, const unsigned* __restrict__ cnt, unsigned char* __restrict__ mask)
{
    __shared__ SegLds S;
    __shared__ unsigned long long s_base[PR_GROUPS];
    __shared__ unsigned s_w[PR_GROUPS][PR_WAVES];
    const int row = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < PR_GROUPS) s_base[threadIdx.x] = 0ull;
    load_segments(S, segs, n_seg, n_vi);
    // equal keys in the ranges in front of this block's (integer sums: the order of the additions does not matter)
#pragma unroll
    for (int g = 0; g < PR_GROUPS; ++g) {
        const unsigned* __restrict__ c = cnt + ((long long)row * PR_GROUPS + g) * PR_MAX_BLOCKS;
        unsigned long long s = 0ull;
        for (int b = threadIdx.x; b < (int)blockIdx.x; b += PR_THREADS) s += c[b];
        if (s) atomicAdd(&s_base[g], s);
    }
    __syncthreads();
    unsigned thr[PR_GROUPS];
    long long ties[PR_GROUPS], seen[PR_GROUPS];
#pragma unroll
    for (int g = 0; g < PR_GROUPS; ++g) {
        thr[g] = st[row * PR_GROUPS + g].prefix; ties[g] = st[row * PR_GROUPS + g].k_rem; seen[g] = (long long)s_base[g];
    }
    const float* __restrict__ k = keys + (long long)row * n_vi;
    unsigned char* __restrict__ m = mask + (long long)row * n_vi;
    long long j0, j1;
    block_range(n_vi, j0, j1);
    for (long long t = j0; t < j1; t += PR_THREADS) {                 // t and the trip count are uniform over the block
        const long long j = t + threadIdx.x;
        const bool in = j < j1;
        const int g = in ? group_of(S, n_seg, (int)j) : -1;
        const unsigned b = in ? key_bits(k[j]) : 0u;
        const bool eq0 = g == 0 && b == thr[0], eq1 = g == 1 && b == thr[1];
        const unsigned long long bal0 = __ballot(eq0), bal1 = __ballot(eq1);
        if (lane == 0) { s_w[0][wave] = (unsigned)__popcll(bal0); s_w[1][wave] = (unsigned)__popcll(bal1); }
        __syncthreads();
        const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
        long long rank[PR_GROUPS] = {seen[0] + __popcll(bal0 & below), seen[1] + __popcll(bal1 & below)};
#pragma unroll
        for (int w = 0; w < PR_WAVES; ++w) {
            if (w < wave) { rank[0] += s_w[0][w]; rank[1] += s_w[1][w]; }
            seen[0] += s_w[0][w]; seen[1] += s_w[1][w];
        }
        if (in) {
            bool pruned = false;
            if (g >= 0 && ties[g] > 0) pruned = b < thr[g] || (b == thr[g] && rank[g] < ties[g]);
            m[j] = pruned ? 0 : 1;
        }
        __syncthreads();                                              // s_w is rewritten by the next trip
    }
}

// dst row = src row, with mu = +0 and rho = MFVI_PRUNED_RHO where the mask is 0; the BN tail (and whatever else lies below row_floats) copied
__global__ __launch_bounds__(PR_THREADS) void prune_apply_kernel(const float* __restrict__ src, float* __restrict__ dst, const unsigned char* __restrict__ mask,
                                                                 long long stride, int n_vi, long long row_floats)
{
    const float* __restrict__ s = src + (long long)blockIdx.y * stride;
    float* __restrict__ d = dst + (long long)blockIdx.y * stride;
    const unsigned char* __restrict__ m = mask + (long long)blockIdx.y * n_vi;
    for (long long j = (long long)blockIdx.x * PR_THREADS + threadIdx.x; j < row_floats; j += (long long)gridDim.x * PR_THREADS) {
        float v = s[j];
        if (j < n_vi) { if (!m[j]) v = 0.f; }
        else if (j < 2LL * n_vi) { if (!m[j - n_vi]) v = MFVI_PRUNED_RHO; }
        d[j] = v;
    }
}

// bin = the number of boundaries b[i] <= key (np.searchsorted(b, key, side='right')): 0 underflow, n_bins + 1 overflow; NaN counts as overflow
__device__ __forceinline__ int hist_bin(float key, const float* b, int nb1)
{
    if (key != key) return nb1;
    int lo = 0, hi = nb1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (b[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PR_THREADS) void snr_hist_zero_kernel(unsigned long long* __restrict__ counts, long long n)
{
    for (long long i = (long long)blockIdx.x * PR_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * PR_THREADS) counts[i] = 0ull;
}

__global__ __launch_bounds__(PR_THREADS) void snr_hist_kernel(const float* __restrict__ keys, int n_vi, const mfvi_prune_segment* __restrict__ segs, int n_seg,
                                                              const float* __restrict__ bounds, int n_bins, unsigned long long* __restrict__ counts)
{
    __shared__ SegLds S;
    __shared__ float s_b[PR_MAX_HBINS + 1];
    __shared__ unsigned s_h[PR_GROUPS][PR_MAX_HBINS + 2];
    const int row = blockIdx.y, slots = n_bins + 2;
    for (int i = threadIdx.x; i <= n_bins; i += PR_THREADS) s_b[i] = bounds[i];
    for (int i = threadIdx.x; i < slots; i += PR_THREADS) { s_h[0][i] = 0u; s_h[1][i] = 0u; }
    load_segments(S, segs, n_seg, n_vi);
    const float* __restrict__ k = keys + (long long)row * n_vi;
    for (long long j = (long long)blockIdx.x * PR_THREADS + threadIdx.x; j < n_vi; j += (long long)gridDim.x * PR_THREADS) {
        const int g = group_of(S, n_seg, (int)j);
        if (g >= 0) atomicAdd(&s_h[g][hist_bin(k[j], s_b, n_bins + 1)], 1u);
    }
    __syncthreads();
    unsigned long long* __restrict__ c = counts + (long long)row * PR_GROUPS * slots;
    for (int i = threadIdx.x; i < PR_GROUPS * slots; i += PR_THREADS) {
        const unsigned v = s_h[i / slots][i % slots];
        if (v) atomicAdd(&c[i], (unsigned long long)v);
    }
}

inline bool rows_ok(int rows) { return rows >= 1 && rows <= 65535; }
inline bool nvi_ok(int64_t n_vi) { return n_vi >= 1 && n_vi < (1LL << 31); }

}  // namespace

extern "C" {

int mfvi_snr_keys(const float* params, int rows, int64_t stride, int64_t n_vi, float* keys, void* stream)
{
    if (!nvi_ok(n_vi)) { set_error("snr_keys: n_vi=%lld outside 1..2^31-1", (long long)n_vi); return -2; }
    if (!params || !keys || !rows_ok(rows) || stride < 2 * n_vi) {
        set_error("snr_keys: bad arguments (rows=%d stride=%lld n_vi=%lld; stride >= 2 n_vi, rows in 1..65535)", rows, (long long)stride, (long long)n_vi);
        return -1;
    }
    hipLaunchKernelGGL(snr_keys_kernel, dim3(nblocks(n_vi, PR_MAX_BLOCKS), rows), dim3(PR_THREADS), 0, (hipStream_t)stream, params, (long long)stride, (int)n_vi, keys);
    return (int)hipGetLastError();
}

int64_t mfvi_snr_select_scratch_bytes(int rows)
{
    if (!rows_ok(rows)) { set_error("snr_select_scratch_bytes: rows=%d outside 1..65535", rows); return -1; }
    return total_bytes(rows);
}

int mfvi_snr_select(const float* keys, int rows, int64_t n_vi, const mfvi_prune_segment* segs, int n_seg, const int64_t* k, uint8_t* mask,
                    uint32_t* threshold, int64_t* ties, void* scratch, void* stream)
{
    if (!nvi_ok(n_vi)) { set_error("snr_select: n_vi=%lld outside 1..2^31-1", (long long)n_vi); return -2; }
    if (n_seg < 0 || n_seg > PR_MAX_SEG) { set_error("snr_select: n_seg=%d outside 0..%d", n_seg, PR_MAX_SEG); return -2; }
    if (!keys || (!segs && n_seg) || !k || !mask || !threshold || !ties || !scratch || !rows_ok(rows) || ((uintptr_t)scratch & 7)) {
        set_error("snr_select: bad arguments (rows=%d n_vi=%lld n_seg=%d; scratch 8-byte aligned)", rows, (long long)n_vi, n_seg); return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    const int pairs = rows * PR_GROUPS, nvi = (int)n_vi, nb = nblocks(n_vi, PR_MAX_BLOCKS);
    unsigned* hist = (unsigned*)scratch;
    SelState* state = (SelState*)((char*)scratch + state_off_bytes(rows));
    unsigned* cnt = (unsigned*)((char*)scratch + cnt_off_bytes(rows));
    hipLaunchKernelGGL(select_init_kernel, dim3(nblocks((long long)pairs * PR_BINS, 256)), dim3(PR_THREADS), 0, st, (const long long*)k, pairs, hist, state);
    for (int pass = 0; pass < PR_DIGITS; ++pass) {
        hipLaunchKernelGGL(select_hist_kernel, dim3(nb, rows), dim3(PR_THREADS), 0, st, keys, nvi, segs, n_seg, pass, (const SelState*)state, hist);
        hipLaunchKernelGGL(select_pick_kernel, dim3((pairs + 63) / 64), dim3(64), 0, st, pairs, pass, hist, state, (unsigned*)threshold, (long long*)ties);
    }
    hipError_t e = hipGetLastError(); if (e) return (int)e;
    hipLaunchKernelGGL(select_count_kernel, dim3(nb, rows), dim3(PR_THREADS), 0, st, keys, nvi, segs, n_seg, (const SelState*)state, cnt);
    hipLaunchKernelGGL(select_mark_kernel, dim3(nb, rows), dim3(PR_THREADS), 0, st, keys, nvi, segs, n_seg, (const SelState*)state, (const unsigned*)cnt,
                       (unsigned char*)mask);
    return (int)hipGetLastError();
}

int mfvi_prune_apply(const float* src, float* dst, const uint8_t* mask, int rows, int64_t stride, int64_t n_vi, int64_t row_floats, void* stream)
{
    if (!nvi_ok(n_vi)) { set_error("prune_apply: n_vi=%lld outside 1..2^31-1", (long long)n_vi); return -2; }
    if (!src || !dst || !mask || src == dst || !rows_ok(rows) || row_floats < 2 * n_vi || stride < row_floats) {
        set_error("prune_apply: bad arguments (rows=%d stride=%lld n_vi=%lld row_floats=%lld; 2 n_vi <= row_floats <= stride, dst != src)", rows,
                  (long long)stride, (long long)n_vi, (long long)row_floats);
        return -1;
    }
    hipLaunchKernelGGL(prune_apply_kernel, dim3(nblocks(row_floats, PR_MAX_BLOCKS), rows), dim3(PR_THREADS), 0, (hipStream_t)stream, src, dst,
                       (const unsigned char*)mask, (long long)stride, (int)n_vi, (long long)row_floats);
    return (int)hipGetLastError();
}

int mfvi_snr_histogram(const float* keys, int rows, int64_t n_vi, const mfvi_prune_segment* segs, int n_seg, const float* bounds, int n_bins,
                       int64_t* counts, void* stream)
{
    if (n_bins < 1 || n_bins > PR_MAX_HBINS) { set_error("snr_histogram: n_bins=%d outside 1..%d", n_bins, PR_MAX_HBINS); return -2; }
    if (!nvi_ok(n_vi)) { set_error("snr_histogram: n_vi=%lld outside 1..2^31-1", (long long)n_vi); return -2; }
    if (n_seg < 0 || n_seg > PR_MAX_SEG) { set_error("snr_histogram: n_seg=%d outside 0..%d", n_seg, PR_MAX_SEG); return -2; }
    if (!keys || (!segs && n_seg) || !bounds || !counts || !rows_ok(rows)) {
        set_error("snr_histogram: bad arguments (rows=%d n_vi=%lld)", rows, (long long)n_vi); return -1;
    }
    hipStream_t st = (hipStream_t)stream;
    const long long words = (long long)rows * PR_GROUPS * (n_bins + 2);
    hipLaunchKernelGGL(snr_hist_zero_kernel, dim3(nblocks(words, 256)), dim3(PR_THREADS), 0, st, (unsigned long long*)counts, words);
    hipLaunchKernelGGL(snr_hist_kernel, dim3(nblocks(n_vi, PR_MAX_BLOCKS), rows), dim3(PR_THREADS), 0, st, keys, (int)n_vi, segs, n_seg, bounds, n_bins,
                       (unsigned long long*)counts);
    return (int)hipGetLastError();
}

}  // extern "C"
