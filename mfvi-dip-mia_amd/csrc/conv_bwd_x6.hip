// K2a' for the 3x3 stride-1 layers on maps a multiple of 64 wide: backward-data WITH the fold of the input tensor, on the BF16 matrix cores
// at fp32 accuracy ("bf16x6", round 4).  Autograd of BayTorch/modules/reparam_layers.py:37 behind the ReflectionPad2d(1) of
// models/common.py:100-135, followed by LeakyReLU' and the BatchNorm-backward sums of the layer's input (models/common.py:77-97).
//
// Arithmetic as conv_x6.hip / conv_bww_x6.hip: every fp32 operand is the exact sum of three round-to-nearest bf16 pieces and six
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation stand for one fp32 product-sum (dropped terms <= 2^-23 |a b|).  Here
//     dx[ci][y][x] = sum_{co, ky, kx} W[co][ci][ky][kx] * dy[co][y + 1 - ky][x + 1 - kx]        (dy zero outside the image)
//   M = 16 consecutive pixels of a row, N = 16 INPUT channels ci of the convolution (a "fragment" f), K = 32 OUTPUT channels co of one tap.
//   16 output channels (the 36 -> 16 layer): K = 32 is [piece a | piece b] of the same 16 channels, so THREE instructions
//   ([x_h|x_l].[w_l|w_h], [x_m|x_m].[w_h|w_m], [x_h|x_h].[w_h|w_m]) carry the six products and no K slot is empty.
//
// What the round-3 design note asked for: the staged tensor is staged ONCE per block.  A block owns a 64-pixel
// band and walks T strips of SR output rows down it; the strip's dy window ((SR + 2) rows x 66 pixels x all Cout channels, BN-backward
// formed on load, as three bf16 pieces in channel-octet planes) is resident in LDS while the four matrix waves (wave = 16-pixel fragment)
// run one PASS per (input-channel fragment f, 32-channel reduction group): the pass's weight pieces (pre-split per sample by
// x6b_split_kernel: [f][group][tap][piece][n][k-octet]) go LDS -> registers at its head (108 VGPRs; 72 in the 16-channel form), then the
// window rows stream by: an input row meets the three tap rows of three output rows, the strip's accumulators stay in registers (4 per
// output row).  At the end of a fragment's last pass the SAME waves fold straight from the accumulators: the raw x of their 4 x SR pixels
// of channel 16 f + (lane & 15) was requested at the head of the pass, LeakyReLU'(BN(x)), the BN-backward sums of x (two floats per
// (wave, channel) in LDS, one fp64 atomic per (block, channel, moment) at the end) and ga written once as float4.
// The four staging waves prefetch the NEXT strip's SR new rows during the strip's passes (global dwords -> BN-backward -> three pieces,
// kept in 60 registers) and write them over the SR oldest ring rows at the strip boundary (one short exposed phase per strip); they
// also copy the next pass's weight pieces global -> registers -> LDS.
//
// Reflection adjoint (the gradient is formed on the UN-padded domain):
//   rows:    padded row -1 folds onto image row 1: image row 0 with tap row ky = 0 accumulates into output row 1 as well (18 extra matrix
//            instructions per fragment in a band's first strip); likewise image row H-1 with ky = 2 into row H-2 in the last strip.
//   columns: pixel 1 takes tap kx = 0 from dy[2] + dy[0], pixel W-2 takes kx = 2 from dy[W-3] + dy[W-1]: the staging waves write these
//            two sums (formed in fp32 like conv_rp.hip's column fix-up, then split) into two spare pixel slots of the row planes and the
//            one lane concerned reads its operand there — no extra matrix instruction, no branch.
#include "common.h"
#include <type_traits>
#include <cstdlib>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma_bf(u32x4 a, u32x4 b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__device__ __forceinline__ void split8(const float (&e)[8], u32x4& h, u32x4& m, u32x4& l)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) { unsigned hh, mm, ll; split_pair_bf16x3(e[2 * i], e[2 * i + 1], hh, mm, ll); h[i] = hh; m[i] = mm; l[i] = ll; }
}

#ifndef X6B_PRIO_S
#define X6B_PRIO_S 0
#endif
#ifndef X6B_PRIO_M
#define X6B_PRIO_M 2
#endif
#ifdef X6B_PROF
// dev build: per-phase s_memtime sums of matrix wave 0 / staging wave 0 of every block (scripts/dev/bwdx6_prof.py)
__device__ unsigned long long g_x6b_prof[24];
__device__ __forceinline__ unsigned long long xb_now() { unsigned long long t; asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory"); return t; }
#define XB_T(v) const unsigned long long v = xb_now()
#define XB_ACC(slot, d) prof[slot] += (d)
#else
#define XB_T(v)
#define XB_ACC(slot, d)
#endif

// Global accesses of the staging waves: wave-uniform base pointer + 32-bit BYTE offset per lane (the launcher keeps a sample's tensors
// below 2^29 elements), so the compiler emits the scalar-base form and no per-lane 64-bit address lives in registers (with element
// offsets it could not prove the scaling by 4 free of wrap-around and fell back to v_lshl_add_u64 per access: 16 spilled address registers)
__device__ __forceinline__ float ldg_f(const float* base, unsigned boff) { return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + boff); }
__device__ __forceinline__ float4 ldg_f4(const float* base, unsigned boff) { return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + boff); }
__device__ __forceinline__ void stg_f4(float* base, unsigned boff, float4 v) { *reinterpret_cast<float4*>(reinterpret_cast<char*>(base) + boff) = v; }

// sum over the 16 lanes of a DPP row, result in lane 15 of the row (lanes shifted in from outside the row read 0: bound_ctrl)
__device__ __forceinline__ float row_sum16(float v)
{
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));      // row_shr:1
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));      // row_shr:2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));      // row_shr:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));      // row_shr:8
    return v;
}

// BN-backward on load (conv_rp.hip's dy = (y - mean) * qc + (ga * c1 + k2) with the mean folded into the constant)
struct BwdC { float qc, c1, k3, pad; };                   // dy = ga * c1 + (y * qc + k3), k3 = -c1 c2 - mean * qc: two operations per element

template <bool K16, int SR, int NG>
struct X6BCfg {
    static constexpr int NOCT = K16 ? 2 : 4;               // channel octets per reduction group
    static constexpr int NOCTT = NOCT * NG;                 // octets of the staged tensor
    static constexpr int PLANE = 80 * 16;                   // one (piece, octet) row plane: slots 0..65 = image columns c0-1 .. c0+64, 66 / 67 = the column-adjoint sums; == 0 (mod 256 B): a ds_read_b128 lane group hits 64 distinct banks
    static constexpr int PIECE = NOCTT * PLANE;
    static constexpr int ROWB = 3 * PIECE;
    static constexpr int NR = SR + 2;                       // ring = exactly the strip's window
    static constexpr int RING = NR * ROWB;
    static constexpr int NV = K16 ? 2 : 3;                  // weight operand variants per tap
    static constexpr int WB = 9 * NV * 1024;                // weight pieces of one pass
    static constexpr int NWU = (WB / 16 + 255) / 256;       // 16-byte units per staging thread
    static constexpr int OPB = SR * 256 + 16;               // channel pitch of the finished tile [16][SR][64] floats; == 16 (mod 128 B): the 8 lanes of a ds_write_b128 group (8 channels) hit 32 distinct banks
    static constexpr int SUMW = 1;                           // BN-backward sum slots per channel (the fold gives every channel ONE owner lane)
};

struct X6BArgs {
    GView gin; TView xin; ConvGeom g;
    const unsigned* wsp; long long wsp_stride_u4;           // split pieces, per-sample stride in 16-byte units (0: one copy for all samples)
    float* fga; long long fga_sstride; double* fbsums;
    int NF, bands, strips, tpb, nx, nz;
};

// ---- weight pieces: thread = (f, group, tap, n, k-octet) of sample k -> NV 16-byte operand units ----
// destination (16-byte units): (((f * NG + grp) * 9 + tap) * NV + v) * 64 + g4 * 16 + n
__device__ __forceinline__ void x6b_split_body(const X6BSplitEntry& E, int u, int k, const float* w, long long wstride, float* arena)
{
    if (u >= E.units + E.rem_units) return;
    const float* __restrict__ ww = w + (long long)k * wstride + E.w_off;
    const long long sample_u4 = (long long)(E.units + E.rem_units) * (E.k16 ? 2 : 3);       // 16-byte units per sample
    if (u >= E.units) {
        // the last 4 input channels as ONE operand per kx (conv_bwd_x6s.hip): column n = (tap row ky, channel c), k-octets as the 16-channel form
        const int uu = u - E.units, ln = uu & 63, kx = uu >> 6, g4 = ln >> 4, n = ln & 15, ky = n >> 2, ci = 32 + (n & 3), co0 = 8 * (g4 & 1);
        float e8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e8[j] = ky < 3 ? ww[((long long)(co0 + j) * E.CI + ci) * 9 + ky * 3 + kx] : 0.f;
        u32x4 h, m, l; split8(e8, h, m, l);
        u32x4* d = reinterpret_cast<u32x4*>(arena + E.dst_off) + (long long)k * sample_u4 + (long long)E.units * 2 + (kx * 2) * 64 + ln;
        d[0] = g4 < 2 ? h : m; d[64] = g4 < 2 ? l : h;
        return;
    }
    const int g4 = u & 3, n = (u >> 2) & 15, r = u >> 6, tap = r % 9, fg = r / 9, grp = fg % E.NG, f = fg / E.NG;
    const int ci = 16 * f + n, co0 = 32 * grp + 8 * (E.k16 ? (g4 & 1) : g4);
    float e8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e8[j] = ci < E.CI ? ww[((long long)(co0 + j) * E.CI + ci) * 9 + tap] : 0.f;
    u32x4 h, m, l; split8(e8, h, m, l);
    const int NV = E.k16 ? 2 : 3;
    u32x4* d = reinterpret_cast<u32x4*>(arena + E.dst_off) + (long long)k * sample_u4 + ((long long)r * NV) * 64 + g4 * 16 + n;      // lane order (lane = 16 g4 + n): the wave's read of a unit is 1 KB of consecutive words, conflict-free
    if (E.k16) { d[0] = g4 < 2 ? h : m; d[64] = g4 < 2 ? l : h; }      // [w_h | w_m], [w_l | w_h]
    else { d[0] = h; d[64] = m; d[128] = l; }
}
// every bf16x6 backward-data layer of a plan in ONE launch behind the weight draw
__global__ void x6b_split_kernel(const X6BSplitEntry* __restrict__ table, int n_entries, const float* w, long long wstride, float* arena)
{
    int e = 0;
    while (e + 1 < n_entries && (int)blockIdx.x >= table[e + 1].first_block) ++e;
    const X6BSplitEntry E = table[e];
    x6b_split_body(E, ((int)blockIdx.x - E.first_block) * blockDim.x + threadIdx.x, blockIdx.y, w, wstride, arena);
}
// one layer by itself (autotuning; a launch outside a pass-wide split): the entry travels as a kernel argument
__global__ void x6b_split_one_kernel(X6BSplitEntry E, const float* w, long long wstride, float* arena)
{
    x6b_split_body(E, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y, w, wstride, arena);
}

template <bool K16, int SR, int NG>
__global__ __launch_bounds__(512, 2) void conv_bwd_x6_kernel(X6BArgs A)
{
    using C = X6BCfg<K16, SR, NG>;
    constexpr int NOCTT = C::NOCTT, PLANE = C::PLANE, PIECE = C::PIECE, ROWB = C::ROWB, NR = C::NR, NV = C::NV, OPB = C::OPB, SUMW = C::SUMW;
    extern __shared__ __align__(16) char lds[];             // ring [NR][3][NOCTT][80][16] | weight pieces [9][NV][64][16] | finished tile [16][OPB] | tables
    char* const s_w = lds + C::RING;
    char* const s_out = s_w + C::WB;
    const ConvGeom& g = A.g;
    const int CI = g.Cin, CO = g.Cout, H = g.H, W = g.W, HW = H * W;
    const int NF = A.NF, NFS = NF * 16;
    BwdC* const s_chb = reinterpret_cast<BwdC*>(s_out + 16 * OPB);                  // [CO]
    ChanFwd* const s_ch = reinterpret_cast<ChanFwd*>(s_chb + CO);                   // [NFS]
    float* const s_sum = reinterpret_cast<float*>(s_ch + NFS);                      // [SUMW][NFS][2]

    const int tid = threadIdx.x;
    const bool producer = tid >= 256;
    const int t = tid & 255, lane = t & 63;
    const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
#ifdef X6B_PROF
    unsigned long long prof[24] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    XB_T(t_entry);
#endif
    int bx, by, k;
    xcd_decode(blockIdx.x, A.nx, 1, A.nz, bx, by, k);
    const int band = bx % A.bands, strip0 = (bx / A.bands) * A.tpb;
    const int n_strip = min(A.tpb, A.strips - strip0);
    const int c0 = band * 64;
    const int n_pps = NF * NG;                              // passes per strip
    const int n_pass = n_strip * n_pps;
    const bool fuse_sums = A.fbsums != nullptr;
    const unsigned* __restrict__ wsp = A.wsp + (long long)k * A.wsp_stride_u4 * 4;

    // ---- staging helpers (all eight waves stage the first window; afterwards only waves 4-7 use them) ----
    const float* __restrict__ gsrc = A.gin.ga + (long long)k * A.gin.gstride;
    // no BatchNorm behind the layer (never the case in skip()): the y loads still run, on ga, against qc = 0 — every load of the staging waves is unconditional
    const float* __restrict__ ysrc = A.gin.stats ? A.gin.y + (long long)k * A.gin.ystride : gsrc;
    const bool lb = c0 == 0, rb = c0 + 64 == W;
    // The SR new rows of a strip are 16 tasks (row j, octet q) of 64 pixels — SR * NOCTT == 16 for every instantiation — four per
    // staging wave (task i of wave w: number w + 4 i), plus one task of the four special pixel slots of this wave's four (row, octet)
    // pairs on lanes 0..15 (pair = lane >> 2, kind = lane & 3: left halo, right halo, left sum dy[2] + dy[0], right sum dy[W-3] + dy[W-1]).
    static_assert(SR * NOCTT == 16, "task geometry");
    const int pair = lane >> 2, kind = lane & 3;
    u32x4 pc[5][3];                                     // finished pieces of the five tasks, waiting for the strip boundary
    int jrow[5], qoct[5];                               // (task 4: per lane)
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int tn = wv + 4 * i; jrow[i] = tn / NOCTT; qoct[i] = tn % NOCTT; }
    { const int tn = wv + 4 * min(pair, 3); jrow[4] = tn / NOCTT; qoct[4] = tn % NOCTT; }
    const bool sp_on = lane < 16 && (kind == 0 ? !lb : kind == 1 ? !rb : kind == 2 ? lb : rb);
    const int colA = kind == 0 ? max(c0 - 1, 0) : kind == 1 ? min(c0 + 64, W - 1) : kind == 2 ? 2 : W - 3;
    const int colB = kind == 2 ? 0 : W - 1;
    const bool two = kind >= 2;
    const int sslot = kind == 0 ? 0 : kind == 1 ? 65 : kind == 2 ? 66 : 67;
    // (32-bit element offsets from a wave-uniform base: with 64-bit per-lane addresses the compiler kept ~100 address registers live)
    const unsigned uHW = (unsigned)HW;
    auto fetch_to = [&](int i, float (&ga)[8], float (&yy)[8], int Rb) {
        const int R = min(max(Rb + jrow[i], 0), H - 1);
        const unsigned off = 4u * ((unsigned)(8 * qoct[i]) * uHW + (unsigned)(R * W + c0) + (unsigned)lane);
#pragma unroll
        for (int j = 0; j < 8; ++j) { ga[j] = ldg_f(gsrc, off + 4u * (unsigned)j * uHW); yy[j] = ldg_f(ysrc, off + 4u * (unsigned)j * uHW); }
    };
    auto fetch_sp_to = [&](float (&ga)[8], float (&ya)[8], float (&gb)[8], float (&yb)[8], int Rb) {
        const int R = min(max(Rb + jrow[4], 0), H - 1);
        const unsigned base = (unsigned)(8 * qoct[4]) * uHW + (unsigned)(R * W);
        const unsigned oa = 4u * (base + (unsigned)colA), ob = 4u * (base + (unsigned)colB);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            ga[j] = ldg_f(gsrc, oa + 4u * (unsigned)j * uHW); ya[j] = ldg_f(ysrc, oa + 4u * (unsigned)j * uHW);
            gb[j] = ldg_f(gsrc, ob + 4u * (unsigned)j * uHW); yb[j] = ldg_f(ysrc, ob + 4u * (unsigned)j * uHW);
        }
    };
    auto finish_from = [&](int i, const float (&ga)[8], const float (&yy)[8], int Rb) {
        const int R = Rb + jrow[i];
        float e[8];
        int qi = __builtin_amdgcn_readfirstlane(8 * qoct[i]); asm volatile("" : "+s"(qi));      // opaque: the loop-invariant table reads are NOT hoisted over the strip loop
#pragma unroll
        for (int j = 0; j < 8; ++j) { const BwdC b = s_chb[qi + j]; e[j] = __builtin_fmaf(ga[j], b.c1, __builtin_fmaf(yy[j], b.qc, b.k3)); }
        if (R < 0 || R >= H) {
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = 0.f;
        }
        split8(e, pc[i][0], pc[i][1], pc[i][2]);
    };
    auto finish_sp_from = [&](const float (&ga)[8], const float (&ya)[8], const float (&gb)[8], const float (&yb)[8], int Rb) {
        const int R = Rb + jrow[4];
        float e[8];
        int qi = 8 * qoct[4]; asm volatile("" : "+v"(qi));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const BwdC b = s_chb[qi + j];
            const float a = __builtin_fmaf(ga[j], b.c1, __builtin_fmaf(ya[j], b.qc, b.k3));
            const float c = __builtin_fmaf(gb[j], b.c1, __builtin_fmaf(yb[j], b.qc, b.k3));
            e[j] = two ? a + c : a;
        }
        if (!sp_on || R < 0 || R >= H) {
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = 0.f;
        }
        split8(e, pc[4][0], pc[4][1], pc[4][2]);
    };
    // write the five tasks' pieces into the ring rows of image rows Rb .. Rb + nvalid - 1 (ring slot of image row R: (R + 1) mod NR)
    auto write = [&](int Rb, int nvalid) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            if (jrow[i] >= nvalid) continue;
            if (i == 4 && lane >= 16) continue;
            const int slot = (Rb + jrow[i] + 1 + NR) % NR;
            char* d = lds + slot * ROWB + qoct[i] * PLANE + (i == 4 ? sslot : 1 + lane) * 16;
            *reinterpret_cast<u32x4*>(d) = pc[i][0]; *reinterpret_cast<u32x4*>(d + PIECE) = pc[i][1]; *reinterpret_cast<u32x4*>(d + 2 * PIECE) = pc[i][2];
        }
    };
    // weight pieces of pass p (fragment p / NG % NF, group p % NG): WB contiguous bytes
    u32x4 wq[C::NWU];
    auto wfetch = [&](int p) {
        const int fg = p % n_pps;
        const u32x4* __restrict__ src = reinterpret_cast<const u32x4*>(wsp) + (long long)fg * (C::WB / 16);
#pragma unroll
        for (int j = 0; j < C::NWU; ++j) wq[j] = src[min(t + 256 * j, C::WB / 16 - 1)];
    };
    auto wstore = [&]() {
#pragma unroll
        for (int j = 0; j < C::NWU; ++j) if (t + 256 * j < C::WB / 16) *reinterpret_cast<u32x4*>(s_w + (t + 256 * j) * 16) = wq[j];
    };

    // Prologue, part 1: the first strip's window (image rows r0 - 1 .. r0 + SR) is staged by ALL eight waves — waves 4-7 its first SR
    // rows, waves 0-3 the last two — and every global load of it is issued before anything waits, the channel tables included: one
    // memory round trip (first version: seven, 26 k cycles per block).
    const int pro_rd = producer ? 0 : 1;
    const int pro_Rb = strip0 * SR - 1 + pro_rd * SR, pro_nvalid = pro_rd == 0 ? SR : 2;
    float pg[6][8], py[6][8];
#pragma unroll
    for (int i = 0; i < 4; ++i) if (pro_rd == 0 || jrow[i] < 2) fetch_to(i, pg[i], py[i], pro_Rb);
    fetch_sp_to(pg[4], py[4], pg[5], py[5], pro_Rb);
    if (producer) wfetch(0);

    if (!producer) {
        for (int c = t; c < CO; c += 256) { const ChanBwd b = chan_bwd(A.gin, k, c); BwdC r; r.qc = -b.c1 * b.c3 * b.rstd; r.c1 = b.c1; r.k3 = __builtin_fmaf(-b.mean, r.qc, -b.c1 * b.c2); r.pad = 0.f; s_chb[c] = r; }
        for (int c = t; c < NFS; c += 256) { ChanFwd f; if (fuse_sums) f = chan_fwd(A.xin, k, min(c, CI - 1)); else { f.mean = 0.f; f.scale = 1.f; f.beta = 0.f; f.rstd = 1.f; } s_ch[c] = f; }
        for (int i = t; i < SUMW * NFS * 2; i += 256) s_sum[i] = 0.f;
    }

    XB_T(sp0); XB_ACC(19, sp0 - t_entry);                                       // prologue: loads issued, tables built
    __syncthreads();                                        // (S0) channel tables visible
    XB_T(sp1); XB_ACC(20, sp1 - sp0);                                           // prologue: wait at S0
#pragma unroll
    for (int i = 0; i < 4; ++i) if (pro_rd == 0 || jrow[i] < 2) finish_from(i, pg[i], py[i], pro_Rb);
    finish_sp_from(pg[4], py[4], pg[5], py[5], pro_Rb);
    write(pro_Rb, pro_nvalid);
    XB_T(sp2); XB_ACC(21, sp2 - sp1);                                           // prologue: transform + split + write

#ifdef X6B_DBG_NOPROD
    if (false) {
#else
    if (producer) {
#endif
        // ======================= staging waves =======================
        __builtin_amdgcn_s_setprio(X6B_PRIO_S);
        // The staging of the next strip's SR rows rides on the strip's passes in PHASES: a phase first consumes (BN-backward, split) what the
        // phase before requested, then requests its own loads.  Four phases on two raw register sets; the 16-output-channel layers have only
        // three passes per strip (three input-channel fragments), so they run three phases on three sets (a consume right behind its own
        // request would expose a memory round trip every strip).
        //
        // Control flow (round 4, found on conv_bwd_x6s.hip): the compiler's s_waitcnt insertion counts the younger memory operations of the
        // path it is on; a run-time branch around a group of loads ("if (more)", "if (ph == ps)", the per-load "ysrc ? load : 0", the fold's
        // activation variant) makes every later consumer wait for vmcnt(0) — an exposed memory round trip.  So: the fold variant is chosen
        // once around the whole loop, a strip's first NPH passes are written out with their phase as a compile-time constant (when the strip
        // has that many passes; fewer: the old run-time form), "a next strip exists" is a compile-time flag of the strip, every load is
        // unconditional (clamped addresses where a lane or the last weight copy has nothing to fetch).
        constexpr int NSET = K16 ? 3 : 2, NPH = K16 ? 3 : 4;
        constexpr int NIT = SR;                             // items (tile rows) per thread
        const bool xact = (A.xin.act & 1) != 0; const float xslope = A.xin.slope;
        const float* __restrict__ xq = A.xin.data + (long long)k * A.xin.sstride;
        float* __restrict__ gout = A.fga + (long long)k * A.fga_sstride;
        const int fchl = t >> 4, fv = t & 15;
        auto run = [&](auto sums_c, auto act_c) {
            constexpr bool SUMS = decltype(sums_c)::value;
            float ga_[NSET][8], y_[NSET][8];
            auto phase_consume = [&](auto ph_c, int Rb) {
                constexpr int ph = decltype(ph_c)::value;
                Rb = __builtin_amdgcn_readfirstlane(Rb); asm volatile("" : "+s"(Rb));      // opaque: per-load offsets are recomputed where they are used, not hoisted out of the pass loop (~100 registers)
                if constexpr (K16) {
                    if constexpr (ph == 1) { finish_from(0, ga_[0], y_[0], Rb); finish_from(1, ga_[1], y_[1], Rb); finish_from(2, ga_[2], y_[2], Rb); }
                    else if constexpr (ph == 2) { finish_from(3, ga_[0], y_[0], Rb); finish_sp_from(ga_[1], y_[1], ga_[2], y_[2], Rb); }
                } else {
                    if constexpr (ph == 1) { finish_from(0, ga_[0], y_[0], Rb); finish_from(1, ga_[1], y_[1], Rb); }
                    else if constexpr (ph == 2) { finish_from(2, ga_[0], y_[0], Rb); finish_from(3, ga_[1], y_[1], Rb); }
                    else if constexpr (ph == 3) finish_sp_from(ga_[0], y_[0], ga_[1], y_[1], Rb);
                }
            };
            auto phase_request = [&](auto ph_c, int Rb) {
                constexpr int ph = decltype(ph_c)::value;
                Rb = __builtin_amdgcn_readfirstlane(Rb); asm volatile("" : "+s"(Rb));
                if constexpr (K16) {
                    if constexpr (ph == 0) { fetch_to(0, ga_[0], y_[0], Rb); fetch_to(1, ga_[1], y_[1], Rb); fetch_to(2, ga_[2], y_[2], Rb); }
                    else if constexpr (ph == 1) { fetch_to(3, ga_[0], y_[0], Rb); fetch_sp_to(ga_[1], y_[1], ga_[2], y_[2], Rb); }
                } else {
                    if constexpr (ph == 0) { fetch_to(0, ga_[0], y_[0], Rb); fetch_to(1, ga_[1], y_[1], Rb); }
                    else if constexpr (ph == 1) { fetch_to(2, ga_[0], y_[0], Rb); fetch_to(3, ga_[1], y_[1], Rb); }
                    else if constexpr (ph == 2) fetch_sp_to(ga_[0], y_[0], ga_[1], y_[1], Rb);
                }
            };
            // ---- the fold of a finished tile (fragment f of the strip at image row r0), dumped into s_out by the matrix waves at the head of the
            //      pass after the one that finished it.  Thread t owns channel t >> 4 of the fragment and float4 column t & 15 of every tile row:
            //      16 lanes = one 256-byte row of one channel in every global access, and a thread's SR items share their channel — its two
            //      BN-backward sums stay in registers over the tile and cost ONE 16-lane DPP reduction per pass (first version: a wave-wide
            //      ds_bpermute reduction per item, 13 k cycles per pass).
            float4 xpre[NIT] = {};                          // raw x of the pending fold, requested one pass ahead
            auto xprefetch = [&](int r0, int f) {
#ifdef X6B_DBG_NOFOLDLD
                return;
#endif
                if constexpr (SUMS) {
                    r0 = __builtin_amdgcn_readfirstlane(r0); asm volatile("" : "+s"(r0));
                    const int ch = min(16 * f + fchl, CI - 1);      // (a padded channel reads the last real one: every lane loads, nothing is stored for it)
                    const unsigned off = 4u * ((unsigned)ch * uHW + (unsigned)(r0 * W + c0 + 4 * fv));
#pragma unroll
                    for (int j = 0; j < NIT; ++j) xpre[j] = ldg_f4(xq, off + 4u * (unsigned)(j * W));
                }
            };
            auto fold = [&](int r0, int f) {
                r0 = __builtin_amdgcn_readfirstlane(r0); asm volatile("" : "+s"(r0));
                const int ch = 16 * f + fchl;
                const unsigned off = 4u * ((unsigned)ch * uHW + (unsigned)(r0 * W + c0 + 4 * fv));
                const char* so = s_out + fchl * OPB + fv * 16;
                const ChanFwd cf = s_ch[ch];
                float fs = 0.f, fx = 0.f;
                constexpr int CH = NIT < 4 ? NIT : 4;       // items in flight (registers: NIT = 8 tile rows at once spilled)
#pragma unroll
                for (int j0 = 0; j0 < NIT; j0 += CH) {
                    float4 d4[CH];
#pragma unroll
                    for (int j = 0; j < CH; ++j) d4[j] = *reinterpret_cast<const float4*>(so + (j0 + j) * 256);
#pragma unroll
                    for (int jj = 0; jj < CH; ++jj) {
                        const int j = j0 + jj;
                        float dd[4] = {d4[jj].x, d4[jj].y, d4[jj].z, d4[jj].w};
                        if constexpr (SUMS) {
                            const float yy[4] = {xpre[j].x, xpre[j].y, xpre[j].z, xpre[j].w};
                            float ymv[4];
#pragma unroll
                            for (int l = 0; l < 4; ++l)
                                ymv[l] = yy[l] - cf.mean;
                            if (xact) {     // wave-uniform branch around vector arithmetic ONLY (no memory operation inside: the waitcnt bookkeeping stays exact)
#pragma unroll
                                for (int l = 0; l < 4; ++l) { const float vv = __builtin_fmaf(ymv[l], cf.scale, cf.beta); dd[l] *= (vv > 0.f) ? 1.f : xslope; }
                            }
#pragma unroll
                            for (int l = 0; l < 4; ++l) { fs += dd[l]; fx = __builtin_fmaf(dd[l], ymv[l], fx); }      // (views without an activation — the concat tensors of the skip() nets — three operations per element)
                        }
#ifdef X6B_DBG_NOFOLDST
                        if (ch < CI && dd[0] == 1.2345f)
#else
                        if (ch < CI)
#endif
                            stg_f4(gout, off + 4u * (unsigned)(j * W), make_float4(dd[0], dd[1], dd[2], dd[3]));
                    }
                }
                if constexpr (SUMS) {
                    // sums over the channel's 16 lanes on the DPP path (v += row_shr(v) by 1, 2, 4, 8: the total lands in lane 15 of the row)
                    fs = row_sum16(fs); fx = row_sum16(fx);
                    if (fv == 15 && ch < CI) { float* sp = s_sum + ch * 2; sp[0] += fs; sp[1] += fx; }      // one owner per channel: no atomics
                }
            };

            wstore();
            XB_T(s_pro); XB_ACC(12, s_pro - t_entry);
            lds_barrier();                                  // (B1) window of strip 0 and W(0) published
            int p = 0;
            bool pend = false; int pend_r0 = 0, pend_f = 0; // a finished tile waits in the matrix waves' registers / s_out
            // One pass.  PS: the pass's index in its strip when its staging phase is a compile-time constant, -1: no phase (passes >= NPH);
            // LASTG: the pass finishes its fragment (group NG - 1); MORE: a next strip exists.
            // Order inside a pass: everything that CONSUMES loads of the pass before (the fold: raw x; the phase: dy rows), then everything
            // that REQUESTS (raw x of the tile this pass finishes, the phase's next rows) — vmcnt retires in order, so a consumer behind a
            // fresh request would wait for that request as well
            auto pass = [&](auto ps_c, auto lastg_c, auto more_c, int r0, int Rb, int f) {
                constexpr int PS = decltype(ps_c)::value; constexpr bool LASTG = decltype(lastg_c)::value, MORE = decltype(more_c)::value;
                XB_T(s0);
#ifndef X6B_DBG_NOWCOPY
                wfetch(min(p + 1, n_pass - 1));             // (the block's last pass fetches its own pieces again: no branch around the loads)
#endif
                lds_barrier();                              // (B2) the matrix waves hold W(p) in registers; a pending tile is in s_out
                XB_T(s1); XB_ACC(13, s1 - s0);                                  // wait at B2
#ifndef X6B_DBG_NOWCOPY
                wstore();
#endif
                XB_T(s2); XB_ACC(14, s2 - s1);                                  // weight copy (waits for its loads)
                if (pend) { fold(pend_r0, pend_f); pend = false; }
                XB_T(s2b); XB_ACC(18, s2b - s2);                                // fold of the previous tile
#ifndef X6B_DBG_NOSTAGE
                if constexpr (MORE && PS >= 1 && PS < NPH) phase_consume(std::integral_constant<int, (PS >= 1 ? PS : 1)>{}, Rb);
#endif
                if constexpr (LASTG) { pend = true; pend_r0 = r0; pend_f = f; xprefetch(r0, f); }      // this pass finishes fragment f
#ifndef X6B_DBG_NOSTAGE
                if constexpr (MORE && PS >= 0 && PS < NPH - 1) phase_request(std::integral_constant<int, (PS >= 0 ? PS : 0)>{}, Rb);
#endif
                XB_T(s3); XB_ACC(15, s3 - s2b);                                 // staging phase of this pass
                lds_barrier();                              // (B1) W(p + 1) published; the matrix waves are done with pass p
                XB_T(s4); XB_ACC(16, s4 - s3);                                  // wait at B1
                ++p;
            };
            // a strip whose passes number at least NPH: passes 0 .. NPH - 1 written out, the rest in a loop over fragments
            auto strip_static = [&](int ts, auto more_c) {
                constexpr bool MORE = decltype(more_c)::value;
                const int r0 = (strip0 + ts) * SR, Rb = r0 + SR + 1;      // Rb: first NEW image row of the next strip's window
                using T = std::true_type; using F = std::false_type;
                if constexpr (NG == 1) {
                    pass(std::integral_constant<int, 0>{}, T{}, more_c, r0, Rb, 0);
                    pass(std::integral_constant<int, 1>{}, T{}, more_c, r0, Rb, 1);
                    pass(std::integral_constant<int, 2>{}, T{}, more_c, r0, Rb, 2);
                    if constexpr (NPH == 4) pass(std::integral_constant<int, 3>{}, T{}, more_c, r0, Rb, 3);
#pragma unroll 1
                    for (int f = NPH; f < NF; ++f) pass(std::integral_constant<int, -1>{}, T{}, more_c, r0, Rb, f);
                } else {
                    static_assert(NG == 2 && NPH == 4, "two groups: four phases on the first two fragments");
                    pass(std::integral_constant<int, 0>{}, F{}, more_c, r0, Rb, 0);
                    pass(std::integral_constant<int, 1>{}, T{}, more_c, r0, Rb, 0);
                    pass(std::integral_constant<int, 2>{}, F{}, more_c, r0, Rb, 1);
                    pass(std::integral_constant<int, 3>{}, T{}, more_c, r0, Rb, 1);
#pragma unroll 1
                    for (int f = 2; f < NF; ++f) { pass(std::integral_constant<int, -1>{}, F{}, more_c, r0, Rb, f); pass(std::integral_constant<int, -1>{}, T{}, more_c, r0, Rb, f); }
                }
                XB_T(s5);
                if constexpr (MORE) { write(Rb, SR); lds_barrier(); }     // (B3) next strip's window published
                XB_T(s6); XB_ACC(17, s6 - s5);
            };
            // a strip with fewer passes than phases (one or two input-channel fragments): phases by run-time index, the rest one after the other
            auto strip_dynamic = [&](int ts) {
                const bool more = ts + 1 < n_strip;
                const int r0 = (strip0 + ts) * SR, Rb = r0 + SR + 1;
#pragma unroll 1
                for (int ps = 0; ps < n_pps; ++ps, ++p) {
                    wfetch(min(p + 1, n_pass - 1));
                    lds_barrier();                          // (B2)
                    wstore();
                    if (pend) { fold(pend_r0, pend_f); pend = false; }
                    if (more) {
                        if (ps == 1) phase_consume(std::integral_constant<int, 1>{}, Rb);
                        if (ps == 2) phase_consume(std::integral_constant<int, 2>{}, Rb);
                        if (NPH == 4 && ps == 3) phase_consume(std::integral_constant<int, (NPH == 4 ? 3 : 1)>{}, Rb);
                    }
                    if (ps % NG == NG - 1) { pend = true; pend_r0 = r0; pend_f = ps / NG; xprefetch(r0, pend_f); }
                    if (more) {
                        if (ps == 0) phase_request(std::integral_constant<int, 0>{}, Rb);
                        if (ps == 1) phase_request(std::integral_constant<int, 1>{}, Rb);
                        if (NPH == 4 && ps == 2) phase_request(std::integral_constant<int, (NPH == 4 ? 2 : 0)>{}, Rb);
                        if (ps == n_pps - 1) {      // the remaining phases one after the other (each consume waits for its own request)
                            if (ps < 1) { phase_consume(std::integral_constant<int, 1>{}, Rb); phase_request(std::integral_constant<int, 1>{}, Rb); }
                            if (ps < 2) { phase_consume(std::integral_constant<int, 2>{}, Rb); if constexpr (NPH == 4) phase_request(std::integral_constant<int, (NPH == 4 ? 2 : 0)>{}, Rb); }
                            if constexpr (NPH == 4) { if (ps < 3) phase_consume(std::integral_constant<int, (NPH == 4 ? 3 : 1)>{}, Rb); }
                        }
                    }
                    lds_barrier();                          // (B1)
                }
                if (more) { write(Rb, SR); lds_barrier(); }     // (B3)
            };
            if (n_pps >= NPH) {
#pragma unroll 1
                for (int ts = 0; ts + 1 < n_strip; ++ts) strip_static(ts, std::true_type{});
                strip_static(n_strip - 1, std::false_type{});
            } else {
#pragma unroll 1
                for (int ts = 0; ts < n_strip; ++ts) strip_dynamic(ts);
            }
            lds_barrier();                                  // (BF) the last tile is in s_out
            if (pend) fold(pend_r0, pend_f);
        };
#ifdef X6B_DBG_NOPROD
#else
        // ONE variant: the raw x is loaded and the sums are formed even when the input carries no BatchNorm (never the case on this path in
        // skip(): identity constants, the sums are not written); three variants around the loop made the compiler hoist their common
        // address arithmetic in front of the dispatch and spill
        run(std::true_type{}, std::true_type{});
#endif
#ifdef X6B_PROF
        if (t == 0) { for (int i = 12; i < 24; ++i) atomicAdd(&g_x6b_prof[i], prof[i]); atomicAdd(&g_x6b_prof[10], prof[10]); atomicAdd(&g_x6b_prof[11], prof[11]); }
#endif
        if (fuse_sums) __syncthreads();                     // (Z)
#ifdef X6B_DBG_NOMAT
    } else if (false) {
#else
    } else {
#endif
        // ======================= matrix waves: wave = 16-pixel fragment =======================
        __builtin_amdgcn_s_setprio(X6B_PRIO_M);
        const int pf = wv;
        const bool lb = c0 == 0, rbd = c0 + 64 == W;
        int ax[3], axl[3];                                  // byte offsets of this lane's pixel operand inside a ring row, per kx
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            int sl = 16 * pf + l15 + 2 - kx;
            if (lb && pf == 0 && l15 == 1 && kx == 0) sl = 66;
            if (rbd && pf == 3 && l15 == 14 && kx == 2) sl = 67;
            ax[kx] = (K16 ? (l4 & 1) : l4) * PLANE + sl * 16;
            axl[kx] = ax[kx] + (l4 >= 2 ? 2 * PIECE : 0);   // K16: [x_h | x_l]
        }
        const char* const swl = s_w + lane * 16;            // ((l15 * 4 + l4) * 16, conv_x6.hip's order, is a 2-way bank conflict: lanes l15 and l15 + 4 share banks)
        char* const so = s_out + l15 * OPB + (16 * pf + 4 * l4) * 4;      // register r of acc[o] = pixel 16 pf + 4 l4 + r of channel l15, tile row o
        f32x4 acc[SR];
        bool dump = false;
        auto dump_tile = [&]() {
#pragma unroll
            for (int o = 0; o < SR; ++o) *reinterpret_cast<f32x4*>(so + o * 256) = acc[o];
        };
        lds_barrier();                                      // (B1)
        XB_T(m_pro); XB_ACC(0, m_pro - t_entry);
#pragma unroll 1
        for (int ts = 0; ts < n_strip; ++ts) {
            const int r0 = (strip0 + ts) * SR;
            const bool first = r0 == 0, last = r0 + SR == H;
            int ro[SR + 2];                                 // ring row offsets of the window rows (image rows r0 - 1 + ii)
            { const int b0 = r0 % NR;
#pragma unroll
              for (int ii = 0; ii < SR + 2; ++ii) { int s = b0 + ii; s = s >= NR ? s - NR : s; ro[ii] = s * ROWB; } }
#pragma unroll 1
            for (int f = 0; f < NF; ++f) {
#pragma unroll 1
                for (int grp = 0; grp < NG; ++grp) {
                    XB_T(m0);
                    if (dump) { dump_tile(); dump = false; }      // the tile finished by the previous pass: the staging waves fold it during this pass
                    u32x4 Wr[9][NV];
#pragma unroll
                    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
                        for (int v = 0; v < NV; ++v) Wr[tp][v] = *reinterpret_cast<const u32x4*>(swl + (tp * NV + v) * 1024);
#ifdef X6B_PROF
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
                    XB_T(m1); XB_ACC(1, m1 - m0);                               // tile dump + weight reads
                    lds_barrier();                          // (B2) W in registers, tile in s_out
                    XB_T(m2); XB_ACC(2, m2 - m1);                               // wait at B2
                    if (grp == 0) {
#pragma unroll
                        for (int o = 0; o < SR; ++o) acc[o] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    }
                    const int goff = grp * 4 * PLANE;
                    constexpr int NGRP = (SR + 2) * 3;
                    u32x4 X[2][3];
                    auto issue = [&](int gi, u32x4 (&x)[3]) {
                        const int ii = gi / 3, kx = gi - 3 * ii;
#ifdef X6B_DBG_NOXREAD
                        if (ii >= 0) { x[0] = (u32x4){1u, 2u, 3u, (unsigned)gi}; x[1] = x[0]; x[2] = x[0]; return; }
#endif
                        if constexpr (K16) {
                            const char* p = lds + ro[ii] + ax[kx];
                            x[0] = *reinterpret_cast<const u32x4*>(p);                           // [x_h | x_h]
                            x[1] = *reinterpret_cast<const u32x4*>(p + PIECE);                   // [x_m | x_m]
                            x[2] = *reinterpret_cast<const u32x4*>(lds + ro[ii] + axl[kx]);      // [x_h | x_l]
                        } else {
                            const char* p = lds + ro[ii] + ax[kx] + goff;
#pragma unroll
                            for (int pc = 0; pc < 3; ++pc) x[pc] = *reinterpret_cast<const u32x4*>(p + pc * PIECE);
                        }
                    };
                    // products of one (x, w) operand pair of a tap, small terms first: K16 ([x_h|x_l].[w_l|w_h], [x_m|x_m].[w_h|w_m], [x_h|x_h].[w_h|w_m]);
                    // otherwise pieces (x, w): (l,h), (h,l), (m,m), (m,h), (h,m), (h,h)
                    constexpr int NQ = K16 ? 3 : 6;
                    constexpr int QX[6] = {2, K16 ? 1 : 0, K16 ? 0 : 1, 1, 0, 0}, QW[6] = {K16 ? 1 : 0, K16 ? 0 : 2, K16 ? 0 : 1, 0, 1, 0};
                    issue(0, X[0]);
#pragma unroll
                    for (int gi = 0; gi < NGRP; ++gi) {
                        const int ii = gi / 3, kx = gi - 3 * ii;
                        __builtin_amdgcn_sched_barrier(0);
                        if (gi + 1 < NGRP) issue(gi + 1, X[(gi + 1) & 1]);
                        __builtin_amdgcn_sched_barrier(0);
                        const u32x4 (&x)[3] = X[gi & 1];
#ifdef X6B_DBG_NOMFMA
                        if (ii >= 0) continue;
#endif
                        // image row r0 - 1 + ii meets output row o = ii + ky - 2 through tap row ky; the product loop is OUTSIDE the tap-row loop so
                        // that consecutive matrix instructions accumulate into different rows' registers
#pragma unroll
                        for (int q = 0; q < NQ; ++q)
#pragma unroll
                            for (int ky = 0; ky < 3; ++ky) {
                                const int o = ii + ky - 2;
                                if (o >= 0 && o < SR) acc[o] = mfma_bf(x[QX[q]], Wr[ky * 3 + kx][QW[q]], acc[o]);
                            }
                        if (ii == 1 && first) {             // image row 0 -> padded row -1 -> row 1 (tap row 0)
#pragma unroll
                            for (int q = 0; q < NQ; ++q) acc[1] = mfma_bf(x[QX[q]], Wr[kx][QW[q]], acc[1]);
                        }
                        if (ii == SR && last) {             // image row H-1 -> padded row H -> row H-2 (tap row 2)
#pragma unroll
                            for (int q = 0; q < NQ; ++q) acc[SR - 2] = mfma_bf(x[QX[q]], Wr[6 + kx][QW[q]], acc[SR - 2]);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    XB_T(m3); XB_ACC(3, m3 - m2);                               // rows (issue time)
                    if (grp == NG - 1) dump = true;
                    lds_barrier();                          // (B1)
                    XB_T(m5); XB_ACC(5, m5 - m3); XB_ACC(7, 1);                 // wait at B1; passes
                }
            }
            XB_T(m6);
            if (ts + 1 < n_strip) lds_barrier();            // (B3)
            XB_T(m7); XB_ACC(6, m7 - m6);
        }
        if (dump) dump_tile();
        lds_barrier();                                      // (BF)
#ifdef X6B_PROF
        if (t == 0) { for (int i = 0; i < 8; ++i) atomicAdd(&g_x6b_prof[i], prof[i]); atomicAdd(&g_x6b_prof[8], 1ull); atomicAdd(&g_x6b_prof[9], xb_now() - t_entry); }
#endif
        if (fuse_sums) __syncthreads();                     // (Z)
    }
    if (fuse_sums) {
        for (int i = tid; i < NFS * 2; i += 512) {
            const int q = i >> 1, which = i & 1;
            if (q < CI) {
                float v = s_sum[q * 2 + which];
#pragma unroll
                for (int w2 = 1; w2 < SUMW; ++w2) v += s_sum[(w2 * NFS + q) * 2 + which];
                if (which) v *= s_ch[q].rstd;
                atomicAdd(A.fbsums + ((long long)k * CI + q) * 2 + which, (double)v);
            }
        }
    }
}

template <bool K16, int SR, int NG>
int launch_one(X6BArgs& A, Launch& L)
{
    using C = X6BCfg<K16, SR, NG>;
    const size_t lds_bytes = (size_t)C::RING + C::WB + 16 * C::OPB + sizeof(BwdC) * A.g.Cout + sizeof(ChanFwd) * A.NF * 16 + sizeof(float) * C::SUMW * A.NF * 16 * 2;
    if (lds_bytes > 160 * 1024) return CONV_BAD_TILING;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(conv_bwd_x6_kernel<K16, SR, NG>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (attr != hipSuccess) return (int)attr;
    L.family = FAM_BF16X6;
    mfvi_launch(L, (conv_bwd_x6_kernel<K16, SR, NG>), dim3(A.nx * A.nz), dim3(512), lds_bytes, A);
    return (int)hipGetLastError();
}

bool x6b_shape_ok(const ConvGeom& g)
{
    return g.ks == 3 && g.stride == 1 && !(g.W & 63) && g.H >= 4 && (g.Cout == 16 || g.Cout == 32 || g.Cout == 64) && g.Cin >= 4 && g.Cin <= MFVI_MAX_C && !(g.w_off & 3);
}

}  // namespace

// floats of split weight pieces for n_samples samples (0: shape not served)
long long x6_bwd_scratch_floats(const ConvGeom& g, int n_samples)
{
    if (!x6b_shape_ok(g)) return 0;
    const int NF = (g.Cin + 15) / 16, NG = g.Cout == 64 ? 2 : 1, NV = g.Cout == 16 ? 2 : 3;
    return ((long long)NF * NG * 9 * NV * 256 + (g.Cout == 16 && g.Cin == 36 ? 192 * NV * 4 : 0)) * n_samples;
}

bool x6b_split_entry(const ConvGeom& g, long long dst_off, X6BSplitEntry* e)
{
    if (!x6b_shape_ok(g)) return false;
    e->w_off = g.w_off; e->dst_off = dst_off; e->CI = g.Cin; e->CO = g.Cout; e->NF = (g.Cin + 15) / 16; e->NG = g.Cout == 64 ? 2 : 1;
    e->k16 = g.Cout == 16 ? 1 : 0; e->units = e->NF * e->NG * 9 * 64; e->first_block = 0; e->rem_units = (g.Cout == 16 && g.Cin == 36) ? 192 : 0;
    return true;
}

int launch_x6b_split_all(const X6BSplitEntry* table_dev, int n_entries, int n_blocks, const float* w, long long wstride, int n_k, float* arena, hipStream_t st)
{
    if (n_entries <= 0 || n_blocks <= 0) return 0;
    hipLaunchKernelGGL(x6b_split_kernel, dim3(n_blocks, n_k), dim3(256), 0, st, table_dev, n_entries, w, wstride, arena);
    return (int)hipGetLastError();
}

// tune: T | sr << 8 (strips per block, output rows per strip; MFVI_TUNE_X6 stripped by the caller).  -2: shape not served / no scratch, -3: tiling not valid.
int launch_conv_bwd_data_x6(const GView& gy, const ConvGeom& g, const float* w, long long wstride, int tune, int n_samples, Launch& L, const FoldFuse& fuse)
{
    float* scratch = L.x6_scratch;
    if (!scratch || !x6b_shape_ok(g)) return CONV_NOT_SERVED;
    if (!fuse.ga || (fuse.ga_sstride & 3) || ((uintptr_t)fuse.ga & 15)) return CONV_NOT_SERVED;
    if ((fuse.x.sstride & 3) || ((uintptr_t)fuse.x.data & 15)) return CONV_NOT_SERVED;      // (the raw x is read as float4 whether or not it carries a BatchNorm)
    if ((long long)max(g.Cin, g.Cout) * g.H * g.W >= (1LL << 29)) return CONV_NOT_SERVED;      // 32-bit element offsets per sample
    const int T = max(1, tune & 255), sr = (tune >> 8) & 255;
    const int want_sr = g.Cout == 16 ? 8 : g.Cout == 32 ? 4 : 2;          // SR * octets == 16 (the staging waves' task geometry)
    if (sr != want_sr || (g.H % sr)) return CONV_BAD_TILING;
    X6BSplitEntry E;
    if (!x6b_split_entry(g, 0, &E)) return CONV_NOT_SERVED;
    const int NV = E.k16 ? 2 : 3;
    const int n_k = wstride ? n_samples : 1;
    if (!L.x6_ready) {      // no pass-wide split ran: this layer's own launch (dst_off 0: `scratch` is the layer's region)
        E.dst_off = 0;
        hipLaunchKernelGGL(x6b_split_one_kernel, dim3((E.units + E.rem_units + 255) / 256, n_k), dim3(256), 0, L.st, E, w, wstride, scratch);
    }
    X6BArgs A{};
    A.gin = gy; A.xin = fuse.x; A.g = g;
    A.wsp = reinterpret_cast<const unsigned*>(scratch); A.wsp_stride_u4 = wstride ? (long long)(E.units + E.rem_units) * NV : 0;
    if (tune & (1 << 16))      // strip-resident form (conv_bwd_x6s.hip)
        return launch_conv_bwd_data_x6s(gy, g, A.wsp, A.wsp_stride_u4, E.units * NV, T, n_samples, L, fuse);
    A.fga = fuse.ga; A.fga_sstride = fuse.ga_sstride; A.fbsums = fuse.bsums;
    A.NF = E.NF; A.bands = g.W / 64; A.strips = g.H / sr; A.tpb = T;
    A.nx = A.bands * ((A.strips + T - 1) / T); A.nz = n_samples;
    if (g.Cout == 16) return launch_one<true, 8, 1>(A, L);
    if (g.Cout == 32) return launch_one<false, 4, 1>(A, L);
    return launch_one<false, 2, 2>(A, L);
}

#ifdef X6B_PROF
extern "C" int mfvi_debug_x6b_prof(unsigned long long* out24, int reset)
{
    hipError_t e = hipMemcpyFromSymbol(out24, HIP_SYMBOL(g_x6b_prof), sizeof(unsigned long long) * 24);
    if (e == hipSuccess && reset) { unsigned long long z[24] = {0}; e = hipMemcpyToSymbol(HIP_SYMBOL(g_x6b_prof), z, sizeof(z)); }
    return (int)e;
}
#endif
