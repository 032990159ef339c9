// Per-thread bodies of the element-wise kernels of one ELBO iteration (losses.hip), shared with the kernels that run the same pass for
// many independent fits in one launch (fits.hip): the arithmetic of a fit in a batch is the single-fit arithmetic by construction.
#pragma once
#include "common.h"
#include "../../include/mfvi_hip.h"

// blocks of 256 threads over n elements, capped (the kernels stride over the rest)
inline int nblocks(long long n, int cap = 2048) { long long b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > cap ? cap : b)); }
// the grid cap of every fused KL + Adam launch, single fit or one row of a batch: the same blocks, so the same KL partial sums in the same order
constexpr int ELBO_UPDATE_MAX_BLOCKS = 2048;

__device__ __forceinline__ void block_atomic_add(double v, double* dst, double* red)
{
    const double s = block_sum_d(v, red);
    if (threadIdx.x == 0) atomicAdd(dst, s);
}

// ---- gaussian_nll (utils/bayesian_utils.py:29-32) of ONE sample o[2][H][W] against target[H/f][W/f]: this thread's share of the sum over the
// pixels (grid x strides over them) and, with d, the gradient d[2][H][W] ----
__device__ __forceinline__ double gnll_sample(const float* __restrict__ o, const float* __restrict__ target, int H, int W, int f, float grad_scale,
                                              float* __restrict__ d)
{
    const int h = H / f, w = W / f;
    const long long n = (long long)h * w, HW = (long long)H * W;
    double acc = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int y = (int)(i / w), x = (int)(i - (long long)y * w);
        const long long p = (long long)(y * f) * W + (long long)x * f;
        const float m = o[p], sraw = o[HW + p];
        const float s = fminf(fmaxf(sraw, -20.f), 20.f);
        const bool inside = (sraw >= -20.f) && (sraw <= 20.f);
        const float df = target[i] - m, e = expf(s);
        acc += (double)(e * df * df - s);
        if (d) {
            d[p] = grad_scale * (-2.f * e * df) / (float)n;
            d[HW + p] = inside ? grad_scale * (e * df * df - 1.f) / (float)n : 0.f;
        }
    }
    return acc / (double)n;
}
// factor 1, W % 4 == 0, 16-byte aligned rows: float4 lanes, a thread's four groups requested before any is used (round 4: the scalar form was
// a chain of 16 dependent-latency iterations per thread, 15 us for 24 MB).  Same per-element arithmetic, float partial sums per group folded
// into the thread's fp64 sum.
__device__ __forceinline__ double gnll_sample_vec(const float* __restrict__ o, const float* __restrict__ target, long long HW, float grad_scale,
                                                  float* __restrict__ d)
{
    const long long ng = HW >> 2;
    const float nf = (float)HW;
    double acc = 0;
    for (long long g0 = (long long)blockIdx.x * 256 + threadIdx.x; g0 < ng; g0 += (long long)gridDim.x * 256 * 4) {
        float4 m4[4], s4[4], t4[4]; long long gi[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            gi[u] = g0 + (long long)u * gridDim.x * 256;
            const long long gc = gi[u] < ng ? gi[u] : ng - 1;
            m4[u] = *reinterpret_cast<const float4*>(o + 4 * gc); s4[u] = *reinterpret_cast<const float4*>(o + HW + 4 * gc); t4[u] = *reinterpret_cast<const float4*>(target + 4 * gc);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (gi[u] >= ng) continue;
            const float mm[4] = {m4[u].x, m4[u].y, m4[u].z, m4[u].w}, ss[4] = {s4[u].x, s4[u].y, s4[u].z, s4[u].w}, tt[4] = {t4[u].x, t4[u].y, t4[u].z, t4[u].w};
            float dm[4], ds[4];
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                const float sraw = ss[l];
                const float s_ = fminf(fmaxf(sraw, -20.f), 20.f);
                const bool inside = (sraw >= -20.f) && (sraw <= 20.f);
                const float df = tt[l] - mm[l], e = expf(s_);
                acc += (double)(e * df * df - s_);
                dm[l] = grad_scale * (-2.f * e * df) / nf;
                ds[l] = inside ? grad_scale * (e * df * df - 1.f) / nf : 0.f;
            }
            if (d) {
                *reinterpret_cast<float4*>(d + 4 * gi[u]) = make_float4(dm[0], dm[1], dm[2], dm[3]);
                *reinterpret_cast<float4*>(d + HW + 4 * gi[u]) = make_float4(ds[0], ds[1], ds[2], ds[3]);
            }
        }
    }
    return acc / (double)HW;
}

// ---- AdamW(weight_decay = 0) on element i of a flat block: THE statement of the update, for every kernel that applies one.  next() stores
// the two moments and returns the new value of a parameter that was `pi` (the bf16 update rounds it, adam_kernel decays pi first); () stores it ----
struct AdamStep {
    float* __restrict__ p; float* __restrict__ m; float* __restrict__ v;
    float b1, b2, eps, step_size, inv_sqrt_bc2;
    __device__ __forceinline__ float next(long long i, float gi, float pi) const
    {
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        return pi - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
    }
    __device__ __forceinline__ void operator()(long long i, float gi) const { p[i] = next(i, gi, p[i]); }
};

// ---- the KL term of ONE (mu, rho) pair as a policy: term() returns the term, float32 pieces added in float64, and
// yields smu / srho = scale * its two derivatives.  The scale is applied in here because the directions associate that product differently
// and the bits depend on it.  Arg is the prior as a kernel takes it: the policy is built on the device (log s0 is the device's logf) ----
struct GaussPrior { float m0, s0; };
// the reverse direction KL(prior || posterior) (BayTorch/modules/module.py:64-80): scale * d * inv * inv, left to right
struct KlReverse {
    typedef GaussPrior Arg;
    float m0, log_s0, s0sq;
    __device__ __forceinline__ explicit KlReverse(const GaussPrior& pr) : m0(pr.m0), log_s0(logf(pr.s0)), s0sq(pr.s0 * pr.s0) {}
    __device__ __forceinline__ double term(float mu, float r, float scale, float& smu, float& srho) const
    {
        const float s = softplus_f(r), d = mu - m0, inv = 1.f / s;
        smu = scale * d * inv * inv;
        srho = scale * (inv - (s0sq + d * d) * inv * inv * inv) * sigmoid_f(r);
        return (double)(logf(s) - log_s0) + (double)((s0sq + d * d) / (2.f * s * s)) - 0.5;
    }
};

// ---- the forward direction, KL(posterior || prior) (modules/module.py:76-80 with kl_type != 'reverse'; the textbook ELBO's term), of ONE
// (mu, rho) pair: returns the term, float32 pieces added in float64 as the reverse kernels add theirs; gmu / grho = its two derivatives.
// Every forward kernel takes its arithmetic from here, and every operation of it is rounded on its own (no fma contraction: which products
// fuse would depend on what the kernel around it keeps of the three results, and the fused and the unfused KL would part in the ninth digit) ----
__device__ __forceinline__ double kl_forward_terms(float mu, float r, float m0, float log_s0, float s0sq, float& gmu, float& grho)
{
#pragma clang fp contract(off)
    const float s = softplus_f(r), d = mu - m0;
    gmu = d / s0sq;
    grho = (s / s0sq - 1.f / s) * sigmoid_f(r);
    return (double)(log_s0 - logf(s)) + (double)((s * s + d * d) / (2.f * s0sq)) - 0.5;
}

// the forward direction as a policy: scale * (the derivatives of kl_forward_terms)
struct KlForward {
    typedef GaussPrior Arg;
    float m0, log_s0, s0sq;
    __device__ __forceinline__ explicit KlForward(const GaussPrior& pr) : m0(pr.m0), log_s0(logf(pr.s0)), s0sq(pr.s0 * pr.s0) {}
    // the product with the scale is outside the contract-off body: it may fuse with the caller's add
    __device__ __forceinline__ double term(float mu, float r, float scale, float& smu, float& srho) const
    {
        float gmu, grho;
        const double t = kl_forward_terms(mu, r, m0, log_s0, s0sq, gmu, grho);
        smu = scale * gmu; srho = scale * grho;
        return t;
    }
};

// ---- fused tail of an ELBO iteration on ONE flat block [MU | RHO | BN] (adam.p): this thread's share (grid x strides over the elements) of
// the KL sum; unless `skip`, grads += temp * dKL (written back) and Adam on p / m / v.  The loop shape fixes which thread owns which element
// and with that the order of the float64 sum: this one serves the closed-form terms, elbo_update_share_quads the drawn one ----
template <class Term>
__device__ __forceinline__ double elbo_update_share(const Term& kl, float* __restrict__ g, long long n_vi, long long n_bn, float temp, const AdamStep& adam,
                                                    bool skip)
{
    const float* p = adam.p;
    double acc = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_vi; i += (long long)gridDim.x * 256) {
        float dkm, dkr;
        acc += kl.term(p[i], p[n_vi + i], temp, dkm, dkr);
        if (skip) continue;
        const float gmu = g[i] + dkm;
        const float grho = g[n_vi + i] + dkr;
        g[i] = gmu; g[n_vi + i] = grho;
        adam(i, gmu); adam(n_vi + i, grho);
    }
    if (!skip)
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_bn; i += (long long)gridDim.x * 256) adam(2 * n_vi + i, g[2 * n_vi + i]);
    return acc;
}

// ---- the scale-mixture prior p(w) = sum_j pi_j N(w; m_j, sigma_j^2), J <= 4 (MixtureNormal, BayTorch/distributions/distributions.py:6-28;
// DESIGN.md section 26).  The KL term against it has no closed form: the reference estimates it with ONE draw w = mu + s eps per weight
// (mc_kl_divergence, :30-35, through VIModule._kl with kl_type != 'reverse') as log q(w) - log p(w) ----
// the ONE statement of what is wrong with a prior: an entry point refuses it on the host with the fault's name (mix_fault_name), a per-fit
// kernel meets it on the device (that row is marked dead).  A NaN fails every comparison.
enum { MIX_OK = 0, MIX_BAD_N, MIX_BAD_PI, MIX_BAD_SIGMA, MIX_BAD_IV, MIX_BAD_MU };
__host__ __device__ __forceinline__ int mix_prior_fault(const mfvi_mixture_prior& p)
{
    if (p.n < 1 || p.n > MFVI_MIXTURE_MAX) return MIX_BAD_N;
    for (int j = 0; j < p.n; ++j) {
        if (!(p.pi[j] > 0.f && p.pi[j] <= 3.40282347e38f)) return MIX_BAD_PI;
        if (!(p.sigma[j] > 0.f && p.sigma[j] <= 3.40282347e38f)) return MIX_BAD_SIGMA;
        const float iv = 1.f / (p.sigma[j] * p.sigma[j]);      // the factor of every squared distance: a normal float32
        if (!(iv >= 1.17549435e-38f && iv <= 3.40282347e38f)) return MIX_BAD_IV;
        if (!(p.mu[j] >= -3.40282347e38f && p.mu[j] <= 3.40282347e38f)) return MIX_BAD_MU;
    }
    return MIX_OK;
}
inline const char* mix_fault_name(int fault)
{
    static const char* const names[] = {nullptr, "prior->n outside 1..MFVI_MIXTURE_MAX", "a pi not finite or <= 0", "a sigma not finite or <= 0",
                                        "a 1 / sigma^2 that is not a normal float32", "a component mean not finite"};
    return names[fault];
}
// the key of the term's draw: RNG domain KLMC, stream 0; step_dev: the device-resident part of the counter word (key_now), or nullptr
inline RngKey klmc_key(uint64_t seed, uint32_t sample, uint32_t step, const int32_t* step_dev)
{
    RngKey k; k.k0 = (uint32_t)seed; k.k1 = (uint32_t)(seed >> 32); k.stream = (uint32_t)DOMAIN_KLMC << 24; k.sample = sample; k.step = step; k.step_dev = step_dev;
    return k;
}
// the per-component constants, formed once per block: c_j = log pi_j - log sigma_j, iv_j = 1 / sigma_j^2.  A component past the prior's n
// has c = -inf and iv = 0: its a_j is -inf, its weight exp(a_j - max) and its share of G are exactly 0, so the loops over the compile-time
// maximum need no branch on n.  That holds while (w - m_j)^2 is finite, |w| below ~1.8e19: beyond it inf * 0 is NaN, and where every real
// component's a_j is -inf (a squared distance times iv that overflows) a_j - max is NaN too.  Both need parameters that have long
// diverged; the NaN then shows in the term and the gradients as any overflow of the Gaussian kernels does.
struct MixPrep { float c[MFVI_MIXTURE_MAX], m[MFVI_MIXTURE_MAX], iv[MFVI_MIXTURE_MAX]; };
__device__ __forceinline__ MixPrep mix_prepare(const mfvi_mixture_prior& p)
{
#pragma clang fp contract(off)
    MixPrep q;
#pragma unroll
    for (int j = 0; j < MFVI_MIXTURE_MAX; ++j) {
        const bool on = j < p.n;
        q.c[j] = on ? logf(p.pi[j]) - logf(p.sigma[j]) : -INFINITY;
        q.m[j] = on ? p.mu[j] : 0.f;
        q.iv[j] = on ? 1.f / (p.sigma[j] * p.sigma[j]) : 0.f;
    }
    return q;
}
// ONE (mu, rho, eps) triple: returns the term (the two 1/2 log 2 pi cancel), float32 pieces added in float64; gmu / grho = its two derivatives
// with w = mu + s eps differentiated through (the reparametrised draw).  The mixture density goes through a log-sum-exp, so the term is
// finite where the reference's log(sum pi_j exp(log_prob_j)) underflows to log 0; the responsibilities are r_j = e_j / sum e_j with
// e_j = exp(a_j - max), the same numbers as exp(a_j - L) without a second round of exponentials.  d log q / d mu is identically 0 (the
// reference's autograd forms it as eps / s - eps / s and keeps the rounding).  Every mixture kernel takes its arithmetic from here, every
// operation rounded on its own, as kl_forward_terms.
__device__ __forceinline__ double kl_mixture_terms(float mu, float r, float eps, const MixPrep& q, float& gmu, float& grho)
{
#pragma clang fp contract(off)
    const float s = softplus_f(r), w = mu + s * eps;
    float a[MFVI_MIXTURE_MAX], d[MFVI_MIXTURE_MAX], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < MFVI_MIXTURE_MAX; ++j) {
        d[j] = w - q.m[j];
        a[j] = q.c[j] - (d[j] * d[j]) * (0.5f * q.iv[j]);
        mx = fmaxf(mx, a[j]);
    }
    float se = 0.f, ge = 0.f;
#pragma unroll
    for (int j = 0; j < MFVI_MIXTURE_MAX; ++j) {
        const float e = expf(a[j] - mx);
        se = se + e;
        ge = ge + e * (d[j] * q.iv[j]);
    }
    const float G = ge / se, L = mx + logf(se);
    gmu = G;
    grho = (G * eps - 1.f / s) * sigmoid_f(r);
    return (double)(-0.5f * (eps * eps) - logf(s)) - (double)L;
}

// the policy of the drawn term: the prior's constants and the key of the draw, its counter word resolved (Arg: key_now does that here)
struct KlMixture {
    struct Arg { mfvi_mixture_prior prior; RngKey key; };
    MixPrep q; RngKey key;
    __device__ __forceinline__ KlMixture(const mfvi_mixture_prior& prior, const RngKey& k) : q(mix_prepare(prior)), key(k) {}
    __device__ __forceinline__ explicit KlMixture(const Arg& a) : q(mix_prepare(a.prior)), key(key_now(a.key)) {}
    __device__ __forceinline__ double term(float mu, float r, float eps, float scale, float& smu, float& srho) const
    {
        float gmu, grho;
        const double t = kl_mixture_terms(mu, r, eps, q, gmu, grho);
        smu = scale * gmu; srho = scale * grho;
        return t;
    }
};

// ---- elbo_update_share for the drawn term: the same Adam and BN loop; the (mu, rho) pairs go in quads, element i = lane
// i & 3 of Philox block i >> 2 of the key's stream (RNG domain KLMC), so a weight's draw costs a quarter of a Philox block and no memory.
// A quad's four pairs and gradients are requested before any is used, with clamped indices (no branch around a load); the stores and the
// Adam of a lane past n_vi are predicated ----
template <class Term>
__device__ __forceinline__ double elbo_update_share_quads(const Term& kl, float* __restrict__ g, long long n_vi, long long n_bn, float temp,
                                                          const AdamStep& adam, bool skip)
{
    const float* p = adam.p;
    double acc = 0;
    const long long nq = (n_vi + 3) >> 2;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long long)gridDim.x * 256) {
        float z[4], mu4[4], r4[4], gm4[4], gr4[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const long long ic = 4 * q + l < n_vi ? 4 * q + l : n_vi - 1;
            mu4[l] = p[ic]; r4[l] = p[n_vi + ic]; gm4[l] = g[ic]; gr4[l] = g[n_vi + ic];
        }
        spec_normal4(kl.key, (uint32_t)q, z);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const long long i = 4 * q + l;
            float dkm, dkr;
            const double term = kl.term(mu4[l], r4[l], z[l], temp, dkm, dkr);
            if (i < n_vi) {
                acc += term;
                if (!skip) {
                    const float gmu = gm4[l] + dkm;
                    const float grho = gr4[l] + dkr;
                    g[i] = gmu; g[n_vi + i] = grho;
                    adam(i, gmu); adam(n_vi + i, grho);
                }
            }
        }
    }
    if (!skip)
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_bn; i += (long long)gridDim.x * 256) adam(2 * n_vi + i, g[2 * n_vi + i]);
    return acc;
}

// ---- out[j] = (base ? base[j] : a) + b * N(0,1), element j = lane j & 3 of Philox block j >> 2 of the key's stream (grid x strides over the blocks) ----
__device__ __forceinline__ void normal_fill_share(const RngKey& key, long long n, float a, float b, const float* __restrict__ base, float* __restrict__ out)
{
    const long long nblk = (n + 3) >> 2;
    for (long long blk = (long long)blockIdx.x * 256 + threadIdx.x; blk < nblk; blk += (long long)gridDim.x * 256) {
        float z[4]; spec_normal4(key, (uint32_t)blk, z);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const long long j = blk * 4 + l;
            if (j < n) out[j] = (base ? base[j] : a) + b * z[l];
        }
    }
}

// ---- the runner's smoothed outputs (bayesian_optimization.py:1376-1381) at pixel i: m = mean_k out[k][0], a = mean_k exp(-out[k][1]) over the
// n samples out[n][C][HW]; ema[c] = first ? value : ema[c] * w + value * (1 - w).  Returns the new ema[0][i] ----
__device__ __forceinline__ float sample_means_ema(const float* __restrict__ out, int n, int C, long long HW, long long i, float* __restrict__ ema, float w,
                                                  int first, float& m, float& a)
{
    m = 0.f; a = 0.f;
    for (int k = 0; k < n; ++k) {
        m += out[(long long)k * C * HW + i];
        if (C > 1) a += expf(-out[(long long)k * C * HW + HW + i]);
    }
    m /= (float)n; a /= (float)n;
    const float e0 = first ? m : ema[i] * w + m * (1.f - w);
    ema[i] = e0;
    if (C > 1) ema[HW + i] = first ? a : ema[HW + i] * w + a * (1.f - w);
    return e0;
}

// ---- gaussian_nll with the sigmoid on the 3 colour channels, one shared log-precision channel and a mask (bayesian_optimization.py:3001-3010)
// of ONE sample o[4][HW] against target[3][HW] / mask[mask_channels][HW]: this thread's share of the mean over 3 HW elements (grid x strides
// over the pixels) and, with d, the gradient d[4][HW] ----
__device__ __forceinline__ double gnll_inp_sample(const float* __restrict__ o, const float* __restrict__ target, const float* __restrict__ mask,
                                                  int mask_channels, long long HW, float grad_scale, float* __restrict__ d)
{
    const float inv_n = 1.f / (float)(3 * HW);
    double acc = 0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < HW; p += (long long)gridDim.x * 256) {
        const float sraw = o[3 * HW + p];
        const float s = fminf(fmaxf(sraw, -20.f), 20.f);
        const bool inside = (sraw >= -20.f) && (sraw <= 20.f);
        const float e = expf(s);
        float ds = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float m = sigmoid_f(o[c * HW + p]);
            const float mk = mask[(mask_channels == 3 ? c : 0) * HW + p];
            const float df = target[c * HW + p] - m;
            acc += (double)((e * df * df - s) * mk);
            if (d) {
                d[c * HW + p] = grad_scale * (-2.f * e * df) * mk * m * (1.f - m) * inv_n;
                ds += (e * df * df - 1.f) * mk;
            }
        }
        if (d) d[3 * HW + p] = inside ? grad_scale * ds * inv_n : 0.f;
    }
    return acc * (double)inv_n;
}

// ---- the inpainting runner's smoothed outputs (bayesian_optimization.py:3039-3064) at pixel i over the n samples out[n][4][HW]:
// m[c] = mean_k sigmoid(out[k][c]), a = mean_k exp(-out[k][3]); ema[c] = first ? value : ema[c] * w + value * (1 - w), e0[c] the new ema[c][i] ----
__device__ __forceinline__ void sample_means_ema_inp(const float* __restrict__ out, int n, long long HW, long long i, float* __restrict__ ema, float w,
                                                     int first, float m[3], float e0[3], float& a)
{
    a = 0.f;
    for (int k = 0; k < n; ++k) a += expf(-out[((long long)k * 4 + 3) * HW + i]);
    a /= (float)n;
    ema[3 * HW + i] = first ? a : ema[3 * HW + i] * w + a * (1.f - w);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float mc = 0.f;
        for (int k = 0; k < n; ++k) mc += sigmoid_f(out[((long long)k * 4 + c) * HW + i]);
        mc /= (float)n;
        m[c] = mc;
        e0[c] = first ? mc : ema[c * HW + i] * w + mc * (1.f - w);
        ema[c * HW + i] = e0[c];
    }
}
