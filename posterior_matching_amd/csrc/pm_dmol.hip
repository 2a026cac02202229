// Discretised mixture of logistics with C = 2..4 channels and autoregressive channel coefficients, reference
// posterior_matching/models/vdvae.py:331-476 (_LogisticMixtureDist / LogisticMixture with num_channels > 1).
//   params [rows, nm, 2C + K + 1], K = C(C-1)/2; per component (logit, loc_0..loc_{C-1}, raw_scale_0.., coef_0..coef_{K-1}),
//   coefficient order (1,0), (2,0), (2,1), (3,0), ...; the coefficients are used raw (no tanh).
//   value [rows, C] raw pixel values in [low, high].
// One thread per pixel row, 64 rows per workgroup.  A row of params is (2C + K + 1) * nm floats (400 B at C = 3, nm = 10), so
// a thread-per-row read of global memory would stride by that: each workgroup stages its contiguous slab through LDS with
// 16-B loads instead, rows padded to an odd number of dwords (ds_read_b32 of 64 rows at an odd stride is conflict-free).
// The backward pass writes its gradients into the same slab and stores it back the same way.  No per-(component, channel)
// arrays: the backward pass recomputes each component's channel terms in a second pass (only [C]-sized arrays, in registers).
#include <cstdint>
#include "pm_common.h"

namespace {

constexpr int MC_ROWS = 64;          // rows (threads) per workgroup: one wave
constexpr int MC_MAXM = 16;          // = DMOL_MAXM of the one-channel kernels

__device__ __forceinline__ float log_sig(float x) { return -pm_softplus(-x); }

template <int C>
struct McLayout {
    static constexpr int K = C * (C - 1) / 2;
    static constexpr int NOUT = 2 * C + K + 1;
    __device__ static constexpr int loc(int c) { return 1 + c; }
    __device__ static constexpr int scale(int c) { return 1 + C + c; }
    __device__ static constexpr int coef(int i, int j) { return 1 + 2 * C + i * (i - 1) / 2 + j; }
};

inline int mc_stride(int C, int nm) { return (2 * C + C * (C - 1) / 2 + 1) * nm; }
inline int mc_lds_stride(int S) { return S | 1; }

// slab of rows [r0, r0 + n) of a [*, S] array -> LDS [n, SP]; 16-B global loads where the slab start is 16-B aligned
__device__ __forceinline__ void mc_stage_in(const float* __restrict__ src, float* lds, int n, int S, int SP) {
    const int total = n * S;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int n4 = total >> 2;
        for (int q = threadIdx.x; q < n4; q += MC_ROWS) {
            const f32x4 v = reinterpret_cast<const f32x4*>(src)[q];
            int i = q * 4, row = i / S, f = i - row * S;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                lds[row * SP + f] = v[u];
                if (++f == S) { f = 0; ++row; }
            }
        }
        done = n4 * 4;
    }
    for (int i = done + threadIdx.x; i < total; i += MC_ROWS) {
        const int row = i / S;
        lds[row * SP + (i - row * S)] = src[i];
    }
}

__device__ __forceinline__ void mc_stage_out(float* __restrict__ dst, const float* lds, int n, int S, int SP) {
    const int total = n * S;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const int n4 = total >> 2;
        for (int q = threadIdx.x; q < n4; q += MC_ROWS) {
            f32x4 v;
            int i = q * 4, row = i / S, f = i - row * S;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = lds[row * SP + f];
                if (++f == S) { f = 0; ++row; }
            }
            reinterpret_cast<f32x4*>(dst)[q] = v;
        }
        done = n4 * 4;
    }
    for (int i = done + threadIdx.x; i < total; i += MC_ROWS) {
        const int row = i / S;
        dst[i] = lds[row * SP + (i - row * S)];
    }
}

// log P(bin of y) of the quantised logistic shifted by -0.5 (tfd.QuantizedDistribution with open edge bins at low / high) and
// its partial derivatives a_up = d/d up, a_dn = d/d dn, up = (y + .5 - loc) / sc, dn = (y - .5 - loc) / sc.  Same arithmetic as
// dmol_kernel in pm_vdvae.hip.
__device__ __forceinline__ float mc_term(float y, float up, float dn, float low, float high, float& a_up, float& a_dn) {
    float c;
    a_up = 0.f;
    a_dn = 0.f;
    if (y >= high) {
        c = log_sig(-dn);
        a_dn = -pm_sigmoid(dn);
    } else if (y <= low) {
        c = log_sig(up);
        a_up = pm_sigmoid(-up);
    } else {
        const float lcu = log_sig(up), lsu = log_sig(-up), lcd = log_sig(dn), lsd = log_sig(-dn);
        const bool use_sf = lsu < lcu;     // TFP: difference of the smaller pair (log-survival vs log-cdf)
        const float big = use_sf ? lsd : lcu, small = use_sf ? lsu : lcd;
        c = big + log1pf(-expf(fminf(small - big, 0.f)));
        a_up = expf(lcu + lsu - c);
        a_dn = -expf(lcd + lsd - c);
    }
    return c;
}

// One component's channel terms: comp = sum_c log P_c; with dloc / dsc (d comp / d raw loc_c, d comp / d raw scale_c).
template <int C, bool GRAD>
__device__ __forceinline__ float mc_component(const float* pk, const float (&y)[C], const float (&xt)[C], float low, float high,
                                              float (&dloc)[C], float (&dsc)[C]) {
    using L = McLayout<C>;
    const float half = 0.5f * (high - low);
    float comp = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float m = pk[L::loc(c)];
#pragma unroll
        for (int j = 0; j < c; ++j) m += xt[j] * pk[L::coef(c, j)];     // conditioning in the [-1, 1] space (:355-369)
        const float raw = pk[L::scale(c)];
        const float loc = low + half * (m + 1.f);
        const float sc = (pm_softplus(raw) + expf(-7.f)) * half;
        const float up = (y[c] + 0.5f - loc) / sc, dn = (y[c] - 0.5f - loc) / sc;
        float a_up, a_dn;
        comp += mc_term(y[c], up, dn, low, high, a_up, a_dn);
        if (GRAD) {
            dloc[c] = -(a_up + a_dn) * half / sc;
            dsc[c] = -(up * a_up + dn * a_dn) / sc * half * pm_sigmoid(raw);
        }
    }
    return comp;
}

template <int C>
__device__ __forceinline__ void mc_load_value(const float* __restrict__ value, long long r, float low, float high, float (&y)[C],
                                              float (&xt)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float v = value[(size_t)r * C + c];
        xt[c] = 2.f * (v - low) / (high - low) - 1.f;       // unclamped (:355-357)
        y[c] = fminf(fmaxf(v, low), high);
    }
}

// log_softmax normaliser of the logits and the mixture log-prob of one row (online logsumexp: no per-component arrays)
template <int C>
__device__ __forceinline__ float mc_row_ll(const float* pr, int nm, const float (&y)[C], const float (&xt)[C], float low,
                                           float high, float& lse_w) {
    constexpr int S = McLayout<C>::NOUT;
    float mx = -INFINITY;
    for (int k = 0; k < nm; ++k) mx = fmaxf(mx, pr[S * k]);
    float se = 0.f;
    for (int k = 0; k < nm; ++k) se += expf(pr[S * k] - mx);
    lse_w = mx + logf(se);
    float best = -INFINITY, s = 0.f;
    float unused_l[C], unused_s[C];
    for (int k = 0; k < nm; ++k) {
        const float v = pr[S * k] - lse_w + mc_component<C, false>(pr + S * k, y, xt, low, high, unused_l, unused_s);
        if (v > best) {
            s = s * expf(best - v) + 1.f;
            best = v;
        } else {
            s += expf(v - best);
        }
    }
    return best + logf(s);
}

template <int C>
__global__ __launch_bounds__(MC_ROWS) void dmol_mc_fwd_kernel(const float* __restrict__ params, const float* __restrict__ value,
                                                              float* __restrict__ ll, long long R, int nm, int P, float low,
                                                              float high) {
    extern __shared__ float slab[];
    const int S = McLayout<C>::NOUT * nm, SP = S | 1;
    const long long r0 = (long long)blockIdx.x * MC_ROWS;
    const int n = (int)min((long long)MC_ROWS, R - r0);
    mc_stage_in(params + (size_t)r0 * S, slab, n, S, SP);
    __syncthreads();
    const bool active = threadIdx.x < n;
    const long long r = r0 + (active ? threadIdx.x : n - 1);    // idle lanes redo the last row and add nothing
    float y[C], xt[C], lse_w;
    mc_load_value<C>(value, r, low, high, y, xt);
    const float lp = mc_row_ll<C>(slab + (size_t)(r - r0) * SP, nm, y, xt, low, high, lse_w);
    // one atomic add per wave when its rows belong to one example (as dmol_kernel<false>)
    const int e = active ? (int)(r / P) : -1;
    const int e0 = __shfl(e, 0, 64);
    if (__all(!active || e == e0)) {
        const float t = pm_wave_sum(active ? lp : 0.f);
        if ((threadIdx.x & 63) == 0 && e0 >= 0) atomicAdd(ll + e0, t);
    } else if (active) {
        atomicAdd(ll + e, lp);
    }
}

// dparams = g * d ll / d params, every element of every row written (no atomics: deterministic)
template <int C>
__global__ __launch_bounds__(MC_ROWS) void dmol_mc_bwd_kernel(const float* __restrict__ params, const float* __restrict__ value,
                                                              const float g, float* __restrict__ dparams, long long R, int nm,
                                                              float low, float high) {
    using L = McLayout<C>;
    constexpr int NO = L::NOUT;
    extern __shared__ float slab[];
    const int S = NO * nm, SP = S | 1;
    const long long r0 = (long long)blockIdx.x * MC_ROWS;
    const int n = (int)min((long long)MC_ROWS, R - r0);
    mc_stage_in(params + (size_t)r0 * S, slab, n, S, SP);
    __syncthreads();
    if (threadIdx.x < n) {
        const long long r = r0 + threadIdx.x;
        float* pr = slab + (size_t)threadIdx.x * SP;
        float y[C], xt[C], lse_w;
        mc_load_value<C>(value, r, low, high, y, xt);
        const float lp = mc_row_ll<C>(pr, nm, y, xt, low, high, lse_w);
        // second pass: component k's terms again, its gradients written over its own (already consumed) parameters
        for (int k = 0; k < nm; ++k) {
            float* pk = pr + NO * k;
            float dloc[C], dsc[C];
            const float lw = pk[0] - lse_w;
            const float comp = mc_component<C, true>(pk, y, xt, low, high, dloc, dsc);
            const float resp = expf(lw + comp - lp);            // posterior responsibility of component k
            pk[0] = g * (resp - expf(lw));
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float gl = g * resp * dloc[c];
                pk[L::loc(c)] = gl;
                pk[L::scale(c)] = g * resp * dsc[c];
#pragma unroll
                for (int j = 0; j < c; ++j) pk[L::coef(c, j)] = gl * xt[j];
            }
        }
    }
    __syncthreads();
    mc_stage_out(dparams + (size_t)r0 * S, slab, n, S, SP);
}

// _LogisticMixtureDist.mean (:396-435): softmax-weighted locs and coeffs, channels in order, each clipped to [-1, 1] before
// it conditions the next; round half to even
template <int C>
__global__ __launch_bounds__(MC_ROWS) void dmol_mc_mean_kernel(const float* __restrict__ params, float* __restrict__ out,
                                                               long long R, int nm, float low, float high) {
    using L = McLayout<C>;
    constexpr int NO = L::NOUT;
    extern __shared__ float slab[];
    const int S = NO * nm, SP = S | 1;
    const long long r0 = (long long)blockIdx.x * MC_ROWS;
    const int n = (int)min((long long)MC_ROWS, R - r0);
    mc_stage_in(params + (size_t)r0 * S, slab, n, S, SP);
    __syncthreads();
    if (threadIdx.x >= n) return;
    const float* pr = slab + (size_t)threadIdx.x * SP;
    float mx = -INFINITY;
    for (int k = 0; k < nm; ++k) mx = fmaxf(mx, pr[NO * k]);
    float se = 0.f, loc[C], coef[L::K > 0 ? L::K : 1];
#pragma unroll
    for (int c = 0; c < C; ++c) loc[c] = 0.f;
#pragma unroll
    for (int q = 0; q < L::K; ++q) coef[q] = 0.f;
    for (int k = 0; k < nm; ++k) {
        const float* pk = pr + NO * k;
        const float w = expf(pk[0] - mx);
        se += w;
#pragma unroll
        for (int c = 0; c < C; ++c) loc[c] += w * pk[L::loc(c)];
#pragma unroll
        for (int q = 0; q < L::K; ++q) coef[q] += w * pk[1 + 2 * C + q];
    }
    const float half = 0.5f * (high - low);
    float m[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float v = loc[c] / se;
#pragma unroll
        for (int j = 0; j < c; ++j) v += (coef[c * (c - 1) / 2 + j] / se) * m[j];
        m[c] = fminf(fmaxf(v, -1.f), 1.f);
        out[(size_t)(r0 + threadIdx.x) * C + c] = rintf(low + half * (m[c] + 1.f));
    }
}

inline unsigned mc_blocks(long long rows) { return (unsigned)((rows + MC_ROWS - 1) / MC_ROWS); }
inline size_t mc_lds_bytes(int C, int nm) { return (size_t)MC_ROWS * mc_lds_stride(mc_stride(C, nm)) * sizeof(float); }
inline bool mc_args_ok(long long rows, int C, int nm) { return rows > 0 && C >= 2 && C <= 4 && nm >= 1 && nm <= MC_MAXM; }

}  // namespace

extern "C" int pm_dmol_mc_ll_fwd(pm_stream_t stream, const float* params, const float* value, float* ll, long long rows,
                                 int num_channels, int num_mixtures, int P, float low, float high) {
    if (!params || !value || !ll || !mc_args_ok(rows, num_channels, num_mixtures) || P <= 0 || rows % P) return PM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (pm_zero_async(s, ll, (size_t)(rows / P) * sizeof(float))) return PM_ELAUNCH;
    const size_t lds = mc_lds_bytes(num_channels, num_mixtures);
    PM_KTAG("dmol_mc_fwd_kernel<%d>", num_channels);
#define PM_MC_FWD(CC) hipLaunchKernelGGL(dmol_mc_fwd_kernel<CC>, dim3(mc_blocks(rows)), dim3(MC_ROWS), lds, s, params, value, ll, \
                                         rows, num_mixtures, P, low, high)
    switch (num_channels) {
        case 2: PM_MC_FWD(2); break;
        case 3: PM_MC_FWD(3); break;
        default: PM_MC_FWD(4); break;
    }
#undef PM_MC_FWD
    return pm_check_launch("pm_dmol_mc_ll_fwd");
}

extern "C" int pm_dmol_mc_ll_bwd(pm_stream_t stream, const float* params, const float* value, float g, float* dparams,
                                 long long rows, int num_channels, int num_mixtures, int P, float low, float high) {
    if (!params || !value || !dparams || !mc_args_ok(rows, num_channels, num_mixtures) || P <= 0) return PM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = mc_lds_bytes(num_channels, num_mixtures);
    PM_KTAG("dmol_mc_bwd_kernel<%d>", num_channels);
#define PM_MC_BWD(CC) hipLaunchKernelGGL(dmol_mc_bwd_kernel<CC>, dim3(mc_blocks(rows)), dim3(MC_ROWS), lds, s, params, value, g, \
                                         dparams, rows, num_mixtures, low, high)
    switch (num_channels) {
        case 2: PM_MC_BWD(2); break;
        case 3: PM_MC_BWD(3); break;
        default: PM_MC_BWD(4); break;
    }
#undef PM_MC_BWD
    return pm_check_launch("pm_dmol_mc_ll_bwd");
}

extern "C" int pm_dmol_mc_mean(pm_stream_t stream, const float* params, float* out, long long rows, int num_channels,
                               int num_mixtures, float low, float high) {
    if (!params || !out || !mc_args_ok(rows, num_channels, num_mixtures)) return PM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = mc_lds_bytes(num_channels, num_mixtures);
    PM_KTAG("dmol_mc_mean_kernel<%d>", num_channels);
#define PM_MC_MEAN(CC) hipLaunchKernelGGL(dmol_mc_mean_kernel<CC>, dim3(mc_blocks(rows)), dim3(MC_ROWS), lds, s, params, out, rows, \
                                          num_mixtures, low, high)
    switch (num_channels) {
        case 2: PM_MC_MEAN(2); break;
        case 3: PM_MC_MEAN(3); break;
        default: PM_MC_MEAN(4); break;
    }
#undef PM_MC_MEAN
    return pm_check_launch("pm_dmol_mc_mean");
}
