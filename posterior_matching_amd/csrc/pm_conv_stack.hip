// Fused forward of a ConvEncoder's first four layers (reference networks.py:9-38): one workgroup per image, one launch
// per encoder, every intermediate activation resident in LDS.
//
//   L1  IHxIWxC0 -> 5x5, N = 32, stride 1      the lane form of pm_thin.hip (f32 FMAs on the VALU)
//   L2  .. L4                                  the TR form of image_conv_bf16_kernel (pm_conv.hip: bf16x3 on the MFMA)
//
// Layer by layer, the image-resident kernels spend most of their time outside the matrix pipe: every launch reads its
// f32 input back from HBM and splits it into hi / lo bf16 planes in LDS, runs the k-loop, stores f32 results, and the
// next launch reads them straight back (one workgroup per image, the whole chip in lockstep through the three phases).
// Here each layer's epilogue computes its f32 value once, stores it to HBM (out_i: the backward pass and the weight
// gradients read those buffers) and, for L1 - L3, writes its hi / lo split into LDS where the next layer's k-loop reads
// it.  One barrier separates two layers.
//
// The arithmetic is the layer-wise path's, bit for bit:
//  * L1: accumulator 0, fmaf over (c, jy, jx), then + bias and leaky - thin_conv_lane_kernel's order;
//  * L2 - L4: per 32 x 32 output tile the tap walk (ky, kx, channel chunk), the same six 32x32x16 bf16 MFMAs per k-step in
//    the same order, no split-K, pm_epilogue_tile_t's bias + activation;
//  * the hi / lo planes equal what the next layer-wise launch's staging computes (split4 of the same f32 value).
// How waves are dealt tiles is free (it does not change any tile's k-sequence).
//
// LDS (MNIST: 28x28x{1,2} -> 28x28x32 -> 14x14x32 -> 14x14x64 -> 7x7x64), planes with the 16-byte position pad PS = C + 8
// and a 128-byte zero slot behind each plane:
//   region X (offset 0):  L1 out = L2 in (125 696 B);  later L3 out = L4 in (56 704 B), written once L2 is done with X
//   region Y:             L1's f32 input patch (8 KB);  later L2 out = L3 in (31 616 B)
#include <cstdint>
#include <cstdlib>
#include <type_traits>
#include "pm_common.h"

namespace {

constexpr int BK = 32;
constexpr int NW = 8;                      // waves per workgroup
constexpr int ROW_INVALID = -(1 << 28);
constexpr size_t LDS_MAX = 160 * 1024;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// hi = bf16(a), lo = bf16(a - hi) for two floats: split4's arithmetic (pm_conv.hip), element by element
__device__ __forceinline__ void split2(float a0, float a1, unsigned& hi, unsigned& lo) {
    const unsigned h = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a0, a1}, bf16x2));
    const float f0 = __builtin_bit_cast(float, h << 16);
    const float f1 = __builtin_bit_cast(float, h & 0xffff0000u);
    hi = h;
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a0 - f0, a1 - f1}, bf16x2));
}

struct StackConv {          // one image-form layer (L2 - L4)
    int IH, IW, C, OH, OW, N, KH, KW, a, cs, off, offx;
    int npad, nct, wct;     // column tiles, waves per column tile
    long long plane;        // elements between the hi and the lo plane of the pre-split weights
    const __bf16* ws;
    const float* bias;
    float* out;
    int in_off, out_off;    // LDS byte offsets of the input planes and of the output planes (out_off < 0: none)
};

struct StackArgs {
    int IH, IW, OH, OW, N, off;            // L1 (lane form: a = 1, cs = +1, off_x = off)
    int wts, wcs, wns;
    float slope;
    const float* in;
    const float* w;
    const float* bias;
    float* out;
    int out_off, patch_off;                // LDS byte offsets of L1's output planes and of its f32 input patch
    StackConv L[3];
};

// zero the 64-element slots behind the hi and lo planes of `npos` positions x PS at byte offset `off`
__device__ __forceinline__ void zero_slots(char* lds, int off, int npos, int PS, int tid) {
    if (tid < 32) {
        __bf16* h = reinterpret_cast<__bf16*>(lds + off);
        reinterpret_cast<unsigned*>(h + (size_t)npos * PS)[tid] = 0u;
        reinterpret_cast<unsigned*>(h + 2 * (size_t)npos * PS + 64)[tid] = 0u;
    }
}

// L1: thin_conv_lane_kernel<C0, KS> over the whole image (TH = OH), 512 threads = 16 slots x 32 output channels
template <int C0, int KS>
__device__ __forceinline__ void lane_layer(const StackArgs& p, char* lds, int b, int tid) {
    constexpr int NSLOT = 64 * NW / 32;
    const int n = tid & 31, slot = tid >> 5;
    const int PH = p.OH + KS - 1;
    const int QX = (p.OW + 3) >> 2;
    const int PW = 4 * QX + 4;
    float* P = reinterpret_cast<float*>(lds + p.patch_off);
    const float* img = p.in + (size_t)b * p.IH * p.IW * C0;
    for (int e = tid; e < C0 * PH * PW; e += 64 * NW) {
        const int c = e / (PH * PW);
        const int r = e - c * PH * PW;
        const int py = r / PW, px = r - py * PW;
        const int gy = p.off + py, gx = p.off + px;
        float v = 0.f;
        if ((unsigned)gy < (unsigned)p.IH && (unsigned)gx < (unsigned)p.IW) v = img[(gy * p.IW + gx) * C0 + c];
        P[e] = v;
    }
    float wr[C0][KS][KS];
#pragma unroll
    for (int c = 0; c < C0; ++c)
#pragma unroll
        for (int jy = 0; jy < KS; ++jy)
#pragma unroll
            for (int jx = 0; jx < KS; ++jx) wr[c][jy][jx] = p.w[(jy * KS + jx) * p.wts + c * p.wcs + n * p.wns];
    const float bv = p.bias ? p.bias[n] : 0.f;
    const int PS = p.N + 8;
    unsigned short* Qh = reinterpret_cast<unsigned short*>(lds + p.out_off);
    unsigned short* Ql = Qh + (size_t)p.OH * p.OW * PS + 64;
    __syncthreads();                                                    // the patch
    for (int item = slot; item < p.OH * QX; item += NSLOT) {
        const int y = item / QX, qx = item - y * QX;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < C0; ++c)
#pragma unroll
            for (int jy = 0; jy < KS; ++jy) {
                const float* row = P + (c * PH + y + jy) * PW + 4 * qx;
                const f32x4 x0 = *reinterpret_cast<const f32x4*>(row);
                const f32x4 x1 = *reinterpret_cast<const f32x4*>(row + 4);
                const float xv[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
#pragma unroll
                for (int jx = 0; jx < KS; ++jx)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = fmaf(xv[j + jx], wr[c][jy][jx], acc[j]);
            }
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float xx = acc[j] + bv;
            xx = pm_act(xx, PM_ACT_LEAKY, p.slope);
            asm volatile("" : "+v"(xx));
            v[j] = xx;
        }
        const int nv = p.OW - 4 * qx < 4 ? p.OW - 4 * qx : 4;          // valid positions of the item
        const int pos0 = y * p.OW + 4 * qx;
        const size_t o0 = ((size_t)b * p.OH * p.OW + pos0) * p.N + n;
        unsigned h01, l01, h23, l23;
        split2(v[0], v[1], h01, l01);
        split2(v[2], v[3], h23, l23);
        const unsigned hv[4] = {h01 & 0xffffu, h01 >> 16, h23 & 0xffffu, h23 >> 16};
        const unsigned lv[4] = {l01 & 0xffffu, l01 >> 16, l23 & 0xffffu, l23 >> 16};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nv) {
                p.out[o0 + (size_t)j * p.N] = v[j];
                Qh[(pos0 + j) * PS + n] = (unsigned short)hv[j];
                Ql[(pos0 + j) * PS + n] = (unsigned short)lv[j];
            }
    }
}

// L2 - L4: image_conv_bf16_kernel<NW, T, true>'s k-loop over input planes already in LDS; the epilogue also writes the
// hi / lo planes of the next layer when L.out_off >= 0
template <int T>
__device__ __forceinline__ void image_layer(const StackConv& L, char* lds, int b, int wave, int lane, float slope) {
    constexpr int NSET = 4;
    const int i = lane & 31;
    const int h = lane >> 5;
    const int PS = L.C + 8;
    const int cch = L.C / BK;
    const int nsteps = L.KH * L.KW * cch;
    const int npos = L.IH * L.IW;
    const __bf16* Ph = reinterpret_cast<const __bf16*>(lds + L.in_off);
    const __bf16* Pl = Ph + (size_t)npos * PS + 64;
    const int zoff = npos * PS;
    const int ct = wave / L.wct, rt0 = wave - ct * L.wct;
    const int Mi = L.OH * L.OW;
    if (ct >= L.nct || rt0 * 32 >= Mi) return;                          // wave-uniform: no tile for this wave
    const int n = ct * 32 + i;
    const int ncl = (n < L.npad ? n : 0) * BK + 8 * h;

    bf16x8 bq[NSET][4];
    auto load_b = [&](int s, bf16x8 (&bb)[4]) {
        const int sc = s < nsteps ? s : nsteps - 1;
        const __bf16* src = L.ws + (size_t)sc * L.npad * BK + ncl;
        bb[0] = *reinterpret_cast<const bf16x8*>(src);
        bb[1] = *reinterpret_cast<const bf16x8*>(src + L.plane);
        bb[2] = *reinterpret_cast<const bf16x8*>(src + 16);
        bb[3] = *reinterpret_cast<const bf16x8*>(src + L.plane + 16);
    };
    load_b(0, bq[0]);
    load_b(1, bq[1]);
    load_b(2, bq[2]);
    load_b(3, bq[3]);

    int py[T], px[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int m = 32 * (rt0 + j * L.wct) + i;
        const int oy = m / L.OW, ox = m - oy * L.OW;
        py[j] = m < Mi ? oy * L.a + L.off : ROW_INVALID;
        px[j] = ox * L.a + L.offx;
    }
    f32x16 acc[T];
#pragma unroll
    for (int j = 0; j < T; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

    bf16x8 a[4][4];
    struct Tap { int dy, dx, c0; };
    int wky = 0, wkx = 0, wcc = 0;
    auto advance = [&]() -> Tap {
        const Tap t{wky * L.cs, wkx * L.cs, wcc * BK};
        if (++wcc == cch) {
            wcc = 0;
            if (++wkx == L.KW) {
                wkx = 0;
                ++wky;
            }
        }
        return t;
    };
    auto read_a = [&](const Tap& k, int j, bf16x8 (&aa)[4]) {
        const int iy = py[j] + k.dy, ix = px[j] + k.dx;
        const bool ok = (unsigned)iy < (unsigned)L.IH && (unsigned)ix < (unsigned)L.IW;
        const int o = (ok ? (iy * L.IW + ix) * PS + k.c0 : zoff) + 8 * h;
        aa[0] = *reinterpret_cast<const bf16x8*>(Ph + o);
        aa[1] = *reinterpret_cast<const bf16x8*>(Ph + o + 16);
        aa[2] = *reinterpret_cast<const bf16x8*>(Pl + o);
        aa[3] = *reinterpret_cast<const bf16x8*>(Pl + o + 16);
    };
    Tap t0, t1, t2;
    auto step = [&](int s, auto uc) {
        constexpr int u = decltype(uc)::value;
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int cur = (u * T + j) & 3;
            const int jn = j + 2;
            read_a(jn / T == 0 ? t0 : jn / T == 1 ? t1 : t2, jn % T, a[(cur + 2) & 3]);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq[u][0], a[cur][0], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq[u][1], a[cur][0], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq[u][0], a[cur][2], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq[u][2], a[cur][1], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq[u][3], a[cur][1], acc[j], 0, 0, 0);
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bq[u][2], a[cur][3], acc[j], 0, 0, 0);
        }
        t0 = t1;
        t1 = t2;
        t2 = advance();
        load_b(s + NSET, bq[u]);
        __builtin_amdgcn_sched_barrier(0);
    };
    using U0 = std::integral_constant<int, 0>;
    using U1 = std::integral_constant<int, 1>;
    using U2 = std::integral_constant<int, 2>;
    using U3 = std::integral_constant<int, 3>;
    static_assert(T == 1 || T == 2 || T == 4, "item index mod 4 must be static inside a group of NSET k-steps");
    t0 = advance();
    t1 = advance();
    t2 = advance();
    read_a(t0, 0, a[0]);
    read_a(T == 1 ? t1 : t0, T == 1 ? 0 : 1, a[1]);
    int s0 = 0;
    for (; s0 + NSET <= nsteps; s0 += NSET) {
        step(s0, U0{});
        step(s0 + 1, U1{});
        step(s0 + 2, U2{});
        step(s0 + 3, U3{});
    }
    if (s0 < nsteps) {
        step(s0, U0{});
        if (s0 + 1 < nsteps) {
            step(s0 + 1, U1{});
            if (s0 + 2 < nsteps) step(s0 + 2, U2{});
        }
    }

    // pm_epilogue_tile_t (bias, leaky; no aux / residual) + the split of the same values into the next layer's planes
    const int PSq = L.N + 8;
    __bf16* Qh = reinterpret_cast<__bf16*>(lds + (L.out_off >= 0 ? L.out_off : 0));
    __bf16* Ql = Qh + (size_t)Mi * PSq + 64;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int m = 32 * (rt0 + j * L.wct) + i;
        f32x4 v[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = ct * 32 + 8 * g + 4 * h;
            const int cc = c < L.N ? c : 0;
            const f32x4 bv = L.bias ? *reinterpret_cast<const f32x4*>(L.bias + cc) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float x = acc[j][4 * g + q] + bv[q];
                x = pm_act(x, PM_ACT_LEAKY, slope);
                asm volatile("" : "+v"(x));
                v[g][q] = x;
            }
        }
        if (m >= Mi) continue;
        float* orow = L.out + ((long long)b * Mi + m) * L.N;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = ct * 32 + 8 * g + 4 * h;
            if (c >= L.N) continue;
            *reinterpret_cast<f32x4*>(orow + c) = v[g];
            if (L.out_off >= 0) {
                unsigned h0, l0, h1, l1;
                split2(v[g][0], v[g][1], h0, l0);
                split2(v[g][2], v[g][3], h1, l1);
                *reinterpret_cast<u32x2*>(Qh + m * PSq + c) = u32x2{h0, h1};
                *reinterpret_cast<u32x2*>(Ql + m * PSq + c) = u32x2{l0, l1};
            }
        }
    }
}

template <int C0, int KS, int T2, int T3, int T4>
__global__ __launch_bounds__(64 * NW, 1) void conv_stack_fwd_bf16_kernel(StackArgs p) {
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    char* lds = reinterpret_cast<char*>(dsm);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    zero_slots(lds, p.out_off, p.OH * p.OW, p.N + 8, tid);
    lane_layer<C0, KS>(p, lds, b, tid);
    __syncthreads();                                                    // L1's planes; the patch is dead
    zero_slots(lds, p.L[0].out_off, p.L[0].OH * p.L[0].OW, p.L[0].N + 8, tid);
    image_layer<T2>(p.L[0], lds, b, wave, lane, p.slope);
    __syncthreads();                                                    // L2's planes; L1's are dead
    zero_slots(lds, p.L[1].out_off, p.L[1].OH * p.L[1].OW, p.L[1].N + 8, tid);
    image_layer<T3>(p.L[1], lds, b, wave, lane, p.slope);
    __syncthreads();                                                    // L3's planes
    image_layer<T4>(p.L[2], lds, b, wave, lane, p.slope);
}

// ------------------------------------------------------------ host side ------------------------------------------------------
struct StackPlan {
    size_t lds;
    int c0, t[3];
};

inline size_t planes_bytes(int npos, int C) { return 2 * ((size_t)npos * (C + 8) + 64) * 2; }
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

bool plan_stack(const pm_gather_desc* d, int nl, StackPlan& sp, StackArgs* args) {
    if (!d || nl != 4) return false;
    const int B = d[0].B;
    if (B < 1) return false;
    for (int l = 0; l < 4; ++l) {
        const pm_gather_desc& x = d[l];
        if (x.B != B || x.groups != 1 || x.d != 1 || x.cs != 1 || x.off_x != x.off || x.kws != x.KW) return false;
        if (x.in_act != PM_ACT_NONE || x.out_act != PM_ACT_LEAKY || x.aux_act != PM_ACT_NONE || x.slope != d[0].slope)
            return false;
        if (x.a < 1 || x.IH < 1 || x.IW < 1 || x.OH < 1 || x.OW < 1 || x.C < 1 || x.N < 1 || x.KH < 1 || x.KW < 1) return false;
        if (x.wts < 0 || x.wcs < 0 || x.wns < 0) return false;
        if ((long long)B * x.OH * x.OW * x.N >= 0x7fffffffLL || (long long)B * x.IH * x.IW * x.C >= 0x7fffffffLL) return false;
        if (l > 0 && (x.IH != d[l - 1].OH || x.IW != d[l - 1].OW || x.C != d[l - 1].N)) return false;
        if (x.off < -64 || x.off > 64) return false;
    }
    // L1: the lane form (a = 1, 5x5, C0 in {1, 2}, exactly 32 output channels: lane = channel)
    const pm_gather_desc& f = d[0];
    if (f.a != 1 || f.KH != 5 || f.KW != 5 || (f.C != 1 && f.C != 2) || f.N != 32 || f.OW > 128 || f.OH > 128) return false;
    if ((long long)(f.KH * f.KW - 1) * f.wts + (long long)(f.C - 1) * f.wcs + 31LL * f.wns >= 0x7fffffffLL) return false;
    // L2 - L4: plan_image's qualification (pm_conv.hip), 8 waves, a column tile per 8 / nct waves
    size_t in_bytes[3];
    for (int l = 1; l < 4; ++l) {
        const pm_gather_desc& x = d[l];
        if (x.C % BK != 0 || x.KH * x.KW < 4 || x.KH > 16 || x.KW > 16 || x.IH < x.KH || x.IW < x.KW || x.OH * x.OW < 32)
            return false;
        if (x.N % 4 != 0) return false;                                  // the TR epilogue's 16-byte column runs
        if (x.KH * x.KW * (x.C / BK) > 2048) return false;
        const int nct = (x.N + 31) / 32;
        if (nct > NW || NW % nct != 0) return false;
        const int wct = NW / nct;
        const int rt = (x.OH * x.OW + 31) / 32;
        int t = (rt + wct - 1) / wct;
        if (t == 3) t = 4;
        if (t > 4) return false;
        sp.t[l - 1] = t;
        in_bytes[l - 1] = planes_bytes(x.IH * x.IW, x.C);
        if (args) {
            StackConv& L = args->L[l - 1];
            L.IH = x.IH; L.IW = x.IW; L.C = x.C; L.OH = x.OH; L.OW = x.OW; L.N = x.N; L.KH = x.KH; L.KW = x.KW;
            L.a = x.a; L.cs = x.cs; L.off = x.off; L.offx = x.off_x;
            L.npad = nct * 32; L.nct = nct; L.wct = wct;
            L.plane = (long long)x.KH * x.KW * (x.C / BK) * BK * L.npad;
        }
    }
    // the instantiated deal: 28 x 28 -> 14 x 14 (s2) -> 14 x 14 -> 7 x 7 (s2) with 32 / 64 / 64 columns
    if (sp.t[0] != 1 || sp.t[1] != 2 || sp.t[2] != 1) return false;
    const size_t patch = (size_t)f.C * (f.OH + f.KH - 1) * (4 * ((f.OW + 3) / 4) + 4) * 4;
    const size_t x_bytes = align16(in_bytes[0] > in_bytes[2] ? in_bytes[0] : in_bytes[2]);
    const size_t y_bytes = in_bytes[1] > patch ? in_bytes[1] : patch;
    sp.lds = x_bytes + y_bytes;
    if (sp.lds > LDS_MAX) return false;
    sp.c0 = f.C;
    if (args) {
        args->IH = f.IH; args->IW = f.IW; args->OH = f.OH; args->OW = f.OW; args->N = f.N; args->off = f.off;
        args->wts = f.wts; args->wcs = f.wcs; args->wns = f.wns; args->slope = f.slope;
        args->out_off = 0;
        args->patch_off = (int)x_bytes;
        args->L[0].in_off = 0;                 args->L[0].out_off = (int)x_bytes;   // L2: X -> Y
        args->L[1].in_off = (int)x_bytes;      args->L[1].out_off = 0;              // L3: Y -> X
        args->L[2].in_off = 0;                 args->L[2].out_off = -1;             // L4: X -> HBM only
    }
    return true;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int C0>
void launch_stack(hipStream_t s, const StackPlan& sp, const StackArgs& a, int B) {
    static bool attr = false;
    if (!attr) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_stack_fwd_bf16_kernel<C0, 5, 1, 2, 1>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_MAX);
        attr = true;
    }
    PM_KTAG("conv_stack_fwd_bf16_kernel<%d, 5, 1, 2, 1>", C0);
    hipLaunchKernelGGL((conv_stack_fwd_bf16_kernel<C0, 5, 1, 2, 1>), dim3((unsigned)B), dim3(64 * NW), sp.lds, s, a);
}

}  // namespace

extern "C" int pm_conv_stack_plan(const pm_gather_desc* layers, int nlayers, long long* lds_bytes) {
    StackPlan sp;
    if (!plan_stack(layers, nlayers, sp, nullptr)) return PM_EINVAL;
    if (lds_bytes) *lds_bytes = (long long)sp.lds;
    return PM_OK;
}

extern "C" int pm_conv_stack_fwd_bf16(pm_stream_t stream, const pm_gather_desc* layers, int nlayers, const float* in,
                                      const float* w0, const void* const* wsplit, const float* const* bias, float* const* out) {
    StackPlan sp;
    StackArgs a;
    if (!plan_stack(layers, nlayers, sp, &a) || !in || !w0 || !wsplit || !bias || !out) return PM_EINVAL;
    for (int l = 0; l < 4; ++l) {
        if (!out[l] || !al16(out[l]) || (bias[l] && !al16(bias[l]))) return PM_EINVAL;
        if (l > 0 && (!wsplit[l] || !al16(wsplit[l]))) return PM_EINVAL;
    }
    a.in = in; a.w = w0; a.bias = bias[0]; a.out = out[0];
    for (int l = 1; l < 4; ++l) {
        a.L[l - 1].ws = reinterpret_cast<const __bf16*>(wsplit[l]);
        a.L[l - 1].bias = bias[l];
        a.L[l - 1].out = out[l];
    }
    hipStream_t s = (hipStream_t)stream;
    if (sp.c0 == 1) launch_stack<1>(s, sp, a, layers[0].B);
    else launch_stack<2>(s, sp, a, layers[0].B);
    return pm_check_launch("pm_conv_stack_fwd_bf16");
}
