// gmm_rate_kernels.hip -- the GMM rate loss of the training objective as one pass over NCHW data, forward and backward (DESIGN.md "Fused GMM rate loss").
// The reference trains on  sum(EntropyGmm(softmax(ContextReshape(w)), relu(ContextReshape(s)) + 1e-5, ContextReshape(m), label) * mask)
// (train/EntropyNet2.py:67-74, train/model_zoo.py:295-296): three transposed copies, a softmax, a ReLU, the loss kernel with four gradient buffers,
// a product and a sum.  Every element of that depends on the nine parameters, the label and the mask of its own symbol only, so:
//   * k_gmm_rate<NG, VEC>: a workgroup of 256 threads owns GR_CHUNK = 1024 consecutive cells (y * W + x: lanes run along x) of one (n, g) plane, four
//     cells per thread.  Symbol (n, g, y, x) reads channel g * ng + i of each net -- the element ContextReshape puts in row ((n G + g) H + y) W + x,
//     column i.  VEC: thread t holds cells 4 t .. 4 t + 3 and moves them with 16-byte accesses (W % 4 == 0 and every base 16-byte aligned); otherwise
//     cells t, t + 256, t + 512, t + 768 with 4-byte accesses.  The mask is read first; a wave none of whose cells is coded (mask >= 0.5, the coder's
//     rule) reads no parameter and does no arithmetic.  NG > 0 (3 in production) keeps a symbol's parameters in registers; NG == 0 takes ng (1..16) at
//     run time and streams over the components in passes that read them again (L1/L2 hits), so no array is indexed at run time and nothing goes
//     to scratch memory.  Each coded symbol's fp32 loss is added in double: a thread's cells in index order, then plane_walk.h's workgroup sum
//     (total and count to the workgroup's scratch slot) and its finish kernel, which adds an image's slots in index order.  No atomics: the same
//     bits on every call.
//   * k_gmm_rate_backward<NG, VEC, LABEL>: the same walk; recomputes the symbol from the inputs and writes d_logit, d_sigma, d_mean (and d_label)
//     in place of the reads, exact zeros for uncoded cells.
// Arithmetic (the contract of DESIGN.md, restated in tests/gmm_rate_cases.py): lic360_softmax_inplace's order, the sigma floor, then k_entropy_gmm's
// per-component body (csrc/tile_table_kernels.hip) stated a second time in gmm_component below -- that kernel is untouched.
#include "common.h"
#include "lic360_exact_math.h"
#include "plane_walk.h"

namespace {
constexpr int GR_THREADS = 256, GR_PER_THREAD = 4, GR_CHUNK = GR_THREADS * GR_PER_THREAD, GR_MAX_NG = 16;
constexpr float GR_SIGMA_FLOOR = 0.00001f;

// one struct by value: the number of arguments of a launch costs like their bytes do (DESIGN.md 4.1 b'')
struct GmmRateArgs {
    const float *logit, *sigma, *mean, *label, *mask;   // mask: null = every symbol coded
    const float *grad;                                  // backward: grad_nats [N]
    float *o_logit, *o_sigma, *o_mean, *o_label;        // backward: the gradients; forward: o_label is the map (or null)
    PlaneSlots<1> slots;                                // forward: one slot per workgroup (total, coded symbols)
    int G, ng, HW, chunks;                              // chunks: workgroups per plane
};

struct GmmComp { float p, lw, dd, md; };
// one mixture component of k_entropy_gmm: p = Phi_b - Phi_a, and the terms of the label, sigma and mean gradients before the 1 / sum_p factor
LIC360_HD GmmComp gmm_component(float w, float s, float mu, float lab) {
    const float s2 = 0x1.6a09e6p-1f, sp2 = 0x1.988454p-2f;
    float xa = (float)((double)lab - 0.5 - (double)mu);
    float xb = (float)((double)lab + 0.5 - (double)mu);
    float id = (float)(1.0 / (double)s);
    float fa = (float)(0.5 + 0.5 * (double)lic360_erff(xa * id * s2));
    float fb = (float)(0.5 + 0.5 * (double)lic360_erff(xb * id * s2));
    float ga = sp2 * id * lic360_expf((float)(-0.5 * (double)xa * (double)xa * (double)id * (double)id));
    float gb = sp2 * id * lic360_expf((float)(-0.5 * (double)xb * (double)xb * (double)id * (double)id));
    GmmComp c;
    c.p = fb - fa;
    c.lw = (gb - ga) * w;
    c.dd = id * (-xb * gb + xa * ga) * w;
    c.md = (ga - gb) * w;
    return c;
}
LIC360_HD float gmm_sigma(float raw) { return raw > 0.0f ? raw + GR_SIGMA_FLOOR : GR_SIGMA_FLOOR; }
LIC360_HD float gmm_loss(float sum_p) { return -lic360_logf((float)((double)sum_p + 0.0000001)); }
LIC360_HD float gmm_inv_p(float sum_p) { return (float)(-1.0 / ((double)sum_p + 0.0000001)); }

// the plane walk of this loss, and which of the thread's cells are coded
template <bool VEC>
struct Walk : PlaneWalk<GR_THREADS, GR_PER_THREAD, VEC> {
    using PlaneWalk<GR_THREADS, GR_PER_THREAD, VEC>::plane;
    using PlaneWalk<GR_THREADS, GR_PER_THREAD, VEC>::cells;
    bool coded[GR_PER_THREAD];
    bool any;                  // a cell of this WAVE is coded
    __device__ __forceinline__ Walk(const GmmRateArgs &a) : PlaneWalk<GR_THREADS, GR_PER_THREAD, VEC>(a.chunks, a.G, a.HW) {
        float m[GR_PER_THREAD];
        if (a.mask) cells.load(a.mask + plane * a.HW, m);
        bool mine = false;
#pragma unroll
        for (int k = 0; k < GR_PER_THREAD; ++k) {
            coded[k] = cells.inside(k) && (!a.mask || m[k] >= 0.5f);
            mine |= coded[k];
        }
        any = __ballot(mine) != 0;
    }
};

// loss (and, BWD, the gradients written over L, S, M, lab) of the coded cells among this thread's four, parameters in registers
template <int NG, bool BWD>
__device__ __forceinline__ void gmm_cells_static(float (&L)[NG][GR_PER_THREAD], float (&S)[NG][GR_PER_THREAD], float (&M)[NG][GR_PER_THREAD],
                                                 float (&lab)[GR_PER_THREAD], const bool (&coded)[GR_PER_THREAD], float t, float (&loss)[GR_PER_THREAD]) {
#pragma unroll
    for (int k = 0; k < GR_PER_THREAD; ++k) {
        loss[k] = 0.0f;
        if (coded[k]) {
            float w[NG];
            GmmComp c[NG];
#pragma unroll
            for (int i = 0; i < NG; ++i) w[i] = L[i][k];
            lic360_softmax_inplace(w, NG);
            float sum_p = 0.0f, l = 0.0f;
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                c[i] = gmm_component(w[i], gmm_sigma(S[i][k]), M[i][k], lab[k]);
                sum_p = __builtin_fmaf(w[i], c[i].p, sum_p);
                l += c[i].lw;
            }
            loss[k] = gmm_loss(sum_p);
            if (BWD) {
                const float ip = gmm_inv_p(sum_p);
                float gw[NG], dot = 0.0f;
#pragma unroll
                for (int i = 0; i < NG; ++i) {
                    gw[i] = c[i].p * ip * t;
                    dot = __builtin_fmaf(gw[i], w[i], dot);
                }
#pragma unroll
                for (int i = 0; i < NG; ++i) {
                    L[i][k] = w[i] * (gw[i] - dot);
                    S[i][k] = S[i][k] > 0.0f ? c[i].dd * ip * t : 0.0f;
                    M[i][k] = c[i].md * ip * t;
                }
                lab[k] = l * ip * t;
            }
        } else if (BWD) {
#pragma unroll
            for (int i = 0; i < NG; ++i) L[i][k] = S[i][k] = M[i][k] = 0.0f;
            lab[k] = 0.0f;
        }
    }
}

// the same with ng at run time: passes over the components that read the planes again, accumulators only
template <bool VEC, bool BWD, bool LABEL>
__device__ __forceinline__ void gmm_cells_stream(const GmmRateArgs &a, const Walk<VEC> &wk, float t, float (&loss)[GR_PER_THREAD]) {
    const long HW = a.HW, base = wk.plane * a.ng * HW;
    const float *pl = a.logit + base, *ps = a.sigma + base, *pm = a.mean + base;
    float lab[GR_PER_THREAD], mx[GR_PER_THREAD], sm[GR_PER_THREAD], sum_p[GR_PER_THREAD], l[GR_PER_THREAD], v[GR_PER_THREAD], s[GR_PER_THREAD], m[GR_PER_THREAD];
    wk.cells.load(a.label + wk.plane * HW, lab);
    for (int i = 0; i < a.ng; ++i) {                                       // the maximum, lic360_softmax_inplace's way
        wk.cells.load(pl + i * HW, v);
#pragma unroll
        for (int k = 0; k < GR_PER_THREAD; ++k) mx[k] = (i == 0 || mx[k] < v[k]) ? v[k] : mx[k];
    }
#pragma unroll
    for (int k = 0; k < GR_PER_THREAD; ++k) sm[k] = sum_p[k] = l[k] = loss[k] = 0.0f;
    for (int i = 0; i < a.ng; ++i) {                                       // the sum, in index order
        wk.cells.load(pl + i * HW, v);
#pragma unroll
        for (int k = 0; k < GR_PER_THREAD; ++k)
            if (wk.coded[k]) sm[k] = sm[k] + lic360_expf(v[k] - mx[k]);
    }
    for (int i = 0; i < a.ng; ++i) {
        wk.cells.load(pl + i * HW, v);
        wk.cells.load(ps + i * HW, s);
        wk.cells.load(pm + i * HW, m);
#pragma unroll
        for (int k = 0; k < GR_PER_THREAD; ++k)
            if (wk.coded[k]) {
                const float w = lic360_expf(v[k] - mx[k]) / sm[k];
                const GmmComp c = gmm_component(w, gmm_sigma(s[k]), m[k], lab[k]);
                sum_p[k] = __builtin_fmaf(w, c.p, sum_p[k]);
                l[k] += c.lw;
            }
    }
#pragma unroll
    for (int k = 0; k < GR_PER_THREAD; ++k)
        if (wk.coded[k]) loss[k] = gmm_loss(sum_p[k]);
    if (!BWD) return;
    float ip[GR_PER_THREAD], dot[GR_PER_THREAD];
#pragma unroll
    for (int k = 0; k < GR_PER_THREAD; ++k) {
        ip[k] = wk.coded[k] ? gmm_inv_p(sum_p[k]) : 0.0f;
        dot[k] = 0.0f;
    }
    for (int i = 0; i < a.ng; ++i) {
        wk.cells.load(pl + i * HW, v);
        wk.cells.load(ps + i * HW, s);
        wk.cells.load(pm + i * HW, m);
#pragma unroll
        for (int k = 0; k < GR_PER_THREAD; ++k)
            if (wk.coded[k]) {
                const float w = lic360_expf(v[k] - mx[k]) / sm[k];
                const GmmComp c = gmm_component(w, gmm_sigma(s[k]), m[k], lab[k]);
                dot[k] = __builtin_fmaf(c.p * ip[k] * t, w, dot[k]);
            }
    }
    for (int i = 0; i < a.ng; ++i) {
        wk.cells.load(pl + i * HW, v);
        wk.cells.load(ps + i * HW, s);
        wk.cells.load(pm + i * HW, m);
#pragma unroll
        for (int k = 0; k < GR_PER_THREAD; ++k) {
            float dl = 0.0f, ds = 0.0f, dm = 0.0f;
            if (wk.coded[k]) {
                const float w = lic360_expf(v[k] - mx[k]) / sm[k];
                const GmmComp c = gmm_component(w, gmm_sigma(s[k]), m[k], lab[k]);
                dl = w * (c.p * ip[k] * t - dot[k]);
                ds = s[k] > 0.0f ? c.dd * ip[k] * t : 0.0f;
                dm = c.md * ip[k] * t;
            }
            v[k] = dl; s[k] = ds; m[k] = dm;
        }
        wk.cells.store(a.o_logit + base + i * HW, v);
        wk.cells.store(a.o_sigma + base + i * HW, s);
        wk.cells.store(a.o_mean + base + i * HW, m);
    }
    if (LABEL) {
#pragma unroll
        for (int k = 0; k < GR_PER_THREAD; ++k) v[k] = wk.coded[k] ? l[k] * ip[k] * t : 0.0f;
        wk.cells.store(a.o_label + wk.plane * HW, v);
    }
}

template <int NG, bool VEC>
__global__ __launch_bounds__(GR_THREADS) void k_gmm_rate(const GmmRateArgs a) {
    const Walk<VEC> wk(a);
    const long HW = a.HW;
    float loss[GR_PER_THREAD] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (wk.any) {
        if constexpr (NG > 0) {
            constexpr int N_ = NG;
            float L[N_][GR_PER_THREAD], S[N_][GR_PER_THREAD], M[N_][GR_PER_THREAD], lab[GR_PER_THREAD];
            const long base = wk.plane * N_ * HW;
#pragma unroll
            for (int i = 0; i < N_; ++i) {
                wk.cells.load(a.logit + base + i * HW, L[i]);
                wk.cells.load(a.sigma + base + i * HW, S[i]);
                wk.cells.load(a.mean + base + i * HW, M[i]);
            }
            wk.cells.load(a.label + wk.plane * HW, lab);
            gmm_cells_static<N_, false>(L, S, M, lab, wk.coded, 0.0f, loss);
        } else {
            gmm_cells_stream<VEC, false, false>(a, wk, 0.0f, loss);
        }
    }
    if (a.o_label) wk.cells.store(a.o_label + wk.plane * HW, loss);          // the map: 0 where uncoded
    double acc = 0.0;
    int cnt[1] = {0};
#pragma unroll
    for (int k = 0; k < GR_PER_THREAD; ++k)
        if (wk.coded[k]) { acc += (double)loss[k]; ++cnt[0]; }
    block_sum_to_slot<GR_THREADS, 1>(acc, cnt, a.slots);
}

template <int NG, bool VEC, bool LABEL>
__global__ __launch_bounds__(GR_THREADS) void k_gmm_rate_backward(const GmmRateArgs a) {
    const Walk<VEC> wk(a);
    const long HW = a.HW;
    const float t = a.grad[wk.n];
    float loss[GR_PER_THREAD];
    if constexpr (NG == 0) {
        if (wk.any) {
            gmm_cells_stream<VEC, true, LABEL>(a, wk, t, loss);
            return;
        }
    }
    constexpr int N_ = NG > 0 ? NG : 1;
    const int ng = NG > 0 ? NG : a.ng;
    const long base = wk.plane * ng * HW;
    if constexpr (NG > 0) if (wk.any) {
        float L[N_][GR_PER_THREAD], S[N_][GR_PER_THREAD], M[N_][GR_PER_THREAD], lab[GR_PER_THREAD];
#pragma unroll
        for (int i = 0; i < N_; ++i) {
            wk.cells.load(a.logit + base + i * HW, L[i]);
            wk.cells.load(a.sigma + base + i * HW, S[i]);
            wk.cells.load(a.mean + base + i * HW, M[i]);
        }
        wk.cells.load(a.label + wk.plane * HW, lab);
        gmm_cells_static<N_, true>(L, S, M, lab, wk.coded, t, loss);
#pragma unroll
        for (int i = 0; i < N_; ++i) {
            wk.cells.store(a.o_logit + base + i * HW, L[i]);
            wk.cells.store(a.o_sigma + base + i * HW, S[i]);
            wk.cells.store(a.o_mean + base + i * HW, M[i]);
        }
        if (LABEL) wk.cells.store(a.o_label + wk.plane * HW, lab);
        return;
    }
    const float zero[GR_PER_THREAD] = {0.0f, 0.0f, 0.0f, 0.0f};                // a wave without a coded cell: zeros, nothing read but the mask
    for (int i = 0; i < ng; ++i) {
        wk.cells.store(a.o_logit + base + i * HW, zero);
        wk.cells.store(a.o_sigma + base + i * HW, zero);
        wk.cells.store(a.o_mean + base + i * HW, zero);
    }
    if (LABEL) wk.cells.store(a.o_label + wk.plane * HW, zero);
}

int gmm_rate_geometry(int n, int g, int h, int w, int ng, int *chunks, long *groups) { return plane_walk_geometry(n, g, h, w, ng, GR_CHUNK, chunks, groups); }
bool aligned16(const void *p) { return plane_walk_aligned(p, 4 * GR_PER_THREAD); }
}  // namespace

LIC360_API long lic360_gmm_rate_scratch_bytes(int n, int g, int h, int w) {
    int chunks;
    long groups;
    if (n <= 0 || g <= 0 || h <= 0 || w <= 0 || gmm_rate_geometry(n, g, h, w, GR_MAX_NG, &chunks, &groups)) return 0;
    return plane_slots_bytes<1>(groups);
}

LIC360_API int lic360_gmm_rate(void *stream, const float *logit, const float *sigma, const float *mean, const float *label, const float *mask,
                               int n, int g, int h, int w, int ng, double *nats, long long *symbols, float *map, void *scratch) {
    ARG_CHECK(n >= 0 && g >= 0 && h >= 0 && w >= 0);
    ARG_CHECK(ng >= 1 && ng <= GR_MAX_NG);
    hipStream_t s = (hipStream_t)stream;
    long long *const totals[1] = {symbols};
    if (n == 0 || g == 0 || h == 0 || w == 0) return plane_walk_no_symbol(s, n, nats, totals);
    ARG_CHECK(logit && sigma && mean && label && nats && symbols && scratch);
    int chunks;
    long groups;
    ARG_CHECK(!gmm_rate_geometry(n, g, h, w, ng, &chunks, &groups));
    ARG_CHECK(((uintptr_t)scratch & 7) == 0);
    const GmmRateArgs a{logit, sigma, mean, label, mask, nullptr, nullptr, nullptr, nullptr, map, plane_slots_carve<1>(scratch, groups), g, ng, h * w, chunks};
    const bool vec = w % 4 == 0 && aligned16(logit) && aligned16(sigma) && aligned16(mean) && aligned16(label) && aligned16(mask) && aligned16(map);
    const dim3 grid((unsigned)groups), block(GR_THREADS);
    if (ng == 3 && vec) hipLaunchKernelGGL((k_gmm_rate<3, true>), grid, block, 0, s, a);
    else if (ng == 3) hipLaunchKernelGGL((k_gmm_rate<3, false>), grid, block, 0, s, a);
    else if (vec) hipLaunchKernelGGL((k_gmm_rate<0, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_gmm_rate<0, false>), grid, block, 0, s, a);
    LAUNCH_CHECK();
    plane_sum_finish_launch<GR_THREADS, 1>(s, n, g * chunks, a.slots, nats, totals);
    LAUNCH_CHECK();
    return 0;
}

LIC360_API int lic360_gmm_rate_backward(void *stream, const float *logit, const float *sigma, const float *mean, const float *label,
                                        const float *mask, const float *grad_nats, int n, int g, int h, int w, int ng, float *d_logit,
                                        float *d_sigma, float *d_mean, float *d_label) {
    ARG_CHECK(n >= 0 && g >= 0 && h >= 0 && w >= 0);
    ARG_CHECK(ng >= 1 && ng <= GR_MAX_NG);
    if (n == 0 || g == 0 || h == 0 || w == 0) return 0;
    ARG_CHECK(logit && sigma && mean && label && grad_nats && d_logit && d_sigma && d_mean);
    int chunks;
    long groups;
    ARG_CHECK(!gmm_rate_geometry(n, g, h, w, ng, &chunks, &groups));
    const GmmRateArgs a{logit, sigma, mean, label, mask, grad_nats, d_logit, d_sigma, d_mean, d_label, {}, g, ng, h * w, chunks};
    const bool vec = w % 4 == 0 && aligned16(logit) && aligned16(sigma) && aligned16(mean) && aligned16(label) && aligned16(mask) &&
                     aligned16(d_logit) && aligned16(d_sigma) && aligned16(d_mean) && aligned16(d_label);
    const dim3 grid((unsigned)groups), block(GR_THREADS);
    hipStream_t s = (hipStream_t)stream;
#define GR_BWD(NG_, VEC_, LAB_) hipLaunchKernelGGL((k_gmm_rate_backward<NG_, VEC_, LAB_>), grid, block, 0, s, a)
    if (ng == 3) {
        if (vec) { if (d_label) GR_BWD(3, true, true); else GR_BWD(3, true, false); }
        else { if (d_label) GR_BWD(3, false, true); else GR_BWD(3, false, false); }
    } else {
        if (vec) { if (d_label) GR_BWD(0, true, true); else GR_BWD(0, true, false); }
        else { if (d_label) GR_BWD(0, false, true); else GR_BWD(0, false, false); }
    }
#undef GR_BWD
    LAUNCH_CHECK();
    return 0;
}
