// ce_rate_kernels.hip -- the cross-entropy rate loss of the importance map's entropy model as one pass over NCHW logits, forward and backward
// (DESIGN.md "Fused cross-entropy rate loss").
// The reference trains on  CrossEntropyLoss(reduce=False)(ContextReshape(net(x)), x.view(-1).long())  (test/model_zoo.py:275-300): a transposed copy of
// the logits, a log-softmax and a gather; the backward adds a scatter and the adjoint copy.  Every element of that depends on the K logits and the
// label of its own symbol only, so:
//   * k_ce_rate<KS, VEC>: a workgroup of 128 threads owns CE_CHUNK = 256 consecutive cells (y * W + x: lanes run along x) of one (n, g) plane, two
//     cells per thread.  Symbol (n, g, y, x) reads channel g * K + i -- the element ContextReshape puts in row ((n G + g) H + y) W + x, column i.
//     VEC: thread t holds cells 2 t, 2 t + 1 and moves them with 8-byte accesses (W % 2 == 0 and every base 8-byte aligned); otherwise cells t,
//     t + 128 with 4-byte accesses.  KS > 0 (49 in production) keeps a symbol's logits in registers and reads them once: 2 x 49 live values per
//     thread; KS == 0 takes K (1..64) at run time and streams over the classes in passes that read them again (L1/L2 hits), so no array is indexed
//     at run time and nothing goes to scratch memory.  A symbol is valid iff label > -1 && label < K (NaN is not), its class (int)label.  Each valid
//     symbol's fp32 loss is added in double: a thread's cells in index order, then plane_walk.h's workgroup sum (total, count and the count of
//     invalid symbols to the workgroup's scratch slot) and its finish kernel, which adds an image's slots in index order.  No atomics: the same
//     bits on every call.
//   * k_ce_rate_backward<KS, VEC>: the same walk; recomputes the symbol from the inputs and writes d_logit in place of the reads, exact zeros for
//     invalid symbols.
// Arithmetic (the contract of DESIGN.md, restated in tests/ce_rate_cases.py), every operation rounded once in fp32:
//     m = l_0; for i = 1..K-1: if (m < l_i) m = l_i;   e_i = lic360_expf(l_i - m);   s = 0; s = s + e_i in index order
//     loss = lic360_logf(s) - (l_c - m);   backward, t = grad_nats[n]:  p_i = e_i / s,  d_logit_i = (i == c ? p_i - 1 : p_i) * t
#include "common.h"
#include "lic360_exact_math.h"
#include "plane_walk.h"

namespace {
constexpr int CE_THREADS = 128, CE_PER_THREAD = 2, CE_CHUNK = CE_THREADS * CE_PER_THREAD, CE_MAX_K = 64, CE_STATIC_K = 49;

// one struct by value: the number of arguments of a launch costs like their bytes do (DESIGN.md 4.1 b'')
struct CeRateArgs {
    const float *logit, *label;
    const float *grad;                                  // backward: grad_nats [N]
    float *out;                                         // forward: the map (or null); backward: d_logit
    PlaneSlots<2> slots;                                // forward: one slot per workgroup (total, valid symbols, invalid symbols)
    int G, K, HW, chunks;                               // chunks: workgroups per plane
};

// the plane walk of this loss, which of the thread's cells hold a valid label and its class
template <bool VEC>
struct CeWalk : PlaneWalk<CE_THREADS, CE_PER_THREAD, VEC> {
    using PlaneWalk<CE_THREADS, CE_PER_THREAD, VEC>::plane;
    using PlaneWalk<CE_THREADS, CE_PER_THREAD, VEC>::cells;
    bool valid[CE_PER_THREAD];
    int cls[CE_PER_THREAD];    // -1 where invalid
    __device__ __forceinline__ CeWalk(const CeRateArgs &a) : PlaneWalk<CE_THREADS, CE_PER_THREAD, VEC>(a.chunks, a.G, a.HW) {
        float lab[CE_PER_THREAD];
        cells.load(a.label + plane * a.HW, lab);
        const float top = (float)a.K;
#pragma unroll
        for (int k = 0; k < CE_PER_THREAD; ++k) {
            valid[k] = cells.inside(k) && lab[k] > -1.0f && lab[k] < top;           // NaN: neither comparison holds
            cls[k] = valid[k] ? (int)lab[k] : -1;                                  // truncated: -0.5 -> 0, 3.7 -> 3
        }
    }
};

// loss (and, BWD, d_logit written over L) of this thread's cells, logits in registers
template <int K, bool BWD>
__device__ __forceinline__ void ce_cells_static(float (&L)[K][CE_PER_THREAD], const bool (&valid)[CE_PER_THREAD], const int (&cls)[CE_PER_THREAD], float t,
                                                float (&loss)[CE_PER_THREAD]) {
#pragma unroll
    for (int k = 0; k < CE_PER_THREAD; ++k) {
        loss[k] = 0.0f;
        if (valid[k]) {
            float m = L[0][k];
#pragma unroll
            for (int i = 1; i < K; ++i) m = m < L[i][k] ? L[i][k] : m;
            float s = 0.0f, dc = 0.0f;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const float d = L[i][k] - m;
                const float e = lic360_expf(d);
                s = s + e;
                dc = i == cls[k] ? d : dc;
                if (BWD) L[i][k] = e;
            }
            loss[k] = lic360_logf(s) - dc;
            if (BWD) {
#pragma unroll
                for (int i = 0; i < K; ++i) {
                    const float p = L[i][k] / s;
                    L[i][k] = (i == cls[k] ? p - 1.0f : p) * t;
                }
            }
        } else if (BWD) {
#pragma unroll
            for (int i = 0; i < K; ++i) L[i][k] = 0.0f;
        }
    }
}

// the same with K at run time: passes over the classes that read the planes again, accumulators only
template <bool VEC, bool BWD>
__device__ __forceinline__ void ce_cells_stream(const CeRateArgs &a, const CeWalk<VEC> &wk, float t, float (&loss)[CE_PER_THREAD]) {
    const long HW = a.HW, base = wk.plane * a.K * HW;
    const float *pl = a.logit + base;
    float mx[CE_PER_THREAD], sm[CE_PER_THREAD], dc[CE_PER_THREAD], v[CE_PER_THREAD];
    for (int i = 0; i < a.K; ++i) {                                        // the maximum, lic360_softmax_inplace's way
        wk.cells.load(pl + i * HW, v);
#pragma unroll
        for (int k = 0; k < CE_PER_THREAD; ++k) mx[k] = (i == 0 || mx[k] < v[k]) ? v[k] : mx[k];
    }
#pragma unroll
    for (int k = 0; k < CE_PER_THREAD; ++k) sm[k] = dc[k] = loss[k] = 0.0f;
    for (int i = 0; i < a.K; ++i) {                                        // the sum, in index order
        wk.cells.load(pl + i * HW, v);
#pragma unroll
        for (int k = 0; k < CE_PER_THREAD; ++k)
            if (wk.valid[k]) {
                const float d = v[k] - mx[k];
                sm[k] = sm[k] + lic360_expf(d);
                dc[k] = i == wk.cls[k] ? d : dc[k];
            }
    }
#pragma unroll
    for (int k = 0; k < CE_PER_THREAD; ++k)
        if (wk.valid[k]) loss[k] = lic360_logf(sm[k]) - dc[k];
    if (!BWD) return;
    for (int i = 0; i < a.K; ++i) {
        wk.cells.load(pl + i * HW, v);
#pragma unroll
        for (int k = 0; k < CE_PER_THREAD; ++k) {
            float d = 0.0f;
            if (wk.valid[k]) {
                const float p = lic360_expf(v[k] - mx[k]) / sm[k];
                d = (i == wk.cls[k] ? p - 1.0f : p) * t;
            }
            v[k] = d;
        }
        wk.cells.store(a.out + base + i * HW, v);
    }
}

template <int KS, bool VEC>
__global__ __launch_bounds__(CE_THREADS) void k_ce_rate(const CeRateArgs a) {
    const CeWalk<VEC> wk(a);
    const long HW = a.HW;
    float loss[CE_PER_THREAD];
    if constexpr (KS > 0) {
        float L[KS][CE_PER_THREAD];
        const long base = wk.plane * KS * HW;
#pragma unroll
        for (int i = 0; i < KS; ++i) wk.cells.load(a.logit + base + i * HW, L[i]);
        ce_cells_static<KS, false>(L, wk.valid, wk.cls, 0.0f, loss);
    } else {
        ce_cells_stream<VEC, false>(a, wk, 0.0f, loss);
    }
    if (a.out) wk.cells.store(a.out + wk.plane * HW, loss);                  // the map: 0 where invalid
    double acc = 0.0;
    int cnt[2] = {0, 0};                                                     // valid, invalid
#pragma unroll
    for (int k = 0; k < CE_PER_THREAD; ++k) {
        if (wk.valid[k]) { acc += (double)loss[k]; ++cnt[0]; }
        else if (wk.cells.inside(k)) ++cnt[1];
    }
    block_sum_to_slot<CE_THREADS, 2>(acc, cnt, a.slots);
}

template <int KS, bool VEC>
__global__ __launch_bounds__(CE_THREADS) void k_ce_rate_backward(const CeRateArgs a) {
    const CeWalk<VEC> wk(a);
    const long HW = a.HW;
    const float t = a.grad[wk.n];
    float loss[CE_PER_THREAD];
    if constexpr (KS > 0) {
        float L[KS][CE_PER_THREAD];
        const long base = wk.plane * KS * HW;
#pragma unroll
        for (int i = 0; i < KS; ++i) wk.cells.load(a.logit + base + i * HW, L[i]);
        ce_cells_static<KS, true>(L, wk.valid, wk.cls, t, loss);
#pragma unroll
        for (int i = 0; i < KS; ++i) wk.cells.store(a.out + base + i * HW, L[i]);
    } else {
        ce_cells_stream<VEC, true>(a, wk, t, loss);
    }
}

int ce_rate_geometry(int n, int g, int h, int w, int k, int *chunks, long *groups) { return plane_walk_geometry(n, g, h, w, k, CE_CHUNK, chunks, groups); }
bool aligned8(const void *p) { return plane_walk_aligned(p, 4 * CE_PER_THREAD); }
}  // namespace

LIC360_API long lic360_ce_rate_scratch_bytes(int n, int g, int h, int w) {
    int chunks;
    long groups;
    if (n <= 0 || g <= 0 || h <= 0 || w <= 0 || ce_rate_geometry(n, g, h, w, CE_MAX_K, &chunks, &groups)) return 0;
    return plane_slots_bytes<2>(groups);
}

LIC360_API int lic360_ce_rate(void *stream, const float *logit, const float *label, int n, int g, int h, int w, int k, double *nats,
                              long long *symbols, long long *invalid, float *map, void *scratch) {
    ARG_CHECK(n >= 0 && g >= 0 && h >= 0 && w >= 0);
    ARG_CHECK(k >= 1 && k <= CE_MAX_K);
    hipStream_t s = (hipStream_t)stream;
    long long *const totals[2] = {symbols, invalid};
    if (n == 0 || g == 0 || h == 0 || w == 0) return plane_walk_no_symbol(s, n, nats, totals);
    ARG_CHECK(logit && label && nats && symbols && invalid && scratch);
    int chunks;
    long groups;
    ARG_CHECK(!ce_rate_geometry(n, g, h, w, k, &chunks, &groups));
    ARG_CHECK(((uintptr_t)scratch & 7) == 0);
    const CeRateArgs a{logit, label, nullptr, map, plane_slots_carve<2>(scratch, groups), g, k, h * w, chunks};
    const bool vec = w % 2 == 0 && aligned8(logit) && aligned8(label) && aligned8(map);
    const dim3 grid((unsigned)groups), block(CE_THREADS);
    if (k == CE_STATIC_K && vec) hipLaunchKernelGGL((k_ce_rate<CE_STATIC_K, true>), grid, block, 0, s, a);
    else if (k == CE_STATIC_K) hipLaunchKernelGGL((k_ce_rate<CE_STATIC_K, false>), grid, block, 0, s, a);
    else if (vec) hipLaunchKernelGGL((k_ce_rate<0, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_ce_rate<0, false>), grid, block, 0, s, a);
    LAUNCH_CHECK();
    plane_sum_finish_launch<CE_THREADS, 2>(s, n, g * chunks, a.slots, nats, totals);
    LAUNCH_CHECK();
    return 0;
}

LIC360_API int lic360_ce_rate_backward(void *stream, const float *logit, const float *label, const float *grad_nats, int n, int g, int h, int w,
                                       int k, float *d_logit) {
    ARG_CHECK(n >= 0 && g >= 0 && h >= 0 && w >= 0);
    ARG_CHECK(k >= 1 && k <= CE_MAX_K);
    if (n == 0 || g == 0 || h == 0 || w == 0) return 0;
    ARG_CHECK(logit && label && grad_nats && d_logit);
    int chunks;
    long groups;
    ARG_CHECK(!ce_rate_geometry(n, g, h, w, k, &chunks, &groups));
    const CeRateArgs a{logit, label, grad_nats, d_logit, {}, g, k, h * w, chunks};
    const bool vec = w % 2 == 0 && aligned8(logit) && aligned8(label) && aligned8(d_logit);
    const dim3 grid((unsigned)groups), block(CE_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (k == CE_STATIC_K && vec) hipLaunchKernelGGL((k_ce_rate_backward<CE_STATIC_K, true>), grid, block, 0, s, a);
    else if (k == CE_STATIC_K) hipLaunchKernelGGL((k_ce_rate_backward<CE_STATIC_K, false>), grid, block, 0, s, a);
    else if (vec) hipLaunchKernelGGL((k_ce_rate_backward<0, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_ce_rate_backward<0, false>), grid, block, 0, s, a);
    LAUNCH_CHECK();
    return 0;
}
