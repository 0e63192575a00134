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
//     to scratch memory.  Each coded symbol's fp32 loss is added in double: a thread's cells in index order, the wave by a butterfly, the four waves in
//     index order; total and count go to the workgroup's scratch slot.  k_gmm_rate_finish adds an image's slots in index order.  No atomics: the same
//     bits on every call.
//   * k_gmm_rate_backward<NG, VEC, LABEL>: the same walk; recomputes the symbol from the inputs and writes d_logit, d_sigma, d_mean (and d_label)
//     in place of the reads, exact zeros for uncoded cells.
// Arithmetic (the contract of DESIGN.md, restated in tests/gmm_rate_cases.py): lic360_softmax_inplace's order, the sigma floor, then k_entropy_gmm's
// per-component body (csrc/tile_table_kernels.hip) stated a second time in gmm_component below -- that kernel is untouched.
#include "common.h"
#include "lic360_exact_math.h"

namespace {
constexpr int GR_THREADS = 256, GR_PER_THREAD = 4, GR_CHUNK = GR_THREADS * GR_PER_THREAD, GR_MAX_NG = 16;
constexpr float GR_SIGMA_FLOOR = 0.00001f;

// one struct by value: the number of arguments of a launch costs like their bytes do (DESIGN.md 4.1 b'')
struct GmmRateArgs {
    const float *logit, *sigma, *mean, *label, *mask;   // mask: null = every symbol coded
    const float *grad;                                  // backward: grad_nats [N]
    float *o_logit, *o_sigma, *o_mean, *o_label;        // backward: the gradients; forward: o_label is the map (or null)
    double *slot_nats;                                  // forward: one slot per workgroup
    long long *slot_sym;
    int G, ng, HW, chunks;                              // chunks: workgroups per plane
};
struct GmmFinishArgs {
    const double *slot_nats;
    const long long *slot_sym;
    double *nats;
    long long *symbols;
    int per_image;
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

// this thread's four cells of a plane: which they are, and moving them
template <bool VEC>
struct Cells {
    int first;                 // VEC: the first of four consecutive cells; else the first of four GR_THREADS apart
    int hw;
    __device__ __forceinline__ Cells(int chunk, int tid, int hw_) : first(chunk * GR_CHUNK + (VEC ? GR_PER_THREAD * tid : tid)), hw(hw_) {}
    __device__ __forceinline__ bool inside(int k) const { return VEC ? first < hw : first + k * GR_THREADS < hw; }     // (VEC: hw % 4 == 0)
    __device__ __forceinline__ void load(const float *plane, float (&v)[GR_PER_THREAD]) const {
        if (VEC) {
            float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (first < hw) q = *(const float4 *)(plane + first);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < GR_PER_THREAD; ++k) v[k] = inside(k) ? plane[first + k * GR_THREADS] : 0.0f;
        }
    }
    __device__ __forceinline__ void store(float *plane, const float (&v)[GR_PER_THREAD]) const {
        if (VEC) {
            if (first < hw) *(float4 *)(plane + first) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int k = 0; k < GR_PER_THREAD; ++k)
                if (inside(k)) plane[first + k * GR_THREADS] = v[k];
        }
    }
};

// what a workgroup is: (image, plane, chunk) of its index, the cells of this thread and which of them are coded
template <bool VEC>
struct Walk {
    long plane;                // n * G + g
    int n;
    Cells<VEC> cells;
    bool coded[GR_PER_THREAD];
    bool any;                  // a cell of this WAVE is coded
    __device__ __forceinline__ Walk(const GmmRateArgs &a) : plane(blockIdx.x / a.chunks), n((int)(plane / a.G)), cells(blockIdx.x % a.chunks, threadIdx.x, a.HW) {
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
    __shared__ double s_nats[GR_THREADS / 64];
    __shared__ int s_sym[GR_THREADS / 64];
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
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < GR_PER_THREAD; ++k)
        if (wk.coded[k]) { acc += (double)loss[k]; ++cnt; }
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_xor(acc, off);
        cnt += __shfl_xor(cnt, off);
    }
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) { s_nats[tid >> 6] = acc; s_sym[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        double tot = s_nats[0];
        int c = s_sym[0];
        for (int wv = 1; wv < GR_THREADS / 64; ++wv) { tot += s_nats[wv]; c += s_sym[wv]; }
        a.slot_nats[blockIdx.x] = tot;
        a.slot_sym[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(GR_THREADS) void k_gmm_rate_finish(const GmmFinishArgs a) {
    __shared__ double s_nats[GR_THREADS];
    __shared__ long long s_sym[GR_THREADS];
    const int tid = threadIdx.x;
    const long first = (long)blockIdx.x * a.per_image;
    double tot = 0.0;
    long long sym = 0;
    for (int lo = 0; lo < a.per_image; lo += GR_THREADS) {
        const int j = lo + tid;
        s_nats[tid] = j < a.per_image ? a.slot_nats[first + j] : 0.0;
        s_sym[tid] = j < a.per_image ? a.slot_sym[first + j] : 0;
        __syncthreads();
        if (tid == 0) {
            const int cnt = a.per_image - lo < GR_THREADS ? a.per_image - lo : GR_THREADS;
#pragma unroll 8
            for (int q = 0; q < cnt; ++q) { tot += s_nats[q]; sym += s_sym[q]; }               // index order; the unrolled reads overlap
        }
        __syncthreads();
    }
    if (tid == 0) { a.nats[blockIdx.x] = tot; a.symbols[blockIdx.x] = sym; }
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

// geometry shared by the three entry points: 0 on success with *chunks / *groups filled, 1 when a product leaves the index types
// (cells of a plane and workgroups are ints, element offsets are longs)
int gmm_rate_geometry(int n, int g, int h, int w, int ng, int *chunks, long *groups) {
    long hw, planes, elems, wg;
    if (__builtin_mul_overflow((long)h, (long)w, &hw) || hw > 0x7fffffffL - GR_CHUNK) return 1;
    if (__builtin_mul_overflow((long)n, (long)g, &planes)) return 1;
    if (__builtin_mul_overflow(planes, hw, &elems) || __builtin_mul_overflow(elems, (long)ng, &elems) || elems > (1L << 60)) return 1;
    const long per_plane = (hw + GR_CHUNK - 1) / GR_CHUNK;
    if (__builtin_mul_overflow(planes, per_plane, &wg) || wg > 0x7fffffffL) return 1;
    *chunks = (int)per_plane;
    *groups = wg;
    return 0;
}
bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
}  // namespace

LIC360_API long lic360_gmm_rate_scratch_bytes(int n, int g, int h, int w) {
    int chunks;
    long groups;
    if (n <= 0 || g <= 0 || h <= 0 || w <= 0 || gmm_rate_geometry(n, g, h, w, GR_MAX_NG, &chunks, &groups)) return 0;
    return groups * (long)(sizeof(double) + sizeof(long long));
}

LIC360_API int lic360_gmm_rate(void *stream, const float *logit, const float *sigma, const float *mean, const float *label, const float *mask,
                               int n, int g, int h, int w, int ng, double *nats, long long *symbols, float *map, void *scratch) {
    ARG_CHECK(n >= 0 && g >= 0 && h >= 0 && w >= 0);
    ARG_CHECK(ng >= 1 && ng <= GR_MAX_NG);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0 || g == 0 || h == 0 || w == 0) {                              // no symbol: nothing is launched; an image's totals are still written
        if (n > 0) {
            ARG_CHECK(nats && symbols);
            HIP_TRY(hipMemsetAsync(nats, 0, (size_t)n * sizeof(double), s));
            HIP_TRY(hipMemsetAsync(symbols, 0, (size_t)n * sizeof(long long), s));
        }
        return 0;
    }
    ARG_CHECK(logit && sigma && mean && label && nats && symbols && scratch);
    int chunks;
    long groups;
    ARG_CHECK(!gmm_rate_geometry(n, g, h, w, ng, &chunks, &groups));
    ARG_CHECK(((uintptr_t)scratch & 7) == 0);
    double *slot_nats = (double *)scratch;
    long long *slot_sym = (long long *)(slot_nats + groups);
    const GmmRateArgs a{logit, sigma, mean, label, mask, nullptr, nullptr, nullptr, nullptr, map, slot_nats, slot_sym, g, ng, h * w, chunks};
    const bool vec = w % 4 == 0 && aligned16(logit) && aligned16(sigma) && aligned16(mean) && aligned16(label) && aligned16(mask) && aligned16(map);
    const dim3 grid((unsigned)groups), block(GR_THREADS);
    if (ng == 3 && vec) hipLaunchKernelGGL((k_gmm_rate<3, true>), grid, block, 0, s, a);
    else if (ng == 3) hipLaunchKernelGGL((k_gmm_rate<3, false>), grid, block, 0, s, a);
    else if (vec) hipLaunchKernelGGL((k_gmm_rate<0, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_gmm_rate<0, false>), grid, block, 0, s, a);
    LAUNCH_CHECK();
    const GmmFinishArgs f{slot_nats, slot_sym, nats, symbols, g * chunks};
    hipLaunchKernelGGL(k_gmm_rate_finish, dim3((unsigned)n), block, 0, s, f);
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
    const GmmRateArgs a{logit, sigma, mean, label, mask, grad_nats, d_logit, d_sigma, d_mean, d_label, nullptr, nullptr, g, ng, h * w, chunks};
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
