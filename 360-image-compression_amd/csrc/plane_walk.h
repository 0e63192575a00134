// plane_walk.h -- what the plane-wise training losses share (gmm_rate_kernels.hip, ce_rate_kernels.hip; DESIGN.md "Fused GMM rate loss"): a workgroup
// of THREADS threads owns THREADS * PER consecutive cells (y * W + x) of one (n, g) plane, PER cells per thread, and every image's loss is one
// deterministic double sum.  Each loss instantiates the pieces with its own constants and keeps its arithmetic, its Args struct and its kernels.
// The order of every addition is the contract (the same bits on every call, no atomics):
//   a thread adds its cells in index order (the loss's own loop); block_sum_to_slot adds the wave by a butterfly 32..1, then thread 0 the waves
//   in index order into the workgroup's slot; k_plane_sum_finish adds an image's slots in index order, in passes of THREADS slots.
// Beside the double, NC counters travel the same way: int inside a workgroup, long long in the slots and totals.
#pragma once
#include "common.h"

template <int PER> struct PlaneVec;
template <> struct PlaneVec<2> {
    typedef float2 type;
    static __device__ __forceinline__ void get(const float2 &q, float (&v)[2]) { v[0] = q.x; v[1] = q.y; }
    static __device__ __forceinline__ float2 make(const float (&v)[2]) { return make_float2(v[0], v[1]); }
};
template <> struct PlaneVec<4> {
    typedef float4 type;
    static __device__ __forceinline__ void get(const float4 &q, float (&v)[4]) { v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    static __device__ __forceinline__ float4 make(const float (&v)[4]) { return make_float4(v[0], v[1], v[2], v[3]); }
};

// this thread's PER cells of a plane: which they are, and moving them.  VEC: cells PER * t .. PER * t + PER - 1 of the chunk in one access of
// 4 * PER bytes (hw % PER == 0, so the PER cells are inside together); else cells t + k * THREADS with 4-byte accesses.  Cells past the plane's
// end load as 0 and are never stored.
template <int THREADS, int PER, bool VEC>
struct PlaneCells {
    typedef typename PlaneVec<PER>::type V;
    int first;                 // VEC: the first of PER consecutive cells; else the first of PER, THREADS apart
    int hw;
    __device__ __forceinline__ PlaneCells(int chunk, int tid, int hw_) : first(chunk * (THREADS * PER) + (VEC ? PER * tid : tid)), hw(hw_) {}
    __device__ __forceinline__ bool inside(int k) const { return VEC ? first < hw : first + k * THREADS < hw; }
    __device__ __forceinline__ void load(const float *plane, float (&v)[PER]) const {
        if (VEC) {
            V q = PlaneVec<PER>::make({});
            if (first < hw) q = *(const V *)(plane + first);
            PlaneVec<PER>::get(q, v);
        } else {
#pragma unroll
            for (int k = 0; k < PER; ++k) v[k] = inside(k) ? plane[first + k * THREADS] : 0.0f;
        }
    }
    __device__ __forceinline__ void store(float *plane, const float (&v)[PER]) const {
        if (VEC) {
            if (first < hw) *(V *)(plane + first) = PlaneVec<PER>::make(v);
        } else {
#pragma unroll
            for (int k = 0; k < PER; ++k)
                if (inside(k)) plane[first + k * THREADS] = v[k];
        }
    }
};

// what a workgroup is: (image, plane, chunk) of its index and the cells of this thread; a loss's Walk adds which of them count
template <int THREADS, int PER, bool VEC>
struct PlaneWalk {
    long plane;                // n * G + g
    int n;
    PlaneCells<THREADS, PER, VEC> cells;
    __device__ __forceinline__ PlaneWalk(int chunks, int G, int hw) : plane(blockIdx.x / chunks), n((int)(plane / G)), cells(blockIdx.x % chunks, threadIdx.x, hw) {}
};

// one slot per workgroup: the scratch buffer carved into an array of doubles, then NC arrays of long long (8-byte aligned base)
template <int NC>
struct PlaneSlots {
    double *nats;
    long long *cnt[NC];
};
template <int NC>
struct PlaneFinishArgs {
    PlaneSlots<NC> slots;
    double *nats;              // [images]
    long long *totals[NC];     // [images] each
    int per_image;             // slots per image
};

// the workgroup's sum of every thread's (acc, cnt) into its slot
template <int THREADS, int NC>
__device__ __forceinline__ void block_sum_to_slot(double acc, int (&cnt)[NC], const PlaneSlots<NC> &slots) {
    __shared__ double s_nats[THREADS / 64];
    __shared__ int s_cnt[NC][THREADS / 64];
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_xor(acc, off);
#pragma unroll
        for (int c = 0; c < NC; ++c) cnt[c] += __shfl_xor(cnt[c], off);
    }
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) {
        s_nats[tid >> 6] = acc;
#pragma unroll
        for (int c = 0; c < NC; ++c) s_cnt[c][tid >> 6] = cnt[c];
    }
    __syncthreads();
    if (tid == 0) {
        double tot = s_nats[0];
        int tc[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) tc[c] = s_cnt[c][0];
        for (int wv = 1; wv < THREADS / 64; ++wv) {
            tot += s_nats[wv];
#pragma unroll
            for (int c = 0; c < NC; ++c) tc[c] += s_cnt[c][wv];
        }
        slots.nats[blockIdx.x] = tot;
#pragma unroll
        for (int c = 0; c < NC; ++c) slots.cnt[c][blockIdx.x] = tc[c];
    }
}

// one workgroup per image: its slots added in index order by thread 0, staged through LDS THREADS at a time
template <int THREADS, int NC>
__global__ __launch_bounds__(THREADS) void k_plane_sum_finish(const PlaneFinishArgs<NC> a) {
    __shared__ double s_nats[THREADS];
    __shared__ long long s_cnt[NC][THREADS];
    const int tid = threadIdx.x;
    const long first = (long)blockIdx.x * a.per_image;
    double tot = 0.0;
    long long sum[NC] = {};
    for (int lo = 0; lo < a.per_image; lo += THREADS) {
        const int j = lo + tid;
        s_nats[tid] = j < a.per_image ? a.slots.nats[first + j] : 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) s_cnt[c][tid] = j < a.per_image ? a.slots.cnt[c][first + j] : 0;
        __syncthreads();
        if (tid == 0) {
            const int cnt = a.per_image - lo < THREADS ? a.per_image - lo : THREADS;
#pragma unroll 8
            for (int q = 0; q < cnt; ++q) {                                  // index order; the unrolled reads overlap
                tot += s_nats[q];
#pragma unroll
                for (int c = 0; c < NC; ++c) sum[c] += s_cnt[c][q];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.nats[blockIdx.x] = tot;
#pragma unroll
        for (int c = 0; c < NC; ++c) a.totals[c][blockIdx.x] = sum[c];
    }
}

// geometry shared by a loss's entry points: 0 on success with *chunks / *groups filled, 1 when a product leaves the index types (cells of a
// plane, workgroups and an image's slots are ints, element offsets are longs).  per_symbol: floats per symbol of the widest operand; chunk:
// THREADS * PER.  An image's slots, g * chunks, need no check of their own: n >= 1 here, so they are at most planes * chunks <= INT_MAX.
inline int plane_walk_geometry(int n, int g, int h, int w, int per_symbol, int chunk, int *chunks, long *groups) {
    long hw, planes, elems, wg;
    if (__builtin_mul_overflow((long)h, (long)w, &hw) || hw > 0x7fffffffL - chunk) return 1;
    if (__builtin_mul_overflow((long)n, (long)g, &planes)) return 1;
    if (__builtin_mul_overflow(planes, hw, &elems) || __builtin_mul_overflow(elems, (long)per_symbol, &elems) || elems > (1L << 60)) return 1;
    const long per_plane = (hw + chunk - 1) / chunk;
    if (__builtin_mul_overflow(planes, per_plane, &wg) || wg > 0x7fffffffL) return 1;
    *chunks = (int)per_plane;
    *groups = wg;
    return 0;
}
// p is null or a multiple of `bytes` (a power of two): the vector form's condition on every base
inline bool plane_walk_aligned(const void *p, unsigned bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

template <int NC>
inline long plane_slots_bytes(long groups) { return groups * (long)(sizeof(double) + NC * sizeof(long long)); }
template <int NC>
inline PlaneSlots<NC> plane_slots_carve(void *scratch, long groups) {
    PlaneSlots<NC> s;
    s.nats = (double *)scratch;
    for (int c = 0; c < NC; ++c) s.cnt[c] = (long long *)(s.nats + groups) + c * groups;
    return s;
}

// a call without a symbol (n, g, h or w is 0) launches nothing; an image's totals are still written
template <int NC>
inline int plane_walk_no_symbol(hipStream_t s, int n, double *nats, long long *const (&totals)[NC]) {
    if (n <= 0) return 0;
    ARG_CHECK(nats);
    for (int c = 0; c < NC; ++c) ARG_CHECK(totals[c]);
    HIP_TRY(hipMemsetAsync(nats, 0, (size_t)n * sizeof(double), s));
    for (int c = 0; c < NC; ++c) HIP_TRY(hipMemsetAsync(totals[c], 0, (size_t)n * sizeof(long long), s));
    return 0;
}

// the finish launch of a loss: one workgroup per image over its g * chunks slots
template <int THREADS, int NC>
inline void plane_sum_finish_launch(hipStream_t s, int n, int per_image, const PlaneSlots<NC> &slots, double *nats, long long *const (&totals)[NC]) {
    PlaneFinishArgs<NC> f;
    f.slots = slots;
    f.nats = nats;
    for (int c = 0; c < NC; ++c) f.totals[c] = totals[c];
    f.per_image = per_image;
    hipLaunchKernelGGL((k_plane_sum_finish<THREADS, NC>), dim3((unsigned)n), dim3(THREADS), 0, s, f);
}
