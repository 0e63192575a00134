// cconv_wgrad_kernels.hip -- weight gradient of the group-causal masked 5x5 convolution (DESIGN.md "Native backward of the group-causal
// convolution"; contract in include/lic360_hip_grad.h):
//     gw[oc, ic, th, tw] = sum_{n, y, x} gy[n, oc, y, x] * x[n, ic, y + th - 2, x + tw - 2]       at kept taps, +0.0 elsewhere.
// A GEMM per tap with M = output channels, N = input channels, K = the n * h * w positions, on v_mfma_f32_16x16x4_f32:
//   * a PAIR is (row block rb, column block cb): 16 consecutive output channels by 16 consecutive input channels, whatever groups they fall
//     in; a block may straddle groups and may be partial (operands past nout / channel are zeros, their results are never stored).
//   * tap (th, tw) of a pair is LIVE when the rule keeps at least one of its 256 weights: th + tw <= d, d = (last oc of the block) / cout -
//     (first ic of the block) / cin + 4 (- 1 for constrain 5).  A live (pair, tap) is a TILE; dead taps are not computed, pairs without a
//     live tap are not scheduled.
//   * k_cconv_wgrad_plan (one workgroup): the pair table {live mask, first tile} and the live pairs ordered by tap count, heavy first.
//   * k_cconv_wgrad: one wave per (live pair, split).  The n * h image rows are cut into `nsplit` runs of `rps` rows (the last may be shorter).
//     Per row and per chunk of CW_KW = 32 positions the wave stages gy [16][32] and x [16][5 rows][36 columns] (2-cell halo, zero outside the
//     map, zero past the end of the row; only the rows th <= d of a pair of reach d) in LDS, then runs 8 K steps of 4 positions: the A operand (gy) is shared by all taps of a step, the B
//     operand is the staged x tile read at the tap's shift, one 4-register accumulator per live tap (at most 25: 100 registers).  The
//     accumulators go to the split's slice of the scratch buffer as lane-major float4.
//   * k_cconv_wgrad_finish: one wave per (pair, tap) of the whole tensor adds the splits' fp32 partials in index order in double and rounds once,
//     writes kept elements and +0.0 everywhere else.  No atomics: the same bits on every call.  Short accumulator chains (a split is as few rows
//     as CW_MAX_SPLITS allows) and the double finish keep the result as close to the exact sum as a library convolution's.
// LDS pitches: 5 * CW_XP = 180 = 52 (mod 64) and CW_GP = 36 are 4 * odd, so the 16 channels x 4 positions of an operand read fall in 64
// different banks.  Offsets are 64-bit; the entry refuses sizes whose row, pair or workgroup counts leave int.
#include "common.h"
#include "../../include/lic360_hip_grad.h"

namespace {
constexpr int CW_THREADS = 64, CW_TILE = 16, CW_KW = 32, CW_HALO = 2, CW_KSZ = 5, CW_TAPS = CW_KSZ * CW_KSZ;
constexpr int CW_XP = CW_KW + 2 * CW_HALO, CW_XCH = CW_KSZ * CW_XP, CW_GP = 36;
constexpr int CW_SPLIT_ROWS = 1, CW_MAX_SPLITS = 32;
constexpr int CW_TILE_FLOATS = CW_TILE * CW_TILE;
constexpr long CW_MAX_PAIRS = 1L << 20;

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct CwGeom {
    int channel, nout, cin, cout, strict, nrb, ncb;
};

// d of pair (rb, cb): its live taps are th + tw <= d (none for d < 0), the most permissive rule among its 256 weights
__host__ __device__ inline int cw_reach(const CwGeom &g, int rb, int cb) {
    const int oc_hi = rb * CW_TILE + CW_TILE - 1 < g.nout ? rb * CW_TILE + CW_TILE - 1 : g.nout - 1;
    const int d = oc_hi / g.cout - (cb * CW_TILE) / g.cin + CW_KSZ - 1 - g.strict;
    return d < 2 * (CW_KSZ - 1) ? d : 2 * (CW_KSZ - 1);
}

// the live taps of pair (rb, cb), bit th * 5 + tw
__host__ __device__ inline unsigned cw_live_mask(const CwGeom &g, int rb, int cb) {
    const int d = cw_reach(g, rb, cb);
    unsigned m = 0;
    for (int th = 0; th < CW_KSZ; ++th)
        for (int tw = 0; tw < CW_KSZ; ++tw)
            if (th + tw <= d) m |= 1u << (th * CW_KSZ + tw);
    return m;
}

__host__ __device__ inline int cw_count(unsigned m) {
    int c = 0;
    for (int t = 0; t < CW_TAPS; ++t) c += (m >> t) & 1;
    return c;
}

struct CwArgs {
    const float *x, *gy;
    float *partial;                                     // [nsplit][ntiles][64 lanes][4]
    float *gw;
    const int2 *ptab;                                   // per pair: {live mask, first tile}
    const int *order;                                   // live pairs, heavy first
    CwGeom g;
    int n, h, w, nsplit, rps, ntiles;
};

__global__ __launch_bounds__(CW_THREADS) void k_cconv_wgrad_plan(const CwGeom g, int2 *ptab, int *order) {
    __shared__ int cnt[CW_TAPS + 1];
    const int npairs = g.nrb * g.ncb;
    for (int p = threadIdx.x; p < npairs; p += CW_THREADS) ptab[p] = make_int2((int)cw_live_mask(g, p / g.ncb, p % g.ncb), 0);
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int c = 0; c <= CW_TAPS; ++c) cnt[c] = 0;
    for (int p = 0; p < npairs; ++p) cnt[cw_count((unsigned)ptab[p].x)] += 1;
    int run = 0;
    for (int c = CW_TAPS; c >= 1; --c) {                // where the pairs of c live taps start in `order`
        const int t = cnt[c];
        cnt[c] = run;
        run += t;
    }
    int tiles = 0;
    for (int p = 0; p < npairs; ++p) {
        const int c = cw_count((unsigned)ptab[p].x);
        ptab[p].y = tiles;
        tiles += c;
        if (c) order[cnt[c]++] = p;
    }
}

// the work of one (live pair, split) for a pair whose live taps are th + tw <= D: straight-line code per K step, only the x rows th <= D are staged
template <int D>
__device__ __forceinline__ void cw_task(const CwArgs &a, float *xs, float *gs, int oc0, int ic0, int r0, int r1, f32x4 *dst) {
    constexpr int XROWS = D < CW_KSZ - 1 ? D + 1 : CW_KSZ;
    const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    const long HW = (long)a.h * a.w;
    f32x4 acc[CW_TAPS];
#pragma unroll
    for (int t = 0; t < CW_TAPS; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int r = r0; r < r1; ++r) {
        const int img = r / a.h, y = r - img * a.h;
        const float *ximg = a.x + (long)img * a.g.channel * HW;
        const float *gimg = a.gy + ((long)img * a.g.nout) * HW + (long)y * a.w;
        for (int x0 = 0; x0 < a.w; x0 += CW_KW) {
            __syncthreads();                                                    // the previous tiles have been read
            for (int e = lane; e < CW_TILE * XROWS * CW_XP; e += CW_THREADS) {
                const int j = e / (XROWS * CW_XP), rem = e - j * (XROWS * CW_XP), rr = rem / CW_XP, c = rem - rr * CW_XP;
                const int ic = ic0 + j, yy = y + rr - CW_HALO, xx = x0 + c - CW_HALO;
                float v = 0.f;
                if (ic < a.g.channel && yy >= 0 && yy < a.h && xx >= 0 && xx < a.w) v = ximg[(long)ic * HW + (long)yy * a.w + xx];
                xs[j * CW_XCH + rem] = v;
            }
            for (int e = lane; e < CW_TILE * CW_KW; e += CW_THREADS) {
                const int i = e / CW_KW, c = e - i * CW_KW;
                const int oc = oc0 + i, xx = x0 + c;
                float v = 0.f;
                if (oc < a.g.nout && xx < a.w) v = gimg[(long)oc * HW + xx];
                gs[i * CW_GP + c] = v;
            }
            __syncthreads();
            const int left = a.w - x0;
            const int steps = left >= CW_KW ? CW_KW / 4 : (left + 3) / 4;
            for (int ks = 0; ks < steps; ++ks) {
                const float av = gs[li * CW_GP + 4 * ks + lk];
                const float *xb = xs + li * CW_XCH + 4 * ks + lk;
#pragma unroll
                for (int t = 0; t < CW_TAPS; ++t) {
                    if (t / CW_KSZ + t % CW_KSZ <= D) {
                        const float bv = xb[(t / CW_KSZ) * CW_XP + (t % CW_KSZ)];
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
                    }
                }
            }
        }
    }
    int ord = 0;
#pragma unroll
    for (int t = 0; t < CW_TAPS; ++t) {
        if (t / CW_KSZ + t % CW_KSZ <= D) {
            dst[(long)ord * CW_THREADS] = acc[t];
            ++ord;
        }
    }
}

__global__ __launch_bounds__(CW_THREADS) void k_cconv_wgrad(const CwArgs a) {
    __shared__ float xs[CW_TILE * CW_XCH];
    __shared__ float gs[CW_TILE * CW_GP];
    const int k = blockIdx.x / a.nsplit, s = blockIdx.x - k * a.nsplit;
    const int pair = __builtin_amdgcn_readfirstlane(a.order[k]);
    const int first_tile = __builtin_amdgcn_readfirstlane(a.ptab[pair].y);
    const int rb = pair / a.g.ncb, cb = pair - rb * a.g.ncb;
    const int oc0 = rb * CW_TILE, ic0 = cb * CW_TILE;
    const int rows = a.n * a.h;
    const int r0 = s * a.rps, r1 = r0 + a.rps < rows ? r0 + a.rps : rows;
    f32x4 *dst = reinterpret_cast<f32x4 *>(a.partial) + ((long)s * a.ntiles + first_tile) * CW_THREADS + threadIdx.x;
    switch (cw_reach(a.g, rb, cb)) {                                            // scheduled pairs have d >= 0; d > 8 adds no tap
    case 0: cw_task<0>(a, xs, gs, oc0, ic0, r0, r1, dst); break;
    case 1: cw_task<1>(a, xs, gs, oc0, ic0, r0, r1, dst); break;
    case 2: cw_task<2>(a, xs, gs, oc0, ic0, r0, r1, dst); break;
    case 3: cw_task<3>(a, xs, gs, oc0, ic0, r0, r1, dst); break;
    case 4: cw_task<4>(a, xs, gs, oc0, ic0, r0, r1, dst); break;
    case 5: cw_task<5>(a, xs, gs, oc0, ic0, r0, r1, dst); break;
    case 6: cw_task<6>(a, xs, gs, oc0, ic0, r0, r1, dst); break;
    case 7: cw_task<7>(a, xs, gs, oc0, ic0, r0, r1, dst); break;
    default: cw_task<8>(a, xs, gs, oc0, ic0, r0, r1, dst); break;
    }
}

// one wave per (pair, tap) of the whole tensor: lane l holds rows 4 (l >> 4) .. + 3, column l & 15 of the tile, as the MFMA leaves them
__global__ __launch_bounds__(CW_THREADS) void k_cconv_wgrad_finish(const CwArgs a) {
    const int lane = threadIdx.x;
    const int pair = blockIdx.x / CW_TAPS, t = blockIdx.x - pair * CW_TAPS;
    const int2 pt = a.ptab[pair];
    const unsigned mask = (unsigned)__builtin_amdgcn_readfirstlane(pt.x);
    const int first_tile = __builtin_amdgcn_readfirstlane(pt.y);
    const int rb = pair / a.g.ncb, cb = pair - rb * a.g.ncb;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (mask & (1u << t)) {
        const int ord = __popc(mask & ((1u << t) - 1u));
        const f32x4 *src = reinterpret_cast<const f32x4 *>(a.partial) + ((long)first_tile + ord) * CW_THREADS + lane;
        for (int s = 0; s < a.nsplit; ++s) {                                    // index order, in double: one rounding at the end
            const f32x4 p = src[(long)s * a.ntiles * CW_THREADS];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] += (double)p[q];
        }
    }
    const int ic = cb * CW_TILE + (lane & 15);
    if (ic >= a.g.channel) return;
    const int th = t / CW_KSZ, tw = t - th * CW_KSZ;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int oc = rb * CW_TILE + 4 * (lane >> 4) + q;
        if (oc >= a.g.nout) continue;
        const bool keep = th + tw + ic / a.g.cin + a.g.strict <= oc / a.g.cout + CW_KSZ - 1;
        a.gw[((long)oc * a.g.channel + ic) * CW_TAPS + t] = keep ? (float)v[q] : 0.f;
    }
}

struct CwPlan {
    CwGeom g;
    int nsplit, rps, nlive, ntiles;
    long table_bytes, bytes;
};

long cw_align16(long v) { return (v + 15) / 16 * 16; }

// 0 with *pl filled; 1 when a product leaves the index types (rows of all images, pairs and workgroups are ints, element offsets longs).
// All sizes positive, channel and nout divisible by ngroup.
int cw_geometry(int n, int channel, int nout, int h, int w, int ngroup, int constrain, CwPlan *pl) {
    const long rows = (long)n * h, hw = (long)h * w;
    long e;
    if (rows > 0x7fffffffL - CW_MAX_SPLITS * CW_SPLIT_ROWS) return 1;
    if (__builtin_mul_overflow((long)n * channel, hw, &e) || e > (1L << 60)) return 1;
    if (__builtin_mul_overflow((long)n * nout, hw, &e) || e > (1L << 60)) return 1;
    CwGeom &g = pl->g;
    g.channel = channel, g.nout = nout, g.cin = channel / ngroup, g.cout = nout / ngroup, g.strict = constrain == 5 ? 1 : 0;
    g.nrb = (int)(((long)nout + CW_TILE - 1) / CW_TILE), g.ncb = (int)(((long)channel + CW_TILE - 1) / CW_TILE);
    const long npairs = (long)g.nrb * g.ncb;
    if (npairs > CW_MAX_PAIRS) return 1;
    long nlive = 0, ntiles = 0;
    for (int rb = 0; rb < g.nrb; ++rb)
        for (int cb = 0; cb < g.ncb; ++cb) {
            const int c = cw_count(cw_live_mask(g, rb, cb));
            nlive += c > 0;
            ntiles += c;
        }
    const long rps = std::max<long>(CW_SPLIT_ROWS, (rows + CW_MAX_SPLITS - 1) / CW_MAX_SPLITS);
    pl->rps = (int)rps, pl->nsplit = (int)((rows + rps - 1) / rps);
    pl->nlive = (int)nlive, pl->ntiles = (int)ntiles;
    if (nlive * pl->nsplit > 0x7fffffffL || npairs * CW_TAPS > 0x7fffffffL) return 1;
    pl->table_bytes = cw_align16(npairs * (long)(sizeof(int2) + sizeof(int)));
    // sized by a bound on nsplit that never shrinks when the rows grow (nsplit itself can: 128 rows are 32 runs of 4, 129 rows 26 runs of 5)
    const long bound = std::min<long>((rows + CW_SPLIT_ROWS - 1) / CW_SPLIT_ROWS, CW_MAX_SPLITS);
    pl->bytes = pl->table_bytes + bound * ntiles * CW_TILE_FLOATS * (long)sizeof(float);
    return 0;
}

bool cw_scalars_ok(int n, int channel, int nout, int h, int w, int ngroup, int ksz, int constrain) {
    return n >= 0 && channel >= 0 && nout >= 0 && h >= 0 && w >= 0 && ngroup >= 1 && ksz == CW_KSZ && (constrain == 5 || constrain == 6) &&
           channel % ngroup == 0 && nout % ngroup == 0;
}
}  // namespace

LIC360_API long lic360_cconv_wgrad_scratch_bytes(int n, int channel, int nout, int h, int w, int ngroup, int ksz, int constrain) {
    CwPlan pl;
    if (!cw_scalars_ok(n, channel, nout, h, w, ngroup, ksz, constrain) || n == 0 || channel == 0 || nout == 0 || h == 0 || w == 0) return 0;
    if (cw_geometry(n, channel, nout, h, w, ngroup, constrain, &pl)) return 0;
    return pl.bytes;
}

LIC360_API int lic360_cconv_wgrad(void *stream, const float *x, const float *gy, float *gw, void *scratch, int n, int channel, int nout, int h,
                                  int w, int ngroup, int ksz, int constrain) {
    ARG_CHECK(n >= 0 && channel >= 0 && nout >= 0 && h >= 0 && w >= 0 && ngroup >= 1);
    ARG_CHECK(ksz == CW_KSZ);
    ARG_CHECK(constrain == 5 || constrain == 6);
    ARG_CHECK(channel % ngroup == 0 && nout % ngroup == 0);
    if (n == 0 || channel == 0 || nout == 0) return 0;                       // no image, or an empty gw: nothing to write
    long gw_elems;
    ARG_CHECK(!__builtin_mul_overflow((long)nout * channel, (long)CW_TAPS, &gw_elems) && gw_elems <= (1L << 60));
    ARG_CHECK(gw);
    hipStream_t s = (hipStream_t)stream;
    if (h == 0 || w == 0) {                                                  // an empty sum
        HIP_TRY(hipMemsetAsync(gw, 0, (size_t)gw_elems * sizeof(float), s));
        return 0;
    }
    ARG_CHECK(x && gy && scratch);
    CwPlan pl;
    ARG_CHECK(!cw_geometry(n, channel, nout, h, w, ngroup, constrain, &pl));
    ARG_CHECK(((uintptr_t)scratch & 15) == 0);
    const long npairs = (long)pl.g.nrb * pl.g.ncb;
    int2 *ptab = (int2 *)scratch;
    int *order = (int *)(ptab + npairs);
    float *partial = (float *)((char *)scratch + pl.table_bytes);
    const CwArgs a{x, gy, partial, gw, ptab, order, pl.g, n, h, w, pl.nsplit, pl.rps, pl.ntiles};
    const dim3 block(CW_THREADS);
    hipLaunchKernelGGL(k_cconv_wgrad_plan, dim3(1), block, 0, s, pl.g, ptab, order);
    LAUNCH_CHECK();
    if (pl.nlive > 0) {
        hipLaunchKernelGGL(k_cconv_wgrad, dim3((unsigned)((long)pl.nlive * pl.nsplit)), block, 0, s, a);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_cconv_wgrad_finish, dim3((unsigned)(npairs * CW_TAPS)), block, 0, s, a);
    LAUNCH_CHECK();
    return 0;
}
