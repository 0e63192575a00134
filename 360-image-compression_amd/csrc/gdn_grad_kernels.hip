// gdn_grad_kernels.hip -- backward of the one-pass GDN of gdn_kernels.hip (DESIGN.md "Native backward of the one-pass GDN"; contract in
// include/lic360_hip_gdn_grad.h).  With s_i = beta_i + sum_j gamma_ij x_j^2, n_i = sqrt(s_i) and the upstream gradient g:
//                GDN (y = x / n)                    inverse (y = x * n)
//     r_i        g_i / n_i                          g_i * n_i
//     t_i        (g_i * (x_i / n_i)) / s_i          (g_i * x_i) / n_i
//     u_k        sum_i gamma_ik t_i                 same
//     dx_k       r_k - x_k * u_k                    r_k + x_k * u_k
//     dgamma_ij  -1/2 sum_{n,p} t_i x_j^2           +1/2 sum_{n,p} t_i x_j^2
//     dbeta_i    -1/2 sum_{n,p} t_i                 +1/2 sum_{n,p} t_i
// every operation one fp32 rounding in the order written (-ffp-contract=off), every contraction on v_mfma_f32_16x16x4_f32.
//   * k_gdn_backward_dx: a workgroup owns GB_PT = 32 positions of one image and all C channels.  x and g go to LDS as [half][C][16] (half = which 16
//     positions; the B-operand read of 4 channels x 16 positions then covers 64 consecutive floats); wave w owns positions 16 (w & 1) .. + 15 and the
//     channel tiles a = (w >> 1), (w >> 1) + 2, ...  The first contraction is the forward's: the same gamma slabs of 16 input channels at pitch 17, the
//     same MFMA chain in ascending j, then acc + beta -- s is the forward's bits.  n, r and t are formed by the lane that owns the cell (the D layout gives a
//     lane the same cells in both contractions), r stays in registers, t overwrites g in LDS and goes to the scratch t-map [n][c][p] row-wise.  The second
//     contraction reads gamma transposed -- slabs of 16 ROWS of gamma, the A operand walks a row -- and sums over i in ascending order; dx overwrites the x
//     tile and leaves row-wise.  Without gx the second contraction and the store are skipped, without a t-map its store.
//   * k_gdn_backward_param: dgamma = T X2^T, a [C x K] [K x C] GEMM over the K = n * P positions.  A TILE is GP_KT = 32 positions of one image (the last
//     tile of an image may be short: positions past P contribute zeros and are never read); the n * ceil(P / 32) tiles are cut into at most
//     GP_MAX_SPLITS contiguous splits of `tps` tiles (the last may be shorter).  One workgroup per split holds the whole C x C partial in accumulators:
//     wave (wr, wc) owns the row tiles of parity wr and the column tiles of parity wc, 36 tiles = 144 registers per lane at C = 192, plus, for wc = 0, the row
//     sums of t as one more column whose B operand is 1.0.  t and x^2 (squared on the way in) are staged at pitch 34: 16 channels x 2 positions of an operand
//     read fall in 32 different banks.  The partial and the row sums go to the split's slice of the scratch.
//   * k_gdn_backward_finish: adds the splits' fp32 partials in index order in double, applies -+1/2, rounds once, writes dgamma [c][c] and dbeta [c].
// No atomics anywhere: the same bits on every call.  Offsets are 64-bit; the entry refuses sizes whose tile counts leave int or whose element counts leave long.
#include "common.h"
#include "../../include/lic360_hip_gdn_grad.h"

namespace {
constexpr int GB_THREADS = 256;
constexpr int GB_PT = 32;                           // positions per workgroup of the dx kernel: 16 per wave pair
constexpr int GB_JS = 16;                           // channels per gamma slab
constexpr int GB_GP = 17;                           // pitch of a slab row in the first contraction (the forward's)
constexpr int GP_KT = 32;                           // positions per tile of the param kernel
constexpr int GP_PITCH = 34;                        // pitch of its staged rows: 2 (mod 32)
constexpr int GP_MAX_SPLITS = 256;                  // workgroups of the param kernel, and slices of its scratch, at most
typedef float gb_f4 __attribute__((ext_vector_type(4)));

// pitch of a slab of 16 gamma ROWS in the second contraction: 16 (mod 32), so that the two k rows a 32-lane half reads fall in different banks
template <int C> struct GbPitch2 { static constexpr int value = C % 32 == 0 ? C + 16 : C; };

// where quad q (4 positions) of channel j of a [half][C][16] tile starts
template <int C> __device__ __forceinline__ int gb_quad_at(int j, int q) { return ((q >> 2) * C + j) * 16 + 4 * (q & 3); }

template <bool VEC> __device__ __forceinline__ gb_f4 gb_load_quad(const float *row, long p, long P) {
    gb_f4 r;
    if (VEC && p + 3 < P) r = *(const gb_f4 *)(row + p);
    else {
#pragma unroll
        for (int t = 0; t < 4; ++t) r[t] = p + t < P ? row[p + t] : 0.0f;
    }
    return r;
}

template <bool VEC> __device__ __forceinline__ void gb_store_quad(float *row, long p, long P, gb_f4 r) {
    if (VEC && p + 3 < P) *(gb_f4 *)(row + p) = r;
    else {
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (p + t < P) row[p + t] = r[t];
    }
}

// v_mfma_f32_16x16x4_f32: lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15], D rows 4 (l >> 4) + v, column l & 15.  Rows = channels, columns = positions.
template <int CT, bool VEC>                         // CT = C / 16; VEC: 16-byte global accesses (P % 4 == 0, every tensor on a 16-byte boundary)
__global__ __launch_bounds__(GB_THREADS) void k_gdn_backward_dx(const float *__restrict__ x, const float *__restrict__ gy, const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, float *__restrict__ gx, float *__restrict__ tmap, long P,
                                                                int tpi, int inverse) {
    constexpr int C = CT * 16, NA = (CT + 1) / 2, G2P = GbPitch2<C>::value;
    constexpr int QUADS = C * (GB_PT / 4), NQ = (QUADS + GB_THREADS - 1) / GB_THREADS;     // quads of a tile, and per thread (the last round may be partial)
    constexpr int GQ = CT;                                                                  // slab elements per thread (C * 16 / 256)
    extern __shared__ float lds[];
    float *xs = lds, *ts = lds + C * GB_PT, *gs = lds + 2 * C * GB_PT;                      // x (later dx) | g (later t) | gamma slab
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4, pw = wave & 1, ah = wave >> 1;
    const long img = blockIdx.x / tpi, p0 = (long)(blockIdx.x - img * tpi) * GB_PT;
    const float *xn = x + img * C * P, *gn = gy + img * C * P;
    // ---- x and g tiles: every load is issued before the first LDS write; past the end: zeros
    gb_f4 xr[NQ], gr4[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const int e = tid + GB_THREADS * k;
        if (e < QUADS) {
            const int j = e / (GB_PT / 4), q = e - j * (GB_PT / 4);
            xr[k] = gb_load_quad<VEC>(xn + (long)j * P, p0 + 4 * q, P);
            gr4[k] = gb_load_quad<VEC>(gn + (long)j * P, p0 + 4 * q, P);
        }
    }
    float gr[GQ];
#pragma unroll
    for (int k = 0; k < GQ; ++k) { const int e = tid + GB_THREADS * k; gr[k] = gamma[(long)(e / GB_JS) * C + (e % GB_JS)]; }
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const int e = tid + GB_THREADS * k;
        if (e < QUADS) {
            const int j = e / (GB_PT / 4), q = e - j * (GB_PT / 4);
            *(gb_f4 *)(xs + gb_quad_at<C>(j, q)) = xr[k];
            *(gb_f4 *)(ts + gb_quad_at<C>(j, q)) = gr4[k];
        }
    }
    // ---- s: the forward's contraction, gamma slabs of 16 input channels, ascending j
    gb_f4 acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = (gb_f4){0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < C; j0 += GB_JS) {
        __syncthreads();                                                     // the previous slab is consumed (first pass: the tiles are written)
#pragma unroll
        for (int k = 0; k < GQ; ++k) { const int e = tid + GB_THREADS * k; gs[(e / GB_JS) * GB_GP + (e % GB_JS)] = gr[k]; }
        if (j0 + GB_JS < C) {
#pragma unroll
            for (int k = 0; k < GQ; ++k) { const int e = tid + GB_THREADS * k; gr[k] = gamma[(long)(e / GB_JS) * C + j0 + GB_JS + (e % GB_JS)]; }
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < GB_JS / 4; ++ks) {
            const float v = xs[(pw * C + j0 + 4 * ks + kq) * 16 + col], b = v * v;
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                const int a = ah + 2 * k;
                if (a < CT) acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(gs[(16 * a + col) * GB_GP + 4 * ks + kq], b, acc[k], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                                         // every wave is done with the x^2 operands and the last slab
    if (gx) {                                                                // rows 0 .. 15 of gamma for the second contraction, in flight over the cell pass
#pragma unroll
        for (int k = 0; k < GQ; ++k) gr[k] = gamma[tid + GB_THREADS * k];
    }
    // ---- n, r, t: each cell by the lane that owns it; t over g
    gb_f4 rr[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const int a = ah + 2 * k;
        if (a < CT) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = 16 * a + 4 * kq + v, at = (pw * C + i) * 16 + col;
                const float s = acc[k][v] + beta[i], nrm = sqrtf(s), xv = xs[at], gv = ts[at];
                float r, t;
                if (inverse) {
                    r = gv * nrm;
                    t = (gv * xv) / nrm;
                } else {
                    r = gv / nrm;
                    t = (gv * (xv / nrm)) / s;
                }
                rr[k][v] = r;
                ts[at] = t;
            }
        }
    }
    __syncthreads();
    if (tmap) {
        float *tn = tmap + img * C * P;
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const int e = tid + GB_THREADS * k;
            if (e < QUADS) {
                const int j = e / (GB_PT / 4), q = e - j * (GB_PT / 4);
                gb_store_quad<VEC>(tn + (long)j * P, p0 + 4 * q, P, *(const gb_f4 *)(ts + gb_quad_at<C>(j, q)));
            }
        }
    }
    if (!gx) return;
    // ---- u_k = sum_i gamma[i][k] t_i: slabs of 16 rows of gamma, the A operand read along a row; ascending i
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = (gb_f4){0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < C; i0 += GB_JS) {
        __syncthreads();                                                     // the previous slab is consumed
#pragma unroll
        for (int k = 0; k < GQ; ++k) { const int e = tid + GB_THREADS * k; gs[(e / C) * G2P + (e % C)] = gr[k]; }
        if (i0 + GB_JS < C) {
#pragma unroll
            for (int k = 0; k < GQ; ++k) gr[k] = gamma[(long)(i0 + GB_JS) * C + tid + GB_THREADS * k];
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < GB_JS / 4; ++ks) {
            const float b = ts[(pw * C + i0 + 4 * ks + kq) * 16 + col];
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                const int a = ah + 2 * k;
                if (a < CT) acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(gs[(4 * ks + kq) * G2P + 16 * a + col], b, acc[k], 0, 0, 0);
            }
        }
    }
    // ---- dx over the x tile (a cell of it is read by its owner alone since the first contraction ended), then stored row-wise
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const int a = ah + 2 * k;
        if (a < CT) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int at = (pw * C + 16 * a + 4 * kq + v) * 16 + col;
                const float xu = xs[at] * acc[k][v];
                xs[at] = inverse ? rr[k][v] + xu : rr[k][v] - xu;
            }
        }
    }
    __syncthreads();
    float *on = gx + img * C * P;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const int e = tid + GB_THREADS * k;
        if (e < QUADS) {
            const int j = e / (GB_PT / 4), q = e - j * (GB_PT / 4);
            gb_store_quad<VEC>(on + (long)j * P, p0 + 4 * q, P, *(const gb_f4 *)(xs + gb_quad_at<C>(j, q)));
        }
    }
}

// one workgroup per split: partial[split] = { sum over the split's positions of t_i x_j^2  [C][C],  of t_i  [C] }
template <int CT, bool VEC>
__global__ __launch_bounds__(GB_THREADS) void k_gdn_backward_param(const float *__restrict__ x, const float *__restrict__ tmap, float *__restrict__ partial,
                                                                   long P, int tpi, long ntiles, long tps) {
    constexpr int C = CT * 16, NR = (CT + 1) / 2;
    constexpr int QUADS = C * (GP_KT / 4), NQ = (QUADS + GB_THREADS - 1) / GB_THREADS;
    extern __shared__ float lds[];
    float *ts = lds, *qs = lds + C * GP_PITCH;                                              // t [C][34] | x^2 [C][34]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kq = lane >> 4, wr = wave & 1, wc = wave >> 1;
    const long t0 = (long)blockIdx.x * tps, t1 = t0 + tps < ntiles ? t0 + tps : ntiles;
    gb_f4 acc[NR][NR], accb[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        accb[r] = (gb_f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NR; ++c) acc[r][c] = (gb_f4){0.f, 0.f, 0.f, 0.f};
    }
    gb_f4 tr[NQ], xr[NQ];
    auto load = [&](long tile) {                                            // positions past P: zeros, nothing read
        const long img = tile / tpi, p0 = (tile - img * tpi) * GP_KT;
        const float *tn = tmap + img * C * P, *xn = x + img * C * P;
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const int e = tid + GB_THREADS * k;
            if (e < QUADS) {
                const int j = e / (GP_KT / 4), q = e - j * (GP_KT / 4);
                tr[k] = gb_load_quad<VEC>(tn + (long)j * P, p0 + 4 * q, P);
                xr[k] = gb_load_quad<VEC>(xn + (long)j * P, p0 + 4 * q, P);
            }
        }
    };
    if (t0 < t1) load(t0);
    for (long tile = t0; tile < t1; ++tile) {
        __syncthreads();                                                     // the previous tile is consumed
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const int e = tid + GB_THREADS * k;
            if (e < QUADS) {
                const int j = e / (GP_KT / 4), q = e - j * (GP_KT / 4);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    ts[j * GP_PITCH + 4 * q + t] = tr[k][t];
                    qs[j * GP_PITCH + 4 * q + t] = xr[k][t] * xr[k][t];
                }
            }
        }
        __syncthreads();
        if (tile + 1 < t1) load(tile + 1);                                   // in flight during this tile's MFMAs
#pragma unroll
        for (int ks = 0; ks < GP_KT / 4; ++ks) {
            float av[NR], bv[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                av[r] = wr + 2 * r < CT ? ts[(16 * (wr + 2 * r) + col) * GP_PITCH + 4 * ks + kq] : 0.f;
                bv[r] = wc + 2 * r < CT ? qs[(16 * (wc + 2 * r) + col) * GP_PITCH + 4 * ks + kq] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                if (wr + 2 * r < CT) {
#pragma unroll
                    for (int c = 0; c < NR; ++c)
                        if (wc + 2 * c < CT) acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], bv[c], acc[r][c], 0, 0, 0);
                    if (wc == 0) accb[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], 1.0f, accb[r], 0, 0, 0);
                }
            }
        }
    }
    float *out = partial + (long)blockIdx.x * (C * C + C);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        if (wr + 2 * r < CT) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int i = 16 * (wr + 2 * r) + 4 * kq + v;
#pragma unroll
                for (int c = 0; c < NR; ++c)
                    if (wc + 2 * c < CT) out[i * C + 16 * (wc + 2 * c) + col] = acc[r][c][v];
                if (wc == 0 && col == 0) out[C * C + i] = accb[r][v];
            }
        }
    }
}

// element e of [C * C + C]: the splits' partials added in index order in double, times -+1/2 (exact), rounded once
__global__ __launch_bounds__(GB_THREADS) void k_gdn_backward_finish(const float *__restrict__ partial, float *__restrict__ ggamma, float *__restrict__ gbeta,
                                                                    int C, int nsplit, int inverse) {
    const int total = C * C + C, e = blockIdx.x * GB_THREADS + threadIdx.x;
    if (e >= total) return;
    double v = 0.0;
    for (int s = 0; s < nsplit; ++s) v += (double)partial[(long)s * total + e];
    const float r = (float)((inverse ? 0.5 : -0.5) * v);
    if (e < C * C) ggamma[e] = r;
    else gbeta[e - C * C] = r;
}

struct GbPlan {
    int tpi;                                            // tiles (of 32 positions, both kernels) per image
    long ntiles, tps;                                   // tiles of all images; tiles per split
    int nsplit;
    long tmap_bytes, bytes;
};

bool gb_channels_ok(int c) { return c == 16 || c == 32 || c == 48 || c == 64 || c == 96 || c == 128 || c == 192; }

long gb_align16(long v) { return (v + 15) / 16 * 16; }

// 0 with *pl filled; 1 when a count leaves its type (tiles of all images are an int, element and byte counts longs).  n, p > 0, c supported.
int gb_geometry(int n, int c, long p, GbPlan *pl) {
    static_assert(GB_PT == GP_KT, "one tile count serves both kernels");
    long elems;
    if (__builtin_mul_overflow((long)n * c, p, &elems) || elems > (1L << 58)) return 1;
    const long tpi = (p + GP_KT - 1) / GP_KT, ntiles = tpi * n;
    if (ntiles > 0x7fffffffL) return 1;
    pl->tpi = (int)tpi, pl->ntiles = ntiles;
    pl->tps = std::max<long>(1, (ntiles + GP_MAX_SPLITS - 1) / GP_MAX_SPLITS);
    pl->nsplit = (int)((ntiles + pl->tps - 1) / pl->tps);
    pl->tmap_bytes = gb_align16(elems * (long)sizeof(float));
    // sized by a bound on nsplit that never shrinks when the tiles grow (nsplit itself can: 512 tiles are 256 splits of 2, 513 tiles 171 of 3)
    const long bound = std::min<long>(ntiles, GP_MAX_SPLITS);
    pl->bytes = pl->tmap_bytes + bound * ((long)c * c + c) * (long)sizeof(float);
    return 0;
}

size_t gb_lds_dx(int c) {
    const int g2p = c % 32 == 0 ? c + 16 : c;
    return ((size_t)2 * c * GB_PT + (size_t)std::max(c * GB_GP, GB_JS * g2p)) * sizeof(float);
}
}  // namespace

LIC360_API long lic360_gdn_backward_scratch_bytes(int n, int c, long p) {
    GbPlan pl;
    if (n <= 0 || p <= 0 || !gb_channels_ok(c) || gb_geometry(n, c, p, &pl)) return 0;
    return pl.bytes;
}

LIC360_API int lic360_gdn_backward(void *stream, const float *x, const float *gy, const float *gamma, const float *beta, float *gx, float *ggamma,
                                   float *gbeta, void *scratch, int n, int c, long p, int inverse) {
    ARG_CHECK(n >= 0 && p >= 0);
    ARG_CHECK(gb_channels_ok(c));
    ARG_CHECK((ggamma == nullptr) == (gbeta == nullptr));
    ARG_CHECK(((uintptr_t)scratch & 15) == 0);
    const bool need_p = ggamma != nullptr;
    if (!gx && !need_p) return 0;                                            // nothing asked for
    ARG_CHECK(n > 0 && p > 0);
    ARG_CHECK(x && gy && gamma && beta);
    ARG_CHECK(scratch || !need_p);
    GbPlan pl;
    ARG_CHECK(!gb_geometry(n, c, p, &pl));
    hipStream_t s = (hipStream_t)stream;
    float *tmap = need_p ? (float *)scratch : nullptr;
    float *partial = need_p ? (float *)((char *)scratch + pl.tmap_bytes) : nullptr;
    const bool vec = p % 4 == 0 && (((uintptr_t)x | (uintptr_t)gy | (uintptr_t)gx) & 15) == 0;
    const dim3 block(GB_THREADS), grid_dx((unsigned)pl.ntiles), grid_p((unsigned)pl.nsplit);
    const size_t lds_dx = gb_lds_dx(c), lds_p = (size_t)2 * c * GP_PITCH * sizeof(float);
#define GB_LAUNCH(CT_)                                                                                                                         \
    do {                                                                                                                                       \
        if (vec) hipLaunchKernelGGL((k_gdn_backward_dx<CT_, true>), grid_dx, block, lds_dx, s, x, gy, gamma, beta, gx, tmap, p, pl.tpi, inverse);  \
        else hipLaunchKernelGGL((k_gdn_backward_dx<CT_, false>), grid_dx, block, lds_dx, s, x, gy, gamma, beta, gx, tmap, p, pl.tpi, inverse);     \
        LAUNCH_CHECK();                                                                                                                        \
        if (need_p) {                                                                                                                          \
            if (vec) hipLaunchKernelGGL((k_gdn_backward_param<CT_, true>), grid_p, block, lds_p, s, x, tmap, partial, p, pl.tpi, pl.ntiles, pl.tps);  \
            else hipLaunchKernelGGL((k_gdn_backward_param<CT_, false>), grid_p, block, lds_p, s, x, tmap, partial, p, pl.tpi, pl.ntiles, pl.tps);     \
            LAUNCH_CHECK();                                                                                                                    \
        }                                                                                                                                      \
    } while (0)
    switch (c / 16) {
        case 1: GB_LAUNCH(1); break;   case 2: GB_LAUNCH(2); break;   case 3: GB_LAUNCH(3); break;   case 4: GB_LAUNCH(4); break;
        case 6: GB_LAUNCH(6); break;   case 8: GB_LAUNCH(8); break;   default: GB_LAUNCH(12); break;
    }
#undef GB_LAUNCH
    if (need_p) {
        const int total = c * c + c;
        hipLaunchKernelGGL(k_gdn_backward_finish, dim3((unsigned)((total + GB_THREADS - 1) / GB_THREADS)), block, 0, s, partial, ggamma, gbeta, c, pl.nsplit,
                           inverse);
        LAUNCH_CHECK();
    }
    return 0;
}
