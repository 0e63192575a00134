// viewport_quality_kernels.hip -- the viewport metrics of the evaluation mode (test/lic360_demo.py:406-449, test/eval_models.py:17-48) in one
// pass: an ERP pair -> mean squared error and mean SSIM of each of the 14 rectilinear viewports of each image.  Nothing of the size of the
// projected views [14 n][c][h_out][w_out] is written (DESIGN.md "Fused viewport metrics").
//   * k_viewport_quality: one workgroup of 256 threads per 16x16 tile of one viewport of one image, a loop over the channels.  Per channel:
//       gather      the tile and a halo of `win / 2` cells a side of both images into LDS, sampled by lic360_project_sample (the arithmetic of
//                   k_projects_forward, same tf table); cells outside the viewport are 0, the zero padding of conv2d(padding = win / 2);
//       horizontal  the `win` taps over a, b, a*a, b*b, a*b: halo rows x 16 columns of each, in LDS;
//       vertical    the `win` taps over those columns, in registers; then SSIM per cell in the operation order of lic360_operator/extras.py
//                   (SSIM.forward) and the squared difference of the cell's own samples.
//     Taps go in ascending order from a zero accumulator, one rounded product and one rounded sum each (the unit is built with
//     -ffp-contract=off).  Each thread sums its cells in double; the workgroup reduces in double (wave butterfly, then the four waves in wave
//     order) into its own slot of `partials`: no atomics, so the result does not depend on the order in which workgroups run.
//   * k_viewport_quality_finish: one thread per (image, viewport) adds the tiles' partials in ascending tile order, divides by c*h_out*w_out.
//   * k_viewport_quality<.., COEF = true> (lic360_viewport_quality_coef) and k_viewport_quality_backward (lic360_viewport_quality_backward): the
//     differentiable form, described at the backward kernel below.  The plain kernels are the COEF = false instantiations.
//   LDS: halo rows at a pitch of 48 floats.  The horizontal pass reads with 32-lane halves that span two halo rows x 16 columns; ds_read_b32
//   banks are (address / 4) % 32, so the second row has to start 16 banks after the first: pitch % 32 == 16, and 48 is the smallest such pitch
//   that holds 26 cells (at 26 the two rows share ten banks).  The row sums are [26][16] at pitch 16: the vertical pass's halves read two
//   adjacent rows = 32 consecutive floats.  2 * 26 * 48 * 4 + 5 * 26 * 16 * 4 + 64 = 18368 B (a 26-float pitch would make it about 14 KB; the pad costs
//   nothing: the registers, not the LDS, set the occupancy -- 79 VGPRs at window 11 leave 6 waves a SIMD, 6 workgroups a CU).
//   Precondition, as for lic360_projects_forward: every coordinate of `tf` must index inside an ERP plane.  A table whose viewport has a row that
//   looks exactly at a pole (a square viewport of fov 0.5 pitched by 45 degrees) has longitudes outside [0, w - 1] there;
//   lic360_projects_tf_inside tells on the host, and the Python shim refuses such a table before it launches.
#include "common.h"
#include "project_sample.h"
#include <cstdint>

namespace {
constexpr int VQ_TILE = 16, VQ_MAX_WIN = 11, VQ_HALO = VQ_TILE + VQ_MAX_WIN - 1, VQ_PITCH = 48, VQ_VIEWS = 14;
struct VqTaps { float w[VQ_MAX_WIN]; };
struct VqCoef { float *pa, *pb, *q, *r; };       // [14 n][c][h_out][w_out] each, the layout of ssim_map; pa or pb may be null

// The taps of one window pass of the backward kernel, ascending.  ROLLED = false: taps in scalar registers, the loop unrolled (the form of the plain forward
// kernels, which spell it out themselves so that their instructions stay what they were).  ROLLED = true, the run-time window of the kernels that came
// with the backward: taps from LDS in a rolled loop, which leaves the scalar registers that the unrolled form spends on eleven taps and their bounds
// (unrolled, those kernels spill 13 to 37 scalar registers into vector lanes; rolled, none).
template <int WIN, bool ROLLED, class F>
__device__ __forceinline__ void vq_for_taps(const VqTaps &taps, const float *lds_taps, int win, F body) {
    if constexpr (ROLLED) {
        for (int k = 0; k < win; ++k) body(k, lds_taps[k]);
    } else {
#pragma unroll
        for (int k = 0; k < (WIN ? WIN : VQ_MAX_WIN); ++k)
            if (k < win) body(k, taps.w[k]);
    }
}

// WIN: the window size when it is known at compile time (the 11 of the reference's SSIM(11, 3)), 0 = `win_rt` (any odd size up to 11)
// COEF: also store the four coefficient maps of the backward (VqCoef; see k_viewport_quality_backward) for the workgroup's own cells; `coef` is
// not read otherwise
template <bool NEAREST, int WIN, bool COEF>
__global__ __launch_bounds__(256) void k_viewport_quality(const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ tf,
                                                          double2 *__restrict__ partials, float *__restrict__ map, VqTaps taps, int win_rt, int n,
                                                          int c, int hs, int ws, int ho, int wo, int tiles_x, float c1, float c2, VqCoef coef) {
    __shared__ float sA[VQ_HALO * VQ_PITCH], sB[VQ_HALO * VQ_PITCH], sH[5][VQ_HALO * VQ_TILE];
    __shared__ double sR[2][4];
    constexpr bool ROLLED = COEF && !WIN;
    __shared__ float sT[ROLLED ? VQ_MAX_WIN : 1];
    const int win = WIN ? WIN : win_rt, r = win >> 1, hd = VQ_TILE + 2 * r;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    if constexpr (ROLLED) { if (tid < VQ_MAX_WIN) sT[tid] = taps.w[tid]; }   // (read after the channel loop's first barrier)
    const int tile = blockIdx.x, v = blockIdx.y, img = blockIdx.z, tiles = tiles_x * ((ho + VQ_TILE - 1) / VQ_TILE);
    const int y0 = tile / tiles_x * VQ_TILE, x0 = tile % tiles_x * VQ_TILE, gy = y0 + ty, gx = x0 + tx, inner = ho * wo;
    const bool own = gy < ho && gx < wo;                           // cells of a partial tile beyond the viewport contribute nothing
    const float2 *tfv = (const float2 *)tf + (long)v * inner;
    double ssim_sum = 0, sq_sum = 0;
    for (int ch = 0; ch < c; ++ch) {
        const float *pa = a + ((long)img * c + ch) * hs * ws, *pb = b + ((long)img * c + ch) * hs * ws;
        __syncthreads();                                           // the previous channel's readers of sA, sB and sH are done
        // (the coordinates are fetched again for every channel on purpose: kept in registers across the channel loop, with what the compiler then
        // hoists with them, the kernel needs 131 VGPRs instead of 79 and was measured slower, 0.46 against 0.40 ms at batch 8: DESIGN 7b')
        for (int i = tid; i < hd * hd; i += 256) {
            const int hy = i / hd, hx = i - hy * hd, y = y0 - r + hy, x = x0 - r + hx;
            float va = 0.0f, vb = 0.0f;
            if (y >= 0 && y < ho && x >= 0 && x < wo) {
                const float2 f = tfv[y * wo + x];
                va = lic360_project_sample<NEAREST>(pa, f, hs, ws);
                vb = lic360_project_sample<NEAREST>(pb, f, hs, ws);
            }
            sA[hy * VQ_PITCH + hx] = va;
            sB[hy * VQ_PITCH + hx] = vb;
        }
        __syncthreads();
        for (int i = tid; i < hd * VQ_TILE; i += 256) {
            const float *ra = sA + (i >> 4) * VQ_PITCH + (i & 15), *rb = sB + (i >> 4) * VQ_PITCH + (i & 15);
            float ha = 0.0f, hb = 0.0f, haa = 0.0f, hbb = 0.0f, hab = 0.0f;
#define VQ_ROW_TAP(WK)                      \
    {                                       \
        const float wk = WK, xa = ra[k], xb = rb[k]; \
        ha = ha + wk * xa;                  \
        hb = hb + wk * xb;                  \
        haa = haa + wk * (xa * xa);         \
        hbb = hbb + wk * (xb * xb);         \
        hab = hab + wk * (xa * xb);         \
    }
            if constexpr (ROLLED) {
                for (int k = 0; k < win; ++k) VQ_ROW_TAP(sT[k])
            } else {
#pragma unroll
                for (int k = 0; k < (WIN ? WIN : VQ_MAX_WIN); ++k) {
                    if (k < win) VQ_ROW_TAP(taps.w[k])
                }
            }
#undef VQ_ROW_TAP
            sH[0][i] = ha;  sH[1][i] = hb;  sH[2][i] = haa;  sH[3][i] = hbb;  sH[4][i] = hab;
        }
        __syncthreads();
        float mu_a = 0.0f, mu_b = 0.0f, e_aa = 0.0f, e_bb = 0.0f, e_ab = 0.0f;
#define VQ_COLUMN_TAP(WK)                   \
    {                                       \
        const float wk = WK;                \
        const int o = (ty + k) * VQ_TILE + tx; \
        mu_a = mu_a + wk * sH[0][o];        \
        mu_b = mu_b + wk * sH[1][o];        \
        e_aa = e_aa + wk * sH[2][o];        \
        e_bb = e_bb + wk * sH[3][o];        \
        e_ab = e_ab + wk * sH[4][o];        \
    }
        if constexpr (ROLLED) {
            for (int k = 0; k < win; ++k) VQ_COLUMN_TAP(sT[k])
        } else {
#pragma unroll
            for (int k = 0; k < (WIN ? WIN : VQ_MAX_WIN); ++k) {
                if (k < win) VQ_COLUMN_TAP(taps.w[k])
            }
        }
#undef VQ_COLUMN_TAP
        if (own) {
            // lic360_operator/extras.py, SSIM.forward: var = blur(x * x) - mu * mu;  m = ((2 mu_a mu_b + c1)(2 cov + c2)) / ((mu_a^2 + mu_b^2 + c1)(var_a + var_b + c2))
            const float var_a = e_aa - mu_a * mu_a, var_b = e_bb - mu_b * mu_b, cov = e_ab - mu_a * mu_b;
            const float num = (2.0f * mu_a * mu_b + c1) * (2.0f * cov + c2);
            const float den = (mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2);
            const float m = num / den;
            const float d = sA[(ty + r) * VQ_PITCH + tx + r] - sB[(ty + r) * VQ_PITCH + tx + r];
            ssim_sum += (double)m;
            sq_sum += (double)(d * d);
            if (map) map[((((long)v * n + img) * c + ch) * ho + gy) * wo + gx] = m;
            if constexpr (COEF) {
                // d m / d (mu_a, mu_b, E_aa = E_bb, E_ab) with A1, A2 the factors of num and B1, B2 those of den (DESIGN 7b'-grad), each operation rounded once
                const float a1 = 2.0f * mu_a * mu_b + c1, a2 = 2.0f * cov + c2, b1 = mu_a * mu_a + mu_b * mu_b + c1, b2 = var_a + var_b + c2;
                const float t1 = m / b1, t2 = m / b2, u = (a2 - a1) / den, dt = t2 - t1;
                const long o = ((((long)v * n + img) * c + ch) * ho + gy) * wo + gx;
                coef.q[o] = -t2;
                coef.r[o] = (2.0f * a1) / den;
                if (coef.pa) coef.pa[o] = 2.0f * (mu_b * u + mu_a * dt);
                if (coef.pb) coef.pb[o] = 2.0f * (mu_a * u + mu_b * dt);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        ssim_sum += __shfl_xor(ssim_sum, off);
        sq_sum += __shfl_xor(sq_sum, off);
    }
    if ((tid & 63) == 0) { sR[0][tid >> 6] = ssim_sum;  sR[1][tid >> 6] = sq_sum; }
    __syncthreads();
    if (tid == 0)
        partials[((long)img * VQ_VIEWS + v) * tiles + tile] = make_double2(((sR[0][0] + sR[0][1]) + sR[0][2]) + sR[0][3], ((sR[1][0] + sR[1][1]) + sR[1][2]) + sR[1][3]);
}

__global__ void k_viewport_quality_finish(const double2 *__restrict__ partials, float *__restrict__ mse, float *__restrict__ ssim, int count, int tiles,
                                          double cells) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double s = 0, q = 0;
    for (int t = 0; t < tiles; ++t) {
        const double2 p = partials[(long)i * tiles + t];
        s += p.x;
        q += p.y;
    }
    ssim[i] = (float)(s / cells);
    mse[i] = (float)(q / cells);
}

// The backward of the pair above for upstream gradients g_mse, g_ssim [n][14] (DESIGN "Fused viewport metrics: backward").  The forward's COEF form left,
// per view cell i, Q = d m_i / d E_aa = d m_i / d E_bb, R = d m_i / d E_ab, Pa = d m_i / d mu_a, Pb = d m_i / d mu_b.  The view-domain gradient of cell j is
//     gva_j = gs * (blurT(Pa)_j + 2 a_j blurT(Q)_j + b_j blurT(R)_j) + gm * 2 (a_j - b_j),        gs = g_ssim / N, gm = g_mse / N, N = c * h_out * w_out
// (gvb_j with a and b, Pa and Pb exchanged), blurT the adjoint of the zero-padded window pass: the same separable pass with the taps in reversed index
// order (`taps` arrives reversed, so the loops below are the forward's) over maps that are 0 outside the viewport.  Same mapping as the forward: one workgroup
// of 256 threads per 16x16 tile of one viewport of one image, a loop over the channels.  Per channel:
//     load      the tile and a halo of `win / 2` cells of Q, R and the live P maps into LDS (cells outside the viewport are 0 and are not read);
//     rows      the `win` taps along x: halo rows x 16 columns of each map, in LDS;
//     columns   the `win` taps along y, in registers; taps ascending from a zero accumulator, one rounded product and one rounded sum each;
//     gradient  xa, xb sampled again with lic360_project_sample, then in this order, every operation rounded once:
//                   t = bP + (2.0f * xa) * bQ;   t = t + xb * bR;   gva = gs * t + gm * (2.0f * (xa - xb))           (gvb: xa <-> xb, bPb)
//     scatter   lic360_project_scatter: weight * gv into grad_a / grad_b with float atomic adds (four per cell, one when NEAREST); the order in which
//               the adds of an ERP cell arrive is not fixed, so grad_a / grad_b can differ in their last bits from run to run (gva / gvb cannot).
// A side is live when its grad pointer is not null (a wave-uniform branch).  views_a / views_b: null, or [14 n][c][h_out][w_out] for gva / gvb.
// LDS: the pitches of the forward for the same two read patterns: 4 * 26 * 48 * 4 + 4 * 26 * 16 * 4 = 26624 B.
struct VqBackArgs {
    const float *a, *b, *tf, *pa, *pb, *q, *r, *g_mse, *g_ssim;
    float *grad_a, *grad_b, *views_a, *views_b;
    VqTaps taps;                                                    // reversed: taps.w[k] = window[win - 1 - k]
    int win_rt, n, c, hs, ws, ho, wo, tiles_x;
    float cells;                                                    // (float)(c * h_out * w_out)
};

template <bool NEAREST, int WIN>
__global__ __launch_bounds__(256) void k_viewport_quality_backward(VqBackArgs p) {
    __shared__ float sM[4][VQ_HALO * VQ_PITCH], sH[4][VQ_HALO * VQ_TILE];      // 0 Q, 1 R, 2 Pa, 3 Pb
    __shared__ float sT[VQ_MAX_WIN];
    const int win = WIN ? WIN : p.win_rt, r = win >> 1, hd = VQ_TILE + 2 * r;
    if (!WIN && threadIdx.x < VQ_MAX_WIN) sT[threadIdx.x] = p.taps.w[threadIdx.x];       // (read after the channel loop's first barrier)
    const int n = p.n, c = p.c, hs = p.hs, ws = p.ws, ho = p.ho, wo = p.wo;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int tile = blockIdx.x, v = blockIdx.y, img = blockIdx.z;
    const int y0 = tile / p.tiles_x * VQ_TILE, x0 = tile % p.tiles_x * VQ_TILE, gy = y0 + ty, gx = x0 + tx;
    const bool own = gy < ho && gx < wo, live_a = p.grad_a != nullptr, live_b = p.grad_b != nullptr;
    const float gs = p.g_ssim[img * VQ_VIEWS + v] / p.cells, gm = p.g_mse[img * VQ_VIEWS + v] / p.cells;
    float2 f = make_float2(0.0f, 0.0f);
    if (own) f = ((const float2 *)p.tf)[(long)v * ho * wo + gy * wo + gx];
    const float *maps[4] = {p.q, p.r, p.pa, p.pb};
    for (int ch = 0; ch < c; ++ch) {
        const long plane = (((long)v * n + img) * c + ch) * ho * wo, erp = ((long)img * c + ch) * hs * ws;
        __syncthreads();                                           // the previous channel's readers of sM and sH are done
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if ((m == 2 && !live_a) || (m == 3 && !live_b)) continue;
            const float *src = maps[m] + plane;
            for (int i = tid; i < hd * hd; i += 256) {
                const int hy = i / hd, hx = i - hy * hd, y = y0 - r + hy, x = x0 - r + hx;
                sM[m][hy * VQ_PITCH + hx] = (y >= 0 && y < ho && x >= 0 && x < wo) ? src[y * wo + x] : 0.0f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if ((m == 2 && !live_a) || (m == 3 && !live_b)) continue;
            for (int i = tid; i < hd * VQ_TILE; i += 256) {
                const float *row = sM[m] + (i >> 4) * VQ_PITCH + (i & 15);
                float h = 0.0f;
                vq_for_taps<WIN, !WIN>(p.taps, sT, win, [&](int k, float wk) { h = h + wk * row[k]; });
                sH[m][i] = h;
            }
        }
        __syncthreads();
        float bl[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if ((m == 2 && !live_a) || (m == 3 && !live_b)) continue;
            vq_for_taps<WIN, !WIN>(p.taps, sT, win, [&](int k, float wk) { bl[m] = bl[m] + wk * sH[m][(ty + k) * VQ_TILE + tx]; });
        }
        if (own) {
            const float xa = lic360_project_sample<NEAREST>(p.a + erp, f, hs, ws), xb = lic360_project_sample<NEAREST>(p.b + erp, f, hs, ws);
            const long o = plane + gy * wo + gx;
            if (live_a) {
                float t = bl[2] + (2.0f * xa) * bl[0];
                t = t + xb * bl[1];
                const float gva = gs * t + gm * (2.0f * (xa - xb));
                if (p.views_a) p.views_a[o] = gva;
                lic360_project_scatter<NEAREST>(p.grad_a + erp, f, hs, ws, gva);
            }
            if (live_b) {
                float t = bl[3] + (2.0f * xb) * bl[0];
                t = t + xa * bl[1];
                const float gvb = gs * t + gm * (2.0f * (xb - xa));
                if (p.views_b) p.views_b[o] = gvb;
                lic360_project_scatter<NEAREST>(p.grad_b + erp, f, hs, ws, gvb);
            }
        }
    }
}

long vq_tiles(int h_out, int w_out) { return (long)((h_out + VQ_TILE - 1) / VQ_TILE) * ((w_out + VQ_TILE - 1) / VQ_TILE); }
bool vq_disjoint(const void *p, size_t np, const void *q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a + np <= b || b + nq <= a;
}
}  // namespace

LIC360_API long lic360_viewport_quality_scratch_bytes(int n, int h_out, int w_out) {
    if (n < 1 || h_out < 1 || w_out < 1) return 0;
    return (long)sizeof(double2) * n * VQ_VIEWS * vq_tiles(h_out, w_out);
}

namespace {
// both forward entries: the checks, then the launch of the plain form (coef == nullptr) or of the COEF form
int vq_forward(void *stream, const float *a, const float *b, const float *tf, int n, int c, int h, int w, int h_out, int w_out, int nearest,
               const float *taps, int window, void *scratch, float *mse, float *ssim, float *ssim_map, const VqCoef *coef) {
    ARG_CHECK(a && b && tf && taps && scratch && mse && ssim);
    ARG_CHECK(n >= 1 && n <= 65535 && c >= 1 && h > 0 && w > 0 && h_out > 0 && w_out > 0);
    ARG_CHECK(window >= 1 && window <= VQ_MAX_WIN && window % 2 == 1);
    const long tiles = vq_tiles(h_out, w_out), cells = (long)c * h_out * w_out;
    ARG_CHECK((long)h * w <= 0x7fffffffL && (long)h_out * w_out <= 0x7fffffffL);          // the kernels index one plane with an int
    ARG_CHECK((uintptr_t)scratch % alignof(double2) == 0);
    const size_t out_bytes = sizeof(float) * VQ_VIEWS * (size_t)n, scratch_bytes = (size_t)lic360_viewport_quality_scratch_bytes(n, h_out, w_out);
    const size_t map_bytes = ssim_map ? sizeof(float) * VQ_VIEWS * (size_t)n * (size_t)cells : 0;
    ARG_CHECK(vq_disjoint(mse, out_bytes, ssim, out_bytes) && vq_disjoint(mse, out_bytes, scratch, scratch_bytes) && vq_disjoint(ssim, out_bytes, scratch, scratch_bytes));
    ARG_CHECK(!ssim_map || (vq_disjoint(ssim_map, map_bytes, mse, out_bytes) && vq_disjoint(ssim_map, map_bytes, ssim, out_bytes) &&
                            vq_disjoint(ssim_map, map_bytes, scratch, scratch_bytes)));
    if (coef) {
        ARG_CHECK(coef->q && coef->r && (coef->pa || coef->pb));
        const size_t coef_bytes = sizeof(float) * VQ_VIEWS * (size_t)n * (size_t)cells;
        const void *cp[4] = {coef->pa, coef->pb, coef->q, coef->r};
        for (int i = 0; i < 4; ++i) {
            if (!cp[i]) continue;
            ARG_CHECK(vq_disjoint(cp[i], coef_bytes, mse, out_bytes) && vq_disjoint(cp[i], coef_bytes, ssim, out_bytes) && vq_disjoint(cp[i], coef_bytes, scratch, scratch_bytes));
            ARG_CHECK(vq_disjoint(cp[i], coef_bytes, a, sizeof(float) * (size_t)n * c * h * w) && vq_disjoint(cp[i], coef_bytes, b, sizeof(float) * (size_t)n * c * h * w));
            for (int j = i + 1; j < 4; ++j) ARG_CHECK(!cp[j] || vq_disjoint(cp[i], coef_bytes, cp[j], coef_bytes));
        }
    }
    VqTaps t{};
    for (int k = 0; k < window; ++k) t.w[k] = taps[k];
    // the two constants of SSIM.forward, as the fp32 tensor arithmetic there takes them
    const float c1 = (float)(0.01 * 0.01), c2 = (float)(0.03 * 0.03);
    const dim3 grid((unsigned)tiles, VQ_VIEWS, (unsigned)n);
    const int tiles_x = (w_out + VQ_TILE - 1) / VQ_TILE;
    double2 *partials = (double2 *)scratch;
#define VQ_LAUNCH(NEAR, WIN)                                                                                                                        \
    do {                                                                                                                                           \
        if (coef) hipLaunchKernelGGL((k_viewport_quality<NEAR, WIN, true>), grid, dim3(256), 0, (hipStream_t)stream, a, b, tf, partials, ssim_map, t, window, n, c, h, w, h_out, w_out, tiles_x, c1, c2, *coef); \
        else hipLaunchKernelGGL((k_viewport_quality<NEAR, WIN, false>), grid, dim3(256), 0, (hipStream_t)stream, a, b, tf, partials, ssim_map, t, window, n, c, h, w, h_out, w_out, tiles_x, c1, c2, VqCoef{}); \
    } while (0)
    if (nearest) { if (window == VQ_MAX_WIN) VQ_LAUNCH(true, VQ_MAX_WIN); else VQ_LAUNCH(true, 0); }
    else { if (window == VQ_MAX_WIN) VQ_LAUNCH(false, VQ_MAX_WIN); else VQ_LAUNCH(false, 0); }
#undef VQ_LAUNCH
    LAUNCH_CHECK();
    const int count = VQ_VIEWS * n;
    hipLaunchKernelGGL(k_viewport_quality_finish, dim3((count + 63) / 64), dim3(64), 0, (hipStream_t)stream, partials, mse, ssim, count, (int)tiles, (double)cells);
    LAUNCH_CHECK();
    return 0;
}
}  // namespace

LIC360_API int lic360_viewport_quality(void *stream, const float *a, const float *b, const float *tf, int n, int c, int h, int w, int h_out, int w_out,
                                       int nearest, const float *taps, int window, void *scratch, float *mse, float *ssim, float *ssim_map) {
    return vq_forward(stream, a, b, tf, n, c, h, w, h_out, w_out, nearest, taps, window, scratch, mse, ssim, ssim_map, nullptr);
}

LIC360_API int lic360_viewport_quality_coef(void *stream, const float *a, const float *b, const float *tf, int n, int c, int h, int w, int h_out, int w_out,
                                            int nearest, const float *taps, int window, void *scratch, float *mse, float *ssim, float *coef_pa,
                                            float *coef_pb, float *coef_q, float *coef_r) {
    const VqCoef coef{coef_pa, coef_pb, coef_q, coef_r};
    return vq_forward(stream, a, b, tf, n, c, h, w, h_out, w_out, nearest, taps, window, scratch, mse, ssim, nullptr, &coef);
}

LIC360_API int lic360_viewport_quality_backward(void *stream, const float *a, const float *b, const float *tf, int n, int c, int h, int w, int h_out,
                                                int w_out, int nearest, const float *taps, int window, const float *coef_pa, const float *coef_pb,
                                                const float *coef_q, const float *coef_r, const float *grad_mse, const float *grad_ssim, float *grad_a,
                                                float *grad_b, float *grad_views_a, float *grad_views_b) {
    ARG_CHECK(a && b && tf && taps && coef_q && coef_r && grad_mse && grad_ssim);
    ARG_CHECK(grad_a || grad_b);
    ARG_CHECK((grad_a != nullptr) == (coef_pa != nullptr) && (grad_b != nullptr) == (coef_pb != nullptr));
    ARG_CHECK((!grad_views_a || grad_a) && (!grad_views_b || grad_b));
    ARG_CHECK(n >= 1 && n <= 65535 && c >= 1 && h > 0 && w > 0 && h_out > 0 && w_out > 0);
    ARG_CHECK(window >= 1 && window <= VQ_MAX_WIN && window % 2 == 1);
    ARG_CHECK((long)h * w <= 0x7fffffffL && (long)h_out * w_out <= 0x7fffffffL);          // the kernel indexes one plane with an int
    const long tiles = vq_tiles(h_out, w_out), cells = (long)c * h_out * w_out;
    const size_t erp_bytes = sizeof(float) * (size_t)n * c * h * w, view_bytes = sizeof(float) * VQ_VIEWS * (size_t)n * (size_t)cells;
    const size_t up_bytes = sizeof(float) * VQ_VIEWS * (size_t)n;
    const void *out[4] = {grad_a, grad_b, grad_views_a, grad_views_b}, *in[8] = {a, b, coef_pa, coef_pb, coef_q, coef_r, grad_mse, grad_ssim};
    const size_t out_bytes[4] = {erp_bytes, erp_bytes, view_bytes, view_bytes};
    const size_t in_bytes[8] = {erp_bytes, erp_bytes, view_bytes, view_bytes, view_bytes, view_bytes, up_bytes, up_bytes};
    for (int i = 0; i < 4; ++i) {                                  // what is written overlaps nothing that is read or written
        if (!out[i]) continue;
        for (int j = i + 1; j < 4; ++j) ARG_CHECK(!out[j] || vq_disjoint(out[i], out_bytes[i], out[j], out_bytes[j]));
        for (int j = 0; j < 8; ++j) ARG_CHECK(!in[j] || vq_disjoint(out[i], out_bytes[i], in[j], in_bytes[j]));
    }
    VqBackArgs p{};
    p.a = a;  p.b = b;  p.tf = tf;  p.pa = coef_pa;  p.pb = coef_pb;  p.q = coef_q;  p.r = coef_r;  p.g_mse = grad_mse;  p.g_ssim = grad_ssim;
    p.grad_a = grad_a;  p.grad_b = grad_b;  p.views_a = grad_views_a;  p.views_b = grad_views_b;
    for (int k = 0; k < window; ++k) p.taps.w[k] = taps[window - 1 - k];
    p.win_rt = window;  p.n = n;  p.c = c;  p.hs = h;  p.ws = w;  p.ho = h_out;  p.wo = w_out;  p.tiles_x = (w_out + VQ_TILE - 1) / VQ_TILE;
    p.cells = (float)cells;
    if (grad_a) HIP_TRY(hipMemsetAsync(grad_a, 0, erp_bytes, (hipStream_t)stream));
    if (grad_b) HIP_TRY(hipMemsetAsync(grad_b, 0, erp_bytes, (hipStream_t)stream));
    const dim3 grid((unsigned)tiles, VQ_VIEWS, (unsigned)n);
#define VQ_LAUNCH(NEAR, WIN) hipLaunchKernelGGL((k_viewport_quality_backward<NEAR, WIN>), grid, dim3(256), 0, (hipStream_t)stream, p)
    if (nearest) { if (window == VQ_MAX_WIN) VQ_LAUNCH(true, VQ_MAX_WIN); else VQ_LAUNCH(true, 0); }
    else { if (window == VQ_MAX_WIN) VQ_LAUNCH(false, VQ_MAX_WIN); else VQ_LAUNCH(false, 0); }
#undef VQ_LAUNCH
    LAUNCH_CHECK();
    return 0;
}
