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

// WIN: the window size when it is known at compile time (the 11 of the reference's SSIM(11, 3)), 0 = `win_rt` (any odd size up to 11)
template <bool NEAREST, int WIN>
__global__ __launch_bounds__(256) void k_viewport_quality(const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ tf,
                                                          double2 *__restrict__ partials, float *__restrict__ map, VqTaps taps, int win_rt, int n,
                                                          int c, int hs, int ws, int ho, int wo, int tiles_x, float c1, float c2) {
    __shared__ float sA[VQ_HALO * VQ_PITCH], sB[VQ_HALO * VQ_PITCH], sH[5][VQ_HALO * VQ_TILE];
    __shared__ double sR[2][4];
    const int win = WIN ? WIN : win_rt, r = win >> 1, hd = VQ_TILE + 2 * r;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
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
#pragma unroll
            for (int k = 0; k < (WIN ? WIN : VQ_MAX_WIN); ++k) {
                if (k < win) {
                    const float wk = taps.w[k], xa = ra[k], xb = rb[k];
                    ha = ha + wk * xa;
                    hb = hb + wk * xb;
                    haa = haa + wk * (xa * xa);
                    hbb = hbb + wk * (xb * xb);
                    hab = hab + wk * (xa * xb);
                }
            }
            sH[0][i] = ha;  sH[1][i] = hb;  sH[2][i] = haa;  sH[3][i] = hbb;  sH[4][i] = hab;
        }
        __syncthreads();
        float mu_a = 0.0f, mu_b = 0.0f, e_aa = 0.0f, e_bb = 0.0f, e_ab = 0.0f;
#pragma unroll
        for (int k = 0; k < (WIN ? WIN : VQ_MAX_WIN); ++k) {
            if (k < win) {
                const float wk = taps.w[k];
                const int o = (ty + k) * VQ_TILE + tx;
                mu_a = mu_a + wk * sH[0][o];
                mu_b = mu_b + wk * sH[1][o];
                e_aa = e_aa + wk * sH[2][o];
                e_bb = e_bb + wk * sH[3][o];
                e_ab = e_ab + wk * sH[4][o];
            }
        }
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

LIC360_API int lic360_viewport_quality(void *stream, const float *a, const float *b, const float *tf, int n, int c, int h, int w, int h_out, int w_out,
                                       int nearest, const float *taps, int window, void *scratch, float *mse, float *ssim, float *ssim_map) {
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
    VqTaps t{};
    for (int k = 0; k < window; ++k) t.w[k] = taps[k];
    // the two constants of SSIM.forward, as the fp32 tensor arithmetic there takes them
    const float c1 = (float)(0.01 * 0.01), c2 = (float)(0.03 * 0.03);
    const dim3 grid((unsigned)tiles, VQ_VIEWS, (unsigned)n);
    const int tiles_x = (w_out + VQ_TILE - 1) / VQ_TILE;
    double2 *partials = (double2 *)scratch;
#define VQ_LAUNCH(NEAR, WIN) \
    hipLaunchKernelGGL((k_viewport_quality<NEAR, WIN>), grid, dim3(256), 0, (hipStream_t)stream, a, b, tf, partials, ssim_map, t, window, n, c, h, w, h_out, w_out, tiles_x, c1, c2)
    if (nearest) { if (window == VQ_MAX_WIN) VQ_LAUNCH(true, VQ_MAX_WIN); else VQ_LAUNCH(true, 0); }
    else { if (window == VQ_MAX_WIN) VQ_LAUNCH(false, VQ_MAX_WIN); else VQ_LAUNCH(false, 0); }
#undef VQ_LAUNCH
    LAUNCH_CHECK();
    const int count = VQ_VIEWS * n;
    hipLaunchKernelGGL(k_viewport_quality_finish, dim3((count + 63) / 64), dim3(64), 0, (hipStream_t)stream, partials, mse, ssim, count, (int)tiles, (double)cells);
    LAUNCH_CHECK();
    return 0;
}
