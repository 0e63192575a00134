// gdn_bf16x3.inc -- the split-bf16 ("bf16x3") form of the one-pass GDN (csrc/gdn_kernels.hip, which includes this file behind k_gdn): the same
// operation and contract -- x, out [n][c][p] contiguous fp32, beta [c], inverse flag, P of any size and parity, x / out on 4-byte boundaries,
// nothing outside `out` written -- with the sum over input channels on bf16 MFMAs, opt-in (lic360_models.set_conv_precision(.., gdn="bf16x3")).
//
// Arithmetic.  sq = x * x in fp32 (one rounding; the library is built -ffp-contract=off).  sq and the effective gamma are each split into
// hi = bf16(v) and lo = bf16(v - hi) (both round to nearest even; v - hi is exact in fp32); each product is g_hi sq_hi + g_hi sq_lo + g_lo sq_hi on
// v_mfma_f32_16x16x32_bf16 accumulated in fp32; g_lo sq_lo is dropped.  The epilogue is k_gdn's and stays fp32: nrm = sqrtf(acc + beta[i]), x / nrm
// or x * nrm on the unsquared, unrounded fp32 x, with the correctly rounded sqrtf and / of -fno-fast-math.
//
// Contract.  hi + lo holds an operand to 2^-17 relative, the dropped term is below 2^-18 of a product.  Effective gamma >= 0 and beta > 0 by
// GDN.py's reparametrisation and x^2 >= 0, so no term of s = beta + sum gamma x^2 cancels another and s keeps a relative error of about 2^-16;
// its square root keeps 2^-17.  Worst-case fp32 accumulation adds (C + 1) 2^-24 to s, halved under the root; the roundings of x^2, sqrtf and / are
// at the 2^-24 level.  At C = 192 that is about 1.55e-5 per output element; the stated bound is 2^-15 RELATIVE PER ELEMENT against the float64
// GDN, for gamma >= 0 (twice the derived worst case).  A negative gamma is computed the same way, the bound then being relative to
// sum |gamma| x^2.  NaN, infinity and values whose square overflows fp32 are outside the contract.
//
// Mapping.  A workgroup (4 waves) owns 64 positions of one image and all C channels.
//   * Loading and the split happen once per workgroup, with no fp32 staging: a thread loads 4 channels x 4 consecutive positions (four 16-byte
//     loads, 16 lanes per 256-byte row piece), keeps them in registers for the epilogue, squares and splits them and writes half a 16-byte
//     cell (4 of its 8 channels) per position and part: the split image [hl][C / 8 channel groups][64 slots] x 16 bytes (a plane = 0 mod 64
//     banks, as in sconv_bf16x3.inc: the four kq planes of a ds_read_b128 fall on disjoint slots).  Position 4 q + t sits in slot 16 t + q, so
//     that the 16 lanes of a write hold consecutive cells, and MFMA position tile t, column c is position 4 c + t: a lane's accumulators of
//     the four position tiles are four CONSECUTIVE positions of one channel -- the epilogue's 16-byte accesses.
//   * Waves split the OUTPUT CHANNELS (and, at C / 16 not a multiple of 4, the position tiles): NCG channel groups x NPG = 4 / NCG position groups,
//     MT = C / 16 / NCG row tiles per wave.  A wave reads only its own share of the packed gamma, straight into A-operand registers: per K step
//     (32 input channels) MT x (hi, lo) 16-byte loads per lane, 1 KiB coalesced each, the next step's in flight during this step's MFMAs.
//   * K step: a position tile's B operands are two ds_read_b128 (hi, lo), used by MT x 3 MFMAs.
//   * Epilogue: nrm goes to LDS over the (consumed) split image as fp32 [C][64] -- the same 4 bytes per element -- and the loading threads, which
//     still hold the fp32 x, read it row-wise, divide or multiply and store 16 bytes per lane.
// LDS: 4 C x 64 bytes (48 KiB at C = 192: three workgroups per CU).  C in {32, 64, 96, 128, 192} (K = 32 per MFMA).  Measurements: DESIGN 7c⁗.
typedef __bf16 gb3_bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 gb3_bf4 __attribute__((ext_vector_type(4)));
typedef unsigned gb3_u4 __attribute__((ext_vector_type(4)));
typedef unsigned gb3_u2 __attribute__((ext_vector_type(2)));

#define GB3_PT 64                                                           // positions per workgroup
constexpr int gb3_ncg(int c) { return c / 16 % 4 == 0 ? 4 : 2; }           // channel groups of waves (192, 128, 64: 4; 96, 32: 2 x 2 position groups)
constexpr bool gb3_ok(int c) { return c == 32 || c == 64 || c == 96 || c == 128 || c == 192; }

// packed gamma: [cg < NCG][s < C / 32][m < MT][hl < 2][lane] x 8 bf16; lane l = 16 kq + i, element j: the hi (hl = 0) or lo (hl = 1) part of
// gamma[16 (cg MT + m) + i][32 s + 8 kq + j] -- the A operand of K step s for row tile m of a wave of channel group cg.  One thread per 16-byte cell.
__global__ void k_gdn_b3_pack(const float *__restrict__ gamma, gb3_u4 *__restrict__ packed, int c, int total) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int mt = c / 16 / gb3_ncg(c), ns = c / 32;
    const int lane = idx & 63;
    int r = idx >> 6;
    const int hl = r & 1; r >>= 1;
    const int m = r % mt; r /= mt;
    const int s = r % ns, cg = r / ns;
    const float *g = gamma + (long)(16 * (cg * mt + m) + (lane & 15)) * c + 32 * s + 8 * (lane >> 4);
    gb3_bf8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 h = (__bf16)g[j];
        o[j] = hl ? (__bf16)(g[j] - (float)h) : h;
    }
    packed[idx] = __builtin_bit_cast(gb3_u4, o);
}

template <int C, bool VEC>                                                  // VEC: 16-byte global accesses (P % 4 == 0, x and out on 16-byte boundaries)
__global__ __launch_bounds__(256) void k_gdn_b3(const float *__restrict__ x, const gb3_u4 *__restrict__ packed, const float *__restrict__ beta,
                                                float *__restrict__ out, long P, int inverse) {
    constexpr int NCG = gb3_ncg(C), NPG = 4 / NCG, MT = C / 16 / NCG, NTP = 4 / NPG, NS = C / 32, NG = C / 8;
    constexpr int NTASK = C / 4 * 16, TK = (NTASK + 255) / 256;            // loader tasks: (channel quad, position quad); per thread 3 at C = 192
    static_assert(gb3_ok(C) && MT * NCG * 16 == C, "channel count");
    extern __shared__ float lds[];
    gb3_u4 *sp = (gb3_u4 *)lds;                                             // split image [hl][NG][64] cells, then nrm fp32 [C][64]
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), cg = wave % NCG, pg = wave / NCG;
    const long n = blockIdx.y, p0 = (long)blockIdx.x * GB3_PT;
    const float *xn = x + n * C * P;
    float *on = out + n * C * P;
    // ---- x: every load is issued before the first use; past the end of the map: zeros (their outputs are not stored)
    gdn_f4 xr[TK][4];
#pragma unroll
    for (int k = 0; k < TK; ++k) {
        const int task = tid + 256 * k, q = task & 15, j0 = 8 * (task >> 5) + 4 * ((task >> 4) & 1);
        const long p = p0 + 4 * q;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xr[k][i] = (gdn_f4){0.f, 0.f, 0.f, 0.f};
            if (NTASK % 256 != 0 && task >= NTASK) continue;               // (wave-uniform: tasks come in multiples of 128)
            const float *row = xn + (long)(j0 + i) * P;
            if (VEC) {
                if (p < P) xr[k][i] = *(const gdn_f4 *)(row + p);
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (p + t < P) xr[k][i][t] = row[p + t];
            }
        }
    }
    // the wave's first A operands fly meanwhile
    const gb3_u4 *ap = packed + (long)cg * NS * MT * 2 * 64 + lane;         // + s * MT * 2 * 64 per K step, + (2 m + hl) * 64 per operand
    gb3_u4 A[2][MT * 2];
#pragma unroll
    for (int a = 0; a < MT * 2; ++a) A[0][a] = ap[a * 64];
    // ---- square, split, write the image: position 4 q + t -> slot 16 t + q
#pragma unroll
    for (int k = 0; k < TK; ++k) {
        const int task = tid + 256 * k, q = task & 15, half = (task >> 4) & 1, g = task >> 5;
        if (NTASK % 256 != 0 && task >= NTASK) continue;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            gb3_bf4 h, l;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float sq = xr[k][i][t] * xr[k][i][t];
                h[i] = (__bf16)sq;
                l[i] = (__bf16)(sq - (float)h[i]);
            }
            gb3_u2 *cell = (gb3_u2 *)(sp + g * GB3_PT + 16 * t + q) + half;
            cell[0] = __builtin_bit_cast(gb3_u2, h);
            cell[2 * NG * GB3_PT] = __builtin_bit_cast(gb3_u2, l);
        }
    }
    __syncthreads();
    // ---- the sum: K steps of 32 input channels
    gdn_f4 acc[MT][NTP];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int t = 0; t < NTP; ++t) acc[m][t] = (gdn_f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (s + 1 < NS) {
#pragma unroll
            for (int a = 0; a < MT * 2; ++a) A[(s + 1) & 1][a] = ap[((s + 1) * MT * 2 + a) * 64];
        }
        const gb3_u4 *bl = sp + (4 * s + kq) * GB3_PT + 16 * pg * NTP + col;
#pragma unroll
        for (int t = 0; t < NTP; ++t) {
            const gb3_bf8 bh = __builtin_bit_cast(gb3_bf8, bl[16 * t]), blo = __builtin_bit_cast(gb3_bf8, bl[NG * GB3_PT + 16 * t]);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const gb3_bf8 ah = __builtin_bit_cast(gb3_bf8, A[s & 1][2 * m]), alo = __builtin_bit_cast(gb3_bf8, A[s & 1][2 * m + 1]);
                acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, bh, acc[m][t], 0, 0, 0);
                acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, blo, acc[m][t], 0, 0, 0);
                acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc[m][t], 0, 0, 0);
            }
        }
    }
    __syncthreads();                                                         // every wave is done reading the split image
    // ---- nrm over the image: row i, positions 4 col + NTP pg .. (a lane's position tiles are consecutive positions)
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = 16 * (cg * MT + m) + 4 * kq + v;
            const float b = beta[i];
            float *cell = lds + i * GB3_PT + 4 * col + NTP * pg;
#pragma unroll
            for (int t = 0; t < NTP; ++t) cell[t] = sqrtf(acc[m][t][v] + b);
        }
    __syncthreads();
    // ---- y = x / nrm (x * nrm) by the threads that hold x, 16 bytes per lane
#pragma unroll
    for (int k = 0; k < TK; ++k) {
        const int task = tid + 256 * k, q = task & 15, j0 = 8 * (task >> 5) + 4 * ((task >> 4) & 1);
        if (NTASK % 256 != 0 && task >= NTASK) continue;
        const long p = p0 + 4 * q;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const gdn_f4 nr = *(const gdn_f4 *)(lds + (j0 + i) * GB3_PT + 4 * q);
            gdn_f4 r;
#pragma unroll
            for (int t = 0; t < 4; ++t) r[t] = inverse ? xr[k][i][t] * nr[t] : xr[k][i][t] / nr[t];
            float *row = on + (long)(j0 + i) * P;
            if (VEC) {
                if (p < P) *(gdn_f4 *)(row + p) = r;
            } else {
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (p + t < P) row[p + t] = r[t];
            }
        }
    }
}

LIC360_API int lic360_gdn_bf16x3_supported(int c) { return gb3_ok(c) ? 1 : 0; }

LIC360_API long lic360_gdn_bf16x3_packed_bytes(int c) { return gb3_ok(c) ? 4L * c * c : 0; }   // hi + lo: 2 x 2 bytes per gamma

// effective gamma [c][c] -> its hi and lo bf16 parts in the waves' A-operand order (packed_bytes bytes, 16-byte aligned)
LIC360_API int lic360_gdn_bf16x3_pack(void *stream, const float *gamma, void *packed, int c) {
    ARG_CHECK(gamma && packed && gb3_ok(c) && ((uintptr_t)packed & 15) == 0);
    const int total = c * c / 4;                                            // 16-byte cells
    hipLaunchKernelGGL(k_gdn_b3_pack, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, gamma, (gb3_u4 *)packed, c, total);
    LAUNCH_CHECK();
    return 0;
}

// x, out: [n][c][p] contiguous; packed: lic360_gdn_bf16x3_pack of the EFFECTIVE gamma; beta [c] effective (as lic360_gdn)
LIC360_API int lic360_gdn_bf16x3(void *stream, const float *x, const void *packed, const float *beta, float *out, int n, int c, long p, int inverse) {
    ARG_CHECK(x && packed && beta && out && n > 0 && n <= 65535 && p > 0 && p <= 0x7fffffffL * GB3_PT && gb3_ok(c) && ((uintptr_t)packed & 15) == 0);
    const dim3 grid((unsigned)((p + GB3_PT - 1) / GB3_PT), (unsigned)n);
    const size_t lds = (size_t)c * GB3_PT * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    const gb3_u4 *pk = (const gb3_u4 *)packed;
    const bool vec = p % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
#define GB3_LAUNCH(C_)                                                                                           \
    do {                                                                                                         \
        if (vec) hipLaunchKernelGGL((k_gdn_b3<C_, true>), grid, dim3(256), lds, s, x, pk, beta, out, p, inverse); \
        else hipLaunchKernelGGL((k_gdn_b3<C_, false>), grid, dim3(256), lds, s, x, pk, beta, out, p, inverse);    \
    } while (0)
    switch (c) {
        case 32: GB3_LAUNCH(32); break;     case 64: GB3_LAUNCH(64); break;     case 96: GB3_LAUNCH(96); break;
        case 128: GB3_LAUNCH(128); break;   default: GB3_LAUNCH(192); break;
    }
#undef GB3_LAUNCH
    LAUNCH_CHECK();
    return 0;
}
