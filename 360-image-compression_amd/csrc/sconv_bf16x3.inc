// sconv_bf16x3.inc -- the split-bf16 ("bf16x3") form of the transforms' sphere convolutions (csrc/conv3x3_kernels.hip): the same
// operation -- sphere apron read by index, output window (ring, ring_w), tall last tile row, crop, x2 pixel-shuffle store, bias + PReLU +
// residual in the epilogue, cells outside the window untouched -- on bf16 MFMAs, opt-in (lic360_models.set_conv_precision).
//
// Arithmetic.  Every fp32 operand v becomes hi = bf16(v) and lo = bf16(v - hi) (both round to nearest even; v - hi is exact in fp32); each
// product is w_hi x_hi + w_hi x_lo + w_lo x_hi on v_mfma_f32_16x16x32_bf16, accumulated in fp32.  hi + lo holds v to 2^-17 relative, the
// dropped w_lo x_lo is below 2^-16 of the product: about 2^-16 relative per product (fp32: 2^-24), i.e. 1e-4 parity with a library convolution
// on the transforms' data.  Three 16x16x32 bf16 MFMAs (16 cycles each) do the K = 32 that eight 16x16x4 fp32 MFMAs (32 cycles each) do:
// 3/16 of the matrix time.  Inference only; NaN / infinity and values within 2^-8 of FLT_MAX are outside the contract.
//
// Mapping.  As the fp32 body: M = output channels, N = positions, K = (input channel, tap); a workgroup (8 waves, two per SIMD) owns a 16 x 16
// tile (or the tall last tile row) of one image and NQ * 48 output channels, wave (mq, nh) 3 row tiles x RW rows in 12 RW accumulator registers.
// K step = 32 input channels of one tap (kw, kh): lane (kq, i) of the A operand holds W[co = 48 mq + 16 mt + i][ci = 32 cg + 8 kq + j][kh][kw],
// j < 8, lane (kq, col) of the B operand x[ci = 32 cg + 8 kq + j] at (row + kh, col + kw).  Input channels arrive in chunks of 32: their halo
// tiles go by the fp32 body's per-lane LDS-DMA (sphere rule by index) to a double-buffered fp32 staging image, one chunk ahead.
//
// Where the split happens: ONCE per chunk, in a conversion pass over the LDS halo tile (not at fragment-read time, where each of the NQ waves
// that share a row group would split the same values again, from 8 strided ds_read_b32 per operand).  Each lane of the pass reads 8 channels of
// one halo cell (ds_read_b32, conflict-free: consecutive lanes, consecutive cells), converts them (8 v_cvt to bf16 + 8 subtractions + 8 more
// conversions) and writes one 16-byte hi cell and one 16-byte lo cell; a B operand is then one ds_read_b128 for hi and one for lo.  Split image:
// [hl][kq < 4][PS cells] x 16 bytes, PS = halo cells rounded up to 16 (a plane = 0 mod 64 banks: the four kq planes of a ds_read_b128 fall
// on disjoint banks, the 16 columns of a lane group on all 64).  Cost: 3 pass iterations per lane and chunk and a second barrier per chunk
// against 648 MFMAs per wave (192 channels, 3x3); measurements: DESIGN 7c'.
// Included by conv3x3_kernels.hip behind its fp32 body (one translation unit; the tests that check every M0-writing translation unit compile it).
// This file holds only what the form does differently: the split, the weight pack kernel and b3_body's chunk loop.  S3Args, the LDS-DMA helpers,
// the sphere rule, the loader's cell offsets (s3_cell_offsets), the epilogue (s3_epilogue), the kernel wrapper, the launch and the C entry
// points are that file's, shared with the fp32 body.
//
// The single-pass form ("bf16x1", NT = 1 below; kernels k_sconv_b1).  The same body with the lo parts left out: every input value and every weight is
// rounded ONCE to bf16 (nearest even) and each product is one MFMA, w_hi x_hi, accumulated in fp32 -- the fp32-accumulated convolution of the rounded
// operands (about 2^-8 relative per operand); bias, PReLU and residual stay fp32 in the shared epilogue.  What NT = 1 changes: the conversion pass writes
// hi cells only (split image: 4 planes, not 8), the pack holds hi planes only (2 bytes per weight), a K step loads three A operands (one 3 KiB block per
// wave, one address register) and issues one MFMA per (row, row tile).  Loader, staging, chunk, counted waits, barriers and epilogue are the split form's.
#include <type_traits>

typedef __bf16 b3_bf8 __attribute__((ext_vector_type(8)));
typedef unsigned b3_u4 __attribute__((ext_vector_type(4)));

#define B3_THREADS S3_THREADS
#define B3_CK 32                                                            // input channels per chunk (= the K of one MFMA)
constexpr int b3_ndma(int ncell) { return (B3_CK * ncell + 511) / 512; }   // DMA instructions per wave and chunk (fp32 staging pitch = halo cells)
constexpr int b3_ps(int ncell) { return (ncell + 15) / 16 * 16; }          // split-image plane pitch in 16-byte cells
// LDS floats of a body: two fp32 staging buffers + the split image (hi and lo, or at NT = 1 hi only: 4 planes of PS 16-byte cells each)
constexpr int b3_lds(int tr, int ks, int nt = 3) {
    return 2 * 8 * b3_ndma((tr + ks - 1) * (S3_T + ks - 1)) * 64 + (nt == 3 ? 32 : 16) * b3_ps((tr + ks - 1) * (S3_T + ks - 1));
}

__device__ __forceinline__ b3_u4 b3_split(const float (&v)[8], bool lo) {  // 8 values -> their bf16 hi (lo = false) or lo parts, packed
    b3_bf8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 h = (__bf16)v[j];
        r[j] = lo ? (__bf16)(v[j] - (float)h) : h;
    }
    return __builtin_bit_cast(b3_u4, r);
}

// weights: [cout block of NQ * 48][it = (cg * ks + kw) * ks + kh < cin / 32 * ks * ks][mq][mt < 3][hl < 2][lane] x 8 bf16; lane l = 16 kq + i,
// element j: the hi (hl = 0) or lo (hl = 1) part of W[co = 48 mq + 16 mt + i][ci = 32 cg + 8 kq + j][kh][kw] -- the A operand of the K step
// (cg, kw, kh) for row tile mt; a wave reads its six operands of a step as one 6 KiB block.  One thread per 16-byte cell.
// nhl = 1 (the single-pass form's pack): no hl index, hi parts only -- three operands, 3 KiB per wave and step.
__global__ void k_sconv_b3_pack(const float *__restrict__ w, b3_u4 *__restrict__ packed, int cin, int cout, int nq, int ks, int nhl, long total) {
    const int nit = cin / B3_CK * ks * ks;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(idx & 63);
        long r = idx >> 6;
        const int hl = (int)(r % nhl); r /= nhl;
        const int mt = (int)(r % 3); r /= 3;
        const int mq = (int)(r % nq); r /= nq;
        const int it = (int)(r % nit), blk = (int)(r / nit);
        const int kh = it % ks, kw = it / ks % ks, cg = it / (ks * ks);
        const int co = blk * nq * 48 + 48 * mq + 16 * mt + (lane & 15), ci0 = B3_CK * cg + 8 * (lane >> 4);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = w[(((long)co * cin + ci0 + j) * ks + kh) * ks + kw];
        packed[idx] = b3_split(v, hl != 0);
    }
}

// NQ * 48 output channels per workgroup, RW rows per wave, KS x KS taps, NT bf16 MFMAs per product: 3 = the split form, 1 = single pass (hi parts only);
// ST = 2: the 1x1 at stride 2 (tile and window in the OUTPUT's grid, even / even source cells: s3_cell_offset; the 3x3 at stride 2 is sconv_b1s2.inc)
template <int NQ, int RW, int KS, int NT = 3, int ST = 1, int GT = 0, int PQ = NQ>   // GT: the gate epilogue (s3_epilogue<RW, 1, 1>, the 1x1 at stride 1); PQ: the pack's NQ (s3_body)
__device__ __forceinline__ void b3_body(const S3Args &a, float *lds, int ty, int tx, int img, const float *trunk = nullptr) {
    constexpr int NR = 8 / NQ, TR = NR * RW, XR = TR + KS - 1, XC = S3_T + KS - 1, NCELL = XR * XC;
    constexpr int NDMA = b3_ndma(NCELL), BUF = 8 * NDMA * 64, PS = b3_ps(NCELL), NSTEP = KS * KS;
    constexpr int NA = NT == 3 ? 6 : 3;                                     // A operands of a K step: (row tile, hi | lo), or the row tiles' hi parts
    static_assert(NT == 3 || NT == 1, "split (hi + lo) or single pass (hi)");
    static_assert(ST == 1 || (ST == 2 && KS == 1), "the stride-2 1x1 has the stride-1 image");
    static_assert(NDMA <= 63, "s_waitcnt vmcnt takes at most 63 on gfx950");
    float (*xs)[BUF] = (float (*)[BUF])lds;
    b3_u4 *sp = (b3_u4 *)(lds + 2 * BUF);                                   // split image [hl][kq][PS] (NT = 1: [kq][PS])
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), mq = wave % NQ, nh = wave / NQ;
    const int tr0 = (ST == 1 ? a.ring : 0) + ty * (NR * a.rw), tc0 = (ST == 1 ? a.ringw : 0) + tx * S3_T;
    const int blk = PQ == NQ ? blockIdx.y : blockIdx.y / (PQ / NQ), pmq = PQ == NQ ? mq : (int)(blockIdx.y % (PQ / NQ)) * NQ + mq;   // pack block, mq slot in it
    const long PLg = (long)a.hp * a.wp;
    unsigned voff[NDMA];
    if constexpr (PQ == NQ) s3_cell_offsets<NDMA, B3_CK, NCELL, XR, XC, KS, ST>(a, tr0, tc0, wave, lane, PLg, voff);
    else {                                                                  // (narrow: one offset finished before the next begins -- the 30 of the 24-row tile otherwise keep their lane masks in scalars)
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            voff[i] = s3_cell_offset<B3_CK, NCELL, XR, XC, KS, ST>(a, tr0, tc0, (i * 8 + wave) * 64 + lane, PLg);
            asm volatile("" : "+v"(voff[i]));
        }
    }
    const float *xb = a.x + (long)img * a.cin * PLg;
    const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) const float *)&xs[0][0];
    auto issue_dma = [&](const float *sb0, int buf) __attribute__((always_inline)) {
        const float *sb = s3_uniform(sb0);
        unsigned lb = lds0 + (unsigned)(buf * BUF + wave * 64) * 4u;
        if constexpr (PQ != NQ) asm volatile("" : "+s"(lb));               // (narrow: the NDMA LDS addresses are made per call, not kept in as many scalar registers across the chunk loop)
#pragma unroll
        for (int i = 0; i < NDMA; ++i) s3_dma(voff[i], sb, lb + (unsigned)(i * 8 * 64 * 4));
    };
    const int nck = a.cin / B3_CK, niter = nck * NSTEP;
    // A operands: six 16-byte loads per lane and K step (two address registers: the offset field stops at 4 KiB; NT = 1: three loads, one register), one
    // step ahead, waited for by counted vmcnt as in the fp32 body: the chunk's DMAs are issued behind the loads of its second step, so the wait at step 1 skips them
    const char *wl = (const char *)a.w + (((long)blk * niter * PQ + pmq) * NA * 64 + lane) * 16;   // + it * PQ * NA KiB per K step
    auto load_a = [&](int it, b3_u4 (&A)[NA]) __attribute__((always_inline)) {
        const char *p = wl + (long)it * (PQ * NA * 1024);
        if constexpr (NA == 6) {
            const char *q = p + 3072;
            asm volatile("global_load_dwordx4 %0, %6, off\n\tglobal_load_dwordx4 %1, %6, off offset:1024\n\tglobal_load_dwordx4 %2, %6, off offset:2048\n\t"
                         "global_load_dwordx4 %3, %7, off\n\tglobal_load_dwordx4 %4, %7, off offset:1024\n\tglobal_load_dwordx4 %5, %7, off offset:2048"
                         : "=&v"(A[0]), "=&v"(A[1]), "=&v"(A[2]), "=&v"(A[3]), "=&v"(A[4]), "=&v"(A[5]) : "v"(p), "v"(q));
        } else
            asm volatile("global_load_dwordx4 %0, %3, off\n\tglobal_load_dwordx4 %1, %3, off offset:1024\n\tglobal_load_dwordx4 %2, %3, off offset:2048"
                         : "=&v"(A[0]), "=&v"(A[1]), "=&v"(A[2]) : "v"(p));
    };
#define B3_WAIT_A(N, A_)                                                                                                                                     \
    do {                                                                                                                                                     \
        if constexpr (NA == 6) asm volatile("s_waitcnt vmcnt(%6)" : "+v"(A_[0]), "+v"(A_[1]), "+v"(A_[2]), "+v"(A_[3]), "+v"(A_[4]), "+v"(A_[5]) : "n"(N)); \
        else asm volatile("s_waitcnt vmcnt(%3)" : "+v"(A_[0]), "+v"(A_[1]), "+v"(A_[2]) : "n"(N));                                                           \
    } while (0)
    s3_f4 acc[3][RW];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[m][r] = (s3_f4){0.f, 0.f, 0.f, 0.f};
    b3_u4 A[2][NA];                                                         // operand ring: K step `it` in set it & 1
    issue_dma(xb, 0);
    load_a(0, A[0]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // one chunk; P = ck & 1 makes the operand set of every step static (NSTEP is odd)
    auto chunk = [&](int ck, auto par) __attribute__((always_inline)) {
        constexpr int P = decltype(par)::value;
        // the split pass: fp32 staging buffer ck & 1 -> the split image (its last readers passed the barrier that ended the previous chunk)
        const float *xf = xs[ck & 1];
#pragma unroll
        for (int c0 = 0; c0 < 4 * NCELL; c0 += B3_THREADS) {
            const int c = c0 + tid;
            if (c0 + B3_THREADS <= 4 * NCELL || c < 4 * NCELL) {
                const int g = c / NCELL, pos = c - g * NCELL;
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = xf[(8 * g + j) * NCELL + pos];
                sp[g * PS + pos] = b3_split(v, false);
                if constexpr (NT == 3) sp[(4 + g) * PS + pos] = b3_split(v, true);
            }
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < NSTEP; ++p) {
            const int kw = p / KS, kh = p - KS * kw, sa = (P * NSTEP + p) & 1;
            // in-order counter: behind step 1's operands come only the chunk's DMAs (issued at step 0); at step 0 the end-of-chunk wait covered it
            if (p == 1) B3_WAIT_A(NDMA, A[sa]);
            else if (p > 1) B3_WAIT_A(0, A[sa]);
            const int itn = ck * NSTEP + p + 1;
            load_a(itn < niter ? itn : niter - 1, A[sa ^ 1]);
            if (p == 0) issue_dma(ck + 1 < nck ? xb + (long)(ck + 1) * B3_CK * PLg : xb, (ck + 1) & 1);   // the last chunk's are harmless loads into the idle buffer
            const b3_u4 *bl = sp + kq * PS + (nh * RW + kh) * XC + col + kw;
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const b3_bf8 bh = __builtin_bit_cast(b3_bf8, bl[r * XC]);
                if constexpr (NT == 3) {
                    const b3_bf8 blo = __builtin_bit_cast(b3_bf8, bl[4 * PS + r * XC]);
#pragma unroll
                    for (int m = 0; m < 3; ++m) {
                        const b3_bf8 ah = __builtin_bit_cast(b3_bf8, A[sa][2 * m]), alo = __builtin_bit_cast(b3_bf8, A[sa][2 * m + 1]);
                        acc[m][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(alo, bh, acc[m][r], 0, 0, 0);
                        acc[m][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, blo, acc[m][r], 0, 0, 0);
                        acc[m][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc[m][r], 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int m = 0; m < 3; ++m) acc[m][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b3_bf8, A[sa][m]), bh, acc[m][r], 0, 0, 0);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // the next chunk's DMAs have landed (and its first operands)
        __syncthreads();
    };
    for (int ck = 0; ck < nck; ck += 2) {
        chunk(ck, std::integral_constant<int, 0>{});
        if (ck + 1 < nck) chunk(ck + 1, std::integral_constant<int, 1>{});
    }
#undef B3_WAIT_A
    if constexpr (GT) s3_epilogue<RW, 1, 1>(a, acc, img, tr0, tc0, blk * PQ * 48 + 48 * pmq, nh, col, kq, PLg, trunk);
    else if constexpr (ST == 1) s3_epilogue<RW>(a, acc, img, tr0, tc0, blk * PQ * 48 + 48 * pmq, nh, col, kq, PLg);
    else s3_epilogue<RW, ST>(a, acc, img, a.ring + tr0, a.ringw + tc0, blk * PQ * 48 + 48 * pmq, nh, col, kq, PLg);
}
