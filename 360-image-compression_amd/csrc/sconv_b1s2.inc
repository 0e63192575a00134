// sconv_b1s2.inc -- the single-pass bf16 ("bf16x1") form of the 3x3 STRIDE-2 sphere convolution (csrc/conv3x3_kernels.hip, "Stride 2"; kernels
// k_sconv_b1s2<NQ, RW, 3>), opt-in (lic360_models.set_conv_precision(.., stride2="bf16x1")).  The contract is the stride-1 single-pass form's
// (sconv_bf16x3.inc): every input value and every weight rounded once to bf16 (nearest even), one v_mfma_f32_16x16x32_bf16 per product, fp32
// accumulation, bias / PReLU / residual in fp32 in the shared epilogue.  The 1x1 stride-2 form is b3_body<.., 1, 1, 2> (the loader fetches the even / even
// cells only: the stride-1 1x1 image, reads and waits); this file is the 3x3, whose LDS arithmetic leaves no room for b3_body's fp32 staging:
//   halo      a 16 x 16 tile of outputs reads 33 x 33 = 1089 cells per channel; a chunk is 32 channels (the K of one MFMA)
//   image     hi-only bf16, [kq < 4][1089 cells] x 16 bytes = 69 696 bytes
//   staging   32 channels x 1089 x 4 bytes = 139 392 bytes of fp32: with the image past the 160 KiB of a CU
// The loader therefore goes through REGISTERS: a cell task (kq, cell) is the 8 channels 8 kq .. 8 kq + 7 of one halo cell; a lane fetches them with 8 plain
// global loads at the sphere-rule offset (s3_cell_offset<.., 3, 2>; consecutive lanes take consecutive cells, so each load is as coalesced as the fp32 form's
// per-lane DMA), rounds them and writes ONE 16-byte cell of a DOUBLE-BUFFERED bf16 image: 2 x 69 696 = 139 392 bytes, no staging, no conversion pass, one
// barrier per chunk.  4 x 1089 tasks over 512 lanes are 9 rounds, and a chunk has 9 K steps (kw, kh): one round per step, one chunk ahead.
//   in flight a round's loads are issued 2 steps before its cell is written (two sets, 16 registers), a step's A operands 1 step before their MFMAs (two
//             sets, 24 registers, as in b3_body; the chunk's parity makes every set index static).  A step issues A(step + 1) and then X(round + 2), so at the
//             top of a step the only loads younger than what it needs are one round's 8: one counted wait, vmcnt(8), per step and nothing else.  (Three rounds
//             and two operand steps in flight -- 60 registers -- spill at 192 output channels: 96 accumulators.)
//   banks     B operand = ds_read_b128 at a column stride of TWO cells; plane pitch 1089 cells = 1 (mod 16) slots of 16 bytes.  ds_read_b128 is served in four
//             16-lane groups, {0-3, 12-15, 20-27} first: lanes 0-3, 12-15 (kq 0, columns 0-3, 12-15) take slots 0 2 4 6 8 10 12 14, lanes 20-27 (kq 1, columns
//             4-11) slots 1 + {8 .. 14, 0 .. 6}: all sixteen slots once.  The other three groups likewise (kq 2, 3: pitch offsets 2, 3): conflict-free.
//             The loader's ds_write_b128 (8 consecutive lanes, consecutive cells) covers the 32 store banks once.
// The weight pack is the stride-1 single-pass pack (k_sconv_b3_pack, nhl = 1), read in its K-step order (cg, kw, kh).  No LDS-DMA here, M0 is not written.

constexpr int B1S2_XR = 2 * S3_T + 1, B1S2_NCELL = B1S2_XR * B1S2_XR, B1S2_PS = B1S2_NCELL | 1;   // 33 x 33 halo cells, odd plane pitch (in 16-byte cells)
constexpr int b1s2_lds() { return 2 * 4 * B1S2_PS * 4; }                    // LDS floats: two images of 4 kq planes

template <int NQ, int RW>
__device__ __forceinline__ void b1s2_body(const S3Args &a, float *lds, int ty, int tx, int img) {
    constexpr int NR = 8 / NQ, TR = NR * RW, XC = B1S2_XR, NCELL = B1S2_NCELL, PS = B1S2_PS, NSTEP = 9;
    constexpr int NTASK = 4 * NCELL, NRND = (NTASK + B3_THREADS - 1) / B3_THREADS;
    static_assert(TR == S3_T, "a tile is 16 x 16 outputs");
    static_assert(NRND == NSTEP, "one loader round per K step");
    constexpr int XL = 8;                                                   // loads of a round: the channels of a kq plane
    static_assert(XL <= 63, "s_waitcnt vmcnt takes at most 63 on gfx950");   // (the largest immediate below: one round behind the operands a step needs)
    b3_u4 *sp = (b3_u4 *)lds;                                               // image b at sp + b * 4 * PS: [kq][PS]
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), mq = wave % NQ, nh = wave / NQ;
    const int tr0 = ty * S3_T, tc0 = tx * S3_T;                             // the tile's first output, interior coordinates of the output
    const int blk = blockIdx.y;
    const long PLg = (long)a.hp * a.wp;
    // task c = round * 512 + tid = kq plane c / NCELL, halo cell c % NCELL: s3_cell_offset with 4 "channels" of 8 planes each.  The pitch IS the cell count
    // (1089 is odd already), so task c writes image cell c.
    static_assert(PS == NCELL, "task index = image cell");
    unsigned voff[NRND];
#pragma unroll
    for (int r = 0; r < NRND; ++r) voff[r] = s3_cell_offset<4, NCELL, B1S2_XR, XC, 3, 2>(a, tr0, tc0, r * B3_THREADS + tid, 8 * PLg);
    const float *xb = a.x + (long)img * a.cin * PLg;
    const int nck = a.cin / B3_CK, niter = nck * NSTEP;
    // round r of chunk cn -> registers X_; a chunk past the last: every lane loads the map's first cell (the counted waits stay right, no traffic)
    auto load_x = [&](int cn, int r, float (&X_)[8]) __attribute__((always_inline)) {
        const bool real = cn < nck;
        const float *sb = s3_uniform(xb + (real ? (long)cn * B3_CK * PLg : 0L));
        const unsigned v = real ? voff[r] : 0u;
        asm volatile("global_load_dword %0, %8, %9\n\tglobal_load_dword %1, %8, %10\n\tglobal_load_dword %2, %8, %11\n\tglobal_load_dword %3, %8, %12\n\t"
                     "global_load_dword %4, %8, %13\n\tglobal_load_dword %5, %8, %14\n\tglobal_load_dword %6, %8, %15\n\tglobal_load_dword %7, %8, %16"
                     : "=&v"(X_[0]), "=&v"(X_[1]), "=&v"(X_[2]), "=&v"(X_[3]), "=&v"(X_[4]), "=&v"(X_[5]), "=&v"(X_[6]), "=&v"(X_[7])
                     : "v"(v), "s"(sb), "s"(sb + PLg), "s"(sb + 2 * PLg), "s"(sb + 3 * PLg), "s"(sb + 4 * PLg), "s"(sb + 5 * PLg), "s"(sb + 6 * PLg), "s"(sb + 7 * PLg));
    };
    auto store_x = [&](b3_u4 *im, int r, const float (&X_)[8]) __attribute__((always_inline)) {
        if ((r + 1) * B3_THREADS <= NTASK || r * B3_THREADS + tid < NTASK) im[r * B3_THREADS + tid] = b3_split(X_, false);
    };
    // A operands: the stride-1 single-pass pack, three 16-byte loads per lane and K step
    const char *wl = (const char *)a.w + (((long)blk * niter * NQ + mq) * 3 * 64 + lane) * 16;   // + it * NQ * 3 KiB per K step
    auto load_a = [&](int it, b3_u4 (&A_)[3]) __attribute__((always_inline)) {
        const char *p = wl + (long)(it < niter ? it : niter - 1) * (NQ * 3 * 1024);
        asm volatile("global_load_dwordx4 %0, %3, off\n\tglobal_load_dwordx4 %1, %3, off offset:1024\n\tglobal_load_dwordx4 %2, %3, off offset:2048"
                     : "=&v"(A_[0]), "=&v"(A_[1]), "=&v"(A_[2]) : "v"(p));
    };
#define B1S2_WAIT_X(N, X_)                                                                                                                         \
    asm volatile("s_waitcnt vmcnt(%8)" : "+v"(X_[0]), "+v"(X_[1]), "+v"(X_[2]), "+v"(X_[3]), "+v"(X_[4]), "+v"(X_[5]), "+v"(X_[6]), "+v"(X_[7]) : "n"(N))
#define B1S2_WAIT_AX(N, A_, X_)                                                                                                                    \
    asm volatile("s_waitcnt vmcnt(%11)" : "+v"(A_[0]), "+v"(A_[1]), "+v"(A_[2]), "+v"(X_[0]), "+v"(X_[1]), "+v"(X_[2]), "+v"(X_[3]), "+v"(X_[4]), \
                 "+v"(X_[5]), "+v"(X_[6]), "+v"(X_[7]) : "n"(N))
    s3_f4 acc[3][RW];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[m][r] = (s3_f4){0.f, 0.f, 0.f, 0.f};
    float X[2][8];                                                          // loader ring: round r of chunk c in set (9 c + r) & 1
    b3_u4 A[2][3];                                                          // operand ring: K step `it` in set it & 1
    // chunk 0, in the open: two rounds in flight
    load_x(0, 0, X[0]); load_x(0, 1, X[1]);
#pragma unroll
    for (int r = 0; r < NRND; ++r) {
        if (r + 1 < NRND) B1S2_WAIT_X(XL, X[r & 1]);
        else B1S2_WAIT_X(0, X[r & 1]);
        store_x(sp, r, X[r & 1]);
        if (r + 2 < NRND) load_x(0, r + 2, X[r & 1]);
    }
    // the steady state's order, as if steps -2 and -1 had run: X(0), A(0), X(1)
    load_x(1, 0, X[1]); load_a(0, A[0]); load_x(1, 1, X[0]);
    __syncthreads();
    // one chunk; P = ck & 1 makes the ring sets of every step static (NSTEP is odd)
    auto chunk = [&](int ck, auto par) __attribute__((always_inline)) {
        constexpr int P = decltype(par)::value;
        const b3_u4 *cur = sp + P * (4 * PS);
        b3_u4 *nxt = sp + (P ^ 1) * (4 * PS);                               // its last readers passed the barrier that ended chunk ck - 1
#pragma unroll
        for (int p = 0; p < NSTEP; ++p) {
            const int kw = p / 3, kh = p - 3 * kw, sa = (P + p) & 1, sx = sa ^ 1;
            B1S2_WAIT_AX(XL, A[sa], X[sx]);                                // this step's operands (issued one step ago) and round p of the next chunk (two); behind them X(p + 1)
            store_x(nxt, p, X[sx]);
            load_a(ck * NSTEP + p + 1, A[sa ^ 1]);
            load_x(p + 2 < NSTEP ? ck + 1 : ck + 2, (p + 2) % NSTEP, X[sx]);
            const b3_u4 *bl = cur + kq * PS + (2 * nh * RW + kh) * XC + 2 * col + kw;
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const b3_bf8 bh = __builtin_bit_cast(b3_bf8, bl[2 * r * XC]);
#pragma unroll
                for (int m = 0; m < 3; ++m) acc[m][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b3_bf8, A[sa][m]), bh, acc[m][r], 0, 0, 0);
            }
        }
        __syncthreads();                                                    // the next chunk's image is written; this chunk's is free
    };
    for (int ck = 0;; ck += 2) {                                            // (an odd chunk count leaves behind an even chunk: no path from one even chunk into another)
        chunk(ck, std::integral_constant<int, 0>{});
        if (ck + 1 >= nck) break;
        chunk(ck + 1, std::integral_constant<int, 1>{});
        if (ck + 2 >= nck) break;
    }
    // the loads issued ahead of steps and chunks that do not exist are still in flight INTO the rings: the drain names both operand sets and both loader sets,
    // so that they stay allocated until it (a register the compiler took for something else before the wait would be overwritten by a late return)
    B1S2_WAIT_AX(0, A[0], X[0]);
    B1S2_WAIT_AX(0, A[1], X[1]);
#undef B1S2_WAIT_X
#undef B1S2_WAIT_AX
    s3_epilogue<RW, 2>(a, acc, img, a.ring + tr0, a.ringw + tc0, blk * NQ * 48 + 48 * mq, nh, col, kq, PLg);
}
