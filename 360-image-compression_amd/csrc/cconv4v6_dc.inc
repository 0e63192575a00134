// cconv4v6_dc.inc -- decode-order leaf-resident conv (included by cconv4_kernels.hip; arithmetic and lane/class mapping: see its header).
//
// Persistent workgroups of 12 waves = 3 adjacent groups (adjacent anti-diagonals of the current plane) of one sample x 4 lane classes;
// one workgroup per CU walks the plane's (group block, sample) task list heaviest-first.  Activations live in a ZERO-PADDED
// diagonal-major layout [n][c][SP][HP], cell (s = th+tw, th) at row s + D3_S0, column th + D3_C0, SP = H+W-1 + 2*D3_S0 rows of
// HP = H + 2*D3_C0 floats; slots outside the image are never written and stay zero, so the halo band of a task is fetched
// UNCONDITIONALLY (no per-cell bounds logic) and the output stores of a diagonal are contiguous.
// The generation before this one (LDS-DMA staging, one ds_read per tap; git show c0e481c) was bound
// by the LDS pipe, not by MFMA (335 ns of 4x4x1 MFMAs per CU-step vs 424 ns of ds_read_b32, 150 ns of staging writes and 190 ns of
// VMEM return, all serialised).  Hence:
//   * ONE ds_read_b32 PER TAP DIAGONAL instead of one per tap.  In the diagonal-major tile the taps with kh+kw = d read
//     the same LDS row of the same input channel (tap = 4*kh + d, so (class - tap) & 3 is constant on a diagonal) at
//     column offsets kh = 0..4.  Lanes are ABSOLUTE image rows (lane = th, H <= 64): all taps of a diagonal multiply
//     the ONE operand register read at the diagonal's centre-most tap, and it is the ACCUMULATOR of tap kh that is
//     lane-shifted (lane l = position l - (kh - k0)); what falls off the wave are products with rows outside the image,
//     exact zeros.  The shifts are undone once per task with `v_mov_b32_dpp wave_shl/shr:1 bound_ctrl:1` (conv6_align).
//     9 LDS reads and no other VALU work per wave and step instead of 27 reads (tools/coexec_probe: a DPP move costs as
//     much VALU time as a 4x4x1 MFMA, so shifting operands per tap was measured slower than this).
//   * the band of a task is 11 FULL rows of the padded layout (68 columns = H + 4), i.e. contiguous memory per channel.
//   * weights never touch LDS: each wave loads its two weight registers (16 leaves x 4 rows each, selected with
//     abid) straight from the packed array, in a register ring of their own.
//   * REGISTER-staged prefetch ring instead of LDS-DMA (DMA writes cost ~30 LDS cycles per KB, ds_write_b128 ~13):
//     thread t owns quad t of the step's 748-quad band; 4 register sets; the loads of step i+5 are issued while step i
//     computes, the quad of step i+1 is written to the other half of an LDS double buffer; one barrier per step; the
//     step loop is unrolled by 4 so the ring index is static and hipcc's own vmcnt counting stays exact.  For that the
//     ring loads must be unconditional and the loop must have a single exit at its bottom -- a load under a branch or
//     a mid-loop break makes the waitcnt pass fall back to vmcnt(0).  Loads use scalar base + 32-bit lane offset, so a
//     step costs no vector address arithmetic: with 4x4x1 MFMAs the VALU does not co-issue (SQ_VALU_MFMA_COEXEC_CYCLES
//     = 0), every other VALU instruction is time taken from the matrix pipe.
// H <= 64: lane = image row.  Taller images are cut into 64-row windows (SEG, see dc6_body).
// D6_GRID (workgroups per launch: one per CU) is stated in need.h, where the list builder's placement pass reads it too
#define D6_TAPE_BLOCKS 16                            // group blocks of a taped launch (ngroup <= 48)
#define D6_TAPE_WAVES 6                              // waves per tape (tape_c <= 6 samples)
#define D3_S0 (4 + C4_PS - 1)                         // zero rows before diagonal 0 (and after the last)
#define D3_C0 2                                      // zero columns before th = 0 (and after th = H-1)
#define D3_SP(h, w) ((h) + (w) - 1 + 2 * D3_S0)
#define D3_HP(h) ((h) + 2 * D3_C0)
struct Dc3Args {
    const float *x, *packed, *bias, *act, *residual;
    float *out;
    int ngroup, cout, hidden, H, W, npb, x_mod, N, psum, n_gb, n_gbv, nseg, pack0, gstep;   // pack0: tall images, see PACK below
    int wblk;                                  // `packed` = the quad-packed weights, wblk 4 KB blocks per output group
    int nprod;                                 // task records produced before the first barrier (the issue side's lead in tasks + 2, at most 6)
    // TAPE packing (round 5; throughput mode, H <= 64, 8 | samples per net): the row windows of `tape_c` consecutive samples of an XCD's list (one net)
    // are laid end to end over the lanes of nw(j) waves (tasks) per group block j -- a window may be cut between two waves -- instead of one window per
    // task.  A piece: sample k of the tape stores rows slo..shi in lanes a0.., word k | slo << 3 | shi << 9 | a0 << 15 | 1 << 21 (0 = none), (a0 - slo) % 4
    // == 0, the column ranges (a0 .. a0 + rows + 3) of neighbouring pieces in different quads (dc6_wave_pieces).  The launch carries only where each wave
    // STARTS (the rule that lays out a wave is run again by the kernel's producer wave): kernel arguments of 1.8 KB (all pieces spelled out) cost 4.6 %
    // of the three-stream step whether or not the kernel read them.
    int tape_c, tape_n, tape_total;            // samples per tape; tapes per XCD list (N / 8 / tape_c); tasks per XCD list (sum over the blocks of tape_n * nw(j))
    unsigned tape_magic;                       // ceil(2^32 / tape_n): task index inside a block -> (wave of the tape, tape) without a division
    unsigned tape_nw4[2];                      // nw(j): 4 bits each (the kernel keeps the two words in scalar registers)
};
// What a launch actually carries: Dc3Args packed into 96 bytes (+ 64 bytes of Dc3Tape for a taped launch, which has kernels of its own).  The size of the
// kernel arguments is not free on this machine: the same kernels with their argument struct padded from 128 to 144 / 272 bytes ran the three-stream
// 1024x2048 configuration 2.8 / 6.2 % slower (2 518 -> 2 590 -> 2 674 ms; 64 images in sub-batches of 22: +2.4 % at 272 bytes; the headline +0.6 %), and
// 1.8 KB of spelled-out tape pieces cost the headline 4.6 % whether or not the kernel read them (profiles/r05_dc6_micro_variants.txt).  Isolated launches
// do not show it.  (A struct with a dynamically indexed array inside also stays in argument memory as a whole: every use of a pointer or a shape in the
// task set-up became a scalar load -- 66 s_load instead of 13 -- hence the separate Dc3Tape argument.)
struct Dc3Packed {
    const float *x, *packed, *bias, *act, *residual;
    float *out;
    unsigned w0;                               // ngroup | cout << 7 | hidden << 10 | gstep << 11 | nseg << 13 | pack0 << 17 | nprod << 18 | tape_c << 21
    unsigned hw;                               // H | W << 16
    int npb, x_mod, N;
    unsigned pg;                               // psum | n_gb << 16 | n_gbv << 24
    int wblk, tape_n, tape_total;
    unsigned tape_magic, tape_nw4[2];
};
static_assert(sizeof(Dc3Packed) == 96, "kernel arguments of the decode-order kernel");
// where the waves of a tape start: per group block, 9 bits (k | slo << 3: the wave's first piece) for waves 1, 3, 5 at bits 0, 9, 18; wave 0 starts the
// tape at (0, lo), an even wave where the rule leaves its predecessor (dc6_wave_start)
struct Dc3Tape { unsigned s[D6_TAPE_BLOCKS]; };
static Dc3Packed dc6_pack(const Dc3Args &a) {
    Dc3Packed p;
    p.x = a.x; p.packed = a.packed; p.bias = a.bias; p.act = a.act; p.residual = a.residual; p.out = a.out;
    p.w0 = (unsigned)a.ngroup | (unsigned)a.cout << 7 | (unsigned)a.hidden << 10 | (unsigned)a.gstep << 11 | (unsigned)a.nseg << 13 | (unsigned)a.pack0 << 17 |
           (unsigned)a.nprod << 18 | (unsigned)a.tape_c << 21;
    p.hw = (unsigned)a.H | (unsigned)a.W << 16;
    p.npb = a.npb; p.x_mod = a.x_mod; p.N = a.N;
    p.pg = (unsigned)a.psum | (unsigned)a.n_gb << 16 | (unsigned)a.n_gbv << 24;
    p.wblk = a.wblk; p.tape_n = a.tape_n; p.tape_total = a.tape_total; p.tape_magic = a.tape_magic; p.tape_nw4[0] = a.tape_nw4[0]; p.tape_nw4[1] = a.tape_nw4[1];
    return p;
}
__device__ __forceinline__ Dc3Args dc6_unpack(const Dc3Packed &p) {
    Dc3Args a;
    a.x = p.x; a.packed = p.packed; a.bias = p.bias; a.act = p.act; a.residual = p.residual; a.out = p.out;
    a.ngroup = p.w0 & 127; a.cout = (p.w0 >> 7) & 7; a.hidden = (p.w0 >> 10) & 1; a.gstep = (p.w0 >> 11) & 3; a.nseg = (p.w0 >> 13) & 15; a.pack0 = (p.w0 >> 17) & 1;
    a.nprod = (p.w0 >> 18) & 7; a.tape_c = (p.w0 >> 21) & 7;
    a.H = p.hw & 0xffff; a.W = p.hw >> 16;
    a.npb = p.npb; a.x_mod = p.x_mod; a.N = p.N;
    a.psum = p.pg & 0xffff; a.n_gb = (p.pg >> 16) & 255; a.n_gbv = p.pg >> 24;
    a.wblk = p.wblk; a.tape_n = p.tape_n; a.tape_total = p.tape_total; a.tape_magic = p.tape_magic; a.tape_nw4[0] = p.tape_nw4[0]; a.tape_nw4[1] = p.tape_nw4[1];
    return a;
}

// The pieces of ONE wave of a tape (host: dc6_build_tape; device: the producer wave's decode()): from the wave's first piece (sample k of the tape, first
// row slo) lay pieces end to end until the wave is full, three are placed or the tape ends.  lo..hi: the rows of the block's diagonals, h: image rows,
// c: samples per tape.  Rules: (a0 - slo) % 4 == 0 (the band quads a lane reads stay 16-byte aligned behind the per-quad sample offset); the next piece's
// columns start in the quad behind this piece's last column (lane + 4); a stored lane takes shifted partial sums from the lanes two below and two above
// it, which must exist in the wave unless what they would hold are products with rows outside the image (a0 >= 2 unless slo == 0; last lane <= 61 unless
// the piece ends with the image).  Returns the number of pieces; (k, slo) advance to the start of the next wave (k == c: the tape is complete).
__host__ __device__ __forceinline__ int dc6_wave_pieces(int lo, int hi, int h, int c, int &k, int &slo, unsigned out[3]) {
    int nwin = 0, pos = 0;
    out[0] = out[1] = out[2] = 0u;
    while (nwin < 3 && k < c) {
        int a0 = pos;
        if (slo != 0 && a0 < 2) a0 = 2;
        a0 += (slo - a0) & 3;
        const int top = hi == h - 1 ? 63 : 61;
        int shi = hi;
        if (a0 + (hi - slo) > top) shi = slo + (61 - a0);               // cut
        if (a0 > 61 || (shi < hi && (a0 > 57 || shi - slo + 1 < 4))) break;   // no room (for a useful piece of a cut window)
        out[nwin++] = (unsigned)k | (unsigned)slo << 3 | (unsigned)shi << 9 | (unsigned)a0 << 15 | 1u << 21;
        pos = ((a0 + (shi - slo) + 4) / 4 + 1) * 4;
        slo = shi + 1;
        if (slo > hi) { slo = lo; ++k; }
    }
    return nwin;
}
// (k, slo) of the first piece of wave wv of a tape, from the block's word of Dc3Tape
__host__ __device__ __forceinline__ void dc6_wave_start(unsigned word, int lo, int hi, int h, int c, int wv, int &k, int &slo) {
    k = 0; slo = lo;
    if (wv == 0) return;
    const unsigned st = (word >> (9 * ((wv - 1) >> 1))) & 511u;       // the odd wave at or before wv
    k = st & 7; slo = st >> 3;
    if (!(wv & 1)) {                                                    // even: one wave further (wave 2 from wave 1, wave 4 from wave 3)
        unsigned pc[3];
        dc6_wave_pieces(lo, hi, h, c, k, slo, pc);
    }
}
#ifndef D6_STAGE_AT_END
#define D6_STAGE_AT_END 1                            // see D6_STAGE_MID / D6_STAGE_END
#endif
#ifndef D6_NB
#define D6_NB 2                                      // double steps per workgroup barrier (LDS: 2 * D6_NB double-step buffers of 24 KB)
#endif
#define D6_COLS 68                                   // 64 positions + 4 tap columns
#define D6_QPR (D6_COLS / 4)
#define D6_ROWS (9 + C4_PS - 1)
#define D6_XQ(CIN) (4 * D6_ROWS * D6_QPR)              // 16-byte quads of x per staged step: 4 channel planes (cin = 4: one input group, cin = 1: four)
#define D6_XFL(CIN) (D6_XQ(CIN) * 4)

#define DPP_WAVE_SHL1 0x130
#define DPP_WAVE_SHR1 0x138
__device__ __forceinline__ float dpp_shl1(float v) {                       // out[l] = v[l+1], out[63] = 0
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), DPP_WAVE_SHL1, 0xf, 0xf, true));
}
__device__ __forceinline__ float dpp_shr1(float v) {                       // out[l] = v[l-1], out[0] = 0
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), DPP_WAVE_SHR1, 0xf, 0xf, true));
}

// one K step of lane class CLS, in two halves.  xl = tile origin of this wave + lane.
// conv6_load: the 9 (cin = 4) or 2-3 (cin = 1) operand reads of the step, one per tap diagonal, all issued up front
template <int CIN, int CLS, int XPLANE>
__device__ __forceinline__ void conv6_load(float *r0, const float *xl) {
    static_for<9>([&](auto dd) {
        constexpr int d = decltype(dd)::value, gid = CIN == 4 ? ((CLS - d) & 3) : 0, kmin = d > 4 ? d - 4 : 0, kmax = d < 4 ? d : 4;
        constexpr int k0 = kmax < 2 ? kmax : (kmin > 2 ? kmin : 2);         // the tap nearest to the centre column
        if constexpr (CIN == 4 || (d & 3) == CLS) r0[d] = xl[gid * XPLANE + d * D6_COLS + k0];
    });
}
// conv6_diags: the MFMAs of tap diagonals D_LO..D_HI.  EVERY tap of a diagonal multiplies the same operand register (the
// one read at the diagonal's centre-most tap k0), so the accumulator of tap kh holds, in lane l, the partial sum of the
// position l - (kh - k0): accumulators are lane-shifted instead of operands, which costs nothing per step (a DPP move per
// tap would cost as much VALU time as the MFMA it feeds).  The terms that fall off the ends of the wave are products
// with rows outside the image, i.e. exact zeros.  conv6_align undoes the shifts once per task.
template <int CIN, int CLS, int D_LO, int D_HI>
__device__ __forceinline__ void conv6_diags(f32x4 *acc, const float *r0, float w0, float w1) {
    static_for<9>([&](auto dd) {
        constexpr int d = decltype(dd)::value, kmin = d > 4 ? d - 4 : 0, kmax = d < 4 ? d : 4;
        if constexpr (d >= D_LO && d <= D_HI && (CIN == 4 || (d & 3) == CLS)) {
            static_for<kmax - kmin + 1>([&](auto kk) {
                constexpr int kh = kmin + decltype(kk)::value, tap = 5 * kh + (d - kh), i = CIN == 4 ? tap : (tap - CLS) / 4;
                acc[i] = mfma4<i % 16>(i < 16 ? w0 : w1, r0[d], acc[i]);
            });
        }
    });
    __builtin_amdgcn_sched_barrier(0);
}
// conv6_align: lane l of every accumulator <- the partial sum of position l (wave shifts with zero fill)
template <int CIN, int CLS>
__device__ __forceinline__ void conv6_align(f32x4 *acc) {
    static_for<9>([&](auto dd) {
        constexpr int d = decltype(dd)::value, kmin = d > 4 ? d - 4 : 0, kmax = d < 4 ? d : 4;
        constexpr int k0 = kmax < 2 ? kmax : (kmin > 2 ? kmin : 2);
        if constexpr (CIN == 4 || (d & 3) == CLS) {
            static_for<kmax - kmin + 1>([&](auto kk) {
                constexpr int kh = kmin + decltype(kk)::value, tap = 5 * kh + (d - kh), i = CIN == 4 ? tap : (tap - CLS) / 4, sh = kh - k0;
                static_for<(sh > 0 ? sh : -sh)>([&](auto) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][r] = sh > 0 ? dpp_shl1(acc[i][r]) : dpp_shr1(acc[i][r]);
                });
            });
        }
    });
}

struct W8 {
    float a0, a1, a2, a3, b0, b1, b2, b3;
    template <int H, int J> __device__ __forceinline__ float get() const {
        if constexpr (H == 0) return J == 0 ? a0 : (J == 1 ? a1 : (J == 2 ? a2 : a3));
        else return J == 0 ? b0 : (J == 1 ? b1 : (J == 2 ? b2 : b3));
    }
};

// SEG: images taller than one wave (H > 64) are cut into row segments.  Segment k is a window of 64 consecutive rows
// starting at row rb = 60k (lane = row - rb) whose valid output rows are lanes 2..61 (lanes 0..61 for k = 0): every
// accumulator shift (|shift| <= 2) then stays inside the wave, and the only terms that fall off are still products with
// rows outside the image (first segment, and the last one where it ends with the image).
#define D6_SEG_STEP 60
#define D6_NSEG(h) ((h) <= 64 ? 1 : 1 + ((h) - 62 + D6_SEG_STEP - 1) / D6_SEG_STEP)
// rows of a piece word (need.h): six bits each, and a seventh at bits 25 / 26 on latents taller than a wave (TALL)
template <bool TALL> __device__ __forceinline__ int dc6_piece_slo(unsigned wd) { if constexpr (TALL) return dcl_piece_slo(wd); else return (wd >> 3) & 63; }
template <bool TALL> __device__ __forceinline__ int dc6_piece_shi(unsigned wd) { if constexpr (TALL) return dcl_piece_shi(wd); else return (wd >> 9) & 63; }
#ifdef DC6_STAMP
// diagnostic build only (tools/dc6_stamp.sh): cycles per phase of the decode-order hidden-layer instantiation, summed per wave over the launches
__device__ unsigned long long dc6_stamps[256 * 12 * 10];
#ifndef DC6_STAMP_CIN
#define DC6_STAMP_CIN 4                                // which instantiation is stamped: 4 = hidden / last layers, 1 = first layer
#endif
#define DC6_T(i) do { if constexpr (CIN == DC6_STAMP_CIN && !SEG) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); st[i] += t_ - t0; t0 = t_; } } while (0)
LIC360_API int lic360_dc6_stamps(unsigned long long *host_out, int clear) {
    if (host_out) HIP_TRY(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(dc6_stamps), sizeof(dc6_stamps)));
    if (clear) { static unsigned long long z[256 * 12 * 10]; HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(dc6_stamps), z, sizeof(z))); }
    return 0;
}
#else
#define DC6_T(i)
#endif
// LIST (round 6, need.h): the tasks of the launch come from a device-built list of records per XCD (lic360_dc_lists_build: the dead-cone skip -- every
// sample's row window trimmed to the rows some coded symbol can observe, the windows packed like a tape's) instead of being derived from the plane's
// geometry.  list: [8][a.tape_total] records, lcnt: [8] counts.  A LIST kernel is a TAPE kernel whose producer wave reads its records.
// NETS = 3 (first layer, cin = 1; throughput mode, H <= 64): the three stacked nets read the SAME input, so one task = (group block, image or tape of
// images) carries all three: the band is fetched, staged and read from LDS once, the MFMAs, the tree and the epilogue run once per net, on that net's
// accumulators (3 x 7) with that net's weights.  The launch then counts IMAGES: a.N = a.npb = a.x_mod = images, net k's weights / bias / slopes lie k nets
// behind net 0's, its outputs k * a.npb samples behind.  Per accumulator the arithmetic is the one-net kernel's, in the same order.
// TALL (LIST only; latents of 65..128 rows): the list's pieces carry seven-bit rows (need.h: dcl_piece) and every record is packed.  Nothing else differs
// from the list kernel of the short latents: a piece already sits at a lane of its own (a0) and fetches the 68-column window of the padded rows that
// starts at its own row base (band column c <- padded column slo + c - a0), and HP = H + 4 = 132 is only the row pitch of that fetch.
// The shifts.  A stored lane li of a piece (a0 <= li <= a0 + shi - slo) takes the partial sum of tap kh from source lane li + sh, sh = kh - k0 in
// [-2, 2], which read band column li + sh + k0 with -sh <= k0 <= 4 - sh: columns li .. li + 4, all inside the piece's own a0 .. a0 + rows + 3, which
// issue_setup fetches from the piece's own sample whole -- the two rows on either side of a cut included (the next wave's piece fetches them again).
// The source lane itself must exist in the wave: a0 >= 2 unless the piece starts with image row 0, last lane <= 61 unless it ends with row H - 1 (what
// would come from lanes -2, -1, 64, 65 there are products with the zero rows around the image).  A piece cut in mid-image has real rows on both sides
// and therefore always keeps lanes 0, 1 / 62, 63 free: dcl_wave_pieces cuts at lane 61 and restarts at lane 2 whatever the image's height.
template <int CIN, int CLS, bool SEG, bool LAT = false, bool TAPE = false, bool LIST = false, int NETS = 1, bool TALL = false>
__device__ __forceinline__ void dc6_body(const Dc3Args &a, const Dc3Tape *tape, const uint4 *__restrict__ list, const int *__restrict__ lcnt, float *xs, float *comb,
                                         int (*trec)[16], int tid, int lane, int ps) {
    static_assert(!LIST || (TAPE && !SEG && !LAT), "list launches are throughput-mode launches whose lanes are placed by their records, not by row segments");
    static_assert(!TALL || (LIST && CIN == 4 && NETS == 1), "seven-bit rows: the list kernel of the hidden / last layers");
    static_assert(NETS == 1 || (NETS == 3 && CIN == 1 && !SEG && !LAT && !LIST), "three nets per task: the first layer in throughput mode");
    constexpr int NA = NAcc<CIN>::value;
    constexpr int XQ = D6_XQ(CIN), XFL = D6_XFL(CIN);
    static_assert(XQ <= C4_THREADS, "one quad slot per thread");
    constexpr int XPLANE = D6_ROWS * D6_COLS;
    const int H = a.H, W = a.W, G = a.ngroup, S = H + W - 1, HP = D3_HP(H);
    // groups per task: C4_PS, or 1 in latency mode (few samples: one group per workgroup, the wave sets ps > 0 idle through the
    // barriers, so a step costs one wave's MFMAs per SIMD instead of three and three times as many CUs work)
    const int gs = a.gstep;
    constexpr int TCS = CIN == 1 ? 4 : 1;                                // input groups per staged step (always 4 channel planes)
    const long SKP = (long)D3_SP(H, W) * HP, tcs = 4 * SKP;
    f32x4 acc[NETS * NA];
#ifdef DC6_STAMP
    unsigned long long st[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, t0 = __builtin_amdgcn_s_memtime();
    const unsigned long long t_entry = t0;
#endif
    // ---- task list of this workgroup: XCD-aware static walk, heaviest group blocks first (see cconv4v3_dc.inc).
    // A task = 3 groups g0..g0+2 on the staggered diagonals s0, s0-1, s0-2 of one sample; decode order has one s0 per
    // group block (s0 = psum - g0).
    // (latency mode walks ONE list over the whole grid instead: with 3 samples the per-XCD lists would leave five XCDs idle)
    const bool flat = gs == 1;
    const int xcd = flat ? 0 : blockIdx.x & 7, xstep = flat ? 1 : 8, wg_in_xcd = flat ? blockIdx.x : blockIdx.x >> 3;
    // (the grid is a constant of the launcher: reading gridDim / blockDim would make the kernel carry the 256 bytes of HIP's implicit arguments in every
    //  launch on top of its own 96 -- see Dc3Packed for what argument bytes cost)
    const int wgs_per_xcd = flat ? D6_GRID : (D6_GRID - xcd + 7) >> 3;
    // the k-th task of a workgroup: boustrophedon order (round k forwards, round k+1 backwards), so a workgroup alternates
    // between long (late group blocks) and short tasks: the static walk balances to ~1% (plain round-robin: 11%)
    auto nth_task = [&](int k) __attribute__((always_inline)) { return k * wgs_per_xcd + ((k & 1) ? wgs_per_xcd - 1 - wg_in_xcd : wg_in_xcd); };
    const int ns_x = flat ? a.N : (a.N - xcd + 7) >> 3;
    // Task order.  Decode order: group block major (heaviest first), sample minor -- with the boustrophedon walk below the
    // static schedule balances to ~1% (sample-major order was measured: 15% less HBM traffic but 3% slower).  LIST launches take whatever order
    // their builder emitted (need.h: grouped emission and the placement pass, LIC360_DC_ORDER; DESIGN 4.6 "List order").
    const int nseg = SEG ? a.nseg : 1;
    // Packing several samples into the 64 lanes of a task: lane l always reads LDS column l + k0, so all that changes is which sample's band columns
    // sit where in LDS and which (sample, row) a lane stores.  H <= 64: TAPE packing (Dc3Args, launch_cconv4v6_dc; rounds 1-4 packed two / three
    // EQUAL windows per task on the corner diagonals only -- the tape subsumes that).  SEG (taller images): the LAST row segment, when it holds at
    // most 26 rows (rows 122..127 of the 128-row latents of 1024x2048 ERPs), takes TWO samples per task -- sample A in lanes 0..27, sample B in lanes
    // 36..63, both on the row window H-28.., their 32-column band windows side by side in LDS (quads 0..7 and 9..16 of a band row) (a.pack0 != 0).
    // What a STORED lane's partial sums read stays inside its own window: a source lane li + sh (|sh| <= 2) reads column li + sh + k0 with
    // -sh <= k0 <= 4 - sh, i.e. columns li .. li + 4.
    constexpr bool PACK = true;
    const bool pack_last = PACK && SEG && a.pack0 != 0;
    const int per_j = SEG ? ns_x * (nseg - 1) + (pack_last ? (ns_x + 1) >> 1 : ns_x) : 0;   // tasks per group block, SEG
    const int tape_c = TAPE ? a.tape_c : 0;                             // > 0: tape packing (host: gs == C4_PS, ns_x % tape_c == 0 on every XCD)
    const unsigned nw4[2] = {a.tape_nw4[0], a.tape_nw4[1]};
    auto blk_tasks = [&](int j) __attribute__((always_inline)) {
        return tape_c ? a.tape_n * (int)((nw4[(j >> 3) & 1] >> ((j & 7) * 4)) & 15u) : ns_x;
    };
    // LIST: lane i of the PRODUCER wave holds the record of the workgroup's i-th task (one 16-byte load per lane, issued together with the list's
    // count at the top of the kernel: one memory round trip before the first task instead of one per record -- a first version that loaded each
    // record where it was decoded cost the hidden layer 10 % per launch); produce() then reads a record with four v_readlane.  Tasks past the
    // 64th of a workgroup (batches of several hundred images) load theirs directly.
    uint4 lrec = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (LIST) {
        if (CLS == 0 && ps == 0) {
            int u = nth_task(lane);
            if (u > a.tape_total - 1) u = a.tape_total - 1;                 // (inside the list's room; whether the record exists is decided against n_my)
            lrec = list[(long)xcd * a.tape_total + u];
        }
    }
    int n_my_ = 0;
    if constexpr (LIST) n_my_ = __builtin_amdgcn_readfirstlane(lcnt[xcd]);
    else if constexpr (SEG) n_my_ = per_j * a.n_gbv;
    else if (tape_c) n_my_ = a.tape_total;
    else n_my_ = ns_x * a.n_gbv;
    const int n_my = n_my_;
    int pk = -1, pq = 0;                                                // producer state (wave 0 only): task sequence number, ring slot
    // -> first group g0, sample n (and nb = the second sample of a packed task, or -1), first diagonal s0, segment,
    //    prb = row of lane 0 (packed tasks), packed = 0: one sample, 2: two samples of a tall image's last segment, 4: a tape task (seg / nb2 / prb = its pieces)
    auto decode = [&](int u, int &g0, int &n, int &s0, int &seg, int &nb2, int &prb, int &packed) __attribute__((always_inline)) {
        nb2 = -1; prb = 0; packed = 0;
        if constexpr (LIST) {
            uint4 r;                                                        // x: g0 | packed << 7 | n << 10; y, z, w: the pieces of a packed record
            if (pk < 64) {                                                  // (pk: the producer's task sequence number, see produce())
                r.x = (unsigned)__builtin_amdgcn_readlane((int)lrec.x, pk); r.y = (unsigned)__builtin_amdgcn_readlane((int)lrec.y, pk);
                r.z = (unsigned)__builtin_amdgcn_readlane((int)lrec.z, pk); r.w = (unsigned)__builtin_amdgcn_readlane((int)lrec.w, pk);
            } else r = list[(long)xcd * a.tape_total + u];
            g0 = (int)(r.x & 127u);
            n = (int)(r.x >> 10);
            s0 = a.psum - g0;
            seg = 0;
            if ((r.x >> 7) & 7u) { seg = (int)(r.y & (TALL ? 0xfe3fffffu : 0x3fffffu)); nb2 = (int)r.z; prb = (int)r.w; packed = 4; }   // (without the live-group bits)
            packed |= (int)((r.y >> 22) & 7u) << 4;                         // bits 4..6: which of the block's three groups are live somewhere in the record's rows
        } else if constexpr (!SEG) {
            int j = 0, rem = u;
            for (; j < a.n_gbv - 1 && rem >= blk_tasks(j); ++j) rem -= blk_tasks(j);
            g0 = (a.n_gb - 1 - j) * gs;
            s0 = a.psum - g0;
            seg = 0;
            if (tape_c && (int)((nw4[(j >> 3) & 1] >> ((j & 7) * 4)) & 15u) < tape_c) {   // (a block whose tapes need a wave per sample anyway keeps plain tasks: they are cheaper to set up)
                // record: n = first sample of the tape, seg / nb2 / prb = its (up to) three windows
                const int wv = a.tape_n == 1 ? rem : (int)__umulhi((unsigned)rem, a.tape_magic), tp = rem - wv * a.tape_n;   // wave-major inside a block: rem = wv * tape_n + tp
                n = xcd + 8 * tp * tape_c;
                int lo = 1 << 30, hi = -1;                                  // rows of the block's diagonals (as the host)
#pragma unroll
                for (int q = 0; q < C4_PS; ++q) {
                    const int sq = s0 - q, l = sq >= W ? sq - W + 1 : 0, h2 = sq < H ? sq : H - 1;
                    if (g0 + q < G && sq >= 0 && sq < S) { lo = l < lo ? l : lo; hi = h2 > hi ? h2 : hi; }
                }
                int k, slo;
                dc6_wave_start(tape->s[j & (D6_TAPE_BLOCKS - 1)], lo, hi, H, tape_c, wv, k, slo);
                unsigned pc[3];
                dc6_wave_pieces(lo, hi, H, tape_c, k, slo, pc);
                seg = (int)pc[0]; nb2 = (int)pc[1]; prb = (int)pc[2];
                packed = 4;
            } else n = xcd + xstep * rem;
        } else {
            const int j = u / per_j, rem = u - j * per_j;
            g0 = (a.n_gb - 1 - j) * gs;
            s0 = a.psum - g0;
            if (pack_last && rem >= ns_x * (nseg - 1)) {                       // two samples of the last segment per task
                seg = nseg - 1;
                n = xcd + 16 * (rem - ns_x * (nseg - 1));
                nb2 = n + 8;
                prb = H - 28;
                packed = 2;
            } else {
                seg = rem / ns_x;
                n = xcd + xstep * (rem - seg * ns_x);
            }
        }
    };
    // rows a segment may store: [seg_lo(k), seg_hi(k)] (absolute image rows)
    auto seg_lo = [&](int k) __attribute__((always_inline)) { return k == 0 ? 0 : D6_SEG_STEP * k + 2; };
    auto seg_hi = [&](int k) __attribute__((always_inline)) { const int h = D6_SEG_STEP * k + 61; return SEG ? (h < H - 1 ? h : H - 1) : H - 1; };
    // decode order: does any of the task's three diagonals have a row inside the segment?  (both cursors skip dead tasks)
    auto task_live = [&](int u) __attribute__((always_inline)) {
        if constexpr (!SEG) return true;
        int g0, n, s0, seg, nb2, prb, packed;
        decode(u, g0, n, s0, seg, nb2, prb, packed);
        bool live = false;
#pragma unroll
        for (int q = 0; q < gs; ++q) {
            const int sq = s0 - q, lo = sq >= W ? sq - W + 1 : 0, hi = sq < H ? sq : H - 1;
            live = live || (g0 + q < G && sq >= 0 && sq < S && (lo > seg_lo(seg) ? lo : seg_lo(seg)) <= (hi < seg_hi(seg) ? hi : seg_hi(seg)));
        }
        return live;
    };
    auto next_task = [&](int &k) __attribute__((always_inline)) {
        int u;
        do { u = nth_task(++k); } while (u < n_my && !task_live(u));
        return u;
    };
    auto steps_of = [&](int g0) __attribute__((always_inline)) { int l = g0 + (gs - 1) + 4 + a.hidden; return l > G ? G : l; };
    // Task records: ONE wave (class 0, position set 0) walks the task list and decodes it -- the divisions, the block search
    // of the packed schedule, the liveness tests -- into a ring of 8 LDS records, 6 tasks ahead of the compute side; the
    // twelve waves' two cursors (issue and compute) then just read record q.  (All waves used to run the identical ~300
    // scalar instructions per task and cursor through the CU's one scalar unit.)
    //   record: 0 valid, 1 g0, 2 n, 3 s0, 4 seg, 5 nb2, 6 prb, 7 packed
    auto produce = [&]() __attribute__((always_inline)) {
        const int u = next_task(pk);
        int g0 = 0, n = 0, s0 = 0, seg = 0, nb2 = -1, prb = 0, packed = 0;
        if (u < n_my) decode(u, g0, n, s0, seg, nb2, prb, packed);
        if (lane == 0) {
            int *r = trec[pq & 7];
            r[0] = u < n_my; r[1] = g0; r[2] = n; r[3] = s0; r[4] = seg; r[5] = nb2; r[6] = prb; r[7] = LIST ? packed : (packed | 7 << 4);   // (bits 4..6: live groups; every group without a list)
        }
        ++pq;
    };
    auto rec = [&](int q, int f) __attribute__((always_inline)) { return __builtin_amdgcn_readfirstlane(trec[q & 7][f]); };
    const bool producer = CLS == 0 && ps == 0;
    // a.nprod records before the first barrier, one more at every task switch: the issue side runs 2 NB + ... = four double steps ahead of the compute
    // side, i.e. ceil(4 / shortest task) tasks (host); every record costs the producer wave ~1 500 cycles of scalar work at the head of the launch.
    // (all eight slots start invalid: a record that were read before it is produced would stop the issue side, not send it to a stale address)
    if (producer) {
        if (lane < 8) trec[lane][0] = 0;
        for (int i = 0; i < a.nprod; ++i) produce();
    }
    __syncthreads();
    // ---- this thread's quad of the band: band (row, col) = padded (s0 + row, col), 11 full rows per channel.  Byte
    // offset from the task's scalar base; threads past the band re-read quad 0 and do not write it.
    const bool hasA = tid < XQ;
    const int qa = hasA ? tid : 0;
    const int rowA = (qa % (D6_ROWS * D6_QPR)) / D6_QPR, tcoA = CIN == 1 ? qa / (D6_ROWS * D6_QPR) : 0;   // tcoA: input group of this thread's plane
    const unsigned offA = (unsigned)(((qa / (D6_ROWS * D6_QPR)) * SKP + (long)rowA * HP + (qa % D6_QPR) * 4) * 4);
    const unsigned offA0 = offA - (unsigned)(rowA * HP * 4);               // same quad of band row 0 (always needed, so cached)
    const unsigned offP0 = offA0 - (unsigned)(tcoA * SKP * 4);             // ... of the staged step's first plane (always inside the sample)
    const unsigned offW = (unsigned)((CLS * 64 + lane) * 16);              // this lane's quad inside a 4 KB weight block
    float *const ldsA = xs + tid * 4;
    // ---- issue side (4 steps ahead of the compute side).  A workgroup that has run out of tasks keeps re-reading its
    // last addresses: every ring load stays unconditional and inside the tensors.
    int iq = 0, itc = 0, iL = 0, irl = 0;                                // iq: task sequence number of the issue side
    bool ivalid = rec(0, 0) != 0;
    // decode order: only the band columns the task's diagonals can touch are fetched (rows th_lo..th_hi + 4 tap columns);
    // the other quads of a row read offset 0 of the step instead -- they only ever feed lanes that are not stored
    unsigned t_off = offA, t_off0 = offA0;                              // this thread's offsets for the current issue-side task
    const char *ixn = nullptr, *iwp = nullptr;
    auto issue_setup = [&]() __attribute__((always_inline)) {
        const int ig0 = rec(iq, 1), n = rec(iq, 2), is0 = rec(iq, 3), iseg = rec(iq, 4), inb = rec(iq, 5), iprb = rec(iq, 6);
        const int ipacked = rec(iq, 7) & 15;
        iL = steps_of(ig0);
        irl = ig0 + (C4_PS - 1) + 4 + a.hidden;                         // band rows >= irl - step hold no causal input
        const int irb = ipacked == 4 ? 0 : ((SEG && !ipacked) ? D6_SEG_STEP * iseg : iprb);   // the band window starts at padded column irb
        ixn = (const char *)(a.x + (long)(n % a.x_mod) * G * CIN * SKP + (long)is0 * HP + irb);
        {
            const int qc = qa % D6_QPR;
            if (TAPE && ipacked == 4) {
                // tape: LDS columns 4 qc .. 4 qc + 3 belong to the window whose column range a0 .. a0 + rows + 3 holds them: LDS column c of window
                // (k, slo, a0) <- padded column slo + c - a0 of sample n + 8 k (16-byte aligned: (a0 - slo) % 4 == 0); quads of no window fetch offset 0
                // (the samples of a tape are 8 apart in n and do not wrap around x_mod: the host requires 8 tape_c | x_mod)
                unsigned sh = 0u;
                bool cov = false;
                const unsigned stride8 = (unsigned)(8 * G * CIN * SKP * 4);
#pragma unroll
                for (int wi = 0; wi < 3; ++wi) {
                    const unsigned wd = (unsigned)(wi == 0 ? iseg : (wi == 1 ? inb : iprb));
                    const int k = wd & 7, slo = dc6_piece_slo<TALL>(wd), shi = dc6_piece_shi<TALL>(wd), a0 = (wd >> 15) & 63;
                    const bool in = (wd >> 21) != 0 && 4 * qc + 3 >= a0 && 4 * qc <= a0 + (shi - slo) + 4;   // lanes a0 .. a0 + rows - 1 read columns up to lane + 4
                    if (in) { sh = (unsigned)k * stride8 + (unsigned)((slo - a0) * 4); cov = true; }
                }
                t_off = cov ? offA + sh : 0u;
                t_off0 = cov ? offA0 + sh : 0u;
            } else if (SEG && PACK && ipacked) {
                // quads 0..7 <- sample A's window columns 0..31, quads 9..16 <- sample B's (quad 8 is never read by a stored lane)
                const bool hb = qc > 8;
                const unsigned shift = hb ? (unsigned)(((long)((inb >= 0 ? inb : n) % a.x_mod) - (long)(n % a.x_mod)) * G * CIN * SKP * 4 - 9 * 16) : 0u;
                t_off = offA + shift;
                t_off0 = offA0 + shift;
            } else {
                const int lo = is0 - (gs - 1) - W + 1 - irb, hi = (is0 < H - 1 ? is0 : H - 1) - irb;   // window rows of the task's diagonals
                const bool col_ok = qc >= ((lo > 0 ? lo : 0) >> 2) && qc <= ((hi + 4) >> 2);
                t_off = col_ok ? offA : 0u;
                t_off0 = col_ok ? offA0 : 0u;
            }
        }
        const int gg = ig0 + ps < G ? ig0 + ps : G - 1;                 // a wave without a group reads (and ignores) the last one's weights
        iwp = (const char *)(a.packed + (((long)(n / a.npb) * G + gg) * a.wblk) * 1024);
    };
    if (!ivalid) return;
    issue_setup();
    const long tcs_b = tcs * 4;
    constexpr int WPSTEP = CIN == 4 ? 4096 : 8192;                      // bytes of quad-packed weights per double step (one / two blocks)
    const char *px = ixn, *pw = iwp;
    // Work advances in DOUBLE steps (two staged steps = 2*TCS input groups per barrier): issue_x2 fetches this thread's
    // quads of the next double step and returns where its weights live (*tc0 = its first input group).  Planes of input
    // groups >= G (past the sample) and rows a step cannot use re-read row 0 of the thread's first plane instead.
    auto issue_x2 = [&](f32x4 &ra, f32x4 &rb, int &tc0) __attribute__((always_inline)) -> const char * {
        const char *pwr = pw;
        tc0 = itc;
        unsigned oa, ob;
        if constexpr (CIN == 4) {
            oa = rowA < irl - itc ? t_off : t_off0;
            ob = rowA < irl - itc - 1 ? t_off : t_off0;
        } else {                                                            // plane j of a staged step is input group +j
            const int ta = itc + tcoA, tb = ta + TCS;
            oa = rowA < irl - ta ? t_off : t_off0;
            ob = rowA < irl - tb ? t_off : t_off0;
            if (ta >= G) oa = offP0;
            if (tb >= G) ob = offP0;
        }
        ra = *(const f32x4 *)(px + oa);
        rb = *(const f32x4 *)(px + (itc + TCS < G ? tcs_b : 0) + ob);
        if (ivalid) {
            px += 2 * tcs_b;
            pw += WPSTEP;
            itc += 2 * TCS;
            if (itc >= iL) {
                itc = 0;
                ++iq;
                ivalid = rec(iq, 0) != 0;
                if (ivalid) { issue_setup(); px = ixn; pw = iwp; }
                else { px -= 2 * tcs_b; pw -= WPSTEP; itc = tc0; }              // idle: keep re-reading the last double step
            }
        }
        return pwr;
    };
    // weights of the double step starting at input group tc0: half h uses (a0, a1) / (b0, b1) as the two abid-indexed
    // registers (cin = 4) or a0..a3 / b0..b3 as the single register of its four input groups (cin = 1)
    const long wnet_b = NETS > 1 ? (long)G * a.wblk * 4096 : 0;           // bytes from a net's packed weights to the next net's (NETS = 3)
    auto issue_w2 = [&](const char *p, int tc0, W8 *ws) __attribute__((always_inline)) {
        (void)tc0;                                                          // (blocks past the last input group exist and hold zeros)
#pragma unroll
        for (int net = 0; net < NETS; ++net) {
            W8 &w = ws[net];
            const f32x4 v = *(const f32x4 *)(p + net * wnet_b + offW);
            w.a0 = v[0]; w.a1 = v[1];
            if constexpr (CIN == 4) { w.b0 = v[2]; w.b1 = v[3]; }
            else {
                const f32x4 u = *(const f32x4 *)(p + net * wnet_b + offW + 4096);
                w.a2 = v[2]; w.a3 = v[3];
                w.b0 = u[0]; w.b1 = u[1]; w.b2 = u[2]; w.b3 = u[3];
            }
        }
    };
    // NETS = 3: one half (four input groups) of a double step's weights, every net's -- see the weight ring below
    auto issue_wh = [&](const char *p, auto hh, W8 *ws) __attribute__((always_inline)) {
        constexpr int hf = decltype(hh)::value;
#pragma unroll
        for (int net = 0; net < NETS; ++net) {
            W8 &w = ws[net];
            const f32x4 v = *(const f32x4 *)(p + net * wnet_b + offW + hf * 4096);
            if constexpr (hf == 0) { w.a0 = v[0]; w.a1 = v[1]; w.a2 = v[2]; w.a3 = v[3]; }
            else { w.b0 = v[0]; w.b1 = v[1]; w.b2 = v[2]; w.b3 = v[3]; }
        }
    };
    // register ring: two x sets of two quads, two weight sets; LDS ring: 2 D6_NB double-step buffers.  Double step d reads buffer d mod 2 NB;
    // during it the set loaded two double steps earlier -- the data of double step d + NB -- goes to buffer (d + NB) mod 2 NB and is refilled with
    // double step d + NB + 2; a workgroup barrier every NB double steps (the buffers written between two barriers are the ones read before the first).
    constexpr bool MIDST = D6_STAGE_AT_END == 0 || CIN == 1 || LAT || LIST;   // where the staging block sits (see D6_STAGE_MID / END; LIST: the list kernel's shorter,
                                                                        // more unequal tasks prefer it between the halves again: 120.7 -> 119.9 us per 64-image hidden layer, tools/dc6_list_variants.sh)
    constexpr int NB = D6_NB, NBUF = 2 * D6_NB;
    static_assert(NB == 1 || NB == 2, "one or two double steps per barrier");
    f32x4 xa0 = {0.f, 0.f, 0.f, 0.f}, xb0 = xa0, xa1 = xa0, xb1 = xa0;
    // Weight ring.  NETS = 1: two sets, the set of double step d is refilled with double step d + 2 behind its last MFMA.  NETS = 3: 48 weight registers
    // beside 84 accumulators do not fit the 168 registers of three waves per SIMD, so the ring is ONE set per net, refilled by halves: behind the first
    // half of double step d its a-registers take the first half of double step d + 1, behind the second half the b-registers -- each load still has
    // half a double step (three nets' MFMAs, ~2 700 cycles) to arrive.
    W8 w0[NETS], w1[NETS];
    const char *pw_one = nullptr;                                       // NETS = 3: where the weights of the next double step live
    int tcw;
    { const char *p = issue_x2(xa0, xb0, tcw); issue_w2(p, tcw, w0); }  // double step 0
    { const char *p = issue_x2(xa1, xb1, tcw); if constexpr (NETS == 1) issue_w2(p, tcw, w1); else pw_one = p; }  // double step 1
    if (hasA) { *(f32x4 *)ldsA = xa0; *(f32x4 *)(ldsA + XFL) = xb0; }
    int tcw_next, tcw_next2 = 0;
    const char *pw_next = issue_x2(xa0, xb0, tcw_next), *pw_next2 = nullptr;   // double step 2 (its weights are fetched in double step 0)
    if constexpr (NB == 2) {
        if (hasA) { *(f32x4 *)(ldsA + 2 * XFL) = xa1; *(f32x4 *)(ldsA + 3 * XFL) = xb1; }
        pw_next2 = issue_x2(xa1, xb1, tcw_next2);                       // double step 3
    }
    // ---- compute side: lane = image row th
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    int tq = 0, tc = 0, g0 = 0, n = 0, Lwg = 0, g = 0, s = 0, step = 0;   // tq: task sequence number of the compute side
    bool glive = false, lane_ok = false;
    int n_lane = 0;                                                     // the sample this lane stores to (packed tasks: two per wave)
    // bias / PReLU slope / residual of the task are fetched when the task STARTS (unconditionally, from clamped
    // addresses): by the epilogue they are the oldest loads in flight, so waiting for them does not drain the ring.
    float e_bias[NETS], e_act[NETS], e_res = 0.f;                       // (net k's output channels lie G * cout behind net k - 1's)
    long e_oi = 0;
    const float *const act_p = a.act ? a.act : a.bias, *const res_p = a.residual ? a.residual : a.x;
    const float *const xl0 = xs + (C4_PS - 1 - ps) * D6_COLS + lane;
    auto task_setup = [&]() __attribute__((always_inline)) {
        g0 = rec(tq, 1); n = rec(tq, 2);
        const int s0 = rec(tq, 3), seg = rec(tq, 4), nb2 = rec(tq, 5), prb = rec(tq, 6);
        const int pk7 = rec(tq, 7), packed = pk7 & 15;
        Lwg = steps_of(g0);
        g = g0 + ps;
        s = s0 - ps;
        const int rb = packed == 4 ? 0 : ((SEG && !packed) ? D6_SEG_STEP * seg : prb);
        int row = rb + lane;                                            // this lane's image row
        n_lane = n;
        bool half_ok = true;
        if (TAPE && packed == 4) {                                      // tape: the window that holds this lane
            half_ok = false;
            row = 0;
#pragma unroll
            for (int wi = 0; wi < 3; ++wi) {
                const unsigned wd = (unsigned)(wi == 0 ? seg : (wi == 1 ? nb2 : prb));
                const int k = wd & 7, slo = dc6_piece_slo<TALL>(wd), shi = dc6_piece_shi<TALL>(wd), a0 = (wd >> 15) & 63;
                if ((wd >> 21) != 0 && lane >= a0 && lane <= a0 + (shi - slo)) { half_ok = true; row = slo + lane - a0; n_lane = n + 8 * k; }
            }
        } else if (SEG && PACK && packed) {                             // lanes 0..27: sample n, lanes 36..63: sample nb2
            if (lane >= 36) { row = rb + lane - 36; n_lane = nb2 >= 0 ? nb2 : n; half_ok = nb2 >= 0; }
            else half_ok = lane < 28;
        }
        int sc;
        {
            int lo = s >= W ? s - W + 1 : 0, hi = s < H ? s : H - 1;
            const int segx = packed == 4 ? 0 : seg;                     // (tape records carry a window where the others carry the segment)
            if (lo < seg_lo(segx)) lo = seg_lo(segx);
            if (hi > seg_hi(segx)) hi = seg_hi(segx);
            glive = g < G && ps < gs && s >= 0 && s < S && lo <= hi && ((pk7 >> (4 + ps)) & 1) != 0;   // (a group that is dead on all rows of a list record: its wave set idles through the task)
            lane_ok = glive && half_ok && row >= lo && row <= hi;
            sc = s < 0 ? 0 : (s >= S ? S - 1 : s);
        }
#pragma unroll
        for (int i = 0; i < NETS * NA; ++i) acc[i] = zero4;
        tc = 0;
        const int nout = G * a.cout, gc = g < G ? g : G - 1;
        const int o = gc * a.cout + (CLS < a.cout ? CLS : a.cout - 1), bid = (n / a.npb) * nout + o;
        e_oi = ((long)n_lane * nout + o) * SKP + (long)(sc + D3_S0) * HP + row + D3_C0;
#pragma unroll
        for (int net = 0; net < NETS; ++net) { e_bias[net] = a.bias[bid + net * nout]; e_act[net] = act_p[bid + net * nout]; }
        e_res = res_p[a.residual ? e_oi : 0];
    };
    // The exchange buffer is double-buffered by task parity (round 6).  A task's partial sums are read AFTER the epilogue's barrier, and the next barrier
    // is the step barrier of an even double step: a ONE-double-step task (first layer, group block 0: six input groups) that starts on an odd step reaches
    // its own epilogue -- and rewrote the single buffer -- while a slower wave was still reading the previous task's sums.  Needs two consecutive such tasks in
    // one workgroup: never with <= 32 of them per XCD (48 images), four workgroups per XCD with 96 images -- one image of a 96-image sub-batch decoded wrongly
    // in about one of four three-stream steps, with rounds 1-5's kernels as well (tools/debug/stress_big.py).
    // NETS = 3: one exchange buffer PER NET instead of the pair.  Net k's sums of task t are read between barrier k of t's epilogue and the next barrier
    // the reading wave arrives at; buffer k is written again at net k of task t + 1, by a wave that has passed the barrier in front of that write in its
    // own program order -- barrier k - 1 of t + 1's epilogue (k > 0) or the last barrier before that epilogue (k = 0; barrier 2 of t's epilogue if no
    // step barrier lies in between).  Either one comes AFTER barrier k + 1 (or, for k = 2, barrier 0 of the next epilogue) in every wave's program order,
    // and a wave arrives at that only with its reads of buffer k behind it: whatever the length of a task and the parity of the step it starts on, two
    // other nets' barriers lie between a read and the next write of the same buffer.
    auto epilogue = [&]() __attribute__((always_inline)) {
        static_for<NETS>([&](auto nn) {
            constexpr int net = decltype(nn)::value;
            f32x4 *const ac = acc + net * NA;
            conv6_align<CIN, CLS>(ac);
            const f32x4 part = tree4_eval<CIN, CLS>(ac);
            // (one net, cin = 4: tasks are at least three double steps long, a step barrier always lies in between)
            float *const cb = NETS > 1 ? comb + net * C4_COMB_FLOATS : (CIN == 1 ? comb + (tq & 1) * C4_COMB_FLOATS : comb);
#pragma unroll
            for (int r = 0; r < 4; ++r) cb[((ps * 4 + CLS) * 4 + r) * 64 + lane] = part[r];
            __syncthreads();
            const int r = CLS;
            if (lane_ok && r < a.cout) {
                const long oi = NETS > 1 ? e_oi + net * ((long)a.npb * G * a.cout * SKP) : e_oi;   // net k stores k * npb samples further
                const float f0 = cb[((ps * 4 + 0) * 4 + r) * 64 + lane], f1 = cb[((ps * 4 + 1) * 4 + r) * 64 + lane];
                const float f2 = cb[((ps * 4 + 2) * 4 + r) * 64 + lane], f3 = cb[((ps * 4 + 3) * 4 + r) * 64 + lane];
                float sv = ((f0 + f2) + (f1 + f3)) + e_bias[net];
                if (a.act) { if (sv < 0) sv = sv * e_act[net]; }        // cconv_dc_cuda.cu:360-362
                if (a.residual) sv = sv + (NETS > 1 ? a.residual[oi] : e_res);   // fused TileAdd
                a.out[oi] = sv;
            }
        });
    };
    task_setup();
    // one double step: barrier ; [operands + MFMAs of the first staged step] ; write the next double step's two quads to the
    // other LDS half and refill the set with double step +3 ; [operands + MFMAs of the second staged step] ; refill this
    // double step's weights with double step +2.  A staged step is one input group (cin = 4) or four (cin = 1: plane j of
    // the band is input group tc + j).  (Reading the next step's operands ahead of the barrier from a deeper LDS ring was
    // measured: no gain.)
#define DC6_SUB(H_, J_, W_)                                                                     \
    if constexpr ((J_) < TCS) {                                                                 \
        constexpr int k = (H_) * TCS + (J_);                                                    \
        const int dl = dlim - k;                    /* tap diagonals d >= dl carry zero weights */ \
        if (dl > 0 && tc + k < Lwg) {                                                           \
            float r0[9];                                                                        \
            conv6_load<CIN, CLS, XPLANE>(r0, xl + (H_) * XFL + (J_) * XPLANE);                  \
            __builtin_amdgcn_sched_barrier(0);                                                  \
            static_for<NETS>([&](auto nn) {         /* the operands are read once for all nets */ \
                constexpr int net = decltype(nn)::value;                                        \
                const float wa = W_[net].template get<(H_), (CIN == 4 ? 0 : (J_))>(), wb = W_[net].template get<(H_), 1>(); \
                conv6_diags<CIN, CLS, 0, 3>(acc + net * NA, r0, wa, wb);                        \
                if (dl > 4) conv6_diags<CIN, CLS, 4, 5>(acc + net * NA, r0, wa, wb);            \
                if (dl > 6) conv6_diags<CIN, CLS, 6, 8>(acc + net * NA, r0, wa, wb);            \
            });                                                                                 \
        }                                                                                       \
    }
#define DC6_HALF(H_, W_) DC6_SUB(H_, 0, W_) DC6_SUB(H_, 1, W_) DC6_SUB(H_, 2, W_) DC6_SUB(H_, 3, W_)
#define D6_STAGE_WRITE(XA_, XB_)                                                                \
        if (hasA) {                                                                             \
            float *q = ldsA + ((step + NB) & (NBUF - 1)) * (2 * XFL);                           \
            *(f32x4 *)q = XA_;                                                                  \
            *(f32x4 *)(q + XFL) = XB_;                                                          \
        }
#define D6_STAGE_BLOCK(XA_, XB_)                                                                \
        D6_STAGE_WRITE(XA_, XB_)                                                                \
        DC6_T(8);                       /* (the LDS writes wait for the loads of two double steps ago) */ \
        pw_new = issue_x2(XA_, XB_, tcw_new);                                                   \
        __builtin_amdgcn_sched_barrier(0);
/* The staging block (LDS writes of the set loaded two double steps ago, address selection, the two band loads) sits BEHIND the second half of the */
/* double step for the cin = 4 kernels in throughput mode: hidden layer 106.1 -> 104.4 us against its round-1 place between the halves ("in the */
/* shadow of the first half's MFMAs" -- with twelve waves issuing 24 loads at once the shadow was the other waves' stall).  The first layer */
/* (cin = 1: +1.6 % at the end) and the one-group-per-task latency mode (LAT: single-image decode +1.4 %) keep it between the halves; */
/* D6_STAGE_AT_END=0 restores that everywhere. */
#define D6_STAGE_MID(XA_, XB_) if constexpr (MIDST) { D6_STAGE_BLOCK(XA_, XB_) }
#define D6_STAGE_END(XA_, XB_) if constexpr (!MIDST) { D6_STAGE_BLOCK(XA_, XB_) }
#define DC6_SUBSTEP(XA_, XB_, W_)                                                               \
    {                                                                                           \
        if (tc >= Lwg) {                                                                        \
            epilogue();                                                                         \
            ++tq;                                                                               \
            if (producer) produce();            /* record tq + 5, read many barriers later */   \
            if (rec(tq, 0)) task_setup();                                                       \
            else { done = true; glive = false; Lwg = 0x7fffffff; }                              \
            DC6_ST7                                                                             \
        }                                                                                       \
        DC6_T(0);                                                                               \
        if (NB == 1 || (step & 1) == 0) __syncthreads();                                        \
        DC6_T(1);                                                                               \
        const int dlim = glive ? g + 4 + a.hidden - tc : 0;                                     \
        const float *xl = xl0 + (step & (NBUF - 1)) * (2 * XFL);                                \
        int tcw_new = 0;                                                                        \
        const char *pw_new = nullptr;                                                           \
        DC6_HALF(0, W_)                                                                         \
        if constexpr (NETS > 1) issue_wh(pw_one, IC<0>{}, W_);                                  \
        DC6_T(2);                                                                               \
        D6_STAGE_MID(XA_, XB_)                                                                  \
        DC6_T(3);                                                                               \
        DC6_HALF(1, W_)                                                                         \
        D6_STAGE_END(XA_, XB_)                                                                  \
        DC6_T(4);                                                                               \
        if constexpr (NETS > 1) { issue_wh(pw_one, IC<1>{}, W_); pw_one = pw_next; }            \
        else issue_w2(pw_next, tcw_next, W_);                                                   \
        if constexpr (NB == 2) { pw_next = pw_next2; tcw_next = tcw_next2; pw_next2 = pw_new; tcw_next2 = tcw_new; } \
        else { pw_next = pw_new; tcw_next = tcw_new; }                                          \
        tc += 2 * TCS;                                                                          \
        ++step;                                                                                 \
        DC6_T(5);                                                                               \
        DC6_ST6                                                                                 \
    }
#ifdef DC6_STAMP
#define DC6_ST6 st[6] += 1;
#define DC6_ST7 st[7] += 1;
#else
#define DC6_ST6
#define DC6_ST7
#endif
    bool done = false;
    do {
        if constexpr (NB == 2) {
            if constexpr (NETS == 1) {
                DC6_SUBSTEP(xa0, xb0, w0)                               // double step = 0 (mod 2): stage double step + 2 = x set 0
                DC6_SUBSTEP(xa1, xb1, w1)
            } else {
                DC6_SUBSTEP(xa0, xb0, w0)                               // (one weight set: see the weight ring)
                DC6_SUBSTEP(xa1, xb1, w0)
            }
        } else {
            DC6_SUBSTEP(xa1, xb1, w0)                                   // double step = 0 (mod 2): stage double step + 1 = x set 1
            DC6_SUBSTEP(xa0, xb0, w1)
        }
    } while (!done);
#ifdef DC6_STAMP
    if constexpr (CIN == DC6_STAMP_CIN && !SEG) {
        st[9] = __builtin_amdgcn_s_memtime() - t_entry;
        if (lane == 0) for (int i = 0; i < 10; ++i) dc6_stamps[((blockIdx.x & 255) * 12 + ps * 4 + CLS) * 10 + i] += st[i];
    }
#endif
#undef DC6_ST6
#undef DC6_ST7
#undef DC6_HALF
#undef DC6_SUB
#undef DC6_SUBSTEP
}

template <int CIN, bool SEG, bool LAT, bool TAPE, bool LIST = false, int NETS = 1, bool TALL = false>
__device__ __forceinline__ void dc6_kernel(const Dc3Packed &p, const Dc3Tape *tape, const uint4 *list = nullptr, const int *lcnt = nullptr) {
    __shared__ float xs[4 * D6_NB * D6_XFL(CIN)];
    __shared__ float comb[(NETS > 1 ? NETS : 2) * C4_COMB_FLOATS];       // (two: task parity; three nets per task: one per net -- see epilogue)
    __shared__ int trec[8][16];
    const Dc3Args a = dc6_unpack(p);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), ps = wave >> 2, cls = wave & 3;
    switch (cls) {
        case 0: dc6_body<CIN, 0, SEG, LAT, TAPE, LIST, NETS, TALL>(a, tape, list, lcnt, xs, comb, trec, tid, lane, ps); break;
        case 1: dc6_body<CIN, 1, SEG, LAT, TAPE, LIST, NETS, TALL>(a, tape, list, lcnt, xs, comb, trec, tid, lane, ps); break;
        case 2: dc6_body<CIN, 2, SEG, LAT, TAPE, LIST, NETS, TALL>(a, tape, list, lcnt, xs, comb, trec, tid, lane, ps); break;
        default: dc6_body<CIN, 3, SEG, LAT, TAPE, LIST, NETS, TALL>(a, tape, list, lcnt, xs, comb, trec, tid, lane, ps); break;
    }
}
template <int CIN, bool SEG, bool LAT = false, int NETS = 1>
__global__ __launch_bounds__(C4_THREADS) void k_cconv4v6(Dc3Packed p) { dc6_kernel<CIN, SEG, LAT, false, false, NETS>(p, nullptr); }
// the taped launches (throughput mode, H <= 64): 64 more bytes of arguments and the lane -> piece code only where a plane tapes
template <int CIN, int NETS = 1>
__global__ __launch_bounds__(C4_THREADS) void k_cconv4v6t(Dc3Packed p, Dc3Tape tape) { dc6_kernel<CIN, false, false, true, false, NETS>(p, &tape); }
// the list launches (dead-cone skip, need.h): 16 more bytes of arguments; p.tape_total = records per XCD the list has room for
template <int CIN>
__global__ __launch_bounds__(C4_THREADS) void k_cconv4v6l(Dc3Packed p, const uint4 *list, const int *lcnt) { dc6_kernel<CIN, false, false, true, true>(p, nullptr, list, lcnt); }
// ... of latents of 65..128 rows (TALL: seven-bit rows in the pieces, every record packed)
template <int CIN>
__global__ __launch_bounds__(C4_THREADS) void k_cconv4v6lt(Dc3Packed p, const uint4 *list, const int *lcnt) { dc6_kernel<CIN, false, false, true, true, 1, true>(p, nullptr, list, lcnt); }

// TAPE packing (see Dc3Args), host side: per group block of the launch, the row windows of tape_c consecutive samples of an XCD's list laid end to
// end over as few waves as the kernel's rules allow -- a window piece stores rows slo..shi in lanes a0.. with (a0 - slo) % 4 == 0 (16-byte aligned band
// quads); the column ranges a0 .. a0 + rows + 3 (lane + 0 .. 4) of neighbouring pieces lie in different quads; a stored lane needs its source lanes +-2
// inside the wave unless what they would hold is a product with rows outside the image; at most three pieces per wave (the task record's three words).
// Used where it needs fewer tasks than one sample per task; a block whose tape needs a wave per sample anyway keeps plain tasks inside a taped launch.
// Expects a.ngroup, H, W, npb, x_mod, N, psum, n_gb, n_gbv, nseg set.  (tests/test_dc_tape.py checks the rules on the CPU through lic360_dc4_tape_layout.)
static void dc6_build_tape(Dc3Args &a, Dc3Tape &tape, int h, int w, int cin, int n, int gs, bool nopack) {
    a.tape_c = 0; a.tape_n = 1; a.tape_total = 0; a.tape_magic = 0u; a.tape_nw4[0] = a.tape_nw4[1] = 0u;
    for (int j = 0; j < D6_TAPE_BLOCKS; ++j) tape.s[j] = 0u;
    const int S = h + w - 1, m = a.npb / 8;                             // m: samples per net in an XCD's list
    int c = 0;
    for (int t = D6_TAPE_WAVES; t >= 2 && !c; --t) if (m % t == 0) c = t;
    const bool ok = !nopack && a.nseg == 1 && gs == C4_PS && n % 8 == 0 && a.npb % 8 == 0 && c >= 2 && a.x_mod % (8 * c) == 0 && a.n_gbv <= D6_TAPE_BLOCKS &&
                    8.0 * c * a.ngroup * cin * (double)D3_SP(h, w) * D3_HP(h) * 4.0 < 4294967296.0;     // 32-bit byte offsets between the samples of a tape
    if (!ok) return;
    long old_tasks = 0, new_tasks = 0;
    int nws[D6_TAPE_BLOCKS];
    for (int j = 0; j < a.n_gbv; ++j) {
        const int gb = a.n_gb - 1 - j, s0 = a.psum - gb * C4_PS;
        int lo = 1 << 30, hi = -1;
        for (int q = 0; q < C4_PS; ++q) {
            const int sq = s0 - q;
            if (gb * C4_PS + q >= a.ngroup || sq < 0 || sq >= S) continue;
            const int l = sq >= w ? sq - w + 1 : 0, u = sq < h ? sq : h - 1;
            if (l < lo) lo = l;
            if (u > hi) hi = u;
        }
        int nw = 0, k = 0, slo = lo;
        unsigned starts = 0u;
        bool fits = hi >= 0;
        while (fits && k < c) {
            if (nw >= D6_TAPE_WAVES) { fits = false; break; }
            if (nw & 1) starts |= ((unsigned)k | (unsigned)slo << 3) << (9 * (nw >> 1));
            unsigned pc[3];
            if (dc6_wave_pieces(lo, hi, h, c, k, slo, pc) == 0) fits = false;
            ++nw;
        }
        if (!fits || nw >= c) {                                          // nothing saved (or no room): this block keeps one sample per task
            // (taping only the blocks that save two / three waves of a tape was measured: +0.7 / +2.3 % on the hidden layer)
            nw = c;
            starts = 0u;
        }
        tape.s[j] = starts;
        a.tape_nw4[j >> 3] |= (unsigned)nw << ((j & 7) * 4);
        nws[j] = nw;
        new_tasks += (long)nw * (m / c);
        old_tasks += m;
    }
    if (new_tasks > 0 && new_tasks < old_tasks) {
        a.tape_c = c;
        a.tape_n = n / 8 / c;
        a.tape_magic = (unsigned)((4294967296ull + a.tape_n - 1) / a.tape_n);
        for (int j = 0; j < a.n_gbv; ++j) a.tape_total += a.tape_n * nws[j];
    }
}

// the schedule half of Dc3Args (everything but the pointers): group blocks of the plane, latency / throughput mode, records to produce ahead, packing.
// false: no group block of the layer has a diagonal on this plane (nothing to launch)
static bool dc6_schedule(Dc3Args &a, Dc3Tape &tape, int ngroup, int cin, int cout, int constrain, int n, int h, int w, int nb, int psum, int x_mod, bool nopack, int gstep_mode) {
    a.ngroup = ngroup; a.cout = cout; a.hidden = constrain == 5 ? 0 : 1; a.H = h; a.W = w; a.npb = n / nb; a.x_mod = x_mod; a.N = n;
    a.psum = psum;
    const int S = h + w - 1;
    int gb_lo = 1 << 30, gb_hi = -1;
    // latency mode: with few samples (<= 128 three-group tasks) every group is a task of its own
    const int n_gb3 = (ngroup + C4_PS - 1) / C4_PS;
    const int gs = gstep_mode == 1 || (gstep_mode == 0 && (long)n * n_gb3 <= 128 && D6_NSEG(h) == 1) ? 1 : C4_PS;
    a.gstep = gs;
    {   // shortest task of the launch, in double steps of 2 TCS input groups (chain length of the first group block, capped by the group count)
        const int tcs2 = cin == 4 ? 2 : 8, lmin0 = (gs - 1) + 4 + a.hidden, lmin = lmin0 < ngroup ? lmin0 : ngroup;
        const int dmin = (lmin + tcs2 - 1) / tcs2, lead = (4 + dmin - 1) / dmin;
        a.nprod = lead + 2 < 6 ? lead + 2 : 6;
    }
    const int n_gb_all = (ngroup + gs - 1) / gs;
    for (int gb = 0; gb < n_gb_all; ++gb) {
        int s0 = psum - gb * gs;
        if (s0 - (gs - 1) >= S || s0 < 0) continue;
        if (gb < gb_lo) gb_lo = gb;
        if (gb > gb_hi) gb_hi = gb;
    }
    a.tape_c = 0; a.pack0 = 0;
    if (gb_hi < 0) return false;
    a.n_gb = gb_hi + 1;
    a.n_gbv = gb_hi - gb_lo + 1;
    a.nseg = D6_NSEG(h);
    dc6_build_tape(a, tape, h, w, cin, n, gs, nopack);
    // tall images: the last row segment packs two samples per task when it holds at most 26 rows
    if (a.nseg > 1 && a.npb % 16 == 0 && x_mod % 16 == 0 && !nopack && gs == C4_PS && h >= 28 && D6_SEG_STEP * (a.nseg - 1) + 2 >= h - 28 + 2) a.pack0 = 1;
    return true;
}

// The schedule of a launch.  The FIRST layer of three stacked nets over one input (cin = 1, nb = 3, x_mod * nb == n: sample i of every net reads image
// i), in throughput mode on images of at most 64 rows, is scheduled over its n / 3 IMAGES -- per-XCD lists, tapes, records to produce -- and every task
// runs the three nets (*nets = 3, dc6_body); the kernel then sees a one-net launch of n / 3 samples.  Whether a launch is a throughput-mode launch is
// decided on its n samples, as for every other layer.  no_nets: keep one net per task (the A/B switch LIC360_DC_NONETS).
static bool dc6_schedule_nets(Dc3Args &a, Dc3Tape &tape, int ngroup, int cin, int cout, int constrain, int n, int h, int w, int nb, int psum, int x_mod, bool nopack,
                              int gstep_mode, bool no_nets, int *nets) {
    *nets = 1;
    if (!dc6_schedule(a, tape, ngroup, cin, cout, constrain, n, h, w, nb, psum, x_mod, nopack, gstep_mode)) return false;
    if (no_nets || cin != 1 || nb != 3 || (long)x_mod * nb != n || a.gstep != C4_PS || a.nseg != 1) return true;
    *nets = 3;
    return dc6_schedule(a, tape, ngroup, cin, cout, constrain, n / nb, h, w, 1, psum, x_mod, nopack, 3);
}

static int launch_cconv4v6_dc(hipStream_t stream, const lic360_conv_plan *p, const float *x, const float *packed4, const float *bias,
                              const float *act, const float *residual, float *out, int n, int h, int w, int nb, int psum, int x_mod, bool nopack,
                              int gstep_mode, bool no_nets) {
    Dc3Args a;
    a.x = x; a.packed = packed4; a.wblk = conv4_wblk(p); a.bias = bias; a.act = act; a.residual = residual; a.out = out;
    // the packed tasks add per-lane 32-bit byte offsets of up to 16 samples to the task's base pointer (issue_setup)
    ARG_CHECK(16.0 * p->ngroup * p->cin * (double)D3_SP(h, w) * D3_HP(h) * 4.0 < 4294967296.0);
    ARG_CHECK(h < 32768 && w < 32768 && D6_NSEG(h) <= 15 && p->ngroup <= 127 && p->cout <= 7 && psum >= 0 && psum < 65536);   // the packed argument words (Dc3Packed)
    Dc3Tape tape;
    int nets;
    if (!dc6_schedule_nets(a, tape, p->ngroup, p->cin, p->cout, p->constrain, n, h, w, nb, psum, x_mod, nopack, gstep_mode, no_nets, &nets)) return 0;
    const int gs = a.gstep;
    const Dc3Packed pk = dc6_pack(a);
    if (nets == 3) {                                                    // first layer, three nets per task
        if (a.tape_c) hipLaunchKernelGGL((k_cconv4v6t<1, 3>), dim3(D6_GRID), dim3(C4_THREADS), 0, stream, pk, tape);
        else hipLaunchKernelGGL((k_cconv4v6<1, false, false, 3>), dim3(D6_GRID), dim3(C4_THREADS), 0, stream, pk);
    } else if (a.nseg > 1) {
        if (p->cin == 4) hipLaunchKernelGGL((k_cconv4v6<4, true>), dim3(D6_GRID), dim3(C4_THREADS), 0, stream, pk);
        else hipLaunchKernelGGL((k_cconv4v6<1, true>), dim3(D6_GRID), dim3(C4_THREADS), 0, stream, pk);
    } else if (a.tape_c) {
        if (p->cin == 4) hipLaunchKernelGGL((k_cconv4v6t<4>), dim3(D6_GRID), dim3(C4_THREADS), 0, stream, pk, tape);
        else hipLaunchKernelGGL((k_cconv4v6t<1>), dim3(D6_GRID), dim3(C4_THREADS), 0, stream, pk, tape);
    } else if (p->cin == 4 && gs == 1) hipLaunchKernelGGL((k_cconv4v6<4, false, true>), dim3(D6_GRID), dim3(C4_THREADS), 0, stream, pk);   // latency mode
    else if (p->cin == 4) hipLaunchKernelGGL((k_cconv4v6<4, false>), dim3(D6_GRID), dim3(C4_THREADS), 0, stream, pk);
    else hipLaunchKernelGGL((k_cconv4v6<1, false>), dim3(D6_GRID), dim3(C4_THREADS), 0, stream, pk);
    LAUNCH_CHECK();
    return 0;
}

// The same plane over a device-built task list (lic360_dc_lists_build: [8][cap] records + [8] counts of THIS layer and plane).  Throughput-mode launches
// of images of at most DCL_MAX_H = 128 rows only (the list's records are three-group tasks with tape pieces; taller than a wave: k_cconv4v6lt); cin = 4.
static int launch_cconv4v6_dc_list(hipStream_t stream, const lic360_conv_plan *p, const float *x, const float *packed4, const float *bias,
                                   const float *act, const float *residual, float *out, int n, int h, int w, int nb, int psum, int x_mod,
                                   const uint4 *list, const int *lcnt, int cap) {
    Dc3Args a;
    a.x = x; a.packed = packed4; a.wblk = conv4_wblk(p); a.bias = bias; a.act = act; a.residual = residual; a.out = out;
    // a record's pieces add per-lane 32-bit byte offsets of up to 8 * (DCL_CHUNK - 1) samples to the task's base pointer (issue_setup)
    ARG_CHECK(64.0 * p->ngroup * p->cin * (double)D3_SP(h, w) * D3_HP(h) * 4.0 < 4294967296.0);
    ARG_CHECK(h <= DCL_MAX_H && w < 32768 && p->ngroup <= 127 && p->cout <= 7 && psum >= 0 && psum < 65536 && p->cin == 4 && list && lcnt && cap > 0);
    ARG_CHECK(n % 8 == 0 && (n / nb) % 8 == 0 && x_mod == n);           // XCD lists hold whole nets' samples; the samples of a record are 8 apart and never wrap
    Dc3Tape tape;
    if (!dc6_schedule(a, tape, p->ngroup, p->cin, p->cout, p->constrain, n, h, w, nb, psum, x_mod, true, 3)) return 0;
    ARG_CHECK(a.gstep == C4_PS && a.nseg == D6_NSEG(h));
    a.nseg = 1;                                                         // (a list kernel knows no row segments: its records place every lane)
    a.tape_c = 1;                                                       // (a taped kernel: any non-zero value)
    a.tape_total = cap;
    const Dc3Packed pk = dc6_pack(a);
    if (h > 64) hipLaunchKernelGGL((k_cconv4v6lt<4>), dim3(D6_GRID), dim3(C4_THREADS), 0, stream, pk, list, lcnt);
    else hipLaunchKernelGGL((k_cconv4v6l<4>), dim3(D6_GRID), dim3(C4_THREADS), 0, stream, pk, list, lcnt);
    LAUNCH_CHECK();
    return 0;
}

// Host-only view of the tape packing of one plane (no GPU work): what launch_cconv4v6_dc would put into the kernel's arguments for a layer of `ngroup`
// groups (cin = 4: hidden / last layers, 1: first layer) over n samples of nb nets on plane psum.  *tape_c: samples per tape (0: the launch does not
// tape); blocks[j] = first group of group block j (launch order, heaviest first), nwaves[j] = tasks per tape of block j, windows[(j * 6 + t) * 3 + i] =
// piece i of wave t: k | slo << 3 | shi << 9 | a0 << 15 | 1 << 21 (0 = none).  A first-layer launch that runs its three nets per task (cin = 1, nb = 3,
// x_mod * 3 == n, throughput mode; dc6_schedule_nets) reports the schedule over its n / 3 images.  Arrays of 24 / 24 / 24 * 6 * 3 entries: a bound for ngroup <= 64 (22 three-group blocks), independent of D6_TAPE_BLOCKS (a launch that would need more than
// D6_TAPE_BLOCKS = 16 blocks is not taped); *n_blocks <= 24.
LIC360_API int lic360_dc4_tape_layout(int ngroup, int cin, int n, int nb, int h, int w, int psum, int x_mod, int *tape_c, int *n_blocks, int *blocks, int *nwaves, unsigned *windows) {
    ARG_CHECK(tape_c && n_blocks && blocks && nwaves && windows && ngroup > 0 && ngroup <= 64 && (cin == 1 || cin == 4) && n > 0 && nb > 0 && n % nb == 0 && h > 0 && w > 0 && x_mod > 0);
    Dc3Args a;
    *tape_c = 0; *n_blocks = 0;
    Dc3Tape tape;
    int nets;                                                           // (a first-layer launch of three nets over one input: the schedule over its images)
    if (!dc6_schedule_nets(a, tape, ngroup, cin, 4, cin == 4 ? 6 : 5, n, h, w, nb, psum, x_mod, false, 0, false, &nets)) return 0;
    *n_blocks = a.n_gbv < 24 ? a.n_gbv : 24;                            // (the arrays hold 24 entries; latency-mode schedules of ngroup > 24 one-group blocks are clamped)
    *tape_c = a.tape_c;
    for (int j = 0; j < 24 * 6 * 3; ++j) windows[j] = 0u;
    for (int j = 0; j < a.n_gbv && j < 24; ++j) {
        blocks[j] = (a.n_gb - 1 - j) * a.gstep;
        nwaves[j] = a.tape_c ? (int)((a.tape_nw4[(j >> 3) & 1] >> ((j & 7) * 4)) & 15u) : 0;
        if (!a.tape_c || nwaves[j] >= a.tape_c) continue;
        int lo = 1 << 30, hi = -1;
        for (int q = 0; q < C4_PS; ++q) {
            const int sq = psum - blocks[j] - q;
            if (blocks[j] + q >= ngroup || sq < 0 || sq >= h + w - 1) continue;
            const int l = sq >= w ? sq - w + 1 : 0, u = sq < h ? sq : h - 1;
            if (l < lo) lo = l;
            if (u > hi) hi = u;
        }
        for (int t = 0; t < nwaves[j]; ++t) {                            // what the kernel's producer wave does for a task of wave t
            int k, slo;
            dc6_wave_start(tape.s[j], lo, hi, h, a.tape_c, t, k, slo);
            dc6_wave_pieces(lo, hi, h, a.tape_c, k, slo, &windows[(j * 6 + t) * 3]);
        }
    }
    return 0;
}
