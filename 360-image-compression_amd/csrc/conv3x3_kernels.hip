// conv3x3_kernels.hip -- the 3x3 and 1x1 convolutions of the analysis / synthesis transforms on sphere-apron maps: stride 1, and the
// stride-2 (down-sampling) layers of the analysis transform as a stride parameter of the same body (below: "Stride 2"),
// hand-written for gfx950: the tile loader reads the SPHERE APRON BY INDEX (no padded copy, no SpherePad launch), the epilogue applies
// bias + PReLU + the block's residual add, and the SphereTrim that follows every such convolution becomes the output window (cells outside
// it are simply not computed).  Replaces, per layer, nn.Conv2d + SpherePad + nn.PReLU + SphereTrim (+ the residual add) of
// test/model_zoo.py:45-62 of the reference (ResidualBlockV2), :8-23 (ResidualBlock.conv2), :64-94 (ResidualBlockDown.conv2),
// :144-169 (ResidualBlockUp.conv1 / conv2); apron rule: extension/sphere_pad_cuda.cu:48-65.
//
// Arithmetic: fp32 throughout, v_mfma_f32_16x16x4_f32 (bit for bit a k-ordered fmaf chain of 4 terms); the summation order over
// (input channel, tap) is this kernel's own -- a library convolution fixes none either -- so parity with the oracle's conv2d is to 1e-4.
//
// Mapping.  Implicit GEMM with M = output channels, N = positions, K = (input channel, tap).  A workgroup (8 waves, two per SIMD) owns
// a 16 x 16 tile of output positions of one image and NQ * 48 output channels: wave (mq, nh) keeps 48 channels (3 MFMA row tiles) x
// RW rows x 16 columns in 12 RW accumulator registers (96 at NQ = 4, RW = 8).  Input channels arrive in chunks of 16: their 18 x 18 halo tiles
// go to a double-buffered LDS image by per-lane LDS-DMA (`global_load_lds_dword`: each lane fetches ONE cell from wherever the sphere
// rule says it lives -- longitude wrap, pole rows reflected and mirrored -- so interior and apron cells cost the same), one chunk ahead;
// one barrier per chunk (864 MFMAs per wave).  For a (4-channel group, kw) pair a wave reads RW + 2 B operands (one per input row:
// output row r at tap row kh reads input row r + kh) and 9 A operands (3 kh x 3 row tiles, three 16-byte loads per lane from a stream
// packed in exactly this order, one pair ahead) for 9 RW MFMAs: 0.26 operand fetches per MFMA.  LDS plane pitch 336 = 16 (mod 64)
// banks: the four k-planes of a B read fall on disjoint bank quarters.
//
// Stride 2 (k_sconv3x3s2, the fp32 form; lic360_sconv3x3s2 / lic360_sconv1x1s2).  Replaces SpherePad(2) + nn.Conv2d(c, c', 3, 2, 3) + nn.PReLU + SphereTrim of
// test/model_zoo.py:64-106 (ResidualBlockDown.conv1, SphereConv2) and nn.Conv2d(c, c', 1, 2, 2) + the block's add (ResidualBlockDown.short_cut).  A tile is
// 16 x 16 cells of the OUTPUT's interior; the output has its own grid, and the residual has the output's geometry.  3x3: the halo is 33 x 33 cells per
// channel (output (r, col) at tap (kh, kw) reads halo cell (2 r + kh, 2 col + kw)), 2 RW + 1 B operands per pair for the same 72 MFMAs.  Decisions:
//   LDS      16 channels x 1089 cells = 70 KB per chunk image, 140 KB double-buffered (one workgroup per CU); no tall last tile row (a 35-row halo does not
//            fit twice): a remainder takes an ordinary extra tile row -- every production window is a multiple of 16.
//   waits    35 DMAs per wave and chunk: the counted wait at a chunk's second pair is vmcnt(35), under the 6-bit limit of 63 (static_assert in s3_body).
//   banks    the 16 columns of a plane fall on the even banks, so the plane pitch is ODD (1089): of the two kq planes that a ds_read_b32 group of 32 lanes
//            covers, the second takes the odd banks -- conflict-free, and the per-lane loader needs no de-interleave.  (16 mod 64, the stride-1 pitch,
//            would put every plane on the even banks.)
//   1x1      the loader fetches the even / even cells only: LDS image, reads and waits are the stride-1 1x1's.
// The weight packs are the stride-1 ones.  The stride-1 instantiations compile to the instructions they had before the stride parameter existed.
// The single-pass bf16 form of the pair (k_sconv_b1s2; lic360_sconv3x3s2_bf16x1 / lic360_sconv1x1s2_bf16x1, opt-in): the 1x1 is b3_body<.., 1, 1, 2> on the same
// even / even loader; the 3x3 has a loader of its own -- through registers into a double-buffered bf16 image -- in sconv_b1s2.inc.  Tile decode and launch are shared.
//
// Three arithmetic forms, one of everything else.  s3_body (here) is the fp32 form, b3_body (sconv_bf16x3.inc, opt-in) the split-bf16 form ("bf16x3") and,
// with its lo parts left out, the single-pass bf16 form ("bf16x1"); they differ in their chunk loop, LDS layout and weight pack.  What decides which cells a convolution reads and writes exists once and serves both:
// s3_cell_offset (the source cell of a loader's LDS cell), s3_epilogue (bias, PReLU, residual, window test, store), sconv_tile (a workgroup's LDS and tile decode,
// under the kernel wrappers sconv_workgroup<NT, ..> -- tall last tile row --, sconv_s2_workgroup and sconv_gate_workgroup) and, on the host, one path for every
// entry point: a SconvCall (form, kernel size, stride, gate, channels per workgroup; the operands) through sconv_plan (shape predicate, argument contract, tile
// geometry, grid: the shared checks once, the stride's own beside them) and sconv_launch (the one pick of the kernel instantiation).
//
// The gate of the attention blocks (k_gate_sconv / k_gate_sconv_b3 / k_gate_sconv_b1; lic360_sconv1x1_gate / _bf16x3 / _bf16x1, opt-in:
// lic360_models.set_conv_precision(.., gate="fused")).  Replaces the tail of AttentionBlock, test/model_zoo.py:25-46: nn.Conv2d(c, c, 1) + nn.Sigmoid + the `*` with
// the trunk + the `+` with the input.  The 1x1 stride-1 bodies of the three forms with a compile-time variant of the epilogue (s3_epilogue<RW, 1, 1>):
// out = residual + trunk * (1 / (1 + lic360_expf(-(acc + bias)))), one fp32 rounding per operation.  The trunk pointer travels in S3GateArgs, beside S3Args.
// (The names do not carry the k_sconv prefix: the kernels of that prefix are counted by tests/test_asm_load_hazards.py.)
#include "common.h"
#include "lic360_exact_math.h"
#include <cstdint>
#include <type_traits>

typedef float s3_f4 __attribute__((ext_vector_type(4)));

#define S3_T 16                                      // tile columns (and rows of the main tile shape)
#define S3_THREADS 512
// tile shapes: TR rows x 16 columns, kernel size KS (3, or 1: the transforms' 1x1 layers on the same body).  LDS plane of a channel:
// (TR + KS - 1) x (16 + KS - 1) floats, pitch rounded up to 16 (mod 64) banks; CK input channels per LDS chunk (16 at KS = 3, 32 at KS = 1)
constexpr int s3_pitch(int tr, int ks) { int p = (tr + ks - 1) * (S3_T + ks - 1); while (p % 64 != 16) ++p; return p; }   // TR = 16, KS = 3: 324 -> 336
constexpr int s3_ck(int ks) { return ks == 3 ? 16 : 32; }
constexpr int s3_ndma(int tr, int ks) { return (s3_ck(ks) * s3_pitch(tr, ks) + 511) / 512; }       // DMA instructions per wave and chunk (8 waves x 64 lanes)
constexpr int s3_na4(int ks) { return (3 * ks + 3) / 4; }                                          // 16-byte A loads per lane and (channel group, kw) pair: 3 ks row-tile operands
constexpr int s3_lds(int tr, int ks) { return 2 * 8 * s3_ndma(tr, ks) * 64; }                      // LDS floats of a body: two chunk images

struct S3Args {
    const float *x, *w, *bias, *slope, *res;
    float *out;
    int n, cin, cout, hp, wp;                        // x: [n][cin][hp][wp]; cout = output channels of this launch (all blocks)
    int pad, sphere;                                 // 1: cells of the `pad`-wide apron are read from the interior by the sphere rule; 2: longitude wrap only
                                                     // (rows as they are: a map whose pole rows hold computed values, the 1-ring output of another launch)
    int ring, ringw;                                 // output window = rows [ring, hp - ring) x columns [ringw, wp - ringw) of the input grid
    int rw, tall_last;                               // rows per wave of a tile; tall_last != 0: the last tile row runs rw + 1 rows per wave (the window's remainder rows)
    int ohp, owp, ooff;                              // out: [n][cout][ohp][owp], window cell (ph, pw) at (ph - ooff, pw - ooff)
    int shuffle;                                     // != 0: out is the x2 pixel shuffle of that (Dtow(2, d2w), dtow_cuda.cu:38-75): [n][cout / 4][2 ohp][2 owp], channel 4 p + v of
                                                     // cell (y, x) at channel p, cell (2 y + v / 2, 2 x + v % 2) -- a lane's four accumulator registers are one 2 x 2 block
    int tiles_x, tiles_y;
};

__device__ __forceinline__ void s3_dma(unsigned voff, const float *sbase, unsigned lds_byte_addr) {
    // LDS destination = M0 + lane * 4; M0 is written inside the statement (tests/test_asm_m0.py: the compiler itself never reads M0 here)
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_byte_addr) : "memory");
}
__device__ __forceinline__ const float *s3_uniform(const float *p) {       // the value IS wave-uniform; this tells the compiler
    const unsigned long v = (unsigned long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (const float *)(((unsigned long)hi << 32) | lo);
}
// padded cell (ph, pw) of a sphere map -> the padded cell that holds its value (interior cells map to themselves); sphere_pad_cuda.cu:48-65
__device__ __forceinline__ void s3_sphere(int &ph, int &pw, int hp, int wp, int pad) {
    const int H = hp - 2 * pad, W = wp - 2 * pad;
    int th = ph - pad, tw = pw - pad;
    tw = tw < 0 ? tw + W : (tw >= W ? tw - W : tw);
    if (th < 0) { th = -1 - th; tw = W - 1 - tw; }
    else if (th >= H) { th = 2 * H - 1 - th; tw = W - 1 - tw; }
    ph = th + pad; pw = tw + pad;
}

// float q of a chunk's LDS image <-> (channel q / PL, halo row, halo column) of the CK channels of a chunk, a channel's XR x XC halo cells at
// pitch PL; returns the byte offset of the cell's source in the chunk's first input plane (sphere rule applied).
// ST = 2 (the down-sampling forms): (tr0, tc0) is the tile's first output in INTERIOR coordinates of the output, and halo cell (r, c) is input cell
// (pad + 2 tr0 - KS / 2 + r, pad + 2 tc0 - KS / 2 + c) at KS = 3 -- a (2 TR + 1) x 33 halo -- and the even / even cell (pad + 2 (tr0 + r), pad + 2 (tc0 + c))
// at KS = 1, whose LDS image is therefore the stride-1 one (TR x 16).
template <int CK, int PL, int XR, int XC, int KS, int ST = 1>
__device__ __forceinline__ unsigned s3_cell_offset(const S3Args &a, int tr0, int tc0, int q, long PLg) {
    int ch = q / PL, rem = q - ch * PL;
    if (ch >= CK || rem >= XR * XC) { ch = 0; rem = 0; }                    // pitch padding and the slack behind the last plane: any valid cell
    const int r = rem / XC, c = rem - r * XC;
    int ph, pw;
    if constexpr (ST == 1) { ph = tr0 - KS / 2 + r; pw = tc0 - KS / 2 + c; }
    else if constexpr (KS == 3) { ph = a.pad + 2 * tr0 - 1 + r; pw = a.pad + 2 * tc0 - 1 + c; }
    else { ph = a.pad + 2 * (tr0 + r); pw = a.pad + 2 * (tc0 + c); }
    ph = ph < 0 ? 0 : (ph > a.hp - 1 ? a.hp - 1 : ph);                      // (only cells of outputs outside the window reach past the map)
    pw = pw < 0 ? 0 : (pw > a.wp - 1 ? a.wp - 1 : pw);
    if (a.sphere == 1) s3_sphere(ph, pw, a.hp, a.wp, a.pad);
    else if (a.sphere == 2) { const int W = a.wp - 2 * a.pad; pw = pw < a.pad ? pw + W : (pw >= a.pad + W ? pw - W : pw); }
    return (unsigned)(((long)ch * PLg + (long)ph * a.wp + pw) * 4);
}

// this lane's cells of a chunk: LDS float q = (i * 8 + wave) * 64 + lane, i < NDMA.  b3_body takes them through this loop.  s3_body spells the
// same loop out in place: inlined from here, its kernels recompute the map's extents for every cell (1 - 3 % more instructions, all ahead of
// the first DMA, 0.2 - 0.6 % of the run time of the large shapes), written in place they hoist them as they always did.  b3_body's kernels
// are the other way round: through this call they keep the code they had, with the loop in place their register allocation moves.
template <int NDMA, int CK, int PL, int XR, int XC, int KS, int ST = 1>
__device__ __forceinline__ void s3_cell_offsets(const S3Args &a, int tr0, int tc0, int wave, int lane, long PLg, unsigned (&voff)[NDMA]) {
#pragma unroll
    for (int i = 0; i < NDMA; ++i) voff[i] = s3_cell_offset<CK, PL, XR, XC, KS, ST>(a, tr0, tc0, (i * 8 + wave) * 64 + lane, PLg);
}

// bias, PReLU, residual, store.  Accumulator m, row r, register v: channel co0 + 16 m + 4 kq + v (co0 = the wave's first output channel),
// position (tr0 + nh * RW + r, tc0 + col) of the input grid (col = lane & 15, kq = lane >> 4, PLg = hp * wp); cells outside the window are not written.
// ST = 2: the position is a cell of the OUTPUT's own grid (ohp x owp, window [ring, ohp - ring) x [ringw, owp - ringw)), and so is the residual's.
// GT = 1 (the attention blocks' gate, k_gate_sconv*: stride 1, no PReLU, crop or shuffle): out = residual + trunk * sigmoid(acc + bias), with
// sigmoid(y) = 1 / (1 + lic360_expf(-y)) -- host / device bit-identical -- and one fp32 rounding per operation (the unit is built without contraction);
// `trunk` has the residual's geometry, and both are required.  A compile-time variant: the GT = 0 instantiations are the code they were.
template <int RW, int ST = 1, int GT = 0>
__device__ __forceinline__ void s3_epilogue(const S3Args &a, const s3_f4 (&acc)[3][RW], int img, int tr0, int tc0, int co0, int nh, int col, int kq,
                                            long PLg, const float *trunk = nullptr) {
    const int pw = tc0 + col;
    if constexpr (GT) {
        static_assert(ST == 1, "the gate is a stride-1 epilogue");
        const float *__restrict__ resp = a.res, *__restrict__ trkp = trunk;
        float *__restrict__ outp = a.out;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            const int co = co0 + 16 * m + 4 * kq;
            const s3_f4 bs = *(const s3_f4 *)(a.bias + co);
            s3_f4 rv[RW], tv[RW];
#pragma unroll
            for (int r = 0; r < RW; ++r) {                                  // all trunk and residual loads of the row tile in flight before its first store
                const int ph = tr0 + nh * RW + r;
                const bool ok = ph < a.hp - a.ring && pw < a.wp - a.ringw;
                const long ri = ((long)img * a.cout + co) * PLg + (long)(ok ? ph : a.ring) * a.wp + (ok ? pw : a.ringw);
#pragma unroll
                for (int v = 0; v < 4; ++v) { tv[r][v] = trkp[ri + v * PLg]; rv[r][v] = resp[ri + v * PLg]; }
            }
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const int ph = tr0 + nh * RW + r;
                if (ph < a.hp - a.ring && pw < a.wp - a.ringw) {
                    const long o = ((long)img * a.cout + co) * PLg + (long)ph * a.wp + pw;
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const float y = acc[m][r][v] + bs[v];
                        const float g = 1.0f / (1.0f + lic360_expf(-y));
                        const float tg = tv[r][v] * g;
                        outp[o + v * PLg] = rv[r][v] + tg;
                    }
                }
            }
        }
        return;
    }
    const long oPL = (long)a.ohp * a.owp;
    const int wh = ST == 1 ? a.hp : a.ohp, ww = ST == 1 ? a.wp : a.owp;    // the grid the window is a window of
    const float *__restrict__ resp = a.res;
    float *__restrict__ outp = a.out;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int co = co0 + 16 * m + 4 * kq;
        const s3_f4 bs = *(const s3_f4 *)(a.bias + co);
        s3_f4 sl = {1.f, 1.f, 1.f, 1.f};
        if (a.slope) sl = *(const s3_f4 *)(a.slope + co);
        s3_f4 rv[RW];
        if (resp) {                                                         // all residual loads of the row tile in flight before its first store
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const int ph = tr0 + nh * RW + r;
                const bool ok = ph < wh - a.ring && pw < ww - a.ringw;
                const int rh = ok ? ph : a.ring, rw_ = ok ? pw : a.ringw;
                if constexpr (ST == 2) {                                   // the residual has the OUTPUT's geometry
                    const long ri = ((long)img * a.cout + co) * oPL + (long)rh * a.owp + rw_;
#pragma unroll
                    for (int v = 0; v < 4; ++v) rv[r][v] = resp[ri + v * oPL];
                } else if (a.shuffle) {                                    // the residual has the OUTPUT's (shuffled) geometry
                    typedef float s3_f2 __attribute__((ext_vector_type(2)));
                    const long ri = (((long)img * (a.cout >> 2) + (co >> 2)) * (2 * a.ohp) + 2 * (rh - a.ooff)) * (2 * a.owp) + 2 * (rw_ - a.ooff);
                    const s3_f2 lo = *(const s3_f2 *)(resp + ri), hi = *(const s3_f2 *)(resp + ri + 2 * a.owp);
                    rv[r] = (s3_f4){lo[0], lo[1], hi[0], hi[1]};
                } else {
                    const long ri = ((long)img * a.cout + co) * PLg + (long)rh * a.wp + rw_;
#pragma unroll
                    for (int v = 0; v < 4; ++v) rv[r][v] = resp[ri + v * PLg];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int ph = tr0 + nh * RW + r;
            if (ph < wh - a.ring && pw < ww - a.ringw) {
                float y[4];
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    y[v] = acc[m][r][v] + bs[v];
                    if (a.slope) y[v] = y[v] > 0.f ? y[v] : y[v] * sl[v];
                    if (resp) y[v] = y[v] + rv[r][v];
                }
                if (ST == 1 && a.shuffle) {                                // two 8-byte stores per lane: 16 lanes write 128 contiguous bytes of each of two rows
                    typedef float s3_f2 __attribute__((ext_vector_type(2)));
                    const long o = (((long)img * (a.cout >> 2) + (co >> 2)) * (2 * a.ohp) + 2 * (ph - a.ooff)) * (2 * a.owp) + 2 * (pw - a.ooff);
                    *(s3_f2 *)(outp + o) = (s3_f2){y[0], y[1]};
                    *(s3_f2 *)(outp + o + 2 * a.owp) = (s3_f2){y[2], y[3]};
                } else {
                    const long o = ((long)img * a.cout + co) * oPL + (long)(ph - a.ooff) * a.owp + (pw - a.ooff);
#pragma unroll
                    for (int v = 0; v < 4; ++v) outp[o + v * oPL] = y[v];
                }
            }
        }
    }
}

// weights: [cout block of NQ * 48][cin / 4][kw < ks][mq][j < na4][lane] x 4 floats; lane l = 16 k + i, element e = 4 j + t = 3 kh + mt (e < 3 ks):
// W[co = 48 mq + 16 mt + i][ci = 4 cg + k][kh][kw] -- the A operand of the MFMA for (kh, row tile mt)
__global__ void k_sconv3x3_pack(const float *__restrict__ w, float *__restrict__ packed, int cin, int cout, int nq, int ks, long total) {
    const int na4 = (3 * ks + 3) / 4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int t = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
        long r = idx >> 8;
        const int j = (int)(r % na4); r /= na4;
        const int mq = (int)(r % nq); r /= nq;
        const int kw = (int)(r % ks); r /= ks;
        const int cg = (int)(r % (cin / 4)), blk = (int)(r / (cin / 4));
        const int e = 4 * j + t, kh = e / 3, mt = e - 3 * kh;
        float v = 0.0f;
        if (e < 3 * ks) {
            const int co = blk * nq * 48 + 48 * mq + 16 * mt + (lane & 15), ci = 4 * cg + (lane >> 4);
            v = w[(((long)co * cin + ci) * ks + kh) * ks + kw];
        }
        packed[idx] = v;
    }
}

// the LDS geometry with the stride (file header, "Stride 2"): a (2 TR + 1) x 33 halo at an odd pitch for the 3x3 at stride 2, the stride-1 image otherwise
constexpr int s3_xr(int tr, int ks, int st) { return st == 2 && ks == 3 ? 2 * tr + 1 : tr + ks - 1; }       // halo rows / columns of a tile
constexpr int s3_xc(int ks, int st) { return st == 2 && ks == 3 ? 2 * S3_T + 1 : S3_T + ks - 1; }
constexpr int s3_pitch_st(int tr, int ks, int st) { return st == 2 && ks == 3 ? (s3_xr(tr, ks, st) * s3_xc(ks, st)) | 1 : s3_pitch(tr, ks); }
constexpr int s3_ndma_st(int tr, int ks, int st) { return (s3_ck(ks) * s3_pitch_st(tr, ks, st) + 511) / 512; }
constexpr int s3_lds_st(int tr, int ks, int st) { return 2 * 8 * s3_ndma_st(tr, ks, st) * 64; }
// PQ: the NQ of the weight pack's channel blocks.  PQ > NQ is a "narrow" workgroup (k_narrow_conv / k_narrow_gate below): blockIdx.y counts blocks of NQ * 48
// channels, PQ / NQ of them per pack block; the workgroup reads the pack as it is, its waves at mq slots (blockIdx.y % (PQ / NQ)) * NQ + mq of pack block blockIdx.y / (PQ / NQ)
template <int NQ, int RW, int KS, int ST = 1, int GT = 0, int PQ = NQ>      // NQ * 48 output channels per workgroup, RW rows per wave, KS x KS taps, stride ST; GT: the gate epilogue
__device__ __forceinline__ void s3_body(const S3Args &a, float *lds, int ty, int tx, int img, const float *trunk = nullptr) {
    constexpr int PD = KS == 3 && RW > 3 ? 1 : 3;                           // A operands PD pairs ahead: a 1x1 pair is 24 MFMAs (768 cycles), its operand is fetched three pairs ahead;
                                                                            // so is that of the 3x3 at RW = 2 / 3 (the narrow NQ = 1 form: 18 / 27 MFMAs per pair) -- by
                                                                            // that MFMA count alone: the depth of those bodies has not been measured against one pair
    static_assert(PQ % NQ == 0 && PQ >= NQ, "a narrow workgroup takes a whole fraction of a pack block");
    constexpr int NR = 8 / NQ, TR = NR * RW;                                // row groups per workgroup, tile rows
    constexpr int S3_CK = s3_ck(KS), NPAIR = S3_CK / 4 * KS, NA4 = s3_na4(KS), S3_XC = s3_xc(KS, ST);
    constexpr int S3_PL = s3_pitch_st(TR, KS, ST), S3_NDMA = s3_ndma_st(TR, KS, ST), S3_BUF = 8 * S3_NDMA * 64, S3_XR = s3_xr(TR, KS, ST);
    constexpr int LS = ST == 2 && KS == 3 ? 2 : 1, NB = LS * (RW - 1) + KS;  // LDS cells between neighbouring outputs; B operands (halo rows) per pair
    static_assert(NPAIR % (PD + 1) == 0, "the operand ring's index must be static across chunks");
    static_assert(NA4 * (PD - 1) + S3_NDMA <= 63, "s_waitcnt vmcnt takes at most 63 on gfx950");
    static_assert(S3_CK * S3_PL <= S3_BUF && S3_XR * S3_XC <= S3_PL, "a chunk's planes fit its LDS image");
    float (*xs)[S3_BUF] = (float (*)[S3_BUF])lds;
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), mq = wave % NQ, nh = wave / NQ;
    // input-grid cell of the tile's first output (a.rw: rows per wave of the ordinary tile rows); ST = 2: its interior coordinates in the output
    const int tr0 = (ST == 1 ? a.ring : 0) + ty * (NR * a.rw), tc0 = (ST == 1 ? a.ringw : 0) + tx * S3_T;
    const int blk = PQ == NQ ? blockIdx.y : blockIdx.y / (PQ / NQ), pmq = PQ == NQ ? mq : (int)(blockIdx.y % (PQ / NQ)) * NQ + mq, cblk = PQ * 48;   // pack block, mq slot in it
    const long PLg = (long)a.hp * a.wp;
    unsigned voff[S3_NDMA];
#pragma unroll                                                              // (s3_cell_offsets' loop, in place: see there)
    for (int i = 0; i < S3_NDMA; ++i) voff[i] = s3_cell_offset<S3_CK, S3_PL, S3_XR, S3_XC, KS, ST>(a, tr0, tc0, (i * 8 + wave) * 64 + lane, PLg);
    const float *xb = a.x + (long)img * a.cin * PLg;
    const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) const float *)&xs[0][0];
    auto issue_dma = [&](int ck) __attribute__((always_inline)) {
        const float *sb = s3_uniform(xb + (long)ck * S3_CK * PLg);
        const unsigned lb = lds0 + (unsigned)((ck & 1) * S3_BUF + wave * 64) * 4u;
#pragma unroll
        for (int i = 0; i < S3_NDMA; ++i) s3_dma(voff[i], sb, lb + (unsigned)(i * 8 * 64 * 4));
    };
    const int nck = a.cin / S3_CK, niter = nck * NPAIR;
    // A operands: asm loads + counted waits (hipcc sinks visible loads to just before their first use to save registers, which leaves their
    // L2 latency exposed twice per pair; here the three 16-byte loads of pair it + 1 are issued at the top of pair it and waited for at the
    // top of pair it + 1).  In-order counter: a chunk's 11 DMAs are issued BEHIND the A loads of its first pair, so `vmcnt(11)` at the second
    // pair waits for the operands only and the DMAs have two pairs (~9000 cycles) before a `vmcnt(0)` asks for them.
    const char *wl = (const char *)((const s3_f4 *)a.w + ((long)blk * (a.cin / 4) * KS * PQ + pmq) * NA4 * 64 + lane);   // + it * PQ * NA4 KB per (cg, kw) pair
    auto load_a = [&](int it, s3_f4 (&A)[3]) __attribute__((always_inline)) {
        const char *p = wl + (long)it * (PQ * NA4 * 1024);
        if constexpr (NA4 == 3)
            asm volatile("global_load_dwordx4 %0, %3, off\n\tglobal_load_dwordx4 %1, %3, off offset:1024\n\tglobal_load_dwordx4 %2, %3, off offset:2048"
                         : "=&v"(A[0]), "=&v"(A[1]), "=&v"(A[2]) : "v"(p));
        else
            asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(A[0]) : "v"(p));
    };
#define S3_WAIT_A(N, A_)                                                                                              \
    do {                                                                                                              \
        if constexpr (NA4 == 3) asm volatile("s_waitcnt vmcnt(%3)" : "+v"(A_[0]), "+v"(A_[1]), "+v"(A_[2]) : "n"(N)); \
        else asm volatile("s_waitcnt vmcnt(%1)" : "+v"(A_[0]) : "n"(N));                                              \
    } while (0)
    s3_f4 acc[3][RW];
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int r = 0; r < RW; ++r) acc[m][r] = (s3_f4){0.f, 0.f, 0.f, 0.f};
    issue_dma(0);
    // operand ring: PD + 1 sets, pair `it` in set it % (PD + 1).  The 3x3 tiles of RW >= 4 run one pair ahead (a pair is 72 MFMAs = 2304 cycles per wave at RW = 8);
    // the 1x1 and the 3x3 at RW = 2 / 3 run three ahead (PD above).
    s3_f4 A[PD + 1][3];
#pragma unroll
    for (int d = 0; d < PD; ++d) load_a(d < niter ? d : niter - 1, A[d]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int ck = 0; ck < nck; ++ck) {
        const float *xl = &xs[ck & 1][kq * S3_PL + nh * RW * LS * S3_XC + col * LS];
        float b[2][NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) b[0][j] = xl[j * S3_XC];                // pair 0 of the chunk (the later pairs are read one pair ahead)
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) {                                   // (4-channel group, kw) pairs of the chunk
            const int cur = p & 1, nxt = cur ^ 1, sa = p % (PD + 1), sn = (p + PD) % (PD + 1);
            // in-order counter: behind set sa's loads came PD - 1 younger sets and -- for the PD pairs that follow a chunk's first -- its DMAs
            if (p >= 1 && p <= PD) S3_WAIT_A(NA4 * (PD - 1) + S3_NDMA, A[sa]);  // (registers written by an asm load are only read behind the wait that names them)
            else S3_WAIT_A(NA4 * (PD - 1), A[sa]);
            const int itn = ck * NPAIR + p + PD;
            load_a(itn < niter ? itn : niter - 1, A[sn]);
            if (p == 0 && ck + 1 < nck) issue_dma(ck + 1);
            if (p == 0 && ck + 1 >= nck) {                                   // keep the counts of the waits at p = 1 .. PD right: harmless loads into the idle buffer
#pragma unroll
                for (int i = 0; i < S3_NDMA; ++i) s3_dma(voff[i], s3_uniform(xb), lds0 + (unsigned)(((ck & 1) ^ 1) * S3_BUF + (i * 8 + wave) * 64) * 4u);
            }
            if (p + 1 < NPAIR) {
                const int cgn = (p + 1) / KS, kwn = (p + 1) - KS * cgn;
#pragma unroll
                for (int j = 0; j < NB; ++j) b[nxt][j] = xl[cgn * 4 * S3_PL + j * S3_XC + kwn];
            }
#pragma unroll
            for (int kh = 0; kh < KS; ++kh)
#pragma unroll
                for (int r = 0; r < RW; ++r)
#pragma unroll
                    for (int m = 0; m < 3; ++m) {
                        const int e = 3 * kh + m;
                        acc[m][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[sa][e >> 2][e & 3], b[cur][LS * r + kh], acc[m][r], 0, 0, 0);
                    }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                   // the next chunk's DMAs have landed (and the prefetched A operands)
        __syncthreads();
    }
#undef S3_WAIT_A
    if constexpr (GT) s3_epilogue<RW, 1, 1>(a, acc, img, tr0, tc0, blk * cblk + 48 * pmq, nh, col, kq, PLg, trunk);
    else if constexpr (ST == 1) s3_epilogue<RW>(a, acc, img, tr0, tc0, blk * cblk + 48 * pmq, nh, col, kq, PLg);
    else s3_epilogue<RW, ST>(a, acc, img, a.ring + tr0, a.ringw + tc0, blk * cblk + 48 * pmq, nh, col, kq, PLg);
}

#include "sconv_bf16x3.inc"          // b3_body: the split-bf16 and single-pass bf16 forms of s3_body (arithmetic, pack kernel); everything around the bodies is below
#include "sconv_b1s2.inc"            // b1s2_body: the single-pass bf16 form of the 3x3 at stride 2 (a register-path loader into a double-buffered bf16 image)

// ---- what every workgroup starts with: its LDS (LDS_FLOATS: the body's, of its tallest tile) and its tile, blockIdx.x = (image, tile row, tile column);
// `body(lds, ty, tx, img)` is the rest of the kernel
template <int LDS_FLOATS, class Body>
__device__ __forceinline__ void sconv_tile(const S3Args &a, Body body) {
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    static_assert(sizeof(lds) <= 160 * 1024, "LDS of a gfx950 CU");
    const int tpi = a.tiles_x * a.tiles_y, img = blockIdx.x / tpi, trem = blockIdx.x - img * tpi, ty = trem / a.tiles_x, tx = trem - ty * a.tiles_x;
    body(lds, ty, tx, img);
}
// ---- one workgroup wrapper, one launch for all forms.  NT = bf16 MFMAs per product: 0 the fp32 body, 3 the split-bf16 body, 1 its single-pass form.
template <int NT, int NQ, int RW, int KS, int PQ = NQ>
__device__ __forceinline__ void sconv_body(const S3Args &a, float *lds, int ty, int tx, int img) {
    if constexpr (NT == 3) b3_body<NQ, RW, KS, 3, 1, 0, PQ>(a, lds, ty, tx, img);
    else if constexpr (NT == 1) b3_body<NQ, RW, KS, 1, 1, 0, PQ>(a, lds, ty, tx, img);
    else s3_body<NQ, RW, KS, 1, 0, PQ>(a, lds, ty, tx, img);
}
// the tall last tile row exists where its LDS fits: not in the split-bf16 form at NQ = 1, whose 24-row tile would need 183 KB (sconv_plan leaves tall_last 0 there)
constexpr bool sconv_tall(int nt, int nq, int ks) { return ks == 3 && !(nt == 3 && nq == 1); }
// A window of 16 k + 2 rows (every 1-ring window of these maps) would need a seventeenth tile row with 14 dead rows; instead its LAST tile row
// runs one more row per wave (18 rows at 192 channels, 20 at 96): the workgroup picks its body by its tile row (uniform per workgroup).
template <int NT, int NQ, int RW, int KS, int PQ = NQ>
__device__ __forceinline__ void sconv_workgroup(const S3Args &a) {
    constexpr int TR = 8 / NQ * (RW + (sconv_tall(NT, NQ, KS) ? 1 : 0));    // rows of the tallest tile
    sconv_tile<NT ? b3_lds(TR, KS, NT) : s3_lds(TR, KS)>(a, [&](float *lds, int ty, int tx, int img) {
        if constexpr (sconv_tall(NT, NQ, KS)) {
            if (a.tall_last && ty == a.tiles_y - 1) { sconv_body<NT, NQ, RW + 1, 3, PQ>(a, lds, ty, tx, img); return; }
        }
        sconv_body<NT, NQ, RW, KS, PQ>(a, lds, ty, tx, img);
    });
}
// the stride-2 workgroup (NT = 0: the fp32 form, 1: the single-pass bf16 form): no tall last tile row -- (2 (TR + NR) + 1) x 33 halos do not fit LDS twice -- a
// remainder takes an ordinary tile row
template <int NQ, int RW, int KS, int NT = 0>
__device__ __forceinline__ void sconv_s2_workgroup(const S3Args &a) {
    sconv_tile<NT == 0 ? s3_lds_st(8 / NQ * RW, KS, 2) : KS == 3 ? b1s2_lds() : b3_lds(8 / NQ * RW, 1, 1)>(a, [&](float *lds, int ty, int tx, int img) {
        if constexpr (NT == 0) s3_body<NQ, RW, KS, 2>(a, lds, ty, tx, img);
        else if constexpr (KS == 3) b1s2_body<NQ, RW>(a, lds, ty, tx, img);
        else b3_body<NQ, RW, 1, 1, 2>(a, lds, ty, tx, img);
    });
}
template <int NQ, int RW, int KS> __global__ __launch_bounds__(S3_THREADS) void k_sconv3x3s2(S3Args a) { sconv_s2_workgroup<NQ, RW, KS>(a); }
template <int NQ, int RW, int KS> __global__ __launch_bounds__(S3_THREADS) void k_sconv_b1s2(S3Args a) { sconv_s2_workgroup<NQ, RW, KS, 1>(a); }
template <int NT, int NQ, int RW, int KS>
static auto sconv_s2_kernel() {
    if constexpr (NT == 1) return &k_sconv_b1s2<NQ, RW, KS>;
    else return &k_sconv3x3s2<NQ, RW, KS>;
}
// (a kernel name per form, so that a profile tells the forms apart)
template <int NQ, int RW, int KS> __global__ __launch_bounds__(S3_THREADS) void k_sconv3x3(S3Args a) { sconv_workgroup<0, NQ, RW, KS>(a); }
template <int NQ, int RW, int KS> __global__ __launch_bounds__(S3_THREADS) void k_sconv_b3(S3Args a) { sconv_workgroup<3, NQ, RW, KS>(a); }
template <int NQ, int RW, int KS> __global__ __launch_bounds__(S3_THREADS) void k_sconv_b1(S3Args a) { sconv_workgroup<1, NQ, RW, KS>(a); }
template <int NT, int NQ, int RW, int KS>
static auto sconv_kernel() {
    if constexpr (NT == 3) return &k_sconv_b3<NQ, RW, KS>;
    else if constexpr (NT == 1) return &k_sconv_b1<NQ, RW, KS>;
    else return &k_sconv3x3<NQ, RW, KS>;
}
// ---- the gate of the attention blocks (k_gate_sconv*): the 1x1 stride-1 bodies of the three forms with the gate epilogue (s3_epilogue<RW, 1, 1>).  The
// trunk pointer travels beside S3Args, in an argument struct of the gate kernels' own: the other kernels keep their argument bytes.
struct S3GateArgs {
    S3Args a;
    const float *trunk;                              // [n][cout][hp][wp], as a.res and a.out
};
template <int NT, int NQ, int RW, int PQ = NQ>
__device__ __forceinline__ void sconv_gate_workgroup(const S3GateArgs &g) {
    sconv_tile<NT ? b3_lds(8 / NQ * RW, 1, NT) : s3_lds(8 / NQ * RW, 1)>(g.a, [&](float *lds, int ty, int tx, int img) {
        if constexpr (NT == 0) s3_body<NQ, RW, 1, 1, 1, PQ>(g.a, lds, ty, tx, img, g.trunk);
        else b3_body<NQ, RW, 1, NT, 1, 1, PQ>(g.a, lds, ty, tx, img, g.trunk);
    });
}
template <int NQ, int RW> __global__ __launch_bounds__(S3_THREADS) void k_gate_sconv(S3GateArgs g) { sconv_gate_workgroup<0, NQ, RW>(g); }
template <int NQ, int RW> __global__ __launch_bounds__(S3_THREADS) void k_gate_sconv_b3(S3GateArgs g) { sconv_gate_workgroup<3, NQ, RW>(g); }
template <int NQ, int RW> __global__ __launch_bounds__(S3_THREADS) void k_gate_sconv_b1(S3GateArgs g) { sconv_gate_workgroup<1, NQ, RW>(g); }
template <int NT, int NQ, int RW>
static auto sconv_gate_kernel() {
    if constexpr (NT == 3) return &k_gate_sconv_b3<NQ, RW>;
    else if constexpr (NT == 1) return &k_gate_sconv_b1<NQ, RW>;
    else return &k_gate_sconv<NQ, RW>;
}
// ---- the narrow workgroups (k_narrow_conv / k_narrow_gate; lic360_sconv_narrow / lic360_sconv1x1_gate_narrow, opt-in: lic360_models.set_conv_precision(.., small="narrow")).
// A workgroup of the kernels above takes a whole pack block of output channels (192, or 96 at cout = 96), so a launch has as many workgroups as tiles: 128 on a
// 132 x 260 map, 8 on a 36 x 68 one.  A narrow workgroup takes `cpw` = 96 or 48 of them -- the stride-1 bodies at NQ = 2, RW = 4 resp. NQ = 1, RW = 2 (8 row
// groups; the tall last tile row: RW = 3, 24 rows) with PQ = the pack's NQ -- and the launch has cout / cpw times as many; each re-reads the tile's input (it fits L2)
// and, in the bf16 forms, repeats the chunk's conversion pass.  Same packs, loaders, epilogues, sphere rule, crop and shuffled store: an output's sequence of K steps
// is that of the wide kernel, so the results are bit-identical to it.  The argument struct is S3Args in a wrapper of the kernels' own: tests/test_asm_gate_kernels.py
// counts the kernels whose argument type is S3Args itself, tests/test_asm_load_hazards.py those of the k_sconv prefix.
struct S3NarrowArgs {
    S3Args a;
};
template <int NT, int NQ, int RW, int KS, int PQ> __global__ __launch_bounds__(S3_THREADS) void k_narrow_conv(S3NarrowArgs g) { sconv_workgroup<NT, NQ, RW, KS, PQ>(g.a); }
template <int NT, int NQ, int RW, int PQ> __global__ __launch_bounds__(S3_THREADS) void k_narrow_gate(S3GateArgs g) { sconv_gate_workgroup<NT, NQ, RW, PQ>(g); }

// the forms differ in their chunk of input channels (and so in the shapes they take), in the pack, and in the body
static inline int sconv_ck(int nt, int ks) { return nt ? B3_CK : s3_ck(ks); }
static inline bool sconv_ok(int nt, int cin, int cout, int ks) {
    return (ks == 3 || ks == 1) && cin >= sconv_ck(nt, ks) && cin % sconv_ck(nt, ks) == 0 && cout >= 96 && (cout % 192 == 0 || cout == 96);
}
static inline int sconv_nq(int cout) { return cout % 192 == 0 ? 4 : 2; }    // the pack's channel blocks: NQ * 48 = 192 output channels, or the 96 of cout = 96
static inline long s3_packed(int cin, int cout, int ks) { return sconv_ok(0, cin, cout, ks) ? (long)cout / 48 * (cin / 4) * ks * s3_na4(ks) * 256 : 0; }
static inline long b3_packed_bytes(int nt, int cin, int cout, int ks) { return sconv_ok(nt, cin, cout, ks) ? (long)cout * cin * ks * ks * (nt == 3 ? 4 : 2) : 0; }   // hi + lo bf16 per weight, or hi
static int s3_pack(void *stream, const float *weight, float *packed, int cin, int cout, int ks) {
    ARG_CHECK(weight && packed && sconv_ok(0, cin, cout, ks));
    const long total = s3_packed(cin, cout, ks);
    hipLaunchKernelGGL(k_sconv3x3_pack, dim3(lic360_blocks(total, 4)), dim3(256), 0, (hipStream_t)stream, weight, packed, cin, cout, sconv_nq(cout), ks, total);
    LAUNCH_CHECK();
    return 0;
}
static int b3_pack(int nt, void *stream, const float *weight, void *packed, int cin, int cout, int ks) {
    ARG_CHECK(weight && packed && sconv_ok(nt, cin, cout, ks) && ((uintptr_t)packed & 15) == 0);
    const long total = b3_packed_bytes(nt, cin, cout, ks) / 16;
    hipLaunchKernelGGL(k_sconv_b3_pack, dim3(lic360_blocks(total)), dim3(256), 0, (hipStream_t)stream, weight, (b3_u4 *)packed, cin, cout,
                       sconv_nq(cout), ks, nt == 3 ? 2 : 1, total);
    LAUNCH_CHECK();
    return 0;
}
// the narrow launches: a form the three bodies have, 48 or 96 channels per workgroup and fewer than the pack's block (192 where cout is a multiple of 192, else 96)
static inline bool sconv_narrow_ok(int form, int ks, int cin, int cout, int cpw) {
    return (form == 0 || form == 3 || form == 1) && (cpw == 48 || cpw == 96) && sconv_ok(form, cin, cout, ks) && cpw < sconv_nq(cout) * 48;
}

// ---- one call, one contract, one kernel pick.  Every entry point below fills a SconvCall; sconv_launch is the only way from there to a kernel.
struct SconvCall {
    int nt, ks, stride, gate, cpw;                   // what is asked: the form (0 fp32, 3 split-bf16, 1 single-pass bf16), 3 or 1, 1 or 2, the gate epilogue,
                                                     // channels per workgroup (0: wide, the pack's block)
    const float *x;                                  // the operands: [n][cin][hp][wp]
    const void *packed;                              // the form's stride-1 pack of that kernel size
    const float *bias, *slope, *residual, *trunk;
    float *out;
    int n, cin, cout, hp, wp, pad, sphere;
    int ring, ring_w;                                // stride 1: the window in the input's grid; stride 2: the ring of the OUTPUT's grid around its interior, the window
    int out_crop, shuffle;                           // stride 1 only
};
// the argument contract, tile geometry and grid of a launch.  Stride 2: x has a `pad` apron and an even interior H x W; out / residual are
// [n][cout][H / 2 + 2 ring][W / 2 + 2 ring], whose interior is written; in S3Args hp / wp / pad / sphere are the input's, ohp / owp / ring / ringw the output's grid and window.
static int sconv_plan(const SconvCall &c, S3Args &a, dim3 &grid, int &nq) {
    // what the forms ask of a call of their own
    ARG_CHECK(!c.cpw || (c.stride == 1 && sconv_narrow_ok(c.nt, c.ks, c.cin, c.cout, c.cpw) && (c.ks == 3 || (c.pad == 0 && c.sphere == 0)) && (!c.gate || c.cout % 192 == 0)));
    ARG_CHECK(!c.gate || (c.trunk && c.residual && c.stride == 1 && c.ks == 1));
    // what every call owes
    ARG_CHECK(c.x && c.packed && c.bias && c.out && c.n > 0 && sconv_ok(c.nt, c.cin, c.cout, c.ks) && c.pad >= 0 && c.sphere >= 0);
    ARG_CHECK(!c.sphere || (c.pad >= 1 && c.hp >= 4 * c.pad && c.wp >= 4 * c.pad));   // the wrapped / reflected source of an apron cell is an interior cell
    ARG_CHECK((double)sconv_ck(c.nt, c.ks) * c.hp * c.wp * 4.0 < 4294967296.0 && (!c.nt || ((uintptr_t)c.packed & 15) == 0) && ((uintptr_t)c.bias & 15) == 0 &&
              (!c.slope || ((uintptr_t)c.slope & 15) == 0));                // a chunk's cells at 32-bit byte offsets; 16-byte operand loads
    int rows, cols;                                                         // the window, in cells of the output
    if (c.stride == 1) {
        ARG_CHECK(c.ring >= c.ks / 2 && c.ring_w >= c.ring && c.hp > 2 * c.ring && c.wp > 2 * c.ring_w && c.out_crop >= 0 && c.out_crop <= c.ring && c.sphere <= 2);
        ARG_CHECK(!c.residual || c.out_crop == 0 || c.shuffle);             // the residual has the input's geometry -- or, shuffled, the output's
        ARG_CHECK(!c.shuffle || (((uintptr_t)c.out & 7) == 0 && ((uintptr_t)c.residual & 7) == 0));   // the shuffled store / residual load move aligned pairs
        rows = c.hp - 2 * c.ring; cols = c.wp - 2 * c.ring_w;
        a.ooff = c.out_crop; a.ohp = c.hp - 2 * c.out_crop; a.owp = c.wp - 2 * c.out_crop; a.shuffle = c.shuffle;
    } else {
        ARG_CHECK(c.stride == 2 && c.nt != 3 && c.ring >= 0 && c.ring_w == c.ring && c.hp > 2 * c.pad && c.wp > 2 * c.pad && c.sphere <= 1);
        ARG_CHECK((c.hp - 2 * c.pad) % 2 == 0 && (c.wp - 2 * c.pad) % 2 == 0);   // even interiors: the last tap row / column is the interior's last
        ARG_CHECK(c.ks == 1 || c.pad >= 1);                                 // the 3x3 taps reach one apron row above / column left of the interior
        rows = (c.hp - 2 * c.pad) / 2; cols = (c.wp - 2 * c.pad) / 2;
        ARG_CHECK((long)rows + 2L * c.ring < (1L << 30) && (long)cols + 2L * c.ring < (1L << 30));
        a.ooff = 0; a.ohp = rows + 2 * c.ring; a.owp = cols + 2 * c.ring; a.shuffle = 0;
    }
    a.x = c.x; a.w = (const float *)c.packed; a.bias = c.bias; a.slope = c.slope; a.res = c.residual; a.out = c.out;
    a.n = c.n; a.cin = c.cin; a.cout = c.cout; a.hp = c.hp; a.wp = c.wp; a.pad = c.pad; a.sphere = c.sphere; a.ring = c.ring; a.ringw = c.ring_w;
    nq = c.cpw ? c.cpw / 48 : sconv_nq(c.cout);                             // a workgroup's NQ * 48 channels
    const int nrg = 8 / nq, full = rows / S3_T, rem = rows - full * S3_T;
    a.rw = S3_T / nrg;
    // the remainder fits one more row per wave of the last tile row; not at stride 2 (no tall tile there: a remainder takes an ordinary tile row)
    a.tall_last = c.stride == 1 && sconv_tall(c.nt, nq, c.ks) && rem > 0 && rem <= nrg && full > 0;
    a.tiles_x = (cols + S3_T - 1) / S3_T;
    a.tiles_y = a.tall_last ? full : (rows + S3_T - 1) / S3_T;
    const long tiles = (long)c.n * a.tiles_x * a.tiles_y;
    ARG_CHECK(tiles < (1L << 31) && (!c.cpw || c.cout / c.cpw < 65536));
    grid = dim3((unsigned)tiles, c.cout / (nq * 48));
    return 0;
}
// A run-time value as a template argument, through a generic lambda (codec_fused.hip: imp_tables_launch).  The workgroup shapes are (NQ, PQ) with RW = 2 NQ:
// the wide (4, 4) and (2, 2), the narrow (2, 4), (1, 4) and (1, 2).  Each branch below is closed where no kernel of it exists, and the contract above refuses
// the same calls: no split-bf16 form at stride 2, no narrow gate on a pack of 96-channel blocks.
template <int V> using sconv_int = std::integral_constant<int, V>;
static int sconv_launch(void *stream, const SconvCall &c) {
    S3GateArgs g;
    dim3 grid;
    int nq;
    if (const int rc = sconv_plan(c, g.a, grid, nq)) return rc;
    g.trunk = c.trunk;
    const int pq = sconv_nq(c.cout);
    auto launch = [&](auto kernel, const auto &args) { hipLaunchKernelGGL(kernel, grid, dim3(S3_THREADS), 0, (hipStream_t)stream, args); };
    auto pick = [&](auto nt_, auto ks_, auto nq_, auto pq_) {
        constexpr int NT = decltype(nt_)::value, KS = decltype(ks_)::value, NQ = decltype(nq_)::value, PQ = decltype(pq_)::value, RW = 2 * NQ;
        if constexpr (NQ != PQ) {
            if (!c.gate) launch(&k_narrow_conv<NT, NQ, RW, KS, PQ>, S3NarrowArgs{g.a});
            else if constexpr (PQ == 4) launch(&k_narrow_gate<NT, NQ, RW, PQ>, g);
        } else if (c.gate) launch(sconv_gate_kernel<NT, NQ, RW>(), g);
        else if (c.stride == 1) launch(sconv_kernel<NT, NQ, RW, KS>(), g.a);
        else if constexpr (NT != 3) launch(sconv_s2_kernel<NT, NQ, RW, KS>(), g.a);
    };
    auto by_shape = [&](auto nt_, auto ks_) {
        if (nq == 4) pick(nt_, ks_, sconv_int<4>(), sconv_int<4>());
        else if (nq == pq) pick(nt_, ks_, sconv_int<2>(), sconv_int<2>());
        else if (nq == 2) pick(nt_, ks_, sconv_int<2>(), sconv_int<4>());
        else if (pq == 4) pick(nt_, ks_, sconv_int<1>(), sconv_int<4>());
        else pick(nt_, ks_, sconv_int<1>(), sconv_int<2>());
    };
    auto by_ks = [&](auto nt_) { if (c.ks == 3) by_shape(nt_, sconv_int<3>()); else by_shape(nt_, sconv_int<1>()); };
    if (c.nt == 3) by_ks(sconv_int<3>()); else if (c.nt == 1) by_ks(sconv_int<1>()); else by_ks(sconv_int<0>());
    LAUNCH_CHECK();
    return 0;
}

LIC360_API int lic360_sconv3x3_supported(int cin, int cout) { return sconv_ok(0, cin, cout, 3) ? 1 : 0; }
LIC360_API long lic360_sconv3x3_packed_floats(int cin, int cout) { return s3_packed(cin, cout, 3); }
LIC360_API int lic360_sconv3x3_pack(void *stream, const float *weight, float *packed, int cin, int cout) { return s3_pack(stream, weight, packed, cin, cout, 3); }
LIC360_API int lic360_sconv3x3(void *stream, const float *x, const float *packed, const float *bias, const float *slope, const float *residual, float *out,
                               int n, int cin, int cout, int hp, int wp, int pad, int sphere, int ring, int ring_w, int out_crop, int shuffle) {
    return sconv_launch(stream, {0, 3, 1, 0, 0, x, packed, bias, slope, residual, nullptr, out, n, cin, cout, hp, wp, pad, sphere, ring, ring_w, out_crop, shuffle});
}
// the transforms' 1x1 layers on the same body (K = input channels only, no halo): bias + PReLU + residual in the epilogue, the window as above
LIC360_API int lic360_sconv1x1_supported(int cin, int cout) { return sconv_ok(0, cin, cout, 1) ? 1 : 0; }
LIC360_API long lic360_sconv1x1_packed_floats(int cin, int cout) { return s3_packed(cin, cout, 1); }
LIC360_API int lic360_sconv1x1_pack(void *stream, const float *weight, float *packed, int cin, int cout) { return s3_pack(stream, weight, packed, cin, cout, 1); }
LIC360_API int lic360_sconv1x1(void *stream, const float *x, const float *packed, const float *bias, const float *slope, const float *residual, float *out,
                               int n, int cin, int cout, int hp, int wp, int ring, int ring_w, int crop, int shuffle) {
    return sconv_launch(stream, {0, 1, 1, 0, 0, x, packed, bias, slope, residual, nullptr, out, n, cin, cout, hp, wp, 0, 0, ring, ring_w, crop, shuffle});
}
// the split-bf16 forms of the four
LIC360_API int lic360_sconv3x3_bf16x3_supported(int cin, int cout) { return sconv_ok(3, cin, cout, 3) ? 1 : 0; }
LIC360_API long lic360_sconv3x3_bf16x3_packed_bytes(int cin, int cout) { return b3_packed_bytes(3, cin, cout, 3); }
LIC360_API int lic360_sconv3x3_bf16x3_pack(void *stream, const float *weight, void *packed, int cin, int cout) { return b3_pack(3, stream, weight, packed, cin, cout, 3); }
LIC360_API int lic360_sconv3x3_bf16x3(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                                      int n, int cin, int cout, int hp, int wp, int pad, int sphere, int ring, int ring_w, int out_crop, int shuffle) {
    return sconv_launch(stream, {3, 3, 1, 0, 0, x, packed, bias, slope, residual, nullptr, out, n, cin, cout, hp, wp, pad, sphere, ring, ring_w, out_crop, shuffle});
}
LIC360_API int lic360_sconv1x1_bf16x3_supported(int cin, int cout) { return sconv_ok(3, cin, cout, 1) ? 1 : 0; }
LIC360_API long lic360_sconv1x1_bf16x3_packed_bytes(int cin, int cout) { return b3_packed_bytes(3, cin, cout, 1); }
LIC360_API int lic360_sconv1x1_bf16x3_pack(void *stream, const float *weight, void *packed, int cin, int cout) { return b3_pack(3, stream, weight, packed, cin, cout, 1); }
LIC360_API int lic360_sconv1x1_bf16x3(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                                      int n, int cin, int cout, int hp, int wp, int ring, int ring_w, int crop, int shuffle) {
    return sconv_launch(stream, {3, 1, 1, 0, 0, x, packed, bias, slope, residual, nullptr, out, n, cin, cout, hp, wp, 0, 0, ring, ring_w, crop, shuffle});
}
// the single-pass bf16 forms of the four: the argument lists of the split-bf16 ones, a pack of their own (hi planes only, 2 bytes per weight)
LIC360_API int lic360_sconv3x3_bf16x1_supported(int cin, int cout) { return sconv_ok(1, cin, cout, 3) ? 1 : 0; }
LIC360_API long lic360_sconv3x3_bf16x1_packed_bytes(int cin, int cout) { return b3_packed_bytes(1, cin, cout, 3); }
LIC360_API int lic360_sconv3x3_bf16x1_pack(void *stream, const float *weight, void *packed, int cin, int cout) { return b3_pack(1, stream, weight, packed, cin, cout, 3); }
LIC360_API int lic360_sconv3x3_bf16x1(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                                      int n, int cin, int cout, int hp, int wp, int pad, int sphere, int ring, int ring_w, int out_crop, int shuffle) {
    return sconv_launch(stream, {1, 3, 1, 0, 0, x, packed, bias, slope, residual, nullptr, out, n, cin, cout, hp, wp, pad, sphere, ring, ring_w, out_crop, shuffle});
}
LIC360_API int lic360_sconv1x1_bf16x1_supported(int cin, int cout) { return sconv_ok(1, cin, cout, 1) ? 1 : 0; }
LIC360_API long lic360_sconv1x1_bf16x1_packed_bytes(int cin, int cout) { return b3_packed_bytes(1, cin, cout, 1); }
LIC360_API int lic360_sconv1x1_bf16x1_pack(void *stream, const float *weight, void *packed, int cin, int cout) { return b3_pack(1, stream, weight, packed, cin, cout, 1); }
LIC360_API int lic360_sconv1x1_bf16x1(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                                      int n, int cin, int cout, int hp, int wp, int ring, int ring_w, int crop, int shuffle) {
    return sconv_launch(stream, {1, 1, 1, 0, 0, x, packed, bias, slope, residual, nullptr, out, n, cin, cout, hp, wp, 0, 0, ring, ring_w, crop, shuffle});
}
// the attention blocks' gate in the three forms: out = residual + trunk * sigmoid(conv1x1(x) + bias) on the window, one launch; they read the stride-1 1x1 packs
LIC360_API int lic360_sconv1x1_gate(void *stream, const float *x, const float *packed, const float *bias, const float *trunk, const float *residual, float *out,
                                    int n, int cin, int cout, int hp, int wp, int ring, int ring_w) {
    return sconv_launch(stream, {0, 1, 1, 1, 0, x, packed, bias, nullptr, residual, trunk, out, n, cin, cout, hp, wp, 0, 0, ring, ring_w, 0, 0});
}
LIC360_API int lic360_sconv1x1_gate_bf16x3(void *stream, const float *x, const void *packed, const float *bias, const float *trunk, const float *residual, float *out,
                                           int n, int cin, int cout, int hp, int wp, int ring, int ring_w) {
    return sconv_launch(stream, {3, 1, 1, 1, 0, x, packed, bias, nullptr, residual, trunk, out, n, cin, cout, hp, wp, 0, 0, ring, ring_w, 0, 0});
}
LIC360_API int lic360_sconv1x1_gate_bf16x1(void *stream, const float *x, const void *packed, const float *bias, const float *trunk, const float *residual, float *out,
                                           int n, int cin, int cout, int hp, int wp, int ring, int ring_w) {
    return sconv_launch(stream, {1, 1, 1, 1, 0, x, packed, bias, nullptr, residual, trunk, out, n, cin, cout, hp, wp, 0, 0, ring, ring_w, 0, 0});
}
// the stride-2 forms of the fp32 pair (the analysis transform's down-sampling layers); they read the stride-1 packs
LIC360_API int lic360_sconv3x3s2_supported(int cin, int cout) { return sconv_ok(0, cin, cout, 3) ? 1 : 0; }
LIC360_API int lic360_sconv3x3s2(void *stream, const float *x, const float *packed, const float *bias, const float *slope, const float *residual, float *out,
                                 int n, int cin, int cout, int hp, int wp, int pad, int sphere, int oring) {
    return sconv_launch(stream, {0, 3, 2, 0, 0, x, packed, bias, slope, residual, nullptr, out, n, cin, cout, hp, wp, pad, sphere, oring, oring, 0, 0});
}
LIC360_API int lic360_sconv1x1s2_supported(int cin, int cout) { return sconv_ok(0, cin, cout, 1) ? 1 : 0; }
LIC360_API int lic360_sconv1x1s2(void *stream, const float *x, const float *packed, const float *bias, const float *slope, const float *residual, float *out,
                                 int n, int cin, int cout, int hp, int wp, int pad, int oring) {
    return sconv_launch(stream, {0, 1, 2, 0, 0, x, packed, bias, slope, residual, nullptr, out, n, cin, cout, hp, wp, pad, 0, oring, oring, 0, 0});
}
// the single-pass bf16 forms of the stride-2 pair (opt-in: lic360_models.set_conv_precision(.., stride2="bf16x1")); they read the stride-1 single-pass packs
LIC360_API int lic360_sconv3x3s2_bf16x1_supported(int cin, int cout) { return sconv_ok(1, cin, cout, 3) ? 1 : 0; }
LIC360_API int lic360_sconv3x3s2_bf16x1(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                                        int n, int cin, int cout, int hp, int wp, int pad, int sphere, int oring) {
    return sconv_launch(stream, {1, 3, 2, 0, 0, x, packed, bias, slope, residual, nullptr, out, n, cin, cout, hp, wp, pad, sphere, oring, oring, 0, 0});
}
LIC360_API int lic360_sconv1x1s2_bf16x1_supported(int cin, int cout) { return sconv_ok(1, cin, cout, 1) ? 1 : 0; }
LIC360_API int lic360_sconv1x1s2_bf16x1(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                                        int n, int cin, int cout, int hp, int wp, int pad, int oring) {
    return sconv_launch(stream, {1, 1, 2, 0, 0, x, packed, bias, slope, residual, nullptr, out, n, cin, cout, hp, wp, pad, 0, oring, oring, 0, 0});
}
// the narrow workgroups (above: "the narrow workgroups"): one entry point for the stride-1 convolutions of every form and kernel size, one for the gate.  form: 0 fp32,
// 3 split-bf16, 1 single-pass bf16; `packed` is the form's ordinary pack of that kernel size; ks = 1 takes pad = 0, sphere = 0.  Refusals precede any launch.
LIC360_API int lic360_sconv_narrow_supported(int form, int ks, int cin, int cout, int cpw) { return sconv_narrow_ok(form, ks, cin, cout, cpw) ? 1 : 0; }
LIC360_API int lic360_sconv_narrow(void *stream, int form, int ks, int cpw, const float *x, const void *packed, const float *bias, const float *slope, const float *residual,
                                   float *out, int n, int cin, int cout, int hp, int wp, int pad, int sphere, int ring, int ring_w, int out_crop, int shuffle) {
    ARG_CHECK(cpw != 0);                                                    // (0 is the descriptor's "wide")
    return sconv_launch(stream, {form, ks, 1, 0, cpw, x, packed, bias, slope, residual, nullptr, out, n, cin, cout, hp, wp, pad, sphere, ring, ring_w, out_crop, shuffle});
}
LIC360_API int lic360_sconv1x1_gate_narrow(void *stream, int form, int cpw, const float *x, const void *packed, const float *bias, const float *trunk, const float *residual,
                                           float *out, int n, int cin, int cout, int hp, int wp, int ring, int ring_w) {
    ARG_CHECK(cpw != 0);
    return sconv_launch(stream, {form, 1, 1, 1, cpw, x, packed, bias, nullptr, residual, trunk, out, n, cin, cout, hp, wp, 0, 0, ring, ring_w, 0, 0});
}
