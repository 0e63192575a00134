// need.h -- the "dead cone" of the latent entropy nets (round 6), shared by need_kernels.hip, the two conv kernels and the fused codec.
//
// A symbol (g, y, x) with mask < 0.5 is never coded (extension/coder.cpp:79), so nothing can observe the last layer's outputs at it; and
// an activation of layer l at (g, q) is dead unless some live output of layer l + 1 reads it with a non-zero weight.  Layer l + 1 at
// position p, group gp reads q = p + d, d in [-2, 2]^2, input groups <= gp - d_y - d_x (extension/cconv_ec_cuda.cu:288-290 with hidden = 1,
// the same rule in decode order: cconv_dc_cuda.cu:313-364), and the residual blocks read (g, q) itself (covered by d = 0).  With the
// importance mask a prefix in g (g < L[y/2, x/2]: ImpMap -> Dtow) the live groups of a position are a prefix too:
//   need_11(p)  = highest group with mask >= 0.5 at p                      (-1: none)
//   need_l(q)   = min(G - 1, max over p in q + [-2, 2]^2 of need_{l+1}(p) + (p_y - q_y) + (p_x - q_x))   (need_{l+1}(p) >= 0 only; < 0: -1)
// i.e. "plane of the last consumer" t = need + y + x is dilated 5 x 5 per layer.  The reference computes the dead cells too; skipping them
// changes no bitstream and no decoded symbol (they are only read by chains whose own outputs are dead, or with zero weights: the cells
// hold finite values and fma(0, finite, acc) == acc.  Finite because a cell is never more than 12 layers away from real symbols: the decode order
// has one buffer per layer, the encode order clears its two sparsely written ping-pong buffers at the start of every call -- DESIGN 4.6,
// tests/skip_age_cases.py).
#pragma once
#include <cstdint>

#define NEED_LAYERS 12
#define NEED_STAT_G 64                     // statistics rows: [layer][group] stored cells (decode order), [layer][group block] live tiles (encode order)

// ---- decode order: per (layer, plane, XCD) lists of task records for cconv4v6_dc.inc's LIST kernels.
// record = uint4: x = g0 | packed << 7 | n << 10   (packed 4: up to three pieces y / z / w, sample n + 8 k each; packed 0: sample n, whole diagonals);
//                 bits 22..24 of y: which of the block's three groups g0, g0 + 1, g0 + 2 are live on some row of the record (the others' wave sets idle)
// piece  = k | slo << 3 | shi << 9 | a0 << 15 | 1 << 21   (rows slo..shi of sample k of the chunk in lanes a0.., as the tape's pieces)
// Latents of 65..128 rows ("tall"): a row has seven bits.  The six low bits stay where they are, bit 6 of slo is bit 25 of the piece word, bit 6 of shi
// bit 26 -- a piece of a latent of at most 64 rows is the word it always was, and the kernel of those latents decodes it with the instructions it always
// had.  Every live block of a tall latent is packed (a whole image does not fit a wave, so there is no plain record); a window of up to 128 rows is cut
// over two or three waves by the same rule that cuts a 64-row window over two.
#define DCL_CHUNK 8                        // samples per packing chunk (k has 3 bits)
#define DCL_MAX_H 128                      // tallest latent the lists pack
__host__ __device__ inline unsigned dcl_piece(int k, int slo, int shi, int a0) {
    return (unsigned)k | (unsigned)(slo & 63) << 3 | (unsigned)(shi & 63) << 9 | (unsigned)a0 << 15 | 1u << 21 | (unsigned)(slo >> 6) << 25 | (unsigned)(shi >> 6) << 26;
}
__host__ __device__ inline int dcl_piece_slo(unsigned w) { return (int)((w >> 3) & 63u) | (int)((w >> 25) & 1u) << 6; }
__host__ __device__ inline int dcl_piece_shi(unsigned w) { return (int)((w >> 9) & 63u) | (int)((w >> 26) & 1u) << 6; }
// Waves that can START with a piece of one window of an image of h rows: a wave's first piece begins at lane a0 <= 5 and, unless it ends its window,
// is cut at lane 61 -- it holds at least 57 rows.  So a window of r rows is the first piece of at most 1 + (r - 1) / 57 waves, every wave has exactly
// one first piece, and the waves of a chunk of c windows number at most c times that: the records a list must have room for, per sample.
// (At most 64 rows: a block whose packing needs more waves than it has live samples keeps one plain record per sample instead.)
#define DCL_WAVES_PER_WINDOW(h) ((h) <= 64 ? 1 : 1 + ((h) - 1) / 57)

// The pieces of ONE wave: cconv4v6_dc.inc's dc6_wave_pieces with a row window PER SAMPLE (lo[k]..hi[k], hi < lo: nothing of that sample
// is live on this plane).  Same rules: (a0 - slo) % 4 == 0; the next piece starts in the quad behind this piece's last band column (last lane + 4);
// a0 >= 2 unless the piece starts with image row 0, last lane <= 61 unless it ends with the image's last row; a window may be cut between two
// waves; at most three pieces.  (k, slo) advance to the start of the next wave (k == c: all samples placed).
__host__ __device__ inline int dcl_wave_pieces(const int *lo, const int *hi, int h, int c, int &k, int &slo, unsigned out[3]) {
    int nwin = 0, pos = 0;
    out[0] = out[1] = out[2] = 0u;
    while (nwin < 3 && k < c) {
        if (hi[k] < lo[k]) { ++k; if (k < c) slo = lo[k]; continue; }
        int a0 = pos;
        if (slo != 0 && a0 < 2) a0 = 2;
        a0 += (slo - a0) & 3;
        const int top = hi[k] == h - 1 ? 63 : 61;
        int shi = hi[k];
        if (a0 + (hi[k] - slo) > top) shi = slo + (61 - a0);               // cut
        if (a0 > 61 || (shi < hi[k] && (a0 > 57 || shi - slo + 1 < 4))) break;   // no room (for a useful piece of a cut window)
        out[nwin++] = dcl_piece(k, slo, shi, a0);
        pos = ((a0 + (shi - slo) + 4) / 4 + 1) * 4;
        slo = shi + 1;
        if (slo > hi[k]) { ++k; if (k < c) slo = lo[k]; }
    }
    return nwin;
}

// ---- decode order: which workgroup meets which record when (LIC360_DC_ORDER; DESIGN 4.6 "List order").
// The decode kernel's static walk (cconv4v6_dc.inc: nth_task): workgroup w of an XCD's W runs, as its k-th task, the record at k W + w (k even) or
// k W + W - 1 - w (k odd) of the XCD's list.  A ROUND is therefore W consecutive records, run side by side through one L2; the builder decides which
// records share a round (the emission order, k_dc_tasks) and which workgroup gets which of them (the placement pass, k_dc_place).
#define D6_GRID 256                        // workgroups per launch of the decode kernels: one per CU
#define DCL_WGS(xcd) ((D6_GRID - (xcd) + 7) >> 3)   // workgroups of a launch that run on XCD xcd (the kernel's wgs_per_xcd)
#define DCL_MAXW 32                        // DCL_WGS(0)
#define DCL_MAX_NB 8                       // blocks per emission group (LIC360_DC_ORDER = 1, 2, 4, 8)
// Work of a record = the steps of its block's longest chain (what k_dc_balance evens out between the XCDs); a workgroup's load in the placement pass
// counts DCL_TASK_SWITCH more per task (setup, drain and epilogue of a task, in steps).
#define DCL_TASK_SWITCH 3
__host__ __device__ inline int dcl_steps(unsigned x, int G) { const int g0 = (int)(x & 127u), s = g0 + 2 + 4 + 1; return s < G ? s : G; }
// Grouped emission: the blocks of a plane (heaviest first) in groups of nb; inside a group net, then record index r, then block -- record r of every
// block of the group, one net, lie next to each other (neighbouring blocks of a sample read band rows that overlap in 8 of 11 diagonals).
// -> position inside the group of record r of net `net` of the group's block jj (nrec[0..n): records per net of the group's blocks).  nb = 1: net * nrec + r.
__host__ __device__ inline int dcl_group_pos(const int *nrec, int n, int jj, int net, int r) {
    int tot = 0, before = 0;
    for (int i = 0; i < n; ++i) { tot += nrec[i]; before += (nrec[i] < r ? nrec[i] : r) + (i < jj && nrec[i] > r); }
    return net * tot + before;
}
// Placement of ONE round: its n <= W records (cost[i], list order) sorted by cost descending (ties: list index) go to the workgroups that have a slot
// in this round (all of them; in a short last round those of its first n slots) by load ascending (ties: workgroup index); pos[i] = the slot of record i
// in the round, load[w] += its cost.  Threads t0, t0 + tstep, .. share the work between `sync`s (device: the lanes of a workgroup and __syncthreads;
// host: t0 = 0, tstep = 1 and a sync that does nothing); inv: n ints of scratch.
template <class Sync>
__host__ __device__ inline void dcl_place_round(const int *cost, int n, int W, int odd, int *load, int *inv, int *pos, int t0, int tstep, Sync sync) {
    for (int t = t0; t < n; t += tstep) {
        const int w = odd ? W - n + t : t;                                  // candidate t, ascending workgroup index
        int rl = 0, rc = 0;
        for (int u = 0; u < n; ++u) {
            const int wu = odd ? W - n + u : u;
            rl += load[wu] < load[w] || (load[wu] == load[w] && u < t);
            rc += cost[u] > cost[t] || (cost[u] == cost[t] && u < t);
        }
        inv[rl] = w;
        pos[t] = rc;
    }
    sync();
    for (int t = t0; t < n; t += tstep) {
        const int w = inv[pos[t]];
        pos[t] = odd ? W - 1 - w : w;
        load[w] += cost[t];
    }
    sync();
}
// The order in which the placement pass takes the rounds of a list of n records: a short last round FIRST, then the full rounds in list order.  The short
// round's records can only go to the workgroups of its first slots; charged first, the full rounds even that out (taken last, it lands on whatever those
// workgroups carry by then: modelled max / mean load of the smooth-mask lists' last layer at NB = 4 1.079 against 1.040 this way, block major 1.072).
__host__ __device__ inline int dcl_place_order(int it, int n, int W) { return n % W == 0 ? it : (it == 0 ? (n - 1) / W : it - 1); }
__host__ __device__ inline int dcl_max(const int *v, int n) { int m = 0; for (int i = 0; i < n; ++i) m = v[i] > m ? v[i] : m; return m; }

// internal entries (hidden visibility)
// need [B][12][H][W] and its diagonal-major copy need_d [B][12][H+W-1][H] (cell (y, x) at [(y + x) * H + y]; cells outside the image: -1),
// tile maxima tmax [B][12][nty][ntx] over the encode kernels' 4 x 16 tiles; all int8
int lic360_need_build(void *stream, const float *mask, int B, int G, int H, int W, signed char *need, signed char *need_d, signed char *tmax);
struct lic360_ec_lists {                   // encode order: compact lists of the live (sample, chunk of tiles, group block) tasks per layer and XCD
    int *list = nullptr;                   // [12][8][cap] entries u | tile mask << 28 in launch order
    int *cnt = nullptr;                    // [12][8]
    int cap = 0;
    int gbk = 16;                          // units per block of the encode kernels' task order: the builder numbers the tasks with it and the codec hands the same
                                           // field to the launchers that decode them (c16_fill_args).  16 measured best without lists (DESIGN 4.1 a)
};
int lic360_ec_lists_build(void *stream, const signed char *tmax, int B, int G, int H, int W, const lic360_ec_lists &l, unsigned long long *stats);
struct lic360_dc_lists {                   // decode order
    uint4 *list = nullptr;                 // [12][P][8][cap]
    int *cnt = nullptr;                    // [12][P][8]
    int cap = 0, P = 0;
    int nb = 1;                            // blocks per emission group (1: block major, the order of round 6)
    bool place = false;                    // the placement pass after the XCD balancing
    bool balance = true;                   // the XCD balancing pass
};
int lic360_dc_lists_build(void *stream, const signed char *need_d, int B, int G, int H, int W, const lic360_dc_lists &l, unsigned long long *stats);
