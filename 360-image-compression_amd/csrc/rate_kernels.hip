// rate_kernels.hip -- the ideal code length of what the fused codecs would write, without running the coder (DESIGN.md "Rate estimation").
// Both codecs end their encode-order pass with one record (cdf[sym], cdf[sym + 1]) per symbol in coding order, (0, 0) for a symbol the coder skips.
// A coded symbol of frequency f = hi - lo in [1, 65536] costs
//     cost(f) = round(2^32 (16 - log2 f))                      Q32 bits, an unsigned 64-bit integer; cost(2^k) = (16 - k) 2^32 exactly
// and an image's code length is the INTEGER sum of its symbols' costs: the result does not depend on the order of the reduction, so it can be held
// bit for bit whatever the kernel's shape.  393 216 symbols of at most 16 * 2^32 each stay below 2^55.
//   * k_rate_sum: grid (chunks of RS_CHUNK records of an image, images), 256 threads.  A thread streams record pairs with 16-byte loads (one 8-byte
//     record first where the image's base is only 8-byte aligned -- odd n, every second image -- and one last where the chunk's tail is odd), looks the
//     cost up in the 65 537-entry table (512 KB: L2 resident) and keeps the total and the count of coded symbols in registers.  With a breakdown asked
//     for, the cost also goes to two LDS bins by 64-bit integer LDS atomics: the symbol's latitude row and its group.  Coding order runs along
//     anti-diagonals, so the lanes of a wave hold 64 different rows but one or two groups: the group bins are kept in up to 32 copies, one per lane of a
//     half wave (256 contiguous bytes per group: no two lanes of a half share an address or a bank), and summed when the chunk ends.  Then one wave
//     reduction of the total and one 64-bit integer global atomic per non-zero bin: at most 2 + G + H per workgroup of 8192 records.
//   No float atomics; integer sums only.
#include "rate.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace {
constexpr int RS_THREADS = 256, RS_CHUNK = 8192, RS_LDS_BYTES = 48 * 1024;
typedef unsigned long long u64;

// one struct by value: the number of arguments of a launch costs like their bytes do (DESIGN.md 4.1 b'')
struct RateArgs {
    const uint2 *rec;
    const unsigned *bkt;
    const u64 *table;
    u64 *bits, *nsym, *group, *row;
    long n;
    int G, H, gshift;
};

// The frequency of a record.  (0, 0) -- what the codecs' table kernels write for a symbol the coder skips -- is 0: entry 0 of the table, not counted.
// A record no table of this codec can give (hi < lo, hi - lo > 65536) is taken as uncoded too: the lookup stays inside the table whatever the buffer holds.
__device__ __forceinline__ unsigned rate_freq(uint2 r) {
    const unsigned f = r.y - r.x;
    return f > 65536u ? 0u : f;
}

template <bool BINS>
__global__ __launch_bounds__(RS_THREADS) void k_rate_sum(const RateArgs a) {
    extern __shared__ u64 s_bins[];                                    // BINS: [G << gshift] group bins (1 << gshift copies each), then [H] row bins
    __shared__ u64 s_tot[2];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long base = (long)b * a.n, lo = (long)blockIdx.x * RS_CHUNK, hi = a.n < lo + RS_CHUNK ? a.n : lo + RS_CHUNK;
    const int copies = 1 << a.gshift, rows0 = a.G << a.gshift;
    if (BINS)
        for (int i = tid; i < rows0 + a.H; i += RS_THREADS) s_bins[i] = 0;
    if (tid < 2) s_tot[tid] = 0;
    __syncthreads();
    u64 tot = 0;
    unsigned cnt = 0;
    const int copy = tid & (copies - 1);
    auto take = [&](uint2 r, unsigned k) __attribute__((always_inline)) {
        const unsigned f = rate_freq(r);
        const u64 c = a.table[f];
        tot += c;
        cnt += f != 0u;
        if (BINS && c) {
            atomicAdd(&s_bins[((k & 0xffffu) << a.gshift) + copy], c);
            atomicAdd(&s_bins[rows0 + (k >> 16)], c);
        }
    };
    const uint2 *r = a.rec + base;
    // lo and RS_CHUNK are even: a chunk starts on a 16-byte boundary exactly when its image does
    const int head = (int)((base + lo) & 1);
    const long m = hi - lo - head, npairs = m >> 1;
    if (head && tid == 0) take(r[lo], BINS ? a.bkt[lo] : 0u);
    if ((m & 1) && tid == 64) take(r[hi - 1], BINS ? a.bkt[hi - 1] : 0u);
#pragma unroll 4
    for (long j = tid; j < npairs; j += RS_THREADS) {
        const long k = lo + head + 2 * j;
        const uint4 v = *(const uint4 *)(r + k);
        uint2 q = make_uint2(0u, 0u);
        if (BINS) {
            if (!head) q = *(const uint2 *)(a.bkt + k);                // (k is even here)
            else q = make_uint2(a.bkt[k], a.bkt[k + 1]);
        }
        take(make_uint2(v.x, v.y), q.x);
        take(make_uint2(v.z, v.w), q.y);
    }
    for (int off = 32; off > 0; off >>= 1) {
        tot += __shfl_xor(tot, off);
        cnt += __shfl_xor(cnt, off);
    }
    if ((tid & 63) == 0) {
        atomicAdd(&s_tot[0], tot);
        atomicAdd(&s_tot[1], (u64)cnt);
    }
    __syncthreads();
    if (tid == 0 && s_tot[0]) atomicAdd(a.bits + b, s_tot[0]);
    if (tid == 1 && s_tot[1]) atomicAdd(a.nsym + b, s_tot[1]);
    if (BINS) {
        if (a.group)
            for (int g = tid; g < a.G; g += RS_THREADS) {
                u64 v = 0;
                for (int c = 0; c < copies; ++c) v += s_bins[(g << a.gshift) + ((c + tid) & (copies - 1))];   // (rotated: neighbouring threads start on different banks)
                if (v) atomicAdd(a.group + (long)b * a.G + g, v);
            }
        if (a.row)
            for (int h = tid; h < a.H; h += RS_THREADS) {
                const u64 v = s_bins[rows0 + h];
                if (v) atomicAdd(a.row + (long)b * a.H + h, v);
            }
    }
}

const std::vector<u64> &rate_table_host() {
    static const std::vector<u64> table = [] {
        std::vector<u64> t(RATE_TABLE_N, 0);
        for (int f = 1; f < RATE_TABLE_N; ++f) t[f] = (u64)std::floor(4294967296.0 * (16.0 - std::log2((double)f)) + 0.5);
        return t;
    }();
    return table;
}
}  // namespace

LIC360_API int lic360_rate_table(unsigned long long *out) {
    ARG_CHECK(out);
    memcpy(out, rate_table_host().data(), RATE_TABLE_N * sizeof(u64));
    return 0;
}

int lic360_rate_table_upload(DevBuf<unsigned long long> &out) {
    if (out.alloc(RATE_TABLE_N)) return 1;
    HIP_TRY(hipMemcpy(out, rate_table_host().data(), RATE_TABLE_N * sizeof(u64), hipMemcpyHostToDevice));
    return 0;
}

int lic360_rate_buckets_upload(int G, int H, int W, const int *pidx, const int *plane_start, DevBuf<unsigned> &out) {
    ARG_CHECK(G > 0 && G < 65536 && H > 0 && H < 65536 && W > 0 && pidx && (plane_start || G == 1));
    std::vector<unsigned> bkt((size_t)G * H * W);
    for (int g = 0; g < G; ++g)
        for (int th = 0; th < H; ++th)
            for (int tw = 0; tw < W; ++tw) {
                // the position k_enc_tables / k_imp_enc_tables write this symbol's record at
                const int s = th + tw, p = s + g, la = p >= G ? p - G + 1 : 0;
                const long k = (plane_start ? plane_start[p] + (pidx[s] - pidx[la]) : pidx[s]) + (th - (s >= W ? s - W + 1 : 0));
                if (k < 0 || k >= (long)bkt.size()) { lic360_set_error("internal: coding order leaves the latent"); return 1; }
                bkt[k] = (unsigned)g | (unsigned)th << 16;
            }
    if (out.alloc(bkt.size())) return 1;
    HIP_TRY(hipMemcpy(out, bkt.data(), bkt.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    return 0;
}

int lic360_rate_sum(hipStream_t s, const uint2 *rec, const unsigned *bkt, const unsigned long long *table, long n, int B, int G, int H,
                    unsigned long long *bits_q32, unsigned long long *nsym, unsigned long long *group_q32, unsigned long long *row_q32) {
    ARG_CHECK(rec && table && bits_q32 && nsym && n >= 0 && n < (1L << 40) && B > 0 && B <= 65535);
    const bool bins = group_q32 || row_q32;
    ARG_CHECK(!bins || (bkt && G > 0 && G < 65536 && H > 0 && H < 65536));
    int gshift = 5;
    while (bins && gshift > 0 && (((size_t)G << gshift) + H) * sizeof(u64) > RS_LDS_BYTES) --gshift;
    const size_t lds = bins ? (((size_t)G << gshift) + H) * sizeof(u64) : 0;
    ARG_CHECK(lds <= RS_LDS_BYTES);
    HIP_TRY(hipMemsetAsync(bits_q32, 0, (size_t)B * sizeof(u64), s));
    HIP_TRY(hipMemsetAsync(nsym, 0, (size_t)B * sizeof(u64), s));
    if (group_q32) HIP_TRY(hipMemsetAsync(group_q32, 0, (size_t)B * G * sizeof(u64), s));
    if (row_q32) HIP_TRY(hipMemsetAsync(row_q32, 0, (size_t)B * H * sizeof(u64), s));
    if (n == 0) return 0;
    const RateArgs a{rec, bkt, table, bits_q32, nsym, group_q32, row_q32, n, bins ? G : 0, bins ? H : 0, bins ? gshift : 0};
    const dim3 grid((unsigned)((n + RS_CHUNK - 1) / RS_CHUNK), (unsigned)B);
    if (bins) hipLaunchKernelGGL(k_rate_sum<true>, grid, dim3(RS_THREADS), lds, s, a);
    else hipLaunchKernelGGL(k_rate_sum<false>, grid, dim3(RS_THREADS), 0, s, a);
    LAUNCH_CHECK();
    return 0;
}
