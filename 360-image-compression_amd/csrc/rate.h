// rate.h -- the code-length reduction over a codec's (cdf[sym], cdf[sym + 1]) records (csrc/rate_kernels.hip) as the fused codecs call it.
#pragma once
#include "common.h"

#define RATE_TABLE_N 65537                     // cost of every frequency f = hi - lo in [0, 65536]; entry 0 (an uncoded record) = 0

// the table of lic360_rate_table (built once per process) on the device
int lic360_rate_table_upload(DevBuf<unsigned long long> &out);
// The side table of a codec: position k of its coding order -> group | latitude row << 16, the breakdown bins the record's cost goes to.  From the
// order lic360_code_contex gives (pidx: [h + w] first position of every diagonal) and, for the latent codec, the plane starts (plane_start:
// [g + h + w - 1] first position of every plane; null: one group, the positions in diagonal order).
int lic360_rate_buckets_upload(int G, int H, int W, const int *pidx, const int *plane_start, DevBuf<unsigned> &out);
// B images of n records each -> bits_q32[B], nsym[B] and, where given, group_q32[B][G], row_q32[B][H]; zeroes every output it is given, in the
// stream, before the launch.  bkt (the [n] side table; G, H its bin counts) is only read for a breakdown.
int lic360_rate_sum(hipStream_t s, const uint2 *rec, const unsigned *bkt, const unsigned long long *table, long n, int B, int G, int H,
                    unsigned long long *bits_q32, unsigned long long *nsym, unsigned long long *group_q32, unsigned long long *row_q32);
