/* lic360_hip_gdn_grad.h -- C ABI of the one-pass GDN's backward, which liblic360_hip.so adds to include/lic360_hip.h and
 * include/lic360_hip_grad.h (each keeps its own table).  Same conventions: every entry returns 0 on success, 1 for a HIP failure, 2 for a
 * refused argument ("bad argument: ..." in lic360_last_error()); refusals come before anything is launched.  tools/gen_abi.py renders this
 * header into lic360/_abi_table_gdn_grad.py. */
#ifndef LIC360_HIP_GDN_GRAD_H
#define LIC360_HIP_GDN_GRAD_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- backward of lic360_gdn (csrc/gdn_grad_kernels.hip) ----
 * x, gy, gx [n][c][p] (p = h*w, contiguous), gamma, ggamma [c][c], beta, gbeta [c], all fp32 on the stream's device; gamma and beta are the
 * EFFECTIVE parameters, as in lic360_gdn.  With s_i = beta_i + sum_j gamma_ij x_j^2 (the forward's bits), n_i = sqrt(s_i):
 *     GDN     (inverse == 0, y = x / n):  t_i = (gy_i * (x_i / n_i)) / s_i,   gx_k = gy_k / n_k - x_k * sum_i gamma_ik t_i
 *     inverse (inverse != 0, y = x * n):  t_i = (gy_i * x_i) / n_i,           gx_k = gy_k * n_k + x_k * sum_i gamma_ik t_i
 *     ggamma_ij = -+1/2 sum over n, p of t_i x_j^2,   gbeta_i = -+1/2 sum over n, p of t_i      (- for GDN, + for the inverse)
 * every operation one fp32 rounding in the order written; the two parameter sums are split over workgroups whose fp32 partials go to
 * `scratch` and are added in a fixed order in double: no float atomics, the same bits on every call.  Every output is written completely.
 * gx == NULL skips gx; ggamma == gbeta == NULL skips the parameters (exactly one of the two NULL is refused); with all three NULL the call
 * does nothing and returns 0, also for n == 0.
 * c in {16, 32, 48, 64, 96, 128, 192}, any p >= 1.  x, gy and gx need no alignment beyond 4 bytes.
 * scratch: needed when the parameters are asked for; at least the bytes the query returns, 16-byte aligned; it holds the t-map [n][c][p]
 * and the splits' partials, and its contents mean nothing before or after the call.
 * Refused: null required pointers, an unsupported c, negative n or p, n or p == 0 while an output is asked for, scratch off a 16-byte
 * boundary, sizes whose tile count leaves int or whose element count leaves long. */
int lic360_gdn_backward(void *stream, const float *x, const float *gy, const float *gamma, const float *beta, float *gx, float *ggamma,
                        float *gbeta, void *scratch, int n, int c, long p, int inverse);
/* bytes of device scratch one call with these sizes needs; positive and non-decreasing in n and p; 0 for refused or empty arguments */
long lic360_gdn_backward_scratch_bytes(int n, int c, long p);

#ifdef __cplusplus
}
#endif
#endif
