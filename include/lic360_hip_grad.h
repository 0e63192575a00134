/* lic360_hip_grad.h -- C ABI of the training-side gradients that liblic360_hip.so adds to include/lic360_hip.h (which keeps its own table).
 * Same conventions: every entry returns 0 on success, 1 for a HIP failure, 2 for a refused argument ("bad argument: ..." in
 * lic360_last_error()); refusals come before anything is launched.  tools/gen_abi.py renders this header into lic360/_abi_table_grad.py. */
#ifndef LIC360_HIP_GRAD_H
#define LIC360_HIP_GRAD_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- weight gradient of the group-causal masked 5x5 convolution (csrc/cconv_wgrad_kernels.hip) ----
 * x [n, channel, h, w], gy [n, nout, h, w], gw [nout, channel, 5, 5], all fp32 contiguous NCHW on the stream's device:
 *     gw[oc, ic, th, tw] = sum over n, y, x of  gy[n, oc, y, x] * x[n, ic, y + th - 2, x + tw - 2]      (x is zero outside the map)
 * at the taps the mask rule keeps (cin = channel / ngroup, cout = nout / ngroup):
 *     th + tw + ic / cin <= oc / cout + 4  for constrain 6,  <  for constrain 5,
 * and +0.0 at every other tap: the whole tensor is written, no memset is owed by the caller.  The sum over n * h * w is split over
 * workgroups whose partial tiles go to `scratch` and are added in a fixed order: no float atomics, the same bits on every call.
 * scratch: at least the bytes the query returns, 16-byte aligned; its contents mean nothing before or after the call.
 * n == 0 is a no-op that touches nothing; h == 0 or w == 0 with n > 0 writes zeros.  Refused: null pointers, negative sizes, ngroup < 1,
 * ksz != 5, constrain outside {5, 6}, channel or nout not divisible by ngroup, sizes whose products leave the index types, scratch
 * that is not 16-byte aligned. */
int lic360_cconv_wgrad(void *stream, const float *x, const float *gy, float *gw, void *scratch, int n, int channel, int nout, int h, int w,
                       int ngroup, int ksz, int constrain);
/* bytes of device scratch one call with these sizes needs; non-decreasing in n, h and w; 0 for refused or empty arguments */
long lic360_cconv_wgrad_scratch_bytes(int n, int channel, int nout, int h, int w, int ngroup, int ksz, int constrain);

#ifdef __cplusplus
}
#endif
#endif
