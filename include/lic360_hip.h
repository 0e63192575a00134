/* lic360_hip.h -- C ABI of liblic360_hip.so, the MI355X (gfx950) implementation of the
 * LIC360 spherical-tiling + latent entropy-coding hot path.
 *
 * This is the drop-in boundary: each entry point replaces one method of a
 * class bound in the reference's pybind11 module `lic360` (extension/main.cpp:4-178).  The
 * citation after each declaration names the reference interface it replaces.  Conventions:
 *   - every pointer named *_dev / x / out ... is DEVICE memory (fp32, contiguous NCHW) unless
 *     the name says host; `stream` is the caller's hipStream_t passed as void* (the reference
 *     captured the ATen stream at construction, extension/base_opt.hpp:21-23);
 *   - plain C types only -- no torch / ATen types cross this boundary;
 *   - return value 0 = ok, non-zero = error; lic360_last_error() returns the message (the
 *     reference printed CUDA errors and carried on, extension/caffe_cuda_macro.h:21-33);
 *   - nothing here falls back to the CPU: if no HIP device is usable the call fails.
 */
#ifndef LIC360_HIP_H
#define LIC360_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char *lic360_last_error(void);
int lic360_version(void);

/* ---- A1-A3 sphere ops ------------------------------------------------------------------ */
/* SpherePadOp.forward, not in place          extension/sphere_pad_cuda.cu:67-105 (kernel :29-46) */
int lic360_sphere_pad(void *stream, const float *x, float *out, int nc, int h, int w, int pad);
/* SpherePadOp.forward, inplace=true          extension/sphere_pad_cuda.cu:48-65; hp,wp = padded dims */
int lic360_sphere_pad_inplace(void *stream, float *x, int nc, int hp, int wp, int pad);
/* SphereTrimOp.forward then SpherePadOp.forward(inplace) of the same width on the same tensor, as the reference's blocks run them back to back
 * (test/model_zoo.py:83-84,90-91,160-161): the refresh overwrites every cell the trim zeroed, so the pair is ONE pass over the apron */
int lic360_sphere_trim_pad_inplace(void *stream, float *x, int nc, int hp, int wp, int pad);
/* SphereTrimOp.forward                       extension/sphere_trim_cuda.cu:28-46 */
int lic360_sphere_trim(void *stream, float *x, int nc, int h, int w, int pad);
/* SphereCutEdgeOp.forward                    extension/sphere_cut_edge_cuda.cu:43-62 */
int lic360_sphere_cut_edge(void *stream, const float *x, float *out, int nc, int h, int w, int pad);
/* SpherePadOp.backward: gradient of the un-padded tensor [nc][h][w] from top_diff [nc][h+2p][w+2p]: own cell + wrap column + mirrored pole
 * row + pole corner, added in that order     extension/sphere_pad_cuda.cu:107-136,181-198
 * Both backward forms need 2 * pad <= h and 2 * pad <= w (that rule is the adjoint of the pad only there) and fail otherwise. */
int lic360_sphere_pad_backward(void *stream, float *in_diff, const float *top_diff, int nc, int h, int w, int pad);
/* SpherePadOp.backward, inplace=true: interior cells of diff [nc][hp][wp] accumulate their apron copies, the apron stays
 *                                            extension/sphere_pad_cuda.cu:138-180 */
int lic360_sphere_pad_backward_inplace(void *stream, float *diff, int nc, int hp, int wp, int pad);
/* SphereCutEdgeOp.backward: in_diff [nc][h][w] = top_diff [nc][h-2p][w-2p] inside a zero apron   extension/sphere_cut_edge_cuda.cu:63-96 */
int lic360_sphere_cut_edge_backward(void *stream, float *in_diff, const float *top_diff, int nc, int h, int w, int pad);
/* SphereLatScaleOp.forward / backward (same product)  extension/sphere_lat_scale_cuda.cu:40-58,69-87 */
int lic360_sphere_lat_scale(void *stream, const float *x, const float *weight, float *out, int nc, int h, int w, int npart);

/* ---- A4-A7, A18 pointwise ops ---------------------------------------------------------- */
/* ImpMapOp.forward (mask may be NULL)        extension/imp_map_cuda.cu:112-136 */
int lic360_imp_map(void *stream, const float *x, const float *imp, float *out, float *mask, int n, int c, int h, int w, int levels);
/* ImpMapOp constraint tensor top[1]          extension/imp_map_cuda.cu:27-71 (host computes, device write) */
int lic360_imp_map_constrain(void *stream, float *constrain, int n, int h, float rt, float scale_constrain);
/* alpha_t [h] of ImpMapOp: alpha / (|cos((0.5-(i+0.5)/h) pi)| / max * scale_weight + 1 - scale_weight) (host computes, device write)
 *                                            extension/imp_map_cuda.cu:27-36,49-52 */
int lic360_imp_map_alpha(void *stream, float *alpha_t, int h, float alpha, float scale_weight);
/* ImpMapOp.backward: data_diff [n,c,h,w] = top_diff under the mask floor(imp*levels); imp_diff [n,1,h,w] by rule imp_kernel 0..3
 * (kernels v1..v4), channel sums in ascending order; sphere_constrain [n,h], alpha_t [h]
 *                                            extension/imp_map_cuda.cu:138-298 */
int lic360_imp_map_backward(void *stream, const float *top_diff, const float *imp, const float *sphere_constrain, const float *alpha_t,
                            float *data_diff, float *imp_diff, int n, int c, int h, int w, int levels, int imp_kernel, float gamma);
/* Imp2maskOp.forward                         extension/imp2mask_cuda.cu:41-57 */
int lic360_imp2mask(void *stream, const float *x, float *out, int n, int c, int h, int w, int cpn);
/* MaskConstrainOp.forward / .backward (in place on a conv weight or its gradient [nout][channel][ksz][ksz]; constrain 5: taps with
 * tw + th + tc >= tn + ksz - 1 are zeroed, 6: tw + th + tc > tn + ksz - 1; tc / tn = input / output group)
 *                                            extension/mask_constrain_cuda.cu:17-41,47-91 */
int lic360_mask_constrain(void *stream, float *weight, int nout, int channel, int ksz, int ngroup, int constrain);
/* ScaleOp.forward                            extension/scale_cuda.cu:32-48 */
int lic360_scale(void *stream, const float *x, float *out, long count, float bias, float scale);
/* QuantOp.forward (train=false path); qidx may be NULL; wq_scratch/count are [c,levels] device buffers
 *                                            extension/quant_cuda.cu:136-169 */
int lic360_quant(void *stream, const float *x, const float *weight_b, float *wq_scratch, float *top, float *qidx, float *count,
                 int n, int c, int h, int w, int levels);
/* QuantOp training side.  update_weight: trailing levels without samples share one increment, an empty first level moves the first
 * centre, then the counts decay by weight_decay (in place on weight [c,levels] and ncount [c,levels])
 *                                            extension/quant_cuda.cu:87-133 */
int lic360_quant_update_weight(void *stream, float *weight, float *ncount, int c, int levels, float weight_decay);
/* QuantOp.backward: weight_diff [c,levels] = per-channel sums of (top_data - bottom_data) over the elements with index >= j (times the
 * level increment for j > 0; summed per workgroup in a fixed order, the reference uses float atomics), data_diff = top_diff0
 * (+ top_alpha * top_diff1 / beta when top_diff1 != NULL); qidx = the indices of the forward pass as floats, wq = its level increments
 *                                            extension/quant_cuda.cu:170-262 */
int lic360_quant_backward(void *stream, const float *top_diff0, const float *top_diff1, const float *bottom_data, const float *top_data,
                          const float *qidx, const float *wq, float *data_diff, float *weight_diff, int n, int c, int h, int w, int levels,
                          float top_alpha);
/* DquantOp.forward                           extension/dquant_cuda.cu:49-68 */
int lic360_dquant(void *stream, const float *x, const float *mask, const float *weight_b, float *wc_scratch, float *out,
                  int n, int c, int h, int w, int levels);
/* DtowOp.forward (d2w: pixel shuffle, else unshuffle)   extension/dtow_cuda.cu:77-102 */
int lic360_dtow(void *stream, const float *x, float *out, int n, int c, int h, int w, int stride, int d2w);

/* ---- A17 layout ops ---------------------------------------------------------------------- */
/* ContextReshapeOp.forward / backward(inverse=1)  extension/context_reshape_cuda.cu:42-60,74-92 */
int lic360_context_reshape(void *stream, const float *x, float *out, int n, int c, int h, int w, int ngroup, int inverse);
/* ContexShiftOp.forward (inv=0 zero-fills the skewed tensor first)  extension/contex_shift_cuda.cu:65-90 */
int lic360_contex_shift(void *stream, const float *x, float *out, int n, int c, int hin, int w, int cpn, int inv);

/* ---- A8 scan order ----------------------------------------------------------------------- */
/* CodeContexOp.forward: HOST tables idx[2*h*w], plane_idx[h+w]   extension/code_contex_cuda.cu:11-38 */
int lic360_code_contex(int h, int w, int *idx_host, int *plane_idx_host);
/* window [start,len) of plane psum in the scan order (extension/cconv_dc_cuda.cu:374-376); len 0 past the end */
int lic360_plane_window(int psum, int ngroup, int h, int w, const int *plane_idx_host, int *start, int *len);

/* ---- A11-A13 plane gather / scatter / add -------------------------------------------------- */
/* TileExtractOp.forward gather of plane psum -> out[n][len][cpn]   extension/tile_extract_cuda.cu:31-45,48-98 */
int lic360_tile_extract(void *stream, const float *x, float *out, int n, int c, int h, int w, int ngroup,
                        const int *idx_dev, int start, int len, int psum);
/* TileExtractOp.forward_batch (3 stacked nets, slab stride cpn*h*w*(n/3))  extension/tile_extract_cuda.cu:101-151 */
int lic360_tile_extract_batch(void *stream, const float *x, float *out, int n, int c, int h, int w, int ngroup,
                              const int *idx_dev, int start, int len, int psum);
/* TileInputOp.forward scatter of plane psum (already decremented) -> out[rep*n,g,h,w]  extension/tile_input_cuda.cu:27-76 */
int lic360_tile_input(void *stream, const float *sym, float *out, int n, int g, int h, int w, float bias, float scale, int rep,
                      const int *idx_dev, int start, int len, int psum);
/* TileAddOp.forward y += x on plane psum      extension/tile_add_cuda.cu:22-60 */
int lic360_tile_add(void *stream, float *y, const float *x, int n, int c, int h, int w, int ngroup,
                    const int *idx_dev, int start, int len, int psum);

/* ---- A14-A16 probability tables ------------------------------------------------------------ */
/* EntropyGmmTableOp.forward / forward_batch: w,d are rewritten in place (softmax, sigma floor);
 * out float[tn][nstep+1].  For forward_batch pass w=data, d=data+stride, m=data+2*stride.
 *                                            extension/entropy_gmm_table_cuda.cu:109-135,161-191 */
int lic360_gmm_table(void *stream, float *w, float *d, const float *m, float *out, int tn, int ng, int nstep,
                     float bias, float total, float beta);
/* EntropyTableOp.forward                     extension/entropy_table_cuda.cu:78-96 */
int lic360_entropy_table(void *stream, const float *logits, float *out, int count, int nstep, float total);
/* EntropyGmmOp.forward (loss + stored grads) / backward (scale stored grads by top_diff)
 *                                            extension/entropy_gmm_cuda.cu:71-91,108-124 */
int lic360_entropy_gmm(void *stream, const float *w, const float *d, const float *m, const float *label, float *loss,
                       float *wd, float *dd, float *md, float *ld, int count, int ng);
int lic360_entropy_gmm_backward(void *stream, float *wd, float *dd, float *md, float *ld, const float *top_diff, int count, int ng);

/* ---- A9/A10 group-causal masked convolution ------------------------------------------------ */
/* A plan holds the weight-independent schedule of one layer shape (term lists per 16-channel
 * output tile in the reference's 128-lane tree order) in host and device memory. */
typedef struct lic360_conv_plan lic360_conv_plan;
/* shape of CconvEcOp/CconvDcOp ctor (channel, ngroup, nout, kernel_size, constrain)  extension/cconv_ec.hpp:7-16 */
int lic360_conv_plan_create(int channel, int ngroup, int nout, int ksz, int constrain, lic360_conv_plan **plan);
void lic360_conv_plan_destroy(lic360_conv_plan *plan);
/* floats of packed weights per stacked net */
long lic360_conv_plan_packed_floats(const lic360_conv_plan *plan);
/* re-layout weight[nb][nout][channel][k][k] into MFMA A-fragments packed[nb][packed_floats] */
int lic360_conv_pack(void *stream, const lic360_conv_plan *plan, const float *weight, int nb, float *packed);
/* CconvEcOp.forward / forward_act / forward_batch / forward_act_batch (act NULL = no PReLU; nb = weight.size(0) or 1)
 *                                            extension/cconv_ec_cuda.cu:99-121,170-192,242-265,317-339 */
int lic360_cconv_ec(void *stream, const lic360_conv_plan *plan, const float *x, const float *packed, const float *bias,
                    const float *act, float *out, int n, int h, int w, int nb);
/* CconvDcOp.forward* for ONE plane psum: writes the plane's outputs into the persistent out[n,nout,h,w]
 * (caller zero-fills at psum==0 like :385).  plane_idx_dev = device copy of CodeContex's prefix table.
 *                                            extension/cconv_dc_cuda.cu:108-138,193-224,279-310,367-398 */
int lic360_cconv_dc_plane(void *stream, const lic360_conv_plan *plan, const float *x, const float *packed, const float *bias,
                          const float *act, float *out, int n, int h, int w, int nb,
                          const int *idx_dev, const int *plane_idx_dev, const int *plane_idx_host, int psum);

/* Extended forms used by the fused codec: `residual` (same layout as out, may be NULL) is added after the
 * activation (EntropyResidualBlock*: `conv2(conv1(x)) + x`, test/lic360_demo.py:29-41, extension/tile_add_cuda.cu:35);
 * x_mod < n lets the stacked nets share one input (the reference concatenates three copies, lic360_demo.py:131);
 * skewed != 0 selects the diagonal-major activation layout [n][c][th+tw][th] for x, residual and out. */
int lic360_cconv_ec_ex(void *stream, const lic360_conv_plan *plan, const float *x, const float *packed, const float *bias,
                       const float *act, const float *residual, float *out, int n, int h, int w, int nb, int x_mod);
int lic360_cconv_dc_plane_ex(void *stream, const lic360_conv_plan *plan, const float *x, const float *packed, const float *bias,
                             const float *act, const float *residual, float *out, int n, int h, int w, int nb,
                             const int *idx_dev, const int *plane_idx_dev, const int *plane_idx_host, int psum, int x_mod, int skewed);

/* Decode order, leaf-resident variant (v_mfma_f32_4x4x1, csrc/cconv4_kernels.hip + cconv4v6_dc.inc) for the latent-net shapes cin in {1,4},
 * cout <= 4, ngroup <= 64: replaces CconvDcOp.forward_act_batch / forward_batch of one plane (extension/cconv_dc_cuda.cu:313-398), same
 * results bit for bit as lic360_cconv_dc_plane, own weight layout.  Activations: zero-padded diagonal-major [n][c][rows][pitch] with cell
 * (s = th+tw, th) at [(s + row0) * pitch + th + col0] (lic360_dc4_layout; the padding must be zero).  Buffers are sized with
 * lic360_conv4_buffer_floats(0, planes, h, w) -- planes = samples x channels -- which includes the slack the 16-byte band fetches of the
 * last plane may touch (whole quads of 11-row bands, not clamped at the end of the tensor); the whole buffer starts zeroed. */
long lic360_conv4_buffer_floats(int layout, long planes, int h, int w);
int lic360_dc4_layout(int h, int w, int *rows, int *pitch, int *row0, int *col0);
int lic360_conv4_supported(const lic360_conv_plan *plan);
/* packed4: nb * lic360_conv4_packed_floats(plan) floats: per (net, output group) blocks of 4 KB in which the registers a wave needs for one
 * double step are adjacent per lane (one or two 16-byte loads per wave and double step) */
long lic360_conv4_packed_floats(const lic360_conv_plan *plan);
int lic360_conv4_pack(void *stream, const lic360_conv_plan *plan, const float *weight, int nb, float *packed4);
int lic360_cconv4_dc_plane(void *stream, const lic360_conv_plan *plan, const float *x, const float *packed4, const float *bias,
                           const float *act, const float *residual, float *out, int n, int h, int w, int nb, int psum, int x_mod);
/* Host-only (no GPU work): the sample packing lic360_cconv4_dc_plane uses on plane psum for a layer of ngroup groups (cin = 4: hidden / last
 * layers, 1: first layer) over n samples of nb nets -- "tape" packing: the row windows of *tape_c consecutive samples of an XCD's list laid end to
 * end over the 64 lanes of nwaves[j] tasks per group block j (a window may be cut between two tasks).  *tape_c = 0: one sample per task on this
 * plane.  blocks[j] = first group of block j (launch order); windows[(j * 6 + t) * 3 + i] = piece i of task t of a tape:
 * k | slo << 3 | shi << 9 | a0 << 15 | 1 << 21 (sample k of the tape stores rows slo..shi from lanes a0..; 0 = none).  Arrays of 24, 24 and
 * 24 * 6 * 3 entries (the launch itself carries only where each task of a tape starts; the pieces follow from one rule on both sides).  For tests of the packing rules (tests/test_dc_tape.py). */
int lic360_dc4_tape_layout(int ngroup, int cin, int n, int nb, int h, int w, int psum, int x_mod, int *tape_c, int *n_blocks, int *blocks,
                           int *nwaves, unsigned *windows);

/* Encode-order variant on v_mfma_f32_16x16x4_f32 (csrc/cconv16_kernels.hip): rows = 4 consecutive groups x 4 output channels, K = 4
 * consecutive input groups of a lane's chain; same results bit for bit as lic360_cconv_ec (extension/cconv_ec_cuda.cu:271-331).
 * Shapes: cin in {1,4}, cout <= 4 (the latent nets).  Activations are zero-haloed NCHW planes [n][c][hp][wp], cell (r, c) at
 * [(r+2)*wp + c+2] (lic360_ec16_layout: hp = 4*ceil(h/4)+4, wp = 16*ceil(w/16)+4); halo and round-up cells must be zero
 * and are never written.  ctr: 8 ints of device scratch (per-XCD task counters, zeroed on the stream by the call). */
int lic360_ec16_layout(int h, int w, int *hp, int *wp);
int lic360_conv16_supported(const lic360_conv_plan *plan);
long lic360_conv16_packed_floats(const lic360_conv_plan *plan);
int lic360_conv16_pack(void *stream, const lic360_conv_plan *plan, const float *weight, int nb, float *packed16);
/* the weight layout lic360_cconv16_ec_tables reads (cin = 4, cout = 3): five groups per block, MFMA row = 3 (group in block) + channel,
 * so that 15 of 16 MFMA rows carry an output; fits a lic360_conv16_packed_floats allocation */
int lic360_conv16_pack_tables(void *stream, const lic360_conv_plan *plan, const float *weight, int nb, float *packed16);
int lic360_cconv16_ec(void *stream, const lic360_conv_plan *plan, const float *x, const float *packed16, const float *bias,
                      const float *act, const float *residual, float *out, int n, int h, int w, int nb, int x_mod, int *ctr);

/* Last layer of the latent entropy model with the CDF-table build fused into its epilogue (SURVEY.md §7 k_cconv_ec_last_gmm;
 * replaces the last CconvEcBatch.forward + TileExtractBatch + EntropyBatchGmmTable.forward_batch of
 * test/lic360_demo.py:132-140, extension/entropy_gmm_table_cuda.cu:138-191): x = activations of the three stacked nets
 * [weight, sigma, mu], [3*images][C][hp][wp] net-major in the lic360_ec16_layout; code / mask [images, G, h, w]; pidx_dev /
 * plane_start_dev = device copies of CodeContex's prefix table [h+w] and of the index of each plane's first record
 * [h+w+G-1]; rec = uint32 pairs [images][G*h*w] (cdf[sym], cdf[sym+1]) in coding order, (0,0) where masked.
 * packed16: from lic360_conv16_pack_tables (NOT lic360_conv16_pack). */
int lic360_cconv16_ec_tables(void *stream, const lic360_conv_plan *plan, const float *x, const float *packed16, const float *bias,
                             const float *code, const float *mask, const int *pidx_dev, const int *plane_start_dev,
                             void *rec, int images, int h, int w, int *ctr);

/* The importance-map net's hidden / last layers (one group, C = 144, constrain 6: test/lic360_demo.py:153-161, 254-262) on
 * v_mfma_f32_16x16x4_f32 (csrc/cconv144_kernels.hip): same results bit for bit as lic360_cconv_ec / lic360_cconv_dc_plane.
 * Encode order: x = zero-haloed NCHW planes [n][144][hp][wp] (lic360_ec144_layout, cell (r, c) at [(r+2)*wp + c+2]); out /
 * residual = [n][nout] planes with stride oplane, rows of opitch floats, cell (r, c) at [(r+ooff)*opitch + c+ooff] (ooff 2 =
 * the same haloed layout, 0 = plain NCHW).  Decode order (plane = anti-diagonal s of every map): x / residual / out are
 * zero-padded diagonal-major planes [n][c][rows][pitch] (lic360_dc144_layout), cell (th, tw) at [(th+tw+4)*pitch + th+2]. */
int lic360_conv144_supported(const lic360_conv_plan *plan);
long lic360_conv144_packed_floats(const lic360_conv_plan *plan);
int lic360_conv144_pack(void *stream, const lic360_conv_plan *plan, const float *weight, float *packed144);
int lic360_ec144_layout(int h, int w, int *hp, int *wp);
int lic360_cconv144_ec(void *stream, const lic360_conv_plan *plan, const float *x, const float *packed144, const float *bias,
                       const float *act, const float *residual, float *out, int n, int h, int w, long oplane, int opitch, int ooff);
int lic360_dc144_layout(int h, int w, int *rows, int *pitch);
int lic360_cconv144_dc_plane(void *stream, const lic360_conv_plan *plan, const float *x, const float *packed144, const float *bias,
                             const float *act, const float *residual, float *out, int n, int h, int w, int s);

/* ---- A19/A20 arithmetic coder (host side, as in the reference) ----------------------------- */
/* Coder operates on HOST int32 tables exactly like the reference's Coder (extension/coder.h:10-63,
 * extension/coder.cpp:30-113): the op API hands it CPU tensors. */
typedef struct lic360_coder lic360_coder;
lic360_coder *lic360_coder_enc_open(void);                                   /* Coder::start_encoder  coder.h:15-21 */
int lic360_coder_encode_slice(lic360_coder *c, const int *table, int ncode, const int *label, const float *mask, int num);
                                                                             /* encodes / encodes_mask coder.cpp:30-48,70-89 */
long lic360_coder_enc_finish(lic360_coder *c);                               /* Coder::end_encoder    coder.h:22-26 */
const uint8_t *lic360_coder_bytes(const lic360_coder *c);
lic360_coder *lic360_coder_dec_open(const uint8_t *bytes, long n);           /* Coder::start_decoder  coder.h:30-35 */
int lic360_coder_decode_slice(lic360_coder *c, const int *table, int ncode, const float *mask, float file_value, float *out, int num);
                                                                             /* decodes / decodes_mask coder.cpp:49-69,90-113 */
void lic360_coder_close(lic360_coder *c);

/* ---- D1/D2 device-resident latent codec ------------------------------------------------------- */
/* One object per (ngroup, h, w) entropy-domain shape and GPU; replaces EntEncoderFast / EntDecoder
 * (test/lic360_demo.py:95-141,191-238) for batches of up to max_batch images.  All pointers are device
 * memory; bitstreams live in HBM as bytes[b*cap .. b*cap+nbytes[b]) and are byte-identical to what
 * Coder::end_encoder would have written to `<code>` (extension/coder.h:22-26). */
typedef struct lic360_codec lic360_codec;
int lic360_codec_create(int ngroup, int h, int w, int max_batch, lic360_codec **codec);
void lic360_codec_destroy(lic360_codec *codec);
/* layer 0..11 of the 3 stacked nets [weight, sigma, mu]: weight [3,nout,cin_total,5,5], bias/act [3,nout]
 * (act NULL for layer 11) -- the tensors cast_entropy_parameter fills (test/lic360_demo.py:296-311) */
int lic360_codec_set_layer(void *stream, lic360_codec *codec, int layer, const float *weight, const float *bias, const float *act);
/* code/mask [b,ngroup,h,w] fp32 (symbols 0..7, mask 0/1) -> bitstreams; err[b] != 0 flags a coder fault or cap overflow */
int lic360_codec_encode(void *stream, lic360_codec *codec, const float *code, const float *mask, int b,
                        uint8_t *bytes, long cap, int *nbytes, int *err);
/* bitstreams + mask -> code_out [b,ngroup,h,w] (decoded symbol where mask, 0 elsewhere: `b[0:1] + 3.5*mask`, lic360_demo.py:236-237) */
int lic360_codec_decode(void *stream, lic360_codec *codec, const uint8_t *bytes, long cap, const int *nbytes,
                        const float *mask, int b, float *code_out, int *err);
/* Device-resident importance-map stream (ImpEntEncoderFast / ImpEntDecoder, test/lic360_demo.py:143-189, 241-290): one
 * group, 12 spatially causal layers with `hidden_channels` channels, nsym-way softmax tables (entropy_table_cuda.cu:24-96),
 * symbols = importance levels.  levels / levels_out: float [B,1,h,w]; weights per layer as [nout][C][5][5] (one net).
 * Bitstream buffers as in lic360_codec_encode / _decode. */
typedef struct lic360_impcodec lic360_impcodec;
int lic360_impcodec_create(int h, int w, int hidden_channels, int nsym, int max_batch, lic360_impcodec **out);
void lic360_impcodec_destroy(lic360_impcodec *c);
int lic360_impcodec_set_layer(void *stream, lic360_impcodec *c, int layer, const float *weight, const float *bias, const float *act);
int lic360_impcodec_encode(void *stream, lic360_impcodec *c, const float *levels, int B, uint8_t *bytes, long cap, int *nbytes, int *err);
int lic360_impcodec_decode(void *stream, lic360_impcodec *c, const uint8_t *bytes, long cap, const int *nbytes, int B, float *levels_out, int *err);
/* The map's decode AND the latent codec's mask, plane by plane: after plane p, mask_out = Dtow(stride)(Imp2mask(levels_out)) -- the
 * last three lines of ImpEntDecoder.forward (test/lic360_demo.py:283-287) -- is refreshed and the codec-owned event p is recorded,
 * so that lic360_codec_decode_gated on ANOTHER stream runs behind the map's decode instead of after it.  mask_out:
 * [B][mask_c / stride^2][stride h][stride w] (LIC360: mask_c = 192, stride = 2); *generation_out: the ticket of this masked decode.
 * ORDERING CONTRACT: (1) the events are re-recorded by every call, so the gated latent decode of a step must be enqueued AFTER this call
 * of the same step (enforced: the ticket); (2) the next step's masked decode overwrites mask_out -- order it after the latent decode
 * that still reads the buffer (an event on the latent stream, or alternate between two mask buffers as bench.py does). */
int lic360_impcodec_decode_masked(void *stream, lic360_impcodec *c, const uint8_t *bytes, long cap, const int *nbytes, int B,
                                  float *levels_out, int *err, float *mask_out, int mask_c, int stride, long *generation_out);
/* lic360_codec_decode behind that map decode: the convolutions of a latent plane read no mask; the plane's table kernel waits for the
 * map codec's event min(P - 1, plane / stride).  Same results as lic360_codec_decode on the finished mask.  `generation` must be the
 * ticket of map_codec's LATEST lic360_impcodec_decode_masked into this very `mask`, not yet used: anything else (a gate of an earlier
 * step, a gate used twice, the latent decode enqueued first) returns an error instead of decoding against a stale mask.  map_codec
 * must outlive the call.  No reference counterpart: EntDecoder.forward takes the finished mask (test/lic360_demo.py:218-238); this
 * only moves the 18 ms of a map's decode under the 97 ms of the latent's. */
int lic360_codec_decode_gated(void *stream, lic360_codec *codec, const uint8_t *bytes, long cap, const int *nbytes,
                              const float *mask, int b, float *code_out, int *err, lic360_impcodec *map_codec, long generation);

/* ---- f3 viewport projection (ProjectsOp, the sampling stage of VPSNR / VSSIM) -------------------------------------------------
 * Sampling coordinates tf [14][h_out*w_out][2] = (x, y) in ERP pixels of the 14 rectilinear viewports (yaw theta*pi, pitch phi*pi, field
 * of view fov*pi) on an ERP of height x width; host computes in fp32, device write
 *                                            extension/projects.hpp:8-20, projects_cuda.cu:7-67,101-153 */
int lic360_projects_tf(void *stream, float *tf_dev, int h_out, int w_out, const float *theta14, const float *phi14, float fov,
                       int height, int width);
/* 1 when every index the sampling of lic360_projects_forward / lic360_viewport_quality forms from the table of these arguments lies inside one
 * ERP plane [height][width], 0 when one does not, -1 on bad arguments.  Host arithmetic only (no device, no stream).  A viewport with a row that
 * looks exactly at a pole -- a square viewport of fov 0.5 in the views pitched by 45 degrees -- has an undefined longitude there: the reference's
 * table (and this one) then leaves [0, width - 1], and the sampling kernels, which trust the table as the reference's do, read outside x. */
int lic360_projects_tf_inside(int h_out, int w_out, const float *theta14, const float *phi14, float fov, int height, int width, int nearest);
/* ProjectsOp.forward: x [nc][h][w] -> out [14][nc][h_out][w_out] (viewport-major), bilinear or nearest
 *                                            extension/projects_cuda.cu:181-232 */
int lic360_projects_forward(void *stream, const float *x, const float *tf, float *out, int nc, int h, int w, int h_out, int w_out, int nearest);
/* ProjectsOp.backward: scatter-add of the viewport gradients (in_diff) and of their interpolation weights (count), both [nc][h][w]
 *                                            extension/projects_cuda.cu:234-329 */
int lic360_projects_backward(void *stream, const float *top_diff, const float *tf, float *in_diff, float *count, int nc, int h, int w,
                             int h_out, int w_out, int nearest);

/* Fused viewport metrics (no reference kernel: the evaluation mode of test/lic360_demo.py:406-449 projects both images with ProjectsOp and
 * runs lic360_operator/pytorch_ssim.py and an MSE on the views).  a, b [n][c][h][w] fp32 ERP batches; tf the table of lic360_projects_tf for
 * (h_out, w_out) on an h x w ERP; taps: `window` floats in HOST memory, the normalised 1-D window (window odd, at most 11; the 2-D window is
 * their outer product, applied as a row pass and a column pass with zero padding).  mse, ssim [n][14] fp32 (device): per image and viewport,
 * the mean over c*h_out*w_out cells of (a - b)^2 and of the SSIM map, summed in double in a fixed order (no atomics: bit-reproducible).
 * ssim_map: NULL, or [14][n][c][h_out][w_out] fp32 (the layout of lic360_projects_forward's output) for the per-cell SSIM.  scratch:
 * lic360_viewport_quality_scratch_bytes(n, h_out, w_out) bytes of device memory, 16-byte aligned, fully written before it is read (the
 * query returns 0 for arguments the launch refuses).  The outputs, the map and the scratch must not overlap.  The samples are bit for
 * bit those of lic360_projects_forward, and like it this entry trusts tf: a table for which lic360_projects_tf_inside returns 0 makes it
 * read outside a and b (the Python shim asks and refuses). */
long lic360_viewport_quality_scratch_bytes(int n, int h_out, int w_out);
int lic360_viewport_quality(void *stream, const float *a, const float *b, const float *tf, int n, int c, int h, int w, int h_out, int w_out,
                            int nearest, const float *taps, int window, void *scratch, float *mse, float *ssim, float *ssim_map);
/* The differentiable form of the fused viewport metrics, in two launches.  lic360_viewport_quality_coef: the arguments, checks and mse / ssim (bit
 * for bit) of lic360_viewport_quality without the map; it also stores, per view cell, the derivatives of the cell's SSIM with respect to its five
 * window sums: coef_q (E_aa and E_bb), coef_r (E_ab), coef_pa (mu_a), coef_pb (mu_b), each [14][n][c][h_out][w_out] fp32.  coef_q and coef_r are
 * required, and at least one of coef_pa / coef_pb (the sides that will be differentiated); all buffers must be disjoint.
 * lic360_viewport_quality_backward: from a, b, tf, taps of that call, its maps and the upstream gradients grad_mse, grad_ssim [n][14] (device), the
 * gradients grad_a / grad_b [n][c][h][w] of the ERP batches.  At least one of grad_a / grad_b; coef_pa is required exactly when grad_a is given,
 * coef_pb when grad_b is.  The entry zeroes grad_a / grad_b in the stream, then adds with float atomics (their last bits can differ from run to
 * run).  grad_views_a / grad_views_b: NULL, or [14][n][c][h_out][w_out] for the gradients of the projected views before the scatter (a side's
 * views need that side's grad; these are bit-reproducible).  Nothing written may overlap anything read or written.
 * Both refuse (2) before anything is launched, and both trust tf as lic360_viewport_quality does. */
int lic360_viewport_quality_coef(void *stream, const float *a, const float *b, const float *tf, int n, int c, int h, int w, int h_out, int w_out,
                                 int nearest, const float *taps, int window, void *scratch, float *mse, float *ssim, float *coef_pa,
                                 float *coef_pb, float *coef_q, float *coef_r);
int lic360_viewport_quality_backward(void *stream, const float *a, const float *b, const float *tf, int n, int c, int h, int w, int h_out,
                                     int w_out, int nearest, const float *taps, int window, const float *coef_pa, const float *coef_pb,
                                     const float *coef_q, const float *coef_r, const float *grad_mse, const float *grad_ssim, float *grad_a,
                                     float *grad_b, float *grad_views_a, float *grad_views_b);

/* Fused GMM rate loss (no reference kernel: the reference's training objective, train/EntropyNet2.py:67-74 and train/model_zoo.py:295-296, runs
 * ContextReshape x 3, softmax, ReLU + 1e-5, EntropyGmm, a product with the mask and a sum).  logit, sigma, mean [n][g*ng][h][w] fp32: the raw
 * outputs of the three nets; label [n][g][h][w]; mask [n][g][h][w] or NULL (every symbol coded).  Symbol (n, g, y, x) reads channel g*ng + i of
 * each net, i < ng, and is coded iff mask >= 0.5.  A coded symbol's loss is lic360_entropy_gmm's, bit for bit, of
 * (lic360 softmax of the logits, sigma > 0 ? sigma + 1e-5f : 1e-5f, mean, label); an uncoded symbol costs 0, counts as no symbol and gets exact
 * zeros in every gradient whatever its parameters hold.  nats [n] double (device): the coded symbols' fp32 losses added in double in a fixed
 * order (no atomics: the same bits on every call); symbols [n] int64 (device): their count; map: NULL or [n][g][h][w] fp32, the per-symbol loss,
 * 0 where uncoded.  scratch: lic360_gmm_rate_scratch_bytes(n, g, h, w) bytes of device memory, 8-byte aligned, fully written before it is read
 * (the query returns 0 for arguments the launch refuses or that hold no symbol).
 * lic360_gmm_rate_backward: with t = grad_nats[n] (device, fp32), d_logit, d_sigma, d_mean [n][g*ng][h][w] and, unless NULL, d_label
 * [n][g][h][w], recomputed from the inputs: d_mean = md t, d_sigma = sigma > 0 ? dd t : 0, d_label = ld t, d_logit_i = w_i (wd_i t - dot),
 * dot = sum_i fmaf(wd_i t, w_i, dot) in index order, with wd, dd, md, ld lic360_entropy_gmm's.  Every output element is written by every call.
 * Nothing written may overlap anything read.  Both refuse (2) before anything is launched: a negative dimension, ng outside 1..16, a null
 * pointer, a product of the dimensions that leaves the kernels' index types.  n*g*h*w == 0 is no error and launches nothing (pointers may then
 * be NULL; with n > 0, nats and symbols are zeroed in the stream). */
long lic360_gmm_rate_scratch_bytes(int n, int g, int h, int w);
int lic360_gmm_rate(void *stream, const float *logit, const float *sigma, const float *mean, const float *label, const float *mask, int n, int g,
                    int h, int w, int ng, double *nats, long long *symbols, float *map, void *scratch);
int lic360_gmm_rate_backward(void *stream, const float *logit, const float *sigma, const float *mean, const float *label, const float *mask,
                             const float *grad_nats, int n, int g, int h, int w, int ng, float *d_logit, float *d_sigma, float *d_mean,
                             float *d_label);

/* Fused cross-entropy rate loss (no reference kernel: the importance map's entropy model, test/model_zoo.py:275-300, runs ContextReshape and
 * CrossEntropyLoss over nvalue + 1 classes).  logit [n][g*k][h][w] fp32: the net's raw output; label [n][g][h][w] fp32 holding class indices.
 * Symbol (n, g, y, x) reads channel g*k + i, i < k (1 <= k <= 64), and is valid iff label > -1.0f && label < (float)k (so NaN is invalid); its
 * class is c = (int)label, truncated (-0.5 -> 0, 3.7 -> 3).  A valid symbol, every operation rounded once in fp32 and nothing contracted:
 *   m = l_0; for i = 1..k-1: if (m < l_i) m = l_i;   e_i = lic360_expf(l_i - m);   s = 0.0f; s = s + e_i in index order;
 *   loss = lic360_logf(s) - (l_c - m).
 * An invalid symbol costs 0, is counted in invalid[n] and not in symbols[n], and gets exact zeros in d_logit whatever its logits hold.
 * nats [n] double (device): the valid symbols' fp32 losses added in double in a fixed order (no atomics: the same bits on every call); symbols,
 * invalid [n] int64 (device): the counts; map: NULL or [n][g][h][w] fp32, the per-symbol loss, 0 where invalid.  scratch:
 * lic360_ce_rate_scratch_bytes(n, g, h, w) bytes of device memory, 8-byte aligned, fully written before it is read (the query returns 0 for
 * arguments the launch refuses or that hold no symbol; it does not know k and answers for k = 64, so for n*g*h*w above 2^60 / 64 elements it
 * returns 0 where a launch with a smaller k would still be accepted).
 * lic360_ce_rate_backward: with t = grad_nats[n] (device, fp32), d_logit [n][g*k][h][w] recomputed from the inputs: p_i = e_i / s,
 * d_logit_i = (i == c ? p_i - 1.0f : p_i) * t.  Every element of d_logit is written by every call.
 * Nothing written may overlap anything read.  Both refuse (2) before anything is launched: a negative dimension, k outside 1..64, a null
 * pointer, a product of the dimensions that leaves the kernels' index types.  n*g*h*w == 0 is no error and launches nothing (pointers may then
 * be NULL; with n > 0, nats, symbols and invalid are zeroed in the stream). */
long lic360_ce_rate_scratch_bytes(int n, int g, int h, int w);
int lic360_ce_rate(void *stream, const float *logit, const float *label, int n, int g, int h, int w, int k, double *nats, long long *symbols,
                   long long *invalid, float *map, void *scratch);
int lic360_ce_rate_backward(void *stream, const float *logit, const float *label, const float *grad_nats, int n, int g, int h, int w, int k,
                            float *d_logit);

/* CppOp: ERP -> Craster parabolic projection.  lic360_cpp_rows fills the per-row column window ws [h][2] = (first column, count) and the
 * row angle theta [h] (host computes, device write); lic360_cpp_forward resamples x [nc][h][w] row by row, zero outside the window; mask
 * (may be NULL) gets 1 inside / 0 outside     extension/CPP.hpp:6-11, CPP_cuda.cu:11-22,46-122 */
int lic360_cpp_rows(void *stream, int *ws_dev, float *theta_dev, int h, int w);
int lic360_cpp_forward(void *stream, const float *x, float *out, float *mask, const int *ws_dev, const float *theta_dev, int nc, int h, int w);

/* ViewportOp: one rectilinear viewport per sample looking at theta_phi [n,2] (radians, device), field of view fov_deg.
 * cal_rota_matrix -> rota [n,9]; forward -> out [n,c,ho,wo], rays0 / rays [n,ho,wo,3] (camera frame / rotated), tf [n,ho,wo,2] = (longitude,
 * latitude) of every viewport pixel; get_viewport_xy -> where the directions theta_phi_next fall in the current viewports, in pixels
 *                                            extension/viewport.hpp:7-13, viewport_cuda.cu:8-289 (its backward returns nothing) */
int lic360_viewport_rota(void *stream, const float *theta_phi, float *rota, int n);
int lic360_viewport_forward(void *stream, const float *x, const float *theta_phi, float *out, float *rays0, float *rota, float *rays, float *tf,
                            int n, int c, int h, int w, int ho, int wo, float fov_deg);
int lic360_viewport_xy(void *stream, const float *theta_phi_next, const float *rota, float *xy, int n, int ho, int wo, float fov_deg);

/* ---- f1 generalised divisive normalisation, one pass (the reference's GDN is four torch kernels: lic360_operator/GDN.py:66-100) ------
 * out[n,i,p] = x / sqrt(beta[i] + sum_j gamma[i,j] x[n,j,p]^2)   (inverse != 0: x * sqrt(...)); x / out [n][c][p] contiguous,
 * gamma [c][c] and beta [c] are the effective (reparametrised) parameters; c in {16,32,48,64,96,128,192}; j summed in ascending order */
int lic360_gdn(void *stream, const float *x, const float *gamma, const float *beta, float *out, int n, int c, long p, int inverse);
/* ---- the split-bf16 ("bf16x3") form of lic360_gdn (csrc/gdn_bf16x3.inc, kernel k_gdn_b3), opt-in: the same operation, operands and output contract
 * (x / out [n][c][p] contiguous on 4-byte boundaries, any p, nothing outside out written).  sq = x * x in fp32; sq and the effective gamma are each split
 * into hi = bf16(v) and lo = bf16(v - hi) (round to nearest even); each product is g_hi sq_hi + g_hi sq_lo + g_lo sq_hi on v_mfma_f32_16x16x32_bf16 with
 * fp32 accumulation; sqrtf, the division (or product) and beta stay fp32 on the unrounded x.  2^-15 relative per element against the float64 GDN for
 * gamma >= 0 (a negative gamma: relative to sum |gamma| x^2); NaN, infinity and squares that overflow fp32 are outside the contract.  c in
 * {32,64,96,128,192}; packed = lic360_gdn_bf16x3_pack of the effective gamma [c][c] (packed_bytes = 4 c c bytes, 16-byte aligned: hi and lo bf16
 * parts in the waves' A-operand order).  Refused before any launch: null operands, n <= 0, n > 65535, p <= 0, an unsupported c, a misaligned pack. */
int lic360_gdn_bf16x3_supported(int c);
long lic360_gdn_bf16x3_packed_bytes(int c);
int lic360_gdn_bf16x3_pack(void *stream, const float *gamma, void *packed, int c);
int lic360_gdn_bf16x3(void *stream, const float *x, const void *packed, const float *beta, float *out, int n, int c, long p, int inverse);

/* ---- f1 3x3 stride-1 convolution on sphere-apron maps with the apron read BY INDEX in the tile loader and bias + PReLU + residual in the
 * epilogue (csrc/conv3x3_kernels.hip): replaces, per layer, nn.Conv2d(c, c', 3, 1, 1 | 0) + the in-place SpherePad in front of it + the
 * nn.PReLU + SphereTrim (+ residual add) behind it in test/model_zoo.py:8-23,45-62,64-94,144-169 (sphere rule: extension/sphere_pad_cuda.cu:48-65).
 * x [n][cin][hp][wp]; sphere = 1: only the interior (pad cells in from every edge) is read, apron cells come from the interior by the sphere
 * rule; sphere = 2: longitude wrap only (columns of the apron come from the interior, rows are read as they are: the input is the 1-ring output
 * of another launch, whose wrapped columns need not be computed twice); sphere = 0: read as it is.
 * out [n][cout][hp - 2 crop][wp - 2 crop]: the cells of rows [ring, hp - ring) x columns [ring_w, wp - ring_w) of the input grid are
 * written (out = conv + bias; PReLU if slope; + residual [n][cout][hp][wp] if given), the others are NOT touched (SphereTrim(ring) = leave or
 * zero them: lic360_sphere_trim / lic360_sphere_apron_from).  crop = 1 is the unpadded nn.Conv2d(.., 3, 1) of ResidualBlockUp.conv1;
 * shuffle != 0 stores through Dtow(2, d2w) (extension/dtow_cuda.cu:38-75): out [n][cout / 4][2 (hp - 2 crop)][2 (wp - 2 crop)], channel 4 p + v of a
 * cell (y, x) at channel p, cell (2 y + v / 2, 2 x + v % 2) -- the conv -> PReLU -> Dtow chain of test/model_zoo.py:160-162 in one launch.
 * fp32 MFMA, this kernel's own summation order (1e-4 against a library convolution).  cin % 16 == 0, cout in {96} or a multiple of 192;
 * packed = lic360_sconv3x3_pack of the [cout][cin][3][3] weight; bias / slope 16-byte aligned. */
int lic360_sconv3x3_supported(int cin, int cout);
long lic360_sconv3x3_packed_floats(int cin, int cout);
int lic360_sconv3x3_pack(void *stream, const float *weight, float *packed, int cin, int cout);
int lic360_sconv3x3(void *stream, const float *x, const float *packed, const float *bias, const float *slope, const float *residual, float *out,
                    int n, int cin, int cout, int hp, int wp, int pad, int sphere, int ring, int ring_w, int crop, int shuffle);
/* the transforms' 1x1 layers on the same kernel body (K = input channels only): replaces nn.Conv2d(c, c', 1) + nn.PReLU (+ residual add) of
 * test/model_zoo.py:8-23 (ResidualBlock.conv1 / conv3) and, with crop = 1 and shuffle != 0, SphereCutEdge(1) + nn.Conv2d(c, 4c, 1) + Dtow(2) (+ add) of
 * the shortcut of ResidualBlockUp (test/model_zoo.py:165-168).  x [n][cin][hp][wp]; out (and residual) [n][cout][hp - 2 crop][wp - 2 crop], or shuffled
 * [n][cout / 4][2 (hp - 2 crop)][2 (wp - 2 crop)]; the cells of rows [ring, hp - ring) x columns [ring_w, wp - ring_w) of the input grid are written, the
 * others not touched; cin % 32 == 0, cout = 96 or a multiple of 192 */
int lic360_sconv1x1_supported(int cin, int cout);
long lic360_sconv1x1_packed_floats(int cin, int cout);
int lic360_sconv1x1_pack(void *stream, const float *weight, float *packed, int cin, int cout);
int lic360_sconv1x1(void *stream, const float *x, const float *packed, const float *bias, const float *slope, const float *residual, float *out,
                    int n, int cin, int cout, int hp, int wp, int ring, int ring_w, int crop, int shuffle);
/* ---- the split-bf16 ("bf16x3") form of lic360_sconv3x3 / lic360_sconv1x1 (csrc/sconv_bf16x3.inc), opt-in: the same operation and the same
 * argument lists (sphere apron by index, window, crop, shuffle, bias + PReLU + residual; cells outside the window not touched), replacing the
 * same reference layers as its fp32 sibling.  Every fp32 operand is split into hi = bf16(v) and lo = bf16(v - hi); each product is
 * w_hi x_hi + w_hi x_lo + w_lo x_hi on v_mfma_f32_16x16x32_bf16 with fp32 accumulation: about 2^-16 relative error per product (fp32: 2^-24), this
 * kernel's own summation order -- 1e-4 against a library convolution on the transforms' data, at least 16x closer than single-pass bf16.
 * Inference only.  cin % 32 == 0, cout in {96} or a multiple of 192; packed = lic360_sconv3x3_bf16x3_pack (packed_bytes bytes, 16-byte aligned:
 * hi and lo bf16 planes in the waves' operand order) -- NOT the fp32 pack. */
int lic360_sconv3x3_bf16x3_supported(int cin, int cout);
long lic360_sconv3x3_bf16x3_packed_bytes(int cin, int cout);
int lic360_sconv3x3_bf16x3_pack(void *stream, const float *weight, void *packed, int cin, int cout);
int lic360_sconv3x3_bf16x3(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                           int n, int cin, int cout, int hp, int wp, int pad, int sphere, int ring, int ring_w, int crop, int shuffle);
/* the 1x1 layers in the same form (replaces what lic360_sconv1x1 replaces; same accuracy statement; cin % 32 == 0, cout = 96 or a multiple of 192) */
int lic360_sconv1x1_bf16x3_supported(int cin, int cout);
long lic360_sconv1x1_bf16x3_packed_bytes(int cin, int cout);
int lic360_sconv1x1_bf16x3_pack(void *stream, const float *weight, void *packed, int cin, int cout);
int lic360_sconv1x1_bf16x3(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                           int n, int cin, int cout, int hp, int wp, int ring, int ring_w, int crop, int shuffle);
/* ---- the single-pass bf16 ("bf16x1") form of the same four (csrc/sconv_bf16x3.inc with the lo parts left out; kernels k_sconv_b1), opt-in: the same
 * operation, argument lists and shape predicate as the bf16x3 entry points.  Every input value and every weight is rounded ONCE to bf16 (nearest even);
 * each product is one v_mfma_f32_16x16x32_bf16 with fp32 accumulation; bias, PReLU and residual are applied in fp32, unrounded: the result is the
 * fp32-accumulated convolution of the rounded operands (about 2^-8 relative per operand, this kernel's own summation order).  Inference only; NaN,
 * infinity and values within 2^-8 of FLT_MAX are outside the contract.  packed = lic360_sconv{3x3,1x1}_bf16x1_pack (packed_bytes = cout cin ks^2 2
 * bytes, 16-byte aligned: the hi bf16 planes in the waves' operand order) -- neither the fp32 nor the bf16x3 pack. */
int lic360_sconv3x3_bf16x1_supported(int cin, int cout);
long lic360_sconv3x3_bf16x1_packed_bytes(int cin, int cout);
int lic360_sconv3x3_bf16x1_pack(void *stream, const float *weight, void *packed, int cin, int cout);
int lic360_sconv3x3_bf16x1(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                           int n, int cin, int cout, int hp, int wp, int pad, int sphere, int ring, int ring_w, int crop, int shuffle);
int lic360_sconv1x1_bf16x1_supported(int cin, int cout);
long lic360_sconv1x1_bf16x1_packed_bytes(int cin, int cout);
int lic360_sconv1x1_bf16x1_pack(void *stream, const float *weight, void *packed, int cin, int cout);
int lic360_sconv1x1_bf16x1(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                           int n, int cin, int cout, int hp, int wp, int ring, int ring_w, int crop, int shuffle);
/* ---- the stride-2 (down-sampling) forms of the two, fp32, on the same kernel body with a stride parameter (csrc/conv3x3_kernels.hip).
 * lic360_sconv3x3s2 replaces the in-place SpherePad(2) + nn.Conv2d(cin, c, 3, 2, 3) + nn.PReLU + SphereTrim of test/model_zoo.py:64-106
 * (ResidualBlockDown.conv1, SphereConv2); lic360_sconv1x1s2 replaces nn.Conv2d(cin, c, 1, 2, 2) + the `t + y` add of ResidualBlockDown.short_cut.
 * x [n][cin][hp][wp] with a pad-cell apron, interior H x W = (hp - 2 pad) x (wp - 2 pad), both even; out (and residual: the OUTPUT's geometry)
 * [n][cout][H / 2 + 2 oring][W / 2 + 2 oring].  With X(r, c) the value the sphere rule puts at interior coordinates (r, c) (sphere = 0: the apron cell
 * as it is), interior output (i, j) = bias + sum w[kh][kw] X(2 i + kh - 1, 2 j + kw - 1), resp. bias + w X(2 i, 2 j); PReLU if slope; + residual if given.
 * The interior window [oring, oring + H / 2) x [oring, oring + W / 2) of out is written, every other cell left untouched.  The 3x3 form reads one apron
 * row above and one apron column left of the interior (pad >= 1), the 1x1 form the interior only.  packed = the STRIDE-1 packs (lic360_sconv3x3_pack,
 * lic360_sconv1x1_pack); shapes as the stride-1 forms (cin % 16 resp. % 32, cout = 96 or a multiple of 192); bias / slope 16-byte aligned. */
int lic360_sconv3x3s2_supported(int cin, int cout);
int lic360_sconv3x3s2(void *stream, const float *x, const float *packed, const float *bias, const float *slope, const float *residual, float *out,
                      int n, int cin, int cout, int hp, int wp, int pad, int sphere, int oring);
int lic360_sconv1x1s2_supported(int cin, int cout);
int lic360_sconv1x1s2(void *stream, const float *x, const float *packed, const float *bias, const float *slope, const float *residual, float *out,
                      int n, int cin, int cout, int hp, int wp, int pad, int oring);
/* ---- the single-pass bf16 ("bf16x1") forms of the stride-2 pair (kernels k_sconv_b1s2; the 3x3: csrc/sconv_b1s2.inc, the 1x1: csrc/sconv_bf16x3.inc at
 * stride 2), opt-in.  lic360_sconv3x3s2_bf16x1 replaces what lic360_sconv3x3s2 replaces (SpherePad(2) + nn.Conv2d(cin, c, 3, 2, 3) + nn.PReLU + SphereTrim
 * of test/model_zoo.py:64-106), lic360_sconv1x1s2_bf16x1 what lic360_sconv1x1s2 replaces (nn.Conv2d(cin, c, 1, 2, 2) + the add of
 * ResidualBlockDown.short_cut): the same operation, argument lists, shapes of x / out / residual and output window.  Arithmetic: the bf16x1 contract -- every
 * input value and every weight rounded ONCE to bf16 (nearest even), one v_mfma_f32_16x16x32_bf16 per product, fp32 accumulation, bias / PReLU / residual
 * in fp32: the fp32-accumulated stride-2 convolution of the rounded operands.  Inference only; NaN and infinity are outside the contract.
 * packed = the STRIDE-1 single-pass packs (lic360_sconv3x3_bf16x1_pack, lic360_sconv1x1_bf16x1_pack; 16-byte aligned) -- not an fp32 pack; the shape
 * predicates are the stride-1 single-pass ones (cin % 32 == 0, cout = 96 or a multiple of 192); bias / slope 16-byte aligned. */
int lic360_sconv3x3s2_bf16x1_supported(int cin, int cout);   /* == lic360_sconv3x3_bf16x1_supported */
int lic360_sconv3x3s2_bf16x1(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                             int n, int cin, int cout, int hp, int wp, int pad, int sphere, int oring);
int lic360_sconv1x1s2_bf16x1_supported(int cin, int cout);   /* == lic360_sconv1x1_bf16x1_supported */
int lic360_sconv1x1s2_bf16x1(void *stream, const float *x, const void *packed, const float *bias, const float *slope, const float *residual, float *out,
                             int n, int cin, int cout, int hp, int wp, int pad, int oring);
/* ---- the gate of the attention blocks in one launch (kernels k_gate_sconv / k_gate_sconv_b3 / k_gate_sconv_b1: the 1x1 stride-1 bodies of the three forms with
 * a gate epilogue, csrc/conv3x3_kernels.hip), opt-in: replaces the tail of AttentionBlock, test/model_zoo.py:25-46 -- the gate's nn.Conv2d(c, c, 1) + nn.Sigmoid +
 * the `*` with the trunk + the `+` with the input.  x [n][cin][hp][wp] (the attention branch's last bottleneck output); trunk, residual and out
 * [n][cout][hp][wp]; on rows [ring, hp - ring) x columns [ring_w, wp - ring_w):
 *     y = conv1x1(x) + bias (the form's own accumulation);  g = 1.0f / (1.0f + lic360_expf(-y));  out = residual + trunk * g
 * with one fp32 rounding per operation and no fused multiply-add (lic360_expf: csrc/lic360_exact_math.h, host / device bit-identical, so the epilogue is
 * reproducible on the CPU bit for bit; g == 1 for y >= 32, g == 0 for y <= -89; NaN and infinity are outside the contract).  The other cells of out are NOT touched.
 * No PReLU, crop or shuffle.  packed = the form's stride-1 1x1 pack (lic360_sconv1x1_pack / _bf16x3_pack / _bf16x1_pack); shapes, alignments (bias, a bf16
 * pack: 16 bytes) and refusals are those of lic360_sconv1x1 / _bf16x3 / _bf16x1; trunk and residual are required (a null pointer is refused). */
int lic360_sconv1x1_gate(void *stream, const float *x, const float *packed, const float *bias, const float *trunk, const float *residual, float *out,
                         int n, int cin, int cout, int hp, int wp, int ring, int ring_w);
int lic360_sconv1x1_gate_bf16x3(void *stream, const float *x, const void *packed, const float *bias, const float *trunk, const float *residual, float *out,
                                int n, int cin, int cout, int hp, int wp, int ring, int ring_w);
int lic360_sconv1x1_gate_bf16x1(void *stream, const float *x, const void *packed, const float *bias, const float *trunk, const float *residual, float *out,
                                int n, int cin, int cout, int hp, int wp, int ring, int ring_w);
/* ---- narrow workgroups for small launches (kernels k_narrow_conv / k_narrow_gate, csrc/conv3x3_kernels.hip), opt-in.  The stride-1 convolutions and the gate above
 * with `cpw` = 96 or 48 output channels per workgroup instead of a whole pack block (192 where cout is a multiple of 192, else 96): cout / cpw times as many
 * workgroups, for maps with too few 16 x 16 tiles to fill the chip.  Results are bit-identical to the wide calls; packs, shapes, alignments, window, crop and shuffle
 * are theirs.  form: 0 = fp32, 3 = split-bf16, 1 = single-pass bf16 (packed = that form's stride-1 pack of kernel size ks); ks: 3 or 1 (ks = 1: pad = 0, sphere = 0).
 * Refused before any launch: an unknown form, cpw outside {48, 96}, cpw not below the pack's block, and whatever the wide call refuses; the gate takes cout % 192 == 0.
 * Tall last tile row: a remainder of up to 8 / (cpw / 48) rows, except in the split-bf16 form at cpw = 48, where a remainder takes a tile row of its own. */
int lic360_sconv_narrow_supported(int form, int ks, int cin, int cout, int cpw);
int lic360_sconv_narrow(void *stream, int form, int ks, int cpw, const float *x, const void *packed, const float *bias, const float *slope, const float *residual,
                        float *out, int n, int cin, int cout, int hp, int wp, int pad, int sphere, int ring, int ring_w, int out_crop, int shuffle);
int lic360_sconv1x1_gate_narrow(void *stream, int form, int cpw, const float *x, const void *packed, const float *bias, const float *trunk, const float *residual,
                                float *out, int n, int cin, int cout, int hp, int wp, int ring, int ring_w);
/* apron of dst <- sphere-wrapped interior of src (src == dst: lic360_sphere_pad_inplace); [nc][hp][wp] planes      sphere_pad_cuda.cu:48-65 */
int lic360_sphere_apron_from(void *stream, const float *src, float *dst, int nc, int hp, int wp, int pad);

/* Test hooks of the DEVICE arithmetic coder (A19/A20 as they run inside the fused codec): raw int32 tables [n][ncode+1]
 * (every table totals 65536), labels and an optional mask, all in device memory, through the same kernels the codec
 * launches -- encode: k_ac_encode; decode: k_dec_init + k_dec_plane (ncode == 8) or k_imp_dec_plane (other alphabets),
 * `chunk` symbols per launch with the coder state carried between launches like between planes.  Reference behaviour:
 * extension/coder.cpp:30-113 over extension/ArithmeticCoder.cpp:34-116.  Synchronises the stream before returning.
 * The 8-symbol decoder carries the 7 inner table entries as 16-bit values (they are < 65536 whenever the last symbol has a
 * non-zero frequency, as every table of this codec does); a table that does not fit sets error bit 64. */
int lic360_devcoder_encode(void *stream, const int *tables, int ncode, const int *labels, const float *mask, long n,
                           uint8_t *bytes, long cap, int *nbytes, int *err);
int lic360_devcoder_decode(void *stream, const int *tables, int ncode, const float *mask, long n, int chunk,
                           const uint8_t *bytes, long cap, const int *nbytes, float *out, int *err);

/* ---- rate estimation: the exact ideal code length of what the fused codecs would write, without running the coder (csrc/rate_kernels.hip; no
 * reference counterpart -- the reference's evaluation loop, train/trainDDP_IMP_ENT.py:54-88, reports a float entropy estimate beside the real rate).
 * Both codecs end their encode-order pass with one record (cdf[sym], cdf[sym + 1]) per symbol in coding order, (0, 0) for a symbol the coder skips.  A
 * coded symbol of frequency f = hi - lo in [1, 65536] costs cost(f) = round(2^32 (16 - log2 f)) Q32 bits, an unsigned 64-bit integer (cost(2^k) =
 * (16 - k) 2^32 exactly, cost(65536) = 0); a record with hi == lo costs 0 and is not counted.  An image's code length is the integer sum of its symbols'
 * costs: independent of the reduction order, below 2^55 for 393 216 symbols, so every output fits int64.  All outputs are device memory, one unsigned
 * 64-bit integer per entry, and are zeroed in the stream before the launch: bits_q32[b], nsym[b] (coded symbols), and where the pointer is not NULL
 * group_q32[b][g], row_q32[b][h] -- the same bits by group and by latitude row of the latent (each sums to bits_q32[b]).
 * lic360_rate_table: the 65 537 costs by f (entry 0 = 0), host memory, built in double precision; host-only, needs no GPU.
 * lic360_rate_records: test hook, the twin of lic360_devcoder_encode -- raw tables [b n][ncode + 1], labels and an optional mask for b images of n
 *   symbols through the same record construction, then the reduction without a breakdown; synchronises the stream before returning.
 * lic360_codec_estimate / lic360_impcodec_estimate: everything lic360_codec_encode / lic360_impcodec_encode do up to and including the records, then the
 *   reduction instead of the coder (no bitstream, no D2H copy, no host threads whatever the coder mode).  The maps have one group: a row breakdown only.
 * lic360_codec_rate_last / lic360_impcodec_rate_last: the same reduction over the records the codec's most recent encode or estimate left, for callers
 *   who want the streams and the breakdown; refused (argument error, no launch) unless that call held at least b images. */
int lic360_rate_table(unsigned long long *out);
int lic360_rate_records(void *stream, const int *tables, int ncode, const int *labels, const float *mask, long n, int b,
                        unsigned long long *bits_q32, unsigned long long *nsym);
int lic360_codec_estimate(void *stream, lic360_codec *codec, const float *code, const float *mask, int b, unsigned long long *bits_q32,
                          unsigned long long *nsym, unsigned long long *group_q32, unsigned long long *row_q32);
int lic360_codec_rate_last(void *stream, lic360_codec *codec, int b, unsigned long long *bits_q32, unsigned long long *nsym,
                           unsigned long long *group_q32, unsigned long long *row_q32);
int lic360_impcodec_estimate(void *stream, lic360_impcodec *codec, const float *levels, int b, unsigned long long *bits_q32,
                             unsigned long long *nsym, unsigned long long *row_q32);
int lic360_impcodec_rate_last(void *stream, lic360_impcodec *codec, int b, unsigned long long *bits_q32, unsigned long long *nsym,
                              unsigned long long *row_q32);

/* Where the serial arithmetic-coder phases of the fused latent codec run.  The reference runs its coder on the CPU (extension/coder.cpp:70-113, called per
 * plane from test/lic360_demo.py:139-140,234); the fused codec keeps it on the GPU (one wave per image) where many images per call hide it, and hands it
 * to host threads -- records D2H / per-plane tables through pinned memory, polled flags -- when a call holds few images.  mode 0: device, 1: host
 * (<= 64 images per call), 2 (default): host for calls of at most 8 images.  LIC360_HOST_CODER=0|1, read when a codec is created (codec_switches.h), sets the mode.  Bitstreams are identical. */
int lic360_codec_set_coder(lic360_codec *codec, int mode);

/* ---- dead-cone skip of the fused latent codec (round 6; csrc/need.h) -------------------------------------------------------------
 * The reference evaluates every output of the entropy nets (extension/cconv_ec_cuda.cu:317-339, cconv_dc_cuda.cu:367-398) and coder.cpp:79 then
 * skips the masked symbols.  The fused codec does not compute what no coded symbol can observe: need_l(y, x) = highest group of layer l whose
 * output some coded symbol reads (-1: none), need_11 = the mask's highest coded group, need_l = min(G - 1, 5 x 5 dilation of need_{l+1} + dy + dx).
 * Bitstreams and decoded symbols are unchanged.  lic360_need_maps: masks [b, g, h, w] -> need [b][12][h][w] int8 (device), the kernel the codec runs. */
int lic360_need_maps(void *stream, const float *mask, int b, int g, int h, int w, signed char *need_out);
/* Host-only (no GPU work): how the decode-order task lists pack the live row windows lo[k]..hi[k] (k < c <= 8 samples of one chunk; hi < lo: none) of an
 * image of h <= 128 rows into waves -- round 5's tape rules with a window per sample; pieces[3 w + i] = piece i of wave w
 * (k | (slo & 63) << 3 | (shi & 63) << 9 | a0 << 15 | 1 << 21 | (slo >> 6) << 25 | (shi >> 6) << 26, 0 = none; room for 6 c words, 9 c words where
 * h > 64: a window taller than a wave is cut over up to three), *n_waves = waves used.  tests/test_dcl_pack.py, tests/test_dc_tall_cpu.py. */
int lic360_dcl_pack_layout(int h, int c, const int *lo, const int *hi, unsigned *pieces, int *n_waves);
/* Host-only (no GPU work): the order of ONE XCD's decode list of one (layer, plane) -- LIC360_DC_ORDER, read when a codec is created: "1" block major
 * (heaviest three-group block first, then net, then record), "2" / "4" / "8" the blocks in groups of nb and inside a group net, record, block, followed by
 * the placement pass (per round of w records -- what the XCD's w workgroups run side by side -- the heaviest record to the least loaded workgroup; a
 * record stays in its round; "8" is the default), "1p" the block-major order with the placement pass.  The list's n_blocks blocks in list order: first group g0[j], nrec[j]
 * records per net; record (j, net, r) is id = 3 * (nrec[0] + .. + nrec[j - 1]) + net * nrec[j] + r, its block-major position.  emit[id] = its position after
 * the grouped emission, slot[id] = after the placement too (place = 0: emit[id]).  ngroup: the latent's groups (cost of a record =
 * min(g0 + 7, ngroup) steps + 3 per task); 1 <= nb <= 8, 1 <= w <= 32, n_blocks <= 24.  tests/test_dc_order_cpu.py. */
int lic360_dcl_order_layout(int n_blocks, const int *g0, const int *nrec, int ngroup, int nb, int place, int w, int *emit, int *slot);
/* enable > 0: the following encodes / decodes count what they execute (0: stop; < 0: leave as it is).  out (host, 2 * 12 * 64 values, may be NULL; reading clears):
 * [0][layer][group block] live (tile, group block) pairs of the encode-order launches (64 positions x the block's groups, per sample),
 * [1][layer][group] cells the decode-order launches stored.  *skip_active_out (may be NULL): 0 the codec does not skip (generic kernels or
 * LIC360_NOSKIP), 1 encode order only, 2 both orders (decode order: batches of >= 16 images, 8 | batch, h <= 128; LIC360_DC_NOTALL=1, read when a codec is created (codec_switches.h): h <= 64). */
int lic360_codec_skip_stats(lic360_codec *codec, int enable, unsigned long long *out, int *skip_active_out);
/* test hooks: every interior cell of the codec's activation buffers <- value (finite); what the last encode / decode scheduled
 * (which 0: need maps, 1 / 2: encode-order list counts / entries, 3 / 4: decode-order list counts / records; see csrc/codec_fused.hip) */
int lic360_codec_debug_fill(void *stream, lic360_codec *codec, float value);
int lic360_codec_debug_lists(lic360_codec *codec, int which, void *host_out, long bytes, int *cap_out);
/* test hook: what the codec's activation buffers hold once the stream's work is done, over the interior cells that lic360_codec_debug_fill fills.  15 values
 * each (host), in the order e_buf[0..2] (encode order's ping-pong buffers), d_act[0..10] (decode order's layers), d_y: absmax = the largest |v| among the
 * finite cells, nonfinite = the number of Inf / NaN cells.  tests/test_gpu_skip_age.py: a skipped cell must stay bounded across calls. */
int lic360_codec_debug_absmax(void *stream, lic360_codec *codec, float *absmax, int *nonfinite);

/* calibration for bench.py (no reference counterpart): the fp32 MFMA rate (v_mfma_f32_16x16x4_f32, 8 waves per CU) this device sustains right now, in
 * TFLOP/s, and its compute-unit count; ~50 ms.  bench.py prints it beside the headline so that figures of different boxes of a pool can be normalised. */
int lic360_calib_mfma_f32(void *stream, double *tflops, int *cus_out);

/* timing hooks for bench.py's instrumented pass: HIP events around every launch of each kernel class of the codec
 * (classes() names them, comma separated: first / hidden / last conv layers in both orders, table builds, coder kernels),
 * recorded on the caller's stream; read() fills ms[k] / launches[k] per class (n >= number of classes) and resets */
/* the kernels behind each kernel class of the timing hooks, "class=kernel+kernel;..." (names as rocprofv3 prints them) */
const char *lic360_codec_kernel_names(void);
int lic360_codec_profile_enable(lic360_codec *codec, int on);
const char *lic360_codec_profile_classes(void);
int lic360_codec_profile_read(lic360_codec *codec, int n, double *ms, long *launches);

#ifdef __cplusplus
}
#endif
#endif /* LIC360_HIP_H */
