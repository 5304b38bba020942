/* u3d_ext.h — the C-ABI of libu3d_ext_hip.so, the extension library next to libu3d_hip.so (csrc/u3d_c16_bf16.hip,
 * csrc/u3d_wgrad_f32s.hip with its header csrc/u3d_conv2d_f32s.h).
 *
 * A header PART: declarations only — no guard, no C++ wrapper, no constants.  Include it after <u3d.h>, inside extern "C":
 *     extern "C" {
 *     #include <u3d.h>      (u3d.h carries its own wrapper; it does not include this file)
 *     #include <u3d_ext.h>
 *     }
 * The extension links against the core library: error codes, u3d_last_error() and the device handling are the core's own.
 *
 * ---- 16-channel 3x3x3 convolutions of a UNet3D on the bf16 MFMA (`bf16_stem: true`) ------
 * The twins of u3d_conv3d_bf16_ex (without `residual`) and u3d_conv3d_wgrad_bf16 on v_mfma_f32_32x32x16_bf16 for layers whose channel
 * counts are multiples of 16 in EVERY role (forward, data gradient with the roles swapped, weight gradient).  Tensors are fp32 NDHWC,
 * accumulation is fp32, pointers 16-byte aligned, N * D * H * W < 2^31.
 * Rounding points: the weight is rounded once, nearest even, by the pack kernel; activations and dz are rounded once while staged to
 * LDS, after the optional per-sample affine applied in fp32 as fmaf(x, a, b); zero padding applies after the affine and stays exactly 0.
 *   u3d_conv3d_bf16_c16_supported            1 iff both counts > 0 and both % 16 == 0
 *   u3d_packed_weight_bf16_c16_elems         2-byte elements of the image u3d_pack_weights_bf16_c16 writes; 0 outside the envelope
 *   u3d_pack_weights_bf16_c16                w (Cout, Cin, 3, 3, 3) fp32 -> image [K / 16 chunk][27 taps][n-tile][64 lanes][8] of B[k][n];
 *              mode 0 forward (B[k = ci][n = co] = w[co][ci][tap]), mode 1 data gradient (B[k = co][n = ci] = w[co][ci][26 - tap]); the
 *              columns of a half n-tile (n >= the produced channel count) are zero
 *   u3d_conv3d_bf16_c16_workspace_floats     always 0: no split-K (narrow layers sit at high resolution); workspace may be NULL
 *   u3d_conv3d_bf16_c16                      out (N,D,H,W,Cout) = [relu](conv3d(bf16(a * x + b), bf16(w))); affine optional, (N, Cin, 2);
 *              out_stats optional, double[N][Cout][2] += (sum y, sum y^2) of the stored values.  Data-gradient form: the mode-1 image,
 *              relu = 0, x = dz, Cin / Cout swapped, gx = the layer's forward input: gstats double[N][Cout][2] += (sum y, sum y * gx).
 *              out_stats and gstats are exclusive.
 *   u3d_wgrad_bf16_c16_workspace_floats      floats of the plan that fills the current device; one slot is 27 * Cin * Cout floats
 *   u3d_conv3d_wgrad_bf16_c16                dw (Cout, Cin, 3, 3, 3) = sum_v bf16(dz[v, co]) * bf16(g[v + tap - 1, ci]), g = a * x + b zero
 *              padded; WRITTEN, not accumulated.  No atomics: every block writes its partial sums to its workspace slot and a second kernel
 *              adds the slots in slot order — the same inputs and workspace size give the same bits.  A workspace smaller than the size
 *              function's runs on as many splits as it holds; smaller than one slot: U3D_EINVAL.
 * Outside the envelope, or with unaligned pointers, every launch returns U3D_EINVAL with u3d_last_error() set and launches nothing.
 *
 * ---- the weight gradient of `compute_dtype: fp32_split` on the bf16 MFMA (`fp32_split_wgrad: true`; csrc/u3d_wgrad_f32s.hip) ------
 * The contract of u3d_conv3d_wgrad_bf16_strided with fp32-grade arithmetic.  Both operands are split exactly into three bf16 values while
 * staged, after the fp32 affine: h = bf16(g), m = bf16(g - h), l = bf16(g - h - m); the six products hh, hm, mh, hl, lh, mm run on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation; every voxel tile's MFMA chain starts from zero and is added to the running sums with
 * the sign of dz alternating per tile, which cancels the MFMA's round-down accumulation drift.
 *   u3d_conv3d_wgrad_f32s_supported          1 iff both counts > 0 and both % 32 == 0
 *   u3d_wgrad_f32s_workspace_floats          floats of the plan that fills the current device; one slot is 27 * Cin * Cout floats; 0 outside
 *              the envelope
 *   u3d_conv3d_wgrad_f32s                    dw[co][ci][tap] = sum_v dz[v, co] * g[v + tap - 1, ci], g = fmaf(x, a, b) from the optional
 *              (N, Cin, 2) affine, zero padded after it; WRITTEN, not accumulated, into channels [dw, dw + Cin) of a
 *              (Cout, dw_cin_stride, 3, 3, 3) gradient (dw_cin_stride = Cin: the plain layout).  x, affine, dz and workspace 16-byte
 *              aligned.  No atomics: every block writes its partial sums to its workspace slot and a second kernel adds the slots in a
 *              fixed order — the same inputs and workspace size give the same bits.  A workspace smaller than the size function's runs
 *              on as many splits as it holds; outside the envelope, or smaller than one slot: U3D_EINVAL, nothing launched.
 *   u3d_ext_version                          the extension's own version, compared by the Python host with its constant */
int u3d_ext_version(void);
int u3d_conv3d_bf16_c16_supported(int Cin, int Cout);
long long u3d_packed_weight_bf16_c16_elems(int Cin, int Cout, int mode);
int u3d_pack_weights_bf16_c16(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, void* packed);
long long u3d_conv3d_bf16_c16_workspace_floats(int N, int D, int H, int W, int Cin, int Cout);
int u3d_conv3d_bf16_c16(int device, u3d_stream_t stream, const float* x, const float* affine, const void* packed_w, float* out, int N,
                        int D, int H, int W, int Cin, int Cout, int relu, double* out_stats, const float* gx, double* gstats,
                        float* workspace, long long workspace_floats);
long long u3d_wgrad_bf16_c16_workspace_floats(int N, int D, int H, int W, int Cin, int Cout);
int u3d_conv3d_wgrad_bf16_c16(int device, u3d_stream_t stream, const float* x, const float* affine, const float* dz, float* dw, int N,
                              int D, int H, int W, int Cin, int Cout, float* workspace, long long workspace_floats);
int u3d_conv3d_wgrad_f32s_supported(int Cin, int Cout);
long long u3d_wgrad_f32s_workspace_floats(int N, int D, int H, int W, int Cin, int Cout);
int u3d_conv3d_wgrad_f32s(int device, u3d_stream_t stream, const float* x, const float* affine, const float* dz, float* dw, int dw_cin_stride,
                          int N, int D, int H, int W, int Cin, int Cout, float* workspace, long long workspace_floats);
/* ---- the residual epilogue of a ResidualUNet2D in fp32_split (`native_2d_residual_fp32_split: true`; csrc/u3d_conv2d_f32s.h) ------
 * u3d_conv2d_f32s (below: arithmetic, rounding points, mode-0 images of u3d_pack_weights2d_f32s, envelope of u3d_conv2d_f32s_supported,
 * replica rows, no split-K) on ONE real source x (N,H,W,Cin), plus the tail of a ResNetBlock: the twin of u3d_conv2d_res_reps.
 *   u3d_conv2d_f32s_res                      out (N,H,W,Cout) = [relu](conv2d(a * x + b, w) + residual); residual (N,H,W,Cout) fp32, 16-byte
 *              aligned, added in fp32 to the signed accumulator — before the ReLU and before the statistics, never rounded to bf16;
 *              out_stats optional, double[stat_reps][N][Cout][2] += (sum y, sum y^2) of the STORED values.  residual may alias out: the
 *              lane that writes an element has read it first.  A NULL or unaligned residual, or channel counts outside the envelope:
 *              U3D_EINVAL with u3d_last_error() set, nothing launched. */
int u3d_conv2d_f32s_res(int device, u3d_stream_t stream, const float* x, const float* affine, const void* packed_w, float* out, int N,
                        int H, int W, int Cin, int Cout, int relu, double* out_stats, int stat_reps, const float* residual);
/* ---- the 3x3 convolutions of a UNet2D in fp32_split (`native_2d_fp32_split: true`; csrc/u3d_conv2d_f32s.h, a header of
 * csrc/u3d_wgrad_f32s.hip) ------
 * The twins of u3d_conv2d_ex_reps / u3d_conv2d_wgrad with fp32-grade arithmetic on v_mfma_f32_32x32x16_bf16.  Tensors are fp32 NHWC,
 * pointers 16-byte aligned, N * H * W < 2^31.  A source (p0, p1, ymap, xmap, C0, C1, H1, W1) is the virtual concat cat(skip,
 * nearest(low)) of a decoder's first convolution: p0 (N,H,W,C0), channels [C0, C0 + C1) from p1 (N,H1,W1,C1) at (ymap[y], xmap[x]);
 * p1 == NULL with C1 == 0 is a single tensor.  Virtual envelope: C0 % 32 == 0 and C1 % 32 == 0.
 * Rounding points: every fp32 operand is split exactly into three bf16 values, h = bf16(g), m = bf16(g - h), l = bf16(g - h - m) — the
 * weight by the pack kernel, activations and dz while staged to LDS, after the optional per-sample affine applied in fp32 as
 * fmaf(x, a, b); zero padding applies after the affine and stays exactly 0.  The six products hh, hm, mh, hl, lh, mm run smallest class
 * first with fp32 accumulation.  The MFMA's round-down accumulation drift is cancelled by sign alternation: forward / data gradient —
 * the images carry (-1)^chunk and the sums are negated between 16-channel chunks; weight gradient — every 16 x 16 pixel tile's chain
 * starts from zero and is added to the running sums, the sign of dz alternating per tile.  No split-K: workspace only in the weight gradient.
 *   u3d_conv2d_f32s_supported                1 iff both counts > 0, contraction channels K % 16 == 0 and produced channels Nn % 32 == 0
 *   u3d_conv2d_wgrad_f32s_supported          1 iff both counts > 0 and both % 32 == 0
 *   u3d_packed_weight2d_f32s_elems           2-byte elements of the three images u3d_pack_weights2d_f32s writes; 0 outside the envelope
 *   u3d_pack_weights2d_f32s                  w (Cout, Cin, 3, 3) fp32 -> three images (h | m | l of (-1)^chunk * w), each
 *              [K / 16 chunk][9 taps][n-tile][64 lanes][8] of B[k][n]; mode 0 forward (B[k = ci][n = co] = w[co][ci][tap]), mode 1 data
 *              gradient (B[k = co][n = ci] = w[co][ci][8 - tap])
 *   u3d_conv2d_f32s                          out (N,H,W,Cout) = [relu](conv2d(a * src + b, w)) with the mode-0 images; affine optional,
 *              (N, C0 + C1, 2); out_stats optional, double[stat_reps][N][Cout][2] += (sum y, sum y^2) of the stored values, a block
 *              adding into replica row block % stat_reps
 *   u3d_conv2d_f32s_dgrad                    dg (N,H,W,C0 + C1) = the data gradient of that layer from dz (N,H,W,Cout) with the mode-1
 *              images (Cout % 16, C0 + C1 % 32); gstats optional, double[stat_reps][N][C0 + C1][2] += (sum dg, sum dg * gx), gx = the
 *              layer's forward input (gx0, gx1, ymap, xmap: single or virtual, read only with gstats)
 *   u3d_wgrad2d_f32s_workspace_floats        floats of the plan that fills the current device; one slot is 9 * Cin * Cout floats; 0 outside
 *              the envelope
 *   u3d_conv2d_wgrad_f32s                    dw (Cout, C0 + C1, 3, 3) = sum_v dz[v, co] * g[v + tap - 1, ci], g = fmaf(src, a, b) zero
 *              padded; WRITTEN, not accumulated.  No atomics: every block writes its partial sums to its workspace slot and a second
 *              kernel adds the slots in slot order — the same inputs and workspace size give the same bits.  A workspace smaller than the
 *              size function's runs on as many splits as it holds; smaller than one slot: U3D_EINVAL.
 * Outside the envelope, or with unaligned pointers, every launch returns U3D_EINVAL with u3d_last_error() set and launches nothing. */
int u3d_conv2d_f32s_supported(int K, int Nn);
int u3d_conv2d_wgrad_f32s_supported(int Cin, int Cout);
long long u3d_packed_weight2d_f32s_elems(int Cin, int Cout, int mode);
int u3d_pack_weights2d_f32s(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, void* packed);
int u3d_conv2d_f32s(int device, u3d_stream_t stream, const float* p0, const float* p1, const int32_t* ymap, const int32_t* xmap, int C0,
                    int C1, int H1, int W1, const float* affine, const void* packed_w, float* out, int N, int H, int W, int Cout, int relu,
                    double* out_stats, int stat_reps);
int u3d_conv2d_f32s_dgrad(int device, u3d_stream_t stream, const float* dz, const void* packed_w, float* dg, int N, int H, int W, int Cout,
                          const float* gx0, const float* gx1, const int32_t* ymap, const int32_t* xmap, int C0, int C1, int H1, int W1,
                          double* gstats, int stat_reps);
long long u3d_wgrad2d_f32s_workspace_floats(int N, int H, int W, int Cin, int Cout);
int u3d_conv2d_wgrad_f32s(int device, u3d_stream_t stream, const float* p0, const float* p1, const int32_t* ymap, const int32_t* xmap,
                          int C0, int C1, int H1, int W1, const float* affine, const float* dz, float* dw, int N, int H, int W, int Cout,
                          float* workspace, long long workspace_floats);
