/* u3d_subpix_bf16.h — a part of include/u3d.h, which includes it inside its extern "C" block (it has no guard and no wrapper of its own and
 * uses u3d_stream_t: include u3d.h, never this file).  Declarations in the form of u3d.h: pytorch3dunet_amd/_native.py reads them with the
 * same reader into the second table of the binding.
 * ---- (Added, U3D_VERSION unchanged.)  Sub-pixel decoder convolutions of a UNet3D on the bf16 MFMA (`bf16_subpixel: true`;
 * csrc/u3d_subpix_bf16.hip, the slice helpers in csrc/u3d_bf16.hip) ------
 * The bf16 twins of u3d_subpixel_conv_fwd / _dgrad_reps / _wgrad on v_mfma_f32_32x32x16_bf16 and the 3-D twins of the 2-D block of u3d.h: the
 * upsampled half of cat(skip, F.interpolate(low, nearest)) under a decoder's first Conv3d at a level that upsamples by exactly 2 on all
 * three axes, as eight parity-class 2x2x2 convolutions over the low-res grid — 8/27 of the multiply-adds in all three directions, the
 * data gradient at low resolution with the children sum folded in.  Tensors in HBM are fp32 NDHWC, accumulation is fp32.
 * Rounding points: WEIGHTS — the pre-summed taps are added in fp32 from the fp32 master weight (ascending (tz, ty, tx) order) and rounded
 * ONCE to bf16, nearest even, by the pack kernel; ACTIVATIONS and dz — rounded once while staged to LDS, after the fp32 affine fmaf(x, a,
 * b); zero padding applies after the affine and stays exactly 0.  Forward and data gradient are therefore not bit-equal to the 27-tap bf16
 * kernels on a written-out concat (which round every tap); the weight gradient multiplies the same bf16 operands.
 * Envelope: C1 % 32 == 0, Cout % 32 == 0 (the skip slice: Cin % 32 == 0), 16-byte aligned pointers (affine_sample_stride % 4 == 0), any
 * D1, H1, W1 >= 1, N * 8 * D1 * H1 * W1 < 2^31; outside it every entry point returns U3D_EINVAL (u3d_last_error) without launching
 * anything and the size functions return 0.
 *   u3d_pack_subpixel_weights_bf16  channels [c_off, c_off + C1) of the full (Cout, Cin_total, 3, 3, 3) weight -> an image of
 *              u3d_subpixel_bf16_packed_elems(C1, Cout, dgrad) = 64 * C1 * Cout 2-byte elements (exactly: the B prefetch never leaves a
 *              chunk, so there is no tail padding) in the B-operand lane layout of u3d_pack_weights_bf16, [K / 16 chunk][64][n-tile][64
 *              lanes][8].  dgrad = 0 (forward, K = C1): entry (4a + 2b + c) * 8 + 4u + 2v + w = parity class (a, b, c), tap half (u, v,
 *              w); per axis parity 0 reads low-res offsets (-1, 0) with taps {t0}, {t1 + t2}, parity 1 reads (0, +1) with {t0 + t1},
 *              {t2}.  dgrad = 1 (K = Cout): entry 16 rz + 4 ry + rx of the 4 x 4 x 4 stride-2 gather; per axis dz[2j - 1 .. 2j + 2]
 *              carry t2, t1 + t2, t0 + t1, t0
 *   u3d_subpixel_conv_fwd_bf16      the contract of u3d_subpixel_conv_fwd: low (N,D1,H1,W1,C1), affine optional (sample n at affine + n *
 *              affine_sample_stride floats), out (N,2*D1,2*H1,2*W1,Cout) receives the plain partial sums (no ReLU, no statistics): add
 *              the skip half with u3d_conv3d_bf16_ex(skip, sliced image, residual = out).  ONE launch; the staged low-res halo of a
 *              16-channel chunk serves all eight classes: 27 A-fragment positions, 64 MFMAs per M-tile and n-tile.  No split-K
 *   u3d_subpixel_conv_dgrad_bf16    dlow (N,D1,H1,W1,C1) from dz (N,2*D1,2*H1,2*W1,Cout), de-interleaved into its eight parity planes
 *              while staged; optional gstats double[reps][N][C1][2] += (sum dlow, sum dlow * x_low), zeroed by the caller (needs x_low);
 *              dlow is bit-identical for any reps
 *   u3d_subpixel_conv_wgrad_bf16    the 64 (class, tap half) C1 x Cout matrices over the low-res grid, written per block to its slot of
 *              `workspace` and folded into the 27 taps by a second kernel that adds the slots in slot order: no atomics, the same inputs
 *              (and workspace size) give the same bits.  workspace: u3d_subpixel_wgrad_bf16_workspace_floats() floats hold the plan that
 *              fills the CURRENT device (the size function takes no device); the launch runs at most as many splits as `workspace_floats`
 *              holds slots of 64 * C1 * Cout floats, so a size asked on another device still runs; less than one slot is U3D_EINVAL.  dw points at the first
 *              upsampled input channel inside the (Cout, dw_cin_stride, 3, 3, 3) gradient; only channels [dw, dw + C1) are written
 *   u3d_pack_weights_bf16_slice     u3d_pack_weights_bf16 of the input channels [c_off, c_off + Cin) of a (Cout, cin_stride, 3, 3, 3)
 *              weight; c_off = 0, cin_stride = Cin writes the image of u3d_pack_weights_bf16 bit for bit
 *   u3d_conv3d_wgrad_bf16_strided   u3d_conv3d_wgrad_bf16 writing a CHANNEL SLICE of a wider gradient: dw points at the slice's first
 *              input channel inside (Cout, dw_cin_stride, 3, 3, 3); dw_cin_stride = Cin writes u3d_conv3d_wgrad_bf16's dw bit for bit
 *              (workspace: u3d_wgrad_bf16_workspace_floats)
 * The skip half's forward and data gradient are u3d_conv3d_bf16_ex on sliced images, unchanged. */
long long u3d_subpixel_bf16_packed_elems(int C1, int Cout, int dgrad);
int u3d_pack_subpixel_weights_bf16(int device, u3d_stream_t stream, const float* w, int Cout, int Cin_total, int c_off, int C1, int dgrad,
                                   void* packed);
int u3d_subpixel_conv_fwd_bf16(int device, u3d_stream_t stream, const float* low, const float* affine, long long affine_sample_stride,
                               const void* packed, float* out, int N, int D1, int H1, int W1, int C1, int Cout);
int u3d_subpixel_conv_dgrad_bf16(int device, u3d_stream_t stream, const float* dz, const void* packed, const float* x_low, float* dlow,
                                 double* gstats, int N, int D1, int H1, int W1, int C1, int Cout, int reps);
long long u3d_subpixel_wgrad_bf16_workspace_floats(int N, int D1, int H1, int W1, int C1, int Cout);
int u3d_subpixel_conv_wgrad_bf16(int device, u3d_stream_t stream, const float* low, const float* affine, long long affine_sample_stride,
                                 const float* dz, float* dw, int dw_cin_stride, int N, int D1, int H1, int W1, int C1, int Cout,
                                 float* workspace, long long workspace_floats);
int u3d_pack_weights_bf16_slice(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, int cin_stride, int c_off,
                                void* packed);
int u3d_conv3d_wgrad_bf16_strided(int device, u3d_stream_t stream, const float* x, const float* affine, const float* dz, float* dw,
                                  int dw_cin_stride, int N, int D, int H, int W, int Cin, int Cout, float* workspace,
                                  long long workspace_floats);
