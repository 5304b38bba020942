// u3d_conv2d_bf16.hip — the bf16-operand twins of the 3x3 Conv2d kernels of csrc/u3d_conv2d.hip (`native_2d_bf16: true` on a UNet2D):
// forward / data gradient / weight gradient as implicit GEMM on v_mfma_f32_32x32x16_bf16 — bf16 operands, FP32 accumulation; the
// activations in HBM (NHWC fp32, the D = 1 layout), the statistics, ReLU and the parameter gradients stay fp32.  Operands are rounded
// once, to nearest even: the weights when u3d_pack_weights2d_bf16 writes the image from the fp32 master copy, the activations while
// they are staged into LDS, after the fp32 affine fmaf(x, a, b) of the GroupNorm / BatchNorm in front of the convolution (zero padding
// applies after the affine and stays exactly 0).
//
// Replaces the ATen kernels behind nn.Conv2d(in, out, 3, padding=1, bias=False) (buildingblocks.py:55-58) and its autograd for the
// layers whose channel counts fit (contraction channels % 16, produced channels % 32; the 3-D rule of csrc/u3d_bf16.hip).
//
// Forward / data gradient (conv2d_bf16_kernel): a block = 4 waves owns the 16(y) x 16(x) pixel tile of the fp32 kernel (256 GEMM rows,
// wave w rows 4w .. 4w + 3 as two M-tiles of 2(y) x 16(x)) and 32 * NT output channels.  Per 16-channel chunk the 18 x 18 halo sits in
// LDS as [hy][hx][16 bf16]: 32 bytes per pixel, 592 bytes per row (18 pixels + 16 bytes).  A lane's A fragment — 8 channels of one pixel
// — is one ds_read_b128; a 16-lane service group of that read covers 8 pixels of one row (even 16-byte slots) and 8 pixels of the next
// (odd slots, the row stride being an odd number of slots): 16 distinct slots of the 256-byte bank row, conflict-free at every tap.
// Double-buffered like the fp32 kernel: the next chunk's halo is in flight (registers) during the current chunk's 9 * 2 * NT MFMAs and
// stored to the other buffer after them, one barrier per chunk.  B fragments (16 bytes per lane) stream from the pre-swizzled packed
// image one tap ahead.  Small grids split the channel reduction over blocks and add the partial sums in a fixed order
// (conv2d_bf16_splitk_reduce_kernel).  With a residual (u3d_conv2d_bf16_res: conv3 of a ResNetBlock, `native_2d_residual_bf16: true` on a
// ResidualUNet2D) the epilogue that owns ReLU and statistics — the fused one, or the split-K reduction — adds the fp32 residual to the fp32
// sum first: out = [relu](conv + residual); it is read where the output is stored (lane = channel: 128 contiguous bytes per half-wave).
//
// Weight gradient (conv2d_wgrad_bf16_kernel): the contraction runs over PIXELS while both tensors are channel-innermost, so both operand
// fragments (8 pixels of one channel per lane) are transposed reads: the g halo and the dz tile sit in LDS as [pixel][32 channels] bf16
// and are fetched with ds_read_b64_tr_b16 (csrc/u3d_bf16.hip, tools/tr_probe.hip; the 32 lanes of one LDS cycle cover 4 pixels x 64
// contiguous bytes: conflict-free).  A block owns 32 output x 32 input channels x 9 taps and a contiguous range of pixel tiles; wave w
// takes rows 4w .. 4w + 3 of a tile, one 16-pixel row per MFMA k-step, one dz fragment feeding 9 taps.  Partial sums go to a workspace and
// are added in a fixed order (conv2d_wgrad_bf16_reduce_kernel): the same inputs give a bitwise-identical dW.
//
// Virtual concat (`native_2d_bf16_vcat`, the `_src` entry points): the first convolution of a decoder reads cat(skip, nearest(low)) through
// u3d_src_t — two base pointers and the nearest tables ymap / xmap — instead of a written-out copy.  Compile-time variants of the same
// kernels (template parameter V / VC and a parameter struct with the second base): with both halves % 32 channels a staged 16-channel
// chunk, a 32-channel weight-gradient block and a 32-channel n-tile of the data gradient's gx lie wholly in one source, so the choice
// is a uniform branch; the affine, the rounding and the zero padding stay in c2b_stage8.  The single-source instantiations are unchanged.
//
// Sub-pixel decoder convolutions (`native_2d_bf16_subpixel`, the u3d_subpixel2d_*_bf16 entry points at the end of this file): the upsampled
// half of a decoder's first convolution at an exact-2x level as four parity-class 2x2 convolutions over the low-res tensor.  Rounding
// points: WEIGHTS — the pre-summed taps are added in fp32 from the fp32 master weight and rounded once to bf16, nearest even, by
// pack_subpix2d_bf16_kernel; ACTIVATIONS and dz — once while staged to LDS, after the fp32 affine fmaf(x, a, b), through the same
// c2b_stage8 (zero padding applies after the affine and stays exactly 0).  The skip half runs the kernels above on channel-sliced images
// (u3d_pack_weights2d_bf16_slice, u3d_conv2d_wgrad_bf16_strided: the same kernels with a row stride, bit-identical at stride = Cin).
#include <algorithm>

#include "u3d_common.h"

typedef __bf16 c2b_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 c2b_bf16x4 __attribute__((ext_vector_type(4)));
typedef short c2b_s16x4 __attribute__((ext_vector_type(4)));
typedef short c2b_s16x8 __attribute__((ext_vector_type(8)));

namespace {

namespace c2b {
constexpr int TY = 16, TX = 16;          // output tile
constexpr int HY = TY + 2, HX = TX + 2;  // halo
constexpr int CC = 16;                   // input channels per chunk = one MFMA k-step per tap
constexpr int PS = 32;                   // bytes per staged pixel (16 bf16)
constexpr int RS = HX * PS + 16;         // 592 bytes per halo row: an odd number of 16-byte slots
constexpr int BUF = HY * RS;             // 10656 bytes per staging buffer
constexpr int NITEMS = HY * HX * 2;      // 648 (pixel, channel octet) items per chunk
constexpr int NIT = (NITEMS + 255) / 256;  // 3
constexpr int RED = 2 * BUF;             // [4 waves][NT <= 2][32][4] partial statistics (floats)
constexpr int LDS_BYTES = RED + 4 * 2 * 32 * 4 * 4;  // 25408
// weight gradient
constexpr int WCB = 32;                  // channels per block (both roles)
constexpr int WPP = 2 * WCB;             // bytes per staged pixel
constexpr int WG_G = 0;                  // [HY*HX][32] bf16 source halo
constexpr int WG_DZ = HY * HX * WPP;     // [TY*TX][32] bf16 dz tile
constexpr int WG_LDS_BYTES = WG_DZ + TY * TX * WPP;  // 37120 (the final [4][32][32] float reduction reuses the first 16384)
constexpr int WG_GIT = (HY * HX * 4 + 255) / 256;    // 6 halo items (pixel, octet) per thread
constexpr int WG_DIT = TY * TX * 4 / 256;            // 4 dz items per thread
constexpr int WG_GB = 2, WG_DB = 2;                  // items staged per batch
}  // namespace c2b

inline long long c2b_cdiv(long long a, long long b) { return (a + b - 1) / b; }

int c2b_cu_count(int device) {
    static int cached[64] = {0};
    if (device >= 0 && device < 64 && cached[device] > 0) return cached[device];
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
    if (device >= 0 && device < 64) cached[device] = n;
    return n;
}

inline bool c2b_fwd_ok(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 16 == 0 && Cout % 32 == 0; }
inline bool c2b_wgrad_ok(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0; }
// the `_c16` entry points (`native_2d_stem` next to `native_2d_bf16`): both channel counts % 16.  16 produced channels are half an n-tile:
// the image holds zeros there and the epilogue masks co >= Cout; the weight gradient stages zeros for the two missing channel octets
inline bool c2b_c16_ok(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 16 == 0 && Cout % 16 == 0; }
inline bool c2b_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

void c2b_dims(int Cin, int Cout, int mode, int& K, int& Nn) {
    K = mode == 0 ? Cin : Cout;
    Nn = mode == 0 ? Cout : Cin;
}

// 8 staged channels: affine in fp32 (one fused multiply-add per element), ONE rounding to bf16 (nearest even), zero outside the image
__device__ __forceinline__ c2b_bf16x8 c2b_stage8(const f32x4& lo, const f32x4& hi, const float* aff, bool ok) {
    f32x4 v0 = lo, v1 = hi;
    if (aff != nullptr) {
        const f32x4 q0 = u3d_ldq(aff), q1 = u3d_ldq(aff + 4), q2 = u3d_ldq(aff + 8), q3 = u3d_ldq(aff + 12);  // (a, b) pairs
        v0 = f32x4{fmaf(lo[0], q0[0], q0[1]), fmaf(lo[1], q0[2], q0[3]), fmaf(lo[2], q1[0], q1[1]), fmaf(lo[3], q1[2], q1[3])};
        v1 = f32x4{fmaf(hi[0], q2[0], q2[1]), fmaf(hi[1], q2[2], q2[3]), fmaf(hi[2], q3[0], q3[1]), fmaf(hi[3], q3[2], q3[3])};
    }
    if (!ok) v0 = v1 = f32x4{0.f, 0.f, 0.f, 0.f};  // padding stays exactly 0
    const c2b_bf16x4 b0 = __builtin_convertvector(v0, c2b_bf16x4), b1 = __builtin_convertvector(v1, c2b_bf16x4);
    return __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// =================================================================================================
// weight packing: image [chunk][tap][ntile][lane][8] of B[k][n]: lane l holds k = 16 * chunk + 8 * (l >> 5) + j, column n = 32 * ntile +
// (l & 31) — the B operand of v_mfma_f32_32x32x16_bf16; the A fragment of the same lane half is the 8 channels of its ds_read_b128.
//   mode 0 (forward): B[k = ci][n = co] = w[co][ci][tap]           mode 1 (data gradient): B[k = co][n = ci] = w[co][ci][8 - tap]
// (cs, coff: the input channels [coff, coff + Cin) of a (Cout, cs, 3, 3) weight — u3d_pack_weights2d_bf16_slice; cs = Cin, coff = 0: the whole)
__global__ void pack_weights2d_bf16_kernel(const float* __restrict__ w, int Cout, int Cin, int mode, int K, int Nn, int ntg,
                                           long long total, __bf16* __restrict__ packed, int cs, int coff) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        long long r = i >> 9;
        const int nt = (int)(r % ntg);
        r /= ntg;
        const int tap = (int)(r % 9);
        const int chunk = (int)(r / 9);
        const int k = chunk * c2b::CC + 8 * (lane >> 5) + j;
        const int nn = nt * 32 + (lane & 31);
        float v = 0.f;
        if (k < K && nn < Nn)
            v = mode == 0 ? w[((size_t)nn * cs + coff + k) * 9 + tap] : w[((size_t)k * cs + coff + nn) * 9 + (8 - tap)];
        packed[i] = (__bf16)v;
    }
}

// =================================================================================================
// forward / data gradient
struct Conv2dBf16Params {
    const float* x;       // (N,H,W,Cin) fp32
    const float* affine;  // (N,Cin,2) or null
    const c2b_bf16x8* wp;
    const float* gx;      // (N,H,W,Cout) fp32 or null
    const float* residual;  // (N,H,W,Cout) fp32 or null: added to the fp32 sum before the ReLU (never with gx)
    float* out;           // ksplit == 1: the output; else the workspace of partial sums [ksplit][N*H*W*Cout]
    double* out_stats;
    double* gstats;
    int N, H, W, Cin, Cout;
    int nchunks, ntg, ncb, ty, tx;
    int relu, stat_reps;
    int ksplit, cps;
    long long part_stride;
};

// ... of the `_src` entry points (`native_2d_bf16_vcat`): ONE of the two fp32 tensors is the virtual concat cat(skip, nearest(low)) of a
// decoder's first convolution, read through two bases — x in the forward (V = 1), gx in the data gradient (V = 2).  The base struct's
// pointer (x / gx) is the skip half (N,H,W,C0); channels [C0, C0 + C1) come from v1 (N,H1,W1,C1) at (ymap[y], xmap[x]).  Cin (V = 1) /
// Cout (V = 2) stay the concat width C0 + C1: the affine table, the weight image and dg are indexed by concat channel.
struct Conv2dBf16VParams : Conv2dBf16Params {
    const float* v1;
    const int32_t* ymap;
    const int32_t* xmap;
    int C0, C1, H1, W1;
};

// per-block statistics, as c2_flush_stats of csrc/u3d_conv2d.hip: column sums s[nt][0..3] = (sum v, sum v^2, sum v, sum v * gx) combined
// over the lane halves, over the 4 waves in LDS (fixed order), then one f64 atomic per (sample, channel, quantity) and block into replica
// row block % reps
template <int NT>
__device__ __forceinline__ void c2b_flush_stats(const Conv2dBf16Params& p, float* red, float (&s)[NT][4], int n, int cb, int t) {
    const int l = t & 63, w = t >> 6;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[nt][q] += __shfl_xor(s[nt][q], 32);
    if (l < 32)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[((w * NT + nt) * 32 + l) * 4 + q] = s[nt][q];
    __syncthreads();
    if (t < NT * 32) {
        const int nt = t >> 5, col = t & 31;
        const int co = (cb * NT + nt) * 32 + col;
        if (co < p.Cout) {
            float a[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                a[q] = ((red[((0 * NT + nt) * 32 + col) * 4 + q] + red[((1 * NT + nt) * 32 + col) * 4 + q]) +
                        red[((2 * NT + nt) * 32 + col) * 4 + q]) + red[((3 * NT + nt) * 32 + col) * 4 + q];
            const size_t row = (size_t)(blockIdx.x % p.stat_reps) * p.N * p.Cout;
            if (p.out_stats) {
                double* o = p.out_stats + (row + (size_t)n * p.Cout + co) * 2;
                u3d_atomic_add_f64(o, (double)a[0]);
                u3d_atomic_add_f64(o + 1, (double)a[1]);
            }
            if (p.gx) {
                double* o = p.gstats + (row + (size_t)n * p.Cout + co) * 2;
                u3d_atomic_add_f64(o, (double)a[2]);
                u3d_atomic_add_f64(o + 1, (double)a[3]);
            }
        }
    }
}

// V = 0: single tensors (P = Conv2dBf16Params, the kernels of u3d_conv2d_bf16 / _c16 / _res).  V = 1 / 2 (P = Conv2dBf16VParams): x / gx is
// a virtual concat.  C0 and C1 are multiples of 32, so a staged 16-channel chunk and a 32-channel n-tile lie wholly in one source: the
// choice is uniform over the block (per chunk) / over the n-tile and costs one scalar compare.
template <int NT, int V, typename P>
__global__ __launch_bounds__(256, 2) void conv2d_bf16_kernel(const P p) {
    constexpr bool VX = V == 1, VG = V == 2;
    using namespace c2b;
    extern __shared__ __attribute__((aligned(16))) char lds_c2b[];
    char* const lds = lds_c2b;
    const int t = threadIdx.x;
    const int l = t & 63, w = t >> 6, h = l >> 5;

    int logical = blockIdx.x;
    int ch0 = 0, nch = p.nchunks, split = 0;
    if (p.ksplit > 1) {
        split = logical % p.ksplit;
        ch0 = split * p.cps;
        nch = min(p.cps, p.nchunks - ch0);
        logical /= p.ksplit;
    }
    const int cb = logical % p.ncb;
    int tile = logical / p.ncb;
    const int txi = tile % p.tx;
    tile /= p.tx;
    const int tyi = tile % p.ty;
    const int n = tile / p.ty;
    const int y0 = tyi * TY, x0 = txi * TX;
    const int H = p.H, W = p.W, Cin = p.Cin;

    // ---- staging descriptors (constant across chunks): item = (halo pixel, channel octet q)
    int ldsoff[NIT], cqs[NIT];
    size_t goff[NIT];
    size_t goff1[VX ? NIT : 1];  // (V = 1) the same halo pixel in the low-res half, through the nearest maps
    bool oks[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int item = t + 256 * it;
        const bool in = item < NITEMS;
        const int pix = item >> 1, q = item & 1;
        const int hy = pix / HX, hx = pix - (pix / HX) * HX;
        const int gy = y0 - 1 + hy, gxx = x0 - 1 + hx;
        const bool ok = in && gy >= 0 && gy < H && gxx >= 0 && gxx < W;
        oks[it] = ok;
        ldsoff[it] = in ? hy * RS + hx * PS + 16 * q : -1;
        cqs[it] = 8 * q;
        if constexpr (VX) {
            goff[it] = ok ? ((size_t)(n * H + gy) * W + gxx) * p.C0 : 0;
            goff1[it] = ok ? ((size_t)(n * p.H1 + p.ymap[gy]) * p.W1 + p.xmap[gxx]) * p.C1 : 0;
        } else {
            goff[it] = ok ? ((size_t)(n * H + gy) * W + gxx) * Cin : 0;
        }
    }
    f32x4 raw[NIT][2];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            raw[it][0] = raw[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (oks[it]) {
                const float* src;
                if constexpr (VX) {  // (the chunk's source: block-uniform)
                    const int ch = c * CC;
                    src = (ch >= p.C0 ? p.v1 + goff1[it] + (ch - p.C0) : p.x + goff[it] + ch) + cqs[it];
                } else {
                    src = p.x + goff[it] + c * CC + cqs[it];
                }
                raw[it][0] = u3d_ldq(src);
                raw[it][1] = u3d_ldq(src + 4);
            }
        }
    };
    auto store_chunk = [&](int c, char* buf) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (ldsoff[it] < 0) continue;
            const float* aff = (p.affine != nullptr && oks[it]) ? p.affine + ((size_t)n * Cin + c * CC + cqs[it]) * 2 : nullptr;
            *reinterpret_cast<c2b_bf16x8*>(buf + ldsoff[it]) = c2b_stage8(raw[it][0], raw[it][1], aff, oks[it]);
        }
    };

    f32x16 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    // A-fragment base: lane (i = l & 31, h) of M-tile mt reads pixel (4w + 2mt + (i >> 4), i & 15), channels 8h .. 8h + 7
    const int i32 = l & 31;
    const int abase = (4 * w + (i32 >> 4)) * RS + (i32 & 15) * PS + 16 * h;
    // B image: [chunk][tap][ntg][lane] records of 8 bf16
    auto bidx = [&](int c, int tap, int nt) -> long long { return ((long long)(c * 9 + tap) * p.ntg + (cb * NT + nt)) * 64 + l; };
    const c2b_bf16x8 bzero = __builtin_bit_cast(c2b_bf16x8, f32x4{0.f, 0.f, 0.f, 0.f});

    load_chunk(ch0);
    store_chunk(ch0, lds);
    __syncthreads();
    for (int ci = 0; ci < nch; ++ci) {
        const int c = ch0 + ci;
        const char* cur = lds + (ci & 1) * BUF;
        if (ci + 1 < nch) load_chunk(c + 1);  // in flight during the k-loop
        c2b_bf16x8 bq[NT], bn[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bq[nt] = (cb * NT + nt < p.ntg) ? p.wp[bidx(c, 0, nt)] : bzero;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap - (tap / 3) * 3;
            if (tap + 1 < 9) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bn[nt] = (cb * NT + nt < p.ntg) ? p.wp[bidx(c, tap + 1, nt)] : bzero;
            }
            c2b_bf16x8 a[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) a[mt] = *reinterpret_cast<const c2b_bf16x8*>(cur + abase + (2 * mt + dy) * RS + dx * PS);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt], bq[nt], acc[mt][nt], 0, 0, 0);
            if (tap + 1 < 9) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bq[nt] = bn[nt];
            }
        }
        if (ci + 1 < nch) store_chunk(c + 1, lds + ((ci + 1) & 1) * BUF);  // (that buffer was last read in chunk ci - 1)
        __syncthreads();
    }

    // ---- epilogue: lane column = output channel (l & 31), register r = M row (r & 3) + 8 (r >> 2) + 4h
    float s[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[nt][q] = 0.f;
    float* const outp = p.out + (size_t)split * p.part_stride;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = (cb * NT + nt) * 32 + i32;
        if (co >= p.Cout) continue;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int y = y0 + 4 * w + 2 * mt + (row >> 4), x = x0 + (row & 15);
                if (y >= H || x >= W) continue;
                float v = acc[mt][nt][r];
                const size_t o = ((size_t)(n * H + y) * W + x) * p.Cout + co;
                if (p.ksplit > 1) {
                    outp[o] = v;
                    continue;
                }
                if (p.residual) v += p.residual[o];  // (uniform over the grid; the split-K partial sums above carry none)
                if (p.relu) v = fmaxf(v, 0.f);
                outp[o] = v;
                s[nt][0] += v;
                s[nt][1] += v * v;
                if (p.gx) {
                    s[nt][2] += v;
                    if constexpr (VG) {  // (the n-tile's source: uniform over the wave)
                        const float xv = (cb * NT + nt) * 32 >= p.C0
                                             ? p.v1[((size_t)(n * p.H1 + p.ymap[y]) * p.W1 + p.xmap[x]) * p.C1 + (co - p.C0)]
                                             : p.gx[((size_t)(n * H + y) * W + x) * p.C0 + co];
                        s[nt][3] += v * xv;
                    } else {
                        s[nt][3] += v * p.gx[o];
                    }
                }
            }
    }
    if (p.ksplit == 1 && (p.out_stats || p.gx)) c2b_flush_stats<NT>(p, reinterpret_cast<float*>(lds + RED), s, n, cb, t);
}

// split-K: out = [relu](sum over runs in run order [+ residual]), statistics as the main kernel (replica row 0).  Block = 64 pixels of one sample,
// threads walk the channels (coalesced), one f64 atomic per (block, channel, quantity).
__global__ __launch_bounds__(256) void conv2d_bf16_splitk_reduce_kernel(const float* __restrict__ part, long long part_stride, int ksplit,
                                                                        float* __restrict__ out, int P, int Cout, int relu,
                                                                        double* out_stats, const float* __restrict__ gx, double* gstats,
                                                                        const float* __restrict__ residual) {
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * 64, p1 = min(P, p0 + 64);
    for (int co = threadIdx.x; co < Cout; co += blockDim.x) {
        double s0 = 0.0, s1 = 0.0, g0 = 0.0, g1 = 0.0;
        for (int pp = p0; pp < p1; ++pp) {
            const size_t o = ((size_t)n * P + pp) * Cout + co;
            float v = 0.f;
            for (int k = 0; k < ksplit; ++k) v += part[(size_t)k * part_stride + o];
            if (residual) v += residual[o];
            if (relu) v = fmaxf(v, 0.f);
            out[o] = v;
            s0 += v;
            s1 += (double)v * v;
            if (gx) {
                g0 += v;
                g1 += (double)v * gx[o];
            }
        }
        if (out_stats) {
            u3d_atomic_add_f64(out_stats + ((size_t)n * Cout + co) * 2, s0);
            u3d_atomic_add_f64(out_stats + ((size_t)n * Cout + co) * 2 + 1, s1);
        }
        if (gx) {
            u3d_atomic_add_f64(gstats + ((size_t)n * Cout + co) * 2, g0);
            u3d_atomic_add_f64(gstats + ((size_t)n * Cout + co) * 2 + 1, g1);
        }
    }
}

// ... of u3d_conv2d_bf16_dgrad_src (a data gradient: no ReLU, no output statistics, no residual): the same sums in the same order, gx read
// as the virtual concat — skip half gx0 (N,H,W,C0), channels from C0 in gx1 (N,H1,W1,C1) through the nearest maps
__global__ __launch_bounds__(256) void conv2d_bf16_splitk_reduce_vsrc_kernel(const float* __restrict__ part, long long part_stride,
                                                                             int ksplit, float* __restrict__ out, int P, int Cout,
                                                                             double* gstats, const float* __restrict__ gx0,
                                                                             const float* __restrict__ gx1,
                                                                             const int32_t* __restrict__ ymap,
                                                                             const int32_t* __restrict__ xmap, int W, int C0, int C1,
                                                                             int H1, int W1) {
    const int n = blockIdx.y;
    const int p0 = blockIdx.x * 64, p1 = min(P, p0 + 64);
    for (int co = threadIdx.x; co < Cout; co += blockDim.x) {
        double g0 = 0.0, g1 = 0.0;
        for (int pp = p0; pp < p1; ++pp) {
            const size_t o = ((size_t)n * P + pp) * Cout + co;
            float v = 0.f;
            for (int k = 0; k < ksplit; ++k) v += part[(size_t)k * part_stride + o];
            out[o] = v;
            const int y = pp / W, x = pp - y * W;
            const float xv = co < C0 ? gx0[((size_t)n * P + pp) * C0 + co]
                                     : gx1[((size_t)(n * H1 + ymap[y]) * W1 + xmap[x]) * C1 + (co - C0)];
            g0 += v;
            g1 += (double)v * xv;
        }
        u3d_atomic_add_f64(gstats + ((size_t)n * Cout + co) * 2, g0);
        u3d_atomic_add_f64(gstats + ((size_t)n * Cout + co) * 2 + 1, g1);
    }
}

struct C2bPlan {
    int nt, ncb, ty, tx, ntg, nchunks, ksplit, cps;
};

C2bPlan c2b_plan(int device, int N, int H, int W, int Cin, int Cout) {
    C2bPlan pl;
    pl.ntg = (int)c2b_cdiv(Cout, 32);
    pl.ty = (int)c2b_cdiv(H, c2b::TY);
    pl.tx = (int)c2b_cdiv(W, c2b::TX);
    pl.nchunks = (int)c2b_cdiv(Cin, c2b::CC);
    const long long tiles = (long long)N * pl.ty * pl.tx;
    const int slots = 2 * c2b_cu_count(device);  // (the block count the fp32 kernel's plan fills the chip with)
    pl.nt = (pl.ntg >= 2 && tiles * c2b_cdiv(pl.ntg, 2) >= slots) ? 2 : 1;
    pl.ncb = (int)c2b_cdiv(pl.ntg, pl.nt);
    const long long blocks = tiles * pl.ncb;
    pl.ksplit = 1;
    pl.cps = pl.nchunks;
    if (blocks < slots / 2 && pl.nchunks >= 2) {  // bottom of the U: fewer blocks than CUs -> split the channel reduction
        int ks = (int)std::min<long long>(pl.nchunks, c2b_cdiv(slots, blocks));
        pl.cps = (int)c2b_cdiv(pl.nchunks, ks);
        pl.ksplit = (int)c2b_cdiv(pl.nchunks, pl.cps);
    }
    return pl;
}

// the split a launch really uses: the plan's, when the caller brought the scratch for it; else the unsplit kernel with its fused epilogue
// (ONE statement for the launcher and the host-only query u3d_conv2d_bf16_variant)
inline int c2b_launch_ksplit(const C2bPlan& pl, bool has_workspace) { return (pl.ksplit > 1 && has_workspace) ? pl.ksplit : 1; }

// =================================================================================================
// weight gradient: dw[co][ci][tap] = sum_{n,y,x} dz[n,y,x,co] * g[n, y + dy - 1, x + dx - 1, ci], g = affine(x), zero padded.
// MFMA: M = 32 output channels (A = dz), N = 32 input channels (B = g), K = 16 pixels of one tile row; the same A fragment feeds 9 taps.
struct Wgrad2dBf16Params {
    const float* x;
    const float* affine;
    const float* dz;
    float* dst;  // nsplit == 1: dw; else workspace [nsplit][Cout][Cin][9]
    int N, H, W, Cin, Cout;
    int ty, tx, ncob, ncib, ntiles, tps;
    int dstride;  // input channels per output channel of dst: Cin, or dw_cin_stride of u3d_conv2d_wgrad_bf16_strided writing dw directly
};

// ... of u3d_conv2d_wgrad_bf16_src: x is the skip half (N,H,W,C0), channels [C0, C0 + C1) of the virtual concat come from v1 (N,H1,W1,C1)
// through the nearest maps; Cin = C0 + C1 (affine rows, dw layout).  A block's 32 input channels lie wholly in one source.
struct Wgrad2dBf16VParams : Wgrad2dBf16Params {
    const float* v1;
    const int32_t* ymap;
    const int32_t* xmap;
    int C0, C1, H1, W1;
};

// two transposed reads of a [pixel][32 channels] bf16 image (64 bytes per pixel): pixels +0..3 and +4..7 of this lane's 8-pixel half.
// (Every lane of the wave must be active: the gather crosses lanes.)
__device__ __forceinline__ c2b_bf16x8 c2b_tr_frag(const char* lds_addr) {
    const c2b_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) c2b_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)lds_addr);
    const c2b_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) c2b_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)(lds_addr + 4 * c2b::WPP));
    const c2b_s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(c2b_bf16x8, v);
}

template <bool VC, typename P>
__global__ __launch_bounds__(256, 2) void conv2d_wgrad_bf16_kernel(const P p) {
    using namespace c2b;
    extern __shared__ __attribute__((aligned(16))) char lds_w2b[];
    char* const lds = lds_w2b;
    const int t = threadIdx.x, l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int b = blockIdx.x;
    const int cib = b % p.ncib;
    b /= p.ncib;
    const int cob = b % p.ncob;
    const int split = b / p.ncob;
    const int ci0 = cib * WCB, co0 = cob * WCB;
    const int tile0 = split * p.tps, tile1 = min(p.ntiles, tile0 + p.tps);
    const int H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout;
    char* const gl = lds + WG_G;
    char* const dzl = lds + WG_DZ;

    f32x16 acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    // transposed-read lane offset: source lane s of a 16-lane group addresses 4 channels of pixel (s >> 2); lane l receives channel
    // (l & 31) of the 8 pixels 8 * (l >> 5) .. + 7
    const int g4 = l >> 4, sidx = l & 15;
    const int lane_off = (8 * (g4 >> 1) + (sidx >> 2)) * WPP + (16 * (g4 & 1) + 4 * (sidx & 3)) * 2;

    for (int tile = tile0; tile < tile1; ++tile) {
        int tt = tile;
        const int txi = tt % p.tx;
        tt /= p.tx;
        const int tyi = tt % p.ty;
        const int n = tt / p.ty;
        const int y0 = tyi * TY, x0 = txi * TX;
        // stage g (18 x 18 halo, 32 channels from ci0, affine, zero padding) and dz (16 x 16, 32 channels from co0), a few items at a
        // time (loads first, then the conversions and LDS stores): the 9 accumulators leave ~100 registers for the staging
        auto stage_g = [&](int it0) {
            f32x4 rg[WG_GB][2];
            bool okg[WG_GB];
#pragma unroll
            for (int k = 0; k < WG_GB; ++k) {
                const int item = t + 256 * (it0 + k);
                const int pix = item >> 2, q = item & 3;
                const int hy = pix / HX, hx = pix - (pix / HX) * HX;
                const int gy = y0 - 1 + hy, gxx = x0 - 1 + hx;
                // (ci0 + 8q >= Cin: the missing channel octets of a 16-channel cell are staged as zeros, `_c16`)
                okg[k] = item < HY * HX * 4 && gy >= 0 && gy < H && gxx >= 0 && gxx < W && ci0 + 8 * q < Cin;
                rg[k][0] = rg[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (okg[k]) {
                    const float* src;
                    if constexpr (VC) {  // (the channel block's source: block-uniform)
                        src = (ci0 >= p.C0 ? p.v1 + ((size_t)(n * p.H1 + p.ymap[gy]) * p.W1 + p.xmap[gxx]) * p.C1 + (ci0 - p.C0)
                                           : p.x + ((size_t)(n * H + gy) * W + gxx) * p.C0 + ci0) + 8 * q;
                    } else {
                        src = p.x + ((size_t)(n * H + gy) * W + gxx) * Cin + ci0 + 8 * q;
                    }
                    rg[k][0] = u3d_ldq(src);
                    rg[k][1] = u3d_ldq(src + 4);
                }
            }
#pragma unroll
            for (int k = 0; k < WG_GB; ++k) {
                const int item = t + 256 * (it0 + k);
                if (item >= HY * HX * 4) continue;
                const int q = item & 3;
                const float* aff = (p.affine != nullptr && okg[k]) ? p.affine + ((size_t)n * Cin + ci0 + 8 * q) * 2 : nullptr;
                *reinterpret_cast<c2b_bf16x8*>(gl + (item >> 2) * WPP + 16 * q) = c2b_stage8(rg[k][0], rg[k][1], aff, okg[k]);
            }
        };
        auto stage_dz = [&](int it0) {
            f32x4 rd[WG_DB][2];
            bool okd[WG_DB];
#pragma unroll
            for (int k = 0; k < WG_DB; ++k) {
                const int item = t + 256 * (it0 + k);
                const int pix = item >> 2, q = item & 3;
                const int y = y0 + (pix >> 4), x = x0 + (pix & 15);
                okd[k] = y < H && x < W && co0 + 8 * q < Cout;
                rd[k][0] = rd[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (okd[k]) {
                    const float* src = p.dz + ((size_t)(n * H + y) * W + x) * Cout + co0 + 8 * q;
                    rd[k][0] = u3d_ldq(src);
                    rd[k][1] = u3d_ldq(src + 4);
                }
            }
#pragma unroll
            for (int k = 0; k < WG_DB; ++k) {
                const int item = t + 256 * (it0 + k);
                *reinterpret_cast<c2b_bf16x8*>(dzl + (item >> 2) * WPP + 16 * (item & 3)) = c2b_stage8(rd[k][0], rd[k][1], nullptr, okd[k]);
            }
        };
        for (int it0 = 0; it0 < WG_GIT; it0 += WG_GB) stage_g(it0);
        for (int it0 = 0; it0 < WG_DIT; it0 += WG_DB) stage_dz(it0);
        __syncthreads();
        // wave w: rows 4w .. 4w + 3 of the tile, one 16-pixel row per k-step
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {  // (not unrolled: 40 fragment reads in flight would push the 9 accumulators out of the registers)
            const int py = 4 * w + r;
            const c2b_bf16x8 a = c2b_tr_frag(dzl + py * TX * WPP + lane_off);
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const c2b_bf16x8 g = c2b_tr_frag(gl + ((py + dy) * HX + dx) * WPP + lane_off);
                    acc[dy * 3 + dx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, g, acc[dy * 3 + dx], 0, 0, 0);
                }
        }
        __syncthreads();
    }

    // ---- add the 4 waves' partial sums in a fixed order, one tap at a time, through LDS; write [co][ci][tap]
    float* red = reinterpret_cast<float*>(lds);  // [4][32][32]
    for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;  // output channel within the block
            red[(w * 32 + row) * 32 + i32] = acc[tap][r];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = t + 256 * e;  // (row, col) of the 32 x 32 tile
            const int row = idx >> 5, col = idx & 31;
            const float v = ((red[(0 * 32 + row) * 32 + col] + red[(1 * 32 + row) * 32 + col]) + red[(2 * 32 + row) * 32 + col]) +
                            red[(3 * 32 + row) * 32 + col];
            const int co = co0 + row, ci = ci0 + col;
            if (co < Cout && ci < Cin) p.dst[(size_t)split * Cout * Cin * 9 + ((size_t)co * p.dstride + ci) * 9 + tap] = v;
        }
        __syncthreads();
    }
}

// dw[i] = sum over splits in split order (bitwise-reproducible); row = 9 * Cin elements per output channel, drow = 9 * dw_cin_stride
__global__ void conv2d_wgrad_bf16_reduce_kernel(const float* __restrict__ ws, int nsplit, long long total, float* __restrict__ dw, int row,
                                                int drow) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) v += ws[(size_t)s * total + i];
        dw[row == drow ? i : (i / row) * drow + i % row] = v;
    }
}

struct W2bPlan {
    int ty, tx, ncob, ncib, ntiles, tps, nsplit;
};

W2bPlan w2b_plan(int device, int N, int H, int W, int Cin, int Cout) {
    W2bPlan pl;
    pl.ty = (int)c2b_cdiv(H, c2b::TY);
    pl.tx = (int)c2b_cdiv(W, c2b::TX);
    pl.ncob = (int)c2b_cdiv(Cout, c2b::WCB);
    pl.ncib = (int)c2b_cdiv(Cin, c2b::WCB);
    pl.ntiles = N * pl.ty * pl.tx;
    const long long cells = (long long)pl.ncob * pl.ncib;
    const long long target = 4LL * c2b_cu_count(device);  // ~4 blocks per CU over the launch
    long long ns = std::max<long long>(1, std::min<long long>(pl.ntiles, c2b_cdiv(target, cells)));
    pl.tps = (int)c2b_cdiv(pl.ntiles, ns);
    pl.nsplit = (int)c2b_cdiv(pl.ntiles, pl.tps);
    return pl;
}

int c2b_current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return dev;
}

}  // namespace

extern "C" int u3d_conv2d_bf16_supported(int Cin, int Cout) { return c2b_fwd_ok(Cin, Cout) ? 1 : 0; }

extern "C" int u3d_conv2d_wgrad_bf16_supported(int Cin, int Cout) { return c2b_wgrad_ok(Cin, Cout) ? 1 : 0; }

extern "C" int u3d_conv2d_bf16_c16_supported(int Cin, int Cout) { return c2b_c16_ok(Cin, Cout) ? 1 : 0; }

extern "C" int u3d_conv2d_wgrad_bf16_c16_supported(int Cin, int Cout) { return c2b_c16_ok(Cin, Cout) ? 1 : 0; }

namespace {

// envelope of an entry point: today's (forward: contraction % 16, produced % 32; weight gradient: both % 32) or the `_c16` one
inline bool c2b_env_fwd(int Cin, int Cout, bool c16) { return c16 ? c2b_c16_ok(Cin, Cout) : c2b_fwd_ok(Cin, Cout); }
inline bool c2b_env_wgrad(int Cin, int Cout, bool c16) { return c16 ? c2b_c16_ok(Cin, Cout) : c2b_wgrad_ok(Cin, Cout); }

long long c2b_packed_elems(int Cin, int Cout, int mode, bool c16) {
    if (mode != 0 && mode != 1) return 0;
    int K, Nn;
    c2b_dims(Cin, Cout, mode, K, Nn);
    if (!c2b_env_fwd(K, Nn, c16)) return 0;
    return (long long)(K / c2b::CC) * 9 * c2b_cdiv(Nn, 32) * 64 * 8;  // (a half n-tile is stored whole, its upper columns zero)
}

int c2b_pack_launch(const char* who, int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, void* packed, bool c16,
                    int cin_stride = 0, int c_off = 0) {
    U3D_ENTER(device);
    U3D_REQUIRE(w && packed && Cout > 0 && Cin > 0 && (mode == 0 || mode == 1), "%s: bad argument", who);
    if (cin_stride == 0) cin_stride = Cin;
    U3D_REQUIRE(c_off >= 0 && c_off + Cin <= cin_stride, "%s: channels [%d, %d) do not lie inside a weight of %d input channels", who, c_off,
                c_off + Cin, cin_stride);
    int K, Nn;
    c2b_dims(Cin, Cout, mode, K, Nn);
    U3D_REQUIRE(c2b_env_fwd(K, Nn, c16), "%s: mode %d of a (%d -> %d) weight is outside the bf16 envelope (contraction %% 16, "
                "produced %% %d)", who, mode, Cin, Cout, c16 ? 16 : 32);
    U3D_REQUIRE(c2b_aligned(packed), "%s: the image must be 16-byte aligned", who);
    const long long total = c2b_packed_elems(Cin, Cout, mode, c16);
    long long blocks = c2b_cdiv(total, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_weights2d_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin, mode, K, Nn,
                       (int)c2b_cdiv(Nn, 32), total, reinterpret_cast<__bf16*>(packed), cin_stride, c_off);
    U3D_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" long long u3d_packed_weight2d_bf16_elems(int Cin, int Cout, int mode) { return c2b_packed_elems(Cin, Cout, mode, false); }

extern "C" long long u3d_packed_weight2d_bf16_c16_elems(int Cin, int Cout, int mode) { return c2b_packed_elems(Cin, Cout, mode, true); }

extern "C" int u3d_pack_weights2d_bf16(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, void* packed) {
    return c2b_pack_launch("u3d_pack_weights2d_bf16", device, stream, w, Cout, Cin, mode, packed, false);
}

// ... of the input channels [c_off, c_off + Cin) of a (Cout, cin_stride, 3, 3) weight (the skip half of a sub-pixel decoder layer): the
// image of a (Cout, Cin, 3, 3) weight holding those channels; c_off = 0, cin_stride = Cin is u3d_pack_weights2d_bf16 bit for bit
extern "C" int u3d_pack_weights2d_bf16_slice(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, int cin_stride,
                                             int c_off, void* packed) {
    U3D_REQUIRE(cin_stride > 0, "u3d_pack_weights2d_bf16_slice: bad argument");
    return c2b_pack_launch("u3d_pack_weights2d_bf16_slice", device, stream, w, Cout, Cin, mode, packed, false, cin_stride, c_off);
}

// ... of a layer with both channel counts % 16: the same fragment layout (for produced channels % 32 the same image bit for bit)
extern "C" int u3d_pack_weights2d_bf16_c16(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, void* packed) {
    return c2b_pack_launch("u3d_pack_weights2d_bf16_c16", device, stream, w, Cout, Cin, mode, packed, true);
}

namespace {

long long c2b_fwd_workspace(int N, int H, int W, int Cin, int Cout, bool c16) {
    if (N <= 0 || H <= 0 || W <= 0 || !c2b_env_fwd(Cin, Cout, c16)) return 0;
    const C2bPlan pl = c2b_plan(c2b_current_device(), N, H, W, Cin, Cout);
    return pl.ksplit > 1 ? (long long)pl.ksplit * N * H * W * Cout : 0;
}

int c2b_fwd_variant(int N, int H, int W, int Cin, int Cout, int has_workspace, bool c16) {
    if (N <= 0 || H <= 0 || W <= 0 || !c2b_env_fwd(Cin, Cout, c16)) return -1;
    const C2bPlan pl = c2b_plan(c2b_current_device(), N, H, W, Cin, Cout);
    return (c2b_launch_ksplit(pl, has_workspace != 0) << 8) | pl.nt;
}

}  // namespace

extern "C" long long u3d_conv2d_bf16_workspace_floats(int N, int H, int W, int Cin, int Cout) {
    return c2b_fwd_workspace(N, H, W, Cin, Cout, false);
}

extern "C" long long u3d_conv2d_bf16_c16_workspace_floats(int N, int H, int W, int Cin, int Cout) {
    return c2b_fwd_workspace(N, H, W, Cin, Cout, true);
}

// host-only query of that plan (tests assert that the shapes they pin really run the variants a full-resolution level runs)
extern "C" int u3d_conv2d_bf16_variant(int N, int H, int W, int Cin, int Cout, int has_workspace) {
    return c2b_fwd_variant(N, H, W, Cin, Cout, has_workspace, false);
}

extern "C" int u3d_conv2d_bf16_c16_variant(int N, int H, int W, int Cin, int Cout, int has_workspace) {
    return c2b_fwd_variant(N, H, W, Cin, Cout, has_workspace, true);
}

namespace {

// envelope of a virtual source of the `_src` entry points: both halves present and % 32 (a chunk, an n-tile and a weight-gradient
// channel block then lie in one source), D1 = 1, the two index tables, 16-byte aligned halves
inline bool c2b_vsrc_ok(const u3d_src_t* s) {
    return s && s->p0 && s->p1 && s->ymap && s->xmap && s->C0 > 0 && s->C1 > 0 && s->C0 % 32 == 0 && s->C1 % 32 == 0 && s->D1 == 1 &&
           s->H1 > 0 && s->W1 > 0 && c2b_aligned(s->p0) && c2b_aligned(s->p1);
}

// the one launcher behind u3d_conv2d_bf16 (residual == nullptr), u3d_conv2d_bf16_res and the `_src` entry points: same plan, same
// kernels.  vmode 1: x is the virtual concat `vsrc` (x == vsrc->p0); vmode 2: gx is (gx == vsrc->p0); 0: single tensors
int c2b_conv2d_launch(const char* who, int device, u3d_stream_t stream, const float* x, const float* affine, const void* packed_w,
                      float* out, int N, int H, int W, int Cin, int Cout, int relu, double* out_stats, const float* gx, double* gstats,
                      float* workspace, long long workspace_floats, int stat_reps, const float* residual, bool c16 = false,
                      int vmode = 0, const u3d_src_t* vsrc = nullptr) {
    U3D_ENTER(device);
    U3D_REQUIRE(c2b_env_fwd(Cin, Cout, c16), "%s: (%d -> %d) channels are outside the bf16 envelope (Cin %% 16, Cout %% %d)", who, Cin,
                Cout, c16 ? 16 : 32);
    U3D_REQUIRE(x && packed_w && out && N > 0 && H > 0 && W > 0 && stat_reps >= 1 && (long long)N * H * W < (1LL << 31),
                "%s: bad argument", who);
    U3D_REQUIRE(!gx || gstats, "%s: gx needs gstats", who);
    U3D_REQUIRE(c2b_aligned(x) && c2b_aligned(affine) && c2b_aligned(packed_w) && c2b_aligned(out) && c2b_aligned(workspace) &&
                    c2b_aligned(residual),
                "%s: pointers must be 16-byte aligned", who);
    const C2bPlan pl = c2b_plan(device, N, H, W, Cin, Cout);
    const long long need = pl.ksplit > 1 ? (long long)pl.ksplit * N * H * W * Cout : 0;
    const int ksplit = c2b_launch_ksplit(pl, workspace != nullptr);
    const bool split = ksplit > 1;
    U3D_REQUIRE(!split || workspace_floats >= need, "%s: workspace too small (%lld < %lld floats)", who, workspace_floats,
                need);
    Conv2dBf16Params p = {};
    p.x = x;
    p.affine = affine;
    p.wp = reinterpret_cast<const c2b_bf16x8*>(packed_w);
    p.gx = gx;
    p.residual = residual;
    p.out = split ? workspace : out;
    p.out_stats = out_stats;
    p.gstats = gstats;
    p.N = N, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout;
    p.nchunks = pl.nchunks, p.ntg = pl.ntg, p.ncb = pl.ncb, p.ty = pl.ty, p.tx = pl.tx;
    p.relu = relu ? 1 : 0;
    p.stat_reps = stat_reps;
    p.ksplit = ksplit;
    p.cps = split ? pl.cps : pl.nchunks;
    p.part_stride = (long long)N * H * W * Cout;
    const long long blocks = (long long)N * pl.ty * pl.tx * pl.ncb * p.ksplit;
    U3D_REQUIRE(blocks < (1LL << 31), "%s: grid too large", who);
    const dim3 grid((unsigned)blocks), block(256);
    if (vmode == 0) {
        if (pl.nt == 2)
            hipLaunchKernelGGL((conv2d_bf16_kernel<2, 0, Conv2dBf16Params>), grid, block, c2b::LDS_BYTES, (hipStream_t)stream, p);
        else
            hipLaunchKernelGGL((conv2d_bf16_kernel<1, 0, Conv2dBf16Params>), grid, block, c2b::LDS_BYTES, (hipStream_t)stream, p);
    } else {
        Conv2dBf16VParams vp = {};
        static_cast<Conv2dBf16Params&>(vp) = p;
        vp.v1 = vsrc->p1, vp.ymap = vsrc->ymap, vp.xmap = vsrc->xmap;
        vp.C0 = vsrc->C0, vp.C1 = vsrc->C1, vp.H1 = vsrc->H1, vp.W1 = vsrc->W1;
        if (vmode == 1 && pl.nt == 2)
            hipLaunchKernelGGL((conv2d_bf16_kernel<2, 1, Conv2dBf16VParams>), grid, block, c2b::LDS_BYTES, (hipStream_t)stream, vp);
        else if (vmode == 1)
            hipLaunchKernelGGL((conv2d_bf16_kernel<1, 1, Conv2dBf16VParams>), grid, block, c2b::LDS_BYTES, (hipStream_t)stream, vp);
        else if (pl.nt == 2)
            hipLaunchKernelGGL((conv2d_bf16_kernel<2, 2, Conv2dBf16VParams>), grid, block, c2b::LDS_BYTES, (hipStream_t)stream, vp);
        else
            hipLaunchKernelGGL((conv2d_bf16_kernel<1, 2, Conv2dBf16VParams>), grid, block, c2b::LDS_BYTES, (hipStream_t)stream, vp);
    }
    U3D_LAUNCH_CHECK();
    if (split) {
        const int P = H * W;
        if (vmode == 2)
            hipLaunchKernelGGL(conv2d_bf16_splitk_reduce_vsrc_kernel, dim3((unsigned)c2b_cdiv(P, 64), N), dim3(256), 0, (hipStream_t)stream,
                               workspace, p.part_stride, p.ksplit, out, P, Cout, gstats, vsrc->p0, vsrc->p1, vsrc->ymap, vsrc->xmap, W,
                               vsrc->C0, vsrc->C1, vsrc->H1, vsrc->W1);
        else
            hipLaunchKernelGGL(conv2d_bf16_splitk_reduce_kernel, dim3((unsigned)c2b_cdiv(P, 64), N), dim3(256), 0, (hipStream_t)stream,
                               workspace, p.part_stride, p.ksplit, out, P, Cout, p.relu, out_stats, gx, gstats, residual);
        U3D_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

extern "C" int u3d_conv2d_bf16(int device, u3d_stream_t stream, const float* x, const float* affine, const void* packed_w, float* out,
                               int N, int H, int W, int Cin, int Cout, int relu, double* out_stats, const float* gx, double* gstats,
                               float* workspace, long long workspace_floats, int stat_reps) {
    return c2b_conv2d_launch("u3d_conv2d_bf16", device, stream, x, affine, packed_w, out, N, H, W, Cin, Cout, relu, out_stats, gx, gstats,
                             workspace, workspace_floats, stat_reps, nullptr);
}

// the same launch for a layer with both channel counts % 16 (image of u3d_pack_weights2d_bf16_c16): the kernels mask co >= Cout
extern "C" int u3d_conv2d_bf16_c16(int device, u3d_stream_t stream, const float* x, const float* affine, const void* packed_w, float* out,
                                   int N, int H, int W, int Cin, int Cout, int relu, double* out_stats, const float* gx, double* gstats,
                                   float* workspace, long long workspace_floats, int stat_reps) {
    return c2b_conv2d_launch("u3d_conv2d_bf16_c16", device, stream, x, affine, packed_w, out, N, H, W, Cin, Cout, relu, out_stats, gx, gstats,
                             workspace, workspace_floats, stat_reps, nullptr, true);
}

// out = [relu](conv2d(bf16(a*x + b), bf16(w)) + residual): the bf16 twin of u3d_conv2d_res_reps.  The plan (u3d_conv2d_bf16_variant,
// u3d_conv2d_bf16_workspace_floats) does not depend on the residual.
extern "C" int u3d_conv2d_bf16_res(int device, u3d_stream_t stream, const float* x, const float* affine, const void* packed_w, float* out,
                                   int N, int H, int W, int Cin, int Cout, int relu, double* out_stats, const float* gx, double* gstats,
                                   float* workspace, long long workspace_floats, int stat_reps, const float* residual) {
    U3D_REQUIRE(residual && !gx && !gstats, "u3d_conv2d_bf16_res: needs a residual, and a residual excludes gx / gstats");
    return c2b_conv2d_launch("u3d_conv2d_bf16_res", device, stream, x, affine, packed_w, out, N, H, W, Cin, Cout, relu, out_stats, nullptr,
                             nullptr, workspace, workspace_floats, stat_reps, residual);
}

// ---- the `_src` entry points (`native_2d_bf16_vcat`): the first convolution of a decoder reads its input cat(skip, nearest(low)) through
// two bases instead of a written-out copy.  Same plans (they depend on (N, H, W, C0 + C1, Cout) only), same images, same staged values.
extern "C" int u3d_conv2d_bf16_src(int device, u3d_stream_t stream, const u3d_src_t* src, const void* packed_w, float* out, int N, int H,
                                   int W, int Cout, int relu, double* out_stats, float* workspace, long long workspace_floats,
                                   int stat_reps) {
    U3D_REQUIRE(c2b_vsrc_ok(src), "u3d_conv2d_bf16_src: needs a virtual source with C0 %% 32 == 0, C1 %% 32 == 0, C0 > 0, C1 > 0 (C1 == 0 is "
                "u3d_conv2d_bf16), D1 == 1, ymap / xmap and 16-byte aligned halves");
    return c2b_conv2d_launch("u3d_conv2d_bf16_src", device, stream, src->p0, src->affine, packed_w, out, N, H, W, src->C0 + src->C1, Cout,
                             relu, out_stats, nullptr, nullptr, workspace, workspace_floats, stat_reps, nullptr, false, 1, src);
}

// dg (N,H,W,C0 + C1) = the data gradient of that layer from dz (N,H,W,Cout) with the mode-1 image; gstats += (sum dg, sum dg * gx) with gx
// the VIRTUAL forward input (its affine field is ignored)
extern "C" int u3d_conv2d_bf16_dgrad_src(int device, u3d_stream_t stream, const float* dz, const void* packed_w, float* dg, int N, int H,
                                         int W, int Cout, const u3d_src_t* gx, double* gstats, float* workspace,
                                         long long workspace_floats, int stat_reps) {
    U3D_REQUIRE(c2b_vsrc_ok(gx), "u3d_conv2d_bf16_dgrad_src: gx must be a virtual source with C0 %% 32 == 0, C1 %% 32 == 0, C0 > 0, C1 > 0, "
                "D1 == 1, ymap / xmap and 16-byte aligned halves");
    U3D_REQUIRE(gstats, "u3d_conv2d_bf16_dgrad_src: gx needs gstats");
    return c2b_conv2d_launch("u3d_conv2d_bf16_dgrad_src", device, stream, dz, nullptr, packed_w, dg, N, H, W, Cout, gx->C0 + gx->C1, 0,
                             nullptr, gx->p0, gstats, workspace, workspace_floats, stat_reps, nullptr, false, 2, gx);
}

namespace {

long long c2b_wgrad_workspace(int N, int H, int W, int Cin, int Cout, bool c16) {
    if (N <= 0 || H <= 0 || W <= 0 || !c2b_env_wgrad(Cin, Cout, c16)) return 0;
    const W2bPlan pl = w2b_plan(c2b_current_device(), N, H, W, Cin, Cout);
    return pl.nsplit > 1 ? (long long)pl.nsplit * Cout * Cin * 9 : 0;
}

int c2b_wgrad_variant(int N, int H, int W, int Cin, int Cout, bool c16) {
    if (N <= 0 || H <= 0 || W <= 0 || !c2b_env_wgrad(Cin, Cout, c16)) return -1;
    const W2bPlan pl = w2b_plan(c2b_current_device(), N, H, W, Cin, Cout);
    return (std::min(pl.tps, 0x7fff) << 16) | std::min(pl.nsplit, 0xffff);
}

int c2b_wgrad_launch(const char* who, int device, u3d_stream_t stream, const float* x, const float* affine, const float* dz, float* dw,
                     int N, int H, int W, int Cin, int Cout, float* workspace, long long workspace_floats, bool c16,
                     const u3d_src_t* vsrc = nullptr, int dw_cin_stride = 0) {
    U3D_ENTER(device);
    if (dw_cin_stride == 0) dw_cin_stride = Cin;
    U3D_REQUIRE(dw_cin_stride >= Cin, "%s: dw_cin_stride %d is smaller than Cin %d", who, dw_cin_stride, Cin);
    U3D_REQUIRE(c2b_env_wgrad(Cin, Cout, c16), "%s: (%d -> %d) channels are outside the bf16 envelope (both %% %d)", who, Cin, Cout,
                c16 ? 16 : 32);
    U3D_REQUIRE(x && dz && dw && N > 0 && H > 0 && W > 0 && (long long)N * H * W < (1LL << 31), "%s: bad argument", who);
    U3D_REQUIRE(c2b_aligned(x) && c2b_aligned(affine) && c2b_aligned(dz), "%s: pointers must be 16-byte aligned", who);
    const W2bPlan pl = w2b_plan(device, N, H, W, Cin, Cout);
    const long long need = pl.nsplit > 1 ? (long long)pl.nsplit * Cout * Cin * 9 : 0;
    U3D_REQUIRE(need == 0 || (workspace && workspace_floats >= need), "%s: workspace too small (%lld < %lld floats)", who,
                workspace_floats, need);
    Wgrad2dBf16Params p = {};
    p.x = x;
    p.affine = affine;
    p.dz = dz;
    p.dst = need ? workspace : dw;
    p.N = N, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout;
    p.ty = pl.ty, p.tx = pl.tx, p.ncob = pl.ncob, p.ncib = pl.ncib, p.ntiles = pl.ntiles, p.tps = pl.tps;
    p.dstride = need ? Cin : dw_cin_stride;
    const long long blocks = (long long)pl.nsplit * pl.ncob * pl.ncib;
    U3D_REQUIRE(blocks < (1LL << 31), "%s: grid too large", who);
    if (vsrc == nullptr) {
        hipLaunchKernelGGL((conv2d_wgrad_bf16_kernel<false, Wgrad2dBf16Params>), dim3((unsigned)blocks), dim3(256), c2b::WG_LDS_BYTES,
                           (hipStream_t)stream, p);
    } else {  // (x == vsrc->p0: the skip half)
        Wgrad2dBf16VParams vp = {};
        static_cast<Wgrad2dBf16Params&>(vp) = p;
        vp.v1 = vsrc->p1, vp.ymap = vsrc->ymap, vp.xmap = vsrc->xmap;
        vp.C0 = vsrc->C0, vp.C1 = vsrc->C1, vp.H1 = vsrc->H1, vp.W1 = vsrc->W1;
        hipLaunchKernelGGL((conv2d_wgrad_bf16_kernel<true, Wgrad2dBf16VParams>), dim3((unsigned)blocks), dim3(256), c2b::WG_LDS_BYTES,
                           (hipStream_t)stream, vp);
    }
    U3D_LAUNCH_CHECK();
    if (need) {
        const long long total = (long long)Cout * Cin * 9;
        long long rb = c2b_cdiv(total, 256);
        if (rb > 4096) rb = 4096;
        hipLaunchKernelGGL(conv2d_wgrad_bf16_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace, pl.nsplit, total,
                           dw, 9 * Cin, 9 * dw_cin_stride);
        U3D_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

extern "C" long long u3d_wgrad2d_bf16_workspace_floats(int N, int H, int W, int Cin, int Cout) {
    return c2b_wgrad_workspace(N, H, W, Cin, Cout, false);
}

extern "C" long long u3d_wgrad2d_bf16_c16_workspace_floats(int N, int H, int W, int Cin, int Cout) {
    return c2b_wgrad_workspace(N, H, W, Cin, Cout, true);
}

extern "C" int u3d_conv2d_wgrad_bf16_variant(int N, int H, int W, int Cin, int Cout) { return c2b_wgrad_variant(N, H, W, Cin, Cout, false); }

extern "C" int u3d_conv2d_wgrad_bf16_c16_variant(int N, int H, int W, int Cin, int Cout) {
    return c2b_wgrad_variant(N, H, W, Cin, Cout, true);
}

extern "C" int u3d_conv2d_wgrad_bf16(int device, u3d_stream_t stream, const float* x, const float* affine, const float* dz, float* dw,
                                     int N, int H, int W, int Cin, int Cout, float* workspace, long long workspace_floats) {
    return c2b_wgrad_launch("u3d_conv2d_wgrad_bf16", device, stream, x, affine, dz, dw, N, H, W, Cin, Cout, workspace, workspace_floats, false);
}

// ... writing a CHANNEL SLICE of a wider gradient (the skip half of a sub-pixel decoder layer): dw points at the slice's first input channel
// inside (Cout, dw_cin_stride, 3, 3); same plan, same sums in the same order — dw_cin_stride = Cin is u3d_conv2d_wgrad_bf16 bit for bit
extern "C" int u3d_conv2d_wgrad_bf16_strided(int device, u3d_stream_t stream, const float* x, const float* affine, const float* dz, float* dw,
                                             int dw_cin_stride, int N, int H, int W, int Cin, int Cout, float* workspace,
                                             long long workspace_floats) {
    U3D_REQUIRE(dw_cin_stride > 0, "u3d_conv2d_wgrad_bf16_strided: bad argument");
    return c2b_wgrad_launch("u3d_conv2d_wgrad_bf16_strided", device, stream, x, affine, dz, dw, N, H, W, Cin, Cout, workspace,
                            workspace_floats, false, nullptr, dw_cin_stride);
}

// ... of a layer with both channel counts % 16: a 16-channel cell stages zeros for its two missing channel octets, dw stores are masked
extern "C" int u3d_conv2d_wgrad_bf16_c16(int device, u3d_stream_t stream, const float* x, const float* affine, const float* dz, float* dw,
                                         int N, int H, int W, int Cin, int Cout, float* workspace, long long workspace_floats) {
    return c2b_wgrad_launch("u3d_conv2d_wgrad_bf16_c16", device, stream, x, affine, dz, dw, N, H, W, Cin, Cout, workspace, workspace_floats,
                            true);
}

// ... of a decoder's first convolution on its virtual concat (`native_2d_bf16_vcat`): g = affine(cat(skip, nearest(low))), dw (Cout, C0 +
// C1, 3, 3); plan and workspace as u3d_conv2d_wgrad_bf16 for Cin = C0 + C1
extern "C" int u3d_conv2d_wgrad_bf16_src(int device, u3d_stream_t stream, const u3d_src_t* src, const float* dz, float* dw, int N, int H,
                                         int W, int Cout, float* workspace, long long workspace_floats) {
    U3D_REQUIRE(c2b_vsrc_ok(src), "u3d_conv2d_wgrad_bf16_src: needs a virtual source with C0 %% 32 == 0, C1 %% 32 == 0, C0 > 0, C1 > 0 (C1 == 0 "
                "is u3d_conv2d_wgrad_bf16), D1 == 1, ymap / xmap and 16-byte aligned halves");
    return c2b_wgrad_launch("u3d_conv2d_wgrad_bf16_src", device, stream, src->p0, src->affine, dz, dw, N, H, W, src->C0 + src->C1, Cout,
                            workspace, workspace_floats, false, src);
}

// =================================================================================================
// ConvTranspose2d(k = 3, stride = 2, padding = 1, bias = False) of ResidualUNet2D's decoders on the same MFMA (`native_2d_residual_bf16_deconv:
// true`): the bf16 twins of u3d_convtr2d_fwd / _dgrad / _wgrad of csrc/u3d_res.hip.  (N,H1,W1,Cin) -> (N,2H1-1,2W1-1,Cout), NHWC fp32 in HBM,
// master weight (Cin,Cout,3,3); output coordinate s = 2i - 1 + tap per axis, so an even s = 2j takes (input j, tap 1) and an odd s = 2j + 1
// takes (input j + 1, tap 0) and (input j, tap 2).  Operands are rounded where the 3x3 family rounds them: the weights when the image is
// packed, x / dt once while they are staged into LDS; fp32 accumulation; padding and the inserted zeros are never multiplied.
//
// Forward (convtr2d_fwd_bf16_kernel, sub-pixel form): a block stages its 16 x 16 INPUT tile plus the right / bottom halo pixel (17 x 17,
// [hy][hx][16 bf16], 35 slots of 16 bytes per row: the odd row stride of the 3x3 kernel, same conflict-free ds_read_b128) once per 16-channel
// chunk and feeds all four output parity classes from it — 1 + 2 + 2 + 4 = 9 MFMAs per M-tile and chunk, the four distinct A fragments
// (input offsets (0|1, 0|1)) read once per chunk.  8 accumulators (2 M-tiles x 4 classes) = 128 registers, so a block owns 32 output channels.
// Every element of t is written exactly once: class (py, px) of input pixel (i, j) is t[2i + py][2j + px], dropped past 2H1 - 2 / 2W1 - 2.
//
// Data gradient (convtr2d_dgrad_bf16_kernel<NT>): dx[i] = sum_tap dt[2i - 1 + tap] * w[tap], a stride-2 3x3 convolution of dt.  The
// 33 x 33 dt halo of a 16 x 16 dx tile is staged DE-INTERLEAVED: halo row / column h sits in slot (h & 1) * 17 + (h >> 1), so the 16 pixels
// a tap reads at stride 2 are 16 neighbouring slots and neighbouring tile rows are neighbouring LDS rows — the 3x3 kernel's read pattern
// again (67 slots per row).  One 35 KB buffer (two would not leave two blocks per CU their registers' worth of LDS): the next chunk's halo
// is in flight in registers during the MFMAs and stored between two barriers.  NT = 2 (64 produced channels per block) when Cin % 64 == 0.
//
// Weight gradient (convtr2d_wgrad_bf16_kernel): dw[ci][co][tap] = sum_i x[i, ci] * dt[2i - 1 + tap, co], contraction over INPUT pixels;
// A = x (8 x 16-pixel tile, [pixel][32 ci]), B = dt (17 x 33 halo, columns de-interleaved as above, [pixel][32 co]), both fetched with
// the transposed read of the 3x3 weight gradient; 9 accumulators, one x fragment feeds 9 taps.  Partial sums over tile ranges go to the
// workspace and convtr2d_wgrad_bf16_reduce_kernel adds them in split order (bitwise-reproducible; no atomics, no fp64).
namespace {

namespace ct2b {
constexpr int T = 16;                      // tile edge (input pixels forward, dx pixels in the data gradient)
constexpr int PS = 32;                     // bytes per staged pixel (16 bf16)
// forward
constexpr int FH = T + 1;                  // tile + right / bottom halo
constexpr int FRS = FH * PS + 16;          // 560 bytes per row: 35 slots
constexpr int FBUF = FH * FRS;             // 9520
constexpr int FITEMS = FH * FH * 2;        // 578 (pixel, channel octet) items per chunk
constexpr int FNIT = (FITEMS + 255) / 256; // 3
constexpr int F_LDS_BYTES = 2 * FBUF;      // 19040 (double-buffered)
// data gradient
constexpr int DH = 2 * T + 1;              // 33: dt rows 2 y0 - 1 .. 2 y0 + 31
constexpr int DODD = T + 1;                // first slot of the odd rows / columns (17 even ones in front)
constexpr int DRS = DH * PS + 16;          // 1072 bytes per row: 67 slots
constexpr int DBUF = DH * DRS;             // 35376
constexpr int DITEMS = DH * DH * 2;        // 2178
constexpr int DNIT = (DITEMS + 255) / 256; // 9
constexpr int D_LDS_BYTES = DBUF;
// weight gradient
constexpr int WTY = 8;                     // tile rows (x 16 columns)
constexpr int WHY = 2 * WTY + 1;           // 17 dt rows
constexpr int WHX = 2 * T + 1;             // 33 dt columns (slots)
constexpr int WPP = 64;                    // bytes per staged pixel (32 bf16)
constexpr int W_DT = 0;                    // [17][33][32] bf16
constexpr int W_X = WHY * WHX * WPP;       // 35904: [8 * 16][32] bf16
constexpr int W_LDS_BYTES = W_X + WTY * T * WPP;  // 44096 (the final [4][32][32] float reduction reuses the first 16384)
constexpr int W_DIT = (WHY * WHX * 4 + 255) / 256;  // 9 dt items (pixel, octet) per thread
constexpr int W_XIT = WTY * T * 4 / 256;            // 2 x items per thread
constexpr int W_DB = 3, W_XB = 2;                   // items staged per batch
}  // namespace ct2b

inline bool ct2b_ok(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0; }

// (the limits of convtr2d_dims_ok, csrc/u3d_res.hip)
inline bool ct2b_dims_ok(int N, int H1, int W1, int Cin, int Cout) {
    return N > 0 && H1 > 0 && W1 > 0 && Cin > 0 && Cout > 0 && (long long)N * (2LL * H1 - 1) * (2LL * W1 - 1) < (1ll << 31) &&
           (long long)9 * Cin * Cout < (1ll << 31);
}

// image [K / 16 chunk][tap][n-tile][lane][8] of B[k][n], the fragment layout of pack_weights2d_bf16_kernel; taps are NOT flipped:
//   mode 0 (forward): B[k = ci][n = co] = w[ci][co][tap]           mode 1 (data gradient): B[k = co][n = ci] = w[ci][co][tap]
__global__ void pack_convtr2d_bf16_kernel(const float* __restrict__ w, int Cout, int mode, int ntg, long long total,
                                          __bf16* __restrict__ packed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        long long r = i >> 9;
        const int nt = (int)(r % ntg);
        r /= ntg;
        const int tap = (int)(r % 9);
        const int chunk = (int)(r / 9);
        const int k = chunk * 16 + 8 * (lane >> 5) + j;
        const int nn = nt * 32 + (lane & 31);
        packed[i] = (__bf16)(mode == 0 ? w[((size_t)k * Cout + nn) * 9 + tap] : w[((size_t)nn * Cout + k) * 9 + tap]);
    }
}

struct ConvTr2dBf16Params {
    const float* src;     // forward: x (N,H1,W1,Cin); data gradient: dt (N,Ht,Wt,Cout)
    const c2b_bf16x8* wp;
    const float* x_low;   // data gradient: optional ReLU mask (N,H1,W1,Cin)
    float* out;           // forward: t; data gradient: dx
    int N, H1, W1, Ht, Wt, Cin, Cout;
    int nchunks, ntg, ncb, ty, tx;
};

__global__ __launch_bounds__(256, 2) void convtr2d_fwd_bf16_kernel(const ConvTr2dBf16Params p) {
    using namespace ct2b;
    extern __shared__ __attribute__((aligned(16))) char lds_ct2f[];
    char* const lds = lds_ct2f;
    const int t = threadIdx.x;
    const int l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int tile = blockIdx.x;
    const int cb = tile % p.ntg;
    tile /= p.ntg;
    const int txi = tile % p.tx;
    tile /= p.tx;
    const int tyi = tile % p.ty;
    const int n = tile / p.ty;
    const int y0 = tyi * T, x0 = txi * T;
    const int H1 = p.H1, W1 = p.W1, Cin = p.Cin;

    int ldsoff[FNIT], gpix[FNIT];  // gpix < 0: outside the image (stays exactly 0)
#pragma unroll
    for (int it = 0; it < FNIT; ++it) {
        const int item = t + 256 * it;
        const bool in = item < FITEMS;
        const int pix = item >> 1, q = item & 1;
        const int hy = pix / FH, hx = pix - (pix / FH) * FH;
        const int gy = y0 + hy, gxx = x0 + hx;
        const bool ok = in && gy < H1 && gxx < W1;
        ldsoff[it] = in ? hy * FRS + hx * PS + 16 * q : -1;
        gpix[it] = ok ? (n * H1 + gy) * W1 + gxx : -1;
    }
    f32x4 raw[FNIT][2];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int it = 0; it < FNIT; ++it) {
            raw[it][0] = raw[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (gpix[it] >= 0) {
                const float* src = p.src + (size_t)gpix[it] * Cin + c * 16 + 8 * ((t + 256 * it) & 1);
                raw[it][0] = u3d_ldq(src);
                raw[it][1] = u3d_ldq(src + 4);
            }
        }
    };
    auto store_chunk = [&](char* buf) {
#pragma unroll
        for (int it = 0; it < FNIT; ++it)
            if (ldsoff[it] >= 0)
                *reinterpret_cast<c2b_bf16x8*>(buf + ldsoff[it]) = c2b_stage8(raw[it][0], raw[it][1], nullptr, gpix[it] >= 0);
    };

    f32x16 acc[2][4];  // [M-tile][parity class 2 py + px]
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int cls = 0; cls < 4; ++cls)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][cls][r] = 0.f;

    // A-fragment base: lane (i32, h) of M-tile mt reads input pixel (4w + 2mt + (i32 >> 4), i32 & 15), channels 8h .. 8h + 7
    const int abase = (4 * w + (i32 >> 4)) * FRS + (i32 & 15) * PS + 16 * h;
    auto bidx = [&](int c, int tap) -> long long { return ((long long)(c * 9 + tap) * p.ntg + cb) * 64 + l; };

    load_chunk(0);
    store_chunk(lds);
    __syncthreads();
    for (int c = 0; c < p.nchunks; ++c) {
        const char* cur = lds + (c & 1) * FBUF;
        if (c + 1 < p.nchunks) load_chunk(c + 1);  // in flight during the MFMAs
        c2b_bf16x8 a[2][2][2];                     // [input dy][input dx][M-tile]
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    a[dy][dx][mt] = *reinterpret_cast<const c2b_bf16x8*>(cur + abase + (2 * mt + dy) * FRS + dx * PS);
        c2b_bf16x8 bq = p.wp[bidx(c, 0)], bn = bq;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - (tap / 3) * 3;
            if (tap + 1 < 9) bn = p.wp[bidx(c, tap + 1)];
            // tap 1 serves the even outputs from input +0; taps 0 / 2 serve the odd outputs from inputs +1 / +0
            const int cls = 2 * (ky != 1) + (kx != 1), dy = ky == 0, dx = kx == 0;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) acc[mt][cls] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[dy][dx][mt], bq, acc[mt][cls], 0, 0, 0);
            bq = bn;
        }
        if (c + 1 < p.nchunks) store_chunk(lds + ((c + 1) & 1) * FBUF);  // (that buffer was last read in chunk c - 1)
        __syncthreads();
    }

    // ---- lane column = output channel, register r = M row (r & 3) + 8 (r >> 2) + 4h; class (py, px) of input (i, j) is t[2i + py][2j + px]
    const int co = cb * 32 + i32;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int cls = 0; cls < 4; ++cls)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int i = y0 + 4 * w + 2 * mt + (row >> 4), j = x0 + (row & 15);
                const int oy = 2 * i + (cls >> 1), ox = 2 * j + (cls & 1);
                if (i >= H1 || j >= W1 || oy >= p.Ht || ox >= p.Wt) continue;
                p.out[((size_t)(n * p.Ht + oy) * p.Wt + ox) * p.Cout + co] = acc[mt][cls][r];
            }
}

template <int NT>
__global__ __launch_bounds__(256, 2) void convtr2d_dgrad_bf16_kernel(const ConvTr2dBf16Params p) {
    using namespace ct2b;
    extern __shared__ __attribute__((aligned(16))) char lds_ct2d[];
    char* const lds = lds_ct2d;
    const int t = threadIdx.x;
    const int l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int tile = blockIdx.x;
    const int cb = tile % p.ncb;
    tile /= p.ncb;
    const int txi = tile % p.tx;
    tile /= p.tx;
    const int tyi = tile % p.ty;
    const int n = tile / p.ty;
    const int y0 = tyi * T, x0 = txi * T;
    const int H1 = p.H1, W1 = p.W1, Ht = p.Ht, Wt = p.Wt, K = p.Cout;  // the contraction runs over the layer's Cout

    int ldsoff[DNIT], gpix[DNIT];  // gpix < 0: outside dt (zero)
#pragma unroll
    for (int it = 0; it < DNIT; ++it) {
        const int item = t + 256 * it;
        const bool in = item < DITEMS;
        const int pix = item >> 1, q = item & 1;
        const int hy = pix / DH, hx = pix - (pix / DH) * DH;
        const int gy = 2 * y0 - 1 + hy, gxx = 2 * x0 - 1 + hx;
        const bool ok = in && gy >= 0 && gy < Ht && gxx >= 0 && gxx < Wt;
        ldsoff[it] = in ? ((hy & 1) * DODD + (hy >> 1)) * DRS + ((hx & 1) * DODD + (hx >> 1)) * PS + 16 * q : -1;
        gpix[it] = ok ? (n * Ht + gy) * Wt + gxx : -1;
    }
    f32x4 raw[DNIT][2];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int it = 0; it < DNIT; ++it) {
            raw[it][0] = raw[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (gpix[it] >= 0) {
                const float* src = p.src + (size_t)gpix[it] * K + c * 16 + 8 * ((t + 256 * it) & 1);
                raw[it][0] = u3d_ldq(src);
                raw[it][1] = u3d_ldq(src + 4);
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int it = 0; it < DNIT; ++it)
            if (ldsoff[it] >= 0)
                *reinterpret_cast<c2b_bf16x8*>(lds + ldsoff[it]) = c2b_stage8(raw[it][0], raw[it][1], nullptr, gpix[it] >= 0);
    };

    f32x16 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    // lane (i32, h) of M-tile mt owns dx pixel (ii, jj) = (4w + 2mt + (i32 >> 4), i32 & 15); tap (ty, tx) reads halo (2 ii + ty, 2 jj + tx),
    // i.e. slot row (ty & 1) * 17 + (ty >> 1) + ii and slot column (tx & 1) * 17 + (tx >> 1) + jj
    const int abase = (4 * w + (i32 >> 4)) * DRS + (i32 & 15) * PS + 16 * h;
    auto bidx = [&](int c, int tap, int nt) -> long long { return ((long long)(c * 9 + tap) * p.ntg + (cb * NT + nt)) * 64 + l; };

    load_chunk(0);
    store_chunk();
    __syncthreads();
    for (int c = 0; c < p.nchunks; ++c) {
        if (c + 1 < p.nchunks) load_chunk(c + 1);  // in flight during the MFMAs
        c2b_bf16x8 bq[NT], bn[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bq[nt] = p.wp[bidx(c, 0, nt)];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ty = tap / 3, tx = tap - (tap / 3) * 3;
            if (tap + 1 < 9) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bn[nt] = p.wp[bidx(c, tap + 1, nt)];
            }
            const int toff = ((ty & 1) * DODD + (ty >> 1)) * DRS + ((tx & 1) * DODD + (tx >> 1)) * PS;
            c2b_bf16x8 a[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) a[mt] = *reinterpret_cast<const c2b_bf16x8*>(lds + abase + toff + 2 * mt * DRS);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt], bq[nt], acc[mt][nt], 0, 0, 0);
            if (tap + 1 < 9) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bq[nt] = bn[nt];
            }
        }
        __syncthreads();  // every wave is done reading the one buffer
        if (c + 1 < p.nchunks) {
            store_chunk();
            __syncthreads();
        }
    }

#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ci = (cb * NT + nt) * 32 + i32;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int y = y0 + 4 * w + 2 * mt + (row >> 4), x = x0 + (row & 15);
                if (y >= H1 || x >= W1) continue;
                const size_t o = ((size_t)(n * H1 + y) * W1 + x) * p.Cin + ci;
                float v = acc[mt][nt][r];
                if (p.x_low != nullptr && !(p.x_low[o] > 0.f)) v = 0.f;  // ReLU backward of the block that produced x
                p.out[o] = v;
            }
    }
}

struct ConvTr2dWgradBf16Params {
    const float* x;   // (N,H1,W1,Cin)
    const float* dt;  // (N,Ht,Wt,Cout)
    float* ws;        // [nsplit][Cin][Cout][9]
    int N, H1, W1, Ht, Wt, Cin, Cout;
    int ty, tx, ncob, ncib, ntiles, tps;
};

__global__ __launch_bounds__(256, 2) void convtr2d_wgrad_bf16_kernel(const ConvTr2dWgradBf16Params p) {
    using namespace ct2b;
    extern __shared__ __attribute__((aligned(16))) char lds_ct2w[];
    char* const lds = lds_ct2w;
    const int t = threadIdx.x, l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int b = blockIdx.x;
    const int cob = b % p.ncob;
    b /= p.ncob;
    const int cib = b % p.ncib;
    const int split = b / p.ncib;
    const int ci0 = cib * 32, co0 = cob * 32;
    const int tile0 = split * p.tps, tile1 = min(p.ntiles, tile0 + p.tps);
    const int H1 = p.H1, W1 = p.W1, Ht = p.Ht, Wt = p.Wt, Cin = p.Cin, Cout = p.Cout;
    char* const dtl = lds + W_DT;
    char* const xl = lds + W_X;

    f32x16 acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    // transposed-read lane offset, as conv2d_wgrad_bf16_kernel: lane l receives channel (l & 31) of the 8 pixels 8 * (l >> 5) .. + 7
    const int g4 = l >> 4, sidx = l & 15;
    const int lane_off = (8 * (g4 >> 1) + (sidx >> 2)) * WPP + (16 * (g4 & 1) + 4 * (sidx & 3)) * 2;

    for (int tile = tile0; tile < tile1; ++tile) {
        int tt = tile;
        const int txi = tt % p.tx;
        tt /= p.tx;
        const int tyi = tt % p.ty;
        const int n = tt / p.ty;
        const int y0 = tyi * WTY, x0 = txi * T;
        // stage dt (17 x 33 halo from (2 y0 - 1, 2 x0 - 1), 32 channels from co0, columns de-interleaved, zero outside) and x (8 x 16, 32
        // channels from ci0), a few items at a time: the 9 accumulators leave ~100 registers for the staging
        auto stage_dt = [&](int it0) {
            f32x4 rg[W_DB][2];
            bool okg[W_DB];
#pragma unroll
            for (int k = 0; k < W_DB; ++k) {
                const int item = t + 256 * (it0 + k);
                const int pix = item >> 2, q = item & 3;
                const int hy = pix / WHX, hx = pix - (pix / WHX) * WHX;
                const int gy = 2 * y0 - 1 + hy, gxx = 2 * x0 - 1 + hx;
                okg[k] = item < WHY * WHX * 4 && gy >= 0 && gy < Ht && gxx >= 0 && gxx < Wt;
                rg[k][0] = rg[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (okg[k]) {
                    const float* src = p.dt + ((size_t)(n * Ht + gy) * Wt + gxx) * Cout + co0 + 8 * q;
                    rg[k][0] = u3d_ldq(src);
                    rg[k][1] = u3d_ldq(src + 4);
                }
            }
#pragma unroll
            for (int k = 0; k < W_DB; ++k) {
                const int item = t + 256 * (it0 + k);
                if (item >= WHY * WHX * 4) continue;
                const int pix = item >> 2, q = item & 3;
                const int hy = pix / WHX, hx = pix - (pix / WHX) * WHX;
                *reinterpret_cast<c2b_bf16x8*>(dtl + (hy * WHX + (hx & 1) * DODD + (hx >> 1)) * WPP + 16 * q) =
                    c2b_stage8(rg[k][0], rg[k][1], nullptr, okg[k]);
            }
        };
        auto stage_x = [&](int it0) {
            f32x4 rd[W_XB][2];
            bool okd[W_XB];
#pragma unroll
            for (int k = 0; k < W_XB; ++k) {
                const int item = t + 256 * (it0 + k);
                const int pix = item >> 2, q = item & 3;
                const int y = y0 + (pix >> 4), x = x0 + (pix & 15);
                okd[k] = y < H1 && x < W1;
                rd[k][0] = rd[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (okd[k]) {
                    const float* src = p.x + ((size_t)(n * H1 + y) * W1 + x) * Cin + ci0 + 8 * q;
                    rd[k][0] = u3d_ldq(src);
                    rd[k][1] = u3d_ldq(src + 4);
                }
            }
#pragma unroll
            for (int k = 0; k < W_XB; ++k) {
                const int item = t + 256 * (it0 + k);
                *reinterpret_cast<c2b_bf16x8*>(xl + (item >> 2) * WPP + 16 * (item & 3)) = c2b_stage8(rd[k][0], rd[k][1], nullptr, okd[k]);
            }
        };
        for (int it0 = 0; it0 < W_DIT; it0 += W_DB) stage_dt(it0);
        for (int it0 = 0; it0 < W_XIT; it0 += W_XB) stage_x(it0);
        __syncthreads();
        // wave w: rows 2w, 2w + 1 of the tile, one 16-pixel row per k-step; tap (ty, tx) pairs input (py, jj) with dt halo (2 py + ty, 2 jj + tx)
#pragma unroll 1
        for (int r = 0; r < 2; ++r) {
            const int py = 2 * w + r;
            const c2b_bf16x8 a = c2b_tr_frag(xl + py * T * WPP + lane_off);
#pragma unroll
            for (int ty = 0; ty < 3; ++ty)
#pragma unroll
                for (int tx = 0; tx < 3; ++tx) {
                    const c2b_bf16x8 g = c2b_tr_frag(dtl + ((2 * py + ty) * WHX + (tx & 1) * DODD + (tx >> 1)) * WPP + lane_off);
                    acc[ty * 3 + tx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, g, acc[ty * 3 + tx], 0, 0, 0);
                }
        }
        __syncthreads();
    }

    // ---- add the 4 waves' partial sums in a fixed order, one tap at a time, through LDS; write [ci][co][tap] of this split
    float* red = reinterpret_cast<float*>(lds);  // [4][32][32]
    float* const dst = p.ws + (size_t)split * Cin * Cout * 9;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {  // (unrolled: acc[tap] must stay a register index)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;  // input channel within the block
            red[(w * 32 + row) * 32 + i32] = acc[tap][r];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = t + 256 * e;  // (row, col) of the 32 x 32 tile
            const int row = idx >> 5, col = idx & 31;
            const float v = ((red[(0 * 32 + row) * 32 + col] + red[(1 * 32 + row) * 32 + col]) + red[(2 * 32 + row) * 32 + col]) +
                            red[(3 * 32 + row) * 32 + col];
            dst[((size_t)(ci0 + row) * Cout + co0 + col) * 9 + tap] = v;
        }
        __syncthreads();
    }
}

// dw[i] = [dw[i] +] sum over splits in split order (bitwise-reproducible)
__global__ void convtr2d_wgrad_bf16_reduce_kernel(const float* __restrict__ ws, int nsplit, long long total, int accumulate,
                                                  float* __restrict__ dw) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) v += ws[(size_t)s * total + i];
        dw[i] = accumulate ? dw[i] + v : v;
    }
}

// data gradient: 64 produced channels per block whenever they divide evenly (shape-only: no device in this plan)
inline int ct2b_dgrad_nt(int Cin) { return Cin % 64 == 0 ? 2 : 1; }

struct Ct2bWPlan {
    int ty, tx, ncob, ncib, ntiles, tps, nsplit;
};

// the plan fills the chip (~4 blocks per CU); a launch takes as many of its splits as the caller's workspace holds (at least one).
// ONE function for the launcher, the workspace size and the host-only query.  max_splits <= 0: no cap.
Ct2bWPlan ct2b_wplan(int device, int N, int H1, int W1, int Cin, int Cout, long long max_splits) {
    Ct2bWPlan pl;
    pl.ty = (int)c2b_cdiv(H1, ct2b::WTY);
    pl.tx = (int)c2b_cdiv(W1, ct2b::T);
    pl.ncob = Cout / 32;
    pl.ncib = Cin / 32;
    pl.ntiles = N * pl.ty * pl.tx;
    const long long cells = (long long)pl.ncob * pl.ncib;
    const long long target = 4LL * c2b_cu_count(device);
    long long ns = std::max<long long>(1, std::min<long long>(pl.ntiles, c2b_cdiv(target, cells)));
    if (max_splits > 0) ns = std::min(ns, max_splits);
    pl.tps = (int)c2b_cdiv(pl.ntiles, ns);
    pl.nsplit = (int)c2b_cdiv(pl.ntiles, pl.tps);
    return pl;
}

inline long long ct2b_splits_in(long long workspace_floats, int Cin, int Cout) { return workspace_floats / ((long long)9 * Cin * Cout); }

}  // namespace

extern "C" int u3d_convtr2d_bf16_supported(int Cin, int Cout) { return ct2b_ok(Cin, Cout) ? 1 : 0; }

extern "C" long long u3d_packed_convtr2d_bf16_elems(int Cin, int Cout, int mode) {
    if ((mode != 0 && mode != 1) || !ct2b_ok(Cin, Cout) || (long long)9 * Cin * Cout >= (1ll << 31)) return 0;
    return (long long)9 * Cin * Cout;  // [K / 16][9][Nn / 32][64][8]
}

extern "C" int u3d_pack_convtr2d_bf16(int device, u3d_stream_t stream, const float* w, int Cin, int Cout, int mode, void* packed) {
    U3D_ENTER(device);
    U3D_REQUIRE(w && packed && (mode == 0 || mode == 1), "u3d_pack_convtr2d_bf16: bad argument");
    U3D_REQUIRE(ct2b_ok(Cin, Cout) && (long long)9 * Cin * Cout < (1ll << 31),
                "u3d_pack_convtr2d_bf16: (%d -> %d) channels are outside the bf16 envelope (both %% 32)", Cin, Cout);
    U3D_REQUIRE(c2b_aligned(packed), "u3d_pack_convtr2d_bf16: the image must be 16-byte aligned");
    const long long total = (long long)9 * Cin * Cout;
    long long blocks = c2b_cdiv(total, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_convtr2d_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, Cout, mode,
                       (mode == 0 ? Cout : Cin) / 32, total, reinterpret_cast<__bf16*>(packed));
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_convtr2d_fwd_bf16(int device, u3d_stream_t stream, const float* x, const void* packed, float* t, int N, int H1, int W1,
                                     int Cin, int Cout) {
    U3D_ENTER(device);
    U3D_REQUIRE(ct2b_ok(Cin, Cout), "u3d_convtr2d_fwd_bf16: (%d -> %d) channels are outside the bf16 envelope (both %% 32)", Cin, Cout);
    U3D_REQUIRE(x && packed && t, "u3d_convtr2d_fwd_bf16: bad argument");
    U3D_REQUIRE(ct2b_dims_ok(N, H1, W1, Cin, Cout), "u3d_convtr2d_fwd_bf16: bad sizes (the output pixel count must be < 2^31)");
    U3D_REQUIRE(c2b_aligned(x) && c2b_aligned(packed) && c2b_aligned(t), "u3d_convtr2d_fwd_bf16: pointers must be 16-byte aligned");
    ConvTr2dBf16Params p = {};
    p.src = x;
    p.wp = reinterpret_cast<const c2b_bf16x8*>(packed);
    p.out = t;
    p.N = N, p.H1 = H1, p.W1 = W1, p.Ht = 2 * H1 - 1, p.Wt = 2 * W1 - 1, p.Cin = Cin, p.Cout = Cout;
    p.nchunks = Cin / 16, p.ntg = Cout / 32, p.ncb = p.ntg;
    p.ty = (int)c2b_cdiv(H1, ct2b::T), p.tx = (int)c2b_cdiv(W1, ct2b::T);
    const long long blocks = (long long)N * p.ty * p.tx * p.ncb;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_convtr2d_fwd_bf16: grid too large");
    hipLaunchKernelGGL(convtr2d_fwd_bf16_kernel, dim3((unsigned)blocks), dim3(256), ct2b::F_LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    return 0;
}

// host-only: 32-channel n-tiles per data-gradient block (1 or 2), from the function the launch calls; -1 outside the envelope
extern "C" int u3d_convtr2d_dgrad_bf16_variant(int N, int H1, int W1, int Cin, int Cout) {
    if (!ct2b_ok(Cin, Cout) || !ct2b_dims_ok(N, H1, W1, Cin, Cout)) return -1;
    return ct2b_dgrad_nt(Cin);
}

extern "C" int u3d_convtr2d_dgrad_bf16(int device, u3d_stream_t stream, const float* dt, const void* packed_t, const float* x_low,
                                       float* dx, int N, int H1, int W1, int Cin, int Cout) {
    U3D_ENTER(device);
    U3D_REQUIRE(ct2b_ok(Cin, Cout), "u3d_convtr2d_dgrad_bf16: (%d -> %d) channels are outside the bf16 envelope (both %% 32)", Cin, Cout);
    U3D_REQUIRE(dt && packed_t && dx, "u3d_convtr2d_dgrad_bf16: bad argument");
    U3D_REQUIRE(ct2b_dims_ok(N, H1, W1, Cin, Cout), "u3d_convtr2d_dgrad_bf16: bad sizes (the output pixel count must be < 2^31)");
    U3D_REQUIRE(c2b_aligned(dt) && c2b_aligned(packed_t) && c2b_aligned(dx), "u3d_convtr2d_dgrad_bf16: pointers must be 16-byte aligned");
    const int nt = ct2b_dgrad_nt(Cin);
    ConvTr2dBf16Params p = {};
    p.src = dt;
    p.wp = reinterpret_cast<const c2b_bf16x8*>(packed_t);
    p.x_low = x_low;
    p.out = dx;
    p.N = N, p.H1 = H1, p.W1 = W1, p.Ht = 2 * H1 - 1, p.Wt = 2 * W1 - 1, p.Cin = Cin, p.Cout = Cout;
    p.nchunks = Cout / 16, p.ntg = Cin / 32, p.ncb = p.ntg / nt;
    p.ty = (int)c2b_cdiv(H1, ct2b::T), p.tx = (int)c2b_cdiv(W1, ct2b::T);
    const long long blocks = (long long)N * p.ty * p.tx * p.ncb;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_convtr2d_dgrad_bf16: grid too large");
    if (nt == 2)
        hipLaunchKernelGGL(convtr2d_dgrad_bf16_kernel<2>, dim3((unsigned)blocks), dim3(256), ct2b::D_LDS_BYTES, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(convtr2d_dgrad_bf16_kernel<1>, dim3((unsigned)blocks), dim3(256), ct2b::D_LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" long long u3d_convtr2d_wgrad_bf16_workspace_floats(int N, int H1, int W1, int Cin, int Cout) {
    if (!ct2b_ok(Cin, Cout) || !ct2b_dims_ok(N, H1, W1, Cin, Cout)) return 0;
    return (long long)ct2b_wplan(c2b_current_device(), N, H1, W1, Cin, Cout, 0).nsplit * 9 * Cin * Cout;
}

// host-only: (tiles per block << 16) | nsplit of the launch a workspace of that many floats gets (< 0: the full workspace); -1 outside
// the envelope or for a workspace shorter than one split
extern "C" int u3d_convtr2d_wgrad_bf16_variant(int N, int H1, int W1, int Cin, int Cout, long long workspace_floats) {
    if (!ct2b_ok(Cin, Cout) || !ct2b_dims_ok(N, H1, W1, Cin, Cout)) return -1;
    const long long cap = workspace_floats < 0 ? 0 : ct2b_splits_in(workspace_floats, Cin, Cout);
    if (workspace_floats >= 0 && cap < 1) return -1;
    const Ct2bWPlan pl = ct2b_wplan(c2b_current_device(), N, H1, W1, Cin, Cout, cap);
    return (std::min(pl.tps, 0x7fff) << 16) | std::min(pl.nsplit, 0xffff);
}

extern "C" int u3d_convtr2d_wgrad_bf16(int device, u3d_stream_t stream, const float* x, const float* dt, float* dw, int N, int H1, int W1,
                                       int Cin, int Cout, int accumulate, float* workspace, long long workspace_floats) {
    U3D_ENTER(device);
    U3D_REQUIRE(ct2b_ok(Cin, Cout), "u3d_convtr2d_wgrad_bf16: (%d -> %d) channels are outside the bf16 envelope (both %% 32)", Cin, Cout);
    U3D_REQUIRE(x && dt && dw && workspace, "u3d_convtr2d_wgrad_bf16: bad argument");
    U3D_REQUIRE(ct2b_dims_ok(N, H1, W1, Cin, Cout), "u3d_convtr2d_wgrad_bf16: bad sizes (the output pixel count must be < 2^31)");
    U3D_REQUIRE(c2b_aligned(x) && c2b_aligned(dt), "u3d_convtr2d_wgrad_bf16: pointers must be 16-byte aligned");
    const long long total = (long long)9 * Cin * Cout;
    const long long cap = ct2b_splits_in(workspace_floats, Cin, Cout);
    U3D_REQUIRE(cap >= 1, "u3d_convtr2d_wgrad_bf16: workspace too small (%lld < %lld floats, one split)", workspace_floats, total);
    const Ct2bWPlan pl = ct2b_wplan(device, N, H1, W1, Cin, Cout, cap);
    ConvTr2dWgradBf16Params p = {};
    p.x = x;
    p.dt = dt;
    p.ws = workspace;
    p.N = N, p.H1 = H1, p.W1 = W1, p.Ht = 2 * H1 - 1, p.Wt = 2 * W1 - 1, p.Cin = Cin, p.Cout = Cout;
    p.ty = pl.ty, p.tx = pl.tx, p.ncob = pl.ncob, p.ncib = pl.ncib, p.ntiles = pl.ntiles, p.tps = pl.tps;
    const long long blocks = (long long)pl.nsplit * pl.ncob * pl.ncib;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_convtr2d_wgrad_bf16: grid too large");
    hipLaunchKernelGGL(convtr2d_wgrad_bf16_kernel, dim3((unsigned)blocks), dim3(256), ct2b::W_LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    long long rb = c2b_cdiv(total, 256);
    if (rb > 4096) rb = 4096;
    hipLaunchKernelGGL(convtr2d_wgrad_bf16_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace, pl.nsplit, total,
                       accumulate ? 1 : 0, dw);
    U3D_LAUNCH_CHECK();
    return 0;
}

// =================================================================================================
// Sub-pixel decoder convolutions of a UNet2D in bf16 (`native_2d_bf16_subpixel: true`): the bf16 twins of u3d_subpixel2d_conv_fwd /
// _dgrad_reps / _wgrad of csrc/u3d_subpix2d.hip on v_mfma_f32_32x32x16_bf16.  The upsampled half of cat(skip, nearest2x(low)) under a 3x3
// convolution: an output pixel of parity p reads, per axis, only the two low-res pixels j + p - 1 + e (e = 0, 1) — p = 0: {t0}, {t1 + t2};
// p = 1: {t0 + t1}, {t2} — so each of the 4 parity classes is a 2x2 convolution over the low-res grid, 4/9 of the multiply-adds, and the data
// gradient lands at low resolution with the children sum folded in.  Tensors in HBM are fp32 NHWC, accumulation is fp32.
// Rounding points: the pre-summed taps are added in fp32 from the fp32 master weight (in ascending (ty, tx) order) and rounded ONCE to
// bf16, nearest even, by the pack kernel; activations and dz are rounded once while staged to LDS, after the fp32 affine fmaf(x, a, b);
// zero padding applies after the affine and stays exactly 0 (c2b_stage8).  Not bit-equal to the 9-tap bf16 kernels on the written-out
// concat in forward and data gradient (those round every tap); the weight gradient multiplies the same bf16 operands.
//
// Forward (subpix2d_fwd_bf16_kernel): the 3x3 kernel's block — 16 x 16 LOW-RES pixels, 18 x 18 halo [hy][hx][16 bf16] with 37 slots per row,
// double-buffered over 16-channel chunks — serving all four classes from one staged halo: nine A-fragment positions, sixteen MFMAs per
// M-tile (class (a, b) takes halo offsets (a + u, b + v)); 2 M-tiles x 4 classes = 128 accumulator registers, so a block owns 32 output
// channels.  out (N, 2H1, 2W1, Cout) receives the plain partial sums: the skip half joins through u3d_conv2d_bf16_res(residual = out).
//
// Data gradient (subpix2d_dgrad_bf16_kernel): dlow[i] = sum over the 4 x 4 stride-2 gather dz[2i - 1 + r], per axis r = 0..3 carrying t2,
// t1 + t2, t0 + t1, t0.  The 34 x 34 dz region of a 16 x 16 dlow tile is staged DE-INTERLEAVED into its four parity planes (17 x 17 each,
// 35 slots per row): tap r reads plane (r + 1) & 1 at offset r >> 1, unit-stride A-fragment reads with the forward's conflict-free pattern.
// One 38 KB buffer, the next chunk in flight in registers (convtr2d_dgrad_bf16_kernel's schedule).  The epilogue adds (sum dlow, sum dlow *
// x_low) per block into gstats, replica row block % reps.
//
// Weight gradient (subpix2d_wgrad_bf16_kernel): the sixteen (class, tap half) 32 x 32 matrices M[a, b, u, v][co][ci] = sum_{i, j} dz[2i + a,
// 2j + b, co] * g[i + a - 1 + u, j + b - 1 + v, ci] over 8 x 16 low-res tiles; wave w owns class w (4 accumulators), its dz plane and the
// shared low-res halo sit in LDS as [pixel][32 channels] and are fetched with ds_read_b64_tr_b16 (8-byte aligned addresses: 64-byte pixels,
// lane offsets multiples of 8).  Every block writes its 16 matrices to its workspace slot; subpix2d_wgrad_bf16_fold_kernel folds them into
// the nine taps (4 matrices per tap) and adds the slots in slot order: no atomics, the same inputs give the same bits.
namespace {

namespace sp2b {
constexpr int T = 16;                       // low-res tile edge
constexpr int PS = 32;                      // bytes per staged pixel (16 bf16)
// forward: the 3x3 kernel's halo
constexpr int FH = T + 2;                   // 18
constexpr int FRS = FH * PS + 16;           // 592 bytes per row: 37 slots
constexpr int FBUF = FH * FRS;              // 10656
constexpr int FITEMS = FH * FH * 2;         // 648 (pixel, channel octet) items per chunk
constexpr int FNIT = (FITEMS + 255) / 256;  // 3
constexpr int F_LDS_BYTES = 2 * FBUF;       // 21312 (double-buffered)
// data gradient: four parity planes
constexpr int DP = T + 1;                   // 17 rows / columns per plane
constexpr int DRS = DP * PS + 16;           // 560 bytes per row: 35 slots
constexpr int DPL = DP * DRS;               // 9520 bytes per plane
constexpr int DITEMS = 4 * DP * DP * 2;     // 2312
constexpr int DNIT = (DITEMS + 255) / 256;  // 10
constexpr int D_LDS_BYTES = 4 * DPL;        // 38080 (the final [4][32][2] float reduction reuses the first 1024)
// weight gradient
constexpr int WTY = 8;                      // tile rows (x 16 columns) of the low-res grid
constexpr int WHY = WTY + 2, WHX = T + 2;   // 10 x 18 low-res halo
constexpr int WPP = 64;                     // bytes per staged pixel (32 bf16)
constexpr int W_G = 0;                      // [10 * 18][32] bf16
constexpr int W_DZ = WHY * WHX * WPP;       // 11520: [4 planes][8 * 16][32] bf16
constexpr int W_LDS_BYTES = W_DZ + 4 * WTY * T * WPP;  // 44288
constexpr int W_GIT = (WHY * WHX * 4 + 255) / 256;     // 3 halo items (pixel, octet) per thread
constexpr int W_DIT = 4 * WTY * T * 4 / 256;           // 8 dz items per thread
constexpr int W_DB = 4;                                // dz items staged per batch

// the sixteen (class, tap half) products of one chunk in halo-position order: q = (2a + b) * 4 + 2u + v reads halo offset (a + u, b + v)
struct Seq {
    int q[16], pos[16];
};
constexpr Seq make_seq() {
    Seq s{};
    int n = 0;
    for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx)
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b) {
                    const int u = dy - a, v = dx - b;
                    if (u < 0 || u > 1 || v < 0 || v > 1) continue;
                    s.q[n] = (2 * a + b) * 4 + 2 * u + v;
                    s.pos[n] = dy * 3 + dx;
                    ++n;
                }
    return s;
}
}  // namespace sp2b

inline bool sp2b_ok(int C1, int Cout) { return C1 > 0 && Cout > 0 && C1 % 32 == 0 && Cout % 32 == 0; }
inline bool sp2b_dims_ok(int N, int H1, int W1, int C1, int Cout) {
    return N > 0 && H1 > 0 && W1 > 0 && (long long)N * 4 * H1 * W1 < (1ll << 31) && (long long)16 * C1 * Cout < (1ll << 31);
}

// the taps of the 3-tap axis summed into tap half e of parity p (forward, index 2p + e) and into gather row r (data gradient)
__device__ __forceinline__ void sp2b_taps_fwd(int p, int e, int& t0, int& t1) {
    t0 = (p == 0) ? (e == 0 ? 0 : 1) : (e == 0 ? 0 : 2);
    t1 = (p == 0) ? (e == 0 ? 0 : 2) : (e == 0 ? 1 : 2);
}
__device__ __forceinline__ void sp2b_taps_dgrad(int r, int& t0, int& t1) {
    t0 = r == 0 ? 2 : (r == 1 ? 1 : 0);
    t1 = r == 0 ? 2 : (r == 1 ? 2 : (r == 2 ? 1 : 0));
}

// images [K / 16 chunk][16][n-tile][lane][8] of B[k][n], the fragment layout of pack_weights2d_bf16_kernel; w (Cout, cs, 3, 3), channels
// from coff.  dgrad == 0: entry q = (2a + b) * 4 + 2u + v, B[k = ci][n = co]; dgrad == 1: entry 4 ry + rx, B[k = co][n = ci].  The taps
// are added in fp32 in ascending (ty, tx) order, then rounded once.
__global__ void pack_subpix2d_bf16_kernel(const float* __restrict__ w, int cs, int coff, int dgrad, int ntg, long long total,
                                          __bf16* __restrict__ packed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        long long r = i >> 9;
        const int nt = (int)(r % ntg);
        r /= ntg;
        const int q = (int)(r % 16);
        const int chunk = (int)(r / 16);
        const int k = chunk * 16 + 8 * (lane >> 5) + j;
        const int nn = nt * 32 + (lane & 31);
        int y0, y1, x0, x1;
        if (dgrad == 0) {
            sp2b_taps_fwd(q >> 3, (q >> 1) & 1, y0, y1);
            sp2b_taps_fwd((q >> 2) & 1, q & 1, x0, x1);
        } else {
            sp2b_taps_dgrad(q >> 2, y0, y1);
            sp2b_taps_dgrad(q & 3, x0, x1);
        }
        const float* base = dgrad == 0 ? w + ((size_t)nn * cs + coff + k) * 9 : w + ((size_t)k * cs + coff + nn) * 9;
        float v = 0.f;
        for (int ty = y0; ty <= y1; ty += (y1 > y0 ? y1 - y0 : 1))
            for (int tx = x0; tx <= x1; tx += (x1 > x0 ? x1 - x0 : 1)) v += base[ty * 3 + tx];
        packed[i] = (__bf16)v;
    }
}

struct Subpix2dBf16Params {
    const float* src;     // forward: low (N,H1,W1,C1); data gradient: dz (N,2H1,2W1,Cout)
    const float* affine;  // forward: (a, b) rows of the C1 channels, sample n at affine + n * astride; or null
    long long astride;
    const c2b_bf16x8* wp;
    const float* x_low;   // data gradient: (N,H1,W1,C1) for gstats, or null
    float* out;           // forward: out (N,2H1,2W1,Cout); data gradient: dlow (N,H1,W1,C1)
    double* gstats;
    int N, H1, W1, C1, Cout;
    int nchunks, ntg, ty, tx, reps;
};

__global__ __launch_bounds__(256, 2) void subpix2d_fwd_bf16_kernel(const Subpix2dBf16Params p) {
    using namespace sp2b;
    extern __shared__ __attribute__((aligned(16))) char lds_sp2f[];
    char* const lds = lds_sp2f;
    const int t = threadIdx.x;
    const int l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int tile = blockIdx.x;
    const int cb = tile % p.ntg;
    tile /= p.ntg;
    const int txi = tile % p.tx;
    tile /= p.tx;
    const int tyi = tile % p.ty;
    const int n = tile / p.ty;
    const int y0 = tyi * T, x0 = txi * T;
    const int H1 = p.H1, W1 = p.W1, C1 = p.C1;

    int ldsoff[FNIT], gpix[FNIT];  // gpix < 0: outside the image (stays exactly 0)
#pragma unroll
    for (int it = 0; it < FNIT; ++it) {
        const int item = t + 256 * it;
        const bool in = item < FITEMS;
        const int pix = item >> 1, q = item & 1;
        const int hy = pix / FH, hx = pix - (pix / FH) * FH;
        const int gy = y0 - 1 + hy, gxx = x0 - 1 + hx;
        const bool ok = in && gy >= 0 && gy < H1 && gxx >= 0 && gxx < W1;
        ldsoff[it] = in ? hy * FRS + hx * PS + 16 * q : -1;
        gpix[it] = ok ? (n * H1 + gy) * W1 + gxx : -1;
    }
    const float* const aff_n = p.affine != nullptr ? p.affine + (size_t)n * p.astride : nullptr;
    f32x4 raw[FNIT][2];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int it = 0; it < FNIT; ++it) {
            raw[it][0] = raw[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (gpix[it] >= 0) {
                const float* src = p.src + (size_t)gpix[it] * C1 + c * 16 + 8 * ((t + 256 * it) & 1);
                raw[it][0] = u3d_ldq(src);
                raw[it][1] = u3d_ldq(src + 4);
            }
        }
    };
    auto store_chunk = [&](int c, char* buf) {
#pragma unroll
        for (int it = 0; it < FNIT; ++it) {
            if (ldsoff[it] < 0) continue;
            const bool ok = gpix[it] >= 0;
            const float* aff = (aff_n != nullptr && ok) ? aff_n + (c * 16 + 8 * ((t + 256 * it) & 1)) * 2 : nullptr;
            *reinterpret_cast<c2b_bf16x8*>(buf + ldsoff[it]) = c2b_stage8(raw[it][0], raw[it][1], aff, ok);
        }
    };

    f32x16 acc[2][4];  // [M-tile][parity class 2a + b]
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int cls = 0; cls < 4; ++cls)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][cls][r] = 0.f;

    // A-fragment base: lane (i32, h) of M-tile mt owns low-res pixel (4w + 2mt + (i32 >> 4), i32 & 15), channels 8h .. 8h + 7; halo offset
    // (dy, dx) of it is halo pixel (+dy, +dx)
    const int abase = (4 * w + (i32 >> 4)) * FRS + (i32 & 15) * PS + 16 * h;
    auto bidx = [&](int c, int q) -> long long { return ((long long)(c * 16 + q) * p.ntg + cb) * 64 + l; };
    constexpr Seq SQ = make_seq();

    load_chunk(0);
    store_chunk(0, lds);
    __syncthreads();
    for (int c = 0; c < p.nchunks; ++c) {
        const char* cur = lds + (c & 1) * FBUF;
        if (c + 1 < p.nchunks) load_chunk(c + 1);  // in flight during the MFMAs
        c2b_bf16x8 bq = p.wp[bidx(c, SQ.q[0])], bn = bq;
        c2b_bf16x8 a[2];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            if (s + 1 < 16) bn = p.wp[bidx(c, SQ.q[s + 1])];
            if (s == 0 || SQ.pos[s] != SQ.pos[s - 1]) {
                const int dy = SQ.pos[s] / 3, dx = SQ.pos[s] - (SQ.pos[s] / 3) * 3;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) a[mt] = *reinterpret_cast<const c2b_bf16x8*>(cur + abase + (2 * mt + dy) * FRS + dx * PS);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                acc[mt][SQ.q[s] >> 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt], bq, acc[mt][SQ.q[s] >> 2], 0, 0, 0);
            bq = bn;
        }
        if (c + 1 < p.nchunks) store_chunk(c + 1, lds + ((c + 1) & 1) * FBUF);  // (that buffer was last read in chunk c - 1)
        __syncthreads();
    }

    // ---- lane column = output channel, register r = M row (r & 3) + 8 (r >> 2) + 4h; class (a, b) of low-res (i, j) is out[2i + a][2j + b]
    const int co = cb * 32 + i32;
    const int Ho = 2 * H1, Wo = 2 * W1;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int cls = 0; cls < 4; ++cls)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int i = y0 + 4 * w + 2 * mt + (row >> 4), j = x0 + (row & 15);
                if (i >= H1 || j >= W1) continue;
                p.out[((size_t)(n * Ho + 2 * i + (cls >> 1)) * Wo + 2 * j + (cls & 1)) * p.Cout + co] = acc[mt][cls][r];
            }
}

__global__ __launch_bounds__(256, 2) void subpix2d_dgrad_bf16_kernel(const Subpix2dBf16Params p) {
    using namespace sp2b;
    extern __shared__ __attribute__((aligned(16))) char lds_sp2d[];
    char* const lds = lds_sp2d;
    const int t = threadIdx.x;
    const int l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int tile = blockIdx.x;
    const int cb = tile % p.ntg;
    tile /= p.ntg;
    const int txi = tile % p.tx;
    tile /= p.tx;
    const int tyi = tile % p.ty;
    const int n = tile / p.ty;
    const int y0 = tyi * T, x0 = txi * T;
    const int H1 = p.H1, W1 = p.W1, Hd = 2 * p.H1, Wd = 2 * p.W1, K = p.Cout;  // the contraction runs over the layer's Cout

    // item = (plane 2pa + pb, plane row py, plane column px, channel octet q): dz pixel (2 (y0 + py) - pa, 2 (x0 + px) - pb)
    int ldsoff[DNIT], gpix[DNIT];  // gpix < 0: outside dz (zero)
#pragma unroll
    for (int it = 0; it < DNIT; ++it) {
        const int item = t + 256 * it;
        const bool in = item < DITEMS;
        const int q = item & 1;
        int pix = item >> 1;
        const int px = pix % DP;
        pix /= DP;
        const int py = pix % DP;
        const int pl = pix / DP;
        const int gy = 2 * (y0 + py) - (pl >> 1), gxx = 2 * (x0 + px) - (pl & 1);
        const bool ok = in && gy >= 0 && gy < Hd && gxx >= 0 && gxx < Wd;
        ldsoff[it] = in ? pl * DPL + py * DRS + px * PS + 16 * q : -1;
        gpix[it] = ok ? (n * Hd + gy) * Wd + gxx : -1;
    }
    f32x4 raw[DNIT][2];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int it = 0; it < DNIT; ++it) {
            raw[it][0] = raw[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (gpix[it] >= 0) {
                const float* src = p.src + (size_t)gpix[it] * K + c * 16 + 8 * ((t + 256 * it) & 1);
                raw[it][0] = u3d_ldq(src);
                raw[it][1] = u3d_ldq(src + 4);
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int it = 0; it < DNIT; ++it)
            if (ldsoff[it] >= 0)
                *reinterpret_cast<c2b_bf16x8*>(lds + ldsoff[it]) = c2b_stage8(raw[it][0], raw[it][1], nullptr, gpix[it] >= 0);
    };

    f32x16 acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;

    // lane (i32, h) of M-tile mt owns dlow pixel (ii, jj) = (4w + 2mt + (i32 >> 4), i32 & 15); gather row ry reads dz row 2 (y0 + ii) - 1 + ry:
    // plane pa = (ry + 1) & 1, plane row ii + (ry >> 1); columns alike
    const int abase = (4 * w + (i32 >> 4)) * DRS + (i32 & 15) * PS + 16 * h;
    auto bidx = [&](int c, int q) -> long long { return ((long long)(c * 16 + q) * p.ntg + cb) * 64 + l; };

    load_chunk(0);
    store_chunk();
    __syncthreads();
    for (int c = 0; c < p.nchunks; ++c) {
        if (c + 1 < p.nchunks) load_chunk(c + 1);  // in flight during the MFMAs
        c2b_bf16x8 bq = p.wp[bidx(c, 0)], bn = bq;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int ry = q >> 2, rx = q & 3;
            if (q + 1 < 16) bn = p.wp[bidx(c, q + 1)];
            const int toff = (2 * ((ry + 1) & 1) + ((rx + 1) & 1)) * DPL + (ry >> 1) * DRS + (rx >> 1) * PS;
            c2b_bf16x8 a[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) a[mt] = *reinterpret_cast<const c2b_bf16x8*>(lds + abase + toff + 2 * mt * DRS);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mt], bq, acc[mt], 0, 0, 0);
            bq = bn;
        }
        __syncthreads();  // every wave is done reading the one buffer
        if (c + 1 < p.nchunks) {
            store_chunk();
            __syncthreads();
        }
    }

    const int ci = cb * 32 + i32;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int y = y0 + 4 * w + 2 * mt + (row >> 4), x = x0 + (row & 15);
            if (y >= H1 || x >= W1) continue;
            const size_t o = ((size_t)(n * H1 + y) * W1 + x) * p.C1 + ci;
            const float v = acc[mt][r];
            p.out[o] = v;
            if (p.gstats != nullptr) {
                s0 += v;
                s1 += v * p.x_low[o];
            }
        }
    if (p.gstats != nullptr) {  // (uniform over the grid) lane halves, then the 4 waves in a fixed order, one f64 atomic per quantity
        float* red = reinterpret_cast<float*>(lds);  // [4][32][2]; the last barrier of the chunk loop freed the buffer
        s0 += __shfl_xor(s0, 32);
        s1 += __shfl_xor(s1, 32);
        if (l < 32) {
            red[(w * 32 + l) * 2] = s0;
            red[(w * 32 + l) * 2 + 1] = s1;
        }
        __syncthreads();
        if (t < 32) {
            const float a0 = ((red[t * 2] + red[(32 + t) * 2]) + red[(64 + t) * 2]) + red[(96 + t) * 2];
            const float a1 = ((red[t * 2 + 1] + red[(32 + t) * 2 + 1]) + red[(64 + t) * 2 + 1]) + red[(96 + t) * 2 + 1];
            double* o = p.gstats + ((size_t)(blockIdx.x % p.reps) * p.N * p.C1 + (size_t)n * p.C1 + cb * 32 + t) * 2;
            u3d_atomic_add_f64(o, (double)a0);
            u3d_atomic_add_f64(o + 1, (double)a1);
        }
    }
}

struct Subpix2dWgradBf16Params {
    const float* low;     // (N,H1,W1,C1)
    const float* affine;  // rows of the C1 channels, sample n at affine + n * astride; or null
    long long astride;
    const float* dz;      // (N,2H1,2W1,Cout)
    float* ws;            // [nsplit][16][Cout][C1]
    int N, H1, W1, C1, Cout;
    int ty, tx, ncob, ncib, ntiles, tps;
};

__global__ __launch_bounds__(256, 2) void subpix2d_wgrad_bf16_kernel(const Subpix2dWgradBf16Params p) {
    using namespace sp2b;
    extern __shared__ __attribute__((aligned(16))) char lds_sp2w[];
    char* const lds = lds_sp2w;
    const int t = threadIdx.x, l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int b = blockIdx.x;
    const int cib = b % p.ncib;
    b /= p.ncib;
    const int cob = b % p.ncob;
    const int split = b / p.ncob;
    const int ci0 = cib * 32, co0 = cob * 32;
    const int tile0 = split * p.tps, tile1 = min(p.ntiles, tile0 + p.tps);
    const int H1 = p.H1, W1 = p.W1, Hd = 2 * p.H1, Wd = 2 * p.W1, C1 = p.C1, Cout = p.Cout;
    char* const gl = lds + W_G;
    char* const dzl = lds + W_DZ;
    const int pa = w >> 1, pb = w & 1;  // this wave's parity class

    f32x16 acc[4];  // [tap half 2u + v]
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    // transposed-read lane offset, as conv2d_wgrad_bf16_kernel: lane l receives channel (l & 31) of the 8 pixels 8 * (l >> 5) .. + 7
    const int g4 = l >> 4, sidx = l & 15;
    const int lane_off = (8 * (g4 >> 1) + (sidx >> 2)) * WPP + (16 * (g4 & 1) + 4 * (sidx & 3)) * 2;

    for (int tile = tile0; tile < tile1; ++tile) {
        int tt = tile;
        const int txi = tt % p.tx;
        tt /= p.tx;
        const int tyi = tt % p.ty;
        const int n = tt / p.ty;
        const int y0 = tyi * WTY, x0 = txi * T;
        const float* const aff_n = p.affine != nullptr ? p.affine + (size_t)n * p.astride : nullptr;
        // stage g (10 x 18 low-res halo from (y0 - 1, x0 - 1), 32 channels from ci0, affine, zero padding) ...
        {
            f32x4 rg[W_GIT][2];
            bool okg[W_GIT];
#pragma unroll
            for (int k = 0; k < W_GIT; ++k) {
                const int item = t + 256 * k;
                const int pix = item >> 2, q = item & 3;
                const int hy = pix / WHX, hx = pix - (pix / WHX) * WHX;
                const int gy = y0 - 1 + hy, gxx = x0 - 1 + hx;
                okg[k] = item < WHY * WHX * 4 && gy >= 0 && gy < H1 && gxx >= 0 && gxx < W1;
                rg[k][0] = rg[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (okg[k]) {
                    const float* src = p.low + ((size_t)(n * H1 + gy) * W1 + gxx) * C1 + ci0 + 8 * q;
                    rg[k][0] = u3d_ldq(src);
                    rg[k][1] = u3d_ldq(src + 4);
                }
            }
#pragma unroll
            for (int k = 0; k < W_GIT; ++k) {
                const int item = t + 256 * k;
                if (item >= WHY * WHX * 4) continue;
                const float* aff = (aff_n != nullptr && okg[k]) ? aff_n + (ci0 + 8 * (item & 3)) * 2 : nullptr;
                *reinterpret_cast<c2b_bf16x8*>(gl + (item >> 2) * WPP + 16 * (item & 3)) = c2b_stage8(rg[k][0], rg[k][1], aff, okg[k]);
            }
        }
        // ... and dz de-interleaved into its four parity planes (8 x 16 pixels each, 32 channels from co0): plane (a, b), pixel (py, px) is
        // dz[2 (y0 + py) + a][2 (x0 + px) + b]
        auto stage_dz = [&](int it0) {
            f32x4 rd[W_DB][2];
            bool okd[W_DB];
#pragma unroll
            for (int k = 0; k < W_DB; ++k) {
                const int item = t + 256 * (it0 + k);
                const int q = item & 3, pix = (item >> 2) & (WTY * T - 1), pl = item >> 9;
                const int i = y0 + (pix >> 4), j = x0 + (pix & 15);
                okd[k] = i < H1 && j < W1;
                rd[k][0] = rd[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (okd[k]) {
                    const float* src = p.dz + ((size_t)(n * Hd + 2 * i + (pl >> 1)) * Wd + 2 * j + (pl & 1)) * Cout + co0 + 8 * q;
                    rd[k][0] = u3d_ldq(src);
                    rd[k][1] = u3d_ldq(src + 4);
                }
            }
#pragma unroll
            for (int k = 0; k < W_DB; ++k) {
                const int item = t + 256 * (it0 + k);
                *reinterpret_cast<c2b_bf16x8*>(dzl + (item >> 2) * WPP + 16 * (item & 3)) = c2b_stage8(rd[k][0], rd[k][1], nullptr, okd[k]);
            }
        };
        for (int it0 = 0; it0 < W_DIT; it0 += W_DB) stage_dz(it0);
        __syncthreads();
        // wave w = class (pa, pb): all 8 rows of its dz plane, one 16-pixel row per k-step; tap half (u, v) pairs dz plane pixel (py, jj) with
        // low-res halo pixel (py + pa + u, jj + pb + v)
#pragma unroll 2
        for (int py = 0; py < WTY; ++py) {
            const c2b_bf16x8 a = c2b_tr_frag(dzl + (w * WTY * T + py * T) * WPP + lane_off);
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const c2b_bf16x8 g = c2b_tr_frag(gl + ((py + pa + u) * WHX + pb + v) * WPP + lane_off);
                    acc[2 * u + v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, g, acc[2 * u + v], 0, 0, 0);
                }
        }
        __syncthreads();
    }

    // ---- this block's slot: matrix q = 4w + 2u + v, [co][ci]; register r = output channel (r & 3) + 8 (r >> 2) + 4h, lane column = ci
    float* const dst = p.ws + ((size_t)split * 16 + 4 * w) * Cout * C1;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            dst[((size_t)k * Cout + co0 + row) * C1 + ci0 + i32] = acc[k][r];
        }
}

// dw[co][ci][ky][kx] = sum over slots in slot order of the 4 matrices that carry the tap: per axis tap 0 <- (p, e) = (0, 0), (1, 0); tap 1 <-
// (0, 1), (1, 0); tap 2 <- (0, 1), (1, 1).  drow = 9 * dw_cin_stride elements per output channel of dw.
__global__ void subpix2d_wgrad_bf16_fold_kernel(const float* __restrict__ ws, int nsplit, int Cout, int C1, float* __restrict__ dw,
                                                long long drow) {
    const long long total = (long long)Cout * C1 * 9;
    const size_t mat = (size_t)Cout * C1;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int tap = (int)(i % 9);
        const long long cc = i / 9;  // co * C1 + ci
        const int ky = tap / 3, kx = tap - ky * 3;
        // (parity, tap half) pairs of the two contributions per axis
        const int ay0 = 0, uy0 = ky == 0 ? 0 : 1, ay1 = 1, uy1 = ky == 2 ? 1 : 0;
        const int ax0 = 0, ux0 = kx == 0 ? 0 : 1, ax1 = 1, ux1 = kx == 2 ? 1 : 0;
        const int q00 = (2 * ay0 + ax0) * 4 + 2 * uy0 + ux0, q01 = (2 * ay0 + ax1) * 4 + 2 * uy0 + ux1;
        const int q10 = (2 * ay1 + ax0) * 4 + 2 * uy1 + ux0, q11 = (2 * ay1 + ax1) * 4 + 2 * uy1 + ux1;
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) {
            const float* m = ws + (size_t)s * 16 * mat + cc;
            v += ((m[q00 * mat] + m[q01 * mat]) + m[q10 * mat]) + m[q11 * mat];
        }
        dw[(cc / C1) * drow + (cc % C1) * 9 + tap] = v;
    }
}

struct Sp2bWPlan {
    int ty, tx, ncob, ncib, ntiles, tps, nsplit;
};

// ~4 blocks per CU over the launch; ONE function for the launcher and the workspace size
Sp2bWPlan sp2b_wplan(int device, int N, int H1, int W1, int C1, int Cout) {
    Sp2bWPlan pl;
    pl.ty = (int)c2b_cdiv(H1, sp2b::WTY);
    pl.tx = (int)c2b_cdiv(W1, sp2b::T);
    pl.ncob = Cout / 32;
    pl.ncib = C1 / 32;
    pl.ntiles = N * pl.ty * pl.tx;
    const long long cells = (long long)pl.ncob * pl.ncib;
    const long long target = 4LL * c2b_cu_count(device);
    const long long ns = std::max<long long>(1, std::min<long long>(pl.ntiles, c2b_cdiv(target, cells)));
    pl.tps = (int)c2b_cdiv(pl.ntiles, ns);
    pl.nsplit = (int)c2b_cdiv(pl.ntiles, pl.tps);
    return pl;
}

}  // namespace

extern "C" long long u3d_subpixel2d_bf16_packed_elems(int C1, int Cout, int dgrad) {
    if ((dgrad != 0 && dgrad != 1) || !sp2b_ok(C1, Cout) || (long long)16 * C1 * Cout >= (1ll << 31)) return 0;
    return (long long)16 * C1 * Cout;  // [K / 16][16][Nn / 32][64][8]
}

extern "C" int u3d_pack_subpixel2d_weights_bf16(int device, u3d_stream_t stream, const float* w, int Cout, int Cin_total, int c_off, int C1,
                                                int dgrad, void* packed) {
    U3D_ENTER(device);
    U3D_REQUIRE(w && packed && (dgrad == 0 || dgrad == 1), "u3d_pack_subpixel2d_weights_bf16: bad argument");
    U3D_REQUIRE(sp2b_ok(C1, Cout) && (long long)16 * C1 * Cout < (1ll << 31),
                "u3d_pack_subpixel2d_weights_bf16: (%d -> %d) channels are outside the bf16 sub-pixel envelope (both %% 32)", C1, Cout);
    U3D_REQUIRE(c_off >= 0 && c_off + C1 <= Cin_total, "u3d_pack_subpixel2d_weights_bf16: channels [%d, %d) do not lie inside a weight of %d "
                "input channels", c_off, c_off + C1, Cin_total);
    U3D_REQUIRE(c2b_aligned(packed), "u3d_pack_subpixel2d_weights_bf16: the image must be 16-byte aligned");
    const long long total = (long long)16 * C1 * Cout;
    long long blocks = c2b_cdiv(total, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_subpix2d_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, Cin_total, c_off, dgrad,
                       (dgrad == 0 ? Cout : C1) / 32, total, reinterpret_cast<__bf16*>(packed));
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_subpixel2d_conv_fwd_bf16(int device, u3d_stream_t stream, const float* low, const float* affine,
                                            long long affine_sample_stride, const void* packed, float* out, int N, int H1, int W1, int C1,
                                            int Cout) {
    U3D_ENTER(device);
    U3D_REQUIRE(sp2b_ok(C1, Cout), "u3d_subpixel2d_conv_fwd_bf16: (%d -> %d) channels are outside the bf16 sub-pixel envelope (both %% 32)", C1,
                Cout);
    U3D_REQUIRE(low && packed && out, "u3d_subpixel2d_conv_fwd_bf16: bad argument");
    U3D_REQUIRE(sp2b_dims_ok(N, H1, W1, C1, Cout), "u3d_subpixel2d_conv_fwd_bf16: bad sizes (the output pixel count must be < 2^31)");
    U3D_REQUIRE(c2b_aligned(low) && c2b_aligned(affine) && c2b_aligned(packed) && c2b_aligned(out) && affine_sample_stride % 4 == 0,
                "u3d_subpixel2d_conv_fwd_bf16: pointers must be 16-byte aligned");
    Subpix2dBf16Params p = {};
    p.src = low;
    p.affine = affine;
    p.astride = affine_sample_stride;
    p.wp = reinterpret_cast<const c2b_bf16x8*>(packed);
    p.out = out;
    p.N = N, p.H1 = H1, p.W1 = W1, p.C1 = C1, p.Cout = Cout;
    p.nchunks = C1 / 16, p.ntg = Cout / 32, p.reps = 1;
    p.ty = (int)c2b_cdiv(H1, sp2b::T), p.tx = (int)c2b_cdiv(W1, sp2b::T);
    const long long blocks = (long long)N * p.ty * p.tx * p.ntg;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_subpixel2d_conv_fwd_bf16: grid too large");
    hipLaunchKernelGGL(subpix2d_fwd_bf16_kernel, dim3((unsigned)blocks), dim3(256), sp2b::F_LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_subpixel2d_conv_dgrad_bf16(int device, u3d_stream_t stream, const float* dz, const void* packed, const float* x_low,
                                              float* dlow, double* gstats, int N, int H1, int W1, int C1, int Cout, int reps) {
    U3D_ENTER(device);
    U3D_REQUIRE(sp2b_ok(C1, Cout), "u3d_subpixel2d_conv_dgrad_bf16: (%d -> %d) channels are outside the bf16 sub-pixel envelope (both %% 32)",
                C1, Cout);
    U3D_REQUIRE(dz && packed && dlow && reps >= 1 && (!gstats || x_low), "u3d_subpixel2d_conv_dgrad_bf16: bad argument (gstats needs x_low)");
    U3D_REQUIRE(sp2b_dims_ok(N, H1, W1, C1, Cout), "u3d_subpixel2d_conv_dgrad_bf16: bad sizes (the dz pixel count must be < 2^31)");
    U3D_REQUIRE(c2b_aligned(dz) && c2b_aligned(packed) && c2b_aligned(dlow) && c2b_aligned(x_low),
                "u3d_subpixel2d_conv_dgrad_bf16: pointers must be 16-byte aligned");
    Subpix2dBf16Params p = {};
    p.src = dz;
    p.wp = reinterpret_cast<const c2b_bf16x8*>(packed);
    p.x_low = x_low;
    p.out = dlow;
    p.gstats = gstats;
    p.N = N, p.H1 = H1, p.W1 = W1, p.C1 = C1, p.Cout = Cout;
    p.nchunks = Cout / 16, p.ntg = C1 / 32, p.reps = reps;
    p.ty = (int)c2b_cdiv(H1, sp2b::T), p.tx = (int)c2b_cdiv(W1, sp2b::T);
    const long long blocks = (long long)N * p.ty * p.tx * p.ntg;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_subpixel2d_conv_dgrad_bf16: grid too large");
    hipLaunchKernelGGL(subpix2d_dgrad_bf16_kernel, dim3((unsigned)blocks), dim3(256), sp2b::D_LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" long long u3d_subpixel2d_wgrad_bf16_workspace_floats(int N, int H1, int W1, int C1, int Cout) {
    if (!sp2b_ok(C1, Cout) || !sp2b_dims_ok(N, H1, W1, C1, Cout)) return 0;
    return (long long)sp2b_wplan(c2b_current_device(), N, H1, W1, C1, Cout).nsplit * 16 * C1 * Cout;
}

extern "C" int u3d_subpixel2d_conv_wgrad_bf16(int device, u3d_stream_t stream, const float* low, const float* affine,
                                              long long affine_sample_stride, const float* dz, float* dw, int dw_cin_stride, int N, int H1,
                                              int W1, int C1, int Cout, float* workspace, long long workspace_floats) {
    U3D_ENTER(device);
    U3D_REQUIRE(sp2b_ok(C1, Cout), "u3d_subpixel2d_conv_wgrad_bf16: (%d -> %d) channels are outside the bf16 sub-pixel envelope (both %% 32)",
                C1, Cout);
    U3D_REQUIRE(low && dz && dw && workspace && dw_cin_stride >= C1, "u3d_subpixel2d_conv_wgrad_bf16: bad argument");
    U3D_REQUIRE(sp2b_dims_ok(N, H1, W1, C1, Cout), "u3d_subpixel2d_conv_wgrad_bf16: bad sizes (the dz pixel count must be < 2^31)");
    U3D_REQUIRE(c2b_aligned(low) && c2b_aligned(affine) && c2b_aligned(dz) && c2b_aligned(workspace) && affine_sample_stride % 4 == 0,
                "u3d_subpixel2d_conv_wgrad_bf16: pointers must be 16-byte aligned");
    const Sp2bWPlan pl = sp2b_wplan(device, N, H1, W1, C1, Cout);
    const long long need = (long long)pl.nsplit * 16 * C1 * Cout;
    U3D_REQUIRE(workspace_floats >= need, "u3d_subpixel2d_conv_wgrad_bf16: workspace too small (%lld < %lld floats)", workspace_floats, need);
    Subpix2dWgradBf16Params p = {};
    p.low = low;
    p.affine = affine;
    p.astride = affine_sample_stride;
    p.dz = dz;
    p.ws = workspace;
    p.N = N, p.H1 = H1, p.W1 = W1, p.C1 = C1, p.Cout = Cout;
    p.ty = pl.ty, p.tx = pl.tx, p.ncob = pl.ncob, p.ncib = pl.ncib, p.ntiles = pl.ntiles, p.tps = pl.tps;
    const long long blocks = (long long)pl.nsplit * pl.ncob * pl.ncib;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_subpixel2d_conv_wgrad_bf16: grid too large");
    hipLaunchKernelGGL(subpix2d_wgrad_bf16_kernel, dim3((unsigned)blocks), dim3(256), sp2b::W_LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    const long long total = (long long)9 * C1 * Cout;
    long long rb = c2b_cdiv(total, 256);
    if (rb > 4096) rb = 4096;
    hipLaunchKernelGGL(subpix2d_wgrad_bf16_fold_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace, pl.nsplit, Cout, C1,
                       dw, (long long)9 * dw_cin_stride);
    U3D_LAUNCH_CHECK();
    return 0;
}
