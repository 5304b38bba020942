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
__global__ void pack_weights2d_bf16_kernel(const float* __restrict__ w, int Cout, int Cin, int mode, int K, int Nn, int ntg,
                                           long long total, __bf16* __restrict__ packed) {
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
            v = mode == 0 ? w[((size_t)nn * Cin + k) * 9 + tap] : w[((size_t)k * Cin + nn) * 9 + (8 - tap)];
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

template <int NT>
__global__ __launch_bounds__(256, 2) void conv2d_bf16_kernel(const Conv2dBf16Params p) {
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
        goff[it] = ok ? ((size_t)(n * H + gy) * W + gxx) * Cin : 0;
    }
    f32x4 raw[NIT][2];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            raw[it][0] = raw[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (oks[it]) {
                const float* src = p.x + goff[it] + c * CC + cqs[it];
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
                    s[nt][3] += v * p.gx[o];
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

__global__ __launch_bounds__(256, 2) void conv2d_wgrad_bf16_kernel(const Wgrad2dBf16Params p) {
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
                okg[k] = item < HY * HX * 4 && gy >= 0 && gy < H && gxx >= 0 && gxx < W;
                rg[k][0] = rg[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (okg[k]) {
                    const float* src = p.x + ((size_t)(n * H + gy) * W + gxx) * Cin + ci0 + 8 * q;
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
                okd[k] = y < H && x < W;
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
            if (co < Cout && ci < Cin) p.dst[(size_t)split * Cout * Cin * 9 + ((size_t)co * Cin + ci) * 9 + tap] = v;
        }
        __syncthreads();
    }
}

// dw[i] = sum over splits in split order (bitwise-reproducible)
__global__ void conv2d_wgrad_bf16_reduce_kernel(const float* __restrict__ ws, int nsplit, long long total, float* __restrict__ dw) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) v += ws[(size_t)s * total + i];
        dw[i] = v;
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

extern "C" long long u3d_packed_weight2d_bf16_elems(int Cin, int Cout, int mode) {
    if (mode != 0 && mode != 1) return 0;
    int K, Nn;
    c2b_dims(Cin, Cout, mode, K, Nn);
    if (!c2b_fwd_ok(K, Nn)) return 0;
    return (long long)(K / c2b::CC) * 9 * (Nn / 32) * 64 * 8;
}

extern "C" int u3d_pack_weights2d_bf16(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, void* packed) {
    U3D_ENTER(device);
    U3D_REQUIRE(w && packed && Cout > 0 && Cin > 0 && (mode == 0 || mode == 1), "u3d_pack_weights2d_bf16: bad argument");
    int K, Nn;
    c2b_dims(Cin, Cout, mode, K, Nn);
    U3D_REQUIRE(c2b_fwd_ok(K, Nn), "u3d_pack_weights2d_bf16: mode %d of a (%d -> %d) weight is outside the bf16 envelope (contraction %% 16, "
                "produced %% 32)", mode, Cin, Cout);
    U3D_REQUIRE(c2b_aligned(packed), "u3d_pack_weights2d_bf16: the image must be 16-byte aligned");
    const long long total = u3d_packed_weight2d_bf16_elems(Cin, Cout, mode);
    long long blocks = c2b_cdiv(total, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_weights2d_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin, mode, K, Nn,
                       Nn / 32, total, reinterpret_cast<__bf16*>(packed));
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" long long u3d_conv2d_bf16_workspace_floats(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || !c2b_fwd_ok(Cin, Cout)) return 0;
    const C2bPlan pl = c2b_plan(c2b_current_device(), N, H, W, Cin, Cout);
    return pl.ksplit > 1 ? (long long)pl.ksplit * N * H * W * Cout : 0;
}

// host-only query of that plan (tests assert that the shapes they pin really run the variants a full-resolution level runs)
extern "C" int u3d_conv2d_bf16_variant(int N, int H, int W, int Cin, int Cout, int has_workspace) {
    if (N <= 0 || H <= 0 || W <= 0 || !c2b_fwd_ok(Cin, Cout)) return -1;
    const C2bPlan pl = c2b_plan(c2b_current_device(), N, H, W, Cin, Cout);
    return (c2b_launch_ksplit(pl, has_workspace != 0) << 8) | pl.nt;
}

namespace {

// the one launcher behind u3d_conv2d_bf16 (residual == nullptr) and u3d_conv2d_bf16_res: same plan, same kernels
int c2b_conv2d_launch(const char* who, int device, u3d_stream_t stream, const float* x, const float* affine, const void* packed_w,
                      float* out, int N, int H, int W, int Cin, int Cout, int relu, double* out_stats, const float* gx, double* gstats,
                      float* workspace, long long workspace_floats, int stat_reps, const float* residual) {
    U3D_ENTER(device);
    U3D_REQUIRE(c2b_fwd_ok(Cin, Cout), "%s: (%d -> %d) channels are outside the bf16 envelope (Cin %% 16, Cout %% 32)", who, Cin,
                Cout);
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
    if (pl.nt == 2)
        hipLaunchKernelGGL(conv2d_bf16_kernel<2>, dim3((unsigned)blocks), dim3(256), c2b::LDS_BYTES, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(conv2d_bf16_kernel<1>, dim3((unsigned)blocks), dim3(256), c2b::LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    if (split) {
        const int P = H * W;
        hipLaunchKernelGGL(conv2d_bf16_splitk_reduce_kernel, dim3((unsigned)c2b_cdiv(P, 64), N), dim3(256), 0, (hipStream_t)stream, workspace,
                           p.part_stride, p.ksplit, out, P, Cout, p.relu, out_stats, gx, gstats, residual);
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

// out = [relu](conv2d(bf16(a*x + b), bf16(w)) + residual): the bf16 twin of u3d_conv2d_res_reps.  The plan (u3d_conv2d_bf16_variant,
// u3d_conv2d_bf16_workspace_floats) does not depend on the residual.
extern "C" int u3d_conv2d_bf16_res(int device, u3d_stream_t stream, const float* x, const float* affine, const void* packed_w, float* out,
                                   int N, int H, int W, int Cin, int Cout, int relu, double* out_stats, const float* gx, double* gstats,
                                   float* workspace, long long workspace_floats, int stat_reps, const float* residual) {
    U3D_REQUIRE(residual && !gx && !gstats, "u3d_conv2d_bf16_res: needs a residual, and a residual excludes gx / gstats");
    return c2b_conv2d_launch("u3d_conv2d_bf16_res", device, stream, x, affine, packed_w, out, N, H, W, Cin, Cout, relu, out_stats, nullptr,
                             nullptr, workspace, workspace_floats, stat_reps, residual);
}

extern "C" long long u3d_wgrad2d_bf16_workspace_floats(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || !c2b_wgrad_ok(Cin, Cout)) return 0;
    const W2bPlan pl = w2b_plan(c2b_current_device(), N, H, W, Cin, Cout);
    return pl.nsplit > 1 ? (long long)pl.nsplit * Cout * Cin * 9 : 0;
}

extern "C" int u3d_conv2d_wgrad_bf16_variant(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || !c2b_wgrad_ok(Cin, Cout)) return -1;
    const W2bPlan pl = w2b_plan(c2b_current_device(), N, H, W, Cin, Cout);
    return (std::min(pl.tps, 0x7fff) << 16) | std::min(pl.nsplit, 0xffff);
}

extern "C" int u3d_conv2d_wgrad_bf16(int device, u3d_stream_t stream, const float* x, const float* affine, const float* dz, float* dw,
                                     int N, int H, int W, int Cin, int Cout, float* workspace, long long workspace_floats) {
    U3D_ENTER(device);
    U3D_REQUIRE(c2b_wgrad_ok(Cin, Cout), "u3d_conv2d_wgrad_bf16: (%d -> %d) channels are outside the bf16 envelope (both %% 32)", Cin,
                Cout);
    U3D_REQUIRE(x && dz && dw && N > 0 && H > 0 && W > 0 && (long long)N * H * W < (1LL << 31), "u3d_conv2d_wgrad_bf16: bad argument");
    U3D_REQUIRE(c2b_aligned(x) && c2b_aligned(affine) && c2b_aligned(dz), "u3d_conv2d_wgrad_bf16: pointers must be 16-byte aligned");
    const W2bPlan pl = w2b_plan(device, N, H, W, Cin, Cout);
    const long long need = pl.nsplit > 1 ? (long long)pl.nsplit * Cout * Cin * 9 : 0;
    U3D_REQUIRE(need == 0 || (workspace && workspace_floats >= need), "u3d_conv2d_wgrad_bf16: workspace too small (%lld < %lld floats)",
                workspace_floats, need);
    Wgrad2dBf16Params p = {};
    p.x = x;
    p.affine = affine;
    p.dz = dz;
    p.dst = need ? workspace : dw;
    p.N = N, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout;
    p.ty = pl.ty, p.tx = pl.tx, p.ncob = pl.ncob, p.ncib = pl.ncib, p.ntiles = pl.ntiles, p.tps = pl.tps;
    const long long blocks = (long long)pl.nsplit * pl.ncob * pl.ncib;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_conv2d_wgrad_bf16: grid too large");
    hipLaunchKernelGGL(conv2d_wgrad_bf16_kernel, dim3((unsigned)blocks), dim3(256), c2b::WG_LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    if (need) {
        const long long total = (long long)Cout * Cin * 9;
        long long rb = c2b_cdiv(total, 256);
        if (rb > 4096) rb = 4096;
        hipLaunchKernelGGL(conv2d_wgrad_bf16_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace, pl.nsplit, total,
                           dw);
        U3D_LAUNCH_CHECK();
    }
    return 0;
}
