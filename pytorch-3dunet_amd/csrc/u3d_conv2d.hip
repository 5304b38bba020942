// u3d_conv2d.hip — the 2-D path of UNet2D (reference model.py:281-318, `native_2d: true`): Conv2d 3x3 (stride 1, pad 1, bias-free)
// forward / data gradient / weight gradient as implicit GEMM on the gfx950 fp32 matrix cores (v_mfma_f32_32x32x2_f32), the packed
// weight images they read, and MaxPool2d(2) forward / backward merges.
//
// Replaces the ATen kernels behind nn.Conv2d(in, out, 3, padding=1, bias=False) (buildingblocks.py:55-58) and its autograd, and
// nn.MaxPool2d(kernel_size=2) (buildingblocks.py:358).  Activations are NHWC fp32 — the library's NDHWC layout with D = 1 — so the
// GroupNorm / BatchNorm statistics, the fused apply passes, the virtual concat (u3d_src_t with nearest maps), the 1x1 head, the loss
// and the optimizer of the 3-D path run unchanged on them; only the 3x3x3 convolutions (4x8x8 tiles, 27 taps) and the 2x2x2 pool are
// genuinely 3-D.
//
// Forward / data gradient (conv2d_mfma_kernel): a block = 4 waves owns a 16(y) x 16(x) pixel tile (256 GEMM rows) and BN = 32*NT
// output channels.  Per 16-channel input chunk the 18x18 halo goes through LDS with the GroupNorm / BatchNorm affine applied while
// staging (zero padding stays exactly 0), layout [hy][hx][16] with a pixel stride of 20 floats and a row stride of 384 — conflict-free
// for the ds_read_b128 A-fragment reads of a 2(y) x 16(x) M-tile at every tap (tools/lds_bank_model.py).  Double-buffered: the next
// chunk's halo is loaded into registers before the current chunk's 72 MFMAs per M-tile and stored into the other buffer after them,
// one barrier per chunk.  B fragments stream from the packed global image, one step ahead.  Small grids split the channel reduction
// over blocks (split-K) and add the partial sums in a fixed order (conv2d_splitk_reduce_kernel).
//
// Weight gradient (conv2d_wgrad_kernel): a block owns 32 output x 32 input channels x 9 taps (9 x 16 accumulator registers per wave)
// and a contiguous range of pixel tiles; partial sums go to a workspace and are added in a fixed order (conv2d_wgrad_reduce_kernel):
// the same inputs give a bitwise-identical dW.
#include <algorithm>

#include "u3d_common.h"

namespace c2 {
constexpr int TY = 16, TX = 16;          // output tile
constexpr int HY = TY + 2, HX = TX + 2;  // halo
constexpr int CC = 16;                   // input channels per chunk
constexpr int CS = 20;                   // pixel stride in LDS (floats)
constexpr int RS = 384;                  // row stride in LDS (floats)
constexpr int BUF = HY * RS;             // 6912 floats per staging buffer
constexpr int NITEMS = HY * HX * (CC / 4);  // 1296 float4 items per chunk
constexpr int NIT = (NITEMS + 255) / 256;   // 6
constexpr int RED = 2 * BUF;                // [4 waves][NT <= 2][32][4] partial statistics
constexpr int LDS_FLOATS = RED + 4 * 2 * 32 * 4;  // 14848 floats = 59392 B
// weight gradient
constexpr int WCB = 32;                    // channels per block (both roles)
constexpr int WG_PS = WCB;                 // pixel stride of the staged tensors
constexpr int WG_G = 0;                    // [HY*HX][32] source halo
constexpr int WG_DZ = HY * HX * WG_PS;     // [TY*TX][32] dz tile
constexpr int WG_LDS_FLOATS = WG_DZ + TY * TX * WG_PS;  // 18560 floats = 74240 B
}  // namespace c2

static inline long long c2_cdiv(long long a, long long b) { return (a + b - 1) / b; }

static int c2_cu_count(int device) {
    static int cached[64] = {0};
    if (device >= 0 && device < 64 && cached[device] > 0) return cached[device];
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
    if (device >= 0 && device < 64) cached[device] = n;
    return n;
}

static bool c2_src_vec_ok(const u3d_src_t* s) {
    if (s->C0 % 4 != 0 || s->C1 % 4 != 0) return false;
    if (((uintptr_t)s->p0 & 15) != 0) return false;
    if (s->C1 > 0 && ((uintptr_t)s->p1 & 15) != 0) return false;
    return true;
}

// =================================================================================================
// weight packing: image [chunk][tap][g][ntile][lane][4] of B[k][n] with k = (chunk, tap, 8-channel group g, lane half h, element j)
//   mode 0 (forward): B[k = ci][n = co] = w[co][ci][tap]           mode 1 (data gradient): B[k = co][n = ci] = w[co][ci][8 - tap]
// lane l of an MFMA k-step j holds channel 16*chunk + 8g + 4*(l >> 5) + j of column (l & 31) — the A fragment of the same lane is the
// j-th float of its ds_read_b128 (channels 8g + 4h .. +3 of one pixel).  Padding (k or n beyond the layer) is zero.
static void c2_dims(int Cin, int Cout, int mode, int& K, int& Nn) {
    K = mode == 0 ? Cin : Cout;
    Nn = mode == 0 ? Cout : Cin;
}

extern "C" size_t u3d_packed_weight2d_floats(int Cin, int Cout, int mode) {
    if (Cin <= 0 || Cout <= 0 || (mode != 0 && mode != 1)) return 0;
    int K, Nn;
    c2_dims(Cin, Cout, mode, K, Nn);
    return (size_t)c2_cdiv(K, c2::CC) * 9 * 2 * c2_cdiv(Nn, 32) * 256;
}

__global__ void pack_weights2d_kernel(const float* __restrict__ w, int Cout, int Cin, int mode, int K, int Nn, int ntg,
                                      long long total, float* __restrict__ packed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 3);
        const int lane = (int)((i >> 2) & 63);
        long long r = i >> 8;
        const int nt = (int)(r % ntg);
        r /= ntg;
        const int g = (int)(r & 1);
        r >>= 1;
        const int tap = (int)(r % 9);
        const int chunk = (int)(r / 9);
        const int k = chunk * c2::CC + 8 * g + 4 * (lane >> 5) + j;
        const int nn = nt * 32 + (lane & 31);
        float v = 0.f;
        if (k < K && nn < Nn)
            v = mode == 0 ? w[((size_t)nn * Cin + k) * 9 + tap] : w[((size_t)k * Cin + nn) * 9 + (8 - tap)];
        packed[i] = v;
    }
}

extern "C" int u3d_pack_weights2d(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, float* packed) {
    U3D_ENTER(device);
    U3D_REQUIRE(w && packed && Cout > 0 && Cin > 0 && (mode == 0 || mode == 1), "u3d_pack_weights2d: bad argument");
    int K, Nn;
    c2_dims(Cin, Cout, mode, K, Nn);
    const long long total = (long long)u3d_packed_weight2d_floats(Cin, Cout, mode);
    long long blocks = c2_cdiv(total, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_weights2d_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin, mode, K, Nn,
                       (int)c2_cdiv(Nn, 32), total, packed);
    U3D_LAUNCH_CHECK();
    return 0;
}

// =================================================================================================
// forward / data gradient
struct Conv2dParams {
    u3d_src_t src;
    u3d_src_t gx;
    const float* wp;
    const float* residual;  // (N,H,W,Cout) added before the ReLU (conv2d_mfma_kernel<.., RES = true>), or null
    float* out;        // ksplit == 1: the output; else the workspace of partial sums [ksplit][N*H*W*Cout]
    double* out_stats;
    double* gstats;
    int N, H, W, Cout;
    int nchunks, ntg, ncb, ty, tx;
    int relu, has_gx, stat_reps;
    int ksplit, cps;
    long long part_stride;
};

// one value of the (virtual) gx tensor at pixel v0 / low-res pixel v1, channel c (gx has Cout channels in data-gradient use)
__device__ __forceinline__ float c2_gx_value(const u3d_src_t& g, int n, int y, int x, int H, int W, int c) {
    const int v0 = (n * H + y) * W + x;
    int v1 = 0;
    if (g.C1 > 0) v1 = (n * g.H1 + g.ymap[y]) * g.W1 + g.xmap[x];
    return u3d_load_elem(g, v0, v1, c);
}

// per-block statistics: lanes hold column sums s[nt][0..3] = (sum v, sum v^2, sum v, sum v * gx); combined over the lane halves,
// over the 4 waves in LDS (fixed order), then one f64 atomic per (sample, channel, quantity) and block into replica row block % reps
template <int NT>
__device__ __forceinline__ void c2_flush_stats(const Conv2dParams& p, float* red, float (&s)[NT][4], int n, int cb, int t) {
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
            if (p.has_gx) {
                double* o = p.gstats + (row + (size_t)n * p.Cout + co) * 2;
                u3d_atomic_add_f64(o, (double)a[2]);
                u3d_atomic_add_f64(o + 1, (double)a[3]);
            }
        }
    }
}

template <int NT, bool VEC, bool RES>
__global__ __launch_bounds__(256, 2) void conv2d_mfma_kernel(const Conv2dParams p) {
    using namespace c2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
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
    const int H = p.H, W = p.W;
    const int Ctot = p.src.C0 + p.src.C1;

    // ---- staging descriptors (constant across chunks)
    int ldsoff[NIT], v0s[NIT], v1s[NIT], cqs[NIT];
    bool oks[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int item = t + 256 * it;
        const bool in = item < NITEMS;
        const int pix = item >> 2, q = item & 3;
        const int hy = pix / HX, hx = pix - (pix / HX) * HX;
        const int gy = y0 - 1 + hy, gxx = x0 - 1 + hx;
        const bool ok = in && gy >= 0 && gy < H && gxx >= 0 && gxx < W;
        oks[it] = ok;
        ldsoff[it] = in ? hy * RS + hx * CS + 4 * q : -1;
        cqs[it] = 4 * q;
        v0s[it] = ok ? (n * H + gy) * W + gxx : 0;
        v1s[it] = (ok && p.src.C1 > 0) ? (n * p.src.H1 + p.src.ymap[gy]) * p.src.W1 + p.src.xmap[gxx] : 0;
    }
    f32x4 raw[NIT];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int cq = c * CC + cqs[it];
            raw[it] = (oks[it] && cq < Ctot) ? u3d_load_quad(p.src, v0s[it], v1s[it], cq, VEC) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_chunk = [&](int c, float* buf) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (ldsoff[it] < 0) continue;
            const int cq = c * CC + cqs[it];
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (oks[it] && cq < Ctot) {
                f32x4 a, b;
                u3d_load_affine(p.src.affine, n, Ctot, cq, VEC, a, b);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (cq + e < Ctot) ? raw[it][e] * a[e] + b[e] : 0.f;  // padding stays exactly 0
            }
            *reinterpret_cast<f32x4*>(buf + ldsoff[it]) = v;
        }
    };

    f32x16 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    // A-fragment base: lane (i = l & 31, h) of M-tile mt reads pixel (4w + 2mt + (i >> 4), i & 15), channels 8g + 4h .. +3
    const int i32 = l & 31;
    const int abase = (4 * w + (i32 >> 4)) * RS + (i32 & 15) * CS + 4 * h;
    // B image: [chunk][tap][g][ntg][lane][4]
    const f32x4* bimg = reinterpret_cast<const f32x4*>(p.wp);
    auto bidx = [&](int c, int step, int nt) -> long long {
        return ((long long)(c * 18 + step) * p.ntg + (cb * NT + nt)) * 64 + l;
    };

    load_chunk(ch0);
    store_chunk(ch0, lds);
    __syncthreads();
    for (int ci = 0; ci < nch; ++ci) {
        const int c = ch0 + ci;
        float* cur = lds + (ci & 1) * BUF;
        if (ci + 1 < nch) load_chunk(c + 1);  // in flight during the k-loop
        f32x4 bq[NT], bn[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            bq[nt] = (cb * NT + nt < p.ntg) ? bimg[bidx(c, 0, nt)] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int step = 0; step < 18; ++step) {
            const int tap = step >> 1, g = step & 1;
            const int dy = tap / 3, dx = tap - (tap / 3) * 3;
            if (step + 1 < 18) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    bn[nt] = (cb * NT + nt < p.ntg) ? bimg[bidx(c, step + 1, nt)] : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            f32x4 a[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                a[mt] = *reinterpret_cast<const f32x4*>(cur + abase + (2 * mt + dy) * RS + dx * CS + 8 * g);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][j], bq[nt][j], acc[mt][nt], 0, 0, 0);
            if (step + 1 < 18) {
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
                if (RES) v += p.residual[o];
                if (p.relu) v = fmaxf(v, 0.f);
                outp[o] = v;
                s[nt][0] += v;
                s[nt][1] += v * v;
                if (p.has_gx) {
                    s[nt][2] += v;
                    s[nt][3] += v * c2_gx_value(p.gx, n, y, x, H, W, co);
                }
            }
    }
    if (p.ksplit == 1 && (p.out_stats || p.has_gx)) c2_flush_stats<NT>(p, lds + RED, s, n, cb, t);
}

// split-K: out = [relu](sum over runs in run order [+ residual]), statistics as the main kernel.  Block = 64 pixels of one sample, threads walk the
// channels (coalesced), one f64 atomic per (block, channel, quantity).
__global__ __launch_bounds__(256) void conv2d_splitk_reduce_kernel(const float* __restrict__ part, long long part_stride, int ksplit,
                                                                   float* __restrict__ out, int N, int P, int Cout, int relu,
                                                                   double* out_stats, u3d_src_t gx, int has_gx, double* gstats,
                                                                   int H, int W, const float* __restrict__ residual) {
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
            if (has_gx) {
                g0 += v;
                g1 += (double)v * c2_gx_value(gx, n, pp / W, pp % W, H, W, co);
            }
        }
        if (out_stats) {
            u3d_atomic_add_f64(out_stats + ((size_t)n * Cout + co) * 2, s0);
            u3d_atomic_add_f64(out_stats + ((size_t)n * Cout + co) * 2 + 1, s1);
        }
        if (has_gx) {
            u3d_atomic_add_f64(gstats + ((size_t)n * Cout + co) * 2, g0);
            u3d_atomic_add_f64(gstats + ((size_t)n * Cout + co) * 2 + 1, g1);
        }
    }
}

struct C2Plan {
    int nt, ncb, ty, tx, ntg, nchunks, ksplit, cps;
};

static C2Plan c2_plan(int device, int N, int H, int W, int Cin, int Cout) {
    C2Plan pl;
    pl.ntg = (int)c2_cdiv(Cout, 32);
    pl.ty = (int)c2_cdiv(H, c2::TY);
    pl.tx = (int)c2_cdiv(W, c2::TX);
    pl.nchunks = (int)c2_cdiv(Cin, c2::CC);
    const long long tiles = (long long)N * pl.ty * pl.tx;
    const int slots = 2 * c2_cu_count(device);  // two blocks per CU (59 KB of LDS, 256 threads)
    pl.nt = (pl.ntg >= 2 && tiles * c2_cdiv(pl.ntg, 2) >= slots) ? 2 : 1;
    pl.ncb = (int)c2_cdiv(pl.ntg, pl.nt);
    const long long blocks = tiles * pl.ncb;
    pl.ksplit = 1;
    pl.cps = pl.nchunks;
    if (blocks < slots / 2 && pl.nchunks >= 2) {  // bottom of the U: fewer blocks than CUs -> split the channel reduction
        int ks = (int)std::min<long long>(pl.nchunks, c2_cdiv(slots, blocks));
        pl.cps = (int)c2_cdiv(pl.nchunks, ks);
        pl.ksplit = (int)c2_cdiv(pl.nchunks, pl.cps);
    }
    return pl;
}

extern "C" long long u3d_conv2d_workspace_floats(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const C2Plan pl = c2_plan(dev, N, H, W, Cin, Cout);
    return pl.ksplit > 1 ? (long long)pl.ksplit * N * H * W * Cout : 0;
}

static int conv2d_impl(int device, u3d_stream_t stream, const u3d_src_t* src, const float* packed_w, float* out, int N, int H, int W,
                       int Cout, int relu, double* out_stats, const u3d_src_t* gx, double* gstats, const float* residual,
                       float* workspace, long long workspace_floats, int stat_reps) {
    U3D_ENTER(device);
    U3D_REQUIRE(src && src->p0 && packed_w && out && N > 0 && H > 0 && W > 0 && Cout > 0 && src->C0 >= 0 && src->C1 >= 0 &&
                    src->C0 + src->C1 > 0 && stat_reps >= 1 && (long long)N * H * W < (1LL << 31),
                "u3d_conv2d_ex_reps: bad argument");
    U3D_REQUIRE(src->C1 == 0 || (src->p1 && src->ymap && src->xmap && src->D1 == 1 && src->H1 > 0 && src->W1 > 0),
                "u3d_conv2d_ex_reps: virtual source needs p1, ymap, xmap and D1 == 1");
    U3D_REQUIRE(!gx || (gstats && gx->p0 && gx->C0 + gx->C1 == Cout), "u3d_conv2d_ex_reps: gx needs gstats and Cout channels");
    const int Cin = src->C0 + src->C1;
    const C2Plan pl = c2_plan(device, N, H, W, Cin, Cout);
    const long long need = pl.ksplit > 1 ? (long long)pl.ksplit * N * H * W * Cout : 0;
    const bool split = need > 0 && workspace != nullptr;
    U3D_REQUIRE(!split || workspace_floats >= need, "u3d_conv2d_ex_reps: workspace too small (%lld < %lld floats)", workspace_floats, need);
    Conv2dParams p = {};
    p.src = *src;
    if (gx) p.gx = *gx;
    p.wp = packed_w;
    p.residual = residual;
    p.out = split ? workspace : out;
    p.out_stats = out_stats;
    p.gstats = gstats;
    p.N = N, p.H = H, p.W = W, p.Cout = Cout;
    p.nchunks = pl.nchunks, p.ntg = pl.ntg, p.ncb = pl.ncb, p.ty = pl.ty, p.tx = pl.tx;
    p.relu = relu ? 1 : 0;
    p.has_gx = gx ? 1 : 0;
    p.stat_reps = stat_reps;
    p.ksplit = split ? pl.ksplit : 1;
    p.cps = split ? pl.cps : pl.nchunks;
    p.part_stride = (long long)N * H * W * Cout;
    const bool vec = c2_src_vec_ok(src);
    const long long blocks = (long long)N * pl.ty * pl.tx * pl.ncb * p.ksplit;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_conv2d_ex_reps: grid too large");
    const size_t lds = c2::LDS_FLOATS * sizeof(float);
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, p); };
    if (residual) {  // (a template flag: the kernel without a residual operand is the one u3d_conv2d_ex_reps always ran)
        if (pl.nt == 2)
            vec ? go(conv2d_mfma_kernel<2, true, true>) : go(conv2d_mfma_kernel<2, false, true>);
        else
            vec ? go(conv2d_mfma_kernel<1, true, true>) : go(conv2d_mfma_kernel<1, false, true>);
    } else if (pl.nt == 2) {
        vec ? go(conv2d_mfma_kernel<2, true, false>) : go(conv2d_mfma_kernel<2, false, false>);
    } else {
        vec ? go(conv2d_mfma_kernel<1, true, false>) : go(conv2d_mfma_kernel<1, false, false>);
    }
    U3D_LAUNCH_CHECK();
    if (split) {
        const int P = H * W;
        u3d_src_t g = {};
        if (gx) g = *gx;
        hipLaunchKernelGGL(conv2d_splitk_reduce_kernel, dim3((unsigned)c2_cdiv(P, 64), N), dim3(256), 0, (hipStream_t)stream, workspace,
                           p.part_stride, p.ksplit, out, N, P, Cout, p.relu, out_stats, g, p.has_gx, gstats, H, W, residual);
        U3D_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int u3d_conv2d_ex_reps(int device, u3d_stream_t stream, const u3d_src_t* src, const float* packed_w, float* out, int N,
                                  int H, int W, int Cout, int relu, double* out_stats, const u3d_src_t* gx, double* gstats,
                                  float* workspace, long long workspace_floats, int stat_reps) {
    return conv2d_impl(device, stream, src, packed_w, out, N, H, W, Cout, relu, out_stats, gx, gstats, nullptr, workspace,
                       workspace_floats, stat_reps);
}

// the tail of ResNetBlock (buildingblocks.py:277-288) in the epilogue: out = [relu](conv + residual); statistics of the written values
extern "C" int u3d_conv2d_res_reps(int device, u3d_stream_t stream, const u3d_src_t* src, const float* packed_w, float* out, int N,
                                   int H, int W, int Cout, int relu, double* out_stats, const u3d_src_t* gx, double* gstats,
                                   float* workspace, long long workspace_floats, int stat_reps, const float* residual) {
    U3D_REQUIRE(residual && !gx, "u3d_conv2d_res_reps: needs a residual, and a residual excludes gx");
    return conv2d_impl(device, stream, src, packed_w, out, N, H, W, Cout, relu, out_stats, gx, gstats, residual, workspace,
                       workspace_floats, stat_reps);
}

// =================================================================================================
// weight gradient: dw[co][ci][tap] = sum_{n,y,x} dz[n,y,x,co] * g[n, y + dy - 1, x + dx - 1, ci], g = affine(src), zero padded.
// MFMA: M = 32 output channels (A = dz), N = 32 input channels (B = g), K = pixels two at a time; the same A fragment feeds 9 taps.
struct Wgrad2dParams {
    u3d_src_t src;
    const float* dz;
    float* dst;  // nsplit == 1: dw; else workspace [nsplit][Cout][Cin][9]
    int N, H, W, Cin, Cout;
    int ty, tx, ncob, ncib, ntiles, tps;
    int vec_dz;
};

template <bool VEC>
__global__ __launch_bounds__(256, 2) void conv2d_wgrad_kernel(const Wgrad2dParams p) {
    using namespace c2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int t = threadIdx.x, l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int b = blockIdx.x;
    const int cib = b % p.ncib;
    b /= p.ncib;
    const int cob = b % p.ncob;
    const int split = b / p.ncob;
    const int ci0 = cib * WCB, co0 = cob * WCB;
    const int tile0 = split * p.tps, tile1 = min(p.ntiles, tile0 + p.tps);
    const int H = p.H, W = p.W, Cin = p.Cin;
    float* const gl = lds + WG_G;
    float* const dzl = lds + WG_DZ;

    f32x16 acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    for (int tile = tile0; tile < tile1; ++tile) {
        int tt = tile;
        const int txi = tt % p.tx;
        tt /= p.tx;
        const int tyi = tt % p.ty;
        const int n = tt / p.ty;
        const int y0 = tyi * TY, x0 = txi * TX;
        // stage g (18 x 18 halo, 32 channels from ci0, affine, zero padding) and dz (16 x 16, 32 channels from co0)
        for (int item = t; item < HY * HX * (WCB / 4); item += 256) {
            const int pix = item >> 3, q = item & 7;
            const int hy = pix / HX, hx = pix - (pix / HX) * HX;
            const int gy = y0 - 1 + hy, gxx = x0 - 1 + hx;
            const int cq = ci0 + 4 * q;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (gy >= 0 && gy < H && gxx >= 0 && gxx < W && cq < Cin) {
                const int v0 = (n * H + gy) * W + gxx;
                const int v1 = p.src.C1 > 0 ? (n * p.src.H1 + p.src.ymap[gy]) * p.src.W1 + p.src.xmap[gxx] : 0;
                const f32x4 r = u3d_load_quad(p.src, v0, v1, cq, VEC);
                f32x4 a, bb;
                u3d_load_affine(p.src.affine, n, Cin, cq, VEC, a, bb);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (cq + e < Cin) ? r[e] * a[e] + bb[e] : 0.f;
            }
            *reinterpret_cast<f32x4*>(gl + pix * WG_PS + 4 * q) = v;
        }
        for (int item = t; item < TY * TX * (WCB / 4); item += 256) {
            const int pix = item >> 3, q = item & 7;
            const int y = y0 + (pix >> 4), x = x0 + (pix & 15);
            const int cq = co0 + 4 * q;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (y < H && x < W) {
                const float* src = p.dz + ((size_t)(n * H + y) * W + x) * p.Cout;
                if (p.vec_dz && cq + 3 < p.Cout) {
                    v = *reinterpret_cast<const f32x4*>(src + cq);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (cq + e < p.Cout) v[e] = src[cq + e];
                }
            }
            *reinterpret_cast<f32x4*>(dzl + pix * WG_PS + 4 * q) = v;
        }
        __syncthreads();
        // wave w: pixels 64w .. 64w + 63 of the tile (rows 4w .. 4w + 3), two per k-step
#pragma unroll 2
        for (int kk = 0; kk < 32; ++kk) {
            const int pix = 64 * w + 2 * kk + h;
            const int py = pix >> 4, px = pix & 15;
            const float a = dzl[pix * WG_PS + i32];
            const float* gp = gl + (py * HX + px) * WG_PS + i32;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx)
                    acc[dy * 3 + dx] =
                        __builtin_amdgcn_mfma_f32_32x32x2f32(a, gp[(dy * HX + dx) * WG_PS], acc[dy * 3 + dx], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- add the 4 waves' partial sums in a fixed order, one tap at a time, through LDS; write [co][ci][tap]
    float* red = lds;  // [4][32][32]
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
            if (co < p.Cout && ci < Cin) p.dst[(size_t)split * p.Cout * Cin * 9 + ((size_t)co * Cin + ci) * 9 + tap] = v;
        }
        __syncthreads();
    }
}

// dw[i] = sum over splits in split order (bitwise-reproducible)
__global__ void conv2d_wgrad_reduce_kernel(const float* __restrict__ ws, int nsplit, long long total, float* __restrict__ dw) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) v += ws[(size_t)s * total + i];
        dw[i] = v;
    }
}

struct W2Plan {
    int ty, tx, ncob, ncib, ntiles, tps, nsplit;
};

static W2Plan w2_plan(int device, int N, int H, int W, int Cin, int Cout) {
    W2Plan pl;
    pl.ty = (int)c2_cdiv(H, c2::TY);
    pl.tx = (int)c2_cdiv(W, c2::TX);
    pl.ncob = (int)c2_cdiv(Cout, c2::WCB);
    pl.ncib = (int)c2_cdiv(Cin, c2::WCB);
    pl.ntiles = N * pl.ty * pl.tx;
    const long long cells = (long long)pl.ncob * pl.ncib;
    const long long target = 4LL * c2_cu_count(device);  // ~4 blocks per CU over the launch
    long long ns = std::max<long long>(1, std::min<long long>(pl.ntiles, c2_cdiv(target, cells)));
    pl.tps = (int)c2_cdiv(pl.ntiles, ns);
    pl.nsplit = (int)c2_cdiv(pl.ntiles, pl.tps);
    return pl;
}

extern "C" size_t u3d_wgrad2d_workspace_floats(int N, int H, int W, int Cin, int Cout) {
    if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const W2Plan pl = w2_plan(dev, N, H, W, Cin, Cout);
    return pl.nsplit > 1 ? (size_t)pl.nsplit * Cout * Cin * 9 : 0;
}

extern "C" int u3d_conv2d_wgrad(int device, u3d_stream_t stream, const u3d_src_t* src, const float* dz, float* dw, int N, int H, int W,
                                int Cout, float* workspace, size_t workspace_floats) {
    U3D_ENTER(device);
    U3D_REQUIRE(src && src->p0 && dz && dw && N > 0 && H > 0 && W > 0 && Cout > 0 && src->C0 >= 0 && src->C1 >= 0 &&
                    src->C0 + src->C1 > 0 && (long long)N * H * W < (1LL << 31),
                "u3d_conv2d_wgrad: bad argument");
    U3D_REQUIRE(src->C1 == 0 || (src->p1 && src->ymap && src->xmap && src->D1 == 1 && src->H1 > 0 && src->W1 > 0),
                "u3d_conv2d_wgrad: virtual source needs p1, ymap, xmap and D1 == 1");
    const int Cin = src->C0 + src->C1;
    const W2Plan pl = w2_plan(device, N, H, W, Cin, Cout);
    const size_t need = pl.nsplit > 1 ? (size_t)pl.nsplit * Cout * Cin * 9 : 0;
    U3D_REQUIRE(need == 0 || (workspace && workspace_floats >= need), "u3d_conv2d_wgrad: workspace too small (%zu < %zu floats)",
                workspace_floats, need);
    Wgrad2dParams p = {};
    p.src = *src;
    p.dz = dz;
    p.dst = need ? workspace : dw;
    p.N = N, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout;
    p.ty = pl.ty, p.tx = pl.tx, p.ncob = pl.ncob, p.ncib = pl.ncib, p.ntiles = pl.ntiles, p.tps = pl.tps;
    p.vec_dz = (Cout % 4 == 0 && ((uintptr_t)dz & 15) == 0) ? 1 : 0;
    const size_t lds = c2::WG_LDS_FLOATS * sizeof(float);
    static bool attr_set[2] = {false, false};
    if (!attr_set[0]) {
        U3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv2d_wgrad_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
        U3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv2d_wgrad_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
        attr_set[0] = true;
    }
    const long long blocks = (long long)pl.nsplit * pl.ncob * pl.ncib;
    if (c2_src_vec_ok(src))
        hipLaunchKernelGGL(conv2d_wgrad_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(conv2d_wgrad_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    if (need) {
        const long long total = (long long)Cout * Cin * 9;
        long long rb = c2_cdiv(total, 256);
        if (rb > 4096) rb = 4096;
        hipLaunchKernelGGL(conv2d_wgrad_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace, pl.nsplit, total,
                           dw);
        U3D_LAUNCH_CHECK();
    }
    return 0;
}

// =================================================================================================
// MaxPool2d(2): stride 2, floor.  argmax byte k = 2 * dy + dx of the first maximum in (y, x) scan order (ATen); NaN propagates.
__global__ void maxpool2d_fwd_kernel(const float* __restrict__ x, int N, int H, int W, int C, float* __restrict__ out,
                                     uint8_t* __restrict__ argmax) {
    const int H2 = H >> 1, W2 = W >> 1;
    const long long total = (long long)N * H2 * W2 * C;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % C);
        long long v = idx / C;
        const int xo = (int)(v % W2);
        v /= W2;
        const int yo = (int)(v % H2);
        const int n = (int)(v / H2);
        float best = -INFINITY;
        int bi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = 2 * yo + (k >> 1), xx = 2 * xo + (k & 1);
            const float val = x[((size_t)(n * H + y) * W + xx) * C + c];
            if (val > best || val != val) {
                best = val;
                bi = k;
            }
        }
        out[idx] = best;
        argmax[idx] = (uint8_t)bi;
    }
}

static int c2_grid(long long total) {
    long long b = c2_cdiv(total, 256);
    if (b < 1) b = 1;
    return (int)(b > 16384 ? 16384 : b);
}

extern "C" int u3d_maxpool2d_fwd(int device, u3d_stream_t stream, const float* x, int N, int H, int W, int C, float* out, uint8_t* argmax,
                                 double* out_stats) {
    U3D_ENTER(device);
    U3D_REQUIRE(x && out && argmax && N > 0 && H >= 2 && W >= 2 && C > 0, "u3d_maxpool2d_fwd: bad argument");
    const long long total = (long long)N * (H / 2) * (W / 2) * C;
    hipLaunchKernelGGL(maxpool2d_fwd_kernel, dim3(c2_grid(total)), dim3(256), 0, (hipStream_t)stream, x, N, H, W, C, out, argmax);
    U3D_LAUNCH_CHECK();
    if (out_stats) {
        u3d_src_t s = {};
        s.p0 = out;
        s.C0 = C;
        return u3d_chan_stats(device, stream, &s, N, 1, H / 2, W / 2, out_stats);
    }
    return 0;
}

// dz_e = (skip + scatter(dpool)) * (e > 0) over 2x2 windows covering ceil dims; dpool = p*dg + q*pooled + r (coef optional); skip absent,
// a plain tensor (sdg, Csdg channels per pixel) or the GroupNorm backward ps*sdg + qs*e + rs of the decoder's first conv (scoef).
// A unit is VW (4 or 1) channels.  The 2-D twin of maxpool2_bwd_merge_kernel (csrc/u3d_ops.hip).
template <int VW>
__global__ void maxpool2d_bwd_merge_kernel(const float* __restrict__ dg, const float* __restrict__ pooled, const uint8_t* __restrict__ argmax,
                                           const float* __restrict__ coef, const float* __restrict__ sdg, int Csdg,
                                           const float* __restrict__ scoef, int Cstot, const float* __restrict__ e, int N, int H, int W,
                                           int C, int relu_mask, float* __restrict__ out) {
    const int H2 = H >> 1, W2 = W >> 1;
    const int Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    const int Q = C / VW;
    const long long total = (long long)N * Hc * Wc * Q;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % Q) * VW;
        long long v = idx / Q;
        const int xo = (int)(v % Wc);
        v /= Wc;
        const int yo = (int)(v % Hc);
        const int n = (int)(v / Hc);
        const bool pv = yo < H2 && xo < W2;
        float dp[VW], ps[VW], qs[VW], rs[VW];
        int am[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            dp[k] = 0.f;
            am[k] = -1;
            ps[k] = 1.f, qs[k] = 0.f, rs[k] = 0.f;
            if (scoef) {
                ps[k] = scoef[((size_t)n * 3 + 0) * Cstot + c + k];
                qs[k] = scoef[((size_t)n * 3 + 1) * Cstot + c + k];
                rs[k] = scoef[((size_t)n * 3 + 2) * Cstot + c + k];
            }
        }
        if (pv) {
            const size_t pi = ((size_t)(n * H2 + yo) * W2 + xo) * C + c;
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                dp[k] = dg[pi + k];
                if (coef)
                    dp[k] = coef[((size_t)n * 3 + 0) * C + c + k] * dp[k] + coef[((size_t)n * 3 + 1) * C + c + k] * pooled[pi + k] +
                            coef[((size_t)n * 3 + 2) * C + c + k];
                am[k] = argmax[pi + k];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int y = 2 * yo + (j >> 1), xx = 2 * xo + (j & 1);
            if (y < H && xx < W) {
                const size_t vi = (size_t)(n * H + y) * W + xx;
                const size_t ei = vi * C + c;
                float ev[VW], sv[VW], o[VW];
                if (VW == 4) {
                    const f32x4 tq = (relu_mask || scoef) ? u3d_ldq(e + ei) : f32x4{1.f, 1.f, 1.f, 1.f};
                    const f32x4 u = sdg ? u3d_ldq(sdg + vi * Csdg + c) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < VW; ++k) ev[k] = tq[k], sv[k] = u[k];
                } else {
                    ev[0] = (relu_mask || scoef) ? e[ei] : 1.f;
                    sv[0] = sdg ? sdg[vi * Csdg + c] : 0.f;
                }
#pragma unroll
                for (int k = 0; k < VW; ++k) {
                    float g = sdg ? (scoef ? ps[k] * sv[k] + qs[k] * ev[k] + rs[k] : sv[k]) : 0.f;
                    if (j == am[k]) g += dp[k];
                    if (relu_mask && !(ev[k] > 0.f)) g = 0.f;
                    o[k] = g;
                }
                if (VW == 4)
                    u3d_stq(out + ei, f32x4{o[0], o[1], o[2], o[3]});
                else
                    out[ei] = o[0];
            }
        }
    }
}

static int maxpool2d_bwd_impl(int device, u3d_stream_t stream, const float* dg, const float* pooled, const uint8_t* argmax,
                              const float* coef, const float* sdg, int Csdg, const float* scoef, int Cstot, const float* e, int N, int H,
                              int W, int C, int relu_mask, float* out) {
    U3D_ENTER(device);
    U3D_REQUIRE(dg && argmax && out && (coef == nullptr || pooled) && (!(relu_mask || scoef) || e) && N > 0 && H >= 2 && W >= 2 && C > 0 &&
                    (!sdg || Csdg >= C) && (!scoef || (sdg && Cstot >= C)),
                "u3d_maxpool2d_bwd_merge: bad argument");
    const bool vec = C % 4 == 0 && (!sdg || Csdg % 4 == 0) && (((uintptr_t)e | (uintptr_t)sdg | (uintptr_t)out) & 15) == 0;
    const long long total = (long long)N * ((H + 1) / 2) * ((W + 1) / 2) * (vec ? C / 4 : C);
    if (vec)
        hipLaunchKernelGGL(maxpool2d_bwd_merge_kernel<4>, dim3(c2_grid(total)), dim3(256), 0, (hipStream_t)stream, dg, pooled, argmax, coef,
                           sdg, Csdg, scoef, Cstot, e, N, H, W, C, relu_mask, out);
    else
        hipLaunchKernelGGL(maxpool2d_bwd_merge_kernel<1>, dim3(c2_grid(total)), dim3(256), 0, (hipStream_t)stream, dg, pooled, argmax, coef,
                           sdg, Csdg, scoef, Cstot, e, N, H, W, C, relu_mask, out);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_maxpool2d_bwd_merge(int device, u3d_stream_t stream, const float* dg, const float* pooled, const uint8_t* argmax,
                                       const float* coef, const float* skip_grad, const float* e, int N, int H, int W, int C, int relu_mask,
                                       float* out) {
    return maxpool2d_bwd_impl(device, stream, dg, pooled, argmax, coef, skip_grad, C, nullptr, 0, e, N, H, W, C, relu_mask, out);
}

extern "C" int u3d_maxpool2d_bwd_merge_gn(int device, u3d_stream_t stream, const float* dg, const float* pooled, const uint8_t* argmax,
                                          const float* coef, const float* skip_dg, int Cdg, const float* skip_coef, int Ctot, const float* e,
                                          int N, int H, int W, int C, int relu_mask, float* out) {
    if (!skip_dg || !skip_coef) return u3d_set_err(U3D_EINVAL, "u3d_maxpool2d_bwd_merge_gn: skip_dg / skip_coef are NULL");
    return maxpool2d_bwd_impl(device, stream, dg, pooled, argmax, coef, skip_dg, Cdg, skip_coef, Ctot, e, N, H, W, C, relu_mask, out);
}
