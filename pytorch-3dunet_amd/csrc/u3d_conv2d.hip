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
//
// Both kernels have a BOX instantiation (u3d_conv2d_box, u3d_conv2d_wgrad_box): tiles enumerated from the origin of a box of the image,
// only pixels inside it written (forward / data gradient) or contracted over (weight gradient) — the 2-pixel slab of a decoder level that
// upsamples n -> 2n + 1 under `native_2d_subpixel_plus`, next to the windowed kernels of csrc/u3d_subpix2d.hip.  The other instantiations
// are the code they were.
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

// (w row = `ld` input channels, the packed ones start at channel `off`: a whole weight has ld = Cin, off = 0)
__global__ void pack_weights2d_kernel(const float* __restrict__ w, int Cout, int Cin, int mode, int K, int Nn, int ntg,
                                      long long total, float* __restrict__ packed, int ld, int off) {
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
            v = mode == 0 ? w[((size_t)nn * ld + off + k) * 9 + tap] : w[((size_t)k * ld + off + nn) * 9 + (8 - tap)];
        packed[i] = v;
    }
}

static int pack_weights2d_impl(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, int ld, int off,
                               float* packed) {
    U3D_ENTER(device);
    U3D_REQUIRE(w && packed && Cout > 0 && Cin > 0 && (mode == 0 || mode == 1) && off >= 0 && off + Cin <= ld,
                "u3d_pack_weights2d: bad argument");
    int K, Nn;
    c2_dims(Cin, Cout, mode, K, Nn);
    const long long total = (long long)u3d_packed_weight2d_floats(Cin, Cout, mode);
    long long blocks = c2_cdiv(total, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_weights2d_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin, mode, K, Nn,
                       (int)c2_cdiv(Nn, 32), total, packed, ld, off);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_pack_weights2d(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, float* packed) {
    return pack_weights2d_impl(device, stream, w, Cout, Cin, mode, Cin, 0, packed);
}

// the same image of the input channels [c_off, c_off + Cin) of a (Cout, cin_stride, 3, 3) weight (the skip half of a sub-pixel layer)
extern "C" int u3d_pack_weights2d_slice(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, int cin_stride,
                                        int c_off, float* packed) {
    return pack_weights2d_impl(device, stream, w, Cout, Cin, mode, cin_stride, c_off, packed);
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
    // conv2d_mfma_kernel<.., BOX = true> (u3d_conv2d_box): tiles are enumerated from the origin of the OUTPUT BOX [b*0, b*1) and only pixels
    // inside it are written, to out[(y - ooy, x - oox)] of an (N, oH, oW, Cout) tensor; a source pixel counts only if
    // my && y < my || mx && x < mx (my = mx = 0: every pixel counts)
    int by0, bx0, by1, bx1, my, mx, oH, oW, ooy, oox;
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

template <int NT, bool VEC, bool RES, bool BOX = false>
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
    const int y0 = tyi * TY + (BOX ? p.by0 : 0), x0 = txi * TX + (BOX ? p.bx0 : 0);
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
        bool ok = in && gy >= 0 && gy < H && gxx >= 0 && gxx < W;
        if (BOX && (p.my | p.mx) != 0) ok = ok && ((p.my != 0 && gy < p.my) || (p.mx != 0 && gxx < p.mx));
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
                if (BOX ? (y >= p.by1 || x >= p.bx1) : (y >= H || x >= W)) continue;
                float v = acc[mt][nt][r];
                const size_t o = BOX ? ((size_t)(n * p.oH + y - p.ooy) * p.oW + x - p.oox) * p.Cout + co
                                     : ((size_t)(n * H + y) * W + x) * p.Cout + co;
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

// The same convolution for the output pixels inside out_box = {y0, x0, y1, x1} only — the near-boundary slab of a decoder level that
// upsamples n -> 2n + 1 (`native_2d_subpixel_plus`; the 2-D twin of u3d_conv3d_box).  src->C0 may be 0 (only the upsampled half; p0 must
// still be readable).  in_mask = {my, mx} or NULL: a source pixel counts only if my && y < my || mx && x < mx (the slab's data gradient:
// dz outside the slab is zero).  out_win = {Ho, Wo, oy, ox} or NULL: pixel (y, x) goes to out[(y - oy, x - ox)] of an (N, Ho, Wo, Cout)
// tensor — a scratch the size of the box instead of the image (NULL: out is (N, H, W, Cout)).  Plain sums: no ReLU, no statistics, no
// split-K; pixels outside the box are not touched.  A 2-pixel slab in 16 x 16 tiles wastes 7/8 of its MFMAs; it is well under 1 % of the level.
extern "C" int u3d_conv2d_box(int device, u3d_stream_t stream, const u3d_src_t* src, const float* packed_w, float* out, int N, int H,
                              int W, int Cout, const int* out_box, const int* in_mask, const int* out_win) {
    U3D_ENTER(device);
    U3D_REQUIRE(src && src->p0 && packed_w && out && out_box && N > 0 && H > 0 && W > 0 && Cout > 0 && src->C0 >= 0 && src->C1 >= 0 &&
                    src->C0 + src->C1 > 0 && (long long)N * H * W < (1LL << 31),
                "u3d_conv2d_box: bad argument");
    U3D_REQUIRE(src->C1 == 0 || (src->p1 && src->ymap && src->xmap && src->D1 == 1 && src->H1 > 0 && src->W1 > 0),
                "u3d_conv2d_box: virtual source needs p1, ymap, xmap and D1 == 1");
    Conv2dParams p = {};
    p.by0 = out_box[0], p.bx0 = out_box[1], p.by1 = out_box[2], p.bx1 = out_box[3];
    U3D_REQUIRE(0 <= p.by0 && p.by0 < p.by1 && p.by1 <= H && 0 <= p.bx0 && p.bx0 < p.bx1 && p.bx1 <= W,
                "u3d_conv2d_box: output box outside the image or empty");
    if (in_mask) p.my = in_mask[0], p.mx = in_mask[1];
    U3D_REQUIRE(p.my >= 0 && p.mx >= 0, "u3d_conv2d_box: negative mask");
    p.oH = H, p.oW = W, p.ooy = p.oox = 0;
    if (out_win) {
        p.oH = out_win[0], p.oW = out_win[1], p.ooy = out_win[2], p.oox = out_win[3];
        U3D_REQUIRE(p.ooy >= 0 && p.oox >= 0 && p.ooy <= p.by0 && p.oox <= p.bx0 && p.by1 - p.ooy <= p.oH && p.bx1 - p.oox <= p.oW &&
                        (long long)N * p.oH * p.oW < (1LL << 31),
                    "u3d_conv2d_box: the output box does not fit the output window");
    }
    const int Cin = src->C0 + src->C1;
    p.src = *src;
    p.wp = packed_w;
    p.out = out;
    p.N = N, p.H = H, p.W = W, p.Cout = Cout;
    p.nchunks = (int)c2_cdiv(Cin, c2::CC), p.ntg = (int)c2_cdiv(Cout, 32);
    p.ty = (int)c2_cdiv(p.by1 - p.by0, c2::TY), p.tx = (int)c2_cdiv(p.bx1 - p.bx0, c2::TX);
    const int nt = p.ntg >= 2 ? 2 : 1;
    p.ncb = (int)c2_cdiv(p.ntg, nt);
    p.stat_reps = 1;
    p.ksplit = 1, p.cps = p.nchunks;
    const bool vec = c2_src_vec_ok(src);
    const long long blocks = (long long)N * p.ty * p.tx * p.ncb;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_conv2d_box: grid too large");
    const size_t lds = c2::LDS_FLOATS * sizeof(float);
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, p); };
    if (nt == 2)
        vec ? go(conv2d_mfma_kernel<2, true, false, true>) : go(conv2d_mfma_kernel<2, false, false, true>);
    else
        vec ? go(conv2d_mfma_kernel<1, true, false, true>) : go(conv2d_mfma_kernel<1, false, false, true>);
    U3D_LAUNCH_CHECK();
    return 0;
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
    int dst_cin;  // input channels per row of dst: Cin, or the parent's count when dw is a channel slice written directly
    int by0, bx0, by1, bx1;  // conv2d_wgrad_kernel<.., BOX = true> (u3d_conv2d_wgrad_box): the dz pixels that take part; tiles from its origin
};

template <bool VEC, bool BOX = false>
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
        const int y0 = tyi * TY + (BOX ? p.by0 : 0), x0 = txi * TX + (BOX ? p.bx0 : 0);
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
            if (BOX ? (y < p.by1 && x < p.bx1) : (y < H && x < W)) {
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
            if (co < p.Cout && ci < Cin) p.dst[(size_t)split * p.Cout * Cin * 9 + ((size_t)co * p.dst_cin + ci) * 9 + tap] = v;
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

// ... into a channel slice: row (output channel) i / row of `row` floats lands at dw + (i / row) * dw_row
__global__ void conv2d_wgrad_reduce_strided_kernel(const float* __restrict__ ws, int nsplit, long long total, int row, int dw_row,
                                                   float* __restrict__ dw) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) v += ws[(size_t)s * total + i];
        dw[(i / row) * dw_row + (i % row)] = v;
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

static int conv2d_wgrad_impl(int device, u3d_stream_t stream, const u3d_src_t* src, const float* dz, float* dw, int dw_cin_stride, int N,
                             int H, int W, int Cout, float* workspace, size_t workspace_floats, const int* box = nullptr) {
    U3D_ENTER(device);
    U3D_REQUIRE(src && src->p0 && dz && dw && N > 0 && H > 0 && W > 0 && Cout > 0 && src->C0 >= 0 && src->C1 >= 0 &&
                    src->C0 + src->C1 > 0 && (long long)N * H * W < (1LL << 31),
                "u3d_conv2d_wgrad: bad argument");
    U3D_REQUIRE(src->C1 == 0 || (src->p1 && src->ymap && src->xmap && src->D1 == 1 && src->H1 > 0 && src->W1 > 0),
                "u3d_conv2d_wgrad: virtual source needs p1, ymap, xmap and D1 == 1");
    const int Cin = src->C0 + src->C1;
    if (dw_cin_stride == 0) dw_cin_stride = Cin;
    U3D_REQUIRE(dw_cin_stride >= Cin, "u3d_conv2d_wgrad_strided: dw_cin_stride below the source's channel count");
    if (box)
        U3D_REQUIRE(0 <= box[0] && box[0] < box[2] && box[2] <= H && 0 <= box[1] && box[1] < box[3] && box[3] <= W,
                    "u3d_conv2d_wgrad_box: box outside the image or empty");
    // (a box: the plan of an image of the box's size — workspace: u3d_wgrad2d_workspace_floats of the box dims)
    const W2Plan pl = box ? w2_plan(device, N, box[2] - box[0], box[3] - box[1], Cin, Cout) : w2_plan(device, N, H, W, Cin, Cout);
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
    p.dst_cin = need ? Cin : dw_cin_stride;
    if (box) p.by0 = box[0], p.bx0 = box[1], p.by1 = box[2], p.bx1 = box[3];
    const size_t lds = c2::WG_LDS_FLOATS * sizeof(float);
    static bool attr_set[2] = {false, false};
    if (!attr_set[0]) {
        U3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv2d_wgrad_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
        U3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv2d_wgrad_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
        attr_set[0] = true;
    }
    if (box && !attr_set[1]) {
        U3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv2d_wgrad_kernel<false, true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        U3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv2d_wgrad_kernel<true, true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set[1] = true;
    }
    const long long blocks = (long long)pl.nsplit * pl.ncob * pl.ncib;
    if (box) {
        if (c2_src_vec_ok(src))
            hipLaunchKernelGGL((conv2d_wgrad_kernel<true, true>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, p);
        else
            hipLaunchKernelGGL((conv2d_wgrad_kernel<false, true>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, p);
    } else if (c2_src_vec_ok(src))
        hipLaunchKernelGGL(conv2d_wgrad_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(conv2d_wgrad_kernel<false>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    if (need) {
        const long long total = (long long)Cout * Cin * 9;
        long long rb = c2_cdiv(total, 256);
        if (rb > 4096) rb = 4096;
        if (dw_cin_stride == Cin)
            hipLaunchKernelGGL(conv2d_wgrad_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace, pl.nsplit,
                               total, dw);
        else
            hipLaunchKernelGGL(conv2d_wgrad_reduce_strided_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace,
                               pl.nsplit, total, Cin * 9, dw_cin_stride * 9, dw);
        U3D_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int u3d_conv2d_wgrad(int device, u3d_stream_t stream, const u3d_src_t* src, const float* dz, float* dw, int N, int H, int W,
                                int Cout, float* workspace, size_t workspace_floats) {
    return conv2d_wgrad_impl(device, stream, src, dz, dw, 0, N, H, W, Cout, workspace, workspace_floats);
}

// the same, writing the gradient of a CHANNEL SLICE of a wider weight: dw points at the slice's first input channel inside the
// (Cout, dw_cin_stride, 3, 3) gradient; src holds only the slice's channels (the skip half of a sub-pixel layer)
extern "C" int u3d_conv2d_wgrad_strided(int device, u3d_stream_t stream, const u3d_src_t* src, const float* dz, float* dw,
                                        int dw_cin_stride, int N, int H, int W, int Cout, float* workspace, size_t workspace_floats) {
    return conv2d_wgrad_impl(device, stream, src, dz, dw, dw_cin_stride, N, H, W, Cout, workspace, workspace_floats);
}

// the same over the dz pixels inside box = {y0, x0, y1, x1} only (the slab of a level that upsamples n -> 2n + 1; the 2-D twin of
// u3d_conv3d_wgrad_box): dw (Cout, Cin, 3, 3) is written; workspace: u3d_wgrad2d_workspace_floats() of the BOX dims
extern "C" int u3d_conv2d_wgrad_box(int device, u3d_stream_t stream, const u3d_src_t* src, const float* dz, float* dw, int N, int H, int W,
                                    int Cout, float* workspace, size_t workspace_floats, const int* box) {
    U3D_REQUIRE(box != nullptr, "u3d_conv2d_wgrad_box: box is NULL");
    return conv2d_wgrad_impl(device, stream, src, dz, dw, 0, N, H, W, Cout, workspace, workspace_floats, box);
}

// =================================================================================================
// Small-Cin family (`native_2d_stem`): the net's first convolution, Cin <= 4 and Cout <= 32, exact fp32 — the 2-D twins of
// csrc/u3d_smallc.hip.  K = 9 * Cin is far too small for the tiling above (Cin would be padded to a 16-channel chunk, 16 produced
// channels to a 32-column n-tile, and the weight gradient owns 32 x 32 channels), so the layer gets bandwidth-shaped kernels on the
// reference (Cout,Cin,3,3) weight layout, no packed image:
//   forward : a block walks 16 x 16-pixel tiles b, b + B, ... of one sample; the 18 x 18 halo goes through LDS with the affine applied
//             (padding stays exactly 0).  Cout % 4 == 0: GEMM on v_mfma_f32_16x16x4_f32 with the WEIGHTS as the A operand (rows = output
//             channels, K = 9 * Cin padded to 4: registers, loaded once per block) and 16 pixels of a row as the B columns — a lane's
//             accumulator is four consecutive channels of one pixel, stored as one 16-byte store (a row of 16 pixels x 16 channels =
//             1 KB contiguous).  Otherwise a direct kernel, one pixel per thread.  Statistics are carried in registers over a block's
//             tiles and leave it as one f64 atomic pair per channel.
//   backward: no data gradient.  With X[n,k,c,t] = sum_u dz[n,u,k] * x[n,u+t-1,c] and T[n,k,t] = sum_{u : u+t-1 in bounds} dz[n,u,k]
//             (9 taps t, T = the 9 border-class sums), dw and the GroupNorm-backward sums are linear in (X, T) — the identity at the
//             top of csrc/u3d_smallc.hip.  One pass over (dz, x) forms per-block partials of the GEMM P[k][(t,c)] (x with an in-bounds
//             indicator as channel Cin); the finalize kernel adds them in a fixed order: the same inputs give a bitwise-identical dw.
typedef float f32x4s __attribute__((ext_vector_type(4)));

namespace c2s {
constexpr int TY = 16, TX = 16;
constexpr int HY = TY + 2, HX = TX + 2;
constexpr int HV = HY * HX;  // 324 halo pixels
constexpr int MAXC = 4;
constexpr int FWD_BLOCKS = 512;   // blocks per launch over all samples (2 per CU: one f64 atomic pair per channel and block)
constexpr int BWD_BLOCKS = 1024;  // ~4 per CU; the finalize kernel's work is proportional to it
}  // namespace c2s

struct Small2dFwdParams {
    const float* x;       // (N,H,W,Cin)
    const float* affine;  // [N][Cin][2] or null
    const float* w;       // (Cout,Cin,9) reference layout
    float* out;           // (N,H,W,Cout)
    double* out_stats;    // optional [reps][N][Cout][2] += (sum, sum of squares) of the written values; block b adds to row b % reps
    int N, H, W, Cin, Cout, relu;
    int ty, tx, B, reps;
};

// direct form: any Cout <= COUTP, scalar stores (Cout % 4 != 0, or an `out` that is not 16-byte aligned)
template <int COUTP>
__global__ __launch_bounds__(256) void conv2d_small_fwd_kernel(const Small2dFwdParams p) {
    using namespace c2s;
    __shared__ __attribute__((aligned(16))) float xs[HV * MAXC];
    __shared__ __attribute__((aligned(16))) float ws[9 * MAXC * COUTP];
    __shared__ double sred[COUTP][2];
    const int t = threadIdx.x;
    const int n = blockIdx.y;
    const int Cin = p.Cin, H = p.H, W = p.W;
    // weights -> LDS as [tap][c][k] (k padded to COUTP with zeros)
    for (int i = t; i < 9 * Cin * COUTP; i += 256) {
        const int k = i % COUTP;
        const int r = i / COUTP;
        const int c = r % Cin, tap = r / Cin;
        ws[i] = k < p.Cout ? p.w[((size_t)k * Cin + c) * 9 + tap] : 0.f;
    }
    if (t < COUTP) sred[t][0] = sred[t][1] = 0.0;
    float s1[COUTP], s2[COUTP];
#pragma unroll
    for (int k = 0; k < COUTP; ++k) s1[k] = s2[k] = 0.f;
    const int yl = t >> 4, xl = t & 15;
    const int ntiles = p.ty * p.tx;
    for (int tile = blockIdx.x; tile < ntiles; tile += p.B) {
        const int y0 = (tile / p.tx) * TY, x0 = (tile % p.tx) * TX;
        __syncthreads();  // the previous tile's reads of xs are done (and ws / sred are initialised)
        for (int i = t; i < HV * Cin; i += 256) {
            const int c = i % Cin;
            const int hv = i / Cin;
            const int hy = hv / HX, hx = hv - hy * HX;
            const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
            float v = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                v = p.x[((size_t)(n * H + gy) * W + gx) * Cin + c];
                if (p.affine) v = v * p.affine[((size_t)n * Cin + c) * 2] + p.affine[((size_t)n * Cin + c) * 2 + 1];
            }
            xs[i] = v;
        }
        __syncthreads();
        float acc[COUTP];
#pragma unroll
        for (int k = 0; k < COUTP; ++k) acc[k] = 0.f;
        for (int tap = 0; tap < 9; ++tap) {
            const int hv = (yl + tap / 3) * HX + xl + tap % 3;
            for (int c = 0; c < Cin; ++c) {
                const float xv = xs[hv * Cin + c];
                const f32x4* wr = reinterpret_cast<const f32x4*>(&ws[(tap * Cin + c) * COUTP]);
#pragma unroll
                for (int k4 = 0; k4 < COUTP / 4; ++k4) {
                    const f32x4 wv = wr[k4];  // broadcast read
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[4 * k4 + e] = fmaf(xv, wv[e], acc[4 * k4 + e]);
                }
            }
        }
        const int y = y0 + yl, x = x0 + xl;
        if (y < H && x < W) {
            float* o = p.out + ((size_t)(n * H + y) * W + x) * p.Cout;
#pragma unroll
            for (int k = 0; k < COUTP; ++k) {
                if (p.relu) acc[k] = fmaxf(acc[k], 0.f);
                s1[k] += acc[k];  // padded channels (k >= Cout) are exactly 0
                s2[k] += acc[k] * acc[k];
                if (k < p.Cout) o[k] = acc[k];
            }
        }
    }
    if (p.out_stats) {
#pragma unroll
        for (int k = 0; k < COUTP; ++k) {
            float a = s1[k], b2 = s2[k];
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) {
                a += __shfl_xor(a, m);
                b2 += __shfl_xor(b2, m);
            }
            if ((t & 63) == 0) {
                __hip_atomic_fetch_add(&sred[k][0], (double)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&sred[k][1], (double)b2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
        if (t < p.Cout) {
            double* dst = p.out_stats + ((size_t)(blockIdx.x % (unsigned)p.reps) * p.N * p.Cout + (size_t)n * p.Cout + t) * 2;
            u3d_atomic_add_f64(dst, sred[t][0]);
            u3d_atomic_add_f64(dst + 1, sred[t][1]);
        }
    }
}

// matrix-pipe form: Cout % 4 == 0, `out` 16-byte aligned.  RT = row tiles of 16 output channels.  Wave w owns rows 4w .. 4w + 3 of the
// tile = 4 M-tiles of 16 pixels; the halo is double-buffered (the next tile's loads run under the current tile's MFMAs and stores).
template <int CIN, int RT>
__global__ __launch_bounds__(256) void conv2d_small_fwd_mfma_kernel(const Small2dFwdParams p) {
    using namespace c2s;
    constexpr int K = 9 * CIN;
    constexpr int KS = (K + 3) / 4;             // k-steps of 4
    constexpr int NH = (HV * CIN + 255) / 256;  // halo elements per thread
    __shared__ __attribute__((aligned(16))) float xsb[2][HV * CIN];
    __shared__ double sred[16 * RT][2];
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int j = l & 15, kq = l >> 4;  // B column (pixel of the M-tile) / A row (output channel); k index within a step
    const int n = blockIdx.y;
    const int H = p.H, W = p.W;
    // A fragments: W[k = 16 * rt + j][kk = 4 * s + kq], kk = tap * CIN + c
    float wa[RT][KS];
    int boff[KS];  // LDS offset of this lane's B element of step s, relative to the pixel's halo origin
#pragma unroll
    for (int s_ = 0; s_ < KS; ++s_) {
        const int kk = 4 * s_ + kq;
        const int tap = kk / CIN, c = kk - tap * CIN;
        const bool ok = kk < K;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) wa[rt][s_] = (ok && 16 * rt + j < p.Cout) ? p.w[((size_t)(16 * rt + j) * CIN + c) * 9 + tap] : 0.f;
        boff[s_] = ok ? ((tap / 3) * HX + tap % 3) * CIN + c : 0;  // dead k: any valid slot (A is 0)
    }
    if (t < 16 * RT) sred[t][0] = sred[t][1] = 0.0;
    f32x4s s1[RT], s2[RT];  // this lane's channels 16 * rt + 4 * kq .. +3 over its pixels
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) s1[rt] = s2[rt] = f32x4s{0.f, 0.f, 0.f, 0.f};
    const int vbase = 4 * w * HX + j;  // pixel of column j in M-tile mt: y = 4 * w + mt, x = j
    const int ntiles = p.ty * p.tx;
    // this thread's halo elements (element i = hv * CIN + c): constant coordinates inside the tile, and the affine of its channel
    int hrel[NH];  // hy * W + hx relative to the halo origin, in pixels; -1: beyond the 324 halo pixels
    int hco[NH];   // hy | hx << 8 | c << 24
    float ha[NH], hb[NH];
#pragma unroll
    for (int it = 0; it < NH; ++it) {
        const int i = t + 256 * it;
        const int c = i % CIN, hv = i / CIN;
        const int hy = hv / HX, hx = hv - hy * HX;
        hrel[it] = i < HV * CIN ? hy * W + hx : -1;
        hco[it] = hy | (hx << 8) | (c << 24);
        ha[it] = p.affine ? p.affine[((size_t)n * CIN + c) * 2] : 1.f;
        hb[it] = p.affine ? p.affine[((size_t)n * CIN + c) * 2 + 1] : 0.f;
    }
    auto halo_load = [&](int tile, float (&hv)[NH], unsigned& inside) {
        const int y0 = (tile / p.tx) * TY, x0 = (tile % p.tx) * TX;
        const long long base = ((long long)n * H + y0 - 1) * W + x0 - 1;
        inside = 0;
#pragma unroll
        for (int it = 0; it < NH; ++it) {
            const int gy = y0 - 1 + (hco[it] & 255), gx = x0 - 1 + ((hco[it] >> 8) & 255);
            const bool in = hrel[it] >= 0 && gy >= 0 && gy < H && gx >= 0 && gx < W;
            inside |= (in ? 1u : 0u) << it;
            hv[it] = in ? p.x[(size_t)(base + hrel[it]) * CIN + (hco[it] >> 24)] : 0.f;
        }
    };
    auto halo_store = [&](float* xs, const float (&hv)[NH], unsigned inside) {
#pragma unroll
        for (int it = 0; it < NH; ++it)
            if (t + 256 * it < HV * CIN) xs[t + 256 * it] = ((inside >> it) & 1u) ? fmaf(hv[it], ha[it], hb[it]) : 0.f;  // padding stays 0
    };
    float hv[NH];
    unsigned hin = 0;
    int cur = 0;
    if ((int)blockIdx.x < ntiles) {
        halo_load(blockIdx.x, hv, hin);
        halo_store(xsb[0], hv, hin);
    }
    __syncthreads();  // (also: sred initialised)
    for (int tile = blockIdx.x; tile < ntiles; tile += p.B) {
        const int y0 = (tile / p.tx) * TY, x0 = (tile % p.tx) * TX;
        const float* xs = xsb[cur];
        const bool has_next = tile + p.B < ntiles;
        if (has_next) halo_load(tile + p.B, hv, hin);
        f32x4s acc[RT][4];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[rt][mt] = f32x4s{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s_ = 0; s_ < KS; ++s_) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const float b = xs[(vbase + mt * HX) * CIN + boff[s_]];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[rt][s_], b, acc[rt][mt], 0, 0, 0);
            }
        }
        const int x = x0 + j;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int y = y0 + 4 * w + mt;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                f32x4s v = acc[rt][mt];
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                }
                if (16 * rt + 4 * kq < p.Cout && y < H && x < W) {  // (Cout % 4 == 0 on this path)
                    *reinterpret_cast<f32x4s*>(p.out + ((size_t)(n * H + y) * W + x) * p.Cout + 16 * rt + 4 * kq) = v;
                    s1[rt] += v;
                    s2[rt] += v * v;
                }
            }
        }
        if (has_next) halo_store(xsb[cur ^ 1], hv, hin);
        __syncthreads();  // the next tile's halo is complete; nobody reads the current buffer any more
        cur ^= 1;
    }
    if (p.out_stats) {
        // the 16 lanes j of a k-group hold 16 pixels of the same four channels: butterfly over j, then the four waves through LDS (f64),
        // one global f64 atomic pair per channel and block
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = s1[rt][e], b2 = s2[rt][e];
#pragma unroll
                for (int m = 8; m > 0; m >>= 1) {
                    a += __shfl_xor(a, m);
                    b2 += __shfl_xor(b2, m);
                }
                const int k = 16 * rt + 4 * kq + e;
                if (j == 0 && k < p.Cout) {
                    __hip_atomic_fetch_add(&sred[k][0], (double)a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&sred[k][1], (double)b2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        __syncthreads();
        if (t < p.Cout) {
            double* dst = p.out_stats + ((size_t)(blockIdx.x % (unsigned)p.reps) * p.N * p.Cout + (size_t)n * p.Cout + t) * 2;
            u3d_atomic_add_f64(dst, sred[t][0]);
            u3d_atomic_add_f64(dst + 1, sred[t][1]);
        }
    }
}

static bool c2s_envelope(int N, int H, int W, int Cin, int Cout) {
    return N > 0 && N <= 65535 && H > 0 && W > 0 && (long long)N * H * W < (1LL << 31) && Cin >= 1 && Cin <= c2s::MAXC && Cout >= 1 &&
           Cout <= 32;
}

static int c2s_blocks(int total, int N, int H, int W) {
    const long long ntiles = c2_cdiv(H, c2s::TY) * c2_cdiv(W, c2s::TX);
    long long B = total / N;
    if (B < 1) B = 1;
    if (B > ntiles) B = ntiles;
    return (int)B;
}

// which forward plan a launch with a 16-byte aligned `out` takes: bit 0 = matrix-pipe kernel (Cout % 4 == 0; else the direct one),
// bit 1 = a block walks more than one tile; -1 outside the envelope.  Host-only.
extern "C" int u3d_conv2d_small_cin_fwd_variant(int N, int H, int W, int Cin, int Cout) {
    if (!c2s_envelope(N, H, W, Cin, Cout)) return -1;
    const long long ntiles = c2_cdiv(H, c2s::TY) * c2_cdiv(W, c2s::TX);
    return (Cout % 4 == 0 ? 1 : 0) | (ntiles > c2s_blocks(c2s::FWD_BLOCKS, N, H, W) ? 2 : 0);
}

extern "C" int u3d_conv2d_small_cin_fwd_reps(int device, u3d_stream_t stream, const float* x, const float* affine, const float* w,
                                             float* out, int N, int H, int W, int Cin, int Cout, int relu, double* out_stats, int reps) {
    U3D_ENTER(device);
    U3D_REQUIRE(x && w && out, "u3d_conv2d_small_cin_fwd_reps: bad argument");
    U3D_REQUIRE(c2s_envelope(N, H, W, Cin, Cout), "u3d_conv2d_small_cin_fwd_reps: needs Cin<=4, Cout<=32, N*H*W < 2^31 (got %d,%d)", Cin,
                Cout);
    U3D_REQUIRE(reps >= 1 && reps <= 64, "u3d_conv2d_small_cin_fwd_reps: reps must be 1 .. 64");
    Small2dFwdParams p;
    p.x = x, p.affine = affine, p.w = w, p.out = out, p.out_stats = out_stats;
    p.N = N, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout, p.relu = relu;
    p.ty = (int)c2_cdiv(H, c2s::TY), p.tx = (int)c2_cdiv(W, c2s::TX);
    p.B = c2s_blocks(c2s::FWD_BLOCKS, N, H, W);
    p.reps = reps;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p.B, (unsigned)N);
    const bool mfma = Cout % 4 == 0 && ((uintptr_t)out & 15) == 0;
#define U3D_SMALL2D_FWD(CIN_)                                                                             \
    do {                                                                                                  \
        if (Cout <= 16)                                                                                   \
            hipLaunchKernelGGL((conv2d_small_fwd_mfma_kernel<CIN_, 1>), grid, dim3(256), 0, st, p);       \
        else                                                                                              \
            hipLaunchKernelGGL((conv2d_small_fwd_mfma_kernel<CIN_, 2>), grid, dim3(256), 0, st, p);       \
    } while (0)
    if (mfma && Cin == 1)
        U3D_SMALL2D_FWD(1);
    else if (mfma && Cin == 2)
        U3D_SMALL2D_FWD(2);
    else if (mfma && Cin == 3)
        U3D_SMALL2D_FWD(3);
    else if (mfma)
        U3D_SMALL2D_FWD(4);
    else if (Cout <= 8)
        hipLaunchKernelGGL(conv2d_small_fwd_kernel<8>, grid, dim3(256), 0, st, p);
    else if (Cout <= 16)
        hipLaunchKernelGGL(conv2d_small_fwd_kernel<16>, grid, dim3(256), 0, st, p);
    else
        hipLaunchKernelGGL(conv2d_small_fwd_kernel<32>, grid, dim3(256), 0, st, p);
#undef U3D_SMALL2D_FWD
    U3D_LAUNCH_CHECK();
    return 0;
}

// backward: partial[n][b][(k * 9 + tap) * (Cin + 1) + c]  (c == Cin is the T slot).  grid (B, N).  The contraction
// P[k][(tap,c)] = sum_u dz[u,k] * xs[u + tap][c] (xs = raw x with an in-bounds indicator as channel Cin, zero outside the image) is a
// GEMM with M = Cout, N = 9 * (Cin + 1), K = pixels on v_mfma_f32_16x16x4_f32: A[i = k][kk = pixel] straight from global dz,
// B[kk = pixel][j = column] from the LDS halo tile.  Wave w owns rows 4w .. 4w + 3 of the tile = 16 k-steps of 4 consecutive x; the four
// waves' sums are folded in a fixed order at the end of the block.
struct Small2dBwdParams {
    const float* x;   // raw input (N,H,W,Cin)
    const float* dz;  // (N,H,W,Cout)
    float* partial;
    int N, H, W, Cin, Cout;
    int ty, tx, B;
};

template <int CIN, int RT>  // RT = row tiles of 16 output channels (Cout <= 16 * RT)
__global__ __launch_bounds__(256) void conv2d_small_bwd_kernel(const Small2dBwdParams p) {
    using namespace c2s;
    constexpr int C1 = CIN + 1;
    constexpr int NCOL = 9 * C1;
    constexpr int NCT = (NCOL + 15) / 16;
    constexpr int NH = (HV + 255) / 256;  // halo pixels per thread (2)
    __shared__ float xsb[2][HV * C1];     // [hv][CIN + 1]: raw x, then the in-bounds indicator; two buffers
    __shared__ float red[RT * NCT * 4 * 64];
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int n = blockIdx.y;
    const int j = l & 15, kk = l >> 4;
    const int Cout = p.Cout, H = p.H, W = p.W;
    int boff[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
        const int col = ct * 16 + j;
        const int tap = col / C1, c = col - tap * C1;
        boff[ct] = col < NCOL ? ((tap / 3) * HX + tap % 3) * C1 + c : 0;  // dead columns read column 0; never written out
    }
    const int bbase = (4 * w * HX + kk) * C1;
    f32x4s acc[RT][NCT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = f32x4s{0.f, 0.f, 0.f, 0.f};
    const int ntiles = p.ty * p.tx;
    // A operands of a whole tile: dz[pixel(step, kk)][k = j + 16 * rt], zero outside the image / beyond Cout
    auto a_load = [&](int tile, float (&a)[RT][16]) {
        const int y0 = (tile / p.tx) * TY, x0 = (tile % p.tx) * TX;
#pragma unroll
        for (int s_ = 0; s_ < 16; ++s_) {
            const int y = y0 + 4 * w + (s_ >> 2), x = x0 + (s_ & 3) * 4 + kk;
            const bool vin = y < H && x < W;
            const size_t pix = (size_t)(n * H + (vin ? y : 0)) * W + (vin ? x : 0);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int k = j + 16 * rt;
                const float v = p.dz[pix * Cout + (k < Cout ? k : 0)];
                a[rt][s_] = (vin && k < Cout) ? v : 0.f;
            }
        }
    };
    auto halo_load = [&](int tile, float (&hx)[NH][CIN], unsigned& inside) {
        const int y0 = (tile / p.tx) * TY, x0 = (tile % p.tx) * TX;
        inside = 0;
#pragma unroll
        for (int it = 0; it < NH; ++it) {
            const int i = t + 256 * it;
            const int hy = i / HX, hxx = i - hy * HX;
            const int gy = y0 - 1 + hy, gx = x0 - 1 + hxx;
            const bool in = i < HV && gy >= 0 && gy < H && gx >= 0 && gx < W;
            inside |= (in ? 1u : 0u) << it;
            const float* src = p.x + (in ? ((size_t)(n * H + gy) * W + gx) * CIN : 0);
#pragma unroll
            for (int c = 0; c < CIN; ++c) hx[it][c] = in ? src[c] : 0.f;
        }
    };
    auto halo_store = [&](float* xs, const float (&hx)[NH][CIN], unsigned inside) {
#pragma unroll
        for (int it = 0; it < NH; ++it) {
            const int i = t + 256 * it;
            if (i < HV) {
#pragma unroll
                for (int c = 0; c < CIN; ++c) xs[i * C1 + c] = hx[it][c];
                xs[i * C1 + CIN] = ((inside >> it) & 1u) ? 1.f : 0.f;
            }
        }
    };
    float a[RT][16], hx[NH][CIN];
    unsigned hin = 0;
    int cur = 0;
    if ((int)blockIdx.x < ntiles) {
        a_load(blockIdx.x, a);
        halo_load(blockIdx.x, hx, hin);
        halo_store(xsb[0], hx, hin);
    }
    __syncthreads();
    for (int tile = blockIdx.x; tile < ntiles; tile += p.B) {
        const float* xs = xsb[cur];
        const bool has_next = tile + p.B < ntiles;
        float an[RT][16];
        if (has_next) {
            a_load(tile + p.B, an);
            halo_load(tile + p.B, hx, hin);
        }
#pragma unroll
        for (int s_ = 0; s_ < 16; ++s_) {
            const int so = ((s_ >> 2) * HX + (s_ & 3) * 4) * C1;
            float b[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) b[ct] = xs[bbase + so + boff[ct]];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][s_], b[ct], acc[rt][ct], 0, 0, 0);
        }
        if (has_next) {
            halo_store(xsb[cur ^ 1], hx, hin);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int s_ = 0; s_ < 16; ++s_) a[rt][s_] = an[rt][s_];
        }
        __syncthreads();  // the next tile's halo is complete; nobody reads the current buffer any more
        cur ^= 1;
    }
    // fold the four waves' partials (fixed order 0+1+2+3) through LDS, then write the block's partial.
    // D layout of 16x16x4: col = lane & 15, row = 4 * (lane >> 4) + reg
    for (int src = 1; src < 4; ++src) {
        __syncthreads();
        if (w == src) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[((rt * NCT + ct) * 4 + r) * 64 + l] = acc[rt][ct][r];
        }
        __syncthreads();
        if (w == 0) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[rt][ct][r] += red[((rt * NCT + ct) * 4 + r) * 64 + l];
        }
    }
    if (w != 0) return;
    float* dst = p.partial + ((size_t)n * p.B + blockIdx.x) * ((size_t)Cout * NCOL);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            const int col = ct * 16 + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = rt * 16 + 4 * kk + r;
                if (k < Cout && col < NCOL) dst[(size_t)k * NCOL + col] = acc[rt][ct][r];
            }
        }
}

// finalize: grid = ceil(Cout * 9 / 64) blocks of 1024 threads = 64 (k,tap) lanes x 16 partial-groups.  Fixed summation order; forms dw
// (summed over n in-thread) and adds the GroupNorm-backward sums (S1, S2) per (n, c).
constexpr int C2S_FIN_GROUPS = 16, C2S_FIN_UNROLL = 4;
__global__ __launch_bounds__(64 * C2S_FIN_GROUPS) void conv2d_small_bwd_finalize_kernel(const float* __restrict__ partial,
                                                                                       const float* __restrict__ affine,
                                                                                       const float* __restrict__ w, int N, int B, int Cin,
                                                                                       int Cout, float* __restrict__ dw,
                                                                                       double* __restrict__ gstats) {
    __shared__ float red[C2S_FIN_GROUPS][64][c2s::MAXC + 1];
    const int C1 = Cin + 1;
    const int nkt = Cout * 9;
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int kt = blockIdx.x * 64 + lane;
    const bool valid = kt < nkt;
    const int k = valid ? kt / 9 : 0, tap = valid ? kt % 9 : 0;
    double dwacc[c2s::MAXC];
    for (int c = 0; c < c2s::MAXC; ++c) dwacc[c] = 0.0;
    for (int n = 0; n < N; ++n) {
        float acc[c2s::MAXC + 1];
#pragma unroll
        for (int c = 0; c <= c2s::MAXC; ++c) acc[c] = 0.f;
        if (valid) {
            const float* base = partial + (size_t)n * B * ((size_t)nkt * C1) + (size_t)kt * C1;
            for (int b = grp; b < B; b += C2S_FIN_GROUPS * C2S_FIN_UNROLL) {
                float tmp[C2S_FIN_UNROLL][c2s::MAXC + 1];
#pragma unroll
                for (int u = 0; u < C2S_FIN_UNROLL; ++u) {
                    const int bb = b + u * C2S_FIN_GROUPS;
                    const float* src = base + (size_t)(bb < B ? bb : b) * ((size_t)nkt * C1);
#pragma unroll
                    for (int c = 0; c <= c2s::MAXC; ++c) tmp[u][c] = (c < C1 && bb < B) ? src[c] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < C2S_FIN_UNROLL; ++u)
#pragma unroll
                    for (int c = 0; c <= c2s::MAXC; ++c) acc[c] += tmp[u][c];
            }
        }
#pragma unroll
        for (int c = 0; c <= c2s::MAXC; ++c)
            if (c < C1) red[grp][lane][c] = acc[c];
        __syncthreads();
        if (grp == 0) {  // wave 0: lanes = 64 (k,tap) pairs
            double X[c2s::MAXC + 1];
            for (int c = 0; c < C1; ++c) {
                double sum = 0.0;
                for (int g = 0; g < C2S_FIN_GROUPS; ++g) sum += (double)red[g][lane][c];
                X[c] = sum;
            }
            const double T = X[Cin];
            for (int c = 0; c < Cin; ++c) {
                double s1 = 0.0, s2 = 0.0;
                if (valid) {
                    const double a = affine ? (double)affine[((size_t)n * Cin + c) * 2] : 1.0;
                    const double bb = affine ? (double)affine[((size_t)n * Cin + c) * 2 + 1] : 0.0;
                    dwacc[c] += a * X[c] + bb * T;
                    const double wv = (double)w[((size_t)k * Cin + c) * 9 + tap];
                    s1 = wv * T;
                    s2 = wv * X[c];
                }
                for (int m = 32; m > 0; m >>= 1) {
                    s1 += __shfl_xor(s1, m);
                    s2 += __shfl_xor(s2, m);
                }
                if (lane == 0 && gstats) {
                    u3d_atomic_add_f64(&gstats[((size_t)n * Cin + c) * 2], s1);
                    u3d_atomic_add_f64(&gstats[((size_t)n * Cin + c) * 2 + 1], s2);
                }
            }
        }
        __syncthreads();
    }
    if (grp == 0 && valid)
        for (int c = 0; c < Cin; ++c) dw[((size_t)k * Cin + c) * 9 + tap] = (float)dwacc[c];
}

extern "C" size_t u3d_small_cin2d_bwd_workspace_floats(int N, int H, int W, int Cin, int Cout) {
    if (!c2s_envelope(N, H, W, Cin, Cout)) return 0;
    return (size_t)N * c2s_blocks(c2s::BWD_BLOCKS, N, H, W) * Cout * 9 * (Cin + 1);
}

// which backward plan a launch takes: bit 0 = two row tiles of 16 output channels (Cout > 16), bit 1 = a block walks more than one
// tile, bit 2 = the finalize kernel adds more than one partial per sample; -1 outside the envelope.  Host-only.
extern "C" int u3d_conv2d_small_cin_bwd_variant(int N, int H, int W, int Cin, int Cout) {
    if (!c2s_envelope(N, H, W, Cin, Cout)) return -1;
    const long long ntiles = c2_cdiv(H, c2s::TY) * c2_cdiv(W, c2s::TX);
    const int B = c2s_blocks(c2s::BWD_BLOCKS, N, H, W);
    return (Cout > 16 ? 1 : 0) | (ntiles > B ? 2 : 0) | (B > 1 ? 4 : 0);
}

extern "C" int u3d_conv2d_small_cin_bwd(int device, u3d_stream_t stream, const float* x, const float* affine, const float* dz,
                                        const float* w, float* dw, double* gstats, int N, int H, int W, int Cin, int Cout,
                                        float* workspace, size_t workspace_floats) {
    U3D_ENTER(device);
    U3D_REQUIRE(x && dz && w && dw && workspace, "u3d_conv2d_small_cin_bwd: bad argument");
    U3D_REQUIRE(c2s_envelope(N, H, W, Cin, Cout), "u3d_conv2d_small_cin_bwd: needs Cin<=4, Cout<=32, N*H*W < 2^31 (got %d,%d)", Cin, Cout);
    Small2dBwdParams p;
    p.x = x, p.dz = dz, p.partial = workspace;
    p.N = N, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout;
    p.ty = (int)c2_cdiv(H, c2s::TY), p.tx = (int)c2_cdiv(W, c2s::TX);
    p.B = c2s_blocks(c2s::BWD_BLOCKS, N, H, W);
    const size_t need = (size_t)N * p.B * Cout * 9 * (Cin + 1);
    U3D_REQUIRE(workspace_floats >= need, "u3d_conv2d_small_cin_bwd: workspace too small (%zu < %zu floats)", workspace_floats, need);
    const dim3 grid((unsigned)p.B, (unsigned)N), block(256);
    hipStream_t st = (hipStream_t)stream;
#define U3D_SMALL2D_BWD(CIN_)                                                                \
    do {                                                                                     \
        if (Cout <= 16)                                                                      \
            hipLaunchKernelGGL((conv2d_small_bwd_kernel<CIN_, 1>), grid, block, 0, st, p);   \
        else                                                                                 \
            hipLaunchKernelGGL((conv2d_small_bwd_kernel<CIN_, 2>), grid, block, 0, st, p);   \
    } while (0)
    if (Cin == 1)
        U3D_SMALL2D_BWD(1);
    else if (Cin == 2)
        U3D_SMALL2D_BWD(2);
    else if (Cin == 3)
        U3D_SMALL2D_BWD(3);
    else
        U3D_SMALL2D_BWD(4);
#undef U3D_SMALL2D_BWD
    U3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(conv2d_small_bwd_finalize_kernel, dim3((Cout * 9 + 63) / 64), dim3(64 * C2S_FIN_GROUPS), 0, st, workspace, affine, w,
                       N, p.B, Cin, Cout, dw, gstats);
    U3D_LAUNCH_CHECK();
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
