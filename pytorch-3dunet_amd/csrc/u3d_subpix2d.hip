// u3d_subpix2d.hip — 3x3 convolution over a NEAREST-2x-UPSAMPLED tensor without the upsampled work: the 2-D twin of u3d_subpix.hip
// for the decoders of a UNet2D (`native_2d_subpixel: true`).
//
// A decoder's first SingleConv convolves cat(skip, interpolate(low, nearest)) (buildingblocks.py:491,:614,:56).  For the upsampled
// half, full-res pixel v reads low-res pixel v >> 1, so for an output pixel 2j + p (p = parity, per axis) the three taps t = 0,1,2 at
// full-res positions 2j + p + t - 1 hit only TWO low-res pixels:
//      p = 0:  t=0 -> j-1,  t=1,2 -> j          p = 1:  t=0,1 -> j,  t=2 -> j+1
// Taps that hit the same low-res pixel are added up ONCE in the weights (pack kernels), so each of the 4 output parity classes is a
// 2x2 convolution over the low-res grid: 16 instead of 36 multiply-adds per (low-res pixel, cin, cout) — 4/9 of the FLOPs, the same
// result up to fp32 association.  Zero padding carries over: full-res positions outside the image map exactly to low-res positions
// outside the low-res image.  All three kernels are implicit GEMMs on v_mfma_f32_32x32x2_f32 over fp32 NHWC tensors, built like the
// kernels of u3d_conv2d.hip (halo of a 16-channel chunk through LDS, two buffers, one barrier per chunk, B fragments streamed from a
// packed global image one k-step ahead).
//
// A level that upsamples n -> 2n + 1 along an axis (`native_2d_subpixel_plus`; F.interpolate(nearest) to an odd size reads
// src = (dst - 1) >> 1, src(0) = 0) is the same 2x tensor shifted by one pixel with low[0] once more in front: the `_win` entry points run
// the SAME three kernels with pixel u of the 2x grid at out[u + o] / dz[u + o] (and, for the gradients, counted only if u >= l) — offsets and
// predicate live in the staging descriptors and the epilogue addresses, the k-loops and the LDS layout do not know about them; the exact
// entry points pass o = l = 0.  The slab d < 2 of a shifted axis belongs to u3d_conv2d_box / u3d_conv2d_wgrad_box (csrc/u3d_conv2d.hip).
//
// Layout choices (why):
//   forward   a block of 4 waves owns a 16(y) x 8(x) LOW-RES tile (= 32 x 16 output pixels) and 32 output channels; wave w owns the
//             low-res rows 4w .. 4w + 3 as ONE 32-row M-tile and keeps the accumulators of all FOUR parity classes (4 x 16 registers).
//             The 18 x 10 halo of a chunk is staged once (GroupNorm affine fused, padding exactly 0) and serves every class: at each
//             of the 9 halo offsets only the classes that use it issue MFMAs (1, 2 or 4) — 16 k-steps of MFMAs per 9 A-fragment reads,
//             where four separate 2x2 convolutions would read 16.  An M-tile of 4 rows x 8 pixels with a pixel stride of 20 floats and
//             a row stride of 224 (= 32 mod 64) puts the 16 lanes of a ds_read_b128 phase on 16 distinct 4-bank groups: conflict-free.
//             The tile is tall rather than square so that every wave has the same work without sharing accumulators.  No split-K: the
//             workspace arguments are accepted and ignored, grids with fewer blocks than CUs run on few blocks.
//   dgrad     dlow[j] = sum over the 4 x 4 full-res neighbourhood dz[2j - 1 .. 2j + 2] with pre-summed taps (per axis t2, t1 + t2,
//             t0 + t1, t0): 16 multiply-adds where the full-resolution data gradient + children sum spends 36.  The stride-2 gather
//             would make every A-fragment read a 2-way bank conflict (pixel stride 2 x 20 floats), so dz is DE-INTERLEAVED while it
//             is staged: four parity planes of 9 x 9 pixels, each read exactly like the forward halo (tap = plane x 2 x 2 shifts).
//             A block owns an 8 x 8 low-res tile and 64 * NT input channels (wave = M-tile w & 1, n-tile group w >> 1).  The
//             GroupNorm-backward sums (sum dlow, sum dlow * x_low) leave the block as one f64 atomic per (sample, channel, quantity)
//             into replica row block % reps.
//   wgrad     the 16 matrices sum_j dz[2j + p] (x) g[j + p + e - 1] (4 parity classes p x 4 tap halves e) over the low-res grid; a
//             block owns 32 x 32 channels and a run of 8 x 8 low-res tiles, wave w owns class w (4 x 16 accumulator registers; dz is
//             staged per class, so a wave reads its A operands contiguously).  The block folds its 16 matrices into the 9 taps through
//             LDS in a fixed order and writes them to its slot of the workspace; a second kernel adds the slots in slot order into the
//             channel slice of dw: no atomics, the same inputs give a bitwise-identical result.
#include <algorithm>

#include "u3d_common.h"

namespace s2 {
constexpr int CC = 16;   // contraction channels per chunk
constexpr int CS = 20;   // pixel stride in LDS (floats)
constexpr int RS = 224;  // row stride in LDS (floats): >= 10 * CS and = 32 mod 64
// forward
constexpr int FLY = 16, FLX = 8;             // low-res tile
constexpr int FHY = FLY + 2, FHX = FLX + 2;  // halo
constexpr int FBUF = FHY * RS;               // 4032 floats per staging buffer
constexpr int FNITEMS = FHY * FHX * (CC / 4);
constexpr int FNIT = (FNITEMS + 255) / 256;  // 3
// data gradient
constexpr int DLY = 8, DLX = 8;              // low-res tile
constexpr int DPY = DLY + 1, DPX = DLX + 1;  // pixels per parity plane
constexpr int DPLANE = DPY * RS;             // 2016
constexpr int DBUF = 4 * DPLANE;             // 8064 floats per staging buffer
constexpr int DNITEMS = 4 * DPY * DPX * (CC / 4);
constexpr int DNIT = (DNITEMS + 255) / 256;  // 6
// weight gradient
constexpr int WLY = 8, WLX = 8;
constexpr int WHY = WLY + 2, WHX = WLX + 2;
constexpr int WCB = 32;
constexpr int WG_G = 0;                          // [WHY * WHX][32] low-res halo
constexpr int WG_DZ = WHY * WHX * WCB;           // [4 classes][64][32] dz
constexpr int WG_LDS_FLOATS = 16 * WCB * WCB;    // the fold: 16 matrices of 32 x 32 (>= WG_DZ + 4 * 64 * 32)
static_assert(WG_DZ + 4 * WLY * WLX * WCB <= WG_LDS_FLOATS, "staging must fit the fold buffer");
}  // namespace s2

static inline long long s2_cdiv(long long a, long long b) { return (a + b - 1) / b; }

static int s2_cu_count(int device) {
    static int cached[64] = {0};
    if (device >= 0 && device < 64 && cached[device] > 0) return cached[device];
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
    if (device >= 0 && device < 64) cached[device] = n;
    return n;
}

// per axis: the taps that hit low-res offset (a - 1 + p) for an output of parity p  — (first tap, count) of {t0}, {t1,t2} / {t0,t1}, {t2}
__host__ __device__ __forceinline__ void s2_fwd_taps(int p, int a, int& t0, int& nt) {
    if (p == 0) {
        t0 = a == 0 ? 0 : 1;
        nt = a == 0 ? 1 : 2;
    } else {
        t0 = a == 0 ? 0 : 2;
        nt = a == 0 ? 2 : 1;
    }
}
// per axis: the taps dz[2j - 1 + e] carries in the gradient of low[j], e = 0..3: t2, t1 + t2, t0 + t1, t0
__host__ __device__ __forceinline__ void s2_dgrad_taps(int e, int& t0, int& nt) {
    t0 = e == 0 ? 2 : (e == 1 ? 1 : 0);
    nt = (e == 1 || e == 2) ? 2 : 1;
}

// =================================================================================================
// weight images.  Forward: [chunk][class py*2+px][tap a*2+b][g][ntile][lane][4] of B[k = c1][n = co]; lane l of k-step j holds channel
// 16*chunk + 8g + 4*(l >> 5) + j of column l & 31 (the fragment convention of u3d_pack_weights2d).  Data gradient:
// [chunk][plane qy*2+qx][shift a*2+b][g][ntile][lane][4] of B[k = co][n = c1], the tap of dz[2j - 1 + (2a + q)] per axis.
extern "C" long long u3d_subpixel2d_packed_floats(int C1, int Cout) {
    if (C1 <= 0 || Cout <= 0) return 0;
    return s2_cdiv(C1, s2::CC) * 16 * 2 * s2_cdiv(Cout, 32) * 256;
}

extern "C" long long u3d_subpixel2d_dgrad_packed_floats(int Cout, int C1) {
    if (C1 <= 0 || Cout <= 0) return 0;
    return s2_cdiv(Cout, s2::CC) * 16 * 2 * s2_cdiv(C1, 32) * 256;
}

__global__ void pack_subpixel2d_kernel(const float* __restrict__ w, int Cout, int Cin_total, int c_off, int C1, int dgrad, int ntg,
                                       long long total, float* __restrict__ packed) {
    const int K = dgrad ? Cout : C1, Nn = dgrad ? C1 : Cout;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 3);
        const int lane = (int)((i >> 2) & 63);
        long long r = i >> 8;
        const int nt = (int)(r % ntg);
        r /= ntg;
        const int g = (int)(r & 1);
        r >>= 1;
        const int tap = (int)(r & 3);   // (a, b)
        const int cls = (int)((r >> 2) & 3);  // forward: parity class (py, px); data gradient: parity plane (qy, qx)
        const int chunk = (int)(r >> 4);
        const int k = chunk * s2::CC + 8 * g + 4 * (lane >> 5) + j;
        const int nn = nt * 32 + (lane & 31);
        float v = 0.f;
        if (k < K && nn < Nn) {
            int y0, ny, x0, nx;
            if (dgrad) {
                s2_dgrad_taps(2 * (tap >> 1) + (cls >> 1), y0, ny);
                s2_dgrad_taps(2 * (tap & 1) + (cls & 1), x0, nx);
            } else {
                s2_fwd_taps(cls >> 1, tap >> 1, y0, ny);
                s2_fwd_taps(cls & 1, tap & 1, x0, nx);
            }
            const int co = dgrad ? k : nn, c1 = dgrad ? nn : k;
            const float* wr = w + ((size_t)co * Cin_total + c_off + c1) * 9;
            for (int ty = y0; ty < y0 + ny; ++ty)
                for (int tx = x0; tx < x0 + nx; ++tx) v += wr[ty * 3 + tx];
        }
        packed[i] = v;
    }
}

static int s2_pack(int device, u3d_stream_t stream, const float* w, int Cout, int Cin_total, int c_off, int C1, int dgrad, float* packed,
                   const char* who) {
    U3D_ENTER(device);
    U3D_REQUIRE(w && packed && Cout > 0 && C1 > 0 && c_off >= 0 && c_off + C1 <= Cin_total, "%s: bad argument", who);
    const long long total = dgrad ? u3d_subpixel2d_dgrad_packed_floats(Cout, C1) : u3d_subpixel2d_packed_floats(C1, Cout);
    long long blocks = s2_cdiv(total, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_subpixel2d_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, Cout, Cin_total, c_off, C1,
                       dgrad, (int)s2_cdiv(dgrad ? C1 : Cout, 32), total, packed);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_pack_subpixel2d_weights(int device, u3d_stream_t stream, const float* w, int Cout, int Cin_total, int c_off, int C1,
                                           float* packed) {
    return s2_pack(device, stream, w, Cout, Cin_total, c_off, C1, 0, packed, "u3d_pack_subpixel2d_weights");
}

extern "C" int u3d_pack_subpixel2d_dgrad_weights(int device, u3d_stream_t stream, const float* w, int Cout, int Cin_total, int c_off,
                                                 int C1, float* packed) {
    return s2_pack(device, stream, w, Cout, Cin_total, c_off, C1, 1, packed, "u3d_pack_subpixel2d_dgrad_weights");
}

// GroupNorm (a, b) of 4 consecutive channels from interleaved rows (a0 b0 a1 b1 ...); rows == nullptr: identity
__device__ __forceinline__ void s2_load_affine(const float* rows, int cq, bool vec, f32x4& a, f32x4& b) {
    if (rows == nullptr) {
        a = f32x4{1.f, 1.f, 1.f, 1.f};
        b = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const float* p = rows + 2 * cq;
    if (vec) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(p);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(p + 4);
        a = f32x4{lo[0], lo[2], hi[0], hi[2]};
        b = f32x4{lo[1], lo[3], hi[1], hi[3]};
    } else {
        a = f32x4{p[0], p[2], p[4], p[6]};
        b = f32x4{p[1], p[3], p[5], p[7]};
    }
}

static bool s2_affine_vec(const float* affine, long long stride) { return affine && ((uintptr_t)affine & 15) == 0 && stride % 4 == 0; }

// =================================================================================================
// forward
struct Sp2FwdParams {
    const float* low;     // (N, H1, W1, C1)
    const float* affine;  // optional (a, b) rows of the C1 channels: affine[n * aff_stride + 2 * c]
    long long aff_stride;
    const float* wp;
    float* out;  // (N, 2 * H1, 2 * W1, Cout)
    int N, H1, W1, C1, Cout;
    int ty, tx, nchunks, ntg, avec;
    int Ho, Wo, oy, ox;  // u3d_subpixel2d_conv_fwd_win: pixel u of the 2x grid is written to out[u + o] of an (Ho, Wo) image (exact: 2*H1, 2*W1, 0, 0)
};

__global__ __launch_bounds__(256, 2) void subpixel2d_fwd_kernel(const Sp2FwdParams p) {
    using namespace s2;
    __shared__ __attribute__((aligned(16))) float lds[2 * FBUF];
    const int t = threadIdx.x;
    const int l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int tile = blockIdx.x;
    const int cb = tile % p.ntg;
    tile /= p.ntg;
    const int txi = tile % p.tx;
    tile /= p.tx;
    const int tyi = tile % p.ty;
    const int n = tile / p.ty;
    const int y0 = tyi * FLY, x0 = txi * FLX;
    const int H1 = p.H1, W1 = p.W1, C1 = p.C1;
    const float* arows = p.affine ? p.affine + (size_t)n * p.aff_stride : nullptr;

    // ---- staging descriptors (constant across chunks)
    int ldsoff[FNIT], cqs[FNIT];
    size_t goff[FNIT];
    bool oks[FNIT];
#pragma unroll
    for (int it = 0; it < FNIT; ++it) {
        const int item = t + 256 * it;
        const bool in = item < FNITEMS;
        const int pix = item >> 2, q = item & 3;
        const int hy = pix / FHX, hx = pix - (pix / FHX) * FHX;
        const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
        const bool ok = in && gy >= 0 && gy < H1 && gx >= 0 && gx < W1;
        oks[it] = ok;
        ldsoff[it] = in ? hy * RS + hx * CS + 4 * q : -1;
        cqs[it] = 4 * q;
        goff[it] = ok ? (((size_t)n * H1 + gy) * W1 + gx) * C1 : 0;
    }
    f32x4 raw[FNIT];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int it = 0; it < FNIT; ++it) {
            const int cq = c * CC + cqs[it];
            raw[it] = (oks[it] && cq < C1) ? *reinterpret_cast<const f32x4*>(p.low + goff[it] + cq) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_chunk = [&](int c, float* buf) {
#pragma unroll
        for (int it = 0; it < FNIT; ++it) {
            if (ldsoff[it] < 0) continue;
            const int cq = c * CC + cqs[it];
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (oks[it] && cq < C1) {  // (C1 % 4 == 0: whole quads)
                f32x4 a, b;
                s2_load_affine(arows, cq, p.avec != 0, a, b);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = raw[it][e] * a[e] + b[e];  // padding stays exactly 0
            }
            *reinterpret_cast<f32x4*>(buf + ldsoff[it]) = v;
        }
    };

    f32x16 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

    // A-fragment base: lane (i32, h) reads low-res pixel (4w + (i32 >> 3), i32 & 7), channels 8g + 4h .. +3
    const int abase = (4 * w + (i32 >> 3)) * RS + (i32 & 7) * CS + 4 * h;
    const f32x4* bimg = reinterpret_cast<const f32x4*>(p.wp) + cb * 64 + l;
    const int bstride = p.ntg * 64;  // fragments between two (class, tap, g) slots of the image
    // the B fragments of halo offset (hy, hx), channel octet g: one per class that uses the offset, in class order
    auto load_b = [&](const f32x4* bc, int step, f32x4 (&b)[4]) {
        const int off = step >> 1, g = step & 1;
        const int hy = off / 3, hx = off - (off / 3) * 3;
        int k = 0;
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            const int a = hy - (cls >> 1), bb = hx - (cls & 1);
            if (a < 0 || a > 1 || bb < 0 || bb > 1) continue;
            b[k++] = bc[((cls * 4 + (a * 2 + bb)) * 2 + g) * bstride];
        }
    };

    load_chunk(0);
    store_chunk(0, lds);
    __syncthreads();
    for (int c = 0; c < p.nchunks; ++c) {
        float* cur = lds + (c & 1) * FBUF;
        if (c + 1 < p.nchunks) load_chunk(c + 1);  // in flight during the k-loop
        f32x4 bq[4], bn[4];
        const f32x4* bc = bimg + (long long)c * 32 * bstride;
        load_b(bc, 0, bq);
#pragma unroll
        for (int step = 0; step < 18; ++step) {
            const int off = step >> 1, g = step & 1;
            const int hy = off / 3, hx = off - (off / 3) * 3;
            if (step + 1 < 18) load_b(bc, step + 1, bn);
            const f32x4 a = *reinterpret_cast<const f32x4*>(cur + abase + hy * RS + hx * CS + 8 * g);
            int k = 0;
#pragma unroll
            for (int cls = 0; cls < 4; ++cls) {
                const int ay = hy - (cls >> 1), ax = hx - (cls & 1);
                if (ay < 0 || ay > 1 || ax < 0 || ax > 1) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[cls] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], bq[k][j], acc[cls], 0, 0, 0);
                ++k;
            }
            if (step + 1 < 18) {
#pragma unroll
                for (int q = 0; q < 4; ++q) bq[q] = bn[q];
            }
        }
        if (c + 1 < p.nchunks) store_chunk(c + 1, lds + ((c + 1) & 1) * FBUF);  // (that buffer was last read in chunk c - 1)
        __syncthreads();
    }

    // ---- epilogue: lane column = output channel, register r = M row (r & 3) + 8 (r >> 2) + 4h = low-res pixel (row >> 3, row & 7)
    const int co = cb * 32 + i32;
    if (co >= p.Cout) return;
    const int H = p.Ho, W = p.Wo;
#pragma unroll
    for (int cls = 0; cls < 4; ++cls)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int ly = y0 + 4 * w + (row >> 3), lx = x0 + (row & 7);
            if (ly >= H1 || lx >= W1) continue;
            const int y = 2 * ly + (cls >> 1) + p.oy, x = 2 * lx + (cls & 1) + p.ox;  // (2 * H1 + oy <= Ho: inside the image)
            p.out[(((size_t)n * H + y) * W + x) * p.Cout + co] = acc[cls][r];
        }
}

static int s2_fwd_impl(int device, u3d_stream_t stream, const float* low, const float* affine, long long affine_sample_stride,
                       const float* packed, float* out, int N, int H1, int W1, int C1, int Cout, const int* win) {
    U3D_ENTER(device);
    U3D_REQUIRE(low && packed && out && N > 0 && H1 > 0 && W1 > 0 && C1 > 0 && Cout > 0 && C1 % 4 == 0 && Cout % 4 == 0 &&
                    4LL * N * H1 * W1 < (1LL << 31) && ((uintptr_t)low & 15) == 0 && ((uintptr_t)packed & 15) == 0,
                "u3d_subpixel2d_conv_fwd: bad argument (C1 %% 4 == Cout %% 4 == 0, 16-byte aligned tensors)");
    Sp2FwdParams p = {};
    p.low = low, p.affine = affine, p.aff_stride = affine_sample_stride, p.wp = packed, p.out = out;
    p.N = N, p.H1 = H1, p.W1 = W1, p.C1 = C1, p.Cout = Cout;
    p.ty = (int)s2_cdiv(H1, s2::FLY), p.tx = (int)s2_cdiv(W1, s2::FLX);
    p.nchunks = (int)s2_cdiv(C1, s2::CC), p.ntg = (int)s2_cdiv(Cout, 32);
    p.avec = s2_affine_vec(affine, affine_sample_stride) ? 1 : 0;
    p.Ho = 2 * H1, p.Wo = 2 * W1, p.oy = p.ox = 0;
    if (win) {
        p.Ho = win[0], p.Wo = win[1], p.oy = win[2], p.ox = win[3];
        U3D_REQUIRE(p.oy >= 0 && p.ox >= 0 && 2 * H1 + p.oy <= p.Ho && 2 * W1 + p.ox <= p.Wo && (long long)N * p.Ho * p.Wo < (1LL << 31),
                    "u3d_subpixel2d_conv_fwd_win: the shifted 2x grid does not fit the output");
    }
    const long long blocks = (long long)N * p.ty * p.tx * p.ntg;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_subpixel2d_conv_fwd: grid too large");
    hipLaunchKernelGGL(subpixel2d_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_subpixel2d_conv_fwd(int device, u3d_stream_t stream, const float* low, const float* affine,
                                       long long affine_sample_stride, const float* packed, float* out, int N, int H1, int W1, int C1,
                                       int Cout, float* workspace, long long workspace_floats) {
    (void)workspace;  // no split-K form: small grids run on few blocks
    (void)workspace_floats;
    return s2_fwd_impl(device, stream, low, affine, affine_sample_stride, packed, out, N, H1, W1, C1, Cout, nullptr);
}

// ... on a WINDOW, for a decoder level that upsamples n -> 2n + 1 along some axes (F.interpolate(nearest) to an odd skip size reads
// src = (dst - 1) >> 1: the exact 2x tensor shifted by one pixel with low[0] once more in front): win = {Ho, Wo, oy, ox}, pixel u of the
// 2x grid is written to out[u + o] of an (N, Ho, Wo, Cout) tensor.  Every output d >= 2 of a shifted axis is right; d = o is written but
// WRONG (it misses the extra copy of low[0]) and d = 0 is not written: u3d_conv2d_box overwrites the slab d < 2 on the same stream.
extern "C" int u3d_subpixel2d_conv_fwd_win(int device, u3d_stream_t stream, const float* low, const float* affine,
                                           long long affine_sample_stride, const float* packed, float* out, int N, int H1, int W1,
                                           int C1, int Cout, const int* win) {
    U3D_REQUIRE(win != nullptr, "u3d_subpixel2d_conv_fwd_win: win is NULL");
    return s2_fwd_impl(device, stream, low, affine, affine_sample_stride, packed, out, N, H1, W1, C1, Cout, win);
}

// =================================================================================================
// data gradient with respect to the low-res tensor (children sum included)
struct Sp2DgradParams {
    const float* dz;    // (N, 2 * H1, 2 * W1, Cout)
    const float* wp;
    const float* xlow;  // (N, H1, W1, C1), read only with gstats
    float* dlow;        // (N, H1, W1, C1)
    double* gstats;     // optional [reps][N][C1][2]
    int N, H1, W1, C1, Cout;
    int ty, tx, nchunks, ntg, ncb, reps;
    // u3d_subpixel2d_conv_dgrad_win: pixel u of the 2x grid is dz[u + o] of an (Hd, Wd) image and counts only if u >= l
    int Hd, Wd, oy, ox, ly, lx;
};

template <int NT>
__global__ __launch_bounds__(256, 2) void subpixel2d_dgrad_kernel(const Sp2DgradParams p) {
    using namespace s2;
    __shared__ __attribute__((aligned(16))) float lds[2 * DBUF];
    const int t = threadIdx.x;
    const int l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int tile = blockIdx.x;
    const int cb = tile % p.ncb;
    tile /= p.ncb;
    const int txi = tile % p.tx;
    tile /= p.tx;
    const int tyi = tile % p.ty;
    const int n = tile / p.ty;
    const int y0 = tyi * DLY, x0 = txi * DLX;
    const int H1 = p.H1, W1 = p.W1, C1 = p.C1, Cout = p.Cout;
    const int H = 2 * H1, W = 2 * W1;

    // ---- staging descriptors: plane (qy, qx) pixel (rr, cc) = dz[2 (y0 + rr) + qy - 1][2 (x0 + cc) + qx - 1]
    int ldsoff[DNIT], cqs[DNIT];
    size_t goff[DNIT];
    bool oks[DNIT];
#pragma unroll
    for (int it = 0; it < DNIT; ++it) {
        const int item = t + 256 * it;
        const bool in = item < DNITEMS;
        const int q = item & 3;
        int r = item >> 2;
        const int cc = r % DPX;
        r /= DPX;
        const int rr = r % DPY;
        const int plane = r / DPY;
        const int gy = 2 * (y0 + rr) + (plane >> 1) - 1, gx = 2 * (x0 + cc) + (plane & 1) - 1;
        const bool ok = in && gy >= p.ly && gy < H && gx >= p.lx && gx < W;  // (l >= 0)
        oks[it] = ok;
        ldsoff[it] = in ? plane * DPLANE + rr * RS + cc * CS + 4 * q : -1;
        cqs[it] = 4 * q;
        goff[it] = ok ? (((size_t)n * p.Hd + gy + p.oy) * p.Wd + gx + p.ox) * Cout : 0;
    }
    f32x4 raw[DNIT];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int it = 0; it < DNIT; ++it) {
            const int cq = c * CC + cqs[it];
            raw[it] = (oks[it] && cq < Cout) ? *reinterpret_cast<const f32x4*>(p.dz + goff[it] + cq) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_chunk = [&](float* buf) {
#pragma unroll
        for (int it = 0; it < DNIT; ++it)
            if (ldsoff[it] >= 0) *reinterpret_cast<f32x4*>(buf + ldsoff[it]) = raw[it];
    };

    f32x16 acc[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    const int mt = w & 1, np = w >> 1;  // M-tile (low-res rows 4mt .. 4mt + 3), n-tile group
    const int nt0 = (cb * 2 + np) * NT;
    const int abase = (4 * mt + (i32 >> 3)) * RS + (i32 & 7) * CS + 4 * h;
    const f32x4* bimg = reinterpret_cast<const f32x4*>(p.wp);
    auto load_b = [&](int c, int step, f32x4 (&b)[NT]) {
#pragma unroll
        for (int k = 0; k < NT; ++k)
            b[k] = (nt0 + k < p.ntg) ? bimg[(((long long)c * 32 + step) * p.ntg + nt0 + k) * 64 + l] : f32x4{0.f, 0.f, 0.f, 0.f};
    };

    load_chunk(0);
    store_chunk(lds);
    __syncthreads();
    for (int c = 0; c < p.nchunks; ++c) {
        float* cur = lds + (c & 1) * DBUF;
        if (c + 1 < p.nchunks) load_chunk(c + 1);
        f32x4 bq[NT], bn[NT];
        load_b(c, 0, bq);
#pragma unroll
        for (int step = 0; step < 32; ++step) {  // step = ((plane * 4 + shift) * 2 + g), the image's own order
            const int g = step & 1, shift = (step >> 1) & 3, plane = step >> 3;
            if (step + 1 < 32) load_b(c, step + 1, bn);
            const f32x4 a = *reinterpret_cast<const f32x4*>(cur + plane * DPLANE + abase + (shift >> 1) * RS + (shift & 1) * CS + 8 * g);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < NT; ++k) acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], bq[k][j], acc[k], 0, 0, 0);
            if (step + 1 < 32) {
#pragma unroll
                for (int k = 0; k < NT; ++k) bq[k] = bn[k];
            }
        }
        if (c + 1 < p.nchunks) store_chunk(lds + ((c + 1) & 1) * DBUF);
        __syncthreads();
    }

    // ---- epilogue: dlow and the GroupNorm-backward sums of its channels
    float s[NT][2];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        s[k][0] = s[k][1] = 0.f;
        const int c1 = (nt0 + k) * 32 + i32;
        if (c1 >= C1) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int ly = y0 + 4 * mt + (row >> 3), lx = x0 + (row & 7);
            if (ly >= H1 || lx >= W1) continue;
            const size_t o = (((size_t)n * H1 + ly) * W1 + lx) * C1 + c1;
            const float v = acc[k][r];
            p.dlow[o] = v;
            if (p.gstats) {
                s[k][0] += v;
                s[k][1] += v * p.xlow[o];
            }
        }
    }
    if (p.gstats == nullptr) return;  // (uniform)
    float* red = lds;  // [4 waves][NT][32][2] — the staging buffers are free after the loop's last barrier
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int q = 0; q < 2; ++q) s[k][q] += __shfl_xor(s[k][q], 32);
    if (l < 32)
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int q = 0; q < 2; ++q) red[((w * NT + k) * 32 + l) * 2 + q] = s[k][q];
    __syncthreads();
    if (t < 2 * NT * 32) {
        const int col = t & 31, k = (t >> 5) % NT, g = t / (32 * NT);
        const int c1 = ((cb * 2 + g) * NT + k) * 32 + col;
        if (c1 < C1) {
            const int w0 = 2 * g, w1 = 2 * g + 1;  // the two M-tiles of this n-tile group, in a fixed order
            const float a0 = red[((w0 * NT + k) * 32 + col) * 2] + red[((w1 * NT + k) * 32 + col) * 2];
            const float a1 = red[((w0 * NT + k) * 32 + col) * 2 + 1] + red[((w1 * NT + k) * 32 + col) * 2 + 1];
            double* o = p.gstats + (((size_t)(blockIdx.x % p.reps) * p.N + n) * C1 + c1) * 2;
            u3d_atomic_add_f64(o, (double)a0);
            u3d_atomic_add_f64(o + 1, (double)a1);
        }
    }
}

static int s2_dgrad_impl(int device, u3d_stream_t stream, const float* dz, const float* packed, const float* x_low, float* dlow,
                         double* gstats, int N, int H1, int W1, int C1, int Cout, int reps, const int* win) {
    U3D_ENTER(device);
    U3D_REQUIRE(dz && packed && dlow && N > 0 && H1 > 0 && W1 > 0 && C1 > 0 && Cout > 0 && C1 % 4 == 0 && Cout % 4 == 0 && reps >= 1 &&
                    4LL * N * H1 * W1 < (1LL << 31) && ((uintptr_t)dz & 15) == 0 && ((uintptr_t)packed & 15) == 0 && (!gstats || x_low),
                "u3d_subpixel2d_conv_dgrad_reps: bad argument (C1 %% 4 == Cout %% 4 == 0, 16-byte aligned tensors, gstats needs x_low)");
    Sp2DgradParams p = {};
    p.dz = dz, p.wp = packed, p.xlow = x_low, p.dlow = dlow, p.gstats = gstats;
    p.N = N, p.H1 = H1, p.W1 = W1, p.C1 = C1, p.Cout = Cout;
    p.ty = (int)s2_cdiv(H1, s2::DLY), p.tx = (int)s2_cdiv(W1, s2::DLX);
    p.nchunks = (int)s2_cdiv(Cout, s2::CC), p.ntg = (int)s2_cdiv(C1, 32);
    p.reps = reps;
    p.Hd = 2 * H1, p.Wd = 2 * W1, p.oy = p.ox = p.ly = p.lx = 0;
    if (win) {
        p.Hd = win[0], p.Wd = win[1], p.oy = win[2], p.ox = win[3], p.ly = win[4], p.lx = win[5];
        U3D_REQUIRE(p.oy >= 0 && p.ox >= 0 && 2 * H1 + p.oy <= p.Hd && 2 * W1 + p.ox <= p.Wd && p.ly >= 0 && p.lx >= 0 &&
                        (long long)N * p.Hd * p.Wd < (1LL << 31),
                    "u3d_subpixel2d_conv_dgrad_win: bad window");
    }
    const int nt = p.ntg > 2 ? 2 : 1;  // a block produces 64 * nt channels
    p.ncb = (int)s2_cdiv(p.ntg, 2 * nt);
    const long long blocks = (long long)N * p.ty * p.tx * p.ncb;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_subpixel2d_conv_dgrad_reps: grid too large");
    if (nt == 2)
        hipLaunchKernelGGL(subpixel2d_dgrad_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(subpixel2d_dgrad_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_subpixel2d_conv_dgrad_reps(int device, u3d_stream_t stream, const float* dz, const float* packed, const float* x_low,
                                              float* dlow, double* gstats, int N, int H1, int W1, int C1, int Cout, int reps) {
    return s2_dgrad_impl(device, stream, dz, packed, x_low, dlow, gstats, N, H1, W1, C1, Cout, reps, nullptr);
}

// ... reading dz through the window of u3d_subpixel2d_conv_fwd_win: win = {Hd, Wd, oy, ox, ly, lx} — dz is (N, Hd, Wd, Cout), pixel u of
// the 2x grid is dz[u + o] and counts only if u >= l (l = 1 on a shifted axis: the outputs d >= 2; the slab's share of the gradient
// comes from u3d_conv2d_box + u3d_nearest_childsum_add2d).  dlow is written, gstats as u3d_subpixel2d_conv_dgrad_reps.
extern "C" int u3d_subpixel2d_conv_dgrad_win(int device, u3d_stream_t stream, const float* dz, const float* packed, const float* x_low,
                                             float* dlow, double* gstats, int N, int H1, int W1, int C1, int Cout, int reps,
                                             const int* win) {
    U3D_REQUIRE(win != nullptr, "u3d_subpixel2d_conv_dgrad_win: win is NULL");
    return s2_dgrad_impl(device, stream, dz, packed, x_low, dlow, gstats, N, H1, W1, C1, Cout, reps, win);
}

// =================================================================================================
// weight gradient of the upsampled channels
struct Sp2WgradParams {
    const float* low;
    const float* affine;
    long long aff_stride;
    const float* dz;
    float* dst;  // workspace [nsplit][Cout][C1][9]
    int N, H1, W1, C1, Cout;
    int ty, tx, ncob, ncib, ntiles, tps, avec;
    int Hd, Wd, oy, ox, ly, lx;  // the dz window of Sp2DgradParams
};

__global__ __launch_bounds__(256, 2) void subpixel2d_wgrad_kernel(const Sp2WgradParams p) {
    using namespace s2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int t = threadIdx.x, l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int b = blockIdx.x;
    const int cib = b % p.ncib;
    b /= p.ncib;
    const int cob = b % p.ncob;
    const int split = b / p.ncob;
    const int ci0 = cib * WCB, co0 = cob * WCB;
    const int tile0 = split * p.tps, tile1 = min(p.ntiles, tile0 + p.tps);
    const int H1 = p.H1, W1 = p.W1, C1 = p.C1, Cout = p.Cout;
    float* const gl = lds + WG_G;
    float* const dzl = lds + WG_DZ;
    const int py = w >> 1, px = w & 1;  // wave w owns parity class w

    f32x16 acc[4];  // tap halves (a, b): g[j + py + a - 1][i + px + b - 1]
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    for (int tile = tile0; tile < tile1; ++tile) {
        int tt = tile;
        const int txi = tt % p.tx;
        tt /= p.tx;
        const int tyi = tt % p.ty;
        const int n = tt / p.ty;
        const int y0 = tyi * WLY, x0 = txi * WLX;
        const float* arows = p.affine ? p.affine + (size_t)n * p.aff_stride : nullptr;
        // stage g (10 x 10 low-res halo, 32 channels from ci0, affine, zero padding) ...
        for (int item = t; item < WHY * WHX * (WCB / 4); item += 256) {
            const int pix = item >> 3, q = item & 7;
            const int hy = pix / WHX, hx = pix - (pix / WHX) * WHX;
            const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
            const int cq = ci0 + 4 * q;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (gy >= 0 && gy < H1 && gx >= 0 && gx < W1 && cq < C1) {
                const f32x4 r = *reinterpret_cast<const f32x4*>(p.low + (((size_t)n * H1 + gy) * W1 + gx) * C1 + cq);
                f32x4 a, bb;
                s2_load_affine(arows, cq, p.avec != 0, a, bb);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = r[e] * a[e] + bb[e];
            }
            *reinterpret_cast<f32x4*>(gl + pix * WCB + 4 * q) = v;
        }
        // ... and dz (16 x 16 full-res pixels, 32 channels from co0) by parity class: [class][8 x 8 low-res pixel][32]
        for (int item = t; item < 4 * WLY * WLX * (WCB / 4); item += 256) {
            const int q = item & 7, idx = item >> 3;
            const int cls = idx >> 6, pp = idx & 63;
            const int ly = y0 + (pp >> 3), lx = x0 + (pp & 7);
            const int cq = co0 + 4 * q;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            const int uy = 2 * ly + (cls >> 1), ux = 2 * lx + (cls & 1);  // pixel of the 2x grid
            if (ly < H1 && lx < W1 && cq < Cout && uy >= p.ly && ux >= p.lx)
                v = *reinterpret_cast<const f32x4*>(p.dz + (((size_t)n * p.Hd + uy + p.oy) * p.Wd + ux + p.ox) * Cout + cq);
            *reinterpret_cast<f32x4*>(dzl + idx * WCB + 4 * q) = v;
        }
        __syncthreads();
        // K = the tile's 64 low-res pixels, two per k-step (lane half h)
#pragma unroll 2
        for (int kk = 0; kk < 32; ++kk) {
            const int pix = 2 * kk + h;
            const float a = dzl[(w * 64 + pix) * WCB + i32];
            const float* gp = gl + (((pix >> 3) + py) * WHX + (pix & 7) + px) * WCB + i32;
#pragma unroll
            for (int ay = 0; ay < 2; ++ay)
#pragma unroll
                for (int ax = 0; ax < 2; ++ax)
                    acc[ay * 2 + ax] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, gp[(ay * WHX + ax) * WCB], acc[ay * 2 + ax], 0, 0, 0);
        }
        __syncthreads();
    }

    // ---- fold the 16 (class, tap half) matrices into the 9 taps in a fixed order through LDS; write [co][c1][tap] of this split
    float* red = lds;  // [class][tap half][32][32]
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;  // output channel within the block
            red[((w * 4 + k) * WCB + row) * WCB + i32] = acc[k][r];
        }
    __syncthreads();
    float* const dst = p.dst + (size_t)split * Cout * C1 * 9;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int idx = t + 256 * e;
        const int row = idx >> 5, col = idx & 31;
        const int co = co0 + row, ci = ci0 + col;
        if (co >= Cout || ci >= C1) continue;
#pragma unroll
        for (int ty = 0; ty < 3; ++ty)
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) {
                // per axis, tap t lies in (parity, half): t0 -> (0,0), (1,0); t1 -> (0,1), (1,0); t2 -> (0,1), (1,1)
                const int ya[2] = {ty == 0 ? 0 : 1, ty == 2 ? 1 : 0};
                const int xa[2] = {tx == 0 ? 0 : 1, tx == 2 ? 1 : 0};
                float v = 0.f;
#pragma unroll
                for (int qy = 0; qy < 2; ++qy)
#pragma unroll
                    for (int qx = 0; qx < 2; ++qx)
                        v += red[(((qy * 2 + qx) * 4 + ya[qy] * 2 + xa[qx]) * WCB + row) * WCB + col];
                dst[((size_t)co * C1 + ci) * 9 + ty * 3 + tx] = v;
            }
    }
}

// dw[co][c_off + c1][tap] = sum over splits in split order (bitwise-reproducible)
__global__ void subpixel2d_wgrad_reduce_kernel(const float* __restrict__ ws, int nsplit, long long total, int row, int dw_row,
                                               float* __restrict__ dw) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) v += ws[(size_t)s * total + i];
        dw[(i / row) * dw_row + (i % row)] = v;
    }
}

struct S2WPlan {
    int ty, tx, ncob, ncib, ntiles, tps, nsplit;
};

static S2WPlan s2_wplan(int device, int N, int H1, int W1, int C1, int Cout) {
    S2WPlan pl;
    pl.ty = (int)s2_cdiv(H1, s2::WLY);
    pl.tx = (int)s2_cdiv(W1, s2::WLX);
    pl.ncob = (int)s2_cdiv(Cout, s2::WCB);
    pl.ncib = (int)s2_cdiv(C1, s2::WCB);
    pl.ntiles = N * pl.ty * pl.tx;
    const long long cells = (long long)pl.ncob * pl.ncib;
    const long long target = 4LL * s2_cu_count(device);  // ~4 blocks per CU over the launch
    const long long ns = std::max<long long>(1, std::min<long long>(pl.ntiles, s2_cdiv(target, cells)));
    pl.tps = (int)s2_cdiv(pl.ntiles, ns);
    pl.nsplit = (int)s2_cdiv(pl.ntiles, pl.tps);
    return pl;
}

extern "C" long long u3d_subpixel2d_wgrad_workspace_floats(int N, int H1, int W1, int C1, int Cout) {
    if (N <= 0 || H1 <= 0 || W1 <= 0 || C1 <= 0 || Cout <= 0) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const S2WPlan pl = s2_wplan(dev, N, H1, W1, C1, Cout);
    return (long long)pl.nsplit * Cout * C1 * 9;  // (always: the block results go through the workspace, also with one split)
}

static int s2_wgrad_impl(int device, u3d_stream_t stream, const float* low, const float* affine, long long affine_sample_stride,
                         const float* dz, float* dw, int dw_cin_stride, int N, int H1, int W1, int C1, int Cout, float* workspace,
                         long long workspace_floats, const int* win) {
    U3D_ENTER(device);
    U3D_REQUIRE(low && dz && dw && N > 0 && H1 > 0 && W1 > 0 && C1 > 0 && Cout > 0 && C1 % 4 == 0 && Cout % 4 == 0 &&
                    dw_cin_stride >= C1 && 4LL * N * H1 * W1 < (1LL << 31) && ((uintptr_t)low & 15) == 0 && ((uintptr_t)dz & 15) == 0,
                "u3d_subpixel2d_conv_wgrad: bad argument (C1 %% 4 == Cout %% 4 == 0, 16-byte aligned tensors, dw_cin_stride >= C1)");
    const S2WPlan pl = s2_wplan(device, N, H1, W1, C1, Cout);
    const long long need = (long long)pl.nsplit * Cout * C1 * 9;
    if (!workspace || workspace_floats < need)
        return u3d_set_err(U3D_EWORKSPACE, "u3d_subpixel2d_conv_wgrad: workspace too small (%lld < %lld floats)", workspace_floats, need);
    Sp2WgradParams p = {};
    p.low = low, p.affine = affine, p.aff_stride = affine_sample_stride, p.dz = dz, p.dst = workspace;
    p.N = N, p.H1 = H1, p.W1 = W1, p.C1 = C1, p.Cout = Cout;
    p.ty = pl.ty, p.tx = pl.tx, p.ncob = pl.ncob, p.ncib = pl.ncib, p.ntiles = pl.ntiles, p.tps = pl.tps;
    p.avec = s2_affine_vec(affine, affine_sample_stride) ? 1 : 0;
    p.Hd = 2 * H1, p.Wd = 2 * W1, p.oy = p.ox = p.ly = p.lx = 0;
    if (win) {
        p.Hd = win[0], p.Wd = win[1], p.oy = win[2], p.ox = win[3], p.ly = win[4], p.lx = win[5];
        U3D_REQUIRE(p.oy >= 0 && p.ox >= 0 && 2 * H1 + p.oy <= p.Hd && 2 * W1 + p.ox <= p.Wd && p.ly >= 0 && p.lx >= 0 &&
                        (long long)N * p.Hd * p.Wd < (1LL << 31),
                    "u3d_subpixel2d_conv_wgrad_win: bad window");
    }
    const size_t lds = s2::WG_LDS_FLOATS * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
        U3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(subpixel2d_wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
        attr_set = true;
    }
    const long long blocks = (long long)pl.nsplit * pl.ncob * pl.ncib;
    hipLaunchKernelGGL(subpixel2d_wgrad_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    const long long total = (long long)Cout * C1 * 9;
    long long rb = s2_cdiv(total, 256);
    if (rb > 4096) rb = 4096;
    hipLaunchKernelGGL(subpixel2d_wgrad_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace, pl.nsplit, total,
                       C1 * 9, dw_cin_stride * 9, dw);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_subpixel2d_conv_wgrad(int device, u3d_stream_t stream, const float* low, const float* affine,
                                         long long affine_sample_stride, const float* dz, float* dw, int dw_cin_stride, int N, int H1,
                                         int W1, int C1, int Cout, float* workspace, long long workspace_floats) {
    return s2_wgrad_impl(device, stream, low, affine, affine_sample_stride, dz, dw, dw_cin_stride, N, H1, W1, C1, Cout, workspace,
                         workspace_floats, nullptr);
}

// ... with dz read through the window of u3d_subpixel2d_conv_dgrad_win (the same 6 integers): the weight gradient of the outputs d >= 2
// of a level that upsamples n -> 2n + 1; the slab's share comes from u3d_conv2d_wgrad_box.  Same plan, same fixed-order fold and reduce.
extern "C" int u3d_subpixel2d_conv_wgrad_win(int device, u3d_stream_t stream, const float* low, const float* affine,
                                             long long affine_sample_stride, const float* dz, float* dw, int dw_cin_stride, int N, int H1,
                                             int W1, int C1, int Cout, float* workspace, long long workspace_floats, const int* win) {
    U3D_REQUIRE(win != nullptr, "u3d_subpixel2d_conv_wgrad_win: win is NULL");
    return s2_wgrad_impl(device, stream, low, affine, affine_sample_stride, dz, dw, dw_cin_stride, N, H1, W1, C1, Cout, workspace,
                         workspace_floats, win);
}
