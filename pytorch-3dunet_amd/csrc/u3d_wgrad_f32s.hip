// u3d_wgrad_f32s.hip — the weight gradient of `compute_dtype: fp32_split` on the bf16 MFMA (`fp32_split_wgrad: true`): fp32-grade
// arithmetic from six bf16 partial products, the weight-gradient twin of conv3d_f32s_kernel (csrc/u3d_bf16.hip).  The second translation
// unit of libu3d_ext_hip.so (include/u3d_ext.h); u3d_set_err / u3d_last_error and u3d_device_guard are the core library's.
// Self-contained like csrc/u3d_c16_bf16.hip, whose weight-gradient tiling it takes over.  The unit also carries the 3x3 Conv2d kernels of
// a UNet2D in fp32_split (`native_2d_fp32_split: true`): csrc/u3d_conv2d_f32s.h, included at the end of this file.
//
// dw[co][ci][tap] = sum_v dz[v][co] * g[v + tap - 1][ci], g = fmaf(x, a, b) zero padded after the affine.  Tensors are fp32 NDHWC.
//
// Arithmetic.  Both operands are split while staged to LDS, after the fp32 affine: h = bf16(g), m = bf16(g - h), l = bf16(g - h - m)
// (round to nearest even; the two subtractions are exact, so h + m + l == g bit for bit whenever g's 24 significant bits fit — always
// but for values next to the bf16 underflow).  The six products of conv3d_f32s_kernel, smallest class first: (dz, g) parts
// (h, l) (l, h) (m, m) (h, m) (m, h) (h, h); the three dropped ones are below 2^-24 of the product.  Accumulation is fp32, in the MFMA.
//
// The accumulation drift.  v_mfma_f32_32x32x16_bf16 rounds its fp32 accumulation toward minus infinity (DESIGN_HISTORY.md 4.9): a drift
// linear in the chain length, which here runs over voxels.  CHOSEN: both remedies, because each alone leaves something.  (1) The MFMA
// chain is closed after every tile: a tile's 8 K-steps x 6 products = 48 MFMAs (128 voxels) per accumulator start from zero and are
// added to a second fp32 register set with VALU adds (round to nearest).  What remains is that chain of 48.  Alone this still leaves the
// chain's own round-down bias, the same relative amount in every tile when the operands have a mean.  (2) Sign alternation, as in the
// forward kernel: the three parts of dz are staged with the sign (-1)^(tile - first tile of the block) — negating an fp32 value before
// the split negates its three parts exactly — and the closing add becomes a subtract for odd tiles, so the bias of consecutive tiles has
// opposite sign in the result and cancels.  Alone (one chain over the block's whole tile range, accumulators negated between tiles) it
// cancels the bias but keeps a chain of thousands of fp32 additions at the magnitude of the final sum: measured 9.5e-7 relative L2 on 80
// tiles in one slot against 1.8e-7 on one tile per slot.
//
// Tiling (wf_wgrad_kernel).  A block of 9 waves owns one (32 co, 32 ci) cell and a range of 2 x 4 x 16-voxel tiles.  The three bf16 parts
// of the 4 x 6 x 18 halo of g and of the 128 voxels of dz sit in LDS as [part][voxel][32 channels] (3 x 27648 + 3 x 8192 = 107520
// bytes, ONE buffer, one block per CU) and are fetched as MFMA operands with ds_read_b64_tr_b16, one 16-voxel x-row per K step.  Wave
// = (kz, ky), which owns the taps kx = 0, 1, 2 as three running sums; it walks them one kx at a time, 8 rows x 6 products in ONE
// accumulator, reading 3 + 3 fragments per row and kx for 6 MFMAs (all three kx per row in three accumulators next to the three sums
// read a third fewer fragments but needs 168 registers and spills 11: measured slower).  The next tile's global loads are in flight during
// the MFMAs of this one.  Every block writes its 27 matrices to its workspace slot [tap][Cout][Cin]; wf_reduce_kernel adds the slots —
// four contiguous slot ranges in slot order each, then the four in order — and writes dw in the reference layout with the caller's
// channel stride.  No atomics: the same inputs and workspace size give the same bits.
#include "u3d_common.h"

extern "C" {
#include <u3d_ext.h>
}

#include <algorithm>

typedef __bf16 wf_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wf_bf16x4 __attribute__((ext_vector_type(4)));
typedef short wf_s16x4 __attribute__((ext_vector_type(4)));
typedef short wf_s16x8 __attribute__((ext_vector_type(8)));

namespace {

namespace wf {
constexpr int TZ = 2, TY = 4, TX = 16;                 // tile: 8 rows of 16 x
constexpr int HZ = TZ + 2, HY = TY + 2, HX = TX + 2;   // 4 x 6 x 18 halo
constexpr int PP = 64;                                 // bytes per staged voxel and part (32 bf16)
constexpr int VOX = TZ * TY * TX;                      // 128
constexpr int THREADS = 576;                           // 9 waves: (kz, ky)
constexpr int G_PART = HZ * HY * HX * PP;              // 27648 bytes per part of the halo
constexpr int D_PART = VOX * PP;                       // 8192 bytes per part of dz
constexpr int L_G = 0;
constexpr int L_DZ = 3 * G_PART;                       // 82944
constexpr int LDS_BYTES = L_DZ + 3 * D_PART;           // 107520
constexpr int GITEMS = HZ * HY * HX * 4;               // 1728 (voxel, octet) halo items = 3 per thread
constexpr int GIT = GITEMS / THREADS;                  // 3
static_assert(GIT * THREADS == GITEMS, "the halo items divide evenly over the block");
constexpr int DITEMS = VOX * 4;                        // 512 dz items: threads 0 .. 511
constexpr int RED_PARTS = 4;                           // slot ranges of the reduce kernel
}  // namespace wf

inline long long wf_cdiv(long long a, long long b) { return (a + b - 1) / b; }
inline bool wf_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool wf_ok(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0; }
inline bool wf_dims_ok(int N, int D, int H, int W, int Cin, int Cout) {
    return N > 0 && D > 0 && H > 0 && W > 0 && (long long)N * D * H * W < (1ll << 31) && (long long)27 * Cin * Cout < (1ll << 31);
}

int wf_cu_count(int device) {
    static int cached[64] = {0};
    if (device >= 0 && device < 64 && cached[device] > 0) return cached[device];
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
    if (device >= 0 && device < 64) cached[device] = n;
    return n;
}

int wf_current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return dev;
}

// 8 staged channels: affine in fp32 (one fused multiply-add per element), sign, zero outside the volume, then the exact three-way split
__device__ __forceinline__ void wf_split8(const f32x4& lo, const f32x4& hi, const float* aff, bool ok, bool neg, wf_bf16x8& oh, wf_bf16x8& om,
                                          wf_bf16x8& ol) {
    f32x4 v0 = lo, v1 = hi;
    if (aff != nullptr) {
        const f32x4 q0 = u3d_ldq(aff), q1 = u3d_ldq(aff + 4), q2 = u3d_ldq(aff + 8), q3 = u3d_ldq(aff + 12);  // (a, b) pairs
        v0 = f32x4{fmaf(lo[0], q0[0], q0[1]), fmaf(lo[1], q0[2], q0[3]), fmaf(lo[2], q1[0], q1[1]), fmaf(lo[3], q1[2], q1[3])};
        v1 = f32x4{fmaf(hi[0], q2[0], q2[1]), fmaf(hi[1], q2[2], q2[3]), fmaf(hi[2], q3[0], q3[1]), fmaf(hi[3], q3[2], q3[3])};
    }
    if (!ok) v0 = v1 = f32x4{0.f, 0.f, 0.f, 0.f};  // padding stays exactly 0
    if (neg) v0 = -v0, v1 = -v1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float g = e < 4 ? v0[e & 3] : v1[e & 3];
        const __bf16 h = (__bf16)g;
        const float r1 = g - (float)h;
        const __bf16 m = (__bf16)r1;
        oh[e] = h, om[e] = m, ol[e] = (__bf16)(r1 - (float)m);
    }
}

// ds_read_b64_tr_b16 x 2: lane l receives channel (l & 31) of the 8 voxels 8 * (l >> 5) .. + 7 of a [voxel][32 channels] run
__device__ __forceinline__ wf_bf16x8 wf_tr_frag(const char* lds_addr) {
    const wf_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) wf_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)lds_addr);
    const wf_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) wf_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)(lds_addr + 4 * wf::PP));
    const wf_s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(wf_bf16x8, v);
}

struct WfParams {
    const float* x;       // (N,D,H,W,Cin)
    const float* affine;  // (N,Cin,2) or null
    const float* dz;      // (N,D,H,W,Cout)
    float* ws;            // [nsplit][27][Cout][Cin]
    int N, D, H, W, Cin, Cout;
    int tz, ty, tx, ncob, ncib, ntiles, tps;
};

__global__ __launch_bounds__(576) void wf_wgrad_kernel(const WfParams p) {
    using namespace wf;
    extern __shared__ __attribute__((aligned(16))) char lds_wf[];
    char* const lds = lds_wf;
    const int t = threadIdx.x, l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int b = blockIdx.x;
    const int cib = b % p.ncib;
    b /= p.ncib;
    const int cob = b % p.ncob;
    const int split = b / p.ncob;
    const int ci0 = cib * 32, co0 = cob * 32;
    const int tile0 = split * p.tps, tile1 = min(p.ntiles, tile0 + p.tps);
    const int D = p.D, H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout;
    char* const gl = lds + L_G;
    char* const dzl = lds + L_DZ;
    const int kz = w / 3, ky = w % 3;  // this wave's tap plane and row

    // the block's running sums; a tile's MFMA chains start from zero and are closed into them with VALU adds (round to nearest)
    f32x16 tot[3];  // [kx]
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[k][r] = 0.f;

    // transposed-read lane offset: lane l receives channel (l & 31) of the 8 voxels 8 * (l >> 5) .. + 7
    const int g4 = l >> 4, sidx = l & 15;
    const int lane_off = (8 * (g4 >> 1) + (sidx >> 2)) * PP + (16 * (g4 & 1) + 4 * (sidx & 3)) * 2;

    // a tile's operands: g (4 x 6 x 18 halo from (z0 - 1, y0 - 1, x0 - 1), 32 channels from ci0: affine, zero padding) and dz (the 128
    // voxels of the tile, 32 channels from co0, zero outside the volume).  load_tile puts the raw fp32 values in registers — the next
    // tile's are in flight during this tile's MFMAs (one block is resident per CU) —, store_tile splits and stages them
    f32x4 rg[GIT][2], rd[2];
    bool okg[GIT], okd = false;
    const float* aff_n = nullptr;
    auto load_tile = [&](int tile) {
        int tt = tile;
        const int txi = tt % p.tx;
        tt /= p.tx;
        const int tyi = tt % p.ty;
        tt /= p.ty;
        const int tzi = tt % p.tz;
        const int n = tt / p.tz;
        const int z0 = tzi * TZ, y0 = tyi * TY, x0 = txi * TX;
        aff_n = p.affine != nullptr ? p.affine + (size_t)n * Cin * 2 : nullptr;
#pragma unroll
        for (int k = 0; k < GIT; ++k) {
            const int item = t + THREADS * k;
            const int q = item & 3;
            int pix = item >> 2;
            const int hx = pix % HX;
            pix /= HX;
            const int hy = pix % HY;
            const int hz = pix / HY;
            const int gz = z0 - 1 + hz, gy = y0 - 1 + hy, gxx = x0 - 1 + hx;
            okg[k] = gz >= 0 && gz < D && gy >= 0 && gy < H && gxx >= 0 && gxx < W;
            rg[k][0] = rg[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (okg[k]) {
                const float* src = p.x + ((size_t)((n * D + gz) * H + gy) * W + gxx) * Cin + ci0 + 8 * q;
                rg[k][0] = u3d_ldq(src);
                rg[k][1] = u3d_ldq(src + 4);
            }
        }
        rd[0] = rd[1] = f32x4{0.f, 0.f, 0.f, 0.f};
        okd = false;
        if (t < DITEMS) {
            const int q = t & 3, pix = t >> 2;
            const int zi = z0 + (pix >> 6), yi = y0 + ((pix >> 4) & 3), xi = x0 + (pix & 15);
            okd = zi < D && yi < H && xi < W;
            if (okd) {
                const float* src = p.dz + ((size_t)((n * D + zi) * H + yi) * W + xi) * Cout + co0 + 8 * q;
                rd[0] = u3d_ldq(src);
                rd[1] = u3d_ldq(src + 4);
            }
        }
    };
    auto store_tile = [&](bool neg) {
        wf_bf16x8 oh, om, ol;
#pragma unroll
        for (int k = 0; k < GIT; ++k) {
            const int item = t + THREADS * k;
            const float* aff = (aff_n != nullptr && okg[k]) ? aff_n + (ci0 + 8 * (item & 3)) * 2 : nullptr;
            wf_split8(rg[k][0], rg[k][1], aff, okg[k], false, oh, om, ol);
            char* const dst = gl + (item >> 2) * PP + 16 * (item & 3);
            *reinterpret_cast<wf_bf16x8*>(dst) = oh;
            *reinterpret_cast<wf_bf16x8*>(dst + G_PART) = om;
            *reinterpret_cast<wf_bf16x8*>(dst + 2 * G_PART) = ol;
        }
        if (t < DITEMS) {
            wf_split8(rd[0], rd[1], nullptr, okd, neg, oh, om, ol);
            char* const dst = dzl + (t >> 2) * PP + 16 * (t & 3);
            *reinterpret_cast<wf_bf16x8*>(dst) = oh;
            *reinterpret_cast<wf_bf16x8*>(dst + D_PART) = om;
            *reinterpret_cast<wf_bf16x8*>(dst + 2 * D_PART) = ol;
        }
    };
    load_tile(tile0);
    for (int tile = tile0; tile < tile1; ++tile) {
        const bool neg = ((tile - tile0) & 1) != 0;  // dz carries (-1)^(tile - tile0): see the header comment
        store_tile(neg);
        __syncthreads();
        if (tile + 1 < tile1) load_tile(tile + 1);
        // wave (kz, ky): the 8 rows of dz, one 16-voxel row per K step; tap (kz, ky, kx) pairs dz voxel (pz, py, px) with halo voxel
        // (pz + kz, py + ky, px + kx).  One kx at a time: its chain of 48 MFMAs runs in ONE accumulator and is closed into tot[kx]
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 2
            for (int row = 0; row < TZ * TY; ++row) {
                const int pz = row >> 2, py = row & 3;
                wf_bf16x8 a[3], g[3];  // [part]
                const char* const ab = dzl + row * TX * PP + lane_off;
                const char* const gb = gl + (((pz + kz) * HY + py + ky) * HX + kx) * PP + lane_off;
#pragma unroll
                for (int pa = 0; pa < 3; ++pa) a[pa] = wf_tr_frag(ab + pa * D_PART);
#pragma unroll
                for (int pb = 0; pb < 3; ++pb) g[pb] = wf_tr_frag(gb + pb * G_PART);
                // the six product classes, smallest first
#pragma unroll
                for (int cls = 0; cls < 6; ++cls) {
                    constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA[cls]], g[PB[cls]], acc, 0, 0, 0);
                }
            }
            // close the chain: tot += (-1)^(tile - tile0) * acc
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[kx][r] = neg ? tot[kx][r] - acc[r] : tot[kx][r] + acc[r];
        }
        __syncthreads();
    }

    // ---- this block's cell of its slot [tap][Cout][Cin]: register r = output channel (r & 3) + 8 (r >> 2) + 4h, lane column = ci
    const size_t mat = (size_t)Cout * Cin;
    float* const dst = p.ws + (size_t)split * 27 * mat;
    const int ci = ci0 + i32;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            dst[(size_t)((kz * 3 + ky) * 3 + kx) * mat + (size_t)co * Cin + ci] = tot[kx][r];
        }
}

// dw[(co * stride + ci) * 27 + tap] = the slots' [tap][co][ci] added: thread (e, q) adds the q-th of four contiguous slot ranges in slot
// order, thread (e, 0) adds the four in order.  64 elements per block.
__global__ __launch_bounds__(256) void wf_reduce_kernel(const float* __restrict__ ws, int nsplit, int Cin, long long mat, int stride,
                                                        float* __restrict__ dw) {
    __shared__ float part[wf::RED_PARTS][64];
    const long long total = 27 * mat;
    const int e = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int per = (nsplit + wf::RED_PARTS - 1) / wf::RED_PARTS;
    const int s0 = q * per, s1 = min(nsplit, s0 + per);
    for (long long base = (long long)blockIdx.x * 64; base < total; base += (long long)gridDim.x * 64) {
        const long long i = base + e;
        float v = 0.f;
        if (i < total) {
            const float* m = ws + i;
#pragma unroll 8
            for (int s = s0; s < s1; ++s) v += m[(size_t)s * total];
        }
        part[q][e] = v;
        __syncthreads();
        if (q == 0 && i < total) {
            const float sum = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
            const int tap = (int)(i / mat);
            const long long cc = i - tap * mat;
            const long long co = cc / Cin, ci = cc - co * Cin;
            dw[(co * stride + ci) * 27 + tap] = sum;
        }
        __syncthreads();
    }
}

struct WfPlan {
    int tz, ty, tx, ncob, ncib, ntiles, tps, nsplit;
};

// one block per CU over the launch (9 waves, 107520 bytes of LDS: one block is resident per CU); ONE function for the launcher and the
// workspace size.  max_slots > 0: no more splits than that many workspace slots hold (the launcher passes what it was given, so a
// workspace sized on another device — other CU count — still runs, on as many splits as it holds)
WfPlan wf_plan(int device, int N, int D, int H, int W, int Cin, int Cout, long long max_slots = 0) {
    WfPlan pl;
    pl.tz = (int)wf_cdiv(D, wf::TZ);
    pl.ty = (int)wf_cdiv(H, wf::TY);
    pl.tx = (int)wf_cdiv(W, wf::TX);
    pl.ncob = Cout / 32;
    pl.ncib = Cin / 32;
    pl.ntiles = N * pl.tz * pl.ty * pl.tx;
    const long long cells = (long long)pl.ncob * pl.ncib;
    const long long target = wf_cu_count(device);
    long long ns = std::max<long long>(1, std::min<long long>(pl.ntiles, wf_cdiv(target, cells)));
    if (max_slots > 0) ns = std::min(ns, max_slots);
    pl.tps = (int)wf_cdiv(pl.ntiles, ns);
    pl.nsplit = (int)wf_cdiv(pl.ntiles, pl.tps);
    return pl;
}

}  // namespace

extern "C" int u3d_conv3d_wgrad_f32s_supported(int Cin, int Cout) { return wf_ok(Cin, Cout) ? 1 : 0; }

extern "C" long long u3d_wgrad_f32s_workspace_floats(int N, int D, int H, int W, int Cin, int Cout) {
    if (!wf_ok(Cin, Cout) || !wf_dims_ok(N, D, H, W, Cin, Cout)) return 0;
    return (long long)wf_plan(wf_current_device(), N, D, H, W, Cin, Cout).nsplit * 27 * Cin * Cout;
}

extern "C" int u3d_conv3d_wgrad_f32s(int device, u3d_stream_t stream, const float* x, const float* affine, const float* dz, float* dw,
                                     int dw_cin_stride, int N, int D, int H, int W, int Cin, int Cout, float* workspace,
                                     long long workspace_floats) {
    U3D_ENTER(device);
    U3D_REQUIRE(wf_ok(Cin, Cout), "u3d_conv3d_wgrad_f32s: (%d -> %d) channels are outside the split weight gradient's envelope (both %% 32)",
                Cin, Cout);
    U3D_REQUIRE(x && dz && dw && workspace, "u3d_conv3d_wgrad_f32s: bad argument (the workspace is always needed)");
    U3D_REQUIRE(wf_dims_ok(N, D, H, W, Cin, Cout), "u3d_conv3d_wgrad_f32s: bad sizes (the voxel count must be < 2^31)");
    U3D_REQUIRE(dw_cin_stride >= Cin, "u3d_conv3d_wgrad_f32s: dw_cin_stride %d is below Cin %d", dw_cin_stride, Cin);
    U3D_REQUIRE(wf_aligned(x) && wf_aligned(affine) && wf_aligned(dz) && wf_aligned(workspace),
                "u3d_conv3d_wgrad_f32s: pointers must be 16-byte aligned");
    const long long slot = (long long)27 * Cin * Cout;
    U3D_REQUIRE(workspace_floats >= slot, "u3d_conv3d_wgrad_f32s: workspace too small (%lld floats; one slot is %lld)", workspace_floats, slot);
    const WfPlan pl = wf_plan(device, N, D, H, W, Cin, Cout, workspace_floats / slot);
    WfParams p = {};
    p.x = x;
    p.affine = affine;
    p.dz = dz;
    p.ws = workspace;
    p.N = N, p.D = D, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout;
    p.tz = pl.tz, p.ty = pl.ty, p.tx = pl.tx, p.ncob = pl.ncob, p.ncib = pl.ncib, p.ntiles = pl.ntiles, p.tps = pl.tps;
    const long long blocks = (long long)pl.nsplit * pl.ncob * pl.ncib;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_conv3d_wgrad_f32s: grid too large");
    U3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&wf_wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, wf::LDS_BYTES));
    hipLaunchKernelGGL(wf_wgrad_kernel, dim3((unsigned)blocks), dim3(wf::THREADS), wf::LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    long long rb = wf_cdiv(slot, 64);
    if (rb > 8192) rb = 8192;
    hipLaunchKernelGGL(wf_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace, pl.nsplit, Cin, slot / 27,
                       dw_cin_stride, dw);
    U3D_LAUNCH_CHECK();
    return 0;
}

// the 3x3 Conv2d kernels of a UNet2D in fp32_split (`native_2d_fp32_split`): device code and entry points, on this file's helpers
#include "u3d_conv2d_f32s.h"
