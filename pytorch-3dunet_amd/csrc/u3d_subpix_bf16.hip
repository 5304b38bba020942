// u3d_subpix_bf16.hip — sub-pixel decoder convolutions of a UNet3D on the bf16 MFMA (`bf16_subpixel: true`): the bf16 twins of
// u3d_subpixel_conv_fwd / _dgrad_reps / _wgrad of csrc/u3d_subpix.hip on v_mfma_f32_32x32x16_bf16, and the 3-D twins of the
// u3d_subpixel2d_*_bf16 kernels of csrc/u3d_conv2d_bf16.hip.  The upsampled half of cat(skip, nearest2x(low)) under a 3x3x3 convolution:
// an output voxel of parity p reads, per axis, only the two low-res voxels j + p - 1 + e (e = 0, 1) — p = 0: {t0}, {t1 + t2}; p = 1:
// {t0 + t1}, {t2} — so each of the 8 parity classes is a 2x2x2 convolution over the low-res grid, 8/27 of the multiply-adds, and the data
// gradient lands at low resolution with the children sum folded in.  Tensors in HBM are fp32 NDHWC, accumulation is fp32.
// Rounding points: the pre-summed taps are added in fp32 from the fp32 master weight (in ascending (tz, ty, tx) order) and rounded ONCE to
// bf16, nearest even, by the pack kernel; activations and dz are rounded once while staged to LDS, after the fp32 affine fmaf(x, a, b);
// zero padding applies after the affine and stays exactly 0 (sp3b_stage8).  Not bit-equal to the 27-tap bf16 kernels on the written-out
// concat in forward and data gradient (those round every tap); the weight gradient multiplies the same bf16 operands.
//
// Forward (subpix3d_fwd_bf16_kernel): a block of 4 waves owns 4 x 4 x 8 LOW-RES voxels x 32 output channels; wave w owns z-plane w as one
// M-tile (row r -> (y = r & 3, x = r >> 2), the M-tile of csrc/u3d_bf16.hip).  The 6 x 6 x 10 halo of a 16-channel chunk is staged in that
// file's record layout — two channel-half planes [kh][hz][hy][hx pad HS = 12] of 16-byte records, so its bank-conflict argument carries
// over unchanged — double-buffered, and serves all eight classes: 27 A-fragment positions, 64 MFMAs per M-tile and n-tile (class (a, b, c)
// takes halo offsets (a + u, b + v, c + w)).  8 classes x 16 = 128 accumulator registers per wave, two blocks per CU.  out (N, 2D1, 2H1,
// 2W1, Cout) receives the plain partial sums: the skip half joins through u3d_conv3d_bf16_ex(residual = out).  No split-K: a grid of fewer
// blocks than CUs stays that small.
//
// Data gradient (subpix3d_dgrad_bf16_kernel): dlow[i] = sum over the 4 x 4 x 4 stride-2 gather dz[2i - 1 + r], per axis r = 0..3 carrying
// t2, t1 + t2, t0 + t1, t0.  The 10 x 10 x 18 dz region of a 4 x 4 x 8 dlow tile is read in raster order (64 contiguous bytes per voxel,
// rows contiguous in x) and DE-INTERLEAVED on the way into LDS into its eight parity planes (5 x 5 x 9 each, rows padded to HS): gather
// (rz, ry, rx) reads plane ((rz + 1) & 1, (ry + 1) & 1, (rx + 1) & 1) at offset (rz >> 1, ry >> 1, rx >> 1) with the forward's unit-stride
// fragment pattern.  One 75 KB buffer, the next chunk in flight in registers.  The epilogue adds (sum dlow, sum dlow * x_low) per block
// into gstats, replica row block % reps; dlow itself does not depend on reps.
//
// Weight gradient (subpix3d_wgrad_bf16_kernel): the 64 (class, tap half) 32 x 32 matrices M[a, b, c, u, v, w][co][ci] = sum_i dz[2i + (a, b,
// c), co] * g[i + (a, b, c) - 1 + (u, v, w), ci] over 2 x 4 x 16 low-res tiles; 8 waves, wave = class (8 accumulators), its dz plane and the
// shared 4 x 6 x 18 low-res halo sit in LDS as [voxel][32 channels] and are fetched with ds_read_b64_tr_b16.  Every block writes its 64
// matrices to its workspace slot; subpix3d_wgrad_bf16_fold_kernel folds them into the 27 taps (8 matrices per tap) and adds the slots in
// slot order: no atomics, the same inputs give the same bits.
#include "u3d_common.h"

#include <algorithm>

typedef __bf16 sp3b_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 sp3b_bf16x4 __attribute__((ext_vector_type(4)));
typedef short sp3b_s16x4 __attribute__((ext_vector_type(4)));
typedef short sp3b_s16x8 __attribute__((ext_vector_type(8)));

namespace {

namespace sp3b {
constexpr int HS = 12;                             // halo row stride in 16-byte records (csrc/u3d_bf16.hip)
constexpr int TZ = 4, TY = 4, TX = 8;              // low-res tile: wave = z-plane, M-tile = 4 y x 8 x
// forward
constexpr int FZ = TZ + 2, FY = TY + 2, FX = TX + 2;  // 6 x 6 x 10 halo
constexpr int FPLANE = FZ * FY * HS * 16 + 64;     // 6976 bytes per channel-half plane (+64: the two planes' writes land on different banks)
constexpr int FBUF = 2 * FPLANE;                   // 13952
constexpr int FITEMS = FZ * FY * FX * 2;           // 720 (voxel, channel octet) items per chunk
constexpr int FNIT = (FITEMS + 255) / 256;         // 3
constexpr int F_LDS_BYTES = 2 * FBUF;              // 27904 (double-buffered)
// data gradient: eight parity planes
constexpr int PZ = TZ + 1, PY = TY + 1, PX = TX + 1;  // 5 x 5 x 9 voxels per plane
constexpr int DPL = PZ * PY * HS * 16;             // 4800 bytes per (plane, channel half)
constexpr int DKH = 8 * DPL + 64;                  // 38464 bytes per channel half
constexpr int RZ = 2 * TZ + 2, RY = 2 * TY + 2, RX = 2 * TX + 2;  // 10 x 10 x 18 dz region, raster order
constexpr int DITEMS = RZ * RY * RX * 2;           // 3600
constexpr int DNIT = (DITEMS + 255) / 256;         // 15
constexpr int D_LDS_BYTES = 2 * DKH;               // 76928 (the final [4][32][2] float reduction reuses the first 1024)
// weight gradient
constexpr int WTZ = 2, WTY = 4, WTX = 16;          // low-res tile: 8 rows of 16 x
constexpr int WHZ = WTZ + 2, WHY = WTY + 2, WHX = WTX + 2;  // 4 x 6 x 18 halo
constexpr int WPP = 64;                            // bytes per staged voxel (32 bf16)
constexpr int WVOX = WTZ * WTY * WTX;              // 128
constexpr int W_G = 0;                             // [4 * 6 * 18][32] bf16
constexpr int W_DZ = WHZ * WHY * WHX * WPP;        // 27648: [8 planes][128][32] bf16
constexpr int W_LDS_BYTES = W_DZ + 8 * WVOX * WPP; // 93184
constexpr int W_GITEMS = WHZ * WHY * WHX * 4;      // 1728 (voxel, octet) halo items
constexpr int W_GIT = (W_GITEMS + 511) / 512;      // 4
constexpr int W_DIT = 8 * WVOX * 4 / 512;          // 8 dz items per thread
constexpr int W_DB = 4;                            // dz items staged per batch

// the 64 (class, tap half) products of one chunk in halo-position order: q = (4a + 2b + c) * 8 + 4u + 2v + w reads halo offset
// (a + u, b + v, c + w)
struct Seq {
    int q[64], pos[64];
};
constexpr Seq make_seq() {
    Seq s{};
    int n = 0;
    for (int dz = 0; dz < 3; ++dz)
        for (int dy = 0; dy < 3; ++dy)
            for (int dx = 0; dx < 3; ++dx)
                for (int a = 0; a < 2; ++a)
                    for (int b = 0; b < 2; ++b)
                        for (int c = 0; c < 2; ++c) {
                            const int u = dz - a, v = dy - b, w = dx - c;
                            if (u < 0 || u > 1 || v < 0 || v > 1 || w < 0 || w > 1) continue;
                            s.q[n] = (4 * a + 2 * b + c) * 8 + 4 * u + 2 * v + w;
                            s.pos[n] = (dz * 3 + dy) * 3 + dx;
                            ++n;
                        }
    return s;
}
}  // namespace sp3b

inline long long sp3b_cdiv(long long a, long long b) { return (a + b - 1) / b; }
inline bool sp3b_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool sp3b_ok(int C1, int Cout) { return C1 > 0 && Cout > 0 && C1 % 32 == 0 && Cout % 32 == 0; }
inline bool sp3b_dims_ok(int N, int D1, int H1, int W1, int C1, int Cout) {
    return N > 0 && D1 > 0 && H1 > 0 && W1 > 0 && (long long)N * 8 * D1 * H1 * W1 < (1ll << 31) && (long long)64 * C1 * Cout < (1ll << 31);
}

int sp3b_cu_count(int device) {
    static int cached[64] = {0};
    if (device >= 0 && device < 64 && cached[device] > 0) return cached[device];
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
    if (device >= 0 && device < 64) cached[device] = n;
    return n;
}
// the > 64 KB dynamic-LDS opt-in of a kernel, once per device and process
template <typename K>
hipError_t sp3b_allow_lds(K kernel, int bytes, int device, bool (&done)[64]) {
    if (device >= 0 && device < 64 && done[device]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && device >= 0 && device < 64) done[device] = true;
    return e;
}

int sp3b_current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return dev;
}

// 8 staged channels: affine in fp32 (one fused multiply-add per element), ONE rounding to bf16 (nearest even), zero outside the volume
__device__ __forceinline__ sp3b_bf16x8 sp3b_stage8(const f32x4& lo, const f32x4& hi, const float* aff, bool ok) {
    f32x4 v0 = lo, v1 = hi;
    if (aff != nullptr) {
        const f32x4 q0 = u3d_ldq(aff), q1 = u3d_ldq(aff + 4), q2 = u3d_ldq(aff + 8), q3 = u3d_ldq(aff + 12);  // (a, b) pairs
        v0 = f32x4{fmaf(lo[0], q0[0], q0[1]), fmaf(lo[1], q0[2], q0[3]), fmaf(lo[2], q1[0], q1[1]), fmaf(lo[3], q1[2], q1[3])};
        v1 = f32x4{fmaf(hi[0], q2[0], q2[1]), fmaf(hi[1], q2[2], q2[3]), fmaf(hi[2], q3[0], q3[1]), fmaf(hi[3], q3[2], q3[3])};
    }
    if (!ok) v0 = v1 = f32x4{0.f, 0.f, 0.f, 0.f};  // padding stays exactly 0
    const sp3b_bf16x4 b0 = __builtin_convertvector(v0, sp3b_bf16x4), b1 = __builtin_convertvector(v1, sp3b_bf16x4);
    return __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ds_read_b64_tr_b16 x 2: lane l receives channel (l & 31) of the 8 voxels 8 * (l >> 5) .. + 7 of a [voxel][32 channels] run
__device__ __forceinline__ sp3b_bf16x8 sp3b_tr_frag(const char* lds_addr) {
    const sp3b_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) sp3b_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)lds_addr);
    const sp3b_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) sp3b_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)(lds_addr + 4 * sp3b::WPP));
    const sp3b_s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(sp3b_bf16x8, v);
}

// the taps of the 3-tap axis summed into tap half e of parity p (forward) and into gather row r (data gradient): [t0, t1], t0 <= t1
__device__ __forceinline__ void sp3b_taps_fwd(int p, int e, int& t0, int& t1) {
    t0 = (p == 0) ? (e == 0 ? 0 : 1) : (e == 0 ? 0 : 2);
    t1 = (p == 0) ? (e == 0 ? 0 : 2) : (e == 0 ? 1 : 2);
}
__device__ __forceinline__ void sp3b_taps_dgrad(int r, int& t0, int& t1) {
    t0 = r == 0 ? 2 : (r == 1 ? 1 : 0);
    t1 = r == 0 ? 2 : (r == 1 ? 2 : (r == 2 ? 1 : 0));
}

// images [K / 16 chunk][64][n-tile][lane][8] of B[k][n], the fragment layout of pack_weights_bf16_kernel; w (Cout, cs, 3, 3, 3), channels
// from coff.  dgrad == 0: entry q = (4a + 2b + c) * 8 + 4u + 2v + w, B[k = ci][n = co]; dgrad == 1: entry 16 rz + 4 ry + rx, B[k = co][n =
// ci].  The taps are added in fp32 in ascending (tz, ty, tx) order, then rounded once.
__global__ void pack_subpix3d_bf16_kernel(const float* __restrict__ w, int cs, int coff, int dgrad, int ntg, long long total,
                                          __bf16* __restrict__ packed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        long long r = i >> 9;
        const int nt = (int)(r % ntg);
        r /= ntg;
        const int q = (int)(r % 64);
        const int chunk = (int)(r / 64);
        const int k = chunk * 16 + 8 * (lane >> 5) + j;
        const int nn = nt * 32 + (lane & 31);
        int z0, z1, y0, y1, x0, x1;
        if (dgrad == 0) {
            sp3b_taps_fwd(q >> 5, (q >> 2) & 1, z0, z1);
            sp3b_taps_fwd((q >> 4) & 1, (q >> 1) & 1, y0, y1);
            sp3b_taps_fwd((q >> 3) & 1, q & 1, x0, x1);
        } else {
            sp3b_taps_dgrad(q >> 4, z0, z1);
            sp3b_taps_dgrad((q >> 2) & 3, y0, y1);
            sp3b_taps_dgrad(q & 3, x0, x1);
        }
        const float* base = dgrad == 0 ? w + ((size_t)nn * cs + coff + k) * 27 : w + ((size_t)k * cs + coff + nn) * 27;
        float v = 0.f;
        for (int tz = z0; tz <= z1; tz += (z1 > z0 ? z1 - z0 : 1))
            for (int ty = y0; ty <= y1; ty += (y1 > y0 ? y1 - y0 : 1))
                for (int tx = x0; tx <= x1; tx += (x1 > x0 ? x1 - x0 : 1)) v += base[(tz * 3 + ty) * 3 + tx];
        packed[i] = (__bf16)v;
    }
}

struct Subpix3dBf16Params {
    const float* src;     // forward: low (N,D1,H1,W1,C1); data gradient: dz (N,2D1,2H1,2W1,Cout)
    const float* affine;  // forward: (a, b) rows of the C1 channels, sample n at affine + n * astride; or null
    long long astride;
    const sp3b_bf16x8* wp;
    const float* x_low;   // data gradient: (N,D1,H1,W1,C1) for gstats, or null
    float* out;           // forward: out (N,2D1,2H1,2W1,Cout); data gradient: dlow (N,D1,H1,W1,C1)
    double* gstats;
    int N, D1, H1, W1, C1, Cout;
    int nchunks, ntg, tz, ty, tx, reps;
};

__global__ __launch_bounds__(256, 2) void subpix3d_fwd_bf16_kernel(const Subpix3dBf16Params p) {
    using namespace sp3b;
    extern __shared__ __attribute__((aligned(16))) char lds_sp3f[];
    char* const lds = lds_sp3f;
    const int t = threadIdx.x;
    const int l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int tile = blockIdx.x;
    const int cb = tile % p.ntg;
    tile /= p.ntg;
    const int txi = tile % p.tx;
    tile /= p.tx;
    const int tyi = tile % p.ty;
    tile /= p.ty;
    const int tzi = tile % p.tz;
    const int n = tile / p.tz;
    const int z0 = tzi * TZ, y0 = tyi * TY, x0 = txi * TX;
    const int D1 = p.D1, H1 = p.H1, W1 = p.W1, C1 = p.C1;

    int ldsoff[FNIT], gpix[FNIT];  // gpix < 0: outside the volume (stays exactly 0)
#pragma unroll
    for (int it = 0; it < FNIT; ++it) {
        const int item = t + 256 * it;
        const bool in = item < FITEMS;
        const int q = item & 1;
        int pix = item >> 1;
        const int hx = pix % FX;
        pix /= FX;
        const int hy = pix % FY;
        const int hz = pix / FY;
        const int gz = z0 - 1 + hz, gy = y0 - 1 + hy, gxx = x0 - 1 + hx;
        const bool ok = in && gz >= 0 && gz < D1 && gy >= 0 && gy < H1 && gxx >= 0 && gxx < W1;
        ldsoff[it] = in ? q * FPLANE + ((hz * FY + hy) * HS + hx) * 16 : -1;
        gpix[it] = ok ? ((n * D1 + gz) * H1 + gy) * W1 + gxx : -1;
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
            *reinterpret_cast<sp3b_bf16x8*>(buf + ldsoff[it]) = sp3b_stage8(raw[it][0], raw[it][1], aff, ok);
        }
    };

    f32x16 acc[8];  // [parity class 4a + 2b + c]
#pragma unroll
    for (int cls = 0; cls < 8; ++cls)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cls][r] = 0.f;

    // A-fragment base: lane (i32, h) owns low-res voxel (w, i32 & 3, i32 >> 2) of the tile, channels 8h .. 8h + 7; halo offset (dz, dy, dx)
    // of it is halo voxel (+dz, +dy, +dx)
    const int abase = h * FPLANE + ((w * FY + (i32 & 3)) * HS + (i32 >> 2)) * 16;
    auto bidx = [&](int c, int q) -> long long { return ((long long)(c * 64 + q) * p.ntg + cb) * 64 + l; };
    constexpr Seq SQ = make_seq();

    load_chunk(0);
    store_chunk(0, lds);
    __syncthreads();
    for (int c = 0; c < p.nchunks; ++c) {
        const char* cur = lds + (c & 1) * FBUF;
        if (c + 1 < p.nchunks) load_chunk(c + 1);  // in flight during the MFMAs
        sp3b_bf16x8 bq = p.wp[bidx(c, SQ.q[0])], bn = bq;
        sp3b_bf16x8 a;
#pragma unroll
        for (int s = 0; s < 64; ++s) {
            if (s + 1 < 64) bn = p.wp[bidx(c, SQ.q[s + 1])];
            if (s == 0 || SQ.pos[s] != SQ.pos[s - 1]) {
                const int dz = SQ.pos[s] / 9, dy = (SQ.pos[s] / 3) % 3, dx = SQ.pos[s] % 3;
                a = *reinterpret_cast<const sp3b_bf16x8*>(cur + abase + ((dz * FY + dy) * HS + dx) * 16);
            }
            acc[SQ.q[s] >> 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bq, acc[SQ.q[s] >> 3], 0, 0, 0);
            bq = bn;
        }
        if (c + 1 < p.nchunks) store_chunk(c + 1, lds + ((c + 1) & 1) * FBUF);  // (that buffer was last read in chunk c - 1)
        __syncthreads();
    }

    // ---- lane column = output channel, register r = M row (r & 3) + 8 (r >> 2) + 4h = (y = row & 3, x = row >> 2); class (a, b, c) of
    // low-res (i, j, k) is out[2i + a][2j + b][2k + c]
    const int co = cb * 32 + i32;
    const int Ho = 2 * H1, Wo = 2 * W1;
    const int zi = z0 + w;
    if (zi >= D1) return;
#pragma unroll
    for (int cls = 0; cls < 8; ++cls)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int yi = y0 + (row & 3), xi = x0 + (row >> 2);
            if (yi >= H1 || xi >= W1) continue;
            const size_t vox = ((size_t)(n * 2 * D1 + 2 * zi + (cls >> 2)) * Ho + 2 * yi + ((cls >> 1) & 1)) * Wo + 2 * xi + (cls & 1);
            p.out[vox * p.Cout + co] = acc[cls][r];
        }
}

__global__ __launch_bounds__(256, 2) void subpix3d_dgrad_bf16_kernel(const Subpix3dBf16Params p) {
    using namespace sp3b;
    extern __shared__ __attribute__((aligned(16))) char lds_sp3d[];
    char* const lds = lds_sp3d;
    const int t = threadIdx.x;
    const int l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int tile = blockIdx.x;
    const int cb = tile % p.ntg;
    tile /= p.ntg;
    const int txi = tile % p.tx;
    tile /= p.tx;
    const int tyi = tile % p.ty;
    tile /= p.ty;
    const int tzi = tile % p.tz;
    const int n = tile / p.tz;
    const int z0 = tzi * TZ, y0 = tyi * TY, x0 = txi * TX;
    const int D1 = p.D1, H1 = p.H1, W1 = p.W1, Dd = 2 * p.D1, Hd = 2 * p.H1, Wd = 2 * p.W1, K = p.Cout;  // the contraction runs over Cout

    // item = (region voxel (rz, ry, rx) in raster order, channel octet q): dz voxel (2 z0 - 1 + rz, ...) goes to plane ((rz + 1) & 1, ...)
    // at plane voxel (rz >> 1, ...)
    int ldsoff[DNIT], gpix[DNIT];  // gpix < 0: outside dz (zero)
#pragma unroll
    for (int it = 0; it < DNIT; ++it) {
        const int item = t + 256 * it;
        const bool in = item < DITEMS;
        const int q = item & 1;
        int pix = item >> 1;
        const int rx = pix % RX;
        pix /= RX;
        const int ry = pix % RY;
        const int rz = pix / RY;
        const int gz = 2 * z0 - 1 + rz, gy = 2 * y0 - 1 + ry, gxx = 2 * x0 - 1 + rx;
        const bool ok = in && gz >= 0 && gz < Dd && gy >= 0 && gy < Hd && gxx >= 0 && gxx < Wd;
        const int pl = 4 * ((rz + 1) & 1) + 2 * ((ry + 1) & 1) + ((rx + 1) & 1);
        ldsoff[it] = in ? q * DKH + pl * DPL + (((rz >> 1) * PY + (ry >> 1)) * HS + (rx >> 1)) * 16 : -1;
        gpix[it] = ok ? ((n * Dd + gz) * Hd + gy) * Wd + gxx : -1;
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
                *reinterpret_cast<sp3b_bf16x8*>(lds + ldsoff[it]) = sp3b_stage8(raw[it][0], raw[it][1], nullptr, gpix[it] >= 0);
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    // lane (i32, h) owns dlow voxel (w, i32 & 3, i32 >> 2) of the tile
    const int abase = h * DKH + ((w * PY + (i32 & 3)) * HS + (i32 >> 2)) * 16;
    auto bidx = [&](int c, int q) -> long long { return ((long long)(c * 64 + q) * p.ntg + cb) * 64 + l; };

    load_chunk(0);
    store_chunk();
    __syncthreads();
    for (int c = 0; c < p.nchunks; ++c) {
        if (c + 1 < p.nchunks) load_chunk(c + 1);  // in flight during the MFMAs
        sp3b_bf16x8 bq = p.wp[bidx(c, 0)], bn = bq;
#pragma unroll
        for (int q = 0; q < 64; ++q) {
            const int rz = q >> 4, ry = (q >> 2) & 3, rx = q & 3;
            if (q + 1 < 64) bn = p.wp[bidx(c, q + 1)];
            const int toff = (4 * ((rz + 1) & 1) + 2 * ((ry + 1) & 1) + ((rx + 1) & 1)) * DPL + (((rz >> 1) * PY + (ry >> 1)) * HS + (rx >> 1)) * 16;
            const sp3b_bf16x8 a = *reinterpret_cast<const sp3b_bf16x8*>(lds + abase + toff);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bq, acc, 0, 0, 0);
            bq = bn;
        }
        __syncthreads();  // every wave is done reading the one buffer
        if (c + 1 < p.nchunks) {
            store_chunk();
            __syncthreads();
        }
    }

    const int ci = cb * 32 + i32;
    const int zi = z0 + w;
    float s0 = 0.f, s1 = 0.f;
    if (zi < D1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int yi = y0 + (row & 3), xi = x0 + (row >> 2);
            if (yi >= H1 || xi >= W1) continue;
            const size_t o = (((size_t)(n * D1 + zi) * H1 + yi) * W1 + xi) * p.C1 + ci;
            const float v = acc[r];
            p.out[o] = v;
            if (p.gstats != nullptr) {
                s0 += v;
                s1 += v * p.x_low[o];
            }
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

struct Subpix3dWgradBf16Params {
    const float* low;     // (N,D1,H1,W1,C1)
    const float* affine;  // rows of the C1 channels, sample n at affine + n * astride; or null
    long long astride;
    const float* dz;      // (N,2D1,2H1,2W1,Cout)
    float* ws;            // [nsplit][64][Cout][C1]
    int N, D1, H1, W1, C1, Cout;
    int tz, ty, tx, ncob, ncib, ntiles, tps;
};

__global__ __launch_bounds__(512, 1) void subpix3d_wgrad_bf16_kernel(const Subpix3dWgradBf16Params p) {
    using namespace sp3b;
    extern __shared__ __attribute__((aligned(16))) char lds_sp3w[];
    char* const lds = lds_sp3w;
    const int t = threadIdx.x, l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int b = blockIdx.x;
    const int cib = b % p.ncib;
    b /= p.ncib;
    const int cob = b % p.ncob;
    const int split = b / p.ncob;
    const int ci0 = cib * 32, co0 = cob * 32;
    const int tile0 = split * p.tps, tile1 = min(p.ntiles, tile0 + p.tps);
    const int D1 = p.D1, H1 = p.H1, W1 = p.W1, Dd = 2 * p.D1, Hd = 2 * p.H1, Wd = 2 * p.W1, C1 = p.C1, Cout = p.Cout;
    char* const gl = lds + W_G;
    char* const dzl = lds + W_DZ;
    const int pa = w >> 2, pb = (w >> 1) & 1, pc = w & 1;  // this wave's parity class

    f32x16 acc[8];  // [tap half 4u + 2v + w]
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    // transposed-read lane offset, as conv2d_wgrad_bf16_kernel: lane l receives channel (l & 31) of the 8 voxels 8 * (l >> 5) .. + 7
    const int g4 = l >> 4, sidx = l & 15;
    const int lane_off = (8 * (g4 >> 1) + (sidx >> 2)) * WPP + (16 * (g4 & 1) + 4 * (sidx & 3)) * 2;

    for (int tile = tile0; tile < tile1; ++tile) {
        int tt = tile;
        const int txi = tt % p.tx;
        tt /= p.tx;
        const int tyi = tt % p.ty;
        tt /= p.ty;
        const int tzi = tt % p.tz;
        const int n = tt / p.tz;
        const int z0 = tzi * WTZ, y0 = tyi * WTY, x0 = txi * WTX;
        const float* const aff_n = p.affine != nullptr ? p.affine + (size_t)n * p.astride : nullptr;
        // stage g (4 x 6 x 18 low-res halo from (z0 - 1, y0 - 1, x0 - 1), 32 channels from ci0, affine, zero padding) ...
        {
            f32x4 rg[W_GIT][2];
            bool okg[W_GIT];
#pragma unroll
            for (int k = 0; k < W_GIT; ++k) {
                const int item = t + 512 * k;
                const int q = item & 3;
                int pix = item >> 2;
                const int hx = pix % WHX;
                pix /= WHX;
                const int hy = pix % WHY;
                const int hz = pix / WHY;
                const int gz = z0 - 1 + hz, gy = y0 - 1 + hy, gxx = x0 - 1 + hx;
                okg[k] = item < W_GITEMS && gz >= 0 && gz < D1 && gy >= 0 && gy < H1 && gxx >= 0 && gxx < W1;
                rg[k][0] = rg[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (okg[k]) {
                    const float* src = p.low + ((size_t)((n * D1 + gz) * H1 + gy) * W1 + gxx) * C1 + ci0 + 8 * q;
                    rg[k][0] = u3d_ldq(src);
                    rg[k][1] = u3d_ldq(src + 4);
                }
            }
#pragma unroll
            for (int k = 0; k < W_GIT; ++k) {
                const int item = t + 512 * k;
                if (item >= W_GITEMS) continue;
                const float* aff = (aff_n != nullptr && okg[k]) ? aff_n + (ci0 + 8 * (item & 3)) * 2 : nullptr;
                *reinterpret_cast<sp3b_bf16x8*>(gl + (item >> 2) * WPP + 16 * (item & 3)) = sp3b_stage8(rg[k][0], rg[k][1], aff, okg[k]);
            }
        }
        // ... and dz de-interleaved into its eight parity planes (2 x 4 x 16 voxels each, 32 channels from co0): plane (a, b, c), voxel
        // (pz, py, px) is dz[2 (z0 + pz) + a][2 (y0 + py) + b][2 (x0 + px) + c]
        auto stage_dz = [&](int it0) {
            f32x4 rd[W_DB][2];
            bool okd[W_DB];
#pragma unroll
            for (int k = 0; k < W_DB; ++k) {
                const int item = t + 512 * (it0 + k);
                const int q = item & 3, pix = (item >> 2) & (WVOX - 1), pl = item >> 9;
                const int i = z0 + (pix >> 6), j = y0 + ((pix >> 4) & 3), kk = x0 + (pix & 15);
                okd[k] = i < D1 && j < H1 && kk < W1;
                rd[k][0] = rd[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (okd[k]) {
                    const float* src = p.dz + ((size_t)((n * Dd + 2 * i + (pl >> 2)) * Hd + 2 * j + ((pl >> 1) & 1)) * Wd + 2 * kk + (pl & 1)) * Cout +
                                       co0 + 8 * q;
                    rd[k][0] = u3d_ldq(src);
                    rd[k][1] = u3d_ldq(src + 4);
                }
            }
#pragma unroll
            for (int k = 0; k < W_DB; ++k) {
                const int item = t + 512 * (it0 + k);
                *reinterpret_cast<sp3b_bf16x8*>(dzl + (item >> 2) * WPP + 16 * (item & 3)) = sp3b_stage8(rd[k][0], rd[k][1], nullptr, okd[k]);
            }
        };
        for (int it0 = 0; it0 < W_DIT; it0 += W_DB) stage_dz(it0);
        __syncthreads();
        // wave w = class (pa, pb, pc): the 8 rows of its dz plane, one 16-voxel row per k-step; tap half (u, v, ww) pairs dz plane voxel
        // (pz, py, px) with low-res halo voxel (pz + pa + u, py + pb + v, px + pc + ww)
#pragma unroll 2
        for (int row = 0; row < WTZ * WTY; ++row) {
            const int pz = row >> 2, py = row & 3;
            const sp3b_bf16x8 a = sp3b_tr_frag(dzl + (w * WVOX + row * WTX) * WPP + lane_off);
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 2; ++v)
#pragma unroll
                    for (int ww = 0; ww < 2; ++ww) {
                        const sp3b_bf16x8 g = sp3b_tr_frag(gl + (((pz + pa + u) * WHY + py + pb + v) * WHX + pc + ww) * WPP + lane_off);
                        acc[4 * u + 2 * v + ww] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, g, acc[4 * u + 2 * v + ww], 0, 0, 0);
                    }
        }
        __syncthreads();
    }

    // ---- this block's slot: matrix q = 8 w + 4u + 2v + ww, [co][ci]; register r = output channel (r & 3) + 8 (r >> 2) + 4h, lane column = ci
    float* const dst = p.ws + ((size_t)split * 64 + 8 * w) * Cout * C1;
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
            dst[((size_t)k * Cout + co0 + row) * C1 + ci0 + i32] = acc[k][r];
        }
}

// dw[co][ci][kz][ky][kx] = sum over slots in slot order of the 8 matrices that carry the tap: per axis tap 0 <- (p, e) = (0, 0), (1, 0);
// tap 1 <- (0, 1), (1, 0); tap 2 <- (0, 1), (1, 1).  drow = 27 * dw_cin_stride elements per output channel of dw.
__global__ void subpix3d_wgrad_bf16_fold_kernel(const float* __restrict__ ws, int nsplit, int Cout, int C1, float* __restrict__ dw,
                                                long long drow) {
    const long long total = (long long)Cout * C1 * 27;
    const size_t mat = (size_t)Cout * C1;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int tap = (int)(i % 27);
        const long long cc = i / 27;  // co * C1 + ci
        const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        // tap half of the parity-0 and the parity-1 contribution per axis
        const int uz[2] = {kz == 0 ? 0 : 1, kz == 2 ? 1 : 0}, uy[2] = {ky == 0 ? 0 : 1, ky == 2 ? 1 : 0}, ux[2] = {kx == 0 ? 0 : 1, kx == 2 ? 1 : 0};
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) {
            const float* m = ws + (size_t)s * 64 * mat + cc;
            float sv = 0.f;
#pragma unroll
            for (int cls = 0; cls < 8; ++cls) {
                const int a = cls >> 2, b = (cls >> 1) & 1, c = cls & 1;
                sv += m[(size_t)(cls * 8 + 4 * uz[a] + 2 * uy[b] + ux[c]) * mat];
            }
            v += sv;
        }
        dw[(cc / C1) * drow + (cc % C1) * 27 + tap] = v;
    }
}

struct Sp3bWPlan {
    int tz, ty, tx, ncob, ncib, ntiles, tps, nsplit;
};

// one block per CU over the launch (93 KB of LDS and 8 waves of 128 accumulators: one block is resident per CU); ONE function for the
// launcher and the workspace size.  max_slots > 0: no more splits than that many workspace slots hold (the launcher passes what it was
// given, so a workspace sized on another device — other CU count — still runs, on as many splits as it holds)
Sp3bWPlan sp3b_wplan(int device, int N, int D1, int H1, int W1, int C1, int Cout, long long max_slots = 0) {
    Sp3bWPlan pl;
    pl.tz = (int)sp3b_cdiv(D1, sp3b::WTZ);
    pl.ty = (int)sp3b_cdiv(H1, sp3b::WTY);
    pl.tx = (int)sp3b_cdiv(W1, sp3b::WTX);
    pl.ncob = Cout / 32;
    pl.ncib = C1 / 32;
    pl.ntiles = N * pl.tz * pl.ty * pl.tx;
    const long long cells = (long long)pl.ncob * pl.ncib;
    const long long target = sp3b_cu_count(device);
    long long ns = std::max<long long>(1, std::min<long long>(pl.ntiles, sp3b_cdiv(target, cells)));
    if (max_slots > 0) ns = std::min(ns, max_slots);
    pl.tps = (int)sp3b_cdiv(pl.ntiles, ns);
    pl.nsplit = (int)sp3b_cdiv(pl.ntiles, pl.tps);
    return pl;
}

}  // namespace

extern "C" long long u3d_subpixel_bf16_packed_elems(int C1, int Cout, int dgrad) {
    if ((dgrad != 0 && dgrad != 1) || !sp3b_ok(C1, Cout) || (long long)64 * C1 * Cout >= (1ll << 31)) return 0;
    return (long long)64 * C1 * Cout;  // [K / 16][64][Nn / 32][64][8]; the B prefetch never leaves a chunk: no tail padding
}

extern "C" int u3d_pack_subpixel_weights_bf16(int device, u3d_stream_t stream, const float* w, int Cout, int Cin_total, int c_off, int C1,
                                              int dgrad, void* packed) {
    U3D_ENTER(device);
    U3D_REQUIRE(w && packed && (dgrad == 0 || dgrad == 1), "u3d_pack_subpixel_weights_bf16: bad argument");
    U3D_REQUIRE(sp3b_ok(C1, Cout) && (long long)64 * C1 * Cout < (1ll << 31),
                "u3d_pack_subpixel_weights_bf16: (%d -> %d) channels are outside the bf16 sub-pixel envelope (both %% 32)", C1, Cout);
    U3D_REQUIRE(c_off >= 0 && c_off + C1 <= Cin_total, "u3d_pack_subpixel_weights_bf16: channels [%d, %d) do not lie inside a weight of %d "
                "input channels", c_off, c_off + C1, Cin_total);
    U3D_REQUIRE(sp3b_aligned(packed), "u3d_pack_subpixel_weights_bf16: the image must be 16-byte aligned");
    const long long total = (long long)64 * C1 * Cout;
    long long blocks = sp3b_cdiv(total, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_subpix3d_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, Cin_total, c_off, dgrad,
                       (dgrad == 0 ? Cout : C1) / 32, total, reinterpret_cast<__bf16*>(packed));
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_subpixel_conv_fwd_bf16(int device, u3d_stream_t stream, const float* low, const float* affine,
                                          long long affine_sample_stride, const void* packed, float* out, int N, int D1, int H1, int W1,
                                          int C1, int Cout) {
    U3D_ENTER(device);
    U3D_REQUIRE(sp3b_ok(C1, Cout), "u3d_subpixel_conv_fwd_bf16: (%d -> %d) channels are outside the bf16 sub-pixel envelope (both %% 32)", C1,
                Cout);
    U3D_REQUIRE(low && packed && out, "u3d_subpixel_conv_fwd_bf16: bad argument");
    U3D_REQUIRE(sp3b_dims_ok(N, D1, H1, W1, C1, Cout), "u3d_subpixel_conv_fwd_bf16: bad sizes (the output voxel count must be < 2^31)");
    U3D_REQUIRE(sp3b_aligned(low) && sp3b_aligned(affine) && sp3b_aligned(packed) && sp3b_aligned(out) && affine_sample_stride % 4 == 0,
                "u3d_subpixel_conv_fwd_bf16: pointers must be 16-byte aligned");
    Subpix3dBf16Params p = {};
    p.src = low;
    p.affine = affine;
    p.astride = affine_sample_stride;
    p.wp = reinterpret_cast<const sp3b_bf16x8*>(packed);
    p.out = out;
    p.N = N, p.D1 = D1, p.H1 = H1, p.W1 = W1, p.C1 = C1, p.Cout = Cout;
    p.nchunks = C1 / 16, p.ntg = Cout / 32, p.reps = 1;
    p.tz = (int)sp3b_cdiv(D1, sp3b::TZ), p.ty = (int)sp3b_cdiv(H1, sp3b::TY), p.tx = (int)sp3b_cdiv(W1, sp3b::TX);
    const long long blocks = (long long)N * p.tz * p.ty * p.tx * p.ntg;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_subpixel_conv_fwd_bf16: grid too large");
    hipLaunchKernelGGL(subpix3d_fwd_bf16_kernel, dim3((unsigned)blocks), dim3(256), sp3b::F_LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_subpixel_conv_dgrad_bf16(int device, u3d_stream_t stream, const float* dz, const void* packed, const float* x_low,
                                            float* dlow, double* gstats, int N, int D1, int H1, int W1, int C1, int Cout, int reps) {
    U3D_ENTER(device);
    U3D_REQUIRE(sp3b_ok(C1, Cout), "u3d_subpixel_conv_dgrad_bf16: (%d -> %d) channels are outside the bf16 sub-pixel envelope (both %% 32)",
                C1, Cout);
    U3D_REQUIRE(dz && packed && dlow && reps >= 1 && (!gstats || x_low), "u3d_subpixel_conv_dgrad_bf16: bad argument (gstats needs x_low)");
    U3D_REQUIRE(sp3b_dims_ok(N, D1, H1, W1, C1, Cout), "u3d_subpixel_conv_dgrad_bf16: bad sizes (the dz voxel count must be < 2^31)");
    U3D_REQUIRE(sp3b_aligned(dz) && sp3b_aligned(packed) && sp3b_aligned(dlow) && sp3b_aligned(x_low),
                "u3d_subpixel_conv_dgrad_bf16: pointers must be 16-byte aligned");
    Subpix3dBf16Params p = {};
    p.src = dz;
    p.wp = reinterpret_cast<const sp3b_bf16x8*>(packed);
    p.x_low = x_low;
    p.out = dlow;
    p.gstats = gstats;
    p.N = N, p.D1 = D1, p.H1 = H1, p.W1 = W1, p.C1 = C1, p.Cout = Cout;
    p.nchunks = Cout / 16, p.ntg = C1 / 32, p.reps = reps;
    p.tz = (int)sp3b_cdiv(D1, sp3b::TZ), p.ty = (int)sp3b_cdiv(H1, sp3b::TY), p.tx = (int)sp3b_cdiv(W1, sp3b::TX);
    const long long blocks = (long long)N * p.tz * p.ty * p.tx * p.ntg;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_subpixel_conv_dgrad_bf16: grid too large");
    static bool lds_ok[64] = {false};
    U3D_HIP(sp3b_allow_lds(&subpix3d_dgrad_bf16_kernel, sp3b::D_LDS_BYTES, device, lds_ok));
    hipLaunchKernelGGL(subpix3d_dgrad_bf16_kernel, dim3((unsigned)blocks), dim3(256), sp3b::D_LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" long long u3d_subpixel_wgrad_bf16_workspace_floats(int N, int D1, int H1, int W1, int C1, int Cout) {
    if (!sp3b_ok(C1, Cout) || !sp3b_dims_ok(N, D1, H1, W1, C1, Cout)) return 0;
    return (long long)sp3b_wplan(sp3b_current_device(), N, D1, H1, W1, C1, Cout).nsplit * 64 * C1 * Cout;
}

extern "C" int u3d_subpixel_conv_wgrad_bf16(int device, u3d_stream_t stream, const float* low, const float* affine,
                                            long long affine_sample_stride, const float* dz, float* dw, int dw_cin_stride, int N, int D1,
                                            int H1, int W1, int C1, int Cout, float* workspace, long long workspace_floats) {
    U3D_ENTER(device);
    U3D_REQUIRE(sp3b_ok(C1, Cout), "u3d_subpixel_conv_wgrad_bf16: (%d -> %d) channels are outside the bf16 sub-pixel envelope (both %% 32)",
                C1, Cout);
    U3D_REQUIRE(low && dz && dw && workspace && dw_cin_stride >= C1, "u3d_subpixel_conv_wgrad_bf16: bad argument");
    U3D_REQUIRE(sp3b_dims_ok(N, D1, H1, W1, C1, Cout), "u3d_subpixel_conv_wgrad_bf16: bad sizes (the dz voxel count must be < 2^31)");
    U3D_REQUIRE(sp3b_aligned(low) && sp3b_aligned(affine) && sp3b_aligned(dz) && sp3b_aligned(workspace) && affine_sample_stride % 4 == 0,
                "u3d_subpixel_conv_wgrad_bf16: pointers must be 16-byte aligned");
    const long long slot = (long long)64 * C1 * Cout;
    U3D_REQUIRE(workspace_floats >= slot, "u3d_subpixel_conv_wgrad_bf16: workspace too small (%lld floats; one slot is %lld)", workspace_floats,
                slot);
    const Sp3bWPlan pl = sp3b_wplan(device, N, D1, H1, W1, C1, Cout, workspace_floats / slot);
    Subpix3dWgradBf16Params p = {};
    p.low = low;
    p.affine = affine;
    p.astride = affine_sample_stride;
    p.dz = dz;
    p.ws = workspace;
    p.N = N, p.D1 = D1, p.H1 = H1, p.W1 = W1, p.C1 = C1, p.Cout = Cout;
    p.tz = pl.tz, p.ty = pl.ty, p.tx = pl.tx, p.ncob = pl.ncob, p.ncib = pl.ncib, p.ntiles = pl.ntiles, p.tps = pl.tps;
    const long long blocks = (long long)pl.nsplit * pl.ncob * pl.ncib;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_subpixel_conv_wgrad_bf16: grid too large");
    static bool lds_ok[64] = {false};
    U3D_HIP(sp3b_allow_lds(&subpix3d_wgrad_bf16_kernel, sp3b::W_LDS_BYTES, device, lds_ok));
    hipLaunchKernelGGL(subpix3d_wgrad_bf16_kernel, dim3((unsigned)blocks), dim3(512), sp3b::W_LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    const long long total = (long long)27 * C1 * Cout;
    long long rb = sp3b_cdiv(total, 256);
    if (rb > 4096) rb = 4096;
    hipLaunchKernelGGL(subpix3d_wgrad_bf16_fold_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace, pl.nsplit, Cout, C1,
                       dw, (long long)27 * dw_cin_stride);
    U3D_LAUNCH_CHECK();
    return 0;
}
