// u3d_c16_bf16.hip — the 16-channel 3x3x3 convolutions of a UNet3D on the bf16 MFMA (`bf16_stem: true`): forward / data gradient and weight
// gradient for layers whose channel counts are multiples of 16 but not both of 32 (16 -> 32 at full resolution, the 48 -> 16 top decoder
// of an `f_maps: 16` net), the 3-D twins of the `_c16` entry points of csrc/u3d_conv2d_bf16.hip.  This is the first translation unit of
// libu3d_ext_hip.so (include/u3d_ext.h; the second is csrc/u3d_wgrad_f32s.hip), linked against libu3d_hip.so: u3d_set_err / u3d_last_error and u3d_device_guard are the core's.
// Self-contained like csrc/u3d_subpix_bf16.hip: it restates the LDS record layout of csrc/u3d_bf16.hip instead of sharing templates.
// Tensors in HBM are fp32 NDHWC, accumulation is fp32.  Rounding points: the weight is rounded ONCE to bf16, nearest even, by the pack
// kernel; activations and dz are rounded once while staged to LDS, after the fp32 affine fmaf(x, a, b); zero padding applies after the
// affine and stays exactly 0 (c16_stage8).
//
// Forward / data gradient (c16_conv_kernel): a block of 4 waves owns 4 x 8 x 8 voxels x one 32-channel n-tile; wave w owns z-plane w as two
// M-tiles (M-tile m: row r -> (y = 4m + (r & 3), x = r >> 2)).  The 6 x 10 x 10 halo of a 16-channel chunk is staged as two channel-half
// planes [kh][hz][hy][hx pad HS = 12] of 16-byte records, double-buffered — the layout of csrc/u3d_bf16.hip, whose argument carries over
// because the M-tile is the same 4 y x 8 x: the 8 lanes that share a ds_read_b128 pass read records (y .. y + 3, x .. x + 1) at row
// stride HS = 12 records = 48 banks, i.e. bank offsets {0, 48, 32, 16} + {0, 4} — each of the 64 banks once; the second plane starts 64
// bytes off a multiple of 128 so the two planes' staging writes of a (voxel, octet pair) land on different banks.  Cin = 16 is exactly one K = 16 step of
// v_mfma_f32_32x32x16_bf16 per tap: 27 B fragments per chunk, each used by both M-tiles.  A produced channel count of 16 (mod 32) is half
// an n-tile: its image columns are zero and the epilogue masks co >= Cout.  No split-K (these layers sit at high resolution: thousands of
// blocks).  A one-chunk layer (Cin = 16) is launched with one LDS buffer, so four blocks are resident per CU.  The epilogue adds (sum y, sum y^2) or (sum y, sum y * gx) of the stored values, summed in f64 per lane, over the lane halves
// and the four waves in a fixed order, then one f64 atomic per (sample, channel, quantity) and block.
//
// Weight gradient (c16_wgrad_kernel): voxel contraction.  dw[co][ci][tap] = sum_v dz[v][co] * g[v + tap - 1][ci] over 2 x 4 x 16-voxel
// tiles: dz (128 voxels) and the 4 x 6 x 18 halo of g sit in LDS as [voxel][32 channels] bf16 and are fetched as MFMA operands with
// ds_read_b64_tr_b16 (one 16-voxel x-row per K step).  9 waves, wave = (kz, ky), 3 accumulators (kx); the next tile's global loads are in
// flight during the MFMAs of this one.  A block owns one (32 co, 32 ci)
// cell (channels past the count are staged as zero and masked on the way out) and a range of tiles; it writes its 27 matrices to its
// workspace slot [tap][Cout][Cin]; c16_wgrad_reduce_kernel adds the slots in slot order and writes dw in the reference layout: no atomics.
#include "u3d_common.h"

extern "C" {
#include <u3d_ext.h>
}

#include <algorithm>

#define U3D_EXT_VERSION 2

typedef __bf16 c16_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 c16_bf16x4 __attribute__((ext_vector_type(4)));
typedef short c16_s16x4 __attribute__((ext_vector_type(4)));
typedef short c16_s16x8 __attribute__((ext_vector_type(8)));

namespace {

namespace c16 {
constexpr int HS = 12;                                // halo row stride in 16-byte records (csrc/u3d_bf16.hip)
constexpr int TZ = 4, TY = 8, TX = 8;                 // tile: wave = z-plane, two M-tiles of 4 y x 8 x
constexpr int FZ = TZ + 2, FY = TY + 2, FX = TX + 2;  // 6 x 10 x 10 halo
constexpr int FPLANE = FZ * FY * HS * 16 + 64;        // 11584 bytes per channel-half plane
constexpr int FBUF = 2 * FPLANE;                      // 23168
constexpr int FITEMS = FZ * FY * FX * 2;              // 1200 (voxel, channel octet) items per chunk
constexpr int FNIT = (FITEMS + 255) / 256;            // 5
constexpr int F_LDS_BYTES = 2 * FBUF;                 // 46336 (double-buffered; the f64 reduction reuses the first 2048); ONE chunk
                                                      // (Cin = 16, the full-resolution stem layer) never touches the second buffer and is
                                                      // launched with FBUF: a block there is load -> stage -> 54 MFMAs -> store with nothing
                                                      // to overlap inside it, so resident blocks (4 per CU by registers) hide its latency
// weight gradient
constexpr int WTZ = 2, WTY = 4, WTX = 16;             // tile: 8 rows of 16 x
constexpr int WHZ = WTZ + 2, WHY = WTY + 2, WHX = WTX + 2;  // 4 x 6 x 18 halo
constexpr int WPP = 64;                               // bytes per staged voxel (32 bf16)
constexpr int WVOX = WTZ * WTY * WTX;                 // 128
constexpr int WTHREADS = 576;                         // 9 waves: (kz, ky)
constexpr int W_G = 0;                                // [4 * 6 * 18][32] bf16
constexpr int W_DZ = WHZ * WHY * WHX * WPP;           // 27648: [128][32] bf16
constexpr int W_LDS_BYTES = W_DZ + WVOX * WPP;        // 35840
constexpr int W_GITEMS = WHZ * WHY * WHX * 4;         // 1728 (voxel, octet) halo items = 3 per thread
constexpr int W_GIT = W_GITEMS / WTHREADS;            // 3
static_assert(W_GIT * WTHREADS == W_GITEMS, "the halo items divide evenly over the block");
constexpr int W_DITEMS = WVOX * 4;                    // 512 dz items: threads 0 .. 511
}  // namespace c16

inline long long c16_cdiv(long long a, long long b) { return (a + b - 1) / b; }
inline bool c16_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool c16_ok(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 16 == 0 && Cout % 16 == 0; }
inline bool c16_dims_ok(int N, int D, int H, int W, int Cin, int Cout) {
    return N > 0 && D > 0 && H > 0 && W > 0 && (long long)N * D * H * W < (1ll << 31) && (long long)27 * 32 * (Cin + 16) * (Cout + 16) < (1ll << 31);
}

int c16_cu_count(int device) {
    static int cached[64] = {0};
    if (device >= 0 && device < 64 && cached[device] > 0) return cached[device];
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
    if (device >= 0 && device < 64) cached[device] = n;
    return n;
}

int c16_current_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    return dev;
}

// 8 staged channels: affine in fp32 (one fused multiply-add per element), ONE rounding to bf16 (nearest even), zero outside the volume
__device__ __forceinline__ c16_bf16x8 c16_stage8(const f32x4& lo, const f32x4& hi, const float* aff, bool ok) {
    f32x4 v0 = lo, v1 = hi;
    if (aff != nullptr) {
        const f32x4 q0 = u3d_ldq(aff), q1 = u3d_ldq(aff + 4), q2 = u3d_ldq(aff + 8), q3 = u3d_ldq(aff + 12);  // (a, b) pairs
        v0 = f32x4{fmaf(lo[0], q0[0], q0[1]), fmaf(lo[1], q0[2], q0[3]), fmaf(lo[2], q1[0], q1[1]), fmaf(lo[3], q1[2], q1[3])};
        v1 = f32x4{fmaf(hi[0], q2[0], q2[1]), fmaf(hi[1], q2[2], q2[3]), fmaf(hi[2], q3[0], q3[1]), fmaf(hi[3], q3[2], q3[3])};
    }
    if (!ok) v0 = v1 = f32x4{0.f, 0.f, 0.f, 0.f};  // padding stays exactly 0
    const c16_bf16x4 b0 = __builtin_convertvector(v0, c16_bf16x4), b1 = __builtin_convertvector(v1, c16_bf16x4);
    return __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ds_read_b64_tr_b16 x 2: lane l receives channel (l & 31) of the 8 voxels 8 * (l >> 5) .. + 7 of a [voxel][32 channels] run
__device__ __forceinline__ c16_bf16x8 c16_tr_frag(const char* lds_addr) {
    const c16_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) c16_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)lds_addr);
    const c16_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) c16_s16x4*)(uintptr_t)(uint32_t)(uintptr_t)(lds_addr + 4 * c16::WPP));
    const c16_s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(c16_bf16x8, v);
}

// image [K / 16 chunk][27 taps][n-tile][lane][8] of B[k = chunk * 16 + 8 (lane >> 5) + j][n = 32 n-tile + (lane & 31)]; w (Cout, Cin, 27).
// mode 0: B[ci][co] = w[co][ci][tap]; mode 1: B[co][ci] = w[co][ci][26 - tap].  Columns n >= Nn (half an n-tile) are zero.
__global__ void c16_pack_kernel(const float* __restrict__ w, int Cin, int Nn, int mode, int ntg, long long total, __bf16* __restrict__ packed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        long long r = i >> 9;
        const int nt = (int)(r % ntg);
        r /= ntg;
        const int tap = (int)(r % 27);
        const int chunk = (int)(r / 27);
        const int k = chunk * 16 + 8 * (lane >> 5) + j;
        const int nn = nt * 32 + (lane & 31);
        float v = 0.f;
        if (nn < Nn) v = mode == 0 ? w[((size_t)nn * Cin + k) * 27 + tap] : w[((size_t)k * Cin + nn) * 27 + 26 - tap];
        packed[i] = (__bf16)v;
    }
}

struct C16ConvParams {
    const float* x;       // (N,D,H,W,Cin)
    const float* affine;  // (N,Cin,2) or null
    const c16_bf16x8* wp;
    float* out;           // (N,D,H,W,Cout)
    const float* gx;      // (N,D,H,W,Cout) for gstats, or null
    double* stats;        // out_stats or gstats, or null
    int N, D, H, W, Cin, Cout;
    int nchunks, ntg, tz, ty, tx, relu;
};

__global__ __launch_bounds__(256, 4) void c16_conv_kernel(const C16ConvParams p) {
    using namespace c16;
    extern __shared__ __attribute__((aligned(16))) char lds_c16f[];
    char* const lds = lds_c16f;
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
    const int D = p.D, H = p.H, W = p.W, Cin = p.Cin;

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
        const bool ok = in && gz >= 0 && gz < D && gy >= 0 && gy < H && gxx >= 0 && gxx < W;
        ldsoff[it] = in ? q * FPLANE + ((hz * FY + hy) * HS + hx) * 16 : -1;
        gpix[it] = ok ? ((n * D + gz) * H + gy) * W + gxx : -1;
    }
    const float* const aff_n = p.affine != nullptr ? p.affine + (size_t)n * Cin * 2 : nullptr;
    f32x4 raw[FNIT][2];
    auto load_chunk = [&](int c) {
#pragma unroll
        for (int it = 0; it < FNIT; ++it) {
            raw[it][0] = raw[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (gpix[it] >= 0) {
                const float* src = p.x + (size_t)gpix[it] * Cin + c * 16 + 8 * ((t + 256 * it) & 1);
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
            *reinterpret_cast<c16_bf16x8*>(buf + ldsoff[it]) = c16_stage8(raw[it][0], raw[it][1], aff, ok);
        }
    };

    f32x16 acc[2];  // [M-tile]
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

    // A-fragment base: lane (i32, h) owns voxel (w, i32 & 3 [+ 4 for M-tile 1], i32 >> 2) of the tile, channels 8h .. 8h + 7; tap (dz, dy, dx)
    // of it is halo voxel (+dz, +dy, +dx)
    const int abase = h * FPLANE + ((w * FY + (i32 & 3)) * HS + (i32 >> 2)) * 16;
    auto bidx = [&](int c, int tap) -> long long { return ((long long)(c * 27 + tap) * p.ntg + cb) * 64 + l; };

    load_chunk(0);
    store_chunk(0, lds);
    __syncthreads();
    for (int c = 0; c < p.nchunks; ++c) {
        const char* cur = lds + (c & 1) * FBUF;
        if (c + 1 < p.nchunks) load_chunk(c + 1);  // in flight during the MFMAs
        // (B one tap ahead: holding all 27 fragments of a chunk — 108 registers — was measured and lost to the occupancy it costs)
        c16_bf16x8 bq = p.wp[bidx(c, 0)], bn = bq;
#pragma unroll
        for (int tap = 0; tap < 27; ++tap) {
            if (tap + 1 < 27) bn = p.wp[bidx(c, tap + 1)];  // (never leaves the chunk: no tail padding of the image)
            const int dz = tap / 9, dy = (tap / 3) % 3, dx = tap % 3;
            const char* a = cur + abase + ((dz * FY + dy) * HS + dx) * 16;
            const c16_bf16x8 a0 = *reinterpret_cast<const c16_bf16x8*>(a);
            const c16_bf16x8 a1 = *reinterpret_cast<const c16_bf16x8*>(a + 4 * HS * 16);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bq, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bq, acc[1], 0, 0, 0);
            bq = bn;
        }
        if (c + 1 < p.nchunks) store_chunk(c + 1, lds + ((c + 1) & 1) * FBUF);  // (that buffer was last read in chunk c - 1)
        __syncthreads();
    }

    // ---- lane column = produced channel, register r = M row (r & 3) + 8 (r >> 2) + 4h = (y = row & 3, x = row >> 2)
    const int co = cb * 32 + i32;
    const bool cok = co < p.Cout;
    const int zi = z0 + w;
    double s0 = 0.0, s1 = 0.0;
    if (zi < D && cok) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int yi = y0 + 4 * m + (row & 3), xi = x0 + (row >> 2);
                if (yi >= H || xi >= W) continue;
                const size_t o = ((size_t)((n * D + zi) * H + yi) * W + xi) * p.Cout + co;
                float v = acc[m][r];
                if (p.relu) v = v > 0.f ? v : 0.f;
                p.out[o] = v;
                if (p.stats != nullptr) {
                    s0 += (double)v;
                    s1 += (double)v * (double)(p.gx != nullptr ? p.gx[o] : v);
                }
            }
    }
    if (p.stats != nullptr) {  // (uniform over the grid) lane halves, then the 4 waves in a fixed order, one f64 atomic per quantity
        double* red = reinterpret_cast<double*>(lds);  // [4][32][2]; the last barrier of the chunk loop freed the buffers
        s0 += __shfl_xor(s0, 32);
        s1 += __shfl_xor(s1, 32);
        if (l < 32) {
            red[(w * 32 + l) * 2] = s0;
            red[(w * 32 + l) * 2 + 1] = s1;
        }
        __syncthreads();
        if (t < 32 && cb * 32 + t < p.Cout) {
            const double a0 = ((red[t * 2] + red[(32 + t) * 2]) + red[(64 + t) * 2]) + red[(96 + t) * 2];
            const double a1 = ((red[t * 2 + 1] + red[(32 + t) * 2 + 1]) + red[(64 + t) * 2 + 1]) + red[(96 + t) * 2 + 1];
            double* o = p.stats + ((size_t)n * p.Cout + cb * 32 + t) * 2;
            u3d_atomic_add_f64(o, a0);
            u3d_atomic_add_f64(o + 1, a1);
        }
    }
}

struct C16WgradParams {
    const float* x;       // (N,D,H,W,Cin)
    const float* affine;  // (N,Cin,2) or null
    const float* dz;      // (N,D,H,W,Cout)
    float* ws;            // [nsplit][27][Cout][Cin]
    int N, D, H, W, Cin, Cout;
    int tz, ty, tx, ncob, ncib, ntiles, tps;
};

__global__ __launch_bounds__(576) void c16_wgrad_kernel(const C16WgradParams p) {
    using namespace c16;
    extern __shared__ __attribute__((aligned(16))) char lds_c16w[];
    char* const lds = lds_c16w;
    const int t = threadIdx.x, l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int b = blockIdx.x;
    const int cib = b % p.ncib;
    b /= p.ncib;
    const int cob = b % p.ncob;
    const int split = b / p.ncob;
    const int ci0 = cib * 32, co0 = cob * 32;
    const int tile0 = split * p.tps, tile1 = min(p.ntiles, tile0 + p.tps);
    const int D = p.D, H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout;
    char* const gl = lds + W_G;
    char* const dzl = lds + W_DZ;
    const int kz = w / 3, ky = w % 3;  // this wave's tap plane and row

    f32x16 acc[3];  // [kx]
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    // transposed-read lane offset: lane l receives channel (l & 31) of the 8 voxels 8 * (l >> 5) .. + 7
    const int g4 = l >> 4, sidx = l & 15;
    const int lane_off = (8 * (g4 >> 1) + (sidx >> 2)) * WPP + (16 * (g4 & 1) + 4 * (sidx & 3)) * 2;

    // a tile's operands: g (4 x 6 x 18 halo from (z0 - 1, y0 - 1, x0 - 1), 32 channels from ci0: affine, zero padding, zero past Cin) and
    // dz (the 128 voxels of the tile, 32 channels from co0, zero outside the volume and past Cout).  load_tile puts the raw fp32 values in
    // registers — the next tile's are in flight during this tile's MFMAs (one block is resident per CU) —, store_tile stages them
    f32x4 rg[W_GIT][2], rd[2];
    bool okg[W_GIT], okd = false;
    const float* aff_n = nullptr;
    auto load_tile = [&](int tile) {
        int tt = tile;
        const int txi = tt % p.tx;
        tt /= p.tx;
        const int tyi = tt % p.ty;
        tt /= p.ty;
        const int tzi = tt % p.tz;
        const int n = tt / p.tz;
        const int z0 = tzi * WTZ, y0 = tyi * WTY, x0 = txi * WTX;
        aff_n = p.affine != nullptr ? p.affine + (size_t)n * Cin * 2 : nullptr;
#pragma unroll
        for (int k = 0; k < W_GIT; ++k) {
            const int item = t + WTHREADS * k;
            const int q = item & 3;
            int pix = item >> 2;
            const int hx = pix % WHX;
            pix /= WHX;
            const int hy = pix % WHY;
            const int hz = pix / WHY;
            const int gz = z0 - 1 + hz, gy = y0 - 1 + hy, gxx = x0 - 1 + hx;
            okg[k] = gz >= 0 && gz < D && gy >= 0 && gy < H && gxx >= 0 && gxx < W && ci0 + 8 * q < Cin;
            rg[k][0] = rg[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (okg[k]) {
                const float* src = p.x + ((size_t)((n * D + gz) * H + gy) * W + gxx) * Cin + ci0 + 8 * q;
                rg[k][0] = u3d_ldq(src);
                rg[k][1] = u3d_ldq(src + 4);
            }
        }
        rd[0] = rd[1] = f32x4{0.f, 0.f, 0.f, 0.f};
        okd = false;
        if (t < W_DITEMS) {
            const int q = t & 3, pix = t >> 2;
            const int zi = z0 + (pix >> 6), yi = y0 + ((pix >> 4) & 3), xi = x0 + (pix & 15);
            okd = zi < D && yi < H && xi < W && co0 + 8 * q < Cout;
            if (okd) {
                const float* src = p.dz + ((size_t)((n * D + zi) * H + yi) * W + xi) * Cout + co0 + 8 * q;
                rd[0] = u3d_ldq(src);
                rd[1] = u3d_ldq(src + 4);
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int k = 0; k < W_GIT; ++k) {
            const int item = t + WTHREADS * k;
            const float* aff = (aff_n != nullptr && okg[k]) ? aff_n + (ci0 + 8 * (item & 3)) * 2 : nullptr;
            *reinterpret_cast<c16_bf16x8*>(gl + (item >> 2) * WPP + 16 * (item & 3)) = c16_stage8(rg[k][0], rg[k][1], aff, okg[k]);
        }
        if (t < W_DITEMS) *reinterpret_cast<c16_bf16x8*>(dzl + (t >> 2) * WPP + 16 * (t & 3)) = c16_stage8(rd[0], rd[1], nullptr, okd);
    };

    load_tile(tile0);
    for (int tile = tile0; tile < tile1; ++tile) {
        store_tile();
        __syncthreads();
        if (tile + 1 < tile1) load_tile(tile + 1);
        // wave (kz, ky): the 8 rows of dz, one 16-voxel row per K step; tap (kz, ky, kx) pairs dz voxel (pz, py, px) with halo voxel
        // (pz + kz, py + ky, px + kx)
#pragma unroll 2
        for (int row = 0; row < WTZ * WTY; ++row) {
            const int pz = row >> 2, py = row & 3;
            const c16_bf16x8 a = c16_tr_frag(dzl + row * WTX * WPP + lane_off);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const c16_bf16x8 g = c16_tr_frag(gl + (((pz + kz) * WHY + py + ky) * WHX + kx) * WPP + lane_off);
                acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, g, acc[kx], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---- this block's cell of its slot [tap][Cout][Cin]: register r = output channel (r & 3) + 8 (r >> 2) + 4h, lane column = ci
    const size_t mat = (size_t)Cout * Cin;
    float* const dst = p.ws + (size_t)split * 27 * mat;
    const int ci = ci0 + i32;
    if (ci < Cin) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (co < Cout) dst[(size_t)((kz * 3 + ky) * 3 + kx) * mat + (size_t)co * Cin + ci] = acc[kx][r];
            }
    }
}

// dw[co][ci][tap] = the slots' [tap][co][ci] added in slot order
__global__ void c16_wgrad_reduce_kernel(const float* __restrict__ ws, int nsplit, long long mat, float* __restrict__ dw) {
    const long long total = 27 * mat;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int tap = (int)(i % 27);
        const long long cc = i / 27;  // co * Cin + ci
        const float* m = ws + (size_t)tap * mat + cc;
        float v = 0.f;
        for (int s = 0; s < nsplit; ++s) v += m[(size_t)s * total];
        dw[i] = v;
    }
}

struct C16WPlan {
    int tz, ty, tx, ncob, ncib, ntiles, tps, nsplit;
};

// one block per CU over the launch (9 waves of 128 VGPRs: one block is resident per CU); ONE function for the launcher and the workspace
// size.  max_slots > 0: no more splits than that many workspace slots hold (the launcher passes what it
// was given, so a workspace sized on another device — other CU count — still runs, on as many splits as it holds)
C16WPlan c16_wplan(int device, int N, int D, int H, int W, int Cin, int Cout, long long max_slots = 0) {
    C16WPlan pl;
    pl.tz = (int)c16_cdiv(D, c16::WTZ);
    pl.ty = (int)c16_cdiv(H, c16::WTY);
    pl.tx = (int)c16_cdiv(W, c16::WTX);
    pl.ncob = (int)c16_cdiv(Cout, 32);
    pl.ncib = (int)c16_cdiv(Cin, 32);
    pl.ntiles = N * pl.tz * pl.ty * pl.tx;
    const long long cells = (long long)pl.ncob * pl.ncib;
    const long long target = c16_cu_count(device);
    long long ns = std::max<long long>(1, std::min<long long>(pl.ntiles, c16_cdiv(target, cells)));
    if (max_slots > 0) ns = std::min(ns, max_slots);
    pl.tps = (int)c16_cdiv(pl.ntiles, ns);
    pl.nsplit = (int)c16_cdiv(pl.ntiles, pl.tps);
    return pl;
}

}  // namespace

extern "C" int u3d_ext_version(void) { return U3D_EXT_VERSION; }

extern "C" int u3d_conv3d_bf16_c16_supported(int Cin, int Cout) { return c16_ok(Cin, Cout) ? 1 : 0; }

extern "C" long long u3d_packed_weight_bf16_c16_elems(int Cin, int Cout, int mode) {
    if ((mode != 0 && mode != 1) || !c16_ok(Cin, Cout) || (long long)27 * 32 * (Cin + 16) * (Cout + 16) >= (1ll << 31)) return 0;
    const int K = mode == 0 ? Cin : Cout, Nn = mode == 0 ? Cout : Cin;
    return (long long)(K / 16) * 27 * c16_cdiv(Nn, 32) * 512;  // the B prefetch never leaves a chunk: no tail padding
}

extern "C" int u3d_pack_weights_bf16_c16(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, void* packed) {
    U3D_ENTER(device);
    U3D_REQUIRE(w && packed && (mode == 0 || mode == 1), "u3d_pack_weights_bf16_c16: bad argument");
    const long long total = u3d_packed_weight_bf16_c16_elems(Cin, Cout, mode);
    U3D_REQUIRE(total > 0, "u3d_pack_weights_bf16_c16: (%d -> %d) channels are outside the 16-channel bf16 envelope (both %% 16)", Cin, Cout);
    U3D_REQUIRE(c16_aligned(packed), "u3d_pack_weights_bf16_c16: the image must be 16-byte aligned");
    long long blocks = c16_cdiv(total, 256);
    if (blocks > 4096) blocks = 4096;
    const int Nn = mode == 0 ? Cout : Cin;
    hipLaunchKernelGGL(c16_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, Cin, Nn, mode, (int)c16_cdiv(Nn, 32),
                       total, reinterpret_cast<__bf16*>(packed));
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" long long u3d_conv3d_bf16_c16_workspace_floats(int, int, int, int, int, int) { return 0; }

extern "C" int u3d_conv3d_bf16_c16(int device, u3d_stream_t stream, const float* x, const float* affine, const void* packed_w, float* out,
                                   int N, int D, int H, int W, int Cin, int Cout, int relu, double* out_stats, const float* gx,
                                   double* gstats, float* workspace, long long workspace_floats) {
    U3D_ENTER(device);
    (void)workspace;
    (void)workspace_floats;
    U3D_REQUIRE(c16_ok(Cin, Cout), "u3d_conv3d_bf16_c16: (%d -> %d) channels are outside the 16-channel bf16 envelope (both %% 16)", Cin, Cout);
    U3D_REQUIRE(x && packed_w && out && !(out_stats && gstats) && (!gstats || gx),
                "u3d_conv3d_bf16_c16: bad argument (gstats needs gx and is exclusive with out_stats)");
    U3D_REQUIRE(c16_dims_ok(N, D, H, W, Cin, Cout), "u3d_conv3d_bf16_c16: bad sizes (the voxel count must be < 2^31)");
    U3D_REQUIRE(c16_aligned(x) && c16_aligned(affine) && c16_aligned(packed_w) && c16_aligned(out) && c16_aligned(gx),
                "u3d_conv3d_bf16_c16: pointers must be 16-byte aligned");
    C16ConvParams p = {};
    p.x = x;
    p.affine = affine;
    p.wp = reinterpret_cast<const c16_bf16x8*>(packed_w);
    p.out = out;
    p.gx = gstats ? gx : nullptr;
    p.stats = out_stats ? out_stats : gstats;
    p.N = N, p.D = D, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout;
    p.nchunks = Cin / 16, p.ntg = (int)c16_cdiv(Cout, 32), p.relu = relu ? 1 : 0;
    p.tz = (int)c16_cdiv(D, c16::TZ), p.ty = (int)c16_cdiv(H, c16::TY), p.tx = (int)c16_cdiv(W, c16::TX);
    const long long blocks = (long long)N * p.tz * p.ty * p.tx * p.ntg;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_conv3d_bf16_c16: grid too large");
    hipLaunchKernelGGL(c16_conv_kernel, dim3((unsigned)blocks), dim3(256), p.nchunks > 1 ? c16::F_LDS_BYTES : c16::FBUF,
                       (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" long long u3d_wgrad_bf16_c16_workspace_floats(int N, int D, int H, int W, int Cin, int Cout) {
    if (!c16_ok(Cin, Cout) || !c16_dims_ok(N, D, H, W, Cin, Cout)) return 0;
    return (long long)c16_wplan(c16_current_device(), N, D, H, W, Cin, Cout).nsplit * 27 * Cin * Cout;
}

extern "C" int u3d_conv3d_wgrad_bf16_c16(int device, u3d_stream_t stream, const float* x, const float* affine, const float* dz, float* dw,
                                         int N, int D, int H, int W, int Cin, int Cout, float* workspace, long long workspace_floats) {
    U3D_ENTER(device);
    U3D_REQUIRE(c16_ok(Cin, Cout), "u3d_conv3d_wgrad_bf16_c16: (%d -> %d) channels are outside the 16-channel bf16 envelope (both %% 16)", Cin,
                Cout);
    U3D_REQUIRE(x && dz && dw && workspace, "u3d_conv3d_wgrad_bf16_c16: bad argument (the workspace is always needed)");
    U3D_REQUIRE(c16_dims_ok(N, D, H, W, Cin, Cout), "u3d_conv3d_wgrad_bf16_c16: bad sizes (the voxel count must be < 2^31)");
    U3D_REQUIRE(c16_aligned(x) && c16_aligned(affine) && c16_aligned(dz) && c16_aligned(workspace),
                "u3d_conv3d_wgrad_bf16_c16: pointers must be 16-byte aligned");
    const long long slot = (long long)27 * Cin * Cout;
    U3D_REQUIRE(workspace_floats >= slot, "u3d_conv3d_wgrad_bf16_c16: workspace too small (%lld floats; one slot is %lld)", workspace_floats, slot);
    const C16WPlan pl = c16_wplan(device, N, D, H, W, Cin, Cout, workspace_floats / slot);
    C16WgradParams p = {};
    p.x = x;
    p.affine = affine;
    p.dz = dz;
    p.ws = workspace;
    p.N = N, p.D = D, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout;
    p.tz = pl.tz, p.ty = pl.ty, p.tx = pl.tx, p.ncob = pl.ncob, p.ncib = pl.ncib, p.ntiles = pl.ntiles, p.tps = pl.tps;
    const long long blocks = (long long)pl.nsplit * pl.ncob * pl.ncib;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_conv3d_wgrad_bf16_c16: grid too large");
    hipLaunchKernelGGL(c16_wgrad_kernel, dim3((unsigned)blocks), dim3(c16::WTHREADS), c16::W_LDS_BYTES, (hipStream_t)stream, p);
    U3D_LAUNCH_CHECK();
    long long rb = c16_cdiv(slot, 256);
    if (rb > 4096) rb = 4096;
    hipLaunchKernelGGL(c16_wgrad_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace, pl.nsplit, slot / 27, dw);
    U3D_LAUNCH_CHECK();
    return 0;
}
