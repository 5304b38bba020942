// u3d_conv2d_f32s.h — the 3x3 Conv2d kernels of a UNet2D in `compute_dtype: fp32_split` (`native_2d_fp32_split: true`): forward, data
// gradient and weight gradient as six bf16 partial products of exactly split fp32 operands on v_mfma_f32_32x32x16_bf16.  Device code and
// entry points of libu3d_ext_hip.so (include/u3d_ext.h); a header of csrc/u3d_wgrad_f32s.hip, included at its end: wf_split8, wf_tr_frag
// and the small host helpers (wf_cdiv, wf_aligned, wf_cu_count, wf_current_device) are that file's.
//
// Arithmetic (conv3d_f32s_kernel of csrc/u3d_bf16.hip, wf_wgrad_kernel of csrc/u3d_wgrad_f32s.hip).  Every fp32 operand is split while it
// is staged, after the fp32 affine fmaf(x, a, b): h = bf16(g), m = bf16(g - h), l = bf16(g - h - m), nearest even, both subtractions
// exact; zero padding applies after the affine and stays exactly 0.  The weights are split by u3d_pack_weights2d_f32s into three images.
// Six products, smallest class first: (h, l) (l, h) (m, m) (h, m) (m, h) (h, h); fp32 accumulation in the MFMA.  The bf16 MFMA rounds its
// accumulation toward minus infinity, a drift linear in the chain length:
//   forward / data gradient   the weight images carry the sign (-1)^chunk and the accumulators are negated between 16-channel chunks
//                             (exact), so the drift of consecutive chunks has opposite sign: result = (-1)^(last chunk) * acc
//   weight gradient           every 16 x 16 pixel tile's chain (16 rows x 6 products) starts from zero and is closed into a second
//                             register set with VALU adds; dz is staged with the sign (-1)^(tile - first tile) and the closing add is a
//                             subtract for odd tiles
//
// Forward / data gradient (c2s_conv_kernel): the tiling of conv2d_bf16_kernel (csrc/u3d_conv2d_bf16.hip).  A block of 4 waves owns a
// 16 x 16 pixel tile and 32 * NT produced channels (NT = 2 when the produced count is a multiple of 64); per 16-channel chunk the 18 x 18
// halo sits in LDS as three part planes [hy][hx][16 bf16] of 10656 bytes (592 bytes per row: an odd number of 16-byte slots, the
// conflict-free ds_read_b128 pattern of that kernel), double-buffered: 63936 bytes per block, two blocks per CU.  Per tap a wave reads
// 3 x 2 A fragments and 3 x NT B fragments for 6 * 2 * NT MFMAs; the B fragments stream from the packed images one tap ahead.
// NO split-K in this version: a small grid at the bottom of the U runs its whole channel reduction in one block.
// The RES variants (u3d_conv2d_f32s_res, `native_2d_residual_fp32_split: true`: conv3 of a ResidualUNet2D's ResNetBlock) add the fp32
// residual to the signed sum in the epilogue, before the ReLU and the statistics.
//
// Weight gradient (c2s_wgrad_kernel): a block of 9 waves owns one (32 co, 32 ci) cell and a contiguous range of 16 x 16 pixel tiles; the
// three parts of the 18 x 18 halo of g and of the 256 pixels of dz sit in LDS as [part][pixel][32 channels] (3 x 20736 + 3 x 16384 =
// 111360 bytes, one block per CU) and are fetched with ds_read_b64_tr_b16, one 16-pixel row per K step.  Wave = tap (ky, kx): 3 + 3
// fragments per row for 6 MFMAs in ONE accumulator.  The next tile's global loads are in flight during this tile's MFMAs.  Every block
// writes its 9 matrices to its workspace slot [tap][Cout][Cin]; c2s_wreduce_kernel adds the slots — four contiguous slot ranges in slot
// order each, then the four in order — and writes dw (Cout, Cin, 3, 3).  No atomics.
//
// Virtual concat: every entry point reads cat(skip, nearest(low)) through two bases and the ymap / xmap tables (template parameter V / VC,
// as the `_src` variants of the bf16 kernels).  With both halves % 32 channels a 16-channel chunk, a 32-channel n-tile and a 32-channel
// weight-gradient cell lie wholly in one source: the choice is a uniform branch, and the staged values are those of the written-out concat.
#pragma once

namespace {

namespace c2s {
constexpr int TY = 16, TX = 16;          // output tile
constexpr int HY = TY + 2, HX = TX + 2;  // halo
constexpr int CC = 16;                   // contraction channels per chunk = one MFMA k-step per tap
constexpr int PS = 32;                   // bytes per staged pixel and part (16 bf16)
constexpr int RS = HX * PS + 16;         // 592 bytes per halo row: an odd number of 16-byte slots
constexpr int PLANE = HY * RS;           // 10656 bytes per part plane
constexpr int BUF = 3 * PLANE;           // 31968 bytes per staging buffer (h | m | l)
constexpr int LDS_BYTES = 2 * BUF;       // 63936 (the final [4 waves][NT][32][4] statistics reduction reuses the first 4096)
constexpr int NITEMS = HY * HX * 2;      // 648 (pixel, channel octet) items per chunk
constexpr int NIT = (NITEMS + 255) / 256;  // 3
// weight gradient
constexpr int WPP = 64;                  // bytes per staged pixel and part (32 bf16)
constexpr int W_THREADS = 576;           // 9 waves: (ky, kx)
constexpr int W_GPART = HY * HX * WPP;   // 20736 bytes per part of the halo
constexpr int W_DPART = TY * TX * WPP;   // 16384 bytes per part of dz
constexpr int W_G = 0;
constexpr int W_DZ = 3 * W_GPART;        // 62208
constexpr int W_LDS_BYTES = W_DZ + 3 * W_DPART;  // 111360
constexpr int W_GITEMS = HY * HX * 4;    // 1296 (pixel, octet) halo items
constexpr int W_GIT = (W_GITEMS + W_THREADS - 1) / W_THREADS;  // 3 (the third only for threads 0 .. 143)
constexpr int W_DITEMS = TY * TX * 4;    // 1024 dz items
constexpr int W_DIT = (W_DITEMS + W_THREADS - 1) / W_THREADS;  // 2
constexpr int RED_PARTS = 4;             // slot ranges of the reduce kernel
static_assert(WPP == wf::PP, "wf_tr_frag reads [pixel][32 channels] images");
}  // namespace c2s

inline bool c2s_fwd_ok(int K, int Nn) { return K > 0 && Nn > 0 && K % 16 == 0 && Nn % 32 == 0; }
inline bool c2s_wgrad_ok(int Cin, int Cout) { return Cin > 0 && Cout > 0 && Cin % 32 == 0 && Cout % 32 == 0; }
inline bool c2s_dims_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && (long long)N * H * W < (1ll << 31); }
// a virtual source: both halves present and % 32, the two index tables
inline bool c2s_vsrc_ok(const float* p1, const int32_t* ymap, const int32_t* xmap, int C0, int C1, int H1, int W1) {
    return p1 && ymap && xmap && C0 > 0 && C1 > 0 && C0 % 32 == 0 && C1 % 32 == 0 && H1 > 0 && W1 > 0;
}

inline long long c2s_part_elems(int K, int Nn) { return c2s_fwd_ok(K, Nn) ? (long long)(K / c2s::CC) * 9 * (Nn / 32) * 64 * 8 : 0; }

// =================================================================================================
// weight packing: three images (h | m | l of the signed weight), each [chunk][tap][ntile][lane][8] of B[k][n] as
// pack_weights2d_bf16_kernel writes them: lane l holds k = 16 * chunk + 8 * (l >> 5) + j, column n = 32 * ntile + (l & 31).
//   mode 0 (forward): B[k = ci][n = co] = w[co][ci][tap]           mode 1 (data gradient): B[k = co][n = ci] = w[co][ci][8 - tap]
// times (-1)^chunk: see the accumulator negation in c2s_conv_kernel
__global__ void c2s_pack_kernel(const float* __restrict__ w, int Cin, int mode, int ntg, long long per_part, __bf16* __restrict__ packed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < per_part; i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7);
        const int lane = (int)((i >> 3) & 63);
        long long r = i >> 9;
        const int nt = (int)(r % ntg);
        r /= ntg;
        const int tap = (int)(r % 9);
        const int chunk = (int)(r / 9);
        const int k = chunk * c2s::CC + 8 * (lane >> 5) + j;
        const int nn = nt * 32 + (lane & 31);
        float v = mode == 0 ? w[((size_t)nn * Cin + k) * 9 + tap] : w[((size_t)k * Cin + nn) * 9 + (8 - tap)];
        if (chunk & 1) v = -v;
        const __bf16 h = (__bf16)v;
        const float r1 = v - (float)h;
        const __bf16 m = (__bf16)r1;
        packed[i] = h;
        packed[per_part + i] = m;
        packed[2 * per_part + i] = (__bf16)(r1 - (float)m);
    }
}

// =================================================================================================
// forward / data gradient
struct C2sParams {
    const float* x;        // (N,H,W,Cin) fp32; V = 1: the skip half (N,H,W,C0)
    const float* x1;       // V = 1: the low-res half (N,H1,W1,C1)
    const float* affine;   // (N,Cin,2) or null
    const wf_bf16x8* wp;   // three images, `wpart` records of 8 bf16 apart
    long long wpart;
    const float* gx;       // data gradient: the layer's forward input (N,H,W,Cout) or null; V = 2: its skip half (N,H,W,C0)
    const float* gx1;      // V = 2: its low-res half (N,H1,W1,C1)
    const int32_t* ymap;
    const int32_t* xmap;
    float* out;
    double* out_stats;
    double* gstats;
    int N, H, W, Cin, Cout;
    int C0, C1, H1, W1;
    int nchunks, ntg, ncb, ty, tx;
    int relu, stat_reps;
    const float* residual;  // RES: (N,H,W,Cout) fp32, added to the signed sum before the ReLU and the statistics; may alias `out`
};

// per-block statistics, as c2b_flush_stats of csrc/u3d_conv2d_bf16.hip: column sums s[nt][0..3] = (sum v, sum v^2, sum v, sum v * gx)
// combined over the lane halves, over the 4 waves in LDS (fixed order), then one f64 atomic per (sample, channel, quantity) and block
// into replica row block % reps
template <int NT>
__device__ __forceinline__ void c2s_flush_stats(const C2sParams& p, float* red, float (&s)[NT][4], int n, int cb, int t) {
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
        if (p.gstats) {
            double* o = p.gstats + (row + (size_t)n * p.Cout + co) * 2;
            u3d_atomic_add_f64(o, (double)a[2]);
            u3d_atomic_add_f64(o + 1, (double)a[3]);
        }
    }
}

// V = 0: single tensors.  V = 1 / 2: x / gx is a virtual concat (C0 and C1 multiples of 32: a staged chunk / an n-tile lies in one source)
// RES (u3d_conv2d_f32s_res, V = 0 only): out = [relu](conv + residual), the tail of a ResNetBlock — the fp32 residual is read with the
// store's access pattern (lane = channel, register = pixel row) by the lane that then writes the element, so it may alias `out`
template <int NT, int V, bool RES = false>
__global__ __launch_bounds__(256, 2) void c2s_conv_kernel(const C2sParams p) {
    constexpr bool VX = V == 1, VG = V == 2;
    using namespace c2s;
    extern __shared__ __attribute__((aligned(16))) char lds_c2s[];
    char* const lds = lds_c2s;
    const int t = threadIdx.x;
    const int l = t & 63, w = t >> 6, h = l >> 5;

    int logical = blockIdx.x;
    const int cb = logical % p.ncb;
    int tile = logical / p.ncb;
    const int txi = tile % p.tx;
    tile /= p.tx;
    const int tyi = tile % p.ty;
    const int n = tile / p.ty;
    const int y0 = tyi * TY, x0 = txi * TX;
    const int H = p.H, W = p.W, Cin = p.Cin;
    const int nch = p.nchunks;

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
                    src = (ch >= p.C0 ? p.x1 + goff1[it] + (ch - p.C0) : p.x + goff[it] + ch) + cqs[it];
                } else {
                    src = p.x + goff[it] + c * CC + cqs[it];
                }
                raw[it][0] = u3d_ldq(src);
                raw[it][1] = u3d_ldq(src + 4);
            }
        }
    };
    auto store_chunk = [&](int c, char* buf) {  // fp32 -> affine -> zero padding -> (h, m, l) planes
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            if (ldsoff[it] < 0) continue;
            const float* aff = (p.affine != nullptr && oks[it]) ? p.affine + ((size_t)n * Cin + c * CC + cqs[it]) * 2 : nullptr;
            wf_bf16x8 oh, om, ol;
            wf_split8(raw[it][0], raw[it][1], aff, oks[it], false, oh, om, ol);
            *reinterpret_cast<wf_bf16x8*>(buf + ldsoff[it]) = oh;
            *reinterpret_cast<wf_bf16x8*>(buf + PLANE + ldsoff[it]) = om;
            *reinterpret_cast<wf_bf16x8*>(buf + 2 * PLANE + ldsoff[it]) = ol;
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
    // B images: [chunk][tap][ntg][lane] records of 8 bf16, part pb at pb * wpart
    auto bidx = [&](int c, int tap, int nt) -> long long { return ((long long)(c * 9 + tap) * p.ntg + (cb * NT + nt)) * 64 + l; };

    load_chunk(0);
    store_chunk(0, lds);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        const char* cur = lds + (c & 1) * BUF;
        if (c + 1 < nch) load_chunk(c + 1);  // in flight during the k-loop
        if (c > 0) {  // the images carry (-1)^chunk: negating the sums between chunks alternates the sign of the MFMA's round-down drift
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mt][nt][r] = -acc[mt][nt][r];
        }
        wf_bf16x8 bq[3][NT], bn[3][NT];
#pragma unroll
        for (int pb = 0; pb < 3; ++pb)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bq[pb][nt] = p.wp[pb * p.wpart + bidx(c, 0, nt)];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap - (tap / 3) * 3;
            if (tap + 1 < 9) {
#pragma unroll
                for (int pb = 0; pb < 3; ++pb)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bn[pb][nt] = p.wp[pb * p.wpart + bidx(c, tap + 1, nt)];
            }
            wf_bf16x8 a[3][2];
#pragma unroll
            for (int pa = 0; pa < 3; ++pa)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    a[pa][mt] = *reinterpret_cast<const wf_bf16x8*>(cur + pa * PLANE + abase + (2 * mt + dy) * RS + dx * PS);
            // the six product classes, smallest first; consecutive MFMAs go to different accumulators
#pragma unroll
            for (int cls = 0; cls < 6; ++cls) {
                constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA[cls]][mt], bq[PB[cls]][nt], acc[mt][nt], 0, 0, 0);
            }
            if (tap + 1 < 9) {
#pragma unroll
                for (int pb = 0; pb < 3; ++pb)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) bq[pb][nt] = bn[pb][nt];
            }
        }
        if (c + 1 < nch) store_chunk(c + 1, lds + ((c + 1) & 1) * BUF);  // (that buffer was last read in chunk c - 1)
        __syncthreads();
    }
    const float sgn = ((nch - 1) & 1) ? -1.f : 1.f;  // result = (-1)^(last chunk) * acc

    // ---- epilogue: lane column = output channel (l & 31), register r = M row (r & 3) + 8 (r >> 2) + 4h
    float s[NT][4];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int q = 0; q < 4; ++q) s[nt][q] = 0.f;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = (cb * NT + nt) * 32 + i32;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int y = y0 + 4 * w + 2 * mt + (row >> 4), x = x0 + (row & 15);
                if (y >= H || x >= W) continue;
                float v = sgn * acc[mt][nt][r];
                const size_t o = ((size_t)(n * H + y) * W + x) * p.Cout + co;
                if constexpr (RES) v += p.residual[o];
                if (p.relu) v = fmaxf(v, 0.f);
                p.out[o] = v;
                s[nt][0] += v;
                s[nt][1] += v * v;
                if (p.gstats) {
                    s[nt][2] += v;
                    if constexpr (VG) {  // (the n-tile's source: uniform over the wave)
                        const float xv = (cb * NT + nt) * 32 >= p.C0
                                             ? p.gx1[((size_t)(n * p.H1 + p.ymap[y]) * p.W1 + p.xmap[x]) * p.C1 + (co - p.C0)]
                                             : p.gx[((size_t)(n * H + y) * W + x) * p.C0 + co];
                        s[nt][3] += v * xv;
                    } else {
                        s[nt][3] += v * p.gx[o];
                    }
                }
            }
    }
    if (p.out_stats || p.gstats) c2s_flush_stats<NT>(p, reinterpret_cast<float*>(lds), s, n, cb, t);  // (the loop ended on a barrier)
}

template <int NT, int V, bool RES = false>
int c2s_conv_launch_as(const C2sParams& p, long long blocks, hipStream_t stream) {
    U3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&c2s_conv_kernel<NT, V, RES>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                c2s::LDS_BYTES));
    hipLaunchKernelGGL((c2s_conv_kernel<NT, V, RES>), dim3((unsigned)blocks), dim3(256), c2s::LDS_BYTES, stream, p);
    U3D_LAUNCH_CHECK();
    return 0;
}

// the one launcher of u3d_conv2d_f32s (vmode 0 / 1), u3d_conv2d_f32s_dgrad (vmode 0 / 2) and u3d_conv2d_f32s_res (vmode 0 with
// p.residual: the RES variants); K contraction, Nn produced channels
int c2s_conv_launch(const char* who, C2sParams p, int vmode, u3d_stream_t stream) {
    p.nchunks = p.Cin / c2s::CC;
    p.ntg = p.Cout / 32;
    const int nt = p.ntg % 2 == 0 ? 2 : 1;  // by the channel count alone: a shape runs the same variant on every grid
    p.ncb = p.ntg / nt;
    p.ty = (int)wf_cdiv(p.H, c2s::TY);
    p.tx = (int)wf_cdiv(p.W, c2s::TX);
    p.wpart = c2s_part_elems(p.Cin, p.Cout) / 8;
    const long long blocks = (long long)p.N * p.ty * p.tx * p.ncb;
    U3D_REQUIRE(blocks < (1LL << 31), "%s: grid too large", who);
    hipStream_t s = (hipStream_t)stream;
    if (p.residual) return nt == 2 ? c2s_conv_launch_as<2, 0, true>(p, blocks, s) : c2s_conv_launch_as<1, 0, true>(p, blocks, s);
    if (nt == 2) return vmode == 0 ? c2s_conv_launch_as<2, 0>(p, blocks, s) : vmode == 1 ? c2s_conv_launch_as<2, 1>(p, blocks, s)
                                                                                         : c2s_conv_launch_as<2, 2>(p, blocks, s);
    return vmode == 0 ? c2s_conv_launch_as<1, 0>(p, blocks, s) : vmode == 1 ? c2s_conv_launch_as<1, 1>(p, blocks, s)
                                                                            : c2s_conv_launch_as<1, 2>(p, blocks, s);
}

// =================================================================================================
// weight gradient: dw[co][ci][tap] = sum_{n,y,x} dz[n,y,x,co] * g[n, y + ky - 1, x + kx - 1, ci], g = affine(x), zero padded.
// MFMA: M = 32 output channels (A = dz), N = 32 input channels (B = g), K = 16 pixels of one tile row.
struct C2sWParams {
    const float* x;       // (N,H,W,Cin); VC: the skip half (N,H,W,C0)
    const float* x1;      // VC: the low-res half (N,H1,W1,C1)
    const int32_t* ymap;
    const int32_t* xmap;
    const float* affine;  // (N,Cin,2) or null
    const float* dz;      // (N,H,W,Cout)
    float* ws;            // [nsplit][9][Cout][Cin]
    int N, H, W, Cin, Cout;
    int C0, C1, H1, W1;
    int ty, tx, ncob, ncib, ntiles, tps;
};

template <bool VC>
__global__ __launch_bounds__(576) void c2s_wgrad_kernel(const C2sWParams p) {
    using namespace c2s;
    extern __shared__ __attribute__((aligned(16))) char lds_c2sw[];
    char* const lds = lds_c2sw;
    const int t = threadIdx.x, l = t & 63, w = t >> 6, h = l >> 5, i32 = l & 31;
    int b = blockIdx.x;
    const int cib = b % p.ncib;
    b /= p.ncib;
    const int cob = b % p.ncob;
    const int split = b / p.ncob;
    const int ci0 = cib * 32, co0 = cob * 32;
    const int tile0 = split * p.tps, tile1 = min(p.ntiles, tile0 + p.tps);
    const int H = p.H, W = p.W, Cin = p.Cin, Cout = p.Cout;
    char* const gl = lds + W_G;
    char* const dzl = lds + W_DZ;
    const int ky = w / 3, kx = w % 3;  // this wave's tap

    // the block's running sum of this wave's tap; a tile's MFMA chain starts from zero and is closed into it with VALU adds
    f32x16 tot;
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] = 0.f;

    // transposed-read lane offset: lane l receives channel (l & 31) of the 8 pixels 8 * (l >> 5) .. + 7
    const int g4 = l >> 4, sidx = l & 15;
    const int lane_off = (8 * (g4 >> 1) + (sidx >> 2)) * WPP + (16 * (g4 & 1) + 4 * (sidx & 3)) * 2;

    // a tile's operands in registers (raw fp32: the next tile's are in flight during this tile's MFMAs), then split and staged
    f32x4 rg[W_GIT][2], rd[W_DIT][2];
    bool okg[W_GIT], okd[W_DIT];
    const float* aff_n = nullptr;
    auto load_tile = [&](int tile) {
        int tt = tile;
        const int txi = tt % p.tx;
        tt /= p.tx;
        const int tyi = tt % p.ty;
        const int n = tt / p.ty;
        const int y0 = tyi * TY, x0 = txi * TX;
        aff_n = p.affine != nullptr ? p.affine + (size_t)n * Cin * 2 : nullptr;
#pragma unroll
        for (int k = 0; k < W_GIT; ++k) {
            const int item = t + W_THREADS * k;
            const int q = item & 3, pix = item >> 2;
            const int hy = pix / HX, hx = pix - (pix / HX) * HX;
            const int gy = y0 - 1 + hy, gxx = x0 - 1 + hx;
            okg[k] = item < W_GITEMS && gy >= 0 && gy < H && gxx >= 0 && gxx < W;
            rg[k][0] = rg[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (okg[k]) {
                const float* src;
                if constexpr (VC) {  // (the cell's source: block-uniform)
                    src = (ci0 >= p.C0 ? p.x1 + ((size_t)(n * p.H1 + p.ymap[gy]) * p.W1 + p.xmap[gxx]) * p.C1 + (ci0 - p.C0)
                                       : p.x + ((size_t)(n * H + gy) * W + gxx) * p.C0 + ci0) + 8 * q;
                } else {
                    src = p.x + ((size_t)(n * H + gy) * W + gxx) * Cin + ci0 + 8 * q;
                }
                rg[k][0] = u3d_ldq(src);
                rg[k][1] = u3d_ldq(src + 4);
            }
        }
#pragma unroll
        for (int k = 0; k < W_DIT; ++k) {
            const int item = t + W_THREADS * k;
            const int q = item & 3, pix = item >> 2;
            const int y = y0 + (pix >> 4), x = x0 + (pix & 15);
            okd[k] = item < W_DITEMS && y < H && x < W;
            rd[k][0] = rd[k][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (okd[k]) {
                const float* src = p.dz + ((size_t)(n * H + y) * W + x) * Cout + co0 + 8 * q;
                rd[k][0] = u3d_ldq(src);
                rd[k][1] = u3d_ldq(src + 4);
            }
        }
    };
    auto store_tile = [&](bool neg) {
        wf_bf16x8 oh, om, ol;
#pragma unroll
        for (int k = 0; k < W_GIT; ++k) {
            const int item = t + W_THREADS * k;
            if (item >= W_GITEMS) continue;
            const float* aff = (aff_n != nullptr && okg[k]) ? aff_n + (ci0 + 8 * (item & 3)) * 2 : nullptr;
            wf_split8(rg[k][0], rg[k][1], aff, okg[k], false, oh, om, ol);
            char* const dst = gl + (item >> 2) * WPP + 16 * (item & 3);
            *reinterpret_cast<wf_bf16x8*>(dst) = oh;
            *reinterpret_cast<wf_bf16x8*>(dst + W_GPART) = om;
            *reinterpret_cast<wf_bf16x8*>(dst + 2 * W_GPART) = ol;
        }
#pragma unroll
        for (int k = 0; k < W_DIT; ++k) {
            const int item = t + W_THREADS * k;
            if (item >= W_DITEMS) continue;
            wf_split8(rd[k][0], rd[k][1], nullptr, okd[k], neg, oh, om, ol);
            char* const dst = dzl + (item >> 2) * WPP + 16 * (item & 3);
            *reinterpret_cast<wf_bf16x8*>(dst) = oh;
            *reinterpret_cast<wf_bf16x8*>(dst + W_DPART) = om;
            *reinterpret_cast<wf_bf16x8*>(dst + 2 * W_DPART) = ol;
        }
    };
    load_tile(tile0);
    for (int tile = tile0; tile < tile1; ++tile) {
        const bool neg = ((tile - tile0) & 1) != 0;  // dz carries (-1)^(tile - tile0): see the header comment
        store_tile(neg);
        __syncthreads();
        if (tile + 1 < tile1) load_tile(tile + 1);
        // tap (ky, kx) pairs dz pixel (py, px) with halo pixel (py + ky, px + kx): one 16-pixel row per K step, 16 rows x 6 products in
        // ONE accumulator, closed into tot
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 2
        for (int row = 0; row < TY; ++row) {
            wf_bf16x8 a[3], g[3];  // [part]
            const char* const ab = dzl + row * TX * WPP + lane_off;
            const char* const gb = gl + ((row + ky) * HX + kx) * WPP + lane_off;
#pragma unroll
            for (int pa = 0; pa < 3; ++pa) a[pa] = wf_tr_frag(ab + pa * W_DPART);
#pragma unroll
            for (int pb = 0; pb < 3; ++pb) g[pb] = wf_tr_frag(gb + pb * W_GPART);
#pragma unroll
            for (int cls = 0; cls < 6; ++cls) {
                constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, PB[6] = {2, 0, 1, 1, 0, 0};
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[PA[cls]], g[PB[cls]], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[r] = neg ? tot[r] - acc[r] : tot[r] + acc[r];
        __syncthreads();
    }

    // ---- this block's cell of its slot [tap][Cout][Cin]: register r = output channel (r & 3) + 8 (r >> 2) + 4h, lane column = ci
    const size_t mat = (size_t)Cout * Cin;
    float* const dst = p.ws + (size_t)split * 9 * mat + (size_t)(ky * 3 + kx) * mat;
    const int ci = ci0 + i32;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        dst[(size_t)co * Cin + ci] = tot[r];
    }
}

// dw[(co * Cin + ci) * 9 + tap] = the slots' [tap][co][ci] added: thread (e, q) adds the q-th of four contiguous slot ranges in slot order,
// thread (e, 0) adds the four in order.  64 elements per block.
__global__ __launch_bounds__(256) void c2s_wreduce_kernel(const float* __restrict__ ws, int nsplit, long long mat, float* __restrict__ dw) {
    __shared__ float part[c2s::RED_PARTS][64];
    const long long total = 9 * mat;
    const int e = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int per = (nsplit + c2s::RED_PARTS - 1) / c2s::RED_PARTS;
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
            const long long cc = i - tap * mat;  // co * Cin + ci
            dw[cc * 9 + tap] = sum;
        }
        __syncthreads();
    }
}

struct C2sWPlan {
    int ty, tx, ncob, ncib, ntiles, tps, nsplit;
};

// one block per CU over the launch (9 waves, 111360 bytes of LDS: one block is resident per CU); ONE function for the launcher and the
// workspace size.  max_slots > 0: no more splits than that many workspace slots hold
C2sWPlan c2s_wplan(int device, int N, int H, int W, int Cin, int Cout, long long max_slots = 0) {
    C2sWPlan pl;
    pl.ty = (int)wf_cdiv(H, c2s::TY);
    pl.tx = (int)wf_cdiv(W, c2s::TX);
    pl.ncob = Cout / 32;
    pl.ncib = Cin / 32;
    pl.ntiles = N * pl.ty * pl.tx;
    const long long cells = (long long)pl.ncob * pl.ncib;
    const long long target = wf_cu_count(device);
    long long ns = std::max<long long>(1, std::min<long long>(pl.ntiles, wf_cdiv(target, cells)));
    if (max_slots > 0) ns = std::min(ns, max_slots);
    pl.tps = (int)wf_cdiv(pl.ntiles, ns);
    pl.nsplit = (int)wf_cdiv(pl.ntiles, pl.tps);
    return pl;
}

}  // namespace

extern "C" int u3d_conv2d_f32s_supported(int K, int Nn) { return c2s_fwd_ok(K, Nn) ? 1 : 0; }

extern "C" int u3d_conv2d_wgrad_f32s_supported(int Cin, int Cout) { return c2s_wgrad_ok(Cin, Cout) ? 1 : 0; }

extern "C" long long u3d_packed_weight2d_f32s_elems(int Cin, int Cout, int mode) {
    if (mode != 0 && mode != 1) return 0;
    return 3 * (mode == 0 ? c2s_part_elems(Cin, Cout) : c2s_part_elems(Cout, Cin));
}

extern "C" int u3d_pack_weights2d_f32s(int device, u3d_stream_t stream, const float* w, int Cout, int Cin, int mode, void* packed) {
    U3D_ENTER(device);
    U3D_REQUIRE(w && packed && (mode == 0 || mode == 1), "u3d_pack_weights2d_f32s: bad argument");
    const int K = mode == 0 ? Cin : Cout, Nn = mode == 0 ? Cout : Cin;
    U3D_REQUIRE(c2s_fwd_ok(K, Nn), "u3d_pack_weights2d_f32s: mode %d of a (%d -> %d) weight is outside the split envelope (contraction %% 16, "
                "produced %% 32)", mode, Cin, Cout);
    U3D_REQUIRE(wf_aligned(packed), "u3d_pack_weights2d_f32s: the image must be 16-byte aligned");
    const long long per = c2s_part_elems(K, Nn);
    long long blocks = wf_cdiv(per, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(c2s_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, Cin, mode, Nn / 32, per,
                       reinterpret_cast<__bf16*>(packed));
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_conv2d_f32s(int device, u3d_stream_t stream, const float* p0, const float* p1, const int32_t* ymap, const int32_t* xmap,
                               int C0, int C1, int H1, int W1, const float* affine, const void* packed_w, float* out, int N, int H, int W,
                               int Cout, int relu, double* out_stats, int stat_reps) {
    U3D_ENTER(device);
    const bool virt = p1 != nullptr || C1 != 0;
    U3D_REQUIRE(C0 > 0 && C1 >= 0 && c2s_fwd_ok(C0 + C1, Cout),
                "u3d_conv2d_f32s: (%d + %d -> %d) channels are outside the split envelope (Cin %% 16, Cout %% 32)", C0, C1, Cout);
    U3D_REQUIRE(!virt || c2s_vsrc_ok(p1, ymap, xmap, C0, C1, H1, W1),
                "u3d_conv2d_f32s: a virtual source needs C0 %% 32 == 0, C1 %% 32 == 0 (got %d, %d), p1, ymap / xmap and H1, W1 > 0", C0, C1);
    U3D_REQUIRE(p0 && packed_w && out && stat_reps >= 1 && c2s_dims_ok(N, H, W), "u3d_conv2d_f32s: bad argument (N * H * W must be < 2^31)");
    U3D_REQUIRE(wf_aligned(p0) && wf_aligned(p1) && wf_aligned(affine) && wf_aligned(packed_w) && wf_aligned(out),
                "u3d_conv2d_f32s: pointers must be 16-byte aligned");
    C2sParams p = {};
    p.x = p0, p.x1 = p1, p.ymap = ymap, p.xmap = xmap;
    p.affine = affine;
    p.wp = reinterpret_cast<const wf_bf16x8*>(packed_w);
    p.out = out;
    p.out_stats = out_stats;
    p.N = N, p.H = H, p.W = W, p.Cin = C0 + C1, p.Cout = Cout;
    p.C0 = C0, p.C1 = C1, p.H1 = H1, p.W1 = W1;
    p.relu = relu ? 1 : 0;
    p.stat_reps = stat_reps;
    return c2s_conv_launch("u3d_conv2d_f32s", p, virt ? 1 : 0, stream);
}

extern "C" int u3d_conv2d_f32s_res(int device, u3d_stream_t stream, const float* x, const float* affine, const void* packed_w, float* out,
                                   int N, int H, int W, int Cin, int Cout, int relu, double* out_stats, int stat_reps, const float* residual) {
    U3D_ENTER(device);
    U3D_REQUIRE(c2s_fwd_ok(Cin, Cout), "u3d_conv2d_f32s_res: (%d -> %d) channels are outside the split envelope (Cin %% 16, Cout %% 32)", Cin,
                Cout);
    U3D_REQUIRE(residual != nullptr, "u3d_conv2d_f32s_res: residual is NULL (u3d_conv2d_f32s is the convolution without one)");
    U3D_REQUIRE(x && packed_w && out && stat_reps >= 1 && c2s_dims_ok(N, H, W), "u3d_conv2d_f32s_res: bad argument (N * H * W must be < 2^31)");
    U3D_REQUIRE(wf_aligned(x) && wf_aligned(affine) && wf_aligned(packed_w) && wf_aligned(out) && wf_aligned(residual),
                "u3d_conv2d_f32s_res: pointers must be 16-byte aligned");
    C2sParams p = {};
    p.x = x;
    p.affine = affine;
    p.wp = reinterpret_cast<const wf_bf16x8*>(packed_w);
    p.out = out;
    p.out_stats = out_stats;
    p.residual = residual;
    p.N = N, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout;
    p.C0 = Cin;
    p.relu = relu ? 1 : 0;
    p.stat_reps = stat_reps;
    return c2s_conv_launch("u3d_conv2d_f32s_res", p, 0, stream);
}

extern "C" int u3d_conv2d_f32s_dgrad(int device, u3d_stream_t stream, const float* dz, const void* packed_w, float* dg, int N, int H, int W,
                                     int Cout, const float* gx0, const float* gx1, const int32_t* ymap, const int32_t* xmap, int C0, int C1,
                                     int H1, int W1, double* gstats, int stat_reps) {
    U3D_ENTER(device);
    const bool virt = gx1 != nullptr || C1 != 0;
    U3D_REQUIRE(C0 > 0 && C1 >= 0 && c2s_fwd_ok(Cout, C0 + C1),
                "u3d_conv2d_f32s_dgrad: (%d + %d -> %d) channels are outside the split envelope (Cout %% 16, Cin %% 32)", C0, C1, Cout);
    U3D_REQUIRE(!virt || (C0 % 32 == 0 && C1 % 32 == 0 && C1 > 0 && H1 > 0 && W1 > 0),
                "u3d_conv2d_f32s_dgrad: a virtual gx needs C0 %% 32 == 0, C1 %% 32 == 0 (got %d, %d) and H1, W1 > 0", C0, C1);
    U3D_REQUIRE(dz && packed_w && dg && stat_reps >= 1 && c2s_dims_ok(N, H, W),
                "u3d_conv2d_f32s_dgrad: bad argument (N * H * W must be < 2^31)");
    U3D_REQUIRE(!gstats || (gx0 && (!virt || (gx1 && ymap && xmap))), "u3d_conv2d_f32s_dgrad: gstats needs gx (both halves and ymap / xmap "
                "of a virtual one)");
    U3D_REQUIRE(wf_aligned(dz) && wf_aligned(packed_w) && wf_aligned(dg) && wf_aligned(gx0) && wf_aligned(gx1),
                "u3d_conv2d_f32s_dgrad: pointers must be 16-byte aligned");
    C2sParams p = {};
    p.x = dz;
    p.wp = reinterpret_cast<const wf_bf16x8*>(packed_w);
    p.out = dg;
    p.gstats = gstats;
    p.gx = gstats ? gx0 : nullptr, p.gx1 = gstats ? gx1 : nullptr, p.ymap = ymap, p.xmap = xmap;
    p.N = N, p.H = H, p.W = W, p.Cin = Cout, p.Cout = C0 + C1;
    p.C0 = C0, p.C1 = C1, p.H1 = H1, p.W1 = W1;
    p.stat_reps = stat_reps;
    return c2s_conv_launch("u3d_conv2d_f32s_dgrad", p, (virt && gstats) ? 2 : 0, stream);
}

extern "C" long long u3d_wgrad2d_f32s_workspace_floats(int N, int H, int W, int Cin, int Cout) {
    if (!c2s_wgrad_ok(Cin, Cout) || !c2s_dims_ok(N, H, W)) return 0;
    return (long long)c2s_wplan(wf_current_device(), N, H, W, Cin, Cout).nsplit * 9 * Cin * Cout;
}

extern "C" int u3d_conv2d_wgrad_f32s(int device, u3d_stream_t stream, const float* p0, const float* p1, const int32_t* ymap,
                                     const int32_t* xmap, int C0, int C1, int H1, int W1, const float* affine, const float* dz, float* dw,
                                     int N, int H, int W, int Cout, float* workspace, long long workspace_floats) {
    U3D_ENTER(device);
    const bool virt = p1 != nullptr || C1 != 0;
    const int Cin = C0 + C1;
    U3D_REQUIRE(C0 > 0 && C1 >= 0 && c2s_wgrad_ok(Cin, Cout),
                "u3d_conv2d_wgrad_f32s: (%d + %d -> %d) channels are outside the split weight gradient's envelope (both %% 32)", C0, C1, Cout);
    U3D_REQUIRE(!virt || c2s_vsrc_ok(p1, ymap, xmap, C0, C1, H1, W1),
                "u3d_conv2d_wgrad_f32s: a virtual source needs C0 %% 32 == 0, C1 %% 32 == 0 (got %d, %d), p1, ymap / xmap and H1, W1 > 0", C0,
                C1);
    U3D_REQUIRE(p0 && dz && dw && workspace && c2s_dims_ok(N, H, W),
                "u3d_conv2d_wgrad_f32s: bad argument (the workspace is always needed; N * H * W must be < 2^31)");
    U3D_REQUIRE(wf_aligned(p0) && wf_aligned(p1) && wf_aligned(affine) && wf_aligned(dz) && wf_aligned(workspace),
                "u3d_conv2d_wgrad_f32s: pointers must be 16-byte aligned");
    const long long slot = (long long)9 * Cin * Cout;
    U3D_REQUIRE(workspace_floats >= slot, "u3d_conv2d_wgrad_f32s: workspace too small (%lld floats; one slot is %lld)", workspace_floats, slot);
    const C2sWPlan pl = c2s_wplan(device, N, H, W, Cin, Cout, workspace_floats / slot);
    C2sWParams p = {};
    p.x = p0, p.x1 = p1, p.ymap = ymap, p.xmap = xmap;
    p.affine = affine;
    p.dz = dz;
    p.ws = workspace;
    p.N = N, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout;
    p.C0 = C0, p.C1 = C1, p.H1 = H1, p.W1 = W1;
    p.ty = pl.ty, p.tx = pl.tx, p.ncob = pl.ncob, p.ncib = pl.ncib, p.ntiles = pl.ntiles, p.tps = pl.tps;
    const long long blocks = (long long)pl.nsplit * pl.ncob * pl.ncib;
    U3D_REQUIRE(blocks < (1LL << 31), "u3d_conv2d_wgrad_f32s: grid too large");
    if (virt) {
        U3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&c2s_wgrad_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    c2s::W_LDS_BYTES));
        hipLaunchKernelGGL(c2s_wgrad_kernel<true>, dim3((unsigned)blocks), dim3(c2s::W_THREADS), c2s::W_LDS_BYTES, (hipStream_t)stream, p);
    } else {
        U3D_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&c2s_wgrad_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    c2s::W_LDS_BYTES));
        hipLaunchKernelGGL(c2s_wgrad_kernel<false>, dim3((unsigned)blocks), dim3(c2s::W_THREADS), c2s::W_LDS_BYTES, (hipStream_t)stream, p);
    }
    U3D_LAUNCH_CHECK();
    long long rb = wf_cdiv(slot, 64);
    if (rb > 8192) rb = 8192;
    hipLaunchKernelGGL(c2s_wreduce_kernel, dim3((unsigned)rb), dim3(256), 0, (hipStream_t)stream, workspace, pl.nsplit, slot / 9, dw);
    U3D_LAUNCH_CHECK();
    return 0;
}
