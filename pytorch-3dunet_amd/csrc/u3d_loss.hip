// u3d_loss.hip — BCEDiceLoss / DiceLoss(sigmoid) / BCEWithLogitsLoss on the logits, fused, and the
// multi-class losses (softmax cross entropy, weighted CE, softmax / none / generalized Dice) further down.
//
// Reference: pytorch3dunet/unet3d/losses.py — BCEDiceLoss :187-201 (= nn.BCEWithLogitsLoss() + alpha * DiceLoss()),
// DiceLoss / _AbstractDiceLoss :84-127 (sigmoid normalisation, 1 - mean_c dice_c), compute_per_channel_dice :11-37
// (dice_c = 2 * w_c * sum(p*t) / clamp(sum(p^2) + sum(t^2), eps), sums over (N, spatial) per channel, flatten :253-271).
// The stock path launches ~15 elementwise / reduction kernels plus a permute+contiguous copy and keeps 6 full-size
// temporaries for autograd; here:
//   pass 1  one read of (logits, target): 4 sums per block (BCE terms, p*t, p^2, t^2) as per-block partials in double
//   pass 2  one block: the partials summed in a fixed order (bit-reproducible), the scalar loss + per-channel gradient
//           coefficients (dL/dp_c = a_c*t + b_c*p is affine)
//   pass 3  backward: one read of (logits, target), one write of dlogits, scaled by the upstream scalar ON DEVICE
// logits / target are (N, C, V) contiguous fp32 — the reference's NCDHW, which is what the model's head writes.
#include "u3d_common.h"

namespace {

__device__ __forceinline__ void sigmoid_softplus(float x, float& p, float& sp_pos) {
    // p = sigmoid(x); sp_pos = max(x,0) + log1p(exp(-|x|)) = softplus(x)  (BCE-with-logits = softplus(x) - x*t)
    const float e = expf(-fabsf(x));
    const float r = 1.f / (1.f + e);
    p = x >= 0.f ? r : e * r;
    sp_pos = fmaxf(x, 0.f) + log1pf(e);
}

// The options of the *_ex entry points (the reference's SkipLastTargetChannelWrapper / MaskingLossWrapper / pos_weight, losses.py:40-88,
// :312).  The kernels below are templates on EX: EX = false is the option-free code of the plain entry points, unchanged.
struct LossOpt {
    long long t_stride;  // elements between the targets of consecutive samples (dense inside a sample); N*... contiguous otherwise
    int use_mask;        // t == ignore: compute with x = 0, t = 0 and write dx = 0 (MaskingLossWrapper's arithmetic)
    float ignore;
    float pos_weight;  // BCE term: -(pw t log p + (1 - t) log(1 - p)); 1 = the plain form
};

// MaskingLossWrapper on one element: true (and x = t = 0) where the fp32 target equals the ignore value
template <bool EX>
__device__ __forceinline__ bool mask_elem(const LossOpt& o, float& xv, float& tv) {
    if (EX && o.use_mask && tv == o.ignore) {
        xv = 0.f;
        tv = 0.f;
        return true;
    }
    return false;
}

// grid (blocks_per_row, N*C), 256 threads; row = one (n, c) plane of V voxels
template <bool EX>
__global__ __launch_bounds__(256) void loss_sums_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                        int C, long long V, int vec, double* __restrict__ sums, LossOpt o) {
    const int row = blockIdx.y;
    const int c = row % C;
    const float* x = logits + (size_t)row * V;
    const float* t = EX ? target + (size_t)(row / C) * o.t_stride + (size_t)c * V : target + (size_t)row * V;
    float s_bce = 0.f, s_pt = 0.f, s_pp = 0.f, s_tt = 0.f;
    auto acc = [&](float xv, float tv) {
        float p, sp;
        mask_elem<EX>(o, xv, tv);
        sigmoid_softplus(xv, p, sp);
        if (EX && o.pos_weight != 1.f)  // torch's stable form: (1 - t) x + (1 + (pw - 1) t) softplus(-x)
            s_bce += (1.f - tv) * xv + (1.f + (o.pos_weight - 1.f) * tv) * (sp - xv);
        else
            s_bce += sp - xv * tv;
        s_pt += p * tv;
        s_pp += p * p;
        s_tt += tv * tv;
    };
    const long long stride = (long long)gridDim.x * 256;
    if (vec) {
        const long long nq = V >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nq; i += stride) {
            const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
            const f32x4 tv = reinterpret_cast<const f32x4*>(t)[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc(xv[e], tv[e]);
        }
        for (long long i = (nq << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += stride) acc(x[i], t[i]);
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += stride) acc(x[i], t[i]);
    }
    // block reduction: wave butterflies, then 4 waves through LDS (fixed order), one f64 atomic per sum and block
    __shared__ float red[4][4];
    float v[4] = {s_bce, s_pt, s_pp, s_tt};
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v[k] += __shfl_xor(v[k], m);
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (l == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) red[w][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        // per-block partial, plain store (round 6: 512 blocks adding to the same four doubles were 10 of the kernel's 15 us — a
        // same-address f64 atomic retires every 19.5 ns, tools/atomic_bench.hip; the one-block second pass sums them in a fixed order)
        const int k = threadIdx.x;
        sums[((size_t)row * gridDim.x + blockIdx.x) * 4 + k] = ((double)red[0][k] + (double)red[1][k]) + ((double)red[2][k] + (double)red[3][k]);
    }
}

// one block of 256 threads: the partials [N*C rows][per_row blocks][4] -> loss[0] and coef[2*C + 1] = {a_c, b_c}_c, k_bce
__global__ __launch_bounds__(256) void loss_finalize_kernel(const double* __restrict__ partial, int N, int per_row,
                                                            const float* __restrict__ weight, int C, double count, float w_bce,
                                                            float w_dice, float eps, float* __restrict__ loss, float* __restrict__ coef) {
    __shared__ double red[256][4];
    __shared__ double acc_bce, acc_dice;
    const int t = threadIdx.x;
    if (t == 0) acc_bce = 0.0, acc_dice = 0.0;
    for (int c = 0; c < C; ++c) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = t; i < N * per_row; i += 256) {
            const int n = i / per_row, bx = i - n * per_row;
            const double* pp = partial + ((size_t)(n * C + c) * per_row + bx) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] += pp[k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) red[t][k] = v[k];
        __syncthreads();
        for (int m = 128; m > 0; m >>= 1) {  // fixed-order tree
            if (t < m)
#pragma unroll
                for (int k = 0; k < 4; ++k) red[t][k] += red[t + m][k];
            __syncthreads();
        }
        if (t == 0) {
            const double I = red[0][1], A = red[0][2], B = red[0][3];
            const double wc = weight ? (double)weight[c] : 1.0;
            const double raw = A + B;
            const bool clamped = raw < (double)eps;  // torch.clamp(min=eps): gradient 0 through the clamped branch
            const double den = clamped ? (double)eps : raw;
            acc_bce += red[0][0];
            acc_dice += 2.0 * wc * I / den;
            // L_dice = w_dice * (1 - (1/C) sum_c dice_c);  d dice_c / dp = 2 wc t / den - (clamped ? 0 : 2 wc I * 2p / den^2)
            const double k = -(double)w_dice / C;
            coef[2 * c + 0] = (float)(k * 2.0 * wc / den);
            coef[2 * c + 1] = clamped ? 0.f : (float)(-k * 4.0 * wc * I / (den * den));
        }
        __syncthreads();
    }
    if (t == 0) {
        coef[2 * C] = (float)((double)w_bce / count);
        loss[0] = (float)((double)w_bce * acc_bce / count + (double)w_dice * (1.0 - acc_dice / C));
    }
}

// dlogits = g * [ k_bce * (p - t) + (a_c * t + b_c * p) * p * (1 - p) ],  g = *grad_out (device scalar) or 1
template <bool EX>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                       const float* __restrict__ coef, const float* __restrict__ grad_out,
                                                       int C, long long V, int vec, float* __restrict__ dlogits, LossOpt o) {
    const int row = blockIdx.y;
    const int c = row % C;
    const float g = grad_out ? grad_out[0] : 1.f;
    const float a = coef[2 * c] * g, b = coef[2 * c + 1] * g, kb = coef[2 * C] * g;
    const float* x = logits + (size_t)row * V;
    const float* t = EX ? target + (size_t)(row / C) * o.t_stride + (size_t)c * V : target + (size_t)row * V;
    float* d = dlogits + (size_t)row * V;
    auto one = [&](float xv, float tv) {
        float p, sp;
        if (mask_elem<EX>(o, xv, tv)) return 0.f;
        sigmoid_softplus(xv, p, sp);
        if (EX && o.pos_weight != 1.f)
            return kb * ((1.f - tv) - (1.f + (o.pos_weight - 1.f) * tv) * (1.f - p)) + (a * tv + b * p) * p * (1.f - p);
        return kb * (p - tv) + (a * tv + b * p) * p * (1.f - p);
    };
    const long long stride = (long long)gridDim.x * 256;
    if (vec) {
        const long long nq = V >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nq; i += stride) {
            const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
            const f32x4 tv = reinterpret_cast<const f32x4*>(t)[i];
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = one(xv[e], tv[e]);
            reinterpret_cast<f32x4*>(d)[i] = o;
        }
        for (long long i = (nq << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += stride) d[i] = one(x[i], t[i]);
    } else {
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < V; i += stride) d[i] = one(x[i], t[i]);
    }
}

inline bool rows_vec_ok(const void* a, const void* b, const void* c, long long V) {
    return V % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

inline dim3 loss_grid(int rows, long long V) {
    // ~4 float4 per thread; keep >= ~1024 blocks in flight when the tensor is large enough
    long long per_row = (V + 4095) / 4096;
    if (per_row < 1) per_row = 1;
    if (per_row > 4096) per_row = 4096;
    return dim3((unsigned)per_row, (unsigned)rows);
}

}  // namespace

extern "C" long long u3d_bce_dice_scratch_doubles(int N, int C, int64_t V) {
    if (N <= 0 || C <= 0 || V <= 0) return 0;
    return (long long)N * C * loss_grid(N * C, V).x * 4;
}

extern "C" int u3d_bce_dice_fwd(int device, u3d_stream_t stream, const float* logits, const float* target,
                                const float* weight, int N, int C, int64_t V, float w_bce, float w_dice, float eps,
                                double* sums, float* loss, float* coef) {
    U3D_ENTER(device);
    U3D_REQUIRE(logits && target && sums && loss && coef && N > 0 && C > 0 && V > 0, "u3d_bce_dice_fwd: bad argument");
    U3D_REQUIRE((long long)N * C < 65536, "u3d_bce_dice_fwd: N*C must be < 65536");
    hipStream_t st = (hipStream_t)stream;
    const int vec = rows_vec_ok(logits, target, logits, V) ? 1 : 0;
    const dim3 grid = loss_grid(N * C, V);
    hipLaunchKernelGGL(loss_sums_kernel<false>, grid, dim3(256), 0, st, logits, target, C, (long long)V, vec, sums, LossOpt{});
    U3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, sums, N, (int)grid.x, weight, C, (double)N * C * (double)V,
                       w_bce, w_dice, eps, loss, coef);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_bce_dice_bwd(int device, u3d_stream_t stream, const float* logits, const float* target,
                                const float* coef, const float* grad_out, int N, int C, int64_t V, float* dlogits) {
    U3D_ENTER(device);
    U3D_REQUIRE(logits && target && coef && dlogits && N > 0 && C > 0 && V > 0, "u3d_bce_dice_bwd: bad argument");
    U3D_REQUIRE((long long)N * C < 65536, "u3d_bce_dice_bwd: N*C must be < 65536");
    const int vec = rows_vec_ok(logits, target, dlogits, V) ? 1 : 0;
    hipLaunchKernelGGL(loss_bwd_kernel<false>, loss_grid(N * C, V), dim3(256), 0, (hipStream_t)stream, logits, target, coef,
                       grad_out, C, (long long)V, vec, dlogits, LossOpt{});
    U3D_LAUNCH_CHECK();
    return 0;
}

// the same with the options of LossOpt; the target of sample n starts at target + n * t_batch_stride (>= C*V), dense inside
extern "C" int u3d_bce_dice_fwd_ex(int device, u3d_stream_t stream, const float* logits, const float* target,
                                   const float* weight, int N, int C, int64_t V, float w_bce, float w_dice, float eps,
                                   int64_t t_batch_stride, int use_mask, float ignore_value, float pos_weight, double* sums,
                                   float* loss, float* coef) {
    U3D_ENTER(device);
    U3D_REQUIRE(logits && target && sums && loss && coef && N > 0 && C > 0 && V > 0, "u3d_bce_dice_fwd_ex: bad argument");
    U3D_REQUIRE((long long)N * C < 65536, "u3d_bce_dice_fwd_ex: N*C must be < 65536");
    U3D_REQUIRE(t_batch_stride >= (int64_t)C * V, "u3d_bce_dice_fwd_ex: t_batch_stride must be >= C*V");
    hipStream_t st = (hipStream_t)stream;
    const int vec = rows_vec_ok(logits, target, logits, V) && t_batch_stride % 4 == 0 ? 1 : 0;
    const dim3 grid = loss_grid(N * C, V);
    const LossOpt o{(long long)t_batch_stride, use_mask ? 1 : 0, ignore_value, pos_weight};
    hipLaunchKernelGGL(loss_sums_kernel<true>, grid, dim3(256), 0, st, logits, target, C, (long long)V, vec, sums, o);
    U3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, sums, N, (int)grid.x, weight, C, (double)N * C * (double)V,
                       w_bce, w_dice, eps, loss, coef);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_bce_dice_bwd_ex(int device, u3d_stream_t stream, const float* logits, const float* target,
                                   const float* coef, const float* grad_out, int N, int C, int64_t V, int64_t t_batch_stride,
                                   int use_mask, float ignore_value, float pos_weight, float* dlogits) {
    U3D_ENTER(device);
    U3D_REQUIRE(logits && target && coef && dlogits && N > 0 && C > 0 && V > 0, "u3d_bce_dice_bwd_ex: bad argument");
    U3D_REQUIRE((long long)N * C < 65536, "u3d_bce_dice_bwd_ex: N*C must be < 65536");
    U3D_REQUIRE(t_batch_stride >= (int64_t)C * V, "u3d_bce_dice_bwd_ex: t_batch_stride must be >= C*V");
    const int vec = rows_vec_ok(logits, target, dlogits, V) && t_batch_stride % 4 == 0 ? 1 : 0;
    const LossOpt o{(long long)t_batch_stride, use_mask ? 1 : 0, ignore_value, pos_weight};
    hipLaunchKernelGGL(loss_bwd_kernel<true>, loss_grid(N * C, V), dim3(256), 0, (hipStream_t)stream, logits, target, coef,
                       grad_out, C, (long long)V, vec, dlogits, o);
    U3D_LAUNCH_CHECK();
    return 0;
}

// =====================================================================================================================
// Multi-class losses on the logits (losses.py:11-37, :84-184, :204-227 and nn.CrossEntropyLoss, built by :316-319).
// logits (N, C, V) contiguous fp32; a voxel's C values are V apart, so consecutive threads (consecutive voxels) read
// consecutive addresses for every channel.  Every reduction writes per-block partials in double that a one-block
// finalize sums in a fixed order: the loss and the gradient are bit-reproducible.  No float atomics anywhere.
//   softmax CE   pass 1 (Σ w[t]·(lse − x_t), Σ w[t]) per block -> finalize: loss, coef = {w_c}, 1/W
//                backward: dlogits = g·w[t]/W·(softmax − onehot(t)), zero on ignored voxels
//   weighted CE  a channel-sums pass (S_c = Σ softmax_c) -> finalize w_c = (M − S_c)/S_c into coef -> softmax CE
//   Dice family  a channel-sums pass (Σpt, Σp², Σt², Σp, Σt per channel, p normalised) -> finalize: loss and the affine
//                dL/dp_c = a_c·t + b_c·p + k_c -> backward through the normalisation
namespace {

constexpr int MC_K = 5;        // per-channel sums: p*t, p*p, t*t, p, t
constexpr int MC_MAX_C = 1024;  // the head's channel limit
constexpr int MC_NORM_SIGMOID = 0, MC_NORM_SOFTMAX = 1, MC_NORM_NONE = 2;

// per-row block count: ~4 voxels per thread on large problems, one on small ones (a wide head on a small grid), at most 4096
// partial rows and 2^18 (block, channel) pairs in all
inline unsigned mc_blocks_per_row(int N, int C, long long V) {
    const long long vpt = (long long)N * V >= (1LL << 20) ? 4 : 1;
    long long gx = (V + 256 * vpt - 1) / (256 * vpt);
    long long cap = 4096 / N;
    if (cap < 1) cap = 1;
    const long long cap2 = (1LL << 18) / ((long long)N * C);
    if (cap2 < cap) cap = cap2 < 1 ? 1 : cap2;
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    return (unsigned)gx;
}

// channel chunks of the passes that are parallel over channels (grid.z): the voxel's softmax terms are recomputed per chunk
constexpr int MC_CS_CHUNK = 16;  // channel sums: one register accumulator set per channel of the chunk
constexpr int MC_BWD_CHUNK = 64;  // backward kernels
inline unsigned mc_chunks(int C, int chunk) { return (unsigned)((C + chunk - 1) / chunk); }

// max-shifted log-sum-exp terms of one voxel: x points at (n, 0, v); on return sum_c exp(x_c - m) = s
__device__ __forceinline__ void voxel_max_sum(const float* __restrict__ x, long long V, int C, float& m, float& s) {
    m = x[0];
    s = 1.f;
#pragma unroll 4
    for (int c = 1; c < C; ++c) {
        const float xv = x[(size_t)c * V];
        const float mn = fmaxf(m, xv);
        s = s * expf(m - mn) + expf(xv - mn);
        m = mn;
    }
}

// the same with MaskingLossWrapper's element mask: x_c counts as 0 where t_c == ignore (t points at the voxel's target)
__device__ __forceinline__ void voxel_max_sum_masked(const float* __restrict__ x, const float* __restrict__ t, long long V, int C,
                                                     float ignore, float& m, float& s) {
    m = t[0] == ignore ? 0.f : x[0];
    s = 1.f;
#pragma unroll 4
    for (int c = 1; c < C; ++c) {
        const float xv = t[(size_t)c * V] == ignore ? 0.f : x[(size_t)c * V];
        const float mn = fmaxf(m, xv);
        s = s * expf(m - mn) + expf(xv - mn);
        m = mn;
    }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// sum of (a, b) over a 256-thread block, fixed order; valid in thread 0
__device__ __forceinline__ void block_sum2_256(double& a, double& b) {
    __shared__ double red[4][2];
    for (int m = 32; m >= 1; m >>= 1) {
        a += __shfl_xor(a, m);
        b += __shfl_xor(b, m);
    }
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (l == 0) red[w][0] = a, red[w][1] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        a = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        b = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    }
}

// one 256-thread block: tot[q] = sum_b part[b * CK + q] for q < CK, in a fixed order (G threads per q, then G in sequence)
__device__ void reduce_partials(const double* __restrict__ part, int nb, int CK, double* tot) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    if (CK >= 256) {
        for (int q = t; q < CK; q += 256) {
            double s = 0.0;
            for (int b = 0; b < nb; ++b) s += part[(size_t)b * CK + q];
            tot[q] = s;
        }
    } else {
        const int G = 256 / CK, q = t / G, j = t - q * G;
        double s = 0.0;
        if (q < CK)
            for (int b = j; b < nb; b += G) s += part[(size_t)b * CK + q];
        red[t] = s;
        __syncthreads();
        if (q < CK && j == 0) {
            double a = 0.0;
            for (int i = 0; i < G; ++i) a += red[t + i];
            tot[q] = a;
        }
    }
    __syncthreads();
}

// grid (blocks_per_row, N), 256 threads: per block (Σ w[t]·nll, Σ w[t]) over the non-ignored voxels; a label outside [0, C)
// is never used as an index and makes the loss sum NaN
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                     const float* weight, int C, long long V, long long ignore,
                                                     double* __restrict__ part, long long t_stride) {
    const int n = blockIdx.y;
    const float* x = logits + (size_t)n * C * V;
    const int64_t* tg = target + (size_t)n * t_stride;  // V for a contiguous (N, V) target
    double sl = 0.0, sw = 0.0;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
        const long long t = tg[v];
        if (t == ignore) continue;
        if (t < 0 || t >= C) {
            sl = __builtin_nan("");  // the loss only: Σ w stays finite, so the other voxels keep their gradient
            continue;
        }
        float m, s;
        voxel_max_sum(x + v, V, C, m, s);
        const float w = weight ? weight[t] : 1.f;
        sl += (double)(w * (m + logf(s) - x[(size_t)t * V + v]));
        sw += (double)w;
    }
    block_sum2_256(sl, sw);
    if (threadIdx.x == 0) {
        double* p = part + ((size_t)n * gridDim.x + blockIdx.x) * 2;
        p[0] = sl;
        p[1] = sw;
    }
}

// one block: loss = Σ w·nll / Σ w (0/0 = NaN when every voxel is ignored), coef[c] = w_c, coef[C] = 1 / Σ w
__global__ __launch_bounds__(256) void ce_finalize_kernel(const double* __restrict__ part, int nb, const float* weight, int C,
                                                          float* loss, float* coef) {
    __shared__ double tot[2];
    reduce_partials(part, nb, 2, tot);
    if (weight != coef)
        for (int c = threadIdx.x; c < C; c += 256) coef[c] = weight ? weight[c] : 1.f;
    if (threadIdx.x == 0) {
        loss[0] = (float)(tot[0] / tot[1]);
        coef[C] = (float)(1.0 / tot[1]);
    }
}

// dlogits = g · coef[t] · coef[C] · (softmax − onehot(t)); 0 on ignored voxels, NaN (in range) for labels outside [0, C);
// grid (blocks_per_row, N, channel chunks)
__global__ __launch_bounds__(256) void ce_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                     const float* __restrict__ coef, const float* __restrict__ grad_out, int C,
                                                     long long V, long long ignore, float* __restrict__ dlogits,
                                                     long long t_stride) {
    const int n = blockIdx.y;
    const float* x = logits + (size_t)n * C * V;
    const int64_t* tg = target + (size_t)n * t_stride;
    float* d = dlogits + (size_t)n * C * V;
    const int c0 = blockIdx.z * MC_BWD_CHUNK, c1 = min(C, c0 + MC_BWD_CHUNK);  // this block's channels
    const float g = (grad_out ? grad_out[0] : 1.f) * coef[C];
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
        const long long t = tg[v];
        if (t == ignore || t < 0 || t >= C) {
            const float z = t == ignore ? 0.f : __builtin_nanf("");
            for (int c = c0; c < c1; ++c) d[(size_t)c * V + v] = z;
            continue;
        }
        float m, s;
        voxel_max_sum(x + v, V, C, m, s);
        const float sc = g * coef[t], inv = 1.f / s;
        for (int c = c0; c < c1; ++c) {
            const float p = expf(x[(size_t)c * V + v] - m) * inv;
            d[(size_t)c * V + v] = sc * (c == t ? p - 1.f : p);
        }
    }
}

// channel sums; grid (blocks_per_row, N, channel chunks of CR), 256 threads; accumulators in registers for the chunk's
// channels [c0, c0 + CR); part[(n*gx + bx)][C][MC_K]
template <int CR, bool EX>
__global__ __launch_bounds__(256) void chan_sums_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                        int C, long long V, int norm, double* __restrict__ part, LossOpt o) {
    const int n = blockIdx.y, c0 = blockIdx.z * CR;
    const int cn = min(CR, C - c0);  // channels of this chunk
    const float* x = logits + (size_t)n * C * V;
    const float* xc = x + (size_t)c0 * V;
    const float* tg = !target ? nullptr : EX ? target + (size_t)n * o.t_stride + (size_t)c0 * V : target + ((size_t)n * C + c0) * V;
    float acc[CR][MC_K];
#pragma unroll
    for (int c = 0; c < CR; ++c)
#pragma unroll
        for (int k = 0; k < MC_K; ++k) acc[c][k] = 0.f;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
        float p[CR];
#pragma unroll
        for (int c = 0; c < CR; ++c) p[c] = c < cn ? xc[(size_t)c * V + v] : 0.f;
        float tt[EX ? CR : 1];  // EX: the chunk's targets, read before the normalisation (the mask zeroes x as well)
        if constexpr (EX) {
#pragma unroll
            for (int c = 0; c < CR; ++c) {
                tt[c] = c < cn ? tg[(size_t)c * V + v] : 0.f;
                mask_elem<true>(o, p[c], tt[c]);
            }
        }
        if (norm == MC_NORM_SOFTMAX) {
            float m, s;
            if (cn == C) {  // the whole voxel is in registers
                m = p[0];
#pragma unroll
                for (int c = 1; c < CR; ++c)
                    if (c < cn) m = fmaxf(m, p[c]);
                s = 0.f;
#pragma unroll
                for (int c = 0; c < CR; ++c)
                    if (c < cn) s += expf(p[c] - m);
            } else if (EX && o.use_mask) {
                voxel_max_sum_masked(x + v, target + (size_t)n * o.t_stride + v, V, C, o.ignore, m, s);
            } else {
                voxel_max_sum(x + v, V, C, m, s);
            }
            const float inv = 1.f / s;
#pragma unroll
            for (int c = 0; c < CR; ++c) p[c] = expf(p[c] - m) * inv;
        } else if (norm == MC_NORM_SIGMOID) {
#pragma unroll
            for (int c = 0; c < CR; ++c) p[c] = sigmoidf_(p[c]);
        }
#pragma unroll
        for (int c = 0; c < CR; ++c)
            if (c < cn) {
                const float t = EX ? tt[EX ? c : 0] : tg ? tg[(size_t)c * V + v] : 0.f;
                acc[c][0] += p[c] * t;
                acc[c][1] += p[c] * p[c];
                acc[c][2] += t * t;
                acc[c][3] += p[c];
                acc[c][4] += t;
            }
    }
    __shared__ float red[4][CR * MC_K];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < CR; ++c)
        if (c < cn)
#pragma unroll
            for (int k = 0; k < MC_K; ++k) {
                float s = acc[c][k];
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
                if (l == 0) red[w][c * MC_K + k] = s;
            }
    __syncthreads();
    double* out = part + ((size_t)n * gridDim.x + blockIdx.x) * C * MC_K + (size_t)c0 * MC_K;
    for (int q = threadIdx.x; q < cn * MC_K; q += 256)
        out[q] = ((double)red[0][q] + (double)red[1][q]) + ((double)red[2][q] + (double)red[3][q]);
}

// one block: w_c = (M − S_c) / S_c (WeightedCrossEntropyLoss._class_weights) into coef[0, C)
__global__ __launch_bounds__(256) void wce_weights_kernel(const double* __restrict__ part, int nb, int C, double M,
                                                          float* __restrict__ coef) {
    __shared__ double tot[MC_MAX_C * MC_K];
    reduce_partials(part, nb, C * MC_K, tot);
    for (int c = threadIdx.x; c < C; c += 256) {
        const double S = tot[c * MC_K + 3];
        coef[c] = (float)((M - S) / S);
    }
}

// one block: the Dice loss and the affine gradient coef[3c..3c+2] = (a_c, b_c, k_c) of dL/dp_c = a_c·t + b_c·p + k_c
__global__ __launch_bounds__(256) void dice_finalize_kernel(const double* __restrict__ part, int nb, int C,
                                                            const float* __restrict__ weight, int generalized, float eps_f,
                                                            double M, float* __restrict__ loss, float* __restrict__ coef) {
    __shared__ double tot[MC_MAX_C * MC_K];
    reduce_partials(part, nb, C * MC_K, tot);
    if (threadIdx.x != 0) return;
    const double eps = (double)eps_f;
    if (!generalized) {
        // compute_per_channel_dice: dice_c = 2 w_c I_c / clamp(P2_c + T2_c, eps); loss = 1 − mean_c dice_c
        double acc = 0.0;
        for (int c = 0; c < C; ++c) {
            const double I = tot[c * MC_K + 0], raw = tot[c * MC_K + 1] + tot[c * MC_K + 2];
            const double wc = weight ? (double)weight[c] : 1.0;
            const bool clamped = raw < eps;  // clamp(min=eps): no gradient through the clamped branch
            const double den = clamped ? eps : raw;
            acc += 2.0 * wc * I / den;
            coef[3 * c + 0] = (float)(-2.0 * wc / (C * den));
            coef[3 * c + 1] = clamped ? 0.f : (float)(4.0 * wc * I / (C * den * den));
            coef[3 * c + 2] = 0.f;
        }
        loss[0] = (float)(1.0 - acc / C);
        return;
    }
    // GeneralizedDiceLoss.dice: w_j = 1 / clamp(T_j², eps) (constant), I = Σ_j w_j I_j, D = Σ_j clamp(w_j (P_j + T_j), eps),
    // loss = 1 − 2 I / D; a single channel becomes the pair (p, 1 − p) / (t, 1 − t)
    const int J = C == 1 ? 2 : C;
    double I = 0.0, D = 0.0;
    for (int j = 0; j < J; ++j) {
        const double* s = tot + (C == 1 ? 0 : j * MC_K);
        const double pt = s[0], P = s[3], T = s[4];
        const double Ij = j == 1 && C == 1 ? M - P - T + pt : pt;
        const double Pj = j == 1 && C == 1 ? M - P : P, Tj = j == 1 && C == 1 ? M - T : T;
        const double w = 1.0 / fmax(Tj * Tj, eps);
        I += w * Ij;
        D += fmax(w * (Pj + Tj), eps);
    }
    loss[0] = (float)(1.0 - 2.0 * I / D);
    // dL/dp_j = −2 w_j t_j / D + 2 I w_j [w_j (P_j + T_j) >= eps] / D²
    double a[2] = {0.0, 0.0}, k[2] = {0.0, 0.0};
    for (int j = 0; j < J; ++j) {
        const double* s = tot + (C == 1 ? 0 : j * MC_K);
        const double P = s[3], T = s[4];
        const double Pj = j == 1 && C == 1 ? M - P : P, Tj = j == 1 && C == 1 ? M - T : T;
        const double w = 1.0 / fmax(Tj * Tj, eps);
        const double aj = -2.0 * w / D, kj = w * (Pj + Tj) < eps ? 0.0 : 2.0 * I * w / (D * D);
        if (C == 1) {
            a[j] = aj, k[j] = kj;
        } else {
            coef[3 * j + 0] = (float)aj;
            coef[3 * j + 1] = 0.f;
            coef[3 * j + 2] = (float)kj;
        }
    }
    if (C == 1) {  // p_1 = 1 − p, t_1 = 1 − t: dL/dp = (a_0 t + k_0) − (a_1 (1 − t) + k_1)
        coef[0] = (float)(a[0] + a[1]);
        coef[1] = 0.f;
        coef[2] = (float)(k[0] - a[1] - k[1]);
    }
}

// dlogits = g · dL/dx through the normalisation: sigmoid p(1−p)·G_c, softmax p_c (G_c − Σ_k p_k G_k), none G_c;
// grid (blocks_per_row, N, channel chunks)
template <bool EX>
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ target,
                                                       const float* __restrict__ coef, const float* __restrict__ grad_out, int C,
                                                       long long V, int norm, float* __restrict__ dlogits, LossOpt o) {
    const int n = blockIdx.y;
    const float* x = logits + (size_t)n * C * V;
    const float* tg = EX ? target + (size_t)n * o.t_stride : target + (size_t)n * C * V;
    float* d = dlogits + (size_t)n * C * V;
    const int c0 = blockIdx.z * MC_BWD_CHUNK, c1 = min(C, c0 + MC_BWD_CHUNK);  // this block's channels
    const float g = grad_out ? grad_out[0] : 1.f;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < V; v += (long long)gridDim.x * 256) {
        if (norm == MC_NORM_SOFTMAX) {
            float m, s;
            if (EX && o.use_mask)
                voxel_max_sum_masked(x + v, tg + v, V, C, o.ignore, m, s);
            else
                voxel_max_sum(x + v, V, C, m, s);
            const float inv = 1.f / s;
            float dot = 0.f;
            for (int c = 0; c < C; ++c) {
                const size_t i = (size_t)c * V + v;
                float xv = x[i], tv = tg[i];
                mask_elem<EX>(o, xv, tv);
                const float p = expf(xv - m) * inv;
                dot += p * (coef[3 * c] * tv + coef[3 * c + 1] * p + coef[3 * c + 2]);
            }
            for (int c = c0; c < c1; ++c) {
                const size_t i = (size_t)c * V + v;
                float xv = x[i], tv = tg[i];
                const bool off = mask_elem<EX>(o, xv, tv);
                const float p = expf(xv - m) * inv;
                const float dv = g * p * (coef[3 * c] * tv + coef[3 * c + 1] * p + coef[3 * c + 2] - dot);
                d[i] = off ? 0.f : dv;
            }
        } else {
            for (int c = c0; c < c1; ++c) {
                const size_t i = (size_t)c * V + v;
                float xv = x[i], tv = tg[i];
                const bool off = mask_elem<EX>(o, xv, tv);
                const float p = norm == MC_NORM_SIGMOID ? sigmoidf_(xv) : xv;
                const float gc = coef[3 * c] * tv + coef[3 * c + 1] * p + coef[3 * c + 2];
                const float dv = g * (norm == MC_NORM_SIGMOID ? gc * p * (1.f - p) : gc);
                d[i] = off ? 0.f : dv;
            }
        }
    }
}

inline long long chan_sums_doubles(int N, int C, long long V) { return (long long)N * mc_blocks_per_row(N, C, V) * C * MC_K; }

// the channel-sums pass; returns the number of partial rows
template <bool EX = false>
inline int launch_chan_sums(hipStream_t st, const float* logits, const float* target, int N, int C, long long V, int norm,
                            double* part, LossOpt o = LossOpt{}) {
    const unsigned gx = mc_blocks_per_row(N, C, V);
    if (C <= 4)
        hipLaunchKernelGGL((chan_sums_kernel<4, EX>), dim3(gx, (unsigned)N, 1), dim3(256), 0, st, logits, target, C, V, norm, part,
                           o);
    else
        hipLaunchKernelGGL((chan_sums_kernel<MC_CS_CHUNK, EX>), dim3(gx, (unsigned)N, mc_chunks(C, MC_CS_CHUNK)), dim3(256), 0, st,
                           logits, target, C, V, norm, part, o);
    return (int)(gx * N);
}

}  // namespace

extern "C" long long u3d_softmax_ce_scratch_doubles(int N, int C, int64_t V) {
    if (N <= 0 || C <= 0 || V <= 0 || C > MC_MAX_C) return 0;
    const long long ce = (long long)N * mc_blocks_per_row(N, 1, V) * 2;
    const long long cs = chan_sums_doubles(N, C, V);
    return ce > cs ? ce : cs;
}

// the target of sample n starts at target + n * t_batch_stride (V for a contiguous (N, V) target)
extern "C" int u3d_softmax_ce_fwd_ex(int device, u3d_stream_t stream, const float* logits, const int64_t* target,
                                     const float* weight, int N, int C, int64_t V, int64_t ignore_index, int auto_weight,
                                     int64_t t_batch_stride, double* scratch, float* loss, float* coef) {
    U3D_ENTER(device);
    U3D_REQUIRE(logits && target && scratch && loss && coef && N > 0 && C > 0 && V > 0, "u3d_softmax_ce_fwd: bad argument");
    U3D_REQUIRE(N < 65536 && C <= MC_MAX_C, "u3d_softmax_ce_fwd: needs N < 65536 and C <= 1024");
    U3D_REQUIRE(!(auto_weight && weight), "u3d_softmax_ce_fwd: auto_weight excludes a weight vector");
    U3D_REQUIRE(t_batch_stride >= V, "u3d_softmax_ce_fwd: t_batch_stride must be >= V");
    hipStream_t st = (hipStream_t)stream;
    if (auto_weight) {
        const int nb = launch_chan_sums(st, logits, nullptr, N, C, (long long)V, MC_NORM_SOFTMAX, scratch);
        U3D_LAUNCH_CHECK();
        hipLaunchKernelGGL(wce_weights_kernel, dim3(1), dim3(256), 0, st, scratch, nb, C, (double)N * (double)V, coef);
        U3D_LAUNCH_CHECK();
        weight = coef;
    }
    const dim3 grid(mc_blocks_per_row(N, 1, V), (unsigned)N);
    hipLaunchKernelGGL(ce_fwd_kernel, grid, dim3(256), 0, st, logits, target, weight, C, (long long)V, (long long)ignore_index,
                       scratch, (long long)t_batch_stride);
    U3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, st, scratch, (int)(grid.x * grid.y), weight, C, loss, coef);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_softmax_ce_fwd(int device, u3d_stream_t stream, const float* logits, const int64_t* target, const float* weight,
                                  int N, int C, int64_t V, int64_t ignore_index, int auto_weight, double* scratch, float* loss,
                                  float* coef) {
    return u3d_softmax_ce_fwd_ex(device, stream, logits, target, weight, N, C, V, ignore_index, auto_weight, V, scratch, loss, coef);
}

extern "C" int u3d_softmax_ce_bwd_ex(int device, u3d_stream_t stream, const float* logits, const int64_t* target,
                                     const float* coef, const float* grad_out, int N, int C, int64_t V, int64_t ignore_index,
                                     int64_t t_batch_stride, float* dlogits) {
    U3D_ENTER(device);
    U3D_REQUIRE(logits && target && coef && dlogits && N > 0 && C > 0 && V > 0, "u3d_softmax_ce_bwd: bad argument");
    U3D_REQUIRE(N < 65536 && C <= MC_MAX_C, "u3d_softmax_ce_bwd: needs N < 65536 and C <= 1024");
    U3D_REQUIRE(t_batch_stride >= V, "u3d_softmax_ce_bwd: t_batch_stride must be >= V");
    const dim3 grid(mc_blocks_per_row(N, 1, V), (unsigned)N, mc_chunks(C, MC_BWD_CHUNK));
    hipLaunchKernelGGL(ce_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, logits, target, coef, grad_out, C, (long long)V,
                       (long long)ignore_index, dlogits, (long long)t_batch_stride);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_softmax_ce_bwd(int device, u3d_stream_t stream, const float* logits, const int64_t* target, const float* coef,
                                  const float* grad_out, int N, int C, int64_t V, int64_t ignore_index, float* dlogits) {
    return u3d_softmax_ce_bwd_ex(device, stream, logits, target, coef, grad_out, N, C, V, ignore_index, V, dlogits);
}

extern "C" long long u3d_dice_scratch_doubles(int N, int C, int64_t V) {
    if (N <= 0 || C <= 0 || V <= 0 || C > MC_MAX_C) return 0;
    return chan_sums_doubles(N, C, V);
}

namespace {

template <bool EX>
int dice_fwd_impl(int device, u3d_stream_t stream, const float* logits, const float* target, const float* weight, int N, int C,
                  int64_t V, int norm, int generalized, float eps, LossOpt o, double* scratch, float* loss, float* coef) {
    U3D_ENTER(device);
    U3D_REQUIRE(logits && target && scratch && loss && coef && N > 0 && C > 0 && V > 0, "u3d_dice_fwd: bad argument");
    U3D_REQUIRE(N < 65536 && C <= MC_MAX_C, "u3d_dice_fwd: needs N < 65536 and C <= 1024");
    U3D_REQUIRE(norm >= MC_NORM_SIGMOID && norm <= MC_NORM_NONE, "u3d_dice_fwd: norm must be 0 (sigmoid), 1 (softmax) or 2 (none)");
    U3D_REQUIRE(!(generalized && weight), "u3d_dice_fwd: the generalized Dice takes no class weight");
    U3D_REQUIRE(o.t_stride >= (long long)C * V, "u3d_dice_fwd: t_batch_stride must be >= C*V");
    hipStream_t st = (hipStream_t)stream;
    const int nb = launch_chan_sums<EX>(st, logits, target, N, C, (long long)V, norm, scratch, o);
    U3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(256), 0, st, scratch, nb, C, weight, generalized ? 1 : 0, eps,
                       (double)N * (double)V, loss, coef);
    U3D_LAUNCH_CHECK();
    return 0;
}

template <bool EX>
int dice_bwd_impl(int device, u3d_stream_t stream, const float* logits, const float* target, const float* coef,
                  const float* grad_out, int N, int C, int64_t V, int norm, LossOpt o, float* dlogits) {
    U3D_ENTER(device);
    U3D_REQUIRE(logits && target && coef && dlogits && N > 0 && C > 0 && V > 0, "u3d_dice_bwd: bad argument");
    U3D_REQUIRE(N < 65536 && C <= MC_MAX_C, "u3d_dice_bwd: needs N < 65536 and C <= 1024");
    U3D_REQUIRE(norm >= MC_NORM_SIGMOID && norm <= MC_NORM_NONE, "u3d_dice_bwd: norm must be 0 (sigmoid), 1 (softmax) or 2 (none)");
    U3D_REQUIRE(o.t_stride >= (long long)C * V, "u3d_dice_bwd: t_batch_stride must be >= C*V");
    const dim3 grid(mc_blocks_per_row(N, 1, V), (unsigned)N, mc_chunks(C, MC_BWD_CHUNK));
    hipLaunchKernelGGL(dice_bwd_kernel<EX>, grid, dim3(256), 0, (hipStream_t)stream, logits, target, coef, grad_out, C, (long long)V,
                       norm, dlogits, o);
    U3D_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int u3d_dice_fwd(int device, u3d_stream_t stream, const float* logits, const float* target, const float* weight,
                            int N, int C, int64_t V, int norm, int generalized, float eps, double* scratch, float* loss,
                            float* coef) {
    return dice_fwd_impl<false>(device, stream, logits, target, weight, N, C, V, norm, generalized, eps,
                                LossOpt{(long long)C * V, 0, 0.f, 1.f}, scratch, loss, coef);
}

extern "C" int u3d_dice_bwd(int device, u3d_stream_t stream, const float* logits, const float* target, const float* coef,
                            const float* grad_out, int N, int C, int64_t V, int norm, float* dlogits) {
    return dice_bwd_impl<false>(device, stream, logits, target, coef, grad_out, N, C, V, norm, LossOpt{(long long)C * V, 0, 0.f, 1.f},
                                dlogits);
}

extern "C" int u3d_dice_fwd_ex(int device, u3d_stream_t stream, const float* logits, const float* target, const float* weight,
                               int N, int C, int64_t V, int norm, int generalized, float eps, int64_t t_batch_stride, int use_mask,
                               float ignore_value, double* scratch, float* loss, float* coef) {
    return dice_fwd_impl<true>(device, stream, logits, target, weight, N, C, V, norm, generalized, eps,
                               LossOpt{(long long)t_batch_stride, use_mask ? 1 : 0, ignore_value, 1.f}, scratch, loss, coef);
}

extern "C" int u3d_dice_bwd_ex(int device, u3d_stream_t stream, const float* logits, const float* target, const float* coef,
                               const float* grad_out, int N, int C, int64_t V, int norm, int64_t t_batch_stride, int use_mask,
                               float ignore_value, float* dlogits) {
    return dice_bwd_impl<true>(device, stream, logits, target, coef, grad_out, N, C, V, norm,
                               LossOpt{(long long)t_batch_stride, use_mask ? 1 : 0, ignore_value, 1.f}, dlogits);
}

// =====================================================================================================================
// Regression losses on (N, C, V) fp32: nn.MSELoss / nn.L1Loss / nn.SmoothL1Loss (mean reduction) and WeightedSmoothL1Loss
// (losses.py:230-250), with the target options of LossOpt.  loss = mean over all N*C*V elements of w * f(x - t):
//   MSE d^2 | L1 |d| (gradient sign(d), sign(0) = 0) | SmoothL1 0.5 d^2 / beta below beta, |d| - 0.5 beta from beta on
//   weighted: w = weight where t < threshold (apply_below) or t >= threshold (otherwise), else 1, on the SmoothL1 value
// forward: one read of (x, t), per-block partials in double, a one-block finalize in a fixed order (bit-reproducible);
// backward: one read of (x, t), one write of dx = g * w * f'(d) / (N*C*V), g the upstream DEVICE scalar.
namespace {

constexpr int REG_MSE = 0, REG_L1 = 1, REG_SMOOTH_L1 = 2, REG_WEIGHTED_SMOOTH_L1 = 3;

struct RegOpt {
    int mode;
    float beta, threshold, weight;
    int below;
};

__device__ __forceinline__ float reg_weight(const RegOpt& r, float tv) {
    if (r.mode != REG_WEIGHTED_SMOOTH_L1) return 1.f;
    return (r.below ? tv < r.threshold : tv >= r.threshold) ? r.weight : 1.f;
}

__device__ __forceinline__ float reg_value(const RegOpt& r, float d) {
    const float z = fabsf(d);
    if (r.mode == REG_MSE) return d * d;
    if (r.mode == REG_L1) return z;
    return z < r.beta ? 0.5f * z * z / r.beta : z - 0.5f * r.beta;
}

__device__ __forceinline__ float reg_slope(const RegOpt& r, float d) {
    const float sgn = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
    if (r.mode == REG_MSE) return 2.f * d;
    if (r.mode == REG_L1) return sgn;
    return fabsf(d) < r.beta ? d / r.beta : sgn;
}

// grid (blocks_per_row, N), 256 threads; row = one sample of M = C*V elements
__global__ __launch_bounds__(256) void reg_sums_kernel(const float* __restrict__ input, const float* __restrict__ target,
                                                       long long M, int vec, RegOpt r, LossOpt o, double* __restrict__ part) {
    const int n = blockIdx.y;
    const float* x = input + (size_t)n * M;
    const float* t = target + (size_t)n * o.t_stride;
    float s = 0.f;
    auto acc = [&](float xv, float tv) {
        mask_elem<true>(o, xv, tv);
        s += reg_weight(r, tv) * reg_value(r, xv - tv);
    };
    const long long stride = (long long)gridDim.x * 256;
    const long long nq = vec ? M >> 2 : 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nq; i += stride) {
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        const f32x4 tv = reinterpret_cast<const f32x4*>(t)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc(xv[e], tv[e]);
    }
    for (long long i = (nq << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += stride) acc(x[i], t[i]);
    double a = (double)s, b = 0.0;
    block_sum2_256(a, b);
    if (threadIdx.x == 0) part[(size_t)n * gridDim.x + blockIdx.x] = a;
}

// one block: loss = sum of the partials (fixed order) / count
__global__ __launch_bounds__(256) void reg_finalize_kernel(const double* __restrict__ part, int nb, double count,
                                                           float* __restrict__ loss) {
    __shared__ double tot[1];
    reduce_partials(part, nb, 1, tot);
    if (threadIdx.x == 0) loss[0] = (float)(tot[0] / count);
}

__global__ __launch_bounds__(256) void reg_bwd_kernel(const float* __restrict__ input, const float* __restrict__ target,
                                                      const float* __restrict__ grad_out, long long M, int vec, float inv_count,
                                                      RegOpt r, LossOpt o, float* __restrict__ dinput) {
    const int n = blockIdx.y;
    const float* x = input + (size_t)n * M;
    const float* t = target + (size_t)n * o.t_stride;
    float* d = dinput + (size_t)n * M;
    const float g = (grad_out ? grad_out[0] : 1.f) * inv_count;
    auto one = [&](float xv, float tv) {
        if (mask_elem<true>(o, xv, tv)) return 0.f;
        return g * reg_weight(r, tv) * reg_slope(r, xv - tv);
    };
    const long long stride = (long long)gridDim.x * 256;
    const long long nq = vec ? M >> 2 : 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nq; i += stride) {
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        const f32x4 tv = reinterpret_cast<const f32x4*>(t)[i];
        f32x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = one(xv[e], tv[e]);
        reinterpret_cast<f32x4*>(d)[i] = ov;
    }
    for (long long i = (nq << 2) + (long long)blockIdx.x * 256 + threadIdx.x; i < M; i += stride) d[i] = one(x[i], t[i]);
}

inline bool reg_args_ok(int N, int C, int64_t V, int64_t t_batch_stride, int mode, float beta) {
    return N > 0 && N < 65536 && C > 0 && V > 0 && t_batch_stride >= (int64_t)C * V && mode >= REG_MSE &&
           mode <= REG_WEIGHTED_SMOOTH_L1 && (mode < REG_SMOOTH_L1 || beta > 0.f);
}

}  // namespace

extern "C" long long u3d_reg_loss_scratch_doubles(int N, int C, int64_t V) {
    if (N <= 0 || C <= 0 || V <= 0) return 0;
    return (long long)N * loss_grid(N, (long long)C * V).x;
}

extern "C" int u3d_reg_loss_fwd(int device, u3d_stream_t stream, const float* input, const float* target, int N, int C, int64_t V,
                                int64_t t_batch_stride, int mode, float beta, float threshold, float weight, int apply_below,
                                int use_mask, float ignore_value, double* scratch, float* loss) {
    U3D_ENTER(device);
    U3D_REQUIRE(input && target && scratch && loss, "u3d_reg_loss_fwd: bad argument");
    U3D_REQUIRE(reg_args_ok(N, C, V, t_batch_stride, mode, beta),
                "u3d_reg_loss_fwd: needs 0 < N < 65536, C, V > 0, t_batch_stride >= C*V, mode 0..3 and beta > 0 for the SmoothL1 modes");
    hipStream_t st = (hipStream_t)stream;
    const long long M = (long long)C * V;
    const int vec = rows_vec_ok(input, target, input, M) && t_batch_stride % 4 == 0 ? 1 : 0;
    const dim3 grid = loss_grid(N, M);
    const RegOpt r{mode, beta, threshold, weight, apply_below ? 1 : 0};
    const LossOpt o{(long long)t_batch_stride, use_mask ? 1 : 0, ignore_value, 1.f};
    hipLaunchKernelGGL(reg_sums_kernel, grid, dim3(256), 0, st, input, target, M, vec, r, o, scratch);
    U3D_LAUNCH_CHECK();
    hipLaunchKernelGGL(reg_finalize_kernel, dim3(1), dim3(256), 0, st, scratch, (int)(grid.x * grid.y), (double)N * (double)M, loss);
    U3D_LAUNCH_CHECK();
    return 0;
}

extern "C" int u3d_reg_loss_bwd(int device, u3d_stream_t stream, const float* input, const float* target, const float* grad_out,
                                int N, int C, int64_t V, int64_t t_batch_stride, int mode, float beta, float threshold, float weight,
                                int apply_below, int use_mask, float ignore_value, float* dinput) {
    U3D_ENTER(device);
    U3D_REQUIRE(input && target && dinput, "u3d_reg_loss_bwd: bad argument");
    U3D_REQUIRE(reg_args_ok(N, C, V, t_batch_stride, mode, beta),
                "u3d_reg_loss_bwd: needs 0 < N < 65536, C, V > 0, t_batch_stride >= C*V, mode 0..3 and beta > 0 for the SmoothL1 modes");
    const long long M = (long long)C * V;
    const int vec = rows_vec_ok(input, target, dinput, M) && t_batch_stride % 4 == 0 ? 1 : 0;
    const RegOpt r{mode, beta, threshold, weight, apply_below ? 1 : 0};
    const LossOpt o{(long long)t_batch_stride, use_mask ? 1 : 0, ignore_value, 1.f};
    hipLaunchKernelGGL(reg_bwd_kernel, loss_grid(N, M), dim3(256), 0, (hipStream_t)stream, input, target, grad_out, M, vec,
                       (float)(1.0 / ((double)N * (double)M)), r, o, dinput);
    U3D_LAUNCH_CHECK();
    return 0;
}
