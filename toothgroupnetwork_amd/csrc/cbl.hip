// cbl.hip -- one decoder stage of the contrastive-boundary criterion (heads.ContrastHead.point_contrast, losses.py) as fused kernels:
//   tgn_cbl_stage_forward   distances to the K-1 listed neighbours, the soft nearest-neighbour sums, the stage loss and, per pair,
//                           the weight the backward multiplies the latent difference with
//   tgn_cbl_stage_backward  the gradient of the latent features, every row gathered by its owner
// The (m, K-1, C) tensor of latent differences is never formed: the forward keeps one (m, K-1) float per pair, the backward reads
// the feature rows again (3 MB at 24 000 x 32, resident in L2).  Forward: one wave per point, lane = neighbour slot, every lane
// streams its neighbour's row with 16-byte loads.  Backward: one lane per 16-byte piece of a row, 64 / LP points per wave; a point
// adds its own K-1 pairs and then the pairs that name it (the caller's reverse lists), so nothing is scattered: no float atomics,
// every row stored once, the same inputs give the same bits.  The sum over points is loss.hip's: float64, wave -> LDS -> per-block
// partials in the caller's workspace -> a finishing kernel, rounded to float32 once.
// Arithmetic: float32 with each operation rounded (-ffp-contract=off), correctly rounded sqrtf and division, the accurate expf / logf.
#include "dispatch.h"

namespace tgn {

constexpr int kCblThreads = 256, kCblWaves = kCblThreads / kWave;
constexpr int kCblPointsPerWave = 4, kCblPointsPerBlock = kCblWaves * kCblPointsPerWave;   // forward: 16 points per workgroup
constexpr int kCblMaxK1 = kWave - 1, kCblMaxC = 128;
constexpr float kCblEps = 1e-12f;    // basic_operators._eps
constexpr float kCblWeight = 0.1f;   // default.yaml `weight: w.1`: the backward's float32 factor
constexpr double kCblWeight64 = 0.1;  // the forward's, applied to the float64 sum

// butterflies over lane distances 32, 16, .., 1: every lane ends with the same bits
__device__ __forceinline__ float cbl_wave_sum(float v) {
    for (int d = kWave / 2; d > 0; d >>= 1) v = v + __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ float cbl_wave_min(float v) {
    for (int d = kWave / 2; d > 0; d >>= 1) v = fminf(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ double cbl_wave_sum(double v) {
    for (int d = kWave / 2; d > 0; d >>= 1) v = v + __shfl_xor(v, d);
    return v;
}

// grid ceil(m / 16).  C = 0: c_rt channels (any multiple of 4); otherwise C channels, the same arithmetic unrolled.
// partials (gridDim.x, 2) float64: the block's sum of per-point values and its number of contributing points.
template <int C>
__global__ void __launch_bounds__(kCblThreads) cbl_stage_forward_kernel(int m, int k1, int c_rt, const float *__restrict__ f,
                                                                        const int *__restrict__ idx,
                                                                        const long long *__restrict__ labels,
                                                                        float *__restrict__ pair_w, double *__restrict__ partials,
                                                                        int *__restrict__ err) {
    __shared__ double s_sum[kCblWaves];
    __shared__ int s_cnt[kCblWaves];
    const int c4 = (C ? C : c_rt) / 4;
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    const bool active = lane < k1;
    double acc = 0.0;     // wave-uniform: this wave's points, in point order
    int cnt = 0;
    bool bad = false;
    for (int t = 0; t < kCblPointsPerWave; ++t) {
        const long long i = (long long)blockIdx.x * kCblPointsPerBlock + wave * kCblPointsPerWave + t;   // wave-uniform
        if (i >= m) break;
        const long long lab_i = labels[i];
        const long long q = i * k1 + lane;             // < 2^31 for an active lane
        float d = INFINITY;
        bool same = false;
        if (active) {
            int nb = idx[q];
            if ((unsigned)nb >= (unsigned)m) nb = 0, bad = true;     // the gather family's convention: point 0, and the error word
            const float4 *a = (const float4 *)(f + (size_t)i * (4 * c4)), *b = (const float4 *)(f + (size_t)nb * (4 * c4));
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll 8
            for (int g = 0; g < c4; ++g) {
                const float4 x = a[g], y = b[g];
                const float t0 = x.x - y.x, t1 = x.y - y.y, t2 = x.z - y.z, t3 = x.w - y.w;
                s0 = s0 + t0 * t0, s1 = s1 + t1 * t1, s2 = s2 + t2 * t2, s3 = s3 + t3 * t3;
            }
            d = sqrtf(((s0 + s1) + (s2 + s3)) + kCblEps);
            same = labels[nb] == lab_i;
        }
        const float dmin = cbl_wave_min(d);
        const float e = active ? expf(dmin - d) : 0.0f;
        const float neg = cbl_wave_sum(e), pos = cbl_wave_sum(same ? e : 0.0f);
        const int npos = __popcll(__ballot(same));
        const bool on = npos > 0 && npos < k1;         // a neighbour of the point's own label and one of another
        const float r = pos / neg, re = r + kCblEps;
        if (active) pair_w[q] = on ? (e * ((same ? 1.0f : 0.0f) - r)) / ((neg * re) * d) : 0.0f;
        if (on) acc += (double)(-logf(re)), ++cnt;
    }
    if (lane == 0) s_sum[wave] = acc, s_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        double v = 0.0, n = 0.0;
        for (int w = 0; w < kCblWaves; ++w) v += s_sum[w], n += (double)s_cnt[w];
        partials[2 * (size_t)blockIdx.x] = v;
        partials[2 * (size_t)blockIdx.x + 1] = n;
    }
    if (__syncthreads_or(bad) && tid == 0 && err) atomicOr(err, kIndexErrGather);
}

// One wave.  Lane l adds the partials of blocks l, l + 64, .. in that order, then the butterfly.  nblocks = 0: loss 0, count 0.
__global__ void __launch_bounds__(kWave) cbl_stage_finish_kernel(int nblocks, const double *__restrict__ partials, float *__restrict__ loss,
                                                                 long long *__restrict__ count) {
    double v = 0.0, n = 0.0;
    for (int g = threadIdx.x; g < nblocks; g += kWave) v += partials[2 * (size_t)g], n += partials[2 * (size_t)g + 1];
    v = cbl_wave_sum(v), n = cbl_wave_sum(n);
    if (threadIdx.x == 0) {
        *count = (long long)n;
        *loss = (float)(kCblWeight64 * v / (n > 1.0 ? n : 1.0));
    }
}

// grid ceil(m / (256 / LP)): LP lanes per point, lane q of them the channels 4q .. 4q+3 (idle where q >= c4).
template <int LP>
__global__ void __launch_bounds__(kCblThreads) cbl_stage_backward_kernel(int m, int k1, int c4, const float4 *__restrict__ f,
                                                                         const int *__restrict__ idx, const float *__restrict__ pair_w,
                                                                         const long long *__restrict__ count,
                                                                         const int *__restrict__ rev_start,
                                                                         const int *__restrict__ rev_pair,
                                                                         const float *__restrict__ grad_loss, float4 *__restrict__ grad_f,
                                                                         int *__restrict__ err) {
    const long long i = (long long)blockIdx.x * (kCblThreads / LP) + threadIdx.x / LP;
    const int q = threadIdx.x % LP;
    bool bad = false;
    if (i < m && q < c4) {
        const long long n = *count;
        const float s = (grad_loss[0] * kCblWeight) / (float)(n > 1 ? n : 1);
        const int pairs = m * k1;                      // < 2^31
        const float4 fi = f[(size_t)i * c4 + q];
        float4 a = {0.0f, 0.0f, 0.0f, 0.0f};
        const int row = (int)i * k1;
        for (int j = 0; j < k1; ++j) {                 // the point's own pairs, in slot order
            const float w = pair_w[row + j];
            if (w == 0.0f) continue;                   // a pair without weight is not read
            int nb = idx[row + j];
            if ((unsigned)nb >= (unsigned)m) nb = 0, bad = true;
            const float4 fj = f[(size_t)nb * c4 + q];
            a.x = a.x + w * (fi.x - fj.x), a.y = a.y + w * (fi.y - fj.y), a.z = a.z + w * (fi.z - fj.z), a.w = a.w + w * (fi.w - fj.w);
        }
        int beg = rev_start[i], end = rev_start[i + 1];
        if (beg < 0 || end > pairs) beg = beg < 0 ? 0 : beg, end = end > pairs ? pairs : end, bad = true;
        for (int t = beg; t < end; ++t) {              // the pairs that name the point, in list order
            const int p = rev_pair[t];
            if ((unsigned)p >= (unsigned)pairs) {
                bad = true;
                continue;
            }
            const float w = pair_w[p];
            if (w == 0.0f) continue;
            const float4 fs = f[(size_t)(p / k1) * c4 + q];
            a.x = a.x - w * (fs.x - fi.x), a.y = a.y - w * (fs.y - fi.y), a.z = a.z - w * (fs.z - fi.z), a.w = a.w - w * (fs.w - fi.w);
        }
        grad_f[(size_t)i * c4 + q] = float4{s * a.x, s * a.y, s * a.z, s * a.w};
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0 && err) atomicOr(err, kIndexErrGather);
}

static int cbl_blocks(int m) { return (int)(((long long)m + kCblPointsPerBlock - 1) / kCblPointsPerBlock); }

// The sizes the kernels exist for; checked before anything touches the device.
static int cbl_check_sizes(const char *who, int m, int k1, int c) {
    if (m < 0) {
        set_error("%s: bad arguments (m=%d; need m >= 0)", who, m);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (k1 < 1 || k1 > kCblMaxK1) {
        set_error("%s: k1 = %d unsupported (1 <= k1 <= %d: one lane of a wave per neighbour slot)", who, k1, kCblMaxK1);
        return TGN_ERR_UNSUPPORTED;
    }
    if (c < 4 || c > kCblMaxC || c % 4) {
        set_error("%s: c = %d unsupported (a multiple of 4, 4 <= c <= %d)", who, c, kCblMaxC);
        return TGN_ERR_UNSUPPORTED;
    }
    if ((long long)m * k1 >= (1ll << 31)) {
        set_error("%s: m * k1 = %lld unsupported (pair numbers are 32-bit: m * k1 < 2^31)", who, (long long)m * k1);
        return TGN_ERR_UNSUPPORTED;
    }
    return TGN_OK;
}

}  // namespace tgn

using namespace tgn;

TGN_API size_t tgn_cbl_stage_workspace_bytes(int m) { return m < 1 ? 0 : (size_t)cbl_blocks(m) * 2 * sizeof(double); }

TGN_API int tgn_cbl_stage_forward(int m, int k1, int c, const float *f, const int *idx, const long long *labels, float *loss,
                                  long long *count, float *pair_w, void *workspace, size_t ws_bytes, tgn_stream_t stream) {
    const char *who = "tgn_cbl_stage_forward";
    if (const int rc = cbl_check_sizes(who, m, k1, c)) return rc;
    if (!loss || !count || (m > 0 && (!f || !idx || !labels || !pair_w || !workspace || ws_bytes < tgn_cbl_stage_workspace_bytes(m))) ||
        ((uintptr_t)f & 15)) {
        set_error("%s: bad arguments (m=%d ws_bytes=%zu; need non-NULL pointers, f 16-byte aligned, ws_bytes >= "
                  "tgn_cbl_stage_workspace_bytes(m))", who, m, ws_bytes);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    const int blocks = cbl_blocks(m);
    double *partials = (double *)workspace;
    if (m > 0) {
        int *err = index_error_word((hipStream_t)stream);
        if (!err) {
            set_error("%s: cannot allocate the error word", who);
            return TGN_ERR_LAUNCH;
        }
        // c = 32 (the criterion's latent width), 64 and 128 unrolled; every other multiple of 4 through the run-time loop
        const int cc = c == 32 || c == 64 || c == 128 ? c : 0;
        if (!dispatch_int<0, 32, 64, 128>(cc, [&](auto C) {
                hipLaunchKernelGGL(cbl_stage_forward_kernel<decltype(C)::value>, dim3(blocks), dim3(kCblThreads), 0, (hipStream_t)stream,
                                   m, k1, c, f, idx, labels, pair_w, partials, err);
            }))
            return dispatch_miss(who, "c", c);
    }
    hipLaunchKernelGGL(cbl_stage_finish_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, blocks, partials, loss, count);
    return check_launch(who);
}

TGN_API int tgn_cbl_stage_backward(int m, int k1, int c, const float *f, const int *idx, const float *pair_w, const long long *count,
                                   const int *rev_start, const int *rev_pair, const float *grad_loss, float *grad_f,
                                   tgn_stream_t stream) {
    const char *who = "tgn_cbl_stage_backward";
    if (const int rc = cbl_check_sizes(who, m, k1, c)) return rc;
    if (m == 0) return TGN_OK;
    if (!f || !idx || !pair_w || !count || !rev_start || !rev_pair || !grad_loss || !grad_f || ((uintptr_t)f & 15) ||
        ((uintptr_t)grad_f & 15)) {
        set_error("%s: bad arguments (m=%d; need non-NULL pointers, f and grad_f 16-byte aligned)", who, m);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    int *err = index_error_word((hipStream_t)stream);
    if (!err) {
        set_error("%s: cannot allocate the error word", who);
        return TGN_ERR_LAUNCH;
    }
    const int c4 = c / 4;
    int lp = 1;                                        // lanes per point: the power of two that holds c / 4 pieces
    while (lp < c4) lp *= 2;
    if (!dispatch_int<1, 2, 4, 8, 16, 32>(lp, [&](auto LP) {
            constexpr int per_block = kCblThreads / decltype(LP)::value;
            hipLaunchKernelGGL(cbl_stage_backward_kernel<decltype(LP)::value>, dim3((unsigned)(((long long)m + per_block - 1) / per_block)), dim3(kCblThreads), 0,
                               (hipStream_t)stream, m, k1, c4, (const float4 *)f, idx, pair_w, count, rev_start, rev_pair, grad_loss,
                               (float4 *)grad_f, err);
        }))
        return dispatch_miss(who, "lanes per point", lp);
    return check_launch(who);
}
