// linear_max.hip -- a pointwise linear layer fused with the max over the points (PointNet's stn.conv3, fstn.conv3 and feat.conv3,
// pointnet_utils.py:29-32 / 69-72 / 127-128; DGCNN's conv6, dgcnn.py:117-118), eval mode with BatchNorm folded:
//
//   out[b, c] = max_{n < N} act( (sum_{k < K} x[b, k, n] * Wt[k, c]) + shift[c] )
//
// The (B, C, N) activation tensor the reference writes and reads once (98 MB per 24 000-point scan at C = 1024) never exists: the
// max is taken on the MFMA accumulators.  The tile scheme is sa_point_transform_kernel's (sa.hip): a 128-point x 128-channel tile
// per 256-thread block, 2 x 2 tiles of v_mfma_f32_32x32x2_f32 per wave, K in steps of 16 through LDS with the next K-tile in flight
// in registers during the MFMAs.  x is channel-first, so an A-tile row is 128 consecutive floats of one channel: no transpose.
// A block walks the point tiles of its chunk with the running maximum in registers and writes ONE partial row of 128 channels into
// the caller's workspace; tgn_linear_act_max's second launch reduces the chunks.  No float atomics, no allocation, no
// synchronisation.
//
// Arithmetic: the sum is the fp32 MFMA's fma chain over k ascending from 0 (K is padded to a multiple of 16 with zero PRODUCTS, which
// leave the chain as it is), shift is added once, the activation is applied before the max.  Each candidate depends on its own point
// and channel alone and the max is exact, so the result depends neither on B nor on how the launch cuts N.  A NaN candidate gives NaN
// (nan_max below), as torch.max does.  Rows at or beyond N never take part (a zero row would evaluate to act(shift[c])), and the
// running maximum starts at -inf.
#include "tgn_common.h"

namespace tgn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kLmTM = 128, kLmTN = 128, kLmTK = 16, kLmPad = 4;
constexpr int kLmTargetBlocks = 512;   // two blocks for each of the 256 CUs

// torch.max's order: NaN beats everything, and stays
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

struct LmPlan {
    int ncb;      // 128-channel blocks
    int tpc;      // point tiles per chunk
    int chunks;   // point chunks: partial rows per (scan, channel)
};

// The number of point chunks follows from B * ceil(C / 128) alone (and N's tile count), so that one scan at C = 1024 still fills
// the chip.  Host only.
static LmPlan lm_plan(int B, int N, int C) {
    LmPlan p;
    p.ncb = (C + kLmTN - 1) / kLmTN;
    const long long tiles = ((long long)N + kLmTM - 1) / kLmTM;
    const long long base = (long long)B * p.ncb;
    long long want = (kLmTargetBlocks + base - 1) / base;
    if (want < 1) want = 1;
    if (want > tiles) want = tiles;
    p.tpc = (int)((tiles + want - 1) / want);
    p.chunks = (int)((tiles + p.tpc - 1) / p.tpc);
    return p;
}

// grid: ncb * chunks * B blocks rounded up to a multiple of 8, in XCD order with the channel block fastest: the blocks that read
// one point tile run on one XCD and share its L2.  part: (B, chunks, C).
__global__ __launch_bounds__(256) void linear_act_max_kernel(int N, int K, int C, int ncb, int tpc, int chunks, unsigned total,
                                                              const float *__restrict__ x, const float *__restrict__ Wt,
                                                              const float *__restrict__ shift, int act, float slope,
                                                              float *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[kLmTK][kLmTM + kLmPad];
    __shared__ __attribute__((aligned(16))) float Bs[kLmTK][kLmTN + kLmPad];
    __shared__ float red[2][kLmTN];
    const unsigned logical = xcd_block_order();
    if (logical >= total) return;   // (block-uniform: in front of every barrier)
    const int cb = (int)(logical % (unsigned)ncb);
    const unsigned rest = logical / (unsigned)ncb;
    const int chunk = (int)(rest % (unsigned)chunks);
    const int b = (int)(rest / (unsigned)chunks);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv >> 1, wn = wv & 1;
    const int lo = lane & 31, hi = lane >> 5;
    const int col0 = cb * kLmTN;
    const long long tile_first = (long long)chunk * tpc;
    const long long all_tiles = ((long long)N + kLmTM - 1) / kLmTM;
    const int ntiles = (int)((all_tiles - tile_first < tpc) ? all_tiles - tile_first : tpc);   // >= 1 by lm_plan
    const int ksteps = (K + kLmTK - 1) / kLmTK;
    const float *xb = x + (size_t)b * K * N;
    // global -> register staging, the same shape for both operands: thread (k = tid >> 4, j = (tid & 15) * 8) holds 8 consecutive
    // points of channel k0 + k and 8 consecutive columns of weight row k0 + k
    const int sk = tid >> 4, sj = (tid & 15) * 8;
    const bool x4 = (N & 3) == 0 && ((uintptr_t)x & 15) == 0;
    const bool w4 = (C & 3) == 0 && ((uintptr_t)Wt & 15) == 0;
    f32x4 ra[2], rb[2];
    auto fetch = [&](int it) {
        const int t = it / ksteps, ks = it - t * ksteps;
        const int kr = ks * kLmTK + sk;
        const long long n = (tile_first + t) * kLmTM + sj;
        const float *xr = xb + (size_t)kr * N;
        if (kr < K && x4 && n + 8 <= N) {
            ra[0] = *(const f32x4 *)(xr + n);
            ra[1] = *(const f32x4 *)(xr + n + 4);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) ra[i >> 2][i & 3] = (kr < K && n + i < N) ? xr[n + i] : 0.0f;
        }
        const int c = col0 + sj;
        const float *wr = Wt + (size_t)kr * C;
        if (kr < K && w4 && c + 8 <= C) {
            rb[0] = *(const f32x4 *)(wr + c);
            rb[1] = *(const f32x4 *)(wr + c + 4);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) rb[i >> 2][i & 3] = (kr < K && c + i < C) ? wr[c + i] : 0.0f;
        }
    };
    float sh[2], best[2];
#pragma unroll
    for (int j2 = 0; j2 < 2; ++j2) {
        const int col = col0 + wn * 64 + j2 * 32 + lo;
        sh[j2] = col < C ? shift[col] : 0.0f;
        best[j2] = -__builtin_inff();
    }
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j2][r] = 0.0f;
    const int iters = ntiles * ksteps;
    fetch(0);
    int ks = 0, t = 0;
    for (int it = 0; it < iters; ++it) {
        __syncthreads();   // the previous tile has been consumed
        *(f32x4 *)&As[sk][sj] = ra[0];
        *(f32x4 *)&As[sk][sj + 4] = ra[1];
        *(f32x4 *)&Bs[sk][sj] = rb[0];
        *(f32x4 *)&Bs[sk][sj + 4] = rb[1];
        __syncthreads();
        if (it + 1 < iters) fetch(it + 1);   // in flight during the MFMAs below (the next point tile's first step included)
#pragma unroll
        for (int s = 0; s < kLmTK / 2; ++s) {
            const float a0 = As[2 * s + hi][wm * 64 + lo], a1 = As[2 * s + hi][wm * 64 + 32 + lo];
            const float b0 = Bs[2 * s + hi][wn * 64 + lo], b1 = Bs[2 * s + hi][wn * 64 + 32 + lo];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (++ks < ksteps) continue;
        // this point tile is complete: shift, activation, max over the lane's 16 points per 32 x 32 tile, then a fresh accumulator
        const long long row0 = (tile_first + t) * kLmTM + wm * 64 + 4 * hi;
        const bool whole = (tile_first + t + 1) * kLmTM <= N;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[i][j2][r] + sh[j2];
                    if (act == 1) v = v < 0.0f ? 0.0f : v;              // (keeps a NaN)
                    else if (act == 2) v = v > 0.0f ? v : v * slope;
                    const long long row = row0 + i * 32 + (r & 3) + 8 * (r >> 2);
                    if (whole || row < N) best[j2] = nan_max(best[j2], v);
                    acc[i][j2][r] = 0.0f;
                }
        ks = 0;
        ++t;
    }
    // across the two lane halves (rows 4 * hi + ...), then across the two waves that share these columns
#pragma unroll
    for (int j2 = 0; j2 < 2; ++j2) best[j2] = nan_max(best[j2], __shfl_xor(best[j2], 32));
    if (wm == 1 && hi == 0) {
        red[wn][lo] = best[0];
        red[wn][32 + lo] = best[1];
    }
    __syncthreads();
    if (wm == 0 && hi == 0) {
        float *dst = part + ((size_t)b * chunks + chunk) * C;
#pragma unroll
        for (int j2 = 0; j2 < 2; ++j2) {
            const int col = col0 + wn * 64 + j2 * 32 + lo;
            if (col < C) dst[col] = nan_max(best[j2], red[wn][j2 * 32 + lo]);
        }
    }
}

// out[b, c] = max over the chunks of part[b, chunk, c]
__global__ __launch_bounds__(256) void linear_act_max_finish_kernel(long long BC, int C, int chunks, const float *__restrict__ part,
                                                                     float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const long long b = i / C;
    const int c = (int)(i - b * C);
    const float *p = part + (size_t)b * chunks * C + c;
    float m = -__builtin_inff();
    for (int k = 0; k < chunks; ++k) m = nan_max(m, p[(size_t)k * C]);
    out[i] = m;
}

static bool lm_check_shape(const char *fn, int B, int N, int K, int C) {
    if (B < 1) { set_error("%s: B must be at least 1 (got %d)", fn, B); return false; }
    if (N < 1) { set_error("%s: N must be at least 1 (got %d)", fn, N); return false; }
    if (K < 1 || K > 512) { set_error("%s: K must be 1 .. 512 (got %d)", fn, K); return false; }
    if (C < 1) { set_error("%s: C must be at least 1 (got %d)", fn, C); return false; }
    return true;
}

}  // namespace tgn

using namespace tgn;

TGN_API size_t tgn_linear_act_max_workspace_bytes(int B, int N, int K, int C) {
    if (!lm_check_shape("tgn_linear_act_max_workspace_bytes", B, N, K, C)) return 0;
    return (size_t)B * lm_plan(B, N, C).chunks * C * sizeof(float);
}

TGN_API int tgn_linear_act_max(int B, int N, int K, int C, const float *x, const float *Wt, const float *shift, int act, float slope,
                               float *out, void *ws, size_t ws_bytes, tgn_stream_t stream) {
    if (!lm_check_shape("tgn_linear_act_max", B, N, K, C)) return TGN_ERR_UNSUPPORTED;
    if (act < 0 || act > 2) {
        set_error("tgn_linear_act_max: act must be 0 (identity), 1 (relu) or 2 (leaky relu) (got %d)", act);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (!x || !Wt || !shift || !out || !ws) {
        set_error("tgn_linear_act_max: null pointer (%s)", !x ? "x" : !Wt ? "Wt" : !shift ? "shift" : !out ? "out" : "ws");
        return TGN_ERR_INVALID_ARGUMENT;
    }
    const LmPlan p = lm_plan(B, N, C);
    const size_t need = (size_t)B * p.chunks * C * sizeof(float);
    if (ws_bytes < need) {
        set_error("tgn_linear_act_max: ws_bytes %zu is short of tgn_linear_act_max_workspace_bytes = %zu", ws_bytes, need);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    const long long total = (long long)B * p.chunks * p.ncb, BC = (long long)B * C;
    if (total > 0x7FFFFFF0LL || (BC + 255) / 256 > 0x7FFFFFFFLL) {
        set_error("tgn_linear_act_max: B * C too large for one launch (B %d, C %d)", B, C);
        return TGN_ERR_UNSUPPORTED;
    }
    const unsigned grid = (unsigned)((total + 7) / 8 * 8);
    hipLaunchKernelGGL(linear_act_max_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, N, K, C, p.ncb, p.tpc, p.chunks,
                       (unsigned)total, x, Wt, shift, act, slope, (float *)ws);
    int rc = check_launch("linear_act_max_kernel");
    if (rc != TGN_OK) return rc;
    hipLaunchKernelGGL(linear_act_max_finish_kernel, dim3((unsigned)((BC + 255) / 256)), dim3(256), 0, (hipStream_t)stream, BC, C,
                       p.chunks, (const float *)ws, out);
    return check_launch("linear_act_max_finish_kernel");
}
