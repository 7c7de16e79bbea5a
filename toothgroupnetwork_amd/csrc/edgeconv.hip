// edgeconv.hip -- the neighbourhood work of DGCNN (models/modules/dgcnn.py): the feature-space kNN and the eval-mode EdgeConv levels.
//
//   tgn_feature_knn        knn(x, k) (dgcnn.py:4-10) without the N x N matrix: per query row i the k smallest direct-form fp32
//                          distances  acc = acc + t*t, t = x_i[c] - x_j[c], c = 0..D-1 in order (each operation rounded), in ascending
//                          (distance, index) order.  A lane owns one query (its D values in registers), a workgroup owns 256 queries
//                          and one contiguous split of the candidates, staged through LDS in tiles of 128; a running top-k per lane
//                          in registers (sorted 64-bit keys (distance bits << 32 | index), insertion below a threshold).  Splits
//                          fill the GPU at batch 1; their sorted partial lists are merged by key, which is exact: the top k of a
//                          union is the top k of the union of the parts' top k.
//   tgn_edgeconv2_max      max_j lrelu(W2 lrelu(P_j + Q_i) + b2) (conv1+conv2, conv3+conv4 with BatchNorm folded): one wave per query,
//                          32 MFMA rows = the k <= 32 neighbours, the 64 x 64 second layer on v_mfma_f32_32x32x2_f32 with W2 held in
//                          registers for the wave's life.  The (B, 2C, N, k) edge tensor never exists.
//   tgn_edgeconv1_max      max_j lrelu(P_j + Q_i) (conv5): one wave per query, lane = channel.
// Both EdgeConv kernels write channel slices of a channel-first (B, Ctot, N) tensor (the concatenation conv6 reads).  Neighbour
// indices are local to their scan; one outside [0, N) reads point 0 and latches bit 1 of the launch stream's error word
// (tgn_take_index_error).
#include "tgn_common.h"

namespace tgn {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- tgn_feature_knn ----------------------------------------------------------------------------------------------------------
constexpr int kFkThreads = 256, kFkTile = 128, kFkMaxD = 64, kFkMaxK = 32, kFkMaxSplits = 16, kFkMinChunk = 512;

// Insert `key` into the ascending list keys[0..KP): the largest entry drops out.  Slots [0, KP - k) hold 0 and never move (no key
// is below 0), so the live list is keys[KP - k .. KP) and its threshold keys[KP - 1] sits at a compile-time position.
template <int KP>
__device__ __forceinline__ void topk_insert(unsigned long long (&keys)[KP], unsigned long long key) {
#pragma unroll
    for (int p = 0; p < KP; ++p) {
        const unsigned long long a = keys[p];
        const bool lt = key < a;
        keys[p] = lt ? key : a;
        key = lt ? a : key;
    }
}

__device__ __forceinline__ unsigned long long knn_key(float d, int j) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j;   // d >= +0 or NaN: bit order = value order, NaN last
}

// grid (query tiles, splits, B).  part: (B, S, N, k) keys when S > 1; else idx / dist2 directly.
template <int DP, int KP>
__global__ __launch_bounds__(kFkThreads) void feature_knn_kernel(int N, int D, int k, int S, int chunk, const float *__restrict__ x,
                                                                 unsigned long long *__restrict__ part, long long *__restrict__ idx_out,
                                                                 float *__restrict__ dist_out) {
    // candidate pairs (j, j+1) interleaved per channel: one ds_read_b128 (every lane the same address: a broadcast) gives channels
    // c, c+1 of both candidates, and the packed-f32 VALU computes the pair.
    __shared__ __attribute__((aligned(16))) float s_c[kFkTile * DP];
    const int tid = threadIdx.x, b = blockIdx.z, s = blockIdx.y;
    const int i = blockIdx.x * kFkThreads + tid;
    const int iq = i < N ? i : N - 1;
    const float *__restrict__ X = x + (size_t)b * D * N;
    float q[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) q[c] = c < D ? X[(size_t)c * N + iq] : 0.0f;   // padded channels: t = 0 - 0, acc + 0 = acc exactly
    unsigned long long keys[KP];
#pragma unroll
    for (int p = 0; p < KP; ++p) keys[p] = p < KP - k ? 0ull : ~0ull;
    const int j0 = s * chunk, j1 = min(N, j0 + chunk);
    for (int t0 = j0; t0 < j1; t0 += kFkTile) {
        __syncthreads();
        for (int e = tid; e < kFkTile * DP; e += kFkThreads) {
            const int c = e / kFkTile, jj = e % kFkTile, j = t0 + jj;
            s_c[(jj >> 1) * (2 * DP) + 2 * c + (jj & 1)] = (c < D && j < j1) ? X[(size_t)c * N + j] : 0.0f;
        }
        __syncthreads();
        const int np = min(kFkTile, j1 - t0 + 1) >> 1;   // pairs holding at least one real candidate
        for (int pp = 0; pp < np; ++pp) {
            const float *__restrict__ row = s_c + pp * (2 * DP);
            f32x2 acc = {0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < DP; c += 2) {
                const f32x4 v = *(const f32x4 *)(row + 2 * c);
                const f32x2 qa = {q[c], q[c]}, qb = {q[c + 1], q[c + 1]};
                f32x2 t = qa - (f32x2){v.x, v.y};
                acc = acc + t * t;
                if (c + 1 < DP) {
                    t = qb - (f32x2){v.z, v.w};
                    acc = acc + t * t;
                }
            }
            const int j = t0 + 2 * pp;
            const unsigned long long ka = knn_key(acc.x, j);
            const unsigned long long kb = j + 1 < j1 ? knn_key(acc.y, j + 1) : ~0ull;
            if (ka < keys[KP - 1]) topk_insert<KP>(keys, ka);
            if (kb < keys[KP - 1]) topk_insert<KP>(keys, kb);
        }
    }
    if (i >= N) return;
    if (S > 1) {
        unsigned long long *__restrict__ o = part + (((size_t)b * S + s) * N + i) * k;
#pragma unroll
        for (int p = 0; p < KP; ++p)
            if (p >= KP - k) o[p - (KP - k)] = keys[p];
    } else {
        long long *__restrict__ oi = idx_out + ((size_t)b * N + i) * k;
#pragma unroll
        for (int p = 0; p < KP; ++p)
            if (p >= KP - k) {
                oi[p - (KP - k)] = (long long)(unsigned)keys[p];
                if (dist_out) dist_out[((size_t)b * N + i) * k + p - (KP - k)] = __uint_as_float((unsigned)(keys[p] >> 32));
            }
    }
}

// One thread per query: the S sorted partial lists merged by key.  A list stops at its first key at or above the threshold.
template <int KP>
__global__ __launch_bounds__(256) void feature_knn_merge_kernel(int B, int N, int k, int S, const unsigned long long *__restrict__ part,
                                                                long long *__restrict__ idx_out, float *__restrict__ dist_out) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)B * N) return;
    const int b = (int)(g / N), i = (int)(g - (long long)b * N);
    unsigned long long keys[KP];
#pragma unroll
    for (int p = 0; p < KP; ++p) keys[p] = p < KP - k ? 0ull : ~0ull;
    for (int s = 0; s < S; ++s) {
        const unsigned long long *__restrict__ l = part + (((size_t)b * S + s) * N + i) * k;
        for (int r = 0; r < k; ++r) {
            const unsigned long long key = l[r];
            if (!(key < keys[KP - 1])) break;
            topk_insert<KP>(keys, key);
        }
    }
#pragma unroll
    for (int p = 0; p < KP; ++p)
        if (p >= KP - k) {
            idx_out[g * k + p - (KP - k)] = (long long)(unsigned)keys[p];
            if (dist_out) dist_out[g * k + p - (KP - k)] = __uint_as_float((unsigned)(keys[p] >> 32));
        }
}

// Splits of the candidate range: enough workgroups for 4 per CU at batch 1 (256 CUs), at least kFkMinChunk candidates per split.
static int knn_splits(int B, int N) {
    const long long tiles = (long long)B * ((N + kFkThreads - 1) / kFkThreads);
    long long s = (1024 + tiles - 1) / tiles;
    s = s < 1 ? 1 : (s > kFkMaxSplits ? kFkMaxSplits : s);
    const long long by_len = (N + kFkMinChunk - 1) / kFkMinChunk;
    if (s > by_len) s = by_len;
    return (int)(s < 1 ? 1 : s);
}

static int knn_chunk(int N, int S) {
    int c = (N + S - 1) / S;
    return (c + 1) & ~1;   // even: candidate pairs never straddle two splits
}

// ---- tgn_edgeconv2_max --------------------------------------------------------------------------------------------------------
constexpr int kEcThreads = 256, kEcC = 64;

__device__ __forceinline__ float lrelu02(float v) { return v >= 0.0f ? v : v * 0.2f; }   // nn.LeakyReLU(0.2)

__device__ __forceinline__ long long ec_neighbour(const long long *__restrict__ row, int r, int N, bool &bad) {
    long long v = row[r];
    if (v < 0 || v >= N) {
        bad = true;
        v = 0;
    }
    return v;
}

// P, Q: (B, N, 64) point-major; idx (B, N, K); W2 (64 out, 64 in) row-major; out (B, *, N) at channel coff, batch stride ostride.
// Lane l: MFMA row r = l & 31 (neighbour slot; slots >= K repeat neighbour 0, which the max does not see), k half h = l >> 5: step s
// of the 32 takes input channels s (h = 0) and 32 + s (h = 1) -- the sum over the 64 channels in another order, the same terms.
__global__ __launch_bounds__(kEcThreads) void edgeconv2_max_kernel(int B, int N, int K, const float *__restrict__ P,
                                                                   const float *__restrict__ Q, const long long *__restrict__ idx,
                                                                   const float *__restrict__ W2, const float *__restrict__ b2,
                                                                   float *__restrict__ out, long long ostride, int coff,
                                                                   int *__restrict__ err) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const long long nq = (long long)B * N;
    const long long wave0 = ((long long)blockIdx.x * kEcThreads + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * kEcThreads) >> 6;
    float w0[32], w1[32];   // B operands: W2[j][32h + s] for output columns j = r and 32 + r
#pragma unroll
    for (int s = 0; s < 32; s += 4) {
        const f32x4 a = *(const f32x4 *)(W2 + (size_t)r * kEcC + 32 * h + s);
        const f32x4 c = *(const f32x4 *)(W2 + (size_t)(32 + r) * kEcC + 32 * h + s);
        w0[s] = a.x, w0[s + 1] = a.y, w0[s + 2] = a.z, w0[s + 3] = a.w;
        w1[s] = c.x, w1[s + 1] = c.y, w1[s + 2] = c.z, w1[s + 3] = c.w;
    }
    const float bias = b2[32 * h + r];
    bool bad = false;
    for (long long g = wave0; g < nq; g += nwaves) {
        const int b = (int)(g / N), i = (int)(g - (long long)b * N);
        const long long v = ec_neighbour(idx + g * K, r < K ? r : 0, N, bad);
        const float *__restrict__ pr = P + ((size_t)b * N + (size_t)v) * kEcC + 32 * h;
        const float *__restrict__ qr = Q + (size_t)g * kEcC + 32 * h;
        f32x16 acc0 = {}, acc1 = {};
#pragma unroll
        for (int s = 0; s < 32; s += 4) {
            const f32x4 pv = *(const f32x4 *)(pr + s), qv = *(const f32x4 *)(qr + s);
            const float hv[4] = {lrelu02(pv.x + qv.x), lrelu02(pv.y + qv.y), lrelu02(pv.z + qv.z), lrelu02(pv.w + qv.w)};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(hv[u], w0[s + u], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(hv[u], w1[s + u], acc1, 0, 0, 0);
            }
        }
        // lane holds column r of each tile for rows (reg & 3) + 8 (reg >> 2) + 4h: max over its 16, then over the two halves
        float m0 = acc0[0], m1 = acc1[0];
#pragma unroll
        for (int u = 1; u < 16; ++u) {
            m0 = fmaxf(m0, acc0[u]);
            m1 = fmaxf(m1, acc1[u]);
        }
        m0 = fmaxf(m0, __shfl_xor(m0, 32));
        m1 = fmaxf(m1, __shfl_xor(m1, 32));
        // bias and LeakyReLU are monotone, so they commute with the max (exactly: rounding is monotone too)
        const float y = lrelu02((h ? m1 : m0) + bias);
        out[(size_t)b * ostride + (size_t)(coff + 32 * h + r) * N + i] = y;
    }
    if (__any(bad) && lane == 0 && err) atomicOr(err, kIndexErrGather);
}

// ---- tgn_edgeconv1_max --------------------------------------------------------------------------------------------------------
// lane = channel: max_j (P_j + Q_i) = max_j P_j + Q_i exactly (a rounded add is monotone), and so is the LeakyReLU after it.
__global__ __launch_bounds__(kEcThreads) void edgeconv1_max_kernel(int B, int N, int K, const float *__restrict__ P,
                                                                   const float *__restrict__ Q, const long long *__restrict__ idx,
                                                                   float *__restrict__ out, long long ostride, int coff,
                                                                   int *__restrict__ err) {
    const int lane = threadIdx.x & 63;
    const long long nq = (long long)B * N;
    const long long wave0 = ((long long)blockIdx.x * kEcThreads + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * kEcThreads) >> 6;
    bool bad = false;
    for (long long g = wave0; g < nq; g += nwaves) {
        const int b = (int)(g / N), i = (int)(g - (long long)b * N);
        const long long *__restrict__ row = idx + g * K;
        float m = -INFINITY;
        for (int r = 0; r < K; ++r) {
            const long long v = ec_neighbour(row, r, N, bad);
            m = fmaxf(m, P[((size_t)b * N + (size_t)v) * kEcC + lane]);
        }
        out[(size_t)b * ostride + (size_t)(coff + lane) * N + i] = lrelu02(m + Q[(size_t)g * kEcC + lane]);
    }
    if (__any(bad) && lane == 0 && err) atomicOr(err, kIndexErrGather);
}

static int ec_grid(long long nq) {
    const long long want = (nq + 3) / 4;   // one query per wave at most
    return (int)(want < 2048 ? (want < 1 ? 1 : want) : 2048);
}

}  // namespace tgn

using namespace tgn;

TGN_API size_t tgn_feature_knn_workspace_bytes(int B, int N, int k) {
    if (B < 1 || N < 1 || k < 1) return 0;
    const int S = knn_splits(B, N);
    return S > 1 ? (size_t)B * S * N * k * sizeof(unsigned long long) : 0;
}

template <int DP>
static void launch_knn(int KP, dim3 grid, hipStream_t st, int N, int D, int k, int S, int chunk, const float *x, unsigned long long *part,
                       long long *idx, float *dist2) {
    if (KP == 8)
        hipLaunchKernelGGL((feature_knn_kernel<DP, 8>), grid, dim3(kFkThreads), 0, st, N, D, k, S, chunk, x, part, idx, dist2);
    else if (KP == 16)
        hipLaunchKernelGGL((feature_knn_kernel<DP, 16>), grid, dim3(kFkThreads), 0, st, N, D, k, S, chunk, x, part, idx, dist2);
    else
        hipLaunchKernelGGL((feature_knn_kernel<DP, 32>), grid, dim3(kFkThreads), 0, st, N, D, k, S, chunk, x, part, idx, dist2);
}

TGN_API int tgn_feature_knn(int B, int N, int D, int k, const float *x, long long *idx, float *dist2, void *workspace, size_t ws_bytes,
                            tgn_stream_t stream) {
    if (B < 1 || N < 1 || D < 1 || D > kFkMaxD || k < 1 || k > kFkMaxK || N < k || !x || !idx) {
        set_error("tgn_feature_knn: bad arguments (B=%d N=%d D=%d k=%d; need B >= 1, 1 <= D <= %d, 1 <= k <= min(N, %d), x and idx non-NULL)",
                  B, N, D, k, kFkMaxD, kFkMaxK);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    const size_t need = tgn_feature_knn_workspace_bytes(B, N, k);
    if (ws_bytes < need || (need && !workspace)) {
        set_error("tgn_feature_knn: workspace of %zu bytes given, %zu needed (tgn_feature_knn_workspace_bytes)", ws_bytes, need);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    const int S = knn_splits(B, N), chunk = knn_chunk(N, S);
    const int KP = k <= 8 ? 8 : (k <= 16 ? 16 : 32);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *part = (unsigned long long *)workspace;
    const dim3 grid((N + kFkThreads - 1) / kFkThreads, S, B);
    if (D <= 4) launch_knn<4>(KP, grid, st, N, D, k, S, chunk, x, part, idx, dist2);
    else if (D <= 8) launch_knn<8>(KP, grid, st, N, D, k, S, chunk, x, part, idx, dist2);
    else if (D <= 16) launch_knn<16>(KP, grid, st, N, D, k, S, chunk, x, part, idx, dist2);
    else if (D <= 32) launch_knn<32>(KP, grid, st, N, D, k, S, chunk, x, part, idx, dist2);
    else launch_knn<64>(KP, grid, st, N, D, k, S, chunk, x, part, idx, dist2);
    int rc = check_launch("tgn_feature_knn");
    if (rc != TGN_OK || S == 1) return rc;
    const dim3 mg((unsigned)(((long long)B * N + 255) / 256));
    if (KP == 8) hipLaunchKernelGGL(feature_knn_merge_kernel<8>, mg, dim3(256), 0, st, B, N, k, S, part, idx, dist2);
    else if (KP == 16) hipLaunchKernelGGL(feature_knn_merge_kernel<16>, mg, dim3(256), 0, st, B, N, k, S, part, idx, dist2);
    else hipLaunchKernelGGL(feature_knn_merge_kernel<32>, mg, dim3(256), 0, st, B, N, k, S, part, idx, dist2);
    return check_launch("tgn_feature_knn (merge)");
}

static int ec_check(const char *what, int B, int N, int K, const void *P, const void *Q, const void *idx, const void *out, long long ostride,
                    int coff) {
    if (B < 1 || N < 1 || K < 1 || K > 32 || !P || !Q || !idx || !out || coff < 0 || ostride < (long long)(coff + kEcC) * N) {
        set_error("%s: bad arguments (B=%d N=%d K=%d coff=%d ostride=%lld; need 1 <= K <= 32, ostride >= (coff + 64) * N, non-NULL pointers)",
                  what, B, N, K, coff, ostride);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    return TGN_OK;
}

TGN_API int tgn_edgeconv2_max(int B, int N, int K, const float *P, const float *Q, const long long *idx, const float *W2, const float *b2,
                              float *out, long long ostride, int coff, tgn_stream_t stream) {
    int rc = ec_check("tgn_edgeconv2_max", B, N, K, P, Q, idx, out, ostride, coff);
    if (rc != TGN_OK) return rc;
    if (!W2 || !b2) {
        set_error("tgn_edgeconv2_max: W2 and b2 must be non-NULL");
        return TGN_ERR_INVALID_ARGUMENT;
    }
    int *err = index_error_word((hipStream_t)stream);
    if (!err) {
        set_error("tgn_edgeconv2_max: cannot allocate the error word");
        return TGN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(edgeconv2_max_kernel, dim3(ec_grid((long long)B * N)), dim3(kEcThreads), 0, (hipStream_t)stream, B, N, K, P, Q, idx,
                       W2, b2, out, ostride, coff, err);
    return check_launch("tgn_edgeconv2_max");
}

TGN_API int tgn_edgeconv1_max(int B, int N, int K, const float *P, const float *Q, const long long *idx, float *out, long long ostride, int coff,
                              tgn_stream_t stream) {
    int rc = ec_check("tgn_edgeconv1_max", B, N, K, P, Q, idx, out, ostride, coff);
    if (rc != TGN_OK) return rc;
    int *err = index_error_word((hipStream_t)stream);
    if (!err) {
        set_error("tgn_edgeconv1_max: cannot allocate the error word");
        return TGN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(edgeconv1_max_kernel, dim3(ec_grid((long long)B * N)), dim3(kEcThreads), 0, (hipStream_t)stream, B, N, K, P, Q, idx,
                       out, ostride, coff, err);
    return check_launch("tgn_edgeconv1_max");
}
