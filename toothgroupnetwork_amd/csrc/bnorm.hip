// bnorm.hip -- training-mode BatchNorm1d over the ROWS of a (rows, C) matrix, optionally fused with the ReLU behind it: the
// normalisations of the Point-Transformer training path (blocks.py:37,40 transpose to (n, c, nsample) for nn.BatchNorm1d; the
// mirrors normalise the flattened (n * nsample, c) rows, point_transformer._mlp_rows), 124 of them per step of the tgnet_fps
// network, most on small deep-stage tensors where torch's five-odd launches per normalisation and direction (statistics,
// transform, counter, ReLU / zero-fill, reduce, element-wise) cost more than their bytes.
//
//   forward : (1) per-column sum and sum of squares in DOUBLE (one pass; LDS double atomics per block, one global double atomic per
//                 column and block); the last block to finish turns them into mean / 1/sqrt(var + eps), updates the running
//                 statistics exactly like nn.BatchNorm1d (momentum, unbiased variance) and leaves the workspace zeroed;
//             (2) y = [relu]((x - mean) * invstd * gamma + beta), 16 B per lane when C % 4 == 0.
//   backward: (3) per-column sum(g) and sum(g * xhat) with g = dy * (y > 0) under ReLU -- same reduction, the last block writes
//                 dbeta / dgamma; (4) dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)).
// A thread keeps ONE column: the grid is sized so that the total thread count is a multiple of C and element e of thread t sits in
// column t % C on every trip.
// The two reductions (1) and (3) have a second, ORDERED form (tgn_bn_rows_*_ordered): the same grid and the same per-thread sums, but
// no atomic at all -- a block's threads are combined through LDS in thread order, the blocks' partials by a finishing launch in a
// fixed order -- so the bits are a function of the operands and (rows, C) alone.  (2) and (4) are order-free and shared.
#include "tgn_common.h"

namespace tgn {

constexpr int kBnThreads = 256;
constexpr int kBnMaxC = 1024;

__host__ __device__ inline size_t bn_ws_bytes(int C) { return (size_t)2 * C * sizeof(double) + 16; }

// What one thread of a reduction adds up: elements t0, t0 + T, t0 + 2 T, ... of its column, each sum in ascending element order from
// +0.0 (four loads in flight, the adds sequential).  forward: s1 = sum x, s2 = sum x * x (the product in double, exact);
// backward: s1 = sum g, s2 = sum g * xhat with g = dy * (y > 0) under ReLU and xhat = (x - mean) * invstd, the products in float.
template <bool BWD>
__device__ __forceinline__ void bn_thread_sums(long long total, long long T, long long t0, int col, const float *__restrict__ x,
                                               const float *__restrict__ y, const float *__restrict__ dy,
                                               const float *__restrict__ mean_in, const float *__restrict__ invstd_in, int relu,
                                               double &s1, double &s2) {
    s1 = s2 = 0.0;
    float mu = 0.0f, is = 0.0f;
    if (BWD) {
        mu = mean_in[col];
        is = invstd_in[col];
    }
    long long e = t0;
    for (; e + 3 * T < total; e += 4 * T) {                        // four loads in flight
        float v[4], g[4], w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = x[e + u * T];
            if (BWD) {
                g[u] = dy[e + u * T];
                w[u] = relu ? y[e + u * T] : 1.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (BWD) {
                const float gg = w[u] > 0.0f ? g[u] : 0.0f;
                s1 += (double)gg;
                s2 += (double)(gg * ((v[u] - mu) * is));
            } else {
                s1 += (double)v[u];
                s2 += (double)v[u] * (double)v[u];
            }
        }
    }
    for (; e < total; e += T) {
        const float v = x[e];
        if (BWD) {
            const float gg = (!relu || y[e] > 0.0f) ? dy[e] : 0.0f;
            s1 += (double)gg;
            s2 += (double)(gg * ((v - mu) * is));
        } else {
            s1 += (double)v;
            s2 += (double)v * (double)v;
        }
    }
}

// What a column's two sums become, the same double expressions in both forms of the reduction.  forward: mean, biased variance
// clamped at 0, 1 / sqrt(var + eps), the running statistics with the unbiased estimate; backward: dbeta / dgamma cast to float.
template <bool BWD>
__device__ __forceinline__ void bn_finalise(int c, double a1, double a2, double n, float eps, float momentum,
                                            float *__restrict__ running_mean, float *__restrict__ running_var,
                                            float *__restrict__ save_mean, float *__restrict__ save_invstd, float *__restrict__ dgamma,
                                            float *__restrict__ dbeta) {
    if (BWD) {
        dbeta[c] = (float)a1;
        dgamma[c] = (float)a2;
    } else {
        const double mean = a1 / n;
        double var = a2 / n - mean * mean;                     // biased, what the batch is normalised with
        if (var < 0.0) var = 0.0;
        save_mean[c] = (float)mean;
        save_invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
        if (running_mean) {
            const double unbiased = var * (n / (n - 1.0));     // nn.BatchNorm1d keeps the unbiased estimate
            running_mean[c] = (float)((1.0 - (double)momentum) * (double)running_mean[c] + (double)momentum * mean);
            running_var[c] = (float)((1.0 - (double)momentum) * (double)running_var[c] + (double)momentum * unbiased);
        }
    }
}

template <bool BWD>
__global__ __launch_bounds__(kBnThreads) void bn_rows_reduce_kernel(
    long long total, long long rows, int C, const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ dy,
    const float *__restrict__ mean_in, const float *__restrict__ invstd_in, int relu, double *__restrict__ acc,
    unsigned *__restrict__ counter,
    // forward finalisation
    float eps, float momentum, float *__restrict__ running_mean, float *__restrict__ running_var,
    long long *__restrict__ num_batches_tracked, float *__restrict__ save_mean, float *__restrict__ save_invstd,
    // backward finalisation
    float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double lacc[2][kBnMaxC];
    __shared__ unsigned ticket_s;
    const int tid = threadIdx.x;
    for (int c = tid; c < C; c += kBnThreads) lacc[0][c] = lacc[1][c] = 0.0;
    __syncthreads();
    const long long T = (long long)gridDim.x * kBnThreads;        // a multiple of C
    const long long t0 = (long long)blockIdx.x * kBnThreads + tid;
    const int col = (int)(t0 % C);
    double s1, s2;
    bn_thread_sums<BWD>(total, T, t0, col, x, y, dy, mean_in, invstd_in, relu, s1, s2);
    atomicAdd(&lacc[0][col], s1);
    atomicAdd(&lacc[1][col], s2);
    __syncthreads();
    for (int c = tid; c < C; c += kBnThreads) {
        atomicAdd(&acc[c], lacc[0][c]);
        atomicAdd(&acc[C + c], lacc[1][c]);
    }
    __threadfence();
    __syncthreads();
    if (tid == 0) ticket_s = atomicAdd(counter, 1u);
    __syncthreads();
    if (ticket_s != gridDim.x - 1) return;
    // last block: every partial sum is in
    __threadfence();
    const double n = (double)rows;
    for (int c = tid; c < C; c += kBnThreads) {
        const double a1 = __hip_atomic_load(&acc[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double a2 = __hip_atomic_load(&acc[C + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        acc[c] = 0.0;
        acc[C + c] = 0.0;
        bn_finalise<BWD>(c, a1, a2, n, eps, momentum, running_mean, running_var, save_mean, save_invstd, dgamma, dbeta);
    }
    if (tid == 0) {
        *counter = 0u;
        if (!BWD && num_batches_tracked) *num_batches_tracked += 1;
    }
}

// element-wise halves.  VEC: C % 4 == 0, 16 B per lane.
template <bool BWD, bool VEC>
__global__ __launch_bounds__(kBnThreads) void bn_rows_apply_kernel(long long total, long long rows, int C,
                                                                   const float *__restrict__ x, const float *__restrict__ y_in,
                                                                   const float *__restrict__ dy, const float *__restrict__ gamma,
                                                                   const float *__restrict__ beta, const float *__restrict__ mean,
                                                                   const float *__restrict__ invstd, const float *__restrict__ dgamma,
                                                                   const float *__restrict__ dbeta, int relu, float *__restrict__ out) {
    // forward: out = x * p0 + p1;  backward: out = p0 * (g - p1 - (x - p3) * p2)
    __shared__ float p0[kBnMaxC], p1[kBnMaxC], p2[kBnMaxC], p3[kBnMaxC];
    const float inv_n = 1.0f / (float)rows;
    for (int c = threadIdx.x; c < C; c += kBnThreads) {
        const float is = invstd[c], sc = is * gamma[c];
        if (BWD) {
            p0[c] = sc;
            p1[c] = dbeta[c] * inv_n;
            p2[c] = is * (dgamma[c] * inv_n);                      // xhat * mean(g xhat) = (x - mean) * p2
            p3[c] = mean[c];
        } else {
            p0[c] = sc;
            p1[c] = beta[c] - mean[c] * sc;
        }
    }
    __syncthreads();
    constexpr int W = VEC ? 4 : 1;
    const long long units = total / W;
    const long long T = (long long)gridDim.x * kBnThreads;
    for (long long u = (long long)blockIdx.x * kBnThreads + threadIdx.x; u < units; u += T) {
        const long long e = u * W;
        int c = (int)(e % C);
        float xv[W], gv[W], yv[W], ov[W];
        if (VEC) {
            *(float4 *)xv = *(const float4 *)(x + e);
            if (BWD) {
                *(float4 *)gv = *(const float4 *)(dy + e);
                if (relu) *(float4 *)yv = *(const float4 *)(y_in + e);
            }
        } else {
            xv[0] = x[e];
            if (BWD) {
                gv[0] = dy[e];
                if (relu) yv[0] = y_in[e];
            }
        }
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const int cc = c + i;                                  // (VEC: C % 4 == 0, so the four stay inside one row)
            if (BWD) {
                const float g = (!relu || yv[i] > 0.0f) ? gv[i] : 0.0f;
                ov[i] = p0[cc] * (g - p1[cc] - (xv[i] - p3[cc]) * p2[cc]);
            } else {
                const float v = xv[i] * p0[cc] + p1[cc];
                ov[i] = relu ? fmaxf(v, 0.0f) : v;
            }
        }
        if (VEC)
            *(float4 *)(out + e) = *(float4 *)ov;
        else
            out[e] = ov[0];
    }
}

// ---- the ordered form of the two reductions: no float or double atomic, one summation order per (rows, C) -------------------------
// (include/tgn_pointops.h states the order with tgn_bn_rows_forward_ordered; tests/bn_ordered_ref.py restates it in numpy)
constexpr int kBnChains = 64;

// step 1 and 2: a thread's sums, then per block the threads of a column in ascending thread order; part[block][2][C], every entry
// written (+0.0 for a column none of the block's threads keeps: C > 256)
template <bool BWD>
__global__ __launch_bounds__(kBnThreads) void bn_rows_partials_kernel(long long total, int C, const float *__restrict__ x,
                                                                      const float *__restrict__ y, const float *__restrict__ dy,
                                                                      const float *__restrict__ mean_in,
                                                                      const float *__restrict__ invstd_in, int relu,
                                                                      double *__restrict__ part) {
    __shared__ double ls[2][kBnThreads];
    const int tid = threadIdx.x;
    const long long T = (long long)gridDim.x * kBnThreads;        // a multiple of C
    const long long b0 = (long long)blockIdx.x * kBnThreads;
    const int col = (int)((b0 + tid) % C);
    double s1, s2;
    bn_thread_sums<BWD>(total, T, b0 + tid, col, x, y, dy, mean_in, invstd_in, relu, s1, s2);
    ls[0][tid] = s1;
    ls[1][tid] = s2;
    __syncthreads();
    double *mine = part + (size_t)blockIdx.x * 2 * C;
    if (tid < C) {                                                 // the first thread of its column here reads the others: tid + C, + 2 C, ...
        for (int u = tid + C; u < kBnThreads; u += C) {
            s1 += ls[0][u];
            s2 += ls[1][u];
        }
        mine[col] = s1;
        mine[C + col] = s2;
    }
    for (int j = kBnThreads + tid; j < C; j += kBnThreads) {       // threads 0 .. 255 keep columns (b0 + 0 .. 255) % C; these are the rest
        const int c = (int)((b0 + j) % C);
        mine[c] = 0.0;
        mine[C + c] = 0.0;
    }
}

// step 3 and 4: one wave per column.  Lane j adds the partials of blocks j, j + 64, ... in ascending order from +0.0; lane 0 adds the
// chains in ascending lane order from +0.0 and finalises the column.
template <bool BWD>
__global__ __launch_bounds__(kBnChains) void bn_rows_finish_kernel(int blocks, long long rows, int C, const double *__restrict__ part,
                                                                   float eps, float momentum, float *__restrict__ running_mean,
                                                                   float *__restrict__ running_var,
                                                                   long long *__restrict__ num_batches_tracked,
                                                                   float *__restrict__ save_mean, float *__restrict__ save_invstd,
                                                                   float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double chain[2][kBnChains];
    const int c = blockIdx.x, lane = threadIdx.x;
    double a1 = 0.0, a2 = 0.0;
#pragma unroll 4
    for (int b = lane; b < blocks; b += kBnChains) {
        a1 += part[(size_t)b * 2 * C + c];
        a2 += part[(size_t)b * 2 * C + C + c];
    }
    chain[0][lane] = a1;
    chain[1][lane] = a2;
    __syncthreads();
    if (lane != 0) return;
    a1 = a2 = 0.0;
    const int chains = blocks < kBnChains ? blocks : kBnChains;    // (the chains behind them are +0.0)
    for (int j = 0; j < chains; ++j) {
        a1 += chain[0][j];
        a2 += chain[1][j];
    }
    bn_finalise<BWD>(c, a1, a2, (double)rows, eps, momentum, running_mean, running_var, save_mean, save_invstd, dgamma, dbeta);
    if (!BWD && c == 0 && num_batches_tracked) *num_batches_tracked += 1;
}

static int bn_gcd(int a, int b) { return b ? bn_gcd(b, a % b) : a; }

// blocks of the reduction: enough to fill the chip on big inputs, a multiple of C / gcd(256, C) so that a thread keeps its column
static unsigned bn_reduce_blocks(long long total, int C) {
    const int m = C / bn_gcd(kBnThreads, C);
    long long b = (total + (long long)kBnThreads * 32 - 1) / ((long long)kBnThreads * 32);
    if (b > 1024) b = 1024;
    if (b < 1) b = 1;
    b = (b + m - 1) / m * m;
    return (unsigned)b;
}

static bool bn_vec_ok(int C, const void *a, const void *b, const void *c, const void *d) {
    auto al = [](const void *p) { return p == nullptr || ((unsigned long long)p & 15ull) == 0ull; };
    return C % 4 == 0 && al(a) && al(b) && al(c) && al(d);
}

static size_t bn_ordered_ws_bytes(long long rows, int C) { return (size_t)bn_reduce_blocks(rows * C, C) * 2 * C * sizeof(double); }

// both reductions in either form, then the element-wise half.  ordered: workspace = part[blocks][2][C]; else the zeroed accumulators + ticket
template <bool BWD>
static int bn_rows_launch(const char *name, bool ordered, long long rows, int C, const float *x, const float *y, const float *dy,
                          const float *gamma, const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                          long long *num_batches_tracked, float *save_mean, float *save_invstd, int relu, float *out, float *dgamma,
                          float *dbeta, void *workspace, size_t workspace_bytes, hipStream_t st) {
    if (rows < 2 || C <= 0 || C > kBnMaxC) {
        set_error("%s: rows = %lld, C = %d (needs rows >= 2 and 1 <= C <= %d)", name, rows, C, kBnMaxC);
        return TGN_ERR_UNSUPPORTED;
    }
    const bool null = BWD ? (!x || !dy || !gamma || !save_mean || !save_invstd || !out || !dgamma || !dbeta || !workspace || (relu && !y))
                          : (!x || !gamma || !beta || !out || !save_mean || !save_invstd || !workspace || (!running_mean != !running_var));
    if (null) {
        set_error("%s: null pointer", name);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (ordered && workspace_bytes < bn_ordered_ws_bytes(rows, C)) {
        set_error("%s: workspace of %zu bytes, tgn_bn_rows_ordered_workspace_bytes(%lld, %d) = %zu", name, workspace_bytes, rows, C,
                  bn_ordered_ws_bytes(rows, C));
        return TGN_ERR_INVALID_ARGUMENT;
    }
    const long long total = rows * C;
    const unsigned rblocks = bn_reduce_blocks(total, C);
    if (ordered) {
        hipLaunchKernelGGL((bn_rows_partials_kernel<BWD>), dim3(rblocks), dim3(kBnThreads), 0, st, total, C, x, y, dy,
                           (const float *)save_mean, (const float *)save_invstd, relu, (double *)workspace);
        if (int rc = check_launch("bn_rows_partials_kernel")) return rc;
        hipLaunchKernelGGL((bn_rows_finish_kernel<BWD>), dim3(C), dim3(kBnChains), 0, st, (int)rblocks, rows, C,
                           (const double *)workspace, eps, momentum, running_mean, running_var, num_batches_tracked, save_mean,
                           save_invstd, dgamma, dbeta);
        if (int rc = check_launch("bn_rows_finish_kernel")) return rc;
    } else {
        double *acc = (double *)workspace;
        unsigned *counter = (unsigned *)((char *)workspace + (size_t)2 * C * sizeof(double));
        hipLaunchKernelGGL((bn_rows_reduce_kernel<BWD>), dim3(rblocks), dim3(kBnThreads), 0, st, total, rows, C, x, y, dy,
                           (const float *)save_mean, (const float *)save_invstd, relu, acc, counter, eps, momentum, running_mean,
                           running_var, num_batches_tracked, save_mean, save_invstd, dgamma, dbeta);
        if (int rc = check_launch("bn_rows_reduce_kernel")) return rc;
    }
    const bool vec = BWD ? bn_vec_ok(C, x, dy, relu ? y : nullptr, out) : bn_vec_ok(C, x, out, nullptr, nullptr);
    long long blocks = (total / (vec ? 4 : 1) + kBnThreads * 4 - 1) / (kBnThreads * 4);
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    if (vec)
        hipLaunchKernelGGL((bn_rows_apply_kernel<BWD, true>), dim3((unsigned)blocks), dim3(kBnThreads), 0, st, total, rows, C, x, y, dy,
                           gamma, beta, (const float *)save_mean, (const float *)save_invstd, (const float *)dgamma,
                           (const float *)dbeta, relu, out);
    else
        hipLaunchKernelGGL((bn_rows_apply_kernel<BWD, false>), dim3((unsigned)blocks), dim3(kBnThreads), 0, st, total, rows, C, x, y, dy,
                           gamma, beta, (const float *)save_mean, (const float *)save_invstd, (const float *)dgamma,
                           (const float *)dbeta, relu, out);
    return check_launch("bn_rows_apply_kernel");
}

}  // namespace tgn

using namespace tgn;

TGN_API size_t tgn_bn_rows_workspace_bytes(int C) { return C > 0 && C <= kBnMaxC ? bn_ws_bytes(C) : 0; }

TGN_API size_t tgn_bn_rows_ordered_workspace_bytes(long long rows, int C) {
    return rows >= 2 && C > 0 && C <= kBnMaxC ? bn_ordered_ws_bytes(rows, C) : 0;
}

TGN_API int tgn_bn_rows_forward(long long rows, int C, const float *x, const float *gamma, const float *beta, float eps,
                                float momentum, float *running_mean, float *running_var, long long *num_batches_tracked,
                                int relu, float *y, float *save_mean, float *save_invstd, void *workspace, tgn_stream_t stream) {
    return bn_rows_launch<false>("tgn_bn_rows_forward", false, rows, C, x, nullptr, nullptr, gamma, beta, eps, momentum, running_mean,
                                 running_var, num_batches_tracked, save_mean, save_invstd, relu, y, nullptr, nullptr, workspace, 0,
                                 (hipStream_t)stream);
}

TGN_API int tgn_bn_rows_forward_ordered(long long rows, int C, const float *x, const float *gamma, const float *beta, float eps,
                                        float momentum, float *running_mean, float *running_var, long long *num_batches_tracked,
                                        int relu, float *y, float *save_mean, float *save_invstd, void *workspace,
                                        size_t workspace_bytes, tgn_stream_t stream) {
    return bn_rows_launch<false>("tgn_bn_rows_forward_ordered", true, rows, C, x, nullptr, nullptr, gamma, beta, eps, momentum,
                                 running_mean, running_var, num_batches_tracked, save_mean, save_invstd, relu, y, nullptr, nullptr,
                                 workspace, workspace_bytes, (hipStream_t)stream);
}

TGN_API int tgn_bn_rows_backward(long long rows, int C, const float *x, const float *y, const float *dy, const float *gamma,
                                 const float *save_mean, const float *save_invstd, int relu, float *dx, float *dgamma, float *dbeta,
                                 void *workspace, tgn_stream_t stream) {
    return bn_rows_launch<true>("tgn_bn_rows_backward", false, rows, C, x, y, dy, gamma, nullptr, 0.0f, 0.0f, nullptr, nullptr, nullptr,
                                (float *)save_mean, (float *)save_invstd, relu, dx, dgamma, dbeta, workspace, 0, (hipStream_t)stream);
}

TGN_API int tgn_bn_rows_backward_ordered(long long rows, int C, const float *x, const float *y, const float *dy, const float *gamma,
                                         const float *save_mean, const float *save_invstd, int relu, float *dx, float *dgamma,
                                         float *dbeta, void *workspace, size_t workspace_bytes, tgn_stream_t stream) {
    return bn_rows_launch<true>("tgn_bn_rows_backward_ordered", true, rows, C, x, y, dy, gamma, nullptr, 0.0f, 0.0f, nullptr, nullptr,
                                nullptr, (float *)save_mean, (float *)save_invstd, relu, dx, dgamma, dbeta, workspace, workspace_bytes,
                                (hipStream_t)stream);
}
