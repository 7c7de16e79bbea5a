// loss.hip -- the geometric training losses of tgnet_fps and tsegnet as fused kernels, forward and backward:
//   tgn_offset_loss_*    batch_center_offset_loss + batch_chamfer_distance_loss (models/tgn_loss.py:6-61, 263-302)
//   tgn_centroid_loss_*  centroid_loss (models/tsg_loss.py:4-61), with an optional mask of the centroids that exist
// The reference loops over B x 16 teeth with boolean masks (one host round trip per tooth) and sorts a (B, M, C) distance matrix
// to read its first two columns.  Here a point is one thread, a scan's at most 16 centroids sit in LDS, and every sum is ordered:
// float64 wave reduction -> LDS -> per-block partials in the caller's workspace -> a finishing kernel that adds them in block order
// and rounds to float32 once.  No float atomics, no allocation, no copy, no synchronisation: the same inputs give the same bits,
// and forward + backward can be captured in a graph.
// Arithmetic: squared distances in the direct form ((dx*dx) + (dy*dy)) + (dz*dz) in float32 (the reference's expanded form cancels);
// every other per-point operation in float32 with each operation rounded (-ffp-contract=off).
#include "tgn_common.h"

namespace tgn {

constexpr int kLossThreads = 256, kLossWaves = kLossThreads / kWave, kLossTeeth = 16;
constexpr int kLossMaxBlocks = 128;                  // point blocks per scan of the forward pass (grid-stride beyond)
constexpr int kLossPartials = 3 * kLossTeeth + 2;    // per block: (E, Q, kept) per tooth, then R and the foreground count
constexpr int kLossScales = 2 * kLossTeeth + 1;      // per scan: (offset, direction) scale per tooth, then the chamfer scale
constexpr float kDirMinNorm = 0.0002f;               // tgn_loss.py:50
constexpr float kCentMask = 0.2f;                    // tsg_loss.py:26,33,49

__device__ __forceinline__ double wave_sum_f64(double v) {   // butterfly: every lane ends with the same bits
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}

// The smallest and second smallest squared distance from m to the centroids flagged in `use`, with their slots (lowest slot on a tie).
struct Nearest2 {
    float d1, d2;
    int c1, c2;
};
__device__ __forceinline__ Nearest2 nearest2(float mx, float my, float mz, const float (*cent)[3], const int *use, int nc) {
    Nearest2 r = {INFINITY, INFINITY, -1, -1};
    for (int s = 0; s < nc; ++s) {
        if (!use[s]) continue;
        const float d = dist_direct_nofma(mx - cent[s][0], my - cent[s][1], mz - cent[s][2]);
        if (d < r.d1) {
            r.d2 = r.d1, r.c2 = r.c1;
            r.d1 = d, r.c1 = s;
        } else if (d < r.d2) {
            r.d2 = d, r.c2 = s;
        }
    }
    r.c1 = r.c1 < 0 ? 0 : r.c1, r.c2 = r.c2 < 0 ? 0 : r.c2;   // nothing flagged, or NaN coordinates: a slot that can be read
    return r;
}

// ---- tgnet_fps: offset, direction and chamfer terms ------------------------------------------------------------------------
struct DirTerm {          // the direction term of one point: dot = d . o_hat, and the unit vectors behind it
    float dot, dx, dy, dz, ox, oy, oz, onorm;
};
__device__ __forceinline__ DirTerm dir_term(float px, float py, float pz, float ox, float oy, float oz, const float *c, float onorm) {
    DirTerm r;
    const float tx = c[0] - px, ty = c[1] - py, tz = c[2] - pz;
    const float tn = sqrtf(sumsq3(tx, ty, tz));
    r.dx = tx / tn, r.dy = ty / tn, r.dz = tz / tn;
    r.ox = ox / onorm, r.oy = oy / onorm, r.oz = oz / onorm;
    r.onorm = onorm;
    r.dot = ((r.dx * r.ox) + (r.dy * r.oy)) + (r.dz * r.oz);
    return r;
}

// grid (blocks per scan, B).  partials (B, gridDim.x, kLossPartials) float64.
__global__ void __launch_bounds__(kLossThreads) offset_loss_points_kernel(int n, const float *__restrict__ offset,
                                                                          const float *__restrict__ xyz,
                                                                          const long long *__restrict__ labels,
                                                                          const int *__restrict__ counts, const float *__restrict__ cent,
                                                                          double *__restrict__ partials, int *__restrict__ err) {
    __shared__ float s_c[kLossTeeth][3];
    __shared__ int s_valid[kLossTeeth];
    __shared__ double s_w[kLossWaves][kLossPartials];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    if (tid < kLossTeeth) {
        s_valid[tid] = counts[b * kLossTeeth + tid] >= 5;
        for (int a = 0; a < 3; ++a) s_c[tid][a] = cent[(b * kLossTeeth + tid) * 3 + a];
    }
    __syncthreads();
    const float *O = offset + (long long)b * 3 * n, *X = xyz + (long long)b * 3 * n;
    const long long *L = labels + (long long)b * n;
    double acc_e = 0.0, acc_q = 0.0, acc_k = 0.0;     // lane t < 16: tooth t's sums over this wave's points
    double acc_r = 0.0, acc_f = 0.0;                   // every lane: its own points
    bool bad = false;
    for (int base = blockIdx.x * kLossThreads; base < n; base += gridDim.x * kLossThreads) {   // uniform over the block
        const int i = base + tid;
        int lab = -1;
        float e = 0.0f, q = 0.0f;
        bool kept = false;
        if (i < n) {
            const long long v = L[i];
            if (v < -1 || v >= kLossTeeth) bad = true;
            else lab = (int)v;
        }
        if (lab >= 0) {
            const float px = X[i], py = X[n + i], pz = X[2 * n + i];
            const float ox = O[i], oy = O[n + i], oz = O[2 * n + i];
            const float mx = px + ox, my = py + oy, mz = pz + oz;
            if (s_valid[lab]) {
                e = dist_direct_nofma(mx - s_c[lab][0], my - s_c[lab][1], mz - s_c[lab][2]);
                const float onorm = sqrtf(sumsq3(ox, oy, oz));
                if (onorm > kDirMinNorm) {
                    const float dm1 = dir_term(px, py, pz, ox, oy, oz, s_c[lab], onorm).dot - 1.0f;
                    q = dm1 * dm1;
                    kept = true;
                }
            } else {
                lab = -2 - lab;                        // foreground, but of a tooth that is skipped
            }
            const Nearest2 nn = nearest2(mx, my, mz, s_c, s_valid, kLossTeeth);
            acc_r += (double)(nn.d1 / nn.d2);          // fewer than two valid teeth: the finishing kernel gives NaN
            acc_f += 1.0;
        }
        for (int t = 0; t < kLossTeeth; ++t) {
            const bool mine = lab == t;
            if (!__ballot(mine)) continue;             // wave-uniform
            const double ve = wave_sum_f64(mine ? (double)e : 0.0), vq = wave_sum_f64(mine ? (double)q : 0.0);
            const int vk = __popcll(__ballot(mine && kept));
            if (lane == t) acc_e += ve, acc_q += vq, acc_k += (double)vk;
        }
    }
    acc_r = wave_sum_f64(acc_r);
    acc_f = wave_sum_f64(acc_f);
    if (lane < kLossTeeth) {
        s_w[wave][3 * lane] = acc_e;
        s_w[wave][3 * lane + 1] = acc_q;
        s_w[wave][3 * lane + 2] = acc_k;
    }
    if (lane == 0) {
        s_w[wave][3 * kLossTeeth] = acc_r;
        s_w[wave][3 * kLossTeeth + 1] = acc_f;
    }
    __syncthreads();
    if (tid < kLossPartials) {
        double v = 0.0;
        for (int w = 0; w < kLossWaves; ++w) v += s_w[w][tid];
        partials[((long long)b * gridDim.x + blockIdx.x) * kLossPartials + tid] = v;
    }
    if (__syncthreads_or(bad) && tid == 0 && err) atomicOr(err, kIndexErrCrop);
}

// One workgroup.  Adds the partials in block order, then the teeth in (scan, tooth) order; writes losses (3) and scales
// (B, kLossScales).  sums (B, kLossPartials) float64 is scratch between its two passes.
__global__ void __launch_bounds__(kWave) offset_loss_finish_kernel(int nb, int nblocks, const int *__restrict__ counts,
                                                                   const double *__restrict__ partials, double *__restrict__ sums,
                                                                   float *__restrict__ losses, float *__restrict__ scales) {
    __shared__ double s_tot[2];
    const int tid = threadIdx.x;
    for (int b = 0; b < nb; ++b) {
        if (tid < kLossPartials) {
            double v = 0.0;
            for (int g = 0; g < nblocks; ++g) v += partials[((long long)b * nblocks + g) * kLossPartials + tid];
            sums[b * kLossPartials + tid] = v;
        }
    }
    __syncthreads();                                   // (one workgroup: its own global writes are visible behind the barrier)
    if (tid == 0) {
        double off = 0.0, dir = 0.0, chamf = 0.0, n_cen = 0.0, n_dir = 0.0;
        for (int b = 0; b < nb; ++b) {
            const double *S = sums + b * kLossPartials;
            int valid = 0;
            for (int t = 0; t < kLossTeeth; ++t) {
                const int n_t = counts[b * kLossTeeth + t];
                if (n_t < 5) continue;
                ++valid;
                n_cen += 1.0;
                off += S[3 * t] / (double)n_t;
                if (S[3 * t + 2] > 0.0) {
                    n_dir += 1.0;
                    dir += S[3 * t + 1] / S[3 * t + 2];
                }
            }
            chamf += valid >= 2 ? S[3 * kLossTeeth] / S[3 * kLossTeeth + 1] : (double)NAN;   // 0 / 0 without foreground
        }
        losses[0] = (float)(off / n_cen);              // 0 / 0 = NaN without a valid tooth, as the reference
        losses[1] = (float)(dir / n_dir);
        losses[2] = (float)(chamf / (double)nb);
        s_tot[0] = n_cen, s_tot[1] = n_dir;
    }
    __syncthreads();
    const double n_cen = s_tot[0], n_dir = s_tot[1];
    for (int e = tid; e < nb * kLossTeeth; e += kWave) {
        const int b = e / kLossTeeth, t = e % kLossTeeth, n_t = counts[e];
        const double k_t = sums[b * kLossPartials + 3 * t + 2];
        scales[b * kLossScales + 2 * t] = n_t >= 5 ? (float)(1.0 / ((double)n_t * n_cen)) : 0.0f;
        scales[b * kLossScales + 2 * t + 1] = n_t >= 5 && k_t > 0.0 ? (float)(1.0 / (k_t * n_dir)) : 0.0f;
    }
    for (int b = tid; b < nb; b += kWave) {
        int valid = 0;
        for (int t = 0; t < kLossTeeth; ++t) valid += counts[b * kLossTeeth + t] >= 5;
        const double fg = sums[b * kLossPartials + 3 * kLossTeeth + 1];
        scales[b * kLossScales + 2 * kLossTeeth] = valid >= 2 && fg > 0.0 ? (float)(1.0 / (fg * (double)nb)) : 0.0f;
    }
}

// grid (blocks per scan, B), grid-stride.  grad (B, 3, n) = g[0] d offset_loss + g[1] d dir_loss + g[2] d chamf_loss.
__global__ void __launch_bounds__(kLossThreads) offset_loss_backward_kernel(int n, const float *__restrict__ offset,
                                                                            const float *__restrict__ xyz,
                                                                            const long long *__restrict__ labels,
                                                                            const int *__restrict__ counts,
                                                                            const float *__restrict__ cent,
                                                                            const float *__restrict__ scales,
                                                                            const float *__restrict__ g, float *__restrict__ grad) {
    __shared__ float s_c[kLossTeeth][3];
    __shared__ int s_valid[kLossTeeth];
    __shared__ float s_scale[kLossScales];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < kLossTeeth) {
        s_valid[tid] = counts[b * kLossTeeth + tid] >= 5;
        for (int a = 0; a < 3; ++a) s_c[tid][a] = cent[(b * kLossTeeth + tid) * 3 + a];
    }
    if (tid < kLossScales) s_scale[tid] = scales[b * kLossScales + tid];
    __syncthreads();
    const float g_off = g[0], g_dir = g[1], g_ch = g[2];
    const float *O = offset + (long long)b * 3 * n, *X = xyz + (long long)b * 3 * n;
    const long long *L = labels + (long long)b * n;
    float *G = grad + (long long)b * 3 * n;
    for (int i = blockIdx.x * kLossThreads + tid; i < n; i += gridDim.x * kLossThreads) {
        const long long v = L[i];
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        if (v >= 0 && v < kLossTeeth) {
            const int lab = (int)v;
            const float px = X[i], py = X[n + i], pz = X[2 * n + i];
            const float ox = O[i], oy = O[n + i], oz = O[2 * n + i];
            const float mx = px + ox, my = py + oy, mz = pz + oz;
            if (s_valid[lab]) {
                const float w = 2.0f * (g_off * s_scale[2 * lab]);
                gx = w * (mx - s_c[lab][0]), gy = w * (my - s_c[lab][1]), gz = w * (mz - s_c[lab][2]);
                const float onorm = sqrtf(sumsq3(ox, oy, oz));
                if (onorm > kDirMinNorm) {             // a point the term does not keep, a zero offset included: no gradient
                    const DirTerm d = dir_term(px, py, pz, ox, oy, oz, s_c[lab], onorm);
                    const float u = (2.0f * (g_dir * s_scale[2 * lab + 1])) * (d.dot - 1.0f) / onorm;
                    gx += u * (d.dx - d.dot * d.ox), gy += u * (d.dy - d.dot * d.oy), gz += u * (d.dz - d.dot * d.oz);
                }
            }
            const float s_ch = s_scale[2 * kLossTeeth];
            if (s_ch != 0.0f) {                        // at least two valid teeth
                const Nearest2 nn = nearest2(mx, my, mz, s_c, s_valid, kLossTeeth);
                const float *c1 = s_c[nn.c1], *c2 = s_c[nn.c2];
                const float u = (g_ch * s_ch) / (nn.d2 * nn.d2);
                gx += u * (2.0f * (mx - c1[0]) * nn.d2 - 2.0f * (mx - c2[0]) * nn.d1);
                gy += u * (2.0f * (my - c1[1]) * nn.d2 - 2.0f * (my - c2[1]) * nn.d1);
                gz += u * (2.0f * (mz - c1[2]) * nn.d2 - 2.0f * (mz - c2[2]) * nn.d1);
            }
        }
        G[i] = gx, G[n + i] = gy, G[2 * n + i] = gz;
    }
}

// ---- tsegnet: centroid_loss ----------------------------------------------------------------------------------------------
constexpr int kCentPartials = 7;   // per scan: smooth-L1 sum, sum d1 | distance <= 0.2, its count, sum d1/d2 | d1 <= 0.2, its count,
                                   // sum g | g <= 0.2, its count
// scales (4): 1 / (B M), 1 / forward count, 1 / reverse count, 1 / ratio count (0 where the count is 0)

__device__ __forceinline__ void load_centroids(int b, int nc, const float *centroid, const unsigned char *exists, float (*s_c)[3],
                                               int *s_use) {
    const int tid = threadIdx.x;
    if (tid < kLossTeeth) {
        const bool in = tid < nc;
        s_use[tid] = in && (!exists || exists[b * nc + tid]);
        for (int a = 0; a < 3; ++a) s_c[tid][a] = in ? centroid[((long long)b * 3 + a) * nc + tid] : 0.0f;
    }
}

// One workgroup per scan.  partials (B, kCentPartials) float64; rev_arg (B, 16) int32: the point nearest to centroid c after the
// move where that squared distance is <= 0.2 (lowest index on a tie), otherwise -1.
__global__ void __launch_bounds__(kLossThreads) centroid_loss_points_kernel(int m, int nc, const float *__restrict__ offset,
                                                                            const float *__restrict__ xyz,
                                                                            const float *__restrict__ distance,
                                                                            const float *__restrict__ centroid,
                                                                            const unsigned char *__restrict__ exists,
                                                                            double *__restrict__ partials, int *__restrict__ rev_arg) {
    __shared__ float s_c[kLossTeeth][3];
    __shared__ int s_use[kLossTeeth];
    __shared__ double s_w[kLossWaves][5];
    __shared__ unsigned long long s_key[kLossWaves][kLossTeeth];
    __shared__ double s_g[kLossTeeth];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    load_centroids(b, nc, centroid, exists, s_c, s_use);
    __syncthreads();
    int n_use = 0;
    for (int c = 0; c < kLossTeeth; ++c) n_use += s_use[c];
    const float *O = offset + (long long)b * 3 * m, *X = xyz + (long long)b * 3 * m, *D = distance + (long long)b * m;
    double a_sl = 0.0, a_fwd = 0.0, a_nfwd = 0.0, a_ratio = 0.0, a_nratio = 0.0;
    unsigned long long key[kLossTeeth];
#pragma unroll
    for (int c = 0; c < kLossTeeth; ++c) key[c] = ~0ull;
    for (int j = tid; j < m; j += kLossThreads) {
        const float px = X[j], py = X[m + j], pz = X[2 * m + j];
        const float mx = px + O[j], my = py + O[m + j], mz = pz + O[2 * m + j];
        const float dist = D[j];
        float ds = INFINITY, d1 = INFINITY, d2 = INFINITY;
#pragma unroll
        for (int c = 0; c < kLossTeeth; ++c) {
            if (!s_use[c]) continue;                   // uniform
            ds = fminf(ds, dist_direct_nofma(px - s_c[c][0], py - s_c[c][1], pz - s_c[c][2]));
            const float d = dist_direct_nofma(mx - s_c[c][0], my - s_c[c][1], mz - s_c[c][2]);
            if (d < d1) d2 = d1, d1 = d;
            else if (d < d2) d2 = d;
            const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j;   // d >= 0: bits order like values
            key[c] = k < key[c] ? k : key[c];
        }
        const float diff = dist - sqrtf(ds), ad = fabsf(diff);
        a_sl += (double)(ad < 1.0f ? 0.5f * diff * diff : ad - 0.5f);
        if (dist <= kCentMask) a_fwd += (double)d1, a_nfwd += 1.0;
        if (d1 <= kCentMask) a_ratio += (double)(n_use >= 2 ? d1 / d2 : NAN), a_nratio += 1.0;
    }
    a_sl = wave_sum_f64(a_sl), a_fwd = wave_sum_f64(a_fwd), a_nfwd = wave_sum_f64(a_nfwd);
    a_ratio = wave_sum_f64(a_ratio), a_nratio = wave_sum_f64(a_nratio);
    if (lane == 0) s_w[wave][0] = a_sl, s_w[wave][1] = a_fwd, s_w[wave][2] = a_nfwd, s_w[wave][3] = a_ratio, s_w[wave][4] = a_nratio;
#pragma unroll
    for (int c = 0; c < kLossTeeth; ++c) {
        const unsigned long long k = wave_min_u64(key[c]);
        if (lane == 0) s_key[wave][c] = k;
    }
    __syncthreads();
    if (tid < kLossTeeth) {
        unsigned long long k = s_key[0][tid];
        for (int w = 1; w < kLossWaves; ++w) k = s_key[w][tid] < k ? s_key[w][tid] : k;
        const float gd = __uint_as_float((unsigned)(k >> 32));
        const bool in = s_use[tid] && gd <= kCentMask;     // an unused slot keeps the all-ones key: NaN, not <=
        s_g[tid] = in ? (double)gd : -1.0;
        rev_arg[b * kLossTeeth + tid] = in ? (int)(unsigned)k : -1;
    }
    __syncthreads();
    if (tid < 5) {
        double v = 0.0;
        for (int w = 0; w < kLossWaves; ++w) v += s_w[w][tid];
        partials[b * kCentPartials + tid] = v;
    }
    if (tid == 5) {
        double v = 0.0, cnt = 0.0;
        for (int c = 0; c < kLossTeeth; ++c)
            if (s_g[c] >= 0.0) v += s_g[c], cnt += 1.0;
        partials[b * kCentPartials + 5] = v;
        partials[b * kCentPartials + 6] = cnt;
    }
}

__global__ void __launch_bounds__(kWave) centroid_loss_finish_kernel(int nb, int m, const double *__restrict__ partials,
                                                                     float *__restrict__ losses, float *__restrict__ scales) {
    if (threadIdx.x != 0) return;
    double t[kCentPartials];
    for (int q = 0; q < kCentPartials; ++q) t[q] = 0.0;
    for (int b = 0; b < nb; ++b)
        for (int q = 0; q < kCentPartials; ++q) t[q] += partials[b * kCentPartials + q];
    const double total = (double)nb * (double)m;
    losses[0] = (float)(t[0] / total);
    losses[1] = (float)(t[1] / t[2] + t[5] / t[6]);    // an empty mask: 0 / 0 = NaN, as the reference
    losses[2] = (float)(t[3] / t[4]);
    scales[0] = (float)(1.0 / total);
    scales[1] = t[2] > 0.0 ? (float)(1.0 / t[2]) : 0.0f;
    scales[2] = t[6] > 0.0 ? (float)(1.0 / t[6]) : 0.0f;
    scales[3] = t[4] > 0.0 ? (float)(1.0 / t[4]) : 0.0f;
}

// grid (blocks per scan, B), grid-stride.  g (3): the gradients of dist_loss, cent_loss, chamf_loss.
__global__ void __launch_bounds__(kLossThreads) centroid_loss_backward_kernel(int m, int nc, const float *__restrict__ offset,
                                                                              const float *__restrict__ xyz,
                                                                              const float *__restrict__ distance,
                                                                              const float *__restrict__ centroid,
                                                                              const unsigned char *__restrict__ exists,
                                                                              const float *__restrict__ scales,
                                                                              const int *__restrict__ rev_arg, const float *__restrict__ g,
                                                                              float *__restrict__ grad_offset,
                                                                              float *__restrict__ grad_distance) {
    __shared__ float s_c[kLossTeeth][3];
    __shared__ int s_use[kLossTeeth], s_arg[kLossTeeth];
    const int b = blockIdx.y, tid = threadIdx.x;
    load_centroids(b, nc, centroid, exists, s_c, s_use);
    if (tid < kLossTeeth) s_arg[tid] = rev_arg[b * kLossTeeth + tid];
    __syncthreads();
    int n_use = 0;
    for (int c = 0; c < kLossTeeth; ++c) n_use += s_use[c];
    const float w_dist = g[0] * scales[0], w_fwd = g[1] * scales[1], w_rev = g[1] * scales[2], w_ratio = g[2] * scales[3];
    const float *O = offset + (long long)b * 3 * m, *X = xyz + (long long)b * 3 * m, *D = distance + (long long)b * m;
    float *GO = grad_offset + (long long)b * 3 * m, *GD = grad_distance + (long long)b * m;
    for (int j = blockIdx.x * kLossThreads + tid; j < m; j += gridDim.x * kLossThreads) {
        const float px = X[j], py = X[m + j], pz = X[2 * m + j];
        const float mx = px + O[j], my = py + O[m + j], mz = pz + O[2 * m + j];
        const float dist = D[j];
        float ds = INFINITY;
        for (int c = 0; c < kLossTeeth; ++c)
            if (s_use[c]) ds = fminf(ds, dist_direct_nofma(px - s_c[c][0], py - s_c[c][1], pz - s_c[c][2]));
        const float diff = dist - sqrtf(ds);
        GD[j] = w_dist * fminf(fmaxf(diff, -1.0f), 1.0f);          // smooth-L1's derivative, beta 1
        float gx = 0.0f, gy = 0.0f, gz = 0.0f;
        if (n_use >= 1) {
            const Nearest2 nn = nearest2(mx, my, mz, s_c, s_use, kLossTeeth);
            const float *c1 = s_c[nn.c1];
            if (dist <= kCentMask) {
                const float w = 2.0f * w_fwd;
                gx += w * (mx - c1[0]), gy += w * (my - c1[1]), gz += w * (mz - c1[2]);
            }
            if (nn.d1 <= kCentMask && n_use >= 2) {
                const float *c2 = s_c[nn.c2];
                const float u = w_ratio / (nn.d2 * nn.d2);
                gx += u * (2.0f * (mx - c1[0]) * nn.d2 - 2.0f * (mx - c2[0]) * nn.d1);
                gy += u * (2.0f * (my - c1[1]) * nn.d2 - 2.0f * (my - c2[1]) * nn.d1);
                gz += u * (2.0f * (mz - c1[2]) * nn.d2 - 2.0f * (mz - c2[2]) * nn.d1);
            }
            for (int c = 0; c < kLossTeeth; ++c) {                 // the reverse direction: centroids whose nearest point this is
                if (s_arg[c] != j) continue;
                const float w = 2.0f * w_rev;
                gx += w * (mx - s_c[c][0]), gy += w * (my - s_c[c][1]), gz += w * (mz - s_c[c][2]);
            }
        }
        GO[j] = gx, GO[m + j] = gy, GO[2 * m + j] = gz;
    }
}

static int loss_blocks(int n, int cap) {
    const int need = (n + kLossThreads - 1) / kLossThreads;
    return need < cap ? need : cap;
}

}  // namespace tgn

using namespace tgn;

TGN_API size_t tgn_offset_loss_workspace_bytes(int b, int n) {
    if (b < 1 || n < 1) return 0;
    return ((size_t)b * loss_blocks(n, kLossMaxBlocks) + (size_t)b) * kLossPartials * sizeof(double);
}

TGN_API int tgn_offset_loss_forward(int b, int n, const float *offset, const float *xyz, const long long *labels, const int *counts,
                                    const float *cent, float *losses, float *scales, void *workspace, size_t ws_bytes,
                                    tgn_stream_t stream) {
    if (b < 1 || b > 65535 || n < 1 || !offset || !xyz || !labels || !counts || !cent || !losses || !scales || !workspace ||
        ws_bytes < tgn_offset_loss_workspace_bytes(b, n)) {
        set_error("tgn_offset_loss_forward: bad arguments (b=%d n=%d ws_bytes=%zu; need 1 <= b <= 65535, n >= 1, non-NULL pointers, "
                  "ws_bytes >= tgn_offset_loss_workspace_bytes(b, n))", b, n, ws_bytes);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    int *err = index_error_word((hipStream_t)stream);
    if (!err) {
        set_error("tgn_offset_loss_forward: cannot allocate the error word");
        return TGN_ERR_LAUNCH;
    }
    const int blocks = loss_blocks(n, kLossMaxBlocks);
    double *partials = (double *)workspace, *sums = partials + (size_t)b * blocks * kLossPartials;
    hipLaunchKernelGGL(offset_loss_points_kernel, dim3(blocks, b), dim3(kLossThreads), 0, (hipStream_t)stream, n, offset, xyz, labels,
                       counts, cent, partials, err);
    hipLaunchKernelGGL(offset_loss_finish_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, b, blocks, counts, partials, sums, losses,
                       scales);
    return check_launch("tgn_offset_loss_forward");
}

TGN_API int tgn_offset_loss_backward(int b, int n, const float *offset, const float *xyz, const long long *labels, const int *counts,
                                     const float *cent, const float *scales, const float *grad_losses, float *grad_offset,
                                     tgn_stream_t stream) {
    if (b < 1 || b > 65535 || n < 1 || !offset || !xyz || !labels || !counts || !cent || !scales || !grad_losses || !grad_offset) {
        set_error("tgn_offset_loss_backward: bad arguments (b=%d n=%d; need 1 <= b <= 65535, n >= 1, non-NULL pointers)", b, n);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(offset_loss_backward_kernel, dim3(loss_blocks(n, 1024), b), dim3(kLossThreads), 0, (hipStream_t)stream, n, offset,
                       xyz, labels, counts, cent, scales, grad_losses, grad_offset);
    return check_launch("tgn_offset_loss_backward");
}

TGN_API size_t tgn_centroid_loss_workspace_bytes(int b) { return b < 1 ? 0 : (size_t)b * kCentPartials * sizeof(double); }

TGN_API int tgn_centroid_loss_forward(int b, int m, int c, const float *offset, const float *xyz, const float *distance,
                                      const float *centroid, const unsigned char *exists, float *losses, float *scales, int *rev_arg,
                                      void *workspace, size_t ws_bytes, tgn_stream_t stream) {
    if (b < 1 || b > 65535 || m < 1 || c < 1 || c > kLossTeeth || !offset || !xyz || !distance || !centroid || !losses || !scales ||
        !rev_arg || !workspace || ws_bytes < tgn_centroid_loss_workspace_bytes(b)) {
        set_error("tgn_centroid_loss_forward: bad arguments (b=%d m=%d c=%d ws_bytes=%zu; need 1 <= b <= 65535, m >= 1, 1 <= c <= %d, "
                  "non-NULL pointers, ws_bytes >= tgn_centroid_loss_workspace_bytes(b))", b, m, c, ws_bytes, kLossTeeth);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(centroid_loss_points_kernel, dim3(b), dim3(kLossThreads), 0, (hipStream_t)stream, m, c, offset, xyz, distance,
                       centroid, exists, (double *)workspace, rev_arg);
    hipLaunchKernelGGL(centroid_loss_finish_kernel, dim3(1), dim3(kWave), 0, (hipStream_t)stream, b, m, (const double *)workspace, losses,
                       scales);
    return check_launch("tgn_centroid_loss_forward");
}

TGN_API int tgn_centroid_loss_backward(int b, int m, int c, const float *offset, const float *xyz, const float *distance,
                                       const float *centroid, const unsigned char *exists, const float *scales, const int *rev_arg,
                                       const float *grad_losses, float *grad_offset, float *grad_distance, tgn_stream_t stream) {
    if (b < 1 || b > 65535 || m < 1 || c < 1 || c > kLossTeeth || !offset || !xyz || !distance || !centroid || !scales || !rev_arg ||
        !grad_losses || !grad_offset || !grad_distance) {
        set_error("tgn_centroid_loss_backward: bad arguments (b=%d m=%d c=%d; need 1 <= b <= 65535, m >= 1, 1 <= c <= %d, non-NULL "
                  "pointers)", b, m, c, kLossTeeth);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(centroid_loss_backward_kernel, dim3(loss_blocks(m, 1024), b), dim3(kLossThreads), 0, (hipStream_t)stream, m, c,
                       offset, xyz, distance, centroid, exists, scales, rev_arg, grad_losses, grad_offset, grad_distance);
    return check_launch("tgn_centroid_loss_backward");
}
