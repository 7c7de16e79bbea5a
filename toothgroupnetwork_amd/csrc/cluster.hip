// cluster.hip -- the clustering of tgnet_fps's unlabelled path (ops_utils.get_clustering_labels, grouping_network_module.py:57-69):
// sklearn's DBSCAN and flat-kernel MeanShift on the moved foreground points, the per-cluster moments behind its PCA split test, and
// the nearest-labelled-point vote for noise points.  The reference runs all of it on the host; these kernels reproduce its results:
//   tgn_dbscan           DBSCAN(eps, min_samples).fit(X): core flags, cluster numbers in sklearn's dbscan_inner order
//   tgn_mean_shift       MeanShift's per-seed climb (_mean_shift_single_seed), every point a seed
//   tgn_nearest_center   the index of the nearest centre, ties to the lower index
//   tgn_cluster_moments  per-label count, float64 mean and covariance (ddof = 1) of the masked points
//   tgn_cluster_vote     the most frequent of k neighbour labels, ties to the smallest label (np.unique + argmax)
// The neighbour test everywhere is KDTree's euclidean rdist in float64, ((0 + dx*dx) + dy*dy) + dz*dz <= r*r, unfused.
#include "tgn_common.h"

namespace tgn {

// ---- tgn_dbscan ----------------------------------------------------------------------------------------------------------
// A spatial hash: cell (cx, cy, cz) = floor(x / h) per axis with h = eps * (1 + 2^-10), so that two points within eps (in the
// rounded float64 test) are never more than one cell apart; the cell and the cloud hash to one of nb buckets (a power of two
// >= 2n).  A counting sort by bucket lays every bucket out contiguously; a point's candidates are the points of the (distinct)
// buckets of its 27 neighbour cells, cloud checked by index range.  Buckets shared by several cells only add candidates that fail
// the distance test, and visiting each distinct bucket once keeps every candidate counted once.
// Then: a neighbour count capped at min_samples; union-find over core pairs (the larger root always hooks under the smaller, so a
// component's root is its smallest index, whatever order the hooks land in); a scan over the root flags numbers the components in
// ascending order of their smallest core index; border points take the smallest number among their core neighbours'.
// Where a point lands inside its bucket depends on atomic order; no output does: the capped count, the min-index roots and the
// min over neighbour labels are all order-free.
constexpr int kDbThreads = 256, kScanThreads = 1024;

struct DbWs {
    int *bcount, *bstart, *cloud, *parent, *flag, *scan;
    float4 *sorted;
    unsigned char *score;
};

__host__ __device__ inline size_t db_align(size_t v) { return (v + 255) & ~(size_t)255; }

__host__ inline int db_buckets(int n) {
    int nb = 1024;
    while (nb < 2 * n && nb < (1 << 30)) nb <<= 1;
    return nb;
}

__host__ inline size_t db_layout(int n, int nb, char *base, DbWs *w) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += db_align(bytes); return p; };
    char *bc = take(sizeof(int) * nb), *bs = take(sizeof(int) * ((size_t)nb + 1)), *cl = take(sizeof(int) * (size_t)n);
    char *pa = take(sizeof(int) * (size_t)n), *fl = take(sizeof(int) * (size_t)n), *sc = take(sizeof(int) * ((size_t)n + 1));
    char *so = take(sizeof(float4) * (size_t)n), *cs = take((size_t)n);
    if (w) *w = DbWs{(int *)bc, (int *)bs, (int *)cl, (int *)pa, (int *)fl, (int *)sc, (float4 *)so, (unsigned char *)cs};
    return off;
}

__device__ __forceinline__ int db_cell(float x, double inv_h) {
    double c = floor((double)x * inv_h);
    c = c < -1073741824.0 ? -1073741824.0 : (c > 1073741823.0 ? 1073741823.0 : c);   // clamping is monotone: neighbours stay <= 1 apart
    return (int)c;
}

__device__ __forceinline__ int db_hash(int cx, int cy, int cz, int cloud, int nb) {
    unsigned h = (unsigned)cx * 73856093u ^ (unsigned)cy * 19349663u ^ (unsigned)cz * 83492791u ^ (unsigned)cloud * 2654435761u;
    h ^= h >> 15;
    h *= 0x2c1b3c6du;
    h ^= h >> 12;
    return (int)(h & (unsigned)(nb - 1));
}

__device__ __forceinline__ double rdist3(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return ((0.0 + dx * dx) + dy * dy) + dz * dz;      // sklearn's euclidean rdist, unfused (-ffp-contract=off)
}

__device__ __forceinline__ int db_cloud_of(int i, int b, const int *offset) {
    int lo = 0, hi = b - 1;                              // first cloud whose end offset exceeds i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offset[mid] > i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ void db_neighbour_buckets(const float4 &p, double inv_h, int cloud, int nb, int *bk) {
    const int cx = db_cell(p.x, inv_h), cy = db_cell(p.y, inv_h), cz = db_cell(p.z, inv_h);
    int m = 0;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                const int h = db_hash(cx + dx, cy + dy, cz + dz, cloud, nb);
                bool seen = false;
                for (int j = 0; j < m; ++j) seen |= bk[j] == h;
                bk[m] = seen ? -1 : h;
                ++m;
            }
}

__global__ void db_bucket_count_kernel(int b, int n, const float *__restrict__ xyz, const int *__restrict__ offset, double inv_h, int nb,
                                       int *__restrict__ bcount, int *__restrict__ cloud) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = db_cloud_of(i, b, offset);
    cloud[i] = c;
    const int h = db_hash(db_cell(xyz[3 * i], inv_h), db_cell(xyz[3 * i + 1], inv_h), db_cell(xyz[3 * i + 2], inv_h), c, nb);
    atomicAdd(&bcount[h], 1);
}

// exclusive scan of in[0..m) into out[0..m] (out[m] = total) by one workgroup
__global__ void __launch_bounds__(kScanThreads) db_scan_kernel(const int *__restrict__ in, int m, int *__restrict__ out) {
    __shared__ int s_wave[kScanThreads / kWave];
    __shared__ int s_carry;
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < m; base += kScanThreads) {
        const int i = base + tid;
        const int v = i < m ? in[i] : 0;
        int incl = v;
        for (int d = 1; d < kWave; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == kWave - 1) s_wave[wave] = incl;
        __syncthreads();
        int before = s_carry;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        if (i < m) out[i] = before + incl - v;
        __syncthreads();
        if (tid == kScanThreads - 1) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) out[m] = s_carry;
}

__global__ void db_scatter_kernel(int n, const float *__restrict__ xyz, double inv_h, int nb, const int *__restrict__ cloud,
                                  const int *__restrict__ bstart, int *__restrict__ bcount, float4 *__restrict__ sorted) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const int h = db_hash(db_cell(x, inv_h), db_cell(y, inv_h), db_cell(z, inv_h), cloud[i], nb);
    const int pos = bstart[h] + atomicSub(&bcount[h], 1) - 1;      // the slot inside the bucket depends on order; nothing below does
    sorted[pos] = make_float4(x, y, z, __int_as_float(i));
}

// per sorted slot: the neighbour count, capped at min_samples -> core flags (by point and by slot); parent = self
__global__ void __launch_bounds__(kDbThreads) db_core_kernel(int b, int n, const int *__restrict__ offset, double inv_h, double eps2,
                                                             int min_samples, int nb, const int *__restrict__ cloud,
                                                             const int *__restrict__ bstart, const float4 *__restrict__ sorted,
                                                             unsigned char *__restrict__ score, unsigned char *__restrict__ core,
                                                             int *__restrict__ parent) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const float4 p = sorted[s];
    const int pi = __float_as_int(p.w), c = cloud[pi];
    const int lo = c ? offset[c - 1] : 0, hi = offset[c];
    int bk[27];
    db_neighbour_buckets(p, inv_h, c, nb, bk);
    int cnt = 0;
    for (int j = 0; j < 27 && cnt < min_samples; ++j) {
        if (bk[j] < 0) continue;
        const int e = bstart[bk[j] + 1];
        for (int t = bstart[bk[j]]; t < e; ++t) {
            const float4 q = sorted[t];
            const int qi = __float_as_int(q.w);
            if (qi < lo || qi >= hi) continue;
            if (rdist3(p.x, p.y, p.z, q.x, q.y, q.z) <= eps2 && ++cnt >= min_samples) break;
        }
    }
    const unsigned char is_core = cnt >= min_samples;
    score[s] = is_core;
    core[pi] = is_core;
    parent[pi] = pi;
}

__device__ __forceinline__ int uf_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(int *parent, int x) {
    int px = uf_load(parent + x);
    while (px != x) {
        const int gp = uf_load(parent + px);
        if (gp != px) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // path halving (values only move rootwards)
        x = px;
        px = gp;
    }
    return x;
}

__device__ __forceinline__ void uf_union(int *parent, int a, int b) {
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(parent + b, b, a);     // hook the larger root under the smaller
        if (old == b) return;
        b = old;
    }
}

// per sorted slot of a core point p: union with every core q < p within eps
__global__ void __launch_bounds__(kDbThreads) db_union_kernel(int b, int n, const int *__restrict__ offset, double inv_h, double eps2,
                                                              int nb, const int *__restrict__ cloud, const int *__restrict__ bstart,
                                                              const float4 *__restrict__ sorted, const unsigned char *__restrict__ score,
                                                              int *parent) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n || !score[s]) return;
    const float4 p = sorted[s];
    const int pi = __float_as_int(p.w), c = cloud[pi];
    const int lo = c ? offset[c - 1] : 0;
    int bk[27];
    db_neighbour_buckets(p, inv_h, c, nb, bk);
    for (int j = 0; j < 27; ++j) {
        if (bk[j] < 0) continue;
        const int e = bstart[bk[j] + 1];
        for (int t = bstart[bk[j]]; t < e; ++t) {
            const float4 q = sorted[t];
            const int qi = __float_as_int(q.w);
            if (qi < lo || qi >= pi || !score[t]) continue;
            if (rdist3(p.x, p.y, p.z, q.x, q.y, q.z) <= eps2) uf_union(parent, pi, qi);
        }
    }
}

// per point: the final root (core points) and the root flags the numbering scans
__global__ void db_root_kernel(int n, const unsigned char *__restrict__ core, int *parent, int *__restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int r = -1;
    if (core[i]) {
        r = uf_find(parent, i);
        parent[i] = r;
    }
    flag[i] = r == i;
}

__global__ void db_number_kernel(int b, int n, const int *__restrict__ offset, const unsigned char *__restrict__ core,
                                 const int *__restrict__ cloud, const int *__restrict__ parent, const int *__restrict__ scan,
                                 long long *__restrict__ labels, int *__restrict__ nclusters) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < b) nclusters[i] = scan[offset[i]] - scan[i ? offset[i - 1] : 0];
    if (i >= n) return;
    const int c = cloud[i], lo = c ? offset[c - 1] : 0;
    labels[i] = core[i] ? (long long)(scan[parent[i]] - scan[lo]) : -1;
}

// per sorted slot of a non-core point: the smallest cluster number among its core neighbours (-1: noise)
__global__ void __launch_bounds__(kDbThreads) db_border_kernel(int b, int n, const int *__restrict__ offset, double inv_h, double eps2,
                                                               int nb, const int *__restrict__ cloud, const int *__restrict__ bstart,
                                                               const float4 *__restrict__ sorted, const unsigned char *__restrict__ score,
                                                               long long *__restrict__ labels) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n || score[s]) return;
    const float4 p = sorted[s];
    const int pi = __float_as_int(p.w), c = cloud[pi];
    const int lo = c ? offset[c - 1] : 0, hi = offset[c];
    int bk[27];
    db_neighbour_buckets(p, inv_h, c, nb, bk);
    long long best = -1;
    for (int j = 0; j < 27; ++j) {
        if (bk[j] < 0) continue;
        const int e = bstart[bk[j] + 1];
        for (int t = bstart[bk[j]]; t < e; ++t) {
            const float4 q = sorted[t];
            const int qi = __float_as_int(q.w);
            if (qi < lo || qi >= hi || !score[t]) continue;
            if (rdist3(p.x, p.y, p.z, q.x, q.y, q.z) <= eps2) {
                const long long l = labels[qi];
                if (best < 0 || l < best) best = l;
            }
        }
    }
    labels[pi] = best;
}

// ---- tgn_mean_shift ------------------------------------------------------------------------------------------------------
// One thread per seed; a workgroup's seeds walk the points together in ascending order, kMsThreads points at a time staged in LDS,
// and iterate until every seed of the workgroup has stopped.  A seed's sum is sequential in point order and starts from -0.0 (the
// identity of IEEE addition), so it is p0 + p1 + ... alone: numpy's row-by-row axis-0 sum over the same points in the same order, which
// starts from +0.0 and so differs in one case only (a column of nothing but -0.0 gives +0.0 there, -0.0 here).
constexpr int kMsThreads = 256;

__global__ void __launch_bounds__(kMsThreads) mean_shift_kernel(int n, const double *__restrict__ xyz, double bw2, double stop_thresh,
                                                                int max_iter, double *__restrict__ means, int *__restrict__ counts) {
    __shared__ double s_p[3][kMsThreads];
    const int tid = threadIdx.x, s = blockIdx.x * kMsThreads + tid;
    double mx = 0.0, my = 0.0, mz = 0.0;
    int cnt = 0, iter = 0;
    bool active = s < n;
    if (active) {
        mx = xyz[3 * s];
        my = xyz[3 * s + 1];
        mz = xyz[3 * s + 2];
    }
    while (__syncthreads_or(active)) {
        double sx = -0.0, sy = -0.0, sz = -0.0;
        int c = 0;
        for (int base = 0; base < n; base += kMsThreads) {
            const int m = min(kMsThreads, n - base);
            if (tid < m) {
                s_p[0][tid] = xyz[3 * (base + tid)];
                s_p[1][tid] = xyz[3 * (base + tid) + 1];
                s_p[2][tid] = xyz[3 * (base + tid) + 2];
            }
            __syncthreads();
            if (active)
                for (int j = 0; j < m; ++j) {
                    const double px = s_p[0][j], py = s_p[1][j], pz = s_p[2][j];
                    if (rdist3(mx, my, mz, px, py, pz) <= bw2) {
                        sx = sx + px;
                        sy = sy + py;
                        sz = sz + pz;
                        ++c;
                    }
                }
            __syncthreads();
        }
        if (active) {
            if (c == 0) {                       // no point within the bandwidth: the seed stops where it is, with count 0
                cnt = 0;
                active = false;
            } else {
                const double dc = (double)c, nx = sx / dc, ny = sy / dc, nz = sz / dc;
                const double dx = nx - mx, dy = ny - my, dz = nz - mz;
                const double shift = sqrt((dx * dx + dy * dy) + dz * dz);
                mx = nx;
                my = ny;
                mz = nz;
                cnt = c;
                if (shift <= stop_thresh || iter == max_iter) active = false;
                else ++iter;
            }
        }
    }
    if (s < n) {
        means[3 * s] = mx;
        means[3 * s + 1] = my;
        means[3 * s + 2] = mz;
        counts[s] = cnt;
    }
}

__global__ void nearest_center_kernel(int n, const double *__restrict__ xyz, int m, const double *__restrict__ centers,
                                      long long *__restrict__ labels) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    double best = 0.0;
    int arg = 0;
    for (int j = 0; j < m; ++j) {
        const double d = rdist3(x, y, z, centers[3 * j], centers[3 * j + 1], centers[3 * j + 2]);
        if (j == 0 || d < best) {
            best = d;
            arg = j;
        }
    }
    labels[i] = arg;
}

// ---- tgn_cluster_moments -------------------------------------------------------------------------------------------------
// One workgroup per label: a pass for the mean, a pass for the centred second moments; every sum is a per-thread sequential sum in
// point order followed by a fixed tree over the threads, so the result depends on the input alone.
constexpr int kMomThreads = 256;

__device__ double block_sum(double v, double *s_red) {
    const int tid = threadIdx.x;
    s_red[tid] = v;
    __syncthreads();
    for (int w = kMomThreads / 2; w > 0; w >>= 1) {
        if (tid < w) s_red[tid] = s_red[tid] + s_red[tid + w];
        __syncthreads();
    }
    const double r = s_red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kMomThreads) cluster_moments_kernel(int n, const float *__restrict__ xyz,
                                                                      const long long *__restrict__ labels,
                                                                      const unsigned char *__restrict__ mask, int *__restrict__ counts,
                                                                      double *__restrict__ mean, double *__restrict__ cov) {
    __shared__ double s_red[kMomThreads];
    const int l = blockIdx.x, tid = threadIdx.x;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int c = 0;
    for (int i = tid; i < n; i += kMomThreads)
        if (labels[i] == l && (!mask || mask[i])) {
            sx += (double)xyz[3 * i];
            sy += (double)xyz[3 * i + 1];
            sz += (double)xyz[3 * i + 2];
            ++c;
        }
    const double tot = block_sum((double)c, s_red);
    const double mx = block_sum(sx, s_red) / tot, my = block_sum(sy, s_red) / tot, mz = block_sum(sz, s_red) / tot;
    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += kMomThreads)
        if (labels[i] == l && (!mask || mask[i])) {
            const double dx = (double)xyz[3 * i] - mx, dy = (double)xyz[3 * i + 1] - my, dz = (double)xyz[3 * i + 2] - mz;
            a[0] += dx * dx;
            a[1] += dx * dy;
            a[2] += dx * dz;
            a[3] += dy * dy;
            a[4] += dy * dz;
            a[5] += dz * dz;
        }
    double r[6];
    for (int k = 0; k < 6; ++k) {
        const double s = block_sum(a[k], s_red);
        r[k] = tot >= 2.0 ? s / (tot - 1.0) : __builtin_nan("");      // np.cov: NaN below 2 points (0 / -1 would be -0.0 for none)
    }
    if (tid == 0) {
        counts[l] = (int)tot;
        mean[3 * l] = mx;
        mean[3 * l + 1] = my;
        mean[3 * l + 2] = mz;
        const int ix[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
        for (int k = 0; k < 9; ++k) cov[9 * l + k] = r[ix[k]];
    }
}

// ---- tgn_cluster_vote ----------------------------------------------------------------------------------------------------
constexpr int kVoteMaxK = 32;

__global__ void cluster_vote_kernel(int m, int k, const long long *__restrict__ nn_idx, int n_cand, const long long *__restrict__ cand_labels,
                                    long long *__restrict__ out, int *__restrict__ err) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    long long v[kVoteMaxK];
    bool bad = false;
    for (int j = 0; j < k; ++j) {
        long long q = nn_idx[(long long)i * k + j];
        if (q < 0 || q >= n_cand) {
            bad = true;
            q = 0;
        }
        v[j] = cand_labels[q];
    }
    long long best = 0;
    int best_c = 0;
    for (int j = 0; j < k; ++j) {
        int c = 0;
        for (int t = 0; t < k; ++t) c += v[t] == v[j];
        if (c > best_c || (c == best_c && v[j] < best)) {
            best_c = c;
            best = v[j];
        }
    }
    out[i] = best;
    if (bad && err) atomicOr(err, kIndexErrCrop);
}

}  // namespace tgn

using namespace tgn;

static inline int db_blocks(int n, int t) { return (n + t - 1) / t; }

TGN_API size_t tgn_dbscan_workspace_bytes(int b, int n) {
    if (b < 1 || n < 1) return 0;
    return db_layout(n, db_buckets(n), nullptr, nullptr);
}

TGN_API int tgn_dbscan(int b, int n, const float *xyz, const int *offset, double eps, int min_samples, long long *labels,
                       unsigned char *core, int *nclusters, void *workspace, size_t workspace_bytes, tgn_stream_t stream) {
    if (b < 1 || n < 1 || !(eps > 0.0) || !(eps < 1e30) || min_samples < 1 || !xyz || !offset || !labels || !core || !nclusters ||
        !workspace || workspace_bytes < tgn_dbscan_workspace_bytes(b, n)) {
        set_error("tgn_dbscan: bad arguments (b=%d n=%d eps=%g min_samples=%d workspace=%zu of %zu bytes; need b, n >= 1, eps > 0, "
                  "min_samples >= 1, non-NULL pointers)", b, n, eps, min_samples, workspace_bytes, tgn_dbscan_workspace_bytes(b, n));
        return TGN_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = (hipStream_t)stream;
    const int nb = db_buckets(n);
    DbWs w;
    db_layout(n, nb, (char *)workspace, &w);
    const double h = eps * (1.0 + 1.0 / 1024.0), inv_h = 1.0 / h, eps2 = eps * eps;
    if (hipMemsetAsync(w.bcount, 0, sizeof(int) * nb, st) != hipSuccess) {
        set_error("tgn_dbscan: hipMemsetAsync failed");
        return TGN_ERR_LAUNCH;
    }
    const int g = db_blocks(n, kDbThreads);
    hipLaunchKernelGGL(db_bucket_count_kernel, dim3(g), dim3(kDbThreads), 0, st, b, n, xyz, offset, inv_h, nb, w.bcount, w.cloud);
    hipLaunchKernelGGL(db_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, w.bcount, nb, w.bstart);
    hipLaunchKernelGGL(db_scatter_kernel, dim3(g), dim3(kDbThreads), 0, st, n, xyz, inv_h, nb, w.cloud, w.bstart, w.bcount, w.sorted);
    hipLaunchKernelGGL(db_core_kernel, dim3(g), dim3(kDbThreads), 0, st, b, n, offset, inv_h, eps2, min_samples, nb, w.cloud, w.bstart,
                       w.sorted, w.score, core, w.parent);
    hipLaunchKernelGGL(db_union_kernel, dim3(g), dim3(kDbThreads), 0, st, b, n, offset, inv_h, eps2, nb, w.cloud, w.bstart, w.sorted,
                       w.score, w.parent);
    hipLaunchKernelGGL(db_root_kernel, dim3(g), dim3(kDbThreads), 0, st, n, core, w.parent, w.flag);
    hipLaunchKernelGGL(db_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, w.flag, n, w.scan);
    hipLaunchKernelGGL(db_number_kernel, dim3(db_blocks(n > b ? n : b, kDbThreads)), dim3(kDbThreads), 0, st, b, n, offset, core, w.cloud,
                       w.parent, w.scan, labels, nclusters);
    hipLaunchKernelGGL(db_border_kernel, dim3(g), dim3(kDbThreads), 0, st, b, n, offset, inv_h, eps2, nb, w.cloud, w.bstart, w.sorted,
                       w.score, labels);
    return check_launch("tgn_dbscan");
}

TGN_API int tgn_mean_shift(int n, const double *xyz, double bandwidth, int max_iter, double *means, int *counts, tgn_stream_t stream) {
    if (n < 0 || !(bandwidth > 0.0) || max_iter < 0 || (n && (!xyz || !means || !counts))) {
        set_error("tgn_mean_shift: bad arguments (n=%d bandwidth=%g max_iter=%d; need bandwidth > 0, max_iter >= 0)", n, bandwidth, max_iter);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return TGN_OK;
    hipLaunchKernelGGL(mean_shift_kernel, dim3(db_blocks(n, kMsThreads)), dim3(kMsThreads), 0, (hipStream_t)stream, n, xyz,
                       bandwidth * bandwidth, 1e-3 * bandwidth, max_iter, means, counts);
    return check_launch("tgn_mean_shift");
}

TGN_API int tgn_nearest_center(int n, const double *xyz, int m, const double *centers, long long *labels, tgn_stream_t stream) {
    if (n < 0 || m < 1 || (n && (!xyz || !centers || !labels))) {
        set_error("tgn_nearest_center: bad arguments (n=%d m=%d; need m >= 1)", n, m);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return TGN_OK;
    hipLaunchKernelGGL(nearest_center_kernel, dim3(db_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, n, xyz, m, centers, labels);
    return check_launch("tgn_nearest_center");
}

TGN_API int tgn_cluster_moments(int n, const float *xyz, const long long *labels, const unsigned char *mask, int nlab, int *counts,
                                double *mean, double *cov, tgn_stream_t stream) {
    if (n < 1 || nlab < 0 || !xyz || !labels || (nlab && (!counts || !mean || !cov))) {
        set_error("tgn_cluster_moments: bad arguments (n=%d nlab=%d)", n, nlab);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (nlab == 0) return TGN_OK;
    hipLaunchKernelGGL(cluster_moments_kernel, dim3(nlab), dim3(kMomThreads), 0, (hipStream_t)stream, n, xyz, labels, mask, counts, mean,
                       cov);
    return check_launch("tgn_cluster_moments");
}

TGN_API int tgn_cluster_vote(int m, int k, const long long *nn_idx, int n_cand, const long long *cand_labels, long long *out,
                             tgn_stream_t stream) {
    if (m < 0 || k < 1 || k > kVoteMaxK || n_cand < 1 || (m && (!nn_idx || !cand_labels || !out))) {
        set_error("tgn_cluster_vote: bad arguments (m=%d k=%d n_cand=%d; need 1 <= k <= %d, n_cand >= 1)", m, k, n_cand, kVoteMaxK);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (m == 0) return TGN_OK;
    int *err = index_error_word((hipStream_t)stream);
    if (!err) {
        set_error("tgn_cluster_vote: cannot allocate the error word");
        return TGN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(cluster_vote_kernel, dim3(db_blocks(m, 256)), dim3(256), 0, (hipStream_t)stream, m, k, nn_idx, n_cand, cand_labels,
                       out, err);
    return check_launch("tgn_cluster_vote");
}
