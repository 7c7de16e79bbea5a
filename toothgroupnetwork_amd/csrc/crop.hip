// crop.hip -- the crop step between the two stages of tgnet_fps's GroupingNetworkModule
// (models/modules/grouping_network_module.py:45-72): label centroids, the k nearest points of every centroid, the centred crops.
// The reference does this on the host (numpy means, an sklearn KDTree, python gathers); these kernels reproduce its results:
//   tgn_label_centroids     numpy's xyz[label == t].mean(axis=0): a sequential float32 sum in point order, divided by the count
//   tgn_label_centroids_f64 the same mean from a float64 sum, rounded once: for consumers that want the mean, not numpy's bits
//   tgn_crop_knn            KDTree.query(k) order: ascending float64 squared distance, equal distances by ascending index
//   tgn_crop_gather_center  feats[b][:, idx] with xyz centred by a float64 mean rounded once (ops_utils.centering_object)
// Inputs the kernels cannot trust (labels, scan numbers, crop indices) latch bit 1 of the launch stream's error word
// (tgn_take_index_error) instead of faulting.
#include "tgn_common.h"

namespace tgn {

// ---- tgn_label_centroids -------------------------------------------------------------------------------------------------
// One workgroup per scan walks the scan in chunks of kCentThreads points.  Per chunk: a stable counting sort of the chunk's points by
// label into LDS (ballot per label and wave; the rank inside a wave is mbcnt, so point order is kept within a label), then lane
// (label, axis) adds that label's coordinates of the chunk, in point order, to its running float32 sum.  The dependent chain of a
// label is its point count; no lane scans points of other labels.  Acc = float is numpy's sum; Acc = double (tgn_label_centroids_f64)
// keeps the sum exact to 2^-53 of its terms and rounds the mean once: a float32 sum of n terms drifts by about sqrt(n) roundings.
constexpr int kCentThreads = 1024, kCentWaves = kCentThreads / kWave, kCentMaxLab = 64;

template <typename Acc>
__global__ void __launch_bounds__(kCentThreads) label_centroids_kernel(int n, int c_stride, const float *__restrict__ feats,
                                                                       const long long *__restrict__ labels, int nlab,
                                                                       int *__restrict__ counts, float *__restrict__ cent,
                                                                       int *__restrict__ err) {
    __shared__ float s_xyz[3][kCentThreads];           // the chunk's coordinates, sorted by label
    __shared__ int s_wcnt[kCentMaxLab][kCentWaves];    // points of label l in wave w of the chunk -> exclusive offsets
    __shared__ int s_lbase[kCentMaxLab + 1];           // first sorted slot of label l in the chunk
    __shared__ int s_wtot[kCentWaves];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const float *X = feats + (long long)b * c_stride * n;
    const long long *L = labels + (long long)b * n;
    const int my_l = tid / 3, my_ax = tid % 3;          // summing lanes: tid < 3 * nlab
    const bool summer = tid < 3 * nlab;
    Acc acc = 0;
    int total = 0;
    bool bad_seen = false;
    for (int base = 0; base < n; base += kCentThreads) {
        const int i = base + tid;
        int lab = -1;
        if (i < n) {
            const long long v = L[i];
            if (v < -1 || v >= nlab) bad_seen = true;
            else lab = (int)v;
        }
        int rank = 0;
        for (int l = 0; l < nlab; ++l) {
            const unsigned long long m = __ballot(lab == l);
            if (lab == l) rank = mbcnt(m);
            if (lane == 0) s_wcnt[l][wave] = __popcll(m);
        }
        __syncthreads();
        {                                               // exclusive offsets in (label, wave) order: one block-wide scan
            const int e = tid, el = e / kCentWaves, ew = e % kCentWaves;
            const int v = e < nlab * kCentWaves ? s_wcnt[el][ew] : 0;
            int incl = v;
            for (int d = 1; d < kWave; d <<= 1) {
                const int o = __shfl_up(incl, d);
                if (lane >= d) incl += o;
            }
            if (lane == kWave - 1) s_wtot[wave] = incl;
            __syncthreads();
            int before = 0;
            for (int w = 0; w < wave; ++w) before += s_wtot[w];
            const int excl = before + incl - v;
            if (e < nlab * kCentWaves) {
                s_wcnt[el][ew] = excl;
                if (ew == 0) s_lbase[el] = excl;
            }
            if (e == nlab * kCentWaves - 1) s_lbase[nlab] = excl + v;
        }
        __syncthreads();
        if (lab >= 0) {
            const int pos = s_wcnt[lab][wave] + rank;
            s_xyz[0][pos] = X[i];
            s_xyz[1][pos] = X[n + i];
            s_xyz[2][pos] = X[2 * n + i];
        }
        __syncthreads();
        if (summer) {
            const int lo = s_lbase[my_l], hi = s_lbase[my_l + 1];
            for (int p = lo; p < hi; ++p) acc = acc + (Acc)s_xyz[my_ax][p];
            total += hi - lo;
        }
        __syncthreads();
    }
    if (__any(bad_seen) && lane == 0 && err) atomicOr(err, kIndexErrCrop);
    if (summer) {
        cent[((long long)b * nlab + my_l) * 3 + my_ax] = (float)(acc / (Acc)total);   // 0 / 0 = NaN for an absent label, as numpy's mean
        if (my_ax == 0) counts[(long long)b * nlab + my_l] = total;
    }
}

// ---- tgn_crop_knn --------------------------------------------------------------------------------------------------------
// One workgroup per crop.  The key of point i is the bit pattern of its float64 squared distance from the centroid (non-negative
// doubles order like their bit patterns), recomputed from xyz in every pass (a 24 000-point scan is 288 KB and stays in L2):
//   1. radix select of the k-th smallest key: digits of 11 bits from the top (11,11,11,11,11,9), LDS histogram per pass;
//   2. compaction of the keys below that threshold (LDS slot counter: where an entry lands is sorted away in step 3) and of the
//      lowest-index entries equal to it (block-wide prefix of the ties in index order);
//   3. bitonic sort of the k (key, index) pairs in LDS; the pairs are distinct, so the result does not depend on slot order.
constexpr int kKnnThreads = 1024, kKnnMaxK = 4096, kKnnBins = 2048;

__device__ __forceinline__ unsigned long long crop_key(const float *X, int n, int i, double cx, double cy, double cz) {
    const double dx = (double)X[i] - cx, dy = (double)X[n + i] - cy, dz = (double)X[2 * n + i] - cz;
    const double d = ((0.0 + dx * dx) + dy * dy) + dz * dz;   // sklearn's euclidean rdist, unfused (-ffp-contract=off)
    return (unsigned long long)__double_as_longlong(d);
}

__global__ void __launch_bounds__(kKnnThreads) crop_knn_kernel(int nscan, int n, int c_stride, const float *__restrict__ feats,
                                                               const int *__restrict__ crop_scan, const float *__restrict__ cent,
                                                               int k, long long *__restrict__ idx_out, int *__restrict__ err) {
    __shared__ unsigned long long s_key[kKnnMaxK];
    __shared__ unsigned s_idx[kKnnMaxK];
    __shared__ unsigned s_hist[kKnnBins];
    __shared__ int s_weq[kKnnThreads / kWave];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_rem, s_slot, s_eqbase;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    long long *out = idx_out + (long long)t * k;
    const int b = crop_scan[t];
    if (b < 0 || b >= nscan) {                          // uniform over the block
        for (int j = tid; j < k; j += kKnnThreads) out[j] = 0;
        if (tid == 0 && err) atomicOr(err, kIndexErrCrop);
        return;
    }
    const float *X = feats + (long long)b * c_stride * n;
    const double cx = cent[3 * t], cy = cent[3 * t + 1], cz = cent[3 * t + 2];
    if (tid == 0) {
        s_prefix = 0;
        s_rem = k;
    }
    unsigned long long pmask = 0;
    for (int pass = 0; pass < 6; ++pass) {
        const int shift = pass < 5 ? 53 - 11 * pass : 0, width = pass < 5 ? 11 : 9;
        const unsigned dmask = (1u << width) - 1u;
        for (int j = tid; j < kKnnBins; j += kKnnThreads) s_hist[j] = 0;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        for (int i = tid; i < n; i += kKnnThreads) {
            const unsigned long long key = crop_key(X, n, i, cx, cy, cz);
            if ((key & pmask) == prefix) atomicAdd(&s_hist[(unsigned)(key >> shift) & dmask], 1u);
        }
        __syncthreads();
        if (wave == 0) {                                // find the digit whose bin holds the rem-th smallest remaining key
            const int per = (int)(dmask + 1) / kWave;   // 32 or 8 bins per lane
            unsigned own = 0;
            for (int j = 0; j < per; ++j) own += s_hist[lane * per + j];
            unsigned incl = own;
            for (int d = 1; d < kWave; d <<= 1) {
                const unsigned o = __shfl_up(incl, d);
                if (lane >= d) incl += o;
            }
            const unsigned excl = incl - own, rem = (unsigned)s_rem;
            if (excl < rem && rem <= incl) {            // exactly one lane
                unsigned run = excl;
                int j = 0;
                for (; j < per; ++j) {
                    const unsigned h = s_hist[lane * per + j];
                    if (run + h >= rem) break;
                    run += h;
                }
                s_prefix = prefix | ((unsigned long long)(lane * per + j) << shift);
                s_rem = (int)(rem - run);
            }
        }
        pmask |= (unsigned long long)dmask << shift;
        __syncthreads();
    }
    const unsigned long long thr = s_prefix;
    const int need_eq = s_rem, nless = k - need_eq;
    if (tid == 0) {
        s_slot = 0;
        s_eqbase = 0;
    }
    __syncthreads();
    // Three barriers per chunk.  Before the first: the slot counter's atomics and the per-wave tie counts.  Between the first and the
    // second: every thread takes s_slot into `filled` -- final for this chunk, since the chunk's atomics are behind the first barrier
    // and the next chunk's come after the third -- and places its tie from s_eqbase as the previous chunk left it.  Between the second
    // and the third: thread 0 alone advances s_eqbase, which is next written two barriers after the third.  The exit test after the
    // third barrier therefore reads the same two values in every thread: the exit is uniform.  (Reading s_slot itself there is not:
    // a wave already in the next chunk may be raising it to nless while a slower wave still reads, and the two would leave the loop
    // one chunk apart, with their barriers mispaired through the whole sort below.)
    for (int base = 0; base < n; base += kKnnThreads) {   // index order: the ties kept are the lowest-index ones
        const int i = base + tid;
        const unsigned long long key = i < n ? crop_key(X, n, i, cx, cy, cz) : ~0ull;
        if (key < thr) {
            const int pos = atomicAdd(&s_slot, 1);
            s_key[pos] = key;
            s_idx[pos] = (unsigned)i;
        }
        const bool eq = key == thr;
        const unsigned long long m = __ballot(eq);
        if (lane == 0) s_weq[wave] = __popcll(m);
        __syncthreads();
        int before = s_eqbase;
        const int filled = s_slot;
        for (int w = 0; w < wave; ++w) before += s_weq[w];
        if (eq) {
            const int r = before + mbcnt(m);
            if (r < need_eq) {
                s_key[nless + r] = key;
                s_idx[nless + r] = (unsigned)i;
            }
        }
        __syncthreads();
        if (tid == 0) {
            int all = 0;
            for (int w = 0; w < kKnnThreads / kWave; ++w) all += s_weq[w];
            s_eqbase += all;
        }
        __syncthreads();
        if (s_eqbase >= need_eq && filled >= nless) break;   // every slot filled
    }
    int P = 1;
    while (P < k) P <<= 1;
    for (int j = k + tid; j < P; j += kKnnThreads) {
        s_key[j] = ~0ull;
        s_idx[j] = 0xFFFFFFFFu;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int q = tid; q < P / 2; q += kKnnThreads) {
                const int i = 2 * q - (q & (stride - 1)), j = i + stride;
                const bool asc = (i & size) == 0;
                const unsigned long long ki = s_key[i], kj = s_key[j];
                const unsigned ii = s_idx[i], ij = s_idx[j];
                const bool gt = ki > kj || (ki == kj && ii > ij);
                if (gt == asc) {
                    s_key[i] = kj;
                    s_key[j] = ki;
                    s_idx[i] = ij;
                    s_idx[j] = ii;
                }
            }
            __syncthreads();
        }
    }
    for (int j = tid; j < k; j += kKnnThreads) out[j] = (long long)s_idx[j];
}

// ---- tgn_crop_gather_center -----------------------------------------------------------------------------------------------
// One workgroup per crop.  Channels 0..2: the gathered values' float64 sum in a fixed order (per-thread strided sums, then a tree in
// LDS), the mean rounded once to float32 and subtracted in float32; channels 3..C-1 are copied; crop labels map >= 0 to 0.
constexpr int kGatherThreads = 256;

__global__ void __launch_bounds__(kGatherThreads) crop_gather_center_kernel(
    int nscan, int n, int c, int k, const float *__restrict__ feats, const int *__restrict__ crop_scan,
    const long long *__restrict__ idx, const long long *__restrict__ labels, float *__restrict__ out,
    long long *__restrict__ out_labels, int *__restrict__ err) {
    __shared__ double s_sum[3][kGatherThreads];
    const int t = blockIdx.x, tid = threadIdx.x;
    const long long *I = idx + (long long)t * k;
    float *O = out + (long long)t * c * k;
    int b = crop_scan[t];
    bool bad = b < 0 || b >= nscan;
    if (bad) b = 0;
    const float *X = feats + (long long)b * c * n;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int j = tid; j < k; j += kGatherThreads) {
        long long p = I[j];
        if (p < 0 || p >= n) {
            bad = true;
            p = 0;
        }
        sx += (double)X[p];
        sy += (double)X[n + p];
        sz += (double)X[2 * n + p];
    }
    s_sum[0][tid] = sx;
    s_sum[1][tid] = sy;
    s_sum[2][tid] = sz;
    __syncthreads();
    for (int h = kGatherThreads / 2; h > 0; h >>= 1) {
        if (tid < h)
            for (int a = 0; a < 3; ++a) s_sum[a][tid] += s_sum[a][tid + h];
        __syncthreads();
    }
    const float mean[3] = {(float)(s_sum[0][0] / (double)k), (float)(s_sum[1][0] / (double)k), (float)(s_sum[2][0] / (double)k)};
    for (int j = tid; j < k; j += kGatherThreads) {
        long long p = I[j];
        if (p < 0 || p >= n) p = 0;
        for (int a = 0; a < 3; ++a) O[(long long)a * k + j] = X[(long long)a * n + p] - mean[a];
        for (int ch = 3; ch < c; ++ch) O[(long long)ch * k + j] = X[(long long)ch * n + p];
        if (out_labels) {
            const long long v = labels[(long long)b * n + p];
            out_labels[(long long)t * k + j] = v >= 0 ? 0 : v;
        }
    }
    if (__syncthreads_or(bad) && tid == 0 && err) atomicOr(err, kIndexErrCrop);
}

}  // namespace tgn

using namespace tgn;

template <typename Acc>
static int launch_label_centroids(const char *who, int b, int n, int c_stride, const float *feats, const long long *labels, int nlab,
                                  int *counts, float *cent, tgn_stream_t stream) {
    if (b < 1 || n < 1 || c_stride < 3 || nlab < 1 || nlab > kCentMaxLab || !feats || !labels || !counts || !cent) {
        set_error("%s: bad arguments (b=%d n=%d c_stride=%d nlab=%d; need b, n >= 1, c_stride >= 3, 1 <= nlab <= %d, "
                  "non-NULL pointers)", who, b, n, c_stride, nlab, kCentMaxLab);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    int *err = index_error_word((hipStream_t)stream);
    if (!err) {
        set_error("%s: cannot allocate the error word", who);
        return TGN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(label_centroids_kernel<Acc>, dim3(b), dim3(kCentThreads), 0, (hipStream_t)stream, n, c_stride, feats, labels, nlab,
                       counts, cent, err);
    return check_launch(who);
}

TGN_API int tgn_label_centroids(int b, int n, int c_stride, const float *feats, const long long *labels, int nlab, int *counts,
                                float *cent, tgn_stream_t stream) {
    return launch_label_centroids<float>("tgn_label_centroids", b, n, c_stride, feats, labels, nlab, counts, cent, stream);
}

TGN_API int tgn_label_centroids_f64(int b, int n, int c_stride, const float *feats, const long long *labels, int nlab, int *counts,
                                    float *cent, tgn_stream_t stream) {
    return launch_label_centroids<double>("tgn_label_centroids_f64", b, n, c_stride, feats, labels, nlab, counts, cent, stream);
}

TGN_API int tgn_crop_knn(int b, int n, int c_stride, const float *feats, int t_total, const int *crop_scan, const float *cent,
                         int k, long long *idx_out, tgn_stream_t stream) {
    if (b < 1 || n < 1 || c_stride < 3 || t_total < 0 || k < 1 || k > n || k > kKnnMaxK || !feats || (t_total && (!crop_scan || !cent || !idx_out))) {
        set_error("tgn_crop_knn: bad arguments (b=%d n=%d c_stride=%d t_total=%d k=%d; need 1 <= k <= min(n, %d), c_stride >= 3)", b, n,
                  c_stride, t_total, k, kKnnMaxK);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (t_total == 0) return TGN_OK;
    int *err = index_error_word((hipStream_t)stream);
    if (!err) {
        set_error("tgn_crop_knn: cannot allocate the error word");
        return TGN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(crop_knn_kernel, dim3(t_total), dim3(kKnnThreads), 0, (hipStream_t)stream, b, n, c_stride, feats, crop_scan,
                       cent, k, idx_out, err);
    return check_launch("tgn_crop_knn");
}

TGN_API int tgn_crop_gather_center(int b, int n, int c, int t_total, int k, const float *feats, const int *crop_scan,
                                   const long long *idx, const long long *labels, float *out, long long *out_labels,
                                   tgn_stream_t stream) {
    if (b < 1 || n < 1 || c < 3 || t_total < 0 || k < 1 || !feats || (t_total && (!crop_scan || !idx || !out)) ||
        (out_labels && !labels)) {
        set_error("tgn_crop_gather_center: bad arguments (b=%d n=%d c=%d t_total=%d k=%d; need c >= 3, k >= 1, labels with out_labels)",
                  b, n, c, t_total, k);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (t_total == 0) return TGN_OK;
    int *err = index_error_word((hipStream_t)stream);
    if (!err) {
        set_error("tgn_crop_gather_center: cannot allocate the error word");
        return TGN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(crop_gather_center_kernel, dim3(t_total), dim3(kGatherThreads), 0, (hipStream_t)stream, b, n, c, k, feats,
                       crop_scan, idx, labels, out, out_labels, err);
    return check_launch("tgn_crop_gather_center");
}
