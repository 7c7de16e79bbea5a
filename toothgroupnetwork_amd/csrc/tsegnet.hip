// tsegnet.hip -- the join between the two stages of tsegnet (models/modules/tsegnet.py:57-81) and the label painting of its inference
// pipeline (inference_pipelines/inference_pipeline_tsegnet.py:60-66).  The reference does all of it on the host (numpy filters, python
// gathers, a python loop over the crops); the clustering and the crop indices in between are cluster.hip's and crop.hip's:
//   tgn_tsg_proposals      (l3_xyz + offset)[dist < threshold], compacted in ascending point order, scan after scan
//   tgn_tsg_crop_features  the segmentation module's input: xyz and per-point features at the crop indices, plus the distance feature
//                          exp(-4 sqrt(square_distance(point, centre))); raw labels at the crop indices
//   tgn_tsg_paint          every scan point takes the tooth id of the LAST crop (largest crop number) whose mask holds it, else 0
// Inputs the kernels cannot trust (scan numbers, crop indices) latch bit 1 of the launch stream's error word (tgn_take_index_error)
// instead of faulting.
#include "tgn_common.h"

namespace tgn {

// ---- tgn_tsg_proposals ---------------------------------------------------------------------------------------------------
// One workgroup per scan, one lane per coarse point (m <= 1024).  The scan's first output row is the number of points kept in the
// scans in front of it: every workgroup counts those itself from `dist` (b * m comparisons, b small), so no workgroup waits for
// another and there is no atomic.  Inside the scan: ballot per wave, the waves' counts through LDS, mbcnt inside the wave.
constexpr int kPropMaxM = 1024, kPropMaxWaves = kPropMaxM / kWave;

__global__ void __launch_bounds__(kPropMaxM) tsg_proposals_kernel(int m, const float *__restrict__ l3_xyz,
                                                                  const float *__restrict__ offset, const float *__restrict__ dist,
                                                                  float threshold, float *__restrict__ moved, int *__restrict__ counts) {
    __shared__ int s_prev[kPropMaxWaves], s_own[kPropMaxWaves];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave, nwaves = blockDim.x / kWave;
    int prev = 0;                                          // wave-uniform: kept points of this wave's lanes in the scans in front
    for (int s = 0; s < b; ++s) {
        const bool keep = tid < m && dist[(long long)s * m + tid] < threshold;      // NaN compares false: dropped
        prev += __popcll(__ballot(keep));
    }
    const bool keep = tid < m && dist[(long long)b * m + tid] < threshold;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) {
        s_prev[wave] = prev;
        s_own[wave] = __popcll(mask);
    }
    __syncthreads();
    int base = 0, before = 0, total = 0;
    for (int w = 0; w < nwaves; ++w) {
        base += s_prev[w];
        if (w < wave) before += s_own[w];
        total += s_own[w];
    }
    if (keep) {
        const float *X = l3_xyz + (long long)b * 3 * m, *O = offset + (long long)b * 3 * m;
        float *out = moved + (long long)(base + before + mbcnt(mask)) * 3;
        for (int a = 0; a < 3; ++a) out[a] = X[a * m + tid] + O[a * m + tid];
    }
    if (tid == 0) counts[b] = total;
}

// ---- tgn_tsg_crop_features -----------------------------------------------------------------------------------------------
// Lanes run along k: the index of a crop point is read once and serves every channel, and every store of a wave is one
// contiguous 256-byte row piece.  The loads are gathers by nature (k of n points of a scan that stays in L2).
constexpr int kFeatThreads = 256;

__global__ void __launch_bounds__(kFeatThreads) tsg_crop_features_kernel(
    int nscan, int n, int c_stride, int cf, int k, const float *__restrict__ feats, const float *__restrict__ l0_points,
    const int *__restrict__ crop_scan, const float *__restrict__ cent, const long long *__restrict__ idx,
    const long long *__restrict__ labels, float *__restrict__ out, long long *__restrict__ out_labels, int *__restrict__ err) {
    const int t = blockIdx.y, j = blockIdx.x * kFeatThreads + threadIdx.x;
    if (j >= k) return;
    int b = crop_scan[t];
    bool bad = b < 0 || b >= nscan;
    if (bad) b = 0;
    long long p = idx[(long long)t * k + j];
    if (p < 0 || p >= n) {
        bad = true;
        p = 0;
    }
    if (bad && err) atomicOr(err, kIndexErrCrop);
    const float *X = feats + (long long)b * c_stride * n + p;
    float *O = out + (long long)t * (3 + cf + 1) * k + j;
    const float x = X[0], y = X[n], z = X[2 * (long long)n];
    O[0] = x;
    O[k] = y;
    O[2 * (long long)k] = z;
    if (cf > 0) {                                          // (l0_points may be NULL when cf = 0)
        const float *F = l0_points + (long long)b * cf * n + p;
        for (int ch = 0; ch < cf; ++ch) O[(long long)(3 + ch) * k] = F[(long long)ch * n];
    }
    // get_ddf (tsegnet.py:24-33): square_distance(crop points, centre) in its expanded form, not clamped -- a d that rounds below
    // zero gives NaN here exactly where the reference's torch.sqrt does
    const float cx = cent[3 * t], cy = cent[3 * t + 1], cz = cent[3 * t + 2];
    const float d = sqdist_expanded(x, y, z, sumsq3(x, y, z), cx, cy, cz, sumsq3(cx, cy, cz));
    O[(long long)(3 + cf) * k] = expf(sqrtf(d) * -4.0f);
    if (out_labels) out_labels[(long long)t * k + j] = labels[(long long)b * n + p];
}

// ---- tgn_tsg_paint -------------------------------------------------------------------------------------------------------
// Pass 1: out[scan, p] = max(crop number + 1) over the masked crop entries that name p (an integer maximum: whatever order the
// atomics land in, the result is the same).  Pass 2: 0 stays 0, v becomes ids[v - 1].  `out` is zeroed in front (a memset node).
constexpr int kPaintThreads = 256;

__global__ void __launch_bounds__(kPaintThreads) tsg_paint_mark_kernel(int nscan, int n, int k, const int *__restrict__ crop_scan,
                                                                       const long long *__restrict__ idx,
                                                                       const unsigned char *__restrict__ mask,
                                                                       unsigned long long *__restrict__ out, int *__restrict__ err) {
    const int t = blockIdx.y, j = blockIdx.x * kPaintThreads + threadIdx.x;
    if (j >= k) return;
    const long long e = (long long)t * k + j;
    if (!mask[e]) return;
    const int b = crop_scan[t];
    const long long p = idx[e];
    if (b < 0 || b >= nscan || p < 0 || p >= n) {
        if (err) atomicOr(err, kIndexErrCrop);
        return;
    }
    atomicMax(out + (long long)b * n + p, (unsigned long long)t + 1ull);
}

__global__ void __launch_bounds__(kPaintThreads) tsg_paint_lookup_kernel(long long total, const long long *__restrict__ ids,
                                                                         long long *__restrict__ out) {
    const long long i = (long long)blockIdx.x * kPaintThreads + threadIdx.x;
    if (i >= total) return;
    const long long v = out[i];
    if (v > 0) out[i] = ids[v - 1];
}

}  // namespace tgn

using namespace tgn;

TGN_API int tgn_tsg_proposals(int b, int m, const float *l3_xyz, const float *offset, const float *dist, float threshold, float *moved,
                              int *counts, tgn_stream_t stream) {
    if (b < 1 || m < 1 || m > kPropMaxM || !l3_xyz || !offset || !dist || !moved || !counts) {
        set_error("tgn_tsg_proposals: bad arguments (b=%d m=%d; need b >= 1, 1 <= m <= %d, non-NULL pointers)", b, m, kPropMaxM);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    const int threads = (m + kWave - 1) / kWave * kWave;
    hipLaunchKernelGGL(tsg_proposals_kernel, dim3(b), dim3(threads), 0, (hipStream_t)stream, m, l3_xyz, offset, dist, threshold, moved,
                       counts);
    return check_launch("tgn_tsg_proposals");
}

TGN_API int tgn_tsg_crop_features(int b, int n, int c_stride, int cf, int t_total, int k, const float *feats, const float *l0_points,
                                  const int *crop_scan, const float *cent, const long long *idx, const long long *labels, float *out,
                                  long long *out_labels, tgn_stream_t stream) {
    if (b < 1 || n < 1 || c_stride < 3 || cf < 0 || t_total < 0 || k < 1 || t_total > 65535 || !feats || (cf && !l0_points) ||
        (t_total && (!crop_scan || !cent || !idx || !out)) || (out_labels && !labels)) {
        set_error("tgn_tsg_crop_features: bad arguments (b=%d n=%d c_stride=%d cf=%d t_total=%d k=%d; need c_stride >= 3, cf >= 0, k >= 1, "
                  "t_total <= 65535, l0_points with cf, labels with out_labels)", b, n, c_stride, cf, t_total, k);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (t_total == 0) return TGN_OK;
    int *err = index_error_word((hipStream_t)stream);
    if (!err) {
        set_error("tgn_tsg_crop_features: cannot allocate the error word");
        return TGN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(tsg_crop_features_kernel, dim3((k + kFeatThreads - 1) / kFeatThreads, t_total), dim3(kFeatThreads), 0,
                       (hipStream_t)stream, b, n, c_stride, cf, k, feats, l0_points, crop_scan, cent, idx, labels, out, out_labels, err);
    return check_launch("tgn_tsg_crop_features");
}

TGN_API int tgn_tsg_paint(int b, int n, int t_total, int k, const int *crop_scan, const long long *idx, const unsigned char *mask,
                          const long long *ids, long long *out, tgn_stream_t stream) {
    if (b < 1 || n < 1 || t_total < 0 || k < 1 || t_total > 65535 || !out || (t_total && (!crop_scan || !idx || !mask || !ids))) {
        set_error("tgn_tsg_paint: bad arguments (b=%d n=%d t_total=%d k=%d; need b, n, k >= 1, t_total <= 65535, non-NULL pointers)", b, n,
                  t_total, k);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    const long long total = (long long)b * n;
    if (hipMemsetAsync(out, 0, (size_t)total * sizeof(long long), (hipStream_t)stream) != hipSuccess) return check_launch("tgn_tsg_paint");
    if (t_total == 0) return TGN_OK;
    int *err = index_error_word((hipStream_t)stream);
    if (!err) {
        set_error("tgn_tsg_paint: cannot allocate the error word");
        return TGN_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(tsg_paint_mark_kernel, dim3((k + kPaintThreads - 1) / kPaintThreads, t_total), dim3(kPaintThreads), 0,
                       (hipStream_t)stream, b, n, k, crop_scan, idx, mask, (unsigned long long *)out, err);
    hipLaunchKernelGGL(tsg_paint_lookup_kernel, dim3((unsigned)((total + kPaintThreads - 1) / kPaintThreads)), dim3(kPaintThreads), 0,
                       (hipStream_t)stream, total, ids, out);
    return check_launch("tgn_tsg_paint");
}
