// metrics.hip -- scoring a predicted segmentation against its ground truth: the reference's cal_metric (eval_visualize_results.py:20-57),
// which loops over the predicted instances with about ten full-length numpy passes each.  All of it is a function of two small integer
// tables per scan, so the vertices are read once:
//   tgn_seg_confusion         ins_gt[p][g] / ins_sem[p][s]: vertices with ins == p and gt == g / sem == s, for b scans packed end to end
//   tgn_seg_confusion_logits  the same tables for a semantic network's (B, C, N) logits, torch.argmax fused in
//   tgn_seg_scores            per scan: the majority tooth of every instance, then IoU, F1, ACC and SEM_ACC in float64
// The tables are integer counts (LDS adds per workgroup, then integer atomics into global memory: no arrival order reaches a value) and
// the scores are float64 arithmetic in the reference's order, unfused, so the outputs equal the reference's bit for bit.
#include "tgn_common.h"

namespace tgn {

constexpr int kSegThreads = 256;
constexpr int kSegMaxLab = 64;
constexpr int kSegChunk = 8192;          // vertices of the packed array one workgroup takes (tgn_seg_confusion_chunk)
constexpr int kSegLogitChunk = 2048;     // vertices of one scan a workgroup of the logits kernel takes
constexpr int kSegTabInts = 2 * kSegMaxLab * kSegMaxLab;      // both tables of one workgroup in LDS: 32 KB

// One count per lane with key >= 0 into tab[key] (LDS).  Most vertices of a jaw are gingiva and neighbouring vertices share a tooth, so
// the lanes of a wave mostly hold one key and would queue on one LDS word: the lanes that hold the first active lane's key are counted
// with a ballot and added once; only the others add one each.  Every lane of the wave must call it (key < 0: nothing to count).
__device__ __forceinline__ void wave_count(int *tab, int key, int lane) {
    const unsigned long long act = __ballot(key >= 0);
    if (act == 0) return;                                   // wave-uniform
    const int lead = __ffsll((long long)act) - 1;
    const int k0 = __shfl(key, lead);
    const unsigned long long same = __ballot(key == k0);
    if (lane == lead) atomicAdd(&tab[k0], (int)__popcll(same));
    else if (key >= 0 && key != k0) atomicAdd(&tab[key], 1);
}

// The workgroup's LDS tables (the first `ints` words, a multiple of 4; [0, l2) is ins_gt, [l2, 2 l2) ins_sem) into one scan's global
// tables and back to zero.  Barriers on both sides: the caller's adds are complete before, the zeros are visible after.
__device__ __forceinline__ void seg_flush(int *s_tab, int ints, int l2, int *__restrict__ g_gt, int *__restrict__ g_sem) {
    __syncthreads();
    for (int e = 4 * threadIdx.x; e < ints; e += 4 * kSegThreads) {
        const int4 v = *reinterpret_cast<const int4 *>(s_tab + e);
        if ((v.x | v.y | v.z | v.w) == 0) continue;
        const int q[4] = {v.x, v.y, v.z, v.w};
        for (int j = 0; j < 4; ++j) {
            const int f = e + j;
            if (q[j] != 0 && f < 2 * l2) atomicAdd(f < l2 ? g_gt + f : g_sem + (f - l2), q[j]);
        }
        *reinterpret_cast<int4 *>(s_tab + e) = make_int4(0, 0, 0, 0);
    }
    __syncthreads();
}

__device__ __forceinline__ void seg_zero(int *s_tab, int ints) {
    for (int e = 4 * threadIdx.x; e < ints; e += 4 * kSegThreads) *reinterpret_cast<int4 *>(s_tab + e) = make_int4(0, 0, 0, 0);
    __syncthreads();
}

__device__ __forceinline__ bool seg_in(long long v, int nlab) { return v >= 0 && v < nlab; }

// Workgroup k takes vertices [k * kSegChunk, (k + 1) * kSegChunk) of the packed array and walks the scans that overlap them: for each,
// its vertices of the chunk into the LDS tables, then the tables into that scan's global ones.  Whatever `offset` holds, a load stays
// inside the chunk and inside [0, n), and a table index inside [0, b).  VEC: the three arrays are 16-byte aligned and a lane reads two
// labels of each per load; otherwise one.
template <bool VEC>
__global__ void __launch_bounds__(kSegThreads) seg_confusion_kernel(int b, long long n, const int *__restrict__ offset,
                                                                    const long long *__restrict__ gt, const long long *__restrict__ sem,
                                                                    const long long *__restrict__ ins, int nlab, int *__restrict__ ins_gt,
                                                                    int *__restrict__ ins_sem, int *__restrict__ err) {
    __shared__ __attribute__((aligned(16))) int s_tab[kSegTabInts];
    const int tid = threadIdx.x, lane = tid % kWave;
    const int l2 = nlab * nlab, ints = (2 * l2 + 3) & ~3;
    int *s_gt = s_tab, *s_sem = s_tab + l2;
    const long long cs = (long long)blockIdx.x * kSegChunk;
    const long long ce = cs + kSegChunk < n ? cs + kSegChunk : n;
    seg_zero(s_tab, ints);
    int s = 0;
    {
        int hi = b - 1;                                    // first scan whose end lies beyond the chunk's first vertex
        while (s < hi) {
            const int mid = (s + hi) >> 1;
            if ((long long)offset[mid] > cs) hi = mid;
            else s = mid + 1;
        }
    }
    bool bad = false;
    for (; s < b; ++s) {
        long long lo = s ? (long long)offset[s - 1] : 0, hi = (long long)offset[s];
        lo = lo < cs ? cs : lo;
        hi = hi > ce ? ce : hi;
        if (lo >= ce) break;
        if (hi <= lo) continue;                            // an empty scan, or one that ends in front of the chunk
        constexpr int W = VEC ? 2 : 1;
        const long long first = VEC ? (lo & ~1LL) : lo;    // cs is even, so `first` stays inside the chunk
        const int rounds = (int)((hi - first + W * kSegThreads - 1) / (W * kSegThreads));
        for (int r = 0; r < rounds; ++r) {                 // (wave-uniform trip count: wave_count ballots)
            const long long i = first + ((long long)r * kSegThreads + tid) * W;
            long long g[W], m[W], p[W];
            for (int j = 0; j < W; ++j) g[j] = m[j] = p[j] = -1;
            if constexpr (VEC) {
                if (i + 1 < n && i < hi) {                  // (n odd: the last vertex is read alone below)
                    const longlong2 vg = *reinterpret_cast<const longlong2 *>(gt + i);
                    const longlong2 vm = *reinterpret_cast<const longlong2 *>(sem + i);
                    const longlong2 vp = *reinterpret_cast<const longlong2 *>(ins + i);
                    g[0] = vg.x, g[1] = vg.y, m[0] = vm.x, m[1] = vm.y, p[0] = vp.x, p[1] = vp.y;
                } else if (i < hi) {
                    g[0] = gt[i], m[0] = sem[i], p[0] = ins[i];
                }
            } else {
                if (i < hi) g[0] = gt[i], m[0] = sem[i], p[0] = ins[i];
            }
            for (int j = 0; j < W; ++j) {
                const long long v = i + j;
                int ka = -1, ks = -1;
                if (v >= lo && v < hi) {
                    if (seg_in(g[j], nlab) && seg_in(m[j], nlab) && seg_in(p[j], nlab)) {
                        ka = (int)p[j] * nlab + (int)g[j];
                        ks = (int)p[j] * nlab + (int)m[j];
                    } else {
                        bad = true;
                    }
                }
                wave_count(s_gt, ka, lane);
                wave_count(s_sem, ks, lane);
            }
        }
        seg_flush(s_tab, ints, l2, ins_gt + (long long)s * l2, ins_sem + (long long)s * l2);
    }
    if (bad) atomicOr(err, kIndexErrCrop);
}

// torch.argmax's order over one more value: a larger value wins, equal values keep the lower channel, a NaN beats every number and
// the first NaN stays.
__device__ __forceinline__ void argmax_step(float v, int c, float &best, int &arg) {
    if (best == best && (v > best || v != v)) {
        best = v;
        arg = c;
    }
}

// grid (chunks of a scan, B).  V = 4: N is a multiple of 4 and logits 16-byte aligned, a lane reads four vertices of a channel per load.
template <int V>
__global__ void __launch_bounds__(kSegThreads) seg_confusion_logits_kernel(int C, int N, const float *__restrict__ logits,
                                                                           const long long *__restrict__ gt, int gt_shift,
                                                                           int *__restrict__ ins_gt, int *__restrict__ ins_sem,
                                                                           int *__restrict__ err) {
    __shared__ __attribute__((aligned(16))) int s_tab[kSegTabInts];
    const int tid = threadIdx.x, lane = tid % kWave, bi = blockIdx.y;
    const int l2 = C * C, ints = (2 * l2 + 3) & ~3;
    int *s_gt = s_tab, *s_sem = s_tab + l2;
    const int cs = blockIdx.x * kSegLogitChunk, ce = min(cs + kSegLogitChunk, N);
    const float *X = logits + (long long)bi * C * N;
    const long long *G = gt + (long long)bi * N;
    seg_zero(s_tab, ints);
    bool bad = false;
    const int rounds = (ce - cs + V * kSegThreads - 1) / (V * kSegThreads);
    for (int r = 0; r < rounds; ++r) {
        const int i = cs + (r * kSegThreads + tid) * V;      // V = 4: i and ce are multiples of 4, so i < ce covers i .. i + 3
        float best[V];
        int arg[V];
        for (int j = 0; j < V; ++j) best[j] = 0.0f, arg[j] = 0;
        if (i < ce) {
            for (int c = 0; c < C; ++c) {
                float v[V];
                if constexpr (V == 4) {
                    const float4 q = *reinterpret_cast<const float4 *>(X + (long long)c * N + i);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
                    v[0] = X[(long long)c * N + i];
                }
                for (int j = 0; j < V; ++j) {
                    if (c == 0) best[j] = v[j];
                    else argmax_step(v[j], c, best[j], arg[j]);
                }
            }
        }
        for (int j = 0; j < V; ++j) {
            int ka = -1, ks = -1;
            if (i + j < ce) {
                const long long g = G[i + j] + gt_shift;
                if (seg_in(g, C)) {
                    ka = arg[j] * C + (int)g;
                    ks = arg[j] * C + arg[j];
                } else {
                    bad = true;
                }
            }
            wave_count(s_gt, ka, lane);
            wave_count(s_sem, ks, lane);
        }
    }
    seg_flush(s_tab, ints, l2, ins_gt + (long long)bi * l2, ins_sem + (long long)bi * l2);
    if (bad) atomicOr(err, kIndexErrCrop);
}

// One wave per scan.  Lane p owns instance p (the row sums, the two majority votes, the instance's terms) and column p (the ground
// truth's count); lane 0 then adds the terms of the instances that occur, in ascending p.
__global__ void __launch_bounds__(kWave) seg_scores_kernel(int nlab, const int *__restrict__ ins_gt, const int *__restrict__ ins_sem,
                                                           int is_half, double *__restrict__ scores, int *__restrict__ instances,
                                                           double *__restrict__ iou_per_instance, int *__restrict__ matched_gt) {
    __shared__ long long s_insc[kSegMaxLab], s_gtc[kSegMaxLab];
    __shared__ double s_term[3][kSegMaxLab];               // acc, f1, iou of instance p
    __shared__ int s_hit[kSegMaxLab], s_present[kSegMaxLab];
    const int i = blockIdx.x, p = threadIdx.x;
    const int *A = ins_gt + (long long)i * nlab * nlab, *S = ins_sem + (long long)i * nlab * nlab;
    long long insc = 0, gtc = 0;
    int g = 0, s = 0, tp = 0, smax = 0;
    if (p < nlab) {
        for (int k = 0; k < nlab; ++k) {
            const int a = A[p * nlab + k], m = S[p * nlab + k];
            insc += a;
            gtc += A[k * nlab + p];
            if (a > tp) tp = a, g = k;                       // the first maximum: np.unique + argmax
            if (m > smax) smax = m, s = k;
        }
    }
    s_insc[p] = insc;
    s_gtc[p] = gtc;
    __syncthreads();
    long long n = 0;
    for (int k = 0; k < nlab; ++k) n += s_insc[k];
    const bool present = p >= 1 && p < nlab && insc > 0;
    double iou = __builtin_nan("");
    if (present) {
        const long long TP = tp, FP = insc - TP, FN = s_gtc[g] - TP, TN = n - TP - FP - FN;
        s_term[0][p] = (double)(TP + TN) / (double)(FP + TP + FN + TN);
        const double prec = (double)TP / (double)(TP + FP), rec = (double)TP / (double)(TP + FN);
        s_term[1][p] = (2.0 * (prec * rec)) / (prec + rec);
        iou = (double)TP / (double)(FP + TP + FN);
        s_term[2][p] = iou;
        s_hit[p] = (s == g || (is_half && s + 8 == g)) ? 1 : 0;
    }
    s_present[p] = present ? 1 : 0;
    if (p < nlab) {
        iou_per_instance[(long long)i * nlab + p] = iou;
        matched_gt[(long long)i * nlab + p] = present ? g : -1;
    }
    __syncthreads();
    if (p == 0) {
        double acc = 0.0, f1 = 0.0, io = 0.0;
        int hit = 0, cnt = 0;
        for (int k = 1; k < nlab; ++k)
            if (s_present[k]) {
                acc = acc + s_term[0][k];
                f1 = f1 + s_term[1][k];
                io = io + s_term[2][k];
                hit += s_hit[k];
                ++cnt;
            }
        const double d = (double)cnt, nan = __builtin_nan("");
        scores[4 * i] = cnt ? io / d : nan;
        scores[4 * i + 1] = cnt ? f1 / d : nan;
        scores[4 * i + 2] = cnt ? acc / d : nan;
        scores[4 * i + 3] = cnt ? (double)hit / d : nan;
        instances[i] = cnt;
    }
}

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace tgn

using namespace tgn;

TGN_API int tgn_seg_confusion_chunk(void) { return kSegChunk; }

TGN_API int tgn_seg_confusion(int b, long long n, const int *offset, const long long *gt, const long long *sem, const long long *ins,
                              int nlab, int *ins_gt, int *ins_sem, tgn_stream_t stream) {
    if (nlab < 2 || nlab > kSegMaxLab) {
        set_error("tgn_seg_confusion: nlab %d unsupported (2 <= nlab <= %d: the tables of a workgroup live in LDS)", nlab, kSegMaxLab);
        return TGN_ERR_UNSUPPORTED;
    }
    if (b < 0 || n < 0 || n > 0x7fffffffLL || (b && (!ins_gt || !ins_sem)) || (b && n && (!offset || !gt || !sem || !ins))) {
        set_error("tgn_seg_confusion: bad arguments (b=%d n=%lld; need b >= 0, 0 <= n < 2^31, non-NULL pointers)", b, n);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (b == 0) return TGN_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = sizeof(int) * (size_t)b * nlab * nlab;
    if (hipMemsetAsync(ins_gt, 0, bytes, st) != hipSuccess || hipMemsetAsync(ins_sem, 0, bytes, st) != hipSuccess) {
        set_error("tgn_seg_confusion: hipMemsetAsync failed");
        return TGN_ERR_LAUNCH;
    }
    if (n == 0) return TGN_OK;
    int *err = index_error_word(st);
    if (!err) {
        set_error("tgn_seg_confusion: cannot allocate the error word");
        return TGN_ERR_LAUNCH;
    }
    const int blocks = (int)((n + kSegChunk - 1) / kSegChunk);
    if (aligned16(gt) && aligned16(sem) && aligned16(ins))
        hipLaunchKernelGGL(seg_confusion_kernel<true>, dim3(blocks), dim3(kSegThreads), 0, st, b, n, offset, gt, sem, ins, nlab, ins_gt,
                           ins_sem, err);
    else
        hipLaunchKernelGGL(seg_confusion_kernel<false>, dim3(blocks), dim3(kSegThreads), 0, st, b, n, offset, gt, sem, ins, nlab, ins_gt,
                           ins_sem, err);
    return check_launch("tgn_seg_confusion");
}

TGN_API int tgn_seg_confusion_logits(int B, int C, int N, const float *logits, const long long *gt, int gt_shift, int *ins_gt,
                                     int *ins_sem, tgn_stream_t stream) {
    if (C < 2 || C > kSegMaxLab) {
        set_error("tgn_seg_confusion_logits: %d channels unsupported (2 <= C <= %d: the tables of a workgroup live in LDS)", C, kSegMaxLab);
        return TGN_ERR_UNSUPPORTED;
    }
    if (B < 0 || N < 0 || B > 65535 || (B && (!ins_gt || !ins_sem)) || (B && N && (!logits || !gt))) {
        set_error("tgn_seg_confusion_logits: bad arguments (B=%d N=%d; need 0 <= B <= 65535, N >= 0, non-NULL pointers)", B, N);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (B == 0) return TGN_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes = sizeof(int) * (size_t)B * C * C;
    if (hipMemsetAsync(ins_gt, 0, bytes, st) != hipSuccess || hipMemsetAsync(ins_sem, 0, bytes, st) != hipSuccess) {
        set_error("tgn_seg_confusion_logits: hipMemsetAsync failed");
        return TGN_ERR_LAUNCH;
    }
    if (N == 0) return TGN_OK;
    int *err = index_error_word(st);
    if (!err) {
        set_error("tgn_seg_confusion_logits: cannot allocate the error word");
        return TGN_ERR_LAUNCH;
    }
    const dim3 grid((N + kSegLogitChunk - 1) / kSegLogitChunk, B);
    if (N % 4 == 0 && aligned16(logits))
        hipLaunchKernelGGL(seg_confusion_logits_kernel<4>, grid, dim3(kSegThreads), 0, st, C, N, logits, gt, gt_shift, ins_gt, ins_sem, err);
    else
        hipLaunchKernelGGL(seg_confusion_logits_kernel<1>, grid, dim3(kSegThreads), 0, st, C, N, logits, gt, gt_shift, ins_gt, ins_sem, err);
    return check_launch("tgn_seg_confusion_logits");
}

TGN_API int tgn_seg_scores(int b, int nlab, const int *ins_gt, const int *ins_sem, int is_half, double *scores, int *instances,
                           double *iou_per_instance, int *matched_gt, tgn_stream_t stream) {
    if (nlab < 2 || nlab > kSegMaxLab) {
        set_error("tgn_seg_scores: nlab %d unsupported (2 <= nlab <= %d)", nlab, kSegMaxLab);
        return TGN_ERR_UNSUPPORTED;
    }
    if (b < 0 || (b && (!ins_gt || !ins_sem || !scores || !instances || !iou_per_instance || !matched_gt))) {
        set_error("tgn_seg_scores: bad arguments (b=%d; need b >= 0 and non-NULL pointers)", b);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (b == 0) return TGN_OK;
    hipLaunchKernelGGL(seg_scores_kernel, dim3(b), dim3(kWave), 0, (hipStream_t)stream, nlab, ins_gt, ins_sem, is_half, scores, instances,
                       iou_per_instance, matched_gt);
    return check_launch("tgn_seg_scores");
}
