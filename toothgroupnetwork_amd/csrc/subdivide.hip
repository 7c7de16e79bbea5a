// subdivide.hip -- one pass of open3d's TriangleMesh::SubdivideMidpoint on the device: what the reference's inference pipelines do to a
// mesh below 24 000 vertices before they sample it (inference_pipeline_sem.py:25-26).  The contract (include/tgn_pointops.h, section 4):
// walk the triangles in order and, per triangle (a, b, c), the edges (a,b), (b,c), (c,a); an edge is the unordered pair {min, max}; the
// first time an edge is met it gets vertex nv + (number of distinct edges met before it) = 0.5 * (V[p] + V[q]); triangle t becomes
// (a, ab, ca), (ab, b, bc), (bc, c, ca), (ab, bc, ca) at rows 4t .. 4t+3.
//
// One thread per half-edge h = 3t + e, so that "met before" is "has a smaller h":
//   sub_init_kernel      the table's keys to EMPTY, its first-occurrence words to the largest unsigned, the error word to 0
//   sub_insert_kernel    claims a slot of an open-addressed table for the key min << 32 | max (64-bit compare-and-swap, linear probing) and
//                        lowers the slot's first-occurrence word to h (integer atomic minimum): which thread claims a slot depends on the
//                        schedule, the minimum does not
//   sub_rank_kernel      flag[h] = (first[slot[h]] == h); an exclusive scan of the flags by one workgroup = the edge's rank in
//                        first-occurrence order; the total (or the negated error word) goes to the caller's counter
//   sub_vertex_kernel    old vertices (and normals) copied bit for bit, the midpoints written at nv + rank
//   sub_triangle_kernel  the four children of every triangle
// Nothing is summed across threads and no float atomic is used: every output word has one writer whose value does not depend on the
// schedule.  Every loop is bounded: a probe sequence ends after `cap` slots and latches kSubErrProbe instead of spinning.
#include "tgn_common.h"

namespace tgn {

constexpr int kSubThreads = 256, kSubScanThreads = 1024, kSubScanItems = 4;
constexpr unsigned long long kSubEmpty = ~0ull;      // never a key: both halves of a key are below 2^31
constexpr unsigned kSubNoSlot = ~0u;
constexpr int kSubErrIndex = 1;                      // a triangle index outside [0, nv)
constexpr int kSubErrProbe = 2;                      // a probe sequence ran out (the table was full)
constexpr long long kSubLimit = 1ll << 31;           // nv + 3 nf must stay below it: vertex indices and half-edge numbers are 32-bit here

struct SubWs {
    unsigned long long *keys;   // cap
    unsigned *first;            // cap: the smallest half-edge number that met the slot's edge
    int *err;                   // 1
    unsigned *slot;             // 3 nf: the slot of each half-edge (kSubNoSlot: none)
    int *rank;                  // 3 nf: exclusive scan of the first-occurrence flags
};

__host__ inline size_t sub_align(size_t v) { return (v + 255) & ~(size_t)255; }

// a power of two of at least 2 * 3 nf (and at least 1024): the load stays at or below one half
__host__ inline unsigned long long sub_capacity(long long nh) {
    unsigned long long cap = 1024;
    while (cap < 2ull * (unsigned long long)nh) cap <<= 1;
    return cap;
}

__host__ inline size_t sub_layout(long long nh, unsigned long long cap, char *base, SubWs *w) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += sub_align(bytes); return p; };
    char *k = take(sizeof(unsigned long long) * cap), *f = take(sizeof(unsigned) * cap), *e = take(sizeof(int));
    char *s = take(sizeof(unsigned) * (size_t)nh), *r = take(sizeof(int) * (size_t)nh);
    if (w) *w = SubWs{(unsigned long long *)k, (unsigned *)f, (int *)e, (unsigned *)s, (int *)r};
    return off;
}

__device__ __forceinline__ unsigned long long sub_mix(unsigned long long k) {      // the 64-bit finaliser of MurmurHash3
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

__global__ void __launch_bounds__(kSubThreads) sub_init_kernel(unsigned long long cap, unsigned long long *__restrict__ keys,
                                                               unsigned *__restrict__ first, int *__restrict__ err) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kSubThreads + threadIdx.x;
    if (i == 0) *err = 0;
    if (i >= cap) return;
    keys[i] = kSubEmpty;
    first[i] = ~0u;
}

__global__ void __launch_bounds__(kSubThreads) sub_insert_kernel(long long nv, long long nh, const long long *__restrict__ tri,
                                                                 unsigned long long cap, unsigned long long *__restrict__ keys,
                                                                 unsigned *__restrict__ first, unsigned *__restrict__ slot,
                                                                 int *__restrict__ err) {
    const long long h = (long long)blockIdx.x * kSubThreads + threadIdx.x;
    if (h >= nh) return;
    const long long t = h / 3;
    const int e = (int)(h - 3 * t);
    const long long p = tri[3 * t + e], q = tri[3 * t + (e == 2 ? 0 : e + 1)];
    if (p < 0 || p >= nv || q < 0 || q >= nv) {
        slot[h] = kSubNoSlot;
        atomicOr(err, kSubErrIndex);
        return;
    }
    const unsigned long long key = pack64((unsigned)(p < q ? p : q), (unsigned)(p < q ? q : p));
    const unsigned long long mask = cap - 1;
    unsigned long long s = sub_mix(key) & mask;
    unsigned found = kSubNoSlot;
    for (unsigned long long probe = 0; probe < cap; ++probe) {                     // bounded: at most one visit per slot
        const unsigned long long old = atomicCAS(&keys[s], kSubEmpty, key);
        if (old == kSubEmpty || old == key) {
            found = (unsigned)s;
            break;
        }
        s = (s + 1) & mask;
    }
    slot[h] = found;
    if (found == kSubNoSlot) {
        atomicOr(err, kSubErrProbe);
        return;
    }
    atomicMin(&first[found], (unsigned)h);
}

// rank[h] = number of half-edges below h that are the first of their edge; *n_new = their total, or -(error word)
__global__ void __launch_bounds__(kSubScanThreads) sub_rank_kernel(long long nh, const unsigned *__restrict__ slot,
                                                                   const unsigned *__restrict__ first, int *__restrict__ rank,
                                                                   const int *__restrict__ err, int *__restrict__ n_new) {
    __shared__ int s_wave[kSubScanThreads / kWave];
    __shared__ int s_carry;
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    constexpr long long kChunk = (long long)kSubScanThreads * kSubScanItems;
    for (long long base = 0; base < nh; base += kChunk) {
        const long long i0 = base + (long long)tid * kSubScanItems;
        int f[kSubScanItems], v = 0;
#pragma unroll
        for (int j = 0; j < kSubScanItems; ++j) {
            const long long i = i0 + j;
            f[j] = 0;
            if (i < nh) {
                const unsigned s = slot[i];
                f[j] = s != kSubNoSlot && first[s] == (unsigned)i;
            }
            v += f[j];
        }
        int incl = v;
        for (int d = 1; d < kWave; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == kWave - 1) s_wave[wave] = incl;
        __syncthreads();
        int before = s_carry;
        for (int w = 0; w < wave; ++w) before += s_wave[w];
        int run = before + incl - v;
#pragma unroll
        for (int j = 0; j < kSubScanItems; ++j) {
            if (i0 + j < nh) rank[i0 + j] = run;
            run += f[j];
        }
        __syncthreads();
        if (tid == kSubScanThreads - 1) s_carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) {
        const int e = *err;
        *n_new = e ? -e : s_carry;
    }
}

__global__ void __launch_bounds__(kSubThreads) sub_vertex_kernel(long long nv, long long nh, const double *__restrict__ v,
                                                                 const double *__restrict__ n, const long long *__restrict__ tri,
                                                                 const unsigned *__restrict__ slot, const unsigned *__restrict__ first,
                                                                 const int *__restrict__ rank, double *__restrict__ out_v,
                                                                 double *__restrict__ out_n) {
    const long long i = (long long)blockIdx.x * kSubThreads + threadIdx.x;
    if (i >= nv + nh) return;
    if (i < nv) {                                                                  // old vertices keep their indices and bits
        for (int c = 0; c < 3; ++c) out_v[3 * i + c] = v[3 * i + c];
        if (n)
            for (int c = 0; c < 3; ++c) out_n[3 * i + c] = n[3 * i + c];
        return;
    }
    const long long h = i - nv;
    const unsigned s = slot[h];
    if (s == kSubNoSlot || first[s] != (unsigned)h) return;
    const long long t = h / 3;
    const int e = (int)(h - 3 * t);
    const long long p = tri[3 * t + e], q = tri[3 * t + (e == 2 ? 0 : e + 1)];      // in range: the half-edge has a slot
    const long long o = nv + rank[h];
    for (int c = 0; c < 3; ++c) out_v[3 * o + c] = 0.5 * (v[3 * p + c] + v[3 * q + c]);
    if (n)
        for (int c = 0; c < 3; ++c) out_n[3 * o + c] = 0.5 * (n[3 * p + c] + n[3 * q + c]);   // not renormalised
}

__global__ void __launch_bounds__(kSubThreads) sub_triangle_kernel(long long nv, long long nf, const long long *__restrict__ tri,
                                                                   const unsigned *__restrict__ slot, const unsigned *__restrict__ first,
                                                                   const int *__restrict__ rank, long long *__restrict__ out_t) {
    const long long t = (long long)blockIdx.x * kSubThreads + threadIdx.x;
    if (t >= nf) return;
    const unsigned s0 = slot[3 * t], s1 = slot[3 * t + 1], s2 = slot[3 * t + 2];
    if (s0 == kSubNoSlot || s1 == kSubNoSlot || s2 == kSubNoSlot) return;           // the error word is set: the rows stay unwritten
    const long long a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    const long long ab = nv + rank[first[s0]], bc = nv + rank[first[s1]], ca = nv + rank[first[s2]];
    long long *o = out_t + 12 * t;
    o[0] = a, o[1] = ab, o[2] = ca;
    o[3] = ab, o[4] = b, o[5] = bc;
    o[6] = bc, o[7] = c, o[8] = ca;
    o[9] = ab, o[10] = bc, o[11] = ca;
}

}  // namespace tgn

using namespace tgn;

static inline unsigned sub_blocks(long long n) { return (unsigned)((n + kSubThreads - 1) / kSubThreads); }

TGN_API size_t tgn_subdivide_midpoint_workspace_bytes(long long nf) {
    if (nf < 0 || 3 * nf >= kSubLimit) return 0;
    return sub_layout(3 * nf, sub_capacity(3 * nf), nullptr, nullptr);
}

TGN_API int tgn_subdivide_midpoint(long long nv, long long nf, const double *vertices, const double *normals, const long long *triangles,
                                   double *out_vertices, double *out_normals, long long *out_triangles, int *n_new, void *workspace,
                                   size_t workspace_bytes, tgn_stream_t stream) {
    if (nv < 0 || nf < 0 || (nv && (!vertices || !out_vertices)) || (nf && (!triangles || !out_triangles)) || !n_new || !workspace ||
        (normals && !out_normals)) {
        set_error("tgn_subdivide_midpoint: bad arguments (nv=%lld nf=%lld; need nv, nf >= 0, non-NULL counter and workspace, non-NULL vertices "
                  "and out_vertices unless nv = 0, triangles and out_triangles unless nf = 0, and out_normals wherever normals are given)", nv, nf);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (nv >= kSubLimit || nf >= kSubLimit || nv + 3 * nf >= kSubLimit) {
        set_error("tgn_subdivide_midpoint: nv + 3 * nf >= 2147483648 unsupported (nv=%lld nf=%lld; vertex indices and half-edge numbers are "
                  "32-bit)", nv, nf);
        return TGN_ERR_UNSUPPORTED;
    }
    const long long nh = 3 * nf;
    const size_t need = tgn_subdivide_midpoint_workspace_bytes(nf);
    if (workspace_bytes < need) {
        set_error("tgn_subdivide_midpoint: workspace of %zu bytes, need %zu (tgn_subdivide_midpoint_workspace_bytes)", workspace_bytes, need);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long cap = sub_capacity(nh);
    SubWs w;
    sub_layout(nh, cap, (char *)workspace, &w);
    hipLaunchKernelGGL(sub_init_kernel, dim3(sub_blocks((long long)cap)), dim3(kSubThreads), 0, st, cap, w.keys, w.first, w.err);
    if (nh)
        hipLaunchKernelGGL(sub_insert_kernel, dim3(sub_blocks(nh)), dim3(kSubThreads), 0, st, nv, nh, triangles, cap, w.keys, w.first, w.slot,
                           w.err);
    hipLaunchKernelGGL(sub_rank_kernel, dim3(1), dim3(kSubScanThreads), 0, st, nh, w.slot, w.first, w.rank, w.err, n_new);
    if (nv + nh)
        hipLaunchKernelGGL(sub_vertex_kernel, dim3(sub_blocks(nv + nh)), dim3(kSubThreads), 0, st, nv, nh, vertices, normals, triangles,
                           w.slot, w.first, w.rank, out_vertices, out_normals);
    if (nf)
        hipLaunchKernelGGL(sub_triangle_kernel, dim3(sub_blocks(nf)), dim3(kSubThreads), 0, st, nv, nf, triangles, w.slot, w.first, w.rank,
                           out_triangles);
    return check_launch("tgn_subdivide_midpoint");
}
