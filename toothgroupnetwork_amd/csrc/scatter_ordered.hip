// scatter_ordered.hip -- the transposed-graph backward of the gather family (gfx950): no float atomics, the same bits every time.
//
// A scatter-add  out[idx[q]] += term(q)  is turned round: tgn_reverse_lists builds, per target row, the ascending list of the pair
// numbers q that target it, and tgn_scatter_ordered lets ONE lane group own a row and add that row's terms in list order.  The
// order of the float additions is then a property of the lists, not of the launch (include/tgn_pointops.h states both contracts).
//
//   tgn_reverse_lists     count (integer atomics) -> exclusive scan -> slot claim (integer atomics, any order) -> every segment sorted.
//                         The sorted lists are unique, so the order in which the integer atomics land does not show in the result.
//   tgn_scatter_ordered   the layout of gather.hip: a group of 2^cx_log2 lanes per output row, lanes along the channel axis.  The
//                         adds of a segment are a dependent chain; its loads are not: kAhead pairs' terms are requested before the
//                         first is added.
#include "dispatch.h"
#include "tgn_common.h"

namespace tgn {

constexpr int kRevBlock = 256;                       // threads of every pass below
constexpr int kRevScanItems = 4;                     // counts per thread of the scan's first pass
constexpr int kRevScanTile = kRevBlock * kRevScanItems;   // 1024 rows per workgroup of the scan
constexpr int kRevWaveSegment = kWave;               // segments up to a wave's lanes are sorted in registers, one wave each
constexpr int kRevLongTile = 1024;                   // pairs of a longer segment staged in LDS per round of the workgroup sort
constexpr int kRevLongOwn = 4;                       // entries a thread of that sort places per pass over the segment
constexpr int kOrderedAhead = 4;                    // pairs whose terms are in flight ahead of the add chain

struct RevWorkspace {
    int *cursor;   // b * n: the counts, then the claim cursors
    int *bsum;     // one per scan tile
    int *slots;    // b * pairs_per_batch: the claimed, unsorted lists
};

static long long rev_scan_tiles(long long rows) { return (rows + kRevScanTile - 1) / kRevScanTile; }

static size_t rev_workspace_bytes(long long rows, long long pairs) {
    return (size_t)(rows + rev_scan_tiles(rows) + pairs) * sizeof(int);
}

static unsigned rev_grid(long long items, int per_block) {
    long long blocks = (items + per_block - 1) / per_block;
    const long long cap = 256LL * 32;   // grid-stride beyond 32 workgroups per CU
    return (unsigned)(blocks < 1 ? 1 : (blocks > cap ? cap : blocks));
}

// the row a pair targets: an index outside [0, n) counts as row 0 of its batch
template <typename IdxT>
__device__ __forceinline__ long long rev_row(const IdxT *__restrict__ idx, long long q, long long pairs_per_batch, int n) {
    const long long bi = q / pairs_per_batch;
    long long v = (long long)idx[q];
    if (v < 0 || v >= n) v = 0;
    return bi * n + v;
}

__global__ __launch_bounds__(kRevBlock) void rev_zero_kernel(long long rows, int *__restrict__ cursor) {
    for (long long i = (long long)blockIdx.x * kRevBlock + threadIdx.x; i < rows; i += (long long)gridDim.x * kRevBlock) cursor[i] = 0;
}

template <typename IdxT>
__global__ __launch_bounds__(kRevBlock) void rev_count_kernel(long long pairs, long long pairs_per_batch, int n,
                                                               const IdxT *__restrict__ idx, int *__restrict__ cursor) {
    for (long long q = (long long)blockIdx.x * kRevBlock + threadIdx.x; q < pairs; q += (long long)gridDim.x * kRevBlock)
        atomicAdd(cursor + rev_row(idx, q, pairs_per_batch, n), 1);
}

// exclusive scan of the counts, pass 1: a workgroup per tile of kRevScanTile rows writes the tile-local prefixes and the tile's sum
__global__ __launch_bounds__(kRevBlock) void rev_scan_tile_kernel(long long rows, long long tiles, const int *__restrict__ cursor,
                                                                   int *__restrict__ rev_start, int *__restrict__ bsum) {
    __shared__ int part[kRevBlock];
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long base = tile * kRevScanTile + (long long)threadIdx.x * kRevScanItems;
        int v[kRevScanItems], s = 0;
#pragma unroll
        for (int u = 0; u < kRevScanItems; ++u) {
            v[u] = base + u < rows ? cursor[base + u] : 0;
            s += v[u];
        }
        part[threadIdx.x] = s;
        __syncthreads();
        for (int off = 1; off < kRevBlock; off <<= 1) {   // Hillis-Steele over the 256 thread sums
            const int add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        int run = part[threadIdx.x] - s;   // exclusive
#pragma unroll
        for (int u = 0; u < kRevScanItems; ++u) {
            if (base + u < rows) rev_start[base + u] = run;
            run += v[u];
        }
        if (threadIdx.x == kRevBlock - 1) bsum[tile] = part[kRevBlock - 1];
        __syncthreads();   // part is rewritten by the next tile
    }
}

// pass 2: ONE workgroup turns the tile sums into exclusive prefixes, kRevBlock at a time with a carry
__global__ __launch_bounds__(kRevBlock) void rev_scan_sums_kernel(long long tiles, int *__restrict__ bsum) {
    __shared__ int part[kRevBlock];
    int carry = 0;
    for (long long t0 = 0; t0 < tiles; t0 += kRevBlock) {
        const long long t = t0 + threadIdx.x;
        const int v = t < tiles ? bsum[t] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < kRevBlock; off <<= 1) {
            const int add = (int)threadIdx.x >= off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (t < tiles) bsum[t] = carry + part[threadIdx.x] - v;
        carry += part[kRevBlock - 1];
        __syncthreads();
    }
}

// pass 3: the tile prefix onto every row; the claim cursor of a row starts at its segment; the closing entry
__global__ __launch_bounds__(kRevBlock) void rev_scan_apply_kernel(long long rows, int pairs, const int *__restrict__ bsum,
                                                                    int *__restrict__ rev_start, int *__restrict__ cursor) {
    for (long long i = (long long)blockIdx.x * kRevBlock + threadIdx.x; i < rows; i += (long long)gridDim.x * kRevBlock) {
        const int s = rev_start[i] + bsum[i / kRevScanTile];
        rev_start[i] = s;
        cursor[i] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) rev_start[rows] = pairs;
}

template <typename IdxT>
__global__ __launch_bounds__(kRevBlock) void rev_claim_kernel(long long pairs, long long pairs_per_batch, int n,
                                                               const IdxT *__restrict__ idx, int *__restrict__ cursor,
                                                               int *__restrict__ slots) {
    for (long long q = (long long)blockIdx.x * kRevBlock + threadIdx.x; q < pairs; q += (long long)gridDim.x * kRevBlock) {
        const int slot = atomicAdd(cursor + rev_row(idx, q, pairs_per_batch, n), 1);
        if (slot >= 0 && slot < pairs) slots[slot] = (int)q;   // (always: the cursors partition [0, pairs))
    }
}

// Segments of at most kRevWaveSegment pairs, a wave each: lane l holds entry l, its place is the number of entries below it (the
// entries of a segment are distinct pair numbers).
__global__ __launch_bounds__(kRevBlock) void rev_sort_wave_kernel(long long rows, const int *__restrict__ rev_start,
                                                                   const int *__restrict__ slots, int *__restrict__ rev_pair) {
    const int lane = threadIdx.x & (kWave - 1);
    const int waves = kRevBlock / kWave;
    for (long long r = (long long)blockIdx.x * waves + (threadIdx.x >> 6); r < rows; r += (long long)gridDim.x * waves) {
        const int s = rev_start[r];
        const int len = rev_start[r + 1] - s;   // wave-uniform
        if (len <= 0 || len > kRevWaveSegment) continue;
        const int mine = lane < len ? slots[s + lane] : 0x7fffffff;
        int below = 0;
        for (int j = 0; j < len; ++j) below += __shfl(mine, j, kWave) < mine;
        if (lane < len) rev_pair[s + below] = mine;
    }
}

// Longer segments (a hub: a row that very many pairs target), a workgroup each: the same counting, the segment staged through LDS
// kRevLongTile entries at a time.  len^2 / kRevBlock comparisons per thread: slow for a hub, bounded, and exact.
__global__ __launch_bounds__(kRevBlock) void rev_sort_long_kernel(long long rows, const int *__restrict__ rev_start,
                                                                   const int *__restrict__ slots, int *__restrict__ rev_pair) {
    __shared__ int stage[kRevLongTile];
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const int s = rev_start[r];
        const int len = rev_start[r + 1] - s;   // workgroup-uniform
        if (len <= kRevWaveSegment) continue;
        for (long long own0 = 0; own0 < len; own0 += kRevBlock * kRevLongOwn) {
            int mine[kRevLongOwn], below[kRevLongOwn];
#pragma unroll
            for (int u = 0; u < kRevLongOwn; ++u) {
                const long long own = own0 + u * kRevBlock + (int)threadIdx.x;
                mine[u] = own < len ? slots[s + own] : 0x7fffffff;
                below[u] = 0;
            }
            for (long long t0 = 0; t0 < len; t0 += kRevLongTile) {
                const int cnt = len - t0 < kRevLongTile ? (int)(len - t0) : kRevLongTile;
                __syncthreads();   // the previous round's readers are done
                for (int e = threadIdx.x; e < cnt; e += kRevBlock) stage[e] = slots[s + t0 + e];
                __syncthreads();
                for (int e = 0; e < cnt; ++e) {
                    const int v = stage[e];
#pragma unroll
                    for (int u = 0; u < kRevLongOwn; ++u) below[u] += v < mine[u];
                }
            }
#pragma unroll
            for (int u = 0; u < kRevLongOwn; ++u)
                if (own0 + u * kRevBlock + (int)threadIdx.x < len) rev_pair[s + below[u]] = mine[u];
        }
        __syncthreads();
    }
}

// ---- the ordered scatter ----------------------------------------------------------------------------------------------------
// QUERY: term = (sign * src[(q / k) * c + ch]) * coef[q * g + ch % g]; else term = sign * src[q * c + ch].  IDENT: row r owns the
// pairs r * k .. r * k + k - 1 and the lists are not read.
template <bool QUERY, bool IDENT>
__global__ __launch_bounds__(256) void scatter_ordered_kernel(long long rows, int c, int k, int g, int cx_log2,
                                                               const int *__restrict__ rev_start, const int *__restrict__ rev_pair,
                                                               const float *__restrict__ src, const float *__restrict__ coef,
                                                               float sign, float *__restrict__ out) {
    const int cx = 1 << cx_log2;
    const int tx = threadIdx.x & (cx - 1);
    const int ty = threadIdx.x >> cx_log2;
    const int ry = blockDim.x >> cx_log2;
    for (long long r = (long long)blockIdx.x * ry + ty; r < rows; r += (long long)gridDim.x * ry) {
        long long s;
        int len;
        if (IDENT) {
            s = r * k;
            len = k;
        } else {
            s = rev_start[r];
            len = rev_start[r + 1] - (int)s;
        }
        for (int ch = tx; ch < c; ch += cx) {
            const int gc = QUERY ? ch % g : 0;
            float acc = 0.0f;
            int j = 0;
            for (; j + kOrderedAhead <= len; j += kOrderedAhead) {
                float t[kOrderedAhead], w[kOrderedAhead];
#pragma unroll
                for (int u = 0; u < kOrderedAhead; ++u) {
                    const long long q = IDENT ? s + j + u : (long long)rev_pair[s + j + u];
                    t[u] = src[(size_t)(QUERY ? q / k : q) * c + ch];
                    if (QUERY) w[u] = coef[(size_t)q * g + gc];
                }
#pragma unroll
                for (int u = 0; u < kOrderedAhead; ++u) {
                    float term = __fmul_rn(sign, t[u]);
                    if (QUERY) term = __fmul_rn(term, w[u]);
                    acc = __fadd_rn(acc, term);
                }
            }
            for (; j < len; ++j) {
                const long long q = IDENT ? s + j : (long long)rev_pair[s + j];
                float term = __fmul_rn(sign, src[(size_t)(QUERY ? q / k : q) * c + ch]);
                if (QUERY) term = __fmul_rn(term, coef[(size_t)q * g + gc]);
                acc = __fadd_rn(acc, term);
            }
            out[(size_t)r * c + ch] = acc;
        }
    }
}

}  // namespace tgn

using namespace tgn;

static bool rev_sizes_ok(int b, int n, long long pairs_per_batch) {
    return b >= 0 && n >= 0 && pairs_per_batch >= 0 && (long long)b * n < (1LL << 31) &&
           (pairs_per_batch == 0 || (long long)b <= ((1LL << 31) - 1) / pairs_per_batch);
}

TGN_API size_t tgn_reverse_lists_workspace_bytes(int b, int n, long long pairs_per_batch) {
    if (!rev_sizes_ok(b, n, pairs_per_batch)) return 0;
    return rev_workspace_bytes((long long)b * n, (long long)b * pairs_per_batch);
}

TGN_API int tgn_reverse_lists(int b, int n, long long pairs_per_batch, const void *idx, int idx_is64, int *rev_start, int *rev_pair,
                              void *ws, size_t ws_bytes, tgn_stream_t stream) {
    if (!rev_sizes_ok(b, n, pairs_per_batch)) {
        set_error("tgn_reverse_lists: b * n (%d * %d) and b * pairs_per_batch (%d * %lld) must be non-negative and below 2^31", b, n, b,
                  pairs_per_batch);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    const long long rows = (long long)b * n, pairs = (long long)b * pairs_per_batch;
    if (!rev_start || (pairs > 0 && (!idx || !rev_pair)) || (pairs > 0 && rows == 0)) {
        set_error("tgn_reverse_lists: null pointer, or pairs without a row to target");
        return TGN_ERR_INVALID_ARGUMENT;
    }
    hipStream_t st = (hipStream_t)stream;
    if (pairs == 0) {   // every segment is empty; the workspace is not used
        hipLaunchKernelGGL(rev_zero_kernel, dim3(rev_grid(rows + 1, kRevBlock)), dim3(kRevBlock), 0, st, rows + 1, rev_start);
        return check_launch("rev_zero_kernel");
    }
    if (!ws || ws_bytes < rev_workspace_bytes(rows, pairs)) {
        set_error("tgn_reverse_lists: workspace of %zu bytes, needs tgn_reverse_lists_workspace_bytes = %zu", ws_bytes,
                  rev_workspace_bytes(rows, pairs));
        return TGN_ERR_INVALID_ARGUMENT;
    }
    const long long tiles = rev_scan_tiles(rows);
    RevWorkspace w;
    w.cursor = (int *)ws;
    w.bsum = w.cursor + rows;
    w.slots = w.bsum + tiles;
    hipLaunchKernelGGL(rev_zero_kernel, dim3(rev_grid(rows, kRevBlock)), dim3(kRevBlock), 0, st, rows, w.cursor);
    int rc = dispatch_idx(idx, idx_is64, [&](auto *ip) {
        hipLaunchKernelGGL((rev_count_kernel<idx_elem_t<decltype(ip)>>), dim3(rev_grid(pairs, kRevBlock)), dim3(kRevBlock), 0, st, pairs,
                           pairs_per_batch, n, ip, w.cursor);
        return check_launch("rev_count_kernel");
    });
    if (rc != TGN_OK) return rc;
    hipLaunchKernelGGL(rev_scan_tile_kernel, dim3(rev_grid(tiles, 1)), dim3(kRevBlock), 0, st, rows, tiles, w.cursor, rev_start, w.bsum);
    hipLaunchKernelGGL(rev_scan_sums_kernel, dim3(1), dim3(kRevBlock), 0, st, tiles, w.bsum);
    hipLaunchKernelGGL(rev_scan_apply_kernel, dim3(rev_grid(rows, kRevBlock)), dim3(kRevBlock), 0, st, rows, (int)pairs, w.bsum, rev_start,
                       w.cursor);
    if ((rc = check_launch("rev_scan kernels")) != TGN_OK) return rc;
    rc = dispatch_idx(idx, idx_is64, [&](auto *ip) {
        hipLaunchKernelGGL((rev_claim_kernel<idx_elem_t<decltype(ip)>>), dim3(rev_grid(pairs, kRevBlock)), dim3(kRevBlock), 0, st, pairs,
                           pairs_per_batch, n, ip, w.cursor, w.slots);
        return check_launch("rev_claim_kernel");
    });
    if (rc != TGN_OK) return rc;
    hipLaunchKernelGGL(rev_sort_wave_kernel, dim3(rev_grid(rows, kRevBlock / kWave)), dim3(kRevBlock), 0, st, rows, rev_start, w.slots,
                       rev_pair);
    hipLaunchKernelGGL(rev_sort_long_kernel, dim3(rev_grid(rows, 1)), dim3(kRevBlock), 0, st, rows, rev_start, w.slots, rev_pair);
    return check_launch("rev_sort kernels");
}

TGN_API int tgn_scatter_ordered(long long n_rows, int c, int k, int g, const int *rev_start, const int *rev_pair, const float *src,
                                const float *coef, float sign, float *out, tgn_stream_t stream) {
    if (n_rows <= 0 || c <= 0) return TGN_OK;
    if (!src || !out || !rev_start != !rev_pair) {
        set_error("tgn_scatter_ordered: null pointer (rev_start and rev_pair come together)");
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (k < 1 || (coef && (g < 1 || c % g)) || !(sign == 1.0f || sign == -1.0f)) {
        set_error("tgn_scatter_ordered: needs k >= 1, sign +1 or -1 and, with coef, g >= 1 dividing c (k %d, g %d, c %d, sign %g)", k, g, c,
                  (double)sign);
        return TGN_ERR_INVALID_ARGUMENT;
    }
    if (!rev_start && n_rows > ((1LL << 62) / k)) {
        set_error("tgn_scatter_ordered: n_rows * k overflows");
        return TGN_ERR_INVALID_ARGUMENT;
    }
    int l = 0;
    while ((1 << l) < c && l < 6) ++l;
    const int rows_per_block = 256 >> l;
    long long blocks = (n_rows + rows_per_block - 1) / rows_per_block;
    if (blocks > 256LL * 32) blocks = 256LL * 32;
    hipStream_t st = (hipStream_t)stream;
    dispatch_bool(coef != nullptr, [&](auto query) {
        dispatch_bool(rev_start == nullptr, [&](auto ident) {
            hipLaunchKernelGGL((scatter_ordered_kernel<decltype(query)::value, decltype(ident)::value>), dim3((unsigned)blocks), dim3(256), 0,
                               st, n_rows, c, k, g, l, rev_start, rev_pair, src, coef, sign, out);
        });
    });
    return check_launch("scatter_ordered_kernel");
}
