// grid_common.h -- the per-cloud uniform grid shared by the ball query (ball_query.hip) and the grid kNN (neighbors.hip).
//
// Both builders run one workgroup per cloud and the same steps: bounding box and bad-coordinate census -> cell size grown
// until the grid fits the LDS histogram -> histogram with LDS atomics -> exclusive scan -> cursor scatter of records sorted
// by cell.  What differs stays in the kernels: the first cell-size guess, the coordinate threshold, the record layout and
// the ball side's LDS-permutation scatter.
#pragma once
#include "tgn_common.h"

namespace tgn {

constexpr int kGridCells = 16384;    // cells per cloud (LDS histogram: 64 KiB)
constexpr int kGridThreads = 1024;   // threads of a build workgroup

struct GridHeader {   // one per cloud, 64 bytes
    float lo[3];
    float inv_h;
    int g[3];
    int use_scan;     // 1: this cloud's queries scan it linearly (bad coordinates, degenerate or tiny grid)
    float h;          // cell size
    int pad[7];
};
static_assert(sizeof(GridHeader) == 64, "the workspace layouts of both users count on 64 bytes");

// the __shfl_xor butterfly: result in every lane
__device__ __forceinline__ float wave_min_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// Cell coordinate on one axis: the same expression for points and queries.  Two clamps, on purpose.  The ball grid only
// visits the 3x3x3 cells around a query, so a query outside the box must keep a coordinate that says so: it clamps to
// [-1, g] and floors, and a far query simply finds no cell.  The kNN grid widens its block until the k-th neighbour is
// covered, so an outside query is sent to the border cell (NaN -> 0) and the query kernel corrects the covered radius
// with its `outside` distance.
__device__ __forceinline__ int cell_coord(float p, float lo, float inv_h, int g) {
    float t = (p - lo) * inv_h;
    t = fminf(fmaxf(t, -1.0f), (float)g);
    return (int)floorf(t);
}
__device__ __forceinline__ int knn_cell(float p, float lo, float inv_h, int g) {
    float t = (p - lo) * inv_h;
    t = fminf(fmaxf(t, 0.0f), (float)(g - 1));
    return (int)t;
}
// linear cell index of a point of the cloud (x fastest), COORD = cell_coord or knn_cell
template <int (*COORD)(float, float, float, int)>
__device__ __forceinline__ int grid_cell_of(const GridHeader &h, float px, float py, float pz) {
    const int cx = COORD(px, h.lo[0], h.inv_h, h.g[0]);
    const int cy = COORD(py, h.lo[1], h.inv_h, h.g[1]);
    const int cz = COORD(pz, h.lo[2], h.inv_h, h.g[2]);
    return (cz * h.g[1] + cy) * h.g[0] + cx;
}

// Bounding box and bad-coordinate census of a cloud, first half (every thread of the block): the thread's points, the wave
// reductions, one partial per wave into red[0..2] (min), red[3..5] (max), red[6] (bad).  A coordinate is bad unless
// |v| <= bad_above (NaN is bad).  The caller's __syncthreads() goes between the two halves.
template <int NT>
__device__ __forceinline__ void grid_box_partials(const float *__restrict__ pts, int n, float bad_above, float (&red)[7][NT / kWave]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    float bad = 0.0f;
    for (int i = tid; i < n; i += NT) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[(size_t)i * 3 + a];
            if (!(fabsf(v) <= bad_above)) bad = 1.0f;
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = wave_min_f32(lo[a]), h = wave_max_f32(hi[a]);
        if (lane == 0) {
            red[a][wave] = l;
            red[3 + a][wave] = h;
        }
    }
    {
        const float bb = wave_max_f32(bad);
        if (lane == 0) red[6][wave] = bb;
    }
}
// Second half (one thread): the box, its extents, and whether any coordinate was bad (> 0).
template <int NW>
__device__ __forceinline__ float grid_box_collect(const float (&red)[7][NW], float (&lo)[3], float (&hi)[3], float (&ext)[3]) {
    float any_bad = 0.0f;
    for (int a = 0; a < 3; ++a) {
        float l = INFINITY, u = -INFINITY;
        for (int w = 0; w < NW; ++w) {
            l = fminf(l, red[a][w]);
            u = fmaxf(u, red[3 + a][w]);
        }
        lo[a] = l;
        hi[a] = u;
        ext[a] = u - l;
    }
    for (int w = 0; w < NW; ++w) any_bad = fmaxf(any_bad, red[6][w]);
    return any_bad;
}

// Fit the grid: g[a] = floor(ext[a] / hcell) + 1 cells per axis, hcell grown by 1.1 for at most max_iter rounds until the
// grid has at most kGridCells cells.  Returns the cell count (still larger if the rounds ran out).
__device__ __forceinline__ long long grid_fit(const float (&ext)[3], float &hcell, int max_iter, int (&g)[3]) {
    for (int it = 0; it < max_iter; ++it) {
        const float inv = 1.0f / hcell;
        long long cells = 1;
        for (int a = 0; a < 3; ++a) {
            const float t = ext[a] * inv;   // same expression as the cell coordinate of the box's upper corner: (int)t = g - 1
            g[a] = (t < 1.0e6f) ? (int)t + 1 : 1000001;
            cells *= g[a];
        }
        if (cells <= kGridCells) break;
        hcell *= 1.1f;
    }
    return (long long)g[0] * g[1] * g[2];
}

// Exclusive scan of the histogram cnt[0..CELLS) by the NT threads of the block: CELLS / NT cells per thread, wave scan,
// block scan through wave_tot.  Writes cell_start[0..CELLS] and leaves the running insert positions in cnt.  Between two
// barriers: call it after the __syncthreads() that ends the histogram; the scatter may follow at once.
template <int CELLS, int NT>
__device__ __forceinline__ void grid_scan_cells(int *cnt, int (&wave_tot)[NT / kWave], int *__restrict__ cell_start) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int PER = CELLS / NT;
    int local[PER];
    int sum = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        local[i] = sum;
        sum += cnt[tid * PER + i];
    }
    int incl = sum;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == kWave - 1) wave_tot[wave] = incl;
    __syncthreads();
    int wave_base = 0;
    for (int w = 0; w < wave; ++w) wave_base += wave_tot[w];
    const int thread_base = wave_base + incl - sum;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int v = thread_base + local[i];
        cell_start[tid * PER + i] = v;
        cnt[tid * PER + i] = v;
    }
    if (tid == NT - 1) cell_start[CELLS] = thread_base + sum;
    __syncthreads();
}

}  // namespace tgn
