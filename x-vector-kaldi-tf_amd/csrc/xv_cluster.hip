// xv_cluster.hip -- average-linkage agglomerative clustering of an n x n score matrix on the MI355X.
//
// Clustering-based PLDA adaptation clusters the unlabelled in-domain vectors by their PLDA scores; the matrix is already on the
// device (xv_score_matrix_f32) and is the part that scales with the data.  The semantics are fixed bit for bit in
// include/xvector_hip.h: T[c, e] is the fp64 sum of the scores between the members of clusters c and e, avg = T / (size size),
// the largest avg merges first, ties go to the lexicographically smallest (c, e).
//
// State (the workspace): T as a full symmetric n x n fp64 matrix (row c is read and written contiguously; the mirror cell
// T[k, c] is the one strided write per live k), and O(n) bookkeeping: size[n] (0 = dead), parent[n] (the slot a dead slot merged
// into), and per row k its cached best partner best_j[k] > k with best_avg[k] = avg(k, best_j[k]) (-1: no live partner).
// The avg values are pure functions of T and the sizes, so the cache cannot change the answer; it only saves the n^2 rescan.
//
// Launches, all in stream order, no host synchronisation:
//   ahc_init_kernel      T from the strict upper triangle of scores, 32 x 32 tiles, the mirror through LDS
//   ahc_rows_kernel      one workgroup per row: its best partner; the bookkeeping, labels[i] = i, *n_merges = 0
//   ahc_merge_kernel     ONE workgroup of 1024 threads runs up to AHC_STEPS merges; ceil((n - min_clusters) / AHC_STEPS) launches
//                        are chained, and a "done" word in the workspace turns the launches after the stop into immediate exits.
//                        The merges are sequential by nature and a single workgroup needs no barrier wider than s_barrier: no
//                        workgroup ever waits on another.
//   ahc_labels_kernel    labels[i] = the live slot at the end of i's parent chain (parents only decrease)
// One merge inside the workgroup: (1) argmax of best_avg over the rows, (2) the stop test, (3) every live k adds row e into row c
// and column c, compares the one updated cell of a row k < c against its cached best (same tie rule) or queues the row for a
// rescan when its partner was c or e; the same pass collects row c's own new best, (4) the queued rows are rescanned.
// The merge itself is one device function (ahc_merge_step) over the state pointers.  ahc_batch_kernel (xv_ahc_average_batch_f64,
// DESIGN.md §8.15) runs it for G independent small problems, one workgroup of 256 threads per problem, with the problem's init, row
// caches and labels in the same workgroup: one launch, every problem resident at once.
// No floating-point atomics; fp64 + and / are plain C++ (this unit is not built with fast-math, and it has no a * b + c to contract).
#include "xv_device.h"

#include <cmath>

namespace {

constexpr int AHC_NT = 1024;                 // threads of the merge workgroup (16 waves)
constexpr int AHC_STEPS = 256;               // merges per launch of ahc_merge_kernel
constexpr int AHC_U = 8;                     // slots per thread whose loads are issued together (latency, not bandwidth, bounds a merge)
constexpr int AHC_TILE = 32;
constexpr int AHC_ROW_NT = 256;
constexpr int AHC_HDR = 16;                  // header words: [0] live clusters, [1] merges so far, [2] done
constexpr int AHC_BATCH_NT = 256;            // threads of a group's workgroup in ahc_batch_kernel (4 waves: at n of a few hundred more
                                             // threads only pay for wider barriers)
constexpr int AHC_BATCH_U = 2;               // its slots per thread in flight: one pass covers 512 slots

__host__ __device__ inline size_t ahc_bookkeeping_bytes(size_t n)
{
    return n * sizeof(double) + 4 * n * sizeof(int) + AHC_HDR * sizeof(int);       // best_avg | best_j, size, parent, queue | header
}

struct Cand {
    double v;
    int i;                                   // < 0: empty
};

// a before b: the larger value, ties to the smaller index; an empty candidate never wins
__device__ __forceinline__ bool better(const Cand &a, const Cand &b)
{
    return a.i >= 0 && (b.i < 0 || a.v > b.v || (a.v == b.v && a.i < b.i));
}

__device__ __forceinline__ double avg_of(double t, int sa, int sb)
{
    return t / (double)((long long)sa * (long long)sb);
}

__device__ __forceinline__ Cand wave_best(Cand c, int width)
{
    for (int off = width >> 1; off > 0; off >>= 1) {
        Cand o;
        o.v = __shfl_down(c.v, off, 64);
        o.i = __shfl_down(c.i, off, 64);
        if (better(o, c)) c = o;
    }
    return c;
}

// the best candidate of the workgroup, returned to every thread.  slots: NW + 1 entries of LDS; two barriers, and the barrier a
// caller needs before its next write to memory that others read here is its own business
template <int NW>
__device__ __forceinline__ Cand block_best(Cand c, Cand *slots)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    c = wave_best(c, 64);
    if (lane == 0) slots[wave] = c;
    __syncthreads();
    if (wave == 0) {
        Cand d = lane < NW ? slots[lane] : Cand{0.0, -1};
        d = wave_best(d, 64);
        if (lane == 0) slots[NW] = d;
    }
    __syncthreads();
    return slots[NW];
}

// T[i, j] = T[j, i] = (double)scores[i * ld + j] for i < j.  Grid: the tiles (bi <= bj); only cells with i < j are read.
__global__ __launch_bounds__(AHC_TILE * 8) void ahc_init_kernel(const float *__restrict__ scores, long ld, int n, int tiles,
                                                                 double *__restrict__ T)
{
    __shared__ double sm[AHC_TILE][AHC_TILE + 1];
    // tile index -> (bi, bj), bi <= bj, row-major over the upper triangle of the tile grid
    int t = blockIdx.x, bi = 0;
    while (t >= tiles - bi) {
        t -= tiles - bi;
        ++bi;
    }
    const int bj = bi + t;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < AHC_TILE; r += 8) {
        const int i = bi * AHC_TILE + r, j = bj * AHC_TILE + tx;
        double v = 0.0;
        if (i < n && j < n && i < j) {
            v = (double)scores[(long)i * ld + j];
            T[(long)i * n + j] = v;
        }
        sm[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < AHC_TILE; r += 8) {
        const int j = bj * AHC_TILE + r, i = bi * AHC_TILE + tx;          // the mirror cell T[j, i], i < j
        if (i < n && j < n && i < j) T[(long)j * n + i] = sm[tx][r];
    }
}

// row k's best partner among j > k (every slot is live with size 1), and the bookkeeping of slot k
__global__ __launch_bounds__(AHC_ROW_NT) void ahc_rows_kernel(const double *__restrict__ T, int n, int min_clusters, double *best_avg,
                                                              int *best_j, int *size, int *parent, int *hdr, int32_t *labels,
                                                              int32_t *n_merges)
{
    __shared__ Cand slots[AHC_ROW_NT / 64 + 1];
    const int k = blockIdx.x;
    const double *row = T + (long)k * n;
    Cand c = {0.0, -1};
    for (int j = k + 1 + threadIdx.x; j < n; j += AHC_ROW_NT) {
        const Cand o = {avg_of(row[j], 1, 1), j};
        if (better(o, c)) c = o;
    }
    c = block_best<AHC_ROW_NT / 64>(c, slots);
    if (threadIdx.x == 0) {
        best_avg[k] = c.v;
        best_j[k] = c.i;
        size[k] = 1;
        parent[k] = k;
        labels[k] = k;
        if (k == 0) {
            hdr[0] = n;
            hdr[1] = 0;
            hdr[2] = n <= min_clusters ? 1 : 0;
            *n_merges = 0;
        }
    }
}

// One merge over the state pointers, by a workgroup of NT threads (U slots per thread in flight): the one place the merge
// lives, for ahc_merge_kernel and ahc_batch_kernel.  (1) argmax of best_avg over the rows, (2) the stop test, (3) row c += row e
// with the mirror column and the caches, (4) the rescans.  Returns false, with nothing written, when the stop rule holds; else
// records merge number `merges` and returns true after its closing barrier.  Every thread returns the same value.  The integer
// and fp64 results do not depend on NT or U: candidates are compared under one total order and every T cell has one writer.
template <int NT, int U>
__device__ __forceinline__ bool ahc_merge_step(double *T, int n, double threshold, int clusters, int min_clusters, double *best_avg,
                                               int *best_j, int *size, int *parent, int *queue, Cand *slots, int *queued,
                                               int32_t *merge_a, int32_t *merge_b, double *merge_score, int merges)
{
    const int tid = threadIdx.x;
    // (1) the best pair: the rows' cached bests, ties to the smaller row (its cached partner is its smallest)
    Cand g = {0.0, -1};
    for (int k0 = tid; k0 < n; k0 += NT * U) {
        int bj[U];
        double bv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + u * NT;
            bj[u] = k < n ? best_j[k] : -1;
            bv[u] = k < n ? best_avg[k] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const Cand o = {bv[u], bj[u] >= 0 ? k0 + u * NT : -1};
            if (better(o, g)) g = o;
        }
    }
    if (tid == 0) *queued = 0;
    g = block_best<NT / 64>(g, slots);
    // (2) stop?  (uniform: every thread holds the same g)
    if (clusters == min_clusters || g.i < 0 || !(g.v >= threshold)) return false;
    const int c = g.i, e = best_j[c];
    const int sc = size[c], se = size[e], snew = sc + se;
    if (tid == 0) {
        merge_a[merges] = c;
        merge_b[merges] = e;
        merge_score[merges] = g.v;
    }
    // (3) row c += row e, the mirror column, the caches of the rows above c, row c's own best
    double *Tc = T + (long)c * n;
    const double *Te = T + (long)e * n;
    Cand rc = {0.0, -1};
    for (int k0 = tid; k0 < n; k0 += NT * U) {
        // every load of the batch first (dead slots too: in bounds, unused), so that they are in flight together
        int sk[U], bj[U];
        double tc[U], te[U], bv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + u * NT;
            const bool in = k < n;
            sk[u] = in ? size[k] : 0;
            tc[u] = in ? Tc[k] : 0.0;
            te[u] = in ? Te[k] : 0.0;
            bj[u] = in ? best_j[k] : -1;
            bv[u] = in && k < c ? best_avg[k] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = k0 + u * NT;
            if (sk[u] == 0 || k == c || k == e) continue;
            const double t = tc[u] + te[u];
            Tc[k] = t;
            T[(long)k * n + c] = t;
            if (k > c) {
                const Cand o = {avg_of(t, snew, sk[u]), k};
                if (better(o, rc)) rc = o;
                if (k < e && bj[u] == e) queue[atomicAdd(queued, 1)] = k;
            } else if (bj[u] == c || bj[u] == e) {
                queue[atomicAdd(queued, 1)] = k;
            } else {
                const Cand o = {avg_of(t, sk[u], snew), c}, cur = {bv[u], bj[u]};
                if (better(o, cur)) {
                    best_avg[k] = o.v;
                    best_j[k] = c;
                }
            }
        }
    }
    rc = block_best<NT / 64>(rc, slots);                     // its first barrier also orders the writes above before what follows
    if (tid == 0) {
        best_avg[c] = rc.v;
        best_j[c] = rc.i;
        best_j[e] = -1;
        size[c] = snew;
        size[e] = 0;
        parent[e] = c;
    }
    __syncthreads();
    // (4) the rows whose partner was c or e: a full rescan each, the whole workgroup on one row at a time
    const int nq = *queued;
    for (int q = 0; q < nq; ++q) {
        const int k = queue[q];
        const int sk = size[k];
        const double *row = T + (long)k * n;
        Cand b = {0.0, -1};
        for (int j0 = k + 1 + tid; j0 < n; j0 += NT * U) {
            int sj[U];
            double tv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + u * NT;
                sj[u] = j < n ? size[j] : 0;
                tv[u] = j < n ? row[j] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (sj[u] == 0) continue;
                const Cand o = {avg_of(tv[u], sk, sj[u]), j0 + u * NT};
                if (better(o, b)) b = o;
            }
        }
        b = block_best<NT / 64>(b, slots);
        if (tid == 0) {
            best_avg[k] = b.v;
            best_j[k] = b.i;
        }
    }
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(AHC_NT) void ahc_merge_kernel(double *__restrict__ T, int n, double threshold, int min_clusters,
                                                           double *best_avg, int *best_j, int *size, int *parent, int *queue, int *hdr,
                                                           int32_t *merge_a, int32_t *merge_b, double *merge_score, int32_t *n_merges)
{
    __shared__ Cand slots[AHC_NT / 64 + 1];
    __shared__ int queued;
    const int tid = threadIdx.x;
    if (hdr[2]) return;                                      // a launch after the stop
    int clusters = hdr[0], merges = hdr[1];
    bool done = false;
    for (int step = 0; step < AHC_STEPS; ++step) {
        if (!ahc_merge_step<AHC_NT, AHC_U>(T, n, threshold, clusters, min_clusters, best_avg, best_j, size, parent, queue, slots, &queued,
                                           merge_a, merge_b, merge_score, merges)) {
            done = true;
            break;
        }
        --clusters;
        ++merges;
    }
    if (tid == 0) {
        hdr[0] = clusters;
        hdr[1] = merges;
        if (done || clusters == min_clusters) hdr[2] = 1;
        *n_merges = merges;
    }
}

// G independent problems, one workgroup each (xv_ahc_average_batch_f64): init, first row caches, merges and labels of group
// blockIdx.x all run here, between s_barriers; no workgroup waits on another.  A group that breaks its contract is skipped whole
// and *status = 1 (every test is uniform over the workgroup).  The state is laid out as xv_ahc_average_f64 lays it out, in the
// group's slice of the workspace; all of it that is read is written here first.
struct AhcBatchParams {
    const float *scores; long scores_elems;
    const int32_t *grp_row0; const int64_t *grp_score0, *grp_ws0;
    const double *threshold; const int32_t *min_clusters;
    int max_n, n_rows;
    int32_t *merge_a, *merge_b; double *merge_score; int32_t *n_merges, *labels, *status;
    char *workspace; size_t workspace_bytes;
};

__global__ __launch_bounds__(AHC_BATCH_NT) void ahc_batch_kernel(const AhcBatchParams p)
{
    __shared__ Cand slots[AHC_BATCH_NT / 64 + 1];
    __shared__ int queued;
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = p.grp_row0[g], nl = (long)p.grp_row0[g + 1] - row0;
    const long off = p.grp_score0[g], ld = (nl + 3) & ~3L, ws0 = p.grp_ws0[g];
    const double threshold = p.threshold[g];
    const int min_clusters = p.min_clusters[g];
    bool ok = nl >= 1 && nl <= p.max_n && row0 >= 0 && row0 + nl <= p.n_rows && off >= 0 && !(off & 3) && off <= p.scores_elems &&
              nl * ld <= p.scores_elems - off && min_clusters >= 1 && min_clusters <= nl && threshold == threshold;
    if (ok) {
        const size_t need = (size_t)nl * (size_t)nl * sizeof(double) + ahc_bookkeeping_bytes((size_t)nl);
        ok = ws0 >= 0 && !(ws0 & 7) && (size_t)ws0 <= p.workspace_bytes && need <= p.workspace_bytes - (size_t)ws0;
    }
    if (!ok) {
        if (tid == 0) *p.status = 1;
        return;
    }
    const int n = (int)nl;
    const float *scores = p.scores + off;
    double *T = reinterpret_cast<double *>(p.workspace + ws0);
    double *best_avg = T + (size_t)n * (size_t)n;
    int *best_j = reinterpret_cast<int *>(best_avg + n);
    int *size = best_j + n, *parent = size + n, *queue = parent + n;
    // T[i, j] = T[j, i] = (double)scores[i * ld + j] for i < j (the diagonal: 0, never used), written row by row
    for (long f = tid; f < (long)n * n; f += AHC_BATCH_NT) {
        const int i = (int)(f / n), j = (int)(f % n);
        T[f] = i == j ? 0.0 : (double)scores[i < j ? i * ld + j : j * ld + i];
    }
    __syncthreads();
    // row k's best partner among j > k (every slot is live with size 1) and the bookkeeping of slot k: one wave per row
    for (int k = wave; k < n; k += AHC_BATCH_NT / 64) {
        const double *row = T + (long)k * n;
        Cand c = {0.0, -1};
        for (int j = k + 1 + lane; j < n; j += 64) {
            const Cand o = {avg_of(row[j], 1, 1), j};
            if (better(o, c)) c = o;
        }
        c = wave_best(c, 64);
        if (lane == 0) {
            best_avg[k] = c.v;
            best_j[k] = c.i;
            size[k] = 1;
            parent[k] = k;
        }
    }
    __syncthreads();
    int32_t *merge_a = p.merge_a + row0, *merge_b = p.merge_b + row0;
    double *merge_score = p.merge_score + row0;
    int merges = 0;
    for (int m = 0; m < n - min_clusters; ++m) {             // bounded by construction, whatever the scores hold
        if (!ahc_merge_step<AHC_BATCH_NT, AHC_BATCH_U>(T, n, threshold, n - merges, min_clusters, best_avg, best_j, size, parent, queue,
                                                       slots, &queued, merge_a, merge_b, merge_score, merges))
            break;
        ++merges;
    }
    if (tid == 0) p.n_merges[g] = merges;
    // labels[i] = the live slot at the end of i's parent chain (parents only decrease); the last barrier ordered parent[]
    for (int i = tid; i < n; i += AHC_BATCH_NT) {
        int r = i;
        for (int q = parent[r]; q != r; q = parent[r]) r = q;
        p.labels[row0 + i] = r;
    }
}

__global__ void ahc_labels_kernel(const int *__restrict__ parent, int n, int32_t *__restrict__ labels)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int r = i;
    for (int p = parent[r]; p != r; p = parent[r]) r = p;    // parent[e] = c < e: the chain only descends and ends at a live slot
    labels[i] = r;
}

}  // namespace

extern "C" size_t xv_ahc_average_workspace_bytes(int n)
{
    if (n < 1 || n > XV_AHC_MAX_N) return 0;
    return (size_t)n * (size_t)n * sizeof(double) + ahc_bookkeeping_bytes((size_t)n);
}

extern "C" int xv_ahc_average_f64(const float *scores, int64_t ld, int n, double threshold, int min_clusters, int32_t *merge_a,
                                  int32_t *merge_b, double *merge_score, int32_t *n_merges, int32_t *labels, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    if (n < 1) return fail(XV_ERR_BAD_ARG, "ahc_average: n must be at least 1");
    if (n > XV_AHC_MAX_N) return fail(XV_ERR_UNSUPPORTED, "ahc_average: n exceeds XV_AHC_MAX_N (32768)");
    if (!scores || !merge_a || !merge_b || !merge_score || !n_merges || !labels)
        return fail(XV_ERR_BAD_ARG, "ahc_average: NULL pointer");
    if (ld < n || ld % 4 || ((uintptr_t)scores & 15))
        return fail(XV_ERR_BAD_ARG, "ahc_average: ld must be >= n and a multiple of 4, scores 16-byte aligned");
    if (((uintptr_t)merge_a | (uintptr_t)merge_b | (uintptr_t)n_merges | (uintptr_t)labels) & 3 || ((uintptr_t)merge_score & 7))
        return fail(XV_ERR_BAD_ARG, "ahc_average: misaligned output");
    if (min_clusters < 1 || min_clusters > n) return fail(XV_ERR_BAD_ARG, "ahc_average: min_clusters must be in [1, n]");
    if (std::isnan(threshold)) return fail(XV_ERR_BAD_ARG, "ahc_average: the threshold is NaN");
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < xv_ahc_average_workspace_bytes(n))
        return fail(XV_ERR_BAD_ARG, "ahc_average: the workspace is missing, misaligned or smaller than xv_ahc_average_workspace_bytes");
    hipStream_t st = (hipStream_t)stream;
    double *T = static_cast<double *>(workspace);
    double *best_avg = T + (size_t)n * (size_t)n;
    int *best_j = reinterpret_cast<int *>(best_avg + n);
    int *size = best_j + n, *parent = size + n, *queue = parent + n, *hdr = queue + n;
    const int tiles = (n + AHC_TILE - 1) / AHC_TILE;
    hipLaunchKernelGGL(ahc_init_kernel, dim3((unsigned)(tiles * (tiles + 1) / 2)), dim3(AHC_TILE * 8), 0, st, scores, (long)ld, n, tiles, T);
    if (const int rc = launch_status("ahc_init_kernel")) return rc;
    hipLaunchKernelGGL(ahc_rows_kernel, dim3((unsigned)n), dim3(AHC_ROW_NT), 0, st, T, n, min_clusters, best_avg, best_j, size, parent, hdr,
                       labels, n_merges);
    if (const int rc = launch_status("ahc_rows_kernel")) return rc;
    const int launches = (n - min_clusters + AHC_STEPS - 1) / AHC_STEPS;
    for (int l = 0; l < launches; ++l) {
        hipLaunchKernelGGL(ahc_merge_kernel, dim3(1), dim3(AHC_NT), 0, st, T, n, threshold, min_clusters, best_avg, best_j, size, parent,
                           queue, hdr, merge_a, merge_b, merge_score, n_merges);
        if (const int rc = launch_status("ahc_merge_kernel")) return rc;
    }
    if (launches) {
        hipLaunchKernelGGL(ahc_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, parent, n, labels);
        return launch_status("ahc_labels_kernel");
    }
    return 0;
}

extern "C" size_t xv_ahc_average_batch_workspace_bytes(int n)
{
    if (n < 1 || n > XV_AHC_BATCH_MAX_N) return 0;
    return (size_t)n * (size_t)n * sizeof(double) + ahc_bookkeeping_bytes((size_t)n);
}

extern "C" int xv_ahc_average_batch_f64(const float *scores, int64_t scores_elems, const int32_t *grp_row0, const int64_t *grp_score0,
                                        const int64_t *grp_ws0, const double *threshold, const int32_t *min_clusters, int n_groups,
                                        int max_n, int n_rows, int32_t *merge_a, int32_t *merge_b, double *merge_score,
                                        int32_t *n_merges, int32_t *labels, int32_t *status, void *workspace, size_t workspace_bytes,
                                        void *stream)
{
    if (n_groups < 1 || max_n < 1 || n_rows < 1 || scores_elems < 1)
        return fail(XV_ERR_BAD_ARG, "ahc_average_batch: n_groups, max_n, n_rows and scores_elems must be at least 1");
    if (max_n > XV_AHC_BATCH_MAX_N) return fail(XV_ERR_UNSUPPORTED, "ahc_average_batch: max_n exceeds XV_AHC_BATCH_MAX_N (4096)");
    if (!scores || !grp_row0 || !grp_score0 || !grp_ws0 || !threshold || !min_clusters || !merge_a || !merge_b || !merge_score ||
        !n_merges || !labels || !status)
        return fail(XV_ERR_BAD_ARG, "ahc_average_batch: NULL pointer");
    if (((uintptr_t)scores & 15) || (((uintptr_t)grp_row0 | (uintptr_t)min_clusters | (uintptr_t)merge_a | (uintptr_t)merge_b |
                                      (uintptr_t)n_merges | (uintptr_t)labels | (uintptr_t)status) & 3) ||
        (((uintptr_t)grp_score0 | (uintptr_t)grp_ws0 | (uintptr_t)threshold | (uintptr_t)merge_score) & 7))
        return fail(XV_ERR_BAD_ARG, "ahc_average_batch: misaligned pointer (scores 16 bytes, 64-bit tables 8, the rest 4)");
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes == 0)
        return fail(XV_ERR_BAD_ARG, "ahc_average_batch: the workspace is missing, misaligned or empty");
    const AhcBatchParams p{scores, (long)scores_elems, grp_row0, grp_score0, grp_ws0, threshold, min_clusters, max_n, n_rows,
                           merge_a, merge_b, merge_score, n_merges, labels, status, static_cast<char *>(workspace), workspace_bytes};
    hipLaunchKernelGGL(ahc_batch_kernel, dim3((unsigned)n_groups), dim3(AHC_BATCH_NT), 0, (hipStream_t)stream, p);
    return launch_status("ahc_batch_kernel");
}
