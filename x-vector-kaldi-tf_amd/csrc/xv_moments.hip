// xv_moments.hip -- first and second moment of N vectors in fp64 on the MI355X (PLDA adaptation).
//
// What ivector-adapt-plda accumulates over the unlabelled in-domain vectors at the end of stage 8 of the recipe (run.sh):
//     sum[j] = sum_i x[i, j]        outer[j, k] = sum_i x[i, j] x[i, k]        (j, k < dim <= 256)
// The moments feed an eigenproblem, so they are fp64: the fp32 inputs are widened (exact), their products go through
// v_mfma_f64_16x16x4_f64 (a product of two fp32 values is exact in fp64) and every accumulation is fp64.  Two kernels:
//   moment_slab_kernel    rows are cut into slabs of XV_MOMENT_SLAB rows (a compile-time constant: the sum order never depends on
//                         the grid or the CU count).  A workgroup takes one slab and 16 of the 16 x 16 output tiles on or above the
//                         diagonal (4 per wave); the slab passes through LDS 32 rows at a time (fp32, next stage prefetched in
//                         registers), and each tile accumulates the slab's rows in ascending groups of 4 (one MFMA per group) into
//                         its partial in the workspace.  The workgroups of tile group 0 also add the column sums of their slab,
//                         rows ascending, one column per thread.
//   moment_reduce_kernel  one thread per output element adds the partials in slab order, writes the tile and, for a tile above
//                         the diagonal, its mirror image; of a diagonal tile only the elements on or above the diagonal are
//                         used, so outer is exactly symmetric by construction.
// No floating-point atomics; every workspace word that is read was written by the same call.  The f64 MFMA's C/D layout is its
// own: lane l, register r holds D[(l >> 4) + 4 r][l & 15]; A and B are one f64 per lane, A[l & 15][k = l >> 4], B[k = l >> 4][l & 15].
#include "xv_device.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int MS_SLAB = XV_MOMENT_SLAB;      // rows per partial
constexpr int MS_DMAX = 256;                 // dim <= 256 (16 tile rows)
constexpr int MS_NT = 256;                   // 4 waves
constexpr int MS_RC = 32;                    // rows per LDS stage (8 MFMA k-steps)
constexpr int MS_TPW = 4;                    // output tiles per wave
constexpr int MS_TPB = 4 * MS_TPW;           // output tiles per workgroup
constexpr int MS_LDW = MS_DMAX + 16;         // LDS row stride (floats): the 4 rows of a fragment read fall in 4 x 16 distinct banks
constexpr int MS_UNITS = MS_RC * (MS_DMAX / 4) / MS_NT;      // 16-byte pieces per thread and stage (8)
constexpr int MS_TILE = 256;                 // doubles per tile partial, stored [register][lane]
static_assert(MS_SLAB % MS_RC == 0 && MS_RC % 4 == 0, "a slab is whole stages, a stage whole k-steps");

// tile t of the upper triangle, row-major (tile row i holds T - i tiles): -> (i, j), i <= j
__host__ __device__ __forceinline__ void ms_tile(int t, int T, int &i, int &j)
{
    i = 0;
    while (t >= T - i) {
        t -= T - i;
        ++i;
    }
    j = i + t;
}

__global__ __launch_bounds__(MS_NT) void moment_slab_kernel(const float *__restrict__ x, long ldx, long n_rows, int dim, int ntiles,
                                                            double *__restrict__ ws, double *__restrict__ ws_sum)
{
    __shared__ f32x4 smem[MS_RC * MS_LDW / 4];
    float *Xs = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long slab = blockIdx.x;
    const int group = blockIdx.y;
    const long row0 = slab * MS_SLAB;
    const int rows = (int)min((long)MS_SLAB, n_rows - row0);
    const int T = (dim + 15) >> 4;
    const int nv = (dim + 3) >> 2;           // 16-byte pieces of a row that hold a column below dim
    const int nfull = dim >> 2;              // ... of which these lie wholly below dim

    // columns [4 nv, 16 T) of the stage are never staged: they stay zero
    for (int f = tid; f < MS_RC * MS_LDW / 4; f += MS_NT) smem[f] = f32x4{0, 0, 0, 0};

    // the wave's tiles are t0, t0 + 4, ...: the first nq of them exist (nq is wave-uniform and picks the loop's instantiation,
    // so that no MFMA sits behind a branch)
    const int t0 = group * MS_TPB + wave;
    const int nq = __builtin_amdgcn_readfirstlane(t0 < ntiles ? min(MS_TPW, (ntiles - t0 + 3) >> 2) : 0);
    int ti[MS_TPW], tj[MS_TPW];
#pragma unroll
    for (int q = 0; q < MS_TPW; ++q) ms_tile(q < nq ? t0 + 4 * q : 0, T, ti[q], tj[q]);

    f32x4 reg[MS_UNITS];
    // rows [r0, r0 + 32) of the slab, columns [0, dim): rows past the slab's end and columns past dim are zeros, and no
    // address at or past column dim is read
    auto load = [&](int r0) {
#pragma unroll
        for (int u = 0; u < MS_UNITS; ++u) {
            const int v = tid + MS_NT * u;
            const int rr = v / nv, cv = v - rr * nv;
            f32x4 val = {0, 0, 0, 0};
            if (rr < MS_RC && r0 + rr < rows) {
                const float *src = x + (row0 + r0 + rr) * ldx + 4 * cv;
                if (cv < nfull) {
                    val = *reinterpret_cast<const f32x4 *>(src);
                } else {
                    if (4 * cv + 0 < dim) val[0] = src[0];
                    if (4 * cv + 1 < dim) val[1] = src[1];
                    if (4 * cv + 2 < dim) val[2] = src[2];
                }
            }
            reg[u] = val;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int u = 0; u < MS_UNITS; ++u) {
            const int v = tid + MS_NT * u;
            const int rr = v / nv, cv = v - rr * nv;
            if (rr < MS_RC) *reinterpret_cast<f32x4 *>(Xs + rr * MS_LDW + 4 * cv) = reg[u];
        }
    };

    f64x4 acc[MS_TPW];
#pragma unroll
    for (int q = 0; q < MS_TPW; ++q) acc[q] = f64x4{0, 0, 0, 0};
    double csum = 0.0;
    const bool sums = group == 0 && tid < dim;

    // The loop is instantiated once per tile count and each wave enters the instantiation of its own nq, so the waves of a
    // workgroup may wait at different s_barrier instructions.  That is sound only because every instantiation executes the
    // same sequence of barriers (one before the loop, two per stage, the stage count depending on `rows` alone): keep every
    // __syncthreads() of this lambda independent of NQ.
    auto run = [&](auto nq_c) {
        constexpr int NQ = decltype(nq_c)::value;
        load(0);
        __syncthreads();
        for (int r0 = 0; r0 < rows; r0 += MS_RC) {
            store();
            __syncthreads();
            if (r0 + MS_RC < rows) load(r0 + MS_RC);
            const int nks = (min(MS_RC, rows - r0) + 3) >> 2;
            const float *p = Xs + (lane >> 4) * MS_LDW + (lane & 15);
            for (int ks = 0; ks < nks; ++ks, p += 4 * MS_LDW) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const double a = (double)p[16 * ti[q]];
                    const double b = (double)p[16 * tj[q]];
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
                }
            }
            if (sums) {
#pragma unroll 8
                for (int rr = 0; rr < MS_RC; ++rr) csum += (double)Xs[rr * MS_LDW + tid];
            }
            __syncthreads();
        }
    };
    switch (nq) {
    case 4: run(std::integral_constant<int, 4>{}); break;
    case 3: run(std::integral_constant<int, 3>{}); break;
    case 2: run(std::integral_constant<int, 2>{}); break;
    case 1: run(std::integral_constant<int, 1>{}); break;
    default: run(std::integral_constant<int, 0>{}); break;
    }
    static_assert(MS_TPW == 4, "one instantiation of the loop per tile count of a wave");

#pragma unroll
    for (int q = 0; q < MS_TPW; ++q)
        if (q < nq) {
            double *o = ws + (slab * ntiles + (t0 + 4 * q)) * MS_TILE + lane;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[64 * r] = acc[q][r];
        }
    if (sums) ws_sum[slab * MS_DMAX + tid] = csum;
}

// block b < ntiles: tile b of outer; block ntiles: sum.  The partials are added in slab order, one chain per element.
__global__ __launch_bounds__(MS_NT) void moment_reduce_kernel(const double *__restrict__ ws, const double *__restrict__ ws_sum, long nslab,
                                                              int dim, int ntiles, double *__restrict__ sum, double *__restrict__ outer,
                                                              long ldo)
{
    const int tid = threadIdx.x, b = blockIdx.x;
    const bool tile = b < ntiles;
    if (!tile && tid >= dim) return;
    const double *p = tile ? ws + (long)b * MS_TILE + tid : ws_sum + tid;
    const long stride = tile ? (long)ntiles * MS_TILE : MS_DMAX;
    double a = 0.0;
    long s = 0;
    for (; s + 8 <= nslab; s += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(s + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (; s < nslab; ++s) a += p[s * stride];
    if (!tile) {
        sum[tid] = a;
        return;
    }
    int i, j;
    ms_tile(b, (dim + 15) >> 4, i, j);
    const int lane = tid & 63, r = tid >> 6;
    const int row = 16 * i + (lane >> 4) + 4 * r, col = 16 * j + (lane & 15);
    if (row >= dim || col >= dim || row > col) return;          // row > col: the lower half of a diagonal tile
    outer[row * ldo + col] = a;
    if (row != col) outer[col * ldo + row] = a;
}

long ms_ntiles(int dim)
{
    const long T = (dim + 15) >> 4;
    return T * (T + 1) / 2;
}

}  // namespace

extern "C" size_t xv_moment_stats_workspace_bytes(int64_t n_rows, int dim)
{
    if (n_rows < 1 || dim < 1 || dim > MS_DMAX) return 0;
    const size_t nslab = ((size_t)n_rows + MS_SLAB - 1) / MS_SLAB;
    return nslab * ((size_t)ms_ntiles(dim) * MS_TILE + MS_DMAX) * sizeof(double);
}

extern "C" int xv_moment_stats_f64(const float *x, int64_t ldx, int64_t n_rows, int dim, double *sum, double *outer, int64_t ld_outer,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    if (dim < 1 || dim > MS_DMAX) return fail(XV_ERR_UNSUPPORTED, "moment_stats: 1 <= dim <= 256 only");
    if (!x || !sum || !outer || n_rows < 1 || ldx < dim || ld_outer < dim)
        return fail(XV_ERR_BAD_ARG, "moment_stats: bad argument (n_rows >= 1, ldx >= dim, ld_outer >= dim, no NULL pointer)");
    if (ldx % 4 || ((uintptr_t)x & 15) || (((uintptr_t)sum | (uintptr_t)outer) & 7))
        return fail(XV_ERR_BAD_ARG, "moment_stats: x must be 16-byte aligned with ldx a multiple of 4, sum and outer 8-byte aligned");
    const long nslab = (n_rows + MS_SLAB - 1) / MS_SLAB;
    if (nslab > 0x7fffffffL) return fail(XV_ERR_UNSUPPORTED, "moment_stats: too many rows for one launch");
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < xv_moment_stats_workspace_bytes(n_rows, dim))
        return fail(XV_ERR_BAD_ARG, "moment_stats: the workspace is missing, misaligned or smaller than xv_moment_stats_workspace_bytes");
    const int ntiles = (int)ms_ntiles(dim);
    double *ws = static_cast<double *>(workspace);
    double *ws_sum = ws + nslab * ntiles * MS_TILE;
    hipLaunchKernelGGL(moment_slab_kernel, dim3((unsigned)nslab, (ntiles + MS_TPB - 1) / MS_TPB), dim3(MS_NT), 0, (hipStream_t)stream, x,
                       (long)ldx, (long)n_rows, dim, ntiles, ws, ws_sum);
    if (const int rc = launch_status("moment_slab_kernel")) return rc;
    hipLaunchKernelGGL(moment_reduce_kernel, dim3(ntiles + 1), dim3(MS_NT), 0, (hipStream_t)stream, ws, ws_sum, nslab, dim, ntiles, sum,
                       outer, (long)ld_outer);
    return launch_status("moment_reduce_kernel");
}
