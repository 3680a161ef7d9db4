// xv_pool.hip -- statistics pooling and the chunk average (gfx950).
//   stats_pool_kernel         HBM-bound mean/std reduction: one wave64 per (chunk, split, 64 channels),
//                             16 B/lane loads, blocked two-pass + Chan merges, wave shuffle combine
//   stats_pool_merge_kernel   the splits of a long chunk
//   stats_pool_blocks_kernel  the per-8-row block statistics that the POOL epilogues of the GEMM families write
//                             (layout [ceil(R/8)][2][Cout]: include/xvector_hip.h) merged per chunk
//   chunk_average_kernel      an utterance's x-vector from its chunks' embeddings, in NumPy's float32 operation order
#include "xv_device.h"

namespace {

struct Stat4 {
    f32x4 mean, m2;
    float n;
};

// merge a block of `m` values per channel given as (block mean, block M2) into the running stats
__device__ __forceinline__ void chan_merge(Stat4 &s, const f32x4 bmean, const f32x4 bm2, float m)
{
    const float nn = s.n + m;
    if (nn > 0.f) {
        const float w = m / nn;
        const f32x4 d = bmean - s.mean;
        s.mean += d * w;
        s.m2 += bm2 + d * d * (s.n * w);
        s.n = nn;
    }
}

constexpr int POOL_UNROLL = 8;

// One wave64 per (chunk b, time split sp, 64-channel group).  lane = (phase = lane>>4 : which of 4
// interleaved rows, cg = lane&15 : which float4 of the 64 channels).  A wave instruction therefore
// reads 4 rows x 256 contiguous bytes; a 4-wave workgroup covers a 256-channel slab.
__global__ __launch_bounds__(256) void stats_pool_kernel(const float *__restrict__ h, long ldh, int C,
                                                         const int *__restrict__ row_start,
                                                         const int *__restrict__ row_len, int split_rows,
                                                         int max_splits, float eps, float *__restrict__ out,
                                                         float *__restrict__ partial, int raw)
{
    const int b = blockIdx.z, sp = blockIdx.y;
    const int len = row_len[b];
    const int begin = sp * split_rows;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int phase = lane >> 4;
    const int c = (blockIdx.x * 4 + wave) * 64 + (lane & 15) * 4;
    if (c >= C) return;          // C % 4 == 0: whole float4 in or out (lanes of other phases agree)
    if (len <= 0) {              // an empty chunk has no statistics: NaN (the split path: stats_pool_merge_kernel)
        if (max_splits == 1 && phase == 0) {
            const float nan = __builtin_nanf("");
            float *o = out + (size_t)b * 2 * C;
            *reinterpret_cast<f32x4 *>(o + c) = (f32x4){nan, nan, nan, nan};
            *reinterpret_cast<f32x4 *>(o + C + c) = (f32x4){nan, nan, nan, nan};
        }
        return;
    }
    if (begin >= len) return;
    const int n_rows = min(split_rows, len - begin);
    const float *base = h + ((size_t)row_start[b] + begin) * ldh + c;

    Stat4 s;
    s.mean = (f32x4){0.f, 0.f, 0.f, 0.f};
    s.m2 = s.mean;
    s.n = 0.f;

    int r = phase;
    // full blocks: 8 rows per lane (rows r, r+4, ..., r+28)
    for (; r + 4 * (POOL_UNROLL - 1) < n_rows; r += 4 * POOL_UNROLL) {
        f32x4 v[POOL_UNROLL];
#pragma unroll
        for (int i = 0; i < POOL_UNROLL; ++i)
            v[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(base + (size_t)(r + 4 * i) * ldh));
        // block statistics about v[0] (shifted): exact for constant channels, no cancellation
        f32x4 d[POOL_UNROLL];
        f32x4 sumd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 1; i < POOL_UNROLL; ++i) {
            d[i] = v[i] - v[0];
            sumd += d[i];
        }
        const f32x4 md = sumd * (1.0f / POOL_UNROLL);
        const f32x4 bm = v[0] + md;
        f32x4 m2 = md * md;                 // element 0: (0 - md)^2
#pragma unroll
        for (int i = 1; i < POOL_UNROLL; ++i) {
            const f32x4 e = d[i] - md;
            m2 += e * e;
        }
        chan_merge(s, bm, m2, (float)POOL_UNROLL);
    }
    // tail: fewer than 8 rows left for this lane
    if (r < n_rows) {
        f32x4 v[POOL_UNROLL];
        int m = 0;
#pragma unroll
        for (int i = 0; i < POOL_UNROLL; ++i) {
            const bool ok = (r + 4 * i) < n_rows;
            v[i] = ok ? *reinterpret_cast<const f32x4 *>(base + (size_t)(r + 4 * i) * ldh) : (f32x4){0.f, 0.f, 0.f, 0.f};
            m += ok ? 1 : 0;
        }
        const float fm = (float)m;          // m >= 1: v[0] is always a real row
        f32x4 sumd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 1; i < POOL_UNROLL; ++i)
            if ((r + 4 * i) < n_rows) sumd += v[i] - v[0];
        const f32x4 md = sumd / fm;
        const f32x4 bm = v[0] + md;
        f32x4 m2 = md * md;
#pragma unroll
        for (int i = 1; i < POOL_UNROLL; ++i) {
            const f32x4 e = (v[i] - v[0]) - md;
            if ((r + 4 * i) < n_rows) m2 += e * e;
        }
        chan_merge(s, bm, m2, fm);
    }

    // combine the 4 row phases of the wave: shuffle-xor 16 then 32 (Chan merge of (n, mean, M2))
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        Stat4 o;
        o.n = __shfl_xor(s.n, off, 64);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o.mean[i] = __shfl_xor(s.mean[i], off, 64);
            o.m2[i] = __shfl_xor(s.m2[i], off, 64);
        }
        chan_merge(s, o.mean, o.m2, o.n);
    }
    if (phase != 0) return;
    if (max_splits == 1) {
        const f32x4 var = s.m2 / s.n;
        f32x4 sd;
#pragma unroll
        for (int i = 0; i < 4; ++i) sd[i] = raw ? var[i] : sqrtf(var[i] + eps);      // raw: (mean, biased variance)
        float *o = out + (size_t)b * 2 * C;
        *reinterpret_cast<f32x4 *>(o + c) = s.mean;
        *reinterpret_cast<f32x4 *>(o + C + c) = sd;
    } else {
        float *pm = partial + ((size_t)b * max_splits + sp) * 2 * C;
        *reinterpret_cast<f32x4 *>(pm + c) = s.mean;
        *reinterpret_cast<f32x4 *>(pm + C + c) = s.m2;
    }
}

// second stage for split chunks: merge the per-split (mean, M2) in split order, finalize
__global__ void stats_pool_merge_kernel(const float *__restrict__ partial, int C, const int *__restrict__ row_len,
                                        int split_rows, int max_splits, float eps, float *__restrict__ out, int raw)
{
    const int b = blockIdx.y;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int len = row_len[b];
    if (len <= 0) {              // empty chunk: NaN, as the direct path
        out[(size_t)b * 2 * C + c] = __builtin_nanf("");
        out[(size_t)b * 2 * C + C + c] = __builtin_nanf("");
        return;
    }
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int sp = 0; sp * split_rows < len; ++sp) {
        const float m = (float)min(split_rows, len - sp * split_rows);
        const float *pm = partial + ((size_t)b * max_splits + sp) * 2 * C;
        const float bm = pm[c], bm2 = pm[C + c];
        const float nn = n + m;
        const float w = m / nn;
        const float d = bm - mean;
        mean += d * w;
        m2 += bm2 + d * d * (n * w);
        n = nn;
    }
    out[(size_t)b * 2 * C + c] = mean;
    out[(size_t)b * 2 * C + C + c] = raw ? m2 / n : sqrtf(m2 / n + eps);
}

// finalize for the POOL epilogue of the bf16x3 GEMM: chunk b = the 8-row blocks row_start[b]/8 ... in order (all full but
// the last); per channel  mean = sum n_i*mean_i / N,  var = sum(M2_i + n_i*mean_i^2)/N - mean^2  in fp64 (the inputs are
// fp32, so the subtraction loses nothing that matters), out = [mean | sqrt(var + eps)].  A chunk that does not start on a
// multiple of 8 rows was not reduced block-wise by the epilogue: its outputs are set to NaN.
__global__ void stats_pool_blocks_kernel(const float *__restrict__ blk, int C, const int *__restrict__ row_start,
                                         const int *__restrict__ row_len, float eps, float *__restrict__ out)
{
    const int b = blockIdx.y;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int rs = row_start[b], len = row_len[b];
    float *o = out + (size_t)b * 2 * C;
    if ((rs & 7) || len <= 0) {
        o[c] = __builtin_nanf("");
        o[C + c] = __builtin_nanf("");
        return;
    }
    const float *pb = blk + (size_t)(rs >> 3) * 2 * C + c;
    const int nb = (len + 7) >> 3;
    double S = 0.0, Q = 0.0;
#pragma unroll 4
    for (int i = 0; i < nb; ++i) {
        const double m = (double)__builtin_nontemporal_load(pb + (size_t)i * 2 * C);
        const double m2 = (double)__builtin_nontemporal_load(pb + (size_t)i * 2 * C + C);
        const double n = (double)min(8, len - 8 * i);
        S += n * m;
        Q += m2 + n * m * m;
    }
    const double mean = S / (double)len;
    const double var = fmax(Q / (double)len - mean * mean, 0.0);
    o[c] = (float)mean;
    o[C + c] = sqrtf((float)var + eps);
}

// float32 op order of NumPy in local/tf/models.py:418-421: p = len*e (rounded), acc += p (rounded),
// acc /= total.  __fmul_rn/__fadd_rn/__fdiv_rn forbid FMA contraction.
__global__ void chunk_average_kernel(const float *__restrict__ e, const int *__restrict__ seg_start,
                                     const int *__restrict__ chunk_len, int dim, float *__restrict__ out)
{
#pragma clang fp contract(off)      // hipcc contracts a*b+c into fma by default; NumPy does not
    const int u = blockIdx.y;
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= dim) return;
    const int s0 = seg_start[u], s1 = seg_start[u + 1];
    float acc = 0.f;
    double tot = 0.0;
    for (int i = s0; i < s1; ++i) {
        const float w = (float)chunk_len[i];
        float prod = w * e[(size_t)i * dim + d];
        asm volatile("" : "+v"(prod));      // opaque to the optimiser: product is rounded before the add
        acc = acc + prod;
        tot += (double)chunk_len[i];
    }
    out[(size_t)u * dim + d] = acc / (float)tot;      // IEEE-correct fp32 division (hipcc default)
}

}  // namespace

extern "C" {

size_t xv_block_stats_bytes(int64_t R, int cout)
{
    if (R <= 0 || cout <= 0) return 0;
    return (size_t)((R + 7) / 8) * 2 * (size_t)cout * sizeof(float);
}

int xv_stats_pool_blocks_f32(const float *block_stats, int c, const int32_t *row_start, const int32_t *row_len, int nchunks,
                             float eps, float *out, void *stream)
{
    if (nchunks <= 0) return 0;
    if (!block_stats || !row_start || !row_len || !out || c <= 0) return fail(XV_ERR_BAD_ARG, "stats_pool_blocks: bad argument");
    hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < nchunks; b0 += 65535) {
        const int nb = min(65535, nchunks - b0);
        hipLaunchKernelGGL(stats_pool_blocks_kernel, dim3((c + 255) / 256, nb), dim3(256), 0, st, block_stats, c, row_start + b0,
                           row_len + b0, eps, out + (size_t)b0 * 2 * c);
        int rc = launch_status("stats_pool_blocks_kernel");
        if (rc) return rc;
    }
    return 0;
}

size_t xv_stats_pool_workspace_bytes(int c, int nchunks, int max_len, int split_rows)
{
    if (split_rows <= 0 || max_len <= split_rows) return 0;
    const size_t splits = ((size_t)max_len + split_rows - 1) / split_rows;
    return (size_t)nchunks * splits * 2 * (size_t)c * sizeof(float);
}

static int stats_pool_impl(const float *h, int64_t ldh, int c, const int32_t *row_start, const int32_t *row_len, int nchunks,
                           int max_len, int split_rows, float eps, float *out, void *workspace, void *stream, int raw)
{
    if (nchunks <= 0) return 0;
    if (!h || !row_start || !row_len || !out) return fail(XV_ERR_BAD_ARG, "stats_pool: NULL pointer");
    if (c <= 0 || (c & 3) || (ldh & 3) || ldh < c || (((uintptr_t)h) & 15) || (((uintptr_t)out) & 15))
        return fail(XV_ERR_BAD_ARG, "stats_pool: C, ldh >= C must be multiples of 4 and h/out 16-byte aligned");
    if (split_rows <= 0 || max_len <= 0) return fail(XV_ERR_BAD_ARG, "stats_pool: split_rows/max_len must be > 0");
    const int max_splits = (max_len + split_rows - 1) / split_rows;
    if (max_splits > 1 && !workspace) return fail(XV_ERR_BAD_ARG, "stats_pool: workspace required for split chunks");
    if (max_splits > 65535) return fail(XV_ERR_UNSUPPORTED, "stats_pool: too many splits");
    hipStream_t st = (hipStream_t)stream;
    // grid.z is limited to 65535: loop over slices of chunks
    for (int b0 = 0; b0 < nchunks; b0 += 65535) {
        const int nb = min(65535, nchunks - b0);
        const dim3 grid((c + 255) / 256, max_splits, nb);
        hipLaunchKernelGGL(stats_pool_kernel, grid, dim3(256), 0, st, h, (long)ldh, c, row_start + b0, row_len + b0,
                           split_rows, max_splits, eps, out + (size_t)b0 * 2 * c,
                           (float *)workspace + (size_t)b0 * max_splits * 2 * c, raw);
        int rc = launch_status("stats_pool_kernel");
        if (rc) return rc;
        if (max_splits > 1) {
            hipLaunchKernelGGL(stats_pool_merge_kernel, dim3((c + 255) / 256, nb), dim3(256), 0, st,
                               (const float *)workspace + (size_t)b0 * max_splits * 2 * c, c, row_len + b0, split_rows,
                               max_splits, eps, out + (size_t)b0 * 2 * c, raw);
            rc = launch_status("stats_pool_merge_kernel");
            if (rc) return rc;
        }
    }
    return 0;
}

int xv_stats_pool_f32(const float *h, int64_t ldh, int c, const int32_t *row_start, const int32_t *row_len, int nchunks,
                      int max_len, int split_rows, float eps, float *out, void *workspace, void *stream)
{
    return stats_pool_impl(h, ldh, c, row_start, row_len, nchunks, max_len, split_rows, eps, out, workspace, stream, 0);
}

int xv_chunk_moments_f32(const float *h, int64_t ldh, int c, const int32_t *row_start, const int32_t *row_len, int nchunks,
                         int max_len, int split_rows, float *out, void *workspace, void *stream)
{
    return stats_pool_impl(h, ldh, c, row_start, row_len, nchunks, max_len, split_rows, 0.f, out, workspace, stream, 1);
}

int xv_chunk_average_f32(const float *e, const int32_t *seg_start, const int32_t *chunk_len, int nutts, int dim, float *out,
                         void *stream)
{
    if (nutts <= 0) return 0;
    if (!e || !seg_start || !chunk_len || !out || dim <= 0) return fail(XV_ERR_BAD_ARG, "chunk_average: bad argument");
    hipStream_t st = (hipStream_t)stream;
    for (int u0 = 0; u0 < nutts; u0 += 65535) {
        const int nu = min(65535, nutts - u0);
        hipLaunchKernelGGL(chunk_average_kernel, dim3((dim + 255) / 256, nu), dim3(256), 0, st, e, seg_start + u0, chunk_len,
                           dim, out + (size_t)u0 * dim);
        int rc = launch_status("chunk_average_kernel");
        if (rc) return rc;
    }
    return 0;
}

}  // extern "C"
