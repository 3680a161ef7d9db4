// xv_backend.hip -- the PLDA / cosine scoring back-end on the MI355X.
//
// What stage 9 of the recipe (run.sh) does with Kaldi binaries, for the part that scales with the data:
//     ivector-subtract-global-mean mean.vec | transform-vec transform.mat | ivector-normalize-length   (both sides)
//     ivector-plda-scoring --num-utts=...                                                             (TransformIvector + LLR)
// The PLDA log-likelihood ratio of Kaldi's Plda::LogLikelihoodRatio is one dot product of length K = 2d plus a per-enrolment
// constant:
//     enrolment row [ (a/v) z , 1/v - 1/w ]    test row [ t , -t^2/2 ]    r_e = -1/2 sum a^2 z^2 / v + 1/2 sum (log w - log v)
// with a = n psi / (n psi + 1), v = 1 + psi / (n psi + 1), w = 1 + psi.  Five kernels:
//   backend_prepare_kernel   x -> operand rows: (x - mu), LDA, length norm, PLDA transform, PLDA length norm, side packing.
//                            32 rows per workgroup; both products on v_mfma_f32_32x32x2_f32 (exact fp32), the rows stay in LDS
//                            between the two products and the two norms.
//   score_matrix_kernel      S = E T^T + r on v_mfma_f32_32x32x2_f32, 128 x 128 tiles, one accumulator per score, k ascending.
//   score_blocks_kernel      the same tile body (score_tile) over ragged groups of rows: each group against itself, every
//                            group's matrix from one launch (diarization).
//   score_pairs_kernel       one trial per thread: an fmaf chain over k ascending from 0, then + r.
//   topk_row_stats_kernel    AS-norm cohort statistics: mean and population std of the top-N scores of each row, by an exact
//                            MSB-first radix select on order-preserving keys (rows of <= 32768 columns staged in LDS), fp64 sums.
// The f32-input MFMA is an fmaf chain over its two k values (lanes 0-31 carry k, lanes 32-63 carry k + 1), so the matrix kernel
// feeds k in ascending pairs (2s, 2s + 1) and the pairs kernel reproduces its bits (tests/test_gpu_backend.py checks it).
#include "xv_device.h"

namespace {

constexpr int KSTEP = XV_BACKEND_KSTEP;      // operand rows are padded to a multiple of this (zeros)

// ---------------------------------------------------------------------------------------------------------------------------
// prepare
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int PR_ROWS = 32;                  // rows per workgroup (one MFMA block of rows)
constexpr int PR_NT = 256;                   // 4 waves; wave w owns output columns [64 w, 64 w + 64)
constexpr int PR_BK = 32;                    // k per LDS stage of the products
constexpr int PR_LDK = PR_BK + 1;            // odd stride: the 32 lanes of a half-wave read 32 rows at one k without conflicts
constexpr int PR_DMAX = 256;                 // d <= 256 (8 column blocks of 32)
constexpr int PR_LDY = PR_DMAX + 1;

struct PrepParams {
    const float *x; long ldx; int N, D;
    const int32_t *n;
    const float *mu, *A; long lda; const float *a0; int d; int length_norm;
    const float *P, *m, *psi;
    int side; float *out; long ldo; float *r;
};

// acc[b] (b = column block 0/1 of the wave) += rows(32 x kc of Xs) * (cols of Bs)^T over kc values of the current stage
__device__ __forceinline__ void prep_mfma_stage(const float *__restrict__ Xs, int ldx, const float *__restrict__ Bs, int kc, int wave,
                                                int lane, int ncols, f32x16 &acc0, f32x16 &acc1)
{
    const int h = lane >> 5, l = lane & 31;
    const int c0 = wave * 64 + l;
    const bool b0 = wave * 64 < ncols, b1 = wave * 64 + 32 < ncols;
    for (int k = 0; k < kc; k += 2) {
        const float a = Xs[l * ldx + k + h];
        if (b0) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[c0 * PR_LDK + k + h], acc0, 0, 0, 0);
        if (b1) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[(c0 + 32) * PR_LDK + k + h], acc1, 0, 0, 0);
    }
}

// the 32 x ncols result of a product into Ys (+ bias[c] when bias is not NULL)
__device__ __forceinline__ void prep_store_acc(float *Ys, const f32x16 &acc0, const f32x16 &acc1, int wave, int lane, int ncols,
                                               const float *__restrict__ bias)
{
    const int col = wave * 64 + (lane & 31);
    const int rowb = 4 * (lane >> 5);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = rowb + (i & 3) + 8 * (i >> 2);
        if (col < ncols) Ys[row * PR_LDY + col] = acc0[i] + (bias ? bias[col] : 0.0f);
        if (col + 32 < ncols) Ys[row * PR_LDY + col + 32] = acc1[i] + (bias ? bias[col + 32] : 0.0f);
    }
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(PR_NT) void backend_prepare_kernel(const PrepParams p)
{
    __shared__ float Xs[PR_ROWS * PR_LDK];           // 32 rows x 32 k of the input (mean subtracted)
    __shared__ float Bs[PR_DMAX * PR_LDK];           // up to 256 rows x 32 k of A or P
    __shared__ float Ys[PR_ROWS * PR_LDY];           // the workgroup's rows between the steps
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.x * PR_ROWS;
    const int d = p.d;

    // ---- y = A (x - mu) + a0   (A NULL: y = x - mu, d == D) ----
    if (p.A) {
        f32x16 acc0 = {0}, acc1 = {0};
        for (int k0 = 0; k0 < p.D; k0 += PR_BK) {
            const int kc = min(PR_BK, p.D - k0);
            for (int f = tid; f < PR_ROWS * PR_BK; f += PR_NT) {
                const int rr = f / PR_BK, kk = f % PR_BK;
                float v = 0.0f;
                if (row0 + rr < p.N && kk < kc) v = p.x[(row0 + rr) * p.ldx + k0 + kk] - (p.mu ? p.mu[k0 + kk] : 0.0f);
                Xs[rr * PR_LDK + kk] = v;
            }
            for (int f = tid; f < d * PR_BK; f += PR_NT) {
                const int rr = f / PR_BK, kk = f % PR_BK;
                Bs[rr * PR_LDK + kk] = kk < kc ? p.A[rr * p.lda + k0 + kk] : 0.0f;
            }
            __syncthreads();
            prep_mfma_stage(Xs, PR_LDK, Bs, (kc + 1) & ~1, wave, lane, d, acc0, acc1);
            __syncthreads();
        }
        prep_store_acc(Ys, acc0, acc1, wave, lane, d, p.a0);
    } else {
        for (int f = tid; f < PR_ROWS * d; f += PR_NT) {
            const int rr = f / d, c = f % d;
            Ys[rr * PR_LDY + c] = row0 + rr < p.N ? p.x[(row0 + rr) * p.ldx + c] - (p.mu ? p.mu[c] : 0.0f) : 0.0f;
        }
    }
    __syncthreads();

    // ---- ivector-normalize-length: y *= sqrt(d) / |y|  (a zero vector stays as it is) ----
    if (p.length_norm) {
        for (int rr = wave; rr < PR_ROWS; rr += PR_NT / 64) {
            float s = 0.0f;
            for (int c = lane; c < d; c += 64) s = fmaf(Ys[rr * PR_LDY + c], Ys[rr * PR_LDY + c], s);
            s = wave_sum(s);
            const float scale = s > 0.0f ? sqrtf((float)d) / sqrtf(s) : 1.0f;
            for (int c = lane; c < d; c += 64) Ys[rr * PR_LDY + c] *= scale;
        }
        __syncthreads();
    }

    // ---- PLDA TransformIvector: z = P (y - m), z *= sqrt(d / sum z^2 / (psi + 1/n)) ----
    if (p.P) {
        for (int f = tid; f < PR_ROWS * d; f += PR_NT) {
            const int rr = f / d, c = f % d;
            Ys[rr * PR_LDY + c] -= p.m[c];
        }
        f32x16 acc0 = {0}, acc1 = {0};
        for (int k0 = 0; k0 < d; k0 += PR_BK) {
            const int kc = min(PR_BK, d - k0);
            __syncthreads();
            for (int f = tid; f < d * PR_BK; f += PR_NT) {
                const int rr = f / PR_BK, kk = f % PR_BK;
                Bs[rr * PR_LDK + kk] = kk < kc ? p.P[(long)rr * d + k0 + kk] : 0.0f;
            }
            // the operand rows (y - m) for this stage, zero past d
            for (int f = tid; f < PR_ROWS * PR_BK; f += PR_NT) {
                const int rr = f / PR_BK, kk = f % PR_BK;
                Xs[rr * PR_LDK + kk] = kk < kc ? Ys[rr * PR_LDY + k0 + kk] : 0.0f;
            }
            __syncthreads();
            prep_mfma_stage(Xs, PR_LDK, Bs, (kc + 1) & ~1, wave, lane, d, acc0, acc1);
        }
        __syncthreads();
        prep_store_acc(Ys, acc0, acc1, wave, lane, d, nullptr);
        __syncthreads();
        for (int rr = wave; rr < PR_ROWS; rr += PR_NT / 64) {
            const float nn = (row0 + rr < p.N && p.n) ? (float)p.n[row0 + rr] : 1.0f;
            float s = 0.0f;
            for (int c = lane; c < d; c += 64) {
                const float z = Ys[rr * PR_LDY + c];
                s += z * z / (p.psi[c] + 1.0f / nn);
            }
            s = wave_sum(s);
            const float scale = s > 0.0f ? sqrtf((float)d / s) : 1.0f;
            for (int c = lane; c < d; c += 64) Ys[rr * PR_LDY + c] *= scale;
        }
        __syncthreads();
    }

    // ---- operand rows of the side ----
    for (int rr = wave; rr < PR_ROWS; rr += PR_NT / 64) {
        const long row = row0 + rr;
        if (row >= p.N) break;                                   // wave-uniform
        float *o = p.out + row * p.ldo;
        const float *z = Ys + rr * PR_LDY;
        float rv = 0.0f;
        if (p.side == XV_SIDE_ENROL) {
            const float nn = p.n ? (float)p.n[row] : 1.0f;
            for (int c = lane; c < d; c += 64) {
                const float psi = p.psi[c];
                const float a = nn * psi / (nn * psi + 1.0f);
                const float v = 1.0f + psi / (nn * psi + 1.0f);
                const float w = 1.0f + psi;
                o[c] = a / v * z[c];
                o[d + c] = 1.0f / v - 1.0f / w;
                rv += -0.5f * a * a * z[c] * z[c] / v + 0.5f * (logf(w) - logf(v));
            }
            for (long c = 2 * d + lane; c < p.ldo; c += 64) o[c] = 0.0f;
        } else if (p.side == XV_SIDE_TEST) {
            for (int c = lane; c < d; c += 64) {
                o[c] = z[c];
                o[d + c] = -0.5f * z[c] * z[c];
            }
            for (long c = 2 * d + lane; c < p.ldo; c += 64) o[c] = 0.0f;
        } else {
            float scale = 1.0f;
            if (p.side == XV_SIDE_COSINE) {
                float s = 0.0f;
                for (int c = lane; c < d; c += 64) s = fmaf(z[c], z[c], s);
                s = wave_sum(s);
                scale = s > 0.0f ? 1.0f / sqrtf(s) : 1.0f;
            }
            for (int c = lane; c < d; c += 64) o[c] = z[c] * scale;
            for (long c = d + lane; c < p.ldo; c += 64) o[c] = 0.0f;
        }
        rv = wave_sum(rv);
        if (p.r && lane == 0) p.r[row] = rv;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// dense scorer: S[Ne, Nt] = E[Ne, K] T[Nt, K]^T + r[e]
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int SM_BM = 128, SM_BN = 128;      // tile; 4 waves in 2 x 2, 64 x 64 (2 x 2 MFMA blocks) per wave
constexpr int SM_BK = 32;                    // k per LDS stage
constexpr int SM_NT = 256;
constexpr int SM_LDK = SM_BK + 4;            // row stride in LDS (floats): 16-B aligned f32x4 reads
constexpr int SM_UNITS = (SM_BM + SM_BN) * (SM_BK / 8) / SM_NT;     // 8-float pieces per thread and stage (4)

// LDS image of 8 consecutive k of one row: [k0 k2 k4 k6 | k1 k3 k5 k7], so that a lane of half h reads ONE f32x4 at
// 8 kk + 4 h and finds k = 8 kk + 2 s + h in element s: the MFMA of step s then sums k = 2s (lanes 0-31) and 2s + 1 (32-63).
// The tile body of both dense kernels: the 128 x 128 tile at (e0, t0) of S = E T^T + r.  smem: (SM_BM + SM_BN) * SM_LDK floats.
__device__ __forceinline__ void score_tile(const float *__restrict__ E, const float *__restrict__ T, int ldk, int kpad, int Ne, int Nt,
                                           const float *__restrict__ r, float *__restrict__ S, long lds, long e0, long t0,
                                           f32x4 *smem)
{
    float *As = reinterpret_cast<float *>(smem);
    float *Bs = As + SM_BM * SM_LDK;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;

    f32x4 reg[SM_UNITS][2];
    auto load = [&](int k0) {
#pragma unroll
        for (int u = 0; u < SM_UNITS; ++u) {
            const int f = tid + SM_NT * u;               // piece: row (f >> 2) of A | B, k block (f & 3)
            const int rr = f >> 2, kb = (f & 3) * 8;
            const bool isA = rr < SM_BM;
            const long grow = isA ? e0 + rr : t0 + rr - SM_BM;
            const long nrows = isA ? Ne : Nt;
            const float *src = (isA ? E : T) + grow * ldk + k0 + kb;
            if (grow < nrows && k0 + kb < kpad) {
                reg[u][0] = *reinterpret_cast<const f32x4 *>(src);
                reg[u][1] = *reinterpret_cast<const f32x4 *>(src + 4);
            } else {
                reg[u][0] = f32x4{0, 0, 0, 0};
                reg[u][1] = f32x4{0, 0, 0, 0};
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int u = 0; u < SM_UNITS; ++u) {
            const int f = tid + SM_NT * u;
            const int rr = f >> 2, kb = (f & 3) * 8;
            float *dst = As + rr * SM_LDK + kb;          // (Bs follows As: rows >= 128 land in Bs)
            const f32x4 lo = reg[u][0], hi = reg[u][1];
            *reinterpret_cast<f32x4 *>(dst) = f32x4{lo[0], lo[2], hi[0], hi[2]};
            *reinterpret_cast<f32x4 *>(dst + 4) = f32x4{lo[1], lo[3], hi[1], hi[3]};
        }
    };

    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
    load(0);
    for (int k0 = 0; k0 < kpad; k0 += SM_BK) {
        store();
        __syncthreads();
        if (k0 + SM_BK < kpad) load(k0 + SM_BK);
        const int h = lane >> 5, l = lane & 31;
        const float *Ab = As + (wr * 64 + l) * SM_LDK + 4 * h;
        const float *Bb = Bs + (wc * 64 + l) * SM_LDK + 4 * h;
        const int nkk = min(SM_BK, kpad - k0) / 8;
        for (int kk = 0; kk < nkk; ++kk) {
            const f32x4 a0 = *reinterpret_cast<const f32x4 *>(Ab + kk * 8);
            const f32x4 a1 = *reinterpret_cast<const f32x4 *>(Ab + 32 * SM_LDK + kk * 8);
            const f32x4 b0 = *reinterpret_cast<const f32x4 *>(Bb + kk * 8);
            const f32x4 b1 = *reinterpret_cast<const f32x4 *>(Bb + 32 * SM_LDK + kk * 8);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b0[s], acc00, 0, 0, 0);
                acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b1[s], acc01, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b0[s], acc10, 0, 0, 0);
                acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b1[s], acc11, 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // epilogue: score + r[e], masked edges; 32 lanes of a half-wave store 128 consecutive bytes of one row
    const long colb = t0 + wc * 64 + (lane & 31);
    const long rowb = e0 + wr * 64 + 4 * (lane >> 5);
    auto put = [&](const f32x16 &acc, int rb, int cb) {
        const long c = colb + 32 * cb;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long e = rowb + 32 * rb + (i & 3) + 8 * (i >> 2);
            if (e < Ne && c < Nt) S[e * lds + c] = acc[i] + (r ? r[e] : 0.0f);
        }
    };
    put(acc00, 0, 0);
    put(acc01, 0, 1);
    put(acc10, 1, 0);
    put(acc11, 1, 1);
}

__global__ __launch_bounds__(SM_NT, 2) void score_matrix_kernel(const float *__restrict__ E, const float *__restrict__ T, int ldk,
                                                                int kpad, int Ne, int Nt, const float *__restrict__ r,
                                                                float *__restrict__ S, long lds)
{
    __shared__ f32x4 smem[(SM_BM + SM_BN) * SM_LDK / 4];
    score_tile(E, T, ldk, kpad, Ne, Nt, r, S, lds, (long)blockIdx.y * SM_BM, (long)blockIdx.x * SM_BN, smem);
}

// Block-diagonal self-scoring of ragged groups: workgroup (tile, group).  Group g = g0 + blockIdx.y is rows
// [grp_row0[g], grp_row0[g + 1]) of E, T and r; its n x n matrix goes to S + grp_score0[g] with row stride (n + 3) & ~3.  A tile
// past the group's own tiles exits; a group that breaks the contract of xv_score_blocks_f32 is skipped whole (nothing of it is read
// or written) and *status = 1.  Every test below is uniform over the workgroup.
__global__ __launch_bounds__(SM_NT, 2) void score_blocks_kernel(const float *__restrict__ E, const float *__restrict__ T, int ldk,
                                                                int kpad, int n_rows, const float *__restrict__ r,
                                                                const int32_t *__restrict__ grp_row0,
                                                                const int64_t *__restrict__ grp_score0, int g0, int max_n,
                                                                float *__restrict__ S, long scores_elems, int32_t *status)
{
    __shared__ f32x4 smem[(SM_BM + SM_BN) * SM_LDK / 4];
    const int g = g0 + blockIdx.y;
    const long row0 = grp_row0[g], n = (long)grp_row0[g + 1] - row0;
    const long off = grp_score0[g], ld = (n + 3) & ~3L;
    if (n < 1 || n > max_n || row0 < 0 || row0 + n > n_rows || off < 0 || (off & 3) || off > scores_elems ||
        n * ld > scores_elems - off) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *status = 1;
        return;
    }
    const int tiles = (int)((n + SM_BM - 1) / SM_BM);
    if ((int)blockIdx.x >= tiles * tiles) return;
    const int by = blockIdx.x / tiles, bx = blockIdx.x % tiles;
    score_tile(E + row0 * ldk, T + row0 * ldk, ldk, kpad, (int)n, (int)n, r ? r + row0 : nullptr, S + off, ld, (long)by * SM_BM,
               (long)bx * SM_BN, smem);
}

// ---------------------------------------------------------------------------------------------------------------------------
// trial-list scorer: score[i] = sum_k E[e_idx[i], k] T[t_idx[i], k] (fmaf chain, k ascending) + r[e_idx[i]]
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void score_pairs_kernel(const float *__restrict__ E, const float *__restrict__ T, int ldk, int kpad,
                                                          const int32_t *__restrict__ e_idx, const int32_t *__restrict__ t_idx, long M,
                                                          const float *__restrict__ r, float *__restrict__ score)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const long e = e_idx[i], t = t_idx[i];
    const f32x4 *a = reinterpret_cast<const f32x4 *>(E + e * ldk);
    const f32x4 *b = reinterpret_cast<const f32x4 *>(T + t * ldk);
    float acc = 0.0f;
    for (int k = 0; k < kpad / 4; ++k) {
        const f32x4 x = a[k], y = b[k];
        acc = fmaf(x[0], y[0], acc);
        acc = fmaf(x[1], y[1], acc);
        acc = fmaf(x[2], y[2], acc);
        acc = fmaf(x[3], y[3], acc);
    }
    score[i] = acc + (r ? r[e] : 0.0f);
}

// ---------------------------------------------------------------------------------------------------------------------------
// top-N row statistics (AS-norm): mean and population std of the top_n largest values of each row, by an exact radix select
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int TK_NT = 256;                   // one workgroup per row; thread t owns bin t of the 8-bit digit in the scan
constexpr int TK_STAGE_MAX = 32768;          // rows of up to this many columns are staged in LDS as keys (128 KiB)
constexpr int TK_HDR = 1280;                 // LDS in front of the staged keys: histogram (1 KiB), scan and reduction scratch
constexpr int TK_LDS_MAX = TK_HDR + 4 * TK_STAGE_MAX;

// order-preserving float -> uint32 (x < y implies key(x) < key(y)); every NaN, of either sign, maps to the largest key
__device__ __forceinline__ uint32_t tk_key(float x)
{
    const uint32_t u = __float_as_uint(x);
    if (x != x) return 0xffffffffu;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float tk_value(uint32_t k)
{
    if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Row blockIdx.x.  Four MSB-first passes over 8-bit digits find tau, the key of the top_n-th largest value, and g, the number
// of keys above it; the selection is every key above tau plus (top_n - g) copies of tau.  Its sum, then its centred sum of
// squares, are accumulated in fp64.  Every thread visits its columns in one fixed order (4-column groups tid, tid + NT, ...,
// then the tail group) and the block sums in one fixed tree, so a row's bits depend on its values, n_cols and top_n alone.
__global__ __launch_bounds__(TK_NT) void topk_row_stats_kernel(const float *__restrict__ scores, long ld, int n_cols, int top_n,
                                                               float *__restrict__ mean, float *__restrict__ stdev)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    uint32_t *hist = reinterpret_cast<uint32_t *>(lds);          // [256]
    uint32_t *wtot = hist + 256;                                  // [4] wave totals of the scan
    uint32_t *sel = wtot + 4;                                     // [2] the chosen digit, keys above its bin
    double *dred = reinterpret_cast<double *>(lds + 1088);        // [4] wave partial sums
    uint32_t *stage = reinterpret_cast<uint32_t *>(lds + TK_HDR);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *row = scores + (long)blockIdx.x * ld;
    const bool staged = n_cols <= TK_STAGE_MAX;
    const int nvec = n_cols >> 2;

    // f(column, key, value) over the thread's columns from global memory (four 16-B loads in flight) or from the staged keys
    auto visit = [&](bool from_lds, auto &&f) {
        if (from_lds) {
            for (int v = tid; v < nvec; v += TK_NT) {
                const uint4 k = reinterpret_cast<const uint4 *>(stage)[v];
                f(4 * v, k.x, tk_value(k.x));
                f(4 * v + 1, k.y, tk_value(k.y));
                f(4 * v + 2, k.z, tk_value(k.z));
                f(4 * v + 3, k.w, tk_value(k.w));
            }
        } else {
            const f32x4 *rv = reinterpret_cast<const f32x4 *>(row);
            int v = tid;
            for (; v + 3 * TK_NT < nvec; v += 4 * TK_NT) {
                f32x4 x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) x[u] = rv[v + u * TK_NT];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) f(4 * (v + u * TK_NT) + j, tk_key(x[u][j]), x[u][j]);
            }
            for (; v < nvec; v += TK_NT) {
                const f32x4 x = rv[v];
#pragma unroll
                for (int j = 0; j < 4; ++j) f(4 * v + j, tk_key(x[j]), x[j]);
            }
        }
        if (tid == nvec % TK_NT)
            for (int c = 4 * nvec; c < n_cols; ++c) {
                const uint32_t k = from_lds ? stage[c] : tk_key(row[c]);
                f(c, k, from_lds ? tk_value(k) : row[c]);
            }
    };

    // ---- radix select ----
    uint32_t prefix = 0, mask = 0;
    uint32_t k = (uint32_t)top_n;                                 // rank of the target among the keys matching prefix / mask
    for (int p = 0; p < 4; ++p) {
        const int shift = 24 - 8 * p;
        hist[tid] = 0;
        __syncthreads();
        auto count = [&](int c, uint32_t key, float) {
            if (p == 0 && staged) stage[c] = key;
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        };
        visit(p > 0 && staged, count);
        __syncthreads();
        // inclusive sums from the top bin down: thread t holds bin 255 - t
        const uint32_t h = hist[255 - tid];
        uint32_t inc = h;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(inc, o, 64);
            if (lane >= o) inc += y;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        for (int w = 0; w < wave; ++w) inc += wtot[w];
        if (inc - h < k && k <= inc) {                           // exactly one bin: the count crosses k inside it
            sel[0] = 255 - tid;
            sel[1] = inc - h;
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        mask |= 255u << shift;
        k -= sel[1];
        __syncthreads();
    }
    const uint32_t tau = prefix;                                  // k copies of tau complete the selection

    auto block_sum = [&](double v) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        __syncthreads();
        if (lane == 0) dred[wave] = v;
        __syncthreads();
        return (dred[0] + dred[1]) + (dred[2] + dred[3]);
    };
    const double tv = (double)tk_value(tau);
    double s = 0.0;
    visit(staged, [&](int, uint32_t key, float x) {
        if (key > tau) s += (double)x;
    });
    const double mu = (block_sum(s) + (double)k * tv) / top_n;
    double q = 0.0;
    visit(staged, [&](int, uint32_t key, float x) {
        if (key > tau) {
            const double d = (double)x - mu;
            q += d * d;
        }
    });
    const double dt = tv - mu;
    const double var = (block_sum(q) + (double)k * dt * dt) / top_n;
    if (tid == 0) {
        mean[blockIdx.x] = (float)mu;
        stdev[blockIdx.x] = (float)sqrt(var);
    }
}

}  // namespace

extern "C" int xv_backend_prepare_f32(const float *x, int64_t ldx, int n_rows, int dim_in, const int32_t *num_utts, const float *mean,
                                      const float *lda, int64_t ld_lda, const float *lda_offset, int dim, int length_norm,
                                      const float *plda_transform, const float *plda_mean, const float *plda_psi, int side, float *out,
                                      int64_t ldo, float *r, void *stream)
{
    if (n_rows <= 0) return 0;
    if (!x || !out || dim <= 0 || dim_in <= 0 || ldx < dim_in || side < XV_SIDE_PLAIN || side > XV_SIDE_COSINE)
        return fail(XV_ERR_BAD_ARG, "backend_prepare: bad argument");
    if (lda ? ld_lda < dim_in : dim != dim_in) return fail(XV_ERR_BAD_ARG, "backend_prepare: bad LDA transform");
    const bool plda = plda_transform || plda_mean || plda_psi;
    if (plda && !(plda_transform && plda_mean && plda_psi)) return fail(XV_ERR_BAD_ARG, "backend_prepare: partial PLDA");
    if (!plda && (side == XV_SIDE_ENROL || side == XV_SIDE_TEST))
        return fail(XV_ERR_BAD_ARG, "backend_prepare: the enrolment / test sides need the PLDA");
    const long k = (side == XV_SIDE_ENROL || side == XV_SIDE_TEST) ? 2L * dim : dim;
    if (ldo < k || ldo % KSTEP) return fail(XV_ERR_BAD_ARG, "backend_prepare: ldo must be >= K and a multiple of XV_BACKEND_KSTEP");
    if (dim_in > 2048 || dim > PR_DMAX) return fail(XV_ERR_UNSUPPORTED, "backend_prepare: D <= 2048 and d <= 256 only");
    PrepParams p{x, (long)ldx, n_rows, dim_in, num_utts, mean, lda, (long)ld_lda, lda_offset, dim, length_norm ? 1 : 0,
                 plda_transform, plda_mean, plda_psi, side, out, (long)ldo, r};
    hipLaunchKernelGGL(backend_prepare_kernel, dim3((n_rows + PR_ROWS - 1) / PR_ROWS), dim3(PR_NT), 0, (hipStream_t)stream, p);
    return launch_status("backend_prepare_kernel");
}

extern "C" int xv_score_matrix_f32(const float *e, const float *t, int64_t ldk, int kpad, int n_enrol, int n_test, const float *r,
                                   float *scores, int64_t ld_scores, void *stream)
{
    if (n_enrol <= 0 || n_test <= 0) return 0;
    if (!e || !t || !scores || kpad <= 0 || kpad % KSTEP || ldk < kpad || ldk % 4 || ld_scores < n_test ||
        (((uintptr_t)e | (uintptr_t)t) & 15))
        return fail(XV_ERR_BAD_ARG, "score_matrix: bad argument");
    if (kpad > 1024) return fail(XV_ERR_UNSUPPORTED, "score_matrix: K <= 1024 only");
    const long gy = ((long)n_enrol + SM_BM - 1) / SM_BM;
    if (gy > 65535) return fail(XV_ERR_UNSUPPORTED, "score_matrix: too many enrolment rows for one launch");
    hipLaunchKernelGGL(score_matrix_kernel, dim3((n_test + SM_BN - 1) / SM_BN, (unsigned)gy), dim3(SM_NT), 0, (hipStream_t)stream, e, t,
                       (int)ldk, kpad, n_enrol, n_test, r, scores, (long)ld_scores);
    return launch_status("score_matrix_kernel");
}

extern "C" int xv_score_blocks_f32(const float *e, const float *t, int64_t ldk, int kpad, int n_rows, const float *r,
                                   const int32_t *grp_row0, const int64_t *grp_score0, int n_groups, int max_n, float *scores,
                                   int64_t scores_elems, int32_t *status, void *stream)
{
    if (!e || !t || !grp_row0 || !grp_score0 || !scores || !status || n_groups < 1 || max_n < 1 || n_rows < 1 || scores_elems < 1)
        return fail(XV_ERR_BAD_ARG, "score_blocks: NULL pointer, or n_groups, max_n, n_rows or scores_elems below 1");
    if (kpad <= 0 || kpad % KSTEP || ldk < kpad || ldk % 4 || (((uintptr_t)e | (uintptr_t)t | (uintptr_t)scores) & 15) ||
        ((uintptr_t)grp_row0 & 3) || ((uintptr_t)grp_score0 & 7) || ((uintptr_t)status & 3))
        return fail(XV_ERR_BAD_ARG, "score_blocks: bad argument");
    if (kpad > 1024) return fail(XV_ERR_UNSUPPORTED, "score_blocks: K <= 1024 only");
    const long tiles = ((long)max_n + SM_BM - 1) / SM_BM;
    if (tiles * tiles > 0x7fffffffL) return fail(XV_ERR_UNSUPPORTED, "score_blocks: max_n too large for one launch");
    for (int g0 = 0; g0 < n_groups; g0 += 65535) {                   // grid.y holds at most 65535 groups
        const int ng = n_groups - g0 < 65535 ? n_groups - g0 : 65535;
        hipLaunchKernelGGL(score_blocks_kernel, dim3((unsigned)(tiles * tiles), (unsigned)ng), dim3(SM_NT), 0, (hipStream_t)stream, e, t,
                           (int)ldk, kpad, n_rows, r, grp_row0, grp_score0, g0, max_n, scores, (long)scores_elems, status);
        if (const int rc = launch_status("score_blocks_kernel")) return rc;
    }
    return 0;
}

extern "C" int xv_score_pairs_f32(const float *e, const float *t, int64_t ldk, int kpad, const int32_t *e_idx, const int32_t *t_idx,
                                  int64_t n_trials, const float *r, float *scores, void *stream)
{
    if (n_trials <= 0) return 0;
    if (!e || !t || !e_idx || !t_idx || !scores || kpad <= 0 || kpad % KSTEP || ldk < kpad || ldk % 4 ||
        (((uintptr_t)e | (uintptr_t)t) & 15))
        return fail(XV_ERR_BAD_ARG, "score_pairs: bad argument");
    if (kpad > 1024) return fail(XV_ERR_UNSUPPORTED, "score_pairs: K <= 1024 only");
    const long g = (n_trials + 255) / 256;
    if (g > 0x7fffffffL) return fail(XV_ERR_UNSUPPORTED, "score_pairs: too many trials for one launch");
    hipLaunchKernelGGL(score_pairs_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, e, t, (int)ldk, kpad, e_idx, t_idx,
                       (long)n_trials, r, scores);
    return launch_status("score_pairs_kernel");
}

extern "C" int xv_topk_row_stats_f32(const float *scores, int64_t ld, int n_rows, int n_cols, int top_n, float *mean, float *std,
                                     void *stream)
{
    if (n_rows <= 0) return 0;
    if (!scores || !mean || !std || n_cols < 1 || top_n < 1 || top_n > n_cols || ld < n_cols || ld % 4 || ((uintptr_t)scores & 15))
        return fail(XV_ERR_BAD_ARG, "topk_row_stats: bad argument (1 <= top_n <= n_cols <= ld, ld a multiple of 4, 16-B aligned base)");
    using tk_t = decltype(&topk_row_stats_kernel);
    static const tk_t kerns[1] = {topk_row_stats_kernel};
    static std::atomic<unsigned long long> lds_done{0};
    if (const int rc = opt_in_dynamic_lds(lds_done, kerns, TK_LDS_MAX)) return rc;
    const size_t lds = TK_HDR + (n_cols <= TK_STAGE_MAX ? 4 * (size_t)((n_cols + 3) & ~3) : 0);
    hipLaunchKernelGGL(topk_row_stats_kernel, dim3((unsigned)n_rows), dim3(TK_NT), lds, (hipStream_t)stream, scores, (long)ld, n_cols,
                       top_n, mean, std);
    return launch_status("topk_row_stats_kernel");
}
