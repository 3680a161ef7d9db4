// xv_pca.hip -- per-recording PCA and the PLDA projected into it, for diarization on the MI355X.
//
// ivector-plda-scoring-dense --target-energy: every recording estimates a PCA on its own vectors, keeps the leading directions that
// hold target_energy of the variance, projects the PLDA model into that subspace and diagonalises it again.  The rule is fixed in
// include/xvector_hip.h.  The work is a ragged batch of independent, small, dense fp64 eigenproblems (d <= 128), one workgroup per
// recording, every recording resident at once -- the shape of ahc_batch_kernel (xv_cluster.hip).
//
//   pca_plda_kernel        group blockIdx.x, all phases between s_barriers:
//                          covariance C (fp64, rows ascending) -> LDS; cyclic Jacobi on C; eigenvalues sorted, the energy rule picks
//                          p; A = the first p eigenvectors as rows; W_g = A W A^T, B_g = A B A^T; Cholesky of W_g and T1 = its
//                          inverse, in LDS; S = T1 B_g T1^T; cyclic Jacobi on S; P_g = V^T T1, M_g = P_g A, c_g = -P_g (A mu).
//   prepare_groups_kernel  z = M_g y + c_g in fp32 (an fmaf chain per element), Plda::TransformIvector's scaling with psi_g, p_g and one
//                          utterance, the enrolment / test operand rows of the scorers with exact zeros past 2 p_g.
//
// The Jacobi iteration (jacobi_eig, one device function for both eigenproblems) holds the n x n iterate in LDS -- 128 x 129 doubles are
// 129 KiB of gfx950's 160 KiB; the row stride is odd, so a column is as free of bank conflicts as a row -- and the accumulated
// eigenvectors, as rows, in the group's workspace slice, where a rotation touches two contiguous rows.  The rotation order is a
// round-robin tournament (the circle method): n - 1 steps (n for odd n, one index sitting out) of n / 2 disjoint rotations, which are
// applied together: J^T A J with J their product.  One thread owns the 2 x 2 block (rows of pair k) x (columns of pair l), k <= l,
// and writes its mirror image too, so the iterate stays exactly symmetric and is updated in place behind one barrier.  The
// convergence test at the head of every sweep is max |a_ij| <= 2^-58 max |a_ii| (a maximum: no summation order), and the sweep
// count is capped at XV_PCA_MAX_SWEEPS.  Every value has one writer and every sum one order, so a group's bits depend on its own
// values, dim and target_energy alone.  No floating-point atomics, no cooperative launch, no workgroup waits on another.
#include "xv_device.h"

#include <cmath>

namespace {

constexpr int PCA_MAXD = XV_PCA_MAX_DIM;
constexpr double PCA_TOL = 0x1p-58;          // converged: max off-diagonal <= PCA_TOL * max diagonal (both in magnitude)
constexpr int PCA_U = 4;                     // covariance cells per thread whose row loops run together
constexpr int PCA_VU = 8;                    // eigenvector cells per thread whose loads are in flight together (latency bounds a step)

struct PcaLds {                              // in front of the matrix
    double red[2 * 16 + 2];                  // wave maxima (off-diagonal, diagonal)
    double rot[3 * (PCA_MAXD / 2)];          // c, s, t of a step's rotations
    double ev[PCA_MAXD];                     // eigenvalues / the Cholesky diagonal
    double vec[PCA_MAXD];                    // the mean of the rows; scratch of the sort
    double mu[PCA_MAXD];                     // mu_g = A mu
    int perm[PCA_MAXD];
    int pq[PCA_MAXD];                        // p, q of a step's pairs
    int flag[4];                             // [0] p, [1] info, [2] eigvals written
};

__host__ __device__ inline int pca_m(int n) { return (n + 1) & ~1; }                 // players of the tournament
__host__ __device__ inline int pca_ld(int n) { return pca_m(n) + 1; }                // odd row stride of the LDS matrix
inline size_t pca_lds_bytes(int dim) { return sizeof(PcaLds) + (size_t)pca_m(dim) * pca_ld(dim) * sizeof(double); }
inline int pca_threads(int dim) { return dim <= 32 ? 256 : dim <= 64 ? 512 : 1024; }
__host__ __device__ inline size_t pca_group_doubles(int dim) { return 4 * (size_t)dim * dim; }           // the workspace slice of one group

struct PcaParams {
    const float *y; long ldy; int n_rows;
    const int32_t *grp_row0; int dim; double target_energy;
    const double *mean, *within, *between, *transform, *psi;
    int32_t *grp_dim, *grp_info; double *eigvals, *pca, *grp_psi, *grp_map, *grp_off; int32_t *status;
    double *workspace;
};

// the larger of two magnitudes; a NaN, once seen, stays
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// pair k of step r of the round-robin over m players (m even): the circle method, player m - 1 fixed.  p < q.
__device__ __forceinline__ void rr_pair(int m, int r, int k, int &p, int &q)
{
    int a = m - 1, b = r;
    if (k) {
        a = (r + k) % (m - 1);
        b = (r + m - 1 - k) % (m - 1);
    }
    p = min(a, b);
    q = max(a, b);
}

// Eigenpairs of the symmetric n x n matrix A (LDS, row stride ld = pca_ld(n); for odd n the caller's matrix has room for the row and
// column n, zeroed here): on return the diagonal holds the eigenvalues and row i of Vt (global, n x n) the eigenvector of a_ii.
// Returns whether the test of convergence held within XV_PCA_MAX_SWEEPS sweeps; every thread returns the same value.  The caller
// places a barrier between its last write to A and this call.
__device__ bool jacobi_eig(double *A, int n, double *Vt, PcaLds &s)
{
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = NT >> 6;
    const int m = pca_m(n), ld = pca_ld(n), half = m >> 1;
    for (int f = tid; f < n * n; f += NT) Vt[f] = (f / n == f % n) ? 1.0 : 0.0;
    if (m > n)
        for (int f = tid; f < m; f += NT) A[f * ld + n] = A[n * ld + f] = 0.0;
    __syncthreads();
    // the k <= l blocks of a step, rows k and half - 1 - k folded into one row of half + 1 cells.  A thread's cells of both update
    // loops are f = tid, tid + NT, ...: their (row, column) advance by a fixed step, so the loops divide nothing.
    const int fold_rows = (half + 1) >> 1, fold_w = half + 1;
    const int b_r0 = tid / fold_w, b_c0 = tid % fold_w, b_dr = NT / fold_w, b_dc = NT % fold_w;
    const int v_k0 = tid / n, v_j0 = tid % n, v_dk = NT / n, v_dj = NT % n;
    bool converged = false;
    for (int sweep = 0; sweep <= XV_PCA_MAX_SWEEPS; ++sweep) {
        double off = 0.0, dg = 0.0;
        for (int i = v_k0, j = v_j0; i < n;) {
            const double a = fabs(A[i * ld + j]);
            if (i == j) dg = nan_max(dg, a);
            else off = nan_max(off, a);
            i += v_dk;
            j += v_dj;
            if (j >= n) {
                j -= n;
                ++i;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            off = nan_max(off, __shfl_xor(off, o, 64));
            dg = nan_max(dg, __shfl_xor(dg, o, 64));
        }
        if (lane == 0) {
            s.red[2 * wave] = off;
            s.red[2 * wave + 1] = dg;
        }
        __syncthreads();
        off = dg = 0.0;
        for (int w = 0; w < nw; ++w) {
            off = nan_max(off, s.red[2 * w]);
            dg = nan_max(dg, s.red[2 * w + 1]);
        }
        if (off <= PCA_TOL * dg) {                               // false for a NaN
            converged = true;
            break;
        }
        if (sweep == XV_PCA_MAX_SWEEPS || off != off || dg != dg) break;
        for (int r = 0; r < m - 1; ++r) {
            // (1) the step's pairs, and their rotations from the pivots a_pp, a_qq, a_pq
            if (tid < half) {
                int p, q;
                rr_pair(m, r, tid, p, q);
                double c = 1.0, sn = 0.0, t = 0.0;
                const double apq = A[p * ld + q];
                if (q < n && apq != 0.0) {
                    const double theta = (A[q * ld + q] - A[p * ld + p]) / (2.0 * apq);
                    t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    sn = t * c;
                }
                s.rot[3 * tid] = c;
                s.rot[3 * tid + 1] = sn;
                s.rot[3 * tid + 2] = t;
                s.pq[2 * tid] = p;
                s.pq[2 * tid + 1] = q;
            }
            __syncthreads();
            // (2a) A <- J^T A J, block (k, l) and its mirror by one thread
            for (int rr = b_r0, cc = b_c0; rr < fold_rows;) {
                int k, l;
                bool on = true;
                if (cc < half - rr) {
                    k = rr;
                    l = rr + cc;
                } else {
                    k = half - 1 - rr;
                    l = k + cc - (half - rr);
                    on = k != rr;                                // odd half: the middle row is not folded
                }
                rr += b_dr;
                cc += b_dc;
                if (cc >= fold_w) {
                    cc -= fold_w;
                    ++rr;
                }
                if (!on) continue;
                const double ck = s.rot[3 * k], sk = s.rot[3 * k + 1], cl = s.rot[3 * l], sl = s.rot[3 * l + 1];
                if (sk == 0.0 && sl == 0.0) continue;
                const int pk = s.pq[2 * k], qk = s.pq[2 * k + 1], pl = s.pq[2 * l], ql = s.pq[2 * l + 1];
                if (k == l) {
                    const double tpq = s.rot[3 * k + 2] * A[pk * ld + qk];
                    A[pk * ld + pk] -= tpq;
                    A[qk * ld + qk] += tpq;
                    A[pk * ld + qk] = A[qk * ld + pk] = 0.0;
                    continue;
                }
                const double a00 = A[pk * ld + pl], a01 = A[pk * ld + ql], a10 = A[qk * ld + pl], a11 = A[qk * ld + ql];
                const double r00 = ck * a00 - sk * a10, r01 = ck * a01 - sk * a11;          // rows: J_k^T
                const double r10 = sk * a00 + ck * a10, r11 = sk * a01 + ck * a11;
                const double b00 = cl * r00 - sl * r01, b01 = sl * r00 + cl * r01;          // columns: J_l
                const double b10 = cl * r10 - sl * r11, b11 = sl * r10 + cl * r11;
                A[pk * ld + pl] = A[pl * ld + pk] = b00;
                A[pk * ld + ql] = A[ql * ld + pk] = b01;
                A[qk * ld + pl] = A[pl * ld + qk] = b10;
                A[qk * ld + ql] = A[ql * ld + qk] = b11;
            }
            // (2b) Vt <- J^T Vt: rows p and q of the eigenvectors (global memory: the loads of PCA_VU cells are issued together,
            //      then their stores)
            for (int k = v_k0, j = v_j0; k < half;) {
                double c[PCA_VU], sn[PCA_VU], vp[PCA_VU], vq[PCA_VU];
                int ip[PCA_VU], iq[PCA_VU];
#pragma unroll
                for (int u = 0; u < PCA_VU; ++u) {
                    const bool on = k < half;
                    const int kk = on ? k : 0;
                    c[u] = s.rot[3 * kk];
                    sn[u] = on ? s.rot[3 * kk + 1] : 0.0;
                    ip[u] = s.pq[2 * kk] * n + j;
                    iq[u] = s.pq[2 * kk + 1] * n + j;
                    if (sn[u] != 0.0) {                          // a pair that sits out has sn = 0: its q is never addressed
                        vp[u] = Vt[ip[u]];
                        vq[u] = Vt[iq[u]];
                    }
                    k += v_dk;
                    j += v_dj;
                    if (j >= n) {
                        j -= n;
                        ++k;
                    }
                }
#pragma unroll
                for (int u = 0; u < PCA_VU; ++u) {
                    if (sn[u] != 0.0) {
                        Vt[ip[u]] = c[u] * vp[u] - sn[u] * vq[u];
                        Vt[iq[u]] = sn[u] * vp[u] + c[u] * vq[u];
                    }
                }
            }
            __syncthreads();
        }
    }
    return converged;
}

// s.ev[0, n) = the diagonal of A sorted descending, ties to the smaller index; s.perm[r] = the index that took rank r
__device__ void sort_eigenvalues(const double *A, int n, PcaLds &s)
{
    const int tid = threadIdx.x, ld = pca_ld(n);
    if (tid < n) s.vec[tid] = A[tid * ld + tid];
    __syncthreads();
    if (tid < n) {
        const double v = s.vec[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double w = s.vec[j];
            rank += (w > v || (w == v && j < tid)) ? 1 : 0;
        }
        s.perm[rank] = tid;
        s.ev[rank] = v;
    }
    __syncthreads();
}

// dst row r (r < rows, row stride ldd) = row perm[r] of Vt (n x n), its sign chosen so that its first component of largest
// magnitude is positive.  One wave per row.
__device__ void copy_rows_sorted(double *dst, int ldd, const double *Vt, int n, int rows, const PcaLds &s)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int r = wave; r < rows; r += nw) {
        const double *src = Vt + (long)s.perm[r] * n;
        double best = -1.0;
        int at = n;
        for (int j = lane; j < n; j += 64) {
            const double a = fabs(src[j]);
            if (a > best) {
                best = a;
                at = j;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(at, o, 64);
            if (ob > best || (ob == best && oa < at)) {
                best = ob;
                at = oa;
            }
        }
        const double sign = (at < n && src[at] < 0.0) ? -1.0 : 1.0;
        for (int j = lane; j < n; j += 64) dst[(long)r * ldd + j] = sign * src[j];
    }
}

// C[i, j] = sum_k X[i, k] * (trans ? Y[j, k] : Y[k, j]), i < m, j < n, k ascending from a zero start.  sym: only i <= j is
// computed and the cell is written to (j, i) as well.  The pointers may be LDS or global.
__device__ void mat_mul(double *C, int ldc, const double *X, int ldx, const double *Y, int ldy, int m, int n, int kk, bool trans,
                        bool sym)
{
    for (int f = threadIdx.x; f < m * n; f += blockDim.x) {
        const int i = f / n, j = f - i * n;
        if (sym && i > j) continue;
        const double *x = X + (long)i * ldx;
        double acc = 0.0;
        if (trans) {
            const double *yv = Y + (long)j * ldy;
            for (int k = 0; k < kk; ++k) acc = fma(x[k], yv[k], acc);
        } else {
            for (int k = 0; k < kk; ++k) acc = fma(x[k], Y[(long)k * ldy + j], acc);
        }
        C[(long)i * ldc + j] = acc;
        if (sym) C[(long)j * ldc + i] = acc;
    }
}

// out[i] = -(sum_k M[i, k] v[k]), i < m: rounded products added in order k ascending from a zero start (no fused multiply-add)
__device__ void neg_mat_vec(double *out, const double *M, int ldm, const double *v, int m, int kk)
{
#pragma clang fp contract(off)
    for (int i = threadIdx.x; i < m; i += blockDim.x) {
        double acc = 0.0;
        for (int k = 0; k < kk; ++k) {
            const double prod = M[(long)i * ldm + k] * v[k];
            acc = acc + prod;
        }
        out[i] = -acc;
    }
}

// The group's model.  Returns 0 with s.flag[0] = p, s.ev = the PCA eigenvalues, and As (p x d), psi_g, M_g, c_g written to their
// outputs; or the reason of the fallback (1 energy, 2 no convergence) with none of the outputs written.
__device__ int pca_plda_group(const PcaParams &P, long row0, int n, double *A, double *ws, PcaLds &s, double *out_psi, double *out_map,
                              double *out_off)
{
    const int tid = threadIdx.x, NT = blockDim.x, d = P.dim;
    const int ld = pca_ld(d);
    const float *y = P.y + row0 * P.ldy;
    double *Vt = ws, *As = ws + (size_t)d * d, *X1 = As + (size_t)d * d, *X2 = X1 + (size_t)d * d;
    // ---- 1. covariance: C = (1/n) sum y y^T - m m^T, rows ascending ----
    for (int j = tid; j < d; j += NT) {
        double acc = 0.0;
        for (int r = 0; r < n; ++r) acc += (double)y[r * P.ldy + j];
        s.vec[j] = acc / n;
    }
    __syncthreads();
    for (int f0 = tid; f0 < d * d; f0 += NT * PCA_U) {
        int ci[PCA_U], cj[PCA_U];
        double acc[PCA_U];
#pragma unroll
        for (int u = 0; u < PCA_U; ++u) {
            const int f = min(f0 + u * NT, d * d - 1);
            ci[u] = f / d;
            cj[u] = f - ci[u] * d;
            acc[u] = 0.0;
        }
        for (int r = 0; r < n; ++r) {
            const float *yr = y + r * P.ldy;
#pragma unroll
            for (int u = 0; u < PCA_U; ++u) acc[u] = fma((double)yr[ci[u]], (double)yr[cj[u]], acc[u]);
        }
#pragma unroll
        for (int u = 0; u < PCA_U; ++u)
            if (f0 + u * NT < d * d) A[ci[u] * ld + cj[u]] = acc[u] / n - s.vec[ci[u]] * s.vec[cj[u]];
    }
    __syncthreads();
    if (tid == 0) {
        double tr = 0.0;
        for (int i = 0; i < d; ++i) tr += A[i * ld + i];
        s.flag[1] = (isfinite(tr) && tr > 0.0) ? 0 : 1;
    }
    __syncthreads();
    if (s.flag[1]) return 1;
    // ---- 2. eigenpairs, descending ----
    if (!jacobi_eig(A, d, Vt, s)) return 2;
    sort_eigenvalues(A, d, s);
    for (int i = tid; i < d; i += NT) P.eigvals[(long)blockIdx.x * d + i] = s.ev[i];
    // ---- 3. the energy rule ----
    if (tid == 0) {
        s.flag[2] = 1;
        double total = 0.0;
        for (int i = 0; i < d; ++i) total += s.ev[i];
        int info = 0, p = d;
        if (!(isfinite(total) && total > 0.0)) {
            info = 1;
        } else {
            double cum = 0.0;
            int k = d;
            for (int i = 0; i < d; ++i) {
                cum += s.ev[i];
                if (cum / total > P.target_energy) {
                    k = i + 1;
                    break;
                }
            }
            p = min(k + 1, d);
        }
        s.flag[0] = p;
        s.flag[1] = info;
    }
    __syncthreads();
    if (s.flag[1]) return 1;
    const int p = s.flag[0], lp = pca_ld(p);
    // ---- 4. A = the first p eigenvectors as rows, in the workspace and in LDS ----
    copy_rows_sorted(As, d, Vt, d, p, s);
    __syncthreads();
    for (int f = tid; f < p * d; f += NT) A[(f / d) * ld + f % d] = As[f];
    __syncthreads();
    // ---- 5. the projected model: W_g -> X1, B_g -> X2 (Vt is the scratch of the products) ----
    mat_mul(Vt, d, A, ld, P.within, d, p, d, d, false, false);
    __syncthreads();
    mat_mul(X1, p, Vt, d, A, ld, p, p, d, true, true);
    __syncthreads();
    mat_mul(Vt, d, A, ld, P.between, d, p, d, d, false, false);
    __syncthreads();
    mat_mul(X2, p, Vt, d, A, ld, p, p, d, true, true);
    for (int i = tid; i < p; i += NT) {                          // mu_g = A mu
        double acc = 0.0;
        for (int k = 0; k < d; ++k) acc = fma(A[i * ld + k], P.mean[k], acc);
        s.mu[i] = acc;
    }
    __syncthreads();
    // Cholesky W_g = L L^T in LDS (lower triangle, the diagonal of L in s.ev from here on), then T1 = L^-1 in place
    for (int f = tid; f < p * p; f += NT) A[(f / p) * lp + f % p] = X1[f];
    __syncthreads();
    bool bad = false;
    for (int j = 0; j < p; ++j) {
        const double ajj = A[j * lp + j];
        if (!(ajj > 0.0) || !isfinite(ajj)) {                    // uniform: every thread reads the same cell
            bad = true;
            break;
        }
        const double ljj = sqrt(ajj);
        if (tid == 0) s.ev[j] = ljj;
        for (int i = j + 1 + tid; i < p; i += NT) A[i * lp + j] /= ljj;
        __syncthreads();
        const int rem = p - j - 1;
        for (int f = tid; f < rem * rem; f += NT) {
            const int i = j + 1 + f / rem, k = j + 1 + f % rem;
            if (k <= i) A[i * lp + k] -= A[i * lp + j] * A[k * lp + j];
        }
        __syncthreads();
    }
    if (bad) return 2;
    // X L = I, column j from the last to the first: x_ij = -(sum_{j < k <= i} x_ik l_kj) / l_jj, the column of L staged first
    double *col = s.rot;                                         // PCA_MAXD doubles fit (3 * PCA_MAXD / 2)
    for (int j = p - 1; j >= 0; --j) {
        for (int k = j + 1 + tid; k < p; k += NT) col[k] = A[k * lp + j];
        __syncthreads();
        const double ljj = s.ev[j];
        for (int i = j + tid; i < p; i += NT) {
            if (i == j) {
                A[j * lp + j] = 1.0 / ljj;
            } else {
                double acc = 0.0;
                for (int k = j + 1; k <= i; ++k) acc = fma(A[i * lp + k], col[k], acc);      // x_ii = 1 / l_ii since step i
                A[i * lp + j] = -acc / ljj;
            }
        }
        __syncthreads();
    }
    for (int f = tid; f < p * p; f += NT) {                      // the upper triangle of the LDS matrix still holds W_g: zero it
        const int i = f / p, k = f - i * p;
        if (k > i) A[i * lp + k] = 0.0;
    }
    __syncthreads();
    for (int f = tid; f < p * p; f += NT) X1[f] = A[(f / p) * lp + f % p];              // T1 -> X1
    mat_mul(Vt, p, A, lp, X2, p, p, p, p, false, false);        // T1 B_g
    __syncthreads();
    mat_mul(X2, p, Vt, p, A, lp, p, p, p, true, true);          // S = (T1 B_g) T1^T -> X2 (B_g is done with)
    __syncthreads();
    for (int f = tid; f < p * p; f += NT) A[(f / p) * lp + f % p] = X2[f];
    __syncthreads();
    if (!jacobi_eig(A, p, X2, s)) return 2;
    sort_eigenvalues(A, p, s);
    copy_rows_sorted(Vt, p, X2, p, p, s);                        // V^T, sorted
    __syncthreads();
    mat_mul(X2, p, Vt, p, X1, p, p, p, p, false, false);        // P_g = V^T T1
    __syncthreads();
    mat_mul(out_map, d, X2, p, As, d, p, d, p, false, false);   // M_g = P_g A
    neg_mat_vec(out_off, X2, p, s.mu, p, p);                     // c_g = -P_g mu_g
    for (int i = tid; i < p; i += NT) out_psi[i] = fmax(s.ev[i], 0.0);
    return 0;
}

__global__ __launch_bounds__(1024) void pca_plda_kernel(const PcaParams P)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    PcaLds &s = *reinterpret_cast<PcaLds *>(lds_raw);
    double *A = reinterpret_cast<double *>(lds_raw + sizeof(PcaLds));
    const int g = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, d = P.dim;
    const long row0 = P.grp_row0[g], n = (long)P.grp_row0[g + 1] - row0;
    if (n < 1 || row0 < 0 || row0 + n > P.n_rows) {              // uniform over the workgroup
        if (tid == 0) *P.status = 1;
        return;
    }
    if (tid == 0) s.flag[2] = 0;                                 // ordered before its readers by the barriers of the covariance
    double *ws = P.workspace + (size_t)g * pca_group_doubles(d);
    double *out_psi = P.grp_psi + (long)g * d, *out_map = P.grp_map + (long)g * d * d, *out_off = P.grp_off + (long)g * d;
    const int info = pca_plda_group(P, row0, (int)n, A, ws, s, out_psi, out_map, out_off);
    __syncthreads();
    if (info == 0) {
        const int p = s.flag[0];
        if (P.pca) {
            const double *As = ws + (size_t)d * d;
            for (int f = tid; f < p * d; f += NT) P.pca[(long)g * d * d + f] = As[f];
        }
        if (tid == 0) {
            P.grp_dim[g] = p;
            P.grp_info[g] = 0;
        }
        return;
    }
    // the fallback: the global model as it is, the identity as the PCA
    for (int f = tid; f < d * d; f += NT) {
        out_map[f] = P.transform[f];
        if (P.pca) P.pca[(long)g * d * d + f] = (f / d == f % d) ? 1.0 : 0.0;
    }
    for (int i = tid; i < d; i += NT) out_psi[i] = P.psi[i];
    neg_mat_vec(out_off, P.transform, d, P.mean, d, d);
    // eigvals: the PCA's eigenvalues when its iteration converged (written there), else zeros
    if (s.flag[2] == 0)
        for (int i = tid; i < d; i += NT) P.eigvals[(long)g * d + i] = 0.0;
    if (tid == 0) {
        P.grp_dim[g] = d;
        P.grp_info[g] = info;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the grouped twin of backend_prepare_kernel's PLDA stage
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int PG_ROWS = 16;                  // rows of one group per workgroup
constexpr int PG_NT = 256;
constexpr int PG_LD = PCA_MAXD + 1;

struct PrepGroupsParams {
    const float *y; long ldy; int n_rows;
    const int32_t *grp_row0; int g0, max_n, dim;
    const int32_t *grp_dim; const double *grp_psi, *grp_map, *grp_off;
    int side; float *out; long ldo; float *r; int32_t *status;
};

__device__ __forceinline__ float wave_sum_f(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// workgroup (row block, group): rows [blockIdx.x * PG_ROWS, ...) of group g0 + blockIdx.y
__global__ __launch_bounds__(PG_NT) void prepare_groups_kernel(const PrepGroupsParams P)
{
    __shared__ float ys[PG_ROWS * PG_LD];
    __shared__ float zs[PG_ROWS * PG_LD];
    __shared__ float psis[PCA_MAXD];
    const int g = P.g0 + blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = P.dim;
    const long row0 = P.grp_row0[g], n = (long)P.grp_row0[g + 1] - row0;
    const int p = P.grp_dim[g];
    if (n < 1 || n > P.max_n || row0 < 0 || row0 + n > P.n_rows || p < 1 || p > d) {
        if (blockIdx.x == 0 && tid == 0) *P.status = 1;
        return;
    }
    const long b0 = (long)blockIdx.x * PG_ROWS;
    if (b0 >= n) return;
    const int nr = (int)min((long)PG_ROWS, n - b0);
    const double *M = P.grp_map + (long)g * d * d, *c = P.grp_off + (long)g * d, *psi = P.grp_psi + (long)g * d;
    for (int f = tid; f < PG_ROWS * d; f += PG_NT) {
        const int rr = f / d, k = f - rr * d;
        ys[rr * PG_LD + k] = rr < nr ? P.y[(row0 + b0 + rr) * P.ldy + k] : 0.0f;
    }
    if (tid < p) psis[tid] = (float)psi[tid];
    __syncthreads();
    // z[rr, i] = sum_k (float)M[i, k] y[rr, k] (fmaf, k ascending from 0) + (float)c[i]: 16 lanes share one row of M
    const int rr = tid % PG_ROWS;
    for (int i = tid / PG_ROWS; i < p; i += PG_NT / PG_ROWS) {
        const double *mi = M + (long)i * d;
        float acc = 0.0f;
        for (int k = 0; k < d; ++k) acc = fmaf((float)mi[k], ys[rr * PG_LD + k], acc);
        zs[rr * PG_LD + i] = acc + (float)c[i];
    }
    __syncthreads();
    for (int q = wave; q < nr; q += PG_NT / 64) {
        float *z = zs + q * PG_LD;
        float sq = 0.0f;
        for (int i = lane; i < p; i += 64) sq += z[i] * z[i] / (psis[i] + 1.0f);
        sq = wave_sum_f(sq);
        const float scale = sq > 0.0f ? sqrtf((float)p / sq) : 1.0f;
        const long row = row0 + b0 + q;
        float *o = P.out + row * P.ldo;
        float rv = 0.0f;
        if (P.side == XV_SIDE_ENROL) {
            for (int i = lane; i < p; i += 64) {
                const float zi = z[i] * scale, ps = psis[i];
                const float a = ps / (ps + 1.0f);
                const float v = 1.0f + ps / (ps + 1.0f);
                const float w = 1.0f + ps;
                o[i] = a / v * zi;
                o[p + i] = 1.0f / v - 1.0f / w;
                rv += -0.5f * a * a * zi * zi / v + 0.5f * (logf(w) - logf(v));
            }
        } else {
            for (int i = lane; i < p; i += 64) {
                const float zi = z[i] * scale;
                o[i] = zi;
                o[p + i] = -0.5f * zi * zi;
            }
        }
        for (long k = 2 * p + lane; k < P.ldo; k += 64) o[k] = 0.0f;
        rv = wave_sum_f(rv);
        if (P.r && lane == 0) P.r[row] = rv;
    }
}

}  // namespace

extern "C" size_t xv_pca_plda_groups_workspace_bytes(int n_groups, int dim)
{
    if (n_groups < 1 || dim < 1 || dim > XV_PCA_MAX_DIM) return 0;
    return (size_t)n_groups * pca_group_doubles(dim) * sizeof(double);
}

extern "C" int xv_pca_plda_groups_f64(const float *y, int64_t ldy, int n_rows, const int32_t *grp_row0, int n_groups, int dim,
                                      double target_energy, const double *mean, const double *within, const double *between,
                                      const double *transform, const double *psi, int32_t *grp_dim, int32_t *grp_info, double *eigvals,
                                      double *pca, double *grp_psi, double *grp_map, double *grp_off, int32_t *status, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    if (n_groups < 1 || n_rows < 1 || dim < 1) return fail(XV_ERR_BAD_ARG, "pca_plda_groups: n_groups, n_rows and dim must be at least 1");
    if (dim > XV_PCA_MAX_DIM) return fail(XV_ERR_UNSUPPORTED, "pca_plda_groups: dim exceeds XV_PCA_MAX_DIM (128)");
    if (!(target_energy > 0.0 && target_energy <= 1.0))
        return fail(XV_ERR_BAD_ARG, "pca_plda_groups: target_energy must be in (0, 1]");
    if (!y || !grp_row0 || !mean || !within || !between || !transform || !psi || !grp_dim || !grp_info || !eigvals || !grp_psi ||
        !grp_map || !grp_off || !status)
        return fail(XV_ERR_BAD_ARG, "pca_plda_groups: NULL pointer");
    if (ldy < dim) return fail(XV_ERR_BAD_ARG, "pca_plda_groups: ldy must be at least dim");
    if ((((uintptr_t)y | (uintptr_t)grp_row0 | (uintptr_t)grp_dim | (uintptr_t)grp_info | (uintptr_t)status) & 3) ||
        (((uintptr_t)mean | (uintptr_t)within | (uintptr_t)between | (uintptr_t)transform | (uintptr_t)psi | (uintptr_t)eigvals |
          (uintptr_t)pca | (uintptr_t)grp_psi | (uintptr_t)grp_map | (uintptr_t)grp_off) & 7))
        return fail(XV_ERR_BAD_ARG, "pca_plda_groups: misaligned pointer (fp64 arrays and the workspace 8 bytes, the rest 4)");
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < xv_pca_plda_groups_workspace_bytes(n_groups, dim))
        return fail(XV_ERR_BAD_ARG,
                    "pca_plda_groups: the workspace is missing, misaligned or smaller than xv_pca_plda_groups_workspace_bytes");
    using k_t = decltype(&pca_plda_kernel);
    static const k_t kerns[1] = {pca_plda_kernel};
    static std::atomic<unsigned long long> lds_done{0};
    if (const int rc = opt_in_dynamic_lds(lds_done, kerns, (int)pca_lds_bytes(XV_PCA_MAX_DIM))) return rc;
    const PcaParams p{y, (long)ldy, n_rows, grp_row0, dim, target_energy, mean, within, between, transform, psi, grp_dim, grp_info,
                      eigvals, pca, grp_psi, grp_map, grp_off, status, static_cast<double *>(workspace)};
    hipLaunchKernelGGL(pca_plda_kernel, dim3((unsigned)n_groups), dim3(pca_threads(dim)), pca_lds_bytes(dim), (hipStream_t)stream, p);
    return launch_status("pca_plda_kernel");
}

extern "C" int xv_backend_prepare_groups_f32(const float *y, int64_t ldy, int n_rows, const int32_t *grp_row0, int n_groups, int max_n,
                                             int dim, const int32_t *grp_dim, const double *grp_psi, const double *grp_map,
                                             const double *grp_off, int side, float *out, int64_t ldo, float *r, int32_t *status,
                                             void *stream)
{
    if (n_groups < 1 || n_rows < 1 || max_n < 1 || dim < 1)
        return fail(XV_ERR_BAD_ARG, "backend_prepare_groups: n_groups, n_rows, max_n and dim must be at least 1");
    if (dim > XV_PCA_MAX_DIM) return fail(XV_ERR_UNSUPPORTED, "backend_prepare_groups: dim exceeds XV_PCA_MAX_DIM (128)");
    if (side != XV_SIDE_ENROL && side != XV_SIDE_TEST)
        return fail(XV_ERR_BAD_ARG, "backend_prepare_groups: only the enrolment and test sides are supported");
    if (!y || !grp_row0 || !grp_dim || !grp_psi || !grp_map || !grp_off || !out || !status)
        return fail(XV_ERR_BAD_ARG, "backend_prepare_groups: NULL pointer");
    if (ldy < dim || ldo < 2L * dim || ldo % XV_BACKEND_KSTEP)
        return fail(XV_ERR_BAD_ARG, "backend_prepare_groups: ldy >= dim, ldo >= 2 dim and a multiple of XV_BACKEND_KSTEP");
    if ((((uintptr_t)y | (uintptr_t)grp_row0 | (uintptr_t)grp_dim | (uintptr_t)out | (uintptr_t)r | (uintptr_t)status) & 3) ||
        (((uintptr_t)grp_psi | (uintptr_t)grp_map | (uintptr_t)grp_off) & 7))
        return fail(XV_ERR_BAD_ARG, "backend_prepare_groups: misaligned pointer (fp64 tables 8 bytes, the rest 4)");
    const unsigned blocks = (unsigned)(((long)max_n + PG_ROWS - 1) / PG_ROWS);
    for (int g0 = 0; g0 < n_groups; g0 += 65535) {                   // grid.y holds at most 65535 groups
        const int ng = n_groups - g0 < 65535 ? n_groups - g0 : 65535;
        const PrepGroupsParams p{y, (long)ldy, n_rows, grp_row0, g0, max_n, dim, grp_dim, grp_psi, grp_map, grp_off, side, out, (long)ldo,
                                 r, status};
        hipLaunchKernelGGL(prepare_groups_kernel, dim3(blocks, (unsigned)ng), dim3(PG_NT), 0, (hipStream_t)stream, p);
        if (const int rc = launch_status("prepare_groups_kernel")) return rc;
    }
    return 0;
}
