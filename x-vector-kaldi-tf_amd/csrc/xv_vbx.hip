// xv_vbx.hip -- VBx resegmentation of every recording's x-vector sequence on the MI355X.
//
// A variational-Bayes HMM over one recording's vectors (Landini et al., "Bayesian HMM clustering of x-vector sequences"): one state
// per speaker, speaker means under the PLDA's between-class prior, initialised from the clustering's labels; speakers the data do
// not support fade out.  The rule is fixed in include/xvector_hip.h.  The work is a ragged batch of independent small fp64
// problems, one workgroup (4 waves) per recording, every phase between s_barriers -- the shape of ahc_batch_kernel and
// pca_plda_kernel.
//
//   once        z = P (y - mu) by v_mfma_f64_16x16x4_f64 (16-row tiles of the recording dealt to the waves, a wave walks its
//               tile's column tiles in ascending order and sums z^2 on the way), rho = z * sqrt(Phi) and G into the workspace slice.
//   iteration   N_s (a wave per speaker); R = gamma^T rho by MFMA (the 16 x 16 output tiles dealt to the waves, each tile one chain
//               over t ascending: no partials to merge, the order does not depend on the wave count), alpha and 1 / L in the tile's
//               epilogue; the per-speaker terms (a wave per speaker); l = rho alpha^T by MFMA (k ascending), row maxima, b = exp;
//               the forward and backward chains in wave 0, lane s = speaker s: per step one butterfly sum (xor 1, 2, 4, ... below
//               the power of two that holds S) and one division, no exp / log; then ln c, the pi update and the stop rule.
//   at the end  argmax labels, gamma, pi.
//
// a / gamma, b, beta and c live in LDS when (3 S + 1) T doubles fit the launch's dynamic LDS, in the workspace slice otherwise: the
// same code on another pointer, the same bits.  No floating-point atomics, every value has one writer and every sum one order.
// The f64 MFMA's C/D layout is its own: lane l, register r holds D[(l >> 4) + 4 r][l & 15]; A and B are one f64 per lane,
// A[l & 15][k = l >> 4], B[k = l >> 4][l & 15].  Every MFMA sits in wave-uniform control flow; a guarded operand is a select.
#include "xv_device.h"

#include <cmath>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int VBX_NT = 256;                  // 4 waves
constexpr int VBX_NW = VBX_NT / 64;
constexpr int VBX_MAXS = XV_VBX_MAX_SPK;
constexpr size_t VBX_LDS_CAP = 96 * 1024;    // dynamic LDS of a launch at most: the chain arrays of T S <= ~4000
constexpr double VBX_LN_2PI = 1.8378770664093454835606594728112;

struct VbxLds {
    double pi[VBX_MAXS], ns[VBX_MAXS], q[VBX_MAXS], e2[VBX_MAXS], pacc[VBX_MAXS];
    double red[VBX_NW];
    double elbo_prev;
    int flag[4];                             // [0] stop, [1] info
};

__host__ __device__ inline int vbx_dp(int dim) { return (dim + 3) & ~3; }                       // row stride of rho, alpha, 1 / L
__host__ __device__ inline size_t vbx_row_doubles(int dim, int max_spk) { return (size_t)vbx_dp(dim) + 3 + 3 * (size_t)max_spk; }
__host__ __device__ inline size_t vbx_group_doubles(int dim, int max_spk) { return 2 * (size_t)max_spk * vbx_dp(dim); }
__host__ __device__ inline size_t vbx_chain_doubles(long T, int S) { return (3 * (size_t)S + 1) * (size_t)T; }

struct VbxParams {
    const float *y; long ldy; int n_rows;
    const int32_t *grp_row0; int dim;
    const int32_t *row_of_t, *init_label, *grp_spk; int max_spk;
    const double *mean, *transform, *psi;
    double fa, fb, loop_prob, smooth; int max_iters; double eps;
    int32_t *labels; double *gamma, *pi, *elbo; int32_t *grp_iters, *grp_info, *status;
    double *ws; size_t lds_doubles;
};

// the sum over the W lanes of a lane's aligned group (W a power of two, wave-uniform): xor 1, 2, 4, ...; every lane of the group
// ends with the same bits
__device__ __forceinline__ double group_sum(double v, int W)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
        if (o < W) v += __shfl_xor(v, o, 64);
    return v;
}

// one 16 x 16 output tile: sum over k = 0 .. 4 ksteps - 1 of a(row l & 15, k) b(k, column l & 15), k in ascending groups of 4
template <class FA, class FB>
__device__ __forceinline__ f64x4 mfma_tile(int ksteps, FA fa, FB fb)
{
    const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    int ks = 0;
    for (; ks + 4 <= ksteps; ks += 4) {
        double a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = fa(lr, 4 * (ks + u) + lk);
            b[u] = fb(4 * (ks + u) + lk, lr);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    for (; ks < ksteps; ++ks) {
        const double a = fa(lr, 4 * ks + lk), b = fb(4 * ks + lk, lr);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    return acc;
}

// One recording.  ch: (3 S + 1) T doubles for a / gamma, b, beta [T, S] and c [T] -- LDS or the workspace slice.
__device__ __forceinline__ void vbx_group(const VbxParams &P, int g, long row0, int T, int S, double *ws, double *ch, VbxLds &s)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
    const int D = P.dim, Dp = vbx_dp(D), ms = P.max_spk;
    const int32_t *rot = P.row_of_t ? P.row_of_t + row0 : nullptr;
    const int32_t *lab0 = P.init_label + row0;
    double *rho = ws, *G = rho + (size_t)T * Dp, *M = G + T;
    double *alpha = ws + (size_t)T * vbx_row_doubles(D, ms), *invl = alpha + (size_t)ms * Dp;
    double *A = ch, *B = A + (size_t)T * S, *BE = B + (size_t)T * S, *C = BE + (size_t)T * S;
    const double lp = P.loop_prob, q1 = 1.0 - P.loop_prob, ratio = P.fa / P.fb;
    const int ttiles = (T + 15) >> 4, stiles = (S + 15) >> 4, dtiles = (D + 15) >> 4;
    int W = 1;
    while (W < S) W <<= 1;
    auto row_of = [&](int t) -> long { return row0 + (rot ? rot[t] : t); };

    // ---- once: rho, G; the zero columns of rho and alpha past D; the initial gamma and pi ----
    if (Dp > D) {
        const int pad = Dp - D;
        for (long f = tid; f < (long)T * pad; f += VBX_NT) rho[(f / pad) * Dp + D + f % pad] = 0.0;
        for (int f = tid; f < S * pad; f += VBX_NT) alpha[(f / pad) * Dp + D + f % pad] = 0.0;
    }
    for (int tt = wave; tt < ttiles; tt += VBX_NW) {
        const int t0 = 16 * tt;
        const int ta = t0 + lr;                                  // the row of this lane's A operand
        const float *ya = P.y + row_of(ta < T ? ta : T - 1) * P.ldy;
        double zz[4] = {0.0, 0.0, 0.0, 0.0};
        for (int it = 0; it < dtiles; ++it) {
            const int i = 16 * it + lr;                          // this lane's output column, and the row of P of its B operand
            const double *pr = P.transform + (size_t)(i < D ? i : D - 1) * D;
            const f64x4 acc = mfma_tile(
                Dp >> 2, [&](int, int k) { return (ta < T && k < D) ? (double)ya[k] - P.mean[k] : 0.0; },
                [&](int k, int) { return (i < D && k < D) ? pr[k] : 0.0; });
            const double sq = i < D ? sqrt(P.psi[i]) : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = t0 + lk + 4 * r;
                if (t < T && i < D) {
                    rho[(size_t)t * Dp + i] = acc[r] * sq;
                    zz[r] = fma(acc[r], acc[r], zz[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double tot = group_sum(zz[r], 16);
            const int t = t0 + lk + 4 * r;
            if (lr == 0 && t < T) G[t] = -0.5 * (tot + D * VBX_LN_2PI);
        }
    }
    {
        const double es = exp(P.smooth), den = es + (double)(S - 1);
        const double hit = es / den, miss = 1.0 / den;
        for (long f = tid; f < (long)T * S; f += VBX_NT) {
            const int t = (int)(f / S), sp = (int)(f - (long)t * S);
            A[f] = lab0[row_of(t) - row0] == sp ? hit : miss;
        }
        if (tid < S) s.pi[tid] = 1.0 / S;
        if (tid == 0) {
            s.flag[0] = 0;
            s.flag[1] = 0;
            s.elbo_prev = 0.0;
        }
    }
    __syncthreads();

    int iters = 0;
    for (int it = 0; it < P.max_iters; ++it) {
        // (a) N_s = sum_t gamma_ts: a wave per speaker, lane partials over t = lane, lane + 64, ..., then the butterfly
        for (int sp = wave; sp < S; sp += VBX_NW) {
            double acc = 0.0;
            for (int t = lane; t < T; t += 64) acc += A[(size_t)t * S + sp];
            acc = group_sum(acc, 64);
            if (lane == 0) s.ns[sp] = acc;
        }
        __syncthreads();
        // (b) R = gamma^T rho, one chain over t per tile; alpha = ratio invL R, invL = 1 / (1 + ratio N_s Phi_d)
        for (int tile = wave; tile < stiles * dtiles; tile += VBX_NW) {
            const int s0 = 16 * (tile / dtiles), d0 = 16 * (tile % dtiles);
            const int sa = s0 + lr, db = d0 + lr;
            const f64x4 acc = mfma_tile(
                (T + 3) >> 2, [&](int, int k) { return (sa < S && k < T) ? A[(size_t)k * S + sa] : 0.0; },
                [&](int k, int) { return (db < D && k < T) ? rho[(size_t)k * Dp + db] : 0.0; });
            const double phi = db < D ? P.psi[db] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int sp = s0 + lk + 4 * r;
                if (sp < S && db < D) {
                    const double il = 1.0 / (1.0 + ratio * s.ns[sp] * phi);
                    invl[(size_t)sp * Dp + db] = il;
                    alpha[(size_t)sp * Dp + db] = ratio * il * acc[r];
                }
            }
        }
        __syncthreads();
        // (c) q_s = sum_d (invL + alpha^2) Phi_d, e2_s = sum_d (ln invL - invL - alpha^2 + 1): a wave per speaker
        for (int sp = wave; sp < S; sp += VBX_NW) {
            double q = 0.0, e = 0.0;
            for (int d = lane; d < D; d += 64) {
                const double il = invl[(size_t)sp * Dp + d], al = alpha[(size_t)sp * Dp + d];
                q += (il + al * al) * P.psi[d];
                e += log(il) - il - al * al + 1.0;
            }
            q = group_sum(q, 64);
            e = group_sum(e, 64);
            if (lane == 0) {
                s.q[sp] = q;
                s.e2[sp] = e;
            }
        }
        __syncthreads();
        // (d) l_ts = Fa (rho_t . alpha_s - q_s / 2 + G_t) -> B; row maxima -> M; b = exp(l - m) in place
        for (int tile = wave; tile < ttiles * stiles; tile += VBX_NW) {
            const int t0 = 16 * (tile / stiles), s0 = 16 * (tile % stiles);
            const int ta = t0 + lr, sb = s0 + lr;
            const double *ra = rho + (size_t)(ta < T ? ta : T - 1) * Dp, *ab = alpha + (size_t)(sb < S ? sb : S - 1) * Dp;
            const f64x4 acc = mfma_tile(
                Dp >> 2, [&](int, int k) { return ta < T ? ra[k] : 0.0; }, [&](int k, int) { return sb < S ? ab[k] : 0.0; });
            const double hq = sb < S ? 0.5 * s.q[sb] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = t0 + lk + 4 * r;
                if (t < T && sb < S) B[(size_t)t * S + sb] = P.fa * (acc[r] - hq + G[t]);
            }
        }
        __syncthreads();
        for (int t = tid; t < T; t += VBX_NT) {
            double m = B[(size_t)t * S];
            for (int sp = 1; sp < S; ++sp) m = fmax(m, B[(size_t)t * S + sp]);
            M[t] = m;
        }
        __syncthreads();
        for (long f = tid; f < (long)T * S; f += VBX_NT) B[f] = exp(B[f] - M[f / S]);
        __syncthreads();
        // (e) the chains: wave 0, lane s = speaker s
        if (wave == 0) {
            const bool on = lane < S;
            const int sl = on ? lane : 0;
            const double pis = on ? s.pi[sl] : 0.0;
            double a_prev = 0.0;
            double bn = on ? B[sl] : 0.0;
            for (int t = 0; t < T; ++t) {
                const double b = bn;
                if (t + 1 < T) bn = on ? B[(size_t)(t + 1) * S + sl] : 0.0;
                const double v = (t == 0 ? pis : lp * a_prev + q1 * pis) * b;
                const double c = group_sum(v, W);
                const double a = v / c;
                if (on) A[(size_t)t * S + sl] = a;
                if (lane == 0) C[t] = c;
                a_prev = a;
            }
            __threadfence_block();                               // c, written by lane 0, is read by every lane below
            double beta = 1.0;
            if (on) BE[(size_t)(T - 1) * S + sl] = 1.0;
            double bnx = (on && T > 1) ? B[(size_t)(T - 1) * S + sl] : 0.0, cn = T > 1 ? C[T - 1] : 1.0;
            double an = (on && T > 1) ? A[(size_t)(T - 2) * S + sl] : 0.0;
            for (int t = T - 2; t >= 0; --t) {
                const double w = bnx * beta, c = cn, a = an;
                if (t > 0) {
                    bnx = on ? B[(size_t)t * S + sl] : 0.0;
                    cn = C[t];
                    an = on ? A[(size_t)(t - 1) * S + sl] : 0.0;
                }
                const double sw = group_sum(pis * w, W);
                beta = (lp * w + q1 * sw) / c;
                if (on) {
                    BE[(size_t)t * S + sl] = beta;
                    A[(size_t)t * S + sl] = a * beta;            // gamma
                }
            }
        }
        __syncthreads();
        // (f) sum_t (ln c_t + m_t), c_t checked; per speaker sum_{t >= 1} b beta / c
        int bad = 0;
        {
            double acc = 0.0;
            for (int t = tid; t < T; t += VBX_NT) {
                const double c = C[t];
                if (!(isfinite(c) && c != 0.0)) bad = 1;
                acc += log(c) + M[t];
            }
            acc = group_sum(acc, 64);
            if (lane == 0) s.red[wave] = acc;
        }
        for (int sp = wave; sp < S; sp += VBX_NW) {
            double acc = 0.0;
            for (int t = lane; t < T; t += 64)
                if (t >= 1) acc += B[(size_t)t * S + sp] * BE[(size_t)t * S + sp] / C[t];
            acc = group_sum(acc, 64);
            if (lane == 0) s.pacc[sp] = acc;
        }
        bad = __syncthreads_or(bad);
        if (tid == 0) {
            double e1 = 0.0, e2 = 0.0, norm = 0.0;
            for (int w = 0; w < VBX_NW; ++w) e1 += s.red[w];
            for (int sp = 0; sp < S; ++sp) e2 += s.e2[sp];
            const double elbo = e1 + 0.5 * P.fb * e2;
            for (int sp = 0; sp < S; ++sp) {
                const double pn = A[sp] + q1 * s.pi[sp] * s.pacc[sp];
                s.pacc[sp] = pn;
                norm += pn;
            }
            if (bad || !isfinite(elbo) || !(isfinite(norm) && norm != 0.0)) {
                s.flag[1] = 2;
                s.flag[0] = 1;
            } else {
                for (int sp = 0; sp < S; ++sp) s.pi[sp] = s.pacc[sp] / norm;
                P.elbo[(size_t)g * P.max_iters + it] = elbo;
                if (it > 0 && elbo - s.elbo_prev < P.eps) s.flag[0] = 1;
                s.elbo_prev = elbo;
            }
        }
        __syncthreads();
        iters = it + 1;
        if (s.flag[0]) break;
    }

    // ---- outputs ----
    const int info = s.flag[1];
    if (info) {
        for (int t = tid; t < T; t += VBX_NT) P.labels[row0 + t] = lab0[t];
    } else {
        for (int t = tid; t < T; t += VBX_NT) {
            const double *gt = A + (size_t)t * S;
            double best = gt[0];
            int at = 0;
            for (int sp = 1; sp < S; ++sp)
                if (gt[sp] > best) {
                    best = gt[sp];
                    at = sp;
                }
            P.labels[row_of(t)] = at;
        }
        if (P.gamma)
            for (long f = tid; f < (long)T * S; f += VBX_NT) {
                const int t = (int)(f / S), sp = (int)(f - (long)t * S);
                P.gamma[(size_t)row_of(t) * ms + sp] = A[f];
            }
        if (tid < S) P.pi[(size_t)g * ms + tid] = s.pi[tid];
    }
    if (tid == 0) {
        P.grp_iters[g] = iters;
        P.grp_info[g] = info;
    }
}

__global__ __launch_bounds__(VBX_NT) void vbx_kernel(const VbxParams P)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    VbxLds &s = *reinterpret_cast<VbxLds *>(lds_raw);
    double *dyn = reinterpret_cast<double *>(lds_raw + sizeof(VbxLds));
    const int g = blockIdx.x, tid = threadIdx.x;
    const long row0 = P.grp_row0[g], n = (long)P.grp_row0[g + 1] - row0;
    const int S = P.grp_spk[g];
    int bad = n < 1 || row0 < 0 || row0 + n > P.n_rows || S < 1 || S > P.max_spk;        // uniform over the workgroup
    if (!bad) {
        for (long t = tid; t < n; t += VBX_NT) {
            const int l = P.init_label[row0 + t];
            if (l < 0 || l >= S) bad = 1;
            if (P.row_of_t) {
                const int r = P.row_of_t[row0 + t];
                if (r < 0 || r >= n) bad = 1;
            }
        }
        bad = __syncthreads_or(bad);
    }
    if (bad) {
        if (tid == 0) *P.status = 1;
        return;
    }
    double *ws = P.ws + (size_t)row0 * vbx_row_doubles(P.dim, P.max_spk) + (size_t)g * vbx_group_doubles(P.dim, P.max_spk);
    const int T = (int)n;
    if (vbx_chain_doubles(T, S) <= P.lds_doubles) vbx_group(P, g, row0, T, S, ws, dyn, s);
    else vbx_group(P, g, row0, T, S, ws, ws + (size_t)T * (vbx_dp(P.dim) + 2), s);
}

}  // namespace

extern "C" size_t xv_vbx_groups_workspace_bytes(int n_rows, int n_groups, int dim, int max_spk)
{
    if (n_rows < 1 || n_groups < 1 || dim < 1 || dim > XV_PCA_MAX_DIM || max_spk < 1 || max_spk > XV_VBX_MAX_SPK) return 0;
    return ((size_t)n_rows * vbx_row_doubles(dim, max_spk) + (size_t)n_groups * vbx_group_doubles(dim, max_spk)) * sizeof(double);
}

extern "C" int xv_vbx_groups_f64(const float *y, int64_t ldy, int n_rows, const int32_t *grp_row0, int n_groups, int dim,
                                 const int32_t *row_of_t, const int32_t *init_label, const int32_t *grp_spk, int max_spk,
                                 const double *plda_mean, const double *transform, const double *psi, double fa, double fb,
                                 double loop_prob, double init_smoothing, int max_iters, double epsilon, int32_t *labels, double *gamma,
                                 double *pi, double *elbo, int32_t *grp_iters, int32_t *grp_info, int32_t *status, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    if (n_groups < 1 || n_rows < 1 || dim < 1) return fail(XV_ERR_BAD_ARG, "vbx_groups: n_groups, n_rows and dim must be at least 1");
    if (dim > XV_PCA_MAX_DIM) return fail(XV_ERR_UNSUPPORTED, "vbx_groups: dim exceeds XV_PCA_MAX_DIM (128)");
    if (ldy < dim) return fail(XV_ERR_BAD_ARG, "vbx_groups: ldy must be at least dim");
    if (max_spk < 1 || max_spk > XV_VBX_MAX_SPK) return fail(XV_ERR_BAD_ARG, "vbx_groups: max_spk must be in [1, XV_VBX_MAX_SPK]");
    if (max_iters < 1 || max_iters > XV_VBX_MAX_ITERS) return fail(XV_ERR_BAD_ARG, "vbx_groups: max_iters must be in [1, XV_VBX_MAX_ITERS]");
    if (!(fa > 0.0 && std::isfinite(fa)) || !(fb > 0.0 && std::isfinite(fb)) || !(loop_prob >= 0.0 && loop_prob < 1.0) ||
        !(init_smoothing >= 0.0 && std::isfinite(init_smoothing)) || epsilon != epsilon)
        return fail(XV_ERR_BAD_ARG,
                    "vbx_groups: fa and fb must be finite and > 0, loop_prob in [0, 1), init_smoothing finite and >= 0, epsilon not NaN");
    if (!y || !grp_row0 || !init_label || !grp_spk || !plda_mean || !transform || !psi || !labels || !pi || !elbo || !grp_iters ||
        !grp_info || !status)
        return fail(XV_ERR_BAD_ARG, "vbx_groups: NULL pointer");
    if ((((uintptr_t)y | (uintptr_t)grp_row0 | (uintptr_t)row_of_t | (uintptr_t)init_label | (uintptr_t)grp_spk | (uintptr_t)labels |
          (uintptr_t)grp_iters | (uintptr_t)grp_info | (uintptr_t)status) & 3) ||
        (((uintptr_t)plda_mean | (uintptr_t)transform | (uintptr_t)psi | (uintptr_t)gamma | (uintptr_t)pi | (uintptr_t)elbo) & 7))
        return fail(XV_ERR_BAD_ARG, "vbx_groups: misaligned pointer (fp64 arrays and the workspace 8 bytes, the rest 4)");
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < xv_vbx_groups_workspace_bytes(n_rows, n_groups, dim, max_spk))
        return fail(XV_ERR_BAD_ARG, "vbx_groups: the workspace is missing, misaligned or smaller than xv_vbx_groups_workspace_bytes");
    // no group needs more LDS than all rows with max_spk speakers would
    size_t dyn = vbx_chain_doubles(n_rows, max_spk) * sizeof(double);
    if (dyn > VBX_LDS_CAP) dyn = VBX_LDS_CAP;
    using k_t = decltype(&vbx_kernel);
    static const k_t kerns[1] = {vbx_kernel};
    static std::atomic<unsigned long long> lds_done{0};
    if (const int rc = opt_in_dynamic_lds(lds_done, kerns, (int)(sizeof(VbxLds) + VBX_LDS_CAP))) return rc;
    const VbxParams p{y, (long)ldy, n_rows, grp_row0, dim, row_of_t, init_label, grp_spk, max_spk, plda_mean, transform, psi,
                      fa, fb, loop_prob, init_smoothing, max_iters, epsilon, labels, gamma, pi, elbo, grp_iters, grp_info, status,
                      static_cast<double *>(workspace), dyn / sizeof(double)};
    hipLaunchKernelGGL(vbx_kernel, dim3((unsigned)n_groups), dim3(VBX_NT), sizeof(VbxLds) + dyn, (hipStream_t)stream, p);
    return launch_status("vbx_kernel");
}
