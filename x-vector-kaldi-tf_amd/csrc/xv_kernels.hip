// xv_kernels.hip -- the exact-fp32 GEMM family of libxvector_hip.so (gfx950: MI355X / CDNA4) and the library's bookkeeping.
//
// Hot path of BUTSpeechFIT/x-vector-kaldi-tf's extraction (local/tf/models.py:50-94 evaluated by
// local/tf/models.py:414), written for CDNA4 from scratch:
//   tdnn_gemm_kernel   implicit-im2col GEMM on v_mfma_f32_32x32x2_f32 (exact fp32), 128x128 tile,
//                      4 wave64 per workgroup (2x2 waves, 2x2 MFMA tiles each), the dilated temporal
//                      context window staged ONCE per channel slab in LDS and re-used by all K taps,
//                      double-buffered LDS with register prefetch, fused bias/act/BN/gap-mask epilogue
//   tdnn_gemm_dma_kernel, tdnn_gemm_k1_kernel   the same arithmetic fed by global->LDS DMA; launch_gemm chooses
//   splitk_reduce_kernel, pack_weights(_rows), fold_bn   small helpers
//   xv_version, xv_last_error, xv_set_tuning (every family owns its knob: xv_internal_* setters)
// The other arithmetics of the same layers: xv_gemm3.hip (bf16x3), xv_gemm8*.hip (f16bf8), xv_toom.hip; the statistics
// pooling: xv_pool.hip.  See include/xvector_hip.h for the ABI contract and DESIGN.md for the layout / roofline notes.
#include "xv_device.h"

namespace {

thread_local char g_err[256] = "";

// ------------------------------------------------------------------------------------------------
// TDNN / FC GEMM (MAX_SPAN, the (K-1)*dilation limit of every GEMM family: xv_device.h -> the A tile holds BM+8 rows)
// ------------------------------------------------------------------------------------------------
constexpr int BM = 128;        // frames per workgroup tile
constexpr int BN = 128;        // output channels per workgroup tile
constexpr int BK = 32;         // input channels per LDS stage
constexpr int LDS_LD = 36;     // padded LDS row (floats): 144 B keeps ds_read_b128 conflict-free
constexpr int A_ROWS = BM + MAX_SPAN;
constexpr int NT = 256;

struct GemmParams {
    const float *x;
    long R;
    int cin, ldx;
    const float *wp;
    int kred;
    const float *bias, *scale, *shift;
    int act;
    const float *alpha;
    int K, dil, cout;
    const uint8_t *valid;
    float *y;
    int ldy;
    float *ypre;
    float *blk;         // POOL epilogue (no y / ypre): per-8-row-block (mean, M2) planes [ceil(R/8)][2][cout] (include/xvector_hip.h)
    int n_mt, n_nt;
    int vec_out;        // outputs take 16-byte stores: cout % 4 == 0, ldy % 4 == 0, y / ypre / per-column parameters 16-byte aligned
    int k_splits;       // split-K (xv_fc_splitk_f32, register-staged kernel only): the slabs are dealt to k_splits groups of workgroups, group ks
    float *part;        //   writes its raw partial sums to part + ks * part_stride ([R, cout] fp32 rows); a second kernel adds them up in order
    long part_stride;
    int lead;           // "rows" form (xv_tdnn_layer_rows_f32): K = 1 over rows that OVERLAP -- virtual row r = the cin floats from
                        // x + (r - lead) * ldx on, cin > ldx; reads are bounded by the END OF THE BUFFER (R * ldx floats), not by the row
};

constexpr size_t GEMM_LDS_BYTES = (size_t)(2 * A_ROWS * LDS_LD + 2 * BN * LDS_LD) * sizeof(float) + BM;

__device__ __forceinline__ float apply_act(float z, int act, float a)
{
    switch (act) {
    case XV_ACT_RELU: return fmaxf(z, 0.0f);
    case XV_ACT_LRELU: return z > 0.0f ? z : a * z;
    case XV_ACT_PRELU: return fmaxf(z, 0.0f) + a * fminf(z, 0.0f);
    default: return z;
    }
}

// act_t<ACT> (xv_device.h) is the same with the kind as a compile-time constant: identical expressions, hence identical bits -- but
// no switch per ELEMENT (the row-wise epilogue below used to evaluate one: ~6 scalar compares / branches around every 4 VALU
// instructions, nothing packed; beside an fp32 MFMA a co-resident workgroup pays for every one of them, cf. csrc/xv_toom.hip)

// Fused epilogue of the fp32 GEMM kernels, register-direct form.
// D layout of a 32x32 MFMA tile: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
template <int WROWS>      // rows of the tile one wave owns: 64 (two 32-row MFMA blocks) or 32 (one)
__device__ __forceinline__ void gemm_epilogue(const GemmParams &p, const uint8_t *Ms, long m0, int n0, int wr, int wc,
                                              int lane, const f32x16 &acc00, const f32x16 &acc01, const f32x16 &acc10,
                                              const f32x16 &acc11)
{
    const int colb = n0 + wc * 64 + (lane & 31);
    const int rowb = wr * WROWS + 4 * (lane >> 5);
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int gc = colb + cb * 32;
        if (gc >= p.cout) continue;
        const float bias = p.bias ? p.bias[gc] : 0.f;
        const float sc = p.scale ? p.scale[gc] : 1.f;
        const float sh = p.shift ? p.shift[gc] : 0.f;
        const float al = (p.act == XV_ACT_LRELU) ? p.alpha[0] : (p.act == XV_ACT_PRELU ? p.alpha[gc] : 0.f);
#pragma unroll
        for (int rb = 0; rb < WROWS / 32; ++rb) {
            const f32x16 &a = (rb == 0) ? (cb == 0 ? acc00 : acc01) : (cb == 0 ? acc10 : acc11);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int lr = rowb + rb * 32 + (reg & 3) + 8 * (reg >> 2);
                const long gr = m0 + lr;
                if (gr >= p.R) continue;
                const float z = a[reg] + bias;
                if (p.ypre) p.ypre[(size_t)gr * p.ldy + gc] = z;
                if (p.y) {
                    float v = apply_act(z, p.act, al) * sc + sh;
                    if (!Ms[lr]) v = 0.f;
                    __builtin_nontemporal_store(v, &p.y[(size_t)gr * p.ldy + gc]);   // streamed once: no L2 write-allocate
                }
            }
        }
    }
}

// The same epilogue with the output rows written as they lie in memory (round 3): the accumulators go through an fp32 tile in LDS
// (the operand buffers are dead by then: 128 x 132 floats of their 76 KB), and a thread then owns 4 consecutive columns of a row
// -- 32 lanes cover 512 contiguous bytes of an output row with one 16-byte store each, where the register-direct form above
// writes two 128-byte segments per 4-byte store instruction (a timing-only build without those stores ran the exact-fp32 step
// 3.8 % faster).  Element for element the same arithmetic: results are bit-identical to gemm_epilogue.
template <int BMT, int ACT>
__device__ __forceinline__ void gemm_epilogue_rows_body(const GemmParams &p, const float *T, const uint8_t *Ms, long m0, int n0, int tid)
{
    constexpr int TLD = BN + 4;
    const int cg = tid & 31, rp = tid >> 5;              // 4 columns; rows rp, rp + 8, ...
    const int gc = n0 + cg * 4;
    if (gc >= p.cout) return;                             // (cout % 4 == 0: a column group is inside or outside as a whole)
    const f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 bias = p.bias ? *reinterpret_cast<const f32x4 *>(p.bias + gc) : zero;
    const f32x4 sc = p.scale ? *reinterpret_cast<const f32x4 *>(p.scale + gc) : one;
    const f32x4 sh = p.shift ? *reinterpret_cast<const f32x4 *>(p.shift + gc) : zero;
    f32x4 al = zero;
    if constexpr (ACT == XV_ACT_LRELU) al = (f32x4){p.alpha[0], p.alpha[0], p.alpha[0], p.alpha[0]};
    else if constexpr (ACT == XV_ACT_PRELU) al = *reinterpret_cast<const f32x4 *>(p.alpha + gc);
    if (p.blk) {
        // POOL: the layer output is not stored; every 8-row block of the tile is reduced to per-channel (mean, M2) of its valid
        // rows, shifted by the block's first row (as the POOL epilogue of tdnn_gemm_bf16x3_kernel, xv_gemm3.hip: same planes, same finalize).
        // Thread = (4 channels, blocks rp and rp + 8).  Explicit fma: the two unrolled instances must round alike, a block's
        // statistics may not depend on where it sits in the tile.
#pragma unroll
        for (int bb = 0; bb < (BMT / 8 + 7) / 8; ++bb) {
            const int blk = rp + 8 * bb;
            if (blk >= BMT / 8 || m0 + blk * 8 >= p.R) continue;          // (a 32-row pass has four blocks: rp < 4)
            f32x4 tv[8];
            float keep[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                tv[j] = *reinterpret_cast<const f32x4 *>(T + (blk * 8 + j) * TLD + cg * 4);
                keep[j] = Ms[blk * 8 + j] ? 1.f : 0.f;
            }
            f32x4 v0 = zero, s1 = zero, s2 = zero;
            float n = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                n += keep[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = __builtin_fmaf(act_t<ACT>(tv[j][i] + bias[i], al[i]), sc[i], sh[i]);
                    if (j == 0) v0[i] = v;
                    else {
                        const float d = keep[j] != 0.f ? v - v0[i] : 0.f;       // (a select: a row past R may hold anything)
                        s1[i] += d;
                        s2[i] = __builtin_fmaf(d, d, s2[i]);
                    }
                }
            }
            // row 0 of a block is valid whenever any row is (chunks start on block boundaries, gaps follow the frames)
            const float rn = n > 0.f ? 1.f / n : 0.f;
            f32x4 mean, m2;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float t = s1[i] * rn;
                mean[i] = n > 0.f ? v0[i] + t : 0.f;
                m2[i] = fmaxf(__builtin_fmaf(-t, s1[i], s2[i]), 0.f);
            }
            float *o = p.blk + ((size_t)((m0 >> 3) + blk) * 2) * p.cout + gc;
            *reinterpret_cast<f32x4 *>(o) = mean;
            *reinterpret_cast<f32x4 *>(o + p.cout) = m2;
        }
        return;
    }
#pragma unroll 4
    for (int j = 0; j < BMT / 8; ++j) {
        const int lr = rp + 8 * j;
        const long gr = m0 + lr;
        if (gr >= p.R) continue;
        const f32x4 a = *reinterpret_cast<const f32x4 *>(T + lr * TLD + cg * 4);
        f32x4 z, v;
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = a[i] + bias[i];
        if (p.ypre) *reinterpret_cast<f32x4 *>(p.ypre + (size_t)gr * p.ldy + gc) = z;
        if (p.y) {
            const bool keep = Ms[lr] != 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float t = act_t<ACT>(z[i], al[i]) * sc[i] + sh[i];
                v[i] = keep ? t : 0.f;
            }
            __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(p.y + (size_t)gr * p.ldy + gc));   // streamed once: no L2 write-allocate
        }
    }
}

template <int BMT>
__device__ __forceinline__ void gemm_epilogue_rows(const GemmParams &p, float *T, const uint8_t *Ms, long m0, int n0, int wr, int wc,
                                                   int tid, const f32x16 &acc00, const f32x16 &acc01, const f32x16 &acc10,
                                                   const f32x16 &acc11)
{
    constexpr int WROWS = BMT / 2;
    constexpr int TLD = BN + 4;
    const int lane = tid & 63;
    {
        const int col = wc * 64 + (lane & 31);
        const int rowb = wr * WROWS + 4 * (lane >> 5);
#pragma unroll
        for (int rb = 0; rb < WROWS / 32; ++rb)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int lr = rowb + rb * 32 + (reg & 3) + 8 * (reg >> 2);
                T[lr * TLD + col] = rb == 0 ? acc00[reg] : acc10[reg];
                T[lr * TLD + col + 32] = rb == 0 ? acc01[reg] : acc11[reg];
            }
    }
    __syncthreads();
    switch (p.act) {                                      // (uniform: one switch per thread, not one per element)
    case XV_ACT_RELU: gemm_epilogue_rows_body<BMT, XV_ACT_RELU>(p, T, Ms, m0, n0, tid); break;
    case XV_ACT_LRELU: gemm_epilogue_rows_body<BMT, XV_ACT_LRELU>(p, T, Ms, m0, n0, tid); break;
    case XV_ACT_PRELU: gemm_epilogue_rows_body<BMT, XV_ACT_PRELU>(p, T, Ms, m0, n0, tid); break;
    default: gemm_epilogue_rows_body<BMT, XV_ACT_NONE>(p, T, Ms, m0, n0, tid); break;
    }
}

// VEC: Cin % 4 == 0 and 16-B aligned rows -> dwordx4 staging loads; otherwise dword loads (the
// 23-dim MFCC input layer).
// BMT: rows per workgroup tile, 128 or 64.  The 64-row form (each wave one 32-row MFMA block x two column blocks) exists
// for small problems -- a training minibatch of 19 k rows makes 608 128-row tiles on Cout = 512, i.e. 1.19 rounds of the
// 512 resident workgroups; 1216 half-size tiles are 2.4 rounds of half the length.
template <bool VEC, int BMT>
__global__ __launch_bounds__(NT, 2) void tdnn_gemm_kernel(const GemmParams p)
{
    constexpr int WROWS = BMT / 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *As = smem;                                 // [2][A_ROWS][LDS_LD]
    float *Bs = smem + 2 * A_ROWS * LDS_LD;           // [2][BN][LDS_LD]
    uint8_t *Ms = (uint8_t *)(Bs + 2 * BN * LDS_LD);  // [BM] row-valid bytes

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;

    // XCD-aware tile order: hardware places block b on XCD b%8; give each XCD a contiguous run of
    // logical tiles so that the n_nt tiles sharing one A panel sit on one L2 (bijective form).
    const int nwg = p.n_mt * p.n_nt;
    int bid = blockIdx.x, ks = 0;
    if (p.k_splits > 1) {                              // split-K: blocks [ks * nwg, (ks + 1) * nwg) work on slab group ks
        ks = bid / nwg;
        bid -= ks * nwg;
    }
    const int xcd = bid & 7, idx = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    const int mt = wg / p.n_nt, nt = wg - mt * p.n_nt;
    const long m0 = (long)mt * BMT;
    const int n0 = nt * BN;

    const int span = (p.K - 1) * p.dil;
    const int left = (span >> 1) + p.lead;
    const int rowsA = BMT + span;
    const int all_chunks = (p.cin + BK - 1) / BK;
    const int per_split = p.k_splits > 1 ? (all_chunks + p.k_splits - 1) / p.k_splits : all_chunks;
    const int c_lo = ks * per_split;
    const int n_chunks = (c_lo + per_split < all_chunks ? c_lo + per_split : all_chunks) - c_lo;      // (the launcher leaves no group empty)
    const int n_stages = n_chunks * p.K;
    const long flat_end = p.R * p.ldx;                 // (rows form: what the DMA-fed kernel's buffer descriptor checks)

    if (tid < BMT) {
        const long gr = m0 + tid;
        Ms[tid] = (gr < p.R) ? (p.valid ? p.valid[gr] : (uint8_t)1) : (uint8_t)0;
    }

    constexpr int B_REGS = VEC ? 4 : 16;
    constexpr int A_REGS = VEC ? ((BMT + MAX_SPAN) * 8 + NT - 1) / NT : ((BMT + MAX_SPAN) * 32 + NT - 1) / NT;
    typedef typename std::conditional<VEC, f32x4, float>::type stage_t;
    stage_t breg[B_REGS];
    stage_t areg[A_REGS];

    auto load_b = [&](int chunk, int tap) {
        const int c0 = chunk * BK;
#pragma unroll
        for (int j = 0; j < B_REGS; ++j) {
            const int f = tid + NT * j;
            if constexpr (VEC) {
                const int col = f >> 3, qq = f & 7;
                const int gcol = n0 + col, c = c0 + qq * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (gcol < p.cout && c < p.cin)
                    v = *reinterpret_cast<const f32x4 *>(p.wp + (size_t)gcol * p.kred + (size_t)tap * p.cin + c);
                breg[j] = v;
            } else {
                const int col = f >> 5, cc = f & 31;
                const int gcol = n0 + col, c = c0 + cc;
                float v = 0.f;
                if (gcol < p.cout && c < p.cin) v = p.wp[(size_t)gcol * p.kred + (size_t)tap * p.cin + c];
                breg[j] = v;
            }
        }
    };
    auto load_a = [&](int chunk) {
        const int c0 = chunk * BK;
#pragma unroll
        for (int j = 0; j < A_REGS; ++j) {
            const int f = tid + NT * j;
            if constexpr (VEC) {
                const int lr = f >> 3, qq = f & 7;
                const long gr = m0 - left + lr;
                const int c = c0 + qq * 4;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (lr < rowsA && gr >= 0 && c < p.cin && (p.lead ? gr * p.ldx + c + 4 <= flat_end : gr < p.R))
                    v = *reinterpret_cast<const f32x4 *>(p.x + (size_t)gr * p.ldx + c);
                areg[j] = v;
            } else {
                const int lr = f >> 5, cc = f & 31;
                const long gr = m0 - left + lr;
                const int c = c0 + cc;
                float v = 0.f;
                if (lr < rowsA && gr >= 0 && gr < p.R && c < p.cin) v = p.x[(size_t)gr * p.ldx + c];
                areg[j] = v;
            }
        }
    };
    auto store_b = [&](int buf) {
        float *dst = Bs + buf * (BN * LDS_LD);
#pragma unroll
        for (int j = 0; j < B_REGS; ++j) {
            const int f = tid + NT * j;
            if constexpr (VEC)
                *reinterpret_cast<f32x4 *>(dst + (f >> 3) * LDS_LD + (f & 7) * 4) = breg[j];
            else
                dst[(f >> 5) * LDS_LD + (f & 31)] = breg[j];
        }
    };
    auto store_a = [&](int buf) {
        float *dst = As + buf * (A_ROWS * LDS_LD);
#pragma unroll
        for (int j = 0; j < A_REGS; ++j) {
            const int f = tid + NT * j;
            if constexpr (VEC) {
                const int lr = f >> 3;
                if (lr < BMT + MAX_SPAN) *reinterpret_cast<f32x4 *>(dst + lr * LDS_LD + (f & 7) * 4) = areg[j];
            } else {
                const int lr = f >> 5;
                if (lr < BMT + MAX_SPAN) dst[lr * LDS_LD + (f & 31)] = areg[j];
            }
        }
    };

    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};

    // prologue: stage 0
    load_a(c_lo);
    load_b(c_lo, 0);
    store_a(c_lo & 1);
    store_b(0);
    __syncthreads();

    int chunk = c_lo, tap = 0;
    for (int s = 0; s < n_stages; ++s) {
        int nchunk = chunk, ntap = tap + 1;
        if (ntap == p.K) { ntap = 0; nchunk = chunk + 1; }
        const bool has_next = (s + 1) < n_stages;
        const bool new_a = has_next && (ntap == 0);
        if (has_next) {
            load_b(nchunk, ntap);
            if (new_a) load_a(nchunk);
        }

        const float *Ab = As + (chunk & 1) * (A_ROWS * LDS_LD) +
                          (wr * WROWS + (lane & 31) + tap * p.dil) * LDS_LD + (lane >> 5) * 4;
        const float *Bb = Bs + (s & 1) * (BN * LDS_LD) + (wc * 64 + (lane & 31)) * LDS_LD + (lane >> 5) * 4;
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
            const f32x4 a0 = *reinterpret_cast<const f32x4 *>(Ab + kk * 8);
            f32x4 a1 = a0;
            if constexpr (BMT == 128) a1 = *reinterpret_cast<const f32x4 *>(Ab + 32 * LDS_LD + kk * 8);
            const f32x4 b0 = *reinterpret_cast<const f32x4 *>(Bb + kk * 8);
            const f32x4 b1 = *reinterpret_cast<const f32x4 *>(Bb + 32 * LDS_LD + kk * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc00, 0, 0, 0);
                acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b1[j], acc01, 0, 0, 0);
                if constexpr (BMT == 128) {
                    acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b0[j], acc10, 0, 0, 0);
                    acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc11, 0, 0, 0);
                }
            }
        }

        if (has_next) {
            store_b((s + 1) & 1);
            if (new_a) store_a(nchunk & 1);
        }
        __syncthreads();
        chunk = nchunk;
        tap = ntap;
    }

    if (p.k_splits > 1) {
        // raw partial sums of this slab group as fp32 rows: the ordinary epilogue with nothing to add (bias, activation and BN
        // belong to the kernel that adds the groups up)
        GemmParams qp = p;
        qp.bias = qp.scale = qp.shift = nullptr;
        qp.act = XV_ACT_NONE;
        qp.y = nullptr;
        qp.blk = nullptr;
        qp.ypre = p.part + (size_t)ks * p.part_stride;
        qp.ldy = p.cout;
        if (p.vec_out) gemm_epilogue_rows<BMT>(qp, smem, Ms, m0, n0, wr, wc, tid, acc00, acc01, acc10, acc11);
        else gemm_epilogue<WROWS>(qp, Ms, m0, n0, wr, wc, lane, acc00, acc01, acc10, acc11);
        return;
    }
    if (p.vec_out) gemm_epilogue_rows<BMT>(p, smem, Ms, m0, n0, wr, wc, tid, acc00, acc01, acc10, acc11);     // (the loop ended with a barrier)
    else gemm_epilogue<WROWS>(p, Ms, m0, n0, wr, wc, lane, acc00, acc01, acc10, acc11);
}

// y = act(bias + sum_s part[s]) * scale + shift, ypre = bias + sum: the groups of a split-K launch added in group order (deterministic)
__global__ void splitk_reduce_kernel(const float *__restrict__ part, long part_stride, int nsplit, int R, int cout, const float *bias,
                                     const float *scale, const float *shift, int act, const float *alpha, float *y, int ldy, float *ypre,
                                     int ldpre)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)R * cout) return;
    const int r = (int)(i / cout), c = (int)(i - (size_t)r * cout);
    float z = bias ? bias[c] : 0.f;
    for (int k = 0; k < nsplit; ++k) z += part[(size_t)k * part_stride + i];
    if (ypre) ypre[(size_t)r * ldpre + c] = z;
    if (y) {
        const float a = act == XV_ACT_LRELU ? alpha[0] : act == XV_ACT_PRELU ? alpha[c] : 0.f;
        y[(size_t)r * ldy + c] = apply_act(z, act, a) * (scale ? scale[c] : 1.f) + (shift ? shift[c] : 0.f);
    }
}

// ------------------------------------------------------------------------------------------------
// Exact-fp32 GEMM, DMA-fed (round 4): the arithmetic of tdnn_gemm_kernel -- the same v_mfma_f32_32x32x2_f32 sequence on the same
// fragments in the same order, hence bit-identical results -- in the form of the 16-bit kernels:
//  * both operands go global -> LDS by buffer_load ... lds straight from the fp32 rows x[R, Cin] and the packed weights wp[Cout, K Cin]
//    as they lie (no staging registers, no ds_write, no exec-masked blocks of bounds logic: rows and columns outside the matrices
//    come back as zeros from the buffer descriptors' range check);
//  * an LDS row is 128 bytes (32 channels), unpadded; the 16-byte slot s of row r holds channel group s ^ ((r >> 1) & 7) -- the
//    swizzle is applied on the GLOBAL side of the DMA (lane (row, slot) of an 8-row piece fetches group slot ^ swz), fragment reads
//    are conflict-free for every tap offset;
//  * K is a template constant, the stage loop is unrolled over the taps of a slab; ONE barrier per stage, placed in front of the last
//    quarter of the stage's MFMAs: behind it the DMA of stage s + 2 goes out and the first fragments of stage s + 1 are read under the
//    remaining 16 MFMAs (two fragment sets, k-group granularity) -- no wave starts a stage with an empty pipe.
// Needs Cin % 32 == 0, 16-byte aligned rows, matrices below 2^31 bytes, the row-wise epilogue (else tdnn_gemm_kernel).
// ------------------------------------------------------------------------------------------------
constexpr int F_SROW = 128;
constexpr int F_A_BYTES = (BM + MAX_SPAN) * F_SROW;    // 17408
constexpr int F_B_BYTES = BN * F_SROW;                 // 16384
constexpr int F_OPER = 2 * F_A_BYTES + 2 * F_B_BYTES;  // 67584 = the epilogue's 128 x 132 fp32 tile
constexpr size_t F_LDS_BYTES = (size_t)F_OPER + BM;

template <int KT>
__global__ __launch_bounds__(NT, 2) void tdnn_gemm_dma_kernel(const GemmParams p)
{
    extern __shared__ __attribute__((aligned(16))) char flds[];
    char *Abuf = flds;                                 // [2][BM + 8 rows][128 B]
    char *Bbuf = flds + 2 * F_A_BYTES;                 // [2][BN cols][128 B]
    uint8_t *Ms = reinterpret_cast<uint8_t *>(flds + F_OPER);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;

    const int nwg = p.n_mt * p.n_nt;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, idx = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    const int mt = wg / p.n_nt, nt = wg - mt * p.n_nt;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;

    const int span = (KT - 1) * p.dil;
    const int left = (span >> 1) + p.lead;
    const int n_chunks = p.cin / BK;
    const int n_stages = n_chunks * KT;

    if (tid < BM) {
        const long gr = m0 + tid;
        Ms[tid] = (gr < p.R) ? (p.valid ? p.valid[gr] : (uint8_t)1) : (uint8_t)0;
    }

    // ---- DMA: piece pc = 8 rows (columns) x 128 bytes; wave w moves pieces w, w + 4, ...: their parity is the wave's, and with it
    // bit 2 of (row >> 1) & 7 -- the swizzle of the row a lane moves is a per-lane constant.  The row part of an address sits in
    // the VGPR offset (what the range check looks at), the channel / tap part in the scalar offset.
    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x), 0, (int)(p.R * p.ldx * 4), XV_RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wp), 0, (int)((long)p.cout * p.kred * 4), XV_RSRC_FLAGS);
    const int slotb = ((lane & 7) ^ (((wave & 1) * 4 + (lane >> 4)) & 7)) << 4;
    const int arow_bytes = p.ldx * 4, brow_bytes = p.kred * 4;
    const int va0 = (int)(m0 - left + 8 * wave + (lane >> 3)) * arow_bytes + slotb;        // piece `wave`; piece wave + 4 j: + 32 j rows
    const int vb0 = (n0 + 8 * wave + (lane >> 3)) * brow_bytes + slotb;
    constexpr int NP = KT == 1 ? BM / 8 : BM / 8 + 1;   // pieces of a halo tile (BM + span rows, span <= 8)
    auto dma_b = [&](int stage, int buf) {              // the weight tile of (slab, tap) = stage, four pieces per wave
        const int st = stage < n_stages ? stage : n_stages - 1;
        const int c = st / KT, t = st - c * KT;
        const int so = (t * p.cin + c * BK) * 4;
        char *dst = Bbuf + buf * F_B_BYTES + wave * 1024;
#pragma unroll
        for (int j = 0; j < 4; ++j) XV_BLDS16(brs, dst + j * 4096, vb0 + j * 32 * brow_bytes, so, 0);
    };
    auto dma_a_piece = [&](int chunk, int j) {          // piece wave + 4 j of slab `chunk` (clamped: the tail rewrites identical bytes)
        const int c = chunk < n_chunks ? chunk : n_chunks - 1;
        XV_BLDS16(ars, Abuf + (c & 1) * F_A_BYTES + (wave + 4 * j) * 1024, va0 + j * 32 * arow_bytes, c * BK * 4, 0);
    };
    auto dma_a_all = [&](int chunk) {
#pragma unroll
        for (int j = 0; j < 4; ++j) dma_a_piece(chunk, j);
        if (NP > 16 && wave == 0) dma_a_piece(chunk, 4);
    };
    dma_b(0, 0);
    dma_b(1, 1);
    dma_a_all(0);
    if (KT == 1) dma_a_all(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
    struct Fr { f32x4 a0, a1, b0, b1; };
    // fragment addresses: lane (row l & 31, k half kh = l >> 5) reads channels 8 kk + 4 kh .. + 3 = slot 2 kk + kh of its row
    const int kh = lane >> 5;
    int pa[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const int lr0 = wr * 64 + (lane & 31) + t * p.dil;
        pa[t] = lr0 * F_SROW + ((((lr0 >> 1) & 7) ^ kh) << 4);          // + 32 rows: + 4096, the same swizzle; k group kk: ^ (kk << 5)
    }
    const int bcol = wc * 64 + (lane & 31);
    const int pb = 2 * F_A_BYTES + bcol * F_SROW + ((((bcol >> 1) & 7) ^ kh) << 4);
    auto load = [&](Fr &X, int abase, int bbase, int kk) {
        X.a0 = *reinterpret_cast<const f32x4 *>(flds + (abase ^ (kk << 5)));
        X.a1 = *reinterpret_cast<const f32x4 *>(flds + (abase ^ (kk << 5)) + 32 * F_SROW);
        X.b0 = *reinterpret_cast<const f32x4 *>(flds + (bbase ^ (kk << 5)));
        X.b1 = *reinterpret_cast<const f32x4 *>(flds + (bbase ^ (kk << 5)) + 32 * F_SROW);
    };
    auto mma = [&](const Fr &X) {                        // (the order of tdnn_gemm_kernel: results are bit-identical)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(X.a0[j], X.b0[j], acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(X.a0[j], X.b1[j], acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(X.a1[j], X.b0[j], acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(X.a1[j], X.b1[j], acc11, 0, 0, 0);
        }
    };
    auto pin = [&]() {                                   // 16 MFMAs, the four fragment reads behind the first four
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    // halo pieces of the NEXT slab, dealt over taps 0 .. K-2 of the current one (K > 1): five one-piece-per-wave slots
    constexpr int DT = KT == 1 ? 1 : KT - 1;
    constexpr int NS = KT == 1 ? 4 : 5;
    auto slots_of = [](int t) constexpr { return t < DT ? (NS + DT - 1 - t) / DT : 0; };
    auto slot_base = [](int t) constexpr { int b = 0; for (int u = 0; u < t; ++u) b += (NS + DT - 1 - u) / DT; return b; };

    Fr F, G;
    load(F, pa[0], pb, 0);
    int s = 0;
    for (int c = 0; c < n_chunks; ++c) {
        const int abuf = (c & 1) * F_A_BYTES;
        auto tap = [&](auto TT) {
            constexpr int t = decltype(TT)::value;
            const int ab = pa[t] + abuf, bb = pb + (s & 1) * F_B_BYTES;
            load(G, ab, bb, 1);
            mma(F);
            pin();
            load(F, ab, bb, 2);
            mma(G);
            pin();
            load(G, ab, bb, 3);
            mma(F);
            pin();
            // every fragment of stage s is in registers (the reads of k group 3 went out 1024 MFMA cycles ago), stage s + 1 has landed
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            dma_b(s + 2, s & 1);
            if constexpr (KT == 1) {
                dma_a_all(s + 2);
            } else if constexpr (t < DT) {
#pragma unroll
                for (int j = 0; j < slots_of(t); ++j) {
                    const int jj = slot_base(t) + j;
                    if (jj < 4 || wave == 0) dma_a_piece(c + 1, jj);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (t + 1 < KT) load(F, pa[t + 1] + abuf, pb + ((s + 1) & 1) * F_B_BYTES, 0);
            else load(F, pa[0] + (F_A_BYTES - abuf), pb + ((s + 1) & 1) * F_B_BYTES, 0);      // first tap of the next slab (tail: harmless)
            mma(G);
            pin();
            ++s;
        };
        static_for<0, KT>(tap);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (the tail's clamped pieces must have landed before the tile below reuses the LDS)
    __syncthreads();
    gemm_epilogue_rows<BM>(p, reinterpret_cast<float *>(flds), Ms, m0, n0, wr, wc, tid, acc00, acc01, acc10, acc11);
}

// ------------------------------------------------------------------------------------------------
// The K = 1 layers of the exact-fp32 path on 16-CHANNEL slabs (round 6): the same MFMA sequence on the same fragments in the same
// order as tdnn_gemm_dma_kernel<1> (bit-identical), but an LDS row is 64 bytes, a stage 8 + 8 KB, and the epilogue goes through a
// 64-row tile in two passes -- 34 KB of LDS per workgroup instead of 68, THREE workgroups per CU instead of two (four fit the LDS; at 128 VGPRs the epilogue spills).  A K = 1 tile is
// 16 (here 32) stages and pays ~2.1 of the old stages at its boundary (epilogue, then the first DMA's latency; fitted from K = 1 / 5 / 7:
// DESIGN 9.6) with ONE other workgroup on the CU to cover it; a persistent launch changed nothing (profiles/r06_fp32_persistent.txt),
// two other workgroups do: 0.85 -> 0.89-0.91 of the fp32-MFMA peak.
//  * piece = 16 rows x 64 bytes; lane l of a piece moves row l >> 2, 16-byte slot l & 3; physical slot = logical ^ ((row >> 2) & 3),
//    applied on the global side of the DMA: the 16 lanes of a ds_read_b128 group (16 consecutive rows, one logical slot) hit 16
//    different bank quads;
//  * stage = 2 k groups = 32 MFMAs per wave, one barrier per stage, the DMA of stage s + 2 behind it.
// ------------------------------------------------------------------------------------------------
constexpr int G_BK = 16;
constexpr int G_SROW = 64;
constexpr int G_A_BYTES = BM * G_SROW;                 // 8192
constexpr int G_B_BYTES = BN * G_SROW;                 // 8192
constexpr int G_TROWS = 64;                            // the epilogue's tile: two passes of 64 rows (33.8 KB; three or four workgroups per CU)
constexpr int G_TILE = G_TROWS * (BN + 4) * 4;
constexpr int G_OPER = 2 * G_A_BYTES + 2 * G_B_BYTES;  // 32768
constexpr int G_MS = G_TILE > G_OPER ? G_TILE : G_OPER;
constexpr size_t G_LDS_BYTES = (size_t)G_MS + BM;

template <int ACT>
__device__ __forceinline__ void k1_epilogue(const GemmParams &p, char *lds, const uint8_t *Ms, long m0, int n0, int wr, int wc, int tid,
                                            const f32x16 &acc00, const f32x16 &acc01, const f32x16 &acc10, const f32x16 &acc11)
{
    constexpr int TLD = BN + 4;
    float *T = reinterpret_cast<float *>(lds);
    const int lane = tid & 63;
    const int col = wc * 64 + (lane & 31);
#pragma unroll
    for (int pass = 0; pass < BM / G_TROWS; ++pass) {
        if (wr == pass) {                                  // the waves that own rows [64 pass, 64 pass + 64)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int lr = 4 * (lane >> 5) + (reg & 3) + 8 * (reg >> 2);
                T[lr * TLD + col] = acc00[reg];
                T[lr * TLD + col + 32] = acc01[reg];
                T[(lr + 32) * TLD + col] = acc10[reg];
                T[(lr + 32) * TLD + col + 32] = acc11[reg];
            }
        }
        __syncthreads();
        gemm_epilogue_rows_body<G_TROWS, ACT>(p, T, Ms + G_TROWS * pass, m0 + G_TROWS * pass, n0, tid);
        __syncthreads();
    }
}

// three workgroups per CU: 168 VGPRs, no spills (a build for four, at 128 VGPRs, spills in the epilogue)
__global__ __launch_bounds__(NT, 3) void tdnn_gemm_k1_kernel(const GemmParams p)
{
    extern __shared__ __attribute__((aligned(16))) char glds[];
    char *Abuf = glds;                                 // [2][BM rows][64 B]
    char *Bbuf = glds + 2 * G_A_BYTES;                 // [2][BN cols][64 B]
    uint8_t *Ms = reinterpret_cast<uint8_t *>(glds + G_MS);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;

    const int nwg = p.n_mt * p.n_nt;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, idx = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    const int mt = wg / p.n_nt, nt = wg - mt * p.n_nt;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;
    const int n_stages = p.cin / G_BK;

    if (tid < BM) {
        const long gr = m0 + tid;
        Ms[tid] = (gr < p.R) ? (p.valid ? p.valid[gr] : (uint8_t)1) : (uint8_t)0;
    }

    const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x), 0, (int)(p.R * p.ldx * 4), XV_RSRC_FLAGS);
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wp), 0, (int)((long)p.cout * p.kred * 4), XV_RSRC_FLAGS);
    // piece pc = 16 rows (columns); wave w moves pieces w and w + 4 of each operand and stage
    const int slotb = ((lane & 3) ^ ((lane >> 4) & 3)) << 4;
    const int arow_bytes = p.ldx * 4, brow_bytes = p.kred * 4;
    const int va0 = (int)(m0 - p.lead + 16 * wave + (lane >> 2)) * arow_bytes + slotb;
    const int vb0 = (n0 + 16 * wave + (lane >> 2)) * brow_bytes + slotb;
    auto dma = [&](int stage, int buf) {
        const int st = stage < n_stages ? stage : n_stages - 1;          // (the tail rewrites identical bytes)
        const int so = st * G_BK * 4;
        char *da = Abuf + buf * G_A_BYTES + wave * 1024, *db = Bbuf + buf * G_B_BYTES + wave * 1024;
        XV_BLDS16(ars, da, va0, so, 0);
        XV_BLDS16(ars, da + 4096, va0 + 64 * arow_bytes, so, 0);
        XV_BLDS16(brs, db, vb0, so, 0);
        XV_BLDS16(brs, db + 4096, vb0 + 64 * brow_bytes, so, 0);
    };
    dma(0, 0);
    dma(1, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
    struct Fr { f32x4 a0, a1, b0, b1; };
    // lane (row l & 31, k half kh = l >> 5) reads channels 8 kk + 4 kh .. + 3 of the slab = logical slot 2 kk + kh of its row
    const int kh = lane >> 5;
    const int ar = wr * 64 + (lane & 31), bc = wc * 64 + (lane & 31);
    const int pa = ar * G_SROW + ((kh ^ ((ar >> 2) & 3)) << 4);          // + 32 rows: + 2048, the same swizzle; k group 1: ^ 32
    const int pb = 2 * G_A_BYTES + bc * G_SROW + ((kh ^ ((bc >> 2) & 3)) << 4);
    auto load = [&](Fr &X, int buf, int kk) {
        const int ab = (pa ^ (kk << 5)) + buf * G_A_BYTES, bb = (pb ^ (kk << 5)) + buf * G_B_BYTES;
        X.a0 = *reinterpret_cast<const f32x4 *>(glds + ab);
        X.a1 = *reinterpret_cast<const f32x4 *>(glds + ab + 32 * G_SROW);
        X.b0 = *reinterpret_cast<const f32x4 *>(glds + bb);
        X.b1 = *reinterpret_cast<const f32x4 *>(glds + bb + 32 * G_SROW);
    };
    auto mma = [&](const Fr &X) {                        // (the order of tdnn_gemm_kernel / tdnn_gemm_dma_kernel: results are bit-identical)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(X.a0[j], X.b0[j], acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(X.a0[j], X.b1[j], acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(X.a1[j], X.b0[j], acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(X.a1[j], X.b1[j], acc11, 0, 0, 0);
        }
    };
    auto pin = [&]() {                                   // 16 MFMAs, the four fragment reads behind the first four
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    Fr F, G;
    load(F, 0, 0);
    for (int s = 0; s < n_stages; ++s) {
        load(G, s & 1, 1);
        mma(F);
        pin();
        // both fragment sets of stage s are in registers, stage s + 1 has landed.  (A third stage buffer -- the DMA two stages ahead,
        // counted waits -- was measured: +-0, profiles/r06_fp32_k1_slab16.txt.)
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        dma(s + 2, s & 1);
        __builtin_amdgcn_sched_barrier(0);
        load(F, (s + 1) & 1, 0);                         // (tail: harmless)
        mma(G);
        pin();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (the tail's clamped pieces must have landed before the tile below reuses the LDS)
    __syncthreads();
    switch (p.act) {                                      // (uniform: one switch per thread, not one per element)
    case XV_ACT_RELU: k1_epilogue<XV_ACT_RELU>(p, glds, Ms, m0, n0, wr, wc, tid, acc00, acc01, acc10, acc11); break;
    case XV_ACT_LRELU: k1_epilogue<XV_ACT_LRELU>(p, glds, Ms, m0, n0, wr, wc, tid, acc00, acc01, acc10, acc11); break;
    case XV_ACT_PRELU: k1_epilogue<XV_ACT_PRELU>(p, glds, Ms, m0, n0, wr, wc, tid, acc00, acc01, acc10, acc11); break;
    default: k1_epilogue<XV_ACT_NONE>(p, glds, Ms, m0, n0, wr, wc, tid, acc00, acc01, acc10, acc11); break;
    }
}

std::atomic<int> g_fp32_form{0};

int launch_gemm(const GemmParams &p0, hipStream_t st)
{
    GemmParams p = p0;
    if (p.R <= 0 || p.cout <= 0) return 0;
    if (p.cin <= 0 || p.K <= 0 || (p.K & 1) == 0 || p.dil <= 0) return fail(XV_ERR_BAD_ARG, "tdnn: K must be odd, dims > 0");
    if ((p.K - 1) * p.dil > MAX_SPAN) return fail(XV_ERR_UNSUPPORTED, "tdnn: (K-1)*dilation > 8 unsupported");
    if ((p.lead == 0 && p.ldx < p.cin) || p.ldy < p.cout) return fail(XV_ERR_BAD_ARG, "tdnn: leading dimension too small");
    if ((p.act == XV_ACT_LRELU || p.act == XV_ACT_PRELU) && !p.alpha) return fail(XV_ERR_BAD_ARG, "tdnn: act_alpha is NULL");
    p.kred = p.K * p.cin;
    p.n_nt = (p.cout + BN - 1) / BN;
    // 64-row tiles when 128-row tiles would leave the chip with fewer than 1.5 rounds of resident workgroups
    const bool small = ((p.R + BM - 1) / BM) * p.n_nt < 768;
    const int bmt = small ? 64 : BM;
    p.n_mt = (int)((p.R + bmt - 1) / bmt);
    const bool vec = (p.cin % 4 == 0) && (p.ldx % 4 == 0) && (((uintptr_t)p.x) % 16 == 0) && (((uintptr_t)p.wp) % 16 == 0);
    if (p.lead && (!vec || p.K != 1 || p.ypre)) return fail(XV_ERR_UNSUPPORTED, "tdnn_rows: needs 16-byte aligned rows of a multiple of 4 floats");
    const uintptr_t out_bits = (uintptr_t)p.y | (uintptr_t)p.ypre | (uintptr_t)p.bias | (uintptr_t)p.scale | (uintptr_t)p.shift |
                               (p.act == XV_ACT_PRELU ? (uintptr_t)p.alpha : 0);
    p.vec_out = (p.cout % 4 == 0) && (p.ldy % 4 == 0) && (out_bits % 16 == 0);
    if (p.blk && !p.vec_out) return fail(XV_ERR_UNSUPPORTED, "tdnn_pool: needs cout % 4 == 0 and 16-byte aligned per-column parameters");
    typedef void (*kern_t)(const GemmParams);
    const kern_t all[] = {tdnn_gemm_kernel<true, 128>, tdnn_gemm_kernel<false, 128>, tdnn_gemm_kernel<true, 64>,
                          tdnn_gemm_kernel<false, 64>};
    const kern_t dma_all[] = {tdnn_gemm_dma_kernel<1>, tdnn_gemm_dma_kernel<3>, tdnn_gemm_dma_kernel<5>, tdnn_gemm_dma_kernel<7>};
    typedef std::pair<kern_t, size_t> kern_lds;
    const kern_lds lds[] = {{all[0], GEMM_LDS_BYTES}, {all[1], GEMM_LDS_BYTES}, {all[2], GEMM_LDS_BYTES}, {all[3], GEMM_LDS_BYTES},
                            {dma_all[0], F_LDS_BYTES}, {dma_all[1], F_LDS_BYTES}, {dma_all[2], F_LDS_BYTES}, {dma_all[3], F_LDS_BYTES},
                            {tdnn_gemm_k1_kernel, G_LDS_BYTES}};
    static std::atomic<unsigned long long> lds_done{0};
    if (const int rc = opt_in_dynamic_lds(lds_done, lds, [](const kern_lds &kl) { return kl; })) return rc;
    const dim3 grid((unsigned)(p.n_mt * p.n_nt));
    // the DMA-fed form (128-row tiles): whole 32-channel slabs, 16-byte aligned rows, byte offsets that fit the descriptors' 32 bits
    const int form = g_fp32_form.load(std::memory_order_relaxed);       // XV_TUNE_FP32_GEMM: 0 built-in (= 3), 1 register-staged, 2 DMA-fed, 3 DMA-fed with the K = 1 layers on 16-channel slabs
    const bool dma_on = form != 1;
    // K = 1 on 16-channel slabs: profiles/r06_fp32_k1_slab16.txt, 1.03 -> 0.98 ms, 3.06 -> 2.90 ms
    const bool k1_on = form == 0 || form == 3;
    const bool dma_ok = dma_on && !small && p.k_splits <= 1 && vec && p.vec_out && (p.cin % BK) == 0 && (p.K == 1 || p.K == 3 || p.K == 5 || p.K == 7) &&
                        (p.R + BM + MAX_SPAN) * (long)p.ldx * 4 < (1l << 31) && (long)(p.cout + BN) * p.kred * 4 < (1l << 31);
    if (dma_ok && k1_on && p.K == 1 && p.cin >= 2 * G_BK) {
        hipLaunchKernelGGL(tdnn_gemm_k1_kernel, grid, dim3(NT), G_LDS_BYTES, st, p);
        return launch_status("tdnn_gemm_k1_kernel launch");
    }
    if (dma_ok) {
        const kern_t dk = p.K == 1 ? tdnn_gemm_dma_kernel<1> : p.K == 3 ? tdnn_gemm_dma_kernel<3> : p.K == 5 ? tdnn_gemm_dma_kernel<5>
                                                                                                             : tdnn_gemm_dma_kernel<7>;
        hipLaunchKernelGGL(dk, grid, dim3(NT), F_LDS_BYTES, st, p);
        return launch_status("tdnn_gemm_dma_kernel launch");
    }
    if (p.k_splits > 1) {
        hipLaunchKernelGGL(all[(small ? 2 : 0) + (vec ? 0 : 1)], dim3((unsigned)(p.n_mt * p.n_nt * p.k_splits)), dim3(NT), GEMM_LDS_BYTES, st, p);
        return launch_status("tdnn_gemm_kernel (split-K) launch");
    }
    hipLaunchKernelGGL(all[(small ? 2 : 0) + (vec ? 0 : 1)], grid, dim3(NT), GEMM_LDS_BYTES, st, p);
    return launch_status("tdnn_gemm_kernel launch");
}

__global__ void pack_weights_kernel(const float *__restrict__ w, int kred, int cout, float *__restrict__ wp)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)kred * cout) return;
    const int n = (int)(i / kred), k = (int)(i - (size_t)n * kred);
    wp[i] = w[(size_t)k * cout + n];
}

// w[K, cin, cout] -> wp[cout][kpad] for the rows form: column k * ldx + c holds w[k][c][o] (c < cin), every other column zero
__global__ void pack_weights_rows_kernel(const float *__restrict__ w, int K, int cin, int ldx, int cout, int kpad, float *__restrict__ wp)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)kpad * cout) return;
    const int o = (int)(i / kpad), col = (int)(i - (size_t)o * kpad);
    const int k = col / ldx, c = col - k * ldx;
    wp[i] = (k < K && c < cin) ? w[((size_t)k * cin + c) * cout + o] : 0.f;
}

__global__ void fold_bn_kernel(const float *gamma, const float *beta, const float *mean, const float *var, float eps,
                               int c, float *scale, float *shift)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c) return;
    const float s = gamma[i] * (1.0f / sqrtf(var[i] + eps));
    float ms = mean[i] * s;
    asm volatile("" : "+v"(ms));
    scale[i] = s;
    shift[i] = beta[i] - ms;
}

// The share of a producer's BN shift in its consumer's pre-activation (xv_fold_shift_taps_f32): one thread per output channel,
// taps and input channels in ascending order, fp64 throughout.  tap[t][o] = sum_c shift[c] * w[t][c][o];
// bias_full[o] = bias[o] + sum_t tap[t][o] (from the unrounded sums).
__global__ void fold_shift_taps_kernel(const float *__restrict__ w, const float *__restrict__ shift, const float *__restrict__ bias,
                                       int K, int cin, int cout, float *__restrict__ tap, float *__restrict__ bias_full)
{
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= cout) return;
    double total = bias ? (double)bias[o] : 0.0;
    for (int t = 0; t < K; ++t) {
        double acc = 0.0;
        for (int c = 0; c < cin; ++c) acc += (double)shift[c] * (double)w[((size_t)t * cin + c) * cout + o];
        if (tap) tap[(size_t)t * cout + o] = (float)acc;
        total += acc;
    }
    bias_full[o] = (float)total;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

// every family owns its tuning knob; xv_set_tuning checks the range and hands the value over
void xv_internal_gemm3_tile_rows(int value);      // xv_gemm3.hip
void xv_internal_gemm8_tile_rows(int value);      // xv_gemm8.hip
void xv_internal_first_tiles(int tiles);          // xv_first.hip

int xv_version(void) { return 44; }

int xv_set_tuning(int key, int value)
{
    switch (key) {
    case XV_TUNE_TILE_ROWS:
        if (value != 0 && value != 128 && value != 256 && value != 512 && value != 1024)
            return fail(XV_ERR_BAD_ARG, "xv_set_tuning: tile rows must be 0, 128, 256, 512 or 1024");
        xv_internal_gemm3_tile_rows(value >= 512 ? 256 : value);
        xv_internal_gemm8_tile_rows(value);
        return 0;
    case XV_TUNE_FIRST_TILES:
        if (value < 0 || value > 4096) return fail(XV_ERR_BAD_ARG, "xv_set_tuning: first-layer tiles per wave must be 0 .. 4096");
        xv_internal_first_tiles(value);
        return 0;
    case XV_TUNE_FP32_GEMM:
        if (value < 0 || value > 3) return fail(XV_ERR_BAD_ARG, "xv_set_tuning: fp32 GEMM form must be 0, 1, 2 or 3");
        g_fp32_form.store(value, std::memory_order_relaxed);
        return 0;
    default:
        return fail(XV_ERR_BAD_ARG, "xv_set_tuning: unknown key");
    }
}

const char *xv_last_error(void) { return g_err; }

int xv_pack_weights_f32(const float *w, int kred, int cout, float *wp, void *stream)
{
    if (!w || !wp || kred <= 0 || cout <= 0) return fail(XV_ERR_BAD_ARG, "pack_weights: bad argument");
    const size_t n = (size_t)kred * cout;
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, kred, cout, wp);
    return launch_status("pack_weights_kernel");
}

int xv_fold_bn_f32(const float *gamma, const float *beta, const float *mean, const float *var, float eps, int c,
                   float *scale, float *shift, void *stream)
{
    if (!gamma || !beta || !mean || !var || !scale || !shift || c <= 0) return fail(XV_ERR_BAD_ARG, "fold_bn: bad argument");
    hipLaunchKernelGGL(fold_bn_kernel, dim3((c + 255) / 256), dim3(256), 0, (hipStream_t)stream, gamma, beta, mean, var, eps, c, scale, shift);
    return launch_status("fold_bn_kernel");
}

int xv_fold_shift_taps_f32(const float *w, const float *shift, const float *bias, int K, int cin, int cout, float *tap_bias,
                           float *bias_full, void *stream)
{
    if (!w || !shift || !bias_full || K <= 0 || cin <= 0 || cout <= 0) return fail(XV_ERR_BAD_ARG, "fold_shift_taps: bad argument");
    hipLaunchKernelGGL(fold_shift_taps_kernel, dim3((cout + 63) / 64), dim3(64), 0, (hipStream_t)stream, w, shift, bias, K, cin, cout,
                       tap_bias, bias_full);
    return launch_status("fold_shift_taps_kernel");
}

int xv_tdnn_layer_f32(const float *x, int64_t R, int cin, int ldx, const float *wp, const float *bias,
                      const float *bn_scale, const float *bn_shift, int act_kind, const float *act_alpha, int K,
                      int dilation, int cout, const uint8_t *row_valid, float *y, int ldy, float *y_preact,
                      void *stream)
{
    if (!x || !wp || (!y && !y_preact)) return fail(XV_ERR_BAD_ARG, "tdnn: NULL pointer");
    if (act_kind < XV_ACT_NONE || act_kind > XV_ACT_PRELU) return fail(XV_ERR_BAD_ARG, "tdnn: unknown act_kind");
    GemmParams p{};
    p.x = x; p.R = (long)R; p.cin = cin; p.ldx = ldx; p.wp = wp;
    p.bias = bias; p.scale = bn_scale; p.shift = bn_shift; p.act = act_kind; p.alpha = act_alpha;
    p.K = K; p.dil = dilation; p.cout = cout; p.valid = row_valid; p.y = y; p.ldy = ldy; p.ypre = y_preact;
    return launch_gemm(p, (hipStream_t)stream);
}

size_t xv_packed_weights_rows_f32_floats(int K, int cin, int ldx, int cout)
{
    if (K <= 0 || (K & 1) == 0 || cin <= 0 || ldx < cin || (ldx & 3) || cout <= 0) return 0;
    return (size_t)cout * (((size_t)K * ldx + BK - 1) / BK * BK);
}

int xv_pack_weights_rows_f32(const float *w, int K, int cin, int ldx, int cout, float *wp, void *stream)
{
    const size_t n = xv_packed_weights_rows_f32_floats(K, cin, ldx, cout);
    if (!w || !wp || n == 0) return fail(XV_ERR_BAD_ARG, "pack_weights_rows: K odd, cin <= ldx, ldx % 4 == 0");
    hipLaunchKernelGGL(pack_weights_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, K, cin, ldx, cout,
                       (int)(n / cout), wp);
    return launch_status("pack_weights_rows_kernel");
}

int xv_tdnn_layer_rows_f32(const float *x, int64_t R, int cin, int ldx, const float *wp, const float *bias, const float *bn_scale,
                           const float *bn_shift, int act_kind, const float *act_alpha, int K, int cout, const uint8_t *row_valid,
                           float *y, int ldy, void *stream)
{
    if (!x || !wp || !y) return fail(XV_ERR_BAD_ARG, "tdnn_rows: NULL pointer");
    if (act_kind < XV_ACT_NONE || act_kind > XV_ACT_PRELU) return fail(XV_ERR_BAD_ARG, "tdnn_rows: unknown act_kind");
    const size_t n = xv_packed_weights_rows_f32_floats(K, cin, ldx, cout);
    if (n == 0) return fail(XV_ERR_BAD_ARG, "tdnn_rows: K odd, cin <= ldx, ldx % 4 == 0");
    GemmParams p{};
    p.x = x; p.R = (long)R; p.cin = (int)(n / cout); p.ldx = ldx; p.wp = wp;
    p.bias = bias; p.scale = bn_scale; p.shift = bn_shift; p.act = act_kind; p.alpha = act_alpha;
    p.K = 1; p.dil = 1; p.cout = cout; p.valid = row_valid; p.y = y; p.ldy = ldy; p.lead = (K - 1) / 2;
    return launch_gemm(p, (hipStream_t)stream);
}

int xv_tdnn_layer_pool_f32(const float *x, int64_t R, int cin, int ldx, const float *wp, const float *bias, const float *bn_scale,
                           const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                           const uint8_t *row_valid, float *block_stats, void *stream)
{
    if (!x || !wp || !block_stats) return fail(XV_ERR_BAD_ARG, "tdnn_pool: NULL pointer");
    if (act_kind < XV_ACT_NONE || act_kind > XV_ACT_PRELU) return fail(XV_ERR_BAD_ARG, "tdnn_pool: unknown act_kind");
    if (((uintptr_t)block_stats) & 15) return fail(XV_ERR_BAD_ARG, "tdnn_pool: block_stats must be 16-byte aligned");
    GemmParams p{};
    p.x = x; p.R = (long)R; p.cin = cin; p.ldx = ldx; p.wp = wp;
    p.bias = bias; p.scale = bn_scale; p.shift = bn_shift; p.act = act_kind; p.alpha = act_alpha;
    p.K = K; p.dil = dilation; p.cout = cout; p.valid = row_valid; p.ldy = cout; p.blk = block_stats;
    return launch_gemm(p, (hipStream_t)stream);
}

int xv_fc_f32(const float *x, int nrows, int in_dim, const float *wp, const float *bias, const float *bn_scale,
              const float *bn_shift, int act_kind, const float *act_alpha, int out_dim, float *y, float *y_preact,
              void *stream)
{
    return xv_tdnn_layer_f32(x, nrows, in_dim, in_dim, wp, bias, bn_scale, bn_shift, act_kind, act_alpha, 1, 1,
                             out_dim, nullptr, y, out_dim, y_preact, stream);
}

// Split-K plan of a skinny FC: nrows <= 128 (one or two 64-row tiles) and so many slabs that the few tiles would walk them one
// after the other (embed_layer-0 of a 64-chunk training minibatch: 96 slabs on 4 workgroups = 168 us for 0.2 GFLOP).
static int splitk_groups(int nrows, int in_dim, int out_dim)
{
    if (nrows <= 0 || nrows > 128 || in_dim < 16 * BK) return 1;
    const int chunks = (in_dim + BK - 1) / BK;
    const int tiles = ((nrows + 63) / 64) * ((out_dim + BN - 1) / BN);
    int per = (chunks * tiles + 255) / 256;             // ~ one workgroup per CU
    if (per < 2) per = 2;
    return (chunks + per - 1) / per;
}

size_t xv_fc_splitk_workspace_bytes(int nrows, int in_dim, int out_dim)
{
    const int g = splitk_groups(nrows, in_dim, out_dim);
    return g > 1 ? (size_t)g * nrows * out_dim * sizeof(float) : 0;
}

int xv_fc_splitk_f32(const float *x, int nrows, int in_dim, const float *wp, const float *bias, const float *bn_scale,
                     const float *bn_shift, int act_kind, const float *act_alpha, int out_dim, float *y, float *y_preact, void *workspace,
                     void *stream)
{
    const int g = splitk_groups(nrows, in_dim, out_dim);
    if (g <= 1) return xv_fc_f32(x, nrows, in_dim, wp, bias, bn_scale, bn_shift, act_kind, act_alpha, out_dim, y, y_preact, stream);
    if (!x || !wp || (!y && !y_preact) || !workspace) return fail(XV_ERR_BAD_ARG, "fc_splitk: NULL pointer");
    if (act_kind < XV_ACT_NONE || act_kind > XV_ACT_PRELU) return fail(XV_ERR_BAD_ARG, "fc_splitk: unknown act_kind");
    if ((act_kind == XV_ACT_LRELU || act_kind == XV_ACT_PRELU) && !act_alpha) return fail(XV_ERR_BAD_ARG, "fc_splitk: act_alpha is NULL");
    GemmParams p{};
    p.x = x; p.R = nrows; p.cin = in_dim; p.ldx = in_dim; p.wp = wp;
    p.act = XV_ACT_NONE; p.K = 1; p.dil = 1; p.cout = out_dim; p.ldy = out_dim;
    p.ypre = (float *)workspace;                        // (launch_gemm wants an output; the split-K epilogue redirects it per group)
    p.k_splits = g; p.part = (float *)workspace; p.part_stride = (long)nrows * out_dim;
    int rc = launch_gemm(p, (hipStream_t)stream);
    if (rc) return rc;
    const size_t n = (size_t)nrows * out_dim;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float *)workspace,
                       (long)nrows * out_dim, g, nrows, out_dim, bias, bn_scale, bn_shift, act_kind, act_alpha, y, out_dim, y_preact, out_dim);
    return launch_status("splitk_reduce_kernel");
}

void xv_internal_set_error(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }

}  // extern "C"
