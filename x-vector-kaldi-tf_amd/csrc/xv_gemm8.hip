// xv_gemm8.hip -- the hidden frame-level layers (tf.nn.conv1d 'SAME' + bias + activation + BN-eval, local/tf/models.py:54-76)
// in the "f16bf8" arithmetic: x*w = xh*wh (fp16 MFMA) + 2^-11 (xl8*wh8 + xh8*wl8) (ONE block-scaled 8-bit MFMA whose K = 64
// carries both cross terms of a 32-channel slab) -- 128 MFMA passes per stage and wave where the bf16x3 kernel of
// xv_gemm3.hip spends 192.  Representation, accuracy and range rules: xv_split8.h.
//
// Everything around the arithmetic is the design of tdnn_gemm_bf16x3_kernel, unchanged on purpose:
// implicit im2col over a (BM + (K-1)d)-row halo tile that all K taps of a 32-channel slab re-use, operands fed by direct
// global->LDS DMA from pre-formatted buffers (128 bytes per row-slab, 16 KB weight tile per stage, XOR-swizzled 16-byte
// slots), WM x 2 waves of 64 x 64 sub-tiles, XCD-aware tile order, a register-level software pipeline with one barrier per
// stage, the epilogue through an fp32 LDS tile.  Per stage and wave:
//     phase 1:  8 fp16 MFMAs (32x32x16: 2 k-steps x 2 x 2 tiles) on set F   | 8 ds_read_b128: set G = 8-bit fragments of stage s
//     barrier
//     phase 2:  4 scaled 8-bit MFMAs (32x32x64) on set G | DMA of stage s+2 | 8 ds_read_b128: set F = fp16 fragments of stage s+1
// 8-bit fragment of lane (row = lane & 31, half = lane >> 5): slots 4+2*half and 5+2*half of the row-slab = channels
// 16*half .. 16*half+15 as [8 x l8 | 8 x h8] twice -- and the weight tile holds [8 x h8 | 8 x l8] at the same positions.
//
// This file: the 128 / 256 x 128 kernel, launch_gemm8 (argument checks and the tile choice), the weight packer, the split8 codec
// and the entry points.  The 256 x 256 tile lives in xv_gemm8_wide.hip and xv_gemm8_wide16.hip; what the three share: xv_gemm8.h.
#include "xv_gemm8.h"

namespace {

constexpr int T_LD = BN + 4;            // epilogue fp32 tile row (floats)

// (A ring of THREE weight tiles with the DMA issued three stages ahead and a counted s_waitcnt vmcnt was measured on the
// 256-row form: no gain -- DMA latency is not what parks the waves -- so two buffers and vmcnt(0) it is.)
constexpr int g8_ring(int, int) { return 2; }           // weight tiles in LDS
constexpr int g8_oper_bytes(int kt, int wm) { return 2 * (wm * 64 + MAX_SPAN) * SROW + g8_ring(kt, wm) * B_BYTES; }
constexpr int g8_tile_bytes(int wm) { return wm * 64 * T_LD * 4; }
constexpr int g8_mask_off(int kt, int wm) { return g8_oper_bytes(kt, wm) > g8_tile_bytes(wm) ? g8_oper_bytes(kt, wm) : g8_tile_bytes(wm); }
constexpr size_t g8_lds_bytes(int kt, int wm) { return (size_t)g8_mask_off(kt, wm) + wm * 64 + 4 * BN * sizeof(float); }

template <int KT, bool POOL, int WM>
__global__ __launch_bounds__(WM * 128, 2) void tdnn_gemm_f16bf8_kernel(const Gemm8Params p)
{
    constexpr int NW = 2 * WM;
    constexpr int NT = NW * 64;
    constexpr int BM = WM * 64;
    constexpr int A_ROWS = BM + MAX_SPAN;
    constexpr int A_BYTES = A_ROWS * SROW;
    constexpr int BP = 16 / NW;                        // 1 KB pieces of a weight tile per wave
    constexpr int RING = g8_ring(KT, WM);              // weight tiles in LDS
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char *Abuf = lds;                                  // [2][A_ROWS][128 B]
    char *Bbuf = lds + 2 * A_BYTES;                    // [RING][fp16 plane 8 KB | 8-bit plane 8 KB]
    uint8_t *Ms = reinterpret_cast<uint8_t *>(lds + g8_mask_off(KT, WM));
    float *Ps = reinterpret_cast<float *>(lds + g8_mask_off(KT, WM) + BM);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;

    // XCD-aware tile order: every XCD gets a contiguous run of logical tile ids, column tiles fastest
    const int nwg = p.n_mt * p.n_nt;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, idx = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    const int mt = wg / p.n_nt, nt = wg - mt * p.n_nt;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;

    const int span = (KT - 1) * p.dil;
    const int left = span >> 1;
    const int n_stages = p.n_chunks * KT;
    const int goff = (int)((m0 - left) & 15);          // LDS row lr <-> global row gr: (gr & 15) == (lr + goff) & 15

    if (tid < BM) {
        const long gr = m0 + tid;
        Ms[tid] = (gr < p.R) ? (p.valid ? p.valid[gr] : (uint8_t)1) : (uint8_t)0;
    }
    if (tid >= BM && tid < BM + BN) {                  // [bias | BN scale | BN shift | alpha] of the tile's columns
        const int c = tid - BM, gc = n0 + c;
        const bool ok = gc < p.cout;
        Ps[c] = (ok && p.bias) ? p.bias[gc] : 0.f;
        Ps[BN + c] = ok ? (p.scale ? p.scale[gc] : 1.f) : 0.f;
        Ps[2 * BN + c] = (ok && p.shift) ? p.shift[gc] : 0.f;
        Ps[3 * BN + c] = p.act == XV_ACT_NONE ? 1.f : p.act == XV_ACT_LRELU ? p.alpha[0]
                       : (p.act == XV_ACT_PRELU && ok) ? p.alpha[gc] : 0.f;
    }

    const size_t xrow_bytes = (size_t)p.xchunks * SROW;
    const int arow0 = wr * 64 + (lane & 31);
    const int brow = wc * 64 + (lane & 31);
    const int kh = lane >> 5;
    const int boff0 = brow * 64;
    const int bsw0 = (brow >> 2) & 3;                  // (brow + 32) has the same swizzle

    // ---- prologue: the first RING weight tiles and the first halo tile(s) ------------------------------------------
    const uint8_t *bbase = p.wt + (size_t)nt * n_stages * B_BYTES + wave * (BP * 1024) + lane * 16;
    auto dma_b = [&](int stage, int buf) {
        const uint8_t *src = bbase + (size_t)(stage < n_stages ? stage : n_stages - 1) * B_BYTES;
        char *dst = Bbuf + buf * B_BYTES + wave * (BP * 1024);
#pragma unroll
        for (int j = 0; j < BP; ++j) XV_GLDS16(src + j * 1024, dst + j * 1024);
    };
    const uint8_t *abase = p.x + (m0 - left + (lane >> 3)) * (long)xrow_bytes + (lane & 7) * 16;
    constexpr int NP = KT == 1 ? BM / 8 : BM / 8 + 1;   // 8-row (1 KB) pieces of a halo tile
    auto dma_a_slab = [&](int chunk) {                  // whole halo tile of one slab (prologue only)
        char *dst = Abuf + (chunk & 1) * A_BYTES;
        for (int piece = wave; piece < NP; piece += NW)
            XV_GLDS16(abase + (size_t)chunk * SROW + (size_t)piece * 8 * xrow_bytes, dst + piece * 1024);
    };
#pragma unroll
    for (int j = 0; j < RING; ++j) dma_b(j, j);
    dma_a_slab(0);
    if (KT == 1 && n_stages > 1) dma_a_slab(1);
    if constexpr (KT > 1)
        if (p.tapbias && tid < BM) Ms[tid] = gemm8_tap_flags<KT>(p, m0 + tid, left);        // (xv_gemm8.h)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
    struct FragsH {           // fp16 fragments of both k-steps of a stage: 8 x 4 VGPRs
        xv_f16x8 a0[2], a1[2], b0[2], b1[2];
    };
    struct FragsX {           // 8-bit fragments of a stage: 4 x 8 VGPRs
        xv_i32x8 a0, a1, b0, b1;
    };
    int scale_a = XV_SPLIT8_E8M0, scale_b = 127;
    asm volatile("" : "+v"(scale_a), "+v"(scale_b));        // keep them in VGPRs (a literal would be read as an fp32 constant)

    // per-tap, per-lane fragment addresses in A buffer 0.  Slot T of a row sits at ((T ^ sw) << 4):
    //   fp16, k-step ks:  T = 2 ks + kh        ->  pa ^ (ks << 5)
    //   8-bit, part e:    T = 4 + 2 kh + e     ->  px ^ (e << 4)
    int pa[KT], px[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const int lr0 = arow0 + t * p.dil;
        const int sw = ((lr0 + goff) & 15) >> 1;
        pa[t] = lr0 * SROW + ((sw ^ kh) << 4);
        px[t] = lr0 * SROW + ((sw ^ (4 + 2 * kh)) << 4);
    }
    int pb[2];
    pb[0] = 2 * A_BYTES + boff0 + ((kh ^ bsw0) << 4);
    pb[1] = 2 * A_BYTES + boff0 + (((2 + kh) ^ bsw0) << 4);
    const int pbx = 2 * A_BYTES + B_PLANE + boff0 + (((2 * kh) ^ bsw0) << 4);

    auto load_h = [&](FragsH &X, int abase_, int bbase) {        // abase_ = pa[t] + A buffer offset, bbase = B buffer offset
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const char *a = lds + (abase_ ^ (ks << 5));
            const char *b = lds + pb[ks] + bbase;
            X.a0[ks] = *reinterpret_cast<const xv_f16x8 *>(a);
            X.a1[ks] = *reinterpret_cast<const xv_f16x8 *>(a + 32 * SROW);
            X.b0[ks] = *reinterpret_cast<const xv_f16x8 *>(b);
            X.b1[ks] = *reinterpret_cast<const xv_f16x8 *>(b + 32 * 64);
        }
    };
    auto cat = [](xv_i32x4 u, xv_i32x4 v) { return __builtin_shufflevector(u, v, 0, 1, 2, 3, 4, 5, 6, 7); };
    auto load_x = [&](FragsX &X, int abase_, int bbase) {        // abase_ = px[t] + A buffer offset
        const char *a = lds + abase_, *a2 = lds + (abase_ ^ 16);
        const char *b = lds + pbx + bbase, *b2 = lds + ((pbx + bbase) ^ 16);
        X.a0 = cat(*reinterpret_cast<const xv_i32x4 *>(a), *reinterpret_cast<const xv_i32x4 *>(a2));
        X.a1 = cat(*reinterpret_cast<const xv_i32x4 *>(a + 32 * SROW), *reinterpret_cast<const xv_i32x4 *>(a2 + 32 * SROW));
        X.b0 = cat(*reinterpret_cast<const xv_i32x4 *>(b), *reinterpret_cast<const xv_i32x4 *>(b2));
        X.b1 = cat(*reinterpret_cast<const xv_i32x4 *>(b + 32 * 64), *reinterpret_cast<const xv_i32x4 *>(b2 + 32 * 64));
    };
    auto mma_h = [&](const FragsH &X) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            acc00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(X.a0[ks], X.b0[ks], acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(X.a0[ks], X.b1[ks], acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(X.a1[ks], X.b0[ks], acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(X.a1[ks], X.b1[ks], acc11, 0, 0, 0);
        }
    };
    auto mma_x = [&](const FragsX &X) {                          // cbsz = blgp = 1: both operands bf8 (e5m2)
        acc00 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(X.a0, X.b0, acc00, 1, 1, 0, scale_a, 0, scale_b);
        acc01 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(X.a0, X.b1, acc01, 1, 1, 0, scale_a, 0, scale_b);
        acc10 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(X.a1, X.b0, acc10, 1, 1, 0, scale_a, 0, scale_b);
        acc11 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(X.a1, X.b1, acc11, 1, 1, 0, scale_a, 0, scale_b);
    };

    // A-halo DMA schedule (as in tdnn_gemm_bf16x3_kernel): the NS one-piece-per-wave slots of the NEXT slab's halo tile are
    // dealt to taps 0..K-2 of the current slab as evenly as possible, early taps first
    constexpr int DT = KT == 1 ? 1 : KT - 1;
    constexpr int NS = (NP + NW - 1) / NW;
    constexpr int PW = (NS + DT - 1) / DT;
    auto slots_of = [](int t) constexpr { return t < DT ? (NS + DT - 1 - t) / DT : 0; };
    auto slot_base = [](int t) constexpr { int b = 0; for (int u = 0; u < t; ++u) b += (NS + DT - 1 - u) / DT; return b; };
    const uint32_t rowstep = 8u * (uint32_t)xrow_bytes;
    uint32_t ag_off[DT][PW], al_off[DT][PW];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int j = 0; j < PW; ++j) {
            int piece = (slot_base(t) + j) * NW + wave;
            piece = piece < NP ? piece : NP - 1;
            ag_off[t][j] = (uint32_t)piece * rowstep;
            al_off[t][j] = (uint32_t)piece * 1024u;
        }
    const uint8_t *bnext = bbase + (size_t)(RING < n_stages ? RING : n_stages - 1) * B_BYTES;     // tile of stage min(s+RING, last)
    int bcur = 0, bnxt = B_BYTES;                        // ring offsets of the weight tiles of stages s and s+1

    FragsH F;
    FragsX G;
    load_h(F, pa[0], 0);

    int s = 0;
    for (int c = 0; c < p.n_chunks; ++c) {
        const int abuf = (c & 1) * A_BYTES;
        const int abuf_n = A_BYTES - abuf;
        const int cn = (c + 1 < p.n_chunks) ? c + 1 : p.n_chunks - 1;
        const uint8_t *anext = abase + (size_t)cn * SROW;
        char *adst_n = Abuf + (cn & 1) * A_BYTES;
        auto tap = [&](auto TT) {
            constexpr int t = decltype(TT)::value;
            const int bbuf = bcur;
            // ---- phase 1: G <- 8-bit fragments of stage s, interleaved with the 8 fp16 MFMAs on F -------------------
            load_x(G, px[t] + abuf, bbuf);
            mma_h(F);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // 1 DS read
            }
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();                  // stage s fully read by everybody, stage s+1 landed
            // ---- phase 2: DMA(s+2), F <- fp16 fragments of stage s+1, 4 scaled 8-bit MFMAs on G -----------------------
            {
                char *dst = Bbuf + bbuf + wave * (BP * 1024);    // one M0; the immediate advances source AND destination
                XV_GLDS16_OFF(bnext, dst, 0);
                XV_GLDS16_OFF(bnext, dst, 1024);
                if constexpr (BP == 4) {
                    XV_GLDS16_OFF(bnext, dst, 2048);
                    XV_GLDS16_OFF(bnext, dst, 3072);
                }
                bnext += (s + RING + 1 < n_stages) ? B_BYTES : 0;
            }
            if constexpr (KT == 1) {
                const int ca = (s + 2 < p.n_chunks) ? s + 2 : p.n_chunks - 1;
                const uint8_t *ag = abase + (size_t)ca * SROW;
                char *adst = Abuf + (ca & 1) * A_BYTES;
#pragma unroll
                for (int j = 0; j < PW; ++j) XV_GLDS16(ag + ag_off[0][j], adst + al_off[0][j]);
            } else if constexpr (t < DT) {
#pragma unroll
                for (int j = 0; j < slots_of(t); ++j) XV_GLDS16(anext + ag_off[t][j], adst_n + al_off[t][j]);
            }
            if constexpr (t + 1 < KT) load_h(F, pa[t + 1] + abuf, bnxt);
            else load_h(F, pa[0] + abuf_n, bnxt);                 // first tap of the next slab (tail: harmless read)
            mma_x(G);
            constexpr int NV = BP + (KT == 1 ? PW : slots_of(t));
            // per scaled MFMA (64 cycles): its share of the LDS-DMA pieces and 2 DS reads
#define XV_G8_GROUP(i)                                                              \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                      \
            if constexpr ((NV + 3 - (i)) / 4 > 0) __builtin_amdgcn_sched_group_barrier(0x020, (NV + 3 - (i)) / 4, 0); \
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            XV_G8_GROUP(0) XV_G8_GROUP(1) XV_G8_GROUP(2) XV_G8_GROUP(3)
#undef XV_G8_GROUP
            __builtin_amdgcn_sched_barrier(0);
            ++s;
            bcur = bnxt;
            bnxt = bnxt + B_BYTES == RING * B_BYTES ? 0 : bnxt + B_BYTES;
        };
        for_taps<0, KT>(tap);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- epilogue: accumulators -> LDS fp32 tile (the operand buffers are dead after the last barrier) ------
    float *T = reinterpret_cast<float *>(lds);
    {
        const int col = wc * 64 + (lane & 31);
        const int rowb = wr * 64 + 4 * (lane >> 5);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int rr = rowb + (reg & 3) + 8 * (reg >> 2);
            T[rr * T_LD + col] = acc00[reg];
            T[rr * T_LD + col + 32] = acc01[reg];
            T[(rr + 32) * T_LD + col] = acc10[reg];
            T[(rr + 32) * T_LD + col + 32] = acc11[reg];
        }
    }
    __syncthreads();

    const int cg = tid & 15;                            // 8-channel group of the 128-column tile
    const int gc0 = n0 + cg * 8;
    float bias[8], sc[8], sh[8], al[8];
    {
        const f32x4 *P4 = reinterpret_cast<const f32x4 *>(Ps) + cg * 2;
        const f32x4 q0 = P4[0], q1 = P4[1], q2 = P4[BN / 4], q3 = P4[BN / 4 + 1], q4 = P4[2 * BN / 4], q5 = P4[2 * BN / 4 + 1],
                    q6 = P4[3 * BN / 4], q7 = P4[3 * BN / 4 + 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bias[i] = q0[i]; bias[4 + i] = q1[i];
            sc[i] = q2[i]; sc[4 + i] = q3[i];
            sh[i] = q4[i]; sh[4 + i] = q5[i];
            al[i] = q6[i]; al[4 + i] = q7[i];
        }
    }
    const bool lrelu = p.act == XV_ACT_LRELU;           // tf.nn.leaky_relu is max(alpha*z, z) for ANY alpha
    auto act3 = [&](auto MODE, float z, float a) {     // 0: max(z,0) + alpha*min(z,0)   1: leaky max(alpha*z, z)   2: plain ReLU
        constexpr int mode = decltype(MODE)::value;
        return mode == 1 ? fmaxf(a * z, z) : mode == 2 ? fmaxf(z, 0.f) : fmaxf(z, 0.f) + a * fminf(z, 0.f);
    };
    auto by_mode = [&](auto &&f) {
        if (lrelu) f(std::integral_constant<int, 1>{});
        else if (p.act == XV_ACT_RELU) f(std::integral_constant<int, 2>{});
        else f(std::integral_constant<int, 0>{});
    };
    if constexpr (POOL) {
        // thread = (8-row block of the tile, 8 channels): (mean, M2) of the block's valid rows, shifted by its first row
        const int blk = tid >> 4;
        if (m0 + blk * 8 >= p.R) return;
        float v0[8], s1[8], s2[8];
        float n = 0.f;
        f32x4 tv[8][2];
        float keep[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int lr = blk * 8 + j;
            tv[j][0] = *reinterpret_cast<const f32x4 *>(T + lr * T_LD + cg * 8);
            tv[j][1] = *reinterpret_cast<const f32x4 *>(T + lr * T_LD + cg * 8 + 4);
            keep[j] = Ms[lr] ? 1.f : 0.f;
        }
        if constexpr (KT > 1)
            if (p.tapbias) gemm8_drop_missing_taps(p, Ms, gc0, tv, [&](int j) { return blk * 8 + j; });
        __builtin_amdgcn_sched_barrier(0);
        by_mode([&](auto MODE) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                n += keep[j];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float z = (i < 4 ? tv[j][0][i] : tv[j][1][i - 4]) + bias[i];
                    const float v = act3(MODE, z, al[i]) * sc[i] + sh[i];
                    if (j == 0) { v0[i] = v; s1[i] = 0.f; s2[i] = 0.f; }
                    else {
                        const float d = keep[j] != 0.f ? v - v0[i] : 0.f;      // (a select: a row past R may hold NaN, and NaN * 0 is NaN)
                        s1[i] += d;
                        s2[i] += d * d;
                    }
                }
            }
        });
        const float rn = n > 0.f ? 1.f / n : 0.f;
        float mean[8], m2[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            mean[i] = n > 0.f ? v0[i] + s1[i] * rn : 0.f;
            m2[i] = fmaxf(s2[i] - s1[i] * s1[i] * rn, 0.f);
        }
        float *o = p.blk + ((size_t)((m0 >> 3) + blk) * 2) * p.cout + gc0;
        if (gc0 + 8 <= p.cout && !(p.cout & 3)) {
            *reinterpret_cast<f32x4 *>(o) = (f32x4){mean[0], mean[1], mean[2], mean[3]};
            *reinterpret_cast<f32x4 *>(o + 4) = (f32x4){mean[4], mean[5], mean[6], mean[7]};
            *reinterpret_cast<f32x4 *>(o + p.cout) = (f32x4){m2[0], m2[1], m2[2], m2[3]};
            *reinterpret_cast<f32x4 *>(o + p.cout + 4) = (f32x4){m2[4], m2[5], m2[6], m2[7]};
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (gc0 + i < p.cout) { o[i] = mean[i]; o[p.cout + i] = m2[i]; }
        }
        return;
    } else {
        // all 16 LDS reads first (a round trip costs ~1 us under load -- pay it once, not once per row)
        f32x4 tv[8][2];
        float keep[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int lr = (tid >> 4) + (NT / 16) * j;
            tv[j][0] = *reinterpret_cast<const f32x4 *>(T + lr * T_LD + cg * 8);
            tv[j][1] = *reinterpret_cast<const f32x4 *>(T + lr * T_LD + cg * 8 + 4);
            keep[j] = Ms[lr] ? 1.f : 0.f;
        }
        if constexpr (KT > 1)
            if (p.tapbias) gemm8_drop_missing_taps(p, Ms, gc0, tv, [&](int j) { return (tid >> 4) + (NT / 16) * j; });
        __builtin_amdgcn_sched_barrier(0);
        if (p.y_format != XV_FMT_F32 && n0 + BN <= p.cout) {
            // hidden layers: full-width tile into a split format.  Rows >= R of the last tile land in the buffer's zero
            // padding (XV_SPLIT_PAD_AFTER >= BM) and are written as zeros (keep == 0).
            const int ch = gc0 >> 5, slot = cg & 3;
            char *ybase = reinterpret_cast<char *>(p.y) + (size_t)ch * SROW;
            const size_t yrow = (size_t)p.ychunks * SROW;
            float amax = 0.f;
            auto rows = [&](auto MODE, auto Y8) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const long gr = m0 + (tid >> 4) + (NT / 16) * j;
                    float v[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const float z = (i < 4 ? tv[j][0][i] : tv[j][1][i - 4]) + bias[i];
                        v[i] = keep[j] != 0.f ? act3(MODE, z, al[i]) * sc[i] + sh[i] : 0.f;
                    }
                    const int sw = (int)(gr >> 1) & 7;
                    char *row = ybase + (size_t)gr * yrow;
                    if constexpr (decltype(Y8)::value) {
                        xv_f16x8 hi;
                        xv_i32x4 x8;
                        xv_split8_encode8<true>(v, hi, x8, amax);
                        __builtin_nontemporal_store(hi, reinterpret_cast<xv_f16x8 *>(row + ((slot ^ sw) << 4)));
                        __builtin_nontemporal_store(x8, reinterpret_cast<xv_i32x4 *>(row + (((4 + slot) ^ sw) << 4)));
                    } else {
                        bf16x8 hi, lo;
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            hi[i] = (__bf16)v[i];
                            lo[i] = (__bf16)(v[i] - (float)hi[i]);
                        }
                        __builtin_nontemporal_store(hi, reinterpret_cast<bf16x8 *>(row + ((slot ^ sw) << 4)));
                        __builtin_nontemporal_store(lo, reinterpret_cast<bf16x8 *>(row + (((4 + slot) ^ sw) << 4)));
                    }
                }
            };
            if (p.y_format == XV_FMT_SPLIT8) {
                by_mode([&](auto MODE) { rows(MODE, std::true_type{}); });
                if (amax > XV_SPLIT8_MAX && p.status) atomicOr(p.status, 1);
            } else {
                by_mode([&](auto MODE) { rows(MODE, std::false_type{}); });
            }
            return;
        }
        // general path: fp32 rows, or a ragged last column tile of a split output
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int lr = (tid >> 4) + (NT / 16) * j;
            const long gr = m0 + lr;
            if (gr >= p.R) continue;
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float z = (i < 4 ? tv[j][0][i] : tv[j][1][i - 4]) + bias[i];
                const float a = lrelu ? fmaxf(al[i] * z, z) : fmaxf(z, 0.f) + al[i] * fminf(z, 0.f);
                v[i] = keep[j] != 0.f ? a * sc[i] + sh[i] : 0.f;
            }
            if (p.y_format == XV_FMT_F32) {
                float *o = reinterpret_cast<float *>(p.y) + (size_t)gr * p.ldy + gc0;
                if (gc0 + 8 <= p.cout && !(p.ldy & 3)) {
                    __builtin_nontemporal_store((f32x4){v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4 *>(o));
                    __builtin_nontemporal_store((f32x4){v[4], v[5], v[6], v[7]}, reinterpret_cast<f32x4 *>(o + 4));
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (gc0 + i < p.cout) o[i] = v[i];
                }
            } else {
                const int ch = gc0 >> 5;
                if (ch >= p.ychunks) continue;
                const int sw = (int)(gr >> 1) & 7, slot = cg & 3;
                char *row = reinterpret_cast<char *>(p.y) + ((size_t)gr * p.ychunks + ch) * SROW;
                if (p.y_format == XV_FMT_SPLIT8) {
                    xv_f16x8 hi;
                    xv_i32x4 x8;
                    xv_split8_encode8<true>(v, hi, x8, amax);
                    *reinterpret_cast<xv_f16x8 *>(row + ((slot ^ sw) << 4)) = hi;
                    *reinterpret_cast<xv_i32x4 *>(row + (((4 + slot) ^ sw) << 4)) = x8;
                } else {
                    bf16x8 hi, lo;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        hi[i] = (__bf16)v[i];
                        lo[i] = (__bf16)(v[i] - (float)hi[i]);
                    }
                    *reinterpret_cast<bf16x8 *>(row + ((slot ^ sw) << 4)) = hi;
                    *reinterpret_cast<bf16x8 *>(row + (((4 + slot) ^ sw) << 4)) = lo;
                }
            }
        }
        if (amax > XV_SPLIT8_MAX && p.status) atomicOr(p.status, 1);
    }
}

typedef void (*gemm8_fn)(const Gemm8Params);
struct Gemm8Kernel {
    int kt;
    bool pool;
    int wm;
    gemm8_fn fn;
};
#define XV_G8(KT, POOL, WM) {KT, POOL, WM, tdnn_gemm_f16bf8_kernel<KT, POOL, WM>}
const Gemm8Kernel GEMM8_KERNELS[] = {
    XV_G8(1, false, 2), XV_G8(3, false, 2), XV_G8(5, false, 2), XV_G8(7, false, 2),
    XV_G8(1, true, 2),  XV_G8(3, true, 2),  XV_G8(5, true, 2),  XV_G8(7, true, 2),
    XV_G8(1, false, 4), XV_G8(3, false, 4), XV_G8(5, false, 4), XV_G8(7, false, 4),
    XV_G8(1, true, 4),  XV_G8(3, true, 4),  XV_G8(5, true, 4),  XV_G8(7, true, 4),
};
#undef XV_G8

std::atomic<int> g_tile_rows8{0};

int launch_gemm8(const Gemm8Params &p0, hipStream_t st)
{
    Gemm8Params p = p0;
    if (p.R <= 0 || p.cout <= 0) return 0;
    if (p.cin <= 0 || p.dil <= 0) return fail(XV_ERR_BAD_ARG, "tdnn_f16bf8: dims > 0");
    const int span = (p.K - 1) * p.dil;
    if ((p.K != 1 && p.K != 3 && p.K != 5 && p.K != 7) || (p.K > 1 && (span < 2 || span > MAX_SPAN)))
        return fail(XV_ERR_UNSUPPORTED, "tdnn_f16bf8: supports K in {1,3,5,7} with (K-1)*dilation <= 8");
    if ((p.act == XV_ACT_LRELU || p.act == XV_ACT_PRELU) && !p.alpha) return fail(XV_ERR_BAD_ARG, "tdnn_f16bf8: act_alpha is NULL");
    if ((((uintptr_t)p.x) | ((uintptr_t)p.wt)) & 15) return fail(XV_ERR_BAD_ARG, "tdnn_f16bf8: input and packed weights must be 16-byte aligned");
    if (p.tapbias) {
        // a K = 1 layer has no neighbours and its kernels no per-row bias: its share of the producer's shift is all in ``bias``
        if (p.K == 1) return fail(XV_ERR_UNSUPPORTED, "tdnn_f16bf8: a K = 1 layer takes no tap_bias table");
        // the epilogue reads 8 channels of a tap with two 16-byte loads
        if ((p.cout & 7) || (((uintptr_t)p.tapbias) & 15)) return fail(XV_ERR_UNSUPPORTED, "tdnn_f16bf8: tap_bias needs Cout % 8 == 0 and 16-byte alignment");
    }
    p.n_chunks = (p.cin + BK - 1) / BK;
    p.xchunks = p.n_chunks;
    if (p.y) {
        if (((uintptr_t)p.y) & 15) return fail(XV_ERR_BAD_ARG, "tdnn_f16bf8: output must be 16-byte aligned");
        if (p.y_format == XV_FMT_F32) {
            if (p.ldy < p.cout) return fail(XV_ERR_BAD_ARG, "tdnn_f16bf8: ldy < cout");
        } else {
            p.ychunks = (p.cout + 31) / 32;
        }
    }
    p.n_nt = (p.cout + BN - 1) / BN;
    // tile: 128 x 128 (4 waves, two workgroups per CU), 256 x 128 (8 waves) or 256 x 256 (8 waves of 128 x 64; K > 1,
    // Cout % 256 == 0, split-format or POOL output; on the 16 x 16 MFMA shapes where the number of slabs is even, else on the
    // 32 x 32 ones).  XV_TUNE_TILE_ROWS: 128 / 256 force the first two, 512 the 32 x 32 form of the third, 1024 the 16 x 16 form.
    int wm = 2;
    {
        const int want = g_tile_rows8.load(std::memory_order_relaxed);
        const bool wide_ok = p.K > 1 && (p.cout & 255) == 0 && (p.blk != nullptr || p.y_format != XV_FMT_F32);
        const bool big_enough = ((p.R + 255) / 256) * p.n_nt >= 512;
        // the 16 x 16 MFMA form of the 256 x 256 tile pairs (slab, tap) items over two slabs: an even number of slabs
        const bool w16_ok = wide_ok && (p.n_chunks & 1) == 0;
        const bool wide_pays = ((p.R + 255) / 256) * (p.cout / 256) >= 512;
        // The 16 x 16 form adds an element's products in another order than the 32 x 32 tiles (which agree among themselves bit for
        // bit), so a shape that can take it ALWAYS takes it, whatever the number of rows: an utterance's x-vector must not depend on
        // how many utterances share its batch -- on the sharding of a job over ranks, say (tests/test_gpu_eight_ranks.py: 8 ranks
        // write the single process's bytes).  A batch too small to fill the chip twice with 256 x 256 tiles loses a few per cent.
        if (w16_ok && (want == 1024 || want == 0)) wm = 16;
        else if (wide_ok && (want == 512 || want == 1024 || (want == 0 && wide_pays))) wm = 8;
        else if (want == 256 || (want == 0 && p.K >= 5 && big_enough)) wm = 4;
    }
    // the e2m3 forms exist in the 16 x 16 MFMA kernel only: split6 input in its main loop, split6 output in its form of wide_epilogue
    if (p.x_format == XV_FMT_SPLIT6 && wm != 16)
        return fail(XV_ERR_UNSUPPORTED, "tdnn_f16mx6: needs an even number of 32-channel slabs, K in {3,5,7}, Cout % 256 == 0 and a split-format or pooled output");
    if (p.y && p.y_format == XV_FMT_SPLIT6 && (wm != 16 || p.blk))
        return fail(XV_ERR_UNSUPPORTED, "tdnn_f16bf8: XV_FMT_SPLIT6 output needs the 16 x 16 MFMA form of the 256 x 256 tile (an even number of slabs, K in {3,5,7}, Cout % 256 == 0)");
    if (wm >= 8) {
        p.n_nt = p.cout / W_BN;
        p.n_mt = (int)((p.R + W_BM - 1) / W_BM);
    } else {
        p.n_mt = (int)((p.R + wm * 64 - 1) / (wm * 64));
    }
    if (wm == 16) return launch_gemm8_wide16(p, st);
    if (wm == 8) return launch_gemm8_wide(p, st);
    const Gemm8Kernel *k = nullptr;
    for (const Gemm8Kernel &e : GEMM8_KERNELS)
        if (e.kt == p.K && e.pool == (p.blk != nullptr) && e.wm == wm) k = &e;
    if (!k) return fail(XV_ERR_UNSUPPORTED, "tdnn_f16bf8: no kernel for this configuration");
    static std::atomic<unsigned long long> lds_done{0};
    if (const int rc = opt_in_dynamic_lds(lds_done, GEMM8_KERNELS, [](const Gemm8Kernel &e) { return std::make_pair(e.fn, g8_lds_bytes(e.kt, e.wm)); }))
        return rc;
    hipLaunchKernelGGL(k->fn, dim3((unsigned)(p.n_mt * p.n_nt)), dim3(wm * 128), g8_lds_bytes(p.K, wm), st, p);
    return launch_status("tdnn_gemm_f16bf8_kernel launch");
}

// w[K, cin, cout] fp32 -> tiled f16bf8 weights: tile (nt, chunk, tap) = 16 KB [fp16 plane 128 x 64 B][8-bit plane 128 x 64 B]
__global__ void pack_weights_f16bf8_kernel(const float *__restrict__ w, int K, int cin, int cout, int n_chunks,
                                           uint8_t *__restrict__ wt, size_t total)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // one (tile, col, 8-channel group)
    if (i >= total) return;
    const int g = (int)(i & 3);
    const int n = (int)((i >> 2) & 127);
    const size_t tile = i >> 9;
    const int tap = (int)(tile % K);
    const int chunk = (int)((tile / K) % n_chunks);
    const int nt = (int)(tile / ((size_t)K * n_chunks));
    const int gn = nt * 128 + n;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = chunk * 32 + g * 8 + e;
        v[e] = (c < cin && gn < cout) ? w[((size_t)tap * cin + c) * cout + gn] : 0.f;
    }
    xv_f16x8 hi;
    xv_i32x4 x8;
    float amax = 0.f;
    xv_split8_encode8<false>(v, hi, x8, amax);
    uint8_t *t = wt + tile * B_BYTES + n * 64 + ((g ^ ((n >> 2) & 3)) << 4);
    *reinterpret_cast<xv_f16x8 *>(t) = hi;
    *reinterpret_cast<xv_i32x4 *>(t + B_PLANE) = x8;
}

// The same tiles with the 8-bit plane as e2m3 blocks (xv_split6.h): column n, block c = channels 16c..16c+15 of the slab; slot c of the
// plane = dwords 0-3 of [clamp(w) | 2^11 lo], slot 2+c = [dword 4 | dword 5 | E8M0 byte | 0] -- the two 16-byte reads a lane of
// tdnn_gemm_f16bf8_wide16_kernel makes for K block (item, c).  The fp16 plane is xv_pack_weights_f16bf8's, bit for bit.
__global__ void pack_weights_f16mx6_kernel(const float *__restrict__ w, int K, int cin, int cout, int n_chunks,
                                           uint8_t *__restrict__ wt, size_t total)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // one (tile, col, block)
    if (i >= total) return;
    const int c = (int)(i & 1);
    const int n = (int)((i >> 1) & 127);
    const size_t tile = i >> 8;
    const int tap = (int)(tile % K);
    const int chunk = (int)((tile / K) % n_chunks);
    const int nt = (int)(tile / ((size_t)K * n_chunks));
    const int gn = nt * 128 + n;
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int ch = chunk * 32 + c * 16 + e;
        v[e] = (ch < cin && gn < cout) ? w[((size_t)tap * cin + ch) * cout + gn] : 0.f;
    }
    xv_f16x8 h0, h1;
    xv_u32x6 x6;
    int e8m0;
    float amax = 0.f;
    xv_split6_encode16<false>(v, h0, h1, x6, e8m0, amax);
    const int sw = (n >> 2) & 3;
    uint8_t *t = wt + tile * B_BYTES + n * 64;
    *reinterpret_cast<xv_f16x8 *>(t + (((2 * c) ^ sw) << 4)) = h0;
    *reinterpret_cast<xv_f16x8 *>(t + (((2 * c + 1) ^ sw) << 4)) = h1;
    *reinterpret_cast<xv_i32x4 *>(t + B_PLANE + ((c ^ sw) << 4)) = (xv_i32x4){(int)x6[0], (int)x6[1], (int)x6[2], (int)x6[3]};
    *reinterpret_cast<xv_i32x4 *>(t + B_PLANE + (((2 + c) ^ sw) << 4)) = (xv_i32x4){(int)x6[4], (int)x6[5], e8m0, 0};
}

// fp32 rows -> split6 / back (tests and tooling).  Element k of a block sits at bits [6k, 6k + 6) of its six dwords; the conversion
// instruction puts its first source's value i at element XV_SPLIT6_ELEM(0, i), its second source's at XV_SPLIT6_ELEM(1, i).
__global__ void split6_encode_kernel(const float *__restrict__ x, long R, int c, int ldx, uint8_t *__restrict__ xs, int chunks,
                                     int *status)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // one (row, slab, block)
    if (i >= (size_t)R * chunks * 2) return;
    const int b = (int)(i & 1);
    const int ch = (int)((i >> 1) % chunks);
    const long r = (long)(i / ((size_t)2 * chunks));
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int cc = ch * 32 + b * 16 + e;
        v[e] = cc < c ? x[(size_t)r * ldx + cc] : 0.f;
    }
    xv_f16x8 h0, h1;
    xv_u32x6 x6;
    int e8m0;
    float amax = 0.f;
    xv_split6_encode16<true>(v, h0, h1, x6, e8m0, amax);
    const int sw = (int)(r >> 1) & 7;
    uint8_t *row = xs + ((size_t)r * chunks + ch) * SROW;
    *reinterpret_cast<xv_f16x8 *>(row + (((2 * b) ^ sw) << 4)) = h0;
    *reinterpret_cast<xv_f16x8 *>(row + (((2 * b + 1) ^ sw) << 4)) = h1;
    *reinterpret_cast<xv_i32x4 *>(row + (((4 + b) ^ sw) << 4)) = (xv_i32x4){(int)x6[0], (int)x6[1], (int)x6[2], (int)x6[3]};
    *reinterpret_cast<xv_i32x4 *>(row + (((6 + b) ^ sw) << 4)) = (xv_i32x4){(int)x6[4], (int)x6[5], e8m0 - XV_SPLIT6_LO_EXP, 0};
    if (amax > XV_SPLIT8_MAX && status) atomicOr(status, 1);
}

__global__ void split6_decode_kernel(const uint8_t *__restrict__ xs, long R, int c, int chunks, float *__restrict__ x,
                                     float *__restrict__ cq, int ldx)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)R * c) return;
    const long r = (long)(i / c);
    const int cc = (int)(i - (size_t)r * c);
    const int ch = cc >> 5, k = cc & 31, b = k >> 4, e = k & 15;
    const int sw = (int)(r >> 1) & 7;
    const uint8_t *row = xs + ((size_t)r * chunks + ch) * SROW;
    const _Float16 h = *reinterpret_cast<const _Float16 *>(row + (((k >> 3) ^ sw) << 4) + (k & 7) * 2);
    const uint32_t *lo4 = reinterpret_cast<const uint32_t *>(row + (((4 + b) ^ sw) << 4));
    const uint32_t *hi4 = reinterpret_cast<const uint32_t *>(row + (((6 + b) ^ sw) << 4));
    const uint32_t d[7] = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], 0u};
    const float scale = __builtin_bit_cast(float, (hi4[2] & 0xffu) << 23);       // 2^(byte - 127): the 2^-11 is in the byte
    auto elem = [&](int pos) {
        const int bit = 6 * pos;
        const uint64_t w2 = (uint64_t)d[bit >> 5] | ((uint64_t)d[(bit >> 5) + 1] << 32);
        const uint32_t code = (uint32_t)(w2 >> (bit & 31)) & 63u;
        const int ex = (code >> 3) & 3, m = code & 7;
        const float mag = ex == 0 ? m * 0.125f : (1.f + m * 0.125f) * (float)(1 << (ex - 1));
        return (code & 32u) ? -mag : mag;
    };
    x[(size_t)r * ldx + cc] = (float)h + elem(XV_SPLIT6_ELEM(0, e)) * scale;
    if (cq) cq[(size_t)r * ldx + cc] = elem(XV_SPLIT6_ELEM(1, e)) * scale * XV_SPLIT8_LO_SCALE;
}

// fp32 rows -> split8 (tests / tooling; the layers write the format themselves)
__global__ void split8_encode_kernel(const float *__restrict__ x, long R, int c, int ldx, uint8_t *__restrict__ xs, int chunks,
                                     int *status)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // one (row, slab, 8-channel group)
    if (i >= (size_t)R * chunks * 4) return;
    const int g = (int)(i & 3);
    const int ch = (int)((i >> 2) % chunks);
    const long r = (long)(i / ((size_t)4 * chunks));
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int cc = ch * 32 + g * 8 + e;
        v[e] = cc < c ? x[(size_t)r * ldx + cc] : 0.f;
    }
    xv_f16x8 hi;
    xv_i32x4 x8;
    float amax = 0.f;
    xv_split8_encode8<true>(v, hi, x8, amax);
    const int sw = (int)(r >> 1) & 7;
    uint8_t *row = xs + ((size_t)r * chunks + ch) * SROW;
    *reinterpret_cast<xv_f16x8 *>(row + ((g ^ sw) << 4)) = hi;
    *reinterpret_cast<xv_i32x4 *>(row + (((4 + g) ^ sw) << 4)) = x8;
    if (amax > XV_SPLIT8_MAX && status) atomicOr(status, 1);
}

__global__ void split8_decode_kernel(const uint8_t *__restrict__ xs, long R, int c, int chunks, float *__restrict__ x, int ldx)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)R * c) return;
    const long r = (long)(i / c);
    const int cc = (int)(i - (size_t)r * c);
    const int ch = cc >> 5, k = cc & 31;
    const int sw = (int)(r >> 1) & 7;
    const uint8_t *row = xs + ((size_t)r * chunks + ch) * SROW;
    const _Float16 h = *reinterpret_cast<const _Float16 *>(row + (((k >> 3) ^ sw) << 4) + (k & 7) * 2);
    const uint8_t l = row[(((4 + (k >> 3)) ^ sw) << 4) + (k & 7)];
    x[(size_t)r * ldx + cc] = (float)h + xv_bf8_to_float(l) * (1.f / XV_SPLIT8_LO_SCALE);
}

}  // namespace

extern "C" {

void xv_internal_gemm8_tile_rows(int value) { g_tile_rows8.store(value, std::memory_order_relaxed); }

size_t xv_packed_weights_f16bf8_bytes(int K, int cin, int cout)
{
    if (K <= 0 || cin <= 0 || cout <= 0) return 0;
    return (size_t)((cout + BN - 1) / BN) * ((cin + BK - 1) / BK) * K * B_BYTES;
}

int xv_pack_weights_f16bf8(const float *w, int K, int cin, int cout, void *wt, void *stream)
{
    if (!w || !wt || K <= 0 || cin <= 0 || cout <= 0) return fail(XV_ERR_BAD_ARG, "pack_weights_f16bf8: bad argument");
    if (((uintptr_t)wt) & 15) return fail(XV_ERR_BAD_ARG, "pack_weights_f16bf8: wt must be 16-byte aligned");
    const int n_chunks = (cin + BK - 1) / BK;
    const size_t total = xv_packed_weights_f16bf8_bytes(K, cin, cout) / 32;     // one thread per 8-channel group (16 + 16 bytes)
    hipLaunchKernelGGL(pack_weights_f16bf8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, K,
                       cin, cout, n_chunks, (uint8_t *)wt, total);
    return launch_status("pack_weights_f16bf8_kernel");
}

size_t xv_packed_weights_f16mx6_bytes(int K, int cin, int cout)
{
    // what the 16 x 16 MFMA form of the 256 x 256 tile takes (launch_gemm8): an even number of slabs, K in {3,5,7}, Cout % 256 == 0
    if ((K != 3 && K != 5 && K != 7) || cin <= 0 || cout <= 0 || (cout & 255) || (((cin + BK - 1) / BK) & 1)) return 0;
    return xv_packed_weights_f16bf8_bytes(K, cin, cout);
}

int xv_pack_weights_f16mx6(const float *w, int K, int cin, int cout, void *wt, void *stream)
{
    if (!w || !wt) return fail(XV_ERR_BAD_ARG, "pack_weights_f16mx6: bad argument");
    if (((uintptr_t)wt) & 15) return fail(XV_ERR_BAD_ARG, "pack_weights_f16mx6: wt must be 16-byte aligned");
    const size_t bytes = xv_packed_weights_f16mx6_bytes(K, cin, cout);
    if (!bytes) return fail(XV_ERR_UNSUPPORTED, "pack_weights_f16mx6: needs K in {3,5,7}, an even number of 32-channel slabs and Cout % 256 == 0");
    const int n_chunks = (cin + BK - 1) / BK;
    const size_t total = bytes / 64;                   // one thread per block of 16 channels (32 + 32 bytes)
    hipLaunchKernelGGL(pack_weights_f16mx6_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, K,
                       cin, cout, n_chunks, (uint8_t *)wt, total);
    return launch_status("pack_weights_f16mx6_kernel");
}

int xv_split6_encode_f32(const float *x, int64_t R, int c, int ldx, void *xs, int32_t *status, void *stream)
{
    if (R <= 0) return 0;
    if (!x || !xs || c <= 0 || ldx < c) return fail(XV_ERR_BAD_ARG, "split6_encode: bad argument");
    if (((uintptr_t)xs) & 15) return fail(XV_ERR_BAD_ARG, "split6_encode: xs must be 16-byte aligned");
    const int chunks = (c + 31) / 32;
    const size_t n = (size_t)R * chunks * 2;
    hipLaunchKernelGGL(split6_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (long)R, c, ldx,
                       (uint8_t *)xs, chunks, (int *)status);
    return launch_status("split6_encode_kernel");
}

int xv_split6_decode_f32(const void *xs, int64_t R, int c, float *x, float *cq, int ldx, void *stream)
{
    if (R <= 0) return 0;
    if (!x || !xs || c <= 0 || ldx < c) return fail(XV_ERR_BAD_ARG, "split6_decode: bad argument");
    const size_t n = (size_t)R * c;
    hipLaunchKernelGGL(split6_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t *)xs, (long)R, c, (c + 31) / 32, x, cq, ldx);
    return launch_status("split6_decode_kernel");
}

int xv_split8_encode_f32(const float *x, int64_t R, int c, int ldx, void *xs, int32_t *status, void *stream)
{
    if (R <= 0) return 0;
    if (!x || !xs || c <= 0 || ldx < c) return fail(XV_ERR_BAD_ARG, "split8_encode: bad argument");
    if (((uintptr_t)xs) & 15) return fail(XV_ERR_BAD_ARG, "split8_encode: xs must be 16-byte aligned");
    const int chunks = (c + 31) / 32;
    const size_t n = (size_t)R * chunks * 4;
    hipLaunchKernelGGL(split8_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (long)R, c, ldx,
                       (uint8_t *)xs, chunks, (int *)status);
    return launch_status("split8_encode_kernel");
}

int xv_split8_decode_f32(const void *xs, int64_t R, int c, float *x, int ldx, void *stream)
{
    if (R <= 0) return 0;
    if (!x || !xs || c <= 0 || ldx < c) return fail(XV_ERR_BAD_ARG, "split8_decode: bad argument");
    const size_t n = (size_t)R * c;
    hipLaunchKernelGGL(split8_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t *)xs, (long)R, c, (c + 31) / 32, x, ldx);
    return launch_status("split8_decode_kernel");
}

// the layer with x in ``x_format`` (XV_FMT_SPLIT8: xv_tdnn_layer_f16bf8; XV_FMT_SPLIT6: xv_tdnn_layer_f16mx6)
static int tdnn_layer8(int x_format, const void *x, int64_t R, int cin, const void *wt, const float *bias, const float *bn_scale,
                       const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                       const uint8_t *row_valid, const float *tap_bias, void *y, int y_format, int ldy, int32_t *status, void *stream)
{
    if (!x || !wt || !y) return fail(XV_ERR_BAD_ARG, "tdnn_f16bf8: NULL pointer");
    if (act_kind < XV_ACT_NONE || act_kind > XV_ACT_PRELU) return fail(XV_ERR_BAD_ARG, "tdnn_f16bf8: unknown act_kind");
    if (y_format != XV_FMT_F32 && y_format != XV_FMT_SPLIT && y_format != XV_FMT_SPLIT8 && y_format != XV_FMT_SPLIT6)
        return fail(XV_ERR_BAD_ARG, "tdnn_f16bf8: unknown tensor format");
    Gemm8Params p{};
    p.x = (const uint8_t *)x; p.x_format = x_format; p.R = (long)R; p.cin = cin; p.wt = (const uint8_t *)wt;
    p.bias = bias; p.scale = bn_scale; p.shift = bn_shift; p.act = act_kind; p.alpha = act_alpha;
    p.K = K; p.dil = dilation; p.cout = cout; p.valid = row_valid; p.tapbias = tap_bias;
    p.y = y; p.y_format = y_format; p.ldy = ldy; p.status = (int *)status;
    return launch_gemm8(p, (hipStream_t)stream);
}

int xv_tdnn_layer_f16bf8(const void *x, int64_t R, int cin, const void *wt, const float *bias, const float *bn_scale,
                         const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                         const uint8_t *row_valid, const float *tap_bias, void *y, int y_format, int ldy, int32_t *status, void *stream)
{
    return tdnn_layer8(XV_FMT_SPLIT8, x, R, cin, wt, bias, bn_scale, bn_shift, act_kind, act_alpha, K, dilation, cout, row_valid, tap_bias,
                       y, y_format, ldy, status, stream);
}

int xv_tdnn_layer_f16mx6(const void *x, int64_t R, int cin, const void *wt, const float *bias, const float *bn_scale,
                         const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                         const uint8_t *row_valid, const float *tap_bias, void *y, int y_format, int ldy, int32_t *status, void *stream)
{
    return tdnn_layer8(XV_FMT_SPLIT6, x, R, cin, wt, bias, bn_scale, bn_shift, act_kind, act_alpha, K, dilation, cout, row_valid, tap_bias,
                       y, y_format, ldy, status, stream);
}

int xv_tdnn_layer_pool_f16bf8(const void *x, int64_t R, int cin, const void *wt, const float *bias, const float *bn_scale,
                              const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation, int cout,
                              const uint8_t *row_valid, const float *tap_bias, float *block_stats, void *stream)
{
    if (!x || !wt || !block_stats) return fail(XV_ERR_BAD_ARG, "tdnn_pool_f16bf8: NULL pointer");
    if (act_kind < XV_ACT_NONE || act_kind > XV_ACT_PRELU) return fail(XV_ERR_BAD_ARG, "tdnn_pool_f16bf8: unknown act_kind");
    if (((uintptr_t)block_stats) & 15) return fail(XV_ERR_BAD_ARG, "tdnn_pool_f16bf8: block_stats must be 16-byte aligned");
    Gemm8Params p{};
    p.x = (const uint8_t *)x; p.R = (long)R; p.cin = cin; p.wt = (const uint8_t *)wt;
    p.bias = bias; p.scale = bn_scale; p.shift = bn_shift; p.act = act_kind; p.alpha = act_alpha;
    p.K = K; p.dil = dilation; p.cout = cout; p.valid = row_valid; p.tapbias = tap_bias;
    p.x_format = XV_FMT_SPLIT8; p.blk = block_stats; p.y_format = XV_FMT_F32;
    return launch_gemm8(p, (hipStream_t)stream);
}

}  // extern "C"
