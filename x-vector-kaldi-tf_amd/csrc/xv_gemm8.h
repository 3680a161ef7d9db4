// xv_gemm8.h -- what the three translation units of the f16bf8 GEMM family share (internal, not ABI): xv_gemm8.hip (the
// 128 / 256 x 128 kernel, launch_gemm8, packer, codec, entry points), xv_gemm8_wide.hip (256 x 256 tile on the 32 x 32
// MFMAs) and xv_gemm8_wide16.hip (the same tile on the 16 x 16 MFMAs).  Tile geometry, the launch parameters, the epilogue of
// the two 256 x 256 kernels and their launchers.  Like xv_device.h, everything lives in the including unit's anonymous
// namespace, so a kernel's symbol name does not depend on the file that defines it.
#pragma once
#include "xv_device.h"
#include "xv_split6.h"

namespace {

constexpr int BN = 128;                 // output channels per workgroup tile
constexpr int BK = 32;                  // input channels per stage
constexpr int SROW = 128;               // bytes per (row, 32-channel slab)
constexpr int B_PLANE = BN * 64;        // 8192: fp16 plane / 8-bit plane of a weight tile
constexpr int B_BYTES = 2 * B_PLANE;    // 16384

template <int T, int KT, class F>
__device__ __forceinline__ void for_taps(F &f)
{
    if constexpr (T < KT) {
        f(std::integral_constant<int, T>{});
        for_taps<T + 1, KT>(f);
    }
}

struct Gemm8Params {
    const uint8_t *x;     // split8 / split6 buffer, row 0
    int x_format;         // XV_FMT_SPLIT8, or XV_FMT_SPLIT6 (the wide16 kernels' MX6 form only)
    long R;
    int cin, xchunks;
    const uint8_t *wt;    // tiled f16bf8 weights
    const float *bias, *scale, *shift;
    const float *tapbias; // [K][cout] or NULL: see gemm8_tap_flags
    int act;
    const float *alpha;
    int K, dil, cout;
    const uint8_t *valid;
    void *y;              // fp32 rows, bf16 split buffer, split8 or split6 buffer (the last: the wide16 kernels only)
    int y_format, ldy, ychunks;
    float *blk;           // POOL: per-8-row-block (mean, M2) planes
    int *status;          // bit 0 is set when a split8 output had to be clamped (may be NULL)
    int n_mt, n_nt, n_chunks;
};

// The per-row bias (tapbias != NULL).  The producer of x stored u = scale * act(z + b) WITHOUT its BN shift, so that the ReLU's
// zeros reach the MFMAs as zero bits; the shift's share of this layer, c_t[o] = sum_c shift[c] * w[t][c][o], is a constant per
// tap wherever tap t falls on a frame: the caller passes bias + sum_t c_t as ``bias`` and the table c_t as ``tapbias``.  A tap
// that falls on a gap row or outside [0, R) (SAME padding: x is 0 there, shift and all) must not contribute: the epilogue takes
// its c_t out again.  Row flags, one byte per tile row in LDS: bit 0 = the row is valid, bit 1 + t = tap t of a valid row is
// missing.  (K <= 7 taps and the flag: eight bits.)  Without a table the byte is row_valid's, as before.
// The kernels fill the flags of a table launch behind the issue of their prologue DMA: K independent byte loads (clamped addresses, no
// branch between them) that share the DMA's latency, instead of K dependent ones in front of it.
template <int KT>
__device__ __forceinline__ uint8_t gemm8_tap_flags(const Gemm8Params &p, long gr, int left)
{
    bool inside[KT];
    long q[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        q[t] = gr - left + (long)t * p.dil;
        inside[t] = q[t] >= 0 && q[t] < p.R;
    }
    unsigned f = 0;
    if (p.valid) {
        uint8_t v[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) v[t] = p.valid[inside[t] ? q[t] : 0];       // (R > 0: row 0 exists)
#pragma unroll
        for (int t = 0; t < KT; ++t) f |= (inside[t] && v[t]) ? 0u : 2u << t;
    } else {
#pragma unroll
        for (int t = 0; t < KT; ++t) f |= inside[t] ? 0u : 2u << t;
    }
    return (f & (2u << (KT / 2))) ? (uint8_t)0 : (uint8_t)(f | 1u);              // the centre tap is the row itself
}

// tv[j] = 8 channels (from gc0) of the accumulators of tile row lr(j): minus the constants of the row's missing taps.  A
// divergent loop over the set bits -- about one row in fifty at 300-frame chunks has any.
template <class RowOf>
__device__ __forceinline__ void gemm8_drop_missing_taps(const Gemm8Params &p, const uint8_t *Ms, int gc0, f32x4 (&tv)[8][2], RowOf &&lr)
{
    if (gc0 + 8 > p.cout) return;                       // (columns past Cout of a 128-column tile: nothing is stored for them)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        unsigned m = Ms[lr(j)] >> 1;
        while (m) {
            const int t = __builtin_ctz(m);
            m &= m - 1;
            const float *c = p.tapbias + (size_t)t * p.cout + gc0;
            tv[j][0] -= *reinterpret_cast<const f32x4 *>(c);
            tv[j][1] -= *reinterpret_cast<const f32x4 *>(c + 4);
        }
    }
}

// the 256 x 256 workgroup tile of xv_gemm8_wide.hip / xv_gemm8_wide16.hip: LDS = [operand buffers | epilogue fp32 tile of 128
// rows (aliased)] [row mask] [epilogue params]
constexpr int W_BM = 256, W_BN = 256, W_TLD = W_BN + 4;
constexpr int W_A_BYTES = (W_BM + MAX_SPAN) * SROW;        // 33792
constexpr int W_B_BYTES = 2 * B_BYTES;                     // 32768: two 128-column weight tiles
constexpr int W_OPER = 2 * W_A_BYTES + 2 * W_B_BYTES;      // 133120
constexpr int W_TILE = 128 * W_TLD * 4;                    // 133120
constexpr int W_MASK_OFF = W_OPER > W_TILE ? W_OPER : W_TILE;
constexpr size_t W_LDS_BYTES = (size_t)W_MASK_OFF + W_BM + 4 * W_BN * sizeof(float);

// XV_FMT_SPLIT6 output of the 256 x 256 kernels (instantiated by the 16 x 16 MFMA form: wide_epilogue<POOL, true>).  An e2m3
// block is the 16 channels x {lo', c} of one row and needs them in ONE lane (v_cvt_scalef32_2xpk16_fp6_f32), so a thread takes 4 rows x 16 channels of the 128-row half -- rows (tid >> 4) + 32 j, block
// tid & 15 of the tile's 16 -- instead of wide_epilogue's 8 rows x 8 channels: the same 64 tile values, read as four 16-byte
// pieces per row.  The column parameters are read from LDS where they are used (64 registers otherwise).  Bias, missing-tap
// constants, mask, activation, BN scale / shift, amax / status as in wide_epilogue; a masked row is written as zeros (elements 0).
template <class WriteTile>
__device__ __forceinline__ void wide_epilogue_split6(const Gemm8Params &p, char *lds, const uint8_t *Ms, const float *Ps, long m0, int n0,
                                                     int tid, int wr, WriteTile &&write_tile)
{
    float *T = reinterpret_cast<float *>(lds);
    const int cg = tid & 15, r0 = tid >> 4;
    const int gc0 = n0 + cg * 16;
    const f32x4 *P4 = reinterpret_cast<const f32x4 *>(Ps) + cg * 4;
    float amax = 0.f;
    f32x4 tv[4][4];
    float keep[4];
    auto read_tile = [&](int h) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int lr = r0 + 32 * j;
#pragma unroll
            for (int q = 0; q < 4; ++q) tv[j][q] = *reinterpret_cast<const f32x4 *>(T + lr * W_TLD + cg * 16 + 4 * q);
            keep[j] = Ms[h * 128 + lr] ? 1.f : 0.f;
        }
    };
    auto process = [&](int h) {
        const long mh = m0 + h * 128;
        if (p.tapbias) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned m = Ms[h * 128 + r0 + 32 * j] >> 1;
                while (m) {
                    const int t = __builtin_ctz(m);
                    m &= m - 1;
                    const f32x4 *c = reinterpret_cast<const f32x4 *>(p.tapbias + (size_t)t * p.cout + gc0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) tv[j][q] -= c[q];
                }
            }
        }
        const int c = cg & 1;                            // block of the 32-channel slab gc0 >> 5
        char *ybase = reinterpret_cast<char *>(p.y) + (size_t)(gc0 >> 5) * SROW;
        const size_t yrow = (size_t)p.ychunks * SROW;
        auto rows = [&](auto MODE) {
            constexpr int mode = decltype(MODE)::value;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long gr = mh + r0 + 32 * j;
                float v[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 b = P4[q], sc = P4[W_BN / 4 + q], sh = P4[2 * W_BN / 4 + q], al = P4[3 * W_BN / 4 + q];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float z = tv[j][q][i] + b[i];
                        const float a = mode == 1 ? fmaxf(al[i] * z, z) : mode == 2 ? fmaxf(z, 0.f) : fmaxf(z, 0.f) + al[i] * fminf(z, 0.f);
                        v[4 * q + i] = keep[j] != 0.f ? a * sc[i] + sh[i] : 0.f;
                    }
                }
                xv_f16x8 h0, h1;
                xv_u32x6 x6;
                int e8m0;
                xv_split6_encode16<true>(v, h0, h1, x6, e8m0, amax);
                const int sw = (int)(gr >> 1) & 7;
                char *row = ybase + (size_t)gr * yrow;
                *reinterpret_cast<xv_f16x8 *>(row + (((2 * c) ^ sw) << 4)) = h0;
                *reinterpret_cast<xv_f16x8 *>(row + (((2 * c + 1) ^ sw) << 4)) = h1;
                *reinterpret_cast<xv_i32x4 *>(row + (((4 + c) ^ sw) << 4)) = (xv_i32x4){(int)x6[0], (int)x6[1], (int)x6[2], (int)x6[3]};
                // (the 2^-11 of the cross terms rides in the activation side's byte; XV_SPLIT6_E8M0_MIN keeps it positive)
                *reinterpret_cast<xv_i32x4 *>(row + (((6 + c) ^ sw) << 4)) = (xv_i32x4){(int)x6[4], (int)x6[5], e8m0 - XV_SPLIT6_LO_EXP, 0};
            }
        };
        if (p.act == XV_ACT_LRELU) rows(std::integral_constant<int, 1>{});
        else if (p.act == XV_ACT_RELU) rows(std::integral_constant<int, 2>{});
        else rows(std::integral_constant<int, 0>{});
    };
    __syncthreads();                                    // (the sequence of wide_epilogue)
    if (wr == 0) write_tile(T);
    __syncthreads();
    read_tile(0);
    __syncthreads();
    if (wr == 1) write_tile(T);
    __builtin_amdgcn_sched_barrier(0);
    process(0);
    __syncthreads();
    read_tile(1);
    __builtin_amdgcn_sched_barrier(0);
    process(1);
    if (amax > XV_SPLIT8_MAX && p.status) atomicOr(p.status, 1);
}

// Epilogue of the 256 x 256 kernels (both MFMA shapes), 128 rows at a time through an fp32 tile that re-uses the operand area:
// write_tile(T) puts the calling wave's 128 x 64 accumulators into the tile of its half.
template <bool POOL, bool Y6 = false, class WriteTile>
__device__ __forceinline__ void wide_epilogue(const Gemm8Params &p, char *lds, const uint8_t *Ms, const float *Ps, long m0, int n0,
                                              int tid, int wr, WriteTile &&write_tile)
{
    // (a compile-time choice: as a run-time branch beside the other formats it cost every !POOL kernel 70 spilled registers in
    // the epilogue, the SPLIT8 launches included)
    if constexpr (Y6) return wide_epilogue_split6(p, lds, Ms, Ps, m0, n0, tid, wr, write_tile);
    float *T = reinterpret_cast<float *>(lds);
    const int cg = tid & 31;                            // 8-channel group of the 256-column tile
    const int gc0 = n0 + cg * 8;
    float bias[8], sc[8], sh[8], al[8];
    {
        const f32x4 *P4 = reinterpret_cast<const f32x4 *>(Ps) + cg * 2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bias[i] = P4[0][i]; bias[4 + i] = P4[1][i];
            sc[i] = P4[W_BN / 4][i]; sc[4 + i] = P4[W_BN / 4 + 1][i];
            sh[i] = P4[2 * W_BN / 4][i]; sh[4 + i] = P4[2 * W_BN / 4 + 1][i];
            al[i] = P4[3 * W_BN / 4][i]; al[4 + i] = P4[3 * W_BN / 4 + 1][i];
        }
    }
    const bool lrelu = p.act == XV_ACT_LRELU;
    auto act3 = [&](auto MODE, float z, float a) {
        constexpr int mode = decltype(MODE)::value;
        return mode == 1 ? fmaxf(a * z, z) : mode == 2 ? fmaxf(z, 0.f) : fmaxf(z, 0.f) + a * fminf(z, 0.f);
    };
    auto by_mode = [&](auto &&f) {
        if (lrelu) f(std::integral_constant<int, 1>{});
        else if (p.act == XV_ACT_RELU) f(std::integral_constant<int, 2>{});
        else f(std::integral_constant<int, 0>{});
    };
    float amax = 0.f;
    f32x4 tv[8][2];
    float keep[8];
    // thread -> 8 rows x 8 channels of a half: POOL: the 8 rows of block tid >> 5; else rows (tid >> 5) + 16 j
    auto read_tile = [&](int h) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int lr = POOL ? (tid >> 5) * 8 + j : (tid >> 5) + 16 * j;
            tv[j][0] = *reinterpret_cast<const f32x4 *>(T + lr * W_TLD + cg * 8);
            tv[j][1] = *reinterpret_cast<const f32x4 *>(T + lr * W_TLD + cg * 8 + 4);
            keep[j] = Ms[h * 128 + lr] ? 1.f : 0.f;
        }
    };
    auto process = [&](int h) {
        const long mh = m0 + h * 128;
        if (p.tapbias)                                  // (in a branch of its own: the straight path keeps its registers)
            gemm8_drop_missing_taps(p, Ms + h * 128, gc0, tv, [&](int j) { return POOL ? (tid >> 5) * 8 + j : (tid >> 5) + 16 * j; });
        if constexpr (POOL) {
            const int blk = tid >> 5;                   // 16 blocks of 8 rows
            if (mh + blk * 8 >= p.R) return;
            float v0[8], s1[8], s2[8];
            float n = 0.f;
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
            f32x4 mean[2], m2[2];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                mean[i >> 2][i & 3] = n > 0.f ? v0[i] + s1[i] * rn : 0.f;
                m2[i >> 2][i & 3] = fmaxf(s2[i] - s1[i] * s1[i] * rn, 0.f);
            }
            float *o = p.blk + ((size_t)((mh >> 3) + blk) * 2) * p.cout + gc0;
            *reinterpret_cast<f32x4 *>(o) = mean[0];
            *reinterpret_cast<f32x4 *>(o + 4) = mean[1];
            *reinterpret_cast<f32x4 *>(o + p.cout) = m2[0];
            *reinterpret_cast<f32x4 *>(o + p.cout + 4) = m2[1];
        } else {
            const int ch = gc0 >> 5, slot = cg & 3;
            char *ybase = reinterpret_cast<char *>(p.y) + (size_t)ch * SROW;
            const size_t yrow = (size_t)p.ychunks * SROW;
            auto rows = [&](auto MODE, auto Y8) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const long gr = mh + (tid >> 5) + 16 * j;
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
                        *reinterpret_cast<xv_f16x8 *>(row + ((slot ^ sw) << 4)) = hi;              // (plain, not non-temporal: see DESIGN 3.1e)
                        *reinterpret_cast<xv_i32x4 *>(row + (((4 + slot) ^ sw) << 4)) = x8;
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
            if (p.y_format == XV_FMT_SPLIT8) by_mode([&](auto MODE) { rows(MODE, std::true_type{}); });
            else by_mode([&](auto MODE) { rows(MODE, std::false_type{}); });
        }
    };
    // upper half through the tile; the lower half's accumulators go into the tile as soon as the upper half has been read
    // into registers, i.e. BEFORE the arithmetic of the upper half (128 accumulators + 64 tile values + the arithmetic of
    // an epilogue do not fit the register file)
    __syncthreads();                                    // operand buffers are dead
    if (wr == 0) write_tile(T);
    __syncthreads();
    read_tile(0);
    __syncthreads();
    if (wr == 1) write_tile(T);
    __builtin_amdgcn_sched_barrier(0);
    process(0);
    __syncthreads();
    read_tile(1);
    __builtin_amdgcn_sched_barrier(0);
    process(1);
    if constexpr (!POOL)
        if (amax > XV_SPLIT8_MAX && p.status) atomicOr(p.status, 1);
}

}  // namespace

// The 256 x 256 kernels behind launch_gemm8 (xv_gemm8.hip), which has checked the arguments, chosen the tile and set n_mt / n_nt:
// pick the {K, POOL} kernel, opt in to its dynamic LDS, launch.  C linkage because Gemm8Params is each unit's own (identical)
// anonymous-namespace type; hidden: not part of the library's ABI.
extern "C" {
__attribute__((visibility("hidden"))) int launch_gemm8_wide(const Gemm8Params &p, hipStream_t st);        // xv_gemm8_wide.hip
__attribute__((visibility("hidden"))) int launch_gemm8_wide16(const Gemm8Params &p, hipStream_t st);      // xv_gemm8_wide16.hip
}
