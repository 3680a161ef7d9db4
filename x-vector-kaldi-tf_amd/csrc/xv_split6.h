// xv_split6.h -- the cross terms of the f16bf8 arithmetic (xv_split8.h) in block-scaled e2m3 (device code, gfx950).
//
// A value v is still carried as hi = fp16(v) plus the two cross-term operands lo' = 2^11 (v - hi) and c = clamp(v), but the
// cross-term operands of 16 channels share ONE power-of-two block scale and are stored in 6 bits each:
//     block   = the 32 values [lo'[0..15] | c[0..15]] (activations) / [c[0..15] | lo'[0..15]] (weights) of one frame / column
//     m       = the largest magnitude among them
//     s       = the largest power of two with s m <= 7.5 (the largest finite e2m3); s = 1 when m = 0
//     element = e2m3(s value), round to nearest even (1 sign, 2 exponent, 3 mantissa bits: 0, 0.125 .. 0.875, 1 .. 1.875 in
//               steps of 0.125, 2 .. 3.75 in steps of 0.25, 4 .. 7.5 in steps of 0.5) -- nothing saturates, by the choice of s
//     E8M0    = the biased exponent of 1 / s: one byte per block, the scale operand of the MFMA
// v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz:2 blgp:2 takes, in lane (row l & 31, K block l >> 5), the 32 elements of that block
// in six dwords and the block's scale byte in byte op_sel of that lane's scale register (tools/experiments/mx_probe.hip, part
// 3), and runs in half the cycles of the bf8 form.  Element i of an activation block meets element i of a weight block, so lo'
// pairs with c and c with lo'; the 2^-11 of the cross terms is subtracted from the activation side's byte, as XV_SPLIT8_E8M0
// carries it in the bf8 form.  e2m3 has one mantissa bit more than e5m2; its narrow exponent range does no harm because inside
// a block only the large elements matter to the absolute error of a dot product (tools/experiments/cross_term_mx6_sim.py).
//
// The same holds for v_mfma_scale_f32_16x16x128_f8f6f4 (row / column l & 15, K block l >> 4, every lane's own byte: mx_probe part 4),
// which tdnn_gemm_f16bf8_wide16_kernel's MX6 form runs on rows stored in HBM: XV_FMT_SPLIT6 (include/xvector_hip.h), a block = 16
// CONSECUTIVE channels of a 32-channel slab, written by the producing layer's epilogue (wide_epilogue_split6 in xv_gemm8.h).
//
// Both sides are encoded by the same instruction, v_cvt_scalef32_2xpk16_fp6_f32 (32 floats / scale -> six dwords), so the
// order of the elements inside the six dwords agrees by construction.
#pragma once
#include "xv_split8.h"

// position, among the 32 six-bit elements of the result (element k = bits [6k, 6k + 6) of the six dwords), of value i of source
// s (0 / 1) of v_cvt_scalef32_2xpk16_fp6_f32 -- for code that READS a block's bits (xv_split6_decode_f32); the MFMA never needs it
#define XV_SPLIT6_ELEM(s, i) (2 * (i) + (s))

typedef unsigned xv_u32x6 __attribute__((ext_vector_type(6)));
typedef float xv_f32x16 __attribute__((ext_vector_type(16)));

constexpr int XV_SPLIT6_E8M0_MIN = 16;                // floor of a block's byte (a block of denormals: its elements round to 0)
constexpr int XV_SPLIT6_LO_EXP = 11;                  // the 2^-11 of the cross terms: subtracted from the byte an activation block STORES (XV_FMT_SPLIT6)

// The E8M0 byte of 1 / s for the block maximum m >= 0 (finite): m = f 2^e with 1 <= f < 2 gives 1 / s = 2^(e-2) for f <= 1.875
// and 2^(e-1) above -- the carry of (mantissa + 0x0fffff) into the exponent field is exactly "f > 1.875".
__device__ __forceinline__ int xv_split6_e8m0(float m)
{
    const int e = ((__builtin_bit_cast(int, m) + 0x0fffff) >> 23) - 2;
    return m == 0.f ? 127 : (e < XV_SPLIT6_E8M0_MIN ? XV_SPLIT6_E8M0_MIN : e);
}

// Inline asm on purpose: this compiler lets the destination of __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32 overlap its sources
// and its scale register, and the instruction writes its result while it still reads them (seen with mx_probe: everything behind
// the twelfth element converted with a clobbered scale).  The early-clobber constraint keeps the six result registers apart; the
// s_nop covers a matrix instruction that reads them next, which the hazard recogniser cannot see behind asm.
__device__ __forceinline__ xv_u32x6 xv_cvt_2xpk16_e2m3(xv_f32x16 a, xv_f32x16 b, float scale)
{
    xv_u32x6 r;
    asm("v_cvt_scalef32_2xpk16_fp6_f32 %0, %1, %2, %3\n\ts_nop 1" : "=&v"(r) : "v"(a), "v"(b), "v"(scale));
    return r;
}

// 16 channels -> two fp16 fragments + one e2m3 block and its byte.  LO_FIRST: activations ([lo' | c]); weights the opposite order.
// amax as in xv_split8_encode8.
template <bool LO_FIRST>
__device__ __forceinline__ void xv_split6_encode16(const float (&v)[16], xv_f16x8 &h0, xv_f16x8 &h1, xv_u32x6 &x, int &e8m0, float &amax)
{
    xv_f32x16 c, lo;
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        amax = fmaxf(amax, fabsf(v[i]));
        c[i] = __builtin_amdgcn_fmed3f(v[i], -XV_SPLIT8_MAX, XV_SPLIT8_MAX);
        const _Float16 h = (_Float16)c[i];
        if (i < 8) h0[i] = h;
        else h1[i - 8] = h;
        lo[i] = (c[i] - (float)h) * XV_SPLIT8_LO_SCALE;          // (exact: a power of two)
        m = fmaxf(m, fmaxf(fabsf(c[i]), fabsf(lo[i])));
    }
    e8m0 = xv_split6_e8m0(m);
    const float inv = __builtin_bit_cast(float, e8m0 << 23);      // 1 / s: the instruction converts value / scale
    x = LO_FIRST ? xv_cvt_2xpk16_e2m3(lo, c, inv) : xv_cvt_2xpk16_e2m3(c, lo, inv);
}
