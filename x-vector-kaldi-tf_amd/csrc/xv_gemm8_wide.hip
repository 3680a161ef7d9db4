// xv_gemm8_wide.hip -- the f16bf8 layer of xv_gemm8.hip on a 256 x 256 workgroup tile (32 x 32 MFMA shapes; launch_gemm8_wide): 8 waves as 2 x 4, each a 128 x 64 sub-tile (4 x 2 MFMA tiles, 128
// accumulator registers).  With 64 x 64 sub-tiles this arithmetic needs 147 LDS bytes per MFMA cycle -- more than the 128
// the LDS delivers (halving the fragment reads made the kernel 14 % faster); 4 x 2 sub-tiles need 24 fragment reads per
// 1024 MFMA cycles instead of 16 per 512, and a 32 KB weight stage feeds twice the MFMAs: 113 bytes per cycle.
// The fragment sets are pipelined in four steps per stage so that at most four 16-register sets are live next to the
// accumulators (t / b = row tiles 0,1 / 2,3 of the wave; H = fp16 fragments of both k-steps, X = 8-bit fragments):
//     step 1   8 fp16 MFMAs (top,    BH)   | read AHb(s), BX(s)
//     step 2   8 fp16 MFMAs (bottom, BH)   | read AXt(s)
//     barrier  [every B fragment of stage s is in registers; stage s+1 has landed]
//     step 3   4 scaled MFMAs (top,    BX) | DMA of stage s+2 | read AXb(s), BH(s+1)
//     step 4   4 scaled MFMAs (bottom, BX) | read AHt(s+1)
// A fragments may be read after the barrier because a halo buffer is only rewritten one slab later (K > 1 only; the K = 1
// layers keep the narrow kernel).  Cout % 256 == 0, split-format or POOL output (the launcher falls back otherwise).
// The epilogue goes through the LDS in two halves of 128 rows (the fp32 tile of a half is exactly the operand area).
#include "xv_gemm8.h"

namespace {

template <int KT, bool POOL>
__global__ __launch_bounds__(512, 2) void tdnn_gemm_f16bf8_wide_kernel(const Gemm8Params p)
{
    static_assert(KT > 1, "the wide kernel reads A fragments after the stage barrier: K > 1 only");
    constexpr int NW = 8;
    constexpr int BP = 4;                              // 1 KB pieces of a 32 KB weight stage per wave
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char *Abuf = lds;
    char *Bbuf = lds + 2 * W_A_BYTES;
    uint8_t *Ms = reinterpret_cast<uint8_t *>(lds + W_MASK_OFF);
    float *Ps = reinterpret_cast<float *>(lds + W_MASK_OFF + W_BM);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;

    const int nwg = p.n_mt * p.n_nt;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, idx = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    const int mt = wg / p.n_nt, nt = wg - mt * p.n_nt;
    const long m0 = (long)mt * W_BM;
    const int n0 = nt * W_BN;

    const int span = (KT - 1) * p.dil;
    const int left = span >> 1;
    const int n_stages = p.n_chunks * KT;
    const int goff = (int)((m0 - left) & 15);

    if (tid < W_BM) {
        const long gr = m0 + tid;
        Ms[tid] = (gr < p.R) ? (p.valid ? p.valid[gr] : (uint8_t)1) : (uint8_t)0;
    } else {
        const int c = tid - W_BM, gc = n0 + c;           // Cout % 256 == 0: every column exists
        Ps[c] = p.bias ? p.bias[gc] : 0.f;
        Ps[W_BN + c] = p.scale ? p.scale[gc] : 1.f;
        Ps[2 * W_BN + c] = p.shift ? p.shift[gc] : 0.f;
        Ps[3 * W_BN + c] = p.act == XV_ACT_NONE ? 1.f : p.act == XV_ACT_LRELU ? p.alpha[0] : p.act == XV_ACT_PRELU ? p.alpha[gc] : 0.f;
    }

    const size_t xrow_bytes = (size_t)p.xchunks * SROW;
    const int arow0 = wr * 128 + (lane & 31);
    const int bcol = wc * 64 + (lane & 31);            // column of the 256-column stage; + 32 stays inside its 128-column tile
    const int kh = lane >> 5;
    const int boff0 = (bcol >> 7) * B_BYTES + (bcol & 127) * 64;
    const int bsw0 = ((bcol & 127) >> 2) & 3;

    // weight stage = the tiles of column tiles 2 nt and 2 nt + 1; wave w moves pieces 4w .. 4w+3 of its 32 KB
    const uint8_t *bbase = p.wt + ((size_t)(2 * nt + (wave >> 2)) * n_stages) * B_BYTES + (wave & 3) * 4096 + lane * 16;
    const int bdst = (wave >> 2) * B_BYTES + (wave & 3) * 4096;
    const uint8_t *abase = p.x + (m0 - left + (lane >> 3)) * (long)xrow_bytes + (lane & 7) * 16;
    constexpr int NP = W_BM / 8 + 1;
    {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint8_t *src = bbase + (size_t)(j < n_stages ? j : n_stages - 1) * B_BYTES;
            char *dst = Bbuf + j * W_B_BYTES + bdst;
#pragma unroll
            for (int i = 0; i < BP; ++i) XV_GLDS16(src + i * 1024, dst + i * 1024);
        }
        for (int piece = wave; piece < NP; piece += NW) XV_GLDS16(abase + (size_t)piece * 8 * xrow_bytes, Abuf + piece * 1024);
    }
    if (p.tapbias && tid < W_BM) Ms[tid] = gemm8_tap_flags<KT>(p, m0 + tid, left);         // (xv_gemm8.h)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x16){0};
    struct SetH { xv_f16x8 f0[2], f1[2]; };            // two MFMA tiles x two k-steps
    struct SetX { xv_i32x8 f0, f1; };
    int scale_a = XV_SPLIT8_E8M0, scale_b = 127;
    asm volatile("" : "+v"(scale_a), "+v"(scale_b));

    int pa[KT], px[KT];                                // row tile 0 of the wave; tile i is + i * 32 rows (same swizzle)
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const int lr0 = arow0 + t * p.dil;
        const int sw = ((lr0 + goff) & 15) >> 1;
        pa[t] = lr0 * SROW + ((sw ^ kh) << 4);
        px[t] = lr0 * SROW + ((sw ^ (4 + 2 * kh)) << 4);
    }
    const int pb0 = 2 * W_A_BYTES + boff0 + ((kh ^ bsw0) << 4);
    const int pb1 = 2 * W_A_BYTES + boff0 + (((2 + kh) ^ bsw0) << 4);
    const int pbx = 2 * W_A_BYTES + B_PLANE + boff0 + (((2 * kh) ^ bsw0) << 4);

    auto load_ah = [&](SetH &X, int base) {             // base = pa[t] + A buffer offset + (0 | 64 rows)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const char *a = lds + (base ^ (ks << 5));
            X.f0[ks] = *reinterpret_cast<const xv_f16x8 *>(a);
            X.f1[ks] = *reinterpret_cast<const xv_f16x8 *>(a + 32 * SROW);
        }
    };
    auto load_bh = [&](SetH &X, int bbase_) {
        X.f0[0] = *reinterpret_cast<const xv_f16x8 *>(lds + pb0 + bbase_);
        X.f1[0] = *reinterpret_cast<const xv_f16x8 *>(lds + pb0 + bbase_ + 32 * 64);
        X.f0[1] = *reinterpret_cast<const xv_f16x8 *>(lds + pb1 + bbase_);
        X.f1[1] = *reinterpret_cast<const xv_f16x8 *>(lds + pb1 + bbase_ + 32 * 64);
    };
    auto cat = [](xv_i32x4 u, xv_i32x4 v) { return __builtin_shufflevector(u, v, 0, 1, 2, 3, 4, 5, 6, 7); };
    auto load_ax = [&](SetX &X, int base) {             // base = px[t] + A buffer offset + (0 | 64 rows)
        const char *a = lds + base, *a2 = lds + (base ^ 16);
        X.f0 = cat(*reinterpret_cast<const xv_i32x4 *>(a), *reinterpret_cast<const xv_i32x4 *>(a2));
        X.f1 = cat(*reinterpret_cast<const xv_i32x4 *>(a + 32 * SROW), *reinterpret_cast<const xv_i32x4 *>(a2 + 32 * SROW));
    };
    auto load_bx = [&](SetX &X, int bbase_) {
        const char *b = lds + pbx + bbase_, *b2 = lds + ((pbx + bbase_) ^ 16);
        X.f0 = cat(*reinterpret_cast<const xv_i32x4 *>(b), *reinterpret_cast<const xv_i32x4 *>(b2));
        X.f1 = cat(*reinterpret_cast<const xv_i32x4 *>(b + 32 * 64), *reinterpret_cast<const xv_i32x4 *>(b2 + 32 * 64));
    };
    auto mma_h = [&](const SetH &A, const SetH &B, int i0) {      // row tiles i0, i0+1
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            acc[i0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A.f0[ks], B.f0[ks], acc[i0][0], 0, 0, 0);
            acc[i0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A.f0[ks], B.f1[ks], acc[i0][1], 0, 0, 0);
            acc[i0 + 1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A.f1[ks], B.f0[ks], acc[i0 + 1][0], 0, 0, 0);
            acc[i0 + 1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A.f1[ks], B.f1[ks], acc[i0 + 1][1], 0, 0, 0);
        }
    };
    auto mma_x = [&](const SetX &A, const SetX &B, int i0) {
        acc[i0][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A.f0, B.f0, acc[i0][0], 1, 1, 0, scale_a, 0, scale_b);
        acc[i0][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A.f0, B.f1, acc[i0][1], 1, 1, 0, scale_a, 0, scale_b);
        acc[i0 + 1][0] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A.f1, B.f0, acc[i0 + 1][0], 1, 1, 0, scale_a, 0, scale_b);
        acc[i0 + 1][1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(A.f1, B.f1, acc[i0 + 1][1], 1, 1, 0, scale_a, 0, scale_b);
    };

    // In the main loop only waves 0-3 -- one per SIMD (a workgroup's waves go to the SIMDs cyclically: w and w + 4 share one) --
    // issue DMA.  An LDS-DMA instruction holds a wave's issue for 60-180 cycles; when all eight waves issue their pieces behind
    // the same barrier, both waves of every SIMD stand still together and the MFMA pipe with them.  With one issuing wave per
    // SIMD the other one keeps the pipe busy, and the issuing wave catches up while its partner waits at the next barrier.
    constexpr int NI = 4;                              // issuing waves
    constexpr int DT = KT - 1;
    constexpr int NS = (NP + NI - 1) / NI;
    constexpr int PW = (NS + DT - 1) / DT;
    auto slots_of = [](int t) constexpr { return t < DT ? (NS + DT - 1 - t) / DT : 0; };
    auto slot_base = [](int t) constexpr { int b = 0; for (int u = 0; u < t; ++u) b += (NS + DT - 1 - u) / DT; return b; };
    const uint32_t rowstep = 8u * (uint32_t)xrow_bytes;
    uint32_t ag_off[DT][PW], al_off[DT][PW];
#pragma unroll
    for (int t = 0; t < DT; ++t)
#pragma unroll
        for (int j = 0; j < PW; ++j) {
            int piece = (slot_base(t) + j) * NI + wave;
            piece = piece < NP ? piece : NP - 1;
            ag_off[t][j] = (uint32_t)piece * rowstep;
            al_off[t][j] = (uint32_t)piece * 1024u;
        }
    // (main loop: wave w < 4 moves pieces 4w .. 4w+3 of BOTH 16 KB weight tiles of a stage)
    const uint8_t *bnext = p.wt + ((size_t)(2 * nt) * n_stages) * B_BYTES + (wave & 3) * 4096 + lane * 16 +
                           (size_t)(2 < n_stages ? 2 : n_stages - 1) * B_BYTES;
    const size_t btile = (size_t)n_stages * B_BYTES;   // from column tile 2 nt to 2 nt + 1

    constexpr int HALF = 64 * SROW;                    // row tiles 2,3 of the wave
    SetH AHt, AHb, BH;
    SetX AXt, AXb, BX;
    load_ah(AHt, pa[0]);
    load_bh(BH, 0);

    int s = 0;
    for (int c = 0; c < p.n_chunks; ++c) {
        const int abuf = (c & 1) * W_A_BYTES;
        const int abuf_n = W_A_BYTES - abuf;
        const int cn = (c + 1 < p.n_chunks) ? c + 1 : p.n_chunks - 1;
        const uint8_t *anext = abase + (size_t)cn * SROW;
        char *adst_n = Abuf + (cn & 1) * W_A_BYTES;
        auto tap = [&](auto TT) {
            constexpr int t = decltype(TT)::value;
            const int bbuf = (s & 1) * W_B_BYTES;
            // ---- step 1 ----
            load_ah(AHb, pa[t] + abuf + HALF);
            load_bx(BX, bbuf);
            mma_h(AHt, BH, 0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            // ---- step 2 ----
            load_ax(AXt, px[t] + abuf);
            mma_h(AHb, BH, 2);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();                  // every B fragment of stage s is in registers; stage s+1 has landed
            // ---- step 3 ----
            if (wave < NI) {
                char *dst = Bbuf + bbuf + (wave & 3) * 4096;
                XV_GLDS16_OFF(bnext, dst, 0);
                XV_GLDS16_OFF(bnext, dst, 1024);
                XV_GLDS16_OFF(bnext, dst, 2048);
                XV_GLDS16_OFF(bnext, dst, 3072);
                XV_GLDS16_OFF(bnext + btile, dst + B_BYTES, 0);
                XV_GLDS16_OFF(bnext + btile, dst + B_BYTES, 1024);
                XV_GLDS16_OFF(bnext + btile, dst + B_BYTES, 2048);
                XV_GLDS16_OFF(bnext + btile, dst + B_BYTES, 3072);
                if constexpr (t < DT) {
#pragma unroll
                    for (int j = 0; j < slots_of(t); ++j) XV_GLDS16(anext + ag_off[t][j], adst_n + al_off[t][j]);
                }
            }
            bnext += (s + 3 < n_stages) ? B_BYTES : 0;
            load_ax(AXb, px[t] + abuf + HALF);
            load_bh(BH, W_B_BYTES - bbuf);
            mma_x(AXt, BX, 0);
            constexpr int NV = 0;                       // (the DMA block above is a region of its own now)
#define XV_G8W_GROUP(i)                                                             \
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                      \
            if constexpr ((NV + 3 - (i)) / 4 > 0) __builtin_amdgcn_sched_group_barrier(0x020, (NV + 3 - (i)) / 4, 0); \
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            XV_G8W_GROUP(0) XV_G8W_GROUP(1) XV_G8W_GROUP(2) XV_G8W_GROUP(3)
#undef XV_G8W_GROUP
            __builtin_amdgcn_sched_barrier(0);
            // ---- step 4 ----
            if constexpr (t + 1 < KT) load_ah(AHt, pa[t + 1] + abuf);
            else load_ah(AHt, pa[0] + abuf_n);               // first tap of the next slab (tail: harmless read)
            mma_x(AXb, BX, 2);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            ++s;
        };
        for_taps<0, KT>(tap);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- epilogue, 128 rows at a time ---------------------------------------------------------------------------------
    auto write_tile = [&](float *T) {                   // this wave's 128 x 64 accumulators -> the fp32 tile of its half
        const int col = wc * 64 + (lane & 31);
        const int rowb = 4 * (lane >> 5);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int rr = i * 32 + rowb + (reg & 3) + 8 * (reg >> 2);
                T[rr * W_TLD + col] = acc[i][0][reg];
                T[rr * W_TLD + col + 32] = acc[i][1][reg];
            }
    };
    wide_epilogue<POOL>(p, lds, Ms, Ps, m0, n0, tid, wr, write_tile);
}

typedef void (*gemm8_fn)(const Gemm8Params);
struct WideKernel {
    int kt;
    bool pool;
    gemm8_fn fn;
};
const WideKernel WIDE_KERNELS[] = {
    {3, false, tdnn_gemm_f16bf8_wide_kernel<3, false>}, {5, false, tdnn_gemm_f16bf8_wide_kernel<5, false>}, {7, false, tdnn_gemm_f16bf8_wide_kernel<7, false>},
    {3, true, tdnn_gemm_f16bf8_wide_kernel<3, true>},   {5, true, tdnn_gemm_f16bf8_wide_kernel<5, true>},   {7, true, tdnn_gemm_f16bf8_wide_kernel<7, true>},
};

}  // namespace

int launch_gemm8_wide(const Gemm8Params &p, hipStream_t st)
{
    const WideKernel *k = nullptr;
    for (const WideKernel &e : WIDE_KERNELS)
        if (e.kt == p.K && e.pool == (p.blk != nullptr)) k = &e;
    if (!k) return fail(XV_ERR_UNSUPPORTED, "tdnn_f16bf8: no kernel for this configuration");
    static std::atomic<unsigned long long> lds_done{0};
    if (const int rc = opt_in_dynamic_lds(lds_done, WIDE_KERNELS, [](const WideKernel &e) { return std::make_pair(e.fn, W_LDS_BYTES); })) return rc;
    hipLaunchKernelGGL(k->fn, dim3((unsigned)(p.n_mt * p.n_nt)), dim3(512), W_LDS_BYTES, st, p);
    return launch_status("tdnn_gemm_f16bf8_kernel launch");
}
