// xv_gemm3.hip -- the frame-level layers and FCs in the bf16x3 arithmetic (gfx950): tdnn_gemm_bf16x3_kernel with its table
// and launch_gemm3, the weight packers (one layer, or many layers in both orientations for the training step), the bf16 split
// activation format's encode / decode helpers, and the C entry points that end in them.  The exact-fp32 family of the same
// layers is xv_kernels.hip, the f16bf8 one xv_gemm8.hip; the POOL epilogue's block statistics are merged by xv_pool.hip.
#include "xv_device.h"

namespace {

// ------------------------------------------------------------------------------------------------
// bf16x3 split-precision GEMM (v2: DMA-fed).
//
// Every fp32 operand is split x = hi + lo (hi = bf16(x), lo = bf16(x - hi)); products are accumulated in
// fp32 as lo*hi + hi*lo + hi*hi on v_mfma_f32_32x32x16_bf16 (the lo*lo term, ~2^-16 relative, is dropped).
//
// Operand formats (all produced on the GPU, see include/xvector_hip.h):
//  * weights: xv_pack_weights_bf16x3 writes one 16 KB tile per (column tile, channel slab, tap) in exactly the
//    LDS image order ([hi: 128 cols x 64 B][lo: 128 x 64 B], 16-B slots XOR-swizzled by (col>>2)&3), tiles
//    ordered as the K-loop walks them -> a stage's B operand is ONE linear 16 KB global->LDS DMA.
//  * activations between layers: "split" format -- per row and 32-channel slab 128 B = [4 hi slots | 4 lo slots]
//    of 8 bf16, slots XOR-swizzled by (row>>1)&7 -> the (128+(K-1)d)-row halo tile of a slab is a linear DMA of
//    128 B per row, re-used by all K taps; same bytes per element as fp32.
//  * the first layer / the segment FC read plain fp32 rows and split them while staging (FP32 A mode).
// Mainloop per stage and wave: 4 B-DMA + ~1 A-DMA instructions, 16 ds_read_b128, 24 MFMAs, one barrier.
// Epilogue: accumulators -> LDS (fp32 tile) -> bias/act/BN/gap-mask -> 16-byte NON-TEMPORAL stores (fp32 rows or
// split): the outputs are 0.27-0.8 GB streams, and plain stores (L2 write-allocate) measured 7-16 % slower.
// ------------------------------------------------------------------------------------------------
constexpr int BN = 128;                           // output channels per workgroup tile
constexpr int BK = 32;                            // input channels per stage
constexpr int SROW = 128;                         // bytes per (row, 32-channel slab): LDS A row and HBM split row-slab
constexpr int B3_PLANE = BN * 64;                 // 8192
constexpr int B3_BYTES = 2 * B3_PLANE;            // 16384: [hi tile][lo tile]
constexpr int T_LD = BN + 4;                      // epilogue fp32 tile row (floats)
// Workgroup geometry of the bf16x3 kernel: WM x 2 waves, each wave a 64 x 64 sub-tile (2 x 2 MFMA tiles) -> tile of
// WM*64 rows x 128 columns.  WM = 2: 4 waves, 128-row tile, 69.7 KB of LDS, two workgroups per CU.  WM = 4: 8 waves,
// 256-row tile, one workgroup per CU (same waves per SIMD): a weight tile feeds twice the MFMAs, i.e. half the
// global->LDS weight bytes per FLOP.  LDS: [operand buffers | epilogue fp32 tile (aliased)] [row mask] [epilogue params].
constexpr int gemm3_oper_bytes(int wm) { return 2 * (wm * 64 + MAX_SPAN) * SROW + 2 * B3_BYTES; }
constexpr int gemm3_tile_bytes(int wm) { return wm * 64 * T_LD * 4; }
constexpr int gemm3_mask_off(int wm) { return gemm3_oper_bytes(wm) > gemm3_tile_bytes(wm) ? gemm3_oper_bytes(wm) : gemm3_tile_bytes(wm); }
constexpr size_t gemm3_lds_bytes(int wm) { return (size_t)gemm3_mask_off(wm) + wm * 64 + 4 * BN * sizeof(float); }

// f(integral_constant<int, T>) for T = T0 .. KT-1, unrolled at compile time
template <int T, int KT, class F>
__device__ __forceinline__ void for_taps(F &f)
{
    if constexpr (T < KT) {
        f(std::integral_constant<int, T>{});
        for_taps<T + 1, KT>(f);
    }
}

struct Gemm3Params {
    const void *x;        // fp32 rows (x_split == 0) or split buffer (row 0 of it)
    int x_split;
    long R;
    int cin, ldx, xchunks;
    const uint8_t *wt;    // tiled bf16x3 weights
    const float *bias, *scale, *shift;
    int act;
    const float *alpha;
    int K, dil, cout;
    const uint8_t *valid;
    void *y;              // fp32 rows or split buffer (may be NULL when only ypre is wanted)
    int y_split, ldy, ychunks;
    float *ypre;          // fp32 rows, stride ldpre (optional)
    int ldpre;
    float *blk;           // POOL epilogue: per-8-row-block (mean, M2) planes [ceil(R/8)][2][cout]
    int n_mt, n_nt, n_chunks;
    // column sums of the fp32 output (training: the BN backward of the layer BELOW needs sum y and sum y * r over the rows, y = the
    // input gradient this launch produces): per row tile partials cs_part[mt][{sum y, sum y r}][cout] in double, merged in order by
    // xv_col_sums_merge_f32.  cs_r: the other factor, fp32 rows of stride cs_ldr; NULL = the output itself (sum y, sum y^2: the
    // batch moments BN(training) takes of a forward layer's activation output, accumulated in double).  cs_part NULL = off.
    const float *cs_r;
    int cs_ldr;
    double *cs_part;
};

// KT: kernel size K of the split-input path as a compile-time constant (1, 3, 5, 7; 0 = the fp32-input path, runtime K).
// The stage loop of that path is unrolled over the K taps of a slab, so everything that depends on the tap -- fragment
// row offsets, the A-halo DMA schedule -- is computed once, and an iteration carries ~15 integer instructions next to
// its 24 MFMAs instead of ~85 (each one beside an MFMA costs issue slots AND clock on this power-limited loop).
// A-halo DMA pieces (8 rows = 1 KB each): the (<=17)-piece halo tile of the NEXT slab is spread over taps 0..K-2 of
// the current slab, PW pieces per wave per tap (K=1: 4 -- every stage loads its own slab --, K=3: 3, K=5: 2, K=7: 1).
// POOL: the layer output is not stored; the epilogue reduces every 8-row block of the tile to per-channel (mean, M2)
// for the statistics pooling that follows the last frame-level layer (see stats_pool_blocks_kernel).
// S16 (split input, K > 1, an even number of slabs): the same tile and the same bytes through LDS on v_mfma_f32_16x16x32_bf16 -- a
// dot product twice as long per instruction, quarter-size accumulator tiles: fewer joules per product on the power-limited pipe
// (tools/experiments/shape_probe.hip).  A wave holds ALL 16 fragments of a stage (4 row tiles + 4 column tiles, hi and lo: 64
// VGPRs) and reads the next stage's 16 behind the 48 MFMAs of the current one: two fragment sets + 64 accumulators = 192 VGPRs.
template <bool SPLIT_A, int KT, bool POOL, int WM, bool S16 = false>
__global__ __launch_bounds__(WM * 128, (S16 && WM == 4) ? 1 : 2) void tdnn_gemm_bf16x3_kernel(const Gemm3Params p)
{
    static_assert(!S16 || (SPLIT_A && KT > 1), "the 16 x 16 form exists for split input and K > 1");
    constexpr int NW = 2 * WM;                         // waves per workgroup
    constexpr int NT = NW * 64;                        // threads
    constexpr int BM = WM * 64;                        // rows per workgroup tile
    constexpr int A_ROWS = BM + MAX_SPAN;
    constexpr int A3_BYTES = A_ROWS * SROW;
    constexpr int BP = 16 / NW;                        // 1 KB pieces of a 16 KB weight tile per wave
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char *Abuf = lds;                                  // [2][A_ROWS][128 B]
    char *Bbuf = lds + 2 * A3_BYTES;                   // [2][hi 8 KB | lo 8 KB]
    uint8_t *Ms = reinterpret_cast<uint8_t *>(lds + gemm3_mask_off(WM));
    float *Ps = reinterpret_cast<float *>(lds + gemm3_mask_off(WM) + BM);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;

    // XCD-aware tile order.  Hardware places block b on XCD b%8; every XCD gets a contiguous run of logical tile ids
    // L = mt*n_nt + nt (bijective chunking), column tiles fastest, so the n_nt tiles sharing an A panel run close
    // together on one L2.  (Measured alternatives that did NOT help: column-tile-major order to pin one weight panel
    // in L2 (-3 %), persistent workgroups (-4 %), de-synchronised start delays (0 %), s_setprio around the MFMAs (0 %).)
    const int nwg = p.n_mt * p.n_nt;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, idx = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    const int mt = wg / p.n_nt, nt = wg - mt * p.n_nt;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;

    const int span = (p.K - 1) * p.dil;
    const int left = span >> 1;
    const int rowsA = BM + span;
    const int n_stages = p.n_chunks * p.K;
    const int goff = (int)((m0 - left) & 15);          // LDS row lr <-> global row gr: (gr & 15) == (lr + goff) & 15

    if (tid < BM) {
        const long gr = m0 + tid;
        Ms[tid] = (gr < p.R) ? (p.valid ? p.valid[gr] : (uint8_t)1) : (uint8_t)0;
    }
    // epilogue parameters of the tile's 128 columns, staged now so that their latency hides behind the main loop:
    // [bias | BN scale | BN shift | alpha], alpha such that act(z) = max(z,0) + alpha*min(z,0) for none (1), relu (0), prelu.
    // Columns beyond Cout (ragged last tile) get scale = shift = 0 so they come out as exact zeros.
    if (tid >= BM && tid < BM + BN) {
        const int c = tid - BM, gc = n0 + c;
        const bool ok = gc < p.cout;
        Ps[c] = (ok && p.bias) ? p.bias[gc] : 0.f;
        Ps[BN + c] = ok ? (p.scale ? p.scale[gc] : 1.f) : 0.f;
        Ps[2 * BN + c] = (ok && p.shift) ? p.shift[gc] : 0.f;
        Ps[3 * BN + c] = p.act == XV_ACT_NONE ? 1.f : p.act == XV_ACT_LRELU ? p.alpha[0]
                       : (p.act == XV_ACT_PRELU && ok) ? p.alpha[gc] : 0.f;
    }

    // ---- B: one 16 KB tile per stage, 4 x 1 KB DMA pieces per wave ---------------------------------------
    const uint8_t *bsrc = p.wt + (size_t)nt * n_stages * B3_BYTES + wave * (BP * 1024) + lane * 16;
    auto dma_b = [&](int buf) {
        char *dst = Bbuf + buf * B3_BYTES + wave * (BP * 1024);
#pragma unroll
        for (int j = 0; j < BP; ++j) XV_GLDS16(bsrc + j * 1024, dst + j * 1024);
        bsrc += B3_BYTES;
    };

    // ---- A (split input): halo tile = rowsA rows x 128 B, DMA pieces of 8 rows --------------------------
    const size_t xrow_bytes = (size_t)p.xchunks * SROW;
    const uint8_t *asrc = nullptr;
    if constexpr (SPLIT_A)
        asrc = reinterpret_cast<const uint8_t *>(p.x) + (m0 - left + wave * 8 + (lane >> 3)) * (long)xrow_bytes + (lane & 7) * 16;
    const int n_pieces = (rowsA + 7) >> 3;             // <= BM/8 + 1
    auto dma_a = [&](int buf) {
        char *dst = Abuf + buf * A3_BYTES + wave * 1024;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int piece = wave + NW * j;
            if (piece < n_pieces) XV_GLDS16(asrc + (size_t)(8 * NW * j) * xrow_bytes, dst + j * (NW * 1024));
        }
        asrc += SROW;                                   // next 32-channel slab
    };

    // ---- A (fp32 input): load rows, split to hi/lo while writing the same LDS image -----------------------
    f32x4 areg[5];
    auto load_a = [&](int chunk) {
        const float *xf = reinterpret_cast<const float *>(p.x);
        const int c0 = chunk * BK;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int f = tid + NT * j;
            const int lr = f >> 3, qq = f & 7;
            const long gr = m0 - left + lr;
            const int c = c0 + qq * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (lr < rowsA && gr >= 0 && gr < p.R && c < p.cin) v = *reinterpret_cast<const f32x4 *>(xf + (size_t)gr * p.ldx + c);
            areg[j] = v;
        }
    };
    auto store_a = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int f = tid + NT * j;
            const int lr = f >> 3, qq = f & 7;
            if (lr < A_ROWS) {
                bf16x4 hi, lo;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    hi[i] = (__bf16)areg[j][i];
                    lo[i] = (__bf16)(areg[j][i] - (float)hi[i]);
                }
                const int sw = ((lr + goff) & 15) >> 1;
                char *row = Abuf + buf * A3_BYTES + lr * SROW + (qq & 1) * 8;
                *reinterpret_cast<bf16x4 *>(row + (((qq >> 1)) ^ sw) * 16) = hi;
                *reinterpret_cast<bf16x4 *>(row + ((4 + (qq >> 1)) ^ sw) * 16) = lo;
            }
        }
    };

    f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};

    // fragment addressing (B is stage-invariant up to the buffer toggle)
    const int arow0 = wr * 64 + (lane & 31);
    const int brow = wc * 64 + (lane & 31);
    const int kh = lane >> 5;
    const int boff0 = brow * 64, boff1 = (brow + 32) * 64;
    const int bsw0 = (brow >> 2) & 3, bsw1 = ((brow + 32) >> 2) & 3;

    struct Frags {            // fragments of one k-step (16 of the 32 channels of a stage): 8 x 4 VGPRs
        bf16x8 ah0, al0, ah1, al1, bh0, bl0, bh1, bl1;
    };
    auto load_frags = [&](Frags &F, int st, int ch, int tp, int ks) {
        const char *Ab = Abuf + (ch & 1) * A3_BYTES;
        const char *Bb = Bbuf + (st & 1) * B3_BYTES;
        const int lr0 = arow0 + tp * p.dil, lr1 = lr0 + 32;
        const int sw0 = ((lr0 + goff) & 15) >> 1, sw1 = ((lr1 + goff) & 15) >> 1;
        const char *a0 = Ab + lr0 * SROW, *a1 = Ab + lr1 * SROW;
        const int t = ks * 2 + kh;
        F.al0 = *reinterpret_cast<const bf16x8 *>(a0 + (((t + 4) ^ sw0) << 4));
        F.bh0 = *reinterpret_cast<const bf16x8 *>(Bb + boff0 + ((t ^ bsw0) << 4));
        F.bh1 = *reinterpret_cast<const bf16x8 *>(Bb + boff1 + ((t ^ bsw1) << 4));
        F.al1 = *reinterpret_cast<const bf16x8 *>(a1 + (((t + 4) ^ sw1) << 4));
        F.ah0 = *reinterpret_cast<const bf16x8 *>(a0 + ((t ^ sw0) << 4));
        F.bl0 = *reinterpret_cast<const bf16x8 *>(Bb + B3_PLANE + boff0 + ((t ^ bsw0) << 4));
        F.bl1 = *reinterpret_cast<const bf16x8 *>(Bb + B3_PLANE + boff1 + ((t ^ bsw1) << 4));
        F.ah1 = *reinterpret_cast<const bf16x8 *>(a1 + ((t ^ sw1) << 4));
    };
    auto mma = [&](const Frags &F) {
        acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.al0, F.bh0, acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.al0, F.bh1, acc01, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.al1, F.bh0, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.al1, F.bh1, acc11, 0, 0, 0);
        acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.ah0, F.bl0, acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.ah0, F.bl1, acc01, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.ah1, F.bl0, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.ah1, F.bl1, acc11, 0, 0, 0);
        acc00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.ah0, F.bh0, acc00, 0, 0, 0);
        acc01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.ah0, F.bh1, acc01, 0, 0, 0);
        acc10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.ah1, F.bh0, acc10, 0, 0, 0);
        acc11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(F.ah1, F.bh1, acc11, 0, 0, 0);
    };

    // Register-level software pipeline at k-step granularity (two 32-VGPR fragment sets F, G):
    //   iteration s:  G <- LDS(stage s, k-step 1) | 12 MFMAs on F (stage s, k-step 0)
    //                 barrier B(s)   [stage s fully read by everybody; stage s+1 landed]
    //                 DMA(stage s+2) into the buffers of stage s | F <- LDS(stage s+1, k-step 0) | 12 MFMAs on G
    // Each MFMA group hides the LDS latency of the other set's reads; a DMA has a full stage to land.
    int c1 = 0, t1 = 0;                       // (chunk, tap) of stage s+1
    auto advance = [&](int &c, int &t) { if (++t == p.K) { t = 0; ++c; } };

    dma_b(0);
    if constexpr (SPLIT_A) dma_a(0);
    else { load_a(0); store_a(0); }
    advance(c1, t1);
    if (n_stages > 1) {
        dma_b(1);
        if (t1 == 0) {
            if constexpr (SPLIT_A) dma_a(1);
            else { load_a(1); store_a(1); }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    Frags F = {}, G = {};
    if constexpr (!S16) load_frags(F, 0, 0, 0, 0);

    int c0 = 0, t0 = 0;                       // (chunk, tap) of stage s
    int c2 = c1, t2 = t1;                     // (chunk, tap) of stage s+2
    advance(c2, t2);
    f32x4 acc16[4][4];                        // S16: row tile i, column tile j of the wave's 64 x 64
    if constexpr (S16) {
        constexpr int NP = BM / 8 + 1;
        constexpr int DT = KT - 1;
        constexpr int NS = (NP + NW - 1) / NW;
        constexpr int PW = (NS + DT - 1) / DT;
        auto slots_of = [](int t) constexpr { return t < DT ? (NS + DT - 1 - t) / DT : 0; };
        auto slot_base = [](int t) constexpr { int b = 0; for (int u = 0; u < t; ++u) b += (NS + DT - 1 - u) / DT; return b; };
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc16[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // lane (row / column l & 15, k block l >> 4 = the 16-byte slot of the 32-channel slab).  A ds_read_b128 is served in four
        // groups of 16 lanes that mix two k blocks ({0-3, 12-15, 20-27}, ...): with tile row i = lane & 15 read where it lies, the
        // slot swizzles of the operand formats (made for 32-row fragments) collide two-way (SQ_LDS_BANK_CONFLICT 221 M cycles per
        // K = 7 launch against 1 M for the 32 x 32 form).  MFMA tile row / column i is therefore ROW16(i) / COL16(i) of the 16 --
        // permutations under which every lane group touches 16 different 16-byte chunks for every tap offset (found by
        // search over the bank model of MI355X_MICROARCH.md); the accumulators go back through the same maps.
        const int kb = lane >> 4;
        auto ROW16 = [](int i) { return (int)((0x48c67dbf391502eaull >> (4 * i)) & 15); };
        auto COL16 = [](int i) { return (int)((0xfedc76543210ba98ull >> (4 * i)) & 15); };
        int pa16[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int lr0 = wr * 64 + ROW16(lane & 15) + t * p.dil;
            pa16[t] = lr0 * SROW + (((((lr0 + goff) & 15) >> 1) ^ kb) << 4);      // (+ 16 i rows: the same swizzle; lo plane: ^ 64)
        }
        const int col16 = wc * 64 + COL16(lane & 15);
        const int pb16 = 2 * A3_BYTES + col16 * 64 + ((kb ^ ((col16 >> 2) & 3)) << 4);   // (+ 16 j columns: + 1024, the same swizzle)
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
        const uint8_t *bnext = bsrc;
        if (n_stages <= 2) bnext = bsrc - B3_BYTES;
        const uint8_t *abase = reinterpret_cast<const uint8_t *>(p.x) + (m0 - left + (lane >> 3)) * (long)xrow_bytes + (lane & 7) * 16;
        struct Set16 { bf16x8 ah[4], al[4], bh[4], bl[4]; };
        auto load16 = [&](Set16 &X, int abase_off, int bbase_off) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                X.ah[i] = *reinterpret_cast<const bf16x8 *>(lds + abase_off + i * 16 * SROW);
                X.al[i] = *reinterpret_cast<const bf16x8 *>(lds + (abase_off ^ 64) + i * 16 * SROW);
                X.bh[i] = *reinterpret_cast<const bf16x8 *>(lds + bbase_off + i * 1024);
                X.bl[i] = *reinterpret_cast<const bf16x8 *>(lds + bbase_off + B3_PLANE + i * 1024);
            }
        };
        auto mma16 = [&](const Set16 &X) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(X.al[i], X.bh[j], acc16[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(X.ah[i], X.bl[j], acc16[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(X.ah[i], X.bh[j], acc16[i][j], 0, 0, 0);
        };
        Set16 F16, G16;
        load16(F16, pa16[0], pb16);
        int s = 0;
        for (int c = 0; c < p.n_chunks; c += 2) {         // two slabs per trip: the fragment sets swap roles every stage, K is odd
            auto stage = [&](auto UU) {
                constexpr int u = decltype(UU)::value;
                constexpr int t = u % KT;
                const int cc = c + u / KT;
                const int abuf = (cc & 1) * A3_BYTES;
                const int cn = (cc + 1 < p.n_chunks) ? cc + 1 : p.n_chunks - 1;
                const uint8_t *anext = abase + (size_t)cn * SROW;
                char *adst_n = Abuf + (cn & 1) * A3_BYTES;
                const int bbuf = (s & 1) * B3_BYTES;
                // stage s is in registers (everybody's reads of it have returned), stage s+1 has landed
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __syncthreads();
                {
                    char *dst = Bbuf + bbuf + wave * (BP * 1024);
                    XV_GLDS16_OFF(bnext, dst, 0);
                    XV_GLDS16_OFF(bnext, dst, 1024);
                    if constexpr (BP == 4) {
                        XV_GLDS16_OFF(bnext, dst, 2048);
                        XV_GLDS16_OFF(bnext, dst, 3072);
                    }
                    bnext += (s + 3 < n_stages) ? B3_BYTES : 0;
                }
                if constexpr (t < KT - 1) {
#pragma unroll
                    for (int j = 0; j < slots_of(t); ++j) XV_GLDS16(anext + ag_off[t][j], adst_n + al_off[t][j]);
                }
                const int a_next = (t + 1 < KT) ? pa16[(t + 1) % KT] + abuf : pa16[0] + (A3_BYTES - abuf);
                if constexpr ((u & 1) == 0) { load16(G16, a_next, pb16 + (B3_BYTES - bbuf)); mma16(F16); }
                else { load16(F16, a_next, pb16 + (B3_BYTES - bbuf)); mma16(G16); }
                constexpr int NV = BP + slots_of(t);
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // 1 VMEM read (LDS-DMA piece)
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // 1 DS read
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 48 - 32 - NV, 0);
                __builtin_amdgcn_sched_barrier(0);
                ++s;
            };
            for_taps<0, 2 * KT>(stage);
        }
    } else if constexpr (SPLIT_A) {
        // Straight-line iteration body (no branches): DMA is issued unconditionally (clamped at the tail, where it
        // rewrites identical bytes), so that sched_group_barrier can interleave every memory instruction with the
        // MFMAs of the same wave: the wave overlaps its own memory issue instead of relying on the co-resident block.
        constexpr int NP = KT == 1 ? BM / 8 : BM / 8 + 1;   // pieces of a halo tile: BM + (K-1)*dil rows, (K-1)*dil in 2..8
        constexpr int DT = KT == 1 ? 1 : KT - 1;            // taps that carry A pieces
        // a "slot" = one piece per wave; the NS slots a halo tile needs are dealt to the taps as evenly as possible,
        // early taps first (K=7: 1,1,1,1,1,0  K=5: 2,1,1,1  K=3: 3,2  K=1: 4), so that at most NW-1 pieces per slab are
        // clamped duplicates
        constexpr int NS = (NP + NW - 1) / NW;
        constexpr int PW = (NS + DT - 1) / DT;              // most slots any tap carries
        auto slots_of = [](int t) constexpr { return t < DT ? (NS + DT - 1 - t) / DT : 0; };
        auto slot_base = [](int t) constexpr { int b = 0; for (int u = 0; u < t; ++u) b += (NS + DT - 1 - u) / DT; return b; };
        // per-tap, per-lane fragment row offset in A buffer 0 with the slot swizzle and the lane's k-half folded in:
        // the 16-B slot T of a row sits at ((T ^ sw) << 4), T = ks*2 + kh (+4 for lo)  ->  pa ^ (ks << 5) ^ (lo << 6)
        int pa[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            const int lr0 = arow0 + t * p.dil;
            pa[t] = lr0 * SROW + (((((lr0 + goff) & 15) >> 1) ^ kh) << 4);
        }
        // B fragments: (col + 32) has the same swizzle, the lo plane is +B3_PLANE -> immediates; per k-step one base
        int pb[2];
        pb[0] = 2 * A3_BYTES + boff0 + ((kh ^ bsw0) << 4);
        pb[1] = 2 * A3_BYTES + boff0 + (((2 + kh) ^ bsw0) << 4);
        // A-halo DMA schedule of this wave: byte offset of piece (t, j) in the split buffer / in an LDS A buffer
        const uint32_t rowstep = 8u * (uint32_t)xrow_bytes;
        uint32_t ag_off[DT][PW], al_off[DT][PW];
#pragma unroll
        for (int t = 0; t < DT; ++t)
#pragma unroll
            for (int j = 0; j < PW; ++j) {
                int piece = (slot_base(t) + j) * NW + wave;      // slots beyond slots_of(t) are never issued
                piece = piece < NP ? piece : NP - 1;
                ag_off[t][j] = (uint32_t)piece * rowstep;
                al_off[t][j] = (uint32_t)piece * 1024u;
            }
        const uint8_t *bnext = bsrc;                         // tile of stage min(s+2, n_stages-1)
        if (n_stages <= 2) bnext = bsrc - B3_BYTES;
        const uint8_t *abase = reinterpret_cast<const uint8_t *>(p.x) + (m0 - left + (lane >> 3)) * (long)xrow_bytes + (lane & 7) * 16;
        auto load_a_frags = [&](Frags &X, int base, int ks) {       // base = pa[t] (+ buffer offset), ks compile-time
            const char *a = lds + (base ^ (ks << 5));
            const char *al = lds + (base ^ (ks << 5) ^ 64);
            X.al0 = *reinterpret_cast<const bf16x8 *>(al);
            X.al1 = *reinterpret_cast<const bf16x8 *>(al + 32 * SROW);
            X.ah0 = *reinterpret_cast<const bf16x8 *>(a);
            X.ah1 = *reinterpret_cast<const bf16x8 *>(a + 32 * SROW);
        };
        auto load_b_frags = [&](Frags &X, int base) {               // base = pb[ks] + stage buffer offset
            const char *b = lds + base;
            X.bh0 = *reinterpret_cast<const bf16x8 *>(b);
            X.bh1 = *reinterpret_cast<const bf16x8 *>(b + 32 * 64);
            X.bl0 = *reinterpret_cast<const bf16x8 *>(b + B3_PLANE);
            X.bl1 = *reinterpret_cast<const bf16x8 *>(b + B3_PLANE + 32 * 64);
        };
        int s = 0;
        for (int c = 0; c < p.n_chunks; ++c) {
            const int abuf = (c & 1) * A3_BYTES;                     // A buffer of slab c / of slab c+1
            const int abuf_n = A3_BYTES - abuf;
            // slab whose halo is loaded while slab c is consumed (K > 1), clamped at the tail
            const int cn = (c + 1 < p.n_chunks) ? c + 1 : p.n_chunks - 1;
            const uint8_t *anext = abase + (size_t)cn * SROW;
            char *adst_n = Abuf + (cn & 1) * A3_BYTES;
            auto tap = [&](auto TT) {
                constexpr int t = decltype(TT)::value;
                const int bbuf = (s & 1) * B3_BYTES;
                // ---- phase 1: G <- LDS(stage s, k-step 1) interleaved with the 12 MFMAs on F -----------------------
                load_a_frags(G, pa[t] + abuf, 1);
                load_b_frags(G, pb[1] + bbuf);
                mma(F);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // 1 DS read
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();                  // B(s): stage s fully read by everybody, stage s+1 landed
                // ---- phase 2: DMA(s+2), F <- LDS(stage s+1, k-step 0), 12 MFMAs on G --------------------------------
                {
                    char *dst = Bbuf + bbuf + wave * (BP * 1024);    // one M0; the immediate advances source AND destination
                    XV_GLDS16_OFF(bnext, dst, 0);
                    XV_GLDS16_OFF(bnext, dst, 1024);
                    if constexpr (BP == 4) {
                        XV_GLDS16_OFF(bnext, dst, 2048);
                        XV_GLDS16_OFF(bnext, dst, 3072);
                    }
                    bnext += (s + 3 < n_stages) ? B3_BYTES : 0;
                }
                if constexpr (KT == 1) {
                    // every stage is its own slab: all 16 pieces of slab min(s+2, last) now, into the buffer of slab s
                    const int ca = (s + 2 < p.n_chunks) ? s + 2 : p.n_chunks - 1;
                    const uint8_t *ag = abase + (size_t)ca * SROW;
                    char *adst = Abuf + (ca & 1) * A3_BYTES;
#pragma unroll
                    for (int j = 0; j < PW; ++j) XV_GLDS16(ag + ag_off[0][j], adst + al_off[0][j]);
                } else if constexpr (t < KT - 1) {
#pragma unroll
                    for (int j = 0; j < slots_of(t); ++j) XV_GLDS16(anext + ag_off[t][j], adst_n + al_off[t][j]);
                }
                if constexpr (t + 1 < KT) load_a_frags(F, pa[t + 1] + abuf, 0);
                else load_a_frags(F, pa[0] + abuf_n, 0);             // first tap of the next slab (tail: harmless read)
                load_b_frags(F, pb[0] + (B3_BYTES - bbuf));
                mma(G);
                constexpr int NV = BP + (KT == 1 ? PW : slots_of(t));
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // 1 VMEM read (LDS-DMA piece)
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);      // 2 DS reads
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 12 - (4 + NV) > 0 ? 12 - (4 + NV) : 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                ++s;
            };
            for_taps<0, KT>(tap);
        }
    } else {
        for (int s = 0; s < n_stages; ++s) {
            load_frags(G, s, c0, t0, 1);
            __builtin_amdgcn_sched_barrier(0);
            mma(F);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();                  // B(s)
            const bool dma2 = (s + 2) < n_stages;
            const bool newa2 = dma2 && (t2 == 0);
            if (dma2) {
                dma_b(s & 1);
                if (newa2) load_a(c2);
            }
            if (s + 1 < n_stages) load_frags(F, s + 1, c1, t1, 0);
            __builtin_amdgcn_sched_barrier(0);
            mma(G);
            __builtin_amdgcn_sched_barrier(0);
            if (newa2) store_a(c2 & 1);
            c0 = c1; t0 = t1;
            advance(c1, t1);
            advance(c2, t2);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- epilogue: accumulators -> LDS fp32 tile (the operand buffers are dead after the last barrier) ------
    float *T = reinterpret_cast<float *>(lds);
    if constexpr (S16) {
        const int col = wc * 64 + (int)((0xfedc76543210ba98ull >> (4 * (lane & 15))) & 15);                 // COL16
        int rows4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) rows4[e] = wr * 64 + (int)((0x48c67dbf391502eaull >> (4 * (4 * (lane >> 4) + e))) & 15);   // ROW16
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) T[(rows4[e] + 16 * i) * T_LD + col + 16 * j] = acc16[i][j][e];
    } else {
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
    const bool full = gc0 + 8 <= p.cout;
    const bool lrelu = p.act == XV_ACT_LRELU;           // tf.nn.leaky_relu is max(alpha*z, z) for ANY alpha
    auto activate = [&](float z, float a) { return lrelu ? fmaxf(a * z, z) : fmaxf(z, 0.f) + a * fminf(z, 0.f); };
    if constexpr (POOL) {
        // thread = (8-row block tid>>4 of the tile, 8 channels): statistics of the block's valid rows, shifted by the
        // block's first row so that s2 - s1^2/n does not cancel.  Blocks are aligned to global row multiples of 8;
        // callers start every chunk on such a row, so a block never mixes two chunks and its statistics do not depend
        // on where the chunk sits in the batch.
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
        __builtin_amdgcn_sched_barrier(0);
        auto rows = [&](auto MODE) {                   // 0: max(z,0) + alpha*min(z,0)   1: leaky max(alpha*z, z)   2: plain ReLU
            constexpr int mode = decltype(MODE)::value;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                n += keep[j];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float z = (i < 4 ? tv[j][0][i] : tv[j][1][i - 4]) + bias[i];
                    const float a = mode == 1 ? fmaxf(al[i] * z, z) : mode == 2 ? fmaxf(z, 0.f) : fmaxf(z, 0.f) + al[i] * fminf(z, 0.f);
                    const float v = a * sc[i] + sh[i];
                    if (j == 0) { v0[i] = v; s1[i] = 0.f; s2[i] = 0.f; }
                    else {
                        const float d = keep[j] != 0.f ? v - v0[i] : 0.f;      // (a select: a row past R may hold anything, NaN * 0 is NaN)
                        s1[i] += d;
                        s2[i] += d * d;
                    }
                }
            }
        };
        if (lrelu) rows(std::integral_constant<int, 1>{});
        else if (p.act == XV_ACT_RELU) rows(std::integral_constant<int, 2>{});
        else rows(std::integral_constant<int, 0>{});
        // row 0 of a block is valid whenever any row is (chunks start on block boundaries, gaps follow the frames)
        const float rn = n > 0.f ? 1.f / n : 0.f;
        float mean[8], m2[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            mean[i] = n > 0.f ? v0[i] + s1[i] * rn : 0.f;
            m2[i] = fmaxf(s2[i] - s1[i] * s1[i] * rn, 0.f);
        }
        float *o = p.blk + ((size_t)((m0 >> 3) + blk) * 2) * p.cout + gc0;
        if (full && !(p.cout & 3)) {
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
    }
    if (p.y && p.y_split && !p.ypre && n0 + BN <= p.cout) {
        // fast path (hidden layers): full-width tile into the split format, straight-line.  Rows >= R of the last tile
        // land in the buffer's zero padding (XV_SPLIT_PAD_AFTER >= BM) and are written as zeros (keep == 0).
        const int ch = gc0 >> 5, slot = cg & 3;
        char *ybase = reinterpret_cast<char *>(p.y) + (size_t)ch * SROW;
        const size_t yrow = (size_t)p.ychunks * SROW;
        // all 16 LDS reads first: the LDS pipe is kept busy by the co-resident workgroup's main loop, so a round trip costs
        // ~1 us under load -- pay it once, not once per row
        f32x4 tv[8][2];
        float keep[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int lr = (tid >> 4) + (NT / 16) * j;
            tv[j][0] = *reinterpret_cast<const f32x4 *>(T + lr * T_LD + cg * 8);
            tv[j][1] = *reinterpret_cast<const f32x4 *>(T + lr * T_LD + cg * 8 + 4);
            keep[j] = Ms[lr] ? 1.f : 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);
        // every instruction here competes with the co-resident workgroup's MFMA stream for issue slots (an epilogue takes
        // 5-15 us of wall time for ~500 VALU instructions), so the common cases are specialised at compile time: plain ReLU
        // (no alpha term) and threads none of whose 8 rows is a gap row (no mask multiply; ~99 % of threads)
        auto rows = [&](auto MODE, auto MASKED) {
            constexpr int mode = decltype(MODE)::value;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long gr = m0 + (tid >> 4) + (NT / 16) * j;
                bf16x8 hi, lo;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float z = (i < 4 ? tv[j][0][i] : tv[j][1][i - 4]) + bias[i];
                    const float a = mode == 1 ? fmaxf(al[i] * z, z) : mode == 2 ? fmaxf(z, 0.f) : fmaxf(z, 0.f) + al[i] * fminf(z, 0.f);
                    float v = a * sc[i] + sh[i];
                    if constexpr (decltype(MASKED)::value) v *= keep[j];
                    hi[i] = (__bf16)v;
                    lo[i] = (__bf16)(v - (float)hi[i]);
                }
                const int sw = (int)(gr >> 1) & 7;
                char *row = ybase + (size_t)gr * yrow;
                __builtin_nontemporal_store(hi, reinterpret_cast<bf16x8 *>(row + ((slot ^ sw) << 4)));
                __builtin_nontemporal_store(lo, reinterpret_cast<bf16x8 *>(row + (((4 + slot) ^ sw) << 4)));
            }
        };
        const bool masked = keep[0] * keep[1] * keep[2] * keep[3] * keep[4] * keep[5] * keep[6] * keep[7] == 0.f;
        auto run = [&](auto MODE) {
            if (masked) rows(MODE, std::true_type{});
            else rows(MODE, std::false_type{});
        };
        if (lrelu) run(std::integral_constant<int, 1>{});
        else if (p.act == XV_ACT_RELU) run(std::integral_constant<int, 2>{});
        else run(std::integral_constant<int, 0>{});
        return;
    }
    // column sums (training, see Gemm3Params::cs_part): the rows of the other factor are fetched before anything else so that
    // their latency is paid once; cout % 8 == 0 is the launcher's condition, so a column group is inside or outside as a whole
    const bool sums = p.cs_part != nullptr;             // (uniform)
    const bool sums_self = sums && p.cs_r == nullptr;   // (uniform)
    f32x4 rq[8][2];
    float cs1[8], cs2[8];
    double ds1[8], ds2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        cs1[i] = cs2[i] = 0.f;
        ds1[i] = ds2[i] = 0.0;
    }
    if (sums && !sums_self) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long gr = m0 + (tid >> 4) + (NT / 16) * j;
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            rq[j][0] = rq[j][1] = zero4;
            if (gr < p.R && full) {
                const float *rr = p.cs_r + (size_t)gr * p.cs_ldr + gc0;
                rq[j][0] = *reinterpret_cast<const f32x4 *>(rr);
                rq[j][1] = *reinterpret_cast<const f32x4 *>(rr + 4);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int lr = (tid >> 4) + (NT / 16) * j;
        const long gr = m0 + lr;
        if (gr >= p.R) continue;
        const f32x4 t0 = *reinterpret_cast<const f32x4 *>(T + lr * T_LD + cg * 8);
        const f32x4 t1 = *reinterpret_cast<const f32x4 *>(T + lr * T_LD + cg * 8 + 4);
        float z[8], v[8];
        const float keep = Ms[lr] ? 1.f : 0.f;          // gap rows: one multiply per element instead of a select
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            z[i] = (i < 4 ? t0[i] : t1[i - 4]) + bias[i];
            v[i] = (activate(z[i], al[i]) * sc[i] + sh[i]) * keep;
        }
        if (sums_self) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double d = (double)v[i];
                ds1[i] += d;
                ds2[i] = __builtin_fma(d, d, ds2[i]);
            }
        } else if (sums) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                cs1[i] += v[i];
                cs2[i] = __builtin_fmaf(v[i], i < 4 ? rq[j][0][i] : rq[j][1][i - 4], cs2[i]);
            }
        }
        if (p.ypre) {
            float *o = p.ypre + (size_t)gr * p.ldpre + gc0;
            if (full && !(p.ldpre & 3)) {
                *reinterpret_cast<f32x4 *>(o) = (f32x4){z[0], z[1], z[2], z[3]};
                *reinterpret_cast<f32x4 *>(o + 4) = (f32x4){z[4], z[5], z[6], z[7]};
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (gc0 + i < p.cout) o[i] = z[i];
            }
        }
        if (p.y) {
            if (p.y_split) {
                const int ch = gc0 >> 5;
                if (ch < p.ychunks) {
                    bf16x8 hi, lo;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        hi[i] = (__bf16)v[i];
                        lo[i] = (__bf16)(v[i] - (float)hi[i]);
                    }
                    const int sw = (int)(gr >> 1) & 7;
                    const int slot = cg & 3;
                    char *row = reinterpret_cast<char *>(p.y) + ((size_t)gr * p.ychunks + ch) * SROW;
                    __builtin_nontemporal_store(hi, reinterpret_cast<bf16x8 *>(row + ((slot ^ sw) << 4)));
                    __builtin_nontemporal_store(lo, reinterpret_cast<bf16x8 *>(row + (((4 + slot) ^ sw) << 4)));
                }
            } else {
                float *o = reinterpret_cast<float *>(p.y) + (size_t)gr * p.ldy + gc0;
                if (full && !(p.ldy & 3)) {
                    __builtin_nontemporal_store((f32x4){v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4 *>(o));
                    __builtin_nontemporal_store((f32x4){v[4], v[5], v[6], v[7]}, reinterpret_cast<f32x4 *>(o + 4));
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (gc0 + i < p.cout) o[i] = v[i];
                }
            }
        }
    }
    if (sums) {
        // a thread holds 8 rows x 8 columns (fp32); the NT / 16 row groups of a column are added in double, in group order
        constexpr int NG = NT / 16;
        __syncthreads();                                // every thread has read its rows of T
        double *D = reinterpret_cast<double *>(lds);    // [2][NG][BN]
        const int g = tid >> 4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            D[(0 * NG + g) * BN + cg * 8 + i] = sums_self ? ds1[i] : (double)cs1[i];
            D[(1 * NG + g) * BN + cg * 8 + i] = sums_self ? ds2[i] : (double)cs2[i];
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid >> 7, col = tid & (BN - 1);
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < NG; ++k) a += D[(which * NG + k) * BN + col];
            if (n0 + col < p.cout) p.cs_part[((size_t)mt * 2 + which) * p.cout + n0 + col] = a;
        }
    }
}

typedef void (*gemm3_fn)(const Gemm3Params);
struct Gemm3Kernel {
    int kt;       // 0: fp32-row input (runtime K), else the compile-time kernel size of the split-input path
    bool pool;
    int wm;
    gemm3_fn fn;
    bool s16 = false;
};
#define XV_G3(SPLIT, KT, POOL, WM) {KT, POOL, WM, tdnn_gemm_bf16x3_kernel<SPLIT, KT, POOL, WM>}
const Gemm3Kernel GEMM3_KERNELS[] = {
    XV_G3(false, 0, false, 2), XV_G3(false, 0, true, 2),
    XV_G3(true, 1, false, 2), XV_G3(true, 3, false, 2), XV_G3(true, 5, false, 2), XV_G3(true, 7, false, 2),
    XV_G3(true, 1, true, 2),  XV_G3(true, 3, true, 2),  XV_G3(true, 5, true, 2),  XV_G3(true, 7, true, 2),
    XV_G3(true, 1, false, 4), XV_G3(true, 3, false, 4), XV_G3(true, 5, false, 4), XV_G3(true, 7, false, 4),
    XV_G3(true, 1, true, 4),  XV_G3(true, 3, true, 4),  XV_G3(true, 5, true, 4),  XV_G3(true, 7, true, 4),
    // the 16 x 16 MFMA form (split input, K > 1)
#define XV_G3S(KT, POOL, WM) {KT, POOL, WM, tdnn_gemm_bf16x3_kernel<true, KT, POOL, WM, true>, true}
    XV_G3S(3, false, 2), XV_G3S(5, false, 2), XV_G3S(7, false, 2), XV_G3S(3, true, 2), XV_G3S(5, true, 2), XV_G3S(7, true, 2),
    XV_G3S(3, false, 4), XV_G3S(5, false, 4), XV_G3S(7, false, 4), XV_G3S(3, true, 4), XV_G3S(5, true, 4), XV_G3S(7, true, 4),
#undef XV_G3S
};
#undef XV_G3
const Gemm3Kernel *find_gemm3(int kt, bool pool, int wm, bool s16 = false)
{
    for (const Gemm3Kernel &e : GEMM3_KERNELS)
        if (e.kt == kt && e.pool == pool && e.wm == wm && e.s16 == s16) return &e;
    return nullptr;
}

// tuning knob (xv_set_tuning(XV_TUNE_TILE_ROWS) through xv_internal_gemm3_tile_rows): 0 = built-in choice, 128 or 256
std::atomic<int> g_tile_rows{0};

int launch_gemm3(const Gemm3Params &p0, hipStream_t st)
{
    Gemm3Params p = p0;
    if (p.R <= 0 || p.cout <= 0) return 0;
    if (p.cin <= 0 || p.K <= 0 || (p.K & 1) == 0 || p.dil <= 0) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3: K must be odd, dims > 0");
    if ((p.K - 1) * p.dil > MAX_SPAN) return fail(XV_ERR_UNSUPPORTED, "tdnn_bf16x3: (K-1)*dilation > 8 unsupported");
    if ((p.act == XV_ACT_LRELU || p.act == XV_ACT_PRELU) && !p.alpha) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3: act_alpha is NULL");
    p.n_chunks = (p.cin + BK - 1) / BK;
    if (p.x_split) {
        p.xchunks = p.n_chunks;
        if (((uintptr_t)p.x) & 15) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3: split input must be 16-byte aligned");
    } else {
        if (p.ldx < p.cin) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3: ldx < cin");
        if ((p.cin & 3) || (p.ldx & 3) || (((uintptr_t)p.x) & 15))
            return fail(XV_ERR_UNSUPPORTED, "tdnn_bf16x3: fp32 input needs Cin and ldx multiples of 4 and a 16-byte aligned pointer");
    }
    if (p.y) {
        if (p.y_split) {
            p.ychunks = (p.cout + 31) / 32;
            if (((uintptr_t)p.y) & 15) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3: split output must be 16-byte aligned");
        } else if (p.ldy < p.cout || (((uintptr_t)p.y) & 15)) {
            return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3: ldy < cout or output not 16-byte aligned");
        }
    }
    if (p.ypre && (p.ldpre < p.cout || (((uintptr_t)p.ypre) & 15))) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3: bad y_preact");
    if (((uintptr_t)p.wt) & 15) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3: packed weights must be 16-byte aligned");
    p.n_nt = (p.cout + BN - 1) / BN;
    int kt = 0;
    if (p.x_split) {
        kt = p.K;
        const int span = (p.K - 1) * p.dil;
        if ((kt != 1 && kt != 3 && kt != 5 && kt != 7) || (kt > 1 && (span < 2 || span > MAX_SPAN)))
            return fail(XV_ERR_UNSUPPORTED, "tdnn_bf16x3: split-format input supports K in {1,3,5,7} with (K-1)*dilation <= 8");
    }
    // workgroup tile: 256 rows (8 waves, one workgroup per CU) for the wide-context layers when the input is in the split
    // format and there are enough rows to fill the chip with such tiles, else 128 rows (4 waves, two per CU);
    // xv_set_tuning(XV_TUNE_TILE_ROWS) overrides
    // the 16 x 16 MFMA form where it exists: split input, K > 1, an even number of 32-channel slabs
    const bool s16 = p.x_split && kt > 1 && (p.n_chunks & 1) == 0;
    int wm = 2;
    if (p.x_split) {
        const int want = g_tile_rows.load(std::memory_order_relaxed);
        // measured on 262144-row batches (tools/layer_bench.py, profiles/r02a_layer_tile.txt): K = 7 +2.7 %, K = 5 +1.2 %,
        // K = 1 -1.5 ... -3.5 % (with one workgroup per CU the prologue and epilogue of a 16-stage tile are exposed).  The
        // 16 x 16 form is faster on 128-row tiles (K = 5 1.306 against 1.357 ms, K = 7 1.759 against 1.773)
        const bool big_enough = ((p.R + 255) / 256) * p.n_nt >= 512;          // two rounds of 256 CUs
        if (want == 256 || (want == 0 && p.K >= 5 && big_enough && !s16)) wm = 4;
    }
    if (p.cs_part) wm = 2;                                   // one partial per 128 rows: the split xv_col_sums_merge_f32 walks
    p.n_mt = (int)((p.R + wm * 64 - 1) / (wm * 64));
    const Gemm3Kernel *k = find_gemm3(kt, p.blk != nullptr, wm, s16);
    if (!k) return fail(XV_ERR_UNSUPPORTED, "tdnn_bf16x3: no kernel for this configuration");
    static std::atomic<unsigned long long> lds_done{0};
    if (const int rc = opt_in_dynamic_lds(lds_done, GEMM3_KERNELS, [](const Gemm3Kernel &e) { return std::make_pair(e.fn, gemm3_lds_bytes(e.wm)); }))
        return rc;
    hipLaunchKernelGGL(k->fn, dim3((unsigned)(p.n_mt * p.n_nt)), dim3(wm * 128), gemm3_lds_bytes(wm), st, p);
    return launch_status("tdnn_gemm_bf16x3_kernel launch");
}

// w[K, cin, cout] fp32 -> tiled bf16x3 weights: tile (nt, chunk, tap) = 16 KB [hi 128x64B][lo 128x64B], slots swizzled
__global__ void pack_weights_bf16x3_kernel(const float *__restrict__ w, int K, int cin, int cout, int n_chunks,
                                           uint8_t *__restrict__ wt, size_t total)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // one (tile, col, k) element
    if (i >= total) return;
    const int k = (int)(i & 31);
    const int n = (int)((i >> 5) & 127);
    const size_t tile = i >> 12;
    const int tap = (int)(tile % K);
    const int chunk = (int)((tile / K) % n_chunks);
    const int nt = (int)(tile / ((size_t)K * n_chunks));
    const int c = chunk * 32 + k, gn = nt * 128 + n;
    const float x = (c < cin && gn < cout) ? w[((size_t)tap * cin + c) * cout + gn] : 0.f;
    const __bf16 hi = (__bf16)x;
    const __bf16 lo = (__bf16)(x - (float)hi);
    uint8_t *t = wt + tile * B3_BYTES + n * 64 + (((k >> 3) ^ ((n >> 2) & 3)) << 4) + (k & 7) * 2;
    *reinterpret_cast<uint16_t *>(t) = __builtin_bit_cast(uint16_t, hi);
    *reinterpret_cast<uint16_t *>(t + B3_PLANE) = __builtin_bit_cast(uint16_t, lo);
}

// The same tiles for MANY layers in one launch, each in one or both of two orientations (the training step re-packs every
// weight after every optimizer step: sixteen launches and as many torch flip / permute / cat kernels per step before this):
//   forward   wt_fwd = pack(w[K, cin_pad, cout])                                    (columns cin .. cin_pad-1 read as zero)
//   backward  wt_bwd = pack(w'[K, cout, cin_pad]),  w'[k, o, c] = w[K-1-k, c, o]    (the input-gradient GEMM's operand)
struct PackJob {
    const float *w;
    uint8_t *wt;
    int K, cin_src, cin, cout, cout_src;      // logical [K, cin, cout] of the tiles; the source is w[K, cin_src, cout_src]
    int transposed;
    unsigned first_block;
    unsigned long long total;
};
constexpr int PACK_MAX_JOBS = 24;
struct PackJobs {
    int n;
    PackJob j[PACK_MAX_JOBS];
};

__global__ void pack_weights_bf16x3_many_kernel(const PackJobs jobs)
{
    int ji = 0;
#pragma unroll 1
    for (int t = 1; t < jobs.n; ++t)
        if (blockIdx.x >= jobs.j[t].first_block) ji = t;
    const PackJob &J = jobs.j[ji];
    // one thread per 16-byte slot (8 channels of one column): the four slots of a column's 64-byte row are neighbouring lanes, so a wave
    // writes 1 KB contiguous per plane; the transposed orientation also READS 32 contiguous bytes per thread
    const size_t i = (size_t)(blockIdx.x - J.first_block) * blockDim.x + threadIdx.x;
    if (i >= J.total) return;
    const int n_chunks = (J.cin + BK - 1) / BK;
    const int k8 = (int)(i & 3);
    const int n = (int)((i >> 2) & 127);
    const size_t tile = i >> 9;
    const int tap = (int)(tile % J.K);
    const int chunk = (int)((tile / J.K) % n_chunks);
    const int nt = (int)(tile / ((size_t)J.K * n_chunks));
    const int c0 = chunk * 32 + k8 * 8, gn = nt * 128 + n;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = 0.f;
    if (gn < J.cout) {
        if (!J.transposed) {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c0 + e < J.cin_src) x[e] = J.w[((size_t)tap * J.cin_src + c0 + e) * J.cout_src + gn];
        } else if (gn < J.cin_src) {                       // logical input channel c = source column, output gn = source row
            const float *row = J.w + ((size_t)(J.K - 1 - tap) * J.cin_src + gn) * J.cout_src;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c0 + e < J.cin) x[e] = row[c0 + e];
        }
    }
    bf16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        hi[e] = (__bf16)x[e];
        lo[e] = (__bf16)(x[e] - (float)hi[e]);
    }
    uint8_t *t = J.wt + tile * B3_BYTES + n * 64 + ((k8 ^ ((n >> 2) & 3)) << 4);
    *reinterpret_cast<bf16x8 *>(t) = hi;
    *reinterpret_cast<bf16x8 *>(t + B3_PLANE) = lo;
}

// fp32 rows -> split format (test / tooling helper; the layers write the format themselves)
__global__ void split_encode_kernel(const float *__restrict__ x, long R, int c, int ldx, uint8_t *__restrict__ xs, int chunks)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)R * chunks * 32) return;
    const int k = (int)(i & 31);
    const int ch = (int)((i >> 5) % chunks);
    const long r = (long)(i / ((size_t)32 * chunks));
    const int cc = ch * 32 + k;
    const float v = cc < c ? x[(size_t)r * ldx + cc] : 0.f;
    const __bf16 hi = (__bf16)v;
    const __bf16 lo = (__bf16)(v - (float)hi);
    const int sw = (int)(r >> 1) & 7;
    uint8_t *row = xs + ((size_t)r * chunks + ch) * SROW + (k & 7) * 2;
    *reinterpret_cast<uint16_t *>(row + (((k >> 3) ^ sw) << 4)) = __builtin_bit_cast(uint16_t, hi);
    *reinterpret_cast<uint16_t *>(row + (((4 + (k >> 3)) ^ sw) << 4)) = __builtin_bit_cast(uint16_t, lo);
}

__global__ void split_decode_kernel(const uint8_t *__restrict__ xs, long R, int c, int chunks, float *__restrict__ x, int ldx)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)R * c) return;
    const long r = (long)(i / c);
    const int cc = (int)(i - (size_t)r * c);
    const int ch = cc >> 5, k = cc & 31;
    const int sw = (int)(r >> 1) & 7;
    const uint8_t *row = xs + ((size_t)r * chunks + ch) * SROW + (k & 7) * 2;
    const uint16_t h = *reinterpret_cast<const uint16_t *>(row + (((k >> 3) ^ sw) << 4));
    const uint16_t l = *reinterpret_cast<const uint16_t *>(row + (((4 + (k >> 3)) ^ sw) << 4));
    x[(size_t)r * ldx + cc] = __builtin_bit_cast(float, (uint32_t)h << 16) + __builtin_bit_cast(float, (uint32_t)l << 16);
}

}  // namespace

extern "C" {

void xv_internal_gemm3_tile_rows(int value) { g_tile_rows.store(value, std::memory_order_relaxed); }

size_t xv_packed_weights_bf16x3_bytes(int K, int cin, int cout)
{
    if (K <= 0 || cin <= 0 || cout <= 0) return 0;
    return (size_t)((cout + BN - 1) / BN) * ((cin + BK - 1) / BK) * K * B3_BYTES;
}

int xv_pack_weights_bf16x3(const float *w, int K, int cin, int cout, void *wt, void *stream)
{
    if (!w || !wt || K <= 0 || cin <= 0 || cout <= 0) return fail(XV_ERR_BAD_ARG, "pack_weights_bf16x3: bad argument");
    const int n_chunks = (cin + BK - 1) / BK;
    const size_t total = xv_packed_weights_bf16x3_bytes(K, cin, cout) / 4;      // 4 bytes (hi+lo) per element
    hipLaunchKernelGGL(pack_weights_bf16x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, K,
                       cin, cout, n_chunks, (uint8_t *)wt, total);
    return launch_status("pack_weights_bf16x3_kernel");
}

int xv_pack_weights_bf16x3_many(int n, const float *const *w, const int32_t *K, const int32_t *cin, const int32_t *cin_pad,
                                const int32_t *cout, void *const *wt_fwd, void *const *wt_bwd, void *stream)
{
    if (n <= 0) return 0;
    if (!w || !K || !cin || !cin_pad || !cout || !wt_fwd || !wt_bwd) return fail(XV_ERR_BAD_ARG, "pack_weights_bf16x3_many: NULL pointer");
    PackJobs jobs{};
    unsigned blocks = 0;
    auto flush = [&]() -> int {
        if (jobs.n == 0) return 0;
        hipLaunchKernelGGL(pack_weights_bf16x3_many_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, jobs);
        jobs.n = 0;
        blocks = 0;
        return launch_status("pack_weights_bf16x3_many_kernel");
    };
    for (int i = 0; i < n; ++i) {
        if (!w[i] || K[i] <= 0 || cin[i] <= 0 || cin_pad[i] < cin[i] || cout[i] <= 0)
            return fail(XV_ERR_BAD_ARG, "pack_weights_bf16x3_many: bad layer shape");
        for (int dir = 0; dir < 2; ++dir) {
            void *dst = dir ? wt_bwd[i] : wt_fwd[i];
            if (!dst) continue;
            if (((uintptr_t)dst) & 15) return fail(XV_ERR_BAD_ARG, "pack_weights_bf16x3_many: destinations must be 16-byte aligned");
            if (jobs.n == PACK_MAX_JOBS)
                if (int e = flush()) return e;
            PackJob &J = jobs.j[jobs.n++];
            J.w = w[i]; J.wt = (uint8_t *)dst; J.K = K[i]; J.cin_src = cin[i]; J.cout_src = cout[i]; J.transposed = dir;
            J.cin = dir ? cout[i] : cin_pad[i];
            J.cout = dir ? cin_pad[i] : cout[i];
            J.total = xv_packed_weights_bf16x3_bytes(J.K, J.cin, J.cout) / 32;     // one thread per 16-byte slot of each plane
            J.first_block = blocks;
            blocks += (unsigned)((J.total + 255) / 256);
        }
    }
    return flush();
}

size_t xv_split_row_bytes(int channels) { return channels <= 0 ? 0 : (size_t)((channels + 31) / 32) * SROW; }

int xv_split_encode_f32(const float *x, int64_t R, int c, int ldx, void *xs, void *stream)
{
    if (R <= 0) return 0;
    if (!x || !xs || c <= 0 || ldx < c) return fail(XV_ERR_BAD_ARG, "split_encode: bad argument");
    const int chunks = (c + 31) / 32;
    const size_t n = (size_t)R * chunks * 32;
    hipLaunchKernelGGL(split_encode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (long)R, c, ldx,
                       (uint8_t *)xs, chunks);
    return launch_status("split_encode_kernel");
}

int xv_split_decode_f32(const void *xs, int64_t R, int c, float *x, int ldx, void *stream)
{
    if (R <= 0) return 0;
    if (!x || !xs || c <= 0 || ldx < c) return fail(XV_ERR_BAD_ARG, "split_decode: bad argument");
    const size_t n = (size_t)R * c;
    hipLaunchKernelGGL(split_decode_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t *)xs, (long)R, c, (c + 31) / 32, x, ldx);
    return launch_status("split_decode_kernel");
}

int xv_tdnn_layer_bf16x3(const void *x, int x_format, int64_t R, int cin, int ldx, const void *wt, const float *bias,
                         const float *bn_scale, const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation,
                         int cout, const uint8_t *row_valid, void *y, int y_format, int ldy, float *y_preact, int ldpre,
                         void *stream)
{
    if (!x || !wt || (!y && !y_preact)) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3: NULL pointer");
    if (act_kind < XV_ACT_NONE || act_kind > XV_ACT_PRELU) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3: unknown act_kind");
    if ((x_format != XV_FMT_F32 && x_format != XV_FMT_SPLIT) || (y_format != XV_FMT_F32 && y_format != XV_FMT_SPLIT))
        return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3: unknown tensor format");
    Gemm3Params p{};
    p.x = x; p.x_split = x_format == XV_FMT_SPLIT; p.R = (long)R; p.cin = cin; p.ldx = ldx; p.wt = (const uint8_t *)wt;
    p.bias = bias; p.scale = bn_scale; p.shift = bn_shift; p.act = act_kind; p.alpha = act_alpha;
    p.K = K; p.dil = dilation; p.cout = cout; p.valid = row_valid;
    p.y = y; p.y_split = y_format == XV_FMT_SPLIT; p.ldy = ldy; p.ypre = y_preact; p.ldpre = ldpre;
    return launch_gemm3(p, (hipStream_t)stream);
}

int xv_tdnn_layer_bf16x3_sums(const void *x, int x_format, int64_t R, int cin, int ldx, const void *wt, const float *bias,
                              const float *bn_scale, const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation,
                              int cout, const uint8_t *row_valid, float *y, int ldy, const float *sum_r, int ld_sum_r, void *workspace,
                              void *stream)
{
    if (!x || !wt || !y || !sum_r || !workspace) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3_sums: NULL pointer");
    if (act_kind < XV_ACT_NONE || act_kind > XV_ACT_PRELU) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3_sums: unknown act_kind");
    if (x_format != XV_FMT_F32 && x_format != XV_FMT_SPLIT) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3_sums: unknown tensor format");
    if ((cout & 7) || (ldy & 3) || (ld_sum_r & 3) || ld_sum_r < cout || (((uintptr_t)sum_r) & 15) || (((uintptr_t)workspace) & 7))
        return fail(XV_ERR_UNSUPPORTED, "tdnn_bf16x3_sums: needs cout % 8 == 0, row strides % 4 == 0 and aligned pointers");
    Gemm3Params p{};
    p.x = x; p.x_split = x_format == XV_FMT_SPLIT; p.R = (long)R; p.cin = cin; p.ldx = ldx; p.wt = (const uint8_t *)wt;
    p.bias = bias; p.scale = bn_scale; p.shift = bn_shift; p.act = act_kind; p.alpha = act_alpha;
    p.K = K; p.dil = dilation; p.cout = cout; p.valid = row_valid;
    p.y = y; p.y_split = 0; p.ldy = ldy;
    p.cs_r = sum_r; p.cs_ldr = ld_sum_r; p.cs_part = (double *)workspace;
    return launch_gemm3(p, (hipStream_t)stream);
}

int xv_tdnn_layer_bf16x3_moments(const void *x, int x_format, int64_t R, int cin, int ldx, const void *wt, const float *bias,
                                 const float *bn_scale, const float *bn_shift, int act_kind, const float *act_alpha, int K, int dilation,
                                 int cout, const uint8_t *row_valid, float *y, int ldy, float *y_preact, int ldpre, void *workspace,
                                 void *stream)
{
    if (!x || !wt || !y || !workspace) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3_moments: NULL pointer");
    if (act_kind < XV_ACT_NONE || act_kind > XV_ACT_PRELU) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3_moments: unknown act_kind");
    if (x_format != XV_FMT_F32 && x_format != XV_FMT_SPLIT) return fail(XV_ERR_BAD_ARG, "tdnn_bf16x3_moments: unknown tensor format");
    if ((cout & 7) || (ldy & 3) || (((uintptr_t)workspace) & 7))
        return fail(XV_ERR_UNSUPPORTED, "tdnn_bf16x3_moments: needs cout % 8 == 0, ldy % 4 == 0 and an 8-byte aligned workspace");
    Gemm3Params p{};
    p.x = x; p.x_split = x_format == XV_FMT_SPLIT; p.R = (long)R; p.cin = cin; p.ldx = ldx; p.wt = (const uint8_t *)wt;
    p.bias = bias; p.scale = bn_scale; p.shift = bn_shift; p.act = act_kind; p.alpha = act_alpha;
    p.K = K; p.dil = dilation; p.cout = cout; p.valid = row_valid;
    p.y = y; p.y_split = 0; p.ldy = ldy; p.ypre = y_preact; p.ldpre = ldpre;
    p.cs_r = nullptr; p.cs_part = (double *)workspace;
    return launch_gemm3(p, (hipStream_t)stream);
}

int xv_tdnn_layer_pool_bf16x3(const void *x, int x_format, int64_t R, int cin, int ldx, const void *wt, const float *bias,
                              const float *bn_scale, const float *bn_shift, int act_kind, const float *act_alpha, int K,
                              int dilation, int cout, const uint8_t *row_valid, float *block_stats, void *stream)
{
    if (!x || !wt || !block_stats) return fail(XV_ERR_BAD_ARG, "tdnn_pool_bf16x3: NULL pointer");
    if (act_kind < XV_ACT_NONE || act_kind > XV_ACT_PRELU) return fail(XV_ERR_BAD_ARG, "tdnn_pool_bf16x3: unknown act_kind");
    if (x_format != XV_FMT_F32 && x_format != XV_FMT_SPLIT) return fail(XV_ERR_BAD_ARG, "tdnn_pool_bf16x3: unknown tensor format");
    if (((uintptr_t)block_stats) & 15) return fail(XV_ERR_BAD_ARG, "tdnn_pool_bf16x3: block_stats must be 16-byte aligned");
    Gemm3Params p{};
    p.x = x; p.x_split = x_format == XV_FMT_SPLIT; p.R = (long)R; p.cin = cin; p.ldx = ldx; p.wt = (const uint8_t *)wt;
    p.bias = bias; p.scale = bn_scale; p.shift = bn_shift; p.act = act_kind; p.alpha = act_alpha;
    p.K = K; p.dil = dilation; p.cout = cout; p.valid = row_valid;
    p.blk = block_stats;
    return launch_gemm3(p, (hipStream_t)stream);
}

int xv_fc_bf16x3(const float *x, int nrows, int in_dim, const void *wt, const float *bias, const float *bn_scale,
                 const float *bn_shift, int act_kind, const float *act_alpha, int out_dim, float *y, float *y_preact, void *stream)
{
    return xv_tdnn_layer_bf16x3(x, XV_FMT_F32, nrows, in_dim, in_dim, wt, bias, bn_scale, bn_shift, act_kind, act_alpha, 1, 1,
                                out_dim, nullptr, y, XV_FMT_F32, out_dim, y_preact, out_dim, stream);
}

}  // extern "C"
