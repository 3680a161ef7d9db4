// xv_compress.hip -- feature matrices as Kaldi CompressedMatrix payloads, encoded on the MI355X.
//
// What copy-feats --compress=true / compute-mfcc-feats --compress=true do on the host with CompressedMatrix::CopyFromMat
// (kAutomaticMethod), restated from the published algorithm; include/xvector_hip.h holds the arithmetic as the contract:
//   "CM2 " (rows <= 8)  one uint16 per element on the global [min, min + range] scale, row-major;
//   "CM "  (rows  > 8)  per column four uint16 percentiles (0, 25, 75, 100) on that scale, then one byte per element on the
//                       column's 3-segment piecewise-linear scale, column-major.
// Three launches per call, each reading what the one before left in the payload itself (no scratch memory):
//   cm_range_kernel     one workgroup per utterance: min / max over order-preserving integer keys (so the result has no
//                       reduction order, and of a zero extreme the sign is fixed: -0.0 for the minimum, +0.0 for the maximum),
//                       the non-finite flag, the 16-byte header;
//   cm_column_kernel    one workgroup per (utterance, column): the order statistics s[0], s[T/4], s[3(T/4)], s[T-1] exactly,
//                       by an MSB-first radix select (8 bits a pass, both inner ranks in the same passes) over the column's
//                       keys, staged in LDS up to CM_STAGE_MAX rows and re-read from global memory beyond;
//   cm_quantise_kernel  tiles of CM_TILE rows: rows are read coalesced, quantised, transposed through LDS as bytes and stored
//                       column-major as whole dwords where a dword lies inside the tile's run of the column, byte by byte
//                       at its unaligned head and tail (two workgroups never write the same dword).
// Exactness: every fp32 expression below is evaluated as written -- this unit is compiled with `#pragma clang fp contract(off)`
// (no fused multiply-add is formed), hipcc's correctly rounded fp32 division, and the default kernel mode that keeps subnormals.
// All stores are ordinary vector stores from plain C++.
#include "xv_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int CM_NT = 256;                   // threads of the column and quantise kernels
constexpr int CM_RANGE_NT = 1024;            // threads of the range kernel
constexpr int CM_STAGE_MAX = 8192;           // rows of a column staged in LDS (32 KiB of keys)
constexpr int CM_TILE = 256;                 // rows per quantise tile
constexpr int CM_MAX_COLS = 128;
constexpr int CM_SLOTS = CM_TILE / 4 + 1;    // dwords a tile's run of one column can touch
constexpr int CM_TILE_LD = CM_TILE + 4;      // bytes between two columns of the LDS tile: 65 dwords, so the columns of one row
                                             // (written by neighbouring lanes) fall into different banks

__device__ __forceinline__ uint32_t cm_key(float v)
{
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float cm_value(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// (int)trunc(d) where that is defined; INT_MIN for a NaN, an infinity or a value outside int, which is what the x86 conversion
// of the host encoders gives (a zero-width segment divides by zero; the clamps that follow keep the byte in its segment)
__device__ __forceinline__ int cm_int(double d) { return fabs(d) < 2147483648.0 ? (int)trunc(d) : (int)0x80000000; }

__device__ __forceinline__ int cm_u16(float v, float gmin, float grange)
{
    float f = (v - gmin) / grange;
    f = fminf(fmaxf(f, 0.0f), 1.0f);
    const float s = f * 65535.0f;
    return cm_int((double)s + 0.499);
}

__device__ __forceinline__ float cm_f16(int q, float gmin, float grange)
{
    const float step = grange * 1.52590218966964e-05f;
    const float d = step * (float)q;
    return gmin + d;
}

__device__ __forceinline__ int cm_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ int cm_byte(float v, float p0, float p25, float p75, float p100)
{
    if (v < p25) {
        const float f = ((v - p0) / (p25 - p0)) * 64.0f;
        return cm_clamp(cm_int((double)f + 0.5), 0, 64);
    }
    if (v < p75) {
        const float f = ((v - p25) / (p75 - p25)) * 128.0f;
        return cm_clamp(64 + cm_int((double)f + 0.5), 64, 192);
    }
    const float f = ((v - p75) / (p100 - p75)) * 63.0f;
    return cm_clamp(192 + cm_int((double)f + 0.5), 192, 255);
}

// ---------------------------------------------------------------------------------------------------------------------------
// pass 1: range, status, header
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CM_RANGE_NT) void cm_range_kernel(const float *__restrict__ feats, int64_t ld,
                                                               const int64_t *__restrict__ row0, const int32_t *__restrict__ n_frames,
                                                               int C, const int64_t *__restrict__ out_offset, uint8_t *__restrict__ out,
                                                               int32_t *__restrict__ status)
{
    __shared__ uint32_t s_min[CM_RANGE_NT / 64], s_max[CM_RANGE_NT / 64], s_bad[CM_RANGE_NT / 64];
    const int u = blockIdx.x;
    const int T = n_frames[u];
    if (T <= 0) {
        if (threadIdx.x == 0) status[u] = 0;
        return;
    }
    if ((int64_t)T * C > 0x7fffffff) {                    // the frame counts live on the device: refused here, per utterance
        if (threadIdx.x == 0) status[u] = 2;
        return;
    }
    const float *x = feats + row0[u] * ld;
    const int n = T * C;
    uint32_t kmin = 0xffffffffu, kmax = 0u, bad = 0u;
    for (int e = threadIdx.x; e < n; e += CM_RANGE_NT) {
        const int t = e / C, c = e - t * C;
        const float v = x[(int64_t)t * ld + c];
        const uint32_t k = cm_key(v);
        kmin = min(kmin, k);
        kmax = max(kmax, k);
        bad |= ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o, 64));
        kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
        bad |= (uint32_t)__shfl_xor((int)bad, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_min[wave] = kmin;
        s_max[wave] = kmax;
        s_bad[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < CM_RANGE_NT / 64; ++w) {
            kmin = min(kmin, s_min[w]);
            kmax = max(kmax, s_max[w]);
            bad |= s_bad[w];
        }
        const float gmin = cm_value(kmin);
        float gmax = cm_value(kmax);
        if (gmax == gmin) gmax = (float)((double)gmin + (1.0 + fabs((double)gmin)));
        const float grange = gmax - gmin;
        uint4 h;
        h.x = __float_as_uint(gmin);
        h.y = __float_as_uint(grange);
        h.z = (uint32_t)T;
        h.w = (uint32_t)C;
        *reinterpret_cast<uint4 *>(out + out_offset[u]) = h;
        status[u] = (bad || !(fabs(grange) < __builtin_huge_valf())) ? 1 : 0;      // finite values whose range overflows: refused too
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// pass 2: the four order statistics of a column
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CM_NT) void cm_column_kernel(const float *__restrict__ feats, int64_t ld, const int64_t *__restrict__ row0,
                                                          const int32_t *__restrict__ n_frames, int C,
                                                          const int64_t *__restrict__ out_offset, uint8_t *__restrict__ out,
                                                          const int32_t *__restrict__ status)
{
    __shared__ uint32_t stage[CM_STAGE_MAX];
    __shared__ uint32_t hist[2][256];
    __shared__ uint32_t s_prefix[2], s_rank[2], s_ext[2];
    const int u = blockIdx.x / C, c = blockIdx.x - u * C;
    const int T = n_frames[u];
    if (T <= 8 || status[u] != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *col = feats + row0[u] * ld + c;
    const bool staged = T <= CM_STAGE_MAX;
    const int q = T / 4;

    if (tid == 0) {
        s_prefix[0] = s_prefix[1] = 0u;
        s_rank[0] = (uint32_t)q;
        s_rank[1] = (uint32_t)(3 * q);
        s_ext[0] = 0xffffffffu;
        s_ext[1] = 0u;
    }
    __syncthreads();
    {   // the column's keys into LDS (where they fit) and its extremes
        uint32_t kmin = 0xffffffffu, kmax = 0u;
        for (int t = tid; t < T; t += CM_NT) {
            const uint32_t k = cm_key(col[(int64_t)t * ld]);
            if (staged) stage[t] = k;
            kmin = min(kmin, k);
            kmax = max(kmax, k);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o, 64));
            kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
        }
        if (lane == 0) {
            atomicMin(&s_ext[0], kmin);
            atomicMax(&s_ext[1], kmax);
        }
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        hist[0][tid] = 0u;
        hist[1][tid] = 0u;
        __syncthreads();                                  // also: stage, s_prefix, s_rank of the pass before are visible
        const uint32_t pa = s_prefix[0], pb = s_prefix[1];
        for (int t = tid; t < T; t += CM_NT) {
            const uint32_t k = staged ? stage[t] : cm_key(col[(int64_t)t * ld]);
            const uint32_t hi = pass == 0 ? 0u : k >> (shift + 8);
            const uint32_t digit = (k >> shift) & 255u;
            if (hi == pa) atomicAdd(&hist[0][digit], 1u);
            if (hi == pb) atomicAdd(&hist[1][digit], 1u);
        }
        __syncthreads();
        if (wave < 2) {                                   // wave r finds the bin of rank r: lane l owns bins 4l .. 4l + 3
            const uint32_t rank = s_rank[wave];
            uint32_t cnt[4], sum = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                cnt[j] = hist[wave][4 * lane + j];
                sum += cnt[j];
            }
            uint32_t incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
                if (lane >= o) incl += up;
            }
            uint32_t below = incl - sum;
            if (below <= rank && rank < incl) {           // exactly one lane: the counts of the live prefix sum to > rank
                int bin = 0;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (bin == j && rank >= below + cnt[j]) {
                        below += cnt[j];
                        bin = j + 1;
                    }
                }
                s_prefix[wave] = (s_prefix[wave] << 8) | (uint32_t)(4 * lane + bin);
                s_rank[wave] = rank - below;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        uint8_t *pay = out + out_offset[u];
        const uint4 h = *reinterpret_cast<const uint4 *>(pay);
        const float gmin = __uint_as_float(h.x), grange = __uint_as_float(h.y);
        int p0 = cm_u16(cm_value(s_ext[0]), gmin, grange);
        int p25 = cm_u16(cm_value(s_prefix[0]), gmin, grange);
        int p75 = cm_u16(cm_value(s_prefix[1]), gmin, grange);
        int p100 = cm_u16(cm_value(s_ext[1]), gmin, grange);
        p0 = min(p0, 65532);
        p25 = min(max(p25, p0 + 1), 65533);
        p75 = min(max(p75, p25 + 1), 65534);
        p100 = max(p100, p75 + 1);
        uint2 w;
        w.x = (uint32_t)p0 | ((uint32_t)p25 << 16);
        w.y = (uint32_t)p75 | ((uint32_t)p100 << 16);
        *reinterpret_cast<uint2 *>(pay + 16 + 8 * c) = w;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// pass 3: the elements
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CM_NT) void cm_quantise_kernel(const float *__restrict__ feats, int64_t ld, const int64_t *__restrict__ row0,
                                                            const int32_t *__restrict__ n_frames, int C,
                                                            const int64_t *__restrict__ out_offset, uint8_t *__restrict__ out,
                                                            const int32_t *__restrict__ status)
{
    __shared__ float pct[CM_MAX_COLS][4];
    __shared__ __attribute__((aligned(4))) uint8_t tile[CM_MAX_COLS * CM_TILE_LD];
    const int u = blockIdx.y;
    const int T = n_frames[u];
    if (T <= 0 || status[u] != 0) return;
    const int tid = threadIdx.x;
    const float *x = feats + row0[u] * ld;
    uint8_t *pay = out + out_offset[u];
    const uint4 h = *reinterpret_cast<const uint4 *>(pay);
    const float gmin = __uint_as_float(h.x), grange = __uint_as_float(h.y);

    if (T <= 8) {                                         // "CM2 ": row-major uint16
        if (blockIdx.x != 0) return;
        uint16_t *dst = reinterpret_cast<uint16_t *>(pay + 16);
        for (int e = tid; e < T * C; e += CM_NT) {
            const int t = e / C, c = e - t * C;
            dst[e] = (uint16_t)cm_u16(x[(int64_t)t * ld + c], gmin, grange);
        }
        return;
    }
    const int n_tiles = (T + CM_TILE - 1) / CM_TILE;
    if ((int)blockIdx.x >= n_tiles) return;
    for (int c = tid; c < C; c += CM_NT) {
        const uint2 w = *reinterpret_cast<const uint2 *>(pay + 16 + 8 * c);
        pct[c][0] = cm_f16((int)(w.x & 0xffffu), gmin, grange);
        pct[c][1] = cm_f16((int)(w.x >> 16), gmin, grange);
        pct[c][2] = cm_f16((int)(w.y & 0xffffu), gmin, grange);
        pct[c][3] = cm_f16((int)(w.y >> 16), gmin, grange);
    }
    uint8_t *body = pay + 16 + 8 * (int64_t)C;
    for (int tl = blockIdx.x; tl < n_tiles; tl += gridDim.x) {
        const int t0 = tl * CM_TILE;
        const int n = min(CM_TILE, T - t0);
        __syncthreads();                                  // pct is written; the tile before is stored
        for (int e = tid; e < n * C; e += CM_NT) {
            const int t = e / C, c = e - t * C;
            const float v = x[(int64_t)(t0 + t) * ld + c];
            tile[c * CM_TILE_LD + t] = (uint8_t)cm_byte(v, pct[c][0], pct[c][1], pct[c][2], pct[c][3]);
        }
        __syncthreads();
        // column c's run of the tile is payload bytes [a, a + n): slot j is the aligned dword j of [a & ~3, ...)
        for (int i = tid; i < C * CM_SLOTS; i += CM_NT) {
            const int c = i / CM_SLOTS, j = i - c * CM_SLOTS;
            const int64_t a = (int64_t)c * T + t0;        // byte offset in body; body itself is 8-byte aligned
            const int lead = (int)(a & 3);
            const int b0 = 4 * j - lead;                  // tile-local index of the dword's first byte
            if (b0 >= n) continue;
            const uint8_t *src = tile + c * CM_TILE_LD;
            uint8_t *dst = body + a + b0;
            if (b0 >= 0 && b0 + 4 <= n) {
                const uint32_t w = (uint32_t)src[b0] | ((uint32_t)src[b0 + 1] << 8) | ((uint32_t)src[b0 + 2] << 16) |
                                   ((uint32_t)src[b0 + 3] << 24);
                *reinterpret_cast<uint32_t *>(dst) = w;
            } else {
                for (int k = 0; k < 4; ++k)
                    if (b0 + k >= 0 && b0 + k < n) dst[k] = src[b0 + k];
            }
        }
    }
}

}  // namespace

extern "C" int64_t xv_cm_payload_bytes(int rows, int cols)
{
    if (rows <= 0 || cols < 0) return 0;
    return 16 + (rows > 8 ? 8 * (int64_t)cols + (int64_t)rows * cols : 2 * (int64_t)rows * cols);
}

extern "C" int xv_cm_encode_f32(const float *feats, int64_t ld, const int64_t *utt_row0, const int32_t *n_frames, int n_utts,
                                int n_cols, const int64_t *out_offset, uint8_t *out, int32_t *status, void *stream)
{
    if (n_utts == 0) return 0;
    if (n_cols < 1 || n_cols > CM_MAX_COLS) return fail(XV_ERR_UNSUPPORTED, "cm_encode: n_cols must be in [1, 128]");
    if (n_utts < 0 || !feats || ld < n_cols || !utt_row0 || !n_frames || !out_offset || !out || !status ||
        ((uintptr_t)out & 15) != 0)
        return fail(XV_ERR_BAD_ARG, "cm_encode: bad argument");
    if ((int64_t)n_utts * n_cols > 0x7fffffff) return fail(XV_ERR_UNSUPPORTED, "cm_encode: too many utterances for one launch");
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cm_range_kernel, dim3(n_utts), dim3(CM_RANGE_NT), 0, s, feats, ld, utt_row0, n_frames, n_cols, out_offset, out,
                       status);
    if (const int rc = launch_status("cm_range_kernel")) return rc;
    hipLaunchKernelGGL(cm_column_kernel, dim3((unsigned)(n_utts * n_cols)), dim3(CM_NT), 0, s, feats, ld, utt_row0, n_frames, n_cols,
                       out_offset, out, status);
    if (const int rc = launch_status("cm_column_kernel")) return rc;
    // the frame counts live on the device: a few workgroups per utterance walk its tiles (more of them when the batch is small)
    const int per_utt = n_utts >= 1024 ? 1 : (1024 / n_utts > 64 ? 64 : 1024 / n_utts);
    for (int u0 = 0; u0 < n_utts; u0 += 65535) {
        const int nu = n_utts - u0 < 65535 ? n_utts - u0 : 65535;
        hipLaunchKernelGGL(cm_quantise_kernel, dim3(per_utt, nu), dim3(CM_NT), 0, s, feats, ld, utt_row0 + u0, n_frames + u0, n_cols,
                           out_offset + u0, out, status + u0);
        if (const int rc = launch_status("cm_quantise_kernel")) return rc;
    }
    return 0;
}
