// xv_sphere.hip -- NIST SPHERE audio decoded in front of the MFCC kernel: what `sph2pipe -f wav -p [-c N] x.sph |` does for an
// uncompressed file (G.711 mu-law / A-law expansion, or a byte swap of 16-bit PCM, and the choice of one channel), for many ragged
// utterances of any mix of codings per launch.  The raw data regions of the files are uploaded as they lie on disk; the host
// side (xvector_amd/sphere.py) reads the headers and builds the per-utterance descriptors and the tile list.  The formulas are
// restated in include/xvector_hip.h and DESIGN.md §8.12.
//
// One workgroup per tile of XV_DEC_TILE consecutive elements of `out`, cut at multiples of 8 elements (16 bytes of int16, 32 of
// fp32) of the output buffer rather than of the utterance: with h = OUT_OFF mod 8, tile (u, o0) makes the samples s with
// o0 <= s + h < o0 + XV_DEC_TILE.  Three phases:
//   1. the raw bytes the tile reads, from the 16-byte boundary at or below its first one, go to LDS: 16 bytes per lane from global
//      memory, one 16-byte LDS store each (the last chunk byte by byte where it would leave `raw`);
//   2. lane t decodes samples t, t + 256, ...: one or two byte reads from LDS (consecutive lanes read addresses STRIDE apart: no
//      bank conflict beyond the stride's own), the formula in registers, one 2- or 4-byte LDS store at the sample's place in the
//      tile -- consecutive lanes, consecutive elements;
//   3. lane t takes 16-byte groups t, t + 256, ... of the staged tile: a group that lies inside the utterance is one aligned
//      16-byte global store, the (at most two, at the utterance's ends) others are stored element by element, so nothing
//      outside [OUT_OFF, OUT_OFF + N) is written and the neighbour's samples in the same 16 bytes stay.
// The expansion is computed, not looked up: ~10 integer VALU operations per sample against 2 to 8 bytes moved, far below what the
// kernel's bandwidth leaves free, while a 256-entry table in LDS would have to be formed per workgroup and read at random banks.
// The coding is one per utterance, so its branch is uniform over the workgroup.  Static LDS only (33 KiB), no scratch.
#include "xv_device.h"

namespace {

constexpr int DT = 256;                     // threads per workgroup
constexpr int TILE = XV_DEC_TILE;           // output elements per workgroup
constexpr int RAW_CAP = TILE * 4 + 32;      // staged raw bytes: TILE frames of at most 4 bytes, the bytes below the first frame
                                            // (< 16) and the round-up of the last chunk (< 16)

__device__ __forceinline__ int ulaw_expand(int b)
{
    const int u = ~b & 0xff;
    const int t = (((u & 15) << 3) + 132) << ((u >> 4) & 7);
    return (u & 128) ? 132 - t : t - 132;
}

__device__ __forceinline__ int alaw_expand(int b)
{
    const int a = (b ^ 0x55) & 0xff;
    int t = (a & 15) << 4;
    const int s = (a >> 4) & 7;
    t += s ? 0x108 : 8;
    if (s > 1) t <<= s - 1;
    return (a & 128) ? t : -t;
}

// T: int16_t or float, the element of `out`
template <class T>
__global__ __launch_bounds__(DT) void wave_decode_kernel(const uint8_t *__restrict__ raw, int64_t raw_bytes,
                                                         const int64_t *__restrict__ utt, int n_utts,
                                                         const int64_t *__restrict__ tiles, T *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint8_t raws[RAW_CAP];
    __shared__ __attribute__((aligned(16))) T outs[TILE];
    constexpr int G = 16 / (int)sizeof(T);          // elements of a 16-byte group
    const int tid = threadIdx.x;
    const int64_t u = tiles[2 * blockIdx.x], o0 = tiles[2 * blockIdx.x + 1];
    if (u < 0 || u >= n_utts) return;
    const int64_t *d = utt + XV_DEC_FIELDS * u;
    const int64_t raw_off = d[XV_DEC_RAW_OFF], n = d[XV_DEC_N], out_off = d[XV_DEC_OUT_OFF];
    const int stride = (int)d[XV_DEC_STRIDE], ch_off = (int)d[XV_DEC_CH_OFF], coding = (int)d[XV_DEC_CODING];
    // what the host binding refuses; a workgroup that meets it anyway writes nothing
    if ((stride != 1 && stride != 2 && stride != 4) || coding < 0 || coding > 3 || ch_off < 0 || ch_off + (coding < 2 ? 2 : 1) > stride ||
        raw_off < 0 || n < 0 || out_off < 0 || n > (raw_bytes - raw_off) / stride || o0 < 0 || (o0 & 7))
        return;
    const int h = (int)(out_off & 7);
    const int64_t s_lo = max((int64_t)0, o0 - h), s_hi = min(n, o0 + TILE - h);
    if (s_lo >= s_hi) return;
    const int cnt = (int)(s_hi - s_lo);

    // phase 1
    const int64_t b_lo = raw_off + s_lo * stride, b_hi = raw_off + s_hi * stride;
    const int64_t a = b_lo & ~(int64_t)15;
    const int span = (int)(b_hi - a);                           // <= 15 + TILE * 4
    for (int e = 16 * tid; e < span; e += 16 * DT) {
        uint4 q;
        if (a + e + 16 <= raw_bytes) q = *(const uint4 *)(raw + a + e);
        else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (int i = 0; i < 16; ++i)
                if (a + e + i < raw_bytes) w[i >> 2] |= (uint32_t)raw[a + e + i] << (8 * (i & 3));
            q = uint4{w[0], w[1], w[2], w[3]};
        }
        *(uint4 *)(raws + e) = q;
    }
    __syncthreads();

    // phase 2: sample s_lo + i lies at byte p0 + i * stride of the staged span and at element e0 + i of the staged tile
    const int p0 = (int)(b_lo - a) + ch_off;
    const int e0 = (int)(s_lo + h - o0);
    for (int i = tid; i < cnt; i += DT) {
        const int p = p0 + i * stride;
        const int b0 = raws[p];
        int y;
        if (coding == XV_DEC_ULAW) y = ulaw_expand(b0);
        else if (coding == XV_DEC_ALAW) y = alaw_expand(b0);
        else {
            const int b1 = raws[p + 1];
            y = (int)(int16_t)(coding == XV_DEC_PCM16_LE ? (b0 | (b1 << 8)) : ((b0 << 8) | b1));
        }
        outs[e0 + i] = (T)y;
    }
    __syncthreads();

    // phase 3: out + base is 16-byte aligned (out is, and out_off - h + o0 is a multiple of 8 elements)
    T *dst = out + (out_off - h + o0);
    const int e1 = e0 + cnt;
    for (int g = tid; g < TILE / G; g += DT) {
        const int e = g * G;
        if (e + G <= e0 || e >= e1) continue;
        if (e >= e0 && e + G <= e1) *(uint4 *)(dst + e) = *(const uint4 *)(outs + e);
        else {
            for (int i = 0; i < G; ++i)
                if (e + i >= e0 && e + i < e1) dst[e + i] = outs[e + i];
        }
    }
}

}  // namespace

extern "C" int xv_wave_decode(const uint8_t *raw, int64_t raw_bytes, const int64_t *utt, int n_utts, const int64_t *tiles,
                              int64_t n_tiles, void *out, int sample_format, void *stream)
{
    if (n_utts < 0 || n_tiles < 0 || raw_bytes < 0 || (sample_format != 0 && sample_format != 1))
        return fail(XV_ERR_BAD_ARG, "wave_decode: bad argument");
    if (n_tiles == 0) return 0;
    if (!raw || !utt || !tiles || !out || n_utts == 0) return fail(XV_ERR_BAD_ARG, "wave_decode: bad argument");
    if ((uintptr_t)raw % 16 || (uintptr_t)out % 16) return fail(XV_ERR_BAD_ARG, "wave_decode: raw and out must be 16-byte aligned");
    if (n_tiles > 0x7fffffff) return fail(XV_ERR_UNSUPPORTED, "wave_decode: too many tiles for one launch");
    if (sample_format == 0)
        hipLaunchKernelGGL(wave_decode_kernel<int16_t>, dim3((unsigned)n_tiles), dim3(DT), 0, (hipStream_t)stream, raw, raw_bytes, utt,
                           n_utts, tiles, (int16_t *)out);
    else
        hipLaunchKernelGGL(wave_decode_kernel<float>, dim3((unsigned)n_tiles), dim3(DT), 0, (hipStream_t)stream, raw, raw_bytes, utt,
                           n_utts, tiles, (float *)out);
    return launch_status("wave_decode_kernel");
}
