// xv_device.h -- the preamble every translation unit of libxvector_hip.so shares (internal, not ABI): error reporting into
// xv_last_error(), the launch status, the per-device dynamic-LDS opt-in, vector types, the LDS-DMA macros and the compile-time
// helpers of the kernels.  Each unit includes it once; the helpers live in the unit's anonymous namespace like its own code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <type_traits>
#include <utility>

#include "xvector_hip.h"

extern "C" void xv_internal_set_error(const char *msg);      // xv_kernels.hip: the thread's xv_last_error() text

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// 16 bytes per lane global -> LDS (FLAT encoding): from gptr to lptr + imm + 16 * lane
#define XV_GLDS16_OFF(gptr, lptr, imm)                                                                          \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gptr),                    \
                                     (__attribute__((address_space(3))) void *)(lptr), 16, imm, 0)
#define XV_GLDS16(gptr, lptr) XV_GLDS16_OFF(gptr, lptr, 0)
// MUBUF form: 16 bytes per lane from buffer rsrc at voff (per lane) + soff (wave-uniform) + imm to LDS lptr + imm + 16 * lane
#define XV_BLDS16(rsrc, lptr, voff, soff, imm)                                                                  \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)(lptr), 16, voff, soff, imm, 0)
constexpr int XV_RSRC_FLAGS = 0x00020000;              // raw buffer, 32-bit data format (gfx9 family dword 3)

namespace {

// (K-1)*dilation limit of the GEMM families (xv_kernels.hip, xv_gemm3.hip, xv_gemm8*.hip): a tile's halo is at most 8 rows
constexpr int MAX_SPAN = 8;

int fail(int code, const char *msg)
{
    xv_internal_set_error(msg);
    return code;
}

int hip_fail(hipError_t e, const char *where)
{
    char buf[256];
    snprintf(buf, sizeof(buf), "%s: %s", where, hipGetErrorString(e));
    xv_internal_set_error(buf);
    return (int)e;
}

// the status of the launch just made: 0, or the error reported as "where: <hipGetErrorString>" (where NULL: the bare string)
int launch_status(const char *where = nullptr)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    return where ? hip_fail(e, where) : fail((int)e, hipGetErrorString(e));
}

// The dynamic-LDS opt-in of a call site's kernels, per device and idempotent: `done` (one static per call site) holds one bit per
// device id, set after the first pass in which every hipFuncSetAttribute succeeded, so a launch pays one atomic load.  `lds` is the
// byte count of every kernel in `kernels`, or a function giving the {kernel, bytes} of an element of `kernels` (a table).
template <class Kernels, class Lds>
int opt_in_dynamic_lds(std::atomic<unsigned long long> &done, const Kernels &kernels, Lds lds)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    if ((done.load(std::memory_order_acquire) >> (dev & 63)) & 1ull) return 0;
    for (const auto &k : kernels) {
        hipError_t e;
        if constexpr (std::is_integral_v<Lds>) e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        else e = hipFuncSetAttribute((const void *)lds(k).first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds(k).second);
        if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute");
    }
    done.fetch_or(1ull << (dev & 63), std::memory_order_release);
    return 0;
}

// f(integral_constant<int, I>) for I .. N-1, unrolled at compile time
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// The activation with its kind as a compile-time constant: the expressions of apply_act (xv_kernels.hip), hence the same bits, but
// no switch per element
template <int ACT>
__device__ __forceinline__ float act_t(float z, float a)
{
    if constexpr (ACT == XV_ACT_RELU) return fmaxf(z, 0.0f);
    else if constexpr (ACT == XV_ACT_LRELU) return z > 0.0f ? z : a * z;
    else if constexpr (ACT == XV_ACT_PRELU) return fmaxf(z, 0.0f) + a * fminf(z, 0.0f);
    else return z;
}

// The pair kernels' activation.  MODE 0: max(z,0) + alpha*min(z,0) (identity with alpha = 1, PReLU with per-channel alpha)
// 1: tf.nn.leaky_relu = max(alpha*z, z)   2: plain ReLU.  A compile-time choice: the epilogues are straight-line code.
template <int MODE>
__device__ __forceinline__ float act_fn(float z, float a)
{
    return MODE == 1 ? fmaxf(a * z, z) : MODE == 2 ? fmaxf(z, 0.f) : fmaxf(z, 0.f) + a * fminf(z, 0.f);
}

// Kaldi's SlidingWindowCmn window [ws, we) around frame t of an utterance of T frames (the rule is written out at the top of
// xv_frontend.hip).  Integers only.
__device__ __forceinline__ void cmn_window_bounds(int t, int T, int window, int center, int min_window, int &ws, int &we)
{
    if (center) { ws = t - window / 2; we = ws + window; }
    else { ws = t - window; we = t + 1; }
    if (ws < 0) { we -= ws; ws = 0; }
    if (!center && we > t) we = max(t + 1, min_window);
    if (we > T) { ws -= we - T; we = T; if (ws < 0) ws = 0; }
}

// The fp64 sum of col[s * ldx], ws <= s < we, moved right to the window [nws, nwe): the frames that leave are subtracted in
// ascending order, then the frames that enter are added in ascending order.  One order for every caller: the bits of the sum
// depend on the path of windows, never on which kernel walks it.
__device__ __forceinline__ void cmn_window_slide(const float *col, int ldx, int &ws, int &we, int nws, int nwe, double &sum)
{
    for (; ws < nws; ++ws) sum -= (double)col[(long)ws * ldx];
    for (; we < nwe; ++we) sum += (double)col[(long)we * ldx];
}

// cmn_window_slide for windows that follow an index list (voiced frames): the window moves right by the gap to the previous
// frame; one that has left the old window behind, or a list that does not ascend, starts its sum afresh.
__device__ __forceinline__ void cmn_window_move(const float *col, int ldx, int &ws, int &we, int nws, int nwe, double &sum)
{
    if (nws >= we || nws < ws || nwe < we) { sum = 0.0; ws = we = nws; }
    cmn_window_slide(col, ldx, ws, we, nws, nwe, sum);
}

}  // namespace
