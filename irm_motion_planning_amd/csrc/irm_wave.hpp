// irm_wave.hpp — wave-level device helpers of the gfx950 kernels: the packed-fp32 types, the DPP wave
// reductions (sum, max, min, argmax with first-index ties) and the store of a 16x16 MFMA result tile.
// Included by irm_physics.hpp, irm_opt_common.hpp, irm_kernels_impl.hpp, irm_dense.hip, irm_clearance.hip and
// irm_self_clearance.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "irm_kernels.hpp"

namespace irm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// The kernels are compiled with -ffp-contract=off (build.py): every fused multiply-add is written
// as one, so the arithmetic does not depend on the compiler's contraction choices.
__device__ __forceinline__ f32x2 pkfma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// ------------------------------------------------------------ wave helpers
// DPP row reductions (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
// row_mirror) leave each 16-lane row reduced in all its lanes; the four
// rows are then combined from v_readlane (uniform result, no LDS).
// Every control used here is an in-row permutation (no lane reads outside its row), so the old value
// is never kept: mov_dpp (old undefined, bound_ctrl) lets the compiler fold the move into the consuming
// VALU op as a DPP source (v_add_f32_dpp …) instead of v_mov_b32 + v_mov_b32_dpp + the op.
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
    static_assert(CTRL == 0xB1 || CTRL == 0x4E || CTRL == 0x141 || CTRL == 0x140, "in-row permutations only");
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dppi(int v) {
    static_assert(CTRL == 0xB1 || CTRL == 0x4E || CTRL == 0x141 || CTRL == 0x140, "in-row permutations only");
    return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, true);
}
// s + (row_bcast:15 of s) in rows 1 and 3 (ROW = 15), s + (row_bcast:31 of s) in rows 2 and 3 (ROW = 31);
// the other rows keep s.  As one v_add_f32_dpp (the compiler's DPP combine leaves the float add with a
// partial row mask as a v_mov_b32_dpp + v_add_f32 pair); s_nop 1: the VALU-write → DPP-read hazard.
template <int ROW>
__device__ __forceinline__ float bcast_add(float s) {
    static_assert(ROW == 15 || ROW == 31, "row broadcasts");
    if constexpr (ROW == 15)
        asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : "+v"(s));
    else
        asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" : "+v"(s));
    return s;
}
// max of floats that are ≥ +0 or −inf, on their bit patterns (signed-int order = float order there):
// no NaN canonicalisation, and the DPP move folds into v_max_i32_dpp
__device__ __forceinline__ float maxpos(float a, float b) {
    return __int_as_float(max(__float_as_int(a), __float_as_int(b)));
}
__device__ __forceinline__ float lanef(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ float wred_sum(float v) {
    v += dppf<0xB1>(v);
    v += dppf<0x4E>(v);
    v += dppf<0x141>(v);
    v += dppf<0x140>(v);
    return (lanef(v, 0) + lanef(v, 16)) + (lanef(v, 32) + lanef(v, 48));
}
__device__ __forceinline__ float wred_max(float v) {
    v = fmaxf(v, dppf<0xB1>(v));
    v = fmaxf(v, dppf<0x4E>(v));
    v = fmaxf(v, dppf<0x141>(v));
    v = fmaxf(v, dppf<0x140>(v));
    return fmaxf(fmaxf(lanef(v, 0), lanef(v, 16)), fmaxf(lanef(v, 32), lanef(v, 48)));
}
__device__ __forceinline__ float wred_min(float v) {
    v = fminf(v, dppf<0xB1>(v));
    v = fminf(v, dppf<0x4E>(v));
    v = fminf(v, dppf<0x141>(v));
    v = fminf(v, dppf<0x140>(v));
    return fminf(fminf(lanef(v, 0), lanef(v, 16)), fminf(lanef(v, 32), lanef(v, 48)));
}
// max with first-index tie break (jnp.argmax, trajectory.py:97)
__device__ __forceinline__ void amax_step(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}
template <int CTRL>
__device__ __forceinline__ void amax_dpp(float& v, int& i) {
    float ov = dppf<CTRL>(v);
    int oi = dppi<CTRL>(i);
    amax_step(v, i, ov, oi);
}
__device__ __forceinline__ void wred_argmax(float& v, int& i) {
    amax_dpp<0xB1>(v, i);
    amax_dpp<0x4E>(v, i);
    amax_dpp<0x141>(v, i);
    amax_dpp<0x140>(v, i);
    float bv = lanef(v, 0);
    int bi = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
    for (int r = 16; r < 64; r += 16) amax_step(bv, bi, lanef(v, r), __builtin_amdgcn_readlane(i, r));
    v = bv;
    i = bi;
}

// ---------------------------------------------------------- MFMA contraction
// D layout of 16x16x4: lane l holds rows 4*(l>>4)+i, column l&15.
// Callers keep every tile inside the buffer (row extents are multiples of 16).
__device__ __forceinline__ void store_tile(float* out, int tile, f32x4 acc, unsigned colmask) {
    const int lane = threadIdx.x & 63;
    const int col = lane & 15;
    if (!((colmask >> col) & 1u)) return;
    float* o = out + (tile * 16 + 4 * (lane >> 4)) * kLd + col;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i * kLd] = acc[i];
}

}  // namespace irm
