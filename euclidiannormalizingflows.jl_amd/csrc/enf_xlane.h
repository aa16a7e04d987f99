// enf_xlane.h -- the cross-lane moves and sums of every kernel: DPP row moves, gfx950's permlane swaps (inline asm
// with a hand-placed hazard pad) and the group / class / tree sums built from them. The only place such code lives;
// tests/xlane/xlane.hip checks each sum against the __shfl_xor butterfly or the exact sum on the GPU
// (tests/test_gpu_round6.py::test_cross_lane_primitives).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "enf_internal.h"

namespace enf {

// A DPP move of every lane's value, the flow kernels' form. quad_perm(1,0,3,2) = 0xB1, quad_perm(2,3,0,1) = 0x4E,
// row_half_mirror = 0x141, row_mirror = 0x140. float: update_dpp (the form the headline kernel was tuned with);
// double: mov_dpp with bound_ctrl -- every lane of these patterns reads a lane of its own row, so no `old` value is
// needed and none is materialised (update_dpp(0, ...) cost two v_mov of zero per stage; round 4).
template <int CTRL, typename T>
__device__ __forceinline__ T dpp(T x) {
  if constexpr (std::is_same_v<T, float>) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, false));
  } else {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
  }
}
// Cross-lane moves without an LDS round trip (ds_bpermute, the __shfl_xor form, costs a round trip per stage on the
// chains of the one-block steps). dpp_mov<CTRL>: a DPP row move (quad_perm / row_ror) of every lane's value.
template <int CTRL, typename T>
__device__ __forceinline__ T dpp_mov(T x) {
  if constexpr (sizeof(T) == 4) {
    return __builtin_bit_cast(T, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
  } else {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const int lo = __builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(T, ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
  }
}
// x + (the value of lane ^ M), M = 16 or 32, by gfx950's v_permlane16_swap / v_permlane32_swap (VALU): with both
// operands x the swap leaves x and its partner side by side, and their sum is x + __shfl_xor(x, M) bit for bit
// (the two addends are the same, and addition commutes)
template <int M, typename T>
__device__ __forceinline__ T add_xor_swap(T x) {
  static_assert(M == 16 || M == 32, "the permlane swaps pair lanes 16 or 32 apart");
#if defined(__gfx950__)
  // The instruction itself, not the builtin: hipcc 7.2 reads the builtin's second result from the first result's
  // register for a 32-bit value in this use (the swapped half added to itself: the round-5 run-27 failure, DESIGN
  // §4). Hazard (gfx950): a v_permlane16/32_swap that reads a VGPR written by a VALU instruction needs two wait
  // states after that write -- the compiler's own hazard recognizer pads its builtin with the same `s_nop 1`, but
  // it cannot see into this asm, so the pad is written here. tests/test_gpu_round6.py::test_cross_lane_primitives
  // checks every group size against the __shfl_xor butterfly bit for bit on the GPU (tests/xlane/).
  struct Pair {
    uint32_t a, b;
  };
  auto sw = [](uint32_t u) {
    Pair p{u, u};
    if constexpr (M == 32) asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(p.a), "+v"(p.b));
    else asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(p.a), "+v"(p.b));
    return p;
  };
  if constexpr (sizeof(T) == 4) {
    const Pair r = sw(__builtin_bit_cast(uint32_t, x));
    return __builtin_bit_cast(T, r.a) + __builtin_bit_cast(T, r.b);
  } else {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const Pair lo = sw((uint32_t)u), hi = sw((uint32_t)(u >> 32));
    return __builtin_bit_cast(T, ((uint64_t)hi.a << 32) | lo.a) + __builtin_bit_cast(T, ((uint64_t)hi.b << 32) | lo.b);
  }
#else
  // (other targets -- and the host pass -- have no permlane swaps: the shuffle, bit-identical)
  return x + __shfl_xor(x, M);
#endif
}

// Sum over aligned groups of G lanes (G <= 64, power of two); every lane of the group gets it. All 64 lanes must be
// active. After the quad steps every lane of a quad holds the quad sum, so a mirror partner always lies in the other
// quad / half-row. Strides 16 and 32 are __shfl_xor in the flow kernels; SWAP (the generic gradient kernel): the
// permlane swaps, the same two addends.
template <int G, bool SWAP = false, typename T>
__device__ __forceinline__ T group_sum(T x) {
  if constexpr (G >= 2) x += dpp<0xB1>(x);
  if constexpr (G >= 4) x += dpp<0x4E>(x);
  if constexpr (G >= 8) x += dpp<0x141>(x);
  if constexpr (G >= 16) x += dpp<0x140>(x);
  if constexpr (SWAP) {
    if constexpr (G >= 32) x = add_xor_swap<16>(x);
    if constexpr (G >= 64) x = add_xor_swap<32>(x);
  } else {
    if constexpr (G >= 32) x += __shfl_xor(x, 16);
    if constexpr (G >= 64) x += __shfl_xor(x, 32);
  }
  return x;
}

// DPP max over aligned groups of G lanes (as group_sum)
template <int G>
__device__ __forceinline__ float group_max(float x) {
  if constexpr (G >= 2) x = fmaxf(x, dpp<0xB1>(x));
  if constexpr (G >= 4) x = fmaxf(x, dpp<0x4E>(x));
  if constexpr (G >= 8) x = fmaxf(x, dpp<0x141>(x));
  if constexpr (G >= 16) x = fmaxf(x, dpp<0x140>(x));
  if constexpr (G >= 32) x = fmaxf(x, __shfl_xor(x, 16));
  if constexpr (G >= 64) x = fmaxf(x, __shfl_xor(x, 32));
  return x;
}

// Sum over the lanes of a class -- the lanes with equal lane % G (G <= 64, power of two), which hold the same rows of
// different columns -- valid in lanes < G: strides G, 2G, ... < 64. Within a 16-lane row the stages are DPP moves
// (quad_perm xor 1 / xor 2, row_ror 4 / 8: shifts by a multiple of the class size keep lanes in their class), the two
// cross-row stages permlane swaps.
template <int G, typename T>
__device__ __forceinline__ T class_sum(T v) {
  if constexpr (G < 2) v += dpp_mov<0xB1>(v);   // quad_perm(1,0,3,2): lane ^ 1
  if constexpr (G < 4) v += dpp_mov<0x4E>(v);   // quad_perm(2,3,0,1): lane ^ 2
  if constexpr (G < 8) v += dpp_mov<0x124>(v);  // row_ror:4
  if constexpr (G < 16) v += dpp_mov<0x128>(v); // row_ror:8
  if constexpr (G < 32) v = add_xor_swap<16>(v);
  if constexpr (G < 64) v = add_xor_swap<32>(v);
  return v;
}

// The xor butterfly over the lanes of a group of P (power of two, <= 64) consecutive lanes, strides P/2 .. 1 in that
// order: exactly `for (m = P / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m)`. Strides 32 and 16 are permlane swaps,
// 8 is row_ror:8 (lane (l + 8) mod 16 of the row is l ^ 8), 4 is row_ror:4 once stride 8 has made every value equal
// to its lane ^ 8 partner's (then (l + 4) mod 16 holds l ^ 4's value), 2 and 1 quad_perm; a stride-4 first stage
// (P = 8) keeps the shuffle.
template <typename T>
__device__ __forceinline__ T xor_tree(T v, int P) {
  if (P >= 64) v = add_xor_swap<32>(v);
  if (P >= 32) v = add_xor_swap<16>(v);
  if (P >= 16) v += dpp_mov<0x128>(v);  // row_ror:8
  if (P >= 16) v += dpp_mov<0x124>(v);  // row_ror:4
  else if (P >= 8) v += __shfl_xor(v, 4);
  if (P >= 4) v += dpp_mov<0x4E>(v);    // quad_perm(2,3,0,1): lane ^ 2
  if (P >= 2) v += dpp_mov<0xB1>(v);    // quad_perm(1,0,3,2): lane ^ 1
  return v;
}

// The sum over a wave's lanes of values held as d = lane, lane + 64, ... < D (lanes >= D hold zeros): the xor
// tree from half the smallest power of two >= min(D, 64) down; the strides it leaves out would only add zeros, so
// the value is that of the full 64-lane tree (round 5: 1 stage instead of 6 at D = 2). Every lane < D gets it.
__device__ __forceinline__ double lane_sum(double v, int64_t D) {
  return xor_tree(v, D < 64 ? next_pow2<int>(D) : 64);
}

}  // namespace enf
