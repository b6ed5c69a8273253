// The device primitives of the fp16-pair split kernels ("fp16x2": conv3x3s.hip has the scheme and its error budget), shared by
// conv3x3s.hip, conv3ds.hip, conv3dsw.hip, conv3dm.hip, conv3duw.hip, conv3dwm.hip and conv3dt.hip, and the z-segment choice of the two
// weight-gradient marchers.
#pragma once
#include "conv3x3_common.h"
#include <type_traits>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

// power-of-two scale exponent of a tensor whose max |.| is amax: |a| * 2^e < 2^15 (fp16 max 65504)
__device__ __forceinline__ int scale_exp(float amax) {
  const int be = (int)((__float_as_uint(amax) >> 23) & 0xffu) - 127;
  int e = (amax > 0.f) ? 14 - be : 0;
  e = e < -100 ? -100 : (e > 100 ? 100 : e);   // 2^e and 2^-e stay normal fp32 numbers
  return e;
}
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }

// The scaled fp16x2 split of a pair in 4 instructions, (x0, x1) * s -> leading fp16 pair h and residual pair r:
// v_fma_mix{lo,hi}_f16 multiply by the (power-of-two) scale, subtract the leading term read straight from its fp16 half,
// and round to fp16 once -- the same values as cvt(x*s), cvt(x*s - float(h)) (x*s and the difference are exact), without
// the 2 multiplies, 2 conversions back and 2 subtractions.  Every VALU instruction of the converting wave costs the
// computing wave matrix-pipe time.
__device__ __forceinline__ void split_pair_scaled(float x0, float x1, float s, unsigned& h, unsigned& r) {
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h) : "v"(x0), "v"(s));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h) : "v"(x1), "v"(s));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(r) : "v"(x0), "v"(s), "v"(h));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(r) : "v"(x1), "v"(s), "v"(h));
}
// 8 fp32 times the scale s -> two 16-B vectors of 8 halves
__device__ __forceinline__ void split8_scaled(const float* v, float s, u32x4& h, u32x4& r) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned hh, rr;
    split_pair_scaled(v[2 * q], v[2 * q + 1], s, hh, rr);
    h[q] = hh; r[q] = rr;
  }
}

// v_mfma_f32_32x32x16_f16 and v_mfma_f32_16x16x32_f16 on operands that travel as 16-B vectors of 8 halves
__device__ __forceinline__ f32x16 mfma32_f16(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16_f16(u32x4 a, u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// ds_read_b64_tr_b16, 16 lanes x 8 bytes: lane 4 j + q supplies the address of (voxel j, channel quad q); lane 4 q + c
// receives the c-th channel of quad q at voxels j = 0..3 (scripts/ubench/tr_read_probe.hip)
__device__ __forceinline__ uint2 tr_read(unsigned byte_addr) {
  return __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(uintptr_t)byte_addr));
}
__device__ __forceinline__ u32x4 tr_pair(unsigned a0, unsigned a1) {
  const uint2 u0 = tr_read(a0), u1 = tr_read(a1);
  return u32x4{u0.x, u0.y, u1.x, u1.y};
}

// compile-time loop: f(std::integral_constant<int, I>) for I = B .. E - 1 (the plane step's schedule is a table over its
// MFMA groups; `#pragma unroll` left some of these loops peeled instead of unrolled and the register arrays in scratch)
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}

// z segments of a weight-gradient marcher (conv3duw.hip, conv3dwm.hip): the split of D planes into nseg segments of zlen
// that costs the fewest plane steps -- rounds of ncu resident workgroups over cols columns x nseg, each zlen steps plus a
// prologue worth prologue_planes; the first minimum over 1 .. min(D, 64) pieces wins.  forced in 1 .. D overrides the choice.
struct ZSegments { int nseg, zlen; };
static inline ZSegments march_z_segments(int D, long long cols, int ncu, int prologue_planes, long long forced) {
  int best = 1;
  long long best_cost = -1;
  for (int s = 1; s <= D && s <= 64; ++s) {
    const int zl = (D + s - 1) / s;
    const int ns = (D + zl - 1) / zl;
    const long long rounds = (cols * ns + ncu - 1) / ncu;
    const long long cost = rounds * (zl + prologue_planes);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = ns; }
  }
  if (forced > 0 && forced <= D) best = (int)forced;
  ZSegments z;
  z.zlen = (D + best - 1) / best;
  z.nseg = (D + z.zlen - 1) / z.zlen;
  return z;
}
