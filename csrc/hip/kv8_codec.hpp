// The fp8 KV-cache codec on the device (the _kv8 kernels of decode_kernels.hip
// and prefill_kernels.hip; pbs_amd.ops.llm.kv8_quant_ref is its definition).
//
// One scale per cached row and KV head, a power of two: for a row x[128] of
// finite bf16 values with amax = max |x| = m 2^ex, m in [0.5, 1),
//   e = ex - 9 if m <= 0.875 else ex - 8, clamped to e >= -100 (e = 0 if amax == 0),
//   scale = 2^e (fp32), code = e4m3fn(x 2^-e), round to nearest even.
// amax / scale lies in (224, 448], so nothing saturates; x 2^-e is exact in
// fp32, and float(code) * scale is exact and representable in bf16, so the
// dequantised value has one definition and no rounding of its own.
#pragma once
#include "common.hpp"

namespace gpbs_hip {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// 8 codes and their row's scale -> the 16 bytes the bf16 cache holds for them:
// one scaled conversion per pair of codes.  The scale is a power of two and
// every product is a bf16 value, so the instruction has nothing to round.
__device__ __forceinline__ u32x4 kv8_dequant8(u32x2 c, float sc) {
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bf16x2 p = (e & 1) ? __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[e >> 1], sc, true)
                             : __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c[e >> 1], sc, false);
    o[e] = __builtin_bit_cast(u32, p);
  }
  return o;
}

// kv8_dequant8 for a kernel that goes on in shared text written for words loaded
// from a bf16 cache: each word is made opaque, so the compiler meets the same
// unpack, multiply and add expressions over the same kind of operand as in the
// bf16 compilation and takes the same fused multiply-add decisions for them
// (a product folded into the unpack would be free to contract differently).
__device__ __forceinline__ u32x4 kv8_words(u32x2 c, float sc) {
  u32x4 o = kv8_dequant8(c, sc);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    u32 w = o[e];
    asm("" : "+v"(w));
    o[e] = w;
  }
  return o;
}

// Quantise one row held by 16 lanes, 8 bf16 values (4 words) each: returns the
// lane's 8 codes and the row's scale.  The 16 lanes must be consecutive, start
// at a multiple of 16 within the wave and call this together: the amax exchange
// uses xor 8, 4, 2, 1, which never leaves such a group.
__device__ __forceinline__ u32x2 kv8_quant8(u32x4 v, float* scale) {
  u32 a = 0;  // |x| as bf16 bits: for finite values their order is the order of the magnitudes
#pragma unroll
  for (int e = 0; e < 4; ++e) a = max(a, max(v[e] & 0x7fffu, (v[e] >> 16) & 0x7fffu));
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) a = max(a, (u32)__shfl_xor((int)a, o, 64));
  // frexp on the bits: amax = (1 + mant / 128) 2^(E - 127), so ex = E - 126 and m <= 0.875 iff mant <= 96
  const int E = (int)(a >> 7), mant = (int)(a & 127u);
  const int ex = a ? max(E - 126 - (mant <= 96 ? 9 : 8), -100) : 0;
  *scale = __uint_as_float((u32)(127 + ex) << 23);
  const float inv = __uint_as_float((u32)(127 - ex) << 23);
  u32x2 c;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const u32 w0 = v[2 * h], w1 = v[2 * h + 1];
    const int p = __builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(w0 << 16) * inv,
                                                  __uint_as_float(w0 & 0xffff0000u) * inv, 0, false);
    c[h] = (u32)__builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(w1 << 16) * inv,
                                                __uint_as_float(w1 & 0xffff0000u) * inv, p, true);
  }
  return c;
}

// One row of an fp8 cache (128 elements: 16 pieces of 8 codes) from the 16 lanes
// that hold it, under the conditions of kv8_quant8: lane c stores its 8 codes at
// codes[row * 16 + c], lane 0 the scale at scales[row].  The words are made
// opaque first, so what the quantiser does with them has no say in how the
// compiler contracts the arithmetic that produced them (the RoPE of a k row is
// text shared with the bf16 kernels and must round as it does there).
__device__ __forceinline__ void kv8_store_row(u32x4 v, u32x2* __restrict__ codes, float* __restrict__ scales,
                                              size_t row, int c) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    u32 w = v[e];
    asm("" : "+v"(w));
    v[e] = w;
  }
  float sc;
  const u32x2 q = kv8_quant8(v, &sc);
  codes[row * 16 + c] = q;
  if (c == 0) scales[row] = sc;
}

}  // namespace gpbs_hip
