// MXFP4 (OCP e2m1 codes, one E8M0 scale per 32 k) weight-streaming linear for the
// Llama inference tenant: the fp8 decode linear of fp8_kernels.hip with the
// weight at 4.25 bits per element instead of 8.
//
//     Y[m, n] = (sum_k Xq[m, k] deq(W)[n, k]) * sx[m]  (+ resid[m, n])
//
// Xq are the e4m3 rows and sx the fp32 row scales of the fp8 quantisers
// (k_quant_rows_fp8, k_rmsnorm_quant_fp8, k_swiglu_quant_fp8), unchanged.  W is
// dequantised inside the MFMA and nowhere else: the block-scaled
// v_mfma_scale_f32_16x16x128_f8f6f4 takes Xq as its e4m3 operand (cbsz = 0,
// scale byte 0x7f = 1.0) and the e2m1 codes as its fp4 operand (blgp = 4, 4
// VGPRs), with the E8M0 byte of each lane's 32 codes in the lane's scale
// register, the byte picked by op_sel.  Accumulation is fp32, the output bf16
// through the f2bf rounding of the fp8 kernel.
//
// Operand lane map, measured with one-hot rows (tests/test_gpu_mxfp4_linear.py):
// lane l holds row / column (l & 15).  Its fp4 operand, 16 bytes in 4 VGPRs, is
// the 32 consecutive k from 32 (l >> 4) of the instruction's 128, element 2 i
// in the low nibble of byte i: exactly one MX block, and the lane's scale byte
// is that block's.  Its e4m3 operand, 32 bytes in 8 VGPRs, is two runs of 16:
// VGPRs 0..3 hold k = 16 (l >> 4) .. + 16, VGPRs 4..7 hold k = 64 + 16 (l >> 4)
// .. + 16.  (A kernel that builds both operands as e4m3 the same way, like
// fp8_gemm_kernels.hip, cannot tell: any common k order gives the same sum.)
// The one-hot and scale-placement tests prove the pairing, the nibble order
// and the byte that op_sel picks on exact data, for every k.
//
// Work shape, as k_fp8_gemm_skinny: one workgroup per 16 output columns, 8 waves
// splitting K in blocks of 256 k (128 bytes of a weight row), two blocks of a
// wave in flight per trip, partials reduced through LDS.  A block is two MFMAs
// (u = 0, 1) per 16-row M tile.  W is stored in lane order (Mxfp4Weight):
// for strip n0 / 16, block kb, step u the 64 lanes' 16-byte pieces are one
// contiguous 1 KiB run, and the block's 128 scale bytes one contiguous run of
// a 2-byte word per lane: byte u is the scale of the lane's codes at step u.
#include "common.hpp"

namespace gpbs_fp4 {

using namespace gpbs_hip;

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int kWaves = 8;
constexpr int kOne = 0x7f7f7f7f;  // E8M0 1.0 in every byte: the scale of the e4m3 operand

__device__ __forceinline__ unsigned short f2bf(float f) {
  u32 u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even
  return (unsigned short)(u >> 16);
}

__device__ __forceinline__ i32x8 frag8(u32x4 lo, u32x4 hi) {
  return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// The fp4 operand is read from the first 4 of the 8 registers.
__device__ __forceinline__ i32x8 frag4(u32x4 v) {
  return i32x8{(int)v[0], (int)v[1], (int)v[2], (int)v[3], 0, 0, 0, 0};
}

// One 256-k block of one M tile: a[2 u], a[2 u + 1] are the lane's two runs of
// 16 e4m3 bytes of step u, b[u] its 32 codes, byte u of sc their scale.
__device__ __forceinline__ f32x4 block_mfma(const u32x4* a, const u32x4* b, int sc, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag8(a[0], a[1]), frag4(b[0]), acc, 0, 4, 0, kOne, 0, sc);
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(frag8(a[2], a[3]), frag4(b[1]), acc, 0, 4, 0, kOne, 1, sc);
}

// MT = number of 16-row M tiles (M <= 16 * MT).  K % 256 == 0, N % 16 == 0.
template <int MT, int WV>
__global__ __launch_bounds__(WV * 64) void k_mxfp4_gemm_skinny(const unsigned char* __restrict__ xq,
                                                                const float* __restrict__ sx,
                                                                const unsigned char* __restrict__ wq,
                                                                const unsigned char* __restrict__ ws,
                                                                unsigned short* __restrict__ y,
                                                                const unsigned short* __restrict__ resid, int M, int N,
                                                                int K) {
  __shared__ f32x4 red[WV][MT][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int k16 = K >> 4;  // 16-byte units per row of X
  const int nkb = K >> 8;  // blocks of 256 k: 2 KiB of codes and 128 scale bytes per strip
  const u32x4* wrow = reinterpret_cast<const u32x4*>(wq) + (size_t)blockIdx.x * nkb * 128 + lane;
  const unsigned short* srow = reinterpret_cast<const unsigned short*>(ws) + (size_t)blockIdx.x * nkb * 64 + lane;
  const u32x4* xb = reinterpret_cast<const u32x4*>(xq);
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int kb = w; kb < nkb; kb += 2 * WV) {
    const bool two = kb + WV < nkb;
    u32x4 b0[2], b1[2];
    int s0, s1 = 0;
#pragma unroll
    for (int u = 0; u < 2; ++u) b0[u] = wrow[kb * 128 + u * 64];
    s0 = srow[kb * 64];
    if (two) {
#pragma unroll
      for (int u = 0; u < 2; ++u) b1[u] = wrow[(kb + WV) * 128 + u * 64];
      s1 = srow[(kb + WV) * 64];
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = t * 16 + r;
      const u32x4* xr = xb + (size_t)m * k16 + g;  // 16-byte units g and 4 + g of each 128 k
      u32x4 a[4];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        a[2 * u] = m < M ? xr[kb * 16 + u * 8] : u32x4{0u, 0u, 0u, 0u};
        a[2 * u + 1] = m < M ? xr[kb * 16 + u * 8 + 4] : u32x4{0u, 0u, 0u, 0u};
      }
      acc[t] = block_mfma(a, b0, s0, acc[t]);
      if (two) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          a[2 * u] = m < M ? xr[(kb + WV) * 16 + u * 8] : u32x4{0u, 0u, 0u, 0u};
          a[2 * u + 1] = m < M ? xr[(kb + WV) * 16 + u * 8 + 4] : u32x4{0u, 0u, 0u, 0u};
        }
        acc[t] = block_mfma(a, b1, s1, acc[t]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < MT; ++t) red[w][t][lane] = acc[t];
  __syncthreads();
  // C/D map of 16x16 MFMA: col = lane & 15 (n), row = 4 * (lane >> 4) + i (m).
  for (int e = threadIdx.x; e < MT * 64; e += WV * 64) {
    const int t = e >> 6, l = e & 63;
    f32x4 s = red[0][t][l];
#pragma unroll
    for (int v = 1; v < WV; ++v) s += red[v][t][l];
    const int n = n0 + (l & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = t * 16 + 4 * (l >> 4) + i;
      if (m < M) {
        float v = s[i] * sx[m];
        if (resid) v += __uint_as_float((u32)resid[(size_t)m * N + n] << 16);  // fused residual add
        y[(size_t)m * N + n] = f2bf(v);
      }
    }
  }
}

}  // namespace gpbs_fp4

using namespace gpbs_fp4;

extern "C" {

int gpbs_hip_mxfp4_linear_res(const void* xq, const float* sx, const void* wq, const void* ws, void* y,
                              const void* resid, int M, int N, int K, hipStream_t s) {
  if (M <= 0 || M > 64 || N <= 0 || N % 16 || K <= 0 || K % 256) return -22;
  const auto* xp = (const unsigned char*)xq;
  const auto* wp = (const unsigned char*)wq;
  const auto* sp = (const unsigned char*)ws;
  auto* yp = (unsigned short*)y;
  const auto* rp = (const unsigned short*)resid;
  const dim3 grid(N / 16), block(kWaves * 64);
  if (M <= 16)
    hipLaunchKernelGGL((k_mxfp4_gemm_skinny<1, kWaves>), grid, block, 0, s, xp, sx, wp, sp, yp, rp, M, N, K);
  else if (M <= 32)
    hipLaunchKernelGGL((k_mxfp4_gemm_skinny<2, kWaves>), grid, block, 0, s, xp, sx, wp, sp, yp, rp, M, N, K);
  else
    hipLaunchKernelGGL((k_mxfp4_gemm_skinny<4, kWaves>), grid, block, 0, s, xp, sx, wp, sp, yp, rp, M, N, K);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int gpbs_hip_mxfp4_linear(const void* xq, const float* sx, const void* wq, const void* ws, void* y, int M, int N,
                          int K, hipStream_t s) {
  return gpbs_hip_mxfp4_linear_res(xq, sx, wq, ws, y, nullptr, M, N, K, s);
}

}  // extern "C"
