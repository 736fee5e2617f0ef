// Fused single-token decode kernels for the graph-captured Llama decode step
// (config #5).  Every launch saved is ~4-5 us per layer at batch 8, so the
// attention block runs in two launches after the qkv linear:
//
//   k_qkv_rope_cache : packed qkv linear output [B, (H + 2 Hkv) hd] ->
//                      q with RoPE -> q_out [B, H, hd]; k with RoPE and v written
//                      straight into the static KV cache [B, Hkv, C, hd] at the
//                      device-resident position (replaces 2 slice copies, 2 RoPE
//                      launches, 2 index_copy_ and their transposes)
//   k_decode_attn    : grouped-query attention of the new token over cache rows
//                      0..pos: one workgroup per (batch, KV head), the G query
//                      heads of the group share every K/V row read; 8 waves split
//                      the keys in 64-key steps (a lane owns a key for QK^T; for
//                      PV a lane owns 8 dims of every 4th key), online softmax,
//                      wave partials merged in LDS; with nsplit > 1 the keys are
//                      split over workgroups too and k_decode_attn_combine merges.
//
// The _seq forms take one position per sequence (int32 [B]) instead of one for
// the batch: sequence b is active iff 0 <= pos[b] < C, any other value is an
// idle slot.  An idle sequence writes no cache row, loads none, and its q / out
// rows are zero bits; an active one computes exactly what the uniform kernel
// computes at pos = pos[b] (same chunking, same order of operations).
//
// The _paged forms are the _seq forms over a paged cache: pools
// [P, Hkv, page, hd] and an int32 block table [B, NP]; logical row r of sequence
// b lives in page table[b, r / page] at page row r % page, page in 64/128/256,
// and Cl = NP * page takes the place of C in the slot rule.  Only the entries
// of pages that hold rows 0 .. pos[b] are read.  An entry outside [0, P) never
// forms an address outside the pools: the write through it is dropped, the
// reads through it come from page 0.
//
// The _kv8 forms are the _paged forms over an fp8 cache (kv8_codec.hpp): e4m3
// code pools [P, Hkv, page, hd] of one byte per element and fp32 scales
// [P, Hkv, page], one power of two per cached row and KV head.  The write kernel
// quantises the row the bf16 kernel would have stored; the attention kernel
// rebuilds that row's bf16 words exactly (code times scale rounds nowhere) and
// goes on in the shared text, so it gives the bits of k_decode_attn_paged over
// the dequantised pools.  The out-of-range rule covers all four tensors.
#include <algorithm>
#include <climits>

#include "common.hpp"
#include "kv8_codec.hpp"

namespace gpbs_dec {

using namespace gpbs_hip;

__device__ __forceinline__ float bfl(u32 w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bfh(u32 w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ u32 pack2(float lo, float hi) {
  return (u32)__builtin_bit_cast(u16, (__bf16)lo) | ((u32)__builtin_bit_cast(u16, (__bf16)hi) << 16);
}

__global__ __launch_bounds__(256) void k_qkv_rope_cache(const u32x4* __restrict__ qkv, const float* __restrict__ cosb,
                                                        const float* __restrict__ sinb, const int* __restrict__ dpos,
                                                        u32x4* __restrict__ qo, u32x4* __restrict__ kc,
                                                        u32x4* __restrict__ vc, int B, int H, int Hkv, int C, int hd) {
  const int pos = *dpos;
  const int per_head = hd / 8, heads = H + 2 * Hkv;
  const size_t n8 = (size_t)B * heads * per_head;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const int b = (int)(i / per_head / heads);
    const u32x4 v = qkv[i];
    if (hh >= H + Hkv) {  // v: plain copy into the cache row
      vc[(((size_t)b * Hkv + (hh - H - Hkv)) * C + pos) * per_head + c] = v;
      continue;
    }
    const float* cr = cosb + (size_t)pos * (hd / 2) + c * 4;
    const float* sr = sinb + (size_t)pos * (hd / 2) + c * 4;
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = bfl(v[e]), bb = bfh(v[e]), cs = cr[e], sn = sr[e];
      o[e] = pack2(a * cs - bb * sn, a * sn + bb * cs);
    }
    if (hh < H)
      qo[((size_t)b * H + hh) * per_head + c] = o;
    else
      kc[(((size_t)b * Hkv + (hh - H)) * C + pos) * per_head + c] = o;
  }
}

// k_qkv_rope_cache with one position per sequence; an idle sequence (pos[b] outside
// [0, C)) touches neither cache nor RoPE table and gets a zero q row.
__global__ __launch_bounds__(256) void k_qkv_rope_cache_seq(const u32x4* __restrict__ qkv,
                                                            const float* __restrict__ cosb,
                                                            const float* __restrict__ sinb,
                                                            const int* __restrict__ posb, u32x4* __restrict__ qo,
                                                            u32x4* __restrict__ kc, u32x4* __restrict__ vc, int B,
                                                            int H, int Hkv, int C, int hd) {
  const int per_head = hd / 8, heads = H + 2 * Hkv;
  const size_t n8 = (size_t)B * heads * per_head;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const int b = (int)(i / per_head / heads);
    const int pos = posb[b];
    if (pos < 0 || pos >= C) {  // idle slot
      if (hh < H) qo[((size_t)b * H + hh) * per_head + c] = u32x4{0u, 0u, 0u, 0u};
      continue;
    }
    const u32x4 v = qkv[i];
    if (hh >= H + Hkv) {  // v: plain copy into the cache row
      vc[(((size_t)b * Hkv + (hh - H - Hkv)) * C + pos) * per_head + c] = v;
      continue;
    }
    const float* cr = cosb + (size_t)pos * (hd / 2) + c * 4;
    const float* sr = sinb + (size_t)pos * (hd / 2) + c * 4;
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = bfl(v[e]), bb = bfh(v[e]), cs = cr[e], sn = sr[e];
      o[e] = pack2(a * cs - bb * sn, a * sn + bb * cs);
    }
    if (hh < H)
      qo[((size_t)b * H + hh) * per_head + c] = o;
    else
      kc[(((size_t)b * Hkv + (hh - H)) * C + pos) * per_head + c] = o;
  }
}

// a block-table entry as a page to read: anything outside [0, P) is page 0
__device__ __forceinline__ int page_or0(int e, int P) { return (e >= 0 && e < P) ? e : 0; }

// k_qkv_rope_cache_seq through the block table: an active sequence (0 <= pos[b] <
// NP * page) writes row pos[b] % page of page table[b, pos[b] / page]; the write
// is dropped if that entry is outside [0, P).
__global__ __launch_bounds__(256) void k_qkv_rope_cache_paged(const u32x4* __restrict__ qkv,
                                                              const float* __restrict__ cosb,
                                                              const float* __restrict__ sinb,
                                                              const int* __restrict__ posb,
                                                              const int* __restrict__ table, u32x4* __restrict__ qo,
                                                              u32x4* __restrict__ kp, u32x4* __restrict__ vp, int B,
                                                              int H, int Hkv, int NP, int P, int psh, int hd) {
  const int per_head = hd / 8, heads = H + 2 * Hkv;
  const size_t n8 = (size_t)B * heads * per_head;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const int b = (int)(i / per_head / heads);
    const int pos = posb[b];
    if (pos < 0 || pos >= (NP << psh)) {  // idle slot
      if (hh < H) qo[((size_t)b * H + hh) * per_head + c] = u32x4{0u, 0u, 0u, 0u};
      continue;
    }
    const u32x4 v = qkv[i];
    const int pg = table[(size_t)b * NP + (pos >> psh)];
    const bool ok = pg >= 0 && pg < P;
    const int prow = pos & ((1 << psh) - 1);
    if (hh >= H + Hkv) {  // v: plain copy into the page row
      if (ok) vp[((((size_t)pg * Hkv + (hh - H - Hkv)) << psh) + prow) * per_head + c] = v;
      continue;
    }
    const float* cr = cosb + (size_t)pos * (hd / 2) + c * 4;
    const float* sr = sinb + (size_t)pos * (hd / 2) + c * 4;
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = bfl(v[e]), bb = bfh(v[e]), cs = cr[e], sn = sr[e];
      o[e] = pack2(a * cs - bb * sn, a * sn + bb * cs);
    }
    if (hh < H)
      qo[((size_t)b * H + hh) * per_head + c] = o;
    else if (ok)
      kp[((((size_t)pg * Hkv + (hh - H)) << psh) + prow) * per_head + c] = o;
  }
}

// k_qkv_rope_cache_paged over an fp8 cache (kv8_codec.hpp): code pools kp / vp
// [P, Hkv, page, 128] of one byte per element and scales ksc / vsc [P, Hkv, page].
// q as above.  A k row (after RoPE and the rounding of pack2, the row the bf16
// kernel stores) or a v row is quantised by the 16 threads that hold it: 8 bytes
// of codes each, and thread 0 of the 16 stores the scale.  Threads i .. i + 15 of
// a row are consecutive from a multiple of 16 (256, the grid stride and n8 are
// multiples of 16) and share (b, hh): they take the idle and dropped-write
// branches together and leave the loop together, so the shuffles of kv8_quant8
// stay inside the group.  hd = 128 only.  Control flow and RoPE text are those of
// the bf16 _paged kernel, so that q and the k row round as they do there.
__global__ __launch_bounds__(256) void k_qkv_rope_cache_paged_kv8(const u32x4* __restrict__ qkv,
                                                                  const float* __restrict__ cosb,
                                                                  const float* __restrict__ sinb,
                                                                  const int* __restrict__ posb,
                                                                  const int* __restrict__ table,
                                                                  u32x4* __restrict__ qo, u32x2* __restrict__ kp,
                                                                  u32x2* __restrict__ vp, float* __restrict__ ksc,
                                                                  float* __restrict__ vsc, int B, int H, int Hkv,
                                                                  int NP, int P, int psh, int hd) {
  const int per_head = hd / 8, heads = H + 2 * Hkv;
  const size_t n8 = (size_t)B * heads * per_head;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const int b = (int)(i / per_head / heads);
    const int pos = posb[b];
    if (pos < 0 || pos >= (NP << psh)) {  // idle slot
      if (hh < H) qo[((size_t)b * H + hh) * per_head + c] = u32x4{0u, 0u, 0u, 0u};
      continue;
    }
    const u32x4 v = qkv[i];
    const int pg = table[(size_t)b * NP + (pos >> psh)];
    const bool ok = pg >= 0 && pg < P;
    const int prow = pos & ((1 << psh) - 1);
    if (hh >= H + Hkv) {  // v: the raw row, quantised into the page row
      if (ok) kv8_store_row(v, vp, vsc, (((size_t)pg * Hkv + (hh - H - Hkv)) << psh) + prow, c);
      continue;
    }
    const float* cr = cosb + (size_t)pos * (hd / 2) + c * 4;
    const float* sr = sinb + (size_t)pos * (hd / 2) + c * 4;
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = bfl(v[e]), bb = bfh(v[e]), cs = cr[e], sn = sr[e];
      o[e] = pack2(a * cs - bb * sn, a * sn + bb * cs);
    }
    if (hh < H)
      qo[((size_t)b * H + hh) * per_head + c] = o;
    else if (ok)
      kv8_store_row(o, kp, ksc, (((size_t)pg * Hkv + (hh - H)) << psh) + prow, c);
  }
}

constexpr int kHd = 128;  // head_dim of every Llama-3 size
constexpr int kAttnWaves = 8;

__device__ __forceinline__ float wmax(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wsum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// k_decode_attn<G>, k_decode_attn_combine and their per-sequence forms
// k_decode_attn_seq<G>, k_decode_attn_combine_seq are one source text compiled
// twice: the uniform kernels get exactly the tokens they always had.
#define GPBS_SEQ 0
#include "decode_attn_body.hpp"
#undef GPBS_SEQ
#define GPBS_SEQ 1
#include "decode_attn_body.hpp"
#undef GPBS_SEQ
// third compilation: k_decode_attn_paged<G> (merged by k_decode_attn_combine_seq)
#define GPBS_SEQ 2
#include "decode_attn_body.hpp"
#undef GPBS_SEQ
// fourth compilation: k_decode_attn_paged_kv8<G> (merged by k_decode_attn_combine_seq)
#define GPBS_SEQ 3
#include "decode_attn_body.hpp"
#undef GPBS_SEQ

}  // namespace gpbs_dec

using namespace gpbs_dec;

extern "C" {

int gpbs_hip_qkv_rope_cache(const void* qkv, const float* cosb, const float* sinb, const int* dpos, void* qo, void* kc,
                            void* vc, int B, int H, int Hkv, int C, int hd, hipStream_t s) {
  if (B <= 0 || H <= 0 || Hkv <= 0 || C <= 0 || hd % 8 || !dpos) return -22;
  const size_t n8 = (size_t)B * (H + 2 * Hkv) * hd / 8;
  int grid = (int)std::min<size_t>((n8 + 255) / 256, 2048);
  hipLaunchKernelGGL(k_qkv_rope_cache, dim3(grid), dim3(256), 0, s, (const u32x4*)qkv, cosb, sinb, dpos, (u32x4*)qo,
                     (u32x4*)kc, (u32x4*)vc, B, H, Hkv, C, hd);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int gpbs_hip_decode_attn(const void* q, const void* kc, const void* vc, const int* dpos, void* out, void* ws,
                         int nsplit, int B, int H, int Hkv, int C, int hd, float scale, hipStream_t s) {
  if (hd != kHd || B <= 0 || Hkv <= 0 || H % Hkv || C <= 0 || !dpos || nsplit < 1 || (nsplit > 1 && !ws)) return -22;
  const int G = H / Hkv;
  const dim3 grid(B * Hkv * nsplit), block(kAttnWaves * 64);
  float* w = (float*)ws;
  switch (G) {
    case 1: hipLaunchKernelGGL(k_decode_attn<1>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kc, (const u32*)vc,
                               dpos, (u32*)out, w, Hkv, C, scale, nsplit); break;
    case 2: hipLaunchKernelGGL(k_decode_attn<2>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kc, (const u32*)vc,
                               dpos, (u32*)out, w, Hkv, C, scale, nsplit); break;
    case 4: hipLaunchKernelGGL(k_decode_attn<4>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kc, (const u32*)vc,
                               dpos, (u32*)out, w, Hkv, C, scale, nsplit); break;
    case 8: hipLaunchKernelGGL(k_decode_attn<8>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kc, (const u32*)vc,
                               dpos, (u32*)out, w, Hkv, C, scale, nsplit); break;
    default: return -22;
  }
  if (nsplit > 1)
    hipLaunchKernelGGL(k_decode_attn_combine, dim3(B * Hkv), dim3(G * 64), 0, s, (const float*)w, (u32*)out, Hkv, G,
                       nsplit);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int gpbs_hip_qkv_rope_cache_seq(const void* qkv, const float* cosb, const float* sinb, const int* posb, void* qo,
                                void* kc, void* vc, int B, int H, int Hkv, int C, int hd, hipStream_t s) {
  if (B <= 0 || H <= 0 || Hkv <= 0 || C <= 0 || hd % 8 || !posb) return -22;
  const size_t n8 = (size_t)B * (H + 2 * Hkv) * hd / 8;
  int grid = (int)std::min<size_t>((n8 + 255) / 256, 2048);
  hipLaunchKernelGGL(k_qkv_rope_cache_seq, dim3(grid), dim3(256), 0, s, (const u32x4*)qkv, cosb, sinb, posb,
                     (u32x4*)qo, (u32x4*)kc, (u32x4*)vc, B, H, Hkv, C, hd);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int gpbs_hip_decode_attn_seq(const void* q, const void* kc, const void* vc, const int* posb, void* out, void* ws,
                             int nsplit, int B, int H, int Hkv, int C, int hd, float scale, hipStream_t s) {
  if (hd != kHd || B <= 0 || Hkv <= 0 || H % Hkv || C <= 0 || !posb || nsplit < 1 || (nsplit > 1 && !ws)) return -22;
  const int G = H / Hkv;
  const dim3 grid(B * Hkv * nsplit), block(kAttnWaves * 64);
  float* w = (float*)ws;
#define GPBS_DEC_SEQ_LAUNCH(g)                                                                                  \
  hipLaunchKernelGGL(k_decode_attn_seq<g>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kc, (const u32*)vc, \
                     posb, (u32*)out, w, Hkv, C, scale, nsplit)
  switch (G) {
    case 1: GPBS_DEC_SEQ_LAUNCH(1); break;
    case 2: GPBS_DEC_SEQ_LAUNCH(2); break;
    case 4: GPBS_DEC_SEQ_LAUNCH(4); break;
    case 8: GPBS_DEC_SEQ_LAUNCH(8); break;
    default: return -22;
  }
#undef GPBS_DEC_SEQ_LAUNCH
  if (nsplit > 1)
    hipLaunchKernelGGL(k_decode_attn_combine_seq, dim3(B * Hkv), dim3(G * 64), 0, s, (const float*)w, (u32*)out, Hkv,
                       G, nsplit);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// log2(page) for the page sizes the paged kernels take, -1 otherwise
static int page_shift(int page) { return page == 64 ? 6 : page == 128 ? 7 : page == 256 ? 8 : -1; }

int gpbs_hip_qkv_rope_cache_paged(const void* qkv, const float* cosb, const float* sinb, const int* posb,
                                  const int* table, void* qo, void* kp, void* vp, int B, int H, int Hkv, int NP, int P,
                                  int page, int hd, hipStream_t s) {
  const int psh = page_shift(page);
  if (B <= 0 || H <= 0 || Hkv <= 0 || NP < 1 || P < 1 || psh < 0 || hd != kHd || !posb || !table ||
      ((long long)NP << psh) > INT_MAX)
    return -22;
  const size_t n8 = (size_t)B * (H + 2 * Hkv) * hd / 8;
  int grid = (int)std::min<size_t>((n8 + 255) / 256, 2048);
  hipLaunchKernelGGL(k_qkv_rope_cache_paged, dim3(grid), dim3(256), 0, s, (const u32x4*)qkv, cosb, sinb, posb, table,
                     (u32x4*)qo, (u32x4*)kp, (u32x4*)vp, B, H, Hkv, NP, P, psh, hd);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int gpbs_hip_decode_attn_paged(const void* q, const void* kp, const void* vp, const int* posb, const int* table,
                               void* out, void* ws, int nsplit, int B, int H, int Hkv, int NP, int P, int page, int hd,
                               float scale, hipStream_t s) {
  const int psh = page_shift(page);
  if (hd != kHd || B <= 0 || Hkv <= 0 || H % Hkv || NP < 1 || P < 1 || psh < 0 || !posb || !table || nsplit < 1 ||
      (nsplit > 1 && !ws) || ((long long)NP << psh) > INT_MAX)
    return -22;
  const int G = H / Hkv;
  const dim3 grid(B * Hkv * nsplit), block(kAttnWaves * 64);
  float* w = (float*)ws;
#define GPBS_DEC_PAGED_LAUNCH(g)                                                                                   \
  hipLaunchKernelGGL(k_decode_attn_paged<g>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kp, (const u32*)vp, \
                     posb, table, (u32*)out, w, Hkv, NP, P, psh, scale, nsplit)
  switch (G) {
    case 1: GPBS_DEC_PAGED_LAUNCH(1); break;
    case 2: GPBS_DEC_PAGED_LAUNCH(2); break;
    case 4: GPBS_DEC_PAGED_LAUNCH(4); break;
    case 8: GPBS_DEC_PAGED_LAUNCH(8); break;
    default: return -22;
  }
#undef GPBS_DEC_PAGED_LAUNCH
  if (nsplit > 1)
    hipLaunchKernelGGL(k_decode_attn_combine_seq, dim3(B * Hkv), dim3(G * 64), 0, s, (const float*)w, (u32*)out, Hkv,
                       G, nsplit);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// the paged entry points over an fp8 cache: e4m3 code pools kp / vp [P, Hkv, page, 128] and fp32 scales
// ksc / vsc [P, Hkv, page]
int gpbs_hip_qkv_rope_cache_paged_kv8(const void* qkv, const float* cosb, const float* sinb, const int* posb,
                                      const int* table, void* qo, void* kp, void* vp, float* ksc, float* vsc, int B,
                                      int H, int Hkv, int NP, int P, int page, int hd, hipStream_t s) {
  const int psh = page_shift(page);
  if (!qkv || !cosb || !sinb || !qo || !kp || !vp || !ksc || !vsc || B <= 0 || H <= 0 || Hkv <= 0 || NP < 1 ||
      P < 1 || psh < 0 || hd != kHd || !posb || !table || ((long long)NP << psh) > INT_MAX)
    return -22;
  const size_t n8 = (size_t)B * (H + 2 * Hkv) * hd / 8;
  int grid = (int)std::min<size_t>((n8 + 255) / 256, 2048);
  hipLaunchKernelGGL(k_qkv_rope_cache_paged_kv8, dim3(grid), dim3(256), 0, s, (const u32x4*)qkv, cosb, sinb, posb,
                     table, (u32x4*)qo, (u32x2*)kp, (u32x2*)vp, ksc, vsc, B, H, Hkv, NP, P, psh, hd);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int gpbs_hip_decode_attn_paged_kv8(const void* q, const void* kp, const void* vp, const float* ksc, const float* vsc,
                                   const int* posb, const int* table, void* out, void* ws, int nsplit, int B, int H,
                                   int Hkv, int NP, int P, int page, int hd, float scale, hipStream_t s) {
  const int psh = page_shift(page);
  if (!q || !kp || !vp || !ksc || !vsc || !out || hd != kHd || B <= 0 || Hkv <= 0 || H % Hkv || NP < 1 || P < 1 ||
      psh < 0 || !posb || !table || nsplit < 1 || (nsplit > 1 && !ws) || ((long long)NP << psh) > INT_MAX)
    return -22;
  const int G = H / Hkv;
  const dim3 grid(B * Hkv * nsplit), block(kAttnWaves * 64);
  float* w = (float*)ws;
#define GPBS_DEC_KV8_LAUNCH(g)                                                                                \
  hipLaunchKernelGGL(k_decode_attn_paged_kv8<g>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kp,       \
                     (const u32x2*)vp, ksc, vsc, posb, table, (u32*)out, w, Hkv, NP, P, psh, scale, nsplit)
  switch (G) {
    case 1: GPBS_DEC_KV8_LAUNCH(1); break;
    case 2: GPBS_DEC_KV8_LAUNCH(2); break;
    case 4: GPBS_DEC_KV8_LAUNCH(4); break;
    case 8: GPBS_DEC_KV8_LAUNCH(8); break;
    default: return -22;
  }
#undef GPBS_DEC_KV8_LAUNCH
  if (nsplit > 1)
    hipLaunchKernelGGL(k_decode_attn_combine_seq, dim3(B * Hkv), dim3(G * 64), 0, s, (const float*)w, (u32*)out, Hkv,
                       G, nsplit);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
