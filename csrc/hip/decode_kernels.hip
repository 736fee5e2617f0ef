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
// Each kernel exists in four forms, one per KV-cache form of attn_cache.hpp:
// the plain names are for DenseUniform, _seq for DenseSeq, _paged for Paged and
// _paged_kv8 for PagedKv8.  A write kernel is a wrapper that builds its view from
// its own parameters and calls the one template; the attention kernels share
// their text by inclusion (see below).
#include "attn_entry.hpp"

namespace gpbs_dec {

using namespace gpbs_hip;

// The write kernel over cache view cv.  A live sequence (its position is a row of
// the cache: 0 <= pos < cv.rows()) gets q with RoPE and its k (with RoPE) and v row stored at
// its position; an idle one touches neither cache nor RoPE table and gets a zero
// q row.  The uniform view has no idle sequences and takes any hd % 8 == 0; the
// paged views take hd = 128 only.
// Fp8Rows::store: threads i .. i + 15 of a row are consecutive from a multiple of
// 16 (kWriteThreads, the grid stride and n8 are multiples of 16) and share (b, hh): they
// take the idle and dropped-write branches together and leave the loop together,
// so the shuffles of kv8_quant8 stay inside the group.
// Launch with kWriteThreads threads a workgroup only (launch_write): the loop strides by that constant.
template <class View>
__device__ __forceinline__ void qkv_rope_cache(const View cv, const u32x4* qkv, const float* cosb, const float* sinb,
                                               const int* posb, const int* table, u32x4* qo,
                                               typename View::Piece* kc, typename View::Piece* vc, float* ksc,
                                               float* vsc, int B, int H, int Hkv, int hd) {
  int pos0 = 0;  // the batch's position
  if constexpr (!View::kPerSeq) pos0 = *posb;
  const int per_head = hd / 8, heads = H + 2 * Hkv;
  const size_t n8 = (size_t)B * heads * per_head;
  for (size_t i = (size_t)blockIdx.x * kWriteThreads + threadIdx.x; i < n8; i += (size_t)gridDim.x * kWriteThreads) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const int b = (int)(i / per_head / heads);
    int pos = pos0;
    if constexpr (View::kPerSeq) {
      pos = posb[b];
      if (pos < 0 || pos >= cv.rows()) {  // idle slot
        if (hh < H) qo[((size_t)b * H + hh) * per_head + c] = u32x4{0u, 0u, 0u, 0u};
        continue;
      }
    }
    const u32x4 v = qkv[i];
    const typename View::Where w = cv.locate(table, b, pos, 0);
    if (hh >= H + Hkv) {  // v: the raw row into the cache row
      if (w.ok) View::store(v, vc, vsc, cv.row(w, Hkv, hh - H - Hkv), c, per_head);
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
    else if (w.ok)  // k: after RoPE and the rounding of pack2
      View::store(o, kc, ksc, cv.row(w, Hkv, hh - H), c, per_head);
  }
}

__global__ __launch_bounds__(kWriteThreads) void k_qkv_rope_cache(const u32x4* __restrict__ qkv,
                                                                  const float* __restrict__ cosb,
                                                                  const float* __restrict__ sinb,
                                                                  const int* __restrict__ dpos, u32x4* __restrict__ qo,
                                                                  u32x4* __restrict__ kc, u32x4* __restrict__ vc, int B,
                                                                  int H, int Hkv, int C, int hd) {
  qkv_rope_cache(DenseUniform(C), qkv, cosb, sinb, dpos, nullptr, qo, kc, vc, nullptr, nullptr, B, H, Hkv, hd);
}

__global__ __launch_bounds__(kWriteThreads) void k_qkv_rope_cache_seq(const u32x4* __restrict__ qkv,
                                                            const float* __restrict__ cosb,
                                                            const float* __restrict__ sinb,
                                                            const int* __restrict__ posb, u32x4* __restrict__ qo,
                                                            u32x4* __restrict__ kc, u32x4* __restrict__ vc, int B,
                                                            int H, int Hkv, int C, int hd) {
  qkv_rope_cache(DenseSeq(C), qkv, cosb, sinb, posb, nullptr, qo, kc, vc, nullptr, nullptr, B, H, Hkv, hd);
}

__global__ __launch_bounds__(kWriteThreads) void k_qkv_rope_cache_paged(const u32x4* __restrict__ qkv,
                                                              const float* __restrict__ cosb,
                                                              const float* __restrict__ sinb,
                                                              const int* __restrict__ posb,
                                                              const int* __restrict__ table, u32x4* __restrict__ qo,
                                                              u32x4* __restrict__ kp, u32x4* __restrict__ vp, int B,
                                                              int H, int Hkv, int NP, int P, int psh, int hd) {
  qkv_rope_cache(Paged(NP, P, psh), qkv, cosb, sinb, posb, table, qo, kp, vp, nullptr, nullptr, B, H, Hkv, hd);
}

__global__ __launch_bounds__(kWriteThreads) void k_qkv_rope_cache_paged_kv8(const u32x4* __restrict__ qkv,
                                                                  const float* __restrict__ cosb,
                                                                  const float* __restrict__ sinb,
                                                                  const int* __restrict__ posb,
                                                                  const int* __restrict__ table,
                                                                  u32x4* __restrict__ qo, u32x2* __restrict__ kp,
                                                                  u32x2* __restrict__ vp, float* __restrict__ ksc,
                                                                  float* __restrict__ vsc, int B, int H, int Hkv,
                                                                  int NP, int P, int psh, int hd) {
  qkv_rope_cache(PagedKv8(NP, P, psh), qkv, cosb, sinb, posb, table, qo, kp, vp, ksc, vsc, B, H, Hkv, hd);
}

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

// Merge the nsplit partials of each (batch, KV head): grid B * Hkv, G * 64 threads.
// The merge touches no cache.  kIdleRows is its only switch: where sequences can
// be idle, an idle one has Ls == 0 in every partial and gets zero bits, not
// 0 * inf; the uniform kernel keeps its unguarded division.
template <bool kIdleRows>
__device__ __forceinline__ void decode_attn_combine(const float* ws, u32* out, int Hkv, int G, int nsplit) {
  const int bh = blockIdx.x, b = bh / Hkv, kvh = bh % Hkv;
  const int g = threadIdx.x / 64, d = 2 * (threadIdx.x % 64);
  if (g >= G) return;
  float M = -INFINITY;
  for (int sp = 0; sp < nsplit; ++sp) M = fmaxf(M, ws[(((size_t)bh * nsplit + sp) * G + g) * (kHd + 2) + kHd]);
  float Ls = 0.f, a0 = 0.f, a1 = 0.f;
  for (int sp = 0; sp < nsplit; ++sp) {
    const float* p = ws + (((size_t)bh * nsplit + sp) * G + g) * (kHd + 2);
    const float f = p[kHd] == -INFINITY ? 0.f : __expf(p[kHd] - M);
    Ls += p[kHd + 1] * f;
    a0 += p[d] * f;
    a1 += p[d + 1] * f;
  }
  float inv;
  if constexpr (kIdleRows)
    inv = Ls == 0.f ? 0.f : 1.f / Ls;
  else
    inv = 1.f / Ls;
  out[((size_t)b * Hkv * G + kvh * G + g) * (kHd / 2) + d / 2] = pack2(a0 * inv, a1 * inv);
}

__global__ __launch_bounds__(512) void k_decode_attn_combine(const float* __restrict__ ws, u32* __restrict__ out,
                                                             int Hkv, int G, int nsplit) {
  decode_attn_combine<false>(ws, out, Hkv, G, nsplit);
}

// serves the _seq, _paged and _paged_kv8 attention kernels alike
__global__ __launch_bounds__(512) void k_decode_attn_combine_seq(const float* __restrict__ ws, u32* __restrict__ out,
                                                                 int Hkv, int G, int nsplit) {
  decode_attn_combine<true>(ws, out, Hkv, G, nsplit);
}

// The attention kernel is the one part of this file that is not a template over
// a view: decode_attn_body.hpp is its text, included once per cache form.  As a
// function template called from four wrappers the same text compiles to other
// fused multiply-adds in the QK^T sum for G >= 2 (the compiler simplifies an
// inlined callee twice, and the contraction of q0 * k0 + q1 * k1 follows the
// shape that leaves), which moves output bits; only text that is compiled in the
// kernel itself keeps the instructions these kernels always had.
// GPBS_SEQ: 0 DenseUniform (k_decode_attn), 1 DenseSeq (k_decode_attn_seq),
// 2 Paged (k_decode_attn_paged), 3 PagedKv8 (k_decode_attn_paged_kv8).
#define GPBS_SEQ 0
#include "decode_attn_body.hpp"
#undef GPBS_SEQ
#define GPBS_SEQ 1
#include "decode_attn_body.hpp"
#undef GPBS_SEQ
#define GPBS_SEQ 2
#include "decode_attn_body.hpp"
#undef GPBS_SEQ
#define GPBS_SEQ 3
#include "decode_attn_body.hpp"
#undef GPBS_SEQ

}  // namespace gpbs_dec

using namespace gpbs_dec;

namespace {

// pieces of 16 bytes in the packed qkv rows of a launch
size_t qkv_pieces(int B, int H, int Hkv, int hd) { return (size_t)B * (H + 2 * Hkv) * hd / 8; }

// what every decode attention entry point refuses, whatever the cache
bool bad_attn(int B, int H, int Hkv, int hd, const int* pos, int nsplit, const void* ws) {
  return hd != kHd || B <= 0 || Hkv <= 0 || H % Hkv || !pos || nsplit < 1 || (nsplit > 1 && !ws);
}

// an attention kernel for G = H / Hkv (launch(g, grid, block)), then the merge of its nsplit partials
template <class Launch>
int launch_attn(int B, int H, int Hkv, int nsplit, void* out, void* ws, bool idle_rows, hipStream_t s, Launch launch) {
  const int G = H / Hkv;
  const dim3 grid(B * Hkv * nsplit), block(kAttnWaves * 64);
  if (!for_group(G, [&](auto g) { launch(g, grid, block); })) return -22;
  if (nsplit > 1)
    hipLaunchKernelGGL(idle_rows ? k_decode_attn_combine_seq : k_decode_attn_combine, dim3(B * Hkv), dim3(G * 64), 0, s,
                       (const float*)ws, (u32*)out, Hkv, G, nsplit);
  return launched();
}

}  // namespace

extern "C" {

int gpbs_hip_qkv_rope_cache(const void* qkv, const float* cosb, const float* sinb, const int* dpos, void* qo, void* kc,
                            void* vc, int B, int H, int Hkv, int C, int hd, hipStream_t s) {
  if (B <= 0 || H <= 0 || Hkv <= 0 || C <= 0 || hd % 8 || !dpos) return -22;
  return launch_write(k_qkv_rope_cache, qkv_pieces(B, H, Hkv, hd), 2048, s,
                      (const u32x4*)qkv, cosb, sinb, dpos, (u32x4*)qo, (u32x4*)kc,
                      (u32x4*)vc, B, H, Hkv, C, hd);
}

int gpbs_hip_decode_attn(const void* q, const void* kc, const void* vc, const int* dpos, void* out, void* ws,
                         int nsplit, int B, int H, int Hkv, int C, int hd, float scale, hipStream_t s) {
  if (bad_attn(B, H, Hkv, hd, dpos, nsplit, ws) || C <= 0) return -22;
  return launch_attn(B, H, Hkv, nsplit, out, ws, false, s, [&](auto g, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_decode_attn<decltype(g)::value>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kc,
                       (const u32*)vc, dpos, (u32*)out, (float*)ws, Hkv, C, scale, nsplit);
  });
}

int gpbs_hip_qkv_rope_cache_seq(const void* qkv, const float* cosb, const float* sinb, const int* posb, void* qo,
                                void* kc, void* vc, int B, int H, int Hkv, int C, int hd, hipStream_t s) {
  if (B <= 0 || H <= 0 || Hkv <= 0 || C <= 0 || hd % 8 || !posb) return -22;
  return launch_write(k_qkv_rope_cache_seq, qkv_pieces(B, H, Hkv, hd), 2048, s,
                      (const u32x4*)qkv, cosb, sinb, posb, (u32x4*)qo,
                      (u32x4*)kc, (u32x4*)vc, B, H, Hkv, C, hd);
}

int gpbs_hip_decode_attn_seq(const void* q, const void* kc, const void* vc, const int* posb, void* out, void* ws,
                             int nsplit, int B, int H, int Hkv, int C, int hd, float scale, hipStream_t s) {
  if (bad_attn(B, H, Hkv, hd, posb, nsplit, ws) || C <= 0) return -22;
  return launch_attn(B, H, Hkv, nsplit, out, ws, true, s, [&](auto g, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_decode_attn_seq<decltype(g)::value>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kc,
                       (const u32*)vc, posb, (u32*)out, (float*)ws, Hkv, C, scale, nsplit);
  });
}

int gpbs_hip_qkv_rope_cache_paged(const void* qkv, const float* cosb, const float* sinb, const int* posb,
                                  const int* table, void* qo, void* kp, void* vp, int B, int H, int Hkv, int NP, int P,
                                  int page, int hd, hipStream_t s) {
  const int psh = page_shift(page);
  if (B <= 0 || H <= 0 || Hkv <= 0 || bad_pages(NP, P, psh) || hd != kHd || !posb || !table) return -22;
  return launch_write(k_qkv_rope_cache_paged, qkv_pieces(B, H, Hkv, hd), 2048, s,
                      (const u32x4*)qkv, cosb, sinb, posb, table,
                      (u32x4*)qo, (u32x4*)kp, (u32x4*)vp, B, H, Hkv, NP, P, psh, hd);
}

int gpbs_hip_decode_attn_paged(const void* q, const void* kp, const void* vp, const int* posb, const int* table,
                               void* out, void* ws, int nsplit, int B, int H, int Hkv, int NP, int P, int page, int hd,
                               float scale, hipStream_t s) {
  const int psh = page_shift(page);
  if (bad_attn(B, H, Hkv, hd, posb, nsplit, ws) || bad_pages(NP, P, psh) || !table) return -22;
  return launch_attn(B, H, Hkv, nsplit, out, ws, true, s, [&](auto g, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_decode_attn_paged<decltype(g)::value>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kp,
                       (const u32*)vp, posb, table, (u32*)out, (float*)ws, Hkv, NP, P, psh, scale, nsplit);
  });
}

// the paged entry points over an fp8 cache: e4m3 code pools kp / vp [P, Hkv, page, 128] and fp32 scales
// ksc / vsc [P, Hkv, page]
int gpbs_hip_qkv_rope_cache_paged_kv8(const void* qkv, const float* cosb, const float* sinb, const int* posb,
                                      const int* table, void* qo, void* kp, void* vp, float* ksc, float* vsc, int B,
                                      int H, int Hkv, int NP, int P, int page, int hd, hipStream_t s) {
  const int psh = page_shift(page);
  if (any_null({qkv, cosb, sinb, qo, kp, vp, ksc, vsc, posb, table}) || B <= 0 || H <= 0 || Hkv <= 0 ||
      bad_pages(NP, P, psh) || hd != kHd)
    return -22;
  return launch_write(k_qkv_rope_cache_paged_kv8, qkv_pieces(B, H, Hkv, hd), 2048, s,
                      (const u32x4*)qkv, cosb, sinb, posb, table,
                      (u32x4*)qo, (u32x2*)kp, (u32x2*)vp, ksc, vsc, B, H, Hkv, NP, P, psh, hd);
}

int gpbs_hip_decode_attn_paged_kv8(const void* q, const void* kp, const void* vp, const float* ksc, const float* vsc,
                                   const int* posb, const int* table, void* out, void* ws, int nsplit, int B, int H,
                                   int Hkv, int NP, int P, int page, int hd, float scale, hipStream_t s) {
  const int psh = page_shift(page);
  if (any_null({q, kp, vp, ksc, vsc, out, table}) || bad_attn(B, H, Hkv, hd, posb, nsplit, ws) ||
      bad_pages(NP, P, psh))
    return -22;
  return launch_attn(B, H, Hkv, nsplit, out, ws, true, s, [&](auto g, dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_decode_attn_paged_kv8<decltype(g)::value>, grid, block, 0, s, (const u32x4*)q,
                       (const u32x4*)kp, (const u32x2*)vp, ksc, vsc, posb, table, (u32*)out, (float*)ws, Hkv, NP, P,
                       psh, scale, nsplit);
  });
}

}  // extern "C"
