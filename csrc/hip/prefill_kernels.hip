// Prefill (S new tokens) attention block of the Llama tenant on gfx950: two
// launches between the qkv and o linears, for any cache position, so a prompt
// can be run in chunks.
//
//   k_qkv_rope_cache_prefill : packed qkv [B, S, (H + 2 Hkv) hd] -> q with RoPE
//                      [B, S, H, hd]; k with RoPE and v written into rows
//                      pos .. pos + S - 1 of the static KV cache [B, Hkv, C, hd]
//                      (the S-token form of k_qkv_rope_cache; pos from the host).
//   k_prefill_attn   : causal grouped-query flash attention of the S new tokens
//                      over cache rows 0 .. pos + s, on v_mfma_f32_32x32x16_bf16.
//
// k_prefill_attn tiling.  A workgroup is 8 waves and owns 256 query rows of one
// (batch, KV head): the G query heads of the group times 256 / G consecutive
// tokens, row = g * (256 / G) + token, so every wave holds 32 consecutive tokens
// of one head and all rows of the workgroup share each K/V tile (staged once).
// Keys are walked in ascending tiles of 64 rows up to the workgroup's diagonal;
// a wave skips the tiles wholly above its own diagonal, and only tiles that
// cross a wave's diagonal (the tile holding row pos + S - 1 is one of them) are
// masked, by select.  Cache rows > pos + S - 1 are never addressed: the rows of
// the last tile past it are filled in LDS with a copy of row pos + S - 1, whose
// weight is an exact 0.  Workgroups are issued heaviest (latest tokens) first,
// and blockIdx % (B Hkv) is the (batch, KV head), so with B Hkv % 8 == 0 the
// query tiles of a head meet in one XCD's L2.
//
// Staging: each thread carries 2 + 2 16-byte pieces of the next K and V tile in
// registers across the MFMAs of the current one and writes them to LDS after the
// barrier.  Both tiles use one LDS image of 256-byte rows, 16-byte chunk ch of
// row r at 256 r + 16 (ch ^ (4 (r & 3) | ((r >> 2) & 3))), which serves the row
// reads of K (ds_read_b128) and the transposed reads of V (ds_read_b64_tr_b16).
//
// Lane maps (lane l: c = l & 31, h = l >> 5; reg i -> row(i, h) = (i & 3) +
// 8 (i >> 2) + 4 h):
//   S^T = K Q^T   A = K[key c][d = 16 ks + 8 h + j], B = Q[query c][same d]
//                 (Q fragments live in registers for the whole kernel);
//                 result reg i = score of key row(i, h), query c.  A query's
//                 scores sit in one lane pair (l, l ^ 32): the row max is 31
//                 fmax and one cross-lane exchange, m and the O rescale are
//                 per-lane scalars.
//   O^T = V^T P^T the score registers 8 s .. 8 s + 7 rounded to bf16 are the B
//                 fragment of k-step s as they stand (k = key row(8 s + j, h));
//                 A = V[key row(8 s + j, h)][d = 32 dt + c] comes from two
//                 transposed reads: lane group l >> 4 reads the 4-key x 16-dim
//                 block at keys 16 s + 4 h (+ 8), dims 32 dt + 16 ((l >> 4) & 1).
//                 result reg i of tile dt = O[query c][d = 32 dt + row(i, h)].
// Softmax is online in fp32 in the log2 domain; P is rounded to bf16 only as the
// PV operand, l is summed from those rounded values, 1 / l is applied in the
// epilogue.  Every tile rescales (no deferred rescale).  Keys ascend and key 0 is
// visible to every query, so a row's max is finite after the first tile.  No
// workspace, no atomics: equal inputs give equal bits.
//
// The _seq forms take a position and a length per sequence (int32 [B] each):
// sequence b contributes n_b = min(len[b], S, C - pos[b]) tokens at cache rows
// pos[b] .. pos[b] + n_b - 1, or none if pos[b] is outside [0, C) or len[b] <= 0.
// The launch is sized for S; tokens s >= n_b are padding: they write no cache
// row, their q / out rows are zero, and no q row >= n_b or cache row past
// pos[b] + n_b - 1 is addressed.  The tile walk of a workgroup depends on its
// sequence alone, so sequence b gets the bits of the uniform kernel run on it
// alone with (S = n_b, pos = pos[b]).
//
// The _paged forms are the _seq forms over a paged cache: pools
// [P, Hkv, page, hd] and an int32 block table [B, NP]; logical row r of sequence
// b lives in page table[b, r / page] at page row r % page, page in 64/128/256,
// and Cl = NP * page takes the place of C in n_b.  Only the entries of pages
// that hold rows 0 .. pos[b] + n_b - 1 are read.  An entry outside [0, P) never
// forms an address outside the pools: writes through it are dropped, reads
// through it come from page 0.
//
// The _kv8 forms are the _paged forms over an fp8 cache (kv8_codec.hpp): e4m3
// code pools [P, Hkv, page, hd] of one byte per element and fp32 scales
// [P, Hkv, page], one power of two per cached row and KV head.  The write kernel
// quantises the rows the bf16 kernel would have stored; the attention kernel
// prefetches codes and scales and dequantises (exactly) into the same LDS images,
// so it gives the bits of k_prefill_attn_paged over the dequantised pools.  The
// MFMAs stay bf16.  The out-of-range rule covers all four tensors.
#include <algorithm>
#include <climits>

#include "common.hpp"
#include "kv8_codec.hpp"

namespace gpbs_pf {

using namespace gpbs_hip;

__device__ __forceinline__ float bfl(u32 w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bfh(u32 w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ u32 pack2(float lo, float hi) {
  return (u32)__builtin_bit_cast(u16, (__bf16)lo) | ((u32)__builtin_bit_cast(u16, (__bf16)hi) << 16);
}

__global__ __launch_bounds__(256) void k_qkv_rope_cache_prefill(const u32x4* __restrict__ qkv,
                                                                const float* __restrict__ cosb,
                                                                const float* __restrict__ sinb,
                                                                u32x4* __restrict__ qo, u32x4* __restrict__ kc,
                                                                u32x4* __restrict__ vc, int B, int S, int H, int Hkv,
                                                                int C, int hd, int pos) {
  const int per_head = hd / 8, heads = H + 2 * Hkv;
  const size_t n8 = (size_t)B * S * heads * per_head;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const size_t bs = i / per_head / heads;
    const int s = (int)(bs % S), b = (int)(bs / S);
    const u32x4 v = qkv[i];
    if (hh >= H + Hkv) {  // v: plain copy into the cache row
      vc[(((size_t)b * Hkv + (hh - H - Hkv)) * C + pos + s) * per_head + c] = v;
      continue;
    }
    const float* cr = cosb + (size_t)(pos + s) * (hd / 2) + c * 4;
    const float* sr = sinb + (size_t)(pos + s) * (hd / 2) + c * 4;
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = bfl(v[e]), bb = bfh(v[e]), cs = cr[e], sn = sr[e];
      o[e] = pack2(a * cs - bb * sn, a * sn + bb * cs);
    }
    if (hh < H)
      qo[(bs * H + hh) * per_head + c] = o;
    else
      kc[(((size_t)b * Hkv + (hh - H)) * C + pos + s) * per_head + c] = o;
  }
}

// tokens that sequence b really has in a ragged launch of S (0: idle slot)
__device__ __forceinline__ int seq_tokens(int pos, int len, int S, int C) {
  return (pos < 0 || pos >= C || len <= 0) ? 0 : min(min(len, S), C - pos);
}

__global__ __launch_bounds__(256) void k_qkv_rope_cache_prefill_seq(const u32x4* __restrict__ qkv,
                                                                    const float* __restrict__ cosb,
                                                                    const float* __restrict__ sinb,
                                                                    const int* __restrict__ posb,
                                                                    const int* __restrict__ lenb,
                                                                    u32x4* __restrict__ qo, u32x4* __restrict__ kc,
                                                                    u32x4* __restrict__ vc, int B, int S, int H,
                                                                    int Hkv, int C, int hd) {
  const int per_head = hd / 8, heads = H + 2 * Hkv;
  const size_t n8 = (size_t)B * S * heads * per_head;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const size_t bs = i / per_head / heads;
    const int s = (int)(bs % S), b = (int)(bs / S);
    const int pos = posb[b];
    if (s >= seq_tokens(pos, lenb[b], S, C)) {  // padding token
      if (hh < H) qo[(bs * H + hh) * per_head + c] = u32x4{0u, 0u, 0u, 0u};
      continue;
    }
    const u32x4 v = qkv[i];
    if (hh >= H + Hkv) {  // v: plain copy into the cache row
      vc[(((size_t)b * Hkv + (hh - H - Hkv)) * C + pos + s) * per_head + c] = v;
      continue;
    }
    const float* cr = cosb + (size_t)(pos + s) * (hd / 2) + c * 4;
    const float* sr = sinb + (size_t)(pos + s) * (hd / 2) + c * 4;
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = bfl(v[e]), bb = bfh(v[e]), cs = cr[e], sn = sr[e];
      o[e] = pack2(a * cs - bb * sn, a * sn + bb * cs);
    }
    if (hh < H)
      qo[(bs * H + hh) * per_head + c] = o;
    else
      kc[(((size_t)b * Hkv + (hh - H)) * C + pos + s) * per_head + c] = o;
  }
}

// a block-table entry as a page to read: anything outside [0, P) is page 0
__device__ __forceinline__ int page_or0(int e, int P) { return (e >= 0 && e < P) ? e : 0; }

// k_qkv_rope_cache_prefill_seq through the block table: token s < n_b of sequence
// b goes to row (pos[b] + s) % page of page table[b, (pos[b] + s) / page]; the
// write is dropped if that entry is outside [0, P).
__global__ __launch_bounds__(256) void k_qkv_rope_cache_prefill_paged(const u32x4* __restrict__ qkv,
                                                                      const float* __restrict__ cosb,
                                                                      const float* __restrict__ sinb,
                                                                      const int* __restrict__ posb,
                                                                      const int* __restrict__ lenb,
                                                                      const int* __restrict__ table,
                                                                      u32x4* __restrict__ qo, u32x4* __restrict__ kp,
                                                                      u32x4* __restrict__ vp, int B, int S, int H,
                                                                      int Hkv, int NP, int P, int psh, int hd) {
  const int per_head = hd / 8, heads = H + 2 * Hkv;
  const size_t n8 = (size_t)B * S * heads * per_head;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const size_t bs = i / per_head / heads;
    const int s = (int)(bs % S), b = (int)(bs / S);
    const int pos = posb[b];
    if (s >= seq_tokens(pos, lenb[b], S, NP << psh)) {  // padding token
      if (hh < H) qo[(bs * H + hh) * per_head + c] = u32x4{0u, 0u, 0u, 0u};
      continue;
    }
    const u32x4 v = qkv[i];
    const int r = pos + s;
    const int pg = table[(size_t)b * NP + (r >> psh)];
    const bool ok = pg >= 0 && pg < P;
    const int prow = r & ((1 << psh) - 1);
    if (hh >= H + Hkv) {  // v: plain copy into the page row
      if (ok) vp[((((size_t)pg * Hkv + (hh - H - Hkv)) << psh) + prow) * per_head + c] = v;
      continue;
    }
    const float* cr = cosb + (size_t)r * (hd / 2) + c * 4;
    const float* sr = sinb + (size_t)r * (hd / 2) + c * 4;
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = bfl(v[e]), bb = bfh(v[e]), cs = cr[e], sn = sr[e];
      o[e] = pack2(a * cs - bb * sn, a * sn + bb * cs);
    }
    if (hh < H)
      qo[(bs * H + hh) * per_head + c] = o;
    else if (ok)
      kp[((((size_t)pg * Hkv + (hh - H)) << psh) + prow) * per_head + c] = o;
  }
}

// k_qkv_rope_cache_prefill_paged over an fp8 cache (kv8_codec.hpp): code pools
// kp / vp [P, Hkv, page, 128] of one byte per element and scales ksc / vsc
// [P, Hkv, page].  q as above.  A k row (after RoPE and the rounding of pack2,
// the row the bf16 kernel stores) or a v row is quantised by the 16 threads that
// hold it: 8 bytes of codes each, and thread 0 of the 16 stores the scale.
// Threads i .. i + 15 of a row are consecutive from a multiple of 16 (256, the
// grid stride and n8 are multiples of 16) and share (b, s, hh): they take the
// padding and dropped-write branches together and leave the loop together, so
// the shuffles of kv8_quant8 stay inside the group.  hd = 128 only.  Control flow and RoPE text are those of
// the bf16 _paged kernel, so that q and the k row round as they do there.
__global__ __launch_bounds__(256) void k_qkv_rope_cache_prefill_paged_kv8(
    const u32x4* __restrict__ qkv, const float* __restrict__ cosb, const float* __restrict__ sinb,
    const int* __restrict__ posb, const int* __restrict__ lenb, const int* __restrict__ table, u32x4* __restrict__ qo,
    u32x2* __restrict__ kp, u32x2* __restrict__ vp, float* __restrict__ ksc, float* __restrict__ vsc, int B, int S,
    int H, int Hkv, int NP, int P, int psh, int hd) {
  const int per_head = hd / 8, heads = H + 2 * Hkv;
  const size_t n8 = (size_t)B * S * heads * per_head;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const size_t bs = i / per_head / heads;
    const int s = (int)(bs % S), b = (int)(bs / S);
    const int pos = posb[b];
    if (s >= seq_tokens(pos, lenb[b], S, NP << psh)) {  // padding token
      if (hh < H) qo[(bs * H + hh) * per_head + c] = u32x4{0u, 0u, 0u, 0u};
      continue;
    }
    const u32x4 v = qkv[i];
    const int r = pos + s;
    const int pg = table[(size_t)b * NP + (r >> psh)];
    const bool ok = pg >= 0 && pg < P;
    const int prow = r & ((1 << psh) - 1);
    if (hh >= H + Hkv) {  // v: the raw row, quantised into the page row
      if (ok) kv8_store_row(v, vp, vsc, (((size_t)pg * Hkv + (hh - H - Hkv)) << psh) + prow, c);
      continue;
    }
    const float* cr = cosb + (size_t)r * (hd / 2) + c * 4;
    const float* sr = sinb + (size_t)r * (hd / 2) + c * 4;
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = bfl(v[e]), bb = bfh(v[e]), cs = cr[e], sn = sr[e];
      o[e] = pack2(a * cs - bb * sn, a * sn + bb * cs);
    }
    if (hh < H)
      qo[(bs * H + hh) * per_head + c] = o;
    else if (ok)
      kv8_store_row(o, kp, ksc, (((size_t)pg * Hkv + (hh - H)) << psh) + prow, c);
  }
}

constexpr int kHd = 128;
constexpr int kWaves = 8;
constexpr int kRows = kWaves * 32;  // query rows (token x head of the group) per workgroup
constexpr int kKT = 64;             // keys per tile
constexpr int kTileBytes = kKT * kHd * 2;

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// byte offset of 16-byte chunk ch of row r in a tile image
__device__ __forceinline__ int img_off(int r, int ch) { return 256 * r + 16 * (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))); }

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// k_prefill_attn<G> and its per-sequence form k_prefill_attn_seq<G> are one
// source text compiled twice: the uniform kernel gets exactly the tokens it
// always had.
#define GPBS_SEQ 0
#include "prefill_attn_body.hpp"
#undef GPBS_SEQ
#define GPBS_SEQ 1
#include "prefill_attn_body.hpp"
#undef GPBS_SEQ
// third compilation: k_prefill_attn_paged<G>
#define GPBS_SEQ 2
#include "prefill_attn_body.hpp"
#undef GPBS_SEQ
// fourth compilation: k_prefill_attn_paged_kv8<G>
#define GPBS_SEQ 3
#include "prefill_attn_body.hpp"
#undef GPBS_SEQ

}  // namespace gpbs_pf

using namespace gpbs_pf;

extern "C" {

int gpbs_hip_qkv_rope_cache_prefill(const void* qkv, const float* cosb, const float* sinb, void* qo, void* kc,
                                    void* vc, int B, int S, int H, int Hkv, int C, int hd, int pos, hipStream_t s) {
  if (!qkv || !cosb || !sinb || !qo || !kc || !vc || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0 || C <= 0 || hd <= 0 ||
      hd % 8 || pos < 0 || (long long)pos + S > C)
    return -22;
  const size_t n8 = (size_t)B * S * (H + 2 * Hkv) * hd / 8;
  const int grid = (int)std::min<size_t>((n8 + 255) / 256, 8192);
  hipLaunchKernelGGL(k_qkv_rope_cache_prefill, dim3(grid), dim3(256), 0, s, (const u32x4*)qkv, cosb, sinb, (u32x4*)qo,
                     (u32x4*)kc, (u32x4*)vc, B, S, H, Hkv, C, hd, pos);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int gpbs_hip_prefill_attn(const void* q, const void* kc, const void* vc, void* out, int B, int S, int H, int Hkv, int C,
                          int hd, int pos, float scale, hipStream_t s) {
  if (!q || !kc || !vc || !out || hd != kHd || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0 || H % Hkv || C <= 0 ||
      pos < 0 || (long long)pos + S > C)
    return -22;
  const int G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return -22;
  const int tpw = kRows / G;
  const long long nwg = (long long)((S + tpw - 1) / tpw) * B * Hkv;
  if (nwg > INT_MAX) return -22;
  const dim3 grid((unsigned)nwg), block(kWaves * 64);
  const float sl = scale * 1.44269504088896340736f;
#define GPBS_PF_LAUNCH(g)                                                                                        \
  hipLaunchKernelGGL(k_prefill_attn<g>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kc, (const u32x4*)vc, \
                     (u32x2*)out, S, Hkv, C, pos, sl, B * Hkv)
  switch (G) {
    case 1: GPBS_PF_LAUNCH(1); break;
    case 2: GPBS_PF_LAUNCH(2); break;
    case 4: GPBS_PF_LAUNCH(4); break;
    default: GPBS_PF_LAUNCH(8); break;
  }
#undef GPBS_PF_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int gpbs_hip_qkv_rope_cache_prefill_seq(const void* qkv, const float* cosb, const float* sinb, const int* posb,
                                        const int* lenb, void* qo, void* kc, void* vc, int B, int S, int H, int Hkv,
                                        int C, int hd, hipStream_t s) {
  if (!qkv || !cosb || !sinb || !posb || !lenb || !qo || !kc || !vc || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0 ||
      C <= 0 || hd <= 0 || hd % 8)
    return -22;
  const size_t n8 = (size_t)B * S * (H + 2 * Hkv) * hd / 8;
  const int grid = (int)std::min<size_t>((n8 + 255) / 256, 8192);
  hipLaunchKernelGGL(k_qkv_rope_cache_prefill_seq, dim3(grid), dim3(256), 0, s, (const u32x4*)qkv, cosb, sinb, posb,
                     lenb, (u32x4*)qo, (u32x4*)kc, (u32x4*)vc, B, S, H, Hkv, C, hd);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// out must come in zeroed: rows s >= n_b are left as they are
int gpbs_hip_prefill_attn_seq(const void* q, const void* kc, const void* vc, const int* posb, const int* lenb,
                              void* out, int B, int S, int H, int Hkv, int C, int hd, float scale, hipStream_t s) {
  if (!q || !kc || !vc || !posb || !lenb || !out || hd != kHd || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0 ||
      H % Hkv || C <= 0)
    return -22;
  const int G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return -22;
  const int tpw = kRows / G;
  const long long nwg = (long long)((S + tpw - 1) / tpw) * B * Hkv;
  if (nwg > INT_MAX) return -22;
  const dim3 grid((unsigned)nwg), block(kWaves * 64);
  const float sl = scale * 1.44269504088896340736f;
#define GPBS_PF_SEQ_LAUNCH(g)                                                                                        \
  hipLaunchKernelGGL(k_prefill_attn_seq<g>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kc, (const u32x4*)vc, \
                     posb, lenb, (u32x2*)out, S, Hkv, C, sl, B * Hkv)
  switch (G) {
    case 1: GPBS_PF_SEQ_LAUNCH(1); break;
    case 2: GPBS_PF_SEQ_LAUNCH(2); break;
    case 4: GPBS_PF_SEQ_LAUNCH(4); break;
    default: GPBS_PF_SEQ_LAUNCH(8); break;
  }
#undef GPBS_PF_SEQ_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// log2(page) for the page sizes the paged kernels take, -1 otherwise
static int page_shift(int page) { return page == 64 ? 6 : page == 128 ? 7 : page == 256 ? 8 : -1; }

int gpbs_hip_qkv_rope_cache_prefill_paged(const void* qkv, const float* cosb, const float* sinb, const int* posb,
                                          const int* lenb, const int* table, void* qo, void* kp, void* vp, int B,
                                          int S, int H, int Hkv, int NP, int P, int page, int hd, hipStream_t s) {
  const int psh = page_shift(page);
  if (!qkv || !cosb || !sinb || !posb || !lenb || !table || !qo || !kp || !vp || B <= 0 || S <= 0 || H <= 0 ||
      Hkv <= 0 || NP < 1 || P < 1 || psh < 0 || hd != kHd || ((long long)NP << psh) > INT_MAX)
    return -22;
  const size_t n8 = (size_t)B * S * (H + 2 * Hkv) * hd / 8;
  const int grid = (int)std::min<size_t>((n8 + 255) / 256, 8192);
  hipLaunchKernelGGL(k_qkv_rope_cache_prefill_paged, dim3(grid), dim3(256), 0, s, (const u32x4*)qkv, cosb, sinb, posb,
                     lenb, table, (u32x4*)qo, (u32x4*)kp, (u32x4*)vp, B, S, H, Hkv, NP, P, psh, hd);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// out must come in zeroed: rows s >= n_b are left as they are
int gpbs_hip_prefill_attn_paged(const void* q, const void* kp, const void* vp, const int* posb, const int* lenb,
                                const int* table, void* out, int B, int S, int H, int Hkv, int NP, int P, int page,
                                int hd, float scale, hipStream_t s) {
  const int psh = page_shift(page);
  if (!q || !kp || !vp || !posb || !lenb || !table || !out || hd != kHd || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0 ||
      H % Hkv || NP < 1 || P < 1 || psh < 0 || ((long long)NP << psh) > INT_MAX)
    return -22;
  const int G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return -22;
  const int tpw = kRows / G;
  const long long nwg = (long long)((S + tpw - 1) / tpw) * B * Hkv;
  if (nwg > INT_MAX) return -22;
  const dim3 grid((unsigned)nwg), block(kWaves * 64);
  const float sl = scale * 1.44269504088896340736f;
#define GPBS_PF_PAGED_LAUNCH(g)                                                                                        \
  hipLaunchKernelGGL(k_prefill_attn_paged<g>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kp, (const u32x4*)vp, \
                     posb, lenb, table, (u32x2*)out, S, Hkv, NP, P, psh, sl, B * Hkv)
  switch (G) {
    case 1: GPBS_PF_PAGED_LAUNCH(1); break;
    case 2: GPBS_PF_PAGED_LAUNCH(2); break;
    case 4: GPBS_PF_PAGED_LAUNCH(4); break;
    default: GPBS_PF_PAGED_LAUNCH(8); break;
  }
#undef GPBS_PF_PAGED_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// the paged entry points over an fp8 cache: e4m3 code pools kp / vp [P, Hkv, page, 128] and fp32 scales
// ksc / vsc [P, Hkv, page]
int gpbs_hip_qkv_rope_cache_prefill_paged_kv8(const void* qkv, const float* cosb, const float* sinb, const int* posb,
                                              const int* lenb, const int* table, void* qo, void* kp, void* vp,
                                              float* ksc, float* vsc, int B, int S, int H, int Hkv, int NP, int P,
                                              int page, int hd, hipStream_t s) {
  const int psh = page_shift(page);
  if (!qkv || !cosb || !sinb || !posb || !lenb || !table || !qo || !kp || !vp || !ksc || !vsc || B <= 0 || S <= 0 ||
      H <= 0 || Hkv <= 0 || NP < 1 || P < 1 || psh < 0 || hd != kHd || ((long long)NP << psh) > INT_MAX)
    return -22;
  const size_t n8 = (size_t)B * S * (H + 2 * Hkv) * hd / 8;
  const int grid = (int)std::min<size_t>((n8 + 255) / 256, 8192);
  hipLaunchKernelGGL(k_qkv_rope_cache_prefill_paged_kv8, dim3(grid), dim3(256), 0, s, (const u32x4*)qkv, cosb, sinb,
                     posb, lenb, table, (u32x4*)qo, (u32x2*)kp, (u32x2*)vp, ksc, vsc, B, S, H, Hkv, NP, P, psh, hd);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// out must come in zeroed: rows s >= n_b are left as they are
int gpbs_hip_prefill_attn_paged_kv8(const void* q, const void* kp, const void* vp, const float* ksc, const float* vsc,
                                    const int* posb, const int* lenb, const int* table, void* out, int B, int S, int H,
                                    int Hkv, int NP, int P, int page, int hd, float scale, hipStream_t s) {
  const int psh = page_shift(page);
  if (!q || !kp || !vp || !ksc || !vsc || !posb || !lenb || !table || !out || hd != kHd || B <= 0 || S <= 0 ||
      H <= 0 || Hkv <= 0 || H % Hkv || NP < 1 || P < 1 || psh < 0 || ((long long)NP << psh) > INT_MAX)
    return -22;
  const int G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return -22;
  const int tpw = kRows / G;
  const long long nwg = (long long)((S + tpw - 1) / tpw) * B * Hkv;
  if (nwg > INT_MAX) return -22;
  const dim3 grid((unsigned)nwg), block(kWaves * 64);
  const float sl = scale * 1.44269504088896340736f;
#define GPBS_PF_KV8_LAUNCH(g)                                                                                  \
  hipLaunchKernelGGL(k_prefill_attn_paged_kv8<g>, grid, block, 0, s, (const u32x4*)q, (const u32x2*)kp,       \
                     (const u32x2*)vp, ksc, vsc, posb, lenb, table, (u32x2*)out, S, Hkv, NP, P, psh, sl, B * Hkv)
  switch (G) {
    case 1: GPBS_PF_KV8_LAUNCH(1); break;
    case 2: GPBS_PF_KV8_LAUNCH(2); break;
    case 4: GPBS_PF_KV8_LAUNCH(4); break;
    default: GPBS_PF_KV8_LAUNCH(8); break;
  }
#undef GPBS_PF_KV8_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
