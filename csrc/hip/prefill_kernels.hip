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
// Each kernel exists in four forms, one per KV-cache view of attn_cache.hpp:
// the plain names take DenseUniform (S and pos are kernel arguments), _seq
// DenseSeq, _paged Paged and _paged_kv8 PagedKv8.  A write kernel is a wrapper
// that builds its view from its own parameters and calls the one template; the
// attention kernels share their text by inclusion (see below).
//
// The per-sequence forms take a position and a length per sequence (int32 [B]
// each): sequence b contributes n_b = min(len[b], S, C - pos[b]) tokens at cache
// rows pos[b] .. pos[b] + n_b - 1, or none if pos[b] is outside [0, C) or
// len[b] <= 0 (seq_tokens; C is Cl = NP * page over a paged view).  The launch is
// sized for S; tokens s >= n_b are padding: they write no cache row, their q /
// out rows are zero, and no q row >= n_b or cache row past pos[b] + n_b - 1 is
// addressed; of a block table only the entries of pages that hold rows
// 0 .. pos[b] + n_b - 1 are read.  The tile walk of a workgroup depends on its
// sequence alone, so sequence b gets the bits of the uniform kernel run on it
// alone with (S = n_b, pos = pos[b]).
#include "attn_entry.hpp"

namespace gpbs_pf {

using namespace gpbs_hip;

// The write kernel over cache view cv (the S-token form of gpbs_dec::qkv_rope_cache):
// token s of sequence b gets q with RoPE and its k (with RoPE) and v row stored at
// cache row pos + s; a padding token (s >= cv.tokens) touches neither cache nor
// RoPE table and gets a zero q row.  The uniform view has no padding, takes pos
// from the host and any hd % 8 == 0; the paged views take hd = 128 only.
// Fp8Rows::store: threads i .. i + 15 of a row are consecutive from a multiple of
// 16 (kWriteThreads, the grid stride and n8 are multiples of 16) and share (b, s, hh): they
// take the padding and dropped-write branches together and leave the loop
// together, so the shuffles of kv8_quant8 stay inside the group.
// Launch with kWriteThreads threads a workgroup only (launch_write): the loop strides by that constant.
template <class View>
__device__ __forceinline__ void qkv_rope_cache_prefill(const View cv, const u32x4* qkv, const float* cosb,
                                                       const float* sinb, const int* posb, const int* lenb,
                                                       const int* table, u32x4* qo, typename View::Piece* kc,
                                                       typename View::Piece* vc, float* ksc, float* vsc, int B, int S,
                                                       int H, int Hkv, int hd, int pos0) {
  const int per_head = hd / 8, heads = H + 2 * Hkv;
  const size_t n8 = (size_t)B * S * heads * per_head;
  for (size_t i = (size_t)blockIdx.x * kWriteThreads + threadIdx.x; i < n8; i += (size_t)gridDim.x * kWriteThreads) {
    const int c = (int)(i % per_head);
    const int hh = (int)((i / per_head) % heads);
    const size_t bs = i / per_head / heads;
    const int s = (int)(bs % S), b = (int)(bs / S);
    int pos = pos0;  // the host's position; a per-sequence view reads its own
    if constexpr (View::kPerSeq) {
      pos = posb[b];
      if (s >= cv.tokens(pos, lenb[b], S)) {  // padding token
        if (hh < H) qo[(bs * H + hh) * per_head + c] = u32x4{0u, 0u, 0u, 0u};
        continue;
      }
    }
    const u32x4 v = qkv[i];
    const int r = pos + s;
    const typename View::Where w = cv.locate(table, b, pos, s);
    if (hh >= H + Hkv) {  // v: the raw row into the cache row
      if (w.ok) View::store(v, vc, vsc, cv.row(w, Hkv, hh - H - Hkv), c, per_head);
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
    else if (w.ok)  // k: after RoPE and the rounding of pack2
      View::store(o, kc, ksc, cv.row(w, Hkv, hh - H), c, per_head);
  }
}

__global__ __launch_bounds__(kWriteThreads) void k_qkv_rope_cache_prefill(const u32x4* __restrict__ qkv,
                                                                const float* __restrict__ cosb,
                                                                const float* __restrict__ sinb,
                                                                u32x4* __restrict__ qo, u32x4* __restrict__ kc,
                                                                u32x4* __restrict__ vc, int B, int S, int H, int Hkv,
                                                                int C, int hd, int pos) {
  qkv_rope_cache_prefill(DenseUniform(C), qkv, cosb, sinb, nullptr, nullptr, nullptr, qo, kc, vc, nullptr, nullptr, B,
                         S, H, Hkv, hd, pos);
}

__global__ __launch_bounds__(kWriteThreads) void k_qkv_rope_cache_prefill_seq(const u32x4* __restrict__ qkv,
                                                                    const float* __restrict__ cosb,
                                                                    const float* __restrict__ sinb,
                                                                    const int* __restrict__ posb,
                                                                    const int* __restrict__ lenb,
                                                                    u32x4* __restrict__ qo, u32x4* __restrict__ kc,
                                                                    u32x4* __restrict__ vc, int B, int S, int H,
                                                                    int Hkv, int C, int hd) {
  qkv_rope_cache_prefill(DenseSeq(C), qkv, cosb, sinb, posb, lenb, nullptr, qo, kc, vc, nullptr, nullptr, B, S, H, Hkv,
                         hd, 0);
}

__global__ __launch_bounds__(kWriteThreads) void k_qkv_rope_cache_prefill_paged(const u32x4* __restrict__ qkv,
                                                                      const float* __restrict__ cosb,
                                                                      const float* __restrict__ sinb,
                                                                      const int* __restrict__ posb,
                                                                      const int* __restrict__ lenb,
                                                                      const int* __restrict__ table,
                                                                      u32x4* __restrict__ qo, u32x4* __restrict__ kp,
                                                                      u32x4* __restrict__ vp, int B, int S, int H,
                                                                      int Hkv, int NP, int P, int psh, int hd) {
  qkv_rope_cache_prefill(Paged(NP, P, psh), qkv, cosb, sinb, posb, lenb, table, qo, kp, vp, nullptr, nullptr, B, S, H,
                         Hkv, hd, 0);
}

__global__ __launch_bounds__(kWriteThreads) void k_qkv_rope_cache_prefill_paged_kv8(
    const u32x4* __restrict__ qkv, const float* __restrict__ cosb, const float* __restrict__ sinb,
    const int* __restrict__ posb, const int* __restrict__ lenb, const int* __restrict__ table, u32x4* __restrict__ qo,
    u32x2* __restrict__ kp, u32x2* __restrict__ vp, float* __restrict__ ksc, float* __restrict__ vsc, int B, int S,
    int H, int Hkv, int NP, int P, int psh, int hd) {
  qkv_rope_cache_prefill(PagedKv8(NP, P, psh), qkv, cosb, sinb, posb, lenb, table, qo, kp, vp, ksc, vsc, B, S, H, Hkv,
                         hd, 0);
}

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

// The attention kernel is not a template over a view: prefill_attn_body.hpp is
// its text, included once per cache form.  As a function template called from
// four wrappers the same text gave the same bits at the same speed but three
// more VGPRs in every instantiation (the compiler simplifies an inlined callee
// twice); only text compiled in the kernel itself keeps the instructions these
// kernels always had.  GPBS_SEQ: 0 DenseUniform (k_prefill_attn), 1 DenseSeq
// (k_prefill_attn_seq), 2 Paged (k_prefill_attn_paged), 3 PagedKv8
// (k_prefill_attn_paged_kv8).
#define GPBS_SEQ 0
#include "prefill_attn_body.hpp"
#undef GPBS_SEQ
#define GPBS_SEQ 1
#include "prefill_attn_body.hpp"
#undef GPBS_SEQ
#define GPBS_SEQ 2
#include "prefill_attn_body.hpp"
#undef GPBS_SEQ
#define GPBS_SEQ 3
#include "prefill_attn_body.hpp"
#undef GPBS_SEQ

}  // namespace gpbs_pf

using namespace gpbs_pf;

namespace {

// what the uniform entry points refuse of their host-side position
bool bad_pos(int pos, int S, int C) { return pos < 0 || (long long)pos + S > C; }

// pieces of 16 bytes in the packed qkv rows of a launch
size_t qkv_pieces(int B, int S, int H, int Hkv, int hd) { return (size_t)B * S * (H + 2 * Hkv) * hd / 8; }

// what every prefill attention entry point refuses, whatever the cache
bool bad_attn(int B, int S, int H, int Hkv, int hd) {
  return hd != kHd || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0 || H % Hkv;
}

// an attention kernel for G = H / Hkv in {1, 2, 4, 8}: launch(g, grid, block, sl) with
// g = std::integral_constant<int, G> and sl the softmax scale in the log2 domain
template <class Launch>
int launch_attn(int B, int S, int H, int Hkv, float scale, Launch launch) {
  const int G = H / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return -22;
  const int tpw = kRows / G;
  const long long nwg = (long long)((S + tpw - 1) / tpw) * B * Hkv;
  if (nwg > INT_MAX) return -22;
  const dim3 grid((unsigned)nwg), block(kWaves * 64);
  const float sl = scale * 1.44269504088896340736f;
  for_group(G, [&](auto g) { launch(g, grid, block, sl); });
  return launched();
}

}  // namespace

extern "C" {

int gpbs_hip_qkv_rope_cache_prefill(const void* qkv, const float* cosb, const float* sinb, void* qo, void* kc,
                                    void* vc, int B, int S, int H, int Hkv, int C, int hd, int pos, hipStream_t s) {
  if (any_null({qkv, cosb, sinb, qo, kc, vc}) || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0 || C <= 0 || hd <= 0 ||
      hd % 8 || bad_pos(pos, S, C))
    return -22;
  return launch_write(k_qkv_rope_cache_prefill, qkv_pieces(B, S, H, Hkv, hd), 8192, s,
                      (const u32x4*)qkv, cosb, sinb, (u32x4*)qo,
                      (u32x4*)kc, (u32x4*)vc, B, S, H, Hkv, C, hd, pos);
}

int gpbs_hip_prefill_attn(const void* q, const void* kc, const void* vc, void* out, int B, int S, int H, int Hkv, int C,
                          int hd, int pos, float scale, hipStream_t s) {
  if (any_null({q, kc, vc, out}) || bad_attn(B, S, H, Hkv, hd) || C <= 0 || bad_pos(pos, S, C)) return -22;
  return launch_attn(B, S, H, Hkv, scale, [&](auto g, dim3 grid, dim3 block, float sl) {
    hipLaunchKernelGGL(k_prefill_attn<decltype(g)::value>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kc,
                       (const u32x4*)vc, (u32x2*)out, S, Hkv, C, pos, sl, B * Hkv);
  });
}

int gpbs_hip_qkv_rope_cache_prefill_seq(const void* qkv, const float* cosb, const float* sinb, const int* posb,
                                        const int* lenb, void* qo, void* kc, void* vc, int B, int S, int H, int Hkv,
                                        int C, int hd, hipStream_t s) {
  if (any_null({qkv, cosb, sinb, posb, lenb, qo, kc, vc}) || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0 || C <= 0 ||
      hd <= 0 || hd % 8)
    return -22;
  return launch_write(k_qkv_rope_cache_prefill_seq, qkv_pieces(B, S, H, Hkv, hd), 8192, s,
                      (const u32x4*)qkv, cosb, sinb, posb, lenb,
                      (u32x4*)qo, (u32x4*)kc, (u32x4*)vc, B, S, H, Hkv, C, hd);
}

// out must come in zeroed: rows s >= n_b are left as they are
int gpbs_hip_prefill_attn_seq(const void* q, const void* kc, const void* vc, const int* posb, const int* lenb,
                              void* out, int B, int S, int H, int Hkv, int C, int hd, float scale, hipStream_t s) {
  if (any_null({q, kc, vc, posb, lenb, out}) || bad_attn(B, S, H, Hkv, hd) || C <= 0) return -22;
  return launch_attn(B, S, H, Hkv, scale, [&](auto g, dim3 grid, dim3 block, float sl) {
    hipLaunchKernelGGL(k_prefill_attn_seq<decltype(g)::value>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kc,
                       (const u32x4*)vc, posb, lenb, (u32x2*)out, S, Hkv, C, sl, B * Hkv);
  });
}

int gpbs_hip_qkv_rope_cache_prefill_paged(const void* qkv, const float* cosb, const float* sinb, const int* posb,
                                          const int* lenb, const int* table, void* qo, void* kp, void* vp, int B,
                                          int S, int H, int Hkv, int NP, int P, int page, int hd, hipStream_t s) {
  const int psh = page_shift(page);
  if (any_null({qkv, cosb, sinb, posb, lenb, table, qo, kp, vp}) || B <= 0 || S <= 0 || H <= 0 || Hkv <= 0 ||
      bad_pages(NP, P, psh) || hd != kHd)
    return -22;
  return launch_write(k_qkv_rope_cache_prefill_paged, qkv_pieces(B, S, H, Hkv, hd), 8192, s,
                      (const u32x4*)qkv, cosb, sinb, posb, lenb,
                      table, (u32x4*)qo, (u32x4*)kp, (u32x4*)vp, B, S, H, Hkv, NP, P, psh, hd);
}

// out must come in zeroed: rows s >= n_b are left as they are
int gpbs_hip_prefill_attn_paged(const void* q, const void* kp, const void* vp, const int* posb, const int* lenb,
                                const int* table, void* out, int B, int S, int H, int Hkv, int NP, int P, int page,
                                int hd, float scale, hipStream_t s) {
  const int psh = page_shift(page);
  if (any_null({q, kp, vp, posb, lenb, table, out}) || bad_attn(B, S, H, Hkv, hd) || bad_pages(NP, P, psh)) return -22;
  return launch_attn(B, S, H, Hkv, scale, [&](auto g, dim3 grid, dim3 block, float sl) {
    hipLaunchKernelGGL(k_prefill_attn_paged<decltype(g)::value>, grid, block, 0, s, (const u32x4*)q, (const u32x4*)kp,
                       (const u32x4*)vp, posb, lenb, table, (u32x2*)out, S, Hkv, NP, P, psh, sl, B * Hkv);
  });
}

// the paged entry points over an fp8 cache: e4m3 code pools kp / vp [P, Hkv, page, 128] and fp32 scales
// ksc / vsc [P, Hkv, page]
int gpbs_hip_qkv_rope_cache_prefill_paged_kv8(const void* qkv, const float* cosb, const float* sinb, const int* posb,
                                              const int* lenb, const int* table, void* qo, void* kp, void* vp,
                                              float* ksc, float* vsc, int B, int S, int H, int Hkv, int NP, int P,
                                              int page, int hd, hipStream_t s) {
  const int psh = page_shift(page);
  if (any_null({qkv, cosb, sinb, posb, lenb, table, qo, kp, vp, ksc, vsc}) || B <= 0 || S <= 0 || H <= 0 ||
      Hkv <= 0 || bad_pages(NP, P, psh) || hd != kHd)
    return -22;
  return launch_write(k_qkv_rope_cache_prefill_paged_kv8, qkv_pieces(B, S, H, Hkv, hd), 8192, s,
                      (const u32x4*)qkv, cosb, sinb, posb,
                      lenb, table, (u32x4*)qo, (u32x2*)kp, (u32x2*)vp, ksc, vsc, B, S, H, Hkv, NP, P, psh, hd);
}

// out must come in zeroed: rows s >= n_b are left as they are
int gpbs_hip_prefill_attn_paged_kv8(const void* q, const void* kp, const void* vp, const float* ksc, const float* vsc,
                                    const int* posb, const int* lenb, const int* table, void* out, int B, int S, int H,
                                    int Hkv, int NP, int P, int page, int hd, float scale, hipStream_t s) {
  const int psh = page_shift(page);
  if (any_null({q, kp, vp, ksc, vsc, posb, lenb, table, out}) || bad_attn(B, S, H, Hkv, hd) || bad_pages(NP, P, psh))
    return -22;
  return launch_attn(B, S, H, Hkv, scale, [&](auto g, dim3 grid, dim3 block, float sl) {
    hipLaunchKernelGGL(k_prefill_attn_paged_kv8<decltype(g)::value>, grid, block, 0, s, (const u32x4*)q,
                       (const u32x2*)kp, (const u32x2*)vp, ksc, vsc, posb, lenb, table, (u32x2*)out, S, Hkv, NP, P, psh,
                       sl, B * Hkv);
  });
}

}  // extern "C"
