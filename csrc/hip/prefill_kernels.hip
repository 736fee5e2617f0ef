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
#include <algorithm>
#include <climits>

#include "common.hpp"

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

// q [B, S, H, 128], caches [B, Hkv, C, 128], out [B, S, H * 128]; H = G * Hkv.
template <int G>
__global__ __launch_bounds__(kWaves * 64) void k_prefill_attn(const u32x4* __restrict__ q,
                                                              const u32x4* __restrict__ kc,
                                                              const u32x4* __restrict__ vc, u32x2* __restrict__ out,
                                                              int S, int Hkv, int C, int pos, float scale_log2e,
                                                              int nbh) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kTileBytes];  // K image, V image
  constexpr int TPW = kRows / G;  // tokens per workgroup (a multiple of 32)
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bh = blockIdx.x % nbh, qt = gridDim.x / nbh - 1 - blockIdx.x / nbh;  // heaviest query tiles first
  const int b = bh / Hkv, kvh = bh % Hkv, H = G * Hkv;
  const int q0 = qt * TPW;
  const int c = lane & 31, h = lane >> 5;
  const int g = (32 * w) / TPW, t0 = q0 + (32 * w) % TPW;  // the wave's head and first token
  const bool wave_on = t0 < S;
  const int s_raw = t0 + c;
  const int s = min(s_raw, S - 1);          // padding rows repeat token S - 1 and are not stored
  const int lim = pos + s;                  // last key this lane's query sees
  const int wave_kmin = pos + t0;           // smallest lim of the wave
  const int wave_kmax = pos + min(t0 + 31, S - 1);
  const int ntiles = (pos + min(q0 + TPW - 1, S - 1)) / kKT + 1;
  const int krow_last = pos + S - 1;        // <= C - 1: no address beyond it is formed

  bf16x8 qf[8];
  {
    const u32x4* qp = q + (((size_t)b * S + s) * H + kvh * G + g) * (kHd / 8) + h;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = __builtin_bit_cast(bf16x8, qp[2 * ks]);
  }

  // staging: piece i of this thread is chunk sch of tile row srow + 32 i
  const int srow = tid >> 4, sch = tid & 15;
  const size_t head = ((size_t)b * Hkv + kvh) * C;
  u32x4 kr[2], vr[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const size_t row = head + min(srow + 32 * i, krow_last);
    kr[i] = kc[row * (kHd / 8) + sch];
    vr[i] = vc[row * (kHd / 8) + sch];
  }

  // K row reads: row 32 kt + c, chunk 2 ks + h
  const int kx = ((c & 3) << 2) | ((c >> 2) & 3);
  // V transposed reads: lane 4 qq + p of a 16-lane group gives row qq, dims 4 p .. 4 p + 3 of the block
  const int gi = lane >> 4, qq = (lane >> 2) & 3, p = lane & 3;
  const int vcl = 2 * (gi & 1) + (p >> 1);  // chunk within the 32-dim tile dt
  int vbase[2], vx[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = 4 * h + 8 * u + qq;  // + 32 kt + 16 s2
    vbase[u] = kTileBytes + 256 * row + 8 * (p & 1);
    vx[u] = ((row & 3) << 2) | ((row >> 2) & 3);
  }

  f32x16 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();  // the previous tile's reads are done
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<u32x4*>(lds + img_off(srow + 32 * i, sch)) = kr[i];
      *reinterpret_cast<u32x4*>(lds + kTileBytes + img_off(srow + 32 * i, sch)) = vr[i];
    }
    __syncthreads();
    if (t + 1 < ntiles) {  // next tile in flight under this tile's MFMAs
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const size_t row = head + min((t + 1) * kKT + srow + 32 * i, krow_last);
        kr[i] = kc[row * (kHd / 8) + sch];
        vr[i] = vc[row * (kHd / 8) + sch];
      }
    }
    const int k0 = t * kKT;
    if (!wave_on || k0 > wave_kmax) continue;  // wave-uniform: tile wholly above this wave's diagonal

    f32x16 sc[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[kt][i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(lds + 256 * (32 * kt + c) + 16 * ((2 * ks + h) ^ kx));
        sc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[ks], sc[kt], 0, 0, 0);
      }
    }
    // scores in the log2 domain (a separate rounding: the max and the exponent see the same value)
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int i = 0; i < 16; ++i) sc[kt][i] = __fmul_rn(sc[kt][i], scale_log2e);
    if (k0 + kKT - 1 > wave_kmin) {  // the tile crosses the wave's diagonal
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = k0 + 32 * kt + (i & 3) + 8 * (i >> 2) + 4 * h;
          sc[kt][i] = key <= lim ? sc[kt][i] : -INFINITY;
        }
    }
    float tm = sc[0][0];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int i = 0; i < 16; ++i) tm = fmaxf(tm, sc[kt][i]);
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
    const float mn = fmaxf(m, tm);  // finite: key 0 is in the first tile and visible to every query
    const float corr = ex2(m - mn);
    m = mn;
    l *= corr;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[dt][i] *= corr;
    bf16x8 pb[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const __bf16 pv = (__bf16)ex2(sc[kt][i] - mn);
        pb[kt][i >> 3][i & 7] = pv;
        l += (float)pv;  // the value that multiplies V
      }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      int va[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) va[u] = vbase[u] + 16 * ((4 * dt + vcl) ^ vx[u]);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const int add = 256 * (32 * kt + 16 * s2);
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + va[0] + add));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + va[1] + add));
          const s16x8 a8 = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a8), pb[kt][s2], o[dt], 0, 0, 0);
        }
    }
  }

  if (!wave_on) return;
  l += __shfl_xor(l, 32, 64);
  if (s_raw >= S) return;
  const float inv = 1.f / l;
  u32x2* op = out + (((size_t)b * S + s) * H + kvh * G + g) * (kHd / 4) + h;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // dims 32 dt + 8 j + 4 h .. + 3
      u32x2 v;
      v[0] = pack2(o[dt][4 * j] * inv, o[dt][4 * j + 1] * inv);
      v[1] = pack2(o[dt][4 * j + 2] * inv, o[dt][4 * j + 3] * inv);
      op[8 * dt + 2 * j] = v;
    }
}

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

}  // extern "C"
