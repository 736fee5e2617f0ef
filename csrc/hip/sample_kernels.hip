// Token sampling for the Llama tenant on gfx950: temperature, top-k and top-p per row, one token per row.
//
// The sampler is defined in integers (pbs_amd/ops/llm.py, "token sampling"): every logit becomes a weight in
// [0, 2^30] by fp32 steps of one rounding each, and everything after that -- the top-k and top-p thresholds, the sums,
// the draw -- is integer arithmetic, the same in any order of summation.  The kernel therefore returns the token and
// the stats row of llm.sample_ref bit for bit.
//
// One workgroup of up to 1024 threads per row.  A row of 128256 bf16 logits (250 KiB) does not fit the LDS, so every
// pass re-reads it (16 bytes per lane, from L2 after the first pass) and recomputes the weights:
//   1. row maximum (greedy rows: the lowest index of it, and done);
//   2. threshold t: a radix select over the 31-bit weights, most significant byte first, on an LDS histogram of
//      (count, mass) per bin -- by count for top-k, then by mass for top-p; only the active selects run, and a row
//      with neither sums its weights in one pass;
//   3. tile-wise prefix scan of the kept weights in index order with a carry, until the tile that crosses r.
#include "common.hpp"

namespace gpbs_hip {

constexpr int kSampleThreads = 1024;
constexpr int kSampleWaves = kSampleThreads / 64;

// c0 .. c5 of SAMPLE_EXP2_COEF and fp32(log2 e) of SAMPLE_LOG2E (pbs_amd/ops/llm.py)
constexpr float kC0 = 0x1.62e42cp-1f, kC1 = 0x1.ebfd5ap-3f, kC2 = 0x1.c688f0p-5f, kC3 = 0x1.3d0c40p-7f,
                kC4 = 0x1.46d326p-10f, kC5 = 0x1.c54640p-13f, kLog2e = 0x1.715476p+0f;

// The weight of one logit: every step one fp32 rounding.  The pragma keeps the compiler from contracting a
// multiply and the add after it into a fused multiply-add (one rounding where the contract has two).
__device__ __forceinline__ u32 sample_weight(float x, float m, float it) {
#pragma clang fp contract(off)
  float y = ((x - m) * it) * kLog2e;
  y = fmaxf(y, -64.0f);
  const float n = floorf(y);
  const float f = y - n;
  float p = f * kC5;
  p = f * (p + kC4);
  p = f * (p + kC3);
  p = f * (p + kC2);
  p = f * (p + kC1);
  p = f * (p + kC0);
  p = p + 1.0f;
  const u32 q = (u32)(p * 0x1p30f);  // p in [1, 2]: exact product, truncation is the floor
  const int sh = (int)(-n);                  // 0 .. 64
  return sh >= 32 ? 0u : q >> sh;
}

__device__ __forceinline__ void unpack8(const u32x4 v, float* x) {
  x[0] = bfl(v.x); x[1] = bfh(v.x); x[2] = bfl(v.y); x[3] = bfh(v.y);
  x[4] = bfl(v.z); x[5] = bfh(v.z); x[6] = bfl(v.w); x[7] = bfh(v.w);
}

__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
  const u32 lo = __shfl_up((u32)v, d), hi = __shfl_up((u32)(v >> 32), d);
  return (u64)lo | ((u64)hi << 32);
}
__device__ __forceinline__ u64 shfl_xor64(u64 v, int d) {
  const u32 lo = __shfl_xor((u32)v, d), hi = __shfl_xor((u32)(v >> 32), d);
  return (u64)lo | ((u64)hi << 32);
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += shfl_xor64(v, d);
  return v;
}
__device__ __forceinline__ u32 wave_sum32(u32 v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ void philox_round(u32* c, const u32 k0, const u32 k1) {
  const u64 p0 = (u64)0xD2511F53u * c[0], p1 = (u64)0xCD9E8D57u * c[2];
  const u32 n0 = (u32)(p1 >> 32) ^ c[1] ^ k0, n2 = (u32)(p0 >> 32) ^ c[3] ^ k1;
  c[0] = n0; c[1] = (u32)p1; c[2] = n2; c[3] = (u32)p0;
}
// 64 bits of Philox4x32-10: counter (ctr, 0, 0, 0), key (low, high word of seed); out[0] + 2^32 out[1]
__device__ __forceinline__ u64 philox_u64(u32 ctr, u64 seed) {
  u32 c[4] = {ctr, 0u, 0u, 0u};
  u32 k0 = (u32)seed, k1 = (u32)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return (u64)c[0] | ((u64)c[1] << 32);
}

struct SampleShared {
  u64 mass[256];
  u32 cnt[256];
  u64 wsum[kSampleWaves];
  float wmax[kSampleWaves];
  u32 widx[kSampleWaves];
  // the result of a select step / the scan, written by one thread and read by all
  u32 digit, digit_cnt, above_cnt;
  u64 digit_mass, above_mass;
  int found;
};

// One radix step: histogram of byte `shift / 8` over the weights whose bits above it equal those of `prefix`, then
// the highest digit d at which the count (by_mass: the mass) of the digits >= d reaches `need`.  Leaves in sh:
// digit, the count / mass of the digit itself and of the digits above it.  Digit 0 collects most weights (they
// are small against the maximum), so every thread sums it in registers and the waves add it once.
__device__ __forceinline__ void select_step(SampleShared& sh, const u32x4* row, int chunks, float m, float it,
                                            u32 prefix, int shift, bool by_mass, u64 need) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int i = tid; i < 256; i += nthr) { sh.mass[i] = 0; sh.cnt[i] = 0; }
  __syncthreads();
  const u32 himask = shift == 24 ? 0u : ~0u << (shift + 8);
  u32 c0 = 0;
  u64 m0 = 0;
  for (int c = tid; c < chunks; c += nthr) {
    float x[8];
    unpack8(row[c], x);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const u32 w = sample_weight(x[e], m, it);
      if ((w & himask) != prefix) continue;
      const u32 d = (w >> shift) & 255u;
      if (d == 0) {
        ++c0;
        m0 += w;
      } else {
        atomicAdd(&sh.cnt[d], 1u);
        atomicAdd(&sh.mass[d], (u64)w);
      }
    }
  }
  c0 = wave_sum32(c0);
  m0 = wave_sum64(m0);
  if ((tid & 63) == 0 && c0) {
    atomicAdd(&sh.cnt[0], c0);
    atomicAdd(&sh.mass[0], m0);
  }
  __syncthreads();
  if (tid < 64) {  // wave 0: lane l owns digits 255 - 4l .. 252 - 4l, scanned from the top
    u32 lc[4];
    u64 lm[4];
    u32 tc = 0;
    u64 tm = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lc[j] = sh.cnt[255 - 4 * tid - j];
      lm[j] = sh.mass[255 - 4 * tid - j];
      tc += lc[j];
      tm += lm[j];
    }
    u32 ic = tc;
    u64 im = tm;  // inclusive scan over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u32 oc = __shfl_up(ic, d);
      const u64 om = shfl_up64(im, d);
      if (tid >= d) { ic += oc; im += om; }
    }
    u32 ac = ic - tc;
    u64 am = im - tm;  // what lies above this lane's digits
    const u64 before = by_mass ? am : (u64)ac, after = by_mass ? im : (u64)ic;
    if (before < need && need <= after) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u64 with = (by_mass ? am + lm[j] : (u64)(ac + lc[j]));
        if (with >= need || j == 3) {
          sh.digit = 255 - 4 * tid - j;
          sh.digit_cnt = lc[j];
          sh.digit_mass = lm[j];
          sh.above_cnt = ac;
          sh.above_mass = am;
          break;
        }
        ac += lc[j];
        am += lm[j];
      }
    }
  }
  __syncthreads();
}

// The value v with: by count, the need-th largest weight; by mass, the largest v whose weights >= v sum to >= need.
// Returns v; cnt / mass are those of the weights > v and of the weights == v.  need is at least 1 and at most the
// count / mass of the whole row, so every step finds its digit.
__device__ __forceinline__ u32 radix_select(SampleShared& sh, const u32x4* row, int chunks, float m, float it,
                                            bool by_mass, u64 need, u32* cnt_gt, u64* mass_gt, u32* cnt_eq,
                                            u64* mass_eq) {
  u32 prefix = 0, cg = 0;
  u64 mg = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (threadIdx.x == 0) {  // defaults, should no lane find the crossing (it always does: see above)
      sh.digit = 0; sh.digit_cnt = 0; sh.digit_mass = 0; sh.above_cnt = 0; sh.above_mass = 0;
    }
    select_step(sh, row, chunks, m, it, prefix, shift, by_mass, need);
    prefix |= sh.digit << shift;
    cg += sh.above_cnt;
    mg += sh.above_mass;
    need -= by_mass ? sh.above_mass : (u64)sh.above_cnt;
    *cnt_eq = sh.digit_cnt;
    *mass_eq = sh.digit_mass;
    __syncthreads();  // sh is rewritten by the next step
  }
  *cnt_gt = cg;
  *mass_gt = mg;
  return prefix;
}

__global__ __launch_bounds__(kSampleThreads) void k_sample_rows(const u32x4* __restrict__ logits,
                                                                const float* __restrict__ inv_temp,
                                                                const int* __restrict__ top_k,
                                                                const float* __restrict__ top_p,
                                                                const long long* __restrict__ seed,
                                                                const int* __restrict__ ctr, long long* tokens,
                                                                long long* stats, int V) {
  __shared__ SampleShared sh;
  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
  const int nwaves = nthr >> 6;
  const int c_ctr = ctr[b];
  if (c_ctr < 0) {  // idle row
    if (tid == 0) tokens[b] = 0;
    if (tid < 4) stats[4 * b + tid] = 0;
    return;
  }
  const int chunks = V >> 3;
  const u32x4* row = logits + (size_t)b * chunks;
  const float it = inv_temp[b];

  // ---- 1. row maximum
  float m = -INFINITY;
  for (int c = tid; c < chunks; c += nthr) {
    float x[8];
    unpack8(row[c], x);
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, x[e]);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  if (lane == 0) sh.wmax[wave] = m;
  __syncthreads();
  m = sh.wmax[0];
  for (int w = 1; w < nwaves; ++w) m = fmaxf(m, sh.wmax[w]);

  if (it == 0.0f) {  // greedy: the lowest index of the maximum
    u32 idx = 0xffffffffu;
    for (int c = tid; c < chunks; c += nthr) {
      float x[8];
      unpack8(row[c], x);
#pragma unroll
      for (int e = 7; e >= 0; --e)
        if (x[e] == m) idx = min(idx, (u32)(8 * c + e));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) idx = min(idx, (u32)__shfl_xor(idx, d));
    if (lane == 0) sh.widx[wave] = idx;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < nwaves; ++w) idx = min(idx, sh.widx[w]);
      tokens[b] = idx;
    }
    if (tid < 4) stats[4 * b + tid] = 0;
    return;
  }

  // ---- 2. the threshold t, with cnt and S of the weights >= t
  const int k = top_k[b];
  const float tp = top_p[b];
  const bool k_on = k > 0 && k < V, p_on = tp < 1.0f;
  u32 t = 1, cnt;
  u64 S;
  if (k_on) {
    u32 cg, ce;
    u64 mg, me;
    const u32 v = radix_select(sh, row, chunks, m, it, false, (u64)k, &cg, &mg, &ce, &me);
    // v == 0: the k-th largest weight is zero, t stays 1 and the weights above it are the kept ones
    t = v > 1u ? v : 1u;
    cnt = v ? cg + ce : cg;
    S = mg + me;
  }
  if (!k_on) {  // t = 1: one pass for the sum and the number of the nonzero weights
    u32 c1 = 0;
    u64 s1 = 0;
    for (int c = tid; c < chunks; c += nthr) {
      float x[8];
      unpack8(row[c], x);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const u32 w = sample_weight(x[e], m, it);
        c1 += w != 0u;
        s1 += w;
      }
    }
    c1 = wave_sum32(c1);
    s1 = wave_sum64(s1);
    __syncthreads();  // sh.wsum / widx may still be read from an earlier use
    if (lane == 0) { sh.widx[wave] = c1; sh.wsum[wave] = s1; }
    __syncthreads();
    cnt = 0;
    S = 0;
    for (int w = 0; w < nwaves; ++w) { cnt += sh.widx[w]; S += sh.wsum[w]; }
    __syncthreads();
  }
  if (p_on) {
    float pf = floorf(tp * 65536.0f);  // exact: a power of two
    pf = fminf(fmaxf(pf, 0.0f), 65535.0f);
    const u64 P = (u64)pf;
    u64 target = (S >> 16) * P + (((S & 0xffffull) * P) >> 16);
    if (target < 1) target = 1;
    u32 cg, ce;
    u64 mg, me;
    t = radix_select(sh, row, chunks, m, it, true, target, &cg, &mg, &ce, &me);
    cnt = cg + ce;
    S = mg + me;
  }

  // ---- 3. the draw: r = floor(R S / 2^64), then the first index whose kept prefix sum exceeds r
  const u64 r = __umul64hi(philox_u64((u32)c_ctr, (u64)seed[b]), S);
  if (tid == 0) {
    stats[4 * b + 0] = (long long)t;
    stats[4 * b + 1] = (long long)cnt;
    stats[4 * b + 2] = (long long)S;
    stats[4 * b + 3] = (long long)r;
    sh.found = 0;
  }
  __syncthreads();
  u64 carry = 0;
  for (int base = 0; base < chunks; base += nthr) {  // block-uniform trip count
    const int c = base + tid;
    u32 w8[8];
    u64 mine = 0;
    if (c < chunks) {
      float x[8];
      unpack8(row[c], x);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const u32 w = sample_weight(x[e], m, it);
        w8[e] = w >= t ? w : 0u;
        mine += w8[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) w8[e] = 0u;
    }
    u64 inc = mine;  // inclusive scan in the wave, then over the waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 o = shfl_up64(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) sh.wsum[wave] = inc;
    __syncthreads();
    u64 before = carry, total = 0;
    for (int w = 0; w < nwaves; ++w) {
      const u64 s = sh.wsum[w];
      if (w < wave) before += s;
      total += s;
    }
    before += inc - mine;
    if (before <= r && r < before + mine) {  // exactly one thread of the row
      u64 acc = before;
      int e = 0;
#pragma unroll
      for (; e < 7; ++e) {
        acc += w8[e];
        if (acc > r) break;
      }
      tokens[b] = 8 * c + e;
      sh.found = 1;
    }
    carry += total;
    __syncthreads();
    if (sh.found) break;
  }
}

}  // namespace gpbs_hip

using namespace gpbs_hip;

extern "C" {

// logits bf16 [B, V] (V % 8 == 0, 8 <= V <= 2^20); inv_temp / top_p fp32 [B], top_k / ctr int32 [B], seed int64 [B];
// tokens int64 [B], stats int64 [B, 4].  All device pointers, read at run time.
int gpbs_hip_sample_rows(const void* logits, const void* inv_temp, const void* top_k, const void* top_p,
                         const void* seed, const void* ctr, void* tokens, void* stats, int B, int V, hipStream_t s) {
  if (B <= 0 || V < 8 || V > (1 << 20) || V % 8) return -22;
  if (!logits || !inv_temp || !top_k || !top_p || !seed || !ctr || !tokens || !stats) return -22;
  const int chunks = V / 8;
  int threads = ((chunks + 63) / 64) * 64;
  if (threads > kSampleThreads) threads = kSampleThreads;
  hipLaunchKernelGGL(k_sample_rows, dim3(B), dim3(threads), 0, s, (const u32x4*)logits, (const float*)inv_temp,
                     (const int*)top_k, (const float*)top_p, (const long long*)seed, (const int*)ctr,
                     (long long*)tokens, (long long*)stats, V);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
