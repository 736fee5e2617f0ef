// The decode attention kernel.  Not a header of its own:
// decode_kernels.hip includes this text four times, inside namespace gpbs_dec, with
// GPBS_SEQ 0 (k_decode_attn: one device position for
// the batch) and GPBS_SEQ 1 (k_decode_attn_seq: dpos
// is int32 [B]; sequence b has L = dpos[b] + 1 keys if 0 <= dpos[b] < C and is
// idle otherwise: L = 0, no key loop, zero output).  Everything outside the
// #if blocks is shared, so an active sequence gets the uniform kernel's bits.
// GPBS_SEQ 2 is a third compilation, k_decode_attn_paged: the _seq kernel over
// pools [P, Hkv, page, 128] addressed through an int32 block table [B, NP]
// (logical row r of sequence b: page table[b, r / page], page row r % page;
// Cl = NP * page stands where C stood).  A 64-key step never straddles a page,
// so the only new work is one wave-uniform table entry per step, loaded one
// step ahead; an entry outside [0, P) reads page 0.
// GPBS_SEQ 3 is a fourth compilation, k_decode_attn_paged_kv8: the paged kernel
// over e4m3 pools (one byte per element) with one power-of-two fp32 scale per
// (page, KV head, page row).  A lane's key row is 8 16-byte loads and its scale,
// the V piece of a (key, dl) 8 bytes and that key's scale; code times scale is
// exact and is a bf16 value, so kv8_words rebuilds the very words the dequantised
// bf16 pools hold, and everything from bfl / bfh on is shared text.
#if GPBS_SEQ == 3
#define GPBS_DEC_ATTN k_decode_attn_paged_kv8
#elif GPBS_SEQ == 2
#define GPBS_DEC_ATTN k_decode_attn_paged
#elif GPBS_SEQ
#define GPBS_DEC_ATTN k_decode_attn_seq
#else
#define GPBS_DEC_ATTN k_decode_attn
#endif

// q [B, H, 128], caches [B, Hkv, C, 128], out [B, H * 128]; H = G * Hkv.
template <int G>
__global__ __launch_bounds__(kAttnWaves * 64) void GPBS_DEC_ATTN(const u32x4* __restrict__ q,
                                                               const u32x4* __restrict__ kc,
#if GPBS_SEQ == 3
                                                               const u32x2* __restrict__ vc,
                                                               const float* __restrict__ ksc,
                                                               const float* __restrict__ vsc,
#else
                                                               const u32* __restrict__ vc,
#endif
#if GPBS_SEQ >= 2
                                                               const int* __restrict__ dpos,
                                                               const int* __restrict__ table, u32* __restrict__ out,
                                                               float* __restrict__ ws, int Hkv, int NP, int P, int psh,
                                                               float scale, int nsplit) {
  const int C = NP << psh;  // the logical context Cl
#else
                                                               const int* __restrict__ dpos, u32* __restrict__ out,
                                                               float* __restrict__ ws, int Hkv, int C, float scale,
                                                               int nsplit) {
#endif
  __shared__ float qs[G][kHd];
  __shared__ float ms[kAttnWaves][G], ls[kAttnWaves][G];
  __shared__ float os[kAttnWaves][G][kHd];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int split = blockIdx.x % nsplit, bh = blockIdx.x / nsplit;
  const int b = bh / Hkv, kvh = bh % Hkv;
#if GPBS_SEQ
  const int pb = dpos[b];
  const int L = (pb >= 0 && pb < C) ? pb + 1 : 0;  // keys 0..pos[b]; an idle slot has none
#else
  const int L = min(*dpos + 1, C);  // keys 0..pos
#endif
  // flash-decoding split: this workgroup takes keys [k0, k1) (64-aligned chunks)
  const int chunk = ((L + nsplit - 1) / nsplit + 63) & ~63;
  const int k0 = split * chunk, k1 = min(L, k0 + chunk);
  const int H = G * Hkv;
  // stage the group's queries (pre-scaled) in LDS: read as broadcasts below
  for (int e = threadIdx.x; e < G * kHd / 8; e += kAttnWaves * 64) {
    const int g = e / (kHd / 8), c = e % (kHd / 8);
    const u32x4 v = q[((size_t)b * H + kvh * G + g) * (kHd / 8) + c];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      qs[g][c * 8 + 2 * k] = bfl(v[k]) * scale;
      qs[g][c * 8 + 2 * k + 1] = bfh(v[k]) * scale;
    }
  }
  __syncthreads();
#if GPBS_SEQ >= 2
#if GPBS_SEQ == 3
  // the bases of KV head kvh in page 0: 128-byte rows of codes, one scale per row
  const u32x4* kh = kc + ((size_t)kvh << psh) * (kHd / 16);
  const u32x2* vh = vc + ((size_t)kvh << psh) * (kHd / 8);
  const float* ksh = ksc + ((size_t)kvh << psh);
  const float* vsh = vsc + ((size_t)kvh << psh);
#else
  // the bases of KV head kvh in page 0; a page is Hkv << psh rows further on
  const u32x4* kh = kc + ((size_t)kvh << psh) * (kHd / 8);
  const u32* vh = vc + ((size_t)kvh << psh) * (kHd / 2);
#endif
  const int* trow = table + (size_t)b * NP;
  const int base0 = __builtin_amdgcn_readfirstlane(k0 + w * 64);
  int pg = base0 < k1 ? page_or0(trow[base0 >> psh], P) : 0;  // the page of this wave's first step
#else
  const size_t head = (size_t)b * Hkv + kvh;
  const u32x4* kh = kc + head * C * (kHd / 8);
  const u32* vh = vc + head * C * (kHd / 2);
#endif
  // PV lane map: key group kg = lane >> 4 takes keys kg, kg + 4, ...; dl = lane & 15
  // owns dims 8 dl .. 8 dl + 7 (one 16-byte V load per key)
  const int kg = lane >> 4, dl = lane & 15;
  float m[G], l[G], o[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY, l[g] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[g][e] = 0.f;
  }

#if GPBS_SEQ >= 2
  for (int base = base0; base < k1; base += kAttnWaves * 64) {
    // rows of this step within the pools: page pg, page rows base % page ..; the
    // next step's entry (only if that step has keys) is in flight under this one
    const size_t prow = ((size_t)pg * Hkv << psh) + (base & ((1 << psh) - 1));
    if (base + kAttnWaves * 64 < k1) pg = page_or0(trow[(base + kAttnWaves * 64) >> psh], P);
#else
  for (int base = k0 + w * 64; base < k1; base += kAttnWaves * 64) {
#endif
    const int j = base + lane;
    float s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) s[g] = 0.f;
    // opaque zero: keeps the (loop-invariant) LDS query reads inside this loop, so
    // the compiler does not hoist G x 128 floats into registers and spill
    int z = 0;
    asm volatile("" : "+s"(z));
    const float* qz = &qs[0][0] + z;
    if (j < k1) {
#if GPBS_SEQ == 3
      const u32x4* kr = kh + (prow + lane) * (kHd / 16);
      u32x4 krow[kHd / 16];  // the lane's whole 128-byte key row in flight at once, and its scale
#pragma unroll
      for (int c = 0; c < kHd / 16; ++c) krow[c] = kr[c];
      const float ks = ksh[prow + lane];
#else
#if GPBS_SEQ == 2
      const u32x4* kr = kh + (prow + lane) * (kHd / 8);
#else
      const u32x4* kr = kh + (size_t)j * (kHd / 8);
#endif
      u32x4 krow[kHd / 8];  // the lane's whole 256-byte key row in flight at once
#pragma unroll
      for (int c = 0; c < kHd / 8; ++c) krow[c] = kr[c];
#endif
#pragma unroll
      for (int c = 0; c < kHd / 8; ++c) {
#if GPBS_SEQ == 3
        // dims 8 c .. 8 c + 7 are words 2 (c & 1), + 1 of the row's 16-byte piece c >> 1
        const u32x4 kv = kv8_words(u32x2{krow[c >> 1][2 * (c & 1)], krow[c >> 1][2 * (c & 1) + 1]}, ks);
#else
        const u32x4 kv = krow[c];
#endif
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float k0 = bfl(kv[k]), k1 = bfh(kv[k]);
#pragma unroll
          for (int g = 0; g < G; ++g) s[g] += qz[g * kHd + c * 8 + 2 * k] * k0 + qz[g * kHd + c * 8 + 2 * k + 1] * k1;
        }
      }
    }
    const int nk = min(64, k1 - base);
    float p[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float sg = j < k1 ? s[g] : -INFINITY;
      const float mn = fmaxf(m[g], wmax(sg));
      const float corr = __expf(m[g] - mn);
      p[g] = j < k1 ? __expf(sg - mn) : 0.f;
      l[g] = l[g] * corr + wsum(p[g]);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[g][e] *= corr;
      m[g] = mn;
    }
    // PV: 16 rounds of 4 keys (one per key group), 16-byte V loads, weights by shuffle
#if GPBS_SEQ == 3
    const u32x2* vb = vh + prow * (kHd / 8) + dl;
    const float* vsb = vsh + prow;
#elif GPBS_SEQ == 2
    const u32x4* vb = reinterpret_cast<const u32x4*>(vh) + prow * (kHd / 8) + dl;
#else
    const u32x4* vb = reinterpret_cast<const u32x4*>(vh) + (size_t)base * (kHd / 8) + dl;
#endif
#pragma unroll 4
    for (int t = 0; t < 16; ++t) {
      const int jj = 4 * t + kg;
      float pj[G];
#pragma unroll
      for (int g = 0; g < G; ++g) pj[g] = __shfl(p[g], jj, 64);
      if (jj < nk) {
#if GPBS_SEQ == 3
        const u32x4 vv = kv8_words(vb[(size_t)jj * (kHd / 8)], vsb[jj]);  // 8 codes: dims 8 dl .. 8 dl + 7
#else
        const u32x4 vv = vb[(size_t)jj * (kHd / 8)];
#endif
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v0 = bfl(vv[e]), v1 = bfh(vv[e]);
#pragma unroll
          for (int g = 0; g < G; ++g) {
            o[g][2 * e] += pj[g] * v0;
            o[g][2 * e + 1] += pj[g] * v1;
          }
        }
      }
    }
  }
  // sum the 4 key groups' partials (lanes dl, dl + 16, dl + 32, dl + 48)
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o[g][e] += __shfl_xor(o[g][e], 16, 64);
      o[g][e] += __shfl_xor(o[g][e], 32, 64);
    }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (kg == 0)
#pragma unroll
      for (int e = 0; e < 8; ++e) os[w][g][8 * dl + e] = o[g][e];
    if (lane == 0) ms[w][g] = m[g], ls[w][g] = l[g];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < G * 64; e += kAttnWaves * 64) {
    const int g = e / 64, d = 2 * (e % 64);
    float M = -INFINITY;
#pragma unroll
    for (int v = 0; v < kAttnWaves; ++v) M = fmaxf(M, ms[v][g]);
    float Ls = 0.f, a0 = 0.f, a1 = 0.f;
#pragma unroll
    for (int v = 0; v < kAttnWaves; ++v) {
      const float f = ms[v][g] == -INFINITY ? 0.f : __expf(ms[v][g] - M);
      Ls += ls[v][g] * f;
      a0 += os[v][g][d] * f;
      a1 += os[v][g][d + 1] * f;
    }
    if (nsplit == 1) {
#if GPBS_SEQ
      const float inv = Ls == 0.f ? 0.f : 1.f / Ls;  // idle: zero bits, not 0 * inf
#else
      const float inv = 1.f / Ls;
#endif
      out[((size_t)b * H + kvh * G + g) * (kHd / 2) + d / 2] = pack2(a0 * inv, a1 * inv);
    } else {  // partial (max, sum, unnormalised o) for k_decode_attn_combine
      float* p = ws + ((size_t)blockIdx.x * G + g) * (kHd + 2);
      p[d] = a0;
      p[d + 1] = a1;
      if (d == 0) p[kHd] = M, p[kHd + 1] = Ls;
    }
  }
}

#undef GPBS_DEC_ATTN

