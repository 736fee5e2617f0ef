// The prefill attention kernel.  Not a header of its own: prefill_kernels.hip
// includes this text four times, inside namespace gpbs_pf, with GPBS_SEQ 0
// (k_prefill_attn: S and pos are kernel arguments) and GPBS_SEQ 1
// (k_prefill_attn_seq: the launch is sized for Sq tokens per sequence, the row
// stride of q / out, and a workgroup takes pos = posb[b] and S = n_b, the tokens
// its sequence really has, from device memory).  Everything outside the #if
// blocks is shared: tiles, diagonal and clamps follow the workgroup's own
// (S, pos), so sequence b gets the bits of the uniform kernel run on it alone.
// Rows s >= n_b of out are not stored: the caller hands in a zeroed out.
// GPBS_SEQ 2 is a third compilation, k_prefill_attn_paged: the _seq kernel over
// pools [P, Hkv, page, 128] addressed through an int32 block table [B, NP]
// (logical row r of sequence b: page table[b, r / page], page row r % page;
// Cl = NP * page stands where C stood).  A staged tile of kKT rows never
// straddles a page, and the krow_last clamp stays inside the tile that holds
// krow_last, so the only new work is one workgroup-uniform table entry per
// tile, loaded one prefetch ahead of the rows it addresses; an entry outside
// [0, P) reads page 0.
// GPBS_SEQ 3 is a fourth compilation, k_prefill_attn_paged_kv8: the paged kernel
// over e4m3 pools (one byte per element) with one power-of-two fp32 scale per
// (page, KV head, page row).  The prefetch registers hold 8-byte pieces and their
// rows' scales; a piece becomes its 16 bytes of bf16 (kv8_dequant8: exact) where
// it is stored to LDS, so the loads stay in flight under the MFMAs and the K and
// V images, and with them everything from the first LDS read on, are those of
// the paged kernel on the dequantised pools.
#if GPBS_SEQ
#define GPBS_PF_STRIDE Sq
#else
#define GPBS_PF_STRIDE S
#endif

// q [B, S, H, 128], caches [B, Hkv, C, 128], out [B, S, H * 128]; H = G * Hkv.
template <int G>
#if GPBS_SEQ == 3
__global__ __launch_bounds__(kWaves * 64) void k_prefill_attn_paged_kv8(const u32x4* __restrict__ q,
                                                                        const u32x2* __restrict__ kc,
                                                                        const u32x2* __restrict__ vc,
                                                                        const float* __restrict__ ksc,
                                                                        const float* __restrict__ vsc,
                                                                        const int* __restrict__ posb,
                                                                        const int* __restrict__ lenb,
                                                                        const int* __restrict__ table,
                                                                        u32x2* __restrict__ out, int Sq, int Hkv,
                                                                        int NP, int P, int psh, float scale_log2e,
                                                                        int nbh) {
  const int C = NP << psh;  // the logical context Cl
#elif GPBS_SEQ == 2
__global__ __launch_bounds__(kWaves * 64) void k_prefill_attn_paged(const u32x4* __restrict__ q,
                                                                    const u32x4* __restrict__ kc,
                                                                    const u32x4* __restrict__ vc,
                                                                    const int* __restrict__ posb,
                                                                    const int* __restrict__ lenb,
                                                                    const int* __restrict__ table,
                                                                    u32x2* __restrict__ out, int Sq, int Hkv, int NP,
                                                                    int P, int psh, float scale_log2e, int nbh) {
  const int C = NP << psh;  // the logical context Cl
#elif GPBS_SEQ
__global__ __launch_bounds__(kWaves * 64) void k_prefill_attn_seq(const u32x4* __restrict__ q,
                                                                  const u32x4* __restrict__ kc,
                                                                  const u32x4* __restrict__ vc,
                                                                  const int* __restrict__ posb,
                                                                  const int* __restrict__ lenb,
                                                                  u32x2* __restrict__ out, int Sq, int Hkv, int C,
                                                                  float scale_log2e, int nbh) {
#else
__global__ __launch_bounds__(kWaves * 64) void k_prefill_attn(const u32x4* __restrict__ q,
                                                              const u32x4* __restrict__ kc,
                                                              const u32x4* __restrict__ vc, u32x2* __restrict__ out,
                                                              int S, int Hkv, int C, int pos, float scale_log2e,
                                                              int nbh) {
#endif
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kTileBytes];  // K image, V image
  constexpr int TPW = kRows / G;  // tokens per workgroup (a multiple of 32)
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bh = blockIdx.x % nbh, qt = gridDim.x / nbh - 1 - blockIdx.x / nbh;  // heaviest query tiles first
  const int b = bh / Hkv, kvh = bh % Hkv, H = G * Hkv;
  const int q0 = qt * TPW;
#if GPBS_SEQ
  const int pos = posb[b];
  const int S = seq_tokens(pos, lenb[b], Sq, C);  // 0 <= pos and pos + S <= C, or S == 0
  if (q0 >= S) return;  // workgroup-uniform, before the first barrier: only padding tokens here
#endif
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
    const u32x4* qp = q + (((size_t)b * GPBS_PF_STRIDE + s) * H + kvh * G + g) * (kHd / 8) + h;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = __builtin_bit_cast(bf16x8, qp[2 * ks]);
  }

  // staging: piece i of this thread is chunk sch of tile row srow + 32 i
  const int srow = tid >> 4, sch = tid & 15;
#if GPBS_SEQ >= 2
  // row r of tile t sits in page table[b, t kKT / page] at page row r % page;
  // pgn is the entry of the tile the next prefetch loads, fetched one tile ahead
  const int* trow = table + (size_t)b * NP;
  const int pmask = (1 << psh) - 1;
  const size_t head = (size_t)kvh << psh;
  const size_t pstride = (size_t)Hkv << psh;
  const int pg0 = page_or0(trow[0], P);
  int pgn = ntiles > 1 ? page_or0(trow[kKT >> psh], P) : 0;
#else
  const size_t head = ((size_t)b * Hkv + kvh) * C;
#endif
#if GPBS_SEQ == 3
  u32x2 kr[2], vr[2];  // 8 codes each, and the scales of their rows
  float ksr[2], vsr[2];
#else
  u32x4 kr[2], vr[2];
#endif
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#if GPBS_SEQ >= 2
    const size_t row = head + pg0 * pstride + min(srow + 32 * i, krow_last);  // tile 0: page row == row
#else
    const size_t row = head + min(srow + 32 * i, krow_last);
#endif
    kr[i] = kc[row * (kHd / 8) + sch];
    vr[i] = vc[row * (kHd / 8) + sch];
#if GPBS_SEQ == 3
    ksr[i] = ksc[row];
    vsr[i] = vsc[row];
#endif
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
#if GPBS_SEQ == 3
      *reinterpret_cast<u32x4*>(lds + img_off(srow + 32 * i, sch)) = kv8_dequant8(kr[i], ksr[i]);
      *reinterpret_cast<u32x4*>(lds + kTileBytes + img_off(srow + 32 * i, sch)) = kv8_dequant8(vr[i], vsr[i]);
#else
      *reinterpret_cast<u32x4*>(lds + img_off(srow + 32 * i, sch)) = kr[i];
      *reinterpret_cast<u32x4*>(lds + kTileBytes + img_off(srow + 32 * i, sch)) = vr[i];
#endif
    }
    __syncthreads();
    if (t + 1 < ntiles) {  // next tile in flight under this tile's MFMAs
#if GPBS_SEQ >= 2
      const size_t pbase = head + pgn * pstride;
      if (t + 2 < ntiles) pgn = page_or0(trow[((t + 2) * kKT) >> psh], P);
#endif
#pragma unroll
      for (int i = 0; i < 2; ++i) {
#if GPBS_SEQ >= 2
        const size_t row = pbase + (min((t + 1) * kKT + srow + 32 * i, krow_last) & pmask);
#else
        const size_t row = head + min((t + 1) * kKT + srow + 32 * i, krow_last);
#endif
        kr[i] = kc[row * (kHd / 8) + sch];
        vr[i] = vc[row * (kHd / 8) + sch];
#if GPBS_SEQ == 3
        ksr[i] = ksc[row];
        vsr[i] = vsc[row];
#endif
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
  u32x2* op = out + (((size_t)b * GPBS_PF_STRIDE + s) * H + kvh * G + g) * (kHd / 4) + h;
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

#undef GPBS_PF_STRIDE
