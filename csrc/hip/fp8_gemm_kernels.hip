// Gated, LDS-tiled fp8 (OCP e4m3fn) GEMM for gfx950 (MI355X): the compute
// tenant at the part's headline matrix rate, and the large-M path of the fp8
// linear (prefill).
//
//     C[M][N] (bf16) = ((Aq[M][K] . Bq[N][K]^T) * sa[m]) * sb[n]
//
// Aq / Bq are e4m3fn bytes, sa / sb fp32 per-row / per-output-column scales
// (quant_rows_fp8), the accumulation is fp32 and the epilogue multiplies in
// the order written before rounding to bf16 (RNE).  The MFMA is the
// block-scaled v_mfma_scale_f32_16x16x128_f8f6f4 with e4m3 operands (cbsz =
// blgp = 0): twice the bf16 rate, where the non-scaled 16x16x32_fp8_fp8 of
// the skinny kernel (fp8_kernels.hip) runs at the bf16 rate.  Its E8M0 block
// scales are all 1.0 (0x7f in every byte, so the op_sel byte choice cannot
// matter); the real scales are applied in the epilogue.
//
// The tile loop, the A staging and the epilogue walk are gemm_q_tile.hpp's.
// Row-major B is staged as A is, byte for byte: LDS holds [buf][A|B][128
// rows][128 B] (64 KiB, 2 workgroups per CU).
//
// Operand fragments: lane l holds row / column (l & 15) and the 32
// consecutive k bytes from 32 * (l >> 4): chunks 2g and 2g + 1, g = l >> 4.
// A and B fragments are built the same way, so each lane group pairs the same
// 32 k's of both operands and the sum is right whatever k the hardware gives
// each byte.  The instruction's own map of an e4m3 operand is not this one
// (fp4_kernels.hip measured it: VGPRs 0..3 are k = 16 g .. + 16, VGPRs 4..7
// k = 64 + 16 g .. + 16); it matters only where the two operands differ in
// format or carry real scales.
//
// BSHUF = 1: B is llm.Fp8Weight.qs, the lane-order layout of the skinny
// kernel: the 16 bytes W[n][k .. k+16), k % 16 == 0, live at
//   ((n/16)*(K/256) + k/256)*4096 + ((k%256)/64)*1024 + ((k%64)/16)*256 + (n%16)*16
// (K % 256 == 0): per 16-row strip and 64 k, four 256-byte runs [chunk][row]
// that are one contiguous 1 KiB.  global_load_lds writes LDS lane-linear, so
// an image keeps the order in which the lanes of one instruction read their
// source.  Filling the row-major image above from this layout makes
// consecutive lanes read 16 bytes each from lines 256 B apart; measured, that
// costs 18 % (966 vs 1171 TF/s at 4224x4224x4096, the rows marked superseded
// in profiles/kbench_gemm_fp8.jsonl).  So the B image of this variant keeps the
// source order instead: piece p = 2 strip + (k half) holds [4 chunks][16
// rows][16 B], one wave-instruction copies one contiguous 1 KiB (four whole
// runs), and a wave stages the two strips its pieces 4w .. 4w + 3 cover.  A
// fragment is the same two ds_read_b128 (chunks 2g, 2g + 1 are 256 B apart
// in the piece of half g >> 1; 16 lanes read 256 contiguous bytes, no
// swizzle needed).  The lane -> (row, k) map, the MFMA order and the
// epilogue are those of BSHUF = 0, so both give the same bits on the same
// operands.
#include "gemm_q_tile.hpp"

namespace gpbs_fp8g {

using namespace gpbs_qtile;

template <int BSHUF>
struct Fp8Tile {
  static constexpr int kLds = 2 * 2 * kTileA;  // [buf][A|B][128][128 B]
  const unsigned char* __restrict__ B;
  const float* __restrict__ sb;

  __device__ __forceinline__ void k_loop(const Lanes& L, lds_t* lds, const unsigned char* __restrict__ A,
                                         const size_t (&aoff)[4], int tn, int K, f32x4 (&acc)[4][4]) const {
    size_t boff[4];  // source byte offsets of this lane's four B pieces at K-tile 0
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (BSHUF) {
        // piece p = 4 wid + j: strip p/2 of the tile, k half p%2.  k = 128 kt +
        // 64 half + 16 chunk: block k/256 = kt/2, step u = 2 (kt & 1) + half,
        // then [chunk][row][16 B] = lane order
        const int p = L.wid * 4 + j;
        boff[j] = (size_t)(tn * (BN / 16) + (p >> 1)) * (K >> 8) * 4096 + (p & 1) * 1024 + L.lane * 16;
      } else {
        boff[j] = (size_t)(tn * BN + L.srow(j)) * K + L.schunk(j) * 16;
      }
    }
    const int nk = K / BK;  // steps of 128 k on alternating buffers; K % 128 == 0, the count may be odd (BSHUF = 0)
    constexpr int bstep = BSHUF ? 2048 : BK;  // B bytes per K-tile at fixed (row, chunk)
    auto stage = [&](int buf, int kt) {
      lds_t* la = lds + buf * (2 * kTileA);
      lds_t* lb = la + kTileA;
      L.stage_a(A, aoff, kt, la);
#pragma unroll
      for (int j = 0; j < 4; ++j) glds16(B + boff[j] + (size_t)kt * bstep, lb + (L.wid * 4 + j) * 1024);
    };
    // 16 rows from r0 of a row-major image: k bytes 32 lq .. 32 lq + 31 of row r0 + l16.
    auto frag = [&](const lds_t* img, int r0) -> i32x8 { return L.frag_rows(img, r0, 2 * L.lq, 2 * L.lq + 1); };
    // The same fragment of the BSHUF = 1 B image (r0 % 16 == 0): strip r0/16,
    // piece of k half lq/2, chunks 2 (lq & 1) and + 1 of its [chunk][row][16 B].
    auto frag_shuf = [&](const lds_t* img, int r0) -> i32x8 {
      const lds_t* p = img + ((r0 >> 4) * 2 + (L.lq >> 1)) * 1024 + (L.lq & 1) * 512 + L.l16 * 16;
      const u32x4 lo = *(const __attribute__((address_space(3))) u32x4*)p;
      const u32x4 hi = *(const __attribute__((address_space(3))) u32x4*)(p + 256);
      return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    };

    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
      const lds_t* la = lds + cur * (2 * kTileA);
      const lds_t* lb = la + kTileA;
      i32x8 a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[i] = frag(la, L.wr * 64 + i * 16);
        b[i] = BSHUF ? frag_shuf(lb, L.wc * 64 + i * 16) : frag(lb, L.wc * 64 + i * 16);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], b[j], acc[i][j], 0, 0, 0, kOne, 0, kOne);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      cur ^= 1;
    }
  }

  __device__ __forceinline__ float col(int n) const { return sb[n]; }
  static __device__ __forceinline__ u16 out(float acc, float sa, float wsc) {
    return __builtin_bit_cast(u16, (__bf16)((acc * sa) * wsc));
  }
};

template <int BSHUF>
__global__ __launch_bounds__(NT, 2) void k_gemm_fp8_tn(const unsigned char* __restrict__ A,
                                                       const float* __restrict__ sa,
                                                       const unsigned char* __restrict__ B,
                                                       const float* __restrict__ sb, u16* __restrict__ C, int M,
                                                       int N, int K, WorkQueue* q, const PartTable* table, u32 mode,
                                                       u32 me, u64* cnt, u32 inst_per_tile, u32 refs_per_tile,
                                                       u32 miss_per_tile, u32* status) {
  tile_loop(Fp8Tile<BSHUF>{B, sb}, A, sa, C, M, N, K, q, table, mode, me, cnt, inst_per_tile, refs_per_tile,
            miss_per_tile, status);
}

}  // namespace gpbs_fp8g

using namespace gpbs_fp8g;

extern "C" {

int gpbs_hip_gemm_fp8_units(int M, int N) { return tile_count(M, N); }

int gpbs_hip_gemm_fp8(const void* Aq, const float* sa, const void* Bq, const float* sb, void* C, int M, int N, int K,
                      int b_shuffled, void* q, const void* table, unsigned mode, unsigned me, void* cnt, void* status,
                      int grid, hipStream_t s) {
  if (M <= 0 || N <= 0 || K <= 0 || N % BN || K % BK || (b_shuffled && K % 256)) return -22;
  const int ntiles = tile_count(M, N);
  grid = launch_grid(grid, ntiles);
  // Model of the 128x128 bf16 path with fp8 byte counts: per tile and K-tile
  // 64 MFMA + 32 glds + 64 ds_read_b128 (4 waves); refs = A + B panels in
  // 128-B lines; fills = compulsory bytes spread over the tiles + the C tile.
  const u32 inst = (u32)((K / BK) * (64 + 32 + 64) + 64);
  const u32 refs = (u32)(((u64)(BM + BN) * K) / 128);
  const u32 miss = (u32)((((u64)M + N) * K / 128) / ntiles + (u64)BM * BN * 2 / 128);
  auto kern = b_shuffled ? k_gemm_fp8_tn<1> : k_gemm_fp8_tn<0>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), 0, s, (const unsigned char*)Aq, sa, (const unsigned char*)Bq, sb,
                     (u16*)C, M, N, K, (WorkQueue*)q, (const PartTable*)table, mode, me, (u64*)cnt, inst, refs, miss,
                     (u32*)status);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
