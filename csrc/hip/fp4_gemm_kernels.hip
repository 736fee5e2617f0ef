// Gated, LDS-tiled MXFP4 GEMM for gfx950 (MI355X): the large-M (prefill) path
// of the MXFP4 linear, one launch for any M where k_mxfp4_gemm_skinny
// (fp4_kernels.hip) streams the whole weight once per 64 rows.
//
//     Y[M][N] (bf16) = (Xq[M][K] . deq(W)[N][K]^T) * sx[m]
//
// Xq are the e4m3 rows and sx the fp32 row scales of the fp8 quantisers, W is
// an llm.Mxfp4Weight exactly as the skinny kernel reads it (qs, ss): no second
// layout, no second copy.  The MFMA is v_mfma_scale_f32_16x16x128_f8f6f4 with
// the e4m3 operand (cbsz = 0, scale bytes 0x7f) against the e2m1 codes (blgp =
// 4, 4 VGPRs, the upper four zero) and the E8M0 byte of each lane's 32 codes in
// the lane's scale register.  Accumulation is fp32, the output one RNE
// rounding to bf16; there is no residual form.
//
// The tile loop, the A image and its staging, and the epilogue walk are
// gemm_q_tile.hpp's, shared with k_gemm_fp8_tn (fp8_gemm_kernels.hip).  What
// is this kernel's:
//
// A fragment.  Against an fp4 B the instruction's own k map of the e4m3
// operand decides which products are formed: for lane group g = lane >> 4,
// VGPRs 0..3 are k = 16 g .. + 16 and VGPRs 4..7 are k = 64 + 16 g .. + 16 of
// the 128-k step (measured in fp4_kernels.hip).  So the lane of row r reads
// chunks g and 4 + g, at slots g ^ (r & 7) and (4 + g) ^ (r & 7); the fp8
// kernel's 2 g, 2 g + 1 would pair every k with the wrong weight.
//
// B operand.  The codes of a 16-row strip for one 128-k step (block kb of 256
// k, step u) are one contiguous 1 KiB run of qs, at ((n / 16) (K / 256) + kb)
// 2048 + 1024 u, already in lane order [g][r][16 B].  One wave-wide 16-byte
// global_load_lds copies it and lane l reads its fragment with one
// ds_read_b128 at strip * 1024 + 16 l: consecutive lanes, consecutive 16 B, no
// swizzle.  A tile is 8 strips, 8 KiB per 128 k: half the fp8 kernel's B bytes
// in global traffic and in LDS.
//
// Scales.  The lane's E8M0 word of block kb is at ((n / 16) (K / 256) + kb)
// 128 + 2 l in ss, byte u the scale of its codes at step u.  The 8 strips x
// 128 B of a tile's block are staged with the block's first step as one more
// 1 KiB wave-wide copy (lane l: strip l >> 3, bytes 16 (l & 7) .. + 16), so no
// plain global load is outstanding beside the LDS-DMA.  A wave reads its four
// words (one per strip of its 64 columns) in the first step and keeps them in
// registers for the second, so one scale image serves both buffers.  op_sel is
// an immediate: the K loop is unrolled by two, step u = 0 on buffer 0 and u =
// 1 on buffer 1 (K % 256 == 0 makes the count of 128-k steps even).
//
// LDS: 2 x (16 + 8) KiB + 1 KiB of scales + the queue slot: two workgroups
// per CU.  N % 128 == 0 and K % 256 == 0.
#include "gemm_q_tile.hpp"

namespace gpbs_fp4g {

using namespace gpbs_qtile;

constexpr int kTileB = BN * BK / 2;      // bytes of the fp4 B image of one step: 8 strips of 1 KiB
constexpr int kBuf = kTileA + kTileB;    // one buffer: [A | B]
constexpr int kScale = (BN / 16) * 128;  // scale words of one 256-k block: [8 strips][64 lanes][2 B]

struct None {};  // what col(n) loads here: the output has no per-column factor

struct Mxfp4Tile {
  static constexpr int kLds = 2 * kBuf + kScale;
  const unsigned char* __restrict__ Bq;
  const unsigned char* __restrict__ Bs;

  __device__ __forceinline__ void k_loop(const Lanes& L, lds_t* lds, const unsigned char* __restrict__ A,
                                         const size_t (&aoff)[4], int tn, int K, f32x4 (&acc)[4][4]) const {
    const int nkb = K >> 8;  // blocks of 256 k = two 128-k steps
    const int wid = L.wid, lane = L.lane, wr = L.wr, wc = L.wc;
    lds_t* lsc = lds + 2 * kBuf;
    // Source byte offsets at step 0: the two B strips 2 wid and 2 wid + 1 (one
    // 1 KiB run per step, 1 KiB on per step: u = 1 follows u = 0 and the next
    // block follows that), and this lane's 16 bytes of the tile's scale words
    // (128 B on per block).
    size_t boff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) boff[j] = (size_t)(tn * (BN / 16) + wid * 2 + j) * nkb * 2048 + lane * 16;
    const size_t soff = (size_t)(tn * (BN / 16) + (lane >> 3)) * nkb * 128 + (lane & 7) * 16;
    // Step kt (128 k) into buffer buf; the first step of a block brings the
    // block's scale words with it (wave 0, one instruction).
    auto stage = [&](int buf, int kt, bool scales) {
      lds_t* la = lds + buf * kBuf;
      lds_t* lb = la + kTileA;
      L.stage_a(A, aoff, kt, la);
#pragma unroll
      for (int j = 0; j < 2; ++j) glds16(Bq + boff[j] + (size_t)kt * 1024, lb + (wid * 2 + j) * 1024);
      if (scales && wid == 0) glds16(Bs + soff + (size_t)(kt >> 1) * 128, lsc);
    };
    // 16 rows from r0 of the A image: the k the instruction takes from the lane of row r0 + l16.
    auto frag_a = [&](const lds_t* img, int r0) -> i32x8 { return L.frag_rows(img, r0, L.lq, 4 + L.lq); };
    // The lane's 32 codes of one strip: the first 4 of the 8 registers.
    auto frag_b = [&](const lds_t* img, int strip) -> i32x8 {
      const u32x4 v = *(const __attribute__((address_space(3))) u32x4*)(img + strip * 1024 + lane * 16);
      return i32x8{(int)v[0], (int)v[1], (int)v[2], (int)v[3], 0, 0, 0, 0};
    };

    int sc[4];  // the lane's scale words of the current block, one per strip of the wave's 64 columns
    stage(0, 0, true);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kb = 0; kb < nkb; ++kb) {
      {  // step u = 0 on buffer 0
        stage(1, 2 * kb + 1, false);
        const lds_t* la = lds;
        const lds_t* lb = la + kTileA;
        i32x8 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = frag_a(la, wr * 64 + i * 16);
          b[i] = frag_b(lb, wc * 4 + i);
          sc[i] = *(const __attribute__((address_space(3))) u16*)(lsc + (wc * 4 + i) * 128 + lane * 2);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] =
                __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], b[j], acc[i][j], 0, 4, 0, kOne, 0, sc[j]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
      {  // step u = 1 on buffer 1
        if (kb + 1 < nkb) stage(0, 2 * kb + 2, true);
        const lds_t* la = lds + kBuf;
        const lds_t* lb = la + kTileA;
        i32x8 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = frag_a(la, wr * 64 + i * 16);
          b[i] = frag_b(lb, wc * 4 + i);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] =
                __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], b[j], acc[i][j], 0, 4, 0, kOne, 1, sc[j]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
  }

  // No column factor.  The rounding is that of k_mxfp4_gemm_skinny, so both
  // kernels give the same bits on the same fp32 value.
  __device__ __forceinline__ None col(int) const { return {}; }
  static __device__ __forceinline__ u16 out(float acc, float sa, None) {
    u32 u = __float_as_uint(acc * sa);
    u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even
    return (u16)(u >> 16);
  }
};

__global__ __launch_bounds__(NT, 2) void k_gemm_mxfp4_tn(const unsigned char* __restrict__ A,
                                                         const float* __restrict__ sa,
                                                         const unsigned char* __restrict__ Bq,
                                                         const unsigned char* __restrict__ Bs, u16* __restrict__ C,
                                                         int M, int N, int K, WorkQueue* q, const PartTable* table,
                                                         u32 mode, u32 me, u64* cnt, u32 inst_per_tile,
                                                         u32 refs_per_tile, u32 miss_per_tile, u32* status) {
  tile_loop(Mxfp4Tile{Bq, Bs}, A, sa, C, M, N, K, q, table, mode, me, cnt, inst_per_tile, refs_per_tile,
            miss_per_tile, status);
}

}  // namespace gpbs_fp4g

using namespace gpbs_fp4g;

extern "C" {

int gpbs_hip_gemm_mxfp4(const void* xq, const float* sx, const void* wq, const void* ws, void* y, int M, int N, int K,
                        void* q, const void* table, unsigned mode, unsigned me, void* cnt, void* status, int grid,
                        hipStream_t s) {
  if (M <= 0 || N <= 0 || K <= 0 || N % BN || K % 256) return -22;
  const int ntiles = tile_count(M, N);
  grid = launch_grid(grid, ntiles);
  // The model of gpbs_hip_gemm_fp8 with this kernel's counts.  Per tile and
  // 256-k block (4 waves): 128 MFMA, 32 A + 16 B + 1 scale glds, 64 A + 32 B
  // ds_read_b128 and 16 scale reads.  refs = the A panel, the B panel at half
  // a byte per element and its scale bytes (one per 32 k) in 128-B lines;
  // fills = the compulsory bytes spread over the tiles + the C tile.
  const u32 inst = (u32)((K / 256) * (128 + 49 + 96 + 16) + 64);
  const u32 refs = (u32)(((u64)BM * K + (u64)BN * K / 2 + (u64)BN * K / 32) / 128);
  const u32 miss =
      (u32)((((u64)M * K + (u64)N * K / 2 + (u64)N * K / 32) / 128) / ntiles + (u64)BM * BN * 2 / 128);
  hipLaunchKernelGGL(k_gemm_mxfp4_tn, dim3(grid), dim3(NT), 0, s, (const unsigned char*)xq, sx,
                     (const unsigned char*)wq, (const unsigned char*)ws, (u16*)y, M, N, K, (WorkQueue*)q,
                     (const PartTable*)table, mode, me, (u64*)cnt, inst, refs, miss, (u32*)status);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
