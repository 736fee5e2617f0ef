// The 128x128 tile skeleton of the quantised tiled GEMMs for gfx950 (MI355X):
// k_gemm_fp8_tn (fp8_gemm_kernels.hip) and k_gemm_mxfp4_tn
// (fp4_gemm_kernels.hip).  Everything the two share is here once; each .hip
// holds its operand policy: B and scale staging, the K loop, the output
// expression.
//
// Structure of k_gemm_bf16_tn (tenant_kernels.hip): persistent workgroups
// over a tile queue, ownership re-checked between tiles, 128x128 output
// tile, 4 waves (2x2) of 64x64, each a 4x4 grid of 16x16 blocks, one MFMA per
// block and 128 k: 16 per wave and step.  Operands are staged by
// global_load_lds_dwordx4 in 1 KiB pieces, in two buffers of 128 k.
//
// A image of one step: [128 rows][128 B], BK = 128 e4m3 elements = one
// 128-byte row, filled in pieces of 8 rows, 16-B chunk c of row r kept at slot
// c ^ (r & 7) (the swizzle is applied on the global SOURCE address, LDS is
// written lane-linear).  A fragment is two ds_read_b128 of one row; which two
// logical chunks a lane group reads is the policy's (frag_rows).
//
// Ragged M: any M > 0.  Staging clamps the row index to M - 1 (the clamped
// rows feed only accumulators whose stores are skipped), rows >= M are not
// stored.  N % 128 == 0; K as the policy needs.
#pragma once
#include <algorithm>
#include "common.hpp"

namespace gpbs_qtile {

using namespace gpbs_hip;

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) char lds_t;

constexpr int BM = 128, BN = 128, BK = 128, NT = 256;
constexpr int kTileA = BM * BK;   // bytes of the e4m3 A image of one step
constexpr int kOne = 0x7f7f7f7f;  // E8M0 1.0 in every byte: the scale of an e4m3 operand
constexpr int kGroupM = 8;

__device__ __forceinline__ void glds16(const void* g, lds_t* l) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// L2-friendly grouped order: GROUP_M = 8 row panels share B column panels; the
// last group has the tile rows that are left.
__device__ __forceinline__ void tile_of(int t, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int in_group = kGroupM * tiles_n;
  const int first_m = t / in_group * kGroupM;
  const int gsz = min(tiles_m - first_m, kGroupM);
  tm = first_m + (t % in_group) % gsz;
  tn = (t % in_group) / gsz;
}

// A thread's place in the workgroup and its part of the A operand.
struct Lanes {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wr = wid >> 1, wc = wid & 1;      // the wave computes rows 64 wr .., columns 64 wc .. of the tile
  const int l16 = lane & 15, lq = lane >> 4;  // lane = 16 lq + l16
  // Staging geometry: this wave loads pieces c = wid*4 + j (8 rows of 128 B
  // each); lane -> row 8c + lane/8, LDS slot lane%8, global 16-B chunk
  // (slot ^ (row & 7)) of the K-tile.
  __device__ __forceinline__ int srow(int j) const { return 8 * (wid * 4 + j) + (lane >> 3); }
  __device__ __forceinline__ int schunk(int j) const { return (lane & 7) ^ (srow(j) & 7); }

  // Source byte offsets of this lane's four A pieces of tile row tm at K-tile 0.
  __device__ __forceinline__ void a_offsets(int tm, int M, int K, size_t (&aoff)[4]) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ra = min(tm * BM + srow(j), M - 1);  // ragged M: clamp, never read past the last row
      aoff[j] = (size_t)ra * K + schunk(j) * 16;
    }
  }

  // K-tile kt of A into the image at img.
  __device__ __forceinline__ void stage_a(const unsigned char* A, const size_t (&aoff)[4], int kt, lds_t* img) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(A + aoff[j] + (size_t)kt * BK, img + (wid * 4 + j) * 1024);
  }

  // 16 rows from r0 of a swizzled [rows][128 B] image: the lane reads logical
  // chunks c_lo and c_hi of row r0 + l16 into registers 0..3 and 4..7.
  __device__ __forceinline__ i32x8 frag_rows(const lds_t* img, int r0, int c_lo, int c_hi) const {
    const int r = r0 + l16;
    const lds_t* row = img + r * 128;
    const u32x4 lo = *(const __attribute__((address_space(3))) u32x4*)(row + ((c_lo ^ (r & 7)) << 4));
    const u32x4 hi = *(const __attribute__((address_space(3))) u32x4*)(row + ((c_hi ^ (r & 7)) << 4));
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  }
};

// The persistent tile loop, the body of both kernels.  The policy P supplies
//   P::kLds                         bytes of its LDS images
//   p.k_loop(L, lds, A, aoff, tn, K, acc)
//                                   its B and scale source offsets of column panel tn, and all of K into
//                                   acc[i][j]: block (i, j) of the wave's 4x4
//   p.col(n), P::out(acc, sa, col)  the bf16 bits of one output from its sum, its row scale and what col(n)
//                                   loaded once for column n
template <class P>
__device__ __forceinline__ void tile_loop(const P p, const unsigned char* __restrict__ A,
                                          const float* __restrict__ sa, u16* __restrict__ C, int M, int N, int K,
                                          WorkQueue* q, const PartTable* table, u32 mode, u32 me, u64* cnt,
                                          u32 inst_per_tile, u32 refs_per_tile, u32 miss_per_tile, u32* status) {
  __shared__ __attribute__((aligned(16))) char smem[P::kLds + 16];
  lds_t* lds = (lds_t*)smem;
  int* s_slot = (int*)(smem + P::kLds);
  const u32 xcc = xcc_id();
  u64 t_last = __builtin_amdgcn_s_memtime();
  const Lanes L;
  const int tiles_m = (M + BM - 1) / BM, tiles_n = N / BN, ntiles = tiles_m * tiles_n;

  for (;;) {
    const int t = grab_unit(q, table, mode, me, xcc, s_slot, (u32)ntiles);
    if (t < 0) break;
    int tm, tn;
    tile_of(t, tiles_m, tiles_n, tm, tn);
    size_t aoff[4];
    L.a_offsets(tm, M, K, aoff);
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    p.k_loop(L, lds, A, aoff, tn, K, acc);

    // Epilogue: D(row = (lane>>4)*4 + r, col = lane&15) per 16x16 block.
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = tn * BN + L.wc * 64 + j * 16 + L.l16;
      const auto col = p.col(n);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = tm * BM + L.wr * 64 + i * 16 + L.lq * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (m + r < M) C[(size_t)(m + r) * N + n] = P::out(acc[i][j][r], sa[m + r], col);
      }
    }
    count_unit(cnt, me, xcc, inst_per_tile, &t_last, refs_per_tile, miss_per_tile, q);
  }
  finish(q, status, (u32)ntiles);
}

// Host side: the tiles of an [M, N] output (0 where there are none) and the
// launch grid for them (grid <= 0: two workgroups on each of the 256 CUs).
inline int tile_count(int M, int N) { return M <= 0 || N <= 0 || N % BN ? 0 : ((M + BM - 1) / BM) * (N / BN); }

inline int launch_grid(int grid, int ntiles) { return std::min(grid <= 0 ? 256 * 2 : grid, ntiles); }

}  // namespace gpbs_qtile
