// Tenant workload kernels for gfx950 (MI355X), partition-aware.
//
// Every kernel is a persistent grid over a WorkQueue: workgroups read their
// XCD id (HW_REG_XCC_ID), leave at once when the scheduler's partition table
// does not give that XCD to their tenant, and otherwise pull tiles/chunks with
// one atomic per unit, re-checking ownership between units.  This is the
// MI355X actuation of the reference's context switch: the credit scheduler
// hands XCD partitions to tenants and a revoked XCD drains within one tile
// (X:xen/arch/x86/domain.c:1584-1660 is what it replaces).  Each workgroup
// adds its modeled counters (instructions, busy cycles, L2 line references,
// HBM line fills) into a per-(tenant, XCD) block at exit: the vPMU analog
// (X:xen/arch/x86/perfctr.c:1547-1572).
#include "common.hpp"

namespace gpbs_hip {

// ---------------------------------------------------------------- helpers --

// Thread 0 decides for the whole workgroup: grab the next unit, or stop when
// the XCD was revoked.  Returns the unit index, or -1 to stop.
__device__ __forceinline__ int grab_unit_x(WorkQueue* q, const PartTable* table, u32 mode, u32 me, u32 xcc,
                                           int* s_slot, u32 total) {
  if (threadIdx.x == 0) {
    int u = -1;
    hold_wait(table, mode);
    const u32 per = (total + kXcds - 1) / kXcds;
    for (u32 spins = 0;; ++spins) {
      if (owns(table, mode, me, xcc)) {
        for (u32 k = 0; k < (u32)kXcds; ++k) {
          const u32 r = (xcc + k) & (kXcds - 1);
          const u32 lo = r * per, hi = min(lo + per, total);
          if (lo >= hi) continue;
          if (__hip_atomic_load(&q->xnext[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= hi - lo) continue;
          const u32 t = atomicAdd(&q->xnext[r], 1u);
          if (t < hi - lo) {
            u = (int)(lo + t);
            atomicAdd(&q->next, 1u);
            break;
          }
        }
        break;
      }
      if ((mode & 3) != GATE_PARK || spins >= kParkSpins ||
          __hip_atomic_load(&q->next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= total) {
        atomicAdd(&q->stopped, 1u);
        break;
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) __builtin_amdgcn_s_sleep(127);
    }
    *s_slot = u;
  }
  __syncthreads();
  int u = *s_slot;
  __syncthreads();
  return u;
}

// Per-unit counter accumulation by thread 0 (tile-granular vPMU: the scheduler
// sees a smooth rate instead of bursts at kernel exit).

__device__ __forceinline__ u16 f2bf(float x) { return __builtin_bit_cast(u16, (__bf16)x); }
__device__ __forceinline__ float bf2f(u16 x) { return __uint_as_float(((u32)x) << 16); }

// ------------------------------------------------------------------ GEMM ---
// C[M][N] = A[M][K] * Bt[N][K]^T, bf16 inputs, fp32 MFMA accumulation, bf16
// output.  128x128 output tile, BK = 64, 4 waves (2x2) of 64x64, each wave a
// 4x4 grid of v_mfma_f32_16x16x32_bf16.  A and B tiles are staged by
// global_load_lds_dwordx4 (LDS-DMA, 1 KiB per wave-instruction) into a
// double-buffered, XOR-swizzled [128][64] image (swizzle applied on the
// global SOURCE address, LDS written lane-linear); fragments are read with
// conflict-free ds_read_b128.  64 KiB LDS -> 2 workgroups per CU.
constexpr int GBM = 128, GBN = 128, GBK = 64, GNT = 256;
constexpr int kGemmLds = 2 * 2 * GBM * GBK * 2;  // [buf][A|B][128][64] bf16

typedef __attribute__((address_space(3))) char lds_t;

__device__ __forceinline__ void glds16(const void* g, lds_t* l) {
  __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

__global__ __launch_bounds__(GNT, 2) void k_gemm_bf16_tn(const u16* __restrict__ A, const u16* __restrict__ Bt,
                                                         u16* __restrict__ C, int M, int N, int K, WorkQueue* q,
                                                         const PartTable* table, u32 mode, u32 me, u64* cnt,
                                                         u32 inst_per_tile, u32 refs_per_tile, u32 miss_per_tile,
                                                         u32* status) {
  __shared__ __attribute__((aligned(16))) char smem[kGemmLds + 16];
  lds_t* lds = (lds_t*)smem;
  int* s_slot = (int*)(smem + kGemmLds);
  const u32 xcc = xcc_id();
  // Ownership is decided by thread 0 inside grab_unit (workgroup-uniform).
  u64 t_last = __builtin_amdgcn_s_memtime();
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int tiles_m = M / GBM, tiles_n = N / GBN, ntiles = tiles_m * tiles_n;
  const int nk = K / GBK;
  constexpr int GROUP_M = 8;

  // Per-lane staging geometry: this wave loads chunks c = wid*4 + j (8 rows of
  // 128 B each); lane -> row 8c + lane/8, LDS slot lane%8, global k-chunk
  // (slot ^ (row & 7)).
  int srow[4], scol[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = wid * 4 + j;
    srow[j] = 8 * c + (lane >> 3);
    scol[j] = (((lane & 7) ^ (srow[j] & 7)) * 8);
  }

  for (;;) {
    const int t = grab_unit(q, table, mode, me, xcc, s_slot, (u32)ntiles);
    if (t < 0) break;
    // L2-friendly grouped order (GROUP_M row panels share B column panels).
    const int in_group = GROUP_M * tiles_n;
    const int g = t / in_group;
    const int first_m = g * GROUP_M;
    const int gsz = min(tiles_m - first_m, GROUP_M);
    const int tm = first_m + (t % in_group) % gsz;
    const int tn = (t % in_group) / gsz;
    const u16* Ab = A + (size_t)tm * GBM * K;
    const u16* Bb = Bt + (size_t)tn * GBN * K;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto stage = [&](int buf, int kt) {
      lds_t* la = lds + buf * (2 * GBM * GBK * 2);
      lds_t* lb = la + GBM * GBK * 2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = wid * 4 + j;
        glds16(Ab + (size_t)srow[j] * K + kt * GBK + scol[j], la + c * 1024);
        glds16(Bb + (size_t)srow[j] * K + kt * GBK + scol[j], lb + c * 1024);
      }
    };

    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
      const lds_t* la = lds + cur * (2 * GBM * GBK * 2);
      const lds_t* lb = la + GBM * GBK * 2;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 a[4], b[4];
        const int chunk = s * 4 + (lane >> 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int ra = wr * 64 + i * 16 + (lane & 15);
          a[i] = *(const __attribute__((address_space(3))) bf16x8*)(la + ra * 128 + ((chunk ^ (ra & 7)) << 4));
          const int rb = wc * 64 + i * 16 + (lane & 15);
          b[i] = *(const __attribute__((address_space(3))) bf16x8*)(lb + rb * 128 + ((chunk ^ (rb & 7)) << 4));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      cur ^= 1;
    }
    // Epilogue: D(row=(lane>>4)*4+r, col=lane&15) per 16x16 block.
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = tm * GBM + wr * 64 + i * 16 + (lane >> 4) * 4;
        const int n = tn * GBN + wc * 64 + j * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) C[(size_t)(m + r) * N + n] = f2bf(acc[i][j][r]);
      }
    count_unit(cnt, me, xcc, inst_per_tile, &t_last, refs_per_tile, miss_per_tile, q);
  }
  finish(q, status, (u32)ntiles);
}

// -------------------------------------------------------- GEMM 256x256 ----
// The fast path for M, N % 256 == 0 (the co-run GEMM tenant): 256x256 output
// tile per workgroup, BK = 64, 8 waves as 2(M) x 4(N), 128x64 per wave, one
// workgroup per CU (128 KiB LDS).  Halving the A/B panel traffic per FLOP vs
// the 128x128 kernel matters twice here: solo throughput, and how hard the
// GEMM leans on the L2 a co-running memory tenant also streams through.
// This is the one schedule that ships; the variants measured against it and
// their numbers are in docs/gemm_lab.md.
//
// LDS image: [buf][A|B][half][128 rows][128 B].  A half h = rows 128h.. of the
// tile (read only by the waves wr == h), B half h = columns 128h.. (waves
// wc >> 1 == h).  16-B chunk c of row r is stored at slot c ^ g2_swz(r) =
// c ^ ((r >> 1) & 7): a 16-lane ds_read_b128 group (16 consecutive rows, one
// logical chunk) covers all 16 slots of a 256-B bank row.  The swizzle is
// applied to the global source address; global_load_lds writes lane-linear,
// 1 KiB (8 rows) per wave-instruction ("glds" below).
//
// Wave groups: g0 = the four waves wr 0, g1 = wr 1.  g1 takes one extra
// barrier after the prologue and so runs one barrier interval behind g0 for
// the whole K loop (g0 takes the matching one after it): each SIMD holds one
// wave of either group, and one's ds_reads overlap the other's MFMA cluster.
// 1155 TF/s against 1035 with the groups in lock-step, where MFMA busy was
// 41 % (4096^3, profiles/kbench_r1.jsonl).
//
// Two phases per K-tile t (LDS buffer t & 1), four barrier intervals per wave:
//   R_A  read the wave's 8 B fragments (kept for both phases) and A rows 0-63
//        of its 128 (8); stage its share of both B halves of t+1 (4 glds)
//   M_A  lgkmcnt(0); 32 MFMAs: rows 0-63 x all 64 columns x K = 64
//   R_B  read A rows 64-127 (8); stage the group's OWN A half of t+1 (wave wc
//        writes rows 32 wc .. 32 wc + 31: 4 glds); vmcnt(4) retires its B share
//   M_B  lgkmcnt(0); 32 MFMAs: rows 64-127; then vmcnt(0): its A share landed
// With interval 0 = g0's R_A, g0 reads in intervals 0 and 2 and g1 in 1 and 3.
// A barrier interval costs a fixed ~200 cycles (barrier round trip, the MFMA
// wave's restart) beside its MFMA work, so four intervals per K-tile beat the
// earlier eight of 16 MFMAs each (profiles/pmc/gemm_stamps_r3_4phase.json,
// profiles/r3/kbench_gemm_k.log).  A half h is read by group h alone, so a
// group staging its own A half puts 4 glds into every read interval; with one
// group issuing all 8 glds of t+1 in one interval that interval took ~1100
// cycles against ~700 for the others (same files).
// WAR: a half of buffer (t+1) & 1 is restaged only after the barrier that
// follows the lgkmcnt(0) retiring its last read of tile t-1.  B: read in
// intervals 0/1 of t-1, free from interval 3 of t-1, restaged in 0/1 of t.
// A0: read in 2 of t-1, free from 0 of t, restaged in 2.  A1: read in 3 of
// t-1, free from 1 of t, restaged in 3.
// RAW: every issuer's counted vmcnt precedes a barrier the reader passes
// before its read.  B of t+1: g0 retires its share in interval 2, g1 in 3,
// both before barrier 3|4; first read by g0 in 4.  A0: g0 retires it at the
// end of 3 and reads it in 4.  A1: g1 retires it at the end of 4 and reads it
// in 5.  The last K-tile stages nothing and waits vmcnt(0) in R_A.
// The barrier is a raw s_barrier: __syncthreads adds a fence that would drain
// the LDS-DMA queue and with it the counted waits.  All LDS is one __shared__
// array.
//
// Epilogue: C goes through LDS -- the K loop's two buffers are exactly the
// 256x256 bf16 tile, and every wave's K-loop reads retired before the
// re-align barrier.  mfma(B, A) holds C^T per 16x16 block, so a lane owns 4
// consecutive columns of one row: each wave writes its 8-byte fragments at
// row m, 8-byte chunk n/4 XOR (m & 15); after a __syncthreads the workgroup
// stores 16 rows per pass, each row as 32 contiguous 16-byte stores: full
// 128-byte lines instead of 32-byte runs, +1.1-1.3 % in three processes on two
// boxes (profiles/r4/kbench_gemm_ldsc_s51_s52.jsonl).  Banking
// (MI355X_MICROARCH.md §LDS): a ds_write_b64 is four groups of 16 contiguous
// lanes on (a/4) mod 32 -- one group is 16 rows of one chunk column, and XOR
// (m & 15) puts them on 16 distinct 8-byte positions of the 128-byte bank row
// (XOR 2 (m & 15) used 8: a 2-way conflict on every C write, 2.6 M extra
// cycles per 4096^3 GEMM); a ds_read_b128 group reads one row's 16 distinct
// 16-byte slots.  An odd row's two 8-byte chunks of a slot come swapped and
// are swapped back in registers.  The stores are non-temporal, so C does not
// sit dirty in L2 for the end-of-kernel writeback: another +1.0-1.3 % in three
// processes on two boxes (profiles/r4/kbench_gemm_ldsc_nt_s54_s55.jsonl).  A
// closing __syncthreads keeps the next tile's prologue, which restages buffer
// 0, behind the reads.
//
// Tile dealing, three mode bits set by the host (gpbs_hip_set_gemm_opts):
//   kGemmBlock2D (opts bit 3, the default): the tiles one XCD computes form a
//     (tiles_m/4) x (tiles_n/2) block (4096^3: 4 A + 8 B panels per XCD instead
//     of 2 A + 16 B row-major, or 16 A + 2 B dealt round-robin), so its 32
//     concurrent tiles pull 12 operand-panel slices per K-step into its L2
//     instead of 18 (PMC: L2 hit rate 0.68 with row-major dealing).  The XCD
//     of a tile: its range (XCD-range queue: the workgroup's own XCD), or
//     ticket mod 8 (plain queue: tickets follow the round-robin dispatch only
//     approximately).  Solo that is worth 0.2-0.5 %; in the co-runs, where the
//     memory tenants stream through the same L2s, the GEMM keeps its panels
//     and runs 13 % faster: 4mix 1.169 -> 1.250, 8mix 1.275 -> 1.340, static-se
//     and gpbs alike (profiles/r5/s21_gemm_blocks_ab.txt).  Needs tiles_m % 4
//     == 0, tiles_n % 2 == 0 and ntiles % 8 == 0; other shapes are dealt
//     row-major.
//   kGemmXRange (opts bit 0): one tile queue per XCD range (grab_unit_x), so a
//     workgroup computes tiles of its own XCD's range.  Not the default: 946
//     TF/s against 1155 with the plain queue (profiles/kbench_r1.jsonl), 1060
//     against 1129 with 2-D blocks -- the dispatch already deals consecutive
//     tickets round-robin over the XCDs.
//   kGemmStatic (opts bit 23; ungated launches with one unit per workgroup
//     that pass neither a status word nor a counter block only): unit =
//     blockIdx.x, no work-queue atomic.  A diagnostic of what the persistent
//     queue -- which gating, parking and relaunch need -- costs a solo launch
//     (scripts/gemm_shapes.py).  The path skips finish(), so a status word
//     would never be written; the host (gpbs_hip_gemm_bf16) therefore selects
//     it for direct calls alone, and a runner's launch, which always carries
//     its status word, keeps the queue whatever the opts say.  Measured
//     (profiles/r6/s61_gemm_shapes.jsonl): 4096^3 0.1130 -> 0.1052 ms (1216 ->
//     1306 TF/s; torch.mm 1475 on that box).  The queue costs ~8 us per launch:
//     each workgroup waits on three device-scope atomics with returns (its
//     grab, the grab that finds the queue empty, the exit count), a memory
//     round trip each, at the start and end of the kernel where nothing hides
//     them.  At 8192^3 (4 units per workgroup) the two tie.
constexpr int G2_BM = 256, G2_BK = 64, G2_NT = 512;
constexpr u32 kGemmXRange = 1u << 16;
constexpr u32 kGemmBlock2D = 1u << 17;
constexpr u32 kGemmStatic = 1u << 18;
// Host opts (gpbs_hip_set_gemm_opts): the dealing bits that are live, and the
// bits that used to select this schedule among its variants and are still
// accepted, so that a recorded `--gemm-opts 205064` means what it meant.
constexpr int kGemmOptsLive = 1 | 8 | 1 << 23;
constexpr int kGemmOptsShipped = 256 | 8192 | 65536 | 131072;
static int g_gemm_opts = 8;
constexpr int kG2Half = 128 * 128;           // bytes per half-tile
constexpr int kG2Buf = 4 * kG2Half;          // A0 A1 B0 B1
constexpr int kG2Lds = 2 * kG2Buf;           // 128 KiB

__device__ __forceinline__ int g2_swz(int r) { return (r >> 1) & 7; }

__global__ __launch_bounds__(G2_NT, 1) void k_gemm256_bf16_tn(const u16* __restrict__ A, const u16* __restrict__ Bt,
                                                             u16* __restrict__ C, int M, int N, int K, WorkQueue* q,
                                                             const PartTable* table, u32 mode, u32 me, u64* cnt,
                                                             u32 inst_per_tile, u32 refs_per_tile, u32 miss_per_tile,
                                                             u32* status) {
  __shared__ __attribute__((aligned(16))) char smem[kG2Lds + 16];
  lds_t* lds = (lds_t*)smem;
  int* s_slot = (int*)(smem + kG2Lds);
  const u32 xcc = xcc_id();
  u64 t_last = __builtin_amdgcn_s_memtime();
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wu = __builtin_amdgcn_readfirstlane(wid);  // wave-uniform: scalar branches on the group
  const int wr = wu >> 2, wc = wu & 3;
  const int tiles_m = M / G2_BM, tiles_n = N / G2_BM, ntiles = tiles_m * tiles_n;
  const int nt = K / G2_BK;
  // B staging: wave w's glds j writes 1 KiB chunk c = 2w + j of a half-tile =
  // rows 8c .. 8c+7; lane -> row 8c + lane/8, slot lane%8, source chunk
  // slot ^ swz(row).  Same offsets for either half.
  int soff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int row = 8 * (2 * wid + j) + (lane >> 3);
    soff[j] = row * K + (((lane & 7) ^ g2_swz(row)) * 8);
  }
  // own-A staging: wave wc of the group writes rows 32 wc .. 32 wc + 31 (4 glds)
  int soffa[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = 8 * (4 * (wid & 3) + j) + (lane >> 3);
    soffa[j] = row * K + (((lane & 7) ^ g2_swz(row)) * 8);
  }
  const int l16 = lane & 15, lq = lane >> 4;
  const int bh = wc >> 1, bc = (wc & 1) * 64;  // the B half this wave reads, its 64 columns within it
  int units_seen = 0;

  for (;;) {
    const int tile = (mode & kGemmStatic) ? (units_seen ? -1 : (int)blockIdx.x)
                     : (mode & kGemmXRange) ? grab_unit_x(q, table, mode, me, xcc, s_slot, (u32)ntiles)
                                            : grab_unit(q, table, mode, me, xcc, s_slot, (u32)ntiles);
    if (tile < 0) break;
    int tm = tile / tiles_n, tn = tile % tiles_n;
    if ((mode & kGemmBlock2D) && (tiles_m & 3) == 0 && (tiles_n & 1) == 0 && ntiles % kXcds == 0) {
      const int per = ntiles / kXcds;
      const int bm = tiles_m / 4, bn = tiles_n / 2;
      const int g = (mode & kGemmXRange) ? tile / per : tile % kXcds;
      const int jj = (mode & kGemmXRange) ? tile % per : tile / kXcds;
      tm = (g >> 1) * bm + jj / bn;
      tn = (g & 1) * bn + jj % bn;
    }
    const u16* Ab = A + (size_t)tm * G2_BM * K;
    const u16* Bb = Bt + (size_t)tn * G2_BM * K;
    // stage(kind, h, t): this wave's share of half h of K-tile t; kind 0 = A, 1 = B
    auto stage = [&](int kind, int h, int t) {
      const u16* src = (kind ? Bb : Ab) + (size_t)h * 128 * K + t * G2_BK;
      lds_t* dst = lds + (t & 1) * kG2Buf + (kind * 2 + h) * kG2Half + wid * 2048;
      glds16(src + soff[0], dst);
      glds16(src + soff[1], dst + 1024);
    };
    auto stage_own_a = [&](int t) {  // all of A half wr of K-tile t, by this group
      const u16* src = Ab + (size_t)wr * 128 * K + t * G2_BK;
      lds_t* dst = lds + (t & 1) * kG2Buf + wr * kG2Half + (wid & 3) * 4096;
#pragma unroll
      for (int j = 0; j < 4; ++j) glds16(src + soffa[j], dst + j * 1024);
    };
    // Fragment read: 16 rows starting at `r0` of half-tile (kind, h) of buffer
    // b, k-substep s (32 k): lane reads row r0 + l16, logical chunk 4s + lq.
    auto frag = [&](int b, int kind, int h, int r0, int s) -> bf16x8 {
      const int r = r0 + l16;
      const lds_t* p = lds + b * kG2Buf + (kind * 2 + h) * kG2Half + r * 128 + (((4 * s + lq) ^ g2_swz(r)) << 4);
      return *(const __attribute__((address_space(3))) bf16x8*)p;
    };
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // prologue: all of tile 0 from every wave, landed and visible
    stage(1, 0, 0); stage(1, 1, 0); stage(0, 0, 0); stage(0, 1, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();  // g1 runs one barrier behind
    bf16x8 a[4][2], b[4][2];
    for (int t = 0; t < nt; ++t) {
      const int buf = t & 1;
      const bool more = t + 1 < nt;
      // ---- R_A: B fragments (kept for both phases), A rows 0-63
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) b[j][s2] = frag(buf, 1, bh, bc + j * 16, s2);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) a[i][s2] = frag(buf, 0, wr, i * 16, s2);
      if (more) {
        stage(1, 0, t + 1); stage(1, 1, t + 1);
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
      // ---- M_A
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][s2], a[i][s2], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_s_barrier();
      // ---- R_B: A rows 64-127
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) a[i][s2] = frag(buf, 0, wr, 64 + i * 16, s2);
      if (more) {
        stage_own_a(t + 1);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // retires this group's B0/B1(t+1)
      }
      __builtin_amdgcn_s_barrier();
      // ---- M_B
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][s2], a[i][s2], acc[4 + i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the group's own A half of t+1 lands before its next R_A
      __builtin_amdgcn_s_barrier();
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();  // re-align the groups
    // ---- epilogue: C through LDS, full-line non-temporal stores
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = wr * 128 + i * 16 + l16;
        const int c8 = wc * 16 + j * 4 + lq;
        const u32 lo = (u32)f2bf(acc[i][j][0]) | ((u32)f2bf(acc[i][j][1]) << 16);
        const u32 hi = (u32)f2bf(acc[i][j][2]) | ((u32)f2bf(acc[i][j][3]) << 16);
        *(__attribute__((address_space(3))) u32x2*)(lds + m * 512 + ((c8 ^ (m & 15)) << 3)) = u32x2{lo, hi};
      }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int row = p * 16 + (tid >> 5), c16 = tid & 31;
      u32x4 v = *(const __attribute__((address_space(3))) u32x4*)(lds + row * 512 + (((2 * c16) ^ (row & 14)) << 3));
      if (row & 1) v = u32x4{v.z, v.w, v.x, v.y};
      u32x4* dst = (u32x4*)(C + (size_t)(tm * G2_BM + row) * N + tn * G2_BM + c16 * 8);
      __builtin_nontemporal_store(v, dst);
    }
    __syncthreads();  // the next tile's prologue restages buffer 0
    ++units_seen;
    if (!(mode & kGemmStatic)) count_unit(cnt, me, xcc, inst_per_tile, &t_last, refs_per_tile, miss_per_tile, q);
  }
  if (!(mode & kGemmStatic)) finish(q, status, (u32)ntiles);  // (static: the queue was never touched)
}

// ------------------------------------------------------------ HBM stream ---
// dst = src (float4 copy), 16 B per lane, 16 loads in flight per thread: one
// 256-thread workgroup per CU keeps 64 KiB of reads in flight (enough for
// HBM3E at ~2 us loaded latency) while occupying only one wave slot per SIMD,
// so a co-resident GEMM keeps its two waves/SIMD (VGPR budget 512/SIMD: GEMM
// 2x136 + stream 80 + reduce 64 + gemv 96 = 512 fits; the old 4 WG/CU grids did not).
constexpr int SNT = 256, SUNROLL = 16, RUNROLL = 6;

template <int U, bool NTS>
__global__ __launch_bounds__(SNT) void k_stream_copy(const f32x4* __restrict__ src, f32x4* __restrict__ dst,
                                                    u64 n4, u32 chunk4, WorkQueue* q, const PartTable* table, u32 mode,
                                                    u32 me, u64* cnt, u32* status) {
  __shared__ int s_slot[4];
  const u32 xcc = xcc_id();
  // Ownership is decided by thread 0 inside grab_unit (workgroup-uniform).
  u64 t_last = __builtin_amdgcn_s_memtime();
  const u32 nchunks = (u32)((n4 + chunk4 - 1) / chunk4);
  // 16 B/lane: one load + one store wave-instruction per 1 KiB moved; every
  // line is a fill (streaming, no reuse).
  const u64 lines = (u64)chunk4 * 16 / 128;
  const u64 inst = (u64)chunk4 * 2 / 64 + 8;
  for (;;) {
    const int c = grab_unit(q, table, mode, me, xcc, s_slot, nchunks);
    if (c < 0) break;
    const u64 base = (u64)c * chunk4;
    const u64 end = min(base + chunk4, n4);
    for (u64 i = base + threadIdx.x; i < end; i += (u64)SNT * U) {
      f32x4 v[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const u64 idx = i + (u64)k * SNT;
        if (idx < end) v[k] = __builtin_nontemporal_load(src + idx);
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const u64 idx = i + (u64)k * SNT;
        if (idx < end) {
          if constexpr (NTS)
            __builtin_nontemporal_store(v[k], dst + idx);
          else
            dst[idx] = v[k];
        }
      }
    }
    count_unit(cnt, me, xcc, inst, &t_last, 2 * lines, 2 * lines, q);
  }
  finish(q, status, nchunks);
}

// ------------------------------------------------- reduce-copy (all-reduce) -
// out = a + b on bf16 (the traffic shape of a ring all-reduce step: two reads
// and one write per element).  Used as the collective tenant on one GPU; on
// N > 1 GPUs the tenant issues RCCL all-reduce over xGMI instead.
// Variants (gpbs_hip_set_reduce_opts, swept by scripts/kbench.py): NT threads
// per workgroup, U 16-byte element pairs in flight per thread, non-temporal
// (streaming) loads / stores on or off.
template <int NT, int U, bool NTL, bool NTS>
__global__ __launch_bounds__(NT) void k_reduce_bf16(const u32x4* __restrict__ a, const u32x4* __restrict__ b,
                                                    u32x4* __restrict__ out, u64 n8, u32 chunk8, WorkQueue* q,
                                                    const PartTable* table, u32 mode, u32 me, u64* cnt,
                                                    u32* status) {
  __shared__ int s_slot[4];
  const u32 xcc = xcc_id();
  // Ownership is decided by thread 0 inside grab_unit (workgroup-uniform).
  u64 t_last = __builtin_amdgcn_s_memtime();
  const u32 nchunks = (u32)((n8 + chunk8 - 1) / chunk8);
  const u64 lines = (u64)chunk8 * 16 / 128;
  const u64 inst = (u64)chunk8 * 3 / 64 + (u64)chunk8 * 16 / 64;
  for (;;) {
    const int c = grab_unit(q, table, mode, me, xcc, s_slot, nchunks);
    if (c < 0) break;
    const u64 base = (u64)c * chunk8, end = min(base + chunk8, n8);
    for (u64 i = base + threadIdx.x; i < end; i += (u64)NT * U) {
      u32x4 x[U], y[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const u64 idx = i + (u64)k * NT;
        if (idx < end) {
          if constexpr (NTL) {
            x[k] = __builtin_nontemporal_load(a + idx);
            y[k] = __builtin_nontemporal_load(b + idx);
          } else {
            x[k] = a[idx];
            y[k] = b[idx];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const u64 idx = i + (u64)k * NT;
        if (idx >= end) continue;
        const u32* px = (const u32*)&x[k];
        const u32* py = (const u32*)&y[k];
        u32x4 r;
        u32* pr = (u32*)&r;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const float lo = bf2f((u16)(px[w] & 0xffff)) + bf2f((u16)(py[w] & 0xffff));
          const float hi = bf2f((u16)(px[w] >> 16)) + bf2f((u16)(py[w] >> 16));
          pr[w] = (u32)f2bf(lo) | ((u32)f2bf(hi) << 16);
        }
        if constexpr (NTS)
          __builtin_nontemporal_store(r, out + idx);
        else
          out[idx] = r;
      }
    }
    count_unit(cnt, me, xcc, inst, &t_last, 3 * lines, 3 * lines, q);
  }
  finish(q, status, nchunks);
}

// --------------------------------------------------------------- GEMV -----
// y[R] = W[R][K] x[K] (bf16 in, fp32 out): the latency-critical "idle" tenant
// request (a decode-step sized matvec).  A wave owns 4 rows; each lane streams
// 16 B per row per 512-column chunk straight into VGPRs, GV_U chunks (4 rows
// x GV_U W loads + GV_U x loads) in flight before the first use -- no LDS
// round trip, no per-load guards (rows past R are clamped, not branched).
constexpr int GV_U = 2;

__device__ __forceinline__ float dot8(const u32x4 w, const u32x4 v) {
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s += __uint_as_float(w[e] << 16) * __uint_as_float(v[e] << 16);
    s += __uint_as_float(w[e] & 0xffff0000u) * __uint_as_float(v[e] & 0xffff0000u);
  }
  return s;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_gemv_bf16(const u16* __restrict__ W, const u16* __restrict__ x,
                                                  float* __restrict__ y, int R, int K, WorkQueue* q,
                                                  const PartTable* table, u32 mode, u32 me, u64* cnt,
                                                  u32* status) {
  __shared__ int s_slot[4];
  if (mode & GATE_WAVEPRIO) __builtin_amdgcn_s_setprio(3);
  const u32 xcc = xcc_id();
  // Ownership is decided by thread 0 inside grab_unit (workgroup-uniform).
  u64 t_last = __builtin_amdgcn_s_memtime();
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const u32 nchunks = (u32)((R + 15) / 16);  // 16 rows per unit (4 per wave)
  const u64 lines = (u64)16 * K * 2 / 128;
  const int nk = K / 512;  // 512 columns per wave-wide chunk (8 per lane)
  const u32x4* xv = (const u32x4*)x;
  for (;;) {
    const int c = grab_unit(q, table, mode, me, xcc, s_slot, nchunks);
    if (c < 0) break;
    const int row0 = c * 16 + wid * 4;
    const u32x4* wr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) wr[r] = (const u32x4*)(W + (size_t)min(row0 + r, R - 1) * K);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int kc = 0;
    for (; kc + GV_U <= nk; kc += GV_U) {
      u32x4 xr[GV_U], wv[GV_U][4];
#pragma unroll
      for (int u = 0; u < GV_U; ++u) {
        const int k = (kc + u) * 64 + lane;
        xr[u] = xv[k];
#pragma unroll
        for (int r = 0; r < 4; ++r) wv[u][r] = __builtin_nontemporal_load(wr[r] + k);
      }
#pragma unroll
      for (int u = 0; u < GV_U; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] += dot8(wv[u][r], xr[u]);
    }
    for (; kc < nk; ++kc) {
      const int k = kc * 64 + lane;
      const u32x4 xr = xv[k];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] += dot8(__builtin_nontemporal_load(wr[r] + k), xr);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = acc[r];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == 0 && row0 + r < R) y[row0 + r] = s;
    }
    count_unit(cnt, me, xcc, (u64)16 * (K / 512 + 8), &t_last, lines, lines, q);
  }
  finish(q, status, nchunks);
}

// ------------------------------------------------------------- census ------
// Records (XCC_ID, HW_ID) per workgroup: verifies the workgroup->XCD dealing
// and that XCD gating confines a kernel to its partitions.
__global__ void k_census(u32* out, const PartTable* table, u32 mode, u32 me) {
  const u32 xcc = xcc_id();
  const bool ok = owns(table, mode, me, xcc);
  if (threadIdx.x == 0) {
    out[blockIdx.x * 4 + 0] = xcc;
    out[blockIdx.x * 4 + 1] = hw_id();
    out[blockIdx.x * 4 + 2] = ok ? 1u : 0u;
    out[blockIdx.x * 4 + 3] = 0xC0FFEEu;
  }
  if (ok) {  // keep the workgroup resident a little so dealing is visible
    u64 t = __builtin_amdgcn_s_memtime();
    while (__builtin_amdgcn_s_memtime() - t < 2000) __builtin_amdgcn_s_sleep(1);
  }
}

}  // namespace gpbs_hip

// ---------------------------------------------------------------- C ABI ----
using namespace gpbs_hip;

extern "C" {

// Sets the 256x256 kernel's tile dealing (kGemmOptsLive; opts < 0 only
// queries) and returns the previous value.  The bits that spell the shipped
// schedule are accepted; any other bit named a variant that now lives in
// docs/gemm_lab.md and is ignored, with one line on stderr per process.
int gpbs_hip_set_gemm_opts(int opts) {
  const int old = g_gemm_opts;
  if (opts < 0) return old;
  const int gone = opts & ~(kGemmOptsLive | kGemmOptsShipped);
  static bool warned = false;
  if (gone && !warned) {
    warned = true;
    fprintf(stderr,
            "gpbs_hip_set_gemm_opts: bits 0x%x select GEMM variants that were removed (docs/gemm_lab.md); "
            "the shipped schedule runs\n",
            gone);
  }
  g_gemm_opts = opts & kGemmOptsLive;
  return old;
}

int gpbs_hip_gemm_units(int M, int N) {
  if (M % G2_BM == 0 && N % G2_BM == 0) return (M / G2_BM) * (N / G2_BM);
  return (M / GBM) * (N / GBN);
}

int gpbs_hip_gemm_bf16(const void* A, const void* Bt, void* C, int M, int N, int K, void* q, const void* table,
                       unsigned mode, unsigned me, void* cnt, void* status, int grid, hipStream_t s) {
  if (M % GBM || N % GBN || K % GBK || M <= 0 || N <= 0 || K <= 0) return -22;
  if (M % G2_BM == 0 && N % G2_BM == 0) {
    const int ntiles = (M / G2_BM) * (N / G2_BM);
    if (grid <= 0) grid = 256;  // one workgroup per CU
    if (grid > ntiles) grid = ntiles;
    const u32 inst = (u32)((G2_BM / 16) * (G2_BM / 16) * (K / 32) + (K / G2_BK) * 64 + 128);
    const u32 refs = (u32)(((u64)2 * G2_BM * K * 2) / 128);
    const u32 miss = (u32)((((u64)M + N) * K * 2 / 128) / ntiles + (u64)G2_BM * G2_BM * 2 / 128);
    const u32 m2 = mode | ((g_gemm_opts & 1) ? kGemmXRange : 0u) |
                   ((g_gemm_opts & 8) && ntiles % kXcds == 0 ? kGemmBlock2D : 0u) |
                   ((g_gemm_opts & (1 << 23)) && (mode & 3) == GATE_NONE && grid == ntiles && !status && !cnt
                        ? kGemmStatic : 0u);
    hipLaunchKernelGGL(k_gemm256_bf16_tn, dim3(grid), dim3(G2_NT), 0, s, (const u16*)A, (const u16*)Bt, (u16*)C, M, N,
                       K, (WorkQueue*)q, (const PartTable*)table, m2, me, (u64*)cnt, inst, refs, miss, (u32*)status);
    return hipGetLastError() == hipSuccess ? 0 : -5;
  }
  const int ntiles = (M / GBM) * (N / GBN);
  if (grid <= 0) grid = 256 * 2;
  if (grid > ntiles) grid = ntiles;
  // Model: per tile 8192 MFMA + ds_read/glds/epilogue issue; refs = A+B
  // panels in 128-B lines; fills = compulsory bytes spread over the tiles.
  const u32 inst = (u32)((GBM / 16) * (GBN / 16) * (K / 32) * 2 + (K / GBK) * 32 + 64);
  const u32 refs = (u32)(((u64)(GBM + GBN) * K * 2) / 128);
  const u32 miss = (u32)((((u64)M + N) * K * 2 / 128) / ntiles + (u64)GBM * GBN * 2 / 128);
  hipLaunchKernelGGL(k_gemm_bf16_tn, dim3(grid), dim3(GNT), 0, s, (const u16*)A, (const u16*)Bt, (u16*)C, M, N, K,
                     (WorkQueue*)q, (const PartTable*)table, mode, me, (u64*)cnt, inst, refs, miss, (u32*)status);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

static int g_stream_opts = 0;

// bit 0: temporal stores; bit 1: 8 (not 16) loads in flight per thread.
int gpbs_hip_set_stream_opts(int opts) {
  const int old = g_stream_opts;
  if (opts >= 0) g_stream_opts = opts;
  return old;
}

int gpbs_hip_stream_copy(const void* src, void* dst, unsigned long long bytes, unsigned chunk_bytes, void* q,
                         const void* table, unsigned mode, unsigned me, void* cnt, void* status, int grid, hipStream_t s) {
  if (bytes % 16 || chunk_bytes % 16 || chunk_bytes == 0) return -22;
  if (grid <= 0) grid = 256;  // one workgroup per CU (see SUNROLL)
  using K = void (*)(const f32x4*, f32x4*, u64, u32, WorkQueue*, const PartTable*, u32, u32, u64*, u32*);
  static const K tab[4] = {k_stream_copy<SUNROLL, true>, k_stream_copy<SUNROLL, false>, k_stream_copy<8, true>,
                           k_stream_copy<8, false>};
  hipLaunchKernelGGL(tab[g_stream_opts & 3], dim3(grid), dim3(SNT), 0, s, (const f32x4*)src, (f32x4*)dst, bytes / 16,
                     chunk_bytes / 16, (WorkQueue*)q, (const PartTable*)table, mode, me, (u64*)cnt, (u32*)status);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// Default: 6 pairs in flight, streaming (non-temporal) loads, TEMPORAL
// stores: 5.57-5.76 TB/s vs 5.02-5.13 with non-temporal stores and 5.84 for
// torch.add on the same box (profiles/kbench_r2.jsonl); unroll depth and
// 512-thread workgroups are within noise.
static int g_reduce_opts = 8;

// bits 0-1: in-flight pairs per thread 6 / 8 / 4 / 12; bit 2: temporal loads;
// bit 3: temporal stores; bit 4: 512-thread workgroups.  Returns the old value.
int gpbs_hip_set_reduce_opts(int opts) {
  const int old = g_reduce_opts;
  if (opts >= 0) g_reduce_opts = opts;
  return old;
}

int gpbs_hip_reduce_bf16(const void* a, const void* b, void* out, unsigned long long bytes, unsigned chunk_bytes,
                         void* q, const void* table, unsigned mode, unsigned me, void* cnt, void* status, int grid, hipStream_t s) {
  if (bytes % 16 || chunk_bytes % 16 || chunk_bytes == 0) return -22;
  if (grid <= 0) grid = 256;
  using K = void (*)(const u32x4*, const u32x4*, u32x4*, u64, u32, WorkQueue*, const PartTable*, u32, u32, u64*, u32*);
#define RV(NT, U) {k_reduce_bf16<NT, U, true, true>, k_reduce_bf16<NT, U, false, true>, \
                   k_reduce_bf16<NT, U, true, false>, k_reduce_bf16<NT, U, false, false>}
  static const K table256[4][4] = {RV(256, 6), RV(256, 8), RV(256, 4), RV(256, 12)};
  static const K table512[4][4] = {RV(512, 6), RV(512, 8), RV(512, 4), RV(512, 12)};
#undef RV
  const int o = g_reduce_opts;
  const int nt = (o & 16) ? 512 : 256;
  const K kern = ((o & 16) ? table512 : table256)[o & 3][((o >> 2) & 1) | (((o >> 3) & 1) << 1)];
  hipLaunchKernelGGL(kern, dim3(grid), dim3(nt), 0, s, (const u32x4*)a, (const u32x4*)b, (u32x4*)out,
                     bytes / 16, chunk_bytes / 16, (WorkQueue*)q, (const PartTable*)table, mode, me, (u64*)cnt, (u32*)status);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int gpbs_hip_gemv_bf16(const void* W, const void* x, void* y, int R, int K, void* q, const void* table, unsigned mode,
                       unsigned me, void* cnt, void* status, int grid, hipStream_t s) {
  if (K % 512 || R <= 0) return -22;
  if (grid <= 0) grid = (R + 15) / 16;
  if (grid > 256) grid = 256;
  hipLaunchKernelGGL(k_gemv_bf16, dim3(grid), dim3(256), 0, s, (const u16*)W, (const u16*)x, (float*)y, R, K,
                     (WorkQueue*)q, (const PartTable*)table, mode, me, (u64*)cnt, (u32*)status);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

int gpbs_hip_census(void* out, int blocks, const void* table, unsigned mode, unsigned me, hipStream_t s) {
  hipLaunchKernelGGL(k_census, dim3(blocks), dim3(64), 0, s, (u32*)out, (const PartTable*)table, mode, me);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // extern "C"
