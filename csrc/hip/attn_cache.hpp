// The KV-cache forms of the attention path (decode_kernels.hip, prefill_kernels.hip).
//
// The write kernels of both files are each one template over a cache view; the
// uniform, _seq, _paged and _paged_kv8 kernels are wrappers that build their view
// and call it.  (The attention kernels keep their text in decode_attn_body.hpp
// and prefill_attn_body.hpp, included once per form: the .hip files say why.
// They follow the same rules, with seq_tokens and page_or0 from here.)
// A view is a few integers and answers the questions on which the forms differ:
// how many rows a sequence may hold and which of its tokens are live, where
// logical row r of sequence b is, and how a row is stored.  Everything else is
// shared text, so an active sequence gets the same bits from every form.  The
// views hold no pointers: the tensors stay __restrict__ parameters of the
// kernels, which hand them to the templates as they are.
//
//   DenseUniform  caches [B, Hkv, C, hd], one position for the whole batch.
//   DenseSeq      the same caches, one position (and, for prefill, one length)
//                 per sequence, int32 [B]: sequence b is active iff
//                 0 <= pos[b] < C, any other value is an idle slot.  An idle
//                 sequence writes no cache row, loads none, and its q / out rows
//                 are zero bits; an active one computes exactly what the uniform
//                 kernel computes at pos = pos[b].
//   Paged         DenseSeq over pools [P, Hkv, page, hd] and an int32 block table
//                 [B, NP]: logical row r of sequence b lives in page
//                 table[b, r / page] at page row r % page, page in 64/128/256,
//                 and Cl = NP * page takes the place of C.  An entry outside
//                 [0, P) never forms an address outside the pools: a write
//                 through it is dropped (locate), reads through it come from
//                 page 0 (page_or0).
//   PagedKv8      Paged over an fp8 cache (kv8_codec.hpp): e4m3 code pools
//                 [P, Hkv, page, hd] of one byte per element and fp32 scales
//                 [P, Hkv, page], one power of two per cached row and KV head.
//                 A stored row is the quantised row the bf16 kernel would have
//                 stored; a loaded piece is rebuilt into the very bf16 words the
//                 dequantised pools hold (code times scale rounds nowhere).  The
//                 out-of-range rule covers all four tensors.
#ifndef GPBS_HIP_ATTN_CACHE_HPP
#define GPBS_HIP_ATTN_CACHE_HPP

#include "common.hpp"
#include "kv8_codec.hpp"

namespace gpbs_hip {

constexpr int kHd = 128;  // head_dim of every Llama-3 size, and the only one the attention kernels take

// Threads of a write kernel's workgroup.  The write templates stride by this
// constant, not by blockDim.x: read inside an inlined template, blockDim.x
// compiles to the general lookup (a dependent global load in the prologue)
// where the kernel itself gets the launch-bounds shortcut.  A write kernel is
// therefore right only when launched with kWriteThreads threads a workgroup (any
// other block size would skip or repeat pieces); launch_write (attn_entry.hpp)
// is the one place that launches them.
constexpr int kWriteThreads = 256;

// a block-table entry as a page to read: anything outside [0, P) is page 0
__device__ __forceinline__ int page_or0(int e, int P) { return (e >= 0 && e < P) ? e : 0; }

// tokens that sequence b really has in a ragged launch of S (0: idle slot)
__device__ __forceinline__ int seq_tokens(int pos, int len, int S, int C) {
  return (pos < 0 || pos >= C || len <= 0) ? 0 : min(min(len, S), C - pos);
}

// ---- how a row is stored: bf16 words, or e4m3 codes plus one scale per row ----

struct Bf16Rows {
  typedef u32x4 Piece;  // pool element: 8 elements of a row
  // piece c of a row of per_head pieces
  static __device__ __forceinline__ void store(u32x4 v, Piece* pool, float*, size_t row, int c, int per_head) {
    pool[row * per_head + c] = v;
  }
};

struct Fp8Rows {
  typedef u32x2 Piece;  // pool element: the 8 codes of 8 elements of a row
  // hd = 128 only; the 16 lanes that hold the row call this together (kv8_store_row)
  static __device__ __forceinline__ void store(u32x4 v, Piece* pool, float* scales, size_t row, int c, int) {
    kv8_store_row(v, pool, scales, row, c);
  }
};

// ---- where rows are: a cache is blocks of [Hkv, block rows, hd] ----
//
// rows()        the most rows a sequence can hold (C, or Cl = NP * page)
// tokens()      prefill: the tokens sequence b really has in a launch of S
// locate()      for a write: where logical row pos + s of sequence b is (Where:
//               its block, its place in it, and ok: false if the write is to be
//               dropped)
// row()         that row of KV head kvh as an index into the cache tensors

struct DenseUniform : Bf16Rows {
  static constexpr bool kPerSeq = false;
  int C;
  __device__ __forceinline__ explicit DenseUniform(int C) : C(C) {}
  __device__ __forceinline__ int rows() const { return C; }
  // a sequence's cache is one block of C rows; no write is dropped
  struct Where {
    int blk, pos, s;
    static constexpr bool ok = true;
  };
  __device__ __forceinline__ Where locate(const int*, int b, int pos, int s) const { return {b, pos, s}; }
  __device__ __forceinline__ size_t row(const Where& w, int Hkv, int kvh) const {
    return ((size_t)w.blk * Hkv + kvh) * C + w.pos + w.s;
  }
};

struct DenseSeq : DenseUniform {
  static constexpr bool kPerSeq = true;
  using DenseUniform::DenseUniform;
  __device__ __forceinline__ int tokens(int pos, int len, int S) const { return seq_tokens(pos, len, S, C); }
};

template <class Rows>
struct PagedCache : Rows {
  static constexpr bool kPerSeq = true;
  int NP, P, psh;  // table width, pool pages, log2(page)
  __device__ __forceinline__ PagedCache(int NP, int P, int psh) : NP(NP), P(P), psh(psh) {}
  __device__ __forceinline__ int rows() const { return NP << psh; }
  __device__ __forceinline__ int tokens(int pos, int len, int S) const { return seq_tokens(pos, len, S, rows()); }
  // writes: an entry outside [0, P) drops the row
  // the page and page row; an entry outside [0, P) drops the write
  struct Where {
    int blk, brow;
    bool ok;
  };
  __device__ __forceinline__ Where locate(const int* table, int b, int pos, int s) const {
    const int r = pos + s, pg = table[(size_t)b * NP + (r >> psh)];
    return {pg, r & ((1 << psh) - 1), pg >= 0 && pg < P};
  }
  __device__ __forceinline__ size_t row(const Where& w, int Hkv, int kvh) const {
    return (((size_t)w.blk * Hkv + kvh) << psh) + w.brow;
  }
};

typedef PagedCache<Bf16Rows> Paged;
typedef PagedCache<Fp8Rows> PagedKv8;

}  // namespace gpbs_hip

#endif  // GPBS_HIP_ATTN_CACHE_HPP
