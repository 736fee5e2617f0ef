"""Torch-facing wrappers of the Llama tenant kernels (csrc/hip/llm_kernels.hip).

Inference-only (no autograd): the decode path of ``LlamaDecoder``.  The
library must load on a GPU box -- shape/dtype violations raise instead of
falling back to eager PyTorch.
"""
from __future__ import annotations

import ctypes as C
import operator
from typing import Optional

import torch

from .kernels import _check, _ptr, _stream, gemm_fp8, gemm_mxfp4, lib


def _need(t: torch.Tensor, what: str):
    if not (t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()):
        raise ValueError(f"{what}: need a contiguous bf16 CUDA tensor, got {t.dtype} {t.device} "
                         f"contiguous={t.is_contiguous()}")


def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """y = x * rsqrt(mean(x^2, -1) + eps) * w (fp32 statistics)."""
    x = x.contiguous()
    _need(x, "rmsnorm x")
    w = w.to(torch.bfloat16).contiguous()
    dim = x.shape[-1]
    if w.numel() != dim or dim % 8:
        raise ValueError(f"rmsnorm: weight {tuple(w.shape)} vs dim {dim} (dim % 8 == 0 required)")
    y = torch.empty_like(x)
    _check(lib().gpbs_hip_rmsnorm_bf16(_ptr(x), _ptr(w), _ptr(y), x.numel() // dim, dim, C.c_float(eps),
                                       _stream()), "rmsnorm_bf16")
    return y


def swiglu(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """y = silu(a) * b."""
    a, b = a.contiguous(), b.contiguous()
    _need(a, "swiglu a")
    _need(b, "swiglu b")
    if a.shape != b.shape or a.numel() % 8:
        raise ValueError(f"swiglu: shapes {tuple(a.shape)} / {tuple(b.shape)}")
    y = torch.empty_like(a)
    _check(lib().gpbs_hip_swiglu_bf16(_ptr(a), _ptr(b), _ptr(y), a.numel(), _stream()), "swiglu_bf16")
    return y


def rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: int) -> torch.Tensor:
    """Rotary embedding on interleaved pairs; x [B, S, H, hd], cos/sin fp32
    [max_seq, hd/2]; token s gets angle row pos + s."""
    x = x.contiguous()
    _need(x, "rope x")
    B, S, H, hd = x.shape
    if cos.dtype != torch.float32 or cos.shape[-1] * 2 != hd or pos + S > cos.shape[0]:
        raise ValueError(f"rope: tables {tuple(cos.shape)} {cos.dtype} for hd={hd}, pos={pos}, S={S}")
    y = torch.empty_like(x)
    _check(lib().gpbs_hip_rope_bf16(_ptr(x), _ptr(y), _ptr(cos.contiguous()), _ptr(sin.contiguous()), B, S, H, hd,
                                    int(pos), _stream()), "rope_bf16")
    return y



def rope_dpos(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos_t: torch.Tensor) -> torch.Tensor:
    """rope() with the start position in a 1-element int32 CUDA tensor (read by
    the kernel at run time: valid inside a captured graph).  No bounds check on
    the device value: the caller keeps pos + S <= cos.shape[0]."""
    x = x.contiguous()
    _need(x, "rope x")
    B, S, H, hd = x.shape
    if cos.dtype != torch.float32 or cos.shape[-1] * 2 != hd or pos_t.dtype != torch.int32 or not pos_t.is_cuda:
        raise ValueError(f"rope_dpos: tables {tuple(cos.shape)} {cos.dtype}, pos {pos_t.dtype} {pos_t.device}")
    y = torch.empty_like(x)
    _check(lib().gpbs_hip_rope_bf16_dpos(_ptr(x), _ptr(y), _ptr(cos), _ptr(sin), B, S, H, hd, _ptr(pos_t),
                                         _stream()), "rope_bf16_dpos")
    return y


def prefill_attn_ref(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, pos: int) -> torch.Tensor:
    """Plain-torch reference of prefill_attn for any head_dim / group size (runs
    on CPU too): fp32 compute, fp64 for fp64 inputs, grouped per KV head without
    repeating K/V, mask key <= pos + s.  Returns [B, S, H * hd] in the compute
    dtype."""
    B, S, H, hd = q.shape
    Hkv, Cn = kc.shape[1], kc.shape[2]
    if kc.shape[0] != B or kc.shape[3] != hd or vc.shape != kc.shape or H % Hkv or pos < 0 or pos + S > Cn:
        raise ValueError(f"prefill_attn_ref: q {tuple(q.shape)}, cache {tuple(kc.shape)}, pos={pos}")
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    L, G = pos + S, H // Hkv
    qg = q.to(ct).view(B, S, Hkv, G, hd).permute(0, 2, 3, 1, 4)  # [B, Hkv, G, S, hd]
    k, v = kc[:, :, :L].to(ct), vc[:, :, :L].to(ct)
    sc = torch.matmul(qg, k.transpose(-1, -2).unsqueeze(2)) * (hd ** -0.5)  # [B, Hkv, G, S, L]
    seen = torch.arange(L, device=q.device)[None, :] <= pos + torch.arange(S, device=q.device)[:, None]
    sc = sc.masked_fill(~seen, float("-inf"))
    o = torch.matmul(torch.softmax(sc, -1), v.unsqueeze(2))  # [B, Hkv, G, S, hd]
    return o.permute(0, 3, 1, 2, 4).reshape(B, S, H * hd)


# --------------------------------------------------------------------------- per-sequence positions (ragged batches)
# Slot rules, applied by the kernels themselves on the device values:
#   decode   sequence b is active iff 0 <= pos[b] < C; it writes row pos[b] and
#            attends rows 0 .. pos[b].  Any other value is an idle slot.
#   prefill  sequence b has n_b = min(len[b], S, C - pos[b]) new tokens at rows
#            pos[b] .. pos[b] + n_b - 1; n_b = 0 if pos[b] < 0, pos[b] >= C or
#            len[b] <= 0.
# An idle slot / a padding token writes nothing to the caches and gets zero q
# and output rows.
def seq_tokens(pos: int, length: int, S: int, Cn: int) -> int:
    """n_b of the prefill slot rule (the host twin of the kernels' clamp)."""
    pos, length = int(pos), int(length)
    return 0 if pos < 0 or pos >= Cn or length <= 0 else min(length, S, Cn - pos)


def attn_seq_ref(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, pos, lens) -> torch.Tensor:
    """Plain-torch reference of prefill_attn_seq (and, with S = 1 and lens = 1
    for the active slots, of decode_attn_seq); runs on the CPU.  pos / lens are
    B ints each (lists or tensors).  prefill_attn_ref per sequence on its
    n_b tokens, zeros for rows >= n_b; [B, S, H * hd] in the compute dtype of
    prefill_attn_ref."""
    B, S, H, hd = q.shape
    Cn = kc.shape[2]
    pos = [int(p) for p in (pos.tolist() if isinstance(pos, torch.Tensor) else pos)]
    lens = [int(n) for n in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
    if len(pos) != B or len(lens) != B:
        raise ValueError(f"attn_seq_ref: {len(pos)} positions / {len(lens)} lengths for a batch of {B}")
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    out = torch.zeros(B, S, H * hd, dtype=ct, device=q.device)
    for b in range(B):
        n = seq_tokens(pos[b], lens[b], S, Cn)
        if n:
            out[b, :n] = prefill_attn_ref(q[b:b + 1, :n], kc[b:b + 1], vc[b:b + 1], pos[b])[0]
    return out


# --------------------------------------------------------------------------- paged KV cache (block-table kernels)
# The _seq kernels over pools kpool / vpool bf16 [P, Hkv, page, 128] and an int32
# block table [B, NP] on the device: logical row r of sequence b lives in page
# table[b, r // page] at page row r % page.  Cl = NP * page takes the place of C
# in the slot rules above.  The kernels read only the table entries of pages
# that hold rows 0 .. pos[b] (decode) or 0 .. pos[b] + n_b - 1 (prefill): the
# tail of a table row, and the whole row of an idle slot, may hold anything.  A
# read entry outside [0, P) forms no address outside the pools: the write
# through it is dropped, the reads through it come from page 0.
PAGE_SIZES = (64, 128, 256)


def paged_gather(pool: torch.Tensor, table_row, rows: int) -> torch.Tensor:
    """Logical rows 0 .. rows - 1 of one sequence as a dense [Hkv, rows, hd]
    tensor: row r is pool[table_row[r // page], :, r % page].  Plain torch, any
    device; only the first ceil(rows / page) entries of table_row are read."""
    P, Hkv, page, hd = pool.shape
    n = -(-rows // page)
    ids = [int(e) for e in (table_row.tolist() if isinstance(table_row, torch.Tensor) else table_row)][:n]
    if len(ids) < n or any(not 0 <= e < P for e in ids):
        raise ValueError(f"paged_gather: {rows} rows need {n} table entries in [0, {P}), got {ids}")
    if not n:
        return pool.new_zeros(Hkv, 0, hd)
    idx = torch.tensor(ids, dtype=torch.long, device=pool.device)
    return pool[idx].permute(1, 0, 2, 3).reshape(Hkv, n * page, hd)[:, :rows]


def attn_paged_ref(q: torch.Tensor, kpool: torch.Tensor, vpool: torch.Tensor, table, pos, lens) -> torch.Tensor:
    """Plain-torch reference of prefill_attn_paged (and, with S = 1 and lens = 1
    for the active slots, of decode_attn_paged): each active sequence's rows
    gathered into dense caches of Cl = NP * page rows, then attn_seq_ref."""
    B, S, H, hd = q.shape
    P, Hkv, page, _ = kpool.shape
    table = torch.as_tensor(table)
    NP = table.shape[1]
    Cl = NP * page
    pos = [int(p) for p in (pos.tolist() if isinstance(pos, torch.Tensor) else pos)]
    lens = [int(n) for n in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
    kc, vc = kpool.new_zeros(B, Hkv, Cl, hd), vpool.new_zeros(B, Hkv, Cl, hd)
    for b in range(B):
        n = seq_tokens(pos[b], lens[b], S, Cl)
        if n:
            kc[b, :, :pos[b] + n] = paged_gather(kpool, table[b], pos[b] + n)
            vc[b, :, :pos[b] + n] = paged_gather(vpool, table[b], pos[b] + n)
    return attn_seq_ref(q, kc, vc, pos, lens)


# --------------------------------------------------------------------------- fp8 paged KV cache (the _kv8 kernels)
# The paged kernels over e4m3 pools: kpool8 / vpool8 float8_e4m3fn [P, Hkv, page, 128] and kscale / vscale fp32
# [P, Hkv, page], one power-of-two scale per cached row and KV head; 132 bytes per row and head where bf16 stores
# 256.  Table, page sizes, slot rules and the out-of-range rule are the paged ones: an entry outside [0, P) forms no
# address outside any of the four tensors, its write is dropped (codes and scale), its reads come from page 0.
#
# The codec, for a row x[128] of finite bf16 values (inf, NaN and bf16 subnormals are outside the contract):
#   amax = max |x|; (m, ex) = frexp(amax), m in [0.5, 1); e = ex - 9 if m <= 0.875 else ex - 8, clamped to
#   e >= -100; e = 0 if amax == 0; scale = 2^e; code = e4m3fn(x * 2^-e), round to nearest even.
# amax / scale lies in (224, 448], so nothing saturates; x * 2^-e is exact in fp32; float(code) * scale is exact and
# representable in bf16, so dequantisation rounds nowhere and a kernel over the fp8 pools can be held, bit for bit,
# to the bf16 _paged kernel over the dequantised pools.  The error per element is at most 16 * scale < amax / 14.
# The codec is not idempotent in the scale (an amax that rounds down to 224 * scale gets half the scale on a second
# pass): nothing may rely on requantising.
def kv8_quant_ref(x: torch.Tensor):
    """The fp8 KV-cache codec, plain torch on any device: x [..., 128] (any last
    dimension) -> (codes float8_e4m3fn of x's shape, scale fp32 [...]).  The
    exponent is taken from the bits of amax, which is frexp without a
    transcendental on any device."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    bits = amax.view(torch.int32)
    # amax = (1 + mant / 2^23) * 2^(E - 127): ex = E - 126, and m <= 0.875 iff mant <= 0.75 * 2^23
    E, mant = bits >> 23, bits & 0x7FFFFF
    e = (E - 126 - torch.where(mant <= 0x600000, 9, 8)).clamp(min=-100)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    scale = ((e + 127) << 23).to(torch.int32).view(torch.float32)
    inv = ((127 - e) << 23).to(torch.int32).view(torch.float32)
    return (xf * inv.unsqueeze(-1)).to(torch.float8_e4m3fn), scale


def kv8_dequant(codes: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """float(code) * scale as bf16 (exact for what kv8_quant_ref produced)."""
    return (codes.float() * scale.unsqueeze(-1)).to(torch.bfloat16)


def kv8_round(x: torch.Tensor) -> torch.Tensor:
    """x [..., hd] rounded row by row through the codec, in x's dtype: what a read
    of the fp8 cache returns for a row written as x."""
    return kv8_dequant(*kv8_quant_ref(x)).to(x.dtype)


def kv8_emulate_rows(kpool: torch.Tensor, vpool: torch.Tensor, table: torch.Tensor, pos_t: torch.Tensor,
                     len_t: Optional[torch.Tensor] = None, S: int = 1):
    """The fp8 cache emulated on bf16 pools: after a paged write launch
    (qkv_rope_cache_paged with len_t None, qkv_rope_cache_prefill_paged of S
    tokens otherwise), round exactly the rows it wrote through the codec, in
    place, with torch ops on the pools' device.  The rows are those of the paged
    slot rule: tokens s < n_b of sequence b whose table entry lies in [0, P)."""
    P, Hkv, page, hd = kpool.shape
    B, NP = table.shape
    Cl = NP * page
    pos = pos_t.long()
    n = torch.ones_like(pos) if len_t is None else len_t.long().clamp(max=S)
    n = torch.where((pos >= 0) & (pos < Cl) & (n > 0), torch.minimum(n, Cl - pos), torch.zeros_like(n))
    s = torch.arange(S, device=pos.device)
    r = (pos[:, None] + s[None, :]).clamp(0, Cl - 1)
    pg = torch.gather(table.long(), 1, r // page)
    valid = (s[None, :] < n[:, None]) & (pg >= 0) & (pg < P)
    pgv, prv = pg[valid], (r % page)[valid]
    for pool in (kpool, vpool):
        pool[pgv, :, prv] = kv8_round(pool[pgv, :, prv])  # [rows, Hkv, hd]


def attn_paged_kv8_ref(q: torch.Tensor, kpool8: torch.Tensor, vpool8: torch.Tensor, kscale: torch.Tensor,
                       vscale: torch.Tensor, table, pos, lens) -> torch.Tensor:
    """Plain-torch reference of the two _kv8 attention kernels: attn_paged_ref
    over the dequantised pools."""
    return attn_paged_ref(q, kv8_dequant(kpool8, kscale), kv8_dequant(vpool8, vscale), table, pos, lens)


# --------------------------------------------------------------------------- cache views (csrc/hip/attn_cache.hpp)
# The attention block of a layer is two launches: "write" splits the packed qkv, applies RoPE to q and k and stores
# k / v into the cache; "attend" runs grouped-query attention of the new tokens over it.  Each exists for one new
# token per sequence (decode_kernels.hip) and for S of them (prefill_kernels.hip), and in the four cache forms of
# attn_cache.hpp.  The classes below are the host side of those forms.  A view holds the cache tensors of one layer
# (`cache`, in the order of the C ABI, named `names` in messages) and what addresses them, and answers only what the
# forms differ in:
#   entry                   (name in messages, library symbol) of its four entry points, indexed by WRITE_DECODE ..
#   check(what, S, attend)  its host-side checks (type, dtype, rank, sizes, strides; no device, no device value) for
#                           a decode launch (S None) or a prefill launch of S new tokens, `attend` for the attention
#                           launch; returns (B, Hkv, hd, rows) with rows = C or NP * page per sequence
#   args(S)                 its part of an entry point's arguments: the names and the device tensors that address the
#                           cache, the geometry before hd, the host position after it
#   wrote(S)                if not None, runs after the write launch
# Everything else (q / qkv, the RoPE tables, nsplit, the workspace, the result, the call) is in write_decode /
# attend_decode / write_prefill / attend_prefill, once for all forms.  Pointers go to the library as plain ints
# (data_ptr()), which its c_void_p prototypes take.
WRITE_DECODE, ATTEND_DECODE, WRITE_PREFILL, ATTEND_PREFILL = range(4)


def _entry(suffix: str):
    return tuple((op + suffix, "gpbs_hip_" + op + suffix)
                 for op in ("qkv_rope_cache", "decode_attn", "qkv_rope_cache_prefill", "prefill_attn"))


def _need_vectors(what: str, B: int, vectors):
    """The per-sequence device vectors (pos_t, len_t): each a contiguous int32 [B].  Only the host side is checked:
    the kernels clamp the values themselves, and reading one would force a sync inside a captured graph."""
    for name, t in vectors:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.numel() != B:
            raise ValueError(f"{what}: {name} must be an int32 tensor of exactly B={B} elements, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous (strides {t.stride()})")


_BF16, _F32 = torch.bfloat16, torch.float32


def _need_layout(what: str, dtype, dtype_name: str, names, a, b):
    """Two tensors of one dtype, both contiguous."""
    if a.dtype is not dtype or b.dtype is not dtype or not (a.is_contiguous() and b.is_contiguous()):
        for name, t in zip(names, (a, b)):
            if t.dtype is not dtype:
                raise ValueError(f"{what}: {name} must be {dtype_name}, got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be contiguous (strides {t.stride()})")


def _need_dense(what: str, kc, vc):
    """The dense caches of DenseUniform / DenseSeq; returns (B, Hkv, C, hd)."""
    shape = kc.shape  # read once: every .shape builds a new torch.Size
    if len(shape) != 4 or vc.shape != shape:
        raise ValueError(f"{what}: caches {tuple(shape)} / {tuple(vc.shape)} must be [B, Hkv, C, hd] of one shape")
    B, Hkv, Cn, hd = shape
    if B < 1 or Hkv < 1 or Cn < 1 or hd < 8 or hd % 8:
        raise ValueError(f"{what}: caches {tuple(shape)} must be [B, Hkv, C, hd], none empty, hd % 8 == 0")
    _need_layout(what, _BF16, "bf16", ("kc", "vc"), kc, vc)
    return B, Hkv, Cn, hd


class DenseUniform:
    """Caches kc / vc bf16 [B, Hkv, C, hd], every sequence at the position `pos`: an int32 [1] device tensor for the
    decode launches (the kernel reads it at run time: valid inside a captured graph; the caller keeps 0 <= pos < C),
    a host int for the prefill ones, whose S tokens go to rows pos .. pos + S - 1."""
    entry, names = _entry(""), ("kc", "vc")
    partial = False  # attend_prefill stores every row of its result
    wrote = None

    def __init__(self, kc, vc, pos):
        self.cache, self.pos = (kc, vc), pos

    def check(self, what: str, S, attend: bool):
        B, Hkv, Cn, hd = _need_dense(what, *self.cache)
        pos = self.pos
        if S is None:
            if not isinstance(pos, torch.Tensor) or pos.dtype != torch.int32 or pos.numel() != 1:
                raise ValueError(f"{what}: pos_t must be a 1-element int32 tensor, got "
                                 f"{getattr(pos, 'dtype', type(pos))} {tuple(getattr(pos, 'shape', ()))}")
        elif not isinstance(pos, int) or isinstance(pos, bool) or pos < 0 or pos + S > Cn:
            raise ValueError(f"{what}: pos={pos!r} with S={S} must satisfy 0 <= pos and pos + S <= C={Cn}")
        return B, Hkv, hd, Cn

    def args(self, S):
        Cn = self.cache[0].shape[2]
        return (("pos_t",), (self.pos,), (Cn,), ()) if S is None else ((), (), (Cn,), (self.pos,))


class DenseSeq:
    """The same caches with one device position per sequence, pos_t int32 [B], and for prefill one length, len_t
    int32 [B], under the slot rules above."""
    entry, names = _entry("_seq"), ("kc", "vc")
    partial = True  # attend_prefill stores rows s < n_b only: its result starts as zeros
    wrote = None

    def __init__(self, kc, vc, pos_t, len_t=None):
        self.cache, self.pos_t, self.len_t = (kc, vc), pos_t, len_t

    def check(self, what: str, S, attend: bool):
        B, Hkv, Cn, hd = _need_dense(what, *self.cache)
        if S is None:
            _need_vectors(what, B, (("pos_t", self.pos_t),))
        else:
            if attend and S > Cn:  # the attention launch is sized for S
                raise ValueError(f"{what}: S={S} must satisfy pos + S <= C={Cn} at pos = 0")
            _need_vectors(what, B, (("pos_t", self.pos_t), ("len_t", self.len_t)))
        return B, Hkv, hd, Cn

    def args(self, S):
        Cn = self.cache[0].shape[2]
        if S is None:
            return ("pos_t",), (self.pos_t,), (Cn,), ()
        return ("pos_t", "len_t"), (self.pos_t, self.len_t), (Cn,), ()


class Paged:
    """Pools kpool / vpool bf16 [P, Hkv, page, 128] behind the block table `table` int32 [B, NP], with pos_t / len_t
    as DenseSeq and NP * page rows per sequence (the paged rules above)."""
    entry, names, dtype, dtype_name = _entry("_paged"), ("kpool", "vpool"), torch.bfloat16, "bf16"
    partial = True
    wrote = None

    def __init__(self, kpool, vpool, table, pos_t, len_t=None):
        self.cache, self.scales = (kpool, vpool), ()
        self.table, self.pos_t, self.len_t = table, pos_t, len_t

    def check(self, what: str, S, attend: bool):
        """One check for both pool dtypes: `scales` is empty here and (kscale, vscale) in PagedKv8."""
        kp, vp, table = self.cache[0], self.cache[1], self.table
        if not isinstance(kp, torch.Tensor) or not isinstance(vp, torch.Tensor) or kp.dim() != 4 \
                or vp.shape != kp.shape:
            raise ValueError(f"{what}: pools {tuple(getattr(kp, 'shape', ()))} / {tuple(getattr(vp, 'shape', ()))} "
                             f"must be [P, Hkv, page, 128] of one shape")
        P, Hkv, page, hd = kp.shape
        if page not in PAGE_SIZES or hd != 128 or P < 1 or Hkv < 1:
            raise ValueError(f"{what}: pools {tuple(kp.shape)} must be [P, Hkv, page, 128] with page in {PAGE_SIZES}")
        _need_layout(what, self.dtype, self.dtype_name, self.names, kp, vp)
        for name, t in zip(("kscale", "vscale"), self.scales):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (P, Hkv, page) \
                    or not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be a contiguous fp32 tensor [P, Hkv, page] = {(P, Hkv, page)}, "
                                 f"got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 2 \
                or table.shape[0] < 1 or table.shape[1] < 1:
            raise ValueError(f"{what}: table must be an int32 tensor [B >= 1, NP >= 1], got "
                             f"{getattr(table, 'dtype', type(table))} {tuple(getattr(table, 'shape', ()))}")
        if not table.is_contiguous():
            raise ValueError(f"{what}: table must be contiguous (strides {table.stride()})")
        B, NP = table.shape
        _need_vectors(what, B, (("pos_t", self.pos_t),) if S is None else
                      (("pos_t", self.pos_t), ("len_t", self.len_t)))
        return B, Hkv, hd, NP * page

    def args(self, S):
        P, _, page, _ = self.cache[0].shape
        geom = (self.table.shape[1], P, page)
        if S is None:
            return ("pos_t", "table"), (self.pos_t, self.table), geom, ()
        return ("pos_t", "len_t", "table"), (self.pos_t, self.len_t, self.table), geom, ()


class PagedKv8(Paged):
    """The fp8 paged cache: code pools kpool8 / vpool8 float8_e4m3fn [P, Hkv, page, 128] and the scales kscale /
    vscale fp32 [P, Hkv, page] of the codec above."""
    entry, names = _entry("_paged_kv8"), ("kpool8", "vpool8", "kscale", "vscale")
    dtype, dtype_name = torch.float8_e4m3fn, "float8_e4m3fn"

    def __init__(self, kpool8, vpool8, kscale, vscale, table, pos_t, len_t=None):
        self.cache, self.scales = (kpool8, vpool8, kscale, vscale), (kscale, vscale)
        self.table, self.pos_t, self.len_t = table, pos_t, len_t


class PagedEmulated(Paged):
    """The fp8 cache emulated on bf16 pools with the bf16 paged kernels: after the write launch, torch ops round
    exactly the rows it stored through the codec (kv8_emulate_rows), so the attention launch reads what PagedKv8
    would hold.  The oracle of PagedKv8; torch indexing between the launches, so not for a captured graph."""

    def wrote(self, S):
        kv8_emulate_rows(*self.cache, self.table, self.pos_t, None if S is None else self.len_t, S or 1)


_DATA_PTR, _IS_CUDA = torch.Tensor.data_ptr, operator.attrgetter("is_cuda")


def _need_cuda(what: str, tensors, *names):
    """Every tensor an entry point reads or writes is on the GPU: asked last, of the addressing tensors first.
    `names`: tuples of the tensors' names, put together only to name the first that is not."""
    if not all(map(_IS_CUDA, tensors)):
        name, t = next((name, t) for name, t in zip(sum(names, ()), tensors) if not t.is_cuda)
        raise ValueError(f"{what}: {name} must be a CUDA tensor (the kernel reads it), got {t.device}")


def _write(what: str, sym: str, view, qkv, cos, sin, S, rows, dims, hd):
    """The part of write_decode / write_prefill after the shape of qkv: dims = (B, [S,] H, Hkv)."""
    if qkv.dtype is not _BF16:
        raise ValueError(f"{what}: qkv must be bf16, got {qkv.dtype}")
    if not qkv.is_contiguous():
        raise ValueError(f"{what}: qkv must be contiguous (strides {qkv.stride()})")
    tables = cos.shape
    if len(tables) != 2 or tables[1] * 2 != hd or sin.shape != tables:
        raise ValueError(f"{what}: rope tables {tuple(tables)} / {tuple(sin.shape)} must be [rows, hd / 2] of one "
                         f"shape for hd={hd}")
    if cos.dtype is not _F32 or sin.dtype is not _F32 or not (cos.is_contiguous() and sin.is_contiguous()):
        raise ValueError(f"{what}: rope tables {tuple(tables)} {cos.dtype} / {sin.dtype} must be contiguous fp32")
    names, index, geom, tail = view.args(S)
    need = tail[0] + S if tail else rows  # a host position: rows pos .. pos + S - 1; else any row can be a position
    if tables[0] < need:
        raise ValueError(f"{what}: rope tables {tuple(tables)} must cover {need} rows")
    _need_cuda(what, (*index, qkv, cos, sin, *view.cache), names, ("qkv", "cos", "sin"), view.names)
    q = torch.empty(*dims[:-1], hd, dtype=torch.bfloat16, device=qkv.device)
    _check(getattr(lib(), sym)(*map(_DATA_PTR, (qkv, cos, sin, *index, q, *view.cache)), *dims, *geom, hd, *tail,
                               _stream()), what)
    if view.wrote is not None:
        view.wrote(S)
    return q


def write_decode(view, qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, n_heads: int) -> torch.Tensor:
    """One new token per sequence: split the packed qkv [B, 1, (H + 2 Hkv) hd], RoPE q and k at the sequence's
    position (angle rows of the fp32 tables cos / sin [>= rows, hd / 2]), store k / v at that cache row; returns q
    [B, H, hd].  An idle sequence of a per-sequence form stores nothing and gets a zero q row."""
    what, sym = view.entry[WRITE_DECODE]
    B, Hkv, hd, rows = view.check(what, None, False)
    if qkv.numel() != B * (n_heads + 2 * Hkv) * hd:
        raise ValueError(f"{what}: qkv {tuple(qkv.shape)} vs cache {tuple(view.cache[0].shape)}, B={B}, H={n_heads}")
    return _write(what, sym, view, qkv, cos, sin, None, rows, (B, n_heads, Hkv), hd)


def write_prefill(view, qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, n_heads: int) -> torch.Tensor:
    """S new tokens per sequence: qkv [B, S, (H + 2 Hkv) hd]; token s is rotated at angle row pos + s and stored at
    that cache row; returns q [B, S, H, hd].  A padding token (s >= n_b) stores nothing and gets a zero q row."""
    what, sym = view.entry[WRITE_PREFILL]
    if qkv.dim() != 3 or qkv.shape[1] < 1:
        raise ValueError(f"{what}: qkv {tuple(qkv.shape)} must be [B, S >= 1, (H + 2 Hkv) hd]")
    S = qkv.shape[1]
    B, Hkv, hd, rows = view.check(what, S, False)
    if qkv.shape[0] != B or qkv.shape[2] != (n_heads + 2 * Hkv) * hd:
        raise ValueError(f"{what}: qkv {tuple(qkv.shape)} must be [B={B}, S, (H + 2 Hkv) hd] for cache "
                         f"{tuple(view.cache[0].shape)}, H={n_heads}")
    return _write(what, sym, view, qkv, cos, sin, S, rows, (B, S, n_heads, Hkv), hd)


def _need_q(what: str, q, qs, ok: bool, lay: str, B: int, Hkv: int, hd: int) -> int:
    """q of an attention launch, `lay` = [B, (S,) H, 128] bf16 contiguous (qs: its shape, `ok`: it fits); returns H."""
    if hd != 128:
        raise ValueError(f"{what}: head_dim 128 required, the cache has {hd}")
    if not ok:
        raise ValueError(f"{what}: q {tuple(qs)} must be {lay} with B = {B}")
    H = qs[-2]
    if H % Hkv or (H // Hkv) not in (1, 2, 4, 8):
        raise ValueError(f"{what}: group size H / Hkv = {H} / {Hkv} must be 1, 2, 4 or 8")
    if q.dtype is not _BF16:
        raise ValueError(f"{what}: q must be bf16, got {q.dtype}")
    if not q.is_contiguous():
        raise ValueError(f"{what}: q must be contiguous (strides {q.stride()})")
    return H


def attend_decode(view, q: torch.Tensor, nsplit: Optional[int] = None) -> torch.Tensor:
    """Grouped-query attention of one new token per sequence over cache rows 0 .. pos: q [B, H, 128] -> [B, H * 128].
    The keys are split over `nsplit` workgroups per (batch, KV head) (flash-decoding; default: from the shapes alone,
    enough to give the chip >= 256 workgroups, so a row's split does not depend on its position) and merged by a
    combine kernel.  The row of an idle sequence is zero."""
    what, sym = view.entry[ATTEND_DECODE]
    B, Hkv, hd, rows = view.check(what, None, True)
    qs = q.shape
    H = _need_q(what, q, qs, len(qs) == 3 and qs[0] == B and qs[2] == hd, "[B, H, 128]", B, Hkv, hd)
    if nsplit is None:
        nsplit = max(1, min(8, -(-256 // (B * Hkv)), -(-rows // 64)))
    elif not isinstance(nsplit, int) or isinstance(nsplit, bool) or nsplit < 1:
        raise ValueError(f"{what}: nsplit={nsplit!r} must be None or an int >= 1")
    names, index, geom, _ = view.args(None)
    _need_cuda(what, (*index, q, *view.cache), names, ("q",), view.names)
    out = torch.empty(B, H * hd, dtype=torch.bfloat16, device=q.device)
    ws = torch.empty(B * Hkv * nsplit * (H // Hkv) * (hd + 2), dtype=torch.float32, device=q.device) \
        if nsplit > 1 else None
    _check(getattr(lib(), sym)(*map(_DATA_PTR, (q, *view.cache, *index, out)), None if ws is None else ws.data_ptr(),
                               nsplit, B, H, Hkv, *geom, hd, C.c_float(hd ** -0.5), _stream()), what)
    return out


def attend_prefill(view, q: torch.Tensor) -> torch.Tensor:
    """Causal grouped-query attention of S new tokens per sequence over the cache, which already holds their rows
    (bf16 MFMA): q [B, S, H, 128] (RoPE applied); query s attends rows 0 .. pos + s.  Returns [B, S, H * 128] bf16,
    rows s >= n_b zero.  No row past the last new one is read."""
    what, sym = view.entry[ATTEND_PREFILL]
    qs = q.shape
    if len(qs) != 4 or qs[1] < 1:
        raise ValueError(f"{what}: q {tuple(qs)} must be [B, S >= 1, H, 128]")
    S = qs[1]
    B, Hkv, hd, _ = view.check(what, S, True)
    H = _need_q(what, q, qs, qs[0] == B and qs[3] == hd, "[B, S, H, 128]", B, Hkv, hd)
    names, index, geom, tail = view.args(S)
    _need_cuda(what, (*index, q, *view.cache), names, ("q",), view.names)
    out = (torch.zeros if view.partial else torch.empty)(B, S, H * hd, dtype=torch.bfloat16, device=q.device)
    _check(getattr(lib(), sym)(*map(_DATA_PTR, (q, *view.cache, *index, out)), B, S, H, Hkv, *geom, hd, *tail,
                               C.c_float(hd ** -0.5), _stream()), what)
    return out


# The sixteen entry points by name: each builds the view of its form and calls the function of its operation.
def qkv_rope_cache(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos_t: torch.Tensor, kc: torch.Tensor,
                   vc: torch.Tensor, n_heads: int) -> torch.Tensor:
    """One-token decode: split the packed qkv [B, 1, (H + 2 Hkv) hd], RoPE q and k
    at the device position pos_t (int32 [1]), write k / v into the caches
    [B, Hkv, C, hd] at that row, return q [B, H, hd].  No bounds check on the
    device value: the caller keeps 0 <= pos < C."""
    return write_decode(DenseUniform(kc, vc, pos_t), qkv, cos, sin, n_heads)


def decode_attn(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, pos_t: torch.Tensor,
                nsplit: Optional[int] = None) -> torch.Tensor:
    """Grouped-query attention of one new token per sequence over cache rows
    0..pos (pos_t int32 [1] on device): q [B, H, 128] -> [B, H * 128].  The keys
    are split over `nsplit` workgroups per (batch, KV head) (flash-decoding,
    default: enough to give the chip >= 256 workgroups) and merged by a combine
    kernel.  Everything the kernel takes as a raw pointer is checked on the host
    tensors before the library is touched, except the device value of pos_t:
    reading it would force a sync inside a captured graph, so the caller keeps
    0 <= pos (the kernel clamps pos + 1 to C)."""
    return attend_decode(DenseUniform(kc, vc, pos_t), q, nsplit)


def qkv_rope_cache_prefill(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: int, kc: torch.Tensor,
                           vc: torch.Tensor, n_heads: int) -> torch.Tensor:
    """S-token form of qkv_rope_cache with a host position: split the packed qkv
    [B, S, (H + 2 Hkv) hd], RoPE q and k at angle rows pos + s, write k / v into
    rows pos .. pos + S - 1 of the caches [B, Hkv, C, hd]; returns q [B, S, H, hd]."""
    return write_prefill(DenseUniform(kc, vc, pos), qkv, cos, sin, n_heads)


def prefill_attn(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, pos: int) -> torch.Tensor:
    """Causal grouped-query attention of S new tokens over the static KV cache
    (k_prefill_attn, bf16 MFMA): q [B, S, H, 128] (RoPE applied), caches
    [B, Hkv, C, 128] already holding rows pos .. pos + S - 1; query s attends
    cache rows 0 .. pos + s.  Returns [B, S, H * 128] bf16.  Rows >= pos + S of
    the caches are never read."""
    return attend_prefill(DenseUniform(kc, vc, pos), q)


def qkv_rope_cache_seq(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos_t: torch.Tensor,
                       kc: torch.Tensor, vc: torch.Tensor, n_heads: int) -> torch.Tensor:
    """qkv_rope_cache with one device position per sequence (pos_t int32 [B]):
    an active sequence gets the arithmetic of qkv_rope_cache at pos_t[b]; an
    idle one writes nothing to its caches and its q row is zero."""
    return write_decode(DenseSeq(kc, vc, pos_t), qkv, cos, sin, n_heads)


def decode_attn_seq(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, pos_t: torch.Tensor,
                    nsplit: Optional[int] = None) -> torch.Tensor:
    """decode_attn with one device position per sequence (pos_t int32 [B]):
    row b is bit-identical to decode_attn at pos = pos_t[b] with the same
    nsplit; an idle sequence loads no cache row and its row is zero."""
    return attend_decode(DenseSeq(kc, vc, pos_t), q, nsplit)


def qkv_rope_cache_prefill_seq(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos_t: torch.Tensor,
                               len_t: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor,
                               n_heads: int) -> torch.Tensor:
    """qkv_rope_cache_prefill with a device position and length per sequence
    (int32 [B] each): token s < n_b of sequence b is rotated at angle row
    pos_t[b] + s and written to that cache row; tokens s >= n_b write nothing
    and their q rows are zero.  Returns q [B, S, H, hd]."""
    return write_prefill(DenseSeq(kc, vc, pos_t, len_t), qkv, cos, sin, n_heads)


def prefill_attn_seq(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, pos_t: torch.Tensor,
                     len_t: torch.Tensor) -> torch.Tensor:
    """prefill_attn with a device position and length per sequence (int32 [B]
    each): q [B, S, H, 128] padded to the longest sequence; query s < n_b of
    sequence b attends cache rows 0 .. pos_t[b] + s and its row is bit-identical
    to prefill_attn on that sequence alone with (S = n_b, pos = pos_t[b]).  Rows
    s >= n_b of the result are zero, their q rows are never loaded, and no cache
    row past pos_t[b] + n_b - 1 is addressed.  Returns [B, S, H * 128] bf16."""
    return attend_prefill(DenseSeq(kc, vc, pos_t, len_t), q)


def qkv_rope_cache_paged(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos_t: torch.Tensor,
                         table: torch.Tensor, kpool: torch.Tensor, vpool: torch.Tensor, n_heads: int) -> torch.Tensor:
    """qkv_rope_cache_seq through a block table: an active sequence
    (0 <= pos_t[b] < NP * page) gets the same q and writes the same k / v row,
    into row pos_t[b] % page of page table[b, pos_t[b] // page]."""
    return write_decode(Paged(kpool, vpool, table, pos_t), qkv, cos, sin, n_heads)


def decode_attn_paged(q: torch.Tensor, kpool: torch.Tensor, vpool: torch.Tensor, table: torch.Tensor,
                      pos_t: torch.Tensor, nsplit: Optional[int] = None) -> torch.Tensor:
    """decode_attn_seq through a block table: row b is bit-identical to
    decode_attn_seq on the dense cache of Cl = NP * page rows gathered from
    sequence b's pages, with the same nsplit (default: from (B, Hkv, Cl))."""
    return attend_decode(Paged(kpool, vpool, table, pos_t), q, nsplit)


def qkv_rope_cache_prefill_paged(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos_t: torch.Tensor,
                                 len_t: torch.Tensor, table: torch.Tensor, kpool: torch.Tensor, vpool: torch.Tensor,
                                 n_heads: int) -> torch.Tensor:
    """qkv_rope_cache_prefill_seq through a block table: token s < n_b of
    sequence b (n_b from Cl = NP * page) is written to logical row pos_t[b] + s
    of its pages.  Returns q [B, S, H, hd]."""
    return write_prefill(Paged(kpool, vpool, table, pos_t, len_t), qkv, cos, sin, n_heads)


def prefill_attn_paged(q: torch.Tensor, kpool: torch.Tensor, vpool: torch.Tensor, table: torch.Tensor,
                       pos_t: torch.Tensor, len_t: torch.Tensor) -> torch.Tensor:
    """prefill_attn_seq through a block table: rows s < n_b of sequence b are
    bit-identical to prefill_attn_seq on the dense cache gathered from its
    pages; no row past pos_t[b] + n_b - 1 is addressed, through any page.
    Returns [B, S, H * 128] bf16, rows s >= n_b zero."""
    return attend_prefill(Paged(kpool, vpool, table, pos_t, len_t), q)


def qkv_rope_cache_paged_kv8(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos_t: torch.Tensor,
                             table: torch.Tensor, kpool8: torch.Tensor, vpool8: torch.Tensor, kscale: torch.Tensor,
                             vscale: torch.Tensor, n_heads: int) -> torch.Tensor:
    """qkv_rope_cache_paged over an fp8 cache: the same q; the k / v row the bf16
    kernel would have stored goes through kv8_quant_ref into the code pools and
    the scales, at the same page and page row."""
    return write_decode(PagedKv8(kpool8, vpool8, kscale, vscale, table, pos_t), qkv, cos, sin, n_heads)


def decode_attn_paged_kv8(q: torch.Tensor, kpool8: torch.Tensor, vpool8: torch.Tensor, kscale: torch.Tensor,
                          vscale: torch.Tensor, table: torch.Tensor, pos_t: torch.Tensor,
                          nsplit: Optional[int] = None) -> torch.Tensor:
    """decode_attn_paged over an fp8 cache: bit-identical to decode_attn_paged on
    the bf16 pools kv8_dequant(kpool8, kscale) / kv8_dequant(vpool8, vscale) with
    the same nsplit (default: from (B, Hkv, Cl))."""
    return attend_decode(PagedKv8(kpool8, vpool8, kscale, vscale, table, pos_t), q, nsplit)


def qkv_rope_cache_prefill_paged_kv8(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos_t: torch.Tensor,
                                     len_t: torch.Tensor, table: torch.Tensor, kpool8: torch.Tensor,
                                     vpool8: torch.Tensor, kscale: torch.Tensor, vscale: torch.Tensor,
                                     n_heads: int) -> torch.Tensor:
    """qkv_rope_cache_prefill_paged over an fp8 cache: the same q; every k / v row
    the bf16 kernel would have stored goes through kv8_quant_ref into the code
    pools and the scales.  Returns q [B, S, H, hd]."""
    return write_prefill(PagedKv8(kpool8, vpool8, kscale, vscale, table, pos_t, len_t), qkv, cos, sin, n_heads)


def prefill_attn_paged_kv8(q: torch.Tensor, kpool8: torch.Tensor, vpool8: torch.Tensor, kscale: torch.Tensor,
                           vscale: torch.Tensor, table: torch.Tensor, pos_t: torch.Tensor,
                           len_t: torch.Tensor) -> torch.Tensor:
    """prefill_attn_paged over an fp8 cache: bit-identical to prefill_attn_paged
    on the bf16 pools kv8_dequant(kpool8, kscale) / kv8_dequant(vpool8, vscale).
    Returns [B, S, H * 128] bf16, rows s >= n_b zero."""
    return attend_prefill(PagedKv8(kpool8, vpool8, kscale, vscale, table, pos_t, len_t), q)


# --------------------------------------------------------------------------- fp8 (config #5, CDNA4 fp8 MFMA)
FP8_MAX = 448.0  # OCP e4m3fn (gfx950), not the MI300 fnuz variant
FP8_M_TILE = 64  # rows per gpbs_hip_fp8_linear launch


def quant_rows_fp8(x: torch.Tensor):
    """Per-row symmetric e4m3fn quantisation on device: returns (q [rows, K]
    float8_e4m3fn, scale [rows] fp32) with scale = absmax / 448."""
    x = x.contiguous()
    _need(x, "quant_rows_fp8 x")
    K = x.shape[-1]
    if K % 8:
        raise ValueError(f"quant_rows_fp8: K={K} must be a multiple of 8")
    rows = x.numel() // K
    q = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
    s = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    _check(lib().gpbs_hip_quant_rows_fp8(_ptr(x), _ptr(q), _ptr(s), rows, K, _stream()), "quant_rows_fp8")
    return q, s


def quant_rows_fp8_ref(x: torch.Tensor):
    """fp32 PyTorch reference of quant_rows_fp8 (runs on CPU too).  It mirrors the
    kernel's arithmetic (x * (448 / amax) in fp32, clamp, round to nearest even),
    so on finite input the codes and scales agree bit for bit.  Inputs must be
    finite; behaviour differs otherwise (a NaN becomes a NaN code here and -448
    in the kernel's clamp)."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    # Both quotients as tensor / tensor: one correctly rounded division each, as in
    # the kernel.  torch evaluates `scalar / tensor` as reciprocal(tensor) * scalar
    # (two roundings, which moves values onto and off e4m3 ties) and, on the GPU,
    # `tensor / scalar` as tensor * (1 / scalar).
    top = torch.full_like(amax, FP8_MAX)
    s = torch.where(amax > 0, amax / top, torch.ones_like(amax))
    inv = torch.where(amax > 0, top / amax, torch.ones_like(amax))  # multiply, as the kernel does
    q = (xf * inv.unsqueeze(-1)).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return q, s


class Fp8Weight:
    """A linear weight [N, K] stored as e4m3fn rows plus per-output-channel scales."""

    def __init__(self, w: torch.Tensor):
        w = w.detach().to(torch.bfloat16).contiguous()
        self.N, self.K = w.shape
        if self.N % 16 or self.K % 256:
            raise ValueError(f"Fp8Weight: [N={self.N}, K={self.K}] needs N % 16 == 0 and K % 256 == 0")
        q, self.s = quant_rows_fp8(w) if w.is_cuda else quant_rows_fp8_ref(w)
        self.qs = self.shuffle(q)  # the only stored copy: the kernel's lane-order layout

    @classmethod
    def from_quantised(cls, q: torch.Tensor, s: torch.Tensor) -> "Fp8Weight":
        """The weight of given row-major e4m3fn codes q [N, K] and fp32 row scales
        s [N] (no quantiser involved): only the shuffled copy is built."""
        if q.dtype != torch.float8_e4m3fn or q.dim() != 2:
            raise ValueError(f"Fp8Weight.from_quantised: q must be e4m3fn [N, K], got {q.dtype} {tuple(q.shape)}")
        self = cls.__new__(cls)
        self.N, self.K = q.shape
        if self.N % 16 or self.K % 256:
            raise ValueError(f"Fp8Weight: [N={self.N}, K={self.K}] needs N % 16 == 0 and K % 256 == 0")
        if s.dtype != torch.float32 or s.numel() != self.N or s.device != q.device:
            raise ValueError(f"Fp8Weight.from_quantised: s must be fp32 with {self.N} elements on {q.device}, got "
                             f"{s.dtype} {tuple(s.shape)} on {s.device}")
        self.s = s.reshape(self.N).contiguous()
        self.qs = self.shuffle(q.contiguous())
        return self

    # Kernel layout: [N/16 strips][K/256 blocks][4 steps u][4 lane groups g][16 rows r][16 B];
    # lane l = 16 g + r of the wave that owns (strip, block) reads the 16 bytes
    # W[16 strip + r][256 block + 64 u + 16 g : +16] at step u, so each load
    # instruction is one contiguous 1 KiB run.
    def shuffle(self, q: torch.Tensor) -> torch.Tensor:
        b = q.view(torch.uint8).view(self.N // 16, 16, self.K // 256, 4, 4, 16)
        return b.permute(0, 2, 3, 4, 1, 5).contiguous().view(torch.float8_e4m3fn).view(self.N, self.K)

    @property
    def q(self) -> torch.Tensor:
        """Row-major [N, K] e4m3fn view (a copy; for references and tests)."""
        b = self.qs.view(torch.uint8).view(self.N // 16, self.K // 256, 4, 4, 16, 16)
        return b.permute(0, 4, 1, 2, 3, 5).contiguous().view(torch.float8_e4m3fn).view(self.N, self.K)

    def nbytes(self) -> int:
        return self.qs.numel() + 4 * self.s.numel()


def fp8_shuffled_offset(n: int, k: int, K: int) -> int:
    """Byte offset in ``Fp8Weight.qs`` of the 16 bytes W[n][k : k + 16]
    (k % 16 == 0); the Python twin of the staging address of
    k_gemm_fp8_tn<1> (csrc/hip/fp8_gemm_kernels.hip)."""
    if k % 16 or K % 256 or not 0 <= k < K:
        raise ValueError(f"fp8_shuffled_offset: k={k} (k % 16 == 0, 0 <= k < K), K={K} (K % 256 == 0)")
    return ((n // 16) * (K // 256) + k // 256) * 4096 + ((k % 256) // 64) * 1024 + ((k % 64) // 16) * 256 \
        + (n % 16) * 16


def fp8_linear_q(xq: torch.Tensor, sx: torch.Tensor, w: Fp8Weight, resid: Optional[torch.Tensor] = None,
                 tiled: bool = False) -> torch.Tensor:
    """y = (xq @ Wq^T) * sx[m] * sw[n] (+ resid, fused into the epilogue) on
    already-quantised rows (the output of quant_rows_fp8 / rmsnorm_quant_fp8 /
    swiglu_quant_fp8); bf16 out.  ``tiled`` (opt-in, no resid, N % 128 == 0):
    one launch of the LDS-tiled fp8 GEMM over the shuffled weight for any M,
    instead of one weight-streaming launch per 64 rows.  The library takes raw
    pointers, so everything it reads is checked here first."""
    lead = xq.shape[:-1]
    if xq.dtype != torch.float8_e4m3fn or xq.shape[-1] != w.K or not xq.is_contiguous():
        raise ValueError(f"fp8_linear_q: need contiguous e4m3fn [..., {w.K}], got {xq.dtype} {tuple(xq.shape)}")
    M = xq.numel() // w.K
    if M == 0:
        raise ValueError(f"fp8_linear_q: xq {tuple(xq.shape)} has no rows")
    if sx.dtype != torch.float32 or not sx.is_contiguous() or sx.numel() != M:
        raise ValueError(f"fp8_linear_q: sx must be contiguous fp32 with {M} elements, got {sx.dtype} "
                         f"{tuple(sx.shape)} contiguous={sx.is_contiguous()}")
    if resid is not None and (resid.dtype != torch.bfloat16 or not resid.is_contiguous()
                              or resid.numel() != M * w.N):
        raise ValueError(f"fp8_linear_q: resid must be contiguous bf16 with {M} x {w.N} elements, got {resid.dtype} "
                         f"{tuple(resid.shape)} contiguous={resid.is_contiguous()}")
    for name, t in (("xq", xq), ("sx", sx), ("weight", w.qs), ("weight scale", w.s), ("resid", resid)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"fp8_linear_q: {name} must be a CUDA tensor, got {t.device}")
        if t is not None and t.device != xq.device:
            raise ValueError(f"fp8_linear_q: {name} is on {t.device}, xq on {xq.device}")
    y = torch.empty(*lead, w.N, dtype=torch.bfloat16, device=xq.device)
    if tiled and resid is None and w.N % 128 == 0:
        gemm_fp8(xq.view(M, w.K), sx.reshape(M), w.qs, w.s, y.view(M, w.N), b_shuffled=True)
        return y
    L, st = lib(), _stream()
    if resid is not None:
        _need(resid, "fp8_linear_q resid")
        if resid.numel() != M * w.N or M > FP8_M_TILE:
            raise ValueError(f"fp8_linear_q: resid {tuple(resid.shape)} for [{M}, {w.N}] (M <= {FP8_M_TILE})")
        _check(L.gpbs_hip_fp8_linear_res(_ptr(xq), _ptr(sx), _ptr(w.qs), _ptr(w.s), _ptr(y), _ptr(resid), M, w.N,
                                         w.K, st), "fp8_linear_res")
        return y
    if M <= FP8_M_TILE:
        _check(L.gpbs_hip_fp8_linear(_ptr(xq), _ptr(sx), _ptr(w.qs), _ptr(w.s), _ptr(y), M, w.N, w.K, st),
               "fp8_linear")
        return y
    x2, s2, y2 = xq.view(M, w.K), sx.reshape(M), y.view(M, w.N)
    for m0 in range(0, M, FP8_M_TILE):
        m1 = min(M, m0 + FP8_M_TILE)
        _check(L.gpbs_hip_fp8_linear(_ptr(x2[m0:m1]), _ptr(s2[m0:m1]), _ptr(w.qs), _ptr(w.s), _ptr(y2[m0:m1]),
                                     m1 - m0, w.N, w.K, st), "fp8_linear")
    return y


def fp8_linear(x: torch.Tensor, w: Fp8Weight, tiled: bool = False) -> torch.Tensor:
    """y = x @ W^T with W in fp8 and x quantised per token to fp8 on the fly;
    fp32 MFMA accumulation, bf16 output.  x [..., K] bf16.  ``tiled``: as
    fp8_linear_q."""
    xq, sx = quant_rows_fp8(x)
    return fp8_linear_q(xq, sx, w, tiled=tiled)


def rmsnorm_quant_fp8(x: torch.Tensor, w: torch.Tensor, eps: float):
    """e4m3 rows of rmsnorm(x) * w plus their scales, in one kernel."""
    x = x.contiguous()
    _need(x, "rmsnorm_quant_fp8 x")
    dim = x.shape[-1]
    w = w.to(torch.bfloat16).contiguous()
    if w.numel() != dim or dim % 8:
        raise ValueError(f"rmsnorm_quant_fp8: weight {tuple(w.shape)} vs dim {dim}")
    q = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
    s = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    _check(lib().gpbs_hip_rmsnorm_quant_fp8(_ptr(x), _ptr(w), _ptr(q), _ptr(s), x.numel() // dim, dim,
                                            C.c_float(eps), _stream()), "rmsnorm_quant_fp8")
    return q, s


def swiglu_quant_fp8(gu: torch.Tensor):
    """e4m3 rows of silu(gu[..., :F]) * gu[..., F:] plus their scales (gu is the
    packed gate|up linear output, read in place)."""
    gu = gu.contiguous()
    _need(gu, "swiglu_quant_fp8 gu")
    F2 = gu.shape[-1]
    if F2 % 16:
        raise ValueError(f"swiglu_quant_fp8: packed width {F2} must be a multiple of 16")
    q = torch.empty(*gu.shape[:-1], F2 // 2, dtype=torch.float8_e4m3fn, device=gu.device)
    s = torch.empty(gu.shape[:-1], dtype=torch.float32, device=gu.device)
    _check(lib().gpbs_hip_swiglu_quant_fp8(_ptr(gu), _ptr(q), _ptr(s), gu.numel() // F2, F2 // 2, _stream()),
           "swiglu_quant_fp8")
    return q, s


def fp8_linear_ref(x: torch.Tensor, w: Fp8Weight) -> torch.Tensor:
    """fp32 reference of fp8_linear on the same quantised operands."""
    xq, sx = quant_rows_fp8_ref(x.reshape(-1, w.K))
    acc = xq.float() @ w.q.float().t()
    return (acc * sx.unsqueeze(1) * w.s.float().unsqueeze(0)).view(*x.shape[:-1], w.N)


# --------------------------------------------------------------------------- MXFP4 weights (csrc/hip/fp4_kernels.hip)
# OCP MXFP4: e2m1 codes (1 sign, 2 exponent, 1 mantissa bit; magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6), two per byte
# with the even k in the low nibble, and one E8M0 scale byte per 32 consecutive k of a row, value 2^(byte - 127);
# no per-row scale.  4.25 bits per weight.
MXFP4_BLOCK = 32
MXFP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # by the low three bits of a code; bit 3 is the sign


def mxfp4_quant_ref(w: torch.Tensor):
    """The MXFP4 quantiser of the OCP MX specification, plain torch on any device:
    w [N, K] (K % 32 == 0) of finite bf16 values -> (codes uint8 [N, K / 2], scales
    uint8 [N, K / 32]).  Per block of 32: amax = max |v|, E = floor(log2 amax) - 2
    clamped to [-127, 127] (0 for an all-zero block), byte = E + 127, and every
    element is v 2^-E (exact in fp32) rounded to the nearest e2m1 value, ties to
    the even code, saturating at +-6.  The exponent comes from the bits of amax
    and the rounding is seven comparisons with exact constants, so CPU and GPU
    give the same bits.  inf, NaN and bf16 subnormals are outside the contract.
    Requantising dequant() gives the same codes and scales back (a block's
    largest code is a 4 or a 6, which names the same E), except where
    0.5 * 2^E is no bf16 normal."""
    N, K = w.shape
    if K % MXFP4_BLOCK:
        raise ValueError(f"mxfp4_quant_ref: K={K} must be a multiple of {MXFP4_BLOCK}")
    v = w.detach().to(torch.bfloat16).float().reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = v.abs().amax(-1)
    e = ((amax.view(torch.int32) >> 23) - 127 - 2).clamp(-127, 127)  # the biased exponent field is floor(log2 amax) + 127
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    inv = ((127 - e) << 23).to(torch.int32).view(torch.float32)  # 2^-E, E in [-127, 125] for bf16 input
    t = v * inv.unsqueeze(-1)
    a = t.abs()
    # the midpoints of adjacent magnitudes; the tie goes to the even code: up at 0.75, 1.75, 3.5, down at the others
    mag = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) + (a >= 3.5) + (a > 5.0))
    code = (mag | ((v.view(torch.int32) >> 28) & 8).to(torch.uint8)).reshape(N, K // 2, 2)
    return (code[..., 0] | (code[..., 1] << 4)).contiguous(), (e + 127).to(torch.uint8)


def _e8m0_value(b: torch.Tensor) -> torch.Tensor:
    """2^(byte - 127) as fp32 (byte 0 is the fp32 subnormal 2^-127)."""
    i = b.to(torch.int32)
    return torch.where(i > 0, i << 23, torch.full_like(i, 0x00400000)).view(torch.float32)


class Mxfp4Weight:
    """A linear weight [N, K] stored as OCP MXFP4: e2m1 codes and one E8M0 scale
    byte per 32 k of a row, both in the lane order of k_mxfp4_gemm_skinny."""

    def __init__(self, w: torch.Tensor):
        w = w.detach().to(torch.bfloat16).contiguous()
        if w.dim() != 2 or w.shape[0] % 16 or w.shape[1] % 256:
            raise ValueError(f"Mxfp4Weight: {tuple(w.shape)} needs [N, K] with N % 16 == 0 and K % 256 == 0")
        self._store(*mxfp4_quant_ref(w))

    @classmethod
    def from_quantised(cls, codes: torch.Tensor, scales: torch.Tensor) -> "Mxfp4Weight":
        """The weight of given row-major data (no quantiser involved): codes uint8
        [N, K / 2], the even k in the low nibble, and scales uint8 [N, K / 32],
        none of them 0xFF (the NaN of E8M0)."""
        if codes.dtype != torch.uint8 or codes.dim() != 2:
            raise ValueError(f"Mxfp4Weight.from_quantised: codes must be uint8 [N, K / 2], got {codes.dtype} "
                             f"{tuple(codes.shape)}")
        N, K = codes.shape[0], 2 * codes.shape[1]
        if N % 16 or K % 256 or N == 0 or K == 0:
            raise ValueError(f"Mxfp4Weight: [N={N}, K={K}] needs N % 16 == 0 and K % 256 == 0")
        if scales.dtype != torch.uint8 or tuple(scales.shape) != (N, K // MXFP4_BLOCK) or scales.device != codes.device:
            raise ValueError(f"Mxfp4Weight.from_quantised: scales must be uint8 [{N}, {K // MXFP4_BLOCK}] on "
                             f"{codes.device}, got {scales.dtype} {tuple(scales.shape)} on {scales.device}")
        if bool((scales == 0xFF).any()):
            raise ValueError("Mxfp4Weight.from_quantised: a scale byte is 0xFF (NaN in E8M0)")
        self = cls.__new__(cls)
        self._store(codes.contiguous(), scales.contiguous())
        return self

    def _store(self, codes: torch.Tensor, scales: torch.Tensor):
        self.N, self.K = codes.shape[0], 2 * codes.shape[1]
        self.qs = self.shuffle(codes)  # the only stored copies: the kernel's lane-order layouts
        self.ss = self.shuffle_scales(scales)

    # Kernel layout of the codes: [N/16 strips][K/256 blocks][2 steps u][4 lane groups g][16 rows r][16 B];
    # lane l = 16 g + r of the wave that owns (strip, block) reads the 16 bytes (32 codes, one MX block)
    # W[16 strip + r][256 block + 128 u + 32 g : +32] at step u, so each load instruction is one
    # contiguous 1 KiB run.
    def shuffle(self, codes: torch.Tensor) -> torch.Tensor:
        b = codes.view(self.N // 16, 16, self.K // 256, 2, 4, 16)
        return b.permute(0, 2, 3, 4, 1, 5).contiguous().view(self.N, self.K // 2)

    # Kernel layout of the scales: [N/16 strips][K/256 blocks][4 lane groups g][16 rows r][2 steps u]; lane
    # l = 16 g + r reads one 2-byte word per block, byte u the scale of its codes at step u (MX block
    # 8 block + 4 u + g of row 16 strip + r), so each load instruction is one contiguous 128-byte run.
    def shuffle_scales(self, scales: torch.Tensor) -> torch.Tensor:
        b = scales.view(self.N // 16, 16, self.K // 256, 2, 4)
        return b.permute(0, 2, 4, 1, 3).contiguous().view(self.N, self.K // MXFP4_BLOCK)

    @property
    def codes(self) -> torch.Tensor:
        """Row-major [N, K / 2] uint8 (a copy; for references and tests)."""
        b = self.qs.view(self.N // 16, self.K // 256, 2, 4, 16, 16)
        return b.permute(0, 4, 1, 2, 3, 5).contiguous().view(self.N, self.K // 2)

    @property
    def scales(self) -> torch.Tensor:
        """Row-major [N, K / 32] uint8 (a copy)."""
        b = self.ss.view(self.N // 16, self.K // 256, 4, 16, 2)
        return b.permute(0, 3, 1, 4, 2).contiguous().view(self.N, self.K // MXFP4_BLOCK)

    def dequant(self) -> torch.Tensor:
        """fp32 [N, K] of value(code) * 2^(byte - 127): exact (one significant bit
        pair times a power of two) wherever that is a finite fp32."""
        c = self.codes
        nib = torch.stack([c & 0xF, c >> 4], -1).view(self.N, self.K).long()
        lut = torch.tensor(MXFP4_VALUES + tuple(-x for x in MXFP4_VALUES), dtype=torch.float32, device=c.device)
        return (lut[nib].view(self.N, -1, MXFP4_BLOCK) * _e8m0_value(self.scales).unsqueeze(-1)).view(self.N, self.K)

    def nbytes(self) -> int:
        return self.qs.numel() + self.ss.numel()


def mxfp4_shuffled_offset(n: int, k: int, K: int) -> int:
    """Byte offset in ``Mxfp4Weight.qs`` of the 16 bytes holding the codes
    W[n][k : k + 32] (k % 32 == 0); the Python twin of the weight address of
    k_mxfp4_gemm_skinny (csrc/hip/fp4_kernels.hip)."""
    if k % 32 or K % 256 or not 0 <= k < K:
        raise ValueError(f"mxfp4_shuffled_offset: k={k} (k % 32 == 0, 0 <= k < K), K={K} (K % 256 == 0)")
    return ((n // 16) * (K // 256) + k // 256) * 2048 + ((k % 256) // 128) * 1024 + ((k % 128) // 32) * 256 \
        + (n % 16) * 16


def mxfp4_scale_offset(n: int, k: int, K: int) -> int:
    """Byte offset in ``Mxfp4Weight.ss`` of the scale of the MX block that holds
    W[n][k]; the twin of the scale address of k_mxfp4_gemm_skinny."""
    if K % 256 or not 0 <= k < K:
        raise ValueError(f"mxfp4_scale_offset: k={k} (0 <= k < K), K={K} (K % 256 == 0)")
    return ((n // 16) * (K // 256) + k // 256) * 128 + (((k % 128) // 32) * 16 + n % 16) * 2 + (k % 256) // 128


def mxfp4_linear_q(xq: torch.Tensor, sx: torch.Tensor, w: Mxfp4Weight,
                   resid: Optional[torch.Tensor] = None, tiled: bool = False) -> torch.Tensor:
    """y = (xq @ deq(W)^T) * sx[m] (+ resid, fused into the epilogue) on
    already-quantised e4m3 rows, as fp8_linear_q; bf16 out.  M > 64 without a
    residual runs one launch per 64 rows.  ``tiled`` (opt-in, no resid,
    N % 128 == 0): one launch of the LDS-tiled fp4 GEMM (gemm_mxfp4) for any M
    instead.  The library takes raw pointers, so everything it reads is checked
    here first."""
    lead = xq.shape[:-1]
    if xq.dtype != torch.float8_e4m3fn or xq.shape[-1] != w.K or not xq.is_contiguous():
        raise ValueError(f"mxfp4_linear_q: need contiguous e4m3fn [..., {w.K}], got {xq.dtype} {tuple(xq.shape)}")
    M = xq.numel() // w.K
    if M == 0:
        raise ValueError(f"mxfp4_linear_q: xq {tuple(xq.shape)} has no rows")
    if sx.dtype != torch.float32 or not sx.is_contiguous() or sx.numel() != M:
        raise ValueError(f"mxfp4_linear_q: sx must be contiguous fp32 with {M} elements, got {sx.dtype} "
                         f"{tuple(sx.shape)} contiguous={sx.is_contiguous()}")
    if resid is not None and (resid.dtype != torch.bfloat16 or not resid.is_contiguous()
                              or resid.numel() != M * w.N):
        raise ValueError(f"mxfp4_linear_q: resid must be contiguous bf16 with {M} x {w.N} elements, got "
                         f"{resid.dtype} {tuple(resid.shape)} contiguous={resid.is_contiguous()}")
    if w.qs.dtype != torch.uint8 or w.qs.numel() != w.N * w.K // 2 or not w.qs.is_contiguous() \
            or w.ss.dtype != torch.uint8 or w.ss.numel() != w.N * w.K // MXFP4_BLOCK or not w.ss.is_contiguous():
        raise ValueError(f"mxfp4_linear_q: weight [{w.N}, {w.K}] with codes {w.qs.dtype} {tuple(w.qs.shape)}, scales "
                         f"{w.ss.dtype} {tuple(w.ss.shape)}")
    for name, t in (("xq", xq), ("sx", sx), ("weight", w.qs), ("weight scale", w.ss), ("resid", resid)):
        if t is not None and not t.is_cuda:
            raise ValueError(f"mxfp4_linear_q: {name} must be a CUDA tensor, got {t.device}")
        if t is not None and t.device != xq.device:
            raise ValueError(f"mxfp4_linear_q: {name} is on {t.device}, xq on {xq.device}")
    if resid is not None and M > FP8_M_TILE:
        raise ValueError(f"mxfp4_linear_q: resid {tuple(resid.shape)} for [{M}, {w.N}] (M <= {FP8_M_TILE})")
    y = torch.empty(*lead, w.N, dtype=torch.bfloat16, device=xq.device)
    if tiled and resid is None and w.N % 128 == 0:
        gemm_mxfp4(xq.view(M, w.K), sx.reshape(M), w, y.view(M, w.N))
        return y
    L, st = lib(), _stream()
    if resid is not None:
        _check(L.gpbs_hip_mxfp4_linear_res(_ptr(xq), _ptr(sx), _ptr(w.qs), _ptr(w.ss), _ptr(y), _ptr(resid), M, w.N,
                                           w.K, st), "mxfp4_linear_res")
        return y
    if M <= FP8_M_TILE:
        _check(L.gpbs_hip_mxfp4_linear(_ptr(xq), _ptr(sx), _ptr(w.qs), _ptr(w.ss), _ptr(y), M, w.N, w.K, st),
               "mxfp4_linear")
        return y
    x2, s2, y2 = xq.view(M, w.K), sx.reshape(M), y.view(M, w.N)
    for m0 in range(0, M, FP8_M_TILE):
        m1 = min(M, m0 + FP8_M_TILE)
        _check(L.gpbs_hip_mxfp4_linear(_ptr(x2[m0:m1]), _ptr(s2[m0:m1]), _ptr(w.qs), _ptr(w.ss), _ptr(y2[m0:m1]),
                                       m1 - m0, w.N, w.K, st), "mxfp4_linear")
    return y


def mxfp4_linear(x: torch.Tensor, w: Mxfp4Weight, tiled: bool = False) -> torch.Tensor:
    """y = x @ deq(W)^T with x [..., K] bf16 quantised per token to fp8 on the
    fly.  ``tiled``: as mxfp4_linear_q."""
    xq, sx = quant_rows_fp8(x)
    return mxfp4_linear_q(xq, sx, w, tiled=tiled)


def mxfp4_linear_ref(xq: torch.Tensor, sx: torch.Tensor, w: Mxfp4Weight) -> torch.Tensor:
    """fp64 [M, N] product of the activation codes, the dequantised weight and sx."""
    x = xq.reshape(-1, w.K).double()
    return x @ w.dequant().double().t() * sx.reshape(-1, 1).double()


def mxfp4_as_fp8(w: Mxfp4Weight) -> Fp8Weight:
    """The Fp8Weight that holds exactly deq(w): code * 2^E is an e4m3 value times
    the row scale 2^(Emax - 6) while the block exponents of a row (blocks of
    zeros aside) span at most 15 binades: 6 * 2^6 = 384 is the largest e4m3
    value needed and 0.5 * 2^-8 the subnormal step.  ValueError otherwise."""
    c, e = w.codes, w.scales.to(torch.int32) - 127
    live = ((c.view(w.N, -1, MXFP4_BLOCK // 2) & 0x77) != 0).any(-1)  # blocks with a non-zero code
    hi = torch.where(live, e, torch.full_like(e, -1000)).amax(-1)
    lo = torch.where(live, e, torch.full_like(e, 1000)).amin(-1)
    hi, lo = torch.where(hi < -500, torch.zeros_like(hi), hi), torch.where(lo > 500, torch.zeros_like(lo), lo)
    bad = ((hi - lo > 14) | (hi - 6 < -126)).nonzero().flatten()
    if bad.numel():
        n = int(bad[0])
        raise ValueError(f"mxfp4_as_fp8: the block exponents of row {n} span {int(hi[n] - lo[n]) + 1} binades "
                         f"([{int(lo[n])}, {int(hi[n])}]); an e4m3 row with one power-of-two scale holds 15")
    s = ((hi - 6 + 127) << 23).to(torch.int32).view(torch.float32)
    inv = ((127 - (hi - 6)) << 23).to(torch.int32).view(torch.float32)
    d = w.dequant()
    q = (d * inv.unsqueeze(1)).to(torch.float8_e4m3fn)
    if not torch.equal(q.float() * s.unsqueeze(1), d):
        raise ValueError("mxfp4_as_fp8: the e4m3 copy is not exact")
    return Fp8Weight.from_quantised(q, s)


def linear_q(xq: torch.Tensor, sx: torch.Tensor, w, resid: Optional[torch.Tensor] = None,
             tiled: bool = False, tiled4: bool = False) -> torch.Tensor:
    """The decoder's linear on quantised rows, by the weight's type: fp8_linear_q
    with ``tiled`` for an Fp8Weight, mxfp4_linear_q with ``tiled4`` as its
    ``tiled`` for an Mxfp4Weight.  The two flags are separate: ``tiled`` with an
    Mxfp4Weight stays an error (it asks for the fp8 GEMM, which cannot read fp4
    codes), and ``tiled4`` is ignored for an Fp8Weight."""
    if isinstance(w, Mxfp4Weight):
        if tiled:
            raise ValueError("linear_q: there is no tiled fp4 GEMM under tiled=True (tiled4=True selects it)")
        return mxfp4_linear_q(xq, sx, w, resid=resid, tiled=tiled4)
    return fp8_linear_q(xq, sx, w, resid=resid, tiled=tiled)


# --------------------------------------------------------------------------- token sampling (csrc/hip/sample_kernels.hip)
# Temperature, top-k and top-p sampling of one token per row, defined in integers so that the kernel and the torch
# reference agree on every token bit for bit.  One row x[V] (bf16 or fp32; -inf allowed, NaN / +inf / an all -inf row
# are outside the contract) with inv_temp fp32 (0 = greedy; the host computes fp32(1) / fp32(T)), top_k int32 (active
# iff 0 < top_k < V), top_p fp32 (active iff top_p < 1), seed int64 and ctr int32:
#   idle     ctr < 0: token 0, stats 0.
#   greedy   inv_temp == 0: the lowest index of the maximum, stats 0.
#   weights  m = max x; y = max(((x - m) * inv_temp) * fp32(log2 e), -64), each operation one fp32 rounding;
#            n = floor(y), f = y - n; p = 1 + f (c0 + f (c1 + ... + f c5)) in Horner steps of a separate fp32 multiply
#            and add (no fused multiply-add); w = floor(p * 2^30) >> min(-n, 63): an integer in [0, 2^30].
#   top-k    t = 1 (zero weights are never kept); active: t = max(1, k-th largest w); ties at t are all kept.
#   top-p    after top-k: S_k = sum of the w >= t, P = clamp(floor(top_p * 65536), 0, 65535),
#            target = max(1, floor(S_k * P / 65536)); t becomes the largest v whose weights >= v sum to >= target.
#   draw     S, cnt = sum and number of the w >= t; R = 64 bits of Philox4x32-10, counter (ctr, 0, 0, 0), key (low,
#            high word of seed), R = out[0] + 2^32 out[1]; r = floor(R * S / 2^64); the token is the smallest i whose
#            kept weights up to and including i sum to more than r.
#   stats    int64 (t, cnt, S, r).
# Every sum is an integer sum, hence the same in any order over lanes, waves or workgroups.  V <= 2^20 keeps S < 2^50.
SAMPLE_EXP2_COEF = tuple(float.fromhex(h) for h in ("0x1.62e42cp-1", "0x1.ebfd5ap-3", "0x1.c688f0p-5", "0x1.3d0c40p-7",
                                                    "0x1.46d326p-10", "0x1.c54640p-13"))  # c0 .. c5, mirrored in the .hip
SAMPLE_LOG2E = float.fromhex("0x1.715476p+0")  # fp32(log2 e)
SAMPLE_MAX_V = 1 << 20
_PHILOX_M = (0xD2511F53, 0xCD9E8D57)
_PHILOX_W = (0x9E3779B9, 0xBB67AE85)


def philox4x32_ref(counter, key):
    """Philox4x32-10 on Python integers: counter 4 words, key 2 words -> 4 words."""
    c, k = [int(v) & 0xFFFFFFFF for v in counter], [int(v) & 0xFFFFFFFF for v in key]
    for rnd in range(10):
        p0, p1 = _PHILOX_M[0] * c[0], _PHILOX_M[1] * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + _PHILOX_W[0]) & 0xFFFFFFFF, (k[1] + _PHILOX_W[1]) & 0xFFFFFFFF]
    return c


def sample_exp2_poly(f: torch.Tensor) -> torch.Tensor:
    """p(f) ~ 2^f for fp32 f in [0, 1]: the Horner steps of the contract, every multiply and add a torch op of its
    own (one fp32 rounding each)."""
    c = [torch.tensor(v, dtype=torch.float32, device=f.device) for v in SAMPLE_EXP2_COEF]
    p = c[5]
    for ci in reversed(c[:5]):
        p = f * p
        p = p + ci
    p = f * p
    return p + torch.tensor(1.0, dtype=torch.float32, device=f.device)


def sample_weights_ref(x: torch.Tensor, inv_temp: torch.Tensor) -> torch.Tensor:
    """The integer weights of the contract: x [B, V] (bf16 / fp32), inv_temp fp32 [B] (> 0; a greedy row has no
    weights) -> int64 [B, V] in [0, 2^30]."""
    xf = x.float()
    m = xf.amax(-1, keepdim=True)
    y = (xf - m) * inv_temp.to(torch.float32).view(-1, 1)
    y = y * torch.tensor(SAMPLE_LOG2E, dtype=torch.float32, device=x.device)
    y = torch.clamp_min(y, -64.0)
    n = torch.floor(y)
    q = torch.floor(sample_exp2_poly(y - n) * float(1 << 30)).to(torch.int64)
    return q >> (-n).to(torch.int64).clamp(max=63)


def sample_ref(logits: torch.Tensor, inv_temp: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
               seed: torch.Tensor, ctr: torch.Tensor):
    """Plain-torch reference of sample() on any device: logits [B, V], vectors [B] -> (tokens int64 [B, 1], stats
    int64 [B, 4]).  Reads its vectors and the row sums on the host."""
    if logits.dim() != 2 or logits.dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"sample_ref: logits {tuple(logits.shape)} {logits.dtype} must be bf16 / fp32 [B, V]")
    B, V = logits.shape
    for name, t in (("inv_temp", inv_temp), ("top_k", top_k), ("top_p", top_p), ("seed", seed), ("ctr", ctr)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != B:
            raise ValueError(f"sample_ref: {name} must be a tensor of exactly B={B} elements, got "
                             f"{tuple(getattr(t, 'shape', ()))}")
    if not 1 <= V <= SAMPLE_MAX_V:
        raise ValueError(f"sample_ref: V={V} must be in [1, 2^20]")
    dev = logits.device
    it = inv_temp.to(device=dev, dtype=torch.float32)
    idle, greedy = (ctr.to(dev) < 0).view(B, 1), (it == 0).view(B, 1)
    xf = logits.float()
    ar = torch.arange(V, device=dev)
    first_max = torch.where(xf == xf.amax(-1, keepdim=True), ar, V).amin(-1, keepdim=True)
    w = sample_weights_ref(logits, torch.where(it == 0, torch.ones_like(it), it))
    ws = w.sort(-1, descending=True).values
    k = top_k.to(dev).long().view(B, 1)
    k_on = (k > 0) & (k < V)
    t = torch.where(k_on, ws.gather(1, (k - 1).clamp(0, V - 1)), 1).clamp(min=1)
    s_k = (w * (w >= t)).sum(-1, keepdim=True)
    tp = top_p.to(device=dev, dtype=torch.float32).view(B, 1)
    P = torch.floor(tp * 65536.0).clamp(0, 65535).to(torch.int64)
    target = ((s_k >> 16) * P + (((s_k & 0xFFFF) * P) >> 16)).clamp(min=1)
    j = torch.searchsorted(ws.cumsum(-1), target).clamp(max=V - 1)  # first j whose descending prefix sum reaches target
    t = torch.where(tp < 1, ws.gather(1, j), t)
    kept = w * (w >= t)
    S, cnt = kept.sum(-1), (w >= t).sum(-1)
    r = []
    for b, (s_b, seed_b, ctr_b) in enumerate(zip(S.tolist(), seed.tolist(), ctr.tolist())):
        seed_b &= 0xFFFFFFFFFFFFFFFF
        out = philox4x32_ref((max(ctr_b, 0), 0, 0, 0), (seed_b & 0xFFFFFFFF, seed_b >> 32))
        r.append(((out[0] + (out[1] << 32)) * s_b) >> 64)
    r = torch.tensor(r, dtype=torch.int64, device=dev).view(B, 1)
    tok = torch.searchsorted(kept.cumsum(-1), r, right=True).clamp(max=V - 1)
    tok = torch.where(greedy, first_max, tok)
    stats = torch.cat([t, cnt.view(B, 1), S.view(B, 1), r], 1)
    off = idle | greedy
    return torch.where(idle, torch.zeros_like(tok), tok), torch.where(off, torch.zeros_like(stats), stats)


def sample(logits: torch.Tensor, inv_temp: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
           seed: torch.Tensor, ctr: torch.Tensor, stats: bool = False):
    """One token per row by the contract above (k_sample_rows, one workgroup per row): logits bf16 [B, V] with
    V % 8 == 0 and 8 <= V <= 2^20; inv_temp / top_p fp32 [B], top_k / ctr int32 [B], seed int64 [B], all on the
    GPU.  The kernel reads the five vectors at run time (valid inside a captured graph, which then follows their
    values); only the host side of them is checked.  Returns tokens int64 [B, 1], with stats=True also the int64
    [B, 4] rows (t, cnt, S, r).  Bit-equal to sample_ref."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2:
        raise ValueError(f"sample: logits must be [B, V], got {tuple(getattr(logits, 'shape', ()))}")
    _need(logits, "sample logits")
    B, V = logits.shape
    if B < 1 or V % 8 or not 8 <= V <= SAMPLE_MAX_V:
        raise ValueError(f"sample: logits {tuple(logits.shape)} need B >= 1, V % 8 == 0 and 8 <= V <= 2^20")
    for name, t, dt in (("inv_temp", inv_temp, torch.float32), ("top_k", top_k, torch.int32),
                        ("top_p", top_p, torch.float32), ("seed", seed, torch.int64), ("ctr", ctr, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or t.numel() != B:
            raise ValueError(f"sample: {name} must be a {dt} tensor of exactly B={B} elements, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")
        if not t.is_contiguous():
            raise ValueError(f"sample: {name} must be contiguous (strides {t.stride()})")
        if not t.is_cuda or t.device != logits.device:
            raise ValueError(f"sample: {name} must be on the logits' device {logits.device} (the kernel reads it), "
                             f"got {t.device}")
    tok = torch.empty(B, 1, dtype=torch.int64, device=logits.device)
    st = torch.empty(B, 4, dtype=torch.int64, device=logits.device)
    _check(lib().gpbs_hip_sample_rows(_ptr(logits), _ptr(inv_temp), _ptr(top_k), _ptr(top_p), _ptr(seed), _ptr(ctr),
                                      _ptr(tok), _ptr(st), B, V, _stream()), "sample_rows")
    return (tok, st) if stats else tok
