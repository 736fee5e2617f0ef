"""Llama-3 family tenants (BASELINE config #5: "Llama-3-8B inference
co-located with a bf16 training tenant").

Random-initialised weights of the published architecture (no checkpoints
exist offline): GQA attention with RoPE (theta 500k), SwiGLU MLP, RMSNorm,
bf16 parameters and activations.  Two entry points:

* ``LlamaDecoder`` -- inference: prefill into a static KV cache sized for the
  full context, then one-token decode steps.  On a GPU the decode path runs
  the fused gfx950 kernels of ``pbs_amd.ops.llm`` (RMSNorm, SwiGLU, RoPE) and
  hipBLASLt for the projections; ``fused=False`` is the eager reference.
* ``LlamaTrainer`` -- training: causal-LM loss, backward, fused AdamW step
  (autograd through the PyTorch ops; bf16 weights, fp32 optimizer state).

Sizes are the real ones ("llama3-8b": 8.03 B parameters, 16 GB bf16); the
small presets exist for tests.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .paging import PagePool, PoolExhausted  # noqa: F401  (PoolExhausted is part of the decoder's interface)


@dataclass
class LlamaConfig:
    dim: int = 4096
    n_layers: int = 32
    n_heads: int = 32
    n_kv_heads: int = 8
    ffn_dim: int = 14336
    vocab: int = 128256
    rope_theta: float = 500000.0
    norm_eps: float = 1e-5
    max_seq: int = 8192

    @property
    def head_dim(self) -> int:
        return self.dim // self.n_heads

    def n_params(self) -> int:
        hd = self.head_dim
        attn = self.dim * (self.n_heads * hd) * 2 + self.dim * (self.n_kv_heads * hd) * 2
        mlp = 3 * self.dim * self.ffn_dim
        return self.n_layers * (attn + mlp + 2 * self.dim) + 2 * self.vocab * self.dim + self.dim


PRESETS = {
    "llama3-8b": LlamaConfig(),
    "llama3-1b": LlamaConfig(dim=2048, n_layers=16, n_heads=32, n_kv_heads=8, ffn_dim=8192),
    "tiny": LlamaConfig(dim=256, n_layers=2, n_heads=8, n_kv_heads=2, ffn_dim=512, vocab=1024, max_seq=256),
}


def rope_tables(cfg: LlamaConfig, device, dtype=torch.float32):
    hd = cfg.head_dim
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, hd, 2, device=device, dtype=torch.float64) / hd))
    t = torch.arange(cfg.max_seq, device=device, dtype=torch.float64)
    f = torch.outer(t, inv)
    return f.cos().to(dtype), f.sin().to(dtype)  # [max_seq, hd/2]


def apply_rope_ref(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """x [B, S, H, hd] (interleaved pairs), cos/sin [S, hd/2]."""
    xf = x.float().unflatten(-1, (-1, 2))
    a, b = xf[..., 0], xf[..., 1]
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    return torch.stack((a * c - b * s, a * s + b * c), dim=-1).flatten(-2).to(x.dtype)


def apply_rope_seq_ref(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos) -> torch.Tensor:
    """apply_rope_ref with one start position per sequence: token s of sequence b
    is rotated at angle row pos[b] + s (clamped into the tables: rows of idle
    slots and padding tokens are never used).  x [B, S, H, hd], cos/sin
    [max_seq, hd/2], pos B ints.  Same arithmetic as apply_rope_ref."""
    S = x.shape[1]
    rows = torch.as_tensor(pos, device=x.device, dtype=torch.long)[:, None] + torch.arange(S, device=x.device)
    rows = rows.clamp(0, cos.shape[0] - 1)
    xf = x.float().unflatten(-1, (-1, 2))
    a, b = xf[..., 0], xf[..., 1]
    c, s = cos[rows][:, :, None, :], sin[rows][:, :, None, :]
    return torch.stack((a * c - b * s, a * s + b * c), dim=-1).flatten(-2).to(x.dtype)


class RMSNorm(nn.Module):
    def __init__(self, dim: int, eps: float):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps)).to(x.dtype) * self.weight


class Block(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        hd = cfg.head_dim
        self.cfg = cfg
        self.attn_norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.wq = nn.Linear(cfg.dim, cfg.n_heads * hd, bias=False)
        self.wk = nn.Linear(cfg.dim, cfg.n_kv_heads * hd, bias=False)
        self.wv = nn.Linear(cfg.dim, cfg.n_kv_heads * hd, bias=False)
        self.wo = nn.Linear(cfg.n_heads * hd, cfg.dim, bias=False)
        self.mlp_norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.w1 = nn.Linear(cfg.dim, cfg.ffn_dim, bias=False)  # gate
        self.w3 = nn.Linear(cfg.dim, cfg.ffn_dim, bias=False)  # up
        self.w2 = nn.Linear(cfg.ffn_dim, cfg.dim, bias=False)  # down

    def attention(self, h, cos, sin, cache=None, pos: int = 0, fused: bool = False, prefill_attn: bool = False,
                  seq=None, kv8: bool = False):
        B, S, _ = h.shape
        cfg, hd = self.cfg, self.cfg.head_dim
        q = self.wq(h).view(B, S, cfg.n_heads, hd)
        k = self.wk(h).view(B, S, cfg.n_kv_heads, hd)
        v = self.wv(h).view(B, S, cfg.n_kv_heads, hd)
        if kv8:  # eager reference of the fp8 cache: v now, k after RoPE, as the kernels quantise them
            from ..ops import llm
            v = llm.kv8_round(v)
        if seq is not None:  # ragged eager reference: host positions / lengths per sequence
            from ..ops import llm
            pos_b, lens = seq
            kc, vc = cache
            q, k = apply_rope_seq_ref(q, cos, sin, pos_b), apply_rope_seq_ref(k, cos, sin, pos_b)
            if kv8:
                k = llm.kv8_round(k)
            for b in range(B):
                n = llm.seq_tokens(pos_b[b], lens[b], S, kc.shape[2])
                if n:
                    kc[b, :, pos_b[b]:pos_b[b] + n] = k[b, :n].transpose(0, 1)
                    vc[b, :, pos_b[b]:pos_b[b] + n] = v[b, :n].transpose(0, 1)
            return self.wo(llm.attn_seq_ref(q, kc, vc, pos_b, lens).to(h.dtype))
        if fused:
            from ..ops import llm
            q, k = llm.rope(q, cos, sin, pos), llm.rope(k, cos, sin, pos)
        else:
            q = apply_rope_ref(q, cos[pos:pos + S], sin[pos:pos + S])
            k = apply_rope_ref(k, cos[pos:pos + S], sin[pos:pos + S])
        if kv8:
            k = llm.kv8_round(k)
        if cache is not None:
            kc, vc = cache
            kc[:, :, pos:pos + S] = k.transpose(1, 2)
            vc[:, :, pos:pos + S] = v.transpose(1, 2)
            if prefill_attn and S > 1:  # causal mask offset by pos: correct for any chunk of a prompt
                from ..ops import llm
                if fused:
                    return self.wo(llm.prefill_attn(q, kc, vc, pos))
                return self.wo(llm.prefill_attn_ref(q, kc, vc, pos).to(h.dtype))
            k_all, v_all = kc[:, :, :pos + S], vc[:, :, :pos + S]
        else:
            k_all, v_all = k.transpose(1, 2), v.transpose(1, 2)
        # GQA without materialising repeated K/V (at decode the cache read is
        # the attention cost; repeat_interleave would read+write it 4x more)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), k_all, v_all, is_causal=(S > 1), enable_gqa=True)
        return self.wo(o.transpose(1, 2).reshape(B, S, cfg.n_heads * hd))

    def attach_fp8(self):
        """Quantise this block's linears to e4m3fn for the fp8 decode path:
        q/k/v packed into one [(H + 2 Hkv) hd, dim] weight, gate/up into one
        [2 ffn, dim] weight, so a decode step streams each layer in 4 launches."""
        from ..ops import llm
        self._fp8 = {
            "qkv": llm.Fp8Weight(torch.cat([self.wq.weight, self.wk.weight, self.wv.weight], 0)),
            "o": llm.Fp8Weight(self.wo.weight),
            "w13": llm.Fp8Weight(torch.cat([self.w1.weight, self.w3.weight], 0)),
            "w2": llm.Fp8Weight(self.w2.weight),
        }

    def attach_mxfp4(self, emulate: bool = False):
        """The four packed weights of attach_fp8 as MXFP4 (llm.Mxfp4Weight: e2m1
        codes, one E8M0 scale per 32 k, 4.25 bits per weight); forward_fp8 and
        decode_fp8_static then run the fp4 linear.  ``emulate``: the oracle,
        Fp8Weight copies that hold exactly the dequantised MX weights, for the
        stock fp8 kernels (ValueError if a row's block exponents do not fit one
        e4m3 row scale)."""
        from ..ops import llm
        # _fp8 keeps its name from attach_fp8: the packed weights of the fp8 activation path, by linear; a value is
        # an Fp8Weight or an Mxfp4Weight, and llm.linear_q picks the kernel by that type
        self._fp8 = {}
        for name, w in (("qkv", torch.cat([self.wq.weight, self.wk.weight, self.wv.weight], 0)),
                        ("o", self.wo.weight), ("w13", torch.cat([self.w1.weight, self.w3.weight], 0)),
                        ("w2", self.w2.weight)):
            mx = llm.Mxfp4Weight(w)
            self._fp8[name] = llm.mxfp4_as_fp8(mx) if emulate else mx

    def forward_fp8(self, x, cos, sin, cache, pos: int, tiled: bool = False, view=None, tiled4: bool = False):
        """Decode/prefill block on fp8 weights (fp8 MFMA linears + fused gfx950
        RMSNorm/RoPE/SwiGLU); inference only.  ``tiled``: the linears run the
        LDS-tiled fp8 GEMM (one launch for any M) where their N allows it.
        ``tiled4``: the same for MXFP4 weights and the tiled fp4 GEMM.
        ``view``: this layer's cache view (ops.llm: DenseUniform, DenseSeq,
        Paged, ...); the attention block is then two gfx950 launches, write and
        attend, in the view's form, and ``cache`` / ``pos`` are not used.
        Without one: RoPE, cache copies and SDPA on ``cache`` = (kc, vc).  The
        choice is the caller's: Llama.forward_fp8 builds the uniform view for
        prefill_attn, this method never does."""
        from ..ops import llm
        cfg, hd, f = self.cfg, self.cfg.head_dim, self._fp8
        B, S, _ = x.shape
        qkv = llm.linear_q(*llm.rmsnorm_quant_fp8(x, self.attn_norm.weight, self.attn_norm.eps), f["qkv"], tiled=tiled,
                           tiled4=tiled4)
        nq, nkv = cfg.n_heads * hd, cfg.n_kv_heads * hd
        if view is not None:
            o = llm.attend_prefill(view, llm.write_prefill(view, qkv, cos, sin, cfg.n_heads))
        else:
            kc, vc = cache
            q = qkv[..., :nq].reshape(B, S, cfg.n_heads, hd)
            k = qkv[..., nq:nq + nkv].reshape(B, S, cfg.n_kv_heads, hd)
            v = qkv[..., nq + nkv:].reshape(B, S, cfg.n_kv_heads, hd)
            q, k = llm.rope(q, cos, sin, pos), llm.rope(k, cos, sin, pos)
            kc[:, :, pos:pos + S] = k.transpose(1, 2)
            vc[:, :, pos:pos + S] = v.transpose(1, 2)
            o = F.scaled_dot_product_attention(q.transpose(1, 2), kc[:, :, :pos + S], vc[:, :, :pos + S],
                                               is_causal=(S > 1), enable_gqa=True)
            o = o.transpose(1, 2).reshape(B, S, nq)
        x = x + llm.linear_q(*llm.quant_rows_fp8(o), f["o"], tiled=tiled, tiled4=tiled4)
        gu = llm.linear_q(*llm.rmsnorm_quant_fp8(x, self.mlp_norm.weight, self.mlp_norm.eps), f["w13"], tiled=tiled,
                          tiled4=tiled4)
        return x + llm.linear_q(*llm.swiglu_quant_fp8(gu), f["w2"], tiled=tiled, tiled4=tiled4)

    def decode_fp8_static(self, x, cos, sin, cache, pos_i32, pos_i64, mask, view=None):
        """One-token decode with every shape static and the position on device
        (capturable in a HIP graph).  ``view``: this layer's cache view (as in
        forward_fp8, whose position tensors the captured graph keeps reading):
        two gfx950 launches, write and attend, between the qkv and o linears;
        ``cache`` and the three position arguments are not used.  Without one:
        the KV row is written with index_copy_ at pos, and attention runs over
        the whole static cache with an additive mask, grouped per KV head (GQA
        without repeating K/V), for any head geometry.  The choice is the
        caller's: Llama.decode_fp8_static builds the uniform view where the
        kernels take the geometry (head_dim 128), this method never does."""
        from ..ops import llm
        cfg, hd, f = self.cfg, self.cfg.head_dim, self._fp8
        B = x.shape[0]
        G = cfg.n_heads // cfg.n_kv_heads
        qkv = llm.linear_q(*llm.rmsnorm_quant_fp8(x, self.attn_norm.weight, self.attn_norm.eps), f["qkv"])
        nq, nkv = cfg.n_heads * hd, cfg.n_kv_heads * hd
        if view is not None:
            o = llm.attend_decode(view, llm.write_decode(view, qkv, cos, sin, cfg.n_heads))
            x = llm.linear_q(*llm.quant_rows_fp8(o.view(B, 1, nq)), f["o"], resid=x)
            gu = llm.linear_q(*llm.rmsnorm_quant_fp8(x, self.mlp_norm.weight, self.mlp_norm.eps), f["w13"])
            return llm.linear_q(*llm.swiglu_quant_fp8(gu), f["w2"], resid=x)
        kc, vc = cache
        q = llm.rope_dpos(qkv[..., :nq].reshape(B, 1, cfg.n_heads, hd), cos, sin, pos_i32)
        k = llm.rope_dpos(qkv[..., nq:nq + nkv].reshape(B, 1, cfg.n_kv_heads, hd), cos, sin, pos_i32)
        v = qkv[..., nq + nkv:].reshape(B, 1, cfg.n_kv_heads, hd)
        kc.index_copy_(2, pos_i64, k.transpose(1, 2))
        vc.index_copy_(2, pos_i64, v.transpose(1, 2))
        qg = q.view(B, cfg.n_kv_heads, G, hd)
        sc = torch.matmul(qg, kc.transpose(-1, -2)).float() * (hd ** -0.5) + mask
        o = torch.matmul(torch.softmax(sc, -1).to(vc.dtype), vc)  # [B, Hkv, G, hd]
        x = x + llm.linear_q(*llm.quant_rows_fp8(o.reshape(B, 1, nq)), f["o"])
        gu = llm.linear_q(*llm.rmsnorm_quant_fp8(x, self.mlp_norm.weight, self.mlp_norm.eps), f["w13"])
        return x + llm.linear_q(*llm.swiglu_quant_fp8(gu), f["w2"])

    def forward(self, x, cos, sin, cache=None, pos: int = 0, fused: bool = False, prefill_attn: bool = False,
                seq=None, kv8: bool = False):
        if seq is not None:  # ragged: the eager reference path only
            x = x + self.attention(self.attn_norm(x), cos, sin, cache, seq=seq, kv8=kv8)
            h = self.mlp_norm(x)
            return x + self.w2(F.silu(self.w1(h)) * self.w3(h))
        if fused:
            from ..ops import llm
            h = llm.rmsnorm(x, self.attn_norm.weight, self.attn_norm.eps)
            x = x + self.attention(h, cos, sin, cache, pos, fused=True, prefill_attn=prefill_attn)
            h = llm.rmsnorm(x, self.mlp_norm.weight, self.mlp_norm.eps)
            return x + self.w2(llm.swiglu(self.w1(h), self.w3(h)))
        x = x + self.attention(self.attn_norm(x), cos, sin, cache, pos, prefill_attn=prefill_attn, kv8=kv8)
        h = self.mlp_norm(x)
        return x + self.w2(F.silu(self.w1(h)) * self.w3(h))


class Llama(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        self.embed = nn.Embedding(cfg.vocab, cfg.dim)
        self.layers = nn.ModuleList(Block(cfg) for _ in range(cfg.n_layers))
        self.norm = RMSNorm(cfg.dim, cfg.norm_eps)
        self.lm_head = nn.Linear(cfg.dim, cfg.vocab, bias=False)
        self._rope = None

    @torch.no_grad()
    def init_random(self, std: float = 0.02, seed: int = 0):
        g = torch.Generator(device=next(self.parameters()).device).manual_seed(seed)
        for n, p in self.named_parameters():
            if n.endswith("norm.weight"):
                p.fill_(1.0)
            else:
                p.normal_(0.0, std, generator=g)
        return self

    def rope(self, device):
        if self._rope is None or self._rope[0].device != device:
            self._rope = rope_tables(self.cfg, device)
        return self._rope

    def attach_fp8(self):
        """fp8 (e4m3fn) copies of every block linear and the LM head."""
        from ..ops import llm
        for layer in self.layers:
            layer.attach_fp8()
        self._fp8_head = llm.Fp8Weight(self.lm_head.weight)
        return self

    def attach_mxfp4(self, emulate: bool = False):
        """MXFP4 copies of every block linear (Block.attach_mxfp4); the LM head
        stays fp8 (e4m3fn)."""
        from ..ops import llm
        for layer in self.layers:
            layer.attach_mxfp4(emulate=emulate)
        self._fp8_head = llm.Fp8Weight(self.lm_head.weight)
        return self

    def forward_fp8(self, tokens, cache, pos: int = 0, last_only: bool = False, tiled: bool = False,
                    prefill_attn: bool = False, head: bool = True, last_idx=None, views=None, tiled4: bool = False):
        """``tiled4``: the block linears over MXFP4 weights run the tiled fp4 GEMM
        (Block.forward_fp8); the LM head is an Fp8Weight and follows ``tiled``.
        ``head=False`` (a non-final chunk of a chunked prefill): fill the
        caches only, no final norm / LM head; returns None.  ``last_idx`` (long
        [B]): the head runs on token last_idx[b] of sequence b and the result is
        [B, 1, vocab].  ``views``: one cache view per layer, see
        Block.forward_fp8 (``cache`` / ``pos`` are then not used); without them
        ``prefill_attn`` with S > 1 is the uniform view of ``cache`` at ``pos``."""
        from ..ops import llm
        cos, sin = self.rope(tokens.device)
        x = self.embed(tokens)
        if views is None and prefill_attn and tokens.shape[1] > 1:
            views = [llm.DenseUniform(kc, vc, pos) for kc, vc in cache]
        for i, layer in enumerate(self.layers):
            x = layer.forward_fp8(x, cos, sin, cache[i], pos, tiled=tiled, view=None if views is None else views[i],
                                  tiled4=tiled4)
        if not head:
            return None
        if last_idx is not None:
            x = x[torch.arange(x.shape[0], device=x.device), last_idx].unsqueeze(1).contiguous()
        elif last_only:
            x = x[:, -1:].contiguous()
        return llm.fp8_linear_q(*llm.rmsnorm_quant_fp8(x, self.norm.weight, self.norm.eps), self._fp8_head,
                                tiled=tiled)

    def decode_fp8_static(self, tok, cache, pos_i32=None, pos_i64=None, mask=None, views=None):
        """``views``: one cache view per layer, see Block.decode_fp8_static; without
        them the uniform view of ``cache`` at ``pos_i32`` where the kernels take
        the model's head geometry, the index_copy_ + mask step where not."""
        from ..ops import llm
        cfg = self.cfg
        cos, sin = self.rope(tok.device)
        x = self.embed(tok)
        if views is None and cfg.head_dim == 128 and cfg.n_heads // cfg.n_kv_heads in (1, 2, 4, 8):
            views = [llm.DenseUniform(kc, vc, pos_i32) for kc, vc in cache]
        for i, layer in enumerate(self.layers):
            x = layer.decode_fp8_static(x, cos, sin, cache[i], pos_i32, pos_i64, mask,
                                        view=None if views is None else views[i])
        return llm.fp8_linear_q(*llm.rmsnorm_quant_fp8(x, self.norm.weight, self.norm.eps), self._fp8_head)

    def forward(self, tokens, cache=None, pos: int = 0, fused: bool = False, last_only: bool = False,
                prefill_attn: bool = False, head: bool = True, seq=None, last_idx=None, kv8: bool = False):
        """``seq`` = (pos, lens), B host ints each: a ragged batch on the eager
        reference path (needs a cache; ``pos`` / ``fused`` are not used).
        ``last_idx`` (long [B]): the head runs on token last_idx[b] of sequence b
        and the result is [B, 1, vocab].  ``kv8`` (eager path only): every new
        k / v row is rounded through the fp8 cache codec before it is stored."""
        cos, sin = self.rope(tokens.device)
        x = self.embed(tokens)
        for i, layer in enumerate(self.layers):
            if seq is not None:
                x = layer(x, cos, sin, cache[i], seq=seq, kv8=kv8)
            else:
                x = layer(x, cos, sin, None if cache is None else cache[i], pos, fused, prefill_attn, kv8=kv8)
        if not head:  # a non-final chunk of a chunked prefill: the caches are filled, no logits
            return None
        if seq is not None:
            fused = False
        if last_idx is not None:
            x = x[torch.arange(x.shape[0], device=x.device), last_idx].unsqueeze(1)
        elif last_only:
            x = x[:, -1:]
        x = self.norm(x) if not fused else __import__("pbs_amd.ops.llm", fromlist=["rmsnorm"]).rmsnorm(
            x, self.norm.weight, self.norm.eps)
        return self.lm_head(x)


def build(cfg: LlamaConfig, device, dtype) -> "Llama":
    """Construct directly in `dtype` on `device` (no fp32 transient: 8B
    parameters would otherwise pass through 32 GB of fp32)."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.device(device):
            m = Llama(cfg)
    finally:
        torch.set_default_dtype(prev)
    return m.init_random()


class LlamaDecoder:
    """Inference tenant: static KV cache; greedy decode, or with ``sampling=True``
    temperature / top-k / top-p sampling per slot.

    ``sampling=False`` (the default) picks every token with torch ``argmax``.
    ``sampling=True`` sends every pick -- prefill in all its forms, admit, every
    kind of decode step, the captured graph -- through the integer sampler of
    ``pbs_amd.ops.llm`` ("token sampling"): the gfx950 kernel ``llm.sample`` with
    fp8=True, its bit-equal torch reference ``llm.sample_ref`` on the eager paths
    (any device).  Slots start greedy; ``set_sampling`` sets temperature, top_k,
    top_p and seed of one slot or of all, in static device tensors the captured
    graph reads, so a change holds from the next step on without a recapture.
    The counter of a pick is the index its token will have in its sequence
    (the prompt length after a prefill or admission, pos_b[b] + 1 in a decode
    step), so a request's tokens are a function of its logits, its seed and its
    position alone: not of the other slots, nor of how its prompt was chunked.
    ``last_logits`` [B, V] ([1, V] after an admission) are the logits of the last
    pick; with graph=True the static output tensor of the captured step."""

    def __init__(self, cfg: LlamaConfig, batch: int, context: int, device="cuda", dtype=torch.bfloat16,
                 fused: Optional[bool] = None, fp8: bool = False, graph: bool = False, static: bool = False,
                 prefill_tiled: bool = False, prefill_attn: bool = False, ragged: bool = False,
                 paged: bool = False, pages: Optional[int] = None, page: int = 64, kv_fp8=False,
                 sampling: bool = False, w4=False, w4_tiled: bool = False):
        # opt-in (needs fp8=True): the four block linears of every layer stream MXFP4 weights (ops.llm.Mxfp4Weight:
        # e2m1 codes and one E8M0 scale per 32 k, 4.25 bits per weight where fp8 stores 8) through the fp4 MFMA
        # linear; the LM head stays fp8.  Every mode on top (prefill, chunks, ragged, paged, kv_fp8, sampling, admit,
        # the static step and its graph) runs unchanged.  "emulate": the oracle of the former, the stock fp8
        # kernels over Fp8Weight copies that hold exactly the dequantised MX weights.
        if not (w4 is False or w4 is True or w4 == "emulate"):
            raise ValueError(f"LlamaDecoder: w4 {w4!r} must be False, True or 'emulate'")
        if w4 and not fp8:
            raise ValueError("LlamaDecoder: w4 runs on the fp8 path (needs fp8=True)")
        if w4 is True and prefill_tiled:
            raise ValueError("LlamaDecoder: w4=True with prefill_tiled=True: there is no tiled fp4 GEMM under that "
                             "flag (w4_tiled=True selects it)")
        self.w4 = w4
        # opt-in (needs w4=True): every forward_fp8 call (prefill, chunks, ragged, paged, kv_fp8, admit) runs its
        # block linears as one launch of the LDS-tiled fp4 GEMM each instead of one weight-streaming launch per 64
        # rows; the static step and its graph keep the skinny kernel and the fused residual, the LM head stays fp8
        if w4_tiled and w4 is not True:
            raise ValueError(f"LlamaDecoder: w4_tiled=True runs the tiled fp4 GEMM (needs w4=True, got w4={w4!r})")
        self.w4_tiled = bool(w4_tiled)
        # opt-in (implies ragged): the KV cache is a pool of `pages` pages of
        # `page` rows per layer, [pages, Hkv, page, hd], and one block table
        # [batch, ceil(context / page)] for all layers maps every slot's logical
        # rows to pages.  A slot holds ceil(pos / page) pages, a request that
        # does not fit raises PoolExhausted, and admit(..., share=) maps the
        # full pages of another slot's prefix instead of storing them again.
        self.paged = paged
        # opt-in (needs paged=True): the fp8 KV cache, e4m3 codes with one
        # power-of-two fp32 scale per cached row and KV head (the codec of
        # ops.llm.kv8_quant_ref): 132 bytes per row and KV head where bf16 stores 256.
        #   True with fp8=True: per layer (kpool8, vpool8 float8_e4m3fn
        #     [pages, Hkv, page, hd], kscale, vscale fp32 [pages, Hkv, page]) and the
        #     _kv8 kernels in prefill, chunked prefill, admit(share=), the static
        #     decode step and the captured graph; shared pages carry their scales.
        #   "emulate" with fp8=True: bf16 pools and the bf16 paged kernels; after
        #     every write launch torch ops on the device round exactly the rows it
        #     wrote through the codec.  The oracle of the former; no graph.
        #   True with fp8=False (eager, any device): every new k / v row is rounded
        #     through the codec into pools of the model's dtype.  A numerical
        #     reference only: it saves no memory.
        if not (kv_fp8 is False or kv_fp8 is True or kv_fp8 == "emulate"):
            raise ValueError(f"LlamaDecoder: kv_fp8 {kv_fp8!r} must be False, True or 'emulate'")
        if kv_fp8 and not paged:
            raise ValueError("LlamaDecoder: kv_fp8 needs paged=True (the fp8 cache is a paged cache)")
        if kv_fp8 == "emulate" and not fp8:
            raise ValueError("LlamaDecoder: kv_fp8='emulate' emulates the fp8 kernels' cache (needs fp8=True)")
        if kv_fp8 == "emulate" and graph:
            raise ValueError("LlamaDecoder: kv_fp8='emulate' rounds the written rows with torch ops between the "
                             "launches and cannot be captured (graph=True)")
        self.kv_fp8 = kv_fp8
        if paged:
            ragged = True
            if page not in (64, 128, 256):
                raise ValueError(f"LlamaDecoder: page {page!r} must be 64, 128 or 256")
            if not isinstance(pages, int) or isinstance(pages, bool) or pages < 1:
                raise ValueError(f"LlamaDecoder: paged=True needs pages, a positive int, got {pages!r}")
        if not 0 < context <= cfg.max_seq:  # the RoPE tables cover max_seq positions
            raise ValueError(f"LlamaDecoder: context {context} must be in [1, max_seq={cfg.max_seq}]")
        # opt-in: every sequence of the batch has a cache position of its own
        # (pos_b, -1 = idle slot), so prompts of different lengths share a
        # prefill (prefill(tokens, lens=...)), a finished sequence is released
        # and a new request admitted into its slot while the others keep
        # decoding.  fp8=True runs the per-sequence gfx950 kernels; fp8=False is
        # the eager reference on any device and dtype.  No sliding window.
        # The ragged kernels, and those of prefill_attn below (which ragged implies), take one head geometry.
        G = cfg.n_heads // cfg.n_kv_heads
        if (ragged or prefill_attn) and (cfg.head_dim != 128 or cfg.n_heads % cfg.n_kv_heads
                                         or G not in (1, 2, 4, 8)):
            raise ValueError(f"LlamaDecoder: {'ragged' if ragged else 'prefill_attn'} needs head_dim 128 and "
                             f"n_heads / n_kv_heads in 1/2/4/8, got head_dim {cfg.head_dim}, {cfg.n_heads} / "
                             f"{cfg.n_kv_heads} heads")
        if ragged and fused and not fp8:
            raise ValueError("LlamaDecoder: ragged=True runs on the fp8 kernels (fp8=True) or the eager reference "
                             "(fused=False); there is no fused bf16 ragged path")
        self.ragged = ragged
        if ragged:
            prefill_attn = True  # admit() prefills at the slot's own cache position
            if not fp8:
                fused = False
            else:
                static = True  # every ragged decode step is the static-shape step
        # opt-in: calls with S > 1 run causal GQA attention offset by the cache
        # position (the gfx950 MFMA kernel on the fused / fp8 paths, its torch
        # reference on the eager path), which is what lets a prompt be prefilled
        # in chunks; S == 1 steps and the static / graph decode are untouched
        self.prefill_attn = prefill_attn
        self.cfg, self.batch, self.context = cfg, batch, context
        self.model = build(cfg, device, dtype)
        self.model.eval()
        self.fused = (torch.cuda.is_available() and str(device).startswith("cuda")) if fused is None else fused
        self.fp8 = fp8
        # opt-in: prefill runs the block and head linears on the LDS-tiled fp8
        # GEMM (one launch per linear) instead of one weight-streaming launch
        # per 64 rows; decode steps are untouched
        self.prefill_tiled = prefill_tiled
        if fp8:  # weights streamed as e4m3fn through the fp8 MFMA linears (half the bytes of bf16)
            with torch.no_grad():
                if w4:
                    self.model.attach_mxfp4(emulate=(w4 == "emulate"))
                else:
                    self.model.attach_fp8()
        if (graph or static) and not fp8:
            raise ValueError("static-shape / graph decode is the fp8 path (needs fp8=True)")
        self.graph = graph
        self.static = static or graph  # static shapes + device position; graph=True also captures it
        self._g = self._step = None
        hd = cfg.head_dim
        if paged:
            self.page, self.n_table = page, -(-context // page)
            self.pool = PagePool(pages)
            if kv_fp8 is True and fp8:  # codes and scales; a scale sits at the page index of its row
                self.cache = [(torch.zeros(pages, cfg.n_kv_heads, page, hd, device=device, dtype=torch.float8_e4m3fn),
                               torch.zeros(pages, cfg.n_kv_heads, page, hd, device=device, dtype=torch.float8_e4m3fn),
                               torch.zeros(pages, cfg.n_kv_heads, page, device=device, dtype=torch.float32),
                               torch.zeros(pages, cfg.n_kv_heads, page, device=device, dtype=torch.float32))
                              for _ in range(cfg.n_layers)]
            else:
                self.cache = [(torch.zeros(pages, cfg.n_kv_heads, page, hd, device=device, dtype=dtype),
                               torch.zeros(pages, cfg.n_kv_heads, page, hd, device=device, dtype=dtype))
                              for _ in range(cfg.n_layers)]
            # block table: host mirror (-1 = no page) and the static device tensor the kernels read
            self._pages = [[] for _ in range(batch)]
            self._table = torch.full((batch, self.n_table), -1, dtype=torch.int32, device=device)
        else:
            self.cache = [(torch.zeros(batch, cfg.n_kv_heads, context, hd, device=device, dtype=dtype),
                           torch.zeros(batch, cfg.n_kv_heads, context, hd, device=device, dtype=dtype))
                          for _ in range(cfg.n_layers)]
        self.pos = 0
        # ragged state: cache position of every slot (-1 = idle); self.pos is then
        # the largest active position, for information only
        self.pos_b = [-1] * batch
        self.active = [False] * batch
        # opt-in: see the class docstring.  Host mirror of the per-slot parameters (inv_temp as numpy fp32) and
        # the static device tensors [batch] the sampler reads; every slot starts greedy.
        self.sampling = sampling
        self.last_logits = None
        if sampling:
            self._samp = {"inv_temp": [0.0] * batch, "top_k": [0] * batch, "top_p": [1.0] * batch, "seed": [0] * batch}
            self._inv_temp = torch.zeros(batch, dtype=torch.float32, device=device)
            self._top_k = torch.zeros(batch, dtype=torch.int32, device=device)
            self._top_p = torch.ones(batch, dtype=torch.float32, device=device)
            self._seed = torch.zeros(batch, dtype=torch.int64, device=device)

    def set_sampling(self, slot: Optional[int] = None, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                     seed: int = 0):
        """Sampling parameters of one slot, or of every slot (slot=None); they hold
        from the next pick on (the captured graph reads the same tensors) and
        survive release(): the caller sets them at admission.  temperature 0 is
        greedy; top_k 0 (or >= vocab) and top_p 1 are off."""
        if not self.sampling:
            raise ValueError("LlamaDecoder: set_sampling needs sampling=True")
        if slot is not None and (not isinstance(slot, int) or isinstance(slot, bool) or not 0 <= slot < self.batch):
            raise ValueError(f"LlamaDecoder: slot {slot!r} of a batch of {self.batch}")
        if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not 0 <= temperature < math.inf:
            raise ValueError(f"LlamaDecoder: temperature {temperature!r} must be a finite number >= 0")
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 0 <= top_k < 2 ** 31:
            raise ValueError(f"LlamaDecoder: top_k {top_k!r} must be an int >= 0")
        if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0 < top_p <= 1:
            raise ValueError(f"LlamaDecoder: top_p {top_p!r} must be in (0, 1]")
        if isinstance(seed, bool) or not isinstance(seed, int) or not -2 ** 63 <= seed < 2 ** 63:
            raise ValueError(f"LlamaDecoder: seed {seed!r} must be an int64")
        import numpy as np
        with np.errstate(all="ignore"):  # an overflow is refused below
            inv = float(np.float32(1.0) / np.float32(temperature)) if temperature else 0.0
        if temperature and not 0 < inv < math.inf:
            raise ValueError(f"LlamaDecoder: 1 / temperature {temperature!r} is not a finite positive fp32")
        for b in range(self.batch) if slot is None else (slot,):
            for name, v in (("inv_temp", inv), ("top_k", top_k), ("top_p", float(top_p)), ("seed", seed)):
                self._samp[name][b] = v
        self._inv_temp.copy_(torch.tensor(self._samp["inv_temp"], dtype=torch.float32))
        self._top_k.copy_(torch.tensor(self._samp["top_k"], dtype=torch.int32))
        self._top_p.copy_(torch.tensor(self._samp["top_p"], dtype=torch.float32))
        self._seed.copy_(torch.tensor(self._samp["seed"], dtype=torch.int64))

    def _sample(self, x: torch.Tensor, ctr_t: torch.Tensor, slot: Optional[int] = None) -> torch.Tensor:
        """x [B, V] (slot: [1, V], that slot's parameters) and the counters int32 on x's device -> tokens [B, 1]."""
        from ..ops import llm
        sl = slice(None) if slot is None else slice(slot, slot + 1)
        vec = (self._inv_temp[sl], self._top_k[sl], self._top_p[sl], self._seed[sl], ctr_t)
        if self.fp8:  # the kernel; a missing library is an error, not a reason to run the reference
            return llm.sample(x.contiguous(), *vec)
        return llm.sample_ref(x, *vec)[0]

    def _pick(self, logits: torch.Tensor, ctr, slot: Optional[int] = None) -> torch.Tensor:
        """The next token of every row of logits [B, 1, V] -> [B, 1]: argmax, or with
        sampling=True the sampler at the counters ``ctr`` (ints, -1 = idle row)."""
        x = logits[:, -1]
        if not self.sampling:
            return x.argmax(-1, keepdim=True)
        self.last_logits = x
        return self._sample(x, torch.tensor(ctr, dtype=torch.int32).to(x.device), slot)

    def _forward(self, tokens, pos: int, head: bool = True, cache=None, seq=None, last_idx=None):
        """``cache``: other caches than the decoder's own (admit: the batch-1
        views of one slot).  ``seq`` = (pos, lens), B ints each, and
        ``last_idx``: a ragged batch over the decoder's own caches."""
        cache = self.cache if cache is None else cache
        if self.fp8:
            return self.model.forward_fp8(tokens, cache, pos, last_only=True, tiled=self.prefill_tiled,
                                          prefill_attn=self.prefill_attn, head=head, last_idx=last_idx,
                                          views=None if seq is None else self._views(tokens.device, *seq),
                                          tiled4=self.w4_tiled)
        return self.model(tokens, cache=cache, pos=pos, fused=self.fused, last_only=True,
                          prefill_attn=self.prefill_attn, head=head, seq=seq, last_idx=last_idx)

    def _views(self, dev, pos, lens, table=None):
        """One cache view (ops.llm) per layer for a ragged prefill forward on the
        fp8 kernels, in the form of the decoder's mode: pos / lens (B ints each)
        are uploaded once and every layer's view reads the same two tensors."""
        pos_t, len_t = torch.tensor(pos, dtype=torch.int32).to(dev), torch.tensor(lens, dtype=torch.int32).to(dev)
        return self._layer_views(pos_t, len_t, table)

    def _layer_views(self, pos_t, len_t=None, table=None):
        from ..ops import llm
        if not self.paged:
            return [llm.DenseSeq(kc, vc, pos_t, len_t) for kc, vc in self.cache]
        form = {False: llm.Paged, True: llm.PagedKv8, "emulate": llm.PagedEmulated}[self.kv_fp8]
        return [form(*c, table, pos_t, len_t) for c in self.cache]

    @staticmethod
    def _drain(it):
        while True:
            try:
                next(it)
            except StopIteration as e:
                return e.value

    @torch.no_grad()
    def prefill(self, tokens: torch.Tensor, chunk: Optional[int] = None, lens=None) -> torch.Tensor:
        """Run the prompt into the KV cache and return the next token [B, 1].
        ``chunk``: run it in pieces of at most that many tokens (prefill_iter,
        drained here); needs prefill_attn=True.  ``lens`` (ragged=True): B prompt
        lengths for tokens [B, S] padded to the longest; every slot is reset,
        slot b becomes active with its first lens[b] tokens (0 leaves it idle),
        in one ragged launch per layer; idle rows of the result are 0.
        paged=True: every form is a ragged prefill (no lens: lens = [S] * B, also
        with chunk) after ceil(lens[b] / page) pages were found for every slot."""
        if self.paged:
            return self._prefill_paged(tokens, chunk, lens)
        if lens is not None:
            if not self.ragged:
                raise ValueError("LlamaDecoder: lens needs ragged=True")
            return self._prefill_ragged(tokens, self._lens(tokens, lens, chunk))
        if chunk is not None:
            return self._drain(self.prefill_iter(tokens, chunk))
        self.pos = 0
        logits = self._forward(tokens, 0)
        self.pos = tokens.shape[1]
        self._all_slots_at(self.pos)
        return self._pick(logits, [self.pos] * tokens.shape[0])

    def _all_slots_at(self, pos: int):
        """Ragged mode, after a uniform prefill: every slot is active at the same position."""
        if self.ragged:
            self.pos_b = [pos] * self.batch
            self.active = [True] * self.batch

    def _sync_pos(self):
        self.pos = max((p for p, a in zip(self.pos_b, self.active) if a), default=0)

    def _lens(self, tokens: torch.Tensor, lens, chunk) -> list:
        """The prompt lengths of a ragged prefill as B ints; None: every prompt is
        all of tokens [B, S], the one form that may run in chunks."""
        B, S = tokens.shape
        if lens is not None and chunk is not None:
            raise ValueError("LlamaDecoder: lens with chunk is not supported (a ragged prefill is one launch per "
                             "layer; admit_iter chunks one request)")
        if isinstance(lens, torch.Tensor):
            lens = lens.tolist()
        lens = [S] * B if lens is None else [int(n) for n in lens]
        if B != self.batch or len(lens) != B or any(n < 0 or n > S for n in lens):
            raise ValueError(f"LlamaDecoder: lens {lens} for tokens {tuple(tokens.shape)} and a batch of {self.batch} "
                             f"(one length in [0, S] per slot)")
        if max(lens) > self.context:
            raise ValueError(f"LlamaDecoder: prompt of {max(lens)} tokens for a context of {self.context}")
        return lens

    @staticmethod
    def _chunk(chunk):
        if not isinstance(chunk, int) or isinstance(chunk, bool) or chunk < 1:
            raise ValueError(f"LlamaDecoder: chunk must be a positive int, got {chunk!r}")

    def _prefill_ragged(self, tokens: torch.Tensor, lens) -> torch.Tensor:
        B, dev = tokens.shape[0], tokens.device
        last = torch.tensor([max(n - 1, 0) for n in lens], device=dev)
        self.pos_b, self.active = [-1] * B, [False] * B
        logits = self._forward(tokens, 0, seq=([0 if n else -1 for n in lens], lens), last_idx=last)
        self.pos_b = [n if n else -1 for n in lens]
        self.active = [n > 0 for n in lens]
        self._sync_pos()
        tok = self._pick(logits, self.pos_b)  # the counter is the prompt length, -1 for an idle slot
        return tok * torch.tensor(self.active, device=dev).view(B, 1)

    # ------------------------------------------------------------------ paged cache
    @property
    def pages_free(self) -> int:
        return self.pool.free_pages

    def pages_of(self, slot: int):
        """Page ids of a slot, in logical order (page i holds rows i page .. (i + 1) page - 1)."""
        return list(self._pages[slot])

    def _sync_table(self):
        """Host mirror -> the static device table (as _set_pos for the positions)."""
        rows = [ids + [-1] * (self.n_table - len(ids)) for ids in self._pages]
        self._table.copy_(torch.tensor(rows, dtype=torch.int32))

    def _dense_rows(self, slots, rows):
        """Eager reference: dense caches [len(slots), Hkv, Cl, hd] per layer holding
        the first rows[i] logical rows of slot slots[i] (zeros elsewhere)."""
        from ..ops import llm
        Cl = self.n_table * self.page
        out = []
        for kp, vp in self.cache:
            kc = kp.new_zeros(len(slots), kp.shape[1], Cl, kp.shape[3])
            vc = torch.zeros_like(kc)
            for i, (b, n) in enumerate(zip(slots, rows)):
                if n > 0:
                    kc[i, :, :n] = llm.paged_gather(kp, self._pages[b], n)
                    vc[i, :, :n] = llm.paged_gather(vp, self._pages[b], n)
            out.append((kc, vc))
        return out

    def _scatter_rows(self, dense, slots, starts, counts):
        """Eager reference: logical rows starts[i] .. starts[i] + counts[i] - 1 of the
        dense caches back into the pages of slot slots[i]."""
        for (kp, vp), (kc, vc) in zip(self.cache, dense):
            for i, (b, r0, n) in enumerate(zip(slots, starts, counts)):
                for r in range(r0, r0 + n):
                    pg, pr = self._pages[b][r // self.page], r % self.page
                    kp[pg, :, pr] = kc[i, :, r]
                    vp[pg, :, pr] = vc[i, :, r]

    def _forward_paged(self, tokens, pos, lens, head=True, last_idx=None, slot=None):
        """One ragged forward over the paged cache: every slot (pos / lens of B
        ints), or the batch of 1 that is `slot` (one int each).  fp8: the paged
        kernels on the device table (rows of `slot` alone: a [1, NP] view).
        Eager: gather, the dense reference path, scatter of the new rows (with
        kv_fp8 they were rounded through the codec where the path stored them, so
        the attention of the same forward saw what the pools now hold)."""
        slots = list(range(self.batch)) if slot is None else [slot]
        dev = tokens.device
        if self.fp8:
            self._sync_table()
            views = self._views(dev, pos, lens, self._table if slot is None else self._table[slot:slot + 1])
            return self.model.forward_fp8(tokens, self.cache, 0, last_only=True, tiled=self.prefill_tiled, head=head,
                                          last_idx=last_idx, views=views, tiled4=self.w4_tiled)
        dense = self._dense_rows(slots, [max(p, 0) for p in pos])
        if slot is None:
            logits = self.model(tokens, cache=dense, last_only=True, head=head, seq=(list(pos), list(lens)),
                                last_idx=last_idx, kv8=bool(self.kv_fp8))
        else:  # the uniform reference on the slot alone, as the dense decoder admits a request
            logits = self.model(tokens, cache=dense, pos=pos[0], fused=False, last_only=True, prefill_attn=True,
                                head=head, kv8=bool(self.kv_fp8))
        self._scatter_rows(dense, slots, pos, [n if p >= 0 else 0 for p, n in zip(pos, lens)])
        return logits

    def _prefill_paged(self, tokens: torch.Tensor, chunk, lens) -> torch.Tensor:
        B, S = tokens.shape
        lens = self._lens(tokens, lens, chunk)
        if chunk is not None:
            self._chunk(chunk)
        # every slot is reset: its pages go back first, and come back if the new prompts do not fit
        snap, held = self.pool.snapshot(), [list(ids) for ids in self._pages]
        try:
            for ids in self._pages:
                self.pool.free(ids)
            self._pages = [self.pool.alloc(-(-n // self.page)) for n in lens]
        except PoolExhausted:
            self.pool.restore(snap)
            self._pages = held
            raise
        dev = tokens.device
        self.pos_b, self.active = [-1] * B, [False] * B
        if chunk is None:  # one ragged launch per layer over the padded batch
            last = torch.tensor([max(n - 1, 0) for n in lens], device=dev)
            logits = self._forward_paged(tokens, [0 if n else -1 for n in lens], lens, last_idx=last)
        else:  # lens = [S] * B in pieces: every slot at c0, the head on the last piece
            for c0 in range(0, S, chunk):
                c1 = min(S, c0 + chunk)
                logits = self._forward_paged(tokens[:, c0:c1], [c0] * B, [c1 - c0] * B, head=(c1 == S))
        self.pos_b = [n if n else -1 for n in lens]
        self.active = [n > 0 for n in lens]
        self._sync_pos()
        tok = self._pick(logits, self.pos_b)  # the counter is the prompt length, -1 for an idle slot
        return tok * torch.tensor(self.active, device=dev).view(B, 1)

    def _admit_paged(self, slot: int, tokens: torch.Tensor, chunk: int, share):
        """Find the pages (shared prefix pages first) at the call; the chunks then
        run in the generator this returns."""
        S = tokens.shape[1]
        shared = []
        if share is not None:
            src, n = share
            if not isinstance(src, int) or isinstance(src, bool) or not 0 <= src < self.batch or src == slot \
                    or not self.active[src] or not isinstance(n, int) or n < 0:
                raise ValueError(f"LlamaDecoder: share={share!r} must be (an active slot other than {slot}, tokens)")
            # full pages only, and at least one token is left to prefill (its logits give the next token)
            k = min(min(n, self.pos_b[src]) // self.page, (S - 1) // self.page)
            shared = self._pages[src][:k]
        snap = self.pool.snapshot()
        try:
            self.pool.free(self._pages[slot])  # none, unless an earlier admit_iter of this slot was abandoned
            fresh = self.pool.alloc(-(-S // self.page) - len(shared))
        except PoolExhausted:
            self.pool.restore(snap)  # nothing has changed
            raise
        self._pages[slot] = self.pool.share(shared) + fresh
        return self._admit_chunks_paged(slot, tokens, chunk, len(shared) * self.page)

    def _admit_chunks_paged(self, slot: int, tokens: torch.Tensor, chunk: int, start: int):
        S = tokens.shape[1]
        logits = None
        for c0 in range(start, S, chunk):
            c1 = min(S, c0 + chunk)
            with torch.no_grad():
                logits = self._forward_paged(tokens[:, c0:c1], [c0], [c1 - c0], head=(c1 == S), slot=slot)
            yield c1
        self.pos_b[slot], self.active[slot] = S, True
        self._sync_pos()
        return self._pick(logits, [S], slot)

    def _grow_pages(self):
        """Before a decode step: a page for every active slot that starts one."""
        need = [b for b in range(self.batch) if self.active[b] and self.pos_b[b] == len(self._pages[b]) * self.page]
        if len(need) > self.pool.free_pages:
            raise PoolExhausted(f"LlamaDecoder: slots {need} start a new page, {self.pool.free_pages} of "
                                f"{self.pool.pages} pages free; release a slot and retry")
        for b in need:
            self._pages[b] += self.pool.alloc(1)

    @torch.no_grad()
    def admit(self, slot: int, tokens: torch.Tensor, chunk: Optional[int] = None, share=None) -> torch.Tensor:
        """Prefill one request (tokens [S] or [1, S]) into the idle slot `slot`
        while the other slots keep their state; returns its next token [1, 1].
        ``chunk`` / ``share``: as admit_iter, drained here."""
        n = tokens.shape[-1]
        return self._drain(self.admit_iter(slot, tokens, n if chunk is None else chunk, share=share))

    def admit_iter(self, slot: int, tokens: torch.Tensor, chunk: int, share=None):
        """admit() as a generator over chunks of at most `chunk` tokens (the
        uniform chunked prefill on the batch-1 views of the slot's caches): yields
        the prompt tokens done after each chunk, so a scheduled tenant gives every
        chunk a slice of its own and decode steps of the other slots may run in
        between; the slot stays idle until the last chunk is done.  The next
        token [1, 1] is the generator's return value.
        paged=True: the prompt's pages are found here, at the call (PoolExhausted
        if they are not there), and the chunks run the paged kernels on the
        slot's own table row.  ``share`` = (src, n) maps the first
        floor(min(n, pos_b[src]) / page) pages of the active slot src into this
        slot instead of storing them again (the caller asserts the two prompts
        agree on those tokens) and prefill starts after them."""
        if not self.ragged:
            raise ValueError("LlamaDecoder: admit needs ragged=True")
        if share is not None and not self.paged:
            raise ValueError("LlamaDecoder: share needs paged=True")
        if not isinstance(slot, int) or isinstance(slot, bool) or not 0 <= slot < self.batch:
            raise ValueError(f"LlamaDecoder: slot {slot!r} of a batch of {self.batch}")
        if self.active[slot]:
            raise ValueError(f"LlamaDecoder: slot {slot} is active (at position {self.pos_b[slot]}); release it first")
        self._chunk(chunk)
        tokens = tokens.view(1, -1)
        S = tokens.shape[1]
        if not 0 < S <= self.context:
            raise ValueError(f"LlamaDecoder: prompt of {S} tokens for a context of {self.context}")
        if self.paged:
            return self._admit_paged(slot, tokens, chunk, share)
        return self._admit_chunks(slot, tokens, chunk)

    def _admit_chunks(self, slot: int, tokens: torch.Tensor, chunk: int):
        # a dim-0 slice of a contiguous cache is contiguous: the uniform kernels run on it as a batch of 1
        view = [(k[slot:slot + 1], v[slot:slot + 1]) for k, v in self.cache]
        tok = yield from self._prefill_chunks(tokens, chunk, cache=view, slot=slot)
        self.pos_b[slot], self.active[slot] = tokens.shape[1], True
        self._sync_pos()
        return tok

    def release(self, slot: int):
        """Mark a slot idle (its request is done); the cache rows stay as they are.
        paged=True: its pages lose this slot's reference (contents not cleared)."""
        if not self.ragged:
            raise ValueError("LlamaDecoder: release needs ragged=True")
        if self.paged:
            self.pool.free(self._pages[slot])
            self._pages[slot] = []
        self.pos_b[slot], self.active[slot] = -1, False
        self._sync_pos()

    def prefill_iter(self, tokens: torch.Tensor, chunk: int):
        """Chunked prefill as a generator: runs tokens[:, c : c + chunk] at cache
        position c = 0, chunk, 2 chunk, ... and yields the number of prompt
        tokens done after each chunk, so a scheduled tenant can give every
        chunk a slice of its own.  Only the last chunk computes logits; the next
        token [B, 1] is the generator's return value (StopIteration.value)."""
        if not self.prefill_attn:
            raise ValueError("LlamaDecoder: chunked prefill needs prefill_attn=True (SDPA's is_causal mask is "
                             "top-left aligned, wrong for a chunk at pos > 0)")
        self._chunk(chunk)
        S = tokens.shape[1]
        if not 0 < S <= self.context:
            raise ValueError(f"LlamaDecoder: prompt of {S} tokens for a context of {self.context}")
        return self._prefill_chunks(tokens, chunk)

    def _prefill_chunks(self, tokens: torch.Tensor, chunk: int, cache=None, slot=None):
        """``cache``: the batch-1 views of one slot, ``slot`` (admit_iter); the
        decoder's own caches, and with them every slot, otherwise."""
        S = tokens.shape[1]
        self.pos, logits = 0, None
        for c0 in range(0, S, chunk):
            c1 = min(S, c0 + chunk)
            with torch.no_grad():
                logits = self._forward(tokens[:, c0:c1], c0, head=(c1 == S), cache=cache)
            self.pos = c1
            yield c1
        if cache is None:
            self._all_slots_at(S)
        return self._pick(logits, [S] * tokens.shape[0], slot)

    def _graph_setup(self, tok: torch.Tensor):
        """Build the static-shape step; with graph=True capture it (every launch
        of it) into a HIP graph, so later steps are one graph launch plus the
        position/token uploads."""
        dev = tok.device
        self._tok = tok.clone()
        if self.sampling:  # the counters of the step's picks, refreshed with the positions before every step
            self._ctr = torch.full((self.batch,), -1, dtype=torch.int32, device=dev)

        def pick(logits):
            if not self.sampling:
                return logits[:, -1].argmax(-1, keepdim=True)
            self._step_logits = logits[:, -1]  # under capture: the static output tensor every replay rewrites
            return self._sample(self._step_logits, self._ctr)

        if self.ragged:  # one device position per sequence, refreshed from pos_b before every step
            self._pos_seq = torch.full((self.batch,), -1, dtype=torch.int32, device=dev)
            # built once: every step, and the captured graph, reads these position, table and cache tensors
            views = self._layer_views(self._pos_seq, table=self._table if self.paged else None)

            def step():
                return pick(self.model.decode_fp8_static(self._tok, self.cache, views=views))
        else:
            self._pos_i32 = torch.zeros(1, dtype=torch.int32, device=dev)
            self._pos_i64 = torch.zeros(1, dtype=torch.int64, device=dev)
            self._ar = torch.arange(self.context, device=dev)

            def step():
                mask = torch.where(self._ar <= self._pos_i64, 0.0, float("-inf"))
                logits = self.model.decode_fp8_static(self._tok, self.cache, self._pos_i32, self._pos_i64, mask)
                return pick(logits)

        self._step = step
        if not self.graph:
            return
        self._set_pos()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):  # warm the allocator / library handles outside capture
                step()
        torch.cuda.current_stream(dev).wait_stream(side)
        self._g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g):
            self._out = step()

    def _set_pos(self):
        if self.sampling:  # the token picked at position p has index p + 1 in its sequence
            self._ctr.copy_(torch.tensor([p + 1 if a else -1 for p, a in zip(self.pos_b, self.active)]
                                         if self.ragged else [self.pos + 1] * self.batch, dtype=torch.int32))
        if self.ragged:
            self._pos_seq.copy_(torch.tensor(self.pos_b, dtype=torch.int32))
            if self.paged:  # the captured graph reads the same table tensor: admission, release, growth survive
                self._sync_table()
            return
        self._pos_i32.fill_(self.pos)
        self._pos_i64.fill_(self.pos)

    def _static_step(self, tok: torch.Tensor) -> torch.Tensor:
        """The static-shape step at the decoder's positions: the token and the
        positions go into their static tensors, then the graph's replay or the
        step itself."""
        if self._step is None:
            self._graph_setup(tok)
        self._tok.copy_(tok)
        self._set_pos()
        if self.graph:
            self._g.replay()
            out = self._out.clone()
        else:
            out = self._step()
        if self.sampling:
            self.last_logits = self._step_logits
        return out

    def _decode_step_ragged(self, tok: torch.Tensor) -> torch.Tensor:
        for b in range(self.batch):
            if self.active[b] and self.pos_b[b] >= self.context:
                raise ValueError(f"LlamaDecoder: slot {b} is at position {self.pos_b[b]} = context; release it (ragged "
                                 f"mode has no sliding window)")
        if self.paged:
            self._grow_pages()  # before any launch; PoolExhausted leaves everything as it was
        if self.fp8:
            out = self._static_step(tok)
        elif self.paged:
            logits = self._forward_paged(tok, list(self.pos_b), [int(a) for a in self.active])
            out = self._pick(logits, [p + 1 if a else -1 for p, a in zip(self.pos_b, self.active)])
        else:
            logits = self._forward(tok, 0, seq=(list(self.pos_b), [int(a) for a in self.active]))
            out = self._pick(logits, [p + 1 if a else -1 for p, a in zip(self.pos_b, self.active)])
        self.pos_b = [p + 1 if a else -1 for p, a in zip(self.pos_b, self.active)]
        self._sync_pos()
        return out

    @torch.no_grad()
    def decode_step(self, tok: torch.Tensor) -> torch.Tensor:
        if self.ragged:  # advances the active slots; idle rows return a token to ignore and write nothing
            return self._decode_step_ragged(tok)
        if self.pos >= self.context:
            self.pos = self.context // 2  # slide: keep the cache bounded for long runs
        if self.static:
            out = self._static_step(tok)
            self.pos += 1
            return out
        if self.fp8:
            logits = self.model.forward_fp8(tok, self.cache, self.pos, tiled4=self.w4_tiled)
        else:
            logits = self.model(tok, cache=self.cache, pos=self.pos, fused=self.fused)
        self.pos += 1
        return self._pick(logits, [self.pos] * tok.shape[0])


class LlamaTrainer:
    """Training tenant: next-token loss, backward, fused AdamW (fp32 state)."""

    def __init__(self, cfg: LlamaConfig, batch: int, seq: int, device="cuda", dtype=torch.bfloat16, lr=1e-4):
        self.cfg, self.batch, self.seq = cfg, batch, seq
        self.model = build(cfg, device, dtype)
        self.model.train()
        kw = {"fused": True} if str(device).startswith("cuda") else {}
        self.opt = torch.optim.AdamW(self.model.parameters(), lr=lr, weight_decay=0.1, **kw)
        g = torch.Generator(device=device).manual_seed(1)
        self.tokens = torch.randint(0, cfg.vocab, (batch, seq + 1), device=device, generator=g)

    def step(self) -> torch.Tensor:
        x, y = self.tokens[:, :-1], self.tokens[:, 1:]
        logits = self.model(x)
        loss = F.cross_entropy(logits.float().reshape(-1, self.cfg.vocab), y.reshape(-1))
        loss.backward()
        self.opt.step()
        self.opt.zero_grad(set_to_none=True)
        return loss.detach()

    def tokens_per_step(self) -> int:
        return self.batch * self.seq

    def flops_per_step(self) -> float:
        return 6.0 * self.cfg.n_params() * self.tokens_per_step()
