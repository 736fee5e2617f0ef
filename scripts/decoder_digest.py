"""SHA-256 digests of what LlamaDecoder computes in every mode, for comparing two trees bit for bit: run it on
each and compare the one JSON line it prints.  Only the public decoder API and the sixteen attention wrappers of
pbs_amd.ops.llm are used, so the script runs unmodified on older trees.

The model is the dim-512 one of the decoder tests, weights from the decoder's own seeded init.  A ragged mode runs
prefill(lens=[150, 37, 0, 64]), 3 decode steps, admit(2) in chunks of 32, 3 steps, release(1), admit(1) of a prompt
that shares 140 tokens with slot 0 (share=(0, 140) where the cache is paged), 2 steps; a uniform mode a full
prefill and 8 steps.  Per mode the digests of the tokens of the active slots after every call and of every layer's
cache tensors at the end, and the same two of a twin decoder of the same mode with sampling=True and every slot
greedy, which also gives the last-token logits of every pick (last_logits).  On the GPU the twin's tokens must
equal the first's; on the CPU the first runs in fp64 and the twin, for the reference sampler, in fp32.

    python scripts/decoder_digest.py --device cpu    # fp64 eager: uniform, ragged, paged, paged + kv_fp8
    python scripts/decoder_digest.py --device cuda   # the fp8 kernels: every mode, and the wrappers on their own
"""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pbs_amd.models.llama import LlamaConfig, LlamaDecoder  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)
BATCH, CONTEXT, LENS, STEPS = 4, 200, [150, 37, 0, 64], 8

CPU_MODES = {"eager": {}, "eager-ragged": {"ragged": True}, "eager-paged": {"paged": True, "pages": 10},
             "eager-paged-kv8": {"paged": True, "pages": 10, "kv_fp8": True}}
GPU_MODES = {"fp8": {}, "fp8-prefill-attn": {"prefill_attn": True, "chunk": 64}, "static": {"static": True},
             "graph": {"graph": True}, "ragged": {"ragged": True}, "ragged-graph": {"ragged": True, "graph": True},
             "paged-64": {"paged": True, "pages": 10, "page": 64},
             "paged-256": {"paged": True, "pages": 4, "page": 256},
             "kv8": {"paged": True, "pages": 10, "kv_fp8": True},
             "kv8-graph": {"paged": True, "pages": 10, "kv_fp8": True, "graph": True},
             "kv8-emulate": {"paged": True, "pages": 10, "kv_fp8": "emulate"},
             "sampling": {"ragged": True, "graph": True, "sampling": True}}


class Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, t: torch.Tensor):
        t = t.detach().cpu().contiguous()
        self.h.update(repr((str(t.dtype), tuple(t.shape))).encode())
        self.h.update(t.view(torch.uint8).numpy().tobytes())

    def hex(self):
        return self.h.hexdigest()


def prompts(dev):
    g = torch.Generator().manual_seed(5)
    full = torch.randint(0, CFG.vocab, (BATCH, 150), generator=g)
    new = torch.randint(0, CFG.vocab, (50,), generator=g)
    shared = torch.cat([full[0, :140], torch.randint(0, CFG.vocab, (20,), generator=g)])
    return full.to(dev), new.to(dev), shared.to(dev)


def run(dev, kw, sampling):
    """One decoder through the scenario; returns (tokens of the active rows per call, logits of them, the caches)."""
    kw = dict(kw)
    chunk = kw.pop("chunk", None)
    drawn = kw.pop("sampling", False)
    if dev == "cpu":
        # the reference sampler takes bf16 / fp32 logits: the twin of an fp64 mode runs in fp32
        d = LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, device="cpu", fused=False, sampling=sampling,
                         dtype=torch.float32 if sampling else torch.float64, **kw)
    else:
        d = LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, fp8=True, sampling=sampling, **kw)
    if drawn:
        d.set_sampling(temperature=0.8, top_k=50, top_p=0.9, seed=3)
    full, new, shared = prompts(dev)
    toks, logits = [], []

    def keep(tok, rows):
        toks.append(tok[rows].clone())
        if sampling:
            logits.append(d.last_logits[rows if d.last_logits.shape[0] == BATCH else slice(None)].clone())

    def steps(tok, n):
        for _ in range(n):
            rows = torch.tensor(d.active if d.ragged else [True] * BATCH, device=tok.device)
            tok = d.decode_step(tok * rows.view(-1, 1))  # an idle row returns a token to ignore: feed it 0
            keep(tok, rows)
        return tok

    if not d.ragged:
        tok = d.prefill(full, chunk=chunk)
        keep(tok, slice(None))
        steps(tok, STEPS)
        return toks, logits, d.cache
    tok = d.prefill(full, lens=LENS)
    keep(tok, torch.tensor([n > 0 for n in LENS], device=tok.device))
    tok = steps(tok, 3)
    tok[2] = d.admit(2, new, chunk=32)[0]
    keep(tok[2:3], slice(None))
    tok = steps(tok, 3)
    d.release(1)
    tok[1] = d.admit(1, shared, **({"share": (0, 140)} if d.paged else {}))[0]
    keep(tok[1:2], slice(None))
    steps(tok, 2)
    return toks, logits, d.cache


def decoder_digests(dev, modes, out):
    for name, kw in modes.items():
        toks, _, cache = run(dev, kw, kw.get("sampling", False))
        twin, logits, cache2 = run(dev, kw, True)
        if dev != "cpu" and not kw.get("sampling"):  # a greedy sampler picks the argmax of the same logits
            assert all(torch.equal(a, b) for a, b in zip(toks, twin)), f"{name}: the greedy twin chose other tokens"
        for what, tensors in (("tokens", toks), ("cache", [t for layer in cache for t in layer]),
                              ("twin-tokens", twin), ("twin-logits", logits),
                              ("twin-cache", [t for layer in cache2 for t in layer])):
            dg = Digest()
            for t in tensors:
                dg.add(t)
            out[f"{name}:{what}"] = dg.hex()


def wrapper_digests(out):
    """The sixteen wrappers on seeded tensors: B 4, H 4, Hkv 1, 256 cache rows, S 37; per wrapper the result and,
    for a write, the cache tensors after it."""
    B, H, Hkv, hd, Cn, S, page, P = 4, 4, 1, 128, 256, 37, 64, 20
    g = torch.Generator().manual_seed(11)

    def rnd(*shape):
        return torch.randn(*shape, generator=g).bfloat16().cuda()

    f = torch.outer(torch.arange(Cn, dtype=torch.float64), 1.0 / (500000.0 ** (torch.arange(0, hd, 2) / hd)))
    cos, sin = f.cos().float().cuda(), f.sin().float().cuda()
    i32 = dict(dtype=torch.int32, device="cuda")
    pos1, pos_t, len_t = torch.tensor([100], **i32), torch.tensor([150, 37, -1, 64], **i32), \
        torch.tensor([37, 20, 5, 0], **i32)
    table = torch.randperm(P, generator=g)[:B * (Cn // page)].view(B, Cn // page).to(**i32)
    qkv1, qkvS, q1, qS = rnd(B, 1, (H + 2 * Hkv) * hd), rnd(B, S, (H + 2 * Hkv) * hd), rnd(B, H, hd), rnd(B, S, H, hd)
    dense = (rnd(B, Hkv, Cn, hd), rnd(B, Hkv, Cn, hd))
    pools = (rnd(P, Hkv, page, hd), rnd(P, Hkv, page, hd))
    (k8, ks), (v8, vs) = llm.kv8_quant_ref(pools[0]), llm.kv8_quant_ref(pools[1])
    calls = {
        "qkv_rope_cache": lambda c: llm.qkv_rope_cache(qkv1, cos, sin, pos1, *c, H),
        "decode_attn": lambda c: llm.decode_attn(q1, *c, pos1),
        "qkv_rope_cache_prefill": lambda c: llm.qkv_rope_cache_prefill(qkvS, cos, sin, 100, *c, H),
        "prefill_attn": lambda c: llm.prefill_attn(qS, *c, 100),
        "qkv_rope_cache_seq": lambda c: llm.qkv_rope_cache_seq(qkv1, cos, sin, pos_t, *c, H),
        "decode_attn_seq": lambda c: llm.decode_attn_seq(q1, *c, pos_t),
        "qkv_rope_cache_prefill_seq": lambda c: llm.qkv_rope_cache_prefill_seq(qkvS, cos, sin, pos_t, len_t, *c, H),
        "prefill_attn_seq": lambda c: llm.prefill_attn_seq(qS, *c, pos_t, len_t),
        "qkv_rope_cache_paged": lambda c: llm.qkv_rope_cache_paged(qkv1, cos, sin, pos_t, table, *c, H),
        "decode_attn_paged": lambda c: llm.decode_attn_paged(q1, *c, table, pos_t),
        "qkv_rope_cache_prefill_paged": lambda c: llm.qkv_rope_cache_prefill_paged(qkvS, cos, sin, pos_t, len_t, table,
                                                                                  *c, H),
        "prefill_attn_paged": lambda c: llm.prefill_attn_paged(qS, *c, table, pos_t, len_t),
        "qkv_rope_cache_paged_kv8": lambda c: llm.qkv_rope_cache_paged_kv8(qkv1, cos, sin, pos_t, table, *c, H),
        "decode_attn_paged_kv8": lambda c: llm.decode_attn_paged_kv8(q1, *c, table, pos_t),
        "qkv_rope_cache_prefill_paged_kv8": lambda c: llm.qkv_rope_cache_prefill_paged_kv8(qkvS, cos, sin, pos_t, len_t,
                                                                                          table, *c, H),
        "prefill_attn_paged_kv8": lambda c: llm.prefill_attn_paged_kv8(qS, *c, table, pos_t, len_t),
    }
    for name, fn in calls.items():
        src = (k8, v8, ks, vs) if name.endswith("kv8") else pools if "paged" in name else dense
        cache = tuple(t.clone() for t in src)
        dg = Digest()
        dg.add(fn(cache))
        for t in cache:
            dg.add(t)
        out[f"wrapper:{name}"] = dg.hex()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", choices=("cpu", "cuda"), required=True)
    a = ap.parse_args()
    out = {}
    with torch.no_grad():
        decoder_digests(a.device, CPU_MODES if a.device == "cpu" else GPU_MODES, out)
        if a.device == "cuda":
            wrapper_digests(out)
    print(json.dumps({"device": a.device, "digests": len(out), **out}))


if __name__ == "__main__":
    main()
