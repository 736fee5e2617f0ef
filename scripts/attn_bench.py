"""Prefill attention microbench: the gfx950 MFMA kernel (llm.prefill_attn)
against F.scaled_dot_product_attention(enable_gqa=True) on the same tensors,
with the transposes SDPA needs counted (the model pays for them), on the
Llama-3-8B head geometry (H 32, Hkv 8, head_dim 128); then a whole llama3-8b fp8
prefill (batch 8, 1024-token prompt) with and without prefill_attn, unchunked
and in chunks of 256 (and the same on the bf16 weights), with the cosine of the
last-token logits against the SDPA run.  Rounds alternate the variants in one process; a row
reports the median of 5 rounds with min / max.

    python scripts/attn_bench.py [--iters 100] [--out prefill_attn.jsonl] [--skip-model]

--ragged runs instead the per-sequence kernels against their uniform twins (B 8,
C 8192): decode_attn_seq with every length 8192 against decode_attn at 8192,
where decode_attn is timed twice per round so the rows carry the spread of the
uniform kernel against itself; decode_attn_seq with lengths spread over
1024..8192; prefill_attn_seq with lengths 1024, 512, 256, 64 (twice) against
prefill_attn at S 1024.

    python scripts/attn_bench.py --ragged [--iters 100] [--out profiles/ragged_attn.jsonl]

--paged runs instead the block-table kernels against their per-sequence twins at
the same shapes (B 8, 8192 rows per sequence): the dense cache is scattered into
pools of 64-, 128- and 256-row pages, once under the identity table (page i of
sequence b is pool page b NP + i, the dense layout) and once under a shuffled
one; decode_attn_paged against decode_attn_seq with every length 8192 and with
lengths 1024..8192, prefill_attn_paged against prefill_attn_seq at S 1024.  The
_seq twin is timed in the same rounds, twice, so the rows carry its spread
against itself.

    python scripts/attn_bench.py --paged [--iters 100] [--out profiles/paged_attn.jsonl]

--kv8 runs instead the fp8-cache kernels against their bf16 _paged twins, with the
--paged rows' method (B 8, 8192 rows per sequence, pages of 64 / 128 / 256 rows,
identity and shuffled tables, lengths all 8192 and 1024..8192, prefill at S 1024):
the bf16 pools are quantised with llm.kv8_quant_ref, the twin runs on the
dequantised pools, and every kv8 result is checked against its twin bit for bit
before anything is timed.  Within each of the 5 rounds the twin is timed, then the
kv8 kernel, then the twin again, so the rows carry the twin's spread against
itself; ratios are per round.

    python scripts/attn_bench.py --kv8 [--iters 100] [--out profiles/kv8_attn.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pbs_amd.models.llama import PRESETS, LlamaDecoder  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

H, HKV, HD = 32, 8, 128
ROUNDS = 5


def timeit(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def med(ts):
    return sorted(ts)[len(ts) // 2]


def flops(B, S, pos):
    return 4.0 * B * H * HD * S * (pos + (S + 1) / 2)


def kernel_row(emit, g, iters, B, S, pos, C, name, sdpa=True):
    q = torch.randn(B, S, H, HD, device="cuda", generator=g).bfloat16()
    kc = torch.randn(B, HKV, C, HD, device="cuda", generator=g).bfloat16()
    vc = torch.randn(B, HKV, C, HD, device="cuda", generator=g).bfloat16()
    L = pos + S
    # is_causal is top-left aligned: only right for pos == 0; a chunk needs the explicit mask
    mask = None if pos == 0 else \
        (torch.arange(L, device="cuda")[None, :] <= pos + torch.arange(S, device="cuda")[:, None])

    def ours():
        return llm.prefill_attn(q, kc, vc, pos)

    def theirs():
        o = F.scaled_dot_product_attention(q.transpose(1, 2), kc[:, :, :L], vc[:, :, :L], attn_mask=mask,
                                           is_causal=mask is None, enable_gqa=True)
        return o.transpose(1, 2).reshape(B, S, H * HD)

    err = None
    if sdpa:
        try:
            theirs()
        except Exception as e:  # recorded in the row: the comparison is then missing, not the kernel's time
            sdpa, err = False, f"{type(e).__name__}: {e}"[:200]
    to, ts = [], []
    for _ in range(ROUNDS):
        to.append(timeit(ours, iters))
        if sdpa:
            ts.append(timeit(theirs, iters))
    rec = {"bench": "prefill_attn", "name": name, "B": B, "S": S, "pos": pos, "C": C, "H": H, "Hkv": HKV,
           "kernel_us": round(med(to), 1), "kernel_us_minmax": [round(min(to), 1), round(max(to), 1)],
           "kernel_TFs": round(flops(B, S, pos) / med(to) / 1e6, 1)}
    if sdpa:
        a, b = ours().float(), theirs().float()
        rec.update({"sdpa_us": round(med(ts), 1), "sdpa_us_minmax": [round(min(ts), 1), round(max(ts), 1)],
                    "sdpa_TFs": round(flops(B, S, pos) / med(ts) / 1e6, 1),
                    "sdpa_mask": "is_causal" if mask is None else "explicit",
                    "speedup_vs_sdpa": round(med(ts) / med(to), 3),
                    "max_abs_diff": (a - b).abs().max().item(), "max_abs": b.abs().max().item()})
    if err:
        rec["sdpa_error"] = err
    emit(rec)
    return med(to)


def model_rows(emit, batch, prompt, rounds):
    cfg = PRESETS["llama3-8b"]
    torch.manual_seed(0)
    dec = LlamaDecoder(cfg, batch=batch, context=2 * prompt, device="cuda", fp8=True)
    toks = torch.randint(0, cfg.vocab, (batch, prompt), device="cuda")
    variants = [("sdpa", False, None), ("prefill_attn", True, None), ("prefill_attn+chunk256", True, 256)]
    logits = {}
    fwd = dec._forward

    def spy(*a, **k):
        r = fwd(*a, **k)
        if r is not None:
            logits[spy.key] = r[:, -1].float().clone()
        return r

    dec._forward = spy
    kept = {}

    def cos(a, b):
        c = F.cosine_similarity(a, b, dim=-1)
        return c.min().item(), c.mean().item()

    for weights, tiled in (("fp8", False), ("fp8", True), ("bf16", False)):
        dec.fp8, dec.prefill_tiled = weights == "fp8", tiled
        times = {v[0]: [] for v in variants}
        for r in range(rounds + 1):  # round 0 warms every variant
            for key, pa, chunk in variants:
                dec.prefill_attn, spy.key = pa, key
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                dec.prefill(toks, chunk=chunk)
                torch.cuda.synchronize()
                if r:
                    times[key].append((time.perf_counter() - t1) * 1e3)
        for key, _, _ in variants:
            ts = times[key]
            kept[(weights, tiled, key)] = logits[key]
            cmin, cmean = cos(logits[key], logits["sdpa"])
            emit({"bench": "llama3-8b-prefill", "weights": weights, "prefill_tiled": tiled, "attention": key,
                  "batch": batch, "prompt": prompt, "ms": round(med(ts), 2),
                  "ms_minmax": [round(min(ts), 2), round(max(ts), 2)],
                  "tok_per_s": round(batch * prompt / med(ts) * 1e3),
                  "speedup_vs_sdpa": round(med(times["sdpa"]) / med(ts), 3),
                  "min_cos_logits_vs_sdpa": cmin, "mean_cos_logits_vs_sdpa": cmean})
    # how far two stock paths of the same fp8 model are from each other: the
    # yardstick for the cosines above (random weights, 32 layers of fp8 rounding)
    cmin, cmean = cos(kept[("fp8", False, "sdpa")], kept[("fp8", True, "sdpa")])
    emit({"bench": "llama3-8b-prefill-sensitivity", "what": "fp8 sdpa, sliced vs tiled linears (no new code)",
          "min_cos_logits": cmin, "mean_cos_logits": cmean})
    cmin, cmean = cos(kept[("fp8", False, "sdpa")], kept[("bf16", False, "sdpa")])
    emit({"bench": "llama3-8b-prefill-sensitivity", "what": "sdpa, fp8 vs bf16 weights (no new code)",
          "min_cos_logits": cmin, "mean_cos_logits": cmean})


def ragged_rows(emit, g, iters, B=8, C=8192):
    i32 = dict(dtype=torch.int32, device="cuda")
    q = torch.randn(B, H, HD, device="cuda", generator=g).bfloat16()
    kc = torch.randn(B, HKV, C, HD, device="cuda", generator=g).bfloat16()
    vc = torch.randn(B, HKV, C, HD, device="cuda", generator=g).bfloat16()
    pos1 = torch.tensor([C - 1], **i32)
    full = torch.full((B,), C - 1, **i32)
    spread_l = [1024 + (C - 1024) * b // (B - 1) for b in range(B)]
    spread = torch.tensor([n - 1 for n in spread_l], **i32)
    S = 1024
    qp = torch.randn(B, S, H, HD, device="cuda", generator=g).bfloat16()
    lens_l = [1024, 512, 256, 64] * (B // 4)
    zeros, lens, all_s = torch.zeros(B, **i32), torch.tensor(lens_l, **i32), torch.full((B,), S, **i32)
    variants = {
        "decode_attn@8192 (first)": lambda: llm.decode_attn(q, kc, vc, pos1),
        "decode_attn_seq all 8192": lambda: llm.decode_attn_seq(q, kc, vc, full),
        "decode_attn@8192 (second)": lambda: llm.decode_attn(q, kc, vc, pos1),
        "decode_attn_seq 1024..8192": lambda: llm.decode_attn_seq(q, kc, vc, spread),
        "prefill_attn S 1024": lambda: llm.prefill_attn(qp, kc, vc, 0),
        "prefill_attn_seq all 1024": lambda: llm.prefill_attn_seq(qp, kc, vc, zeros, all_s),
        "prefill_attn_seq 1024/512/256/64": lambda: llm.prefill_attn_seq(qp, kc, vc, zeros, lens),
    }
    assert torch.equal(variants["decode_attn_seq all 8192"](), variants["decode_attn@8192 (first)"]())
    assert torch.equal(variants["prefill_attn_seq all 1024"](), variants["prefill_attn S 1024"]())
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):  # the variants alternate within a round
        for k, fn in variants.items():
            times[k].append(timeit(fn, iters))
    m = {k: med(v) for k, v in times.items()}
    base = {"decode_attn@8192 (second)": "decode_attn@8192 (first)",
            "decode_attn_seq all 8192": "decode_attn@8192 (first)",
            "decode_attn_seq 1024..8192": "decode_attn_seq all 8192",
            "prefill_attn_seq all 1024": "prefill_attn S 1024",
            "prefill_attn_seq 1024/512/256/64": "prefill_attn S 1024"}
    info = {"decode_attn_seq 1024..8192": {"lengths": spread_l, "keys_over_full": round(sum(spread_l) / (B * C), 3)},
            "prefill_attn_seq 1024/512/256/64": {
                "lengths": lens_l,
                "work_over_full": round(sum(n * (n + 1) for n in lens_l) / (B * S * (S + 1)), 3)}}
    for k in variants:
        rec = {"bench": "ragged_attn", "name": k, "B": B, "C": C, "H": H, "Hkv": HKV, "us": round(m[k], 1),
               "us_minmax": [round(min(times[k]), 1), round(max(times[k]), 1)]}
        if k in base:
            rec.update({"over": base[k], "ratio": round(m[k] / m[base[k]], 3)})
        rec.update(info.get(k, {}))
        emit(rec)


def paged_rows(emit, g, iters, B=8, C=8192, pages=(64, 128, 256)):
    i32 = dict(dtype=torch.int32, device="cuda")
    q = torch.randn(B, H, HD, device="cuda", generator=g).bfloat16()
    kc = torch.randn(B, HKV, C, HD, device="cuda", generator=g).bfloat16()
    vc = torch.randn(B, HKV, C, HD, device="cuda", generator=g).bfloat16()
    full = torch.full((B,), C - 1, **i32)
    spread_l = [1024 + (C - 1024) * b // (B - 1) for b in range(B)]
    spread = torch.tensor([n - 1 for n in spread_l], **i32)
    S = 1024
    qp = torch.randn(B, S, H, HD, device="cuda", generator=g).bfloat16()
    zeros, all_s = torch.zeros(B, **i32), torch.full((B,), S, **i32)
    variants = {
        "decode_attn_seq all 8192 (first)": lambda: llm.decode_attn_seq(q, kc, vc, full),
        "decode_attn_seq 1024..8192": lambda: llm.decode_attn_seq(q, kc, vc, spread),
        "prefill_attn_seq all 1024 (first)": lambda: llm.prefill_attn_seq(qp, kc, vc, zeros, all_s),
    }
    base, info = {}, {}
    for page in pages:
        NP = C // page
        for kind in ("identity", "shuffled"):
            ids = torch.arange(B * NP, device="cuda")
            if kind == "shuffled":
                ids = ids[torch.randperm(B * NP, device="cuda", generator=g)]
            table = ids.view(B, NP).to(torch.int32).contiguous()
            # pool page table[b, i] holds rows i page .. (i + 1) page - 1 of sequence b
            kp, vp = (torch.empty(B * NP, HKV, page, HD, device="cuda", dtype=torch.bfloat16) for _ in range(2))
            for pool, dense in ((kp, kc), (vp, vc)):
                pool[ids] = dense.view(B, HKV, NP, page, HD).permute(0, 2, 1, 3, 4).reshape(B * NP, HKV, page, HD)
            tag = f"page {page} {kind}"
            for name, over, fn in (
                    (f"decode_attn_paged all 8192, {tag}", "decode_attn_seq all 8192 (first)",
                     lambda kp=kp, vp=vp, table=table: llm.decode_attn_paged(q, kp, vp, table, full)),
                    (f"decode_attn_paged 1024..8192, {tag}", "decode_attn_seq 1024..8192",
                     lambda kp=kp, vp=vp, table=table: llm.decode_attn_paged(q, kp, vp, table, spread)),
                    (f"prefill_attn_paged all 1024, {tag}", "prefill_attn_seq all 1024 (first)",
                     lambda kp=kp, vp=vp, table=table: llm.prefill_attn_paged(qp, kp, vp, table, zeros, all_s))):
                variants[name], base[name] = fn, over
                info[name] = {"page": page, "table": kind}
                assert torch.equal(fn(), variants[over]()), name  # bit for bit before anything is timed
    variants["decode_attn_seq all 8192 (second)"] = variants["decode_attn_seq all 8192 (first)"]
    variants["prefill_attn_seq all 1024 (second)"] = variants["prefill_attn_seq all 1024 (first)"]
    base["decode_attn_seq all 8192 (second)"] = "decode_attn_seq all 8192 (first)"
    base["prefill_attn_seq all 1024 (second)"] = "prefill_attn_seq all 1024 (first)"
    times = {k: [] for k in variants}
    for _ in range(ROUNDS):  # the variants alternate within a round
        for k, fn in variants.items():
            times[k].append(timeit(fn, iters))
    m = {k: med(v) for k, v in times.items()}
    for k in variants:
        rec = {"bench": "paged_attn", "name": k, "B": B, "rows": C, "H": H, "Hkv": HKV, "us": round(m[k], 1),
               "us_minmax": [round(min(times[k]), 1), round(max(times[k]), 1)]}
        if k in base:
            r = [t / u for t, u in zip(times[k], times[base[k]])]  # per round: both timed within the same round
            rec.update({"over": base[k], "ratio": round(med(r), 3),
                        "ratio_minmax": [round(min(r), 3), round(max(r), 3)]})
        rec.update(info.get(k, {}))
        emit(rec)


def kv8_rows(emit, g, iters, B=8, C=8192, pages=(64, 128, 256)):
    i32 = dict(dtype=torch.int32, device="cuda")
    q = torch.randn(B, H, HD, device="cuda", generator=g).bfloat16()
    kc = torch.randn(B, HKV, C, HD, device="cuda", generator=g).bfloat16()
    vc = torch.randn(B, HKV, C, HD, device="cuda", generator=g).bfloat16()
    full = torch.full((B,), C - 1, **i32)
    spread_l = [1024 + (C - 1024) * b // (B - 1) for b in range(B)]
    spread = torch.tensor([n - 1 for n in spread_l], **i32)
    S = 1024
    qp = torch.randn(B, S, H, HD, device="cuda", generator=g).bfloat16()
    zeros, all_s = torch.zeros(B, **i32), torch.full((B,), S, **i32)
    for page in pages:
        NP = C // page
        for kind in ("identity", "shuffled"):
            ids = torch.arange(B * NP, device="cuda")
            if kind == "shuffled":
                ids = ids[torch.randperm(B * NP, device="cuda", generator=g)]
            table = ids.view(B, NP).to(torch.int32).contiguous()
            four, twin = [None] * 4, []
            for i, dense in enumerate((kc, vc)):
                pool = torch.empty(B * NP, HKV, page, HD, device="cuda", dtype=torch.bfloat16)
                pool[ids] = dense.view(B, HKV, NP, page, HD).permute(0, 2, 1, 3, 4).reshape(B * NP, HKV, page, HD)
                four[i], four[2 + i] = llm.kv8_quant_ref(pool)
                twin.append(llm.kv8_dequant(four[i], four[2 + i]))
                del pool
            k8, v8, ks, vs = four
            kt, vt = twin
            shapes = (
                ("decode all 8192", lambda: llm.decode_attn_paged(q, kt, vt, table, full),
                 lambda: llm.decode_attn_paged_kv8(q, k8, v8, ks, vs, table, full), None),
                ("decode 1024..8192", lambda: llm.decode_attn_paged(q, kt, vt, table, spread),
                 lambda: llm.decode_attn_paged_kv8(q, k8, v8, ks, vs, table, spread), {"lengths": spread_l}),
                ("prefill all 1024", lambda: llm.prefill_attn_paged(qp, kt, vt, table, zeros, all_s),
                 lambda: llm.prefill_attn_paged_kv8(qp, k8, v8, ks, vs, table, zeros, all_s), None))
            for shape, twin_fn, kv8_fn, extra in shapes:
                assert torch.equal(kv8_fn(), twin_fn()), (shape, page, kind)  # bit for bit before anything is timed
                t = {"twin (first)": [], "kv8": [], "twin (second)": []}
                for _ in range(ROUNDS):  # the three alternate within a round
                    t["twin (first)"].append(timeit(twin_fn, iters))
                    t["kv8"].append(timeit(kv8_fn, iters))
                    t["twin (second)"].append(timeit(twin_fn, iters))
                for k, v in t.items():
                    kernel = ("prefill_attn_paged" if shape.startswith("prefill") else "decode_attn_paged") \
                        + ("_kv8" if k == "kv8" else "")
                    rec = {"bench": "kv8_attn", "name": f"{kernel} {shape.split(' ', 1)[1]}, page {page} {kind}"
                           + ("" if k == "kv8" else f" {k[5:]}"), "kernel": kernel, "page": page, "table": kind,
                           "B": B, "rows": C, "H": H, "Hkv": HKV, "bit_equal_to_twin": True,
                           "us": round(med(v), 1), "us_minmax": [round(min(v), 1), round(max(v), 1)]}
                    if k != "twin (first)":
                        r = [a / b for a, b in zip(v, t["twin (first)"])]
                        rec.update({"over": "twin (first)", "ratio": round(med(r), 3),
                                    "ratio_minmax": [round(min(r), 3), round(max(r), 3)],
                                    "ratio_rounds": [round(x, 3) for x in r]})
                    rec.update(extra or {})
                    emit(rec)
            del four, twin, k8, v8, ks, vs, kt, vt
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--ragged", action="store_true", help="only the per-sequence kernels against their uniform twins")
    ap.add_argument("--paged", action="store_true", help="only the block-table kernels against their _seq twins")
    ap.add_argument("--kv8", action="store_true", help="only the fp8-cache kernels against their bf16 _paged twins")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if out:
            out.write(json.dumps(rec) + "\n")
            out.flush()

    g = torch.Generator(device="cuda").manual_seed(0)
    if a.ragged:
        ragged_rows(emit, g, a.iters)
        return
    if a.paged:
        paged_rows(emit, g, a.iters)
        return
    if a.kv8:
        kv8_rows(emit, g, a.iters)
        return
    if not a.skip_kernel:
        kernel_row(emit, g, a.iters, 8, 1024, 0, 2048, "llm5 prompt")
        t0 = kernel_row(emit, g, a.iters, 1, 4096, 0, 8192, "4k prompt")
        kernel_row(emit, g, a.iters, 1, 8192, 0, 8192, "8k prompt")
        kernel_row(emit, g, a.iters, 1, 512, 7680, 8192, "chunk 512 at 7680")
        t1 = kernel_row(emit, g, a.iters, 1, 4096, 4096, 8192, "4k chunk at 4096", sdpa=False)
        # the (S 4096, pos 4096) call has 3x the unmasked keys of (S 4096, pos 0): a time
        # ratio near 1 would mean the tiles above the diagonal are not skipped
        emit({"bench": "prefill_attn_causal_skip", "t_pos0_over_t_pos4096": round(t0 / t1, 3), "work_ratio": 0.333})
        torch.cuda.empty_cache()
    if not a.skip_model:
        model_rows(emit, 8, 1024, ROUNDS)


if __name__ == "__main__":
    main()
