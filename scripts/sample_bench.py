"""Token sampling microbench: llm.sample (k_sample_rows, one workgroup per row) against the torch composition a
user would write on the same bf16 logits, softmax(x / T) -> sort -> cumsum -> mask -> multinomial, and against
argmax alone; B 8 and B 64 at V 128256 (llama3's vocabulary), every row with T 0.8, top_k 50, top_p 0.9.  The
kernel's tokens and stats are checked against llm.sample_ref before anything is timed.  Within each of the 5 rounds
the variants alternate and the torch composition is timed twice, so the rows carry its spread against itself; a row
reports the median of the rounds with min / max.  Then the decode step of the dim-512 test model (batch 4, fp8,
graph=True) with sampling=True against sampling=False: what a user pays per token.

    python scripts/sample_bench.py [--iters 100] [--out profiles/sample.jsonl]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pbs_amd.models.llama import LlamaConfig, LlamaDecoder  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

ROUNDS = 5
V = 128256
T, TOP_K, TOP_P = 0.8, 50, 0.9


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


def stat(ts):
    return {"us": round(med(ts), 1), "us_minmax": [round(min(ts), 1), round(max(ts), 1)]}


def torch_sample(x):
    """Temperature, top-k and top-p with torch ops: what the decoder's user writes without the kernel."""
    p = torch.softmax(x.float() / T, -1)
    ps, idx = p.sort(-1, descending=True)
    ps = torch.where(torch.arange(x.shape[1], device=x.device) < TOP_K, ps, torch.zeros_like(ps))
    ps = ps / ps.sum(-1, keepdim=True)
    ps = torch.where(ps.cumsum(-1) - ps < TOP_P, ps, torch.zeros_like(ps))
    return idx.gather(1, torch.multinomial(ps, 1))


def kernel_rows(emit, iters):
    import numpy as np
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in (8, 64):
        x = (torch.randn(B, V, device="cuda", generator=g) * 3.0).bfloat16()
        vec = (torch.full((B,), float(np.float32(1.0) / np.float32(T)), device="cuda"),
               torch.full((B,), TOP_K, dtype=torch.int32, device="cuda"), torch.full((B,), TOP_P, device="cuda"),
               torch.arange(B, device="cuda") + 11, torch.arange(B, dtype=torch.int32, device="cuda") + 100)
        plain = (vec[0], torch.zeros_like(vec[1]), torch.ones_like(vec[2]), vec[3], vec[4])
        greedy = (torch.zeros_like(vec[0]),) + vec[1:]
        for v in (vec, plain, greedy):  # exact against the reference first
            tok, st = llm.sample(x, *v, stats=True)
            want = llm.sample_ref(x.cpu(), *(t.cpu() for t in v))
            assert torch.equal(tok.cpu(), want[0]) and torch.equal(st.cpu(), want[1]), "kernel != sample_ref"
        variants = {"torch composition (first)": lambda: torch_sample(x),
                    "kernel top_k 50 top_p 0.9": lambda: llm.sample(x, *vec),
                    "kernel temperature only": lambda: llm.sample(x, *plain),
                    "kernel greedy": lambda: llm.sample(x, *greedy),
                    "torch argmax": lambda: x.argmax(-1, keepdim=True),
                    "torch composition (second)": lambda: torch_sample(x)}
        times = {k: [] for k in variants}
        for _ in range(ROUNDS):
            for k, fn in variants.items():
                times[k].append(timeit(fn, iters))
        base = med(times["torch composition (first)"])
        for k, ts in times.items():
            emit({"bench": "sample", "variant": k, "B": B, "V": V, "T": T, "top_k": TOP_K, "top_p": TOP_P,
                  "geometry": "one workgroup of 1024 threads per row", **stat(ts),
                  "vs_torch_composition": round(base / med(ts), 2), "exact_vs_sample_ref": k.startswith("kernel")})


def decoder_rows(emit, iters):
    cfg = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=2048)
    decs = {}
    for sampling in (False, True):
        torch.manual_seed(0)
        d = LlamaDecoder(cfg, batch=4, context=2048, fp8=True, graph=True, ragged=True, sampling=sampling)
        if sampling:
            d.set_sampling(temperature=T, top_k=TOP_K, top_p=TOP_P, seed=3)
        g = torch.Generator().manual_seed(1)
        decs[sampling] = (d, [d.prefill(torch.randint(0, cfg.vocab, (4, 64), generator=g).cuda())])
    times = {k: [] for k in decs}

    def step(k):
        d, tok = decs[k]
        tok[0] = d.decode_step(tok[0])

    steps = min(iters, 50)  # 2 + 50 steps per timing, 5 rounds: inside the context of 2048
    for _ in range(ROUNDS):
        for k in decs:
            times[k].append(timeit(lambda: step(k), steps))
    for k, ts in times.items():
        emit({"bench": "sample-decode-step", "model": "dim 512, 2 layers, vocab 1024, batch 4, fp8, ragged, graph",
              "sampling": k, **stat(ts), "vs_argmax_step": round(med(ts) / med(times[False]), 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []

    def emit(rec):
        rows.append(rec)
        print(json.dumps(rec), flush=True)

    kernel_rows(emit, a.iters)
    decoder_rows(emit, a.iters)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
