"""MXFP4 decode-linear microbench: llm.mxfp4_linear_q (k_mxfp4_gemm_skinny, 4.25 bits per weight) against
llm.fp8_linear_q (k_fp8_gemm_skinny, 8 bits) on the four llama3-8b decode shapes at M 1, 8 and 64.  Each result is
checked against its fp64 reference and derived bound before anything is timed.  Within each of the 5 rounds the
fp8 linear is timed, then the fp4 linear, then the fp8 linear again, so the rows carry the spread of the fp8 linear
against itself; a row reports the median of the rounds with min / max and the per-round ratios.  A timing is
--iters launches captured in one graph and replayed 5 times (an eager loop would time the host).  Two settings per
shape: "hot", one weight launched back to back (it stays in the 256 MB last-level cache where it fits), and
"rotating", copies of the weight taken in turn so that the launches of one pass touch at least --rotate-mib of
fp4 bytes (and 1.9 times that in fp8): what a decode step, which streams every weight once, sees.  Then the
dim-512 test model's w4-versus-emulate and sliced-versus-tiled cosines (the numbers of
tests/test_gpu_mxfp4_decoder.py), and a whole llama3-8b decode step (batch 8, graph) with w4 off and on.

    python scripts/mxfp4_bench.py [--iters 200] [--no-model] [--out profiles/mxfp4_linear.jsonl]
"""
import argparse
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pbs_amd.models.llama import PRESETS, LlamaConfig, LlamaDecoder  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

ROUNDS = 5
SHAPES = {"qkv": (6144, 4096), "o": (4096, 4096), "w13": (28672, 4096), "w2": (4096, 14336)}  # [N, K]
MS = (1, 8, 64)
GRAPH_REPLAYS = 5


def timeit(fn, iters):
    """us per call of `iters` calls replayed from one captured graph: the small shapes take less than the host
    needs to enqueue a launch, so an eager loop would time the Python wrappers."""
    dev = torch.cuda.current_device()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(GRAPH_REPLAYS):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (GRAPH_REPLAYS * iters) * 1e3  # us


def timeit_eager(fn, iters):
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


def clones(w, n):
    """n weights with the bytes of w at n places."""
    out = [w]
    for _ in range(n - 1):
        c = copy.copy(w)
        for name in ("qs", "ss", "s"):
            if hasattr(w, name):
                setattr(c, name, getattr(w, name).clone())
        out.append(c)
    return out


def check(xq, sx, w8, w4):
    """Both kernels against the fp64 product of their own operands and the derived bounds of the tests."""
    K = w4.K
    ku = K * 2.0 ** -24
    x = xq.double()
    ref4 = llm.mxfp4_linear_ref(xq, sx, w4)
    a4 = x.abs() @ w4.dequant().double().abs().t() * sx.double()[:, None]
    e4 = (llm.mxfp4_linear_q(xq, sx, w4).double() - ref4).abs()
    f4 = (e4 / (2.0 ** -8 * ref4.abs() + (1 + 2.0 ** -8) * ku / (1 - ku) * a4)).max().item()
    sc = sx.double()[:, None] * w8.s.double()[None, :]
    q8 = w8.q.double()
    ref8 = x @ q8.t() * sc
    e8 = (llm.fp8_linear_q(xq, sx, w8).double() - ref8).abs()
    f8 = (e8 / (2.0 ** -8 * ref8.abs() + K * 2.0 ** -24 * (x.abs() @ q8.abs().t()) * sc)).max().item()
    assert f4 <= 1 and f8 <= 1, f"outside the derived bound: fp4 {f4:.3f}, fp8 {f8:.3f} of it"
    return round(f4, 3), round(f8, 3)


def linear_rows(emit, iters, rotate_mib):
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, (N, K) in SHAPES.items():
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16()
        w8, w4 = llm.Fp8Weight(w), llm.Mxfp4Weight(w)
        del w
        n = max(2, -(-rotate_mib * 2 ** 20 // w4.nbytes()))
        sets = {"hot": ([w8], [w4]), "rotating": (clones(w8, n), clones(w4, n))}
        for M in MS:
            xq, sx = llm.quant_rows_fp8(torch.randn(M, K, device="cuda", generator=g).bfloat16())
            frac = check(xq, sx, w8, w4)
            for setting, (l8, l4) in sets.items():
                turn = [0]

                def run(fn, ws):
                    turn[0] += 1
                    return fn(xq, sx, ws[turn[0] % len(ws)])

                variants = {"fp8 (first)": lambda: run(llm.fp8_linear_q, l8), "fp4": lambda: run(llm.mxfp4_linear_q, l4),
                            "fp8 (second)": lambda: run(llm.fp8_linear_q, l8)}
                times = {k: [] for k in variants}
                for _ in range(ROUNDS):
                    for k, fn in variants.items():
                        times[k].append(timeit(fn, iters))
                t8, t4, t8b = times["fp8 (first)"], times["fp4"], times["fp8 (second)"]
                emit({"bench": "mxfp4-linear", "shape": name, "N": N, "K": K, "M": M, "setting": setting,
                      "copies": len(l4), "bytes_fp8": w8.nbytes(), "bytes_fp4": w4.nbytes(),
                      "bytes_ratio": round(w4.nbytes() / w8.nbytes(), 4), "fp8_first": stat(t8), "fp4": stat(t4),
                      "fp8_second": stat(t8b), "fp4_over_fp8_first_per_round": [round(b / a, 3) for a, b in zip(t8, t4)],
                      "fp8_second_over_first_per_round": [round(b / a, 3) for a, b in zip(t8, t8b)],
                      "fp4_GBps": round(w4.nbytes() / med(t4) / 1e3, 1), "fp8_GBps": round(w8.nbytes() / med(t8) / 1e3, 1),
                      "fraction_of_bound_fp4_fp8": frac})
        del sets, w8, w4
        torch.cuda.empty_cache()


def last_logits(d, toks):
    seen, fwd = [], d._forward

    def spy(*a, **k):
        r = fwd(*a, **k)
        if r is not None:
            seen.append(r[:, -1].float().clone())
        return r

    d._forward = spy
    try:
        d.prefill(toks)
    finally:
        d._forward = fwd
    return seen[-1]


def cosine_rows(emit):
    """The six numbers of test_w4_tracks_its_fp8_oracle...: dim-512 test model, 40-token prefill, three token seeds."""
    cfg = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)
    kw = dict(batch=1, context=64, fp8=True, prefill_attn=True)
    decs = [LlamaDecoder(cfg, w4=True, **kw), LlamaDecoder(cfg, w4="emulate", **kw), LlamaDecoder(cfg, **kw),
            LlamaDecoder(cfg, prefill_tiled=True, **kw)]
    ours, yard = [], []
    for seed in (21, 22, 23):
        toks = torch.randint(0, cfg.vocab, (1, 40), generator=torch.Generator().manual_seed(seed)).cuda()
        lg = [last_logits(d, toks).double() for d in decs]
        cos = torch.nn.functional.cosine_similarity
        ours.append(cos(lg[0], lg[1], dim=-1).min().item())
        yard.append(cos(lg[2], lg[3], dim=-1).min().item())
    emit({"bench": "mxfp4-oracle-cosine", "model": "dim 512, 2 layers, vocab 1024, batch 1, 40-token prefill",
          "token_seeds": [21, 22, 23], "w4_vs_emulate": [round(c, 6) for c in ours],
          "fp8_sliced_vs_tiled": [round(c, 6) for c in yard],
          "threshold": round(min(yard) - (max(yard) - min(yard)), 6)})


def model_rows(emit, iters):
    cfg = PRESETS["llama3-8b"]
    decs = {}
    for w4 in (False, True):
        d = LlamaDecoder(cfg, batch=8, context=1024, fp8=True, graph=True, w4=w4)
        g = torch.Generator().manual_seed(1)
        decs[w4] = (d, [d.prefill(torch.randint(0, cfg.vocab, (8, 64), generator=g).cuda())])
        blocks = sum(w.nbytes() for layer in d.model.layers for w in layer._fp8.values())
        emit({"bench": "mxfp4-model-bytes", "model": "llama3-8b", "w4": w4, "block_linear_bytes": blocks,
              "head_bytes": d.model._fp8_head.nbytes()})
    times = {k: [] for k in decs}

    def step(k):
        d, tok = decs[k]
        tok[0] = d.decode_step(tok[0])

    steps = min(iters, 50)  # 2 + 50 steps per timing, 5 rounds, 2 decoders: inside the context of 1024
    for _ in range(ROUNDS):
        for k in decs:
            times[k].append(timeit_eager(lambda: step(k), steps))  # the step replays its own graph
    for k, ts in times.items():
        emit({"bench": "mxfp4-decode-step", "model": "llama3-8b, batch 8, context 1024, fp8 activations, graph", "w4": k,
              **stat(ts), "vs_fp8_step_per_round": [round(a / b, 3) for a, b in zip(ts, times[False])]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rotate-mib", type=int, default=768)
    ap.add_argument("--no-model", action="store_true", help="skip the llama3-8b decode step")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_bench: needs a GPU")
    rows = []

    def emit(rec):
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:  # rewritten after every row: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")

    linear_rows(emit, a.iters, a.rotate_mib)
    cosine_rows(emit)
    if not a.no_model:
        model_rows(emit, a.iters)


if __name__ == "__main__":
    main()
