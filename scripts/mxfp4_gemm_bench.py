"""Tiled MXFP4 GEMM bench: llm.mxfp4_linear_q(tiled=True) (k_gemm_mxfp4_tn, one launch for any M) against the
sliced llm.mxfp4_linear_q (k_mxfp4_gemm_skinny, one launch per 64 rows: the path of before and the time yardstick)
and against llm.fp8_linear_q(tiled=True) on an fp8 weight of the same shape, on the four llama3-8b shapes at M 512,
2048 and 8192.  Each result is checked against the fp64 product of its own operands and the derived bound of the
tests before anything is timed.  Within each of the 5 rounds the sliced path is timed, then the tiled fp4 launch,
then the tiled fp8 launch, then the sliced path again, so a row carries the spread of the sliced path against
itself; a row reports the median of the rounds with min / max and the per-round ratios.  A timing is an eager loop
between two events: every call here is tens of microseconds to milliseconds of GPU work, more than the host needs
to enqueue it (the sliced path is M / 64 launches per call).  --part model: the whole llama3-8b prefill of 8 x 1024
tokens (prefill_attn=True) with w4=True, with w4=True, w4_tiled=True, and with fp8 weights and prefill_tiled=True.

The two parts are separate runs so that each can have a time limit of its own; the second appends to --out:

    timeout 600 python scripts/mxfp4_gemm_bench.py --part linear --out profiles/mxfp4_gemm.jsonl
    timeout 600 python scripts/mxfp4_gemm_bench.py --part model --out profiles/mxfp4_gemm.jsonl --append
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pbs_amd.models.llama import PRESETS, LlamaDecoder  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

ROUNDS = 5
SHAPES = {"qkv": (6144, 4096), "o": (4096, 4096), "w13": (28672, 4096), "w2": (4096, 14336)}  # [N, K]
MS = (512, 2048, 8192)
ITERS = {512: 20, 2048: 10, 8192: 5}


def timeit(fn, iters):
    """us per call of an eager loop of `iters` calls after 2 warm-up calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def med(ts):
    return sorted(ts)[len(ts) // 2]


def stat(ts):
    return {"us": round(med(ts), 1), "us_minmax": [round(min(ts), 1), round(max(ts), 1)]}


def check(xq, sx, w8, w4, rows=1024):
    """Largest fraction of the derived bound (tests/mxfp4_cases.real_case) of the sliced fp4, tiled fp4 and tiled
    fp8 results, against the fp64 product of each kernel's own operands; `rows` rows at a time."""
    K, ku = w4.K, w4.K * 2.0 ** -24
    ys = {"sliced": llm.mxfp4_linear_q(xq, sx, w4), "tiled": llm.mxfp4_linear_q(xq, sx, w4, tiled=True),
          "fp8": llm.fp8_linear_q(xq, sx, w8, tiled=True)}
    d4, q8, s8 = w4.dequant().double(), w8.q.double(), w8.s.double()
    worst = {k: 0.0 for k in ys}
    for m0 in range(0, xq.shape[0], rows):
        x, s = xq[m0:m0 + rows].double(), sx[m0:m0 + rows].double()[:, None]
        ref = x @ d4.t() * s
        bound = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * ku / (1 - ku) * (x.abs() @ d4.abs().t() * s)
        for k in ("sliced", "tiled"):
            worst[k] = max(worst[k], ((ys[k][m0:m0 + rows].double() - ref).abs() / bound.clamp(min=1e-300)).max().item())
        sc = s * s8[None, :]
        ref = x @ q8.t() * sc
        bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * (x.abs() @ q8.abs().t()) * sc
        worst["fp8"] = max(worst["fp8"], ((ys["fp8"][m0:m0 + rows].double() - ref).abs() / bound.clamp(min=1e-300)).max().item())
    assert all(v <= 1 for v in worst.values()), f"outside the derived bound: {worst}"
    return {k: round(v, 3) for k, v in worst.items()}


def linear_rows(emit):
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, (N, K) in SHAPES.items():
        w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16()
        w8, w4 = llm.Fp8Weight(w), llm.Mxfp4Weight(w)
        del w
        for M in MS:
            xq, sx = llm.quant_rows_fp8(torch.randn(M, K, device="cuda", generator=g).bfloat16())
            frac = check(xq, sx, w8, w4)
            torch.cuda.empty_cache()
            variants = {"sliced (first)": lambda: llm.mxfp4_linear_q(xq, sx, w4),
                        "tiled": lambda: llm.mxfp4_linear_q(xq, sx, w4, tiled=True),
                        "fp8 tiled": lambda: llm.fp8_linear_q(xq, sx, w8, tiled=True),
                        "sliced (second)": lambda: llm.mxfp4_linear_q(xq, sx, w4)}
            times = {k: [] for k in variants}
            for _ in range(ROUNDS):
                for k, fn in variants.items():
                    times[k].append(timeit(fn, ITERS[M]))
            s1, t4, t8, s2 = (times[k] for k in variants)
            emit({"bench": "mxfp4-gemm-linear", "shape": name, "N": N, "K": K, "M": M, "iters": ITERS[M],
                  "sliced_first": stat(s1), "tiled": stat(t4), "fp8_tiled": stat(t8), "sliced_second": stat(s2),
                  "sliced_over_tiled_per_round": [round(a / b, 3) for a, b in zip(s1, t4)],
                  "sliced_second_over_first_per_round": [round(b / a, 3) for a, b in zip(s1, s2)],
                  "tiled_over_fp8_tiled_per_round": [round(a / b, 3) for a, b in zip(t4, t8)],
                  "tiled_TFLOPs": round(2.0 * M * N * K / med(t4) / 1e6, 1),
                  "fp8_tiled_TFLOPs": round(2.0 * M * N * K / med(t8) / 1e6, 1), "fraction_of_bound": frac})
        del w8, w4
        torch.cuda.empty_cache()


def model_rows(emit):
    cfg = PRESETS["llama3-8b"]
    toks = torch.randint(0, cfg.vocab, (8, 1024), generator=torch.Generator().manual_seed(1)).cuda()
    kinds = {"w4 sliced": dict(w4=True), "w4 tiled": dict(w4=True, w4_tiled=True), "fp8 tiled": dict(prefill_tiled=True)}
    times = {k: [] for k in kinds}
    decs = {k: LlamaDecoder(cfg, batch=8, context=1024, fp8=True, prefill_attn=True, **kw) for k, kw in kinds.items()}
    first = {k: d.prefill(toks).flatten().tolist() for k, d in decs.items()}
    for _ in range(ROUNDS):
        for k, d in decs.items():
            times[k].append(timeit(lambda: d.prefill(toks), 2) / 1e3)
    for k, ts in times.items():
        emit({"bench": "mxfp4-gemm-prefill", "model": "llama3-8b, batch 8 x 1024 tokens, fp8 activations, prefill_attn",
              "kind": k, "ms": round(med(ts), 2), "ms_minmax": [round(min(ts), 2), round(max(ts), 2)],
              "vs_w4_sliced_per_round": [round(a / b, 3) for a, b in zip(ts, times["w4 sliced"])],
              "next_tokens_equal_w4_sliced": first[k] == first["w4 sliced"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("linear", "model"), required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="keep the rows already in --out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_gemm_bench: needs a GPU")
    rows = []
    if a.out and a.append and os.path.exists(a.out):
        with open(a.out) as f:
            rows = [json.loads(line) for line in f if line.strip()]

    def emit(rec):
        rows.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:  # rewritten after every row: a run that is cut short keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")

    (linear_rows if a.part == "linear" else model_rows)(emit)


if __name__ == "__main__":
    main()
