"""Fixtures of the token sampler (pbs_amd.ops.llm, "token sampling"): seeded, built on the CPU, no GPU needed.

A case is a dict: name, logits bf16 [B, V], and the vectors [B] inv_temp fp32, top_k int32, top_p fp32, seed int64,
ctr int32.  V is 8 (less than one wave), 1024 (the test model's vocabulary), 8200 (one 1024 x 8 tile of the kernel
plus a tail of 8) or, once, 128256; B is 1, 3 or 8.

* random_cases(): N(0, 9) rows, parameters by row: temperature 0.7 .. 1.4, (top_k, top_p) from (0, 1), (50, 1),
  (0, 0.9), (5, 0.5) in turn, eight counters per row.  This is the mix a serving engine runs, and the one the
  vacuity guard of tests/test_gpu_sample.py is stated over: every row keeps at least two tokens.
* edge_cases(): N(0, 9) rows at the ends of the parameter ranges, where one kept token is the definition and not a
  vacuous case: temperature 0.05, top_k 1, top_k = V (inactive), top_p 2^-16.  Eight counters per row as well.
* constructed_cases(): special_case(), whose rows are: all logits equal, one logit 40 above the rest, a greedy row
  with a tied maximum, a tie that straddles the k-th value, an idle row between active rows, a tie that straddles
  the nucleus edge, a row with -inf entries, and a second row with the same logits, seed and counter; and
  equal_case() at three more shapes.
"""
import functools

import numpy as np
import torch

TILE = 8192  # elements of one scan tile of k_sample_rows: 1024 threads x 8
COUNTERS = (0, 1, 2, 3, 17, 1000, 65535, 2 ** 31 - 1)
MIX = ((0, 1.0), (50, 1.0), (0, 0.9), (5, 0.5))  # (top_k, top_p) of row i % 4
SEEDS = (1, 2 ** 32 + 5, -7, 2 ** 63 - 1, 123456789, 0, 2 ** 40, -2 ** 63)
# (V, B, generator seed): the first seed from 1000 + V + B on at which every row keeps two tokens or more (a row whose
# largest weight alone holds half of its top-5 mass keeps one under (top_k 5, top_p 0.5))
RANDOM_SHAPES = ((8, 8, 1035), (1024, 3, 2027), (8200, 8, 9209), (128256, 3, 129259))
EDGE_SHAPES = ((8, 3), (1024, 8), (8200, 1))


def inv_temp(T: float) -> float:
    """fp32(1) / fp32(T) on the host, 0 for greedy: what the caller of the sampler computes."""
    return float(np.float32(1.0) / np.float32(T)) if T else 0.0


def case(name, logits, temps, top_k, top_p, seed, ctr):
    B = logits.shape[0]
    assert logits.dtype == torch.bfloat16 and all(len(v) == B for v in (temps, top_k, top_p, seed, ctr))
    return {"name": name, "logits": logits,
            "inv_temp": torch.tensor([inv_temp(T) for T in temps], dtype=torch.float32),
            "top_k": torch.tensor(top_k, dtype=torch.int32), "top_p": torch.tensor(top_p, dtype=torch.float32),
            "seed": torch.tensor(seed, dtype=torch.int64), "ctr": torch.tensor(ctr, dtype=torch.int32)}


def args(c, device=None):
    """The six positional arguments of llm.sample / llm.sample_ref."""
    t = [c[k] for k in ("logits", "inv_temp", "top_k", "top_p", "seed", "ctr")]
    return [v.to(device) for v in t] if device is not None else t


def _normal(V, B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * 3.0).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def random_cases():
    out = []
    for V, B, gen in RANDOM_SHAPES:
        x = _normal(V, B, gen)
        temps = [0.7 + 0.1 * (i % 8) for i in range(B)]
        for c in COUNTERS:
            out.append(case(f"random V={V} B={B} ctr={c}", x, temps, [MIX[i % 4][0] for i in range(B)],
                            [MIX[i % 4][1] for i in range(B)], [SEEDS[i % 8] for i in range(B)], [c] * B))
    return out


@functools.lru_cache(maxsize=None)
def edge_cases():
    out = []
    ends = lambda V: ((0.05, 0, 1.0), (1.0, 1, 1.0), (0.9, V, 1.0), (1.1, 0, 2.0 ** -16), (0.05, 5, 0.5),  # noqa: E731
                      (1.4, V, 2.0 ** -16), (0.7, 1, 0.9), (1.0, V + 1, 0.5))
    for V, B in EDGE_SHAPES:
        x = _normal(V, B, 2000 + V + B)
        e = ends(V)[:B] if B > 1 else ends(V)[3:4]
        for c in COUNTERS:
            out.append(case(f"edge V={V} B={B} ctr={c}", x, [p[0] for p in e], [p[1] for p in e], [p[2] for p in e],
                            [SEEDS[(i + 3) % 8] for i in range(B)], [c] * B))
    return out


def equal_case(V, B):
    """All logits equal: every weight is 2^30 and the token is floor(R V / 2^64), the index order of the scan."""
    return case(f"equal V={V} B={B}", torch.full((B, V), 0.5, dtype=torch.bfloat16), [1.0] * B, [0] * B, [1.0] * B,
                [SEEDS[i % 8] for i in range(B)], [COUNTERS[(i + 2) % 8] for i in range(B)])


SPECIAL_ROWS = ("equal", "peak", "greedy_tie", "k_tie", "idle", "p_tie", "neg_inf", "neg_inf_twin")
PEAK_AT, TIE_AT = 777, (900, 41, 333)


@functools.lru_cache(maxsize=None)
def special_case():
    """B 8, V 1024, rows in the order of SPECIAL_ROWS."""
    V = 1024
    g = torch.Generator().manual_seed(31)
    x = torch.empty(8, V)
    x[0] = 0.5
    x[1] = torch.randn(V, generator=g).clamp(-2, 2)
    x[1, PEAK_AT] = 42.0  # 40 above the largest of the rest: every other weight is zero
    x[2] = torch.randn(V, generator=g).clamp(-2, 2)
    x[2, list(TIE_AT)] = 3.0  # greedy: the lowest of the three tied indices
    x[3] = -torch.rand(V, generator=g) * 4 - 1
    x[3, [10, 600]] = 5.0
    x[3, [5, 300, 1023]] = 4.0  # top_k 3: the third largest value is tied three times, all three are kept
    x[4] = torch.randn(V, generator=g) * 3  # idle
    x[5] = -30.0
    x[5, 512] = 3.0
    x[5, [0, 7, 511, 1016]] = 2.0  # top_p 0.5: the first weight is 40 % of the mass, the tie of four crosses the edge
    x[6] = torch.randn(V, generator=g) * 3
    x[6, torch.randperm(V, generator=g)[:V // 3]] = float("-inf")
    x[7] = x[6]
    return case("special", x.to(torch.bfloat16), [1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.8, 0.8], [0, 0, 0, 3, 50, 0, 0, 0],
                [1.0, 1.0, 1.0, 1.0, 0.9, 0.5, 0.9, 0.9], [11, 12, 13, 14, 15, 16, 99, 99], [4, 5, 6, 7, -1, 9, 21, 21])


def constructed_cases():
    return [special_case(), equal_case(8, 1), equal_case(8200, 3), equal_case(1024, 8)]


def all_cases():
    return random_cases() + edge_cases() + constructed_cases()


_REF = {}


def reference(c):
    """llm.sample_ref of a case on the CPU, computed once and shared by the tests: (tokens, stats), read-only."""
    from pbs_amd.ops import llm
    if c["name"] not in _REF:
        _REF[c["name"]] = llm.sample_ref(*args(c))
    return _REF[c["name"]]
