"""fp8 forms of the paged attention fixtures (tests/test_kv8_cpu.py,
tests/test_gpu_kv8_attn.py): a paged case of paged_cases / weighted_cases with
its pools quantised by llm.kv8_quant_ref into e4m3 code pools and fp32 scales,
the dequantised bf16 twin pools (what the bf16 _paged kernels are run on), and,
for the one-hot fixtures, expect8.

Poisoning: every unreferenced page and every page row past a sequence's last
row gets code byte 0x7f (e4m3fn NaN) and a NaN scale, so the twin pools are NaN
there as the bf16 pools were.  Table garbage stays as paged_cases makes it.

On the one-hot fixtures the K codes (+-8 and 0) survive the codec unchanged
(asserted here), so every score is what it was; every V row changes, and the
reference still returns exactly one V row, the dequantised one.  The codec acts
on a row alone, so expect8 is kv8_round of the bf16 expectation, head row by
head row.
"""
import torch

import decode_cases as DC
import paged_cases as PG
import weighted_cases as WC

from pbs_amd.ops import llm

BF = torch.bfloat16
NAN_CODE = 0x7F


def live_rows(c) -> torch.Tensor:
    """bool [P, page]: the pool rows that are a sequence's rows 0 .. rows[b] - 1."""
    P, _, page, _ = c["kpool"].shape
    live = torch.zeros(P, page, dtype=torch.bool)
    for ids, r in zip(c["ids"], c["rows"]):
        for i, pg in enumerate(ids):
            live[pg, :min(page, r - i * page)] = True
    return live


def poison(codes: torch.Tensor, scale: torch.Tensor, live: torch.Tensor):
    """Code 0x7f and a NaN scale in every row that is not live; returns new tensors."""
    c8 = codes.view(torch.uint8).clone()
    c8[~live[:, None, :].expand(c8.shape[:3])] = NAN_CODE
    sc = scale.clone()
    sc[~live[:, None, :].expand_as(sc)] = float("nan")
    return c8.view(torch.float8_e4m3fn), sc


def quantise(c, k_exact: bool = False):
    """A paged case with the four fp8 tensors, the twin pools and `live` added."""
    live = live_rows(c)
    keep = live[:, None, :, None]
    out = dict(c, live=live)
    for name in ("k", "v"):
        pool = c[name + "pool"]
        assert torch.isfinite(pool[keep.expand_as(pool)]).all()
        codes, scale = llm.kv8_quant_ref(torch.where(keep, pool, torch.zeros_like(pool)))
        codes, scale = poison(codes, scale, live)
        twin = llm.kv8_dequant(codes, scale)
        assert torch.isnan(twin[~keep.expand_as(pool)]).all()
        if name == "k" and k_exact:  # the coded K rows are fixed points of the codec
            assert torch.equal(twin[keep.expand_as(pool)], pool[keep.expand_as(pool)])
        out.update({name + "pool8": codes, name + "scale": scale, name + "twin": twin})
    return out


def expect8(expect: torch.Tensor, H: int) -> torch.Tensor:
    """The bf16 expectation of a one-hot fixture ([..., H * 128], one V row per
    head) with every head row rounded through the codec."""
    rows = expect.reshape(*expect.shape[:-1], H, DC.HD)
    out = llm.kv8_round(rows).reshape(expect.shape)
    changed = (out != expect).reshape(-1, H, DC.HD).any(-1)
    live = (expect != 0).reshape(-1, H, DC.HD).any(-1)
    assert changed[live].all()  # every V row of the fixtures changes under the codec
    return out


def decode_case(s: int, H: int, Hkv: int, page: int, shift: int = 0):
    c = quantise(PG.decode_case(s, H, Hkv, page, shift), k_exact=True)
    c["expect8"] = expect8(c["expect"], H)
    return c


def prefill_case(s: int, H: int, Hkv: int, page: int, shift: int = 0):
    c = quantise(PG.prefill_case(s, H, Hkv, page, shift), k_exact=True)
    c["expect8"] = expect8(c["expect"], H)
    return c


def weighted_case(kind: str, pairs, H: int, Hkv: int, page: int):
    """The census / ramp prefill fixtures of weighted_cases: bit-equality with the twin only."""
    return quantise(WC.paged_case(kind, pairs, H, Hkv, page))


def decode_case_256(kind: str, s: int, H: int, Hkv: int):
    c = quantise(WC.decode_case_256(kind, s, H, Hkv), k_exact=(kind == "exact"))
    if kind == "exact":
        c["expect8"] = [None if e is None else expect8(e, H) for e in c["expect"]]
    return c


# ------------------------------------------------------------------ codec rows
EDGE_K = (-90, -20, -1, 0, 3, 40, 100)


def edge_rows(seed: int = 0):
    """(rows bf16 [N, 128], want_e [N]): rows whose amax is 448 * 2^k (the top of a
    scale's range: e = k) and 450 * 2^k (just past it: e = k + 1) for k in EDGE_K,
    224 * 2^k (rounds into the lower scale: e = k - 1), an all-zero row (e = 0)
    and rows with amax 2^-120 and 1.5 * 2^-110, below 224 * 2^-100 (the clamp:
    e = -100).  The other elements are random fractions of amax, both signs; amax
    sits at element 5 n % 128, negative in every second row."""
    g = torch.Generator().manual_seed(seed)
    amax, want = [], []
    for k in EDGE_K:
        amax += [448.0 * 2.0 ** k, 450.0 * 2.0 ** k, 224.0 * 2.0 ** k]
        want += [k, k + 1, k - 1]
    amax += [0.0, 2.0 ** -120, 1.5 * 2.0 ** -110]
    want += [0, -100, -100]
    a = torch.tensor(amax, dtype=torch.float64)
    assert torch.equal(a.to(BF).double(), a)  # every amax is a bf16 value
    rows = ((torch.rand(len(amax), DC.HD, generator=g, dtype=torch.float64) * 2 - 1) * 0.999 * a[:, None]).to(BF)
    rows = torch.where(rows.double().abs() > a[:, None], torch.zeros_like(rows), rows)  # rounding up past amax
    for n in range(len(amax)):
        rows[n, 5 * n % DC.HD] = amax[n] if n % 2 == 0 else -amax[n]
    return rows, torch.tensor(want)
