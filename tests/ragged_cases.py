"""Ragged cases of the per-sequence attention tests (tests/test_ragged_cpu.py,
tests/test_gpu_ragged_attn.py), assembled from the uniform fixtures of
decode_cases (B 4, C 1100) and prefill_cases (B 2, C 400): sequence b of a
ragged case is row b of the uniform exact-data fixture built for that
sequence's own position (and length), so its expected output is still one V
row bit for bit, and the uniform kernel at that position is a second
reference.

An idle sequence (decode: pos outside [0, C); prefill: None) has caches that
are NaN throughout and a NaN query: nothing of it may be loaded, and its
expected output is zero bits.
"""
import functools

import torch

import decode_cases as DC
import prefill_cases as PC

BF = torch.bfloat16

# decode: per-sequence positions; the last set holds an idle sequence by both
# rules (negative, and >= C)
DECODE_SETS = [[0, 63, 512, 1099], [1099, 64, -1, 511], [1023, 1024, 575, 62], [-1, -1, 1100, 5]]

# prefill: per-sequence (S, pos) pairs out of PC.SHAPES, None = idle
PREFILL_SETS = [((200, 0), (7, 0)), ((65, 64), (129, 130)), ((1, 137), (150, 249)), ((63, 5), None)]


@functools.lru_cache(maxsize=None)
def _decode_uniform(pos, H, Hkv, shift):
    return DC.exact_case(pos, H, Hkv, shift)


@functools.lru_cache(maxsize=None)
def _prefill_uniform(S, pos, H, Hkv, shift):
    return PC.exact_case(S, pos, H, Hkv, shift)


def decode_active(pos: int) -> bool:
    return 0 <= pos < DC.C


def decode_case(positions, H: int, Hkv: int, shift: int = 0):
    """(q [B, H, 128], kc, vc [B, Hkv, C, 128], t [B, H], expect [B, H * 128]) in
    bf16: sequence b is row b of DC.exact_case(positions[b], ...).  With shift = 1
    every sequence that has a row pos + 1 takes the shifted fixture (targets one
    up, row pos + 1 coded); a sequence at C - 1 keeps the unshifted one.  Idle
    sequences: NaN q and caches, t = -1, expect 0."""
    assert len(positions) == DC.B
    q = torch.full((DC.B, H, DC.HD), float("nan"), dtype=BF)
    kc = torch.full((DC.B, Hkv, DC.C, DC.HD), float("nan"), dtype=BF)
    vc = torch.full((DC.B, Hkv, DC.C, DC.HD), float("nan"), dtype=BF)
    t = torch.full((DC.B, H), -1, dtype=torch.long)
    expect = torch.zeros(DC.B, H * DC.HD, dtype=BF)
    for b, pos in enumerate(positions):
        if not decode_active(pos):
            continue
        sh = shift if pos + shift + 1 <= DC.C else 0
        uq, uk, uv, ut, ue = _decode_uniform(pos, H, Hkv, sh)
        q[b], kc[b], vc[b], t[b], expect[b] = uq[b], uk[b], uv[b], ut[b], ue[b]
    return q, kc, vc, t, expect


def prefill_tokens(pair) -> int:
    return 0 if pair is None else pair[0]


def prefill_case(pairs, H: int, Hkv: int, shift: int = 0):
    """(q [B, S, H, 128] padded to the longest sequence, kc, vc [B, Hkv, C, 128],
    pos [B], lens [B], expect [B, S, H * 128]) in bf16: sequence b is row b of
    PC.exact_case(S_b, pos_b, ...); its padding query rows are NaN and its
    expected rows >= S_b zero.  An idle sequence has pos -1, len 0, NaN q and
    caches."""
    assert len(pairs) == PC.B
    S = max(prefill_tokens(p) for p in pairs)
    q = torch.full((PC.B, S, H, PC.HD), float("nan"), dtype=BF)
    kc = torch.full((PC.B, Hkv, PC.C, PC.HD), float("nan"), dtype=BF)
    vc = torch.full((PC.B, Hkv, PC.C, PC.HD), float("nan"), dtype=BF)
    expect = torch.zeros(PC.B, S, H * PC.HD, dtype=BF)
    pos, lens = [], []
    for b, pair in enumerate(pairs):
        if pair is None:
            pos.append(-1)
            lens.append(0)
            continue
        n, p = pair
        uq, uk, uv, _, ue = _prefill_uniform(n, p, H, Hkv, shift)
        q[b, :n], kc[b], vc[b], expect[b, :n] = uq[b], uk[b], uv[b], ue[b]
        pos.append(p)
        lens.append(n)
    return q, kc, vc, pos, lens, expect
