"""Shared cases and fixtures of the decode-attention tests
(tests/test_decode_attn_cpu.py, tests/test_gpu_decode_attn.py), all built on
the CPU in bf16.

k_decode_attn gives wave w of a workgroup the keys k0 + 64 w, += 512.  C = 1100
is the smallest cache at which, with nsplit = 1, wave 0 runs a full third
iteration (keys 1024..1087), wave 1 a partial third one (1088..1099) and all 8
waves a second one, so the online rescale inside a wave acts on a finite
running max.

* exact_case: the one-hot coding of prefill_cases with S = 1.  The target of
  (b, h) walks a list of wave, iteration and split edges; the expected output
  is one V row bit for bit.
* census_case: q = 0, so every weight is exactly 1 and l = L; V counts the keys
  per dimension, so one dropped or doubled key moves one dimension by >= 11 %.
* ramp_case: random data with a score ramp in dimension 0: the running max of
  the even heads rises by a few nats from one 512-key iteration to the next
  (corr is neither 0 nor 1), the odd heads see their max first.

Cache rows past the visible ones hold NaN: the kernel predicates both loads, so
nothing of them may reach the arithmetic.
"""
import torch

from prefill_cases import _codes

B, HD, C = 4, 128, 1100
HEADS = [(8, 2), (2, 2), (8, 1), (4, 2)]  # G = 4, 1, 8, 2
POSITIONS = [0, 62, 63, 64, 511, 512, 575, 1023, 1024, 1099]
NSPLITS = [None, 1, 2, 3, 8]
CENSUS_L = [1, 5, 63, 64, 65, 130, 512, 513, 1087, 1088, 1100]
RAMP_POSITIONS = [511, 512, 1023, 1024, 1099]
# the last visible key, then both sides of every 64-key wave step, 512-key
# iteration and split edge below C
BOUNDARY = [None, 0, 63, 64, 511, 512, 513, 575, 576, 1023, 1024, 1087, 1088]

BF = torch.bfloat16


def targets(pos: int, H: int, shift: int = 0) -> torch.Tensor:
    """Target key of query (b, h), [B, H]: BOUNDARY[(b H + h) % 13] (None: pos),
    clamped to pos, moved by `shift`."""
    n = (torch.arange(B).view(B, 1) * H + torch.arange(H).view(1, H)) % len(BOUNDARY)
    edge = torch.tensor([pos if e is None else e for e in BOUNDARY])
    return edge[n].clamp(max=pos) + shift


def exact_case(pos: int, H: int, Hkv: int, shift: int = 0):
    """(q [B, H, 128], kc, vc [B, Hkv, C, 128], t [B, H], expect [B, H * 128]) in
    bf16; expect = V[b, kvh, t].  Rows 0 .. pos + shift are coded, the rest NaN."""
    G = H // Hkv
    coded = pos + shift + 1
    assert coded <= C
    t = targets(pos, H, shift)
    j = torch.arange(C)
    d = torch.arange(HD)
    kc = torch.full((B, Hkv, C, HD), float("nan"))
    vc = torch.full((B, Hkv, C, HD), float("nan"))
    q = torch.zeros(B, H, HD)
    kcode, qcode = _codes(j, 8.0), _codes(t, 128.0)
    for b in range(B):
        for kvh in range(Hkv):
            dims = 8 * torch.arange(16) + (b + kvh) % 8
            krow = torch.zeros(C, HD)
            krow[:, dims] = kcode
            kc[b, kvh, :coded] = krow[:coded]
            vrow = ((7 * j[:, None] + 3 * d[None, :] + 1) % 251 - 125 + b + 2 * kvh).float()
            vc[b, kvh, :coded] = vrow[:coded]
            for gg in range(G):
                h = kvh * G + gg
                q[b, h, dims] = qcode[b, h]
    kvh_of = (torch.arange(H) // G).view(1, H).expand(B, H)
    expect = vc[torch.arange(B).view(B, 1).expand(B, H), kvh_of, t]  # [B, H, 128]
    q, kc, vc, expect = q.to(BF), kc.to(BF), vc.to(BF), expect.to(BF)
    assert torch.equal(expect.float(), expect.float().round())  # integers <= 256: exact in bf16
    return q, kc, vc, t, expect.reshape(B, H * HD)


def census_case(L: int, H: int, Hkv: int):
    """(q, kc, vc, expect [B, H * 128] fp64): expect[.., d] = 256 count_d / L with
    count_d = #{j < L : j % 128 == d}; rows >= L are NaN."""
    assert 1 <= L <= C
    g = torch.Generator().manual_seed(5 * L + H + Hkv)
    q = torch.zeros(B, H, HD)
    kc = torch.full((B, Hkv, C, HD), float("nan"))
    vc = torch.full((B, Hkv, C, HD), float("nan"))
    kc[:, :, :L] = torch.randn(B, Hkv, L, HD, generator=g)
    j = torch.arange(C)
    vrow = (j[:, None] % HD == torch.arange(HD)[None, :]).float() * 256
    vc[:, :, :L] = vrow[:L]
    count = vrow[:L].double().sum(0) / 256
    expect = (256 * count / L).repeat(H).expand(B, H * HD).contiguous()
    return q.to(BF), kc.to(BF), vc.to(BF), expect


def ramp_case(pos: int, H: int, Hkv: int, seed: int = 0):
    """(q, kc, vc) of random normal data with K[.., j, 0] = 16 j / L and
    q[b, h, 0] = +(8 + h) for even h, -(8 + h) for odd h; rows > pos are NaN."""
    L = pos + 1
    assert L <= C
    g = torch.Generator().manual_seed(1000 * seed + 3 * pos + 7 * H + Hkv)
    q = torch.randn(B, H, HD, generator=g)
    h = torch.arange(H)
    q[:, :, 0] = torch.where(h % 2 == 0, 8.0 + h, -(8.0 + h))
    kc = torch.full((B, Hkv, C, HD), float("nan"))
    vc = torch.full((B, Hkv, C, HD), float("nan"))
    kc[:, :, :L] = torch.randn(B, Hkv, L, HD, generator=g)
    kc[:, :, :L, 0] = 16.0 * torch.arange(L) / L
    vc[:, :, :L] = torch.randn(B, Hkv, L, HD, generator=g)
    return q.to(BF), kc.to(BF), vc.to(BF)


def scores64(q: torch.Tensor, kc: torch.Tensor, pos: int) -> torch.Tensor:
    """fp64 scaled scores of the visible keys, [B, H, pos + 1]."""
    Bq, H, hd = q.shape
    Hkv = kc.shape[1]
    qg = q.double().view(Bq, Hkv, H // Hkv, hd)
    return (qg @ kc[:, :, :pos + 1].double().transpose(-1, -2) * hd ** -0.5).view(Bq, H, pos + 1)


def ref64(q: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, pos: int) -> torch.Tensor:
    """fp64 attention of the bf16 inputs over rows 0..pos, [B, H * hd]."""
    Bq, H, hd = q.shape
    Hkv = kc.shape[1]
    w = torch.softmax(scores64(q, kc, pos), -1).view(Bq, Hkv, H // Hkv, pos + 1)
    return (w @ vc[:, :, :pos + 1].double()).reshape(Bq, H * hd)
