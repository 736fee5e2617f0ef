"""Shared cases and the exact-data fixture of the prefill-attention tests
(tests/test_prefill_attn_cpu.py, tests/test_gpu_prefill_attn.py).

The fixture makes softmax a one-hot selection, so the attention output is one
V row bit for bit and every operand lane map, the causal mask and the online
rescale are checked exactly.  All values are exact in bf16.

* key j carries the 16 bits of j as +-8 in dims 8 n + (b + kvh) % 8, n = 0..15;
* query (b, s, h) carries the bits of its target key t as +-128 in the same
  dims: the score of key j is (1024 / sqrt(128)) (16 - 2 hamming(j, t)), so the
  gap to any other key is a multiple of ~181 and its weight underflows to 0
  under any exp;
* V[b, kvh, j, d] = (7 j + 3 d + 1) % 251 - 125 + b + 2 kvh: asymmetric in j and
  d (a transposed or k-permuted PV product changes it), |V| <= 128;
* cache rows past the coded ones hold randn * 100 (stale data of an earlier
  request).
"""
import torch

B, HD, C = 2, 128, 400
SHAPES = [(1, 0), (1, 137), (7, 0), (63, 5), (64, 0), (65, 64), (129, 130), (200, 0), (150, 249)]
HEADS = [(8, 2), (2, 2), (8, 1), (4, 2)]


def _codes(idx: torch.Tensor, amp: float) -> torch.Tensor:
    """[...] int64 -> [..., 16] of +-amp from the low 16 bits."""
    bits = (idx.unsqueeze(-1) >> torch.arange(16)) & 1
    return (bits * 2 - 1).to(torch.float32) * amp


def targets(S: int, pos: int, H: int, shift: int = 0, seed: int = 0) -> torch.Tensor:
    """Target key of query (b, s, h), [B, S, H]: head 0 the diagonal pos + s (the
    last visible key), head 1 key 0, the others seeded random in [0, pos + s];
    all moved by `shift`."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * S + pos + H)
    diag = (pos + torch.arange(S)).view(1, S, 1).expand(B, S, H)
    t = (torch.rand(B, S, H, generator=g) * (diag + 1).float()).long().clamp(max=diag)
    t[:, :, 0] = diag[:, :, 0]
    if H > 1:
        t[:, :, 1] = 0
    return t + shift


def exact_case(S: int, pos: int, H: int, Hkv: int, shift: int = 0, stale_seed: int = 0):
    """(q [B, S, H, 128], kc, vc [B, Hkv, C, 128], t [B, S, H], expect [B, S, H * 128]) in bf16 on
    the CPU; expect = V[b, kvh, t].  Rows 0 .. pos + S - 1 + shift are coded, the rest stale."""
    G = H // Hkv
    coded = pos + S + shift
    assert coded <= C
    t = targets(S, pos, H, shift)
    j = torch.arange(C)
    d = torch.arange(HD)
    g = torch.Generator().manual_seed(77 + stale_seed)
    kc = torch.randn(B, Hkv, C, HD, generator=g) * 100
    vc = torch.randn(B, Hkv, C, HD, generator=g) * 100
    q = torch.zeros(B, S, H, HD)
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
                q[b, :, h][:, dims] = qcode[b, :, h]
    kvh_of = torch.arange(H) // G
    bi = torch.arange(B).view(B, 1, 1).expand(B, S, H)
    expect = vc[bi, kvh_of.view(1, 1, H).expand(B, S, H), t]  # [B, S, H, 128]
    bf = torch.bfloat16
    q, kc, vc, expect = q.to(bf), kc.to(bf), vc.to(bf), expect.to(bf)
    assert torch.equal(expect.float(), expect.float().round())  # integers <= 128: exact in bf16
    return q, kc, vc, t, expect.reshape(B, S, H * HD)
