"""The per-sequence (_seq) forms of the four attention-block kernels on the
MI355X (csrc/hip/decode_kernels.hip, csrc/hip/prefill_kernels.hip): exact data
assembled per sequence from the uniform fixtures, and the uniform kernels at
each sequence's own position as the reference, bit for bit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as DC  # noqa: E402
import prefill_cases as PC  # noqa: E402
import ragged_cases as RC  # noqa: E402

from pbs_amd.models.llama import LlamaConfig, rope_tables  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

pytestmark = pytest.mark.gpu

HD = DC.HD
DECODE = [(tuple(s), H, Hkv) for s in RC.DECODE_SETS for (H, Hkv) in DC.HEADS]
PREFILL = [(pairs, H, Hkv) for pairs in RC.PREFILL_SETS for (H, Hkv) in PC.HEADS]


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ decode
def _check_decode(positions, H, Hkv, shift):
    B = DC.B
    q, kc, vc, t, expect = RC.decode_case(positions, H, Hkv, shift)
    qd, kd, vd = _cuda(q, kc, vc)
    pos_t = _i32(positions)
    for ns in DC.NSPLITS:
        out = llm.decode_attn_seq(qd, kd, vd, pos_t, ns)
        assert out.shape == (B, H * HD) and out.dtype == torch.bfloat16
        for b, p in enumerate(positions):
            if not RC.decode_active(p):
                assert not _bits(out[b]).any(), f"nsplit={ns}: idle sequence {b} (pos {p}) is not zero bits"
                continue
            # the reference is the existing kernel, run for the whole batch at this sequence's position
            uni = llm.decode_attn(qd, kd, vd, _i32([p]), ns)
            assert _same_bits(out[b], uni[b]), f"nsplit={ns}: sequence {b} at pos {p} differs from decode_attn"
            row, want = out[b].cpu().view(H, HD), expect[b].view(H, HD)
            if shift and p + 1 < DC.C:  # heads aimed at the first masked key must not get its V row
                hidden = t[b] == p + 1  # (b, h) = (0, 0) always is one; a sequence of few heads may have none
                same = (_bits(row) == _bits(want)).all(-1)
                assert hidden[0] or b, "the fixture aims head 0 of sequence 0 at the first masked key"
                assert not (same & hidden).any(), f"nsplit={ns}: sequence {b} sees key {p + 1}"
                assert same[~hidden].all()
            else:
                bad = (_bits(row) != _bits(want)).any(-1).nonzero().flatten().tolist()
                assert not bad, f"nsplit={ns}: sequence {b} at pos {p}: wrong heads {bad}, targets {t[b, bad].tolist()}"


@pytest.mark.parametrize("positions,H,Hkv", DECODE)
def test_decode_exact_data_per_sequence_bit_for_bit(positions, H, Hkv):
    """Active rows return their fixture's V row and the bits of decode_attn at
    their own position for every nsplit; idle rows (caches and q all NaN) are
    zero bits through the nsplit == 1 epilogue and the combine kernel."""
    _check_decode(positions, H, Hkv, shift=0)


@pytest.mark.parametrize("positions,H,Hkv", DECODE)
def test_decode_first_masked_key_is_not_seen_per_sequence(positions, H, Hkv):
    _check_decode(positions, H, Hkv, shift=1)


@pytest.mark.parametrize("H,Hkv", DC.HEADS)
def test_decode_positions_refilled_in_place(H, Hkv):
    """One position tensor, refilled long, short, long (the graph-captured step
    does this before every replay): the first and third results are equal bits,
    the second is the uniform kernel's at the short positions."""
    qd, kd, vd = _cuda(*DC.ramp_case(DC.C - 1, H, Hkv, seed=0))
    long_, short = [1099, 1023, 1024, 575], [0, 5, -1, 63]
    pos_t = _i32(long_)
    for ns in (None, 1, 3):
        outs = []
        for vals in (long_, short, long_):
            pos_t.copy_(_i32(vals))
            outs.append(llm.decode_attn_seq(qd, kd, vd, pos_t, ns))
        assert _same_bits(outs[0], outs[2]) and not _same_bits(outs[0], outs[1])
        for vals, out in ((long_, outs[0]), (short, outs[1])):
            for b, p in enumerate(vals):
                if p < 0:
                    assert not _bits(out[b]).any()
                else:
                    assert _same_bits(out[b], llm.decode_attn(qd, kd, vd, _i32([p]), ns)[b]), (ns, b, p)


def _tables(H, Hkv, C):
    return _cuda(*rope_tables(LlamaConfig(dim=H * HD, n_heads=H, n_kv_heads=Hkv, max_seq=C), "cpu"))


@pytest.mark.parametrize("positions", RC.DECODE_SETS)
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
def test_qkv_rope_cache_seq(positions, H, Hkv):
    B, C = DC.B, DC.C
    g = torch.Generator().manual_seed(sum(positions) + H)
    cos, sin = _tables(H, Hkv, C)
    qkv = torch.randn(B, 1, (H + 2 * Hkv) * HD, generator=g).bfloat16().cuda()
    kc0 = torch.randn(B, Hkv, C, HD, generator=g).bfloat16().cuda()
    vc0 = torch.randn(B, Hkv, C, HD, generator=g).bfloat16().cuda()
    kc, vc = kc0.clone(), vc0.clone()
    q = llm.qkv_rope_cache_seq(qkv, cos, sin, _i32(positions), kc, vc, H)
    assert q.shape == (B, H, HD)
    for b, p in enumerate(positions):
        if not RC.decode_active(p):
            assert not _bits(q[b]).any() and _same_bits(kc[b], kc0[b]) and _same_bits(vc[b], vc0[b])
            continue
        ku, vu = kc0.clone(), vc0.clone()
        qu = llm.qkv_rope_cache(qkv, cos, sin, _i32([p]), ku, vu, H)
        assert _same_bits(q[b], qu[b]) and _same_bits(kc[b], ku[b]) and _same_bits(vc[b], vu[b])
        rest = torch.arange(C, device="cuda") != p
        assert _same_bits(kc[b][:, rest], kc0[b][:, rest]) and _same_bits(vc[b][:, rest], vc0[b][:, rest])
        assert not _same_bits(kc[b, :, p], kc0[b, :, p]) and _same_bits(vc[b, :, p], qkv[b, 0, (H + Hkv) * HD:]
                                                                         .view(Hkv, HD))


# ------------------------------------------------------------------ prefill
def _alone(qd, kd, vd, b, n, p):
    """The uniform kernel on sequence b alone: its batch-1 slice with (S = n, pos = p)."""
    return llm.prefill_attn(qd[b:b + 1, :n].contiguous(), kd[b:b + 1], vd[b:b + 1], p)[0]


@pytest.mark.parametrize("pairs,H,Hkv", PREFILL)
def test_prefill_exact_data_per_sequence_bit_for_bit(pairs, H, Hkv):
    """Padding query rows and an idle sequence's caches are NaN: none of them is
    loaded.  Rows >= n_b are zero bits."""
    q, kc, vc, pos, lens, expect = RC.prefill_case(pairs, H, Hkv)
    qd, kd, vd = _cuda(q, kc, vc)
    out = llm.prefill_attn_seq(qd, kd, vd, _i32(pos), _i32(lens))
    assert out.shape == expect.shape and out.dtype == torch.bfloat16
    for b, pair in enumerate(pairs):
        n = RC.prefill_tokens(pair)
        assert not _bits(out[b, n:]).any(), f"sequence {b}: rows >= {n} are not zero bits"
        if n:
            assert _same_bits(out[b, :n], _alone(qd, kd, vd, b, n, pos[b])), f"sequence {b} differs from prefill_attn"
            bad = (_bits(out[b, :n].cpu()) != _bits(expect[b, :n])).view(n, H, HD).any(-1).nonzero()
            assert bad.numel() == 0, f"sequence {b}: {bad.shape[0]} wrong (s, h) rows, first {bad[:8].tolist()}"
    assert _same_bits(out.cpu(), expect)


@pytest.mark.parametrize("pairs,H,Hkv", PREFILL)
def test_prefill_stale_rows_past_each_sequence_do_not_reach_the_output(pairs, H, Hkv):
    """Rows > pos_b + n_b - 1 of each sequence's caches refilled with NaN, +-inf
    and finite garbage: not a bit changes, and equal calls give equal bits."""
    q, kc, vc, pos, lens, _ = RC.prefill_case(pairs, H, Hkv)
    qd, kd, vd = _cuda(q, kc, vc)
    pos_t, len_t = _i32(pos), _i32(lens)
    first = llm.prefill_attn_seq(qd, kd, vd, pos_t, len_t)
    assert _same_bits(first, llm.prefill_attn_seq(qd, kd, vd, pos_t, len_t))
    g = torch.Generator().manual_seed(3)
    for fill in (float("nan"), float("inf"), float("-inf"), None):
        for b, pair in enumerate(pairs):
            end = 0 if pair is None else pair[0] + pair[1]
            for c in (kd, vd):
                if fill is None:
                    c[b, :, end:] = (torch.randn(Hkv, PC.C - end, HD, generator=g) * 100).bfloat16().cuda()
                else:
                    c[b, :, end:] = fill
        assert _same_bits(first, llm.prefill_attn_seq(qd, kd, vd, pos_t, len_t)), f"fill {fill}"


def _rope_inputs(S, H, Hkv, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(PC.B, S, (H + 2 * Hkv) * HD, generator=g).bfloat16().cuda()
    kc0 = torch.randn(PC.B, Hkv, PC.C, HD, generator=g).bfloat16().cuda()
    vc0 = torch.randn(PC.B, Hkv, PC.C, HD, generator=g).bfloat16().cuda()
    return qkv, kc0, vc0


def _check_rope_prefill(qkv, kc0, vc0, pos, lens, n_want, H, Hkv):
    cos, sin = _tables(H, Hkv, PC.C)
    kc, vc = kc0.clone(), vc0.clone()
    q = llm.qkv_rope_cache_prefill_seq(qkv, cos, sin, _i32(pos), _i32(lens), kc, vc, H)
    assert q.shape == (PC.B, qkv.shape[1], H, HD)
    for b, n in enumerate(n_want):
        assert not _bits(q[b, n:]).any()
        if not n:
            assert _same_bits(kc[b], kc0[b]) and _same_bits(vc[b], vc0[b])
            continue
        ku, vu = kc0[b:b + 1].clone(), vc0[b:b + 1].clone()
        qu = llm.qkv_rope_cache_prefill(qkv[b:b + 1, :n].contiguous(), cos, sin, pos[b], ku, vu, H)
        assert _same_bits(q[b, :n], qu[0]) and _same_bits(kc[b], ku[0]) and _same_bits(vc[b], vu[0])
        for new, old in ((kc, kc0), (vc, vc0)):
            assert _same_bits(new[b, :, :pos[b]], old[b, :, :pos[b]])
            assert _same_bits(new[b, :, pos[b] + n:], old[b, :, pos[b] + n:])
            assert not _same_bits(new[b, :, pos[b]:pos[b] + n], old[b, :, pos[b]:pos[b] + n])
    return kc, vc, q


@pytest.mark.parametrize("pairs", RC.PREFILL_SETS)
@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
def test_qkv_rope_cache_prefill_seq(pairs, H, Hkv):
    S = max(RC.prefill_tokens(p) for p in pairs)
    qkv, kc0, vc0 = _rope_inputs(S, H, Hkv, seed=S + H)
    pos = [-1 if p is None else p[1] for p in pairs]
    lens = [RC.prefill_tokens(p) for p in pairs]
    _check_rope_prefill(qkv, kc0, vc0, pos, lens, lens, H, Hkv)


@pytest.mark.parametrize("H,Hkv", [(8, 2), (2, 2)])
def test_the_kernels_clamp_lengths_to_the_launch_and_to_the_cache(H, Hkv):
    """len > C - pos (10 rows left) and len > S: the kernels clamp n_b themselves,
    and pos >= C or len <= 0 is an idle sequence."""
    S, C = 64, PC.C
    qkv, kc0, vc0 = _rope_inputs(S, H, Hkv, seed=7)
    for pos, lens, n in (([C - 10, 0], [64, 1000], [10, 64]), ([C, 17], [5, -3], [0, 0])):
        assert [llm.seq_tokens(p, ln, S, C) for p, ln in zip(pos, lens)] == n
        kc, vc, q = _check_rope_prefill(qkv, kc0, vc0, pos, lens, n, H, Hkv)
        out = llm.prefill_attn_seq(q, kc, vc, _i32(pos), _i32(lens))
        for b in range(PC.B):
            assert not _bits(out[b, n[b]:]).any()
            if n[b]:
                assert _same_bits(out[b, :n[b]], _alone(q, kc, vc, b, n[b], pos[b]))


def test_library_refuses_null_vectors_and_shapes_the_kernels_cannot_do():
    from pbs_amd.ops.kernels import _ptr, _stream, lib
    L, B, C, S = lib(), PC.B, PC.C, 4
    bf = dict(dtype=torch.bfloat16, device="cuda")
    q, kc, vc = torch.zeros(B, S, 8, HD, **bf), torch.zeros(B, 2, C, HD, **bf), torch.zeros(B, 2, C, HD, **bf)
    out, ws = torch.zeros(B, S, 8 * HD, **bf), torch.zeros(B * 2 * 2 * 4 * (HD + 2), device="cuda")
    v, f = _i32([0] * B), torch.zeros(C, HD // 2, device="cuda")
    sc, st = 0.1, _stream()

    def pf(pos_t, len_t, H=8, hd=HD):
        return L.gpbs_hip_prefill_attn_seq(_ptr(q), _ptr(kc), _ptr(vc), _ptr(pos_t), _ptr(len_t), _ptr(out), B, S, H, 2,
                                           C, hd, sc, st)

    def dec(pos_t, H=8, hd=HD):
        return L.gpbs_hip_decode_attn_seq(_ptr(q), _ptr(kc), _ptr(vc), _ptr(pos_t), _ptr(out), _ptr(ws), 2, B, H, 2, C,
                                          hd, sc, st)

    assert pf(None, v) == -22 and pf(v, None) == -22 and pf(v, v, H=6) == -22 and pf(v, v, hd=64) == -22
    assert dec(None) == -22 and dec(v, H=6) == -22 and dec(v, hd=64) == -22
    assert L.gpbs_hip_qkv_rope_cache_seq(_ptr(q), _ptr(f), _ptr(f), None, _ptr(out), _ptr(kc), _ptr(vc), B, 8, 2, C, HD,
                                         st) == -22
    for pos_t, len_t in ((None, v), (v, None)):
        assert L.gpbs_hip_qkv_rope_cache_prefill_seq(_ptr(q), _ptr(f), _ptr(f), _ptr(pos_t), _ptr(len_t), _ptr(out),
                                                     _ptr(kc), _ptr(vc), B, S, 8, 2, C, HD, st) == -22
    assert pf(v, v) == 0 and dec(v) == 0  # the same calls with nothing wrong are accepted
    torch.cuda.synchronize()
