"""k_prefill_attn / k_qkv_rope_cache_prefill on the MI355X and the chunked
prefill of LlamaDecoder on them (csrc/hip/prefill_kernels.hip)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_cases as PC  # noqa: E402

from pbs_amd.models.llama import LlamaConfig, LlamaDecoder, apply_rope_ref, rope_tables  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

pytestmark = pytest.mark.gpu

B, HD, C = PC.B, PC.HD, PC.C
CASES = [(S, pos, H, Hkv) for (S, pos) in PC.SHAPES for (H, Hkv) in PC.HEADS]
CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


@pytest.mark.parametrize("S,pos,H,Hkv", CASES)
def test_exact_data_selects_the_target_value_row_bit_for_bit(S, pos, H, Hkv):
    """Every operand lane map (asymmetric V), the diagonal (head 0 targets the
    last visible key), the first key (head 1) and the online rescale (random
    targets: the max grows late for some rows, never for others), exactly."""
    q, kc, vc, t, expect = PC.exact_case(S, pos, H, Hkv)
    out = llm.prefill_attn(*_cuda(q, kc, vc), pos).cpu()
    assert out.shape == (B, S, H * HD) and out.dtype == torch.bfloat16
    bad = (out != expect).view(B, S, H, HD).any(-1).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong (b, s, h) rows, first {bad[:8].tolist()}"
    assert torch.equal(out.view(torch.int16), expect.view(torch.int16))


@pytest.mark.parametrize("S,pos,H,Hkv", CASES)
def test_first_masked_key_is_not_seen(S, pos, H, Hkv):
    """Every query targets key pos + s + 1, which is in the cache with its code:
    a mask one too loose returns that key's V row."""
    assert pos + S + 1 <= C  # the masked key exists in the cache
    q, kc, vc, t, leaked = PC.exact_case(S, pos, H, Hkv, shift=1)
    assert torch.equal(t[:, :, 0], (pos + 1 + torch.arange(S)).expand(B, S))
    out = llm.prefill_attn(*_cuda(q, kc, vc), pos).cpu().float()
    ref = llm.prefill_attn_ref(q, kc, vc, pos)
    assert not torch.equal(out, leaked.float())
    err, mag = (out - ref).abs().max().item(), ref.abs().max().item()
    print(f"first-masked-key S={S} pos={pos} H={H} Hkv={Hkv}: err {err:.4g} of {mag:.4g}")
    assert err < 2e-2 * mag


def _random_case(S, pos, H, Hkv, seed=0):
    g = torch.Generator().manual_seed(31 * S + pos + 7 * H + Hkv + 1000 * seed)
    q = torch.randn(B, S, H, HD, generator=g).bfloat16()
    kc = torch.randn(B, Hkv, C, HD, generator=g).bfloat16()
    vc = torch.randn(B, Hkv, C, HD, generator=g).bfloat16()
    return q, kc, vc


@pytest.mark.parametrize("S,pos,H,Hkv", CASES)
def test_random_data_against_the_reference(S, pos, H, Hkv):
    q, kc, vc = _random_case(S, pos, H, Hkv)
    ref = llm.prefill_attn_ref(q, kc, vc, pos)
    qd, kd, vd = _cuda(q, kc, vc)
    out = llm.prefill_attn(qd, kd, vd, pos)
    err, mag = (out.cpu().float() - ref).abs().max().item(), ref.abs().max().item()
    print(f"random S={S} pos={pos} H={H} Hkv={Hkv}: err {err:.4g} of {mag:.4g}")
    assert err < 2e-2 * mag
    if S == 1:
        dec = llm.decode_attn(qd.view(B, H, HD), kd, vd, torch.tensor([pos], dtype=torch.int32, device="cuda"))
        assert (dec.cpu().float().view(B, 1, H * HD) - ref).abs().max().item() < 2e-2 * mag
        assert (dec.float().view(B, 1, H * HD) - out.float()).abs().max().item() < 2e-2 * mag


@pytest.mark.parametrize("S,pos,H,Hkv", CASES)
def test_stale_rows_do_not_reach_the_output(S, pos, H, Hkv):
    """Rows >= pos + S hold finite garbage of an earlier request: two different
    fills give the same bits (and two equal calls do: no atomics)."""
    q, kc, vc = _cuda(*_random_case(S, pos, H, Hkv, seed=1))
    outs = []
    for fill in (3, 4, 4):
        g = torch.Generator().manual_seed(fill)
        n = C - (pos + S)
        if n:
            kc[:, :, pos + S:] = (torch.randn(B, Hkv, n, HD, generator=g) * 100).bfloat16().cuda()
            vc[:, :, pos + S:] = (torch.randn(B, Hkv, n, HD, generator=g) * 100).bfloat16().cuda()
        outs.append(llm.prefill_attn(q, kc, vc, pos))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


@pytest.mark.parametrize("H,Hkv", [(8, 2), (4, 1)])
@pytest.mark.parametrize("S,pos", [(1, 0), (65, 64), (150, 249)])
def test_qkv_rope_cache_prefill(S, pos, H, Hkv):
    g = torch.Generator().manual_seed(S + pos + H)
    cfg = LlamaConfig(dim=H * HD, n_heads=H, n_kv_heads=Hkv, max_seq=C)
    cos, sin = rope_tables(cfg, "cpu")
    qkv = torch.randn(B, S, (H + 2 * Hkv) * HD, generator=g).bfloat16()
    kc0 = torch.randn(B, Hkv, C, HD, generator=g).bfloat16()
    vc0 = torch.randn(B, Hkv, C, HD, generator=g).bfloat16()
    kc, vc = kc0.cuda(), vc0.cuda()
    q = llm.qkv_rope_cache_prefill(qkv.cuda(), cos.cuda(), sin.cuda(), pos, kc, vc, H).cpu()
    kc, vc = kc.cpu(), vc.cpu()
    nq, nkv = H * HD, Hkv * HD
    q_in = qkv[..., :nq].view(B, S, H, HD)
    k_in = qkv[..., nq:nq + nkv].view(B, S, Hkv, HD)
    v_in = qkv[..., nq + nkv:].view(B, S, Hkv, HD)
    q_ref = apply_rope_ref(q_in.float(), cos[pos:pos + S], sin[pos:pos + S])
    k_ref = apply_rope_ref(k_in.float(), cos[pos:pos + S], sin[pos:pos + S])
    assert q.shape == (B, S, H, HD)
    assert (q.float() - q_ref).abs().max().item() < 3e-2
    assert (kc[:, :, pos:pos + S].float() - k_ref.transpose(1, 2)).abs().max().item() < 3e-2
    assert torch.equal(vc[:, :, pos:pos + S], v_in.transpose(1, 2))
    for new, old in ((kc, kc0), (vc, vc0)):
        assert torch.equal(new[:, :, :pos], old[:, :, :pos]) and torch.equal(new[:, :, pos + S:], old[:, :, pos + S:])


def test_wrappers_refuse_what_the_kernels_cannot_do():
    q, kc, vc = _cuda(*_random_case(4, 0, 8, 2))
    with pytest.raises(ValueError):
        llm.prefill_attn(q, kc, vc, C - 3)
    with pytest.raises(ValueError):
        llm.prefill_attn(q[:, :, :6].contiguous(), kc, vc, 0)  # G = 3
    from pbs_amd.ops.kernels import _ptr, _stream, lib
    out = torch.empty(B, 4, 8 * HD, dtype=torch.bfloat16, device="cuda")
    assert lib().gpbs_hip_prefill_attn(_ptr(q), _ptr(kc), _ptr(vc), _ptr(out), B, 4, 8, 2, C, HD, C - 3, 0.1,
                                       _stream()) == -22
    assert lib().gpbs_hip_prefill_attn(_ptr(q), _ptr(kc), _ptr(vc), _ptr(out), B, 4, 6, 2, C, HD, 0, 0.1,
                                       _stream()) == -22
    assert lib().gpbs_hip_prefill_attn(_ptr(q), _ptr(kc), _ptr(vc), _ptr(out), B, 4, 8, 2, C, 64, 0, 0.1,
                                       _stream()) == -22
    assert lib().gpbs_hip_qkv_rope_cache_prefill(_ptr(q), _ptr(q), _ptr(q), _ptr(out), _ptr(kc), _ptr(vc), B, 4, 8, 2,
                                                 C, HD, C - 3, _stream()) == -22


@pytest.mark.parametrize("fp8", [True, False])
def test_model_prefill_attn_and_chunked_prefill_match_the_sdpa_decoder(fp8):
    kw = dict(batch=2, context=200, fp8=fp8)
    base = LlamaDecoder(CFG, **kw)
    state = base.model.state_dict()
    own, chunked = LlamaDecoder(CFG, prefill_attn=True, **kw), LlamaDecoder(CFG, prefill_attn=True, **kw)
    for d in (own, chunked):
        d.model.load_state_dict(state)
        if fp8:
            d.model.attach_fp8()
    tokens = torch.randint(0, CFG.vocab, (2, 150), generator=torch.Generator().manual_seed(5)).cuda()

    def last_logits(d, **k):
        seen = []
        fwd = d._forward

        def spy(*a, **b):
            r = fwd(*a, **b)
            if r is not None:
                seen.append(r[:, -1].float().clone())
            return r

        d._forward = spy
        try:
            tok = d.prefill(tokens, **k)
        finally:
            d._forward = fwd
        assert len(seen) == 1  # only the last chunk computes logits
        return tok, seen[0]

    _, lg0 = last_logits(base)
    _, lg1 = last_logits(own)
    tok2, lg2 = last_logits(chunked, chunk=64)
    for lg in (lg1, lg2):
        cos = torch.nn.functional.cosine_similarity(lg, lg0, dim=-1).min().item()
        print(f"fp8={fp8}: min cosine of the last-token logits {cos:.6f}")
        assert cos > 0.995
    for d in (own, chunked):
        for a, b_ in zip(d.cache[0], base.cache[0]):
            assert (a.float() - b_.float()).abs().max().item() < 1e-2
    assert chunked.pos == 150
    tok = tok2
    for _ in range(8):
        tok = chunked.decode_step(tok)
    assert chunked.pos == 158 and tok.shape == (2, 1)
