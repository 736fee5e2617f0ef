"""Prefill attention with a cache-position-offset causal mask, and chunked
prefill of LlamaDecoder: everything that can be checked without a GPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_cases as PC  # noqa: E402

from pbs_amd.models.llama import PRESETS, LlamaConfig, LlamaDecoder  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)


def _sdpa_masked(q, kc, vc, pos):
    B, S, H, hd = q.shape
    L = pos + S
    mask = torch.arange(L)[None, :] <= pos + torch.arange(S)[:, None]
    o = F.scaled_dot_product_attention(q.transpose(1, 2), kc[:, :, :L], vc[:, :, :L], attn_mask=mask,
                                       enable_gqa=True)
    return o.transpose(1, 2).reshape(B, S, H * hd)


@pytest.mark.parametrize("H,Hkv", [(8, 2), (2, 2)])
@pytest.mark.parametrize("S,pos", [(1, 0), (1, 137), (7, 0), (65, 64), (150, 249)])
def test_ref_equals_sdpa_with_the_offset_mask(S, pos, H, Hkv):
    g = torch.Generator().manual_seed(S * 1000 + pos + H)
    q = torch.randn(2, S, H, 128, dtype=torch.float64, generator=g)
    kc = torch.randn(2, Hkv, 400, 128, dtype=torch.float64, generator=g)
    vc = torch.randn(2, Hkv, 400, 128, dtype=torch.float64, generator=g)
    out = llm.prefill_attn_ref(q, kc, vc, pos)
    assert out.dtype == torch.float64 and out.shape == (2, S, H * 128)
    torch.testing.assert_close(out, _sdpa_masked(q, kc, vc, pos))
    if (S, pos) == (65, 64):
        # why chunking needed a kernel of our own: is_causal with fewer queries
        # than keys aligns the mask top-left, which is not key <= pos + s
        L = pos + S
        wrong = F.scaled_dot_product_attention(q.transpose(1, 2), kc[:, :, :L], vc[:, :, :L], is_causal=True,
                                               enable_gqa=True).transpose(1, 2).reshape(2, S, H * 128)
        assert (out - wrong).abs().max() > 1e-3


def test_ref_returns_fp32_for_bf16_inputs():
    q = torch.randn(1, 3, 2, 16).bfloat16()
    kc, vc = torch.randn(1, 1, 9, 16).bfloat16(), torch.randn(1, 1, 9, 16).bfloat16()
    assert llm.prefill_attn_ref(q, kc, vc, 4).dtype == torch.float32


@pytest.mark.parametrize("H,Hkv", PC.HEADS)
@pytest.mark.parametrize("S,pos", PC.SHAPES)
def test_exact_fixture_selects_one_value_row(S, pos, H, Hkv):
    """Guards the fixture of the GPU test: the reference returns V[t] bit for bit."""
    q, kc, vc, t, expect = PC.exact_case(S, pos, H, Hkv)
    assert int(t.max()) <= pos + S - 1 and torch.equal(t[:, :, 0], (pos + torch.arange(S)).expand(PC.B, S))
    out = llm.prefill_attn_ref(q, kc, vc, pos)
    assert torch.equal(out, expect.float())


def _no_lib():
    raise AssertionError("the wrapper touched the library before validating")


def _attn_args(S=4, H=8, Hkv=2, hd=128, Cn=16, dtype=torch.bfloat16):
    return (torch.zeros(2, S, H, hd, dtype=dtype), torch.zeros(2, Hkv, Cn, hd, dtype=torch.bfloat16),
            torch.zeros(2, Hkv, Cn, hd, dtype=torch.bfloat16))


@pytest.mark.parametrize("case,match", [("hd64", "head_dim"), ("g3", "group size"), ("overrun", r"pos \+ S"),
                                        ("strided", "contiguous"), ("fp32", "bf16")])
def test_prefill_attn_rejects_bad_arguments_before_the_library(case, match, monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    pos = 0
    if case == "hd64":
        q, kc, vc = _attn_args(hd=64)
    elif case == "g3":
        q, kc, vc = _attn_args(H=6)
    elif case == "overrun":
        q, kc, vc = _attn_args()
        pos = 13  # 13 + 4 > 16
    elif case == "strided":
        q, kc, vc = _attn_args(S=8)
        q = q[:, ::2]
    else:
        q, kc, vc = _attn_args(dtype=torch.float32)
    with pytest.raises(ValueError, match=match):
        llm.prefill_attn(q, kc, vc, pos)


@pytest.mark.parametrize("case,match", [("hd64", "rope tables"), ("overrun", r"pos \+ S"), ("strided", "contiguous"),
                                        ("fp32", "bf16"), ("short_tables", "cover")])
def test_qkv_rope_cache_prefill_rejects_bad_arguments_before_the_library(case, match, monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    H, Hkv, hd, Cn, S, pos = 8, 2, 128, 16, 4, 0
    cos = torch.zeros(32, 64)
    qkv = torch.zeros(2, S, (H + 2 * Hkv) * hd, dtype=torch.bfloat16)
    kc = torch.zeros(2, Hkv, Cn, hd, dtype=torch.bfloat16)
    if case == "hd64":  # caches of head_dim 64 against tables for 128
        kc = torch.zeros(2, Hkv, Cn, 64, dtype=torch.bfloat16)
        qkv = torch.zeros(2, S, (H + 2 * Hkv) * 64, dtype=torch.bfloat16)
    elif case == "overrun":
        pos = 13
    elif case == "strided":
        qkv = torch.zeros(2, 2 * S, (H + 2 * Hkv) * hd, dtype=torch.bfloat16)[:, ::2]
    elif case == "fp32":
        qkv = qkv.float()
    else:
        cos, pos = torch.zeros(8, 64), 6  # tables of 8 rows, pos + S = 10 <= C
    with pytest.raises(ValueError, match=match):
        llm.qkv_rope_cache_prefill(qkv, cos, cos.clone(), pos, kc, kc.clone(), H)


def _decoder(prefill_attn, state=None):
    d = LlamaDecoder(CFG, batch=2, context=200, device="cpu", dtype=torch.float64, fused=False,
                     prefill_attn=prefill_attn)
    if state is not None:
        d.model.load_state_dict(state)
    return d


def test_chunked_prefill_matches_the_unchunked_and_the_sdpa_path():
    base = _decoder(False)
    state = base.model.state_dict()
    own, chunked = _decoder(True, state), _decoder(True, state)
    tokens = torch.randint(0, CFG.vocab, (2, 150), generator=torch.Generator().manual_seed(5))

    def last_logits(d, **kw):
        seen = {}
        head = d.model.lm_head
        hook = head.register_forward_hook(lambda m, i, o: seen.__setitem__("logits", o.detach().clone()))
        try:
            tok = d.prefill(tokens, **kw)
        finally:
            hook.remove()
        return tok, seen["logits"][:, -1]

    tok0, lg0 = last_logits(base)
    tok1, lg1 = last_logits(own)
    tok2, lg2 = last_logits(chunked, chunk=64)
    torch.testing.assert_close(lg1, lg0)
    torch.testing.assert_close(lg2, lg1)
    assert torch.equal(tok1, tok0) and torch.equal(tok2, tok0)
    assert base.pos == own.pos == chunked.pos == 150
    for (k0, v0), (k1, v1), (k2, v2) in zip(base.cache, own.cache, chunked.cache):
        torch.testing.assert_close(k1, k0)
        torch.testing.assert_close(v1, v0)
        torch.testing.assert_close(k2, k0)
        torch.testing.assert_close(v2, v0)


def test_prefill_iter_yields_the_tokens_done_and_returns_the_next_token():
    d = _decoder(True)
    tokens = torch.randint(0, CFG.vocab, (2, 150), generator=torch.Generator().manual_seed(6))
    it = d.prefill_iter(tokens, 64)
    done = []
    while True:
        try:
            done.append(next(it))
            assert d.pos == done[-1]
        except StopIteration as e:
            tok = e.value
            break
    assert done == [64, 128, 150]
    assert tok.shape == (2, 1) and torch.equal(tok, _decoder(True, d.model.state_dict()).prefill(tokens))


def test_chunk_needs_prefill_attn_and_prefill_attn_needs_head_dim_128():
    tokens = torch.zeros(2, 150, dtype=torch.long)
    with pytest.raises(ValueError, match="prefill_attn"):
        _decoder(False).prefill(tokens, chunk=64)
    with pytest.raises(ValueError, match="chunk"):
        _decoder(True).prefill(tokens, chunk=0)
    with pytest.raises(ValueError, match="head_dim"):
        LlamaDecoder(PRESETS["tiny"], batch=1, context=16, device="cpu", dtype=torch.float32, fused=False,
                     prefill_attn=True)
    with pytest.raises(ValueError, match="head_dim"):  # G = 3
        LlamaDecoder(LlamaConfig(dim=768, n_layers=1, n_heads=6, n_kv_heads=2, ffn_dim=256, vocab=64, max_seq=32),
                     batch=1, context=16, device="cpu", dtype=torch.float32, fused=False, prefill_attn=True)

