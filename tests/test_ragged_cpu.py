"""Per-sequence KV-cache positions: the reference, the assembled fixtures, the
wrappers' refusals and the ragged LlamaDecoder on its eager path.  Everything
that can be checked without a GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as DC  # noqa: E402
import prefill_cases as PC  # noqa: E402
import ragged_cases as RC  # noqa: E402

from pbs_amd.models.llama import LlamaConfig, LlamaDecoder  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)


# ------------------------------------------------------------------ the reference and the fixtures
def test_attn_seq_ref_is_prefill_attn_ref_per_sequence_and_zero_past_the_length():
    g = torch.Generator().manual_seed(11)
    B, S, H, Hkv, Cn, hd = 4, 40, 4, 2, 64, 16
    q = torch.randn(B, S, H, hd, dtype=torch.float64, generator=g)
    kc = torch.randn(B, Hkv, Cn, hd, dtype=torch.float64, generator=g)
    vc = torch.randn(B, Hkv, Cn, hd, dtype=torch.float64, generator=g)
    # full length; clamped by S; clamped by C - pos (64 - 50 = 14); idle by pos, by len
    for pos, lens, n in (([0, 3, 50, 20], [40, 99, 30, 5], [40, 40, 14, 5]),
                         ([-1, 64, 7, 0], [10, 10, 0, 1], [0, 0, 0, 1])):
        out = llm.attn_seq_ref(q, kc, vc, pos, lens)
        assert out.dtype == torch.float64 and out.shape == (B, S, H * hd)
        for b in range(B):
            assert llm.seq_tokens(pos[b], lens[b], S, Cn) == n[b]
            assert not out[b, n[b]:].any()
            if n[b]:
                one = llm.prefill_attn_ref(q[b:b + 1, :n[b]], kc[b:b + 1], vc[b:b + 1], pos[b])
                torch.testing.assert_close(out[b:b + 1, :n[b]], one)
        assert torch.equal(out, llm.attn_seq_ref(q, kc, vc, torch.tensor(pos), torch.tensor(lens, dtype=torch.int32)))
    assert llm.attn_seq_ref(q.float(), kc.float(), vc.float(), pos, lens).dtype == torch.float32
    with pytest.raises(ValueError, match="batch"):
        llm.attn_seq_ref(q, kc, vc, [0, 0, 0], [1, 1, 1, 1])


@pytest.mark.parametrize("H,Hkv", DC.HEADS)
@pytest.mark.parametrize("positions", RC.DECODE_SETS)
def test_decode_fixture_selects_the_expected_value_rows(positions, H, Hkv):
    q, kc, vc, t, expect = RC.decode_case(positions, H, Hkv)
    active = [RC.decode_active(p) for p in positions]
    for b, p in enumerate(positions):
        if active[b]:
            assert 0 <= int(t[b].min()) and int(t[b].max()) <= p
            assert torch.isfinite(kc[b, :, :p + 1].float()).all() and torch.isnan(kc[b, :, p + 1:].float()).all()
        else:
            assert torch.isnan(kc[b].float()).all() and torch.isnan(vc[b].float()).all() and not expect[b].any()
    out = llm.attn_seq_ref(q.view(DC.B, 1, H, DC.HD), kc, vc, positions, [int(a) for a in active])
    assert torch.equal(out.view(DC.B, H * DC.HD), expect.float())
    # the shifted fixture aims every sequence that has a row pos + 1 at it
    _, _, _, t1, _ = RC.decode_case(positions, H, Hkv, shift=1)
    for b, p in enumerate(positions):
        if active[b]:
            assert torch.equal(t1[b], t[b] + (1 if p + 1 < DC.C else 0))


def test_decode_sets_hold_both_kinds_of_idle_sequence_and_the_edges():
    flat = [p for s in RC.DECODE_SETS for p in s]
    assert -1 in flat and DC.C in flat and DC.C - 1 in flat and 0 in flat
    assert all(len(s) == DC.B for s in RC.DECODE_SETS)
    assert {p for p in flat if RC.decode_active(p)} <= set(DC.POSITIONS) | {5}


@pytest.mark.parametrize("H,Hkv", PC.HEADS)
@pytest.mark.parametrize("pairs", RC.PREFILL_SETS)
def test_prefill_fixture_selects_the_expected_value_rows(pairs, H, Hkv):
    q, kc, vc, pos, lens, expect = RC.prefill_case(pairs, H, Hkv)
    S = q.shape[1]
    assert S == max(RC.prefill_tokens(p) for p in pairs)
    for b, pair in enumerate(pairs):
        assert pair is None or pair in PC.SHAPES
        n = RC.prefill_tokens(pair)
        assert torch.isnan(q[b, n:].float()).all() and torch.isfinite(q[b, :n].float()).all()
        if pair is None:
            assert pos[b] == -1 and lens[b] == 0 and torch.isnan(kc[b].float()).all()
    out = llm.attn_seq_ref(q, kc, vc, pos, lens)
    assert torch.equal(out, expect.float())
    for b, pair in enumerate(pairs):
        assert not expect[b, RC.prefill_tokens(pair):].any()


# ------------------------------------------------------------------ validation before the library
def _no_lib():
    raise AssertionError("the wrapper touched the library before validating")


BAD_VECTORS = ["one", "b_plus_1", "int64", "cpu", "strided"]


def _vector(case, B):
    if case == "one":
        return torch.zeros(1, dtype=torch.int32), "exactly B"
    if case == "b_plus_1":
        return torch.zeros(B + 1, dtype=torch.int32), "exactly B"
    if case == "int64":
        return torch.zeros(B, dtype=torch.int64), "int32"
    if case == "cpu":  # every other property is as good as it can be without a GPU
        return torch.zeros(B, dtype=torch.int32), "must be a CUDA tensor"
    t = torch.zeros(2 * B, dtype=torch.int32)[::2]
    assert t.numel() == B and not t.is_contiguous()
    return t, "contiguous"


def _caches(B=2, Hkv=2, Cn=16, hd=128):
    return torch.zeros(B, Hkv, Cn, hd, dtype=torch.bfloat16), torch.zeros(B, Hkv, Cn, hd, dtype=torch.bfloat16)


@pytest.mark.parametrize("case", BAD_VECTORS)
def test_decode_wrappers_reject_a_bad_position_vector_before_the_library(case, monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    kc, vc = _caches()
    pos_t, match = _vector(case, 2)
    with pytest.raises(ValueError, match=f"pos_t.*{match}"):
        llm.decode_attn_seq(torch.zeros(2, 8, 128, dtype=torch.bfloat16), kc, vc, pos_t)
    qkv = torch.zeros(2, 1, (8 + 4) * 128, dtype=torch.bfloat16)
    cos = torch.zeros(16, 64)
    with pytest.raises(ValueError, match=f"pos_t.*{match}"):
        llm.qkv_rope_cache_seq(qkv, cos, cos.clone(), pos_t, kc, vc, 8)


@pytest.mark.parametrize("which,case", [("pos_t", c) for c in BAD_VECTORS]
                         + [("len_t", c) for c in BAD_VECTORS if c != "cpu"])
def test_prefill_wrappers_reject_a_bad_position_or_length_vector_before_the_library(which, case, monkeypatch):
    """Shape, dtype and strides of both vectors are checked before either's device:
    without a GPU the good one of the pair cannot be a CUDA tensor."""
    monkeypatch.setattr(llm, "lib", _no_lib)
    kc, vc = _caches()
    bad, match = _vector(case, 2)
    good = torch.zeros(2, dtype=torch.int32)
    pos_t, len_t = (bad, good) if which == "pos_t" else (good, bad)
    with pytest.raises(ValueError, match=f"{which}.*{match}"):
        llm.prefill_attn_seq(torch.zeros(2, 4, 8, 128, dtype=torch.bfloat16), kc, vc, pos_t, len_t)
    qkv = torch.zeros(2, 4, (8 + 4) * 128, dtype=torch.bfloat16)
    cos = torch.zeros(16, 64)
    with pytest.raises(ValueError, match=f"{which}.*{match}"):
        llm.qkv_rope_cache_prefill_seq(qkv, cos, cos.clone(), pos_t, len_t, kc, vc, 8)


@pytest.mark.parametrize("case,match", [("hd64", "head_dim"), ("g3", "group size"), ("strided", "contiguous"),
                                        ("fp32", "bf16"), ("s_over_c", r"pos \+ S")])
def test_prefill_attn_seq_keeps_the_shape_checks_of_prefill_attn(case, match, monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    bf, v = torch.bfloat16, torch.zeros(2, dtype=torch.int32)
    q, (kc, vc) = torch.zeros(2, 4, 8, 128, dtype=bf), _caches()
    if case == "hd64":
        q, (kc, vc) = torch.zeros(2, 4, 8, 64, dtype=bf), _caches(hd=64)
    elif case == "g3":
        q = torch.zeros(2, 4, 6, 128, dtype=bf)
    elif case == "strided":
        q = torch.zeros(2, 8, 8, 128, dtype=bf)[:, ::2]
    elif case == "fp32":
        q = q.float()
    else:
        q = torch.zeros(2, 17, 8, 128, dtype=bf)  # the launch is sized for S: S <= C
    with pytest.raises(ValueError, match=match):
        llm.prefill_attn_seq(q, kc, vc, v, v)


@pytest.mark.parametrize("case,match", [("g3", "group size"), ("hd64", "128"), ("q_shape", r"must be \[B, H, 128\]"),
                                        ("nsplit0", "nsplit"), ("fp32_kc", "kc must be bf16")])
def test_decode_attn_seq_keeps_the_shape_checks_of_decode_attn(case, match, monkeypatch):
    monkeypatch.setattr(llm, "lib", _no_lib)
    bf, v, nsplit = torch.bfloat16, torch.zeros(2, dtype=torch.int32), None
    q, (kc, vc) = torch.zeros(2, 8, 128, dtype=bf), _caches()
    if case == "g3":
        q = torch.zeros(2, 6, 128, dtype=bf)
    elif case == "hd64":
        q, (kc, vc) = torch.zeros(2, 8, 64, dtype=bf), _caches(hd=64)
    elif case == "q_shape":
        q = torch.zeros(3, 8, 128, dtype=bf)
    elif case == "nsplit0":
        nsplit = 0
    else:
        kc = kc.float()
    with pytest.raises(ValueError, match=match):
        llm.decode_attn_seq(q, kc, vc, v, nsplit)


# ------------------------------------------------------------------ the ragged decoder, eager path, fp64
CONTEXT = 200
PROMPTS = torch.randint(0, CFG.vocab, (3, 150), generator=torch.Generator().manual_seed(5))


def _decoder(batch, state=None, **kw):
    d = LlamaDecoder(CFG, batch=batch, context=CONTEXT, device="cpu", dtype=torch.float64, fused=False, **kw)
    if state is not None:
        d.model.load_state_dict(state)
    return d


def _spy(d, call):
    """call() with d._forward recorded: the last-token logits of every call that
    computed some."""
    seen, fwd = [], d._forward

    def spy(*a, **k):
        r = fwd(*a, **k)
        if r is not None:
            seen.append(r[:, -1].clone())
        return r

    d._forward = spy
    try:
        out = call()
    finally:
        d._forward = fwd
    return out, seen


@pytest.fixture(scope="module")
def state():
    return _decoder(1).model.state_dict()


@pytest.fixture(scope="module")
def alone(state):
    """Every prompt on a batch-1 uniform decoder of the same weights: next token,
    last-token logits, caches, and four greedy steps.  Computed once, left unchanged."""
    res = {}
    for b, n in ((0, 150), (1, 37), (2, 64)):
        d = _decoder(1, state, prefill_attn=True)
        tok, seen = _spy(d, lambda: d.prefill(PROMPTS[b:b + 1, :n]))
        cache = [(k[0, :, :n].clone(), v[0, :, :n].clone()) for k, v in d.cache]
        steps, t = [], tok
        for _ in range(4):
            t = d.decode_step(t)
            steps.append(int(t))
        res[b] = dict(tok=int(tok), logits=seen[-1][0], cache=cache, steps=steps)
    return res


def _check_slot(d, b, n, ref):
    for (k, v), (rk, rv) in zip(d.cache, ref["cache"]):
        torch.testing.assert_close(k[b, :, :n], rk)
        torch.testing.assert_close(v[b, :, :n], rv)


@pytest.mark.parametrize("lens", [[150, 37, 64], [150, 0, 64]])
def test_ragged_prefill_and_decode_match_a_batch_1_decoder_per_sequence(lens, state, alone):
    d = _decoder(3, state, ragged=True)
    assert d.prefill_attn and not any(d.active)
    marker = [(k[1].clone().fill_(3.25), v[1].clone().fill_(-1.5)) for k, v in d.cache]
    if not lens[1]:  # the idle slot's cache rows hold a marker: nothing may write them
        for (k, v), (mk, mv) in zip(d.cache, marker):
            k[1], v[1] = mk, mv
    tok, seen = _spy(d, lambda: d.prefill(PROMPTS, lens=lens))
    assert len(seen) == 1 and tok.shape == (3, 1)
    assert d.pos_b == [n if n else -1 for n in lens] and d.active == [n > 0 for n in lens] and d.pos == 150
    for b, n in enumerate(lens):
        if not n:
            assert int(tok[b]) == 0
            continue
        torch.testing.assert_close(seen[0][b], alone[b]["logits"])
        assert int(tok[b]) == alone[b]["tok"]
        _check_slot(d, b, n, alone[b])
    t = tok
    for i in range(4):
        t = d.decode_step(t)
        assert t.shape == (3, 1) and 0 <= int(t.min()) and int(t.max()) < CFG.vocab
        for b, n in enumerate(lens):
            if n:
                assert int(t[b]) == alone[b]["steps"][i], (b, i)
    assert d.pos_b == [n + 4 if n else -1 for n in lens] and d.pos == 154
    if not lens[1]:
        for (k, v), (mk, mv) in zip(d.cache, marker):
            assert torch.equal(k[1], mk) and torch.equal(v[1], mv)


def test_admit_fills_an_idle_slot_and_leaves_the_others_alone(state, alone):
    d = _decoder(3, state, ragged=True)
    tok = d.prefill(PROMPTS, lens=[150, 0, 64])
    tok = d.decode_step(tok)
    before = [(k.clone(), v.clone()) for k, v in d.cache]
    with pytest.raises(ValueError, match="slot 0 is active"):
        d.admit(0, PROMPTS[1, :37])
    with pytest.raises(ValueError, match="context"):
        d.admit(1, torch.zeros(CONTEXT + 1, dtype=torch.long))
    new = d.admit(1, PROMPTS[1, :37])
    assert new.shape == (1, 1) and int(new) == alone[1]["tok"]
    assert d.pos_b == [151, 37, 65] and d.active == [True] * 3
    for (k, v), (k0, v0) in zip(d.cache, before):
        for b in (0, 2):
            assert torch.equal(k[b], k0[b]) and torch.equal(v[b], v0[b])
    _check_slot(d, 1, 37, alone[1])
    t = torch.cat([tok[0:1], new, tok[2:3]])
    for i in range(2):
        t = d.decode_step(t)
        assert int(t[1]) == alone[1]["steps"][i] and int(t[0]) == alone[0]["steps"][i + 1]


def test_admit_iter_yields_the_tokens_done_and_returns_the_token_of_admit(state, alone):
    d = _decoder(3, state, ragged=True)
    d.prefill(PROMPTS, lens=[0, 37, 64])
    it = d.admit_iter(0, PROMPTS[0:1], 64)
    done = []
    while True:
        try:
            done.append(next(it))
            assert not d.active[0] and d.pos_b[0] == -1  # idle until the last chunk is in
        except StopIteration as e:
            tok = e.value
            break
    assert done == [64, 128, 150] and d.pos_b == [150, 37, 64] and d.active[0]
    assert int(tok) == alone[0]["tok"]
    other = _decoder(3, state, ragged=True)
    other.prefill(PROMPTS, lens=[0, 37, 64])
    assert torch.equal(other.admit(0, PROMPTS[0]), tok)
    other.release(0)
    assert torch.equal(other.admit(0, PROMPTS[0], chunk=64), tok)
    _check_slot(d, 0, 150, alone[0])


def test_release_makes_a_slot_idle_and_decode_writes_nothing_to_it(state):
    d = _decoder(3, state, ragged=True)
    tok = d.prefill(PROMPTS, lens=[150, 37, 64])
    d.release(1)
    assert d.pos_b == [150, -1, 64] and d.active == [True, False, True] and d.pos == 150
    before = [(k[1].clone(), v[1].clone()) for k, v in d.cache]
    for _ in range(2):
        tok = d.decode_step(tok)
    for (k, v), (k0, v0) in zip(d.cache, before):
        assert torch.equal(k[1], k0) and torch.equal(v[1], v0)
    assert d.pos_b == [152, -1, 66]


def test_errors_of_the_ragged_interface(state):
    plain = _decoder(3, state, prefill_attn=True)
    with pytest.raises(ValueError, match="ragged"):
        plain.prefill(PROMPTS, lens=[150, 37, 64])
    with pytest.raises(ValueError, match="ragged"):
        plain.admit(0, PROMPTS[0])
    d = _decoder(3, state, ragged=True)
    with pytest.raises(ValueError, match="chunk"):
        d.prefill(PROMPTS, lens=[150, 37, 64], chunk=64)
    with pytest.raises(ValueError, match="lens"):
        d.prefill(PROMPTS, lens=[150, 37])
    with pytest.raises(ValueError, match="lens"):
        d.prefill(PROMPTS, lens=[151, 37, 64])
    # a slot that reaches the context has to be released: no sliding window
    full = torch.randint(0, CFG.vocab, (3, CONTEXT), generator=torch.Generator().manual_seed(9))
    tok = d.prefill(full, lens=[CONTEXT - 1, 5, 0])
    tok = d.decode_step(tok)
    assert d.pos_b == [CONTEXT, 6, -1]
    with pytest.raises(ValueError, match="slot 0"):
        d.decode_step(tok)
    d.release(0)
    d.decode_step(tok)
    assert d.pos_b == [-1, 7, -1]
    with pytest.raises(ValueError, match="head_dim"):  # G = 3
        LlamaDecoder(LlamaConfig(dim=768, n_layers=1, n_heads=6, n_kv_heads=2, ffn_dim=256, vocab=64, max_seq=32),
                     batch=1, context=16, device="cpu", dtype=torch.float32, fused=False, ragged=True)
    with pytest.raises(ValueError, match="fused"):
        LlamaDecoder(CFG, batch=1, context=16, device="cpu", dtype=torch.float32, fused=True, ragged=True)


def test_without_the_flag_the_decoder_is_the_uniform_one(state):
    d = _decoder(2, state)
    assert not d.ragged and not d.prefill_attn
    tok = d.prefill(PROMPTS[:2, :40])
    assert d.pos == 40 and tok.shape == (2, 1)
    nxt = d.decode_step(tok)
    assert d.pos == 41 and d.pos_b == [-1, -1] and d.active == [False, False]  # the ragged state is not kept
    # a ragged decoder given a uniform prompt (no lens): every slot active at its end, same tokens
    r = _decoder(2, state, ragged=True)
    assert torch.equal(r.prefill(PROMPTS[:2, :40]), tok) and r.pos_b == [40, 40] and r.active == [True, True]
    assert torch.equal(r.decode_step(tok), nxt) and r.pos_b == [41, 41] and r.pos == 41
    r = _decoder(2, state, ragged=True)
    assert torch.equal(r.prefill(PROMPTS[:2, :40], chunk=16), tok) and r.pos_b == [40, 40]
