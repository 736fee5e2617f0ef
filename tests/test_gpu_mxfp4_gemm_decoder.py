"""LlamaDecoder(w4=True, w4_tiled=True) on the MI355X: every forward_fp8 call
runs its block linears on the tiled MXFP4 GEMM (k_gemm_mxfp4_tn), the static
step and its graph stay on the skinny kernel.  The model, its helpers and the
logits floor are those of tests/test_gpu_mxfp4_decoder.py; every decoder is
built from the same seed, so they share their bf16 weights."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_mxfp4_decoder as D  # noqa: E402

from pbs_amd.ops import llm  # noqa: E402

pytestmark = pytest.mark.gpu


def _tiled(**kw):
    return D._decoder(w4=True, w4_tiled=True, **kw)


def _count_gemms(monkeypatch):
    """The M of every gemm_mxfp4 launch that mxfp4_linear_q issues from here on."""
    calls, real = [], llm.gemm_mxfp4
    monkeypatch.setattr(llm, "gemm_mxfp4", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    return calls


def test_chunked_and_unchunked_prefill_give_equal_logits(monkeypatch):
    """A row's bits do not depend on the M it is launched in, so cutting the
    prefill into chunks of 64 changes nothing: logits, tokens and caches."""
    toks = D._tokens((2, 150), 7)
    whole, cut = (_tiled(batch=2, context=200, prefill_attn=True) for _ in range(2))
    assert whole.w4_tiled and cut.w4_tiled
    calls = _count_gemms(monkeypatch)
    t0, l0 = D._prefill_logits(whole, toks)
    assert calls == [300] * (4 * D.CFG.n_layers)  # one launch per block linear, none for the fp8 head
    del calls[:]
    t1, l1 = D._prefill_logits(cut, toks, chunk=64)
    assert sorted(set(calls)) == [2 * 22, 2 * 64] and len(calls) == 3 * 4 * D.CFG.n_layers
    print(f"chunked vs unchunked: min cosine {D._cosine(l0, l1):.6f}, largest difference {(l0 - l1).abs().max().item():.3g}")
    assert torch.equal(l0, l1) and torch.equal(t0, t1)
    for (k0, v0), (k1, v1) in zip(whole.cache, cut.cache):
        assert torch.equal(k0, k1) and torch.equal(v0, v1)


def test_a_ragged_slot_gets_the_same_bits_alone_and_in_a_batch_of_four(monkeypatch):
    toks = D._tokens((4, 150), 5)
    full, alone = (_tiled(batch=4, context=200, ragged=True, sampling=True) for _ in range(2))
    calls = _count_gemms(monkeypatch)
    tf, ta = full.prefill(toks, lens=[150, 37, 20, 64]), alone.prefill(toks, lens=[0, 37, 0, 0])
    assert calls
    assert alone.active == [False, True, False, False] and all(full.active)
    assert torch.equal(full.last_logits[1], alone.last_logits[1]) and torch.equal(tf[1], ta[1])


def _block_linears(d, toks, monkeypatch):
    """(name, xq, sx, weight, tiled4) of the four linears of layer 0 as decoder d ran them on toks."""
    names = {id(w): name for name, w in d.model.layers[0]._fp8.items()}
    seen, real = [], llm.linear_q

    def spy(xq, sx, w, **kw):
        if id(w) in names:
            seen.append((names[id(w)], xq.clone(), sx.clone(), w, kw.get("tiled4", False)))
        return real(xq, sx, w, **kw)

    monkeypatch.setattr(llm, "linear_q", spy)
    d.prefill(toks)
    monkeypatch.undo()
    assert [s[0] for s in seen] == ["qkv", "o", "w13", "w2"]
    return seen


def test_each_block_linear_stays_inside_the_derived_bound(monkeypatch):
    """The four linears of layer 0 on the quantised activations that a 40-token
    tiled prefill fed them, against the fp64 product of those codes and scales
    and the bound of mxfp4_cases.real_case: the tiled and the sliced kernel are
    both inside it, a weight with its rows rolled by 16 is not."""
    d = _tiled(batch=1, context=64, prefill_attn=True)
    for name, xq, sx, W, tiled4 in _block_linears(d, D._tokens((1, 40), 21), monkeypatch):
        assert tiled4 is True and isinstance(W, llm.Mxfp4Weight) and (W.N, W.K) == D.SHAPES[name]
        et = D._excess(llm.mxfp4_linear_q(xq, sx, W, tiled=True), xq, sx, W)
        es = D._excess(llm.mxfp4_linear_q(xq, sx, W), xq, sx, W)
        rolled = llm.Mxfp4Weight.from_quantised(W.codes.roll(16, 0), W.scales.roll(16, 0))
        bad = D._excess(llm.mxfp4_linear_q(xq, sx, rolled, tiled=True), xq, sx, W)
        print(f"layer 0 {name} [{W.N}, {W.K}] x {xq.numel() // W.K} rows: fraction of the bound tiled {et:.3f}, "
              f"sliced {es:.3f}, mis-wired tiled {bad:.3g}")
        assert et <= 1 and es <= 1 and bad > 1


def test_tiled_logits_track_the_sliced_w4_decoder():
    """The two decoders multiply the same numbers and differ only in the fp32
    accumulation order of the block linears: the last-token logits after a
    40-token prefill stay above the project's floor for that kind of pair."""
    kw = dict(batch=1, context=64, prefill_attn=True)
    tiled, sliced = _tiled(**kw), D._decoder(w4=True, **kw)
    for seed in (21, 22, 23):
        toks = D._tokens((1, 40), seed)
        lt, ls = D._prefill_logits(tiled, toks)[1], D._prefill_logits(sliced, toks)[1]
        cos = D._cosine(lt, ls)
        print(f"seed {seed}: w4_tiled vs w4 cosine {cos:.6f}, bit-equal {torch.equal(lt, ls)}")
        assert cos >= D.LOGITS_FLOOR, (seed, cos)


def test_graph_steps_after_a_tiled_prefill_equal_the_static_step_run_eagerly(monkeypatch):
    toks = D._tokens((4, 12), 0)
    ds, dg = _tiled(batch=4, context=64, static=True), _tiled(batch=4, context=64, graph=True)
    calls = _count_gemms(monkeypatch)
    a, b = ds.prefill(toks), dg.prefill(toks)
    assert len(calls) == 2 * 4 * D.CFG.n_layers and set(calls) == {48}
    assert torch.equal(a, b)
    del calls[:]
    for _ in range(4):
        a, b = ds.decode_step(a), dg.decode_step(a)
        assert torch.equal(a, b)
    assert not calls  # the static step and its graph run the skinny kernel
    assert dg._g is not None and dg.pos == ds.pos == 16
