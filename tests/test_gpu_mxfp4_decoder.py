"""LlamaDecoder(w4=True) on the MI355X: MXFP4 block linears under the static and
graph-captured step, ragged batches and chunked prefill, and against its oracle
w4="emulate" (the stock fp8 kernels over exact e4m3 copies of the MX weights).
Every decoder of one configuration is built from the same seed, so they share
their bf16 weights."""
import pytest
import torch

from pbs_amd.models.llama import LlamaConfig, LlamaDecoder
from pbs_amd.ops import llm

pytestmark = pytest.mark.gpu

CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)
HD = CFG.head_dim
SHAPES = {"qkv": ((CFG.n_heads + 2 * CFG.n_kv_heads) * HD, CFG.dim), "o": (CFG.dim, CFG.n_heads * HD),
          "w13": (2 * CFG.ffn_dim, CFG.dim), "w2": (CFG.dim, CFG.ffn_dim)}


def _decoder(**kw):
    return LlamaDecoder(CFG, fp8=True, **kw)


def _tokens(shape, seed):
    return torch.randint(0, CFG.vocab, shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _prefill_logits(d, tokens, **kw):
    """(next tokens, fp32 last-token logits) of d.prefill(tokens, **kw)."""
    seen, fwd = [], d._forward

    def spy(*a, **k):
        r = fwd(*a, **k)
        if r is not None:
            seen.append(r[:, -1].float().clone())
        return r

    d._forward = spy
    try:
        tok = d.prefill(tokens, **kw)
    finally:
        d._forward = fwd
    assert len(seen) == 1
    return tok, seen[0]


def _cosine(a, b):
    return torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=-1).min().item()


def test_attach_mxfp4_packs_the_four_block_weights_and_keeps_the_head_fp8():
    d = _decoder(batch=1, context=64, w4=True)
    assert isinstance(d.model._fp8_head, llm.Fp8Weight)
    for layer in d.model.layers:
        assert sorted(layer._fp8) == sorted(SHAPES)
        for name, (N, K) in SHAPES.items():
            w = layer._fp8[name]
            assert isinstance(w, llm.Mxfp4Weight) and (w.N, w.K) == (N, K)
            assert w.qs.is_cuda and w.ss.is_cuda and w.qs.dtype == w.ss.dtype == torch.uint8
            assert w.nbytes() == (K // 2 + K // 32) * N == w.qs.numel() + w.ss.numel()
    # the packed weight is the quantiser's output on the concatenated bf16 weights
    blk = d.model.layers[1]
    c, s = llm.mxfp4_quant_ref(torch.cat([blk.w1.weight, blk.w3.weight], 0))
    assert torch.equal(blk._fp8["w13"].codes, c) and torch.equal(blk._fp8["w13"].scales, s)


def test_graph_step_is_bit_equal_to_the_static_step_run_eagerly():
    toks = _tokens((4, 12), 0)
    ds, dg = _decoder(batch=4, context=64, static=True, w4=True), _decoder(batch=4, context=64, graph=True, w4=True)
    a, b = ds.prefill(toks), dg.prefill(toks)
    assert torch.equal(a, b)
    for _ in range(8):
        a, b = ds.decode_step(a), dg.decode_step(a)
        assert torch.equal(a, b)
    assert dg._g is not None and dg.pos == ds.pos == 20


def test_a_ragged_slot_gets_the_same_bits_alone_and_in_a_batch_of_four():
    """Slot 1 with the three other slots active or idle: bit-equal last-token
    logits after the ragged prefill and after each of 4 static decode steps."""
    toks = _tokens((4, 150), 5)
    full = _decoder(batch=4, context=200, ragged=True, sampling=True, w4=True)
    alone = _decoder(batch=4, context=200, ragged=True, sampling=True, w4=True)
    tf, ta = full.prefill(toks, lens=[150, 37, 20, 64]), alone.prefill(toks, lens=[0, 37, 0, 0])
    assert alone.active == [False, True, False, False] and all(full.active)
    assert torch.equal(full.last_logits[1], alone.last_logits[1]) and torch.equal(tf[1], ta[1])
    for step in range(4):
        tf, ta = full.decode_step(tf), alone.decode_step(ta)
        assert torch.equal(full.last_logits[1], alone.last_logits[1]), f"step {step}"
        assert torch.equal(tf[1], ta[1])
    assert full.pos_b[1] == alone.pos_b[1] == 41


def test_chunked_and_unchunked_prefill_give_equal_logits():
    toks = _tokens((2, 150), 7)
    whole, cut = (_decoder(batch=2, context=200, prefill_attn=True, w4=True) for _ in range(2))
    t0, l0 = _prefill_logits(whole, toks)
    t1, l1 = _prefill_logits(cut, toks, chunk=64)
    print(f"chunked vs unchunked: min cosine {_cosine(l0, l1):.6f}, largest difference {(l0 - l1).abs().max().item():.3g}")
    assert torch.equal(l0, l1) and torch.equal(t0, t1)
    for (k0, v0), (k1, v1) in zip(whole.cache, cut.cache):
        assert torch.equal(k0, k1) and torch.equal(v0, v1)


# Floor of the w4-versus-emulate cosine of the logits, whatever the yardstick says.  From the README's record of this
# kind of model, not from a w4 run: two stock fp8 paths that differ only in summation order are at 0.972 of each
# other at llama3-8b size, fp8 against bf16 weights (different numbers, not a different order) at 0.76, and a
# mis-wired weight is near 0.  0.9 separates the first from the other two.
LOGITS_FLOOR = 0.9


def oracle_cosines(seeds=(21, 22, 23), S=40):
    """(w4 vs emulate, sliced vs tiled stock fp8) cosines of the last-token logits
    after an S-token prefill, one pair per token seed."""
    kw = dict(batch=1, context=64, prefill_attn=True)
    w4, emu = _decoder(w4=True, **kw), _decoder(w4="emulate", **kw)
    sliced, tiled = _decoder(**kw), _decoder(prefill_tiled=True, **kw)
    ours, yard = [], []
    for seed in seeds:
        toks = _tokens((1, S), seed)
        lg = [_prefill_logits(d, toks)[1] for d in (w4, emu, sliced, tiled)]
        ours.append(_cosine(lg[0], lg[1]))
        yard.append(_cosine(lg[2], lg[3]))
    return ours, yard, (w4, emu)


def _block_linears(emu, toks, monkeypatch):
    """(name, xq, sx, Fp8Weight) of the four linears of layer 0 as the emulate decoder ran them on toks."""
    names = {id(w): name for name, w in emu.model.layers[0]._fp8.items()}
    seen, real = [], llm.linear_q

    def spy(xq, sx, w, **kw):
        if id(w) in names:
            seen.append((names[id(w)], xq.clone(), sx.clone(), w))
        return real(xq, sx, w, **kw)

    monkeypatch.setattr(llm, "linear_q", spy)
    emu.prefill(toks)
    monkeypatch.undo()
    assert [s[0] for s in seen] == ["qkv", "o", "w13", "w2"]
    return seen


def _excess(y, xq, sx, W):
    """Largest |y - ref| over the derived bound of mxfp4_cases.real_case, for the MX weight W on the device:
    2^-8 |ref| + (1 + 2^-8) g (|xq| |deq W|^T) sx, g = K u / (1 - K u), u = 2^-24."""
    x, d = xq.reshape(-1, W.K).double(), W.dequant().double()
    s = sx.reshape(-1, 1).double()
    ref, ku = x @ d.t() * s, W.K * 2.0 ** -24
    bound = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * ku / (1 - ku) * (x.abs() @ d.abs().t() * s)
    return ((y.reshape(-1, W.N).double() - ref).abs() / bound.clamp(min=1e-300)).max().item()


def test_w4_tracks_its_fp8_oracle(monkeypatch):
    """w4=True and w4="emulate" multiply the same numbers: they differ only in the
    fp32 accumulation order of every block linear.  The yardstick for that kind
    of difference is the stock fp8 decoder with sliced against tiled linears on
    the same tokens, measured here for three token seeds: each w4-versus-emulate
    cosine of the last-token logits after a 40-token prefill must be at least
    the smallest yardstick value minus the yardstick's own max - min spread.

    On this model the yardstick pair is bit-equal (cosine 1.0 for all three seeds,
    in two runs), although the tiled decoder does run the tiled GEMM in all five
    linears of a forward (qkv N 768, o 512, gate/up 2048, down 512, head 1024: all
    multiples of 128; K is 512, or 1024 for down).  Why the two kernels' fp32 sums
    come out alike at these K is not established (the 0.972 of the README is at
    llama3-8b's K of 4096 and 14336).  To re-check: compare the two decoders'
    logits with torch.equal.  So the yardstick measures nothing here and the
    test falls back to the derived bound on a single Block: each of the four linears of layer 0, on the
    quantised activations the emulate decoder fed it during the prefill, must
    lie within the bound of mxfp4_cases.real_case of the fp64 product of those
    codes and scales, on the fp4 kernel over the MX weight and on the fp8 kernel
    over its exact e4m3 copy alike (so the two differ by at most twice the
    bound).  A mis-wired weight (rows rolled by 16) must break it, and brings
    the logits' cosine near 0.  The whole two-layer decoder is held to a floor
    of its own, LOGITS_FLOOR."""
    ours, yard, (w4, emu) = oracle_cosines()
    floor = min(yard) - (max(yard) - min(yard))
    print(f"w4 vs emulate {['%.6f' % c for c in ours]}, sliced vs tiled fp8 {['%.6f' % c for c in yard]}, "
          f"threshold {floor:.6f}")
    toks = _tokens((1, 40), 21)
    if max(yard) < 1.0:
        assert all(c >= floor for c in ours), (ours, yard, floor)
    assert all(c >= LOGITS_FLOOR for c in ours), (ours, LOGITS_FLOOR)
    for name, xq, sx, w8 in _block_linears(emu, toks, monkeypatch):
        W = w4.model.layers[0]._fp8[name]
        assert torch.equal(w8.q.float() * w8.s[:, None], W.dequant())
        e4, e8 = _excess(llm.mxfp4_linear_q(xq, sx, W), xq, sx, W), _excess(llm.fp8_linear_q(xq, sx, w8), xq, sx, W)
        rolled = llm.Mxfp4Weight.from_quantised(W.codes.roll(16, 0), W.scales.roll(16, 0))
        bad = _excess(llm.mxfp4_linear_q(xq, sx, rolled), xq, sx, W)
        print(f"layer 0 {name} [{W.N}, {W.K}] x {xq.numel() // W.K} rows: fraction of the bound fp4 {e4:.3f}, "
              f"fp8 over the e4m3 copy {e8:.3f}, mis-wired fp4 {bad:.3g}")
        assert e4 <= 1 and e8 <= 1 and bad > 1
    good = _prefill_logits(emu, toks)[1]
    for layer in w4.model.layers:
        for name, w in layer._fp8.items():
            layer._fp8[name] = llm.Mxfp4Weight.from_quantised(w.codes.roll(16, 0), w.scales.roll(16, 0))
    bad = _cosine(_prefill_logits(w4, toks)[1], good)
    print(f"mis-wired decoder: cosine {bad:.6f}")
    assert bad < 0.5
