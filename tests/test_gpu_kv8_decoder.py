"""LlamaDecoder(paged=True, kv_fp8=True) on the fp8 path of the MI355X against
its decoder-level oracle, kv_fp8="emulate" (bf16 pools, the bf16 paged kernels,
and torch ops that round every written row through the codec), on the same
weights: everything is compared bit for bit.  The config is that of
tests/test_gpu_paged_decoder.py."""
import pytest
import torch

from pbs_amd.models.llama import LlamaConfig, LlamaDecoder, PoolExhausted
from pbs_amd.ops import llm

pytestmark = pytest.mark.gpu

CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)
BATCH, CONTEXT, LENS, PAGE, PAGES = 4, 200, [150, 37, 0, 64], 64, 10


def _decoder(state=None, pages=PAGES, **kw):
    d = LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, fp8=True, paged=True, pages=pages, page=PAGE, **kw)
    if state is not None:
        d.model.load_state_dict(state)
        d.model.attach_fp8()
    return d


def _spy(obj, name, call):
    """call() with obj.<name> recorded: the last-token logits of every call that computed some."""
    seen, fwd = [], getattr(obj, name)

    def spy(*a, **k):
        r = fwd(*a, **k)
        if r is not None:
            seen.append(r[:, -1].float().clone())
        return r

    setattr(obj, name, spy)
    try:
        out = call()
    finally:
        setattr(obj, name, fwd)
    return out, seen


@pytest.fixture(scope="module")
def state():
    return _decoder(kv_fp8="emulate").model.state_dict()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, CFG.vocab, (BATCH, 150), generator=g).cuda(), \
        torch.randint(0, CFG.vocab, (50,), generator=g).cuda()


def _pair(state, **kw):
    real, emu = _decoder(state, kv_fp8=True, **kw), _decoder(state, kv_fp8="emulate")
    assert len(real.cache[0]) == 4 and real.cache[0][0].dtype == torch.float8_e4m3fn
    assert real.cache[0][0].shape == (PAGES, 1, PAGE, 128) and real.cache[0][2].shape == (PAGES, 1, PAGE)
    assert real.cache[0][2].dtype == torch.float32 and len(emu.cache[0]) == 2 and emu.cache[0][0].dtype == torch.bfloat16
    return real, emu


def _same_rows(real, emu):
    """The dequantised gathered rows of every layer are the emulator's pool rows, bit for bit."""
    assert real.pos_b == emu.pos_b
    for layer, ((k8, v8, ks, vs), (kp, vp)) in enumerate(zip(real.cache, emu.cache)):
        kd, vd = llm.kv8_dequant(k8, ks), llm.kv8_dequant(v8, vs)
        for b in range(BATCH):
            n = max(real.pos_b[b], 0)
            if n:
                for name, mine, theirs in (("k", kd, kp), ("v", vd, vp)):
                    got = llm.paged_gather(mine, real.pages_of(b), n)
                    want = llm.paged_gather(theirs, emu.pages_of(b), n)
                    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"layer {layer} slot {b}: {name}"
                    assert got.float().abs().sum() > 0


def _prefill_both(real, emu, tokens, **kw):
    (t0, l0), (t1, l1) = (_spy(d, "_forward_paged", lambda: d.prefill(tokens, **kw)) for d in (real, emu))
    return t0, t1, l0, l1


def _decode_both(real, emu, t0, t1, active, steps, spy_real=True):
    for step in range(steps):
        if spy_real:  # the static step of both: last-token logits, then tokens
            (t0, l0), (t1, l1) = (_spy(d.model, "decode_fp8_static", lambda: d.decode_step(t)) for d, t in
                                  ((real, t0), (emu, t1)))
            assert len(l0) == len(l1) == 1 and torch.equal(l0[0][active], l1[0][active]), f"step {step}: logits"
        else:
            t0, t1 = real.decode_step(t0), emu.decode_step(t1)
        assert torch.equal(t0[active], t1[active]), f"step {step}: tokens"
    return t0, t1


def test_fp8_cache_decoder_is_its_emulation_bit_for_bit(state, prompts):
    real, emu = _pair(state)
    t0, t1, l0, l1 = _prefill_both(real, emu, prompts[0], lens=LENS)
    act = torch.tensor([n > 0 for n in LENS], device="cuda")
    assert len(l0) == len(l1) == 1
    assert torch.equal(t0, t1) and torch.equal(l0[0][act], l1[0][act])
    assert real.pos_b == [150, 37, -1, 64] and real.pages_free == PAGES - 5
    _same_rows(real, emu)
    t0, t1 = _decode_both(real, emu, t0, t1, act, 8)  # slot 3 (position 64) starts its second page on the first step
    assert real.pos_b == [158, 45, -1, 72] and len(real.pages_of(3)) == 2
    _same_rows(real, emu)
    # the cache differs from the bf16 one: the emulator's rows are not what a plain paged decoder stores
    plain = _decoder(state)
    plain.prefill(prompts[0], lens=LENS)
    k_plain = llm.paged_gather(plain.cache[0][0], plain.pages_of(0), 150)
    k_emu = llm.paged_gather(emu.cache[0][0], emu.pages_of(0), 150)
    assert not torch.equal(k_plain, k_emu) and torch.equal(k_emu, llm.kv8_round(k_plain))


def test_graph_captured_fp8_cache_decoder_through_release_and_admission(state, prompts):
    real, emu = _pair(state, graph=True)
    t0, t1, l0, l1 = _prefill_both(real, emu, prompts[0], lens=LENS)
    act = torch.tensor([n > 0 for n in LENS], device="cuda")
    assert torch.equal(t0, t1) and torch.equal(l0[0][act], l1[0][act])
    t0, t1 = _decode_both(real, emu, t0, t1, act, 3, spy_real=False)
    graph = real._g
    assert graph is not None
    # a request arrives while the batch is running
    (n0, l0), (n1, l1) = (_spy(d, "_forward_paged", lambda: d.admit(2, prompts[1], chunk=32)) for d in (real, emu))
    assert torch.equal(n0, n1) and n0.shape == (1, 1) and torch.equal(l0[-1], l1[-1])
    assert real.pos_b == emu.pos_b == [153, 40, 50, 67]
    for t, n in ((t0, n0), (t1, n1)):
        t[2] = n[0]
    act[2] = True
    t0, t1 = _decode_both(real, emu, t0, t1, act, 5, spy_real=False)
    assert real._g is graph and real.pos_b == [158, 45, 55, 72]
    _same_rows(real, emu)
    for d in (real, emu):
        d.release(1)
    act[1] = False
    t0, t1 = _decode_both(real, emu, t0, t1, act, 4, spy_real=False)
    assert real._g is graph and real.pos_b == emu.pos_b == [162, -1, 59, 76]
    _same_rows(real, emu)


def test_shared_prefix_admission_over_the_fp8_cache(state, prompts):
    """The shared pages carry their scales at the same page index: nothing new."""
    real, emu = _pair(state)
    prompt = torch.cat([prompts[0][0, :140], prompts[1][:20]])  # 2 full pages in common
    for d in (real, emu):
        d.prefill(prompts[0], lens=[150, 0, 0, 0])
    src = real.pages_of(0)
    kept = [[t[src].clone() for t in layer] for layer in real.cache]
    (g0, l0), (g1, l1) = (_spy(d, "_forward_paged", lambda: d.admit(1, prompt, share=(0, 140))) for d in (real, emu))
    assert torch.equal(g0, g1) and torch.equal(l0[-1], l1[-1])
    assert real.pages_of(1)[:2] == src[:2] and len(real.pages_of(1)) == 3 and real.pages_of(1)[2] not in src
    assert [real.pool.ref[i] for i in src] == [2, 2, 1] and real.pos_b[:2] == [150, 160]
    for layer, old in zip(real.cache, kept):  # the source's pages keep their bits, codes and scales
        for t, t0 in zip(layer, old):
            assert torch.equal(t[src].view(torch.uint8), t0.view(torch.uint8))
    _same_rows(real, emu)
    for d in (real, emu):
        d.release(0)
    tok = torch.zeros(BATCH, 1, dtype=torch.long, device="cuda")
    tok[1] = g0[0]
    act = torch.tensor([False, True, False, False], device="cuda")
    _decode_both(real, emu, tok, tok.clone(), act, 2)  # the sharer goes on alone
    assert real.pos_b == [-1, 162, -1, -1]
    _same_rows(real, emu)


def test_pool_exhausted_leaves_the_four_tensors_the_table_and_the_positions_unchanged(state, prompts):
    real = _decoder(state, kv_fp8=True)
    tok = real.prefill(prompts[0], lens=[150, 150, 150, 0])  # 9 of 10 pages
    assert real.pages_free == 1

    def snap():
        return (list(real.pos_b), list(real.active), [real.pages_of(b) for b in range(BATCH)], real.pool.snapshot(),
                real._table.clone(), [[t.clone().view(torch.uint8) for t in layer] for layer in real.cache])

    def unchanged(s0):
        s1 = snap()
        assert s0[:4] == s1[:4] and torch.equal(s0[4], s1[4])
        for a, b in zip(s0[5], s1[5]):
            assert all(torch.equal(x, y) for x, y in zip(a, b))

    s0 = snap()
    calls, fwd = [], real._forward_paged
    real._forward_paged = lambda *a, **k: calls.append(1) or fwd(*a, **k)
    with pytest.raises(PoolExhausted):
        real.admit(3, prompts[0][3, :100])  # 2 pages
    assert not calls
    unchanged(s0)
    real.admit(3, prompts[0][3, :64])  # the last page
    s0 = snap()
    with pytest.raises(PoolExhausted):  # slot 3 starts a page, none is free
        real.decode_step(torch.cat([tok[:3], tok[:1]]))
    unchanged(s0)
    real.release(1)
    real.decode_step(torch.cat([tok[:3], tok[:1]]))
    assert real.pos_b == [151, -1, 151, 65]


def test_chunked_and_unchunked_prefill_over_the_fp8_cache_give_equal_logits(state, prompts):
    """A query of a later chunk reads the rows of the earlier chunks from the
    cache, an unchunked query those its own launch wrote: the same dequantised
    rows, so the logits are equal bits."""
    whole, chunked = (_decoder(state, pages=12, kv_fp8=True) for _ in range(2))
    (t0, l0), (t1, l1) = _spy(whole, "_forward_paged", lambda: whole.prefill(prompts[0])), \
        _spy(chunked, "_forward_paged", lambda: chunked.prefill(prompts[0], chunk=64))
    assert len(l0) == len(l1) == 1
    print(f"chunked vs unchunked: max |logit difference| {(l0[0] - l1[0]).abs().max().item():.3g}")
    assert torch.equal(l0[0], l1[0]) and torch.equal(t0, t1)
    for a, b in zip(whole.cache, chunked.cache):
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, b))
