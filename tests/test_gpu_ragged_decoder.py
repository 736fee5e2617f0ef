"""LlamaDecoder(ragged=True) on the fp8 path of the MI355X: ragged prefill,
static and graph-captured per-sequence decode, admission into an idle slot and
release, against a uniform decoder of the same weights."""
import pytest
import torch

from pbs_amd.models.llama import LlamaConfig, LlamaDecoder

pytestmark = pytest.mark.gpu

CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)
BATCH, CONTEXT, LENS = 4, 200, [150, 37, 0, 64]


def _decoder(state=None, **kw):
    d = LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, fp8=True, **kw)
    if state is not None:
        d.model.load_state_dict(state)
        d.model.attach_fp8()
    return d


def _spy(d, call):
    """call() with d._forward recorded: the last-token logits of every call that computed some."""
    seen, fwd = [], d._forward

    def spy(*a, **k):
        r = fwd(*a, **k)
        if r is not None:
            seen.append(r[:, -1].float().clone())
        return r

    d._forward = spy
    try:
        out = call()
    finally:
        d._forward = fwd
    return out, seen


@pytest.fixture(scope="module")
def uniform():
    """The reference: a uniform prefill_attn=True decoder, its weights, and its
    last-token logits and layer-0 caches for a prompt replicated over the batch."""
    d = _decoder(prefill_attn=True)

    def run(prompt):
        _, seen = _spy(d, lambda: d.prefill(prompt.view(1, -1).expand(BATCH, -1).contiguous()))
        n = prompt.numel()
        return seen[-1], d.cache[0][0][:, :, :n].clone(), d.cache[0][1][:, :, :n].clone()

    return d.model.state_dict(), run


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, CFG.vocab, (BATCH, 150), generator=g).cuda(), \
        torch.randint(0, CFG.vocab, (50,), generator=g).cuda()


def _cosine(a, b):
    return torch.nn.functional.cosine_similarity(a, b, dim=-1).min().item()


def test_ragged_prefill_matches_the_uniform_decoder_per_sequence(uniform, prompts):
    state, run = uniform
    d = _decoder(state, ragged=True)
    assert d.static and d.prefill_attn
    tok, seen = _spy(d, lambda: d.prefill(prompts[0], lens=LENS))
    assert len(seen) == 1 and tok.shape == (BATCH, 1) and int(tok[2]) == 0
    assert d.pos_b == [150, 37, -1, 64] and d.active == [True, True, False, True] and d.pos == 150
    for b, n in enumerate(LENS):
        if not n:
            continue
        lg, k0, v0 = run(prompts[0][b, :n])
        cos = _cosine(seen[0][b:b + 1], lg[b:b + 1])
        dk = (d.cache[0][0][b, :, :n].float() - k0[b].float()).abs().max().item()
        dv = (d.cache[0][1][b, :, :n].float() - v0[b].float()).abs().max().item()
        print(f"slot {b} ({n} tokens): min cosine {cos:.6f}, layer-0 cache diff k {dk:.3g} v {dv:.3g}, logits bits "
              f"equal: {torch.equal(seen[0][b], lg[b])}")
        assert cos > 0.995 and dk < 1e-2 and dv < 1e-2
    for k, v in d.cache:
        assert not k[2].view(torch.int16).any() and not v[2].view(torch.int16).any()


def test_static_and_graph_decode_agree_admit_and_release(uniform, prompts):
    state, run = uniform
    st, gr = _decoder(state, ragged=True, static=True), _decoder(state, ragged=True, graph=True)
    active = torch.tensor([n > 0 for n in LENS], device="cuda")
    toks = [d.prefill(prompts[0], lens=LENS) for d in (st, gr)]
    assert torch.equal(toks[0], toks[1])
    for step in range(8):
        toks = [d.decode_step(t) for d, t in zip((st, gr), toks)]
        assert torch.equal(toks[0][active], toks[1][active]), f"step {step}"
        assert all(0 <= int(t.min()) and int(t.max()) < CFG.vocab for t in toks)
        if step == 2:  # a request arrives while the batch is running
            graph = gr._g
            before = [[(k.clone(), v.clone()) for k, v in d.cache] for d in (st, gr)]
            for d in (st, gr):
                for k, v in d.cache:  # nothing has touched the idle slot
                    assert not k[2].view(torch.int16).any() and not v[2].view(torch.int16).any()
            new, seen = zip(*[_spy(d, lambda: d.admit(2, prompts[1], chunk=32)) for d in (st, gr)])
            assert torch.equal(new[0], new[1]) and new[0].shape == (1, 1)
            for d, old in zip((st, gr), before):
                assert d.pos_b == [153, 40, 50, 67] and all(d.active)
                for (k, v), (k0, v0) in zip(d.cache, old):
                    for b in (0, 1, 3):
                        assert torch.equal(k[b], k0[b]) and torch.equal(v[b], v0[b])
            lg, _, _ = run(prompts[1])
            cos = _cosine(seen[1][-1], lg[2:3])
            print(f"admitted slot: min cosine of the next-token logits {cos:.6f}")
            assert cos > 0.995
            for t in toks:
                t[2] = new[0][0]
            active[2] = True
    assert gr._g is graph  # slot 2 decoded with the graph captured before it was admitted
    assert st.pos_b == gr.pos_b == [158, 45, 55, 72]
    # release: the slot's cache rows stay bit for bit while the others go on
    for d in (st, gr):
        d.release(1)
    active[1] = False
    kept = [[(k[1].clone(), v[1].clone()) for k, v in d.cache] for d in (st, gr)]
    for step in range(4):
        toks = [d.decode_step(t) for d, t in zip((st, gr), toks)]
        assert torch.equal(toks[0][active], toks[1][active]), f"step {step} after release"
    for d, old in zip((st, gr), kept):
        assert d.pos_b == [162, -1, 59, 76]
        for (k, v), (k0, v0) in zip(d.cache, old):
            assert torch.equal(k[1], k0) and torch.equal(v[1], v0)
