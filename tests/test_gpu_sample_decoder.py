"""LlamaDecoder(sampling=True) on the fp8 path of the MI355X: the dense ragged decoder and the paged decoder over the
fp8 KV cache, each with the captured graph and without it.  Every pick -- ragged prefill, decode steps, an admission
-- is replayed through llm.sample_ref on the CPU from dec.last_logits and must give the decoder's tokens exactly;
the captured graph and the plain static step must agree on every token.  The config is that of
tests/test_gpu_ragged_decoder.py."""
import pytest
import torch

from pbs_amd.models.llama import LlamaConfig, LlamaDecoder
from pbs_amd.ops import llm

pytestmark = pytest.mark.gpu

CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)
BATCH, CONTEXT, LENS, PAGE, PAGES = 4, 200, [150, 37, 0, 64], 64, 10
PARAMS = (dict(temperature=0.8, top_k=50, top_p=0.9, seed=7), dict(temperature=1.3, seed=2 ** 40 + 1),
          dict(temperature=0.9, top_p=0.8, seed=99), dict(temperature=1.0, top_k=5, top_p=0.5, seed=-3))
KINDS = {"dense": dict(ragged=True), "paged_kv8": dict(paged=True, pages=PAGES, page=PAGE, kv_fp8=True)}


def _decoder(state, kind, **kw):
    d = LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, fp8=True, sampling=True, **KINDS[kind], **kw)
    d.model.load_state_dict(state)
    d.model.attach_fp8()
    return d


@pytest.fixture(scope="module")
def state():
    return LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, fp8=True, ragged=True).model.state_dict()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, CFG.vocab, (BATCH, 150), generator=g).cuda(), \
        torch.randint(0, CFG.vocab, (50,), generator=g).cuda()


def _replay(d, tok, ctr, slot=None):
    sl = slice(None) if slot is None else slice(slot, slot + 1)
    s = d._samp
    assert d.last_logits.dtype == torch.bfloat16 and d.last_logits.shape == (len(ctr), CFG.vocab)
    want, st = llm.sample_ref(d.last_logits.cpu(), torch.tensor(s["inv_temp"][sl], dtype=torch.float32),
                              torch.tensor(s["top_k"][sl], dtype=torch.int32),
                              torch.tensor(s["top_p"][sl], dtype=torch.float32),
                              torch.tensor(s["seed"][sl], dtype=torch.int64), torch.tensor(ctr, dtype=torch.int32))
    assert torch.equal(tok.cpu(), want), (tok.view(-1).tolist(), want.view(-1).tolist(), ctr)
    return st


def _run(d, prompts):
    """Ragged prefill, 8 steps with a parameter change after 4, a release, an admission, 3 steps: every token."""
    out, kept = [], []
    for b, p in enumerate(PARAMS):
        d.set_sampling(b, **p)
    tok = d.prefill(prompts[0], lens=LENS)
    kept.append(_replay(d, tok, [150, 37, -1, 64]))
    assert tok[2, 0] == 0
    out.append(tok.clone())
    for step in range(8):
        if step == 4:
            d.set_sampling(0, temperature=0.0)  # greedy from here on, no recapture
            d.set_sampling(3, temperature=0.7, top_k=20, seed=5)
        pos = list(d.pos_b)
        tok = d.decode_step(tok)
        kept.append(_replay(d, tok, [p + 1 if p >= 0 else -1 for p in pos]))
        assert tok[2, 0] == 0
        if step >= 4:
            assert tok[0, 0] == d.last_logits[0].float().argmax()
        out.append(tok.clone())
    graph = d._g
    d.release(1)
    new = d.admit(2, prompts[1], chunk=32)
    assert new.shape == (1, 1)
    _replay(d, new, [50], slot=2)
    tok[2] = new[0]
    out.append(new.clone())
    for step in range(3):
        pos = list(d.pos_b)
        tok = d.decode_step(tok)
        kept.append(_replay(d, tok, [p + 1 if p >= 0 else -1 for p in pos]))
        assert tok[1, 0] == 0
        out.append(tok.clone())
    assert d._g is graph and d.pos_b == [161, -1, 53, 75]
    cnt = torch.stack(kept)[:, :, 1]
    assert int(cnt.max()) >= 5  # the picks were sampled from several tokens, not an arg-max under another name
    return out


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_sampling_decoder_replays_through_the_reference_with_and_without_the_graph(state, prompts, kind):
    dg, ds = _decoder(state, kind, graph=True), _decoder(state, kind)
    a, b = _run(dg, prompts), _run(ds, prompts)
    assert dg._g is not None and ds._g is None
    assert len(a) == len(b) == 13 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_all_greedy_sampling_decoder_is_the_argmax_decoder(state, prompts):
    samp = _decoder(state, "dense", graph=True)
    plain = LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, fp8=True, ragged=True, graph=True)
    plain.model.load_state_dict(state)
    plain.model.attach_fp8()
    t0, t1 = plain.prefill(prompts[0], lens=LENS), samp.prefill(prompts[0], lens=LENS)
    assert torch.equal(t0, t1)
    act = torch.tensor([n > 0 for n in LENS], device="cuda")
    for step in range(4):
        t0, t1 = plain.decode_step(t0), samp.decode_step(t1)
        assert torch.equal(t0[act], t1[act]) and t1[2, 0] == 0, f"step {step}"
