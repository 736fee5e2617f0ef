"""LlamaDecoder(paged=True) on the fp8 path of the MI355X against the dense
LlamaDecoder(ragged=True) of the same weights: ragged prefill, static and
graph-captured decode across a page boundary, admission, release, pool
exhaustion and shared-prefix admission.  The config is that of
tests/test_gpu_ragged_decoder.py with pages of 64 rows and a pool of 10 pages,
where the dense cache is the equivalent of 16."""
import pytest
import torch

from pbs_amd.models.llama import LlamaConfig, LlamaDecoder, PoolExhausted
from pbs_amd.ops import llm

pytestmark = pytest.mark.gpu

CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)
BATCH, CONTEXT, LENS, PAGE, PAGES = 4, 200, [150, 37, 0, 64], 64, 10


def _decoder(state=None, **kw):
    d = LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, fp8=True, **kw)
    if state is not None:
        d.model.load_state_dict(state)
        d.model.attach_fp8()
    return d


def _paged(state, **kw):
    return _decoder(state, paged=True, pages=PAGES, page=PAGE, **kw)


def _spy(d, name, call):
    """call() with d.<name> recorded: the last-token logits of every call that computed some."""
    seen, fwd = [], getattr(d, name)

    def spy(*a, **k):
        r = fwd(*a, **k)
        if r is not None:
            seen.append(r[:, -1].float().clone())
        return r

    setattr(d, name, spy)
    try:
        out = call()
    finally:
        setattr(d, name, fwd)
    return out, seen


@pytest.fixture(scope="module")
def state():
    return _decoder(ragged=True).model.state_dict()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, CFG.vocab, (BATCH, 150), generator=g).cuda(), \
        torch.randint(0, CFG.vocab, (50,), generator=g).cuda()


def _pages_hold(d, shared=0):
    """ceil(pos / page) pages per slot; `shared` pages are mapped twice; the rest of the pool is free."""
    for b in range(BATCH):
        assert len(d.pages_of(b)) == -(-max(d.pos_b[b], 0) // PAGE), (b, d.pos_b, d.pages_of(b))
    used = [i for b in range(BATCH) for i in d.pages_of(b)]
    assert len(set(used)) == len(used) - shared and d.pages_free == PAGES - len(set(used))
    assert all(d.pool.ref[i] == used.count(i) for i in range(PAGES))


def _same_cache_rows(pg, dn):
    for (kp, vp), (kc, vc) in zip(pg.cache, dn.cache):
        for b in range(BATCH):
            n = max(pg.pos_b[b], 0)
            if n:
                assert torch.equal(llm.paged_gather(kp, pg.pages_of(b), n), kc[b, :, :n]), f"slot {b}: k rows"
                assert torch.equal(llm.paged_gather(vp, pg.pages_of(b), n), vc[b, :, :n]), f"slot {b}: v rows"


def test_paged_decoder_is_the_dense_ragged_decoder_bit_for_bit(state, prompts):
    dn, pg = _decoder(state, ragged=True), _paged(state)
    assert pg.ragged and pg.static and pg.cache[0][0].shape == (PAGES, 1, PAGE, 128) and pg.pages_free == PAGES
    (t0, l0), (t1, l1) = _spy(dn, "_forward", lambda: dn.prefill(prompts[0], lens=LENS)), \
        _spy(pg, "_forward_paged", lambda: pg.prefill(prompts[0], lens=LENS))
    assert len(l0) == len(l1) == 1
    act = torch.tensor([n > 0 for n in LENS], device="cuda")
    assert torch.equal(t0, t1) and torch.equal(l0[0][act], l1[0][act])
    assert pg.pos_b == dn.pos_b == [150, 37, -1, 64] and pg.pages_free == PAGES - 5
    _pages_hold(pg)
    _same_cache_rows(pg, dn)
    for step in range(8):  # slot 3 (position 64) starts its second page on the first step
        t0, t1 = dn.decode_step(t0), pg.decode_step(t1)
        assert torch.equal(t0[act], t1[act]), f"step {step}"
        _pages_hold(pg)
        if step == 0:
            assert len(pg.pages_of(3)) == 2
    assert pg.pos_b == dn.pos_b == [158, 45, -1, 72]
    _same_cache_rows(pg, dn)


def test_static_and_graph_paged_decode_agree_through_admission_and_release(state, prompts):
    st, gr = _paged(state, static=True), _paged(state, graph=True)
    active = torch.tensor([n > 0 for n in LENS], device="cuda")
    toks = [d.prefill(prompts[0], lens=LENS) for d in (st, gr)]
    assert torch.equal(toks[0], toks[1])
    for step in range(8):
        toks = [d.decode_step(t) for d, t in zip((st, gr), toks)]
        assert torch.equal(toks[0][active], toks[1][active]), f"step {step}"
        assert all(0 <= int(t.min()) and int(t.max()) < CFG.vocab for t in toks)
        for d in (st, gr):
            _pages_hold(d)
        if step == 2:  # a request arrives while the batch is running
            graph = gr._g
            before = [[(k.clone(), v.clone()) for k, v in d.cache] for d in (st, gr)]
            new = [d.admit(2, prompts[1], chunk=32) for d in (st, gr)]
            assert torch.equal(new[0], new[1]) and new[0].shape == (1, 1)
            for d, old in zip((st, gr), before):
                assert d.pos_b == [153, 40, 50, 67] and all(d.active) and len(d.pages_of(2)) == 1
                _pages_hold(d)
                mine = d.pages_of(2)[0]
                rest = torch.arange(PAGES, device="cuda") != mine
                for (k, v), (k0, v0) in zip(d.cache, old):  # the admission wrote into its own page alone
                    assert torch.equal(k[rest], k0[rest]) and torch.equal(v[rest], v0[rest])
            for t in toks:
                t[2] = new[0][0]
            active[2] = True
    assert gr._g is graph  # slot 2 decoded with the graph captured before it was admitted
    assert st.pos_b == gr.pos_b == [158, 45, 55, 72]
    for (ks, vs), (kg, vg) in zip(st.cache, gr.cache):
        for b in range(BATCH):
            assert torch.equal(llm.paged_gather(ks, st.pages_of(b), st.pos_b[b]),
                               llm.paged_gather(kg, gr.pages_of(b), gr.pos_b[b]))
    for d in (st, gr):
        held = d.pages_of(1)
        kept = [(k[held].clone(), v[held].clone()) for k, v in d.cache]
        d.release(1)
        assert d.pages_of(1) == [] and d.pos_b[1] == -1
        _pages_hold(d)
        for (k, v), (k0, v0) in zip(d.cache, kept):  # a release clears nothing
            assert torch.equal(k[held], k0) and torch.equal(v[held], v0)
    active[1] = False
    for step in range(4):
        toks = [d.decode_step(t) for d, t in zip((st, gr), toks)]
        assert torch.equal(toks[0][active], toks[1][active]), f"step {step} after release"
    assert gr._g is graph and st.pos_b == gr.pos_b == [162, -1, 59, 76]
    for d in (st, gr):
        _pages_hold(d)


def test_a_request_that_does_not_fit_is_refused_before_any_launch_and_admitted_after_a_release(state, prompts):
    pg = _paged(state)
    tok = pg.prefill(prompts[0], lens=[150, 150, 150, 0])  # 9 of 10 pages
    assert pg.pages_free == 1
    snap = (list(pg.pos_b), [pg.pages_of(b) for b in range(BATCH)], pg.pool.snapshot(), pg._table.clone(),
            [(k.clone(), v.clone()) for k, v in pg.cache])
    calls = []
    fwd = pg._forward_paged
    pg._forward_paged = lambda *a, **k: calls.append(1) or fwd(*a, **k)
    with pytest.raises(PoolExhausted):
        pg.admit(3, prompts[0][3, :100])  # 2 pages
    assert not calls  # nothing was launched
    assert snap[0] == pg.pos_b and snap[1] == [pg.pages_of(b) for b in range(BATCH)] and snap[2] == pg.pool.snapshot()
    assert torch.equal(snap[3], pg._table)
    for (k, v), (k0, v0) in zip(pg.cache, snap[4]):
        assert torch.equal(k, k0) and torch.equal(v, v0)
    returned = pg.pages_of(1)
    pg.release(1)
    assert pg.pages_free == 4
    new = pg.admit(3, prompts[0][3, :100])
    assert calls and new.shape == (1, 1) and pg.pos_b == [150, -1, 150, 100]
    assert set(pg.pages_of(3)) <= set(returned) | set(range(PAGES)) and set(pg.pages_of(3)) & set(returned)
    _pages_hold(pg)
    tok[3] = new[0]
    pg.decode_step(tok)
    assert pg.pos_b == [151, -1, 151, 101]
    _pages_hold(pg)


def test_shared_prefix_admission(state, prompts):
    """Page-level facts are exact.  The next-token logits are compared with an
    unshared admission of the same tokens at cos > 0.995, the bound of
    tests/test_gpu_ragged_decoder.py: the shared rows were computed in the
    source's prefill batch, the unshared ones in a batch of one."""
    pg, whole = _paged(state), _paged(state)
    pg.prefill(prompts[0], lens=[150, 0, 0, 0])
    src = pg.pages_of(0)
    kept = [(k[src].clone(), v[src].clone()) for k, v in pg.cache]
    prompt = torch.cat([prompts[0][0, :140], prompts[1][:20]])  # 2 full pages in common
    want, lw = _spy(whole, "_forward_paged", lambda: whole.admit(1, prompt))
    got, lg = _spy(pg, "_forward_paged", lambda: pg.admit(1, prompt, share=(0, 140)))
    assert pg.pages_of(1)[:2] == src[:2] and len(pg.pages_of(1)) == 3 and pg.pages_of(1)[2] not in src
    assert [pg.pool.ref[i] for i in src] == [2, 2, 1] and pg.pages_free == PAGES - 4 and pg.pos_b[:2] == [150, 160]
    _pages_hold(pg, shared=2)
    for (k, v), (k0, v0) in zip(pg.cache, kept):  # the source's pages keep their bits
        assert torch.equal(k[src], k0) and torch.equal(v[src], v0)
    cos = torch.nn.functional.cosine_similarity(lg[-1], lw[-1], dim=-1).min().item()
    print(f"shared-prefix admission: min cosine of the next-token logits {cos:.6f}, logits bits equal: "
          f"{torch.equal(lg[-1], lw[-1])}, token equal: {torch.equal(got, want)}")
    assert cos > 0.995
    rows = [(llm.paged_gather(k, pg.pages_of(1), 160).clone(), llm.paged_gather(v, pg.pages_of(1), 160).clone())
            for k, v in pg.cache]
    pg.release(0)
    assert [pg.pool.ref[i] for i in src] == [1, 1, 0] and pg.pages_free == PAGES - 3
    tok = torch.zeros(BATCH, 1, dtype=torch.long, device="cuda")
    tok[1] = got[0]
    pg.decode_step(tok)  # the sharer goes on alone
    assert pg.pos_b == [-1, 161, -1, -1]
    for (k, v), (k0, v0) in zip(pg.cache, rows):
        assert torch.equal(llm.paged_gather(k, pg.pages_of(1), 160), k0)
        assert torch.equal(llm.paged_gather(v, pg.pages_of(1), 160), v0)
    pg.release(1)
    assert pg.pages_free == PAGES and not any(pg.pool.ref)
