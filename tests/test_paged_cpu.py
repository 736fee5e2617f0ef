"""The paged KV cache off the GPU: the PagePool allocator, the paged fixtures
(tests/paged_cases.py), paged_gather / attn_paged_ref against attn_seq_ref, and
LlamaDecoder(paged=True) on its eager path against LlamaDecoder(ragged=True)
of the same weights, bit for bit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_cases as DC  # noqa: E402
import paged_cases as PG  # noqa: E402
import prefill_cases as PC  # noqa: E402
import ragged_cases as RC  # noqa: E402

from pbs_amd.models.llama import LlamaConfig, LlamaDecoder, PoolExhausted  # noqa: E402
from pbs_amd.models.paging import PagePool  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)
BATCH, CONTEXT, PAGE, LENS = 4, 200, 64, [150, 37, 0, 64]


# ------------------------------------------------------------------ PagePool
def test_page_pool_allocates_frees_and_shares_by_refcount():
    pool = PagePool(6)
    a, b = pool.alloc(2), pool.alloc(3)
    assert len(set(a + b)) == 5 and pool.free_pages == 1 and all(pool.ref[i] == 1 for i in a + b)
    assert pool.alloc(0) == [] and pool.free_pages == 1
    pool.share(a)
    assert [pool.ref[i] for i in a] == [2, 2] and pool.free_pages == 1
    pool.free(a)  # the first holder lets go: still allocated
    assert [pool.ref[i] for i in a] == [1, 1] and pool.free_pages == 1
    pool.free(a)
    assert [pool.ref[i] for i in a] == [0, 0] and pool.free_pages == 3
    pool.free(b)
    assert pool.free_pages == 6 and not any(pool.ref)
    assert sorted(pool.alloc(6)) == list(range(6))


def test_page_pool_exhaustion_leaves_it_unchanged_and_a_double_free_is_refused():
    pool = PagePool(4)
    a = pool.alloc(3)
    before = pool.snapshot()
    with pytest.raises(PoolExhausted):
        pool.alloc(2)
    assert pool.snapshot() == before and pool.free_pages == 1
    pool.free(a[:1])
    before = pool.snapshot()
    for bad in (a[:1], [a[1], a[1]], [7], [-1]):  # freed already, twice in one call, not a page
        with pytest.raises(ValueError):
            pool.free(bad)
        assert pool.snapshot() == before
    with pytest.raises(ValueError):
        pool.share(a[:1])  # a free page cannot be shared
    assert pool.snapshot() == before
    assert issubclass(PoolExhausted, RuntimeError)
    with pytest.raises(ValueError):
        PagePool(0)


# ------------------------------------------------------------------ fixtures, gather, reference
def _bits(t):
    return t.contiguous().view(torch.int16)


def test_paged_sets_and_contexts():
    assert PG.DECODE_SETS[3] == [-1, -1, 1152, 5] and PG.DECODE_SETS[:3] == RC.DECODE_SETS[:3]
    assert all(PG.n_table(DC.C, page) * page == 1152 for page in PG.PAGES)
    assert [PG.n_table(PC.C, page) * page for page in PG.PAGES] == [448, 512]


@pytest.mark.parametrize("page", PG.PAGES)
@pytest.mark.parametrize("s", range(len(PG.DECODE_SETS)))
def test_decode_fixture_is_shuffled_poisoned_and_paged_gather_inverts_it(s, page):
    c = PG.decode_case(s, 8, 2, page)
    used = [i for ids in c["ids"] for i in ids]
    assert len(set(used)) == len(used) and c["P"] == len(used) + PG.SPARE
    if len(used) > 4:  # non-monotonic, and interleaved between the sequences
        longest = max(c["ids"], key=len)
        assert longest != sorted(longest) and max(longest) - min(longest) + 1 > len(longest)
    free = sorted(set(range(c["P"])) - set(used))
    for pool in (c["kpool"], c["vpool"]):
        assert pool[free].isnan().all()
    for b, (ids, r) in enumerate(zip(c["ids"], c["rows"])):
        tail = c["table"][b, len(ids):].tolist()
        assert all(e in PG.GARBAGE for e in tail) and len(ids) == -(-r // page)
        if not r:
            continue
        for pool, dense in ((c["kpool"], c["kc"]), (c["vpool"], c["vc"])):
            assert torch.equal(_bits(llm.paged_gather(pool, c["table"][b], r)), _bits(dense[b, :, :r]))
            if r % page:  # the last page past the sequence's last row
                assert pool[ids[-1], :, r % page:].isnan().all()
        with pytest.raises(ValueError):  # one row into a garbage entry
            llm.paged_gather(c["kpool"], c["table"][b], len(ids) * page + 1)


@pytest.mark.parametrize("page", PG.PAGES)
@pytest.mark.parametrize("s", range(len(PG.PREFILL_SETS)))
def test_prefill_fixture_and_attn_paged_ref_is_attn_seq_ref_on_the_gathered_caches(s, page):
    H, Hkv = 8, 2
    c = PG.prefill_case(s, H, Hkv, page)
    assert c["Cl"] == (448 if page == 64 else 512)
    for b, r in enumerate(c["rows"]):
        for pool, dense in ((c["kpool"], c["kc"]), (c["vpool"], c["vc"])):
            if r:
                assert torch.equal(_bits(llm.paged_gather(pool, c["table"][b], r)), _bits(dense[b, :, :r]))
    got = llm.attn_paged_ref(c["q"], c["kpool"], c["vpool"], c["table"], c["pos"], c["lens"])
    # the dense fixture holds stale rows past each sequence's end; attn_seq_ref never reads them either
    want = llm.attn_seq_ref(c["q"], c["kc"], c["vc"], c["pos"], c["lens"])
    assert not got.isnan().any() and torch.equal(got, want)
    assert torch.equal(_bits(got.bfloat16()), _bits(c["expect"]))


@pytest.mark.parametrize("page", PG.PAGES)
def test_attn_paged_ref_decode_form_selects_the_expected_value_rows(page):
    for s in range(len(PG.DECODE_SETS)):
        c = PG.decode_case(s, 8, 2, page)
        lens = [int(PG.decode_active(p)) for p in c["positions"]]
        q = torch.nan_to_num(c["q"]).unsqueeze(1)  # an idle sequence's NaN query is never loaded by the kernels
        got = llm.attn_paged_ref(q, c["kpool"], c["vpool"], c["table"], c["positions"], lens)[:, 0]
        kc = PG.gather_dense(c["kpool"], c["ids"], c["rows"], c["Cl"])
        vc = PG.gather_dense(c["vpool"], c["ids"], c["rows"], c["Cl"])
        assert torch.equal(got, llm.attn_seq_ref(q, kc, vc, c["positions"], lens)[:, 0])
        assert torch.equal(_bits(got.bfloat16()), _bits(c["expect"]))


def test_paged_wrappers_check_the_table_and_pools_before_the_library(monkeypatch):
    def no_lib():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(llm, "lib", no_lib)
    pool = torch.zeros(3, 2, 64, 128, dtype=torch.bfloat16)
    q = torch.zeros(2, 8, 128, dtype=torch.bfloat16)
    pos = torch.zeros(2, dtype=torch.int32)
    good = torch.zeros(2, 4, dtype=torch.int32)
    for table, kp, vp, match in ((good.long(), pool, pool, "int32"),
                                 (good.t(), pool, pool, "contiguous|int32"),
                                 (good[0], pool, pool, "int32"),
                                 (good, pool, pool, "CUDA"),
                                 (good, pool, pool[:2], "one shape"),
                                 (good, pool[:, :, :32], pool[:, :, :32], "page in"),
                                 (good, torch.zeros(3, 2, 96, 128, dtype=torch.bfloat16),
                                  torch.zeros(3, 2, 96, 128, dtype=torch.bfloat16), "page in")):
        with pytest.raises(ValueError, match=match):
            llm.decode_attn_paged(q, kp, vp, table, pos)
        with pytest.raises(ValueError, match=match):
            llm.prefill_attn_paged(q.unsqueeze(1), kp, vp, table, pos, pos)


# ------------------------------------------------------------------ decoder (eager path, CPU)
def _decoder(state=None, **kw):
    d = LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, device="cpu", dtype=torch.float64, fused=False, **kw)
    if state is not None:
        d.model.load_state_dict(state)
    return d


def _spy(d, name, call):
    seen, fwd = [], getattr(d, name)

    def spy(*a, **k):
        r = fwd(*a, **k)
        if r is not None:
            seen.append(r[:, -1].clone())
        return r

    setattr(d, name, spy)
    try:
        out = call()
    finally:
        setattr(d, name, fwd)
    return out, seen


@pytest.fixture(scope="module")
def pair():
    """A dense ragged decoder and a paged one of the same weights, 10 pages where
    the dense cache is the equivalent of 16 (4 slots x ceil(200 / 64) pages)."""
    dense = _decoder(ragged=True)
    return dense, dense.model.state_dict()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, CFG.vocab, (BATCH, 150), generator=g), torch.randint(0, CFG.vocab, (50,), generator=g)


def _pages_hold(d):
    """Page accounting: ceil(pos / page) pages per slot, none shared here, the rest free."""
    for b in range(BATCH):
        assert len(d.pages_of(b)) == -(-max(d.pos_b[b], 0) // PAGE), (b, d.pos_b, d.pages_of(b))
    used = [i for b in range(BATCH) for i in d.pages_of(b)]
    assert len(set(used)) == len(used) and d.pages_free == d.pool.pages - len(used)


def _same_cache_rows(pg, dn):
    for (kp, vp), (kc, vc) in zip(pg.cache, dn.cache):
        for b in range(BATCH):
            n = max(pg.pos_b[b], 0)
            if n:
                assert torch.equal(llm.paged_gather(kp, pg.pages_of(b), n), kc[b, :, :n])
                assert torch.equal(llm.paged_gather(vp, pg.pages_of(b), n), vc[b, :, :n])


def test_paged_decoder_is_the_ragged_decoder_bit_for_bit_on_the_eager_path(pair, prompts):
    dn, state = pair
    pg = _decoder(state, paged=True, pages=10, page=PAGE)
    assert pg.ragged and pg.paged and pg.cache[0][0].shape == (10, 1, PAGE, 128) and pg.pages_free == 10
    (t0, l0), (t1, l1) = _spy(dn, "_forward", lambda: dn.prefill(prompts[0], lens=LENS)), \
        _spy(pg, "_forward_paged", lambda: pg.prefill(prompts[0], lens=LENS))
    assert torch.equal(t0, t1) and len(l0) == len(l1) == 1 and torch.equal(l0[0], l1[0])
    assert pg.pos_b == dn.pos_b == [150, 37, -1, 64] and pg.pages_free == 10 - (3 + 1 + 0 + 1)
    _pages_hold(pg)
    _same_cache_rows(pg, dn)
    for step in range(8):  # slot 3 starts its second page on the first step
        (t0, l0), (t1, l1) = _spy(dn, "_forward", lambda: dn.decode_step(t0)), \
            _spy(pg, "_forward_paged", lambda: pg.decode_step(t1))
        act = torch.tensor(pg.active)
        assert torch.equal(t0[act], t1[act]) and torch.equal(l0[0][act], l1[0][act]), f"step {step}"
        _pages_hold(pg)
        if step == 0:
            assert len(pg.pages_of(3)) == 2
    _same_cache_rows(pg, dn)
    (n0, l0), (n1, l1) = _spy(dn, "_forward", lambda: dn.admit(2, prompts[1], chunk=32)), \
        _spy(pg, "_forward_paged", lambda: pg.admit(2, prompts[1], chunk=32))
    assert torch.equal(n0, n1) and torch.equal(l0[-1], l1[-1])
    assert pg.pos_b == dn.pos_b == [158, 45, 50, 72]
    _pages_hold(pg)
    _same_cache_rows(pg, dn)
    held = pg.pages_of(1)
    kept = [(kp[held].clone(), vp[held].clone()) for kp, vp in pg.cache]
    free = pg.pages_free
    for d in (dn, pg):
        d.release(1)
    assert pg.pos_b == dn.pos_b and pg.pages_of(1) == [] and pg.pages_free == free + len(held)
    _pages_hold(pg)
    for (kp, vp), (k0, v0) in zip(pg.cache, kept):  # a release clears nothing
        assert torch.equal(kp[held], k0) and torch.equal(vp[held], v0)
    t0[2], t1[2] = n0[0], n1[0]
    t0, t1 = dn.decode_step(t0), pg.decode_step(t1)
    act = torch.tensor(pg.active)
    assert torch.equal(t0[act], t1[act])
    _same_cache_rows(pg, dn)


def _state_of(d):
    return (list(d.pos_b), list(d.active), [d.pages_of(b) for b in range(BATCH)], d.pool.snapshot(),
            [(k.clone(), v.clone()) for k, v in d.cache])


def _unchanged(d, st):
    now = _state_of(d)
    assert now[:4] == st[:4]
    for (k, v), (k0, v0) in zip(now[4], st[4]):
        assert torch.equal(k, k0) and torch.equal(v, v0)


def test_pool_exhausted_leaves_the_state_unchanged_and_release_makes_room(pair, prompts):
    _, state = pair
    pg = _decoder(state, paged=True, pages=6, page=PAGE)
    with pytest.raises(PoolExhausted):  # 3 + 3 + 0 + 1 pages
        pg.prefill(prompts[0], lens=[150, 150, 0, 64])
    assert pg.pages_free == 6 and pg.pos_b == [-1] * 4
    tok = pg.prefill(prompts[0], lens=[150, 37, 0, 64])  # 5 pages
    st = _state_of(pg)
    with pytest.raises(PoolExhausted):  # 2 pages for the prompt, 1 free
        pg.admit(2, prompts[0][1, :70])
    _unchanged(pg, st)
    with pytest.raises(PoolExhausted):  # a prefill that does not fit gives the old pages back
        pg.prefill(prompts[0], lens=[150, 150, 150, 0])
    _unchanged(pg, st)
    pg.admit(2, prompts[0][1, :64])  # the last page
    st = _state_of(pg)
    with pytest.raises(PoolExhausted):  # slots 2 and 3 start a page, none is free
        pg.decode_step(tok)
    _unchanged(pg, st)
    pg.release(0)
    assert pg.pages_free == 3
    pg.decode_step(tok)
    assert pg.pos_b == [-1, 38, 65, 65] and pg.pages_free == 1
    _pages_hold(pg)


def test_prefill_without_lens_and_in_chunks_is_the_ragged_prefill_of_full_lengths(pair, prompts):
    _, state = pair
    a, b, c = (_decoder(state, paged=True, pages=12, page=PAGE) for _ in range(3))
    ta, tb, tc = a.prefill(prompts[0]), b.prefill(prompts[0], lens=[150] * BATCH), c.prefill(prompts[0], chunk=64)
    assert torch.equal(ta, tb) and a.pos_b == b.pos_b == c.pos_b == [150] * BATCH and a.pages_free == 0
    assert tc.shape == ta.shape
    for (ka, va), (kb, vb) in zip(a.cache, b.cache):
        assert torch.equal(ka, kb) and torch.equal(va, vb)
    with pytest.raises(ValueError):
        a.prefill(prompts[0], lens=LENS, chunk=64)


def test_shared_prefix_admission_maps_pages_and_survives_release_of_the_source(pair, prompts):
    _, state = pair
    pg = _decoder(state, paged=True, pages=10, page=PAGE)
    pg.prefill(prompts[0], lens=[150, 0, 0, 0])
    src = pg.pages_of(0)
    assert len(src) == 3 and pg.pages_free == 7
    # the same prompt, then something else: 2 full pages (128 tokens) are common
    prompt = torch.cat([prompts[0][0, :140], prompts[1][:20]])
    whole = _decoder(state, paged=True, pages=10, page=PAGE)
    want, lw = _spy(whole, "_forward_paged", lambda: whole.admit(1, prompt))
    got, lg = _spy(pg, "_forward_paged", lambda: pg.admit(1, prompt, share=(0, 140)))
    assert pg.pages_of(1)[:2] == src[:2] and len(pg.pages_of(1)) == 3 and pg.pages_of(1)[2] not in src
    assert [pg.pool.ref[i] for i in src] == [2, 2, 1] and pg.pages_free == 6 and pg.pos_b[1] == 160
    # the eager path is exact: rows 0 .. 127 are the source's, so the rest is the unshared admission's
    assert torch.equal(got, want) and torch.equal(lg[-1], lw[-1])
    for (kp, vp), (kw, vw) in zip(pg.cache, whole.cache):
        assert torch.equal(llm.paged_gather(kp, pg.pages_of(1), 160), llm.paged_gather(kw, whole.pages_of(1), 160))
        assert torch.equal(llm.paged_gather(vp, pg.pages_of(1), 160), llm.paged_gather(vw, whole.pages_of(1), 160))
    rows = [(llm.paged_gather(kp, pg.pages_of(1), 160).clone(), llm.paged_gather(vp, pg.pages_of(1), 160).clone())
            for kp, vp in pg.cache]
    pg.release(0)  # the source goes: the shared pages stay allocated
    assert [pg.pool.ref[i] for i in src] == [1, 1, 0] and pg.pages_free == 7 and pg.pages_of(0) == []
    pg.admit(0, prompts[1])  # takes a free page, not a shared one
    assert not set(pg.pages_of(0)) & set(pg.pages_of(1))
    for (kp, vp), (k0, v0) in zip(pg.cache, rows):
        assert torch.equal(llm.paged_gather(kp, pg.pages_of(1), 160), k0)
        assert torch.equal(llm.paged_gather(vp, pg.pages_of(1), 160), v0)
    pg.release(1)
    assert pg.pages_free == 9
    pg.release(0)
    assert pg.pages_free == 10 and not any(pg.pool.ref)
    # share counts full pages of what the source holds, and leaves a token to prefill
    pg.prefill(prompts[0], lens=[100, 0, 0, 0])
    pg.admit(1, prompts[0][0, :64], share=(0, 150))
    assert pg.pages_of(1)[:0] == [] and pg.pool.ref[pg.pages_of(0)[0]] == 1  # 64 tokens: nothing left to prefill
    pg.admit(2, prompts[0][0, :65], share=(0, 150))
    assert pg.pages_of(2)[0] == pg.pages_of(0)[0] and pg.pool.ref[pg.pages_of(0)[0]] == 2
    with pytest.raises(ValueError):
        pg.admit(3, prompts[1], share=(3, 10))
    with pytest.raises(ValueError):
        _decoder(state, ragged=True).admit(0, prompts[1], share=(1, 10))


def test_errors_of_the_paged_interface():
    for kw in (dict(pages=4, page=32), dict(pages=4, page=96), dict(pages=0), dict(pages=None)):
        with pytest.raises(ValueError):
            _decoder(paged=True, **kw)
    d = _decoder(paged=True, pages=4, page=128)
    assert d.n_table == 2 and tuple(d._table.shape) == (BATCH, 2) and d._table.dtype == torch.int32
