"""The token sampler off the GPU: Philox, the exp2 polynomial and the integer weights of llm.sample_ref measured
against fp64, sample_ref against a per-row implementation on Python integers, a chi-square test of its draws, and
LlamaDecoder(sampling=True) on its eager path (CPU, fp32)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_cases as SC  # noqa: E402

from pbs_amd.models.llama import LlamaConfig, LlamaDecoder  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

CFG = LlamaConfig(dim=512, n_layers=2, n_heads=4, n_kv_heads=1, ffn_dim=1024, vocab=1024, max_seq=256)
BATCH, CONTEXT, PAGE, PAGES, LENS = 4, 200, 64, 10, [150, 37, 0, 64]


# ------------------------------------------------------------------ the pieces of the contract
def test_philox4x32_10_known_answers():
    kat = (((0,) * 4, (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            "d16cfe09 94fdcceb 5001e420 24126ea1"))
    for ctr, key, want in kat:
        assert " ".join(f"{v:08x}" for v in llm.philox4x32_ref(ctr, key)) == want


def test_exp2_polynomial_over_every_fraction():
    """All 2^23 fractions f = j / 2^23: p is non-decreasing, stays in [1, 2), and its relative error against fp64
    exp2 is below 2^-22.  Measured: 8.73e-08 = 2^-23.45 (SAMPLE_EXP2_COEF as committed)."""
    assert len(llm.SAMPLE_EXP2_COEF) == 6 and all(float(torch.tensor(c, dtype=torch.float32)) == c
                                                  for c in llm.SAMPLE_EXP2_COEF)
    f = torch.arange(1 << 23, dtype=torch.float32) / float(1 << 23)
    p = llm.sample_exp2_poly(f)
    assert p.dtype == torch.float32 and bool((p[1:] >= p[:-1]).all())
    assert p[0].item() == 1.0 and p.max().item() < 2.0
    rel = ((p.double() - torch.exp2(f.double())) / torch.exp2(f.double())).abs().max().item()
    print(f"exp2 polynomial: max relative error {rel:.3e} = 2^{math.log2(rel):.2f}")
    assert rel < 2.0 ** -22


def _tv(c):
    """Total-variation distance of w / sum w from the fp64 softmax of the same logits, per non-greedy row."""
    w = llm.sample_weights_ref(c["logits"], c["inv_temp"]).double()
    q = torch.softmax(c["logits"].double() * c["inv_temp"].double().view(-1, 1), -1)
    return 0.5 * (w / w.sum(-1, keepdim=True) - q).abs().sum(-1)


def test_weights_against_the_fp64_softmax():
    """Over the random fixtures (N(0, 9) bf16 rows, T 0.7 .. 1.4) the total-variation distance is at most 7.08e-06
    (measured: 3.6e-09 .. 7.08e-06 per row); asserted at twice that.  It is the truncation of the weights to
    integers and the polynomial's error, not the sampler's integer steps, which add none."""
    tv = torch.cat([_tv(c) for c in SC.random_cases() if c["ctr"][0] == 0])
    print(f"TV distance per row: min {tv.min().item():.3e} max {tv.max().item():.3e}")
    assert tv.max().item() < 2 * 7.08e-06


def _slow_row(w, it, k, p, seed, ctr, x):
    """One row of the contract on Python integers, sort and cumulative sums; w: the row's integer weights."""
    V = len(w)
    if ctr < 0:
        return 0, [0, 0, 0, 0]
    if it == 0:
        return max(range(V), key=lambda i: (x[i], -i)), [0, 0, 0, 0]
    t = 1
    order = sorted(w, reverse=True)
    if 0 < k < V:
        t = max(1, order[k - 1])
    if p < 1:
        s_k = sum(v for v in w if v >= t)
        P = min(max(math.floor(p * 65536), 0), 65535)
        target = max(1, s_k * P // 65536)
        acc, i = 0, 0
        while True:  # the values in descending order, ties together: the first at which the mass reaches the target
            j = i
            while j < V and order[j] == order[i]:
                acc, j = acc + order[j], j + 1
            if acc >= target:
                t = order[i]
                break
            i = j
    S, cnt = sum(v for v in w if v >= t), sum(1 for v in w if v >= t)
    seed &= (1 << 64) - 1
    out = llm.philox4x32_ref((ctr, 0, 0, 0), (seed & 0xffffffff, seed >> 32))
    r = ((out[0] + (out[1] << 32)) * S) >> 64
    acc = 0
    for i, v in enumerate(w):
        if v >= t:
            acc += v
            if acc > r:
                return i, [t, cnt, S, r]
    raise AssertionError("r >= S")


def _small(c):
    return c["logits"].shape[1] <= 1024


@pytest.mark.parametrize("c", [c for c in SC.all_cases() if _small(c)], ids=lambda c: c["name"])
def test_sample_ref_is_the_contract_row_by_row(c):
    tok, st = SC.reference(c)
    B, V = c["logits"].shape
    assert tok.shape == (B, 1) and st.shape == (B, 4) and tok.dtype == st.dtype == torch.int64
    it = torch.where(c["inv_temp"] == 0, torch.ones_like(c["inv_temp"]), c["inv_temp"])
    w = llm.sample_weights_ref(c["logits"], it)
    assert int(w.min()) >= 0 and int(w.max()) == 1 << 30
    for b in range(B):
        want = _slow_row(w[b].tolist(), c["inv_temp"][b].item(), c["top_k"][b].item(), c["top_p"][b].item(),
                         c["seed"][b].item(), c["ctr"][b].item(), c["logits"][b].float().tolist())
        assert (tok[b, 0].item(), st[b].tolist()) == want, f"row {b}"


def test_constructed_rows_give_what_they_were_built_for():
    c = SC.special_case()
    tok, st = SC.reference(c)
    row = {n: i for i, n in enumerate(SC.SPECIAL_ROWS)}
    assert st[row["equal"]].tolist()[:3] == [1, 1024, 1024 << 30]
    assert tok[row["peak"], 0] == SC.PEAK_AT and st[row["peak"]].tolist()[:3] == [1, 1, 1 << 30]
    assert tok[row["greedy_tie"], 0] == min(SC.TIE_AT) and not st[row["greedy_tie"]].any()
    assert st[row["k_tie"], 1] == 5 and tok[row["k_tie"], 0] in (10, 600, 5, 300, 1023)
    assert tok[row["idle"], 0] == 0 and not st[row["idle"]].any()
    assert st[row["p_tie"], 1] == 5 and tok[row["p_tie"], 0] in (512, 0, 7, 511, 1016)
    assert torch.isinf(c["logits"][row["neg_inf"]]).sum() == 1024 // 3
    assert not torch.isinf(c["logits"][row["neg_inf"], tok[row["neg_inf"], 0]])
    assert torch.equal(tok[row["neg_inf"]], tok[row["neg_inf_twin"]])
    assert torch.equal(st[row["neg_inf"]], st[row["neg_inf_twin"]])
    for V, B in ((8, 1), (8200, 3), (1024, 8)):  # all logits equal: floor(R V / 2^64), the index order of the scan
        e = SC.equal_case(V, B)
        tok, _ = SC.reference(e)
        for b in range(B):
            seed = e["seed"][b].item() & ((1 << 64) - 1)
            out = llm.philox4x32_ref((e["ctr"][b].item(), 0, 0, 0), (seed & 0xffffffff, seed >> 32))
            assert tok[b, 0].item() == ((out[0] + (out[1] << 32)) * V) >> 64


def test_greedy_is_argmax_where_the_maximum_is_unique():
    for c in SC.random_cases()[::8]:
        x = c["logits"]
        B = x.shape[0]
        srt = x.float().sort(-1, descending=True).values
        unique = srt[:, 0] > srt[:, 1]
        assert unique.any()
        zero = torch.zeros(B)
        tok, st = llm.sample_ref(x, zero, c["top_k"], c["top_p"], c["seed"], c["ctr"])
        assert torch.equal(tok[unique, 0], torch.argmax(x, -1)[unique]) and not st.any()


def test_chi_square_of_20000_draws():
    """20000 draws (counters 0 .. 19999, seed 2024) of one V = 8 row at T = 1 against its integer weights.  Seeds and
    counters are fixed, so the statistic is a constant: 13.49 on 7 degrees of freedom; the 0.999 quantile of chi-square
    with 7 degrees of freedom is 24.32."""
    n = 20000
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 8, generator=g).to(torch.bfloat16)
    one = torch.ones(n)
    tok, st = llm.sample_ref(x.expand(n, 8).contiguous(), one, torch.zeros(n, dtype=torch.int32), one,
                             torch.full((n,), 2024), torch.arange(n, dtype=torch.int32))
    w = llm.sample_weights_ref(x, torch.ones(1))[0].double()
    assert int((w > 0).sum()) == 8 and bool((st[:, 1] == 8).all())
    expect = n * w / w.sum()
    obs = torch.bincount(tok.view(-1), minlength=8).double()
    chi2 = ((obs - expect) ** 2 / expect).sum().item()
    print(f"chi-square {chi2:.3f} on 7 degrees of freedom; expected counts {expect.round().tolist()}")
    assert expect.min().item() >= 5 and chi2 < 24.322


# ------------------------------------------------------------------ the decoder, eager fp32 on the CPU
def _decoder(state=None, paged=False, **kw):
    extra = dict(paged=True, pages=PAGES, page=PAGE) if paged else dict(ragged=True)
    d = LlamaDecoder(CFG, batch=BATCH, context=CONTEXT, device="cpu", dtype=torch.float32, fused=False, **extra, **kw)
    if state is not None:
        d.model.load_state_dict(state)
    return d


@pytest.fixture(scope="module")
def state():
    return _decoder().model.state_dict()


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(5)
    return torch.randint(0, CFG.vocab, (BATCH, 150), generator=g), torch.randint(0, CFG.vocab, (50,), generator=g)


PARAMS = (dict(temperature=0.8, top_k=50, top_p=0.9, seed=7), dict(temperature=1.3, seed=2 ** 40 + 1),
          dict(), dict(temperature=1.0, top_k=5, top_p=0.5, seed=-3))


def _replay(d, tok, ctr, slot=None):
    """The pick just made, again through sample_ref on the logits the decoder kept."""
    sl = slice(None) if slot is None else slice(slot, slot + 1)
    s = d._samp
    want, _ = llm.sample_ref(d.last_logits.clone(), torch.tensor(s["inv_temp"][sl], dtype=torch.float32),
                             torch.tensor(s["top_k"][sl], dtype=torch.int32),
                             torch.tensor(s["top_p"][sl], dtype=torch.float32),
                             torch.tensor(s["seed"][sl], dtype=torch.int64), torch.tensor(ctr, dtype=torch.int32))
    assert torch.equal(tok, want), (tok.view(-1).tolist(), want.view(-1).tolist(), ctr)


@pytest.mark.parametrize("paged", (False, True), ids=("dense", "paged"))
def test_all_greedy_sampling_is_the_argmax_decoder(state, prompts, paged):
    plain, samp = _decoder(state, paged), _decoder(state, paged, sampling=True)
    t0, t1 = plain.prefill(prompts[0], lens=LENS), samp.prefill(prompts[0], lens=LENS)
    assert torch.equal(t0, t1) and plain.last_logits is None and samp.last_logits.shape == (BATCH, CFG.vocab)
    for step in range(8):
        t0, t1 = plain.decode_step(t0), samp.decode_step(t1)
        act = torch.tensor(plain.active)
        assert torch.equal(t0[act], t1[act]), f"step {step}"
        assert t1[2, 0] == 0  # the idle row
    assert plain.pos_b == samp.pos_b == [158, 45, -1, 72]


@pytest.mark.parametrize("paged", (False, True), ids=("dense", "paged"))
def test_every_pick_is_sample_ref_of_last_logits_and_a_request_does_not_see_its_neighbours(state, prompts, paged):
    """Prefill, 8 steps with a parameter change on the way, a release and a chunked admission: every pick replays
    through sample_ref on last_logits.  Then slot 1's request alone in another decoder (another slot, the other
    slots idle): the eager CPU logits of a request turn out bit-equal whatever shares the batch with it (every
    linear runs per token row, the attention per sequence), so the tokens themselves are asserted equal, not only
    their replays."""
    d = _decoder(state, paged, sampling=True)
    for b, p in enumerate(PARAMS):
        d.set_sampling(b, **p)
    tok = d.prefill(prompts[0], lens=LENS)
    _replay(d, tok, [150, 37, -1, 64])
    assert tok[2, 0] == 0
    mine = [tok[1, 0].item()]
    greedy = d.last_logits.argmax(-1)
    for step in range(8):
        if step == 4:
            d.set_sampling(0, temperature=0.0)  # from this step on slot 0 is greedy
        pos = list(d.pos_b)
        tok = d.decode_step(tok)
        _replay(d, tok, [p + 1 if p >= 0 else -1 for p in pos])
        if step >= 4:
            assert tok[0, 0] == d.last_logits[0].argmax()
        mine.append(tok[1, 0].item())
        greedy = torch.cat([greedy, d.last_logits.argmax(-1)])
    d.release(3)
    d.set_sampling(2, temperature=0.9, top_p=0.8, seed=99)
    new = d.admit(2, prompts[1], chunk=32)
    assert new.shape == (1, 1) and d.last_logits.shape == (1, CFG.vocab)
    _replay(d, new, [50], slot=2)
    tok[2] = new[0]
    pos = list(d.pos_b)
    tok = d.decode_step(tok)
    _replay(d, tok, [p + 1 if p >= 0 else -1 for p in pos])
    assert tok[3, 0] == 0 and d.pos_b == [159, 46, 51, -1]
    # the request of slot 1 alone, in slot 3 of a fresh decoder, admitted in chunks
    solo = _decoder(state, paged, sampling=True)
    solo.set_sampling(3, **PARAMS[1])
    t = solo.admit(3, prompts[0][1, :37], chunk=16)
    alone, full = [t[0, 0].item()], torch.zeros(BATCH, 1, dtype=torch.long)
    full[3] = t[0]
    for step in range(8):
        full = solo.decode_step(full)
        alone.append(full[3, 0].item())
    assert alone == mine
    assert sum(a != g for a, g in zip(mine, greedy[1::BATCH].tolist())) >= 2  # sampled, not the argmax in disguise


def test_set_sampling_validation(state):
    d = _decoder(state, sampling=True)
    for bad in (dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")),
                dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.2), dict(top_k=-1), dict(top_k=2.5),
                dict(slot=BATCH), dict(slot=-1), dict(seed=2 ** 63), dict(seed=1.5), dict(temperature=1e-45)):
        with pytest.raises(ValueError):
            d.set_sampling(**bad)
    assert d._samp["inv_temp"] == [0.0] * BATCH  # nothing was set by a refused call
    d.set_sampling(temperature=0.5, top_k=3)
    d.set_sampling(1, temperature=2.0, top_p=0.25, seed=-1)
    assert d._inv_temp.tolist() == [2.0, 0.5, 2.0, 2.0] and d._top_k.tolist() == [3, 0, 3, 3]
    assert d._top_p.tolist() == [1.0, 0.25, 1.0, 1.0] and d._seed.tolist() == [0, -1, 0, 0]
    d.release(1)
    assert d._samp["seed"][1] == -1  # release leaves the parameters alone
    with pytest.raises(ValueError):
        _decoder(state).set_sampling(temperature=1.0)  # sampling=False
