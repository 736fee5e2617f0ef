"""llm.sample (k_sample_rows, csrc/hip/sample_kernels.hip) on the MI355X against llm.sample_ref on the CPU, over the
fixtures of tests/sample_cases.py: tokens and stats (t, cnt, S, r) with torch.equal, no tolerance.  The sampler is
defined in integers, so any difference is a bug: a fused multiply-add in the weight arithmetic, a tie dropped at a
threshold, a scan out of index order."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_cases as SC  # noqa: E402

from pbs_amd.ops import llm  # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_reference_outputs_are_not_vacuous():
    """On the reference alone, before the GPU is touched: over the random fixtures every row keeps cnt >= 2, and in
    at least a third of the (row, counter) pairs the token is not the arg-max.  Measured: 58 %, least cnt 2.  (The
    rows of edge_cases() are not counted: top_k 1, top_p 2^-16 and T 0.05 keep one token by definition.)"""
    pairs = other = 0
    for c in SC.random_cases():
        tok, st = SC.reference(c)
        assert bool((c["inv_temp"] > 0).all()) and bool((c["ctr"] >= 0).all())
        assert int(st[:, 1].min()) >= 2, c["name"]
        pairs += tok.numel()
        other += int((tok.view(-1) != c["logits"].float().argmax(-1)).sum())
    print(f"token is not the arg-max in {other} of {pairs} (row, counter) pairs")
    assert 3 * other >= pairs


def _check(c):
    want_tok, want_st = SC.reference(c)
    tok, st = llm.sample(*SC.args(c, "cuda"), stats=True)
    assert tok.shape == want_tok.shape and tok.dtype == torch.int64 and st.shape == want_st.shape
    tok, st = tok.cpu(), st.cpu()
    assert torch.equal(st, want_st), f"{c['name']}: stats {st.tolist()} != {want_st.tolist()}"
    assert torch.equal(tok, want_tok), f"{c['name']}: tokens {tok.view(-1).tolist()} != {want_tok.view(-1).tolist()}"


@pytest.mark.parametrize("V", sorted({s[0] for s in SC.RANDOM_SHAPES}))
def test_random_rows_match_the_reference_bit_for_bit(V):
    cases = [c for c in SC.random_cases() if c["logits"].shape[1] == V]
    assert len(cases) == len(SC.COUNTERS)
    for c in cases:
        _check(c)


def test_rows_at_the_ends_of_the_parameter_ranges():
    for c in SC.edge_cases():
        _check(c)


def test_constructed_rows():
    for c in SC.constructed_cases():
        _check(c)
    c = SC.special_case()
    tok = llm.sample(*SC.args(c, "cuda")).cpu()  # stats=False: the tokens alone
    assert torch.equal(tok, SC.reference(c)[0])
    row = {n: i for i, n in enumerate(SC.SPECIAL_ROWS)}
    assert tok[row["idle"], 0] == 0 and tok[row["neg_inf"], 0] == tok[row["neg_inf_twin"], 0]


def test_a_captured_launch_follows_the_parameter_and_counter_tensors():
    c = SC.random_cases()[8]  # V 1024, B 3
    x, it, k, p, seed, ctr = SC.args(c, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        llm.sample(x, it, k, p, seed, ctr, stats=True)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tok, st = llm.sample(x, it, k, p, seed, ctr, stats=True)
    g.replay()
    want = SC.reference(c)
    assert torch.equal(tok.cpu(), want[0]) and torch.equal(st.cpu(), want[1])
    # new values in place: another counter, slot 0 greedy, slot 1 idle, slot 2 with other cuts and another seed
    ctr.copy_(torch.tensor([41, -1, 7], dtype=torch.int32))
    it[0] = 0.0
    k[2], p[2], seed[2] = 7, 0.75, 2 ** 45 + 3
    g.replay()
    want2 = llm.sample_ref(*(t.cpu() for t in (x, it, k, p, seed, ctr)))
    assert torch.equal(tok.cpu(), want2[0]) and torch.equal(st.cpu(), want2[1])
    assert not torch.equal(want2[1], want[1]) and want2[0][1, 0] == 0 and want2[1][2, 1] >= 2


def test_host_checks():
    x, it, k, p, seed, ctr = SC.args(SC.random_cases()[8], "cuda")
    ok = dict(logits=x, inv_temp=it, top_k=k, top_p=p, seed=seed, ctr=ctr)
    for bad in (dict(logits=x.float()), dict(logits=x.cpu()), dict(logits=x[:, :1020]),
                dict(logits=x[:, :1020].contiguous()), dict(logits=x[0]), dict(inv_temp=it[:2]), dict(top_k=k[:2]),
                dict(top_p=torch.cat([p, p])), dict(seed=seed[:1]), dict(ctr=ctr[:2]), dict(inv_temp=it.double()),
                dict(top_k=k.long()), dict(seed=seed.int()), dict(ctr=ctr.cpu()), dict(top_p=p.cpu()),
                dict(logits=x[:, :0]), dict(inv_temp=it.view(3, 1))):
        with pytest.raises(ValueError):
            llm.sample(**{**ok, **bad})
    assert llm.sample(**ok).shape == (3, 1)
