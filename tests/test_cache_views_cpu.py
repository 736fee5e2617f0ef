"""The union of the wrappers' host-side checks over every cache form: the bad
position / length vectors of test_ragged_cpu, the bad tables and pools of
test_paged_cpu and test_kv8_cpu, and the bad q / qkv / RoPE tables / nsplit of
test_decode_attn_cpu and test_prefill_attn_cpu, each against all the forms of
all four operations it applies to.  No GPU: a wrapper that reaches the library
fails the test."""
import pytest
import torch

from pbs_amd.ops import llm

BF, I32 = torch.bfloat16, torch.int32
B, H, HKV, HD, CN, S, P, PAGE, NP = 2, 8, 2, 128, 16, 4, 3, 64, 4
FORMS = ["", "_seq", "_paged", "_paged_kv8"]
OPS = ["qkv_rope_cache", "decode_attn", "qkv_rope_cache_prefill", "prefill_attn"]
PER_SEQ = FORMS[1:]
PAGED = FORMS[2:]


@pytest.fixture(autouse=True)
def no_lib(monkeypatch):
    def reached():
        raise AssertionError("the wrapper touched the library before validating")

    monkeypatch.setattr(llm, "lib", reached)


def good(op, form):
    """Arguments of llm.<op><form> by name, every host-side property right (nothing is on a GPU)."""
    prefill = "prefill" in op
    a = {"qkv": torch.zeros(B, S if prefill else 1, (H + 2 * HKV) * HD, dtype=BF),
         "q": torch.zeros(B, S, H, HD, dtype=BF) if prefill else torch.zeros(B, H, HD, dtype=BF),
         "cos": torch.zeros(NP * PAGE, HD // 2), "sin": torch.zeros(NP * PAGE, HD // 2), "n_heads": H,
         "pos_t": torch.zeros(B, dtype=I32), "len_t": torch.zeros(B, dtype=I32),
         "table": torch.zeros(B, NP, dtype=I32), "nsplit": None}
    if form == "":
        a["pos_t"] = 0 if prefill else torch.zeros(1, dtype=I32)
    if form in ("", "_seq"):
        a["k"], a["v"] = torch.zeros(B, HKV, CN, HD, dtype=BF), torch.zeros(B, HKV, CN, HD, dtype=BF)
    else:
        dt = torch.float8_e4m3fn if form == "_paged_kv8" else BF
        a["k"], a["v"] = torch.zeros(P, HKV, PAGE, HD).to(dt), torch.zeros(P, HKV, PAGE, HD).to(dt)
        a["kscale"], a["vscale"] = torch.ones(P, HKV, PAGE), torch.ones(P, HKV, PAGE)
    return a


def call(op, form, a):
    """llm.<op><form> in the argument order of its signature."""
    cache = [a["k"], a["v"]] + ([a["kscale"], a["vscale"]] if form == "_paged_kv8" else [])
    table = [a["table"]] if form in PAGED else []
    lens = [a["len_t"]] if "prefill" in op and form != "" else []
    if op.startswith("qkv"):
        args = [a["qkv"], a["cos"], a["sin"], a["pos_t"]] + lens + table + cache + [a["n_heads"]]
    else:
        args = [a["q"]] + cache + table + [a["pos_t"]] + lens + ([a["nsplit"]] if op == "decode_attn" else [])
    return getattr(llm, op + form)(*args)


def rejects(op, form, match, **bad):
    a = good(op, form)
    a.update(bad)
    with pytest.raises(ValueError, match=f"{op}{form}: .*({match})"):
        call(op, form, a)


def test_the_good_arguments_pass_every_host_side_check():
    """What is left to refuse is the device, asked for last and of the position first."""
    for op in OPS:
        for form in FORMS:
            what = "qkv|q" if form == "" and "prefill" in op else "pos_t"
            rejects(op, form, f"({what}) must be a CUDA tensor")


# ------------------------------------------------------------------ vectors (test_ragged_cpu)
def _vector(case, n):
    if case == "one":
        return torch.zeros(1, dtype=I32), "exactly B"
    if case == "b_plus_1":
        return torch.zeros(n + 1, dtype=I32), "exactly B"
    if case == "int64":
        return torch.zeros(n, dtype=torch.int64), "int32"
    if case == "cpu":
        return torch.zeros(n, dtype=I32), "must be a CUDA tensor"
    t = torch.zeros(2 * n, dtype=I32)[::2]
    assert t.numel() == n and not t.is_contiguous()
    return t, "contiguous"


@pytest.mark.parametrize("case", ["one", "b_plus_1", "int64", "cpu", "strided"])
@pytest.mark.parametrize("form", PER_SEQ)
@pytest.mark.parametrize("op", OPS)
def test_every_per_sequence_form_rejects_a_bad_position_or_length_vector(op, form, case):
    bad, match = _vector(case, B)
    rejects(op, form, f"pos_t.*{match}", pos_t=bad)
    if "prefill" in op and case != "cpu":  # without a GPU the good pos_t is refused for its device first
        rejects(op, form, f"len_t.*{match}", len_t=bad)


@pytest.mark.parametrize("op", ["qkv_rope_cache", "decode_attn"])
def test_the_uniform_decode_form_rejects_a_bad_position_tensor(op):
    rejects(op, "", "pos_t must be a 1-element int32", pos_t=torch.zeros(2, dtype=I32))
    rejects(op, "", "pos_t must be a 1-element int32", pos_t=torch.zeros(1, dtype=torch.int64))
    rejects(op, "", "pos_t must be a 1-element int32", pos_t=0)
    rejects(op, "", "pos_t must be a CUDA tensor")


@pytest.mark.parametrize("op", ["qkv_rope_cache_prefill", "prefill_attn"])
def test_the_uniform_prefill_form_rejects_a_bad_host_position(op):
    for pos in (-1, CN - S + 1, True, 0.0, torch.zeros(1, dtype=I32)):
        rejects(op, "", r"pos \+ S", pos_t=pos)


# ------------------------------------------------------------------ tables (test_paged_cpu)
@pytest.mark.parametrize("form", PAGED)
@pytest.mark.parametrize("op", OPS)
def test_every_paged_form_rejects_a_bad_table(op, form):
    table = torch.zeros(B, NP, dtype=I32)
    for bad, match in ((table.long(), "int32"), (table.t(), "contiguous|int32"), (table[0], "int32"),
                       (torch.zeros(B, 0, dtype=I32), "NP >= 1"), (None, "int32"), (table, "CUDA")):
        rejects(op, form, match, table=bad)


# ------------------------------------------------------------------ caches and pools (test_paged_cpu, test_kv8_cpu)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("op", OPS)
def test_every_form_rejects_bad_cache_tensors(op, form):
    a = good(op, form)
    k, name = a["k"], {"": "kc", "_seq": "kc", "_paged": "kpool", "_paged_kv8": "kpool8"}[form]
    rejects(op, form, "of one shape", v=a["v"][:1])
    rejects(op, form, "of one shape", k=k[0], v=k[0])
    wide = torch.zeros(k.shape[0], HKV, 2 * k.shape[2], HD).to(k.dtype)[:, :, ::2]
    assert wide.shape == k.shape and not wide.is_contiguous()
    rejects(op, form, f"{name} must be contiguous", k=wide)
    rejects(op, form, f"{name} must be " + ("float8_e4m3fn" if form == "_paged_kv8" else "bf16"), k=k.float())
    if form in PAGED:
        for page in (32, 96):
            pool = torch.zeros(P, HKV, page, HD).to(k.dtype)
            rejects(op, form, "page in", k=pool, v=pool.clone())
        rejects(op, form, "page in", k=k[:, :, :32], v=k[:, :, :32])
    if form == "_paged_kv8":
        sc = a["kscale"]
        for which in ("kscale", "vscale"):
            for bad in (sc[:, :, :32], sc.double(), sc.unsqueeze(-1), None):
                rejects(op, form, which, **{which: bad})


# ------------------------------------------------------------------ q, qkv, RoPE tables, nsplit
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("op", ["decode_attn", "prefill_attn"])
def test_every_form_keeps_the_checks_of_q(op, form):
    q = good(op, form)["q"]
    lay = r"must be \[B, S, H, 128\]" if "prefill" in op else r"must be \[B, H, 128\]"
    rejects(op, form, "group size", q=q[..., :6, :].contiguous())
    rejects(op, form, lay, q=torch.zeros(B + 1, *q.shape[1:], dtype=BF))
    rejects(op, form, lay, q=q[..., :64].contiguous())
    rejects(op, form, lay + "|must be .B, S >= 1, H, 128.", q=q.unsqueeze(1))
    rejects(op, form, "q must be bf16", q=q.float())
    rejects(op, form, "q must be contiguous", q=torch.zeros(*q.shape[:-1], 2 * HD, dtype=BF)[..., ::2])
    if op == "decode_attn":
        for nsplit in (0, -1, 2.0, True):
            rejects(op, form, "nsplit", nsplit=nsplit)
    if form in ("", "_seq"):  # the dense caches may have another head_dim, which only the write takes
        a = good(op, form)
        rejects(op, form, "head_dim", q=q[..., :64].contiguous(), k=a["k"][..., :64].contiguous(),
                v=a["v"][..., :64].contiguous())


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("op", ["qkv_rope_cache", "qkv_rope_cache_prefill"])
def test_every_form_keeps_the_checks_of_qkv_and_the_rope_tables(op, form):
    a = good(op, form)
    qkv, cos, rows = a["qkv"], a["cos"], CN if form in ("", "_seq") else NP * PAGE
    rejects(op, form, r"qkv \(\d", qkv=qkv[..., :-HD].contiguous())
    rejects(op, form, r"qkv \(\d", n_heads=H - 1)
    rejects(op, form, "qkv must be bf16", qkv=qkv.float())
    rejects(op, form, "qkv must be contiguous", qkv=torch.zeros(*qkv.shape[:-1], 2 * qkv.shape[-1], dtype=BF)[..., ::2])
    if "prefill" in op:
        rejects(op, form, r"qkv \(\d", qkv=torch.zeros(B + 1, S, qkv.shape[-1], dtype=BF))
        rejects(op, form, r"qkv \(\d", qkv=qkv[:, 0])
    rejects(op, form, "rope tables", cos=cos[:, :32], sin=cos[:, :32])
    rejects(op, form, "rope tables", sin=cos[:-1])
    rejects(op, form, "rope table.*fp32", cos=cos.double(), sin=cos.double())
    rejects(op, form, "rope table.*fp32", sin=cos.double())
    wide = torch.zeros(cos.shape[0], HD)[:, ::2]
    assert wide.shape == cos.shape and not wide.is_contiguous()
    rejects(op, form, "rope table.*contiguous", cos=wide)
    rejects(op, form, "rope table.*contiguous", sin=wide)
    short = S if op + form == "qkv_rope_cache_prefill" else rows  # the uniform prefill needs rows 0 .. pos + S - 1
    rejects(op, form, "cover", cos=cos[:short - 1].clone(), sin=cos[:short - 1].clone())
    a.update(cos=cos[:short].clone(), sin=cos[:short].clone())
    with pytest.raises(ValueError, match="must be a CUDA tensor"):  # tables of exactly the rows needed pass
        call(op, form, a)


def test_a_dense_write_takes_any_head_dim_that_is_a_multiple_of_8():
    for form in ("", "_seq"):
        for op in ("qkv_rope_cache", "qkv_rope_cache_prefill"):
            a = good(op, form)
            for hd, match in ((64, "must be a CUDA tensor"), (4, "hd % 8"), (12, "hd % 8")):
                k = torch.zeros(B, HKV, CN, hd, dtype=BF)
                qkv = torch.zeros(*a["qkv"].shape[:2], (H + 2 * HKV) * hd, dtype=BF)
                cos = torch.zeros(CN, hd // 2)
                rejects(op, form, match, k=k, v=k.clone(), qkv=qkv, cos=cos, sin=cos.clone())


def test_the_per_sequence_attention_launch_is_sized_for_s_and_the_paged_ones_clamp():
    q = torch.zeros(B, CN + 1, H, HD, dtype=BF)
    rejects("prefill_attn", "_seq", r"pos \+ S", q=q)
    qkv = torch.zeros(B, CN + 1, (H + 2 * HKV) * HD, dtype=BF)
    rejects("qkv_rope_cache_prefill", "_seq", "pos_t must be a CUDA tensor", qkv=qkv)  # n_b clamps: accepted as before
    q = torch.zeros(B, NP * PAGE + 1, H, HD, dtype=BF)
    for form in PAGED:
        rejects("prefill_attn", form, "pos_t must be a CUDA tensor", q=q)
