"""GPU tests (MI355X) of the gated fp8 (e4m3) MFMA GEMM, k_gemm_fp8_tn
(csrc/hip/fp8_gemm_kernels.hip): operand lane map and K loop on exact integer
data, orientation, real scales, ragged M, the shuffled-weight staging path,
XCD gating, the native runner kind and the opt-in tiled prefill."""
import threading
import time

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU CI
    pytest.skip("no GPU", allow_module_level=True)

from pbs_amd import _native as N  # noqa: E402
from pbs_amd.ops import kernels as K  # noqa: E402
from pbs_amd.ops import llm  # noqa: E402

F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module", autouse=True)
def _lib():
    N.load_hip(required=True)


def _ints(rows, cols, seed):
    """Integer-valued e4m3 rows in [-8, 8] (exact in e4m3), asymmetric."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (rows, cols), generator=g).float().to(F8)


def _exact_ref(aq, sa, bq, sb):
    """fp32 reference on the CPU; on integer data with power-of-two scales
    every accumulation order gives these bits."""
    return K.gemm_fp8_ref(aq, sa, bq, sb).to(torch.bfloat16)


def _bound_check(out, ref):
    err = (out.float() - ref).abs().max().item()
    lim = 1e-2 * ref.abs().max().item()
    print(f"max err {err:.6g} bound {lim:.6g}")
    assert err <= lim, (err, lim)


# K-tiles: 1 (prologue only), 2 (both buffers), 4 (buffer parity + GROUP_M tail)
@pytest.mark.parametrize("M,Nn,Kd", [(128, 128, 128), (128, 256, 256), (384, 256, 512)])
def test_exact_lane_map_and_k_loop(M, Nn, Kd):
    aq, bq = _ints(M, Kd, M + Kd), _ints(Nn, Kd, Nn + 3 * Kd)
    one_a, one_b = torch.ones(M), torch.ones(Nn)
    out = K.gemm_fp8(aq.cuda(), one_a.cuda(), bq.cuda(), one_b.cuda())
    assert out.dtype == torch.bfloat16 and out.shape == (M, Nn)
    # |sum| <= 64 * 512 < 2^24: the fp32 sum is the exact integer in any order
    assert torch.equal(out.cpu(), _exact_ref(aq, one_a, bq, one_b))
    sa = 2.0 ** (torch.arange(M) % 5 - 2).float()
    sb = 2.0 ** (torch.arange(Nn) % 5 - 2).float()
    out = K.gemm_fp8(aq.cuda(), sa.cuda(), bq.cuda(), sb.cuda())
    assert torch.equal(out.cpu(), _exact_ref(aq, sa, bq, sb))


def test_row_column_orientation():
    """A = I with an asymmetric B catches a row/col swap in the C write."""
    M = Kd = 256
    Nn = 128
    aq = torch.eye(M).to(F8)
    b = (torch.arange(Nn * Kd) % 17 - 8).float().view(Nn, Kd)
    out = K.gemm_fp8(aq.cuda(), torch.ones(M, device="cuda"), b.to(F8).cuda(), torch.ones(Nn, device="cuda"))
    assert torch.equal(out.float().cpu(), b.t())


@pytest.mark.parametrize("M,Nn,Kd", [(256, 384, 1024), (1024, 512, 4096)])
def test_real_data_and_scales(M, Nn, Kd):
    g = torch.Generator(device="cuda").manual_seed(M + Nn)
    aq, sa = llm.quant_rows_fp8(torch.randn(M, Kd, device="cuda", generator=g).bfloat16())
    bq, sb = llm.quant_rows_fp8(torch.randn(Nn, Kd, device="cuda", generator=g).bfloat16())
    out = K.gemm_fp8(aq, sa, bq, sb)
    # fp32 accumulation order + bf16 output rounding (the bound of tests/test_fp8.py)
    _bound_check(out, K.gemm_fp8_ref(aq, sa, bq, sb))


@pytest.mark.parametrize("M", [1, 17, 129, 200])
def test_ragged_m(M):
    Nn = Kd = 256
    aq, bq = _ints(M, Kd, 7 * M), _ints(Nn, Kd, 11)
    ones = torch.ones(max(M, Nn))
    rows = (M + 127) // 128 * 128 + 8  # past the last tile's rows
    buf = torch.full((rows, Nn), -7777.0, dtype=torch.bfloat16, device="cuda")
    sentinel = buf[0, 0].item()
    out = K.gemm_fp8(aq.cuda(), ones[:M].cuda(), bq.cuda(), ones[:Nn].cuda(), out=buf[:M])
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[:M].cpu(), _exact_ref(aq, ones[:M], bq, ones[:Nn]))
    assert bool((buf[M:] == sentinel).all())


@pytest.mark.parametrize("Nn,Kd", [(128, 256), (384, 512)])
def test_shuffled_weight_matches_row_major(Nn, Kd):
    M = 200
    g = torch.Generator(device="cuda").manual_seed(Nn + Kd)
    W = llm.Fp8Weight((torch.randn(Nn, Kd, device="cuda", generator=g) * 0.02).bfloat16())
    xq, sx = llm.quant_rows_fp8(torch.randn(M, Kd, device="cuda", generator=g).bfloat16())
    y = llm.fp8_linear_q(xq, sx, W, tiled=True)
    assert y.shape == (M, Nn) and y.dtype == torch.bfloat16
    # same LDS image, MFMA order and epilogue: the same bits
    assert torch.equal(y, K.gemm_fp8(xq, sx, W.q, W.s))
    _bound_check(y, K.gemm_fp8_ref(xq, sx, W.q, W.s))


def test_gating_confines_fp8_gemm_to_owned_xcds():
    from pbs_amd.runtime.gpu import GpuContext
    ctx = GpuContext(0)
    owners = [5, 5, 7, 7, 7, 7, -1, 5]
    ctx.set_owners(owners)
    n = 1024
    aq, bq = _ints(n, n, 21), _ints(n, n, 22)
    ones = torch.ones(n)
    out = K.gemm_fp8(aq.cuda(), ones.cuda(), bq.cuda(), ones.cuda(), table=ctx.table, tenant=5,
                     counters=ctx.counters)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), _exact_ref(aq, ones, bq, ones))  # |sum| <= 64 * 1024 < 2^24
    per = ctx.read_counters(5, per_xcd=True)
    for x in range(8):
        if owners[x] == 5:
            continue
        assert per[x] == (0, 0, 0, 0), (x, per[x])
    assert sum(p[0] for p in per) > 0
    ctx.close()


def test_fp8_runner_completes_under_revocation():
    """Ownership flips every 200us while the fp8 GEMM tenant runs: units are
    revoked mid-flight and resumed, and the result stays right."""
    from pbs_amd.runtime.gpu import GpuContext, Runner
    ctx = GpuContext(0)
    r = Runner(ctx, "gemm_fp8", 3, engine_wake=False, M=1024, N=1024, K=1024)
    assert r.work_per_unit == 2.0 * 1024 ** 3 and r.unit_name == "FLOP"
    stop = False

    def flipper():
        i = 0
        while not stop:
            ctx.set_owners([3 if (x + i) % 2 == 0 else -1 for x in range(8)] if i % 3 else [-1] * 8)
            i += 1
            time.sleep(200e-6)
        ctx.set_owners([3] * 8)

    th = threading.Thread(target=flipper)
    th.start()
    r.submit(20)
    try:
        r.wait(120)
    finally:
        stop = True
        th.join()
    assert r.stats().units_done == 20
    aq, sa, bq, sb, c = r.fp8_operands()
    assert aq.shape == (1024, 1024) and aq.dtype == F8 and sa.shape == (1024,) and c.shape == (1024, 1024)
    _bound_check(c, K.gemm_fp8_ref(aq, sa, bq, sb))
    r.close()
    ctx.close()


def test_fp8_runner_completes_under_gpbs_next_to_a_stream_tenant():
    from pbs_amd.core.engine import Engine
    from pbs_amd.runtime.gpu import GpuContext, Runner
    e = Engine(sched="credit")
    for x in range(8):
        e.pool_assign(0, e.partition_add(0, x))
    e.tenant_create("Domain-0", nslots=1)
    a = e.tenant_create("gemm_fp8", nslots=8)
    b = e.tenant_create("hbm", nslots=8, weight=512)
    ctx = GpuContext(0, e)
    e.start()
    ra = Runner(ctx, "gemm_fp8", a, M=1024, N=1024, K=1024)
    rb = Runner(ctx, "stream", b, bytes=64 << 20)
    ra.submit(40)
    rb.submit(40)
    ra.wait(120)
    rb.wait(120)
    e.stop()
    assert ra.stats().units_done == 40 and rb.stats().units_done == 40
    assert ctx.read_counters(a)[0] > 0
    assert e.check() == ""
    for r in (ra, rb):
        r.close()
    ctx.close()
    e.close()


def test_bad_runner_shape_is_refused():
    from pbs_amd.runtime.gpu import GpuContext, Runner
    ctx = GpuContext(0)
    with pytest.raises(ValueError):
        Runner(ctx, "gemm_fp8", 3, engine_wake=False, M=200, N=256, K=256)
    ctx.close()


def test_tiled_prefill_tracks_sliced_prefill(monkeypatch):
    from pbs_amd.models.llama import PRESETS, LlamaDecoder
    torch.manual_seed(0)
    cfg = PRESETS["tiny"]
    ds = LlamaDecoder(cfg, batch=4, context=64, device="cuda", fused=True)
    dt = LlamaDecoder(cfg, batch=4, context=64, device="cuda", fused=True, prefill_tiled=True)
    dt.model.load_state_dict(ds.model.state_dict())
    for d in (ds, dt):
        d.model.attach_fp8()
        d.fp8 = True
    assert dt.prefill_tiled and not ds.prefill_tiled
    toks = torch.randint(0, cfg.vocab, (4, 48), device="cuda")  # M = 192: ragged against the 128-row tile
    calls = []
    real = llm.gemm_fp8
    monkeypatch.setattr(llm, "gemm_fp8", lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])
    cos_sim = torch.nn.functional.cosine_similarity
    with torch.no_grad():
        ls = ds.model.forward_fp8(toks, ds.cache, 0, tiled=ds.prefill_tiled)
        assert not calls
        lt = dt.model.forward_fp8(toks, dt.cache, 0, tiled=dt.prefill_tiled)
        assert calls and max(calls) == 192
        cos = cos_sim(lt.float().flatten(1), ls.float().flatten(1)).min().item()
        print("prefill min cosine", cos)
        assert cos > 0.995, cos  # two fp8 paths over the same weights (tests/test_fp8.py)
        # the decoder entry point takes the same paths; decode steps stay on the skinny kernel
        del calls[:]
        ns, nt = ds.prefill(toks), dt.prefill(toks)
        assert ns.shape == nt.shape == (4, 1) and len(calls) == 4 * cfg.n_layers + 1
        del calls[:]
        ss = ds.model.forward_fp8(ns, ds.cache, 48)
        st = dt.model.forward_fp8(ns, dt.cache, 48)
        assert not calls
        cos = cos_sim(st.float().flatten(1), ss.float().flatten(1)).min().item()
        print("decode min cosine", cos)
        assert cos > 0.995, cos
        assert ds.decode_step(ns).shape == dt.decode_step(ns).shape == (4, 1) and not calls
