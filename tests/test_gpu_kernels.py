"""GPU tests (MI355X): HIP kernel numerics vs plain PyTorch fp32 references,
XCD gating confinement, counter attribution, device adapt == host adapt."""
import ctypes as C
import random

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU CI
    pytest.skip("no GPU", allow_module_level=True)

from pbs_amd import _native as N  # noqa: E402
from pbs_amd.ops import kernels as K  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _lib():
    N.load_hip(required=True)


# 128x128-tile path: (128,128,64), (256,384,512); 256x256 path (M, N % 256 ==
# 0; two phases per K-tile): K-tile counts 1, 2, 3, 16 and 64 exercise the
# prologue and the last tile's waits.
@pytest.mark.parametrize("M,Nn,Kd", [(128, 128, 64), (256, 384, 512), (256, 256, 64), (512, 768, 128),
                                     (768, 512, 192), (1024, 512, 1024), (4096, 4096, 4096)])
def test_gemm_bf16_matches_fp32_reference(M, Nn, Kd):
    g = torch.Generator(device="cuda").manual_seed(M + Nn + Kd)
    A = torch.randn(M, Kd, device="cuda", dtype=torch.bfloat16, generator=g)
    B = torch.randn(Nn, Kd, device="cuda", dtype=torch.bfloat16, generator=g)
    out = K.gemm_bf16(A, B)
    ref = A.float() @ B.float().t()
    err = (out.float() - ref).abs()
    tol = 2e-2 * ref.abs().max().item() + 1e-2
    assert err.max().item() < tol, (err.max().item(), tol)
    # relative error vs bf16 output rounding: mean well below one bf16 ulp
    assert (err / (ref.abs() + 1)).mean().item() < 5e-3


@pytest.mark.parametrize("n", [256, 384, 512])
def test_gemm_asymmetric_identity(n):
    """A = I with an asymmetric B catches row/col swaps in the C write."""
    A = torch.eye(n, device="cuda", dtype=torch.bfloat16)
    B = (torch.arange(n * n, device="cuda", dtype=torch.float32).view(n, n) % 97 - 48).to(torch.bfloat16)
    out = K.gemm_bf16(A, B)  # = A @ B^T = B^T
    assert torch.equal(out.float(), B.float().t())


def test_stream_copy_and_reduce_and_gemv():
    x = torch.randn(1 << 22, device="cuda", dtype=torch.bfloat16)
    y = torch.empty_like(x)
    K.stream_copy(x, y, chunk_bytes=1 << 16)
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    a = torch.randn(1 << 20, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(1 << 20, device="cuda", dtype=torch.bfloat16)
    r = K.reduce_bf16(a, b, chunk_bytes=1 << 15)
    ref = (a.float() + b.float()).to(torch.bfloat16)
    assert torch.equal(r, ref)
    W = torch.randn(1000, 1024, device="cuda", dtype=torch.bfloat16)
    v = torch.randn(1024, device="cuda", dtype=torch.bfloat16)
    yv = K.gemv_bf16(W, v)
    ref = W.float() @ v.float()
    assert torch.allclose(yv, ref, rtol=1e-3, atol=1e-2)


def test_census_xcds_dealt_round_robin():
    out = K.census(2048).cpu()
    xcc = out[:, 0]
    assert int(out[:, 3].eq(0xC0FFEE).sum()) == 2048
    counts = torch.bincount(xcc, minlength=8)
    assert counts.numel() == 8 and int((counts > 0).sum()) == 8, counts
    # blocks b and b+8 share an XCD (observed dealing; speed-only property)
    same = (xcc[:-8] == xcc[8:]).float().mean().item()
    assert same > 0.9, same


def test_gating_confines_work_to_owned_xcds():
    from pbs_amd.runtime.gpu import GpuContext
    ctx = GpuContext(0)
    owners = [5, 5, 7, 7, 7, 7, -1, 5]
    ctx.set_owners(owners)
    out = K.census(4096, table=ctx.table, tenant=5).cpu()
    for row in out.tolist():
        xcc, _, ok, _ = row
        assert ok == (1 if owners[xcc] == 5 else 0)
    # gated GEMM: all tiles done, counters only on tenant-5 XCDs
    A = torch.randn(1024, 1024, device="cuda", dtype=torch.bfloat16)
    B = torch.randn(1024, 1024, device="cuda", dtype=torch.bfloat16)
    C_ = K.gemm_bf16(A, B, table=ctx.table, tenant=5, counters=ctx.counters)
    torch.cuda.synchronize()
    ref = A.float() @ B.float().t()
    assert (C_.float() - ref).abs().max().item() < 0.5
    per = ctx.read_counters(5, per_xcd=True)
    for x in range(8):
        if owners[x] == 5:
            continue
        assert per[x] == (0, 0, 0, 0), (x, per[x])
    assert sum(p[0] for p in per) > 0
    ctx.close()


def test_counter_reduce_kernel():
    cnt = torch.randint(0, 1 << 40, (64, 8, 4), device="cuda", dtype=torch.int64)
    prev = torch.randint(0, 1 << 30, (64, 8, 4), device="cuda", dtype=torch.int64)
    prev[3, 2, 1] = cnt[3, 2, 1] + 5  # force one reset
    prev0 = prev.clone()
    ids = torch.tensor([3, 0, 17, 63], device="cuda", dtype=torch.int32)
    out = K.counter_reduce(cnt, prev, ids)
    torch.cuda.synchronize()
    # Q5: a counter that went backwards (reset) contributes 0, per element
    delta = torch.where(cnt >= prev0, cnt - prev0, torch.zeros_like(cnt))
    ref = delta[ids.long()].sum(dim=1)
    assert torch.equal(out, ref)
    assert torch.equal(prev[ids.long()], cnt[ids.long()])


def test_hwc_attribute_kernel_matches_host_reference():
    """k_hwc_attribute (one workgroup: per-partition ownership reductions,
    per-tenant attribution) against the host implementation of the same
    algorithm (csrc/hip/hwc_attr.h) on 40 random snapshot pairs: owned,
    time-shared and idle partitions, SE and co-resident modes, clean windows
    on and off, class-share intervals."""
    L = K.lib()
    worst = C.c_double(1.0)
    rc = L.gpbs_hip_hwc_attr_selftest(7, 40, C.byref(worst))
    assert rc == 0, rc
    assert worst.value < 1e-12, worst.value


def test_hwc_attribute_kernel_cost():
    """the attribution is a parallel kernel now -- the
    snapshot staged into LDS once, wave reductions per partition, a lane per
    tenant -- at <= 10 us of device time per call (round 3: 78 us)."""
    L = K.lib()
    out = (C.c_double * 3)()
    assert L.gpbs_hip_hwc_attr_bench(200, out) == 0
    print(f"k_hwc_attribute: {out[2]:.2f} us kernel (own stamps), {out[0]:.2f} us per back-to-back launch, "
          f"{out[1]:.2f} us launch+wait")
    assert out[2] <= 10.0, out[2]


def test_async_device_adapt_two_pools_harvest_their_own():
    """two PBS pools on one GPU context with device adapt.  Each
    pool's launch is harvested by that pool only (matched by its tenants),
    in either order, with states bit-identical to the host adapt_update;
    a harvest for tenants nobody launched finds nothing."""
    assert K.lib().gpbs_hip_adapt_pools_selftest(60) == 0


def test_device_adapt_bit_exact_vs_host():
    """The batched HIP adapt kernel equals the host engine's adapt_update."""
    lib = N.load_core()
    p = N.AdaptParams()
    from pbs_amd.core.engine import boot_params
    bp = boot_params()
    C.memmove(C.byref(p), C.byref(bp.adapt), C.sizeof(p))
    p.threshold = 2000
    rng = random.Random(7)
    n = 48
    host = [N.AdaptState() for _ in range(n)]
    for s in host:
        lib.gpbs_adapt_init(C.byref(s), C.byref(p), 100)
    dev_states = torch.zeros(n, C.sizeof(N.AdaptState), dtype=torch.uint8)
    for k in range(n):
        C.memmove(dev_states[k].data_ptr(), C.byref(host[k]), C.sizeof(N.AdaptState))
    dev_states = dev_states.cuda()
    for it in range(60):
        inst = [rng.choice([0, rng.randint(1, 10 ** 9)]) for _ in range(n)]
        miss = [rng.randint(0, max(1, i // rng.choice([3, 50, 2000]))) for i in inst]
        ss = [rng.randint(0, 50000) for _ in range(n)]
        sc = [rng.randint(0, 4) for _ in range(n)]
        deltas = torch.tensor([[inst[k], 0, 0, miss[k]] for k in range(n)], dtype=torch.int64, device="cuda")
        K.adapt_batch(dev_states, deltas, torch.tensor(ss, device="cuda"), torch.tensor(sc, device="cuda"), p)
        for k in range(n):
            lib.gpbs_adapt_update(C.byref(host[k]), C.byref(p), inst[k], miss[k], ss[k], sc[k])
    torch.cuda.synchronize()
    got = dev_states.cpu()
    for k in range(n):
        ref = bytes(C.string_at(C.byref(host[k]), C.sizeof(N.AdaptState)))
        assert bytes(got[k].numpy().tobytes()) == ref, k


_G256_SHAPES = ((256, 256, 64), (512, 256, 128), (256, 512, 192), (1024, 768, 1024), (1024, 512, 512))
_G256_DEFAULT = 8


def _g256_operands(M, Nn, Kd):
    g = torch.Generator(device="cuda").manual_seed(M * 7 + Kd)
    A = torch.randn(M, Kd, device="cuda", dtype=torch.bfloat16, generator=g)
    B = torch.randn(Nn, Kd, device="cuda", dtype=torch.bfloat16, generator=g)
    return A, B


@pytest.fixture(scope="module")
def g256_default():
    """Per shape: the fp32 reference and what the default dealing computes."""
    L = K.lib()
    old = L.gpbs_hip_set_gemm_opts(_G256_DEFAULT)
    try:
        res = {}
        for shape in _G256_SHAPES:
            A, B = _g256_operands(*shape)
            res[shape] = (A.float() @ B.float().t(), K.gemm_bf16(A, B))
        torch.cuda.synchronize()
        return res
    finally:
        L.gpbs_hip_set_gemm_opts(old)


# 8: 2-D per-XCD blocks (the default), 1: XCD-range tile queue, 0: row-major
# dealing from the plain queue, bit 23: static unit, 205064: the default as
# recorded command lines spell it.  (1024, 512, K) is the smallest shape at
# which 2-D blocks engage; (1024, 768, 1024) is one where they fall back.
_G256_LIVE = [8, 9, 0, 1, 8 | 1 << 23, 205064]
# Values that recorded command lines and profiles carry: each selected a
# schedule variant that is gone (docs/gemm_lab.md).  The setter keeps their
# dealing bits and the shipped schedule runs, so they stay exact too.
_G256_LEGACY = [2, 3, 4, 5, 16, 32, 256, 256 | 8, 256 | 9, 256 | 1024, 256 | 64, 256 | 4096, 256 | 4096 | 64, 256 | 8192,
                256 | 8192 | 64, 256 | 8192 | 32768, 256 | 8192 | 65536, 256 | 8192 | 65536 | 131072, 256 | 16384,
                256 | 16384 | 64, 262144, 524288, 256 | 8192 | 65536 | 131072 | 9, 32 | (1 << 20), 32 | (1 << 21),
                32 | (1 << 21) | 8, 32 | (1 << 22), 32 | (1 << 22) | 8, 256 | 8192 | 65536 | 131072 | 8 | (1 << 23)]


@pytest.mark.parametrize("opts", _G256_LIVE + _G256_LEGACY)
def test_gemm256_variants_match_reference(opts, g256_default):
    """Every tile dealing of the 256x256 kernel, under its live and its
    legacy spellings, is exact against fp32 on prologue/tail shapes and
    bit-identical to the default dealing: dealing changes which workgroup
    computes a tile, never the arithmetic."""
    L = K.lib()
    old = L.gpbs_hip_set_gemm_opts(opts)
    try:
        assert L.gpbs_hip_set_gemm_opts(-1) == opts & (1 | 8 | 1 << 23)
        for M, Nn, Kd in _G256_SHAPES:
            A, B = _g256_operands(M, Nn, Kd)
            out = K.gemm_bf16(A, B)
            ref, dflt = g256_default[(M, Nn, Kd)]
            err = (out.float() - ref).abs().max().item()
            assert err < 2e-2 * ref.abs().max().item() + 1e-2, (opts, M, Nn, Kd, err)
            assert torch.equal(out, dflt), (opts, M, Nn, Kd)
    finally:
        L.gpbs_hip_set_gemm_opts(old)


def test_gemm_opts_setter_normalises():
    """The setter stores the live dealing bits only: the bits that spell the
    shipped schedule are dropped silently, bits of removed variants with one
    line on stderr, and a negative value only queries."""
    L = K.lib()
    old = L.gpbs_hip_set_gemm_opts(-1)
    try:
        L.gpbs_hip_set_gemm_opts(32 | 1 << 21)
        assert L.gpbs_hip_set_gemm_opts(-1) == 0
        L.gpbs_hip_set_gemm_opts(205065)
        assert L.gpbs_hip_set_gemm_opts(-1) == 9
    finally:
        L.gpbs_hip_set_gemm_opts(old)
