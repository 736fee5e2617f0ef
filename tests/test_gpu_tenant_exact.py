"""The bf16 tenant kernels of csrc/hip/tenant_kernels.hip on the MI355X, held to
the fixtures of tests/tenant_cases.py (checked on the CPU by
tests/test_tenant_cases_cpu.py): both GEMMs bit for bit on integer and
k-select data over several tiles per workgroup and every tile dealing, within
an arithmetic bound on real data; stream copy and reduce in every variant at
sizes around each loop bound with guards on both sides; GEMV through the tail
loop and past the grid cap; and the exit protocol of all of them -- status
word and work-queue reset -- on a queue reused across launches.

One process, direct launches through pbs_amd.ops.kernels and the library: no
runners, no gating, no timing.  Shapes are the smallest that reach a path."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tenant_cases as TC  # noqa: E402

from pbs_amd.ops import kernels as K  # noqa: E402

pytestmark = pytest.mark.gpu

BF = TC.BF
DONE = 0x80000000
STATIC = 1 << 23


def _sentinel16(v):
    return v - 0x10000 if v >= 0x8000 else v


class _gemm_opts:
    """gpbs_hip_set_gemm_opts(opts) for a block, the old value put back after it."""

    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        self.old = K.lib().gpbs_hip_set_gemm_opts(self.opts)

    def __exit__(self, *a):
        K.lib().gpbs_hip_set_gemm_opts(self.old)


# ------------------------------------------------------------------ GEMM ---

def _fresh_c(M, N):
    out = torch.empty(M, N, dtype=BF, device="cuda")
    out.view(torch.int16).fill_(_sentinel16(TC.GEMM_SENTINEL))
    return out


def _assert_bits(out, bits, what):
    got = out.view(torch.int16).cpu()
    if torch.equal(got, bits):
        return
    bad = (got != bits).nonzero()
    unwritten = int(((got.to(torch.int32) & 0xFFFF) == TC.GEMM_SENTINEL).sum())
    m, n = bad[0].tolist()
    raise AssertionError(f"{what}: {bad.shape[0]} of {bits.numel()} elements differ ({unwritten} never written), "
                         f"first at {(m, n)}: got {got.view(BF)[m, n].item()}, expected {bits.view(BF)[m, n].item()}")


def _launches(M, N):
    """(opts, grid) of every launch form of a shape: the 256x256 kernel under its
    four dealings, both kernels at the default grid and at grids that give a
    workgroup several tiles."""
    if TC.is_g256(M, N):
        return [(o, g) for o in TC.G256_OPTS for g in TC.G256_GRIDS]
    return [(None, g) for g in TC.G128_GRIDS]


def _run_all_forms(A, B, bits, what):
    M, N = A.shape[0], B.shape[0]
    Ad, Bd = A.cuda(), B.cuda()
    for opts, grid in _launches(M, N):
        out = _fresh_c(M, N)
        if opts is None:
            K.gemm_bf16(Ad, Bd, out=out, grid=grid)
        else:
            with _gemm_opts(opts):
                K.gemm_bf16(Ad, Bd, out=out, grid=grid)
        _assert_bits(out, bits, f"{what} opts {opts} grid {grid}")


@pytest.mark.parametrize("shape", TC.GEMM_SHAPES)
def test_gemm_integer_operands_bit_exact_in_every_launch_form(shape):
    """Integers in [-8, 8]: the fp32 accumulator holds the exact sum in any order,
    so the output is ref64.to(bf16) bit for bit -- under every dealing, at the
    default grid and with several tiles per workgroup (grid 1; 3 or 5), and
    therefore equal across all of them.  C is prefilled with a NaN pattern no
    reference contains."""
    A, B, _, bits = TC.int_case(*shape)
    _run_all_forms(A, B, bits, f"integer {shape}")


@pytest.mark.parametrize("direction", ["a", "b"])
@pytest.mark.parametrize("shape", TC.GEMM_SHAPES)
def test_gemm_kselect_bit_exact(shape, direction):
    """One 1 per row of A at k = f(m) against a coded B gives C[m, n] = B[n, f(m)]
    ('a'), and the mirror ('b'): f hits all 64 positions of a K-tile and every
    K-tile within every 128-row half, so a wrong swizzle, a wrong LDS buffer or
    a K-tile read twice or not at all shows as a wrong integer."""
    A, B, _, bits = TC.kselect_case(*shape, direction)
    _run_all_forms(A, B, bits, f"k-select {direction} {shape}")


@pytest.mark.parametrize("shape", TC.REAL_SHAPES)
def test_gemm_real_data_within_the_arithmetic_bound(shape):
    """randn bf16 against fp64, per element within
        2^-8 |ref| + K 2^-23 (|A| @ |B|^T):
    rounding of the result to bf16 (half a unit of an 8-bit significand) plus
    K fp32 additions in an unknown order, each within 2^-23 of a partial sum
    that never exceeds sum |a||b| (the products are exact in fp32).  Derived in
    tenant_cases.gemm_bound, not tuned.  At K = 4096 that is about 1.5 where the
    tolerance test allows 6: a dropped or doubled 32-k sub-step is outside."""
    A, B, ref, bound = TC.real_case(*shape)
    M, N = ref.shape
    out = _fresh_c(M, N)
    K.gemm_bf16(A.cuda(), B.cuda(), out=out)
    got = out.cpu().double()
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} elements never written or not finite"
    err = (got - ref).abs()
    print(f"gemm {shape}: max err {err.max().item():.4g}, {(err / bound).max().item():.3g} of the bound")
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements outside the bound, first {bad[:4].tolist()}"


# --------------------------------------------------------- exit protocol ---

def _status_ptr(st):
    return C.c_void_p(st.data_ptr()) if st is not None else None


def _assert_exit(st, q, units, what):
    """After a synchronised launch: the status word reports every unit with the
    done bit, and the last workgroup out left all 16 queue words zero."""
    torch.cuda.synchronize()
    word = st.item() & 0xFFFFFFFF
    assert word == (units | DONE), f"{what}: status word {word:#x}, expected {units | DONE:#x}"
    assert q.cpu().tolist() == [0] * 16, f"{what}: work queue {q.cpu().tolist()}"
    st.zero_()


def _gemm_direct(A, B, out, q, st, grid=0):
    M, Kd = A.shape
    rc = K.lib().gpbs_hip_gemm_bf16(K._ptr(A), K._ptr(B), K._ptr(out), M, B.shape[0], Kd, K._ptr(q), None, K.GATE_NONE,
                                    0, None, _status_ptr(st), grid, K._stream())
    assert rc == 0, rc


@pytest.mark.parametrize("opts", [8, 1])
def test_gemm_exit_protocol_on_a_reused_queue(opts):
    """12 tiles, then 1 tile, on one work queue -- the plain queue (8) and the
    XCD-range queue (1), whose per-range counters must be reset too."""
    q, st = K.work_queue(), K.status_word()
    with _gemm_opts(opts):
        for shape in [(1024, 768, 64), (256, 256, 64)]:
            A, B, _, bits = TC.int_case(*shape)
            out = _fresh_c(shape[0], shape[1])
            _gemm_direct(A.cuda(), B.cuda(), out, q, st)
            _assert_exit(st, q, TC.gemm_units(shape[0], shape[1]), f"opts {opts} {shape}")
            _assert_bits(out, bits, f"opts {opts} {shape} on the reused queue")


def test_gemm128_exit_protocol_on_a_reused_queue():
    q, st = K.work_queue(), K.status_word()
    for shape in [(1152, 384, 128), (128, 128, 64)]:
        A, B, _, bits = TC.int_case(*shape)
        out = _fresh_c(shape[0], shape[1])
        _gemm_direct(A.cuda(), B.cuda(), out, q, st, grid=5)
        _assert_exit(st, q, TC.gemm_units(shape[0], shape[1]), f"128x128 {shape}")
        _assert_bits(out, bits, f"128x128 {shape} on the reused queue")


def test_gemm_static_opts_still_publish_the_status_word():
    """opts 8 | 1 << 23, ungated, one workgroup per tile: with a status pointer
    the launch must still report all its units (a runner relaunches a unit
    whose word stays 0 for ever).  The static unit never runs finish(), so the
    host selects it only for launches without a status word."""
    shape = (1024, 768, 64)
    A, B, _, bits = TC.int_case(*shape)
    q, st = K.work_queue(), K.status_word()
    with _gemm_opts(8 | STATIC):
        out = _fresh_c(shape[0], shape[1])
        _gemm_direct(A.cuda(), B.cuda(), out, q, st)           # default grid, clamped to the 12 tiles
        _assert_exit(st, q, 12, "static opts with a status word")
        _assert_bits(out, bits, "static opts with a status word")


def test_gemm_static_unit_still_runs_for_direct_calls():
    """Without a status word, opts bit 23 keeps meaning unit = blockIdx.x with
    the queue untouched.  Seen on a queue that reads drained (next = 12): the
    static unit computes every tile and leaves the queue as it found it, the
    queued kernel under plain opts 8 finds nothing to grab and writes nothing."""
    shape = (1024, 768, 64)
    A, B, _, bits = TC.int_case(*shape)
    Ad, Bd = A.cuda(), B.cuda()
    drained = [12] + [0] * 15
    q = torch.tensor(drained, dtype=torch.int32, device="cuda")
    with _gemm_opts(8 | STATIC):
        out = _fresh_c(shape[0], shape[1])
        _gemm_direct(Ad, Bd, out, q, None)
        torch.cuda.synchronize()
        _assert_bits(out, bits, "static unit")
        assert q.cpu().tolist() == drained
    with _gemm_opts(8):
        out = _fresh_c(shape[0], shape[1])
        _gemm_direct(Ad, Bd, out, q, None)
        torch.cuda.synchronize()
        got = out.view(torch.int16).cpu().to(torch.int32) & 0xFFFF
        assert (got == TC.GEMM_SENTINEL).all()


def test_stream_reduce_gemv_exit_protocol_on_one_queue():
    """Stream (4 chunks), then reduce (4 chunks), then GEMV (2 units) on one
    queue: each reports its units, leaves the queue zero and is exact."""
    L, q, st = K.lib(), K.work_queue(), K.status_word()
    n = 3 * 256 + 17
    # stream
    payload = TC.stream_payload()
    src = torch.cat([torch.zeros(TC.MEM_LEAD, dtype=torch.uint8), payload]).cuda()[TC.MEM_LEAD:]
    img = TC.copy_image(payload, n * 16).cuda()
    dbuf = torch.full_like(img, TC.COPY_SENTINEL)
    lo = TC.MEM_LEAD + TC.STREAM_GUARD
    rc = L.gpbs_hip_stream_copy(K._ptr(src), K._ptr(dbuf[lo:]), n * 16, 256 * 16, K._ptr(q), None, K.GATE_NONE, 0, None,
                                _status_ptr(st), 3, K._stream())
    assert rc == 0
    _assert_exit(st, q, 4, "stream")
    assert torch.equal(dbuf, img)
    # reduce
    a, b, _, _ = TC.reduce_case(n)
    img, mask = (t.cuda() for t in TC.reduce_image(n))
    obuf = torch.full_like(img, TC.REDUCE_SENTINEL)
    lo = (TC.MEM_LEAD + TC.REDUCE_GUARD) // 2
    ad, bd = a.cuda(), b.cuda()
    rc = L.gpbs_hip_reduce_bf16(K._ptr(ad), K._ptr(bd), K._ptr(obuf[lo:]), n * 16, 256 * 16, K._ptr(q), None,
                                K.GATE_NONE, 0, None, _status_ptr(st), 3, K._stream())
    assert rc == 0
    _assert_exit(st, q, 4, "reduce")
    assert int(_reduce_bad(obuf, img, mask).sum()) == 0
    # gemv
    W, x, bits = TC.gemv_int_case(17, 1536)
    img = TC.gemv_image(bits).cuda()
    ybuf = torch.full_like(img, TC.GEMV_SENTINEL)
    Wd, xd = W.cuda(), x.cuda()
    rc = L.gpbs_hip_gemv_bf16(K._ptr(Wd), K._ptr(xd), K._ptr(ybuf[TC.GEMV_GUARD:]), 17, 1536, K._ptr(q), None,
                              K.GATE_NONE, 0, None, _status_ptr(st), 0, K._stream())
    assert rc == 0
    _assert_exit(st, q, 2, "gemv")
    assert torch.equal(ybuf, img)


# ----------------------------------------------------------- stream copy ---

@pytest.mark.parametrize("opts", TC.STREAM_OPTS)
def test_stream_copy_every_variant_at_every_loop_bound(opts):
    """Random bytes (NaN patterns among them) compared as integers, source and
    destination 16 bytes into their allocations, sentinel guards of more than a
    chunk on both sides of the destination.  Sizes and chunks sit below, on and
    one vector past the workgroup and one pass of the variant's unrolled loop,
    so every idx < end guard takes both branches; grids 1 and 3 walk several
    chunks per workgroup."""
    L = K.lib()
    nt, u = TC.stream_geom(opts)
    payload = TC.stream_payload()
    src = torch.cat([torch.zeros(TC.MEM_LEAD, dtype=torch.uint8), payload]).cuda()[TC.MEM_LEAD:]
    lo = TC.MEM_LEAD + TC.STREAM_GUARD
    assert src.data_ptr() % 256 == 16
    old = L.gpbs_hip_set_stream_opts(opts)
    try:
        for chunk in TC.mem_chunks(nt, u):
            for n in TC.mem_sizes(nt, u, chunk):
                img = TC.copy_image(payload, n * 16).cuda()
                for grid in TC.MEM_GRIDS:
                    dbuf = torch.full_like(img, TC.COPY_SENTINEL)
                    dst = dbuf[lo:lo + n * 16]
                    assert dst.data_ptr() % 256 == 16
                    K.stream_copy(src[:n * 16], dst, chunk_bytes=chunk * 16, grid=grid)
                    bad = (dbuf != img).nonzero().flatten()
                    assert bad.numel() == 0, (f"opts {opts} chunk {chunk} n {n} grid {grid}: {bad.numel()} bytes differ, "
                                              f"first at payload byte {bad[0].item() - lo} of {n * 16}")
    finally:
        L.gpbs_hip_set_stream_opts(old)


# ---------------------------------------------------------------- reduce ---

_reduce_dev = {}


def _reduce_on_device(n8):
    """Per size, once: a and b as views 16 bytes into their allocations, the
    expected image of the output allocation and its must-be-NaN mask."""
    if n8 not in _reduce_dev:
        a, b, _, _ = TC.reduce_case(n8)
        pad = torch.zeros(TC.MEM_LEAD // 2, dtype=BF)
        img, mask = TC.reduce_image(n8)
        _reduce_dev[n8] = (torch.cat([pad, a]).cuda()[pad.numel():], torch.cat([pad, b]).cuda()[pad.numel():],
                           img.cuda(), mask.cuda())
    return _reduce_dev[n8]


def _reduce_bad(obuf, img, mask):
    """Elements whose bits differ from the image, a NaN of any payload counting
    as equal where the image expects a NaN."""
    return (obuf != img) & ~(mask & obuf.view(BF).isnan())


@pytest.mark.parametrize("opts", TC.REDUCE_OPTS)
def test_reduce_every_variant_at_every_loop_bound(opts):
    """out = a + b, bit-equal to the fp64 sum rounded once to fp32 and then to
    bf16 (NaN results compared as NaN), in all 32 variants, with the size, chunk,
    grid and guard scheme of the copy test relative to the variant's NT * U.
    Planted at both ends of the buffer and in both halves of a 32-bit pair:
    +-0, +-inf, inf - inf, largest finite twice, the ties 256 + 1 -> 256 and
    258 + 1 -> 260, and bf16 subnormals.

    Subnormals: the library is built with -O3 and neither -ffast-math nor
    -fgpu-flush-denormals-to-zero, and the kernel descriptors the compiler
    emits for gfx950 carry float_denorm_mode_32 = 3 (denormal sources and
    results preserved), so v_add_f32 and the conversion to bf16 are IEEE here:
    0x0001 + 0x0001 = 0x0002, and 0x0080 - 0x0001 = 0x007F stays subnormal.
    That is what the expected bits pin."""
    L = K.lib()
    nt, u = TC.reduce_geom(opts)
    lo = (TC.MEM_LEAD + TC.REDUCE_GUARD) // 2
    old = L.gpbs_hip_set_reduce_opts(opts)
    try:
        for chunk in TC.mem_chunks(nt, u):
            for n8 in TC.mem_sizes(nt, u, chunk):
                a, b, img, mask = _reduce_on_device(n8)
                assert a.data_ptr() % 256 == 16 and b.data_ptr() % 256 == 16
                for grid in TC.MEM_GRIDS:
                    obuf = torch.full_like(img, TC.REDUCE_SENTINEL)
                    out = obuf[lo:lo + 8 * n8].view(BF)
                    assert out.data_ptr() % 256 == 16
                    K.reduce_bf16(a, b, out=out, chunk_bytes=chunk * 16, grid=grid)
                    bad = _reduce_bad(obuf, img, mask).nonzero().flatten()
                    if bad.numel():
                        i = bad[0].item()
                        raise AssertionError(
                            f"opts {opts} chunk {chunk} n8 {n8} grid {grid}: {bad.numel()} elements differ, first at "
                            f"element {i - lo} of {8 * n8}: got {obuf[i].item() & 0xFFFF:#06x}, expected "
                            f"{img[i].item() & 0xFFFF:#06x}" + (" (any NaN)" if mask[i].item() else ""))
    finally:
        L.gpbs_hip_set_reduce_opts(old)


# ------------------------------------------------------------------ GEMV ---

def _gemv_checked(Wd, xd, bits, grid, what):
    R = Wd.shape[0]
    img = TC.gemv_image(bits).cuda()
    ybuf = torch.full_like(img, TC.GEMV_SENTINEL)
    y = ybuf.view(torch.float32)[TC.GEMV_GUARD:TC.GEMV_GUARD + R]
    K.gemv_bf16(Wd, xd, out=y, grid=grid)
    bad = (ybuf != img).nonzero().flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} words differ, first at row {bad[0].item() - TC.GEMV_GUARD} of {R}: "
                              f"got {ybuf.view(torch.float32)[bad[0]].item()}, expected "
                              f"{img.view(torch.float32)[bad[0]].item()}")


@pytest.mark.parametrize("R", TC.GEMV_R)
@pytest.mark.parametrize("Kd", TC.GEMV_K)
def test_gemv_integer_operands_bit_exact(Kd, R):
    """Integer W and x in [-8, 8]: the fp32 output is the exact integer.  K runs
    the tail loop alone, one unrolled step and the tail, unrolled steps only;
    R has partial and clamped units, and 257 units on the 256-workgroup cap.
    y is a view into a larger buffer whose sentinels must survive."""
    W, x, bits = TC.gemv_int_case(R, Kd)
    _gemv_checked(W.cuda(), x.cuda(), bits, 0, f"gemv R {R} K {Kd}")


@pytest.mark.parametrize("Kd", TC.GEMV_K)
def test_gemv_one_workgroup_walks_every_unit(Kd):
    W, x, bits = TC.gemv_int_case(TC.GEMV_GRID1_R, Kd)
    _gemv_checked(W.cuda(), x.cuda(), bits, 1, f"gemv R {TC.GEMV_GRID1_R} K {Kd} grid 1")


@pytest.mark.parametrize("Kd", TC.GEMV_K)
def test_gemv_one_hot_x_selects_the_column(Kd):
    """x = e_k gives y = W[:, k], for every k of the first and the last
    512-column chunk: all 8 elements of all 64 lanes' slots."""
    W, ks, cols = TC.gemv_onehot_case(Kd)
    R, G = W.shape[0], TC.GEMV_GUARD
    Wd = W.cuda()
    imgs = torch.stack([TC.gemv_image(c) for c in cols]).cuda()
    xd = torch.zeros(Kd, dtype=BF, device="cuda")
    ybuf = torch.empty(R + 2 * G, dtype=torch.int32, device="cuda")
    y = ybuf.view(torch.float32)[G:G + R]
    nbad = torch.zeros(len(ks), dtype=torch.int64, device="cuda")
    for i, k in enumerate(ks):
        xd.zero_()
        xd[k] = 1
        ybuf.fill_(TC.GEMV_SENTINEL)
        K.gemv_bf16(Wd, xd, out=y)
        nbad[i] = (ybuf != imgs[i]).sum()
    wrong = [ks[i] for i in nbad.cpu().nonzero().flatten().tolist()]
    assert not wrong, f"K {Kd}: y != W[:, k] for {len(wrong)} of {len(ks)} k, first {wrong[:8]}"


@pytest.mark.parametrize("Kd", TC.GEMV_K)
def test_gemv_real_data_within_the_arithmetic_bound(Kd):
    """randn data against fp64, per row within K 2^-23 (|W| @ |x|): exact
    products, fewer than K fp32 additions in an unknown order."""
    R = 1000
    W, x, ref, bound = TC.gemv_real_case(R, Kd)
    y = K.gemv_bf16(W.cuda(), x.cuda()).cpu().double()
    assert torch.isfinite(y).all()
    err = (y - ref).abs()
    print(f"gemv {R} x {Kd}: max err {err.max().item():.4g}, {(err / bound).max().item():.3g} of the bound")
    bad = (err > bound).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} rows outside the bound, first {bad[:4].tolist()}"
