"""The fixtures of tests/tenant_cases.py do what they claim: the exactness
premises hold, the k-select maps hit what they must, no GEMM reference has a
constant tile or two equal ones, the planted values of the reduce case sit
where it says with the bits IEEE arithmetic gives them, and the shape lists
still contain every edge class.  Everything that can be checked without a
GPU; tests/test_gpu_tenant_exact.py is the GPU side."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tenant_cases as TC  # noqa: E402

BF = TC.BF
KSELECT = [(s, d) for s in TC.GEMM_SHAPES for d in "ab"]


def _u16(t):
    return t.view(torch.int16).to(torch.int32) & 0xFFFF


# ------------------------------------------------------------------ GEMM ---

@pytest.mark.parametrize("shape", TC.GEMM_SHAPES)
def test_integer_gemm_cases_are_exact_in_fp32(shape):
    A, B, ref, bits = TC.int_case(*shape)
    assert A.dtype == B.dtype == BF and A.shape == (shape[0], shape[2]) and B.shape == (shape[1], shape[2])
    assert A.float().abs().max() <= 8 and B.float().abs().max() <= 8
    assert torch.equal(A.float(), A.float().round()) and torch.equal(B.float(), B.float().round())
    assert (A.double().abs() @ B.double().abs().t()).max().item() < 2 ** 24
    assert torch.equal(ref, ref.round()) and torch.equal(ref.float().double(), ref)
    assert not (_u16(bits) == TC.GEMM_SENTINEL).any() and torch.isfinite(ref).all()


def test_integer_gemm_cases_pin_round_to_nearest_even():
    """Some sums lie exactly between two bf16 values, with the even neighbour
    below and above: truncation, round-half-up and round-half-away all differ
    from the expected bits somewhere."""
    down = up = inexact = 0
    for shape in TC.GEMM_SHAPES:
        _, _, ref, bits = TC.int_case(*shape)
        r = bits.view(BF).double()
        inexact += int((r != ref).sum())
        # a tie: ref lies half a bf16 step (2^-7 of its binade) from the rounded value
        ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=1))) - 7)
        tie = (ref - r).abs() * 2 == ulp
        down += int((tie & (r.abs() < ref.abs())).sum())
        up += int((tie & (r.abs() > ref.abs())).sum())
    assert inexact > 1000 and down > 50 and up > 50, (inexact, down, up)


@pytest.mark.parametrize("shape", TC.GEMM_SHAPES)
def test_kselect_map_hits_every_position_and_every_ktile_in_every_half(shape):
    M, N, K = shape
    nk = K // 64
    for rows in (M, N):
        f = TC.kselect_f(rows, K)
        assert f.shape == (rows,) and int(f.min()) >= 0 and int(f.max()) < K
        for h in range(0, rows, 128):
            blk = f[h:h + 128]
            assert sorted(set((blk % 64).tolist())) == list(range(64)), (rows, h)
            assert sorted(set((blk // 64).tolist())) == list(range(nk)), (rows, h)
            # all 8 chunks x 8 elements, spelled out: the swizzles XOR the chunk index
            assert {(p // 8, p % 8) for p in (blk % 64).tolist()} == {(c, e) for c in range(8) for e in range(8)}


@pytest.mark.parametrize("shape,direction", KSELECT)
def test_kselect_cases_select_what_they_say(shape, direction):
    M, N, K = shape
    A, B, ref, bits = TC.kselect_case(M, N, K, direction)
    hot, code, f = (A, B, TC.kselect_f(M, K)) if direction == "a" else (B, A, TC.kselect_f(N, K))
    assert torch.equal(hot.float().sum(1), torch.ones(hot.shape[0])) and set(hot.float().unique().tolist()) == {0.0, 1.0}
    assert torch.equal(hot.float().argmax(1), f)
    c = code.float()
    assert c.abs().max() <= 125 and torch.equal(c, c.round()) and c.min() < -100 and c.max() > 100
    assert (A.double().abs() @ B.double().abs().t()).max().item() < 2 ** 24
    assert torch.equal(ref, TC.gemm_ref64(A, B))            # the indexing is the product
    assert torch.equal(bits.view(BF).double(), ref)          # and exact in bf16
    m, n = M - 3, N - 2
    assert ref[m, n].item() == (B[n, f[m]] if direction == "a" else A[m, f[n]]).item()


def test_coded_operand_is_not_symmetric():
    c = TC.coded(128, 128).float()
    assert (c != c.t()).float().mean().item() > 0.9


@pytest.mark.parametrize("shape", TC.GEMM_SHAPES + TC.REAL_SHAPES)
def test_no_gemm_reference_has_a_constant_tile_or_two_equal_ones(shape):
    """At 128 x 128, which also covers the 256 x 256 tiles: a tile written to
    the wrong place, or not at all, cannot match."""
    refs = [TC.real_case(*shape)[2]] if shape in TC.REAL_SHAPES else \
        [TC.int_case(*shape)[2], TC.kselect_case(*shape, "a")[2], TC.kselect_case(*shape, "b")[2]]
    for ref in refs:
        tiles = TC.tiles_of(ref, 128)
        assert len(tiles) == (shape[0] // 128) * (shape[1] // 128)
        assert len(set(tiles)) == len(tiles)
        for i in range(0, shape[0], 128):
            for j in range(0, shape[1], 128):
                t = ref[i:i + 128, j:j + 128]
                assert t.min() != t.max()
                # nor is a tile the sentinel-free image of its own transpose
                assert not torch.equal(t, t.t())


@pytest.mark.parametrize("shape", TC.REAL_SHAPES)
def test_real_gemm_bound_is_the_stated_one(shape):
    A, B, ref, bound = TC.real_case(*shape)
    K = shape[2]
    S = A.double().abs() @ B.double().abs().t()
    assert torch.equal(bound, 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * S)
    assert torch.equal(ref, A.double() @ B.double().t())
    # tighter everywhere than the 2e-2 max|ref| + 1e-2 of the tolerance test, and a
    # dropped 32-k sub-step (error ~ sqrt(32)) lands outside it for most elements
    assert bound.max().item() < 0.5 * (2e-2 * ref.abs().max().item() + 1e-2)
    assert bound.median().item() < 0.5 * 32 ** 0.5


def test_gemm_shape_lists_contain_the_edge_classes():
    for M, N, K in TC.G256_SHAPES:
        assert TC.is_g256(M, N) and K % 64 == 0
    for M, N, K in TC.G128_SHAPES:
        assert not TC.is_g256(M, N) and M % 128 == 0 and N % 128 == 0 and K % 64 == 0
    assert TC.GEMM_SHAPES == TC.G256_SHAPES + TC.G128_SHAPES
    one = [K // 64 for M, N, K in TC.G256_SHAPES if (M, N) == (256, 256)]
    assert sorted(one) == [1, 2, 3, 4]                     # prologue only, both buffers, buffer parity
    units = {s: TC.gemm_units(s[0], s[1]) for s in TC.G256_MULTI}
    assert sorted(units.values()) == [4, 8, 12]
    for (M, N, K), n in units.items():
        tm, tn = M // 256, N // 256
        engages = tm % 4 == 0 and tn % 2 == 0 and n % 8 == 0
        assert engages == (n == 8)                          # 2-D blocks: on at 8 tiles, row-major at 4 and 12
    assert 12 % 8 != 0 and any(n % 8 for n in units.values())
    assert set(TC.G256_GRIDS) == {0, 1, 3} and set(TC.G256_OPTS) == {8, 9, 0, 1}
    assert all(max(g for g in TC.G256_GRIDS) < n for n in units.values())  # several tiles per workgroup
    # 128 x 128: one tile at 1 and 2 K-tiles, 3 column panels, nine row panels (groups of 8 and 1)
    assert (128, 128, 64) in TC.G128_SHAPES and (128, 128, 128) in TC.G128_SHAPES
    assert any(M == 128 and N // 128 == 3 and K // 64 == 3 for M, N, K in TC.G128_SHAPES)
    nine = [(M, N, K) for M, N, K in TC.G128_SHAPES if M // 128 > 8 and (M // 128) % 8]
    assert {N // 128 for M, N, K in nine} == {1, 3} and all(M // 128 == 9 for M, N, K in nine)
    assert set(TC.G128_GRIDS) == {0, 1, 5}
    assert TC.REAL_SHAPES == [(256, 256, 4096), (384, 128, 1024)]
    assert TC.is_g256(*TC.REAL_SHAPES[0][:2]) and not TC.is_g256(*TC.REAL_SHAPES[1][:2])


# ------------------------------------------------- stream copy and reduce ---

def _mem_classes(nt, u):
    P = nt * u
    chunks = TC.mem_chunks(nt, u)
    assert chunks == [1, 256, P, P + 1]
    for c in chunks:
        sizes = TC.mem_sizes(nt, u, c)
        for want in (1, 255, 256, 257, nt - 1, nt, nt + 1, P, P + 1, 3 * c + 17):
            assert want in sizes, (nt, u, c, want)
        n = 3 * c + 17
        assert (n + c - 1) // c > max(TC.MEM_GRIDS) and (n % c != 0 or c == 1)   # more chunks than workgroups, ragged


def test_stream_sweep_contains_the_edge_classes():
    assert TC.STREAM_OPTS == (0, 1, 2, 3) and TC.MEM_GRIDS == (0, 1, 3) and TC.MEM_LEAD == 16
    assert [TC.stream_geom(o) for o in TC.STREAM_OPTS] == [(256, 16), (256, 16), (256, 8), (256, 8)]
    for o in TC.STREAM_OPTS:
        nt, u = TC.stream_geom(o)
        _mem_classes(nt, u)
        assert TC.STREAM_GUARD >= max(TC.mem_chunks(nt, u)) * 16
        assert max(max(TC.mem_sizes(nt, u, c)) for c in TC.mem_chunks(nt, u)) <= TC.STREAM_MAX_VEC
    assert TC.STREAM_GUARD % 256 == 0


def test_stream_payload_and_image():
    p = TC.stream_payload()
    assert p.dtype == torch.uint8 and p.numel() == (TC.STREAM_MAX_VEC + 1) * 16
    f = p.view(torch.float32)
    assert int(f.isnan().sum()) > 100 and int(f.isinf().sum()) >= 0     # NaN bit patterns travel as integers
    assert not (p.view(-1, 16) == TC.COPY_SENTINEL).all(1).any()        # no payload vector looks like a guard
    v = p.view(-1, 16)
    assert not (v[1:] == v[:-1]).all(1).any()                           # nor like its neighbour
    n = 257 * 16
    img = TC.copy_image(p, n)
    lo = TC.MEM_LEAD + TC.STREAM_GUARD
    assert img.numel() == lo + n + TC.STREAM_GUARD and lo % 256 == 16
    assert (img[:lo] == TC.COPY_SENTINEL).all() and (img[lo + n:] == TC.COPY_SENTINEL).all()
    assert torch.equal(img[lo:lo + n], p[:n])


def test_reduce_sweep_contains_the_edge_classes():
    assert TC.REDUCE_OPTS == tuple(range(32))
    geoms = {TC.reduce_geom(o) for o in TC.REDUCE_OPTS}
    assert geoms == {(nt, u) for nt in (256, 512) for u in (6, 8, 4, 12)}
    for o in TC.REDUCE_OPTS:
        nt, u = TC.reduce_geom(o)
        assert nt == (512 if o & 16 else 256) and u == (6, 8, 4, 12)[o & 3]
    for nt, u in geoms:
        _mem_classes(nt, u)
        assert TC.REDUCE_GUARD >= max(TC.mem_chunks(nt, u)) * 16
        assert max(max(TC.mem_sizes(nt, u, c)) for c in TC.mem_chunks(nt, u)) <= TC.REDUCE_MAX_VEC
    assert TC.REDUCE_GUARD % 256 == 0


def _bf(bits):
    return TC._bits(bits).view(BF).double().item()


def test_reduce_planted_rows_mean_what_their_comments_say():
    big, tiny = _bf(0x7F7F), 2.0 ** -133
    assert big == 2.0 ** 127 * (2 - 2.0 ** -7) and _bf(0x0001) == tiny and _bf(0x0080) == 2.0 ** -126
    assert (_bf(0x4380), _bf(0x4381), _bf(0x4382), _bf(0x3F80)) == (256, 258, 260, 1)
    kinds = {"zero": 0, "inf": 0, "nan": 0, "overflow": 0, "tie": 0, "sub": 0}
    for k, (a, b, r) in enumerate(TC.REDUCE_PLANTED):
        x, y = _bf(a), _bf(b)
        s = x + y
        if r is None:
            assert s != s
            kinds["nan"] += 1
            continue
        want = _bf(r)
        if abs(x) == float("inf"):
            assert want == s
            kinds["inf"] += 1
        elif abs(s) >= 2.0 ** 128 * (1 - 2.0 ** -25):         # rounds to inf in fp32
            assert abs(want) == float("inf") and abs(x) == big
            kinds["overflow"] += 1
        elif s == 0:
            assert want == 0 and (r == 0x8000) == (a == 0x8000 and b == 0x8000)
            kinds["zero"] += 1
        elif abs(s) in (257, 259):
            assert abs(want) in (256, 260) and abs(want - s) == 1
            kinds["tie"] += 1
        else:
            assert k in TC.REDUCE_SUBNORMAL_ROWS and want == s and abs(s) <= 2.0 ** -126
            assert min(abs(x), abs(y)) < 2.0 ** -126
            kinds["sub"] += 1
    assert kinds == {"zero": 3, "inf": 3, "nan": 2, "overflow": 2, "tie": 4, "sub": 5}, kinds
    assert any(0 < abs(_bf(r)) < 2.0 ** -126 for _, _, r in TC.REDUCE_PLANTED if r is not None)  # subnormal results


@pytest.mark.parametrize("n8", [1, 9, 10, 255, 257, 1024, 3 * 6145 + 17])
def test_reduce_case_plants_both_halves_and_both_ends_and_fp64_gives_the_bits(n8):
    a, b, bits, nan = TC.reduce_case(n8)
    n = 8 * n8
    assert a.shape == b.shape == bits.shape == nan.shape == (n,) and a.dtype == BF
    at = TC.reduce_planted_at(n)
    L = len(TC.REDUCE_PLANTED)
    assert at[0] == (0, 0) and len(at) == (min(n, 2 * L) if n < 4 * L else 4 * L)
    for i, row in at:
        pa, pb, pr = TC.REDUCE_PLANTED[row]
        assert int(_u16(a)[i]) == pa and int(_u16(b)[i]) == pb, (i, row)
        if pr is None:
            assert bool(nan[i])
        else:
            assert int(_u16(bits)[i]) == pr and not bool(nan[i]), (i, row, hex(int(_u16(bits)[i])))
    if n >= 4 * L:
        assert at[-1] == (n - 1, L - 1)
        for row in range(L):                                  # low and high half of a 32-bit pair, at each end
            where = [i for i, r in at if r == row]
            assert {i % 2 for i in where if i < n // 2} == {0, 1} and {i % 2 for i in where if i >= n // 2} == {0, 1}
    # the reference is the IEEE sum everywhere, and nothing looks like a guard
    ref = (a.double() + b.double()).float().to(BF)
    assert torch.equal(ref.view(torch.int16)[~nan], bits[~nan]) and torch.equal(ref.isnan(), nan)
    assert not (_u16(bits) == TC.REDUCE_SENTINEL).any()
    if n8 >= 255:
        assert int((bits.view(BF).double()[~nan] != (a.double() + b.double())[~nan]).sum()) > n // 4   # most sums round
    img, mask = TC.reduce_image(n8)
    lead = (TC.MEM_LEAD + TC.REDUCE_GUARD) // 2
    assert img.numel() == lead + n + TC.REDUCE_GUARD // 2 and (2 * lead) % 256 == 16
    assert (img[:lead] == TC.REDUCE_SENTINEL).all() and (img[lead + n:] == TC.REDUCE_SENTINEL).all()
    assert torch.equal(img[lead:lead + n], bits) and torch.equal(mask[lead:lead + n], nan) and not mask[:lead].any()


# ------------------------------------------------------------------ GEMV ---

def test_gemv_lists_contain_the_edge_classes():
    assert [k // 512 for k in TC.GEMV_K] == [1, 3, 4]      # tail only; unrolled step + tail; unrolled only (GV_U = 2)
    assert set(TC.GEMV_R) == {1, 15, 16, 17, 1000, 4097}
    assert (4097 + 15) // 16 == 257 and TC.GEMV_GRID1_R == 100
    assert TC.GEMV_ONEHOT_R == 17                                       # two units, clamped rows in the second
    assert TC.GEMV_GUARD >= 1 and TC.GEMV_GUARD % 4 != 0                  # y is 4-byte aligned only
    for K in TC.GEMV_K:
        ks = TC.gemv_onehot_ks(K)
        assert set(range(512)) <= set(ks) and set(range(K - 512, K)) <= set(ks)
        assert {(k % 512) // 8 for k in ks} == set(range(64)) and {k % 8 for k in ks} == set(range(8))


@pytest.mark.parametrize("K", TC.GEMV_K)
def test_gemv_cases_are_exact(K):
    for R in TC.GEMV_R + (TC.GEMV_GRID1_R,):
        W, x, bits = TC.gemv_int_case(R, K)
        assert W.shape == (R, K) and x.shape == (K,) and W.float().abs().max() <= 8 and x.float().abs().max() <= 8
        assert (W.double().abs() @ x.double().abs()).max().item() < 2 ** 24
        y = bits.view(torch.float32).double()
        assert torch.equal(y, W.double() @ x.double()) and torch.equal(y, y.round())
        assert not (bits == TC.GEMV_SENTINEL).any()
    W, ks, cols = TC.gemv_onehot_case(K)
    assert W.float().abs().max() <= 125 and cols.shape == (len(ks), TC.GEMV_ONEHOT_R)
    assert torch.equal(cols.view(torch.float32), W.float()[:, ks].t())
    c = cols.view(torch.float32)
    assert len({bytes(r.numpy().tobytes()) for r in c}) == len(ks)        # every column differs: a wrong k shows
    img = TC.gemv_image(cols[0])
    G = TC.GEMV_GUARD
    assert (img[:G] == TC.GEMV_SENTINEL).all() and (img[-G:] == TC.GEMV_SENTINEL).all() and torch.equal(img[G:-G], cols[0])
    W, x, ref, bound = TC.gemv_real_case(1000, K)
    assert torch.equal(bound, K * 2.0 ** -23 * (W.double().abs() @ x.double().abs())) and bound.min() > 0
    assert torch.equal(ref, W.double() @ x.double())
