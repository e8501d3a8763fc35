"""GPU: sgs_gemm_tn_group -- several weight-gradient products C = A^T B in one launch -- against the single calls, bit for bit.

The grouped kernel runs the single kernel's workgroup body on a tile it looks up in a descriptor block, so every C must EQUAL what
sgs_gemm_tn / sgs_gemm_tn_ld writes (torch.equal, no tolerance).  Every case asserts through sgs_gemm_tn_group_supported that its
problems take the path they are meant to: a fallback to the single launcher must not pass for a grouped launch."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

KS = (512, 513, 1013)                                  # the <16> threshold, an odd length (even-slice rounding, K tail), the bench's K
SHAPES = ((41, 256), (256, 70), (33, 31), (256, 256))   # partial tiles in M, in N, in both (one 2 x 1 .. a single-tile N), whole tiles
FILL = -7.25                                            # what a C holds before a call: no product of the operands below gives it


@pytest.fixture(scope="module")
def pkg():
    import sgs_gnn_amd
    return sgs_gnn_amd


@pytest.fixture(scope="module")
def operands():
    """Deterministic fp32 operands, made once: a problem (K, M, N) reads the leading K rows and a column window (from column `shift`)
    of A [1013, 258] and B [1013, 258], copied contiguous (cached per shape)."""
    g = torch.Generator(device=DEV).manual_seed(20)
    A = torch.randn(1013, 258, generator=g, device=DEV)
    B = torch.randn(1013, 258, generator=g, device=DEV)
    cache = {}

    def get(K, M, N, shift=0):
        key = (K, M, N, shift)
        if key not in cache:
            cache[key] = (A[:K, shift:shift + M].contiguous(), B[:K, shift:shift + N].contiguous())
        return cache[key]
    return get


def _single(pkg, A, B, K, M, N, C, ldc=0, col0=0):
    L, ops = pkg._lib.lib(), pkg.ops
    ws = ops.workspace(L.sgs_gemm_tn_workspace_bytes(K, M, N), A.device)
    ptr = C.data_ptr() + 4 * col0
    if ldc:
        pkg._lib.check(L.sgs_gemm_tn_ld(A.data_ptr(), B.data_ptr(), K, M, N, ptr, ldc, None, ws.data_ptr(), ws.numel(), ops._stream()), "sgs_gemm_tn_ld")
    else:
        pkg._lib.check(L.sgs_gemm_tn(A.data_ptr(), B.data_ptr(), K, M, N, ptr, ws.data_ptr(), ws.numel(), ops._stream()), "sgs_gemm_tn")


def _group(pkg, probs):
    """probs: (A, B, K, M, N, C, ldc, col0, ws | None) -> one sgs_gemm_tn_group call (SgsGemmTnProblem: nine 64-bit words each)."""
    L = pkg._lib.lib()
    words = []
    for A, B, K, M, N, C, ldc, col0, ws in probs:
        words += [A.data_ptr(), B.data_ptr(), K, M, N, C.data_ptr() + 4 * col0, ldc, ws.data_ptr() if ws is not None else 0,
                  ws.numel() if ws is not None else 0]
    arr = (ctypes.c_int64 * len(words))(*words)
    pkg._lib.check(L.sgs_gemm_tn_group(arr, len(probs), pkg.ops._stream()), "sgs_gemm_tn_group")


def _expect(pkg, operands, shapes):
    """[(A, B, K, M, N, C_ref)] with C_ref from the single call, and the empty Cs of the same shapes for the grouped call."""
    ref, out = [], []
    for i, (K, M, N) in enumerate(shapes):
        A, B = operands(K, M, N, shift=i % 3)
        C = torch.full((M, N), FILL, device=DEV)
        _single(pkg, A, B, K, M, N, C)
        ref.append((A, B, K, M, N, C))
        out.append(torch.full((M, N), FILL, device=DEV))
    return ref, out


def test_query_names_the_single_launchers_path(pkg):
    """(runs without computing: the query is a pure host function)"""
    L = pkg._lib.lib()
    for K, (M, N) in itertools.product(KS, SHAPES):
        assert L.sgs_gemm_tn_group_supported(K, M, N) == 16, (K, M, N)
    assert L.sgs_gemm_tn_group_supported(1013, 256, 602) == 16 and L.sgs_gemm_tn_group_supported(1013, 41, 256) == 16     # the bench's shapes
    assert L.sgs_gemm_tn_group_supported(511, 256, 256) == 4 and L.sgs_gemm_tn_group_supported(300, 64, 64) == 4
    assert L.sgs_gemm_tn_group_supported(130, 32, 32) == 2
    assert L.sgs_gemm_tn_group_supported(100, 41, 256) == 0          # one K-slice: the tile kernel
    assert L.sgs_gemm_tn_group_supported(100000, 256, 256) == 0      # tall K
    assert L.sgs_gemm_tn_group_supported(1013, 0, 256) == 0 and L.sgs_gemm_tn_group_supported(0, 32, 32) == 0


@pytest.mark.parametrize("K", KS)
def test_every_shape_alone_and_all_four_together(pkg, operands, K):
    L = pkg._lib.lib()
    shapes = [(K, M, N) for M, N in SHAPES]
    assert all(L.sgs_gemm_tn_group_supported(*s) == 16 for s in shapes)
    ref, out = _expect(pkg, operands, shapes)
    for (A, B, K_, M, N, Cr), C in zip(ref, out):                  # count = 1
        _group(pkg, [(A, B, K_, M, N, C, 0, 0, None)])
        assert torch.equal(C, Cr), (K_, M, N)
        C.fill_(FILL)
    _group(pkg, [(A, B, K_, M, N, C, 0, 0, None) for (A, B, K_, M, N, _), C in zip(ref, out)])      # count = 4
    for (_, _, K_, M, N, Cr), C in zip(ref, out):
        assert torch.equal(C, Cr), (K_, M, N)


@pytest.mark.parametrize("count", [2, 5, 8])
def test_mixed_shapes_and_lengths_in_one_call(pkg, operands, count):
    L = pkg._lib.lib()
    every = [(K, M, N) for K, (M, N) in itertools.product(KS, SHAPES)]
    shapes = [every[(5 * i + count) % len(every)] for i in range(count)]            # a fixed mix of Ks and shapes, K changing inside the call
    assert len({s[0] for s in shapes}) > 1
    assert all(L.sgs_gemm_tn_group_supported(*s) == 16 for s in shapes)
    ref, out = _expect(pkg, operands, shapes)
    _group(pkg, [(A, B, K, M, N, C, 0, 0, None) for (A, B, K, M, N, _), C in zip(ref, out)])
    for (_, _, K, M, N, Cr), C in zip(ref, out):
        assert torch.equal(C, Cr), (K, M, N)


def test_strided_output_leaves_the_other_half_alone(pkg, operands):
    """ldc = 2 N: the right half of a wider matrix (d fc1.weight's W1b block), beside a dense problem in the same call."""
    L = pkg._lib.lib()
    K, M, N = 1013, 256, 256
    assert L.sgs_gemm_tn_group_supported(K, M, N) == 16 and L.sgs_gemm_tn_group_supported(K, 41, 256) == 16
    A, B = operands(K, M, N)
    A2, B2 = operands(K, 41, 256, shift=1)
    wide_ref, wide = torch.full((M, 2 * N), FILL, device=DEV), torch.full((M, 2 * N), FILL, device=DEV)
    _single(pkg, A, B, K, M, N, wide_ref, ldc=2 * N, col0=N)
    C2_ref, C2 = torch.full((41, 256), FILL, device=DEV), torch.full((41, 256), FILL, device=DEV)
    _single(pkg, A2, B2, K, 41, 256, C2_ref)
    _group(pkg, [(A2, B2, K, 41, 256, C2, 0, 0, None), (A, B, K, M, N, wide, 2 * N, N, None)])
    assert torch.equal(wide[:, N:], wide_ref[:, N:]) and torch.equal(C2, C2_ref)
    assert bool((wide[:, :N] == FILL).all()) and not bool((wide[:, N:] == FILL).any())


def test_other_shapes_in_the_list_take_the_single_path(pkg, operands):
    """K = 100 has one K-slice (no workgroup-per-tile kernel): the call hands it to the single launcher, with its workspace."""
    L, ops = pkg._lib.lib(), pkg.ops
    shapes = [(1013, 41, 256), (100, 41, 256), (513, 33, 31)]
    assert [L.sgs_gemm_tn_group_supported(*s) for s in shapes] == [16, 0, 16]
    ref, out = _expect(pkg, operands, shapes)
    ws = torch.empty(L.sgs_gemm_tn_workspace_bytes(100, 41, 256), dtype=torch.uint8, device=DEV)
    _group(pkg, [(A, B, K, M, N, C, 0, 0, ws if K == 100 else None) for (A, B, K, M, N, _), C in zip(ref, out)])
    for (_, _, K, M, N, Cr), C in zip(ref, out):
        assert torch.equal(C, Cr), (K, M, N)
    # ... and without one it reports the error instead of computing nothing
    with pytest.raises(RuntimeError, match="workspace"):
        _group(pkg, [ref[1][:5] + (out[1], 0, 0, None)])


def test_smaller_workgroups_group_too(pkg, operands):
    """K < 512: the 4- and 2-wave forms of the kernel; problems of different workgroup sizes in one call go to one launch each."""
    L = pkg._lib.lib()
    shapes = [(300, 33, 31), (130, 32, 32), (511, 256, 70), (1013, 41, 256)]
    assert [L.sgs_gemm_tn_group_supported(*s) for s in shapes] == [4, 2, 4, 16]
    ref, out = _expect(pkg, operands, shapes)
    _group(pkg, [(A, B, K, M, N, C, 0, 0, None) for (A, B, K, M, N, _), C in zip(ref, out)])
    for (_, _, K, M, N, Cr), C in zip(ref, out):
        assert torch.equal(C, Cr), (K, M, N)


def test_same_call_twice_gives_the_same_bits(pkg, operands):
    L = pkg._lib.lib()
    shapes = [(1013, 256, 256), (1013, 41, 256), (513, 256, 70), (512, 33, 31), (1013, 256, 70)]
    assert all(L.sgs_gemm_tn_group_supported(*s) == 16 for s in shapes)
    runs = []
    for _ in range(2):
        probs = []
        for i, (K, M, N) in enumerate(shapes):
            A, B = operands(K, M, N, shift=i % 3)
            probs.append((A, B, K, M, N, torch.full((M, N), FILL, device=DEV), 0, 0, None))
        _group(pkg, probs)
        runs.append([p[5] for p in probs])
    for C0, C1 in zip(*runs):
        assert torch.equal(C0, C1) and not bool((C0 == FILL).any())
