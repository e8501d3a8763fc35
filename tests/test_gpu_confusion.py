"""GPU: sgs_confusion_counts through ops.confusion_counts against a CPU matrix built from torch.argmax of the same logits, by exact integer
equality, in the automatic form and in every forced form the library accepts for the shape.  Shapes: the smallest that reach every code
path -- one row, more than one wave with a ragged last workgroup, hot cells over several grid-stride rounds (4 099 rows of 5 classes: above
the automatic rule's threshold and more than 16 rows per compute unit's workgroup), both sides of lane_argmax's second stride (64 / 65),
both sides of the privatised form's LDS limit (73 / 74) and a wide row.  Half of every matrix holds small integers, so exact ties in every
lane and stride are the rule; constant rows, rows of -inf and ties across the two lane strides are planted on top."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f1_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (1, 2), (67, 3), (4099, 5), (257, 64), (257, 65), (257, 73), (257, 74), (300, 130)]
PRIV_MAX_C = 73


def _logits(N, C, g):
    x = torch.randn(N, C, generator=g)
    half = torch.arange(N) % 2 == 1
    x[half] = torch.randint(0, 3, (N, C), generator=g).float()[half]             # exact ties everywhere
    if N >= 16:
        x[2] = 0.25                                                              # a constant row: class 0
        x[4] = float("-inf")                                                     # nothing exceeds the initial -inf: class 0
        x[6] = -1.0
        x[6, C - 1] = x[6, C // 2] = 7.0                                         # two equal maxima: the first wins
        if C > 64:
            x[8] = -2.0
            x[8, (C - 63) % 64] = x[8, C - 1] = 5.0                              # first maximum in stride 0, an equal one in stride 1 of another lane
            x[10] = -2.0
            x[10, 64] = x[10, 1] = 5.0                                           # lane 0 meets it only in its second stride; lane 1 holds the first
            x[12] = float("-inf")
            x[12, C - 1] = 0.0                                                   # the only finite value sits in the second stride
            x[14] = 1.0
            x[14, 64] = 2.0                                                      # a strict maximum in the second stride beats lane 0's first column
    return x


def _case(N, C, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x = _logits(N, C, g)
    y = torch.randint(0, C, (N,), generator=g)
    u = torch.rand(N, generator=g)
    if kind == "overlap":                 # rows in two splits, rows in none
        masks = [u < 0.4, (u > 0.25) & (u < 0.6), u > 0.8]
    elif kind == "one empty":
        masks = [u < 0.4, torch.zeros(N, dtype=torch.bool), u > 0.5]
    elif kind == "all rows":
        masks = [torch.ones(N, dtype=torch.bool), u < 0.5, torch.ones(N, dtype=torch.bool)]
    else:
        masks = [torch.zeros(N, dtype=torch.bool)] * 3
    outside = ~(masks[0] | masks[1] | masks[2])
    y = y.clone()
    idx = outside.nonzero().flatten()
    y[idx[0::2]] = -100                   # rows outside every mask may hold any label: never read
    y[idx[1::2]] = C
    pred = torch.argmax(x, dim=1)
    want = torch.from_numpy(R.confusion3(y.numpy(), pred.numpy(), [m.numpy() for m in masks], C))
    return x, y, masks, want


def _forms(ops, N, C):
    """(code, form launched) for the automatic choice and every forced form the library accepts for the shape."""
    out = []
    for code in (0, 1, 2):
        ops.confusion_variant_set(code)
        v = ops.confusion_variant(N, C)
        if v > 0:
            out.append((code, v))
    ops.confusion_variant_set(0)
    return out


@pytest.mark.parametrize("N,C", SHAPES)
def test_confusion_counts_exact_in_every_form(N, C):
    import sgs_gnn_amd as S
    ops = S.ops
    try:
        forms = _forms(ops, N, C)
        assert (1, 1) in forms and forms[0][0] == 0                              # the direct form is never refused, nor the automatic one
        assert ((2, 2) in forms) == (C <= PRIV_MAX_C)
        if (N, C) == (4099, 5):
            assert forms[0] == (0, 2)                                            # the automatic rule reaches the privatised form in this file
        if (N, C) == (67, 3):
            assert forms[0] == (0, 1)
        for k, kind in enumerate(("overlap", "one empty", "all rows", "all empty")):
            x, y, masks, want = _case(N, C, kind, 100 * N + C + k)
            xd, yd, md = x.to(DEV), y.to(DEV), [m.to(DEV) for m in masks]
            if kind == "overlap" and N >= 16:
                assert bool((masks[0] & masks[1]).any()) and bool((~(masks[0] | masks[1] | masks[2])).any())
            got = {}
            for code, _ in forms:
                ops.confusion_variant_set(code)
                a = ops.confusion_counts(xd, yd, md)
                assert a.dtype == torch.int64 and a.shape == (3, C, C) and a.device.type == "cuda"
                assert torch.equal(a.cpu(), want), (kind, code)
                b = ops.confusion_counts(xd, yd, md, out=a)                      # the accumulate contract: a second call doubles every cell
                assert b is a and torch.equal(a.cpu(), 2 * want), (kind, code)
                base = torch.arange(3 * C * C, dtype=torch.int64).reshape(3, C, C) * 1000003 + (1 << 33)
                c = base.to(DEV)
                ops.confusion_counts(xd, yd, md, out=c)                          # out= on a non-zero buffer adds to it (64-bit cells)
                assert torch.equal(c.cpu(), base + want), (kind, code)
                got[code] = a.cpu()
            assert all(torch.equal(v, got[0]) for v in got.values())
            if kind == "all empty":
                assert int(want.sum()) == 0
            ops.confusion_variant_set(0)
            for s in range(3):                                                   # consistency with today's kernel, per split
                mc = ops.masked_correct(xd, yd, md[s]).tolist()
                assert [int(want[s].diagonal().sum()), int(want[s].sum())] == mc, (kind, s)
        if C > PRIV_MAX_C:                                                       # forcing the privatised form beyond its LDS limit: refused, not launched
            ops.confusion_variant_set(2)
            buf = torch.full((3, C, C), 5, dtype=torch.int64, device=DEV)
            with pytest.raises(RuntimeError, match="sgs_confusion_counts"):
                ops.confusion_counts(xd, yd, md, out=buf)
            assert bool((buf == 5).all())
    finally:
        ops.confusion_variant_set(0)


def test_confusion_counts_validation_and_empty():
    import sgs_gnn_amd as S
    ops = S.ops
    x = torch.randn(5, 3, device=DEV)
    y = torch.zeros(5, dtype=torch.int64, device=DEV)
    m = torch.ones(5, dtype=torch.bool, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.confusion_counts(x.cpu(), y, (m, m, m))
    with pytest.raises(RuntimeError, match="dtype"):
        ops.confusion_counts(x.double(), y, (m, m, m))
    with pytest.raises(RuntimeError, match="dtype"):
        ops.confusion_counts(x, y.int(), (m, m, m))
    with pytest.raises(RuntimeError, match="bool"):
        ops.confusion_counts(x, y, (m, m, m.float()))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.confusion_counts(x, y, (m, m, m), out=torch.zeros(3, 4, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="one entry per row"):
        ops.confusion_counts(x, y[:4], (m, m, m))
    e = ops.confusion_counts(x[:0], y[:0], (m[:0], m[:0], m[:0]))                # N = 0: zeros, nothing launched
    assert e.shape == (3, 3, 3) and int(e.sum()) == 0
    nc = ops.confusion_counts(x.t().contiguous().t(), y, (m, m, m))              # non-contiguous logits are copied, as masked_correct does
    assert torch.equal(nc, ops.confusion_counts(x, y, (m, m, m)))
    u8 = ops.confusion_counts(x, y, (m.view(torch.uint8), m, m))                 # uint8 masks are taken as they are
    assert torch.equal(u8, nc)
