"""CPU: the edge-weight gradient hand-over (ops._handle_grad, _dw_to_add, _report_dw, _take_parked and the three handle backwards'
reads) against the frozen copy of the inline logic it replaced (tests/handover_ref.py), driven side by side over every sequence of one,
two and three reporting layers.  Nothing here loads the library: the side band is host state, the tensors are CPU tensors."""
import itertools
import types
import weakref

import torch

import sgs_gnn_amd
from tests import handover_ref as R

ops = sgs_gnn_amd.ops
N_EDGES = 6
BAND = (("_g_first", None), ("_g_extra", None), ("_dw_first", None), ("_extra_total", False))


class RefNorm:
    """The side band of the Norm as it was: slots that the hand-made constructors filled one by one (an unset one reads as its default
    through getattr, which is how the inline code read them)."""
    __slots__ = ("_g_first", "_g_extra", "_dw_first", "_park_ok", "_extra_total", "__weakref__")


def ref_norm(style, park):
    nm = RefNorm()
    if style == "edge":                 # gat_edge_attr / edge_attr: every field but _dw_first
        nm._park_ok, nm._extra_total = park, False
        nm._g_first = nm._g_extra = None
    elif park:                          # gcn_norm / cheb_norm: _park_ok alone, and only with a handle
        nm._park_ok = True
    return nm


def new_norm(style, park):
    nm = ops.EdgeAttr() if style == "edge" else ops.Norm()
    nm._park_ok = park
    return nm


def band(nm):
    return tuple(getattr(nm, k, d) for k, d in BAND)


def same(a, b):
    """Identical objects (tensors by identity, flags and None by value)."""
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a) or torch.is_tensor(b) or isinstance(a, weakref.ref):
        return a is b
    return a == b and type(a) is type(b)


def test_fresh_norm_and_edge_attr_have_every_slot_set():
    for cls in (ops.Norm, ops.EdgeAttr):
        nm = cls()
        slots = [s for c in cls.__mro__ for s in getattr(c, "__slots__", ()) if s != "__weakref__"]
        assert {"graph", "w", "handle", "_g_first", "_g_extra", "_dw_first", "_park_ok", "_extra_total"} <= set(slots)
        for s in slots:
            assert hasattr(nm, s), f"{cls.__name__}.{s} is unset"
            assert getattr(nm, s) is (False if s in ("_park_ok", "_extra_total") else None), f"{cls.__name__}.{s} is not neutral"
        assert not hasattr(nm, "__dict__")
        weakref.ref(nm)


LAYERS = [(kind, needs) for kind in ("plain", "edge") for needs in (True, False)]
READERS = ("gcn", "gcn_live_dw", "cheb", "edge_attr", "edge_attr_total_flipped")


def run_case(seq, park, match, reader):
    """One backward pass over one shared Norm: the layers of `seq` report in order, then `reader` (the handle's backward) takes what
    was parked.  Both sides see the very same gradient tensors, so what they return and keep can be compared by identity."""
    plain_only = all(kind == "plain" for kind, _ in seq) and reader in ("gcn", "gcn_live_dw", "cheb")
    style = "gcn" if plain_only else "edge"
    ref, new = ref_norm(style, park), new_norm(style, park)
    steps = 0
    for i, (kind, needs) in enumerate(seq):
        numel = N_EDGES + 3 if (i == 0 and not match) else N_EDGES       # (a first gradient of another size: nothing is added to it)
        dw = torch.full((numel,), float(i + 1))
        if kind == "plain":             # the GCN / Chebyshev layers: `_handle_grad(nm, g) if g is not None else None`
            r_ret = R.handle_grad(ref, dw) if needs else None
            n_ret = ops._handle_grad(new, dw) if needs else None
        else:                           # the edge-attribute layers: d w with the other layer's added, then reported
            r_second, r_add = R.layer_dw_add(ref, N_EDGES)
            n_second, n_add = ops._dw_to_add(new, N_EDGES)
            assert bool(r_second) == bool(n_second) and same(r_add, n_add), (seq, park, match, i)
            r_ret = R.layer_report(ref, dw, r_second, needs)
            n_ret = ops._report_dw(new, dw, n_second) if needs else None
        assert same(r_ret, n_ret), (seq, park, match, i)
        assert same(band(ref), band(new)), (seq, park, match, i)
        steps += 1
    g = torch.full((N_EDGES,), 100.0)
    if reader.startswith("gcn"):
        live = torch.zeros(N_EDGES) if reader == "gcn_live_dw" else None
        if live is not None and park:                                      # _HybridLoss.backward parks its d w only on a _park_ok Norm
            ref._dw_first = new._dw_first = weakref.ref(live)
        r_extra, r_first = R.gcn_norm_take(ref)
        n_extra, _, n_first = ops._take_parked(new)
        assert same((r_extra, r_first), (n_extra, n_first)), (seq, park, match, reader)
    elif reader == "cheb":
        assert same(R.cheb_norm_take(ref), ops._take_parked(new)[0]), (seq, park, match, reader)
    else:
        if reader == "edge_attr_total_flipped":                            # both values of `total` against every parked state
            ref._extra_total = new._extra_total = not new._extra_total
        parked = new._g_extra
        r_g = R.edge_attr_backward(ref, g)
        n_g, n_none = ops._GATEdgeAttr.backward(types.SimpleNamespace(nm=new), g)
        assert n_none is None
        if r_g is g or r_g is parked:                                      # handed on as it is: the same object on both sides
            assert n_g is r_g, (seq, park, match, reader)
        else:                                                              # g + extra: a new tensor on each side
            assert n_g is not g and n_g is not parked and torch.equal(r_g, n_g), (seq, park, match, reader)
    assert same(band(ref), band(new)), (seq, park, match, reader)
    assert band(new) == (None, None, None, False), (seq, park, match, reader)   # neutral after the handle's backward
    return steps + 1


def test_handover_matches_the_frozen_inline_logic_over_every_sequence():
    cases = steps = 0
    for n_layers in (1, 2, 3):
        for seq in itertools.product(LAYERS, repeat=n_layers):
            # an edge-attribute layer runs over an EdgeAttr, whose handle is always _GATEdgeAttr's: the other two readers never see one
            readers = READERS if all(kind == "plain" for kind, _ in seq) else READERS[3:]
            for park, match, reader in itertools.product((True, False), (True, False), readers):
                steps += run_case(seq, park, match, reader)
                cases += 1
    assert cases == ((2 + 4 + 8) * 5 + (2 + 12 + 56) * 2) * 2 * 2


def test_second_edge_layer_parks_the_total_and_the_reader_returns_it_as_it_is():
    """The one path the speed-up rests on, spelled out: layer 2 of an edge-attribute head adds layer 1's d w in its kernel, parks the
    sum, and _GATEdgeAttr.backward returns the parked tensor itself (no add)."""
    nm = new_norm("edge", True)
    dw1, dw2 = torch.ones(N_EDGES), torch.full((N_EDGES,), 2.0)
    second, add = ops._dw_to_add(nm, N_EDGES)
    assert not second and add is None and ops._report_dw(nm, dw1, second) is dw1
    second, add = ops._dw_to_add(nm, N_EDGES)
    assert second and add is dw1 and ops._report_dw(nm, dw2, second) is None
    assert nm._g_extra is dw2 and nm._extra_total is True
    out, _ = ops._GATEdgeAttr.backward(types.SimpleNamespace(nm=nm), dw1)
    assert out is dw2 and band(nm) == (None, None, None, False)
