"""CPU: the edge scorer's path plans (ops._plan_forward, ops._plan_backward) and its active-row prologue (ops._active_rows) against the
frozen copy of the code they replaced (tests/scorer_plan_ref.py).  The library is loaded for its host functions only (the
*_supported / can_colsum answers and the variant getters / setters); no tensor reaches it.

The grid is the product of E, n in SIZES, H in HIDDEN, N in NODES, pairs given or not, codes wanting a gradient or not, precision,
the three switches (eight settings), the variant overrides (default / forward set / backward set), mask kept or not, src_sorted,
and ascending (True / False / no active set).  A plan sees only its own arguments, so the product factorises: the forward plan is
compared over the product of what it reads, the backward plan over the product of what it reads (precision enters the backward as
the bf16 flag the forward recorded, free of `kept` here: the frozen code guards that combination itself and so must the plan)."""
import itertools

import pytest
import torch

import sgs_gnn_amd
from tests import scorer_plan_ref as R

ops = sgs_gnn_amd.ops
SIZES = (0, 1, 65535, 65536, 100003)
HIDDEN = (6, 8, 64, 100, 128, 256, 320, 1024)
NODES = (7, 777)
SWITCHES = list(itertools.product((True, False), repeat=3))             # (_mask_backward, _fwd_mask, _fused_backward)
VARIANTS = {"default": (-1, -1), "forward_set": (3, -1), "backward_set": (-1, 0)}
BOOL = (False, True)


@pytest.fixture(scope="module")
def L():
    return sgs_gnn_amd._lib.lib()


class _Settings:
    """The module switches and the library's variant overrides, set for a block and put back."""

    def __init__(self, L, sw, variants):
        self.L, self.sw, self.variants = L, sw, variants

    def __enter__(self):
        self.prev_sw = (ops._mask_backward, ops._fwd_mask, ops._fused_backward)
        self.prev_var = (self.L.sgs_edge_score_get_variant(), self.L.sgs_edge_score_get_bwd_variant())
        ops._mask_backward, ops._fwd_mask, ops._fused_backward = self.sw
        self.L.sgs_edge_score_set_variant(self.variants[0])
        self.L.sgs_edge_score_set_bwd_variant(self.variants[1])

    def __exit__(self, *exc):
        ops._mask_backward, ops._fwd_mask, ops._fused_backward = self.prev_sw
        self.L.sgs_edge_score_set_variant(self.prev_var[0])
        self.L.sgs_edge_score_set_bwd_variant(self.prev_var[1])
        return False


def forward_entries(plan):
    """What _EdgeScore.forward does with a plan: one call, _call(L, _FWD_ENTRY[form], bf16, ...)."""
    return [ops._FWD_ENTRY[plan.form] + ("_bf16" if plan.bf16 else "")]


def backward_entries(plan):
    """What the bodies do with a plan (ops._score_bwd_dense / _score_bwd_mask / _score_bwd_fused and the shared tail), entry by entry."""
    b = "_bf16" if plan.bf16 else ""
    if plan.form == "dense":
        calls = (["sgs_edge_score_bwd_core"] if plan.core else []) + (["sgs_edge_score_bwd_dfeat"] if plan.row_gemm else [])
        calls += ["sgs_gemm_tn_ld"] + ([] if plan.fused_colsum else ["sgs_colsum"]) + ["sgs_colsum", "sgs_colsum"]
        calls += ["sgs_endpoint_reduce_pair"] if plan.pair_reduce else ["sgs_endpoint_reduce", "sgs_endpoint_reduce"]
    elif plan.form == "fused":
        calls = ["sgs_edge_score_bwd_prep_sd_pack" + b, "sgs_edge_score_bwd_dfeat_fused_packed" + b, "sgs_gemm_tn_mask_gather" + b,
                 "sgs_edge_score_bwd_reduce_fused", "sgs_edge_score_dw2_from_parts"]
    else:
        first, last = {"kept": ("sgs_edge_score_bwd_prep", "sgs_edge_score_dw2_from_parts"), "recompute": ("sgs_edge_score_bwd_core_bits", None)}[plan.form]
        calls = [first, "sgs_edge_score_bwd_dfeat_bits" + b, "sgs_gemm_tn_mask" + b] + ([] if last else ["sgs_colsum"])
        calls += ["sgs_endpoint_reduce_pair_bits"] + ([last] if last else [])
    return calls + ["sgs_gemm_tn_ld"]


def forward_grid():
    return itertools.product(SIZES, HIDDEN, NODES, BOOL, BOOL, ops.PRECISIONS, BOOL)


def backward_grid():
    return itertools.product(SIZES, HIDDEN, NODES, BOOL, BOOL, BOOL, BOOL, (None, False, True))


def forward_form(entries):
    return entries[0]


def backward_form(entries):
    """The form a list of entry points stands for, the dense form with its two sub-choices that change the list's kernels."""
    b = "_bf16" if any(e.endswith("_bf16") for e in entries) else ""
    if "sgs_edge_score_bwd_core_bits" in entries:
        return "recompute"
    if "sgs_edge_score_bwd_prep" in entries:
        return "kept" + b
    if "sgs_edge_score_bwd_prep_sd_pack" + b in entries:
        return "fused" + b
    row_gemm = "sgs_edge_score_bwd_dfeat" in entries
    fused_colsum = entries.count("sgs_colsum") == 2
    return f"dense/row_gemm={row_gemm}", f"dense/fused_colsum={fused_colsum}"


WANT_FORWARD = {f + b for f in ("sgs_edge_score_fwd_mask", "sgs_edge_score_fwd_paired", "sgs_edge_score_fwd") for b in ("", "_bf16")}
WANT_BACKWARD = {"recompute", "kept", "kept_bf16", "fused", "fused_bf16", "dense/row_gemm=True", "dense/row_gemm=False", "dense/fused_colsum=True",
                 "dense/fused_colsum=False"}


def _note(seen, form):
    seen.update(form if isinstance(form, tuple) else (form,))


def test_the_frozen_copy_alone_reaches_every_form(L):
    """The condition that keeps the comparison below from being vacuous, on the reference side."""
    fwd, bwd = set(), set()
    for var in VARIANTS.values():
        for sw in SWITCHES:
            with _Settings(L, sw, var):
                for E, H, N, pairs, cg, prec, srt in forward_grid():
                    _note(fwd, forward_form(R.forward_ref(L, sw, E, H, N, pairs, cg, prec, lambda: srt)[0]))
                for n, H, N, cg, kept, bf16, srt, asc in backward_grid():
                    _note(bwd, backward_form(R.backward_ref(L, sw, n, H, N, cg, kept, bf16, srt, asc)[0]))
    assert fwd == WANT_FORWARD
    assert bwd == WANT_BACKWARD


def test_plans_choose_what_the_frozen_code_chose(L):
    fwd, bwd, points = set(), set(), 0
    for var in VARIANTS.values():
        for sw in SWITCHES:
            with _Settings(L, sw, var):
                for E, H, N, pairs, cg, prec, srt in forward_grid():
                    plan = ops._plan_forward(L, E, H, prec, cg, pairs)
                    ref_asked = []
                    entries, key, (kept, ctx_bf16, ctx_sorted) = R.forward_ref(L, sw, E, H, N, pairs, cg, prec, lambda: ref_asked.append(1) or srt)
                    where = (var, sw, E, H, N, pairs, cg, prec, srt)
                    assert forward_entries(plan) == entries, where
                    assert ("fwd_bf16" if plan.bf16 else "fwd_fp32") == key, where
                    assert (plan.form == "mask", plan.bf16 and plan.form == "mask", plan.ask_sorted and srt) == (kept, ctx_bf16, ctx_sorted), where
                    assert len(ref_asked) == int(plan.ask_sorted), where        # src_sorted (a read-back) is asked when it was asked
                    _note(fwd, forward_form(forward_entries(plan)))
                    points += 1
                for n, H, N, cg, kept, bf16, srt, asc in backward_grid():
                    plan = ops._plan_backward(L, n, H, kept, bf16, srt, cg, asc)
                    entries, key = R.backward_ref(L, sw, n, H, N, cg, kept, bf16, srt, asc)
                    where = (var, sw, n, H, N, cg, kept, bf16, srt, asc)
                    assert backward_entries(plan) == entries, where
                    assert ("bwd_bf16" if plan.bf16 else "bwd_fp32") == key, where
                    _note(bwd, backward_form(backward_entries(plan)))
                    points += 1
    assert fwd == WANT_FORWARD and bwd == WANT_BACKWARD
    assert points == 3 * 8 * (5 * 8 * 2 * 2 * 2 * 2 * 2 + 5 * 8 * 2 * 2 * 2 * 2 * 2 * 3)


def test_settings_are_restored(L):
    assert (L.sgs_edge_score_get_variant(), L.sgs_edge_score_get_bwd_variant()) == (-1, -1)
    assert ops._PRODUCTION_ROWS == 65536


# ------------------------------------------------------------------ the active-row prologue
class _Graph:
    pass


def _active(eid, gq):
    a, b = ops.ActiveSet(), ops.ActiveSet()
    graph = _Graph()
    for act in (a, b):
        act.set(eid, graph, ascending=True)
        act.gq = gq
    return a, b, graph


def _both(a, b, gp, ei, N):
    new = ops._active_rows(a, gp, ei, N)
    ref = R.active_rows_ref(b, gp, ei, N, gp.device, ops._zero_token, ops.get_graph)
    assert a.gq is None and b.gq is None
    return new, ref


def test_prologue_takes_the_handed_over_gradient_as_it_is():
    E, N = 11, 5
    ei = torch.randint(0, N, (2, E))
    eid = torch.tensor([7, 2, 9])
    gq = torch.randn(3)
    a, b, graph = _active(eid, gq)
    gp = ops._zero_token(torch.device("cpu")).expand(E)                     # as _SelectSampled returns it
    new, ref = _both(a, b, gp, ei, N)
    for got in (new, ref):
        assert got[0] is eid and got[1] is graph and got[2] == 3 and got[3] is gq


def test_prologue_gathers_a_dense_gradient():
    E, N = 11, 5
    ei = torch.randint(0, N, (2, E))
    eid = torch.tensor([7, 2, 9])
    a, b, graph = _active(eid, None)
    gp = torch.randn(E)
    new, ref = _both(a, b, gp, ei, N)
    for got in (new, ref):
        assert got[0] is eid and got[1] is graph and got[2] == 3 and torch.equal(got[3], gp[eid])
    # a zero of the right shape that is not the token's expansion is gathered like any other gradient
    a, b, graph = _active(eid, torch.ones(3))
    new, ref = _both(a, b, torch.zeros(1).expand(E), ei, N)
    assert torch.equal(new[3], torch.ones(3)) and torch.equal(ref[3], new[3]) and new[3] is not ref[3]


def test_prologue_adds_the_handed_over_gradient_to_a_gathered_one():
    E, N = 11, 5
    ei = torch.randint(0, N, (2, E))
    eid = torch.tensor([7, 2, 9])
    gq = torch.randn(3)
    a, b, graph = _active(eid, gq)
    gp = torch.randn(E)
    new, ref = _both(a, b, gp, ei, N)
    for got in (new, ref):
        assert got[0] is eid and got[1] is graph and got[2] == 3 and torch.equal(got[3], gp[eid] + gq) and got[3] is not gq
