"""CPU checks of tests/loss_ref.py, the fp64 reference of tests/test_gpu_loss_chain.py: its two forms against each other and against
oracle/, the conditions on the seeded inputs that make an fp32 kernel comparable at all, and the proof that the cases can see the faults
they are meant to see (every single-term mutation of the reference moves a compared quantity by more than 100 x its tolerance)."""
import pytest
import torch
import torch.nn.functional as F

import loss_ref as R
from oracle import sgs_oracle as O

ORDINARY = [n for n in R.HYBRID_CASES if R.make_case(n)["kind"] == "ordinary"]


def _rel(a, b):
    """max |a - b| relative to max(1, max |b|); nan only where both are."""
    a, b = a.detach().double().flatten(), b.detach().double().flatten()
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    ok = ~torch.isnan(b)
    if not bool(ok.any()):
        return 0.0
    return float((a - b)[ok].abs().max()) / max(1.0, float(b[ok].abs().max()))


@pytest.mark.parametrize("name", R.HYBRID_CASES)
def test_closed_form_equals_autograd_form(name):
    c = R.make_case(name)
    a, b = R.reference(name)[0], R.autograd_form(c)
    for k in ("out7", "dlogits", "dw"):
        assert _rel(a[k], b[k]) <= 1e-12, (name, k)
    assert float(a["out7"][2]) == int(a["out7"][2]) and float(a["out7"][3]) == int(a["out7"][3])


def test_closed_form_equals_autograd_form_sharded_divisor():
    c = R.make_case(R.SHARD_CASE)
    for lo, hi in R.SHARDS[1:]:
        sub = dict(c, sei=c["sei"][:, lo:hi].contiguous(), w=c["w"][lo:hi].contiguous(), q=hi - lo)
        a, b = R.closed_form(sub, q_div=c["q"]), R.autograd_form(sub, q_div=c["q"])
        assert _rel(a["out7"][1], b["out7"][1]) <= 1e-12
        full = R.reference(R.SHARD_CASE)[0]
        # reg2's share of the gradient is linear in the edges: the shard's rows are the unsharded ones (reg1's share needs the global counts)
        only2 = dict(sub, c1=0.0)
        s2, f2 = R.closed_form(only2, q_div=c["q"]), R.closed_form(dict(c, c1=0.0))
        assert _rel(s2["dw"], f2["dw"][lo:hi]) <= 1e-12 and _rel(s2["Gs"], f2["Gs"][lo:hi]) <= 1e-12 and _rel(s2["Gd"], full["Gd"][lo:hi]) <= 1e-12
    tot = sum(R.raw_sums(c, lo, hi) for lo, hi in R.SHARDS)
    assert _rel(tot, R.reference(R.SHARD_CASE)[0]["raw"]) <= 1e-12
    assert torch.equal(R.raw_sums(c, 0, 0), torch.zeros(4, dtype=torch.float64))


@pytest.mark.parametrize("name", ORDINARY)
def test_closed_form_equals_oracle_on_ordinary_inputs(name):
    c = R.make_case(name)
    a = R.reference(name)[0]
    L, w = c["logits"].double(), c["w"].double()
    if bool(c["mask"].any()):
        assert _rel(a["out7"][5], F.cross_entropy(L[c["mask"]], c["y"][c["mask"]])) <= 1e-12
    l2, nvalid, lsum = O.reg1_loss(w, c["sei"], c["y"], c["mask"])
    assert int(a["out7"][2]) == nvalid and int(a["out7"][3]) == int(lsum)
    assert _rel(a["out7"][0], torch.as_tensor(float(l2), dtype=torch.float64)) <= 1e-12
    assert _rel(a["out7"][1], O.consistency_loss(w, c["sei"], L)) <= 1e-12


def test_the_two_cosine_forms_agree_on_ordinary_inputs_and_differ_under_the_clamp():
    """cos = <x, y> / sqrt(max(|x|^2 |y|^2, 1e-16)) (the kernel, torch 2.0) against <x, y> / (max(|x|, 1e-8) max(|y|, 1e-8)) (the installed
    torch): equal to 1e-12 whenever both row norms are >= 1e-3, values and gradients; different by a factor 100 at |x| = 1e-10, |y| = 1.4e3,
    and in the gradient at x = 0."""
    for name in ORDINARY:
        c = R.make_case(name)
        L = c["logits"].double().requires_grad_(True)
        s, d = c["sei"]
        a, b = R.cos_documented(L[s], L[d]), R.cos_torch_now(L[s], L[d])
        assert _rel(a, b) <= 1e-12 and _rel(b, F.cosine_similarity(L[s], L[d], dim=-1)) <= 1e-12, name
        ga, gb = torch.autograd.grad(a.sum(), L, retain_graph=True)[0], torch.autograd.grad(b.sum(), L)[0]
        assert _rel(ga, gb) <= 1e-12, name
    x = torch.tensor([[1e-10, 0.0, 0.0]], dtype=torch.float64)
    y = torch.tensor([[1e3, 1e3, 0.0]], dtype=torch.float64)
    assert abs(float(R.cos_documented(x, y)) - 2 ** -0.5) < 1e-12             # |x|^2 |y|^2 = 2e-14 > 1e-16: the true cosine
    assert abs(float(R.cos_torch_now(x, y)) - 2 ** -0.5 * 1e-2) < 1e-9
    z = torch.zeros(1, 3, dtype=torch.float64, requires_grad=True)
    (gz,) = torch.autograd.grad(R.cos_documented(z, y).sum(), z)
    assert _rel(gz, y / R.EPS2 ** 0.5) <= 1e-12                 # the documented form's own gradient at x = 0: y / 1e-8 (the denominator is constant)


@pytest.mark.parametrize("name", R.HYBRID_CASES)
def test_hybrid_inputs_meet_their_conditions(name):
    c = R.make_case(name)
    for k in ("logits", "w"):
        assert not bool(torch.isnan(c[k]).any()) and c[k].dtype == torch.float32
    assert c["sei"].shape == (2, c["q"]) and int(c["sei"].min()) >= 0 and int(c["sei"].max()) < c["N"]
    assert int(c["y"].min()) >= 0 and int(c["y"].max()) < c["C"]
    assert float(c["w"].min()) >= 0.0 and float(c["w"].max()) <= 1.0
    norms = c["logits"].double().norm(dim=1)
    ref = R.reference(name)[0]
    if c["kind"] == "clamp":
        assert bool(ref["clamped"].any()) and float(norms.min()) < 1e-8
        assert float(norms[~ref["hot_rows"]].min()) >= 1e-3
    else:
        assert float(norms.min()) >= 1e-3 and not bool(ref["clamped"].any())


def test_hybrid_case_table_covers_what_it_claims():
    names = set(R.HYBRID_CASES)
    assert {f"N257_C{C}_q65" for C in (1, 2, 15, 16, 17, 41, 64, 65, 130)} <= names
    assert {f"N257_C41_q{q}" for q in (1, 15, 16, 17, 63, 64, 65, 5000, 16500)} <= names
    assert {f"N{N}_C41_q5000" for N in (1, 5, 257, 1030)} <= names
    coefs = {(R.make_case(n)["c1"], R.make_case(n)["c2"]) for n in names}
    assert {(1.0, 0.5), (0.0, 0.5), (1.0, 0.0), (0.3, 0.7)} <= coefs
    big = R.make_case("N257_C41_q5000")
    s, d = big["sei"]
    assert 0.03 < float((s == d).float().mean()) < 0.12
    assert 0.02 < float((big["sei"][:, 1:] == big["sei"][:, :-1]).all(0).float().mean()) < 0.1
    assert 0.5 < float(big["mask"].float().mean()) < 0.7
    assert bool(R.make_case("mask_all")["mask"].all()) and int(R.make_case("mask_one")["mask"].sum()) == 1
    assert not bool(R.make_case("mask_none")["mask"].any())
    for k in (0, 1, 2):
        o = R.reference(f"labelsum_{k}")[0]
        assert int(o["out7"][3]) == k and (float(o["out7"][0]) > 0) == (k == 2)
        bce_share = o["dw"] - R.closed_form(dict(R.make_case(f"labelsum_{k}"), c1=0.0))["dw"]
        assert bool((bce_share != 0).any()) == (k == 2)
    c, o = R.make_case("w_0_and_1"), R.reference("w_0_and_1")[0]
    s, d = c["sei"]
    same = c["y"][s] == c["y"][d]
    for wv in (0.0, 1.0):
        for lab in (True, False):
            assert bool((o["sat"] & (c["w"] == wv) & (same == lab)).any())
    assert bool(torch.isfinite(o["out7"]).all()) and bool(torch.isfinite(o["dw"]).all()) and float(o["dw"].abs().max()) > 1e8
    # the saturating scale: exp(second - max) underflows in fp32, the softmax is an exact one-hot
    c = R.make_case("scale_1e4")
    top = c["logits"].topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= 200.0
    sm = torch.exp(c["logits"] - R.reference("scale_1e4")[1]["row_lse"][:, None])[c["mask"]]
    assert bool(((sm == 0) | (sm == 1)).all()) and bool((sm.sum(1) == 1).all())
    assert float(R.make_case("scale_80")["logits"].abs().max()) > 200.0
    # the empty mask: ce and the loss are nan, the rest is finite
    o = R.reference("mask_none")[0]["out7"]
    assert bool(torch.isnan(o[5:]).all()) and bool(torch.isfinite(o[:5]).all())


@pytest.mark.parametrize("N", R.GATE_N)
@pytest.mark.parametrize("C", R.GATE_C)
def test_gate_inputs_meet_their_conditions(N, C):
    c = R.gate_case(N, C)
    planted = {k for k, *_ in c["ties"]}
    assert not torch.equal(c["A"], c["B"]) or N == 0 or C == 1
    for M in (c["A"], c["B"]):
        assert M.shape == (N, C) and not bool(torch.isnan(M).any())
        assert torch.equal(M, (M.double() * 64).round().div(64).float()) or bool(torch.isinf(M).any())        # exact in fp32: multiples of 2^-6
        for i in range(N):
            v = M[i].double().sort().values
            gaps = v[1:] - v[:-1]
            if i not in planted:
                assert C == 1 or float(gaps.min()) > 1e-3
            else:
                near = gaps[gaps.abs() <= 1e-3]                   # (inf - inf = nan on the row of -inf: not counted, not <= 1e-3)
                assert bool((near == 0).all())                    # a planted row's close columns are EXACT ties
    kinds = {(what, later) for _, what, later, _ in c["ties"]}
    if N >= 17 and C == 130:
        assert {("pair", False), ("pair", True), ("const", False), ("const", True), ("ninf", False), ("ninf", True)} <= kinds
        assert any(c["A"][k, 3] == c["A"][k, 67] == c["A"][k].max() for k, w_, _, inA in c["ties"] if w_ == "pair" and inA)
    if N:
        assert torch.equal(R.argmax_first(c["A"]), c["A"].argmax(1)) or bool(c["ties"])


def test_gate_reference_counts_first_maximum():
    L = torch.tensor([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0], [float("-inf")] * 3, [0.0, -1.0, 5.0]])
    assert R.argmax_first(L).tolist() == [1, 0, 0, 2] and R.argmax_first(L, last=True).tolist() == [2, 2, 2, 2]
    y, m = torch.tensor([1, 0, 0, 2]), torch.tensor([True, True, True, False])
    assert R.argmax_counts(L, y, m) == (3, 3) and R.argmax_counts(L, y, m, mut="last_max") == (0, 3)
    assert R.argmax_counts(torch.zeros(0, 3), y[:0], m[:0]) == (0, 0)


def test_hand_over_inputs_meet_their_conditions():
    for c in (R.hand_case(0), R.hand_case(1), R.hand_case(2, q_loss=450), R.draw_case()):
        s, d = c["sei"]
        loops = s[s == d]
        assert loops.numel() == 30 and loops.unique().numel() == 30            # one loop per node: "the last loop's weight" is unambiguous
        assert bool((c["sei"][:, 40:60] == c["sei"][:, 60:80]).all()) and c["min_preact"] > 1e-4
    c = R.draw_case()
    assert torch.equal(c["parent"][:, c["sel"]], c["sei"]) and torch.equal(c["p"][c["sel"]], c["w"])
    assert torch.equal(torch.zeros(c["E"], dtype=torch.bool).index_fill(0, c["p"].topk(c["q"]).indices, True), c["sel"])
    srt = c["p"].double().sort().values
    assert float((srt[1:] - srt[:-1]).min()) > 5e-5 and float(c["p"][c["sel"]].min() - c["p"][~c["sel"]].max()) > 0.04
    # the dense restatement against the oracle's edge-list GCN (PyG's gcn_norm with remaining self-loops)
    c = R.hand_case(0)
    f = lambda k: c[k].double()                                                                # noqa: E731
    out, _ = R.gcn2_dense(f("x"), f("W1"), f("b1"), f("W2"), f("b2"), c["sei"], f("w"), c["N"])
    h = torch.relu(O.gcn_conv(f("x"), c["sei"], f("w"), f("W1"), f("b1")))
    assert _rel(out, O.gcn_conv(h, c["sei"], f("w"), f("W2"), f("b2"))) <= 1e-12


def test_every_planted_fault_moves_a_compared_quantity_by_100_tolerances():
    """Each mutation of the reference (one term each) against the unmutated one, in units of the tolerance the GPU test uses for that
    quantity on that case.  Integer quantities have tolerance 0: any change counts."""
    def worst(mut, names, q_div=None, rows=None):
        best = 0.0
        for n in names:
            c = R.make_case(n)
            good, bad = R.quantities(R.reference(n)[0]), R.quantities(R.closed_form(c, mut=mut))
            bd = R.bounds(n)
            for k in good:
                if good[k].numel() and bd[k] > 0:
                    ok = ~torch.isnan(good[k])
                    if bool(ok.any()):
                        best = max(best, float((good[k] - bad[k])[ok].abs().max()) / bd[k])
        return best
    assert worst("ge1", ["labelsum_1"]) > 100            # reg1 switches on at label sum 1
    assert worst("ge1", ["labelsum_0", "labelsum_2"]) == 0
    assert worst("loop_one_row", ["clamp_tiny"]) > 100   # (outside the clamp a loop's rows are d cos(x, x) / d x = 0: only the clamp shows it)
    assert worst("no_g", R.HYBRID_CASES[:3]) > 100
    # local q instead of q_global: the shards' gradients against the unsharded rows
    c = R.make_case(R.SHARD_CASE)
    full, bd = R.reference(R.SHARD_CASE), R.shard_bounds()
    for lo, hi in R.SHARDS[1:]:
        sub = dict(c, sei=c["sei"][:, lo:hi].contiguous(), w=c["w"][lo:hi].contiguous(), c1=0.0)
        bad = R.closed_form(sub, q_div=c["q"], mut="local_q")
        good = R.closed_form(sub, q_div=c["q"])
        for k in ("dw", "Gs", "Gd"):
            assert float((bad[k] - good[k]).abs().max()) > 100 * bd[(lo, hi)][k], (lo, hi, k)
    # last maximum wins: the planted ties whose label is the first maximum stop counting, the others start
    moved = 0
    for N in R.GATE_N:
        for C in R.GATE_C:
            g = R.gate_case(N, C)
            for M in (g["A"], g["B"]):
                moved += R.argmax_counts(M, g["y"], g["mask"]) != R.argmax_counts(M, g["y"], g["mask"], mut="last_max")
    assert moved >= 10
