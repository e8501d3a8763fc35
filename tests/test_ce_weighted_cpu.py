"""CPU: the class-weighted / label-smoothed cross entropy below the GPU -- the closed form of tests/ce_weighted_ref.py against torch's own
F.cross_entropy in fp64 (the definition), training._ce_spec's accept / refuse table, the four new entry points of the C ABI (declared in
include/sgs_hip.h, exported by the library, bound with the declared argument lists), and the weight validation of ops.masked_cross_entropy
/ ops.hybrid_loss, which fires before any device work."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

import ce_weighted_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- closed form against torch
def test_case_table_covers_the_shapes_and_settings():
    names = set(W.CASES)
    for N, C in ((1, 1), (7, 2), (63, 5), (200, 41), (130, 70)):
        for eps in (0.0, 0.1, 1.0):
            for wk in ("none", "rand", "zero1"):
                for mk in ("60", "one", "none"):
                    assert f"N{N}_C{C}_eps{eps}_w{wk}_m{mk}" in names
    assert any("dead_train" in n for n in names) and any("scale80" in n for n in names)
    c = W.make_case("N63_C5_eps0.1_dead_train")
    assert float(c["w"][c["y"][c["mask"]]].abs().sum()) == 0.0 and float(c["w"].sum()) > 0      # den = 0 with weight elsewhere
    c = W.make_case("N200_C41_eps0.1_scale80")
    assert float(c["logits"].abs().max()) > 200.0
    c = W.make_case("N200_C41_eps0.0_wzero1_m60")
    assert int((c["w"] == 0).sum()) == 1 and float(c["w"][c["w"] > 0].min()) >= 0.2 and float(c["w"].max()) <= 5.0


@pytest.mark.parametrize("name", W.CASES)
def test_closed_form_equals_torch_in_fp64(name):
    """loss and d logits to 1e-12 relative (of the quantity's largest magnitude); nan exactly where torch has nan, nothing infinite."""
    c = W.make_case(name)
    mine, ref = W.closed_form(c), W.torch_form(c)
    for k in ("loss", "dlogits"):
        a, b = mine[k], ref[k]
        assert a.dtype == torch.float64 and a.shape == b.shape
        assert torch.equal(torch.isnan(a), torch.isnan(b)), (name, k, "nan pattern")
        assert not bool(torch.isinf(a).any()) and not bool(torch.isinf(b).any())
        ok = ~torch.isnan(b)
        if bool(ok.any()):
            scale = float(b[ok].abs().max())
            assert float((a - b)[ok].abs().max()) <= 1e-12 * scale, (name, k)
    empty = not bool(c["mask"].any())
    den0 = float(mine["den"]) == 0.0
    assert bool(torch.isnan(mine["loss"])) == (empty or den0)
    if empty:
        assert float(mine["dlogits"].abs().max()) == 0.0                                    # no row receives a gradient
    elif den0:
        assert bool(torch.isnan(mine["dlogits"][c["mask"]]).all()) and float(mine["dlogits"][~c["mask"]].abs().sum()) == 0.0


def test_uniform_rescaling_of_the_weight_leaves_the_loss_unchanged_but_a_ramp_does_not():
    """What the replay test leans on: w -> 2 w changes nothing (a weighted mean), a non-uniform update does."""
    c = W.make_case("N200_C41_eps0.1_wrand_m60")
    a = W.closed_form(c)["loss"]
    b = W.closed_form(c, w=c["w"] * 2)["loss"]
    d = W.closed_form(c, w=c["w"] * torch.linspace(0.25, 4.0, 41))["loss"]
    assert abs(float(a - b)) < 1e-12 and abs(float(a - d)) > 1e-3


def test_error_model_in_the_stated_form_is_no_looser_than_in_the_kernels_form():
    """The bound is sized by the fp32 evaluation of the form as stated (W lse - sum_c w_c x_c); the kernels sum w_c (lse - x_c).  Were the
    stated form to cancel, its fp32 deviation -- and with it the bound -- would be inflated by orders of magnitude over what the kernels
    can reach, most of all at large logits.  It is not.  Measured over the table: bound(stated) / bound(kernels' form) lies between 0.38
    and 2.8 (which of two fp32 roundings lands nearer is luck, either way) and is exactly 1.0 on the four logits x 80 cases, where
    W lse - sum_c w_c x_c is of the order of W lse itself.  Asserted: at most 2 on the scaled cases, at most 4 anywhere."""
    import loss_ref as R
    ratios = {}
    for name in W.CASES:
        c = W.make_case(name)
        r64, i32, k32 = W.closed_form(c), W.closed_form(c, torch.float32), W.closed_form(c, torch.float32, form="kernel")
        assert torch.equal(r64["loss"].isnan(), k32["loss"].isnan())
        if bool(r64["loss"].isnan()):
            continue
        assert abs(float(W.closed_form(c, form="kernel")["loss"] - r64["loss"])) <= 1e-12 * max(abs(float(r64["loss"])), 1e-300)
        ratios[name] = R.bound(r64["loss"], i32["loss"]) / R.bound(r64["loss"], k32["loss"])
        assert ratios[name] <= (2.0 if c["scale"] != 1.0 else 4.0), (name, ratios[name])
    print(f"bound(stated form) / bound(kernels' form): min {min(ratios.values()):.2f} max {max(ratios.values()):.2f}")
    assert sum(1 for n in ratios if "scale80" in n) == 4


@pytest.mark.parametrize("name", ["N200_C41_eps0.1_wrand_m60", "N130_C70_eps1.0_wzero1_m60", "N63_C5_eps0.0_wrand_m60", "N200_C41_eps0.1_scale80"])
@pytest.mark.parametrize("cut", [0.0, 0.37, 1.0])
def test_node_blocks_with_the_global_den_add_up_to_the_replicated_loss(name, cut):
    """sharded.train_step_blocksharded's split: each block's row sum over the den of ALL train rows.  The shares add up to the loss and
    the blocks' gradient rows are the whole problem's rows (an empty block included); with a block's OWN den they would not."""
    c = W.make_case(name)
    N = c["N"]
    bounds = [0, int(round(cut * N)), N]
    full = W.closed_form(c)
    shares, grads, den = W.block_shares(c, bounds)
    assert abs(float(sum(shares) - full["loss"])) <= 1e-12 * abs(float(full["loss"]))
    assert float((torch.cat(grads) - full["dlogits"]).abs().max()) <= 1e-12 * float(full["dlogits"].abs().max())
    if 0 < bounds[1] < N:
        own = [W.closed_form(dict(c, logits=c["logits"][lo:hi], y=c["y"][lo:hi], mask=c["mask"][lo:hi]))["loss"] for lo, hi in zip(bounds, bounds[1:])]
        assert abs(float(sum(own) - full["loss"])) > 1e-3 * abs(float(full["loss"]))


# ---------------------------------------------------------------------------------------------------- _ce_spec
class _Sub(nn.CrossEntropyLoss):
    pass


def test_ce_spec_accepts_exactly_the_mean_cross_entropy():
    from sgs_gnn_amd.training import _ce_spec, _fused_ce_ok
    w = torch.rand(5)
    assert _ce_spec(nn.CrossEntropyLoss()) == (None, 0.0)
    s = _ce_spec(nn.CrossEntropyLoss(weight=w))
    assert s[0].data_ptr() == w.data_ptr() and s[1] == 0.0
    assert _ce_spec(nn.CrossEntropyLoss(label_smoothing=0.1)) == (None, 0.1)
    s = _ce_spec(nn.CrossEntropyLoss(weight=w, label_smoothing=1.0))
    assert s[0].data_ptr() == w.data_ptr() and s[1] == 1.0
    for crit in (nn.CrossEntropyLoss(reduction="sum"), nn.CrossEntropyLoss(reduction="none"), nn.CrossEntropyLoss(ignore_index=0), _Sub(),
                 _Sub(weight=w), nn.NLLLoss(), nn.MSELoss()):
        assert _ce_spec(crit) is None, crit
    # _fused_ce_ok keeps its meaning: the plain criterion only
    assert _fused_ce_ok(nn.CrossEntropyLoss())
    for crit in (nn.CrossEntropyLoss(weight=w), nn.CrossEntropyLoss(label_smoothing=0.1), nn.CrossEntropyLoss(weight=w, label_smoothing=0.1),
                 nn.CrossEntropyLoss(reduction="sum"), nn.CrossEntropyLoss(ignore_index=0), _Sub(), nn.NLLLoss()):
        assert not _fused_ce_ok(crit), crit


def test_sharded_trainers_refuse_a_criterion_they_cannot_evaluate_by_name():
    from sgs_gnn_amd import sharded
    assert sharded._criterion_spec(nn.CrossEntropyLoss(label_smoothing=0.2), "train_step_sharded") == (None, 0.2)
    for where in ("train_step_sharded", "train_step_blocksharded"):
        with pytest.raises(NotImplementedError, match=f"{where}.*NLLLoss"):
            sharded._criterion_spec(nn.NLLLoss(), where)
        with pytest.raises(NotImplementedError, match="CrossEntropyLoss"):
            sharded._criterion_spec(nn.CrossEntropyLoss(reduction="sum"), where)


# ---------------------------------------------------------------------------------------------------- the C ABI
_NEW = {
    "sgs_masked_ce_w_fwd": ["logits", "N", "C", "y", "train_mask", "weight", "label_smoothing", "loss", "row_lse", "rowloss", "den", "stream"],
    "sgs_masked_ce_w_bwd": ["logits", "N", "C", "y", "train_mask", "weight", "label_smoothing", "row_lse", "den", "grad_loss", "dlogits", "stream"],
    "sgs_masked_ce_w_bwd_acc": ["logits", "N", "C", "y", "train_mask", "weight", "label_smoothing", "row_lse", "den", "grad_loss", "dlogits",
                                "stream"],
    "sgs_hybrid_loss_w_fwd": ["logits", "N", "C", "y", "train_mask", "w", "sampled_edge_index", "q", "coef1", "coef2", "weight", "label_smoothing",
                              "out", "row_lse", "rowloss", "den", "ws", "ws_bytes", "stream"],
}
_OLD = {"sgs_masked_ce_w_fwd": "sgs_masked_ce_fwd", "sgs_masked_ce_w_bwd": "sgs_masked_ce_bwd", "sgs_masked_ce_w_bwd_acc": "sgs_masked_ce_bwd_acc",
        "sgs_hybrid_loss_w_fwd": "sgs_hybrid_loss_fwd"}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()                      # hipcc cross-compiles without a GPU
    import sgs_gnn_amd
    return sgs_gnn_amd


def test_new_entry_points_are_declared_exported_and_bound(pkg):
    protos = pkg._lib.parse_header()
    L = pkg._lib.lib()
    for name, want in _NEW.items():
        assert name in protos, f"{name} is not declared in include/sgs_hip.h"
        restype, argtypes, argnames = protos[name]
        assert restype is ctypes.c_int and argnames == want, (name, argnames)
        fn = getattr(L, name)                                                 # AttributeError: not exported
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == list(argtypes) and len(fn.argtypes) == len(want)
        for a, t in zip(argnames, argtypes):
            assert t is {"N": ctypes.c_int64, "C": ctypes.c_int64, "q": ctypes.c_int64, "coef1": ctypes.c_float, "coef2": ctypes.c_float,
                         "label_smoothing": ctypes.c_float, "ws_bytes": ctypes.c_size_t}.get(a, ctypes.c_void_p), (name, a)
        # the old signature plus weight and label_smoothing, with the float `den` where the old one has the integer `n_rows`
        old = [("den" if a == "n_rows" else a) for a in protos[_OLD[name]][2]]
        assert [a for a in want if a not in ("weight", "label_smoothing")] == old, name
    hdr = open(pkg._lib.HEADER).read()
    for name in _NEW:                                                          # `den` is a float word, `weight` a const float array
        decl = re.search(name + r"\s*\(([^;]*?)\)\s*;", hdr, flags=re.S).group(1)
        assert re.search(r"const float\*\s*weight", decl) and re.search(r"float\*\s*den", decl) and "float label_smoothing" in decl, name


def test_new_entry_points_refuse_bad_arguments_before_any_launch(pkg):
    """SGS_REQUIRE: label_smoothing outside [0, 1] (nan included) and a NULL den -- through the error channel, with no device touched
    (every pointer is a dummy; a check that let them through would fault here)."""
    L = pkg._lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    for eps in (-0.01, 1.5, float("nan")):
        assert L.sgs_masked_ce_w_fwd(p, 4, 3, p, p, None, eps, p, p, p, p, None) == -1 and b"label_smoothing" in L.sgs_last_error()
        assert L.sgs_masked_ce_w_bwd(p, 4, 3, p, p, None, eps, p, p, p, p, None) == -1 and b"label_smoothing" in L.sgs_last_error()
        assert L.sgs_masked_ce_w_bwd_acc(p, 4, 3, p, p, None, eps, p, p, p, p, None) == -1 and b"label_smoothing" in L.sgs_last_error()
        assert L.sgs_hybrid_loss_w_fwd(p, 4, 3, p, p, p, p, 2, 1.0, 0.5, None, eps, p, p, p, p, p, 1 << 20, None) == -1
        assert b"label_smoothing" in L.sgs_last_error()
    assert L.sgs_masked_ce_w_fwd(p, 4, 3, p, p, None, 0.1, p, p, p, None, None) == -1 and b"den" in L.sgs_last_error()
    assert L.sgs_masked_ce_w_bwd(p, 4, 3, p, p, None, 0.1, p, None, p, p, None) == -1 and b"den" in L.sgs_last_error()
    assert L.sgs_masked_ce_w_bwd_acc(p, 4, 3, p, p, None, 0.1, p, None, p, p, None) == -1 and b"den" in L.sgs_last_error()
    assert L.sgs_hybrid_loss_w_fwd(p, 4, 3, p, p, p, p, 2, 1.0, 0.5, None, 0.1, p, p, p, None, p, 1 << 20, None) == -1
    assert b"den" in L.sgs_last_error()
    assert L.sgs_masked_ce_w_fwd(None, 4, 3, p, p, None, 0.1, p, p, p, p, None) == -1 and b"bad arguments" in L.sgs_last_error()


# ---------------------------------------------------------------------------------------------------- weight validation
def test_weight_is_validated_before_the_library_is_touched(monkeypatch):
    import sgs_gnn_amd as S
    ops = S.ops

    def boom():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(S._lib, "lib", boom)
    monkeypatch.setattr(ops, "_need_gpu", lambda *a: boom())
    L, y, m = torch.randn(4, 3), torch.zeros(4, dtype=torch.long), torch.ones(4, dtype=torch.bool)
    w, sei = torch.rand(6), torch.zeros(2, 6, dtype=torch.long)
    bad = [(torch.ones(3, dtype=torch.float64), "float32.*float64"), (torch.ones(4), r"length C = 3.*\(4,\)"), (torch.ones(1, 3), "length C = 3"),
           (torch.ones(3, device="meta"), "device meta.*cpu"), (torch.ones(6)[::2], "contiguous"), ([1.0, 1.0, 1.0], "tensor.*list")]
    for wt, pat in bad:
        with pytest.raises(ValueError, match=pat):
            ops.masked_cross_entropy(L, y, m, weight=wt)
        with pytest.raises(ValueError, match=pat):
            ops.hybrid_loss(L, y, m, w, sei, 1.0, 0.5, weight=wt, label_smoothing=0.1)
        with pytest.raises(ValueError, match=pat):
            ops.check_ce_spec(L, wt, 0.0)
    for eps in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            ops.masked_cross_entropy(L, y, m, label_smoothing=eps)
    good = torch.ones(3)
    assert ops.check_ce_spec(L, good, 0.25)[0].data_ptr() == good.data_ptr() and ops.check_ce_spec(L, None, 1)[1] == 1.0


def test_weighted_call_has_no_cpu_fallback():
    import sgs_gnn_amd as S
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ops.masked_cross_entropy(torch.randn(4, 3), torch.zeros(4, dtype=torch.long), torch.ones(4, dtype=torch.bool), weight=torch.ones(3))
