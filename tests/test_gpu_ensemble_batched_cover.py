"""GPU: the batched ensemble-evaluation engine under node-covering draws (args.sgs_cover_nodes with args.sgs_eval_batch_cover).

Against the serial loop under the same flag from the same clocks: the drawn edge lists are torch.equal, the F1 triple is equal, both
clocks end in the same place, and the logits meet the assertion of the existing no-flag engine test of that head -- GCN, GAT, GIN and
Chebyshev K = 1: |diff| <= 1e-5 x the largest |logit| (tests/test_gpu_ensemble_batched.py, _heads.py); 8-head GAT, GAT with the edge term
and Chebyshev K = 3: bitwise, the mean too (tests/test_gpu_ensemble_batched_variants.py).  Every drawn edge list covers."""
import argparse
import sys

import numpy as np
import pytest
import torch

import cover_ref as CR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DRAWS = 3

# name -> (class, keyword arguments, the no-flag engine test of this head is bitwise)
MODELS = {"GCN": ("GNNModel", {}, False), "GAT": ("GATModel", {}, False), "GIN": ("GINModel", {}, False), "Cheb": ("ChebModel", {}, False),
          "GAT heads=8": ("GATModel", dict(gat_heads=8), True), "GAT edge": ("GATModel", dict(gat_edge_weight=True), True),
          "Cheb K=3": ("ChebModel", dict(cheb_k=3), True)}


def _ev():
    import sgs_gnn_amd  # noqa: F401
    return sys.modules["sgs_gnn_amd.evaluate"]


def _partition(n, n_sym, seed):
    """A synthetic partition plus seven self-loops (they are candidates but never forced), columns shuffled: E = n_sym + 7."""
    import sgs_gnn_amd as S
    b = S.synthetic_graph(n, n_sym, 24, 5, seed=seed, device="cpu")
    g = torch.Generator().manual_seed(seed)
    loops = torch.randperm(n, generator=g)[:7].repeat(2, 1)
    ei = torch.cat([b.edge_index, loops], dim=1)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)].contiguous()
    prob = torch.rand(ei.shape[1], generator=g)
    return S.Batch(x=b.x, edge_index=ei, y=b.y, train_mask=b.train_mask, val_mask=b.val_mask, test_mask=b.test_mask, prob=prob / prob.sum()).to(DEV)


@pytest.fixture(scope="module")
def part():
    b = _partition(900, 4090, seed=31)
    assert tuple(b.edge_index.shape) == (2, 4097) and b.x.shape[0] == 900
    return b


@pytest.fixture(scope="module")
def big():
    b = _partition(20_000, 99_996, seed=32)
    assert tuple(b.edge_index.shape) == (2, 100_003) and b.x.shape[0] == 20_000
    return b


def _model(name, seed=0):
    import sgs_gnn_amd as S
    torch.manual_seed(seed)
    S.fix_seeds(seed)
    cls, kw, _ = MODELS[name]
    m = getattr(S, cls)(24, 16, 5, dropout_prob=0.3, edge_mlp_type="GCN", **kw)
    with torch.no_grad():                                        # biases are zero-initialised: make them count
        for n_, p_ in m.named_parameters():
            if n_.endswith("bias") and not n_.startswith("edge_prob_mlp."):
                p_.copy_(torch.randn(p_.shape) * 0.1)
    return m.to(DEV)


def _has_in_edge(b):
    e = b.edge_index.cpu().numpy()
    has = np.zeros(b.x.shape[0], dtype=bool)
    has[e[1][e[0] != e[1]]] = True
    return has


def _both(m, batches, q, mode, flag, noises=None, seed=7):
    """The serial loop and the engine under the cover flag, from the same randomness state."""
    import sgs_gnn_amd as S
    ev = _ev()
    res = {}
    for path in ("serial", "batched"):
        a = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=DRAWS, sgs_cover_nodes=True, sgs_eval_batch=flag,
                               sgs_eval_batch_heads="all", sgs_eval_batch_variants=True, _sgs_trace_eval={})
        if path == "batched":
            a.sgs_eval_batch_cover = True
        if noises is not None:
            a._sgs_noise_eval = list(noises)
        S.manual_seed(seed)
        before = dict(ev.PATH_COUNTS)
        f1 = S.ensemble_evaluate(a, m, batches, DEV, q=q, mode=mode)
        other = "batched" if path == "serial" else "serial"
        assert ev.PATH_COUNTS[path] == before[path] + 1 and ev.PATH_COUNTS[other] == before[other], path
        res[path] = (f1, a._sgs_trace_eval, (S.sampling._NoiseClock.tick, S.model._DropoutClock.tick))
    return res


def _assert_same(res, bitwise):
    (f_s, t_s, k_s), (f_b, t_b, k_b) = res["serial"], res["batched"]
    assert set(t_b) == set(t_s) == {"logits", "mean", "edges"}
    assert k_s == k_b                                            # _NoiseClock and _DropoutClock end where the serial loop leaves them
    assert torch.equal(t_s["edges"], t_b["edges"])
    assert f_s == f_b
    assert t_b["logits"].shape == t_s["logits"].shape and t_b["mean"].shape == t_s["mean"].shape
    if bitwise:
        assert torch.equal(t_b["logits"], t_s["logits"])
        assert torch.equal(t_b["mean"], t_s["mean"])
    else:
        scale = float(t_s["logits"].abs().max())
        assert torch.allclose(t_b["logits"], t_s["logits"], rtol=0, atol=1e-5 * scale)
        assert torch.allclose(t_b["mean"], t_s["mean"], rtol=0, atol=1e-5 * scale)


def _assert_covers(edges, b, q):
    has = _has_in_edge(b)
    assert int(has.sum()) <= q                                   # M <= q: every node with a candidate non-loop in-edge keeps one
    e = edges.cpu().numpy()
    assert e.shape == (DRAWS, 2, q)
    for d in range(DRAWS):
        got = np.zeros(has.size, dtype=bool)
        s_, d_ = e[d]
        got[d_[s_ != d_]] = True
        assert not (has & ~got).any(), d
    assert not np.array_equal(e[0], e[1])                        # draws really happen


# (mode, sgs_eval_batch): 2 splits the three draws into passes of 2 and 1
RUNS = [("learned", True), ("learned", 2), ("random", True), ("edge", True)]


@pytest.mark.parametrize("mode,flag", RUNS)
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_equals_the_serial_loop_under_the_flag(part, name, mode, flag):
    q = 1500
    ev = _ev()
    m = _model(name)
    if flag == 2:
        H, C = ev._head_dims(m, ev._head_of(m))
        assert ev.plan_draws(4097, q, 900, H, C, DRAWS, flag, head=ev._head_of(m), cover=True) == [2, 1]
    res = _both(m, [part, part], q, mode, flag)
    _assert_same(res, MODELS[name][2])
    _assert_covers(res["batched"][1]["edges"], part, q)
    if name != "Cheb":                                           # (Chebyshev K = 1 ignores the graph)
        assert not torch.equal(res["batched"][1]["logits"][0], res["batched"][1]["logits"][1])


@pytest.mark.parametrize("mode", ["learned", "random", "edge"])
def test_gcn_head_at_partition_size(big, mode):
    q = 30_000
    res = _both(_model("GCN"), [big], q, mode, True)
    _assert_same(res, False)
    _assert_covers(res["batched"][1]["edges"], big, q)


def test_without_the_opt_in_the_flag_keeps_the_serial_loop_and_without_the_flag_nothing_changes(part):
    import sgs_gnn_amd as S
    ev = _ev()
    m = _model("GCN")
    on = dict(degree_bias_coef=0.3, num_samples_eval=DRAWS, sgs_eval_batch=True, sgs_eval_batch_heads="all", sgs_eval_batch_variants=True)
    runs = {}
    for key, kw in (("plain", {}), ("optin only", dict(sgs_eval_batch_cover=True)), ("flag only", dict(sgs_cover_nodes=True)),
                    ("flag, optin False", dict(sgs_cover_nodes=True, sgs_eval_batch_cover=False))):
        a = argparse.Namespace(**on, **kw, _sgs_trace_eval={})
        S.manual_seed(7)
        before = dict(ev.PATH_COUNTS)
        f1 = S.ensemble_evaluate(a, m, [part], DEV, q=1500, mode="learned")
        took = "serial" if kw.get("sgs_cover_nodes") else "batched"
        assert ev.PATH_COUNTS[took] == before[took] + 1, key
        runs[key] = (f1, a._sgs_trace_eval)
    # the opt-in alone changes nothing: the no-flag engine, bit for bit
    assert runs["plain"][0] == runs["optin only"][0]
    for k in ("logits", "mean", "edges"):
        assert torch.equal(runs["plain"][1][k], runs["optin only"][1][k])
        assert torch.equal(runs["flag only"][1][k], runs["flag, optin False"][1][k])
    assert not torch.equal(runs["plain"][1]["edges"], runs["flag only"][1]["edges"])      # the plain draws are other draws


@pytest.mark.parametrize("name", ["GCN", "GAT edge", "Cheb"])
@pytest.mark.parametrize("n_explicit", [3, 2])
def test_explicit_noise_is_honoured(part, name, n_explicit):
    """args._sgs_noise_eval: the first n_explicit draws take the given noise, the rest the clock (a pass never mixes the two)."""
    import sgs_gnn_amd as S
    ops = S.ops
    q = 1500
    E = part.edge_index.shape[1]
    g = torch.Generator().manual_seed(11)
    noises = [torch.empty(E).exponential_(1, generator=g).to(DEV) for _ in range(n_explicit)]
    m = _model(name)
    res = _both(m, [part], q, "learned", True, noises=noises)
    _assert_same(res, MODELS[name][2])
    edges = res["batched"][1]["edges"]
    _assert_covers(edges, part, q)
    assert res["batched"][2][0] == DRAWS - n_explicit            # noise-clock ticks after manual_seed: only the clock draws took one
    with torch.no_grad():
        m.eval()
        p = m.edge_prob_mlp(part.x, part.edge_index).squeeze().contiguous()
    cover = ops.get_graph(part.edge_index, part.x.shape[0])
    for d, nz in enumerate(noises):                              # the draws by hand from the given noise
        r = ops.sample_topq(ops.SAMPLE_LEARNED, p, None, 0.3, q, part.edge_index, noise=nz, want_keys=True, cover=cover)
        assert torch.equal(edges[d], r.edge_index), d
        plain = ops.sample_topq(ops.SAMPLE_LEARNED, p, None, 0.3, q, part.edge_index, noise=nz, want_keys=True)
        ref = CR.cover_ref(plain.keys, part.edge_index, part.x.shape[0], q)
        assert torch.equal(edges[d].cpu(), part.edge_index.cpu()[:, torch.from_numpy(ref["eid"])]), d
