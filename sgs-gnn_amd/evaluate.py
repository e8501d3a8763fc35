"""Mirror of the reference's evaluate.py: `evaluate` and `ensemble_evaluate` (same signatures and
return tuple).  The three kernels of the training path are reused forward-only; differences that do
not change results: the scorer runs ONCE per batch instead of once per ensemble draw (model.eval():
no dropout, identical inputs => identical probabilities, evaluate.py:84), logits are averaged with a
running sum, and the per-split correct counts stay on the device until the end of the loader.

Test hooks: `args._sgs_noise_eval = [noise_0, noise_1, ...]` feeds explicit Exp(1) noise per draw; `args._sgs_trace_eval = {}`
receives the last partition's per-draw logits [D, N, C] ("logits"), averaged logits ("mean") and drawn edge lists ("edges").

Batched engine (opt-in, `args.sgs_eval_batch`; True: draws per pass from a byte budget, an int k >= 1: at most k per pass): all draws
of a partition run as one pass of batched kernels (ops.ensemble_partition_head) instead of the serial loop below.  Draw d uses the same
(seed, stream id) as the serial loop's d-th draw, so the drawn edge sets are identical.  Which heads take it is a second opt-in,
`args.sgs_eval_batch_heads`: absent / None = ("GCN",) (GNNModel only), "all" = GCN, GAT, GIN and Cheb, or a collection of those names;
other heads keep the serial loop.  A third opt-in, `args.sgs_eval_batch_variants` (absent / None / False = off, True = on), lets the heads'
own options take the engine too: a GATModel with gat_heads in 2..16 and / or gat_edge_weight=True and a ChebModel with cheb_k in 2..8, when
their head is selected; without it these models keep the serial loop.  A GINModel(gin_edge_weight=True) has an engine of its own
(ops._drawn_gine_logits: the GINE aggregation of all draws in one launch per layer, at the input width; the plain batched GIN engine
aggregates transformed features with unit weights and would be wrong for it) behind a fifth opt-in, `args.sgs_eval_batch_gine` (absent /
None / False = off, True = on): it takes the engine iff that is True and "GIN" is among the selected heads; without it, it keeps the serial
loop whatever else is set.  A GATModel(gat_v2=True) has an engine of its own as well (ops._drawn_gatv2_logits: the gathering GATv2
softmax of all draws in one launch per layer, sgs_gatv2_alpha_heads_fwd_multi) behind a sixth opt-in, `args.sgs_eval_batch_gatv2` (absent /
None / False = off, True = on): it takes the engine iff that is True and "GAT" is among the selected heads, for every gat_heads in 1..16 with
and without gat_edge_weight (sgs_eval_batch_variants is not consulted for it); without it, it keeps the serial loop whatever else is set.
Under `args.sgs_cover_nodes` (node-covering draws) every model keeps the serial loop unless a fourth opt-in,
`args.sgs_eval_batch_cover` (absent / None / False = off, True = on), is set: then the cover flag no longer blocks the engine, the other
opt-ins decide exactly as they do without the flag, and every pass draws with ops.sample_topq_multi(..., cover=) -- row d is the serial
loop's d-th covering draw.  `PATH_COUNTS` records which path each ensemble_evaluate call took.

Per-class metrics (both functions, the serial loop and every batched engine): `args.sgs_f1_average` (absent / None / "micro" = the accuracy
triple as ever; "macro" / "weighted" = the returned triple holds that F1 average) and `args.sgs_eval_report` (absent / None = off; a dict
receives "confusion", an int64 CPU tensor [3, C, C] (split, true class, predicted class), and "report", utils.classification_report of it;
both None for an empty loader).  When either asks for per-class counts, one [3, C, C] int64 buffer is zeroed per evaluation, every partition
adds one ops.confusion_counts launch on its final mean logits, and the buffer is read once after the loader is exhausted; otherwise nothing
new is launched or allocated, and with "micro" the triple always comes from the six counters.  The averages are POOLED over the loader:
they are taken from the confusion matrix of all masked nodes of all partitions.  (The reference, with its macro line switched on, would
weight per-partition macro values by partition size; the two agree for micro and on a one-partition loader.  The pooled value does not
depend on how the graph was partitioned and does not drop a class from the partitions where it happens to be absent.)
"""
from __future__ import annotations

import torch

from . import ops
from .model import _DropoutClock
from .utils import F1_AVERAGES, classification_report, f1_from_confusion
from .sampling import _NoiseClock, cover_graph, cover_nodes, draw_learned, draw_prior, random_edge_sampling

PATH_COUNTS = {"serial": 0, "batched": 0}
EVAL_BATCH_BUDGET = 512 << 20          # bytes of per-pass buffers when args.sgs_eval_batch is True
HEADS = ("GCN", "GAT", "GIN", "Cheb")


def _one_draw(args, model, batch, q, mode, edge_probs, noise):
    """-> (logits, the edge list the model ran on)."""
    if mode == 'learned':
        if batch.edge_index.shape[1] > q:
            smp = draw_learned(None, edge_probs, batch.edge_index, q, args.degree_bias_coef, istest=True, noise=noise,
                               cover=cover_graph(args, batch))
            w = ops.st_weights(edge_probs, None, args.degree_bias_coef, smp.stats, smp.eid)     # sampling.py:137-155
            return model(batch, smp.edge_index, w), smp.edge_index
        return model(batch, batch.edge_index), batch.edge_index
    if mode == 'random':
        if batch.edge_index.shape[1] > q:
            ei = random_edge_sampling(batch.edge_index, q=q, cover=cover_graph(args, batch))
            return model(batch, ei), ei
        return model(batch, batch.edge_index), batch.edge_index
    if mode == 'edge':
        if batch.edge_index.shape[1] > q:
            ei = draw_prior(batch.prob, batch.edge_index, q, noise=noise, cover=cover_graph(args, batch)).edge_index
            return model(batch, ei), ei
        return model(batch, batch.edge_index), batch.edge_index
    if mode == 'full':
        return model(batch, batch.edge_index), batch.edge_index
    raise ValueError("Invalid mode. Choose 'learned', 'random', or 'full'.")


def _f1_opts(args):
    """(average, report dict or None, whether per-class counts are needed) from args.sgs_f1_average and args.sgs_eval_report; a bad value
    raises ValueError here, before any partition is read."""
    avg = getattr(args, "sgs_f1_average", None)
    if avg is None:
        avg = "micro"
    if not isinstance(avg, str) or avg not in F1_AVERAGES:
        raise ValueError(f"args.sgs_f1_average={avg!r}: need None or one of {F1_AVERAGES}")
    rep = getattr(args, "sgs_eval_report", None)
    if rep is not None and not isinstance(rep, dict):
        raise ValueError(f"args.sgs_eval_report={rep!r}: need None or a dict (it receives 'confusion' and 'report')")
    return avg, rep, avg != "micro" or rep is not None


def _add_confusion(conf, out, batch):
    """One partition's confusion counts of its final mean logits `out`, added to the evaluation's buffer (made on the first partition)."""
    if conf is None:
        conf = torch.zeros(3, out.shape[1], out.shape[1], dtype=torch.int64, device=out.device)
    return ops.confusion_counts(out, batch.y, (batch.train_mask, batch.val_mask, batch.test_mask), out=conf)


def _finish(avg, rep, conf, micro):
    """The triple to return: `micro` (from the six counters) unless another average was asked for; fills the report dict."""
    if rep is not None:
        rep["confusion"] = rep["report"] = None
    if conf is None:
        return micro
    M = conf.cpu()
    if rep is not None:
        rep["confusion"], rep["report"] = M, classification_report(M)
    return micro if avg == "micro" else f1_from_confusion(M, avg)


def _run(args, model, cluster_loader, device, q, mode, n_draws):
    cover_nodes(args)                       # args.sgs_cover_nodes: validated before any partition is read
    avg, rep, per_class = _f1_opts(args)
    model.eval()
    counts = conf = None
    noises = list(getattr(args, "_sgs_noise_eval", None) or [])
    trace = getattr(args, "_sgs_trace_eval", None)
    with torch.no_grad():
        for batch in cluster_loader:
            batch = batch.to(device)
            ops.new_memo_scope()
            edge_probs = None
            if mode == 'learned' and batch.edge_index.shape[1] > q:
                ops.get_pairs(batch.edge_index, batch.x.shape[0], build=True)     # once per partition (cached)
                edge_probs = model.edge_prob_mlp(batch.x, batch.edge_index).squeeze()         # encoder over the FULL batch graph
            out = None
            logs, edges = [], []
            for _ in range(n_draws):
                o, ei = _one_draw(args, model, batch, q, mode, edge_probs, noises.pop(0) if noises else None)
                out = o if out is None else out + o
                if trace is not None:
                    logs.append(o)
                    edges.append(ei)
            if n_draws > 1:
                out = out / n_draws                                                           # torch.mean(torch.stack(outs))
            if trace is not None:
                trace["logits"], trace["mean"], trace["edges"] = torch.stack(logs), out, torch.stack(edges)
            c = torch.stack([ops.masked_correct(out, batch.y, m) for m in (batch.train_mask, batch.val_mask, batch.test_mask)])
            counts = c.to(torch.int64) if counts is None else counts + c
            if per_class:
                conf = _add_confusion(conf, out, batch)
    if counts is None:
        return _finish(avg, rep, None, (0, 0, 0))
    c = counts.tolist()
    # sum_b f1_b * n_b / sum_b n_b  ==  sum_b correct_b / sum_b n_b   (utils.calculate_f1 is accuracy)
    return _finish(avg, rep, conf, tuple((c[s][0] / c[s][1]) if c[s][1] > 0 else 0 for s in range(3)))


def plan_draws(E: int, q: int, N: int, H: int, C: int, D: int, budget, head: str = "GCN", *, gat_heads: int = 1, gat_edge: bool = False,
               cheb_k: int = 1, cover: bool = False, gine_in: int = 0, gat_v2: bool = False) -> list:
    """Draws per pass of the batched engine: a list of pass sizes summing to D, each >= 1.  `budget` is True (the largest pass whose
    per-draw buffers fit EVAL_BATCH_BUDGET bytes), an int number of bytes via ("bytes", n), or an int k >= 1 (at most k draws per pass).
    Per draw (an upper estimate of the engine's per-draw allocations): keys 4 E + mask E + filter positions 4 E; per drawn edge 40 B
    (int64 id 8, int64 endpoints 16 -- allocated only under the trace hook, counted always --, weight 4, CSR source and id 8, normalised
    weight 4); per-node arrays 36 N; hidden 4 N H; two logit blocks 8 N C.  `head` adds what that head allocates on top: GAT 4 q + 12 N
    (attention values, loop attentions, layer-2 node scores), GIN 4 N H + 8 N C + 4 q + 4 N (the MLP's second hidden block, the second
    conv's product and aggregate, unit edge values and the 1 + eps diagonal); GCN and Cheb nothing.  The keyword-only parameters describe
    the heads' options (their defaults reproduce the numbers above): GAT with K = gat_heads >= 1 allocates K values per attention entry,
    so its term becomes 4 q K + 12 N K (attention values [q, K], loop terms [N, K], layer-2 node scores 2 [N, K]) plus 4 N C (K - 1) for the
    layer-2 product [N, K C] beside the logits; gat_edge adds 8 N (the mean loop weight and count of the edge term; the kernels take them
    as optional outputs, counted always).  Cheb with K = cheb_k >= 2 adds the (K - 1) out-wide block of b's of each layer,
    4 N (K - 1) (H + C), the per-draw Laplacian values 4 q, dis 4 N and the weights scattered by parent edge id 4 E.  `cover`
    (node-covering draws, ops.sample_topq_multi(..., cover=)) adds that call's per-draw workspace and output: 1024 per-workgroup counts
    of forced edges (4096 B) and the cover_info pair (8 B); it never makes a pass larger.  `gine_in` = F > 0 (head "GIN" only; 0 = the
    numbers above for every head) describes the GINE head (gin_edge_weight) at input width F: GIN's term is replaced by what
    ops._drawn_gine_logits allocates per draw beside the counted hidden block and two logit blocks (the second MLP's two [N, C] products),
    4 N F + 8 N H: the first aggregate [N, F] at the input width, the first MLP's second product [N, H] and the second aggregate [N, H]
    (its unit weights are a NULL pointer and 1 + eps a scalar: neither is allocated; the straight-through weights are the 4 B per drawn
    edge counted above).  `gat_v2` (head "GAT" only; False = the numbers above for every head) describes the GATv2 head: GAT's term is
    replaced by what ops._drawn_gatv2_logits allocates per draw beside the counted hidden block, the logits and the 4 B weight per drawn
    edge, 4 q K + 4 N K + 16 N K C: attention values [q, K] and loop attentions [N, K] (one pair, reused by layer 2; eval takes no soft
    copies and no mean loop weight / count, so gat_edge adds nothing), the layer-2 product [N, 2 K C] (lin_l and lin_r in one GEMM, the
    biases added in place) and its two contiguous halves x_l, x_r [N, K C] each.  It is never below the GAT term at the same arguments
    (12 N K C + 4 N C >= 8 N K + 8 N for K, C >= 1), so it never makes a pass larger than that term would.
    The result of the engine does not depend on the split."""
    D = int(D)
    if D < 1:
        raise ValueError(f"plan_draws: D={D} draws")
    if head not in HEADS:
        raise ValueError(f"plan_draws: head={head!r}, need one of {HEADS}")
    if not 1 <= int(gat_heads) <= 16 or not 1 <= int(cheb_k) <= 8:
        raise ValueError(f"plan_draws: gat_heads={gat_heads}, cheb_k={cheb_k}: need 1..16 and 1..8")
    gine_in = int(gine_in)
    if gine_in < 0 or (gine_in and head != "GIN"):
        raise ValueError(f"plan_draws: gine_in={gine_in} with head={head!r}: need 0, or the GINE head's input width >= 1 with head 'GIN'")
    if not isinstance(gat_v2, bool) or (gat_v2 and head != "GAT"):
        raise ValueError(f"plan_draws: gat_v2={gat_v2!r} with head={head!r}: need False, or True with head 'GAT'")
    if budget is True or (isinstance(budget, tuple) and budget[0] == "bytes"):
        nbytes = EVAL_BATCH_BUDGET if budget is True else int(budget[1])
        ks = (int(E) + 63) & ~63
        per = 4 * ks + int(E) + 4 * int(E) + 40 * int(q) + 36 * (int(N) + 1) + 4 * int(N) * int(H) + 8 * int(N) * int(C) + 3 * 2048 * 4 + 64
        K = int(gat_heads)
        if head == "GAT" and gat_v2:
            per += 4 * int(q) * K + 4 * int(N) * K + 16 * int(N) * K * int(C)
        elif head == "GAT":
            per += 4 * int(q) * K + 12 * int(N) * K + 4 * int(N) * int(C) * (K - 1) + (8 * int(N) if gat_edge else 0)
        elif head == "GIN" and gine_in:
            per += 4 * int(N) * gine_in + 8 * int(N) * int(H)
        elif head == "GIN":
            per += 4 * int(N) * int(H) + 8 * int(N) * int(C) + 4 * int(q) + 4 * int(N)
        elif head == "Cheb" and int(cheb_k) > 1:
            per += 4 * int(N) * (int(cheb_k) - 1) * (int(H) + int(C)) + 4 * int(q) + 4 * int(N) + 4 * int(E)
        if cover:
            per += 4 * 1024 + 8
        k = max(1, min(D, int(nbytes) // per))
    else:
        k = int(budget)
        if k < 1:
            raise ValueError(f"sgs_eval_batch={budget}: need True or an int >= 1")
        k = min(k, D)
    return [k] * (D // k) + ([D % k] if D % k else [])


def _batched_ok(args, model, n_draws) -> bool:
    """Whether this call takes the batched engine.  A falsy flag (False, None, 0) means off; anything else must be True or an
    int >= 1, and args.sgs_eval_batch_heads and args.sgs_eval_batch_variants (consulted only then) a valid head selection and None / a
    bool, all checked here, before any partition is read.  A model with gat_heads > 1, gat_edge_weight or cheb_k > 1 takes the engine only
    with sgs_eval_batch_variants=True (per-head GAT kernels / per-draw Chebyshev steps, ops.ensemble_partition_head).  A gat_v2 model takes
    the engine (ops._drawn_gatv2_logits, the multi-draw GATv2 softmax) iff args.sgs_eval_batch_gatv2 is True and "GAT" is a selected head,
    for every gat_heads in 1..16 with and without gat_edge_weight: sgs_eval_batch_variants is not consulted for it, and without the opt-in
    it keeps the serial loop whatever else is set (the v1 engines take node-level scores, which GATv2 has none of).  sgs_eval_batch_gatv2
    is validated with the other opt-ins (None / a bool, only when sgs_eval_batch is truthy); absent, None or False it changes no model's
    routing.  A gin_edge_weight model takes the engine
    (ops._drawn_gine_logits, the multi-draw GINE aggregation) iff args.sgs_eval_batch_gine is True and "GIN" is a selected head; the
    plain batched GIN engine (ops._drawn_gin_logits) aggregates transformed features with unit weights, which is not the GINE layer, so
    without that opt-in the model keeps the serial loop whatever else is set.  sgs_eval_batch_gine is validated with the other opt-ins
    (None / a bool, only when sgs_eval_batch is truthy); absent, None or False it changes no model's routing.  Under
    args.sgs_cover_nodes (node-covering draws, validated first) every model keeps the serial loop unless args.sgs_eval_batch_cover is
    True: with it the cover flag no longer blocks the engine (sgs_sample_topq_multi_cover draws all of a pass's covering draws) and the
    other opt-ins decide exactly as they do without the flag.  sgs_eval_batch_cover is validated with the other opt-ins (None / a bool,
    only when sgs_eval_batch is truthy); absent, None or False it changes nothing."""
    cover = cover_nodes(args)
    flag = getattr(args, "sgs_eval_batch", False)
    if not flag:
        return False
    if cover and (getattr(args, "sgs_eval_batch_cover", None) is None or getattr(args, "sgs_eval_batch_cover", None) is False):
        return False                            # the routing from before the opt-in existed: nothing else is consulted
    if flag is not True and (isinstance(flag, bool) or not isinstance(flag, int) or flag < 1):
        raise ValueError(f"args.sgs_eval_batch={flag!r}: need True (draws per pass from a byte budget) or an int >= 1 (at most k per pass)")
    heads = _eval_heads(args)
    variants = _eval_variants(args)
    _eval_batch_cover(args)
    gine = _eval_batch_gine(args)
    gatv2 = _eval_batch_gatv2(args)
    if n_draws >= 1 and gatv2 and getattr(model, "gat_v2", False):
        return _head_of(model) == "GAT" and "GAT" in heads and 1 <= getattr(model, "gat_heads", 1) <= 16
    if n_draws < 1 or getattr(model, "gat_v2", False) or (getattr(model, "gin_edge_weight", False) and not gine):
        return False
    if not variants:                            # without the third opt-in the heads' options keep the serial loop, as before it existed
        if getattr(model, "gat_heads", 1) > 1 or getattr(model, "gat_edge_weight", False) or getattr(model, "cheb_k", 1) > 1:
            return False
    elif not (1 <= getattr(model, "gat_heads", 1) <= 16 and 1 <= getattr(model, "cheb_k", 1) <= 8):
        return False
    return _head_of(model) in heads


def _eval_batch_cover(args) -> bool:
    """args.sgs_eval_batch_cover: absent / None / False -> False, True -> True.  Anything else raises ValueError."""
    v = getattr(args, "sgs_eval_batch_cover", None)
    if v is None or v is False:
        return False
    if v is True:
        return True
    raise ValueError(f"args.sgs_eval_batch_cover={v!r}: need None, False or True")


def _eval_batch_gatv2(args) -> bool:
    """args.sgs_eval_batch_gatv2: absent / None / False -> False, True -> True.  Anything else raises ValueError."""
    v = getattr(args, "sgs_eval_batch_gatv2", None)
    if v is None or v is False:
        return False
    if v is True:
        return True
    raise ValueError(f"args.sgs_eval_batch_gatv2={v!r}: need None, False or True")


def _eval_batch_gine(args) -> bool:
    """args.sgs_eval_batch_gine: absent / None / False -> False, True -> True.  Anything else raises ValueError."""
    v = getattr(args, "sgs_eval_batch_gine", None)
    if v is None or v is False:
        return False
    if v is True:
        return True
    raise ValueError(f"args.sgs_eval_batch_gine={v!r}: need None, False or True")


def _eval_variants(args) -> bool:
    """args.sgs_eval_batch_variants: absent / None / False -> False, True -> True.  Anything else raises ValueError."""
    v = getattr(args, "sgs_eval_batch_variants", None)
    if v is None or v is False:
        return False
    if v is True:
        return True
    raise ValueError(f"args.sgs_eval_batch_variants={v!r}: need None, False or True")


def _eval_heads(args) -> frozenset:
    """The heads args.sgs_eval_batch_heads sends to the batched engine: absent / None -> {"GCN"}, "all" -> all four, else a list, tuple or
    set of names from HEADS.  Anything else raises ValueError."""
    v = getattr(args, "sgs_eval_batch_heads", None)
    if v is None:
        return frozenset(("GCN",))
    if isinstance(v, str):
        if v == "all":
            return frozenset(HEADS)
    elif isinstance(v, (list, tuple, set, frozenset)) and all(isinstance(h, str) and h in HEADS for h in v):
        return frozenset(v)
    raise ValueError(f"args.sgs_eval_batch_heads={v!r}: need None, 'all' or a collection of names from {HEADS}")


def _head_of(model):
    """-> "GCN" / "GAT" / "GIN" / "Cheb" for the four heads, None for any other module."""
    from .model import ChebModel, GATModel, GINModel, GNNModel
    for cls, name in ((GNNModel, "GCN"), (GATModel, "GAT"), (GINModel, "GIN"), (ChebModel, "Cheb")):
        if isinstance(model, cls):
            return name
    return None


def _head_dims(model, head):
    """(hidden width, classes) of a head."""
    if head == "GCN":
        return model.gcn1.out_channels, model.gcn2.out_channels
    if head == "GAT":
        return model.GAT.convs[0].out_channels * model.GAT.convs[0].heads, model.GAT.convs[1].out_channels
    if head == "GIN":
        return model.GIN.convs[0].nn.lins[0].out_features, model.GIN.convs[1].nn.lins[0].out_features
    return model.gcn1.lins[0].out_features, model.gcn2.lins[0].out_features


def _eval_forward_ticks(head) -> int:
    """Dropout seeds one eval-mode forward of the head takes: GNNModel and GAT draw one on every call, GIN and Cheb only when training
    with p > 0."""
    return 1 if head in ("GCN", "GAT") else 0


def _run_batched(args, model, cluster_loader, device, q, mode, n_draws):
    """The serial loop's result with every partition's draws in batched passes (ops.ensemble_partition_head: one host call per partition)."""
    if mode not in ('learned', 'random', 'edge', 'full'):
        raise ValueError("Invalid mode. Choose 'learned', 'random', or 'full'.")
    flag = args.sgs_eval_batch
    avg, rep, per_class = _f1_opts(args)
    model.eval()
    counts = conf = None
    noises = list(getattr(args, "_sgs_noise_eval", None) or [])
    trace = getattr(args, "_sgs_trace_eval", None)
    head = _head_of(model)
    H, C = _head_dims(model, head)
    ticks = _eval_forward_ticks(head)
    variant = dict(gat_heads=getattr(model, "gat_heads", 1), gat_edge=bool(getattr(model, "gat_edge_weight", False)),
                   cheb_k=getattr(model, "cheb_k", 1), cover=cover_nodes(args))       # (under the flag only with sgs_eval_batch_cover: _batched_ok)
    if getattr(model, "gin_edge_weight", False):
        variant["gine_in"] = model.GIN.convs[0].in_channels                          # (here only with sgs_eval_batch_gine: _batched_ok)
    if getattr(model, "gat_v2", False):
        variant["gat_v2"] = True                                                     # (here only with sgs_eval_batch_gatv2: _batched_ok)
    with torch.no_grad():
        for batch in cluster_loader:
            batch = batch.to(device)
            ops.new_memo_scope()
            if counts is None:
                counts = torch.zeros(6, dtype=torch.int64, device=device)
            E, N = batch.edge_index.shape[1], batch.x.shape[0]
            given = [noises.pop(0) if noises else None for _ in range(n_draws)]     # the serial loop pops one per draw, whatever the mode
            if mode == 'full' or E <= q:
                out = model(batch, batch.edge_index)                                 # every draw runs on the whole partition
                _DropoutClock.tick += (n_draws - 1) * ticks                          # the serial loop's other n_draws - 1 forwards
                acc = torch.empty_like(out)
                ops.ensemble_mean_correct(out, 0, n_draws, acc, True, True, n_draws, batch.y,
                                          (batch.train_mask, batch.val_mask, batch.test_mask), counts)
                if trace is not None:
                    trace["logits"], trace["mean"] = out.unsqueeze(0).expand(n_draws, *out.shape), acc
                    trace["edges"] = batch.edge_index.unsqueeze(0).expand(n_draws, *batch.edge_index.shape)
                if per_class:
                    conf = _add_confusion(conf, acc, batch)
                continue
            if mode == 'learned':
                ops.get_pairs(batch.edge_index, N, build=True)
                p = model.edge_prob_mlp(batch.x, batch.edge_index).squeeze().contiguous()
                kind = ops.SAMPLE_LEARNED
            elif mode == 'edge':
                p, kind = batch.prob, ops.SAMPLE_PRIOR
            else:
                p, kind = None, ops.SAMPLE_LEARNED
                given = [None] * n_draws                                             # random_edge_sampling takes no noise
            passes, d = [], 0
            for k in plan_draws(E, q, N, H, C, n_draws, flag, head=head, **variant):
                while k > 0:                                                         # a pass never mixes explicit noise and clock draws
                    explicit = given[d] is not None
                    n = 1
                    while n < k and (given[d + n] is not None) == explicit:
                        n += 1
                    if explicit:
                        passes.append((n, torch.stack([t.to(device, torch.float32) for t in given[d:d + n]]).contiguous(), 0, 0))
                    else:
                        passes.append((n, None, _NoiseClock.seed, _NoiseClock.tick + 1))
                        _NoiseClock.tick += n
                    d += n
                    k -= n
            acc = ops.ensemble_partition_head(batch, model, q, kind, p, passes, counts, trace, cover=cover_graph(args, batch))
            if per_class:
                conf = _add_confusion(conf, acc, batch)                              # the mean the last sgs_ensemble_mean_correct pass left
            # GNNModel.forward and GAT.forward take one dropout seed per call, in eval mode too (GIN and Cheb none): leave the dropout
            # clock where the serial loop's n_draws forwards leave it, so that training after an evaluation draws the same masks whichever
            # path evaluated
            _DropoutClock.tick += n_draws * ticks
    if counts is None:
        return _finish(avg, rep, None, (0, 0, 0))
    c = counts.tolist()
    return _finish(avg, rep, conf, tuple((c[2 * s] / c[2 * s + 1]) if c[2 * s + 1] > 0 else 0 for s in range(3)))


def evaluate(args, model, cluster_loader, device, q=500, mode=None, temperature=1.0):
    """evaluate.py:6-67.  args.sgs_precision ("fp32" default / "bf16"): the scorer's precision for the pass (ops.scorer_precision)."""
    with ops.scorer_precision(getattr(args, "sgs_precision", None)):
        return _run(args, model, cluster_loader, device, q, mode, 1)


def ensemble_evaluate(args, model, cluster_loader, device, q=500, mode=None, temperature=1.0):
    """evaluate.py:70-173: mean of the logits of args.num_samples_eval independent draws."""
    with ops.scorer_precision(getattr(args, "sgs_precision", None)):
        n_draws = int(args.num_samples_eval)
        if _batched_ok(args, model, n_draws):
            PATH_COUNTS["batched"] += 1
            return _run_batched(args, model, cluster_loader, device, q, mode, n_draws)
        PATH_COUNTS["serial"] += 1
        return _run(args, model, cluster_loader, device, q, mode, n_draws)
