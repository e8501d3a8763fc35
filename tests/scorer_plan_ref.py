"""A frozen copy of the edge scorer's path choice as it stood before the choices moved into ops._plan_forward / ops._plan_backward:
the `if`s of _EdgeScore.forward, _EdgeScore.backward, the dense body, _edge_score_backward_mask and _edge_score_backward_fused, in
their order and with their own spellings (the literal 65536, `ctx.bf16 and kept`, `bool(kept) and ctx.bf16`), as pure functions of
the same inputs.  Each returns the C entry points that code would call, in order, and the PRECISION_COUNTS key it would bump; the
forward also what it left on its ctx.  `sw` = (_mask_backward, _fwd_mask, _fused_backward).  Also the active-row prologue that
_EdgeScore.backward and _EdgeScoreEPD.backward both carried.  Nothing here imports the package: `L` is the loaded library.

Not to be edited with ops.py: tests/test_scorer_plan_cpu.py compares the two."""


def _variant_overrides_are_default(L):
    return L.sgs_edge_score_get_variant() < 0 and L.sgs_edge_score_get_bwd_variant() < 0


def forward_ref(L, sw, E, H, N, pairs_given, codes_grad, precision, is_src_sorted):
    """-> (entries, counts key, (kept, ctx.bf16, ctx.src_sorted))"""
    _mask_backward, _fwd_mask, _fused_backward = sw
    kept = False
    bf16 = (precision == "bf16" and E >= 65536 and L.sgs_edge_score_bf16_supported(H) and _variant_overrides_are_default(L))
    if (_fwd_mask and _mask_backward and E >= 65536 and L.sgs_edge_score_bwd_bits_supported(H) and codes_grad
            and _variant_overrides_are_default(L)):
        kept = True
        fn = "sgs_edge_score_fwd_mask_bf16" if bf16 else "sgs_edge_score_fwd_mask"
    elif pairs_given and E >= 65536 and L.sgs_edge_score_paired_supported(H):
        fn = "sgs_edge_score_fwd_paired_bf16" if bf16 else "sgs_edge_score_fwd_paired"
    else:
        fn = "sgs_edge_score_fwd_bf16" if bf16 else "sgs_edge_score_fwd"
    key = "fwd_bf16" if bf16 else "fwd_fp32"
    ctx_bf16 = bool(bf16 and kept)
    ctx_src_sorted = bool(kept and _fused_backward and is_src_sorted())
    return [fn], key, (kept, ctx_bf16, ctx_src_sorted)


def backward_ref(L, sw, n, H, N, codes_grad, kept, ctx_bf16, ctx_src_sorted, ascending):
    """-> (entries, counts key).  ascending: ActiveSet.ascending, None without an active set (eid None).  The last entry is the tail's
    _leaf_dw outside a deferred_weight_grads scope."""
    _mask_backward, _fwd_mask, _fused_backward = sw
    eid_is_none = ascending is None
    if (_mask_backward and n >= 65536 and L.sgs_edge_score_bwd_bits_supported(H) and L.sgs_gemm_tn_mask_supported(n, H, H)
            and codes_grad):
        key = "bwd_bf16" if ctx_bf16 and kept else "bwd_fp32"
        return _backward_mask_ref(sw, kept, ctx_bf16, ctx_src_sorted, eid_is_none, ascending), key
    key = "bwd_fp32"
    calls = []
    if n > 0:
        calls.append("sgs_edge_score_bwd_core")
    if n >= 65536 and L.sgs_edge_score_bwd_dfeat_supported(H):
        calls.append("sgs_edge_score_bwd_dfeat")
    if L.sgs_gemm_tn_can_colsum(n, H, H):
        calls.append("sgs_gemm_tn_ld")
    else:
        calls += ["sgs_gemm_tn_ld", "sgs_colsum"]
    calls += ["sgs_colsum", "sgs_colsum"]
    if H % 4 == 0:
        calls.append("sgs_endpoint_reduce_pair")
    else:
        calls += ["sgs_endpoint_reduce", "sgs_endpoint_reduce"]
    calls.append("sgs_gemm_tn_ld")
    return calls, key


def _backward_mask_ref(sw, kept, ctx_bf16, ctx_src_sorted, eid_is_none, ascending):
    _mask_backward, _fwd_mask, _fused_backward = sw
    in_order = eid_is_none or bool(ascending)
    if kept and ctx_src_sorted and _fused_backward and in_order:
        bf16 = ctx_bf16
        b = "_bf16" if bf16 else ""
        return ["sgs_edge_score_bwd_prep_sd_pack" + b, "sgs_edge_score_bwd_dfeat_fused_packed" + b, "sgs_gemm_tn_mask_gather" + b,
                "sgs_edge_score_bwd_reduce_fused", "sgs_edge_score_dw2_from_parts", "sgs_gemm_tn_ld"]
    calls = []
    hdz = False
    if kept:
        calls.append("sgs_edge_score_bwd_prep")
    else:
        hdz = True
        calls.append("sgs_edge_score_bwd_core_bits")
    bf16 = bool(kept) and ctx_bf16
    calls.append("sgs_edge_score_bwd_dfeat_bits_bf16" if bf16 else "sgs_edge_score_bwd_dfeat_bits")
    calls.append("sgs_gemm_tn_mask_bf16" if bf16 else "sgs_gemm_tn_mask")
    if hdz:
        calls.append("sgs_colsum")
    calls.append("sgs_endpoint_reduce_pair_bits")
    if not hdz:
        calls.append("sgs_edge_score_dw2_from_parts")
    calls.append("sgs_gemm_tn_ld")
    return calls


def active_rows_ref(act, gp, edge_index, N, dev, zero_token, get_graph):
    """The prologue as both backwards carried it -> (eid, graph, n, gp_act)."""
    E = edge_index.shape[1]
    if act is not None and act.eid is not None:
        eid, graph = act.eid, act.graph
        n = eid.numel()
        tok = zero_token(dev)
        if act.gq is not None and gp.numel() == E and gp.stride(0) == 0 and gp.data_ptr() == tok.data_ptr():
            gp_act = act.gq                     # handed over by _SelectSampled: `gp` is the stride-0 zero, nothing to gather
        else:
            gp_act = gp.index_select(0, eid)
            if act.gq is not None:              # another consumer of the scores contributed a dense gradient as well
                gp_act = gp_act + act.gq
        act.gq = None
    else:
        eid, graph, n = None, get_graph(edge_index, N), E
        gp_act = gp.contiguous()
    return eid, graph, n, gp_act
