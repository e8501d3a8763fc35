"""Argument-validation table of the edge scorer's C entry points: tests/golden/scorer_entry_table.json.

    SGS_LIB_PATH=<library to record from> python tests/golden/gen_scorer_entry_table.py     # rewrites the json

Every case is one call that must return BEFORE the first kernel launch or memset -- a bad hidden size, a dropout probability of 1, zero
rows, a null pointer, a workspace one byte short, ... -- so the table runs without a GPU, with dummy non-null pointers.  The recorded result
of a case is the return code and the full text of sgs_last_error().  tests/test_scorer_entry_table_cpu.py imports `cases` and `run_case`
from here and compares the library under test with the recorded table, so a refactor of the launchers cannot move a check, reorder two
checks or reword a message unnoticed.

The committed table was recorded from the library built at commit 490170e ("GAT / Chebyshev kernels: one copy of the per-head row
code"), the parent of the launcher refactor.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "scorer_entry_table.json")
SGS_OK, SGS_EINVAL, SGS_EWORKSPACE, SGS_EHIP = 0, -1, -2, -3

_BUF = ctypes.create_string_buffer(4096)
DUMMY = ctypes.addressof(_BUF)          # a non-null pointer that no case may reach a kernel with

BASE = dict(N=300, H=128, E=1000, M=500, n=700, n_active=700, nnz=1000, edge_id_offset=0, p_drop=0.25, p_hidden=0.25, p_ep=0.125, seed=1, site=2,
            seed_x=3, site_x=4, seed_y=5, site_y=6, sign_out=1.0, sign_in=-1.0)

FP32 = (6, 300)             # not 4 <= H <= 256 with H % 4 == 0, not 256 < H <= 1024 with H % 32 == 0
LOOP = (64, 512)            # the 128 / 256-only forms
# entry point -> (unsupported H values, the argument that counts rows, pointers that may be NULL with rows > 0, workspace kind)
SPEC = {
    "sgs_edge_score_fwd": (FP32, "E", (), "fwd"),
    "sgs_edge_score_fwd_paired": (FP32 + (64,), "E", (), "fwd"),
    "sgs_edge_score_fwd_mask": (FP32 + LOOP, "E", (), "fwd"),
    "sgs_edge_score_fwd_bf16": (LOOP, "E", (), "fwd"),
    "sgs_edge_score_fwd_paired_bf16": (LOOP, "E", (), "fwd"),
    "sgs_edge_score_fwd_mask_bf16": (LOOP, "E", (), "fwd"),
    "sgs_edge_score_bwd_core": (FP32, "n_active", (), "bwd"),
    "sgs_edge_score_bwd_core_bits": (LOOP, "n_active", (), "bwd"),
    "sgs_edge_score_bwd_dfeat": (LOOP, "n", (), "dfeat"),
    "sgs_edge_score_bwd_dfeat_bits": (LOOP, "n", (), "dfeat"),
    "sgs_edge_score_bwd_dfeat_bits_bf16": (LOOP, "n", (), "dfeat"),
    "sgs_edge_score_bwd_prep": ((100,), "n_active", (), None),
    "sgs_edge_score_bwd_prep_sd": ((100,), "n_active", (), None),
    "sgs_edge_score_bwd_prep_sd_pack": (LOOP, "n_active", (), "dfeat"),
    "sgs_edge_score_bwd_prep_sd_pack_bf16": (LOOP, "n_active", (), "dfeat"),
    "sgs_edge_score_bwd_dfeat_fused": (LOOP, "n", (), "dfeat"),
    "sgs_edge_score_bwd_dfeat_fused_bf16": (LOOP, "n", (), "dfeat"),
    "sgs_edge_score_bwd_dfeat_fused_packed": (LOOP, "n", (), "dfeat"),
    "sgs_edge_score_bwd_dfeat_fused_packed_bf16": (LOOP, "n", (), "dfeat"),
    "sgs_edge_score_bwd_reduce_fused": ((100,), "N", ("out_U_raw",), None),
    "sgs_edge_score_dw2_from_parts": ((0,), None, (), None),
    "sgs_edge_score_epd_fwd": (FP32 + (20,), "E", (), "epd"),
    "sgs_edge_score_epd_bwd_core": (FP32 + (20,), "n_active", (), "epd"),
    "sgs_edge_score_epd_reduce": ((6, 0), "N", ("active_eid",), None),
    "sgs_endpoint_reduce": ((-1,), "N", ("T", "in_src", "in_eid", "out_dst", "out_eid"), None),
    "sgs_endpoint_reduce_pair": ((6,), "N", ("in_src", "in_eid", "out_dst", "out_eid"), None),
    "sgs_endpoint_reduce_pair_bits": ((100,), "N", ("in_src", "in_eid", "out_dst", "out_eid", "out_U_raw"), None),
}


def _protos():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import sgs_gnn_amd
    return sgs_gnn_amd._lib.parse_header()


def cases():
    """-> [(case id, entry point, {argument: value}, returns SGS_OK)]; a pointer argument is "ptr" (dummy) or None."""
    protos = _protos()
    exported = sorted(n for n, (_, argtypes, _) in protos.items()
                      if (n.startswith("sgs_edge_score_") or n.startswith("sgs_endpoint_reduce")) and ctypes.c_void_p in argtypes
                      and n != "sgs_edge_score_probe_trace")
    assert exported == sorted(SPEC), "an entry point with pointers to validate is missing from SPEC (or SPEC names one that is gone)"
    out = []
    for fn in sorted(SPEC):
        bad_h, rows, optional, _ = SPEC[fn]
        _, argtypes, names = protos[fn]
        ptrs = [n for n, t in zip(names, argtypes) if t is ctypes.c_void_p and n != "stream"]
        base = {n: ("ptr" if n in ptrs else BASE[n]) for n in names if n not in ("stream", "ws_bytes")}

        def add(kind, ok=False, **over):
            out.append((f"{fn}:{kind}", fn, dict(base, **over), ok))

        for h in bad_h:
            add(f"H={h}", H=h)
        for p in ("p_drop", "p_hidden", "p_ep"):
            if p in names:
                add(f"{p}=1", **{p: 1.0})
        if rows:
            add(f"{rows}=0", ok=True, **dict({rows: 0}, **({"M": 0} if "M" in names else {})))
        if "M" in names:
            add("M=0", ok=True, M=0)
            add("M>E", M=BASE["E"] + 1)
            add("canon_without_mate", mate=None)
        if fn == "sgs_endpoint_reduce":
            add("H=0", ok=True, H=0)
        if "N" in names:
            add("N=-1", N=-1)
        for p in ptrs:
            if p not in optional:
                add(f"null_{p}", **{p: None})
        if "ws_bytes" in names:
            add("ws_short", ws_short=True)
        if "active_eid" in names and "n_active" in names:
            add("n_active!=E_null_active", active_eid=None)
    out.append(("sgs_edge_score_fwd:wide_N=0", "sgs_edge_score_fwd",
                dict({n: "ptr" for n in ("codes", "U", "edge_index", "W1", "b1", "w2", "b2", "p_out", "ws")}, N=0, H=512, E=1000, edge_id_offset=0,
                     p_drop=0.25, seed=1, site=2), False))
    return out


def _ws_bytes(L, fn, a):
    kind = SPEC[fn][3]
    if kind == "epd":
        return L.sgs_edge_score_epd_workspace_bytes(a["H"])
    N, E = {"fwd": (a.get("N", 0), a.get("E", 0)), "bwd": (a.get("N", 0), 0), "dfeat": (0, 0)}[kind]
    return L.sgs_edge_score_workspace_bytes(N, a["H"], E)


def run_case(L, protos, fn, a):
    """Calls entry point `fn` of the loaded library `L` -> [return code, sgs_last_error() text]."""
    _, argtypes, names = protos[fn]
    vals = []
    for n, t in zip(names, argtypes):
        if n == "stream":
            vals.append(None)
        elif n == "ws_bytes":
            vals.append(max(0, _ws_bytes(L, fn, a) - (1 if a.get("ws_short") else 0)))
        elif t is ctypes.c_void_p:
            vals.append(DUMMY if a[n] == "ptr" else None)
        else:
            vals.append(a[n])
    rc = getattr(L, fn)(*vals)
    return [rc, (L.sgs_last_error() or b"").decode() if rc != 0 else ""]


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import sgs_gnn_amd
    L, protos = sgs_gnn_amd._lib.lib(), sgs_gnn_amd._lib.parse_header()
    table = {}
    for cid, fn, a, ok in cases():
        rc, msg = run_case(L, protos, fn, a)
        assert rc != SGS_EHIP, f"{cid}: reached the HIP runtime ({msg}): not a validation case"
        assert (rc == SGS_OK) == ok and rc in (SGS_OK, SGS_EINVAL, SGS_EWORKSPACE), f"{cid}: rc={rc} ({msg})"
        table[cid] = [rc, msg]
    with open(TABLE, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} cases from {sgs_gnn_amd._lib.LIB_PATH} -> {TABLE}")


if __name__ == "__main__":
    main()
