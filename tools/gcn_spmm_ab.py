"""The CSR SpMM / SDDMM entry points of this tree against the parent commit's on the MI355X: the same bits, the same launch times.

    python tools/gcn_spmm_ab.py --parent-root DIR [--bench-ab FILE] [--skip-speed] [--out profiles/r36_gcn_spmm_ab.json]

DIR is a checkout of the parent commit with its library built.  Every GPU run is a child process with the package imported from this
tree ("branch") or from DIR ("parent"); each child has a time limit of its own and the first one that does not exit 0 stops the run.

Bits: one child per tree runs, on the inputs of this tree's tests (so both trees see the same arrays),
  - every tests/gcn_ref.py SPMM_CASES / SDDMM_CASES case with N <= 4096: sgs_spmm_csr under all SPMM_COMBOS, sgs_sddmm_csr;
  - the two graphs and the widths of tests/test_gpu_spmm_long_rows.py, long rows on and off: sgs_spmm_csr_next, sgs_spmm_csr_bwd_prev
    (with W, and column sums only), sgs_spmm_csr_dual, sgs_spmm_csr_next_dual, and sgs_spmm_csr_multi over the two graphs as two draws;
  - every tests/cheb_kernels_ref.py STEP_CASES case under all STEP_COMBOS: sgs_cheb_spmm (Y and Y2),
and writes the SHA-256 of every output array's bytes.  The two lists must be equal entry by entry: the same bytes, which is
torch.equal and NaN payloads besides.
Speed: tools/spmm_skew_probe.py --root, children in the order b p p b b p.  Per case and tree: the median of the three children's
medians and the [min, max] over all their rounds.  Condition per case: the branch median lies inside the parent's [min, max] of this call
widened on each side by the parent's own (max - min) -- the margin is what the shared machine did to the parent during the same minutes,
not a figure chosen in advance.  `--bench-ab FILE`: a JSON file of bench.py result lines ({"parent": ..., "branch": ...}) to embed."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ("branch", "parent", "parent", "branch", "branch", "parent")
CHILD_LIMIT_S = {"bits": 420, "speed": 240}


# ------------------------------------------------------------------------------------------------ the bits child
def bits_child(root, out):
    sys.path[:0] = [root, HERE, os.path.join(HERE, "tests")]
    import torch
    import sgs_gnn_amd as S
    assert os.path.abspath(os.path.dirname(S.__file__)).startswith(os.path.abspath(root)), (S.__file__, root)
    import cheb_kernels_ref as CR
    import gcn_ref as R
    import test_gpu_cheb_kernels as TC
    import test_gpu_gcn_variants as TV
    import test_gpu_spmm_long_rows as TL
    L, ops, DEV = S._lib.lib(), S.ops, "cuda:0"
    rec = []

    def put(name, *arrays):
        torch.cuda.synchronize()
        for t, a in enumerate(arrays):
            a = a.detach().contiguous().cpu()
            rec.append({"name": f"{name} #{t}", "floats": a.numel(), "sha256": hashlib.sha256(a.numpy().tobytes()).hexdigest()})

    for case in (c for c in R.SPMM_CASES if c["N"] <= 4096):
        gr = R.graph(case["N"], case["nnz"], case["nw"], case["hub"])
        dev = {k: gr[k].to(DEV) for k in ("ptr", "col", "val")}
        for diag_on, bias_on, act in R.SPMM_COMBOS:
            X, diag, bias = R.spmm_inputs(case["N"], case["D"], R.DROP_BIAS if act == R.ACT_RELU_DROPOUT else 0.0)
            Xd = TV.shifted(X, 1 if case["align"] == "a" else 0)
            _, Y = TV.run_spmm(S, case, gr, dev, Xd, diag.to(DEV) if diag_on else None, bias.to(DEV) if bias_on else None, act,
                               1 if case["align"] == "b" else 0)
            put(f"spmm_csr {case['name']} diag={diag_on} bias={bias_on} act={act}", Y)
    for case in (c for c in R.SDDMM_CASES if c["N"] <= 4096):
        gr = R.graph(case["N"], case["nnz"], case["nw"], case["hub"])
        dev = {k: gr[k].to(DEV) for k in ("ptr", "col", "eid")}
        A, B = (torch.randn(case["N"], case["D"], generator=gr["gen"]) for _ in range(2))
        _, g, _, gd = TV.run_sddmm(S, case, gr, dev, TV.shifted(A, 1 if case["align"] == "a" else 0),
                                   TV.shifted(B, 1 if case["align"] == "b" else 0), True)
        put(f"sddmm_csr {case['name']}", g, gd)

    thr = L.sgs_spmm_long_rows_threshold()
    ln4 = TL.nw4_lengths(thr)
    ln16 = torch.randint(256, 301, (301,), generator=torch.Generator().manual_seed(5)).tolist()
    ln16[0], ln16[150], ln16[300] = 256, 300, 257
    graphs = {"nw4": (TL.build_csr(ln4, 1), TL.build_csr(ln4, 2)), "nw16": (TL.build_csr(ln16, 3), TL.build_csr(ln16, 4))}
    gen = torch.Generator().manual_seed(9)
    for gname, (GA, GB) in graphs.items():
        N, nnz = GA["N"], GA["nnz"]
        ptr2, col2, val2 = (torch.stack([GA[k], GB[k]]).contiguous().to(DEV) for k in ("ptr", "col", "val"))
        for width in TL.WIDTHS:
            for diag_on, bias_on, act in TL.COMBOS:
                D, XA, diagA, bias, off = TL.inputs(GA, width, act)
                _, XB, diagB, _, _ = TL.inputs(GB, width, act, seed=6)
                Dn = 41 if D >= 64 else 64
                XAd, XBd = TL.shifted(XA, off), TL.shifted(XB, off)
                da, db = (diagA.to(DEV) if diag_on else None), (diagB.to(DEV) if diag_on else None)
                bd = bias.to(DEV) if bias_on else None
                Wn, W = torch.randn(Dn, D, generator=gen).to(DEV), torch.randn(D, Dn, generator=gen).to(DEV)
                Yp = torch.relu(torch.randn(N, Dn, generator=gen)).to(DEV)
                X2 = torch.stack([XA, XB]).contiguous().to(DEV)
                d2 = torch.stack([diagA, diagB]).contiguous().to(DEV) if diag_on else None
                for on in (1, 0):
                    tag = f"{gname} D={width} diag={diag_on} bias={bias_on} act={act} long={on}"
                    with TL.switch(L, on):
                        put(f"spmm_csr_next {tag}", *TL.call_next(S, GA, XAd, da, bd, act, Wn))
                        put(f"spmm_csr_bwd_prev W {tag}", *TL.call_bwd(S, GA, XAd, da, W, Yp, act))
                        put(f"spmm_csr_bwd_prev colsum {tag}", *TL.call_bwd(S, GA, XAd, da, None, None, R.ACT_NONE))
                        put(f"spmm_csr_dual {tag}", *TL.call_dual(S, GA, GB, XAd, XBd, da, db, bd, act))
                        put(f"spmm_csr_next_dual {tag}", *TL.call_next_dual(S, GA, GB, XAd, da, db, bd, act, Wn))
                        Ym = TL.nan(2, N, D)
                        ops._lib.check(L.sgs_spmm_csr_multi(X2.data_ptr(), N * D, N, D, nnz + R.PAD, 2, ptr2.data_ptr(), col2.data_ptr(),
                                                            val2.data_ptr(), TL.dptr(d2), TL.dptr(bd), min(act, R.ACT_RELU), Ym.data_ptr(),
                                                            ops._stream()), "sgs_spmm_csr_multi")
                        put(f"spmm_csr_multi {tag}", Ym)

    for case in CR.STEP_CASES:
        gr = CR.case_graph(case)
        n = case["nnz"]
        dev = dict(ptr=gr["ptr"].to(DEV), col=gr["col"].to(DEV) if n else None, val=gr["val"].to(DEV) if n else None)
        x = CR.step_inputs(case)
        for combo in CR.STEP_COMBOS:
            r = TC.run_step(S, case, combo, dev, x)
            put(f"cheb_spmm {case['name']} {combo['name']}", *([r["Y"]] + ([r["Y2"]] if r["Y2"] is not None else [])))
    with open(out, "w") as f:
        json.dump(rec, f)


# ------------------------------------------------------------------------------------------------ the parent process
def run_child(kind, cmd):
    env = {k: v for k, v in os.environ.items() if k != "SGS_LIB_PATH"}
    r = subprocess.run(cmd, timeout=CHILD_LIMIT_S[kind], env=env)
    if r.returncode != 0:
        raise SystemExit(f"gcn_spmm_ab: child {' '.join(cmd[1:])} exited {r.returncode}; stopping")


def load(tmp):
    with open(tmp) as f:
        res = json.load(f)
    os.remove(tmp)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--bench-ab", default=None)
    ap.add_argument("--skip-speed", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r36_gcn_spmm_ab.json"))
    ap.add_argument("--child-bits", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_bits:
        return bits_child(a.child_bits, a.out)
    trees = {"branch": HERE, "parent": os.path.abspath(a.parent_root)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    bits = {}
    for tree, root in trees.items():
        tmp = a.out + f".bits.{tree}.tmp"
        run_child("bits", [sys.executable, os.path.abspath(__file__), "--parent-root", trees["parent"], "--child-bits", root, "--out", tmp])
        bits[tree] = load(tmp)
    b, p = bits["branch"], bits["parent"]
    differing = [x["name"] for x, y in zip(b, p) if x != y]
    same = len(b) == len(p) and not differing
    entries = {}
    for x in b:
        e = entries.setdefault(x["name"].split(" ")[0], {"arrays": 0, "floats": 0})
        e["arrays"] += 1
        e["floats"] += x["floats"]
    out = {"tool": "tools/gcn_spmm_ab.py",
           "bits": {"arrays_compared": len(b), "floats_compared": sum(x["floats"] for x in b), "per_entry_point": entries,
                    "arrays_in_parent": len(p), "differing": differing, "all_equal": same}}
    print(f"[ab] bits: {len(b)} arrays, {out['bits']['floats_compared']} floats -> {'all equal' if same else 'DIFFERENT: ' + str(differing[:5])}",
          flush=True)
    ok = same
    if not a.skip_speed:
        runs = {t: {} for t in trees}
        for i, tree in enumerate(ORDER):
            tmp = a.out + f".speed.{tree}{i}.tmp"
            run_child("speed", [sys.executable, os.path.join(HERE, "tools", "spmm_skew_probe.py"), tmp, "--root", trees[tree]])
            res = load(tmp)
            for ename, per_graph in res["us"].items():
                for gname, v in per_graph.items():
                    for sw in ("on", "off"):
                        runs[tree].setdefault(f"{ename} {gname} long={sw}", []).append(
                            {"median": v[sw], "min": v[sw + "_min_max"][0], "max": v[sw + "_min_max"][1]})
            out.setdefault("graphs", res["graphs"])
        cases, inside_all = {}, True
        for case in runs["parent"]:
            arm = {t: {"median": statistics.median(r["median"] for r in runs[t][case]), "min": min(r["min"] for r in runs[t][case]),
                       "max": max(r["max"] for r in runs[t][case]), "child_medians": [r["median"] for r in runs[t][case]]} for t in trees}
            pa = arm["parent"]
            spread = pa["max"] - pa["min"]
            inside = pa["min"] - spread <= arm["branch"]["median"] <= pa["max"] + spread
            inside_all = inside_all and inside
            cases[case] = {"us": arm, "parent_spread_us": round(spread, 2), "branch_median_inside_widened_parent_range": inside}
            print(f"[ab] {case}: branch {arm['branch']['median']:.1f} us, parent {pa['median']:.1f} [{pa['min']:.1f}, {pa['max']:.1f}] -> "
                  f"{'inside' if inside else 'OUTSIDE'}", flush=True)
        out["speed"] = {"probe": "tools/spmm_skew_probe.py", "order": ORDER, "cases": cases, "all_inside": inside_all}
        ok = ok and inside_all
    if a.bench_ab and os.path.exists(a.bench_ab):
        with open(a.bench_ab) as f:
            out["bench_ab"] = json.load(f)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
