"""The device batch builders of this tree against the parent commit's on the MI355X: time per batch of the neighbour-sampled collate
(uniform draw) and of the cluster collate, at the shapes of tools/neighbor_weighted_probe.py and tools/cluster_batch_probe.py.

    python tools/batch_rows_ab.py --parent-root DIR [--rounds 3] [--bench-ab FILE] [--out profiles/r35_batch_rows_ab.json]

DIR is a checkout of the parent commit with its library built.  Both probes are run as child processes with the package imported from
this tree ("branch") or from DIR ("parent"), in the order b p p b b p, each child with its own arms alternating over `--rounds` rounds
after an untimed one (`neighbor_weighted_probe.py --uniform-only --root`, `cluster_batch_probe.py --collate-only --root`).  Per case and
tree: the median of the three children's medians and the [min, max] over all their rounds.  Condition per case: the branch median lies
inside the parent's [min, max] of this call widened on each side by the parent's own (max - min) -- the margin is what the shared
machine did to the parent during the same minutes, not a figure chosen in advance.  `--bench-ab FILE`: a JSON file of bench.py result
lines ({"parent": ..., "branch": ...}) to embed."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ("branch", "parent", "parent", "branch", "branch", "parent")
PROBES = {"neighbor": ("neighbor_weighted_probe.py", "--uniform-only"), "cluster": ("cluster_batch_probe.py", "--collate-only")}


def _cases(probe, res):
    """one child's result -> {case: its median / min / max record}"""
    if probe == "cluster":
        return {f"cluster collate {k}": v["us_per_batch"]["hip"] for k, v in res["collate"].items()}
    out = {f"neighbor select {k}": v["us_per_call_two_launches"]["uniform"] for k, v in res["select"].items()}
    out.update({f"neighbor collate {k}": v["us_per_batch"]["hip_uniform"] for k, v in res["collate"].items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-ab", default=None)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r35_batch_rows_ab.json"))
    a = ap.parse_args()
    trees = {"branch": HERE, "parent": os.path.abspath(a.parent_root)}
    runs, extra = {t: {} for t in trees}, {}
    for i, tree in enumerate(ORDER):
        for probe, (script, flag) in PROBES.items():
            tmp = a.out + f".{probe}.{tree}{i}.tmp"
            cmd = [sys.executable, os.path.join(HERE, "tools", script), flag, "--root", trees[tree], "--rounds", str(a.rounds), "--out", tmp]
            subprocess.run(cmd, check=True, timeout=600, env={k: v for k, v in os.environ.items() if k != "SGS_LIB_PATH"})
            with open(tmp) as f:
                res = json.load(f)
            os.remove(tmp)
            for case, rec in _cases(probe, res).items():
                runs[tree].setdefault(case, []).append(rec)
            extra.setdefault(f"{probe} {tree}", {k: res[k] for k in ("device", "graph", "collate_mismatch_word", "hub_row") if k in res})
    cases, ok = {}, True
    for case in runs["parent"]:
        arm = {t: {"median": statistics.median(r["median"] for r in runs[t][case]), "min": min(r["min"] for r in runs[t][case]),
                   "max": max(r["max"] for r in runs[t][case]), "child_medians": [r["median"] for r in runs[t][case]]} for t in trees}
        p = arm["parent"]
        spread = p["max"] - p["min"]
        inside = p["min"] - spread <= arm["branch"]["median"] <= p["max"] + spread
        ok = ok and inside
        cases[case] = {"us": arm, "parent_spread_us": spread, "branch_median_inside_widened_parent_range": inside}
        print(f"[ab] {case}: branch {arm['branch']['median']:.1f} us, parent {p['median']:.1f} [{p['min']:.1f}, {p['max']:.1f}] -> "
              f"{'inside' if inside else 'OUTSIDE'}", flush=True)
    out = {"tool": "tools/batch_rows_ab.py", "order": ORDER, "rounds_per_child": a.rounds, "cases": cases, "all_inside": ok, "children": extra}
    if a.bench_ab and os.path.exists(a.bench_ab):
        with open(a.bench_ab) as f:
            out["bench_ab"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
