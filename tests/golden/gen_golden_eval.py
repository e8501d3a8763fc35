#!/usr/bin/env python3
"""Generate tests/golden/ensemble_eval_gcn.pt by RUNNING THE REFERENCE's `evaluate.ensemble_evaluate` unmodified (learned and edge
modes, 11 draws per partition).  Reuses gen_golden.py's PyG stand-in, multinomial / dropout recorders and graph helper by import
(that file is not changed), so the same rules hold: the reference's own code is pinned, the third-party GCN layer is not.

    python tests/golden/gen_golden_eval.py

Stored per mode: the Exp(1) noise every draw's multinomial consumed (in call order), the logits of every draw (a forward hook on the
model), the reference's averaged logits of every partition (torch.mean(torch.stack(outs))) and the F1 triple it returned.  Two
partitions: one with E > q (draws) and one with E <= q (the whole partition, no noise consumed).
"""
import argparse
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402


def main():
    G.install_pyg_stub()
    sys.path.insert(0, G.REF)
    rec = G.Recorder()
    rec.install()
    try:
        import evaluate as ref_eval
        import model as ref_model
        torch.manual_seed(2024)
        big = G.make_graph(48, 10, 12, 5, 131)
        small = G.make_graph(20, 4, 12, 5, 132)
        batches = [big, small]
        q = int(big.edge_index.shape[1] * 0.2)
        assert small.edge_index.shape[1] <= q < big.edge_index.shape[1]
        m = ref_model.GNNModel(12, 16, 5, dropout_prob=0.3, edge_mlp_type="GCN")
        with torch.no_grad():
            for k, v in m.named_parameters():
                if k.endswith("bias"):
                    v.uniform_(-0.05, 0.05)
            # a head that reads the graphs' class signal (x[:, y] += 2): predictions that vary with the drawn edges, not one class
            m.gcn1.lin.weight[:5, :5] += 1.5 * torch.eye(5)
            m.gcn2.lin.weight[:, :5] += 1.5 * torch.eye(5)
        state0 = G.sd_clone(m)
        draws = 11
        cap = []
        hook = m.register_forward_hook(lambda mod, i, o: cap.append(o.detach().clone()))
        modes = {}
        try:
            for mode in ("learned", "edge"):
                rec.clear()
                cap.clear()
                args = argparse.Namespace(degree_bias_coef=0.3, num_samples_eval=draws)
                f1 = ref_eval.ensemble_evaluate(args, m, batches, "cpu", q=q, mode=mode)
                assert len(cap) == draws * len(batches) and len(rec.noise) == draws
                logits = [torch.stack(cap[b * draws:(b + 1) * draws]) for b in range(len(batches))]
                modes[mode] = dict(f1=tuple(float(v) for v in f1), noise=[n for (_, _, n, _) in rec.noise],
                                   noise_idx=[i for (_, _, _, i) in rec.noise], logits=logits,
                                   mean=[torch.mean(lg, dim=0) for lg in logits])
                print(f"{mode}: f1={modes[mode]['f1']}")
        finally:
            hook.remove()
    finally:
        rec.uninstall()
    fx = dict(q=q, draws=draws, state0=state0, degree_bias_coef=0.3,
              batches=[dict(x=b.x, edge_index=b.edge_index, y=b.y, train_mask=b.train_mask, val_mask=b.val_mask, test_mask=b.test_mask,
                            prob=b.prob) for b in batches],
              modes=modes)
    torch.save(fx, os.path.join(HERE, "ensemble_eval_gcn.pt"))
    print(f"ensemble_eval_gcn.pt: E={[b.edge_index.shape[1] for b in batches]} q={q} draws={draws}")


if __name__ == "__main__":
    main()
