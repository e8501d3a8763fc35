"""bench.py --dump-outputs: the arrays written after the timed steps (CPU check of the writer; the GPU run is bench.py itself)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_parameters_gradients_and_return(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    import sgs_gnn_amd as S
    model, *_ = bench.build_model(S, "cpu")
    for name, p in model.named_parameters():
        p.grad = torch.full_like(p, 0.5) if name.startswith("gcn") else None
    bench.dump_outputs(str(tmp_path), model, (3.25, 0.7, 10, 20))
    files = set(os.listdir(tmp_path))
    names = [n for n, _ in model.named_parameters()]
    assert files == {"train_return.npy"} | {f"param.{n}.npy" for n in names} | {f"grad.{n}.npy" for n in names if n.startswith("gcn")}
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= bench.DUMP_LIMIT_BYTES
    ret = np.load(tmp_path / "train_return.npy")
    assert ret.dtype == np.float64 and ret.tolist() == [3.25, 0.7, 10.0, 20.0]
    for n, p in model.named_parameters():
        a = np.load(tmp_path / f"param.{n}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, p.detach().numpy())
    assert np.all(np.load(tmp_path / "grad.gcn1.lin.weight.npy") == 0.5)


def test_dump_outputs_is_refused_off_the_s3_line(tmp_path):
    import subprocess
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "S2", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "S3 line only" in r.stderr
    assert not out.exists()
