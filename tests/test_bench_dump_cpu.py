"""bench.py --dump-outputs: the writer of the last timed step's loss and gradients, on CPU tensors.  Every array is float32 / float64, a gradient
too large for the byte budget becomes a sample of its elements, and the same inputs give the same files."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _model():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(300, 200), torch.nn.LayerNorm(200)).to(torch.bfloat16)
    m[1].bias.requires_grad = False
    m(torch.randn(4, 300, dtype=torch.bfloat16)).float().square().sum().backward()
    return m


def test_dump_outputs_writes_float_arrays_within_the_budget_and_repeats(tmp_path):
    bench = _bench()
    m = _model()
    params = bench.trainable(m=m)
    assert [n for n, _ in params] == ["m.0.weight", "m.0.bias", "m.1.weight"]
    budget = 3 * 4 * 1000  # 1000 elements per gradient: the 300 x 200 weight is sampled, the rest are whole
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        bench.dump_outputs(str(d), torch.tensor(2.5), params, budget_bytes=budget)
    names = sorted(os.listdir(dirs[0]))
    assert names == ["grad.m.0.bias.npy", "grad.m.0.weight.npy", "grad.m.1.weight.npy", "grad_norms.npy", "loss.npy"]
    for f in names:
        a, b = np.load(dirs[0] / f), np.load(dirs[1] / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    assert sum(os.path.getsize(dirs[0] / f) for f in names if f.startswith("grad.")) <= budget + 3 * 128  # (+ the .npy headers)
    assert np.load(dirs[0] / "loss.npy").tolist() == [2.5]
    assert np.array_equal(np.load(dirs[0] / "grad.m.0.bias.npy"), m[0].bias.grad.float().numpy())
    w = m[0].weight.grad.float().reshape(-1).numpy()
    sample = np.load(dirs[0] / "grad.m.0.weight.npy")
    assert sample.shape == (1000,) and np.isin(sample, w).all()
    norms = np.load(dirs[0] / "grad_norms.npy")
    assert norms.dtype == np.float64 and abs(norms[0] - np.linalg.norm(w.astype(np.float64))) < 1e-9 * max(1.0, norms[0])
