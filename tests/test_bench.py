"""bench.py's --dump-outputs: what the last timed step returned, written as float32 .npy files that two runs (or two builds)
can compare output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(6, 4)
        self.frozen = torch.nn.Linear(4, 4)
        self.bn = torch.nn.BatchNorm1d(4)
        self.frozen.requires_grad_(False)

    def forward(self, x):
        return self.bn(self.frozen(self.lin(x)))


def test_step_outputs_and_dump(tmp_path):
    import bench
    torch.manual_seed(0)
    net = torch.nn.Module()
    net.module = _Toy()                                  # as DistributedDataParallel holds it: the bare module's names count
    opt = torch.optim.AdamW([p for p in net.module.parameters() if p.requires_grad], lr=1e-2)
    loss = net.module(torch.randn(8, 6)).square().mean()
    loss.backward()
    opt.step()
    outs = bench.step_outputs(net, opt, loss.detach(), ssl=False)
    assert set(outs) == {"loss", "param.lin.weight", "param.lin.bias", "grad.lin.weight", "grad.lin.bias",
                         "param.bn.weight", "param.bn.bias", "grad.bn.weight", "grad.bn.bias",
                         "buffer.bn.running_mean", "buffer.bn.running_var"}
    bench.dump_outputs(str(tmp_path / "full"), outs)
    for k, t in outs.items():
        a = np.load(tmp_path / "full" / (k + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, t.detach().float().numpy()), k

    big = {"a": torch.arange(3000, dtype=torch.float64), "b": torch.randn(10, 100)}
    limit = 4 * 1000
    bench.dump_outputs(str(tmp_path / "s1"), big, limit=limit)
    bench.dump_outputs(str(tmp_path / "s2"), big, limit=limit)
    total = 0
    for k, t in big.items():
        a1, a2 = np.load(tmp_path / "s1" / (k + ".npy")), np.load(tmp_path / "s2" / (k + ".npy"))
        assert a1.dtype == np.float32 and np.array_equal(a1, a2), k          # the same fixed sample every time
        assert np.isin(a1, t.float().reshape(-1).numpy()).all(), k
        assert a1.size == int(t.numel() * limit / (4 * 4000)), k
        total += a1.nbytes
    assert total <= limit
    assert np.all(np.diff(np.load(tmp_path / "s1" / "a.npy")) > 0)           # positions kept in order


def _bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--steps", "3", "--warmup", "1",
                        "--settle", "4", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dump_outputs_repeat(tmp_path):
    """Two plain runs with the same arguments: one result line each with the timed step count, and the same outputs bit
    for bit (seeded inputs, a fixed settle count, deterministic kernels)."""
    d1, d2 = _bench(tmp_path / "r1"), _bench(tmp_path / "r2")
    for d in (d1, d2):
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["unit"] == "volumes/s" and d["higher_is_better"] is True
        assert abs(d["value"] - d["config"]["global_batch"] * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
        assert "roofline" not in d and "cpu_baseline" not in d                 # those take --full
    names = sorted(os.listdir(tmp_path / "r1"))
    assert names == sorted(os.listdir(tmp_path / "r2")) and "loss.npy" in names
    assert any(n.startswith("param.") for n in names) and any(n.startswith("grad.") for n in names)
    assert float(np.load(tmp_path / "r1" / "loss.npy")) == d1["config"]["final_loss"]
    for n in names:
        a, b = np.load(tmp_path / "r1" / n), np.load(tmp_path / "r2" / n)
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, b), n
