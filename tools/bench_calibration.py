#!/usr/bin/env python3
"""Calibration table throughput (mivp_amd.calibration), timed on device events after a warm-up, on a 2-class 512 x 512 x 96
probability volume (the size DESIGN 4.15 predicts in 187 ms) with a uint8 reference.  Two probability fields:

- ``spread``: the softmax of logits of deviation 2 (every bin is hit);
- ``saturated``: the softmax of logits of deviation 32 (nearly every voxel in the first or the last bin, exact 0 and 1
  included), the common case of a trained model.

Each is timed with plain per-lane adds (the default) and with the wave-level combining of same-cell lanes
(``FLAG_COMBINE``), and next to
them the same tables composed from eager torch ops on the same GPU (per row a multiply / round / shift, then ``bincount``
with and without weights).  The eager tables are compared with the kernel's before anything is timed.  One JSON line per
case: ms per call, the eager ms and their ratio, the algorithmic bytes ``4 C V + V sizeof(ref)`` and that over time as a
fraction of the 6.3 TB/s HBM rate DESIGN 4.8 uses, and the call as a share of the 187 ms ``predict``.  The lines are appended
to profiles/calibration_bench.jsonl."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
PREDICT_MS = 187.0
SHAPE = (512, 512, 96)
NCLS = 2
Q = 1 << 20


def timed(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def eager_tables(probs, target, n_bins):
    """count / pos / qsum [C + 1, n_bins] from torch ops (inputs without invalid or ignored voxels)."""
    import torch
    ncls = probs.shape[0]
    p = probs.reshape(ncls, -1)
    t = target.reshape(-1).long()
    top, arg = p.max(0)
    rows = [(p[c], t == c) for c in range(ncls)] + [(top, arg == t)]
    out = []
    for pr, y in rows:
        q = torch.round(pr * float(Q)).long()
        b = torch.clamp((q * n_bins) >> 20, max=n_bins - 1)
        out.append(torch.stack([torch.bincount(b, minlength=n_bins), torch.bincount(b[y], minlength=n_bins),
                                torch.bincount(b, weights=q.double(), minlength=n_bins).long()]))
    return torch.stack(out, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bins", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import calibration as K
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    target = (torch.rand(SHAPE, device=dev, generator=gen) < 0.1).to(torch.uint8)
    nvox = target.numel()
    nbytes = 4 * NCLS * nvox + nvox * target.element_size()
    lines = []
    for field, sigma in (("spread", 2.0), ("saturated", 32.0)):
        probs = torch.softmax(torch.randn((NCLS,) + SHAPE, device=dev, generator=gen) * sigma, 0)
        rep = K.CalibrationReport(NCLS, a.bins, dev)
        K.calibration_tables(probs, target, NCLS, a.bins, out=rep)
        want = eager_tables(probs, target, a.bins)
        assert torch.equal(torch.stack([rep.count, rep.pos, rep.qsum]), want)
        other = K.calibration_tables(probs, target, NCLS, a.bins, flags=K.FLAG_COMBINE)
        assert torch.equal(other.tables, rep.tables)
        edge = float(rep.count[0, [0, -1]].sum()) / nvox          # row 0's share in its first and last bin
        eager_ms = timed(lambda: eager_tables(probs, target, a.bins), max(3, a.calls // 10), 2)
        for case, flags in (("plain", 0), ("combine", K.FLAG_COMBINE)):
            ms = timed(lambda: K.calibration_tables(probs, target, NCLS, a.bins, out=rep, flags=flags), a.calls, a.warmup)
            rec = {"shape": list(SHAPE), "classes": NCLS, "n_bins": a.bins, "field": field, "case": case,
                   "edge_bin_share": round(edge, 4), "ms": round(ms, 4), "eager_ms": round(eager_ms, 4),
                   "eager_over_kernel": round(eager_ms / ms, 2), "bytes": int(nbytes),
                   "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM, 3), "predict_ms": PREDICT_MS,
                   "share_of_predict": round(ms / PREDICT_MS, 5)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
