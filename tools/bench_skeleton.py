#!/usr/bin/env python3
"""Thinning and centreline-metric times (mivp_amd.skeleton), on device events: the median and min..max of
``--runs`` timed calls after a warm-up.  2-class 512x512x96 operands built on the device:

- ``vessels``: a synthetic vessel tree, 63 tubes of radius 6 down to 2 voxels that branch in the H-W plane;
- ``body``: the centred ellipsoid inscribed in the volume (the body of tools/bench_predict.py);
- ``all_fg``: every voxel foreground, the worst case (the most iterations, and every border voxel a candidate).

One JSON line per operand:
- ``skeletonize_ms``: ``skeletonize(x, 2)``, the converged loop with its one int32 host read per iteration;
- ``skeletonize_fixed_ms``: ``skeletonize(x, 2, max_iter=iterations)``, the same launches issued with no host read;
- ``iterations``, ``skeleton_voxels``;
- ``bytes_ms``: what ``9 * iterations`` passes over the map's bytes (one byte per voxel: a mark pass and eight sub-passes
  per iteration) would take at the 6.3 TB/s streaming figure of DESIGN 6, and ``x_bytes`` = skeletonize_fixed_ms over it;
- ``centerline_ms``: ``centerline_metrics(pred, x, 2)`` with pred = x shifted by (3, 2, 1) voxels: two thinnings, the
  counting pass and the two statistics passes;
- ``postprocess_ms``: ``postprocess_labels(x, 2, largest=True)`` on the same map, for scale."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (512, 512, 96)
STREAM_TBS = 6.3


def tubes(shape, dev):
    """uint8 [H, W, D]: a binary tree of 63 straight tubes; a child is 0.8 of its parent in length and radius (radius
    6 .. 2), turned +-35 degrees in the H-W plane and tilted a little along D"""
    import torch
    out = torch.zeros(shape, dtype=torch.uint8, device=dev)
    segs = []

    def grow(p, ang, tilt, length, radius, depth):
        q = (p[0] + length * math.cos(ang) * math.cos(tilt), p[1] + length * math.sin(ang) * math.cos(tilt),
             p[2] + length * math.sin(tilt))
        q = tuple(min(max(q[a], 8.0), shape[a] - 9.0) for a in range(3))
        segs.append((p, q, max(radius, 2.0)))
        if depth < 5:
            for k, s in enumerate((-1.0, 1.0)):
                grow(q, ang + s * math.radians(35), -tilt + s * 0.12 * (depth + 1 + k), length * 0.8, radius * 0.8, depth + 1)

    grow((24.0, shape[1] / 2.0, shape[2] / 2.0), 0.0, 0.05, 120.0, 6.0, 0)
    for p, q, r in segs:
        lo = [max(0, int(min(p[a], q[a]) - r - 1)) for a in range(3)]
        hi = [min(shape[a], int(max(p[a], q[a]) + r + 2)) for a in range(3)]
        g = torch.meshgrid(*[torch.arange(lo[a], hi[a], device=dev, dtype=torch.float32) for a in range(3)], indexing="ij")
        d = [q[a] - p[a] for a in range(3)]
        dd = sum(a * a for a in d) or 1.0
        t = sum((g[a] - p[a]) * d[a] for a in range(3)) / dd
        t = t.clamp(0.0, 1.0)
        dist2 = sum((g[a] - (p[a] + t * d[a])) ** 2 for a in range(3))
        box = out[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        box[dist2 <= r * r] = 1
    return out, len(segs)


def body(shape, dev):
    import torch
    ax = [((torch.arange(n, dtype=torch.float32, device=dev) + 0.5) / n * 2 - 1) ** 2 for n in shape]
    rho = ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :]
    return (rho <= 1.0).to(torch.uint8)


def timed(fn, runs, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def run_case(name, x, runs, warmup, extra=None):
    import torch
    from mivp_amd.components import postprocess_labels
    from mivp_amd.skeleton import centerline_metrics, skeletonize
    res = skeletonize(x, 2)
    it = res.iterations
    nbytes = x.numel()
    bytes_ms = 9 * it * nbytes / (STREAM_TBS * 1e12) * 1e3
    pred = torch.roll(x, (3, 2, 1), dims=(0, 1, 2))
    rec = {"case": name, "shape": list(x.shape), "foreground": int((x != 0).sum()), "iterations": it,
           "skeleton_voxels": int((res.skeleton != 0).sum()),
           "skeletonize_ms": timed(lambda: skeletonize(x, 2), runs, warmup),
           "skeletonize_fixed_ms": timed(lambda: skeletonize(x, 2, max_iter=it), runs, warmup),
           "bytes_ms": round(bytes_ms, 3)}
    rec["x_bytes"] = round(rec["skeletonize_fixed_ms"]["median"] / bytes_ms, 1)
    rec["centerline_ms"] = timed(lambda: centerline_metrics(pred, x, 2), runs, warmup)
    rep = centerline_metrics(pred, x, 2).cpu()
    rec["cldice"] = round(float(rep["cldice"][1]), 4)
    rec["centerline_iterations"] = list(rep["iterations"])
    rec["postprocess_ms"] = timed(lambda: postprocess_labels(x, 2, largest=True), runs, warmup)
    rec.update(extra or {})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="vessels,body,all_fg")
    a = ap.parse_args()
    import torch
    import mivp_amd  # noqa: F401
    dev = torch.device("cuda:0")
    for name in a.cases.split(","):
        extra = None
        if name == "vessels":
            x, n = tubes(SHAPE, dev)
            extra = {"tubes": n}
        elif name == "body":
            x = body(SHAPE, dev)
        elif name == "all_fg":
            x = torch.ones(SHAPE, dtype=torch.uint8, device=dev)
        else:
            raise SystemExit(f"unknown case {name}")
        print(json.dumps(run_case(name, x, a.runs, a.warmup, extra)), flush=True)


if __name__ == "__main__":
    main()
