#!/usr/bin/env python3
"""Surface-distance metrics throughput (mivp_amd.surface.surface_metrics), timed on device events after a warm-up
volume.  Synthetic ellipsoid label maps built on the device: the target holds num_classes - 1 ellipsoids side by side,
the prediction is a perturbed copy (each ellipsoid shifted and rescaled).  Cases: 256x256x160 and 512x512x96, 2 and 4
classes, spacings (1, 1, 1) and (0.8, 0.8, 2.5).

One JSON line per case: ms per volume for the whole metric (one surface map, per foreground class and direction one
EDT and one statistics chain, one host read), ms per EDT timed alone, and the algorithmic bytes of the EDT passes
(D pass: 1 byte read + 4 written per voxel; W and H passes: 4 read + 4 written per voxel; the envelope stacks are not
counted) against 6.3 TB/s.  If scipy is importable, the CPU time of the same metrics through scipy.ndimage is reported
once per shape (2 classes, unit spacing), for context.

Kernel shares come from a run under the kernel tracer:
    rocprofv3 --kernel-trace --stats -d OUT -o surf -- python tools/bench_surface.py --volumes 2 --no-scipy
then ``python tools/bench_surface.py --stats OUT/.../surf_kernel_stats.csv`` prints each kernel's share."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
SHAPES = {"256x256x160": (256, 256, 160), "512x512x96": (512, 512, 96)}
CLASSES = (2, 4)
SPACINGS = {"unit": (1.0, 1.0, 1.0), "aniso": (0.8, 0.8, 2.5)}
EDT_BYTES_PER_VOXEL = (1 + 4) + (4 + 4) + (4 + 4)


def ellipsoids(shape, ncls, dev, perturb):
    """uint8 [1, 1, H, W, D]: ncls - 1 ellipsoids side by side along W (class k in the k-th), optionally perturbed."""
    import torch
    g = torch.Generator().manual_seed(7)
    H, W, D = shape
    h = torch.arange(H, device=dev, dtype=torch.float32).view(H, 1, 1)
    w = torch.arange(W, device=dev, dtype=torch.float32).view(1, W, 1)
    d = torch.arange(D, device=dev, dtype=torch.float32).view(1, 1, D)
    out = torch.zeros(shape, dtype=torch.uint8, device=dev)
    nf = ncls - 1
    for k in range(1, ncls):
        c = [H / 2, W * (k - 0.5) / nf, D / 2]
        r = [H * 0.35, W * 0.4 / nf, D * 0.35]
        if perturb:
            c = [a + float(torch.empty(1).uniform_(-3, 3, generator=g)) for a in c]
            r = [a * float(torch.empty(1).uniform_(0.92, 1.08, generator=g)) for a in r]
        inside = ((h - c[0]) / r[0]) ** 2 + ((w - c[1]) / r[1]) ** 2 + ((d - c[2]) / r[2]) ** 2 <= 1.0
        out[inside] = k
    return out.view((1, 1) + shape)


def run_case(shape, ncls, spacing, volumes, warmup):
    import torch
    from mivp_amd.surface import distance_transform_sq, surface_map, surface_metrics
    dev = torch.device("cuda:0")
    tgt = ellipsoids(shape, ncls, dev, False)
    pred = ellipsoids(shape, ncls, dev, True)
    for _ in range(warmup):
        res = surface_metrics(pred, tgt, ncls, spacing)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(volumes):
        res = surface_metrics(pred, tgt, ncls, spacing)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / volumes
    seeds = surface_map(tgt, ncls)[0, 0] == 1
    for _ in range(warmup):
        distance_transform_sq(seeds, spacing)
    torch.cuda.synchronize()
    a.record()
    for _ in range(volumes):
        distance_transform_sq(seeds, spacing)
    b.record()
    torch.cuda.synchronize()
    edt_ms = a.elapsed_time(b) / volumes
    nvox = shape[0] * shape[1] * shape[2]
    edt_bytes = EDT_BYTES_PER_VOXEL * nvox
    return {"shape": list(shape), "classes": ncls, "spacing": list(spacing), "ms_per_volume": round(ms, 3),
            "edts_per_volume": 2 * (ncls - 1), "ms_per_edt": round(edt_ms, 3),
            "edt_bytes": edt_bytes, "edt_TB_per_s": round(edt_bytes / edt_ms / 1e9, 3),
            "edt_of_6.3TBps": round(edt_bytes / edt_ms * 1e3 / HBM, 4),
            "surface_voxels": res["surface_voxels"].tolist(), "hd95": [round(float(v), 4) for v in res["hd_p"]],
            "assd": [round(float(v), 4) for v in res["assd"]]}


def scipy_case(shape, ncls, spacing):
    """CPU seconds of the same metrics through scipy.ndimage (tests/surface_ref.py's definitions)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import surface_ref as R
    dev = torch.device("cuda:0")
    tgt = ellipsoids(shape, ncls, dev, False)[0, 0].cpu().numpy()
    pred = ellipsoids(shape, ncls, dev, True)[0, 0].cpu().numpy()
    t0 = time.perf_counter()
    R.scipy_metrics(pred, tgt, ncls, spacing)
    return time.perf_counter() - t0


def stats(path):
    total, rows = 0.0, []
    with open(path) as f:
        for row in csv.DictReader(f):
            ns = float(row.get("TotalDurationNs", 0) or 0)
            total += ns
            rows.append((row.get("Name", ""), int(row.get("Calls", 0) or 0), ns))
    for name, calls, ns in sorted(rows, key=lambda r: -r[2]):
        print(json.dumps({"kernel": name[:80], "calls": calls, "total_ms": round(ns / 1e6, 3),
                          "share_pct": round(100 * ns / total, 3) if total else None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shape", choices=list(SHAPES) + ["all"], default="all")
    ap.add_argument("--no-scipy", action="store_true", help="skip the CPU scipy timing")
    ap.add_argument("--stats", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
        return
    import mivp_amd  # noqa: F401
    try:
        import scipy.ndimage  # noqa: F401
        have_scipy = not a.no_scipy
    except ImportError:
        have_scipy = False
    for sname in (SHAPES if a.shape == "all" else [a.shape]):
        shape = SHAPES[sname]
        for ncls in CLASSES:
            for sp in SPACINGS.values():
                print(json.dumps(run_case(shape, ncls, sp, a.volumes, a.warmup)), flush=True)
        if have_scipy:
            s = scipy_case(shape, 2, SPACINGS["unit"])
            print(json.dumps({"shape": list(shape), "classes": 2, "spacing": list(SPACINGS["unit"]),
                              "scipy_cpu_s_per_volume": round(s, 3)}), flush=True)


if __name__ == "__main__":
    main()
