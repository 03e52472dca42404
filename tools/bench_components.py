#!/usr/bin/env python3
"""Connected-component labelling and post-processing throughput (mivp_amd.components), timed on device events after a
warm-up.  Volumes are built on the device:

- ``blobsK``: a K-class map of ellipsoids side by side (as tools/bench_surface.py) plus ~0.1 % random single-voxel
  islands of random classes (what a noisy sliding-window prediction leaves), at 256x256x160 and 512x512x96;
- the worst cases at 512x512x96: ``all_fg`` (one component of every voxel), ``checker`` (a 3-D checkerboard: N / 2
  components at 6-connectivity, one at 26), ``rand0.3`` (a random mask at density 0.3, near the 26-connectivity
  percolation threshold: a few huge components span the volume) and ``serpentine`` (one 1-voxel-wide path through every
  even H plane).

One JSON line per case: ms per volume for ``label_components`` (without its one host read of n) and for
``postprocess_labels(largest=True)`` (blob maps: also ``min_size=64`` alone), both at 26-connectivity.  If scipy is
importable, the CPU time of ``scipy.ndimage.label`` on the 2-class map's foreground is reported once per shape, for context.

Kernel shares come from a run under the kernel tracer:
    rocprofv3 --kernel-trace --stats -d OUT -o cc -- python tools/bench_components.py --volumes 2 --no-scipy
then ``python tools/bench_components.py --stats OUT/.../cc_kernel_stats.csv`` prints each kernel's share."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"256x256x160": (256, 256, 160), "512x512x96": (512, 512, 96)}
WORST = ("all_fg", "checker", "rand0.3", "serpentine")


def blobs(shape, ncls, dev):
    """uint8 [1, 1, H, W, D]: ncls - 1 ellipsoids side by side along W plus random single-voxel islands."""
    import torch
    g = torch.Generator(device=dev).manual_seed(7)
    H, W, D = shape
    h = torch.arange(H, device=dev, dtype=torch.float32).view(H, 1, 1)
    w = torch.arange(W, device=dev, dtype=torch.float32).view(1, W, 1)
    d = torch.arange(D, device=dev, dtype=torch.float32).view(1, 1, D)
    out = torch.zeros(shape, dtype=torch.uint8, device=dev)
    nf = ncls - 1
    for k in range(1, ncls):
        c = [H / 2, W * (k - 0.5) / nf, D / 2]
        r = [H * 0.35, W * 0.4 / nf, D * 0.35]
        out[((h - c[0]) / r[0]) ** 2 + ((w - c[1]) / r[1]) ** 2 + ((d - c[2]) / r[2]) ** 2 <= 1.0] = k
    isl = torch.rand(shape, generator=g, device=dev) < 1e-3
    cls = torch.randint(1, ncls, shape, generator=g, device=dev, dtype=torch.uint8)
    out[isl] = cls[isl]
    return out.view((1, 1) + shape)


def worst(name, shape, dev):
    import torch
    H, W, D = shape
    if name == "all_fg":
        m = torch.ones(shape, dtype=torch.uint8, device=dev)
    elif name == "checker":
        i = [torch.arange(n, device=dev) for n in shape]
        m = ((i[0].view(H, 1, 1) + i[1].view(1, W, 1) + i[2].view(1, 1, D)) % 2 == 0).to(torch.uint8)
    elif name == "rand0.3":
        g = torch.Generator(device=dev).manual_seed(3)
        m = (torch.rand(shape, generator=g, device=dev) < 0.3).to(torch.uint8)
    else:                                            # serpentine: rows w = 0, 2, ... of every even plane, joined
        m = torch.zeros(shape, dtype=torch.uint8, device=dev)
        m[0::2, 0::2, :] = 1
        for i, w in enumerate(range(1, W - 1, 2)):
            m[0::2, w, D - 1 if i % 2 == 0 else 0] = 1
        end_d = D - 1 if (W // 2 - 1) % 2 == 0 else 0
        for i, h in enumerate(range(1, H - 1, 2)):
            if i % 2 == 0:
                m[h, W - 2, end_d] = 1
            else:
                m[h, 0, 0] = 1
    return m.view((1, 1) + shape)


def timed(fn, volumes, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(volumes):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / volumes, 3)


def label_device(x, conn):
    """label_components without the host read of n (the device work only)."""
    import ctypes as C
    import torch
    from mivp_amd import _lib as L
    from mivp_amd._host import LABEL_DTYPES, i3, workspace
    v = x[0, 0]
    labels = torch.empty(tuple(v.shape), dtype=torch.int32, device=v.device)
    n = torch.empty(1, dtype=torch.int32, device=v.device)
    ws = workspace("label", v.shape, v.device)
    L.call("mivp_label_components", L.ptr(v), C.c_int32(LABEL_DTYPES[v.dtype]), i3(v.shape), C.c_int32(conn), L.ptr(labels),
           L.ptr(n), L.ptr(ws), L.stream())
    return labels, n


def run_case(name, shape, x, ncls, volumes, warmup):
    from mivp_amd.components import label_components, postprocess_labels
    _, n = label_components(x, 26)
    rec = {"case": name, "shape": list(shape), "classes": ncls, "components_26": n,
           "label_ms": timed(lambda: label_device(x, 26), volumes, warmup),
           "largest_ms": timed(lambda: postprocess_labels(x, ncls, largest=True), volumes, warmup)}
    if name.startswith("blobs"):
        rec["min_size_ms"] = timed(lambda: postprocess_labels(x, ncls, largest=False, min_size=64), volumes, warmup)
    return rec


def scipy_case(x):
    from scipy import ndimage
    m = (x[0, 0] > 0).cpu().numpy()
    t0 = time.perf_counter()
    ndimage.label(m, ndimage.generate_binary_structure(3, 3))
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
    ap.add_argument("--no-scipy", action="store_true", help="skip the CPU scipy timing")
    ap.add_argument("--stats", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool")
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
        return
    import torch
    import mivp_amd  # noqa: F401
    try:
        import scipy.ndimage  # noqa: F401
        have_scipy = not a.no_scipy
    except ImportError:
        have_scipy = False
    dev = torch.device("cuda:0")
    for sname, shape in SHAPES.items():
        for ncls in (2, 4):
            x = blobs(shape, ncls, dev)
            print(json.dumps(run_case(f"blobs{ncls}", shape, x, ncls, a.volumes, a.warmup)), flush=True)
            if have_scipy and ncls == 2:
                print(json.dumps({"case": "blobs2", "shape": list(shape),
                                  "scipy_label_cpu_s": round(scipy_case(x), 3)}), flush=True)
    shape = SHAPES["512x512x96"]
    for name in WORST:
        x = worst(name, shape, dev)
        print(json.dumps(run_case(name, shape, x, 2, a.volumes, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
