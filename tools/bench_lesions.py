#!/usr/bin/env python3
"""Region statistics and lesion-wise metrics throughput (mivp_amd.regions), timed on device events after a warm-up.
Volumes are 512x512x96 and built on the device:

- ``lesions``: a 2-class map with a few dozen ellipsoidal lesions; the prediction is the reference shifted by a few
  voxels with some lesions dropped and a few false alarms added; the image is an int16 noise volume;
- the worst cases: ``all_fg`` (one region of every voxel: every workgroup flushes the same table entry) and ``checker``
  (a 3-D checkerboard at 6-connectivity: N / 2 regions, far above ``max_regions``, so the region tables overflow and
  the pair table holds the pairs of the listed regions only), and ``checker_fit`` (a checkerboard in one corner sized to stay just under
  ``max_regions`` regions and ``max_pairs`` pairs).

One JSON line per case with ms per volume for: ``label_ms`` (the labelling alone), ``region_stats_ms`` (labelling + the
fused reduction, with the image), ``lesion_metrics_ms`` (two labellings + reductions + overlap table + matching),
``torch_stats_ms`` (the same region fields from a composition of torch ops on the same GPU: ``bincount`` /
``scatter_reduce`` over ``label_components`` output, labelling included) and, unless ``--no-scipy``, ``scipy_stats_cpu_s``
(``scipy.ndimage.label`` + ``find_objects`` / ``sum`` / ``center_of_mass`` on the CPU).

``--shape`` runs something else and nothing of the above: ``region_shape`` (mivp_amd.regions) recorded in a
graph and replayed, on the ``lesions`` reference map and on ``all_fg``, three timings each, next to ``region_stats`` (no
image) and an eager torch composition of the second moments and exposed-face counts, all in the one job.  One JSON line per
case with the three timings of each, ``shape_over_stats``, and ``shape_over_bytes`` = the replay over what the label map's
bytes take at 6.3 TB/s.

Kernel shares: ``rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o les -- python tools/bench_lesions.py --volumes 2
--no-scipy --no-torch``."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (512, 512, 96)
MAX_REGIONS = 4096


def lesions(shape, dev, count=48, seed=7):
    """(pred, target) uint8 [H, W, D]: `count` ellipsoids at random places; pred = target shifted, 1 in 6 dropped, 8 added."""
    import torch
    g = torch.Generator().manual_seed(seed)
    H, W, D = shape
    h = torch.arange(H, device=dev, dtype=torch.float32).view(H, 1, 1)
    w = torch.arange(W, device=dev, dtype=torch.float32).view(1, W, 1)
    d = torch.arange(D, device=dev, dtype=torch.float32).view(1, 1, D)

    def blob(out, c, r):
        out[((h - c[0]) / r[0]) ** 2 + ((w - c[1]) / r[1]) ** 2 + ((d - c[2]) / r[2]) ** 2 <= 1.0] = 1

    tgt = torch.zeros(shape, dtype=torch.uint8, device=dev)
    pred = torch.zeros(shape, dtype=torch.uint8, device=dev)
    for i in range(count + 8):
        c = (torch.rand(3, generator=g) * torch.tensor([H, W, D])).tolist()
        r = (3 + torch.rand(3, generator=g) * torch.tensor([20.0, 20.0, 8.0])).tolist()
        if i < count:
            blob(tgt, c, r)
            if i % 6:
                blob(pred, [c[0] + 2, c[1] - 1, c[2] + 1], r)
        else:
            blob(pred, c, r)
    return pred, tgt


def checker(shape, dev, corner=None):
    import torch
    H, W, D = shape
    i = [torch.arange(n, device=dev) for n in shape]
    m = ((i[0].view(H, 1, 1) + i[1].view(1, W, 1) + i[2].view(1, 1, D)) % 2 == 0).to(torch.uint8)
    if corner is not None:
        keep = torch.zeros(shape, dtype=torch.bool, device=dev)
        keep[:corner[0], :corner[1], :corner[2]] = True
        m = m * keep
    return m


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
    import ctypes as C
    import torch
    from mivp_amd import _lib as L
    from mivp_amd._host import LABEL_DTYPES, i3, workspace
    labels = torch.empty(tuple(x.shape), dtype=torch.int32, device=x.device)
    n = torch.empty(1, dtype=torch.int32, device=x.device)
    ws = workspace("label", x.shape, x.device)
    L.call("mivp_label_components", L.ptr(x), C.c_int32(LABEL_DTYPES[x.dtype]), i3(x.shape), C.c_int32(conn), L.ptr(labels),
           L.ptr(n), L.ptr(ws), L.stream())
    return labels, n


def torch_stats(x, image, conn, cap=MAX_REGIONS):
    """The region fields from torch ops over the dense labels (labels above cap dropped, as the fused pass does)."""
    import torch
    labels, _ = label_device(x, conn)
    lab = labels.reshape(-1).long()
    idx = torch.nonzero((lab > 0) & (lab <= cap)).squeeze(1)
    r = lab[idx] - 1
    H, W, D = x.shape
    hh, ww, dd = idx // (W * D), (idx // D) % W, idx % D
    size = torch.bincount(r, minlength=cap)
    out = {"size": size}
    out["first"] = torch.full((cap,), 2 ** 62, dtype=torch.int64, device=x.device).scatter_reduce(0, r, idx, "amin")
    for name, c in (("h", hh), ("w", ww), ("d", dd)):
        out["min_" + name] = torch.full((cap,), 2 ** 31, dtype=torch.int64, device=x.device).scatter_reduce(0, r, c, "amin")
        out["max_" + name] = torch.full((cap,), -1, dtype=torch.int64, device=x.device).scatter_reduce(0, r, c, "amax")
        out["sum_" + name] = torch.zeros(cap, dtype=torch.int64, device=x.device).scatter_add(0, r, c)
    v = image.reshape(-1)[idx].long()
    out["vmin"] = torch.full((cap,), 2 ** 31, dtype=torch.int64, device=x.device).scatter_reduce(0, r, v, "amin")
    out["vmax"] = torch.full((cap,), -2 ** 31, dtype=torch.int64, device=x.device).scatter_reduce(0, r, v, "amax")
    out["vsum"] = torch.zeros(cap, dtype=torch.int64, device=x.device).scatter_add(0, r, v)
    out["vsqsum"] = torch.zeros(cap, dtype=torch.int64, device=x.device).scatter_add(0, r, v * v)
    return out


def scipy_stats(x, image, conn):
    import numpy as np
    from scipy import ndimage
    m, img = x.cpu().numpy() > 0, image.cpu().numpy()
    t0 = time.perf_counter()
    lab, n = ndimage.label(m, ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn]))
    idx = np.arange(1, n + 1)
    ndimage.find_objects(lab)
    ndimage.sum(m, lab, idx)
    ndimage.center_of_mass(m, lab, idx)
    ndimage.mean(img, lab, idx)
    return time.perf_counter() - t0, n


def run_case(name, pred, tgt, image, conn, volumes, warmup, scipy_too, torch_too=True):
    from mivp_amd.regions import lesion_metrics, region_stats
    tab = region_stats(tgt, 2, image=image, connectivity=conn, max_regions=MAX_REGIONS)
    rep = lesion_metrics(pred, tgt, 2, connectivity=conn, max_regions=MAX_REGIONS)
    rec = {"case": name, "shape": list(tgt.shape), "connectivity": conn, "regions": int(tab.n),
           "region_overflow": int(tab.overflow), "pairs": int(rep.n_pairs), "pair_overflow": int(rep.pair_overflow),
           "label_ms": timed(lambda: label_device(tgt, conn), volumes, warmup),
           "region_stats_ms": timed(lambda: region_stats(tgt, 2, image=image, connectivity=conn), volumes, warmup),
           "lesion_metrics_ms": timed(lambda: lesion_metrics(pred, tgt, 2, connectivity=conn), volumes, warmup)}
    if torch_too:
        rec["torch_stats_ms"] = timed(lambda: torch_stats(tgt, image, conn), volumes, warmup)
    if scipy_too:
        s, n = scipy_stats(tgt, image, conn)
        rec["scipy_stats_cpu_s"], rec["scipy_regions"] = round(s, 3), int(n)
    return rec


STREAM_TBS = 6.3          # the streaming rate DESIGN 4.8 measured; what the bytes of a pass predict is bytes / this


def torch_shape(labels, cap=MAX_REGIONS):
    """The second moments and the exposed-face counts of ``region_shape`` from eager torch ops over the dense labels (the
    vertex and edge counts have no short composition and are left out, so this does less than the fused pass)."""
    import torch
    H, W, D = labels.shape
    ok = (labels > 0) & (labels <= cap)
    idx = torch.nonzero(ok.reshape(-1)).squeeze(1)
    r = labels.reshape(-1)[idx].long() - 1
    c = (idx // (W * D), (idx // D) % W, idx % D)
    out = {}
    for name, (a, b) in zip(("hh", "ww", "dd", "hw", "hd", "wd"), ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        out[name] = torch.zeros(cap, dtype=torch.int64, device=labels.device).scatter_add(0, r, c[a] * c[b])
    for axis, name in enumerate("hwd"):
        differs = labels.narrow(axis, 1, labels.shape[axis] - 1) != labels.narrow(axis, 0, labels.shape[axis] - 1)
        edge = torch.ones_like(labels.narrow(axis, 0, 1), dtype=torch.bool)
        exposed = torch.cat([edge, differs], axis).to(torch.int64) + torch.cat([differs, edge], axis).to(torch.int64)
        out["faces_" + name] = torch.zeros(cap, dtype=torch.int64, device=labels.device).scatter_add(
            0, r, exposed.reshape(-1)[idx])
    return out


def run_shape_case(name, x, conn, volumes, warmup, runs=3):
    """``region_shape`` recorded in a graph against ``region_stats`` and the eager torch composition, `runs` timings each."""
    import torch
    from mivp_amd.regions import region_shape, region_stats
    tab = region_stats(x, 2, connectivity=conn, max_regions=MAX_REGIONS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        region_shape(tab)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        shp = region_shape(tab)
    replays = max(volumes, 20)                           # a replay is short: time more of them
    shape_ms = [timed(g.replay, replays, warmup) for _ in range(runs)]
    stats_ms = [timed(lambda: region_stats(x, 2, connectivity=conn, max_regions=MAX_REGIONS), volumes, warmup)
                for _ in range(runs)]
    torch_ms = [timed(lambda: torch_shape(tab.labels), volumes, warmup) for _ in range(runs)]
    nbytes = tab.labels.numel() * 4                      # the pass reads the label map once
    bytes_ms = nbytes / (STREAM_TBS * 1e12) * 1e3
    mid = sorted(shape_ms)[runs // 2]
    return {"case": name, "shape": list(x.shape), "connectivity": conn, "regions": int(tab.n),
            "euler_sum": int(shp.euler.sum()), "region_shape_graph_ms": shape_ms, "region_stats_ms": stats_ms,
            "torch_shape_ms": torch_ms, "shape_over_stats": round(mid / sorted(stats_ms)[runs // 2], 3),
            "torch_over_shape": round(sorted(torch_ms)[runs // 2] / mid, 1), "label_bytes": nbytes,
            "bytes_at_stream_rate_ms": round(bytes_ms, 4), "shape_over_bytes": round(mid / bytes_ms, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-scipy", action="store_true", help="skip the CPU scipy timing")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition (kernel traces of this change alone)")
    ap.add_argument("--shape", action="store_true",
                    help="time region_shape (recorded in a graph) on the lesion map and on all_fg, next to region_stats and "
                         "an eager torch composition of the moments and face counts, three runs each; nothing else runs")
    a = ap.parse_args()
    import torch
    import mivp_amd  # noqa: F401
    if a.shape:
        dev = torch.device("cuda:0")
        _, tgt = lesions(SHAPE, dev)
        print(json.dumps(run_shape_case("lesions", tgt, 26, a.volumes, a.warmup)), flush=True)
        ones = torch.ones(SHAPE, dtype=torch.uint8, device=dev)
        print(json.dumps(run_shape_case("all_fg", ones, 26, a.volumes, a.warmup)), flush=True)
        return
    try:
        import scipy.ndimage  # noqa: F401
        have_scipy = not a.no_scipy
    except ImportError:
        have_scipy = False
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    image = torch.randint(-1024, 3072, SHAPE, generator=g, device=dev, dtype=torch.int16)
    pred, tgt = lesions(SHAPE, dev)
    print(json.dumps(run_case("lesions", pred, tgt, image, 26, a.volumes, a.warmup, have_scipy, not a.no_torch)), flush=True)
    ones = torch.ones(SHAPE, dtype=torch.uint8, device=dev)
    print(json.dumps(run_case("all_fg", ones, ones, image, 26, a.volumes, a.warmup, False, not a.no_torch)), flush=True)
    ck = checker(SHAPE, dev)
    print(json.dumps(run_case("checker", ck, ck, image, 6, a.volumes, a.warmup, False, not a.no_torch)), flush=True)
    fit = checker(SHAPE, dev, corner=(20, 20, 20))                  # 4000 regions and 4000 pairs: just under 4096
    print(json.dumps(run_case("checker_fit", fit, fit, image, 6, a.volumes, a.warmup, False, not a.no_torch)), flush=True)


if __name__ == "__main__":
    main()
