#!/usr/bin/env python3
"""Whole-volume sliding-window prediction throughput (mivp_amd.inference.SlidingWindowPredictor), eager against one
recorded graph per sub-batch, timed on device events after a warm-up volume.  Two shapes:
  cfg1_96  : the cfg1 model (window 7^3), roi 96^3, a 1x1x256x256x160 volume, overlap 0.5, sub-batch 4
  yml_128x8: window (8, 8, 4), roi 128x128x8, a 1x1x512x512x96 volume, overlap 0.5, sub-batch 10
One JSON line per (shape, mode): windows/s, volumes/s, ms per volume, and the algorithmic bytes of gather + blend +
finalize per volume (from the shapes, below).  ``--mirror-axes 0,1,2`` turns on mirror test-time augmentation (the line
then also gives windows x flips per second), ``--maps`` asks for the probability, confidence and entropy maps (the
probability finalize instead of the plain one).

``--skip-background`` times window skipping (``SlidingWindowPredictor(skip=WindowSkip())``) instead: a
synthetic volume that is exactly 0 (air) outside an ellipsoid "body" filling ``1 - --air-fraction`` of the voxels, the
same volume predicted without and with skipping by graph predictors, alternating, on device events.  One JSON line per
shape: ms per volume without and with skipping, kept and total windows, and the time of the occupancy + compact + fill
launches on their own.

``--fit-foreground [--margin M]`` times fitting the windows to the foreground bounding box
(``SlidingWindowPredictor(fit=WindowFit(margin=M))``) on the same synthetic volume: predicted without either,
with skipping and with fitting by graph predictors, alternating, on device events.  One JSON line per shape: ms per volume
of the three, the windows each ran, the box, and the time of the box + plan + fill launches on their own.
``--air-fraction 0`` makes the box the whole volume: the line then shows what the feature costs when it removes nothing.

Kernel shares come from a run under the kernel tracer:
    rocprofv3 --kernel-trace --stats -d OUT -o pred -- python tools/bench_predict.py --volumes 2
then ``python tools/bench_predict.py --stats OUT/.../pred_kernel_stats.csv --volumes 2`` prints the stitching kernels'
share of kernel time and their bytes / time against 6.3 TB/s (bytes of that run, from the traffic model below).  Give
``--stats`` the ``--mirror-axes`` / ``--maps`` / ``--shape`` of the profiled run."""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
SHAPES = {
    "cfg1_96": dict(window=(7, 7, 7), roi=(96, 96, 96), image=(256, 256, 160), sub_batch=4),
    "yml_128x8": dict(window=(8, 8, 4), roi=(128, 128, 8), image=(512, 512, 96), sub_batch=10),
}
NCLS, CIN = 2, 1


def parse_axes(text):
    return tuple(int(a) for a in text.split(",") if a.strip() != "")


def traffic(name, mirror_axes=(), maps=False):
    """Algorithmic bytes of one predicted volume per kernel family: gather reads and writes every window element of each
    sub-batch (tail slots included); blend reads the logits of the valid entries and reads + writes the accumulator and
    weight sum over each sub-batch's union box; finalize reads the accumulator and weight sum of every image voxel and
    writes one label byte (with ``maps``: plus the C + 2 fp32 maps).  Under augmentation the entries are every window
    under every flip code, window-major, and the blend also reads + writes the compensation words over the box."""
    import numpy as np
    from mivp_amd.inference import flip_codes, window_origins
    s = SHAPES[name]
    roi, B = s["roi"], s["sub_batch"]
    rvol = int(np.prod(roi))
    flips = len(flip_codes(mirror_axes))
    windows = window_origins(s["image"], roi, 0.5).shape[0]
    o = np.repeat(window_origins(s["image"], roi, 0.5), flips, axis=0)
    n = o.shape[0]
    n_sub = -(-n // B)
    box = 0
    for k in range(n_sub):
        w = o[k * B:(k + 1) * B]
        box += int(np.prod([w[:, a].max() - w[:, a].min() + roi[a] for a in range(3)]))
    nvox = int(np.prod(s["image"]))
    return {"windows": windows, "flips": flips, "sub_batches": n_sub,
            "gather": 2 * n_sub * B * CIN * rvol * 4,
            "blend": n * rvol * NCLS * 4 + 2 * box * (NCLS + 1) * 4 * (2 if flips > 1 else 1),
            "finalize": nvox * ((NCLS + 1) * 4 + 1 + ((NCLS + 2) * 4 if maps else 0))}


def run(name, volumes, warmup, mirror_axes=(), maps=False):
    import torch
    from mivp_amd import train
    from mivp_amd.inference import SlidingWindowPredictor
    from mivp_amd.swin_unetr import SwinUnetR
    s = SHAPES[name]
    conf, _, _ = train.make_conf("cfg1", window=s["window"])
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SwinUnetR(conf).to(dev).eval()
    x = torch.rand((1, CIN) + s["image"], generator=torch.Generator().manual_seed(1)).to(dev)
    t = traffic(name, mirror_axes, maps)
    algo = t["gather"] + t["blend"] + t["finalize"]
    kw = dict(return_probs=True, return_confidence=True, return_entropy=True) if maps else {}
    out = []
    for mode in ("eager", "graph"):
        p = SlidingWindowPredictor(model, s["image"], CIN, NCLS, s["roi"], overlap=0.5, mode="gaussian",
                                   sub_batch=s["sub_batch"], graph=(mode == "graph"), mirror_axes=mirror_axes)
        for _ in range(warmup):
            labels = p.predict(x, **kw)["labels"]
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(volumes):
            labels = p.predict(x, **kw)["labels"]
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / volumes
        out.append({"shape": name, "mode": mode, "image": list(s["image"]), "roi": list(s["roi"]),
                    "sub_batch": s["sub_batch"], "windows": t["windows"], "mirror_axes": list(mirror_axes),
                    "flips": t["flips"], "maps": bool(maps), "ms_per_volume": round(ms, 3),
                    "volumes_per_s": round(1e3 / ms, 3), "windows_per_s": round(t["windows"] * 1e3 / ms, 1),
                    "window_flips_per_s": round(t["windows"] * t["flips"] * 1e3 / ms, 1),
                    "stitch_bytes_per_volume": algo, "label_hist": torch.bincount(labels.reshape(-1).long()).tolist()})
        del p
        torch.cuda.empty_cache()
    return out


def body_volume(image, air_fraction, dev):
    """fp32 [1, 1, image]: values in (0.1, 1] inside a centred ellipsoid with the image's aspect that holds
    ``1 - air_fraction`` of the voxels (clipped by the volume's faces when it must be larger than the inscribed one),
    exactly 0 outside it."""
    import torch
    ax = [((torch.arange(n, dtype=torch.float32, device=dev) + 0.5) / n * 2 - 1) ** 2 for n in image]
    rho = ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :]
    nvox = rho.numel()
    nbody = min(nvox, max(0, int(round((1.0 - air_fraction) * nvox))))
    x = 0.1 + 0.9 * torch.rand(image, generator=torch.Generator().manual_seed(1)).to(dev)
    if nbody < nvox:
        cut = torch.sort(rho.reshape(-1)).values[nbody] if nbody > 0 else -1.0
        x = torch.where(rho < cut, x, torch.zeros_like(x))
    return x[None, None].contiguous()


def run_skip(name, volumes, warmup, air_fraction, mirror_axes=()):
    import torch
    from mivp_amd import train
    from mivp_amd.inference import SlidingWindowPredictor, WindowSkip
    from mivp_amd.swin_unetr import SwinUnetR
    s = SHAPES[name]
    conf, _, _ = train.make_conf("cfg1", window=s["window"])
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SwinUnetR(conf).to(dev).eval()
    x = body_volume(s["image"], air_fraction, dev)
    air = float((x == 0).double().mean())
    kw = dict(overlap=0.5, mode="gaussian", sub_batch=s["sub_batch"], graph=True, mirror_axes=mirror_axes)
    preds = {"full": SlidingWindowPredictor(model, s["image"], CIN, NCLS, s["roi"], **kw),
             "skip": SlidingWindowPredictor(model, s["image"], CIN, NCLS, s["roi"], skip=WindowSkip(), **kw)}
    for p in preds.values():
        for _ in range(warmup):
            p.predict(x)
    torch.cuda.synchronize()
    ms = {k: [] for k in preds}
    for _ in range(volumes):                                     # alternate the two, one event pair per volume
        for k, p in preds.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            labels = p.predict(x)["labels"]
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    p = preds["skip"]
    # the feature's own launches: occupancy + compact + fill (the fill finds nothing to write after a finished volume)
    reps = 20
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        p._select(p.vol)
        p._fill()
    b.record()
    torch.cuda.synchronize()
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    return [{"shape": name, "mode": "graph", "image": list(s["image"]), "roi": list(s["roi"]), "sub_batch": s["sub_batch"],
             "mirror_axes": list(mirror_axes), "air_fraction": round(air, 4), "windows": p.n_windows, "kept": p.n_kept,
             "kept_over_windows": round(p.n_kept / p.n_windows, 4), "sub_batches": p.n_sub, "sub_batches_run": p.n_sub_run,
             "ms_per_volume_full": round(med["full"], 3), "ms_per_volume_skip": round(med["skip"], 3),
             "skip_over_full": round(med["skip"] / med["full"], 4),
             "ms_min_full": round(min(ms["full"]), 3), "ms_min_skip": round(min(ms["skip"]), 3),
             "occupancy_compact_fill_ms": round(a.elapsed_time(b) / reps, 4),
             "label_hist": torch.bincount(labels.reshape(-1).long()).tolist()}]


def run_fit(name, volumes, warmup, air_fraction, margin, mirror_axes=()):
    import torch
    from mivp_amd import train
    from mivp_amd.inference import SlidingWindowPredictor, WindowFit, WindowSkip
    from mivp_amd.swin_unetr import SwinUnetR
    s = SHAPES[name]
    conf, _, _ = train.make_conf("cfg1", window=s["window"])
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SwinUnetR(conf).to(dev).eval()
    x = body_volume(s["image"], air_fraction, dev)
    air = float((x == 0).double().mean())
    kw = dict(overlap=0.5, mode="gaussian", sub_batch=s["sub_batch"], graph=True, mirror_axes=mirror_axes)
    preds = {"full": SlidingWindowPredictor(model, s["image"], CIN, NCLS, s["roi"], **kw),
             "skip": SlidingWindowPredictor(model, s["image"], CIN, NCLS, s["roi"], skip=WindowSkip(), **kw),
             "fit": SlidingWindowPredictor(model, s["image"], CIN, NCLS, s["roi"], fit=WindowFit(margin=margin), **kw)}
    for p in preds.values():
        for _ in range(warmup):
            p.predict(x)
    torch.cuda.synchronize()
    ms = {k: [] for k in preds}
    for _ in range(volumes):                                     # alternate the three, one event pair per volume
        for k, p in preds.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            labels = p.predict(x)["labels"]
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    p = preds["fit"]
    # the feature's own launches: box + plan + fill (the fill finds nothing to write after a finished volume)
    reps = 20
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        p._plan(p.vol)
        p._fill()
    b.record()
    torch.cuda.synchronize()
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    return [{"shape": name, "mode": "graph", "image": list(s["image"]), "roi": list(s["roi"]), "sub_batch": s["sub_batch"],
             "mirror_axes": list(mirror_axes), "air_fraction": round(air, 4), "margin": margin, "box": p.box.tolist(),
             "windows": p.n_windows, "windows_skip": preds["skip"].n_kept, "windows_fit": p.n_kept,
             "sub_batches": p.n_sub, "sub_batches_skip": preds["skip"].n_sub_run, "sub_batches_fit": p.n_sub_run,
             "ms_per_volume_full": round(med["full"], 3), "ms_per_volume_skip": round(med["skip"], 3),
             "ms_per_volume_fit": round(med["fit"], 3), "fit_over_full": round(med["fit"] / med["full"], 4),
             "ms_min_full": round(min(ms["full"]), 3), "ms_min_skip": round(min(ms["skip"]), 3),
             "ms_min_fit": round(min(ms["fit"]), 3), "box_plan_fill_ms": round(a.elapsed_time(b) / reps, 4),
             "label_hist": torch.bincount(labels.reshape(-1).long()).tolist()}]


def stats(path, volumes, warmup, shapes, mirror_axes=(), maps=False):
    """Share of kernel time and bytes / time of the stitching kernels in a profiled run of ``shapes``.  The flip-aware
    gather / blend and the probability finalize are the kernels of a run with ``mirror_axes`` / ``maps``."""
    tta = len(mirror_axes) > 0
    fam = {"gather": "k_window_gather_tta" if tta else "k_window_gather",
           "blend": "k_window_blend_tta" if tta else "k_window_blend",
           "finalize": "k_stitch_finalize_probs" if maps else "k_stitch_finalize", "advance": "k_window_advance"}
    total_ns, fam_ns, fam_calls = 0.0, {k: 0.0 for k in fam}, {k: 0 for k in fam}
    with open(path) as f:
        for row in csv.DictReader(f):
            ns = float(row.get("TotalDurationNs", 0) or 0)
            total_ns += ns
            m = re.search(r"\bk_[a-z_]+", row.get("Name", ""))
            kernel = m.group(0) if m else ""
            for k, kname in fam.items():
                if kernel == kname:
                    fam_ns[k] += ns
                    fam_calls[k] += int(row.get("Calls", 0) or 0)
    # predicts per shape and mode: warm-up + timed volumes; graph recording adds two eager sub-batches (not counted)
    nvol = 2 * (volumes + warmup)
    byts = {k: 0 for k in ("gather", "blend", "finalize")}
    for name in shapes:
        t = traffic(name, mirror_axes, maps)
        for k in byts:
            byts[k] += nvol * t[k]
    for k in fam:
        line = {"kernel": fam[k], "calls": fam_calls[k], "total_ms": round(fam_ns[k] / 1e6, 3),
                "share_pct": round(100 * fam_ns[k] / total_ns, 3) if total_ns else None}
        if k in byts and fam_ns[k] > 0:
            line["bytes"] = byts[k]
            line["TB_per_s"] = round(byts[k] / fam_ns[k] / 1e3, 3)
            line["of_6.3TBps"] = round(byts[k] / fam_ns[k] * 1e9 / HBM, 3)
        print(json.dumps(line))
    st = sum(fam_ns.values())
    print(json.dumps({"stitch_share_of_kernel_time_pct": round(100 * st / total_ns, 3) if total_ns else None,
                      "stitch_vs_rest_pct": round(100 * st / (total_ns - st), 3) if total_ns > st else None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volumes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shape", choices=list(SHAPES) + ["all"], default="all")
    ap.add_argument("--mirror-axes", type=parse_axes, default=(), metavar="A[,A..]",
                    help="mirror test-time augmentation over these spatial axes (0 = H, 1 = W, 2 = D), e.g. 0,1,2")
    ap.add_argument("--maps", action="store_true", help="also return probs / confidence / entropy (probability finalize)")
    ap.add_argument("--skip-background", action="store_true",
                    help="time window skipping against the unfiltered prediction on a synthetic body-in-air volume")
    ap.add_argument("--fit-foreground", action="store_true",
                    help="time fitting the windows to the foreground box against the unfiltered and the skipping prediction")
    ap.add_argument("--margin", type=int, default=0, help="with --fit-foreground: voxels added around the box per axis")
    ap.add_argument("--air-fraction", type=float, default=0.5,
                    help="with --skip-background / --fit-foreground: the fraction of voxels that are air (exactly 0), in "
                         "[0, 1]")
    ap.add_argument("--stats", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run of this tool with the same "
                                    "--shape / --mirror-axes / --maps")
    a = ap.parse_args()
    if not 0.0 <= a.air_fraction <= 1.0:
        ap.error("--air-fraction must be in [0, 1]")
    if a.margin < 0:
        ap.error("--margin must be >= 0")
    if a.fit_foreground and a.skip_background:
        ap.error("--fit-foreground already times skipping next to fitting: give one of the two")
    import mivp_amd  # noqa: F401
    shapes = list(SHAPES) if a.shape == "all" else [a.shape]
    if a.stats:
        stats(a.stats, a.volumes, a.warmup, shapes, a.mirror_axes, a.maps)
        return
    for name in shapes:
        try:
            if a.fit_foreground:
                lines = run_fit(name, a.volumes, a.warmup, a.air_fraction, a.margin, a.mirror_axes)
            else:
                lines = (run_skip(name, a.volumes, a.warmup, a.air_fraction, a.mirror_axes) if a.skip_background
                         else run(name, a.volumes, a.warmup, a.mirror_axes, a.maps))
        except (RuntimeError, ValueError) as exc:                # a shape the model cannot run: say so, go on
            lines = [{"shape": name, "error": str(exc)[:300]}]
        for line in lines:
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
