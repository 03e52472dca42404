#!/usr/bin/env python3
"""Scan histogram and data-driven window throughput (mivp_amd.scanstats), timed on device events after a warm-up, on a
one-channel int16 512 x 512 x 96 volume (the size DESIGN 4.15 predicts in 187 ms).  Five value fields:

- ``half_air``: half the voxels at -1024 in runs of 32 along D, the rest spread over 4096 consecutive values (a CT:
  air fills whole stretches of a row);
- ``half_air_scattered``: the same share of -1024, voxel by voxel at random (the worst case for run merging);
- ``spread``: every voxel spread over 4096 consecutive values;
- ``constant``: one value everywhere;
- ``full_range``: uniform over the whole int16 range (three quarters of the voxels fall outside the LDS window).

Each is timed with the default run merging and with one atomic per value (``FLAG_PER_VALUE``): the histogram alone, and
the chain histogram -> plan -> ``prepare_scan`` reading the plan from the device (identity geometry), next to the same
window composed from eager torch ops on the same GPU (``bincount`` of the shifted values, ``cumsum``, ``searchsorted``,
then the host-map ``prepare_scan``, which needs the two values on the host).  The eager histogram and order statistics are
compared with the kernels' before anything is timed.  One JSON line per case: ms per call, the eager ms and their ratio,
the bytes of the scan over the histogram's time as a fraction of the 6.3 TB/s HBM rate DESIGN 4.8 uses, and each as a
share of the 187 ms ``predict``.  The lines are appended to profiles/scanstats_bench.jsonl.

``--otsu`` times the Otsu foreground threshold on the ``half_air`` field instead, every figure as the median
of three timed runs with min .. max: the Otsu plan next to the window plan (both one workgroup per channel over the same
512 KB table), the mask kernel against its bytes (2 read, 1 written per voxel) at the 6.3 TB/s rate,
``prepare_scan(window=zscore(above=0, foreground="otsu"))`` next to ``prepare_scan(window=zscore(above=0))``, and an eager
torch composition of the threshold (float64 ``cumsum`` over the table, then ``argmax``) on the same GPU.  One JSON line."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
PREDICT_MS = 187.0
SHAPE = (512, 512, 96)
Q_LO, Q_HI = 0.005, 0.995


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


def field(name, dev, gen):
    import torch
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    if name == "constant":
        v = torch.full((n,), -1024, dtype=torch.int32, device=dev)
    elif name == "full_range":
        v = torch.randint(-32768, 32768, (n,), device=dev, generator=gen, dtype=torch.int32)
    else:
        v = torch.randint(-1000, 3096, (n,), device=dev, generator=gen, dtype=torch.int32)
        if name == "half_air":
            air = (torch.rand(n // 32, device=dev, generator=gen) < 0.5).repeat_interleave(32)
            v = torch.where(air, torch.full_like(v, -1024), v)
        elif name == "half_air_scattered":
            v = torch.where(torch.rand(n, device=dev, generator=gen) < 0.5, torch.full_like(v, -1024), v)
    return v.to(torch.int16).reshape((1,) + SHAPE)


def eager_histogram(raw):
    import torch
    return torch.bincount(raw.reshape(-1).long() + 32768, minlength=65536)


def eager_window(raw):
    """(a_lo, a_hi) on the HOST, through bincount / cumsum / searchsorted: the composition a user writes today."""
    import torch
    cum = torch.cumsum(eager_histogram(raw), 0)
    n = int(raw.numel())
    ks = torch.tensor([max(1, math.ceil(Q_LO * n)), max(1, math.ceil(Q_HI * n))], device=raw.device)
    return [int(b) - 32768 for b in torch.searchsorted(cum, ks).tolist()]


def eager_otsu(table):
    """Otsu's threshold of one channel's table with eager torch ops in float64 (a device scalar)."""
    import torch
    h = table.double()
    v = torch.arange(-32768, 32768, device=table.device, dtype=torch.float64)
    n0, a = torch.cumsum(h, 0), torch.cumsum(h * v, 0)
    n, s = n0[-1], a[-1]
    p, q = a * n - s * n0, n0 * (n - n0)
    score = torch.where((h > 0) & (q > 0), p * p / q.clamp(min=1.0), torch.full_like(p, -1.0))
    return torch.argmax(score) - 32768


def three(fn, calls, warmup):
    """(median, min, max) of three timed runs."""
    ms = sorted(timed(fn, calls, warmup) for _ in range(3))
    return [round(ms[1], 4), round(ms[0], 4), round(ms[2], 4)]


def otsu_main(a):
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import scan
    from mivp_amd import scanstats as S
    dev = torch.device("cuda:0")
    raw = field("half_air", dev, torch.Generator(device=dev).manual_seed(1))
    geom = scan.ScanGeometry.identity(SHAPE)
    out = torch.empty((1, 1) + SHAPE, dtype=torch.float32, device=dev)
    hist = S.scan_histogram(raw)
    rec_slot, mask = S.otsu_slot(hist), torch.empty(SHAPE, dtype=torch.uint8, device=dev)
    t, _, n_gt, valid = (int(x) for x in rec_slot.cpu()[0])
    assert valid and int(S.foreground_mask(raw, rec_slot, out=mask).sum()) == n_gt == int((raw > t).sum())
    t_eager = int(eager_otsu(hist.table[0]))
    spec = S.IntensityWindow.zscore()
    slot = S.WindowSlot(1, dev)
    plain, auto = S.IntensityWindow.zscore(above=0), S.IntensityWindow.zscore(above=0, foreground="otsu")
    otsu_ms = three(lambda: S.otsu_slot(hist, out=rec_slot), a.calls, a.warmup)
    plan_ms = three(lambda: S.window_slot(hist, spec, out=slot), a.calls, a.warmup)
    above_ms = three(lambda: S.window_slot_above(hist, spec, rec_slot, out=slot), a.calls, a.warmup)
    mask_ms = three(lambda: S.foreground_mask(raw, rec_slot, out=mask), a.calls, a.warmup)
    prep_plain_ms = three(lambda: scan.prepare_scan(raw, geom, window=plain, out=out), a.calls, a.warmup)
    prep_auto_ms = three(lambda: scan.prepare_scan(raw, geom, window=auto, out=out), a.calls, a.warmup)
    eager_ms = three(lambda: eager_otsu(hist.table[0]), a.calls, a.warmup)
    nbytes = 3 * raw.numel()
    rec = {"shape": list(SHAPE), "dtype": "int16", "field": "half_air", "case": "otsu", "threshold": t,
           "eager_threshold": t_eager, "median_min_max": True, "otsu_plan_ms": otsu_ms, "window_plan_ms": plan_ms,
           "window_plan_above_ms": above_ms, "otsu_over_window_plan": round(otsu_ms[0] / plan_ms[0], 2),
           "mask_ms": mask_ms, "mask_bytes": int(nbytes), "mask_hbm_fraction": round(nbytes / (mask_ms[0] * 1e-3) / HBM, 4),
           "prepare_zscore_above0_ms": prep_plain_ms, "prepare_zscore_above0_otsu_ms": prep_auto_ms,
           "prepare_otsu_minus_plain_ms": round(prep_auto_ms[0] - prep_plain_ms[0], 4), "eager_otsu_ms": eager_ms,
           "eager_over_otsu_plan": round(eager_ms[0] / otsu_ms[0], 2)}
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scanstats_bench.jsonl"))
    ap.add_argument("--otsu", action="store_true", help="time the Otsu threshold, mask and restricted window instead")
    a = ap.parse_args()
    if a.otsu:
        return otsu_main(a)
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import scan
    from mivp_amd import scanstats as S
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    geom = scan.ScanGeometry.identity(SHAPE)
    out = torch.empty((1, 1) + SHAPE, dtype=torch.float32, device=dev)
    spec = S.IntensityWindow.percentile(Q_LO, Q_HI)
    hist, slot = spec.buffers(1, dev)
    lines = []
    for name in ("half_air", "half_air_scattered", "spread", "constant", "full_range"):
        raw = field(name, dev, gen)
        nbytes = raw.numel() * raw.element_size()
        want = eager_histogram(raw)
        for flags in (0, S.FLAG_PER_VALUE):
            assert torch.equal(S.scan_histogram(raw, flags=flags).table[0], want)
        a_lo, a_hi = eager_window(raw)
        words = S.window_slot(S.scan_histogram(raw), spec).cpu()[0]
        assert (int(words[4]), int(words[5])) == (a_lo, a_hi), (words, a_lo, a_hi)
        few = max(3, a.calls // 10)
        eager_hist_ms = timed(lambda: eager_histogram(raw), few, 2)

        def eager_chain():
            lo, hi = eager_window(raw)
            scan.prepare_scan(raw, geom, a_min=float(lo), a_max=float(hi if hi > lo else lo + 1), out=out)

        eager_chain_ms = timed(eager_chain, few, 2)
        S.scan_histogram(raw, out=hist.zero_())                                   # the plan is timed on this field's table
        plan_ms = timed(lambda: S.window_slot(hist, spec, out=slot), a.calls, a.warmup)
        for case, flags in (("merge_runs", 0), ("per_value", S.FLAG_PER_VALUE)):
            hist_ms = timed(lambda: S.scan_histogram(raw, out=hist, flags=flags), a.calls, a.warmup)

            def chain():
                S.scan_histogram(raw, out=hist.zero_(), flags=flags)
                S.window_slot(hist, spec, out=slot)
                scan.prepare_scan(raw, geom, window=slot, out=out)

            chain_ms = timed(chain, a.calls, a.warmup)
            assert torch.equal(hist.table[0], want)
            rec = {"shape": list(SHAPE), "dtype": "int16", "field": name, "case": case, "hist_ms": round(hist_ms, 4),
                   "plan_ms": round(plan_ms, 4), "chain_ms": round(chain_ms, 4), "eager_hist_ms": round(eager_hist_ms, 4),
                   "eager_chain_ms": round(eager_chain_ms, 4), "eager_over_hist": round(eager_hist_ms / hist_ms, 2),
                   "eager_over_chain": round(eager_chain_ms / chain_ms, 2), "bytes": int(nbytes),
                   "hist_hbm_fraction": round(nbytes / (hist_ms * 1e-3) / HBM, 4), "predict_ms": PREDICT_MS,
                   "hist_share_of_predict": round(hist_ms / PREDICT_MS, 5),
                   "chain_share_of_predict": round(chain_ms / PREDICT_MS, 5)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
