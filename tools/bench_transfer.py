#!/usr/bin/env python3
"""Intensity transfer tables (mivp_amd.transfer), timed on device events after a warm-up on a one-channel int16
512 x 512 x 96 volume (the size DESIGN 4.15 predicts in 187 ms).  Every figure is the median of three timed runs with
min .. max, all in one job:

- each plan kernel alone on the ``half_air`` field's table (equalise, match, landmarks record, landmarks table);
- the apply kernel in both read paths (the LDS window and the global gather) with the table cache-resident, on the typical
  4096-value ``half_air`` field and on ``full_range`` (uniform over int16: three quarters of the voxels fall outside the
  LDS window), against its bytes (2 read, 4 written per voxel) at the 6.3 TB/s streaming rate DESIGN 4.8 uses;
- the whole ``prepare_scan(window=spec)`` chain per mode next to ``prepare_scan(window=IntensityWindow.percentile())``
  (identity geometry), each as a share of the 187 ms ``predict``;
- an eager torch composition of the same maps on the same GPU (``bincount`` / ``cumsum`` / ``searchsorted`` / gather).

The eager tables are compared with the kernels' before anything is timed (equalise and the match integers exactly).  One
JSON line, appended to profiles/transfer_bench.jsonl."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM = 6.3e12
PREDICT_MS = 187.0


def eager_equalize(raw):
    """The equalised volume with eager torch ops: the table in float64 from bincount / cumsum, then a gather."""
    import torch
    h = torch.bincount(raw.reshape(-1).long() + 32768, minlength=65536)
    cum = torch.cumsum(h, 0)
    c0 = h[torch.nonzero(h)[0, 0]]
    table = ((cum - c0).clamp(min=0).double() / (cum[-1] - c0).double()).float()
    return table, table[raw.long() + 32768]


def eager_match(raw, ref_cum):
    """The match integers with eager torch ops in float64 (exact below 2^53): searchsorted of C_src N_ref in C_ref N_src."""
    import torch
    h = torch.bincount(raw.reshape(-1).long() + 32768, minlength=65536)
    cum = torch.cumsum(h, 0)
    u = torch.searchsorted((ref_cum * cum[-1]).double(), (cum.clamp(min=1) * ref_cum[-1]).double())
    table = (u - 32768).float()
    return table, table[raw.long() + 32768]


def main():
    from bench_scanstats import SHAPE, field, three
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transfer_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import scan
    from mivp_amd import scanstats as S
    from mivp_amd import transfer as T
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    raw, wide = field("half_air", dev, gen), field("full_range", dev, gen)
    other = field("spread", dev, gen)
    geom = scan.ScanGeometry.identity(SHAPE)
    out = torch.empty((1, 1) + SHAPE, dtype=torch.float32, device=dev)
    flat = torch.empty((1,) + SHAPE, dtype=torch.float32, device=dev)
    hist, ref_hist = S.scan_histogram(raw), S.scan_histogram(other)
    window = S.IntensityWindow.percentile()
    ref_slot = S.window_slot(ref_hist, window)
    ident = S.WindowSlot(1, dev)
    ident.words[:, :4] = torch.tensor([1.0, 0.0, -3e38, 3e38], device=dev)
    bank = T.LandmarkBank(1, device=dev)
    for r in (raw, other):
        bank.add_scan(r)
    tab, lm = T.TransferTable(1, dev), T.LandmarkSlot(1, dev)
    # the eager compositions agree with the kernels
    e_tab, e_vol = eager_equalize(raw)
    assert torch.equal(T.equalize_table(hist).table[0], e_tab)
    assert torch.equal(T.apply_table(raw, T.equalize_table(hist))[0], e_vol[0])
    ref_cum = torch.cumsum(ref_hist.table[0], 0)
    m_tab, _ = eager_match(raw, ref_cum)
    assert torch.equal(T.match_table(hist, ref_hist, ident, clip=False).table[0], m_tab)

    t3 = lambda fn: three(fn, a.calls, a.warmup)                  # noqa: E731
    rec = {"shape": list(SHAPE), "dtype": "int16", "field": "half_air", "case": "transfer", "median_min_max": True}
    rec["equalize_plan_ms"] = t3(lambda: T.equalize_table(hist, out=tab))
    rec["match_plan_ms"] = t3(lambda: T.match_table(hist, ref_hist, ref_slot, out=tab))
    rec["landmarks_record_ms"] = t3(lambda: T.scan_landmarks(hist, out=lm))
    rec["landmarks_plan_ms"] = t3(lambda: T.landmark_table(lm, bank, out=tab))
    rec["window_plan_ms"] = t3(lambda: S.window_slot(hist, window, out=ref_slot))
    nbytes = raw.numel() * 6
    floor_ms = nbytes / HBM * 1e3
    rec["apply_bytes"], rec["apply_floor_ms"] = int(nbytes), round(floor_ms, 4)
    for name, vol in (("half_air", raw), ("full_range", wide)):
        T.equalize_table(S.scan_histogram(vol), out=tab)
        for path, flags in (("window", 0), ("global", T.FLAG_GLOBAL)):
            ms = t3(lambda: T.apply_table(vol, tab, out=flat, flags=flags))
            rec[f"apply_{name}_{path}_ms"] = ms
            rec[f"apply_{name}_{path}_over_floor"] = round(ms[0] / floor_ms, 2)
        rec[f"apply_{name}_global_over_window"] = round(rec[f"apply_{name}_global_ms"][0] / rec[f"apply_{name}_window_ms"][0], 3)
    specs = {"equalize": T.IntensityTransfer.equalize(), "match": T.IntensityTransfer.match(ref_hist, window),
             "landmarks": T.IntensityTransfer.landmarks(bank)}
    rec["prepare_percentile_ms"] = t3(lambda: scan.prepare_scan(raw, geom, window=window, out=out))
    for name, spec in specs.items():
        ms = t3(lambda: scan.prepare_scan(raw, geom, window=spec, out=out))
        rec[f"prepare_{name}_ms"] = ms
        rec[f"prepare_{name}_share_of_predict"] = round(ms[0] / PREDICT_MS, 5)
        rec[f"prepare_{name}_over_percentile"] = round(ms[0] / rec["prepare_percentile_ms"][0], 2)
    few = max(3, a.calls // 10)
    rec["eager_equalize_ms"] = three(lambda: eager_equalize(raw), few, 2)
    rec["eager_match_ms"] = three(lambda: eager_match(raw, ref_cum), few, 2)
    rec["eager_equalize_over_chain"] = round(rec["eager_equalize_ms"][0] / rec["prepare_equalize_ms"][0], 2)
    rec["eager_match_over_chain"] = round(rec["eager_match_ms"][0] / rec["prepare_match_ms"][0], 2)
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
