#!/usr/bin/env python3
"""Cost of the box and scribble prompts (mivp_amd.strokes).

One process, device events, every call recorded in a HIP graph and warmed up at the shape it is timed at; ``--runs`` whole
measurements (default 3), the median and the min .. max over the runs are reported.

- ``encode`` / ``box`` / ``scribbles``: recorded ``encode_strokes`` (gaussian, filled boxes; 2 boxes and 4 strokes per sample),
  ``simulate_box`` and ``simulate_scribbles(max_iter=32)`` (uint8 prediction, float32 target, blocky random maps) at 96^3 B = 4,
  128 x 128 x 8 B = 14 and 512 x 512 x 96 B = 1, against
  * the time their bytes take at the 6.3 TB/s streaming rate DESIGN 4.8 uses -- encode: the mask read, the two squared fields
    written by the seed pass, read and written by each line pass and read by the closing pass, the two channels written (57
    bytes per voxel); box: the target read once; scribbles: the two maps read by the seed pass, the fields as above and read by
    the core pass, the stacked class map written, copied and committed (about 55 bytes per voxel), WITHOUT the thinning
    iterations, whose traffic depends on how many of the 32 run;
  * an eager composition of the same definitions -- encode: scipy's transform of the two bit planes on the CPU, box and
    value in torch; box: ``nonzero`` / ``min`` / ``max`` per sample in torch; scribbles: scipy's padded transform on the CPU,
    then ``skeleton.skeletonize`` per sample on the GPU (each timed once: they take up to seconds).  The eager results are
    compared with the recorded ones.
- ``step``: the recorded ``downstream`` step (train.GraphedStep) at the two training shapes, from the same job.

One JSON line per row, appended to ``--out`` (profiles/strokes_bench.jsonl).  No target is set here.  Nothing here is a kernel
trace: times are device-event windows around graph replays, so the launches of a call are not told apart."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_clicks import SCAN_SHAPE, STREAM_TBS, TRAIN_SHAPES, bench_step, blocky, recorded, spread, timed  # noqa: E402

SIGMA = 2.0
MAX_ITER = 32


def filled_slot(batch, dims, gen):
    import torch
    from mivp_amd import strokes as ST
    slot = ST.StrokeSlot(batch, dims, max_boxes=4)
    pick = lambda: [int(torch.randint(0, n, (1,), generator=gen)) for n in dims]      # noqa: E731
    for b in range(batch):
        rows = []
        for i in range(2):
            p, q = pick(), pick()
            rows.append((*[min(a, c) for a, c in zip(p, q)], *[max(a, c) for a, c in zip(p, q)], i))
        slot.set_boxes(b, rows)
        for i in range(4):
            slot.draw(b, [pick(), pick(), pick()], i % 2)
    return slot


def row(bench, name, calls, runs, ms, eager_ms, nbytes, **extra):
    bytes_ms = nbytes / (STREAM_TBS * 1e12) * 1e3
    return {"bench": bench, "shape": name, "calls": calls, "runs": runs, "ms": ms, "eager_ms_once": round(eager_ms, 2),
            "speedup": round(eager_ms / ms["median"], 1), "MB": round(nbytes / 1e6, 2), "bytes_at_6.3TBs_ms": round(bytes_ms, 4),
            "of_streaming_rate": round(bytes_ms / ms["median"], 3), **extra}


def bench_encode(name, batch, dims, runs, calls):
    import numpy as np
    import torch
    from scipy import ndimage
    from mivp_amd import strokes as ST
    slot = filled_slot(batch, dims, torch.Generator().manual_seed(1))
    out = torch.zeros((batch, 3, *dims), device="cuda")
    ws = ST.strokes_ws(batch, dims)
    replay = recorded(lambda: ST.encode_strokes(slot, out, channel_offset=1, kind="gaussian", sigma=SIGMA, workspace=ws))
    ms = spread([timed(replay, calls, 3) for _ in range(runs)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = slot.cpu()                                               # eager code reads the record back
    grid = torch.meshgrid(*[torch.arange(n, device="cuda") for n in dims], indexing="ij")
    eager = torch.zeros((batch, 2, *dims), device="cuda")
    for b in range(batch):
        for ch in range(2):
            seeds = (rec.mask[b] >> ch) & 1
            m = ndimage.distance_transform_edt(seeds == 0) ** 2 if seeds.any() else np.full(dims, np.inf)
            v = torch.exp(-torch.from_numpy(m).cuda().float() / (2 * SIGMA * SIGMA))
            for r in rec.boxes[b, :rec.box_count[b]]:
                if r[6] == ch:
                    inside = torch.ones(dims, dtype=torch.bool, device="cuda")
                    for a in range(3):
                        inside &= (grid[a] >= int(r[a])) & (grid[a] <= int(r[3 + a]))
                    v = torch.maximum(v, inside.float())
            eager[b, ch] = v
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t0) * 1e3
    vox = batch * dims[0] * dims[1] * dims[2]
    return row("encode", name, calls, runs, ms, eager_ms, vox * 57, launches=4,
               max_abs_diff_vs_eager=float((eager - out[:, 1:]).abs().max()))


def bench_box(name, batch, dims, runs, calls):
    import torch
    from mivp_amd import strokes as ST
    target = blocky(torch.Generator().manual_seed(2), batch, dims).cuda()
    slot = ST.StrokeSlot(batch, dims, max_boxes=4)

    def call():
        slot.box_count.zero_()
        ST.simulate_box(target, slot, margin=(2, 2, 2))

    replay = recorded(call)
    ms = spread([timed(replay, calls, 3) for _ in range(runs)])
    zero_ms = spread([timed(recorded(lambda: slot.box_count.zero_()), calls, 3) for _ in range(runs)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = []
    for b in range(batch):
        at = (target[b] > 0).nonzero()
        lo, hi = at.min(dim=0).values.tolist(), at.max(dim=0).values.tolist()          # (host reads: eager code)
        want.append([max(l - 2, 0) for l in lo] + [min(h + 2, n - 1) for h, n in zip(hi, dims)])
    eager_ms = (time.perf_counter() - t0) * 1e3
    vox = batch * dims[0] * dims[1] * dims[2]
    return row("box", name, calls, runs, ms, eager_ms, vox * 4, launches=2, count_reset_ms=zero_ms,
               same_box_as_eager=slot.cpu().last[:, :6].tolist() == want)


def bench_scribbles(name, batch, dims, runs, calls):
    import numpy as np
    import torch
    from scipy import ndimage
    from mivp_amd import skeleton as SK
    from mivp_amd import strokes as ST
    gen = torch.Generator().manual_seed(3)
    pred = blocky(gen, batch, dims).to(torch.uint8).cuda()
    target = blocky(gen, batch, dims).cuda()
    slot = ST.StrokeSlot(batch, dims)
    ws = ST.strokes_ws(batch, dims)

    def call():
        slot.clear_scribbles()
        ST.simulate_scribbles(pred, target, slot, max_iter=MAX_ITER, workspace=ws)

    replay = recorded(call)
    ms = spread([timed(replay, calls, 2) for _ in range(runs)])
    zero_ms = spread([timed(recorded(slot.clear_scribbles), calls, 2) for _ in range(runs)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p, t = pred.cpu().numpy() > 0, target.cpu().numpy() > 0
    eager = torch.zeros((batch, *dims), dtype=torch.uint8, device="cuda")
    for b in range(batch):
        core = np.zeros(dims, dtype=np.uint8)
        for cls, reg in ((1, t[b] & ~p[b]), (2, p[b] & ~t[b])):
            core[ndimage.distance_transform_edt(np.pad(reg, 1))[1:-1, 1:-1, 1:-1] ** 2 >= 2.25] = cls
        skel = SK.skeletonize(torch.from_numpy(core).cuda(), 3, max_iter=MAX_ITER).skeleton
        eager[b] = (skel == 1).to(torch.uint8) | ((skel == 2).to(torch.uint8) << 1)
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t0) * 1e3
    replay()
    rec = slot.cpu()
    vox = batch * dims[0] * dims[1] * dims[2]
    return row("scribbles", name, calls, runs, ms, eager_ms, vox * 55, max_iter=MAX_ITER, launches_at_most=6 + 9 * MAX_ITER,
               mask_reset_ms=zero_ms, converged=rec.last[:, 2].tolist(), scribble_voxels=rec.last[:, :2].sum(axis=0).tolist(),
               same_mask_as_eager=bool(np.array_equal(rec.mask, eager.cpu().numpy())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", choices=("encode", "box", "scribbles", "step"), default=None)
    ap.add_argument("--no-scan", action="store_true", help="leave out the 512 x 512 x 96 rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strokes_bench.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_strokes: no GPU (a timing without one says nothing; nothing is measured)")
    import mivp_amd  # noqa: F401
    shapes = list(TRAIN_SHAPES) + ([] if args.no_scan else [SCAN_SHAPE])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(r):
        print(json.dumps(r), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(r) + "\n")

    for name, batch, dims, window in shapes:
        small = dims[0] * dims[1] * dims[2] * batch < 2 ** 23
        calls = args.calls if small else 5
        if args.only in (None, "encode"):
            emit(bench_encode(name, batch, dims, args.runs, calls))
        if args.only in (None, "box"):
            emit(bench_box(name, batch, dims, args.runs, calls))
        if args.only in (None, "scribbles"):
            emit(bench_scribbles(name, batch, dims, args.runs, calls))
        if args.only in (None, "step") and window is not None:
            emit(bench_step(name, batch, dims, window, args.runs, args.calls))


if __name__ == "__main__":
    main()
