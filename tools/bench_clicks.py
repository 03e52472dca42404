#!/usr/bin/env python3
"""Cost of the click encoding and of the click simulation (mivp_amd.clicks).

One process, device events, every call recorded in a HIP graph and warmed up at the shape it is timed at; ``--runs`` whole
measurements (default 3), the median and the min .. max over the runs are reported.

- ``encode`` / ``simulate``: recorded ``encode_clicks`` (gaussian) and ``simulate_clicks`` (uint8 prediction, float32 target,
  blocky random maps) at 96^3 B = 4 and 128 x 128 x 8 B = 14 with 8 clicks per sample, and at 512 x 512 x 96 B = 1, against
  * the time their bytes take at the 6.3 TB/s streaming rate DESIGN 4.8 uses -- encode: the two channels written once;
    simulate: the two maps read twice (the seed pass re-reads nothing else), the two squared fields written by the seed
    pass, read and written by each line pass and read by the pick (48 bytes per voxel);
  * an eager composition -- encode: ``torch.cdist`` / ``min`` / ``exp`` on the same GPU; simulate: scipy's transform of the
    padded masks plus ``argmax`` on the CPU, per sample and region (timed once: it takes seconds).
- ``step``: the recorded ``downstream`` step (train.GraphedStep) at the two training shapes, from the same job, so the rows
  above can be read as a share of it.

One JSON line per row, appended to ``--out`` (profiles/clicks_bench.jsonl).  No target is set here.  Nothing here is a kernel
trace: times are device-event windows around graph replays, so the five launches of the simulation are not told apart."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBS = 6.3
TRAIN_SHAPES = (("96^3 B4", 4, (96, 96, 96), [7, 7, 7]), ("128x128x8 B14", 14, (128, 128, 8), [8, 8, 4]))
SCAN_SHAPE = ("512x512x96 B1", 1, (512, 512, 96), None)
CLICKS = 8
SIGMA = 2.0


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


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def recorded(fn):
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def blocky(gen, batch, dims, cell=8):
    import torch
    coarse = torch.randint(0, 2, (batch, 1, *[-(-n // cell) for n in dims]), generator=gen).float()
    return torch.nn.functional.interpolate(coarse, size=dims, mode="nearest")[:, 0]


def filled_slot(batch, dims, gen):
    import torch
    from mivp_amd import clicks as CK
    slot = CK.ClickSlot(batch, max_clicks=32, dims=dims)
    for b in range(batch):
        rows = [(*[int(torch.randint(0, n, (1,), generator=gen)) for n in dims], i % 2) for i in range(CLICKS)]
        slot.set(b, rows)
    return slot


def bench_encode(name, batch, dims, runs, calls):
    import torch
    from mivp_amd import clicks as CK
    gen = torch.Generator().manual_seed(1)
    slot = filled_slot(batch, dims, gen)
    out = torch.zeros((batch, 3, *dims), device="cuda")
    replay = recorded(lambda: CK.encode_clicks(slot, out, channel_offset=1, sigma=SIGMA))
    grid = torch.stack(torch.meshgrid(*[torch.arange(n, device="cuda", dtype=torch.float32) for n in dims], indexing="ij"),
                       dim=-1).reshape(-1, 3)
    pts = slot.clicks[:, :CLICKS].float()
    eager_out = torch.zeros_like(out)

    def eager():
        for b in range(batch):
            for ch in range(2):
                p = pts[b][pts[b][:, 3] == ch][:, :3]                  # (a host read per sample and channel: eager code)
                m = torch.cdist(grid, p).min(dim=1).values
                eager_out[b, 1 + ch] = torch.exp(-(m * m) / (2 * SIGMA * SIGMA)).view(dims)

    eager()
    diff = float((eager_out - out).abs().max())
    ms = spread([timed(replay, calls, 5) for _ in range(runs)])
    ems = spread([timed(eager, max(calls // 20, 2), 1) for _ in range(runs)])
    nbytes = batch * 2 * dims[0] * dims[1] * dims[2] * 4
    bytes_ms = nbytes / (STREAM_TBS * 1e12) * 1e3
    return {"bench": "encode", "shape": name, "clicks": CLICKS, "calls": calls, "runs": runs, "ms": ms, "eager_ms": ems,
            "speedup": round(ems["median"] / ms["median"], 1), "MB": round(nbytes / 1e6, 2),
            "bytes_at_6.3TBs_ms": round(bytes_ms, 4), "of_streaming_rate": round(bytes_ms / ms["median"], 3),
            "max_abs_diff_vs_eager": diff}


def bench_simulate(name, batch, dims, runs, calls):
    import numpy as np
    import torch
    from scipy import ndimage
    from mivp_amd import clicks as CK
    gen = torch.Generator().manual_seed(2)
    pred = blocky(gen, batch, dims).to(torch.uint8).cuda()
    target = blocky(gen, batch, dims).cuda()
    slot = CK.ClickSlot(batch, max_clicks=32, dims=dims)
    ws = CK.simulate_clicks_ws(batch, dims)

    def call():
        slot.count.zero_()
        CK.simulate_clicks(pred, target, slot, workspace=ws)

    replay = recorded(call)
    ms = spread([timed(replay, calls, 3) for _ in range(runs)])
    zero_ms = spread([timed(recorded(lambda: slot.count.zero_()), calls, 3) for _ in range(runs)])
    p, t = pred.cpu().numpy() > 0, target.cpu().numpy() > 0
    t0 = time.perf_counter()
    picks = []
    for b in range(batch):
        best = (0.0, -1, -1)
        for ch, reg in ((0, t[b] & ~p[b]), (1, p[b] & ~t[b])):
            d = ndimage.distance_transform_edt(np.pad(reg, 1))[1:-1, 1:-1, 1:-1]
            i = int(d.argmax())
            if d.reshape(-1)[i] > best[0]:
                best = (float(d.reshape(-1)[i]), ch, i)
        picks.append(best)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    replay()
    last = slot.cpu().last
    agree = all(int(last[b, 2]) == picks[b][2] and int(last[b, 1]) == picks[b][1] for b in range(batch))
    vox = batch * dims[0] * dims[1] * dims[2]
    nbytes = vox * (48 + 2 * (1 + 4))
    bytes_ms = nbytes / (STREAM_TBS * 1e12) * 1e3
    return {"bench": "simulate", "shape": name, "calls": calls, "runs": runs, "ms": ms, "count_reset_ms": zero_ms,
            "scipy_cpu_ms_once": round(cpu_ms, 1), "speedup": round(cpu_ms / ms["median"], 1), "MB": round(nbytes / 1e6, 2),
            "bytes_at_6.3TBs_ms": round(bytes_ms, 4), "of_streaming_rate": round(bytes_ms / ms["median"], 3),
            "same_click_as_scipy": agree}


def bench_step(name, batch, dims, window, runs, calls):
    import torch
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    conf, _, _ = train.make_conf("cfg1", window=tuple(window))
    conf.roi_size = list(dims)
    g = torch.Generator().manual_seed(1)
    x = torch.rand((batch, conf.input_channels, *dims), generator=g).cuda()
    y = torch.randint(0, conf.output_channels_downstream, (batch, 1, *dims), generator=g).float().cuda()
    torch.manual_seed(5)
    model = SwinUnetR(conf).cuda().train()
    opt = train.build_optimizer(model, conf, capturable=True)
    step = train.graphed_train_step(model, opt, conf, x, y, warmup=2)
    return {"bench": "step", "shape": name, "calls": calls, "runs": runs, "step_ms": spread([timed(step, calls, 3) for _ in range(runs)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernel-calls", type=int, default=100)
    ap.add_argument("--only", choices=("encode", "simulate", "step"), default=None)
    ap.add_argument("--no-scan", action="store_true", help="leave out the 512 x 512 x 96 rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clicks_bench.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_clicks: no GPU (a timing without one says nothing; nothing is measured)")
    import mivp_amd  # noqa: F401
    shapes = list(TRAIN_SHAPES) + ([] if args.no_scan else [SCAN_SHAPE])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(row):
        print(json.dumps(row), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")

    for name, batch, dims, window in shapes:
        small = dims[0] * dims[1] * dims[2] * batch < 2 ** 23
        if args.only in (None, "encode"):
            emit(bench_encode(name, batch, dims, args.runs, args.kernel_calls if small else args.calls))
        if args.only in (None, "simulate"):
            emit(bench_simulate(name, batch, dims, args.runs, args.calls if small else 5))
        if args.only in (None, "step") and window is not None:
            emit(bench_step(name, batch, dims, window, args.runs, args.calls))


if __name__ == "__main__":
    main()
