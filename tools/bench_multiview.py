#!/usr/bin/env python3
"""Phase-1 multi-view step throughput (mivp_amd.multiview): ms/step and volumes/s, eager and as one recorded graph, at the
``ssl_enc`` workload (1-ch 96^3, B = 4) and at the yml's shape (roi 128x128x8, B = batch_size_multi_view x
num_samples_multi_view = 14).  One JSON line per (shape, mode).

The new kernels' times come from a separate run under the kernel tracer:
    rocprofv3 --kernel-trace --stats -d OUT -o mv -- python tools/bench_multiview.py --steps 5 --warmup 2 --eager-only
then ``python tools/bench_multiview.py --stats OUT/.../mv_results.db`` (or a ``kernel_stats.csv``) prints the k_mv_* rows with bytes / time
against 6.3 TB/s (bytes: the compulsory traffic of each kernel at the ssl_enc shape, stated below)."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12


def shapes():
    return {"ssl_enc_96": dict(dims=(96, 96, 96), batch=4), "yml_128x128x8": dict(dims=(128, 128, 8), batch=14)}


def conf_for(name):
    from mivp_amd import train
    conf, _, _ = train.make_conf("ssl_enc")
    s = shapes()[name]
    conf.roi_size = list(s["dims"])
    return conf, s["dims"], s["batch"]


def run(name, steps, warmup, eager_only):
    import numpy as np
    import torch
    from mivp_amd import multiview as mv, train
    from mivp_amd.swin_unetr import SwinUnetR
    conf, dims, B = conf_for(name)
    if dims[2] != dims[0]:
        conf.attn_window_size = [8, 8, 4]                      # the yml's window for its 128x128x8 roi
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    x = torch.rand(B, conf.input_channels, *dims, device=dev)
    rs = np.random.RandomState(0)

    def nxt():
        return mv.draw_views(rs, B, dims, conf.masking_shape, conf.masking_ratio, conf.use_mutual_learning)

    draws = [nxt() for _ in range(steps + warmup + 4)]
    out = []
    for mode in (("eager",) if eager_only else ("eager", "graph")):
        model = SwinUnetR(conf).to(dev).train()
        opt = train.build_optimizer(model, conf, capturable=(mode == "graph"))
        sched = train.build_scheduler(opt, conf)
        if mode == "eager":
            slot = mv.make_slot(conf, x)
            for s in range(warmup):
                mv.multiview_step(model, opt, sched, conf, x, draws[s], slot=slot)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(steps):
                vec = mv.multiview_step(model, opt, sched, conf, x, draws[warmup + s], slot=slot)
            torch.cuda.synchronize()
        else:
            it = iter(draws)
            step = mv.graphed_multiview_step(model, opt, sched, conf, x, lambda: next(it), warmup=max(1, warmup))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                vec = step()
            torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / steps
        v = vec.cpu().tolist()
        out.append({"shape": name, "mode": mode, "batch": B, "dims": list(dims), "ms_per_step": round(ms, 3),
                    "volumes_per_s": round(B / ms * 1e3, 2),
                    "loss": {"rec": v[0], "rot": v[1], "con": v[2], "mut": v[3], "total": v[4]}})
        del model, opt
        torch.cuda.empty_cache()
    return out


def traffic(B=4, S=96, nw=3456):
    """Compulsory bytes per launch at the ssl_enc shape (fp32 volumes of B*S^3 elements, keep maps nw words each)."""
    v = 4 * B * S ** 3
    return {"k_mv_views": 3 * v + 8 * nw, "k_mv_rec_stats": 4 * v + 8 * nw, "k_mv_rec_grad": 6 * v + 8 * nw,
            "k_mv_heads": 4 * (4 * B * 512 + 4 * 2 * B * 4)}


def _stat_rows(path):
    """(name, calls, average ns, percent of kernel time) from a kernel_stats.csv or a results database (top_kernels)."""
    if path.endswith(".db"):
        import sqlite3
        for name, calls, _total, avg_us, pct in sqlite3.connect(path).execute("select * from top_kernels"):
            yield name, int(calls), 1e3 * float(avg_us), float(pct)
        return
    with open(path) as f:
        for row in csv.DictReader(f):
            yield (row.get("Name", ""), int(row.get("Calls", 0) or 0), float(row.get("AverageNs", 0) or 0),
                   float(row.get("Percentage", 0) or 0))


def stats(path):
    t = traffic()
    share = 0.0
    for name, calls, avg_ns, pct in _stat_rows(path):
        key = next((k for k in t if k in name), None)
        if key is None and "k_mv_" not in name:
            continue
        share += pct
        line = {"kernel": name.split("(")[0], "calls": calls, "avg_us": round(avg_ns / 1e3, 2), "share_pct": pct}
        if key is not None and avg_ns > 0:
            line["bytes"] = t[key]
            line["TB_per_s"] = round(t[key] / avg_ns / 1e3, 3)
            line["of_6.3TBps"] = round(t[key] / avg_ns * 1e9 / HBM, 3)
        print(json.dumps(line))
    print(json.dumps({"k_mv_share_of_kernel_time_pct": round(share, 3)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", choices=list(shapes()) + ["all"], default="all")
    ap.add_argument("--eager-only", action="store_true")
    ap.add_argument("--stats", help="results .db or kernel_stats.csv of a rocprofv3 --kernel-trace --stats run: print the k_mv_* rows")
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
        return
    import mivp_amd  # noqa: F401
    for name in (shapes() if a.shape == "all" else [a.shape]):
        try:
            lines = run(name, a.steps, a.warmup, a.eager_only)
        except (RuntimeError, ValueError) as exc:                # a shape the model cannot run: say so, go on
            lines = [{"shape": name, "error": str(exc)[:300]}]
        for line in lines:
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
