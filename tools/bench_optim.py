#!/usr/bin/env python3
"""Cost of the recorded optimizer stage with and without gradient-norm clipping (optim.FusedAdamW).

Two parameter sets: ``downstream`` (workload cfg3, both prompt sides: 142 978 parameters, 0.57 MB of gradients) and
``supervised_learning_all`` (workload sup_all: every parameter, 37.5 MB).  Each stage is what train.GraphedStep replays for the optimizer --
``advance()`` (the host side and its one-wave upload) and a replay of the graph that holds ``step()`` -- on fixed gradient
tensors, timed on device events over ``--calls`` replays after a warm-up.  Three stages, alternated within each of
``--runs`` runs of one process (the median and the min .. max over the runs are reported):

- ``plain``: FusedAdamW(capturable=True), one launch (the launch every earlier version of the optimizer records);
- ``clip``: FusedAdamW(capturable=True, max_grad_norm=1.0, skip_nonfinite=True), three launches, the gradients are over
  the threshold so the step clips;
- ``eager_clip_plain``: ``torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)`` on the same GPU, then the plain stage.

One JSON line per set.  No target is set here: the lines are what DESIGN 4.32 and the README quote."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = (("downstream", "cfg3"), ("supervised_learning_all", "sup_all"))


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


def recorded(opt):
    """One eager step on a side stream, then the step recorded: the stage GraphedStep replays."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()

    def stage():
        opt.advance()
        graph.replay()
    return stage


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    if a.runs < 2:
        ap.error("--runs: at least two, the spread between runs is part of the result")
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    dev = torch.device("cuda:0")
    lines = []
    for name, workload in SETS:
        conf, _, _ = train.make_conf(workload)
        model = SwinUnetR(conf).to(dev).train()
        plain = train.build_optimizer(model, conf, capturable=True)
        clip = train.build_optimizer(model, conf, capturable=True, max_grad_norm=1.0, skip_nonfinite=True)
        params = [p for g in plain.param_groups for p in g["params"]]
        gen = torch.Generator(device=dev).manual_seed(1)
        for p in params:                                          # fixed gradient tensors, norm far above 1
            p.grad = torch.randn(p.shape, generator=gen, device=dev)
        keep = [p.grad.clone() for p in params]

        def refill():
            torch._foreach_copy_([p.grad for p in params], keep)

        stage_plain, stage_clip = recorded(plain), recorded(clip)

        def stage_eager():
            torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
            stage_plain()

        stages = (("plain", stage_plain), ("clip", stage_clip), ("eager_clip_plain", stage_eager))
        ms = {k: [] for k, _ in stages}
        for _ in range(a.runs):
            for k, fn in stages:
                refill()
                ms[k].append(timed(fn, a.calls, a.warmup))
        st = clip.clip_stats()
        assert st["steps"] == st["clipped"] + st["skipped"] and st["skipped"] == 0, st      # every clip stage did clip
        rec = {"set": name, "tensors": len(params), "grad_MB": round(4e-6 * sum(p.numel() for p in params), 2),
               "runs": a.runs, "calls": a.calls}
        for k, v in ms.items():
            v = sorted(v)
            rec[k + "_us"] = {"median": round(1e3 * v[len(v) // 2], 2), "min": round(1e3 * v[0], 2), "max": round(1e3 * v[-1], 2)}
        med = {k: rec[k + "_us"]["median"] for k in ms}
        rec["clip_over_plain"] = round(med["clip"] / med["plain"], 3)
        rec["clip_minus_plain_us"] = round(med["clip"] - med["plain"], 2)
        rec["eager_over_clip"] = round(med["eager_clip_plain"] / med["clip"], 3)
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
