#!/usr/bin/env python3
"""Cost of the input volume's gradient and of a pixel-space prompt (prompting.InputPrompt).

One process, device events, every stage warmed up at the shape it is timed at; ``--runs`` whole measurements (default 3),
the median and the min .. max over the runs are reported, the variants of one comparison alternated within a run.

- ``step``: the recorded ``downstream`` step (train.GraphedStep) at 96^3, B = 4 (workload cfg1) and at the yml's roi
  128 x 128 x 8, B = 14 (window 8 x 8 x 4) -- the model alone against ``PromptedModel`` with an
  ``InputPrompt(lattice=(8, 8, 8))`` whose optimizer steps the prompt together with the ``downstream`` partition.  The
  difference is the prompt's two launches, the patch-embedding dgrad and one more tensor in the optimizer launch.
- ``dgrad``: ``mivp_patch_embed_dgrad`` alone at both shapes (C = 48, Cin = 1) against its compulsory bytes -- dz read once
  (bf16), dx written once (f32) -- at the 6.3 TB/s streaming rate DESIGN 4.8 uses.
- ``prompt``: the prompt's forward and its backward (dP from a given dx') against the eager composition
  ``x + scale * F.interpolate(P, size=roi, mode='trilinear', align_corners=True)`` and its autograd on the same GPU.

One JSON line per row, appended to ``--out`` (profiles/prompting_bench.jsonl).  No target is set here: the lines are what
DESIGN 4.42 and the README quote.  Nothing here is a kernel trace: times are device-event windows around the calls."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBS = 6.3
SHAPES = (("96^3 B4", 4, (96, 96, 96), [7, 7, 7]), ("128x128x8 B14", 14, (128, 128, 8), [8, 8, 4]))
LATTICE = (8, 8, 8)


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


def bench_step(name, batch, dims, window, runs, calls):
    import torch
    from mivp_amd import prompting as PR, train
    from mivp_amd.swin_unetr import SwinUnetR
    conf, _, _ = train.make_conf("cfg1", window=tuple(window))
    conf.roi_size = list(dims)
    g = torch.Generator().manual_seed(1)
    x = torch.rand((batch, conf.input_channels, *dims), generator=g).cuda()
    y = torch.randint(0, conf.output_channels_downstream, (batch, 1, *dims), generator=g).float().cuda()
    torch.manual_seed(5)
    plain = SwinUnetR(conf).cuda().train()
    o_plain = train.build_optimizer(plain, conf, capturable=True)
    s_plain = train.graphed_train_step(plain, o_plain, conf, x, y, warmup=2)
    torch.manual_seed(5)
    wrapped = PR.PromptedModel(SwinUnetR(conf).cuda().train(), PR.InputPrompt(conf.input_channels, dims, lattice=LATTICE).cuda())
    o_wrapped = PR.build_prompt_optimizer(wrapped, conf, include_downstream=True, capturable=True)
    s_wrapped = train.graphed_train_step(wrapped, o_wrapped, conf, x, y, warmup=2)
    t_plain, t_wrapped = [], []
    for _ in range(runs):
        t_plain.append(timed(s_plain, calls, 3))
        t_wrapped.append(timed(s_wrapped, calls, 3))
    a, b = spread(t_plain), spread(t_wrapped)
    return {"bench": "step", "shape": name, "lattice": list(LATTICE), "calls": calls, "runs": runs, "step_ms": a,
            "step_with_prompt_ms": b, "ratio": round(b["median"] / a["median"], 4),
            "added_ms": round(b["median"] - a["median"], 4)}


def bench_dgrad(name, batch, dims, runs, calls):
    import torch
    from mivp_amd import _lib as L, ops
    Cc, cin = 48, 1
    n_out = batch * (dims[0] // 2) * (dims[1] // 2) * (dims[2] // 2)
    d = L.EmbedDesc()
    d.B, d.Cin, d.C = batch, cin, Cc
    for a, v in enumerate(dims):
        d.dims[a] = v
    d.nblk = ops._nblk(n_out * (Cc // 8), Cc // 8, cap=2048)
    dz = torch.randn((n_out, Cc), device="cuda").to(torch.bfloat16)
    w = torch.randn((Cc, cin, 2, 2, 2), device="cuda")
    dx = torch.empty((batch, cin, *dims), device="cuda")

    def call():
        L.call("mivp_patch_embed_dgrad", C.byref(d), L.ptr(dz), L.ptr(w), L.ptr(dx), L.stream())

    ms = spread([timed(call, calls, 5) for _ in range(runs)])
    nbytes = dz.numel() * 2 + dx.numel() * 4
    bytes_ms = nbytes / (STREAM_TBS * 1e12) * 1e3
    return {"bench": "dgrad", "shape": name, "C": Cc, "Cin": cin, "calls": calls, "runs": runs, "ms": ms, "MB": round(nbytes / 1e6, 2),
            "bytes_at_6.3TBs_ms": round(bytes_ms, 4), "of_streaming_rate": round(bytes_ms / ms["median"], 3)}


def bench_prompt(name, batch, dims, runs, calls):
    import torch
    import torch.nn.functional as F
    from mivp_amd import prompting as PR
    cin = 1
    prompt = PR.InputPrompt(cin, dims, lattice=LATTICE, scale=0.5).cuda()
    with torch.no_grad():
        prompt.P.copy_(torch.randn_like(prompt.P))
    x = torch.rand((batch, cin, *dims), device="cuda")
    gout = torch.randn_like(x)
    Pe = prompt.P.detach().clone().requires_grad_(True)

    def eager_fwd():
        return x + 0.5 * F.interpolate(Pe[None], size=dims, mode="trilinear", align_corners=True)

    def hip_fwd():
        return prompt(x)

    y_e, y_h = eager_fwd(), hip_fwd()

    def eager_bwd():
        Pe.grad = None
        y_e.backward(gout, retain_graph=True)

    def hip_bwd():
        prompt.P.grad = None
        y_h.backward(gout, retain_graph=True)

    rows = {k: [] for k in ("fwd_ms", "eager_fwd_ms", "bwd_ms", "eager_bwd_ms")}
    for _ in range(runs):
        rows["fwd_ms"].append(timed(hip_fwd, calls, 5))
        rows["eager_fwd_ms"].append(timed(eager_fwd, calls, 5))
        rows["bwd_ms"].append(timed(hip_bwd, calls, 5))
        rows["eager_bwd_ms"].append(timed(eager_bwd, calls, 5))
    out = {k: spread(v) for k, v in rows.items()}
    fwd_bytes = 2 * x.numel() * 4
    out.update({"bench": "prompt", "shape": name, "lattice": list(LATTICE), "calls": calls, "runs": runs,
                "fwd_speedup": round(out["eager_fwd_ms"]["median"] / out["fwd_ms"]["median"], 2),
                "bwd_speedup": round(out["eager_bwd_ms"]["median"] / out["bwd_ms"]["median"], 2),
                "fwd_of_streaming_rate": round(fwd_bytes / (STREAM_TBS * 1e12) * 1e3 / out["fwd_ms"]["median"], 3),
                "max_abs_diff_fwd": float((y_e - y_h).abs().max())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--kernel-calls", type=int, default=200)
    ap.add_argument("--only", choices=("step", "dgrad", "prompt"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompting_bench.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_prompting: no GPU (a timing without one says nothing; nothing is measured)")
    import mivp_amd  # noqa: F401
    rows = []
    for name, batch, dims, window in SHAPES:
        if args.only in (None, "dgrad"):
            rows.append(bench_dgrad(name, batch, dims, args.runs, args.kernel_calls))
        if args.only in (None, "prompt"):
            rows.append(bench_prompt(name, batch, dims, args.runs, args.kernel_calls))
        if args.only in (None, "step"):
            rows.append(bench_step(name, batch, dims, window, args.runs, args.calls))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            print(json.dumps(r), flush=True)
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
