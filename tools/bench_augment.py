#!/usr/bin/env python3
"""Random intensity augmentation throughput (mivp_amd.augment), timed on device events after a warm-up, on the two shapes
the README reports the phase-1 step at: 1 x 96^3 at B = 4 and 1 x 128 x 128 x 8 at B = 14.  Cases per shape:

- ``all steps``: every sample runs the five steps (the worst case of a batch);
- ``expected mix``: draw sets at the reference's probability 0.05 per step, a new one loaded before every call (most
  samples are a plain copy; the time includes the non-blocking slot load);
- ``all off``: no step fires (the floor: the stats launch exits, the apply launch copies).

Next to each the same formulas composed from eager torch ops on the same GPU are timed (bias field materialised,
``std`` / ``amin`` / ``amax`` reductions, ``pow``, a searchsorted interpolation), for ``all steps`` and the mix.  One JSON
line per case: ms per call (both launches), the eager ms, their ratio, the algorithmic bytes (4 B read by the statistics of
the samples that need them, 4 B read + 4 B written by apply) and that over time as a fraction of the 6.3 TB/s HBM rate
DESIGN 4.8 uses, and the call as a share of the phase-1 step time the README gives for that shape.  The lines are appended
to profiles/augment_bench.jsonl (``--filters``: profiles/filters_bench.jsonl).

``--filters`` times the noise / blur / low-resolution chain (``augment_filters``) instead, RECORDED in a graph (one replay
= its three launches, out of place) on the same two shapes: every flag off, draw sets at ``prob = 0.1`` (a new one loaded
before every replay), every sample with each single flag, every sample with all three.  Each case is timed ``--repeats``
times (the median and the min .. max spread are reported) next to an eager torch composition of the same draws on the same
GPU (``randn``, three ``conv3d`` with 1-D kernels, two ``interpolate``; torch's own generator, so only the cost compares),
and given as a share of the phase-1 step.  At these sizes the batch sits in the Infinity Cache: no HBM rate is claimed."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 6.3e12
SHAPES = [((4, 1, 96, 96, 96), 21.7, "eager step"), ((14, 1, 128, 128, 8), 18.7, "graphed step")]   # README phase-1 ms
STATS = 2 | 4 | 16


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


def legendre(t):
    import torch
    return torch.stack([torch.ones_like(t), t, (3 * t ** 2 - 1) / 2, (5 * t ** 3 - 3 * t) / 2])


def eager_chain(x, d):
    """The chain of draws ``d`` from torch ops, sample by sample (the statistics are per sample)."""
    import torch
    out = torch.empty_like(x)
    for b in range(x.shape[0]):
        v, fl = x[b], int(d.flags[b])
        if fl & 1:
            ph, pw, pd = [legendre(torch.linspace(-1, 1, n, device=x.device)) for n in x.shape[2:]]
            c = torch.zeros(4, 4, 4, device=x.device)
            it = iter(d.coeffs[b].tolist())
            for i in range(4):
                for j in range(4 - i):
                    for k in range(4 - i - j):
                        c[i, j, k] = next(it)
            v = v * torch.exp(torch.einsum("ijk,ih,jw,kd->hwd", c, ph, pw, pd))[None]
        if fl & 2:
            v = v + float(d.shift[b]) * v.std(unbiased=False)
        if fl & 4:
            lo = v.amin()
            rng = v.amax() - lo
            v = ((v - lo) / (rng + 1e-7)) ** float(d.gamma[b]) * rng + lo
        if fl & 8:
            v = v * (1.0 + float(d.scale[b]))
        if fl & 16:
            lo, hi = v.amin(), v.amax()
            n = int(d.n_points[b])
            xp = torch.linspace(0, 1, n, device=x.device) * (hi - lo) + lo
            yp = torch.from_numpy(d.floating[b, :n].copy()).to(x.device) * (hi - lo) + lo
            j = (torch.searchsorted(xp, v.reshape(-1), right=True) - 1).clamp(0, n - 2)
            slope = (yp[1:] - yp[:-1]) / (xp[1:] - xp[:-1]).clamp_min(1e-30)
            v = (slope[j] * (v.reshape(-1) - xp[j]) + yp[j]).clamp(torch.minimum(yp[0], yp[-1]),
                                                                 torch.maximum(yp[0], yp[-1])).reshape(v.shape)
        out[b] = v
    return out


def eager_filters(x, d):
    """The filter chain of draws ``d`` from torch ops, sample by sample."""
    import torch
    import torch.nn.functional as F
    out = torch.empty_like(x)
    dims = tuple(x.shape[2:])
    for b in range(x.shape[0]):
        v, fl = x[b:b + 1], int(d.flags[b])
        C_ = v.shape[1]
        if fl & 1:
            v = v + float(d.noise_std[b]) * torch.randn_like(v) + float(d.noise_mean[b])
        if fl & 2:
            v = v.reshape(C_, 1, *dims)
            for a in (2, 1, 0):
                r = int(d.radius[b, a])
                if r == 0:
                    continue
                k = torch.from_numpy(d.taps[b, a, 8 - r:8 + r + 1].copy()).to(x.device)
                shape, pad = [1, 1, 1, 1, 1], [0, 0, 0]
                shape[2 + a], pad[a] = 2 * r + 1, r
                v = F.conv3d(v, k.view(shape), padding=pad)
            v = v.reshape(1, C_, *dims)
        if fl & 4:
            low = tuple(int(n) for n in d.low_size[b])
            v = F.interpolate(F.interpolate(v, size=low, mode="nearest"), size=dims, mode="trilinear", align_corners=False)
        out[b] = v[0]
    return out


def bench_filters(a):
    import numpy as np
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import augment as A
    dev = torch.device("cuda:0")
    lines = []
    for shape, step_ms, step_kind in SHAPES:
        B, dims = shape[0], shape[2:]
        x = torch.rand(shape, generator=torch.Generator().manual_seed(1)).to(dev)
        out = torch.empty_like(x)
        slot = A.FilterSlot(B, shape[1], dims, dev)

        def only(flags):
            d = A.draw_filters(np.random.RandomState(1), B, dims, prob=1.0)
            d.flags[:] = flags
            return d

        mix = [A.draw_filters(np.random.RandomState(100 + k), B, dims, prob=0.1) for k in range(a.mix_sets)]
        cases = [("all off", [only(0)]), ("expected mix (prob 0.1)", mix), ("noise on every sample", [only(1)]),
                 ("blur on every sample", [only(2)]), ("low-res on every sample", [only(4)]),
                 ("all three on every sample", [only(7)])]
        # blur and low-res agree with torch's before anything is timed (the noise streams differ by design)
        slot.load(only(6))
        got, want = A.augment_filters(x, slot), eager_filters(x, only(6))
        assert float((got - want).abs().max()) < 1e-4
        slot.load(only(0))
        A.augment_filters(x, slot, out=out)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            A.augment_filters(x, slot, out=out)
        for case, sets in cases:
            state = {"k": 0}

            def replay():
                if len(sets) > 1:
                    slot.load(sets[state["k"] % len(sets)])
                    state["k"] += 1
                graph.replay()

            def eager():
                d = sets[state["k"] % len(sets)]
                state["k"] += 1
                eager_filters(x, d)

            slot.load(sets[0])
            ms = sorted(timed(replay, a.calls, a.warmup) for _ in range(a.repeats))
            em = sorted(timed(eager, max(5, a.calls // 10) if len(sets) == 1 else a.calls, 2) for _ in range(a.repeats))
            med, emed = ms[len(ms) // 2], em[len(em) // 2]
            rec = {"shape": list(shape), "case": case, "recorded_ms": round(med, 4), "recorded_ms_min": round(ms[0], 4),
                   "recorded_ms_max": round(ms[-1], 4), "eager_torch_ms": round(emed, 4),
                   "eager_torch_ms_min": round(em[0], 4), "eager_torch_ms_max": round(em[-1], 4),
                   "eager_over_kernel": round(emed / med, 2), "phase1_step_ms": step_ms, "phase1_step": step_kind,
                   "share_of_step": round(med / step_ms, 4)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filters", action="store_true", help="time the noise / blur / low-res chain instead")
    ap.add_argument("--repeats", type=int, default=5, help="--filters: timings per case (median and spread)")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mix-sets", type=int, default=64)
    ap.add_argument("--out", default=None, help="default: profiles/augment_bench.jsonl, profiles/filters_bench.jsonl")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "filters_bench.jsonl" if a.filters else "augment_bench.jsonl")
    if a.filters:
        return bench_filters(a)
    import numpy as np
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import augment as A
    dev = torch.device("cuda:0")
    lines = []

    def report(shape, step_ms, step_kind, case, ms, eager_ms, nbytes):
        rec = {"shape": list(shape), "case": case, "ms": round(ms, 4),
               "eager_ms": None if eager_ms is None else round(eager_ms, 4),
               "eager_over_kernel": None if eager_ms is None else round(eager_ms / ms, 2), "bytes": int(nbytes),
               "hbm_fraction": round(nbytes / (ms * 1e-3) / HBM, 3), "phase1_step_ms": step_ms, "phase1_step": step_kind,
               "share_of_step": round(ms / step_ms, 4)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))

    def nbytes(x, sets):
        per = 4 * x[0].numel()
        return float(np.mean([per * (2 * s.batch + int(((s.flags & STATS) != 0).sum())) for s in sets]))

    for shape, step_ms, step_kind in SHAPES:
        B = shape[0]
        x = torch.rand(shape, generator=torch.Generator().manual_seed(1)).to(dev)
        out = torch.empty_like(x)
        slot = A.IntensitySlot(B, dev)
        full = A.draw_intensity(np.random.RandomState(1), B, prob=1.0)
        off = A.draw_intensity(np.random.RandomState(1), B, prob=0.0)
        mix = [A.draw_intensity(np.random.RandomState(100 + k), B) for k in range(a.mix_sets)]
        # the results agree before anything is timed (device exp / pow against torch's, a few 1e-6 of the range)
        slot.load(full)
        got, want = A.augment_intensity(x, slot), eager_chain(x, full)
        span = (want.amax(dim=(1, 2, 3, 4)) - want.amin(dim=(1, 2, 3, 4))).view(-1, 1, 1, 1, 1)
        assert float(((got - want).abs() / span).max()) < 1e-4

        ms = timed(lambda: A.augment_intensity(x, slot, out=out), a.calls, a.warmup)
        report(shape, step_ms, step_kind, "all steps", ms, timed(lambda: eager_chain(x, full), max(5, a.calls // 10), 2),
               nbytes(x, [full]))
        state = {"k": 0}

        def mixed():
            slot.load(mix[state["k"] % len(mix)])
            state["k"] += 1
            A.augment_intensity(x, slot, out=out)

        def mixed_eager():
            d = mix[state["k"] % len(mix)]
            state["k"] += 1
            eager_chain(x, d)

        ms = timed(mixed, a.calls, a.warmup)
        report(shape, step_ms, step_kind, "expected mix (prob 0.05)", ms, timed(mixed_eager, a.calls, a.warmup), nbytes(x, mix))
        slot.load(off)
        ms = timed(lambda: A.augment_intensity(x, slot, out=out), a.calls, a.warmup)
        report(shape, step_ms, step_kind, "all off", ms, None, nbytes(x, [off]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
