#!/usr/bin/env python3
"""Cost of the geodesic distance guidance (mivp_amd.geodesic).

One process, device events, every timed call recorded in a HIP graph and warmed up at the shape it is timed at; ``--runs`` whole
measurements (default 3), the median and the min .. max over the runs are reported.  Shapes: 96^3 B = 4, 128 x 128 x 8 B = 14 and
512 x 512 x 96 B = 1; a synthetic image of bright blobs on noise, 8 clicks and 4 strokes per sample, gamma = 10.

- ``iterations``: the eager call's record (iterations that lowered a voxel) -- the ``n`` the recorded calls then issue blind.
- ``iteration``: (recorded begin + n iterations + end) minus (recorded begin + end), over n, against the bytes of an iteration
  at the 6.3 TB/s streaming rate DESIGN 4.8 uses: per voxel and field the brick of the field and of the image channel with
  their halo (2 x 4 x 18 x 18 x 34 / (16 x 16 x 32) bytes), the field again for the count and the store: 18.8 bytes, 37.5 per
  voxel of the batch.  An iteration is a relaxation to each brick's fixed point, not a streaming pass: the ratio says how far
  from one it is, no more.
- ``encode``: the whole recorded ``encode_geodesic(max_iter=n)`` against the recorded ``encode_strokes`` of the same slot, and
  against an eager torch min-plus Jacobi composition (26 shifted tensors per round, run to the same fixed point, then the
  gaussian), timed once; the two fields are compared.
- ``step``: the recorded ``downstream`` step (train.GraphedStep) at the two training shapes, from the same job.

One JSON line per row, appended to ``--out`` (profiles/geodesic_bench.jsonl).  No target is set here.  Nothing here is a kernel
trace: times are device-event windows around graph replays, so the launches of a call are not told apart."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_clicks import SCAN_SHAPE, STREAM_TBS, TRAIN_SHAPES, bench_step, filled_slot as click_slot, recorded, spread, timed  # noqa: E402
from bench_strokes import filled_slot as stroke_slot  # noqa: E402

SIGMA = 8.0
GAMMA = 10.0
BYTES_PER_FIELD_VOXEL = 2 * 4 * 18 * 18 * 34 / (16 * 16 * 32) + 8


def blob_image(gen, batch, dims):
    import torch
    grid = torch.meshgrid(*[torch.arange(n, dtype=torch.float32) for n in dims], indexing="ij")
    img = 0.05 * torch.rand((batch, 1, *dims), generator=gen)
    for b in range(batch):
        for _ in range(6):
            c = [float(torch.rand(1, generator=gen)) * n for n in dims]
            r = (0.08 + 0.12 * float(torch.rand(1, generator=gen))) * max(dims)
            img[b, 0][sum((g - a) ** 2 for g, a in zip(grid, c)) <= r * r] += 0.5
    return img


def eager_fields(image, seeds, gamma):
    """min-plus Jacobi in torch at unit spacing: 26 shifted tensors per round, to the fixed point -> ([B, 2, H, W, D], rounds)"""
    import torch
    import torch.nn.functional as F
    inf = float("inf")
    g = torch.stack([torch.where((seeds >> r) & 1 > 0, 0.0, inf) for r in range(2)], dim=1).float()
    offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    H, W, D = image.shape[2:]

    def shifted(t, o, fill):
        p = F.pad(t, (1, 1, 1, 1, 1, 1), value=fill)
        return p[..., 1 + o[0]:1 + o[0] + H, 1 + o[1]:1 + o[1] + W, 1 + o[2]:1 + o[2] + D]

    weights = [torch.sqrt(float(o[0] ** 2 + o[1] ** 2 + o[2] ** 2) + (gamma * (image - shifted(image, o, 0.0))) ** 2) for o in offs]
    rounds = 0
    while True:
        new = g
        for o, w in zip(offs, weights):
            new = torch.minimum(new, shifted(g, o, inf) + w)
        rounds += 1
        if torch.equal(new, g):                                    # (a host read per round: eager code)
            return g, rounds
        g = new


def bench_shape(name, batch, dims, runs, calls, eager):
    import torch
    from mivp_amd import geodesic as GD
    from mivp_amd import strokes as ST
    gen = torch.Generator().manual_seed(1)
    image = blob_image(gen, batch, dims).cuda()
    st, ck = stroke_slot(batch, dims, gen), click_slot(batch, dims, gen)
    st.set_boxes(0, [])
    for b in range(1, batch):
        st.set_boxes(b, [])                                        # seeds only: the boxes cost the same in both encodings
    out = torch.zeros((batch, 3, *dims), device="cuda")
    ws, sws = GD.geodesic_ws(batch, dims), ST.strokes_ws(batch, dims)
    seeds = GD.seed_mask(dims, strokes=st, clicks=ck)
    field = GD.geodesic_distance(image, seeds, gamma=GAMMA, workspace=ws)
    n, converged = [int(v) for v in field.info.tolist()]
    converged_field = field.field.clone()
    lay = GD._Layout(batch, dims)

    def chain(iters):
        GD.geodesic_distance(image, seeds, gamma=GAMMA, max_iter=iters, workspace=ws)

    full, bare = recorded(lambda: chain(n)), recorded(lambda: chain(0))
    full_ms = [timed(full, calls, 2) for _ in range(runs)]
    bare_ms = [timed(bare, calls, 2) for _ in range(runs)]
    per_iter = spread([(a - b) / max(n, 1) for a, b in zip(full_ms, bare_ms)])
    vox = batch * dims[0] * dims[1] * dims[2]
    bytes_ms = 2 * vox * BYTES_PER_FIELD_VOXEL / (STREAM_TBS * 1e12) * 1e3
    rows = [{"bench": "iteration", "shape": name, "calls": calls, "runs": runs, "iterations": n, "converged": converged,
             "bricks": 2 * batch * -(-dims[0] // 16) * -(-dims[1] // 16) * -(-dims[2] // 32), "field_ms": spread(full_ms),
             "ms_per_iteration": per_iter, "bytes_at_6.3TBs_ms": round(bytes_ms, 4),
             "of_streaming_rate": round(bytes_ms / max(per_iter["median"], 1e-9), 3)}]
    enc = recorded(lambda: GD.encode_geodesic(image, out, strokes=st, clicks=ck, channel_offset=1, gamma=GAMMA, spacing=(1, 1, 1),
                                              sigma=SIGMA, max_iter=n, workspace=ws))
    enc_ms = spread([timed(enc, calls, 2) for _ in range(runs)])
    same = bool(torch.equal(lay.field_of(ws, n).view(torch.int32), converged_field.view(torch.int32)))
    euclid = recorded(lambda: ST.encode_strokes(st, out, channel_offset=1, kind="gaussian", sigma=SIGMA, workspace=sws))
    euclid_ms = spread([timed(euclid, calls, 2) for _ in range(runs)])
    r = {"bench": "encode", "shape": name, "calls": calls, "runs": runs, "iterations": n, "ms": enc_ms, "encode_strokes_ms": euclid_ms,
         "times_encode_strokes": round(enc_ms["median"] / euclid_ms["median"], 1), "blind_field_equals_eager_field": same}
    if eager:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g, rounds = eager_fields(image, seeds, GAMMA)
        torch.exp(-(g * g) / (2 * SIGMA * SIGMA))
        torch.cuda.synchronize()
        eager_ms = (time.perf_counter() - t0) * 1e3
        ok = torch.isfinite(converged_field)
        rel = ((g - converged_field).abs()[ok] / converged_field[ok].clamp_min(1e-30)).max() if ok.any() else torch.zeros(())
        r.update(eager_ms_once=round(eager_ms, 1), eager_rounds=rounds, speedup=round(eager_ms / enc_ms["median"], 1),
                 max_rel_diff_vs_eager=float(rel))
    rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--no-scan", action="store_true", help="leave out the 512 x 512 x 96 rows")
    ap.add_argument("--no-eager", action="store_true", help="leave out the eager torch composition")
    ap.add_argument("--no-step", action="store_true", help="leave out the recorded training step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geodesic_bench.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_geodesic: no GPU (a timing without one says nothing; nothing is measured)")
    import mivp_amd  # noqa: F401
    shapes = list(TRAIN_SHAPES) + ([] if args.no_scan else [SCAN_SHAPE])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(r):
        print(json.dumps(r), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(r) + "\n")

    for name, batch, dims, window in shapes:
        small = dims[0] * dims[1] * dims[2] * batch < 2 ** 23
        rows = bench_shape(name, batch, dims, args.runs, args.calls if small else 3, not args.no_eager)
        step = None
        if window is not None and not args.no_step:
            step = bench_step(name, batch, dims, window, args.runs, args.calls)
            rows[1]["of_step"] = round(rows[1]["ms"]["median"] / step["step_ms"]["median"], 3)
        for r in rows + ([step] if step else []):
            emit(r)


if __name__ == "__main__":
    main()
