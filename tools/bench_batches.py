#!/usr/bin/env python3
"""Training-batch sampling throughput (mivp_amd.batches), timed on device events after a warm-up, from a bank of three
resident 512 x 512 x 96 volumes with label maps.  Cases, each with ``random_orientation`` off and on:

- ``downstream``: roi 96^3, B = 4, C = 1, image + mask (what ``train_step`` takes);
- ``students_teacher``: roi 96^3, B = 4, students 96^3 and 72^3, coordinates and student 0's mask;
- ``yml``: the yml's roi 128 x 128 x 8, B = 14, image + mask.

Per case one JSON line: ``ms`` = one ``fill`` issued from Python with the slot as it stands, ``load_ms`` = the same with a
new draw set checked and loaded before every call, ``graph_ms`` = the replay of ``fill`` recorded once (what a recorded
step pays), ``eager_ms`` = the same batch from eager torch ops on the same GPU (the crop sliced in the stored frame, then
``rot90``, ``F.pad`` and ``stack``, the label map by table indexing, the coordinates from per-crop ``meshgrid``s) after it
was checked to be bit-equal, and per launch group the compulsory bytes -- 4 B per channel and 1 B of label read for every
voxel inside the volume, 4 B written per output value -- over the event time of that group's calls issued back to back
from Python (``issue_TB_per_s``).  That figure is NOT a kernel rate and NOT an HBM rate: at ~10 us per call the loop can be
bound by the host's issue, and every call re-reads the same crops and rewrites the same outputs, which fit the Infinity
Cache.  Kernel times come from a kernel trace of one case at a time (``--only NAME:0|1`` under ``rocprofv3 --kernel-trace
--stats``: then every k_crop launch of a ``downstream`` / ``yml`` process is the same teacher launch).  ``share_of_step``
relates ``graph_ms`` to the step the batch feeds: the cfg1 step of DESIGN 6 for ``downstream``, the phase-1 steps of the
README for the other two (the students / teacher step has not been measured at these shapes).
The lines are appended to profiles/batches_bench.jsonl.

``--class-balanced`` measures the class-balanced sampling of DESIGN 4.27 instead (``ClassIndex``, class-mode ``fill``), the
whole measurement ``--runs`` times (2) in one process, every figure as the list of the runs plus their spread
((max - min) / min), appended to profiles/class_crops_bench.jsonl:

- ``index``: the build of the index of ONE 512 x 512 x 96 label map (3 classes; 1 % and 3 % of the voxels in the two
  foreground classes): ``launches_ms`` = the count and scan launches alone, issued back to back (the 25 MB label map stays
  in the Infinity Cache between calls), ``update_ms`` = ``ClassIndex.update()`` of a new index of that one volume, with its
  allocation, its blocking read of the totals and its table write;
- ``fill``: for the ``downstream`` and ``yml`` rows, ``fill`` recorded once and replayed, without an index (``plain_ms``,
  uniform origins) and with one (``class_ms``: pick, then the same teacher launch), the pick recorded alone
  (``pick_ms``), and ``pick_share_of_step`` = (class_ms - plain_ms) / the step the batch feeds;
- ``eager_ms``: the same centres from eager torch on the same GPU, per sample
  ``(lut[lab] == c).flatten().nonzero()[rank]`` (checked to give the voxels the device picked).
Random orientation is on in every class-balanced row.

``--spatial`` measures the random flip / rotation / zoom of DESIGN 4.28 (``BatchFiller(spatial=True)``), again ``--runs``
whole measurements with their spread, appended to profiles/spatial_crops_bench.jsonl.  For the ``downstream`` and
``students_teacher`` rows (random orientation off), every ``fill`` recorded once and replayed:

- ``plain_ms``: the filler without the option (the parent's path); ``identity_ms``: ``spatial=True`` with the identity;
  ``typical_ms``: flips with p = 0.5, +-0.26 rad about every axis, anisotropic zoom 0.8-1.25, sub-voxel shift;
  ``minified_ms``: zoom 0.2 (A = 5 I), whose boxes exceed the staged path's budget;
- ``teacher_direct_ms`` / ``teacher_staged_ms``: the teacher launch alone on the typical draws, every corner read from
  global memory (what ``fill`` issues) and with the LDS staging switched on through the debug entry (``staged_fraction``
  of its workgroups then staged) -- the comparison that decided the default;
- ``eager_ms``: image and mask of the same typical draws from eager torch on the same GPU, per sample ``affine_grid`` +
  ``grid_sample`` (bilinear, and nearest on the label map through the table), checked against the filler's image;
- ``share_of_step`` = (typical_ms - plain_ms) / the step the batch feeds.
The crops are re-read from the Infinity Cache on every replay: none of these is an HBM rate.

``--elastic`` measures the elastic deformation of DESIGN 4.29 (``BatchFiller(spatial=True, elastic=(7, 7, 7))``) on the
``downstream`` row (roi 96^3, B = 4), ``--runs`` whole measurements with their spread, appended to
profiles/elastic_crops_bench.jsonl.  Every ``fill`` is recorded once and replayed, on the typical spatial draws above:

- ``spatial_ms``: the ``spatial=True`` filler, the yardstick of the same run (``mivp_crop_fill_affine``);
- ``flags0_ms``: the elastic filler with no sample deformed (checked to give the spatial filler's bits): what the
  ``1 - p_elastic`` share of the samples costs; ``flags0_over_spatial`` is their ratio;
- ``flags1_ms``: every sample deformed, node displacements uniform in +-2 voxels, no locked border;
  ``share_of_step`` = (flags1_ms - spatial_ms) / the step the batch feeds, ``flags1_share_of_step`` = flags1_ms / that step;
- ``eager_ms``: a deformation of the same kind from eager torch on the same GPU, per sample: the lattice upsampled to a
  displacement volume (``F.interpolate``, trilinear -- not the B-spline: a cost comparison, its values are not compared),
  added to the output grid, the affine map applied, ``grid_sample`` (bilinear, and nearest on the label map).

``--corrupt`` measures the students' corruption of DESIGN 4.30 (``BatchFiller(..., corruption=True)``) on the recorded
students / teacher ``fill`` of two rows -- roi 96^3, B = 4, students 96^3 and 72^3; roi 128 x 128 x 8, B = 14, students
128 x 128 x 8 and 72 x 72 x 8 -- ``--runs`` whole measurements with their spread, appended to
profiles/corrupt_crops_bench.jsonl.  One recording per filler; the corrupting one is fed by its slot:

- ``plain_ms``: the filler without the option, the parent's path and the yardstick of the same run; it alternates with
- ``mode0_ms``: every record at mode 0 (checked to give the plain filler's bits): the two launches per student alone;
  ``mode0_over_plain`` is their ratio;
- ``dropout_ms`` / ``keep_ms`` / ``shuffle_ms``: every (student, sample) in mode 1 / 2 / 3 with the reference's hole
  parameters (``draw_student_corruption``'s defaults); ``mix_ms``: its default weights (0.7, 0.1, 0.1, 0.1), the mean
  over ``--draw-sets`` draw sets, each loaded and then replayed;
- ``eager_*_ms``: a corruption of the same kind from eager torch ops on the same GPU, per (student, sample): ``amin`` /
  ``amax``, ``torch.rand`` noise into the hole slices (dropout) or through a mask (keep), ``randperm`` indexing per hole
  (shuffle) -- a cost comparison with torch's own generators, its values are not compared;
- ``*_share_of_step``: (that time - plain_ms) over the step the batch feeds."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BANK_SHAPE = (512, 512, 96)
CASES = [("downstream", (96, 96, 96), 4, (), False, 2.41, "cfg1 step (DESIGN 6)"),
         ("students_teacher", (96, 96, 96), 4, ((96, 96, 96), (72, 72, 72)), True, 21.7, "phase-1 eager step (README)"),
         ("yml", (128, 128, 8), 14, (), False, 18.7, "phase-1 graphed step (README)")]
ACTIVE = [1, 2]


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


def eager_batch(images, labels, lut, d, roi, sizes, with_coord):
    """The batch of draws ``d`` from eager torch ops: per sample the stored-frame slice, rot90 of the crop, the pad."""
    import torch
    import torch.nn.functional as F
    from mivp_amd.batches import ROT_AXES, rotated_shape

    def pad(v, size):
        flat = []
        for k in (2, 1, 0):
            t = size[k] - v.shape[v.dim() - 3 + k]
            flat += [t // 2, t - t // 2]
        return F.pad(v, flat)

    img, mask, coord = [], [], []
    for b in range(d.batch):
        v, rot = int(d.volume[b]), int(d.rot[b])
        n = images[v].shape[1:]
        n_rot = rotated_shape(n, rot)
        lo = [int(a) for a in d.origin[b]]
        ext = [min(roi[k], n_rot[k]) for k in range(3)]
        if rot:                                                 # rotated box -> stored box: p_a = r_b, p_b = n_b - 1 - r_a
            a, c = ROT_AXES[rot]
            lo_s, ext_s = list(lo), list(ext)
            lo_s[a], ext_s[a] = lo[c], ext[c]
            lo_s[c], ext_s[c] = n[c] - lo[a] - ext[a], ext[a]
        else:
            lo_s, ext_s = lo, ext
        sl = tuple(slice(lo_s[k], lo_s[k] + ext_s[k]) for k in range(3))
        turn = (lambda t: torch.rot90(t, 1, (t.dim() - 3 + a, t.dim() - 3 + c))) if rot else (lambda t: t)
        img.append(pad(turn(images[v][(slice(None),) + sl]), roi))
        mask.append(pad(turn(lut[labels[v][sl].long()][None]), roi))
        if with_coord:
            axes = [torch.arange(lo_s[k], lo_s[k] + ext_s[k], dtype=torch.float32, device=lut.device) - (n[k] - 1) / 2.0
                    for k in range(3)]
            coord.append(pad(turn(torch.stack(torch.meshgrid(*axes, indexing="ij"), 0)), roi))
    out = dict(image=torch.stack(img), mask=torch.stack(mask))
    if with_coord:
        out["coord"] = torch.stack(coord)

    def view(t, s, size):
        rows = []
        for b in range(d.batch):
            o = [int(a) for a in d.student_origin[s, b]]
            e = [min(size[k], t.shape[2 + k]) for k in range(3)]
            rows.append(pad(t[b][:, o[0]:o[0] + e[0], o[1]:o[1] + e[1], o[2]:o[2] + e[2]], size))
        return torch.stack(rows)

    if sizes:
        out["image_st"] = [view(out["image"], s, size) for s, size in enumerate(sizes)]
        out["coord_st"] = [view(out["coord"], s, size) for s, size in enumerate(sizes)]
        out["mask_st_0"] = view(out["mask"], 0, sizes[0])
    return out


def spread(v):
    return round((max(v) - min(v)) / min(v), 4) if min(v) > 0 else None


def class_balanced(a):
    """``--class-balanced``: see the module docstring."""
    import numpy as np
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib as L, batches as BT
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    active, ncls, ratios = [0, 1, 2], 3, (1.0, 1.0, 1.0)
    bank = BT.VolumeBank(dev, 1)
    for _ in range(a.volumes):
        u = torch.rand(BANK_SHAPE, generator=g)
        bank.add(torch.rand((1,) + BANK_SHAPE, generator=g).to(dev), ((u < 0.04).to(torch.uint8) + (u < 0.01).to(torch.uint8)).to(dev))
    index = BT.ClassIndex(bank, ncls, active).update()
    numel = int(np.prod(BANK_SHAPE))
    assert index.counts.sum(axis=1).tolist() == [numel] * a.volumes
    one = BT.VolumeBank(dev, 1, capacity=1)
    one.add(bank.images[0], bank.labels[0])
    scratch = torch.empty_like(index.prefix[0])
    recs = {"index": {"shape": list(BANK_SHAPE), "num_classes": ncls, "chunks": scratch.shape[1] - 1,
                      "counts": index.counts[0].tolist(), "launches_ms": [], "update_ms": []}}
    rows = [c for c in CASES if c[0] in ("downstream", "yml")]
    for name, roi, B, _, _, step_ms, step_kind in rows:
        recs[name] = {"case": name, "roi": list(roi), "B": B, "random_orientation": True, "plain_ms": [], "class_ms": [],
                      "pick_ms": [], "eager_ms": [], "step_ms": step_ms, "step": step_kind}
    for run in range(a.runs):
        r = recs["index"]
        r["launches_ms"].append(round(timed(lambda: L.call("mivp_label_index_build", L.ptr(bank.labels[0]), numel,
                                                           L.ptr(index.lut), ncls, L.ptr(scratch), scratch.shape[1] - 1,
                                                           L.stream()), a.calls, a.warmup), 4))
        assert torch.equal(scratch, index.prefix[0])
        r["update_ms"].append(round(timed(lambda: BT.ClassIndex(one, ncls, active).update(), max(5, a.calls // 10), 2), 4))
        for name, roi, B, _, _, step_ms, _ in rows:
            r = recs[name]
            rs = np.random.RandomState(3 + run)
            ids = [i % len(bank) for i in range(B)]
            plain = BT.BatchFiller(bank, roi, B, active_labels=active)
            balanced = BT.BatchFiller(bank, roi, B, active_labels=active, class_index=index)
            plain.fill(BT.draw_crops(rs, bank.shapes, ids, roi, 1, True))
            d = BT.draw_class_crops(rs, index, ids, roi, 1, ratios, True)
            balanced.fill(d)
            lut = index.lut

            def eager_centres():
                return [(lut[bank.labels[int(v)].long()] == int(c)).flatten().nonzero()[int(k)]
                        for v, c, k in zip(d.volume, d.cls, d.rank)]

            # the device's origins are those of the eager centres, and an unclamped crop has its class at the centre
            q = torch.stack(eager_centres()).reshape(-1).cpu().numpy()
            r_c = rotated(d.rot, np.stack(np.unravel_index(q, BANK_SHAPE), axis=1), BT.ROT_AXES)
            n_rot = np.asarray([BT.rotated_shape(BANK_SHAPE, int(code)) for code in d.rot])
            free = r_c - np.asarray(roi) // 2
            want = np.minimum(np.maximum(free, 0), np.maximum(n_rot - np.asarray(roi), 0))
            assert np.array_equal(balanced.slot.resolved_origins(), want), f"{name}: the eager centres disagree"
            centre = balanced.mask[:, 0, roi[0] // 2, roi[1] // 2, roi[2] // 2].cpu().numpy()
            same = (want == free).all(axis=1)
            assert np.array_equal(centre[same], d.cls[same].astype(np.float32)), f"{name}: a crop is not on its class"
            torch.cuda.synchronize()
            graphs = []
            for fn in (plain.fill, balanced.fill, lambda: balanced.slot.resolve(roi)):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    fn()
                graphs.append(graph)
            for key, graph in zip(("plain_ms", "class_ms", "pick_ms"), graphs):
                r[key].append(round(timed(graph.replay, a.calls, a.warmup), 4))
            r["eager_ms"].append(round(timed(eager_centres, max(5, a.calls // 10), 2), 4))
    lines = []
    for key, r in recs.items():
        for k in [k for k, v in r.items() if k.endswith("_ms") and isinstance(v, list)]:
            r[k.replace("_ms", "_spread")] = spread(r[k])
        if key != "index":
            r["pick_share_of_step"] = [round((c - p) / r["step_ms"], 5) for c, p in zip(r["class_ms"], r["plain_ms"])]
            r["eager_over_pick"] = [round(e / k, 1) for e, k in zip(r["eager_ms"], r["pick_ms"])]
        else:
            r["case"] = "index"
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(a.class_out), exist_ok=True)
    with open(a.class_out, "a") as f:
        f.write("\n".join(lines) + "\n")


def spatial(a):
    """``--spatial``: see the module docstring."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib as L, batches as BT
    from mivp_amd._host import i3
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    bank = BT.VolumeBank(dev, 1)
    for _ in range(a.volumes):
        bank.add(torch.rand((1,) + BANK_SHAPE, generator=g).to(dev),
                 torch.randint(0, 4, BANK_SHAPE, generator=g, dtype=torch.uint8).to(dev))
    rows = [c for c in CASES if c[0] in ("downstream", "students_teacher")]
    keys = ("plain_ms", "identity_ms", "typical_ms", "minified_ms", "teacher_staged_ms", "teacher_direct_ms", "eager_ms")
    recs = {}
    for name, roi, B, sizes, with_coord, step_ms, step_kind in rows:
        recs[name] = {"case": name, "roi": list(roi), "B": B, "students": [list(x) for x in sizes], "brick": list(BT.SPATIAL_BRICK),
                      "box_cells": BT.SPATIAL_BOX_CELLS, **{k: [] for k in keys}, "staged_fraction": [],
                      "minified_staged_fraction": [], "step_ms": step_ms, "step": step_kind}
    typical = dict(p_flip=(0.5, 0.5, 0.5), p_affine=1.0, rotate_range=(0.26, 0.26, 0.26), scale_range=(0.8, 1.25),
                   isotropic=False, shift=True)
    for run in range(a.runs):
        for name, roi, B, sizes, with_coord, step_ms, _ in rows:
            r = recs[name]
            rs = np.random.RandomState(3 + run)
            ids = [i % len(bank) for i in range(B)]
            d = BT.draw_crops(rs, bank.shapes, ids, roi, 1, False, sizes)
            sp = BT.draw_spatial(rs, B, **typical)
            small = BT.draw_spatial(rs, B, p_affine=1.0, scale_range=(0.2, 0.2))
            plain = BT.BatchFiller(bank, roi, B, student_sizes=sizes, active_labels=ACTIVE, with_coord=with_coord)
            own = BT.BatchFiller(bank, roi, B, student_sizes=sizes, active_labels=ACTIVE, with_coord=with_coord, spatial=True)
            plain.fill(d)
            own.fill(d)
            torch.cuda.synchronize()
            assert torch.equal(plain.image, own.image) and torch.equal(plain.mask, own.mask), f"{name}: the identity differs"
            lut = own.lut.float()
            half = (np.asarray(roi) - 1) / 2.0

            def eager():
                img, mask = [], []
                for b in range(B):
                    vol = bank.images[int(d.volume[b])][None]
                    m = np.asarray(vol.shape[2:], np.float64)
                    A = sp.affine[b, :9].astype(np.float64).reshape(3, 3)
                    t = half + d.origin[b] + sp.affine[b, 9:]
                    th = np.zeros((3, 4))
                    th[:, :3] = (2.0 / (m - 1))[:, None] * A * half[None, :]
                    th[:, 3] = 2.0 * t / (m - 1) - 1.0
                    th = th[::-1, [2, 1, 0, 3]].copy()              # grid_sample counts x, y, z from the LAST axis
                    grid = F.affine_grid(torch.from_numpy(th).float().to(dev)[None], (1, 1) + tuple(roi), align_corners=True)
                    img.append(F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0])
                    lab = lut[bank.labels[int(d.volume[b])].long()][None, None]
                    mask.append(F.grid_sample(lab, grid, mode="nearest", padding_mode="zeros", align_corners=True)[0])
                return torch.stack(img), torch.stack(mask)

            own.fill(d, spatial=sp)
            e_img, _ = eager()
            torch.cuda.synchronize()
            # affine_grid works in normalised fp32 coordinates of a 512-voxel axis: the positions agree to ~1e-4 voxel
            assert float((e_img - own.image).abs().max()) < 5e-3, f"{name}: the eager composition disagrees"

            def teacher(stage, paths=None):
                L.call("mivp_crop_fill_affine_debug", L.ptr(bank.table), bank.capacity, bank.channels, L.ptr(own.slot.records),
                       own.slot.words, L.ptr(own.spatial_slot.words), B, i3(roi), L.ptr(own.lut), L.ptr(own.image),
                       L.ptr(own.mask), L.ptr(own.coord), stage, L.ptr(paths), L.stream())

            bricks = int(np.prod([-(-roi[k] // BT.SPATIAL_BRICK[k]) for k in range(3)]))
            paths = torch.zeros((B, bricks), dtype=torch.int32, device=dev)
            teacher(1, paths)
            r["staged_fraction"].append(round(float(paths.float().mean()), 4))

            def record(fn):
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    fn()
                return graph

            r["plain_ms"].append(round(timed(record(plain.fill).replay, a.calls, a.warmup), 4))
            graph = record(own.fill)                                # one recording, fed by the spatial slot
            for key, draws in (("identity_ms", BT.SpatialDraws.identity(B)), ("typical_ms", sp), ("minified_ms", small)):
                own.spatial_slot.load(draws)
                r[key].append(round(timed(graph.replay, a.calls, a.warmup), 4))
            teacher(1, paths)
            r["minified_staged_fraction"].append(round(float(paths.float().mean()), 4))
            own.spatial_slot.load(sp)
            r["teacher_staged_ms"].append(round(timed(record(lambda: teacher(1)).replay, a.calls, a.warmup), 4))
            r["teacher_direct_ms"].append(round(timed(record(lambda: teacher(0)).replay, a.calls, a.warmup), 4))
            r["eager_ms"].append(round(timed(eager, max(5, a.calls // 10), 2), 4))
    lines = []
    for r in recs.values():
        for k in keys:
            r[k.replace("_ms", "_spread")] = spread(r[k])
        r["share_of_step"] = [round((t - p) / r["step_ms"], 5) for t, p in zip(r["typical_ms"], r["plain_ms"])]
        r["eager_over_typical"] = [round(e / t, 1) for e, t in zip(r["eager_ms"], r["typical_ms"])]
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(a.spatial_out), exist_ok=True)
    with open(a.spatial_out, "a") as f:
        f.write("\n".join(lines) + "\n")


def elastic(a):
    """``--elastic``: see the module docstring."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    import mivp_amd  # noqa: F401
    from mivp_amd import batches as BT
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    bank = BT.VolumeBank(dev, 1)
    for _ in range(a.volumes):
        bank.add(torch.rand((1,) + BANK_SHAPE, generator=g).to(dev),
                 torch.randint(0, 4, BANK_SHAPE, generator=g, dtype=torch.uint8).to(dev))
    name, roi, B, sizes, with_coord, step_ms, step_kind = CASES[0]
    nodes = (7, 7, 7)
    keys = ("spatial_ms", "flags0_ms", "flags1_ms", "eager_ms")
    r = {"case": name, "roi": list(roi), "B": B, "nodes": list(nodes), "magnitude": 2.0, **{k: [] for k in keys},
         "step_ms": step_ms, "step": step_kind}
    typical = dict(p_flip=(0.5, 0.5, 0.5), p_affine=1.0, rotate_range=(0.26, 0.26, 0.26), scale_range=(0.8, 1.25),
                   isotropic=False, shift=True)
    for run in range(a.runs):
        rs = np.random.RandomState(3 + run)
        ids = [i % len(bank) for i in range(B)]
        d = BT.draw_crops(rs, bank.shapes, ids, roi, 1, False, sizes)
        sp = BT.draw_spatial(rs, B, **typical)
        ed = BT.draw_elastic(rs, B, roi, nodes=nodes, p_elastic=1.0, magnitude_range=(2.0, 2.0), locked_borders=0)
        ref = BT.BatchFiller(bank, roi, B, active_labels=ACTIVE, with_coord=with_coord, spatial=True)
        own = BT.BatchFiller(bank, roi, B, active_labels=ACTIVE, with_coord=with_coord, spatial=True, elastic=nodes)
        ref.fill(d, spatial=sp)
        own.fill(d, spatial=sp)
        torch.cuda.synchronize()
        assert torch.equal(ref.image, own.image) and torch.equal(ref.mask, own.mask), "flags 0: not the spatial filler's bits"
        own.fill(elastic=ed)
        torch.cuda.synchronize()
        moved = float((own.image != ref.image).float().mean())
        assert moved > 0.5 and bool(torch.isfinite(own.image).all()), f"flags 1: only {moved:.3f} of the voxels changed"
        lut = own.lut.float()
        half = (np.asarray(roi) - 1) / 2.0
        lat = torch.from_numpy(ed.lattice).to(dev)
        to_norm = torch.tensor([2.0 / (roi[k] - 1) for k in (2, 1, 0)], dtype=torch.float32, device=dev)
        eye = torch.eye(3, 4, device=dev)[None]

        def eager():
            img, mask = [], []
            for b in range(B):
                vol = bank.images[int(d.volume[b])][None]
                m = np.asarray(vol.shape[2:], np.float64)
                A = sp.affine[b, :9].astype(np.float64).reshape(3, 3)
                t = half + d.origin[b] + sp.affine[b, 9:]
                th = np.zeros((3, 4))
                th[:, :3] = (2.0 / (m - 1))[:, None] * A * half[None, :]
                th[:, 3] = 2.0 * t / (m - 1) - 1.0
                th = torch.from_numpy(th[::-1, [2, 1, 0, 3]].copy()).float().to(dev)    # x, y, z count from the LAST axis
                disp = F.interpolate(lat[b][None], size=roi, mode="trilinear", align_corners=False)     # voxels, [1, 3, h, w, d]
                base = F.affine_grid(eye, (1, 1) + tuple(roi), align_corners=True)                      # the output grid
                base = base + disp[0].permute(1, 2, 3, 0).flip(-1)[None] * to_norm
                grid = base @ th[:, :3].T + th[:, 3]
                img.append(F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0])
                lab = lut[bank.labels[int(d.volume[b])].long()][None, None]
                mask.append(F.grid_sample(lab, grid, mode="nearest", padding_mode="zeros", align_corners=True)[0])
            return torch.stack(img), torch.stack(mask)

        def record(fn):
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fn()
            return graph

        g_ref, g_own = record(ref.fill), record(own.fill)           # one recording each; the elastic one is fed by its slot
        for _ in range(2):                                          # the yardstick and flags 0 alternate
            r["spatial_ms"].append(round(timed(g_ref.replay, a.calls, a.warmup), 4))
            own.elastic_slot.load(BT.ElasticDraws.identity(B, nodes))
            r["flags0_ms"].append(round(timed(g_own.replay, a.calls, a.warmup), 4))
            own.elastic_slot.load(ed)
            r["flags1_ms"].append(round(timed(g_own.replay, a.calls, a.warmup), 4))
        r["eager_ms"].append(round(timed(eager, max(5, a.calls // 10), 2), 4))
    for k in keys:
        r[k.replace("_ms", "_spread")] = spread(r[k])
    r["flags0_over_spatial"] = [round(z / s, 4) for z, s in zip(r["flags0_ms"], r["spatial_ms"])]
    r["share_of_step"] = [round((e - s) / r["step_ms"], 5) for e, s in zip(r["flags1_ms"], r["spatial_ms"])]
    r["flags1_share_of_step"] = [round(e / r["step_ms"], 5) for e in r["flags1_ms"]]
    r["eager_over_flags1"] = [round(e / min(r["flags1_ms"]), 1) for e in r["eager_ms"]]
    print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.elastic_out), exist_ok=True)
    with open(a.elastic_out, "a") as f:
        f.write(json.dumps(r) + "\n")


CORRUPT_ROWS = [("students_teacher", (96, 96, 96), 4, ((96, 96, 96), (72, 72, 72)), 21.7, "phase-1 eager step (README)"),
                ("yml", (128, 128, 8), 14, ((128, 128, 8), (72, 72, 8)), 18.7, "phase-1 graphed step (README)")]


def corrupt(a):
    """``--corrupt``: see the module docstring."""
    import numpy as np
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import batches as BT
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    bank = BT.VolumeBank(dev, 1)
    for _ in range(a.volumes):
        bank.add(torch.rand((1,) + BANK_SHAPE, generator=g).to(dev),
                 torch.randint(0, 4, BANK_SHAPE, generator=g, dtype=torch.uint8).to(dev))
    pure = {"dropout": (0, 1, 0, 0), "keep": (0, 0, 1, 0), "shuffle": (0, 0, 0, 1)}
    keys = ["plain_ms", "mode0_ms"] + [f"{k}_ms" for k in pure] + ["mix_ms"] + [f"eager_{k}_ms" for k in list(pure) + ["mix"]]
    lines = []
    for name, roi, B, sizes, step_ms, step_kind in CORRUPT_ROWS:
        r = {"case": name, "roi": list(roi), "B": B, "students": [list(x) for x in sizes], **{k: [] for k in keys},
             "step_ms": step_ms, "step": step_kind}
        for run in range(a.runs):
            rs = np.random.RandomState(3 + run)
            ids = [i % len(bank) for i in range(B)]
            d = BT.draw_crops(rs, bank.shapes, ids, roi, 1, False, sizes)
            plain = BT.BatchFiller(bank, roi, B, student_sizes=sizes, active_labels=ACTIVE)
            own = BT.BatchFiller(bank, roi, B, student_sizes=sizes, active_labels=ACTIVE, corruption=True)
            plain.fill(d)
            own.fill(d)
            torch.cuda.synchronize()
            same = lambda: all(torch.equal(x, y) for x, y in zip(plain.image_st + plain.coord_st, own.image_st + own.coord_st))
            assert same(), f"{name}: mode 0 does not give the plain filler's bits"
            draws = {k: BT.draw_student_corruption(rs, B, sizes, weights=w) for k, w in pure.items()}
            mixes = [BT.draw_student_corruption(rs, B, sizes) for _ in range(a.draw_sets)]
            for k, cd in draws.items():
                own.fill(corruption=cd)
                torch.cuda.synchronize()
                changed = [float((x != y).float().mean()) for x, y in zip(plain.image_st, own.image_st)]
                assert min(changed) > 0 and bool(torch.isfinite(torch.stack([t.sum() for t in own.image_st])).all()), (k, changed)
                r.setdefault(f"{k}_changed", []).append([round(c, 4) for c in changed])

            def eager(cd):
                out = [t.clone() for t in plain.image_st]
                for s, x in enumerate(out):
                    for b in range(B):
                        mode, n = int(cd.mode[s, b]), int(cd.n_holes[s, b])
                        if mode == 0:
                            continue
                        boxes = [tuple(slice(int(o), int(o + e)) for o, e in zip(cd.origin[s, b, k], cd.size[s, b, k]))
                                 for k in range(n)]
                        if mode == 3:
                            for sl in boxes:
                                hole = x[b][(slice(None),) + sl]
                                flat = hole.reshape(hole.shape[0], -1)
                                x[b][(slice(None),) + sl] = flat[:, torch.randperm(flat.shape[1], device=dev)].reshape(hole.shape)
                            continue
                        lo, hi = x[b].amin(), x[b].amax()
                        if mode == 1:
                            for sl in boxes:
                                hole = x[b][(slice(None),) + sl]
                                x[b][(slice(None),) + sl] = lo + (hi - lo) * torch.rand(hole.shape, device=dev)
                        else:
                            inside = torch.zeros(x.shape[2:], dtype=torch.bool, device=dev)
                            for sl in boxes:
                                inside[sl] = True
                            x[b] = torch.where(inside, x[b], lo + (hi - lo) * torch.rand(x[b].shape, device=dev))
                return out

            def record(fn):
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    fn()
                return graph

            g_plain, g_own = record(plain.fill), record(own.fill)
            for _ in range(2):                                      # the yardstick and mode 0 alternate
                r["plain_ms"].append(round(timed(g_plain.replay, a.calls, a.warmup), 4))
                own.corruption_slot.load(BT.CorruptionDraws.identity(B, len(sizes)))
                r["mode0_ms"].append(round(timed(g_own.replay, a.calls, a.warmup), 4))
            assert same(), f"{name}: the recorded mode 0 does not give the plain filler's bits"
            for k, cd in draws.items():
                own.corruption_slot.load(cd)
                r[f"{k}_ms"].append(round(timed(g_own.replay, a.calls, a.warmup), 4))
            per_set = []
            for cd in mixes:                                        # loaded outside the timed replays
                own.corruption_slot.load(cd)
                per_set.append(timed(g_own.replay, max(20, a.calls // 8), a.warmup))
            r["mix_ms"].append(round(sum(per_set) / len(per_set), 4))
            for k, cd in list(draws.items()) + [("mix", mixes[0])]:
                r[f"eager_{k}_ms"].append(round(timed(lambda: eager(cd), max(5, a.calls // 20), 2), 4))
        for k in keys:
            r[k.replace("_ms", "_spread")] = spread(r[k])
        base = min(r["plain_ms"])
        r["mode0_over_plain"] = [round(z / p, 4) for z, p in zip(r["mode0_ms"], r["plain_ms"])]
        for k in ("mode0", "dropout", "keep", "shuffle", "mix"):
            r[f"{k}_share_of_step"] = [round((t - base) / step_ms, 5) for t in r[f"{k}_ms"]]
        print(json.dumps(r), flush=True)
        lines.append(json.dumps(r))
    os.makedirs(os.path.dirname(a.corrupt_out), exist_ok=True)
    with open(a.corrupt_out, "a") as f:
        f.write("\n".join(lines) + "\n")


def rotated(codes, p, rot_axes):
    """Stored voxels ``p`` [B, 3] in the frames rotated by ``codes``: for axes (a, b), r_b = p_a and r_a = n_b - 1 - p_b."""
    import numpy as np
    out = np.array(p, dtype=np.int64)
    for b, code in enumerate(codes):
        if int(code):
            x, y = rot_axes[int(code)]
            out[b, y], out[b, x] = p[b][x], BANK_SHAPE[y] - 1 - p[b][y]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--draw-sets", type=int, default=32)
    ap.add_argument("--volumes", type=int, default=3)
    ap.add_argument("--only", default=None, help="one case, as NAME:0 or NAME:1 (random_orientation off / on): for a "
                    "kernel-trace run, where every k_crop launch of the process should be the same launch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batches_bench.jsonl"))
    ap.add_argument("--class-balanced", action="store_true", help="measure the class-balanced sampling (DESIGN 4.27)")
    ap.add_argument("--runs", type=int, default=2,
                    help="--class-balanced, --spatial, --elastic, --corrupt: how often the whole measurement is made")
    ap.add_argument("--class-out", default=os.path.join(ROOT, "profiles", "class_crops_bench.jsonl"))
    ap.add_argument("--spatial", action="store_true", help="measure the random flip / rotation / zoom (DESIGN 4.28)")
    ap.add_argument("--spatial-out", default=os.path.join(ROOT, "profiles", "spatial_crops_bench.jsonl"))
    ap.add_argument("--elastic", action="store_true", help="measure the elastic deformation (DESIGN 4.29)")
    ap.add_argument("--elastic-out", default=os.path.join(ROOT, "profiles", "elastic_crops_bench.jsonl"))
    ap.add_argument("--corrupt", action="store_true", help="measure the students' corruption (DESIGN 4.30)")
    ap.add_argument("--corrupt-out", default=os.path.join(ROOT, "profiles", "corrupt_crops_bench.jsonl"))
    a = ap.parse_args()
    if a.corrupt:
        return corrupt(a)
    if a.elastic:
        return elastic(a)
    if a.class_balanced:
        return class_balanced(a)
    if a.spatial:
        return spatial(a)
    import numpy as np
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import batches as BT
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    bank = BT.VolumeBank(dev, 1)
    for _ in range(a.volumes):
        bank.add(torch.rand((1,) + BANK_SHAPE, generator=g).to(dev),
                 torch.randint(0, 4, BANK_SHAPE, generator=g, dtype=torch.uint8).to(dev))
    lines = []
    for name, roi, B, sizes, with_coord, step_ms, step_kind in CASES:
        for oriented in (False, True):
            if a.only is not None and a.only != f"{name}:{int(oriented)}":
                continue
            filler = BT.BatchFiller(bank, roi, B, student_sizes=sizes, active_labels=ACTIVE, with_coord=with_coord)
            lut = filler.lut.float()
            rs = np.random.RandomState(3)
            ids = [i % len(bank) for i in range(B)]
            sets = [BT.draw_crops(rs, bank.shapes, ids, roi, 1, oriented, sizes) for _ in range(a.draw_sets)]
            d = sets[0]
            got = filler.fill(d)
            want = eager_batch(bank.images, bank.labels, lut, d, roi, sizes, with_coord)
            torch.cuda.synchronize()
            pairs = [(filler.image, want["image"]), (filler.mask, want["mask"])]
            if with_coord:
                pairs.append((filler.coord, want["coord"]))
            if sizes:
                pairs += list(zip(got["image_st"], want["image_st"])) + list(zip(got["coord_st"], want["coord_st"]))
                pairs.append((got["mask_st_0"], want["mask_st_0"]))
            assert all(torch.equal(x, y) for x, y in pairs), f"{name}: the eager composition disagrees"

            slot = filler.slot
            ms = timed(lambda: filler.fill(), a.calls, a.warmup)
            state = {"k": 0}

            def loaded():
                state["k"] += 1
                filler.fill(sets[state["k"] % len(sets)])

            load_ms = timed(loaded, a.calls, a.warmup)
            slot.load(d, bank, roi, sizes)
            eager_ms = timed(lambda: eager_batch(bank.images, bank.labels, lut, d, roi, sizes, with_coord),
                             max(5, a.calls // 10), 2)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                filler.fill()
            graph_ms = timed(graph.replay, a.calls, a.warmup)
            # compulsory bytes per launch group
            vox = int(np.prod(roi))
            inside = sum(int(np.prod([min(roi[k], BT.rotated_shape(bank.shapes[int(v)], int(r))[k]) for k in range(3)]))
                         for v, r in zip(d.volume, d.rot))
            n_out = 1 + 1 + (3 if with_coord else 0)
            groups = [("teacher", 1, inside * (4 + 1) + B * vox * 4 * n_out, lambda: filler._fill_teacher(slot))]
            if sizes:
                sb = sum(int(np.prod([min(s[k], roi[k]) for k in range(3)])) * 4 + int(np.prod(s)) * 4 for s in sizes) * B * 4
                sb += (int(np.prod([min(sizes[0][k], roi[k]) for k in range(3)])) + int(np.prod(sizes[0]))) * 4 * B
                groups.append(("students", 2 * len(sizes) + 1, sb, lambda: filler._fill_students(slot)))
            launches = []
            for gname, n, nbytes, fn in groups:
                gms = timed(fn, a.calls, a.warmup)
                launches.append({"group": gname, "launches": n, "bytes": int(nbytes), "ms": round(gms, 4),
                                 "issue_TB_per_s": round(nbytes / (gms * 1e-3) / 1e12, 3)})
            rec = {"case": name, "roi": list(roi), "B": B, "students": [list(s) for s in sizes], "random_orientation": oriented,
                   "codes": sorted(set(int(r) for r in d.rot)), "ms": round(ms, 4), "load_ms": round(load_ms, 4),
                   "graph_ms": round(graph_ms, 4), "eager_ms": round(eager_ms, 4),
                   "eager_over_fill": round(eager_ms / ms, 2), "eager_over_graph": round(eager_ms / graph_ms, 2),
                   "groups": launches, "step_ms": step_ms, "step": step_kind, "share_of_step": round(graph_ms / step_ms, 4)}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    if not lines:
        raise SystemExit(f"--only {a.only}: no such case")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
