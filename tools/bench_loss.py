"""Time the recorded loss + gradient of mivp_seg_loss (csrc/segloss.hip) against the Dice-focal kernels and eager torch.

    python tools/bench_loss.py [--runs 5] [--replays 50] [--warmup 10] [--boundary | --cldice | --hausdorff | --lovasz |
                                --multilabel]

Shapes: 96^3 at B = 4 (the `downstream` step's) and 128 x 128 x 8 at B = 14, both C = 2.  Settings of the new entry:
  (a) Dice-equivalent options (alpha = beta = 0.5), lambda_voxel = 0
  (b) Dice + weighted cross-entropy, an ignore label on 20 % of the voxels
  (c) Tversky (0.3, 0.7) + focal cross-entropy with gamma = 2, same weights and ignore label
  (d) top-k: Dice + weighted cross-entropy over the hardest 10 % of the valid voxels (mivp_seg_topk, csrc/segtopk.hip), the
      operands of (b); its yardsticks are (b) and the eager composition ``cross_entropy(reduction="none")`` + ``topk``
Baselines in the same job: mivp_dice_focal on the same operands with gamma = 4 and with the Dice term alone (gamma < 0), and
the plain-torch composition of (b) (losses.seg_loss on a contiguous channels-first tensor) with autograd, eager.

``--boundary`` times the boundary term instead (csrc/distmap.hip), same shapes, C = 2, no background class:
  (a) Dice + weighted cross-entropy with 20 % ignored, the launches of SegLoss's forward and backward (mivp_seg_loss,
      then mivp_seg_loss_grad): the path without the term
  (b) the same with lambda_boundary > 0: plus the four launches of the distance maps, the term's value pass and its
      gradient pass accumulating onto the same dz (the launches of losses._SegBoundaryFn)
  (c) mivp_distmap_signed alone
  (d) mivp_boundary_loss alone (value + gradient) on precomputed maps
  (e) for scale, eager and on the CPU: scipy's distance_transform_edt per sample and side plus the torch term with autograd
(a) - (d) are C-ABI call sequences on operands allocated beforehand, recorded in a HIP graph on one stream (no autograd
inside a recording); (b) - (a) is written as a share of the `downstream` step.

``--cldice`` times the clDice term instead (csrc/cldice.hip), same shapes and operands, C = 2, 3 iterations:
  (a) as above: the path without the term
  (b) the same with lambda_cldice > 0: mivp_cldice_loss after the value pass and mivp_cldice_loss_grad accumulating onto
      the same dz after the gradient pass (the launches of losses._SegTermsFn)
  (c) the skeleton passes of one side alone: mivp_cldice_skeleton (kept) + mivp_cldice_skeleton_grad on p_1 [B, 1, H, W, D]
  (d) the clDice authors' max-pool composition of the term with autograd, eager, on the same GPU

``--hausdorff`` times the Hausdorff distance-transform term instead (csrc/hausdorff.hip), same shapes and
operands as ``--boundary``, alpha = 2:
  (a) as above: the path without the term
  (b) the same plus the term through HausdorffDTLoss: mivp_hausdorff_maps, the term's value pass and, after the base's
      gradient pass, its gradient pass (here accumulating onto the same dz; the module leaves that add to autograd)
  (c) mivp_hausdorff_maps alone
  (d) mivp_hausdorff_loss alone (value + gradient) on given maps
  (e) mivp_distmap_signed alone, the maps of ``--boundary``, in the same job: half the fields of (c)
  (f) for scale, eager and on the CPU: scipy's distance_transform_edt of both masks and sides plus the torch term with autograd

``--lovasz`` times the Lovasz-Softmax term instead (csrc/lovasz.hip), same shapes and operands, C = 2, both
classes, the batch as one segment per class (7.1 M and 3.7 M keys):
  (a) as above: the path without the term
  (b) the same plus the term through LovaszSoftmaxLoss: mivp_lovasz_loss after the base's value pass and, after the base's
      gradient pass, mivp_lovasz_loss_grad (here accumulating onto the same dz; the module leaves that add to autograd)
  (c) mivp_lovasz_loss alone, value only: keys, sort, prefix, statistics, finalize
  (d) mivp_lovasz_loss_grad alone: the searches
  (e) a device copy of the term's unsorted keys + mivp_sort_u32 on them, and (f) that copy alone: (e) - (f) is the sort, set
      against the 4 passes x 2 x 4 N bytes its keys have to move (an estimate, at 6.3 TB/s)
  (g) the authors' composition with autograd, eager, on the same GPU: torch.sort per class, cumsum, a gather back

``--multilabel`` times the multi-label loss, decode and counts instead (csrc/multilabel.hip), same two shapes,
R = 3 (the BraTS groups), 20 % of the voxels ignored:
  (a) mivp_multilabel_loss, value + gradient: Dice + binary cross-entropy
  (b) the same with Tversky (0.3, 0.7), gamma = 2, group weights and pos_weight
  (c) mivp_seg_loss at C = 3 on the same logits: Dice + weighted cross-entropy, the softmax sibling moving the same bytes
  (d) the torch composition of (a) with autograd, eager, on the same GPU (multilabel._multilabel_loss_torch)
  (e) on a 512 x 512 x 96 volume: mivp_multilabel_decode (labels + bits) then mivp_group_counts on the bits, (f) the decode
      alone with the probabilities as well, and (g) the eager torch composition of (e): sigmoid, three compares, a table
      lookup, an ``isin`` per group and nine sums

Each kernel variant is one call (value + gradient) recorded in a HIP graph; a run is `replays` replays between two device
events after `warmup` replays; the figure is the median over `runs` runs with the spread (min .. max).  One JSON line per
variant, then one summary line.  No time is a pass criterion."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mivp_amd  # noqa: E402,F401
from mivp_amd import _lib as L  # noqa: E402
from mivp_amd import losses  # noqa: E402

DEV = "cuda"
STEP_MS = 2.41                                                    # the `downstream` step the shares refer to
SHAPES = (("96^3 B4", 4, (96, 96, 96)), ("128x128x8 B14", 14, (128, 128, 8)))
WEIGHTS = (0.5, 2.0)
IGNORE = 255


def timed(fn, runs, replays, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(replays):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / replays)
    return dict(ms=statistics.median(ms), lo=min(ms), hi=max(ms))


def recorded(call):
    """One call in a HIP graph; returns the replay function."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()                                                    # eager once: module load, allocations
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    return g.replay


def seg_variant(z, y, w, dz, loss, alpha, beta, gamma, weighted, ignore, lam_r, lam_v):
    B, vol, Cc = z.shape
    ws = torch.empty(int(L.lib().mivp_seg_loss_ws(B, vol)), dtype=torch.float32, device=DEV)
    wp = w if weighted else None

    def call():
        L.call("mivp_seg_loss", L.ptr(z), L.ptr(y), B, vol, Cc, 1, 0, alpha, beta, gamma, L.ptr(wp), IGNORE, 1 if ignore else 0,
               lam_r, lam_v, L.ptr(ws), L.ptr(loss), L.ptr(dz), L.stream())
    return call


def topk_variant(z, y, w, dz, loss, top_k):
    B, vol, Cc = z.shape
    ws = torch.empty(int(L.lib().mivp_seg_topk_ws(B, vol)), dtype=torch.float32, device=DEV)

    def call():
        L.call("mivp_seg_topk", L.ptr(z), L.ptr(y), B, vol, Cc, 1, 0, 0.5, 0.5, 0.0, L.ptr(w), IGNORE, 1, 1.0, 1.0, top_k,
               L.ptr(ws), L.ptr(loss), L.ptr(dz), L.stream())
    return call


def dice_focal_variant(z, y, dz, loss, gamma):
    B, vol, Cc = z.shape
    ws = torch.empty(int(L.lib().mivp_dice_focal_ws(B, vol)), dtype=torch.float32, device=DEV)

    def call():
        L.call("mivp_dice_focal", L.ptr(z), L.ptr(y), B, vol, Cc, 1, gamma, L.ptr(ws), L.ptr(loss), L.ptr(dz), L.stream())
    return call


def lesion_case(B, dims, Cc):
    """(logits [B, vol, C] on the device, labels [B, 1, H, W, D] on the CPU): 2 randn logits, a few ellipsoid lesions of class 1
    per sample, 20 % of the voxels the ignore label."""
    vol = dims[0] * dims[1] * dims[2]
    g = torch.Generator().manual_seed(1)
    z = (2.0 * torch.randn((B, vol, Cc), generator=g)).to(DEV)
    hh, ww, dd = torch.meshgrid(*[torch.arange(n) for n in dims], indexing="ij")
    y = torch.zeros((B, 1) + dims)
    for b in range(B):
        for _ in range(4):
            c = [float(torch.rand(1, generator=g)) * n for n in dims]
            r = [max(1.5, (0.05 + 0.15 * float(torch.rand(1, generator=g))) * n) for n in dims]
            y[b, 0][((hh - c[0]) / r[0]) ** 2 + ((ww - c[1]) / r[1]) ** 2 + ((dd - c[2]) / r[2]) ** 2 <= 1.0] = 1.0
    y[torch.rand(y.shape, generator=g) < 0.2] = float(IGNORE)
    return z, y


def cldice_main(args):
    """The clDice term: see the module docstring."""
    import torch.nn.functional as F
    summary = {}
    n, lam = 3, 0.5
    for name, B, dims in SHAPES:
        vol, Cc = dims[0] * dims[1] * dims[2], 2
        z, y = lesion_case(B, dims, Cc)
        yf = y.view(B, vol).to(DEV)
        w = torch.tensor(WEIGHTS, dtype=torch.float32, device=DEV)
        # every operand is allocated here, outside the recordings: the recorded calls are the launches of the product path
        # (losses._SegLossFn / _SegTermsFn, forward then backward) and nothing else
        dz, loss = torch.empty_like(z), torch.empty(2, dtype=torch.float32, device=DEV)
        one = torch.ones(1, dtype=torch.float32, device=DEV)     # the incoming gradient, the term's weight
        d3 = (C.c_int32 * 3)(*dims)
        sws = torch.empty(int(L.lib().mivp_seg_loss_ws(B, vol)), dtype=torch.float32, device=DEV)
        cws = torch.empty(int(L.lib().mivp_cldice_ws(B, Cc, d3, n)), dtype=torch.float32, device=DEV)
        kws = torch.empty(int(L.lib().mivp_cldice_skeleton_ws(B, d3, n, 1)), dtype=torch.float32, device=DEV)
        field = torch.softmax(z, -1)[..., 1].contiguous()        # [B, vol]: what the skeleton of the term works on
        skel, gfield, dfield = torch.empty_like(field), torch.randn_like(field), torch.empty_like(field)

        def seg_value():
            L.call("mivp_seg_loss", L.ptr(z), L.ptr(yf), B, vol, Cc, 0, 0, 0.5, 0.5, 0.0, L.ptr(w), IGNORE, 1, 1.0, 1.0, L.ptr(sws),
                   L.ptr(loss), None, L.stream())

        def seg_grad():
            L.call("mivp_seg_loss_grad", L.ptr(z), L.ptr(yf), B, vol, Cc, 0, 0, 0.5, 0.5, 0.0, L.ptr(w), IGNORE, 1, 1.0, 1.0,
                   L.ptr(sws), L.ptr(one), L.ptr(dz), L.stream())

        def plain_step():
            seg_value()
            seg_grad()

        def cldice_step():
            seg_value()
            L.call("mivp_cldice_loss", L.ptr(z), L.ptr(yf), B, Cc, d3, n, 1.0, 0, IGNORE, 1, lam, L.ptr(one), L.ptr(cws),
                   C.c_void_p(loss.data_ptr() + 4), None, 0, L.stream())
            seg_grad()
            L.call("mivp_cldice_loss_grad", L.ptr(z), L.ptr(yf), B, Cc, d3, n, 1.0, 0, IGNORE, 1, lam, L.ptr(one), L.ptr(cws),
                   L.ptr(one), L.ptr(dz), 1, L.stream())

        def skeleton_alone():
            L.call("mivp_cldice_skeleton", L.ptr(field), B, d3, n, L.ptr(skel), L.ptr(kws), 1, L.stream())
            L.call("mivp_cldice_skeleton_grad", L.ptr(field), L.ptr(gfield), B, d3, n, L.ptr(kws), L.ptr(dfield), L.stream())

        res = {}
        for key, label, call in (("a", "(a) dice + weighted CE, value then gradient", plain_step),
                                 ("b", "(b) the same with the clDice term", cldice_step),
                                 ("c", "(c) one side's skeleton passes alone, forward + backward", skeleton_alone)):
            r = timed(recorded(call), args.runs, args.replays, args.warmup)
            r.update(shape=name, variant=label, share_of_step=r["ms"] / STEP_MS)
            res[key] = r
            summary[f"{name} | {label}"] = [round(r[k], 4) for k in ("ms", "lo", "hi")]
            print(json.dumps(r), flush=True)
        extra = res["b"]["ms"] - res["a"]["ms"]
        summary[f"{name} | (b) - (a)"] = dict(ms=round(extra, 4), share_of_step=round(extra / STEP_MS, 4))

        # the clDice authors' composition on the same GPU: max-pool erosions / dilations, autograd (first-index ties)
        def erode(img):
            return torch.min(torch.min(-F.max_pool3d(-img, (3, 1, 1), 1, (1, 0, 0)), -F.max_pool3d(-img, (1, 3, 1), 1, (0, 1, 0))),
                             -F.max_pool3d(-img, (1, 1, 3), 1, (0, 0, 1)))

        def skel_of(img):
            s = F.relu(img - F.max_pool3d(erode(img), 3, 1, 1))
            for _ in range(n):
                img = erode(img)
                d = F.relu(img - F.max_pool3d(erode(img), 3, 1, 1))
                s = s + F.relu(d - s * d)
            return s

        plain = z.view(B, *dims, Cc).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
        yd = y.to(DEV)
        valid = (yd != float(IGNORE)).float()
        t = (yd == 1.0).float()

        def eager():
            plain.grad = None
            p = torch.softmax(plain, 1)[:, 1:] * valid
            sp, sl = skel_of(p), skel_of(t)
            ax = (2, 3, 4)
            tprec = ((sp * t).sum(ax) + 1.0) / (sp.sum(ax) + 1.0)
            tsens = ((sl * p).sum(ax) + 1.0) / (sl.sum(ax) + 1.0)
            (lam * (1.0 - 2.0 * tprec * tsens / (tprec + tsens)).mean()).backward()
        r = timed(eager, args.runs, max(3, args.replays // 10), 3)
        r.update(shape=name, variant="(d) torch max-pool composition of the term, eager", share_of_step=r["ms"] / STEP_MS)
        summary[f"{name} | (d) torch eager"] = [round(r[k], 4) for k in ("ms", "lo", "hi")]
        print(json.dumps(r), flush=True)
    print(json.dumps({"bench_cldice_ms": summary}))


def boundary_main(args):
    """The boundary term: see the module docstring."""
    import time
    summary = {}
    for name, B, dims in SHAPES:
        vol, Cc = dims[0] * dims[1] * dims[2], 2
        z, y = lesion_case(B, dims, Cc)
        yf = y.view(B, vol).to(DEV)
        w = torch.tensor(WEIGHTS, dtype=torch.float32, device=DEV)
        # every operand is allocated here, outside the recordings: the recorded calls are the launches of the product path
        # (losses._SegLossFn / _SegBoundaryFn, forward then backward) and nothing else
        dz, loss = torch.empty_like(z), torch.empty(2, dtype=torch.float32, device=DEV)
        one = torch.ones(1, dtype=torch.float32, device=DEV)     # the incoming gradient, the boundary weight
        sws = torch.empty(int(L.lib().mivp_seg_loss_ws(B, vol)), dtype=torch.float32, device=DEV)
        bws = torch.empty(int(L.lib().mivp_boundary_loss_ws(B, vol)), dtype=torch.float32, device=DEV)
        K, d3, sp = Cc - 1, (C.c_int32 * 3)(*dims), (C.c_float * 3)(1.0, 1.0, 1.0)
        mws = torch.empty(int(L.lib().mivp_distmap_ws(B, K, d3)), dtype=torch.uint8, device=DEV)
        phi = torch.empty((B, K, vol), dtype=torch.float32, device=DEV)
        lam = 0.01

        def seg_value():
            L.call("mivp_seg_loss", L.ptr(z), L.ptr(yf), B, vol, Cc, 0, 0, 0.5, 0.5, 0.0, L.ptr(w), IGNORE, 1, 1.0, 1.0, L.ptr(sws),
                   L.ptr(loss), None, L.stream())

        def seg_grad():
            L.call("mivp_seg_loss_grad", L.ptr(z), L.ptr(yf), B, vol, Cc, 0, 0, 0.5, 0.5, 0.0, L.ptr(w), IGNORE, 1, 1.0, 1.0,
                   L.ptr(sws), L.ptr(one), L.ptr(dz), L.stream())

        def maps_alone():
            L.call("mivp_distmap_signed", L.ptr(yf), B, Cc, 0, IGNORE, 1, d3, sp, L.ptr(phi), L.ptr(mws), L.stream())

        def plain_step():
            seg_value()
            seg_grad()

        def boundary_step():
            seg_value()
            maps_alone()
            L.call("mivp_boundary_loss", L.ptr(z), L.ptr(yf), L.ptr(phi), B, vol, Cc, 0, IGNORE, 1, lam, L.ptr(one), L.ptr(bws),
                   C.c_void_p(loss.data_ptr() + 4), None, 0, L.stream())
            seg_grad()
            L.call("mivp_boundary_loss_grad", L.ptr(z), L.ptr(yf), L.ptr(phi), B, vol, Cc, 0, IGNORE, 1, lam, L.ptr(one),
                   L.ptr(bws), L.ptr(one), L.ptr(dz), 1, L.stream())

        def term_alone():
            L.call("mivp_boundary_loss", L.ptr(z), L.ptr(yf), L.ptr(phi), B, vol, Cc, 0, IGNORE, 1, 1.0, None, L.ptr(bws),
                   L.ptr(loss), L.ptr(dz), 0, L.stream())

        res = {}
        for key, label, call in (("a", "(a) dice + weighted CE, value then gradient", plain_step),
                                 ("b", "(b) the same with the boundary term", boundary_step),
                                 ("c", "(c) the distance maps alone", maps_alone),
                                 ("d", "(d) mivp_boundary_loss alone, maps given", term_alone)):
            r = timed(recorded(call), args.runs, args.replays, args.warmup)
            r.update(shape=name, variant=label, share_of_step=r["ms"] / STEP_MS)
            res[key] = r
            summary[f"{name} | {label}"] = [round(r[k], 4) for k in ("ms", "lo", "hi")]
            print(json.dumps(r), flush=True)
        extra = res["b"]["ms"] - res["a"]["ms"]
        summary[f"{name} | (b) - (a)"] = dict(ms=round(extra, 4), share_of_step=round(extra / STEP_MS, 4))
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None:
            yc, zc = y[:, 0].numpy(), z.cpu()
            ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                maps = []
                for b in range(B):
                    M = yc[b] == 1.0
                    maps.append(ndimage.distance_transform_edt(~M) * ~M - (ndimage.distance_transform_edt(M) - 1.0) * M
                                if M.any() and not M.all() else 0.0 * M)
                dist = torch.from_numpy(__import__("numpy").stack(maps)).float().view(B, 1, *dims)
                zl = zc.clone().requires_grad_(True)
                losses.boundary_loss(zl.view(B, *dims, Cc).permute(0, 4, 1, 2, 3).contiguous(), y, ignore_index=IGNORE,
                                     dist=dist).backward()
                ms.append((time.perf_counter() - t0) * 1e3)
            r = dict(ms=statistics.median(ms), lo=min(ms), hi=max(ms), shape=name, variant="(e) scipy EDT + eager torch term, CPU")
            summary[f"{name} | (e) scipy + torch, CPU"] = [round(r[k], 2) for k in ("ms", "lo", "hi")]
            print(json.dumps(r), flush=True)
    print(json.dumps({"bench_boundary_ms": summary}))


def hausdorff_main(args):
    """The Hausdorff distance-transform term: see the module docstring."""
    import time
    summary = {}
    for name, B, dims in SHAPES:
        vol, Cc = dims[0] * dims[1] * dims[2], 2
        z, y = lesion_case(B, dims, Cc)
        yf = y.view(B, vol).to(DEV)
        w = torch.tensor(WEIGHTS, dtype=torch.float32, device=DEV)
        # every operand is allocated here, outside the recordings
        dz, loss = torch.empty_like(z), torch.empty(2, dtype=torch.float32, device=DEV)
        one = torch.ones(1, dtype=torch.float32, device=DEV)     # the incoming gradient, the term's weight
        sws = torch.empty(int(L.lib().mivp_seg_loss_ws(B, vol)), dtype=torch.float32, device=DEV)
        hws = torch.empty(int(L.lib().mivp_hausdorff_loss_ws(B, vol)), dtype=torch.float32, device=DEV)
        K, d3, sp = Cc - 1, (C.c_int32 * 3)(*dims), (C.c_float * 3)(1.0, 1.0, 1.0)
        mws = torch.empty(int(L.lib().mivp_hausdorff_maps_ws(B, K, d3)), dtype=torch.uint8, device=DEV)
        bws = torch.empty(int(L.lib().mivp_distmap_ws(B, K, d3)), dtype=torch.uint8, device=DEV)
        wmap = torch.empty((B, K, vol), dtype=torch.float32, device=DEV)
        phi = torch.empty((B, K, vol), dtype=torch.float32, device=DEV)
        lam = 0.01

        def seg_value():
            L.call("mivp_seg_loss", L.ptr(z), L.ptr(yf), B, vol, Cc, 0, 0, 0.5, 0.5, 0.0, L.ptr(w), IGNORE, 1, 1.0, 1.0, L.ptr(sws),
                   L.ptr(loss), None, L.stream())

        def seg_grad():
            L.call("mivp_seg_loss_grad", L.ptr(z), L.ptr(yf), B, vol, Cc, 0, 0, 0.5, 0.5, 0.0, L.ptr(w), IGNORE, 1, 1.0, 1.0,
                   L.ptr(sws), L.ptr(one), L.ptr(dz), L.stream())

        def maps_alone():
            L.call("mivp_hausdorff_maps", L.ptr(z), L.ptr(yf), B, Cc, 0, IGNORE, 1, d3, sp, 2.0, L.ptr(wmap), L.ptr(mws), L.stream())

        def boundary_maps():
            L.call("mivp_distmap_signed", L.ptr(yf), B, Cc, 0, IGNORE, 1, d3, sp, L.ptr(phi), L.ptr(bws), L.stream())

        def plain_step():
            seg_value()
            seg_grad()

        def hausdorff_step():
            seg_value()
            maps_alone()
            L.call("mivp_hausdorff_loss", L.ptr(z), L.ptr(yf), L.ptr(wmap), B, vol, Cc, 0, IGNORE, 1, lam, L.ptr(one), L.ptr(hws),
                   C.c_void_p(loss.data_ptr() + 4), None, 0, L.stream())
            seg_grad()
            L.call("mivp_hausdorff_loss_grad", L.ptr(z), L.ptr(yf), L.ptr(wmap), B, vol, Cc, 0, IGNORE, 1, lam, L.ptr(one),
                   L.ptr(hws), L.ptr(one), L.ptr(dz), 1, L.stream())

        def term_alone():
            L.call("mivp_hausdorff_loss", L.ptr(z), L.ptr(yf), L.ptr(wmap), B, vol, Cc, 0, IGNORE, 1, 1.0, None, L.ptr(hws),
                   L.ptr(loss), L.ptr(dz), 0, L.stream())

        res = {}
        for key, label, call in (("a", "(a) dice + weighted CE, value then gradient", plain_step),
                                 ("b", "(b) the same with the Hausdorff term", hausdorff_step),
                                 ("c", "(c) mivp_hausdorff_maps alone", maps_alone),
                                 ("d", "(d) mivp_hausdorff_loss alone, maps given", term_alone),
                                 ("e", "(e) mivp_distmap_signed alone (the --boundary maps)", boundary_maps)):
            r = timed(recorded(call), args.runs, args.replays, args.warmup)
            r.update(shape=name, variant=label, share_of_step=r["ms"] / STEP_MS)
            res[key] = r
            summary[f"{name} | {label}"] = [round(r[k], 4) for k in ("ms", "lo", "hi")]
            print(json.dumps(r), flush=True)
        extra = res["b"]["ms"] - res["a"]["ms"]
        summary[f"{name} | (b) - (a)"] = dict(ms=round(extra, 4), share_of_step=round(extra / STEP_MS, 4))
        summary[f"{name} | (c) / (e)"] = round(res["c"]["ms"] / res["e"]["ms"], 3)
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None:
            import numpy as np
            yc, zc = y[:, 0].numpy(), z.cpu()

            def field_sq(M):
                if not M.any() or M.all():
                    return np.zeros(M.shape)
                return np.where(M, ndimage.distance_transform_edt(M), ndimage.distance_transform_edt(~M)) ** 2
            ms = []
            for _ in range(3):
                t0 = time.perf_counter()
                pred = zc.view(B, *dims, Cc).argmax(-1).numpy()
                maps = np.stack([field_sq(pred[b] == 1) + field_sq(yc[b] == 1.0) for b in range(B)])
                zl = zc.clone().requires_grad_(True)
                losses.hausdorff_dt_loss(zl.view(B, *dims, Cc).permute(0, 4, 1, 2, 3).contiguous(), y, ignore_index=IGNORE,
                                         maps=torch.from_numpy(maps).float().view(B, 1, *dims)).backward()
                ms.append((time.perf_counter() - t0) * 1e3)
            r = dict(ms=statistics.median(ms), lo=min(ms), hi=max(ms), shape=name, variant="(f) scipy EDT + eager torch term, CPU")
            summary[f"{name} | (f) scipy + torch, CPU"] = [round(r[k], 2) for k in ("ms", "lo", "hi")]
            print(json.dumps(r), flush=True)
    print(json.dumps({"bench_hausdorff_ms": summary}))


def lovasz_main(args):
    """The Lovasz-Softmax term: see the module docstring."""
    summary = {}
    lam = 0.5
    for name, B, dims in SHAPES:
        vol, Cc = dims[0] * dims[1] * dims[2], 2
        z, y = lesion_case(B, dims, Cc)
        yf = y.view(B, vol).to(DEV)
        w = torch.tensor(WEIGHTS, dtype=torch.float32, device=DEV)
        # every operand is allocated here, outside the recordings
        dz, loss = torch.empty_like(z), torch.empty(2, dtype=torch.float32, device=DEV)
        one = torch.ones(1, dtype=torch.float32, device=DEV)     # the incoming gradient, the term's weight
        sws = torch.empty(int(L.lib().mivp_seg_loss_ws(B, vol)), dtype=torch.float32, device=DEV)
        lws = torch.empty(int(L.lib().mivp_lovasz_ws(B, Cc, 1, 0, vol)), dtype=torch.uint8, device=DEV)
        S, N = Cc, B * vol
        fresh = torch.empty((S, N), dtype=torch.int32, device=DEV)
        keys, counts = torch.empty_like(fresh), torch.empty((S, 2), dtype=torch.int32, device=DEV)
        L.call("mivp_lovasz_keys", L.ptr(z), L.ptr(yf), B, vol, Cc, 1, IGNORE, 1, 0, L.ptr(fresh), L.ptr(counts), L.stream())
        kws = torch.empty(int(L.lib().mivp_sort_u32_ws(S, N)), dtype=torch.uint8, device=DEV)

        def seg_value():
            L.call("mivp_seg_loss", L.ptr(z), L.ptr(yf), B, vol, Cc, 0, 0, 0.5, 0.5, 0.0, L.ptr(w), IGNORE, 1, 1.0, 1.0, L.ptr(sws),
                   L.ptr(loss), None, L.stream())

        def seg_grad():
            L.call("mivp_seg_loss_grad", L.ptr(z), L.ptr(yf), B, vol, Cc, 0, 0, 0.5, 0.5, 0.0, L.ptr(w), IGNORE, 1, 1.0, 1.0,
                   L.ptr(sws), L.ptr(one), L.ptr(dz), L.stream())

        def term_value():
            L.call("mivp_lovasz_loss", L.ptr(z), L.ptr(yf), B, vol, Cc, 1, IGNORE, 1, 0, 0, lam, L.ptr(one), L.ptr(lws),
                   C.c_void_p(loss.data_ptr() + 4), None, 0, L.stream())

        def term_grad():
            L.call("mivp_lovasz_loss_grad", L.ptr(z), L.ptr(yf), B, vol, Cc, 1, IGNORE, 1, 0, 0, lam, L.ptr(one), L.ptr(lws),
                   L.ptr(one), L.ptr(dz), 1, L.stream())

        def plain_step():
            seg_value()
            seg_grad()

        def lovasz_step():
            seg_value()
            term_value()
            seg_grad()
            term_grad()

        def copy_alone():
            keys.copy_(fresh)

        def copy_and_sort():
            keys.copy_(fresh)
            L.call("mivp_sort_u32", L.ptr(keys), S, N, L.ptr(kws), L.stream())

        res = {}
        term_value()                                              # (d) reads the workspace of a value pass
        for key, label, call in (("a", "(a) dice + weighted CE, value then gradient", plain_step),
                                 ("b", "(b) the same with the Lovasz-Softmax term", lovasz_step),
                                 ("c", "(c) mivp_lovasz_loss alone, value only", term_value),
                                 ("d", "(d) mivp_lovasz_loss_grad alone", term_grad),
                                 ("e", "(e) copy of the unsorted keys + mivp_sort_u32", copy_and_sort),
                                 ("f", "(f) that copy alone", copy_alone)):
            r = timed(recorded(call), args.runs, args.replays, args.warmup)
            r.update(shape=name, variant=label, share_of_step=r["ms"] / STEP_MS)
            res[key] = r
            summary[f"{name} | {label}"] = [round(r[k], 4) for k in ("ms", "lo", "hi")]
            print(json.dumps(r), flush=True)
        extra = res["b"]["ms"] - res["a"]["ms"]
        summary[f"{name} | (b) - (a)"] = dict(ms=round(extra, 4), share_of_step=round(extra / STEP_MS, 4))
        sort_ms = res["e"]["ms"] - res["f"]["ms"]
        est_gb = 4 * 2 * 4 * S * N / 1e9
        summary[f"{name} | (e) - (f), the sort of {S * N} keys"] = dict(
            ms=round(sort_ms, 4), estimate_gb=round(est_gb, 4), estimate_ms_at_6p3_tb_s=round(est_gb / 6.3, 4),
            multiple_of_estimate=round(sort_ms / (est_gb / 6.3), 2))

        # the authors' composition on the same GPU: softmax, then per class a sort of the errors, the Jaccard recurrence on the
        # sorted labels and a dot product; autograd gathers back through the sort's indices
        plain = z.view(B, *dims, Cc).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
        lab = yf.view(-1)
        keep = lab != float(IGNORE)

        def eager():
            plain.grad = None
            p = torch.softmax(plain, 1).permute(0, 2, 3, 4, 1).reshape(-1, Cc)[keep]
            yk = lab[keep]
            terms = []
            for c in range(Cc):
                fg = (yk == c).float()
                if fg.sum() == 0:
                    continue
                es, perm = torch.sort((fg - p[:, c]).abs(), 0, descending=True)
                fs = fg[perm]
                gts = fs.sum()
                jac = 1.0 - (gts - fs.cumsum(0)) / (gts + (1.0 - fs).cumsum(0))
                jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
                terms.append(torch.dot(es, jac))
            (lam * torch.stack(terms).mean()).backward()
        r = timed(eager, args.runs, max(3, args.replays // 10), 3)
        r.update(shape=name, variant="(g) torch.sort composition of the term, eager", share_of_step=r["ms"] / STEP_MS)
        summary[f"{name} | (g) torch eager"] = [round(r[k], 4) for k in ("ms", "lo", "hi")]
        summary[f"{name} | (g) / ((c) + (d))"] = round(r["ms"] / (res["c"]["ms"] + res["d"]["ms"]), 2)
        print(json.dumps(r), flush=True)
    print(json.dumps({"bench_lovasz_ms": summary}))


def multilabel_main(args):
    """The multi-label loss, decode and counts: see the module docstring."""
    from mivp_amd import multilabel as M
    brats = M.LabelGroups([(1, 2, 3), (2, 3), (3,)])
    Rg = brats.R
    member, lut = brats.tables(torch.device(DEV))
    summary = {}

    def put(name, label, r, digits=4):
        r.update(shape=name, variant=label)
        summary[f"{name} | {label}"] = [round(r[k], digits) for k in ("ms", "lo", "hi")]
        print(json.dumps(r), flush=True)
        return r

    for name, B, dims in SHAPES:
        vol = dims[0] * dims[1] * dims[2]
        g = torch.Generator().manual_seed(1)
        z = (2.0 * torch.randn((B, vol, Rg), generator=g)).to(DEV)
        y = torch.randint(0, 4, (B, vol), generator=g).float()
        y[torch.rand((B, vol), generator=g) < 0.2] = float(IGNORE)
        y = y.to(DEV)
        dz, loss = torch.empty_like(z), torch.empty(1, dtype=torch.float32, device=DEV)
        gw = torch.tensor((0.5, 2.0, 1.0), dtype=torch.float32, device=DEV)
        pw = torch.tensor((2.0, 0.5, 3.0), dtype=torch.float32, device=DEV)
        ws = torch.empty(int(L.lib().mivp_multilabel_loss_ws(B, vol)), dtype=torch.float32, device=DEV)

        def ml_plain():
            L.call("mivp_multilabel_loss", L.ptr(z), L.ptr(y), B, vol, Rg, L.ptr(member), 0, 0.5, 0.5, 0.0, None, None, IGNORE, 1,
                   1.0, 1.0, L.ptr(ws), L.ptr(loss), L.ptr(dz), L.stream())

        def ml_full():
            L.call("mivp_multilabel_loss", L.ptr(z), L.ptr(y), B, vol, Rg, L.ptr(member), 0, 0.3, 0.7, 2.0, L.ptr(gw), L.ptr(pw),
                   IGNORE, 1, 1.0, 1.0, L.ptr(ws), L.ptr(loss), L.ptr(dz), L.stream())

        res = {}
        for key, label, call in (("a", "(a) multilabel dice + BCE, R = 3", ml_plain),
                                 ("b", "(b) multilabel tversky + focal BCE gamma 2, weights", ml_full),
                                 ("c", "(c) seg_loss dice + weighted CE, C = 3",
                                  seg_variant(z, y, gw, dz, loss, 0.5, 0.5, 0.0, True, True, 1.0, 1.0))):
            r = put(name, label, timed(recorded(call), args.runs, args.replays, args.warmup))
            r.update(gb_s=3 * z.numel() * 4 / r["ms"] / 1e6)
            res[key] = r
        plain = z.view(B, *dims, Rg).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
        spec = M.MultiLabelSpec(ignore_index=IGNORE)

        def eager():
            plain.grad = None
            M._multilabel_loss_torch(plain.permute(0, 2, 3, 4, 1).reshape(B, -1, Rg), y, member, spec, None, None).backward()
        r = put(name, "(d) torch composition of (a), eager", timed(eager, args.runs, max(3, args.replays // 10), 3))
        summary[f"{name} | (d) / (a)"] = round(r["ms"] / res["a"]["ms"], 2)
        summary[f"{name} | (a) / (c)"] = round(res["a"]["ms"] / res["c"]["ms"], 3)
    # decode + counts on one whole volume, the planes predict(return_logits=True) returns
    name, dims = "512x512x96", (512, 512, 96)
    vol = dims[0] * dims[1] * dims[2]
    g = torch.Generator().manual_seed(2)
    planes = (2.0 * torch.randn((Rg, vol), generator=g)).to(DEV)
    seg = torch.randint(0, 4, (vol,), generator=g).to(torch.uint8).to(DEV)
    tau = torch.zeros(Rg, dtype=torch.float32, device=DEV)
    labels, bitsmap = torch.empty(vol, dtype=torch.uint8, device=DEV), torch.empty(vol, dtype=torch.uint8, device=DEV)
    probs = torch.empty((Rg, vol), dtype=torch.float32, device=DEV)
    counts = torch.zeros((Rg, 3), dtype=torch.int64, device=DEV)

    def decode_counts():
        L.call("mivp_multilabel_decode", L.ptr(planes), 1, vol, Rg, 0, L.ptr(tau), L.ptr(lut), L.ptr(labels), L.ptr(bitsmap), None,
               L.stream())
        L.call("mivp_group_counts", L.ptr(bitsmap), 0, 0, L.ptr(seg), 0, vol, Rg, L.ptr(member), 0, 0, L.ptr(counts), L.stream())

    def decode_probs():
        L.call("mivp_multilabel_decode", L.ptr(planes), 1, vol, Rg, 0, L.ptr(tau), L.ptr(lut), L.ptr(labels), L.ptr(bitsmap),
               L.ptr(probs), L.stream())

    e = put(name, "(e) decode (labels + bits) + group counts", timed(recorded(decode_counts), args.runs, args.replays, args.warmup))
    e.update(gb_s=(planes.numel() * 4 + 4 * vol) / e["ms"] / 1e6)
    f = put(name, "(f) decode with probabilities", timed(recorded(decode_probs), args.runs, args.replays, args.warmup))
    f.update(gb_s=(2 * planes.numel() * 4 + 2 * vol) / f["ms"] / 1e6)
    lut_l = lut.long()
    sets = [torch.tensor(s, dtype=torch.uint8, device=DEV) for s in brats.groups]

    def eager_decode():
        on = torch.sigmoid(planes) > 0.5
        b = on[0].long() + 2 * on[1].long() + 4 * on[2].long()
        lab = lut_l[b]
        out = []
        for r in range(Rg):
            t = torch.isin(seg, sets[r])
            out += [(on[r] & t).sum(), on[r].sum(), t.sum()]
        return lab, torch.stack(out)
    r = put(name, "(g) torch composition of (e), eager", timed(eager_decode, args.runs, max(3, args.replays // 10), 3))
    summary[f"{name} | (g) / (e)"] = round(r["ms"] / e["ms"], 2)
    print(json.dumps({"bench_multilabel_ms": summary}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--boundary", action="store_true", help="time the boundary term (DESIGN 4.35) instead")
    ap.add_argument("--cldice", action="store_true", help="time the clDice term (DESIGN 4.36) instead")
    ap.add_argument("--hausdorff", action="store_true", help="time the Hausdorff distance-transform term (DESIGN 4.39) instead")
    ap.add_argument("--lovasz", action="store_true", help="time the Lovasz-Softmax term (DESIGN 4.40) instead")
    ap.add_argument("--multilabel", action="store_true", help="time the multi-label loss, decode and counts (DESIGN 4.45) instead")
    args = ap.parse_args()
    assert args.runs >= 3
    if args.multilabel:
        return multilabel_main(args)
    if args.lovasz:
        return lovasz_main(args)
    if args.hausdorff:
        return hausdorff_main(args)
    if args.boundary:
        return boundary_main(args)
    if args.cldice:
        return cldice_main(args)
    summary = {}
    for name, B, dims in SHAPES:
        vol, Cc = dims[0] * dims[1] * dims[2], 2
        g = torch.Generator().manual_seed(1)
        z = (2.0 * torch.randn((B, vol, Cc), generator=g)).to(DEV)
        y = torch.randint(0, Cc, (B, vol), generator=g).float()
        y_ig = y.clone()
        y_ig[torch.rand((B, vol), generator=g) < 0.2] = float(IGNORE)
        y, y_ig = y.to(DEV), y_ig.to(DEV)
        w = torch.tensor(WEIGHTS, dtype=torch.float32, device=DEV)
        dz, loss = torch.empty_like(z), torch.empty(1, dtype=torch.float32, device=DEV)
        variants = [
            ("dice_focal gamma 4 (baseline)", dice_focal_variant(z, y, dz, loss, 4.0)),
            ("dice alone (baseline)", dice_focal_variant(z, y, dz, loss, -1.0)),
            ("seg (a) dice-equivalent", seg_variant(z, y, w, dz, loss, 0.5, 0.5, 0.0, False, False, 1.0, 0.0)),
            ("seg (b) dice + weighted CE, 20% ignored", seg_variant(z, y_ig, w, dz, loss, 0.5, 0.5, 0.0, True, True, 1.0, 1.0)),
            ("seg (c) tversky + focal CE gamma 2", seg_variant(z, y_ig, w, dz, loss, 0.3, 0.7, 2.0, True, True, 1.0, 1.0)),
            ("seg (d) dice + top-k 10% weighted CE, 20% ignored", topk_variant(z, y_ig, w, dz, loss, 0.1)),
        ]
        for label, call in variants:
            r = timed(recorded(call), args.runs, args.replays, args.warmup)
            r.update(shape=name, variant=label, share_of_step=r["ms"] / STEP_MS, gb_s=3 * z.numel() * 4 / r["ms"] / 1e6)
            summary[f"{name} | {label}"] = round(r["ms"], 4)
            print(json.dumps(r), flush=True)
        # eager torch composition of (b), autograd
        spec = losses.SegLossSpec(class_weights=WEIGHTS, ignore_index=IGNORE)
        plain = z.view(B, *dims, Cc).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
        target = y_ig.view(B, 1, *dims)

        def eager():
            plain.grad = None
            losses.seg_loss(plain, target, spec, w).backward()
        r = timed(eager, args.runs, max(3, args.replays // 10), 3)
        r.update(shape=name, variant="torch composition of (b), eager", share_of_step=r["ms"] / STEP_MS)
        summary[f"{name} | torch (b) eager"] = round(r["ms"], 4)
        print(json.dumps(r), flush=True)
        # eager composition of (d)'s voxel term alone: per-voxel cross-entropy, a sort-based top-k, autograd through the indices
        flat = z.view(-1, Cc).clone().requires_grad_(True)
        labels = y_ig.view(-1).long()
        k = max(1, int(0.1 * int((labels != IGNORE).sum())))

        def eager_topk():
            flat.grad = None
            ce = torch.nn.functional.cross_entropy(flat, labels, weight=w, ignore_index=IGNORE, reduction="none")
            torch.topk(ce, k, sorted=False)[0].mean().backward()
        r = timed(eager_topk, args.runs, max(3, args.replays // 10), 3)
        r.update(shape=name, variant="torch cross_entropy(none) + topk, eager (voxel term of (d) alone)", share_of_step=r["ms"] / STEP_MS)
        summary[f"{name} | torch topk eager"] = round(r["ms"], 4)
        print(json.dumps(r), flush=True)
    print(json.dumps({"bench_loss_ms": summary}))


if __name__ == "__main__":
    main()
