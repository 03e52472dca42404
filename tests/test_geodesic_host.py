"""CPU: the restatement of the geodesic guidance (tests/geodesic_ref.py) checked against independent computations, and the host
side of mivp_amd.geodesic (refusals before any launch, the declarations of include/mivp.h).

  three float32 computations   Dijkstra = Bellman-Ford to its fixed point in raster and in reverse raster order = a brick-wise
                               Jacobi emulation (brick 4 x 4 x 4, two buffers, the scheme of the kernel), bit for bit, on every
                               case (the serpentine takes the longest, about 5 s: at gamma = 1000 a sweep lowers the voxels behind
                               a wall many times before the winding path reaches them)
  float64                      scipy's Dijkstra on the same graph (the float32 weights, summed in float64): the float32 field is
                               within hops 2^-24 relative.  Derivation: a path's float32 sum is folded left to right, each of
                               its hops - 1 additions within 2^-24 relative of the exact sum of its operands (weights > 0, no
                               cancellation), so the folded sum of a path of n hops lies within (1 +- 2^-24)^(n-1) of its exact
                               sum.  Upwards the float32 minimum is at most the folded sum of the float64 shortest path,
                               so it inherits that path's hop count; downwards it is the folded sum of its own minimising
                               path, whose hop count may differ, so the asserted bound (the hop count of the float64 path in
                               both directions, as the definition of the check sets it) is derived for the upper side and
                               is the same expression, not a derivation, for the lower one; each error and bound is printed
  Euclidean special case       gamma = 0 at unit spacing: the 26-neighbour chamfer distance with steps 1, fl(sqrt 2), fl(sqrt 3)"""
import heapq
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geodesic_ref as R  # noqa: E402

from conftest import ROOT  # noqa: E402



def G():
    import mivp_amd  # noqa: F401
    from mivp_amd import geodesic
    return geodesic


def planes(name):
    """(b, r, image, seeds bool, weights) of every field of a case"""
    c = R.CASES[name]
    for b in range(c["image"].shape[0]):
        W = R.edge_weights(c["image"][b], c["spacing"], c["gamma"])
        for r in range(2):
            yield b, r, c["image"][b], ((c["seeds"][b] >> r) & 1).astype(bool), W


def bellman_ford(W, seeds, reverse):
    """Gauss-Seidel sweeps over the voxels in raster (or reverse raster) order until a sweep changes nothing.  A voxel none of
    whose neighbours was lowered since its own last relaxation is passed over: relaxing it would change nothing, so the
    values after every sweep are those of the plain sweep.  The voxels a sweep has to visit are kept in a heap by their
    place in it: a neighbour further on joins this sweep, one already passed the next."""
    dims = seeds.shape
    n = seeds.size
    step = np.asarray([(o[0] * dims[1] + o[1]) * dims[2] + o[2] for o in R.OFFSETS])
    Wt = np.ascontiguousarray(W.reshape(26, n).T)                  # [n, 26] float32, +inf for an edge that is never taken
    fin = np.isfinite(Wt)
    nb = np.where(fin, np.arange(n)[:, None] + step[None, :], np.arange(n)[:, None])
    users = [nb[v][fin[v]].tolist() for v in range(n)]             # the neighbours that read v (the weights are symmetric)
    dist = np.where(seeds.reshape(-1), np.float32(0), np.float32(np.inf)).astype(np.float32)
    sign = -1 if reverse else 1                                    # a voxel's place in the sweep is sign * v
    ahead = [sign * v for v in range(n)]                           # the voxels this sweep still has to relax, as a heap
    heapq.heapify(ahead)
    queued = [True] * n
    while ahead:
        behind = []                                                # those the next sweep has to
        while ahead:
            v = sign * heapq.heappop(ahead)
            queued[v] = False
            best = (dist[nb[v]] + Wt[v]).min()                     # 26 float32 additions
            if best < dist[v]:
                dist[v] = best
                for u in users[v]:
                    if not queued[u]:
                        queued[u] = True
                        if sign * u > sign * v:
                            heapq.heappush(ahead, sign * u)
                        else:
                            behind.append(sign * u)
        ahead = behind
        heapq.heapify(ahead)
    assert dist.dtype == np.float32
    return dist.reshape(dims)


def brick_jacobi(W, seeds, brick=(4, 4, 4)):
    """Iterations of [every brick: Jacobi rounds on its own voxels, the voxels of other bricks read from buffer A, until the
    brick stops changing; the result is buffer B], swapping A and B, until an iteration lowers nothing."""
    dims = seeds.shape
    inf = np.float32(np.inf)
    ids = np.zeros(dims, dtype=np.int64)
    for a in range(3):
        shape = [1, 1, 1]
        shape[a] = dims[a]
        ids = ids * 65536 + (np.arange(dims[a]) // brick[a]).reshape(shape)
    same = [R._shifted(ids, off, -1) == ids for off in R.OFFSETS]
    A = np.where(seeds, np.float32(0), inf).astype(np.float32)
    iterations = 0
    while True:
        frozen = [R._shifted(A, off, inf) for off in R.OFFSETS]
        cur = A
        while True:
            new = cur.copy()
            for k, off in enumerate(R.OFFSETS):
                np.minimum(new, np.where(same[k], R._shifted(cur, off, inf), frozen[k]) + W[k], out=new)
            if np.array_equal(new, cur):
                break
            cur = new
        iterations += 1
        if np.array_equal(cur, A):
            return A, iterations
        A = cur


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# =============================================================================================
# the restatement
# =============================================================================================
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_dijkstra_equals_bellman_ford_in_both_orders(name):
    want = R.field(name)
    for b, r, _, seeds, W in planes(name):
        for reverse in (False, True):
            assert np.array_equal(bits(bellman_ford(W, seeds, reverse)), bits(want[b, r])), (b, r, reverse)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_dijkstra_equals_brickwise_jacobi(name):
    want = R.field(name)
    most = 0
    for b, r, _, seeds, W in planes(name):
        got, iterations = brick_jacobi(W, seeds)
        most = max(most, iterations)
        assert np.array_equal(bits(got), bits(want[b, r])), (b, r)
        assert np.array_equal(bits(R.relax_all(want[b, r], W)), bits(want[b, r]))      # and it is a fixed point
    if name == "serpentine":
        assert most > 20                                           # the path crosses brick faces many times


def float64_fields(W, seeds):
    """(distance float64 [H, W, D], hops of the float64 shortest path) by scipy's Dijkstra on the float32 weights"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    dims = seeds.shape
    n = seeds.size
    step = [(o[0] * dims[1] + o[1]) * dims[2] + o[2] for o in R.OFFSETS]
    rows, cols, data = [], [], []
    for k in range(26):
        v = np.flatnonzero(np.isfinite(W[k]).reshape(-1))
        rows.append(v)
        cols.append(v + step[k])
        data.append(W[k].reshape(-1)[v].astype(np.float64))
    graph = csr_matrix((np.concatenate(data), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    src = np.flatnonzero(seeds.reshape(-1))
    if src.size == 0:
        return np.full(dims, np.inf), np.zeros(dims, dtype=np.int64)
    dist, pred, _ = dijkstra(graph, directed=True, indices=src, return_predecessors=True, min_only=True)
    hops = np.zeros(n, dtype=np.int64)
    for v in np.argsort(dist, kind="stable").tolist():             # a predecessor is nearer: it comes first
        if pred[v] >= 0:
            hops[v] = hops[pred[v]] + 1
    return dist.reshape(dims), hops.reshape(dims)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_float32_field_against_float64(name):
    want = R.field(name)
    worst = 0.0
    for b, r, _, seeds, W in planes(name):
        g64, hops = float64_fields(W, seeds)
        g32 = want[b, r].astype(np.float64)
        assert np.array_equal(np.isinf(g32), np.isinf(g64)), (b, r)
        ok = np.isfinite(g64)
        err = np.abs(g32[ok] - g64[ok])
        bound = hops[ok] * R.U * g64[ok]
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if ok.any() else 0.0)
        assert (err <= bound).all(), (b, r, float(err.max()))
    print(f"{name}: largest error / (hops 2^-24 g) = {worst:.3f}")


def test_gamma_zero_is_the_chamfer_distance():
    name = "euclid_mid"
    c = R.CASES[name]
    assert c["gamma"] == 0.0 and tuple(c["spacing"]) == (1, 1, 1)
    s2, s3 = float(np.sqrt(np.float32(2))), float(np.sqrt(np.float32(3)))
    dims = c["image"].shape[1:]
    grid = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), axis=-1)
    for b, r, _, seeds, _ in planes(name):
        got = R.field(name)[b, r].astype(np.float64)
        if not seeds.any():
            assert np.isinf(got).all()
            continue
        closed = np.full(dims, np.inf)
        hops = np.zeros(dims)
        for p in np.argwhere(seeds):
            delta = np.sort(np.abs(grid - p), axis=-1)             # c <= b <= a
            dist = delta[..., 0] * s3 + (delta[..., 1] - delta[..., 0]) * s2 + (delta[..., 2] - delta[..., 1])
            hops = np.where(dist < closed, delta[..., 2], hops)
            closed = np.minimum(closed, dist)
        assert (np.abs(got - closed) <= hops * R.U * closed).all(), (b, r)


def test_the_serpentine_winds_through_every_gap():
    c = R.CASES["serpentine"]
    img, seeds = c["image"][0], (c["seeds"][0] & 1).astype(bool)
    assert c["gamma"] == 1000.0 and img.shape == (33, 20, 9) and seeds[0, 0, 0] and seeds.sum() == 1
    far = float(R.field("serpentine")[0, 0, -1, -1, -1])
    flat = float(R.dijkstra32(img, seeds, c["spacing"], 0.0)[-1, -1, -1])
    wall = float(np.sqrt(np.float32(1) + np.float32(1000.0) * np.float32(1000.0)))     # one step into a slab
    print(f"serpentine: far corner {far:.3f}, gamma = 0: {flat:.3f}, a wall: {wall:.1f}")
    assert far > 3 * flat
    assert far < wall


def test_nonfinite_voxels_are_never_entered():
    c, f = R.CASES["nonfinite"], R.field("nonfinite")
    shell = np.isnan(c["image"][0])
    inner = np.zeros_like(shell)
    inner[5:8, 4:7, 2:5] = True
    assert shell.sum() == 125 - 27 and not shell[inner].any()
    assert np.isinf(f[0, :, shell]).all()                          # a NaN voxel keeps +inf in both planes
    assert np.isinf(f[0, 0][inner]).all() and np.isfinite(f[0, 0][~inner & ~shell]).all()      # the seed is outside
    assert np.isfinite(f[0, 1][inner]).all() and np.isinf(f[0, 1][~inner]).all()               # the seed is enclosed
    bad = ~np.isfinite(c["image"][1])
    assert bad.sum() == 3 and np.isinf(f[1, 0][bad]).all() and np.isfinite(f[1, 0][~bad]).all()
    assert f[1, 1, 2, 3, 4] == 0 and np.isinf(f[1, 1]).sum() == f[1, 1].size - 1               # a seed on an inf voxel stays alone


def test_seed_union_and_closing_pass_restatements():
    dims = (4, 3, 5)
    mask = np.zeros((2, *dims), dtype=np.uint8)
    mask[0, 1, 1, 1] = 7                                           # only bits 0 and 1 are seeds
    clicks = np.full((2, 3, 4), -1)
    clicks[1, 0] = (3, 2, 4, 1)
    clicks[1, 1] = (0, 0, 0, -1)
    clicks[1, 2] = (1, 1, 1, 0)
    got = R.seed_union(dims, 2, mask, clicks, [0, 7])
    assert got[0, 1, 1, 1] == 3 and got[0].sum() == 3 and got[1, 3, 2, 4] == 2 and got[1, 1, 1, 1] == 1 and got[1].sum() == 3
    field = np.array([0.0, 1.0, 2.0, 3.0, np.inf], dtype=np.float32).reshape(1, 1, 5, 1, 1).repeat(2, 1)
    disk = R.encode_ref(field, kind="disk", radius=2.0, dtype=np.float32)
    assert disk.dtype == np.float32 and disk[0, 0].reshape(-1).tolist() == [1, 1, 1, 0, 0]
    gauss = R.encode_ref(field, kind="gaussian", sigma=1.0)
    assert np.allclose(gauss[0, 0].reshape(-1), np.exp(-np.array([0, 1, 4, 9, np.inf]) / 2)) and gauss[0, 0, 4, 0, 0] == 0


# =============================================================================================
# the host side of the module
# =============================================================================================
def cpu_setup(B=2, dims=(6, 5, 4), cimg=2):
    from mivp_amd import clicks, strokes
    image = torch.rand((B, cimg, *dims))
    out = torch.zeros((B, cimg + 2, *dims))
    return image, out, strokes.StrokeSlot(B, dims, device="cpu"), clicks.ClickSlot(B, dims=dims, device="cpu")


def test_refusals_come_before_any_launch():
    from mivp_amd import clicks, strokes
    g = G()
    image, out, st, ck = cpu_setup()
    dims = tuple(image.shape[2:])
    seeds = torch.zeros((2, *dims), dtype=torch.uint8)
    good = dict(strokes=st, clicks=ck, channel_offset=2, gamma=1.0, spacing=(1, 1, 1))
    bad_images = [image.double(), image[0], image.transpose(3, 4), "image"]
    for im in bad_images:
        with pytest.raises(ValueError, match="image"):
            g.geodesic_distance(im, seeds)
        with pytest.raises(ValueError, match="image"):
            g.encode_geodesic(im, out, **good)
    for ch in (-1, 2, 1.0, True):
        with pytest.raises(ValueError, match="image_channel"):
            g.geodesic_distance(image, seeds, image_channel=ch)
        with pytest.raises(ValueError, match="image_channel"):
            g.encode_geodesic(image, out, **good, image_channel=ch)
    for off in (-1, 3, 1.5):
        with pytest.raises(ValueError, match="channel_offset"):
            g.encode_geodesic(image, out, **{**good, "channel_offset": off})
    with pytest.raises(ValueError, match="out"):
        g.encode_geodesic(image, out[:, :, :5], **good)
    with pytest.raises(ValueError, match="batch"):
        g.encode_geodesic(image, out, **{**good, "strokes": strokes.StrokeSlot(3, dims, device="cpu")})
    with pytest.raises(ValueError, match="volume"):
        g.encode_geodesic(image, out, **{**good, "strokes": strokes.StrokeSlot(2, (6, 5, 5), device="cpu")})
    with pytest.raises(ValueError, match="batch"):
        g.encode_geodesic(image, out, **{**good, "clicks": clicks.ClickSlot(3, device="cpu")})
    with pytest.raises(ValueError, match="volume"):
        g.encode_geodesic(image, out, **{**good, "clicks": clicks.ClickSlot(2, dims=(6, 5, 5), device="cpu")})
    with pytest.raises(ValueError, match="StrokeSlot"):
        g.encode_geodesic(image, out, **{**good, "strokes": ck})
    for gamma in (-1.0, float("nan"), float("inf"), 1e39, None):
        with pytest.raises(ValueError, match="gamma"):
            g.geodesic_distance(image, seeds, gamma=gamma)
        with pytest.raises(ValueError, match="gamma"):
            g.encode_geodesic(image, out, **{**good, "gamma": gamma})
    for spacing in ((1, 1), (1, 0, 1), (1, -1, 1), (1, float("nan"), 1), (1, float("inf"), 1), (1, 1e-30, 1), (1, 1e30, 1)):
        with pytest.raises(ValueError, match="spacing"):
            g.geodesic_distance(image, seeds, spacing=spacing)
        with pytest.raises(ValueError, match="spacing"):
            g.encode_geodesic(image, out, **{**good, "spacing": spacing})
    for n in (-1, 6 * 5 * 4 + 1, 2.0, True):
        with pytest.raises(ValueError, match="max_iter"):
            g.geodesic_distance(image, seeds, max_iter=n)
        with pytest.raises(ValueError, match="max_iter"):
            g.encode_geodesic(image, out, **good, max_iter=n)
    with pytest.raises(ValueError, match="check_every"):
        g.geodesic_distance(image, seeds, check_every=0)
    for s in (seeds[:1], seeds.int(), seeds.transpose(1, 2), None):
        with pytest.raises(ValueError, match="seeds"):
            g.geodesic_distance(image, s)
    for kw in (dict(kind="cone"), dict(box="hollow"), dict(sigma=0.0), dict(kind="disk", radius=-1.0)):
        with pytest.raises(ValueError):
            g.encode_geodesic(image, out, **good, **kw)
    with pytest.raises(ValueError, match="workspace"):
        g.encode_geodesic(image, out, **good, workspace=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="image is out"):
        g.encode_geodesic(out, out, **{**good, "channel_offset": 1}, image_channel=2)
    flat = torch.zeros(out.numel() + image.numel())                # an image that shares memory with out without being out
    shared_out = flat[:out.numel()].view(out.shape)
    for at in (0, 7, out.numel() - 1):
        with pytest.raises(ValueError, match="overlaps"):
            g.encode_geodesic(flat[at:at + image.numel()].view(image.shape), shared_out, **good)
    with pytest.raises(RuntimeError, match="no CPU"):              # right behind it is fine
        g.encode_geodesic(flat[out.numel():].view(image.shape), shared_out, **good)
    # everything in order: the refusal is the one of a CPU tensor
    with pytest.raises(RuntimeError, match="no CPU"):
        g.geodesic_distance(image, seeds)
    with pytest.raises(RuntimeError, match="no CPU"):
        g.encode_geodesic(image, out, **good)


def test_seed_mask_and_workspace_refusals():
    g = G()
    image, out, st, ck = cpu_setup()
    dims = tuple(image.shape[2:])
    with pytest.raises(ValueError, match="batch"):
        g.seed_mask(dims)
    with pytest.raises(ValueError, match="dims"):
        g.seed_mask((6, 5), strokes=st)
    with pytest.raises(ValueError, match="volume"):
        g.seed_mask((6, 5, 5), strokes=st)
    with pytest.raises(ValueError, match="out"):
        g.seed_mask(dims, strokes=st, out=torch.zeros((2, *dims), dtype=torch.int32))
    with pytest.raises(ValueError, match="out"):
        g.seed_mask((3, 3, 3), out=torch.zeros((1, 3, 3, 3), dtype=torch.uint8))      # 27 bytes: no whole words
    with pytest.raises(RuntimeError, match="no CPU"):
        g.seed_mask(dims, strokes=st, clicks=ck)
    for batch, d in ((0, dims), (1, (0, 4, 4)), (1, (65536, 1, 1)), (2, (1024, 1024, 1024)), (65536, (1, 1, 1))):
        with pytest.raises(ValueError):
            g.geodesic_ws(batch, d, device="cpu")
    ws = g.geodesic_ws(2, dims, device="cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == g._Layout(2, dims).size
    assert g.iteration_cap(dims) == 120 and g.iteration_cap((96, 96, 96)) == g.MAX_ITER


def test_geodesic_model_checks_its_arguments():
    from argparse import Namespace
    from mivp_amd import clicks, strokes
    g = G()

    class Stub(torch.nn.Module):
        def __init__(self, cin):
            super().__init__()
            self.conf = Namespace(input_channels=cin)

    st, ck = strokes.StrokeSlot(2, (6, 5, 4), device="cpu"), clicks.ClickSlot(2, device="cpu")
    m = g.GeodesicModel(Stub(3), strokes=st, clicks=ck, gamma=2.0, max_iter=8, kind="disk")
    assert m.image_channels == 1 and m.conf.input_channels == 3 and m.info is None
    for kw in (dict(gamma=-1.0, max_iter=4), dict(gamma=1.0, max_iter=1.5), dict(gamma=1.0, max_iter=4, image_channel=1),
               dict(gamma=1.0, max_iter=4, depth=3), dict(gamma=1.0, max_iter=4, strokes=ck),
               dict(gamma=1.0, max_iter=4, clicks=clicks.ClickSlot(3, device="cpu"), strokes=st)):
        with pytest.raises(ValueError):
            g.GeodesicModel(Stub(3), **kw)
    with pytest.raises(ValueError, match="input_channels"):
        g.GeodesicModel(Stub(2), gamma=1.0, max_iter=4)
    with pytest.raises(ValueError, match="GeodesicModel"):
        g.geodesic_rounds(Stub(3), torch.zeros(1), None, 1)


def test_entries_are_declared_and_the_abi_stays_18():
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    protos = _lib.parse_header()
    for name in ("mivp_geodesic_ws", "mivp_geodesic_seed", "mivp_geodesic_begin", "mivp_geodesic_iter", "mivp_geodesic_end",
                 "mivp_geodesic_encode"):
        assert name in protos, name
    assert protos["mivp_geodesic_ws"][0] is _lib.C.c_size_t
    assert _lib.ABI_VERSION == 18 and "ABI 19" not in text
    import mivp_amd as pkg
    for name in ("GeodesicModel", "GeodesicField", "geodesic_ws", "seed_mask", "geodesic_distance", "encode_geodesic",
                 "geodesic_rounds"):
        assert getattr(pkg, name) is getattr(G(), name)
