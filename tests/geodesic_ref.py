"""The numpy / heapq restatement of the geodesic guidance (mivp_amd.geodesic, csrc/geodesic.hip), and the cases
the host and GPU tests share.

  edge_weights   w(u, u') = sqrt(l2 + (gamma (I(u) - I(u')))^2), l2 = (a_h |dh| + a_w |dw|) + a_d |dd|, a = the float32
                 squared spacings: every step one float32 numpy operation (arrays of float32: the same IEEE operations as
                 float32 scalars, element by element)
  dijkstra32     float32 Dijkstra (heapq): the sum along a path is folded left to right in numpy float32 scalars
  seed_union     the seed mask of a stroke mask and a click record
  encode_ref     the closing pass max(box, f(g)), m = g g, in float32 or float64
  CASES          name -> dict(image f32 [B, H, W, D], seeds u8 [B, H, W, D], gamma, spacing); ``field(name)`` is the
                 restatement's [B, 2, H, W, D] field, computed once per session and never written"""
import functools
import heapq
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import strokes_ref as SR  # noqa: E402

BRICK = (16, 16, 32)
SHAPES = ((13, 10, 7), (16, 16, 12), (33, 20, 9), (17, 17, 33))     # the first is below the brick on every axis, the last one above
DEGENERATE = ((5, 1, 1), (1, 1, 9), (4, 3, 1))
SPACINGS = ((1, 1, 1), (1, 0.5, 2.5), (1, 0.8, 2.5))
OFFSETS = [(dh, dw, dd) for dh in (-1, 0, 1) for dw in (-1, 0, 1) for dd in (-1, 0, 1) if (dh, dw, dd) != (0, 0, 0)]
U = 2.0 ** -24                                                     # the unit roundoff of float32


def spacing_sq(spacing):
    s = np.asarray(spacing, dtype=np.float32)
    return s * s


def _shifted(a, off, fill):
    """b[v] = a[v + off], ``fill`` where v + off is outside the volume."""
    out = np.full(a.shape, fill, dtype=a.dtype)
    src = tuple(slice(max(o, 0), n + min(o, 0)) for o, n in zip(off, a.shape))
    dst = tuple(slice(max(-o, 0), n + min(-o, 0)) for o, n in zip(off, a.shape))
    out[dst] = a[src]
    return out


def edge_weights(image, spacing, gamma):
    """float32 [26, H, W, D]: weight of the edge from v to v + OFFSETS[k]; +inf where that voxel is outside the volume or the
    weight is not finite (such an edge is never taken)."""
    image = np.asarray(image, dtype=np.float32)
    a = spacing_sq(spacing)
    gamma = np.float32(gamma)
    out = np.empty((26, *image.shape), dtype=np.float32)
    inside = np.ones(image.shape, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, off in enumerate(OFFSETS):
            l2 = (a[0] * np.float32(abs(off[0])) + a[1] * np.float32(abs(off[1]))) + a[2] * np.float32(abs(off[2]))
            diff = image - _shifted(image, off, np.float32(0))
            t = gamma * diff
            q = t * t
            s = np.float32(l2) + q
            w = np.sqrt(s)
            assert w.dtype == np.float32
            w[~np.isfinite(w)] = np.inf
            w[~_shifted(inside, off, False)] = np.inf
            out[k] = w
    return out


def dijkstra32(image, seeds, spacing=(1, 1, 1), gamma=1.0, weights=None, with_hops=False):
    """float32 [H, W, D]: g(v) = the smallest left-to-right float32 sum of the weights over the paths from a voxel of the bool
    map ``seeds``; +inf where no path arrives (no seed at all, or enclosed by non-finite voxels)."""
    dims = np.asarray(seeds).shape
    W = edge_weights(image, spacing, gamma) if weights is None else weights
    n = int(np.prod(dims))
    wl = [list(W[k].reshape(-1)) for k in range(26)]                # numpy float32 scalars
    fin = [np.isfinite(W[k]).reshape(-1).tolist() for k in range(26)]
    step = [(off[0] * dims[1] + off[1]) * dims[2] + off[2] for off in OFFSETS]
    inf = np.float32(np.inf)
    dist = [inf] * n
    hops = [0] * n
    done = [False] * n
    heap = []
    for v in np.flatnonzero(np.asarray(seeds).reshape(-1)).tolist():
        dist[v] = np.float32(0)
        heap.append((0.0, v))
    heapq.heapify(heap)
    while heap:
        _, v = heapq.heappop(heap)
        if done[v]:
            continue
        done[v] = True
        dv = dist[v]
        for k in range(26):
            if not fin[k][v]:
                continue
            u = v + step[k]
            nd = dv + wl[k][v]                                     # one float32 addition
            if nd < dist[u]:
                dist[u] = nd
                hops[u] = hops[v] + 1
                heapq.heappush(heap, (float(nd), u))
    g = np.asarray(dist, dtype=np.float32).reshape(dims)
    return (g, np.asarray(hops).reshape(dims)) if with_hops else g


def relax_all(g, W):
    """One Jacobi round on the whole volume: min(g, min_k (g[v + off_k] + W[k][v])), float32."""
    best = g.copy()
    for k, off in enumerate(OFFSETS):
        np.minimum(best, _shifted(g, off, np.float32(np.inf)) + W[k], out=best)
    return best


def seed_union(dims, batch, stroke_mask=None, clicks=None, count=None):
    """uint8 [B, H, W, D]: bits 0 / 1 of the stroke mask | the clicks (int [B, K, 4], the first clamp(count, 0, K) rows; a row
    whose channel is not 0 / 1 is skipped)."""
    out = np.zeros((batch, *dims), dtype=np.uint8)
    if stroke_mask is not None:
        out |= np.asarray(stroke_mask, dtype=np.uint8) & 3
    if clicks is not None:
        clicks = np.asarray(clicks)
        for b in range(batch):
            for h, w, d, ch in clicks[b, :min(max(int(count[b]), 0), clicks.shape[1])].tolist():
                if ch in (0, 1):
                    out[b, h, w, d] |= 1 << ch
    return out


def fields_ref(image, seeds, spacing, gamma):
    """float32 [B, 2, H, W, D] by dijkstra32."""
    image, seeds = np.asarray(image), np.asarray(seeds)
    out = np.empty((image.shape[0], 2, *image.shape[1:]), dtype=np.float32)
    for b in range(image.shape[0]):
        W = edge_weights(image[b], spacing, gamma)
        for r in range(2):
            out[b, r] = dijkstra32(image[b], (seeds[b] >> r) & 1, weights=W)
    return out


def encode_ref(field, boxes=None, count=None, box="filled", kind="gaussian", radius=2.0, sigma=2.0, dtype=np.float64):
    """[B, 2, H, W, D] of ``dtype``: max(box, f(g)), m = g g, from the float32 ``field``, every step in ``dtype``."""
    field = np.asarray(field)
    g = field.astype(dtype)
    with np.errstate(over="ignore"):
        m = (g * g).astype(dtype)
    val = SR.stroke_value(m, kind, radius, sigma, dtype)
    if boxes is not None:
        val = np.maximum(SR.box_ref(boxes, count, field.shape[2:], box).astype(dtype), val)
    return val


# ------------------------------------------------------------------------------------------------------------- images
def ramp(dims, seed=0):
    h, w, d = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in dims], indexing="ij")
    c = np.random.default_rng(seed).random(3).astype(np.float32)
    return ((c[0] * h + c[1] * w + c[2] * d) / np.float32(sum(dims))).astype(np.float32)


def blocky(dims, seed=0):
    """random values on a 1/16 grid, constant on 3 x 2 x 2 blocks"""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 17, size=[(n + 1) // 2 + 1 for n in dims]).astype(np.float32) / np.float32(16)
    big = small.repeat(3, 0).repeat(2, 1).repeat(2, 2)
    return np.ascontiguousarray(big[:dims[0], :dims[1], :dims[2]])


def blobs(dims, seed=0):
    """two blobs of value 1 and 0.5 with a sharp edge on a dark ground"""
    h, w, d = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dims], indexing="ij")
    rng = np.random.default_rng(seed)
    img = np.zeros(dims, dtype=np.float32)
    for value in (1.0, 0.5):
        c = rng.random(3) * np.asarray(dims)
        r = 0.3 * max(dims)
        img[(h - c[0]) ** 2 + (w - c[1]) ** 2 + (d - c[2]) ** 2 <= r * r] = value
    return img


def serpentine(dims):
    """zero, except slabs h = 3, 7, 11, .. of value 1 over all (w, d) with a one-column gap alternating between w = 0 and w = W - 1"""
    img = np.zeros(dims, dtype=np.float32)
    for i, h in enumerate(range(3, dims[0], 4)):
        img[h] = 1
        img[h, 0 if i % 2 == 0 else dims[1] - 1] = 0
    return img


def _seeds(dims, rows):
    """rows: per sample [(h, w, d, bit), ...]; negative coordinates count from the end"""
    out = np.zeros((len(rows), *dims), dtype=np.uint8)
    for b, pts in enumerate(rows):
        for h, w, d, bit in pts:
            out[b, h, w, d] |= 1 << bit
    return out


def _random_seeds(dims, seed, n):
    rng = np.random.default_rng(seed)
    return [(*[int(rng.integers(0, s)) for s in dims], i % 2) for i in range(n)]


def _cases():
    C = {}

    def add(name, image, seeds, gamma, spacing=(1, 1, 1)):
        C[name] = dict(image=np.ascontiguousarray(np.stack(image), dtype=np.float32), seeds=seeds, gamma=gamma, spacing=spacing)

    d = SHAPES[0]
    # seeds at the first and at the last voxel; a plane without seeds; a seed on every voxel
    every = np.zeros((3, *d), dtype=np.uint8)
    every[0, 0, 0, 0] = 1
    every[0, -1, -1, -1] = 2
    every[1] = 1
    every[2] = _seeds(d, [_random_seeds(d, 3, 4)])[0] & 1
    add("ramp_small", [ramp(d, 1), ramp(d, 2), blobs(d, 3)], every, 1.0)
    add("blobs_small_aniso", [blobs(d, 4), blocky(d, 5)], _seeds(d, [_random_seeds(d, 6, 3), _random_seeds(d, 7, 2)]), 1000.0,
        (1, 0.5, 2.5))
    small = serpentine(d)
    add("serpentine_small", [small, small[:, ::-1].copy()], _seeds(d, [[(0, 0, 0, 0)], [(0, 0, 0, 0), (-1, -1, -1, 1)]]),
        1000.0)
    d = SHAPES[1]
    add("blocky_mid_aniso", [blocky(d, 8), blocky(d, 9), ramp(d, 10)],
        _seeds(d, [_random_seeds(d, 11, 4), _random_seeds(d, 12, 1), _random_seeds(d, 13, 6)]), 30.0, (1, 0.8, 2.5))
    add("euclid_mid", [blocky(d, 14), blobs(d, 15)], _seeds(d, [_random_seeds(d, 16, 3), [(0, 0, 0, 0), (-1, -1, -1, 0)]]), 0.0)
    d = SHAPES[2]
    add("serpentine", [serpentine(d), serpentine(d) + np.float32(0.25) * blocky(d, 17)],
        _seeds(d, [[(0, 0, 0, 0)], [(0, 0, 0, 0), (-1, -1, -1, 1)]]), 1000.0)
    add("blobs_long", [blobs(d, 18), blobs(d, 19)], _seeds(d, [_random_seeds(d, 20, 5), _random_seeds(d, 21, 2)]), 30.0, (1, 0.5, 2.5))
    d = SHAPES[3]
    add("blocky_over_brick", [blocky(d, 22), ramp(d, 23)], _seeds(d, [[(0, 0, 0, 0), (-1, -1, -1, 1)], _random_seeds(d, 24, 3)]), 1.0)
    for i, d in enumerate(DEGENERATE):
        add(f"degenerate_{d[0]}x{d[1]}x{d[2]}", [blocky(d, 25 + i), ramp(d, 28 + i)],
            _seeds(d, [[(0, 0, 0, 0), (-1, -1, -1, 1)], [(-1, -1, -1, 0)]]), (1.0, 30.0, 1000.0)[i], SPACINGS[i])
    # NaN and inf voxels: a shell of them around (6, 5, 3) of sample 0, scattered ones in sample 1
    d = SHAPES[0]
    shell = blocky(d, 31)
    shell[4:9, 3:8, 1:6] = np.nan
    shell[5:8, 4:7, 2:5] = 0.5
    loose = ramp(d, 32)
    loose[2, 3, 4] = np.inf
    loose[7, 7, 2] = -np.inf
    loose[9, 1, 1] = np.nan
    add("nonfinite", [shell, loose], _seeds(d, [[(0, 0, 0, 0), (6, 5, 3, 1)], [(0, 0, 0, 0), (2, 3, 4, 1)]]), 1.0)
    return C


CASES = _cases()


@functools.lru_cache(maxsize=None)
def field(name):
    c = CASES[name]
    out = fields_ref(c["image"], c["seeds"], c["spacing"], c["gamma"])
    out.setflags(write=False)
    return out
