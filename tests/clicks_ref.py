"""A numpy restatement of the click encoding and the click simulation (mivp_amd.clicks, csrc/clicks.hip), and the cases the
host and the GPU tests share.  Nothing here imports the package: the restatement is the definition, written a second time.

Simulation.  Per sample, E_pos = {target in the object, pred not}, E_neg = {pred in the object, target a class outside it};
depth^2(v) = the squared Euclidean transform of the region's mask padded by one voxel of background, in mm; the click is the
voxel of the largest float32 depth^2, ties to E_pos, then to the lowest raster index."""
import numpy as np

MAX_CLASSES = 32
DEFAULT_MASK = 0xFFFFFFFE


def spacing_sq(spacing):
    """The squared spacings as the kernels form them: a float32 product, then widened."""
    s = np.asarray(spacing, dtype=np.float32)
    return (s * s).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ encoding
def encode_ref(clicks, count, dims, spacing=(1, 1, 1), kind="gaussian", sigma=2.0, radius=2.0, dtype=np.float64):
    """[B, 2, H, W, D] of ``dtype``: the composition min over clicks -> exp(-m / (2 sigma^2)) or m <= radius^2, every step in
    ``dtype`` (float32: the formula as a float32 program; float64: the yardstick)."""
    clicks, count = np.asarray(clicks), np.asarray(count)
    B, K = clicks.shape[:2]
    H, W, D = dims
    a = spacing_sq(spacing).astype(dtype)
    hh, ww, dd = np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing="ij")
    out = np.zeros((B, 2, H, W, D), dtype=dtype)
    for b in range(B):
        for ch in range(2):
            m = np.full((H, W, D), np.inf, dtype=dtype)
            for i in range(min(max(int(count[b]), 0), K)):
                h, w, d, c = (int(v) for v in clicks[b, i])
                if c != ch:
                    continue
                dist = (a[0] * ((hh - h).astype(dtype) ** 2) + a[1] * ((ww - w).astype(dtype) ** 2)) \
                    + a[2] * ((dd - d).astype(dtype) ** 2)
                m = np.minimum(m, dist.astype(dtype))
            if kind == "gaussian":
                out[b, ch] = np.exp(-m / dtype(np.float32(2.0 * sigma * sigma)))
            else:
                out[b, ch] = (m <= dtype(np.float32(radius * radius))).astype(dtype)
    return out


# ---------------------------------------------------------------------------------------------------------- simulation
def classes_of(a):
    """Class 0 .. 31 of every element, -1 for anything else (negative, too large, a half-integer, NaN)."""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            ok = (a >= 0) & (a < MAX_CLASSES) & (a == np.floor(a))
        return np.where(ok, np.where(ok, a, 0), -1).astype(np.int64)
    a = a.astype(np.int64)
    return np.where((a >= 0) & (a < MAX_CLASSES), a, -1)


def error_regions(pred, target, mask=DEFAULT_MASK, ignore_index=None):
    """(E_pos, E_neg) as bool arrays."""
    p, t = classes_of(pred), classes_of(target)
    valid = t >= 0
    if ignore_index is not None:
        valid &= t != ignore_index
    bit = np.array([(mask >> c) & 1 for c in range(MAX_CLASSES)], dtype=bool)
    tin = valid & bit[np.maximum(t, 0)]
    pin = (p >= 0) & bit[np.maximum(p, 0)]
    return valid & tin & ~pin, valid & pin & ~tin


def _axis_pass(f, a, axis):
    f = np.moveaxis(f, axis, -1)
    n = f.shape[-1]
    x = np.arange(n, dtype=np.float64)
    cost = a * (x[:, None] - x[None, :]) ** 2                      # [x][i]
    out = (f[..., None, :] + cost).min(axis=-1)
    return np.moveaxis(out, -1, axis)


def depth_sq(region, spacing=(1, 1, 1)):
    """float64 [H, W, D]: inside the region the squared distance in mm to the nearest voxel outside it, the outside of the
    volume counting as outside (the exact separable transform of the mask padded by one voxel); 0 outside the region."""
    a = spacing_sq(spacing)
    f = np.where(np.pad(region, 1), np.inf, 0.0)
    for axis in range(3):
        f = _axis_pass(f, a[axis], axis)
    return f[1:-1, 1:-1, 1:-1]


def pick(d_pos, d_neg):
    """(float32 depth^2, channel, raster index) of the winner, or None without a region."""
    best = None
    for ch, d in ((0, d_pos), (1, d_neg)):
        d32 = d.astype(np.float32).reshape(-1)
        if not (d32 > 0).any():
            continue
        top = d32.max()
        idx = int(np.flatnonzero(d32 == top)[0])                   # the lowest raster index
        if best is None or top > best[0]:                          # a tie keeps the positive region
            best = (top, ch, idx)
    return best


def simulate_ref(pred, target, clicks, count, spacing=(1, 1, 1), object_classes=None, ignore_index=None, min_depth=0.0):
    """New (clicks, count, last) after one simulated click per sample."""
    clicks, count = np.array(clicks, dtype=np.int32), np.array(count, dtype=np.int32)
    B, K = clicks.shape[:2]
    pred, target = np.asarray(pred), np.asarray(target)
    pred = pred[:, 0] if pred.ndim == 5 else pred
    target = target[:, 0] if target.ndim == 5 else target
    H, W, D = pred.shape[1:]
    mask = DEFAULT_MASK if object_classes is None else sum(1 << int(c) for c in object_classes)
    last = np.zeros((B, 4), dtype=np.int32)
    md2 = np.float32(float(min_depth) * float(min_depth))
    for b in range(B):
        e_pos, e_neg = error_regions(pred[b], target[b], mask, ignore_index)
        win = pick(depth_sq(e_pos, spacing), depth_sq(e_neg, spacing))
        if win is None:
            last[b] = (0, -1, -1, 0)
            continue
        top, ch, idx = win
        placed = bool(top >= md2) and 0 <= count[b] < K
        if placed:
            clicks[b, count[b]] = (idx // (W * D), (idx // D) % W, idx % D, ch)
            count[b] += 1
        last[b] = (int(np.float32(top).view(np.int32)), ch, idx, int(placed))
    return clicks, count, last


def is_exact(pred, target, spacing=(1, 1, 1), object_classes=None, ignore_index=None):
    """True when every depth^2 of the case is a float32 number: no comparison is then left to rounding, and the stated tie
    rule (region, then raster index) decides every tie there is."""
    mask = DEFAULT_MASK if object_classes is None else sum(1 << int(c) for c in object_classes)
    for b in range(pred.shape[0]):
        for d in (depth_sq(r, spacing) for r in error_regions(pred[b], target[b], mask, ignore_index)):
            if not np.array_equal(d.astype(np.float32).astype(np.float64), d):
                return False
    return True


# -------------------------------------------------------------------------------------------------------------- cases
SHAPES = ((13, 10, 7), (16, 16, 12), (33, 20, 9))
EXACT_SPACING = (1.0, 0.5, 2.5)                # squares 1, 0.25, 6.25: every sum of their integer multiples is a float32 number


def blobs(rng, dims, classes=3, cell=3):
    """A blocky random class map with a little voxel noise: regions of every size, many equal depths."""
    coarse = rng.integers(0, classes, size=[-(-n // cell) for n in dims])
    m = np.kron(coarse, np.ones((cell, cell, cell), dtype=np.int64))[:dims[0], :dims[1], :dims[2]]
    noise = rng.random(dims) < 0.03
    return np.where(noise, rng.integers(0, classes, size=dims), m)


def _box(dims, lo, hi, value=1):
    m = np.zeros(dims, dtype=np.int64)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = value
    return m


def _ball(dims, centre, r):
    g = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    return (sum((g[a] - centre[a]) ** 2 for a in range(3)) <= r * r).astype(np.int64)


def simulate_cases():
    """name -> dict(pred, target [B, H, W, D], dtype names, K, init clicks per sample, kwargs, want: the expected
    (h, w, d, channel) of sample 0 or None).  Sample 1 of every case is another error, so the samples are told apart."""
    rng = np.random.default_rng(20)
    cases = {}

    def add(name, dims, pred0, target0, want, pdt="uint8", tdt="uint8", K=4, init=None, **kwargs):
        p1, t1 = blobs(rng, dims), blobs(rng, dims)
        cases[name] = dict(pred=np.stack([pred0, p1]).astype(pdt), target=np.stack([target0, t1]).astype(tdt), K=K,
                           init=init or [[], []], kwargs=kwargs, want=want)

    d1, d2 = SHAPES[1], SHAPES[0]
    zero = np.zeros(d1, dtype=np.int64)
    add("ball", d1, zero, _ball(d1, (8, 8, 6), 4), (8, 8, 6, 0))
    # the negative cube comes first in raster order and is as deep: the positive one wins
    add("tie_regions", d1, _box(d1, (2, 2, 2), (5, 5, 5)), _box(d1, (9, 9, 6), (12, 12, 9)), (10, 10, 7, 0), pdt="int32")
    add("tie_index", d1, zero, _box(d1, (5, 6, 7), (7, 8, 9)), (5, 6, 7, 0), tdt="int64")
    same = blobs(rng, d1)
    add("no_error", d1, same, same, None, pdt="int64", tdt="float32")
    add("full_slot", d1, zero, _ball(d1, (8, 8, 6), 4), None, K=2, init=[[(1, 1, 1, 0), (2, 2, 2, 1)], [(3, 3, 3, 1)]])
    # without the border rule the deepest voxels of the slab would be those on the face h = 0
    add("face_slab", d2, np.zeros(d2, dtype=np.int64), _box(d2, (0, 0, 0), (4, 10, 7)), (1, 1, 1, 0))
    add("whole_volume", d2, np.zeros(d2, dtype=np.int64), np.ones(d2, dtype=np.int64), (3, 3, 3, 0), tdt="float32")
    add("anisotropic", SHAPES[2], blobs(rng, SHAPES[2]), blobs(rng, SHAPES[2]), "any", spacing=EXACT_SPACING)
    split = _box(d1, (3, 4, 4), (10, 9, 9))
    split[6] = np.where(split[6] > 0, 2, 0)                        # the plane h = 6 of the box is ignored
    add("ignored_split", d1, zero, split, (4, 5, 5, 0), ignore_index=2)     # whole, the box would be clicked at (6, 6, 6)
    add("min_depth", d1, zero, _box(d1, (5, 6, 7), (7, 8, 9)), None, min_depth=2.0)
    add("object_classes", d2, blobs(rng, d2), blobs(rng, d2), "any", object_classes=(2,), pdt="float32", tdt="int32")
    for i, dims in enumerate(SHAPES):
        add(f"random{i}", dims, blobs(rng, dims), blobs(rng, dims), "any", pdt=("uint8", "int32", "float32")[i],
            tdt=("float32", "uint8", "int64")[i])
    # a float map with values that are no class: a half-integer, a negative one, one too large, a NaN
    odd = blobs(rng, d2).astype(np.float32)
    odd[2, 3, 4], odd[5, 5, 5], odd[7, 2, 1], odd[9, 9, 6] = 1.5, -1.0, 40.0, np.nan
    cases["no_class"] = dict(pred=np.stack([blobs(rng, d2), blobs(rng, d2)]).astype("float32"),
                             target=np.stack([odd, blobs(rng, d2).astype(np.float32)]), K=4, init=[[], []], kwargs={},
                             want="any")
    return cases
