"""numpy / Python restatement of the shape descriptors of mivp_amd.regions.region_shape for the tests.  It
does not import the package.

``shape_stats(labels, n, spacing)`` takes a dense label map (values 0..n, as ``region_stats`` writes it) and builds, per
region, the cells of its closed cubical complex literally: every voxel (h, w, d) is the cube centred at the doubled
coordinates (2h + 1, 2w + 1, 2d + 1), and its 27 cells are the points centre + (i, j, k), i, j, k in {-1, 0, 1}: a vertex has
no zero offset, an edge one, a face two, the cube itself three.  The sets of distinct vertices, edges and faces give V, E, F
and the Euler number V - E + F - size.  Moments are Python integers, so nothing can wrap.

``components_tunnels_cavities`` counts, by flood fill, the 26-connected components of a binary shape and the cavities (the
6-connected background components that do not reach the border of the shape padded by one voxel)."""
import itertools
from fractions import Fraction

import numpy as np

OFFSETS = list(itertools.product((-1, 0, 1), repeat=3))
PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))          # h*h, w*w, d*d, h*w, h*d, w*d


def shape_stats(labels, n, spacing=(1.0, 1.0, 1.0), capacity=None):
    """-> dict of per-region arrays for the regions 1..min(n, capacity): size, coord_sum, moment2, faces, cells, euler (int64),
    numerator (Python integers [6]: n M_ab - S_a S_b in the order of PAIRS), covariance_mm2 (float64 [3, 3], formed from the
    numerator by one conversion, one division by float(n * n) and one multiplication by spacing_a * spacing_b)."""
    labels = np.asarray(labels)
    m = n if capacity is None else min(n, capacity)
    shape = labels.shape
    verts = [set() for _ in range(m)]
    edges = [set() for _ in range(m)]
    faces_all = [set() for _ in range(m)]
    size = [0] * m
    csum = [[0, 0, 0] for _ in range(m)]
    mom = [[0] * 6 for _ in range(m)]
    exposed = [[0, 0, 0] for _ in range(m)]
    for h, w, d in zip(*(a.tolist() for a in np.nonzero(labels))):
        lab = int(labels[h, w, d])
        if lab < 1 or lab > m:
            continue
        r = lab - 1
        c = (h, w, d)
        size[r] += 1
        for a in range(3):
            csum[r][a] += c[a]
        for k, (a, b) in enumerate(PAIRS):
            mom[r][k] += c[a] * c[b]
        for off in OFFSETS:
            cell = (2 * h + 1 + off[0], 2 * w + 1 + off[1], 2 * d + 1 + off[2])
            zeros = off.count(0)
            if zeros == 0:
                verts[r].add(cell)
            elif zeros == 1:
                edges[r].add(cell)
            elif zeros == 2:
                faces_all[r].add(cell)
        for a in range(3):
            for side in (-1, 1):
                q = list(c)
                q[a] += side
                outside = q[a] < 0 or q[a] >= shape[a]
                if outside or int(labels[q[0], q[1], q[2]]) != lab:
                    exposed[r][a] += 1
    cells = [[len(verts[r]), len(edges[r])] for r in range(m)]
    nfaces = [len(faces_all[r]) for r in range(m)]
    for r in range(m):                                   # the identity the package uses for F
        assert 2 * nfaces[r] == 6 * size[r] + sum(exposed[r])
    euler = [cells[r][0] - cells[r][1] + nfaces[r] - size[r] for r in range(m)]
    numerator = [[size[r] * mom[r][k] - csum[r][a] * csum[r][b] for k, (a, b) in enumerate(PAIRS)] for r in range(m)]
    sp = [float(s) for s in spacing]
    cov = np.zeros((m, 3, 3), dtype=np.float64)
    for r in range(m):
        for k, (a, b) in enumerate(PAIRS):
            v = np.float64(float(numerator[r][k])) / np.float64(float(size[r] * size[r])) * np.float64(sp[a] * sp[b])
            cov[r, a, b] = cov[r, b, a] = v
    return dict(n=m, size=np.array(size, dtype=np.int64).reshape(m), coord_sum=np.array(csum, dtype=np.int64).reshape(m, 3),
                moment2=np.array(mom, dtype=np.int64).reshape(m, 6), faces=np.array(exposed, dtype=np.int64).reshape(m, 3),
                cells=np.array(cells, dtype=np.int64).reshape(m, 2), euler=np.array(euler, dtype=np.int64).reshape(m),
                n_faces=np.array(nfaces, dtype=np.int64).reshape(m), numerator=numerator, covariance_mm2=cov)


def exact_covariance(numerator, size, spacing):
    """The covariance as exact rationals [6] (order of PAIRS), the spacings taken as the float64 values they are."""
    sp = [Fraction(float(s)) for s in spacing]
    return [Fraction(numerator[k], size * size) * sp[a] * sp[b] for k, (a, b) in enumerate(PAIRS)]


def _flood(mask, neighbours):
    """number of connected components of a boolean array under the given neighbour offsets, and their label map"""
    lab = np.zeros(mask.shape, dtype=np.int64)
    count = 0
    for start in zip(*(a.tolist() for a in np.nonzero(mask))):
        if lab[start]:
            continue
        count += 1
        lab[start] = count
        stack = [start]
        while stack:
            p = stack.pop()
            for o in neighbours:
                q = (p[0] + o[0], p[1] + o[1], p[2] + o[2])
                if all(0 <= q[a] < mask.shape[a] for a in range(3)) and mask[q] and not lab[q]:
                    lab[q] = count
                    stack.append(q)
    return count, lab


N26 = [o for o in OFFSETS if o != (0, 0, 0)]
N6 = [o for o in OFFSETS if sum(abs(a) for a in o) == 1]


def components_and_cavities(mask):
    """(26-connected components of the shape, 6-connected background components enclosed by it)."""
    mask = np.pad(np.asarray(mask, dtype=bool), 1)
    comps, _ = _flood(mask, N26)
    bg, _ = _flood(~mask, N6)
    return comps, bg - 1                                 # the padding joins everything that reaches the border


def ulp_distance(got, want):
    """|got - want| in units of the spacing of float64 at `want` (0 where both are equal, zeros included)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.where(got == want, 0.0, np.abs(got - want) / np.spacing(np.abs(want)))


# ---------------------------------------------------------------------------------------------------- the hand-made shapes
def single_voxel():
    x = np.zeros((3, 3, 3), dtype=np.int32)
    x[1, 1, 1] = 1
    return x


def box(a, b, c, at=(1, 2, 3), pad=2):
    x = np.zeros((at[0] + a + pad, at[1] + b + pad, at[2] + c + pad), dtype=np.int32)
    x[at[0]:at[0] + a, at[1]:at[1] + b, at[2]:at[2] + c] = 1
    return x


def square_ring():
    """a 3 x 3 ring of voxels in one h-plane: one tunnel"""
    x = np.zeros((3, 5, 5), dtype=np.int32)
    x[1, 1:4, 1:4] = 1
    x[1, 2, 2] = 0
    return x


def hollow_cube():
    """a 5^3 cube with a one-voxel cavity"""
    x = np.zeros((7, 7, 7), dtype=np.int32)
    x[1:6, 1:6, 1:6] = 1
    x[3, 3, 3] = 0
    return x


def vertex_pair():
    """two 2^3 cubes that share one vertex only: one 26-connected region"""
    x = np.zeros((6, 6, 6), dtype=np.int32)
    x[1:3, 1:3, 1:3] = 1
    x[3:5, 3:5, 3:5] = 1
    return x


def place(shape_map, volume_shape, corner):
    """the hand-made shape (its zero border cut off) put into a zero volume so that its bounding box is centred on the
    voxel corner `corner` (a brick corner of the kernel: the shape then lies in all eight bricks that meet there)"""
    idx = np.nonzero(shape_map)
    lo = [int(a.min()) for a in idx]
    hi = [int(a.max()) + 1 for a in idx]
    cut = shape_map[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    out = np.zeros(volume_shape, dtype=shape_map.dtype)
    at = [corner[a] - cut.shape[a] // 2 for a in range(3)]
    out[at[0]:at[0] + cut.shape[0], at[1]:at[1] + cut.shape[1], at[2]:at[2] + cut.shape[2]] = cut
    return out
