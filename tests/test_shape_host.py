"""CPU: the restatement of the shape descriptors (tests/shape_ref.py) on shapes whose answers are written out, the identity
chi = components - tunnels + cavities on them, the host checks of mivp_amd.regions.region_shape and the C ABI declarations
of the two entry points (they joined ABI 18 without a bump)."""
import inspect
import os
import re
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shape_ref as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mivp_region_shape", "mivp_region_axes")


def _one(x, spacing=(1.0, 1.0, 1.0)):
    r = S.shape_stats(x, 1, spacing)
    assert r["n"] == 1
    return r


# ------------------------------------------------------------------------------------------- the restatement, by hand
def test_single_voxel():
    r = _one(S.single_voxel())
    assert r["faces"].tolist() == [[2, 2, 2]] and r["cells"].tolist() == [[8, 12]]
    assert r["n_faces"].tolist() == [6] and r["euler"].tolist() == [1]
    assert r["moment2"].tolist() == [[1, 1, 1, 1, 1, 1]]
    assert r["numerator"] == [[0] * 6] and not r["covariance_mm2"].any()


@pytest.mark.parametrize("abc", [(2, 3, 4), (5, 1, 1), (1, 4, 6), (3, 3, 3)])
def test_box(abc):
    a, b, c = abc
    sp = (0.7, 0.7, 2.5)
    r = _one(S.box(a, b, c), sp)
    assert r["size"].tolist() == [a * b * c] and r["euler"].tolist() == [1]
    assert r["faces"].tolist() == [[2 * b * c, 2 * a * c, 2 * a * b]]
    assert r["cells"].tolist() == [[(a + 1) * (b + 1) * (c + 1),
                                    a * (b + 1) * (c + 1) + (a + 1) * b * (c + 1) + (a + 1) * (b + 1) * c]]
    area = 2 * b * c * sp[1] * sp[2] + 2 * a * c * sp[0] * sp[2] + 2 * a * b * sp[0] * sp[1]
    got_area = sum(float(r["faces"][0, i]) * sp[(i + 1) % 3] * sp[(i + 2) % 3] for i in range(3))
    assert got_area == pytest.approx(area, rel=1e-15)
    # the variance of k consecutive integers is (k^2 - 1) / 12, and a box has no cross terms
    exact = S.exact_covariance(r["numerator"][0], a * b * c, sp)
    want = [Fraction(k * k - 1, 12) * Fraction(s) ** 2 for k, s in zip(abc, sp)]
    assert exact[:3] == want and exact[3:] == [0, 0, 0]
    cov = r["covariance_mm2"][0]
    assert np.all(S.ulp_distance(np.diag(cov), [float(v) for v in want]) <= 2)
    assert not (cov - np.diag(np.diag(cov))).any()
    for k, flat in enumerate(abc):
        if flat == 1:                                   # flat along an axis: exact zeros in that row and column
            assert not cov[k].any() and not cov[:, k].any()


def test_ring_cavity_and_vertex_pair():
    assert _one(S.square_ring())["euler"].tolist() == [0]
    assert _one(S.hollow_cube())["euler"].tolist() == [2]
    pair = _one(S.vertex_pair())
    assert pair["euler"].tolist() == [1]
    assert pair["cells"][0, 0] == 2 * 27 - 1 and pair["cells"][0, 1] == 2 * 54 and pair["n_faces"][0] == 2 * 36
    ring = _one(S.square_ring())
    assert ring["faces"].tolist() == [[16, 8, 8]] and ring["size"].tolist() == [8]
    hollow = _one(S.hollow_cube())
    assert hollow["faces"].tolist() == [[52, 52, 52]] and hollow["size"].tolist() == [124]


@pytest.mark.parametrize("make,tunnels", [(S.single_voxel, 0), (lambda: S.box(2, 3, 4), 0), (S.square_ring, 1),
                                          (S.hollow_cube, 0), (S.vertex_pair, 0)])
def test_euler_identity(make, tunnels):
    x = make()
    comps, cavities = S.components_and_cavities(x > 0)
    assert _one(x)["euler"][0] == comps - tunnels + cavities
    assert comps == 1 and cavities == (1 if make is S.hollow_cube else 0)


def test_two_regions_and_capacity():
    x = np.zeros((4, 4, 8), dtype=np.int32)
    x[0, 0, 0] = 1
    x[1, 1, 1] = 2                                      # shares a vertex with region 1: another label, so all faces show
    x[2:4, 2:4, 4:8] = 3
    r = S.shape_stats(x, 3)
    assert r["faces"].tolist() == [[2, 2, 2], [2, 2, 2], [16, 16, 8]]
    assert r["cells"].tolist() == [[8, 12], [8, 12], [3 * 3 * 5, 2 * 3 * 5 + 3 * 2 * 5 + 3 * 3 * 4]]
    assert r["euler"].tolist() == [1, 1, 1]
    # the 2 x 2 x 4 box at h, w in {2, 3}, d in 4..7
    assert r["moment2"][2].tolist() == [8 * (4 + 9), 8 * (4 + 9), 4 * (16 + 25 + 36 + 49), 4 * 5 * 5, 2 * 5 * 22, 2 * 5 * 22]
    two = S.shape_stats(x, 3, capacity=2)               # labels above the capacity are skipped
    assert two["n"] == 2 and two["faces"].tolist() == [[2, 2, 2], [2, 2, 2]]


# ------------------------------------------------------------------------------------------- host checks
def _fake_table(dims, labels="match"):
    import torch
    if labels == "match":
        labels = torch.zeros(tuple(min(d, 4) for d in dims), dtype=torch.int32)
    return types.SimpleNamespace(dims=dims, labels=labels, max_regions=8, spacing=(1.0, 1.0, 1.0))


def test_rejected_tables():
    import torch
    import mivp_amd  # noqa: F401
    from mivp_amd import regions as G
    assert G.MAX_SHAPE_DIM == 65535
    with pytest.raises(ValueError, match="label map"):
        G.region_shape(_fake_table((4, 4, 4), labels=None))
    with pytest.raises(ValueError, match="label map"):
        G._check_shape_table(types.SimpleNamespace(dims=(4, 4, 4)))
    for dims in ((65536, 1, 1), (1, 65536, 2), (2, 2, 65536)):
        t = _fake_table(dims)
        t.labels = types.SimpleNamespace(shape=dims, dtype=torch.int32)          # (nothing that large is allocated)
        with pytest.raises(ValueError, match="65535"):
            G.region_shape(t)
    ok = _fake_table((2, 2, 65535))
    ok.labels = types.SimpleNamespace(shape=(2, 2, 65535), dtype=torch.int32)
    assert G._check_shape_table(ok) == (2, 2, 65535)
    with pytest.raises(ValueError, match="int32"):
        G._check_shape_table(_fake_table((4, 4, 4), labels=torch.zeros((4, 4, 4), dtype=torch.int64)))
    with pytest.raises(ValueError, match="int32"):
        G._check_shape_table(_fake_table((4, 4, 4), labels=torch.zeros((4, 4, 5), dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="GPU"):      # a host label map gets as far as the device check
        G.region_shape(_fake_table((4, 4, 4)))
    for name in ("region_shape", "RegionShape"):
        assert getattr(mivp_amd, name) is getattr(G, name)


def test_public_surface_is_additive():
    import mivp_amd  # noqa: F401
    from mivp_amd import regions as G
    assert list(inspect.signature(G.region_shape).parameters) == ["table"]
    assert G.REGION_KWARGS == ("connectivity", "classes", "max_regions")
    assert G.LESION_KWARGS == ("connectivity", "iou_threshold", "min_size", "classes", "max_regions", "max_pairs")
    for name in ("euler", "major_axis_length", "minor_axis_length", "least_axis_length", "elongation", "flatness",
                 "surface_area_mm2", "surface_to_volume", "sphericity"):
        assert isinstance(getattr(G.RegionShape, name), property), name
    doc = G.__doc__
    for words in ("union of closed voxels", "26-connectivity", "voxel-face area", "2/3", "Feret"):
        assert words in doc, words


# ------------------------------------------------------------------------------------------- C ABI
def test_header_declares_shape_symbols_within_abi_18():
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib
    text = open(os.path.join(ROOT, "include", "mivp.h")).read()
    names = set(re.findall(r"\b(mivp_[a-z0-9_]+)\s*\(", text))
    for n in SYMBOLS:
        assert n in names, n
    assert "ABI 18" in text and "ABI 19" not in text
    assert _lib.ABI_VERSION == 18
    P = _lib.parse_header()
    import ctypes as C
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double
    assert P["mivp_region_shape"] == (C.c_int, [vp, vp, i32, vp, vp, vp, vp])
    assert P["mivp_region_axes"] == (C.c_int, [vp, vp, vp, i32, f64, f64, f64, vp, vp, vp, vp])
    assert "double*" not in re.sub(r"/\*.*?\*/", " ", text, flags=re.S).replace(" ", "")


def test_library_exports_shape_symbols():
    import mivp_amd  # noqa: F401
    from mivp_amd import _lib
    lib = _lib.lib()
    assert lib.mivp_abi_version() == 18
    for n in SYMBOLS:
        assert hasattr(lib, n), n
