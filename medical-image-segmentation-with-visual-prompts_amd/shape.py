"""Per-lesion shape descriptors on the GPU (csrc/region_shape.hip): ``region_shape(table)`` and ``RegionShape``.

They are part of ``mivp_amd.regions`` (``regions.region_shape``, ``regions.RegionShape``), whose docstring has every field,
the derived values and the three conventions (Euler number of the union of closed voxels, voxel-face surface area, what is
out of scope).  This module holds the code so that ``regions`` itself keeps the functions it had; it imports nothing from
``regions`` and takes the ``RegionTable`` as it comes."""
from __future__ import annotations

import math
from typing import TYPE_CHECKING, Dict, Tuple

import numpy as np
import torch

from . import _lib as L
from ._host import check_gpu, i3

if TYPE_CHECKING:
    from .regions import RegionTable


MAX_SHAPE_DIM = 65535       # coordinate products stay below 2^32, so the int64 moments of < 2^31 voxels cannot overflow


def _check_shape_table(table) -> Tuple[int, int, int]:
    """-> the dims of a table ``region_shape`` can take: it carries its dense label map, and no dimension is above
    ``MAX_SHAPE_DIM``."""
    labels = getattr(table, "labels", None)
    if labels is None:
        raise ValueError("region_shape needs a RegionTable with its dense label map (table.labels)")
    dims = tuple(int(d) for d in table.dims)
    if len(dims) != 3 or tuple(labels.shape) != dims or labels.dtype != torch.int32:
        raise ValueError(f"table.labels must be an int32 tensor of the table's dims {dims}, got {labels.dtype} "
                         f"{tuple(labels.shape)}")
    if max(dims) > MAX_SHAPE_DIM:
        raise ValueError(f"region_shape takes no dimension above {MAX_SHAPE_DIM} (the int64 moments could overflow), got "
                         f"{dims}")
    return dims


class RegionShape:
    """The shape descriptors of the regions of a ``RegionTable`` (the module docstring has every field).  All tensors live
    on the device; entry ``r`` describes the region labelled ``r + 1``."""

    _FIELDS = ("moment2", "faces", "cells", "covariance_mm2", "eigenvalues", "axes")
    _DERIVED = ("euler", "major_axis_length", "minor_axis_length", "least_axis_length", "elongation", "flatness",
                "surface_area_mm2", "surface_to_volume", "sphericity")

    def __init__(self, table: RegionTable):
        m, dev = table.max_regions, table.size.device
        self.table, self.spacing = table, table.spacing
        self.moment2 = torch.empty((m, 6), dtype=torch.int64, device=dev)
        self.faces = torch.empty((m, 3), dtype=torch.int64, device=dev)
        self.cells = torch.empty((m, 2), dtype=torch.int64, device=dev)
        self.covariance_mm2 = torch.empty((m, 3, 3), dtype=torch.float64, device=dev)
        self.eigenvalues = torch.empty((m, 3), dtype=torch.float64, device=dev)
        self.axes = torch.empty((m, 3, 3), dtype=torch.float64, device=dev)

    # ---- derived, float64 (euler: int64), from the fields
    @property
    def euler(self) -> torch.Tensor:
        size = self.table.size
        return self.cells[:, 0] - self.cells[:, 1] + (6 * size + self.faces.sum(1)) // 2 - size

    def _axis_length(self, i: int) -> torch.Tensor:
        return 4.0 * torch.sqrt(self.eigenvalues[:, i])

    @property
    def major_axis_length(self) -> torch.Tensor:
        return self._axis_length(0)

    @property
    def minor_axis_length(self) -> torch.Tensor:
        return self._axis_length(1)

    @property
    def least_axis_length(self) -> torch.Tensor:
        return self._axis_length(2)

    def _axis_ratio(self, i: int) -> torch.Tensor:
        l0 = self.eigenvalues[:, 0]
        return torch.where(l0 > 0, torch.sqrt(self.eigenvalues[:, i] / l0), torch.full_like(l0, float("nan")))

    @property
    def elongation(self) -> torch.Tensor:
        return self._axis_ratio(1)

    @property
    def flatness(self) -> torch.Tensor:
        return self._axis_ratio(2)

    @property
    def surface_area_mm2(self) -> torch.Tensor:
        sh, sw, sd = self.spacing
        f = self.faces.to(torch.float64)
        return f[:, 0] * (sw * sd) + f[:, 1] * (sh * sd) + f[:, 2] * (sh * sw)

    @property
    def surface_to_volume(self) -> torch.Tensor:
        return self.surface_area_mm2 / self.table.volume_mm3

    @property
    def sphericity(self) -> torch.Tensor:
        v = self.table.volume_mm3
        return (36.0 * math.pi * v * v) ** (1.0 / 3.0) / self.surface_area_mm2

    def _device_fields(self) -> Dict[str, torch.Tensor]:
        out = {k: getattr(self, k) for k in self._FIELDS}
        out.update({k: getattr(self, k) for k in self._DERIVED})
        return out

    def cpu(self) -> Dict[str, np.ndarray]:
        """The one synchronising call: every field and derived value as a numpy array trimmed to ``n`` (plus ``"n"``).
        Raises ``RuntimeError`` when the map has more regions than ``max_regions``, as ``RegionTable.cpu()`` does."""
        fields = self._device_fields()
        head = torch.stack([self.table.n[0], self.table.overflow[0]]).cpu()
        n, overflow = int(head[0]), int(head[1])
        self.table.check_overflow(n, overflow)
        out = {k: v[:n].cpu().numpy() for k, v in fields.items()}
        out["n"] = n
        return out


def region_shape(table: RegionTable) -> RegionShape:
    """The shape descriptors of the regions of ``table`` (what ``region_stats`` or ``SlidingWindowPredictor.predict_regions``
    returned): second moments, exposed faces, vertex and edge counts from one pass over ``table.labels``, then covariance,
    eigenvalues and principal axes per region from ``table.size`` / ``table.coord_sum`` with ``table.spacing`` (the module
    docstring has the definitions).  Two launches, no host read: ``RegionShape.cpu()`` synchronises."""
    dims = _check_shape_table(table)
    check_gpu("table.labels", table.labels)
    shape = RegionShape(table)
    m = table.max_regions
    sh, sw, sd = table.spacing
    L.call("mivp_region_shape", L.ptr(table.labels), i3(dims), m, L.ptr(shape.moment2), L.ptr(shape.faces),
           L.ptr(shape.cells), L.stream())
    L.call("mivp_region_axes", L.ptr(table.size), L.ptr(table.coord_sum), L.ptr(shape.moment2), m, sh, sw, sd,
           L.ptr(shape.covariance_mm2), L.ptr(shape.eigenvalues), L.ptr(shape.axes), L.stream())
    return shape
