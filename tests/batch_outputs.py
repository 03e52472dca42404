"""What the GPU tests of the batch filler (test_hip_batches.py, test_hip_class_crops.py, test_hip_spatial_crops.py) do to a
``BatchFiller``'s output tensors, and the coordinate grid they hand to crops_ref.  A plain module, imported as crops_ref is."""


def outs(filler):
    """Every output tensor the filler holds."""
    f = filler
    return [t for t in [f.image, f.mask, f.coord, f.mask_st_0] + f.image_st + f.coord_st if t is not None]


def poison(filler):
    """NaN in every output: a voxel the kernels do not write stays visible.  Returns the tensors."""
    tensors = outs(filler)
    for t in tensors:
        t.fill_(float("nan"))
    return tensors


def grid(shape, device):
    from mivp_amd.students_teacher import coord_grid
    return coord_grid(shape, device)
