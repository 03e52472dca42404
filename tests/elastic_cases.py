"""The inputs and the bounds that tests/test_elastic_crops_host.py (CPU) and tests/test_hip_elastic_crops.py (GPU) share, so
that what the CPU test proves about the reference -- how few label voxels sit near a rounding tie -- holds on the exact
inputs of the GPU tolerance test.  A plain module, imported as crops_ref is; it needs no GPU."""
import numpy as np
import torch

# the bank of test_hip_spatial_crops.py (its first three volumes, the same generator): 2 channels, labels 0..7
SHAPES = [(20, 18, 36), (21, 19, 37), (6, 8, 5)]
ACTIVE = [2, 5]
ROI = (12, 10, 20)                                                  # of the general, linear and mixed cases
GENERAL_ORIGINS = {0: (4, 3, 7), 1: (3, 4, 7), 2: (11, 3, 0), 3: (4, 12, 0)}      # volume 0 under each rotation code
GENERAL_NODES = [(4, 4, 4), (5, 4, 7)]
MAX_P = 2.0                                                         # the lattices of the general case: values in +-2 voxels
K = 160
EPS = 2.0 ** -24


def bank_arrays(channels, integer):
    """(images, labels) as numpy: integer voxel values in 0..255 (or uniform floats in [-1, 3)), labels 0..7."""
    g = torch.Generator().manual_seed(31 + channels)
    images, labels = [], []
    for s in SHAPES + [(40, 36, 70)]:                               # the fourth volume is drawn, as there, and dropped
        shape = (channels,) + s
        img = torch.randint(0, 256, shape, generator=g).float() if integer else torch.rand(shape, generator=g) * 4 - 1
        lab = torch.randint(0, 8, s, generator=g, dtype=torch.uint8)
        images.append(img.numpy())
        labels.append(lab.numpy())
    return images[:3], labels[:3]


def general_affine():
    """float32 [2, 12]: the map of the existing general test, angles (0.3, -0.2, 0.5) and zooms (1.1, 0.9, 1.05), written out
    (F = I): A = R2 R1 R0 diag(1 / zoom); the second sample with a sub-voxel shift."""
    c, s = np.cos([0.3, -0.2, 0.5]), np.sin([0.3, -0.2, 0.5])
    R0 = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
    R1 = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
    R2 = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
    A = R2 @ R1 @ R0 @ np.diag(1.0 / np.array([1.1, 0.9, 1.05]))
    out = np.zeros((2, 12), np.float32)
    out[:, :9] = A.reshape(-1)
    out[1, 9:] = [0.3, -0.45, 0.2]
    return out


def general_lattice(nodes, code):
    """float32 [2, 3, n0, n1, n2]: non-dyadic random displacements in +-MAX_P voxels, another set per rotation code."""
    rs = np.random.RandomState(1000 + 10 * int(np.prod(nodes)) + code)
    return rs.uniform(-MAX_P, MAX_P, size=(2, 3) + tuple(nodes)).astype(np.float32)


def bounds(affine, max_p):
    """(delta_d, delta_r) in voxels for fp32 maps ``affine`` [B, 12] and lattices of magnitude <= ``max_p``.

    eps = 2^-24 bounds the relative error of one fp32 operation.  delta_d = K eps max|P| bounds the error of the
    displacement; K is counted from the kernel's evaluation order (mivp.h):
      60  x_k = (u_k + 0.5) * ((n_k - 3) / roi_k) carries two roundings of a value below 5, so f_k is off by at most
          10 eps; d changes by at most max|P[j + 1] - P[j]| <= 2 max|P| per unit of x_k: 20 eps max|P| on each of 3 axes;
      48  each basis weight (at most five operations on intermediates below 6, then the sixth) is within 4 eps of the
          exact one at that f; perturbing the four weights of one axis moves d by at most 4 * 4 eps max|P|: 3 axes;
      21  the sums: w_ab = B_a * B_b (1), sixteen fma per column on partial sums below max|P| (16), four terms of the
          last sum (4);
    129 in all; K = 160 leaves room for the second-order terms.
    delta = 8 eps max(extent) is the existing bound of the affine r (three products and three sums of terms below the
    extent); the one new sum q_k + d_k is another term below the extent and still inside its 8.
    delta_r = delta + (max row sum of |A|) * delta_d."""
    delta = 8 * EPS * max(SHAPES[0])
    delta_d = K * EPS * float(max_p)
    rows = np.abs(np.asarray(affine, np.float64)[:, :9].reshape(-1, 3, 3)).sum(axis=2).max()
    return delta_d, delta + rows * delta_d


def near_tie(r, delta_r):
    """bool [B, h, w, d]: r + 0.5 within delta_r of an integer on any axis -- where fp32 may round a label voxel the other way."""
    h = np.asarray(r) + 0.5
    return (np.abs(h - np.round(h)) <= delta_r).any(axis=1)
