"""numpy / float64 restatement of the input-side formulas (tests/prompt_ref.py is the token-prompt reference, hence this
file's name): the patch embedding's data gradient, the trilinear lattice interpolation T of ``prompting.InputPrompt`` under
torch's ``align_corners=True`` rule, its transpose, and the summation order of the full-resolution backward.

  dgrad   dx[b,ci,2h+a,2w+b',2d+c] = sum_co w[co,ci,a,b',c] dz[b,h,w,d,co]                    (kernel == stride == 2)
  T       voxel o of an axis with n voxels and g nodes sits at s = o (g-1)/(n-1) (0 when g == 1 or n == 1), an exact rational:
          i0 = floor(s), lambda = s - i0, i1 = min(i0 + 1, g - 1); T = M_h (x) M_w (x) M_d with rows (1 - lambda) e_i0 + lambda e_i1
  T^t     dP[ci] = sum_b M_h^t M_w^t M_d^t g[b,ci]
  err     the yardstick: E32 = max |f32 composition - f64| over the tensor; every element of the kernel's result must lie
          within 8 E32 of the float64 value"""
import numpy as np

F64 = np.float64


def embed_dgrad(dz, w):
    """dz [B,h,w,d,C], w [C,Cin,2,2,2] -> dx [B,Cin,2h,2w,2d], float64."""
    dz, w = np.asarray(dz, F64), np.asarray(w, F64)
    B, h, ww, d, _ = dz.shape
    t = np.einsum("bhwdo,oixyz->bihxwydz", dz, w)
    return t.reshape(B, w.shape[1], 2 * h, 2 * ww, 2 * d)


def axis_matrix(n, g):
    """[n, g] float64 interpolation weights of one axis (exact rational coordinates)."""
    num = g - 1 if (n > 1 and g > 1) else 0
    den = n - 1 if n > 1 else 1
    M = np.zeros((n, g), F64)
    for o in range(n):
        t = o * num
        i0 = t // den
        lam = (t - i0 * den) / den
        M[o, i0] += 1.0 - lam
        M[o, min(i0 + 1, g - 1)] += lam
    return M


def interp(P, roi):
    """P [Cin,gh,gw,gd] -> T(P) [Cin,H,W,D], float64."""
    P = np.asarray(P, F64)
    Mh, Mw, Md = (axis_matrix(roi[a], P.shape[1 + a]) for a in range(3))
    return np.einsum("cijk,hi,wj,dk->chwd", P, Mh, Mw, Md)


def interp_t(g, lattice):
    """g [B,Cin,H,W,D] -> T^t g summed over the batch, [Cin,gh,gw,gd], float64."""
    g = np.asarray(g, F64)
    Mh, Mw, Md = (axis_matrix(g.shape[2 + a], lattice[a]) for a in range(3))
    return np.einsum("bchwd,hi,wj,dk->cijk", g, Mh, Mw, Md)


def prompt_fwd(x, P, scale):
    return np.asarray(x, F64) + float(scale) * interp(P, x.shape[2:])[None]


def prompt_bwd(g, lattice, scale):
    return float(scale) * interp_t(g, lattice)


def identity_bwd_f32(g, scale):
    """The full-resolution backward in the kernel's order and precision: one float32 accumulator per node that starts at 0
    and takes the samples b = 0, 1, .. in turn (every weight is exactly 1), then one multiplication by scale."""
    g = np.asarray(g, np.float32)
    acc = np.zeros(g.shape[1:], np.float32)
    for b in range(g.shape[0]):
        acc = (acc + g[b]).astype(np.float32)
    return (np.float32(scale) * acc).astype(np.float32)


def first_bad(bad):
    """Index tuple of the first True of a boolean array (C order), or None."""
    idx = np.argwhere(bad)
    return None if idx.shape[0] == 0 else tuple(int(i) for i in idx[0])


def check_err32(got, ref64, ref32, what, names):
    """8 x E32 per element; returns (worst multiple of E32, E32)."""
    got, ref64, ref32 = np.asarray(got, F64), np.asarray(ref64, F64), np.asarray(ref32, F64)
    assert got.shape == ref64.shape == ref32.shape, (what, got.shape, ref64.shape, ref32.shape)
    e32 = float(np.abs(ref32 - ref64).max())
    err = np.abs(got - ref64)
    worst = float(err.max()) / e32 if e32 > 0 else (0.0 if float(err.max()) == 0 else float("inf"))
    print(f"[E32] {what}: E32 {e32:.3e}, worst error {float(err.max()):.3e} = {worst:.2f} x E32")
    at = first_bad(~(err <= 8 * e32))
    assert at is None, (f"{what}: first element beyond 8 x E32 at {dict(zip(names, at))}: got {got[at]!r}, float64 {ref64[at]!r}, "
                        f"E32 {e32:.3e}")
    return worst, e32
