"""float64 reference and exact cases for the low-resolution head kernels of csrc/uphead.hip (test helper, not a test
module).  The head is conv3x3x3(BatchNorm-affine(upsample_x2(x))) evaluated from the low-resolution x; every weight in
its kernels is dyadic (trilinear .25 / .75, Gram 1.25 / 1.625 / .375 / 2), so the exact-integer method of
tests/exact_ref.py applies once the test chooses scale, shift, mean and rstd itself.  Four conditions are asserted on the
float64 reference of every case, on 100 % of its elements:

  (a)  the reference op applied to absolute values, times the common denominator of the kernel's values (``unit``), stays
       below 2**24: every partial sum in any order is an fp32 number;
  (b)  where the kernel stores bf16 the reference is a bf16 number;
  (c)  every per-tap low-resolution plane value is an fp16 number (the forward parks the planes as fp16);
  (d)  every element of the adjoint tensor D is a bf16 number.

The training-mode dx carries 1/512 fractions from the Gram term into a bf16 store and cannot meet (b): it is held to the
interval |got - ref64| <= half the bf16 spacing at ref64 (all f32 arithmetic before the store is exact under (a), so the
store's single rounding is the only error; ties may go either way).

Everything is float64 torch on the CPU built from F.interpolate, F.conv3d, F.pad, slicing and autograd; nothing shares
code with the kernels.  Volumes are channels-first [B, C, h, w, d] unless a name says otherwise."""
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_ref as E  # noqa: E402

# (B, h, w, d): the smallest shapes that reach each seam (ST_SEG = 16 cells along d, bricks of 4 x 4 x 16 cells,
# 512 tokens per k_uphead_taps workgroup, 64 per k_uphead_dx workgroup)
SHAPES = {
    "S1": (1, 1, 1, 1),        # one cell per axis: Gram diagonal 2, both clamps at once
    "S2": (1, 1, 2, 3),        # two-cell axis: both ends clamped, no interior
    "S3": (2, 5, 4, 17),       # h crosses the 4-brick, w is one brick, d crosses the segment / brick by one cell; T = 680
    "S4": (1, 2, 3, 33),       # three d segments / bricks, the last with one cell
    "S5": (1, 4, 4, 16),       # exactly one brick and one segment
    "S6": (2, 3, 9, 32),       # w crosses two bricks, d exactly two; T = 1728
}
C_LADDER = (8, 16, 24, 40, 48, 56)

X_VALS = (-2, -1, 0, 1, 2)
W_VALS = (-1, 0, 1)
SHIFT_VALS = tuple(range(-3, 4))
BIAS_VALS = tuple(range(-3, 4))
DYADIC = (0.5, 1, 2)
DY_VALS = (-128, -64, 64, 128)          # multiples of 64: the 1/64 weights of the adjoint give integers

UNIT_GATHER = 64                        # a product of three trilinear weights
UNIT_GRAM = 512                         # a product of three Gram weights


class Case(dict):
    __getattr__ = dict.__getitem__


def shape_c_pairs():
    """(shape name, C) of every case family: C = 8 and 48 everywhere, the whole ladder on S3."""
    out = []
    for name in SHAPES:
        for c in (C_LADDER if name == "S3" else (8, 48)):
            out.append((name, c))
    return out


def _seed(*ints):
    s = 17
    for v in ints:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def _pc(v, like):
    return v.view(1, -1, *([1] * (like.dim() - 2)))


def cl64(t):
    """[B, C, h, w, d] -> channels-last [B, h, w, d, C] (float64, contiguous)."""
    return t.permute(0, 2, 3, 4, 1).contiguous()


def up(x):
    return F.interpolate(x, scale_factor=2, mode="trilinear", align_corners=False)


def is_fp16(t):
    return t.float().half().double() == t


# ---------------------------------------------------------------------------------------------
# references (each returns the reference and the same op on absolute values)
# ---------------------------------------------------------------------------------------------
def forward_ref(x, w, b, scale, shift):
    """conv3d(up(x) * scale + shift, w, b, padding=1): (ref, bound), [B, Cout, 2h, 2w, 2d]."""
    def run(x, w, b, scale, shift):
        return F.conv3d(up(x) * _pc(scale, x) + _pc(shift, x), w, b, padding=1)
    return run(x, w, b, scale, shift), run(x.abs(), w.abs(), None if b is None else b.abs(), scale.abs(), shift.abs())


def stats_ref(x):
    """Per channel sum(Ux), sum((Ux)^2) and gx = U^T U x (the autograd gradient of 0.5 * sum((Ux)^2), no Gram
    matrix written down): ((s1, s2, gx), their bounds)."""
    def run(x):
        x = x.clone().requires_grad_(True)
        u = up(x)
        (0.5 * (u * u).sum()).backward()
        u = u.detach()
        return u.sum((0, 2, 3, 4)), (u * u).sum((0, 2, 3, 4)), x.grad
    return run(x), run(x.abs())


def _shifted_sum(planes_up):
    """y[u] = sum_tap [u + tap - 1 inside] planes_up[tap][u + tap - 1]: [27, B, Cout, H, W, D] -> [B, Cout, H, W, D]."""
    H, W, D = planes_up.shape[-3:]
    y = 0
    for tap, (kh, kw, kd) in enumerate(E.taps()):
        p = F.pad(planes_up[tap], (1, 1, 1, 1, 1, 1))
        y = y + p[..., kh:kh + H, kw:kw + W, kd:kd + D]
    return y


def adjoint_ref(dy, dims, cout):
    """D[q][tap * cout + co] by autograd: 27 zero planes Y_tap, y = sum over taps of the upsampled plane shifted by the tap
    and zero padded, D = d<dy, y>/dY.  dy [B, cout, 2h, 2w, 2d]; returns ([T, 27 * cout], bound), rows in (b, h, w, d) order."""
    B = dy.shape[0]
    h, w, d = dims

    def run(dy):
        Y = torch.zeros((27, B, cout, h, w, d), dtype=torch.float64, requires_grad=True)
        y = _shifted_sum(torch.stack([up(Y[tap]) for tap in range(27)]))
        (dy * y).sum().backward()
        return Y.grad.permute(1, 3, 4, 5, 0, 2).reshape(B * h * w * d, 27 * cout)
    return run(dy), run(dy.abs())


def dx_ref(D, wc, x, coef, dims):
    """dx[p][c] = sc_c * ((D Wc^T)[p][c] - 8 k1_c - k2_c * (gram(x)[p][c] - 8 mu_c)), the closed form above k_uphead_dx
    with gram from stats_ref.  D [T, K], wc [C, K], x [B, C, h, w, d], coef [4, C] = (sc | k1 | k2 | mu); returns
    channels-last ([B, h, w, d, C], bound)."""
    B, C = x.shape[:2]
    (_, _, gram), (_, _, gram_abs) = stats_ref(x)
    sc, k1, k2, mu = coef
    dz = (D @ wc.t()).view(B, *dims, C)
    dz_abs = (D.abs() @ wc.abs().t()).view(B, *dims, C)
    ref = sc * (dz - 8 * k1 - k2 * (cl64(gram) - 8 * mu))
    bound = sc.abs() * (dz_abs + 8 * k1.abs() + k2.abs() * (cl64(gram_abs) + 8 * mu.abs()))
    return ref, bound


def head_grads_ref(G, S, w, scale, shift, mean_rstd):
    """The head's four parameter gradients from G [Cout, 27, Cin] and S [Cout, 27] (autograd of BatchNorm -> conv):
    ((dW [Cout, Cin, 27], db, dgamma, dbeta), their bounds)."""
    cout, _, cin = G.shape

    def run(G, S, w, scale, shift, mean, rstd, sign):
        wt = w.reshape(cout, cin, 27).permute(0, 2, 1)                       # [co, tap, ci]
        S1 = S.unsqueeze(-1)
        dW = (G * scale + S1 * shift).permute(0, 2, 1).contiguous()
        dgamma = rstd * (wt * (G + sign * S1 * mean)).sum((0, 1))
        return dW, S[:, 13].clone(), dgamma, (wt * S1).sum((0, 1))

    mean, rstd = mean_rstd[:cin], mean_rstd[cin:]
    return (run(G, S, w, scale, shift, mean, rstd, -1.0),
            run(G.abs(), S.abs(), w.abs(), scale.abs(), shift.abs(), mean.abs(), rstd.abs(), 1.0))


def planes_ref(x, w, scale, shift):
    """Y[tap][b][co][p] = sum_c w[co][c][tap] * scale[c] * x[b][c][p] + sum_c w[co][c][tap] * shift[c]: the per-tap
    low-resolution planes [27, B, Cout, h, w, d] and their bound.  Only used to assert representability (c)."""
    cout, cin = w.shape[:2]

    def run(x, w, scale, shift):
        wt = w.reshape(cout, cin, 27)
        return (torch.einsum("ock,bchwd->kbohwd", wt * scale.view(1, -1, 1), x)
                + (wt * shift.view(1, -1, 1)).sum(1).t().reshape(27, 1, cout, 1, 1, 1))
    return run(x, w, scale, shift), run(x.abs(), w.abs(), scale.abs(), shift.abs())


# ---------------------------------------------------------------------------------------------
# the plane decomposition written out by hand (host test): clamped .25 / .75 interpolation, then masked taps
# ---------------------------------------------------------------------------------------------
def _up_axis(t, axis):
    n = t.shape[axis]
    idx = torch.arange(n)
    prev = t.index_select(axis, (idx - 1).clamp(min=0))
    nxt = t.index_select(axis, (idx + 1).clamp(max=n - 1))
    return torch.stack([0.25 * prev + 0.75 * t, 0.75 * t + 0.25 * nxt], axis + 1).flatten(axis, axis + 1)


def gather_planes(Y, bias=None):
    """Planes [27, B, Cout, h, w, d] -> y [B, Cout, 2h, 2w, 2d]."""
    U = Y
    for axis in (3, 4, 5):
        U = _up_axis(U, axis)
    y = _shifted_sum(U)
    return y if bias is None else y + _pc(bias, y)


# ---------------------------------------------------------------------------------------------
# conditions
# ---------------------------------------------------------------------------------------------
def _flag(ok):
    """An elementwise condition as a (ref, bound) pair that exact_ref.exact_ok rejects wherever it fails."""
    v = (~ok).double() * E.EXACT_LIMIT
    return v, v


def bf16_half_spacing(ref64):
    """Half the bf16 spacing at each float64 value (0 at 0): the most a single round-to-nearest bf16 store can move it."""
    _, ex = torch.frexp(ref64.abs())                       # |v| = m * 2**ex, m in [0.5, 1)
    half = torch.ldexp(torch.ones_like(ref64), ex - 1 - 8)
    return torch.where(ref64 == 0, torch.zeros_like(ref64), half)


def assert_interval_located(got, ref64, what=""):
    """|got - ref64| <= half the bf16 spacing at ref64 at every element of a channels-last [B, h, w, d, C] volume."""
    g = got.detach().double().cpu()
    assert g.shape == ref64.shape, f"{what}: shape {tuple(g.shape)} != reference {tuple(ref64.shape)}"
    err = (g - ref64).abs()
    bad = torch.nonzero(~(err <= bf16_half_spacing(ref64)))          # NaN fails
    if bad.numel() == 0:
        return
    idx = [tuple(int(i) for i in row) for row in bad]
    lines = [f"{what}: {len(idx)} of {g.numel()} elements lie outside half a bf16 spacing of the float64 reference"
             f" (axes bhwdc, shape {tuple(g.shape)})"]
    for i in idx[:10]:
        lines.append(f"  {i}: got {float(g[i])!r} want {float(ref64[i])!r}")
    lines.append(f"  voxels by position: {E._border_report(idx, tuple(g.shape[1:4]))}")
    msg = "\n".join(lines)
    print(msg)
    raise AssertionError(msg)


def _check(case):
    """Assert every condition the case was picked under, with the pairs ``case.conds`` = [(ref, bound, stored, what)]."""
    for ref, bound, stored, what in case.conds:
        E.assert_exact_inputs(ref, bound, stored, what)
    return case


def _pick(make):
    """first_exact over ``make(dens) -> Case`` (with .conds and .dens), then the assertions on what came back."""
    def m(dens):
        c = make(dens)
        c["dens"] = dens
        return (tuple(r for r, _, _, _ in c.conds), tuple(b for _, b, _, _ in c.conds),
                tuple(s for _, _, s, _ in c.conds), c)
    return _check(E.first_exact(m))


# ---------------------------------------------------------------------------------------------
# cases (cached: a reference is computed once and shared)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def forward_case(name, C, cout, bias=True):
    B, h, w, d = SHAPES[name]

    def make(dens):
        g = E.gen(_seed(1, B, h, w, d, C, cout))
        x = E.draw(g, (B, C, h, w, d), X_VALS)
        wt = E.draw(g, (cout, C, 3, 3, 3), W_VALS, dens)
        b = E.draw(g, (cout,), BIAS_VALS) if bias else None
        scale = E.draw(g, (C,), DYADIC)
        shift = E.draw(g, (C,), SHIFT_VALS)
        ref, bound = forward_ref(x, wt, b, scale, shift)
        planes, pbound = planes_ref(x, wt, scale, shift)
        # the planes are multiples of 1/2 (scale 0.5), the gather multiplies them by three trilinear weights
        unit = UNIT_GATHER * 2
        conds = [(ref * unit, bound * unit, False, "forward (a)"), (planes * 2, pbound * 2, False, "planes (a)"),
                 (*_flag(is_fp16(planes)), False, "planes (c)")]
        return Case(x=x, w=wt, b=b, scale=scale, shift=shift, ref=ref, bound=bound, planes=planes, conds=conds)
    c = _pick(make)
    assert bool(is_fp16(c.planes).all()) and float(c.planes.abs().max()) <= 2048, "condition (c)"
    assert bool(((c.planes * 2) == (c.planes * 2).round()).all())
    E.assert_bf16_operands(c.x, c.w * _pc(c.scale, c.w))
    return c


@functools.lru_cache(maxsize=None)
def stats_case(name, C):
    B, h, w, d = SHAPES[name]

    def make(dens):
        g = E.gen(_seed(2, B, h, w, d, C))
        x = E.draw(g, (B, C, h, w, d), X_VALS, dens)
        (s1, s2, gx), (a1, a2, agx) = stats_ref(x)
        conds = [(s1, a1, False, "sum (a)"), (s2 * UNIT_GRAM, a2 * UNIT_GRAM, False, "sum of squares (a)"),
                 (gx * UNIT_GRAM, agx * UNIT_GRAM, False, "gx (a)")]
        return Case(x=x, s1=s1, s2=s2, gx=gx, conds=conds)
    c = _pick(make)
    E.assert_bf16_operands(c.x)
    return c


@functools.lru_cache(maxsize=None)
def adjoint_case(name, cout):
    B, h, w, d = SHAPES[name]

    def make(dens):
        g = E.gen(_seed(3, B, h, w, d, cout))
        dy = E.draw(g, (B, cout, 2 * h, 2 * w, 2 * d), DY_VALS, dens)
        D, bound = adjoint_ref(dy, (h, w, d), cout)
        conds = [(D * UNIT_GATHER, bound * UNIT_GATHER, False, "adjoint (a)"), (D, bound, True, "adjoint (d)")]
        return Case(dy=dy, D=D, conds=conds)
    return _pick(make)


@functools.lru_cache(maxsize=None)
def dx_case(name, C, cout, training):
    """Hand-made D, wc and coef for mivp_uphead_dx.  Eval (k1 = k2 = 0): dx is a bf16 number (b).  Training: the Gram
    term's 1/512 fractions times k2 and sc in {.5, 1, 2} give multiples of 1/2048; (a) at that unit, interval at the store."""
    B, h, w, d = SHAPES[name]
    T, K = B * h * w * d, 27 * cout

    def make(dens):
        g = E.gen(_seed(4, B, h, w, d, C, cout, int(training)))
        x = E.draw(g, (B, C, h, w, d), X_VALS)
        D = E.draw(g, (T, K), X_VALS, 0.5)
        wc = E.draw(g, (C, K), W_VALS, dens)
        sc = E.draw(g, (C,), DYADIC)
        if training:
            k1, k2, mu = E.draw(g, (C,), (-1, -0.5, 0.5, 1)), E.draw(g, (C,), DYADIC), E.draw(g, (C,), (-1, -0.5, 0.5, 1, 1.5))
        else:
            k1, k2, mu = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), E.draw(g, (C,), (-1, 0.5, 1.5))
        coef = torch.stack([sc, k1, k2, mu])
        ref, bound = dx_ref(D, wc, x, coef, (h, w, d))
        (_, _, gram), (_, _, gram_abs) = stats_ref(x)
        unit = UNIT_GRAM * 4 if training else 2
        conds = [(ref * unit, bound * unit, False, "dx (a)"), (gram * UNIT_GRAM, gram_abs * UNIT_GRAM, False, "gram (a)")]
        if not training:
            conds.append((ref, bound, True, "dx (b)"))
        return Case(x=x, D=D, wc=wc, coef=coef, gram=gram, ref=ref, conds=conds)
    c = _pick(make)
    E.assert_bf16_operands(c.x, c.D, c.wc)
    return c


@functools.lru_cache(maxsize=None)
def head_grads_case(C, cout):
    def make(dens):
        g = E.gen(_seed(5, C, cout))
        G = E.draw(g, (cout, 27, C), tuple(range(-9, 10)), dens)
        S = E.draw(g, (cout, 27), tuple(range(-5, 6)))
        w = E.draw(g, (cout, C, 3, 3, 3), W_VALS)
        scale, shift = E.draw(g, (C,), DYADIC), E.draw(g, (C,), SHIFT_VALS)
        mean_rstd = torch.cat([E.draw(g, (C,), (-1, -0.5, 0.5, 1, 2)), E.draw(g, (C,), DYADIC)])
        ref, bound = head_grads_ref(G, S, w, scale, shift, mean_rstd)
        # G * scale and S * mean are multiples of 1/2, rstd * (...) of 1/4
        conds = [(r * 4, b * 4, False, "head grads (a)") for r, b in zip(ref, bound)]
        return Case(G=G, S=S, w=w, scale=scale, shift=shift, mean_rstd=mean_rstd, ref=ref, conds=conds)
    return _pick(make)


def all_cases():
    """(label, builder) of every exact case the GPU module uses; the host test runs each builder on the CPU."""
    out = []
    for name, C in shape_c_pairs():
        for cout in (1, 2):
            out.append((f"forward {name} C={C} Cout={cout}", functools.partial(forward_case, name, C, cout)))
        out.append((f"stats {name} C={C}", functools.partial(stats_case, name, C)))
        for training in (False, True):
            out.append((f"dx {name} C={C} training={training}", functools.partial(dx_case, name, C, dx_cout(C), training)))
    for C in (8, 48):
        for cout in (3, 4):
            out.append((f"forward S3 C={C} Cout={cout}", functools.partial(forward_case, "S3", C, cout)))
    out.append(("forward S3 C=48 Cout=2 no bias", functools.partial(forward_case, "S3", 48, 2, False)))
    for name in SHAPES:
        out.append((f"adjoint {name} Cout=2", functools.partial(adjoint_case, name, 2)))
    for name in ("S3", "S4"):
        for cout in (1, 3, 4):
            out.append((f"adjoint {name} Cout={cout}", functools.partial(adjoint_case, name, cout)))
    for C in (8, 56):
        for cout in (1, 2):
            out.append((f"head_grads C={C} Cout={cout}", functools.partial(head_grads_case, C, cout)))
    return out


def dx_cout(C):
    return 1 if C in (8, 24) else 2
