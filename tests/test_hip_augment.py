"""GPU: the random intensity chain (csrc/intensity.hip through mivp_amd.augment) against tests/intensity_ref.py.

Parity.  Per sample, err = max |kernel - f64 oracle| / (max - min of the f64 output).  The yardstick E32 is the worst such
error of the float32 numpy restatement against the float64 oracle over the same cases (every shape, every draw set, every
sample), computed here; the kernel must stay within 8 x E32 (another reduction order, device exp / pow a few ulp off,
gamma up to 4.5 multiplying the base's relative error).  No case and no voxel is left out.

Exactness.  A sample without flags is bitwise the input while its neighbours are augmented; two runs, in place and out of
place, and a graph replay after new draws were loaded are bitwise equal to the eager result.

Integration.  ``augment=`` on the phase-1 and phase-2 steps: all-off draws change nothing, some draws equal augmenting the
input first, and the graphed steps replay what the eager steps compute."""
import copy
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

import intensity_ref as R
from conftest import load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 1, 13, 10, 9),        # odd D (two groups of four and a one-voxel tail per row), mixed flags per sample
          (2, 2, 8, 8, 1),          # two channels, an axis of length 1
          (1, 1, 40, 36, 33)]       # one sample over 12 workgroups, the last run of items partial
N_DRAWS = 40
BOUND = 8.0


def _aug():
    import mivp_amd  # noqa: F401
    from mivp_amd import augment
    return augment


def _input(shape, seed):
    return np.clip(1.4 * np.random.RandomState(seed).rand(*shape) - 0.2, 0.0, 1.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _cases(si):
    """(x, [(draws, f64 oracle, f32 restatement)]) of one shape: about 40 seeded draw sets, each step dropped with
    probability 0.3.  Computed once and shared; nothing modifies it."""
    A = _aug()
    shape = SHAPES[si]
    x = _input(shape, 100 + si)
    assert (x == 0).any() and (x == 1).any()
    out = []
    for k in range(N_DRAWS):
        d = A.draw_intensity(np.random.RandomState(1000 * si + k), shape[0], prob=0.7)
        out.append((d, R.chain(x.astype(np.float64), d, np.float64), R.chain(x, d, np.float32)))
    return x, out


@functools.lru_cache(maxsize=None)
def _e32():
    worst = 0.0
    for si in range(len(SHAPES)):
        _, cases = _cases(si)
        for d, w64, w32 in cases:
            worst = max(worst, max(R.rel_err(w32[b], w64[b]) for b in range(d.batch)))
    return worst


def _run(A, x, d, out=None, slot=None):
    slot = slot if slot is not None else A.IntensitySlot(d.batch, DEV)
    slot.load(d)
    return A.augment_intensity(x, slot, out=out)


def _draws(A, B, flags, seed=0, **kw):
    """All-on draws of a seed restricted to ``flags`` (one int or one per sample), single parameters overridden."""
    d = A.draw_intensity(np.random.RandomState(seed), B, prob=1.0)
    d.flags[:] = flags
    for k, v in kw.items():
        getattr(d, k)[:] = v
    return d


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_chain_matches_the_float64_oracle_within_8_e32(si):
    A = _aug()
    x, cases = _cases(si)
    e32 = _e32()
    xg = torch.from_numpy(x).to(DEV)
    slot = A.IntensitySlot(x.shape[0], DEV)
    seen, worst = set(), 0.0
    for d, w64, _ in cases:
        got = _run(A, xg, d, slot=slot).cpu().numpy()
        assert np.isfinite(got).all()
        seen |= set(int(f) for f in d.flags)
        worst = max(worst, max(R.rel_err(got[b], w64[b]) for b in range(d.batch)))
    print(f"[augment parity] shape {SHAPES[si]}: E32 {e32:.3e}, kernel {worst:.3e}, ratio {worst / e32:.2f} (bound {BOUND})")
    assert len(seen) >= (20 if x.shape[0] > 1 else 12)               # the draw sets mix the steps
    assert 1e-7 < e32 < 1e-5, e32                                    # the yardstick is what single precision gives
    assert worst <= BOUND * e32, (worst, e32)


@pytest.mark.parametrize("bit", [1, 2, 4, 8, 16])
def test_single_steps_match_the_oracle(bit):
    """Each step alone (the chain cases mostly run several), on the shape with a one-voxel tail and on two channels."""
    A = _aug()
    for si in (0, 1):
        x, _ = _cases(si)
        d = _draws(A, x.shape[0], bit, seed=bit)
        got = _run(A, torch.from_numpy(x).to(DEV), d).cpu().numpy()
        want = R.chain(x.astype(np.float64), d, np.float64)
        err = max(R.rel_err(got[b], want[b]) for b in range(d.batch))
        assert err <= BOUND * _e32(), (bit, si, err)


# ------------------------------------------------------------------------------------------------ exactness
def test_all_off_sample_is_bitwise_the_input_between_augmented_neighbours():
    A = _aug()
    x, _ = _cases(0)
    xg = torch.from_numpy(x).to(DEV)
    d = _draws(A, 3, [31, 0, 31], seed=3)
    got = _run(A, xg, d)
    assert torch.equal(got[1], xg[1])
    assert not torch.equal(got[0], xg[0]) and not torch.equal(got[2], xg[2])
    want = R.chain(x.astype(np.float64), d, np.float64)
    assert max(R.rel_err(got[b].cpu().numpy(), want[b]) for b in range(3)) <= BOUND * _e32()
    off = _run(A, xg, A.draw_intensity(np.random.RandomState(0), 3, prob=0.0))
    assert torch.equal(off, xg) and off.data_ptr() != xg.data_ptr()


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_two_runs_and_in_place_are_bitwise_equal(si):
    A = _aug()
    x, cases = _cases(si)
    xg = torch.from_numpy(x).to(DEV)
    for d, _, _ in cases[:6]:
        a = _run(A, xg, d)
        b = _run(A, xg, d)
        c = xg.clone()
        r = _run(A, c, d, out=c)
        assert r is c
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(xg.cpu(), torch.from_numpy(x))                # out of place leaves the input alone


# ------------------------------------------------------------------------------------------------ edge draws
def _edge(A, x, d):
    got = _run(A, torch.from_numpy(x).to(DEV), d).cpu().numpy()
    want = R.chain(x.astype(np.float64), d, np.float64)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    err = max(R.rel_err(got[b], want[b]) for b in range(d.batch))
    assert err <= BOUND * _e32(), err
    return got, want


def test_edge_constant_image():
    A = _aug()
    x = np.full((2, 1, 13, 10, 9), 0.375, dtype=np.float32)       # (sums of 0.375 are exact: M2 = 0)
    got, _ = _edge(A, x, _draws(A, 2, 2 | 4 | 16, seed=1))                  # std 0, range 0, histogram passes through
    assert (got == np.float32(0.375)).all()
    _edge(A, x, _draws(A, 2, 31, seed=2))                                   # the bias field gives it a range again
    got, _ = _edge(A, np.zeros_like(x), _draws(A, 2, 31, seed=3))
    assert (got == 0).all()


def test_edge_scale_minus_one():
    A = _aug()
    x, _ = _cases(0)
    got, _ = _edge(A, x, _draws(A, 3, [8 | 16, 31, 4 | 8 | 16], seed=4, scale=-1.0))
    assert (got == 0).all()                                                 # zeros, and the histogram passes them through


def test_edge_negative_scale_then_histogram():
    A = _aug()
    x, _ = _cases(0)
    got, want = _edge(A, x, _draws(A, 3, [8 | 16, 31, 2 | 8 | 16], seed=5, scale=[-1.75, -1.2, -2.0]))
    for b in range(3):                                                      # min and max swapped, the knots follow
        assert got[b].max() <= 0 and abs(got[b].min() - want[b].min()) <= BOUND * _e32() * (want[b].max() - want[b].min())


def test_edge_gamma_half_with_voxels_at_the_minimum():
    A = _aug()
    x, _ = _cases(2)
    assert (x == x.min()).sum() > 100
    got, want = _edge(A, x, _draws(A, 1, 4, seed=6, gamma=0.5))
    assert (got[x == x.min()] == x.min()).all()                             # 0 ** 0.5 * range + min
    _edge(A, x, _draws(A, 1, 2 | 4 | 16, seed=7, gamma=0.5))


# ------------------------------------------------------------------------------------------------ graph
def test_graph_replay_uses_the_draws_loaded_since():
    A = _aug()
    x, cases = _cases(0)
    xg = torch.from_numpy(x).to(DEV)
    d0, d1 = cases[0][0], cases[1][0]
    slot = A.IntensitySlot(3, DEV)
    slot.load(d0)
    out = torch.empty_like(xg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.augment_intensity(xg, slot, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        slot.load(d1)                                                       # ignored while recording
        A.augment_intensity(xg, slot, out=out)
    assert slot.draws is d0
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, _run(A, xg, d0))
    slot.load(d1)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, _run(A, xg, d1)) and not torch.equal(out, _run(A, xg, d0))


def test_device_arguments_are_checked_before_launch():
    A = _aug()
    slot = A.IntensitySlot(2, DEV)
    x = torch.rand(2, 1, 8, 8, 4, device=DEV)
    with pytest.raises(ValueError):
        A.augment_intensity(x, slot)                                        # nothing loaded
    slot.load(A.draw_intensity(np.random.RandomState(0), 2, prob=1.0))
    for bad in (x[:1], x.double(), x.permute(0, 1, 3, 2, 4), x[0]):
        with pytest.raises(ValueError):
            A.augment_intensity(bad, slot)
    with pytest.raises(ValueError):
        A.augment_intensity(x, slot, out=torch.empty(2, 1, 8, 8, 4))        # out on the host


# ------------------------------------------------------------------------------------------------ integration: phase 1
def _mv_setup():
    from mivp_amd import multiview as mv
    fx = load_fixture("mv_step_rrc")                                        # the smallest model shape of test_hip_multiview
    conf = Namespace(**fx.meta["conf"])
    x = fx["in"]["x"].to(DEV).contiguous()
    views = [mv.draw_views(np.random.RandomState(50 + s), x.shape[0], conf.roi_size, conf.masking_shape,
                           conf.masking_ratio, False) for s in range(3)]
    return mv, fx, conf, x, views


def _mv_model(fx, conf, capturable=False):
    from mivp_amd import train
    from mivp_amd.swin_unetr import SwinUnetR
    m = SwinUnetR(conf)
    m.load_state_dict(dict(fx["sd"]), strict=True)
    m.to(DEV).train()
    return m, train.build_optimizer(m, conf, capturable=capturable)


def _same_params(a, b):
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    return all(torch.equal(pa[k], pb[k]) for k in pa)


def test_multiview_step_with_augment():
    A = _aug()
    mv, fx, conf, x, views = _mv_setup()
    B = x.shape[0]
    some = _draws(A, B, [31, 2 | 4] + [16] * (B - 2), seed=8)
    runs = {}
    for tag, xin, aug in (("none", x, None), ("off", x, A.draw_intensity(np.random.RandomState(0), B, prob=0.0)),
                          ("some", x, some), ("pre", _run(A, x, some), None)):
        m, o = _mv_model(fx, conf)
        before = {k: p.detach().clone() for k, p in m.named_parameters()}
        vec = mv.multiview_step(m, o, None, conf, xin, views[0], augment=aug)
        torch.cuda.synchronize()
        runs[tag] = (m, vec.clone())
        assert any(not torch.equal(p, before[k]) for k, p in m.named_parameters())     # the step moved the parameters
    assert torch.equal(runs["none"][1], runs["off"][1]) and _same_params(runs["none"][0], runs["off"][0])
    assert torch.equal(runs["some"][1], runs["pre"][1]) and _same_params(runs["some"][0], runs["pre"][0])
    assert not torch.equal(runs["some"][1], runs["none"][1])                            # the augmentation reached the loss
    # a slot with draws loaded is taken as it is
    slot = A.IntensitySlot(B, DEV)
    slot.load(some)
    m, o = _mv_model(fx, conf)
    vec = mv.multiview_step(m, o, None, conf, x, views[0], augment=slot)
    assert torch.equal(vec, runs["some"][1])
    with pytest.raises(ValueError):                                                     # draws of another batch size
        mv.multiview_step(m, o, None, conf, x, views[0], augment=A.draw_intensity(np.random.RandomState(0), B + 1))


def test_graphed_multiview_step_with_augment_equals_eager_steps():
    A = _aug()
    mv, fx, conf, x, views = _mv_setup()
    B = x.shape[0]
    augs = [A.draw_intensity(np.random.RandomState(70 + s), B, prob=0.7) for s in range(3)]
    m_e, o_e = _mv_model(fx, conf, capturable=True)
    eager = [mv.multiview_step(m_e, o_e, None, conf, x, views[s], augment=augs[s]).clone() for s in range(3)]
    torch.cuda.synchronize()
    m_g, o_g = _mv_model(fx, conf, capturable=True)
    iv, ia = iter(views), iter(augs)
    x0 = x.clone()
    step = mv.graphed_multiview_step(m_g, o_g, None, conf, x, lambda: next(iv), warmup=2, augment=lambda: next(ia))
    out = step()
    torch.cuda.synchronize()
    assert torch.equal(out.clone(), eager[2]) and _same_params(m_e, m_g)
    assert step.augment_slot.draws is augs[2] and torch.equal(x, x0)                    # the fixed input is left alone


# ------------------------------------------------------------------------------------------------ integration: phase 2
def _st_setup():
    from mivp_amd import train, students_teacher as ST
    from mivp_amd.losses import ClusteredPrototypeLoss
    from mivp_amd.swin_unetr import SwinUnetR
    conf, size, batch = train.make_conf("cfg0")
    torch.manual_seed(9)
    base = ST.MomentumModel(conf, SwinUnetR).to(DEV).train()
    base.copy_state_dict()
    views = ST.synthetic_views(conf, batch, size, DEV, student_sizes=[32, 24])
    mk = lambda static: ClusteredPrototypeLoss(float(conf.reduction_factor), int(conf.k_means_iterations),   # noqa: E731
                                               float(conf.fwhm), static_jitter=static)
    return train, ST, conf, base, views, mk


JIT = [[[1, 0, 2, 1, 0, 3], [0, 2, 1, 1, 3, 0]], [[0, 0, 0, 0, 0, 0], [3, 3, 3, 3, 3, 3]], [[2, 1, 0, 3, 1, 2], [1, 1, 2, 0, 0, 1]]]


def test_students_teacher_step_with_augment_on_the_teacher_view():
    A = _aug()
    train, ST, conf, base, views, mk = _st_setup()
    B = views["image"].shape[0]
    some = _draws(A, B, [31] + [2 | 4 | 16] * (B - 1), seed=9)
    pre = dict(views, image=_run(A, views["image"], some))
    image0 = views["image"].clone()
    runs = {}
    for tag, batch, aug in (("none", views, None), ("off", views, A.draw_intensity(np.random.RandomState(0), B, prob=0.0)),
                            ("some", views, some), ("pre", pre, None)):
        m = copy.deepcopy(base)
        o = train.build_optimizer(m, conf)
        loss = ST.students_teacher_step(m, o, None, mk(False), conf, batch, jitters=JIT[0], augment=aug)
        torch.cuda.synchronize()
        runs[tag] = (m, loss.clone())
    assert not _same_params(runs["none"][0].net_student, base.net_student)              # the step moved the student
    assert torch.equal(runs["none"][1], runs["off"][1]) and _same_params(runs["none"][0], runs["off"][0])
    assert torch.equal(runs["some"][1], runs["pre"][1]) and _same_params(runs["some"][0], runs["pre"][0])
    assert not torch.equal(runs["some"][1], runs["none"][1])                            # the teacher saw the augmented view
    assert torch.equal(views["image"], image0)                                          # the batch is left alone


def test_graphed_students_teacher_step_with_augment_equals_eager_steps():
    A = _aug()
    train, ST, conf, base, views, mk = _st_setup()
    B = views["image"].shape[0]
    augs = [A.draw_intensity(np.random.RandomState(80 + s), B, prob=0.7) for s in range(3)]
    ref, own = copy.deepcopy(base), copy.deepcopy(base)
    o_ref = train.build_optimizer(ref, conf)
    l_ref = [float(ST.students_teacher_step(ref, o_ref, None, mk(False), conf, views, jitters=JIT[s], augment=augs[s]))
             for s in range(3)]
    o_own = train.build_optimizer(own, conf, capturable=True)
    ij, ia = iter(JIT), iter(augs)
    step = ST.graphed_students_teacher_step(own, o_own, None, mk(True), conf, views, jitters=lambda: next(ij), warmup=2,
                                            augment=lambda: next(ia))
    l_own = float(step())
    torch.cuda.synchronize()
    assert l_own == l_ref[2]
    assert _same_params(ref, own) and step.augment_slot.draws is augs[2]
