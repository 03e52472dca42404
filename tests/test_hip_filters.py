"""GPU: noise, blur and low-resolution simulation (csrc/filters.hip through mivp_amd.augment) against tests/filters_ref.py.

Blur alone is bit-equal to the float32 restatement: the taps, the order of the sum and the rounding of every product and
sum are fixed, so there is nothing a tolerance would have to cover.

Everything with noise or low-res in it is compared by tolerance, the rule of test_hip_augment.py: per sample,
err = max |kernel - f64 oracle| / (max - min of the f64 output).  The yardstick E32 is the worst such error of the float32
numpy restatement against the float64 oracle over the same cases (every shape, every draw set, every sample), computed
here; the kernel must stay within 8 x E32 (device logf / cosf a few ulp off numpy's).  No case and no voxel is left out.

Exactness.  A sample without flags is bitwise the input while its neighbours are augmented; a low grid equal to the volume
and noise of std 0 give the input's bits; two runs, in place and out of place, and a graph replay after new draws were
loaded are bitwise equal to the eager result.

Integration.  ``augment=`` on the phase-1 step takes a list of draws of both kinds, applied in order."""
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

import filters_ref as R
from conftest import load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(3, 1, 13, 10, 9),        # odd sizes, mixed flags per sample, an axis of 9 for radius 8
          (2, 2, 8, 8, 1),          # two channels, an axis of length 1
          (1, 1, 40, 36, 33)]       # several workgroups per stage: tile seams along H (32) and W (32)
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
    """(x, [(draws, f64 oracle, f32 restatement)]) of one shape: 40 seeded draw sets, each step dropped with probability
    0.3.  Computed once and shared; nothing modifies it."""
    A = _aug()
    shape = SHAPES[si]
    x = _input(shape, 100 + si)
    out = []
    for k in range(N_DRAWS):
        d = A.draw_filters(np.random.RandomState(1000 * si + k), shape[0], shape[2:], prob=0.7)
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
    slot = slot if slot is not None else A.FilterSlot(x.shape[0], x.shape[1], tuple(x.shape[2:]), DEV)
    slot.load(d)
    return A.augment_filters(x, slot, out=out)


def _draws(A, shape, flags, seed=0, sigma=(0.25, 1.5), **kw):
    """All-on draws of a seed restricted to ``flags`` (one int or one per sample), single parameters overridden."""
    d = A.draw_filters(np.random.RandomState(seed), shape[0], shape[2:], prob=1.0, sigma=sigma)
    d.flags[:] = flags
    for k, v in kw.items():
        getattr(d, k)[:] = v
    return d


def _set_sigmas(A, d, sigmas):
    """Per axis H, W, D a sigma, or None for an axis that is not filtered, on every sample."""
    for a, s in enumerate(sigmas):
        d.radius[:, a], d.taps[:, a] = (0, 0.0) if s is None else A.gaussian_taps(s)
    return d


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _gpu(x):
    return torch.from_numpy(x).to(DEV)


# ------------------------------------------------------------------------------------------------ blur: bit-equal
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_blur_is_bit_equal_to_the_float32_restatement(si):
    A = _aug()
    shape = SHAPES[si]
    x, _ = _cases(si)
    xg = _gpu(x)
    slot = A.FilterSlot(shape[0], shape[1], shape[2:], DEV)
    sets = [_draws(A, shape, 2, seed=s) for s in range(6)]                               # drawn sigmas, one per axis and sample
    sets.append(_draws(A, shape, 2, seed=9, sigma=(2.0, 2.0)))                           # radius 8 everywhere: > the axes of 1, 8
    assert (sets[-1].radius == 8).all()
    sets.append(_set_sigmas(A, _draws(A, shape, 2), (0.4, 1.0, 2.1)))                    # a different sigma per axis
    for off in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):                    # radius 0 on one, two, three axes
        sets.append(_set_sigmas(A, _draws(A, shape, 2), [None if a in off else 0.8 + 0.3 * a for a in range(3)]))
    for d in sets:
        got = _run(A, xg, d, slot=slot).cpu().numpy()
        want = R.chain(x, d, np.float32)
        assert np.array_equal(_bits(got), _bits(want)), (d.radius.tolist(),)


def test_blur_of_a_one_hot_is_the_outer_product_of_the_taps():
    A = _aug()
    shape = (2, 1, 13, 10, 9)
    d = _set_sigmas(A, _draws(A, shape, 2), (0.7, 1.2, 0.45))
    (rh, rw, rd) = (int(r) for r in d.radius[0])
    th, tw, tz = (d.taps[0, a, 8 - r:8 + r + 1] for a, r in enumerate((rh, rw, rd)))
    x = np.zeros(shape, np.float32)
    x[0, 0, 6, 5, 4] = 1.0                                                                # interior (the W kernel is cut at 0 and 9)
    x[1, 0, 0, 0, 0] = 1.0                                                                # a corner: the border keeps one octant
    got = _run(A, _gpu(x), d).cpu().numpy()
    full = th[:, None, None] * (tw[None, :, None] * tz[None, None, :])                    # the pass order: D, then W, then H
    assert full.dtype == np.float32
    want = np.zeros(shape, np.float32)
    w_lo, w_hi = max(5 - rw, 0), min(5 + rw, 9)
    want[0, 0, 6 - rh:6 + rh + 1, w_lo:w_hi + 1, 4 - rd:4 + rd + 1] = full[:, w_lo - (5 - rw):w_hi - (5 - rw) + 1, :]
    want[1, 0, :rh + 1, :rw + 1, :rd + 1] = full[rh:, rw:, rd:]
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(got), _bits(R.chain(x, d, np.float32)))


# ------------------------------------------------------------------------------------------------ parity by tolerance
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_chain_matches_the_float64_oracle_within_8_e32(si):
    A = _aug()
    x, cases = _cases(si)
    e32 = _e32()
    xg = _gpu(x)
    slot = A.FilterSlot(x.shape[0], x.shape[1], x.shape[2:], DEV)
    worst = 0.0
    for d, w64, _ in cases:
        got = _run(A, xg, d, slot=slot).cpu().numpy()
        assert np.isfinite(got).all()
        worst = max(worst, max(R.rel_err(got[b], w64[b]) for b in range(d.batch)))
    print(f"[filters parity] shape {SHAPES[si]}: E32 {e32:.3e}, kernel {worst:.3e}, ratio {worst / e32:.2f} (bound {BOUND})")
    seen = {int(f) for d, _, _ in cases for f in d.flags}
    assert seen == set(range(8))                                     # all eight flag combinations occur
    assert 1e-8 < e32 < 1e-5, e32                                    # the yardstick is what single precision gives
    assert worst <= BOUND * e32, (worst, e32)


@pytest.mark.parametrize("flags", [1, 1 | 2, 4, 1 | 2 | 4])
def test_stages_match_the_oracle(flags):
    """Noise, noise + blur, low-res and the full chain on every sample, on every shape."""
    A = _aug()
    for si in range(len(SHAPES)):
        x, _ = _cases(si)
        d = _draws(A, SHAPES[si], flags, seed=flags)
        got = _run(A, _gpu(x), d).cpu().numpy()
        want = R.chain(x.astype(np.float64), d, np.float64)
        err = max(R.rel_err(got[b], want[b]) for b in range(d.batch))
        print(f"[filters stage {flags}] shape {SHAPES[si]}: kernel {err:.3e}, E32 {_e32():.3e}, ratio {err / _e32():.2f}")
        assert err <= BOUND * _e32(), (flags, si, err)
        assert not np.array_equal(got, x) or (flags == 4 and (d.low_size == np.asarray(SHAPES[si][2:])).all())


# ------------------------------------------------------------------------------------------------ exactness
def test_no_flag_sample_is_bitwise_the_input_between_augmented_neighbours():
    A = _aug()
    x, _ = _cases(0)
    xg = _gpu(x)
    d = _draws(A, SHAPES[0], [7, 0, 7], seed=3)
    got = _run(A, xg, d)
    assert torch.equal(got[1], xg[1])
    assert not torch.equal(got[0], xg[0]) and not torch.equal(got[2], xg[2])
    c = xg.clone()
    assert _run(A, c, d, out=c) is c and torch.equal(c, got)                            # the same in place
    off = _run(A, xg, A.draw_filters(np.random.RandomState(0), 3, SHAPES[0][2:], prob=0.0))
    assert torch.equal(off, xg) and off.data_ptr() != xg.data_ptr()


def test_neutral_parameters_give_the_inputs_bits():
    A = _aug()
    for si in range(len(SHAPES)):
        x, _ = _cases(si)
        xg = _gpu(x)
        d = _draws(A, SHAPES[si], 4, low_size=np.asarray(SHAPES[si][2:]))               # the low grid is the volume
        assert torch.equal(_run(A, xg, d), xg)
        d = _draws(A, SHAPES[si], 1, noise_std=0.0)                                     # x + (0 + 0 * g)
        assert torch.equal(_run(A, xg, d), xg)
        d = _set_sigmas(A, _draws(A, SHAPES[si], 2), (None, None, None))                # radius 0 on every axis
        assert torch.equal(_run(A, xg, d), xg)


@pytest.mark.parametrize("si", [0, 1])
def test_every_route_in_place_equals_out_of_place_and_a_second_run(si):
    """All eight flag words times the radius patterns that change which stages run (the D / W stage alone, the H stage
    alone, both, none): in place, out of place and a second run agree bit for bit, and the input is left alone."""
    A = _aug()
    shape = SHAPES[si]
    x, _ = _cases(si)
    xg = _gpu(x)
    slot = A.FilterSlot(shape[0], shape[1], shape[2:], DEV)
    out = torch.empty_like(xg)
    for flags in range(8):
        for sig in ((0.9, 0.6, 1.1), (0.9, None, None), (None, 0.6, 1.1), (None, None, 0.5), (None, None, None)):
            d = _set_sigmas(A, _draws(A, shape, flags, seed=flags), sig)
            a = _run(A, xg, d, slot=slot).clone()
            slot.load(d)
            count = torch.cuda.memory_stats()["allocation.all.allocated"]
            b = A.augment_filters(xg, slot, out=out)
            c = xg.clone()
            count_c = torch.cuda.memory_stats()["allocation.all.allocated"]
            r = A.augment_filters(c, slot, out=c)
            assert torch.cuda.memory_stats()["allocation.all.allocated"] == count_c == count + 1   # only the clone
            assert r is c and b is out
            assert torch.equal(a, b) and torch.equal(a, c), (flags, sig)
            want = R.chain(x.astype(np.float64), d, np.float64)
            assert max(R.rel_err(a[i].cpu().numpy(), want[i]) for i in range(shape[0])) <= BOUND * _e32(), (flags, sig)
    assert torch.equal(xg.cpu(), torch.from_numpy(x))


def test_two_runs_and_in_place_are_bitwise_equal_on_the_large_shape():
    A = _aug()
    x, cases = _cases(2)
    xg = _gpu(x)
    for d, _, _ in cases[:8]:
        a = _run(A, xg, d)
        b = _run(A, xg, d)
        c = xg.clone()
        _run(A, c, d, out=c)
        assert torch.equal(a, b) and torch.equal(a, c)


def test_graph_replay_uses_the_draws_loaded_since():
    A = _aug()
    x, cases = _cases(0)
    xg = _gpu(x)
    d0, d1 = _draws(A, SHAPES[0], [7, 2, 5], seed=1), _draws(A, SHAPES[0], [1, 6, 0], seed=2)
    slot = A.FilterSlot(3, 1, SHAPES[0][2:], DEV)
    slot.load(d0)
    out = torch.empty_like(xg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        A.augment_filters(xg, slot, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        slot.load(d1)                                                       # ignored while recording
        A.augment_filters(xg, slot, out=out)
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
    slot = A.FilterSlot(2, 1, (8, 8, 4), DEV)
    x = torch.rand(2, 1, 8, 8, 4, device=DEV)
    with pytest.raises(ValueError):
        A.augment_filters(x, slot)                                          # nothing loaded
    slot.load(A.draw_filters(np.random.RandomState(0), 2, (8, 8, 4), prob=1.0))
    bad = (x[:1], torch.rand(2, 1, 8, 4, 8, device=DEV), torch.rand(2, 2, 8, 8, 4, device=DEV), x.double(),
           torch.rand(2, 1, 8, 4, 8, device=DEV).permute(0, 1, 2, 4, 3), x[0])
    for t in bad:
        with pytest.raises(ValueError):
            A.augment_filters(t, slot)
    with pytest.raises(ValueError):
        A.augment_filters(x, slot, out=torch.empty(2, 1, 8, 8, 4))          # out on the host
    with pytest.raises(ValueError):
        slot.load(A.draw_filters(np.random.RandomState(0), 3, (8, 8, 4)))   # wrong batch
    with pytest.raises(ValueError):
        slot.load(A.draw_filters(np.random.RandomState(0), 2, (8, 8, 5), prob=0.0))   # a low grid of another volume


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


def test_multiview_step_with_a_list_of_augmentations():
    A = _aug()
    mv, fx, conf, x, views = _mv_setup()
    B = x.shape[0]
    inten = A.draw_intensity(np.random.RandomState(8), B, prob=1.0)
    filt = _draws(A, tuple(x.shape), [7] + [3] * (B - 1), seed=8)
    islot = A.IntensitySlot(B, DEV)
    islot.load(inten)
    pre_i = A.augment_intensity(x, islot)
    pre_if = _run(A, pre_i, filt)
    off = A.draw_filters(np.random.RandomState(0), B, tuple(x.shape[2:]), prob=0.0)
    runs = {}
    for tag, xin, aug in (("none", x, None), ("off", x, [off]), ("both", x, [inten, filt]), ("pre", pre_if, None),
                          ("swapped", x, (filt, inten)), ("bare", x, inten), ("pre_i", pre_i, None),
                          ("slots", x, [islot, filt])):
        m, o = _mv_model(fx, conf)
        vec = mv.multiview_step(m, o, None, conf, xin, views[0], augment=aug)
        torch.cuda.synchronize()
        runs[tag] = (m, vec.clone())
    same = lambda a, b: torch.equal(runs[a][1], runs[b][1]) and _same_params(runs[a][0], runs[b][0])   # noqa: E731
    assert same("none", "off")                                              # all flags off changes nothing
    assert same("both", "pre") and same("slots", "pre")                     # both, in the order given
    assert same("bare", "pre_i")                                            # a bare IntensityDraws as before
    assert not torch.equal(runs["both"][1], runs["bare"][1]) and not torch.equal(runs["both"][1], runs["swapped"][1])
    with pytest.raises(ValueError):                                         # draws of another batch size
        mv.multiview_step(m, o, None, conf, x, views[0], augment=[inten, A.draw_filters(np.random.RandomState(0), B + 1,
                                                                                        tuple(x.shape[2:]))])


def test_graphed_multiview_step_with_a_list_equals_eager_steps():
    A = _aug()
    mv, fx, conf, x, views = _mv_setup()
    B, dims = x.shape[0], tuple(x.shape[2:])
    ints = [A.draw_intensity(np.random.RandomState(70 + s), B, prob=0.7) for s in range(3)]
    filts = [A.draw_filters(np.random.RandomState(90 + s), B, dims, prob=0.7) for s in range(3)]
    assert all(f.flags.any() for f in filts)
    m_e, o_e = _mv_model(fx, conf, capturable=True)
    eager = [mv.multiview_step(m_e, o_e, None, conf, x, views[s], augment=[ints[s], filts[s]]).clone() for s in range(3)]
    torch.cuda.synchronize()
    m_g, o_g = _mv_model(fx, conf, capturable=True)
    iv, ii, jf = iter(views), iter(ints), iter(filts)
    x0 = x.clone()
    step = mv.graphed_multiview_step(m_g, o_g, None, conf, x, lambda: next(iv), warmup=2,
                                     augment=[lambda: next(ii), lambda: next(jf)])
    out = step()
    torch.cuda.synchronize()
    assert torch.equal(out.clone(), eager[2]) and _same_params(m_e, m_g)
    assert step.augment_slot[0].draws is ints[2] and step.augment_slot[1].draws is filts[2]
    assert isinstance(step.augment_slot[1], A.FilterSlot) and torch.equal(x, x0)        # the fixed input is left alone
