"""GPU tests of FusedAdamW's gradient-norm clipping and non-finite step skipping against tests/clip_ref.py (float64, CPU).

Entries under test, called through ``_lib.call`` on their own operands and through optim.FusedAdamW:
mivp_grad_sumsq_multi, mivp_grad_clip_plan, mivp_adamw_multi_clip, mivp_adamw_multi_clip_dev (csrc/proto.hip).

Bars:
  sumsq      integer-valued gradients: the record's f64 equals the integer; otherwise (SUMSQ_ADDS + 1) 2^-24 relative, per
             chunk and in total (tests/clip_ref.py derives it)
  norm       1 ulp (f32) of sqrt on exact sums, NORM_REL otherwise
  coef       2 ulp (f32) of the f64 formula on the record's own sumsq, and exactly 1.0 where the formula gives 1
  update     p, exp_avg, exp_avg_sq bit-equal to the plain mivp_adamw_multi on gradients multiplied by the record's coef
             beforehand, and inside adamw_ref64's propagated bounds on those gradients
Parameters, states and the chunk sums sit in guarded arenas (tests/test_hip_loss_optim.py's): a write outside them, or a
chunk sum left unwritten, fails the test.  A NaN or an infinity in a gradient is ordinary data here, not a fault."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref as K  # noqa: E402
from mivp_amd import _lib as L  # noqa: E402
from mivp_amd import optim  # noqa: E402
from test_hip_loss_optim import PATTERN, AdamArena, Arena, assert_same_bits, chunk_tables  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
IDX_1025 = 7                                                      # the 1025-element tensor of the ladder


def read_record(rec):
    raw = rec.cpu().numpy()
    f, u = raw.view(np.float32), raw.view(np.uint32)
    return dict(sumsq=float(raw.view(np.float64)[0]), norm=float(f[2]), coef=float(f[3]), nonfinite=int(u[4]), apply=int(u[5]),
                steps=int(raw[3]), clipped=int(raw[4]), skipped=int(raw[5]), max_norm_seen=float(f[12]))


def numel(shape):
    return int(math.prod(shape))


def chunk_sums64(grads):
    """float64 sum of squares of every 1024-element chunk, in the chunk table's order."""
    out = []
    for g in grads:
        x = g.detach().to(F64).cpu().reshape(-1) ** 2
        pad = (-x.numel()) % 1024
        out.append(torch.cat([x, torch.zeros(pad, dtype=F64)]).view(-1, 1024).sum(1))
    return torch.cat(out)


class Direct:
    """Tables, guarded chunk sums and a zeroed record for direct calls on ``sizes`` (tensors that all carry a gradient)."""

    def __init__(self, sizes, p=None, m=None, v=None, group_of=None):
        self.n = len(sizes)
        assert int(L.lib().mivp_sizeof_opt(0)) == 40 and int(L.lib().mivp_sizeof_opt(3)) == 56
        rows = np.zeros((self.n, 5), np.int64)
        for i, s in enumerate(sizes):
            rows[i] = (p[i].data_ptr() if p else 0, m[i].data_ptr() if m else 0, v[i].data_ptr() if v else 0, s,
                       group_of[i] if group_of else 0)
        self.tensors = torch.from_numpy(rows).to(DEV)
        chunks, begin = chunk_tables(sizes)
        self.chunks = torch.from_numpy(chunks).to(DEV)
        self.begin = (C.c_int32 * (self.n + 1))(*begin)
        self.n_chunks = begin[-1]
        self.partials = Arena([(self.n_chunks,)])
        self.rec = torch.zeros(7, dtype=torch.int64, device=DEV)

    def gptr(self, grads):
        assert len(grads) == self.n and all(g.is_cuda and g.dtype == F32 for g in grads)
        return (C.c_void_p * self.n)(*[g.data_ptr() for g in grads])

    def plan(self, grads, max_norm=None, skip=False, what="plan"):
        """(record, chunk sums): both new kernels, every chunk sum written, nothing around them touched."""
        self.partials.flat.view(torch.int32).fill_(PATTERN)
        L.call("mivp_grad_sumsq_multi", L.ptr(self.tensors), self.gptr(grads), self.n, self.begin, L.ptr(self.chunks),
               L.ptr(self.partials.t[0]), L.stream())
        L.call("mivp_grad_clip_plan", L.ptr(self.partials.t[0]), self.n_chunks, math.inf if max_norm is None else max_norm,
               int(skip), L.ptr(self.rec), L.stream())
        torch.cuda.synchronize()
        return read_record(self.rec), self.partials.done(what)[0]

    def step(self, grads, hyper, clip):
        h = np.ascontiguousarray(hyper, np.float32)
        hp = h.ctypes.data_as(C.POINTER(C.c_float))
        if clip:
            L.call("mivp_adamw_multi_clip", L.ptr(self.tensors), self.gptr(grads), self.n, self.begin, hp, h.shape[0],
                   L.ptr(self.chunks), L.ptr(self.rec), L.stream())
        else:
            L.call("mivp_adamw_multi", L.ptr(self.tensors), self.gptr(grads), self.n, self.begin, hp, h.shape[0],
                   L.ptr(self.chunks), L.stream())
        torch.cuda.synchronize()


def hyper_rows(step):
    return np.stack([K.adam_hyper_row(step=step, **grp) for grp in K.ADAM_GROUPS])


def check_record(rec, want_sumsq, max_norm, exact, what):
    """sumsq, norm and coef of a record against the float64 reference (see the module docstring)."""
    want_norm = math.sqrt(want_sumsq)
    print(f"[{what}] sumsq {rec['sumsq']!r} want {want_sumsq!r} (rel {abs(rec['sumsq'] - want_sumsq) / want_sumsq:.3e}), norm "
          f"{rec['norm']!r} want {want_norm!r}, coef {rec['coef']!r}")
    if exact:
        assert rec["sumsq"] == want_sumsq, what
        assert K.ulps32(rec["norm"], want_norm) <= 1.0, what
    else:
        assert abs(rec["sumsq"] - want_sumsq) <= K.SUMSQ_REL * want_sumsq, what
        assert abs(rec["norm"] - want_norm) <= K.NORM_REL * want_norm, what
    want_coef = K.coef64(math.sqrt(rec["sumsq"]), max_norm)
    if want_coef == 1.0:
        assert rec["coef"] == 1.0, what
    else:
        assert K.ulps32(rec["coef"], want_coef) <= 2.0, what
    assert rec["nonfinite"] == 0 and rec["apply"] == 1, what


def device_views(cpu_tensors):
    """The tensors on the device as views of one arena: odd gaps between them, so most start at an odd address."""
    return Arena([tuple(t.shape) for t in cpu_tensors], cpu_tensors).t


# ---------------------------------------------------------------------------------------------- 1. exact sums
def test_exact_sums_on_the_ladder():
    shapes = K.LADDER_SHAPES
    assert [s[0] for s in shapes[:10]] == [1, 7, 255, 256, 257, 1023, 1024, 1025, 2048, 3073]
    grads = K.integer_grads(shapes, seed=21)
    want = K.sumsq64(grads)
    assert want == float(int(want)) and want < 2.0 ** 53
    d = Direct([numel(s) for s in shapes])
    gd = device_views(grads)
    norm = math.sqrt(want)
    seen = K.Counters()
    for max_norm in (1.0, 0.75 * norm, 2.0 * math.ceil(norm), None):
        rec, part = d.plan(gd, max_norm, what=f"exact sums, max_norm {max_norm}")
        K.assert_equal_located(part, chunk_sums64(grads), "i", "chunk sums of integer gradients")
        check_record(rec, want, max_norm, True, f"exact sums, max_norm {max_norm}")
        assert (rec["coef"] < 1.0) == (max_norm is not None and max_norm < norm)
        seen.update(K.plan_ref(want, max_norm))
    assert (rec["steps"], rec["clipped"], rec["skipped"]) == (4, 2, 0) == (seen.steps, seen.clipped, seen.skipped)
    assert K.ulps32(rec["max_norm_seen"], norm) <= 1.0


# ---------------------------------------------------------------------------------------------- 2. general sums
def test_general_sums_within_the_derived_bound_and_reproducible():
    case = K.adam_case()
    for step, row in enumerate(case["grads"]):
        grads = [g for g in row if g is not None]
        d = Direct([g.numel() for g in grads])
        gd = device_views(grads)
        rec, part = d.plan(gd, 1.0, what=f"general sums, step {step}")
        want = chunk_sums64(grads)
        K.assert_within_located(part, want, K.SUMSQ_REL * want, "i", f"chunk sums, step {step}")
        check_record(rec, K.sumsq64(grads), 1.0, False, f"general sums, step {step}")
        rec2, part2 = d.plan(gd, 1.0, what="second run")
        assert_same_bits(part, part2, "chunk sums of two runs on the same gradients")
        assert np.float64(rec["sumsq"]).tobytes() == np.float64(rec2["sumsq"]).tobytes()
        assert (rec["norm"], rec["coef"]) == (rec2["norm"], rec2["coef"]) and rec2["steps"] == 2


# ---------------------------------------------------------------------------------------------- 3. tail and views
def test_nothing_behind_a_gradient_is_read_and_views_of_one_bucket():
    g = K.gen(22)
    one = torch.randn(1025, generator=g, dtype=F32)
    d = Direct([1025])
    clean, part_clean = d.plan([one.to(DEV)], 1.0, what="contiguous 1025")
    buf = torch.full((4096,), float("nan"), dtype=F32, device=DEV)
    buf[7:7 + 1025] = one.to(DEV)
    rec, part = d.plan([buf[7:7 + 1025]], 1.0, what="a 1025-element view with NaN on both sides")
    check_record(rec, K.sumsq64([one]), 1.0, False, "a view between NaN")
    assert_same_bits(part, part_clean, "chunk sums of the view and of the contiguous copy")
    assert rec["sumsq"] == clean["sumsq"] and rec["norm"] == clean["norm"]

    # every gradient a view of one flat buffer, back to back (the data-parallel bucket), NaN behind the last one
    grads = [x for x in K.adam_case()["grads"][0] if x is not None]
    sizes = [x.numel() for x in grads]
    flat = torch.full((sum(sizes) + 2048,), float("nan"), dtype=F32, device=DEV)
    flat[:sum(sizes)] = torch.cat([x.reshape(-1) for x in grads]).to(DEV)
    views, off = [], 0
    for x in grads:
        views.append(flat[off:off + x.numel()].view(x.shape))
        off += x.numel()
    db = Direct(sizes)
    rec_b, part_b = db.plan(views, 1.0, what="bucket views")
    rec_s, part_s = Direct(sizes).plan([x.to(DEV) for x in grads], 1.0, what="separate tensors")
    check_record(rec_b, K.sumsq64(grads), 1.0, False, "bucket views")
    assert_same_bits(part_b, part_s, "chunk sums of bucket views and of separate tensors")
    assert rec_b["sumsq"] == rec_s["sumsq"]


# ---------------------------------------------------------------------------------------------- 4. the clipped update
def fused(aa, capturable, **kw):
    """FusedAdamW on the arena's parameters and states (tests/test_hip_loss_optim.fused_adamw with the new options)."""
    case = aa.case
    params = [torch.nn.Parameter(p) for p in aa.p]
    assert all(q.data_ptr() == p.data_ptr() for q, p in zip(params, aa.p))
    used = sorted(set(case["group_of"]))
    assert used == list(range(len(used)))
    opt = optim.FusedAdamW([dict(params=[q for q, gi in zip(params, case["group_of"]) if gi == k], **K.ADAM_GROUPS[k])
                            for k in used], capturable=capturable, **kw)
    for i, q in enumerate(params):
        opt.state[q] = {"step": torch.tensor(0.0), "exp_avg": aa.m[i], "exp_avg_sq": aa.v[i]}
    return opt, params


class PlainTwin:
    """The same case in a second arena, stepped by the plain mivp_adamw_multi on the gradients it is handed."""

    def __init__(self, case):
        self.aa = AdamArena(case)
        self.live = [i for i in range(len(case["shapes"])) if i != case["no_grad"]]
        a = self.aa
        self.d = Direct([numel(case["shapes"][i]) for i in self.live], [a.p[i] for i in self.live], [a.m[i] for i in self.live],
                        [a.v[i] for i in self.live], [case["group_of"][i] for i in self.live])

    def step(self, scaled, step_no):
        self.d.step([scaled[i] for i in self.live], hyper_rows(step_no), clip=False)


def assert_arenas_equal(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        name = ("p", "exp_avg", "exp_avg_sq")[i % 3]
        K.assert_equal_located(a.reshape(-1), b.reshape(-1), "i", f"{what}, {name} of tensor {i // 3}")
        assert_same_bits(a, b, f"{what}, {name} of tensor {i // 3}")


def scaled_reference(states, scaled, case, step_no):
    hyper = hyper_rows(step_no)
    return [None if st is None else K.adamw_ref64(st, gs.cpu(), hyper[gi])
            for st, gs, gi in zip(states, scaled, case["group_of"])]


@pytest.mark.parametrize("capturable", [False, True], ids=["host_rows", "dev_rows"])
def test_clipped_update_against_the_plain_kernel_and_float64(capturable):
    case = K.adam_case()
    assert case["grads"][0][case["no_grad"]] is None
    aa = AdamArena(case)
    opt, params = fused(aa, capturable, max_grad_norm=1.0)
    twin = PlainTwin(case)
    states = [None if i == case["no_grad"] else K.AdamState(p) for i, p in enumerate(case["p0"])]
    for step, row in enumerate(case["grads"]):
        gd = [None if g is None else g.to(DEV) for g in row]
        for q, g in zip(params, gd):
            q.grad = g
        opt.step()
        torch.cuda.synchronize()
        rec = read_record(opt._clip_rec)
        check_record(rec, K.sumsq64(row), 1.0, False, f"step {step + 1}")
        assert rec["coef"] < 1.0 and float(opt.clip_coef) == rec["coef"] and float(opt.grad_norm) == rec["norm"]
        assert opt.clip_coef.dim() == 0 and opt.clip_coef.is_cuda and opt.grad_norm.dtype == F32
        coef = opt.clip_coef.clone()
        scaled = [None if g is None else g * coef for g in gd]                # one f32 rounding per element
        twin.step(scaled, step + 1)
        states = scaled_reference(states, [torch.zeros(1) if s is None else s for s in scaled], case, step + 1)
        got = aa.check(states, f"clipped step {step + 1}")                    # the float64 bounds, the untouched tensor, the guards
        assert_arenas_equal(got, twin.aa.arena.done("plain twin"), f"clipped step {step + 1} against the plain kernel")
    assert opt.clip_stats()["clipped"] == 3 and opt.clip_stats()["steps"] == 3


# ---------------------------------------------------------------------------------------------- 5. no-op equality
@pytest.mark.parametrize("capturable", [False, True], ids=["host_rows", "dev_rows"])
def test_options_that_do_nothing_leave_the_bits_of_the_plain_optimizer(capturable):
    case = K.adam_case()
    runs = {}
    for name, kw in (("plain", {}), ("high", dict(max_grad_norm=1e12)), ("skip", dict(skip_nonfinite=True))):
        aa = AdamArena(case)
        opt, params = fused(aa, capturable, **kw)
        for row in case["grads"][:2]:
            for q, g in zip(params, row):
                q.grad = None if g is None else g.to(DEV)
            opt.step()
        torch.cuda.synchronize()
        runs[name] = aa.arena.done(name)
        if kw:
            st = opt.clip_stats()
            assert (st["steps"], st["clipped"], st["skipped"]) == (2, 0, 0) and float(opt.clip_coef) == 1.0
    assert_arenas_equal(runs["high"], runs["plain"], "max_grad_norm above the norm")
    assert_arenas_equal(runs["skip"], runs["plain"], "skip_nonfinite alone on finite gradients")


# ---------------------------------------------------------------------------------------------- 6. more than 384 tensors
def test_more_tensors_than_one_launch_holds():
    case = K.adam_many_case()
    n = len(case["shapes"])
    sizes = [numel(s) for s in case["shapes"]]
    assert n == 400 and sizes[383] == 1025 and sizes[384] == 3073
    aa, bb = AdamArena(case), AdamArena(case)
    d = Direct(sizes, aa.p, aa.m, aa.v, case["group_of"])
    twin = Direct(sizes, bb.p, bb.m, bb.v, case["group_of"])
    states = [K.AdamState(p) for p in case["p0"]]
    for step, row in enumerate(case["grads"]):
        gd = [g.to(DEV) for g in row]
        rec, part = d.plan(gd, 1.0, what=f"400 tensors, step {step + 1}")
        want = chunk_sums64(row)
        K.assert_within_located(part, want, K.SUMSQ_REL * want, "i", f"chunk sums of 400 tensors, step {step + 1}")
        check_record(rec, K.sumsq64(row), 1.0, False, f"400 tensors, step {step + 1}")
        assert rec["coef"] < 1.0
        d.step(gd, hyper_rows(step + 1), clip=True)
        scaled = [g * d.rec.view(F32)[3] for g in gd]
        twin.step(scaled, hyper_rows(step + 1), clip=False)
        states = scaled_reference(states, scaled, case, step + 1)
        got = aa.check(states, f"400 tensors, clipped step {step + 1}")
        assert_arenas_equal(got, bb.arena.done("plain twin"), f"400 tensors, step {step + 1} against the plain kernel")


# ---------------------------------------------------------------------------------------------- 7. non-finite
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_gradient_skips_the_step(bad):
    case = K.adam_case()
    assert case["shapes"][IDX_1025] == (1025,)
    aa = AdamArena(case)
    opt, params = fused(aa, False, max_grad_norm=1.0, skip_nonfinite=True)
    row = [None if g is None else g.clone() for g in case["grads"][0]]
    row[IDX_1025][-1] = bad                                       # the LAST element: the one-element tail chunk
    for q, g in zip(params, row):
        q.grad = None if g is None else g.to(DEV)
    opt.step()
    torch.cuda.synchronize()
    got = aa.arena.done("skipped step")
    for i, p0 in enumerate(case["p0"]):
        assert_same_bits(got[3 * i], p0, f"p of tensor {i} after a skipped step")
        assert not bool(got[3 * i + 1].view(torch.int32).any()) and not bool(got[3 * i + 2].view(torch.int32).any()), i
    rec = read_record(opt._clip_rec)
    assert (rec["apply"], rec["nonfinite"], rec["skipped"], rec["clipped"], rec["steps"]) == (0, 1, 1, 0, 1)
    assert not math.isfinite(float(opt.grad_norm)) and rec["max_norm_seen"] == 0.0

    # the next, finite step: the clipped update of test 4, with the bias corrections of step 2 (the skipped step counted)
    twin = PlainTwin(case)
    gd = [None if g is None else g.to(DEV) for g in case["grads"][1]]
    for q, g in zip(params, gd):
        q.grad = g
    opt.step()
    torch.cuda.synchronize()
    rec = read_record(opt._clip_rec)
    check_record(rec, K.sumsq64(case["grads"][1]), 1.0, False, "the step after the skipped one")
    scaled = [None if g is None else g * opt.clip_coef for g in gd]
    twin.step(scaled, 2)
    states = [None if i == case["no_grad"] else K.AdamState(p) for i, p in enumerate(case["p0"])]
    states = scaled_reference(states, [torch.zeros(1) if s is None else s for s in scaled], case, 2)
    assert_arenas_equal(aa.check(states, "the step after the skipped one"), twin.aa.arena.done("plain twin"),
                        "the step after the skipped one against the plain kernel")
    st = opt.clip_stats()
    assert (st["steps"], st["clipped"], st["skipped"]) == (2, 1, 1) and st["last_norm"] == rec["norm"]


# ---------------------------------------------------------------------------------------------- 8. counters
def test_counters_over_five_steps():
    g = K.gen(23)
    shapes = [(1025,), (7,), (3, 5, 7)]
    base = [torch.randn(s, generator=g, dtype=F32) for s in shapes]
    unit = 1.0 / math.sqrt(K.sumsq64(base))
    params = [torch.nn.Parameter(torch.zeros(s, device=DEV)) for s in shapes]
    opt = optim.FusedAdamW(params, max_grad_norm=1.0, skip_nonfinite=True)
    seen = K.Counters()
    for scale, bad in ((10.0, False), (0.5, False), (3.0, True), (20.0, False), (0.1, False)):
        row = [b * (scale * unit) for b in base]
        if bad:
            row[0][-1] = float("nan")
        for q, x in zip(params, row):
            q.grad = x.to(DEV)
        opt.step()
        seen.update(K.plan_ref(K.sumsq64(row), 1.0, True))
    st = opt.clip_stats()
    assert (st["steps"], st["clipped"], st["skipped"]) == (5, 2, 1) == (seen.steps, seen.clipped, seen.skipped)
    assert abs(st["max_norm_seen"] - seen.max_norm_seen) <= K.NORM_REL * seen.max_norm_seen and 19.9 < st["max_norm_seen"] < 20.1
    assert abs(st["last_norm"] - 0.1) <= 1e-5 and set(st) == {"steps", "clipped", "skipped", "last_norm", "max_norm_seen"}
    assert all(bool(torch.isfinite(p).all()) for p in params)


# ---------------------------------------------------------------------------------------------- 9. recorded
def test_recorded_step_equals_the_eager_sequence():
    case = K.adam_case()
    base = [None if g is None else g for g in case["grads"][0]]
    norm = math.sqrt(K.sumsq64(base))
    max_norm = 100.0
    assert norm > 10.0 * max_norm

    def feed(kind):
        row = [None if g is None else g.clone() for g in base]
        if kind == "under":
            row = [None if g is None else g * (10.0 / norm) for g in row]
        elif kind == "nan":
            row[IDX_1025][-1] = float("nan")
        elif kind == "warm":
            row = [None if g is None else g * 0.5 for g in row]
        return row

    kw = dict(max_grad_norm=max_norm, skip_nonfinite=True)
    ga, ea = AdamArena(case), AdamArena(case)
    opt_g, par_g = fused(ga, True, **kw)
    opt_e, par_e = fused(ea, False, **kw)
    static = [None if g is None else torch.zeros_like(g, device=DEV) for g in base]
    for q, s in zip(par_g, static):
        q.grad = s

    def load(row):
        for s, g in zip(static, row):
            if s is not None:
                s.copy_(g.to(DEV))

    def eager(row, lr_scale):
        for grp in opt_e.param_groups:
            grp["lr"] = grp["lr"] * lr_scale
        for q, g in zip(par_e, row):
            q.grad = None if g is None else g.to(DEV)
        opt_e.step()

    load(feed("warm"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        opt_g.step()                                              # eager: state, tables, the record and the chunk sums
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager(feed("warm"), 1.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.step()                                              # recorded, not run: no step is counted
    with pytest.raises(RuntimeError, match="record"):
        opt_g.max_grad_norm = 5.0
    for kind, lr_scale in (("over", 0.5), ("nan", 3.0), ("under", 0.25)):
        load(feed(kind))
        for grp in opt_g.param_groups:
            grp["lr"] = grp["lr"] * lr_scale
        opt_g.advance()
        graph.replay()
        eager(feed(kind), lr_scale)
        torch.cuda.synchronize()
        assert_arenas_equal(ga.arena.done(f"replay {kind}"), ea.arena.done(f"eager {kind}"), f"replay '{kind}' against eager")
        rg, re_ = read_record(opt_g._clip_rec), read_record(opt_e._clip_rec)
        assert np.float64(rg["sumsq"]).tobytes() == np.float64(re_["sumsq"]).tobytes()
        assert {k: v for k, v in rg.items() if k not in ("sumsq", "norm", "coef")} == \
            {k: v for k, v in re_.items() if k not in ("sumsq", "norm", "coef")}
        assert (rg["apply"] == 0) == (kind == "nan") and (rg["coef"] < 1.0) == (kind == "over")
    assert opt_g.clip_stats() == opt_e.clip_stats()
    st = opt_g.clip_stats()
    assert (st["steps"], st["clipped"], st["skipped"]) == (4, 2, 1)
