"""tests/guarded.py can fail: a toy wrapper (tests/guarded_toy.py, CPU tensors, plain torch indexing) writes one element
past the end, one before the start, leaves one interior element unwritten, or scribbles on its input; each must be
reported at the right allocation site and offset, and the correct wrapper must pass.  Nothing here touches a GPU."""
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G  # noqa: E402
import guarded_toy as toy  # noqa: E402

ROWS, COLS = 5, 7


def site_line(tag):
    """Line number of the toy wrapper's allocation marked ``# SITE <tag>``."""
    hits = [i + 1 for i, line in enumerate(inspect.getsource(toy).splitlines()) if line.rstrip().endswith(f"# SITE {tag}")]
    assert len(hits) == 1
    return hits[0]


def x_case():
    return torch.arange(ROWS * COLS, dtype=torch.float32).reshape(ROWS, COLS) - 3.0


def test_site_lines_are_where_the_allocations_are():
    src = inspect.getsource(toy).splitlines()
    for tag, call in (("out", "torch.empty("), ("ws", "torch.zeros("), ("sums", "torch.empty_like(")):
        assert call in src[site_line(tag) - 1]


def test_correct_wrapper_passes_and_is_fully_described():
    x = x_case()
    (out, sums), g = G.twice(lambda: toy.scaled_rows(x), toy, inputs=(x,), what="toy")
    assert torch.equal(out, 2 * x) and torch.equal(sums, x.sum(1))
    assert toy.torch is torch                                             # the proxy is gone again
    assert [r.call for r in g.records] == ["empty", "zeros", "empty_like", "ones"]      # (ones: the toy's own index mask)
    assert [r.site for r in g.records[:3]] == [f"guarded_toy.py:{site_line(t)} (scaled_rows)" for t in ("out", "ws", "sums")]
    r = g.records[0]
    assert r.shape == (ROWS, COLS) and r.dtype == torch.float32 and r.nbytes == ROWS * COLS * 4
    assert r.band % 256 == 0 and r.band >= 64 * 1024 and r.base.numel() == 2 * r.band + r.nbytes
    assert r.view.data_ptr() == r.base.data_ptr() + r.band and r.view.is_contiguous()
    assert g.record_of(out) is r and g.record_of(sums[1:]) is g.records[2] and g.record_of(x) is None
    assert G.band_bytes(10 ** 6) >= 10 ** 6 and G.band_bytes(10 ** 6) % 256 == 0


def test_fills_and_dtypes():
    """empty / empty_like interiors hold the canary, zeros / ones / full their value; every dtype keeps its shape."""
    with G.guarded(toy, pattern=0x5A) as g:
        p = toy.torch
        assert p.bfloat16 is torch.bfloat16 and p.nn is torch.nn        # everything else is forwarded
        e = p.empty((3, 5), dtype=torch.bfloat16)
        el = p.empty_like(e)
        z = p.zeros(4, 2, dtype=torch.int32)
        zl = p.zeros_like(e)
        o = p.ones(3, dtype=torch.uint8)
        f = p.full((2, 2), 2.5)
        n = p.empty(0, dtype=torch.float32)
        with pytest.raises(NotImplementedError):
            p.empty(3, pin_memory=True)
        with pytest.raises(NotImplementedError):
            p.empty_like(torch.zeros(3, 4).t())
    assert toy.torch is torch
    assert e.shape == (3, 5) and e.dtype == torch.bfloat16 and bool(g.canary(e).all()) and bool(g.canary(el).all())
    assert e.view(torch.int16)[0, 0] == 0x5A5A
    assert z.dtype == torch.int32 and not bool(z.any()) and not bool(g.canary(z).any())
    assert zl.dtype == torch.bfloat16 and zl.shape == e.shape and not bool(zl.any())
    assert o.dtype == torch.uint8 and bool((o == 1).all())
    assert f.dtype == torch.float32 and bool((f == 2.5).all())
    assert n.numel() == 0 and len(g.records) == 7
    g.check_bands()


def test_two_patterns_are_needed_and_enough():
    """A kernel may legitimately store the first run's canary value: one run alone would call it unwritten, two do not."""
    value = torch.tensor([0xA5A5A5A5 - (1 << 32)], dtype=torch.int32).view(torch.float32)
    x = torch.full((ROWS, COLS), float(value) / 2)
    assert bool((2 * x).view(torch.int32).eq(0xA5A5A5A5 - (1 << 32)).all())
    with G.guarded(toy, pattern=0xA5) as g1:
        out1, _ = toy.scaled_rows(x)
    assert bool(g1.canary(out1).all())
    with G.guarded(toy, pattern=0x5A, previous=g1) as g2:
        out2, _ = toy.scaled_rows(x)
    assert not bool(g2.unwritten(out2).any())                             # matched through the records
    assert not bool(g2.unwritten(out2.clone(), before=out1.clone()).any())
    G.twice(lambda: toy.scaled_rows(x), toy, inputs=(x,))


@pytest.mark.parametrize("defect,side,offset", [("past_end", "back", 0), ("before_start", "front", -4)])
def test_write_outside_is_located(defect, side, offset):
    x = x_case()
    with pytest.raises(G.GuardError) as err:
        G.twice(lambda: toy.scaled_rows(x, defect), toy, inputs=(x,))
    (f,) = err.value.findings
    assert f["site"] == f"guarded_toy.py:{site_line('out')} (scaled_rows)"
    assert (f["side"], f["offset"], f["count"]) == (side, offset, 4)     # 7.0f = 00 00 E0 40: no byte equals the canary
    assert f["shape"] == (ROWS, COLS) and f["dtype"] == torch.float32
    msg = str(err.value)
    assert f"guarded_toy.py:{site_line('out')}" in msg and f"byte offset {offset:+d}" in msg and side in msg


def test_unwritten_element_is_located():
    x = x_case()
    with pytest.raises(G.GuardError) as err:
        G.twice(lambda: toy.scaled_rows(x, "skip"), toy, inputs=(x,))
    (f,) = err.value.findings
    assert f["kind"] == "unwritten" and f["name"] == "out[0]" and f["count"] == 1 and f["first"] == (1, 1)
    assert f"guarded_toy.py:{site_line('out')}" in f["site"]
    # an exception mask that covers exactly that element lets the case pass; one that misses it does not
    hole = torch.zeros(ROWS, COLS, dtype=torch.bool)
    hole[1, 1] = True
    G.twice(lambda: toy.scaled_rows(x, "skip"), toy, inputs=(x,), allow=lambda name, t: hole if name == "out[0]" else None)
    with pytest.raises(G.GuardError):
        G.twice(lambda: toy.scaled_rows(x, "skip"), toy, inputs=(x,), allow=lambda name, t: hole.roll(1, 1) if name == "out[0]" else None)


def test_value_derived_from_unwritten_memory_differs_between_the_runs():
    """Arithmetic destroys the canary; what is left is that the two runs disagree."""
    x = x_case()

    def fn():
        out, sums = toy.scaled_rows(x, "skip")
        return out.sum(1)
    with pytest.raises(G.GuardError) as err:
        G.twice(fn, toy, inputs=(x,))
    (f,) = err.value.findings
    assert f["kind"] == "differs between the runs" and f["first"] == (1,) and f["count"] == 1


def test_scribbled_input_is_located():
    x = x_case() + 10.0
    with pytest.raises(G.GuardError) as err:
        G.twice(lambda: toy.scaled_rows(x, "scribble_input"), toy, inputs=(x,))
    (f,) = err.value.findings
    assert f["input"] == 0 and f["first"] == (0, 0) and f["count"] == 1
    assert toy.torch is torch                                             # restored although the check raised


def test_twice_calls_spies_on_the_outermost_wrapper_calls():
    """A body that calls the wrapper and asserts its values itself: results and arguments are found by the spy."""
    x = x_case()

    def body(defect=None):
        out, sums = toy.scaled_rows(x, defect)
        assert torch.equal(sums, x.sum(1))
    calls, g = G.twice_calls(body, toy, what="toy body")
    assert [c.name for c in calls] == ["scaled_rows"] and calls[0].args["x"] is x and len(g.records) == 4
    assert toy.scaled_rows.__name__ == "scaled_rows" and not hasattr(toy.scaled_rows, "__wrapped__")     # the spies are gone
    with pytest.raises(G.GuardError) as err:
        G.twice_calls(lambda: body("skip"), toy)
    (f,) = err.value.findings
    assert f["kind"] == "unwritten" and f["name"] == "call 0 scaled_rows: out[0]" and f["first"] == (1, 1)
    with pytest.raises(G.GuardError) as err:
        G.twice_calls(lambda: toy.scaled_rows(x.clone(), "scribble_input"), toy)
    assert err.value.findings[0]["first"] == (0, 0)
    with pytest.raises(G.GuardError):
        G.twice_calls(lambda: toy.scaled_rows(x, "past_end"), toy)
    hole = torch.zeros(ROWS, COLS, dtype=torch.bool)
    hole[1, 1] = True
    G.twice_calls(lambda: body("skip"), toy, allow=lambda call: {"out[0]": hole} if call.name == "scaled_rows" else None)
    with pytest.raises(G.GuardError, match="no function of the guarded modules was called"):
        G.twice_calls(lambda: None, toy)
