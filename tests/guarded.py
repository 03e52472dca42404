"""A guarded allocator for wrapper-level tests: where a kernel writes, and where it does not (DESIGN.md "Write extent").

``with guarded(ops, swin_ops, pattern=0xA5) as g:`` replaces the name ``torch`` of the given modules by a thin proxy for the
length of the block.  The proxy forwards everything to the real ``torch`` except the allocating calls the wrappers use
(``empty``, ``zeros``, ``full``, ``ones``, ``empty_like``, ``zeros_like``).  Each of those

  * allocates ONE flat byte buffer of ``band + nbytes + band`` bytes, ``band`` a multiple of 256 and at least
    ``max(64 KiB, nbytes)``: the interior keeps the alignment of a real allocation, and an overrun of up to one whole
    output lands in a band -- inside the test's own memory;
  * fills the bands, and for ``empty`` / ``empty_like`` the interior too, with the canary byte ``pattern``;
  * returns the interior viewed with the requested shape and dtype;
  * records the wrapper's source line with the buffer (which stays alive until the guard is dropped, so no later
    allocation of the run can land on a freed one).

Checks:

  ``g.check_bands()``              every band of every buffer is still the canary, bit for bit
  ``g.watch(*inputs)`` and
  ``g.check_inputs_untouched()``   the bits of every watched input are what they were
  ``g.canary(t)``                  boolean map of the elements of ``t`` that hold this run's canary in every byte
  ``g.unwritten(t)``               the two-pattern rule: a case runs twice, with canary 0xA5 and then 0x5A, the second guard
                                   built with ``previous=`` the first.  An element is unwritten if and only if it holds
                                   the run's canary in BOTH runs -- no assumption about the values a kernel can produce,
                                   for bf16, f32, int32 and uint8 alike.  ``t`` is a tensor of the second run: a view into
                                   a guarded buffer (matched with the buffer of the same ordinal of the first run), or any
                                   copy of one (clone, permute + contiguous; copies carry the bits) together with
                                   ``before=`` the same tensor of the first run.

``twice(fn, *modules, inputs=...)`` runs ``fn`` under both patterns and applies all of it (see there)."""
import dataclasses
import functools
import inspect
import os
import sys

import torch as _torch

PATTERNS = (0xA5, 0x5A)
MIN_BAND = 64 * 1024
_ALLOWED_KW = {"dtype", "device"}


class GuardError(AssertionError):
    """A failed check; ``findings`` holds one dict per finding (site, shape, dtype, side, offset, count ...)."""

    def __init__(self, message, findings):
        super().__init__(message)
        self.findings = findings


class Record:
    def __init__(self, ordinal, site, call, shape, dtype, base, band, nbytes, view):
        self.ordinal, self.site, self.call = ordinal, site, call
        self.shape, self.dtype = tuple(shape), dtype
        self.base, self.band, self.nbytes, self.view = base, band, nbytes, view

    def __repr__(self):
        return f"#{self.ordinal} torch.{self.call}({self.shape}, {str(self.dtype).replace('torch.', '')}) at {self.site}"

    def holds(self, t):
        """``t`` lies inside this record's interior."""
        if t.device != self.base.device or t.numel() == 0 or self.nbytes == 0:
            return False
        lo = self.view.data_ptr()
        return lo <= t.data_ptr() < lo + self.nbytes


def band_bytes(nbytes):
    return (max(MIN_BAND, nbytes) + 255) // 256 * 256


def bytes_of(t):
    """The bytes of ``t`` as uint8 [*t.shape, itemsize] (a copy when ``t`` is not contiguous)."""
    t = t.detach().contiguous()
    return t.reshape(-1).view(_torch.uint8).reshape(*t.shape, t.element_size())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(_torch.equal(bytes_of(a), bytes_of(b)))


class _Proxy:
    """``torch`` as a guarded module sees it."""

    def __init__(self, guard):
        object.__setattr__(self, "_guard", guard)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the guarded torch proxy is read-only")

    def empty(self, *a, **k):
        return self._guard._alloc("empty", a, k, None)

    def zeros(self, *a, **k):
        return self._guard._alloc("zeros", a, k, 0)

    def ones(self, *a, **k):
        return self._guard._alloc("ones", a, k, 1)

    def full(self, *a, **k):
        return self._guard._alloc("full", a, k, k["fill_value"] if "fill_value" in k else a[1])

    def empty_like(self, *a, **k):
        return self._guard._alloc("empty_like", a, k, None)

    def zeros_like(self, *a, **k):
        return self._guard._alloc("zeros_like", a, k, 0)


class guarded:
    def __init__(self, *modules, pattern=PATTERNS[0], previous=None):
        if not modules:
            raise ValueError("guarded() needs at least one module")
        if not 0 < int(pattern) < 256:
            raise ValueError("the canary is one non-zero byte")
        self.modules = modules
        self.pattern = int(pattern)
        self.previous = previous
        self.records = []
        self._inputs = []
        self._saved = None
        self._proxy = _Proxy(self)

    # -- the context ----------------------------------------------------------------------------
    def __enter__(self):
        self._saved = [m.__dict__.get("torch") for m in self.modules]
        for m, t in zip(self.modules, self._saved):
            if t is not _torch:
                raise RuntimeError(f"{m.__name__}.torch is not the torch module (a guard is already active?)")
        for m in self.modules:
            m.torch = self._proxy
        return self

    def __exit__(self, *exc):
        for m, t in zip(self.modules, self._saved):
            m.torch = t
        self._saved = None
        return False

    # -- allocation -----------------------------------------------------------------------------
    def _site(self):
        """file:line (function) of the innermost frame that runs in one of the guarded modules."""
        f = sys._getframe(3)
        dicts = [m.__dict__ for m in self.modules]
        while f is not None:
            if any(f.f_globals is d for d in dicts):
                return f"{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} ({f.f_code.co_name})"
            f = f.f_back
        return "<outside the guarded modules>"

    def _alloc(self, call, args, kwargs, fill):
        extra = set(kwargs) - _ALLOWED_KW - ({"fill_value"} if call == "full" else set())
        if extra:
            raise NotImplementedError(f"guarded torch.{call}: keyword(s) {sorted(extra)} are not handled")
        kw = dict(kwargs)
        device = kw.pop("device", None)
        if call.endswith("_like"):
            like = args[0]
            meta = getattr(_torch, call)(like, device="meta", **kw)
            if not meta.is_contiguous():
                raise NotImplementedError(f"guarded torch.{call} of a non-contiguous tensor (strides are preserved there)")
            device = like.device if device is None else device
        else:
            meta = getattr(_torch, call)(*args, device="meta", **kw)
        device = _torch.device("cpu" if device is None else device)
        nbytes = meta.numel() * meta.element_size()
        band = band_bytes(nbytes)
        base = _torch.empty(band + nbytes + band, dtype=_torch.uint8, device=device)
        base.fill_(self.pattern)
        view = base[band:band + nbytes].view(meta.dtype).view(meta.shape)
        if fill is not None:
            view.fill_(fill)
        assert nbytes == 0 or view.data_ptr() == base.data_ptr() + band
        self.records.append(Record(len(self.records), self._site(), call, meta.shape, meta.dtype, base, band, nbytes, view))
        return view

    # -- checks ---------------------------------------------------------------------------------
    def check_bands(self):
        """Every band still holds the canary.  A finding names the allocation site, shape and dtype, the side, the byte
        offset of the first (lowest-address) changed byte from the interior's edge -- negative in front of the interior,
        0 for the first byte behind it -- and how many bytes of that band changed."""
        findings = []
        for r in self.records:
            for side, lo, hi in (("front", 0, r.band), ("back", r.band + r.nbytes, 2 * r.band + r.nbytes)):
                changed = r.base[lo:hi] != self.pattern
                count = int(changed.count_nonzero())
                if count:
                    first = int(_torch.nonzero(changed)[0])
                    findings.append(dict(site=r.site, ordinal=r.ordinal, shape=r.shape, dtype=r.dtype, side=side,
                                         offset=first - r.band if side == "front" else first, count=count))
        if findings:
            lines = [f"  {f['side']} band of #{f['ordinal']} {f['shape']} {str(f['dtype']).replace('torch.', '')} allocated at "
                     f"{f['site']}: {f['count']} byte(s) changed, the first at byte offset {f['offset']:+d} from the "
                     f"interior's {'start' if f['side'] == 'front' else 'end'}" for f in findings]
            raise GuardError("write outside an allocation:\n" + "\n".join(lines), findings)

    def watch(self, *tensors):
        """Snapshot the bits of input tensors (None entries are skipped)."""
        for t in tensors:
            if t is not None and not any(t is seen for seen, _ in self._inputs):
                self._inputs.append((t, t.detach().clone()))

    def check_inputs_untouched(self):
        findings = []
        for k, (t, snap) in enumerate(self._inputs):
            diff = (bytes_of(t) != bytes_of(snap)).reshape(*t.shape, -1).any(-1)
            count = int(diff.count_nonzero())
            if count:
                first = tuple(int(i) for i in _torch.nonzero(diff)[0])
                findings.append(dict(input=k, shape=tuple(t.shape), dtype=t.dtype, first=first, count=count))
        if findings:
            lines = [f"  input {f['input']} {f['shape']} {str(f['dtype']).replace('torch.', '')}: {f['count']} element(s) changed, "
                     f"the first at index {f['first']}" for f in findings]
            raise GuardError("an input tensor was written:\n" + "\n".join(lines), findings)

    def record_of(self, t):
        for r in reversed(self.records):
            if r.holds(t):
                return r
        return None

    def canary(self, t):
        """Elements of ``t`` whose every byte is this run's canary."""
        return (bytes_of(t) == self.pattern).all(-1)

    def unwritten(self, t, before=None):
        """The two-pattern rule (module docstring).  Returns a boolean map shaped like ``t``."""
        prev = self.previous
        if prev is None:
            raise RuntimeError("unwritten() needs the guard of the first run: guarded(..., previous=first)")
        if prev.pattern == self.pattern:
            raise RuntimeError("the two runs must use different canary bytes")
        if before is None:
            r = self.record_of(t)
            if r is None:
                raise RuntimeError("unwritten(): the tensor is no view of a guarded buffer; pass before= the first run's tensor")
            if r.ordinal >= len(prev.records):
                raise GuardError(f"the second run allocated more buffers than the first ({r!r})", [])
            p = prev.records[r.ordinal]
            if (p.site, p.shape, p.dtype) != (r.site, r.shape, r.dtype):
                raise GuardError(f"allocation #{r.ordinal} differs between the runs: {p!r} against {r!r}", [])
            off = (t.data_ptr() - r.view.data_ptr()) // t.element_size()
            before = _torch.as_strided(p.view.reshape(-1), t.shape, t.stride(), off)
        if before.shape != t.shape or before.dtype != t.dtype:
            raise GuardError(f"the runs returned different tensors: {tuple(before.shape)} {before.dtype} against "
                             f"{tuple(t.shape)} {t.dtype}", [])
        return prev.canary(before) & self.canary(t)

    def describe(self, t):
        r = self.record_of(t)
        return repr(r) if r is not None else f"a copy {tuple(t.shape)} {str(t.dtype).replace('torch.', '')}"


def _flatten(res):
    """The tensors of a wrapper's result, in order, with names: tensors, None, and tuples / lists / dicts / dataclasses
    of them (fields that hold anything else are skipped)."""
    out = []

    def walk(v, name):
        if v is None:
            return
        if isinstance(v, _torch.Tensor):
            out.append((name, v))
        elif isinstance(v, dict):
            for k in v:
                walk(v[k], f"{name}[{k!r}]")
        elif isinstance(v, (tuple, list)):
            for i, u in enumerate(v):
                walk(u, f"{name}[{i}]")
        elif dataclasses.is_dataclass(v) and not isinstance(v, type):
            for f in dataclasses.fields(v):
                u = getattr(v, f.name)
                if isinstance(u, _torch.Tensor):
                    out.append((f"{name}.{f.name}", u))
    walk(res, "out")
    return out


def twice(fn, *modules, inputs=(), allow=None, deterministic=True, what=""):
    """Run ``fn()`` under ``guarded(*modules)`` with canary 0xA5 and then 0x5A, and assert

      (a) every band of every buffer of both runs is intact,
      (b) no element of a returned tensor is unwritten, except where ``allow(name, tensor)`` returns a boolean mask
          (``name`` as in ``out[1]`` / ``out[3]['wq']``) -- an exception the caller computes from the descriptor: elements
          without defined content, which may stay unwritten (or be written from other such elements),
      (c) the watched ``inputs`` are untouched,

    and, with ``deterministic``, that the written elements of the two runs are bit-equal.  ``fn`` returns tensors, None, or
    tuples / lists / dicts of them; results of arithmetic on a guarded buffer do not carry the canary, which is what the
    determinism clause is for: a sum over an unwritten element differs between the runs.  Returns the second run's result
    and its guard (for descriptor-level checks on internal buffers)."""
    runs = []
    prev = None
    for pattern in PATTERNS:
        with guarded(*modules, pattern=pattern, previous=prev) as g:
            g.watch(*inputs)
            res = fn()
            if any(t.is_cuda for _, t in _flatten(res)):
                _torch.cuda.synchronize()
        g.check_bands()
        g.check_inputs_untouched()
        runs.append((g, res))
        prev = g
    (g1, res1), (g2, res2) = runs
    if [(r.site, r.shape, r.dtype) for r in g1.records] != [(r.site, r.shape, r.dtype) for r in g2.records]:
        raise GuardError(f"{what}: the two runs allocated different buffers", [])
    findings = _compare(g2, _flatten(res1), _flatten(res2), (lambda name, b: allow(name, b)) if allow else None, deterministic, what)
    _raise_unwritten(findings, what)
    return res2, g2


def _raise_unwritten(findings, what):
    if findings:
        lines = [f"  {f['name']} ({f['site']}): {f['count']} element(s) {f['kind']}, the first at index {f['first']}" for f in findings]
        raise GuardError(f"{what}: elements never stored, or stored from memory that was never stored:\n" + "\n".join(lines), findings)


def _compare(g2, t1, t2, allow, deterministic, what):
    """Findings of the two-pattern rule and the determinism clause over two runs' named tensors."""
    if [n for n, _ in t1] != [n for n, _ in t2]:
        raise GuardError(f"{what}: the two runs returned different structures", [])
    findings = []
    for (name, a), (_, b) in zip(t1, t2):
        un = g2.unwritten(b, before=a)
        mask = allow(name, b) if allow is not None else None
        if mask is not None and mask.shape != un.shape:
            raise ValueError(f"{what}: the exception mask of {name} has shape {tuple(mask.shape)}, the tensor {tuple(un.shape)}")
        bad = un if mask is None else un & ~mask.to(un.device)
        count = int(bad.count_nonzero())
        if count:
            first = tuple(int(i) for i in _torch.nonzero(bad)[0])
            findings.append(dict(name=name, site=g2.describe(b), first=first, count=count, kind="unwritten"))
            continue
        if deterministic:
            diff = (bytes_of(a) != bytes_of(b)).any(-1) & ~un
            if mask is not None:                         # elements without defined content have no defined bits either
                diff &= ~mask.to(un.device)
            count = int(diff.count_nonzero())
            if count:
                first = tuple(int(i) for i in _torch.nonzero(diff)[0])
                findings.append(dict(name=name, site=g2.describe(b), first=first, count=count, kind="differs between the runs"))
    return findings


# ---------------------------------------------------------------------------------------------------------------------
# the same checks around code that calls the wrappers itself (an existing test body, with its own reference and assertion)
# ---------------------------------------------------------------------------------------------------------------------
IN_PLACE = ("running_mean", "running_var", "out")     # arguments the wrappers update by contract (BatchNorm running statistics,
#                                                       gemm_tn's accumulator): not held to "inputs untouched"


class Call:
    """One outermost call of a guarded module's function: its name, bound arguments and result."""

    def __init__(self, name, args, result):
        self.name, self.args, self.result = name, args, result


class spied:
    """Inside the block every function defined in the given modules is wrapped: the outermost call of each chain (a test
    calling ``ops.conv3d_wgrad``, not the ``gemm_tn`` that one calls) is recorded with its bound arguments and result,
    and its tensor arguments are handed to ``guard.watch``."""

    def __init__(self, guard, *modules):
        self.guard, self.modules = guard, modules
        self.calls, self._saved, self._depth = [], [], 0

    def _wrap(self, fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def spy(*a, **k):
            if self._depth:
                return fn(*a, **k)
            bound = sig.bind(*a, **k)
            for name, v in bound.arguments.items():
                if name not in IN_PLACE:
                    self.guard.watch(*[t for _, t in _flatten(v)])
            self._depth += 1
            try:
                res = fn(*a, **k)
            finally:
                self._depth -= 1
            self.calls.append(Call(fn.__name__, dict(bound.arguments), res))
            return res
        return spy

    def __enter__(self):
        names = {m.__name__ for m in self.modules}
        wrapped = {}
        for m in self.modules:
            for name, f in list(vars(m).items()):
                if inspect.isfunction(f) and f.__module__ in names and f.__name__ != "<lambda>":
                    if f not in wrapped:
                        wrapped[f] = self._wrap(f)
                    self._saved.append((m, name, f))
                    setattr(m, name, wrapped[f])
        return self

    def __exit__(self, *exc):
        for m, name, f in self._saved:
            setattr(m, name, f)
        self._saved = []
        return False


def twice_calls(fn, *modules, allow=None, deterministic=True, what=""):
    """``twice`` for a body that calls the wrappers itself and returns nothing -- an existing parity test, reference and
    assertion included: runs ``fn()`` under both canaries with every function of ``modules`` spied on, and asserts
    (a) the bands, (b) nothing unwritten in any tensor an outermost wrapper call returned, (c) every tensor argument of
    those calls untouched (IN_PLACE arguments apart), and that the two runs return the same bits.  ``allow(call)`` may
    return ``{result name: mask}`` for a ``Call`` (names as in ``twice``).  Returns the second run's calls and guard."""
    runs, prev = [], None
    for pattern in PATTERNS:
        with guarded(*modules, pattern=pattern, previous=prev) as g, spied(g, *modules) as s:
            fn()
            if _torch.cuda.is_available():
                _torch.cuda.synchronize()
        g.check_bands()
        g.check_inputs_untouched()
        runs.append((g, s.calls))
        prev = g
    (g1, c1), (g2, c2) = runs
    if [c.name for c in c1] != [c.name for c in c2]:
        raise GuardError(f"{what}: the two runs made different calls", [])
    if not c2:
        raise GuardError(f"{what}: no function of the guarded modules was called", [])
    findings = []
    for k, (a, b) in enumerate(zip(c1, c2)):
        masks = (allow(b) if allow is not None else None) or {}
        named = _flatten(b.result)
        unknown = set(masks) - {n for n, _ in named}
        if unknown:
            raise ValueError(f"{what}: exception masks for results {sorted(unknown)} that {b.name} does not return")
        for f in _compare(g2, _flatten(a.result), named, lambda name, t: masks.get(name), deterministic, what):
            f["name"] = f"call {k} {b.name}: {f['name']}"
            findings.append(f)
    _raise_unwritten(findings, what)
    return c2, g2
