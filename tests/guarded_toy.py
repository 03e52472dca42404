"""A toy "wrapper module" for tests/test_guarded_host.py: allocates with torch.empty / torch.zeros like mivp_amd.ops and
fills the result with plain torch indexing on the CPU; ``defect`` injects the errors the guard exists to see."""
import torch


def _whole_buffer(t):
    """The allocation ``t`` lives in, flat, as elements of t's dtype (only the guarded allocator leaves room around t)."""
    return torch.tensor([], dtype=t.dtype).set_(t.untyped_storage())


def scaled_rows(x, defect=None):
    """out[r] = 2 * x[r] (f32 [rows, cols]) and the per-row sums (f32 [rows]), through a zeroed workspace."""
    rows, cols = x.shape
    out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)          # SITE out
    ws = torch.zeros(rows, dtype=torch.float32, device=x.device)                   # SITE ws
    sums = torch.empty_like(ws)                                                    # SITE sums
    stored = torch.ones(rows * cols, dtype=torch.bool)
    if defect == "skip":
        stored[cols + 1] = False                         # one interior element is never stored
    out.view(-1)[stored] = (2 * x).reshape(-1)[stored]
    ws += x.sum(1)
    sums.copy_(ws)
    if defect in ("past_end", "before_start"):
        base = _whole_buffer(out)
        first = (out.data_ptr() - base.data_ptr()) // 4
        base[first + rows * cols if defect == "past_end" else first - 1] = 7.0
    if defect == "scribble_input":
        x[0, 0] = -1.0
    return out, sums
