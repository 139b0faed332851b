"""Inputs shared by tests/test_gpu_row_edges.py and its CPU companion tests/test_row_edges_cpu.py:
vocabularies below, at and above one 16-byte vector, one wave, one fp32 stage and one 2048-element
span; rows with `-inf` entries; and three row layouts inside a poisoned buffer.

Layouts (place): the rows of x [R, V] are copied into a 1-D buffer filled with `poison` (+inf or NaN)
and the returned tensor is a view of it.
  packed   rows back to back; a row start is 16-byte aligned only where V * itemsize % 16 == 0
  padded   row stride = V rounded up to a whole number of 16-byte vectors, plus one more vector: every
           row starts aligned whatever V is, and poison follows every row
  shifted  the packed rows one element further into the buffer
The first row starts MARGIN_BYTES (16; shifted: 16 + one element) into the buffer, so one vector of
poison lies before it, and at least one vector of poison follows the last row.  A kernel that lets
an element outside [0, V) of a row into a max, a sum, a histogram or a draw returns a flagged or
wrong row.

No GPU and no library import here; everything but `place(..., device=...)` runs on the host.
"""
import functools
import math
from types import SimpleNamespace

import torch

import perf_walk as pw
from oracle import specdec_ref as ref

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = (BF16, F16, F32)
V_GRID = (1, 2, 3, 4, 5, 7, 8, 9, 63, 65, 1023, 1025, 2047, 2049)
LAYOUTS = ("packed", "padded", "shifted")
MASKS = ("none", "half", "most")
MARGIN_BYTES = 16


def dt_name(dtype):
    return str(dtype).split(".")[-1]


def poison_of(*key):
    """+inf for half of the cases and NaN for the other half, fixed by the case's key."""
    h = sum((i + 1) * sum(str(k).encode()) for i, k in enumerate(key))
    return math.inf if h % 2 == 0 else math.nan


# ---------------------------------------------------------------- logits
def seed_of(*key):
    """The input seed of the case named by `key`."""
    return sum((i + 3) * sum(str(k).encode()) for i, k in enumerate(key)) % 100003


def logits(shape, dtype, seed, mask="none"):
    """randn * 3 rows (as the parity tests'); mask "half": V // 2 random entries of every row at -inf,
    "most": all but one (V <= 2) or two entries.  Every row keeps at least one finite entry."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * 3
    V = shape[-1]
    n_masked = {"none": 0, "half": V // 2, "most": V - min(V, 2 if V > 2 else 1)}[mask]
    if n_masked:
        flat = x.view(-1, V)
        for r in range(flat.shape[0]):
            flat[r, torch.randperm(V, generator=g)[:n_masked]] = -math.inf
    return x.to(dtype)


# ---------------------------------------------------------------- layouts
def layout_geometry(R, V, dtype, layout):
    """(first row's element offset, row stride in elements, buffer length in elements)."""
    item = torch.empty(0, dtype=dtype).element_size()
    vec = 16 // item
    margin = MARGIN_BYTES // item + (1 if layout == "shifted" else 0)
    stride = ((V + vec - 1) // vec + 1) * vec if layout == "padded" else V
    return margin, stride, margin + R * stride + 2 * vec


def place(x, layout, poison, device="cpu"):
    """x's rows ([..., V], any leading shape) in `layout` inside a poisoned buffer on `device`: a view
    with x's shape whose last axis is contiguous and whose rows lie `stride` elements apart."""
    V = x.shape[-1]
    lead = x.shape[:-1]
    R = int(math.prod(lead))
    margin, stride, n = layout_geometry(R, V, x.dtype, layout)
    buf = torch.full((n,), poison, dtype=x.dtype, device=device)
    rows = buf[margin:margin + R * stride].view(R, stride)[:, :V]
    rows.copy_(x.reshape(R, V))
    view = rows if len(lead) == 1 else buf[margin:margin + R * stride].view(*lead, stride)[..., :V]
    view.poisoned_buffer = buf        # keeps the geometry checkable (tests/test_row_edges_cpu.py)
    return view


def rows_aligned(*tensors):
    """Every row of every [B, V] tensor starts on a 16-byte boundary (what the vector paths need)."""
    for t in tensors:
        if t.data_ptr() % 16 or (t.shape[0] > 1 and t.stride(0) * t.element_size() % 16):
            return False
    return True


# ---------------------------------------------------------------- one ulp
def within_one_ulp(got, want):
    """Element-wise: got is want or one of its two neighbours in the tensors' dtype."""
    assert got.dtype == want.dtype
    if got.dtype == F32:
        up = torch.nextafter(want, torch.full_like(want, math.inf))
        dn = torch.nextafter(want, torch.full_like(want, -math.inf))
        return (got == want) | (got == up) | (got == dn)
    # non-negative 16-bit values: neighbours differ by one in the bit pattern
    gi, wi = got.view(torch.int16).int(), want.view(torch.int16).int()
    return (gi - wi).abs() <= 1


# ---------------------------------------------------------------- filler ranks
# The fp32 exponent argument (x - max) * log2(e) of a probability down to 2^-64 has magnitude < 64, so
# its ulp is 2^-18: two logits closer than that may round to one probability in fp32 arithmetic (the
# torch-CPU oracle's too), and equal probabilities rank by index.  Their exact probabilities differ by
# less than e^(2^-18) - 1 < 4e-6 (relative): a row with such a pair is a close call for a top-K ranking.
RANK_GAP = 2.0 ** -18
RANK_CLOSE_RTOL = 4e-6


def rank_close(row):
    """The row has two distinct finite logits less than RANK_GAP apart."""
    v = row.double()
    v = v[torch.isfinite(v)].unique()
    return bool(v.numel() > 1 and float((v[1:] - v[:-1]).min()) < RANK_GAP)


# ---------------------------------------------------------------- STREAM verify cases
STREAM_KINDS = ("greedy", "multi_t1", "multi_t07", "topk20", "nucleus09")
STREAM_DTYPES = (BF16, F32)
STREAM_BG = ((1, 1), (1, 4), (3, 1), (3, 4))
# Inputs on which the reference itself raises (a rejected draft whose residual (p - q)+ is all zero
# after rounding: sampling/speculative_decoding.py:167-168 divides 0 by 0 and torch.multinomial
# refuses the NaN row) cannot be compared on their integer outputs: such a case takes the next input
# seed on which every oracle variant runs.  Key: (V, dtype, B, γ, kind) -> how many seeds were passed
# over (tests/test_row_edges_cpu.py proves the table: the recorded seed runs, the ones before it raise).
STREAM_BUMPS = {
    (2, BF16, 3, 1, "multi_t07"): 1,
}


def stream_seed(V, dtype, B, gamma, kind, bump=None):
    bump = STREAM_BUMPS.get((V, dtype, B, gamma, kind), 0) if bump is None else bump
    return seed_of("spec", V, B, gamma, kind, *((bump,) if bump else ()))


# ---------------------------------------------------------------- PHILOX verify cases
PHILOX_V = (5, 8, 9, 65, 2047, 2049)
PHILOX_GAMMAS = (1, 4, 8)
PHILOX_DTYPES = (BF16, F16)
PHILOX_RULES = ("spec", "engine")
PHILOX_LAYOUTS = ("padded", "packed")
# selection -> batch (tests/test_gpu_gamma_edges.py's selected(); "fused" here turns the lean kernel
# off so that B = 8 reaches k_verify_fused)
PHILOX_SELS = {"lean": 8, "fused": 8, "ticket": 16, "two-launch": 16}
# the rules' Philox (seed, offset) bases of tests/test_gpu_gamma_edges.py
PHILOX_NOISE = {"spec": (0x1234_5678_9ABC, 5), "engine": (99, 1 << 33)}


def philox_keys():
    return [(rule, B, g, V, dtype) for rule in PHILOX_RULES for V in PHILOX_V for g in PHILOX_GAMMAS
            for dtype in PHILOX_DTYPES for B in (8, 16)]


def philox_host(rule, B, g, V, dtype, seed):
    """(case, ends, rows): perf_walk's edge case with input seed `seed`, the call's noise offset moved
    by `seed` (as tests/test_gpu_gamma_edges.py's CASE_SEEDS), and the host's per-row results."""
    case = pw.walk_case("edge", B, g, V, dtype, seed)
    nseed, off = PHILOX_NOISE[rule]
    off += seed
    if rule == "spec":
        return case, [], pw.host_rows(case, "spec", nseed, off, ())
    active = pw.active_mask(B)
    ends, _ = pw.engine_ends(case, nseed, off, 0, active)
    return case, ends, pw.host_rows(case, "engine", nseed, off, ends, 0, active)


def philox_seed_ok(rows, g):
    """The two conditions a recorded seed meets: no close call, and both an accepting and a rejecting
    row (accepting: the walk took at least one draft; rejecting: it turned one down)."""
    live = [r for r in rows if r.active]
    return (not any(r.close for r in live) and any(r.want > 0 for r in live)
            and any(r.rejected for r in live))


def find_philox_seed(rule, B, g, V, dtype, limit=400):
    for seed in range(limit):
        try:
            _, _, rows = philox_host(rule, B, g, V, dtype, seed)
        except AssertionError:      # perf_walk's own construction checks (a pivot row with p != q)
            continue
        if philox_seed_ok(rows, g):
            return seed
    raise LookupError((rule, B, g, V, dtype))


# lowest seed for which philox_seed_ok holds (tests/test_row_edges_cpu.py re-proves every entry).
# Key: (rule, B, γ, V, dtype).
PHILOX_SEEDS = {k: 0 for k in philox_keys()}
PHILOX_SEEDS.update({
    ("spec", 8, 1, 5, BF16): 1,      # seed 0: all eight one-draft walks accept
    ("spec", 8, 1, 5, F16): 1,
})


@functools.lru_cache(maxsize=None)
def philox_case(rule, B, g, V, dtype):
    seed = PHILOX_SEEDS[(rule, B, g, V, dtype)]
    case, ends, rows = philox_host(rule, B, g, V, dtype, seed)
    nseed, off = PHILOX_NOISE[rule]
    return SimpleNamespace(case=case, ends=ends, rows=rows, noise=(nseed, off + seed))


# ---------------------------------------------------------------- row-kernel processors
KINDS = {
    "greedy": ref.Processor("greedy"),
    "multi_t1": ref.Processor("multinomial", 1.0),
    "multi_t07": ref.Processor("multinomial", 0.7),
    "topk20": ref.Processor("topk", 1.0, 20),
    "topk50_t08": ref.Processor("topk", 0.8, 50),
    "nucleus09": ref.Processor("nucleus", 1.0, 0, 0.9),
    "nucleus05_t07": ref.Processor("nucleus", 0.7, 0, 0.5),
    "topknucleus": ref.Processor("topknucleus", 1.0, 50, 0.9),
}
KEEP_KINDS = ("topk", "nucleus", "topknucleus")     # their -1e20 fill raises in fp16


def kinds_for(dtype):
    return {k: p for k, p in KINDS.items() if dtype != F16 or p.kind not in KEEP_KINDS}


# ---------------------------------------------------------------- processor extremes
EXTREME_V = (9, 65, 2049, 4096)
EXTREME_DTYPES = (BF16, F32)
EXTREME_MASKS = MASKS + ("tied",)
BIG_V = 128256                      # one bf16 row batch at the production vocabulary
COLD_T = 0.05


def extreme_procs(V):
    """name -> processor: top_k at 1, around V and far above it; top_p at 0, next to 0, next to 1 and
    1; temperatures far from 1."""
    out = {}
    for k in (1, V - 1, V, V + 1, 10 ** 6):
        out[f"topk{k}"] = ref.Processor("topk", 1.0, k)
    for p in (0.0, 1e-6, 0.999, 1.0):
        out[f"nucleus{p:g}"] = ref.Processor("nucleus", 1.0, 0, p)
    out["multi_t005"] = ref.Processor("multinomial", COLD_T)
    out["multi_t5"] = ref.Processor("multinomial", 5.0)
    out["topknucleus_t005"] = ref.Processor("topknucleus", COLD_T, 3, 0.9)
    return out


def extreme_logits(R, V, dtype, mask):
    """The extremes' rows: logits() with its masks, and "tied": the row maximum at three places (one
    in the row's last vector), so top_k = 1 keeps three elements and top_p -> 0 the lowest index."""
    if mask != "tied":
        return logits((R, V), dtype, seed_of("extreme", V, mask), mask)
    x = logits((R, V), dtype, seed_of("extreme", V, mask)).float()
    top = x.max(-1, keepdim=True).values + 1.0
    for r in range(R):
        x[r, [(r + 1) % V, V // 2, V - 1]] = top[r]
    return x.to(dtype)


def kept_softmax(x, kept, temperature):
    """The exact softmax (fp64, rounded once to x's dtype) of x / T over the kept set."""
    y = (x.masked_fill(~kept, -math.inf) / temperature).double()
    return torch.softmax(y, dim=-1).to(x.dtype)


def dropped_mass(x, kept):
    """Σ over the dropped elements of the exact T = 1 softmax of x (what a nucleus cut at top_p = 1 may lose)."""
    return torch.softmax(x.double(), dim=-1).masked_fill(kept, 0).sum(-1)


def cold_deviation():
    """The largest relative deviation of the torch-arithmetic oracle (exact=False) from the exact one
    over the elements with exact p >= 1e-12, on the fp32 extremes' inputs at T = COLD_T (exp arguments
    of magnitude ~200: the argument's own rounding error, which the kernel's fp32 arithmetic shares)."""
    worst = 0.0
    for V in EXTREME_V:
        for mask in EXTREME_MASKS:
            x = extreme_logits(4, V, F32, mask)
            for name in ("multi_t005", "topknucleus_t005"):
                proc = extreme_procs(V)[name]
                proc = ref.Processor(proc.kind, proc.temperature, proc.top_k, proc.top_p, stable_ties=True)
                a, e = ref.process(x, proc, False).double(), ref.process(x, proc, True).double()
                big = e >= 1e-12
                worst = max(worst, float(((a - e).abs() / e)[big].max()))
    return worst


# measured by cold_deviation() (tests/test_row_edges_cpu.py recomputes it); the kernel's fp32 exp may
# round differently from torch's on the same argument error, so the GPU test allows it 4 x this where
# that exceeds test_probs_rows_close_to_oracle's rtol = 2e-6
COLD_DEVIATION_F32 = 8.8416803886867e-07
COLD_RTOL_F32 = max(2e-6, 4 * COLD_DEVIATION_F32)


def extreme_spec_seed(V, name):
    """Input seed of the extremes' check_spec case (B = 1, γ = 4); the reference raises on none of them
    (tests/test_row_edges_cpu.py)."""
    return seed_of("extreme-spec", V, name)
