"""The cases of tests/test_gpu_draw_exact.py — shapes, row values, Philox seeds and offsets — shared with
tests/test_draw_ref_cpu.py, which checks on the host what the GPU cases take for granted: the slack cap
on every case's rows, and that the nucleus cases' seeds need a second round / a later proposal.

All sizes are small on purpose: they are the shapes at which the kernels' branches change (one vector,
exactly one span, a second span of one vector, a ragged third span, 7 spans; partial last vectors; both
sides of k_draw's and k_draw_lean's stage switches), not the workload's.

Row values (make_rows; row r of a case takes kind r mod the kinds that apply to its shape):
  normal  N(0, 3^2)
  flat    N(0, 0.02^2): every element has about equal width, so the order and the uniform decide the token
  hole    normal with one whole span at -inf (span r mod spans; needs two spans)
  tail    the only finite values lie in the ragged last span (needs a ragged last span after a whole one)

No GPU and no library import here; place(..., device=...) alone touches a device.
"""
import math
from types import SimpleNamespace

import torch

import row_edges as re_

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
OFFSETS = (3, 4, (1 << 33) + 5)          # several offsets per case, one past 2^32
ROW_BASES = (0, 5, 70001)                # the global row of the call's row 0, per offset
KINDS = ("normal", "flat", "hole", "tail")


def dt_name(dtype):
    return {BF16: "bf16", F16: "fp16", F32: "fp32"}[dtype]


def kinds_for(V, span_len, kinds=KINDS):
    n_span = (V + span_len - 1) // span_len
    ok = {"normal": True, "flat": True, "hole": n_span >= 2, "tail": n_span >= 2 and V % span_len != 0}
    return [k for k in kinds if ok[k]]


def make_rows(B, V, dtype, seed, span_len, kinds=KINDS):
    """([B, V] host tensor, the kind of every row)."""
    g = torch.Generator().manual_seed(seed)
    usable = kinds_for(V, span_len, kinds)
    n_span = (V + span_len - 1) // span_len
    x = torch.empty(B, V)
    names = []
    for r in range(B):
        kind = usable[r % len(usable)]
        x[r] = torch.randn(V, generator=g) * (0.02 if kind == "flat" else 3.0)
        if kind == "hole":
            c = r % n_span
            x[r, c * span_len:(c + 1) * span_len] = -math.inf
        elif kind == "tail":
            x[r, :(n_span - 1) * span_len] = -math.inf
        names.append(kind)
    return x.to(dtype), names


def place(x, layout, device):
    """x [B, V] on `device`: contiguous; "padded" (tests/row_edges.py: rows at a 16-byte stride inside a
    NaN-filled buffer); or "general": packed rows that start 2 bytes past a 16-byte boundary (16-bit) — rows
    k_draw_lean does not take."""
    if layout == "contiguous":
        return x.to(device)
    if layout == "padded":
        return re_.place(x, "padded", math.nan, device)
    assert layout == "general"
    B, V = x.shape
    buf = torch.zeros(B * V + 16, dtype=x.dtype, device=device)
    view = buf[1:1 + B * V].view(B, V)
    view.copy_(x.to(device))
    return view


def _case(kernel, B, V, dtype, **kw):
    c = SimpleNamespace(kernel=kernel, B=B, V=V, dtype=dtype, layout="contiguous", pin=0, T=1.0, proc="multinomial",
                        top_k=0, top_p=0.0, want_prob=False, offsets=OFFSETS, row_bases=ROW_BASES, mode="plain")
    c.__dict__.update(kw)
    c.noise_seed = 0x5EED0000 + 131 * V + B
    c.input_seed = 7919 * V + 17 * B + {BF16: 0, F16: 1, F32: 2}[dtype]
    extra = "".join(f"-{k}{v}" for k, v in (("nst", c.pin), ("T", c.T if c.T != 1.0 else 0), ("k", c.top_k),
                                            ("p", c.top_p)) if v)
    c.id = f"{kernel}-{c.proc}-V{V}-B{B}-{dt_name(dtype)}-{c.layout}{extra}" + ("" if c.mode == "plain" else f"-{c.mode}")
    return c


def lean_cases():
    out = []
    for dt in (BF16, F16):
        for V in (8, 2048, 2056, 4104, 12296):
            for B in (3, 64):
                out += [_case("lean", B, V, dt, pin=n) for n in (1, 2, 4)]
        for V in (2051, 4099):                    # a partial last vector, rows padded to a 16-byte stride
            out += [_case("lean", 3, V, dt, pin=n, layout="padded") for n in (1, 2, 4)]
    out.append(_case("lean", 129, 4104, BF16))    # unpinned: the default switch to 4 stages
    out.append(_case("lean", 129, 12296, F16))
    out.append(_case("lean", 3, 4104, BF16, mode="counter"))
    out.append(_case("lean", 3, 4104, F16, mode="graph", offsets=(11,), row_bases=(9,)))
    return out


def lean_span_len(c):
    return 2048 * (c.pin if c.pin else (1 if c.B <= 128 else 4))


def draw_cases():
    out = []
    for dt in (BF16, F16):
        for V in (8, 2048, 2056, 4104, 12296):    # the lean draw's values in rows it does not take
            out.append(_case("draw", 3, V, dt, layout="general", want_prob=True))
        out.append(_case("draw", 3, 4104, dt, T=0.7, want_prob=True))
        for V in (4104, 12296):
            out.append(_case("draw", 8, V, dt, proc="topk", top_k=50, T=0.8, want_prob=True))
            out.append(_case("draw", 8, V, dt, proc="nucleus", top_p=0.9, want_prob=True))
            out.append(_case("draw", 8, V, dt, proc="topknucleus", top_k=200, top_p=0.8, want_prob=True))
    # packed odd-length rows: row 0 is aligned, the stride is not, so k_draw runs its aligned T = 1 branch
    out.append(_case("draw", 3, 4099, BF16, want_prob=True))
    for V in (1000, 2048, 4099, 6150):            # fp32: 2 stages of 1024 elements
        out.append(_case("draw", 3, V, F32))
    out.append(_case("draw", 3, 4099, F32, T=0.7))
    # B·ceil(V / 2048) on both sides of 1024: one stage per span, then two
    out.append(_case("draw", 64, 12296, BF16, T=0.7, want_prob=True))
    out.append(_case("draw", 200, 12296, BF16, T=0.7, want_prob=True, offsets=OFFSETS[:2]))
    out.append(_case("draw", 200, 12296, F16, layout="general", want_prob=True, offsets=OFFSETS[:2]))
    return out


def draw_span_len(c):
    if c.dtype == F32:
        return 2048
    return 2048 if c.B * ((c.V + 2047) // 2048) <= 1024 else 4096


NUC_OFFSETS = tuple(range(20, 28))


def nuc_cases():
    return [_case("nuc", 32, V, dt, proc="nucleus", top_p=p, T=T, offsets=NUC_OFFSETS, row_bases=(3,) * 8)
            for dt in (BF16, F16) for V in (2048, 4104, 12296) for p in (0.5, 0.9) for T in (1.0, 0.7)]


def nuc_rows(c):
    """The peaked and tied-value rows of tests/test_gpu_draw.py's nucleus_case and, at top_p = 0.5, a
    near-flat row (about half its proposals are rejected); row r takes kind r mod their number."""
    from test_gpu_draw import nucleus_case
    kinds = ("peaked", "ties") + (("flat",) if c.top_p == 0.5 else ())
    g = torch.Generator().manual_seed(c.input_seed)
    rows, names = [], []
    for r in range(c.B):
        kind = kinds[r % len(kinds)]
        if kind == "flat":
            rows.append((torch.randn(c.V, generator=g) * 0.02).to(c.dtype))
        else:
            rows.append(nucleus_case(kind, c.V, c.dtype, c.input_seed + r))
        names.append(kind)
    return torch.stack(rows), names


def case_rows(c):
    if c.kernel == "nuc":
        return nuc_rows(c)
    span = lean_span_len(c) if c.kernel == "lean" else draw_span_len(c)
    return make_rows(c.B, c.V, c.dtype, c.input_seed, span)
