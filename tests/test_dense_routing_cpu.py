"""CPU: the routing table of the decode projections - which native entries linear_decode, norm_linear_decode and
norm_qkv_rope_update of shadowkv_amd.tensor_op call, with which arguments, for bf16, FP8 and MXFP4 weights.

No GPU and no library: tensor_op.lib is replaced by a recorder whose every attribute logs (entry name, arguments) and returns 0,
tensor_op.current_stream_handle by `lambda: 0`; F.linear and the two dequantisers run on the CPU over zero weights.  A pointer
argument (the c_void_p positions of _lib._SIGS) is logged as the operand it belongs to - "x", "w", "w_scale", "out", ... by
data_ptr(), an address inside `out` / `h_out` as that buffer, 0 as None, any other address (a buffer the call allocated) as "new";
an integer argument or a result dimension equal to the case's K is logged as "K", which keeps the table to one row per route.
For every case the test compares, against the literal table at the end of this file,
  - the sequence of native entries with their arguments,
  - the shape of the result and whether it IS `out` / `h_out` / `x` or a new tensor,
  - the deltas of fp8_native_calls, fp8_fallback_calls, mxfp4_native_calls, mxfp4_fallback_calls,
  - for a refused call the ValueError text.
The table was recorded from the tensor_op.py that still had one dispatch path per weight format (`python
tests/test_dense_routing_cpu.py` prints it) and pasted in as data; the one dispatcher is held to it.

The cases.  Formats x ops x token rows 1, 2, 32, 33 x K 512, 992, 1024, 4096, 4160 (the smallest K on each side of every
format's predicate) x contiguous / non-contiguous x x contiguous / non-contiguous w (MXFP4: also a non-contiguous w_scale) x rows
modes (both "fallback", both "native") form the shape product; it is run once per option set.  The whole product of eight
options, three rows-mode values per keyword and two head sizes on top of it would be some 10^7 calls, so the option sets are:
nothing; each of bias, fuse_silu_mul, out=, h_out=, residual, range_max, near_pull, q_override alone; every pair and triple of
the options that share a check (fuse_silu_mul, bias, range_max, near_pull); out + h_out + residual together; and for
norm_qkv_rope_update head_dim 64 beside 128.  An option set other than "nothing" runs over the shape product with the
contiguity factor cut to {all contiguous, x not, w not}.  SPECIAL holds what lies outside that product: the mixed and the
invalid rows modes, near_pull with more than 8,192 output rows, and the inconsistent (w, w_scale) pairs.

A gap: the 2..32-row MXFP4 predicate requires x.is_cuda, so no CPU test reaches skv_linear_rows_mxfp4 from Python; the call
counters of tests/test_gpu_mxfp4_rows_model.py cover that route.  The device is not faked here."""
import functools
import itertools

import pytest
import torch

from shadowkv_amd import _lib, tensor_op

FORMATS = ("bf16", "fp8", "mxfp4")
OPS = ("linear", "norm", "qkv")
ROWS = (1, 2, 32, 33)
KS = (512, 992, 1024, 4096, 4160)
MODES = {"ff": ("fallback", "fallback"), "nn": ("native", "native"), "nf": ("native", "fallback"), "fn": ("fallback", "native"),
         "xf": ("bogus", "fallback"), "fx": ("fallback", "bogus"), "xx": ("bogus", "wrong"), "nx": ("native", "bogus")}
COUNTERS = ("fp8_native_calls", "fp8_fallback_calls", "mxfp4_native_calls", "mxfp4_fallback_calls")
# the options an op reads
OP_OPTIONS = {"linear": ("bias", "silu", "out", "near_pull"),
              "norm": ("bias", "silu", "out", "h_out", "residual", "range_max", "near_pull"),
              "qkv": ("bias", "residual", "q_override", "d64")}
CHECKED = ("silu", "bias", "range_max", "near_pull")        # the options that meet in one check


def option_sets(op):
    have = OP_OPTIONS[op]
    sets = [()] + [(o,) for o in have]
    shared = [o for o in CHECKED if o in have]
    sets += [c for n in (2, 3, 4) for c in itertools.combinations(shared, n)]
    if op == "norm":
        sets.append(("out", "h_out", "residual"))
    if op == "qkv":
        sets.append(("bias", "residual", "q_override"))
    return sets


def contiguities(fmt, full):
    c = [(True, "c"), (False, "c"), (True, "w")] + ([(False, "w")] if full else [])
    if fmt == "mxfp4":
        c.append((True, "s"))           # w contiguous, w_scale not
    return c


def groups():
    return [(op, fmt, opts) for op in OPS for fmt in FORMATS for opts in option_sets(op)]


def group_cases(op, fmt, opts):
    for rows, K, (xc, wc), mode in itertools.product(ROWS, KS, contiguities(fmt, not opts), ("ff", "nn")):
        yield dict(op=op, fmt=fmt, rows=rows, K=K, xc=xc, wc=wc, mode=mode, opts=opts)


# outside the product: (name, case)
def special_cases():
    for op, fmt in itertools.product(OPS, FORMATS):
        for mode in ("nf", "fn", "xf", "fx", "xx", "nx"):
            for rows in (1, 2):
                yield dict(op=op, fmt=fmt, rows=rows, K=4096, xc=True, wc="c", mode=mode, opts=())
    for fmt in FORMATS:                 # near_pull rides in a launch of at most 8,192 output rows
        for N in (8192, 8208):
            yield dict(op="linear", fmt=fmt, rows=1, K=1024, xc=True, wc="c", mode="ff", opts=("near_pull",), N=N)
    for op in OPS:                      # the (w, w_scale) pairs the checks refuse (and the one they do not: FP8 bytes, no scale)
        for pair in ("bf16_w_f32_scale", "fp8_no_scale", "fp8_scale_f16", "fp8_scale_short", "fp8_scale_strided", "mxfp4_no_scale",
                     "mxfp4_scale_f32", "mxfp4_scale_short", "mxfp4_w_1d", "mxfp4_k_off_block", "mxfp4_x_k_mismatch",
                     "mxfp4_f32_row_scale"):
            for rows in (1, 2):
                yield dict(op=op, fmt=pair.split("_")[0], rows=rows, K=4096, xc=True, wc="c", mode="nn", opts=(), pair=pair)


def strided(t):
    """The same values behind a last dimension of stride 2."""
    wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=torch.uint8 if t.element_size() == 1 else t.dtype).view(t.dtype)
    view = wide[..., ::2]
    view.copy_(t)
    return view


@functools.lru_cache(maxsize=None)
def weights(fmt, N, K, wc, pair=None):
    """(w, w_scale) of zeros; pair: an inconsistent one."""
    if fmt == "bf16":
        w, sc = torch.zeros(N, K, dtype=torch.bfloat16), None
    elif fmt == "fp8":
        w, sc = torch.zeros(N, K, dtype=torch.uint8).view(torch.float8_e4m3fn), torch.ones(N, dtype=torch.float32)
    else:
        w, sc = torch.zeros(N, K // 2, dtype=torch.uint8), torch.full((N, K // 32), 127, dtype=torch.uint8)
    if wc == "w":
        w = strided(w)
    if wc == "s":
        sc = strided(sc)
    if pair == "bf16_w_f32_scale":
        sc = torch.ones(N, dtype=torch.float32)
    elif pair in ("fp8_no_scale", "mxfp4_no_scale"):
        sc = None
    elif pair == "fp8_scale_f16":
        sc = sc.half()
    elif pair == "fp8_scale_short":
        sc = sc[:-1].clone()
    elif pair == "fp8_scale_strided":
        sc = strided(sc)
    elif pair in ("mxfp4_scale_f32", "mxfp4_f32_row_scale"):
        sc = torch.ones(N, dtype=torch.float32) if pair == "mxfp4_f32_row_scale" else sc.float()
    elif pair == "mxfp4_scale_short":
        sc = sc[:, :-1].clone()
    elif pair == "mxfp4_w_1d":
        w = w.reshape(-1)
    elif pair == "mxfp4_k_off_block":
        w, sc = w[:, :-8].clone(), sc
    return w, sc


class Recorder:
    """Stands in for the library: every attribute is a function that logs (entry, arguments) and returns 0."""

    def __init__(self):
        self.log, self.names, self.spans, self.K = [], {}, [], 0

    def operands(self, named, K):
        self.log, self.names, self.spans, self.K = [], {}, [], K
        for name, t in named.items():
            if t is not None:
                self.names[t.data_ptr()] = name
        for name in ("out", "h_out"):
            t = named.get(name)
            if t is not None:
                self.spans.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name))

    def label(self, p):
        if not p:
            return None
        if p in self.names:
            return self.names[p]
        for lo, hi, name in self.spans:
            if lo <= p < hi:
                return name
        return "new"

    def __getattr__(self, entry):
        types = _lib._SIGS[entry][1]

        def fn(*args):
            assert len(args) == len(types), (entry, len(args), len(types))
            self.log.append((entry,) + tuple(self.label(a) if t is _lib.c_p else "K" if a == self.K else a for a, t in zip(args, types)))
            return 0
        return fn


REC = Recorder()


@pytest.fixture(autouse=True)
def recorder(monkeypatch):
    monkeypatch.setattr(tensor_op, "lib", lambda: REC)
    monkeypatch.setattr(tensor_op, "current_stream_handle", lambda: 0)


def which(t, named):
    for name in ("out", "h_out", "x"):
        if named.get(name) is t:
            return name
    return "new"


def run_case(c):
    """The outcome of one case: ("ok", calls, results, counter deltas) or ("ValueError", text); results: (shape, identity) each."""
    op, fmt, rows, K, opts = c["op"], c["fmt"], c["rows"], c["K"], c["opts"]
    D = 64 if "d64" in opts else 128
    N = c.get("N") or (3 * D if op == "qkv" else 64)
    bf = torch.bfloat16
    w, sc = weights(fmt, N, K, c["wc"], c.get("pair"))
    xk = K + 32 if c.get("pair") == "mxfp4_x_k_mismatch" else K
    x = torch.zeros(rows, 1, xk, dtype=bf)
    if not c["xc"]:
        x = strided(x)
    silu = "silu" in opts
    No = N // 2 if silu else N
    named = dict(x=x, w=w, w_scale=sc, bias=torch.zeros(N, dtype=bf) if "bias" in opts else None,
                 out=torch.zeros(rows, 1, No, dtype=bf) if "out" in opts else None,
                 h_out=torch.zeros(rows, 1, xk, dtype=bf) if "h_out" in opts else None,
                 residual=torch.zeros(rows, 1, xk, dtype=bf) if "residual" in opts else None,
                 range_max=torch.zeros(N // 16, dtype=torch.int16) if "range_max" in opts else None,
                 early_state=torch.zeros(8, dtype=torch.uint8), v_host=torch.zeros(8, dtype=torch.uint8))
    near = (named["early_state"].data_ptr(), 2, 1, 8, 8, 4, named["v_host"].data_ptr(), 64, 1, 1) if "near_pull" in opts else None
    fp8_rows, mxfp4_rows = MODES[c["mode"]]
    kw = dict(w_scale=sc, fp8_rows=fp8_rows, mxfp4_rows=mxfp4_rows)
    if op != "linear":
        named["norm_w"] = torch.ones(xk, dtype=bf)
    if op == "qkv":
        named.update(cos_sin=torch.zeros(16, D, dtype=bf), pos=torch.zeros(rows, dtype=torch.int64), row_idx=torch.zeros(1, dtype=torch.int64),
                     k_cache=torch.zeros(rows, 1, 5, D, dtype=bf), v_cache=torch.zeros(rows, 1, 5, D, dtype=bf),
                     q_override=torch.zeros(rows, 1, 1, D, dtype=bf) if "q_override" in opts else None)
    REC.operands(named, xk)
    before = [getattr(tensor_op, n) for n in COUNTERS]
    try:
        if op == "linear":
            res = (tensor_op.linear_decode(x, w, named["bias"], silu, out=named["out"], near_pull=near, **kw),)
        elif op == "norm":
            res = tensor_op.norm_linear_decode(x, named["residual"], named["norm_w"], 1e-5, w, named["bias"], silu, out=named["out"],
                                               h_out=named["h_out"], range_max=named["range_max"], near_pull=near, **kw)
        else:
            res = tensor_op.norm_qkv_rope_update(x, named["residual"], named["norm_w"], 1e-5, w, named["bias"], named["cos_sin"],
                                                 named["pos"], named["row_idx"], named["k_cache"], named["v_cache"], 1, 1,
                                                 q_override=named["q_override"], **kw)
    except ValueError as e:
        assert [getattr(tensor_op, n) for n in COUNTERS] == before, "a refused call moved a counter"
        return ("ValueError", str(e))
    deltas = tuple(getattr(tensor_op, n) - b for n, b in zip(COUNTERS, before))
    return ("ok", tuple(REC.log), tuple((tuple("K" if n == xk else n for n in t.shape), which(t, named)) for t in res), deltas)


def case_id(c):
    return " ".join(f"{k}={v}" for k, v in c.items())


def code(i):
    return "0123456789abcdefghijklmnopqrstuvwxyz"[i // 36] + "0123456789abcdefghijklmnopqrstuvwxyz"[i % 36]


def group_name(g):
    return "-".join((g[0], g[1]) + (g[2] or ("plain",)))


@pytest.mark.parametrize("group", groups(), ids=group_name)
def test_routing(group):
    cases = list(group_cases(*group))
    codes = "".join(TABLE[group_name(group)].split())
    assert len(codes) == 2 * len(cases), "the table and the case list of this group differ in length"
    for i, c in enumerate(cases):
        want = OUTCOMES[int(codes[2 * i:2 * i + 2], 36)]
        assert run_case(c) == want, case_id(c)


def test_routing_special():
    cases = list(special_cases())
    assert len(cases) == len(SPECIAL)
    for c, (cid, want) in zip(cases, SPECIAL):
        assert case_id(c) == cid
        assert run_case(c) == OUTCOMES[want], cid


def record():
    """Print OUTCOMES, TABLE and SPECIAL as recorded from the tensor_op that is imported."""
    tensor_op.lib = lambda: REC
    tensor_op.current_stream_handle = lambda: 0
    outcomes, index = [], {}

    def idx(o):
        if o not in index:
            index[o] = len(outcomes)
            outcomes.append(o)
        return index[o]
    table = {}
    for g in groups():
        codes = [code(idx(run_case(c))) for c in group_cases(*g)]
        table[group_name(g)] = ["".join(codes[i:i + 60]) for i in range(0, len(codes), 60)]
    special = [(case_id(c), idx(run_case(c))) for c in special_cases()]
    assert len(outcomes) <= 36 * 36
    print("OUTCOMES = [")
    for i, o in enumerate(outcomes):
        print(f"    {o!r},  # {code(i)}")
    print("]\n\nTABLE = {")
    for name, lines in table.items():
        print(f"    {name!r}:\n        " + "\n        ".join(repr(s + (" " if j + 1 < len(lines) else "")) for j, s in enumerate(lines)) + ",")
    print("}\n\nSPECIAL = [")
    for cid, i in special:
        print(f"    ({cid!r}, {i}),")
    print("]")


if __name__ == "__main__":
    record()
    raise SystemExit(0)


# ---------------------------------------------------------------------------- the recorded table (data; see the docstring)
OUTCOMES = [
    ('ok', (('skv_gemv_bf16', 'w', 'x', None, 'new', 64, 'K', 0, None),), (((1, 1, 64), 'new'),), (0, 0, 0, 0)),  # 00
    ('ok', (), (((1, 1, 64), 'new'),), (0, 0, 0, 0)),  # 01
    ('ok', (('skv_linear_rows_bf16', 'w', 'x', None, 'new', 2, 64, 'K', 0, None),), (((2, 1, 64), 'new'),), (0, 0, 0, 0)),  # 02
    ('ok', (), (((2, 1, 64), 'new'),), (0, 0, 0, 0)),  # 03
    ('ok', (('skv_linear_rows_bf16', 'w', 'x', None, 'new', 32, 64, 'K', 0, None),), (((32, 1, 64), 'new'),), (0, 0, 0, 0)),  # 04
    ('ok', (), (((32, 1, 64), 'new'),), (0, 0, 0, 0)),  # 05
    ('ok', (), (((33, 1, 64), 'new'),), (0, 0, 0, 0)),  # 06
    ('ok', (('skv_gemv_bf16', 'w', 'x', 'bias', 'new', 64, 'K', 0, None),), (((1, 1, 64), 'new'),), (0, 0, 0, 0)),  # 07
    ('ok', (('skv_linear_rows_bf16', 'w', 'x', 'bias', 'new', 2, 64, 'K', 0, None),), (((2, 1, 64), 'new'),), (0, 0, 0, 0)),  # 08
    ('ok', (('skv_linear_rows_bf16', 'w', 'x', 'bias', 'new', 32, 64, 'K', 0, None),), (((32, 1, 64), 'new'),), (0, 0, 0, 0)),  # 09
    ('ok', (('skv_gemv_bf16', 'w', 'x', None, 'new', 64, 'K', 1, None),), (((1, 1, 32), 'new'),), (0, 0, 0, 0)),  # 0a
    ('ok', (('skv_silu_and_mul', 'new', 'new', 1, 32, None),), (((1, 1, 32), 'new'),), (0, 0, 0, 0)),  # 0b
    ('ok', (('skv_linear_rows_bf16', 'w', 'x', None, 'new', 2, 64, 'K', 1, None),), (((2, 1, 32), 'new'),), (0, 0, 0, 0)),  # 0c
    ('ok', (('skv_silu_and_mul', 'new', 'new', 2, 32, None),), (((2, 1, 32), 'new'),), (0, 0, 0, 0)),  # 0d
    ('ok', (('skv_linear_rows_bf16', 'w', 'x', None, 'new', 32, 64, 'K', 1, None),), (((32, 1, 32), 'new'),), (0, 0, 0, 0)),  # 0e
    ('ok', (('skv_silu_and_mul', 'new', 'new', 32, 32, None),), (((32, 1, 32), 'new'),), (0, 0, 0, 0)),  # 0f
    ('ok', (('skv_silu_and_mul', 'new', 'new', 33, 32, None),), (((33, 1, 32), 'new'),), (0, 0, 0, 0)),  # 0g
    ('ok', (('skv_gemv_bf16', 'w', 'x', None, 'out', 64, 'K', 0, None),), (((1, 1, 64), 'out'),), (0, 0, 0, 0)),  # 0h
    ('ok', (('skv_linear_rows_bf16', 'w', 'x', None, 'out', 2, 64, 'K', 0, None),), (((2, 1, 64), 'out'),), (0, 0, 0, 0)),  # 0i
    ('ok', (('skv_linear_rows_bf16', 'w', 'x', None, 'out', 32, 64, 'K', 0, None),), (((32, 1, 64), 'out'),), (0, 0, 0, 0)),  # 0j
    ('ok', (('skv_gemv_near_pull_bf16', 'w', 'x', None, 'new', 64, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 64), 'new'),), (0, 0, 0, 0)),  # 0k
    ('ValueError', 'near_pull rides in a one-token GEMV launch with at most 8,192 output rows'),  # 0l
    ('ok', (('skv_gemv_bf16', 'w', 'x', 'bias', 'new', 64, 'K', 1, None),), (((1, 1, 32), 'new'),), (0, 0, 0, 0)),  # 0m
    ('ok', (('skv_linear_rows_bf16', 'w', 'x', 'bias', 'new', 2, 64, 'K', 1, None),), (((2, 1, 32), 'new'),), (0, 0, 0, 0)),  # 0n
    ('ok', (('skv_linear_rows_bf16', 'w', 'x', 'bias', 'new', 32, 64, 'K', 1, None),), (((32, 1, 32), 'new'),), (0, 0, 0, 0)),  # 0o
    ('ok', (('skv_gemv_near_pull_bf16', 'w', 'x', 'bias', 'new', 64, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 64), 'new'),), (0, 0, 0, 0)),  # 0p
    ('ok', (), (((1, 1, 64), 'new'),), (0, 1, 0, 0)),  # 0q
    ('ok', (('skv_gemv_fp8', 'w', 'w_scale', 'x', None, 'new', 64, 'K', 0, None),), (((1, 1, 64), 'new'),), (1, 0, 0, 0)),  # 0r
    ('ok', (), (((2, 1, 64), 'new'),), (0, 1, 0, 0)),  # 0s
    ('ok', (('skv_linear_rows_fp8', 'w', 'w_scale', 'x', None, 'new', 2, 64, 'K', 0, None),), (((2, 1, 64), 'new'),), (1, 0, 0, 0)),  # 0t
    ('ok', (), (((32, 1, 64), 'new'),), (0, 1, 0, 0)),  # 0u
    ('ok', (('skv_linear_rows_fp8', 'w', 'w_scale', 'x', None, 'new', 32, 64, 'K', 0, None),), (((32, 1, 64), 'new'),), (1, 0, 0, 0)),  # 0v
    ('ok', (), (((33, 1, 64), 'new'),), (0, 1, 0, 0)),  # 0w
    ('ok', (('skv_gemv_fp8', 'w', 'w_scale', 'x', 'bias', 'new', 64, 'K', 0, None),), (((1, 1, 64), 'new'),), (1, 0, 0, 0)),  # 0x
    ('ok', (('skv_linear_rows_fp8', 'w', 'w_scale', 'x', 'bias', 'new', 2, 64, 'K', 0, None),), (((2, 1, 64), 'new'),), (1, 0, 0, 0)),  # 0y
    ('ok', (('skv_linear_rows_fp8', 'w', 'w_scale', 'x', 'bias', 'new', 32, 64, 'K', 0, None),), (((32, 1, 64), 'new'),), (1, 0, 0, 0)),  # 0z
    ('ok', (('skv_silu_and_mul', 'new', 'new', 1, 32, None),), (((1, 1, 32), 'new'),), (0, 1, 0, 0)),  # 10
    ('ok', (('skv_gemv_fp8', 'w', 'w_scale', 'x', None, 'new', 64, 'K', 1, None),), (((1, 1, 32), 'new'),), (1, 0, 0, 0)),  # 11
    ('ok', (('skv_silu_and_mul', 'new', 'new', 2, 32, None),), (((2, 1, 32), 'new'),), (0, 1, 0, 0)),  # 12
    ('ok', (('skv_linear_rows_fp8', 'w', 'w_scale', 'x', None, 'new', 2, 64, 'K', 1, None),), (((2, 1, 32), 'new'),), (1, 0, 0, 0)),  # 13
    ('ok', (('skv_silu_and_mul', 'new', 'new', 32, 32, None),), (((32, 1, 32), 'new'),), (0, 1, 0, 0)),  # 14
    ('ok', (('skv_linear_rows_fp8', 'w', 'w_scale', 'x', None, 'new', 32, 64, 'K', 1, None),), (((32, 1, 32), 'new'),), (1, 0, 0, 0)),  # 15
    ('ok', (('skv_silu_and_mul', 'new', 'new', 33, 32, None),), (((33, 1, 32), 'new'),), (0, 1, 0, 0)),  # 16
    ('ok', (), (((1, 1, 64), 'out'),), (0, 1, 0, 0)),  # 17
    ('ok', (('skv_gemv_fp8', 'w', 'w_scale', 'x', None, 'out', 64, 'K', 0, None),), (((1, 1, 64), 'out'),), (1, 0, 0, 0)),  # 18
    ('ok', (), (((2, 1, 64), 'out'),), (0, 1, 0, 0)),  # 19
    ('ok', (('skv_linear_rows_fp8', 'w', 'w_scale', 'x', None, 'out', 2, 64, 'K', 0, None),), (((2, 1, 64), 'out'),), (1, 0, 0, 0)),  # 1a
    ('ok', (), (((32, 1, 64), 'out'),), (0, 1, 0, 0)),  # 1b
    ('ok', (('skv_linear_rows_fp8', 'w', 'w_scale', 'x', None, 'out', 32, 64, 'K', 0, None),), (((32, 1, 64), 'out'),), (1, 0, 0, 0)),  # 1c
    ('ok', (), (((33, 1, 64), 'out'),), (0, 1, 0, 0)),  # 1d
    ('ok', (('skv_gemv_near_pull_fp8', 'w', 'w_scale', 'x', None, 'new', 64, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 64), 'new'),), (1, 0, 0, 0)),  # 1e
    ('ok', (('skv_gemv_fp8', 'w', 'w_scale', 'x', 'bias', 'new', 64, 'K', 1, None),), (((1, 1, 32), 'new'),), (1, 0, 0, 0)),  # 1f
    ('ok', (('skv_linear_rows_fp8', 'w', 'w_scale', 'x', 'bias', 'new', 2, 64, 'K', 1, None),), (((2, 1, 32), 'new'),), (1, 0, 0, 0)),  # 1g
    ('ok', (('skv_linear_rows_fp8', 'w', 'w_scale', 'x', 'bias', 'new', 32, 64, 'K', 1, None),), (((32, 1, 32), 'new'),), (1, 0, 0, 0)),  # 1h
    ('ok', (('skv_gemv_near_pull_fp8', 'w', 'w_scale', 'x', 'bias', 'new', 64, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 64), 'new'),), (1, 0, 0, 0)),  # 1i
    ('ok', (), (((1, 1, 64), 'new'),), (0, 0, 0, 1)),  # 1j
    ('ok', (('skv_gemv_mxfp4', 'w', 'w_scale', 'x', None, 'new', 64, 'K', 0, None),), (((1, 1, 64), 'new'),), (0, 0, 1, 0)),  # 1k
    ('ok', (), (((2, 1, 64), 'new'),), (0, 0, 0, 1)),  # 1l
    ('ok', (), (((32, 1, 64), 'new'),), (0, 0, 0, 1)),  # 1m
    ('ok', (), (((33, 1, 64), 'new'),), (0, 0, 0, 1)),  # 1n
    ('ok', (('skv_gemv_mxfp4', 'w', 'w_scale', 'x', 'bias', 'new', 64, 'K', 0, None),), (((1, 1, 64), 'new'),), (0, 0, 1, 0)),  # 1o
    ('ok', (('skv_silu_and_mul', 'new', 'new', 1, 32, None),), (((1, 1, 32), 'new'),), (0, 0, 0, 1)),  # 1p
    ('ok', (('skv_gemv_mxfp4', 'w', 'w_scale', 'x', None, 'new', 64, 'K', 1, None),), (((1, 1, 32), 'new'),), (0, 0, 1, 0)),  # 1q
    ('ok', (('skv_silu_and_mul', 'new', 'new', 2, 32, None),), (((2, 1, 32), 'new'),), (0, 0, 0, 1)),  # 1r
    ('ok', (('skv_silu_and_mul', 'new', 'new', 32, 32, None),), (((32, 1, 32), 'new'),), (0, 0, 0, 1)),  # 1s
    ('ok', (('skv_silu_and_mul', 'new', 'new', 33, 32, None),), (((33, 1, 32), 'new'),), (0, 0, 0, 1)),  # 1t
    ('ok', (), (((1, 1, 64), 'out'),), (0, 0, 0, 1)),  # 1u
    ('ok', (('skv_gemv_mxfp4', 'w', 'w_scale', 'x', None, 'out', 64, 'K', 0, None),), (((1, 1, 64), 'out'),), (0, 0, 1, 0)),  # 1v
    ('ok', (), (((2, 1, 64), 'out'),), (0, 0, 0, 1)),  # 1w
    ('ok', (), (((32, 1, 64), 'out'),), (0, 0, 0, 1)),  # 1x
    ('ok', (), (((33, 1, 64), 'out'),), (0, 0, 0, 1)),  # 1y
    ('ok', (('skv_gemv_near_pull_mxfp4', 'w', 'w_scale', 'x', None, 'new', 64, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 64), 'new'),), (0, 0, 1, 0)),  # 1z
    ('ok', (('skv_gemv_mxfp4', 'w', 'w_scale', 'x', 'bias', 'new', 64, 'K', 1, None),), (((1, 1, 32), 'new'),), (0, 0, 1, 0)),  # 20
    ('ok', (('skv_gemv_near_pull_mxfp4', 'w', 'w_scale', 'x', 'bias', 'new', 64, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 64), 'new'),), (0, 0, 1, 0)),  # 21
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', None, 'new', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 0, 0)),  # 22
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 0, 0)),  # 23
    ('ok', (('skv_norm_gemv_bf16', 'w', 'x', None, 'norm_w', 1e-05, None, None, 'new', 64, 'K', 0, None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (0, 0, 0, 0)),  # 24
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 2, 64, 'K', 0, None)), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (0, 0, 0, 0)),  # 25
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None),), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (0, 0, 0, 0)),  # 26
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 32, 64, 'K', 0, None)), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (0, 0, 0, 0)),  # 27
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None),), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (0, 0, 0, 0)),  # 28
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None),), (((33, 1, 'K'), 'new'), ((33, 1, 64), 'new')), (0, 0, 0, 0)),  # 29
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', 'bias', 'new', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 0, 0)),  # 2a
    ('ok', (('skv_norm_gemv_bf16', 'w', 'x', None, 'norm_w', 1e-05, None, 'bias', 'new', 64, 'K', 0, None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (0, 0, 0, 0)),  # 2b
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', 'bias', 'new', 2, 64, 'K', 0, None)), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (0, 0, 0, 0)),  # 2c
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', 'bias', 'new', 32, 64, 'K', 0, None)), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (0, 0, 0, 0)),  # 2d
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', None, 'new', 64, 'K', 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 32), 'new')), (0, 0, 0, 0)),  # 2e
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 1, 32, None)), (((1, 1, 'K'), 'new'), ((1, 1, 32), 'new')), (0, 0, 0, 0)),  # 2f
    ('ok', (('skv_norm_gemv_bf16', 'w', 'x', None, 'norm_w', 1e-05, None, None, 'new', 64, 'K', 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 32), 'new')), (0, 0, 0, 0)),  # 2g
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 2, 64, 'K', 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 32), 'new')), (0, 0, 0, 0)),  # 2h
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 2, 32, None)), (((2, 1, 'K'), 'new'), ((2, 1, 32), 'new')), (0, 0, 0, 0)),  # 2i
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 32, 64, 'K', 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 32), 'new')), (0, 0, 0, 0)),  # 2j
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 32, 32, None)), (((32, 1, 'K'), 'new'), ((32, 1, 32), 'new')), (0, 0, 0, 0)),  # 2k
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 33, 32, None)), (((33, 1, 'K'), 'new'), ((33, 1, 32), 'new')), (0, 0, 0, 0)),  # 2l
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', None, 'out', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'out')), (0, 0, 0, 0)),  # 2m
    ('ok', (('skv_norm_gemv_bf16', 'w', 'x', None, 'norm_w', 1e-05, None, None, 'out', 64, 'K', 0, None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'out')), (0, 0, 0, 0)),  # 2n
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'out', 2, 64, 'K', 0, None)), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'out')), (0, 0, 0, 0)),  # 2o
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'out', 32, 64, 'K', 0, None)), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'out')), (0, 0, 0, 0)),  # 2p
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', None, 'new', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 0, 0)),  # 2q
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 0, 0)),  # 2r
    ('ok', (('skv_norm_gemv_bf16', 'w', 'x', 'residual', 'norm_w', 1e-05, 'new', None, 'new', 64, 'K', 0, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 0, 0)),  # 2s
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 2, 64, 'K', 0, None)), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (0, 0, 0, 0)),  # 2t
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None),), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (0, 0, 0, 0)),  # 2u
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 32, 64, 'K', 0, None)), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (0, 0, 0, 0)),  # 2v
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None),), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (0, 0, 0, 0)),  # 2w
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 33, 'K', 1e-05, None),), (((33, 1, 'K'), 'new'), ((33, 1, 64), 'new')), (0, 0, 0, 0)),  # 2x
    ('ValueError', 'range_max: one token, hidden size 4096, N % 16 == 0, N <= 262,144, no fused SiLU'),  # 2y
    ('ok', (('skv_norm_gemv_rangemax_bf16', 'w', 'x', None, 'norm_w', 1e-05, None, None, 'new', 64, 'K', 'range_max', None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (0, 0, 0, 0)),  # 2z
    ('ValueError', 'near_pull rides in the one-token gate/up launch (hidden size 4096, fused SiLU * mul, no bias)'),  # 30
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', 'bias', 'new', 64, 'K', 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 32), 'new')), (0, 0, 0, 0)),  # 31
    ('ok', (('skv_norm_gemv_bf16', 'w', 'x', None, 'norm_w', 1e-05, None, 'bias', 'new', 64, 'K', 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 32), 'new')), (0, 0, 0, 0)),  # 32
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', 'bias', 'new', 2, 64, 'K', 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 32), 'new')), (0, 0, 0, 0)),  # 33
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', 'bias', 'new', 32, 64, 'K', 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 32), 'new')), (0, 0, 0, 0)),  # 34
    ('ok', (('skv_norm_gemv_near_pull_bf16', 'w', 'x', None, 'norm_w', 1e-05, None, 'new', 64, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 32), 'new')), (0, 0, 0, 0)),  # 35
    ('ok', (('skv_norm_gemv_rangemax_bf16', 'w', 'x', None, 'norm_w', 1e-05, None, 'bias', 'new', 64, 'K', 'range_max', None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (0, 0, 0, 0)),  # 36
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', None, 'out', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'out')), (0, 0, 0, 0)),  # 37
    ('ok', (('skv_norm_gemv_bf16', 'w', 'x', 'residual', 'norm_w', 1e-05, 'h_out', None, 'out', 64, 'K', 0, None),), (((1, 1, 'K'), 'h_out'), ((1, 1, 64), 'out')), (0, 0, 0, 0)),  # 38
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'out', 2, 64, 'K', 0, None)), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'out')), (0, 0, 0, 0)),  # 39
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'out', 32, 64, 'K', 0, None)), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'out')), (0, 0, 0, 0)),  # 3a
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 1, 0, 0)),  # 3b
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', None, 'new', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (1, 0, 0, 0)),  # 3c
    ('ok', (('skv_norm_gemv_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'new', 64, 'K', 0, None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (1, 0, 0, 0)),  # 3d
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None),), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (0, 1, 0, 0)),  # 3e
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 2, 64, 'K', 0, None)), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (1, 0, 0, 0)),  # 3f
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None),), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (0, 1, 0, 0)),  # 3g
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 32, 64, 'K', 0, None)), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (1, 0, 0, 0)),  # 3h
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None),), (((33, 1, 'K'), 'new'), ((33, 1, 64), 'new')), (0, 1, 0, 0)),  # 3i
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (1, 0, 0, 0)),  # 3j
    ('ok', (('skv_norm_gemv_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, 'bias', 'new', 64, 'K', 0, None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (1, 0, 0, 0)),  # 3k
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 2, 64, 'K', 0, None)), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (1, 0, 0, 0)),  # 3l
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 32, 64, 'K', 0, None)), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (1, 0, 0, 0)),  # 3m
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 1, 32, None)), (((1, 1, 'K'), 'new'), ((1, 1, 32), 'new')), (0, 1, 0, 0)),  # 3n
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', None, 'new', 64, 'K', 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 32), 'new')), (1, 0, 0, 0)),  # 3o
    ('ok', (('skv_norm_gemv_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'new', 64, 'K', 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 32), 'new')), (1, 0, 0, 0)),  # 3p
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 2, 32, None)), (((2, 1, 'K'), 'new'), ((2, 1, 32), 'new')), (0, 1, 0, 0)),  # 3q
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 2, 64, 'K', 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 32), 'new')), (1, 0, 0, 0)),  # 3r
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 32, 32, None)), (((32, 1, 'K'), 'new'), ((32, 1, 32), 'new')), (0, 1, 0, 0)),  # 3s
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 32, 64, 'K', 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 32), 'new')), (1, 0, 0, 0)),  # 3t
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 33, 32, None)), (((33, 1, 'K'), 'new'), ((33, 1, 32), 'new')), (0, 1, 0, 0)),  # 3u
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'out')), (0, 1, 0, 0)),  # 3v
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', None, 'out', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'out')), (1, 0, 0, 0)),  # 3w
    ('ok', (('skv_norm_gemv_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'out', 64, 'K', 0, None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'out')), (1, 0, 0, 0)),  # 3x
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None),), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'out')), (0, 1, 0, 0)),  # 3y
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'out', 2, 64, 'K', 0, None)), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'out')), (1, 0, 0, 0)),  # 3z
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None),), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'out')), (0, 1, 0, 0)),  # 40
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'out', 32, 64, 'K', 0, None)), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'out')), (1, 0, 0, 0)),  # 41
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None),), (((33, 1, 'K'), 'new'), ((33, 1, 64), 'out')), (0, 1, 0, 0)),  # 42
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 1, 0, 0)),  # 43
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', None, 'new', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (1, 0, 0, 0)),  # 44
    ('ok', (('skv_norm_gemv_fp8', 'w', 'w_scale', 'x', 'residual', 'norm_w', 1e-05, 'new', None, 'new', 64, 'K', 0, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (1, 0, 0, 0)),  # 45
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None),), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (0, 1, 0, 0)),  # 46
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 2, 64, 'K', 0, None)), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (1, 0, 0, 0)),  # 47
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None),), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (0, 1, 0, 0)),  # 48
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 32, 64, 'K', 0, None)), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (1, 0, 0, 0)),  # 49
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 33, 'K', 1e-05, None),), (((33, 1, 'K'), 'new'), ((33, 1, 64), 'new')), (0, 1, 0, 0)),  # 4a
    ('ok', (('skv_norm_gemv_rangemax_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'new', 64, 'K', 'range_max', None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (1, 0, 0, 0)),  # 4b
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 64, 'K', 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 32), 'new')), (1, 0, 0, 0)),  # 4c
    ('ok', (('skv_norm_gemv_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, 'bias', 'new', 64, 'K', 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 32), 'new')), (1, 0, 0, 0)),  # 4d
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 2, 64, 'K', 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 32), 'new')), (1, 0, 0, 0)),  # 4e
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 32, 64, 'K', 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 32), 'new')), (1, 0, 0, 0)),  # 4f
    ('ok', (('skv_norm_gemv_near_pull_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, 'new', 64, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 32), 'new')), (1, 0, 0, 0)),  # 4g
    ('ok', (('skv_norm_gemv_rangemax_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, 'bias', 'new', 64, 'K', 'range_max', None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (1, 0, 0, 0)),  # 4h
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'out')), (0, 1, 0, 0)),  # 4i
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', None, 'out', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'out')), (1, 0, 0, 0)),  # 4j
    ('ok', (('skv_norm_gemv_fp8', 'w', 'w_scale', 'x', 'residual', 'norm_w', 1e-05, 'h_out', None, 'out', 64, 'K', 0, None),), (((1, 1, 'K'), 'h_out'), ((1, 1, 64), 'out')), (1, 0, 0, 0)),  # 4k
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None),), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'out')), (0, 1, 0, 0)),  # 4l
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'out', 2, 64, 'K', 0, None)), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'out')), (1, 0, 0, 0)),  # 4m
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None),), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'out')), (0, 1, 0, 0)),  # 4n
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'out', 32, 64, 'K', 0, None)), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'out')), (1, 0, 0, 0)),  # 4o
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 33, 'K', 1e-05, None),), (((33, 1, 'K'), 'new'), ((33, 1, 64), 'out')), (0, 1, 0, 0)),  # 4p
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 0, 1)),  # 4q
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', None, 'new', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 1, 0)),  # 4r
    ('ok', (('skv_norm_gemv_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'new', 64, 'K', 0, None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (0, 0, 1, 0)),  # 4s
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None),), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (0, 0, 0, 1)),  # 4t
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None),), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (0, 0, 0, 1)),  # 4u
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None),), (((33, 1, 'K'), 'new'), ((33, 1, 64), 'new')), (0, 0, 0, 1)),  # 4v
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', 'bias', 'new', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 1, 0)),  # 4w
    ('ok', (('skv_norm_gemv_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, 'bias', 'new', 64, 'K', 0, None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (0, 0, 1, 0)),  # 4x
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 1, 32, None)), (((1, 1, 'K'), 'new'), ((1, 1, 32), 'new')), (0, 0, 0, 1)),  # 4y
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', None, 'new', 64, 'K', 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 32), 'new')), (0, 0, 1, 0)),  # 4z
    ('ok', (('skv_norm_gemv_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'new', 64, 'K', 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 32), 'new')), (0, 0, 1, 0)),  # 50
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 2, 32, None)), (((2, 1, 'K'), 'new'), ((2, 1, 32), 'new')), (0, 0, 0, 1)),  # 51
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 32, 32, None)), (((32, 1, 'K'), 'new'), ((32, 1, 32), 'new')), (0, 0, 0, 1)),  # 52
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_silu_and_mul', 'new', 'new', 33, 32, None)), (((33, 1, 'K'), 'new'), ((33, 1, 32), 'new')), (0, 0, 0, 1)),  # 53
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'out')), (0, 0, 0, 1)),  # 54
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', None, 'out', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'out')), (0, 0, 1, 0)),  # 55
    ('ok', (('skv_norm_gemv_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'out', 64, 'K', 0, None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'out')), (0, 0, 1, 0)),  # 56
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None),), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'out')), (0, 0, 0, 1)),  # 57
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None),), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'out')), (0, 0, 0, 1)),  # 58
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None),), (((33, 1, 'K'), 'new'), ((33, 1, 64), 'out')), (0, 0, 0, 1)),  # 59
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 0, 1)),  # 5a
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', None, 'new', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 1, 0)),  # 5b
    ('ok', (('skv_norm_gemv_mxfp4', 'w', 'w_scale', 'x', 'residual', 'norm_w', 1e-05, 'new', None, 'new', 64, 'K', 0, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'new')), (0, 0, 1, 0)),  # 5c
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None),), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'new')), (0, 0, 0, 1)),  # 5d
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None),), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'new')), (0, 0, 0, 1)),  # 5e
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 33, 'K', 1e-05, None),), (((33, 1, 'K'), 'new'), ((33, 1, 64), 'new')), (0, 0, 0, 1)),  # 5f
    ('ok', (('skv_norm_gemv_rangemax_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'new', 64, 'K', 'range_max', None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (0, 0, 1, 0)),  # 5g
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', 'bias', 'new', 64, 'K', 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 32), 'new')), (0, 0, 1, 0)),  # 5h
    ('ok', (('skv_norm_gemv_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, 'bias', 'new', 64, 'K', 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 32), 'new')), (0, 0, 1, 0)),  # 5i
    ('ok', (('skv_norm_gemv_near_pull_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, 'new', 64, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 32), 'new')), (0, 0, 1, 0)),  # 5j
    ('ok', (('skv_norm_gemv_rangemax_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, 'bias', 'new', 64, 'K', 'range_max', None),), (((1, 1, 'K'), 'x'), ((1, 1, 64), 'new')), (0, 0, 1, 0)),  # 5k
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None),), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'out')), (0, 0, 0, 1)),  # 5l
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', None, 'out', 64, 'K', 0, None)), (((1, 1, 'K'), 'new'), ((1, 1, 64), 'out')), (0, 0, 1, 0)),  # 5m
    ('ok', (('skv_norm_gemv_mxfp4', 'w', 'w_scale', 'x', 'residual', 'norm_w', 1e-05, 'h_out', None, 'out', 64, 'K', 0, None),), (((1, 1, 'K'), 'h_out'), ((1, 1, 64), 'out')), (0, 0, 1, 0)),  # 5n
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None),), (((2, 1, 'K'), 'new'), ((2, 1, 64), 'out')), (0, 0, 0, 1)),  # 5o
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None),), (((32, 1, 'K'), 'new'), ((32, 1, 64), 'out')), (0, 0, 0, 1)),  # 5p
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 33, 'K', 1e-05, None),), (((33, 1, 'K'), 'new'), ((33, 1, 64), 'out')), (0, 0, 0, 1)),  # 5q
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', None, 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 5r
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 5s
    ('ok', (('skv_qkv_gemv_rope_update', 'w', 'x', None, 'norm_w', 1e-05, None, None, 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 5t
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 2, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 5u
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 5v
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 32, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 5w
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 5x
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 5y
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', 'bias', 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 5z
    ('ok', (('skv_qkv_gemv_rope_update', 'w', 'x', None, 'norm_w', 1e-05, None, 'bias', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 60
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', 'bias', 'new', 2, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 61
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', 'bias', 'new', 32, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 62
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', None, 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 63
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 64
    ('ok', (('skv_qkv_gemv_rope_update', 'w', 'x', 'residual', 'norm_w', 1e-05, 'new', None, 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 65
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 2, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 66
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 67
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 32, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 68
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 69
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6a
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', None, 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6b
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6c
    ('ok', (('skv_qkv_gemv_rope_update', 'w', 'x', None, 'norm_w', 1e-05, None, None, 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6d
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 2, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6e
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6f
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 32, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6g
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6h
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6i
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', None, 'new', 192, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 64), 'new')), (0, 0, 0, 0)),  # 6j
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 64), 'new')), (0, 0, 0, 0)),  # 6k
    ('ok', (('skv_norm_gemv_bf16', 'w', 'x', None, 'norm_w', 1e-05, None, None, 'new', 192, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((1, 1, 'K'), 'x'), ((1, 1, 1, 64), 'new')), (0, 0, 0, 0)),  # 6l
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 2, 192, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 64), 'new')), (0, 0, 0, 0)),  # 6m
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 64), 'new')), (0, 0, 0, 0)),  # 6n
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', None, 'new', 32, 192, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 64), 'new')), (0, 0, 0, 0)),  # 6o
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 64), 'new')), (0, 0, 0, 0)),  # 6p
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 33, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 64), 'new')), (0, 0, 0, 0)),  # 6q
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_bf16', 'w', 'new', 'bias', 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6r
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6s
    ('ok', (('skv_qkv_gemv_rope_update', 'w', 'x', 'residual', 'norm_w', 1e-05, 'new', 'bias', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6t
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', 'bias', 'new', 2, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6u
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6v
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_bf16', 'w', 'new', 'bias', 'new', 32, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6w
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6x
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 0, 0, 0)),  # 6y
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 6z
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', None, 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 70
    ('ok', (('skv_qkv_gemv_rope_update_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 71
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 72
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 2, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 73
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 74
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 32, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 75
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 76
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 77
    ('ok', (('skv_qkv_gemv_rope_update_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, 'bias', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 78
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 2, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 79
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 32, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 7a
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 7b
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', None, 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 7c
    ('ok', (('skv_qkv_gemv_rope_update_fp8', 'w', 'w_scale', 'x', 'residual', 'norm_w', 1e-05, 'new', None, 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 7d
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 7e
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 2, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 7f
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 7g
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 32, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 7h
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 7i
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 7j
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', None, 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 7k
    ('ok', (('skv_qkv_gemv_rope_update_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 7l
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 7m
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 2, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 7n
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 7o
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 32, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 7p
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 7q
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 64), 'new')), (0, 1, 0, 0)),  # 7r
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', None, 'new', 192, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 64), 'new')), (1, 0, 0, 0)),  # 7s
    ('ok', (('skv_norm_gemv_fp8', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'new', 192, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((1, 1, 'K'), 'x'), ((1, 1, 1, 64), 'new')), (1, 0, 0, 0)),  # 7t
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 64), 'new')), (0, 1, 0, 0)),  # 7u
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 2, 192, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 64), 'new')), (1, 0, 0, 0)),  # 7v
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 64), 'new')), (0, 1, 0, 0)),  # 7w
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', None, 'new', 32, 192, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 64), 'new')), (1, 0, 0, 0)),  # 7x
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 33, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 64), 'new')), (0, 1, 0, 0)),  # 7y
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 7z
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 80
    ('ok', (('skv_qkv_gemv_rope_update_fp8', 'w', 'w_scale', 'x', 'residual', 'norm_w', 1e-05, 'new', 'bias', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 81
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 82
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 2, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 83
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 84
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_linear_rows_fp8', 'w', 'w_scale', 'new', 'bias', 'new', 32, 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (1, 0, 0, 0)),  # 85
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 1, 0, 0)),  # 86
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 87
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', None, 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 1, 0)),  # 88
    ('ok', (('skv_qkv_gemv_rope_update_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 1, 128), 'new')), (0, 0, 1, 0)),  # 89
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8a
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8b
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8c
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', 'bias', 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 1, 0)),  # 8d
    ('ok', (('skv_qkv_gemv_rope_update_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, 'bias', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 1, 128), 'new')), (0, 0, 1, 0)),  # 8e
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8f
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', None, 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 1, 0)),  # 8g
    ('ok', (('skv_qkv_gemv_rope_update_mxfp4', 'w', 'w_scale', 'x', 'residual', 'norm_w', 1e-05, 'new', None, 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 1, 0)),  # 8h
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8i
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8j
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8k
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8l
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', None, 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 1, 0)),  # 8m
    ('ok', (('skv_qkv_gemv_rope_update_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'x'), ((1, 1, 1, 128), 'new')), (0, 0, 1, 0)),  # 8n
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8o
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8p
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8q
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 64), 'new')), (0, 0, 0, 1)),  # 8r
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', None, 'new', 192, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 64), 'new')), (0, 0, 1, 0)),  # 8s
    ('ok', (('skv_norm_gemv_mxfp4', 'w', 'w_scale', 'x', None, 'norm_w', 1e-05, None, None, 'new', 192, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 1, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((1, 1, 'K'), 'x'), ((1, 1, 1, 64), 'new')), (0, 0, 1, 0)),  # 8t
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 2, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 64), 'new')), (0, 0, 0, 1)),  # 8u
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 32, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 64), 'new')), (0, 0, 0, 1)),  # 8v
    ('ok', (('skv_add_rmsnorm', 'x', None, 'norm_w', None, 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', None, 'new', 'k_cache', 'v_cache', 33, 1, 1, 64, 64, 16, 320, 320, 5, 2, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 64), 'new')), (0, 0, 0, 1)),  # 8w
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 8x
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 1, 'K', 1e-05, None), ('skv_gemv_mxfp4', 'w', 'w_scale', 'new', 'bias', 'new', 384, 'K', 0, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 1, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 1, 0)),  # 8y
    ('ok', (('skv_qkv_gemv_rope_update_mxfp4', 'w', 'w_scale', 'x', 'residual', 'norm_w', 1e-05, 'new', 'bias', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 'K', 1, 1, 128, 128, 16, 640, 5, 1, None),), (((1, 1, 'K'), 'new'), ((1, 1, 1, 128), 'new')), (0, 0, 1, 0)),  # 8z
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 2, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 2, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((2, 1, 'K'), 'new'), ((2, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 90
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 32, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 32, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((32, 1, 'K'), 'new'), ((32, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 91
    ('ok', (('skv_add_rmsnorm', 'x', 'residual', 'norm_w', 'new', 'new', 33, 'K', 1e-05, None), ('skv_qkv_rope_update', 'new', 'cos_sin', 'pos', 'row_idx', 'q_override', 'new', 'k_cache', 'v_cache', 33, 1, 1, 128, 128, 16, 640, 640, 5, 1, None)), (((33, 1, 'K'), 'new'), ((33, 1, 1, 128), 'new')), (0, 0, 0, 1)),  # 92
    ('ValueError', "fp8_rows must be one of ('fallback', 'native'), got 'bogus'"),  # 93
    ('ValueError', "mxfp4_rows must be one of ('fallback', 'native'), got 'bogus'"),  # 94
    ('ok', (('skv_gemv_near_pull_bf16', 'w', 'x', None, 'new', 8192, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 8192), 'new'),), (0, 0, 0, 0)),  # 95
    ('ok', (('skv_gemv_near_pull_fp8', 'w', 'w_scale', 'x', None, 'new', 8192, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 8192), 'new'),), (1, 0, 0, 0)),  # 96
    ('ok', (('skv_gemv_near_pull_mxfp4', 'w', 'w_scale', 'x', None, 'new', 8192, 'K', 'early_state', 2, 1, 8, 8, 4, 'v_host', 64, 1, 1, None),), (((1, 1, 8192), 'new'),), (0, 0, 1, 0)),  # 97
    ('ValueError', 'w_scale goes with float8_e4m3fn weights'),  # 98
    ('ValueError', 'w_scale must be a contiguous f32 vector with one entry per weight row'),  # 99
    ('ValueError', 'MXFP4 weights uint8 [N, K / 2] = (64, 2048) go with e8m0 scales uint8 [N, K / 32] = (64, 128) with K % 32 == 0, got None'),  # 9a
    ('ValueError', 'MXFP4 weights uint8 [N, K / 2] = (64, 2048) go with e8m0 scales uint8 [N, K / 32] = (64, 128) with K % 32 == 0, got (torch.float32, (64, 128))'),  # 9b
    ('ValueError', 'MXFP4 weights uint8 [N, K / 2] = (64, 2048) go with e8m0 scales uint8 [N, K / 32] = (64, 128) with K % 32 == 0, got (torch.uint8, (64, 127))'),  # 9c
    ('ValueError', 'MXFP4 weights are a uint8 [N, K / 2] tensor of packed e2m1 nibbles'),  # 9d
    ('ValueError', 'MXFP4 weights uint8 [N, K / 2] = (64, 2040) go with e8m0 scales uint8 [N, K / 32] = (64, 127) with K % 32 == 0, got (torch.uint8, (64, 128))'),  # 9e
    ('ValueError', 'x [..., K] with K = 4128 does not match MXFP4 weights uint8 [N, K / 2] = (64, 2048) and scales uint8 [N, K / 32]'),  # 9f
    ('ValueError', 'MXFP4 weights uint8 [N, K / 2] = (64, 2048) go with e8m0 scales uint8 [N, K / 32] = (64, 128) with K % 32 == 0, got (torch.float32, (64,))'),  # 9g
    ('ValueError', 'MXFP4 weights uint8 [N, K / 2] = (384, 2048) go with e8m0 scales uint8 [N, K / 32] = (384, 128) with K % 32 == 0, got None'),  # 9h
    ('ValueError', 'MXFP4 weights uint8 [N, K / 2] = (384, 2048) go with e8m0 scales uint8 [N, K / 32] = (384, 128) with K % 32 == 0, got (torch.float32, (384, 128))'),  # 9i
    ('ValueError', 'MXFP4 weights uint8 [N, K / 2] = (384, 2048) go with e8m0 scales uint8 [N, K / 32] = (384, 128) with K % 32 == 0, got (torch.uint8, (384, 127))'),  # 9j
    ('ValueError', 'MXFP4 weights uint8 [N, K / 2] = (384, 2040) go with e8m0 scales uint8 [N, K / 32] = (384, 127) with K % 32 == 0, got (torch.uint8, (384, 128))'),  # 9k
    ('ValueError', 'x [..., K] with K = 4128 does not match MXFP4 weights uint8 [N, K / 2] = (384, 2048) and scales uint8 [N, K / 32]'),  # 9l
    ('ValueError', 'MXFP4 weights uint8 [N, K / 2] = (384, 2048) go with e8m0 scales uint8 [N, K / 32] = (384, 128) with K % 32 == 0, got (torch.float32, (384,))'),  # 9m
]

TABLE = {
    'linear-bf16-plain':
        '000001010101010100000101010101010000010101010101000001010101010100000101010101010202030303030303020203030303030302020303 '
        '030303030202030303030303020203030303030304040505050505050404050505050505040405050505050504040505050505050404050505050505 '
        '06060606060606060606060606060606060606060606060606060606060606060606060606060606',
    'linear-bf16-bias':
        '070701010101070701010101070701010101070701010101070701010101080803030303080803030303080803030303080803030303080803030303 '
        '090905050505090905050505090905050505090905050505090905050505060606060606060606060606060606060606060606060606060606060606',
    'linear-bf16-silu':
        '0a0a0b0b0b0b0a0a0b0b0b0b0a0a0b0b0b0b0a0a0b0b0b0b0a0a0b0b0b0b0c0c0d0d0d0d0c0c0d0d0d0d0c0c0d0d0d0d0c0c0d0d0d0d0c0c0d0d0d0d '
        '0e0e0f0f0f0f0e0e0f0f0f0f0e0e0f0f0f0f0e0e0f0f0f0f0e0e0f0f0f0f0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g',
    'linear-bf16-out':
        '0h0h010101010h0h010101010h0h010101010h0h010101010h0h010101010i0i030303030i0i030303030i0i030303030i0i030303030i0i03030303 '
        '0j0j050505050j0j050505050j0j050505050j0j050505050j0j05050505060606060606060606060606060606060606060606060606060606060606',
    'linear-bf16-near_pull':
        '0k0k0l0l0l0l0k0k0l0l0l0l0k0k0l0l0l0l0k0k0l0l0l0l0k0k0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'linear-bf16-silu-bias':
        '0m0m0b0b0b0b0m0m0b0b0b0b0m0m0b0b0b0b0m0m0b0b0b0b0m0m0b0b0b0b0n0n0d0d0d0d0n0n0d0d0d0d0n0n0d0d0d0d0n0n0d0d0d0d0n0n0d0d0d0d '
        '0o0o0f0f0f0f0o0o0f0f0f0f0o0o0f0f0f0f0o0o0f0f0f0f0o0o0f0f0f0f0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g0g',
    'linear-bf16-silu-near_pull':
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'linear-bf16-bias-near_pull':
        '0p0p0l0l0l0l0p0p0l0l0l0l0p0p0l0l0l0l0p0p0l0l0l0l0p0p0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'linear-bf16-silu-bias-near_pull':
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'linear-fp8-plain':
        '0q0q0q0q0q0q0q0q0q0q0q0q0q0q0q0q0r0r0q0q0q0q0q0q0r0r0q0q0q0q0q0q0r0r0q0q0q0q0q0q0s0t0s0s0s0s0s0s0s0s0s0s0s0s0s0s0s0t0s0s '
        '0s0s0s0s0s0t0s0s0s0s0s0s0s0t0s0s0s0s0s0s0u0v0u0u0u0u0u0u0u0u0u0u0u0u0u0u0u0v0u0u0u0u0u0u0u0v0u0u0u0u0u0u0u0v0u0u0u0u0u0u '
        '0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w',
    'linear-fp8-bias':
        '0q0q0q0q0q0q0q0q0q0q0q0q0x0x0q0q0q0q0x0x0q0q0q0q0x0x0q0q0q0q0s0y0s0s0s0s0s0s0s0s0s0s0s0y0s0s0s0s0s0y0s0s0s0s0s0y0s0s0s0s '
        '0u0z0u0u0u0u0u0u0u0u0u0u0u0z0u0u0u0u0u0z0u0u0u0u0u0z0u0u0u0u0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w0w',
    'linear-fp8-silu':
        '101010101010101010101010111110101010111110101010111110101010121312121212121212121212121312121212121312121212121312121212 '
        '141514141414141414141414141514141414141514141414141514141414161616161616161616161616161616161616161616161616161616161616',
    'linear-fp8-out':
        '171717171717171717171717181817171717181817171717181817171717191a19191919191919191919191a19191919191a19191919191a19191919 '
        '1b1c1b1b1b1b1b1b1b1b1b1b1b1c1b1b1b1b1b1c1b1b1b1b1b1c1b1b1b1b1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d1d',
    'linear-fp8-near_pull':
        '0l0l0l0l0l0l0l0l0l0l0l0l1e1e0l0l0l0l1e1e0l0l0l0l1e1e0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'linear-fp8-silu-bias':
        '1010101010101010101010101f1f101010101f1f101010101f1f10101010121g12121212121212121212121g12121212121g12121212121g12121212 '
        '141h14141414141414141414141h14141414141h14141414141h14141414161616161616161616161616161616161616161616161616161616161616',
    'linear-fp8-silu-near_pull':
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'linear-fp8-bias-near_pull':
        '0l0l0l0l0l0l0l0l0l0l0l0l1i1i0l0l0l0l1i1i0l0l0l0l1i1i0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'linear-fp8-silu-bias-near_pull':
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'linear-mxfp4-plain':
        '1j1j1j1j1j1j1j1j1j1j1j1j1j1j1j1j1j1j1j1j1k1k1j1j1j1j1j1j1j1j1k1k1j1j1j1j1j1j1j1j1k1k1j1j1j1j1j1j1j1j1l1l1l1l1l1l1l1l1l1l '
        '1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m '
        '1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n '
        '1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n',
    'linear-mxfp4-bias':
        '1j1j1j1j1j1j1j1j1j1j1j1j1j1j1j1j1o1o1j1j1j1j1j1j1o1o1j1j1j1j1j1j1o1o1j1j1j1j1j1j1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l '
        '1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1l1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m1m '
        '1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n1n',
    'linear-mxfp4-silu':
        '1p1p1p1p1p1p1p1p1p1p1p1p1p1p1p1p1q1q1p1p1p1p1p1p1q1q1p1p1p1p1p1p1q1q1p1p1p1p1p1p1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r '
        '1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s '
        '1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t',
    'linear-mxfp4-out':
        '1u1u1u1u1u1u1u1u1u1u1u1u1u1u1u1u1v1v1u1u1u1u1u1u1v1v1u1u1u1u1u1u1v1v1u1u1u1u1u1u1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w '
        '1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w1w1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x1x '
        '1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y1y',
    'linear-mxfp4-near_pull':
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l1z1z0l0l0l0l0l0l1z1z0l0l0l0l0l0l1z1z0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'linear-mxfp4-silu-bias':
        '1p1p1p1p1p1p1p1p1p1p1p1p1p1p1p1p20201p1p1p1p1p1p20201p1p1p1p1p1p20201p1p1p1p1p1p1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r '
        '1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1r1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s1s '
        '1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t1t',
    'linear-mxfp4-silu-near_pull':
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'linear-mxfp4-bias-near_pull':
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l21210l0l0l0l0l0l21210l0l0l0l0l0l21210l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'linear-mxfp4-silu-bias-near_pull':
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l '
        '0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l0l',
    'norm-bf16-plain':
        '222222222323232322222222232323232222222223232323242422222323232322222222232323232525252526262626252525252626262625252525 '
        '262626262525252526262626252525252626262627272727282828282727272728282828272727272828282827272727282828282727272728282828 '
        '29292929292929292929292929292929292929292929292929292929292929292929292929292929',
    'norm-bf16-bias':
        '2a2a2a2a23232a2a2a2a23232a2a2a2a23232b2b2a2a23232a2a2a2a23232c2c2c2c26262c2c2c2c26262c2c2c2c26262c2c2c2c26262c2c2c2c2626 '
        '2d2d2d2d28282d2d2d2d28282d2d2d2d28282d2d2d2d28282d2d2d2d2828292929292929292929292929292929292929292929292929292929292929',
    'norm-bf16-silu':
        '2e2e2e2e2f2f2e2e2e2e2f2f2e2e2e2e2f2f2g2g2e2e2f2f2e2e2e2e2f2f2h2h2h2h2i2i2h2h2h2h2i2i2h2h2h2h2i2i2h2h2h2h2i2i2h2h2h2h2i2i '
        '2j2j2j2j2k2k2j2j2j2j2k2k2j2j2j2j2k2k2j2j2j2j2k2k2j2j2j2j2k2k2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l',
    'norm-bf16-out':
        '2m2m2m2m23232m2m2m2m23232m2m2m2m23232n2n2m2m23232m2m2m2m23232o2o2o2o26262o2o2o2o26262o2o2o2o26262o2o2o2o26262o2o2o2o2626 '
        '2p2p2p2p28282p2p2p2p28282p2p2p2p28282p2p2p2p28282p2p2p2p2828292929292929292929292929292929292929292929292929292929292929',
    'norm-bf16-h_out':
        '222222222323222222222323222222222323242422222323222222222323252525252626252525252626252525252626252525252626252525252626 '
        '272727272828272727272828272727272828272727272828272727272828292929292929292929292929292929292929292929292929292929292929',
    'norm-bf16-residual':
        '2q2q2q2q2r2r2q2q2q2q2r2r2q2q2q2q2r2r2s2s2q2q2r2r2q2q2q2q2r2r2t2t2t2t2u2u2t2t2t2t2u2u2t2t2t2t2u2u2t2t2t2t2u2u2t2t2t2t2u2u '
        '2v2v2v2v2w2w2v2v2v2v2w2w2v2v2v2v2w2w2v2v2v2v2w2w2v2v2v2v2w2w2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x',
    'norm-bf16-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2z2z2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-bf16-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-bf16-silu-bias':
        '313131312f2f313131312f2f313131312f2f323231312f2f313131312f2f333333332i2i333333332i2i333333332i2i333333332i2i333333332i2i '
        '343434342k2k343434342k2k343434342k2k343434342k2k343434342k2k2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l2l',
    'norm-bf16-silu-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-bf16-silu-near_pull':
        '303030303030303030303030303030303030353530303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-bf16-bias-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y36362y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-bf16-bias-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-bf16-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-bf16-silu-bias-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-bf16-silu-bias-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-bf16-silu-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-bf16-bias-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-bf16-silu-bias-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-bf16-out-h_out-residual':
        '373737372r2r373737372r2r373737372r2r383837372r2r373737372r2r393939392u2u393939392u2u393939392u2u393939392u2u393939392u2u '
        '3a3a3a3a2w2w3a3a3a3a2w2w3a3a3a3a2w2w3a3a3a3a2w2w3a3a3a3a2w2w2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x2x',
    'norm-fp8-plain':
        '3b3b3b3b3b3b3b3b3b3b3b3b3b3b3b3b3c3c3c3c3b3b3b3b3d3d3c3c3b3b3b3b3c3c3c3c3b3b3b3b3e3f3e3f3e3e3e3e3e3e3e3e3e3e3e3e3e3f3e3f '
        '3e3e3e3e3e3f3e3f3e3e3e3e3e3f3e3f3e3e3e3e3g3h3g3h3g3g3g3g3g3g3g3g3g3g3g3g3g3h3g3h3g3g3g3g3g3h3g3h3g3g3g3g3g3h3g3h3g3g3g3g '
        '3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i',
    'norm-fp8-bias':
        '3b3b3b3b3b3b3b3b3b3b3b3b3j3j3j3j3b3b3k3k3j3j3b3b3j3j3j3j3b3b3e3l3e3l3e3e3e3e3e3e3e3e3e3l3e3l3e3e3e3l3e3l3e3e3e3l3e3l3e3e '
        '3g3m3g3m3g3g3g3g3g3g3g3g3g3m3g3m3g3g3g3m3g3m3g3g3g3m3g3m3g3g3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i',
    'norm-fp8-silu':
        '3n3n3n3n3n3n3n3n3n3n3n3n3o3o3o3o3n3n3p3p3o3o3n3n3o3o3o3o3n3n3q3r3q3r3q3q3q3q3q3q3q3q3q3r3q3r3q3q3q3r3q3r3q3q3q3r3q3r3q3q '
        '3s3t3s3t3s3s3s3s3s3s3s3s3s3t3s3t3s3s3s3t3s3t3s3s3s3t3s3t3s3s3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u',
    'norm-fp8-out':
        '3v3v3v3v3v3v3v3v3v3v3v3v3w3w3w3w3v3v3x3x3w3w3v3v3w3w3w3w3v3v3y3z3y3z3y3y3y3y3y3y3y3y3y3z3y3z3y3y3y3z3y3z3y3y3y3z3y3z3y3y '
        '404140414040404040404040404140414040404140414040404140414040424242424242424242424242424242424242424242424242424242424242',
    'norm-fp8-h_out':
        '3b3b3b3b3b3b3b3b3b3b3b3b3c3c3c3c3b3b3d3d3c3c3b3b3c3c3c3c3b3b3e3f3e3f3e3e3e3e3e3e3e3e3e3f3e3f3e3e3e3f3e3f3e3e3e3f3e3f3e3e '
        '3g3h3g3h3g3g3g3g3g3g3g3g3g3h3g3h3g3g3g3h3g3h3g3g3g3h3g3h3g3g3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i3i',
    'norm-fp8-residual':
        '434343434343434343434343444444444343454544444343444444444343464746474646464646464646464746474646464746474646464746474646 '
        '4849484948484848484848484849484948484849484948484849484948484a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a4a',
    'norm-fp8-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y4b4b2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-fp8-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-fp8-silu-bias':
        '3n3n3n3n3n3n3n3n3n3n3n3n4c4c4c4c3n3n4d4d4c4c3n3n4c4c4c4c3n3n3q4e3q4e3q3q3q3q3q3q3q3q3q4e3q4e3q3q3q4e3q4e3q3q3q4e3q4e3q3q '
        '3s4f3s4f3s3s3s3s3s3s3s3s3s4f3s4f3s3s3s4f3s4f3s3s3s4f3s4f3s3s3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u3u',
    'norm-fp8-silu-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-fp8-silu-near_pull':
        '3030303030303030303030303030303030304g4g30303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-fp8-bias-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y4h4h2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-fp8-bias-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-fp8-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-fp8-silu-bias-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-fp8-silu-bias-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-fp8-silu-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-fp8-bias-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-fp8-silu-bias-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-fp8-out-h_out-residual':
        '4i4i4i4i4i4i4i4i4i4i4i4i4j4j4j4j4i4i4k4k4j4j4i4i4j4j4j4j4i4i4l4m4l4m4l4l4l4l4l4l4l4l4l4m4l4m4l4l4l4m4l4m4l4l4l4m4l4m4l4l '
        '4n4o4n4o4n4n4n4n4n4n4n4n4n4o4n4o4n4n4n4o4n4o4n4n4n4o4n4o4n4n4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p4p',
    'norm-mxfp4-plain':
        '4q4q4q4q4q4q4q4q4q4q4q4q4q4q4q4q4q4q4q4q4r4r4r4r4q4q4q4q4q4q4s4s4r4r4q4q4q4q4q4q4r4r4r4r4q4q4q4q4q4q4t4t4t4t4t4t4t4t4t4t '
        '4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u '
        '4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v '
        '4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v',
    'norm-mxfp4-bias':
        '4q4q4q4q4q4q4q4q4q4q4q4q4q4q4q4q4w4w4w4w4q4q4q4q4x4x4w4w4q4q4q4q4w4w4w4w4q4q4q4q4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t '
        '4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u '
        '4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v',
    'norm-mxfp4-silu':
        '4y4y4y4y4y4y4y4y4y4y4y4y4y4y4y4y4z4z4z4z4y4y4y4y50504z4z4y4y4y4y4z4z4z4z4y4y4y4y5151515151515151515151515151515151515151 '
        '515151515151515151515151515151515151515152525252525252525252525252525252525252525252525252525252525252525252525252525252 '
        '53535353535353535353535353535353535353535353535353535353535353535353535353535353',
    'norm-mxfp4-out':
        '545454545454545454545454545454545555555554545454565655555454545455555555545454545757575757575757575757575757575757575757 '
        '575757575757575757575757575757575757575758585858585858585858585858585858585858585858585858585858585858585858585858585858 '
        '59595959595959595959595959595959595959595959595959595959595959595959595959595959',
    'norm-mxfp4-h_out':
        '4q4q4q4q4q4q4q4q4q4q4q4q4q4q4q4q4r4r4r4r4q4q4q4q4s4s4r4r4q4q4q4q4r4r4r4r4q4q4q4q4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t '
        '4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4t4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u4u '
        '4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v4v',
    'norm-mxfp4-residual':
        '5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5a5b5b5b5b5a5a5a5a5c5c5b5b5a5a5a5a5b5b5b5b5a5a5a5a5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d '
        '5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d5d5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e5e '
        '5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f5f',
    'norm-mxfp4-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y5g5g2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-mxfp4-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '30303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-mxfp4-silu-bias':
        '4y4y4y4y4y4y4y4y4y4y4y4y4y4y4y4y5h5h5h5h4y4y4y4y5i5i5h5h4y4y4y4y5h5h5h5h4y4y4y4y5151515151515151515151515151515151515151 '
        '515151515151515151515151515151515151515152525252525252525252525252525252525252525252525252525252525252525252525252525252 '
        '53535353535353535353535353535353535353535353535353535353535353535353535353535353',
    'norm-mxfp4-silu-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-mxfp4-silu-near_pull':
        '3030303030303030303030303030303030303030303030305j5j30303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '30303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-mxfp4-bias-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y5k5k2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-mxfp4-bias-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '30303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-mxfp4-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '30303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-mxfp4-silu-bias-range_max':
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y '
        '2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y2y',
    'norm-mxfp4-silu-bias-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '30303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-mxfp4-silu-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '30303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-mxfp4-bias-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '30303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-mxfp4-silu-bias-range_max-near_pull':
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030303030 '
        '30303030303030303030303030303030303030303030303030303030303030303030303030303030',
    'norm-mxfp4-out-h_out-residual':
        '5l5l5l5l5l5l5l5l5l5l5l5l5l5l5l5l5m5m5m5m5l5l5l5l5n5n5m5m5l5l5l5l5m5m5m5m5l5l5l5l5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o '
        '5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o5o5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p5p '
        '5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q5q',
    'qkv-bf16-plain':
        '5r5r5r5r5s5s5s5s5r5r5r5r5s5s5s5s5r5r5r5r5s5s5s5s5t5t5r5r5s5s5s5s5r5r5r5r5s5s5s5s5u5u5u5u5v5v5v5v5u5u5u5u5v5v5v5v5u5u5u5u '
        '5v5v5v5v5u5u5u5u5v5v5v5v5u5u5u5u5v5v5v5v5w5w5w5w5x5x5x5x5w5w5w5w5x5x5x5x5w5w5w5w5x5x5x5x5w5w5w5w5x5x5x5x5w5w5w5w5x5x5x5x '
        '5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y',
    'qkv-bf16-bias':
        '5z5z5z5z5s5s5z5z5z5z5s5s5z5z5z5z5s5s60605z5z5s5s5z5z5z5z5s5s616161615v5v616161615v5v616161615v5v616161615v5v616161615v5v '
        '626262625x5x626262625x5x626262625x5x626262625x5x626262625x5x5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y5y',
    'qkv-bf16-residual':
        '636363636464636363636464636363636464656563636464636363636464666666666767666666666767666666666767666666666767666666666767 '
        '6868686869696868686869696868686869696868686869696868686869696a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a6a',
    'qkv-bf16-q_override':
        '6b6b6b6b6c6c6b6b6b6b6c6c6b6b6b6b6c6c6d6d6b6b6c6c6b6b6b6b6c6c6e6e6e6e6f6f6e6e6e6e6f6f6e6e6e6e6f6f6e6e6e6e6f6f6e6e6e6e6f6f '
        '6g6g6g6g6h6h6g6g6g6g6h6h6g6g6g6g6h6h6g6g6g6g6h6h6g6g6g6g6h6h6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i6i',
    'qkv-bf16-d64':
        '6j6j6j6j6k6k6j6j6j6j6k6k6j6j6j6j6k6k6l6l6j6j6k6k6j6j6j6j6k6k6m6m6m6m6n6n6m6m6m6m6n6n6m6m6m6m6n6n6m6m6m6m6n6n6m6m6m6m6n6n '
        '6o6o6o6o6p6p6o6o6o6o6p6p6o6o6o6o6p6p6o6o6o6o6p6p6o6o6o6o6p6p6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q6q',
    'qkv-bf16-bias-residual-q_override':
        '6r6r6r6r6s6s6r6r6r6r6s6s6r6r6r6r6s6s6t6t6r6r6s6s6r6r6r6r6s6s6u6u6u6u6v6v6u6u6u6u6v6v6u6u6u6u6v6v6u6u6u6u6v6v6u6u6u6u6v6v '
        '6w6w6w6w6x6x6w6w6w6w6x6x6w6w6w6w6x6x6w6w6w6w6x6x6w6w6w6w6x6x6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y6y',
    'qkv-fp8-plain':
        '6z6z6z6z6z6z6z6z6z6z6z6z6z6z6z6z707070706z6z6z6z717170706z6z6z6z707070706z6z6z6z7273727372727272727272727272727272737273 '
        '727272727273727372727272727372737272727274757475747474747474747474747474747574757474747474757475747474747475747574747474 '
        '76767676767676767676767676767676767676767676767676767676767676767676767676767676',
    'qkv-fp8-bias':
        '6z6z6z6z6z6z6z6z6z6z6z6z777777776z6z787877776z6z777777776z6z727972797272727272727272727972797272727972797272727972797272 '
        '747a747a7474747474747474747a747a7474747a747a7474747a747a7474767676767676767676767676767676767676767676767676767676767676',
    'qkv-fp8-residual':
        '7b7b7b7b7b7b7b7b7b7b7b7b7c7c7c7c7b7b7d7d7c7c7b7b7c7c7c7c7b7b7e7f7e7f7e7e7e7e7e7e7e7e7e7f7e7f7e7e7e7f7e7f7e7e7e7f7e7f7e7e '
        '7g7h7g7h7g7g7g7g7g7g7g7g7g7h7g7h7g7g7g7h7g7h7g7g7g7h7g7h7g7g7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i7i',
    'qkv-fp8-q_override':
        '7j7j7j7j7j7j7j7j7j7j7j7j7k7k7k7k7j7j7l7l7k7k7j7j7k7k7k7k7j7j7m7n7m7n7m7m7m7m7m7m7m7m7m7n7m7n7m7m7m7n7m7n7m7m7m7n7m7n7m7m '
        '7o7p7o7p7o7o7o7o7o7o7o7o7o7p7o7p7o7o7o7p7o7p7o7o7o7p7o7p7o7o7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q7q',
    'qkv-fp8-d64':
        '7r7r7r7r7r7r7r7r7r7r7r7r7s7s7s7s7r7r7t7t7s7s7r7r7s7s7s7s7r7r7u7v7u7v7u7u7u7u7u7u7u7u7u7v7u7v7u7u7u7v7u7v7u7u7u7v7u7v7u7u '
        '7w7x7w7x7w7w7w7w7w7w7w7w7w7x7w7x7w7w7w7x7w7x7w7w7w7x7w7x7w7w7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y7y',
    'qkv-fp8-bias-residual-q_override':
        '7z7z7z7z7z7z7z7z7z7z7z7z808080807z7z818180807z7z808080807z7z828382838282828282828282828382838282828382838282828382838282 '
        '848584858484848484848484848584858484848584858484848584858484868686868686868686868686868686868686868686868686868686868686',
    'qkv-mxfp4-plain':
        '87878787878787878787878787878787878787878888888887878787878789898888878787878787888888888787878787878a8a8a8a8a8a8a8a8a8a '
        '8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b '
        '8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c '
        '8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c',
    'qkv-mxfp4-bias':
        '878787878787878787878787878787878d8d8d8d878787878e8e8d8d878787878d8d8d8d878787878a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a '
        '8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8a8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b8b '
        '8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c8c',
    'qkv-mxfp4-residual':
        '8f8f8f8f8f8f8f8f8f8f8f8f8f8f8f8f8g8g8g8g8f8f8f8f8h8h8g8g8f8f8f8f8g8g8g8g8f8f8f8f8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i '
        '8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i8i8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j8j '
        '8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k8k',
    'qkv-mxfp4-q_override':
        '8l8l8l8l8l8l8l8l8l8l8l8l8l8l8l8l8m8m8m8m8l8l8l8l8n8n8m8m8l8l8l8l8m8m8m8m8l8l8l8l8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o '
        '8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o8o8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p8p '
        '8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q8q',
    'qkv-mxfp4-d64':
        '8r8r8r8r8r8r8r8r8r8r8r8r8r8r8r8r8s8s8s8s8r8r8r8r8t8t8s8s8r8r8r8r8s8s8s8s8r8r8r8r8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u '
        '8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u8u8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v8v '
        '8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w8w',
    'qkv-mxfp4-bias-residual-q_override':
        '8x8x8x8x8x8x8x8x8x8x8x8x8x8x8x8x8y8y8y8y8x8x8x8x8z8z8y8y8x8x8x8x8y8y8y8y8x8x8x8x9090909090909090909090909090909090909090 '
        '909090909090909090909090909090909090909091919191919191919191919191919191919191919191919191919191919191919191919191919191 '
        '92929292929292929292929292929292929292929292929292929292929292929292929292929292',
}

SPECIAL = [
    ('op=linear fmt=bf16 rows=1 K=4096 xc=True wc=c mode=nf opts=()', 0),
    ('op=linear fmt=bf16 rows=2 K=4096 xc=True wc=c mode=nf opts=()', 2),
    ('op=linear fmt=bf16 rows=1 K=4096 xc=True wc=c mode=fn opts=()', 0),
    ('op=linear fmt=bf16 rows=2 K=4096 xc=True wc=c mode=fn opts=()', 2),
    ('op=linear fmt=bf16 rows=1 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=linear fmt=bf16 rows=2 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=linear fmt=bf16 rows=1 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=linear fmt=bf16 rows=2 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=linear fmt=bf16 rows=1 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=linear fmt=bf16 rows=2 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=linear fmt=bf16 rows=1 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=linear fmt=bf16 rows=2 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=linear fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nf opts=()', 27),
    ('op=linear fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nf opts=()', 29),
    ('op=linear fmt=fp8 rows=1 K=4096 xc=True wc=c mode=fn opts=()', 27),
    ('op=linear fmt=fp8 rows=2 K=4096 xc=True wc=c mode=fn opts=()', 28),
    ('op=linear fmt=fp8 rows=1 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=linear fmt=fp8 rows=2 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=linear fmt=fp8 rows=1 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=linear fmt=fp8 rows=2 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=linear fmt=fp8 rows=1 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=linear fmt=fp8 rows=2 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=linear fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=linear fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nf opts=()', 56),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nf opts=()', 57),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=fn opts=()', 56),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=fn opts=()', 57),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=norm fmt=bf16 rows=1 K=4096 xc=True wc=c mode=nf opts=()', 76),
    ('op=norm fmt=bf16 rows=2 K=4096 xc=True wc=c mode=nf opts=()', 77),
    ('op=norm fmt=bf16 rows=1 K=4096 xc=True wc=c mode=fn opts=()', 76),
    ('op=norm fmt=bf16 rows=2 K=4096 xc=True wc=c mode=fn opts=()', 77),
    ('op=norm fmt=bf16 rows=1 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=norm fmt=bf16 rows=2 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=norm fmt=bf16 rows=1 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=norm fmt=bf16 rows=2 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=norm fmt=bf16 rows=1 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=norm fmt=bf16 rows=2 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=norm fmt=bf16 rows=1 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=norm fmt=bf16 rows=2 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=norm fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nf opts=()', 121),
    ('op=norm fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nf opts=()', 123),
    ('op=norm fmt=fp8 rows=1 K=4096 xc=True wc=c mode=fn opts=()', 121),
    ('op=norm fmt=fp8 rows=2 K=4096 xc=True wc=c mode=fn opts=()', 122),
    ('op=norm fmt=fp8 rows=1 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=norm fmt=fp8 rows=2 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=norm fmt=fp8 rows=1 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=norm fmt=fp8 rows=2 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=norm fmt=fp8 rows=1 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=norm fmt=fp8 rows=2 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=norm fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=norm fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nf opts=()', 172),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nf opts=()', 173),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=fn opts=()', 172),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=fn opts=()', 173),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=qkv fmt=bf16 rows=1 K=4096 xc=True wc=c mode=nf opts=()', 209),
    ('op=qkv fmt=bf16 rows=2 K=4096 xc=True wc=c mode=nf opts=()', 210),
    ('op=qkv fmt=bf16 rows=1 K=4096 xc=True wc=c mode=fn opts=()', 209),
    ('op=qkv fmt=bf16 rows=2 K=4096 xc=True wc=c mode=fn opts=()', 210),
    ('op=qkv fmt=bf16 rows=1 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=qkv fmt=bf16 rows=2 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=qkv fmt=bf16 rows=1 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=qkv fmt=bf16 rows=2 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=qkv fmt=bf16 rows=1 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=qkv fmt=bf16 rows=2 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=qkv fmt=bf16 rows=1 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=qkv fmt=bf16 rows=2 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=qkv fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nf opts=()', 253),
    ('op=qkv fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nf opts=()', 255),
    ('op=qkv fmt=fp8 rows=1 K=4096 xc=True wc=c mode=fn opts=()', 253),
    ('op=qkv fmt=fp8 rows=2 K=4096 xc=True wc=c mode=fn opts=()', 254),
    ('op=qkv fmt=fp8 rows=1 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=qkv fmt=fp8 rows=2 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=qkv fmt=fp8 rows=1 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=qkv fmt=fp8 rows=2 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=qkv fmt=fp8 rows=1 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=qkv fmt=fp8 rows=2 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=qkv fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=qkv fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nf opts=()', 297),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nf opts=()', 298),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=fn opts=()', 297),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=fn opts=()', 298),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=xf opts=()', 327),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=fx opts=()', 328),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=xx opts=()', 327),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nx opts=()', 328),
    ("op=linear fmt=bf16 rows=1 K=1024 xc=True wc=c mode=ff opts=('near_pull',) N=8192", 329),
    ("op=linear fmt=bf16 rows=1 K=1024 xc=True wc=c mode=ff opts=('near_pull',) N=8208", 21),
    ("op=linear fmt=fp8 rows=1 K=1024 xc=True wc=c mode=ff opts=('near_pull',) N=8192", 330),
    ("op=linear fmt=fp8 rows=1 K=1024 xc=True wc=c mode=ff opts=('near_pull',) N=8208", 21),
    ("op=linear fmt=mxfp4 rows=1 K=1024 xc=True wc=c mode=ff opts=('near_pull',) N=8192", 331),
    ("op=linear fmt=mxfp4 rows=1 K=1024 xc=True wc=c mode=ff opts=('near_pull',) N=8208", 21),
    ('op=linear fmt=bf16 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=bf16_w_f32_scale', 332),
    ('op=linear fmt=bf16 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=bf16_w_f32_scale', 332),
    ('op=linear fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_no_scale', 0),
    ('op=linear fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_no_scale', 2),
    ('op=linear fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_f16', 333),
    ('op=linear fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_f16', 333),
    ('op=linear fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_short', 333),
    ('op=linear fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_short', 333),
    ('op=linear fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_strided', 333),
    ('op=linear fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_strided', 333),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_no_scale', 334),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_no_scale', 334),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_f32', 335),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_f32', 335),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_short', 336),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_short', 336),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_w_1d', 337),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_w_1d', 337),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_k_off_block', 338),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_k_off_block', 338),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_x_k_mismatch', 339),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_x_k_mismatch', 339),
    ('op=linear fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_f32_row_scale', 340),
    ('op=linear fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_f32_row_scale', 340),
    ('op=norm fmt=bf16 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=bf16_w_f32_scale', 332),
    ('op=norm fmt=bf16 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=bf16_w_f32_scale', 332),
    ('op=norm fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_no_scale', 76),
    ('op=norm fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_no_scale', 77),
    ('op=norm fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_f16', 333),
    ('op=norm fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_f16', 333),
    ('op=norm fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_short', 333),
    ('op=norm fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_short', 333),
    ('op=norm fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_strided', 333),
    ('op=norm fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_strided', 333),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_no_scale', 334),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_no_scale', 334),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_f32', 335),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_f32', 335),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_short', 336),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_short', 336),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_w_1d', 337),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_w_1d', 337),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_k_off_block', 338),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_k_off_block', 338),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_x_k_mismatch', 339),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_x_k_mismatch', 339),
    ('op=norm fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_f32_row_scale', 340),
    ('op=norm fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_f32_row_scale', 340),
    ('op=qkv fmt=bf16 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=bf16_w_f32_scale', 332),
    ('op=qkv fmt=bf16 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=bf16_w_f32_scale', 332),
    ('op=qkv fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_no_scale', 209),
    ('op=qkv fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_no_scale', 210),
    ('op=qkv fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_f16', 333),
    ('op=qkv fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_f16', 333),
    ('op=qkv fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_short', 333),
    ('op=qkv fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_short', 333),
    ('op=qkv fmt=fp8 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_strided', 333),
    ('op=qkv fmt=fp8 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=fp8_scale_strided', 333),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_no_scale', 341),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_no_scale', 341),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_f32', 342),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_f32', 342),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_short', 343),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_scale_short', 343),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_w_1d', 337),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_w_1d', 337),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_k_off_block', 344),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_k_off_block', 344),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_x_k_mismatch', 345),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_x_k_mismatch', 345),
    ('op=qkv fmt=mxfp4 rows=1 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_f32_row_scale', 346),
    ('op=qkv fmt=mxfp4 rows=2 K=4096 xc=True wc=c mode=nn opts=() pair=mxfp4_f32_row_scale', 346),
]
