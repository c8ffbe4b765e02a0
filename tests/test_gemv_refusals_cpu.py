"""CPU: the refusal table of the decode GEMV entries, bf16, FP8 and MXFP4 - the return code of every extern "C" entry of
skv_gemv.hip, skv_gemv_fp8.hip and skv_gemv_mxfp4.hip for a null pointer in each pointer argument, each shape refusal and each
order of checks, as recorded from the files while each still had entry bodies of its own (MXFP4 shares FP8's order of checks).
One set of entry bodies, one dispatcher (skv_gemv_frame.h) and one near_pull_of (skv_launch.h) serve all formats now: this table
holds them to every format's answers.  Every argument set here returns before any HIP call (no GPU is present: a call that
reached the runtime could not return these codes)."""
import pytest

ARG, UNSUPPORTED = -1, -2
P = 0x1000            # a non-null pointer that is never dereferenced on the host

# arguments of every entry by name, in the order of the bf16 signature; FP8 / MXFP4: `scale` follows W.  Defaults: a valid launch.
BASE = dict(W=P, scale=P, x=P, residual=0, norm_weight=P, eps=1e-5, h_out=0, bias=0, y=P, N=512, K=4096, silu=0, range_max=P,
            early_state=P, blocks=8, groups=4, n_landmarks=1000, n_chunks=2000, early_max=64, v_host=P, stride=8 * 2000 * 1024,
            pull_parts=1, active_lists=1, list=0, cos_sin=P, pos=P, row_idx=P, q_override=0, q_out=P, k_cache=P, v_cache=P,
            q_heads=2, kv_heads=1, head_dim=128, cs_stride=128, cs_rows=64, cache_stride_h=8 * 128, cache_rows=8, rope_mode=1,
            stream=0)
NEAR = "early_state blocks groups n_landmarks n_chunks early_max v_host stride pull_parts"
SIGS = {
    "gemv": ("skv_gemv_{}", "W x bias y N K silu stream"),
    "norm": ("skv_norm_gemv_{}", "W x residual norm_weight eps h_out bias y N K silu stream"),
    "rangemax": ("skv_norm_gemv_rangemax_{}", "W x residual norm_weight eps h_out bias y N K range_max stream"),
    "near_gate_up": ("skv_norm_gemv_near_pull_{}", f"W x residual norm_weight eps h_out y N K {NEAR} active_lists stream"),
    "near_down": ("skv_gemv_near_pull_{}", f"W x bias y N K {NEAR} list stream"),
    "qkv": ("skv_qkv_gemv_rope_update{}", "W x residual norm_weight eps h_out bias cos_sin pos row_idx q_override q_out k_cache v_cache "
            "K q_heads kv_heads head_dim cs_stride cs_rows cache_stride_h cache_rows rope_mode stream"),
    "q_only": ("skv_q_gemv_rope", "W x residual norm_weight eps h_out bias cos_sin pos q_override q_out K q_heads kv_heads head_dim "
               "cs_stride cs_rows rope_mode stream"),                   # bf16 only: FP8 has no q-only launch
}
FORMATS = ("bf16", "fp8", "mxfp4")
ENTRIES = [(f, e) for f in FORMATS for e in SIGS if not (f != "bf16" and e == "q_only")]
NORM = ("norm", "rangemax", "near_gate_up", "qkv", "q_only")
NEARS = ("near_gate_up", "near_down")
BAD_K = {"bf16": (516, 504, 0), "fp8": (4104, 512, 1016),             # K % step != 0, K below one k-step
         "mxfp4": (4104, 4112, 512, 992, 1016, 0)}


def call(fmt, entry, **over):
    from shadowkv_amd import _lib
    name, sig = SIGS[entry]
    name = name.format({"bf16": "", "fp8": "_fp8", "mxfp4": "_mxfp4"}[fmt] if entry == "qkv" else fmt)
    names = sig.split()
    if fmt != "bf16":
        names.insert(1, "scale")
    assert set(over) <= set(names), (entry, set(over) - set(names))
    a = dict(BASE, **over)
    return getattr(_lib.lib(), name)(*[a[n] for n in names])


@pytest.mark.parametrize("fmt,entry", ENTRIES)
def test_null_pointers_and_sizes(fmt, entry):
    ptrs = ["W", "x"] + (["scale"] if fmt != "bf16" else []) + (["y"] if entry not in ("qkv", "q_only") else [])
    for p in ptrs:
        assert call(fmt, entry, **{p: 0}) == ARG, p
        assert call(fmt, entry, **{p: 0}, K=BAD_K[fmt][0]) == (UNSUPPORTED if entry == "q_only" else ARG), p   # pointers before K
    if entry in ("qkv", "q_only"):
        assert call(fmt, entry, q_heads=0, kv_heads=0) == ARG                                   # N = 0
    else:
        assert call(fmt, entry, N=0) == ARG and call(fmt, entry, N=-16) == ARG
    for K in BAD_K[fmt]:
        assert call(fmt, entry, K=K) == UNSUPPORTED, K
    if entry in NORM:
        assert call(fmt, entry, K=2048) == UNSUPPORTED and call(fmt, entry, K=8192) == UNSUPPORTED      # the norm prologue: K == 4096
    if entry in ("norm", "rangemax", "near_gate_up"):
        assert call(fmt, entry, norm_weight=0) == UNSUPPORTED
        assert call(fmt, entry, norm_weight=0, W=0) == ARG


@pytest.mark.parametrize("fmt", FORMATS)
def test_silu_and_range_max_refusals(fmt):
    for entry in ("gemv", "norm"):
        assert call(fmt, entry, silu=1, N=513) == ARG                       # an odd number of [gate; up] rows
        assert call(fmt, entry, silu=1, bias=P) == ARG                      # a SiLU launch has no bias slot
    assert call(fmt, "rangemax", range_max=0) == ARG
    assert call(fmt, "rangemax", range_max=0, K=BAD_K[fmt][0]) == ARG       # the keys buffer is checked first
    assert call(fmt, "rangemax", N=4104) == UNSUPPORTED                     # N % 16 != 0
    assert call(fmt, "rangemax", N=4104, W=0) == ARG


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("entry", NEARS)
def test_near_pull_refusals(fmt, entry):
    for bad in (dict(pull_parts=3), dict(pull_parts=8), dict(pull_parts=0), dict(early_state=0), dict(v_host=0), dict(blocks=0),
                dict(groups=0), dict(n_landmarks=0), dict(n_chunks=0), dict(early_max=0), dict(early_max=129), dict(stride=4)):
        assert call(fmt, entry, **bad) == ARG, bad
    lists = (dict(list=-1), dict(list=2)) if entry == "near_down" else (dict(active_lists=0), dict(active_lists=3))
    for bad in lists:
        assert call(fmt, entry, **bad) == ARG, bad
    assert call(fmt, entry, n_chunks=(1 << 18) + 1) == UNSUPPORTED          # the early state's limit
    assert call(fmt, entry, n_chunks=(1 << 18) + 1, pull_parts=3) == ARG    # the parts are checked before it
    # order of the two groups of checks: bf16 checks the role's arguments first, FP8 and MXFP4 the GEMV's own
    first = (ARG, UNSUPPORTED) if fmt == "bf16" else (UNSUPPORTED, ARG)
    assert call(fmt, entry, pull_parts=3, K=BAD_K[fmt][0]) == first[0]
    assert call(fmt, entry, n_chunks=(1 << 18) + 1, W=0) == first[1]
    # shapes the role does not ride in
    if entry == "near_down":
        assert call(fmt, entry, N=8208) == UNSUPPORTED                      # more than 8,192 rows
        assert call(fmt, entry, N=8208, early_state=0) == ARG
    else:
        assert call(fmt, entry, N=513) == UNSUPPORTED                       # an odd number of [gate; up] rows


@pytest.mark.parametrize("fmt,entry", [e for e in ENTRIES if e[1] in ("qkv", "q_only")])
def test_qkv_refusals(fmt, entry):
    ptrs = ["cos_sin", "pos", "q_out"] + (["row_idx", "k_cache", "v_cache"] if entry == "qkv" else ["norm_weight"])
    for p in ptrs:
        assert call(fmt, entry, **{p: 0}) == ARG, p
        assert call(fmt, entry, **{p: 0}, head_dim=64) == ARG, p            # pointers before the shape
    assert call(fmt, entry, cs_rows=0) == ARG
    assert call(fmt, entry, head_dim=64) == UNSUPPORTED
    for mode in (0, 3):
        assert call(fmt, entry, rope_mode=mode) == UNSUPPORTED
    assert call(fmt, entry, head_dim=64, W=0) == UNSUPPORTED                # the entry's own checks before the GEMV's
    if entry == "q_only":
        for bad in (dict(q_heads=0), dict(kv_heads=0)):
            assert call(fmt, entry, **bad) == ARG, bad
    else:
        # no query head: the FP8 / MXFP4 entry refuses it itself, the bf16 entry has no such check - its first refusal is the GEMV's K
        assert call(fmt, entry, q_heads=0, K=BAD_K[fmt][0]) == (UNSUPPORTED if fmt == "bf16" else ARG)
        if fmt != "bf16":
            assert call(fmt, entry, q_heads=0) == ARG and call(fmt, entry, kv_heads=0) == ARG
