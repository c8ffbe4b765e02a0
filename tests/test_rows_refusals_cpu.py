"""CPU: the refusal table of the two small-M projection entries, skv_linear_rows_bf16 (skv_rows_gemm.hip) and skv_linear_rows_fp8
(skv_rows_gemm_fp8.hip) - the return code for a null pointer in each pointer argument, each shape refusal and the order of the
checks, as recorded from the two files while each still had a branch tree of its own.  One dispatcher (skv_rows_frame.h) serves
both formats now and each format checks its own arguments in front of it: this table holds them to both formats' answers.  Every
argument set here returns before any HIP call (no GPU is present: a call that reached the runtime could not return these codes)."""
import pytest

ARG, UNSUPPORTED = -1, -2
P = 0x1000            # a non-null pointer that is never dereferenced on the host
BASE = dict(W=P, scale=P, X=P, bias=0, Y=P, M=8, N=512, K=4096, silu=0, stream=0)
STEP = {"bf16": 32, "fp8": 64}                                         # elements of one k-step
FORMATS = ("bf16", "fp8")


def call(fmt, **over):
    from shadowkv_amd import _lib
    names = "W X bias Y M N K silu stream".split()
    if fmt == "fp8":
        names.insert(1, "scale")
    assert set(over) <= set(names), set(over) - set(names)
    a = dict(BASE, **over)
    return getattr(_lib.lib(), f"skv_linear_rows_{fmt}")(*[a[n] for n in names])


@pytest.mark.parametrize("fmt", FORMATS)
def test_null_pointers_and_sizes(fmt):
    for p in ["W", "X", "Y"] + (["scale"] if fmt == "fp8" else []):
        assert call(fmt, **{p: 0}) == ARG, p
        assert call(fmt, **{p: 0}, M=33) == ARG and call(fmt, **{p: 0}, K=STEP[fmt] + 8) == ARG, p      # pointers before the shape
    for bad in (dict(M=0), dict(M=-3), dict(N=0), dict(N=-16)):
        assert call(fmt, **bad) == ARG, bad
        assert call(fmt, **bad, K=STEP[fmt] + 8) == ARG, bad                                            # M, N < 1 before K
    assert call(fmt, M=33) == UNSUPPORTED and call(fmt, M=1000) == UNSUPPORTED
    assert call(fmt, M=33, bias=P) == UNSUPPORTED


@pytest.mark.parametrize("fmt", FORMATS)
def test_k_refusals(fmt):
    step = STEP[fmt]
    for K in (4096 + step // 2, 4096 + 8, 100, step + 1):               # not a multiple of the k-step
        assert call(fmt, K=K) == UNSUPPORTED, K
    for K in (step // 2, 8, 0):                                         # below one k-step
        assert call(fmt, K=K) == UNSUPPORTED, K
    assert call(fmt, K=-step) == UNSUPPORTED
    assert call("fp8", K=4096 + 32) == UNSUPPORTED                      # a bf16 k-step is half an FP8 k-step


@pytest.mark.parametrize("fmt", FORMATS)
def test_silu_refusals_and_the_order_of_the_checks(fmt):
    assert call(fmt, silu=1, N=511) == ARG                              # an odd number of [gate; up] rows
    assert call(fmt, silu=1, bias=P) == ARG                             # a SiLU launch has no bias slot
    assert call(fmt, silu=1, N=511, W=0) == ARG
    # bf16 tests the shape before the SiLU arguments, FP8 the SiLU arguments first
    first = {"bf16": UNSUPPORTED, "fp8": ARG}[fmt]
    assert call(fmt, silu=1, N=511, M=33) == first
    assert call(fmt, silu=1, bias=P, M=33) == first
    assert call(fmt, silu=1, N=511, K=STEP[fmt] + 8) == first
    assert call(fmt, silu=1, bias=P, K=8) == first
    assert call(fmt, silu=1, K=STEP[fmt] + 8) == UNSUPPORTED            # valid SiLU arguments: the shape refusal in both
