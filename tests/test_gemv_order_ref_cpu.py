"""CPU: tests/gemv_order_ref.py against exact rational arithmetic, its sensitivity to the order it states, and the seeds
the GPU test uses (no f64 step of theirs is inexact - the helper's condition - at every shape)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import dense_ref as dr
import gemv_order_ref as go


def round_f32(q):
    """Fraction -> nearest f32 (ties to even) as Fraction; normal range only (asserted)."""
    if q == 0:
        return Fraction(0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e <= 127
    ulp = Fraction(2) ** (e - 23)
    n, rest = divmod(a, ulp)
    if rest > ulp / 2 or (rest == ulp / 2 and n % 2):
        n += 1
    return sign * n * ulp


def exact_row(w_row, x):
    """One row by the stated order in rational arithmetic: every fma and every add rounded once, exactly."""
    w_row, x = [Fraction(float(v)) for v in w_row.float()], [Fraction(float(v)) for v in x.float()]
    K = len(x)
    steps, tail = K // go.STEP, K % go.STEP
    acc = [[Fraction(0)] * 8 for _ in range(64)]
    for s in range(steps + (1 if tail else 0)):
        lanes = 64 if s < steps else tail // 8
        for l in range(lanes):
            for e in range(8):
                k = s * go.STEP + 8 * l + e
                acc[l][e] = round_f32(w_row[k] * x[k] + acc[l][e])
    add = lambda a, b: round_f32(a + b)
    v = [add(add(add(a[0], a[1]), add(a[2], a[3])), add(add(a[4], a[5]), add(a[6], a[7]))) for a in acc]
    while len(v) > 1:
        v = [add(v[i], v[i + 1]) for i in range(0, len(v), 2)]
    return v[0]


@pytest.mark.parametrize("N,K,seed", go.PLAIN_CASES + [go.NORM_CASE])
def test_restatement_matches_rational_arithmetic(N, K, seed):
    w, x, _ = go.gaussian(N, K, seed)
    tot, bad = go.row_totals(w, x)
    assert bad == 0
    for n in (0, N // 2, N - 1):
        want = exact_row(w[n], x)
        assert Fraction(float(tot[n])) == want, f"row {n}: restated {float(tot[n])!r}, exact {float(want)!r}"


def test_round_f32_helper():
    for v in (1.0, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -0.3, 1e-20, 12345.678):
        assert float(round_f32(Fraction(v))) == float(np.float32(v)), v


@pytest.mark.parametrize("N,K,seed", go.PLAIN_CASES)
def test_seeds_leave_no_doubly_rounded_step(N, K, seed):
    w, x, bias = go.gaussian(N, K, seed)
    y = go.restate(w, x, bias)            # asserts the condition
    # and the restated result is a sane dot product: within one bf16 ulp of the f64 evaluation
    ref = dr.finish64(x.double() @ w.double().t(), bias)
    assert bool(((y.double() - ref).abs() <= 2.0 ** -7 * ref.abs() + 2.0 ** -133).all())


def test_seeds_of_the_norm_and_q_cases():
    for glm in (False, True):
        c = go.q_case(glm)
        assert go.row_totals(c["w"][:c["Hq"] * 128], c["xn"])[1] == 0
    c = go.norm_case()
    assert go.row_totals(c["w"], c["xn"])[1] == 0


def cancelling_rows_moved(w, x, order):
    tot, _ = go.row_totals(w, x)
    other, _ = go.row_totals(w, x, order)
    return int((dr.bits(go.finish(other)) != dr.bits(go.finish(tot)))[1::2].sum())


@pytest.mark.parametrize("N,K,seed", go.PLAIN_CASES[:2])
def test_a_swapped_k_order_changes_bits(N, K, seed):
    """The order is observable in the bf16 OUTPUTS on these inputs.  An odd row returns the rounding residue of its 512 f32
    chains; a change of order that alters one rounding in one chain gives another residue, so practically every odd row moves
    and at least half of them (N / 4 rows) MUST, for each of: first and last k-step swapped; the steps descending; the two
    buffers of the kernel's pipeline exchanged (k-steps 4 .. 7 in front of 0 .. 3 - the mistake a two-buffer stream invites)."""
    w, x, _ = go.gaussian(N, K, seed)
    for name, order in orders(K // go.STEP):
        moved = cancelling_rows_moved(w, x, order)
        print(f"N {N} K {K} {name}: {moved} of {N // 2} cancelling rows move")
        assert moved >= N // 4, f"{name}: only {moved} of {N // 2} cancelling rows move"


def orders(steps):
    ends = list(range(steps))
    ends[0], ends[-1] = ends[-1], ends[0]
    return (("ends", ends), ("descending", list(range(steps))[::-1]),
            ("buffers", list(range(4, 8)) + list(range(4)) + list(range(8, steps))))


def test_a_swapped_k_order_changes_bits_of_the_norm_and_q_cases():
    for what, c in (("norm", go.norm_case()), ("q neox", go.q_case(False)), ("q glm", go.q_case(True))):
        w = c["w"][:c["Hq"] * 128] if "Hq" in c else c["w"]
        for name, order in orders(8):
            moved = cancelling_rows_moved(w, c["xn"], order)
            print(f"{what} {name}: {moved} of {w.shape[0] // 2} cancelling rows move")
            assert moved >= w.shape[0] // 4, f"{what} {name}: only {moved} of {w.shape[0] // 2} cancelling rows move"
