"""GPU: every boundary of the pipelined weight stream of skv_gemv.hip (NORM == false) on the integer-exact inputs of
tests/dense_ref.py.  The stream runs in groups of 4 k-steps at two rows per wave (2 at four): request the first group; while
three or more are left, two per loop iteration; a drain of two groups or one; then the end of the row - the whole k-steps
that fill no group and the K % 512 tail - as a request of its own.  test_gpu_dense_exact.py reaches 1, 2, 8 and 26 k-steps;
the K values here are 3, 4, 5, 7, 8, 9, 12 + an 8-element tail and 28 k-steps: no whole group, exactly one, one + a step,
one + three steps, two (the drain of two), two + a step, three (one loop iteration + the drain of one) with a one-lane tail,
seven (three iterations + the drain of one).  A dropped, doubled or misplaced k element changes the integer; raw bits;
sentinels past every output."""
import pytest

import dense_ref as dr
from test_gpu_dense_exact import SENT, assert_bits, assert_silu, dev16, run_gemv, weights_on_device

pytestmark = pytest.mark.gpu
KS = (1536, 2048, 2560, 3584, 4096, 4608, 6152, 14336)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", [9, 4101, 8209])
def test_gemv_plain_every_pipeline_boundary(N, K):
    """N 9 and 4101: skv_gemv_kernel<2> (a ragged last wave at both; 4101: more than one workgroup); 8209: <4>."""
    bank = dr.plain_bank(N, K, seed=N + K)
    w = weights_on_device(bank)
    xi, _ = dr.structured_x(1, K, seed=K)
    x = dev16(xi)
    for bias in (None, dr.integer_bias(N, seed=N)):
        y, _, _ = run_gemv(bank, w, x, None if bias is None else dev16(bias), silu=False)
        assert_bits(y[:, :N], dr.gemv_ref(bank, xi, bias)[0], f"gemv N {N} K {K} bias {bias is not None}")
        assert bool((y[:, N:] == SENT).all()), "written past N"


@pytest.mark.parametrize("K", KS)
def test_gemv_silu_pair_every_pipeline_boundary(K):
    I = 1003
    xi, colsign = dr.structured_x(1, K, seed=K + 1)
    bank = dr.pair_bank(I, K, seed=I + K, colsign=colsign)
    w = weights_on_device(bank)
    g, u, ref = dr.pair_ref(bank, xi)
    assert bool((g != 0).all()) and bool((u != 0).all())
    y, _, _ = run_gemv(bank, w, dev16(xi), None, silu=True)
    assert_silu(y[:, :I], ref[0], f"gemv silu I {I} K {K}")
    assert bool((y[:, I:] == SENT).all()), "written past I"
