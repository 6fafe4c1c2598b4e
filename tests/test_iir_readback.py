"""Read-back tests of the IIR plans: the plan-time state-transition tables, and the kernels' impulse responses.

CPU: sgx_iir_transition returns M^(2^j), the table that carries a state over 2^j blocks of L samples of zero input.  The tables are
evaluated by running the recurrence in long double and rounded once, so M^(2^(j+1)) must equal M^(2^j) squared to within the rounding
of the entries: every entry of row r of M2 - M1 M1 is within 4 ulp of the row sum sum_c sum_k |M1[r, k]| |M1[k, c]| (one rounding
of each factor and one of the result come to 1.5 ulp of an entry's own sum; the recurrence's own error is relative to the size of the
states it passes through, which is why the measure is the row's and not the entry's).  A table built as a product of rounded tables would miss this from the third level on for the filters with
poles close to the circle.  M^(2^0) itself is checked against the long-double recurrence of tests/iir_ref.py on unit states: half an f64 ulp of the entry and
the reference's own 16 steps of long-double rounding.

GPU: a unit sample at 0, L - 1, L, tile - 1 and tile (the first and last sample of a work item's block, of a tile): the output is
exactly 0.0 before it and the impulse response within the bound of tests/iir_ref.py after it.
"""
import numpy as np
import pytest

import spectrograms_amd as sg
from spectrograms_amd import _ffi
from tests import iir_ref as R
from tests import test_iir as TI

HOST = _ffi.DEVICE_HOST_ONLY


@pytest.mark.parametrize("name", list(R.FILTERS))
def test_transition_tables_square_into_each_other(name):
    sos = R.FILTERS[name]
    plan = sg.IirPlan(sos, device=HOST)
    S = min(len(sos), 8)
    tabs = [plan.transition(j) for j in range(8)]
    assert all(t.shape == (2 * S, 2 * S) for t in tabs)
    for j in range(7):
        m1, m2 = tabs[j].astype(R.LD), tabs[j + 1].astype(R.LD)
        sums = (np.abs(m1) @ np.abs(m1)).sum(axis=1, keepdims=True)
        tol = 4 * np.spacing(sums.astype(np.float64)).astype(R.LD)
        worst = float(np.max(np.abs(m2 - m1 @ m1) / tol))
        print(f"\n{name} level {j + 1}: {4 * worst:.2f} ulp of the row sums")
        assert worst <= 1.0, (name, j, 4 * worst)
    with pytest.raises(sg.InvalidInputError, match="j must be 0 .. 7"):
        plan.transition(8)
    # level 0 is the recurrence itself: L samples of zero input from each unit state
    L = plan.block
    for c in range(2 * S):
        z = np.zeros((S, 2), R.LD)
        z[c // 2, c % 2] = 1
        _, zf = R.ref(sos[:S], np.zeros(L), z)
        want = zf.reshape(-1)
        assert np.all(np.abs(tabs[0][:, c].astype(R.LD) - want) <= np.spacing(np.abs(want).astype(np.float64)) / 2 + 16 * 2.0 ** -64 * np.max(np.abs(want))), (name, c)


def test_transition_tables_of_an_integrator_are_exact():
    # a double integrator's state grows linearly: entries are small integers at every level
    plan = sg.IirPlan([[1.0, 0.0, 0.0, 1.0, -2.0, 1.0]], device=HOST)
    for j in range(8):
        m = plan.transition(j)
        n = plan.block << j
        assert np.array_equal(m, [[n + 1.0, n], [-float(n), 1.0 - n]]), (j, m)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", TI.DTYPES)
@pytest.mark.parametrize("name", ["butter4_hp_0.001", "ellip6_bp", "fir_only"])
def test_gpu_impulse_read_back(name, dtype):
    sos = R.FILTERS[name]
    plan = sg.IirPlan(sos, dtype=dtype)
    L, tile = plan.block, plan.tile
    at = [0, L - 1, L, tile - 1, tile]
    n = tile + 4 * L + 5
    x = np.zeros((len(at), n), TI.NP[dtype])
    x[np.arange(len(at)), at] = 1.0
    y = plan.filter_torch(TI.dev(x)).cpu().numpy()
    h_ref, h_seq = R.ref(sos, x[0])[0], R.seq(sos, x[0])[0]  # the impulse response, from sample 0
    case = f"impulse-{name}-{dtype}"
    for b, p in enumerate(at):
        assert np.all(y[b, :p] == 0.0), (p, np.flatnonzero(y[b, :p]))
        TI.check(case, y[b, p:], h_seq[:n - p], h_ref[:n - p], dtype)
    assert y[0, 0] == TI.NP[dtype](sos[0, 0] if len(sos) == 1 else np.prod(sos[:, 0]))  # h[0] = the product of the b0
    TI.report(case)
