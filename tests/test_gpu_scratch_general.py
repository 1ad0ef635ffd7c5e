"""step_general_kernel and drag_general_kernel (run-time d, one symbol each) once per reason
scratch_choose (csrc/scratch_choice.h) sends a shape to them: the cases of
tests/instantiations.py: general_cases, run like the from-scratch part of the instantiation sweep
(tests/test_gpu_instantiations.py) -- 5 steps, then d + 7, device against oracle bit for bit, the
kernel pinned by name -- and with the emitted rows compared where a case emits."""
import pytest

pytestmark = pytest.mark.gpu

from tests import instantiations as I  # noqa: E402
from tests.test_gpu_instantiations import run_all  # noqa: E402
from tests.test_gpu_parity import assert_bit_equal, compare_state, make_pair  # noqa: E402

CASES = I.general_cases()


def what_of(c):
    why = ("drag" if c.drag else "own" if c.own else "emit" if c.emit else "periodic" if c.periodic else
           "normal" if c.prior == 2 else f"K{c.K}" if c.K != 1 else f"W{c.W}")
    return f"d{c.d}-{why}"


def run_general_case(c):
    args, kw = I.scratch_pair_arguments(c)
    eng, prob, st = make_pair(*args, **kw)
    try:
        compare_state(eng, st)
        for launch, n in enumerate(I.scratch_steps(c)):
            eng.step(n)
            eng.sync()
            st.run(n, n_threads=8)
            where = f"{what_of(c)}: launch {launch}, after step {st.step}: "
            try:
                compare_state(eng, st)
            except AssertionError as e:
                raise AssertionError(where + str(e)) from None
            if c.emit:
                rows, ref = eng.drain_samples(), st.drain()
                assert rows.shape == ref.shape and len(rows) > 0, where + f"{rows.shape} rows against {ref.shape}"
                assert_bit_equal(rows, ref, where + "emitted rows")
            assert eng.last_step_kernel() == f"{c.name} (d={c.d})", where + eng.last_step_kernel()
        counters = eng.counters()
        assert counters["accepted"] == int(st.n_accept.sum()) and counters["dropped_rows"] == 0
    finally:
        eng.close()


@pytest.mark.parametrize("c", CASES, ids=[what_of(c) for c in CASES])
def test_the_general_kernels_bit_exact_for_every_reason_they_are_chosen(c):
    run_all([c], run_general_case)
