"""How mcmc_hip_step cuts a call into spans of direction cycles (cobaya_amd/csrc/step_span.h), on the
CPU: a stand-alone program, built with the host compiler, prints the spans of a list of calls; they
are compared with a restatement in Python integers and with what a cutting has to satisfy whatever
its rule.  On the device a span ends inside a call only at production sizes (the direction buffer
holds hundreds of thousands of cycles at a test's) or under MCMC_HIP_DIR_BUDGET_KIB
(tests/test_gpu_direction_spans.py)."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cobaya_amd", "csrc")
P32, P33 = 1 << 32, 1 << 33

# standard input: one call per line, "step n_steps L max_cyc n_drag Lf max_cyc_f" (n_drag = 0: no
# dragging); standard output: one span per line, "call step c0 n ncyc"
PROGRAM = r"""
#include <cstdio>

#include "step_span.h"

int main()
{
    unsigned long long step;
    int left, L, max_cyc, n_drag, Lf, max_cyc_f;
    for (int call = 0; std::scanf("%llu %d %d %d %d %d %d", &step, &left, &L, &max_cyc, &n_drag, &Lf,
                                  &max_cyc_f) == 7; ++call)
        while (left > 0) {
            const StepSpan s = n_drag > 0 ? drag_span(step, left, L, max_cyc, n_drag, Lf, max_cyc_f)
                                          : step_span(step, left, L, max_cyc);
            std::printf("%d %llu %llu %d %d\n", call, step, s.c0, s.n, s.ncyc);
            if (s.n < 1) return 1;   // (the test reports it; no endless loop here)
            step += (unsigned long long)s.n;
            left -= s.n;
        }
    return 0;
}
"""


def spans_restated(step, left, L, max_cyc, n_drag=0, Lf=0, max_cyc_f=0):
    """[(step, c0, n, ncyc)] of one call, in Python's integers."""
    out = []
    while left > 0:
        c0 = step // L
        n = min(left, (c0 + max_cyc) * L - step)
        if n_drag:
            fc0 = step * n_drag // Lf
            n = min(n, max(1, ((fc0 + max_cyc_f) * Lf - step * n_drag) // n_drag))
        out.append((step, c0, n, (step + n - 1) // L - c0 + 1))
        step, left = step + n, left - n
    return out


def calls():
    """(step, n_steps, L, max_cyc, n_drag, Lf, max_cyc_f): per cycle length and budget, calls that
    start in the middle of a cycle (L > 1), on a cycle, and far out; that end inside the first span,
    exactly at a span's end, one step past it, and several spans on."""
    out = []
    for L in (1, 2, 13, 60):
        for max_cyc in (1, 2, 9):
            for drag in ((0, 0, 0), (3, 4, 2)):
                starts = [0, L // 2, 5 * L + L - 1, 7 * max_cyc * L + L // 3,
                          P32 - 5, P32 * L - 3, P33 + 8]
                for step in starts:
                    room = (step // L + max_cyc) * L - step      # to the end of the first span
                    for n_steps in {1, room, room + 1, room + 3 * max_cyc * L, room + 3 * max_cyc * L + 1}:
                        out.append((step, n_steps, L, max_cyc) + drag)
    return out


@pytest.fixture(scope="module")
def spans_of_program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("step_span")
    src, exe = tmp / "step_span_main.cpp", tmp / "step_span_main"
    src.write_text(PROGRAM)
    subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                   check=True)
    text = "".join("%d %d %d %d %d %d %d\n" % c for c in calls())
    res = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True)
    per_call = [[] for _ in calls()]
    for line in res.stdout.splitlines():
        call, *span = (int(w) for w in line.split())
        per_call[call].append(tuple(span))
    return per_call


def test_cases_cover_what_they_should():
    cs = calls()
    assert {c[2] for c in cs} == {1, 2, 13, 60} and {c[3] for c in cs} == {1, 2, 9}
    assert any(c[0] % c[2] for c in cs)                                    # starts inside a cycle
    for L in (1, 2, 13, 60):
        assert {P32 - 5, P32 * L - 3, P33 + 8} <= {c[0] for c in cs if c[2] == L}
    assert any(c[4:] == (3, 4, 2) for c in cs)
    ends = [(c, spans_restated(*c)) for c in cs if not c[4]]
    assert any(len(s) == 1 and (c[0] + c[1]) % c[2] == 0 and s[0][3] == c[3] for c, s in ends)   # ends at a span's end
    assert any(len(s) == 2 and s[1][2] == 1 for c, s in ends)                                   # ... one step past it
    assert max(len(s) for c, s in ends) >= 4


def test_spans_equal_the_restatement(spans_of_program):
    for c, got in zip(calls(), spans_of_program):
        assert got == spans_restated(*c), c


def test_spans_tile_the_call_within_the_budget(spans_of_program):
    for c, got in zip(calls(), spans_of_program):
        step0, n_steps, L, max_cyc, n_drag, Lf, max_cyc_f = c
        at = step0
        for i, (step, c0, n, ncyc) in enumerate(got):
            assert step == at and n >= 1, (c, got)                     # no gap, no overlap, never empty
            assert c0 == step // L and ncyc == (step + n - 1) // L - c0 + 1, (c, got)
            assert 1 <= ncyc <= max_cyc, (c, got)
            if n_drag:     # the fast columns [step n_drag, (step + n) n_drag) lie in max_cyc_f cycles
                assert ((step + n) * n_drag - 1) // Lf - step * n_drag // Lf + 1 <= max_cyc_f, (c, got)
            elif i + 1 < len(got):   # without dragging a span inside a call is full: it ends with cycle c0 + max_cyc - 1
                assert step + n == (c0 + max_cyc) * L, (c, got)
            at += n
        assert at == step0 + n_steps, (c, got)
