// How mcmc_hip_step cuts a call into spans: runs of steps whose directions are formed together, at
// most max_cyc cycles of L steps (what the direction buffer's byte budget holds).  Plain C++ with
// nothing of HIP in it, so that tests/test_step_span_host.py compiles it with the host compiler.
#pragma once
#include <algorithm>

struct StepSpan {
    unsigned long long c0;   // the cycle of the first step
    int n, ncyc;             // steps, and the cycles c0 .. c0 + ncyc - 1 they lie in
};

// n steps from `step` on
inline StepSpan span_of(unsigned long long step, int n, int L)
{
    const unsigned long long Lu = (unsigned long long)L, c0 = step / Lu;
    return {c0, n, (int)((step + (unsigned long long)n - 1) / Lu - c0 + 1)};
}

// the next span of a call with `left` steps to go: up to the end of cycle c0 + max_cyc - 1
inline StepSpan step_span(unsigned long long step, int left, int L, int max_cyc)
{
    const unsigned long long Lu = (unsigned long long)L;
    const unsigned long long room = (step / Lu + (unsigned long long)max_cyc) * Lu - step;
    return span_of(step, (int)std::min<unsigned long long>((unsigned long long)left, room), L);
}

// ... when dragging: a step takes n_drag columns of the fast directions, whose cycles are Lf
// columns long, and a span holds at most max_cyc_f of those cycles as well (whole steps; never none)
inline StepSpan drag_span(unsigned long long step, int left, int L, int max_cyc, int n_drag, int Lf,
                          int max_cyc_f)
{
    const StepSpan s = step_span(step, left, L, max_cyc);
    const unsigned long long nd = (unsigned long long)n_drag, uLf = (unsigned long long)Lf;
    const unsigned long long fc0 = step * nd / uLf;
    const unsigned long long fend = (fc0 + (unsigned long long)max_cyc_f) * uLf;
    const unsigned long long room_f = (fend - step * nd) / nd;
    return span_of(step, (int)std::min<unsigned long long>((unsigned long long)s.n,
                                                           std::max<unsigned long long>(1, room_f)), L);
}
