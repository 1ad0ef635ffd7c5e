/* A restatement of the Metropolis step of a FUNCTION target ("Function
 * targets"): the two halves around the user's batched log-likelihood, on heap buffers and for any
 * d.  The Haar columns come from the caller (orc_basis), the log-prior of the trial from the
 * caller too (orc_evaluate of the K = 0 problem: eval_point), the log-likelihoods from OUTSIDE --
 * whatever the function returned for the trial.  The variates are the un-paired stream of the
 * from-scratch kernels (oracle: walker_variates, sub 0; the RandProposer1D form at d = 1), built
 * from the oracle library's exports, resolved at load time.  Compiled by the tests with
 * -ffp-contract=off, like the oracle: fused operations are fma(). */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

void orc_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]);
double orc_dlog(double x);
void orc_sincos2pi(uint64_t k, double* sn, double* cs);

static double u52(uint64_t k) { return (double)(2 * k + 1) * 0x1p-53; }

static void step_variates(uint64_t seed, uint32_t gid, uint64_t step, int oned, double* r_out, double* Ea_out)
{
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t wd[4];
    orc_philox(k0, k1, gid, 0u, (uint32_t)step, (uint32_t)(step >> 32), wd);
    const uint64_t kr = ((uint64_t)wd[1] << 20) | (wd[2] >> 12);
    const uint64_t ka = ((uint64_t)wd[3] << 20) | ((uint64_t)(wd[2] & 0xFFFu) << 8) | (wd[0] & 0xFFu);
    const double Er = -orc_dlog(u52(kr));
    const int expo = (wd[0] >> 8) < 5536481u;   /* 0.33 of 2^24 (proposal.py:79) */
    if (oned) {
        double sn, cs;
        orc_sincos2pi(ka, &sn, &cs);
        const double rr = expo ? Er : sqrt(2.0 * Er) * fabs(cs);
        *r_out = (wd[0] & 0x80u) ? rr : -rr;
        uint32_t w2[4];
        orc_philox(k0, k1, gid, 0x100u, (uint32_t)step, (uint32_t)(step >> 32), w2);
        *Ea_out = -orc_dlog(u52(((uint64_t)w2[0] << 20) | (w2[1] >> 12)));
    } else {
        const double rr = expo ? Er : sqrt(2.0 * Er);
        *r_out = (wd[0] & 0x80u) ? rr : -rr;
        *Ea_out = -orc_dlog(u52(ka));
    }
}

/* PROPOSE: v[G][d] = the column of this step for every group; x[W][d]; out: t[W][d], Ea[W] */
void fn_ref_propose(int d, int W, int gs, uint32_t walker0, uint64_t seed, uint64_t step,
                    const double* v, const double* x, double* t, double* Ea)
{
    for (int w = 0; w < W; ++w) {
        double r;
        step_variates(seed, walker0 + (uint32_t)w, step, d == 1, &r, Ea + w);
        const double* vg = v + (size_t)(w / gs) * d;
        for (int i = 0; i < d; ++i) t[(size_t)w * d + i] = fma(r, vg[i], x[(size_t)w * d + i]);
    }
}

/* ACCEPT: lp[W] log-prior of the trial (-inf outside the support), ll[W] what the function
 * returned (ignored outside the support), Ea[W].  Returns the number of accepted walkers;
 * bad[0] = 1 + global id of the first walker whose value inside the support is NaN or +inf. */
int64_t fn_ref_accept(int d, int W, uint32_t walker0, double temperature, double max_tries,
                      const double* t, const double* lp, const double* ll, const double* Ea,
                      double* x, double* logpost, double* logprior, double* loglike,
                      int32_t* weight, int32_t* prior_rej, int32_t* burn_left, int64_t* n_accept,
                      int32_t* stuck, int32_t* bad)
{
    int64_t total = 0;
    for (int w = 0; w < W; ++w) {
        const int inb = lp[w] != -INFINITY;
        const int isbad = inb && (ll[w] != ll[w] || ll[w] == INFINITY);
        if (isbad && !*bad) *bad = 1 + (int32_t)(walker0 + (uint32_t)w);
        const double lt = inb ? lp[w] + ll[w] : -INFINITY;
        const int accept = inb && !isbad && lt != -INFINITY &&
                           (lt > logpost[w] || Ea[w] > (logpost[w] - lt) / temperature);
        if (accept) {
            if (burn_left[w] > 0) burn_left[w] -= 1;
            for (int i = 0; i < d; ++i) x[(size_t)w * d + i] = t[(size_t)w * d + i];
            logprior[w] = lp[w]; loglike[w] = ll[w]; logpost[w] = lt;
            weight[w] = 1; prior_rej[w] = 0; n_accept[w] += 1;
            ++total;
        } else {
            weight[w] += 1;
            if (!inb) prior_rej[w] += 1;
            const double max_now = max_tries * (burn_left[w] > 0 ? 10.0 : 1.0);
            if ((double)(weight[w] - prior_rej[w]) > max_now && !*stuck)
                *stuck = 1 + (int32_t)(walker0 + (uint32_t)w);
        }
    }
    return total;
}
