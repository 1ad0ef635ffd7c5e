/* A restatement of the stretch move on a function target ("Stretch move"):
 * the two halves of a HALF-UPDATE around the user's batched log-likelihood, on heap buffers and for
 * any d.  The log-prior of the trial comes from the caller (orc_evaluate of the K = 0 problem:
 * eval_point), the log-likelihoods from OUTSIDE -- whatever the function returned for the trial.
 * The variates are one Philox block per walker and step on the stream 0x2000, built from the oracle
 * library's exports, resolved at load time.  Compiled by the tests with -ffp-contract=off, like
 * the oracle: fused operations are fma(). */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

void orc_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]);
double orc_dlog(double x);

static double u52(uint64_t k) { return (double)(2 * k + 1) * 0x1p-53; }

/* (member of the other half, z, E_a) of walker gid at step `step`; log2_half = log2(group_size / 2) */
void st_ref_variates(uint64_t seed, uint32_t gid, uint64_t step, int log2_half, double a,
                     int32_t* member, double* z, double* Ea)
{
    uint32_t w[4];
    orc_philox((uint32_t)seed, (uint32_t)(seed >> 32), gid, 0x2000u, (uint32_t)step, (uint32_t)(step >> 32), w);
    *member = (int32_t)(w[0] >> (32 - log2_half));
    const uint64_t kz = ((uint64_t)w[1] << 20) | (w[2] >> 12);
    const uint64_t ka = ((uint64_t)w[3] << 20) | ((uint64_t)(w[2] & 0xFFFu) << 8) | (w[0] & 0xFFu);
    const double s = fma(a - 1.0, u52(kz), 1.0);
    *z = (s * s) / a;
    *Ea = -orc_dlog(u52(ka));
}

/* PROPOSE of half-update `half`: x[W][d] the current state -- or, where xp != x, the state the
 * PARTNERS are read from (the tests' deliberately wrong ordering) --; out, indexed by the active
 * walker k = g (gs / 2) + m in ascending walker order: t[W / 2][d], Ea[W / 2], q[W / 2] = (d - 1) log z,
 * partner[W / 2] (local walker index) */
void st_ref_propose(int d, int W, int gs, int half, uint32_t walker0, uint64_t seed, uint64_t step, double a,
                    const double* x, const double* xp, double* t, double* Ea, double* q, int32_t* partner)
{
    const int hg = gs / 2;
    int log2_half = 0;
    while ((1 << log2_half) < hg) ++log2_half;
    for (int k = 0; k < W / 2; ++k) {
        const int g = k / hg, m = k % hg;
        const int w = g * gs + half * hg + m;
        int32_t pm;
        double z;
        st_ref_variates(seed, walker0 + (uint32_t)w, step, log2_half, a, &pm, &z, Ea + k);
        const int wp = g * gs + (1 - half) * hg + pm;
        partner[k] = wp;
        q[k] = (double)(d - 1) * orc_dlog(z);
        const double *xw = x + (size_t)w * d, *p = xp + (size_t)wp * d;
        for (int i = 0; i < d; ++i) t[(size_t)k * d + i] = fma(z, xw[i] - p[i], p[i]);
    }
}

/* ACCEPT of half-update `half`: lp[W / 2] log-prior of the trial (-inf outside the support),
 * ll[W / 2] what the function returned (ignored outside the support), Ea, q.  Returns the number of
 * accepted walkers; bad[0] = 1 + global id of the first walker whose value inside the support is NaN
 * or +inf. */
int64_t st_ref_accept(int d, int W, int gs, int half, uint32_t walker0, double temperature, double max_tries,
                      const double* t, const double* lp, const double* ll, const double* Ea, const double* q,
                      double* x, double* logpost, double* logprior, double* loglike,
                      int32_t* weight, int32_t* prior_rej, int32_t* burn_left, int64_t* n_accept,
                      int32_t* stuck, int32_t* bad)
{
    const int hg = gs / 2;
    int64_t total = 0;
    for (int k = 0; k < W / 2; ++k) {
        const int w = (k / hg) * gs + half * hg + k % hg;
        const int inb = lp[k] != -INFINITY;
        const int isbad = inb && (ll[k] != ll[k] || ll[k] == INFINITY);
        if (isbad && !*bad) *bad = 1 + (int32_t)(walker0 + (uint32_t)w);
        const double lt = inb ? lp[k] + ll[k] : -INFINITY;
        const int accept = inb && !isbad && lt != -INFINITY &&
                           Ea[k] > (logpost[w] - lt) / temperature - q[k];
        if (accept) {
            if (burn_left[w] > 0) burn_left[w] -= 1;
            for (int i = 0; i < d; ++i) x[(size_t)w * d + i] = t[(size_t)k * d + i];
            logprior[w] = lp[k]; loglike[w] = ll[k]; logpost[w] = lt;
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
