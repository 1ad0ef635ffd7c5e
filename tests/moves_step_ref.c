/* A restatement of the mixtures of ensemble moves on a function target (DESIGN.md section 2,
 * "Ensemble move mixtures"): the word that chooses the kind of a step, and the two halves of a
 * HALF-UPDATE of each kind -- stretch, differential evolution, snooker -- on heap buffers and for any
 * d.  The log-prior of the trial comes from the caller (orc_evaluate of the K = 0 problem), the
 * log-likelihoods from OUTSIDE.  Built from the oracle library's exports, resolved at load time;
 * compiled by the tests with -ffp-contract=off, like the oracle: fused operations are fma().
 * `flaw` states a deliberately WRONG rule, for the tests' power checks: 1 = DE draws its second
 * partner without the + 1 shift (p1 = p2 is allowed); 2 = snooker takes z from the second draw and
 * z1 from the first. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

void orc_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]);
double orc_dlog(double x);
void orc_sincos2pi(uint64_t k, double* sn, double* cs);

enum { STRETCH = 0, DE = 1, SNOOKER = 2 };
static const uint32_t STREAM[3] = {0x2000u, 0x2002u, 0x2003u};

static double u52(uint64_t k) { return (double)(2 * k + 1) * 0x1p-53; }
static uint64_t k_hi(const uint32_t w[4]) { return ((uint64_t)w[1] << 20) | (w[2] >> 12); }
static uint64_t k_lo(const uint32_t w[4])
{
    return ((uint64_t)w[3] << 20) | ((uint64_t)(w[2] & 0xFFFu) << 8) | (w[0] & 0xFFu);
}

/* word 0 of the block (0, 0x2001, S_lo, S_hi): the kind of step S, by inverse CDF (the caller's) */
uint32_t mv_ref_kind_word(uint64_t seed, uint64_t step)
{
    uint32_t w[4];
    orc_philox((uint32_t)seed, (uint32_t)(seed >> 32), 0u, 0x2001u, (uint32_t)step, (uint32_t)(step >> 32), w);
    return w[0];
}

/* sum of u_i v_i in the chain shape of the log-prior */
static double dot(int d, const double* u, const double* v)
{
    if (d <= 32) {
        double s = 0.0;
        for (int i = 0; i < d; ++i) s = fma(u[i], v[i], s);
        return s;
    }
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < d; ++i) c[i & 3] = fma(u[i], v[i], c[i & 3]);
    return (c[0] + c[1]) + (c[2] + c[3]);
}

/* The variates of walker gid at step `step` for a trial of `kind`: members m[3] of the other half
 * (stretch: m[0]; de: m[0], m[1]; snooker: all three), E_a, and f = z (stretch) or gamma (de; p0 =
 * gamma0, p1 = sigma); snooker has no f. */
void mv_ref_variates(uint64_t seed, uint32_t gid, uint64_t step, int log2_half, int kind, double p0, double p1,
                     int flaw, int32_t m[3], double* f, double* Ea)
{
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), lo = (uint32_t)step, hi = (uint32_t)(step >> 32);
    const int hg = 1 << log2_half;
    uint32_t w[4], b[4];
    orc_philox(k0, k1, gid, STREAM[kind], lo, hi, w);
    m[0] = (int32_t)(w[0] >> (32 - log2_half));
    m[1] = m[2] = -1;
    *Ea = -orc_dlog(u52(k_lo(w)));
    *f = 0.0;
    if (kind == STRETCH) {
        const double s = fma(p0 - 1.0, u52(k_hi(w)), 1.0);
        *f = (s * s) / p0;
        return;
    }
    const int shift = (kind == DE && flaw == 1) ? 0 : 1;
    m[1] = (int32_t)((m[0] + shift + (int)(((uint64_t)w[1] * (uint64_t)(hg - 1)) >> 32)) % hg);
    orc_philox(k0, k1, gid, STREAM[kind] | 0x10u, lo, hi, b);
    if (kind == DE) {
        double sn, cs;
        orc_sincos2pi(k_lo(b), &sn, &cs);
        const double n = sqrt(-2.0 * orc_dlog(u52(k_hi(b)))) * cs;
        *f = p0 * fma(p1, n, 1.0);
        return;
    }
    int j = (int)(((uint64_t)b[0] * (uint64_t)(hg - 2)) >> 32);
    const int mlo = m[0] < m[1] ? m[0] : m[1], mhi = m[0] < m[1] ? m[1] : m[0];
    if (j >= mlo) ++j;
    if (j >= mhi) ++j;
    m[2] = j;
    if (flaw == 2) { const int32_t s = m[0]; m[0] = m[1]; m[1] = s; }
}

/* PROPOSE of half-update `half` with a move of `kind`: x[W][d] the current state; out, indexed by
 * the active walker k = g (gs / 2) + m in ascending walker order: t[W / 2][d], Ea, q, whole[W / 2]
 * (0: the void trial of a snooker walker that sits on its partner -- t = x, q = -inf),
 * partner[W / 2][3] (local walker indices, -1 where the kind draws none); scratch[2 d] */
void mv_ref_propose(int d, int W, int gs, int half, uint32_t walker0, uint64_t seed, uint64_t step, int kind,
                    double p0, double p1, int flaw, const double* x, double* t, double* Ea, double* q,
                    int32_t* whole, int32_t* partner, double* scratch)
{
    const int hg = gs / 2;
    int log2_half = 0;
    while ((1 << log2_half) < hg) ++log2_half;
    double *dl = scratch, *dz = scratch + d;
    for (int k = 0; k < W / 2; ++k) {
        const int g = k / hg, w = g * gs + half * hg + k % hg, other = g * gs + (1 - half) * hg;
        int32_t m[3];
        double f;
        mv_ref_variates(seed, walker0 + (uint32_t)w, step, log2_half, kind, p0, p1, flaw, m, &f, Ea + k);
        for (int j = 0; j < 3; ++j) partner[3 * k + j] = m[j] < 0 ? -1 : other + m[j];
        const double *xw = x + (size_t)w * d, *a = x + (size_t)(other + m[0]) * d;
        double* tk = t + (size_t)k * d;
        whole[k] = 1;
        if (kind == STRETCH) {
            q[k] = (double)(d - 1) * orc_dlog(f);
            for (int i = 0; i < d; ++i) tk[i] = fma(f, xw[i] - a[i], a[i]);
        } else if (kind == DE) {
            const double* b = x + (size_t)(other + m[1]) * d;
            q[k] = 0.0;
            for (int i = 0; i < d; ++i) tk[i] = fma(f, a[i] - b[i], xw[i]);
        } else {
            const double *z1 = x + (size_t)(other + m[1]) * d, *z2 = x + (size_t)(other + m[2]) * d;
            for (int i = 0; i < d; ++i) { dl[i] = xw[i] - a[i]; dz[i] = z1[i] - z2[i]; }
            const double n2 = dot(d, dl, dl), s = dot(d, dl, dz);
            int ok = n2 > 0.0;
            const double c = ok ? (p0 * s) / n2 : 0.0;
            for (int i = 0; i < d; ++i) { tk[i] = fma(c, dl[i], xw[i]); dz[i] = tk[i] - a[i]; }
            const double nt2 = dot(d, dz, dz);
            ok = ok && nt2 > 0.0;
            q[k] = ok ? (double)(d - 1) * (0.5 * orc_dlog(nt2) - 0.5 * orc_dlog(n2)) : -INFINITY;
            whole[k] = ok;
        }
    }
}

/* ACCEPT of half-update `half`, whatever kind proposed it: lp[W / 2] log-prior of the trial (-inf
 * outside the support AND for a void trial), ll[W / 2] what the function returned (ignored where lp
 * is -inf), Ea, q.  A void trial (q = -inf) is rejected and is no prior rejection.  Returns the
 * number of accepted walkers; bad[0] = 1 + global id of the first walker whose value inside the
 * support is NaN or +inf. */
int64_t mv_ref_accept(int d, int W, int gs, int half, uint32_t walker0, double temperature, double max_tries,
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
            if (!inb && q[k] != -INFINITY) prior_rej[w] += 1;
            const double max_now = max_tries * (burn_left[w] > 0 ? 10.0 : 1.0);
            if ((double)(weight[w] - prior_rej[w]) > max_now && !*stuck)
                *stuck = 1 + (int32_t)(walker0 + (uint32_t)w);
        }
    }
    return total;
}
