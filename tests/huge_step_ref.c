/* A d-agnostic restatement of the oracle's incremental Metropolis step (oracle/mcmc_oracle.c:
 * step_core_inc, commit, orc_anchor_loglike and the plain-step branch of orc_run) for ONE
 * parameter block, 1..4 Gaussian modes, no periodic parameter and no emitted rows -- and, for the
 * `one` likelihood (K = 0), its from-scratch step (step_core with eval_point, ll = 0) -- on heap
 * buffers: the oracle's own step functions hold 128-element stack arrays, so they must not see
 * d > 128.  The Haar columns come from the caller (orc_basis, which is d-agnostic); the variates
 * and the table-driven exp / log are the oracle library's exports, resolved at load time.
 * Compiled by the tests with -ffp-contract=off, like the oracle: fused operations are fma(). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

void orc_pair_variates(uint64_t seed, uint32_t gid, uint64_t step, double* r_out, double* Ea_out);
void orc_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]);
double orc_dlog(double x);

/* the un-paired variates of a plain step (oracle: walker_variates, sub 0, not a one-parameter block) */
static void step_variates(uint64_t seed, uint32_t gid, uint64_t step, double* r_out, double* Ea_out)
{
    uint32_t wd[4];
    orc_philox((uint32_t)seed, (uint32_t)(seed >> 32), gid, 0u, (uint32_t)step, (uint32_t)(step >> 32), wd);
    const uint64_t kr = ((uint64_t)wd[1] << 20) | (wd[2] >> 12);
    const uint64_t ka = ((uint64_t)wd[3] << 20) | ((uint64_t)(wd[2] & 0xFFFu) << 8) | (wd[0] & 0xFFu);
    const double Er = -orc_dlog((double)(2 * kr + 1) * 0x1p-53);
    const double rr = ((wd[0] >> 8) < 5536481u) ? Er : sqrt(2.0 * Er);
    *r_out = (wd[0] & 0x80u) ? rr : -rr;
    *Ea_out = -orc_dlog((double)(2 * ka + 1) * 0x1p-53);
}
double orc_dexp_tab(double x);
double orc_dlog_tab(double x);

static double four_chain_squares(const double* a, int d)
{
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < d; ++i) s[i & 3] = fma(a[i], a[i], s[i & 3]);
    return (s[0] + s[1]) + (s[2] + s[3]);
}

/* prior: lo, hi, loc, inv (1/scale; 0 = not normal), mls, each [d].  State walker-major:
 * x [W][d], y [W][K][d].  V: [G][ncyc][d][d] Haar columns (column c of a cycle at c d), cycles
 * counted from cyc0.  anchor: refresh y (and re-anchor one mode) before the first step. */
int64_t huge_ref_run(int d, int K, int W, int gs, uint32_t walker0, uint64_t seed, uint64_t step0,
                     int n_steps, uint64_t refresh, int anchor, const double* V, uint64_t cyc0, int ncyc,
                     const double* lo, const double* hi, const double* loc, const double* inv,
                     const double* mls, const double* scale, const double* Linv, const double* mean, const double* cnorm,
                     const double* mweight, double uniform_logp, double temperature, double max_tries,
                     double* x, double* y, double* logpost, double* logprior, double* loglike,
                     int32_t* weight, int32_t* prior_rej, int32_t* burn_left, int64_t* n_accept,
                     int32_t* stuck)
{
    int any_normal = 0;
    for (int i = 0; i < d; ++i) any_normal |= inv[i] != 0.0;
    const int carry_p = K == 1 && any_normal;
    double* U = (double*)malloc(sizeof(double) * (size_t)K * d);
    double* Wd = (double*)malloc(sizeof(double) * (size_t)d);
    double* t = (double*)malloc(sizeof(double) * (size_t)d);
    double* yt = (double*)malloc(sizeof(double) * (size_t)K * d);
    int64_t total = 0;
    for (int s = 0; s < n_steps; ++s) {
        const uint64_t step = step0 + (uint64_t)s;
        const uint64_t cyc = step / (uint64_t)d;
        const int col = (int)(step % (uint64_t)d);
        for (int w = 0; w < W; ++w) {
            const int g = w / gs;
            const double* v = V + (((size_t)g * ncyc + (size_t)(cyc - cyc0)) * d + col) * d;
            /* directions (orc_whiten_directions, orc_direction_norms, orc_direction_prior) */
            for (int k = 0; k < K; ++k)
                for (int j = 0; j < d; ++j) {
                    double a = 0.0;
                    for (int i = 0; i <= j; ++i) a = fma(Linv[((size_t)k * d + j) * d + i], v[i], a);
                    U[k * d + j] = a;
                }
            const double uu = K > 0 ? four_chain_squares(U, d) : 0.0;
            double nn[4] = {0.0, 0.0, 0.0, 0.0}, lw[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i = 0; i < d; ++i) {
                Wd[i] = (v[i] * inv[i]) * inv[i];
                nn[i & 3] = fma(v[i], Wd[i], nn[i & 3]);
                if (inv[i] != 0.0) lw[i & 3] = fma(loc[i], Wd[i], lw[i & 3]);
            }
            const double nl0 = (nn[0] + nn[1]) + (nn[2] + nn[3]), nl1 = (lw[0] + lw[1]) + (lw[2] + lw[3]);
            double* xw = x + (size_t)w * d;
            double* yw = y + (size_t)w * K * d;
            if ((s == 0 && anchor) || step % refresh == 0) {   /* orc_whiten + orc_anchor_loglike */
                for (int k = 0; k < K; ++k)
                    for (int j = 0; j < d; ++j) {
                        double a = 0.0;
                        for (int i = 0; i <= j; ++i)
                            a = fma(Linv[((size_t)k * d + j) * d + i], xw[i] - mean[k * d + i], a);
                        yw[k * d + j] = a;
                    }
                if (K == 1) {
                    loglike[w] = -0.5 * (cnorm[0] + four_chain_squares(yw, d));
                    if (carry_p) {
                        double sc[4] = {0.0, 0.0, 0.0, 0.0};
                        for (int i = 0; i < d; ++i)
                            if (inv[i] != 0.0) {
                                const double q = (xw[i] - loc[i]) * inv[i];
                                sc[i & 3] = sc[i & 3] + fma(-0.5 * q, q, mls[i]);
                            }
                        logprior[w] = uniform_logp + ((sc[0] + sc[1]) + (sc[2] + sc[3]));
                    }
                    logpost[w] = logprior[w] + loglike[w];
                }
            }
            double r, Ea;
            if (K == 0) step_variates(seed, walker0 + (uint32_t)w, step, &r, &Ea);
            else orc_pair_variates(seed, walker0 + (uint32_t)w, step, &r, &Ea);
            /* step_core_inc */
            int inb = 1;
            for (int i = 0; i < d; ++i) {
                t[i] = fma(r, v[i], xw[i]);
                inb &= (t[i] <= hi[i]) & (t[i] >= lo[i]);
            }
            double lp = -INFINITY, ll = -INFINITY, lt = -INFINITY;
            if (inb) {
                double sc[4] = {0.0, 0.0, 0.0, 0.0};
                if (carry_p) {
                    for (int i = 0; i < d; ++i) sc[i & 3] = fma(xw[i], Wd[i], sc[i & 3]);
                    const double xwv = ((sc[0] + sc[1]) + (sc[2] + sc[3])) - nl1;
                    lp = fma(-0.5 * r, fma(r, nl0, xwv + xwv), logprior[w]);
                } else if (K == 0) {   /* eval_point: the division by the scale; one chain at d <= 32 */
                    for (int i = 0; i < d; ++i)
                        if (inv[i] != 0.0) {
                            const double q = (t[i] - loc[i]) / scale[i];
                            const int c = d > 32 ? (i & 3) : 0;
                            sc[c] = sc[c] + fma(-0.5 * q, q, mls[i]);
                        }
                    lp = uniform_logp + ((sc[0] + sc[1]) + (sc[2] + sc[3]));
                } else {
                    for (int i = 0; i < d; ++i)
                        if (inv[i] != 0.0) {
                            const double q = (t[i] - loc[i]) * inv[i];
                            sc[i & 3] = sc[i & 3] + fma(-0.5 * q, q, mls[i]);
                        }
                    lp = uniform_logp + ((sc[0] + sc[1]) + (sc[2] + sc[3]));
                }
                for (int k = 0; k < K; ++k)
                    for (int i = 0; i < d; ++i) yt[k * d + i] = fma(r, U[k * d + i], yw[k * d + i]);
                if (K == 0) {
                    ll = 0.0;
                } else if (K == 1) {
                    double q[4] = {0.0, 0.0, 0.0, 0.0};
                    for (int i = 0; i < d; ++i) q[i & 3] = fma(yw[i], U[i], q[i & 3]);
                    const double yu = (q[0] + q[1]) + (q[2] + q[3]);
                    ll = fma(-0.5 * r, fma(r, uu, yu + yu), loglike[w]);
                } else {
                    double a[4], amax = -INFINITY, S = 0.0;
                    for (int k = 0; k < K; ++k) {
                        a[k] = -0.5 * (cnorm[k] + four_chain_squares(yt + k * d, d));
                        if (a[k] > amax) amax = a[k];
                    }
                    for (int k = 0; k < K; ++k) S = fma(mweight[k], orc_dexp_tab(a[k] - amax), S);
                    ll = orc_dlog_tab(S) + amax;
                }
                lt = lp + ll;
            }
            int accept;
            if (!inb || lt == -INFINITY) accept = 0;
            else if (lt > logpost[w]) accept = 1;
            else accept = Ea > (logpost[w] - lt) / temperature;
            /* commit */
            if (accept) {
                if (burn_left[w] > 0) burn_left[w] -= 1;
                for (int i = 0; i < K * d; ++i) yw[i] = yt[i];
                for (int i = 0; i < d; ++i) xw[i] = t[i];
                logprior[w] = lp; loglike[w] = ll; logpost[w] = lt;
                weight[w] = 1; prior_rej[w] = 0; n_accept[w] += 1;
                total += 1;
            } else {
                weight[w] += 1;
                if (!inb) prior_rej[w] += 1;
                const double max_now = max_tries * (burn_left[w] > 0 ? 10.0 : 1.0);
                if ((double)(weight[w] - prior_rej[w]) > max_now && !*stuck) *stuck = 1 + (int32_t)(walker0 + (uint32_t)w);
            }
        }
    }
    free(U); free(Wd); free(t); free(yt);
    return total;
}
