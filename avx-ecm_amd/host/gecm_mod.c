/* gecm_mod.c — the device-free part of the host library (gecm_mod.h): the constants of one number, the curve
 * construction, failure records, the factor report and the position layout of a multi-modulus batch.  Mirrors the
 * reference's
 *   Montgomery constants        main.c:597-640
 *   NWORDS/MAXBITS rule         main.c:465-483
 *   build_one_curve             ecm.c:1548-1803
 *   check_factor                ecm.c:1319-1388, 2542-2557
 */
#include "gecm_mod.h"
#include "../../include/gecm.h"
#include "../csrc/gecm_rowk.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

__thread char gecm_mod_err[512];
void gecm_mod_set_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(gecm_mod_err, sizeof gecm_mod_err, fmt, ap);
    va_end(ap);
}

/* K' for the lazy subtraction (csrc/gecm_field.hpp): K = 2^j * mod in [R/32, R/16), written with every
 * limb in [2^28-1, 2^29): +2^28 at limb 0, +2^28-1 in the middle, -1 at the top. */
int gecm_mod_make_kp(uint32_t *kp, const mpl_t *mod, int nl)
{
    mpl_t K;
    uint32_t *kl = (uint32_t *)calloc((size_t)nl, sizeof(uint32_t));
    if (!kl) return -1;
    mpl_shl(&K, mod, (unsigned)(LIMB_BITS * nl - 4 - mpl_bits(mod)));
    mpl_to_limbs32(kl, 1, nl, LIMB_BITS, &K);
    for (int i = 0; i < nl; i++) {
        if (i == 0) kp[i] = kl[i] + (1u << LIMB_BITS);
        else if (i < nl - 1) kp[i] = kl[i] + (1u << LIMB_BITS) - 1;
        else kp[i] = kl[i] - 1;
    }
    free(kl);
    return 0;
}

void gecm_mod_pow2(mpl_t *r, unsigned e, const mpl_t *m)
{
    mpl_t t;
    mpl_set_u64(&t, 1);
    mpl_shl(&t, &t, e);
    mpl_mod(r, &t, m);
}

int gecm_mod_setup(gecm_mod *m, const char *who, const char *n_str, int digitbits, int nl, int (*pick_nl)(int nbits))
{
    if (mpl_set_str(&m->N, n_str) || !mpl_is_odd(&m->N) || mpl_cmp_u64(&m->N, 3) < 0) {
        gecm_mod_set_err("%s: N must be an odd integer >= 3 (decimal or 0x-hex)", who);
        return GECM_ERR_ARG;
    }
    m->digitbits = digitbits;
    m->nbits = mpl_bits(&m->N);
    /* main.c:465-483: MAXBITS = smallest multiple of 208 (128) strictly greater than bitlen */
    int step = digitbits == 52 ? 208 : 128;
    m->maxbits = step;
    while (m->maxbits <= m->nbits) m->maxbits += step;
    m->nwords = m->maxbits / digitbits;
    m->nl = nl ? nl : pick_nl(m->nbits);
    if (!pick_nl(m->nbits) || m->maxbits + 64 > MPL_MAXL * 16) {
        gecm_mod_set_err("%s: N of %d bits is larger than this build supports", who, m->nbits);
        return GECM_ERR_ARG;
    }
    nl = m->nl;
    unsigned rint_bits = (unsigned)(LIMB_BITS * nl), rref_bits = (unsigned)m->maxbits;
    mpl_t t, inv;
    gecm_mod_pow2(&m->rref_mod_n, rref_bits, &m->N);
    gecm_mod_pow2(&m->rint_mod_n, rint_bits, &m->N);
    mpl_invmod(&inv, &m->rref_mod_n, &m->N);
    mpl_mulmod(&m->ref_to_int, &m->rint_mod_n, &inv, &m->N);
    mpl_invmod(&inv, &m->rint_mod_n, &m->N);
    mpl_mulmod(&m->int_to_ref, &m->rref_mod_n, &inv, &m->N);
    /* rho = -N^-1 mod 2^digitbits (main.c:627-628, 636-640) and mod 2^28 */
    mpl_t two64;
    mpl_set_u64(&two64, 1);
    mpl_shl(&two64, &two64, 64);
    mpl_invmod(&inv, &m->N, &two64);
    mpl_sub(&t, &two64, &inv);
    uint64_t nhat = mpl_get_u64(&t);
    m->rho_ref = digitbits == 52 ? (nhat & 0xfffffffffffffull) : (nhat & 0xffffffffull);
    m->rho28 = (uint32_t)(nhat & ((1u << LIMB_BITS) - 1));
    m->n28 = (uint32_t *)calloc((size_t)nl * 7, sizeof(uint32_t));
    if (!m->n28) return GECM_ERR_NOMEM;
    m->kp28 = m->n28 + nl;
    m->one28 = m->kp28 + nl;
    m->fix28 = m->one28 + nl;
    m->r3_28 = m->fix28 + nl;
    m->finv28 = m->r3_28 + nl;
    mpl_to_limbs32(m->n28, 1, nl, LIMB_BITS, &m->N);
    mpl_to_limbs32(m->one28, 1, nl, LIMB_BITS, &m->rint_mod_n);
    if (gecm_mod_make_kp(m->kp28, &m->N, nl)) { gecm_mod_free(m); return GECM_ERR_NOMEM; }
    /* fix = Rint^2 / Rref mod N = Rint * ref_to_int */
    mpl_mulmod(&t, &m->rint_mod_n, &m->ref_to_int, &m->N);
    mpl_to_limbs32(m->fix28, 1, nl, LIMB_BITS, &t);
    /* R^3 mod N for the device inversion (csrc/gecm_stage2.hpp: fe_inv_mont) */
    mpl_mulmod(&t, &m->rint_mod_n, &m->rint_mod_n, &m->N);
    mpl_mulmod(&t, &t, &m->rint_mod_n, &m->N);
    mpl_to_limbs32(m->r3_28, 1, nl, LIMB_BITS, &t);
    /* the device inverts x Rref, read as (x Rref/Rint) Rint, to x^-1 Rint^2/Rref: times Rref^2/Rint, Montgomery-wise, is
     * x^-1 Rref */
    mpl_mulmod(&t, &m->rref_mod_n, &m->int_to_ref, &m->N);
    mpl_to_limbs32(m->finv28, 1, nl, LIMB_BITS, &t);
    /* R^2 mod N: one Montgomery multiply by it takes a plain residue x to x R (csrc/gecm_kernels.hip: k_to_mont) */
    mpl_mulmod(&t, &m->rint_mod_n, &m->rint_mod_n, &m->N);
    mpl_to_limbs32(m->finv28 + nl, 1, nl, LIMB_BITS, &t);
    /* batches of 28 division steps after which the device inversion has converged for a modulus of nbits bits:
     * the bound of the "half-delta" variant, floor((45907 bits + 26313) / 19929), +1, rounded up to whole batches */
    m->inv_iters = (uint32_t)((((45907ull * (unsigned)m->nbits + 26313ull) / 19929ull + 1) + 27) / 28);
    return GECM_OK;
}

void gecm_mod_free(gecm_mod *m)
{
    free(m->n28);                          /* kp28 .. finv28 and R^2 mod N are parts of it */
    m->n28 = NULL;
}

gecm_devmod gecm_mod_devmod(const gecm_mod *m)
{
    const gecm_devmod d = {m->n28, m->kp28, m->one28, m->finv28 + m->nl, m->r3_28, m->rho28, m->inv_iters};
    return d;
}

/* Suyama curve for one sigma up to (but not including) the two modular inversions
 * (ecm.c:1587-1641, 1717-1722): outputs x3 = u^3 mod n, z3 = v^3 mod n, num = (v-u)^3 (3u+v) mod n,
 * den = 16 u^3 v mod n. */
static void suyama_pre(const mpl_t *n, uint64_t sigma, mpl_t *x3, mpl_t *z3, mpl_t *num, mpl_t *den)
{
    mpl_t u, v, t1, t2, t3, t4;
    mpl_set_u64(&v, sigma);
    mpl_shl(&v, &v, 2);                 /* v = 4 sigma            ecm.c:1588-1589 */
    mpl_set_u64(&u, sigma);
    mpl_mul(&u, &u, &u);
    mpl_set_u64(&t1, 5);
    mpl_sub(&u, &u, &t1);               /* u = sigma^2 - 5        ecm.c:1596-1598 */
    mpl_mul(&t1, &u, &u);
    mpl_mul(&t1, &t1, &u);
    mpl_mod(x3, &t1, n);                /* x = u^3                ecm.c:1601-1603 */
    mpl_mul(&t1, &v, &v);
    mpl_mul(&t1, &t1, &v);
    mpl_mod(z3, &t1, n);                /* z = v^3                ecm.c:1607-1609 */
    /* (v - u) mod n                                               ecm.c:1615-1623 */
    mpl_t um, vm;
    mpl_mod(&um, &u, n);
    mpl_mod(&vm, &v, n);
    mpl_submod(&t1, &vm, &um, n);
    mpl_mulmod(&t2, &t1, &t1, n);
    mpl_mulmod(&t4, &t2, &t1, n);       /* (v-u)^3                ecm.c:1626-1629 */
    mpl_mul_u64(&t3, &u, 3);
    mpl_add(&t3, &t3, &v);
    mpl_mod(&t3, &t3, n);               /* 3u + v                 ecm.c:1632-1634 */
    mpl_mulmod(num, &t3, &t4, n);       /* a = (v-u)^3 (3u+v)     ecm.c:1637-1638 */
    mpl_mul_u64(&t2, x3, 16);
    mpl_mul(&t2, &t2, &v);
    mpl_mod(den, &t2, n);               /* 16 u^3 v               ecm.c:1718-1720 */
}

/* ---- GMP-ECM's PARAM 1 and PARAM 3 ---- */
int gecm_mod_param_sigma_ok(int param, uint64_t sigma)
{
    return sigma >= 1 && (param == GECM_PARAM_BATCH_SQUARE || (param == GECM_PARAM_BATCH_32 && sigma >> 32 == 0));
}

void gecm_mod_param_unit(mpl_t *unit, int param, const mpl_t *N)
{
    mpl_t t;
    gecm_mod_pow2(&t, param == GECM_PARAM_BATCH_SQUARE ? 64 : 32, N);
    mpl_invmod(unit, &t, N);                            /* N is odd: a power of two has an inverse */
}

void gecm_mod_param_d(mpl_t *d, int param, uint64_t sigma, const mpl_t *unit, const mpl_t *N)
{
    mpl_t s;
    mpl_set_u64(&s, sigma);
    if (param == GECM_PARAM_BATCH_SQUARE) mpl_mul(&s, &s, &s);
    mpl_mod(&s, &s, N);
    mpl_mulmod(d, &s, unit, N);
}

int gecm_param_s(int param, uint64_t sigma, const char *n_str, char *hex, size_t hexlen)
{
    mpl_t N, unit, d;
    if (param != GECM_PARAM_BATCH_SQUARE && param != GECM_PARAM_BATCH_32) {
        gecm_mod_set_err("gecm_param_s: PARAM %d: s comes from sigma alone for PARAM 1 and 3 only (PARAM 0 needs the "
                         "inversion rule of a build, PARAM 2 a point multiplication on another curve)", param);
        return GECM_ERR_ARG;
    }
    if (!gecm_mod_param_sigma_ok(param, sigma)) {
        gecm_mod_set_err("gecm_param_s: SIGMA = %llu is outside [1, 2^%d), the range of PARAM %d", (unsigned long long)sigma,
                         param == GECM_PARAM_BATCH_SQUARE ? 64 : 32, param);
        return GECM_ERR_ARG;
    }
    if (!n_str || !hex || mpl_set_str(&N, n_str) || !mpl_is_odd(&N) || mpl_cmp_u64(&N, 3) < 0) {
        gecm_mod_set_err("gecm_param_s: N must be an odd integer >= 3 (decimal or 0x-hex), and hex a buffer");
        return GECM_ERR_ARG;
    }
    gecm_mod_param_unit(&unit, param, &N);
    gecm_mod_param_d(&d, param, sigma, &unit, &N);
    static __thread char tmp[MPL_MAXL * 10 + 2];
    const int n = mpl_get_hex(tmp, &d);
    if (n < 0 || (size_t)n >= hexlen) { gecm_mod_set_err("gecm_param_s: buffer too small"); return GECM_ERR_ARG; }
    memcpy(hex, tmp, (size_t)n + 1);
    return n;
}

/* One worker's slice [lo, hi): the whole Suyama construction for those curves.
 * The two inversions per curve, mpz_invert(16u^3v) ecm.c:1745 and mpz_invert(v^3) ecm.c:1759, share the
 * modulus, so each slice does Montgomery's simultaneous inversion: one extended Euclid per slice
 * instead of two per curve.  Inverses mod N are unique, so the values are the ones GMP returns. */
int gecm_mod_build_slice(void *build, size_t lo, size_t hi)
{
    const gecm_mod_build *j = (const gecm_mod_build *)build;
    const gecm_mod *c = j->m;
    const size_t cnt = hi - lo, m = 2 * cnt, batch = j->batch;
    const int nl = c->nl;
    int anybad = 0;
    if (cnt == 0) return 0;
    mpl_t *x3 = (mpl_t *)malloc(cnt * sizeof(mpl_t) * 2);
    mpl_t *dens = (mpl_t *)malloc(m * sizeof(mpl_t));
    mpl_t *pref = (mpl_t *)malloc(m * sizeof(mpl_t));
    if (!x3 || !dens || !pref) { free(x3); free(dens); free(pref); return GECM_ERR_NOMEM; }
    mpl_t *num = x3 + cnt;
    /* a PARAM 1 or 3 curve of a mixed batch (j->param) has no inversion: it stands in the shared one with the
     * denominators 1, 1 — the Suyama curves of the slice get the inverses they get without it, inverses being unique,
     * and the same failure records — and is written by its own formula below */
    const uint8_t *prm = j->param ? j->param + lo : NULL;
    mpl_t unit[2];
    int have_unit[2] = {0, 0};
    for (size_t i = 0; i < cnt; i++) {
        if (prm && prm[i]) {
            mpl_set_u64(&x3[i], 0);
            mpl_set_u64(&num[i], 0);
            mpl_set_u64(&dens[2 * i], 1);
            mpl_set_u64(&dens[2 * i + 1], 1);
        } else
            suyama_pre(&c->N, j->sigma[lo + i], &x3[i], &dens[2 * i + 1], &num[i], &dens[2 * i]);
    }
    int batch_ok = 1;
    pref[0] = dens[0];
    for (size_t i = 1; i < m; i++) mpl_mulmod(&pref[i], &pref[i - 1], &dens[i], &c->N);
    mpl_t inv, t;
    if (!mpl_invmod(&inv, &pref[m - 1], &c->N)) batch_ok = 0;
    mpl_t *invs = pref;   /* overwritten back to front */
    if (batch_ok) {
        for (size_t i = m - 1; i > 0; i--) {
            mpl_mulmod(&t, &inv, &pref[i - 1], &c->N);      /* dens[i]^-1 */
            mpl_mulmod(&inv, &inv, &dens[i], &c->N);
            invs[i] = t;
        }
        invs[0] = inv;
    } else {
        /* Some denominator shares a factor with N.  The reference ignores mpz_invert's return
         * value (ecm.c:1745, 1759); GMP leaves the destination untouched on failure, so the
         * reference goes on with the STALE operand: t2 = 16*u^3 (ecm.c:1718) in place of
         * (16u^3v)^-1 and t1 = (v-u)^3(3u+v) (ecm.c:1637) in place of (v^3)^-1.  Reproduced here so
         * that such curves still give the reference's residues bit for bit; the lane is also
         * flagged (a non-invertible denominator means gcd(denominator, N) is a factor). */
        for (size_t i = 0; i < m; i++)
            if (!mpl_invmod(&invs[i], &dens[i], &c->N)) {
                j->bad[j->off + lo + i / 2] = 1;
                anybad = 1;
                if ((i & 1) == 0) { mpl_mul_u64(&t, &x3[i / 2], 16); mpl_mod(&invs[i], &t, &c->N); }
                else invs[i] = num[i / 2];
            }
    }
    for (size_t i = 0; i < cnt; i++) {
        mpl_t A, X, Xm, Sm;
        const size_t k = j->off + lo + i;
        if (prm && prm[i]) {                                   /* s = d, P = (2 : 1) */
            const int w = prm[i] == GECM_PARAM_BATCH_SQUARE ? 0 : 1;
            if (!have_unit[w]) gecm_mod_param_unit(&unit[w], prm[i], &c->N);
            have_unit[w] = 1;
            gecm_mod_param_d(&A, prm[i], j->sigma[lo + i], &unit[w], &c->N);
            mpl_set_u64(&X, 2);
            mpl_mod(&X, &X, &c->N);
        } else {
            mpl_mulmod(&A, &num[i], &invs[2 * i], &c->N);      /* b = a / 16u^3v   ecm.c:1752-1753 */
            mpl_mulmod(&X, &x3[i], &invs[2 * i + 1], &c->N);   /* X = u^3 / v^3, Z = 1  ecm.c:1759-1761 */
        }
        /* into Montgomery form (ecm.c:1763-1772), internal radix */
        mpl_mulmod(&Xm, &X, &c->rint_mod_n, &c->N);
        mpl_mulmod(&Sm, &A, &c->rint_mod_n, &c->N);
        mpl_to_limbs32(j->hX + k, batch, nl, LIMB_BITS, &Xm);
        mpl_to_limbs32(j->hZ + k, batch, nl, LIMB_BITS, &c->rint_mod_n);
        mpl_to_limbs32(j->hS + k, batch, nl, LIMB_BITS, &Sm);
    }
    free(x3); free(dens); free(pref);
    return anybad;
}

/* The reference overwrites its accumulator with gcd(product of the batch, N) every time a batch inversion fails
 * (ecm.c:1925-1939): what its scan finds in the end is the gcd of the LAST failing batch (times later cross products).
 * Plane 0 holds that gcd for the single-chain inversions — after gecm_stage2_pair the last chunk of the range, cut to
 * be exactly the reference's last batch — and decides when it holds one.  Otherwise the sub-sequences' planes stand
 * for one batch inverted in K pieces: the gcd of N with the PRODUCT of their records is the gcd of the whole batch's
 * product (for a product that covers N that is N itself — "no factor", which is what the reference finds then too:
 * its batch product is 0 modulo N).  Every record is passed through gcd(., N) first: what comes out divides N. */
void gecm_mod_fail_record(const gecm_mod *m, const uint32_t *hfail, uint32_t planes, size_t batch, size_t k, mpl_t *g)
{
    const size_t plane = batch * (size_t)m->nl;
    mpl_t t, prod, gp;
    mpl_from_limbs32(&t, hfail + k, batch, m->nl, LIMB_BITS);
    if (!mpl_is_zero(&t)) { mpl_gcd(g, &t, &m->N); return; }
    mpl_set_u64(g, 0);
    if (planes <= 1) return;
    mpl_set_u64(&prod, 0);
    for (uint32_t p = 1; p < planes; p++) {
        mpl_from_limbs32(&t, hfail + p * plane + k, batch, m->nl, LIMB_BITS);
        if (mpl_is_zero(&t)) continue;
        mpl_gcd(&gp, &t, &m->N);
        if (mpl_is_zero(&prod)) prod = gp;
        else mpl_mulmod(&prod, &prod, &gp, &m->N);
        if (mpl_is_zero(&prod)) { prod = m->N; break; }       /* the product covers N: gcd = N, "no factor" */
    }
    if (!mpl_is_zero(&prod)) mpl_gcd(g, &prod, &m->N);
}

int gecm_mod_factor(const gecm_mod *m, mpl_t *g, const char *who, char *dec, size_t declen, int *is_prp)
{
    if (!to_report(m, g)) return 0;
    static __thread char tmp[MPL_MAXL * 10 + 16];
    int n = mpl_get_dec(tmp, g);
    if (dec && declen) {
        if ((size_t)n >= declen) { gecm_mod_set_err("%s: buffer too small", who); return GECM_ERR_ARG; }
        memcpy(dec, tmp, (size_t)n + 1);
    }
    if (is_prp) *is_prp = mpl_probab_prime(g, 3);   /* ecm.c:1346 */
    return 1;
}

/* Constants of the row kernels (csrc/gecm_row.hpp) for one number, at the shape of a context of nl limbs: L limbs in
 * use (nl + 1), R' = 2^(28 L).  Both kernels share the entry factor R'^2/R mod N, which turns the buffers' x*R into
 * x*R', and the exit multiply by R mod N (modulo N itself), which turns it back, with K' of N.
 *   w (GECM_ROW_KINDS x GECM_ROW_WORDS, or NULL): the 32-lanes-per-curve stage-1 kernel, which works modulo N' = m*N, the
 *     multiple of N that is -1 modulo 2^28 (the Montgomery digit is then the low limb itself), with R' >= 32 N'.
 *   u (GECM_UROW_SET words, or NULL): the 16-lanes-per-residue method kernel, which works modulo
 *     N'' = (m + t 2^28) N with the smallest t >= 0 that makes N'' >= 2^(28 (L - 1) + GECM_UROW_TOP_MIN_BITS): still -1
 *     modulo 2^28, below 2^(28 L - 5) (1 + 2^-3), and with a top limb that tells a value's quotient by N''; with it the
 *     float reciprocal of N'' / 2^(28 (L - 1)), 2 R' mod N'' nearest zero in balanced limbs, and N's own rho.
 * 1 if the constants asked for are made, 0 if this N has none (m->nl is not nl, or a bound does not hold). */
int gecm_mod_row_consts(const gecm_mod *mod, int nl, int L, uint32_t *w, uint32_t *u)
{
    if (mod->nl != nl || L != nl + 1 || L < 3 || L > GECM_ROW_WORDS) return 0;
    mpl_t two28, inv, m, np, cin;
    mpl_set_u64(&two28, 1u << LIMB_BITS);
    if (!mpl_invmod(&inv, &mod->N, &two28)) return 0;
    mpl_sub(&m, &two28, &inv);                        /* m = -N^-1 mod 2^28, in [1, 2^28) */
    mpl_mul(&np, &m, &mod->N);
    gecm_mod_pow2(&cin, (unsigned)(2 * LIMB_BITS * L - LIMB_BITS * nl), &mod->N);
    if (w) {
        memset(w, 0, GECM_ROW_KINDS * GECM_ROW_WORDS * sizeof(uint32_t));
        if (mpl_bits(&np) + 5 > LIMB_BITS * L) return 0;
        mpl_to_limbs32(w + 0 * GECM_ROW_WORDS, 1, L, LIMB_BITS, &np);
        if (w[0] != (1u << LIMB_BITS) - 1u) return 0;
        memcpy(w + 1 * GECM_ROW_WORDS, mod->n28, (size_t)nl * sizeof(uint32_t));
        mpl_to_limbs32(w + 2 * GECM_ROW_WORDS, 1, nl, LIMB_BITS, &cin);
        memcpy(w + 3 * GECM_ROW_WORDS, mod->one28, (size_t)nl * sizeof(uint32_t));
        memcpy(w + 4 * GECM_ROW_WORDS, mod->kp28, (size_t)nl * sizeof(uint32_t));
    }
    if (u) {
        memset(u, 0, GECM_UROW_SET * sizeof(uint32_t));
        mpl_t one, low, step, t, M, lim, v;
        mpl_set_u64(&one, 1);
        mpl_shl(&low, &one, (unsigned)(LIMB_BITS * (L - 1) + GECM_UROW_TOP_MIN_BITS));
        M = np;
        if (mpl_cmp(&M, &low) < 0) {                  /* t = ceil((low - m N) / (2^28 N)) */
            mpl_shl(&step, &mod->N, LIMB_BITS);
            mpl_sub(&t, &low, &M);
            mpl_add(&t, &t, &step);
            mpl_sub(&t, &t, &one);
            mpl_divrem(&v, NULL, &t, &step);
            mpl_mul(&t, &v, &step);
            mpl_add(&M, &M, &t);
        }
        mpl_shl(&lim, &one, (unsigned)(LIMB_BITS * L - 5));
        mpl_shr(&v, &lim, 3);
        mpl_add(&lim, &lim, &v);
        if (mpl_cmp(&M, &low) < 0 || mpl_cmp(&M, &lim) >= 0) return 0;
        uint32_t *um = u + 0 * GECM_ROW_WORDS;
        mpl_to_limbs32(um, 1, L, LIMB_BITS, &M);
        if (um[0] != (1u << LIMB_BITS) - 1u) return 0;
        memcpy(u + 1 * GECM_ROW_WORDS, mod->n28, (size_t)nl * sizeof(uint32_t));
        mpl_to_limbs32(u + 2 * GECM_ROW_WORDS, 1, nl, LIMB_BITS, &cin);
        memcpy(u + 3 * GECM_ROW_WORDS, mod->one28, (size_t)nl * sizeof(uint32_t));
        memcpy(u + 4 * GECM_ROW_WORDS, mod->kp28, (size_t)nl * sizeof(uint32_t));
        /* 2 R' mod N'', or that minus N'' if it is nearer zero, in balanced limbs: (-2^27, 2^27] below the top one */
        gecm_mod_pow2(&v, (unsigned)(LIMB_BITS * L + 1), &M);
        mpl_shl(&t, &v, 1);
        const int neg = mpl_cmp(&t, &M) > 0;
        if (neg) { mpl_sub(&t, &M, &v); v = t; }
        uint32_t *two = u + 5 * GECM_ROW_WORDS;
        mpl_to_limbs32(two, 1, L, LIMB_BITS, &v);
        int32_t carry = 0;
        for (int i = 0; i < L; i++) {
            int32_t x = (int32_t)two[i] + carry;
            carry = 0;
            if (i < L - 1 && x > (1 << (LIMB_BITS - 1))) { x -= 1 << LIMB_BITS; carry = 1; }
            two[i] = (uint32_t)(neg ? -x : x);
        }
        /* the reciprocal the reduction multiplies a top limb by: of N'' / 2^(28 (L - 1)) from its three top limbs */
        const double scaled = (double)um[L - 1] + (double)um[L - 2] / 268435456.0 + (double)um[L - 3] / 72057594037927936.0;
        const float rec = (float)(1.0 / scaled);
        memcpy(u + 6 * GECM_ROW_WORDS, &rec, sizeof rec);
        u[6 * GECM_ROW_WORDS + 1] = mod->rho28;
    }
    return 1;
}

/* ---- wide contexts ---- */
int gecm_wide_max_bits(void) { return GECM_WIDE_MAX_BITS; }

int gecm_mod_wide_nl(int nbits)
{
    static const int wide_nl[] = {40, 43, 47, 0};     /* rows 41, 44, 48 of csrc/gecm_rowk.h: GECM_ROW_WIDE_SHAPES */
    if (nbits > GECM_WIDE_MAX_BITS) return 0;
    for (const int *p = wide_nl; *p; p++)
        if (LIMB_BITS * *p >= nbits + 5) return *p;
    return 0;
}

void gecm_mod_raw_value(mpl_t *r, const uint32_t *limbs, size_t stride, int count)
{
    /* the parts below and from 2^28 of every limb are two numbers in disjoint 28-bit fields (the upper parts have 4 bits) */
    uint32_t lo[MPL_MAXL], hi[MPL_MAXL];
    mpl_t a, b;
    if (count > MPL_MAXL) count = MPL_MAXL;
    for (int i = 0; i < count; i++) {
        const uint32_t w = limbs[(size_t)i * stride];
        lo[i] = w & ((1u << LIMB_BITS) - 1);
        hi[i] = w >> LIMB_BITS;
    }
    mpl_from_limbs32(&a, lo, 1, count, LIMB_BITS);
    mpl_from_limbs32(&b, hi, 1, count, LIMB_BITS);
    mpl_shl(&b, &b, LIMB_BITS);
    mpl_add(r, &a, &b);
}

int gecm_mod_raw_slice(void *job, size_t lo, size_t hi)
{
    const gecm_mod_wide_job *j = (const gecm_mod_wide_job *)job;
    const gecm_mod *m = j->m;
    const uint32_t *src[2] = {j->rawX, j->rawZ};
    uint32_t *dst[2] = {j->hx, j->hz};
    for (size_t k = lo; k < hi; k++)
        for (int w = 0; w < 2; w++) {
            mpl_t v;
            gecm_mod_raw_value(&v, src[w] + k, j->batch, m->nl);     /* t + K', t = x R mod N lazily */
            mpl_mod(&v, &v, &m->N);                                  /* canonical Montgomery form */
            mpl_mulmod(&v, &v, &j->rinv, &m->N);                     /* plain */
            mpl_to_limbs32(dst[w] + k, j->batch, m->nl, LIMB_BITS, &v);
        }
    return 0;
}

int gecm_mod_gcd_slice(void *job, size_t lo, size_t hi)
{
    const gecm_mod_wide_job *j = (const gecm_mod_wide_job *)job;
    const gecm_mod *m = j->m;
    for (size_t k = lo; k < hi; k++) {
        mpl_t z, g;
        mpl_from_limbs32(&z, j->hz + k, j->batch, m->nl, LIMB_BITS);
        mpl_gcd(&g, &z, &m->N);                                      /* z = 0: g = N, no factor (ecm.c:2542-2557) */
        mpl_to_limbs32(j->hg + k, j->batch, m->nl, LIMB_BITS, &g);
        j->flags[k] = mpl_cmp_u64(&g, 1) > 0 && mpl_cmp(&g, &m->N) != 0;
    }
    return 0;
}

/* ---- the position layout of a multi-modulus batch ---- */
size_t gecm_multi_positions(const size_t *counts, size_t n, int packing)
{
    size_t total = 0;
    for (size_t g = 0; counts && g < n; g++) total += packing == GECM_PACK_LANE ? counts[g] : (counts[g] + 63) / 64 * 64;
    return (total + 63) / 64 * 64;
}

int gecm_layout_make(gecm_layout *l, const uint32_t *modulus_index, size_t batch, size_t ngroups, int packing)
{
    const int lane = packing == GECM_PACK_LANE;
    memset(l, 0, sizeof *l);
    if (!modulus_index || batch == 0 || batch >= GECM_PAD || ngroups == 0) return GECM_ERR_ARG;
    int rc = GECM_ERR_NOMEM;
    l->slot = (uint32_t *)malloc(batch * sizeof(uint32_t));
    l->goff = (size_t *)calloc(ngroups, sizeof(size_t));
    l->cnt = (size_t *)calloc(ngroups, sizeof(size_t));
    if (!l->slot || !l->goff || !l->cnt) goto fail;
    rc = GECM_ERR_ARG;
    for (size_t i = 0; i < batch; i++) {
        if (modulus_index[i] >= ngroups) goto fail;
        l->cnt[modulus_index[i]]++;
    }
    l->nuser = batch;
    l->ngroups = ngroups;
    l->total = gecm_multi_positions(l->cnt, ngroups, packing);
    if (l->total >= GECM_PAD) goto fail;
    rc = GECM_ERR_NOMEM;
    l->pos_user = (uint32_t *)malloc(l->total * sizeof(uint32_t));
    l->pos_grp = (uint32_t *)calloc(l->total, sizeof(uint32_t));      /* lane packing: the tail stays on modulus 0 */
    /* wave packing: the modulus of every 64-curve block, which the kernels read there (lane packing: pos_grp) */
    if (!lane) l->blocks = (uint32_t *)malloc(l->total / 64 * sizeof(uint32_t));
    if (!l->pos_user || !l->pos_grp || (!lane && !l->blocks)) goto fail;
    memset(l->pos_user, 0xff, l->total * sizeof(uint32_t));          /* GECM_PAD until a curve takes the position */
    for (size_t g = 0, off = 0; g < ngroups; g++) {
        /* positions of one modulus: its curves, under wave packing with its own padding */
        const size_t span = lane ? l->cnt[g] : gecm_multi_positions(&l->cnt[g], 1, GECM_PACK_WAVE);
        l->goff[g] = off;
        for (size_t p = off; p < off + span; p++) {
            l->pos_grp[p] = (uint32_t)g;
            if (!lane) l->blocks[p / 64] = (uint32_t)g;
        }
        off += span;
    }
    memset(l->cnt, 0, ngroups * sizeof(size_t));
    for (size_t i = 0; i < batch; i++) {
        const uint32_t g = modulus_index[i];
        const size_t p = l->goff[g] + l->cnt[g]++;
        l->slot[i] = (uint32_t)p;
        l->pos_user[p] = (uint32_t)i;
    }
    return GECM_OK;
fail:
    gecm_layout_free(l);
    return rc;
}

void gecm_layout_free(gecm_layout *l)
{
    free(l->slot); free(l->pos_user); free(l->pos_grp); free(l->blocks); free(l->goff); free(l->cnt);
    memset(l, 0, sizeof *l);
}

/* the hash of the host sources this object was compiled from (Makefile: H_SHA); gecm_version() compares them */
#ifdef GECM_MANIFEST_FN
const char *GECM_MANIFEST_FN(void) { return GECM_MANIFEST; }
#endif
