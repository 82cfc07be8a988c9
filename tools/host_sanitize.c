/* tools/host_sanitize.c — the host-side logic of libgecm (everything that runs without a device) under
 * AddressSanitizer + UBSan.  Built and run by tools/host_sanitize.sh on the CPU; GPU sanitizers are not
 * available on the pool.  Exercises: expression evaluator and input preparation with random and
 * hostile strings, mpl arithmetic identities, the stage-1 tape compiler, the stage-2 plan and PAIR, the constants of
 * a modulus and the curve construction. */
#include "../avx-ecm_amd/host/calc_lite.h"
#include "../avx-ecm_amd/host/cunningham.h"
#include "../avx-ecm_amd/host/gecm_mod.h"
#include "../avx-ecm_amd/host/gecm_pair.h"
#include "../avx-ecm_amd/host/gecm_plan.h"
#include "../avx-ecm_amd/host/mpl.h"
#include "../include/gecm.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint64_t rng = 88172645463325252ull;
static uint64_t rnd(void) { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; }

static int need_nl(int nbits) { return (nbits + 5 + 27) / 28; }   /* R = 2^(28 nl) >= 32 N */

int main(void)
{
    static char ndec[2000], log[65536], buf[4096];
    gecm_input_info inf;
    /* 1. hostile and random expressions */
    const char *alphabet = "0123456789+-*/%^!#()<>, xfibluc";
    int ok = 0;
    for (int it = 0; it < 20000; it++) {
        int len = (int)(rnd() % 40);
        for (int i = 0; i < len; i++) buf[i] = alphabet[rnd() % strlen(alphabet)];
        buf[len] = 0;
        if (gecm_prepare_input(buf, it & 1 ? 52 : 32, ndec, sizeof ndec, &inf, log, sizeof log) == 0) ok++;
    }
    const char *fixed[] = {"2^4000", "2^4351-1", "fib(100000)", "100000!", "99999#", "1<<4000", "2^2^2^2^2", "((((((((1))))))))",
                           "modexp(2,1000000,2^1277-1)", "modinv(3,2^1000+1)", "sqrt(2^4000)", "gcd(2^600-1,2^900-1)",
                           "2^1155-1", "2^2047-1", "2^2047+1", "2^1024+1", "0x", "0xffffffffffffffffffffffffffffffff",
                           "3", "1", "", "2^2100+1"};
    for (size_t i = 0; i < sizeof fixed / sizeof *fixed; i++) {
        int rc = gecm_prepare_input(fixed[i], 52, ndec, sizeof ndec, &inf, log, sizeof log);
        printf("%-36s rc=%d form=%d k=%d bits=%d\n", fixed[i], rc, rc ? 0 : inf.form, rc ? 0 : inf.k, rc ? 0 : inf.nbits);
    }
    /* tiny output buffers must be refused, not overrun */
    char small[4], slog[8];
    gecm_prepare_input("2^210-1", 52, small, sizeof small, &inf, slog, sizeof slog);
    printf("random expressions accepted: %d of 20000\n", ok);

    /* 2. mpl identities on random operands */
    for (int it = 0; it < 3000; it++) {
        mpl_t a, b, m, q, r, t, u;
        int la = 1 + (int)(rnd() % 60), lb = 1 + (int)(rnd() % 60);
        a.n = la; b.n = lb;
        for (int i = 0; i < la; i++) a.d[i] = (uint32_t)rnd();
        for (int i = 0; i < lb; i++) b.d[i] = (uint32_t)rnd();
        if (!a.d[la - 1]) a.d[la - 1] = 1;
        if (!b.d[lb - 1]) b.d[lb - 1] = 1;
        mpl_divrem(&q, &r, &a, &b);
        mpl_mul(&t, &q, &b);
        mpl_add(&t, &t, &r);
        if (mpl_cmp(&t, &a) || mpl_cmp(&r, &b) >= 0) { printf("divrem identity failed\n"); return 1; }
        m = b; m.d[0] |= 1;
        if (mpl_cmp_u64(&m, 3) >= 0) {
            mpl_mod(&u, &a, &m);
            if (mpl_invmod(&t, &u, &m)) {
                mpl_mulmod(&t, &t, &u, &m);
                if (mpl_cmp_u64(&t, 1)) { printf("invmod identity failed\n"); return 1; }
            }
            mpl_gcd(&t, &a, &m);
            mpl_mod(&u, &m, &t);
            if (!mpl_is_zero(&u)) { printf("gcd does not divide\n"); return 1; }
        }
        mpl_get_dec(buf, &a);
        mpl_set_str(&t, buf);
        if (mpl_cmp(&t, &a)) { printf("decimal round trip failed\n"); return 1; }
    }
    /* 3. tape compiler */
    const uint64_t b1s[] = {2, 3, 4, 5, 100, 1000, 65537, 1000000};
    for (size_t i = 0; i < sizeof b1s / sizeof *b1s; i++) {
        gecm_tape_t t;
        memset(&t, 0, sizeof t);
        int rc = gecm_tape_build_stage1(&t, b1s[i]);
        printf("tape B1=%lu rc=%d len=%zu adds=%lu dups=%lu\n", (unsigned long)b1s[i], rc, t.len, (unsigned long)t.ptadds,
               (unsigned long)t.ptdups);
        gecm_tape_free(&t);
    }
    /* 4. stage-2 plan and PAIR for several wheels */
    const uint32_t Ds[] = {30, 210, 1155, 2310};
    for (size_t i = 0; i < sizeof Ds / sizeof *Ds; i++)
        for (uint32_t U = 2; U <= 16; U *= 2) {
            gecm_s2_plan p;
            if (gecm_s2_plan_init(&p, Ds[i], U)) { printf("plan %u/%u refused\n", Ds[i], U); continue; }
            gecm_pairmap pm;
            int rc = gecm_pair(&pm, 1000, 300000, Ds[i], U);
            printf("D=%u U=%u npb=%u pair rc=%d steps=%u pairs=%u nump=%u\n", Ds[i], U, p.npb, rc, rc ? 0 : pm.steps,
                   rc ? 0 : pm.pairs, rc ? 0 : pm.nump);
            if (!rc) gecm_pairmap_free(&pm);
            gecm_s2_plan_free(&p);
        }
    /* 5. the device tape of a range: real pair maps, then hostile ones (nothing but window shifts with a tall table —
     * the case that overran a fixed-size tape in round 1 —, random entries, a table too tall for the ring) */
    {
        const uint32_t chunk = 512, ring = 1024;
        for (uint32_t U = 2; U <= 256; U *= 2) {
            gecm_s2_plan p;
            if (gecm_s2_plan_init(&p, 210, U)) continue;
            gecm_pairmap pm;
            gecm_s2_tape t;
            uint32_t bad = 0;
            if (!gecm_pair(&pm, 1000, 200000, 210, U)) {
                int rc = gecm_s2_tape_build(&t, &p, pm.steps, pm.v, pm.u, pm.amin, chunk, ring, &bad);
                uint64_t gen = 0, pairs = 0;
                if (!rc) {
                    for (size_t i = 0; i < t.nwords; i += 2)
                        if (t.words[i] == GECM_S2_GEN) gen += t.words[i + 1] & 0x7fffffffu; else pairs++;
                    if (pairs != pm.pairs || pairs != t.paired) { printf("tape: pair count mismatch\n"); return 1; }
                    free(t.words);
                }
                printf("tape U=%u rc=%d steps=%u marks+pairs=%zu giant steps=%lu\n", U, rc, pm.steps, rc ? 0 : t.nwords / 2,
                       (unsigned long)gen);
                gecm_pairmap_free(&pm);
            }
            /* 5000 window shifts and nothing else */
            uint32_t *z = (uint32_t *)calloc(5000, sizeof(uint32_t));
            int rc = gecm_s2_tape_build(&t, &p, 5000, z, z, 7, chunk, ring, &bad);
            if (!rc) {
                uint64_t gen = 0;
                for (size_t i = 0; i < t.nwords; i += 2) gen += t.words[i + 1] & 0x7fffffffu;
                if (gen != 2ull * p.L + 2ull * U * 5000) { printf("tape: wrong number of giant steps\n"); return 1; }
                if (!(t.words[t.nwords - 1] & 0x80000000u)) { printf("tape: last chunk not flagged\n"); return 1; }
                free(t.words);
            }
            printf("tape U=%u all-shifts rc=%d\n", U, rc);
            /* random entries: refused with the index of the first bad one, never a crash */
            for (int it = 0; it < 200; it++) {
                uint32_t v[64], u[64];
                for (int i = 0; i < 64; i++) { v[i] = (uint32_t)(rnd() % 40); u[i] = (uint32_t)(rnd() % (p.umax + 50)); }
                rc = gecm_s2_tape_build(&t, &p, 64, v, u, (uint32_t)(rnd() % 8), chunk, ring, &bad);
                if (!rc) free(t.words);
            }
            free(z);
            gecm_s2_plan_free(&p);
        }
    }
    /* 6. gecm_mod: N's constants at every limb count of the build (n28 is N; K' is K = 2^j N in [R/32, R/16) with every
     * limb below the top one in [2^28 - 1, 2^29)), and the curve construction, last modulo 3*5*7*11*13, where denominators do not invert and build_slice goes on
     * with the reference's stale operands */
    {
        const int nls[] = {8, 10, 12, 14, 15, 17, 19, 21, 23, 26, 28, 30, 32, 34, 37, 8};
        const size_t cases = sizeof nls / sizeof *nls;
        uint64_t sig[300];
        for (int i = 0; i < 300; i++) sig[i] = 6 + (uint64_t)i;
        for (size_t q = 0; q < cases; q++) {
            const int nl = nls[q], last = q == cases - 1;
            gecm_mod m;
            mpl_t n, t, k;
            memset(&m, 0, sizeof m);
            n.n = nl;                                   /* 28 nl - 5 bits, odd */
            for (int i = 0; i < nl; i++) n.d[i] = (uint32_t)rnd();
            n.d[nl - 1] |= 0x80000000u;
            mpl_shr(&n, &n, (unsigned)(4 * nl + 5));
            n.d[0] |= 1;
            if (last) mpl_set_u64(&n, 15015);
            mpl_get_dec(ndec, &n);
            if (gecm_mod_setup(&m, "sanitize", ndec, 52, nl, need_nl)) { printf("mod_setup: %s\n", gecm_mod_err); return 1; }
            mpl_from_limbs32(&t, m.n28, 1, nl, LIMB_BITS);
            int good = !mpl_cmp(&t, &n);
            mpl_set_u64(&t, 0);
            for (int i = nl - 1; i >= 0; i--) {
                if (i < nl - 1) good &= m.kp28[i] >= (1u << LIMB_BITS) - 1 && m.kp28[i] < (2u << LIMB_BITS);
                mpl_shl(&t, &t, LIMB_BITS);
                mpl_add_u64(&t, &t, m.kp28[i]);
            }
            mpl_shl(&k, &n, (unsigned)(LIMB_BITS * nl - 4 - mpl_bits(&n)));
            good &= !mpl_cmp(&t, &k);
            if (!good) { printf("mod_setup: n28 or kp28 wrong at %d limbs\n", nl); return 1; }
            if (nl == 15 || last) {
                uint32_t *h = (uint32_t *)calloc((size_t)900 * nl, sizeof(uint32_t));
                uint8_t bad[300] = {0};
                gecm_mod_build b = {&m, sig, bad, 300, 0, h, h + 300 * nl, h + 600 * nl};
                int rc = h ? gecm_mod_build_slice(&b, 0, 300) : -1, nbad = 0;
                for (int i = 0; i < 300; i++) nbad += bad[i];
                printf("build_slice at %d limbs: rc=%d bad=%d\n", nl, rc, nbad);
                if (rc != (nbad > 0) || (last && !nbad)) { printf("build_slice: wrong bad flags\n"); return 1; }
                free(h);
            }
            gecm_mod_free(&m);
        }
    }
    size_t np;
    uint64_t *pr = gecm_primes_range(999999000ull, 1000001000ull, &np);
    printf("primes in [999999000, 1000001000): %zu\n", np);
    free(pr);
    printf("host sanitizer run complete\n");
    return 0;
}
