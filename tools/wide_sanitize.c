/* The host side of a wide context (host/gecm_mod.c) under AddressSanitizer + UBSan: CPU only, a program of
 * its own, the device-free host objects only.  tools/wide_sanitize.sh builds and runs it.  For a modulus at both ends of
 * every wide class: gecm_mod_setup with the wide limb rule, gecm_mod_row_consts at L = 41, 44, 48, and raw limbs ->
 * canonical -> plain -> gcd on lazy values built from known integers, in heap blocks of exactly the sizes the library is
 * told, so that a word read or written past an end is an error the sanitizer sees. */
#include "../include/gecm.h"
#include "../avx-ecm_amd/host/gecm_mod.h"
#include "../avx-ecm_amd/csrc/gecm_rowk.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

/* "0x" and the hex digits of an odd number of exactly `bits` bits: the digit `fill` throughout, or = 1 modulo 2^28 */
static void number(char *s, int bits, char fill, int low_one)
{
    const int digits = (bits + 3) / 4, topbits = bits - 4 * (digits - 1);
    strcpy(s, "0x");
    memset(s + 2, fill, (size_t)digits);
    s[2] = "137f"[topbits - 1];
    if (low_one) { memset(s + 2 + digits - 7, '0', 7); }      /* = 1 modulo 2^28 */
    s[2 + digits - 1] = low_one ? '1' : 'f';
    s[2 + digits] = 0;
}

/* x R + (K' as limbs) + j N written lazily: limbs below 2^28 + 16, the top limb what is left, at curve k of [nl][batch] */
static void lazy_limbs(uint32_t *plane, size_t batch, size_t k, const gecm_mod *m, const mpl_t *x, unsigned j)
{
    mpl_t v, t;
    uint32_t *canon = (uint32_t *)malloc((size_t)m->nl * sizeof(uint32_t));
    mpl_mulmod(&v, x, &m->rint_mod_n, &m->N);
    mpl_mul_u64(&t, &m->N, j);
    mpl_add(&v, &v, &t);
    mpl_to_limbs32(canon, 1, m->nl, LIMB_BITS, &v);
    for (int i = 0; i < m->nl; i++) plane[(size_t)i * batch + k] = canon[i] + m->kp28[i];      /* every limb of K' >= 2^28 - 1 */
    /* one carry-save pass as the kernel's: the carry of limb i - 1 into limb i, the top limb keeps its own */
    uint32_t carry = 0;
    for (int i = 0; i < m->nl; i++) {
        const uint32_t w = plane[(size_t)i * batch + k];
        plane[(size_t)i * batch + k] = (i < m->nl - 1 ? (w & ((1u << LIMB_BITS) - 1)) : w) + carry;
        carry = w >> LIMB_BITS;
    }
    free(canon);
}

static void one_modulus(const char *n_str, int want_nl)
{
    gecm_mod m;
    memset(&m, 0, sizeof m);
    CHECK(gecm_mod_setup(&m, "wide_sanitize", n_str, 52, 0, gecm_mod_wide_nl) == GECM_OK);
    CHECK(m.nl == want_nl && gecm_mod_wide_nl(m.nbits) == want_nl);
    /* the row kernel's constants in a block of exactly their size */
    uint32_t *w = (uint32_t *)malloc(GECM_ROW_KINDS * GECM_ROW_WORDS * sizeof(uint32_t));
    CHECK(gecm_mod_row_consts(&m, m.nl, m.nl + 1, w, NULL) == 1);
    CHECK(w[0] == (1u << LIMB_BITS) - 1);
    CHECK(gecm_mod_row_consts(&m, m.nl, m.nl, w, NULL) == 0 && gecm_mod_row_consts(&m, m.nl - 1, m.nl, w, NULL) == 0);
    for (int i = m.nl + 1; i < GECM_ROW_WORDS; i++) CHECK(w[i] == 0);
    free(w);
    /* a batch of 5: x = 0, 1, N - 1, a number that shares 3 with N where 3 divides it (2^k - 1 for even k), 2^100 */
    const size_t batch = 5, words = (size_t)m.nl * batch;
    uint32_t *rawX = (uint32_t *)calloc(words, 4), *rawZ = (uint32_t *)calloc(words, 4);
    uint32_t *hx = (uint32_t *)calloc(words, 4), *hz = (uint32_t *)calloc(words, 4), *hg = (uint32_t *)calloc(words, 4);
    uint32_t *flags = (uint32_t *)calloc(batch, 4);
    mpl_t x[5], one, want_g;
    mpl_set_u64(&x[0], 0);
    mpl_set_u64(&x[1], 1);
    mpl_set_u64(&one, 1);
    mpl_sub(&x[2], &m.N, &one);
    mpl_set_u64(&x[3], 3 * 1000003ull);
    mpl_gcd(&want_g, &x[3], &m.N);
    const int proper = mpl_cmp_u64(&want_g, 1) > 0;
    mpl_set_u64(&x[4], 1);
    mpl_shl(&x[4], &x[4], 100);                     /* a power of two: coprime to every N */
    for (size_t k = 0; k < batch; k++) {
        lazy_limbs(rawX, batch, k, &m, &x[k], (unsigned)k % 2);
        lazy_limbs(rawZ, batch, batch - 1 - k, &m, &x[k], 1);
    }
    gecm_mod_wide_job j = {.m = &m, .batch = batch, .rawX = rawX, .rawZ = rawZ, .hx = hx, .hz = hz, .hg = hg, .flags = flags};
    CHECK(mpl_invmod(&j.rinv, &m.rint_mod_n, &m.N));
    CHECK(gecm_mod_raw_slice(&j, 0, 2) == 0 && gecm_mod_raw_slice(&j, 2, batch) == 0);
    CHECK(gecm_mod_gcd_slice(&j, 0, batch) == 0);
    for (size_t k = 0; k < batch; k++) {
        mpl_t v;
        mpl_from_limbs32(&v, hx + k, batch, m.nl, LIMB_BITS);
        CHECK(mpl_cmp(&v, &x[k]) == 0);
        mpl_from_limbs32(&v, hz + (batch - 1 - k), batch, m.nl, LIMB_BITS);
        CHECK(mpl_cmp(&v, &x[k]) == 0);
    }
    /* z of curve 4 is x[0] = 0: g = N, no factor; curve 3: z = 1; curve 1: z = x[3] */
    CHECK(flags[4] == 0 && flags[3] == 0 && flags[2] == 0 && flags[0] == 0);
    CHECK(flags[1] == (uint32_t)proper);
    mpl_t g;
    mpl_from_limbs32(&g, hg + 4, batch, m.nl, LIMB_BITS);
    CHECK(mpl_cmp(&g, &m.N) == 0);
    mpl_from_limbs32(&g, hg + 1, batch, m.nl, LIMB_BITS);
    CHECK(mpl_cmp(&g, &want_g) == 0);
    /* any 32-bit words are a value */
    uint32_t *ff = (uint32_t *)malloc((size_t)m.nl * 4);
    memset(ff, 0xff, (size_t)m.nl * 4);
    gecm_mod_raw_value(&g, ff, 1, m.nl);
    CHECK(mpl_bits(&g) == LIMB_BITS * (m.nl - 1) + 32 + (m.nl > 1));
    free(ff);
    free(rawX); free(rawZ); free(hx); free(hz); free(hg); free(flags);
    gecm_mod_free(&m);
}

int main(void)
{
    static const struct { int nl, lo, hi; } classes[] = {{40, 1032, 1115}, {43, 1116, 1199}, {47, 1200, 1311}};
    char s[400];
    CHECK(gecm_wide_max_bits() == GECM_WIDE_MAX_BITS && GECM_WIDE_MAX_BITS == 1311);
    CHECK(gecm_mod_wide_nl(1031) == 40 && gecm_mod_wide_nl(1312) == 0 && gecm_mod_wide_nl(1 << 20) == 0);
    for (size_t c = 0; c < sizeof classes / sizeof *classes; c++) {
        CHECK(gecm_mod_wide_nl(classes[c].lo) == classes[c].nl && gecm_mod_wide_nl(classes[c].hi) == classes[c].nl);
        const int ends[2] = {classes[c].lo, classes[c].hi};
        for (int e = 0; e < 2; e++) {
            number(s, ends[e], 'f', 0);                /* 2^k - 1 */
            one_modulus(s, classes[c].nl);
            number(s, ends[e], 'a', 0);                /* no special form */
            one_modulus(s, classes[c].nl);
            number(s, ends[e], 'c', 1);                /* 1 modulo 2^28: the longest N' */
            one_modulus(s, classes[c].nl);
        }
    }
    /* one bit too many: refused with the text, nothing to free */
    gecm_mod m;
    memset(&m, 0, sizeof m);
    number(s, 1312, 'f', 0);
    CHECK(gecm_mod_setup(&m, "wide_sanitize", s, 52, 0, gecm_mod_wide_nl) == GECM_ERR_ARG);
    CHECK(strstr(gecm_mod_err, "larger than this build supports") != NULL);
    if (failures) { printf("wide_sanitize: %d check(s) failed\n", failures); return 1; }
    printf("wide_sanitize: ok\n");
    return 0;
}
