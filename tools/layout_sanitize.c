/* gecm_layout_make and gecm_layout_free (host/gecm_mod.c) under AddressSanitizer + UBSan: CPU only, a program of its
 * own, the host objects only.  tools/layout_sanitize.sh builds and runs it.  The layout's arrays are heap blocks of
 * exactly their size, so that one entry written past an end is an error the sanitizer sees; what is checked here is
 * that every entry read back is in range and that the maps agree with each other.  The shapes are those of
 * tests/test_layout_cpu.py, a batch of one curve and 1000 moduli with one curve each, in both packings. */
#include "../include/gecm.h"
#include "../avx-ecm_amd/host/gecm_mod.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

/* the batch `counts` describes, modulus 0's first curve moved behind modulus 1's when `swap` */
static void by_counts(const size_t *counts, size_t ngroups, int swap, int packing)
{
    size_t batch = 0, i = 0;
    for (size_t g = 0; g < ngroups; g++) batch += counts[g];
    uint32_t *idx = (uint32_t *)malloc(batch * sizeof(uint32_t));      /* exactly batch entries: read, never past them */
    for (size_t g = 0; g < ngroups; g++)
        for (size_t k = 0; k < counts[g]; k++) idx[i++] = (uint32_t)g;
    if (swap) { const uint32_t t = idx[0]; idx[0] = idx[1]; idx[1] = t; }
    gecm_layout l;
    CHECK(gecm_layout_make(&l, idx, batch, ngroups, packing) == GECM_OK);
    CHECK(l.nuser == batch && l.ngroups == ngroups && l.total % 64 == 0 && l.total >= batch);
    CHECK(l.total == gecm_multi_positions(counts, ngroups, packing));
    CHECK((l.blocks == NULL) == (packing == GECM_PACK_LANE));
    size_t live = 0;
    for (size_t p = 0; p < l.total; p++) {
        CHECK(l.pos_grp[p] < ngroups && (l.pos_user[p] == GECM_PAD || l.pos_user[p] < batch));
        if (l.blocks) CHECK(l.blocks[p / 64] == l.pos_grp[p]);
        if (l.pos_user[p] == GECM_PAD) continue;
        live++;
        CHECK(l.slot[l.pos_user[p]] == p && idx[l.pos_user[p]] == l.pos_grp[p]);
    }
    CHECK(live == batch);
    for (i = 0; i < batch; i++) CHECK(l.slot[i] < l.total && l.pos_user[l.slot[i]] == i);
    for (size_t g = 0; g < ngroups; g++) CHECK(l.cnt[g] == counts[g] && l.goff[g] + l.cnt[g] <= l.total);
    gecm_layout_free(&l);
    CHECK(!l.slot && !l.pos_user && !l.pos_grp && !l.blocks && !l.goff && !l.cnt && !l.total);
    gecm_layout_free(&l);                                              /* nothing left: nothing freed twice */
    free(idx);
}

int main(void)
{
    static size_t ones[1000], rnd[7];
    for (size_t g = 0; g < 1000; g++) ones[g] = 1;
    unsigned s = 7300;
    for (int k = 0; k < 300; k++) { s = s * 1103515245u + 12345u; rnd[(s >> 16) % 7]++; }   /* 300 curves on 7 moduli */
    for (int packing = GECM_PACK_WAVE; packing <= GECM_PACK_LANE; packing++) {
        by_counts((const size_t[]){1, 65}, 2, 1, packing);
        by_counts((const size_t[]){64, 64}, 2, 0, packing);
        by_counts((const size_t[]){63, 0, 1}, 3, 0, packing);
        by_counts((const size_t[]){0, 0, 5}, 3, 0, packing);
        by_counts((const size_t[]){128}, 1, 0, packing);
        by_counts(rnd, 7, 1, packing);
        by_counts((const size_t[]){1}, 1, 0, packing);
        by_counts(ones, 1000, 1, packing);
    }
    /* refusals leave nothing behind (the leak check would say) */
    gecm_layout l;
    const uint32_t idx[3] = {0, 2, 1};
    CHECK(gecm_layout_make(&l, idx, 3, 2, GECM_PACK_WAVE) == GECM_ERR_ARG && !l.slot && !l.cnt);
    CHECK(gecm_layout_make(&l, idx, 0, 3, GECM_PACK_LANE) == GECM_ERR_ARG);
    CHECK(gecm_layout_make(&l, idx, 3, 0, GECM_PACK_LANE) == GECM_ERR_ARG);
    CHECK(gecm_layout_make(&l, NULL, 3, 3, GECM_PACK_WAVE) == GECM_ERR_ARG);
    printf(failures ? "%d check(s) FAILED\n" : "layout sanitizer run complete\n", failures);
    return failures != 0;
}
