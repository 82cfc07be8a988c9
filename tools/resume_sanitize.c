/* The resume front end (host/gecm_resume.c: gecm_parse_resume_line, gecm_stage1_resume_range) on well-formed and on
 * malformed input under AddressSanitizer + UBSan: CPU only, a program of its own.  tools/resume_sanitize.sh builds and
 * runs it.  Every line is handed over in a heap block of exactly its size, so that one byte read past its end or before
 * its start is an error the sanitizer sees. */
#include "../include/gecm.h"
#include "../avx-ecm_amd/host/gecm_mod.h"
#include "../avx-ecm_amd/host/gecm_plan.h"
#define gecm_last_error() gecm_mod_err   /* gecm_api.c, which has the accessor, needs the device layer */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static int parse(const char *line, size_t len, gecm_resume_rec *rec)
{
    char *exact = (char *)malloc(len + 1);
    memcpy(exact, line, len);
    exact[len] = 0;
    const int rc = gecm_parse_resume_line(exact, rec);
    if (rc == 0) {       /* what comes back lies inside the line */
        CHECK(rec->n.digits >= exact && rec->n.digits + rec->n.len <= exact + len);
        CHECK(rec->x.digits >= exact && rec->x.digits + rec->x.len <= exact + len);
        CHECK(!rec->z.digits || (rec->z.digits >= exact && rec->z.digits + rec->z.len <= exact + len));
    }
    free(exact);
    return rc;
}

int main(void)
{
    gecm_resume_rec rec;
    const char *good = "METHOD=ECM; SIGMA=1000; B1=2000; N=0x1d5f3b; X=0x1234; Z=0xabc; PROGRAM=AVX-ECM;\n";
    CHECK(parse(good, strlen(good), &rec) == 0 && rec.sigma == 1000 && rec.b1 == 2000 && rec.n.len == 6 && rec.z.base == 16);
    /* every prefix and every suffix of a good line, and the line with each byte in turn replaced */
    for (size_t i = 0; i <= strlen(good); i++) {
        (void)parse(good, i, &rec);
        (void)parse(good + i, strlen(good) - i, &rec);
    }
    for (size_t i = 0; i < strlen(good); i++)
        for (int c = 1; c < 256; c += 7) {
            char tmp[128];
            strcpy(tmp, good);
            tmp[i] = (char)c;
            (void)parse(tmp, strlen(tmp), &rec);
        }
    static const char *refused[] = {
        "METHOD=P-1; SIGMA=1000; B1=2000; N=77; X=5;", "METHOD=ECM; PARAM=1; SIGMA=1000; B1=2000; N=77; X=5;",
        "METHOD=ECM; B1=2000; N=77; X=5;", "METHOD=ECM; SIGMA=1000; N=77; X=5;", "METHOD=ECM; SIGMA=1000; B1=2000; X=5;",
        "METHOD=ECM; SIGMA=1000; B1=2000; N=77;", "METHOD=ECM; SIGMA=5; B1=2000; N=77; X=5;",
        "METHOD=ECM; SIGMA=18446744073709551616; B1=2000; N=77; X=5;", "METHOD=ECM; SIGMA=0x10000000000000000; B1=2000; N=77; X=5;",
        "METHOD=ECM; SIGMA=1000; B1=2000; N=2^127-1; X=5;", "METHOD=ECM; SIGMA=1000; B1=2000; N=77; X=5x;",
        "METHOD=ECM; SIGMA=1000; B1=2000; N=77; X=;", "METHOD=ECM; SIGMA=1000; B1=2000; N=77; X=0x;", "=;=;;;=", "METHOD", ";",
        "SIGMA=;B1=;N=;X=;Z=", "SIGMA=7; B1=8; N=9; X=1; X=2;", "METHOD=ECM; SIGMA=1000; B1=2000; N=77; X=5; Z=0xg",
    };
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) {
        CHECK(parse(refused[i], strlen(refused[i]), &rec) == GECM_ERR_ARG);
        CHECK(strstr(gecm_last_error(), "gecm_parse_resume_line") != NULL);
    }
    CHECK(parse("", 0, &rec) == 1 && parse("  \r\n", 4, &rec) == 1 && parse("# METHOD=ECM", 12, &rec) == 1);
    /* long lines: 10 kB of digits in X (refused: longer than the library computes with), 10 kB of COMMENT (ignored) */
    char *big = (char *)malloc(32768);
    strcpy(big, "METHOD=ECM; SIGMA=1000; B1=2000; N=77; X=0x");
    ((char *)memset(big + strlen(big), 'f', 10240))[10240] = 0;
    strcat(big, "; Z=1;");
    CHECK(parse(big, strlen(big), &rec) == GECM_ERR_ARG && strstr(gecm_last_error(), "X") != NULL);
    strcpy(big, "METHOD=ECM; SIGMA=1000; B1=2000; N=77; X=5; COMMENT=");
    ((char *)memset(big + strlen(big), ' ', 10240))[10240] = 0;
    CHECK(parse(big, strlen(big), &rec) == 0 && !rec.z.digits && rec.x.len == 1);
    free(big);

    uint32_t r = 99;
    CHECK(gecm_stage1_resume_range(1000, 1000, &r) == 0 && r == 1);
    CHECK(gecm_stage1_resume_range(1000, 997, &r) == GECM_ERR_ARG);        /* a range that goes on to primes above B1 writes no checkpoint */
    CHECK(gecm_stage1_resume_range(1000, 991, &r) == GECM_ERR_ARG);
    CHECK(gecm_stage1_resume_range(1, 1, &r) == GECM_ERR_ARG && gecm_stage1_resume_range(1000, 1000, NULL) == GECM_ERR_ARG);
    CHECK(gecm_stage1_resume_range(1000, 0, &r) == GECM_ERR_ARG && gecm_stage1_resume_range(1000, UINT64_MAX, &r) == GECM_ERR_ARG);
    gecm_plan_set_prime_range_for_tests(1000);
    CHECK(gecm_stage1_resume_range(2500, 997, &r) == 0 && r == 1);
    CHECK(gecm_stage1_resume_range(2500, 1999, &r) == 0 && r == 2);
    CHECK(gecm_stage1_resume_range(2500, 2500, &r) == 0 && r == 3);
    CHECK(gecm_stage1_resume_range(2500, 2477, &r) == GECM_ERR_ARG && strstr(gecm_last_error(), "not a checkpoint of a run to B1 = 2500"));
    gecm_plan_set_prime_range_for_tests(503);
    CHECK(gecm_stage1_resume_range(2013, 503, &r) == 0 && r == 1);
    CHECK(gecm_stage1_resume_range(2013, 2011, &r) == 0 && r == 4);
    gecm_plan_set_prime_range_for_tests(0);
    printf(failures ? "resume_sanitize: %d check(s) FAILED\n" : "resume_sanitize: all checks passed\n", failures);
    return failures ? 1 : 0;
}
