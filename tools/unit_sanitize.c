/* gecm_parse_resume_line_method and gecm_resume_line_std_bound_method (host/gecm_resume.c) on good and on malformed input
 * under AddressSanitizer + UBSan: CPU only, a program of its own, the host objects only.  tools/unit_sanitize.sh builds and
 * runs it.  Every line is handed over in a heap block of exactly its size, so that one byte read past its end is an error
 * the sanitizer sees. */
#include "../include/gecm.h"
#include "../avx-ecm_amd/host/gecm_mod.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static int inside(const gecm_resume_num *n, const char *lo, size_t len)
{
    return !n->digits || (n->digits >= lo && n->digits + n->len <= lo + len);
}

static int parse(const char *line, gecm_resume_rec *rec, int *param, int *method, gecm_resume_num *x0)
{
    const size_t len = strlen(line);
    char *exact = (char *)malloc(len + 1);
    memcpy(exact, line, len + 1);
    const int rc = gecm_parse_resume_line_method(exact, rec, param, method, x0);
    if (rc == 0) CHECK(rec->n.digits && rec->x.digits && inside(&rec->n, exact, len) && inside(&rec->x, exact, len) &&
                       inside(&rec->z, exact, len) && inside(x0, exact, len));
    free(exact);
    return rc;
}

static int bound(const char *line, uint64_t *from)
{
    const size_t len = strlen(line);
    char *exact = (char *)malloc(len + 1);
    memcpy(exact, line, len + 1);
    const int rc = gecm_resume_line_std_bound_method(exact, from);
    free(exact);
    return rc;
}

int main(void)
{
    gecm_resume_rec rec;
    gecm_resume_num x0;
    int param = -7, method = -7;
    uint64_t from = 0;
    const char *good[] = {
        "METHOD=P-1; B1=11000; N=0x7fffffffffffffff; X=0x123; X0=0x3; PROGRAM=AVX-ECM-STD;\n",
        "METHOD=P+1; B1=11000; N=0x7fffffffffffffff; X=0x123; X0=0x2f; PROGRAM=AVX-ECM-STD;\n",
        "METHOD=P-1; B1=1000000; N=9223372036854775807; X=291; CHECKSUM=12345; PROGRAM=GMP-ECM 7.0.5; X0=0x3; WHO=someone@host; "
        "TIME=Mon Jan  1 00:00:00 2024;",
        "X=5;N=77;B1=10;METHOD=P+1\r\n",
        "METHOD=ECM; PARAM=1; SIGMA=3456789012; B1=11000; N=0x7fffffffffffffff; X=0x123; PROGRAM=GMP-ECM 7.0.5; X0=0x0; Y0=0x0;",
    };
    CHECK(parse(good[0], &rec, &param, &method, &x0) == 0 && method == GECM_METHOD_PM1 && param == 0 && rec.sigma == 0 &&
          rec.b1 == 11000 && !rec.z.digits && x0.digits && x0.len == 1 && x0.base == 16);   /* (the digits themselves are in the block parse() has freed) */
    CHECK(parse(good[1], &rec, &param, &method, &x0) == 0 && method == GECM_METHOD_PP1 && x0.len == 2);
    CHECK(parse(good[2], &rec, &param, &method, &x0) == 0 && method == GECM_METHOD_PM1 && rec.b1 == 1000000 && rec.x.base == 10);
    CHECK(parse(good[3], &rec, &param, &method, &x0) == 0 && method == GECM_METHOD_PP1 && !x0.digits && rec.b1 == 10);
    CHECK(parse(good[4], &rec, &param, &method, &x0) == 0 && method == GECM_METHOD_ECM && param == 1 && !x0.digits &&
          rec.sigma == 3456789012ull);
    CHECK(bound(good[0], &from) == 0 && from == 11000);
    CHECK(bound(good[3], &from) == 0 && from == 10);
    CHECK(bound(good[4], &from) == 0 && from == 11000);
    CHECK(bound("METHOD=ECM; SIGMA=7; B1=1000; N=77; X=5; PROGRAM=AVX-ECM;", &from) == 0 && from == 999);
    CHECK(bound("METHOD=P-1; SIGMA=7; B1=1000; N=77; X=5; PROGRAM=AVX-ECM;", &from) == 0 && from == 1000);
    CHECK(parse("METHOD=P-1; SIGMA=0; PARAM=2; B1=10; N=77; X=5; Z=1;", &rec, &param, &method, &x0) == 0 && method == 1 && param == 0);
    CHECK(parse("", &rec, &param, &method, &x0) == 1 && parse("  # METHOD=P-1", &rec, &param, &method, &x0) == 1);
    CHECK(bound("", &from) == 1);
    /* refusals, each naming its field */
    const struct { const char *line, *field; } bad[] = {
        {"METHOD=FOO; B1=10; N=77; X=5;", "METHOD"},     {"METHOD=P-1; B1=10; N=77; X=5; Z=2;", "field Z"},
        {"METHOD=P+1; B1=10; N=77; X=5; Z=0;", "field Z"}, {"METHOD=P-1; B1=10; N=77;", "field X"},
        {"METHOD=P-1; N=77; X=5;", "field B1"},           {"METHOD=P-1; B1=10; X=5;", "field N"},
        {"METHOD=P-1; B1=10; N=77; X=5; X=6;", "field X appears twice"},
        {"METHOD=P-1; B1=10; N=77; X=5; X0=6; X0=6", "field X0 appears twice"},
        {"METHOD=P-1; B1=10; N=77; X=5; X0=;", "field X0"}, {"METHOD=P+1; B1=10; N=77; X=5; X0=0xg;", "field X0"},
        {"METHOD=P-1; B1=1e3; N=77; X=5;", "field B1"},   {"METHOD=P-1; B1=10; N=2^7-1; X=5;", "field N"},
        {"METHOD=P-1", "field B1"}, {"METHOD=P-1;;;", "field B1"}, {"METHOD=ECM; B1=10; N=77; X=5;", "SIGMA"},
    };
    for (size_t i = 0; i < sizeof bad / sizeof *bad; i++) {
        CHECK(parse(bad[i].line, &rec, &param, &method, &x0) == GECM_ERR_ARG);
        if (!strstr(gecm_mod_err, bad[i].field)) { printf("FAILED: \"%s\" is refused with \"%s\"\n", bad[i].line, gecm_mod_err); failures++; }
        CHECK(bound(bad[i].line, &from) == GECM_ERR_ARG);
    }
    CHECK(gecm_parse_resume_line_method(NULL, &rec, &param, &method, &x0) == GECM_ERR_ARG);
    CHECK(gecm_parse_resume_line_method(good[0], NULL, &param, &method, &x0) == GECM_ERR_ARG);
    CHECK(gecm_parse_resume_line_method(good[0], &rec, NULL, &method, &x0) == GECM_ERR_ARG);
    CHECK(gecm_parse_resume_line_method(good[0], &rec, &param, NULL, &x0) == GECM_ERR_ARG);
    CHECK(gecm_parse_resume_line_method(good[0], &rec, &param, &method, NULL) == GECM_ERR_ARG);
    CHECK(gecm_resume_line_std_bound_method(NULL, &from) == GECM_ERR_ARG && gecm_resume_line_std_bound_method(good[0], NULL) == GECM_ERR_ARG);
    /* the older parsers keep their refusal */
    CHECK(gecm_parse_resume_line(good[0], &rec) == GECM_ERR_ARG && strstr(gecm_mod_err, "METHOD is not ECM"));
    CHECK(gecm_parse_resume_line_param(good[1], &rec, &param) == GECM_ERR_ARG && strstr(gecm_mod_err, "METHOD is not ECM"));
    CHECK(gecm_resume_line_std_bound(good[0], &from) == GECM_ERR_ARG && gecm_resume_line_std_bound_param(good[0], &from) == GECM_ERR_ARG);
    /* every prefix of every good line, and every line with every single byte replaced by ';', '=', a letter, a digit, a
     * byte above 127 and the end of the string */
    for (size_t g = 0; g < sizeof good / sizeof *good; g++) {
        const size_t len = strlen(good[g]);
        for (size_t n = 0; n <= len; n++) {
            char *cut = (char *)malloc(n + 1);
            memcpy(cut, good[g], n);
            cut[n] = 0;
            (void)parse(cut, &rec, &param, &method, &x0);
            (void)bound(cut, &from);
            free(cut);
        }
        for (size_t n = 0; n < len; n++)
            for (const char *c = ";=g1\xff+- "; *c; c++) {
                char *mut = (char *)malloc(len + 1);
                memcpy(mut, good[g], len + 1);
                mut[n] = *c;
                (void)parse(mut, &rec, &param, &method, &x0);
                (void)bound(mut, &from);
                free(mut);
            }
    }
    printf(failures ? "%d check(s) FAILED\n" : "unit sanitizer run complete\n", failures);
    return failures != 0;
}
