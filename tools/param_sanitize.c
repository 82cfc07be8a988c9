/* gecm_param_s (host/gecm_mod.c) and gecm_parse_resume_line_param (host/gecm_resume.c) on good and on malformed input
 * under AddressSanitizer + UBSan: CPU only, a program of its own, the host objects only.  tools/param_sanitize.sh builds
 * and runs it.  Every line is handed over in a heap block of exactly its size, so that one byte read past its end is an
 * error the sanitizer sees; every hex buffer is a heap block of exactly the size it is said to have. */
#include "../include/gecm.h"
#include "../avx-ecm_amd/host/gecm_mod.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static int parse(const char *line, gecm_resume_rec *rec, int *param)
{
    const size_t len = strlen(line);
    char *exact = (char *)malloc(len + 1);
    memcpy(exact, line, len + 1);
    const int rc = gecm_parse_resume_line_param(exact, rec, param);
    if (rc == 0) CHECK(rec->n.digits >= exact && rec->n.digits + rec->n.len <= exact + len && rec->x.digits + rec->x.len <= exact + len);
    free(exact);
    return rc;
}

/* s into a buffer of exactly `room` bytes; the digits (or "") into out */
static int param_s(int param, uint64_t sigma, const char *n, size_t room, char *out)
{
    char *hex = (char *)malloc(room ? room : 1);
    const int rc = gecm_param_s(param, sigma, n, room ? hex : NULL, room);
    out[0] = 0;
    if (rc >= 0) { CHECK((size_t)rc < room && strlen(hex) == (size_t)rc); strcpy(out, hex); }
    free(hex);
    return rc;
}

int main(void)
{
    char got[4096];
    /* values one can check by hand: N = 2^61 - 1 has 2^-64 = 2^58 and 2^-32 = 2^29; N = 3 has both 1 */
    const char *m61 = "2305843009213693951";
    CHECK(param_s(3, 1, m61, 64, got) == 8 && !strcmp(got, "20000000"));
    CHECK(param_s(1, 1, m61, 64, got) == 15 && !strcmp(got, "400000000000000"));
    CHECK(param_s(1, 2, m61, 64, got) == 16 && !strcmp(got, "1000000000000000"));
    CHECK(param_s(1, 0xffffffffffffffffull, "3", 2, got) == 1 && !strcmp(got, "0"));      /* 2^64 - 1 = 0 mod 3 */
    CHECK(param_s(3, 0xffffffffull, "0x3", 2, got) == 1 && !strcmp(got, "0"));
    CHECK(param_s(3, 7, "3", 2, got) == 1 && !strcmp(got, "1"));
    CHECK(param_s(1, 0x8000000000000000ull, m61, 17, got) > 0);
    /* the largest number the library takes, and one digit too many for the buffer */
    static char big[1100];
    memset(big, 'f', 1030 / 4 + 2);
    memcpy(big, "0x", 2);
    const int digits = param_s(1, 0xfffffffffffffffbull, big, sizeof got, got);
    CHECK(digits > 0 && digits <= 1030 / 4);
    CHECK(param_s(1, 0xfffffffffffffffbull, big, (size_t)digits, got) == GECM_ERR_ARG);
    CHECK(param_s(1, 0xfffffffffffffffbull, big, (size_t)digits + 1, got) == digits);
    /* refusals */
    const int bad_param[] = {0, 2, 4, -1, 255, 1 << 30};
    for (size_t i = 0; i < sizeof bad_param / sizeof *bad_param; i++) CHECK(param_s(bad_param[i], 7, m61, 64, got) == GECM_ERR_ARG);
    CHECK(param_s(1, 0, m61, 64, got) == GECM_ERR_ARG && strstr(gecm_mod_err, "SIGMA"));
    CHECK(param_s(3, 0, m61, 64, got) == GECM_ERR_ARG && strstr(gecm_mod_err, "SIGMA"));
    CHECK(param_s(3, 1ull << 32, m61, 64, got) == GECM_ERR_ARG && strstr(gecm_mod_err, "SIGMA"));
    const char *bad_n[] = {"", "0", "1", "2", "10", "0x", "12x", "2^61-1", "7 x", "-7"};
    for (size_t i = 0; i < sizeof bad_n / sizeof *bad_n; i++) CHECK(param_s(1, 7, bad_n[i], 64, got) == GECM_ERR_ARG);
    CHECK(gecm_param_s(1, 7, NULL, got, sizeof got) == GECM_ERR_ARG && gecm_param_s(1, 7, m61, NULL, 0) == GECM_ERR_ARG);
    CHECK(param_s(1, 7, m61, 0, got) == GECM_ERR_ARG && param_s(1, 7, m61, 1, got) == GECM_ERR_ARG);

    /* the parser: good lines */
    gecm_resume_rec rec;
    int param = -7;
    const char *gmp = "METHOD=ECM; PARAM=1; SIGMA=3456789012; B1=11000; N=0x7fffffffffffffff; X=0x123; CHECKSUM=12345; "
                      "PROGRAM=GMP-ECM 7.0.5; X0=0x0; Y0=0x0; WHO=someone@host; TIME=Mon Jan  1 00:00:00 2024;";
    CHECK(parse(gmp, &rec, &param) == 0 && param == 1 && rec.sigma == 3456789012ull && rec.b1 == 11000 && !rec.z.digits);
    CHECK(parse("METHOD=ECM; SIGMA=1; B1=10; N=77; X=5; PARAM=3", &rec, &param) == 0 && param == 3 && rec.sigma == 1);
    CHECK(parse("PARAM=0x3;METHOD=ECM;SIGMA=4294967295;B1=10;N=77;X=5;\r\n", &rec, &param) == 0 && param == 3);
    CHECK(parse("METHOD=ECM; SIGMA=18446744073709551615; B1=10; N=77; X=5; PARAM = 1 ;", &rec, &param) == 0 && param == 1);
    CHECK(parse("METHOD=ECM; SIGMA=7; B1=10; N=77; X=5; Z=3;", &rec, &param) == 0 && param == 0 && rec.z.len == 1);
    CHECK(parse("METHOD=ECM; PARAM=0; SIGMA=7; B1=10; N=77; X=5;", &rec, &param) == 0 && param == 0);
    CHECK(parse("", &rec, &param) == 1 && parse("  # PARAM=1", &rec, &param) == 1);
    /* refusals, each naming its field */
    const struct { const char *line, *field; } bad[] = {
        {"METHOD=ECM; PARAM=2; SIGMA=7; B1=10; N=77; X=5;", "PARAM"},
        {"METHOD=ECM; PARAM=4; SIGMA=7; B1=10; N=77; X=5;", "PARAM"},
        {"METHOD=ECM; PARAM=18446744073709551616; SIGMA=7; B1=10; N=77; X=5;", "PARAM"},
        {"METHOD=ECM; PARAM=; SIGMA=7; B1=10; N=77; X=5;", "PARAM"},
        {"METHOD=ECM; PARAM=1x; SIGMA=7; B1=10; N=77; X=5;", "PARAM"},
        {"METHOD=ECM; PARAM=1; PARAM=1; SIGMA=7; B1=10; N=77; X=5;", "PARAM"},
        {"METHOD=ECM; PARAM=1; SIGMA=0; B1=10; N=77; X=5;", "SIGMA"},
        {"METHOD=ECM; SIGMA=0; B1=10; N=77; X=5; PARAM=3", "SIGMA"},
        {"METHOD=ECM; PARAM=3; SIGMA=4294967296; B1=10; N=77; X=5;", "SIGMA"},
        {"METHOD=ECM; SIGMA=1; B1=10; N=77; X=5;", "SIGMA"},
        {"METHOD=ECM; PARAM=0; SIGMA=5; B1=10; N=77; X=5;", "SIGMA"},
        {"METHOD=ECM; PARAM=1; SIGMA=18446744073709551616; B1=10; N=77; X=5;", "SIGMA"},
        {"METHOD=ECM; PARAM=1; B1=10; N=77; X=5;", "SIGMA"},
        {"METHOD=P-1; PARAM=1; SIGMA=7; B1=10; N=77; X=5;", "METHOD"},
        {"PARAM", "PARAM"}, {"PARAM=", "PARAM"}, {"PARAM=1", "SIGMA"}, {";;PARAM=3;;", "SIGMA"},
    };
    for (size_t i = 0; i < sizeof bad / sizeof *bad; i++) {
        CHECK(parse(bad[i].line, &rec, &param) == GECM_ERR_ARG);
        if (!strstr(gecm_mod_err, bad[i].field)) { printf("FAILED: \"%s\" is refused with \"%s\"\n", bad[i].line, gecm_mod_err); failures++; }
    }
    CHECK(gecm_parse_resume_line_param(NULL, &rec, &param) == GECM_ERR_ARG && gecm_parse_resume_line_param(gmp, NULL, &param) == GECM_ERR_ARG &&
          gecm_parse_resume_line_param(gmp, &rec, NULL) == GECM_ERR_ARG);
    /* the old parser keeps its refusal; the bound of a PARAM line */
    CHECK(gecm_parse_resume_line(gmp, &rec) == GECM_ERR_ARG && strstr(gecm_mod_err, "PARAM"));
    uint64_t from = 0;
    CHECK(gecm_resume_line_std_bound(gmp, &from) == GECM_ERR_ARG && gecm_resume_line_std_bound_param(gmp, &from) == 0 && from == 11000);
    /* every prefix of a good line, and the line with every single byte replaced by ';', '=', a letter and a byte above 127 */
    const size_t len = strlen(gmp);
    for (size_t n = 0; n <= len; n++) {
        char *cut = (char *)malloc(n + 1);
        memcpy(cut, gmp, n);
        cut[n] = 0;
        (void)gecm_parse_resume_line_param(cut, &rec, &param);
        (void)gecm_resume_line_std_bound_param(cut, &from);
        free(cut);
    }
    for (size_t n = 0; n < len; n++)
        for (const char *c = ";=g\xff"; *c; c++) {
            char *mut = (char *)malloc(len + 1);
            memcpy(mut, gmp, len + 1);
            mut[n] = *c;
            (void)gecm_parse_resume_line_param(mut, &rec, &param);
            free(mut);
        }
    printf(failures ? "%d check(s) FAILED\n" : "param sanitizer run complete\n", failures);
    return failures != 0;
}
