/* The extension planner (host/gecm_plan.c: gecm_tape_build_extend, the segment rule, gecm_extend_segment_info) and
 * gecm_resume_line_std_bound (host/gecm_resume.c) on good and on malformed input under AddressSanitizer + UBSan: CPU
 * only, a program of its own.  tools/extend_sanitize.sh builds and runs it.  Every line is handed over in a heap block of
 * exactly its size, so that one byte read past its end is an error the sanitizer sees. */
#include "../include/gecm.h"
#include "../avx-ecm_amd/host/gecm_mod.h"
#include "../avx-ecm_amd/host/gecm_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int failures;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static int bound(const char *line, uint64_t *from)
{
    const size_t len = strlen(line);
    char *exact = (char *)malloc(len + 1);
    memcpy(exact, line, len + 1);
    const int rc = gecm_resume_line_std_bound(exact, from);
    free(exact);
    return rc;
}

static void tape(uint64_t lo, uint64_t hi, int threads)
{
    gecm_tape_t t;
    const int rc = gecm_tape_build_extend(&t, lo, hi, threads);
    printf("extend (%llu, %llu] threads=%d rc=%d len=%zu adds=%llu dups=%llu chains=%llu last=%llu\n", (unsigned long long)lo,
           (unsigned long long)hi, threads, rc, t.len, (unsigned long long)t.ptadds, (unsigned long long)t.ptdups,
           (unsigned long long)t.prac_calls, (unsigned long long)t.last_prime);
    CHECK(rc == (lo >= 1 && hi >= lo ? 0 : -2));
    gecm_tape_free(&t);
}

int main(void)
{
    /* tapes: small, empty, single powers, threaded, the top of the range, bad bounds */
    const uint64_t top = 1000000000000ull;
    const uint64_t pairs[][2] = {{1, 1}, {1, 2}, {1, 3}, {2, 3}, {1, 1000}, {999, 3000}, {342, 343}, {1023, 1024}, {500, 500},
                                 {1, 300000}, {999999, 3000000}, {top, top}, {top - 1000, top}, {0, 10}, {11, 10}};
    for (size_t i = 0; i < sizeof pairs / sizeof *pairs; i++)
        for (int threads = 1; threads <= 8; threads += 7) tape(pairs[i][0], pairs[i][1], threads);
    /* segments, with the real range and a short one */
    for (int pass = 0; pass < 2; pass++) {
        gecm_plan_set_prime_range_for_tests(pass ? 256 : 0);
        const uint64_t to = pass ? 1000 : 250000000ull;
        const uint32_t n = gecm_extend_segments_plan(1, to);
        CHECK(n == (pass ? 4u : 3u));
        uint64_t prev = 1;
        for (uint32_t s = 0; s < n + 1; s++) {
            uint64_t lo = 0, hi = 0;
            gecm_extend_info ei;
            const int rc = gecm_extend_segment_bounds(1, to, s, &lo, &hi);
            CHECK(rc == (s < n ? 0 : -2));
            CHECK(gecm_extend_segment_info(&ei, 1, to, s) == rc);
            if (rc) continue;
            CHECK(lo == prev && hi > lo && ei.lo == lo && ei.hi == hi);
            printf("segment %u of (1, %llu]: (%llu, %llu] primes=%llu further=%llu last=%llu\n", s, (unsigned long long)to,
                   (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)ei.nprimes,
                   (unsigned long long)ei.power_steps, (unsigned long long)ei.last_prime);
            prev = hi;
        }
        CHECK(prev == to);
    }
    gecm_plan_set_prime_range_for_tests(0);
    CHECK(gecm_extend_segments_plan(0, 5) == 0 && gecm_extend_segments_plan(6, 5) == 0 && gecm_extend_segments_plan(top, top) == 1);
    /* the bound of a line */
    uint64_t from = 0;
    const char *ref = "METHOD=ECM; SIGMA=1000; B1=1000; N=0x7fffffffffffffff; X=0x123; Z=0x45; PROGRAM=AVX-ECM;";
    CHECK(bound(ref, &from) == 0 && from == 999);
    CHECK(bound("METHOD=ECM; SIGMA=1000; B1=1000; N=0x7fffffffffffffff; X=0x123; Z=0x45; PROGRAM=AVX-ECM-STD;\r\n", &from) == 0 && from == 1000);
    CHECK(bound("METHOD=ECM; PARAM=0; SIGMA=1000; B1=1000; N=77; X=5; PROGRAM=GMP-ECM 7.0.5", &from) == 0 && from == 1000);
    CHECK(bound("METHOD=ECM; SIGMA=1000; B1=1000; N=77; X=5", &from) == 0 && from == 1000);
    CHECK(bound("PROGRAM=AVX-ECM;METHOD=ECM;SIGMA=1000;B1=100000001;N=77;X=5", &from) == GECM_ERR_ARG);
    CHECK(strstr(gecm_mod_err, "several prime ranges") != NULL);
    CHECK(bound("PROGRAM = AVX-ECM ;METHOD=ECM;SIGMA=1000;B1=1;N=77;X=5", &from) == GECM_ERR_ARG);
    CHECK(bound("", &from) == 1 && bound("   # x", &from) == 1);
    const char *bad[] = {"PROGRAM", "PROGRAM=", "PROGRAM=;", ";;;=;", "=", "PROGRAM=AVX-ECM", "METHOD=ECM; SIGMA=7; B1=; N=77; X=5;",
                         "METHOD=ECM; SIGMA=7; B1=18446744073709551616; N=77; X=5;", "METHOD=ECM; SIGMA=7; B1=10; N=77; X=5; PROGRAM",
                         "METHOD=ECM; SIGMA=7; B1=10; N=77; X=5; PROGRAM=AVX-ECM; PROGRAM=other"};
    for (size_t i = 0; i < sizeof bad / sizeof *bad; i++) (void)bound(bad[i], &from);
    CHECK(bound(ref, NULL) == GECM_ERR_ARG);
    /* every prefix of a good line */
    for (size_t n = 0; n <= strlen(ref); n++) {
        char *cut = (char *)malloc(n + 1);
        memcpy(cut, ref, n);
        cut[n] = 0;
        (void)gecm_resume_line_std_bound(cut, &from);
        free(cut);
    }
    printf(failures ? "%d check(s) FAILED\n" : "extend sanitizer run complete\n", failures);
    return failures != 0;
}
