/* gecm_resume.c — reading the lines the engine writes (and GMP-ECM's -save files) back: the line parser and the
 * question which prime range a run goes on with.  Device-free, context-free, allocation-free.  Mirrors
 *   save line                   ecm.c:1372-1380
 *   checkpoint line             ecm.c:1295-1305 (the B1 field holds PRIMES[last_pid - 1], ecm.c:1244)
 */
#include "../../include/gecm.h"
#include "gecm_mod.h"
#include "gecm_plan.h"
#include <string.h>

#define set_err gecm_mod_set_err
/* the longest number a line may hold: what an mpl_t takes (mpl_set_str refuses more) */
#define MAX_HEX_DIGITS ((size_t)(MPL_MAXL - 2) * 8)
#define MAX_DEC_DIGITS ((size_t)(MPL_MAXL - 2) * 9)

static int is_space(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }

static int digit_of(char c, int base)
{
    if (c >= '0' && c <= '9') return c - '0';
    if (base == 16 && c >= 'a' && c <= 'f') return c - 'a' + 10;
    if (base == 16 && c >= 'A' && c <= 'F') return c - 'A' + 10;
    return -1;
}

/* the value [p, e) of field `name` as a number: digits only, decimal or after 0x; 0, or GECM_ERR_ARG with the text */
static int take_number(const char *name, const char *p, const char *e, gecm_resume_num *out)
{
    int base = 10;
    if (e - p >= 2 && p[0] == '0' && (p[1] == 'x' || p[1] == 'X')) { base = 16; p += 2; }
    if (p == e) { set_err("gecm_parse_resume_line: field %s is empty", name); return GECM_ERR_ARG; }
    for (const char *q = p; q < e; q++)
        if (digit_of(*q, base) < 0) {
            if (strcmp(name, "N") == 0 && strchr("+-*/^()!#%", *q))
                set_err("gecm_parse_resume_line: field N is an expression, not a number ('%c' at digit %zu)", *q, (size_t)(q - p));
            else
                set_err("gecm_parse_resume_line: field %s: '%c' inside a %s number", name,
                        (*q >= 32 && *q < 127) ? *q : '?', base == 16 ? "hexadecimal" : "decimal");
            return GECM_ERR_ARG;
        }
    while (e - p > 1 && *p == '0') p++;                  /* leading zeros do not count */
    if ((size_t)(e - p) > (base == 16 ? MAX_HEX_DIGITS : MAX_DEC_DIGITS)) {
        set_err("gecm_parse_resume_line: field %s: a number of %zu digits is longer than this build computes with", name,
                (size_t)(e - p));
        return GECM_ERR_ARG;
    }
    out->digits = p;
    out->len = (size_t)(e - p);
    out->base = base;
    return GECM_OK;
}

/* a number that has to fit 64 bits */
static int take_u64(const char *name, const char *p, const char *e, uint64_t *out)
{
    gecm_resume_num n;
    int rc = take_number(name, p, e, &n);
    if (rc) return rc;
    uint64_t v = 0;
    for (size_t i = 0; i < n.len; i++) {
        const uint64_t d = (uint64_t)digit_of(n.digits[i], n.base);
        if (v > (UINT64_MAX - d) / (uint64_t)n.base) {
            set_err("gecm_parse_resume_line: field %s does not fit 64 bits", name);
            return GECM_ERR_ARG;
        }
        v = v * (uint64_t)n.base + d;
    }
    *out = v;
    return GECM_OK;
}

static int name_is(const char *p, const char *e, const char *name)
{
    const size_t n = strlen(name);
    return (size_t)(e - p) == n && memcmp(p, name, n) == 0;
}

/* The METHOD of a line for gecm_parse_resume_line_method: 0 for ECM or no METHOD field, 1 for P-1, 2 for P+1, -1 for
 * anything else.  Looked up before the fields are read: a P-1 / P+1 line's SIGMA and PARAM are not looked at, wherever
 * they stand. */
static int method_of(const char *line)
{
    int meth = 0;
    for (const char *p = line; *p; ) {
        const char *fe = p, *ns = p, *eq = p;
        while (*fe && *fe != ';') fe++;
        while (ns < fe && is_space(*ns)) ns++;
        while (eq < fe && *eq != '=') eq++;
        if (eq < fe) {
            const char *ne = eq, *vs = eq + 1, *ve = fe;
            while (ne > ns && is_space(ne[-1])) ne--;
            while (vs < ve && is_space(*vs)) vs++;
            while (ve > vs && is_space(ve[-1])) ve--;
            if (name_is(ns, ne, "METHOD"))
                meth = name_is(vs, ve, "ECM") ? 0 : name_is(vs, ve, "P-1") ? GECM_METHOD_PM1 : name_is(vs, ve, "P+1") ? GECM_METHOD_PP1 : -1;
        }
        p = *fe ? fe + 1 : fe;
    }
    return meth;
}

/* the body of gecm_parse_resume_line (param == NULL: PARAM 0 only), of gecm_parse_resume_line_param and (x0 != NULL, meth
 * = method_of(line) >= 0) of gecm_parse_resume_line_method */
static int parse_line(const char *line, gecm_resume_rec *rec, int *param, int meth, gecm_resume_num *x0)
{
    uint64_t prm = 0;
    int have_param = 0;
    memset(rec, 0, sizeof *rec);
    const char *p = line;
    while (is_space(*p)) p++;
    if (!*p || *p == '#') return 1;
    int have_sigma = 0, have_b1 = 0;
    while (*p) {
        /* one field: NAME=VALUE up to ';' or the end of the line */
        const char *fe = p;
        while (*fe && *fe != ';') fe++;
        const char *ns = p, *eq = p;
        while (ns < fe && is_space(*ns)) ns++;
        while (eq < fe && *eq != '=') eq++;
        if (ns < fe) {
            if (eq == fe) { set_err("gecm_parse_resume_line: field without '=' (\"%.20s\")", ns); return GECM_ERR_ARG; }
            const char *ne = eq, *vs = eq + 1, *ve = fe;
            while (ne > ns && is_space(ne[-1])) ne--;
            while (vs < ve && is_space(*vs)) vs++;
            while (ve > vs && is_space(ve[-1])) ve--;
            int rc = GECM_OK;
            const int again = (name_is(ns, ne, "SIGMA") && have_sigma) || (name_is(ns, ne, "B1") && have_b1) ||
                              (name_is(ns, ne, "N") && rec->n.digits) || (name_is(ns, ne, "X") && rec->x.digits) ||
                              (name_is(ns, ne, "Z") && rec->z.digits) || (param && name_is(ns, ne, "PARAM") && have_param) ||
                              (x0 && name_is(ns, ne, "X0") && x0->digits);
            if (again) {                              /* two lines run together, most likely */
                set_err("gecm_parse_resume_line: field %.*s appears twice", (int)(ne - ns), ns);
                return GECM_ERR_ARG;
            }
            if (meth && (name_is(ns, ne, "METHOD") || name_is(ns, ne, "SIGMA") || name_is(ns, ne, "PARAM"))) {
                /* a P-1 / P+1 line: METHOD is known, SIGMA and PARAM are ignored */
            } else if (x0 && name_is(ns, ne, "X0")) rc = take_number("X0", vs, ve, x0);
            else if (name_is(ns, ne, "METHOD")) {
                if (!name_is(vs, ve, "ECM")) { set_err("gecm_parse_resume_line: field METHOD is not ECM"); return GECM_ERR_ARG; }
            }
            else if (name_is(ns, ne, "PARAM")) {
                rc = take_u64("PARAM", vs, ve, &prm);
                have_param = 1;
                if (!rc && !param && prm != 0) {
                    set_err("gecm_parse_resume_line: field PARAM = %llu: only PARAM 0 (Suyama's sigma) curves can be resumed",
                            (unsigned long long)prm);
                    return GECM_ERR_ARG;
                }
                if (!rc && prm != GECM_PARAM_SUYAMA && prm != GECM_PARAM_BATCH_SQUARE && prm != GECM_PARAM_BATCH_32) {
                    set_err("gecm_parse_resume_line_param: field PARAM = %llu: curves of PARAM 0, 1 and 3 can be resumed (PARAM 2 "
                            "takes a point multiplication on another curve to get its curve)", (unsigned long long)prm);
                    return GECM_ERR_ARG;
                }
            } else if (name_is(ns, ne, "SIGMA")) {
                rc = take_u64("SIGMA", vs, ve, &rec->sigma);
                have_sigma = 1;
            } else if (name_is(ns, ne, "B1")) {
                rc = take_u64("B1", vs, ve, &rec->b1);
                have_b1 = 1;
            } else if (name_is(ns, ne, "N")) rc = take_number("N", vs, ve, &rec->n);
            else if (name_is(ns, ne, "X")) rc = take_number("X", vs, ve, &rec->x);
            else if (name_is(ns, ne, "Z")) rc = take_number("Z", vs, ve, &rec->z);
            /* CHECKSUM, PROGRAM, WHO, TIME, X0, Y0, Y, COMMENT and whatever else: ignored */
            if (rc) return rc;
        }
        p = *fe ? fe + 1 : fe;
    }
    const char *missing = !have_sigma && !meth ? "SIGMA" : !have_b1 ? "B1" : !rec->n.digits ? "N"
                          : !rec->x.digits ? "X" : NULL;
    if (missing) { set_err("gecm_parse_resume_line: field %s is missing", missing); return GECM_ERR_ARG; }
    if (meth) {
        if (rec->z.digits && !(rec->z.len == 1 && rec->z.digits[0] == '1')) {
            set_err("gecm_parse_resume_line_method: field Z of a %s line is not 1", meth == GECM_METHOD_PM1 ? "P-1" : "P+1");
            return GECM_ERR_ARG;
        }
        if (param) *param = 0;
        return GECM_OK;
    }
    if (prm == GECM_PARAM_SUYAMA && rec->sigma < 6) { set_err("gecm_parse_resume_line: field SIGMA = %llu is below 6", (unsigned long long)rec->sigma); return GECM_ERR_ARG; }
    if (prm != GECM_PARAM_SUYAMA && !gecm_mod_param_sigma_ok((int)prm, rec->sigma)) {
        set_err("gecm_parse_resume_line_param: field SIGMA = %llu is outside [1, 2^%d), the range of PARAM %d",
                (unsigned long long)rec->sigma, prm == GECM_PARAM_BATCH_SQUARE ? 64 : 32, (int)prm);
        return GECM_ERR_ARG;
    }
    if (param) *param = (int)prm;
    return GECM_OK;
}

int gecm_parse_resume_line(const char *line, gecm_resume_rec *rec)
{
    if (!line || !rec) { set_err("gecm_parse_resume_line: bad argument"); return GECM_ERR_ARG; }
    return parse_line(line, rec, NULL, 0, NULL);
}

int gecm_parse_resume_line_param(const char *line, gecm_resume_rec *rec, int *param)
{
    if (!line || !rec || !param) { set_err("gecm_parse_resume_line_param: bad argument"); return GECM_ERR_ARG; }
    return parse_line(line, rec, param, 0, NULL);
}

int gecm_parse_resume_line_method(const char *line, gecm_resume_rec *rec, int *param, int *method, gecm_resume_num *x0)
{
    if (!line || !rec || !param || !method || !x0) { set_err("gecm_parse_resume_line_method: bad argument"); return GECM_ERR_ARG; }
    memset(x0, 0, sizeof *x0);
    *method = GECM_METHOD_ECM;
    const int meth = method_of(line);
    if (meth < 0) { set_err("gecm_parse_resume_line_method: field METHOD is not ECM, P-1 or P+1"); return GECM_ERR_ARG; }
    if (!meth) return parse_line(line, rec, param, 0, NULL);
    gecm_resume_num seed = {NULL, 0, 0};
    const int rc = parse_line(line, rec, param, meth, &seed);
    if (rc) return rc;
    *x0 = seed;
    *method = meth;
    return GECM_OK;
}

int gecm_stage1_resume_range(uint64_t B1, uint64_t b1_field, uint32_t *range)
{
    if (!range || B1 < 2 || B1 > 1000000000000ull) { set_err("gecm_stage1_resume_range: bad argument"); return GECM_ERR_ARG; }
    const uint32_t nranges = gecm_stage1_ranges_plan(B1);
    if (b1_field == B1) { *range = nranges; return GECM_OK; }
    /* the range that ends at prime b1_field is the one the prime lies in; a prime AT a boundary (short test ranges
     * only) ends the list before it */
    const uint64_t at = b1_field / gecm_plan_prime_range();
    for (uint64_t r = at ? at - 1 : 0; r <= at && r < nranges; r++) {
        gecm_range_info ri;
        const int rc = gecm_stage1_range_info(&ri, B1, B1, (uint32_t)r);
        if (rc == -1) { set_err("gecm_stage1_resume_range: out of memory"); return GECM_ERR_NOMEM; }
        if (!rc && ri.exhausted && ri.nprimes && ri.last_prime == b1_field) { *range = (uint32_t)r + 1; return GECM_OK; }
    }
    set_err("gecm_stage1_resume_range: B1 field %llu: not a checkpoint of a run to B1 = %llu", (unsigned long long)b1_field,
            (unsigned long long)B1);
    return GECM_ERR_ARG;
}

/* The standard bound a line's points are complete to.  PROGRAM exactly AVX-ECM: the reference's
 * multiplier, every prime power BELOW the B1 field, which within one prime range is k_std(field - 1); above one range
 * the reference's stage 1 is no prime-power product at all.  Anything else — AVX-ECM-STD, GMP-ECM, no PROGRAM — is a
 * standard line and complete to its field. */
static int std_bound(const char *line, uint64_t *from, int with_param)
{
    gecm_resume_rec rec;
    int prm;
    if (!from) { set_err("gecm_resume_line_std_bound: bad argument"); return GECM_ERR_ARG; }
    int rc = with_param ? gecm_parse_resume_line_param(line, &rec, &prm) : gecm_parse_resume_line(line, &rec);
    if (rc) return rc;
    int reference = 0;
    for (const char *p = line; *p; ) {
        const char *fe = p, *ns = p, *eq = p;
        while (*fe && *fe != ';') fe++;
        while (ns < fe && is_space(*ns)) ns++;
        while (eq < fe && *eq != '=') eq++;
        if (eq < fe) {
            const char *ne = eq, *vs = eq + 1, *ve = fe;
            while (ne > ns && is_space(ne[-1])) ne--;
            while (vs < ve && is_space(*vs)) vs++;
            while (ve > vs && is_space(ve[-1])) ve--;
            if (name_is(ns, ne, "PROGRAM")) reference = name_is(vs, ve, "AVX-ECM");
        }
        p = *fe ? fe + 1 : fe;
    }
    if (!reference) { *from = rec.b1; return GECM_OK; }
    if (rec.b1 > gecm_plan_prime_range()) {
        set_err("gecm_resume_line_std_bound: B1 field %llu of an AVX-ECM line lies above one prime range (%llu): a "
                "reference run over several prime ranges has no standard multiplier (DESIGN.md §5b)",
                (unsigned long long)rec.b1, (unsigned long long)gecm_plan_prime_range());
        return GECM_ERR_ARG;
    }
    if (rec.b1 < 2) { set_err("gecm_resume_line_std_bound: B1 field %llu of an AVX-ECM line is below 2", (unsigned long long)rec.b1); return GECM_ERR_ARG; }
    *from = rec.b1 - 1;
    return GECM_OK;
}

int gecm_resume_line_std_bound(const char *line, uint64_t *from) { return std_bound(line, from, 0); }
int gecm_resume_line_std_bound_param(const char *line, uint64_t *from) { return std_bound(line, from, 1); }

int gecm_resume_line_std_bound_method(const char *line, uint64_t *from)
{
    gecm_resume_rec rec;
    gecm_resume_num x0;
    int prm, meth;
    if (!line || !from) { set_err("gecm_resume_line_std_bound_method: bad argument"); return GECM_ERR_ARG; }
    if (method_of(line) <= 0) return std_bound(line, from, 1);
    const int rc = gecm_parse_resume_line_method(line, &rec, &prm, &meth, &x0);
    if (rc) return rc;
    *from = rec.b1;
    return GECM_OK;
}

/* the hash of the host sources this object was compiled from (Makefile: H_SHA); gecm_version() compares them */
#ifdef GECM_MANIFEST_FN
const char *GECM_MANIFEST_FN(void) { return GECM_MANIFEST; }
#endif
