/* avx_ecm_main.c — the avx-ecm command line on top of libgecm.
 *
 *     avx-ecm input curves B1 [threads] [B2] [sigma]
 *     avx-ecm -f FILE curves B1 [threads] [B2] [sigma]      (a list of inputs, run_file)
 *     avx-ecm -r FILE B1 [B2]                               (go on from resume lines, run_resume)
 *     avx-ecm -x FILE B1 [B2]                               (take resume lines to a higher B1, run_resume)
 *     avx-ecm -g -r FILE B1 [B2],  avx-ecm -g -x FILE B1 [B2]  (the same two, lines of GMP-ECM's PARAM 1 and 3 accepted)
 *     avx-ecm -p PARAM input curves B1 [B2] [sigma]         (a fresh run in standard mode, PARAM 0, 1 or 3, run_param)
 *     avx-ecm -m pm1|pp1 input B1 [x0]                      (P-1 or P+1 stage 1 on one number, run_method)
 *     avx-ecm -m pm1|pp1 -f FILE B1,  avx-ecm -m pm1|pp1 -x FILE B1   (on a list of inputs; P-1 / P+1 lines on to B1)
 *     avx-ecm -m pm1|pp1 -b B2 ...                          (any of the three, followed by stage 2 to B2)
 *
 * Same positional arguments as the reference (main.c:380-384, 459-460, 537-559) and the same FILES, byte for byte:
 * save_b1.txt (GMP-ECM resume lines, ecm.c:1372-1380), ecm_results.txt (factor lines, ecm.c:1356-1367, 1510-1522)
 * and, for B1 above one prime range of 1e8, checkpoint.txt (ecm.c:1236-1312).  GMP-ECM then resumes with
 *     ecm -resume save_b1.txt <B1> <B2>
 *
 * How the reference's run maps onto the GPU.  vececm (ecm.c:1077-1544) works in BATCHES of 8 curves per thread:
 * for every batch it builds the curves, runs stage 1 (one ecm_stage1 call per prime range), appends the batch to
 * save_b1.txt, runs stage 2, and stops after the first batch in which any curve found a factor (ecm.c:1531-1532).
 * Line j*8 + i of a batch belongs to thread j, vector lane i; its label in ecm_results.txt is
 * "curve threads*curve + j*8 + i, thread j, vec i" (ecm.c:1356-1366).  With a sigma on the command line every thread
 * of a batch runs the SAME eight sigmas sigma + curve + i (ecm.c:1187 copies thread 0's): the batch has 8 distinct
 * curves and 8*threads lines.  Without one every lane draws its own (ecm.c:1564-1570).
 *
 * Here a PASS puts many reference batches on the GPU(s) at once — up to 131072 distinct curves per GPU — and then
 * writes exactly what the reference would have written for those batches one after the other: the lines of every
 * batch up to and including the first one with a factor, that batch's factor lines, nothing after it.  With a fixed
 * sigma the 8 distinct curves of a batch are computed once and written `threads` times.  The 4th argument therefore
 * keeps everything a script can observe (curve-count rounding main.c:585-589, banner, labels, line count); it does not
 * select GPUs: the run uses every visible HIP device (or the first GECM_GPUS), one host thread and one gecm_ctx per
 * GPU, and the files do not depend on how many there are.
 *
 * Passes are pipelined when there are several (and B1 is within one prime range): two sets of contexts alternate, so
 * that the curve construction of pass k+1 and the formatting and writing of pass k-1 (host work) run while the
 * kernels of pass k do; files are written in pass order.  stdout carries the reference's lines per PASS, not per
 * batch (its timings are per pass too).
 *
 * Defaults as the reference: B2 = 100*B1 (main.c:462), B2 <= B1 disables stage 2 (main.c:548-552), no sigma = random
 * 64-bit sigmas >= 6.
 */
#include "../../include/gecm.h"
#include "calc_lite.h"
#include "gecm_pair.h"
#include "mpl.h"
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>
#include <unistd.h>

#define MAX_GPUS 16
/* The reference is built in two flavours (avx_ecm.h:65-93): DIGITBITS = 52 with VECLEN = 8 curves per vector, and
 * DIGITBITS = 32 with VECLEN = 16.  The flavour decides the NWORDS/MAXBITS rule and its banner lines, the size of a batch
 * (VECLEN x threads lines) and therefore where a run stops, never a residue.  This source builds both: avx-ecm and
 * avx-ecm-32 (Makefile: -DGECM_CLI_DIGITBITS=32). */
#ifndef GECM_CLI_DIGITBITS
#define GECM_CLI_DIGITBITS 52
#endif
#define VECLEN (GECM_CLI_DIGITBITS == 52 ? 8 : 16)
/* distinct curves per GPU per pass: 2 wavefronts on each of the 1024 SIMDs of an MI355X */
#define FULL_BATCH 131072u
#define PRIME_RANGE 100000000ULL

static double now(void)
{
    struct timeval tv;
    gettimeofday(&tv, NULL);
    return (double)tv.tv_sec + 1e-6 * (double)tv.tv_usec;
}

/* lcg_rand, main.c:993-998 */
static uint64_t lcg_rand(uint64_t *state)
{
    *state = 6364136223846793005ULL * (*state) + 1442695040888963407ULL;
    return *state;
}

/* the pair map of the first prime range of stage 2 (ecm.c:1441-1443): identical for every batch, GPU and pass, so it
 * is made once, on the thread of the first pass, while the GPUs run the first stage 1 */
typedef struct {
    uint64_t lo, hi;
    uint32_t D, U;
    gecm_pairs pm;
    int valid;
    int settled;               /* made or failed: the job threads wait for this before they prepare their tapes */
    int claimed;               /* some pass has taken on making it */
    pthread_mutex_t mu;
    pthread_cond_t cv;
} first_range_t;

/* ---- run-wide state ------------------------------------------------------------------------- */
enum { GPU, OUT };             /* what passes take turns on: the GPUs, and the files and stdout */
enum { DONE, FOUND, FAILED };  /* how a pass leaves a turn */

typedef struct {
    uint64_t B1, B2, sigma0;
    int do_stage2, threads, fixed_sigma;
    int gpus;                  /* contexts per slot */
    int nranges;               /* ecm_stage1 calls per batch (prime ranges of 1e8) */
    size_t per_thread;         /* tdata[0].curves */
    size_t nbatches;           /* reference batches of the run: ceil(per_thread / 8) */
    size_t ub;                 /* distinct curves per reference batch: 8 (fixed sigma) or 8*threads */
    first_range_t fr;
    gecm_stage1_range_desc *rd;   /* what vececm prints and decides around each prime range (made once, on a helper thread) */
    int rd_rc;
    char rd_err[512];          /* gecm_last_error() of the helper thread (the text is thread-local) */
    /* pipeline: passes take the GPUs and write their output in pass order */
    pthread_mutex_t mu;
    pthread_cond_t cv;
    size_t turn[2];            /* the pass whose turn it is on the GPUs / on the output */
    size_t found_pass;         /* the pass that found a factor (SIZE_MAX: none yet): later passes are not run, not written */
    int failed;
    uint64_t lcg;
    double t_start;
    /* avx-ecm -r: the passes start from the lines of a file (resume_t), stage 1 goes on at first_range (nranges:
     * it is complete, the lines are save lines: nothing is added to save_b1.txt and stage-1 factors are old news) */
    const struct resume_t *res;
    int first_range, s1_complete;
    /* avx-ecm -x: the lines are complete to the standard bound ext_from and go on to B1 in nranges extension segments
     * (gecm_stage1_extend_segment); every line written is a normalised standard line (gecm_format_save_line_std) */
    int extend;
    uint64_t ext_from;
    /* avx-ecm -g -r / -g -x: the lines carry their parametrisation (PARAM 0, 1, 3) into the build;
     * avx-ecm -p: fresh curves of the parametrisation fresh_param, run as an extension from the bound 1 */
    int with_params, fresh, fresh_param;
} run_t;

typedef struct {
    char *buf;
    size_t len, cap;
} text_t;

/* ---- the curves of one input's batches and where each lives: all that formatting and writing them needs ---- */
typedef struct {
    gecm_ctx *ctx;
    const uint64_t *sigma;     /* by context index */
    size_t ncurves, first;     /* this context's slice: distinct curves first .. first+ncurves */
    size_t koff;               /* context index of distinct curve `first` (0; a multi-modulus pass: the input's first) */
} part_t;

/* checkpoints (several prime ranges): per range written, its lines in (batch, thread, lane) order and the factor lines
 * of the first flagged batch */
typedef struct {
    char **lines;              /* ucurves resume lines (distinct curves) */
    size_t first_flagged;      /* batch (within the pass), or nb if none */
    text_t res;                /* ecm_results.txt lines of that batch */
} ck_t;

typedef struct {
    const run_t *run;
    size_t b0, nb;             /* reference batches b0 .. b0+nb of the run */
    size_t ucurves;            /* distinct curves = nb * ub */
    int nparts;
    part_t part[MAX_GPUS];
    int nck;
    ck_t *ck;
    long ck_offset;            /* where this pass's part of checkpoint.txt starts */
} view_t;

/* ---- what only the pipeline needs: the per-GPU jobs of a pass, its thread, its place in the order, its log ---- */
typedef struct job_t {
    int gpu;
    const part_t *part;
    int (*step)(struct job_t *);
    uint64_t B1;
    uint32_t range;
    int rc;
    char err[512];
    const gecm_pairs *pm;      /* the pair map of the current prime range (made once, shared) */
    first_range_t *fr;         /* stage 1: the first range's map, being made on the pass thread meanwhile (or NULL) */
    double kernel_ms;
    int progress;              /* print the launches of a long stage 1 as they finish (GPU 0 of a pass that prints live) */
    const void *rx, *rz;       /* -r: the plain residues of the part's curves (vec layout), and what stage 1 has done */
    uint64_t b1_done;
    const uint8_t *param;      /* -g, -p: the parametrisation of the part's curves (NULL: Suyama's throughout) */
} job_t;

typedef struct {
    run_t *run;                /* NULL: no pass in this slot */
    size_t index;              /* pass number */
    view_t v;
    uint64_t *sigma;
    job_t jobs[MAX_GPUS];
    text_t log;                /* this pass's stdout, released in pass order */
    int live;                  /* not pipelined: print as it happens */
    pthread_t th;
    int threaded;              /* th is a thread to join */
    void *rx, *rz;             /* -r: the residues its one job starts from */
    uint8_t *param;            /* -g, -p: the parametrisation of its curves */
} pass_t;

static void text_add(text_t *t, const char *s, size_t n)
{
    if (t->len + n + 1 > t->cap) {
        size_t cap = t->cap ? t->cap * 2 : 4096;
        while (cap < t->len + n + 1) cap *= 2;
        char *p = (char *)realloc(t->buf, cap);
        if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
        t->buf = p;
        t->cap = cap;
    }
    memcpy(t->buf + t->len, s, n);
    t->len += n;
    t->buf[t->len] = 0;
}

static void text_vprintf(text_t *t, const char *fmt, va_list ap)
{
    char tmp[8192];
    int n = vsnprintf(tmp, sizeof tmp, fmt, ap);
    if (n > 0) text_add(t, tmp, (size_t)n < sizeof tmp ? (size_t)n : sizeof tmp - 1);
}

static void text_printf(text_t *t, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    text_vprintf(t, fmt, ap);
    va_end(ap);
}

/* a line of this pass's stdout */
static void plog(pass_t *ps, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    text_vprintf(&ps->log, fmt, ap);
    va_end(ap);
    if (ps->live && ps->log.len) { fputs(ps->log.buf, stdout); fflush(stdout); ps->log.len = 0; }
}

/* an environment knob that counts something: its value, 0 when unset or not positive */
static long env_count(const char *name)
{
    const char *s = getenv(name);
    const long v = s ? atol(s) : 0;
    return v > 0 ? v : 0;
}

/* the sieved interval, prime count, first and last prime and checkpoint decision of every stage-1 range: 0.25 s of
 * sieving per range, done once while the contexts are made and the first curves built */
static void *describe_ranges(void *arg)
{
    run_t *R = (run_t *)arg;
    for (int r = 0; r < R->nranges && !R->rd_rc; r++)
        R->rd_rc = gecm_stage1_describe_range(R->B1, R->B2, (uint32_t)r, &R->rd[r]);
    if (R->rd_rc) snprintf(R->rd_err, sizeof R->rd_err, "%s", gecm_last_error());
    return NULL;
}

/* Where the driver's contexts build their curves: the files are byte for byte the same either way, so this is a matter
 * of time alone (DESIGN.md §15 has the measurement behind the default).  GECM_CURVE_BUILD=host|device overrides it. */
#define CLI_CURVE_BUILD GECM_BUILD_HOST
static int set_curve_build(gecm_ctx *ctx)
{
    const char *s = getenv("GECM_CURVE_BUILD");
    const int where = !s ? CLI_CURVE_BUILD : !strcmp(s, "device") ? GECM_BUILD_DEVICE : !strcmp(s, "host") ? GECM_BUILD_HOST : -1;
    return gecm_set_curve_build(ctx, where);
}

/* How the multi-modulus passes of -f and -r are packed (include/gecm.h gecm_set_multi_packing):
 * GECM_PACKING=lane|wave, wave when unset.  The files are byte for byte the same either way.  Lane packing serves the
 * passes whose inputs all fit it (gecm_multi_packing_max_bits); a pass is closed when the next input falls on the other
 * side of that line, and the passes of larger numbers stay wave-packed.  A lane-packed context builds its curves on the
 * host, so the combination with GECM_CURVE_BUILD=device is refused before anything runs.  Returns the packing, or -1
 * after printing why not. */
static int cli_packing(void)
{
    const char *s = getenv("GECM_PACKING"), *b = getenv("GECM_CURVE_BUILD");
    const int packing = !s || !strcmp(s, "wave") ? GECM_PACK_WAVE : !strcmp(s, "lane") ? GECM_PACK_LANE : -1;
    if (packing < 0) printf("GECM_PACKING must be lane or wave\n");
    else if (packing == GECM_PACK_LANE && b && !strcmp(b, "device")) {
        printf("GECM_PACKING=lane builds its curves on the host: it cannot be combined with GECM_CURVE_BUILD=device\n");
        return -1;
    }
    return packing;
}

/* positions of a pass of n inputs with `each` curves each (gecm_multi_positions has the rule: lane packing rounds the
 * sum, wave packing every input) */
static size_t pass_positions(size_t n, size_t each, int packing)
{
    const size_t all = n * each;
    return packing == GECM_PACK_LANE ? gecm_multi_positions(&all, 1, packing) : n * gecm_multi_positions(&each, 1, packing);
}

/* Sub-sequences per curve in stage 2 of the multi-modulus passes of -f, -r and -x (include/gecm.h
 * gecm_set_stage2_subseq): GECM_MULTI_SUBSEQ=auto|default, default when unset.  The files are byte for
 * byte the same either way.  Returns the setting, or 1 (no setting has that value) after printing why not. */
static int cli_multi_subseq(void)
{
    const char *s = getenv("GECM_MULTI_SUBSEQ");
    if (!s || !strcmp(s, "default")) return GECM_S2_SUBSEQ_DEFAULT;
    if (!strcmp(s, "auto")) return GECM_S2_SUBSEQ_AUTO;
    printf("GECM_MULTI_SUBSEQ must be auto or default\n");
    return 1;
}

/* Stage 1 of the curves of the multi-modulus passes of -f, -r and -x with 32 lanes per curve (include/gecm.h
 * gecm_set_multi_rows): GECM_MULTI_ROWS=on|auto|off, off when unset.  The files are byte for byte the
 * same whatever the value.  Returns the setting, or 2 (no setting has that value) after printing why not. */
static int cli_multi_rows(void)
{
    const char *s = getenv("GECM_MULTI_ROWS");
    if (!s || !strcmp(s, "off")) return GECM_MULTI_ROWS_OFF;
    if (!strcmp(s, "on")) return GECM_MULTI_ROWS_ON;
    if (!strcmp(s, "auto")) return GECM_MULTI_ROWS_AUTO;
    printf("GECM_MULTI_ROWS must be on, auto or off\n");
    return 2;
}

/* Lanes per residue in stage 1 of the -m pm1|pp1 passes (include/gecm.h gecm_set_method_lanes):
 * GECM_METHOD_LANES=1|16|auto, 1 when unset.  The files are byte for byte the same whatever the value.  Returns the
 * setting, or 0 (no setting has that value) after printing why not. */
static int cli_method_lanes(void)
{
    const char *s = getenv("GECM_METHOD_LANES");
    if (!s || !strcmp(s, "1")) return 1;
    if (!strcmp(s, "16")) return 16;
    if (!strcmp(s, "auto")) return GECM_METHOD_LANES_AUTO;
    printf("GECM_METHOD_LANES must be 1, 16 or auto\n");
    return 0;
}

static int fits_lane_packing(int nbits) { return nbits <= gecm_multi_packing_max_bits(GECM_PACK_LANE); }

/* ---- per-GPU jobs of a pass ----------------------------------------------------------------- */
static int step_build(job_t *j)
{
    if (j->param && gecm_set_next_params(j->part->ctx, j->param, j->part->ncurves)) return -1;
    return gecm_build_curves(j->part->ctx, j->part->sigma, j->part->ncurves);
}

/* -r: the curves of the lines; save lines (stage 1 complete) get the factor scan a stage 1 would have ended with */
static int step_resume(job_t *j)
{
    if (j->param && gecm_set_next_params(j->part->ctx, j->param, j->part->ncurves)) return -1;
    int rc = gecm_resume_points(j->part->ctx, j->part->sigma, j->rx, j->rz, j->part->ncurves, j->b1_done);
    if (rc >= 0 && j->b1_done && gecm_scan_factors(j->part->ctx, 1, NULL) < 0) rc = -1;
    return rc;
}

static int step_stage1(job_t *j)
{
    gecm_ctx *ctx = j->part->ctx;
    int rc = gecm_stage1_range(ctx, j->B1, j->range);                     /* returns after the launch */
    if (rc == 0 && j->fr) {
        /* while the kernel runs: this context's launch tape of the first stage-2 range, as soon as the pass
         * thread has the pair map (0.13 s of host time; later passes find it kept) */
        first_range_t *fr = j->fr;
        pthread_mutex_lock(&fr->mu);
        while (!fr->settled) pthread_cond_wait(&fr->cv, &fr->mu);
        pthread_mutex_unlock(&fr->mu);
        if (fr->valid)
            (void)gecm_stage2_pair_prepare(ctx, fr->D, fr->U, fr->pm.steps, fr->pm.pairmap_v, fr->pm.pairmap_u, fr->pm.amin);
    }
    if (rc == 0 && j->progress) {
        /* a 1e8 prime range is 13 launches of up to minutes each: say where it is (the reference prints
         * "accumulating prime" every 8192 primes, ecm.c:1834-1842) */
        uint32_t done = 0, total = 0, shown = 0;
        while (gecm_stage1_progress(ctx, &done, &total) == 0 && total > 1 && done < total) {
            if (done != shown) { printf("stage 1, range %u: launch %u of %u done\r", j->range, done, total); fflush(stdout); shown = done; }
            usleep(200000);
        }
    }
    if (rc == 0) rc = gecm_sync(ctx);
    if (rc == 0) j->kernel_ms += gecm_last_kernel_ms(ctx);
    /* the device factor scan and the download of x, z belong to the GPU's turn (the next pass's kernel would
     * keep them waiting); formatting happens later, off the GPU */
    if (rc == 0 && gecm_scan_factors(ctx, 1, NULL) < 0) rc = -1;
    return rc;
}

/* -x: one extension segment, then the normalisation every standard line needs and the factor scan */
static int step_extend(job_t *j)
{
    gecm_ctx *ctx = j->part->ctx;
    int rc = gecm_stage1_extend_segment(ctx, j->b1_done, j->B1, j->range);
    if (rc == 0) rc = gecm_sync(ctx);
    if (rc == 0) j->kernel_ms += gecm_last_kernel_ms(ctx);
    if (rc == 0 && gecm_normalize_points(ctx) < 0) rc = -1;
    if (rc == 0 && gecm_scan_factors(ctx, 1, NULL) < 0) rc = -1;
    return rc;
}

static int step_stage2_init(job_t *j)
{
    const int rc = gecm_stage2_init(j->part->ctx, 0, 0);                  /* ecm.c:1401-1407 */
    return rc ? rc : gecm_sync(j->part->ctx);
}

static int step_stage2_pair(job_t *j)
{
    const int rc = gecm_stage2_pair(j->part->ctx, j->pm->steps, j->pm->pairmap_v, j->pm->pairmap_u, j->pm->amin);   /* ecm.c:1460 */
    return rc ? rc : gecm_sync(j->part->ctx);
}

static int step_stage2_scan(job_t *j)
{
    return gecm_scan_factors(j->part->ctx, 2, NULL) < 0 ? -1 : 0;
}

/* the thread of a job: nothing to do without curves; the error text is taken here, on the thread that made it
 * (gecm_last_error() is thread-local) */
static void *job_run(void *p)
{
    job_t *j = (job_t *)p;
    j->rc = j->part->ncurves ? j->step(j) : 0;
    if (j->rc < 0) snprintf(j->err, sizeof j->err, "%s", gecm_last_error());
    return NULL;
}

static void make_first_range(first_range_t *fr)
{
    if (!fr->valid) {
        fr->valid = gecm_pair_primes(&fr->pm, fr->lo, fr->hi, fr->D, fr->U) == 0;
    }
    pthread_mutex_lock(&fr->mu);
    fr->settled = 1;
    pthread_cond_broadcast(&fr->cv);
    pthread_mutex_unlock(&fr->mu);
}

static int run_all(job_t *jobs, int n, int (*step)(job_t *), first_range_t *meanwhile, int make_it)
{
    pthread_t th[MAX_GPUS];
    for (int i = 0; i < n; i++) { jobs[i].step = step; jobs[i].fr = meanwhile; }
    /* job 0 on this thread — unless the map is to be made: then every job on a thread of its own, the host work here */
    const int here = !(meanwhile && make_it);
    for (int i = here; i < n; i++) pthread_create(&th[i], NULL, job_run, &jobs[i]);
    if (here) job_run(&jobs[0]);
    else make_first_range(meanwhile);
    for (int i = here; i < n; i++) pthread_join(th[i], NULL);
    for (int i = 0; i < n; i++)
        if (jobs[i].rc < 0) {
            fprintf(stderr, "GPU %d: %s\n", jobs[i].gpu, jobs[i].err);
            return -1;
        }
    return 0;
}

/* ---- where a line of the reference's files comes from ------------------------------------------
 * Line `l` (0 .. 8*threads) of batch b of a view is distinct curve b*ub + (fixed sigma ? l % 8 : l) of the view ... */
static inline size_t line_curve(const run_t *R, size_t b, size_t l)
{
    return b * R->ub + (R->fixed_sigma ? l % VECLEN : l);
}

/* ... and distinct curve u is held by one of the view's contexts: which, and at which index */
static const part_t *locate(const view_t *v, size_t u, size_t *k)
{
    for (int i = 0; i < v->nparts; i++)
        if (u >= v->part[i].first && u < v->part[i].first + v->part[i].ncurves) {
            *k = u - v->part[i].first + v->part[i].koff;
            return &v->part[i];
        }
    *k = 0;
    return &v->part[0];
}

/* the first of batches 0 .. upto with a curve flagged after stage 1 (stages = 2: after either stage); upto if none */
static size_t first_flagged(const view_t *v, size_t upto, int stages)
{
    for (size_t u = 0; u < upto * v->run->ub && u < v->ucurves; u++) {   /* (-r: the last batch may be short) */
        size_t k;
        const part_t *p = locate(v, u, &k);
        if (gecm_curve_flag(p->ctx, 1, k) || (stages > 1 && gecm_curve_flag(p->ctx, 2, k))) return u / v->run->ub;
    }
    return upto;
}

/* the factor lines of batch b (ecm.c:1336-1367 for stage 1, 1485-1522 for stage 2): stdout and ecm_results.txt text.
 * label: the number printed as "B1 = " / "B2 = ". */
static void factor_lines(const view_t *v, int stage, size_t b, uint64_t label, text_t *res, text_t *out)
{
    const run_t *R = v->run;
    static __thread char fac[4096];
    for (size_t l = 0; l < (size_t)VECLEN * (size_t)R->threads; l++) {
        size_t k;
        if (line_curve(R, b, l) >= v->ucurves) continue;
        const part_t *p = locate(v, line_curve(R, b, l), &k);
        if (!gecm_curve_flag(p->ctx, stage, k)) continue;
        int prp = 0;
        int r = stage == 1 ? gecm_stage1_factor(p->ctx, k, fac, sizeof fac, &prp)
                           : gecm_stage2_factor(p->ctx, k, fac, sizeof fac, &prp);
        if (r != 1) continue;
        const size_t j = l / VECLEN, i = l % VECLEN;
        const size_t curve = (size_t)R->threads * VECLEN * (v->b0 + b) + l;        /* threads*curve + j*VECLEN + i */
        const unsigned long sg = (unsigned long)p->sigma[k];
        text_printf(out, "\nfound %s%d factor %s in stage %d (B%d = %lu): thread %zu, vec %zu, sigma %lu\n", prp ? "PRP" : "C",
                    gecm_sizeinbase10(fac), fac, stage, stage, (unsigned long)label, j, i, sg);
        text_printf(res, "\nfound %s%d factor %s in stage %d (B%d = %lu): curve %zu, thread %zu, vec %zu, sigma %lu\n",
                    prp ? "PRP" : "C", gecm_sizeinbase10(fac), fac, stage, stage, (unsigned long)label, curve, j, i, sg);
    }
}

/* resume lines of the view's distinct curves, formatted by worker threads (gecm_format_resume_line only reads the
 * downloaded x, z) */
typedef struct {
    const view_t *v;
    uint64_t b1_field;
    size_t lo, hi;
    char **lines;
} fmt_job;

static void *fmt_run(void *arg)
{
    fmt_job *f = (fmt_job *)arg;
    static __thread char line[16384];
    for (size_t u = f->lo; u < f->hi; u++) {
        size_t k;
        const part_t *p = locate(f->v, u, &k);
        int n = f->v->run->extend ? gecm_format_save_line_std(p->ctx, k, line, sizeof line)    /* at the context's B1 */
                                  : gecm_format_resume_line(p->ctx, k, f->b1_field, line, sizeof line);
        f->lines[u] = n > 0 ? strdup(line) : NULL;
    }
    return NULL;
}

static char **format_lines(const view_t *v, uint64_t b1_field, size_t upto)
{
    char **lines = (char **)calloc(v->ucurves ? v->ucurves : 1, sizeof(char *));
    if (!lines) { fprintf(stderr, "out of memory\n"); return NULL; }
    long ncpu = sysconf(_SC_NPROCESSORS_ONLN);
    int nt = ncpu > 16 ? 16 : ncpu < 1 ? 1 : (int)ncpu;
    if ((size_t)nt > upto / 512 + 1) nt = (int)(upto / 512 + 1);
    fmt_job fj[16];
    pthread_t th[16];
    for (int t = 0; t < nt; t++) {
        fj[t].v = v; fj[t].b1_field = b1_field; fj[t].lines = lines;
        fj[t].lo = upto * (size_t)t / (size_t)nt;
        fj[t].hi = upto * (size_t)(t + 1) / (size_t)nt;
    }
    for (int t = 1; t < nt; t++)
        if (pthread_create(&th[t], NULL, fmt_run, &fj[t])) { fmt_run(&fj[t]); th[t] = 0; }
    fmt_run(&fj[0]);
    for (int t = 1; t < nt; t++)
        if (th[t]) pthread_join(th[t], NULL);
    return lines;
}

/* batches b_from .. b_to of `lines` to f in the reference's order: per batch, thread by thread, lane by lane */
static void write_batches(const view_t *v, FILE *f, char **lines, size_t b_from, size_t b_to)
{
    for (size_t b = b_from; b < b_to; b++)
        for (size_t l = 0; l < (size_t)VECLEN * (size_t)v->run->threads; l++) {
            const size_t u = line_curve(v->run, b, l);
            if (u < v->ucurves && lines[u]) fputs(lines[u], f);
        }
}

static void free_lines(char **lines, size_t n)
{
    if (!lines) return;
    for (size_t i = 0; i < n; i++) free(lines[i]);
    free(lines);
}

/* ---- what a view writes ------------------------------------------------------------------------
 * What the reference would have written for these batches, one after the other: the first batch in which anything
 * was found — at a checkpoint, after stage 1 or after stage 2 — is the last one written. */
typedef struct {
    size_t bstar, nwrite;      /* the first batch with a factor (nb: none); batches to write */
    int found;
    char **lines;
    text_t res, out1, out2;    /* ecm_results.txt lines; stdout lines after stage 1 / after stage 2 */
} output_t;

/* Known from the device scans alone, so a pass settles it before the GPUs go on: a pass behind a factor is not even
 * started. */
static void output_settle(const view_t *v, output_t *o)
{
    memset(o, 0, sizeof *o);
    o->bstar = v->nb;
    for (int c = 0; c < v->nck; c++)
        if (v->ck[c].first_flagged < o->bstar) o->bstar = v->ck[c].first_flagged;
    o->bstar = first_flagged(v, o->bstar, v->run->do_stage2 ? 2 : 1);
    o->found = o->bstar < v->nb;
    o->nwrite = o->found ? o->bstar + 1 : v->nb;
}

/* host work, off the GPU: the resume lines and the factor text; 0, or -1 without memory */
static int output_format(const view_t *v, output_t *o)
{
    const run_t *R = v->run;
    o->lines = format_lines(v, R->B1, o->nwrite * R->ub < v->ucurves ? o->nwrite * R->ub : v->ucurves);
    if (!o->lines) return -1;
    if (o->found) {
        for (int c = 0; c < v->nck; c++)
            if (v->ck[c].first_flagged == o->bstar && v->ck[c].res.len) text_add(&o->res, v->ck[c].res.buf, v->ck[c].res.len);
        if (!R->s1_complete) factor_lines(v, 1, o->bstar, R->B1, &o->res, &o->out1);
        if (R->do_stage2) factor_lines(v, 2, o->bstar, R->B2, &o->res, &o->out2);
    }
    return 0;
}

/* files and stdout; log, s2log: what else the view has to say before and after save_b1.txt (or NULL) */
static void output_write(const view_t *v, const output_t *o, const char *log, const char *s2log)
{
    if (log) fputs(log, stdout);
    if (o->out1.len) fputs(o->out1.buf, stdout);
    FILE *save = v->run->s1_complete ? NULL : fopen("save_b1.txt", "a");
    if (save) { write_batches(v, save, o->lines, 0, o->nwrite); fclose(save); }
    else if (!v->run->s1_complete) printf("could not open save_b1.txt for appending, Stage 1 data will not be saved\n");
    if (s2log) fputs(s2log, stdout);
    if (o->out2.len) fputs(o->out2.buf, stdout);
    if (o->res.len) {
        FILE *f = fopen("ecm_results.txt", "a");
        if (f) { fputs(o->res.buf, f); fclose(f); }
    }
    /* checkpoint.txt of a pass of several batches: the reference has them batch by batch (all ranges of batch
     * 0, then batch 1, ...) and nothing after the batch that found a factor */
    if (v->nck && (v->nb > 1 || o->found)) {
        FILE *cf = fopen("checkpoint.txt", "r+");
        if (cf) {
            if (ftruncate(fileno(cf), v->ck_offset) == 0) {
                fseek(cf, 0, SEEK_END);
                for (size_t b = 0; b < o->nwrite; b++)
                    for (int c = 0; c < v->nck; c++) write_batches(v, cf, v->ck[c].lines, b, b + 1);
            }
            fclose(cf);
        }
    }
    fflush(stdout);
}

static void output_release(const view_t *v, output_t *o)
{
    free_lines(o->lines, v->ucurves);
    free(o->res.buf); free(o->out1.buf); free(o->out2.buf);
}

/* ---- the order of the passes --------------------------------------------------------------------
 * Every pass — run, skipped or failed — waits for its turn on the GPUs and then on the output and leaves each exactly
 * once, in that order: the counters only go up, so a failed run cannot leave a pass waiting. */

/* wait until it is pass i's turn on x (or the run failed); nonzero when the pass is not to take it: an earlier pass
 * found a factor, or the run failed */
static int turn_wait(run_t *R, int x, size_t i)
{
    pthread_mutex_lock(&R->mu);
    while (R->turn[x] != i && !R->failed) pthread_cond_wait(&R->cv, &R->mu);
    const int stop = R->found_pass < i || R->failed;
    pthread_mutex_unlock(&R->mu);
    return stop;
}

/* pass i is done with x, and how: FOUND a factor, FAILED, or just DONE */
static void turn_done(run_t *R, int x, size_t i, int how)
{
    pthread_mutex_lock(&R->mu);
    if (how == FOUND && R->found_pass > i) R->found_pass = i;
    if (how == FAILED) R->failed = 1;
    if (R->turn[x] <= i) R->turn[x] = i + 1;
    pthread_cond_broadcast(&R->cv);
    pthread_mutex_unlock(&R->mu);
}

static void pass_fail(pass_t *ps)
{
    turn_done(ps->run, GPU, ps->index, FAILED);
    turn_done(ps->run, OUT, ps->index, FAILED);
}

/* ---- one pass --------------------------------------------------------------------------------- */

/* ecm.c:1236-1312: the batch goes to checkpoint.txt with the last prime in the B1 field; factors are looked for and
 * reported as after stage 1 proper.  Written now (a checkpoint is for the crash that may follow), all batches of the
 * pass; put into the reference's order when the pass is over. */
static int pass_checkpoint(pass_t *ps, uint64_t last_prime)
{
    view_t *v = &ps->v;
    ck_t *ck = &v->ck[v->nck];
    memset(ck, 0, sizeof *ck);
    ck->lines = format_lines(v, last_prime, v->ucurves);
    if (!ck->lines) return -1;
    ck->first_flagged = first_flagged(v, v->nb, 1);
    if (ck->first_flagged < v->nb) {
        text_t out = {0, 0, 0};
        factor_lines(v, 1, ck->first_flagged, last_prime, &ck->res, &out);
        if (out.len) plog(ps, "%s", out.buf);
        free(out.buf);
    }
    FILE *cf = fopen("checkpoint.txt", "a");
    if (cf) {
        plog(ps, "Saving checkpoint after p=%lu\n", (unsigned long)last_prime);                    /* ecm.c:1244 */
        if (v->nck == 0) { fseek(cf, 0, SEEK_END); v->ck_offset = ftell(cf); }
        write_batches(v, cf, ck->lines, 0, v->nb);
        fclose(cf);
    } else
        plog(ps, "could not open checkpoint.txt for appending, Stage 1 data will not be saved\n");
    v->nck++;
    return 0;
}

/* stage 1 of the pass's batches, prime range by prime range (ecm.c:1209-1312); 0, or -1 after an error */
static int pass_stage1(pass_t *ps)
{
    run_t *R = ps->run;
    const int G = R->gpus;
    const double t = now();
    gecm_stage1_stats st;
    memset(&st, 0, sizeof st);
    for (int r = R->first_range; r < R->nranges; r++) {
        const gecm_stage1_range_desc *rd = &R->rd[r];
        /* the reference sieves range 0 once before its first batch (ecm.c:1139-1146) and again whenever a batch
         * starts after a later range was loaded (ecm.c:1160-1173) */
        if (r > 0 || R->nranges > 1)
            plog(ps, "Found %lu primes in range [%lu : %lu]\n", (unsigned long)rd->nprimes, (unsigned long)rd->lo, (unsigned long)rd->hi);   /* ecm.c:1228 */
        plog(ps, "Commencing Stage 1 @ prime %lu\n", (unsigned long)rd->first_prime);              /* ecm.c:1233 */
        for (int g = 0; g < G; g++) { ps->jobs[g].B1 = R->B1; ps->jobs[g].range = (uint32_t)r; ps->jobs[g].progress = ps->live && g == 0; }
        int make_map = 0;
        first_range_t *fr = NULL;
        if (R->do_stage2 && r == R->nranges - 1) {
            fr = &R->fr;
            pthread_mutex_lock(&fr->mu);
            if (!fr->claimed) { fr->claimed = 1; make_map = 1; }
            pthread_mutex_unlock(&fr->mu);
        }
        if (run_all(ps->jobs, G, step_stage1, fr, make_map)) return -1;
        gecm_get_stage1_stats(ps->v.part[0].ctx, &st);
        plog(ps, "\nStage 1 completed at prime %lu with %lu point-adds and %lu point-doubles\n",
             (unsigned long)st.last_prime, (unsigned long)st.ptadds, (unsigned long)st.ptdups);     /* ecm.c:1849 */
        if (rd->checkpoint && pass_checkpoint(ps, rd->last_prime)) return -1;
    }
    const double t_stage1 = now() - t;
    plog(ps, "Stage 1 took %1.4f seconds\n", t_stage1);                                             /* ecm.c:1317 */
    plog(ps, "(%.1f curves/sec; kernel %.1f ms on GPU 0)\n", (double)ps->v.ucurves / t_stage1, ps->jobs[0].kernel_ms);
    return 0;
}

/* -x: the extension segments of the pass's curves, one after the other; checkpoint.txt gets the standard lines of
 * every segment's end but the last, whose lines are the save lines; 0, or -1 after an error */
static int pass_extend(pass_t *ps)
{
    run_t *R = ps->run;
    const double t = now();
    gecm_stage1_stats st;
    memset(&st, 0, sizeof st);
    for (int sg = 0; sg < R->nranges; sg++) {
        gecm_extend_desc d;
        if (gecm_stage1_describe_extend(R->ext_from, R->B1, (uint32_t)sg, &d)) { fprintf(stderr, "%s\n", gecm_last_error()); return -1; }
        plog(ps, "Extending Stage 1 over (%lu : %lu]: %lu primes and %lu further prime-power steps\n", (unsigned long)d.lo,
             (unsigned long)d.hi, (unsigned long)d.nprimes, (unsigned long)d.power_steps);
        for (int g = 0; g < R->gpus; g++) { ps->jobs[g].B1 = R->B1; ps->jobs[g].range = (uint32_t)sg; ps->jobs[g].b1_done = R->ext_from; }
        if (run_all(ps->jobs, R->gpus, step_extend, NULL, 0)) return -1;
        gecm_get_stage1_stats(ps->v.part[0].ctx, &st);
        plog(ps, "Stage 1 complete to %lu at prime %lu with %lu point-adds and %lu point-doubles\n", (unsigned long)d.hi,
             (unsigned long)st.last_prime, (unsigned long)st.ptadds, (unsigned long)st.ptdups);
        if (sg + 1 < R->nranges && pass_checkpoint(ps, d.hi)) return -1;
    }
    const double t_stage1 = now() - t;
    plog(ps, "Stage 1 took %1.4f seconds\n", t_stage1);
    plog(ps, "(%.1f curves/sec; kernel %.1f ms on GPU 0)\n", (double)ps->v.ucurves / t_stage1, ps->jobs[0].kernel_ms);
    return 0;
}

/* stage 2 (ecm.c:1394-1528); what it prints goes to s2log, which comes after save_b1.txt; 0, or -1 after an error */
static int pass_stage2(pass_t *ps, text_t *s2log)
{
    run_t *R = ps->run;
    const int G = R->gpus;
    gecm_ctx *ctx0 = ps->v.part[0].ctx;
    gecm_stage2_stats s2;
    memset(&s2, 0, sizeof s2);
    const double t = now();
    if (run_all(ps->jobs, G, step_stage2_init, NULL, 0)) return -1;                                /* ecm.c:1401-1421 */
    text_printf(s2log, "Stage 2 Init took %1.4f seconds\n", now() - t);                            /* ecm.c:1421 */
    gecm_get_stage2_stats(ctx0, &s2);
    uint32_t rcount = 0;
    for (uint32_t i = 0; i < 2 * s2.D; i++) {                                                      /* main.c:874-882: R - 3 */
        uint32_t a = i, b = 2 * s2.D;
        while (b) { uint32_t rr = a % b; a = b; b = rr; }
        rcount += a == 1;
    }
    const first_range_t *fr = &R->fr;
    for (uint64_t p = R->B1; p < R->B2; p += PRIME_RANGE) {                                        /* ecm.c:1424-1476 */
        const uint64_t hi = p + PRIME_RANGE < R->B2 ? p + PRIME_RANGE : R->B2;
        gecm_pairs pm;
        const int shared = fr->valid && p == fr->lo && hi == fr->hi && s2.D == fr->D && s2.U == fr->U;
        text_printf(s2log, "commencing pair on range %lu:%lu\n", (unsigned long)p, (unsigned long)hi);       /* ecm.c:2568 */
        if (shared) pm = fr->pm;
        else if (gecm_pair_primes(&pm, p, hi, s2.D, s2.U)) { fprintf(stderr, "%s\n", gecm_last_error()); return -1; }
        text_printf(s2log, "%u pairs found from %u primes (ratio = %1.2f)\n", pm.pairs, pm.primes,
                    pm.primes ? (double)pm.pairs / (double)pm.primes : 0.0);                       /* ecm.c:2904-2905 */
        text_printf(s2log, "\ncommencing stage 2 at A=%lu\nw = %u, R = %u, L = %u, U = %d, umax = %u, amin = %u\n",
                    2ul * (unsigned long)pm.amin * s2.D, s2.D, rcount, s2.L, (int)s2.U, s2.U * s2.D, pm.amin);   /* ecm.c:2440-2442 */
        for (int g = 0; g < G; g++) ps->jobs[g].pm = &pm;
        const int rc = run_all(ps->jobs, G, step_stage2_pair, NULL, 0);
        if (!shared) gecm_pairmap_release(&pm);
        if (rc) return -1;
        gecm_get_stage2_stats(ctx0, &s2);
        text_printf(s2log, "\nlast amin: %u\n", s2.amin_last);                                     /* ecm.c:1462 */
    }
    if (run_all(ps->jobs, G, step_stage2_scan, NULL, 0)) return -1;
    text_printf(s2log, "\nStage 2 took %1.4f seconds\n", now() - t);                               /* ecm.c:1481 */
    text_printf(s2log, "performed %lu pt-adds, %lu inversions, and %lu pair-muls in stage 2\n",
                (unsigned long)s2.ptadds, (unsigned long)s2.numinv, (unsigned long)s2.paired);     /* ecm.c:1482 */
    return 0;
}

static void *pass_run(void *arg)
{
    pass_t *ps = (pass_t *)arg;
    run_t *R = ps->run;
    const view_t *v = &ps->v;
    const size_t i = ps->index, lines_per_batch = (size_t)VECLEN * (size_t)R->threads;
    text_t s2log = {0, 0, 0};
    output_t o = {0};
    int failed = 1;

    /* host: the curves (ecm.c:1177-1204) */
    double t_build = now();
    if (run_all(ps->jobs, R->gpus, R->res ? step_resume : step_build, NULL, 0)) goto out;
    t_build = now() - t_build;

    /* the GPUs, in pass order */
    if (turn_wait(R, GPU, i)) {                   /* an earlier pass found a factor: this one is not run at all */
        turn_done(R, GPU, i, DONE);
        (void)turn_wait(R, OUT, i);
        turn_done(R, OUT, i, DONE);
        return NULL;
    }
    plog(ps, "\nCommencing curves %zu-%zu of %zu\n", lines_per_batch * v->b0, lines_per_batch * (v->b0 + v->nb) - 1,
         (size_t)R->threads * R->per_thread);                                                      /* ecm.c:1201 */
    plog(ps, "Building curves took %1.4f seconds.\n", t_build);                                    /* ecm.c:1204 */
    if ((!R->s1_complete && (R->extend ? pass_extend(ps) : pass_stage1(ps))) || (R->do_stage2 && pass_stage2(ps, &s2log))) goto out;
    output_settle(v, &o);
    turn_done(R, GPU, i, o.found ? FOUND : DONE);   /* the GPUs go to the next pass */

    if (output_format(v, &o)) goto out;
    /* files and stdout, in pass order */
    if (!turn_wait(R, OUT, i)) output_write(v, &o, ps->live ? NULL : ps->log.buf, s2log.buf);
    turn_done(R, OUT, i, DONE);
    failed = 0;
out:
    if (failed) pass_fail(ps);
    output_release(v, &o);
    free(s2log.buf);
    return NULL;
}

/* wait for the pass of a slot, if there is one, and release what it holds */
static void pass_join(pass_t *ps)
{
    if (!ps->run) return;
    if (ps->threaded) pthread_join(ps->th, NULL);
    for (int c = 0; c < ps->v.nck; c++) {
        free_lines(ps->v.ck[c].lines, ps->v.ucurves);
        free(ps->v.ck[c].res.buf);
    }
    free(ps->v.ck);
    free(ps->sigma);
    free(ps->rx);
    free(ps->rz);
    free(ps->param);
    free(ps->log.buf);
    memset(ps, 0, sizeof *ps);
}

/* curves B1 [threads] [B2] [sigma], argv[0] being curves: the reference's rules for them, and what follows from them
 * for the whole run (R->t_start is set already: the seed takes it); 0, or 1 after saying what is wrong */
static int parse_run(run_t *R, int argc, char **argv)
{
    size_t numcurves = strtoul(argv[0], NULL, 10);
    R->B1 = strtoull(argv[1], NULL, 10);
    R->B2 = 100ULL * R->B1;                                                       /* main.c:462 */
    R->threads = 1;
    R->do_stage2 = 1;
    if (argc > 2) R->threads = atoi(argv[2]);
    if (argc > 3) R->B2 = strtoull(argv[3], NULL, 10);
    if (argc > 4) R->sigma0 = strtoull(argv[4], NULL, 10);
    if (R->B2 <= R->B1) { R->do_stage2 = 0; R->B2 = R->B1; }                      /* main.c:548-552 */
    if (R->threads < 1) R->threads = 1;
    R->fixed_sigma = R->sigma0 > 0;                                               /* main.c:754-770 */
    if (numcurves == 0 || R->B1 < 2 || R->B1 > 1000000000000ULL) { printf("need curves >= 1 and 2 <= B1 <= 1e12\n"); return 1; }
    /* main.c:585-589: at least one curve per thread, the same number on every thread; ecm.c:1151: every thread
     * runs whole vectors of VECLEN curves, so "10 curves" on one thread writes 16 resume lines there and here */
    if (numcurves < (size_t)R->threads) numcurves = (size_t)R->threads;
    R->per_thread = numcurves / (size_t)R->threads + (numcurves % (size_t)R->threads != 0);
    R->nbatches = (R->per_thread + VECLEN - 1) / VECLEN;
    R->ub = R->fixed_sigma ? VECLEN : (size_t)VECLEN * (size_t)R->threads;
    R->lcg = (uint64_t)(R->t_start * 1e6) * 0x9E3779B97F4A7C15ULL + (uint64_t)getpid();
    return 0;
}

/* one context per GPU of a slot, on `modulus`, reporting against `report` if that is another number; 0 or 2.
 * wide: a modulus above gecm_create's limit gets a wide context (include/gecm.h gecm_create_wide: stage 1 only), which
 * the plain run takes; every other mode keeps gecm_create and its one-line refusal of such a number. */
static int make_contexts(gecm_ctx **ctx, int n, int devices, const char *modulus, const char *report, int wide)
{
    for (int g = 0; g < n; g++)
        if ((wide ? gecm_create_wide : gecm_create)(&ctx[g], g % devices, modulus, GECM_CLI_DIGITBITS) ||
            (report && gecm_set_report_modulus(ctx[g], report)) ||
            set_curve_build(ctx[g])) {
            fprintf(stderr, "%s\n", gecm_last_error());
            return 2;
        }
    return 0;
}

/* ---- avx-ecm -r: the lines of a resume file --------------------------------------------------------------------
 * One group = consecutive lines on one N.  The text stays as read; rec points into it. */
typedef struct {
    char *text;
    gecm_resume_rec rec;
    int param;                 /* -g: the line's PARAM (0, 1 or 3); else 0 */
} rline_t;

typedef struct resume_t {
    const rline_t *lines;      /* of the group the run is on */
    size_t nlines;
} resume_t;

/* a number of a line as an integer (the parser has checked its digits and its length) */
static void rnum(mpl_t *v, const gecm_resume_num *n)
{
    static __thread char tmp[MPL_MAXL * 10 + 16];
    if (!n->digits) { mpl_set_u64(v, 1); return; }              /* Z absent */
    const size_t off = n->base == 16 ? 2 : 0;
    memcpy(tmp, "0x", off);
    memcpy(tmp + off, n->digits, n->len);
    tmp[off + n->len] = 0;
    if (mpl_set_str(v, tmp)) mpl_set_u64(v, 0);
}

/* x and z of `count` lines as vec operands of a context with this configuration */
static int pack_residues(const gecm_config *cfg, const rline_t *lines, size_t count, size_t lane0, size_t batch, void *x, void *z)
{
    for (size_t i = 0; i < count; i++)
        for (int q = 0; q < 2; q++) {
            mpl_t v;
            rnum(&v, q ? &lines[i].rec.z : &lines[i].rec.x);
            if (cfg->digitbits == 52) mpl_to_limbs64((uint64_t *)(q ? z : x) + lane0 + i, batch, cfg->nwords, 52, &v);
            else mpl_to_limbs32((uint32_t *)(q ? z : x) + lane0 + i, batch, cfg->nwords, 32, &v);
        }
    return 0;
}

/* the sigmas and residues of a pass of a resumed run: lines b0*ub .. of the group, fewer in a last, short batch */
static int resume_pass_input(pass_t *ps, const gecm_ctx *ctx)
{
    const run_t *R = ps->run;
    view_t *v = &ps->v;
    const size_t first = v->b0 * R->ub;
    if (first + v->ucurves > R->res->nlines) v->ucurves = R->res->nlines - first;
    gecm_config cfg;
    gecm_get_config(ctx, &cfg);
    const size_t bytes = v->ucurves * (size_t)cfg.nwords * (cfg.digitbits == 52 ? 8 : 4);
    ps->rx = malloc(bytes);
    ps->rz = malloc(bytes);
    if (!ps->rx || !ps->rz) { fprintf(stderr, "out of memory\n"); return -1; }
    for (size_t u = 0; u < v->ucurves; u++) ps->sigma[u] = R->res->lines[first + u].rec.sigma;
    if (R->with_params) {
        ps->param = (uint8_t *)malloc(v->ucurves);
        if (!ps->param) { fprintf(stderr, "out of memory\n"); return -1; }
        for (size_t u = 0; u < v->ucurves; u++) ps->param[u] = (uint8_t)R->res->lines[first + u].param;
    }
    return pack_residues(&cfg, R->res->lines + first, v->ucurves, 0, v->ucurves, ps->rx, ps->rz);
}

/* the passes of a run, in order, on one or two sets of contexts: batches_per_pass reference batches each; 2 at once when
 * memory runs out */
static int run_passes(run_t *R, gecm_ctx *ctx[2][MAX_GPUS], int gpus, int slots, size_t batches_per_pass)
{
    static pass_t pass[2];
    const size_t npasses = (R->nbatches + batches_per_pass - 1) / batches_per_pass;
    for (size_t pi = 0; pi < npasses; pi++) {
        const int s = (int)(pi % (size_t)slots);
        pass_t *ps = &pass[s];
        pass_join(ps);                            /* the pass before the last one, when there are two slots */
        pthread_mutex_lock(&R->mu);
        const int stop = R->found_pass != (size_t)-1 || R->failed;
        pthread_mutex_unlock(&R->mu);
        if (stop) break;
        view_t *v = &ps->v;
        ps->run = R;
        v->run = R;
        ps->index = pi;
        ps->live = slots == 1;
        v->b0 = pi * batches_per_pass;
        v->nb = R->nbatches - v->b0 < batches_per_pass ? R->nbatches - v->b0 : batches_per_pass;
        v->ucurves = v->nb * R->ub;
        ps->sigma = (uint64_t *)malloc(v->ucurves * sizeof(uint64_t));
        v->ck = (ck_t *)calloc((size_t)R->nranges + 1, sizeof(ck_t));
        if (!ps->sigma || !v->ck) { fprintf(stderr, "out of memory\n"); return 2; }
        if (R->res && resume_pass_input(ps, ctx[s][0])) return 2;
        for (size_t u = 0; u < v->ucurves && !R->res; u++) {
            /* fixed sigma: lane i of every thread of batch b runs sigma + 8 b + i (main.c:761, ecm.c:1187) */
            if (R->fixed_sigma) ps->sigma[u] = R->sigma0 + VECLEN * v->b0 + u;
            else if (R->fresh && R->fresh_param) ps->sigma[u] = 2 + lcg_rand(&R->lcg) % 0xfffffffeULL;   /* -p 1, -p 3: [2, 2^32) */
            else do { ps->sigma[u] = lcg_rand(&R->lcg); } while (ps->sigma[u] < 6);   /* ecm.c:1564-1570 */
        }
        if (R->fresh) {
            ps->param = (uint8_t *)malloc(v->ucurves);
            if (!ps->param) { fprintf(stderr, "out of memory\n"); return 2; }
            memset(ps->param, R->fresh_param, v->ucurves);
        }
        /* host-side split: GPU g owns distinct curves [n*g/G, n*(g+1)/G) of this pass */
        v->nparts = gpus;
        for (int g = 0; g < gpus; g++) {
            const size_t lo = v->ucurves * (size_t)g / (size_t)gpus, hi = v->ucurves * (size_t)(g + 1) / (size_t)gpus;
            v->part[g] = (part_t){ctx[s][g], ps->sigma + lo, hi - lo, lo, 0};
            ps->jobs[g].gpu = g;
            ps->jobs[g].part = &v->part[g];
            ps->jobs[g].rx = ps->rx;                  /* -r runs on one context: its part is the pass */
            ps->jobs[g].rz = ps->rz;
            ps->jobs[g].b1_done = R->s1_complete ? R->B1 : 0;
            ps->jobs[g].param = ps->param ? ps->param + lo : NULL;
        }
        ps->threaded = pthread_create(&ps->th, NULL, pass_run, ps) == 0;
        if (!ps->threaded) pass_run(ps);
    }
    for (int s = 0; s < 2; s++) pass_join(&pass[s]);
    return 0;
}

/* Reference batches per pass: as many as fit FULL_BATCH distinct curves per GPU — or what the device's memory takes
 * (the stage-2 table of 1024-bit curves is 1.1 MB per curve: 149 GB for a full batch).  GECM_PASS_CURVES (distinct
 * curves per pass over all GPUs) overrides it for tests.  *mem_free: what the device reports free (0: unknown);
 * *budget: the part of it one context may fill. */
static size_t pass_batches(const run_t *R, gecm_ctx *c, int gpus, int per_gpu, uint64_t *mem_free, uint64_t *budget)
{
    uint64_t mem_total = 0;
    *mem_free = 0;
    (void)gecm_device_memory(c, mem_free, &mem_total);
    *budget = *mem_free / 10 * 9 / (uint64_t)per_gpu;
    size_t fit = FULL_BATCH;
    while (fit > 64 && *mem_free && gecm_batch_bytes(c, fit, R->do_stage2, R->B1, 0, 0) > *budget) fit = fit / 2 / 64 * 64;
    if (fit < 64) fit = 64;
    const size_t cap = env_count("GECM_PASS_CURVES") ? (size_t)env_count("GECM_PASS_CURVES") : fit * (size_t)gpus;
    return cap / R->ub ? cap / R->ub : 1;
}

/* what the passes of a run share, before the first one starts: the locks, and the first prime range of stage 2 */
static void run_begin(run_t *R)
{
    pthread_mutex_init(&R->fr.mu, NULL);
    pthread_cond_init(&R->fr.cv, NULL);
    pthread_mutex_init(&R->mu, NULL);
    pthread_cond_init(&R->cv, NULL);
    R->fr.lo = R->B1;
    R->fr.hi = R->B1 + PRIME_RANGE < R->B2 ? R->B1 + PRIME_RANGE : R->B2;
    R->fr.D = gecm_s2_default_D(R->B1);
    R->fr.U = GECM_S2_DEFAULT_U;
    R->found_pass = (size_t)-1;
}

/* one input, the reference's command line: avx-ecm input curves B1 [threads] [B2] [sigma] */
static int run_single(int argc, char **argv)
{
    if (argc < 4) {
        printf("usage: avx-ecm $input $numcurves $B1 [$threads] [$B2] [$sigma]\n");   /* main.c:382 */
        return 1;
    }
    static run_t R;
    memset(&R, 0, sizeof R);
    R.t_start = now();
    printf("starting process %d\n", (int)getpid());                               /* main.c:391 */
    /* main.c:393-457: evaluate the expression, recognise Cunningham-type inputs, strip algebraic factors */
    static char ndec[MPL_MAXL * 10 + 16], prep_log[65536];
    gecm_input_info inf;
    if (gecm_prepare_input(argv[1], GECM_CLI_DIGITBITS, ndec, sizeof ndec, &inf, prep_log, sizeof prep_log)) {
        fputs(prep_log, stdout);
        printf("input must evaluate to an odd integer >= 3 (operators + - * / %% ^ ! # fib() luc())\n");
        return 1;
    }
    if (parse_run(&R, argc - 2, argv + 2)) return 1;
    int gpus = gecm_device_count();
    if (gpus < 1) { fprintf(stderr, "no HIP device visible\n"); return 2; }
    if (env_count("GECM_GPUS") && env_count("GECM_GPUS") < gpus) gpus = (int)env_count("GECM_GPUS");
    /* GECM_CONTEXTS_PER_GPU=k (rehearsal knob): k contexts, each with its host thread, on every device used — the
     * multi-context path of this driver on a box with one GPU.  Nothing is gained by it. */
    const int per_gpu = env_count("GECM_CONTEXTS_PER_GPU") > 1 ? (int)env_count("GECM_CONTEXTS_PER_GPU") : 1;
    const int devices = gpus;
    gpus *= per_gpu;
    if (gpus > MAX_GPUS) gpus = MAX_GPUS;
    R.gpus = gpus;
    R.nranges = gecm_stage1_ranges(R.B1);

    fputs(prep_log, stdout);          /* "gen: ...", "removing algebraic ...", "commencing parallel ecm on ..." */
    R.rd = (gecm_stage1_range_desc *)calloc((size_t)R.nranges, sizeof *R.rd);
    if (!R.rd) { fprintf(stderr, "out of memory\n"); return 2; }
    pthread_t rd_thread;
    const int rd_pending = pthread_create(&rd_thread, NULL, describe_ranges, &R) == 0;
    if (!rd_pending) describe_ranges(&R);
    /* Special-form inputs for which the reference leaves REDC (main.c:505-527, 642-684): it then works modulo
     * Mw = 2^k - 1, 2^k + 1 or 2^k - c throughout, curve construction included, and keeps the number given for the "N="
     * of its files and for its factor checks (ecm.c:1111-1118).  Same here: the contexts are made on Mw and report
     * against N (gecm_set_report_modulus); the files come out as the reference's, byte for byte. */
    static char mwdec[MPL_MAXL * 10 + 16];
    const char *modulus = ndec, *report = NULL;
    if (inf.ref_special_reduction) {
        mpl_t mw, t;
        mpl_set_u64(&mw, 1);
        mpl_shl(&mw, &mw, (unsigned)inf.k);
        if (inf.form < 0) { mpl_set_u64(&t, 1); mpl_add(&mw, &mw, &t); }
        else { mpl_set_u64(&t, inf.form > 1 ? (uint64_t)inf.c : 1); mpl_sub(&mw, &mw, &t); }
        mpl_get_dec(mwdec, &mw);
        modulus = mwdec;
        report = ndec;
    }
    static gecm_ctx *ctx[2][MAX_GPUS];
    if (make_contexts(ctx[0], gpus, devices, modulus, report, 1)) return 2;
    /* a number above the ordinary contexts' limit: stage 1 and its files as for any input, no stage 2 */
    const int wide = gecm_is_wide(ctx[0][0]);
    const int skipped_stage2 = wide && R.do_stage2;
    if (skipped_stage2) { R.do_stage2 = 0; R.B2 = R.B1; }
    uint64_t mem_free, budget;
    const size_t batches_per_pass = pass_batches(&R, ctx[0][0], gpus, per_gpu, &mem_free, &budget);
    const size_t npasses = (R.nbatches + batches_per_pass - 1) / batches_per_pass;
    /* two sets of contexts when there is more than one pass to overlap (one prime range only: with several, a pass
     * takes minutes to hours and its checkpoints are written as it goes) — and when two passes' worth of device memory
     * is there: a full pass that needs more than 45 % of it stays alone on its GPU */
    const size_t pass_curves_per_gpu = (batches_per_pass * R.ub + (size_t)gpus - 1) / (size_t)gpus;
    const int room = !mem_free || 2 * gecm_batch_bytes(ctx[0][0], pass_curves_per_gpu, R.do_stage2, R.B1, 0, 0) <= budget;
    /* (B1 in (99999989, 1e8] is one range WITH a checkpoint, ecm.c:1237: checkpoint.txt is appended to inside a pass's
     * turn on the GPU and put in order when the pass is written, which two passes in flight would do to each other) */
    const int slots = (npasses > 1 && R.nranges == 1 && R.B1 <= 99999989ULL && room && !getenv("GECM_NO_PIPELINE")) ? 2 : 1;
    if (slots > 1 && make_contexts(ctx[1], gpus, devices, modulus, report, 1)) return 2;
    gecm_config cfg;
    gecm_get_config(ctx[0][0], &cfg);
    char devname[256];
    gecm_device_name(ctx[0][0], devname, sizeof devname);
    /* main.c:529-533, verbatim: DIGITBITS and VECLEN describe the vector format at the boundary (curves come in
     * groups of 8, limbs of 52 bits); the device's own numbers follow on a line of their own.  For a special-form run
     * the "input size" is k, the size of 2^k -/+ c (main.c:465-483 on size_n = k). */
    printf("ECM has been configured with DIGITBITS = %d, VECLEN = %d, GMP_LIMB_BITS = %d\n", cfg.digitbits, VECLEN, 64);
    printf("Choosing MAXBITS = %d, NWORDS = %d, NBLOCKS = %d based on input size %d\n", cfg.maxbits, cfg.nwords,
           cfg.nwords / 4, inf.ref_special_reduction ? inf.k : cfg.nbits);
    printf("%s: %d GPU(s) [%s], residues of %d limbs x 28 bits on the device\n", gecm_version(), gpus, devname,
           cfg.dev_limbs);
    if (argc > 6) printf("starting with sigma = %lu\n", (unsigned long)R.sigma0);  /* main.c:558 */
    printf("Input has %d bits, using %d threads (%d curves/thread)\n", inf.ref_special_reduction ? inf.nbits : cfg.nbits,
           R.threads, (int)R.per_thread);                                          /* main.c:591-592 */
    printf("Processing in batches of %u primes\n", 100000000u);                   /* main.c:593 */
    if (inf.ref_special_reduction) {                                               /* main.c:644-670 */
        if (inf.form > 1) printf("Using special pseudo-Mersenne mod for factor of: 2^%d-%d\n", inf.k, inf.form);
        else printf("Using special Mersenne mod for factor of: 2^%d%c1\n", inf.k, inf.form > 0 ? '-' : '+');
        int fk = 0, fl = 0;
        if (gecm_get_special_form(ctx[0][0], &fk, &fl) >= 1)
            printf("(batches that fill the GPU multiply modulo it with a special reduction, %d limbs; smaller ones by REDC)\n", fl);
    }
    if (skipped_stage2)
        printf("stage 2 is not run on this number (%d bits, a wide context of %d device limbs does stage 1 only): continue "
               "with ecm -resume save_b1.txt\n", cfg.nbits, cfg.dev_limbs);
    printf("Initialization took %1.4f seconds.\n", now() - R.t_start);             /* main.c:776 */
    fflush(stdout);

    run_begin(&R);

    if (rd_pending) pthread_join(rd_thread, NULL);
    if (R.rd_rc) { fprintf(stderr, "%s\n", R.rd_err); return 2; }
    if (R.nranges == 1)                                                            /* ecm.c:1139-1146 */
        printf("Found %lu primes in range [%lu : %lu]\n", (unsigned long)R.rd[0].nprimes, (unsigned long)R.rd[0].lo, (unsigned long)R.rd[0].hi);
    if (run_passes(&R, ctx, gpus, slots, batches_per_pass)) return 2;
    if (R.fr.valid) gecm_pairmap_release(&R.fr.pm);
    for (int s = 0; s < slots; s++)
        for (int g = 0; g < gpus; g++) gecm_destroy(ctx[s][g]);
    printf("Process took %1.4f seconds.\n", now() - R.t_start);                    /* ecm.c:1538 */
    free(R.rd);
    return R.failed ? 2 : 0;
}

/* ---- avx-ecm -f FILE curves B1 [threads] [B2] [sigma]: a list of inputs ----------------------------------------------
 * The files come out as running `avx-ecm <input> curves B1 threads B2 sigma` for every line in turn, in the same
 * directory: per input, save_b1.txt up to and including its first batch with a factor, and that batch's factor lines
 * in ecm_results.txt.  Consecutive inputs run together in multi-modulus passes (include/gecm.h gecm_create_multi) of up
 * to FULL_BATCH curves on the first GPU; an input the reference works on modulo 2^k -/+ c, one that does not fit a
 * pass, and every input of a run with a checkpoint (B1 above 99999989) go through the one-input path, in their place. */
typedef struct {
    char ndec[MPL_MAXL * 10 + 16];
    char log[65536];
} input_t;

/* One multi-modulus pass: input i has count[i] curves, the caller's curves first[i] .. of sigma / which; rl != NULL
 * (-r): the curves start from the lines' residues, stage 1 complete.  Every input is written as the one-input path
 * writes it: a pass of all its batches on one context.  Returns 0, or 2 after a device or library error. */
static int multi_run(const char **ns, const char *const *logs, size_t n, run_t *R, const uint64_t *sigma, const uint32_t *which,
                     const size_t *first, const size_t *count, size_t total, const rline_t *rl, int packing)
{
    gecm_ctx *mc = NULL;
    void *rx = NULL, *rz = NULL;
    int rc = gecm_create_multi(&mc, 0, ns, n, GECM_CLI_DIGITBITS);
    if (rc == 0) rc = set_curve_build(mc);
    if (rc == 0) rc = gecm_set_multi_packing(mc, packing);
    if (rc == 0) rc = gecm_set_stage2_subseq(mc, cli_multi_subseq());
    if (rc == 0) rc = gecm_set_multi_rows(mc, cli_multi_rows());
    if (rc == 0 && rl) {
        gecm_config cfg;
        gecm_get_config(mc, &cfg);
        const size_t bytes = total * (size_t)cfg.nwords * (cfg.digitbits == 52 ? 8 : 4);
        rx = malloc(bytes);
        rz = malloc(bytes);
        if (!rx || !rz) { fprintf(stderr, "out of memory\n"); exit(2); }
        pack_residues(&cfg, rl, total, 0, total, rx, rz);
        if (R->with_params) {                       /* -g: every curve by its line's parametrisation */
            uint8_t *param = (uint8_t *)malloc(total);
            if (!param) { fprintf(stderr, "out of memory\n"); exit(2); }
            for (size_t u = 0; u < total; u++) param[u] = (uint8_t)rl[u].param;
            rc = gecm_set_next_params(mc, param, total);
            free(param);
        }
        if (rc) rc = 1;
        else if (R->extend) /* -x: one segment from the lines' common bound to B1, then the standard lines' normalisation */
            rc = gecm_resume_points_multi(mc, sigma, which, rx, rz, total, 0) < 0 || gecm_stage1_extend(mc, R->ext_from, R->B1) ||
                 gecm_sync(mc) || gecm_normalize_points(mc) < 0 || gecm_scan_factors(mc, 1, NULL) < 0;
        else
            rc = gecm_resume_points_multi(mc, sigma, which, rx, rz, total, R->B1) < 0 || gecm_scan_factors(mc, 1, NULL) < 0;
    } else if (rc == 0) {
        rc = gecm_build_curves_multi(mc, sigma, which, total) < 0;
        if (rc == 0) rc = gecm_stage1(mc, R->B1) || gecm_sync(mc) || gecm_scan_factors(mc, 1, NULL) < 0;
    }
    if (rc == 0 && R->do_stage2) rc = gecm_stage2(mc, R->B2, 0, 0) || gecm_scan_factors(mc, 2, NULL) < 0;
    if (rc) fprintf(stderr, "%s\n", gecm_last_error());
    for (size_t i = 0; i < n && !rc; i++) {
        const view_t v = {.run = R, .nb = (count[i] + R->ub - 1) / R->ub, .ucurves = count[i], .nparts = 1,
                          .part = {{mc, sigma, count[i], 0, first[i]}}};
        output_t o;
        output_settle(&v, &o);
        rc = output_format(&v, &o);
        if (!rc) output_write(&v, &o, logs ? logs[i] : NULL, NULL);   /* log: "gen: ...", "commencing parallel ecm on ..." */
        output_release(&v, &o);
    }
    if (!rc) {
        char s2[48] = "";
        if (R->do_stage2) snprintf(s2, sizeof s2, " and stage 2 (K = %d)", gecm_get_stage2_subseq(mc, NULL));
        /* (stage 1 in the row layout is named; without GECM_MULTI_ROWS the line is what it was) */
        printf("multi-modulus pass: %zu inputs, %zu curves%s, %s-packed, %s%s%s, %1.4f seconds of kernels after stage 1\n", n,
               rl ? total : count[0], rl ? " in all" : " each", gecm_get_multi_packing(mc) == GECM_PACK_LANE ? "lane" : "wave",
               !rl ? "stage 1" : R->extend ? "stage 1 extended" : "resumed after stage 1",
               gecm_get_lanes_per_curve(mc) == 32 ? " with 32 lanes per curve" : "", s2, gecm_last_kernel_ms(mc) / 1000.0);
    }
    gecm_destroy(mc);
    free(rx); free(rz);
    return rc ? 2 : 0;
}

/* the inputs of one multi-modulus pass of -f, ucurves curves each */
static int multi_pass(input_t **in, size_t n, run_t *R, size_t ucurves, int packing)
{
    const char **ns = (const char **)malloc(n * sizeof *ns), **logs = (const char **)malloc(n * sizeof *logs);
    uint64_t *sigma = (uint64_t *)malloc(n * ucurves * sizeof *sigma);
    uint32_t *which = (uint32_t *)malloc(n * ucurves * sizeof *which);
    size_t *first = (size_t *)malloc(2 * n * sizeof *first), *count = first ? first + n : NULL;
    if (!ns || !logs || !sigma || !which || !first) { fprintf(stderr, "out of memory\n"); exit(2); }
    for (size_t i = 0; i < n; i++) {
        ns[i] = in[i]->ndec;
        logs[i] = in[i]->log;
        first[i] = i * ucurves;
        count[i] = ucurves;
        for (size_t u = 0; u < ucurves; u++) {
            uint64_t *sg = &sigma[i * ucurves + u];
            if (R->fixed_sigma) *sg = R->sigma0 + u;                                  /* as run_single's pass 0 */
            else do { *sg = lcg_rand(&R->lcg); } while (*sg < 6);
            which[i * ucurves + u] = (uint32_t)i;
        }
    }
    const int rc = multi_run(ns, logs, n, R, sigma, which, first, count, n * ucurves, NULL, packing);
    free(ns); free(logs); free(sigma); free(which); free(first);
    return rc;
}

static int run_file(int argc, char **argv)
{
    static const char *usage = "usage: avx-ecm -f $file $numcurves $B1 [$threads] [$B2] [$sigma]\n"
                               "       (one input expression per line; blank lines and lines starting with # are skipped)\n";
    if (argc < 5) { printf("%s", usage); return 1; }
    const int packing = cli_packing();
    if (packing < 0 || cli_multi_subseq() == 1 || cli_multi_rows() == 2) return 1;
    FILE *f = fopen(argv[2], "r");
    if (!f) { printf("cannot read %s\n%s", argv[2], usage); return 1; }
    size_t ninputs = 0, cap_in = 0;
    char **exprs = NULL;
    static char buf[1 << 16];
    while (fgets(buf, sizeof buf, f)) {
        char *p = buf, *e;
        while (*p == ' ' || *p == '\t') p++;
        e = p + strlen(p);
        while (e > p && (e[-1] == '\n' || e[-1] == '\r' || e[-1] == ' ' || e[-1] == '\t')) *--e = 0;
        if (!*p || *p == '#') continue;
        if (ninputs == cap_in) {
            cap_in = cap_in ? 2 * cap_in : 64;
            exprs = (char **)realloc(exprs, cap_in * sizeof *exprs);
            if (!exprs) { fprintf(stderr, "out of memory\n"); return 2; }
        }
        exprs[ninputs++] = strdup(p);
    }
    fclose(f);
    if (!ninputs) { printf("%s holds no input\n%s", argv[2], usage); return 1; }

    static run_t R;
    memset(&R, 0, sizeof R);
    R.t_start = now();
    if (parse_run(&R, argc - 3, argv + 3)) return 1;
    const size_t ucurves = R.nbatches * R.ub, padded = (ucurves + 63) / 64 * 64;
    if (gecm_device_count() < 1) { fprintf(stderr, "no HIP device visible\n"); return 2; }
    printf("starting process %d: %zu inputs from %s\n", (int)getpid(), ninputs, argv[2]);
    const size_t cap = env_count("GECM_PASS_CURVES") ? (size_t)env_count("GECM_PASS_CURVES") : FULL_BATCH;
    const int multi_ok = R.B1 <= 99999989ULL && padded <= cap;    /* one prime range, no checkpoint; one input fits */
    int pend_packing = GECM_PACK_WAVE;                                 /* of the pending pass */

    /* the one-input path's argument list for input i: argv with "-f FILE" replaced by the input */
    char *sargv[8];
    const int sargc = argc - 1;
    sargv[0] = argv[0];
    for (int a = 3; a < argc && a < 8; a++) sargv[a - 1] = argv[a];
    input_t **pend = (input_t **)calloc(ninputs, sizeof *pend);
    if (!pend) { fprintf(stderr, "out of memory\n"); return 2; }
    size_t npend = 0;
    int rc = 0;
    for (size_t i = 0; i <= ninputs && rc != 2; i++) {
        input_t *in = NULL;
        int alone = 1, in_packing = GECM_PACK_WAVE;
        if (i < ninputs && multi_ok) {
            in = (input_t *)calloc(1, sizeof *in);
            if (!in) { fprintf(stderr, "out of memory\n"); return 2; }
            gecm_input_info inf;
            alone = gecm_prepare_input(exprs[i], GECM_CLI_DIGITBITS, in->ndec, sizeof in->ndec, &inf, in->log, sizeof in->log) ||
                    inf.ref_special_reduction;
            if (!alone && packing == GECM_PACK_LANE && fits_lane_packing(inf.nbits)) in_packing = GECM_PACK_LANE;
        }
        /* the pending pass goes first when this input cannot join it */
        if (npend && (i == ninputs || alone || in_packing != pend_packing ||
                      pass_positions(npend + 1, ucurves, pend_packing) > cap)) {
            rc = multi_pass(pend, npend, &R, ucurves, pend_packing);
            for (size_t k = 0; k < npend; k++) free(pend[k]);
            npend = 0;
            if (rc == 2) break;
        }
        if (i == ninputs) break;
        if (!alone) {
            if (!npend) pend_packing = in_packing;
            pend[npend++] = in;
            continue;
        }
        free(in);
        sargv[1] = exprs[i];
        const int r1 = run_single(sargc, sargv);
        if (r1 > rc) rc = r1;
    }
    for (size_t i = 0; i < ninputs; i++) free(exprs[i]);
    free(exprs);
    free(pend);
    printf("Process took %1.4f seconds.\n", now() - R.t_start);
    return rc;
}

/* ---- avx-ecm -r FILE B1 [B2]: go on from save_b1.txt or checkpoint.txt lines ------------------------------------------
 * FILE holds resume lines (gecm_parse_resume_line: ours, the reference's, GMP-ECM -save).  Consecutive lines on one N are
 * a group, its lines the curves of a one-thread run in order: line k is "curve k, thread 0, vec k mod VECLEN", and the
 * run stops after the first VECLEN lines with a factor among them, as every run here does.  The B1 field says where the
 * lines stand (gecm_stage1_resume_range): checkpoint lines of a run to B1 go through the remaining prime ranges
 * (checkpoint.txt after each, as a run from the start), then save_b1.txt, then stage 2 if B2 > B1; save lines (field =
 * B1) go to stage 2 alone and save_b1.txt is left as it is.  One N: the one-input path, on the first GPU.  Several N:
 * multi-modulus passes packed as -f packs its inputs — stage 2 only, a multi pass stays within one prime range — and a
 * group too large for one takes the one-input path.  A number's lines stand together: the same N in two places, with
 * another between, is refused.  Everything is checked before anything runs or is written.
 *
 * avx-ecm -x FILE B1 [B2] reads the same files and takes their lines from the standard bound they are complete to
 * (gecm_resume_line_std_bound: B1 - 1 for a reference line within one prime range, the field itself for a standard line)
 * on to B1 with the standard multiplier, extension segment by segment.  After every segment the curves are
 * normalised; checkpoint.txt gets the standard lines at every segment's end but the last, save_b1.txt those at B1; then
 * stage 2 if B2 > B1.  Grouping, numbering and the stopping rule are -r's.  Refused on top of what -r refuses: lines of one
 * N complete to different bounds, a bound above B1, a reference line above one prime range, and several N when the
 * extension takes more than one segment. */
static const char *resume_usage = "usage: avx-ecm -r $file $B1 [$B2]\n"
                                  "       (resume lines as in save_b1.txt / checkpoint.txt, or of a GMP-ECM -save file)\n";

static const char *extend_usage = "usage: avx-ecm -x $file $B1 [$B2]\n"
                                  "       (resume lines as for -r, complete to any bound up to $B1: stage 1 is extended to $B1)\n";

/* -g before either: the file may hold lines of GMP-ECM's PARAM 1 and PARAM 3 next to PARAM 0, mixed or not
 * (DESIGN.md §19); every line written carries its curve's PARAM=.  Nothing else differs. */
static const char *gmp_resume_usage = "usage: avx-ecm -g -r $file $B1 [$B2]\n"
                                      "       (-r with resume lines of PARAM 0, 1 and 3 accepted, as GMP-ECM 7 and ecm -gpu write them)\n";
static const char *gmp_extend_usage = "usage: avx-ecm -g -x $file $B1 [$B2]\n"
                                      "       (-x with resume lines of PARAM 0, 1 and 3 accepted, as GMP-ECM 7 and ecm -gpu write them)\n";

typedef struct {
    size_t first, count;       /* lines of the file */
    uint32_t range;            /* the range stage 1 goes on with; the range count: complete */
    uint64_t from;             /* -x: the standard bound the lines are complete to (gecm_resume_line_std_bound) */
    char ndec[MPL_MAXL * 10 + 16];
} rgroup_t;

/* one group on the one-input path; extend: -x */
static int resume_single(const rgroup_t *g, const rline_t *lines, char **rargv, int rargc, int extend, int gmp)
{
    static run_t R;
    memset(&R, 0, sizeof R);
    R.t_start = now();
    if (parse_run(&R, rargc, rargv)) return 1;
    const resume_t res = {lines + g->first, g->count};
    R.res = &res;
    R.gpus = 1;
    R.nranges = extend ? gecm_stage1_extend_segments(g->from, R.B1) : gecm_stage1_ranges(R.B1);
    R.first_range = extend ? 0 : (int)g->range;
    R.s1_complete = R.first_range >= R.nranges;
    R.extend = extend;
    R.ext_from = g->from;
    R.with_params = gmp;
    R.rd = (gecm_stage1_range_desc *)calloc((size_t)R.nranges, sizeof *R.rd);
    if (!R.rd) { fprintf(stderr, "out of memory\n"); return 2; }
    for (int r = R.first_range; r < R.nranges && !R.rd_rc && !extend; r++)
        R.rd_rc = gecm_stage1_describe_range(R.B1, R.B2, (uint32_t)r, &R.rd[r]);
    if (R.rd_rc) { fprintf(stderr, "%s\n", gecm_last_error()); return 2; }
    static gecm_ctx *ctx[2][MAX_GPUS];
    if (make_contexts(ctx[0], 1, 1, g->ndec, NULL, 0)) return 2;
    uint64_t mem_free, budget;
    const size_t batches_per_pass = pass_batches(&R, ctx[0][0], 1, 1, &mem_free, &budget);
    if (extend) printf("extending %zu curves on N = %s from B1 = %lu to %lu\n", g->count, g->ndec, (unsigned long)g->from, (unsigned long)R.B1);
    else printf("resuming %zu curves on N = %s %s\n", g->count, g->ndec, R.s1_complete ? "after stage 1" : "inside stage 1");
    run_begin(&R);
    if (run_passes(&R, ctx, 1, 1, batches_per_pass)) return 2;
    if (R.fr.valid) gecm_pairmap_release(&R.fr.pm);
    gecm_destroy(ctx[0][0]);
    free(R.rd);
    return R.failed ? 2 : 0;
}

/* gmp: -g before -r or -x, lines of PARAM 0, 1 and 3 are read (gecm_parse_resume_line_param) */
static int run_resume(int argc, char **argv, int extend, int gmp)
{
    const char *usage = gmp ? (extend ? gmp_extend_usage : gmp_resume_usage) : extend ? extend_usage : resume_usage;
    if (argc < 4) { printf("%s", usage); return 1; }
    const int packing = cli_packing();
    if (packing < 0 || cli_multi_subseq() == 1 || cli_multi_rows() == 2) return 1;
    FILE *f = fopen(argv[2], "r");
    if (!f) { printf("cannot read %s\n%s", argv[2], usage); return 1; }
    /* the run's arguments through the one parser: curves B1 threads [B2], one thread, the curve count per group */
    char ncurves[32] = "1", one[] = "1";
    char *rargv[4] = {ncurves, argv[3], one, argc > 4 ? argv[4] : NULL};
    const int rargc = argc > 4 ? 4 : 3;
    static run_t R0;
    memset(&R0, 0, sizeof R0);
    if (parse_run(&R0, rargc, rargv)) { fclose(f); return 1; }

    rline_t *lines = NULL;
    rgroup_t *groups = NULL;
    size_t nlines = 0, cap_lines = 0, ngroups = 0, cap_groups = 0, lineno = 0;
    char *text = NULL, *pending = NULL;           /* pending: the text of a line that is not counted in nlines yet */
    size_t text_cap = 0;
    int bad = 0, oom = 0;
    mpl_t n_cur, n, v;
    while (!bad && !oom && getline(&text, &text_cap, f) > 0) {
        lineno++;
        gecm_resume_rec rec;
        int param = 0;
        const int rc = gmp ? gecm_parse_resume_line_param(text, &rec, &param) : gecm_parse_resume_line(text, &rec);
        if (rc == 1) continue;
        if (rc) {
            const int other = !gmp && gecm_parse_resume_line_param(text, &rec, &param) == 0;   /* (the first text is gone then) */
            if (other) printf("%s line %zu: field PARAM = %d: only PARAM 0 (Suyama's sigma) curves are resumed without -g "
                              "(avx-ecm -g -%c reads PARAM 1 and 3)\n", argv[2], lineno, param, extend ? 'x' : 'r');
            else printf("%s line %zu: %s\n", argv[2], lineno, gecm_last_error());
            bad = 1;
            break;
        }
        if (nlines == cap_lines) {
            cap_lines = cap_lines ? 2 * cap_lines : 1024;
            rline_t *more = (rline_t *)realloc(lines, cap_lines * sizeof *lines);
            if (!more) { oom = 1; break; }
            lines = more;
        }
        rline_t *l = &lines[nlines];
        l->text = pending = strdup(text);
        l->param = 0;
        if (!l->text || (gmp ? gecm_parse_resume_line_param(l->text, &l->rec, &l->param) : gecm_parse_resume_line(l->text, &l->rec))) { oom = 1; break; }   /* (it parsed a moment ago) */
        rnum(&n, &l->rec.n);
        if (!ngroups || mpl_cmp(&n, &n_cur) != 0) {
            if (ngroups == cap_groups) {
                cap_groups = cap_groups ? 2 * cap_groups : 16;
                rgroup_t *more = (rgroup_t *)realloc(groups, cap_groups * sizeof *groups);
                if (!more) { oom = 1; break; }
                groups = more;
            }
            if (!mpl_is_odd(&n) || mpl_cmp_u64(&n, 3) < 0) { printf("%s line %zu: field N must be an odd number >= 3\n", argv[2], lineno); bad = 1; break; }
            rgroup_t *g = &groups[ngroups];
            g->first = nlines;
            g->count = 0;
            mpl_get_dec(g->ndec, &n);
            /* a number's lines stand together: the same N further down would be a second modulus of one multi pass */
            for (size_t k = 0; k < ngroups && !bad; k++)
                if (strcmp(groups[k].ndec, g->ndec) == 0) {
                    printf("%s line %zu: lines on this N stand further up as well (line %zu of the resume lines on), with another "
                           "N between: put the lines on one number together\n", argv[2], lineno, groups[k].first + 1);
                    bad = 1;
                }
            if (bad) break;
            ngroups++;
            n_cur = n;
            g->range = 0;
            g->from = 0;
            if (extend) {
                /* the standard bound of the lines: a reference line above one prime range has none, and none may lie above B1 */
                if (gmp ? gecm_resume_line_std_bound_param(l->text, &g->from) : gecm_resume_line_std_bound(l->text, &g->from)) { printf("%s line %zu: %s\n", argv[2], lineno, gecm_last_error()); bad = 1; break; }
                if (g->from < 1 || g->from > R0.B1) {
                    printf("%s line %zu: the line is complete to B1 = %lu, which is not in [1, %lu]: stage 1 is extended upwards only\n",
                           argv[2], lineno, (unsigned long)g->from, (unsigned long)R0.B1);
                    bad = 1;
                    break;
                }
            }
            /* what the B1 field says about a run to B1: the one refusal that names what is not offered */
            else if (gecm_stage1_resume_range(R0.B1, l->rec.b1, &g->range)) {
                printf("%s line %zu: B1 field %lu is neither B1 = %lu nor a checkpoint of a run to it: stage 1 is extended from "
                       "no other B1 (the reference's stage 1 is not a product of prime powers cut at that prime)\n",
                       argv[2], lineno, (unsigned long)l->rec.b1, (unsigned long)R0.B1);
                bad = 1;
                break;
            }
        }
        rgroup_t *g = &groups[ngroups - 1];
        uint64_t from_l = 0;
        if (extend && ((gmp ? gecm_resume_line_std_bound_param(l->text, &from_l) : gecm_resume_line_std_bound(l->text, &from_l)) || from_l != g->from)) {
            printf("%s line %zu: the line is not complete to the bound %lu of the lines on this N before it\n", argv[2], lineno,
                   (unsigned long)g->from);
            bad = 1;
            break;
        }
        if (!extend && l->rec.b1 != lines[g->first].rec.b1) {
            printf("%s line %zu: B1 field %lu differs from the %lu of the lines on this N before it\n", argv[2], lineno,
                   (unsigned long)l->rec.b1, (unsigned long)lines[g->first].rec.b1);
            bad = 1;
            break;
        }
        for (int q = 0; q < 2 && !bad; q++) {
            rnum(&v, q ? &l->rec.z : &l->rec.x);
            if (mpl_cmp(&v, &n) >= 0) {
                printf("%s line %zu: %c is not below N.  The reference's special-form runs store residues modulo 2^k -/+ c next "
                       "to N=; such files are resumed through the library: a context on 2^k -/+ c plus gecm_set_report_modulus\n",
                       argv[2], lineno, q ? 'Z' : 'X');
                bad = 1;
            }
        }
        if (bad) break;
        g->count++;
        nlines++;
        pending = NULL;
    }
    fclose(f);
    free(text);
    free(pending);
    if (oom) { fprintf(stderr, "out of memory\n"); bad = 1; }
    const uint32_t nranges = (uint32_t)gecm_stage1_ranges(R0.B1);
    if (!bad && !nlines) { printf("%s holds no resume line\n%s", argv[2], usage); bad = 1; }
    for (size_t i = 0; i < ngroups && !bad && extend; i++)
        if (ngroups > 1 && gecm_stage1_extend_segments(groups[i].from, R0.B1) > 1) {
            printf("%s holds lines on %zu numbers and the extension from %lu to %lu takes several segments: several numbers are "
                   "extended within one segment only (a multi-modulus pass stays within one prime range); extend them one file "
                   "per number\n", argv[2], ngroups, (unsigned long)groups[i].from, (unsigned long)R0.B1);
            bad = 1;
        }
    for (size_t i = 0; i < ngroups && !bad && !extend; i++) {
        if (groups[i].range >= nranges && !R0.do_stage2) {
            printf("stage 1 of these lines is complete at B1 = %lu: nothing to do without B2 > B1\n%s", (unsigned long)R0.B1, resume_usage);
            bad = 1;
        } else if (groups[i].range < nranges && ngroups > 1) {
            printf("%s holds lines on %zu numbers with prime ranges of stage 1 left: several numbers are resumed after stage 1 "
                   "only (a multi-modulus pass stays within one prime range); resume them one file per number\n", argv[2], ngroups);
            bad = 1;
        }
    }
    int rc = oom ? 2 : bad ? 1 : 0;
    if (!bad && gecm_device_count() < 1) { fprintf(stderr, "no HIP device visible\n"); rc = 2; }
    if (rc == 0) {
        printf("starting process %d: %zu resume lines on %zu number(s) from %s\n", (int)getpid(), nlines, ngroups, argv[2]);
        const size_t cap = env_count("GECM_PASS_CURVES") ? (size_t)env_count("GECM_PASS_CURVES") : FULL_BATCH;
        R0.t_start = now();
        R0.s1_complete = !extend;                  /* the multi passes: stage 2 only; -x: one extension segment first */
        R0.extend = extend;
        R0.with_params = gmp;
        R0.nbatches = 0;
        size_t p0 = 0;                             /* the pending multi pass: groups p0 .. i */
        size_t *pcount = (size_t *)calloc(ngroups + 1, sizeof *pcount);   /* curves of the groups */
        if (!pcount) { fprintf(stderr, "out of memory\n"); rc = 2; }
        int pend_packing = GECM_PACK_WAVE;
        for (size_t i = 0; i <= ngroups && rc != 2 && pcount; i++) {
            const size_t pad_i = i < ngroups ? (groups[i].count + 63) / 64 * 64 : 0;
            const int alone = i < ngroups && (ngroups == 1 || pad_i > cap);
            int in_packing = GECM_PACK_WAVE;
            if (i < ngroups && !alone && packing == GECM_PACK_LANE) {
                static char nd[MPL_MAXL * 10 + 16], lg[65536];
                gecm_input_info inf;
                if (!gecm_prepare_input(groups[i].ndec, GECM_CLI_DIGITBITS, nd, sizeof nd, &inf, lg, sizeof lg) && fits_lane_packing(inf.nbits))
                    in_packing = GECM_PACK_LANE;
            }
            if (i < ngroups) pcount[i] = groups[i].count;
            /* (-x: the curves of a pass run one tape, so its groups are complete to one bound) */
            if (i > p0 && (i == ngroups || alone || in_packing != pend_packing || groups[i].from != groups[p0].from ||
                           gecm_multi_positions(pcount + p0, i + 1 - p0, pend_packing) > cap)) {
                R0.ext_from = groups[p0].from;
                const size_t n_in = i - p0, total = groups[i - 1].first + groups[i - 1].count - groups[p0].first;
                const char **ns = (const char **)malloc(n_in * sizeof *ns);
                uint64_t *sigma = (uint64_t *)malloc(total * sizeof *sigma);
                uint32_t *which = (uint32_t *)malloc(total * sizeof *which);
                size_t *first = (size_t *)malloc(2 * n_in * sizeof *first);
                if (!ns || !sigma || !which || !first) {
                    fprintf(stderr, "out of memory\n");
                    free(ns); free(sigma); free(which); free(first);
                    rc = 2;
                    break;
                }
                for (size_t k = 0; k < n_in; k++) {
                    const rgroup_t *g = &groups[p0 + k];
                    ns[k] = g->ndec;
                    first[k] = g->first - groups[p0].first;
                    first[n_in + k] = g->count;
                    for (size_t u = 0; u < g->count; u++) {
                        sigma[first[k] + u] = lines[g->first + u].rec.sigma;
                        which[first[k] + u] = (uint32_t)k;
                    }
                }
                const int r1 = multi_run(ns, NULL, n_in, &R0, sigma, which, first, first + n_in, total, lines + groups[p0].first,
                                         pend_packing);
                if (r1 > rc) rc = r1;
                free(ns); free(sigma); free(which); free(first);
                p0 = i;
            }
            if (i == ngroups || rc == 2) break;
            if (!alone) {
                if (i == p0) pend_packing = in_packing;
                continue;
            }
            snprintf(ncurves, sizeof ncurves, "%zu", groups[i].count);
            const int r1 = resume_single(&groups[i], lines, rargv, rargc, extend, gmp);
            if (r1 > rc) rc = r1;
            p0 = i + 1;
        }
        free(pcount);
        printf("Process took %1.4f seconds.\n", now() - R0.t_start);
    }
    for (size_t i = 0; i < nlines; i++) free(lines[i].text);
    free(lines);
    free(groups);
    return rc;
}

/* ---- avx-ecm -p PARAM input curves B1 [B2] [sigma]: a fresh run in standard mode ------------------------------------
 * Curves of GMP-ECM's parametrisation PARAM (0, 1 or 3) on the input as gecm_prepare_input leaves it —
 * the context is on N itself, without the reference's special-form folding — built and then taken through -x's own
 * path from the bound 1: extension segments, checkpoint.txt after every segment but the last, normalisation, standard
 * lines in save_b1.txt, stage 2 when B2 > B1 (left out: 100 B1), factors to ecm_results.txt.  With a sigma the curves are
 * sigma, sigma + 1, ... as ecm -gpu numbers them; without, sigmas come from the driver's generator, for PARAM 1 and 3
 * reduced into [2, 2^32).  One thread, the first GPU. */
static const char *param_usage = "usage: avx-ecm -p $param $input $numcurves $B1 [$B2] [$sigma]\n"
                                 "       (a fresh run with the standard stage-1 multiplier; $param: 0 = Suyama's sigma, 1 and 3 = GMP-ECM's\n"
                                 "        batch parametrisations d = sigma^2 / 2^64 and sigma / 2^32, start point (2 : 1))\n";

static int run_param(int argc, char **argv)
{
    if (argc < 6) { printf("%s", param_usage); return 1; }
    char *end = NULL;
    const long param = strtol(argv[2], &end, 10);
    if (!*argv[2] || *end || (param != GECM_PARAM_SUYAMA && param != GECM_PARAM_BATCH_SQUARE && param != GECM_PARAM_BATCH_32)) {
        printf("-p %s: the parametrisations offered are 0, 1 and 3 (PARAM 2 takes a point multiplication on another curve)\n%s",
               argv[2], param_usage);
        return 1;
    }
    static run_t R;
    memset(&R, 0, sizeof R);
    R.t_start = now();
    static char ndec[MPL_MAXL * 10 + 16], prep_log[65536];
    gecm_input_info inf;
    if (gecm_prepare_input(argv[3], GECM_CLI_DIGITBITS, ndec, sizeof ndec, &inf, prep_log, sizeof prep_log)) {
        fputs(prep_log, stdout);
        printf("input must evaluate to an odd integer >= 3 (operators + - * / %% ^ ! # fib() luc())\n");
        return 1;
    }
    /* the run's arguments through the one parser: curves B1 threads [B2] [sigma], one thread */
    char one[] = "1";
    char *rargv[5] = {argv[4], argv[5], one, argc > 6 ? argv[6] : NULL, argc > 7 ? argv[7] : NULL};
    if (parse_run(&R, argc > 7 ? 5 : argc > 6 ? 4 : 3, rargv)) return 1;
    const uint64_t last = R.sigma0 + R.nbatches * R.ub - 1;                       /* of sigma, sigma + 1, ... */
    if (R.fixed_sigma && (param == GECM_PARAM_SUYAMA ? R.sigma0 < 6 : last < R.sigma0 || (param == GECM_PARAM_BATCH_32 && last >> 32))) {
        printf("-p %ld: sigma %lu and the curves after it leave the parametrisation's range\n%s", param, (unsigned long)R.sigma0, param_usage);
        return 1;
    }
    if (gecm_device_count() < 1) { fprintf(stderr, "no HIP device visible\n"); return 2; }
    printf("starting process %d\n", (int)getpid());
    fputs(prep_log, stdout);
    R.gpus = 1;
    R.extend = 1;
    R.ext_from = 1;
    R.fresh = 1;
    R.fresh_param = (int)param;
    R.nranges = gecm_stage1_extend_segments(1, R.B1);
    R.rd = (gecm_stage1_range_desc *)calloc((size_t)R.nranges, sizeof *R.rd);
    if (!R.rd) { fprintf(stderr, "out of memory\n"); return 2; }
    static gecm_ctx *ctx[2][MAX_GPUS];
    if (make_contexts(ctx[0], 1, 1, ndec, NULL, 0)) return 2;
    uint64_t mem_free, budget;
    const size_t batches_per_pass = pass_batches(&R, ctx[0][0], 1, 1, &mem_free, &budget);
    printf("running %zu curves of PARAM %ld on N = %s in standard mode to B1 = %lu\n", R.nbatches * R.ub, param, ndec, (unsigned long)R.B1);
    run_begin(&R);
    if (run_passes(&R, ctx, 1, 1, batches_per_pass)) return 2;
    if (R.fr.valid) gecm_pairmap_release(&R.fr.pm);
    gecm_destroy(ctx[0][0]);
    free(R.rd);
    printf("Process took %1.4f seconds.\n", now() - R.t_start);
    return R.failed ? 2 : 0;
}


/* ---- avx-ecm -m pm1|pp1 ...: P-1 and P+1 stage 1 -------------------------------------------------------
 *     avx-ecm -m pm1|pp1 input B1 [x0]     one number; x0 decimal or 0x-hex, below the number
 *     avx-ecm -m pm1|pp1 -f FILE B1        every input of FILE (one expression per line, as -f reads it)
 *     avx-ecm -m pm1|pp1 -x FILE B1        the P-1 / P+1 lines of FILE (of the method named) on to B1
 * Seeds when none is given: P-1 x0 = 3; P+1 two residues per number, x0 = 2/7 mod N and 6/5 mod N, the customary pair; a
 * number for which 7 or 5 has no inverse reports that gcd as its factor and gets no residue for it.  A pass is one
 * context: a single-N one for one number, else a multi-modulus one, closed when it is full (FULL_BATCH positions, or
 * GECM_PASS_CURVES), when the next number falls on the other side of lane packing's 415-bit line under GECM_PACKING=lane,
 * and (-x) when the next number's lines are complete to another bound or differ in whether they name their seed.  A pass
 * goes through the extension segments from its bound to B1 one by one: checkpoint.txt gets the standard lines after every
 * segment but the last, save_b1.txt those at B1, then the factor scan, and every factor one line in ecm_results.txt and on
 * stdout.  A trailing B2 argument is refused; `-b B2` right after the method (B2 > B1, else status 1 and nothing written)
 * adds stage 2 to every pass: gecm_stage2(ctx, B2, 0, 0) on the pass's residues, GECM_MULTI_SUBSEQ honoured
 * on multi-modulus passes as under -f, then the stage-2 scan, whose factor lines name both bounds; a position whose
 * factor stage 1 reported is not reported again.  -x groups and refuses as avx-ecm -x does: consecutive lines on
 * one N are a group, the same N in two places is refused, so are lines of one N complete to different bounds, a bound
 * above B1, ECM lines and lines of the other method.  Everything is checked before anything runs or is written. */
static const char *method_usage = "usage: avx-ecm -m pm1|pp1 $input $B1 [$x0]\n"
                                  "       avx-ecm -m pm1|pp1 -f $file $B1     (one input expression per line)\n"
                                  "       avx-ecm -m pm1|pp1 -x $file $B1     (P-1 / P+1 resume lines, taken on to $B1)\n"
                                  "       (stage 1 only: there is no $B2)\n"
                                  "       avx-ecm -m pm1|pp1 -b $B2 ...       (any of the three, then stage 2 to $B2 > $B1)\n";

typedef struct {
    char ndec[MPL_MAXL * 10 + 16];
    mpl_t n;
    int nbits;
    size_t index;              /* of the input: its place in FILE, 0 for the one of the command line */
    uint64_t from;             /* the bound its residues are complete to (1: fresh) */
    int known;                 /* its residues name their seed */
} mnum_t;

typedef struct {
    size_t num;                /* its number */
    mpl_t x0, x;
} mres_t;

static void vec_set(const gecm_config *cfg, void *vec, size_t lane, size_t batch, const mpl_t *v)
{
    if (cfg->digitbits == 52) mpl_to_limbs64((uint64_t *)vec + lane, batch, cfg->nwords, 52, v);
    else mpl_to_limbs32((uint32_t *)vec + lane, batch, cfg->nwords, 32, v);
}

static void append_lines(const char *file, gecm_ctx *c, size_t count)
{
    FILE *f = fopen(file, "a");
    static char line[MPL_MAXL * 40];
    if (!f) { fprintf(stderr, "cannot write %s\n", file); exit(2); }
    for (size_t k = 0; k < count; k++)
        if (gecm_format_save_line_std(c, k, line, sizeof line) > 0) fputs(line, f);
    fclose(f);
}

/* one pass: the numbers nums[0 .. nn) and their residues res[0 .. nr) (res[r].num counts from nums[0]) */
/* B2 != 0 (-b): after the stage-1 scan, gecm_stage2(c, B2, 0, 0) on the same residues and the stage-2 scan;
 * a position whose factor stage 1 reported already is not reported again */
static int method_pass(int method, const mnum_t *nums, size_t nn, const mres_t *res, size_t nr, uint64_t B1, uint64_t B2, int packing)
{
    const char *mname = method == GECM_METHOD_PM1 ? "P-1" : "P+1";
    const uint64_t from = nums[0].from;
    const int known = nums[0].known, fresh = from == 1 && known;
    gecm_ctx *c = NULL;
    int rc;
    if (nn == 1) rc = gecm_create(&c, 0, nums[0].ndec, GECM_CLI_DIGITBITS);
    else {
        const char **ns = (const char **)malloc(nn * sizeof *ns);
        if (!ns) { fprintf(stderr, "out of memory\n"); exit(2); }
        for (size_t i = 0; i < nn; i++) ns[i] = nums[i].ndec;
        rc = gecm_create_multi(&c, 0, ns, nn, GECM_CLI_DIGITBITS);
        free(ns);
        if (!rc) rc = gecm_set_multi_packing(c, packing);
    }
    if (!rc) rc = gecm_set_method_lanes(c, cli_method_lanes());
    gecm_config cfg;
    if (!rc) rc = gecm_get_config(c, &cfg);
    void *x0 = NULL, *x = NULL;
    uint32_t *which = NULL;
    if (!rc) {
        const size_t bytes = nr * (size_t)cfg.nwords * (cfg.digitbits == 52 ? 8 : 4);
        x0 = calloc(1, bytes);
        x = calloc(1, bytes);
        which = (uint32_t *)malloc(nr * sizeof *which);
        if (!x0 || !x || !which) { fprintf(stderr, "out of memory\n"); exit(2); }
        for (size_t r = 0; r < nr; r++) {
            which[r] = (uint32_t)res[r].num;
            if (known) vec_set(&cfg, x0, r, nr, &res[r].x0);
            vec_set(&cfg, x, r, nr, &res[r].x);
        }
        rc = nn == 1 ? gecm_build_seeds(c, method, known ? x0 : NULL, fresh ? NULL : x, nr, from)
                     : gecm_build_seeds_multi(c, method, which, known ? x0 : NULL, fresh ? NULL : x, nr, from);
    }
    const int nseg = rc ? 0 : gecm_stage1_extend_segments(from, B1);
    double ms = 0;
    for (int seg = 0; seg < nseg && !rc; seg++) {
        rc = gecm_stage1_extend_segment(c, from, B1, (uint32_t)seg) || gecm_sync(c);
        ms += gecm_last_kernel_ms(c);
        if (!rc && seg + 1 < nseg) append_lines("checkpoint.txt", c, nr);
    }
    int found = 0;
    if (!rc) {
        append_lines("save_b1.txt", c, nr);
        found = gecm_scan_factors(c, 1, NULL);
        if (found < 0) rc = found;
    }
    if (rc) fprintf(stderr, "%s\n", gecm_last_error());
    for (size_t r = 0; r < nr && !rc && found > 0; r++) {
        static char fac[4096], seed[MPL_MAXL * 10 + 16], line[4096 + MPL_MAXL * 10 + 512];
        int prp = 0;
        if (!gecm_curve_flag(c, 1, r) || gecm_stage1_factor(c, r, fac, sizeof fac, &prp) != 1) continue;
        if (gecm_curve_seed(c, r, seed, sizeof seed) > 0)
            snprintf(line, sizeof line, "\nfound %s%d factor %s by %s (B1 = %lu): input %zu, x0 0x%s\n", prp ? "PRP" : "C",
                     gecm_sizeinbase10(fac), fac, mname, (unsigned long)B1, nums[res[r].num].index, seed);
        else
            snprintf(line, sizeof line, "\nfound %s%d factor %s by %s (B1 = %lu): input %zu, x0 unknown\n", prp ? "PRP" : "C",
                     gecm_sizeinbase10(fac), fac, mname, (unsigned long)B1, nums[res[r].num].index);
        fputs(line, stdout);
        FILE *f = fopen("ecm_results.txt", "a");
        if (!f) { fprintf(stderr, "cannot write ecm_results.txt\n"); exit(2); }
        fputs(line, f);
        fclose(f);
    }
    double ms2 = 0;
    int found2 = 0;
    if (!rc && B2) {
        rc = gecm_set_method_stage2(c, GECM_METHOD_S2_ON);
        if (!rc && nn > 1) rc = gecm_set_stage2_subseq(c, cli_multi_subseq());
        const double t2 = now();
        if (!rc) rc = gecm_stage2(c, B2, 0, 0);
        ms2 = (now() - t2) * 1000.0;
        if (!rc) {
            found2 = gecm_scan_factors(c, 2, NULL);
            if (found2 < 0) rc = found2;
        }
        if (rc) fprintf(stderr, "%s\n", gecm_last_error());
    }
    for (size_t r = 0; r < nr && !rc && found2 > 0; r++) {
        static char fac[4096], seed[MPL_MAXL * 10 + 16], line[4096 + MPL_MAXL * 10 + 512];
        int prp = 0;
        if (!gecm_curve_flag(c, 2, r) || gecm_curve_flag(c, 1, r) || gecm_stage2_factor(c, r, fac, sizeof fac, &prp) != 1) continue;
        if (gecm_curve_seed(c, r, seed, sizeof seed) > 0)
            snprintf(line, sizeof line, "\nfound %s%d factor %s by %s (B1 = %lu, B2 = %lu): input %zu, x0 0x%s\n", prp ? "PRP" : "C",
                     gecm_sizeinbase10(fac), fac, mname, (unsigned long)B1, (unsigned long)B2, nums[res[r].num].index, seed);
        else
            snprintf(line, sizeof line, "\nfound %s%d factor %s by %s (B1 = %lu, B2 = %lu): input %zu, x0 unknown\n", prp ? "PRP" : "C",
                     gecm_sizeinbase10(fac), fac, mname, (unsigned long)B1, (unsigned long)B2, nums[res[r].num].index);
        fputs(line, stdout);
        FILE *f = fopen("ecm_results.txt", "a");
        if (!f) { fprintf(stderr, "cannot write ecm_results.txt\n"); exit(2); }
        fputs(line, f);
        fclose(f);
    }
    if (!rc && B2) {
        gecm_stage2_stats st;
        uint32_t kch = 0;
        const int K = gecm_get_stage2_subseq(c, &kch);
        if (gecm_get_stage2_stats(c, &st) == GECM_OK)
            printf("%s stage 2: B2 %lu, D %u, U %u, %lu pairs, %d sub-sequence%s, %1.4f seconds\n", mname, (unsigned long)B2, st.D, st.U,
                   (unsigned long)st.paired, K, K == 1 ? "" : "s", ms2 / 1000.0);
    }
    if (!rc) {
        char kn[128] = "";
        gecm_last_kernel_name(c, kn, sizeof kn);
        printf("%s pass: %zu number%s, %zu residue%s, B1 %lu -> %lu in %d segment%s, %s%s, %1.4f seconds of kernels\n", mname, nn,
               nn == 1 ? "" : "s", nr, nr == 1 ? "" : "s", (unsigned long)from, (unsigned long)B1, nseg, nseg == 1 ? "" : "s", kn,
               nn == 1 ? "" : gecm_get_multi_packing(c) == GECM_PACK_LANE ? ", lane-packed" : ", wave-packed", ms / 1000.0);
    }
    if (c) gecm_destroy(c);
    free(x0); free(x); free(which);
    return rc ? 2 : 0;
}

/* a small-factor line for a number whose P+1 seed a/b does not exist: gcd(b, N) */
static void seed_factor_line(text_t *t, const mpl_t *g, uint64_t B1, size_t index, const char *seed)
{
    static char fac[MPL_MAXL * 10 + 16];
    mpl_get_dec(fac, g);
    text_printf(t, "\nfound %s%d factor %s by P+1 (B1 = %lu): input %zu, x0 %s has no inverse\n", mpl_probab_prime(g, 3) ? "PRP" : "C",
                gecm_sizeinbase10(fac), fac, (unsigned long)B1, index, seed);
}

static int run_method(int argc, char **argv)
{
    if (argc < 5) { printf("%s", method_usage); return 1; }
    const int method = !strcmp(argv[2], "pm1") ? GECM_METHOD_PM1 : !strcmp(argv[2], "pp1") ? GECM_METHOD_PP1 : 0;
    if (!method) { printf("-m %s: the methods offered are pm1 (P-1) and pp1 (P+1)\n%s", argv[2], method_usage); return 1; }
    /* -b B2 after the method: taken out of the arguments, the rest is read as without it */
    const char *b2s = NULL;
    char *av[8];
    if (!strcmp(argv[3], "-b")) {
        if (argc < 7 || argc > 9) { printf("%s", method_usage); return 1; }
        b2s = argv[4];
        for (int i = 0; i < 3; i++) av[i] = argv[i];
        for (int i = 5; i < argc; i++) av[i - 2] = argv[i];
        argc -= 2;
        av[argc] = NULL;
        argv = av;
    }
    const int from_file = !strcmp(argv[3], "-f"), from_lines = !strcmp(argv[3], "-x");
    const int listed = from_file || from_lines;
    if (listed ? argc != 6 : argc > 6) { printf("-m: stage 1 only: there is no stage 2, and no $B2 argument\n%s", method_usage); return 1; }
    const char *b1s = listed ? argv[5] : argv[4];
    char *end = NULL;
    const double b1d = strtod(b1s, &end);
    if (!*b1s || *end || !(b1d >= 2) || b1d > 1e12) { printf("-m: B1 must be in [2, 10^12]\n%s", method_usage); return 1; }
    const uint64_t B1 = (uint64_t)b1d;
    uint64_t B2 = 0;
    if (b2s) {
        const double b2d = strtod(b2s, &end);
        if (!*b2s || *end || !(b2d > b1d) || b2d > 1e15) { printf("-m -b: B2 must be above B1 (and at most 10^15)\n%s", method_usage); return 1; }
        B2 = (uint64_t)b2d;
        if (B2 <= B1) { printf("-m -b: B2 must be above B1 (and at most 10^15)\n%s", method_usage); return 1; }
    }
    const int packing = cli_packing();
    if (packing < 0 || (B2 && cli_multi_subseq() == 1) || !cli_method_lanes()) return 1;
    const double t_start = now();
    const size_t per = method == GECM_METHOD_PP1 ? 2 : 1;       /* fresh residues per number */

    mnum_t *nums = NULL;
    mres_t *res = NULL;
    size_t nn = 0, nr = 0, cap_n = 0, cap_r = 0;
    text_t early = {0};                                          /* the factor lines of seeds that do not exist */
    FILE *f = listed ? fopen(argv[4], "r") : NULL;
    if (listed && !f) { printf("cannot read %s\n%s", argv[4], method_usage); return 1; }
    char *text = NULL;
    size_t text_cap = 0, lineno = 0, input = 0;
    int bad = 0;
    for (;;) {
        static char prep_log[65536];
        const char *expr = NULL;
        gecm_resume_rec rec;
        gecm_resume_num seed = {NULL, 0, 0};
        int prm = 0, meth = 0;
        if (!listed) {
            if (input) break;
            expr = argv[3];
        } else {
            if (getline(&text, &text_cap, f) <= 0) break;
            lineno++;
            if (from_file) {
                char *q = text, *e;
                while (*q == ' ' || *q == '\t') q++;
                e = q + strlen(q);
                while (e > q && (e[-1] == '\n' || e[-1] == '\r' || e[-1] == ' ' || e[-1] == '\t')) *--e = 0;
                if (!*q || *q == '#') continue;
                expr = q;
            } else {
                const int rc = gecm_parse_resume_line_method(text, &rec, &prm, &meth, &seed);
                if (rc == 1) continue;
                if (rc) { printf("%s line %zu: %s\n", argv[4], lineno, gecm_last_error()); bad = 1; break; }
                if (meth != method) {
                    printf("%s line %zu: a METHOD=%s line: avx-ecm -m %s -x takes %s lines\n", argv[4], lineno,
                           meth == GECM_METHOD_ECM ? "ECM" : meth == GECM_METHOD_PM1 ? "P-1" : "P+1", argv[2],
                           method == GECM_METHOD_PM1 ? "P-1" : "P+1");
                    bad = 1;
                    break;
                }
            }
        }
        if (nn + 1 > cap_n) { cap_n = cap_n ? 2 * cap_n : 64; nums = (mnum_t *)realloc(nums, cap_n * sizeof *nums); }
        if (nr + 2 > cap_r) { cap_r = cap_r ? 2 * cap_r : 128; res = (mres_t *)realloc(res, cap_r * sizeof *res); }
        if (!nums || !res) { fprintf(stderr, "out of memory\n"); return 2; }
        if (!from_lines) {
            mnum_t *m = &nums[nn];
            gecm_input_info inf;
            if (gecm_prepare_input(expr, GECM_CLI_DIGITBITS, m->ndec, sizeof m->ndec, &inf, prep_log, sizeof prep_log)) {
                fputs(prep_log, stdout);
                printf("input must evaluate to an odd integer >= 3 (operators + - * / %% ^ ! # fib() luc())\n");
                bad = 1;
                break;
            }
            mpl_set_str(&m->n, m->ndec);
            m->nbits = inf.nbits;
            m->index = input++;
            m->from = 1;
            m->known = 1;
            size_t made = 0;
            if (!listed && argc == 6) {                          /* the seed of the command line */
                mres_t *r = &res[nr];
                if (mpl_set_str(&r->x0, argv[5]) || mpl_cmp(&r->x0, &m->n) >= 0) { printf("-m: x0 must be a number below the input\n%s", method_usage); bad = 1; break; }
                r->x = r->x0;
                r->num = nn;
                made = 1;
            } else
                for (size_t k = 0; k < per; k++) {
                    static const uint64_t num[3] = {3, 2, 6}, den[3] = {1, 7, 5};
                    static const char *name[3] = {"3", "2/7", "6/5"};
                    const size_t w = method == GECM_METHOD_PM1 ? 0 : 1 + k;
                    mpl_t a, b, inv;
                    mres_t *r = &res[nr + made];
                    mpl_set_u64(&a, num[w]);
                    mpl_set_u64(&b, den[w]);
                    mpl_mod(&a, &a, &m->n);
                    mpl_mod(&b, &b, &m->n);
                    if (!mpl_invmod(&inv, &b, &m->n)) {
                        mpl_t g;
                        mpl_gcd(&g, &b, &m->n);
                        if (mpl_is_zero(&b)) g = m->n;
                        if (mpl_cmp(&g, &m->n) < 0) seed_factor_line(&early, &g, B1, m->index, name[w]);
                        continue;
                    }
                    mpl_mulmod(&r->x0, &a, &inv, &m->n);
                    r->x = r->x0;
                    r->num = nn;
                    made++;
                }
            if (made) { nr += made; nn++; }
            continue;
        }
        /* -x: one line */
        mpl_t n, v;
        rnum(&n, &rec.n);
        if (!mpl_is_odd(&n) || mpl_cmp_u64(&n, 3) < 0) { printf("%s line %zu: field N must be an odd number >= 3\n", argv[4], lineno); bad = 1; break; }
        uint64_t from = 0;
        if (gecm_resume_line_std_bound_method(text, &from)) { printf("%s line %zu: %s\n", argv[4], lineno, gecm_last_error()); bad = 1; break; }
        if (from < 1 || from > B1) {
            printf("%s line %zu: the line is complete to B1 = %lu, which is not in [1, %lu]: stage 1 is extended upwards only\n", argv[4],
                   lineno, (unsigned long)from, (unsigned long)B1);
            bad = 1;
            break;
        }
        if (!nn || mpl_cmp(&n, &nums[nn - 1].n) != 0) {
            mnum_t *m = &nums[nn];
            m->n = n;
            mpl_get_dec(m->ndec, &n);
            m->nbits = mpl_bits(&n);
            m->index = nn;
            m->from = from;
            m->known = seed.digits != NULL;
            for (size_t k = 0; k < nn && !bad; k++)
                if (mpl_cmp(&nums[k].n, &n) == 0) {
                    printf("%s line %zu: lines on this N stand further up as well, with another N between: put the lines on one "
                           "number together\n", argv[4], lineno);
                    bad = 1;
                }
            if (bad) break;
            nn++;
        }
        mnum_t *m = &nums[nn - 1];
        if (from != m->from) {
            printf("%s line %zu: the line is not complete to the bound %lu of the lines on this N before it\n", argv[4], lineno, (unsigned long)m->from);
            bad = 1;
            break;
        }
        if (m->known && !seed.digits) m->known = 0;             /* one line without its seed: the number's lines omit it */
        mres_t *r = &res[nr];
        rnum(&r->x, &rec.x);
        if (seed.digits) rnum(&r->x0, &seed);
        else mpl_set_u64(&r->x0, 0);
        rnum(&v, &rec.x);
        if (mpl_cmp(&v, &n) >= 0 || mpl_cmp(&r->x0, &n) >= 0) { printf("%s line %zu: X or X0 is not below N\n", argv[4], lineno); bad = 1; break; }
        r->num = nn - 1;
        nr++;
    }
    if (f) fclose(f);
    free(text);
    if (!bad && !nr && !early.len) { printf("%s holds no %s\n%s", listed ? argv[4] : argv[3], from_lines ? "resume line" : "input", method_usage); bad = 1; }
    if (bad) { free(nums); free(res); free(early.buf); return 1; }
    if (gecm_device_count() < 1) { fprintf(stderr, "no HIP device visible\n"); return 2; }
    printf("starting process %d: %s stage 1 to B1 = %lu on %zu number%s, %zu residue%s\n", (int)getpid(),
           method == GECM_METHOD_PM1 ? "P-1" : "P+1", (unsigned long)B1, nn, nn == 1 ? "" : "s", nr, nr == 1 ? "" : "s");
    if (early.len) {
        fputs(early.buf, stdout);
        FILE *rf = fopen("ecm_results.txt", "a");
        if (!rf) { fprintf(stderr, "cannot write ecm_results.txt\n"); return 2; }
        fputs(early.buf, rf);
        fclose(rf);
    }
    /* the passes: numbers in order, closed by size, by the packing's line, by the bound and by whether seeds are known */
    const size_t cap = env_count("GECM_PASS_CURVES") ? (size_t)env_count("GECM_PASS_CURVES") : FULL_BATCH;
    int rc = 0;
    size_t r0 = 0;
    for (size_t n0 = 0; n0 < nn && rc != 2; ) {
        const int pk = packing == GECM_PACK_LANE && fits_lane_packing(nums[n0].nbits) ? GECM_PACK_LANE : GECM_PACK_WAVE;
        size_t n1 = n0, r1 = r0, positions = 0;
        while (n1 < nn) {
            size_t cnt = 0;
            while (r1 + cnt < nr && res[r1 + cnt].num == n1) cnt++;
            const int pk1 = packing == GECM_PACK_LANE && fits_lane_packing(nums[n1].nbits) ? GECM_PACK_LANE : GECM_PACK_WAVE;
            const size_t add = pk == GECM_PACK_LANE ? cnt : gecm_multi_positions(&cnt, 1, GECM_PACK_WAVE);
            if (n1 > n0 && (pk1 != pk || nums[n1].from != nums[n0].from || nums[n1].known != nums[n0].known || positions + add > cap)) break;
            positions += add;
            r1 += cnt;
            n1++;
        }
        for (size_t r = r0; r < r1; r++) res[r].num -= n0;
        rc = method_pass(method, nums + n0, n1 - n0, res + r0, r1 - r0, B1, B2, pk);
        n0 = n1;
        r0 = r1;
    }
    free(nums); free(res); free(early.buf);
    printf("Process took %1.4f seconds.\n", now() - t_start);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "-f") == 0) return run_file(argc, argv);
    if (argc > 1 && strcmp(argv[1], "-r") == 0) return run_resume(argc, argv, 0, 0);
    if (argc > 1 && strcmp(argv[1], "-x") == 0) return run_resume(argc, argv, 1, 0);
    if (argc > 1 && strcmp(argv[1], "-g") == 0) {
        /* -g -r, -g -x: the same two with lines of PARAM 0, 1 and 3 accepted */
        if (argc > 2 && strcmp(argv[2], "-r") == 0) return run_resume(argc - 1, argv + 1, 0, 1);
        if (argc > 2 && strcmp(argv[2], "-x") == 0) return run_resume(argc - 1, argv + 1, 1, 1);
        printf("%s%s", gmp_resume_usage, gmp_extend_usage);
        return 1;
    }
    if (argc > 1 && strcmp(argv[1], "-p") == 0) return run_param(argc, argv);
    if (argc > 1 && strcmp(argv[1], "-m") == 0) return run_method(argc, argv);
    return run_single(argc, argv);
}
