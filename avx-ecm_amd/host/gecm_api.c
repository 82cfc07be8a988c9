/* gecm_api.c — public C ABI of libgecm (include/gecm.h): the contexts, their batch state and the phase functions, in
 * C above the HIP device layer (csrc/gecm_dev.h).  What depends on one number N alone — its constants, the curve
 * construction, failure records, the factor report — is gecm_mod.c, which knows neither device nor context; a context
 * holds the gecm_mod of its number, a multi-modulus context one more per modulus and the gecm_layout of its batch (the
 * position arithmetic is gecm_mod.c's too), and curve_at() leads from a caller's curve to its modulus and its place in
 * the batch arrays.  Every call that puts a batch into a context describes it (batch_desc) and ends in batch_build().
 * Mirrors the reference's phase functions:
 *   ecm_stage1                  ecm.c:1806-1854 (tape built by gecm_plan.c, run by the device)
 *   save line                   ecm.c:1372-1380
 */
#include "../../include/gecm.h"
#include "../csrc/gecm_dev.h"
#include "gecm_plan.h"
#include "gecm_pair.h"
#include "gecm_mod.h"
#include "cunningham.h"
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

/* stage 2: giant steps per device chunk (one inversion each) and ring size (power of two >= chunk + 2L) */
#define S2_GIANT_CHUNK 512u
#define S2_RING 1024u
/* largest B1: the 32-bit offsets of a range's tape and uint32 range indices are nowhere near it; the cap is the
 * reference's own (its prime sieve serves ranges below 10^13 or so; ecm.c keeps primes in 64 bits) kept at a size one
 * can still test */
#define GECM_B1_MAX 1000000000000ull
#define gecm_stage1_ranges_u(b1) gecm_stage1_ranges_plan(b1)

#define set_err gecm_mod_set_err
const char *gecm_last_error(void) { return gecm_mod_err; }
/* "libgecm 0.3 (gfx950) K:<hash> R:<hash> D:<hash> H:<hash>": the hashes of the sources the objects inside this
 * library were compiled from (avx-ecm_amd/Makefile: kernels, 32-lane kernels, device layer, host C), MIXED where
 * objects of one group disagree.  tests/test_abi_cpu.py and __graft_entry__.smoke() recompute them from the tree. */
#ifndef GECM_MANIFEST
#define GECM_MANIFEST "unset"
#endif
const char *gecm_manifest_host_gecm_plan(void);
const char *gecm_manifest_host_gecm_pair(void);
const char *gecm_manifest_host_mpl(void);
const char *gecm_manifest_host_calc_lite(void);
const char *gecm_manifest_host_cunningham(void);
const char *gecm_manifest_host_gecm_mod(void);
const char *gecm_manifest_host_gecm_resume(void);
const char *gecm_version(void)
{
    static char v[256];
    if (!v[0]) {
        const char *h[7] = {gecm_manifest_host_gecm_plan(), gecm_manifest_host_gecm_pair(), gecm_manifest_host_mpl(),
                            gecm_manifest_host_calc_lite(), gecm_manifest_host_cunningham(), gecm_manifest_host_gecm_mod(),
                            gecm_manifest_host_gecm_resume()};
        int mixed = 0;
        for (int i = 0; i < 7; i++) mixed |= strcmp(h[i], GECM_MANIFEST) != 0;
        snprintf(v, sizeof v, "libgecm 0.3 (gfx950) %s H:%s", gecm_dev_manifest(), mixed ? "MIXED" : GECM_MANIFEST);
    }
    return v;
}
int gecm_device_count(void) { return gecm_dev_count(); }

/* which tape: kind 0 = the ecm_stage1 call number b of a reference run to B1 = a (gecm_tape_build_stage1_range),
 * kind 1 = the extension segment (a, b] of the standard multiplier (gecm_tape_build_extend) */
typedef struct {
    int kind;
    uint64_t a, b;
} tape_key;
static int key_eq(const tape_key *x, const tape_key *y) { return x->kind == y->kind && x->a == y->a && x->b == y->b; }
static int tape_build(gecm_tape_t *t, const tape_key *k, int threads)
{
    return k->kind ? gecm_tape_build_extend(t, k->a, k->b, threads) : gecm_tape_build_stage1_range(t, k->a, (uint32_t)k->b, threads);
}

struct gecm_ctx {
    int device;
    gecm_mod mod;        /* the context's number; of a multi-modulus context the largest (what gecm_get_config reports) */
    gecm_dev *dev, *dev_l0;
    /* current batch */
    size_t batch;
    uint64_t *sigma;
    uint8_t *bad;
    uint8_t *param;      /* the parametrisation of every position; NULL: the batch was built without a setting, 0 throughout */
    uint8_t *next_param; /* gecm_set_next_params: of the next build, the caller's order, next_batch curves; NULL: none pending */
    size_t next_batch;
    uint32_t *hx, *hz;   /* last downloaded plain x, z: [nl][batch] */
    int have_plain;
    int normalized;      /* X = x/z, Z = 1 since the last gecm_normalize_points; norm_left[pos] = 1: that curve's Z has no inverse */
    uint8_t *norm_left;
    uint64_t B1;
    /* tape cache: the tape of tape_k, one ecm_stage1 call of the reference or one extension segment */
    gecm_tape_t tape;
    tape_key tape_k;
    tape_key dev_tape_k;     /* the tape dev holds (all zero: none, which is no tape's key) */
    double last_ms;
    /* counters of the stage 1 in progress: summed over the ranges run since range 0 (work->ptadds / ptdups are
     * cleared when the curves are built, ecm.c:1177-1178, and grow through every ecm_stage1 call) */
    uint64_t s1_ptadds, s1_ptdups, s1_last_prime, s1_tape_len;
    /* the next range's tape, compiled by a helper thread while the device runs the current range */
    pthread_t pf_thread;
    int pf_active, pf_rc;
    gecm_tape_t pf_tape;
    tape_key pf_k;
    /* stage 2 */
    gecm_s2_plan s2;
    int s2_ready;
    uint32_t *hacc, *hfail;
    uint32_t fail_planes;    /* planes of hfail: 1, or 1 + sub-sequences (gecm_dev_s2_fail_planes) */
    uint32_t s2_K;           /* sub-sequences per curve of the last gecm_stage2_init; 0 before the first */
    gecm_pairs pm;           /* pair map of the last single-range gecm_stage2 call (pm_valid), reused while (range, D, U) match */
    int pm_valid;
    gecm_s2_tape tp;         /* the device tape made from pm (tp_valid): it depends on (pm, D, U) only, so it is kept with it */
    int tp_valid;
    uint64_t tp_id;          /* identifies the kept tape to the device side, which then keeps its copy too */
    gecm_s2_tape ptp;        /* the tape of the last gecm_stage2_pair call (ptp_valid), found again by a fingerprint of the map */
    int ptp_valid;
    uint64_t ptp_fp, ptp_fp2, ptp_id;
    uint32_t ptp_steps, ptp_amin, ptp_D, ptp_U;
    uint64_t pm_lo, pm_hi;
    uint32_t pm_D, pm_U;
    int have_acc;
    uint32_t *flags[2];      /* per-curve result of the last device factor scan: stage 1, stage 2 */
    uint32_t *hg[2];         /* and the gcds it computed, [nl][batch] */
    int scan_valid[2];       /* the cached scan belongs to the current stage-1 / stage-2 result */
    uint64_t s2_ptadds, s2_numinv, s2_paired, s2_devinv;
    uint32_t s2_amin_last;
    int lanes_per_curve;     /* 0 = auto, 1, 2, 8, 32 (gecm_set_lanes_per_curve) */
    int build_where, build_used;   /* GECM_BUILD_HOST / _DEVICE: asked for (gecm_set_curve_build), used by the last build */
    /* the special-form twin of a context whose N divides Mw = 2^k -/+ 1 or 2^k - c: a second device context working
     * modulo Mw with the special stage-1 multiply (csrc/gecm_field.hpp); see "the special-form twin" below */
    struct {
        gecm_dev *dev;       /* NULL: this N has no twin */
        int k, sign;         /* Mw = 2^k - c for sign > 0 (c = 1: Mersenne form), 2^k + 1 for sign < 0 */
        uint64_t c;
        int nl;              /* limbs of Mw */
        int on;              /* gecm_set_special_form */
        int loaded;          /* the twin holds the main context's points (twin_fill) */
        int pending;         /* a launch ran on the twin and its X, Z are not back in the main context (ff_settle) */
        int ran_last;        /* the last stage-1 launch ran on the twin */
        tape_key tape_k;     /* the tape twin.dev holds, as dev_tape_k */
    } twin;
    /* multi-modulus context (gecm_create_multi): grp[] holds every modulus's N and constants (at this
     * context's limb count); the curves are grouped by modulus, each group padded to whole wavefronts of 64, and the
     * batch arrays are in that device order.  The caller numbers curves in its own order (curve_at). */
    int multi;
    size_t ngroups;
    gecm_mod *grp;
    gecm_devmod *grp_dev;    /* grp[]'s constants as the device layer takes them (gecm_dev_set_groups) */
    gecm_layout lay;         /* the batch's positions (gecm_mod.h); all zero on a single-N context and without a batch */
    /* GECM_PACK_WAVE / GECM_PACK_LANE: asked for (gecm_set_multi_packing), used by the last build.  Lane
     * packing lays the groups back to back and pads only the batch's tail; every lane then carries its own modulus. */
    int packing, packing_used;
    /* P-1 / P+1 batch (gecm_build_seeds): GECM_METHOD_PM1 / _PP1, one residue per position in X, Z = 1;
     * seed = the plain x0 of every position, [nl][batch] in device order, NULL when the caller did not know it */
    int method;
    uint32_t *seed;
    int method_s2;           /* gecm_set_method_stage2: the stage-2 calls work on a method batch; kept across builds */
    int method_lanes;        /* gecm_set_method_lanes: 0 (as 1), 1, 16 or GECM_METHOD_LANES_AUTO; kept across builds */
    int urow_state;          /* the 16-lane method kernel's constants: 0 not made yet, 1 on the device, -1 none (rows_on_device) */
    int multi_rows;          /* gecm_set_multi_rows: GECM_MULTI_ROWS_OFF, _ON or _AUTO; kept across builds */
    int wide;                /* gecm_create_wide made a wide context: stage 1 on the device, the rest on the host */
    int mrow_state;          /* the 32-lane kernel's constants for every modulus of a multi-modulus context, as urow_state */
};

/* what a multi-modulus context cannot do: the reference radix (NWORDS) differs from modulus to modulus, and the L0
 * operators, uploaded points and the special forms work modulo one N */
static int multi_refuse(const char *fn)
{
    set_err("%s: not available on a multi-modulus context (gecm_create_multi)", fn);
    return GECM_ERR_STATE;
}

/* what a wide context cannot do (include/gecm.h): its limb count has the 32-lane stage-1 kernel and no
 * other, so everything that is not stage 1, or host work on its result, is refused before the batch is touched */
static int wide_refuse(const char *fn)
{
    set_err("%s: not available on a wide context (gecm_create_wide): it runs curve build, stage 1 and what the host "
            "makes of the result", fn);
    return GECM_ERR_STATE;
}

static const char *method_name(int method) { return method == GECM_METHOD_PM1 ? "P-1" : method == GECM_METHOD_PP1 ? "P+1" : "ECM"; }

/* what a P-1 / P+1 batch cannot do (include/gecm.h): 0 for a batch of curves.  stage2_call: fn is one of the stage-2
 * calls, which gecm_set_method_stage2 lets through. */
static int method_refuse(const gecm_ctx *c, const char *fn, int stage2_call)
{
    if (!c || !c->method || c->batch == 0) return 0;
    if (stage2_call && c->method_s2) return 0;
    set_err("%s: not available on a %s batch (gecm_build_seeds): it holds residues, not curves", fn, method_name(c->method));
    return GECM_ERR_STATE;
}

/* the device layer's name for the method of the batch */
static int unit_method(const gecm_ctx *c) { return c->method == GECM_METHOD_PP1 ? GECM_UNIT_PP1 : GECM_UNIT_PM1; }

int gecm_set_method_stage2(gecm_ctx *c, int on)
{
    if (!c || (on != GECM_METHOD_S2_OFF && on != GECM_METHOD_S2_ON)) {
        set_err("gecm_set_method_stage2: needs a context and GECM_METHOD_S2_OFF or GECM_METHOD_S2_ON");
        return GECM_ERR_ARG;
    }
    c->method_s2 = on;
    return GECM_OK;
}

int gecm_get_method_stage2(const gecm_ctx *c) { return c ? c->method_s2 : GECM_METHOD_S2_OFF; }

static int pick_nl(int nbits)
{
    int need = (nbits + 5 + LIMB_BITS - 1) / LIMB_BITS;   /* R = 2^(28 nl) >= 32 N */
    for (const int *p = gecm_dev_supported_nl(); *p; p++)
        if (*p >= need) return *p;
    return 0;
}

/* ---- host worker threads ---------------------------------------------------------------------- */
static int host_threads(void)
{
    /* worker threads for host-side batch work: GECM_HOST_THREADS, else min(8, online CPUs) */
    const char *e = getenv("GECM_HOST_THREADS");
    long n = e ? atol(e) : sysconf(_SC_NPROCESSORS_ONLN);
    if (n < 1) n = 1;
    if (!e && n > 8) n = 8;
    if (n > 64) n = 64;
    return (int)n;
}

/* fn(arg, lo, hi) over the slices of [0, n), 256 or more items each, on up to host_threads() threads (a thread that
 * cannot be started: its slice runs here).  Returns an error (< 0) of some slice, else the OR of the slices' results. */
typedef struct {
    int (*fn)(void *arg, size_t lo, size_t hi);
    void *arg;
    size_t lo, hi;
    int ret;
} slice_job;

static void *slice_run(void *job)
{
    slice_job *j = (slice_job *)job;
    j->ret = j->fn(j->arg, j->lo, j->hi);
    return NULL;
}

static int run_slices(size_t n, int (*fn)(void *arg, size_t lo, size_t hi), void *arg)
{
    int nt = host_threads();
    if ((size_t)nt > n / 256 + 1) nt = (int)(n / 256 + 1);
    slice_job jobs[64];
    pthread_t th[64];
    for (int t = 0; t < nt; t++)
        jobs[t] = (slice_job){fn, arg, n * (size_t)t / (size_t)nt, n * (size_t)(t + 1) / (size_t)nt, 0};
    for (int t = 1; t < nt; t++)
        if (pthread_create(&th[t], NULL, slice_run, &jobs[t])) { slice_run(&jobs[t]); th[t] = 0; }
    slice_run(&jobs[0]);
    int err = 0, any = 0;
    for (int t = 0; t < nt; t++) {
        if (t > 0 && th[t]) pthread_join(th[t], NULL);
        if (jobs[t].ret < 0) err = jobs[t].ret;
        any |= jobs[t].ret;
    }
    return err ? err : any;
}

/* ---- the special-form twin --------------------------------------------------------------------
 * N | 2^k - 1, N | 2^k + 1 or N | 2^k - c with c below one reference limb (the reference's isMersenne == +1 / -1 / c,
 * main.c:410-441): ff_setup opens a second device context modulo Mw = 2^k -/+ 1 or 2^k - c for the special stage-1
 * multiply (csrc/gecm_field.hpp, F-form / P-form / C-form) when that is the cheaper multiply.  twin_fill loads it with
 * the main context's batch, stage1_launch runs the chain there, and ff_settle brings X, Z back modulo N: everything
 * after stage 1 (save lines, factor scan, stage 2) works on residues modulo N as always.  Failure to set the twin up
 * is not an error: stage 1 then runs modulo N like everything else. */
static void ff_setup(gecm_ctx *c)
{
    cunningham_form f;
    cunningham_detect(&f, &c->mod.N, c->mod.digitbits);
    if ((f.form != 1 && f.form != -1 && f.form != 2) || f.k < 64) return;
    if (f.form == 2 && (f.c < 3 || !(f.c & 1))) return;              /* 2^k - c with c odd, c > 1 (c = 1 is form +1) */
    const int mbits = f.form < 0 ? f.k + 1 : f.k;
    const int nlf = pick_nl(mbits);
    if (!nlf) return;
    const int G = gecm_dev_fform_generic_limbs(nlf);
    if (G < 0 || f.k < LIMB_BITS * (nlf - G)) return;                 /* limbs below nl-G must be F..F / 1,0..0 */
    if (f.form == 2 && nlf - G < 3) return;                          /* limbs 0, 1 carry c - 1: one pure F limb above */
    /* multiply-adds per modular multiplication: about nl^2 + G*nl (+ 3 nl for 2^k - c) against 2 nl^2 + nl */
    if ((double)(nlf * nlf + (G + (f.form == 2 ? 3 : 0)) * nlf) * 1.15 > (double)(2 * c->mod.nl * c->mod.nl + c->mod.nl)) return;
    mpl_t one, t, M, r;
    mpl_set_u64(&one, 1);
    mpl_shl(&M, &one, (unsigned)f.k);
    if (f.form == 2) { mpl_set_u64(&t, f.c); mpl_sub(&M, &M, &t); }
    else if (f.form > 0) mpl_sub(&M, &M, &one);
    else mpl_add(&M, &M, &one);
    mpl_mod(&r, &M, &c->mod.N);
    if (!mpl_is_zero(&r)) return;                                    /* N | Mw, or nothing below holds */
    /* the constants block, nlf limbs each: Mw, kp, one = R mod Mw, R^2 mod Mw (R = 2^(28 nlf)); the twin never inverts */
    uint32_t *q = (uint32_t *)calloc((size_t)nlf * 4, sizeof(uint32_t));
    if (!q) return;
    gecm_mod_pow2(&r, (unsigned)(LIMB_BITS * nlf), &M);
    mpl_to_limbs32(q, 1, nlf, LIMB_BITS, &M);
    mpl_to_limbs32(q + 2 * nlf, 1, nlf, LIMB_BITS, &r);
    mpl_mulmod(&r, &r, &r, &M);
    mpl_to_limbs32(q + 3 * nlf, 1, nlf, LIMB_BITS, &r);
    /* rho = -Mw^-1 mod 2^28: 1 for 2^k - 1, 2^28 - 1 for 2^k + 1, (c mod 2^28)^-1 for 2^k - c */
    uint32_t rho = f.form == 1 ? 1u : (1u << LIMB_BITS) - 1u;
    if (f.form == 2) {
        mpl_t two28, inv;
        mpl_set_u64(&two28, 1u << LIMB_BITS);
        if (!mpl_invmod(&inv, &M, &two28)) { free(q); return; }
        mpl_sub(&inv, &two28, &inv);
        rho = (uint32_t)mpl_get_u64(&inv);
    }
    const gecm_devmod dm = {q, q + nlf, q + 2 * nlf, q + 3 * nlf, NULL, rho, 0};
    const int failed = gecm_mod_make_kp(q + nlf, &M, nlf) || gecm_dev_open(&c->twin.dev, c->device, nlf, &dm, 0);
    free(q);                                                         /* the device layer has its copy */
    if (failed) {
        c->twin.dev = NULL;
        return;
    }
    gecm_dev_set_fform(c->twin.dev, f.form);
    c->twin.k = f.k;
    c->twin.sign = f.form < 0 ? -1 : 1;
    c->twin.c = f.form == 2 ? f.c : 1;
    c->twin.nl = nlf;
    c->twin.on = 1;
}

/* The batch the main context holds into the twin, converted on the device (gecm_dev_fill_twin): out of Montgomery
 * form modulo N, the limb planes copied, into Montgomery form modulo Mw (x < N <= Mw).  The only code that puts
 * points into the twin, whether or not gecm_set_special_form has it switched on; for its callers a failure is a
 * device error (gecm_dev_error has the text).  Nothing to do on a context without a twin. */
static int twin_fill(gecm_ctx *c)
{
    if (!c->twin.dev) return 0;
    const int rc = gecm_dev_fill_twin(c->twin.dev, c->dev);
    c->twin.loaded = !rc;
    return rc;
}

/* ff_settle: wait for the stage-1 kernel that ran on the twin, fetch its X, Z (canonical, de-Montgomeryised), reduce
 * them modulo N, put them back into Montgomery form modulo N and store them in the main context as if stage 1 had run
 * there.  Nothing to do, and GECM_OK, when no launch on the twin is pending (or c is NULL: the callers check that
 * after it). */
typedef struct {
    const gecm_ctx *c;
    uint32_t *f;              /* fx, fz [twin.nl][batch], then hX, hZ [nl][batch] */
} settle_job;

static int settle_slice(void *arg, size_t lo, size_t hi)
{
    const settle_job *j = (const settle_job *)arg;
    const gecm_ctx *c = j->c;
    const size_t batch = c->batch, fwords = (size_t)c->twin.nl * batch, words = (size_t)c->mod.nl * batch;
    for (size_t i = lo; i < hi; i++)
        for (int q = 0; q < 2; q++) {                /* x, z */
            mpl_t v;
            mpl_from_limbs32(&v, j->f + q * fwords + i, batch, c->twin.nl, LIMB_BITS);
            mpl_mod(&v, &v, &c->mod.N);
            mpl_mulmod(&v, &v, &c->mod.rint_mod_n, &c->mod.N);
            mpl_to_limbs32(j->f + 2 * fwords + q * words + i, batch, c->mod.nl, LIMB_BITS, &v);
        }
    return 0;
}

static int ff_settle(gecm_ctx *c)
{
    if (!c || !c->twin.pending) return GECM_OK;
    c->twin.pending = 0;
    if (gecm_dev_sync(c->twin.dev)) { set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    c->last_ms = gecm_dev_last_kernel_ms(c->twin.dev);
    const size_t batch = c->batch, fwords = (size_t)c->twin.nl * batch, words = (size_t)c->mod.nl * batch;
    uint32_t *f = (uint32_t *)calloc(2 * fwords + 2 * words, 4);
    if (!f) return GECM_ERR_NOMEM;
    if (gecm_dev_download_plain(c->twin.dev, f, f + fwords)) { free(f); set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    settle_job j = {c, f};
    run_slices(batch, settle_slice, &j);
    int rc = gecm_dev_upload_xz(c->dev, f + 2 * fwords, f + 2 * fwords + words);
    free(f);
    if (rc) { set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    return GECM_OK;
}

/* the device the last stage-1 launch ran on */
static inline gecm_dev *last_dev(const gecm_ctx *c) { return c->twin.ran_last ? c->twin.dev : c->dev; }

/* ---- constants of the row kernels (gecm_mod_row_consts) ------------------------------------------ */
/* The kinds of set: the 32-lane stage-1 kernel's for a single N (gecm_dev_set_rowconst), the 16-lane method kernel's
 *  and the 32-lane kernel's on a multi-modulus batch (§23: the first kind, and behind it the modulus's rho). */
enum { ROWC_CURVE, ROWC_METHOD, ROWC_MULTI };
typedef struct {
    uint32_t *words;         /* the sets back to back; the caller frees them */
    uint32_t sets;
    int nq, rows;            /* gecm_row_shape of the context's limb count: rows = limbs in use, 28 (nl + 1) >= bits(N') + 5 */
} row_sets;

/* The sets of one kind for every modulus of the context: its one N, or the numbers of a multi-modulus context in the order
 * gecm_dev_set_groups names them.  1 if made, 0 if some number has none at this limb count, -2 out of memory. */
static int row_sets_build(const gecm_ctx *c, int kind, row_sets *out)
{
    const size_t set_words = kind == ROWC_CURVE ? GECM_ROW_KINDS * GECM_ROW_WORDS : kind == ROWC_METHOD ? GECM_UROW_SET : GECM_MROW_SET;
    out->words = NULL;
    out->sets = c->multi ? (uint32_t)c->ngroups : 1;
    gecm_row_shape(c->mod.nl, &out->nq, &out->rows);
    if (out->nq > GECM_ROW_MAXNQ) return 0;
    uint32_t *s = (uint32_t *)calloc(out->sets * set_words, sizeof(uint32_t));
    if (!s) return -2;
    for (size_t g = 0; g < out->sets; g++) {
        const gecm_mod *m = c->multi ? &c->grp[g] : &c->mod;
        uint32_t *set = s + g * set_words;
        if (!gecm_mod_row_consts(m, c->mod.nl, out->rows, kind == ROWC_METHOD ? NULL : set, kind == ROWC_METHOD ? set : NULL)) {
            free(s);
            return 0;
        }
        if (kind == ROWC_MULTI) set[GECM_ROW_KINDS * GECM_ROW_WORDS] = m->rho28;
    }
    out->words = s;
    return 1;
}

/* The 32-lane stage-1 kernel's constants for the context's modulus.  Not an error if they cannot be set up: the other
 * layouts cover every N. */
static void row_setup(gecm_ctx *c)
{
    row_sets s;
    if (row_sets_build(c, ROWC_CURVE, &s) > 0) (void)gecm_dev_set_rowconst(c->dev, s.nq, s.rows, s.words);
    free(s.words);
}

/* The method kernel's (ROWC_METHOD) or the multi-modulus curve kernel's (ROWC_MULTI) sets on the device.  They depend on
 * the context's numbers alone, so they are made once, when a launch first wants them; urow_state and mrow_state say how
 * that went: 0 not made yet, 1 on the device, -1 some number of the context has none.  1 if the device has them; 0 if there
 * are none (remembered); -2 if host memory, -1 if the upload failed this time (not remembered: the next launch tries again). */
static int rows_on_device(gecm_ctx *c, int kind)
{
    int *state = kind == ROWC_METHOD ? &c->urow_state : &c->mrow_state;
    if (*state) return *state > 0;
    row_sets s;
    const int made = row_sets_build(c, kind, &s);
    if (made <= 0) {
        if (!made) *state = -1;
        return made;
    }
    const int failed = kind == ROWC_METHOD ? gecm_dev_set_unit_rowconst(c->dev, s.nq, s.rows, s.sets, s.words)
                                           : gecm_dev_set_multi_rowconst(c->dev, s.nq, s.rows, s.sets, s.words);
    free(s.words);
    if (failed) return -1;
    *state = 1;
    return 1;
}

/* ---- lanes per residue of a method batch ---------------------------------------- */
/* 16 up to 64 positions per compute unit (four wavefronts of four residues on every SIMD), 1 beyond: read off the table of
 * DESIGN.md §22 (profiles/unit_row/time_rows.txt against time_parent_one_lane.txt, one MI355X of 256 compute units, tape
 * (1, 1e5]).  Up to 16 positions per compute unit the row launch is at most one wavefront per SIMD and its time does not
 * move with the batch: 83 ms against the one-lane kernel's 280 ms at 15 limbs, 205 ms against 1354 ms at 37.  At 64 per
 * compute unit (16,384 positions) it still wins, 162 against 282 ms and 643 against 1364 ms; at 256 per compute unit
 * (65,536) it has lost, 541 against 298 ms and 2445 against 1409 ms.  The crossover lies between the two at both limb
 * counts and was not measured more finely, so the rule stops at the last size measured to win, for every limb count. */
int gecm_method_lanes_auto(size_t positions, int dev_limbs, int cus)
{
    (void)dev_limbs;
    if (positions == 0 || cus <= 0) return 1;
    return positions <= (size_t)64 * (size_t)cus ? 16 : 1;
}

int gecm_set_method_lanes(gecm_ctx *c, int lanes)
{
    if (!c || (lanes != 1 && lanes != 16 && lanes != GECM_METHOD_LANES_AUTO)) {
        set_err("gecm_set_method_lanes: needs a context and 1, 16 or GECM_METHOD_LANES_AUTO");
        return GECM_ERR_ARG;
    }
    c->method_lanes = lanes;
    return GECM_OK;
}

int gecm_get_method_lanes(const gecm_ctx *c) { return c && c->method_lanes ? c->method_lanes : 1; }

/* the lanes the next launch on the method batch takes: 1 or 16, or 0 with the error text set (an explicit 16 without
 * constants) */
static int method_lanes_for_launch(gecm_ctx *c)
{
    const int set = gecm_get_method_lanes(c);
    if (set == 1) return 1;
    if (set == GECM_METHOD_LANES_AUTO &&
        gecm_method_lanes_auto(gecm_dev_stride(c->dev), c->mod.nl, gecm_dev_cus(c->dev)) != 16)
        return 1;
    if (rows_on_device(c, ROWC_METHOD) > 0) return 16;
    if (set == GECM_METHOD_LANES_AUTO) return 1;
    set_err("gecm_stage1_extend: the 16-lane method kernel has no constants for this context's numbers "
            "(gecm_set_method_lanes)");
    return 0;
}

/* ---- curve batches of a multi-modulus context in the 32-lane row layout ---------- */
/* Rows up to 32 positions per compute unit, up to 64 at 37 limbs, the default layout beyond: read off the table of
 * DESIGN.md §23 (profiles/multi_rows/time_rows_on.txt against time_parent_default.txt, one MI355X of 256 compute units,
 * gecm_stage1(1e5), kernel time with the canon pass, 32 numbers).  The default launch (k_stage1_pair_multi, k_stage1_lane)
 * takes the same time up to 32,768 positions; the row launch is flat up to 1,024 and grows with the batch from 4,096 on.
 * 15 limbs, wave packing: 240 against 771 ms at 4,096 positions, 439 against 773 at 8,192, and lost at 16,384 (806 against
 * 779).  15 limbs, lane packing: 240 against 1,405 ms at 4,096, still 806 against 1,412 at 16,384, lost at 32,768.  37
 * limbs: 932 against 4,182 ms at 4,096, 3,453 against 4,253 at 16,384, lost at 32,768 (6,804 against 4,406).  Every
 * difference named is far above the min - max spread of both series (under 25 ms).  The rule does not know the packing,
 * so at 15 limbs it stops where wave packing stops winning.  Only 15 and 37 limbs were measured: the limb counts below
 * 15 (8 to 14) and between 15 and 37 take the smaller bound unmeasured. */
int gecm_multi_rows_auto(size_t positions, int dev_limbs, int cus)
{
    if (positions == 0 || cus <= 0) return 0;
    return positions <= (size_t)(dev_limbs >= 37 ? 64 : 32) * (size_t)cus;
}

int gecm_set_multi_rows(gecm_ctx *c, int rows)
{
    if (!c || (rows != GECM_MULTI_ROWS_OFF && rows != GECM_MULTI_ROWS_ON && rows != GECM_MULTI_ROWS_AUTO)) {
        set_err("gecm_set_multi_rows: needs a context and GECM_MULTI_ROWS_OFF, GECM_MULTI_ROWS_ON or GECM_MULTI_ROWS_AUTO");
        return GECM_ERR_ARG;
    }
    if (!c->multi) { set_err("gecm_set_multi_rows: not a multi-modulus context (gecm_create_multi)"); return GECM_ERR_STATE; }
    c->multi_rows = rows;
    return GECM_OK;
}

int gecm_get_multi_rows(const gecm_ctx *c) { return c ? c->multi_rows : GECM_MULTI_ROWS_OFF; }

/* does the next stage-1 launch of the curve batch run the row layout?  1 or 0, or -1 with the error text set (ON
 * without constants); fn names the call in that text.  The setting has a say only while gecm_set_lanes_per_curve is 0. */
static int multi_rows_for_launch(gecm_ctx *c, const char *fn)
{
    if (!c->multi || c->method || c->multi_rows == GECM_MULTI_ROWS_OFF || c->lanes_per_curve) return 0;
    if (c->multi_rows == GECM_MULTI_ROWS_AUTO &&
        !gecm_multi_rows_auto(gecm_dev_stride(c->dev), c->mod.nl, gecm_dev_cus(c->dev)))
        return 0;
    const int have = rows_on_device(c, ROWC_MULTI);
    if (have > 0) return 1;
    if (c->multi_rows == GECM_MULTI_ROWS_AUTO) return 0;
    if (have == -2) set_err("%s: out of memory for the 32-lane kernel's constants", fn);
    else if (have < 0) set_err("%s: the 32-lane kernel's constants could not be put on the device: %s", fn, gecm_dev_error());
    else set_err("%s: the 32-lane kernel has no constants for this context's numbers (gecm_set_multi_rows)", fn);
    return -1;
}

int gecm_create(gecm_ctx **out, int device, const char *n_str, int digitbits)
{
    if (!out || !n_str || (digitbits != 52 && digitbits != 32)) {
        set_err("gecm_create: bad argument (digitbits must be 52 or 32)");
        return GECM_ERR_ARG;
    }
    gecm_ctx *c = (gecm_ctx *)calloc(1, sizeof *c);
    if (!c) return GECM_ERR_NOMEM;
    int rc = gecm_mod_setup(&c->mod, "gecm_create", n_str, digitbits, 0, pick_nl);
    if (rc) { free(c); return rc; }
    c->device = device;
    const gecm_devmod dm = gecm_mod_devmod(&c->mod);
    if (gecm_dev_open(&c->dev, device, c->mod.nl, &dm, 0)) {
        set_err("gecm_create: %s", gecm_dev_error());
        gecm_mod_free(&c->mod);
        free(c);
        return GECM_ERR_DEVICE;
    }
    row_setup(c);
    ff_setup(c);
    *out = c;
    return GECM_OK;
}

/* Wide contexts.  Above the largest built limb count there is one kernel, the 32-lane stage-1 kernel at
 * the wide shapes of csrc/gecm_rowk.h, and no kernel table: the device context is gecm_dev_open_wide's, the curves are built
 * on the host as on any context, and what follows stage 1 — canonical residues, plain x and z, the factor gcds — is
 * gecm_mod.c's work on the raw limbs (fetch_plain, gecm_scan_factors).  An N that gecm_create serves gets gecm_create's
 * context: a caller may use this constructor for every number. */
int gecm_create_wide(gecm_ctx **out, int device, const char *n_str, int digitbits)
{
    mpl_t n;
    if (!out || !n_str || (digitbits != 52 && digitbits != 32) || mpl_set_str(&n, n_str) || pick_nl(mpl_bits(&n)))
        return gecm_create(out, device, n_str, digitbits);          /* its answer, errors included */
    gecm_ctx *c = (gecm_ctx *)calloc(1, sizeof *c);
    if (!c) return GECM_ERR_NOMEM;
    int rc = gecm_mod_setup(&c->mod, "gecm_create_wide", n_str, digitbits, 0, gecm_mod_wide_nl);
    if (rc) { free(c); return rc; }
    c->device = device;
    c->wide = 1;
    row_sets s;
    const int made = row_sets_build(c, ROWC_CURVE, &s);
    if (made < 0) rc = GECM_ERR_NOMEM;
    else if (!made || s.nq != GECM_ROW_MAXNQ) {
        set_err("gecm_create_wide: the 32-lane kernel has no constants for this N at %d limbs", c->mod.nl);
        rc = GECM_ERR_ARG;
    } else if (gecm_dev_open_wide(&c->dev, device, c->mod.nl, c->mod.rho28) || gecm_dev_set_rowconst(c->dev, s.nq, s.rows, s.words)) {
        set_err("gecm_create_wide: %s", gecm_dev_error());
        rc = GECM_ERR_DEVICE;
    }
    free(s.words);
    if (rc) {
        gecm_dev_close(c->dev);
        gecm_mod_free(&c->mod);
        free(c);
        return rc;
    }
    *out = c;
    return GECM_OK;
}

int gecm_is_wide(const gecm_ctx *c) { return c ? c->wide : 0; }

static void free_batch(gecm_ctx *c)
{
    free(c->norm_left);
    c->norm_left = NULL;
    c->normalized = 0;
    free(c->param);
    c->param = NULL;
    free(c->seed);
    c->seed = NULL;
    c->method = GECM_METHOD_ECM;
    free(c->sigma); free(c->bad); free(c->hx); free(c->hz); free(c->hacc); free(c->hfail);
    free(c->flags[0]); free(c->flags[1]); free(c->hg[0]); free(c->hg[1]);
    c->flags[0] = c->flags[1] = NULL;
    c->hg[0] = c->hg[1] = NULL;
    c->scan_valid[0] = c->scan_valid[1] = 0;
    c->sigma = NULL; c->bad = NULL; c->hx = c->hz = NULL; c->hacc = c->hfail = NULL;
    gecm_layout_free(&c->lay);
    c->have_acc = 0; c->s2_ready = 0;
    c->batch = 0;
    c->have_plain = 0;
}

/* the kept pair map of a single-range stage 2 and the device tape made from it */
static void drop_kept_pairmap(gecm_ctx *c)
{
    if (c->pm_valid) gecm_pairmap_release(&c->pm);
    c->pm_valid = 0;
    if (c->tp_valid) free(c->tp.words);
    c->tp_valid = 0;
}

static uint64_t next_tape_id(void)
{
    static uint64_t next_id = 1;                     /* ids only tell tapes apart on the device side */
    return __atomic_fetch_add(&next_id, 1, __ATOMIC_RELAXED);
}

void gecm_destroy(gecm_ctx *c)
{
    if (!c) return;
    gecm_dev_close(c->dev);
    gecm_dev_close(c->dev_l0);
    gecm_dev_close(c->twin.dev);
    if (c->pf_active) { pthread_join(c->pf_thread, NULL); c->pf_active = 0; gecm_tape_free(&c->pf_tape); }
    gecm_tape_free(&c->tape);
    free_batch(c);
    free(c->next_param);
    gecm_s2_plan_free(&c->s2);
    drop_kept_pairmap(c);
    if (c->ptp_valid) free(c->ptp.words);
    gecm_mod_free(&c->mod);
    for (size_t g = 0; g < c->ngroups; g++) gecm_mod_free(&c->grp[g]);
    free(c->grp);
    free(c->grp_dev);
    free(c);
}

/* The reference's special-form runs (main.c:505-527, 642-684) work modulo Mw = 2^k -/+ 1 or 2^k - c — curve construction,
 * stage 1, stage 2 — while the number given, N | Mw, stays the one its files name and its factor checks use
 * (ecm.c:1111-1118: gmpn = vnhat).  A context on Mw with N as its report modulus writes those files byte for byte. */
int gecm_set_report_modulus(gecm_ctx *c, const char *n_str)
{
    if (!c) return GECM_ERR_ARG;
    if (c && c->multi) return multi_refuse("gecm_set_report_modulus");
    if (!n_str) { c->mod.have_report = 0; return GECM_OK; }
    mpl_t r, m;
    if (mpl_set_str(&r, n_str) || mpl_cmp_u64(&r, 1) <= 0) { set_err("gecm_set_report_modulus: bad number"); return GECM_ERR_ARG; }
    mpl_mod(&m, &c->mod.N, &r);
    if (!mpl_is_zero(&m)) { set_err("gecm_set_report_modulus: the number must divide the context's modulus"); return GECM_ERR_ARG; }
    c->mod.N_report = r;
    c->mod.have_report = 1;
    c->scan_valid[0] = c->scan_valid[1] = 0;
    return GECM_OK;
}

int gecm_get_config(const gecm_ctx *c, gecm_config *cfg)
{
    if (!c || !cfg) return GECM_ERR_ARG;
    cfg->digitbits = c->mod.digitbits;
    cfg->nwords = c->mod.nwords;
    cfg->maxbits = c->mod.maxbits;
    cfg->nbits = c->mod.nbits;
    cfg->dev_limbs = c->mod.nl;
    cfg->device = c->device;
    cfg->rho = c->mod.rho_ref;
    return GECM_OK;
}

int gecm_device_memory(gecm_ctx *c, uint64_t *free_bytes, uint64_t *total_bytes)
{
    if (!c) return GECM_ERR_ARG;
    if (gecm_dev_memory(c->dev, free_bytes, total_bytes)) { set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    return GECM_OK;
}

/* Device bytes a batch of `curves` curves takes: the stage-1 arrays and, with_stage2, the stage-2 allocations for wheel D
 * and height U (0 = the defaults for B1) — the baby-step table is the largest allocation of the path.
 * The same sums the device layer allocates by. */
uint64_t gecm_batch_bytes(const gecm_ctx *c, size_t curves, int with_stage2, uint64_t B1, uint32_t D, uint32_t U)
{
    if (!c || !curves || (c->wide && with_stage2)) return 0;
    /* multi-modulus: every modulus's curves padded to whole wavefronts, at most 63 more per modulus that has curves;
     * lane-packed, the batch's tail only (gecm_multi_positions) */
    if (c->multi && c->packing == GECM_PACK_LANE) curves = gecm_multi_positions(&curves, 1, GECM_PACK_LANE);
    else if (c->multi) curves += 63 * (curves < c->ngroups ? curves : c->ngroups);
    uint32_t npb = 0;
    if (with_stage2) {
        if (!D) D = gecm_s2_default_D(B1 ? B1 : 1000000);
        if (!U) U = GECM_S2_DEFAULT_U;
        gecm_s2_plan p;
        memset(&p, 0, sizeof p);
        if (gecm_s2_plan_init(&p, D, U) == 0) {
            npb = p.npb;
            gecm_s2_plan_free(&p);
        }
    }
    uint64_t b = gecm_dev_batch_bytes(c->dev, curves, npb, S2_GIANT_CHUNK, S2_RING);
    if (c->twin.dev) b += gecm_dev_batch_bytes(c->twin.dev, curves, 0, 0, 0);
    return b;
}

int gecm_device_name(gecm_ctx *c, char *buf, size_t len)
{
    if (gecm_dev_device_name(c->dev, buf, len)) { set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    return GECM_OK;
}

/* ---- reference vec layout <-> mpl ---------------------------------------------------------- */
static void vec_get(const gecm_mod *m, mpl_t *r, const void *vec, size_t batch, size_t lane)
{
    if (m->digitbits == 52) mpl_from_limbs64(r, (const uint64_t *)vec + lane, batch, m->nwords, 52);
    else mpl_from_limbs32(r, (const uint32_t *)vec + lane, batch, m->nwords, 32);
}

static void vec_put(const gecm_mod *m, void *vec, size_t batch, size_t lane, const mpl_t *v)
{
    if (m->digitbits == 52) mpl_to_limbs64((uint64_t *)vec + lane, batch, m->nwords, 52, v);
    else mpl_to_limbs32((uint32_t *)vec + lane, batch, m->nwords, 32, v);
}

int gecm_get_one(const gecm_ctx *c, void *one_limbs)
{
    if (c && c->wide) return wide_refuse("gecm_get_one");
    if (!c || !one_limbs) return GECM_ERR_ARG;
    if (c && c->multi) return multi_refuse("gecm_get_one");
    vec_put(&c->mod, one_limbs, 1, 0, &c->mod.rref_mod_n);
    return GECM_OK;
}

/* ---- L0 ------------------------------------------------------------------------------------ */
/* the L0 operators' own device context, opened by the first of them */
static int l0_open(gecm_ctx *c)
{
    if (c->dev_l0) return GECM_OK;
    const gecm_devmod dm = gecm_mod_devmod(&c->mod);
    if (!gecm_dev_open(&c->dev_l0, c->device, c->mod.nl, &dm, 0)) return GECM_OK;
    set_err("L0: %s", gecm_dev_error());
    return GECM_ERR_DEVICE;
}

static int l0_call(gecm_ctx *c, int op, const void *a, const void *b, void *r0, void *r1, size_t batch)
{
    if (c && c->wide) return wide_refuse("the L0 operators");
    if (c && c->multi) return multi_refuse("the L0 operators");
    if (!c || !a || !r0 || batch == 0) { set_err("L0: bad argument"); return GECM_ERR_ARG; }
    if (l0_open(c)) return GECM_ERR_DEVICE;
    int nl = c->mod.nl;
    size_t words = (size_t)nl * batch;
    uint32_t *ha = (uint32_t *)malloc(words * 4 * 4);
    if (!ha) return GECM_ERR_NOMEM;
    uint32_t *hb = ha + words, *hc = hb + words, *hd = hc + words;
    mpl_t v;
    for (size_t i = 0; i < batch; i++) {
        vec_get(&c->mod, &v, a, batch, i);
        if (mpl_cmp(&v, &c->mod.N) >= 0) { free(ha); set_err("L0: operand a[%zu] not < N", i); return GECM_ERR_ARG; }
        mpl_to_limbs32(ha + i, batch, nl, LIMB_BITS, &v);
        if (b) {
            vec_get(&c->mod, &v, b, batch, i);
            if (mpl_cmp(&v, &c->mod.N) >= 0) { free(ha); set_err("L0: operand b[%zu] not < N", i); return GECM_ERR_ARG; }
        }
        mpl_to_limbs32(hb + i, batch, nl, LIMB_BITS, &v);
    }
    int rc = gecm_dev_l0(c->dev_l0, op, ha, hb, hc, hd, batch, c->mod.fix28);
    if (rc) { free(ha); set_err("L0: %s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    for (size_t i = 0; i < batch; i++) {
        mpl_from_limbs32(&v, hc + i, batch, nl, LIMB_BITS);
        vec_put(&c->mod, r0, batch, i, &v);
        if (op == GECM_L0_ADDSUB) {
            mpl_from_limbs32(&v, hd + i, batch, nl, LIMB_BITS);
            vec_put(&c->mod, r1, batch, i, &v);
        }
    }
    free(ha);
    return GECM_OK;
}

int gecm_vecmulmod(gecm_ctx *c, const void *a, const void *b, void *r, size_t batch)
{
    return b ? l0_call(c, GECM_L0_MUL, a, b, r, NULL, batch) : GECM_ERR_ARG;
}
int gecm_vecsqrmod(gecm_ctx *c, const void *a, void *r, size_t batch)
{
    return l0_call(c, GECM_L0_SQR, a, NULL, r, NULL, batch);
}
int gecm_vecaddmod(gecm_ctx *c, const void *a, const void *b, void *r, size_t batch)
{
    return b ? l0_call(c, GECM_L0_ADD, a, b, r, NULL, batch) : GECM_ERR_ARG;
}
int gecm_vecsubmod(gecm_ctx *c, const void *a, const void *b, void *r, size_t batch)
{
    return b ? l0_call(c, GECM_L0_SUB, a, b, r, NULL, batch) : GECM_ERR_ARG;
}
int gecm_vecaddsubmod(gecm_ctx *c, const void *a, const void *b, void *sum, void *diff, size_t batch)
{
    return (b && diff) ? l0_call(c, GECM_L0_ADDSUB, a, b, sum, diff, batch) : GECM_ERR_ARG;
}

/* The device inversion on chosen inputs: fe_inv_mont with this modulus's inv_iters, as every stage-2 batch inversion
 * runs it.  Operands go to the device as they come, in the reference radix; finv28 brings the result back to it. */
int gecm_vecinvmod(gecm_ctx *c, const void *a, void *inv, void *gcd, size_t batch)
{
    if (c && c->wide) return wide_refuse("gecm_vecinvmod");
    if (c && c->multi) return multi_refuse("the L0 operators");
    if (!c || !a || !inv || !gcd || batch == 0) { set_err("L0: bad argument"); return GECM_ERR_ARG; }
    if (l0_open(c)) return GECM_ERR_DEVICE;
    int nl = c->mod.nl;
    size_t words = (size_t)nl * batch;
    uint32_t *ha = (uint32_t *)malloc(words * 4 * 3);
    if (!ha) return GECM_ERR_NOMEM;
    uint32_t *hi = ha + words, *hg = hi + words;
    mpl_t v;
    for (size_t i = 0; i < batch; i++) {
        vec_get(&c->mod, &v, a, batch, i);
        if (mpl_cmp(&v, &c->mod.N) >= 0) { free(ha); set_err("L0: operand a[%zu] not < N", i); return GECM_ERR_ARG; }
        mpl_to_limbs32(ha + i, batch, nl, LIMB_BITS, &v);
    }
    int rc = gecm_dev_l0_inv(c->dev_l0, ha, hi, hg, batch, c->mod.finv28);
    if (rc) { free(ha); set_err("L0: %s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    for (size_t i = 0; i < batch; i++) {
        mpl_from_limbs32(&v, hi + i, batch, nl, LIMB_BITS);
        vec_put(&c->mod, inv, batch, i, &v);
        mpl_from_limbs32(&v, hg + i, batch, nl, LIMB_BITS);
        vec_put(&c->mod, gcd, batch, i, &v);
    }
    free(ha);
    return GECM_OK;
}

/* The field functions themselves on the caller's limbs (include/gecm.h): sizes and state are checked, the values are
 * not, and nothing is converted on the way in or out. */
int gecm_vecrawop(gecm_ctx *c, int target, int op, const uint32_t *a, const uint32_t *b, uint32_t *r, size_t count)
{
    if (c && c->wide) return wide_refuse("gecm_vecrawop");
    const int one_operand = op == GECM_RAW_SQR || op == GECM_RAW_CONDSUB;
    if (!c || !a || !r || count == 0 || op < GECM_RAW_MUL || op > GECM_RAW_CONDSUB || (!b && !one_operand)) {
        set_err("gecm_vecrawop: bad argument");
        return GECM_ERR_ARG;
    }
    /* GECM_RAW_MUL .. _SUB are the device layer's codes; CONDSUB has one of its own */
    const int dev_op = op == GECM_RAW_CONDSUB ? GECM_L0_CONDSUB : op;
    gecm_dev *dev = NULL;
    if (target == GECM_RAW_BATCH) {
        if (!c->multi || c->batch == 0 || c->packing_used != GECM_PACK_LANE || count != c->batch) {
            set_err("gecm_vecrawop: GECM_RAW_BATCH needs the lane-packed batch of a multi-modulus context and one residue per "
                    "position of it (%zu)", c->multi ? c->batch : (size_t)0);
            return c->multi && c->batch && c->packing_used == GECM_PACK_LANE ? GECM_ERR_ARG : GECM_ERR_STATE;
        }
        dev = c->dev;
    } else if (c->multi) {
        return multi_refuse("gecm_vecrawop on one modulus");
    } else if (target == GECM_RAW_TWIN) {
        if (!c->twin.dev) { set_err("gecm_vecrawop: this N has no special-form twin (gecm_get_special_form)"); return GECM_ERR_STATE; }
        dev = c->twin.dev;
    } else if (target == GECM_RAW_OWN) {
        if (l0_open(c)) return GECM_ERR_DEVICE;
        dev = c->dev_l0;
    } else {
        set_err("gecm_vecrawop: bad target");
        return GECM_ERR_ARG;
    }
    if (gecm_dev_l0_raw(dev, dev_op, target == GECM_RAW_TWIN, a, one_operand ? NULL : b, r, count)) {
        set_err("gecm_vecrawop: %s", gecm_dev_error());
        return GECM_ERR_DEVICE;
    }
    return GECM_OK;
}

/* ---- phase 0 -------------------------------------------------------------------------------- */
/* The one-shot setting of gecm_set_next_params belongs to the build call that follows it, whether that call succeeds
 * or not: the call reads c->next_param where it needs it (seeds do not) and returns through here, which drops the
 * setting.  gecm_upload_points alone leaves it pending. */
static int build_call_end(gecm_ctx *c, int rc)
{
    if (c) {
        free(c->next_param);
        c->next_param = NULL;
        c->next_batch = 0;
    }
    return rc;
}

/* the checks of a build call on its sigmas, before the context gives up its batch: the pending setting is for this
 * batch size, sigma >= 6 for the PARAM 0 curves, the range of the parametrisation for the others (no setting pending:
 * PARAM 0 throughout) */
static int params_fit(const gecm_ctx *c, const char *who, size_t batch)
{
    if (!c->next_param || c->next_batch == batch) return GECM_OK;
    set_err("%s: gecm_set_next_params gave the parametrisations of %zu curves, this batch has %zu", who, c->next_batch, batch);
    return GECM_ERR_ARG;
}

static int sigma_arg(const char *who, const uint64_t *sigma, size_t i, const uint8_t *prm)
{
    if (prm && prm[i]) {
        if (gecm_mod_param_sigma_ok(prm[i], sigma[i])) return GECM_OK;
        set_err("%s: SIGMA: sigma[%zu] = %llu is outside [1, 2^%d), the range of PARAM %d", who, i,
                (unsigned long long)sigma[i], prm[i] == GECM_PARAM_BATCH_SQUARE ? 64 : 32, prm[i]);
        return GECM_ERR_ARG;
    }
    if (sigma[i] < 6) { set_err("%s: sigma[%zu] < 6", who, i); return GECM_ERR_ARG; }
    return GECM_OK;
}

/* the checks gecm_build_curves and gecm_resume_points make on their common arguments */
static int sigma_args(const gecm_ctx *c, const char *who, const uint64_t *sigma, size_t batch)
{
    if (!c || !sigma || batch == 0) { set_err("%s: bad argument", who); return GECM_ERR_ARG; }
    if (c->multi) return multi_refuse(who);
    int rc = params_fit(c, who, batch);
    for (size_t i = 0; i < batch && !rc; i++) rc = sigma_arg(who, sigma, i, c->next_param);
    return rc;
}

int gecm_set_next_params(gecm_ctx *c, const uint8_t *param, size_t batch)
{
    if (param) {
        if (batch == 0) { set_err("gecm_set_next_params: bad argument (an empty batch)"); return GECM_ERR_ARG; }
        for (size_t i = 0; i < batch; i++)
            if (param[i] != GECM_PARAM_SUYAMA && param[i] != GECM_PARAM_BATCH_SQUARE && param[i] != GECM_PARAM_BATCH_32) {
                set_err("gecm_set_next_params: param[%zu] = %d: a parametrisation is 0 (Suyama), 1 (sigma^2 / 2^64) or 3 "
                        "(sigma / 2^32)", i, param[i]);
                return GECM_ERR_ARG;
            }
    }
    if (!c) { set_err("gecm_set_next_params: bad argument (no context)"); return GECM_ERR_ARG; }
    build_call_end(c, 0);
    if (!param) return GECM_OK;
    c->next_param = (uint8_t *)malloc(batch);
    if (!c->next_param) return GECM_ERR_NOMEM;
    memcpy(c->next_param, param, batch);
    c->next_batch = batch;
    return GECM_OK;
}

/* ---- how a batch is constructed -----------------------------------------------
 * Every call that puts a batch into a context checks its arguments, describes the batch and hands the description to
 * batch_build, which is five steps: lay the batch out, begin it, fill it, overlay plain residues, finish it. */
typedef enum {
    BATCH_CURVES,       /* X, Z, S are the curves constructed from sigma */
    BATCH_MONT,         /* planes = X, Z, S in Montgomery form: gecm_upload_points */
    BATCH_PLAIN         /* planes = plain x, z in [0, N): resumed points over the curves of sigma, or seeds without any */
} batch_content;

typedef struct {
    const char *who;                 /* the entry point, for the error texts */
    size_t batch;                    /* the caller's curves; every array below is [batch] or [nl][batch] in its order */
    const uint64_t *sigma;           /* a curve is constructed from each; NULL: the batch has no sigmas (and S stays unset) */
    const uint32_t *modulus_index;   /* the modulus of every curve of a multi-modulus context; NULL on a single-N one */
    const uint8_t *param;            /* the parametrisation of every sigma; NULL: PARAM 0 throughout */
    batch_content content;
    const uint32_t *planes;          /* what `content` says, [nl][batch] each; NULL for BATCH_CURVES */
    int method;                      /* GECM_METHOD_ECM, or what the residues of a seed batch are for */
    const uint32_t *seed;            /* the plain x0 plane a seed batch keeps; NULL: unknown */
} batch_desc;

static inline size_t batch_pos(const gecm_ctx *c, size_t i) { return c->multi ? c->lay.slot[i] : i; }

/* one [nl][nuser] plane in the caller's order into position order, stride c->batch; the padding is left as it is */
static void scatter_plane(const gecm_ctx *c, uint32_t *dst, const uint32_t *src, size_t nuser)
{
    for (size_t i = 0; i < nuser; i++) {
        const size_t p = batch_pos(c, i);
        for (size_t l = 0; l < (size_t)c->mod.nl; l++) dst[l * c->batch + p] = src[l * nuser + i];
    }
}

static int alloc_batch(gecm_ctx *c, size_t batch)
{
    free_batch(c);
    c->sigma = (uint64_t *)calloc(batch, sizeof(uint64_t));
    c->bad = (uint8_t *)calloc(batch, 1);
    c->hx = (uint32_t *)calloc(batch * (size_t)c->mod.nl, 4);
    c->hz = (uint32_t *)calloc(batch * (size_t)c->mod.nl, 4);
    c->hacc = (uint32_t *)calloc(batch * (size_t)c->mod.nl, 4);
    c->hfail = (uint32_t *)calloc(batch * (size_t)c->mod.nl, 4);
    c->fail_planes = 1;
    if (!c->sigma || !c->bad || !c->hx || !c->hz || !c->hacc || !c->hfail) return GECM_ERR_NOMEM;
    c->batch = batch;
    c->twin.pending = 0;
    c->twin.loaded = 0;
    if (gecm_dev_resize(c->dev, batch) || (c->twin.dev && gecm_dev_resize(c->twin.dev, batch))) return GECM_ERR_DEVICE;
    return GECM_OK;
}

/* Step 2: the previous batch goes, the context takes the layout (`lay` is empty afterwards; all zero for a single-N
 * batch) and arrays for its positions, on the host and on the device; sigma and param go into position order, the
 * padding's stay 0. */
static int batch_begin(gecm_ctx *c, const batch_desc *d, gecm_layout *lay)
{
    const int rc = alloc_batch(c, c->multi ? lay->total : d->batch);
    c->lay = *lay;
    memset(lay, 0, sizeof *lay);
    if (rc) return rc;
    if (d->param && !(c->param = (uint8_t *)calloc(c->batch, 1))) return GECM_ERR_NOMEM;
    for (size_t i = 0; i < d->batch; i++) {
        const size_t p = batch_pos(c, i);
        if (d->sigma) c->sigma[p] = d->sigma[i];
        if (d->param) c->param[p] = d->param[i];
    }
    return GECM_OK;
}

/* The batch's moduli and which goes where, to the device (a multi-modulus context; once per batch, after its resize):
 * the block table under wave packing, the per-position table under lane packing. */
static int groups_to_device(gecm_ctx *c)
{
    const gecm_layout *l = &c->lay;
    if (!c->multi) return GECM_OK;
    return gecm_dev_set_groups(c->dev, (uint32_t)c->ngroups, c->grp_dev, l->blocks, l->blocks ? NULL : l->pos_grp) ? GECM_ERR_DEVICE : GECM_OK;
}

/* Step 3, curves on the host: the construction modulus by modulus on the worker threads (a single-N batch: its one
 * modulus at position 0), uploaded; the padding stays zero: computed, never read.  1 if some curve is marked bad. */
static int fill_on_host(gecm_ctx *c)
{
    const size_t words = (size_t)c->mod.nl * c->batch;
    uint32_t *h = (uint32_t *)calloc(words * 3, 4);
    if (!h) return GECM_ERR_NOMEM;
    int rc = 0, anybad = 0;
    for (size_t g = 0; g < (c->multi ? c->ngroups : 1) && rc >= 0; g++) {
        const size_t off = c->multi ? c->lay.goff[g] : 0;
        gecm_mod_build b = {c->multi ? &c->grp[g] : &c->mod, c->sigma + off, c->bad, c->batch, off, h, h + words, h + 2 * words,
                            c->param ? c->param + off : NULL};
        rc = run_slices(c->multi ? c->lay.cnt[g] : c->batch, gecm_mod_build_slice, &b);
        anybad |= rc > 0;
    }
    if (rc >= 0) rc = gecm_dev_upload(c->dev, h, h + words, h + 2 * words) ? GECM_ERR_DEVICE : groups_to_device(c);
    free(h);
    return rc < 0 ? rc : anybad;
}

/* Step 3, curves on the device (gecm_set_curve_build): the kernels read the moduli just set and c->sigma, c->param in
 * position order; c->bad from their flags, the padding's does not count.  1 if some curve is flagged. */
static int fill_on_device(gecm_ctx *c)
{
    if (groups_to_device(c)) return GECM_ERR_DEVICE;
    uint32_t *flags = (uint32_t *)malloc(c->batch * sizeof(uint32_t));
    if (!flags) return GECM_ERR_NOMEM;
    /* with a parametrisation per curve: the Suyama kernel if some curve is PARAM 0, then k_build_param over the others */
    if (c->param ? gecm_dev_build_param(c->dev, c->sigma, c->param, c->batch, flags) : gecm_dev_build(c->dev, c->sigma, c->batch, flags)) {
        free(flags);
        return GECM_ERR_DEVICE;
    }
    int any = 0;
    for (size_t p = 0; p < c->batch; p++)
        if (flags[p] && !(c->multi && c->lay.pos_user[p] == GECM_PAD)) c->bad[p] = (uint8_t)(any = 1);
    free(flags);
    c->last_ms = gecm_dev_last_build_ms(c->dev);
    return any;
}

/* Step 3: what X, Z, S hold first.  Curves where the batch has sigmas, built where gecm_set_curve_build says; else
 * the planes given in Montgomery form, or nothing before step 4. */
static int batch_fill(gecm_ctx *c, const batch_desc *d)
{
    if (d->sigma) return c->build_where == GECM_BUILD_DEVICE ? fill_on_device(c) : fill_on_host(c);
    if (d->content == BATCH_MONT) {
        const size_t words = (size_t)c->mod.nl * c->batch;
        if (gecm_dev_upload(c->dev, d->planes, d->planes + words, d->planes + 2 * words)) return GECM_ERR_DEVICE;
    }
    return groups_to_device(c);
}

/* Step 4: X, Z replaced by the Montgomery forms of the plain residues given, made on the device; a multi-modulus
 * batch through its layout, the padding with x = z = 1. */
static int batch_overlay(gecm_ctx *c, const batch_desc *d)
{
    if (d->content != BATCH_PLAIN) return GECM_OK;
    const size_t words = (size_t)c->mod.nl * c->batch;
    const uint32_t *x = d->planes, *z = d->planes + (size_t)c->mod.nl * d->batch;
    uint32_t *h = NULL;
    if (c->multi) {
        if (!(h = (uint32_t *)calloc(words * 2, 4))) return GECM_ERR_NOMEM;
        scatter_plane(c, h, x, d->batch);
        scatter_plane(c, h + words, z, d->batch);
        for (size_t p = 0; p < c->batch; p++)
            if (c->lay.pos_user[p] == GECM_PAD) h[p] = h[words + p] = 1;
        x = h;
        z = h + words;
    }
    const int rc = gecm_dev_upload_plain(c->dev, x, z) ? GECM_ERR_DEVICE : GECM_OK;
    free(h);
    return rc;
}

/* Step 5: the twin from what the main context now holds (curves on a single-N context; a multi-modulus context has
 * none), the seeds in position order, and what the batch was made with.  A wart kept as it was: build_used follows
 * build_where after every batch with sigmas and every multi-modulus batch, so gecm_get_curve_build answers the
 * asked-for place after gecm_build_seeds_multi and the previous batch's after gecm_build_seeds (and
 * gecm_upload_points). */
static int batch_finish(gecm_ctx *c, const batch_desc *d)
{
    if (!d->method && twin_fill(c)) return GECM_ERR_DEVICE;
    if (d->seed) {
        if (!(c->seed = (uint32_t *)calloc((size_t)c->mod.nl * c->batch, 4))) return GECM_ERR_NOMEM;
        scatter_plane(c, c->seed, d->seed, d->batch);
    }
    c->method = d->method;
    if (c->multi) c->packing_used = c->packing;
    if (d->sigma || c->multi) c->build_used = c->build_where;
    return GECM_OK;
}

/* The batch `d` describes into the context; the caller has checked d's arrays.  1 if some constructed curve is marked
 * bad, GECM_OK, or an error: before the previous batch is given up while the batch is laid out, afterwards with no
 * batch left and, for a device error, "<who>: <the device layer's text>". */
static int batch_build(gecm_ctx *c, const batch_desc *d)
{
    gecm_layout lay;
    memset(&lay, 0, sizeof lay);
    if (c->multi) {                                   /* step 1 */
        if (d->sigma && c->packing == GECM_PACK_LANE && c->build_where == GECM_BUILD_DEVICE) {
            set_err("%s: the device curve build has no per-lane kernel: a lane-packed context builds on the host "
                    "(gecm_set_curve_build, gecm_set_multi_packing)", d->who);
            return GECM_ERR_STATE;
        }
        const int rc = gecm_layout_make(&lay, d->modulus_index, d->batch, c->ngroups, c->packing);
        if (rc) return rc;
    }
    int rc = batch_begin(c, d, &lay), anybad = 0;
    if (!rc && (rc = batch_fill(c, d)) > 0) { anybad = 1; rc = GECM_OK; }
    if (!rc) rc = batch_overlay(c, d);
    if (!rc) rc = batch_finish(c, d);
    if (!rc) return anybad;
    if (rc == GECM_ERR_DEVICE) set_err("%s: %s", d->who, gecm_dev_error());
    free_batch(c);
    return rc;
}

int gecm_build_curves(gecm_ctx *c, const uint64_t *sigma, size_t batch)
{
    /* inputs are checked before the context takes the new batch: after an error it holds no batch at all (the
     * phase functions then return GECM_ERR_STATE instead of running on memory nothing was uploaded to) */
    int rc = sigma_args(c, "gecm_build_curves", sigma, batch);
    if (!rc && c->wide && c->build_where == GECM_BUILD_DEVICE) rc = wide_refuse("gecm_build_curves on the device (gecm_set_curve_build)");
    if (!rc) rc = batch_build(c, &(batch_desc){.who = "gecm_build_curves", .batch = batch, .sigma = sigma, .param = c->next_param});
    return build_call_end(c, rc);
}

int gecm_set_curve_build(gecm_ctx *c, int where)
{
    if (!c || (where != GECM_BUILD_HOST && where != GECM_BUILD_DEVICE)) {
        set_err("gecm_set_curve_build: bad argument (GECM_BUILD_HOST or GECM_BUILD_DEVICE)");
        return GECM_ERR_ARG;
    }
    c->build_where = where;
    return GECM_OK;
}

int gecm_get_curve_build(const gecm_ctx *c) { return c ? c->build_used : GECM_ERR_ARG; }

/* X, Z, s in the reference's Montgomery radix as planes of the internal one, [3][nl][batch]; NULL: *rc and the text say why */
static uint32_t *upload_planes(const gecm_ctx *c, const void *X, const void *Z, const void *s, size_t batch, int *rc)
{
    const size_t words = (size_t)c->mod.nl * batch;
    uint32_t *h = (uint32_t *)calloc(words * 3, 4);
    const void *src[3] = {X, Z, s};
    *rc = GECM_ERR_NOMEM;
    if (!h) return NULL;
    for (int k = 0; k < 3; k++)
        for (size_t i = 0; i < batch; i++) {
            mpl_t v;
            vec_get(&c->mod, &v, src[k], batch, i);
            if (mpl_cmp(&v, &c->mod.N) >= 0) {
                free(h);
                set_err("gecm_upload_points: operand not < N");
                *rc = GECM_ERR_ARG;
                return NULL;
            }
            mpl_mulmod(&v, &v, &c->mod.ref_to_int, &c->mod.N);
            mpl_to_limbs32(h + (size_t)k * words + i, batch, c->mod.nl, LIMB_BITS, &v);
        }
    return h;
}

/* the one build call a pending gecm_set_next_params setting passes by: it waits for the next of the others */
int gecm_upload_points(gecm_ctx *c, const void *X, const void *Z, const void *s, size_t batch)
{
    if (c && c->wide) return wide_refuse("gecm_upload_points");
    if (!c || !X || !Z || !s || batch == 0) { set_err("gecm_upload_points: bad argument"); return GECM_ERR_ARG; }
    if (c->multi) return multi_refuse("gecm_upload_points");
    int rc;
    uint32_t *h = upload_planes(c, X, Z, s, batch, &rc);
    if (!h) free_batch(c);                     /* the context holds no batch after a rejected upload */
    else rc = batch_build(c, &(batch_desc){.who = "gecm_upload_points", .batch = batch, .content = BATCH_MONT, .planes = h});
    free(h);
    return rc;
}

/* ---- phase 1 -------------------------------------------------------------------------------- */
static void *prefetch_run(void *arg)
{
    gecm_ctx *c = (gecm_ctx *)arg;
    c->pf_rc = tape_build(&c->pf_tape, &c->pf_k, host_threads());
    return NULL;
}

/* the tape of key k into c->tape: kept from the last call, taken from the helper thread that compiled it while the
 * device ran the launch before, or compiled now */
static int tape_for(gecm_ctx *c, const tape_key *k)
{
    if (c->tape.ops && key_eq(&c->tape_k, k)) return GECM_OK;
    int rc;
    if (c->pf_active) {
        pthread_join(c->pf_thread, NULL);
        c->pf_active = 0;
        if (!c->pf_rc && key_eq(&c->pf_k, k)) {
            gecm_tape_free(&c->tape);
            c->tape = c->pf_tape;
            memset(&c->pf_tape, 0, sizeof c->pf_tape);
            c->tape_k = *k;
            return GECM_OK;
        }
        gecm_tape_free(&c->pf_tape);
    }
    gecm_tape_free(&c->tape);
    rc = tape_build(&c->tape, k, host_threads());
    if (rc) { set_err("gecm_stage1: tape build failed (%d)", rc); return rc == -1 ? GECM_ERR_NOMEM : GECM_ERR_STATE; }
    c->tape_k = *k;
    return GECM_OK;
}

int gecm_stage1_ranges(uint64_t B1) { return (int)gecm_stage1_ranges_u(B1); }

int gecm_stage1_describe_range(uint64_t B1, uint64_t B2, uint32_t range, gecm_stage1_range_desc *out)
{
    gecm_range_info ri;
    if (!out || B1 < 2 || B1 > GECM_B1_MAX) { set_err("gecm_stage1_describe_range: bad argument"); return GECM_ERR_ARG; }
    int rc = gecm_stage1_range_info(&ri, B1, B2, range);
    if (rc) { set_err("gecm_stage1_describe_range: %s", rc == -1 ? "out of memory" : "no such range"); return rc == -1 ? GECM_ERR_NOMEM : GECM_ERR_ARG; }
    out->lo = ri.lo; out->hi = ri.hi; out->nprimes = ri.nprimes; out->first_prime = ri.first_prime;
    out->last_prime = ri.last_prime; out->checkpoint = ri.exhausted;
    return GECM_OK;
}

/* lane packing's refusal of two lanes per curve, with the error text set */
static int lane_packing_refuses(const gecm_ctx *c)
{
    if (!(c->multi && c->packing_used == GECM_PACK_LANE && c->lanes_per_curve == 2)) return 0;
    set_err("gecm_stage1: a lane-packed multi-modulus batch runs one lane per curve, and this context is set to 2 "
            "(gecm_set_lanes_per_curve)");
    return 1;
}

/* a device call failed: its text is the error */
static int dev_failed(void)
{
    set_err("%s", gecm_dev_error());
    return GECM_ERR_DEVICE;
}

/* Does the next launch of the curve batch run on the special-form twin?  For a batch small enough for the eight-lane
 * layout (generic moduli only) that layout beats the special multiply in its two-lane form: 1.5x against 1.4x at 15
 * limbs, 2.2-2.4x at 30-37 limbs. */
static int twin_takes_launch(const gecm_ctx *c)
{
    const int want = c->lanes_per_curve ? c->lanes_per_curve : gecm_dev_auto_lanes(c->dev);
    return c->twin.dev && c->twin.on && c->twin.loaded && want != 8 && want != 32;
}

/* One stage-1 launch, of a reference range or of an extension segment: the tape of `key` onto the device (and onto the
 * special-form twin when it runs there), the counters (`first`: they start again), the context's B1 afterwards, every
 * cached result of the points dropped, the kernel started, and — next != NULL — the tape of the launch to follow
 * handed to the helper thread.  An extension segment in which no prime gains a power has an empty tape and launches
 * nothing.  The caller has checked its arguments and settled a pending twin. */
static int stage1_launch(gecm_ctx *c, const tape_key *key, uint64_t B1, int first, const tape_key *next)
{
    const int unit_lanes = c->method ? method_lanes_for_launch(c) : 1;
    if (!unit_lanes) return GECM_ERR_STATE;          /* before anything of the batch has changed */
    const int multi_rows = multi_rows_for_launch(c, key->kind == 1 ? "gecm_stage1_extend" : "gecm_stage1");
    if (multi_rows < 0) return GECM_ERR_STATE;
    int rc = tape_for(c, key);
    if (rc) return rc;
    const int idle = key->kind == 1 && c->tape.len == 0;
    if (!idle && !key_eq(&c->dev_tape_k, key)) {
        /* stream-ordered after the kernel of the range before; returns when the copy is done */
        if (gecm_dev_set_tape(c->dev, c->tape.ops, c->tape.len)) return dev_failed();
        c->dev_tape_k = *key;
    }
    if (first) c->s1_ptadds = c->s1_ptdups = 0;
    c->s1_ptadds += c->tape.ptadds;
    c->s1_ptdups += c->tape.ptdups;
    c->s1_last_prime = c->tape.last_prime;
    c->s1_tape_len = c->tape.len;
    c->B1 = B1;
    c->have_plain = 0;
    c->have_acc = 0;
    c->s2_ready = 0;
    c->normalized = 0;
    c->scan_valid[0] = c->scan_valid[1] = 0;
    if (idle) return GECM_OK;
    int failed;
    if (c->method) {                 /* one residue per lane or per row, generic multiply: no curve layouts, no twin */
        c->twin.ran_last = 0;
        failed = gecm_dev_stage1_unit_lanes(c->dev, unit_method(c), unit_lanes);
    } else if (multi_rows) {         /* a multi-modulus context has no twin */
        c->twin.ran_last = 0;
        failed = gecm_dev_stage1_multi_rows(c->dev);
    } else if (twin_takes_launch(c)) {
        /* N | 2^k - 1: run the chain modulo 2^k - 1 with the F-form multiply; ff_settle brings X, Z back */
        failed = !key_eq(&c->twin.tape_k, key) && gecm_dev_set_tape(c->twin.dev, c->tape.ops, c->tape.len);
        if (!failed) {
            c->twin.tape_k = *key;
            failed = gecm_dev_stage1(c->twin.dev, c->lanes_per_curve);
        }
        if (!failed) c->twin.pending = c->twin.ran_last = 1;
    } else {
        c->twin.ran_last = 0;
        c->twin.loaded = 0;          /* the F-form copy of the points no longer matches */
        failed = gecm_dev_stage1(c->dev, c->lanes_per_curve);
    }
    if (failed) return dev_failed();
    if (next && !c->pf_active) {
        /* while the device runs this range: the next one's tape (2 s of host time per 1e8 primes on 8 threads) */
        c->pf_k = *next;
        c->pf_rc = 0;
        c->pf_active = pthread_create(&c->pf_thread, NULL, prefetch_run, c) == 0;
    }
    return GECM_OK;
}

int gecm_stage1_range(gecm_ctx *c, uint64_t B1, uint32_t range)
{
    const int settled = ff_settle(c);
    if (settled) return settled;
    if (!c || c->batch == 0) { set_err("gecm_stage1: no curves uploaded"); return GECM_ERR_STATE; }
    if (method_refuse(c, "gecm_stage1", 0)) return GECM_ERR_STATE;
    if (B1 < 2 || B1 > GECM_B1_MAX) { set_err("gecm_stage1: B1 must be in [2, %llu]", (unsigned long long)GECM_B1_MAX); return GECM_ERR_ARG; }
    if (lane_packing_refuses(c)) return GECM_ERR_STATE;
    if (c->wide && c->lanes_per_curve != 0 && c->lanes_per_curve != 32) {
        set_err("gecm_stage1: a wide context (gecm_create_wide) runs 32 lanes per curve, and this context is set to %d "
                "(gecm_set_lanes_per_curve)", c->lanes_per_curve);
        return GECM_ERR_STATE;
    }
    const uint32_t nranges = gecm_stage1_ranges_u(B1);
    if (range >= nranges) { set_err("gecm_stage1_range: B1 = %llu has %u prime range(s)", (unsigned long long)B1, nranges); return GECM_ERR_ARG; }
    const tape_key key = {0, B1, range}, next = {0, B1, (uint64_t)range + 1};
    return stage1_launch(c, &key, B1, range == 0, range + 1 < nranges ? &next : NULL);
}

/* ---- extension with the standard multiplier ---------------------------------- */
static int extend_args(const char *fn, uint64_t from, uint64_t to)
{
    if (from < 1 || to < from || to > GECM_B1_MAX) {
        set_err("%s: need 1 <= from <= to <= %llu", fn, (unsigned long long)GECM_B1_MAX);
        return GECM_ERR_ARG;
    }
    return GECM_OK;
}

int gecm_stage1_extend_segments(uint64_t from, uint64_t to)
{
    int rc = extend_args("gecm_stage1_extend_segments", from, to);
    return rc ? rc : (int)gecm_extend_segments_plan(from, to);
}

int gecm_stage1_describe_extend(uint64_t from, uint64_t to, uint32_t seg, gecm_extend_desc *out)
{
    gecm_extend_info ei;
    int rc = extend_args("gecm_stage1_describe_extend", from, to);
    if (rc) return rc;
    if (!out) { set_err("gecm_stage1_describe_extend: bad argument"); return GECM_ERR_ARG; }
    rc = gecm_extend_segment_info(&ei, from, to, seg);
    if (rc) { set_err("gecm_stage1_describe_extend: %s", rc == -1 ? "out of memory" : "no such segment"); return rc == -1 ? GECM_ERR_NOMEM : GECM_ERR_ARG; }
    out->lo = ei.lo; out->hi = ei.hi; out->nprimes = ei.nprimes; out->power_steps = ei.power_steps; out->last_prime = ei.last_prime;
    return GECM_OK;
}

int gecm_stage1_extend_segment(gecm_ctx *c, uint64_t from, uint64_t to, uint32_t seg)
{
    if (c && c->wide) return wide_refuse("gecm_stage1_extend_segment");
    const int settled = ff_settle(c);
    if (settled) return settled;
    int rc = extend_args("gecm_stage1_extend", from, to);
    if (rc) return rc;
    if (!c || c->batch == 0) { set_err("gecm_stage1_extend: no curves uploaded"); return GECM_ERR_STATE; }
    if (!c->method && lane_packing_refuses(c)) return GECM_ERR_STATE;
    const uint32_t nseg = gecm_extend_segments_plan(from, to);
    if (seg >= nseg) { set_err("gecm_stage1_extend_segment: the extension from %llu to %llu has %u segment(s)", (unsigned long long)from, (unsigned long long)to, nseg); return GECM_ERR_ARG; }
    tape_key key = {1, 0, 0}, next = {1, 0, 0};
    gecm_extend_segment_bounds(from, to, seg, &key.a, &key.b);
    if (seg + 1 < nseg) gecm_extend_segment_bounds(from, to, seg + 1, &next.a, &next.b);
    /* the context's B1 is the segment's hi: the points are complete to it, whatever follows */
    return stage1_launch(c, &key, key.b, seg == 0, seg + 1 < nseg ? &next : NULL);
}

int gecm_stage1_extend(gecm_ctx *c, uint64_t from, uint64_t to)
{
    int rc = extend_args("gecm_stage1_extend", from, to);
    if (rc) return rc;
    const uint32_t nseg = gecm_extend_segments_plan(from, to);
    for (uint32_t s = 0; s < nseg; s++)
        if ((rc = gecm_stage1_extend_segment(c, from, to, s)) != 0) return rc;
    return GECM_OK;
}

int gecm_stage1(gecm_ctx *c, uint64_t B1)
{
    if (B1 < 2 || B1 > GECM_B1_MAX) { set_err("gecm_stage1: B1 must be in [2, %llu]", (unsigned long long)GECM_B1_MAX); return GECM_ERR_ARG; }
    const uint32_t nranges = gecm_stage1_ranges_u(B1);
    for (uint32_t r = 0; r < nranges; r++) {             /* ecm.c:1209-1234 */
        int rc = gecm_stage1_range(c, B1, r);
        if (rc) return rc;
    }
    return GECM_OK;
}

int gecm_set_special_form(gecm_ctx *c, int on)
{
    if (!c) return GECM_ERR_ARG;
    if (c && c->multi) return multi_refuse("gecm_set_special_form");
    c->twin.on = on != 0;
    return GECM_OK;
}

int gecm_get_special_form(const gecm_ctx *c, int *k, int *limbs)
{
    if (!c) return GECM_ERR_ARG;
    if (k) *k = c->twin.dev ? c->twin.k * c->twin.sign : 0;
    if (limbs) *limbs = c->twin.dev ? c->twin.nl : 0;
    if (!c->twin.dev || !c->twin.on) return 0;
    return c->twin.ran_last ? 2 : 1;
}

int gecm_set_lanes_per_curve(gecm_ctx *c, int lanes)
{
    if (!c || (lanes != 0 && lanes != 1 && lanes != 2 && lanes != 8 && lanes != 32)) {
        set_err("gecm_set_lanes_per_curve: lanes must be 0 (auto), 1, 2, 8 or 32");
        return GECM_ERR_ARG;
    }
    if (c->multi && lanes != 0 && lanes != 1 && lanes != 2) {
        set_err("gecm_set_lanes_per_curve: a multi-modulus context runs with 0 (auto), 1 or 2 lanes per curve");
        return GECM_ERR_ARG;
    }
    c->lanes_per_curve = lanes;
    return GECM_OK;
}

int gecm_get_lanes_per_curve(const gecm_ctx *c)
{
    if (!c) return GECM_ERR_ARG;
    return gecm_dev_last_lanes(last_dev(c));
}

int gecm_stage1_progress(const gecm_ctx *c, uint32_t *done, uint32_t *total)
{
    if (!c) return GECM_ERR_ARG;
    return gecm_dev_stage1_progress(last_dev(c), done, total) ? GECM_ERR_DEVICE : GECM_OK;
}

int gecm_last_kernel_name(const gecm_ctx *c, char *buf, size_t len)
{
    if (!c || !buf || !len) return GECM_ERR_ARG;
    snprintf(buf, len, "%s", gecm_dev_last_kernel(last_dev(c)));
    return GECM_OK;
}

int gecm_sync(gecm_ctx *c)
{
    if (!c) return GECM_ERR_ARG;
    if (c->twin.pending) return ff_settle(c);
    if (gecm_dev_sync(c->dev)) { set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    c->last_ms = gecm_dev_last_kernel_ms(c->dev);
    return GECM_OK;
}

double gecm_last_kernel_ms(const gecm_ctx *c) { return c ? c->last_ms : 0.0; }

int gecm_get_stage1_stats(const gecm_ctx *c, gecm_stage1_stats *st)
{
    if (!c || !st || !c->tape.ops) return GECM_ERR_STATE;
    st->ptadds = c->s1_ptadds;
    st->ptdups = c->s1_ptdups;
    st->last_prime = c->s1_last_prime;
    st->tape_len = c->s1_tape_len;
    return GECM_OK;
}

int gecm_download_points(gecm_ctx *c, void *X, void *Z)
{
    if (c && c->wide) return wide_refuse("gecm_download_points");
    if (c && c->multi) return multi_refuse("gecm_download_points");
    const int settled = ff_settle(c);
    if (settled) return settled;
    if (!c || !X || !Z || c->batch == 0) return GECM_ERR_ARG;
    size_t batch = c->batch, words = (size_t)c->mod.nl * batch;
    uint32_t *h = (uint32_t *)malloc(words * 2 * 4);
    if (!h) return GECM_ERR_NOMEM;
    if (gecm_dev_download_mont(c->dev, h, h + words)) { free(h); set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    void *dst[2] = {X, Z};
    for (int k = 0; k < 2; k++)
        for (size_t i = 0; i < batch; i++) {
            mpl_t v;
            mpl_from_limbs32(&v, h + (size_t)k * words + i, batch, c->mod.nl, LIMB_BITS);
            mpl_mulmod(&v, &v, &c->mod.int_to_ref, &c->mod.N);
            vec_put(&c->mod, dst[k], batch, i, &v);
        }
    free(h);
    return GECM_OK;
}

int gecm_download_s(gecm_ctx *c, void *s)
{
    if (c && c->wide) return wide_refuse("gecm_download_s");
    if (c && c->multi) return multi_refuse("gecm_download_s");
    if (method_refuse(c, "gecm_download_s", 0)) return GECM_ERR_STATE;
    if (!c || !s || c->batch == 0) return GECM_ERR_ARG;
    const size_t batch = c->batch;
    uint32_t *h = (uint32_t *)malloc((size_t)c->mod.nl * batch * 4);
    if (!h) return GECM_ERR_NOMEM;
    if (gecm_dev_download_s(c->dev, h)) { free(h); set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    for (size_t i = 0; i < batch; i++) {
        mpl_t v;
        mpl_from_limbs32(&v, h + i, batch, c->mod.nl, LIMB_BITS);
        mpl_mulmod(&v, &v, &c->mod.int_to_ref, &c->mod.N);
        vec_put(&c->mod, s, batch, i, &v);
    }
    free(h);
    return GECM_OK;
}

static int fetch_plain(gecm_ctx *c)
{
    const int settled = ff_settle(c);
    if (settled) return settled;
    if (c->have_plain) return GECM_OK;
    if (c->batch == 0) { set_err("no batch"); return GECM_ERR_STATE; }
    if (c->wide) {
        /* the kernel's lazy limbs, and on the worker threads: canonical modulo N, then out of Montgomery form */
        const size_t words = (size_t)c->mod.nl * c->batch;
        uint32_t *raw = (uint32_t *)malloc(words * 2 * sizeof(uint32_t));
        if (!raw) return GECM_ERR_NOMEM;
        if (gecm_dev_download_raw(c->dev, raw, raw + words)) { free(raw); set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
        gecm_mod_wide_job j = {.m = &c->mod, .batch = c->batch, .rawX = raw, .rawZ = raw + words, .hx = c->hx, .hz = c->hz};
        mpl_invmod(&j.rinv, &c->mod.rint_mod_n, &c->mod.N);         /* N is odd: a power of two has an inverse */
        run_slices(c->batch, gecm_mod_raw_slice, &j);
        free(raw);
        c->have_plain = 1;
        return GECM_OK;
    }
    if (gecm_dev_download_plain(c->dev, c->hx, c->hz)) { set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    c->have_plain = 1;
    return GECM_OK;
}

int gecm_download_points_plain(gecm_ctx *c, void *x, void *z)
{
    if (!c || !x || !z) return GECM_ERR_ARG;
    if (c && c->multi) return multi_refuse("gecm_download_points_plain");
    int rc = fetch_plain(c);
    if (rc) return rc;
    for (size_t i = 0; i < c->batch; i++) {
        mpl_t v;
        mpl_from_limbs32(&v, c->hx + i, c->batch, c->mod.nl, LIMB_BITS);
        vec_put(&c->mod, x, c->batch, i, &v);
        mpl_from_limbs32(&v, c->hz + i, c->batch, c->mod.nl, LIMB_BITS);
        vec_put(&c->mod, z, c->batch, i, &v);
    }
    return GECM_OK;
}

/* The modulus of the caller's curve k and its position in the batch arrays (stride c->batch); NULL if there is no
 * such curve.  Reads the context only: the per-curve calls may run on several threads at once. */
static const gecm_mod *curve_at(const gecm_ctx *c, size_t k, size_t *pos)
{
    if (!c->multi) { *pos = k; return k < c->batch ? &c->mod : NULL; }
    if (c->batch == 0 || k >= c->lay.nuser) { set_err("curve %zu: no such curve in the batch", k); return NULL; }
    *pos = c->lay.slot[k];
    return &c->grp[c->lay.pos_grp[*pos]];
}

int gecm_curve_param(const gecm_ctx *c, size_t k)
{
    size_t pos;
    if (!c || !curve_at(c, k, &pos)) {
        if (!c || !c->multi) set_err("gecm_curve_param: curve %zu: no such curve in the batch", k);
        return GECM_ERR_ARG;
    }
    return c->param ? c->param[pos] : GECM_PARAM_SUYAMA;
}

int gecm_format_save_line(gecm_ctx *c, size_t k, char *buf, size_t buflen)
{
    return gecm_format_resume_line(c, k, c ? c->B1 : 0, buf, buflen);
}

int gecm_format_resume_line(gecm_ctx *c, size_t k, uint64_t b1_label, char *buf, size_t buflen)
{
    size_t pos;
    const gecm_mod *m = c && buf ? curve_at(c, k, &pos) : NULL;
    if (!m) return GECM_ERR_ARG;
    if (method_refuse(c, "gecm_format_save_line", 0)) return GECM_ERR_STATE;
    int rc = fetch_plain(c);
    if (rc) return rc;
    static __thread char hn[MPL_MAXL * 10 + 2], hxs[MPL_MAXL * 10 + 2], hzs[MPL_MAXL * 10 + 2];
    mpl_t v;
    mpl_get_hex(hn, report_n(m));
    mpl_from_limbs32(&v, c->hx + pos, c->batch, m->nl, LIMB_BITS);
    mpl_get_hex(hxs, &v);
    mpl_from_limbs32(&v, c->hz + pos, c->batch, m->nl, LIMB_BITS);
    mpl_get_hex(hzs, &v);
    /* ecm.c:1372-1380; a curve of another parametrisation says so, or a reader would take its sigma for Suyama's */
    char prm[16] = "";
    if (c->param && c->param[pos]) snprintf(prm, sizeof prm, "PARAM=%d; ", c->param[pos]);
    int n = snprintf(buf, buflen, "METHOD=ECM; %sSIGMA=%llu; B1=%llu; N=0x%s; X=0x%s; Z=0x%s; PROGRAM=AVX-ECM;\n", prm,
                     (unsigned long long)c->sigma[pos], (unsigned long long)b1_label, hn, hxs, hzs);
    if (n < 0 || (size_t)n >= buflen) { set_err("gecm_format_save_line: buffer too small"); return GECM_ERR_ARG; }
    return n;
}

int gecm_stage1_factor(gecm_ctx *c, size_t k, char *dec, size_t declen, int *is_prp)
{
    size_t pos;
    const gecm_mod *m = c ? curve_at(c, k, &pos) : NULL;
    if (!m) return GECM_ERR_ARG;
    int rc = fetch_plain(c);
    if (rc) return rc;
    mpl_t z, g;
    /* check_factor, ecm.c:2542-2557: gcd(Z, N); the reference passes Z in Montgomery form, and
     * gcd(z R mod N, N) = gcd(z, N) because R is a power of two and N is odd.  If the device scan
     * of this batch has run, its gcd is used; otherwise it is computed here. */
    if (c->scan_valid[0] && c->hg[0]) {
        mpl_from_limbs32(&g, c->hg[0] + pos, c->batch, m->nl, LIMB_BITS);
    } else if (c->method) {                          /* gcd(x - 1, N) or gcd(x - 2, N); x - c = 0 gives g = N: no factor */
        mpl_t off;
        mpl_set_u64(&off, c->method == GECM_METHOD_PP1 ? 2 : 1);
        mpl_mod(&off, &off, &m->N);
        mpl_from_limbs32(&z, c->hx + pos, c->batch, m->nl, LIMB_BITS);
        mpl_submod(&z, &z, &off, &m->N);
        mpl_gcd(&g, &z, &m->N);
    } else {
        mpl_from_limbs32(&z, c->hz + pos, c->batch, m->nl, LIMB_BITS);
        mpl_gcd(&g, &z, &m->N);
    }
    return gecm_mod_factor(m, &g, "gecm_stage1_factor", dec, declen, is_prp);
}

/* ---- normalisation and standard lines ---------------------------------------- */
int gecm_normalize_points(gecm_ctx *c)
{
    if (c && c->wide) return wide_refuse("gecm_normalize_points");
    const int settled = ff_settle(c);
    if (settled) return settled;
    if (!c || c->batch == 0) { set_err("gecm_normalize_points: no curves uploaded"); return GECM_ERR_STATE; }
    if (method_refuse(c, "gecm_normalize_points", 0)) return GECM_ERR_STATE;
    if (!c->multi && c->mod.have_report) {
        set_err("gecm_normalize_points: not with a report modulus (gecm_set_report_modulus): x modulo the context's "
                "modulus is not x modulo the number the lines name");
        return GECM_ERR_STATE;
    }
    const size_t batch = c->batch;
    uint32_t *flags = (uint32_t *)malloc(batch * sizeof(uint32_t));
    uint8_t *left = (uint8_t *)calloc(batch, 1);
    if (!flags || !left) { free(flags); free(left); return GECM_ERR_NOMEM; }
    if (gecm_dev_normalize(c->dev, flags)) { free(flags); free(left); set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    int any = 0;
    for (size_t p = 0; p < batch; p++)
        if (flags[p] && !(c->multi && c->lay.pos_user[p] == GECM_PAD)) left[p] = (uint8_t)(any = 1);
    free(flags);
    free(c->norm_left);
    c->norm_left = left;
    c->normalized = 1;
    c->last_ms = gecm_dev_last_build_ms(c->dev);
    c->have_plain = 0;
    c->s2_ready = 0;
    c->scan_valid[0] = 0;
    c->twin.loaded = 0;            /* the twin's copy of the points no longer matches: the next launch runs modulo N */
    return any;
}

int gecm_points_normalized(const gecm_ctx *c) { return c && c->batch && c->normalized; }

/* the standard line of a P-1 / P+1 residue (include/gecm.h): no SIGMA, no Z, X0 when the seed is known */
static int format_method_line(gecm_ctx *c, const gecm_mod *m, size_t pos, char *buf, size_t buflen)
{
    int rc = fetch_plain(c);
    if (rc) return rc;
    static __thread char hn[MPL_MAXL * 10 + 2], hxs[MPL_MAXL * 10 + 2], h0[MPL_MAXL * 10 + 16];
    mpl_t v;
    mpl_get_hex(hn, &m->N);
    mpl_from_limbs32(&v, c->hx + pos, c->batch, m->nl, LIMB_BITS);
    mpl_get_hex(hxs, &v);
    h0[0] = 0;
    if (c->seed) {
        mpl_from_limbs32(&v, c->seed + pos, c->batch, m->nl, LIMB_BITS);
        memcpy(h0, "X0=0x", 5);
        int n0 = mpl_get_hex(h0 + 5, &v);
        memcpy(h0 + 5 + n0, "; ", 3);
    }
    int n = snprintf(buf, buflen, "METHOD=%s; B1=%llu; N=0x%s; X=0x%s; %sPROGRAM=AVX-ECM-STD;\n", method_name(c->method),
                     (unsigned long long)c->B1, hn, hxs, h0);
    if (n < 0 || (size_t)n >= buflen) { set_err("gecm_format_save_line_std: buffer too small"); return GECM_ERR_ARG; }
    return n;
}

int gecm_format_save_line_std(gecm_ctx *c, size_t k, char *buf, size_t buflen)
{
    if (c && c->wide) return wide_refuse("gecm_format_save_line_std");
    size_t pos;
    const gecm_mod *m = c && buf ? curve_at(c, k, &pos) : NULL;
    if (!m) return GECM_ERR_ARG;
    if (c->method) return format_method_line(c, m, pos, buf, buflen);
    if (!c->normalized) { set_err("gecm_format_save_line_std: the batch is not normalised (gecm_normalize_points)"); return GECM_ERR_STATE; }
    int rc = fetch_plain(c);
    if (rc) return rc;
    static __thread char hn[MPL_MAXL * 10 + 2], hxs[MPL_MAXL * 10 + 2], hzs[MPL_MAXL * 10 + 2];
    mpl_t v;
    mpl_get_hex(hn, report_n(m));
    mpl_from_limbs32(&v, c->hx + pos, c->batch, m->nl, LIMB_BITS);
    mpl_get_hex(hxs, &v);
    const int prm = c->param ? c->param[pos] : GECM_PARAM_SUYAMA;
    int n;
    if (c->norm_left[pos]) {
        mpl_from_limbs32(&v, c->hz + pos, c->batch, m->nl, LIMB_BITS);
        mpl_get_hex(hzs, &v);
        n = snprintf(buf, buflen, "METHOD=ECM; PARAM=%d; SIGMA=%llu; B1=%llu; N=0x%s; X=0x%s; Z=0x%s; PROGRAM=AVX-ECM-STD;\n", prm,
                     (unsigned long long)c->sigma[pos], (unsigned long long)c->B1, hn, hxs, hzs);
    } else
        n = snprintf(buf, buflen, "METHOD=ECM; PARAM=%d; SIGMA=%llu; B1=%llu; N=0x%s; X=0x%s; PROGRAM=AVX-ECM-STD;\n", prm,
                     (unsigned long long)c->sigma[pos], (unsigned long long)c->B1, hn, hxs);
    if (n < 0 || (size_t)n >= buflen) { set_err("gecm_format_save_line_std: buffer too small"); return GECM_ERR_ARG; }
    return n;
}

/* ---- stage 2 -------------------------------------------------------------------------------- */
/* point additions next_pt_vec performs for multiplier c (one per bit below the top one, ecm.c:939-966) */
static uint64_t ladder_adds(uint64_t c)
{
    uint64_t n = 0;
    if (c <= 2) return 0;
    while (c > 1) { n++; c >>= 1; }
    return n;
}

int gecm_stage2_init(gecm_ctx *c, uint32_t D, uint32_t U)
{
    if (c && c->wide) return wide_refuse("gecm_stage2_init");
    const int settled = ff_settle(c);
    if (settled) return settled;
    if (method_refuse(c, "gecm_stage2_init", 1)) return GECM_ERR_STATE;
    if (!c || c->batch == 0 || c->B1 == 0) { set_err("gecm_stage2_init: run stage 1 first"); return GECM_ERR_STATE; }
    if (!D) D = gecm_s2_default_D(c->B1);
    if (!U) U = GECM_S2_DEFAULT_U;
    /* the ring holds the 2L = 4U steps of the window plus one chunk being generated */
    if (U > (S2_RING - S2_GIANT_CHUNK) / 4) {
        set_err("gecm_stage2_init: U = %u is more than this build's giant-step ring takes (U <= %u)", U,
                (S2_RING - S2_GIANT_CHUNK) / 4);
        return GECM_ERR_ARG;
    }
    if (c->s2.D != D || c->s2.U != U) {
        gecm_s2_plan_free(&c->s2);
        if (gecm_s2_plan_init(&c->s2, D, U)) { set_err("gecm_stage2_init: bad D/U"); return GECM_ERR_ARG; }
    }
    c->have_acc = 0;
    c->s2_ptadds = (uint64_t)c->s2.umax - 2 + ladder_adds(D);   /* ecm.c:2263: j = 3..U*w; Pd ladder :2334 */
    c->s2_numinv = 1;                                        /* ecm.c:2322 */
    /* a method batch normalises nothing: its only inversion is the seed's x^-1 of P-1 */
    c->s2_devinv = c->method ? (c->method == GECM_METHOD_PM1) : (c->s2.npb - 1 + GECM_S2_BLK - 1) / GECM_S2_BLK;
    c->s2_paired = 0;
    /* small batches: K interleaved sub-sequences per curve (csrc/gecm_stage2.hpp, s2_init_k): the table indices of
     * the kept members of sub-sequence r, j = r, r+K, ... (r = 0: K, 2K, ...), in order */
    const uint32_t K = gecm_dev_s2_subseq(c->dev);
    uint32_t *tgt = NULL, toff[33];
    memset(toff, 0, sizeof toff);
    if (K > 1) {
        tgt = (uint32_t *)malloc(((size_t)c->s2.npb + 1) * sizeof(uint32_t));
        if (!tgt) return GECM_ERR_NOMEM;
        uint32_t n = 0;
        for (uint32_t r = 0; r < K; r++) {
            toff[r] = n;
            for (uint32_t j = r ? r : K; j <= c->s2.umax; j += K)
                if (c->s2.map[j]) tgt[n++] = c->s2.map[j];
        }
        toff[K] = n;
    }
    /* the host copy of the failure planes is sized before the device is touched: after an allocation failure the
     * context still has its old stage-2 state, untouched */
    const uint32_t planes = K > 1 ? K + 1 : 1;
    if (planes != c->fail_planes || !c->hfail) {
        uint32_t *nf = (uint32_t *)calloc(c->batch * (size_t)c->mod.nl * planes, 4);
        if (!nf) { free(tgt); return GECM_ERR_NOMEM; }
        free(c->hfail);
        c->hfail = nf;
        c->fail_planes = planes;
        c->have_acc = 0;
    }
    c->s2_ready = 0;
    int drc = c->method ? gecm_dev_s2_init_unit(c->dev, unit_method(c), c->s2.keep, c->s2.keep_words, c->s2.umax, D, c->s2.npb,
                                                S2_GIANT_CHUNK, S2_RING, tgt, toff, K)
                        : gecm_dev_s2_init(c->dev, c->s2.keep, c->s2.keep_words, c->s2.umax, D, c->s2.npb, S2_GIANT_CHUNK,
                                           S2_RING, tgt, toff, K);
    free(tgt);
    if (drc) {
        set_err("gecm_stage2_init: %s", gecm_dev_error());
        return GECM_ERR_DEVICE;
    }
    if (gecm_dev_s2_fail_planes(c->dev) != planes) { set_err("gecm_stage2_init: failure planes out of step"); return GECM_ERR_STATE; }
    c->s2_ready = 1;
    c->s2_K = K;
    return GECM_OK;
}

/* Sub-sequences per curve in stage 2 (include/gecm.h): the device layer keeps the setting and applies it where it
 * chooses K for a batch (gecm_dev_s2_subseq, gecm_dev_batch_bytes), so memory accounting and init agree. */
int gecm_set_stage2_subseq(gecm_ctx *c, int k)
{
    if (!c) { set_err("gecm_set_stage2_subseq: no context"); return GECM_ERR_ARG; }
    if (gecm_dev_set_s2_subseq(c->dev, k)) {
        set_err("gecm_set_stage2_subseq: %d is not GECM_S2_SUBSEQ_DEFAULT, GECM_S2_SUBSEQ_AUTO or 1, 2, 4, 8, 16, 32", k);
        return GECM_ERR_ARG;
    }
    return GECM_OK;
}

int gecm_get_stage2_subseq(const gecm_ctx *c, uint32_t *k_chunks)
{
    if (!c) { set_err("gecm_get_stage2_subseq: no context"); return GECM_ERR_ARG; }
    if (k_chunks) *k_chunks = c->s2_K ? gecm_dev_s2_k_chunks(c->dev) : 0;
    return (int)c->s2_K;
}

int gecm_pair_primes(gecm_pairs *out, uint64_t B1, uint64_t B2, uint32_t D, uint32_t U)
{
    gecm_pairmap pm;
    if (!out || B2 <= B1 || !D || !U) { set_err("gecm_pair_primes: bad argument"); return GECM_ERR_ARG; }
    if (gecm_pair(&pm, B1, B2, D, U)) { set_err("gecm_pair_primes: out of memory"); return GECM_ERR_NOMEM; }
    out->pairmap_v = pm.v; out->pairmap_u = pm.u; out->steps = pm.steps; out->amin = pm.amin;
    out->pairs = pm.pairs; out->primes = pm.nump;
    return GECM_OK;
}

void gecm_pairmap_release(gecm_pairs *p)
{
    if (!p) return;
    free(p->pairmap_v);
    free(p->pairmap_u);
    memset(p, 0, sizeof *p);
}

/* launch the giant steps and the pair walk of one range from a built tape; tape_id != 0: the device keeps its copy */
static int s2_run_tape(gecm_ctx *c, const gecm_s2_tape *t, uint32_t amin, uint64_t tape_id)
{
    const gecm_s2_plan *p = &c->s2;
    const uint64_t A0 = (uint64_t)amin * p->D * 2;                       /* ecm.c:2378 */
    int rc = c->method ? gecm_dev_s2_pair_unit(c->dev, unit_method(c), t->words, (uint32_t)(t->nwords / 2), p->D, S2_GIANT_CHUNK,
                                               S2_RING, A0, tape_id)
                       : gecm_dev_s2_pair(c->dev, t->words, (uint32_t)(t->nwords / 2), p->D, S2_GIANT_CHUNK, S2_RING, A0, tape_id);
    if (rc) { set_err("gecm_stage2_pair: %s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    c->s2_ptadds += t->adds + ladder_adds(A0) + ladder_adds(A0 - p->D);  /* ecm.c:2383, 2390 */
    c->s2_numinv += t->inv; c->s2_paired += t->paired;
    if (!c->method) c->s2_devinv += t->devinv;                           /* the giant steps of a method batch invert nothing */
    c->s2_amin_last = t->amin_last;
    c->have_acc = 0;
    c->scan_valid[1] = 0;
    return GECM_OK;
}

static int s2_build_tape(gecm_ctx *c, gecm_s2_tape *t, uint32_t steps, const uint32_t *pm_v, const uint32_t *pm_u, uint32_t amin)
{
    uint32_t bad = 0;
    int trc = gecm_s2_tape_build(t, &c->s2, steps, pm_v, pm_u, amin, S2_GIANT_CHUNK, S2_RING, &bad);
    if (trc == -1) return GECM_ERR_NOMEM;
    if (trc) {                                                           /* ecm.c:2508-2517 */
        set_err("gecm_stage2_pair: invalid pair map entry %u: (%u,%u)", bad, pm_v[bad], pm_u[bad]);
        return GECM_ERR_ARG;
    }
    return GECM_OK;
}

/* Two independent 64-bit hashes of the pair map (FNV-1a over the words; a multiply-rotate mix over the 64-bit
 * pairs (v, u) with their position), 8 ms for the 3.0 M entries of a 1e8 range */
static void pairmap_fingerprint(uint32_t steps, const uint32_t *pm_v, const uint32_t *pm_u, uint64_t *h1, uint64_t *h2)
{
    uint64_t a = 1469598103934665603ull, b = 0x9E3779B97F4A7C15ull;
    for (uint32_t i = 0; i < steps; i++) {
        a = (a ^ pm_v[i]) * 1099511628211ull;
        a = (a ^ pm_u[i]) * 1099511628211ull;
        uint64_t w = (((uint64_t)pm_v[i] << 32) | pm_u[i]) + (uint64_t)i * 0xD6E8FEB86659FD93ull;
        w *= 0xBF58476D1CE4E5B9ull;
        b = ((b << 27) | (b >> 37)) ^ w;
        b *= 0x94D049BB133111EBull;
    }
    *h1 = a;
    *h2 = b;
}

/* The tape of a pair map is the same for every batch and costs more host time than reading the map once (130 ms
 * against 8 ms): the last one is kept and recognised by (steps, amin, D, U) and both hashes of the map. */
static int s2_tape_for(gecm_ctx *c, uint32_t steps, const uint32_t *pm_v, const uint32_t *pm_u, uint32_t amin)
{
    uint64_t fp, fp2;
    pairmap_fingerprint(steps, pm_v, pm_u, &fp, &fp2);
    if (c->ptp_valid && c->ptp_steps == steps && c->ptp_amin == amin && c->ptp_D == c->s2.D && c->ptp_U == c->s2.U &&
        c->ptp_fp == fp && c->ptp_fp2 == fp2)
        return GECM_OK;
    if (c->ptp_valid) free(c->ptp.words);
    c->ptp_valid = 0;
    int rc = s2_build_tape(c, &c->ptp, steps, pm_v, pm_u, amin);
    if (rc) return rc;
    c->ptp_valid = 1;
    c->ptp_fp = fp; c->ptp_fp2 = fp2;
    c->ptp_steps = steps; c->ptp_amin = amin; c->ptp_D = c->s2.D; c->ptp_U = c->s2.U;
    c->ptp_id = next_tape_id();
    return GECM_OK;
}

int gecm_stage2_pair(gecm_ctx *c, uint32_t steps, const uint32_t *pm_v, const uint32_t *pm_u, uint32_t amin)
{
    if (c && c->wide) return wide_refuse("gecm_stage2_pair");
    if (method_refuse(c, "gecm_stage2_pair", 1)) return GECM_ERR_STATE;
    if (!c || !c->s2_ready) { set_err("gecm_stage2_pair: gecm_stage2_init has not run"); return GECM_ERR_STATE; }
    if (steps && (!pm_v || !pm_u)) return GECM_ERR_ARG;
    int rc = s2_tape_for(c, steps, pm_v, pm_u, amin);
    if (rc) return rc;
    return s2_run_tape(c, &c->ptp, amin, c->ptp_id);
}

/* Optional, for callers of the phase functions: make (and keep) the tape gecm_stage2_pair will need for this pair map
 * and (D, U) ahead of time — e.g. while the device runs stage 1.  Touches nothing on the device. */
int gecm_stage2_pair_prepare(gecm_ctx *c, uint32_t D, uint32_t U, uint32_t steps, const uint32_t *pm_v, const uint32_t *pm_u,
                             uint32_t amin)
{
    if (c && c->wide) return wide_refuse("gecm_stage2_pair_prepare");
    if (method_refuse(c, "gecm_stage2_pair_prepare", 1)) return GECM_ERR_STATE;
    if (!c || (steps && (!pm_v || !pm_u))) return GECM_ERR_ARG;
    if (!D || !U || U > (S2_RING - S2_GIANT_CHUNK) / 4) { set_err("gecm_stage2_pair_prepare: bad D/U"); return GECM_ERR_ARG; }
    if (c->s2.D != D || c->s2.U != U) {                                  /* the plan gecm_stage2_init(D, U) would make */
        gecm_s2_plan_free(&c->s2);
        c->s2_ready = 0;
        if (gecm_s2_plan_init(&c->s2, D, U)) { set_err("gecm_stage2_pair_prepare: bad D/U"); return GECM_ERR_ARG; }
    }
    return s2_tape_for(c, steps, pm_v, pm_u, amin);
}

/* keep `pm` (ownership passes to the context) and make the tape that goes with it; the plan of (D, U) must be c->s2 */
static int keep_pairmap(gecm_ctx *c, gecm_pairs *pm, uint64_t lo, uint64_t hi)
{
    drop_kept_pairmap(c);
    c->pm = *pm;
    c->pm_valid = 1; c->pm_lo = lo; c->pm_hi = hi; c->pm_D = c->s2.D; c->pm_U = c->s2.U;
    int rc = s2_build_tape(c, &c->tp, c->pm.steps, c->pm.pairmap_v, c->pm.pairmap_u, c->pm.amin);
    if (rc) return rc;                                                   /* the map stays; the tape is made (and refused) again later */
    c->tp_valid = 1;
    c->tp_id = next_tape_id();
    return GECM_OK;
}

/* The pair map of [B1, B2) and the device tape made from it depend on nothing the device computes: a caller can have
 * them made while stage 1 runs (gecm_stage1 returns after the launch).  Kept in the context; gecm_stage2 with the same
 * (B2, D, U) finds them, and the device keeps its copy of the tape from one batch to the next. */
int gecm_stage2_prepare(gecm_ctx *c, uint64_t B2, uint32_t D, uint32_t U)
{
    if (c && c->wide) return wide_refuse("gecm_stage2_prepare");
    const uint64_t PRIME_RANGE = 100000000ull;
    if (method_refuse(c, "gecm_stage2_prepare", 1)) return GECM_ERR_STATE;
    if (!c || c->B1 == 0 || B2 <= c->B1) { set_err("gecm_stage2_prepare: call gecm_stage1 first; B2 > B1"); return GECM_ERR_ARG; }
    if (!D) D = gecm_s2_default_D(c->B1);
    if (!U) U = GECM_S2_DEFAULT_U;
    if (B2 - c->B1 > PRIME_RANGE) return GECM_OK;                        /* several ranges: made range by range later */
    if (U > (S2_RING - S2_GIANT_CHUNK) / 4) return GECM_OK;              /* gecm_stage2_init will refuse it */
    if (c->pm_valid && c->pm_lo == c->B1 && c->pm_hi == B2 && c->pm_D == D && c->pm_U == U) return GECM_OK;
    if (c->s2.D != D || c->s2.U != U) {                                  /* the plan gecm_stage2_init(D, U) would make */
        gecm_s2_plan_free(&c->s2);
        c->s2_ready = 0;
        if (gecm_s2_plan_init(&c->s2, D, U)) { set_err("gecm_stage2_prepare: bad D/U"); return GECM_ERR_ARG; }
    }
    gecm_pairs pm;
    int rc = gecm_pair_primes(&pm, c->B1, B2, D, U);
    if (rc) return rc;
    return keep_pairmap(c, &pm, c->B1, B2);
}

int gecm_stage2(gecm_ctx *c, uint64_t B2, uint32_t D, uint32_t U)
{
    if (c && c->wide) return wide_refuse("gecm_stage2");
    const uint64_t PRIME_RANGE = 100000000ull;                           /* main.c:581 */
    if (method_refuse(c, "gecm_stage2", 1)) return GECM_ERR_STATE;
    if (!c || c->B1 == 0 || B2 <= c->B1) { set_err("gecm_stage2: need B2 > B1 and a finished stage 1"); return GECM_ERR_ARG; }
    int rc = gecm_stage2_init(c, D, U);
    if (rc) return rc;
    for (uint64_t p = c->B1; p < B2; p += PRIME_RANGE) {                 /* ecm.c:1424-1476 */
        uint64_t hi = p + PRIME_RANGE < B2 ? p + PRIME_RANGE : B2;
        /* the pair map depends on (range, D, U) only: a run of many batches (the reference: one per 8 curves and
         * thread) computes it once; the last single-range map is kept in the context, with its tape */
        const int cacheable = (p == c->B1 && hi == B2);
        const int kept = c->pm_valid && c->pm_lo == p && c->pm_hi == hi && c->pm_D == c->s2.D && c->pm_U == c->s2.U;
        if (cacheable && !kept) {
            gecm_pairs pm;
            rc = gecm_pair_primes(&pm, p, hi, c->s2.D, c->s2.U);
            if (rc) return rc;
            rc = keep_pairmap(c, &pm, p, hi);
            if (rc) return rc;
        }
        if (cacheable) {
            if (!c->tp_valid) {                                          /* a map kept without its tape: make it now */
                gecm_pairs pm = c->pm;
                c->pm_valid = 0;
                rc = keep_pairmap(c, &pm, p, hi);
                if (rc) return rc;
            }
            rc = s2_run_tape(c, &c->tp, c->pm.amin, c->tp_id);
            if (rc) return rc;
            continue;
        }
        gecm_pairs pm;
        rc = gecm_pair_primes(&pm, p, hi, c->s2.D, c->s2.U);
        if (rc) return rc;
        rc = gecm_stage2_pair(c, pm.steps, pm.pairmap_v, pm.pairmap_u, pm.amin);
        gecm_pairmap_release(&pm);
        if (rc) return rc;
    }
    return gecm_sync(c);
}

int gecm_get_stage2_stats(const gecm_ctx *c, gecm_stage2_stats *st)
{
    if (!c || !st || !c->s2.D) return GECM_ERR_STATE;
    st->ptadds = c->s2_ptadds; st->numinv = c->s2_numinv; st->paired = c->s2_paired;
    st->device_inversions = c->s2_devinv;
    st->D = c->s2.D; st->U = c->s2.U; st->L = c->s2.L; st->amin_last = c->s2_amin_last;
    return GECM_OK;
}

static int fetch_acc(gecm_ctx *c)
{
    if (c->have_acc) return GECM_OK;
    if (!c->s2_ready) { set_err("no stage-2 state"); return GECM_ERR_STATE; }
    if (gecm_dev_s2_download(c->dev, c->hacc, c->hfail)) { set_err("%s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    c->have_acc = 1;
    return GECM_OK;
}

int gecm_download_acc(gecm_ctx *c, void *acc)
{
    if (c && c->wide) return wide_refuse("gecm_download_acc");
    if (!c || !acc) return GECM_ERR_ARG;
    if (c && c->multi) return multi_refuse("gecm_download_acc");
    int rc = fetch_acc(c);
    if (rc) return rc;
    for (size_t i = 0; i < c->batch; i++) {
        mpl_t v;
        mpl_from_limbs32(&v, c->hacc + i, c->batch, c->mod.nl, LIMB_BITS);
        mpl_mulmod(&v, &v, &c->mod.int_to_ref, &c->mod.N);
        vec_put(&c->mod, acc, c->batch, i, &v);
    }
    return GECM_OK;
}

int gecm_stage2_factor(gecm_ctx *c, size_t k, char *dec, size_t declen, int *is_prp)
{
    if (c && c->wide) return wide_refuse("gecm_stage2_factor");
    size_t pos;
    const gecm_mod *m = c ? curve_at(c, k, &pos) : NULL;
    if (!m) return GECM_ERR_ARG;
    if (method_refuse(c, "gecm_stage2_factor", 1)) return GECM_ERR_STATE;
    int rc = fetch_acc(c);
    if (rc) return rc;
    mpl_t a, g;
    gecm_mod_fail_record(m, c->hfail, c->fail_planes, c->batch, pos, &g);
    if (mpl_is_zero(&g)) {
        if (c->scan_valid[1] && c->hg[1]) {
            mpl_from_limbs32(&g, c->hg[1] + pos, c->batch, m->nl, LIMB_BITS);
        } else {
            mpl_from_limbs32(&a, c->hacc + pos, c->batch, m->nl, LIMB_BITS);
            mpl_gcd(&g, &a, &m->N);                  /* check_factor, ecm.c:2542-2557 */
        }
    }
    return gecm_mod_factor(m, &g, "gecm_stage2_factor", dec, declen, is_prp);
}

/* ---- device factor scan -------------------------------------------------------------------
 * The device compares every curve with its own N.  Of a multi-modulus batch the padding is never flagged, and `first`
 * is in the caller's numbering. */
int gecm_scan_factors(gecm_ctx *c, int stage, size_t *first)
{
    const int settled = ff_settle(c);
    if (settled) return settled;
    if (!c || c->batch == 0 || (stage != 1 && stage != 2)) { set_err("gecm_scan_factors: bad argument"); return GECM_ERR_ARG; }
    if (stage == 2 && c->wide) return wide_refuse("gecm_scan_factors(stage 2)");
    if (stage == 2 && method_refuse(c, "gecm_scan_factors(stage 2)", 1)) return GECM_ERR_STATE;
    if (stage == 2 && !c->s2_ready) { set_err("gecm_scan_factors: no stage-2 state"); return GECM_ERR_STATE; }
    uint32_t **f = &c->flags[stage - 1], **hg = &c->hg[stage - 1];
    if (!*f) *f = (uint32_t *)calloc(c->batch, sizeof(uint32_t));
    if (!*hg) *hg = (uint32_t *)calloc(c->batch * (size_t)c->mod.nl, sizeof(uint32_t));
    if (!*f || !*hg) return GECM_ERR_NOMEM;
    if (c->wide) {                                     /* gcd(z, N) per curve on the worker threads, from the plain z */
        const int rc = fetch_plain(c);
        if (rc) return rc;
        gecm_mod_wide_job j = {.m = &c->mod, .batch = c->batch, .hz = c->hz, .hg = *hg, .flags = *f};
        run_slices(c->batch, gecm_mod_gcd_slice, &j);
    } else
    /* stage 1 of a method batch tests x - 1 or x - 2; its stage-2 accumulator is scanned as any other */
    if (c->method && stage == 1 ? gecm_dev_gcd_scan_off(c->dev, c->method == GECM_METHOD_PP1 ? 2 : 1, *f, *hg)
                                : gecm_dev_gcd_scan(c->dev, stage - 1, *f, *hg)) { set_err("gecm_scan_factors: %s", gecm_dev_error()); return GECM_ERR_DEVICE; }
    /* stage 1: x, z come to the host with the scan: everything a caller does next (save lines, factors of the flagged
     * curves) is then host work, off the device's queue */
    int rc = stage == 1 ? fetch_plain(c) : fetch_acc(c);
    if (rc) return rc;
    size_t n = 0, lo = c->multi ? c->lay.nuser : c->batch;
    for (size_t p = 0; p < c->batch; p++) {
        const gecm_mod *m = &c->mod;
        size_t user = p;
        if (c->multi) {
            if (c->lay.pos_user[p] == GECM_PAD) { (*f)[p] = 0; continue; }
            m = &c->grp[c->lay.pos_grp[p]];
            user = c->lay.pos_user[p];
        }
        mpl_t fr, g;
        mpl_set_u64(&fr, 0);
        if (stage == 2) {                              /* a failed batch inversion also marks its curve (ecm.c:1927-1939) */
            gecm_mod_fail_record(m, c->hfail, c->fail_planes, c->batch, p, &fr);
            if (!mpl_is_zero(&fr)) (*f)[p] = to_report(m, &fr);
        }
        if (m->have_report && (*f)[p] && mpl_is_zero(&fr)) {
            /* the device looked for factors of the context's modulus: keep the curves whose gcd shares one with the
             * report modulus (gcd(gcd(v, Mw), N) = gcd(v, N) for N | Mw); a failure record decides if there is one */
            mpl_from_limbs32(&g, *hg + p, c->batch, m->nl, LIMB_BITS);
            if (!mpl_is_zero(&g) && !to_report(m, &g)) (*f)[p] = 0;
        }
        if ((*f)[p]) { n++; if (user < lo) lo = user; }
    }
    c->scan_valid[stage - 1] = 1;
    if (first) *first = lo;
    return (int)(n > 0x7fffffff ? 0x7fffffff : n);
}

int gecm_curve_flag(const gecm_ctx *c, int stage, size_t k)
{
    size_t pos;
    if (!c || (stage != 1 && stage != 2) || !c->flags[stage - 1] || !curve_at(c, k, &pos)) return 0;
    return (int)c->flags[stage - 1][pos];
}

/* ---- multi-modulus contexts ------------------------------------------------ */
int gecm_create_multi(gecm_ctx **out, int device, const char *const *n_strs, size_t count, int digitbits)
{
    if (!out || !n_strs || (digitbits != 52 && digitbits != 32)) {
        set_err("gecm_create_multi: bad argument (digitbits must be 52 or 32)");
        return GECM_ERR_ARG;
    }
    if (count == 0) { set_err("gecm_create_multi: the list of moduli is empty"); return GECM_ERR_ARG; }
    if (count > 0xfffffffe) { set_err("gecm_create_multi: %zu moduli, more than a 32-bit modulus index holds", count); return GECM_ERR_ARG; }
    gecm_ctx *c = (gecm_ctx *)calloc(1, sizeof *c);
    gecm_mod *grp = (gecm_mod *)calloc(count, sizeof *grp);
    if (!c || !grp) { free(c); free(grp); return GECM_ERR_NOMEM; }
    c->grp = grp;
    c->ngroups = count;
    c->multi = 1;
    c->device = device;
    /* every N on its own first: the largest decides the limb count; then every N again at that count */
    int maxbits = 0, rc = GECM_OK;
    size_t largest = 0;
    char who[64];
    for (size_t g = 0; g < count && !rc; g++) {
        snprintf(who, sizeof who, "gecm_create_multi: N[%zu]", g);
        mpl_t n;
        if (!n_strs[g] || mpl_set_str(&n, n_strs[g]) || !mpl_is_odd(&n) || mpl_cmp_u64(&n, 3) < 0) {
            set_err("%s must be an odd integer >= 3 (decimal or 0x-hex)", who);
            rc = GECM_ERR_ARG;
        } else if (!pick_nl(mpl_bits(&n))) {
            set_err("%s of %d bits is larger than this build supports", who, mpl_bits(&n));
            rc = GECM_ERR_ARG;
        } else if (mpl_bits(&n) > maxbits) {
            maxbits = mpl_bits(&n);
            largest = g;
        }
    }
    const int nl = rc ? 0 : pick_nl(maxbits);
    for (size_t g = 0; g < count && !rc; g++) {
        snprintf(who, sizeof who, "gecm_create_multi: N[%zu]", g);
        rc = gecm_mod_setup(&grp[g], who, n_strs[g], digitbits, nl, pick_nl);
    }
    /* the context itself: the largest N (what gecm_get_config reports) and the device */
    if (!rc) rc = gecm_mod_setup(&c->mod, "gecm_create_multi", n_strs[largest], digitbits, nl, pick_nl);
    if (!rc) {
        c->grp_dev = (gecm_devmod *)calloc(count, sizeof *c->grp_dev);
        if (!c->grp_dev) rc = GECM_ERR_NOMEM;
    }
    if (!rc) {
        for (size_t g = 0; g < count; g++) c->grp_dev[g] = gecm_mod_devmod(&grp[g]);
        const gecm_devmod dm = gecm_mod_devmod(&c->mod);
        if (gecm_dev_open(&c->dev, device, nl, &dm, 1)) {
            set_err("gecm_create_multi: %s", gecm_dev_error());
            rc = GECM_ERR_DEVICE;
        }
    }
    if (rc) { gecm_destroy(c); return rc; }
    *out = c;
    return GECM_OK;
}

size_t gecm_moduli(const gecm_ctx *c) { return c ? (c->multi ? c->ngroups : 1) : 0; }

/* ---- packing of a multi-modulus batch ---- */
int gecm_multi_packing_max_bits(int packing)
{
    if (packing == GECM_PACK_WAVE) return 0;
    if (packing != GECM_PACK_LANE) return GECM_ERR_ARG;
    int nl = 0;                                    /* the largest limb count with per-lane kernels */
    for (const int *p = gecm_dev_supported_nl(); *p; p++)
        if (gecm_dev_lane_packing_built(*p) && *p > nl) nl = *p;
    return nl ? nl * LIMB_BITS - 5 : GECM_ERR_STATE;   /* R = 2^(28 nl) >= 32 N, as pick_nl */
}

int gecm_set_multi_packing(gecm_ctx *c, int packing)
{
    if (!c || (packing != GECM_PACK_WAVE && packing != GECM_PACK_LANE)) {
        set_err("gecm_set_multi_packing: bad argument (GECM_PACK_WAVE or GECM_PACK_LANE)");
        return GECM_ERR_ARG;
    }
    if (!c->multi) { set_err("gecm_set_multi_packing: not a multi-modulus context (gecm_create_multi)"); return GECM_ERR_STATE; }
    if (packing == GECM_PACK_LANE && !gecm_dev_lane_packing_built(c->mod.nl)) {
        set_err("gecm_set_multi_packing: lane packing serves numbers up to %d bits, and this context's largest has %d",
                gecm_multi_packing_max_bits(GECM_PACK_LANE), mpl_bits(&c->mod.N));
        return GECM_ERR_STATE;
    }
    c->packing = packing;
    return GECM_OK;
}

int gecm_get_multi_packing(const gecm_ctx *c) { return c ? c->packing_used : GECM_ERR_ARG; }

/* the checks gecm_build_curves_multi and gecm_resume_points_multi make on their common arguments */
static int multi_args(const gecm_ctx *c, const char *who, const uint64_t *sigma, const uint32_t *modulus_index, size_t batch)
{
    if (!c || !sigma || !modulus_index || batch == 0) { set_err("%s: bad argument", who); return GECM_ERR_ARG; }
    if (!c->multi) { set_err("%s: not a multi-modulus context (gecm_create_multi)", who); return GECM_ERR_STATE; }
    if (batch >= GECM_PAD) { set_err("%s: batch too large", who); return GECM_ERR_ARG; }
    if (params_fit(c, who, batch)) return GECM_ERR_ARG;
    for (size_t i = 0; i < batch; i++) {
        if (sigma_arg(who, sigma, i, c->next_param)) return GECM_ERR_ARG;
        if (modulus_index[i] >= c->ngroups) {
            set_err("%s: modulus_index[%zu] = %u, the context has %zu moduli", who, i, modulus_index[i], c->ngroups);
            return GECM_ERR_ARG;
        }
    }
    return GECM_OK;
}

int gecm_build_curves_multi(gecm_ctx *c, const uint64_t *sigma, const uint32_t *modulus_index, size_t batch)
{
    int rc = multi_args(c, "gecm_build_curves_multi", sigma, modulus_index, batch);
    if (!rc) rc = batch_build(c, &(batch_desc){.who = "gecm_build_curves_multi", .batch = batch, .sigma = sigma,
                                               .modulus_index = modulus_index, .param = c->next_param});
    return build_call_end(c, rc);
}

/* ---- resume ------------------------------------------------------------------- */
/* The caller's plain x, z (vec layout of the context) as 28-bit limb planes [nl][batch] in the caller's order, each
 * checked against its curve's N; worker threads, the first offending curve recorded for the error text. */
typedef struct {
    const gecm_ctx *c;
    const void *src[2];
    const uint32_t *modulus_index;   /* NULL: every curve on c->mod */
    size_t batch;
    uint32_t *planes;                /* x then z */
    size_t first_bad;                /* batch: none */
} plain_job;

static int plain_slice(void *arg, size_t lo, size_t hi)
{
    plain_job *j = (plain_job *)arg;
    const gecm_ctx *c = j->c;
    const size_t words = (size_t)c->mod.nl * j->batch;
    for (size_t i = lo; i < hi; i++) {
        const gecm_mod *m = j->modulus_index ? &c->grp[j->modulus_index[i]] : &c->mod;
        for (int q = 0; q < 2; q++) {
            mpl_t v;
            vec_get(&c->mod, &v, j->src[q], j->batch, i);          /* the context's NWORDS: the largest number's */
            if (mpl_cmp(&v, &m->N) >= 0) {
                size_t seen = __atomic_load_n(&j->first_bad, __ATOMIC_RELAXED);
                while (i < seen && !__atomic_compare_exchange_n(&j->first_bad, &seen, i, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
                return 1;
            }
            mpl_to_limbs32(j->planes + (size_t)q * words + i, j->batch, c->mod.nl, LIMB_BITS, &v);
        }
    }
    return 0;
}

/* a batch that goes on from points given: stage 1 stands at b1_done and the counters start over, they count what runs
 * from here */
static void stage1_restart(gecm_ctx *c, uint64_t b1_done)
{
    c->B1 = b1_done;
    c->s1_ptadds = c->s1_ptdups = c->s1_last_prime = c->s1_tape_len = 0;
}

/* what both resume calls do once their context kind and sigmas are settled; idx NULL on a single-N context */
static int resume_points(gecm_ctx *c, const char *who, const uint64_t *sigma, const uint32_t *idx, const void *x,
                         const void *z, size_t batch, uint64_t b1_done)
{
    if (c && c->wide) return wide_refuse(who);
    if (!x || !z) { set_err("%s: bad argument", who); return GECM_ERR_ARG; }
    if (b1_done == 1 || b1_done > GECM_B1_MAX) { set_err("%s: b1_done must be 0 or a B1 in [2, %llu]", who, (unsigned long long)GECM_B1_MAX); return GECM_ERR_ARG; }
    uint32_t *planes = (uint32_t *)calloc((size_t)c->mod.nl * batch * 2, 4);
    if (!planes) return GECM_ERR_NOMEM;
    plain_job j = {c, {x, z}, idx, batch, planes, batch};
    int rc = run_slices(batch, plain_slice, &j);
    if (rc > 0) {                                 /* the previous batch is untouched */
        set_err("%s: x[%zu] or z[%zu] is not below the curve's N", who, j.first_bad, j.first_bad);
        rc = GECM_ERR_ARG;
    } else if (!rc) {
        /* the curves of the sigmas (S), then X and Z from the planes: mid stage 1 (the caller goes on with
         * gecm_stage1_range), or stage 1 taken as finished at b1_done */
        rc = batch_build(c, &(batch_desc){.who = who, .batch = batch, .sigma = sigma, .modulus_index = idx, .param = c->next_param,
                                          .content = BATCH_PLAIN, .planes = planes});
        if (rc >= 0) stage1_restart(c, b1_done);
    }
    free(planes);
    return rc;
}

int gecm_resume_points(gecm_ctx *c, const uint64_t *sigma, const void *x, const void *z, size_t batch, uint64_t b1_done)
{
    int rc = sigma_args(c, "gecm_resume_points", sigma, batch);
    if (!rc) rc = resume_points(c, "gecm_resume_points", sigma, NULL, x, z, batch, b1_done);
    return build_call_end(c, rc);
}

int gecm_resume_points_multi(gecm_ctx *c, const uint64_t *sigma, const uint32_t *modulus_index, const void *x,
                             const void *z, size_t batch, uint64_t b1_done)
{
    int rc = multi_args(c, "gecm_resume_points_multi", sigma, modulus_index, batch);
    if (!rc) rc = resume_points(c, "gecm_resume_points_multi", sigma, modulus_index, x, z, batch, b1_done);
    return build_call_end(c, rc);
}

/* ---- P-1 and P+1 batches -------------------------------------------------------- */
/* what both seed calls do once their context kind is settled; idx NULL on a single-N context */
static int build_seeds(gecm_ctx *c, const char *who, int method, const uint32_t *idx, const void *x0, const void *x,
                       size_t batch, uint64_t b1_done)
{
    if (c && c->wide) return wide_refuse(who);
    if (method != GECM_METHOD_PM1 && method != GECM_METHOD_PP1) {
        set_err("%s: the method must be GECM_METHOD_PM1 (P-1) or GECM_METHOD_PP1 (P+1)", who);
        return GECM_ERR_ARG;
    }
    if (batch == 0 || batch >= GECM_PAD || (!x0 && !x)) { set_err("%s: bad argument", who); return GECM_ERR_ARG; }
    if (!x && b1_done != 1) { set_err("%s: a fresh batch (x == NULL) has b1_done = 1", who); return GECM_ERR_ARG; }
    if (b1_done < 1 || b1_done > GECM_B1_MAX) { set_err("%s: b1_done must be in [1, %llu]", who, (unsigned long long)GECM_B1_MAX); return GECM_ERR_ARG; }
    if (!c->multi && c->mod.have_report) {
        set_err("%s: not with a report modulus (gecm_set_report_modulus): %s runs modulo the number the lines name", who,
                method_name(method));
        return GECM_ERR_STATE;
    }
    for (size_t i = 0; idx && i < batch; i++)
        if (idx[i] >= c->ngroups) {
            set_err("%s: modulus_index[%zu] = %u, the context has %zu moduli", who, i, idx[i], c->ngroups);
            return GECM_ERR_ARG;
        }
    const size_t words = (size_t)c->mod.nl * batch;
    uint32_t *planes = (uint32_t *)calloc(words * 3, 4);        /* x0 (or x), x (or x0), z = 1: the caller's order */
    if (!planes) return GECM_ERR_NOMEM;
    plain_job j = {c, {x0 ? x0 : x, x ? x : x0}, idx, batch, planes, batch};
    int rc = run_slices(batch, plain_slice, &j);
    if (rc > 0) {                                 /* the previous batch is untouched */
        set_err("%s: x0[%zu] or x[%zu] is not below its N", who, j.first_bad, j.first_bad);
        rc = GECM_ERR_ARG;
    } else if (!rc) {
        for (size_t i = 0; i < batch; i++) planes[2 * words + i] = 1;
        /* no sigmas, so no curves: the residues are all the batch holds, and S stays what it is */
        rc = batch_build(c, &(batch_desc){.who = who, .batch = batch, .modulus_index = idx, .content = BATCH_PLAIN,
                                          .planes = planes + words, .method = method, .seed = x0 ? planes : NULL});
        if (!rc) stage1_restart(c, b1_done);
    }
    free(planes);
    return rc;
}

int gecm_build_seeds(gecm_ctx *c, int method, const void *x0, const void *x, size_t batch, uint64_t b1_done)
{
    int rc;
    if (!c) { set_err("gecm_build_seeds: bad argument"); rc = GECM_ERR_ARG; }
    else if (c->multi) rc = multi_refuse("gecm_build_seeds");
    else rc = build_seeds(c, "gecm_build_seeds", method, NULL, x0, x, batch, b1_done);
    return build_call_end(c, rc);                 /* a pending setting does not apply to seeds: dropped unused */
}

int gecm_build_seeds_multi(gecm_ctx *c, int method, const uint32_t *modulus_index, const void *x0, const void *x,
                           size_t batch, uint64_t b1_done)
{
    int rc;
    if (!c || !modulus_index) { set_err("gecm_build_seeds_multi: bad argument"); rc = GECM_ERR_ARG; }
    else if (!c->multi) { set_err("gecm_build_seeds_multi: not a multi-modulus context (gecm_create_multi)"); rc = GECM_ERR_STATE; }
    else rc = build_seeds(c, "gecm_build_seeds_multi", method, modulus_index, x0, x, batch, b1_done);
    return build_call_end(c, rc);
}

int gecm_batch_method(const gecm_ctx *c) { return c && c->batch ? c->method : GECM_METHOD_ECM; }

int gecm_curve_seed(gecm_ctx *c, size_t k, char *hex, size_t hexlen)
{
    size_t pos;
    const gecm_mod *m = c && hex && hexlen ? curve_at(c, k, &pos) : NULL;
    if (!m) {
        if (!c || !c->multi) set_err("gecm_curve_seed: position %zu: no such residue in the batch", k);
        return GECM_ERR_ARG;
    }
    if (!c->method) { set_err("gecm_curve_seed: the batch holds curves, not P-1 / P+1 residues"); return GECM_ERR_STATE; }
    hex[0] = 0;
    if (!c->seed) return 0;
    mpl_t v;
    mpl_from_limbs32(&v, c->seed + pos, c->batch, m->nl, LIMB_BITS);
    static __thread char tmp[MPL_MAXL * 10 + 2];
    int n = mpl_get_hex(tmp, &v);
    if (n < 0 || (size_t)n >= hexlen) { set_err("gecm_curve_seed: buffer too small"); return GECM_ERR_ARG; }
    memcpy(hex, tmp, (size_t)n + 1);
    return n;
}

int gecm_curve_modulus(const gecm_ctx *c, size_t k)
{
    if (!c || !c->multi || k >= c->lay.nuser) { set_err("gecm_curve_modulus: no such curve in a multi-modulus batch"); return GECM_ERR_ARG; }
    return (int)c->lay.pos_grp[c->lay.slot[k]];
}

int gecm_curve_acc(gecm_ctx *c, size_t k, char *hex, size_t hexlen)
{
    if (c && c->wide) return wide_refuse("gecm_curve_acc");
    size_t pos;
    const gecm_mod *m = c && hex ? curve_at(c, k, &pos) : NULL;
    if (!m) return GECM_ERR_ARG;
    int rc = fetch_acc(c);
    if (rc) return rc;
    mpl_t v;
    mpl_from_limbs32(&v, c->hacc + pos, c->batch, m->nl, LIMB_BITS);
    mpl_mulmod(&v, &v, &m->int_to_ref, &m->N);                   /* what gecm_download_acc returns for the curve */
    static __thread char tmp[MPL_MAXL * 10 + 2];
    int n = mpl_get_hex(tmp, &v);
    if (n < 0 || (size_t)n >= hexlen) { set_err("gecm_curve_acc: buffer too small"); return GECM_ERR_ARG; }
    memcpy(hex, tmp, (size_t)n + 1);
    return n;
}

/* the hash of the host sources this object was compiled from (Makefile: H_SHA); gecm_version() compares them */
#ifdef GECM_MANIFEST_FN
const char *GECM_MANIFEST_FN(void) { return GECM_MANIFEST; }
#endif
