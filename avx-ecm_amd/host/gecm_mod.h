/* gecm_mod.h — one number N and everything derived from it, and the host work that needs nothing else: the Suyama
 * curve construction, the failed-inversion records of stage 2, the factor report, and the position layout of a
 * multi-modulus batch (gecm_layout, with gecm_multi_positions).  No device, no batch state: a context (gecm_api.c)
 * holds one gecm_mod, a multi-modulus context one more per modulus and the gecm_layout of its batch. */
#ifndef GECM_MOD_H
#define GECM_MOD_H
#include "mpl.h"
#include "../csrc/gecm_ops.h"

#define LIMB_BITS 28

typedef struct {
    int digitbits, nwords, maxbits, nbits, nl;
    mpl_t N;
    mpl_t N_report;      /* gecm_set_report_modulus: the number the save lines name and factors are looked for in */
    int have_report;
    mpl_t rref_mod_n;    /* 2^(digitbits*nwords) mod N  = the reference's "one" */
    mpl_t rint_mod_n;    /* 2^(28*nl) mod N */
    mpl_t ref_to_int;    /* Rint * Rref^-1 mod N : x*Rref -> x*Rint by plain modular multiply */
    mpl_t int_to_ref;    /* Rref * Rint^-1 mod N */
    uint64_t rho_ref;
    uint32_t rho28;
    uint32_t *n28, *kp28, *one28, *fix28; /* fix28 = Rint^2/Rref mod N (see gecm_dev_l0) */
    uint32_t *r3_28;     /* Rint^3 mod N for the device inversion */
    uint32_t *finv28;    /* Rref^2/Rint mod N (see gecm_vecinvmod) */
    uint32_t inv_iters;  /* batches of 28 division steps after which the device inversion has converged for N */
} gecm_mod;
/* The constants of N as the device layer takes them (csrc/gecm_ops.h), pointing into the n28 block: valid as long as m.
 * Its r2 = Rint^2 mod N (plain residue -> Montgomery form on the device) is the block's last part, after finv28, and
 * has no pointer of its own in the struct: tests/test_inverse_model_cpu.py mirrors the struct as it is. */
gecm_devmod gecm_mod_devmod(const gecm_mod *m);

/* the calling thread's error text (gecm_last_error) */
extern __thread char gecm_mod_err[512];
void gecm_mod_set_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

/* N and everything derived from it, at nl limbs (0: pick_nl(bits of N), which also says — with 0 — that N is too
 * large); `who` prefixes the error texts.  On error m holds nothing to free. */
int gecm_mod_setup(gecm_mod *m, const char *who, const char *n_str, int digitbits, int nl, int (*pick_nl)(int nbits));
void gecm_mod_free(gecm_mod *m);
int gecm_mod_make_kp(uint32_t *kp, const mpl_t *mod, int nl);
void gecm_mod_pow2(mpl_t *r, unsigned e, const mpl_t *m);       /* 2^e mod m */

static inline const mpl_t *report_n(const gecm_mod *m) { return m->have_report ? &m->N_report : &m->N; }

/* g = gcd(value, N) -> the factor of the report modulus it holds; is it a proper one? */
static inline int to_report(const gecm_mod *m, mpl_t *g)
{
    if (m->have_report && !mpl_is_zero(g)) { mpl_t t = *g; mpl_gcd(g, &t, &m->N_report); }
    return mpl_cmp_u64(g, 1) > 0 && mpl_cmp(g, report_n(m)) != 0;
}

/* The Suyama construction for curves [lo, hi) of `sigma`, written to position off + k of arrays of stride `batch`
 * (gecm_mod_build_slice). */
typedef struct {
    const gecm_mod *m;
    const uint64_t *sigma;
    uint8_t *bad;             /* [batch], set where a denominator does not invert */
    size_t batch, off;
    uint32_t *hX, *hZ, *hS;   /* [nl][batch] */
    const uint8_t *param;     /* next to sigma: the parametrisation of every curve (below); NULL: Suyama's throughout */
} gecm_mod_build;
/* GECM_ERR_NOMEM, 1 if some curve was marked bad, else 0 */
int gecm_mod_build_slice(void *build, size_t lo, size_t hi);

/* GMP-ECM's PARAM 1 and PARAM 3 curves: B y^2 = x^3 + A x^2 + x with (A+2)/4 = d, start point (2 : 1),
 * d = sigma^2 / 2^64 mod N with 1 <= sigma < 2^64 (PARAM 1) or sigma / 2^32 mod N with 1 <= sigma < 2^32 (PARAM 3).  The
 * one place the two formulae live on the host: gecm_param_s and the host build both come here.
 * gecm_mod_param_sigma_ok: is sigma in the range of param (1 or 3)?   gecm_mod_param_unit: 2^-64 or 2^-32 mod N (N odd).
 * gecm_mod_param_d: d from sigma and that unit. */
int gecm_mod_param_sigma_ok(int param, uint64_t sigma);
void gecm_mod_param_unit(mpl_t *unit, int param, const mpl_t *N);
void gecm_mod_param_d(mpl_t *d, int param, uint64_t sigma, const mpl_t *unit, const mpl_t *N);

/* the failed-inversion record of the curve at position k of hfail ([planes][nl][batch]): 0 or a divisor of N */
void gecm_mod_fail_record(const gecm_mod *m, const uint32_t *hfail, uint32_t planes, size_t batch, size_t k, mpl_t *g);

/* g = gcd(value, N): 1 with the decimal string and PRP test if it holds a proper factor of the report modulus,
 * else 0; GECM_ERR_ARG "<who>: buffer too small" */
int gecm_mod_factor(const gecm_mod *m, mpl_t *g, const char *who, char *dec, size_t declen, int *is_prp);

/* The constants of the row kernels for one number at the shape of a context of nl limbs (L = nl + 1 limbs in use): w, the
 * 32-lanes-per-curve stage-1 kernel's GECM_ROW_KINDS x GECM_ROW_WORDS words, and u, the 16-lane method kernel's
 * GECM_UROW_SET words (csrc/gecm_rowk.h); either may be NULL.  1 if made, 0 if this N has none.  See gecm_mod.c. */
int gecm_mod_row_consts(const gecm_mod *mod, int nl, int L, uint32_t *w, uint32_t *u);

/* ---- wide contexts (gecm_create_wide): numbers of up to GECM_WIDE_MAX_BITS bits on 40, 43 or 47 limbs ----
 * The device runs stage 1 alone and leaves lazy residues; what follows is host work and lives here, away from any device.
 * gecm_mod_wide_nl: the smallest wide limb count with 28 nl >= nbits + 5, or 0 above GECM_WIDE_MAX_BITS (the argument
 * of gecm_mod_setup for a wide context).
 * gecm_mod_raw_value: the integer sum of limb[i] 2^(28 i) over count limbs `stride` apart, the limbs being ANY 32-bit
 * words (mpl_from_limbs32 wants them below 2^28).
 * gecm_mod_raw_slice: curves [lo, hi) of a batch from the raw limbs of the kernel, rawX and rawZ ([nl][batch]), to the
 * canonical plain residues hx, hz ([nl][batch]): the value modulo N (the canonical Montgomery form x R mod N) times
 * rinv = R^-1 mod N.  gecm_mod_gcd_slice: g = gcd(z, N) of those curves from hz into hg ([nl][batch]), and
 * flags[k] = 1 iff 1 < g < N.  Both are run_slices workers: they return 0. */
#define GECM_WIDE_MAX_BITS 1311
int gecm_mod_wide_nl(int nbits);
void gecm_mod_raw_value(mpl_t *r, const uint32_t *limbs, size_t stride, int count);
typedef struct {
    const gecm_mod *m;
    mpl_t rinv;                       /* R^-1 mod N, R = 2^(28 nl) */
    size_t batch;
    const uint32_t *rawX, *rawZ;      /* gecm_mod_raw_slice reads */
    uint32_t *hx, *hz;                /* ... and writes; gecm_mod_gcd_slice reads hz */
    uint32_t *hg, *flags;             /* gecm_mod_gcd_slice writes */
} gecm_mod_wide_job;
int gecm_mod_raw_slice(void *job, size_t lo, size_t hi);
int gecm_mod_gcd_slice(void *job, size_t lo, size_t hi);

/* The positions of a multi-modulus batch: the moduli in order, each one's curves in the caller's
 * order.  Wave packing pads every modulus that has curves to whole blocks of 64 positions; lane packing lays them back
 * to back and pads the batch's tail, on modulus 0.  gecm_multi_positions (include/gecm.h) is the padding rule.  A
 * single-N batch has no layout: position = curve, and the struct stays zero. */
#define GECM_PAD 0xffffffffu
typedef struct {
    size_t nuser, total, ngroups;
    uint32_t *slot;          /* [nuser]      caller's curve -> position */
    uint32_t *pos_user;      /* [total]      position -> caller's curve, GECM_PAD for padding */
    uint32_t *pos_grp;       /* [total]      position -> modulus */
    uint32_t *blocks;        /* [total / 64] wave packing: the modulus of every block; NULL under lane packing */
    size_t *goff, *cnt;      /* [ngroups]    first position and curve count of every modulus */
} gecm_layout;
/* GECM_ERR_NOMEM; GECM_ERR_ARG: no curve or GECM_PAD or more positions, no modulus, some modulus_index[i] >= ngroups.
 * On error l holds nothing to free; gecm_layout_free leaves l zero and may be called again. */
int gecm_layout_make(gecm_layout *l, const uint32_t *modulus_index, size_t batch, size_t ngroups, int packing);
void gecm_layout_free(gecm_layout *l);
#endif
