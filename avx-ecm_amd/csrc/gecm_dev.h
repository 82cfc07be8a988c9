/* gecm_dev.h — internal device layer (HIP side) of libgecm.  Plain C interface so that the
 * host logic (C, gcc) never sees HIP types.  Not part of the public ABI (that is include/gecm.h).
 *
 * All residues crossing this layer are NL limbs of 28 bits in uint32_t, struct-of-arrays
 * [limb][curve] (curve index fastest: consecutive lanes of a wavefront read consecutive words),
 * in the engine's internal Montgomery form (R = 2^(28*NL)) unless a function says otherwise.
 */
#ifndef GECM_DEV_H
#define GECM_DEV_H
#include <stddef.h>
#include <stdint.h>
#include "gecm_ops.h"
#include "gecm_rowk.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct gecm_dev gecm_dev;


int gecm_dev_count(void);
/* hashes of the sources the device objects were compiled from: "K:.. R:.. D:.." (Makefile; K = MIXED if the kernel
 * objects disagree) */
const char *gecm_dev_manifest(void);
const char *gecm_dev_error(void);
/* limb counts for which kernels are instantiated, ascending, 0-terminated */
const int *gecm_dev_supported_nl(void);

/* m: the constants of the context's modulus at nl limbs (gecm_ops.h), copied before it returns.  multi != 0: a
 * multi-modulus context, m the modulus gecm_get_config reports; see gecm_dev_set_groups. */
int gecm_dev_open(gecm_dev **out, int device, int nl, const gecm_devmod *m, int multi);
/* ---- a wide context: nl = 40, 43 or 47, limb counts that have the 32-lane stage-1 kernel of
 * gecm_launch_stage1_row_wide and no other.  It holds no modulus constants but those of gecm_dev_set_rowconst (rho is the
 * exit multiply's -N^-1 mod 2^28), and serves gecm_dev_close, _device_name, _memory, _batch_bytes (stage-1 arrays; 0
 * with npb != 0), _resize, _stride, _upload (limbs the host has put into Montgomery form), _set_tape, _set_rowconst,
 * _stage1 (lanes 0 or 32: the row kernel per cut of the tape and NOTHING between or after the launches, the exit values
 * stay lazy), _stage1_progress, _sync, _last_kernel_ms, _last_kernel, _last_lanes, _cus and gecm_dev_download_raw.
 * Every other call answers -2 with a text and touches nothing. */
int gecm_dev_open_wide(gecm_dev **out, int device, int nl, uint32_t rho);
int gecm_dev_is_wide(const gecm_dev *d);
/* X, Z limb for limb as the last kernel left them ([limb][curve]): of a wide context lazy values, limbs below
 * 2^28 + 16 and the top limb whatever the value t + K' < R/16 + 2N needs.  Any context. */
int gecm_dev_download_raw(gecm_dev *d, uint32_t *X, uint32_t *Z);
void gecm_dev_close(gecm_dev *d);
int gecm_dev_device_name(gecm_dev *d, char *buf, size_t len);
int gecm_dev_memory(gecm_dev *d, uint64_t *free_bytes, uint64_t *total_bytes);   /* hipMemGetInfo */
/* device bytes of a batch: stage-1 arrays, plus (npb != 0) the stage-2 allocations for that table / chunk / ring size */
uint64_t gecm_dev_batch_bytes(gecm_dev *d, size_t curves, uint32_t npb, uint32_t G, uint32_t ring_size);

/* (re)allocate state for ncurves curves: X, Z, S (+ scratch for downloads) */
int gecm_dev_resize(gecm_dev *d, size_t ncurves);
size_t gecm_dev_stride(gecm_dev *d);
int gecm_dev_upload(gecm_dev *d, const uint32_t *X, const uint32_t *Z, const uint32_t *S);
int gecm_dev_upload_xz(gecm_dev *d, const uint32_t *X, const uint32_t *Z);   /* X, Z only; S untouched */
/* X, Z from canonical PLAIN residues x, z in [0, N) ([limb][curve], not Montgomery form): the device multiplies each by
 * R^2 mod N (a multi-modulus context: by that of the curve's own modulus).  S untouched; the padding lanes get
 * x = z = 1.  Synchronous. */
int gecm_dev_upload_plain(gecm_dev *d, const uint32_t *x, const uint32_t *z);
/* canonical Montgomery-form S = (A+2)/4 of the batch */
int gecm_dev_download_s(gecm_dev *d, uint32_t *S);
/* ---- curve construction on the device (csrc/gecm_kernels.hip: k_build) ----
 * gecm_dev_build: the Suyama curves of sigma[0 .. count) into X, Z, S of the batch; count is what gecm_dev_resize was
 * given (a multi-modulus context: sigma in device order, any value in the padding).  Inverts.  flags[i] = 1 where a
 * denominator of curve i had no inverse.  Synchronous; the kernel's own time is gecm_dev_last_build_ms.
 * gecm_dev_fill_twin: X, Z, S of dst (a context modulo Mw, N | Mw, on the same device with a batch of the same size)
 * from those of src, on the device: out of src's Montgomery form, the limb planes copied (zero-filled or cut to dst's
 * limb count), into dst's with dst's own R^2 mod Mw.  Synchronous. */
int gecm_dev_build(gecm_dev *d, const uint64_t *sigma, size_t count, uint32_t *flags);
float gecm_dev_last_build_ms(gecm_dev *d);
/* gecm_dev_build for a batch with a parametrisation per curve (param[i] = 0, 1 or 3, the padding of a
 * multi-modulus batch 0): k_build over the batch as gecm_dev_build launches it whenever some param[i] is 0 — the other
 * lanes compute a Suyama curve nobody reads — then k_build_param, which overwrites X, Z, S and the flag (with 0) of the
 * lanes whose parameter is not 0.  Without a 0 among param the first kernel is skipped (and does not need r3), the
 * planes are cleared first.  gecm_dev_last_build_ms is the sum of the kernels launched. */
int gecm_dev_build_param(gecm_dev *d, const uint64_t *sigma, const uint8_t *param, size_t count, uint32_t *flags);
int gecm_dev_fill_twin(gecm_dev *dst, gecm_dev *src);
/* X <- X/Z, Z <- R mod N in the batch planes (canonical), for every curve whose Z has an inverse; the others keep both
 * and get flags[i] = 1 (count = the batch's curves, padding included as for gecm_dev_build).  Inverts.
 * Synchronous; the kernel's own time is gecm_dev_last_build_ms. */
int gecm_dev_normalize(gecm_dev *d, uint32_t *flags);
int gecm_dev_set_tape(gecm_dev *d, const uint8_t *tape, size_t len);
/* stage 1: asynchronous on the context's stream; HIP events bracket the kernel */
/* lanes_per_curve: 1 = one curve per lane, 2 = X and Z of a curve on two adjacent lanes (for batches
 * too small to fill the chip), 0 = let the device layer choose from the batch size and CU count */
int gecm_dev_stage1(gecm_dev *d, int lanes_per_curve);
int gecm_dev_auto_lanes(gecm_dev *d);
/* launches of the last gecm_dev_stage1 finished so far / made (a long tape is cut into several, gecm_dev_set_tape) */
int gecm_dev_stage1_progress(gecm_dev *d, uint32_t *done, uint32_t *total);
/* constants of the 32-lanes-per-curve kernel (csrc/gecm_row.hpp): nq limbs per lane, rows per multiply
 * (gecm_row_shape), GECM_ROW_KINDS x
 * GECM_ROW_WORDS words (N' = m*N = -1 mod 2^28; N; entry factor; R mod N; K' of N), limb j at word j */
int gecm_dev_set_rowconst(gecm_dev *d, int nq, int rows, const uint32_t *words);
/* F-form (modulus 2^k - 1, csrc/gecm_field.hpp): number of top limbs the kernel for `nl` limbs reads from
 * the modulus (all limbs below must be 2^28 - 1), and the switch that makes gecm_dev_stage1 use it. */
int gecm_dev_fform_generic_limbs(int nl);
void gecm_dev_set_fform(gecm_dev *d, int form);   /* +1: 2^k - 1, -1: 2^k + 1, 2: 2^k - c (limbs 0, 1 below F), 0: off */
int gecm_dev_last_lanes(gecm_dev *d);
/* name of the stage-1 kernel the last launch ran, as rocprofv3 prints it ("k_stage1_row<1, 16, false>") */
const char *gecm_dev_last_kernel(gecm_dev *d);
int gecm_dev_sync(gecm_dev *d);
float gecm_dev_last_kernel_ms(gecm_dev *d);
/* canonical Montgomery-form X, Z (what P holds after ecm_stage1 in the reference, modulo R) */
int gecm_dev_download_mont(gecm_dev *d, uint32_t *X, uint32_t *Z);
/* canonical de-Montgomeryised x, z (the reference's X*1, Z*1 of ecm.c:1327-1331) */
int gecm_dev_download_plain(gecm_dev *d, uint32_t *x, uint32_t *z);

/* test-level L0 operators on `count` independent residues.  Inputs canonical (< N), internal
 * Montgomery form; outputs canonical.  For MUL/SQR the product is additionally multiplied by
 * the constant `fix` (internal Montgomery form; pass `one` for none): this is how the public
 * ABI returns results in the reference's own Montgomery radix. */
int gecm_dev_l0(gecm_dev *d, int op, const uint32_t *a, const uint32_t *b, uint32_t *c, uint32_t *dd,
                size_t count, const uint32_t *fix);
/* test-level inversion of `count` independent residues with the stage-2 inversion (fe_inv_mont; needs the context's
 * r3).  a canonical; inv = the inverse as fe_inv_mont returns it, multiplied by the constant `fix`
 * (internal Montgomery form) and canonical, or 0 where gcd(a, N) != 1; g = gcd(a, N), a plain integer. */
int gecm_dev_l0_inv(gecm_dev *d, const uint32_t *a, uint32_t *inv, uint32_t *g, size_t count, const uint32_t *fix);
/* The raw test-level operator (k_l0_raw): r = op(a, b) for `count` residues, op = GECM_L0_MUL, _SQR, _ADD, _SUB or
 * _CONDSUB (fe_cond_sub_n of a; b may be NULL for the one-operand operators), by the field function itself on the limbs
 * exactly as given — any 32-bit words: no canonical check, no Montgomery form assumed — and the limbs exactly as the
 * function left them.  special != 0: the multiply gecm_dev_set_fform chose for this context (its fe_add, fe_sub and
 * fe_cond_sub_n are the generic ones), else the generic REDC.  A single-modulus context takes any count; a
 * multi-modulus context must hold a lane-packed batch and takes count = its positions, padding included: residue p is
 * worked on modulo the N of position p.  Works in device memory of its own: the batch stays as it is.  Values outside
 * the bounds of csrc/gecm_field.hpp give unspecified limbs, nothing else. */
int gecm_dev_l0_raw(gecm_dev *d, int op, int special, const uint32_t *a, const uint32_t *b, uint32_t *r, size_t count);

/* ---- multi-modulus batches ----
 * A context opened with multi != 0 takes the modulus of every launch from device tables, with 1 or 2 lanes per curve
 * and one stage-2 sub-sequence per curve (until gecm_dev_set_s2_subseq says otherwise); the L0 operators are refused.
 * gecm_dev_set_groups, once per batch (a gecm_dev_resize ends what it set): the constants of the batch's ngroups
 * moduli, r3 included, and which modulus goes where.  curve_group == NULL, wave packing: block_group names the modulus
 * of every 64-curve block (stride / 64 entries).  curve_group != NULL, lane packing: it names the modulus of every curve
 * position (stride entries, the padding included), block_group is not read, and the launches of this batch run the
 * per-lane kernels: a modulus per lane, one lane per curve (gecm_dev_stage1 refuses two).  Every entry < ngroups.
 * Host memory, copied before it returns.  gecm_dev_lane_packing_built: whether the per-lane kernels exist at this
 * limb count. */
int gecm_dev_set_groups(gecm_dev *d, uint32_t ngroups, const gecm_devmod *mods, const uint32_t *block_group,
                        const uint32_t *curve_group);
int gecm_dev_lane_packing_built(int nl);
/* ---- stage 1 of such a batch with 32 lanes per curve (csrc/gecm_rowk.hip: k_stage1_row_multi) ----
 * gecm_dev_set_multi_rowconst: the constant sets of the kernel, one for every modulus gecm_dev_set_groups names, in that
 * order (gecm_rowk.h: GECM_MROW_SET words each), with nq limbs per lane and rows per multiply of the context's limb count
 * (gecm_row_shape).  Host memory, copied before it returns; -2 on a single-modulus context.
 * gecm_dev_multi_rows_ready: are there sets for the moduli of the batch?
 * gecm_dev_stage1_multi_rows: gecm_dev_stage1 with that kernel on either packing, then canon, per launch of a cut tape
 * (-2 without constants); gecm_dev_last_lanes is then 32.  gecm_dev_stage1 itself answers as it always has. */
int gecm_dev_set_multi_rowconst(gecm_dev *d, int nq, int rows, uint32_t ngroups, const uint32_t *words);
int gecm_dev_multi_rows_ready(gecm_dev *d);
int gecm_dev_stage1_multi_rows(gecm_dev *d);

/* ---- stage 2 (csrc/gecm_stage2.hpp) ----
 * ecm_stage2_init: baby-step table (npb entries, X/Z normalised), Pd = [D]Q, acc = one.  Inverts.
 * keep: bitmap over j in [0, umax], bit set iff j is stored.  L = ring half-size (2L giant steps). */
/* K = gecm_dev_s2_subseq(d) sub-sequences per curve (1: the plain chain).  For K > 1: tgt_off[r] .. tgt_off[r+1] is
 * the range of tgt[] holding the table indices of the kept members j = r, r+K, ... (r = 0: K, 2K, ...) of
 * sub-sequence r, in order; tgt_off has K + 1 entries. */
uint32_t gecm_dev_s2_subseq(gecm_dev *d);
/* k = 0: K by batch size on a single-modulus context, 1 on a multi-modulus one (the default); -1: by batch size on
 * both; 1, 2, 4, .. 32: that K.  Takes effect at the next gecm_dev_s2_init; -2 for any other value.
 * gecm_dev_s2_k_chunks: giant-step chunks launched with sub-sequences since the last gecm_dev_s2_init. */
int gecm_dev_set_s2_subseq(gecm_dev *d, int k);
uint32_t gecm_dev_s2_k_chunks(gecm_dev *d);
int gecm_dev_s2_init(gecm_dev *d, const uint32_t *keep, size_t keep_words, uint32_t umax, uint32_t D,
                     uint32_t npb, uint32_t G, uint32_t ring_size, const uint32_t *tgt, const uint32_t *tgt_off,
                     uint32_t K);
/* failure records come in planes of [limb][curve]: plane 0 from the single-chain inversions, plane 1 + r from
 * sub-sequence r; gecm_dev_s2_download fills all of them */
uint32_t gecm_dev_s2_fail_planes(gecm_dev *d);
/* ecm_stage2_pair for one range: steps = nsteps words pairs: (0xffffffff, n) = generate the next n
 * giant steps (n <= G), else (ring slot, table index).  G = chunk size, ring_size = power of two. */
int gecm_dev_s2_pair(gecm_dev *d, const uint32_t *steps, uint32_t nsteps, uint32_t D, uint32_t G,
                     uint32_t ring_size, uint64_t A0, uint64_t tape_id);
#define GECM_S2_BLK 256   /* baby-step normalisation block (= S2_BLK in gecm_stage2.hpp) */
/* canonical Montgomery-form accumulator and the failed-inversion gcd records ([limb][curve]) */
int gecm_dev_s2_download(gecm_dev *d, uint32_t *acc, uint32_t *fail);
/* factor scan on the device: which = 0 -> stage-1 Z, 1 -> stage-2 accumulator.  flags[curve] = 1 iff
 * 1 < gcd(value, N) < N; g = the gcds ([limb][curve]); either output may be NULL. */
int gecm_dev_gcd_scan(gecm_dev *d, int which, uint32_t *flags, uint32_t *g);

/* ---- P-1 and P+1 stage 1: the residues in X of the batch (gecm_dev_upload_plain with z = 1) ----
 * gecm_dev_stage1_unit_lanes: the tape of gecm_dev_set_tape on every residue, x <- x^E (P-1) or V_E(x) (P+1), canonical;
 * asynchronous and cut into launches like gecm_dev_stage1, on any kind of context (lane-packed where the per-lane kernels
 * are built).  lanes = 1: a residue per lane.  lanes = 16: a residue per 16-lane DPP row (csrc/gecm_row.hpp:
 * k_unit_row) and canon per launch, -2 without constants.  gecm_dev_last_lanes is then `lanes`.
 * gecm_dev_set_unit_rowconst: the constant sets of k_unit_row, one per modulus (gecm_rowk.h: GECM_UROW_SET words each; a
 * single-N context has one, a multi-modulus context one for every modulus gecm_dev_set_groups names, in that order), with
 * nq limbs per lane and rows per multiply of the context's limb count (gecm_row_shape).  Host memory, copied before it
 * returns.  gecm_dev_unit_rows_ready: are there sets for the moduli of the batch?
 * gecm_dev_gcd_scan_off: gecm_dev_gcd_scan of x - off, off = 1 (P-1) or 2 (P+1). */
#define GECM_UNIT_PM1 1
#define GECM_UNIT_PP1 2
int gecm_dev_set_unit_rowconst(gecm_dev *d, int nq, int rows, uint32_t ngroups, const uint32_t *words);
int gecm_dev_unit_rows_ready(gecm_dev *d);
int gecm_dev_stage1_unit_lanes(gecm_dev *d, int method, int lanes);
int gecm_dev_cus(gecm_dev *d);                 /* compute units of the device */
int gecm_dev_gcd_scan_off(gecm_dev *d, uint32_t off, uint32_t *flags, uint32_t *g);
/* ---- stage 2 of such a batch: gecm_dev_s2_init / gecm_dev_s2_pair with the method as first argument ----
 * The same allocations, slices and K; the table and the giant steps are values V_n(P) of the Lucas sequence of
 * P = x (P+1) or x + 1/x (P-1), written to S of the batch (X and Z stay as they are); the pair walk, the merge,
 * gecm_dev_s2_download and gecm_dev_gcd_scan(which = 1) are shared.  Only P-1 inverts, once per position: where x has
 * no inverse, plane 0 of the failure record takes gcd(x, N).  Bit 31 of a "generate" mark is ignored. */
int gecm_dev_s2_init_unit(gecm_dev *d, int method, const uint32_t *keep, size_t keep_words, uint32_t umax, uint32_t D,
                          uint32_t npb, uint32_t G, uint32_t ring_size, const uint32_t *tgt, const uint32_t *tgt_off,
                          uint32_t K);
int gecm_dev_s2_pair_unit(gecm_dev *d, int method, const uint32_t *steps, uint32_t nsteps, uint32_t D, uint32_t G,
                          uint32_t ring_size, uint64_t A0, uint64_t tape_id);

#ifdef __cplusplus
}
#endif
#endif
