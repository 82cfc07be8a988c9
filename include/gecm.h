/* gecm.h — public C ABI of libgecm, the MI355X-native engine for the hot path of bbuhrow/avx-ecm.
 *
 * Drop-in boundary.  The reference reaches its hot path through
 *   (L0) five global function pointers bound in main.c:642-702 and declared in avx_ecm.h:205-209:
 *          vecmulmod_ptr / vecsqrmod_ptr / vecaddmod_ptr / vecsubmod_ptr / vecaddsubmod_ptr
 *   (L1) four per-thread phase functions dispatched by vececm through tpool_go
 *        (ecm.c:1195, 1234, 1407, 1460):
 *          ecm_build_curve_work_fcn  ecm.c:201-246   -> build_one_curve ecm.c:1548-1803
 *          ecm_stage1_work_fcn       ecm.c:167-176   -> ecm_stage1      ecm.c:1806-1854
 *          ecm_stage2_init_work_fcn  ecm.c:178-186   -> ecm_stage2_init ecm.c:2201-2340
 *          ecm_stage2_work_fcn       ecm.c:188-199   -> ecm_stage2_pair ecm.c:2342-2540
 * This header exports exactly those seams, on a batch of B curves instead of VECLEN=8/16 lanes.
 * Every entry point is extern "C", takes plain pointers and sizes, returns an int status
 * (0 = ok, < 0 = error; text from gecm_last_error()), and never exits the process (the reference
 * printf+exit()s: util.c:56-59, ecm.c:969-970).
 *
 * Vector operands ("vec") use the REFERENCE's memory layout (avx_ecm.h:111-116, main.c:117-138):
 *   data[lane + limb * batch], limb-major / curve-minor, limbs of DIGITBITS bits held in
 *   uint64_t (DIGITBITS = 52) or uint32_t (DIGITBITS = 32), NWORDS limbs per value, values in the
 *   reference's Montgomery form x * 2^(DIGITBITS*NWORDS) mod N, canonical in [0, N).
 * So a maintainer can pass bignum->data straight through (with batch = VECLEN) — INTEGRATION.md.
 *
 * Ownership: the context owns all device memory; every host array is caller-owned and copied.
 * Threading: one context per GPU, used by one host thread at a time; contexts are independent.
 */
#ifndef GECM_H
#define GECM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct gecm_ctx gecm_ctx;

#define GECM_OK 0
#define GECM_ERR_ARG (-2)
#define GECM_ERR_DEVICE (-1)
#define GECM_ERR_NOMEM (-3)
#define GECM_ERR_STATE (-4)

const char *gecm_last_error(void);
int gecm_device_count(void);
const char *gecm_version(void);

/* ---- configuration (replaces monty_alloc + main.c:465-483, 597-640) ------------------------
 * n_str: the number to factor, decimal or 0x-hex (odd, > 1).
 * digitbits: 52 or 32 — the reference limb format used at THIS boundary (vec operands,
 *            NWORDS rule: smallest multiple of 208 (resp. 128) bits strictly greater than
 *            bitlen(N), main.c:465-483).  The device arithmetic is the same either way.
 * device: HIP device ordinal.                                                                 */
int gecm_create(gecm_ctx **out, int device, const char *n_str, int digitbits);
void gecm_destroy(gecm_ctx *ctx);

typedef struct {
    int digitbits;   /* 52 | 32                                   (avx_ecm.h:65-93)   */
    int nwords;      /* NWORDS                                    (main.c:482)        */
    int maxbits;     /* MAXBITS = DIGITBITS * NWORDS                                  */
    int nbits;       /* bitlen(N)                                                     */
    int dev_limbs;   /* 28-bit limbs per residue on the device                         */
    int device;
    uint64_t rho;    /* -N^-1 mod 2^DIGITBITS  (monty->vrho, main.c:636-640)           */
} gecm_config;
int gecm_get_config(const gecm_ctx *ctx, gecm_config *cfg);
int gecm_device_name(gecm_ctx *ctx, char *buf, size_t len);
/* free and total device memory right now (hipMemGetInfo), and the device bytes a batch of `curves` curves takes (stage 1
 * only, or with the stage-2 tables of wheel D and height U; 0 = the defaults for B1): what a caller sizes its batches
 * with.  The reference has no counterpart (its tables are per thread, ecm_work_init).                                */
int gecm_device_memory(gecm_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);
uint64_t gecm_batch_bytes(const gecm_ctx *ctx, size_t curves, int with_stage2, uint64_t B1, uint32_t D, uint32_t U);
/* "one" = R mod N in the reference limb format, single value (monty->one, main.c:633-634) */
int gecm_get_one(const gecm_ctx *ctx, void *one_limbs);

/* ---- L0: the five vector operators (avx_ecm.h:205-209), and the device inversion -----------
 * Test-level exports: same semantics as vecmulmod52/vecsqrmod52/vecaddmod52/vecsubmod52/
 * vec_simul_addsub52 (vecarith52.c:2438, 3317, 4550, 4684, 4877) and their 32-bit twins
 * (vecarith.c:221, 889, 2806, 2870, 2726): inputs canonical, outputs canonical, Montgomery
 * radix 2^(DIGITBITS*NWORDS).  `c` may alias `a` or `b`.  batch >= 1, any size.              */
int gecm_vecmulmod(gecm_ctx *ctx, const void *a, const void *b, void *c, size_t batch);
int gecm_vecsqrmod(gecm_ctx *ctx, const void *a, void *c, size_t batch);
int gecm_vecaddmod(gecm_ctx *ctx, const void *a, const void *b, void *c, size_t batch);
int gecm_vecsubmod(gecm_ctx *ctx, const void *a, const void *b, void *c, size_t batch);
int gecm_vecaddsubmod(gecm_ctx *ctx, const void *a, const void *b, void *sum, void *diff, size_t batch);
/* A sixth test-level operator with no counterpart among the reference's function pointers (it inverts on the host,
 * mpz_invert, ecm.c:1919-1950): the device's own modular inversion, the routine every stage-2 batch inversion and the
 * factor scan run, on inputs of the caller's choice.  a as above (canonical, a = x * 2^(DIGITBITS*NWORDS) mod N);
 * inv[i] = x^-1 * 2^(DIGITBITS*NWORDS) mod N, canonical, or 0 when gcd(a_i, N) != 1; gcd[i] = gcd(a_i, N) as a plain
 * integer in the same vec layout (N for a_i = 0).  inv and gcd must not alias each other.                      */
int gecm_vecinvmod(gecm_ctx *ctx, const void *a, void *inv, void *gcd, size_t batch);
/* A seventh, below the other six: one function of the device's one-lane field arithmetic (csrc/gecm_field.hpp: fe_mul,
 * fe_sqr, fe_add, fe_sub, fe_cond_sub_n) on limbs of the caller's choice, and the limbs it leaves.  A residue is
 * `limbs` 32-bit words, limb j of residue i at [i + j * count] — raw device limbs of 28 bits and whatever the caller
 * puts above them: nothing is checked against N, nothing is converted to or from a Montgomery radix, no canonical form
 * is made of the result.  This is how the lazy operands of the ladders (products, sums, differences at the bounds the
 * header of gecm_field.hpp states) reach the multiply directly.  Inputs outside those bounds give unspecified limbs
 * and nothing worse: the kernel does register arithmetic on what it loaded.  b may be NULL for GECM_RAW_SQR and
 * GECM_RAW_CONDSUB.  target says modulo what, and with which multiply:
 *   GECM_RAW_OWN    the context's N, generic REDC; limbs = gecm_config.dev_limbs, any count.
 *   GECM_RAW_TWIN   the modulus Mw of the special-form twin with its special multiply (2^k - 1, 2^k + 1, 2^k - c);
 *                   limbs = what gecm_get_special_form reports; GECM_ERR_STATE for an N without a twin.
 *   GECM_RAW_BATCH  a multi-modulus context holding a lane-packed batch: count = the positions of the batch
 *                   (gecm_multi_positions), residue p is worked on modulo the number of position p, every lane with its
 *                   own constants; limbs = gecm_config.dev_limbs.  The batch itself is not touched.
 * Sizes and state are checked, values never.                                                                        */
enum { GECM_RAW_MUL = 0, GECM_RAW_SQR = 1, GECM_RAW_ADD = 2, GECM_RAW_SUB = 3, GECM_RAW_CONDSUB = 4 };
enum { GECM_RAW_OWN = 0, GECM_RAW_TWIN = 1, GECM_RAW_BATCH = 2 };
int gecm_vecrawop(gecm_ctx *ctx, int target, int op, const uint32_t *a, const uint32_t *b, uint32_t *r, size_t count);

/* ---- L1 phase 0: curve construction (build_one_curve, ecm.c:1548-1803) ---------------------
 * Suyama parametrisation from sigma[0..batch): the context computes X, Z (=1), s = (A+2)/4 on the
 * host and uploads them.  sigma values must be >= 6 (the reference redraws below 6,
 * ecm.c:1564-1570).  Returns GECM_OK, or 1 if some curve's setup inversion failed because
 * gcd(denominator, N) > 1; such lanes continue exactly as the reference does (it ignores
 * mpz_invert's return value, ecm.c:1745, 1759, and goes on with the stale operand).           */
int gecm_build_curves(gecm_ctx *ctx, const uint64_t *sigma, size_t batch);
/* Alternative phase 0: caller supplies P=(X,Z) and s as vec operands (reference layout and
 * Montgomery radix), e.g. the output of the reference's own build_one_curve.                 */
int gecm_upload_points(gecm_ctx *ctx, const void *X, const void *Z, const void *s, size_t batch);
/* Where the Suyama construction runs.  GECM_BUILD_HOST (the default): big-integer arithmetic on worker threads, then
 * an upload.  GECM_BUILD_DEVICE: one kernel, a curve per lane, in the device's Montgomery arithmetic with its own
 * inversion; the batch holds the same words either way, stale operands of a failed inversion and the
 * return value 1 included, so every file and every result is the same.  Takes effect at the next gecm_build_curves,
 * gecm_build_curves_multi, gecm_resume_points or gecm_resume_points_multi (there s comes from the device, X and Z from
 * the caller); the argument checks of those calls stay on the host.  After a device build gecm_last_kernel_ms is the
 * build kernel's time.  GECM_ERR_ARG for another value or a NULL context.
 * gecm_get_curve_build: what the last build of the context used (GECM_BUILD_HOST before the first). */
#define GECM_BUILD_HOST 0
#define GECM_BUILD_DEVICE 1
int gecm_set_curve_build(gecm_ctx *ctx, int where);
int gecm_get_curve_build(const gecm_ctx *ctx);
/* s = (A+2)/4 of the batch as a vec operand (reference layout and Montgomery radix, canonical): the counterpart of
 * gecm_upload_points' third argument.  GECM_ERR_STATE on a multi-modulus context, like gecm_download_points. */
int gecm_download_s(gecm_ctx *ctx, void *s);

/* ---- GMP-ECM's other parametrisations ----------------------------------------------
 * GMP-ECM 7 writes PARAM 1 on 64-bit CPUs at ordinary B1 and PARAM 3 from its GPU stage 1; both are curves
 * B y^2 = x^3 + A x^2 + x with A = 4d - 2, so s = (A+2)/4 = d, and the start point (X : Z) = (2 : 1):
 *   GECM_PARAM_BATCH_SQUARE (1): d = sigma^2 / 2^64 mod N, 1 <= sigma < 2^64;
 *   GECM_PARAM_BATCH_32     (3): d = sigma / 2^32 mod N,   1 <= sigma < 2^32.
 * No inversion is involved: such a curve never sets a build flag and never makes a build call return 1.  sigma = 0
 * (d = 0, a singular curve) is refused; d = 1 (A = 2) is singular too, is not looked for and finds nothing.  PARAM 2 and
 * every value above 3 stay refused.  Their stage-1 multiplier is the standard one: a fresh PARAM 1 or 3 curve is run with
 * gecm_stage1_extend(ctx, 1, B1); gecm_stage1 stays allowed and writes PROGRAM=AVX-ECM lines, as on any batch.
 * gecm_param_s: s = d for param 1 or 3 in lower-case hex without prefix; returns the digit count.  Pure host code, no
 *   context.  GECM_ERR_ARG for param 0 (its s needs the inversion rule of a build), 2 and above, a SIGMA out of range, a
 *   bad N (odd, >= 3, decimal or 0x-hex) or a buffer too small.
 * gecm_set_next_params: the parametrisation of each curve of the NEXT gecm_build_curves, gecm_build_curves_multi,
 *   gecm_resume_points or gecm_resume_points_multi (the caller's order), as gecm_set_curve_build says where it runs.
 *   One-shot: that call takes the setting and clears it, whether it succeeds or not; param == NULL clears a pending one.
 *   Values other than 0, 1, 3 and batch == 0 are GECM_ERR_ARG.  A build whose batch differs from `batch`, or whose sigma
 *   is outside its parametrisation's range (sigma >= 6 for the PARAM 0 curves of the call), answers GECM_ERR_ARG and keeps
 *   the previous batch.  Mixed batches are allowed.  The PARAM 0 curves get exactly the words, flags, failure records and
 *   return value they get without a setting; the others X = 2, Z = 1, s = d (a resume: the caller's X and Z, s = d).
 *   With GECM_BUILD_DEVICE the Suyama kernel runs over the batch if it holds a PARAM 0 curve, then k_build_param
 *   overwrites the other curves; gecm_last_kernel_ms is the sum.  Without a pending setting every call is what it was.
 * gecm_curve_param: the parametrisation of the caller's curve k; 0 for every batch built without a setting.
 * Save lines carry it: gecm_format_save_line_std writes the curve's PARAM=, gecm_format_save_line and
 * gecm_format_resume_line insert "PARAM=%d; " after "METHOD=ECM; " for a curve whose parametrisation is not 0. */
#define GECM_PARAM_SUYAMA 0
#define GECM_PARAM_BATCH_SQUARE 1
#define GECM_PARAM_BATCH_32 3
int gecm_param_s(int param, uint64_t sigma, const char *n_str, char *hex, size_t hexlen);
int gecm_set_next_params(gecm_ctx *ctx, const uint8_t *param, size_t batch);
int gecm_curve_param(const gecm_ctx *ctx, size_t k);

/* ---- input preparation (main.c:393-527) -----------------------------------------------------
 * What the reference's main() does to its first argument before any curve is built: evaluate the
 * expression (calc.c), recognise N | 2^k - 1, N | 2^k + 1 or 2^k = c (mod N) with c below one limb
 * (main.c:405-441), and for the first two replace N by gcd(N, primitive part of 2^k -/+ 1)
 * (find_primitive_factor, main.c:187-352, 445-457).  n_dec receives the decimal N the run is made on;
 * log receives the lines the reference prints on the way ("gen: ...", "removing algebraic ...",
 * "commencing parallel ecm on ...", "Mersenne input ... determined to be faster by REDC"), byte for byte.
 * When the reference would fold modulo Mw = 2^k -/+ 1 or 2^k - c (ref_special_reduction = 1; main.c:505-527, 642-684,
 * vecarith52.c:284-2436) it works modulo Mw THROUGHOUT — curve construction included — and its files hold residues
 * modulo Mw next to "N=" the number given, in which it also looks for factors (ecm.c:1111-1118).  To write those
 * files byte for byte, create the context on Mw and name N with gecm_set_report_modulus (the command-line driver does;
 * nine reference runs in tests/golden/special.json).  A context created on N itself gives the residues modulo N of a
 * run modulo N — with the cheaper special-form multiply where it pays, gecm_set_special_form — which is what a
 * caller wants who is not after the reference's bytes.                                                              */
typedef struct {
    int form;                   /* the reference's isMersenne: 0, +1 (2^k - 1), -1 (2^k + 1), else c of 2^k - c */
    int k;
    uint64_t c;
    int nbits;                  /* bit length of the prepared N */
    int ref_special_reduction;  /* 1 = the reference would not use REDC for this input (main.c:505-527) */
} gecm_input_info;
int gecm_prepare_input(const char *expr, int digitbits, char *n_dec, size_t n_len, gecm_input_info *info,
                       char *log, size_t loglen);
/* The size the reference prints next to a factor ("found PRP45 factor ...", ecm.c:1346-1366, 1494-1520) is
 * mpz_sizeinbase(f, 10) = floor(bits * log10 2) + 1, which is the digit count or one more (a 12-digit
 * factor of 40 bits is labelled C13).  This returns that number for a decimal string.                 */
int gecm_sizeinbase10(const char *dec);
/* The number the save lines name ("N=0x...") and factors are reported of, when it is not the context's modulus but a
 * divisor of it: the reference's gmpn = vnhat for special-form inputs (ecm.c:1111-1118).  n_str decimal or 0x-hex, must
 * divide the modulus the context was created on; NULL restores the default.  gecm_stage1_factor, gecm_stage2_factor and
 * gecm_scan_factors then report gcd(value, n) as the reference's check_factor(value, gmpn) does.                      */
int gecm_set_report_modulus(gecm_ctx *ctx, const char *n_str);

/* ---- L1 phase 1: stage 1 (ecm_stage1, ecm.c:1806-1854) -------------------------------------
 * P <- [prod of prime powers < B1] P for every curve of the batch.  Asynchronous: returns after
 * the (last) launch; gecm_sync waits.  For B1 > 10^8 this is the whole loop of ecm.c:1209-1234:
 * gecm_stage1_range for range 0, 1, ... in turn.                                               */
int gecm_stage1(gecm_ctx *ctx, uint64_t B1);
int gecm_sync(gecm_ctx *ctx);
/* Stage 1 above one prime range.  vececm re-sieves every PRIME_RANGE = 10^8 and calls ecm_stage1 once per range
 * (ecm.c:1209-1234); between the calls it appends the batch to checkpoint.txt (ecm.c:1236-1312).  One
 * gecm_stage1_range call is one of those ecm_stage1 calls, with the reference's behaviour there reproduced so that
 * the residues stay bit-identical: every call runs the 2-power doublings again (ecm.c:1815-1822) and starts at the
 * SECOND prime of its range (ecm.c:1824: i = 1; the first prime above each multiple of 10^8 is never processed).
 * range = 0 .. gecm_stage1_ranges(B1) - 1, in order, on the points the previous range left on the device;
 * asynchronous like gecm_stage1.  While the device runs range r the library compiles the tape of range r + 1 on a
 * helper thread.  B1 <= 10^12. */
int gecm_stage1_ranges(uint64_t B1);                   /* ceil(B1 / 10^8), at least 1 */
int gecm_stage1_range(gecm_ctx *ctx, uint64_t B1, uint32_t range);
/* What vececm prints and decides around one range (ecm.c:1215-1247, 1849): the sieved interval [lo, hi] with
 * hi = min(B2 + 1000, lo + 10^8) and its prime count ("Found %lu primes in range [lo : hi]"), P_MIN ("Commencing
 * Stage 1 @ prime"), the last prime the call processes ("Stage 1 completed at prime", the B1 field of the
 * checkpoint lines), and whether the reference writes checkpoint.txt after this range: it does when the range
 * holds no prime >= B1 (ecm.c:1237 reads PRIMES[last_pid] one past the list, a zero word of the fresh
 * allocation) — every range but the last, and also the last (or only) one when B1 lies above its last prime.   */
typedef struct {
    uint64_t lo, hi, nprimes, first_prime, last_prime;
    int checkpoint;
} gecm_stage1_range_desc;
int gecm_stage1_describe_range(uint64_t B1, uint64_t B2, uint32_t range, gecm_stage1_range_desc *out);
/* How stage 1 maps curves to lanes.  1 = one curve per lane (64 per wavefront): the throughput layout,
 * full speed from 2 wavefronts per SIMD, i.e. 128 x (4 x CUs) = 131072 curves on MI355X.  2 = the X and
 * the Z coordinate of a curve on two adjacent lanes (32 curves per wavefront): each point operation's
 * independent halves (ecm.c:417-440, 447-454) run side by side, so a curve finishes in half the time
 * and a batch fills the chip at half the size (1.83x the curves/s up to 32768 curves on MI355X).
 * 8 = X and Z on two adjacent quads of lanes and the limbs of each residue spread over the four lanes of
 * its quad (8 curves per wavefront), with a row-wise Montgomery multiply whose digit and operand limbs are
 * broadcast inside the quad: another 1.5x (416-bit) to 2.4x (1024-bit) for batches up to 8192 curves.
 * 0 (default) = chosen per launch from the batch size, the limb count and the CU count
 * (gecm_dev_auto_lanes).  Results are identical in every layout.
 * gecm_get_lanes_per_curve returns what the last gecm_stage1 launch used (0 before the first). */
int gecm_set_lanes_per_curve(gecm_ctx *ctx, int lanes);
/* N | 2^k - 1, N | 2^k + 1 (Cunningham cofactors) or N | 2^k - c with c odd and below one reference limb (pseudo-
 * Mersenne inputs); the reference's isMersenne == +1 / -1 / c, main.c:410-441, for which it switches to
 * vecmulmod52_mersenne: stage 1 runs modulo 2^k -/+ 1 or 2^k - c with a multiply whose reduction
 * half needs almost no multiplications, and X, Z are reduced modulo N when they come back.  Chosen at
 * gecm_create when it is the cheaper multiply; outputs are the same residues modulo N either way.
 * gecm_set_special_form(ctx, 0) keeps everything on the generic REDC path (takes effect at the next
 * gecm_build_curves / gecm_upload_points).  A batch small enough for the eight-lane layout runs there, on
 * generic REDC, which is faster still.  gecm_get_special_form returns 0 if the special multiply is off or not
 * available, 1 if it is enabled, 2 if the last gecm_stage1 launch actually used it, and stores +k for
 * 2^k - 1 and 2^k - c (c: gecm_prepare_input's info.c), -k for 2^k + 1, and the limb count of that modulus (0, 0 if N
 * has no such form or it would not pay). */
int gecm_set_special_form(gecm_ctx *ctx, int on);
int gecm_get_special_form(const gecm_ctx *ctx, int *k, int *limbs);
int gecm_get_lanes_per_curve(const gecm_ctx *ctx);
/* Progress of the stage-1 call in flight: a long op tape (200 MB for a 1e8 prime range) runs as several kernel launches,
 * cut between two prac() calls; *done of *total have finished.  Callable from the launching thread between
 * gecm_stage1 / gecm_stage1_range and gecm_sync (the reference prints "accumulating prime" every 8192 primes). */
int gecm_stage1_progress(const gecm_ctx *ctx, uint32_t *done, uint32_t *total);
/* the stage-1 kernel the last launch ran, by the name rocprofv3 prints for it ("k_stage1_row<1, 16, false>", "k_stage1<15>"):
 * what a profile of the run has to be matched against */
int gecm_last_kernel_name(const gecm_ctx *ctx, char *buf, size_t len);
/* milliseconds of the last stage-1 kernel, from HIP events on the context's stream */
double gecm_last_kernel_ms(const gecm_ctx *ctx);

typedef struct {
    uint64_t ptadds, ptdups;   /* ecm.c:441, 455; printed at ecm.c:1849-1850: summed over the ranges run so far */
    uint64_t last_prime;       /* ecm.c:1849: of the last range run */
    uint64_t tape_len;         /* of the last range run */
} gecm_stage1_stats;
int gecm_get_stage1_stats(const gecm_ctx *ctx, gecm_stage1_stats *st);

/* P after stage 1 as vec operands (reference layout, Montgomery radix, canonical). */
int gecm_download_points(gecm_ctx *ctx, void *X, void *Z);
/* The de-Montgomeryised X*1, Z*1 the reference writes to save_b1.txt (ecm.c:1327-1331). */
int gecm_download_points_plain(gecm_ctx *ctx, void *x, void *z);

/* ---- save / factor path (ecm.c:1319-1388, check_factor ecm.c:2542-2557) --------------------
 * Formats curve k's resume line exactly as ecm.c:1372-1380:
 *   "METHOD=ECM; SIGMA=%lu; B1=%lu; N=0x%Zx; X=0x%Zx; Z=0x%Zx; PROGRAM=AVX-ECM;\n"
 * from the last downloaded stage-1 result.  Returns the line length, or < 0.                  */
int gecm_format_save_line(gecm_ctx *ctx, size_t k, char *buf, size_t buflen);
/* The same line with another B1 field: the checkpoint.txt lines of ecm.c:1295-1305 carry the last prime of the
 * range just finished (PRIMES[last_pid - 1]) instead of B1.                                              */
int gecm_format_resume_line(gecm_ctx *ctx, size_t k, uint64_t b1_field, char *buf, size_t buflen);
/* gcd(Z_k, N) after stage 1 (ecm.c:1336-1344): returns 1 and the factor as a decimal string if
 * 1 < g < N, else 0 (g == N is "no factor", ecm.c:2549-2553).                                 */
int gecm_stage1_factor(gecm_ctx *ctx, size_t k, char *dec, size_t declen, int *is_prp);

/* Whole-batch factor scan on the device (the reference scans lane by lane on the host,
 * ecm.c:1323-1370, 1485-1528): stage = 1 checks gcd(Z_k, N) after stage 1, stage = 2 checks
 * gcd(acc_k, N) after stage 2, for every curve at once.  Returns the number of curves with a factor
 * (>= 0) and, if first != NULL, the lowest such curve index (or batch if none).  The per-curve
 * functions above/below then format the factors of the flagged curves.                          */
int gecm_scan_factors(gecm_ctx *ctx, int stage, size_t *first);
/* 1 if curve k was flagged by the last gecm_scan_factors call of that stage, else 0 */
int gecm_curve_flag(const gecm_ctx *ctx, int stage, size_t k);

/* ---- L1 phase 2: stage-2 init (ecm_stage2_init, ecm.c:2201-2340) --------------------------
 * Q = the stage-1 result resident on the device.  Builds the baby-step table Pb[map[j]] = [j]Q for
 * j <= U*D with gcd(j, D) = 1 (X/Z-normalised by batch inversion, ecm.c:2322), Pd = [D]Q and
 * acc = one.  D = 0 picks the reference's wheel for the current B1 (main.c:838-872); U = 0 picks 16
 * (the value every reference run chose through its uninitialised `paircost`, main.c:912, 943).
 * Asynchronous; gecm_sync waits.                                                                */
int gecm_stage2_init(gecm_ctx *ctx, uint32_t D, uint32_t U);

/* ---- host pair map (pair, ecm.c:2559-2910) --------------------------------------------------
 * Montgomery's PAIR over the primes in [B1, B2) for wheel D and table height U.  Arrays are
 * malloc'ed; release with gecm_pairmap_release.  (0,0) entries mean "advance the window".       */
typedef struct {
    uint32_t *pairmap_v, *pairmap_u;   /* ecm.c:2559 */
    uint32_t steps;                    /* return value of pair() */
    uint32_t amin;                     /* work->amin set at ecm.c:2571 */
    uint32_t pairs, primes;            /* printed at ecm.c:2904-2905 */
} gecm_pairs;
int gecm_pair_primes(gecm_pairs *out, uint64_t B1, uint64_t B2, uint32_t D, uint32_t U);
void gecm_pairmap_release(gecm_pairs *p);

/* ---- L1 phase 3: stage-2 pair (ecm_stage2_pair, ecm.c:2342-2540) ----------------------------
 * One B2 range: giant steps from A = 2*amin*D, window of 2L = 4U steps, walk of the pair map,
 * acc <- acc * (Xa/Za - Xb/Zb) per pair (CROSS_PRODUCT_INV, ecm.c:1857-1859).  Same arguments as the
 * reference (pairmap_steps, pairmap_v, pairmap_u, work->amin).  Asynchronous.                   */
int gecm_stage2_pair(gecm_ctx *ctx, uint32_t steps, const uint32_t *pairmap_v, const uint32_t *pairmap_u,
                     uint32_t amin);
/* Optional: the host-side preparation gecm_stage2_pair makes for a pair map (its launch tape) ahead of time, e.g.
 * while the device runs stage 1; D, U as for gecm_stage2_init (explicit, not 0).  The reference has no counterpart
 * (its ecm_stage2_pair walks the map directly, ecm.c:2448-2533).  gecm_stage2_pair keeps the tape of the last map it
 * saw either way and recognises the map (its length, amin, D, U and two independent hashes of its words), so a run of
 * many batches prepares it once.  Called with a (D, U) other than the one of the last gecm_stage2_init it replaces the
 * context's stage-2 plan: results of a finished stage 2 (accumulator, factors) must have been read before.  The same
 * holds for gecm_stage2_prepare below. */
int gecm_stage2_pair_prepare(gecm_ctx *ctx, uint32_t D, uint32_t U, uint32_t steps, const uint32_t *pairmap_v,
                             const uint32_t *pairmap_u, uint32_t amin);

/* Convenience: the whole stage-2 sequence of vececm (ecm.c:1401-1476) for primes in [B1, B2):
 * init, then pair + stage2_pair per range of 1e8.  Synchronous.                                  */
int gecm_stage2(gecm_ctx *ctx, uint64_t B2, uint32_t D, uint32_t U);
/* Optional: make (and keep) the pair map gecm_stage2(ctx, B2, D, U) will need, e.g. between gecm_stage1 and
 * gecm_sync, while the device runs stage 1 (the reference computes it between the stages, on the main thread:
 * ecm.c:1441-1443).  Also kept after a gecm_stage2 call, so a run of many batches computes it once. */
int gecm_stage2_prepare(gecm_ctx *ctx, uint64_t B2, uint32_t D, uint32_t U);

typedef struct {
    uint64_t ptadds, numinv, paired;   /* the reference's counters, ecm.c:1482-1483 (numinv as the
                                          reference counts it; the device normalises the baby-step
                                          table in blocks, see stage2_device_inversions) */
    uint64_t device_inversions;
    uint32_t D, U, L, amin_last;
} gecm_stage2_stats;
int gecm_get_stage2_stats(const gecm_ctx *ctx, gecm_stage2_stats *st);

/* ---- sub-sequences per curve in stage 2 ----------------------------------------
 * The baby-step table and the giant steps are one dependent chain per curve.  A batch too small to fill the chip
 * splits each chain into K interleaved sub-sequences (K times the wavefronts for those two phases; the pair walk is
 * not touched).  The accumulators are bit for bit those of K = 1.  Where an inversion of stage 2 meets a factor, the
 * factor reported for a curve may be a proper divisor of the one K = 1 reports (a modulus made of many small primes).
 * gecm_set_stage2_subseq: GECM_S2_SUBSEQ_DEFAULT keeps what the library always did: K by batch size on a single-N
 *   context (two wavefronts per SIMD; the GECM_S2_SUBSEQ environment knob overrides), K = 1 on a multi-modulus one.
 *   GECM_S2_SUBSEQ_AUTO applies the batch-size rule on every kind of context, counted over the batch's padded
 *   positions.  1, 2, 4, 8, 16 or 32 is that K on any context.  Takes effect at the next gecm_stage2_init, gecm_stage2
 *   or gecm_stage2_prepare; gecm_batch_bytes counts the scratch of the K the setting gives.  GECM_ERR_ARG for any
 *   other value or a NULL context.
 * gecm_get_stage2_subseq: the K the last gecm_stage2_init used, 0 before the first; *k_chunks (may be NULL) = the
 *   giant-step chunks generated with sub-sequences since that init (the last chunk of a range, and every chunk of a
 *   range that starts at the origin, are plain chains at any K).  GECM_ERR_ARG for a NULL context. */
#define GECM_S2_SUBSEQ_DEFAULT 0    /* single-N: by batch size; multi-modulus: 1 */
#define GECM_S2_SUBSEQ_AUTO   (-1)  /* by batch size on every kind of context */
int gecm_set_stage2_subseq(gecm_ctx *ctx, int k);
int gecm_get_stage2_subseq(const gecm_ctx *ctx, uint32_t *k_chunks);

/* stg2acc as a vec operand (reference layout, Montgomery radix, canonical), ecm.c:1489 */
int gecm_download_acc(gecm_ctx *ctx, void *acc);
/* Factor check after stage 2 (ecm.c:1485-1528): gcd(acc_k, N), or — when a batch inversion met a
 * non-invertible product (ecm.c:1927-1939) — the gcd recorded then.  Returns 1 and the decimal
 * factor if 1 < g < N, else 0.                                                                  */
int gecm_stage2_factor(gecm_ctx *ctx, size_t k, char *dec, size_t declen, int *is_prp);

/* ---- multi-modulus batches --------------------------------------------------
 * One context for curves on many numbers at once: the way to pretest a list of composites (aliquot or Cunningham
 * cofactors, NFS leftovers) with a few thousand curves each without leaving most of the chip idle.
 * gecm_create_multi: count numbers (decimal or 0x-hex; each odd, > 1 and within the size cap of gecm_create).  The
 *   device limb count is the one the largest needs; each number gets its own constants at that count.
 * gecm_build_curves_multi: curve i has sigma[i] on number modulus_index[i] (< count), in any order.  The library
 *   groups the curves by number and pads each group to whole wavefronts of 64 curves: padding lanes are computed and
 *   dropped, so a list with 8 curves per number runs at 1/8 of the chip's throughput (gecm_batch_bytes counts the
 *   padding, at most 63 curves per number) — unless the context is lane-packed: gecm_set_multi_packing below,
 *   DESIGN.md §16.  Returns 1 like gecm_build_curves when a denominator was not invertible.
 * Curve indices k of every per-curve call are the caller's i.  These work per curve against that curve's number,
 * exactly as they do on a single-N context of it: gecm_stage1, gecm_stage1_range, gecm_sync, gecm_stage2*,
 * gecm_format_save_line, gecm_format_resume_line, gecm_stage1_factor, gecm_stage2_factor, gecm_scan_factors (*first:
 * the lowest flagged caller index), gecm_curve_flag.  Stage 1 runs with 1 or 2 lanes per curve (0 = chosen by batch
 * size as for one number), stage 2 with one sub-sequence per curve unless gecm_set_stage2_subseq asks for more.
 * GECM_ERR_STATE on a multi-modulus context: the L0 operators (gecm_vecinvmod among them), gecm_get_one,
 * gecm_upload_points (given points go in through gecm_resume_points_multi), gecm_download_points, gecm_download_points_plain, gecm_download_acc (the reference radix differs from number to number),
 * gecm_build_curves, gecm_set_special_form, gecm_set_report_modulus; gecm_build_curves_multi on a single-N context.
 * gecm_get_config describes the largest number.                                                                     */
int gecm_create_multi(gecm_ctx **out, int device, const char *const *n_strs, size_t count, int digitbits);
int gecm_build_curves_multi(gecm_ctx *ctx, const uint64_t *sigma, const uint32_t *modulus_index, size_t batch);
/* numbers of the context (1 for a single-N context), and the number curve k runs on */
size_t gecm_moduli(const gecm_ctx *ctx);
int gecm_curve_modulus(const gecm_ctx *ctx, size_t k);
/* the stage-2 accumulator of curve k as the integer gecm_download_acc returns for it on a single-N context of its
 * number (reference Montgomery radix, canonical), in lower-case hex without prefix; returns the digit count */
int gecm_curve_acc(gecm_ctx *ctx, size_t k, char *hex, size_t hexlen);

/* ---- packing of a multi-modulus batch -------------------------------------------
 * GECM_PACK_LANE puts one modulus on every lane instead of one on every wavefront: the numbers' curves lie back to
 * back and only the batch's tail is padded to 64, so a list with 8 curves per number no longer computes 56 padding
 * lanes per number.  For contexts whose largest number has at most 415 bits (15 limbs).  Every per-curve result is the
 * one the default packing and a single-N context of the curve's number give, and the caller's curve indices are
 * unchanged.  Stage 1 runs one lane per curve: a context set to 2 lanes per curve answers gecm_stage1 with
 * GECM_ERR_STATE.  Curves are built on the host: with GECM_BUILD_DEVICE gecm_build_curves_multi and
 * gecm_resume_points_multi answer GECM_ERR_STATE, and the previous batch stays.
 * gecm_set_multi_packing takes effect at the next gecm_build_curves_multi or gecm_resume_points_multi, as
 *   gecm_set_curve_build does; GECM_ERR_ARG for a bad value or a NULL context, GECM_ERR_STATE on a single-N context and
 *   on a multi-modulus context of more than 15 limbs.
 * gecm_get_multi_packing: what the last build used; GECM_PACK_WAVE before the first.
 * gecm_multi_positions: padded curve positions a batch with counts[0..n) curves per number occupies under `packing`
 *   (a multiple of 64); pure host code, the one place the rounding rule lives.
 * gecm_multi_packing_max_bits: the largest number, in bits, a context of that packing takes (415 for GECM_PACK_LANE);
 *   0 = no limit of the packing's own (GECM_PACK_WAVE); GECM_ERR_ARG for a bad value. */
#define GECM_PACK_WAVE 0   /* one modulus per wavefront, each number padded to 64 curves (the default) */
#define GECM_PACK_LANE 1   /* one modulus per lane: numbers back to back, only the batch's tail padded to 64 */
int gecm_set_multi_packing(gecm_ctx *ctx, int packing);
int gecm_get_multi_packing(const gecm_ctx *ctx);
size_t gecm_multi_positions(const size_t *counts, size_t n, int packing);
int gecm_multi_packing_max_bits(int packing);

/* ---- resume: save_b1.txt and checkpoint.txt lines back into a context ------------
 * gecm_parse_resume_line reads one line "METHOD=ECM; SIGMA=...; B1=...; N=...; X=...; Z=...; PROGRAM=...;" — ours
 * (ecm.c:1295-1305, 1372-1380) or one of a GMP-ECM -save file: fields in any order, unknown fields (CHECKSUM, PROGRAM,
 * WHO, TIME, X0, Y0, Y, COMMENT, ...) ignored, numbers decimal or 0x-hex, Z absent = 1, PARAM absent or 0 (GMP-ECM's
 * PARAM 0 is the Suyama sigma of the reference), CRLF and a missing last ';' accepted.  Pure host code: no context, no
 * allocation; N, X, Z come back as (pointer to the first digit, digit count, base 10 | 16) into the caller's line.
 * Returns GECM_OK, 1 for a line to skip (blank, or starting with '#'), or GECM_ERR_ARG with a text that names the
 * field: METHOD other than ECM, PARAM other than 0, SIGMA, B1, N or X missing, empty or given twice, SIGMA < 6 or beyond 64 bits, an N
 * that is an expression, anything but digits inside a number, a number longer than the library computes with.     */
typedef struct {
    const char *digits;     /* first digit (after "0x" for base 16); NULL: the field was absent (z only: Z = 1) */
    size_t len;
    int base;               /* 10 | 16 */
} gecm_resume_num;
typedef struct {
    uint64_t sigma, b1;     /* the B1 field: B1 of a save line, the last prime of the range done of a checkpoint line */
    gecm_resume_num n, x, z;
} gecm_resume_rec;
int gecm_parse_resume_line(const char *line, gecm_resume_rec *rec);
/* The same with GMP-ECM's PARAM 1 and 3 accepted and returned in *param (PARAM absent: 0).  The SIGMA range follows the
 * parametrisation: >= 6 for PARAM 0, [1, 2^64) for PARAM 1, [1, 2^32) for PARAM 3.  PARAM 2, PARAM >= 4 and a PARAM
 * field given twice are refused with a text naming the field.  gecm_parse_resume_line itself keeps refusing PARAM 1 and 3:
 * a caller that takes such lines says so by calling this one, and hands *param on to gecm_set_next_params. */
int gecm_parse_resume_line_param(const char *line, gecm_resume_rec *rec, int *param);
/* The range a run to B1 goes on with from lines whose B1 field is b1_field.  b1_field == B1: *range =
 * gecm_stage1_ranges(B1), stage 1 is complete (save lines).  Else the r + 1 for which range r of a run to B1 ends at
 * prime b1_field and writes a checkpoint (gecm_stage1_describe_range(B1, B1, r): last_prime, checkpoint); that can be
 * the range count too — the reference also checkpoints a last range whose last prime lies below B1 — and X, Z then are
 * the final residues.  Anything else: GECM_ERR_ARG, "not a checkpoint of a run to B1 = ...".  The B1 field of a
 * checkpoint says nothing else: the reference's stage 1 is not one prime-power product cut at that prime (every range
 * runs the 2-power doublings again and skips its first prime), so lines are resumed by the run that wrote them only. */
int gecm_stage1_resume_range(uint64_t B1, uint64_t b1_field, uint32_t *range);
/* Phase 0 from given points: curve i has sigma[i] and the PLAIN canonical residues x[i], z[i] in [0, N) of a save or
 * checkpoint line, as vec operands of the context's layout (data[lane + limb*batch], NWORDS limbs of DIGITBITS bits; on
 * a multi-modulus context the NWORDS of gecm_get_config, the largest number's) — not in Montgomery form: the device
 * converts.  s = (A+2)/4 is built from sigma exactly as gecm_build_curves / gecm_build_curves_multi build it (same
 * failure records, same return value 1 when a denominator was not invertible, same stale operand).  Checked before the
 * context gives up its previous batch: sigma >= 6, x, z < the curve's N (GECM_ERR_ARG); the _multi form on a single-N
 * context and the other on a multi-modulus one return GECM_ERR_STATE.  A failure after that leaves no batch.
 * b1_done = 0: the context is mid stage 1; the caller goes on with gecm_stage1_range(ctx, B1, r) for the r of
 * gecm_stage1_resume_range, and gecm_stage2* answer "run stage 1 first".  b1_done = B1 > 0: stage 1 is taken as
 * finished at B1 — save lines, factor scan, gecm_stage2_prepare, gecm_stage2_init, gecm_stage2 work as after
 * gecm_stage1(B1).  gecm_get_stage1_stats of a resumed context counts only the ranges run since the resume.
 * A context with a special-form multiply (gecm_set_special_form) keeps it for the remaining ranges.                */
int gecm_resume_points(gecm_ctx *ctx, const uint64_t *sigma, const void *x, const void *z, size_t batch, uint64_t b1_done);
int gecm_resume_points_multi(gecm_ctx *ctx, const uint64_t *sigma, const uint32_t *modulus_index, const void *x,
                             const void *z, size_t batch, uint64_t b1_done);

/* ---- extension to a higher B1: the standard stage-1 multiplier ------------------
 * k_std(B) = the product over the primes p <= B of p^e, e the largest with p^e <= B — the bound inclusive, GMP-ECM's
 * rule; the reference's own multiplier (every prime power BELOW B1, ecm.c:1816, 1832) is k_std(B1 - 1) as long as B1
 * lies within one prime range, so its save lines with B1 <= 10^8 are standard lines of the bound B1 - 1.
 * gecm_stage1_extend takes points that are complete to `from` on to `to`: P <- [k_std(to) / k_std(from)] P.  `from` is
 * the caller's statement about the points in the context, as b1_done is for gecm_resume_points; from = 1 means a fresh
 * build, so gecm_stage1_extend(ctx, 1, B) IS standard stage 1 to B.  1 <= from <= to <= 10^12 (GECM_ERR_ARG), a batch
 * in the context (GECM_ERR_STATE).  The work is cut at the multiples of the prime range (10^8) strictly between the two
 * bounds: segment j is (lo_j, hi_j] with lo_0 = from and the last hi = to, and after every segment the points are
 * complete to hi_j — the context's B1 is hi_j then, so a checkpoint after a segment is an ordinary standard line.
 * gecm_stage1_extend_segment runs one segment (0 .. gecm_stage1_extend_segments - 1, in order), asynchronous like
 * gecm_stage1_range, and compiles the next segment's tape on the helper thread meanwhile; gecm_stage1_extend runs them
 * all and returns after the last launch.  Afterwards save lines, the factor scan and gecm_stage2* work as after
 * gecm_stage1(to); gecm_get_stage1_stats sums over the segments since segment 0.  A segment in which no prime gains a
 * power (from == to among them) launches nothing.  Every layout, the special-form multiply and both packings of a
 * multi-modulus context run extensions as they run gecm_stage1: only the tape differs. */
typedef struct {
    uint64_t lo, hi;        /* the segment (lo, hi] */
    uint64_t nprimes;       /* primes of (lo, hi]: each enters the multiplier here */
    uint64_t power_steps;   /* further prime-power steps: powers beyond the first, of these primes and of smaller ones */
    uint64_t last_prime;    /* the largest prime that gains a power (0: none does) */
} gecm_extend_desc;
int gecm_stage1_extend_segments(uint64_t from, uint64_t to);
int gecm_stage1_describe_extend(uint64_t from, uint64_t to, uint32_t seg, gecm_extend_desc *out);
int gecm_stage1_extend_segment(gecm_ctx *ctx, uint64_t from, uint64_t to, uint32_t seg);
int gecm_stage1_extend(gecm_ctx *ctx, uint64_t from, uint64_t to);
/* Projective (X : Z) depends on the order the primes were processed in; x = X/Z mod N does not, and is the residue any
 * correct program writes for that sigma and bound (GMP-ECM stores it as X= with no Z=).  gecm_normalize_points gives
 * every curve with gcd(Z, N) = 1 X <- X/Z and Z <- 1 on the device, synchronously; a curve whose Z has no inverse keeps
 * its X and Z word for word — it is a stage-1 factor, which gecm_stage1_factor still reports.  Returns GECM_OK, or 1
 * when some curve was left as it was (the convention of gecm_build_curves).  GECM_ERR_STATE without a batch and on a
 * context with a report modulus (gecm_set_report_modulus).  A special-form multiply in use is settled first; the
 * launches after a normalisation run modulo N.  After it gecm_last_kernel_ms is the normalisation kernel's time.
 * gecm_points_normalized: 1 after a normalisation, until the next stage-1 launch, build, upload or resume.
 * gecm_format_save_line_std writes curve k's standard line at the context's B1,
 *   "METHOD=ECM; PARAM=%d; SIGMA=%llu; B1=%llu; N=0x%s; X=0x%s; PROGRAM=AVX-ECM-STD;\n"   (PARAM: gecm_curve_param)
 * (with "X=0x%s; Z=0x%s;" for a curve left as it was); GECM_ERR_STATE if the batch is not normalised.
 * gecm_parse_resume_line reads both shapes.  Returns the line length, or < 0. */
int gecm_normalize_points(gecm_ctx *ctx);
int gecm_points_normalized(const gecm_ctx *ctx);
int gecm_format_save_line_std(gecm_ctx *ctx, size_t k, char *buf, size_t buflen);
/* The standard bound the points of a resume line are complete to: the `from` of gecm_stage1_extend.  PROGRAM exactly
 * "AVX-ECM": the line holds the reference's multiplier, *from = B1 field - 1, provided the field lies within one prime
 * range; above it GECM_ERR_ARG — a reference run over several prime ranges has no standard multiplier.
 * Any other or no PROGRAM (ours with -STD, GMP-ECM's): *from = the B1 field.  Pure host code, no context; returns what
 * gecm_parse_resume_line returns for a line it refuses or skips. */
int gecm_resume_line_std_bound(const char *line, uint64_t *from);
/* the same for a caller that reads its lines with gecm_parse_resume_line_param: PARAM 1 and 3 lines have a bound too */
int gecm_resume_line_std_bound_param(const char *line, uint64_t *from);

/* ---- P-1 and P+1 stage 1: one residue per lane on the stage-1 tape --------------
 * Pretesting a list of composites is P-1, then P+1, then ECM; a method batch holds one residue x per position instead
 * of a curve and runs the standard multiplier on it:
 *   P-1: x <- x0^E mod N, factor test gcd(x - 1, N);
 *   P+1: x <- V_E(x0) mod N (V_0 = 2, V_1 = x0, V_{m+n} = V_m V_n - V_{m-n}), factor test gcd(x - 2, N);
 * E = k_std(to) / k_std(from), exactly what gecm_stage1_extend(ctx, from, to) means for curves; a fresh run is from = 1.
 * The residue does not depend on the chain that computed it, so there is no normalisation step, and going on needs only
 * x: V_a(V_b(P)) = V_ab(P), (x^a)^b = x^ab.  The reference's own multiplier (gecm_stage1, gecm_stage1_range) is not
 * offered.  The special-form twin is not filled: these batches run the generic multiply modulo N.
 * gecm_build_seeds / gecm_build_seeds_multi: x0 and x are plain canonical residues in the context's vec layout, as for
 *   gecm_resume_points.  x == NULL: a fresh batch, x = x0, and b1_done must be 1.  Otherwise x is the residue of a line
 *   complete to b1_done (1 .. 10^12), and x0 may be NULL: the seed is not known, and the lines omit it.  Checked before
 *   the previous batch is given up: method is GECM_METHOD_PM1 or GECM_METHOD_PP1, batch >= 1, every value below its N
 *   (GECM_ERR_ARG); the _multi form on a single-N context and the reverse, and a context with a report modulus, answer
 *   GECM_ERR_STATE.  x0 = 0, and for P+1 also x0 = 2 and x0 = N - 2, are degenerate but legal: they are computed like
 *   any other seed and find nothing (as is P-1 with x0 = 1).  Both packings of a multi-modulus context work; lane packing
 *   keeps its 415-bit limit.  A pending gecm_set_next_params setting is taken and dropped: it does not apply to seeds.
 * On a method batch work: gecm_stage1_extend, gecm_stage1_extend_segment, gecm_sync, gecm_stage1_progress,
 *   gecm_last_kernel_ms, gecm_last_kernel_name (k_unit, k_unit_multi, k_unit_lane), gecm_get_stage1_stats (ptadds and
 *   ptdups count tape events as they do for curves), gecm_scan_factors(ctx, 1, ..) and gecm_curve_flag(ctx, 1, k) (of
 *   x - 1 or x - 2), gecm_stage1_factor (g = N is "no factor"), gecm_download_points_plain on a single-N context (x, and
 *   z = 1), gecm_curve_modulus, and gecm_format_save_line_std, which writes
 *     "METHOD=P-1; B1=%llu; N=0x%s; X=0x%s; X0=0x%s; PROGRAM=AVX-ECM-STD;\n"   (METHOD=P+1 likewise)
 *   with "X0=0x%s; " left out when the seed is unknown.  One lane per residue whatever gecm_set_lanes_per_curve says;
 *   gecm_get_lanes_per_curve answers 1 after such a launch.
 * GECM_ERR_STATE with a text naming the method: gecm_stage1, gecm_stage1_range, every gecm_stage2* call,
 *   gecm_normalize_points, gecm_download_s, gecm_format_save_line, gecm_format_resume_line, gecm_scan_factors(ctx, 2, ..)
 *   (the stage-2 ones unless gecm_set_method_stage2 opted the context in, below).
 * Any of the build, upload or resume calls for curves makes the context an ECM context again.
 * gecm_batch_method: the method of the batch in the context; GECM_METHOD_ECM for every batch built for curves, and
 *   without a batch.
 * gecm_curve_seed: x0 of the caller's position k, lower-case hex without prefix; returns the digit count, 0 (and an empty
 *   string) if the seed is unknown, GECM_ERR_ARG for no such position, GECM_ERR_STATE on an ECM batch.
 * gecm_parse_resume_line_method: gecm_parse_resume_line_param with METHOD=P-1 and METHOD=P+1 accepted (*method = 1, 2).
 *   On such a line SIGMA and PARAM need not be present and are ignored when they are (rec->sigma = 0, *param = 0), X0 is
 *   returned in *x0 when present (digits NULL otherwise), Z must be absent or 1.  For METHOD=ECM and for lines without
 *   METHOD it returns exactly what gecm_parse_resume_line_param returns, *method = 0, and no x0.  The two older parsers
 *   and bound functions keep refusing other methods.
 * gecm_resume_line_std_bound_method: the B1 field of a P-1 / P+1 line (such lines are always standard); for ECM lines
 *   what gecm_resume_line_std_bound_param returns. */
#define GECM_METHOD_ECM 0
#define GECM_METHOD_PM1 1
#define GECM_METHOD_PP1 2
int gecm_build_seeds(gecm_ctx *ctx, int method, const void *x0, const void *x, size_t batch, uint64_t b1_done);
int gecm_build_seeds_multi(gecm_ctx *ctx, int method, const uint32_t *modulus_index, const void *x0, const void *x,
                           size_t batch, uint64_t b1_done);
int gecm_batch_method(const gecm_ctx *ctx);
int gecm_curve_seed(gecm_ctx *ctx, size_t k, char *hex, size_t hexlen);
int gecm_parse_resume_line_method(const char *line, gecm_resume_rec *rec, int *param, int *method, gecm_resume_num *x0);
int gecm_resume_line_std_bound_method(const char *line, uint64_t *from);

/* ---- P-1 and P+1 stage 2: the pair walk on values of a Lucas sequence ----------
 * With x the stage-1 residue of a position, let P = x for P+1 and P = x + 1/x mod N for P-1.  Then V_n(P) = x^n + x^-n
 * (V_0 = 2, V_1 = P, V_{m+n} = V_m V_n - V_{m-n}, V_{-n} = V_n), and V_a - V_u = 0 modulo a prime p whenever a = +-u
 * modulo the order stage 1 left: one stage 2 serves both methods and finds every p with p -+ 1 = (B1-smooth) * (one
 * prime below B2).  For a pair map of wheel D and height U, walked in order with run_amin starting at amin and growing
 * by U at every (0,0) entry, every other entry (v, u) contributes the factor
 *     V_{(run_amin + v) D}(P) - V_u(P)  mod N,
 * and the accumulator of a position is the product of those factors over every map given since gecm_stage2_init, as a
 * plain residue; gecm_download_acc and gecm_curve_acc return it in the reference's Montgomery radix, as for curves.
 * gecm_set_method_stage2(ctx, GECM_METHOD_S2_ON) opts a context in (GECM_ERR_ARG: another value, NULL ctx);
 *   gecm_get_method_stage2 reads the setting (GECM_METHOD_S2_OFF for NULL).  It holds across builds and changes nothing
 *   on a batch of curves.  Off, the default, every call answers what it answered before the setting existed.
 * On, with a method batch whose stage 1 is complete to some B1, these work as on a batch of curves: gecm_stage2_init,
 *   gecm_stage2_pair, gecm_stage2_pair_prepare, gecm_stage2_prepare, gecm_stage2, gecm_get_stage2_stats,
 *   gecm_set_stage2_subseq / gecm_get_stage2_subseq, gecm_download_acc (single-N), gecm_curve_acc, gecm_stage2_factor,
 *   gecm_scan_factors(ctx, 2, ..) (the plain scan of the accumulator) and gecm_curve_flag(ctx, 2, k).  The other
 *   refusals of a method batch stay.
 * Stage 2 leaves the residues alone (P goes to the batch's S array, which a method batch does not use): afterwards
 *   gecm_format_save_line_std writes the same lines, gecm_stage1_extend goes on from the same residues, and another
 *   stage 2 with other (D, U) starts clean.
 * gecm_get_stage2_stats: D, U, L, amin_last, paired, ptadds, numinv are the plan's host-side counters, as for curves
 *   (what the reference would count for a curve on the same maps); device_inversions is 1 for P-1 (x^-1) and 0 for P+1.
 * P-1 where gcd(x, N) > 1: the position's failure record receives that gcd, as a failed batch inversion does for a curve:
 *   gecm_stage2_factor reports it, gecm_scan_factors(ctx, 2, ..) flags the position, its accumulator is unspecified.
 * gecm_batch_bytes counts a method batch as it counts curves: an upper bound (no block scratch is used). */
#define GECM_METHOD_S2_OFF 0
#define GECM_METHOD_S2_ON  1
int gecm_set_method_stage2(gecm_ctx *ctx, int on);
int gecm_get_method_stage2(const gecm_ctx *ctx);

/* ---- P-1 and P+1 stage 1 with a residue per 16-lane DPP row, for small batches ----
 * A method batch holds one residue per number, so its one-lane launch is a wavefront or two on a chip of a thousand
 * SIMDs.  With 16 lanes per residue the limbs of a residue lie over the 16 lanes of a DPP row, four residues per
 * wavefront, and a multiply is the row-wise one of the 32-lane curve layout (kernel k_unit_row<NQ, ROWS>).
 * gecm_set_method_lanes(ctx, lanes): 1 (the default), 16 or GECM_METHOD_LANES_AUTO; GECM_ERR_ARG for another value or a
 *   NULL context.  gecm_get_method_lanes reads the setting (1 for NULL).  It holds across builds, changes nothing on a
 *   batch of curves (gecm_set_lanes_per_curve keeps having no say over method batches) and takes effect at the next
 *   gecm_stage1_extend or gecm_stage1_extend_segment of a method batch.  With 1 every call answers what it answered
 *   before the setting existed, kernel names and gecm_get_lanes_per_curve() == 1 included.
 * With 16 those calls run k_unit_row, on single-N contexts and on multi-modulus contexts of both packings (lane packing
 *   keeps its 415-bit limit on the context; the row kernel has none of its own): gecm_get_lanes_per_curve answers 16,
 *   gecm_last_kernel_name "k_unit_row<..>".  Every residue is the integer the one-lane kernel gives; progress,
 *   gecm_last_kernel_ms, stats, scan, factors, save lines, gecm_download_points_plain and stage 2 after it
 *   (gecm_set_method_stage2) are unchanged in meaning.  If the kernel's constants cannot be set up for the context's
 *   numbers the launch answers GECM_ERR_STATE with a text, and the batch is as it was.
 * With GECM_METHOD_LANES_AUTO a launch takes gecm_method_lanes_auto(padded positions, device limbs, compute units), and
 *   1 where 16 cannot be set up.
 * gecm_method_lanes_auto: 1 or 16 for a batch of that many positions (padding included: gecm_multi_positions) on a
 *   context of dev_limbs limbs and a device of cus compute units; pure host code, the one place the rule lives. */
#define GECM_METHOD_LANES_AUTO (-1)
int gecm_set_method_lanes(gecm_ctx *ctx, int lanes);   /* 1 (default), 16, GECM_METHOD_LANES_AUTO */
int gecm_get_method_lanes(const gecm_ctx *ctx);
int gecm_method_lanes_auto(size_t positions, int dev_limbs, int cus);   /* 1 or 16; pure host code */

/* ---- curve batches of a multi-modulus context with 32 lanes per curve, for small batches ----
 * A multi-modulus batch is small by construction, and gecm_set_lanes_per_curve gives it 1 or 2 lanes per curve.  With
 * rows on, stage 1 of its curves runs in the layout small single-N batches run in: X and Z of a curve on two DPP rows,
 * the limbs of a residue over the 16 lanes of a row (kernel k_stage1_row_multi<NQ, ROWS>), every curve with the
 * constants of its own number.
 * gecm_set_multi_rows(ctx, rows): GECM_MULTI_ROWS_OFF (the default), _ON or _AUTO; GECM_ERR_ARG for another value or a
 *   NULL context, GECM_ERR_STATE on a single-N context.  gecm_get_multi_rows reads the setting (OFF for NULL).  It holds
 *   across builds and takes effect at the next gecm_stage1, gecm_stage1_range, gecm_stage1_extend or
 *   gecm_stage1_extend_segment of a batch of curves; method batches are not touched (gecm_set_method_lanes).  It applies
 *   only while gecm_set_lanes_per_curve is 0: an explicit 1 or 2 runs what it runs without the setting, lane packing's
 *   refusal of 2 included.  With OFF every call answers what it answered before the setting existed.
 * With ON those launches run k_stage1_row_multi on both packings (lane packing keeps its 415-bit limit on the context):
 *   gecm_get_lanes_per_curve answers 32, gecm_last_kernel_name "k_stage1_row_multi<..>".  Every residue, save and resume
 *   line, flag, factor, failure record, statistic and stage-2 result is the one OFF gives.  If the kernel's constants
 *   cannot be set up for one of the context's numbers the launch answers GECM_ERR_STATE with a text, and the batch is as
 *   it was.
 * With AUTO a launch runs rows where gecm_multi_rows_auto(padded positions, device limbs, compute units) says 1 and the
 *   constants exist, and what OFF runs otherwise.
 * gecm_multi_rows_auto: 0 or 1 for a batch of that many positions (padding included: gecm_multi_positions) on a context
 *   of dev_limbs limbs and a device of cus compute units; pure host code, the one place the rule lives. */
#define GECM_MULTI_ROWS_OFF 0
#define GECM_MULTI_ROWS_ON 1
#define GECM_MULTI_ROWS_AUTO (-1)
int gecm_set_multi_rows(gecm_ctx *ctx, int rows);
int gecm_get_multi_rows(const gecm_ctx *ctx);
int gecm_multi_rows_auto(size_t positions, int dev_limbs, int cus);   /* 0 or 1; pure host code */

/* ---- wide contexts: stage 1 for numbers of 1032 to 1311 bits ----
 * gecm_create and gecm_create_multi serve numbers of up to 1031 bits.  gecm_create_wide serves those too — for an N
 * gecm_create takes it returns what gecm_create returns, an ordinary context (gecm_is_wide == 0), so a caller may use it
 * for every number — and for bitlen(N) from 1032 to gecm_wide_max_bits() = 1311 it makes a WIDE context: 40, 43 or 47
 * device limbs (the smallest with 28 limbs >= bits + 5), the 32-lane stage-1 kernel k_stage1_row<3, limbs + 1, false> and
 * no other kernel.  Above 1311 bits: GECM_ERR_ARG, "larger than this build supports".
 * A wide context builds curves, runs stage 1 and hands out the result; the device does stage 1, the host the rest:
 *   gecm_get_config (the reference's NWORDS/MAXBITS rule, dev_limbs 40, 43 or 47), gecm_device_name, gecm_device_memory,
 *   gecm_batch_bytes (the stage-1 arrays; 0 with with_stage2), gecm_set_report_modulus;
 *   gecm_build_curves on the host, with gecm_set_next_params for PARAM 0, 1 and 3;
 *   gecm_stage1, gecm_stage1_range, gecm_sync, gecm_stage1_progress, gecm_last_kernel_name, gecm_last_kernel_ms,
 *   gecm_get_stage1_stats; gecm_set_lanes_per_curve 0 and 32 run, with 1, 2 or 8 gecm_stage1 answers GECM_ERR_STATE;
 *   gecm_get_lanes_per_curve answers 32, gecm_get_special_form 0 (no twin is opened);
 *   gecm_download_points_plain, gecm_format_save_line, gecm_format_resume_line, gecm_stage1_factor,
 *   gecm_scan_factors(ctx, 1, ..) and gecm_curve_flag(ctx, 1, k), with the meaning they have on any context: the host
 *   reduces the kernel's lazy residues modulo N, takes them out of Montgomery form and computes gcd(Z, N) per curve.
 * Everything else answers GECM_ERR_STATE, "not available on a wide context (gecm_create_wide): ...", and leaves the
 * batch as it was: every gecm_stage2* call, gecm_scan_factors(ctx, 2, ..), gecm_download_acc, gecm_curve_acc; the L0
 * operators, gecm_vecinvmod, gecm_vecrawop, gecm_get_one; gecm_upload_points, gecm_download_points, gecm_download_s;
 * gecm_resume_points; gecm_stage1_extend*, gecm_normalize_points, gecm_format_save_line_std; gecm_build_seeds; and
 * gecm_build_curves while gecm_set_curve_build is GECM_BUILD_DEVICE.  The save lines are what GMP-ECM resumes for stage 2.
 * gecm_is_wide: 1 for a wide context, 0 for any other and for NULL.  gecm_wide_max_bits: 1311; pure host code. */
int gecm_create_wide(gecm_ctx **out, int device, const char *n_str, int digitbits);
int gecm_is_wide(const gecm_ctx *ctx);
int gecm_wide_max_bits(void);

#ifdef __cplusplus
}
#endif
#endif
