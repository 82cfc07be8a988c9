/* gecm_launch.h — the kernel launchers of one limb count (gecm_kernels.hip, two objects per GECM_NL), reached through
 * one table of function pointers per object, and the stage-2 kernel arguments they pass on. */
#ifndef GECM_LAUNCH_H
#define GECM_LAUNCH_H
#include <stddef.h>
#include <stdint.h>
#include "gecm_ops.h"

/* limb counts built into the library; keep in sync with the Makefile's NLS */
#ifdef GECM_DEV_NL15
#define GECM_NL_LIST(X) X(15)      /* `make DEV=1`: quick developer build, 416-bit class only */
#else
#define GECM_NL_LIST(X) X(8) X(10) X(12) X(14) X(15) X(17) X(19) X(21) X(23) X(26) X(28) X(30) X(32) X(34) X(37)
#endif

/* Where the kernels of a launch find the constants of their modulus.  The device layer says it (modconst() in
 * gecm_dev.hip); the launchers pick the kernel by it in one place (launch_by_source in gecm_kernels.hip). */
enum gecm_source {
    GECM_SRC_VALUE = 0, /* single modulus: the record m below, passed as kernel arguments */
    GECM_SRC_WAVE,      /* one modulus per 64-curve block: groups and block_group, the _multi kernels */
    GECM_SRC_LANE       /* one modulus per curve position: groups and curve_group, the _lane kernels of
                         * stage1 (one lane per curve), from_mont, to_mont, gcd_scan, normalize, s2_init and s2_pair
                         * (limb counts with gecm_kernels_p1::has_lane) */
};

/* the constants of a launch: the context's own modulus, and where the kernels are to take theirs from */
typedef struct {
    gecm_devmod m;               /* host memory; m.r3 NULL on a context that never inverts */
    const void *groups;          /* WAVE, LANE: device array of the moduli's constants (pack_group), else NULL */
    const uint32_t *block_group; /* WAVE: the modulus of every 64-curve block (device array), else NULL */
    const uint32_t *curve_group; /* LANE: the modulus of every curve position (device array), else NULL */
    enum gecm_source source;
} gecm_modconst;

/* Stage-2 kernel arguments (csrc/gecm_stage2.hpp), passed by value: the type names are part of the kernel symbols. */
struct S2InitArgs {
    const uint32_t *X, *Z, *S;       // Q = P after stage 1 (Montgomery form), s = (A+2)/4
    uint32_t *PbX;                   // out: normalised baby steps, entries 0..npb-1 (0 unused)
    uint32_t *bx, *bz, *bp;          // block scratch, S2_BLK entries each
    uint32_t *PdX, *PdZ;             // out: Pd = [D]Q
    uint32_t *acc;                   // out: accumulator = one
    uint32_t *fail;                  // per-curve gcd record of a failed inversion (zeroed by host)
    const uint32_t *keep;            // bitmap over j: bit j set iff map[j] > 0
    uint32_t umax, D, npb;
    size_t stride;
    // K sub-sequences per curve (small batches, s2_init_k): table index of the i-th kept member of sub-sequence r
    // at tgt[tgt_off[r] + i]; block scratch kbx/kbz/kbp per (curve block, r); PdK = [K*D]Q for the giant steps
    uint32_t K;
    const uint32_t *tgt, *tgt_off;
    uint32_t *kbx, *kbz, *kbp;
    uint32_t *PdKX, *PdKZ;
};

struct S2PairArgs {
    const uint32_t *X, *Z, *S;       // Q, s
    const uint32_t *PbX;             // normalised baby steps
    uint32_t npb;
    const uint32_t *PdX, *PdZ;       // Pd = [D]Q
    uint32_t *gx, *gz;               // chunk scratch: X, Z of the giant steps being generated, G+2 entries
                                     // (entries 0,1 = the last two steps of the previous chunk)
    uint32_t *gp;                    // prefix products, G entries
    uint32_t *ring;                  // X/Z of the giant steps, ring of `ring_size` entries (power of two)
    uint32_t *acc;                   // in/out accumulator
    uint32_t *fail;
    const uint32_t *steps;           // pair tape, 2 words per step (see S2_STEP_GEN)
    uint32_t nsteps, D, G, ring_size;
    uint64_t A0;                     // multiplier of the first giant step: 2*amin*D   ecm.c:2378
    size_t stride;
    // K sub-sequences per curve (giant_chunk_k): scratch per (curve block, r) with Gs + 2 / Gs entries, the stride
    // point [K*D]Q, and one failure plane per sub-sequence after plane 0
    uint32_t K, Gs;
    uint32_t *kgx, *kgz, *kgp;
    const uint32_t *PdKX, *PdKZ;
};

/* what the stage-2 launchers need besides the kernel arguments */
struct gecm_s2_init_launch {
    S2InitArgs a;
    uint32_t slices;              /* accumulators per curve: with more than one, the launcher also sets them to one */
};

struct gecm_s2_pair_launch {
    S2PairArgs a;
    const uint32_t *host_steps;   /* host copy of the tape: the launcher splits it at the "generate" marks */
    uint32_t slices;              /* accumulators per curve: each run of pairs is cut into this many slices */
    uint32_t *k_chunks;           /* out (may be NULL): one more for every chunk launched with K sub-sequences per curve */
};

/* Part 1: stage 1, canonical form, de-Montgomeryisation, L0 operators, factor scan, curve construction. */
struct gecm_kernels_p1 {
    /* lanes per curve 1 or 2 (form: 0 = generic modulus, +1 = 2^k - 1, -1 = 2^k + 1, 2 = 2^k - c), or 8 (generic
     * moduli only; modq = device array of 80 words: limbs 0..39 of N then of K', zero padded, read per lane).  The
     * eight-lane kernel leaves lazy values in X, Z: run canon afterwards. */
    /* a multi-modulus mc takes lanes 1 or 2 and form 0 only */
    void (*stage1)(void *stream, const gecm_modconst *mc, const uint32_t *tape, uint32_t tape_len, uint32_t *X,
                   uint32_t *Z, const uint32_t *S, size_t stride, const uint32_t *modq, int lanes, int form);
    void (*canon)(void *stream, const gecm_modconst *mc, uint32_t *X, uint32_t *Z, size_t stride);
    void (*from_mont)(void *stream, const gecm_modconst *mc, const uint32_t *X, const uint32_t *Z, uint32_t *ox,
                      uint32_t *oz, size_t stride);
    /* the inverse: canonical plain residues ix, iz in [0, N) -> canonical Montgomery form in X, Z (needs mc->m.r2) */
    void (*to_mont)(void *stream, const gecm_modconst *mc, const uint32_t *ix, const uint32_t *iz, uint32_t *X,
                    uint32_t *Z, size_t stride);
    void (*l0)(void *stream, const gecm_modconst *mc, int op, const uint32_t *A, const uint32_t *B, uint32_t *C,
               uint32_t *D, size_t stride, const uint32_t *fix);
    /* the test-level inversion (single modulus only): C = the inverse of A in the radix `fix` sets, or 0; G = gcd(A, N) */
    void (*l0_inv)(void *stream, const gecm_modconst *mc, const uint32_t *A, uint32_t *C, uint32_t *G, size_t stride,
                   const uint32_t *fix);
    void (*gcd_scan)(void *stream, const gecm_modconst *mc, const uint32_t *V, uint32_t *G, uint32_t *flags,
                     size_t stride);
    /* the Suyama construction on the device: sigma[stride] (64-bit, device memory) -> X, Z, S of the batch, canonical, and
     * flags[curve] = 1 where a denominator had no inverse (needs mc->m.r3; a multi-modulus mc takes every
     * block's from its group constants) */
    void (*build)(void *stream, const gecm_modconst *mc, const uint64_t *sigma, uint32_t *X, uint32_t *Z, uint32_t *S,
                  uint32_t *flags, size_t stride);
    int fform_generic_limbs;      /* limbs of a 2^k -+ c modulus that are not 2^28 - 1 */
    /* one modulus's constants (r3 included) as the multi-modulus kernels read them from device memory: group_bytes bytes
     * at out */
    void (*pack_group)(const gecm_devmod *m, void *out);
    size_t group_bytes;
    const char *manifest;         /* the hash of the sources the object was compiled from (Makefile: K_SHA) */
    int has_lane;                 /* the per-lane kernels are built for this limb count (8 .. 15 limbs) */
    /* X <- X/Z, Z <- R mod N for every curve whose Z has an inverse, canonical; flags[curve] = 1 and X, Z untouched
     * where it has none (needs mc->m.r3; multi-modulus and lane-packed mc as for gcd_scan).  New members go at the
     * end: the ones above keep their places. */
    void (*normalize)(void *stream, const gecm_modconst *mc, uint32_t *X, uint32_t *Z, uint32_t *flags, size_t stride);
    /* GMP-ECM's PARAM 1 and 3 curves: for every curve with param[curve] = 1 or 3 (device array of
     * stride bytes), X = 2, Z = 1, S = sigma^2 / 2^64 or sigma / 2^32 in canonical Montgomery form and flags[curve] = 0;
     * the curves with param 0 keep what they hold.  Needs mc->m.r2, never inverts; a multi-modulus mc as for build. */
    void (*build_param)(void *stream, const gecm_modconst *mc, const uint64_t *sigma, const uint8_t *param, uint32_t *X,
                        uint32_t *Z, uint32_t *S, uint32_t *flags, size_t stride);
    /* P-1 (pp1 = 0) and P+1 (pp1 != 0) stage 1 on the tape: one residue per lane, X <- x^E or V_E(x)
     * in canonical Montgomery form, Z <- R mod N.  Generic REDC; any mc, a lane-packed one where has_lane. */
    void (*stage1_unit)(void *stream, const gecm_modconst *mc, const uint32_t *tape, uint32_t tape_len, uint32_t *X,
                        uint32_t *Z, size_t stride, int pp1);
    /* gcd_scan of V - off R mod N, off = 1 or 2: the factor test of a P-1 / P+1 residue in Montgomery form */
    void (*gcd_scan_off)(void *stream, const gecm_modconst *mc, const uint32_t *V, uint32_t *G, uint32_t *flags,
                         size_t stride, uint32_t off);
    /* the raw test-level operator: C = op(A, B), op = GECM_L0_MUL, _SQR, _ADD, _SUB or _CONDSUB (gecm_ops.h), by the field
     * function itself on the limbs as they are, and the limbs it leaves.  form as for stage1 picks the multiply; a
     * lane-packed mc takes form 0 (limb counts with has_lane), a wave-packed one is not served. */
    void (*l0_raw)(void *stream, const gecm_modconst *mc, int op, int form, const uint32_t *A, const uint32_t *B, uint32_t *C,
                   size_t stride);
};

/* Part 2: stage 2 (any mc takes K = 1, 2, .. 32; a lane-packed one at limb counts with has_lane). */
struct gecm_kernels_p2 {
    void (*s2_init)(void *stream, const gecm_modconst *mc, const gecm_s2_init_launch *h);
    void (*s2_pair)(void *stream, const gecm_modconst *mc, const gecm_s2_pair_launch *h);
    const char *manifest;
    /* Stage 2 of a P-1 / P+1 batch, on the same arguments.  s2_init_unit: P = X (pm1 = 0) or X + 1/X
     * (pm1 != 0; plane 0 of a.fail takes gcd(X, N) where there is no inverse) into a.S, acc = one, the table
     * PbX[map[j]] = V_j(P), PdX = V_D(P) and for a.K > 1 PdKX = V_{K D}(P); bx/bz/bp, PdZ and PdKZ are not touched.
     * s2_pair_unit: the tape as s2_pair walks it, the giant steps ring[s] = V_{(A0 / D + s) D}(P) at its marks (bit 31 of
     * a mark ignored, a.K sub-sequences at every one), the pair walk and the merge of s2_pair between them.  New members
     * go at the end. */
    void (*s2_init_unit)(void *stream, const gecm_modconst *mc, const gecm_s2_init_launch *h, int pm1);
    void (*s2_pair_unit)(void *stream, const gecm_modconst *mc, const gecm_s2_pair_launch *h);
};

/* the accessors: gecm_kernels_<nl>_p1 and _p2, one in each object */
#define GECM_KERNELS_DECL(nl)                                         \
    extern "C" const gecm_kernels_p1 *gecm_kernels_##nl##_p1(void);   \
    extern "C" const gecm_kernels_p2 *gecm_kernels_##nl##_p2(void);
GECM_NL_LIST(GECM_KERNELS_DECL)
#undef GECM_KERNELS_DECL
#endif
