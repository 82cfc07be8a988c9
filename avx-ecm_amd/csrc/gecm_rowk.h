/* gecm_rowk.h — launcher of the 32-lanes-per-curve stage-1 kernels (csrc/gecm_row.hpp, gecm_rowk.hip): one entry
 * point for every limb count. */
#ifndef GECM_ROWK_H
#define GECM_ROWK_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 32 lanes per curve (csrc/gecm_row.hpp, gecm_rowk.hip): nq = limbs per lane, rows = rows of a multiply = limbs in use
 * (the nl + 1 limbs of N' = m*N: 831 bits are 31 rows), nl = limbs per residue of the device buffers, rc = device array
 * of GECM_ROW_KINDS x GECM_ROW_WORDS constants.  Leaves lazy values in X, Z (run k_canon afterwards: canon of
 * gecm_launch.h's part-1 table).
 * a_lds: operand limbs are broadcast through the LDS crossbar instead of DPP (faster from 3 wavefronts per SIMD
 * up; nq = 1 only).  Returns -1 if (nq, rows) is not built, or if a_lds is set and nq != 1. */
#define GECM_ROW_WORDS 48     /* words per constant array: limbs 0 .. 16*nq-1, zero padded */
#define GECM_ROW_KINDS 5
#define GECM_ROW_MAXNQ 3
/* the shapes built: one per built limb count nl (gecm_launch.h's list): nq = ceil((nl+1)/16), rows = nl + 1 */
#define GECM_ROW_SHAPES(X) X(1, 9) X(1, 11) X(1, 13) X(1, 15) X(1, 16) X(2, 18) X(2, 20) X(2, 22) X(2, 24) X(2, 27) X(2, 29) \
    X(2, 31) X(3, 33) X(3, 35) X(3, 38)
static inline void gecm_row_shape(int nl, int *nq, int *rows)
{
    *nq = (nl + 1 + 15) / 16;
    *rows = nl + 1;
}
int gecm_launch_stage1_row(void *stream, int nq, int rows, const uint32_t *tape, uint32_t tape_len, uint32_t *X, uint32_t *Z,
                           const uint32_t *S, size_t stride, uint32_t nl, const uint32_t *rc, uint32_t rho_n,
                           bool a_lds);

/* The wide shapes: limb counts above gecm_launch.h's list, nl = 40, 43 and 47 (N up to 1115, 1199 and
 * 1311 bits), which have no other kernel.  k_stage1_row<3, rows, false> alone is built for them (no multi-modulus form,
 * no method kernel, no crossbar form), in an object of its own from gecm_rowk.hip.  The same arguments and the same lazy
 * exit values as gecm_launch_stage1_row; nothing canonicalises them on the device: the entry multiply of the next launch
 * takes them as they are, and the host reduces what it downloads.  Returns -1 if rows is not one of the list. */
#define GECM_ROW_WIDE_SHAPES(X) X(3, 41) X(3, 44) X(3, 48)
int gecm_launch_stage1_row_wide(void *stream, int rows, const uint32_t *tape, uint32_t tape_len, uint32_t *X, uint32_t *Z,
                                const uint32_t *S, size_t stride, uint32_t nl, const uint32_t *rc, uint32_t rho_n);

/* 32 lanes per curve on a multi-modulus batch (k_stage1_row_multi): the same kernel body, DPP form, with
 * the constants of every curve taken from a table.  rc = device table of one set per modulus, GECM_MROW_KINDS x
 * GECM_ROW_WORDS words each: the GECM_ROW_KINDS arrays above for that modulus ([0] N' = m*N with R' >= 32 N', [1] N,
 * [2] entry factor, [3] R mod N, [4] K'), then [5] word 0: -N^-1 mod 2^28 (the exit multiply's rho).  Not the method
 * kernel's set below: its N'' only has R' > 28 N''.
 * A curve takes set curve_group[curve] (lane packing) or block_group[curve / 64] (wave packing); one of the two is
 * given, with an entry below the table's size for every position of the stride, padding included.
 * Leaves lazy values in X, Z (run canon afterwards).  Returns -1 if (nq, rows) is not built or both tables are NULL. */
#define GECM_MROW_KINDS (GECM_ROW_KINDS + 1)
#define GECM_MROW_SET (GECM_MROW_KINDS * GECM_ROW_WORDS)
int gecm_launch_stage1_row_multi(void *stream, int nq, int rows, const uint32_t *tape, uint32_t tape_len, uint32_t *X,
                                 uint32_t *Z, const uint32_t *S, size_t stride, uint32_t nl, const uint32_t *rc,
                                 const uint32_t *curve_group, const uint32_t *block_group);

/* 16 lanes per residue: P-1 and P+1 stage 1 with one residue per DPP row (k_unit_row).  The kernel works
 * modulo N'' = (m + t 2^28) N, the multiple of N that is -1 modulo 2^28 AND fills the row: N'' >= 2^(28 (rows - 1) + 20),
 * so that the top limb of a value tells its quotient by N'' (the reduction after a P+1 subtraction), and
 * N'' < 2^(28 rows - 5) (1 + 2^-3) (t is the smallest that reaches the first bound): R' = 2^(28 rows) > 28 N''.
 * rc = device table of one constant set per modulus, GECM_UROW_KINDS x GECM_ROW_WORDS words each, limb j at word j:
 *   [0] N''   [1] N   [2] entry factor R'^2 / R mod N   [3] R mod N   [4] K' of N
 *   [5] 2 R' mod N'', the residue nearest zero, in balanced limbs (|limb| <= 2^27 below the top one; two's complement)
 *   [6] word 0: the float 1 / (N'' / 2^(28 (rows - 1))) as its bits; word 1: -N^-1 mod 2^28 (the exit multiply's rho)
 * A position takes set curve_group[pos] (lane packing), block_group[pos / 64] (wave packing) or, with both NULL, set 0.
 * Leaves a lazy value in X (run canon afterwards); Z is not touched.  Returns -1 if (nq, rows) is not built. */
#define GECM_UROW_KINDS 7
#define GECM_UROW_SET (GECM_UROW_KINDS * GECM_ROW_WORDS)
#define GECM_UROW_TOP_MIN_BITS 20   /* limb rows - 1 of N'' is at least 2^20 */
int gecm_launch_unit_row(void *stream, int nq, int rows, const uint32_t *tape, uint32_t tape_len, uint32_t *X, size_t stride,
                         uint32_t nl, int pp1, const uint32_t *rc, const uint32_t *curve_group, const uint32_t *block_group);

#ifdef __cplusplus
}
#endif
#endif
