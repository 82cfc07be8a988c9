/* gecm_ops.h — what the host logic (gecm_mod.h, gecm_api.c), the device layer (gecm_dev.h) and the kernels' launchers
 * (gecm_launch.h, gecm_kernels.hip) all speak: the constants of one modulus as the device layer takes them, and the
 * operator codes of the test-level L0 kernel.  Plain C.  Kept apart from gecm_dev.h so that a change of the host <->
 * device-layer interface does not recompile thirty kernel objects. */
#ifndef GECM_OPS_H
#define GECM_OPS_H
#include <stdint.h>

/* One modulus N at nl limbs of 28 bits, R = 2^(28 nl): N, K' (the lazy subtraction's multiple of N), R mod N, R^2 mod N,
 * R^3 mod N, rho = -N^-1 mod 2^28 and the inversion's batches of 28 division steps.  Filled in one place per kind of
 * modulus (gecm_mod_devmod; ff_setup for the special-form twin) and passed whole; gecm_dev_open and gecm_dev_set_groups
 * copy what the pointers name. */
typedef struct {
    const uint32_t *n, *kp, *one, *r2, *r3;   /* nl limbs each; r3 NULL: a context that never inverts */
    uint32_t rho, inv_iters;
} gecm_devmod;

enum { GECM_L0_MUL = 0, GECM_L0_SQR = 1, GECM_L0_ADD = 2, GECM_L0_SUB = 3, GECM_L0_ADDSUB = 4 };
/* the raw test-level operator (k_l0_raw): MUL, SQR, ADD, SUB as above, and fe_cond_sub_n of the first operand */
enum { GECM_L0_CONDSUB = 5 };
#endif
