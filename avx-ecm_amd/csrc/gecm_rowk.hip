// gecm_rowk.hip — the 32-lanes-per-curve stage-1 kernels (gecm_row.hpp).  One translation unit for all limb
// counts: the kernel is templated on the limbs per lane (NQ = 1, 2, 3 cover up to 16, 32, 48 limbs of 28 bits) and on
// the rows of a multiply (ROWS = the limbs of N' = m*N); the limb count of the device buffers is a run-time argument.
// With -DGECM_ROWK_WIDE the file compiles to the stage-1 kernels of the wide shapes and their launcher, nothing else.
#include "gecm_row.hpp"
#include <hip/hip_runtime.h>

// Four wavefronts per workgroup (they do not interact).  With one, the first launch of a process was 41 % slower than
// every later one in 13 of 18 runs (381 ms against 270 ms at 4096 curves, B1 = 1e5; 3.8 s against 2.7 s at B1 = 1e6 in
// the command-line driver, whose only stage-1 launch is its first): these kernels need few registers, a SIMD can take
// eight of their wavefronts, and nothing makes a cold dispatcher spread 2048 one-wavefront workgroups two per SIMD.
// A workgroup of four puts one wavefront on each SIMD of a CU: 14 first launches of 14 at full speed
// (profiles/r02_first_launch_workgroup_size.txt).
#ifndef GECM_ROW_WG_WAVES
#define GECM_ROW_WG_WAVES 4
#endif
template <int NQ, int ROWS, bool ALDS>
__global__ void __launch_bounds__(64 * GECM_ROW_WG_WAVES, 2)
k_stage1_row(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X, uint32_t *__restrict__ Z,
             const uint32_t *__restrict__ S, size_t stride, uint32_t nl, const uint32_t *__restrict__ rc, uint32_t rho_n)
{
    stage1_row<NQ, ROWS, ALDS>(tape, tape_len, X, Z, S, stride, nl, rc, rho_n);
}

#ifdef GECM_ROWK_WIDE
// The wide shapes (gecm_rowk.h) are an object of their own from this file (Makefile: gecm_rowk_wide.o):
// three more NQ = 3 kernels next to the others would double the build time of the one object, and in a second
// object they compile beside it.  Nothing but k_stage1_row<3, rows, false> is instantiated here.
extern "C" int gecm_launch_stage1_row_wide(void *stream, int rows, const uint32_t *tape, uint32_t tape_len, uint32_t *X,
                                           uint32_t *Z, const uint32_t *S, size_t stride, uint32_t nl, const uint32_t *rc,
                                           uint32_t rho_n)
{
    const dim3 grid((unsigned)(stride / (2 * GECM_ROW_WG_WAVES))), block(64 * GECM_ROW_WG_WAVES);   // stride: a multiple of 64
#define GECM_ROW_LAUNCH(q, r)                                                                                               \
    if (rows == r) {                                                                                                        \
        hipLaunchKernelGGL((k_stage1_row<q, r, false>), grid, block, 0, (hipStream_t)stream, tape, tape_len, X, Z, S,       \
                           stride, nl, rc, rho_n);                                                                          \
        return 0;                                                                                                           \
    }
    GECM_ROW_WIDE_SHAPES(GECM_ROW_LAUNCH)
#undef GECM_ROW_LAUNCH
    return -1;
}
#else
/* rc = device array of GECM_ROW_KINDS x GECM_ROW_WORDS words (gecm_row.hpp).  Leaves lazy values (limbs < 2^28 + 4,
 * value < K + 2N) in X, Z: the caller runs k_canon afterwards.  a_lds: operand broadcasts through the LDS crossbar
 * (for launches of 3 or more wavefronts per SIMD), built for nq = 1 only.  (nq, rows) must be one of the built pairs —
 * gecm_row_shape() of a built limb count; returns -1 otherwise, and for a_lds with nq != 1. */
extern "C" int gecm_launch_stage1_row(void *stream, int nq, int rows, const uint32_t *tape, uint32_t tape_len, uint32_t *X,
                                      uint32_t *Z, const uint32_t *S, size_t stride, uint32_t nl, const uint32_t *rc,
                                      uint32_t rho_n, bool a_lds)
{
    const dim3 grid((unsigned)(stride / (2 * GECM_ROW_WG_WAVES))), block(64 * GECM_ROW_WG_WAVES);   // stride: a multiple of 64
#define GECM_ROW_LAUNCH(q, r)                                                                                               \
    if (nq == q && rows == r) {                                                                                             \
        if constexpr (q == 1) {                                                                                             \
            if (a_lds) {                                                                                                    \
                hipLaunchKernelGGL((k_stage1_row<q, r, true>), grid, block, 0, (hipStream_t)stream, tape, tape_len, X, Z,   \
                                   S, stride, nl, rc, rho_n);                                                               \
                return 0;                                                                                                   \
            }                                                                                                               \
        }                                                                                                                   \
        if (a_lds) return -1;                                                                                               \
        hipLaunchKernelGGL((k_stage1_row<q, r, false>), grid, block, 0, (hipStream_t)stream, tape, tape_len, X, Z, S,       \
                           stride, nl, rc, rho_n);                                                                          \
        return 0;                                                                                                           \
    }
    GECM_ROW_SHAPES(GECM_ROW_LAUNCH)
#undef GECM_ROW_LAUNCH
    return -1;
}

// The same body on a multi-modulus batch, DPP form: the constants come from the table of the batch's
// moduli through the curve's group, which is uniform over the two rows of a curve (with lane packing the two curves of
// a wavefront may be on different numbers), and rho of N from the set instead of the argument list.  The workgroups and
// the grid of k_stage1_row.
template <int NQ, int ROWS>
__global__ void __launch_bounds__(64 * GECM_ROW_WG_WAVES, 2)
k_stage1_row_multi(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X, uint32_t *__restrict__ Z,
                   const uint32_t *__restrict__ S, size_t stride, uint32_t nl, const uint32_t *__restrict__ rc,
                   const uint32_t *__restrict__ curve_group, const uint32_t *__restrict__ block_group)
{
    const uint32_t cidx = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;      // < stride: the grid is stride / 8 blocks
    const uint32_t g = curve_group ? curve_group[cidx] : block_group[cidx >> 6];
    const uint32_t *set = rc + (size_t)g * GECM_MROW_SET;
    stage1_row<NQ, ROWS, false>(tape, tape_len, X, Z, S, stride, nl, set, set[GECM_ROW_KINDS * GECM_ROW_WORDS]);
}

extern "C" int gecm_launch_stage1_row_multi(void *stream, int nq, int rows, const uint32_t *tape, uint32_t tape_len,
                                            uint32_t *X, uint32_t *Z, const uint32_t *S, size_t stride, uint32_t nl,
                                            const uint32_t *rc, const uint32_t *curve_group, const uint32_t *block_group)
{
    if (!curve_group && !block_group) return -1;
    const dim3 grid((unsigned)(stride / (2 * GECM_ROW_WG_WAVES))), block(64 * GECM_ROW_WG_WAVES);   // stride: a multiple of 64
#define GECM_MROW_LAUNCH(q, r)                                                                                              \
    if (nq == q && rows == r) {                                                                                             \
        hipLaunchKernelGGL((k_stage1_row_multi<q, r>), grid, block, 0, (hipStream_t)stream, tape, tape_len, X, Z, S,        \
                           stride, nl, rc, curve_group, block_group);                                                       \
        return 0;                                                                                                           \
    }
    GECM_ROW_SHAPES(GECM_MROW_LAUNCH)
#undef GECM_MROW_LAUNCH
    return -1;
}

// One residue per row, four per wavefront: P-1 and P+1 stage 1 for small method batches (gecm_row.hpp, unit_row).
// Workgroups of four wavefronts for the reason above.  The method is wave-uniform; the constants come from the table of
// the batch's moduli through the position's group, which is uniform over a row (group 0 on a single-N context).
template <int NQ, int ROWS>
__global__ void __launch_bounds__(64 * GECM_ROW_WG_WAVES, 2)
k_unit_row(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X, size_t stride, uint32_t nl,
           uint32_t pp1, const uint32_t *__restrict__ rc, const uint32_t *__restrict__ curve_group,
           const uint32_t *__restrict__ block_group)
{
    const uint32_t pos = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;       // < stride: the grid is stride / 16 blocks
    const uint32_t g = curve_group ? curve_group[pos] : block_group ? block_group[pos >> 6] : 0u;
    unit_row<NQ, ROWS>(tape, tape_len, X, stride, nl, pp1 != 0, rc + (size_t)g * GECM_UROW_SET);
}

extern "C" int gecm_launch_unit_row(void *stream, int nq, int rows, const uint32_t *tape, uint32_t tape_len, uint32_t *X,
                                    size_t stride, uint32_t nl, int pp1, const uint32_t *rc, const uint32_t *curve_group,
                                    const uint32_t *block_group)
{
    const dim3 grid((unsigned)(stride / (4 * GECM_ROW_WG_WAVES))), block(64 * GECM_ROW_WG_WAVES);   // stride: a multiple of 64
#define GECM_UROW_LAUNCH(q, r)                                                                                              \
    if (nq == q && rows == r) {                                                                                             \
        hipLaunchKernelGGL((k_unit_row<q, r>), grid, block, 0, (hipStream_t)stream, tape, tape_len, X, stride, nl,          \
                           (uint32_t)(pp1 != 0), rc, curve_group, block_group);                                             \
        return 0;                                                                                                           \
    }
    GECM_ROW_SHAPES(GECM_UROW_LAUNCH)
#undef GECM_UROW_LAUNCH
    return -1;
}

#endif   // GECM_ROWK_WIDE

// the hash of the sources this object was compiled from (Makefile: R_SHA)
#ifndef GECM_MANIFEST
#define GECM_MANIFEST "unset"
#endif
#ifdef GECM_ROWK_WIDE
extern "C" const char *gecm_manifest_rowk_wide(void) { return GECM_MANIFEST; }
#else
extern "C" const char *gecm_manifest_rowk(void) { return GECM_MANIFEST; }
#endif
