// gecm_kernels.hip — HIP kernels of libgecm for ONE limb count (compile with -DGECM_NL=<n>).
// One translation unit per limb count so the (large, fully unrolled) kernels build in parallel.
// See gecm_field.hpp / gecm_curve.hpp for the arithmetic; DESIGN.md for the layout.
#include "gecm_ops.h"
#include "gecm_launch.h"
#include "gecm_curve.hpp"
#include "gecm_stage2.hpp"
#include "gecm_quad.hpp"
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstring>
#include <type_traits>

#ifndef GECM_NL
#error "compile with -DGECM_NL=<limbs>"
#endif
// GECM_PART splits one limb count over two objects so the build parallelises better:
//   1 = stage 1, de-Montgomeryisation, L0 operators, factor scan;  2 = stage 2;  unset = both.
#ifndef GECM_PART
#define GECM_PART 0
#endif
#define GECM_HAS_PART(p) (GECM_PART == 0 || GECM_PART == (p))

template <int NL>
struct ModArgs {
    ModK<NL> m;
    Fe<NL> one;   // R mod N, canonical
};

// Where a kernel finds the constants of its modulus.  A single-N launch passes ModArgs / S2Const by value; a
// multi-modulus launch (one modulus per wavefront) passes ModGroups: one S2Const per modulus in device
// memory and the modulus of every 64-curve block.  mod_consts() gives a kernel the constants of its curve block from
// either source, as a reference the multiplies read as wave-uniform operands; each single-N kernel and its _multi twin
// share one body (GECM_STAGE1_BODY and the like).
// One modulus's constants block in device memory: S2Const, then what only the multi-modulus kernels without a by-value
// twin of it need.  New fields go at the end: the kernels that read a prefix keep their offsets.
template <int NL>
struct GroupConst {
    S2Const<NL> k;
    Fe<NL> r2;    // R^2 mod N  (plain residue -> Montgomery form, k_to_mont_multi)
};

template <int NL>
struct ModGroups {
    const GroupConst<NL> *groups; // read-only for the whole launch
    const uint32_t *block_group;  // modulus of curve block b (curves 64b .. 64b+63)
};
static_assert(offsetof(GroupConst<GECM_NL>, k) == 0, "S2Const must be a prefix of GroupConst");
static_assert(offsetof(S2Const<GECM_NL>, m) == offsetof(ModArgs<GECM_NL>, m) &&
              offsetof(S2Const<GECM_NL>, one) == offsetof(ModArgs<GECM_NL>, one),
              "ModArgs must be a prefix of S2Const: multi-modulus kernels read one through the other");

template <class A>
__device__ __forceinline__ const A &mod_consts(const A &a, uint32_t) { return a; }

// The loads go through the constant address space: the constants are read-only while the kernel runs, so the
// compiler fetches them with scalar loads at a wave-uniform address and may fetch them again where it needs them
// instead of holding them in registers, as it does with kernel arguments.
template <class A, int NL>
__device__ __forceinline__ const A &mod_consts(const ModGroups<NL> &g, uint32_t block)
{
    typedef const __attribute__((address_space(4))) uint32_t c_u32;
    typedef const __attribute__((address_space(4))) GroupConst<NL> c_grp;
    const uint32_t grp = ((c_u32 *)g.block_group)[block];
    return *(const A *)(const GroupConst<NL> *)((c_grp *)g.groups + grp);
}

// Lane-packed multi-modulus launch (one modulus per lane): the same constants array, and the modulus of
// every curve.  Built for the limb counts up to GECM_LANE_MAXNL; lane_consts() gives a lane the constants of its own
// curve: N and rho into registers, K' into the lane's LDS column `kp_col` (word limb*64), the residues R, R^3 and R^2
// mod N left in global memory behind a pointer (FeG).
#define GECM_LANE_MAXNL 15
#define GECM_HAS_LANE (GECM_NL <= GECM_LANE_MAXNL)
template <int NL>
struct LaneGroups {
    const GroupConst<NL> *groups; // read-only for the whole launch
    const uint32_t *curve_group;  // modulus of curve position p
};

template <int NL>
struct LaneConst : S2ConstV<NL> {
    FeG<NL> r2;
};

template <int NL>
__device__ __forceinline__ void lane_consts(LaneConst<NL> &k, const LaneGroups<NL> &g, uint32_t idx, uint32_t *kp_col)
{
    const uint32_t *gp = (const uint32_t *)(g.groups + g.curve_group[idx]);
    const uint32_t *mp = gp + offsetof(GroupConst<NL>, k.m) / 4;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        k.m.n[i] = mp[offsetof(ModK<NL>, n) / 4 + i];
        kp_col[i * 64] = mp[offsetof(ModK<NL>, kp) / 4 + i];
    }
    k.m.kp = kp_col;
    k.m.rho = mp[offsetof(ModK<NL>, rho) / 4];
    k.one.p = gp + offsetof(GroupConst<NL>, k.one) / 4;
    k.r3.p = gp + offsetof(GroupConst<NL>, k.r3) / 4;
    k.inv_iters = gp[offsetof(GroupConst<NL>, k.inv_iters) / 4];
    k.r2.p = gp + offsetof(GroupConst<NL>, r2) / 4;
}
// every lane kernel starts with this: `k` = the constants of curve position idx
#define GECM_LANE_CONSTS                                                        \
    __shared__ uint32_t lds_kp[NL * 64];                                        \
    LaneConst<NL> k;                                                            \
    lane_consts(k, g, idx, lds_kp + threadIdx.x);

#if GECM_HAS_PART(1)
// ---------------------------------------------------------------- stage 1
// One curve per lane.  64-thread blocks (one wave): a CU holds 8 of them at 2 waves/SIMD, the
// occupancy at which v_mad_u64_u32 issues back-to-back (profiles/r01_valu_ubench_gfx950.txt).
// The body of k_stage1 and k_stage1_multi, with the constants in `a` (a ModArgs<NL>).  A macro, not a device function
// over the constants source: through such a function the single-N kernels compiled to different code at some limb
// counts (operand order, register choice, stack layout), and they must stay instruction for instruction what they
// were.  The other single-N / multi pairs below share their bodies the same way.
#define GECM_STAGE1_BODY                                                        \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Pt<NL> P;                                                                   \
    fe_load(P.X, X, stride, idx);                                               \
    fe_load(P.Z, Z, stride, idx);                                               \
    constexpr bool CL = TapePolicy<NL>::c_in_lds;                               \
    __shared__ uint32_t lds_c[CL ? 2 * NL * 64 : 1];                            \
    CStore<NL, CL> cst;                                                         \
    if constexpr (CL) cst.lds = lds_c + threadIdx.x;                            \
    run_tape<NL>(tape, tape_len, P, S, stride, idx, a.m, cst);                  \
    Fe<NL> ox, oz;                                                              \
    fe_canonical_mont(ox, P.X, a.one, a.m);                                     \
    fe_canonical_mont(oz, P.Z, a.one, a.m);                                     \
    fe_store(X, stride, idx, ox);                                               \
    fe_store(Z, stride, idx, oz);

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_stage1(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
         uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModArgs<NL> a)
{
    GECM_STAGE1_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_stage1_multi(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
               uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModGroups<NL> g)
{
    const ModArgs<NL> &a = mod_consts<ModArgs<NL>>(g, blockIdx.x);
    GECM_STAGE1_BODY
}
#undef GECM_STAGE1_BODY

#if GECM_HAS_LANE
// One curve per lane and a modulus per lane.  The third PRAC point waits in LDS at every limb count (the column the
// C store of TapePolicy uses above its threshold): the registers it leaves hold the lane's N.
template <int NL>
__global__ void __launch_bounds__(64, 2)
k_stage1_lane(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
              uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, LaneGroups<NL> g)
{
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    GECM_LANE_CONSTS
    Pt<NL> P;
    fe_load(P.X, X, stride, idx);
    fe_load(P.Z, Z, stride, idx);
    __shared__ uint32_t lds_c[2 * NL * 64];
    CStore<NL, true> cst;
    cst.lds = lds_c + threadIdx.x;
    run_tape<NL>(tape, tape_len, P, S, stride, idx, k.m, cst);
    Fe<NL> ox, oz;
    fe_canonical_mont(ox, P.X, k.one, k.m);
    fe_canonical_mont(oz, P.Z, k.one, k.m);
    fe_store(X, stride, idx, ox);
    fe_store(Z, stride, idx, oz);
}
#endif

// Stage 1 modulo Mw = 2^k - 1 (gecm_field.hpp, "F-form"): the same interpreter, the REDC half of every
// multiply replaced by the shift-and-subtract form.  Used by the host for N | 2^k - 1.
template <int NL, class MOD>
struct ModArgsS {
    MOD m;
    Fe<NL> one;
};

// MOD = ModF<NL> (2^k - 1), ModP<NL> (2^k + 1) or ModC<NL> (2^k - c)
template <int NL, class MOD>
__global__ void __launch_bounds__(64, 2)
k_stage1_f(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
           uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModArgsS<NL, MOD> a)
{
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    Pt<NL> P;
    fe_load(P.X, X, stride, idx);
    fe_load(P.Z, Z, stride, idx);
    constexpr bool CL = TapePolicy<NL>::c_in_lds;
    __shared__ uint32_t lds_c[CL ? 2 * NL * 64 : 1];
    CStore<NL, CL> cst;
    if constexpr (CL) cst.lds = lds_c + threadIdx.x;
    run_tape<NL>(tape, tape_len, P, S, stride, idx, a.m, cst);
    Fe<NL> ox, oz;
    fe_canonical_mont(ox, P.X, a.one, a.m);
    fe_canonical_mont(oz, P.Z, a.one, a.m);
    fe_store(X, stride, idx, ox);
    fe_store(Z, stride, idx, oz);
}

// Two lanes per curve (gecm_curve.hpp, "split-coordinate"): lane 2j works on X, lane 2j+1 on Z of
// curve blockIdx.x*32 + j.  Chosen by the device layer for batches that leave SIMDs under-occupied.
// (a macro for the reason given at GECM_STAGE1_BODY; the constants are in `a`, a ModArgs<NL>)
#define GECM_STAGE1_PAIR_BODY                                                   \
    const uint32_t cidx = blockIdx.x * 32u + (threadIdx.x >> 1);                \
    const bool isZ = (threadIdx.x & 1u) != 0;                                   \
    uint32_t *mine = isZ ? Z : X;                                               \
    Fe<NL> P;                                                                   \
    fe_load(P, mine, stride, cidx);                                             \
    run_tape_pair<NL>(tape, tape_len, P, S, stride, cidx, isZ, a.m);            \
    Fe<NL> o;                                                                   \
    fe_canonical_mont(o, P, a.one, a.m);                                        \
    fe_store(mine, stride, cidx, o);

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_stage1_pair(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
              uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModArgs<NL> a)
{
    GECM_STAGE1_PAIR_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_stage1_pair_multi(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
                    uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModGroups<NL> g)
{
    const ModArgs<NL> &a = mod_consts<ModArgs<NL>>(g, blockIdx.x >> 1);   // 32 curves per block
    GECM_STAGE1_PAIR_BODY
}
#undef GECM_STAGE1_PAIR_BODY

template <int NL, class MOD>
__global__ void __launch_bounds__(64, 2)
k_stage1_pair_f(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
                uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModArgsS<NL, MOD> a)
{
    const uint32_t cidx = blockIdx.x * 32u + (threadIdx.x >> 1);
    const bool isZ = (threadIdx.x & 1u) != 0;
    uint32_t *mine = isZ ? Z : X;
    Fe<NL> P;
    fe_load(P, mine, stride, cidx);
    run_tape_pair<NL>(tape, tape_len, P, S, stride, cidx, isZ, a.m);
    Fe<NL> o;
    fe_canonical_mont(o, P, a.one, a.m);
    fe_store(mine, stride, cidx, o);
}

// Eight lanes per curve (gecm_quad.hpp).
// 256-thread workgroups (four independent wavefronts): this kernel needs about 65 registers, and one-wavefront
// workgroups of such a kernel are not spread evenly by a cold dispatcher — see gecm_rowk.hip; its first launch of a
// process measured 745 ms against 483 ms at 8192 curves.
template <int NL>
__global__ void __launch_bounds__(256, 2)
k_stage1_quad(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
              uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, const uint32_t *__restrict__ modq,
              uint32_t rho)
{
    const uint32_t cidx = (blockIdx.x * blockDim.x + threadIdx.x) >> 3;
    const uint32_t l = threadIdx.x & 3u;
    const bool isZ = (threadIdx.x & 4u) != 0;
    uint32_t *mine = isZ ? Z : X;
    constexpr int NQ = QuadShape<NL>::NQ;
    QuadMod<NL> m;
#pragma unroll
    for (int t = 0; t < NQ; t++) {         // modq: [n limbs 0..39 | K' limbs 0..39], zero padded
        m.n[t] = modq[NQ * l + t];
        m.kp[t] = modq[40 + NQ * l + t];
    }
    m.rho = rho;
    m.is0 = l == 0;
    m.top_mask = l == 3 ? 0u : 0xffffffffu;
    FeQn<NQ> P;
    feq_load<NL>(P, mine, stride, cidx, l);
    run_tape_quad<NL>(tape, tape_len, P, S, stride, cidx, l, isZ, m);
    feq_store<NL>(mine, stride, cidx, l, P);    // lazy representative; k_canon makes it canonical
}

// canonical Montgomery form of X, Z in place (the tail of k_stage1, for kernels that leave lazy values)
// (macros for the reason given at GECM_STAGE1_BODY; the constants are in `a`, a ModArgs<NL>)
#define GECM_CANON_BODY                                                         \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Fe<NL> x, z, r;                                                             \
    fe_load(x, X, stride, idx);                                                 \
    fe_load(z, Z, stride, idx);                                                 \
    fe_canonical_mont(r, x, a.one, a.m);                                        \
    fe_store(X, stride, idx, r);                                                \
    fe_canonical_mont(r, z, a.one, a.m);                                        \
    fe_store(Z, stride, idx, r);

template <int NL>
__global__ void __launch_bounds__(64)
k_canon(uint32_t *__restrict__ X, uint32_t *__restrict__ Z, size_t stride, ModArgs<NL> a)
{
    GECM_CANON_BODY
}

template <int NL>
__global__ void __launch_bounds__(64)
k_canon_multi(uint32_t *__restrict__ X, uint32_t *__restrict__ Z, size_t stride, ModGroups<NL> g)
{
    const ModArgs<NL> &a = mod_consts<ModArgs<NL>>(g, blockIdx.x);
    GECM_CANON_BODY
}
#undef GECM_CANON_BODY

#define GECM_FROM_MONT_BODY                                                     \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Fe<NL> x, z, r;                                                             \
    fe_load(x, X, stride, idx);                                                 \
    fe_load(z, Z, stride, idx);                                                 \
    fe_from_mont_canonical(r, x, a.m);                                          \
    fe_store(ox, stride, idx, r);                                               \
    fe_from_mont_canonical(r, z, a.m);                                          \
    fe_store(oz, stride, idx, r);

template <int NL>
__global__ void __launch_bounds__(64)
k_from_mont(const uint32_t *__restrict__ X, const uint32_t *__restrict__ Z, uint32_t *__restrict__ ox,
            uint32_t *__restrict__ oz, size_t stride, ModArgs<NL> a)
{
    GECM_FROM_MONT_BODY
}

template <int NL>
__global__ void __launch_bounds__(64)
k_from_mont_multi(const uint32_t *__restrict__ X, const uint32_t *__restrict__ Z, uint32_t *__restrict__ ox,
                  uint32_t *__restrict__ oz, size_t stride, ModGroups<NL> g)
{
    const ModArgs<NL> &a = mod_consts<ModArgs<NL>>(g, blockIdx.x);
    GECM_FROM_MONT_BODY
}
#undef GECM_FROM_MONT_BODY

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64)
k_from_mont_lane(const uint32_t *__restrict__ X, const uint32_t *__restrict__ Z, uint32_t *__restrict__ ox,
                 uint32_t *__restrict__ oz, size_t stride, LaneGroups<NL> g)
{
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    GECM_LANE_CONSTS
    Fe<NL> x, z, r;
    fe_load(x, X, stride, idx);
    fe_load(z, Z, stride, idx);
    fe_from_mont_canonical(r, x, k.m);
    fe_store(ox, stride, idx, r);
    fe_from_mont_canonical(r, z, k.m);
    fe_store(oz, stride, idx, r);
}
#endif

// The inverse: canonical plain residues x, z in [0, N) -> X = x R mod N, Z = z R mod N, canonical, by one multiply with
// R^2 mod N each (x R^2 / R < N^2/R + N < 2N, then one conditional subtract).  The constants are in `a`, a ModArgs<NL>,
// and R^2 mod N in `r2`.
#define GECM_TO_MONT_BODY                                                       \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Fe<NL> x, z, r;                                                             \
    fe_load(x, ix, stride, idx);                                                \
    fe_load(z, iz, stride, idx);                                                \
    fe_mul(r, x, r2, a.m);                                                      \
    fe_cond_sub_n(r, a.m);                                                      \
    fe_store(X, stride, idx, r);                                                \
    fe_mul(r, z, r2, a.m);                                                      \
    fe_cond_sub_n(r, a.m);                                                      \
    fe_store(Z, stride, idx, r);

template <int NL>
__global__ void __launch_bounds__(64)
k_to_mont(const uint32_t *__restrict__ ix, const uint32_t *__restrict__ iz, uint32_t *__restrict__ X,
          uint32_t *__restrict__ Z, size_t stride, ModArgs<NL> a, Fe<NL> r2)
{
    GECM_TO_MONT_BODY
}

template <int NL>
__global__ void __launch_bounds__(64)
k_to_mont_multi(const uint32_t *__restrict__ ix, const uint32_t *__restrict__ iz, uint32_t *__restrict__ X,
                uint32_t *__restrict__ Z, size_t stride, ModGroups<NL> g)
{
    const GroupConst<NL> &c = mod_consts<GroupConst<NL>>(g, blockIdx.x);
    const ModArgs<NL> &a = *(const ModArgs<NL> *)&c;
    const Fe<NL> &r2 = c.r2;
    GECM_TO_MONT_BODY
}
#undef GECM_TO_MONT_BODY

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64)
k_to_mont_lane(const uint32_t *__restrict__ ix, const uint32_t *__restrict__ iz, uint32_t *__restrict__ X,
               uint32_t *__restrict__ Z, size_t stride, LaneGroups<NL> g)
{
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    GECM_LANE_CONSTS
    Fe<NL> x, z, r;
    fe_load(x, ix, stride, idx);
    fe_load(z, iz, stride, idx);
    fe_mul(r, x, k.r2, k.m);
    fe_cond_sub_n(r, k.m);
    fe_store(X, stride, idx, r);
    fe_mul(r, z, k.r2, k.m);
    fe_cond_sub_n(r, k.m);
    fe_store(Z, stride, idx, r);
}
#endif

// ---------------------------------------------------------------- L0 test-level operators
template <int NL>
__global__ void __launch_bounds__(64)
k_l0(int op, const uint32_t *__restrict__ A, const uint32_t *__restrict__ B, uint32_t *__restrict__ C,
     uint32_t *__restrict__ D, size_t stride, ModArgs<NL> a, Fe<NL> fix)
{
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    Fe<NL> x, y, r, t;
    fe_load(x, A, stride, idx);
    fe_load(y, B, stride, idx);
    if (op == GECM_L0_MUL) {
        fe_mul(t, x, y, a.m);
        fe_canonical_mont(r, t, fix, a.m);
        fe_store(C, stride, idx, r);
    } else if (op == GECM_L0_SQR) {
        fe_sqr(t, x, a.m);
        fe_canonical_mont(r, t, fix, a.m);
        fe_store(C, stride, idx, r);
    } else {
        if (op == GECM_L0_ADD || op == GECM_L0_ADDSUB) {
            fe_add(t, x, y);
            fe_canonical_mont(r, t, a.one, a.m);
            fe_store(C, stride, idx, r);
        }
        if (op == GECM_L0_SUB || op == GECM_L0_ADDSUB) {
            fe_sub(t, x, y, a.m);
            fe_canonical_mont(r, t, a.one, a.m);
            fe_store(op == GECM_L0_SUB ? C : D, stride, idx, r);
        }
    }
}

// The sixth test-level operator: the device inversion on chosen inputs, through the routine every stage-2 batch
// inversion goes through (fe_inv_mont: fe_invert with the modulus's inv_iters, the R^3 step, the failure record).
// A = x Rref canonical; fe_inv_mont reads it as (x Rref/Rint) Rint and gives x^-1 Rint^2/Rref, which `fix` =
// Rref^2/Rint takes to x^-1 Rref; 0 where the inverse does not exist.  G = gcd(A, N) as a plain integer: 1, or the
// failure record stage 2 would keep.  A kernel of its own so that k_l0 stays what it was.
template <int NL>
__global__ void __launch_bounds__(64, 2)
k_l0_inv(const uint32_t *__restrict__ A, uint32_t *__restrict__ C, uint32_t *__restrict__ G, size_t stride, S2Const<NL> k,
         Fe<NL> fix)
{
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    Fe<NL> x, t, r, g1;
    fe_load(x, A, stride, idx);
#pragma unroll
    for (int i = 0; i < NL; i++) g1.v[i] = (i == 0) ? 1u : 0u;
    fe_store(G, stride, idx, g1);
    fe_inv_mont(t, x, k, G, stride, idx);
    fe_canonical_mont(r, t, fix, k.m);
    fe_store(C, stride, idx, r);
}

// ---------------------------------------------------------------- factor scan
// check_factor (ecm.c:2542-2557) for every curve on the device: g = gcd(v, N) by the same
// fixed-iteration binary algorithm the stage-2 inversion uses; flag = 1 iff 1 < g < N.
// v is any representative (Montgomery form or not: R is a power of two, N is odd).
// (a macro for the reason given at GECM_STAGE1_BODY; the constants are in `k`, an S2Const<NL>)
#define GECM_GCD_SCAN_BODY                                                      \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Fe<NL> v, c, t, g;                                                          \
    fe_load(v, V, stride, idx);                                                 \
    fe_canonical_mont(c, v, k.one, k.m);                                        \
    fe_invert(t, g, c, k.m, k.inv_iters);                                       \
    bool is_one = g.v[0] == 1u, is_n = true;                                    \
    _Pragma("unroll")                                                           \
    for (int i = 0; i < NL; i++) {                                              \
        if (i > 0) is_one = is_one && g.v[i] == 0;                              \
        is_n = is_n && g.v[i] == k.m.n[i];                                      \
    }                                                                           \
    fe_store(G, stride, idx, g);                                                \
    flags[idx] = (!is_one && !is_n) ? 1u : 0u;

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_gcd_scan(const uint32_t *__restrict__ V, uint32_t *__restrict__ G, uint32_t *__restrict__ flags, size_t stride,
           S2Const<NL> k)
{
    GECM_GCD_SCAN_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_gcd_scan_multi(const uint32_t *__restrict__ V, uint32_t *__restrict__ G, uint32_t *__restrict__ flags, size_t stride,
                 ModGroups<NL> groups)
{
    const S2Const<NL> &k = mod_consts<S2Const<NL>>(groups, blockIdx.x);
    GECM_GCD_SCAN_BODY
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64, 2)
k_gcd_scan_lane(const uint32_t *__restrict__ V, uint32_t *__restrict__ G, uint32_t *__restrict__ flags, size_t stride,
                LaneGroups<NL> g)
{
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    GECM_LANE_CONSTS
    Fe<NL> v, c, t, gc;
    fe_load(v, V, stride, idx);
    fe_canonical_mont(c, v, k.one, k.m);
    fe_invert(t, gc, c, k.m, k.inv_iters);
    bool is_one = gc.v[0] == 1u, is_n = true;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        if (i > 0) is_one = is_one && gc.v[i] == 0;
        is_n = is_n && gc.v[i] == k.m.n[i];
    }
    fe_store(G, stride, idx, gc);
    flags[idx] = (!is_one && !is_n) ? 1u : 0u;
}
#endif
#undef GECM_GCD_SCAN_BODY

// ---------------------------------------------------------------- curve construction
// The Suyama construction of one curve per lane (build_one_curve, ecm.c:1548-1803; on the host: suyama_pre and the tail
// of gecm_mod_build_slice), in Montgomery arithmetic: out come the words the host path uploads, X = (u^3 / v^3) R,
// Z = R, S = ((v-u)^3 (3u+v) / 16 u^3 v) R, canonical in [0, N), and one flag per curve.
//   sigma R = mont(sigma, R^2) with sigma's 64 bits in three limbs: the multiply takes any operand below 1.675 K
//   (gecm_field.hpp) and K >= R/32 >= 2^219, so sigma >= N needs no reduction first; the small constants 3, 4, 5, 16
//   enter the same way.  u = sigma^2 - 5 leaves fe_sub lazy and is passed through one multiply by R mod N before it is
//   subtracted itself (fe_sub wants a normalised subtrahend).  Every other operand of a multiply is a product
//   (< 0.675 K), a sum of two (< 1.35 K) or a difference of two (< 1.675 K).
// One inversion serves both quotients: (16u^3v * v^3)^-1 times v^3 and times 16u^3v.  Inverses are unique, so this is
// what the reference's two mpz_invert calls return (ecm.c:1745, 1759) whenever both exist.  A lane whose shared
// inversion fails inverts the two denominators one by one; a denominator without an inverse gets the reference's stale
// operand in the inverse's place — 16 u^3 for (16u^3v)^-1, (v-u)^3(3u+v) for (v^3)^-1, see gecm_mod_build_slice — and
// the curve is flagged.
// Live set: u^3, 16u^3 and the numerator wait in the X, Z and S planes while the inversion runs, so two residues are
// live across it.  The multiplies are the out-of-line ones of the stage-2 ladders (ModKOut) at every limb count: a
// build is some thirty multiplies next to an inversion of about fifty multiplies' worth, run once per batch, and
// inlined they added more to the build time of an object than the rest of its kernels.
template <int NL>
__device__ __forceinline__ void fe_small(Fe<NL> &r, uint32_t c)
{
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = (i == 0) ? c : 0u;
}

// r = the inverse of the Montgomery-form value a, in Montgomery form (fe_inv_mont without its failure record)
template <int NL>
__device__ __forceinline__ bool build_invert(Fe<NL> &r, const Fe<NL> &a, const S2Const<NL> &k, const ModKOut<NL> &mm)
{
    Fe<NL> c, t, g;
    fe_mul(c, a, k.one, mm);
    fe_cond_sub_n(c, k.m);                        // canonical x R
    const bool ok = fe_invert(t, g, c, k.m, k.inv_iters);
    fe_mul(r, t, k.r3, mm);                       // (x R)^-1 R^3 / R = x^-1 R
    return ok;
}

template <int NL>
__device__ __forceinline__ void build_curve(uint64_t sg, uint32_t *__restrict__ X, uint32_t *__restrict__ Z,
                                            uint32_t *__restrict__ S, uint32_t *__restrict__ flags, size_t stride,
                                            uint32_t idx, const S2Const<NL> &k, const Fe<NL> &r2)
{
    static_assert(NL >= 3, "sigma takes three limbs");
    const ModKOut<NL> mm{k.m};
    Fe<NL> t, u, v, w, den, z3;
    fe_small(t, (uint32_t)sg & GECM_LIMB_MASK);
    t.v[1] = (uint32_t)(sg >> GECM_LIMB_BITS) & GECM_LIMB_MASK;
    t.v[2] = (uint32_t)(sg >> (2 * GECM_LIMB_BITS));
    fe_mul(w, t, r2, mm);                         // sigma R
    fe_small(t, 4u);
    fe_mul(t, t, r2, mm);
    fe_mul(v, w, t, mm);                          // v = 4 sigma            ecm.c:1588-1589
    fe_sqr(u, w, mm);
    fe_small(t, 5u);
    fe_mul(t, t, r2, mm);
    fe_sub(u, u, t, mm);
    fe_mul(u, u, k.one, mm);                      // u = sigma^2 - 5        ecm.c:1596-1598, normalised limbs
    fe_sqr(t, u, mm);
    fe_mul(w, t, u, mm);                          // x = u^3                ecm.c:1601-1603
    fe_store(X, stride, idx, w);
    fe_small(t, 16u);
    fe_mul(t, t, r2, mm);
    fe_mul(w, w, t, mm);                          // 16 u^3                 ecm.c:1718
    fe_store(Z, stride, idx, w);
    fe_mul(den, w, v, mm);                        // 16 u^3 v               ecm.c:1718-1720
    fe_sqr(t, v, mm);
    fe_mul(z3, t, v, mm);                         // z = v^3                ecm.c:1607-1609
    fe_small(t, 3u);
    fe_mul(t, t, r2, mm);
    fe_mul(t, t, u, mm);
    fe_add(t, t, v);                              // 3u + v                 ecm.c:1632-1634
    fe_sub(w, v, u, mm);                          // v - u                  ecm.c:1615-1623
    fe_sqr(u, w, mm);
    fe_mul(w, u, w, mm);                          // (v-u)^3                ecm.c:1626-1629
    fe_mul(w, w, t, mm);                          // a = (v-u)^3 (3u+v)     ecm.c:1637-1638
    fe_store(S, stride, idx, w);

    Fe<NL> di, zi;                                // (16u^3v)^-1 and (v^3)^-1, or what stands for them
    uint32_t flag = 0;
    fe_mul(t, den, z3, mm);
    if (build_invert(w, t, k, mm)) {
        fe_mul(di, w, z3, mm);
        fe_mul(zi, w, den, mm);
    } else {
        if (!build_invert(di, den, k, mm)) {      // ecm.c:1745
            fe_load(di, Z, stride, idx);
            flag = 1;
        }
        if (!build_invert(zi, z3, k, mm)) {       // ecm.c:1759
            fe_load(zi, S, stride, idx);
            flag = 1;
        }
    }
    fe_load(t, S, stride, idx);
    fe_mul(t, t, di, mm);                         // b = a / 16u^3v         ecm.c:1752-1753
    fe_mul(t, t, k.one, mm);
    fe_cond_sub_n(t, k.m);
    fe_store(S, stride, idx, t);
    fe_load(t, X, stride, idx);
    fe_mul(t, t, zi, mm);                         // X = u^3 / v^3, Z = 1   ecm.c:1759-1761
    fe_mul(t, t, k.one, mm);
    fe_cond_sub_n(t, k.m);
    fe_store(X, stride, idx, t);
    fe_store(Z, stride, idx, k.one);
    flags[idx] = flag;
}

// (a macro for the reason given at GECM_STAGE1_BODY; the constants are in `k`, an S2Const<NL>, and R^2 mod N in `r2`)
#define GECM_BUILD_BODY                                                         \
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;                        \
    build_curve<NL>(sigma[idx], X, Z, S, flags, stride, idx, k, r2);

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_build(const uint64_t *__restrict__ sigma, uint32_t *__restrict__ X, uint32_t *__restrict__ Z, uint32_t *__restrict__ S,
        uint32_t *__restrict__ flags, size_t stride, S2Const<NL> k, Fe<NL> r2)
{
    GECM_BUILD_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_build_multi(const uint64_t *__restrict__ sigma, uint32_t *__restrict__ X, uint32_t *__restrict__ Z,
              uint32_t *__restrict__ S, uint32_t *__restrict__ flags, size_t stride, ModGroups<NL> groups)
{
    const GroupConst<NL> &c = mod_consts<GroupConst<NL>>(groups, blockIdx.x);
    const S2Const<NL> &k = c.k;
    const Fe<NL> &r2 = c.r2;
    GECM_BUILD_BODY
}
#undef GECM_BUILD_BODY

// ---------------------------------------------------------------- normalisation
// X <- X/Z, Z <- 1 for one curve per lane: the canonical x = X/Z mod N a standard save line holds.  X, Z come in
// canonical (every stage-1 kernel and every upload leaves them so).  z R goes through build_invert — the multiply by R
// mod N that keeps it what it is, fe_invert, the R^3 step: z^-1 R, a product (< 0.675 K) — then x R * z^-1 R / R, a
// product again, and out through the multiply by R mod N and one conditional subtraction, the tail of k_to_mont and
// k_build.  A lane whose Z has no inverse stores nothing but its flag.  Three out-of-line multiplies (ModKOut) next
// to one inversion, once per batch: small code before speed.
// (a macro for the reason given at GECM_STAGE1_BODY; the constants are in `k`, an S2Const<NL>)
#define GECM_NORMALIZE_BODY                                                     \
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;                        \
    const ModKOut<NL> mm{k.m};                                                  \
    Fe<NL> x, z, zi;                                                            \
    fe_load(z, Z, stride, idx);                                                 \
    const bool ok = build_invert(zi, z, k, mm);                                 \
    fe_load(x, X, stride, idx);                                                 \
    fe_mul(x, x, zi, mm);                                                       \
    fe_mul(x, x, k.one, mm);                                                    \
    fe_cond_sub_n(x, k.m);                                                      \
    if (ok) {                                                                   \
        fe_store(X, stride, idx, x);                                            \
        fe_store(Z, stride, idx, k.one);                                        \
    }                                                                           \
    flags[idx] = ok ? 0u : 1u;

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_normalize(uint32_t *__restrict__ X, uint32_t *__restrict__ Z, uint32_t *__restrict__ flags, size_t stride, S2Const<NL> k)
{
    GECM_NORMALIZE_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_normalize_multi(uint32_t *__restrict__ X, uint32_t *__restrict__ Z, uint32_t *__restrict__ flags, size_t stride,
                  ModGroups<NL> groups)
{
    const S2Const<NL> &k = mod_consts<S2Const<NL>>(groups, blockIdx.x);
    GECM_NORMALIZE_BODY
}
#undef GECM_NORMALIZE_BODY

#if GECM_HAS_LANE
// a modulus per lane: the same steps with the lane's constants (ModV); its multiplies are inline, the per-lane kernels
// being built for 8 to 15 limbs only
template <int NL>
__global__ void __launch_bounds__(64, 2)
k_normalize_lane(uint32_t *__restrict__ X, uint32_t *__restrict__ Z, uint32_t *__restrict__ flags, size_t stride,
                 LaneGroups<NL> g)
{
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    GECM_LANE_CONSTS
    Fe<NL> x, z, c, t, gc;
    fe_load(z, Z, stride, idx);
    fe_canonical_mont(c, z, k.one, k.m);          // canonical z R
    const bool ok = fe_invert(t, gc, c, k.m, k.inv_iters);
    fe_mul(z, t, k.r3, k.m);                      // (z R)^-1 R^3 / R = z^-1 R
    fe_load(x, X, stride, idx);
    fe_mul(x, x, z, k.m);
    fe_mul(x, x, k.one, k.m);
    fe_cond_sub_n(x, k.m);
    if (ok) {
        fe_get(t, k.one);
        fe_store(X, stride, idx, x);
        fe_store(Z, stride, idx, t);
    }
    flags[idx] = ok ? 0u : 1u;
}
#endif

#endif
#if GECM_HAS_PART(2)
// ---------------------------------------------------------------- stage 2
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_init(S2InitArgs a, S2Const<NL> k)
{
    s2_init<NL>(a, k, blockIdx.x * 64u + threadIdx.x);
}

// multi-modulus contexts run stage 2 with one sub-sequence per curve (K = 1): these four kernels are the whole path
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_init_multi(S2InitArgs a, ModGroups<NL> g)
{
    s2_init<NL>(a, mod_consts<S2Const<NL>>(g, blockIdx.x), blockIdx.x * 64u + threadIdx.x);
}

// K sub-sequences per curve (small batches): block b works on curve block b / K, sub-sequence b % K
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_init_k(S2InitArgs a, S2Const<NL> k)
{
    s2_init_k<NL>(a, k, (blockIdx.x / a.K) * 64u + threadIdx.x, blockIdx.x % a.K);
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen_k(S2PairArgs a, uint32_t first_abs, uint32_t n, S2Const<NL> k)
{
    giant_chunk_k<NL>(a, first_abs, n, k, (blockIdx.x / a.K) * 64u + threadIdx.x, blockIdx.x % a.K);
}

// giant steps [first_abs, first_abs+n): generate + normalise into the ring
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen(S2PairArgs a, uint32_t first_abs, uint32_t n, uint32_t kprev, S2Const<NL> k)
{
    giant_chunk<NL>(a, first_abs, n, first_abs == 0, k, blockIdx.x * 64u + threadIdx.x, kprev);
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen_multi(S2PairArgs a, uint32_t first_abs, uint32_t n, ModGroups<NL> g)
{
    giant_chunk<NL>(a, first_abs, n, first_abs == 0, mod_consts<S2Const<NL>>(g, blockIdx.x), blockIdx.x * 64u + threadIdx.x);
}

// pair walk over tape entries [first, first+count)
// (a macro for the reason given at GECM_STAGE1_BODY; the constants are in `k`, an S2Const<NL>)
#define GECM_S2_PAIRS_BODY                                                      \
    /* gridDim.y slices of the segment, one accumulator each (see s2_pairs) */  \
    const uint32_t per = (count + gridDim.y - 1) / gridDim.y;                   \
    const uint32_t off = blockIdx.y * per;                                      \
    if (off >= count) return;                                                   \
    const uint32_t n = count - off < per ? count - off : per;                   \
    s2_pairs<NL>(a, first + off, n, k, blockIdx.x * 64u + threadIdx.x, a.acc + (size_t)blockIdx.y * NL * a.stride);

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_pairs(S2PairArgs a, uint32_t first, uint32_t count, S2Const<NL> k)
{
    GECM_S2_PAIRS_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_pairs_multi(S2PairArgs a, uint32_t first, uint32_t count, ModGroups<NL> g)
{
    const S2Const<NL> &k = mod_consts<S2Const<NL>>(g, blockIdx.x);
    GECM_S2_PAIRS_BODY
}
#undef GECM_S2_PAIRS_BODY

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_merge(uint32_t *acc, uint32_t slices, size_t stride, int init_only,
                                                    S2Const<NL> k)
{
    s2_merge<NL>(acc, slices, stride, init_only != 0, k, blockIdx.x * 64u + threadIdx.x);
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_merge_multi(uint32_t *acc, uint32_t slices, size_t stride, int init_only,
                                                          ModGroups<NL> g)
{
    s2_merge<NL>(acc, slices, stride, init_only != 0, mod_consts<S2Const<NL>>(g, blockIdx.x), blockIdx.x * 64u + threadIdx.x);
}

#if GECM_HAS_LANE
// lane-packed multi-modulus contexts: the same four kernels with a modulus per lane (K = 1)
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_init_lane(S2InitArgs a, LaneGroups<NL> g)
{
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    GECM_LANE_CONSTS
    s2_init<NL>(a, k, idx);
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen_lane(S2PairArgs a, uint32_t first_abs, uint32_t n, LaneGroups<NL> g)
{
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    GECM_LANE_CONSTS
    giant_chunk<NL>(a, first_abs, n, first_abs == 0, k, idx);
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_pairs_lane(S2PairArgs a, uint32_t first, uint32_t count, LaneGroups<NL> g)
{
    const uint32_t per = (count + gridDim.y - 1) / gridDim.y;
    const uint32_t off = blockIdx.y * per;
    if (off >= count) return;
    const uint32_t n = count - off < per ? count - off : per;
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    GECM_LANE_CONSTS
    s2_pairs<NL>(a, first + off, n, k, idx, a.acc + (size_t)blockIdx.y * NL * a.stride);
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_merge_lane(uint32_t *acc, uint32_t slices, size_t stride, int init_only,
                                                         LaneGroups<NL> g)
{
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    GECM_LANE_CONSTS
    s2_merge<NL>(acc, slices, stride, init_only != 0, k, idx);
}
#endif

#endif
// ---------------------------------------------------------------- launchers (gecm_launch.h)
// ModArgs, ModArgsS or S2Const from the host's copy of the modulus constants
template <class A>
static A mod_args(const gecm_modconst *mc)
{
    A a;
    for (int i = 0; i < GECM_NL; i++) {
        a.m.n[i] = mc->n[i];
        a.m.kp[i] = mc->kp[i];
        a.one.v[i] = mc->one[i];
    }
    a.m.rho = mc->rho;
    return a;
}

static S2Const<GECM_NL> s2_const(const gecm_modconst *mc)
{
    S2Const<GECM_NL> k = mod_args<S2Const<GECM_NL>>(mc);
    for (int i = 0; i < GECM_NL; i++) k.r3.v[i] = mc->r3[i];
    k.inv_iters = mc->inv_iters;
    return k;
}

static ModGroups<GECM_NL> mod_groups(const gecm_modconst *mc)
{
    return ModGroups<GECM_NL>{(const GroupConst<GECM_NL> *)mc->groups, mc->block_group};
}

#if GECM_HAS_LANE
static LaneGroups<GECM_NL> lane_groups(const gecm_modconst *mc)
{
    return LaneGroups<GECM_NL>{(const GroupConst<GECM_NL> *)mc->groups, mc->curve_group};
}
#endif

#define CAT_(a, b) a##b
#define CAT(a, b) CAT_(a, b)

// the hash of the sources this object was compiled from (Makefile: K_SHA); gecm_dev.hip collects them
#ifndef GECM_MANIFEST
#define GECM_MANIFEST "unset"
#endif

#if GECM_HAS_PART(1)
// one or two lanes per curve; MOD = ModK<GECM_NL> for a generic modulus
template <class MOD>
static void launch_stage1_mod(hipStream_t stream, const gecm_modconst *mc, const uint32_t *tape, uint32_t tape_len,
                              uint32_t *X, uint32_t *Z, const uint32_t *S, size_t stride, int lanes)
{
    const dim3 grid((unsigned)(stride / (lanes == 2 ? 32 : 64))), block(64);
    if constexpr (std::is_same<MOD, ModK<GECM_NL>>::value) {
#if GECM_HAS_LANE
        if (mc->groups && mc->curve_group) {      // lane packing: one lane per curve (gecm_dev_stage1 refuses two)
            hipLaunchKernelGGL(k_stage1_lane<GECM_NL>, grid, block, 0, stream, tape, tape_len, X, Z, S, stride, lane_groups(mc));
            return;
        }
#endif
        if (mc->groups) {
            const auto g = mod_groups(mc);
            if (lanes == 2) hipLaunchKernelGGL(k_stage1_pair_multi<GECM_NL>, grid, block, 0, stream, tape, tape_len, X, Z, S, stride, g);
            else hipLaunchKernelGGL(k_stage1_multi<GECM_NL>, grid, block, 0, stream, tape, tape_len, X, Z, S, stride, g);
            return;
        }
        const auto a = mod_args<ModArgs<GECM_NL>>(mc);
        if (lanes == 2) hipLaunchKernelGGL(k_stage1_pair<GECM_NL>, grid, block, 0, stream, tape, tape_len, X, Z, S, stride, a);
        else hipLaunchKernelGGL(k_stage1<GECM_NL>, grid, block, 0, stream, tape, tape_len, X, Z, S, stride, a);
    } else {
        const auto a = mod_args<ModArgsS<GECM_NL, MOD>>(mc);
        if (lanes == 2) hipLaunchKernelGGL((k_stage1_pair_f<GECM_NL, MOD>), grid, block, 0, stream, tape, tape_len, X, Z, S, stride, a);
        else hipLaunchKernelGGL((k_stage1_f<GECM_NL, MOD>), grid, block, 0, stream, tape, tape_len, X, Z, S, stride, a);
    }
}

static void launch_stage1(void *stream, const gecm_modconst *mc, const uint32_t *tape, uint32_t tape_len, uint32_t *X,
                          uint32_t *Z, const uint32_t *S, size_t stride, const uint32_t *modq, int lanes, int form)
{
    const hipStream_t s = (hipStream_t)stream;
    if (lanes == 8)
        hipLaunchKernelGGL(k_stage1_quad<GECM_NL>, dim3((unsigned)(stride / 32)), dim3(256), 0, s, tape, tape_len, X, Z, S,   // stride: a multiple of 64
                           stride, modq, mc->rho);
    else if (form == 2) {
        if constexpr (FPolicy<GECM_NL>::NF >= 3) launch_stage1_mod<ModC<GECM_NL>>(s, mc, tape, tape_len, X, Z, S, stride, lanes);
    } else if (form > 0) launch_stage1_mod<ModF<GECM_NL>>(s, mc, tape, tape_len, X, Z, S, stride, lanes);
    else if (form < 0) launch_stage1_mod<ModP<GECM_NL>>(s, mc, tape, tape_len, X, Z, S, stride, lanes);
    else launch_stage1_mod<ModK<GECM_NL>>(s, mc, tape, tape_len, X, Z, S, stride, lanes);
}

static void launch_canon(void *stream, const gecm_modconst *mc, uint32_t *X, uint32_t *Z, size_t stride)
{
    const dim3 grid((unsigned)(stride / 64)), block(64);
    if (mc->groups)
        hipLaunchKernelGGL(k_canon_multi<GECM_NL>, grid, block, 0, (hipStream_t)stream, X, Z, stride, mod_groups(mc));
    else
        hipLaunchKernelGGL(k_canon<GECM_NL>, grid, block, 0, (hipStream_t)stream, X, Z, stride,
                           mod_args<ModArgs<GECM_NL>>(mc));
}

static void launch_from_mont(void *stream, const gecm_modconst *mc, const uint32_t *X, const uint32_t *Z, uint32_t *ox,
                             uint32_t *oz, size_t stride)
{
    const dim3 grid((unsigned)(stride / 64)), block(64);
#if GECM_HAS_LANE
    if (mc->groups && mc->curve_group) {
        hipLaunchKernelGGL(k_from_mont_lane<GECM_NL>, grid, block, 0, (hipStream_t)stream, X, Z, ox, oz, stride,
                           lane_groups(mc));
        return;
    }
#endif
    if (mc->groups)
        hipLaunchKernelGGL(k_from_mont_multi<GECM_NL>, grid, block, 0, (hipStream_t)stream, X, Z, ox, oz, stride,
                           mod_groups(mc));
    else
        hipLaunchKernelGGL(k_from_mont<GECM_NL>, grid, block, 0, (hipStream_t)stream, X, Z, ox, oz, stride,
                           mod_args<ModArgs<GECM_NL>>(mc));
}

static void launch_to_mont(void *stream, const gecm_modconst *mc, const uint32_t *ix, const uint32_t *iz, uint32_t *X,
                           uint32_t *Z, size_t stride)
{
    const dim3 grid((unsigned)(stride / 64)), block(64);
#if GECM_HAS_LANE
    if (mc->groups && mc->curve_group) {
        hipLaunchKernelGGL(k_to_mont_lane<GECM_NL>, grid, block, 0, (hipStream_t)stream, ix, iz, X, Z, stride,
                           lane_groups(mc));
        return;
    }
#endif
    if (mc->groups) {
        hipLaunchKernelGGL(k_to_mont_multi<GECM_NL>, grid, block, 0, (hipStream_t)stream, ix, iz, X, Z, stride,
                           mod_groups(mc));
        return;
    }
    Fe<GECM_NL> r2;
    for (int i = 0; i < GECM_NL; i++) r2.v[i] = mc->r2[i];
    hipLaunchKernelGGL(k_to_mont<GECM_NL>, grid, block, 0, (hipStream_t)stream, ix, iz, X, Z, stride,
                       mod_args<ModArgs<GECM_NL>>(mc), r2);
}

static void launch_l0(void *stream, const gecm_modconst *mc, int op, const uint32_t *A, const uint32_t *B, uint32_t *C,
                      uint32_t *D, size_t stride, const uint32_t *fix)
{
    Fe<GECM_NL> f;
    for (int i = 0; i < GECM_NL; i++) f.v[i] = fix[i];
    hipLaunchKernelGGL(k_l0<GECM_NL>, dim3((unsigned)(stride / 64)), dim3(64), 0, (hipStream_t)stream, op, A, B, C,
                       D, stride, mod_args<ModArgs<GECM_NL>>(mc), f);
}

static void launch_l0_inv(void *stream, const gecm_modconst *mc, const uint32_t *A, uint32_t *C, uint32_t *G, size_t stride,
                          const uint32_t *fix)
{
    Fe<GECM_NL> f;
    for (int i = 0; i < GECM_NL; i++) f.v[i] = fix[i];
    hipLaunchKernelGGL(k_l0_inv<GECM_NL>, dim3((unsigned)(stride / 64)), dim3(64), 0, (hipStream_t)stream, A, C, G, stride,
                       s2_const(mc), f);
}

static void launch_gcd_scan(void *stream, const gecm_modconst *mc, const uint32_t *V, uint32_t *G, uint32_t *flags,
                            size_t stride)
{
    const dim3 grid((unsigned)(stride / 64)), block(64);
#if GECM_HAS_LANE
    if (mc->groups && mc->curve_group) {
        hipLaunchKernelGGL(k_gcd_scan_lane<GECM_NL>, grid, block, 0, (hipStream_t)stream, V, G, flags, stride,
                           lane_groups(mc));
        return;
    }
#endif
    if (mc->groups)
        hipLaunchKernelGGL(k_gcd_scan_multi<GECM_NL>, grid, block, 0, (hipStream_t)stream, V, G, flags, stride,
                           mod_groups(mc));
    else
        hipLaunchKernelGGL(k_gcd_scan<GECM_NL>, grid, block, 0, (hipStream_t)stream, V, G, flags, stride, s2_const(mc));
}

static void launch_build(void *stream, const gecm_modconst *mc, const uint64_t *sigma, uint32_t *X, uint32_t *Z, uint32_t *S,
                         uint32_t *flags, size_t stride)
{
    const dim3 grid((unsigned)(stride / 64)), block(64);
    if (mc->groups) {
        hipLaunchKernelGGL(k_build_multi<GECM_NL>, grid, block, 0, (hipStream_t)stream, sigma, X, Z, S, flags, stride,
                           mod_groups(mc));
        return;
    }
    Fe<GECM_NL> r2;
    for (int i = 0; i < GECM_NL; i++) r2.v[i] = mc->r2[i];
    hipLaunchKernelGGL(k_build<GECM_NL>, grid, block, 0, (hipStream_t)stream, sigma, X, Z, S, flags, stride, s2_const(mc), r2);
}

static void launch_normalize(void *stream, const gecm_modconst *mc, uint32_t *X, uint32_t *Z, uint32_t *flags, size_t stride)
{
    const dim3 grid((unsigned)(stride / 64)), block(64);
#if GECM_HAS_LANE
    if (mc->groups && mc->curve_group) {
        hipLaunchKernelGGL(k_normalize_lane<GECM_NL>, grid, block, 0, (hipStream_t)stream, X, Z, flags, stride,
                           lane_groups(mc));
        return;
    }
#endif
    if (mc->groups)
        hipLaunchKernelGGL(k_normalize_multi<GECM_NL>, grid, block, 0, (hipStream_t)stream, X, Z, flags, stride,
                           mod_groups(mc));
    else
        hipLaunchKernelGGL(k_normalize<GECM_NL>, grid, block, 0, (hipStream_t)stream, X, Z, flags, stride, s2_const(mc));
}

static void pack_group(const gecm_modconst *mc, void *out)
{
    GroupConst<GECM_NL> c;
    c.k = s2_const(mc);
    for (int i = 0; i < GECM_NL; i++) c.r2.v[i] = mc->r2[i];
    memcpy(out, &c, sizeof c);
}

extern "C" const gecm_kernels_p1 *CAT(CAT(gecm_kernels_, GECM_NL), _p1)(void)
{
    static const gecm_kernels_p1 t = {launch_stage1, launch_canon, launch_from_mont, launch_to_mont, launch_l0, launch_l0_inv,
                                      launch_gcd_scan, launch_build, FPolicy<GECM_NL>::G, pack_group, sizeof(GroupConst<GECM_NL>),
                                      GECM_MANIFEST, GECM_HAS_LANE, launch_normalize};
    return &t;
}
#endif
#if GECM_HAS_PART(2)
static void launch_s2_init(void *stream, const gecm_modconst *mc, const gecm_s2_init_launch *h)
{
    const S2InitArgs &a = h->a;
    const S2Const<GECM_NL> k = s2_const(mc);
    const dim3 grid((unsigned)(a.stride / 64)), block(64);
#if GECM_HAS_LANE
    if (mc->groups && mc->curve_group) {
        const auto g = lane_groups(mc);
        hipLaunchKernelGGL(k_s2_init_lane<GECM_NL>, grid, block, 0, (hipStream_t)stream, a, g);
        if (h->slices > 1)
            hipLaunchKernelGGL(k_s2_merge_lane<GECM_NL>, grid, block, 0, (hipStream_t)stream, a.acc, h->slices, a.stride, 1, g);
        return;
    }
#endif
    if (mc->groups) {                 // K = 1 (gecm_dev_s2_init)
        const auto g = mod_groups(mc);
        hipLaunchKernelGGL(k_s2_init_multi<GECM_NL>, grid, block, 0, (hipStream_t)stream, a, g);
        if (h->slices > 1)
            hipLaunchKernelGGL(k_s2_merge_multi<GECM_NL>, grid, block, 0, (hipStream_t)stream, a.acc, h->slices, a.stride, 1, g);
        return;
    }
    if (a.K > 1)
        hipLaunchKernelGGL(k_s2_init_k<GECM_NL>, dim3((unsigned)(a.stride / 64 * a.K)), block, 0, (hipStream_t)stream, a, k);
    else
        hipLaunchKernelGGL(k_s2_init<GECM_NL>, grid, block, 0, (hipStream_t)stream, a, k);
    // the pair walk's other accumulators (slice 0 is acc itself, set by the table build)
    if (h->slices > 1)
        hipLaunchKernelGGL(k_s2_merge<GECM_NL>, grid, block, 0, (hipStream_t)stream, a.acc, h->slices, a.stride, 1, k);
}

static void launch_s2_pair(void *stream, const gecm_modconst *mc, const gecm_s2_pair_launch *h)
{
    const S2PairArgs &a = h->a;
    // the tape on the host decides the launch sequence: one k_s2_gen per "generate" mark, one
    // k_s2_pairs per run of pairs between marks (~84 + 84 launches per 1e8 range)
    const dim3 grid((unsigned)(a.stride / 64)), block(64);
    const dim3 pgrid((unsigned)(a.stride / 64), h->slices ? h->slices : 1);
    const S2Const<GECM_NL> k = s2_const(mc);
    // a "generate" mark with bit 31 set in its count is a single-chain chunk (the reference's last batch of the range,
    // gecm_stage2_pair); the others use K sub-sequences per curve when the batch is small (a.K > 1)
    const dim3 kgrid((unsigned)(a.stride / 64 * (a.K ? a.K : 1)));
    const ModGroups<GECM_NL> g = mc->groups ? mod_groups(mc) : ModGroups<GECM_NL>{};   // multi-modulus: K = 1
    uint32_t generated = 0, i = 0, kprev = 1;
    // lane packing: the same launch sequence over the per-lane kernels (built up to GECM_LANE_MAXNL limbs)
#if GECM_HAS_LANE
    const bool lane = mc->groups && mc->curve_group;
    const LaneGroups<GECM_NL> lg = lane ? lane_groups(mc) : LaneGroups<GECM_NL>{};
#define GECM_LANE_LAUNCH(...) hipLaunchKernelGGL(__VA_ARGS__)
#else
    const bool lane = false;
#define GECM_LANE_LAUNCH(...) (void)0
#endif
    while (i < a.nsteps) {
        if (h->host_steps[2 * i] == S2_STEP_GEN) {
            const uint32_t word = h->host_steps[2 * i + 1];
            const uint32_t n = word & 0x7fffffffu;
            if (lane)
                GECM_LANE_LAUNCH(k_s2_gen_lane<GECM_NL>, grid, block, 0, (hipStream_t)stream, a, generated, n, lg);
            else if (mc->groups)
                hipLaunchKernelGGL(k_s2_gen_multi<GECM_NL>, grid, block, 0, (hipStream_t)stream, a, generated, n, g);
            else if (a.K > 1 && !(word & 0x80000000u)) {
                hipLaunchKernelGGL(k_s2_gen_k<GECM_NL>, kgrid, block, 0, (hipStream_t)stream, a, generated, n, k);
                kprev = a.K;
            } else {
                hipLaunchKernelGGL(k_s2_gen<GECM_NL>, grid, block, 0, (hipStream_t)stream, a, generated, n, generated ? kprev : 1u, k);
                kprev = 1;
            }
            generated += n;
            i++;
        } else {
            uint32_t j = i;
            while (j < a.nsteps && h->host_steps[2 * j] != S2_STEP_GEN) j++;
            if (lane)
                GECM_LANE_LAUNCH(k_s2_pairs_lane<GECM_NL>, pgrid, block, 0, (hipStream_t)stream, a, i, j - i, lg);
            else if (mc->groups)
                hipLaunchKernelGGL(k_s2_pairs_multi<GECM_NL>, pgrid, block, 0, (hipStream_t)stream, a, i, j - i, g);
            else
                hipLaunchKernelGGL(k_s2_pairs<GECM_NL>, pgrid, block, 0, (hipStream_t)stream, a, i, j - i, k);
            i = j;
        }
    }
    if (h->slices > 1) {
        if (lane)
            GECM_LANE_LAUNCH(k_s2_merge_lane<GECM_NL>, grid, block, 0, (hipStream_t)stream, a.acc, h->slices, a.stride, 0, lg);
        else if (mc->groups)
            hipLaunchKernelGGL(k_s2_merge_multi<GECM_NL>, grid, block, 0, (hipStream_t)stream, a.acc, h->slices, a.stride, 0, g);
        else
            hipLaunchKernelGGL(k_s2_merge<GECM_NL>, grid, block, 0, (hipStream_t)stream, a.acc, h->slices, a.stride, 0, k);
    }
#undef GECM_LANE_LAUNCH
}

extern "C" const gecm_kernels_p2 *CAT(CAT(gecm_kernels_, GECM_NL), _p2)(void)
{
    static const gecm_kernels_p2 t = {launch_s2_init, launch_s2_pair, GECM_MANIFEST};
    return &t;
}
#endif
