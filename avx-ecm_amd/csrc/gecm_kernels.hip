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

// ---------------------------------------------------------------- constants sources, prologues, bodies
// A kernel finds the constants of its modulus in one of three places (gecm_source in gecm_launch.h):
//   by value      the kernel argument `k` is the constants: ModArgs / S2Const of a single-N launch;
//   per wavefront ModGroups `g`: one GroupConst per modulus in device memory and the modulus of every
//                 64-curve block; the multiplies read them as wave-uniform operands (the _multi kernels);
//   per lane      LaneGroups `g`: the same array and the modulus of every curve (the _lane kernels,
//                 built up to GECM_LANE_MAXNL limbs).
// The rule: one prologue per source and one body text per operation; a kernel is signature, prologue, body.  The
// prologues (GECM_ARG_CONSTS, GECM_WAVE_CONSTS, GECM_LANE_CONSTS) leave the constants in `k` and, for the two in device
// memory, R^2 mod N in `r2`; the bodies (GECM_*_BODY) read `k`, `r2` and the kernel's own arguments and use no other
// free name.  Where a variant really differs, the difference is a parameter of the body.  Prologues and bodies are
// macros, not device functions or kernel templates over the source: through a function the kernels compiled to other
// instructions (k_gcd_scan<15> 1089 -> 1064, k_stage1_multi<15> 12561 -> 12595, k_s2_pairs<26> 5906 -> 5909, k_stage1
// at the same count in another order), and the single-N kernels must stay instruction for instruction
// what they were.  Shared text costs nothing, but the order of the statements does: what a kernel computes before it
// fetches its constants (the slice of the pair walk, the flag of the merge) stays before the prologue.  After any change
// here, tools/kernel_isa_diff.py compares two builds symbol by symbol.
#define GECM_ARG_CONSTS     // by value: the kernel argument `k` is the constants (and `r2`, where the body wants it)

// One modulus's constants block in device memory: S2Const, then what only the kernels without a by-value copy of it
// need.  New fields go at the end: the kernels that read a prefix keep their offsets.
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
// per wavefront: `k` = the constants of curve block `block`, read as a T (ModArgs or S2Const, prefixes of GroupConst)
#define GECM_WAVE_CONSTS(T, block)                                              \
    const GroupConst<NL> &gk = mod_consts<GroupConst<NL>>(g, block);            \
    const T &k = *(const T *)&gk;                                               \
    [[maybe_unused]] const Fe<NL> &r2 = gk.r2;

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

// The same under a name of its own, for the sub-sequence kernels of stage 2 (k_s2_init_k_lane, k_s2_gen_k_lane).  With
// LaneConst itself they shared block_normalise<NL, LaneConst<NL>> and the lambda in it with k_s2_init_lane, which until
// then had that instance to itself, and k_s2_init_lane came out with other registers and two to nine instructions fewer
// (9770 -> 9768 at 8 limbs, 26820 -> 26811 at 15).  A type of their own gives them instances of their own.
template <int NL>
struct LaneConstK : LaneConst<NL> {
};

// And once more for the P-1 / P+1 stage-2 kernels (k_s2u_*_lane), for the same reason.
template <int NL>
struct LaneConstU : LaneConst<NL> {
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
// per lane: `k` = the constants of the curve at position `pos` (64 curves per block in every lane kernel; the
// sub-sequence kernels of stage 2 run several blocks per curve block and say which position is theirs)
#define GECM_LANE_CONSTS_AT(T, pos)                                             \
    __shared__ uint32_t lds_kp[NL * 64];                                        \
    T k;                                                                        \
    lane_consts(k, g, pos, lds_kp + threadIdx.x);                               \
    [[maybe_unused]] const FeG<NL> &r2 = k.r2;
#define GECM_LANE_CONSTS GECM_LANE_CONSTS_AT(LaneConst<NL>, blockIdx.x * 64u + threadIdx.x)

#if GECM_HAS_PART(1)
// ---------------------------------------------------------------- stage 1
// One curve per lane.  64-thread blocks (one wave): a CU holds 8 of them at 2 waves/SIMD, the
// occupancy at which v_mad_u64_u32 issues back-to-back (profiles/r01_valu_ubench_gfx950.txt).
// C_IN_LDS: the third PRAC point waits in LDS (the C store of the tape interpreter) instead of in registers.
#define GECM_STAGE1_BODY(C_IN_LDS)                                              \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Pt<NL> P;                                                                   \
    fe_load(P.X, X, stride, idx);                                               \
    fe_load(P.Z, Z, stride, idx);                                               \
    constexpr bool CL = C_IN_LDS;                                               \
    __shared__ uint32_t lds_c[CL ? 2 * NL * 64 : 1];                            \
    CStore<NL, CL> cst;                                                         \
    if constexpr (CL) cst.lds = lds_c + threadIdx.x;                            \
    run_tape<NL>(tape, tape_len, P, S, stride, idx, k.m, cst);                  \
    Fe<NL> ox, oz;                                                              \
    fe_canonical_mont(ox, P.X, k.one, k.m);                                     \
    fe_canonical_mont(oz, P.Z, k.one, k.m);                                     \
    fe_store(X, stride, idx, ox);                                               \
    fe_store(Z, stride, idx, oz);

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_stage1(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
         uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModArgs<NL> k)
{
    GECM_ARG_CONSTS
    GECM_STAGE1_BODY(TapePolicy<NL>::c_in_lds)
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_stage1_multi(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
               uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(ModArgs<NL>, blockIdx.x)
    GECM_STAGE1_BODY(TapePolicy<NL>::c_in_lds)
}

#if GECM_HAS_LANE
// A modulus per lane: the third PRAC point waits in LDS at every limb count (the column the C store of TapePolicy uses
// above its threshold): the registers it leaves hold the lane's N.
template <int NL>
__global__ void __launch_bounds__(64, 2)
k_stage1_lane(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
              uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS
    GECM_STAGE1_BODY(true)
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
           uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModArgsS<NL, MOD> k)
{
    GECM_ARG_CONSTS
    GECM_STAGE1_BODY(TapePolicy<NL>::c_in_lds)
}
#undef GECM_STAGE1_BODY

// Two lanes per curve (gecm_curve.hpp, "split-coordinate"): lane 2j works on X, lane 2j+1 on Z of
// curve blockIdx.x*32 + j.  Chosen by the device layer for batches that leave SIMDs under-occupied.
#define GECM_STAGE1_PAIR_BODY                                                   \
    const uint32_t cidx = blockIdx.x * 32u + (threadIdx.x >> 1);                \
    const bool isZ = (threadIdx.x & 1u) != 0;                                   \
    uint32_t *mine = isZ ? Z : X;                                               \
    Fe<NL> P;                                                                   \
    fe_load(P, mine, stride, cidx);                                             \
    run_tape_pair<NL>(tape, tape_len, P, S, stride, cidx, isZ, k.m);            \
    Fe<NL> o;                                                                   \
    fe_canonical_mont(o, P, k.one, k.m);                                        \
    fe_store(mine, stride, cidx, o);

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_stage1_pair(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
              uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModArgs<NL> k)
{
    GECM_ARG_CONSTS
    GECM_STAGE1_PAIR_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_stage1_pair_multi(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
                    uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(ModArgs<NL>, blockIdx.x >> 1)   // 32 curves per block
    GECM_STAGE1_PAIR_BODY
}

template <int NL, class MOD>
__global__ void __launch_bounds__(64, 2)
k_stage1_pair_f(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
                uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride, ModArgsS<NL, MOD> k)
{
    GECM_ARG_CONSTS
    GECM_STAGE1_PAIR_BODY
}
#undef GECM_STAGE1_PAIR_BODY

// One residue per lane: P-1 and P+1 stage 1 (gecm_curve.hpp, run_tape_unit).  X of position idx is the
// residue; out come its canonical Montgomery form and Z = R mod N.  pp1 != 0: P+1, else P-1 (wave-uniform).
#define GECM_UNIT_BODY                                                          \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Fe<NL> P;                                                                   \
    fe_load(P, X, stride, idx);                                                 \
    run_tape_unit<NL>(tape, tape_len, P, pp1 != 0, k.one, k.m);                 \
    Fe<NL> o;                                                                   \
    fe_canonical_mont(o, P, k.one, k.m);                                        \
    fe_store(X, stride, idx, o);                                                \
    fe_store(Z, stride, idx, k.one);

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_unit(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X, uint32_t *__restrict__ Z,
       size_t stride, uint32_t pp1, ModArgs<NL> k)
{
    GECM_ARG_CONSTS
    GECM_UNIT_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_unit_multi(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X, uint32_t *__restrict__ Z,
             size_t stride, uint32_t pp1, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(ModArgs<NL>, blockIdx.x)
    GECM_UNIT_BODY
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64, 2)
k_unit_lane(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X, uint32_t *__restrict__ Z,
            size_t stride, uint32_t pp1, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS
    GECM_UNIT_BODY
}
#endif
#undef GECM_UNIT_BODY

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
#define GECM_CANON_BODY                                                         \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Fe<NL> x, z, r;                                                             \
    fe_load(x, X, stride, idx);                                                 \
    fe_load(z, Z, stride, idx);                                                 \
    fe_canonical_mont(r, x, k.one, k.m);                                        \
    fe_store(X, stride, idx, r);                                                \
    fe_canonical_mont(r, z, k.one, k.m);                                        \
    fe_store(Z, stride, idx, r);

template <int NL>
__global__ void __launch_bounds__(64)
k_canon(uint32_t *__restrict__ X, uint32_t *__restrict__ Z, size_t stride, ModArgs<NL> k)
{
    GECM_ARG_CONSTS
    GECM_CANON_BODY
}

template <int NL>
__global__ void __launch_bounds__(64)
k_canon_multi(uint32_t *__restrict__ X, uint32_t *__restrict__ Z, size_t stride, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(ModArgs<NL>, blockIdx.x)
    GECM_CANON_BODY
}

#if GECM_HAS_LANE
// lane packing: after the 16-lane method kernel (gecm_rowk.hip, k_unit_row), the one lazy kernel that runs on it
template <int NL>
__global__ void __launch_bounds__(64)
k_canon_lane(uint32_t *__restrict__ X, uint32_t *__restrict__ Z, size_t stride, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS
    GECM_CANON_BODY
}
#endif
#undef GECM_CANON_BODY

#define GECM_FROM_MONT_BODY                                                     \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Fe<NL> x, z, r;                                                             \
    fe_load(x, X, stride, idx);                                                 \
    fe_load(z, Z, stride, idx);                                                 \
    fe_from_mont_canonical(r, x, k.m);                                          \
    fe_store(ox, stride, idx, r);                                               \
    fe_from_mont_canonical(r, z, k.m);                                          \
    fe_store(oz, stride, idx, r);

template <int NL>
__global__ void __launch_bounds__(64)
k_from_mont(const uint32_t *__restrict__ X, const uint32_t *__restrict__ Z, uint32_t *__restrict__ ox,
            uint32_t *__restrict__ oz, size_t stride, ModArgs<NL> k)
{
    GECM_ARG_CONSTS
    GECM_FROM_MONT_BODY
}

template <int NL>
__global__ void __launch_bounds__(64)
k_from_mont_multi(const uint32_t *__restrict__ X, const uint32_t *__restrict__ Z, uint32_t *__restrict__ ox,
                  uint32_t *__restrict__ oz, size_t stride, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(ModArgs<NL>, blockIdx.x)
    GECM_FROM_MONT_BODY
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64)
k_from_mont_lane(const uint32_t *__restrict__ X, const uint32_t *__restrict__ Z, uint32_t *__restrict__ ox,
                 uint32_t *__restrict__ oz, size_t stride, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS
    GECM_FROM_MONT_BODY
}
#endif
#undef GECM_FROM_MONT_BODY

// The inverse: canonical plain residues x, z in [0, N) -> X = x R mod N, Z = z R mod N, canonical, by one multiply with
// R^2 mod N each (x R^2 / R < N^2/R + N < 2N, then one conditional subtract).
#define GECM_TO_MONT_BODY                                                       \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Fe<NL> x, z, r;                                                             \
    fe_load(x, ix, stride, idx);                                                \
    fe_load(z, iz, stride, idx);                                                \
    fe_mul(r, x, r2, k.m);                                                      \
    fe_cond_sub_n(r, k.m);                                                      \
    fe_store(X, stride, idx, r);                                                \
    fe_mul(r, z, r2, k.m);                                                      \
    fe_cond_sub_n(r, k.m);                                                      \
    fe_store(Z, stride, idx, r);

template <int NL>
__global__ void __launch_bounds__(64)
k_to_mont(const uint32_t *__restrict__ ix, const uint32_t *__restrict__ iz, uint32_t *__restrict__ X,
          uint32_t *__restrict__ Z, size_t stride, ModArgs<NL> k, Fe<NL> r2)
{
    GECM_ARG_CONSTS
    GECM_TO_MONT_BODY
}

template <int NL>
__global__ void __launch_bounds__(64)
k_to_mont_multi(const uint32_t *__restrict__ ix, const uint32_t *__restrict__ iz, uint32_t *__restrict__ X,
                uint32_t *__restrict__ Z, size_t stride, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(ModArgs<NL>, blockIdx.x)
    GECM_TO_MONT_BODY
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64)
k_to_mont_lane(const uint32_t *__restrict__ ix, const uint32_t *__restrict__ iz, uint32_t *__restrict__ X,
               uint32_t *__restrict__ Z, size_t stride, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS
    GECM_TO_MONT_BODY
}
#endif
#undef GECM_TO_MONT_BODY

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

// The raw test-level operator: one field function of gecm_field.hpp on the limbs as they were uploaded — lazy operands
// at the edge of the contract, not canonical ones — and the limbs it left, with no fe_canonical_mont behind it.  MOD is
// the flavour of the multiply: ModK (generic REDC), ModF, ModP, ModC (the special forms; their fe_sub and fe_cond_sub_n
// are ModK's) by value, and ModV through the lane constants, every lane modulo its own N with K' read from LDS.  Register
// arithmetic on what was loaded: inputs outside the contract give unspecified limbs, never a fault.  Kernels of their
// own so that k_l0 and k_l0_inv stay what they were.
#define GECM_L0_RAW_BODY                                                        \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Fe<NL> x, y, r;                                                             \
    fe_load(x, A, stride, idx);                                                 \
    fe_load(y, B, stride, idx);                                                 \
    if (op == GECM_L0_MUL) fe_mul(r, x, y, k.m);                                \
    else if (op == GECM_L0_SQR) fe_sqr(r, x, k.m);                              \
    else if (op == GECM_L0_ADD) fe_add(r, x, y);                                \
    else if (op == GECM_L0_SUB) fe_sub(r, x, y, k.m);                           \
    else {                                                                      \
        r = x;                                                                  \
        fe_cond_sub_n(r, k.m);                                                  \
    }                                                                           \
    fe_store(C, stride, idx, r);

template <int NL, class MOD>
__global__ void __launch_bounds__(64)
k_l0_raw(int op, const uint32_t *__restrict__ A, const uint32_t *__restrict__ B, uint32_t *__restrict__ C, size_t stride,
         ModArgsS<NL, MOD> k)
{
    GECM_ARG_CONSTS
    GECM_L0_RAW_BODY
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64)
k_l0_raw_lane(int op, const uint32_t *__restrict__ A, const uint32_t *__restrict__ B, uint32_t *__restrict__ C, size_t stride,
              LaneGroups<NL> g)
{
    GECM_LANE_CONSTS
    GECM_L0_RAW_BODY
}
#endif
#undef GECM_L0_RAW_BODY

// ---------------------------------------------------------------- factor scan
// check_factor (ecm.c:2542-2557) for every curve on the device: g = gcd(v, N) by the same
// fixed-iteration binary algorithm the stage-2 inversion uses; flag = 1 iff 1 < g < N.
// v is any representative (Montgomery form or not: R is a power of two, N is odd).
#define GECM_GCD_SCAN_BODY                                                      \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Fe<NL> v, c, t, gcd;                                                        \
    fe_load(v, V, stride, idx);                                                 \
    GECM_GCD_SCAN_TAIL
// the scan of the value in v
#define GECM_GCD_SCAN_TAIL                                                      \
    fe_canonical_mont(c, v, k.one, k.m);                                        \
    fe_invert(t, gcd, c, k.m, k.inv_iters);                                     \
    bool is_one = gcd.v[0] == 1u, is_n = true;                                  \
    _Pragma("unroll")                                                           \
    for (int i = 0; i < NL; i++) {                                              \
        if (i > 0) is_one = is_one && gcd.v[i] == 0;                            \
        is_n = is_n && gcd.v[i] == k.m.n[i];                                    \
    }                                                                           \
    fe_store(G, stride, idx, gcd);                                              \
    flags[idx] = (!is_one && !is_n) ? 1u : 0u;

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_gcd_scan(const uint32_t *__restrict__ V, uint32_t *__restrict__ G, uint32_t *__restrict__ flags, size_t stride,
           S2Const<NL> k)
{
    GECM_ARG_CONSTS
    GECM_GCD_SCAN_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_gcd_scan_multi(const uint32_t *__restrict__ V, uint32_t *__restrict__ G, uint32_t *__restrict__ flags, size_t stride,
                 ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2Const<NL>, blockIdx.x)
    GECM_GCD_SCAN_BODY
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64, 2)
k_gcd_scan_lane(const uint32_t *__restrict__ V, uint32_t *__restrict__ G, uint32_t *__restrict__ flags, size_t stride,
                LaneGroups<NL> g)
{
    GECM_LANE_CONSTS
    GECM_GCD_SCAN_BODY
}
#endif
#undef GECM_GCD_SCAN_BODY

// The scan of a P-1 / P+1 batch: v = X - c R mod N for c = off = 1 or 2 (X canonical, Montgomery form:
// the residue x of the method, so v stands for x - 1 or x - 2), then the same scan.  Kernels of their own: k_gcd_scan*
// keep their code.
#define GECM_GCD_SCAN_OFF_BODY                                                  \
    uint32_t idx = blockIdx.x * 64u + threadIdx.x;                              \
    Fe<NL> v, c, t, gcd;                                                        \
    fe_load(c, V, stride, idx);                                                 \
    unit_const(t, k.one, off == 2u, k.m);                                       \
    fe_sub(v, c, t, k.m);                                                       \
    GECM_GCD_SCAN_TAIL

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_gcd_scan_off(const uint32_t *__restrict__ V, uint32_t *__restrict__ G, uint32_t *__restrict__ flags, size_t stride,
               uint32_t off, S2Const<NL> k)
{
    GECM_ARG_CONSTS
    GECM_GCD_SCAN_OFF_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_gcd_scan_off_multi(const uint32_t *__restrict__ V, uint32_t *__restrict__ G, uint32_t *__restrict__ flags, size_t stride,
                     uint32_t off, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2Const<NL>, blockIdx.x)
    GECM_GCD_SCAN_OFF_BODY
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64, 2)
k_gcd_scan_off_lane(const uint32_t *__restrict__ V, uint32_t *__restrict__ G, uint32_t *__restrict__ flags, size_t stride,
                    uint32_t off, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS
    GECM_GCD_SCAN_OFF_BODY
}
#endif
#undef GECM_GCD_SCAN_OFF_BODY
#undef GECM_GCD_SCAN_TAIL

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

#define GECM_BUILD_BODY                                                         \
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;                        \
    build_curve<NL>(sigma[idx], X, Z, S, flags, stride, idx, k, r2);

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_build(const uint64_t *__restrict__ sigma, uint32_t *__restrict__ X, uint32_t *__restrict__ Z, uint32_t *__restrict__ S,
        uint32_t *__restrict__ flags, size_t stride, S2Const<NL> k, Fe<NL> r2)
{
    GECM_ARG_CONSTS
    GECM_BUILD_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_build_multi(const uint64_t *__restrict__ sigma, uint32_t *__restrict__ X, uint32_t *__restrict__ Z, uint32_t *__restrict__ S,
              uint32_t *__restrict__ flags, size_t stride, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2Const<NL>, blockIdx.x)
    GECM_BUILD_BODY
}
#undef GECM_BUILD_BODY

// GMP-ECM's PARAM 1 and PARAM 3 curves: B y^2 = x^3 + A x^2 + x with (A+2)/4 = d and the start point
// (2 : 1), d = sigma^2 / 2^64 (PARAM 1) or sigma / 2^32 (PARAM 3) modulo N.  One curve per lane; a lane whose parameter is
// 0 (a Suyama curve of a mixed batch, which k_build has made, or padding) stores nothing.  No inversion: the division is
// one Montgomery multiply a b / R with b = R / 2^w = 2^(28 NL - w), a single bit of a single limb — limb NL - 3, bit 20
// for w = 64 and limb NL - 2, bit 24 for w = 32 — which lies below 2^(28 NL - 5) <= K and so is an operand as it stands,
// like sigma's own three limbs and the small constants of build_curve.  sigma R and sigma^2 R are products (< 0.675 K);
// S and X = 2 R leave through the multiply by R mod N and one conditional subtraction, the tail of k_build; Z = R mod N.
// The out-of-line multiplies (ModKOut), as in k_build: five of them, once per batch.
template <int NL>
__device__ __forceinline__ void fe_param_shift(Fe<NL> &r, uint32_t prm)
{
#pragma unroll
    for (int i = 0; i < NL; i++)
        r.v[i] = (i == NL - 3 && prm == 1u) ? 1u << 20 : (i == NL - 2 && prm != 1u) ? 1u << 24 : 0u;
}

#define GECM_BUILD_PARAM_BODY                                                   \
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;                        \
    const uint32_t prm = param[idx];                                            \
    if (prm != 0) {                                                             \
        static_assert(NL >= 3, "sigma takes three limbs");                      \
        const ModKOut<NL> mm{k.m};                                              \
        const uint64_t sg = sigma[idx];                                         \
        Fe<NL> t, w;                                                            \
        fe_small(t, (uint32_t)sg & GECM_LIMB_MASK);                             \
        t.v[1] = (uint32_t)(sg >> GECM_LIMB_BITS) & GECM_LIMB_MASK;             \
        t.v[2] = (uint32_t)(sg >> (2 * GECM_LIMB_BITS));                        \
        fe_mul(w, t, r2, mm);                         /* sigma R */             \
        if (prm == 1) fe_sqr(w, w, mm);               /* sigma^2 R */           \
        fe_param_shift(t, prm);                       /* R / 2^w */             \
        fe_mul(w, w, t, mm);                          /* d R */                 \
        fe_mul(w, w, k.one, mm);                                                \
        fe_cond_sub_n(w, k.m);                                                  \
        fe_store(S, stride, idx, w);                                            \
        fe_small(t, 2u);                                                        \
        fe_mul(t, t, r2, mm);                                                   \
        fe_mul(t, t, k.one, mm);                                                \
        fe_cond_sub_n(t, k.m);                                                  \
        fe_store(X, stride, idx, t);                                            \
        fe_store(Z, stride, idx, k.one);                                        \
        flags[idx] = 0u;                                                        \
    }

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_build_param(const uint64_t *__restrict__ sigma, const uint8_t *__restrict__ param, uint32_t *__restrict__ X,
              uint32_t *__restrict__ Z, uint32_t *__restrict__ S, uint32_t *__restrict__ flags, size_t stride, ModArgs<NL> k,
              Fe<NL> r2)
{
    GECM_ARG_CONSTS
    GECM_BUILD_PARAM_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_build_param_multi(const uint64_t *__restrict__ sigma, const uint8_t *__restrict__ param, uint32_t *__restrict__ X,
                    uint32_t *__restrict__ Z, uint32_t *__restrict__ S, uint32_t *__restrict__ flags, size_t stride,
                    ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(ModArgs<NL>, blockIdx.x)
    GECM_BUILD_PARAM_BODY
}
#undef GECM_BUILD_PARAM_BODY

// ---------------------------------------------------------------- normalisation
// X <- X/Z, Z <- 1 for one curve per lane: the canonical x = X/Z mod N a standard save line holds.  X, Z come in
// canonical (every stage-1 kernel and every upload leaves them so).  z R goes through build_invert — the multiply by R
// mod N that keeps it what it is, fe_invert, the R^3 step: z^-1 R, a product (< 0.675 K) — then x R * z^-1 R / R, a
// product again, and out through the multiply by R mod N and one conditional subtraction, the tail of k_to_mont and
// k_build.  A lane whose Z has no inverse stores nothing but its flag.  Three out-of-line multiplies (ModKOut) next
// to one inversion, once per batch: small code before speed.
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
    GECM_ARG_CONSTS
    GECM_NORMALIZE_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2)
k_normalize_multi(uint32_t *__restrict__ X, uint32_t *__restrict__ Z, uint32_t *__restrict__ flags, size_t stride,
                  ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2Const<NL>, blockIdx.x)
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
// Multi-modulus contexts run stage 2 with one sub-sequence per curve (K = 1) unless they ask for more
// (gecm_set_stage2_subseq): at K = 1 the _multi or _lane kernels of init, gen, pairs and merge are the
// whole path; at K > 1 init and gen go through the _k_multi / _k_lane kernels and the plain-chain chunks through
// k_s2_gen_after_k_*.
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_init(S2InitArgs a, S2Const<NL> k)
{
    GECM_ARG_CONSTS
    s2_init<NL>(a, k, blockIdx.x * 64u + threadIdx.x);
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_init_multi(S2InitArgs a, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2Const<NL>, blockIdx.x)
    s2_init<NL>(a, k, blockIdx.x * 64u + threadIdx.x);
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_init_lane(S2InitArgs a, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS
    s2_init<NL>(a, k, blockIdx.x * 64u + threadIdx.x);
}
#endif

// K sub-sequences per curve (small batches): block b works on curve block b / K, sub-sequence b % K; the constants of
// a launch that keeps them in device memory are those of curve block b / K
#define GECM_S2_INIT_K_BODY                                                     \
    s2_init_k<NL>(a, k, (blockIdx.x / a.K) * 64u + threadIdx.x, blockIdx.x % a.K);
#define GECM_S2_GEN_K_BODY                                                      \
    giant_chunk_k<NL>(a, first_abs, n, k, (blockIdx.x / a.K) * 64u + threadIdx.x, blockIdx.x % a.K);

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_init_k(S2InitArgs a, S2Const<NL> k)
{
    GECM_ARG_CONSTS
    GECM_S2_INIT_K_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_init_k_multi(S2InitArgs a, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2Const<NL>, blockIdx.x / a.K)
    GECM_S2_INIT_K_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen_k(S2PairArgs a, uint32_t first_abs, uint32_t n, S2Const<NL> k)
{
    GECM_ARG_CONSTS
    GECM_S2_GEN_K_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen_k_multi(S2PairArgs a, uint32_t first_abs, uint32_t n, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2Const<NL>, blockIdx.x / a.K)
    GECM_S2_GEN_K_BODY
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_init_k_lane(S2InitArgs a, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS_AT(LaneConstK<NL>, (blockIdx.x / a.K) * 64u + threadIdx.x)
    GECM_S2_INIT_K_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen_k_lane(S2PairArgs a, uint32_t first_abs, uint32_t n, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS_AT(LaneConstK<NL>, (blockIdx.x / a.K) * 64u + threadIdx.x)
    GECM_S2_GEN_K_BODY
}
#endif
#undef GECM_S2_INIT_K_BODY
#undef GECM_S2_GEN_K_BODY

// giant steps [first_abs, first_abs+n): generate + normalise into the ring
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen(S2PairArgs a, uint32_t first_abs, uint32_t n, uint32_t kprev, S2Const<NL> k)
{
    GECM_ARG_CONSTS
    giant_chunk<NL>(a, first_abs, n, first_abs == 0, k, blockIdx.x * 64u + threadIdx.x, kprev);
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen_multi(S2PairArgs a, uint32_t first_abs, uint32_t n, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2Const<NL>, blockIdx.x)
    giant_chunk<NL>(a, first_abs, n, first_abs == 0, k, blockIdx.x * 64u + threadIdx.x);
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen_lane(S2PairArgs a, uint32_t first_abs, uint32_t n, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS
    giant_chunk<NL>(a, first_abs, n, first_abs == 0, k, blockIdx.x * 64u + threadIdx.x);
}
#endif

// The plain-chain chunks of a multi-modulus launch with sub-sequences (the last chunk of a range, and every chunk when
// amin = 0): they take the two steps before first_abs from the sub-sequences' scratch when kprev > 1, as k_s2_gen does.
// Kernels of their own: k_s2_gen_multi and k_s2_gen_lane keep their signatures and their code.
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen_after_k_multi(S2PairArgs a, uint32_t first_abs, uint32_t n, uint32_t kprev,
                                                                ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2Const<NL>, blockIdx.x)
    giant_chunk<NL>(a, first_abs, n, first_abs == 0, k, blockIdx.x * 64u + threadIdx.x, kprev);
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_gen_after_k_lane(S2PairArgs a, uint32_t first_abs, uint32_t n, uint32_t kprev,
                                                               LaneGroups<NL> g)
{
    GECM_LANE_CONSTS
    giant_chunk<NL>(a, first_abs, n, first_abs == 0, k, blockIdx.x * 64u + threadIdx.x, kprev);
}
#endif

// pair walk over tape entries [first, first+count): gridDim.y slices of the segment, one accumulator each (see s2_pairs)
// (a lane fetches its constants after the slice's early return, a wavefront before it)
#define GECM_S2_SLICE                                                           \
    const uint32_t per = (count + gridDim.y - 1) / gridDim.y;                   \
    const uint32_t off = blockIdx.y * per;                                      \
    if (off >= count) return;                                                   \
    const uint32_t n = count - off < per ? count - off : per;
#define GECM_S2_PAIRS_BODY                                                      \
    s2_pairs<NL>(a, first + off, n, k, blockIdx.x * 64u + threadIdx.x, a.acc + (size_t)blockIdx.y * NL * a.stride);

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_pairs(S2PairArgs a, uint32_t first, uint32_t count, S2Const<NL> k)
{
    GECM_ARG_CONSTS
    GECM_S2_SLICE
    GECM_S2_PAIRS_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_pairs_multi(S2PairArgs a, uint32_t first, uint32_t count, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2Const<NL>, blockIdx.x)
    GECM_S2_SLICE
    GECM_S2_PAIRS_BODY
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_pairs_lane(S2PairArgs a, uint32_t first, uint32_t count, LaneGroups<NL> g)
{
    GECM_S2_SLICE
    GECM_LANE_CONSTS
    GECM_S2_PAIRS_BODY
}
#endif
#undef GECM_S2_SLICE
#undef GECM_S2_PAIRS_BODY

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_merge(uint32_t *acc, uint32_t slices, size_t stride, int init_only,
                                                    S2Const<NL> k)
{
    const bool init = init_only != 0;
    GECM_ARG_CONSTS
    s2_merge<NL>(acc, slices, stride, init, k, blockIdx.x * 64u + threadIdx.x);
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_merge_multi(uint32_t *acc, uint32_t slices, size_t stride, int init_only,
                                                          ModGroups<NL> g)
{
    const bool init = init_only != 0;
    GECM_WAVE_CONSTS(S2Const<NL>, blockIdx.x)
    s2_merge<NL>(acc, slices, stride, init, k, blockIdx.x * 64u + threadIdx.x);
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2_merge_lane(uint32_t *acc, uint32_t slices, size_t stride, int init_only,
                                                         LaneGroups<NL> g)
{
    const bool init = init_only != 0;
    GECM_LANE_CONSTS
    s2_merge<NL>(acc, slices, stride, init, k, blockIdx.x * 64u + threadIdx.x);
}
#endif

// ---------------------------------------------------------------- stage 2 of P-1 and P+1
// The table and the giant steps of a method batch (gecm_stage2.hpp, s2u_*); the pair walk and the merge are the kernels
// above.  The by-value kernels read their S2Const argument under the name S2ConstU.
#define GECM_ARG_CONSTS_U const S2ConstU<NL> &k = *(const S2ConstU<NL> *)&kv;
// P of every position into S (pm1 != 0: P-1, else P+1; wave-uniform), acc = one: one thread per position
#define GECM_S2U_SEED_BODY                                                      \
    s2u_seed<NL>(X, S, acc, fail, stride, pm1 != 0, k, blockIdx.x * 64u + threadIdx.x);
// K sub-sequences per position, K >= 1: block b works on position block b / K, sub-sequence b % K
#define GECM_S2U_INIT_BODY                                                      \
    s2u_init<NL>(a, k, (blockIdx.x / a.K) * 64u + threadIdx.x, blockIdx.x % a.K);
#define GECM_S2U_GEN_BODY                                                       \
    s2u_gen<NL>(a, first_abs, n, k, (blockIdx.x / a.K) * 64u + threadIdx.x, blockIdx.x % a.K);

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2u_seed(const uint32_t *__restrict__ X, uint32_t *__restrict__ S,
                                                    uint32_t *__restrict__ acc, uint32_t *__restrict__ fail, size_t stride,
                                                    uint32_t pm1, S2Const<NL> kv)
{
    GECM_ARG_CONSTS_U
    GECM_S2U_SEED_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2u_seed_multi(const uint32_t *__restrict__ X, uint32_t *__restrict__ S,
                                                          uint32_t *__restrict__ acc, uint32_t *__restrict__ fail,
                                                          size_t stride, uint32_t pm1, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2ConstU<NL>, blockIdx.x)
    GECM_S2U_SEED_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2u_init(S2InitArgs a, S2Const<NL> kv)
{
    GECM_ARG_CONSTS_U
    GECM_S2U_INIT_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2u_init_multi(S2InitArgs a, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2ConstU<NL>, blockIdx.x / a.K)
    GECM_S2U_INIT_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2u_gen(S2PairArgs a, uint32_t first_abs, uint32_t n, S2Const<NL> kv)
{
    GECM_ARG_CONSTS_U
    GECM_S2U_GEN_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2u_gen_multi(S2PairArgs a, uint32_t first_abs, uint32_t n, ModGroups<NL> g)
{
    GECM_WAVE_CONSTS(S2ConstU<NL>, blockIdx.x / a.K)
    GECM_S2U_GEN_BODY
}

#if GECM_HAS_LANE
template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2u_seed_lane(const uint32_t *__restrict__ X, uint32_t *__restrict__ S,
                                                         uint32_t *__restrict__ acc, uint32_t *__restrict__ fail,
                                                         size_t stride, uint32_t pm1, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS_AT(LaneConstU<NL>, blockIdx.x * 64u + threadIdx.x)
    GECM_S2U_SEED_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2u_init_lane(S2InitArgs a, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS_AT(LaneConstU<NL>, (blockIdx.x / a.K) * 64u + threadIdx.x)
    GECM_S2U_INIT_BODY
}

template <int NL>
__global__ void __launch_bounds__(64, 2) k_s2u_gen_lane(S2PairArgs a, uint32_t first_abs, uint32_t n, LaneGroups<NL> g)
{
    GECM_LANE_CONSTS_AT(LaneConstU<NL>, (blockIdx.x / a.K) * 64u + threadIdx.x)
    GECM_S2U_GEN_BODY
}
#endif
#undef GECM_ARG_CONSTS_U
#undef GECM_S2U_SEED_BODY
#undef GECM_S2U_INIT_BODY
#undef GECM_S2U_GEN_BODY

#endif
// ---------------------------------------------------------------- launchers (gecm_launch.h)
// ModArgs, ModArgsS or S2Const from the host's record of the modulus constants
template <class A>
static A mod_args(const gecm_devmod *m)
{
    A a;
    for (int i = 0; i < GECM_NL; i++) {
        a.m.n[i] = m->n[i];
        a.m.kp[i] = m->kp[i];
        a.one.v[i] = m->one[i];
    }
    a.m.rho = m->rho;
    return a;
}

// m->r3 is not NULL here: the device layer lets no operation that inverts reach a launcher without it (ready() and
// gecm_dev_l0_inv in gecm_dev.hip; gecm_dev_set_groups for pack_group)
static S2Const<GECM_NL> s2_const(const gecm_devmod *m)
{
    S2Const<GECM_NL> k = mod_args<S2Const<GECM_NL>>(m);
    for (int i = 0; i < GECM_NL; i++) k.r3.v[i] = m->r3[i];
    k.inv_iters = m->inv_iters;
    return k;
}

// the R^2 mod N of a single-modulus launch (to_mont, build)
static Fe<GECM_NL> r2_const(const gecm_devmod *m)
{
    Fe<GECM_NL> r2;
    for (int i = 0; i < GECM_NL; i++) r2.v[i] = m->r2[i];
    return r2;
}

// a by-value kernel's constants argument of type V
template <class V>
static V by_value(const gecm_devmod *m)
{
    if constexpr (std::is_same<V, Fe<GECM_NL>>::value) return r2_const(m);
    else if constexpr (std::is_same<V, S2Const<GECM_NL>>::value) return s2_const(m);
    else return mod_args<V>(m);
}

// The one place that picks a kernel by the constants source of the launch (mc->source, set by the device layer): the
// by-value kernel `kv`, whose last arguments are the V..., its per-wavefront twin `kw` or its per-lane twin `kl`, on
// 64-thread blocks with the arguments `c...` they have in common.  nullptr stands for a twin that does not exist; a
// launch whose source has none goes to the next in that order, as it always has (the device layer refuses such
// launches before they get here).  GECM_LANE names a per-lane kernel where they are built, and nothing above
// GECM_LANE_MAXNL limbs.
#if GECM_HAS_LANE
#define GECM_LANE(kernel) kernel<GECM_NL>
#else
#define GECM_LANE(kernel) nullptr
#endif
template <class KT>
static constexpr bool has_kernel = !std::is_same<KT, std::nullptr_t>::value;

template <class... V, class KV, class KW, class KL, class... C>
static void launch_by_source(void *stream, const gecm_modconst *mc, dim3 grid, KV kv, KW kw, KL kl, const C &...c)
{
    const hipStream_t s = (hipStream_t)stream;
    const dim3 block(64);
    const auto *groups = (const GroupConst<GECM_NL> *)mc->groups;
    if constexpr (has_kernel<KL>)
        if (mc->source == GECM_SRC_LANE) {
            hipLaunchKernelGGL(kl, grid, block, 0, s, c..., LaneGroups<GECM_NL>{groups, mc->curve_group});
            return;
        }
    if constexpr (has_kernel<KW>)
        if (mc->source != GECM_SRC_VALUE) {
            hipLaunchKernelGGL(kw, grid, block, 0, s, c..., ModGroups<GECM_NL>{groups, mc->block_group});
            return;
        }
    if constexpr (has_kernel<KV>) hipLaunchKernelGGL(kv, grid, block, 0, s, c..., by_value<V>(&mc->m)...);
}

// one 64-thread block per 64 curves
static dim3 blocks_of(size_t stride) { return dim3((unsigned)(stride / 64)); }

#define CAT_(a, b) a##b
#define CAT(a, b) CAT_(a, b)

// the hash of the sources this object was compiled from (Makefile: K_SHA); gecm_dev.hip collects them
#ifndef GECM_MANIFEST
#define GECM_MANIFEST "unset"
#endif

#if GECM_HAS_PART(1)
// one or two lanes per curve; MOD = ModK<GECM_NL> for a generic modulus, which alone has multi-modulus kernels (and
// per-lane ones with one lane per curve: gecm_dev_stage1 refuses two)
template <class MOD>
static void launch_stage1_mod(void *stream, const gecm_modconst *mc, const uint32_t *tape, uint32_t tape_len, uint32_t *X,
                              uint32_t *Z, const uint32_t *S, size_t stride, int lanes)
{
    const dim3 grid((unsigned)(stride / (lanes == 2 ? 32 : 64)));
    if constexpr (std::is_same<MOD, ModK<GECM_NL>>::value) {
        if (lanes == 2)
            launch_by_source<ModArgs<GECM_NL>>(stream, mc, grid, k_stage1_pair<GECM_NL>, k_stage1_pair_multi<GECM_NL>, nullptr,
                                               tape, tape_len, X, Z, S, stride);
        else
            launch_by_source<ModArgs<GECM_NL>>(stream, mc, grid, k_stage1<GECM_NL>, k_stage1_multi<GECM_NL>,
                                               GECM_LANE(k_stage1_lane), tape, tape_len, X, Z, S, stride);
    } else if (lanes == 2)
        launch_by_source<ModArgsS<GECM_NL, MOD>>(stream, mc, grid, k_stage1_pair_f<GECM_NL, MOD>, nullptr, nullptr, tape,
                                                 tape_len, X, Z, S, stride);
    else
        launch_by_source<ModArgsS<GECM_NL, MOD>>(stream, mc, grid, k_stage1_f<GECM_NL, MOD>, nullptr, nullptr, tape, tape_len,
                                                 X, Z, S, stride);
}

static void launch_stage1(void *stream, const gecm_modconst *mc, const uint32_t *tape, uint32_t tape_len, uint32_t *X,
                          uint32_t *Z, const uint32_t *S, size_t stride, const uint32_t *modq, int lanes, int form)
{
    if (lanes == 8)
        hipLaunchKernelGGL(k_stage1_quad<GECM_NL>, dim3((unsigned)(stride / 32)), dim3(256), 0, (hipStream_t)stream, tape,
                           tape_len, X, Z, S, stride, modq, mc->m.rho);   // stride: a multiple of 64
    else if (form == 2) {
        if constexpr (FPolicy<GECM_NL>::NF >= 3) launch_stage1_mod<ModC<GECM_NL>>(stream, mc, tape, tape_len, X, Z, S, stride, lanes);
    } else if (form > 0) launch_stage1_mod<ModF<GECM_NL>>(stream, mc, tape, tape_len, X, Z, S, stride, lanes);
    else if (form < 0) launch_stage1_mod<ModP<GECM_NL>>(stream, mc, tape, tape_len, X, Z, S, stride, lanes);
    else launch_stage1_mod<ModK<GECM_NL>>(stream, mc, tape, tape_len, X, Z, S, stride, lanes);
}

static void launch_canon(void *stream, const gecm_modconst *mc, uint32_t *X, uint32_t *Z, size_t stride)
{
    launch_by_source<ModArgs<GECM_NL>>(stream, mc, blocks_of(stride), k_canon<GECM_NL>, k_canon_multi<GECM_NL>,
                                       GECM_LANE(k_canon_lane), X, Z, stride);
}

static void launch_from_mont(void *stream, const gecm_modconst *mc, const uint32_t *X, const uint32_t *Z, uint32_t *ox,
                             uint32_t *oz, size_t stride)
{
    launch_by_source<ModArgs<GECM_NL>>(stream, mc, blocks_of(stride), k_from_mont<GECM_NL>, k_from_mont_multi<GECM_NL>,
                                       GECM_LANE(k_from_mont_lane), X, Z, ox, oz, stride);
}

static void launch_to_mont(void *stream, const gecm_modconst *mc, const uint32_t *ix, const uint32_t *iz, uint32_t *X,
                           uint32_t *Z, size_t stride)
{
    launch_by_source<ModArgs<GECM_NL>, Fe<GECM_NL>>(stream, mc, blocks_of(stride), k_to_mont<GECM_NL>, k_to_mont_multi<GECM_NL>,
                                                    GECM_LANE(k_to_mont_lane), ix, iz, X, Z, stride);
}

static void launch_l0(void *stream, const gecm_modconst *mc, int op, const uint32_t *A, const uint32_t *B, uint32_t *C,
                      uint32_t *D, size_t stride, const uint32_t *fix)
{
    Fe<GECM_NL> f;
    for (int i = 0; i < GECM_NL; i++) f.v[i] = fix[i];
    hipLaunchKernelGGL(k_l0<GECM_NL>, dim3((unsigned)(stride / 64)), dim3(64), 0, (hipStream_t)stream, op, A, B, C,
                       D, stride, mod_args<ModArgs<GECM_NL>>(&mc->m), f);
}

static void launch_l0_inv(void *stream, const gecm_modconst *mc, const uint32_t *A, uint32_t *C, uint32_t *G, size_t stride,
                          const uint32_t *fix)
{
    Fe<GECM_NL> f;
    for (int i = 0; i < GECM_NL; i++) f.v[i] = fix[i];
    hipLaunchKernelGGL(k_l0_inv<GECM_NL>, dim3((unsigned)(stride / 64)), dim3(64), 0, (hipStream_t)stream, A, C, G, stride,
                       s2_const(&mc->m), f);
}

// form as for stage1 (0: generic REDC, which alone has a per-lane twin; +1, -1, 2: the special multiplies, by value)
template <class MOD>
static void launch_l0_raw_mod(void *stream, const gecm_modconst *mc, int op, const uint32_t *A, const uint32_t *B, uint32_t *C,
                              size_t stride)
{
    if constexpr (std::is_same<MOD, ModK<GECM_NL>>::value)
        launch_by_source<ModArgsS<GECM_NL, MOD>>(stream, mc, blocks_of(stride), k_l0_raw<GECM_NL, MOD>, nullptr,
                                                 GECM_LANE(k_l0_raw_lane), op, A, B, C, stride);
    else
        launch_by_source<ModArgsS<GECM_NL, MOD>>(stream, mc, blocks_of(stride), k_l0_raw<GECM_NL, MOD>, nullptr, nullptr, op, A,
                                                 B, C, stride);
}

static void launch_l0_raw(void *stream, const gecm_modconst *mc, int op, int form, const uint32_t *A, const uint32_t *B,
                          uint32_t *C, size_t stride)
{
    if (form == 2) {
        if constexpr (FPolicy<GECM_NL>::NF >= 3) launch_l0_raw_mod<ModC<GECM_NL>>(stream, mc, op, A, B, C, stride);
    } else if (form > 0) launch_l0_raw_mod<ModF<GECM_NL>>(stream, mc, op, A, B, C, stride);
    else if (form < 0) launch_l0_raw_mod<ModP<GECM_NL>>(stream, mc, op, A, B, C, stride);
    else launch_l0_raw_mod<ModK<GECM_NL>>(stream, mc, op, A, B, C, stride);
}

static void launch_gcd_scan(void *stream, const gecm_modconst *mc, const uint32_t *V, uint32_t *G, uint32_t *flags,
                            size_t stride)
{
    launch_by_source<S2Const<GECM_NL>>(stream, mc, blocks_of(stride), k_gcd_scan<GECM_NL>, k_gcd_scan_multi<GECM_NL>,
                                       GECM_LANE(k_gcd_scan_lane), V, G, flags, stride);
}

static void launch_build(void *stream, const gecm_modconst *mc, const uint64_t *sigma, uint32_t *X, uint32_t *Z, uint32_t *S,
                         uint32_t *flags, size_t stride)
{
    launch_by_source<S2Const<GECM_NL>, Fe<GECM_NL>>(stream, mc, blocks_of(stride), k_build<GECM_NL>, k_build_multi<GECM_NL>,
                                                    nullptr, sigma, X, Z, S, flags, stride);
}

static void launch_normalize(void *stream, const gecm_modconst *mc, uint32_t *X, uint32_t *Z, uint32_t *flags, size_t stride)
{
    launch_by_source<S2Const<GECM_NL>>(stream, mc, blocks_of(stride), k_normalize<GECM_NL>, k_normalize_multi<GECM_NL>,
                                       GECM_LANE(k_normalize_lane), X, Z, flags, stride);
}

static void launch_build_param(void *stream, const gecm_modconst *mc, const uint64_t *sigma, const uint8_t *param, uint32_t *X,
                               uint32_t *Z, uint32_t *S, uint32_t *flags, size_t stride)
{
    launch_by_source<ModArgs<GECM_NL>, Fe<GECM_NL>>(stream, mc, blocks_of(stride), k_build_param<GECM_NL>,
                                                    k_build_param_multi<GECM_NL>, nullptr, sigma, param, X, Z, S, flags, stride);
}

static void launch_stage1_unit(void *stream, const gecm_modconst *mc, const uint32_t *tape, uint32_t tape_len, uint32_t *X,
                               uint32_t *Z, size_t stride, int pp1)
{
    launch_by_source<ModArgs<GECM_NL>>(stream, mc, blocks_of(stride), k_unit<GECM_NL>, k_unit_multi<GECM_NL>,
                                       GECM_LANE(k_unit_lane), tape, tape_len, X, Z, stride, (uint32_t)(pp1 != 0));
}

static void launch_gcd_scan_off(void *stream, const gecm_modconst *mc, const uint32_t *V, uint32_t *G, uint32_t *flags,
                                size_t stride, uint32_t off)
{
    launch_by_source<S2Const<GECM_NL>>(stream, mc, blocks_of(stride), k_gcd_scan_off<GECM_NL>, k_gcd_scan_off_multi<GECM_NL>,
                                       GECM_LANE(k_gcd_scan_off_lane), V, G, flags, stride, off);
}

static void pack_group(const gecm_devmod *m, void *out)
{
    const GroupConst<GECM_NL> c = {s2_const(m), r2_const(m)};
    memcpy(out, &c, sizeof c);
}

extern "C" const gecm_kernels_p1 *CAT(CAT(gecm_kernels_, GECM_NL), _p1)(void)
{
    static const gecm_kernels_p1 t = {launch_stage1, launch_canon, launch_from_mont, launch_to_mont, launch_l0, launch_l0_inv,
                                      launch_gcd_scan, launch_build, FPolicy<GECM_NL>::G, pack_group, sizeof(GroupConst<GECM_NL>),
                                      GECM_MANIFEST, GECM_HAS_LANE, launch_normalize, launch_build_param,
                                      launch_stage1_unit, launch_gcd_scan_off, launch_l0_raw};
    return &t;
}
#endif
#if GECM_HAS_PART(2)
static void launch_s2_init(void *stream, const gecm_modconst *mc, const gecm_s2_init_launch *h)
{
    const S2InitArgs &a = h->a;
    const dim3 grid = blocks_of(a.stride);
    if (a.K > 1)
        launch_by_source<S2Const<GECM_NL>>(stream, mc, blocks_of(a.stride * a.K), k_s2_init_k<GECM_NL>,
                                           k_s2_init_k_multi<GECM_NL>, GECM_LANE(k_s2_init_k_lane), a);
    else
        launch_by_source<S2Const<GECM_NL>>(stream, mc, grid, k_s2_init<GECM_NL>, k_s2_init_multi<GECM_NL>,
                                           GECM_LANE(k_s2_init_lane), a);
    // the pair walk's other accumulators (slice 0 is acc itself, set by the table build)
    if (h->slices > 1)
        launch_by_source<S2Const<GECM_NL>>(stream, mc, grid, k_s2_merge<GECM_NL>, k_s2_merge_multi<GECM_NL>,
                                           GECM_LANE(k_s2_merge_lane), a.acc, h->slices, a.stride, 1);
}

static void launch_s2_pair(void *stream, const gecm_modconst *mc, const gecm_s2_pair_launch *h)
{
    const S2PairArgs &a = h->a;
    // the tape on the host decides the launch sequence: one k_s2_gen per "generate" mark, one
    // k_s2_pairs per run of pairs between marks (~84 + 84 launches per 1e8 range)
    const dim3 grid = blocks_of(a.stride);
    const dim3 pgrid((unsigned)(a.stride / 64), h->slices ? h->slices : 1);
    // a "generate" mark with bit 31 set in its count is a single-chain chunk (the reference's last batch of the range,
    // gecm_stage2_pair); the others use K sub-sequences per curve when the batch is small or the context asks (a.K > 1).
    // A multi-modulus mc at K = 1 keeps the gen kernels it always had; at K > 1 its single-chain chunks need kprev.
    const dim3 kgrid = blocks_of(a.stride * (a.K ? a.K : 1));
    uint32_t generated = 0, i = 0, kprev = 1;
    while (i < a.nsteps) {
        if (h->host_steps[2 * i] == S2_STEP_GEN) {
            const uint32_t word = h->host_steps[2 * i + 1];
            const uint32_t n = word & 0x7fffffffu;
            if (mc->source != GECM_SRC_VALUE && a.K <= 1)
                launch_by_source<>(stream, mc, grid, nullptr, k_s2_gen_multi<GECM_NL>, GECM_LANE(k_s2_gen_lane), a, generated, n);
            else if (a.K > 1 && !(word & 0x80000000u)) {
                launch_by_source<S2Const<GECM_NL>>(stream, mc, kgrid, k_s2_gen_k<GECM_NL>, k_s2_gen_k_multi<GECM_NL>,
                                                   GECM_LANE(k_s2_gen_k_lane), a, generated, n);
                kprev = a.K;
                if (h->k_chunks) ++*h->k_chunks;
            } else if (mc->source != GECM_SRC_VALUE) {
                launch_by_source<>(stream, mc, grid, nullptr, k_s2_gen_after_k_multi<GECM_NL>, GECM_LANE(k_s2_gen_after_k_lane), a,
                                   generated, n, generated ? kprev : 1u);
                kprev = 1;
            } else {
                launch_by_source<S2Const<GECM_NL>>(stream, mc, grid, k_s2_gen<GECM_NL>, nullptr, nullptr, a, generated, n,
                                                   generated ? kprev : 1u);
                kprev = 1;
            }
            generated += n;
            i++;
        } else {
            uint32_t j = i;
            while (j < a.nsteps && h->host_steps[2 * j] != S2_STEP_GEN) j++;
            launch_by_source<S2Const<GECM_NL>>(stream, mc, pgrid, k_s2_pairs<GECM_NL>, k_s2_pairs_multi<GECM_NL>,
                                               GECM_LANE(k_s2_pairs_lane), a, i, j - i);
            i = j;
        }
    }
    if (h->slices > 1)
        launch_by_source<S2Const<GECM_NL>>(stream, mc, grid, k_s2_merge<GECM_NL>, k_s2_merge_multi<GECM_NL>,
                                           GECM_LANE(k_s2_merge_lane), a.acc, h->slices, a.stride, 0);
}

// stage 2 of a P-1 / P+1 batch: P into S, then the table with K >= 1 sub-sequences per position
static void launch_s2_init_unit(void *stream, const gecm_modconst *mc, const gecm_s2_init_launch *h, int pm1)
{
    const S2InitArgs &a = h->a;
    const dim3 grid = blocks_of(a.stride);
    launch_by_source<S2Const<GECM_NL>>(stream, mc, grid, k_s2u_seed<GECM_NL>, k_s2u_seed_multi<GECM_NL>, GECM_LANE(k_s2u_seed_lane),
                                       a.X, const_cast<uint32_t *>(a.S), a.acc, a.fail, a.stride, (uint32_t)(pm1 != 0));
    launch_by_source<S2Const<GECM_NL>>(stream, mc, blocks_of(a.stride * a.K), k_s2u_init<GECM_NL>, k_s2u_init_multi<GECM_NL>,
                                       GECM_LANE(k_s2u_init_lane), a);
    if (h->slices > 1)
        launch_by_source<S2Const<GECM_NL>>(stream, mc, grid, k_s2_merge<GECM_NL>, k_s2_merge_multi<GECM_NL>,
                                           GECM_LANE(k_s2_merge_lane), a.acc, h->slices, a.stride, 1);
}

// The tape as launch_s2_pair walks it: k_s2u_gen at the marks, with the K of the batch at every one of them (bit 31 of
// a mark's count, "one chain, one inversion", means nothing where nothing is inverted), the shared walk between them.
static void launch_s2_pair_unit(void *stream, const gecm_modconst *mc, const gecm_s2_pair_launch *h)
{
    const S2PairArgs &a = h->a;
    const dim3 grid = blocks_of(a.stride);
    const dim3 pgrid((unsigned)(a.stride / 64), h->slices ? h->slices : 1);
    const dim3 kgrid = blocks_of(a.stride * a.K);
    uint32_t generated = 0, i = 0;
    while (i < a.nsteps) {
        if (h->host_steps[2 * i] == S2_STEP_GEN) {
            const uint32_t n = h->host_steps[2 * i + 1] & 0x7fffffffu;
            launch_by_source<S2Const<GECM_NL>>(stream, mc, kgrid, k_s2u_gen<GECM_NL>, k_s2u_gen_multi<GECM_NL>,
                                               GECM_LANE(k_s2u_gen_lane), a, generated, n);
            if (a.K > 1 && h->k_chunks) ++*h->k_chunks;
            generated += n;
            i++;
        } else {
            uint32_t j = i;
            while (j < a.nsteps && h->host_steps[2 * j] != S2_STEP_GEN) j++;
            launch_by_source<S2Const<GECM_NL>>(stream, mc, pgrid, k_s2_pairs<GECM_NL>, k_s2_pairs_multi<GECM_NL>,
                                               GECM_LANE(k_s2_pairs_lane), a, i, j - i);
            i = j;
        }
    }
    if (h->slices > 1)
        launch_by_source<S2Const<GECM_NL>>(stream, mc, grid, k_s2_merge<GECM_NL>, k_s2_merge_multi<GECM_NL>,
                                           GECM_LANE(k_s2_merge_lane), a.acc, h->slices, a.stride, 0);
}

extern "C" const gecm_kernels_p2 *CAT(CAT(gecm_kernels_, GECM_NL), _p2)(void)
{
    static const gecm_kernels_p2 t = {launch_s2_init, launch_s2_pair, GECM_MANIFEST, launch_s2_init_unit, launch_s2_pair_unit};
    return &t;
}
#endif
