// gecm_row.hpp — stage 1 with THIRTY-TWO lanes per curve: the X and the Z coordinate of a curve's points on two
// adjacent DPP rows (16 lanes each) of a wavefront, and inside a row each lane holds NQ consecutive limbs of the
// residue (lane l: limbs NQ*l .. NQ*l+NQ-1; NQ = 1 for the 416-bit class).
//
// Why: BASELINE configs[1] is a batch of 4096 curves.  MI355X has 1024 SIMDs and v_mad_u64_u32 only issues at
// its full rate from two wavefronts per SIMD (profiles/r01_valu_ubench_gfx950.txt: 8.2 cycles with one, 4.7
// with two), so the batch has to become 2048 wavefronts: 32 lanes per curve.  The eight-lane layout
// (gecm_quad.hpp) leaves half of the SIMDs without a wavefront and the other half at the slow rate.
//
// The multiply is row-wise (operand scanning) Montgomery, as in the eight-lane layout, re-thought so that a row
// costs 3 multiply-adds and 2.5 DPP moves per lane at NQ = 1 (5 + 2.5 at NQ = 2, 7 + 2.67 at NQ = 3):
//   * arithmetic is modulo N' = m*N with N' = -1 (mod 2^28), so the Montgomery digit is the low limb itself
//     (rho = 1: no multiplication on the dependent path); N' is 28 bits longer than N, which is exactly the room
//     16 lanes x 28 bits leave above a 415-bit N plus the 5 bits of lazy-reduction headroom;
//   * every accumulator is kept multiplied by 16, so that its high register IS the part above 28 bits and its
//     low register IS the low limb (times 16): no shift or mask instructions; the operands are pre-multiplied by
//     4 each, the digit is used as it comes (times 16), and the hand-over "high part into the next slot" is one
//     more v_mad (x16);
//   * digit and operand limbs are broadcast inside the row by DPP row_newbcast — the operand limbs TWO per move
//     (v_mov_b64_dpp, which knows exactly this control) —, the window moves down by DPP row_shl:1;
//   * a multiply ends in the accumulators' own scale: T + 2^31 holds the balanced limb (+ 2^27) in bits 4..31 of its
//     low register and the carry for the lane above AS its high register;
//   * limbs are SIGNED and balanced ([-2^27, 2^27] after a multiply): subtraction is limb-wise without a bias,
//     and the pre-multiplied operands stay inside 32 bits;
//   * between the entry and the exit conversion the tape interpreter keeps every value pre-multiplied (times 4): a
//     multiply delivers its result in that scale in the instructions it spent on the plain one, sums and differences
//     keep it, and no multiply of a point operation shifts an operand;
//   * at one limb per lane in the DPP form a multiply can read a finished broadcast of its scanned operand (fer_scan,
//     fer_mul_scanned), made while an X <-> Z exchange is in flight: the point addition (row_add_scanned, §5f) and the
//     double (row_dup_scanned, §5g) are written for it, and that form has a tape interpreter of its own
//     (run_tape_row_dpp: the rule-3 steps a tight loop, the begin, the end and the add-and-double step a path each, one
//     scan of fA per event, renaming by conditional moves).
// The residues are the same elements of Z/N as in every other layout (N | N'), so results are identical; the
// kernel converts from and to the R = 2^(28*NL) Montgomery form of the device buffers at entry and exit
// (R' = 2^(448*NQ) inside), and k_canon makes the exit values canonical.
#pragma once
#include "gecm_curve.hpp"
#include "gecm_rowk.h"

template <int NQ>
struct FeR {
    int32_t v[NQ];
};

template <int NQ>
struct RowMod {
    uint32_t n[NQ];   // this lane's limbs of the modulus
    uint32_t rho;     // -modulus^-1 mod 2^28 (unused when RHO1)
    int32_t c16;      // 16, in a scalar register, opaque to the compiler (row_c16)
    int32_t kb, zb;   // 2^27 and -2^27 in vector registers (row_bias): the rounding bias of a multiply that delivers its
                      // result times 4 rides on its last two hand-overs (fer_mul, R4); set where R4 is used
};

// An empty asm statement that READS x: a second use of the value stops the compiler from re-associating the sum it
// belongs to (and moving its instruction) and it stays where it is written; no instruction, no register written.
__device__ __forceinline__ void row_pin(const int64_t &x)
{
    asm volatile("" ::"v"(x));
}
__device__ __forceinline__ int32_t row_c16()
{
    int32_t c;
    asm volatile("s_mov_b32 %0, 16" : "=s"(c));
    return c;
}
// v in a vector register of its own for the whole kernel, opaque to the compiler: the high half of an addend pair
template <int32_t V>
__device__ __forceinline__ int32_t row_bias()
{
    int32_t c;
    asm volatile("v_mov_b32 %0, %1" : "=v"(c) : "n"(V));
    return c;
}

#define GECM_DPP_ROW_SHL1 0x101        /* lane l <- lane l+1 of the row (lane 15: 0) */
#define GECM_DPP_ROW_SHR1 0x111        /* lane l <- lane l-1 of the row (lane 0: 0) */
#define GECM_DPP_ROW_ROR1 0x121        /* lane l <- lane l-1 of the row (lane 0 <- lane 15) */
#define GECM_DPP_ROW_NEWBCAST 0x150    /* + i: every lane <- lane i of its row (gfx90a+) */

template <int CTRL>
__device__ __forceinline__ uint32_t row_dpp(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}
template <int I>
__device__ __forceinline__ uint32_t row_bcast(uint32_t x)
{
    return row_dpp<GECM_DPP_ROW_NEWBCAST + I>(x);
}
template <int I>
__device__ __forceinline__ int64_t row_bcast64(int64_t x)       // two registers in one move (v_mov_b64_dpp)
{
    return __builtin_amdgcn_update_dpp((int64_t)0, x, GECM_DPP_ROW_NEWBCAST + I, 0xF, 0xF, true);
}
// every lane <- lane I of its row, through the LDS crossbar (ds_swizzle, bit mode: lane = (lane & 0x10) | I):
// no VALU issue slot, the latency is covered by issuing all broadcasts of a multiply before its first row
template <int I>
__device__ __forceinline__ uint32_t row_bcast_lds(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x10 | (I << 5));
}
__device__ __forceinline__ uint32_t other_row(uint32_t x)       // lane <-> lane ^ 16: the other coordinate
{
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, 0x401F /* bit mode: and 0x1f, or 0, xor 0x10 */);
}

__device__ __forceinline__ void smad(int64_t &acc, int32_t x, int32_t y)
{
    asm("v_mad_i64_i32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(x), "v"(y) : "vcc");
}
__device__ __forceinline__ void umad(int64_t &acc, uint32_t x, uint32_t y)
{
    asm("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc) : "v"(x), "v"(y) : "vcc");
}
__device__ __forceinline__ int64_t smad0(int32_t x, int32_t y)       // x * y
{
    int64_t r;
    asm("v_mad_i64_i32 %0, vcc, %1, %2, 0" : "=v"(r) : "v"(x), "v"(y) : "vcc");
    return r;
}
__device__ __forceinline__ int64_t smad16(int32_t x, int64_t add)    // 16 * x + add
{
    int64_t r;
    asm("v_mad_i64_i32 %0, vcc, %1, 16, %2" : "=v"(r) : "v"(x), "v"(add) : "vcc");
    return r;
}

// 16 * x + add, then + y * z: the hand-over at the end of a row and the first multiply-add of the next row in one
// asm statement (the compiler pads a wait state between two asm statements)
__device__ __forceinline__ int64_t smad16_smad(int32_t x, int64_t add, int32_t y, int32_t z)
{
    int64_t r;
    asm("v_mad_i64_i32 %0, vcc, %1, 16, %2\n\tv_mad_i64_i32 %0, vcc, %3, %4, %0" : "=&v"(r) : "v"(x), "v"(add), "v"(y), "v"(z) : "vcc");
    return r;
}

// The scanned operand of a one-limb-per-lane multiply, broadcast: 4 x limb j of it in every lane of the row (fer_scan).
template <int ROWS>
struct RowScan {
    int32_t Ab[ROWS];
};

// r = a*b/R' mod (modulus of m), R' = 2^(28*ROWS): ROWS = the limbs in use (at most 16*NQ; limbs from ROWS up are
// zero in every operand and in the modulus, so their rows would add nothing).  Operand limbs |.| < 2^29; result limbs in
// [-2^27-4, 2^27+4] (top limb: whatever the value needs), |result| < |a||b|/R' + modulus.
// Three forms: one limb per lane with the limbs of a broadcast by DPP row_newbcast (best up to 2 wavefronts per SIMD),
// one limb per lane with ALDS: through the LDS crossbar (ds_swizzle: no VALU issue slot; best from 3 wavefronts per SIMD
// up), and two or three limbs per lane, by DPP (best at every batch size: profiles/r03/mid_batch_rows.txt).
// A4, B4: the limbs of a, of b come multiplied by 4 already (the scale the rows read); R4: r is delivered times 4.  The
// tape interpreter keeps every value in that scale, so that no multiply of a point operation shifts its operands: the
// bounds above are those of the values, and 4 x (2^29 - 1) still fits the signed 32-bit operand of v_mad_i64_i32.
// SCANNED (one limb per lane, DPP form): the limbs of 4a are in every lane already, in *scan (fer_scan); a is not read and
// the rows make no requests (fer_mul_scanned).
template <int NQ, int ROWS, bool RHO1, bool ALDS, bool A4 = false, bool B4 = false, bool R4 = false, bool SCANNED = false>
__device__ __forceinline__ void fer_mul(FeR<NQ> &r, const FeR<NQ> &a, const FeR<NQ> &b, const RowMod<NQ> &m,
                                        const RowScan<ROWS> *scan = nullptr)
{
    static_assert(ROWS > 16 * (NQ - 1) && ROWS <= 16 * NQ, "the limbs in use fill the lanes but for the last one");
    static_assert(!ALDS || NQ == 1, "the crossbar form is for one limb per lane");
    static_assert(!SCANNED || (NQ == 1 && !ALDS), "a ready-made scan is for the one-limb DPP form");
    int32_t a4[NQ], b4[NQ];
#pragma unroll
    for (int t = 0; t < NQ; t++) {
        a4[t] = A4 ? a.v[t] : (int32_t)((uint32_t)a.v[t] << 2);
        b4[t] = B4 ? b.v[t] : (int32_t)((uint32_t)b.v[t] << 2);
    }
    // The limbs of 4a reach the lanes of the row one per row of the multiply.  A DPP read of a register that a
    // VALU instruction has just written needs two independent instructions in between; a row has two such places
    // (multiply-add -> digit broadcast, multiply-add -> hand-over), and the DPP requests for the next row's limbs
    // are what fills them (a VALU instruction, ready at once: the operand a is only known when the multiply starts).
    // ALDS (3 or more wavefronts per SIMD hide the ~70 cycles of the crossbar): every limb by ds_swizzle, requested
    // up front.
    if constexpr (NQ >= 2) {
        // Two or three limbs per lane (ROWS need not be a multiple of NQ: 31 rows for 831 bits, 38 for 1023): the
        // multiply-adds are written in C and the compiler places them (it knows how many instructions lie between a
        // result and the DPP move that reads it; an asm statement counts as none and is padded).  Two things keep a row at 3 + 2 NQ multiply-adds and 3 DPP moves: the hand-over "16 x high
        // part" multiplies by m.c16, a 16 the compiler cannot see through (it would otherwise spend a shift, a mask
        // and a 64-bit add on it), and the slot the window shift has emptied starts from {lo, 0} as the addend of its
        // first product.  Per row at NQ = 2: 8 VALU instructions and no s_nop where the round-2 form had 9 and two.
        int64_t T[NQ];
        // 4 x limb j of a in every lane of the row: limbs 0 and 1 of a lane travel as ONE 64-bit DPP move
        // (v_mov_b64_dpp knows row_newbcast only, which is the one needed), limb 2 (NQ = 3) on its own
        const int64_t a01 = (int64_t)(((uint64_t)(uint32_t)a4[1] << 32) | (uint32_t)a4[0]);
        int64_t Ap = row_bcast64<0>(a01);
        int32_t As = 0;
        auto limb = [&](auto jc) -> int32_t {     // limb j, which the last request that covers it has brought
            constexpr int q = decltype(jc)::value % NQ;
            return q == 0 ? (int32_t)(uint32_t)Ap : q == 1 ? (int32_t)(Ap >> 32) : As;
        };
#pragma unroll
        for (int t = 0; t < NQ; t++) T[t] = (int64_t)limb(IC<0>{}) * b4[t];
        // The order inside a row is pinned (sched_barrier, row_pin): the digit broadcast and the window shift each read
        // a result two instructions old, so no wait state is left to pad:
        //   digit | q*n (lowest slot first) | a*b into the next lowest slot (and the middle one) | shift | hand-over
        //   | a*b into the emptied slot | request for what the next row's products need
        static_for<0, ROWS>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            constexpr int rot = i % NQ, nxt = (i + 1) % NQ;
            const uint32_t Q = row_bcast<0>(RHO1 ? (uint32_t)T[rot] : (uint32_t)T[rot] * m.rho);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < NQ; t++) {
                T[(t + rot) % NQ] = (int64_t)((uint64_t)T[(t + rot) % NQ] + (uint64_t)Q * m.n[t]);
                __builtin_amdgcn_sched_barrier(0);
            }
            const int32_t Ac = limb(IC<i + 1>{});                  // row i adds limb i + 1 of a
            if constexpr (i + 1 < ROWS) {
#pragma unroll
                for (int t = 0; t < NQ - 1; t++) {
                    T[(t + nxt) % NQ] += (int64_t)Ac * b4[t];
                    row_pin(T[(t + nxt) % NQ]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            const int32_t hi = (int32_t)(T[rot] >> 32);
            const uint32_t lo = row_dpp<GECM_DPP_ROW_SHL1>((uint32_t)T[rot]);
            __builtin_amdgcn_sched_barrier(0);
            T[nxt] += (int64_t)hi * m.c16;
            row_pin(T[nxt]);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (i + 1 < ROWS) {
                T[rot] = (int64_t)Ac * b4[NQ - 1] + (int64_t)(uint64_t)lo;
                row_pin(T[rot]);
            } else {
                T[rot] = (int64_t)(uint64_t)lo;
            }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (i + 2 < ROWS) {
                if constexpr ((i + 2) % NQ == 0) Ap = row_bcast64<(i + 2) / NQ>(a01);
                else if constexpr ((i + 2) % NQ == 2) As = (int32_t)row_bcast<(i + 2) / NQ>((uint32_t)a4[NQ - 1]);
                __builtin_amdgcn_sched_barrier(0);
            }
        });
        // balanced normalisation, in the accumulators' own scale: u16 = 16 x (value + carry + 2^27) has the limb
        // (+ 2^27) in bits 4..31 of its low register and the carry AS its high register
        int32_t lo[NQ];
        int32_t carry = 0;
#pragma unroll
        for (int t = 0; t < NQ - 1; t++) {
            int64_t u16 = T[(t + ROWS) % NQ] + (int64_t)(1u << 31);
            if (t > 0) u16 += (int64_t)carry * m.c16;
            carry = (int32_t)(u16 >> 32);
            lo[t] = (int32_t)(((uint32_t)u16 >> 4) & GECM_LIMB_MASK) - (1 << 27);
        }
        const int32_t ut = (int32_t)(T[(NQ - 1 + ROWS) % NQ] >> 4) + carry + (1 << 27);
        lo[NQ - 1] = (int32_t)((uint32_t)ut & GECM_LIMB_MASK) - (1 << 27);
        const int32_t below = (int32_t)row_dpp<GECM_DPP_ROW_SHR1>((uint32_t)(ut >> GECM_LIMB_BITS));
        lo[0] += below;
#pragma unroll
        for (int t = 0; t < NQ; t++) r.v[t] = R4 ? (int32_t)((uint32_t)lo[t] << 2) : lo[t];
    } else {
        // One limb per lane.  DPP: the limbs travel TWO per move.  Every lane first takes the limb of the lane above
        // next to its own (one row_shl:1 per multiply); a 64-bit move (v_mov_b64_dpp, row_newbcast — the one control it
        // knows) from lane 2k then brings limbs 2k and 2k + 1: 8 moves + 1 instead of 16 for the 416-bit class.
        int32_t Ab[ROWS];
        int64_t a01 = 0;
        if constexpr (SCANNED) {
#pragma unroll
            for (int j = 0; j < ROWS; j++) Ab[j] = scan->Ab[j];
        }
        if constexpr (!ALDS && !SCANNED) a01 = (int64_t)(((uint64_t)row_dpp<GECM_DPP_ROW_SHL1>((uint32_t)a4[0]) << 32) | (uint32_t)a4[0]);
        auto request = [&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if constexpr (SCANNED) {
            } else if constexpr (ALDS) {
                Ab[j] = (int32_t)row_bcast_lds<j>((uint32_t)a4[0]);
            } else if constexpr (j % 2 == 0) {
                const int64_t P = row_bcast64<j>(a01);
                Ab[j] = (int32_t)(uint32_t)P;
                if constexpr (j + 1 < ROWS) Ab[j + 1] = (int32_t)(P >> 32);
            }
        };
        if constexpr (ALDS) static_for<0, ROWS>(request);
        else request(IC<0>{});
        // 16 x this lane's slot of the window.  (An array zeroed in a loop rather than a scalar: the compiler schedules
        // the rows differently when the accumulator is a plain variable from the start.)
        int64_t T[NQ];
#pragma unroll
        for (int t = 0; t < NQ; t++) T[t] = 0;
        static_for<0, ROWS>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            // (the multiply-add was fused with the previous row's hand-over, except in row 0)
            if constexpr (i == 0) T[0] = smad0(Ab[0], b4[0]);
            if constexpr (!ALDS) {
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (i + 1 < ROWS) request(IC<i + 1>{});
                __builtin_amdgcn_sched_barrier(0);
            }
            uint32_t qs = (uint32_t)T[0];                       // 16 x (column mod 2^28)
            if (!RHO1) qs *= m.rho;                             // 16 x the digit (mod 2^32)
            const uint32_t Q = row_bcast<0>(qs);
            umad(T[0], Q, m.n[0]);
            if constexpr (!ALDS) __builtin_amdgcn_sched_barrier(0);    // the hand-over stays after the digit's product
            // the window moves down one limb: the low register (zero on lane 0 by the choice of the digit) goes to the
            // lane below, the high register (the part above 28 bits) is added, times 16, to what comes from the lane
            // above, in the same statement as the next row's first product
            const int32_t hi = (int32_t)(T[0] >> 32);
            const uint32_t lo = row_dpp<GECM_DPP_ROW_SHL1>((uint32_t)T[0]);
            // R4: the rounding bias of the end rides on the last two hand-overs, as the high word of their addend pair
            // (zero everywhere else): + 2^27 into the last row's high part, which its hand-over multiplies by 16, and
            // - 2^27 on that hand-over itself (below)
            int64_t add = (int64_t)(uint64_t)lo;
            if constexpr (R4 && i + 2 == ROWS) add = (int64_t)(((uint64_t)(uint32_t)m.kb << 32) | lo);
            if constexpr (R4 && i + 1 == ROWS) add = (int64_t)(((uint64_t)(uint32_t)m.zb << 32) | lo);
            if constexpr (i + 1 < ROWS) T[0] = smad16_smad(hi, add, Ab[i + 1], b4[0]);
            else T[0] = smad16(hi, add);
        });
        // balanced normalisation in the accumulator's own scale: u16 = 16 x (value + 2^27) has the limb (+ 2^27) in
        // bits 4..31 of its low register and what leaves the lane AS its high register; the neighbour's carry comes in
        // on the add itself (DPP)
        if constexpr (R4) {
            // times 4, and without the add: the hand-overs have put the bias in (m.kb, m.zb above), T[0] is already
            // u16 - 2^59.  Its low register, read unsigned and shifted right by 2, is 4 x limb + 2^29; its high register is
            // the carry - 2^27, which enters shifted on the add (v_lshl_add_u32) and takes the 2^29 away.  Lane 0 has no
            // lane below and needs the bare - 2^27: row_ror:1 brings it lane 15's high register, which is that, because
            // the top lane's carry is 0 (|value| < 1.2 N' < 2^(28 ROWS - 4): the top lane's accumulator is below 2^29
            // in absolute value; lanes from ROWS up hold 0 throughout).  DESIGN.md §5e.
            r.v[0] = (int32_t)(((uint32_t)T[0] >> 2) + (row_dpp<GECM_DPP_ROW_ROR1>((uint32_t)(T[0] >> 32)) << 2));
        } else {
            const int64_t u16 = T[0] + (int64_t)(1u << 31);
            const int32_t lim = (int32_t)(((uint32_t)u16 >> 4) & GECM_LIMB_MASK) - (1 << 27);
            r.v[0] = lim + (int32_t)row_dpp<GECM_DPP_ROW_SHR1>((uint32_t)(u16 >> 32));
        }
    }
}

// The one-limb DPP multiply in two halves, for a scanned operand that is known BEFORE the multiply can start (row_add_scanned:
// each of its two scanned multiplies waits for an X <-> Z exchange that its scanned operand does not need).  fer_scan makes
// all the requests for the limbs of a (times 4) at once: one row_shl:1 and ROWS / 2 v_mov_b64_dpp, VALU work that stays where
// it is written, between a ds_swizzle and the wait that covers it.  fer_mul_scanned is the rows of fer_mul on the finished scan:
// r = a*b/R' times 4, b times 4, the flags A4, B4, R4 and the bounds of fer_mul.  The rows ask for nothing; the wait-state
// slots that a request filled in every other row are padded.  The product is the same integer whichever operand is scanned;
// how its carries are spread over the limbs is not.
template <int ROWS>
__device__ __forceinline__ void fer_scan(RowScan<ROWS> &s, const FeR<1> &a)
{
    const int64_t a01 = (int64_t)(((uint64_t)row_dpp<GECM_DPP_ROW_SHL1>((uint32_t)a.v[0]) << 32) | (uint32_t)a.v[0]);
    static_for<0, (ROWS + 1) / 2>([&](auto kc) {
        constexpr int j = 2 * decltype(kc)::value;
        const int64_t P = row_bcast64<j>(a01);
        s.Ab[j] = (int32_t)(uint32_t)P;
        if constexpr (j + 1 < ROWS) s.Ab[j + 1] = (int32_t)(P >> 32);
    });
    __builtin_amdgcn_sched_barrier(0);
}
template <int ROWS>
__device__ __forceinline__ void fer_mul_scanned(FeR<1> &r, const RowScan<ROWS> &s, const FeR<1> &b, const RowMod<1> &m)
{
    fer_mul<1, ROWS, true, false, true, true, true, true>(r, b, b, m, &s);
}

// A point coordinate as the tape interpreter keeps it: its own limbs and those of the other coordinate, both TIMES 4 (the
// scale the rows of a multiply read: fer_mul, A4 / B4 / R4), from one exchange between the X row and the Z row when the
// point is made.  The exchange goes through the LDS crossbar (ds_swizzle, lane ^ 16): no VALU issue slot, which is what
// a batch at 2 wavefronts per SIMD is short of (v_permlane16_swap, measured: 7% slower at 4096 curves).
// The sum and the difference that the point formulas read (ecm.c:407-457 split into X and Z halves as in gecm_quad.hpp)
// are made where a formula reads them (row_sd, row_ds), not kept: a point addition reads ONE of them of each of two
// points, which costs the four instructions that making both of the new point would, and the renaming of a PRAC step
// moves two registers per point instead of four.
template <int NQ>
struct PtR {
    FeR<NQ> own;   // X rows: 4X       Z rows: 4Z
    FeR<NQ> oth;   // X rows: 4Z       Z rows: 4X         (the operand this point gives as the difference point "C")
};

struct RowSign {
    uint32_t mz, bz;   // Z rows: -1, 1    X rows: 0, 0      (x ^ mz) + bz = -x on Z rows
    uint32_t mx, bx;   // X rows: -1, 1    Z rows: 0, 0
};

template <int NQ>
__device__ __forceinline__ void fer_other(FeR<NQ> &r, const FeR<NQ> &a)
{
#pragma unroll
    for (int t = 0; t < NQ; t++) r.v[t] = (int32_t)other_row((uint32_t)a.v[t]);
}

// r = oth + own on X rows, oth - own on Z rows
template <int NQ>
__device__ __forceinline__ void fer_sum_diff(FeR<NQ> &r, const FeR<NQ> &oth, const FeR<NQ> &own, const RowSign &g)
{
#pragma unroll
    for (int t = 0; t < NQ; t++) r.v[t] = (int32_t)((uint32_t)oth.v[t] + ((uint32_t)own.v[t] ^ g.mz) + g.bz);
}

// the operand a point gives as "A": 4(Z + X) on X rows, 4(X - Z) on Z rows
template <int NQ>
__device__ __forceinline__ void row_sd(FeR<NQ> &r, const PtR<NQ> &p, const RowSign &g)
{
    fer_sum_diff<NQ>(r, p.oth, p.own, g);
}

// the operand a point gives as "B": 4(X - Z) on X rows, 4(Z + X) on Z rows
template <int NQ>
__device__ __forceinline__ void row_ds(FeR<NQ> &r, const PtR<NQ> &p, const RowSign &g)
{
#pragma unroll
    for (int t = 0; t < NQ; t++) r.v[t] = (int32_t)((uint32_t)p.own.v[t] + ((uint32_t)p.oth.v[t] ^ g.mx) + g.bx);
}

// r <- pick ? b : a (pick: all ones or zero, wave-uniform, in a scalar register pair) as an instruction of its own, where
// it is written: the renaming of a rule-3 step (run_tape_row) frees a register BEFORE the new point is made, so that the
// new point is made in it, and does so without a branch.  Left to the compiler, the renaming is a branch with copies on
// both sides at the end of the step, and the new point is copied once more.
template <int NQ>
__device__ __forceinline__ void row_pick(FeR<NQ> &r, const FeR<NQ> &a, const FeR<NQ> &b, uint64_t pick)
{
#pragma unroll
    for (int t = 0; t < NQ; t++) {
        int32_t x;
        asm volatile("v_cndmask_b32 %0, %1, %2, %3" : "=v"(x) : "v"(a.v[t]), "v"(b.v[t]), "s"(pick));
        r.v[t] = x;
    }
}

// own coordinate of T = A + B with difference C (vec_add, ecm.c:407-443): fB = row_ds(B), fA = row_sd(A), c = C.oth;
// every value times 4.  With A and B exchanged the result is the same residue: the X rows then make V and the Z rows U,
// U - V changes sign and the square removes it.  The swap of a rule-3 step is therefore only a renaming (run_tape_row).
template <int NQ, int ROWS, bool ALDS>
__device__ __forceinline__ void row_add(FeR<NQ> &own, const FeR<NQ> &fB, const FeR<NQ> &fA, const FeR<NQ> &c, bool isZ,
                                        const RowSign &g, const RowMod<NQ> &m)
{
    FeR<NQ> w, t, e;
    fer_mul<NQ, ROWS, true, ALDS, true, true, true>(w, fB, fA, m);      // X: U      Z: V
    fer_other<NQ>(t, w);
    fer_sum_diff<NQ>(e, t, w, g);                                       // X: V + U  Z: U - V
    fer_mul<NQ, ROWS, true, ALDS, true, true, true>(e, e, e, m);
    fer_mul<NQ, ROWS, true, ALDS, true, true, true>(own, e, c, m);
}

// row_add for one limb per lane in the DPP form, with VALU work in the shadow of both X <-> Z exchanges.  sA = the scan of
// fA, made by the caller while the exchange that fB waits for is in flight: the first multiply scans the kept point's form
// (old) instead of the new point's.  The exchange of the first product is followed by the scan of c, which has been known
// since the step began, and by shadow(), whatever the caller can do once c has been read (the renaming of a rule-3 step);
// the third multiply then scans c instead of the fresh square.  Bounds: fA and fB are a sum or a difference of two product
// limbs, times 4 (at most 2^30 + 32 in absolute value), c and the square are product limbs times 4: each inside fer_mul's
// 4 x 2^29 whether it is the scanned operand or the lane's own.
template <int ROWS, class Shadow>
__device__ __forceinline__ void row_add_scanned(FeR<1> &own, const RowScan<ROWS> &sA, const FeR<1> &fB, const FeR<1> &c,
                                                const RowSign &g, const RowMod<1> &m, Shadow &&shadow)
{
    FeR<1> w, t, e;
    RowScan<ROWS> sC;
    fer_mul_scanned<ROWS>(w, sA, fB, m);                                // X: U      Z: V
    fer_other<1>(t, w);
    fer_scan<ROWS>(sC, c);
    shadow();
    __builtin_amdgcn_sched_barrier(0);
    fer_sum_diff<1>(e, t, w, g);                                        // X: V + U  Z: U - V
    fer_mul<1, ROWS, true, false, true, true, true>(e, e, e, m);
    fer_mul_scanned<ROWS>(own, sC, e, m);
}

// own coordinate of D = 2A (vec_duplicate, ecm.c:445-457): fA = row_sd(A), s4 = (A+2)/4 of the curve; every value times 4
template <int NQ, int ROWS, bool ALDS>
__device__ __forceinline__ void row_dup(FeR<NQ> &own, const FeR<NQ> &fA, const FeR<NQ> &s4, bool isZ, const RowSign &g,
                                        const RowMod<NQ> &m)
{
    FeR<NQ> q, t, w, p1, p2, r1;
    fer_mul<NQ, ROWS, true, ALDS, true, true, true>(q, fA, fA, m);      // X: U = (x+z)^2    Z: V = (x-z)^2
    fer_other<NQ>(t, q);                                                // X: V              Z: U
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        w.v[i] = t.v[i] - q.v[i];                     // Z: w = U - V
        p1.v[i] = isZ ? s4.v[i] : q.v[i];
        p2.v[i] = isZ ? w.v[i] : t.v[i];
    }
    fer_mul<NQ, ROWS, true, ALDS, true, true, true>(r1, p1, p2, m);     // X: U*V            Z: s*w
#pragma unroll
    for (int i = 0; i < NQ; i++) t.v[i] = r1.v[i] + q.v[i];     // Z: s*w + V
    fer_mul<NQ, ROWS, true, ALDS, true, true, true>(t, t, w, m);        // Z: (s*w + V)*w
#pragma unroll
    for (int i = 0; i < NQ; i++) own.v[i] = isZ ? t.v[i] : r1.v[i];
}

// row_dup for one limb per lane in the DPP form, on the caller's scan of fA (the one the addition of the same event has
// read already), with VALU work in the shadow of its X <-> Z exchange: the second multiply scans p1, which does not wait
// for the exchange (the Z rows' s4, the X rows' own square), and the third scans w, known since before the second.  The
// products are the same residues whichever operand is scanned.  Bounds: fA is a sum or a difference
// of two product limbs times 4 (at most 2^30 + 32 in absolute value), p1 a product limb times 4, w and r1 + q a
// difference and a sum of two such: each inside fer_mul's 4 x 2^29 whether it is the scanned operand or the lane's own.
template <int ROWS>
__device__ __forceinline__ void row_dup_scanned(FeR<1> &own, const RowScan<ROWS> &sA, const FeR<1> &fA, const FeR<1> &s4,
                                                bool isZ, const RowMod<1> &m)
{
    FeR<1> q, t, w, p1, p2, r1;
    RowScan<ROWS> sP, sW;
    fer_mul_scanned<ROWS>(q, sA, fA, m);                                // X: U = (x+z)^2    Z: V = (x-z)^2
    fer_other<1>(t, q);                                                 // X: V              Z: U
    p1.v[0] = isZ ? s4.v[0] : q.v[0];
    fer_scan<ROWS>(sP, p1);
    w.v[0] = t.v[0] - q.v[0];                                           // Z: w = U - V
    p2.v[0] = isZ ? w.v[0] : t.v[0];
    fer_mul_scanned<ROWS>(r1, sP, p2, m);                               // X: U*V            Z: s*w
    t.v[0] = r1.v[0] + q.v[0];                                          // Z: s*w + V
    fer_scan<ROWS>(sW, w);
    fer_mul_scanned<ROWS>(t, sW, t, m);                                 // Z: (s*w + V)*w
    own.v[0] = isZ ? t.v[0] : r1.v[0];
}

template <int NQ>
__device__ __forceinline__ void fer_load(FeR<NQ> &r, const uint32_t *__restrict__ base, size_t stride, uint32_t cidx,
                                         uint32_t l, uint32_t nl)
{
#pragma unroll
    for (int t = 0; t < NQ; t++) {
        const uint32_t limb = (uint32_t)NQ * l + (uint32_t)t;
        r.v[t] = limb < nl ? (int32_t)base[(size_t)limb * stride + cidx] : 0;
    }
}

// run_tape_row (below) for one limb per lane in the DPP form: the same events, the same operands in the same roles, every
// event written the way the loop of rule-3 steps is.  A begin, an end and an add-and-double step are
// three paths that meet only at the head of the tape loop; every path ends with the next tape byte and then the exchange
// of its last result, and what it renames it renames by conditional moves on wave-uniform masks (row_pick) in chosen
// places, so that no path has a join of its own where the compiler copies points (what is left: three copies where a path
// returns to the head, five between the rule-3 loop and the other events).  One scan of fA serves the addition's first
// multiply and the double's.  The rule-3 steps stay a loop of their own inside the tape loop: as one more path of a flat
// loop every step took two jumps across the other paths' 11 KB, and the kernel was 2 % slower than before instead of 2 %
// faster.  The fetch of the tape bytes, the rule-3 renaming and the meaning of every op byte are written
// here and in run_tape_row: a change of the tape format (gecm_tape.h) touches both.
template <int ROWS>
__device__ __forceinline__ void run_tape_row_dpp(const uint32_t *__restrict__ tape, uint32_t tape_len, PtR<1> &A,
                                                 const FeR<1> &s4, bool isZ, const RowSign &g, const RowMod<1> &m)
{
    // Of C only the other coordinate is kept between steps, as in run_tape_row.
    PtR<1> B = A;
    FeR<1> Coth = A.oth;
    auto fetch = [&](uint32_t pc) -> uint32_t {
        uint32_t w = tape[pc >> 2];
        return __builtin_amdgcn_readfirstlane((w >> ((pc & 3u) * 8u)) & 0xffu);
    };
    uint32_t pc = 0;
    uint32_t op = tape_len ? fetch(0) : GECM_OP_NOP;
    uint32_t nxt = 1 < tape_len ? fetch(1) : GECM_OP_NOP;
    // the tape byte before the exchange that ends an event: its scalar load and the wait for it would drain the exchange
    auto advance = [&]() {
        pc++;
        op = nxt;
        nxt = (pc + 1 < tape_len) ? fetch(pc + 1) : GECM_OP_NOP;
        __builtin_amdgcn_sched_barrier(0);
    };
    while (pc < tape_len) {
        // rule 3: T = A + B (C); (A, B, C) <- (A, T, B), after a swap (B, T, A): the sum does not depend on the order of A
        // and B (row_add), so the swap only says which of the two stays A and which becomes C.  Three conditional moves:
        // what stays A is chosen before the addition (B's own register is then free), what becomes C behind the scan of the
        // old C, and the new point is made in B's registers.  The exchange that brings B.oth was issued at the end of the
        // event before, and what does not read it comes first: the form of the kept point, the pick that frees B's
        // register and the scan of that form.  Only then fB, the wait, and the rows.
        while ((op & ~GECM_OP_SWAP) == (GECM_OP_STEP | GECM_OP_RULE3)) {
            const uint64_t swap = (op & GECM_OP_SWAP) ? ~(uint64_t)0 : 0;
            FeR<1> fA, fB;
            RowScan<ROWS> sA;
            row_sd<1>(fA, A, g);
            row_pick<1>(A.own, A.own, B.own, swap);
            fer_scan<ROWS>(sA, fA);
            row_ds<1>(fB, B, g);
            row_add_scanned<ROWS>(B.own, sA, fB, Coth, g, m, [&]() {
                row_pick<1>(Coth, B.oth, A.oth, swap);
                row_pick<1>(A.oth, A.oth, B.oth, swap);
            });
            advance();
            fer_other<1>(B.oth, B.own);
        }
        if (op == GECM_OP_NOP) {
            advance();
            continue;
        }
        FeR<1> fA, fB;
        RowScan<ROWS> sA;
        if (op == GECM_OP_PRAC_END) {                   // A <- A + B (C)
            row_sd<1>(fA, A, g);
            fer_scan<ROWS>(sA, fA);
            row_ds<1>(fB, B, g);
            row_add_scanned<ROWS>(A.own, sA, fB, Coth, g, m, []() {});
            advance();
            fer_other<1>(A.oth, A.own);
            continue;
        }
        if (op == GECM_OP_PRAC_BEGIN) {                 // B <- A, C <- A, A <- 2A
            row_sd<1>(fA, A, g);
            fer_scan<ROWS>(sA, fA);
            B = A;
            Coth = A.oth;
            row_dup_scanned<ROWS>(A.own, sA, fA, s4, isZ, m);
            advance();
            fer_other<1>(A.oth, A.own);
            continue;
        }
        // An add-and-double step.  With a, b = A, B after the swap bit:
        //   rule 4   T = a + b (C)    A <- 2a, B <- T
        //   rule 5   T = a + C (b)    A <- 2a, B <- b, C <- T
        //   rule 9   T = b + C (a)    A <- a, B <- 2b, C <- T: rule 5 with a and b exchanged before and A and B after; the
        //            exchange before is the swap bit inverted, the one after a branch that 42 of a B1 = 1e6 tape's events take
        // a, b by conditional moves; rules 5 and 9 put C in b's place as the addition's second point and b.oth in C's as its
        // difference, by three more, and put b back behind the double, by another three.  C's own coordinate is fetched on
        // rules 5 and 9 alone, as soon as the byte is known, and read behind the scan of fA.  T's exchange has the whole
        // double behind it; the double's goes out behind the next tape byte, with the renaming behind it.
        const bool r59 = (op & GECM_OP_RULE_MASK) != GECM_OP_RULE4, r9 = (op & GECM_OP_RULE_MASK) == GECM_OP_RULE9;
        const uint64_t swap = (uint64_t)0 - (((op >> 2) ^ ((op >> 1) & op)) & 1u);  // SWAP is bit 2; rule 9 has bits 0 and 1
        const uint64_t rot = (uint64_t)0 - ((op >> 1) & 1u);                      // rules 5 and 9 have bit 1
        PtR<1> a, b, q;
        FeR<1> Cown, c, T, Toth;
        // Cown is written on rules 5 and 9 only.  The empty asm gives it a register without an instruction, so that the pick
        // of q.own below has an operand on rule 4 too: rot is 0 there, the pick takes b.own and what the register holds is
        // never selected.
        asm volatile("" : "=v"(Cown.v[0]));
        if (r59) fer_other<1>(Cown, Coth);
        row_pick<1>(a.own, A.own, B.own, swap);
        row_pick<1>(a.oth, A.oth, B.oth, swap);
        row_sd<1>(fA, a, g);
        fer_scan<ROWS>(sA, fA);
        row_pick<1>(b.own, B.own, A.own, swap);
        row_pick<1>(b.oth, B.oth, A.oth, swap);
        row_pick<1>(q.own, b.own, Cown, rot);
        row_pick<1>(q.oth, b.oth, Coth, rot);
        row_pick<1>(c, Coth, b.oth, rot);
        row_ds<1>(fB, q, g);
        row_add_scanned<ROWS>(T, sA, fB, c, g, m, []() {});
        fer_other<1>(Toth, T);
        row_dup_scanned<ROWS>(A.own, sA, fA, s4, isZ, m);
        advance();
        fer_other<1>(A.oth, A.own);
        row_pick<1>(B.own, T, b.own, rot);
        row_pick<1>(B.oth, Toth, b.oth, rot);
        row_pick<1>(Coth, Coth, Toth, rot);
        if (r9) {
            const PtR<1> t = A;
            A = B;
            B = t;
        }
    }
}

// run_tape_quad of gecm_quad.hpp on rows: A, B, C are this lane's limbs of its coordinate (and their forms).  The one-limb
// DPP form goes to run_tape_row_dpp above, which reads the same tape: a change of the tape format touches both.
template <int NQ, int ROWS, bool ALDS>
__device__ __forceinline__ void run_tape_row(const uint32_t *__restrict__ tape, uint32_t tape_len, PtR<NQ> &A,
                                             const FeR<NQ> &s4, bool isZ, const RowSign &g, const RowMod<NQ> &m)
{
    if constexpr (NQ == 1 && !ALDS) {
        run_tape_row_dpp<ROWS>(tape, tape_len, A, s4, isZ, g, m);
        return;
    }
    // Of C only the other coordinate is kept between steps: that is what C gives to an addition, and its own one is the
    // other row's (one more exchange, made in the steps that turn C into A or B: rules 5 and 9).
    PtR<NQ> B = A;
    FeR<NQ> Coth = A.oth;
    auto fetch = [&](uint32_t pc) -> uint32_t {
        uint32_t w = tape[pc >> 2];
        return __builtin_amdgcn_readfirstlane((w >> ((pc & 3u) * 8u)) & 0xffu);
    };
    uint32_t nxt = tape_len ? fetch(0) : GECM_OP_NOP;
    for (uint32_t pc = 0; pc < tape_len; pc++) {
        uint32_t op = nxt;
        nxt = (pc + 1 < tape_len) ? fetch(pc + 1) : GECM_OP_NOP;
        // rule 3: T = A + B (C); (A, B, C) <- (A, T, B), after a swap (B, T, A): the sum does not depend on the order of A
        // and B (row_add), so the swap only says which of the two stays A and which becomes C.  Three conditional moves:
        // what stays A is chosen before the addition (B's own register is then free), what becomes C behind the last
        // multiply, which reads the old C, and the new point is made in B's registers.
        while ((op & ~GECM_OP_SWAP) == (GECM_OP_STEP | GECM_OP_RULE3)) {
            const uint64_t swap = (op & GECM_OP_SWAP) ? ~(uint64_t)0 : 0;
            FeR<NQ> fA, fB;
            row_sd<NQ>(fA, A, g);
            row_ds<NQ>(fB, B, g);
            row_pick<NQ>(A.own, A.own, B.own, swap);
            row_add<NQ, ROWS, ALDS>(B.own, fB, fA, Coth, isZ, g, m);
            row_pick<NQ>(Coth, B.oth, A.oth, swap);
            row_pick<NQ>(A.oth, A.oth, B.oth, swap);
            fer_other<NQ>(B.oth, B.own);
            pc++;
            op = nxt;
            nxt = (pc + 1 < tape_len) ? fetch(pc + 1) : GECM_OP_NOP;
        }
        if (op == GECM_OP_NOP) continue;
        const uint32_t rule = op & GECM_OP_RULE_MASK;
        const bool is_step = op >= GECM_OP_STEP;
        const bool do_add = op != GECM_OP_PRAC_BEGIN;
        const bool do_dup = op != GECM_OP_PRAC_END;
        PtR<NQ> C;
        C.oth = Coth;
        fer_other<NQ>(C.own, Coth);
        if (is_step && (op & GECM_OP_SWAP)) {
            PtR<NQ> t = A;
            A = B;
            B = t;
        }
        if (is_step && rule == GECM_OP_RULE5) {
            PtR<NQ> t = B;
            B = C;
            C = t;
        } else if (is_step && rule == GECM_OP_RULE9) {
            PtR<NQ> t = A;
            A = B;
            B = C;
            C = t;
        } else if (op == GECM_OP_PRAC_BEGIN) {
            B = A;
            C = A;
        }
        PtR<NQ> T, D;
        FeR<NQ> fA, fB;
        row_sd<NQ>(fA, A, g);
        row_ds<NQ>(fB, B, g);
        if (do_add) {
            row_add<NQ, ROWS, ALDS>(T.own, fB, fA, C.oth, isZ, g, m);
            fer_other<NQ>(T.oth, T.own);
        }
        if (do_dup) {
            row_dup<NQ, ROWS, ALDS>(D.own, fA, s4, isZ, g, m);
            fer_other<NQ>(D.oth, D.own);
        }
        if (op == GECM_OP_PRAC_END) {
            A = T;
        } else if (op == GECM_OP_PRAC_BEGIN) {
            A = D;
        } else if (rule == GECM_OP_RULE4) {
            B = T;
            A = D;
        } else if (rule == GECM_OP_RULE5) {
            PtR<NQ> t = C;
            C = T;
            B = t;
            A = D;
        } else {
            PtR<NQ> oldA = C;
            C = T;
            B = D;
            A = oldA;
        }
        Coth = C.oth;
    }
}

// Constants of the row kernel, one array of GECM_ROW_WORDS words per kind, limb j at word j (zero padded):
//   [0] N' = m*N, = -1 mod 2^28      [1] N      [2] c_in = R'^2 / R mod N (entry conversion: x R -> x R')
//   [3] R mod N (exit conversion)    [4] K' of N (bias that makes the exit value's limbs non-negative)
// (GECM_ROW_WORDS, GECM_ROW_KINDS: gecm_rowk.h)

// The whole stage-1 kernel body for one lane.  nl = limbs per residue in the device buffers (R = 2^(28*nl)).
// ALDS: the scanned operand of a multiply reaches the lanes of its row through the LDS crossbar (fer_mul).
template <int NQ, int ROWS, bool ALDS>
__device__ __forceinline__ void stage1_row(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
                                           uint32_t *__restrict__ Z, const uint32_t *__restrict__ S, size_t stride,
                                           uint32_t nl, const uint32_t *__restrict__ rc, uint32_t rho_n)
{
    const uint32_t cidx = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;      // wavefronts of a workgroup are independent
    const uint32_t l = threadIdx.x & 15u;
    const bool isZ = (threadIdx.x & 16u) != 0;
    uint32_t *mine = isZ ? Z : X;
    RowMod<NQ> mp, mn;
    FeR<NQ> cin, one, kp;
#pragma unroll
    for (int t = 0; t < NQ; t++) {
        const uint32_t j = (uint32_t)NQ * l + (uint32_t)t;
        mp.n[t] = rc[0 * GECM_ROW_WORDS + j];
        mn.n[t] = rc[1 * GECM_ROW_WORDS + j];
        cin.v[t] = (int32_t)rc[2 * GECM_ROW_WORDS + j];
        one.v[t] = (int32_t)rc[3 * GECM_ROW_WORDS + j];
        kp.v[t] = (int32_t)rc[4 * GECM_ROW_WORDS + j];
    }
    mp.rho = 1u;
    mn.rho = rho_n;
    mp.c16 = mn.c16 = row_c16();
    mp.kb = mn.kb = mp.zb = mn.zb = 0;
    if constexpr (NQ == 1) {       // (two and three limbs per lane: the same fold saves no instruction)
        mp.kb = mn.kb = row_bias<(1 << 27)>();
        mp.zb = mn.zb = row_bias<-(1 << 27)>();
    }
    PtR<NQ> P;
    FeR<NQ> s4, t;
    fer_load<NQ>(t, mine, stride, cidx, l, nl);
    fer_mul<NQ, ROWS, true, ALDS, false, false, true>(P.own, t, cin, mp);     // x*R -> 4 x*R' (mod N')
    RowSign g;
    g.mz = isZ ? 0xffffffffu : 0u;
    g.bz = isZ ? 1u : 0u;
    g.mx = ~g.mz;
    g.bx = 1u - g.bz;
    fer_other<NQ>(P.oth, P.own);
    fer_load<NQ>(t, S, stride, cidx, l, nl);
    fer_mul<NQ, ROWS, true, ALDS, false, false, true>(s4, t, cin, mp);
    run_tape_row<NQ, ROWS, ALDS>(tape, tape_len, P, s4, isZ, g, mp);
    fer_mul<NQ, ROWS, false, ALDS, true>(t, P.own, one, mn);              // 4 x*R' -> x*R (mod N), in (-N/16, 17N/16)
    // + K' (a multiple of N with every limb >= 2^28 - 1): all limbs positive; then one carry-save pass
    uint32_t u[NQ];
#pragma unroll
    for (int i = 0; i < NQ; i++) u[i] = (uint32_t)(t.v[i] + kp.v[i]);
    const uint32_t below = row_dpp<GECM_DPP_ROW_SHR1>(u[NQ - 1] >> GECM_LIMB_BITS);
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        const uint32_t limb = (uint32_t)NQ * l + (uint32_t)i;
        const uint32_t v = (u[i] & GECM_LIMB_MASK) + (i == 0 ? below : (u[i - 1] >> GECM_LIMB_BITS));
        if (limb < nl) mine[(size_t)limb * stride + cidx] = (limb == nl - 1) ? v + (u[i] & ~GECM_LIMB_MASK) : v;
    }
}

// ======================================================================================
// One residue per row: P-1 and P+1 stage 1 for small method batches.  Four residues per wavefront, the
// limbs of each over the 16 lanes of its DPP row as above; the multiply is fer_mul as it stands (DPP form), the
// interpreter is run_tape_unit of gecm_curve.hpp on FeR values: no X/Z exchange, no PtR forms.
//   add T = X + Y, difference W:  P-1: X*Y       P+1: X*Y - W
//   dup D = 2X:                   P-1: X^2       P+1: X^2 - 2
// Limbs are signed and balanced, so the subtraction is limb-wise.  Its VALUE is not a product, though: with W an earlier
// difference the bound would grow by a modulus per step, so every subtraction ends in a reduction (fer_reduce).  The
// kernel works modulo M = N'' (gecm_rowk.h), whose limb ROWS - 1 is at least 2^20: the top limb of a value then gives
// its quotient by M.

// v <- v - q M with q = rint(top limb of v / (M / 2^(28 (ROWS - 1)))), then one balanced carry pass over the limbs below
// the top one.  In: limbs |.| <= 2^28 + 8 below the top, |v| <= 2.1 M.  Out: limbs in [-2^27 - 3, 2^27 + 2] below the
// top, |v| <= (1/2 + 2^-19) M: with B = 2^(28 (ROWS - 1)), v / B = top + d with |d| < 1.0001, so q differs from v / M by
// at most 1/2 + 1.0001 B / M + the float roundings (three of 2^-24 relative on a quotient below 2.2), and B / M <= 2^-20.
template <int NQ, int ROWS>
__device__ __forceinline__ void fer_reduce(FeR<NQ> &v, const RowMod<NQ> &m, float minv, uint32_t l)
{
    constexpr int TL = (ROWS - 1) / NQ, TS = (ROWS - 1) % NQ;       // lane and slot of the top limb
    const int32_t top = (int32_t)row_bcast<TL>((uint32_t)v.v[TS]);
    const int32_t q = (int32_t)__builtin_rintf((float)top * minv);  // |q| <= 2
    int32_t lo[NQ], c[NQ];
#pragma unroll
    for (int t = 0; t < NQ; t++) {
        const int32_t x = v.v[t] - q * (int32_t)m.n[t];
        const bool split = (uint32_t)NQ * l + (uint32_t)t < (uint32_t)(ROWS - 1);
        c[t] = split ? (x + (1 << 27)) >> GECM_LIMB_BITS : 0;       // arithmetic shift: the balanced carry
        lo[t] = x - (int32_t)((uint32_t)c[t] << GECM_LIMB_BITS);
    }
    v.v[0] = lo[0] + (int32_t)row_dpp<GECM_DPP_ROW_SHR1>((uint32_t)c[NQ - 1]);
#pragma unroll
    for (int t = 1; t < NQ; t++) v.v[t] = lo[t] + c[t - 1];
}

template <int NQ>
struct UnitRow {
    RowMod<NQ> m;      // M = N'', rho = 1
    FeR<NQ> two;       // 2 R' mod M, balanced
    float minv;        // 1 / (M / 2^(28 (ROWS - 1)))
    uint32_t l;        // lane of the row
    bool pp1;          // wave-uniform
};

// T = X*Y (- W)
template <int NQ, int ROWS>
__device__ __forceinline__ void unit_row_add(FeR<NQ> &T, const FeR<NQ> &X, const FeR<NQ> &Y, const FeR<NQ> &W,
                                             const UnitRow<NQ> &u)
{
    fer_mul<NQ, ROWS, true, false>(T, X, Y, u.m);
    if (u.pp1) {
#pragma unroll
        for (int t = 0; t < NQ; t++) T.v[t] -= W.v[t];
        fer_reduce<NQ, ROWS>(T, u.m, u.minv, u.l);
    }
}

// run_tape_unit (gecm_curve.hpp) on rows: the same control flow, the same renamings; A, B, C one FeR each.
template <int NQ, int ROWS>
__device__ __forceinline__ void run_tape_unit_row(const uint32_t *__restrict__ tape, uint32_t tape_len, FeR<NQ> &A,
                                                  const UnitRow<NQ> &u)
{
    FeR<NQ> B = A, C = A;
    auto fetch = [&](uint32_t pc) -> uint32_t {
        uint32_t w = tape[pc >> 2];
        return __builtin_amdgcn_readfirstlane((w >> ((pc & 3u) * 8u)) & 0xffu);
    };
    uint32_t nxt = tape_len ? fetch(0) : GECM_OP_NOP;
    for (uint32_t pc = 0; pc < tape_len; pc++) {
        uint32_t op = nxt;
        nxt = (pc + 1 < tape_len) ? fetch(pc + 1) : GECM_OP_NOP;
        // rule 3: T = B + A (C); (B,T,C) <- (T,C,B)
        while ((op & ~GECM_OP_SWAP) == (GECM_OP_STEP | GECM_OP_RULE3)) {
            if (op & GECM_OP_SWAP) {
                FeR<NQ> t = A;
                A = B;
                B = t;
            }
            FeR<NQ> T;
            unit_row_add<NQ, ROWS>(T, B, A, C, u);
            C = B;
            B = T;
            pc++;
            op = nxt;
            nxt = (pc + 1 < tape_len) ? fetch(pc + 1) : GECM_OP_NOP;
        }
        if (op == GECM_OP_NOP) continue;
        const uint32_t rule = op & GECM_OP_RULE_MASK;
        const bool is_step = op >= GECM_OP_STEP;
        const bool do_add = op != GECM_OP_PRAC_BEGIN;
        const bool do_dup = op != GECM_OP_PRAC_END;
        if (is_step && (op & GECM_OP_SWAP)) {
            FeR<NQ> t = A;
            A = B;
            B = t;
        }
        if (is_step && rule == GECM_OP_RULE5) {
            FeR<NQ> t = B;
            B = C;
            C = t;
        } else if (is_step && rule == GECM_OP_RULE9) {
            FeR<NQ> t = A;
            A = B;
            B = C;
            C = t;
        } else if (op == GECM_OP_PRAC_BEGIN) {
            B = A;
            C = A;
        }
        FeR<NQ> T, D;
        if (do_add) unit_row_add<NQ, ROWS>(T, B, A, C, u);       // T = B + A, difference C
        if (do_dup) unit_row_add<NQ, ROWS>(D, A, A, u.two, u);   // D = 2A
        if (op == GECM_OP_PRAC_END) {
            A = T;
        } else if (op == GECM_OP_PRAC_BEGIN) {
            A = D;
        } else if (rule == GECM_OP_RULE4) {
            B = T;
            A = D;
        } else if (rule == GECM_OP_RULE5) {
            FeR<NQ> t = C;
            C = T;
            B = t;
            A = D;
        } else {
            FeR<NQ> oldA = C;
            C = T;
            B = D;
            A = oldA;
        }
    }
}

// The whole kernel body for one lane: position = global thread index >> 4, rc = the constant set of the position's
// modulus (gecm_rowk.h).  nl = limbs per residue in the device buffers (R = 2^(28*nl)).
template <int NQ, int ROWS>
__device__ __forceinline__ void unit_row(const uint32_t *__restrict__ tape, uint32_t tape_len, uint32_t *__restrict__ X,
                                         size_t stride, uint32_t nl, bool pp1, const uint32_t *__restrict__ rc)
{
    const uint32_t pos = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;       // the rows of a wavefront are independent
    const uint32_t l = threadIdx.x & 15u;
    UnitRow<NQ> u;
    RowMod<NQ> mn;
    FeR<NQ> cin, one, kp;
#pragma unroll
    for (int t = 0; t < NQ; t++) {
        const uint32_t j = (uint32_t)NQ * l + (uint32_t)t;
        u.m.n[t] = rc[0 * GECM_ROW_WORDS + j];
        mn.n[t] = rc[1 * GECM_ROW_WORDS + j];
        cin.v[t] = (int32_t)rc[2 * GECM_ROW_WORDS + j];
        one.v[t] = (int32_t)rc[3 * GECM_ROW_WORDS + j];
        kp.v[t] = (int32_t)rc[4 * GECM_ROW_WORDS + j];
        u.two.v[t] = (int32_t)rc[5 * GECM_ROW_WORDS + j];
    }
    u.minv = __uint_as_float(rc[6 * GECM_ROW_WORDS + 0]);
    u.m.rho = 1u;
    mn.rho = rc[6 * GECM_ROW_WORDS + 1];
    u.m.c16 = mn.c16 = row_c16();
    u.l = l;
    u.pp1 = pp1;
    FeR<NQ> A, t;
    fer_load<NQ>(t, X, stride, pos, l, nl);
    fer_mul<NQ, ROWS, true, false>(A, t, cin, u.m);              // x*R -> x*R' (mod M), |.| < 1.001 M
    fer_reduce<NQ, ROWS>(A, u.m, u.minv, l);                     // |.| <= (1/2 + 2^-19) M
    run_tape_unit_row<NQ, ROWS>(tape, tape_len, A, u);
    fer_mul<NQ, ROWS, false, false>(t, A, one, mn);              // x*R' -> x*R (mod N), in (-N/16, 17N/16)
    // + K', one carry-save pass: as stage1_row ends
    uint32_t w[NQ];
#pragma unroll
    for (int i = 0; i < NQ; i++) w[i] = (uint32_t)(t.v[i] + kp.v[i]);
    const uint32_t below = row_dpp<GECM_DPP_ROW_SHR1>(w[NQ - 1] >> GECM_LIMB_BITS);
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        const uint32_t limb = (uint32_t)NQ * l + (uint32_t)i;
        const uint32_t v = (w[i] & GECM_LIMB_MASK) + (i == 0 ? below : (w[i - 1] >> GECM_LIMB_BITS));
        if (limb < nl) X[(size_t)limb * stride + pos] = (limb == nl - 1) ? v + (w[i] & ~GECM_LIMB_MASK) : v;
    }
}
