"""fe_invert (avx-ecm_amd/csrc/gecm_stage2.hpp) restated on Python integers, step for step, and the directed inputs of
tests/test_inverse_model_cpu.py and tests/test_gpu_inverse.py.

A tool for choosing and classifying inputs, NOT a reference: every assertion of those tests compares with
pow(x, -1, n) and math.gcd.  What the model adds is what the device cannot tell: at which batch g became 0, the sign
of the final f, where d stood before the correction steps of the end game, and how large the values grew.

The 28 division steps of a batch work on 32-bit words; they are done with numpy on all inputs of a call at once
(the same wrapping arithmetic as the kernel's uint32_t), the big values stay Python integers."""
import random

import numpy as np

LIMB = 28
M28 = (1 << LIMB) - 1
BUILT = [8, 10, 12, 14, 15, 17, 19, 21, 23, 26, 28, 30, 32, 34, 37]      # limb counts of the library (gecm_launch.h)
RANGES = ("[-2N,-N)", "[-N,0)", "[0,N)", "[N,2N)")


def dev_limbs(bits):
    """pick_nl of host/gecm_api.c: R = 2^(28 nl) >= 32 N"""
    need = (bits + 5 + LIMB - 1) // LIMB
    return next(nl for nl in BUILT if nl >= need)


def inv_iters(bits):
    """gecm_mod_setup, host/gecm_mod.c: floor((45907 bits + 26313) / 19929) + 1 steps, in whole batches of 28"""
    return ((45907 * bits + 26313) // 19929 + 1 + 27) // 28


def ref_maxbits(bits, digitbits=52):
    """MAXBITS of the reference (main.c:465-483): the smallest multiple of 208 (128) strictly greater than bits"""
    step = 208 if digitbits == 52 else 128
    return step * (bits // step + 1)


def _i32(a):
    return a.astype(np.uint32).view(np.int32).astype(np.int64)


def _batch_matrices(zeta, fl, gl):
    """the inner loop of fe_invert on the low words of all inputs: zeta int32, fl, gl uint32 arrays ->
    (zeta, U, V, Q, W) with the matrix entries as signed 32-bit values"""
    u = np.ones_like(fl)
    v = np.zeros_like(fl)
    q = np.zeros_like(fl)
    w = np.ones_like(fl)
    for _ in range(LIMB):
        c1 = (zeta >> 31).view(np.uint32)
        c2 = np.uint32(0) - (gl & np.uint32(1))
        xx, yy, zz = (fl ^ c1) - c1, (u ^ c1) - c1, (v ^ c1) - c1
        gl = gl + (xx & c2)
        q = q + (yy & c2)
        w = w + (zz & c2)
        c1 = c1 & c2
        zeta = (zeta ^ c1.view(np.int32)) - np.int32(1)
        fl = fl + (gl & c1)
        u = u + (q & c1)
        v = v + (w & c1)
        gl = gl >> np.uint32(1)
        u = u << np.uint32(1)
        v = v << np.uint32(1)
    return zeta, _i32(u), _i32(v), _i32(q), _i32(w)


def invert_many(n, xs, batches=None, nl=None):
    """fe_invert(x, N = n) for every canonical x of xs, `batches` batches of 28 steps (default: inv_iters of n) at nl
    limbs (default: the library's choice for n).  One dict per input:
      inv        x^-1 mod n, or None when gcd != 1 (the kernel returns its d all the same; stage 2 zeroes it)
      d          what the kernel returns as the inverse: d after the end game
      gcd        the final |f|
      converged  first batch count after which g == 0 (None: never within `batches`)
      f_negative sign of the final f
      d_range    index into RANGES: where d stood after the negate, before the two +N steps and the -N
      maxabs     largest |d|, |e|, |f|, |g| seen after any batch"""
    bits = n.bit_length()
    if batches is None:
        batches = inv_iters(bits)
    if nl is None:
        nl = dev_limbs(bits)
    cnt = len(xs)
    ninv = pow(n, -1, 1 << LIMB)                    # (0 - rho) & M28 with rho = -N^-1 mod 2^28
    n0 = n & M28
    f, g, d, e = [n] * cnt, list(xs), [0] * cnt, [1] * cnt
    conv = [0 if x == 0 else None for x in xs]
    mx = [[0, 1, n, x] for x in xs]
    zeta = np.full(cnt, -1, dtype=np.int32)
    if nl == 1:
        raise ValueError("one limb: the low limb would carry the sign")
    with np.errstate(over="ignore"):
        for bt in range(batches):
            fl = np.array([v & M28 for v in f], dtype=np.uint32)
            gl = np.array([v & M28 for v in g], dtype=np.uint32)
            zeta, Ua, Va, Qa, Wa = _batch_matrices(zeta, fl, gl)
            Ua, Va, Qa, Wa = Ua.tolist(), Va.tolist(), Qa.tolist(), Wa.tolist()
            for i in range(cnt):
                U, V, Q, W = Ua[i], Va[i], Qa[i], Wa[i]
                di, ei, fi, gi = d[i], e[i], f[i], g[i]
                # (d, e) <- (U d + V e, Q d + W e) / 2^28 mod N: md, me multiples of N make the sums divisible, and start
                # from the matrix entries where d, e are negative, which pulls the result back towards [0, N)
                md = (U if di < 0 else 0) + (V if ei < 0 else 0)
                me = (Q if di < 0 else 0) + (W if ei < 0 else 0)
                cd = U * (di & M28) + V * (ei & M28)
                ce = Q * (di & M28) + W * (ei & M28)
                md -= (ninv * cd + md) & M28
                me -= (ninv * ce + me) & M28
                assert (cd + n0 * md) & M28 == 0 and (ce + n0 * me) & M28 == 0
                d[i] = (U * di + V * ei + md * n) >> LIMB
                e[i] = (Q * di + W * ei + me * n) >> LIMB
                # (f, g) <- (U f + V g, Q f + W g) / 2^28, exact
                tf, tg = U * fi + V * gi, Q * fi + W * gi
                assert tf & M28 == 0 and tg & M28 == 0
                f[i], g[i] = tf >> LIMB, tg >> LIMB
                m = mx[i]
                m[0] = max(m[0], abs(d[i])); m[1] = max(m[1], abs(e[i]))
                m[2] = max(m[2], abs(f[i])); m[3] = max(m[3], abs(g[i]))
                if conv[i] is None and g[i] == 0:
                    conv[i] = bt + 1
    out = []
    for i in range(cnt):
        fi, di = f[i], d[i]
        neg = fi < 0
        if neg:                                     # negate_if(f, sf); negate_if(d, sf)
            fi, di = -fi, -di
        rng = 0 if di < -n else 1 if di < 0 else 2 if di < n else 3
        in_reach = -2 * n <= di < 2 * n             # what the end game can bring into [0, N)
        if di < 0:                                  # add_n_if, twice
            di += n
        if di < 0:
            di += n
        if di >= n:                                 # fe_sub_borrow + fe_select
            di -= n
        out.append({"inv": di if fi == 1 else None, "d": di, "gcd": fi, "converged": conv[i], "f_negative": neg,
                    "d_range": rng, "in_reach": in_reach, "maxabs": tuple(mx[i])})
    return out


def invert(n, x, batches=None, nl=None):
    return invert_many(n, [x], batches, nl)[0]


def top_limb_bound(nl):
    """a value whose low nl - 1 limbs hold 28 bits each and whose top limb is a signed 32-bit word: |v| < this"""
    return 1 << (LIMB * (nl - 1) + 31)


# ---- the directed inputs -----------------------------------------------------------------------------------------
P = 1000003
KINDS = ("random", "2^k-1", "2^k+1", "1mod2^28", "composite")


def edge_bits():
    """(limb count, bit length) for the smallest and the largest modulus of every built limb count (the rule of
    _edge_cases in tests/test_gpu_fform.py)"""
    out = []
    for i, nl in enumerate(BUILT):
        prev = BUILT[i - 1] if i else 7
        out.append((nl, LIMB * prev - 4))
        out.append((nl, LIMB * nl - 5))
    return out


def modulus(bits, kind):
    """the modulus of that kind with exactly `bits` bits; for "composite" N = P * q"""
    rng = random.Random("modulus:%d:%s" % (bits, kind))
    top = 1 << (bits - 1)
    if kind == "random":
        n = rng.getrandbits(bits) | top | 1
    elif kind == "2^k-1":
        n = (1 << bits) - 1
    elif kind == "2^k+1":
        n = top + 1
    elif kind == "1mod2^28":
        n = ((rng.getrandbits(bits) | top) >> LIMB << LIMB) | 1
    elif kind == "composite":
        lo, hi = -(-top // P), ((1 << bits) - 1) // P
        n = P * (rng.randrange(lo, hi) | 1)
        if n.bit_length() != bits:                  # | 1 stepped over the top: the even neighbour's other side
            n -= 2 * P
    else:
        raise ValueError(kind)
    assert n.bit_length() == bits and n & 1 and dev_limbs(bits) in BUILT
    return n


def searched(n, bits, kind, idx):
    """input idx of the seeded search over one modulus: uniform values, values of a random length, values just below N,
    and sparse values, in turn"""
    rng = random.Random("search:%d:%s:%d" % (bits, kind, idx))
    form = idx % 4
    if form == 0:
        return rng.randrange(n)
    if form == 1:
        return rng.getrandbits(rng.randrange(1, bits)) % n
    if form == 2:
        return n - 1 - rng.getrandbits(rng.randrange(1, bits - 1))
    v = 0
    for _ in range(rng.randrange(1, 6)):
        v ^= 1 << rng.randrange(bits)
    return v % n


SEARCH_PER_MODULUS = 134          # 150 moduli: 20,100 inputs


def fixed_operands(n, bits, kind, nl, rmodn):
    """the inputs every modulus gets: the edges of [0, N), every limb boundary from below and from above, R mod N and,
    for the composite, multiples of its known divisors"""
    rng = random.Random("operands:%d:%s" % (bits, kind))
    xs = [0, 1, 2, n - 1, n - 2, (n - 1) // 2, (n + 1) // 2, rmodn]
    for i in range(nl + 1):
        for j in (LIMB * i - 1, LIMB * i, LIMB * i + 1):
            if 0 <= j and (1 << j) < n:
                xs += [1 << j, n - (1 << j)]
    if kind == "composite":
        q = n // P
        xs += [P, q, n - P, n - q]
        xs += [P * rng.randrange(1, q) for _ in range(4)] + [q * rng.randrange(1, P) for _ in range(4)]
    xs += [rng.randrange(n) for _ in range(64)]
    assert all(0 <= x < n for x in xs)
    return xs


def operands(n, bits, kind, nl, rmodn):
    """fixed_operands and the inputs mined from the search for this modulus (MINED below)"""
    return fixed_operands(n, bits, kind, nl, rmodn) + [searched(n, bits, kind, i) for i in MINED.get((bits, kind), ())]


def mine(per_modulus=SEARCH_PER_MODULUS, keep_late=2, progress=None):
    """The seeded search the directed set was mined from: per modulus the inputs that converge last and one input per
    d-range and sign of f that the fixed operands of that modulus do not reach.  Returns (MINED table, statistics).
    Run as a script to print both; the table is pasted below."""
    table, stats = {}, {"ranges": [0] * 4, "f_negative": 0, "inputs": 0, "min_slack": None, "out_of_reach": 0}
    for nl, bits in edge_bits():
        for kind in KINDS:
            n = modulus(bits, kind)
            iters = inv_iters(bits)
            xs = [searched(n, bits, kind, i) for i in range(per_modulus)]
            res = invert_many(n, xs, iters, nl)
            base = invert_many(n, fixed_operands(n, bits, kind, nl, pow(2, ref_maxbits(bits), n)), iters, nl)
            have = {(r["d_range"], r["f_negative"]) for r in base}
            picks = []
            late = lambda r: iters + 1 if r["converged"] is None else r["converged"]
            order = sorted(range(per_modulus), key=lambda i: -late(res[i]))
            picks += order[:keep_late]
            for i, r in enumerate(res):
                stats["ranges"][r["d_range"]] += 1
                stats["f_negative"] += r["f_negative"]
                stats["out_of_reach"] += not r["in_reach"]
                slack = iters - late(r)
                if stats["min_slack"] is None or slack < stats["min_slack"][0]:
                    stats["min_slack"] = (slack, bits, kind, i)
                key = (r["d_range"], r["f_negative"])
                if key not in have:
                    have.add(key)
                    picks.append(i)
            for r in base:
                slack = iters - late(r)
                if slack < stats["min_slack"][0]:
                    stats["min_slack"] = (slack, bits, kind, "fixed")
            stats["inputs"] += per_modulus
            table[(bits, kind)] = tuple(sorted(set(picks)))
            if progress:
                progress(bits, kind, table[(bits, kind)])
    return table, stats


# (bit length, kind) -> indices of searched() kept for that modulus.  Written by mine().
MINED = {
    (192, '1mod2^28'): (12, 31), (192, '2^k+1'): (0, 1), (192, '2^k-1'): (60, 81), (192, 'composite'): (10, 36),
    (192, 'random'): (22, 39), (219, '1mod2^28'): (0, 10), (219, '2^k+1'): (0, 112), (219, '2^k-1'): (61, 72),
    (219, 'composite'): (21, 52), (219, 'random'): (0, 20), (220, '1mod2^28'): (11, 27), (220, '2^k+1'): (26, 102),
    (220, '2^k-1'): (0, 10), (220, 'composite'): (5, 13), (220, 'random'): (18, 44), (275, '1mod2^28'): (5, 43),
    (275, '2^k+1'): (8, 130), (275, '2^k-1'): (4, 16), (275, 'composite'): (2, 10), (275, 'random'): (36, 38),
    (276, '1mod2^28'): (9, 16), (276, '2^k+1'): (12, 106), (276, '2^k-1'): (3, 9), (276, 'composite'): (1, 6),
    (276, 'random'): (1, 2), (331, '1mod2^28'): (6, 8), (331, '2^k+1'): (10, 42), (331, '2^k-1'): (40, 45),
    (331, 'composite'): (28, 34), (331, 'random'): (10, 37), (332, '1mod2^28'): (0, 4), (332, '2^k+1'): (0, 1),
    (332, '2^k-1'): (10, 14), (332, 'composite'): (4, 10), (332, 'random'): (6, 15), (387, '1mod2^28'): (10, 14),
    (387, '2^k+1'): (21, 22), (387, '2^k-1'): (18, 22), (387, 'composite'): (4, 13), (387, 'random'): (11, 18),
    (388, '1mod2^28'): (4, 9), (388, '2^k+1'): (3, 5), (388, '2^k-1'): (4, 6), (388, 'composite'): (2, 5),
    (388, 'random'): (4, 5), (415, '1mod2^28'): (4, 10), (415, '2^k+1'): (0, 1), (415, '2^k-1'): (4, 5),
    (415, 'composite'): (6, 8), (415, 'random'): (2, 12), (416, '1mod2^28'): (0, 2), (416, '2^k+1'): (0, 10),
    (416, '2^k-1'): (8, 9), (416, 'composite'): (5, 6), (416, 'random'): (3, 6), (471, '1mod2^28'): (2, 10),
    (471, '2^k+1'): (10, 16), (471, '2^k-1'): (0, 1), (471, 'composite'): (1, 13), (471, 'random'): (2, 6),
    (472, '1mod2^28'): (0, 2), (472, '2^k+1'): (0, 4), (472, '2^k-1'): (2, 3), (472, 'composite'): (0, 1),
    (472, 'random'): (1, 4), (527, '1mod2^28'): (0, 2), (527, '2^k+1'): (1, 7), (527, '2^k-1'): (5, 8),
    (527, 'composite'): (2, 5), (527, 'random'): (0, 1), (528, '1mod2^28'): (2, 4), (528, '2^k+1'): (0, 2),
    (528, '2^k-1'): (2, 5), (528, 'composite'): (3, 5), (528, 'random'): (0, 2), (583, '1mod2^28'): (2, 6),
    (583, '2^k+1'): (2, 4), (583, '2^k-1'): (1, 5), (583, 'composite'): (0, 2), (583, 'random'): (1, 3),
    (584, '1mod2^28'): (1, 4), (584, '2^k+1'): (1, 2), (584, '2^k-1'): (0, 1), (584, 'composite'): (1, 3),
    (584, 'random'): (0, 1), (639, '1mod2^28'): (1, 2), (639, '2^k+1'): (8, 16), (639, '2^k-1'): (0, 2),
    (639, 'composite'): (2, 7), (639, 'random'): (0, 1), (640, '1mod2^28'): (0, 3), (640, '2^k+1'): (0, 6),
    (640, '2^k-1'): (0, 2), (640, 'composite'): (0, 1), (640, 'random'): (0, 1), (723, '1mod2^28'): (1, 4),
    (723, '2^k+1'): (0, 1), (723, '2^k-1'): (0, 4), (723, 'composite'): (0, 5), (723, 'random'): (3, 5),
    (724, '1mod2^28'): (1, 2), (724, '2^k+1'): (0, 1), (724, '2^k-1'): (0, 4), (724, 'composite'): (0, 1),
    (724, 'random'): (0, 2), (779, '1mod2^28'): (1, 2), (779, '2^k+1'): (0, 1), (779, '2^k-1'): (4, 46),
    (779, 'composite'): (1, 2), (779, 'random'): (0, 1), (780, '1mod2^28'): (0, 3), (780, '2^k+1'): (0, 4),
    (780, '2^k-1'): (0, 8), (780, 'composite'): (0, 1), (780, 'random'): (1, 2), (835, '1mod2^28'): (0, 1),
    (835, '2^k+1'): (0, 4), (835, '2^k-1'): (1, 2), (835, 'composite'): (0, 97), (835, 'random'): (2, 3),
    (836, '1mod2^28'): (1, 3), (836, '2^k+1'): (0, 4), (836, '2^k-1'): (0, 4), (836, 'composite'): (0, 1),
    (836, 'random'): (0, 1), (891, '1mod2^28'): (0, 1), (891, '2^k+1'): (0, 5), (891, '2^k-1'): (0, 1),
    (891, 'composite'): (0, 2), (891, 'random'): (0, 106), (892, '1mod2^28'): (0, 85), (892, '2^k+1'): (0, 2),
    (892, '2^k-1'): (0, 2), (892, 'composite'): (0, 38), (892, 'random'): (0, 1), (947, '1mod2^28'): (0, 1),
    (947, '2^k+1'): (0, 1), (947, '2^k-1'): (0, 1), (947, 'composite'): (0, 2), (947, 'random'): (0, 1),
    (948, '1mod2^28'): (0, 32), (948, '2^k+1'): (0, 1), (948, '2^k-1'): (0, 5), (948, 'composite'): (1, 81),
    (948, 'random'): (2, 3), (1031, '1mod2^28'): (0, 1), (1031, '2^k+1'): (0, 1), (1031, '2^k-1'): (0, 64),
    (1031, 'composite'): (0, 3), (1031, 'random'): (1, 2),
}


if __name__ == "__main__":
    import sys
    t, s = mine(progress=lambda b, k, p: sys.stderr.write("%d %s %r\n" % (b, k, p)))
    print("MINED = {")
    for k in sorted(t):
        print("    %r: %r," % (k, t[k]))
    print("}")
    print("#", s)
