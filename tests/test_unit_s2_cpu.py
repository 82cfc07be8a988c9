"""CPU tests (no GPU) of P-1 / P+1 stage 2: the operand bounds of the device sequence
(tests/unit_s2_model.py) at both ends of five limb classes, the pair maps the GPU tests walk, the planted-factor moduli in
Python integers, and the new symbols."""
import math
import os
import random
import re

import pytest

from conftest import ROOT
from suyama_model import pick_nl
from unit_model import METHOD_PM1, METHOD_PP1, OFFSET, UNIT_LIMBS, class_moduli, expected, exponent, jacobi, seeds_for
from unit_s2_model import (CLASSES, GPU_CASES, S2Model, pair_map, plain_acc, plan_map, planted_case, shifts_of, walk)
from xladder import _primes

GECM_OK, GECM_ERR_ARG = 0, -2
METHODS = (METHOD_PM1, METHOD_PP1)
SMALL = (50, 3000, 30, 2)                              # amin > 0; with chunks of 16 giant steps: many chunks, carried state


@pytest.fixture(scope="module")
def pyecm():
    import pyecm
    return pyecm


@pytest.mark.parametrize("nl", UNIT_LIMBS)
def test_operand_bounds_at_both_ends_of_every_class(pyecm, nl):
    """s2u_seed, s2u_init, s2u_gen and the pair step in the kernel's arithmetic: every assertion of S2Model holds and the
    result is the exact product, for one chain and for sub-sequences, amin = 0 and amin > 0"""
    big, small = pair_map(pyecm, CLASSES), pair_map(pyecm, SMALL)
    assert big[2] == 0 and small[2] > 0
    for n in class_moduli(nl):
        rng = random.Random(31 * nl)
        seeds = seeds_for(n, 6, rng)
        for method in METHODS:
            for x in (seeds[0], seeds[2], seeds[5]):                     # 2, N - 1, a random one
                want = plain_acc(method, x, n, [big], *CLASSES[2:])
                for K in (1, 8):
                    got, fail = S2Model(n, nl).stage2(x, method, [big], *CLASSES[2:], K=K)
                    assert fail is None and got == want, (method, K)
            for x in seeds[:4]:
                want = plain_acc(method, x, n, [small, small], *SMALL[2:])
                for K in (2, 32):
                    got, fail = S2Model(n, nl).stage2(x, method, [small, small], *SMALL[2:], K=K, chunk=16)
                    assert fail is None and got == want, (method, K)


def test_seed_without_inverse_leaves_its_gcd():
    n = class_moduli(15)[1]
    f = 1000003
    m = S2Model(n * f, 15)
    P, fail = m.seed(m.to_mont(3 * f), METHOD_PM1)
    assert fail == f and 0 <= P < n * f
    assert m.seed(m.to_mont(3 * f), METHOD_PP1)[1] is None


@pytest.mark.parametrize("case", GPU_CASES + [SMALL], ids=str)
def test_pair_maps_cover_their_primes_and_pass_the_tape_s_rule(pyecm, case):
    b1, b2, D, U = case
    v, u, amin = pair_map(pyecm, case)
    pmap, _ = plan_map(D, U)
    covered = set()
    for a, uu, valid in walk(v, u, amin, U):
        assert valid and uu <= U * D and pmap[uu] != 0, (a, uu)
        covered.update((a * D + uu, a * D - uu))
    missing = [q for q in _primes(b2) if q >= b1 and q not in covered]
    assert not missing, missing[:10]
    assert amin == (b1 + D) // (2 * D)


def test_wrap_case_runs_more_than_two_chunks(pyecm):
    from unit_s2_model import S2_CHUNK, S2_RING, WRAP, tape
    v, u, amin = pair_map(pyecm, WRAP)
    E = 4 * WRAP[3] + 2 * WRAP[3] * shifts_of(v, u)
    assert E > S2_RING and E > 2 * S2_CHUNK
    words, e2 = tape(v, u, amin, *WRAP[2:])
    assert e2 == E and sum(1 for w in words if w[0] == 0xffffffff) > 2


@pytest.mark.parametrize("method", METHODS)
def test_planted_factor_is_found_by_stage_2_only(pyecm, method):
    b1, b2, D, U = CLASSES
    n, p, r, seed = planted_case(method, b1, b2)
    order = p - 1 if method == METHOD_PM1 else p + 1
    e = exponent(1, b1)
    cof = order // math.gcd(order, e)
    assert cof in [q for q in _primes(b2) if q > b1]                    # B1-smooth times one prime in (B1, B2)
    if method == METHOD_PP1:
        assert jacobi(seed * seed - 4, p) == -1
    x = expected(method, seed, e, n)
    assert math.gcd((x - OFFSET[method]) % n, n) == 1                    # stage 1 finds nothing
    acc = plain_acc(method, x, n, [pair_map(pyecm, CLASSES)], D, U)
    assert math.gcd(acc, n) == p
    assert pick_nl(n.bit_length()) == 8
    got, fail = S2Model(n, 8).stage2(x, method, [pair_map(pyecm, CLASSES)], D, U, K=1)
    assert fail is None and got == acc


def test_new_symbols(pyecm):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gecm.h")).read(), flags=re.S)
    for name in ("gecm_set_method_stage2", "gecm_get_method_stage2"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in pyecm.EXPORTS and hasattr(pyecm.lib, name)
    for c, v in (("GECM_METHOD_S2_OFF", 0), ("GECM_METHOD_S2_ON", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (c, v), hdr)
    assert (pyecm.METHOD_S2_OFF, pyecm.METHOD_S2_ON) == (0, 1)
    assert pyecm.lib.gecm_set_method_stage2(None, 1) == GECM_ERR_ARG
    assert pyecm.lib.gecm_get_method_stage2(None) == 0
    for cls in (pyecm.Engine, pyecm.MultiEngine):
        assert callable(cls.set_method_stage2) and callable(cls.method_stage2)
