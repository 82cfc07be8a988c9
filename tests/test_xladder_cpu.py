"""tests/xladder.py, the independent check value of the GPU tests, against itself as it was before its parts were exposed
and against the affine group law on a curve small enough to add points one at a time."""
import pytest

from xladder import ladder_point, stage1_multiplier, true_stage1_point

# (n, sigma, b1) -> what true_stage1_point returned when it was one function
RECORDED = [
    ((1 << 89) - 1, 7, 100,
     (87078810313488210985804716, 484036067276956481068985554)),
    (1000003 * ((1 << 61) - 1), 1234567, 500,
     (868113434585341026206655, 423962732889660174831477)),
    (((1 << 127) - 1) * ((1 << 107) - 1), 2 ** 40 + 17, 2000,
     (20089499788092144807953580422095685783524314726504212752821294057452143,
      14699887811741207813626609354238117422886987448981556712203855039735026)),
]


@pytest.mark.parametrize("n,sigma,b1,want", RECORDED, ids=["M89", "1000003*M61", "M127*M107"])
def test_true_stage1_point_is_what_it_was(n, sigma, b1, want):
    assert true_stage1_point(n, sigma, b1) == want


def test_stage1_multiplier():
    assert stage1_multiplier(2) == 1 and stage1_multiplier(3) == 2
    assert stage1_multiplier(9) == 8 * 3 * 5 * 7                        # 9 = 3^2 is not below 9
    assert stage1_multiplier(10) == 8 * 9 * 5 * 7
    assert stage1_multiplier(30) == 16 * 27 * 25 * 7 * 11 * 13 * 17 * 19 * 23 * 29


def _affine_add(p, A, P, Q):
    """P + Q on y^2 = x^3 + A x^2 + x over GF(p); None is the point at infinity"""
    if P is None:
        return Q
    if Q is None:
        return P
    (x1, y1), (x2, y2) = P, Q
    if x1 == x2 and (y1 + y2) % p == 0:
        return None
    if P == Q:
        lam = (3 * x1 * x1 + 2 * A * x1 + 1) * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - A - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


@pytest.mark.parametrize("p,a24,x", [(1009, 3, 5), (10007, 1234, 77), (65537, 40000, 2)])
def test_ladder_point_equals_repeated_affine_addition(p, a24, x):
    A = (4 * a24 - 2) % p
    assert (A * A - 4) % p                                              # a curve
    while True:                                                         # the first abscissa from x on with a point above it
        rhs = (x ** 3 + A * x * x + x) % p
        y = next((y for y in range(1, p) if y * y % p == rhs), None)
        if y is not None:
            break
        x += 1
    P = (x, y)
    mult, Q, order = [None], None, None
    for k in range(1, 3 * p):
        Q = _affine_add(p, A, Q, P)
        mult.append(Q)
        if Q is None and order is None:
            order = k
    assert order is not None and order > 2
    for k in (0, 1, 2, 3, 4, 5, 7, 30, 255, 256, order - 1, order, order + 1, 2 * order, 2 * order + 3,
              stage1_multiplier(12) % (3 * p)):
        X, Z = ladder_point(p, x, a24, k)
        if mult[k] is None:
            assert Z == 0 and X != 0, k
        else:
            assert Z != 0 and X * pow(Z, -1, p) % p == mult[k][0], k
