"""Shared by tests/test_gt_exp_cyclo_host.py and tests/test_gt_exp_cyclo_gpu.py: the modulus of the scalar split, the scalars
that sit on its digit boundaries, and Gt members computed once by the oracle."""
import functools

from oracle import pyref as R

CURVES = ("BN254", "BLS12-381", "BLS12-377")


def split_modulus(cp):
    """(L, dimension): on Gt the Frobenius map is exponentiation by p mod r = x on the BLS12 curves (L = |x|, four digits) and
    6 x^2 on BN254 (two digits)"""
    if cp.name == "BN254":
        return 6 * cp.x * cp.x, 2
    return abs(cp.x), 4


def digits(cp, s):
    """base-L digits of s, the last one the remaining quotient (not reduced again)"""
    lam, dim = split_modulus(cp)
    out = []
    for _ in range(dim - 1):
        s, d = divmod(s, lam)
        out.append(d)
    out.append(s)
    return out


def boundary_scalars(cp):
    """0, 1, r - 1 (on BN254 the scalar whose top digit exceeds L); L^k - 1, L^k, L^k + 1 for every k below the dimension;
    every digit equal to L - 1"""
    lam, dim = split_modulus(cp)
    out = [0, 1, cp.r - 1]
    for k in range(dim):
        out += [lam**k - 1, lam**k, lam**k + 1]
    out.append(lam**dim - 1)
    return out


@functools.lru_cache(maxsize=None)
def member(name):
    """a Gt member: the pairing of two DRBG points"""
    cp = R.CURVES[name]
    d = R.Drbg("gt_exp_cyclo/member/" + name)
    return R.pairing(cp, R.random_g1(cp, d), R.random_g2(cp, d))


@functools.lru_cache(maxsize=None)
def member_pow(name, s):
    cp = R.CURVES[name]
    return R.gt_to_mont_bytes(cp, R.tower(cp).f12_pow(member(name), s % cp.r))
