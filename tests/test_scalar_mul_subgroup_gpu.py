"""mlhip_scalar_mul / mlhip_scalar_mul_device with MLHIP_GROUP_SUBGROUP on the GPU: batched Mul for points promised in
G1 / G2 over the curve's endomorphisms (mathlib_amd/csrc/msm_scalar_mul_endo.h).  Every curve and both groups: byte-equal
to the plain call on the same buffers and to oracle/pyref.py -- one wave, a second wave of lane pairs (33) and of lanes
(65), whole waves plus a remainder (300), one base for all scalars below and above the fixed-base threshold, plain and
Montgomery scalars on the digit boundaries of the split and unreduced ones, infinities in the batch.  A point OUTSIDE the
subgroup shows which route ran: the split gives the endomorphism's value for it, the plain kernel the product."""
import ctypes
import functools

import pytest

from conftest import load_golden
from gt_exp_cyclo_cases import boundary_scalars, split_modulus
from point_sum_cases import distinct_points, outside_subgroup_point

pytestmark = pytest.mark.gpu

CURVES = {"BN254": 0, "BLS12-381": 1, "BLS12-377": 2}
# (n, point_stride): 33 puts a G2 lane pair into a second wave, 65 a G1 lane; 300 = whole waves and a remainder; stride 0 with
# 300 scalars is the split kernel on one base, with 4096 the fixed-base table path (the flag is ignored there)
SHAPES = ((1, 1), (33, 1), (65, 1), (300, 1), (300, 0), (4096, 0))
ENV = ("MLHIP_SCALAR_MUL_ENDO", "MLHIP_FIXED_BASE_MIN", "MLHIP_FB_WINDOW", "MLHIP_FB_CACHE", "MLHIP_SCALAR_MUL_ONE_LANE")


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


@pytest.fixture(autouse=True)
def default_routes(monkeypatch):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def delay(lib, mlhip):
    """the delay of tests/stream_order_cases.py, calibrated once"""
    import stream_order_cases as S

    d = S.Delay(lib, mlhip)
    assert 50.0 <= d.ms <= 2000.0, (d.repeat, d.ms)
    return d


def group_ops(cp, group):
    from oracle import pyref as R

    if group == 1:
        return (lambda P: R.g1_to_mont_bytes(cp, P)), (lambda P, k: R.g1_mul(cp, P, k))
    return (lambda Q: R.g2_to_mont_bytes(cp, Q)), (lambda Q, k: R.g2_mul(cp, Q, k))


@functools.lru_cache(maxsize=None)
def scalar_rows(name):
    """{mont: [(32 scalar bytes, the multiplier they mean)]}: the boundary scalars of the split and values below 2^64 and 2^128
    keep their value in both forms; r, r + 1, 2r + 3 and 2^256 - 1 are taken as they are (with scalars_mont they mean
    s / 2^256 mod r)"""
    from oracle import pyref as R

    cp = R.CURVES[name]
    d = R.Drbg("scalar_mul_subgroup/gpu/" + name)
    reduced = boundary_scalars(cp) + [d.below(1 << 64), d.below(1 << 128)]
    unreduced = [cp.r, cp.r + 1, 2 * cp.r + 3, (1 << 256) - 1]
    rinv = pow(1 << 256, -1, cp.r)
    rows = {}
    for mont in (0, 1):
        rows[mont] = [(R.scalar_to_bytes(s, cp, mont=bool(mont)), s % cp.r) for s in reduced]
        rows[mont] += [(s.to_bytes(32, "little"), (s * rinv if mont else s) % cp.r) for s in unreduced]
    return rows


@functools.lru_cache(maxsize=None)
def batch(name, group, n, stride):
    """(point list, its bytes): n points of the subgroup with infinities at the first, middle and last index (n = 1: the
    point alone); stride 0: one base"""
    from oracle import pyref as R

    cp = R.CURVES[name]
    pts = list(distinct_points(name, group, 300)[: n if stride else 1])
    if stride and n >= 3:
        for i in (0, n // 2, n - 1):
            pts[i] = None
    to_bytes = group_ops(cp, group)[0]
    return pts, b"".join(to_bytes(p) for p in pts)


@functools.lru_cache(maxsize=None)
def oracle_product(name, group, index, k):
    """[k] distinct_points[index] by oracle/pyref.py, computed once (both scalar forms of a reduced scalar mean the same k)"""
    from oracle import pyref as R

    cp = R.CURVES[name]
    to_bytes, ref_mul = group_ops(cp, group)
    return to_bytes(ref_mul(distinct_points(name, group, 300)[index], k))


def mul(lib, mlhip, cid, group, flagged, pts, stride, scs, mont, n, psz):
    out = ctypes.create_string_buffer(psz * n)
    if flagged:
        mlhip.check(mlhip.scalar_mul_subgroup(lib, cid, group, pts, stride, scs, mont, n, out))
    else:
        mlhip.check(lib.mlhip_scalar_mul(cid, group, pts, stride, scs, mont, n, out))
    return out.raw


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("curve", list(CURVES))
def test_flagged_call_equals_plain_call_and_oracle(lib, mlhip, curve, group):
    from oracle import pyref as R

    cid, cp = CURVES[curve], R.CURVES[curve]
    psz = 2 * group * cp.fp_bytes
    to_bytes = group_ops(cp, group)[0]
    for n, stride in SHAPES:
        pts, raw = batch(curve, group, n, stride)
        for mont in (0, 1):
            rows = scalar_rows(curve)[mont]
            scs = b"".join(rows[i % len(rows)][0] for i in range(n))
            got = mul(lib, mlhip, cid, group, True, raw, stride, scs, mont, n, psz)
            plain = mul(lib, mlhip, cid, group, False, raw, stride, scs, mont, n, psz)
            assert got == plain, (curve, group, n, stride, mont, [i for i in range(n) if got[i * psz : (i + 1) * psz] != plain[i * psz : (i + 1) * psz]][:8])
            # against the oracle: in the batch of 300 points every scalar of the set once and 16 more indices spread over
            # the batch; in the other shapes (the same kernels, other grids) the first, a middle and the last product
            if (n, stride) == (300, 1):
                checked = sorted(set(range(len(rows))) | {len(rows) + 1 + k * (n - len(rows) - 2) // 15 for k in range(16)})
                assert len(checked) == len(rows) + 16 and checked[-1] == n - 1
            else:
                checked = sorted({0, min(n // 2 + 1, n - 1), n - 1})
            for i in checked:
                want = oracle_product(curve, group, i if stride else 0, rows[i % len(rows)][1]) if pts[i if stride else 0] else bytes(psz)
                assert got[i * psz : (i + 1) * psz] == want, (curve, group, n, stride, mont, i)


@functools.lru_cache(maxsize=None)
def beta(name):
    """the cube root of unity with (beta x, -y) = [x^2]P on G1, from the oracle's own multiplication"""
    from oracle import pyref as R

    cp = R.CURVES[name]
    P = distinct_points(name, 1, 300)[5]
    Q = R.g1_mul(cp, P, cp.x * cp.x)
    b = Q[0] * pow(P[0], -1, cp.p) % cp.p
    assert b != 1 and pow(b, 3, cp.p) == 1 and Q[1] == cp.p - P[1]
    return b


# (BN254 G1 has no point outside the subgroup: E(Fp) has prime order)
OUTSIDE = [("BN254", 2), ("BLS12-381", 1), ("BLS12-381", 2), ("BLS12-377", 1), ("BLS12-377", 2)]


@pytest.mark.parametrize("stride", [1, 0])
@pytest.mark.parametrize("curve,group", OUTSIDE)
def test_point_outside_the_subgroup_shows_the_route(lib, mlhip, curve, group, stride, monkeypatch):
    """a broken promise costs that element alone: rc 0, every other product right; the element itself is the endomorphism's
    value -- (beta x, -y) for s = x^2 on G1, not the product for s = |x| / 6 x^2 on G2 -- and the plain value again with
    MLHIP_SCALAR_MUL_ENDO=0.  stride 0: the point is the one base -- of the split kernel at 300 scalars, of the fixed-base
    table at 4096, where the flag changes nothing."""
    from oracle import pyref as R

    cid, cp = CURVES[curve], R.CURVES[curve]
    T = outside_subgroup_point(curve, group)
    assert T is not None and outside_subgroup_point("BN254", 1) is None
    psz = 2 * group * cp.fp_bytes
    to_bytes, _ = group_ops(cp, group)
    s = cp.x * cp.x if group == 1 else split_modulus(cp)[0]
    assert s < cp.r
    rows = scalar_rows(curve)[0]
    for n in ((65,) if stride else (300, 4096)):
        mid = n // 2
        if stride:
            pts = list(batch(curve, group, n, 1)[0])
            pts[mid] = T
        else:
            pts = [T]
        raw = b"".join(to_bytes(p) for p in pts)
        scs = b"".join(s.to_bytes(32, "little") if i == mid else rows[i % len(rows)][0] for i in range(n))
        got = mul(lib, mlhip, cid, group, True, raw, stride, scs, 0, n, psz)
        plain = mul(lib, mlhip, cid, group, False, raw, stride, scs, 0, n, psz)
        at = lambda b, i: b[i * psz : (i + 1) * psz]
        unreduced = R.g1_mul_unreduced if group == 1 else R.g2_mul_unreduced
        assert at(plain, mid) == to_bytes(unreduced(cp, T, s))
        if stride:
            assert [i for i in range(n) if i != mid and at(got, i) != at(plain, i)] == []
        if n >= 4096:  # the table path: no doubling to save, the flag is ignored
            assert got == plain
            continue
        if group == 1:
            assert at(got, mid) == to_bytes((beta(curve) * T[0] % cp.p, cp.p - T[1]))
        assert at(got, mid) != at(plain, mid)
        monkeypatch.setenv("MLHIP_SCALAR_MUL_ENDO", "0")
        assert mul(lib, mlhip, cid, group, True, raw, stride, scs, 0, n, psz) == plain
        monkeypatch.delenv("MLHIP_SCALAR_MUL_ENDO")


@pytest.mark.parametrize("cid,group", [(1, 1), (2, 1), (0, 2), (1, 2), (2, 2)])
def test_device_form_on_a_busy_stream(lib, mlhip, delay, cid, group):
    """the _device form with the promise through the scenario of tests/test_stream_order_gpu.py: inputs still being produced
    on the stream, outputs overwritten right behind the call, the stream still busy when the call returns"""
    import torch

    import stream_order_cases as S

    class ScalarMulSubgroup(S.ScalarMul):
        def call(self, lib, mlhip, ins, outs, host, stream):
            mlhip.check(mlhip.scalar_mul_subgroup_device(lib, self.cid, self.group, ins[0], self.stride, ins[1], 0, self.n, outs[0], stream))
            return []

        def host_form(self, lib, mlhip, ins, host):
            out = ctypes.create_string_buffer(self.psz * self.n)
            mlhip.check(mlhip.scalar_mul_subgroup(lib, self.cid, self.group, ins[0], self.stride, ins[1], 0, self.n, out))
            return [out.raw]

    lines = []
    outcome = S.run_scenario(lib, mlhip, ScalarMulSubgroup(cid, group, 1, 300), torch.cuda.Stream(), delay, lines.append,
                             "scalar-mul-subgroup-g%d-%s" % (group, S.NAMES[cid]))
    assert outcome.busy and lines


@pytest.mark.parametrize("curve", list(CURVES))
def test_python_mirror_mul_batch_subgroup(mlhip, curve):
    """MulBatchSubgroup of mathlib_amd/driver.py equals MulBatch and the single Mul on generators and their multiples"""
    from mathlib_amd.driver import Curve

    c = Curve(CURVES[curve])
    co = load_golden(curve)["g2_gen_coords"]  # (the mirror has no built-in BLS12-377 G2 generator)
    g2 = c.NewG2FromCoords((int(co[0][0]), int(co[0][1])), (int(co[1][0]), int(co[1][1])))
    g1 = c.GenG1()
    zs = [c.NewZrFromInt(-1), c.NewZrFromInt(1 << 62), c.NewZrFromInt(7), c.GroupOrder]
    for gen in (g1, g2):
        pts = [gen, gen.Mul(c.NewZrFromInt(12345)), gen.Mul(c.NewZrFromInt(3)), gen]
        fast = c.MulBatchSubgroup(pts, zs)
        assert [p.raw for p in fast] == [p.raw for p in c.MulBatch(pts, zs)]
        assert fast[0].raw == gen.Mul(zs[0]).raw and fast[3].raw == bytes(len(gen.raw))
    assert c.MulBatchSubgroup([], []) == []
    with pytest.raises(ValueError):
        c.MulBatchSubgroup([g1], zs)
