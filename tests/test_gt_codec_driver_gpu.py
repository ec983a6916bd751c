"""The Python mirror (mathlib_amd/driver.py) of the Gt wire codec, the membership test and Gt.Inverse: Gt.Inverse,
Curve.NewGtFromBytes and the batch forms NewGtFromBytesBatch / GtBytesBatch / IsInSubGroupBatch / InverseBatch, on values the
mirror computes itself and on the cases of tests/gt_codec_cases.py."""
import pytest

from conftest import load_golden
from gt_codec_cases import inverse_bytes, wires

pytestmark = pytest.mark.gpu

CURVES = {"BN254": 0, "BLS12-381": 1, "BLS12-377": 2}


@pytest.mark.parametrize("curve", list(CURVES))
def test_inverse_and_bytes_round_trip(mlhip, curve):
    from mathlib_amd.driver import Curve

    c = Curve(CURVES[curve])
    co = load_golden(curve)["g2_gen_coords"]  # (the mirror has no built-in BLS12-377 G2 generator)
    g2 = c.NewG2FromCoords((int(co[0][0]), int(co[0][1])), (int(co[1][0]), int(co[1][1])))
    raw = c.Pairing(g2, c.GenG1())  # a Miller value: outside Gt, and still invertible
    gen = c.FExp(raw)
    for g in (gen, raw):
        inv = g.Copy()
        inv.Inverse()
        assert not inv.Equals(g)
        inv.Mul(g)
        assert inv.IsUnity()
        assert c.NewGtFromBytes(g.Bytes()).Equals(g)
    assert c.IsInSubGroupBatch([gen, raw, gen.Exp(c.NewZrFromInt(5))]) == [True, False, True]
    assert c.GtBytesBatch([gen, raw]) == [gen.Bytes(), raw.Bytes()]
    got, st = c.NewGtFromBytesBatch([gen.Bytes(), raw.Bytes()])
    assert st == [0, 3] and got[0].Equals(gen) and got[1].raw == bytes(c.gt_bytes)
    # a x b^-1 == 1, the verifier equation the inverse exists for
    a = gen.Exp(c.NewZrFromInt(77))
    b = c.InverseBatch([a])[0]
    b.Mul(a)
    assert b.IsUnity()
    assert c.NewGtFromBytesBatch([]) == ([], []) and c.GtBytesBatch([]) == [] and c.IsInSubGroupBatch([]) == [] and c.InverseBatch([]) == []


@pytest.mark.parametrize("curve", list(CURVES))
def test_batch_forms_on_the_case_file(mlhip, curve):
    from mathlib_amd.driver import Curve, Gt
    from oracle import pyref as R

    c = Curve(CURVES[curve])
    cp = R.CURVES[curve]
    ws = wires(curve)
    blobs = [w.wire for w in ws]
    zero = bytes(c.gt_bytes)
    want = [R.gt_to_mont_bytes(cp, w.f) if w.f is not None else zero for w in ws]
    gts, st = c.NewGtFromBytesBatch(blobs)
    assert st == [w.status for w in ws]
    assert [g.raw for g in gts] == [v if w.status == 0 else zero for v, w in zip(want, ws)]
    gts0, st0 = c.NewGtFromBytesBatch(blobs, subgroup_check=False)
    assert st0 == [0 if w.f is not None else 1 for w in ws] and [g.raw for g in gts0] == want
    good = [Gt(v, c) for v, w in zip(want, ws) if w.f is not None]
    assert c.GtBytesBatch(good) == [w.wire for w in ws if w.f is not None] == [g.Bytes() for g in good]
    assert c.IsInSubGroupBatch(good) == [w.status == 0 for w in ws if w.f is not None]
    assert [g.raw for g in c.InverseBatch(good)] == [inverse_bytes(curve)[w.label] for w in ws if w.f is not None]
    for w in ws:
        if w.f is None:  # the reference panics; the single form raises, without the subgroup check as gnark's SetBytes
            with pytest.raises(ValueError):
                c.NewGtFromBytes(w.wire)
        else:
            assert c.NewGtFromBytes(w.wire).raw == R.gt_to_mont_bytes(cp, w.f)
    with pytest.raises(ValueError):
        c.NewGtFromBytes(blobs[0][:-1])
