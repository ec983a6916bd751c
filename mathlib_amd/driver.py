"""Host-side mirror of the reference's plugin boundary for the hot path (driver/math.go:49-360).

The reference is Go; this image has no Go toolchain, so the binding a maintainer would add
(`driver/hip`, shown in INTEGRATION.md and shipped as source under go/driver/hip) cannot run
here.  This module restates the same interface in Python over the same C ABI -- same method
names, argument order and error behaviour -- so the parity tests read like math_test.go:

    Curve.MultiScalarMul(a []G1, b []Zr) G1      driver/math.go:169-170   -> mlhip_msm_g1
    Curve.Pairing(G2, G1) Gt                     driver/math.go:50-52     -> mlhip_miller_loop (ppp=1)
    Curve.Pairing2(p2a, p2b G2, p1a, p1b G1) Gt  driver/math.go:54-55     -> mlhip_miller_loop (ppp=2)
    Curve.FExp(Gt) Gt                            driver/math.go:56-57     -> mlhip_final_exp
    G1.Mul / G2.Mul / Gt.Mul / G1.Add ...        driver/math.go:249-360   -> n=1 MSM, group helpers
    Gt.Exp(Zr) Gt                                driver/math.go:358-359   -> mlhip_gt_exp
  additive: MultiScalarMulG2, PairingBatch, PairingProduct, MultiScalarMulBatch, MultiScalarMulG2Batch,
  Mul2Batch.

Only plumbing happens here (byte packing, Montgomery <-> integer conversion for printing and wire
bytes).  All group / field arithmetic is done by libmlhip.so; nothing under oracle/ is imported.
Like the reference's drivers, failures raise (the Go drivers panic: driver/gurvy/bn254.go:249-251).
"""
from __future__ import annotations

import ctypes
import hashlib
import secrets
from typing import List, Sequence

from . import _lib
from ._lib import CURVE_BLS12_377, CURVE_BLS12_381, CURVE_BN254, GROUP_G1, GROUP_G2, check, load, msm_batch
from ._lib import concrete as _concrete

_X381 = -0xD201000000010000
_X377 = 0x8508C00000000001
_T254 = 4965661367192848881


def _bls_p(x):
    return ((x - 1) ** 2 * (x**4 - x**2 + 1)) // 3 + x


_PARAMS = {
    CURVE_BN254: dict(
        name="BN254",
        p=36 * _T254**4 + 36 * _T254**3 + 24 * _T254**2 + 6 * _T254 + 1,
        r=36 * _T254**4 + 36 * _T254**3 + 18 * _T254**2 + 6 * _T254 + 1,
        g1=(1, 2),
        g2=(
            (10857046999023057135944570762232829481370756359578518086990519993285655852781,
             11559732032986387107991004021392285783925812861821192530917403151452391805634),
            (8495653923123431417604973247489272438418190587263600148770280649306958101930,
             4082367875863433681332203403145435568316851327593401208105741076214120093531),
        ),
        zcash_flags=False,
    ),
    CURVE_BLS12_381: dict(
        name="BLS12_381",
        p=_bls_p(_X381),
        r=_X381**4 - _X381**2 + 1,
        g1=(
            3685416753713387016781088315183077757961620795782546409894578378688607592378376318836054947676345821548104185464507,
            1339506544944476473020471379941921221584933875938349620426543736416511423956333506472724655353366534992391756441569,
        ),
        g2=(
            (0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
             0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
            (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
             0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE),
        ),
        zcash_flags=True,
    ),
    CURVE_BLS12_377: dict(
        name="BLS12_377",
        p=_bls_p(_X377),
        r=_X377**4 - _X377**2 + 1,
        g1=(
            81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695,
            241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030,
        ),
        g2=None,  # supplied by the caller (NewG2FromCoords); gnark's generator is not in the reference tree
        zcash_flags=True,
    ),
}


class Zr:
    """Scalar.  Like the reference's BaseZr (driver/common/big.go:41-137) the value may be negative or
    >= r between operations; it is reduced mod r where the reference reduces (Bytes, and on entry to
    MultiScalarMul via fr.Element.SetBigInt: driver/gurvy/bn254.go:239)."""

    __slots__ = ("v", "curve")

    def __init__(self, v: int, curve: "Curve"):
        self.v = int(v)
        self.curve = curve

    def Plus(self, o: "Zr") -> "Zr":
        return Zr(self.v + o.v, self.curve)

    def Minus(self, o: "Zr") -> "Zr":
        return Zr(self.v - o.v, self.curve)

    def Mul(self, o: "Zr") -> "Zr":
        return Zr(self.v * o.v % self.curve.r, self.curve)

    def Neg(self) -> "Zr":
        return Zr(-self.v, self.curve)

    def Equals(self, o: "Zr") -> bool:
        return (self.v - o.v) % self.curve.r == 0

    def Copy(self) -> "Zr":
        return Zr(self.v, self.curve)

    def Bytes(self) -> bytes:
        return (self.v % self.curve.r).to_bytes(32, "big")

    def le_bytes(self, mont: bool = False) -> bytes:
        """32-byte little-endian limbs as handed to the C ABI (fr.Element layout when mont)."""
        s = self.v % self.curve.r
        if mont:
            s = s * (1 << 256) % self.curve.r
        return s.to_bytes(32, "little")


class _Element:
    __slots__ = ("raw", "curve")

    def __init__(self, raw: bytes, curve: "Curve"):
        self.raw = bytes(raw)
        self.curve = curve

    def Equals(self, o) -> bool:
        return self.raw == o.raw  # affine Montgomery coordinates are canonical

    def Copy(self):
        return type(self)(self.raw, self.curve)


class G1(_Element):
    def IsInfinity(self) -> bool:
        return not any(self.raw)

    def Mul(self, s: Zr) -> "G1":
        return self.curve.MultiScalarMul([self], [s])

    def Mul2(self, e: Zr, Q: "G1", f: Zr) -> "G1":
        return self.curve.MultiScalarMul([self, Q], [e, f])

    def Add(self, o: "G1") -> None:
        out = ctypes.create_string_buffer(self.curve.g1_bytes)
        check(load().mlhip_g1_sum(self.curve.id, self.raw + o.raw, 2, out))
        self.raw = out.raw

    def Neg(self) -> None:
        if self.IsInfinity():
            return
        n = self.curve.fp_bytes
        y = int.from_bytes(self.raw[n:], "little")
        self.raw = self.raw[:n] + ((self.curve.p - y) % self.curve.p).to_bytes(n, "little")

    def Sub(self, o: "G1") -> None:
        t = o.Copy()
        t.Neg()
        self.Add(t)

    def coords(self):
        if self.IsInfinity():
            return None
        c = self.curve
        return tuple(c._from_mont(self.raw[i * c.fp_bytes : (i + 1) * c.fp_bytes]) for i in range(2))

    def Bytes(self) -> bytes:
        """uncompressed wire form (gnark RawBytes; reference bls12-381.go:286-290)"""
        c = self.curve
        n = c.fp_bytes
        xy = self.coords()
        if xy is None:
            out = bytearray(2 * n)
            out[0] |= 0x40
            return bytes(out)
        return xy[0].to_bytes(n, "big") + xy[1].to_bytes(n, "big")

    def Compressed(self) -> bytes:
        c = self.curve
        n = c.fp_bytes
        xy = self.coords()
        if c.zcash_flags:
            if xy is None:
                return bytes([0xC0]) + bytes(n - 1)
            out = bytearray(xy[0].to_bytes(n, "big"))
            out[0] |= 0x80 | (0x20 if xy[1] > (c.p - 1) // 2 else 0)
            return bytes(out)
        if xy is None:
            return bytes([0x40]) + bytes(n - 1)
        out = bytearray(xy[0].to_bytes(n, "big"))
        out[0] |= 0xC0 if xy[1] > (c.p - 1) // 2 else 0x80
        return bytes(out)

    def String(self) -> str:
        xy = self.coords()
        return "(0,0)" if xy is None else "(%d,%d)" % xy


class G2(_Element):
    def IsInfinity(self) -> bool:
        return not any(self.raw)

    def Mul(self, s: Zr) -> "G2":
        return self.curve.MultiScalarMulG2([self], [s])

    def Add(self, o: "G2") -> None:
        out = ctypes.create_string_buffer(self.curve.g2_bytes)
        check(load().mlhip_g2_sum(self.curve.id, self.raw + o.raw, 2, out))
        self.raw = out.raw

    def coords(self):
        if self.IsInfinity():
            return None
        c = self.curve
        v = [c._from_mont(self.raw[i * c.fp_bytes : (i + 1) * c.fp_bytes]) for i in range(4)]
        return ((v[0], v[1]), (v[2], v[3]))

    def Bytes(self) -> bytes:
        """uncompressed wire form: X.A1 | X.A0 | Y.A1 | Y.A0, big-endian"""
        c = self.curve
        n = c.fp_bytes
        q = self.coords()
        if q is None:
            out = bytearray(4 * n)
            out[0] |= 0x40
            return bytes(out)
        return b"".join(v.to_bytes(n, "big") for v in (q[0][1], q[0][0], q[1][1], q[1][0]))

    def Compressed(self) -> bytes:
        """compressed wire form X.A1 | X.A0; the sign bit follows gnark's E2 rule (A1 decides unless zero)"""
        c = self.curve
        n = c.fp_bytes
        q = self.coords()
        zcash = c.id != 0
        if q is None:
            out = bytearray(2 * n)
            out[0] = 0xC0 if zcash else 0x40
            return bytes(out)
        out = bytearray(q[0][1].to_bytes(n, "big") + q[0][0].to_bytes(n, "big"))
        half = (c.p - 1) // 2
        big = q[1][1] > half if q[1][1] else q[1][0] > half
        out[0] |= (0x80 | (0x20 if big else 0)) if zcash else (0xC0 if big else 0x80)
        return bytes(out)


class Gt(_Element):
    def Mul(self, o: "Gt") -> None:
        out = ctypes.create_string_buffer(self.curve.gt_bytes)
        check(load().mlhip_gt_mul(self.curve.id, self.raw, o.raw, 1, out))
        self.raw = out.raw

    def Exp(self, x: "Zr") -> "Gt":
        """driver/math.go:358-359 / bls12-381.go:399-407"""
        c = self.curve
        out = ctypes.create_string_buffer(c.gt_bytes)
        check(load().mlhip_gt_exp(c.id, self.raw, x.le_bytes(c.scalars_mont), 1 if c.scalars_mont else 0, 1, out))
        return Gt(out.raw, c)

    def Inverse(self) -> None:
        """in place, as Mul; any Fp12 value, the inverse of 0 is 0 (bls12-381.go:413-415)"""
        out = ctypes.create_string_buffer(self.curve.gt_bytes)
        check(load().mlhip_gt_inverse(self.curve.id, self.raw, 1, out))
        self.raw = out.raw

    def IsUnity(self) -> bool:
        return self.raw == self.curve._gt_one

    def Bytes(self) -> bytes:
        """gnark GT.Bytes(): 12 big-endian Fp, C1.B2.A1 first ... C0.B0.A0 last"""
        c = self.curve
        n = c.fp_bytes
        v = [c._from_mont(self.raw[i * n : (i + 1) * n]) for i in range(12)]
        return b"".join(x.to_bytes(n, "big") for x in reversed(v))


class Curve:
    """One curve of the HIP backend (the reference registers one driver.Curve per entry of
    math.Curves, math.go:142-255).  Nothing touches the GPU until a hot method is called."""

    def __init__(self, curve_id: int, window_c: int = 0, scalars_mont: bool = True):
        prm = _PARAMS[curve_id]
        self.id = curve_id
        self.name = prm["name"]
        self.p, self.r = prm["p"], prm["r"]
        self.zcash_flags = prm["zcash_flags"]
        self.window_c = window_c
        # the gurvy BLS12-381 driver hands fr.Element (Montgomery) scalars to MultiExp (bls12-381.go:772)
        self.scalars_mont = scalars_mont
        self.fp_bytes, self.g1_bytes, self.g2_bytes, self.gt_bytes = _lib.sizes(curve_id)
        self.Rm = 1 << (8 * self.fp_bytes)
        self._Rinv = pow(self.Rm, -1, self.p)
        self._gt_one = self._to_mont(1) + bytes(11 * self.fp_bytes)
        self.GroupOrder = Zr(self.r, self)
        self._g1 = prm["g1"]
        self._g2 = prm["g2"]

    # ---- plumbing
    def _to_mont(self, a: int) -> bytes:
        return (a % self.p * self.Rm % self.p).to_bytes(self.fp_bytes, "little")

    def _from_mont(self, b: bytes) -> int:
        return int.from_bytes(b, "little") * self._Rinv % self.p

    def NewG1FromCoords(self, x: int, y: int) -> G1:
        return G1(self._to_mont(x) + self._to_mont(y), self)

    def NewG2FromCoords(self, x, y) -> G2:
        return G2(b"".join(self._to_mont(v) for v in (x[0], x[1], y[0], y[1])), self)

    _CODEC_ERRORS = {1: "invalid point encoding", 2: "invalid point: not on the curve", 3: "invalid point: subgroup check failed"}

    def _from_wire(self, group: int, b: bytes, compressed: bool):
        size = self.g1_bytes if group == 1 else self.g2_bytes
        out = ctypes.create_string_buffer(size)
        st = ctypes.create_string_buffer(1)
        if len(b) != (size // 2 if compressed else size):
            raise ValueError("set bytes failed [invalid length]")
        fn = load().mlhip_g1_from_bytes if group == 1 else load().mlhip_g2_from_bytes
        check(fn(self.id, bytes(b), 1, 1 if compressed else 0, 1, out, st))
        if st.raw[0]:
            # the reference panics ("set bytes failed [...]"), the facade turns it into an error (math.go:761-832)
            raise ValueError("set bytes failed [%s]" % self._CODEC_ERRORS[st.raw[0]])
        return G1(out.raw, self) if group == 1 else G2(out.raw, self)

    def _g1_from_wire(self, b: bytes, compressed: bool) -> G1:
        return self._from_wire(1, b, compressed)

    def NewG2FromBytes(self, b: bytes) -> G2:
        """bls12-381.go:541-549"""
        return self._from_wire(2, b, False)

    def NewG2FromCompressed(self, b: bytes) -> G2:
        """bls12-381.go:561-569"""
        return self._from_wire(2, b, True)

    def NewGtFromBytes(self, b: bytes) -> Gt:
        """gnark's GT.SetBytes: decoded without the subgroup check, a coordinate >= p raises (bls12-381.go:571-579)"""
        gts, st = self.NewGtFromBytesBatch([b], subgroup_check=False)
        if st[0]:
            raise ValueError("set bytes failed [invalid fp.Element encoding]")
        return gts[0]

    def NewGtFromBytesBatch(self, blobs: Sequence[bytes], subgroup_check: bool = True):
        """(values, statuses) of len(blobs) encodings in one call (mlhip_gt_from_bytes): status 0 ok, 1 malformed, 3 not in Gt
        (with the check only); a value whose status is not 0 is all zero"""
        n = len(blobs)
        if any(len(b) != self.gt_bytes for b in blobs):
            raise ValueError("set bytes failed [invalid length]")
        if n == 0:
            return [], []
        out = ctypes.create_string_buffer(self.gt_bytes * n)
        st = ctypes.create_string_buffer(n)
        check(load().mlhip_gt_from_bytes(self.id, b"".join(bytes(b) for b in blobs), n, 1 if subgroup_check else 0, out, st))
        return [Gt(out.raw[i * self.gt_bytes : (i + 1) * self.gt_bytes], self) for i in range(n)], list(st.raw)

    def GtBytesBatch(self, gts: Sequence[Gt]) -> List[bytes]:
        """Gt.Bytes of every value in one call (mlhip_gt_to_bytes)"""
        n = len(gts)
        if n == 0:
            return []
        out = ctypes.create_string_buffer(self.gt_bytes * n)
        check(load().mlhip_gt_to_bytes(self.id, b"".join(g.raw for g in gts), n, out))
        return [out.raw[i * self.gt_bytes : (i + 1) * self.gt_bytes] for i in range(n)]

    def IsInSubGroupBatch(self, gts: Sequence[Gt]) -> List[bool]:
        """is each value a member of Gt (order r)?  What ExpBatchGt asks its caller to know (mlhip_gt_is_member)"""
        n = len(gts)
        if n == 0:
            return []
        st = ctypes.create_string_buffer(n)
        check(load().mlhip_gt_is_member(self.id, b"".join(g.raw for g in gts), n, st))
        return [b == 0 for b in st.raw]

    def InverseBatch(self, gts: Sequence[Gt]) -> List[Gt]:
        """Gt.Inverse of every value in one call, not in place (mlhip_gt_inverse)"""
        n = len(gts)
        if n == 0:
            return []
        out = ctypes.create_string_buffer(self.gt_bytes * n)
        check(load().mlhip_gt_inverse(self.id, b"".join(g.raw for g in gts), n, out))
        return [Gt(out.raw[i * self.gt_bytes : (i + 1) * self.gt_bytes], self) for i in range(n)]

    def NewG1FromBytes(self, b: bytes) -> G1:
        """uncompressed wire form, subgroup-checked (driver/gurvy/bls12381/bls12-381.go:531-539)"""
        return self._g1_from_wire(b, False)

    def NewG1FromCompressed(self, b: bytes) -> G1:
        """compressed wire form (bls12-381.go:551-559)"""
        return self._g1_from_wire(b, True)

    def NewG1(self) -> G1:
        return G1(bytes(self.g1_bytes), self)

    def NewG2(self) -> G2:
        return G2(bytes(self.g2_bytes), self)

    def NewZrFromInt(self, i: int) -> Zr:
        return Zr(i, self)

    def NewRandomZr(self, rng=None) -> Zr:
        """driver/common/curve.go:77-84 (crypto/rand there; a caller-seeded stream here when given)"""
        if rng is None:
            return Zr(secrets.randbelow(self.r), self)
        return Zr(rng(self.r), self)

    def HashToZr(self, data: bytes) -> Zr:
        """SHA-256 mod r, driver/common/curve.go:86-92"""
        return Zr(int.from_bytes(hashlib.sha256(data).digest(), "big") % self.r, self)

    def GenG1(self) -> G1:
        return self.NewG1FromCoords(*self._g1)

    def GenG2(self) -> G2:
        if self._g2 is None:
            raise ValueError("no built-in G2 generator for %s; use NewG2FromCoords" % self.name)
        return self.NewG2FromCoords(*self._g2)

    def GenGt(self) -> Gt:
        """FExp(Pairing(GenG2, GenG1)), reference bls12-381.go:490-497"""
        return self.FExp(self.Pairing(self.GenG2(), self.GenG1()))

    # ---- hot path
    def _scalars(self, b: Sequence[Zr]) -> bytes:
        return b"".join(z.le_bytes(self.scalars_mont) for z in b)

    def MultiScalarMul(self, a: Sequence[G1], b: Sequence[Zr]) -> G1:
        """math.go:960-969 raises (index out of range) when len(b) < len(a); mirrored."""
        if len(b) < len(a):
            raise IndexError("MultiScalarMul: fewer scalars than points")
        out = ctypes.create_string_buffer(self.g1_bytes)
        if len(b) != len(a):
            # gnark's MultiExp errors on a length mismatch and the driver drops the error: identity
            return self.NewG1()
        pts = b"".join(p.raw for p in a)
        check(load().mlhip_msm_g1(self.id, pts, self._scalars(b), 1 if self.scalars_mont else 0, len(a), self.window_c, out))
        return G1(out.raw, self)

    def MultiScalarMulG2(self, a: Sequence[G2], b: Sequence[Zr]) -> G2:
        if len(b) < len(a):
            raise IndexError("MultiScalarMulG2: fewer scalars than points")
        out = ctypes.create_string_buffer(self.g2_bytes)
        if len(b) != len(a):
            return self.NewG2()
        pts = b"".join(p.raw for p in a)
        check(load().mlhip_msm_g2(self.id, pts, self._scalars(b), 1 if self.scalars_mont else 0, len(a), self.window_c, out))
        return G2(out.raw, self)

    def _msm_short(self, group: int, a, b: Sequence[Zr], bits: int, name: str):
        if len(b) < len(a):
            raise IndexError("%s: fewer scalars than points" % name)
        if len(b) != len(a):
            return None
        return _lib.msm_bits(self.id, group, b"".join(p.raw for p in a), self._scalars(b), self.scalars_mont, bits, len(a),
                             self.window_c)

    def MultiScalarMulShort(self, a: Sequence[G1], b: Sequence[Zr], bits: int) -> G1:
        """MultiScalarMul for scalars known to be below 2^bits (additive; mlhip_msm_bits): sum_i [b_i mod 2^bits] a_i, the
        same point as MultiScalarMul when the scalars keep the promise, in fewer windows.  bits = 0: full width.  Same length
        rules as MultiScalarMul."""
        raw = self._msm_short(GROUP_G1, a, b, bits, "MultiScalarMulShort")
        return self.NewG1() if raw is None else G1(raw, self)

    def MultiScalarMulG2Short(self, a: Sequence[G2], b: Sequence[Zr], bits: int) -> G2:
        """the same in G2"""
        raw = self._msm_short(GROUP_G2, a, b, bits, "MultiScalarMulG2Short")
        return self.NewG2() if raw is None else G2(raw, self)

    def SumG1(self, points: Sequence[G1]) -> G1:
        """points[0] + points[1] + ...: G1.Add in a loop (driver/gurvy/bls12381/bls12-381.go, Add) as one call; long lists
        are summed on the device (mlhip_g1_sum, MLHIP_SUM_DEVICE_MIN).  An empty list gives the identity."""
        out = ctypes.create_string_buffer(self.g1_bytes)
        check(load().mlhip_g1_sum(self.id, b"".join(p.raw for p in points), len(points), out))
        return G1(out.raw, self)

    def SumG2(self, points: Sequence[G2]) -> G2:
        """the same in G2 (mlhip_g2_sum)"""
        out = ctypes.create_string_buffer(self.g2_bytes)
        check(load().mlhip_g2_sum(self.id, b"".join(p.raw for p in points), len(points), out))
        return G2(out.raw, self)

    def MultiScalarMulG1G2(self, a1: Sequence[G1], a2: Sequence[G2], b: Sequence[Zr]):
        """(MultiScalarMul(a1, b), MultiScalarMulG2(a2, b)) for ONE scalar vector: sorted once on the device, both groups
        accumulate from the same lists (additive; BASELINE configs[3]).  Same length rules as MultiScalarMul."""
        if len(b) < len(a1) or len(b) < len(a2):
            raise IndexError("MultiScalarMulG1G2: fewer scalars than points")
        if len(a1) != len(a2) or len(b) != len(a1):
            return self.NewG1(), self.NewG2()
        o1 = ctypes.create_string_buffer(self.g1_bytes)
        o2 = ctypes.create_string_buffer(self.g2_bytes)
        check(load().mlhip_msm_g1g2(self.id, b"".join(p.raw for p in a1), b"".join(p.raw for p in a2), self._scalars(b),
                                    1 if self.scalars_mont else 0, len(a1), self.window_c, o1, o2))
        return G1(o1.raw, self), G2(o2.raw, self)

    def _msm_batch(self, group: int, a_lists, b_lists, name: str, identity, subgroup: bool = False) -> list:
        """one mlhip_msm_batch call for every segment; each keeps MultiScalarMul's length rules (fewer scalars than points
        raises, more gives the identity: an empty segment).  subgroup: every point is promised to be in G1 / G2"""
        if len(a_lists) != len(b_lists):
            raise ValueError("%s: %d point lists, %d scalar lists" % (name, len(a_lists), len(b_lists)))
        lengths, pts, scs = [], [], []
        for a, b in zip(a_lists, b_lists):
            if len(b) < len(a):
                raise IndexError("%s: fewer scalars than points" % name)
            if len(b) != len(a):
                lengths.append(0)
                continue
            lengths.append(len(a))
            pts.extend(p.raw for p in a)
            scs.append(self._scalars(b))
        if not lengths:
            return []
        raw = msm_batch(self.id, group, b"".join(pts), b"".join(scs), self.scalars_mont, lengths, subgroup)
        return [identity(r) for r in raw]

    def MultiScalarMulBatch(self, a_lists: Sequence[Sequence[G1]], b_lists: Sequence[Sequence[Zr]], subgroup: bool = False) -> List[G1]:
        """out[i] = MultiScalarMul(a_lists[i], b_lists[i]) for many small MSMs in one device call (include/mlhip.h:
        mlhip_msm_batch).  subgroup=True: MultiScalarMulBatchSubgroup"""
        return self._msm_batch(GROUP_G1, a_lists, b_lists, "MultiScalarMulBatch", lambda r: G1(r, self), subgroup)

    def MultiScalarMulG2Batch(self, a_lists: Sequence[Sequence[G2]], b_lists: Sequence[Sequence[Zr]], subgroup: bool = False) -> List[G2]:
        return self._msm_batch(GROUP_G2, a_lists, b_lists, "MultiScalarMulG2Batch", lambda r: G2(r, self), subgroup)

    def MultiScalarMulBatchSubgroup(self, a_lists: Sequence[Sequence[G1]], b_lists: Sequence[Sequence[Zr]]) -> List[G1]:
        """MultiScalarMulBatch for points the caller knows to be in G1 (decoded with the subgroup check, issuer keys,
        generators, outputs of earlier MSMs): the same results with half of the chunks' doublings, from the curve's
        endomorphism and a split of every scalar (mlhip_msm_batch_subgroup).  A point outside the subgroup gives an undefined
        result for its own segment; MultiScalarMulBatch accepts any point of the curve.  On BN254 every point of the curve is
        in G1 (the lattice split of DESIGN.md section 20 runs): only a point that is not on the curve breaks the promise."""
        return self.MultiScalarMulBatch(a_lists, b_lists, subgroup=True)

    def MultiScalarMulG2BatchSubgroup(self, a_lists: Sequence[Sequence[G2]], b_lists: Sequence[Sequence[Zr]]) -> List[G2]:
        """the same for points known to be in G2"""
        return self.MultiScalarMulG2Batch(a_lists, b_lists, subgroup=True)

    def SumG1Batch(self, lists: Sequence[Sequence[G1]]) -> List[G1]:
        """out[i] = SumG1(lists[i]) for many lists in one device call (include/mlhip.h: mlhip_msm_batch with
        MLHIP_SCALARS_UNIT; include/mlhip_sum_batch.h).  An empty list gives the identity."""
        raw = _lib.sum_batch(self.id, GROUP_G1, b"".join(p.raw for a in lists for p in a), [len(a) for a in lists])
        return [G1(r, self) for r in raw]

    def SumG2Batch(self, lists: Sequence[Sequence[G2]]) -> List[G2]:
        """the same in G2"""
        raw = _lib.sum_batch(self.id, GROUP_G2, b"".join(p.raw for a in lists for p in a), [len(a) for a in lists])
        return [G2(r, self) for r in raw]

    def Mul2Batch(self, g: Sequence[G1], e: Sequence[Zr], q: Sequence[G1], f: Sequence[Zr]) -> List[G1]:
        """out[i] = g[i].Mul2(e[i], q[i], f[i]): segments of two pairs in one mlhip_msm_batch call"""
        if not (len(g) == len(e) == len(q) == len(f)):
            raise ValueError("Mul2Batch: length mismatch")
        return self.MultiScalarMulBatch([[g[i], q[i]] for i in range(len(g))], [[e[i], f[i]] for i in range(len(g))])

    def NewBases(self, points: Sequence[G1]) -> "Bases":
        """Upload a G1 point table once; Bases.MultiScalarMul(scalars) then moves only the scalars."""
        return Bases(self, points)

    def NewBasesG2(self, points: Sequence[G2]) -> "Bases":
        """The same for a G2 point table (a Groth16 prover's B2 query)."""
        return Bases(self, points, GROUP_G2)

    def NewBasesSet(self, *members: "Bases") -> "BasesSet":
        """A set of 1..4 resident tables of this curve, any mix of G1 and G2: BasesSet.MultiScalarMul(scalars) returns every
        member's MSM over one scalar vector from one upload and one sort per tile (include/mlhip.h: mlhip_bases_set_create)."""
        return BasesSet(self, members)

    def NewG2Prepared(self, points: Sequence[G2]) -> "G2Prepared":
        """Prepare fixed G2 points once (the generator and an issuer key, say); G2Prepared.PairingBatch(g1_lists) then runs
        the verifier's Pairing2 + FExp over many proofs without any G2 arithmetic (include/mlhip.h: mlhip_g2_prepared_*)."""
        return G2Prepared(self, points)

    def Pairing(self, p2: G2, p1: G1) -> Gt:
        """Miller loop only, like the gurvy drivers (bls12-381.go:448-455); compare after FExp."""
        out = ctypes.create_string_buffer(self.gt_bytes)
        check(load().mlhip_miller_loop(self.id, p1.raw, p2.raw, 1, 1, out))
        return Gt(out.raw, self)

    def Pairing2(self, p2a: G2, p2b: G2, p1a: G1, p1b: G1) -> Gt:
        out = ctypes.create_string_buffer(self.gt_bytes)
        check(load().mlhip_miller_loop(self.id, p1a.raw + p1b.raw, p2a.raw + p2b.raw, 2, 1, out))
        return Gt(out.raw, self)

    def FExp(self, a: Gt) -> Gt:
        out = ctypes.create_string_buffer(self.gt_bytes)
        check(load().mlhip_final_exp(self.id, a.raw, 1, out))
        return Gt(out.raw, self)

    def PairingBatch(self, g2s: Sequence[G2], g1s: Sequence[G1]) -> List[Gt]:
        """out[i] = FExp(Pairing(g2s[i], g1s[i])) -- additive batch entry point."""
        if len(g2s) != len(g1s):
            raise ValueError("PairingBatch: length mismatch")
        n = len(g1s)
        out = ctypes.create_string_buffer(self.gt_bytes * max(n, 1))
        check(load().mlhip_pairing_batch(self.id, b"".join(p.raw for p in g1s), b"".join(q.raw for q in g2s), n, out))
        return [Gt(out.raw[i * self.gt_bytes : (i + 1) * self.gt_bytes], self) for i in range(n)]


    def MulBatch(self, points: Sequence, scalars: Sequence[Zr]) -> list:
        """out[i] = points[i].Mul(scalars[i]) for G1 or G2 points, one launch (additive; SURVEY 8f row 3: the batched form of
        G1.Mul / G2.Mul, bls12-381.go:238-247, :342-351)."""
        if len(points) != len(scalars):
            raise ValueError("MulBatch: length mismatch")
        n = len(points)
        if n == 0:
            return []
        cls = type(points[0])
        group, size = (GROUP_G1, self.g1_bytes) if cls is G1 else (GROUP_G2, self.g2_bytes)
        out = ctypes.create_string_buffer(size * n)
        check(load().mlhip_scalar_mul(self.id, group, b"".join(p.raw for p in points), 1, self._scalars(scalars),
                                      1 if self.scalars_mont else 0, n, out))
        return [cls(out.raw[i * size : (i + 1) * size], self) for i in range(n)]

    def MulBatchSubgroup(self, points: Sequence, scalars: Sequence[Zr]) -> list:
        """MulBatch for points the caller knows to be in G1 / G2 (decoded with the subgroup check, MSM outputs over checked
        bases, generators and their multiples): the same results from the curve's endomorphism and a split of the scalar
        (mlhip_scalar_mul_subgroup).  A point outside the subgroup gives an undefined result for its own product; G1.Mul,
        G2.Mul and MulBatch accept any point of the curve.  On BN254 every point of the curve is in G1 (the lattice split of
        DESIGN.md section 20 runs): only a point that is not on the curve breaks the promise there."""
        if len(points) != len(scalars):
            raise ValueError("MulBatchSubgroup: length mismatch")
        n = len(points)
        if n == 0:
            return []
        cls = type(points[0])
        group, size = (GROUP_G1, self.g1_bytes) if cls is G1 else (GROUP_G2, self.g2_bytes)
        out = ctypes.create_string_buffer(size * n)
        check(_lib.scalar_mul_subgroup(load(), self.id, group, b"".join(p.raw for p in points), 1, self._scalars(scalars),
                                  1 if self.scalars_mont else 0, n, out))
        return [cls(out.raw[i * size : (i + 1) * size], self) for i in range(n)]

    def BaseMulBatch(self, base, scalars: Sequence[Zr]) -> list:
        """out[i] = base.Mul(scalars[i]): one base (a generator, a Pedersen base), many scalars.  From 2^12 scalars on the
        library multiplies through a table of the base's multiples that it keeps on the device for later calls with the
        same base (mlhip_scalar_mul, point_stride 0)."""
        n = len(scalars)
        if n == 0:
            return []
        cls = type(base)
        group, size = (GROUP_G1, self.g1_bytes) if cls is G1 else (GROUP_G2, self.g2_bytes)
        out = ctypes.create_string_buffer(size * n)
        check(load().mlhip_scalar_mul(self.id, group, base.raw, 0, self._scalars(scalars), 1 if self.scalars_mont else 0, n, out))
        return [cls(out.raw[i * size : (i + 1) * size], self) for i in range(n)]

    def ExpBatch(self, gts: Sequence[Gt], scalars: Sequence[Zr]) -> List[Gt]:
        """out[i] = gts[i].Exp(scalars[i]), one launch (additive; SURVEY 8f row 2: Gt.Exp, bls12-381.go:399-407)."""
        if len(gts) != len(scalars):
            raise ValueError("ExpBatch: length mismatch")
        n = len(gts)
        if n == 0:
            return []
        out = ctypes.create_string_buffer(self.gt_bytes * n)
        check(load().mlhip_gt_exp(self.id, b"".join(g.raw for g in gts), self._scalars(scalars), 1 if self.scalars_mont else 0, n, out))
        return [Gt(out.raw[i * self.gt_bytes : (i + 1) * self.gt_bytes], self) for i in range(n)]

    def ExpBatchGt(self, gts: Sequence[Gt], scalars: Sequence[Zr]) -> List[Gt]:
        """ExpBatch for values the caller knows to be MEMBERS of Gt (FExp outputs, GenGt, products and powers of these): the
        same results from cyclotomic squarings and a Frobenius split of the scalar (mlhip_gt_exp_cyclo).  A value outside
        Gt -- a raw Pairing / Pairing2 output before FExp -- gives an undefined result; Gt.Exp and ExpBatch accept any."""
        if len(gts) != len(scalars):
            raise ValueError("ExpBatchGt: length mismatch")
        n = len(gts)
        if n == 0:
            return []
        out = ctypes.create_string_buffer(self.gt_bytes * n)
        check(load().mlhip_gt_exp_cyclo(self.id, b"".join(g.raw for g in gts), self._scalars(scalars), 1 if self.scalars_mont else 0, n, out))
        return [Gt(out.raw[i * self.gt_bytes : (i + 1) * self.gt_bytes], self) for i in range(n)]

    def MillerLoopProducts(self, g2_lists: Sequence[Sequence[G2]], g1_lists: Sequence[Sequence[G1]]) -> List[Gt]:
        """out[k] = prod_j Pairing(g2_lists[k][j], g1_lists[k][j]): K products of m pairs each, any m, in one device call
        (include/mlhip.h: "products of any length", mlhip_miller_loop_products); not final-exponentiated, like Pairing.  Every
        product has the same length: a shorter one is padded with pairs at infinity."""
        if len(g2_lists) != len(g1_lists):
            raise ValueError("MillerLoopProducts: %d G2 lists, %d G1 lists" % (len(g2_lists), len(g1_lists)))
        n = len(g1_lists)
        if n == 0:
            return []
        m = len(g1_lists[0])
        if m == 0 or any(len(a) != m or len(b) != m for a, b in zip(g1_lists, g2_lists)):
            raise ValueError("MillerLoopProducts: every product takes the same number (at least one) of G1 and of G2 points")
        raw = _lib.miller_loop_products(self.id, b"".join(p.raw for l in g1_lists for p in l),
                                        b"".join(q.raw for l in g2_lists for q in l), m, n)
        return [Gt(raw[i * self.gt_bytes : (i + 1) * self.gt_bytes], self) for i in range(n)]

    def PairingProducts(self, g2_lists: Sequence[Sequence[G2]], g1_lists: Sequence[Sequence[G1]]) -> List[Gt]:
        """out[k] = FExp(prod_j Pairing(g2_lists[k][j], g1_lists[k][j])): FExp of MillerLoopProducts, through mlhip_final_exp"""
        ml = self.MillerLoopProducts(g2_lists, g1_lists)
        n = len(ml)
        if n == 0:
            return []
        out = ctypes.create_string_buffer(self.gt_bytes * n)
        check(load().mlhip_final_exp(self.id, b"".join(g.raw for g in ml), n, out))
        return [Gt(out.raw[i * self.gt_bytes : (i + 1) * self.gt_bytes], self) for i in range(n)]

    def PairingProduct(self, g2s: Sequence[G2], g1s: Sequence[G1]) -> Gt:
        """FExp(prod_i Pairing(g2s[i], g1s[i])) with one shared final exponentiation (additive API)."""
        if len(g2s) != len(g1s):
            raise ValueError("PairingProduct: length mismatch")
        out = ctypes.create_string_buffer(self.gt_bytes)
        check(load().mlhip_pairing_product(self.id, b"".join(p.raw for p in g1s), b"".join(q.raw for q in g2s), len(g1s), out))
        return Gt(out.raw, self)


def SetDevices(*devices: int) -> None:
    """the GPUs of this process (hip.SetDevices in the Go shim -> mlhip_init): with two or more listed, large
    MultiScalarMul / MultiScalarMulG2 / NewBases / PairingBatch calls are sharded over them inside the library"""
    _lib.init_devices(list(devices))


def NewCurve(name: str, **kw) -> Curve:
    ids = {"BN254": CURVE_BN254, "BLS12_381": CURVE_BLS12_381, "BLS12_377": CURVE_BLS12_377}
    return Curve(ids[name.upper().replace("-", "_")], **kw)


class Bases:
    """Resident bases (mlhip_bases_*): the additive API a prover with a fixed SRS would use.  G1 (Curve.NewBases) or G2
    (Curve.NewBasesG2)."""

    def __init__(self, curve: "Curve", points: Sequence[G1], group: int = GROUP_G1):
        self.curve = curve
        self.group = group
        self.n = len(points)
        self._h = ctypes.c_void_p()
        blob = b"".join(p.raw for p in points)
        self._lib = _concrete()  # the handle stays with the library that made it
        check(self._lib.mlhip_bases_create(curve.id, group, blob, self.n, curve.window_c, ctypes.byref(self._h)))

    def _point(self, raw: bytes):
        return G1(raw, self.curve) if self.group == GROUP_G1 else G2(raw, self.curve)

    def _point_bytes(self) -> int:
        return self.curve.g1_bytes if self.group == GROUP_G1 else self.curve.g2_bytes

    def MultiScalarMul(self, scalars: Sequence[Zr]):
        if len(scalars) > self.n:
            raise IndexError("MultiScalarMul: more scalars than resident bases")
        out = ctypes.create_string_buffer(self._point_bytes())
        c = self.curve
        check(self._lib.mlhip_bases_msm(self._h, c._scalars(scalars), 1 if c.scalars_mont else 0, len(scalars), out))
        return self._point(out.raw)

    def MultiScalarMulBatch(self, scalar_lists: Sequence[Sequence[Zr]], index_lists=None) -> List[G1]:
        """out[i] = sum_j [scalar_lists[i][j]] B[index_lists[i][j]] (without index lists: B[j], as MultiScalarMul) for many small
        MSMs over the resident bases in one device call (include/mlhip.h: mlhip_bases_msm_batch).  Each segment keeps
        MultiScalarMul's rule: at most n scalars without an index list; with one, as many indices as scalars, each below n."""
        c = self.curve
        lengths = [len(b) for b in scalar_lists]
        if index_lists is None:
            if any(m > self.n for m in lengths):
                raise IndexError("MultiScalarMulBatch: more scalars than resident bases")
        else:
            if len(index_lists) != len(scalar_lists):
                raise ValueError("MultiScalarMulBatch: %d scalar lists, %d index lists" % (len(scalar_lists), len(index_lists)))
            for b, ix in zip(scalar_lists, index_lists):
                if len(ix) != len(b):
                    raise ValueError("MultiScalarMulBatch: as many indices as scalars in every segment")
                if any(i < 0 or i >= self.n for i in ix):
                    raise IndexError("MultiScalarMulBatch: base index out of range")
        scs = b"".join(c._scalars(b) for b in scalar_lists)
        raw = _lib.bases_msm_batch(self._lib, self._h, self._point_bytes(), scs, c.scalars_mont, lengths, index_lists)
        return [self._point(r) for r in raw]

    def SumBatch(self, index_lists=None, lengths=None) -> list:
        """out[i] = sum_j B[index_lists[i][j]], or, without index lists, the sum of the first lengths[i] bases, for many sums
        over the resident bases in one device call (include/mlhip_sum_batch.h: mlhip_bases_sum_batch).  Exactly one of the
        two is given; no batch tables are built or read."""
        if (index_lists is None) == (lengths is None):
            raise ValueError("SumBatch: give index_lists or lengths")
        if index_lists is None:
            lengths = [int(m) for m in lengths]
            if any(m < 0 or m > self.n for m in lengths):
                raise IndexError("SumBatch: more points than resident bases")
        else:
            lengths = [len(ix) for ix in index_lists]
            if any(i < 0 or i >= self.n for ix in index_lists for i in ix):
                raise IndexError("SumBatch: base index out of range")
        raw = _lib.bases_sum_batch(self._lib, self._h, self._point_bytes(), lengths, index_lists)
        return [self._point(r) for r in raw]

    def BatchTabled(self) -> int:
        """the number of leading bases that have MultiScalarMulBatch tables (include/mlhip.h: mlhip_bases_batch_tabled)"""
        return _lib.bases_batch_tabled(self._lib, self._h)

    def CheckedSubgroup(self) -> bool:
        """every point of the table was verified on the device to lie in G1 (BLS12-377: Edwards bucket sums)"""
        return self._lib.mlhip_bases_checked_subgroup(self._h) == 1

    def ShiftedTables(self) -> bool:
        """the handle keeps shifted-base tables (include/mlhip.h: mlhip_bases_create): one bucket set for all digits"""
        from ._lib import plan_timings

        plan = self._lib.mlhip_bases_plan(self._h)
        return bool(plan) and plan_timings(self._lib, plan).get("tables") == 1.0

    def Close(self) -> None:
        if self._h:
            self._lib.mlhip_bases_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass


class BasesSet:
    """A set of resident tables that share one scalar vector (mlhip_bases_set_create).  The members stay usable on their own and
    must outlive the set: the set keeps references to them."""

    def __init__(self, curve: "Curve", members: Sequence[Bases]):
        self.curve = curve
        self.members = list(members)
        self._lib = _concrete()
        if any(m._lib is not self._lib for m in self.members):
            raise ValueError("NewBasesSet: a member was made by another build of the library")
        self._h = _lib.bases_set_create(self._lib, [m._h for m in self.members])
        self.n = min(m.n for m in self.members)

    def MultiScalarMul(self, scalars: Sequence[Zr]) -> list:
        """[member.MultiScalarMul(scalars) for every member], G1 or G2 as the member is"""
        if len(scalars) > self.n:
            raise IndexError("MultiScalarMul: more scalars than the smallest member's resident bases")
        c = self.curve
        raw = _lib.bases_set_msm(self._lib, self._h, [m._point_bytes() for m in self.members], c._scalars(scalars), c.scalars_mont,
                                 len(scalars))
        return [m._point(r) for m, r in zip(self.members, raw)]

    def Route(self):
        """(members, sort trains per tile, uploads of the scalars, 1 iff every member read shifted-base tables) of the last call"""
        return _lib.bases_set_route(self._lib, self._h)

    def Close(self) -> None:
        if self._h:
            self._lib.mlhip_bases_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass


class G2Prepared:
    """Fixed G2 points with their Miller-loop lines resident on the device (mlhip_g2_prepared_*, bls12-381.go:448-468)."""

    def __init__(self, curve: "Curve", points: Sequence[G2]):
        self.curve = curve
        self.m = len(points)
        self._h = ctypes.c_void_p()
        self._lib = _concrete()  # the handle stays with the library that made it
        check(self._lib.mlhip_g2_prepared_create(curve.id, b"".join(q.raw for q in points), self.m, ctypes.byref(self._h)))

    def _run(self, fused: bool, g1_lists: Sequence[Sequence[G1]], index) -> List[Gt]:
        c = self.curve
        n = len(g1_lists)
        if n == 0:
            return []
        ppp = len(g1_lists[0])
        if any(len(l) != ppp for l in g1_lists):
            raise ValueError("G2Prepared: every product takes the same number of G1 points")
        if index is None and ppp > self.m:
            raise IndexError("G2Prepared: more pairs per product than prepared points")
        if index is not None and any(i < 0 or i >= self.m for i in index):
            raise IndexError("G2Prepared: point index out of range")
        # (more than four pairs per product: include/mlhip.h, "products of any length")
        run = _lib.g2_prepared_products if ppp > 4 else _lib.g2_prepared_run
        raw = run(self._lib, self._h, c.gt_bytes, fused, b"".join(p.raw for l in g1_lists for p in l), index, ppp, n)
        return [Gt(raw[i * c.gt_bytes : (i + 1) * c.gt_bytes], c) for i in range(n)]

    def MillerLoopBatch(self, g1_lists: Sequence[Sequence[G1]], index=None) -> List[Gt]:
        """out[k] = prod_j MillerLoop(g1_lists[k][j], Q[index[j]]) (without index: Q[j]), any number of pairs per product; compare
        after FExp, as Curve.Pairing"""
        return self._run(False, g1_lists, index)

    def PairingBatch(self, g1_lists: Sequence[Sequence[G1]], index=None) -> List[Gt]:
        """out[k] = FExp(prod_j MillerLoop(g1_lists[k][j], Q[index[j]])): Pairing2 + FExp over K proofs in one launch"""
        return self._run(True, g1_lists, index)

    def Count(self) -> int:
        m = ctypes.c_size_t()
        check(self._lib.mlhip_g2_prepared_count(self._h, ctypes.byref(m)))
        return m.value

    def Close(self) -> None:
        if self._h:
            self._lib.mlhip_g2_prepared_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.Close()
        except Exception:
            pass
