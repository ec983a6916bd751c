"""Invalid wire encodings of G1 / G2 points, built with the oracle (oracle/pyref.py): the batches the codec tests
(tests/test_gpu_parity.py and the device forms in tests/test_entry_points_gpu.py) feed to mlhip_g{1,2}_from_bytes*."""


def g1_bad_encodings(R, cp, good):
    """compressed G1 encodings that SetBytes rejects, with the compressed encoding of the valid point `good` last:
    four x with x^3 + b a non-residue, a coordinate >= p, infinity with stray bits, and on the BLS12 curves a point of
    the curve outside the r-torsion subgroup"""
    n = cp.fp_bytes
    bad = []
    x = 1
    while len(bad) < 4:  # x^3 + b a non-residue
        x += 1
        if R.fp_sqrt((x**3 + cp.b) % cp.p, cp.p) is None:
            w = bytearray(x.to_bytes(n, "big"))
            w[0] |= 0x80
            bad.append(bytes(w))
    w = bytearray(cp.p.to_bytes(n, "big"))  # coordinate >= p
    w[0] |= 0x80
    bad.append(bytes(w))
    w = bytearray(R.g1_wire_compressed(cp, None))  # infinity with stray bits
    w[7] = 3
    bad.append(bytes(w))
    if cp.family == "BLS12":  # on the curve but outside the r-torsion subgroup
        x = 2
        while True:
            y = R.fp_sqrt((x**3 + cp.b) % cp.p, cp.p)
            if y is not None and R.g1_mul_unreduced(cp, (x, y), cp.r) is not None:
                break
            x += 1
        bad.append(R.g1_wire_compressed(cp, (x, y)))
    bad.append(R.g1_wire_compressed(cp, good))  # a good one in between
    return bad


def g1_off_curve_uncompressed(R, cp, p):
    """the uncompressed encoding of the point p with the last bit of y flipped: off the curve (status 2)"""
    w = bytearray(R.g1_wire_uncompressed(cp, p))
    w[-1] ^= 1
    return bytes(w)


def g2_bad_encodings(R, cp, good):
    """(compressed G2 encodings, the point outside the subgroup among them): three x with no y, a coordinate >= p,
    infinity with stray bits, a point of the twist outside the r-torsion subgroup (second to last) and the compressed
    encoding of the valid point `good` last"""
    T = R.tower(cp)
    n = cp.fp_bytes
    bad = []
    k = 1
    while len(bad) < 3:
        k += 1
        x = (k, 0) if len(bad) == 0 else (k, 1)
        if T.f2_sqrt(T.f2_add(T.f2_mul(T.f2_sqr(x), x), R.twist_b(cp))) is None:
            w = bytearray(x[1].to_bytes(n, "big") + x[0].to_bytes(n, "big"))
            w[0] |= 0x80
            bad.append(bytes(w))
    w = bytearray((1).to_bytes(n, "big") + cp.p.to_bytes(n, "big"))
    w[0] |= 0x80
    bad.append(bytes(w))
    w = bytearray(R.g2_wire_compressed(cp, None))
    w[n + 3] = 1
    bad.append(bytes(w))
    Qx = R._g2_some_point(cp, 3)
    bad.append(R.g2_wire_compressed(cp, Qx))
    bad.append(R.g2_wire_compressed(cp, good))
    return bad, Qx
