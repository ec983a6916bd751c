"""Prepared G2 handles on the GPU (include/mlhip.h: mlhip_g2_prepared_*).  After the final exponentiation a prepared Miller
loop must give, byte for byte, what the general entry points give on the expanded pairs and what the C oracle gives; the
fused mlhip_pairing_prepared the same bytes.  Handles of 1, 2 and 5 points (one at infinity, one on the curve outside G2),
every q_index form, G1 infinities in the batch, 1 .. 4 pairs per product, sizes on both sides of the dispatcher's quad /
lane-pair switch, every kernel family forced once, device pointers on a non-default stream, four threads on one handle."""
import ctypes
import threading

import numpy as np
import pytest

from g2_prepared_cases import expand, g2_bytes, handle_points, index_forms

pytestmark = pytest.mark.gpu

CURVES = {"BN254": 0, "BLS12-381": 1, "BLS12-377": 2}


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


def _cp(cid):
    from oracle import pyref as R

    return R.CURVES_BY_ID[cid]


def sizes(cid):
    fpb = 32 if cid == 0 else 48
    return 2 * fpb, 4 * fpb, 12 * fpb


def quad_switch(cid):
    """largest batch the dispatcher gives to the quad kernels (pairing_prepared_kernels.h: g2_prepared_run)"""
    return 1 << (15 if cid == 2 else 14)


def switch_sizes(cid):
    """one size on each side of every size switch of the dispatcher"""
    sw = quad_switch(cid)
    return [sw, sw + 1]


def g1_points(cid, n, seed, inf_every=9):
    """n distinct G1 points [k0 + i k1]G, a pseudo-random ninth of them replaced by the point at infinity"""
    from oracle import cref

    g1sz = sizes(cid)[0]
    a = np.frombuffer(cref.gen_points(cid, 1, 1000003 + seed, 7919 + 2 * seed, n), dtype=np.uint8).reshape(n, g1sz).copy()
    if inf_every:
        rng = np.random.default_rng(seed)
        a[rng.integers(0, inf_every, size=n) == 0] = 0
    return a.tobytes()


class Handle:
    def __init__(self, mlhip, cid, qbytes, m):
        self.mlhip, self.lib, self.cid, self.m = mlhip, mlhip.concrete(), cid, m
        self.h = ctypes.c_void_p()
        mlhip.check(self.lib.mlhip_g2_prepared_create(cid, qbytes, m, ctypes.byref(self.h)))

    def run(self, fused, g1, index, ppp, n):
        return self.mlhip.g2_prepared_run(self.lib, self.h, sizes(self.cid)[2], fused, g1, index, ppp, n)

    def close(self):
        if self.h:
            assert self.lib.mlhip_g2_prepared_destroy(self.h) == 0
            self.h = ctypes.c_void_p()


def expand_bytes(cid, qbytes, index, ppp, n):
    g2sz = sizes(cid)[1]
    qs = [qbytes[i * g2sz : (i + 1) * g2sz] for i in range(len(qbytes) // g2sz)]
    return b"".join(expand(qs, index, ppp, n))


def general_fexp(mlhip, lib, cid, g1, g2, ppp, n):
    gtsz = sizes(cid)[2]
    raw = ctypes.create_string_buffer(n * gtsz)
    out = ctypes.create_string_buffer(n * gtsz)
    mlhip.check(lib.mlhip_miller_loop(cid, g1, g2, ppp, n, raw))
    mlhip.check(lib.mlhip_final_exp(cid, raw, n, out))
    return out.raw


def fexp(mlhip, lib, cid, raw, n):
    out = ctypes.create_string_buffer(n * sizes(cid)[2])
    mlhip.check(lib.mlhip_final_exp(cid, raw, n, out))
    return out.raw


def check_case(mlhip, lib, cid, hd, qbytes, index, ppp, n, seed, oracle_rows=None):
    """the four equalities of one (handle, index, ppp, n) case; oracle_rows: which products the C oracle recomputes (None = all)"""
    from oracle import cref

    g1sz, g2sz, gtsz = sizes(cid)
    g1 = g1_points(cid, n * ppp, seed)
    g2 = expand_bytes(cid, qbytes, index, ppp, n)
    want = general_fexp(mlhip, lib, cid, g1, g2, ppp, n)
    got = fexp(mlhip, lib, cid, hd.run(False, g1, index, ppp, n), n)
    assert got == want, ("miller", cid, ppp, n, index)
    assert hd.run(True, g1, index, ppp, n) == want, ("fused", cid, ppp, n, index)
    rows = range(n) if oracle_rows is None else oracle_rows
    s1 = b"".join(g1[k * ppp * g1sz : (k + 1) * ppp * g1sz] for k in rows)
    s2 = b"".join(g2[k * ppp * g2sz : (k + 1) * ppp * g2sz] for k in rows)
    ref = cref.final_exp(cid, cref.miller_loop(cid, s1, s2, ppp, len(rows), 8), len(rows), 8)
    for j, k in enumerate(rows):
        assert want[k * gtsz : (k + 1) * gtsz] == ref[j * gtsz : (j + 1) * gtsz], ("oracle", cid, ppp, n, k)
    if ppp == 1:
        out = ctypes.create_string_buffer(n * gtsz)
        mlhip.check(lib.mlhip_pairing_batch(cid, g1, g2, n, out))
        assert out.raw == want


@pytest.mark.parametrize("ppp", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(CURVES))
def test_parity_matrix(mlhip, lib, name, ppp):
    cid = CURVES[name]
    cp = _cp(cid)
    seed = 0
    for m in (1, 2, 5):
        qbytes = g2_bytes(cp, handle_points(cp, m, "gpu"))
        hd = Handle(mlhip, cid, qbytes, m)
        try:
            for fi, index in enumerate(index_forms(m, ppp)):
                for n in (1, 3, 64, 65):
                    seed += 1
                    check_case(mlhip, lib, cid, hd, qbytes, index, ppp, n, seed)
                # 1000 and one size on each side of every dispatch switch: the general entry points check every product,
                # the oracle recomputes a strided sample (all 1000 once per curve and ppp)
                for n in [1000] + switch_sizes(cid):
                    seed += 1
                    rows = None if (n == 1000 and m == 5 and fi == 0) else sorted(set(list(range(0, n, max(1, n // 12))) + [n - 1]))
                    check_case(mlhip, lib, cid, hd, qbytes, index, ppp, n, seed, oracle_rows=rows)
        finally:
            hd.close()


@pytest.mark.parametrize("name", list(CURVES))
def test_pairing_goldens_through_a_one_point_handle(mlhip, lib, name):
    from conftest import load_golden

    cid = CURVES[name]
    for case in load_golden(name)["pairing"]:
        hd = Handle(mlhip, cid, bytes.fromhex(case["g2"]), 1)
        try:
            assert hd.run(True, bytes.fromhex(case["g1"]), None, 1, 1).hex() == case["fexp"]
            assert fexp(mlhip, lib, cid, hd.run(False, bytes.fromhex(case["g1"]), None, 1, 1), 1).hex() == case["fexp"]
        finally:
            hd.close()


@pytest.mark.parametrize("name", list(CURVES))
def test_bilinearity_without_the_general_path(mlhip, lib, name):
    """e([a]P, Q) = e(P, Q)^a through mlhip_gt_exp, and e(P, Q) e(-P, Q) = 1: nothing here runs the general Miller loop"""
    from oracle import cref
    from oracle import pyref as R

    cid = CURVES[name]
    cp = _cp(cid)
    g1sz, _, gtsz = sizes(cid)
    d = R.Drbg("g2prep/bilinear/" + name)
    Q = R.random_g2(cp, d)
    P = R.random_g1(cp, d)
    a = d.below(cp.r)
    pb = R.g1_to_mont_bytes(cp, P)
    apb = cref.point_mul(cid, 1, pb, a, False)
    neg = R.g1_to_mont_bytes(cp, (P[0], (cp.p - P[1]) % cp.p))
    hd = Handle(mlhip, cid, R.g2_to_mont_bytes(cp, Q), 1)
    try:
        e = hd.run(True, pb + apb, None, 1, 2)
        powered = ctypes.create_string_buffer(gtsz)
        mlhip.check(lib.mlhip_gt_exp(cid, e[:gtsz], a.to_bytes(32, "little"), 0, 1, powered))
        assert powered.raw == e[gtsz:]
        one = R.gt_to_mont_bytes(cp, R.tower(cp).f12_one)
        assert e[:gtsz] != one
        assert hd.run(True, pb + neg, [0, 0], 2, 1) == one
    finally:
        hd.close()


FAMILIES = {
    "one_lane": ("MLHIP_PAIRING_ONE_LANE", "1"),
    "quad": ("MLHIP_PAIRING_QUAD", "1"),
    "pairs": ("MLHIP_PAIRING_QUAD", "0"),
    "general": ("MLHIP_G2_PREPARED_GENERAL", "1"),
}


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("name", list(CURVES))
def test_every_kernel_family_forced(mlhip, lib, monkeypatch, name, family):
    """each family the dispatcher has, at a size where it is not the default (the default on both sides of its switch:
    test_parity_matrix); the switch is set first, the handle created after it"""
    cid = CURVES[name]
    cp = _cp(cid)
    for sw in ("MLHIP_PAIRING_ONE_LANE", "MLHIP_PAIRING_QUAD", "MLHIP_G2_PREPARED_GENERAL", "MLHIP_PAIRING_SAT"):
        monkeypatch.delenv(sw, raising=False)
    var, val = FAMILIES[family]
    monkeypatch.setenv(var, val)
    m = 5
    qbytes = g2_bytes(cp, handle_points(cp, m, "family"))
    hd = Handle(mlhip, cid, qbytes, m)
    try:
        n_big = quad_switch(cid) + 70 if family == "quad" else 130
        for ppp, n in ((1, 67), (2, n_big), (4, 5)):
            index = index_forms(m, ppp)[1]
            rows = None if n <= 200 else list(range(0, n, n // 10))
            check_case(mlhip, mlhip.load(), cid, hd, qbytes, index, ppp, n, 40 + ppp, oracle_rows=rows)
    finally:
        hd.close()


@pytest.mark.parametrize("name", list(CURVES))
def test_device_pointer_forms_on_a_side_stream(mlhip, lib, name):
    import torch

    cid = CURVES[name]
    cp = _cp(cid)
    g1sz, g2sz, gtsz = sizes(cid)
    m, ppp, n = 5, 2, 300
    qbytes = g2_bytes(cp, handle_points(cp, m, "device"))
    index = [4, 2]
    g1 = g1_points(cid, n * ppp, 77)
    want = general_fexp(mlhip, lib, cid, g1, expand_bytes(cid, qbytes, index, ppp, n), ppp, n)
    dq = torch.frombuffer(bytearray(qbytes), dtype=torch.uint8).cuda()
    h = ctypes.c_void_p()
    mlhip.check(lib.mlhip_g2_prepared_create_device(cid, dq.data_ptr(), m, ctypes.byref(h)))
    try:
        dq.fill_(0xA5)  # a copy was taken: the caller's buffer is its own again
        torch.cuda.synchronize()
        cnt = ctypes.c_size_t()
        mlhip.check(lib.mlhip_g2_prepared_count(h, ctypes.byref(cnt)))
        assert cnt.value == m
        d1 = torch.frombuffer(bytearray(g1), dtype=torch.uint8).cuda()
        raw = torch.empty(n * gtsz, dtype=torch.uint8, device="cuda")
        out = torch.empty(n * gtsz, dtype=torch.uint8, device="cuda")
        fused = torch.empty(n * gtsz, dtype=torch.uint8, device="cuda")
        idx = (ctypes.c_uint32 * ppp)(*index)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            st = side.cuda_stream
            mlhip.check(lib.mlhip_miller_loop_prepared_device(h, d1.data_ptr(), idx, ppp, n, raw.data_ptr(), st))
            mlhip.check(lib.mlhip_final_exp_device(cid, raw.data_ptr(), n, out.data_ptr(), st))
            mlhip.check(lib.mlhip_pairing_prepared_device(h, d1.data_ptr(), idx, ppp, n, fused.data_ptr(), st))
        side.synchronize()
        assert out.cpu().numpy().tobytes() == want
        assert fused.cpu().numpy().tobytes() == want
    finally:
        assert lib.mlhip_g2_prepared_destroy(h) == 0


def test_handle_behaviour(mlhip, lib):
    """four threads on one handle; the handle outlives mlhip_release_cache; n_products = 0 does nothing; every argument error
    that depends on the handle is MLHIP_EINVAL (checked before any launch: the output stays untouched)"""
    cid = CURVES["BLS12-381"]
    cp = _cp(cid)
    g1sz, g2sz, gtsz = sizes(cid)
    m, ppp, n = 2, 2, 200
    from oracle import pyref as R

    d = R.Drbg("g2prep/threads")
    qbytes = g2_bytes(cp, [R.random_g2(cp, d), R.random_g2(cp, d)])
    hd = Handle(mlhip, cid, qbytes, m)
    try:
        g1 = g1_points(cid, n * ppp, 5)
        want = general_fexp(mlhip, lib, cid, g1, expand_bytes(cid, qbytes, None, ppp, n), ppp, n)
        results, errors = [None] * 4, []

        def work(t):
            try:
                for _ in range(3):
                    results[t] = hd.run(True, g1, None if t % 2 == 0 else [0, 1], ppp, n)
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        ths = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        assert not errors, errors
        assert all(r == want for r in results)
        mlhip.check(lib.mlhip_release_cache())
        assert hd.run(True, g1, None, ppp, n) == want
        assert hd.run(True, b"", None, ppp, 0) == b"" and hd.run(False, b"", None, ppp, 0) == b""

        out = ctypes.create_string_buffer(b"\x5a" * gtsz, gtsz)
        L, h = hd.lib, hd.h
        u32 = lambda *v: (ctypes.c_uint32 * len(v))(*v)  # noqa: E731
        for fn in (L.mlhip_miller_loop_prepared, L.mlhip_pairing_prepared):
            assert fn(h, g1, None, 0, 1, out) == mlhip.EINVAL
            assert fn(h, g1, None, 5, 1, out) == mlhip.EINVAL
            assert fn(h, g1, None, 3, 1, out) == mlhip.EINVAL  # ppp > m without q_index
            assert fn(h, g1, u32(0, 2), 2, 1, out) == mlhip.EINVAL  # index >= m
            assert fn(h, g1, u32(0, 1), 2, 1, None) == mlhip.EINVAL
            assert fn(h, None, u32(0, 1), 2, 1, out) == mlhip.EINVAL
            assert L.mlhip_last_error()
            assert fn(h, g1, u32(1, 1, 0), 3, 1, out) == 0  # a repeated index may exceed m pairs
            out.raw = b"\x5a" * gtsz
        for fn in (L.mlhip_miller_loop_prepared_device, L.mlhip_pairing_prepared_device):
            assert fn(h, None, None, 0, 1, None, None) == mlhip.EINVAL
            assert fn(h, None, None, 3, 1, None, None) == mlhip.EINVAL
            assert fn(h, None, u32(2), 1, 1, None, None) == mlhip.EINVAL
            assert fn(h, None, None, 1, 1, None, None) == mlhip.EINVAL  # null device pointers
            assert fn(h, None, None, 1, 0, None, None) == 0
        assert out.raw == b"\x5a" * gtsz
    finally:
        hd.close()


def test_driver_g2_prepared(mlhip, lib):
    """mathlib_amd.driver: Curve.NewG2Prepared -> G2Prepared.PairingBatch is FExp(Pairing2) per proof"""
    from mathlib_amd.driver import Curve

    c = Curve(mlhip.CURVE_BLS12_381)
    g, pk = c.GenG2(), c.GenG2().Mul(c.NewZrFromInt(1234567))
    prep = c.NewG2Prepared([g, pk])
    assert prep.Count() == 2
    proofs = [[c.GenG1().Mul(c.NewZrFromInt(3 + k)), c.GenG1().Mul(c.NewZrFromInt(1000 + 7 * k))] for k in range(5)]
    fused = prep.PairingBatch(proofs)
    raw = prep.MillerLoopBatch(proofs)
    for k, (a, b) in enumerate(proofs):
        want = c.FExp(c.Pairing2(g, pk, a, b))
        assert fused[k].Equals(want) and c.FExp(raw[k]).Equals(want)
    swapped = prep.PairingBatch(proofs, index=[1, 0])
    assert swapped[0].Equals(c.FExp(c.Pairing2(pk, g, proofs[0][0], proofs[0][1])))
    with pytest.raises(IndexError):
        prep.PairingBatch(proofs, index=[0, 2])
    prep.Close()
    prep.Close()


def test_prepared_pairing2_65536(mlhip):
    """65 536 products of two pairs on BLS12-381 against a handle (g, pk), P_k = [a_k]G1, S_k = [b_k]G1:
    out_k = e(G1, G2)^(a_k + x b_k) with pk = [x]G2.
    (1) EVERY output is covered by one identity: prod_k out_k^(w_k) == GenGt^(sum_k w_k (a_k + x b_k) mod r) with random
        63-bit weights (a wrong, missing or permuted element changes the left side), and the unweighted product likewise;
    (2) a strided sample of 33 outputs byte for byte against the C oracle;
    (3) FExp of the unfused Miller values gives the same bytes as the fused launch."""
    import torch

    from mathlib_amd.driver import Curve
    from oracle import cref
    from oracle import pyref as R

    lib, cid = mlhip.load(), mlhip.CURVE_BLS12_381
    n, ppp = 1 << 16, 2
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    k = torch.randint(-(1 << 63), (1 << 63) - 1, (n * ppp, 4), dtype=torch.int64, generator=gen, device=dev).view(torch.uint8).reshape(-1, 32)
    base = torch.frombuffer(bytearray(Curve(cid).GenG1().raw), dtype=torch.uint8).to(dev)
    pts = torch.empty(n * ppp * 96, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    mlhip.check(lib.mlhip_scalar_mul_device(cid, 1, base.data_ptr(), 0, k.data_ptr(), 0, n * ppp, pts.data_ptr(), st))
    cp = R.BLS12_381
    x = 0x1D3A5B7C9E1F2468ACE13579BDF02468
    g2 = R.g2_to_mont_bytes(cp, R.g2_generator(cp))
    qbytes = g2 + cref.point_mul(cid, 2, g2, x, False)
    h = ctypes.c_void_p()
    mlhip.check(lib.mlhip_g2_prepared_create(cid, qbytes, 2, ctypes.byref(h)))
    try:
        out = torch.empty(n * 576, dtype=torch.uint8, device=dev)
        raw = torch.empty(n * 576, dtype=torch.uint8, device=dev)
        mlhip.check(lib.mlhip_pairing_prepared_device(h, pts.data_ptr(), None, ppp, n, out.data_ptr(), st))
        mlhip.check(lib.mlhip_miller_loop_prepared_device(h, pts.data_ptr(), None, ppp, n, raw.data_ptr(), st))
        mlhip.check(lib.mlhip_final_exp_device(cid, raw.data_ptr(), n, raw.data_ptr(), st))
        torch.cuda.synchronize()
        assert torch.equal(out, raw)  # (3)
    finally:
        assert lib.mlhip_g2_prepared_destroy(h) == 0
    o = out.cpu().numpy()
    hp = pts.cpu().numpy()

    T = R.tower(cp)
    gen_gt = R.pairing(cp, cp.g1, R.g2_generator(cp))
    to_int = lambda row: int(row[0]) | int(row[1]) << 64 | int(row[2]) << 128 | int(row[3]) << 192  # noqa: E731
    kk = k.cpu().numpy().view(np.uint64).reshape(n * ppp, 4)
    es = [(to_int(kk[2 * i]) + x * to_int(kk[2 * i + 1])) % cp.r for i in range(n)]
    w = np.zeros((n, 4), dtype=np.uint64)
    w[:, 0] = np.random.default_rng(4242).integers(1, 1 << 63, size=n, dtype=np.uint64)

    def tree_product(buf):
        m = n
        while m > 1:
            half = m // 2
            mlhip.check(lib.mlhip_gt_mul_device(cid, buf.data_ptr(), buf.data_ptr() + (m - half) * 576, half, buf.data_ptr(), st))
            m -= half
        torch.cuda.synchronize()
        return bytes(buf[:576].cpu().numpy().tobytes())

    assert tree_product(out.clone()) == R.gt_to_mont_bytes(cp, T.f12_pow(gen_gt, sum(es) % cp.r))
    dw = torch.from_numpy(w.view(np.uint8).reshape(-1).copy()).cuda()
    powered = torch.empty_like(out)
    mlhip.check(lib.mlhip_gt_exp_device(cid, out.data_ptr(), dw.data_ptr(), 0, n, powered.data_ptr(), st))
    weighted = sum(int(w[i, 0]) * es[i] for i in range(n)) % cp.r
    assert tree_product(powered) == R.gt_to_mont_bytes(cp, T.f12_pow(gen_gt, weighted))

    idx = list(range(0, n, n // 32)) + [n - 1]
    g1s = b"".join(hp[i * 192 : (i + 1) * 192].tobytes() for i in idx)
    ref = cref.final_exp(cid, cref.miller_loop(cid, g1s, qbytes * len(idx), ppp, len(idx), 8), len(idx), 8)
    for j, i in enumerate(idx):
        assert o[i * 576 : (i + 1) * 576].tobytes() == ref[j * 576 : (j + 1) * 576], i
