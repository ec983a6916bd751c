"""mlhip_gt_exp_cyclo / mlhip_gt_exp_cyclo_device on the GPU: Gt.Exp for members of Gt by cyclotomic squarings and a Frobenius
split of the scalar (mathlib_amd/csrc/gt_exp_cyclo.h), byte-equal to oracle/pyref.py and to mlhip_gt_exp on the same inputs --
every curve, the quad kernel (default) and the lane-pair kernel (MLHIP_PAIRING_QUAD=0), plain and Montgomery scalars, the
scalars on the digit boundaries of the split and unreduced ones, batch sizes that leave a partial last block in both kernels
(a 64-lane block holds 16 quads or 32 pairs).  Inputs: an oracle pairing, 1, and the conjugate (= inverse) of a member."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_golden
from gt_exp_cyclo_cases import boundary_scalars

pytestmark = pytest.mark.gpu

CURVES = {"BN254": 0, "BLS12-381": 1, "BLS12-377": 2}
SIZES = (0, 1, 17, 33, 67)


@pytest.fixture(scope="module")
def lib(mlhip):
    l = mlhip.load()
    assert mlhip.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return l


@functools.lru_cache(maxsize=None)
def case(name):
    """{mont: (inputs, scalars, expected)}: 67 (input, scalar) combinations -- every scalar on the member, then on 1 and on the
    conjugate in turn.  pyref computes member^e once per distinct e; 1^e = 1 and conj(m)^e = conj(m^e)."""
    from oracle import cref
    from oracle import pyref as R

    cid = CURVES[name]
    cp = R.CURVES[name]
    T = R.tower(cp)
    g1, g2 = cref.gen_points(cid, 1, 5 + cid, 0, 1), cref.gen_points(cid, 2, 11 + cid, 0, 1)
    m_bytes = cref.pairing_batch(cid, g1, g2, 1)
    m = R.gt_from_mont_bytes(cp, m_bytes)
    one = R.gt_to_mont_bytes(cp, T.f12_one)
    conj = R.gt_to_mont_bytes(cp, T.f12_conj(m))
    rng = np.random.default_rng(2024 + cid)
    boundary = boundary_scalars(cp)
    unreduced = [cp.r, cp.r + 1, 2 * cp.r + 3, (1 << 256) - 1] + [int.from_bytes(rng.bytes(32), "little") for _ in range(2)]
    rinv = pow(1 << 256, -1, cp.r)

    @functools.lru_cache(maxsize=None)
    def mpow(e):
        return T.f12_pow(m, e)

    res = {}
    for mont in (0, 1):
        # (scalar bytes, exponent): a boundary scalar keeps its exponent in both forms; an unreduced one is taken as it is
        sc = [(R.scalar_to_bytes(s % cp.r, cp, mont=True) if mont else s.to_bytes(32, "little"), s % cp.r) for s in boundary]
        sc += [(s.to_bytes(32, "little"), s * rinv % cp.r if mont else s % cp.r) for s in unreduced]
        combos = [(m_bytes, b, R.gt_to_mont_bytes(cp, mpow(e))) for b, e in sc]
        k = 0
        while len(combos) < max(SIZES):
            b, e = sc[k % len(sc)]
            if k & 1:
                combos.append((conj, b, R.gt_to_mont_bytes(cp, T.f12_conj(mpow(e)))))
            else:
                combos.append((one, b, one))
            k += 1
        combos = combos[: max(SIZES)]
        res[mont] = (b"".join(c[0] for c in combos), b"".join(c[1] for c in combos), [c[2] for c in combos])
    return res


@pytest.mark.parametrize("family", ["quad", "pairs"])
@pytest.mark.parametrize("curve", list(CURVES))
def test_gt_exp_cyclo_matches_pyref_and_gt_exp(lib, mlhip, curve, family, monkeypatch):
    import torch

    cid = CURVES[curve]
    gtb = 12 * (32 if cid == 0 else 48)
    if family == "pairs":
        monkeypatch.setenv("MLHIP_PAIRING_QUAD", "0")
    else:
        monkeypatch.delenv("MLHIP_PAIRING_QUAD", raising=False)
    st = torch.cuda.Stream()
    for mont in (0, 1):
        ins, scs, want = case(curve)[mont]
        for n in SIZES:
            out = ctypes.create_string_buffer(gtb * max(n, 1))
            ref = ctypes.create_string_buffer(gtb * max(n, 1))
            mlhip.check(lib.mlhip_gt_exp_cyclo(cid, ins[: gtb * n], scs[: 32 * n], mont, n, out))
            mlhip.check(lib.mlhip_gt_exp(cid, ins[: gtb * n], scs[: 32 * n], mont, n, ref))
            d_in = torch.frombuffer(bytearray(ins[: gtb * n] or bytes(1)), dtype=torch.uint8).cuda()
            d_sc = torch.frombuffer(bytearray(scs[: 32 * n] or bytes(1)), dtype=torch.uint8).cuda()
            d_out = torch.zeros(gtb * max(n, 1), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            mlhip.check(lib.mlhip_gt_exp_cyclo_device(cid, d_in.data_ptr(), d_sc.data_ptr(), mont, n, d_out.data_ptr(), st.cuda_stream))
            st.synchronize()
            dev = d_out.cpu().numpy().tobytes()
            if n == 0:
                assert out.raw == bytes(gtb) and dev == bytes(gtb)  # nothing written
                continue
            bad = [j for j in range(n) if out.raw[j * gtb : (j + 1) * gtb] != want[j]]
            assert not bad, (curve, family, mont, n, "host form vs pyref", bad)
            assert dev == out.raw, (curve, family, mont, n, "device form")
            assert ref.raw == out.raw, (curve, family, mont, n, "mlhip_gt_exp")


@pytest.mark.parametrize("curve", list(CURVES))
def test_non_member_input_is_not_a_fault(lib, mlhip, curve):
    """a raw Miller value is not in Gt: the result is undefined, the call is MLHIP_OK (its bytes are not compared) -- and a
    member right after it in the same batch still gets its value"""
    from oracle import cref

    cid = CURVES[curve]
    gtb = 12 * (32 if cid == 0 else 48)
    g1, g2 = cref.gen_points(cid, 1, 5 + cid, 0, 1), cref.gen_points(cid, 2, 11 + cid, 0, 1)
    raw = cref.miller_loop(cid, g1, g2, 1, 1)
    ins, scs, want = case(curve)[0]
    k = 2  # scalar r - 1 on the member
    out = ctypes.create_string_buffer(2 * gtb)
    rc = lib.mlhip_gt_exp_cyclo(cid, raw + ins[k * gtb : (k + 1) * gtb], scs[k * 32 : (k + 1) * 32] * 2, 0, 2, out)
    assert rc == 0, mlhip.load().mlhip_last_error()
    assert out.raw[gtb:] == want[k]


def test_unknown_curve_id_is_einval_and_writes_nothing(lib, mlhip):
    """curve id 7 with n = 1 through both entry points, as tests/test_entry_points_gpu.py asks of the entry points in its
    table: MLHIP_EINVAL, the error text names the curve, and zero-filled buffers larger than any Gt value stay zero"""
    import torch

    big = 4096
    hb = [ctypes.create_string_buffer(big) for _ in range(3)]
    db = [torch.zeros(big, dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    st = torch.cuda.Stream().cuda_stream
    calls = (
        lambda: lib.mlhip_gt_exp_cyclo(7, hb[0], hb[1], 0, 1, hb[2]),
        lambda: lib.mlhip_gt_exp_cyclo_device(7, db[0].data_ptr(), db[1].data_ptr(), 0, 1, db[2].data_ptr(), st),
    )
    for call in calls:
        assert lib.mlhip_set_device(99) == mlhip.EINVAL  # changes nothing but the thread's error text
        assert b"unknown curve id" not in lib.mlhip_last_error()
        assert call() == mlhip.EINVAL and b"unknown curve id" in lib.mlhip_last_error()
    torch.cuda.synchronize()
    assert all(bytes(b.raw) == bytes(big) for b in hb) and all(not t.any().item() for t in db)


@pytest.mark.parametrize("curve", list(CURVES))
def test_python_mirror_exp_batch_gt(mlhip, curve):
    """ExpBatchGt of mathlib_amd/driver.py equals ExpBatch and the single Gt.Exp on members of Gt (GenGt, a product, 1)"""
    from mathlib_amd.driver import Curve

    c = Curve(CURVES[curve])
    co = load_golden(curve)["g2_gen_coords"]  # (the mirror has no built-in BLS12-377 G2 generator)
    g2 = c.NewG2FromCoords((int(co[0][0]), int(co[0][1])), (int(co[1][0]), int(co[1][1])))
    gen = c.FExp(c.Pairing(g2, c.GenG1()))
    prod = gen.Exp(c.NewZrFromInt(12345))
    prod.Mul(gen)
    gts = [gen, prod, gen.Exp(c.GroupOrder), prod]
    zs = [c.NewZrFromInt(-1), c.NewZrFromInt(1 << 62), c.NewZrFromInt(7), c.GroupOrder]
    fast = c.ExpBatchGt(gts, zs)
    assert [g.raw for g in fast] == [g.raw for g in c.ExpBatch(gts, zs)]
    assert fast[0].raw == gen.Exp(zs[0]).raw and fast[2].IsUnity() and fast[3].IsUnity()
    assert c.ExpBatchGt([], []) == []
    with pytest.raises(ValueError):
        c.ExpBatchGt(gts, zs[:1])


def test_cpp_mirror_exp_batch_gt():
    """ExpBatchGt of include/mlhip_driver.hpp through tests/cpp/gt_exp_cyclo_test.cpp"""
    src = os.path.join(ROOT, "tests", "cpp", "gt_exp_cyclo_test.cpp")
    hdr = os.path.join(ROOT, "include", "mlhip_driver.hpp")
    so = os.path.join(ROOT, "mathlib_amd", "libmlhip.so")
    exe = os.path.join(ROOT, "tests", "cpp", "gt_exp_cyclo_test")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr), os.path.getmtime(so)):
        subprocess.check_call(
            ["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), src, "-o", exe,
             "-L", os.path.join(ROOT, "mathlib_amd"), "-lmlhip", "-Wl,-rpath," + os.path.join(ROOT, "mathlib_amd")]
        )
    co = load_golden("BLS12-377")["g2_gen_coords"]  # the mirror has no built-in BLS12-377 G2 generator
    out = subprocess.run([exe, co[0][0], co[0][1], co[1][0], co[1][1]], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RESULT OK" in out.stdout, out.stdout + out.stderr
    for name in CURVES:
        assert "%s ExpBatchGt 5/5" % name in out.stdout
