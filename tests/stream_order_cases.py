"""The busy-stream scenario and its table (tests/test_stream_order_gpu.py runs it, tests/test_stream_order_table.py checks the
table against include/mlhip.h): every entry point that takes a `void* stream`, called while its inputs are still being
produced on that stream and while its inputs and outputs are overwritten right behind it.

A Case is one entry point at one shape: real inputs, DECOY inputs of the same shape (valid inputs from another seed: a stale
read gives a wrong answer, never an invalid address), the host arrays the call reads, the call itself, its host form and the
CPU oracle (oracle/cref.py, oracle/pyref.py).  run_scenario drives one Case on one stream behind the delay -- the library's own
k_fp_mul with a calibrated `repeat` (mlhip_fp_mul_device)."""
import ctypes
import functools
import time
from collections import namedtuple

import numpy as np

CURVES = {"BN254": 0, "BLS12-381": 1, "BLS12-377": 2}
NAMES = {v: k for k, v in CURVES.items()}
FPB = {0: 32, 1: 48, 2: 48}


def _cref():
    from oracle import cref

    return cref


def _pyref(cid):
    from oracle import pyref as R

    return R, R.CURVES[NAMES[cid]]


def _scalars(seed, n):
    """n scalars of any 256-bit value (scalars_mont = 0: reduced mod r on the device), as bytes"""
    return np.random.default_rng(seed).integers(0, 1 << 64, size=(n, 4), dtype=np.uint64, endpoint=False).tobytes()


def _ints(sc):
    return [int.from_bytes(sc[i : i + 32], "little") for i in range(0, len(sc), 32)]


def _chunks(raw, size):
    return [raw[i : i + size] for i in range(0, len(raw), size)]


def _pts(cid, group, seed, n):
    return _cref().gen_points(cid, group, 1000 + 17 * seed, 3 + 2 * seed, n)


@functools.lru_cache(maxsize=None)
def _members(cid, seed, n):
    """n members of Gt with the G1 / G2 points they are the pairings of"""
    g1, g2 = _pts(cid, 1, seed, n), _pts(cid, 2, seed + 1, n)
    return _cref().pairing_batch(cid, g1, g2, n, 8), g1, g2


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """real / decoy: the device inputs (lists of bytes); out_bytes: the sizes of the device outputs ([] = the result comes back
    in host memory, from call() or finish()); host_real / host_other: the host arrays {name: (ctype, values)} the call gets and
    what they are overwritten with as soon as it returns"""

    env = {}
    host_real = {}
    host_other = {}

    def open(self, lib, mlhip):
        pass

    def close(self, lib):
        pass

    def call(self, lib, mlhip, ins, outs, host, stream):
        """the entry point on device pointers ins / outs; returns the host-memory results ([] when there are none yet)"""
        raise NotImplementedError

    def finish(self, lib, mlhip):
        """what is left to do after the call (mlhip_msm_finish): host-memory results"""
        return []

    def host_form(self, lib, mlhip, ins, host):
        """the host-buffer entry point on the same inputs, or None when there is none"""
        return None

    def oracle(self, ins, host):
        raise NotImplementedError

    def canon(self, lib, mlhip, outs):
        """what is compared with the oracle (raw Miller values: after mlhip_final_exp)"""
        return outs

    def host_arrays(self, values):
        return {k: (t * max(1, len(v)))(*v) for k, (t, v) in values.items()}


class Miller(Case):
    def __init__(self, cid, what, ppp=1, n=37):
        self.cid, self.what, self.ppp, self.n = cid, what, ppp, n
        self.gtb = 12 * FPB[cid]
        k = n * ppp
        self.real = [_pts(cid, 1, 1, k), _pts(cid, 2, 2, k)]
        self.decoy = [_pts(cid, 1, 3, k), _pts(cid, 2, 4, k)]
        if what == "final_exp":
            self.real = [_cref().miller_loop(cid, self.real[0], self.real[1], 1, n, 8)]
            self.decoy = [_cref().miller_loop(cid, self.decoy[0], self.decoy[1], 1, n, 8)]
        self.out_bytes = [self.gtb * n]

    def call(self, lib, mlhip, ins, outs, host, stream):
        if self.what == "miller":
            mlhip.check(lib.mlhip_miller_loop_device(self.cid, ins[0], ins[1], self.ppp, self.n, outs[0], stream))
        elif self.what == "final_exp":
            mlhip.check(lib.mlhip_final_exp_device(self.cid, ins[0], self.n, outs[0], stream))
        else:
            mlhip.check(lib.mlhip_pairing_batch_device(self.cid, ins[0], ins[1], self.n, outs[0], stream))
        return []

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.gtb * self.n)
        if self.what == "miller":
            mlhip.check(lib.mlhip_miller_loop(self.cid, ins[0], ins[1], self.ppp, self.n, out))
        elif self.what == "final_exp":
            mlhip.check(lib.mlhip_final_exp(self.cid, ins[0], self.n, out))
        else:
            mlhip.check(lib.mlhip_pairing_batch(self.cid, ins[0], ins[1], self.n, out))
        return [out.raw]

    def oracle(self, ins, host):
        cref = _cref()
        if self.what == "miller":
            return [cref.final_exp(self.cid, cref.miller_loop(self.cid, ins[0], ins[1], self.ppp, self.n, 8), self.n, 8)]
        if self.what == "final_exp":
            return [cref.final_exp(self.cid, ins[0], self.n, 8)]
        return [cref.pairing_batch(self.cid, ins[0], ins[1], self.n, 8)]

    def canon(self, lib, mlhip, outs):
        if self.what != "miller":
            return outs
        out = ctypes.create_string_buffer(self.gtb * self.n)
        mlhip.check(lib.mlhip_final_exp(self.cid, outs[0], self.n, out))
        return [out.raw]


class GtOp(Case):
    """mul, inverse, exp, exp_cyclo, to_bytes on members of Gt (pairings of generated points)"""

    def __init__(self, cid, what, n=70):
        self.cid, self.what, self.n = cid, what, n
        self.gtb = 12 * FPB[cid]
        a, self.a1, self.a2 = _members(cid, 10, n)
        d, self.d1, self.d2 = _members(cid, 20, n)
        self.real, self.decoy = [a], [d]
        if what == "mul":
            self.real.append(_members(cid, 30, n)[0])
            self.decoy.append(_members(cid, 40, n)[0])
        elif what in ("exp", "exp_cyclo"):
            self.real.append(_scalars(50 + cid, n))
            self.decoy.append(_scalars(60 + cid, n))
        self.out_bytes = [self.gtb * n]

    def _run(self, lib, mlhip, suffix, ins, out, *tail):
        c, n = self.cid, self.n
        fn = lambda name: getattr(lib, name + suffix)
        if self.what == "mul":
            mlhip.check(fn("mlhip_gt_mul")(c, ins[0], ins[1], n, out, *tail))
        elif self.what == "inverse":
            mlhip.check(fn("mlhip_gt_inverse")(c, ins[0], n, out, *tail))
        elif self.what == "exp":
            mlhip.check(fn("mlhip_gt_exp")(c, ins[0], ins[1], 0, n, out, *tail))
        elif self.what == "exp_cyclo":
            mlhip.check(fn("mlhip_gt_exp_cyclo")(c, ins[0], ins[1], 0, n, out, *tail))
        else:
            mlhip.check(fn("mlhip_gt_to_bytes")(c, ins[0], n, out, *tail))

    def call(self, lib, mlhip, ins, outs, host, stream):
        self._run(lib, mlhip, "_device", ins, outs[0], stream)
        return []

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.gtb * self.n)
        self._run(lib, mlhip, "", ins, out)
        return [out.raw]

    def oracle(self, ins, host):
        cref = _cref()
        R, cp = _pyref(self.cid)
        T = R.tower(cp)
        if self.what == "mul":
            return [cref.gt_mul(self.cid, ins[0], ins[1], self.n)]
        vals = [R.gt_from_mont_bytes(cp, b) for b in _chunks(ins[0], self.gtb)]
        if self.what == "inverse":
            return [b"".join(R.gt_to_mont_bytes(cp, T.f12_inv(f)) for f in vals)]
        if self.what == "to_bytes":
            return [b"".join(R.gt_wire_bytes(cp, f) for f in vals)]
        # e(P, Q)^s = e([s] P, Q): the C oracle's scalar multiplication and pairing
        g1, g2 = (self.a1, self.a2) if ins[0] == self.real[0] else (self.d1, self.d2)
        assert ins[0] in (self.real[0], self.decoy[0])
        psz = 2 * FPB[self.cid]
        sp = b"".join(cref.point_mul(self.cid, 1, p, s) for p, s in zip(_chunks(g1, psz), _ints(ins[1])))
        return [cref.pairing_batch(self.cid, sp, g2, self.n, 8)]


@functools.lru_cache(maxsize=None)
def _gt_pool(cid):
    """three members of Gt and three raw Miller values (outside Gt), each checked by the definition f^r = 1: (bytes, member)"""
    R, cp = _pyref(cid)
    T = R.tower(cp)
    mem, g1, g2 = _members(cid, 70, 3)
    raw = _cref().miller_loop(cid, g1, g2, 1, 3, 1)
    gtb = 12 * FPB[cid]
    pool = [(b, True) for b in _chunks(mem, gtb)] + [(b, False) for b in _chunks(raw, gtb)]
    for b, member in pool:
        assert T.f12_is_one(T.f12_pow(R.gt_from_mont_bytes(cp, b), cp.r)) == member
    return pool


class GtCheck(Case):
    """mlhip_gt_is_member_device / mlhip_gt_from_bytes_device (check on) over members and raw Miller values in a seeded order"""

    def __init__(self, cid, what, n=70):
        self.cid, self.what, self.n = cid, what, n
        self.gtb = 12 * FPB[cid]
        pool = _gt_pool(cid)
        R, cp = _pyref(cid)
        self.values = {b: m for b, m in pool}
        self.wire = {R.gt_wire_bytes(cp, R.gt_from_mont_bytes(cp, b)): (b, m) for b, m in pool}
        src = list(self.wire) if what == "from_bytes" else list(self.values)

        def pick(seed):
            order = np.random.default_rng(seed).integers(0, len(src), size=n)
            return b"".join(src[i] for i in order)

        self.real, self.decoy = [pick(80 + cid)], [pick(90 + cid)]
        self.out_bytes = [self.gtb * n, n] if what == "from_bytes" else [n]

    def call(self, lib, mlhip, ins, outs, host, stream):
        if self.what == "from_bytes":
            mlhip.check(lib.mlhip_gt_from_bytes_device(self.cid, ins[0], self.n, 1, outs[0], outs[1], stream))
        else:
            mlhip.check(lib.mlhip_gt_is_member_device(self.cid, ins[0], self.n, outs[0], stream))
        return []

    def host_form(self, lib, mlhip, ins, host):
        st = ctypes.create_string_buffer(self.n)
        if self.what == "from_bytes":
            out = ctypes.create_string_buffer(self.gtb * self.n)
            mlhip.check(lib.mlhip_gt_from_bytes(self.cid, ins[0], self.n, 1, out, st))
            return [out.raw, st.raw]
        mlhip.check(lib.mlhip_gt_is_member(self.cid, ins[0], self.n, st))
        return [st.raw]

    def oracle(self, ins, host):
        rows = _chunks(ins[0], self.gtb)
        if self.what == "from_bytes":
            got = [self.wire[w] for w in rows]
            return [b"".join(b if m else bytes(self.gtb) for b, m in got), bytes(0 if m else 3 for _, m in got)]
        return [bytes(0 if self.values[b] else 3 for b in rows)]


class PointCodec(Case):
    """mlhip_g{1,2}_from_bytes_device (compressed, subgroup mode 1) and mlhip_g{1,2}_to_bytes_device (compressed)"""

    def __init__(self, cid, group, decode, n=23):
        self.cid, self.group, self.decode, self.n = cid, group, decode, n
        self.psz = 2 * group * FPB[cid]
        R, cp = _pyref(cid)
        self.wire_of = R.g1_wire_compressed if group == 1 else R.g2_wire_compressed
        self.parse = R.g1_from_mont_bytes if group == 1 else R.g2_from_mont_bytes
        self.from_wire = R.g1_from_wire if group == 1 else R.g2_from_wire
        self.to_mont = R.g1_to_mont_bytes if group == 1 else R.g2_to_mont_bytes

        def points(seed):
            b = bytearray(_pts(cid, group, seed, n))
            b[5 * self.psz : 6 * self.psz] = bytes(self.psz)  # an infinity
            return bytes(b)

        self.real, self.decoy = [points(5)], [points(6)]
        if decode:
            self.real, self.decoy = [self._encode(self.real[0])], [self._encode(self.decoy[0])]
            self.out_bytes = [self.psz * n, n]
        else:
            self.out_bytes = [self.psz // 2 * n]

    def _encode(self, affine):
        _, cp = _pyref(self.cid)
        return b"".join(self.wire_of(cp, self.parse(cp, b)) for b in _chunks(affine, self.psz))

    def _fn(self, lib, suffix):
        return getattr(lib, "mlhip_g%d_%s_bytes%s" % (self.group, "from" if self.decode else "to", suffix))

    def call(self, lib, mlhip, ins, outs, host, stream):
        if self.decode:
            mlhip.check(self._fn(lib, "_device")(self.cid, ins[0], self.n, 1, 1, outs[0], outs[1], stream))
        else:
            mlhip.check(self._fn(lib, "_device")(self.cid, ins[0], self.n, 1, outs[0], stream))
        return []

    def host_form(self, lib, mlhip, ins, host):
        if self.decode:
            out, st = ctypes.create_string_buffer(self.psz * self.n), ctypes.create_string_buffer(self.n)
            mlhip.check(self._fn(lib, "")(self.cid, ins[0], self.n, 1, 1, out, st))
            return [out.raw, st.raw]
        out = ctypes.create_string_buffer(self.psz // 2 * self.n)
        mlhip.check(self._fn(lib, "")(self.cid, ins[0], self.n, 1, out))
        return [out.raw]

    def oracle(self, ins, host):
        _, cp = _pyref(self.cid)
        if not self.decode:
            return [self._encode(ins[0])]
        got = [self.from_wire(cp, w, True) for w in _chunks(ins[0], self.psz // 2)]
        return [b"".join(self.to_mont(cp, p) for p, _ in got), bytes(s for _, s in got)]


class ScalarMul(Case):
    """mlhip_scalar_mul_device: one point per scalar (stride 1) or one base for all of them (stride 0: the per-device table)"""

    def __init__(self, cid, group, stride, n, seed=0):
        self.cid, self.group, self.stride, self.n = cid, group, stride, n
        self.psz = 2 * group * FPB[cid]
        k = n if stride else 1
        self.real = [_pts(cid, group, 7 + seed, k), _scalars(100 + cid + seed, n)]
        self.decoy = [_pts(cid, group, 8 + seed, k), _scalars(110 + cid + seed, n)]
        self.out_bytes = [self.psz * n]
        if not stride:
            self.env = {"MLHIP_FIXED_BASE_MIN": "1024", "MLHIP_FB_WINDOW": "6"}

    def call(self, lib, mlhip, ins, outs, host, stream):
        mlhip.check(lib.mlhip_scalar_mul_device(self.cid, self.group, ins[0], self.stride, ins[1], 0, self.n, outs[0], stream))
        return []

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.psz * self.n)
        mlhip.check(lib.mlhip_scalar_mul(self.cid, self.group, ins[0], self.stride, ins[1], 0, self.n, out))
        return [out.raw]

    def oracle(self, ins, host):
        from concurrent.futures import ThreadPoolExecutor

        cref = _cref()
        cref.load()
        pts = _chunks(ins[0], self.psz)
        with ThreadPoolExecutor(8) as pool:  # (the C oracle runs outside the interpreter lock)
            return [b"".join(pool.map(lambda t: cref.point_mul(self.cid, self.group, pts[t[0] if self.stride else 0], t[1]),
                                      enumerate(_ints(ins[1]))))]


def _segments(seed, k, longest=9):
    """k segment lengths of 0 .. longest pairs, both ends among them"""
    lengths = [int(v) for v in np.random.default_rng(seed).integers(0, longest + 1, size=k)]
    lengths[1], lengths[k - 2] = 0, longest
    return lengths


def _offsets(lengths):
    return [0] + [int(v) for v in np.cumsum(lengths)]


def _msm_segments(cid, group, points, scalars, offsets, index=None):
    """cref.msm of every segment; index: the base of each pair (points is then the table)"""
    cref = _cref()
    psz = 2 * group * FPB[cid]
    out = []
    for a, b in zip(offsets, offsets[1:]):
        if a == b:
            out.append(bytes(psz))
            continue
        if index is None:
            p = points[a * psz : b * psz]
        else:
            p = b"".join(points[i * psz : (i + 1) * psz] for i in index[a:b])
        out.append(cref.msm(cid, group, p, scalars[32 * a : 32 * b], b - a, False, 0, 1))
    return b"".join(out)


class MsmBatch(Case):
    """mlhip_msm_batch_device: K segments of 0 .. 9 pairs; the offsets are host memory"""

    def __init__(self, cid, group, k=64, seed=0, reverse=False, inputs=None):
        """reverse: the segmentation of `seed` back to front (same K, same total); inputs: the seed of points and scalars"""
        self.cid, self.group, self.k = cid, group, k
        self.psz = 2 * group * FPB[cid]
        lengths = _segments(200 + seed, k)
        total = sum(lengths)
        other = lengths[::-1]  # another segmentation with the same total
        assert other != lengths
        if reverse:
            lengths, other = other, lengths
        seed = seed if inputs is None else inputs
        self.host_real = {"offsets": (ctypes.c_uint64, _offsets(lengths))}
        self.host_other = {"offsets": (ctypes.c_uint64, _offsets(other))}
        self.real = [_pts(cid, group, 11 + seed, total), _scalars(120 + cid + seed, total)]
        self.decoy = [_pts(cid, group, 12 + seed, total), _scalars(130 + cid + seed, total)]
        self.out_bytes = [self.psz * k]

    def call(self, lib, mlhip, ins, outs, host, stream):
        mlhip.check(lib.mlhip_msm_batch_device(self.cid, self.group, ins[0], ins[1], 0, host["offsets"], self.k, outs[0], stream))
        return []

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.psz * self.k)
        mlhip.check(lib.mlhip_msm_batch(self.cid, self.group, ins[0], ins[1], 0, host["offsets"], self.k, out))
        return [out.raw]

    def oracle(self, ins, host):
        return [_msm_segments(self.cid, self.group, ins[0], ins[1], host["offsets"][1])]


class BasesBatch(Case):
    """mlhip_bases_msm_batch_device on a 16-base handle: offsets and base_index are host memory"""

    def __init__(self, cid, group, indexed, table_free=False, k=64, nb=16):
        self.cid, self.group, self.k, self.nb, self.indexed = cid, group, k, nb, indexed
        self.psz = 2 * group * FPB[cid]
        self.bases = _pts(cid, group, 13, nb)
        lengths = _segments(210 + cid, k)
        total = sum(lengths)
        self.host_real = {"offsets": (ctypes.c_uint64, _offsets(lengths))}
        self.host_other = {"offsets": (ctypes.c_uint64, _offsets(lengths[::-1]))}
        if indexed:
            idx = [int(v) for v in np.random.default_rng(220 + cid).integers(0, nb, size=total)]
            perm = [idx[i] for i in np.random.default_rng(221).permutation(total)]
            assert perm != idx
            self.host_real["base_index"] = (ctypes.c_uint32, idx)
            self.host_other["base_index"] = (ctypes.c_uint32, perm)
        self.real, self.decoy = [_scalars(140 + cid, total)], [_scalars(150 + cid, total)]
        self.out_bytes = [self.psz * k]
        self.env = {"MLHIP_BASES_BATCH_MAX_MB": "0"} if table_free else {}
        self.h = None

    def open(self, lib, mlhip):
        self.h = ctypes.c_void_p()
        mlhip.check(lib.mlhip_bases_create(self.cid, self.group, self.bases, self.nb, 0, ctypes.byref(self.h)))

    def close(self, lib):
        if self.h:
            lib.mlhip_bases_destroy(self.h)
            self.h = None

    def call(self, lib, mlhip, ins, outs, host, stream):
        mlhip.check(lib.mlhip_bases_msm_batch_device(self.h, ins[0], 0, host.get("base_index"), host["offsets"], self.k, stream, outs[0]))
        return []

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.psz * self.k)
        mlhip.check(lib.mlhip_bases_msm_batch(self.h, ins[0], 0, host.get("base_index"), host["offsets"], self.k, out))
        return [out.raw]

    def oracle(self, ins, host):
        offsets = host["offsets"][1]
        if self.indexed:
            index = host["base_index"][1]
        else:  # pair j of a segment takes base j
            index = [i - a for a, b in zip(offsets, offsets[1:]) for i in range(a, b)]
        return [_msm_segments(self.cid, self.group, self.bases, ins[0], offsets, index)]


class BasesMsm(Case):
    """mlhip_bases_msm_device: the MSM over a resident table, result in host memory"""

    def __init__(self, cid, group=1, n=3000):
        self.cid, self.group, self.n = cid, group, n
        self.psz = 2 * group * FPB[cid]
        self.bases = _pts(cid, group, 14, n)
        self.real, self.decoy = [_scalars(160 + cid, n)], [_scalars(170 + cid, n)]
        self.out_bytes = []
        self.h = None

    open = BasesBatch.open
    close = BasesBatch.close

    @property
    def nb(self):
        return self.n

    def call(self, lib, mlhip, ins, outs, host, stream):
        out = ctypes.create_string_buffer(self.psz)
        mlhip.check(lib.mlhip_bases_msm_device(self.h, ins[0], 0, self.n, stream, out))
        return [out.raw]

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.psz)
        mlhip.check(lib.mlhip_bases_msm(self.h, ins[0], 0, self.n, out))
        return [out.raw]

    def oracle(self, ins, host):
        return [_cref().msm(self.cid, self.group, self.bases, ins[0], self.n, False, 0, 8)]


class Prepared(Case):
    """mlhip_miller_loop_prepared_device / mlhip_pairing_prepared_device: m = 3 prepared points, two pairs per product, q_index
    in host memory"""

    def __init__(self, cid, fused, general=False, n=37, m=3, ppp=2):
        self.cid, self.fused, self.n, self.m, self.ppp = cid, fused, n, m, ppp
        self.gtb = 12 * FPB[cid]
        self.qs = _pts(cid, 2, 15, m)
        self.host_real = {"q_index": (ctypes.c_uint32, [2, 0])}
        self.host_other = {"q_index": (ctypes.c_uint32, [0, 2])}
        self.real, self.decoy = [_pts(cid, 1, 16, n * ppp)], [_pts(cid, 1, 17, n * ppp)]
        self.out_bytes = [self.gtb * n]
        self.env = {"MLHIP_G2_PREPARED_GENERAL": "1"} if general else {}
        self.h = None

    def open(self, lib, mlhip):
        self.h = ctypes.c_void_p()
        mlhip.check(lib.mlhip_g2_prepared_create(self.cid, self.qs, self.m, ctypes.byref(self.h)))

    def close(self, lib):
        if self.h:
            lib.mlhip_g2_prepared_destroy(self.h)
            self.h = None

    def call(self, lib, mlhip, ins, outs, host, stream):
        fn = lib.mlhip_pairing_prepared_device if self.fused else lib.mlhip_miller_loop_prepared_device
        mlhip.check(fn(self.h, ins[0], host["q_index"], self.ppp, self.n, outs[0], stream))
        return []

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.gtb * self.n)
        fn = lib.mlhip_pairing_prepared if self.fused else lib.mlhip_miller_loop_prepared
        mlhip.check(fn(self.h, ins[0], host["q_index"], self.ppp, self.n, out))
        return [out.raw]

    def oracle(self, ins, host):
        cref = _cref()
        q = _chunks(self.qs, 4 * FPB[self.cid])
        g2 = b"".join(q[j] for j in host["q_index"][1]) * self.n
        return [cref.final_exp(self.cid, cref.miller_loop(self.cid, ins[0], g2, self.ppp, self.n, 8), self.n, 8)]

    def canon(self, lib, mlhip, outs):
        if self.fused:
            return outs
        out = ctypes.create_string_buffer(self.gtb * self.n)
        mlhip.check(lib.mlhip_final_exp(self.cid, outs[0], self.n, out))
        return [out.raw]


class Msm(Case):
    """mlhip_msm_run, or mlhip_msm_launch + mlhip_msm_finish, on one plan: n = 5000, c = 13, in tiles of 2^10 pairs (five tiles,
    the sort of tile s + 1 ahead on the plan's sort stream) or in one pass"""

    def __init__(self, cid, group, how, tile, n=5000, c=13, seed=0):
        self.cid, self.group, self.how, self.n, self.c = cid, group, how, n, c
        self.psz = 2 * group * FPB[cid]
        self.real = [_pts(cid, group, 18 + seed, n), _scalars(180 + cid + seed, n)]
        self.decoy = [_pts(cid, group, 19 + seed, n), _scalars(190 + cid + seed, n)]
        self.out_bytes = []
        self.env = {"MLHIP_TILE_LOG2": str(tile)}
        self.h = None

    def open(self, lib, mlhip):
        self.h = ctypes.c_void_p()
        mlhip.check(lib.mlhip_msm_plan_create(self.cid, self.group, self.n, self.c, ctypes.byref(self.h)))

    def close(self, lib):
        if self.h:
            lib.mlhip_msm_plan_destroy(self.h)
            self.h = None

    def call(self, lib, mlhip, ins, outs, host, stream):
        if self.how == "run":
            out = ctypes.create_string_buffer(self.psz)
            mlhip.check(lib.mlhip_msm_run(self.h, ins[0], ins[1], 0, self.n, stream, out, None))
            return [out.raw]
        mlhip.check(lib.mlhip_msm_launch(self.h, ins[0], ins[1], 0, self.n, stream))
        return []

    def finish(self, lib, mlhip):
        if self.how == "run":
            return []
        out = ctypes.create_string_buffer(self.psz)
        mlhip.check(lib.mlhip_msm_finish(self.h, out, None))
        return [out.raw]

    def host_form(self, lib, mlhip, ins, host):
        out = ctypes.create_string_buffer(self.psz)
        fn = lib.mlhip_msm_g1 if self.group == 1 else lib.mlhip_msm_g2
        mlhip.check(fn(self.cid, ins[0], ins[1], 0, self.n, self.c, out))
        return [out.raw]

    def oracle(self, ins, host):
        return [_cref().msm(self.cid, self.group, ins[0], ins[1], self.n, False, 0, 8)]


class MsmShared(Case):
    """mlhip_msm_launch_shared: the G1 and the G2 MSM of one scalar vector on two plans of one width, tile by tile"""

    def __init__(self, cid, tile=10, n=5000, c=13):
        self.cid, self.n, self.c = cid, n, c
        self.real = [_pts(cid, 1, 21, n), _pts(cid, 2, 22, n), _scalars(240 + cid, n)]
        self.decoy = [_pts(cid, 1, 23, n), _pts(cid, 2, 24, n), _scalars(250 + cid, n)]
        self.out_bytes = []
        self.env = {"MLHIP_TILE_LOG2": str(tile)}
        self.h = []

    def open(self, lib, mlhip):
        for group in (1, 2):
            h = ctypes.c_void_p()
            mlhip.check(lib.mlhip_msm_plan_create(self.cid, group, self.n, self.c, ctypes.byref(h)))
            self.h.append(h)

    def close(self, lib):
        for h in self.h:
            lib.mlhip_msm_plan_destroy(h)
        self.h = []

    def call(self, lib, mlhip, ins, outs, host, stream):
        mlhip.check(lib.mlhip_msm_launch_shared(self.h[0], self.h[1], ins[0], ins[1], ins[2], 0, self.n, stream))
        return []

    def finish(self, lib, mlhip):
        res = []
        for group, h in zip((1, 2), self.h):
            out = ctypes.create_string_buffer(2 * group * FPB[self.cid])
            mlhip.check(lib.mlhip_msm_finish(h, out, None))
            res.append(out.raw)
        return res

    def host_form(self, lib, mlhip, ins, host):
        o1, o2 = ctypes.create_string_buffer(2 * FPB[self.cid]), ctypes.create_string_buffer(4 * FPB[self.cid])
        mlhip.check(lib.mlhip_msm_g1g2(self.cid, ins[0], ins[1], ins[2], 0, self.n, self.c, o1, o2))
        return [o1.raw, o2.raw]

    def oracle(self, ins, host):
        return [_cref().msm(self.cid, g, ins[g - 1], ins[2], self.n, False, 0, 8) for g in (1, 2)]


def _fp_values(cid, seed, n):
    """n field elements below 2^(bits - 1) < p: any such value is a valid Montgomery form"""
    a = np.random.default_rng(seed).integers(0, 256, size=(n, FPB[cid]), dtype=np.uint8)
    a[:, -1] &= 0x0F  # p has 254 (BN254), 381 and 377 bits: the top byte stays below p's
    return a.tobytes()


def fp_mul_expected(cid, a, b, repeat):
    """lane values of k_fp_mul in Python integers: a, then `repeat` Montgomery products by b"""
    _, cp = _pyref(cid)
    rinv = pow(1 << (8 * FPB[cid]), -1, cp.p)
    x, y = int.from_bytes(a, "little"), int.from_bytes(b, "little")
    return (x * pow(y * rinv, repeat, cp.p) % cp.p).to_bytes(FPB[cid], "little")


class FpMul(Case):
    """mlhip_fp_mul_device itself (the delay is made of it): three dependent products per lane"""

    def __init__(self, cid, n=1000, repeat=3):
        self.cid, self.n, self.repeat = cid, n, repeat
        self.real = [_fp_values(cid, 300, n), _fp_values(cid, 301, n)]
        self.decoy = [_fp_values(cid, 302, n), _fp_values(cid, 303, n)]
        self.out_bytes = [FPB[cid] * n]

    def call(self, lib, mlhip, ins, outs, host, stream):
        mlhip.check(lib.mlhip_fp_mul_device(self.cid, ins[0], ins[1], self.n, self.repeat, outs[0], stream))
        return []

    def oracle(self, ins, host):
        f = FPB[self.cid]
        return [b"".join(fp_mul_expected(self.cid, a, b, self.repeat) for a, b in zip(_chunks(ins[0], f), _chunks(ins[1], f)))]


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
# sync: None = asynchronous (the call returns while the stream is still busy: asserted); otherwise the words of include/mlhip.h
# that make the entry point synchronous by contract.  promise: words of the header sentence that promises the ordering.
Row = namedtuple("Row", "id entry make promise sync host_args")

IN_ORDER = "enqueue their kernels on `stream` and return"
SCALAR_MUL = "the call stays asynchronous"
BATCH = "read on the host"
BASES_BATCH = "in order on `stream`"
PREPARED = "the same on device pointers, in order on `stream`"
LAUNCH = "enqueues the kernels and the"
SHARED = "Finish each"
RUN_SYNC = "the call returns after the result is there"
BASES_SYNC = "as in mlhip_msm_run"
GENERAL_SYNC = "returns only when its work is done"


def _rows():
    rows = []
    turn = [0]

    def add(tag, entry, make, promise, sync=None, host_args=()):
        cid = turn[0] % 3  # the three curves in turn: the stream plumbing is per curve in the ops table
        turn[0] += 1
        rows.append(Row("%s-%s" % (tag, NAMES[cid]), entry, functools.partial(make, cid), promise, sync, tuple(host_args)))

    add("miller-ppp1", "mlhip_miller_loop_device", lambda c: Miller(c, "miller", 1), IN_ORDER)
    add("miller-ppp4", "mlhip_miller_loop_device", lambda c: Miller(c, "miller", 4), IN_ORDER)
    add("final-exp", "mlhip_final_exp_device", lambda c: Miller(c, "final_exp"), IN_ORDER)
    add("pairing-batch", "mlhip_pairing_batch_device", lambda c: Miller(c, "pairing"), IN_ORDER)
    add("gt-mul", "mlhip_gt_mul_device", lambda c: GtOp(c, "mul"), IN_ORDER)
    add("gt-inverse", "mlhip_gt_inverse_device", lambda c: GtOp(c, "inverse"), IN_ORDER)
    add("gt-exp", "mlhip_gt_exp_device", lambda c: GtOp(c, "exp"), IN_ORDER)
    add("gt-exp-cyclo", "mlhip_gt_exp_cyclo_device", lambda c: GtOp(c, "exp_cyclo"), IN_ORDER)
    add("gt-is-member", "mlhip_gt_is_member_device", lambda c: GtCheck(c, "is_member"), IN_ORDER)
    add("gt-from-bytes", "mlhip_gt_from_bytes_device", lambda c: GtCheck(c, "from_bytes"), IN_ORDER)
    add("gt-to-bytes", "mlhip_gt_to_bytes_device", lambda c: GtOp(c, "to_bytes"), IN_ORDER)
    add("g1-from-bytes", "mlhip_g1_from_bytes_device", lambda c: PointCodec(c, 1, True), IN_ORDER)
    add("g2-from-bytes", "mlhip_g2_from_bytes_device", lambda c: PointCodec(c, 2, True), IN_ORDER)
    add("g1-to-bytes", "mlhip_g1_to_bytes_device", lambda c: PointCodec(c, 1, False), IN_ORDER)
    add("g2-to-bytes", "mlhip_g2_to_bytes_device", lambda c: PointCodec(c, 2, False), IN_ORDER)
    add("fp-mul", "mlhip_fp_mul_device", lambda c: FpMul(c), IN_ORDER)
    for g in (1, 2):
        add("scalar-mul-g%d" % g, "mlhip_scalar_mul_device", lambda c, g=g: ScalarMul(c, g, 1, 300), IN_ORDER)
    for g in (1, 2):
        add("scalar-mul-fixed-g%d" % g, "mlhip_scalar_mul_device", lambda c, g=g: ScalarMul(c, g, 0, 2048), SCALAR_MUL)
    for g in (1, 2):
        add("msm-batch-g%d" % g, "mlhip_msm_batch_device", lambda c, g=g: MsmBatch(c, g), BATCH, None, ["offsets"])
    add("bases-batch-indexed", "mlhip_bases_msm_batch_device", lambda c: BasesBatch(c, 1, True), BASES_BATCH, None,
        ["offsets", "base_index"])
    add("bases-batch-positional", "mlhip_bases_msm_batch_device", lambda c: BasesBatch(c, 2, False), BASES_BATCH, None, ["offsets"])
    add("bases-batch-table-free", "mlhip_bases_msm_batch_device", lambda c: BasesBatch(c, 1, True, True), BASES_BATCH, None,
        ["offsets", "base_index"])
    add("bases-msm", "mlhip_bases_msm_device", lambda c: BasesMsm(c), BASES_SYNC, BASES_SYNC)
    for fused, entry in ((False, "mlhip_miller_loop_prepared_device"), (True, "mlhip_pairing_prepared_device")):
        tag = "prepared-pairing" if fused else "prepared-miller"
        add(tag, entry, lambda c, f=fused: Prepared(c, f), PREPARED, None, ["q_index"])
        add(tag + "-general", entry, lambda c, f=fused: Prepared(c, f, True), PREPARED, GENERAL_SYNC, ["q_index"])
    for how, entry in (("run", "mlhip_msm_run"), ("launch", "mlhip_msm_launch")):
        for g in (1, 2):
            for tile in (10, 0):
                add("msm-%s-g%d-tile%d" % (how, g, tile), entry, lambda c, g=g, h=how, t=tile: Msm(c, g, h, t),
                    RUN_SYNC if how == "run" else LAUNCH, RUN_SYNC if how == "run" else None)
    add("msm-launch-shared", "mlhip_msm_launch_shared", lambda c: MsmShared(c), SHARED)
    return rows


ROWS = _rows()
ROWS_BY_ID = {r.id: r for r in ROWS}


def row_for(entry, index=0):
    return [r for r in ROWS if r.entry == entry][index]


# ---------------------------------------------------------------------------------------------------------------------
# the delay
# ---------------------------------------------------------------------------------------------------------------------
class Delay:
    """k_fp_mul on 2^16 lanes with `repeat` dependent products each, calibrated to about 100 ms"""

    CURVE = 1
    LANES = 1 << 16
    TARGET_MS = 100.0
    CHECKED = (0, 31337, LANES - 1)

    def __init__(self, lib, mlhip):
        import torch

        self.lib, self.mlhip = lib, mlhip
        self.a_host, self.b_host = _fp_values(self.CURVE, 400, self.LANES), _fp_values(self.CURVE, 401, self.LANES)
        self.a, self.b = to_dev(self.a_host), to_dev(self.b_host)
        self.out = torch.zeros(len(self.a_host), dtype=torch.uint8, device="cuda")
        self.out2 = torch.zeros_like(self.out)  # of a second delay that runs beside the first on another stream
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        self.repeat = 256
        self._timed(st)  # loads the code object
        first = self._timed(st)
        self.repeat = max(256, int(round(256 * self.TARGET_MS / first)))
        self.ms = self._timed(st)
        self.check()

    def _timed(self, st):
        import torch

        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        self.queue(st)
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1)

    def queue(self, stream, second=False):
        out = self.out2 if second else self.out
        self.mlhip.check(self.lib.mlhip_fp_mul_device(self.CURVE, self.a.data_ptr(), self.b.data_ptr(), self.LANES, self.repeat,
                                                      out.data_ptr(), stream.cuda_stream))

    def independent_stream(self, s, tries=12):
        """A stream whose work does not queue up behind the work on s.  The runtime multiplexes its streams onto a few hardware
        queues (four by default), and two streams that land on the same one run one after the other: a call on such a stream
        would wait for the delay on s like a call on s itself.  Probe: with the delay on s, a small upload and a fill on the
        candidate must finish in less than a quarter of the delay."""
        import torch

        small = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        behind = torch.zeros_like(small)
        src = torch.ones(4096, dtype=torch.uint8)  # pageable host memory, as the tables the library uploads
        torch.cuda.synchronize()
        seen = []
        for _ in range(tries):
            c = torch.cuda.Stream()
            if c.cuda_stream == s.cuda_stream:
                continue
            with torch.cuda.stream(s):
                self.queue(s)
                behind.copy_(small, non_blocking=True)  # a producer's copy waiting behind the delay, as in the scenario
            t0 = time.perf_counter()
            with torch.cuda.stream(c):
                small.copy_(src, non_blocking=True)
                small.fill_(2)
            c.synchronize()
            ms = 1e3 * (time.perf_counter() - t0)
            s.synchronize()
            seen.append(round(ms, 2))
            if ms < self.ms / 4:
                self.probed = seen
                return c
        raise AssertionError("none of %d streams ran beside the busy one (ms until each was done: %s; the delay is %.1f ms)"
                             % (len(seen), seen, self.ms))

    def clear(self):
        import torch

        self.out.zero_()
        self.out2.zero_()
        torch.cuda.synchronize()

    def check(self, second=False):
        """three lanes of the output against a b^repeat: the delay ran to completion"""
        f = FPB[self.CURVE]
        got = to_host(self.out2 if second else self.out)
        for i in self.CHECKED:
            want = fp_mul_expected(self.CURVE, self.a_host[i * f : (i + 1) * f], self.b_host[i * f : (i + 1) * f], self.repeat)
            assert got[i * f : (i + 1) * f] == want, ("delay lane", i)


# ---------------------------------------------------------------------------------------------------------------------
# the scenario
# ---------------------------------------------------------------------------------------------------------------------
def to_dev(data):
    import torch

    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.current_stream().synchronize()
    return t


def to_host(t):
    return bytes(t.cpu().numpy().tobytes())


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


Outcome = namedtuple("Outcome", "busy call_ms")


def run_scenario(lib, mlhip, case, stream, delay, log, label, sync=None):
    """One entry point on one busy stream (the module docstring of tests/test_stream_order_gpu.py lists the steps).  The caller has
    set case.env.  Asserts the bytes; returns (busy, host milliseconds of the call)."""
    import torch

    real, decoy = [to_dev(b) for b in case.real], [to_dev(b) for b in case.decoy]
    ins = [t.clone() for t in decoy]
    outs = [torch.full((sz,), 0xA5, dtype=torch.uint8, device="cuda") for sz in case.out_bytes]
    snap = [torch.zeros_like(t) for t in outs]
    host = case.host_arrays(case.host_real)
    host_values = {k: (t, list(v)) for k, (t, v) in case.host_real.items()}
    want = case.oracle(case.real, host_values)
    case.open(lib, mlhip)
    try:
        # 1. warm-up on the idle stream, real inputs: sizes every scratch buffer, and gives the first expected value
        delay.clear()
        res = case.call(lib, mlhip, _ptrs(real), _ptrs(outs), host, stream.cuda_stream)
        res = res + case.finish(lib, mlhip)
        stream.synchronize()
        warm = [to_host(t) for t in outs] + res
        form = case.host_form(lib, mlhip, case.real, host)
        for t in outs:
            t.fill_(0xA5)
        torch.cuda.synchronize()
        # 2. the delay, then the producer of every input (read after write)
        with torch.cuda.stream(stream):
            delay.queue(stream)
            for t, r in zip(ins, real):
                t.copy_(r, non_blocking=True)
        # 3. the call
        t0 = time.perf_counter()
        res = case.call(lib, mlhip, _ptrs(ins), _ptrs(outs), host, stream.cuda_stream)
        call_ms = 1e3 * (time.perf_counter() - t0)
        # 4. the host arguments are the caller's again
        for name, arr in host.items():
            other = case.host_other[name][1]
            assert len(other) == len(case.host_real[name][1])
            for i, v in enumerate(other):
                arr[i] = v
        # 5. snapshot of the output, then inputs and output are overwritten (write after read)
        with torch.cuda.stream(stream):
            for sn, t in zip(snap, outs):
                sn.copy_(t, non_blocking=True)
            for t, d in zip(ins, decoy):
                t.copy_(d, non_blocking=True)
            for t in outs:
                t.fill_(0x5A)
        # 6. was the stream still busy when all of that had been queued?
        busy = not stream.query()
        res = res + case.finish(lib, mlhip)
        # 7.
        stream.synchronize()
        got = [to_host(t) for t in snap] + res
        log("%-34s %-28s busy %d  call %8.3f ms  (%s)" % (case_entry(label), label, busy, call_ms, "synchronous by contract" if sync else "asynchronous"))
        delay.check()
        assert got == warm, (label, "differs from the call on the idle stream")
        if form is not None:
            assert got == form, (label, "differs from the host form")
        assert case.canon(lib, mlhip, got) == want, (label, "differs from the oracle")
        if sync is None:
            assert busy, (label, "the call returned only after the stream had drained (%.1f ms; the delay is %.1f ms)" % (call_ms, delay.ms))
            assert call_ms < delay.ms / 2, (label, call_ms, delay.ms)
        return Outcome(busy, call_ms)
    finally:
        torch.cuda.synchronize()
        case.close(lib)


def case_entry(label):
    r = ROWS_BY_ID.get(label.split("@")[0])
    return r.entry if r else ""


def run_negative_control(lib, mlhip, case, delay, log, label, attempts=3):
    """The call on an idle stream s2 while the producer of its inputs waits behind the delay on ANOTHER stream s: it must see the
    decoys.  Every byte it reads is valid memory holding valid inputs.
    The control says something only if s2 really runs beside s.  The runtime multiplexes streams onto a few hardware queues, and
    work on one of them can be held up behind the delay by the hardware whatever stream order says: s2 is therefore picked with
    Delay.independent_stream, and an attempt in which the call on s2 still took half the delay or more (timed on the host up to
    the end of s2.synchronize()) is void and repeated on fresh streams, `attempts` times at the most.  An attempt in which the
    call did run beside the delay must give the decoys' value: that is never repeated."""
    import torch

    real, decoy = [to_dev(b) for b in case.real], [to_dev(b) for b in case.decoy]
    outs = [torch.full((sz,), 0xA5, dtype=torch.uint8, device="cuda") for sz in case.out_bytes]
    host = case.host_arrays(case.host_real)
    host_values = {k: (t, list(v)) for k, (t, v) in case.host_real.items()}
    want_decoy, want_real = case.oracle(case.decoy, host_values), case.oracle(case.real, host_values)
    assert want_decoy != want_real
    case.open(lib, mlhip)
    try:
        notes = []
        for _ in range(attempts):
            s = torch.cuda.Stream()
            s2 = delay.independent_stream(s)
            ins = [t.clone() for t in decoy]
            for t in outs:
                t.fill_(0xA5)
            delay.clear()
            case.call(lib, mlhip, _ptrs(real), _ptrs(outs), host, s2.cuda_stream)  # warm-up: sizes the scratch
            torch.cuda.synchronize()
            assert [to_host(t) for t in outs] == want_real
            for t in outs:
                t.fill_(0xA5)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                delay.queue(s)
                for t, r in zip(ins, real):
                    t.copy_(r, non_blocking=True)
            t0 = time.perf_counter()
            case.call(lib, mlhip, _ptrs(ins), _ptrs(outs), host, s2.cuda_stream)
            s2.synchronize()
            done_ms = 1e3 * (time.perf_counter() - t0)
            held = not s.query()
            got = [to_host(t) for t in outs]
            s.synchronize()
            delay.check()
            assert [to_host(t) for t in ins] == case.real  # the producer did run afterwards
            what = "the real inputs' value" if got == want_real else "the decoys' value" if got == want_decoy else "neither value"
            notes.append("%s after %.2f ms, s still busy %d, stream probe %s" % (what, done_ms, held, delay.probed))
            log("%-34s %-28s negative control: %s" % (case_entry(label), label, notes[-1]))
            if held and done_ms < delay.ms / 2:
                assert got == want_decoy, "the call did not see the decoys although it ran beside the delay (%.1f ms): %s" % (delay.ms, notes)
                return
        raise AssertionError("in %d attempts the call on the other stream never ran beside the delay (%.1f ms): %s" % (attempts, delay.ms, notes))
    finally:
        torch.cuda.synchronize()
        case.close(lib)
