"""ctypes binding of libmlhip.so (C ABI: include/mlhip.h).

The library is the product; this module only declares argument types.  There is no fallback of any
kind: if the shared object is missing, or a call fails (no GPU, HIP error), an exception is raised.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_float, c_int, c_size_t, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
# MLHIP_LIB=<path> loads another build of the same library (A/B measurements of kernel variants on one box)
LIB_PATH = os.environ.get("MLHIP_LIB") or os.path.join(HERE, "libmlhip.so")

CURVE_BN254, CURVE_BLS12_381, CURVE_BLS12_377 = 0, 1, 2
GROUP_G1, GROUP_G2 = 1, 2
EINVAL = -1
ENODEVICE = -2

# every symbol include/mlhip.h declares (tests/test_abi.py checks the library exports them all)
SYMBOLS = [
    "mlhip_version",
    "mlhip_last_error",
    "mlhip_device_count",
    "mlhip_set_device",
    "mlhip_init",
    "mlhip_get_devices",
    "mlhip_shutdown",
    "mlhip_msm_multi",
    "mlhip_bases_create_multi",
    "mlhip_sizes",
    "mlhip_msm_g1",
    "mlhip_msm_g2",
    "mlhip_miller_loop",
    "mlhip_final_exp",
    "mlhip_pairing_batch",
    "mlhip_gt_mul",
    "mlhip_gt_exp",
    "mlhip_gt_exp_cyclo",
    "mlhip_pairing_product",
    "mlhip_msm_plan_create",
    "mlhip_msm_plan_destroy",
    "mlhip_msm_run",
    "mlhip_msm_launch",
    "mlhip_msm_launch_shared",
    "mlhip_msm_g1g2",
    "mlhip_msm_finish",
    "mlhip_msm_plan_set_profiling",
    "mlhip_msm_plan_assume_srs",
    "mlhip_msm_plan_timings",
    "mlhip_miller_loop_device",
    "mlhip_final_exp_device",
    "mlhip_pairing_batch_device",
    "mlhip_gt_mul_device",
    "mlhip_gt_exp_device",
    "mlhip_gt_exp_cyclo_device",
    "mlhip_gt_from_bytes",
    "mlhip_gt_to_bytes",
    "mlhip_gt_from_bytes_device",
    "mlhip_gt_to_bytes_device",
    "mlhip_gt_is_member",
    "mlhip_gt_is_member_device",
    "mlhip_gt_inverse",
    "mlhip_gt_inverse_device",
    "mlhip_scalar_mul_device",
    "mlhip_scalar_mul",
    "mlhip_msm_batch_device",
    "mlhip_msm_batch",
    "mlhip_bases_create",
    "mlhip_bases_msm",
    "mlhip_bases_create_device",
    "mlhip_bases_msm_device",
    "mlhip_bases_plan",
    "mlhip_bases_checked_subgroup",
    "mlhip_bases_destroy",
    "mlhip_bases_msm_batch",
    "mlhip_bases_msm_batch_device",
    "mlhip_bases_batch_tabled",
    "mlhip_g2_prepared_create",
    "mlhip_g2_prepared_create_device",
    "mlhip_g2_prepared_count",
    "mlhip_g2_prepared_destroy",
    "mlhip_miller_loop_prepared",
    "mlhip_miller_loop_prepared_device",
    "mlhip_pairing_prepared",
    "mlhip_pairing_prepared_device",
    "mlhip_release_cache",
    "mlhip_g1_from_bytes",
    "mlhip_g1_to_bytes",
    "mlhip_g1_from_bytes_device",
    "mlhip_g1_to_bytes_device",
    "mlhip_g2_from_bytes",
    "mlhip_g2_to_bytes",
    "mlhip_g2_from_bytes_device",
    "mlhip_g2_to_bytes_device",
    "mlhip_g1_sum",
    "mlhip_g2_sum",
    "mlhip_fp_mul_device",
]


class MlhipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("libmlhip error %d: %s" % (code, msg))
        self.code = code


_lib = None
ALT_PATH = os.path.join(HERE, "libmlhip_alt.so")  # the test build (python -m mathlib_amd.build --alt)
_alt = None
_use_alt = False


class _Active:
    """What load() hands out: the product library -- or, while a TEST has asked for a second implementation the product
    does not contain (tests/conftest.py: use_alt), the test build.  Attribute access goes to whichever is active, so the
    `lib` objects tests already hold follow the switch.  Nothing outside the tests ever calls use_alt."""

    def __getattr__(self, name):
        return getattr(_alt if (_use_alt and _alt is not None) else _lib, name)


_active = _Active()


def alt_available() -> bool:
    """Is an up-to-date test build next to the product library?  (build.py stamps both with the hash of the sources.)"""
    if LIB_PATH == ALT_PATH:
        return True
    try:
        from .build import source_hash

        with open(ALT_PATH + ".srchash") as f:
            return os.path.exists(ALT_PATH) and f.read().strip() == source_hash()
    except OSError:
        return False


def concrete():
    """The library that is active right now, as the ctypes object itself: what an object that owns a library handle (MsmPlan,
    driver.Bases) binds at creation, so that the handle is used and destroyed by the library that made it whatever is active
    later."""
    load()
    return _alt if (_use_alt and _alt is not None) else _lib


def use_alt(on: bool) -> None:
    """Tests only: route every call through the test build (True) or back to the product library (False)."""
    global _alt, _use_alt
    if on and _alt is None and LIB_PATH != ALT_PATH:
        load()
        _alt = _bind(ctypes.CDLL(ALT_PATH))
    _use_alt = bool(on)


def load():
    """Load libmlhip.so; raises if it has not been built (python -m mathlib_amd.build)."""
    global _lib
    if _lib is not None:
        return _active
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "mathlib_amd: %s is missing -- the HIP extension has not been built "
            "(run `python -m mathlib_amd.build`); there is no CPU fallback" % LIB_PATH
        )
    # PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7) but its libraries ask for
    # it by file name; if /opt/rocm's copy is mapped first the process ends up with two HIP runtimes
    # and the second one sees no GPU.  Import torch first so both share one runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    _lib = _bind(ctypes.CDLL(LIB_PATH))
    return _active


def _bind(lib: ctypes.CDLL) -> ctypes.CDLL:
    """argument and result types of every entry point"""
    vp, sz, ci = c_void_p, c_size_t, c_int
    lib.mlhip_version.restype = ci
    lib.mlhip_last_error.restype = c_char_p
    lib.mlhip_device_count.argtypes = [POINTER(ci)]
    lib.mlhip_set_device.argtypes = [ci]
    lib.mlhip_init.argtypes = [POINTER(ci), ci]
    lib.mlhip_get_devices.argtypes = [POINTER(ci), ci]
    lib.mlhip_shutdown.argtypes = []
    lib.mlhip_msm_multi.argtypes = [ci, ci, POINTER(ci), ci, vp, vp, ci, sz, ci, vp]
    lib.mlhip_bases_create_multi.argtypes = [ci, ci, POINTER(ci), ci, vp, sz, ci, ctypes.POINTER(c_void_p)]
    lib.mlhip_sizes.argtypes = [ci, POINTER(sz), POINTER(sz), POINTER(sz), POINTER(sz)]
    for f in (lib.mlhip_msm_g1, lib.mlhip_msm_g2):
        f.argtypes = [ci, vp, vp, ci, sz, ci, vp]
    lib.mlhip_msm_g1g2.argtypes = [ci, vp, vp, vp, ci, sz, ci, vp, vp]
    lib.mlhip_miller_loop.argtypes = [ci, vp, vp, sz, sz, vp]
    lib.mlhip_final_exp.argtypes = [ci, vp, sz, vp]
    lib.mlhip_pairing_batch.argtypes = [ci, vp, vp, sz, vp]
    lib.mlhip_gt_mul.argtypes = [ci, vp, vp, sz, vp]
    lib.mlhip_gt_exp.argtypes = [ci, vp, vp, ci, sz, vp]
    lib.mlhip_gt_exp_cyclo.argtypes = [ci, vp, vp, ci, sz, vp]
    lib.mlhip_pairing_product.argtypes = [ci, vp, vp, sz, vp]
    lib.mlhip_gt_exp_device.argtypes = [ci, vp, vp, ci, sz, vp, vp]
    lib.mlhip_gt_exp_cyclo_device.argtypes = [ci, vp, vp, ci, sz, vp, vp]
    lib.mlhip_gt_from_bytes.argtypes = [ci, vp, sz, ci, vp, vp]
    lib.mlhip_gt_to_bytes.argtypes = [ci, vp, sz, vp]
    lib.mlhip_gt_from_bytes_device.argtypes = [ci, vp, sz, ci, vp, vp, vp]
    lib.mlhip_gt_to_bytes_device.argtypes = [ci, vp, sz, vp, vp]
    lib.mlhip_gt_is_member.argtypes = [ci, vp, sz, vp]
    lib.mlhip_gt_is_member_device.argtypes = [ci, vp, sz, vp, vp]
    lib.mlhip_gt_inverse.argtypes = [ci, vp, sz, vp]
    lib.mlhip_gt_inverse_device.argtypes = [ci, vp, sz, vp, vp]
    lib.mlhip_msm_plan_create.argtypes = [ci, ci, sz, ci, POINTER(vp)]
    lib.mlhip_msm_plan_destroy.argtypes = [vp]
    lib.mlhip_msm_run.argtypes = [vp, vp, vp, ci, sz, vp, vp, vp]
    lib.mlhip_msm_launch.argtypes = [vp, vp, vp, ci, sz, vp]
    lib.mlhip_msm_launch_shared.argtypes = [vp, vp, vp, vp, vp, ci, sz, vp]
    lib.mlhip_msm_finish.argtypes = [vp, vp, vp]
    lib.mlhip_msm_plan_set_profiling.argtypes = [vp, ci]
    lib.mlhip_msm_plan_assume_srs.argtypes = [vp, ci]
    lib.mlhip_msm_plan_timings.argtypes = [vp, POINTER(c_float), ci]
    lib.mlhip_miller_loop_device.argtypes = [ci, vp, vp, sz, sz, vp, vp]
    lib.mlhip_final_exp_device.argtypes = [ci, vp, sz, vp, vp]
    lib.mlhip_pairing_batch_device.argtypes = [ci, vp, vp, sz, vp, vp]
    lib.mlhip_gt_mul_device.argtypes = [ci, vp, vp, sz, vp, vp]
    lib.mlhip_scalar_mul_device.argtypes = [ci, ci, vp, sz, vp, ci, sz, vp, vp]
    lib.mlhip_scalar_mul.argtypes = [ci, ci, vp, sz, vp, ci, sz, vp]
    lib.mlhip_msm_batch_device.argtypes = [ci, ci, vp, vp, ci, vp, sz, vp, vp]
    lib.mlhip_msm_batch.argtypes = [ci, ci, vp, vp, ci, vp, sz, vp]
    lib.mlhip_bases_create.argtypes = [ci, ci, vp, sz, ci, ctypes.POINTER(c_void_p)]
    lib.mlhip_bases_msm.argtypes = [vp, vp, ci, sz, vp]
    lib.mlhip_bases_create_device.argtypes = [ci, ci, vp, sz, ci, ctypes.POINTER(c_void_p)]
    lib.mlhip_bases_msm_device.argtypes = [vp, vp, ci, sz, vp, vp]
    lib.mlhip_bases_plan.argtypes = [vp]
    lib.mlhip_bases_plan.restype = c_void_p
    lib.mlhip_bases_destroy.argtypes = [vp]
    lib.mlhip_bases_checked_subgroup.argtypes = [vp]
    lib.mlhip_bases_msm_batch.argtypes = [vp, vp, ci, vp, vp, sz, vp]
    lib.mlhip_bases_msm_batch_device.argtypes = [vp, vp, ci, vp, vp, sz, vp, vp]
    lib.mlhip_bases_batch_tabled.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
    lib.mlhip_g2_prepared_create.argtypes = [ci, vp, sz, ctypes.POINTER(c_void_p)]
    lib.mlhip_g2_prepared_create_device.argtypes = [ci, vp, sz, ctypes.POINTER(c_void_p)]
    lib.mlhip_g2_prepared_count.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
    lib.mlhip_g2_prepared_destroy.argtypes = [vp]
    for f in (lib.mlhip_miller_loop_prepared, lib.mlhip_pairing_prepared):
        f.argtypes = [vp, vp, vp, sz, sz, vp]
    for f in (lib.mlhip_miller_loop_prepared_device, lib.mlhip_pairing_prepared_device):
        f.argtypes = [vp, vp, vp, sz, sz, vp, vp]
    lib.mlhip_g1_from_bytes.argtypes = [ci, vp, sz, ci, ci, vp, vp]
    lib.mlhip_g1_to_bytes.argtypes = [ci, vp, sz, ci, vp]
    lib.mlhip_g1_from_bytes_device.argtypes = [ci, vp, sz, ci, ci, vp, vp, vp]
    lib.mlhip_g1_to_bytes_device.argtypes = [ci, vp, sz, ci, vp, vp]
    lib.mlhip_g2_from_bytes.argtypes = [ci, vp, sz, ci, ci, vp, vp]
    lib.mlhip_g2_to_bytes.argtypes = [ci, vp, sz, ci, vp]
    lib.mlhip_g2_from_bytes_device.argtypes = [ci, vp, sz, ci, ci, vp, vp, vp]
    lib.mlhip_g2_to_bytes_device.argtypes = [ci, vp, sz, ci, vp, vp]
    lib.mlhip_g1_sum.argtypes = [ci, vp, sz, vp]
    lib.mlhip_g2_sum.argtypes = [ci, vp, sz, vp]
    lib.mlhip_fp_mul_device.argtypes = [ci, vp, vp, sz, ci, vp, vp]
    for name in SYMBOLS:
        if name not in ("mlhip_last_error", "mlhip_bases_plan"):
            getattr(lib, name).restype = ci
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise MlhipError(rc, load().mlhip_last_error().decode(errors="replace"))


def sizes(curve: int):
    lib = load()
    a, b, c, d = c_size_t(), c_size_t(), c_size_t(), c_size_t()
    check(lib.mlhip_sizes(curve, byref(a), byref(b), byref(c), byref(d)))
    return a.value, b.value, c.value, d.value


def batch_offsets(lengths):
    """the offsets array of mlhip_msm_batch* (K + 1 uint64 entries) for segments of these lengths"""
    offs = (ctypes.c_uint64 * (len(lengths) + 1))()
    t = 0
    for i, m in enumerate(lengths):
        t += m
        offs[i + 1] = t
    return offs


def msm_batch(curve: int, group: int, points: bytes, scalars: bytes, scalars_mont: bool, lengths, subgroup: bool = False):
    """mlhip_msm_batch: one affine point (bytes) per segment; segment i has lengths[i] consecutive pairs.  subgroup: the
    caller promises that every point is in the prime-order subgroup or at infinity (mlhip_msm_batch_subgroup)"""
    _, g1, g2, _ = sizes(curve)
    ptsz = g1 if group == GROUP_G1 else g2
    k = len(lengths)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k * ptsz)
    call = msm_batch_subgroup if subgroup else (lambda lib, *args: lib.mlhip_msm_batch(*args))
    check(call(load(), curve, group, points, scalars, 1 if scalars_mont else 0, batch_offsets(lengths), k, out))
    raw = out.raw
    return [raw[i * ptsz : (i + 1) * ptsz] for i in range(k)]


def window_bits(window_c: int, scalar_bits: int) -> int:
    """MLHIP_WINDOW_BITS of include/mlhip.h: a window width and a scalar width in one window_c argument"""
    return (0xFF if not 0 <= window_c <= 255 else window_c) | ((0x3FF if not 0 <= scalar_bits <= 256 else scalar_bits) << 8)


def mlhip_msm_plan_create_bits(lib, curve: int, group: int, max_n: int, window_c: int, scalar_bits: int, plan_ref) -> int:
    """include/mlhip_bits.h: a plan for scalars below 2^scalar_bits (the return code, as the C function)"""
    return lib.mlhip_msm_plan_create(curve, group, max_n, window_bits(window_c, scalar_bits), plan_ref)


def mlhip_msm_plan_scalar_bits(lib, plan):
    """include/mlhip_bits.h: (return code, the width the plan was made for)"""
    buf = (c_float * 12)()
    k = lib.mlhip_msm_plan_timings(plan, buf, 12)
    return (k, 0) if k < 0 else (EINVAL, 0) if k < 12 else (0, int(buf[11]))


def mlhip_msm_bits(lib, curve: int, group: int, points, scalars, scalars_mont: int, scalar_bits: int, n: int, window_c: int, out) -> int:
    """include/mlhip_bits.h: mlhip_msm_g1 / mlhip_msm_g2 for short scalars (the return code, as the C function)"""
    if group not in (GROUP_G1, GROUP_G2):
        return EINVAL
    fn = lib.mlhip_msm_g1 if group == GROUP_G1 else lib.mlhip_msm_g2
    return fn(curve, points, scalars, scalars_mont, n, window_bits(window_c, scalar_bits), out)


def msm_bits(curve: int, group: int, points, scalars, scalars_mont: bool, scalar_bits: int, n: int, window_c: int = 0) -> bytes:
    """mlhip_msm_bits: sum_i [(s_i mod r) mod 2^scalar_bits] P_i over host buffers, as one affine point (bytes)"""
    _, g1, g2, _ = sizes(curve)
    out = ctypes.create_string_buffer(g1 if group == GROUP_G1 else g2)
    check(mlhip_msm_bits(load(), curve, group, points, scalars, 1 if scalars_mont else 0, scalar_bits, n, window_c, out))
    return out.raw


def GROUP_SUBGROUP(group: int) -> int:
    """MLHIP_GROUP_SUBGROUP of include/mlhip.h: the group argument of mlhip_scalar_mul / _device with the caller's promise
    that every point is in the prime-order subgroup (or at infinity); -1, which the library rejects, for any other group"""
    return (group | 0x100) if group in (GROUP_G1, GROUP_G2) else -1


def scalar_mul_subgroup(lib, curve: int, group: int, points, point_stride: int, scalars, scalars_mont: int, n: int, out) -> int:
    """include/mlhip_subgroup.h: mlhip_scalar_mul for points promised in G1 / G2 (the return code, as the C function)"""
    return lib.mlhip_scalar_mul(curve, GROUP_SUBGROUP(group), points, point_stride, scalars, scalars_mont, n, out)


def scalar_mul_subgroup_device(lib, curve: int, group: int, d_points, point_stride: int, d_scalars, scalars_mont: int, n: int,
                               d_out, stream) -> int:
    """include/mlhip_subgroup.h: the same on device pointers, asynchronous and in order on `stream`"""
    return lib.mlhip_scalar_mul_device(curve, GROUP_SUBGROUP(group), d_points, point_stride, d_scalars, scalars_mont, n, d_out, stream)


def CURVE_SUBGROUP_POINTS(curve: int) -> int:
    """MLHIP_CURVE_SUBGROUP_POINTS of include/mlhip.h: the curve id of mlhip_msm_batch / _device with the caller's promise that
    every point is in the prime-order subgroup (or at infinity); -1, which the library rejects, for any other curve id"""
    return (curve | 0x100) if 0 <= curve <= 2 else -1


def msm_batch_subgroup(lib, curve: int, group: int, points, scalars, scalars_mont: int, offsets, k: int, out) -> int:
    """include/mlhip_subgroup.h: mlhip_msm_batch for points promised in G1 / G2 (the return code, as the C function)"""
    return lib.mlhip_msm_batch(CURVE_SUBGROUP_POINTS(curve), group, points, scalars, scalars_mont, offsets, k, out)


def msm_batch_subgroup_device(lib, curve: int, group: int, d_points, d_scalars, scalars_mont: int, offsets, k: int, d_out,
                              stream) -> int:
    """include/mlhip_subgroup.h: the same on device pointers, asynchronous and in order on `stream`"""
    return lib.mlhip_msm_batch_device(CURVE_SUBGROUP_POINTS(curve), group, d_points, d_scalars, scalars_mont, offsets, k, d_out, stream)


SCALARS_UNIT = 0x400
"""MLHIP_SCALARS_UNIT of include/mlhip.h: the scalars_mont argument of the four batch entry points that says every scalar is 1"""


def mlhip_sum_batch(lib, curve: int, group: int, points, offsets, k: int, out) -> int:
    """include/mlhip_sum_batch.h: K point sums in one call (the return code, as the C function)"""
    return lib.mlhip_msm_batch(curve, group, points, None, SCALARS_UNIT, offsets, k, out)


def mlhip_sum_batch_device(lib, curve: int, group: int, d_points, offsets, k: int, d_out, stream) -> int:
    """include/mlhip_sum_batch.h: the same on device pointers, asynchronous and in order on `stream`"""
    return lib.mlhip_msm_batch_device(curve, group, d_points, None, SCALARS_UNIT, offsets, k, d_out, stream)


def mlhip_bases_sum_batch(lib, handle, base_index, offsets, k: int, out) -> int:
    """include/mlhip_sum_batch.h: K sums over the resident bases of a handle (the return code, as the C function)"""
    return lib.mlhip_bases_msm_batch(handle, None, SCALARS_UNIT, base_index, offsets, k, out)


def mlhip_bases_sum_batch_device(lib, handle, base_index, offsets, k: int, stream, d_out) -> int:
    """include/mlhip_sum_batch.h: the same with device outputs, in order on `stream`"""
    return lib.mlhip_bases_msm_batch_device(handle, None, SCALARS_UNIT, base_index, offsets, k, stream, d_out)


def sum_batch(curve: int, group: int, points: bytes, lengths):
    """mlhip_sum_batch: one affine point (bytes) per segment; segment i is lengths[i] consecutive points"""
    _, g1, g2, _ = sizes(curve)
    ptsz = g1 if group == GROUP_G1 else g2
    k = len(lengths)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k * ptsz)
    check(mlhip_sum_batch(load(), curve, group, points, batch_offsets(lengths), k, out))
    raw = out.raw
    return [raw[i * ptsz : (i + 1) * ptsz] for i in range(k)]


def bases_sum_batch(lib, handle, ptsz: int, lengths, index_lists=None):
    """mlhip_bases_sum_batch on the handle `handle` of `lib` (points of ptsz bytes): one affine point (bytes) per segment;
    segment i sums lengths[i] bases, those index_lists[i] names or (without index lists) the first lengths[i]"""
    k = len(lengths)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k * ptsz)
    check(mlhip_bases_sum_batch(lib, handle, batch_index(index_lists), batch_offsets(lengths), k, out))
    raw = out.raw
    return [raw[i * ptsz : (i + 1) * ptsz] for i in range(k)]


WINDOW_DEVICE_RESULT = 1 << 20
"""MLHIP_WINDOW_DEVICE_RESULT of include/mlhip.h: OR-ed onto a plain window_c or onto window_bits(c, bits)"""


def mlhip_msm_plan_create_device_result(lib, curve: int, group: int, max_n: int, window_c: int, scalar_bits: int, plan_ref) -> int:
    """include/mlhip_device_result.h: a plan that leaves its result in device memory (the return code, as the C function)"""
    return lib.mlhip_msm_plan_create(curve, group, max_n, window_bits(window_c, scalar_bits) | WINDOW_DEVICE_RESULT, plan_ref)


def mlhip_msm_plan_is_device_result(lib, plan):
    """include/mlhip_device_result.h: (return code, 1 for a device-result plan / 0 for a host-result one)"""
    buf = (c_float * 13)()
    k = lib.mlhip_msm_plan_timings(plan, buf, 13)
    return (k, 0) if k < 0 else (EINVAL, 0) if k < 13 else (0, int(buf[12] != 0.0))


def mlhip_msm_run_device(lib, plan, d_points, d_scalars, scalars_mont: int, n: int, stream, d_out_affine, d_out_xyzz) -> int:
    """include/mlhip_device_result.h: mlhip_msm_run on a device-result plan, device outputs, in order on `stream`"""
    rc, on = mlhip_msm_plan_is_device_result(lib, plan)
    if rc or not on:
        return rc or EINVAL
    return lib.mlhip_msm_run(plan, d_points, d_scalars, scalars_mont, n, stream, d_out_affine, d_out_xyzz)


def mlhip_msm_finish_device(lib, plan, d_out_affine, d_out_xyzz) -> int:
    """include/mlhip_device_result.h: mlhip_msm_finish on a device-result plan: queues the tail and the delivery, no wait"""
    rc, on = mlhip_msm_plan_is_device_result(lib, plan)
    if rc or not on:
        return rc or EINVAL
    return lib.mlhip_msm_finish(plan, d_out_affine, d_out_xyzz)


def mlhip_bases_create_device_result(lib, curve: int, group: int, points, points_on_device: int, n: int, window_c: int, bases_ref) -> int:
    """include/mlhip_device_result.h: a device-result handle over host points or points in the current device's memory"""
    wc = (0xFF if not 0 <= window_c <= 255 else window_c) | WINDOW_DEVICE_RESULT
    fn = lib.mlhip_bases_create_device if points_on_device else lib.mlhip_bases_create
    return fn(curve, group, points, n, wc, bases_ref)


def mlhip_bases_msm_to_device(lib, bases, d_scalars, scalars_mont: int, n: int, stream, d_out_affine) -> int:
    """include/mlhip_device_result.h: mlhip_bases_msm_device on a device-result handle, device output, in order on `stream`"""
    rc, on = mlhip_msm_plan_is_device_result(lib, lib.mlhip_bases_plan(bases))
    if rc or not on:
        return rc or EINVAL
    return lib.mlhip_bases_msm_device(bases, d_scalars, scalars_mont, n, stream, d_out_affine)


def bases_create_device_result(curve: int, group: int, points, n: int, window_c: int = 0, points_on_device: bool = False):
    """a device-result handle (c_void_p) on the library this process runs on; destroy it with mlhip_bases_destroy"""
    h = c_void_p()
    check(mlhip_bases_create_device_result(concrete(), curve, group, points, 1 if points_on_device else 0, n, window_c, byref(h)))
    return h


def batch_index(index_lists):
    """the base_index array of mlhip_bases_msm_batch* (one uint32 per pair, segment after segment), or None"""
    if index_lists is None:
        return None
    flat = [i for lst in index_lists for i in lst]
    return (ctypes.c_uint32 * max(1, len(flat)))(*flat)


def bases_msm_batch(lib, handle, ptsz: int, scalars: bytes, scalars_mont: bool, lengths, index_lists=None):
    """mlhip_bases_msm_batch on the handle `handle` of `lib` (points of ptsz bytes): one affine point (bytes) per segment;
    segment i has lengths[i] consecutive scalars; index_lists[i] (optional) names the base of each of its pairs"""
    k = len(lengths)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k * ptsz)
    check(lib.mlhip_bases_msm_batch(handle, scalars, 1 if scalars_mont else 0, batch_index(index_lists), batch_offsets(lengths), k,
                                    out))
    raw = out.raw
    return [raw[i * ptsz : (i + 1) * ptsz] for i in range(k)]


def bases_batch_tabled(lib, handle) -> int:
    """mlhip_bases_batch_tabled: the number of leading bases of the handle that have batch tables"""
    n = ctypes.c_size_t()
    check(lib.mlhip_bases_batch_tabled(handle, ctypes.byref(n)))
    return n.value


GROUP_SET = 0x200
"""MLHIP_GROUP_SET of include/mlhip.h: the group argument of mlhip_bases_create whose `points` are member handles"""
MSM_SET_ROUTE = 0x100
"""MLHIP_MSM_SET_ROUTE of include/mlhip.h: the scalars_mont argument of mlhip_bases_msm that asks a set for its route"""


def mlhip_bases_set_create(lib, members, k: int, set_ref) -> int:
    """include/mlhip_bases_set.h: a set of k member handles (an array of c_void_p, or None) (the return code, as the C function)"""
    return lib.mlhip_bases_create(0, GROUP_SET, members, k, 0, set_ref)


def mlhip_bases_set_route(lib, handle, info, cap: int) -> int:
    """include/mlhip_bases_set.h: the route of the set's last MSM into the int array `info` (entries written, or the error code)"""
    if cap < 0:
        handle = None
    return lib.mlhip_bases_msm(handle, None, MSM_SET_ROUTE, max(cap, 0), info)


def bases_set_create(lib, handles):
    """mlhip_bases_set_create over the handles (c_void_p) of `lib`: the set (c_void_p); the members are not owned -- destroy
    the set with mlhip_bases_destroy before them"""
    arr = (c_void_p * max(1, len(handles)))(*[h.value if isinstance(h, c_void_p) else h for h in handles])
    s = c_void_p()
    check(mlhip_bases_set_create(lib, arr, len(handles), byref(s)))
    return s


def bases_set_route(lib, handle):
    """mlhip_bases_set_route: (members, sort trains per tile, uploads of the scalar vector, 1 iff every member read tables) of
    the set's last MSM"""
    info = (ctypes.c_int * 4)()
    k = mlhip_bases_set_route(lib, handle, info, 4)
    if k < 0:
        check(k)
    return tuple(info[:k])


def bases_set_msm(lib, handle, ptszs, scalars: bytes, scalars_mont: bool, n: int):
    """mlhip_bases_msm on a set whose members' points have ptszs[i] bytes: one affine point (bytes) per member"""
    out = ctypes.create_string_buffer(sum(ptszs))
    check(lib.mlhip_bases_msm(handle, scalars, 1 if scalars_mont else 0, n, out))
    raw, res, off = out.raw, [], 0
    for sz_ in ptszs:
        res.append(raw[off : off + sz_])
        off += sz_
    return res


def q_index_array(index, ppp: int):
    """the q_index array of mlhip_*_prepared* (ppp uint32 entries shared by every product), or None"""
    if index is None:
        return None
    index = list(index)
    if len(index) != ppp:
        raise ValueError("index must name one G2 point per pair of a product (%d entries, got %d)" % (ppp, len(index)))
    return (ctypes.c_uint32 * max(1, ppp))(*index)


def g2_prepared_run(lib, handle, gtsz: int, fused: bool, g1: bytes, index, ppp: int, n: int) -> bytes:
    """mlhip_miller_loop_prepared (fused = False) / mlhip_pairing_prepared (True) on the handle `handle` of `lib`: n Gt
    values (bytes) for n products of ppp pairs; g1 holds the n * ppp affine G1 points"""
    out = ctypes.create_string_buffer(max(1, n * gtsz))
    fn = lib.mlhip_pairing_prepared if fused else lib.mlhip_miller_loop_prepared
    check(fn(handle, g1, q_index_array(index, ppp), ppp, n, out))
    return out.raw[: n * gtsz]


def product_pairs(m: int) -> int:
    """MLHIP_PRODUCT_PAIRS of include/mlhip.h: a product length in the pairs_per_product / ppp argument of the six Miller-loop
    entry points (bit 63 set, m in the low 32 bits; m = 0 or m >= 2^32 packs to a value they all reject)"""
    return (1 << 63) | (m if 1 <= m <= 0xFFFFFFFF else 0)


def mlhip_miller_loop_products(lib, curve: int, g1, g2, m: int, n_products: int, out) -> int:
    """include/mlhip_products.h: n_products Miller-loop products of m pairs each, any m (the return code, as the C function)"""
    return lib.mlhip_miller_loop(curve, g1, g2, product_pairs(m), n_products, out)


def mlhip_miller_loop_products_device(lib, curve: int, d_g1, d_g2, m: int, n_products: int, d_out, stream) -> int:
    """include/mlhip_products.h: the same on device pointers, in order on `stream`"""
    return lib.mlhip_miller_loop_device(curve, d_g1, d_g2, product_pairs(m), n_products, d_out, stream)


def mlhip_miller_loop_prepared_products(lib, handle, g1, q_index, m: int, n_products: int, out) -> int:
    """include/mlhip_products.h: products of m pairs against the handle's points (q_index: m host entries, or None)"""
    return lib.mlhip_miller_loop_prepared(handle, g1, q_index, product_pairs(m), n_products, out)


def mlhip_miller_loop_prepared_products_device(lib, handle, d_g1, q_index, m: int, n_products: int, d_out, stream) -> int:
    """include/mlhip_products.h: the same on device pointers, in order on `stream`"""
    return lib.mlhip_miller_loop_prepared_device(handle, d_g1, q_index, product_pairs(m), n_products, d_out, stream)


def mlhip_pairing_prepared_products(lib, handle, g1, q_index, m: int, n_products: int, out) -> int:
    """include/mlhip_products.h: FExp of the same products"""
    return lib.mlhip_pairing_prepared(handle, g1, q_index, product_pairs(m), n_products, out)


def mlhip_pairing_prepared_products_device(lib, handle, d_g1, q_index, m: int, n_products: int, d_out, stream) -> int:
    """include/mlhip_products.h: the same on device pointers, in order on `stream`"""
    return lib.mlhip_pairing_prepared_device(handle, d_g1, q_index, product_pairs(m), n_products, d_out, stream)


def miller_loop_products(curve: int, g1: bytes, g2: bytes, m: int, n_products: int) -> bytes:
    """mlhip_miller_loop_products over host buffers: n_products raw Miller values (bytes)"""
    gtsz = sizes(curve)[3]
    out = ctypes.create_string_buffer(max(1, n_products * gtsz))
    check(mlhip_miller_loop_products(load(), curve, g1, g2, m, n_products, out))
    return out.raw[: n_products * gtsz]


def g2_prepared_products(lib, handle, gtsz: int, fused: bool, g1: bytes, index, m: int, n: int) -> bytes:
    """mlhip_miller_loop_prepared_products (fused = False) / mlhip_pairing_prepared_products (True) on the handle `handle`
    of `lib`: n Gt values (bytes) for n products of m pairs; g1 holds the n * m affine G1 points"""
    out = ctypes.create_string_buffer(max(1, n * gtsz))
    fn = mlhip_pairing_prepared_products if fused else mlhip_miller_loop_prepared_products
    check(fn(lib, handle, g1, q_index_array(index, m), m, n, out))
    return out.raw[: n * gtsz]


def init_devices(devices=None) -> None:
    """the process's device list (mlhip_init): None / [] = every visible device"""
    devices = list(devices or [])
    arr = (c_int * max(1, len(devices)))(*devices)
    check(load().mlhip_init(arr, len(devices)))


def get_devices():
    buf = (c_int * 64)()
    k = load().mlhip_get_devices(buf, 64)
    if k < 0:  # MLHIP_DEVICES did not parse
        raise MlhipError(k, load().mlhip_last_error().decode())
    return [buf[i] for i in range(min(k, 64))]


def device_count() -> int:
    n = c_int()
    load().mlhip_device_count(byref(n))
    return n.value


def plan_timings(lib, handle):
    """mlhip_msm_plan_timings as a dict (include/mlhip.h): phase times in ms, tiles, and the two path flags"""
    buf = (c_float * 11)()
    k = lib.mlhip_msm_plan_timings(handle, buf, 11)
    names = ["digits", "sort", "accumulate", "reduce", "device_total", "host_tail", "tiles"]
    t = {names[i]: float(buf[i]) for i in range(min(k, 7))}
    if k >= 9:
        t["window_c"], t["digits_per_scalar"] = int(buf[7]), int(buf[8])
    if k >= 10:
        t["edwards"] = float(buf[9])
    if k >= 11:
        t["tables"] = float(buf[10])
    return t


class MsmPlan:
    """Device workspace for repeated MSMs over device-resident points/scalars (include/mlhip.h)."""

    def __init__(self, curve: int, group: int, max_n: int, window_c: int = 0, scalar_bits: int = 0, device_result: bool = False):
        """scalar_bits != 0: a plan for scalars below 2^scalar_bits (mlhip_msm_plan_create_bits; 0 = full width);
        device_result: the plan leaves its result in device memory (mlhip_msm_plan_create_device_result: run_device /
        finish_device instead of run / finish)"""
        self._h = c_void_p()
        lib = self._lib = concrete()
        self._device_result = bool(device_result)
        if device_result:
            check(mlhip_msm_plan_create_device_result(lib, curve, group, max_n, window_c, scalar_bits, byref(self._h)))
        elif scalar_bits:
            check(mlhip_msm_plan_create_bits(lib, curve, group, max_n, window_c, scalar_bits, byref(self._h)))
        else:
            check(lib.mlhip_msm_plan_create(curve, group, max_n, window_c, byref(self._h)))
        _, g1, g2, _ = sizes(curve)
        self.point_bytes = g1 if group == GROUP_G1 else g2
        self.curve, self.group = curve, group

    def set_profiling(self, on: bool) -> None:
        check(self._lib.mlhip_msm_plan_set_profiling(self._h, 1 if on else 0))

    def assume_srs(self, on: bool) -> None:
        """the points are a fixed SRS: immutable at their address and in the prime-order subgroup (include/mlhip.h)"""
        check(self._lib.mlhip_msm_plan_assume_srs(self._h, 1 if on else 0))

    def timings(self):
        return plan_timings(self._lib, self._h)

    def window(self):
        """(c, W): the window width the plan runs with (the library's pick for window_c = 0) and its number of windows"""
        buf = (c_float * 9)()
        self._lib.mlhip_msm_plan_timings(self._h, buf, 9)
        return int(buf[7]), int(buf[8])

    def scalar_bits(self) -> int:
        """the scalar width the plan was made for (the curve's fr_bits for a full-width plan)"""
        rc, bits = mlhip_msm_plan_scalar_bits(self._lib, self._h)
        check(rc)
        return bits

    def is_device_result(self) -> bool:
        """does the plan leave its result in device memory?  (mlhip_msm_plan_is_device_result)"""
        rc, on = mlhip_msm_plan_is_device_result(self._lib, self._h)
        check(rc)
        return bool(on)

    def run_device(self, d_points: int, d_scalars: int, n: int, scalars_mont: bool, stream: int, d_out: int, d_out_xyzz: int = 0) -> None:
        """mlhip_msm_run_device: the affine result at the device pointer d_out (the XYZZ value at d_out_xyzz unless 0), in
        order on `stream`; returns once everything is queued"""
        check(mlhip_msm_run_device(self._lib, self._h, c_void_p(d_points), c_void_p(d_scalars), 1 if scalars_mont else 0, n,
                                   c_void_p(stream), c_void_p(d_out), c_void_p(d_out_xyzz) if d_out_xyzz else None))

    def finish_device(self, d_out: int, d_out_xyzz: int = 0) -> None:
        """mlhip_msm_finish_device after launch / launch_shared: queues the tail and the delivery, does not wait"""
        check(mlhip_msm_finish_device(self._lib, self._h, c_void_p(d_out), c_void_p(d_out_xyzz) if d_out_xyzz else None))

    def _host_result_only(self, what: str) -> None:
        if self._device_result:
            raise MlhipError(EINVAL, "MsmPlan.%s returns host bytes: a device-result plan has %s_device" % (what, what))

    def run(self, d_points: int, d_scalars: int, n: int, scalars_mont: bool, stream: int = 0, want_xyzz: bool = False):
        self._host_result_only("run")
        out = ctypes.create_string_buffer(self.point_bytes)
        xyzz = ctypes.create_string_buffer(2 * self.point_bytes) if want_xyzz else None
        check(
            self._lib.mlhip_msm_run(
                self._h, c_void_p(d_points), c_void_p(d_scalars), 1 if scalars_mont else 0, n, c_void_p(stream), out, xyzz
            )
        )
        return (out.raw, xyzz.raw) if want_xyzz else out.raw

    def launch(self, d_points: int, d_scalars: int, n: int, scalars_mont: bool, stream: int = 0) -> None:
        check(self._lib.mlhip_msm_launch(self._h, c_void_p(d_points), c_void_p(d_scalars), 1 if scalars_mont else 0, n, c_void_p(stream)))

    def launch_shared(self, g2_plan: "MsmPlan", d_points_g1: int, d_points_g2: int, d_scalars: int, n: int, scalars_mont: bool,
                      stream: int = 0) -> None:
        """self = the G1 plan: the G1 and the G2 MSM of one scalar vector, sorted once (finish both plans afterwards)"""
        check(self._lib.mlhip_msm_launch_shared(self._h, g2_plan._h, c_void_p(d_points_g1), c_void_p(d_points_g2), c_void_p(d_scalars),
                                             1 if scalars_mont else 0, n, c_void_p(stream)))

    def finish(self, want_xyzz: bool = False):
        self._host_result_only("finish")
        out = ctypes.create_string_buffer(self.point_bytes)
        xyzz = ctypes.create_string_buffer(2 * self.point_bytes) if want_xyzz else None
        check(self._lib.mlhip_msm_finish(self._h, out, xyzz))
        return (out.raw, xyzz.raw) if want_xyzz else out.raw

    def close(self) -> None:
        if self._h:
            self._lib.mlhip_msm_plan_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
