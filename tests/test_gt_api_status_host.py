"""The statuses of the pairing and Gt entry points (mathlib_amd/csrc/api_pairing.hip) without a GPU: unknown curve id, n = 0,
every pointer null in turn, and a valid call, through the host and the _device forms.  What is recorded is the status and
what mlhip_last_error() names -- the curve, the pointer or the device -- because the ORDER of the checks is behaviour: the
older _device forms look for a device first and check no pointers, the newer ones check their arguments first.

EXPECTED was taken on a machine without a device from the library as it was before the host wrappers were unified
(`python tests/test_gt_api_status_host.py` prints the table of the library it loads).  On a machine with a device only the
rows that return before any device is looked for are called: the others would run kernels on the stand-in host buffers."""
import ctypes

C, N, P, H = "curve", "n", "pointer", "handle"  # H: a prepared-G2 handle, always null here (none can be made without a device)

# name -> argument pattern; integers stand for themselves, None is the null stream
ENTRY_POINTS = {
    "mlhip_miller_loop": (C, P, P, 1, N, P),
    "mlhip_final_exp": (C, P, N, P),
    "mlhip_pairing_batch": (C, P, P, N, P),
    "mlhip_miller_loop_device": (C, P, P, 1, N, P, None),
    "mlhip_final_exp_device": (C, P, N, P, None),
    "mlhip_pairing_batch_device": (C, P, P, N, P, None),
    "mlhip_pairing_product": (C, P, P, N, P),
    "mlhip_gt_mul": (C, P, P, N, P),
    "mlhip_gt_mul_device": (C, P, P, N, P, None),
    "mlhip_gt_exp": (C, P, P, 0, N, P),
    "mlhip_gt_exp_device": (C, P, P, 0, N, P, None),
    "mlhip_gt_exp_cyclo": (C, P, P, 0, N, P),
    "mlhip_gt_exp_cyclo_device": (C, P, P, 0, N, P, None),
    "mlhip_gt_from_bytes": (C, P, N, 1, P, P),
    "mlhip_gt_from_bytes_device": (C, P, N, 1, P, P, None),
    "mlhip_gt_to_bytes": (C, P, N, P),
    "mlhip_gt_to_bytes_device": (C, P, N, P, None),
    "mlhip_gt_is_member": (C, P, N, P),
    "mlhip_gt_is_member_device": (C, P, N, P, None),
    "mlhip_gt_inverse": (C, P, N, P),
    "mlhip_gt_inverse_device": (C, P, N, P, None),
    "mlhip_fp_mul_device": (C, P, P, N, 1, P, None),
    "mlhip_g2_prepared_create": (C, P, N, P),
    "mlhip_g2_prepared_create_device": (C, P, N, P),
    "mlhip_g2_prepared_count": (H, P),
    "mlhip_miller_loop_prepared": (H, P, None, 1, N, P),
    "mlhip_miller_loop_prepared_device": (H, P, None, 1, N, P, None),
    "mlhip_pairing_prepared": (H, P, None, 1, N, P),
    "mlhip_pairing_prepared_device": (H, P, None, 1, N, P, None),
}

# fmt: off
EXPECTED = {
    "mlhip_miller_loop": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg2": [-1, "pointer"], "null_arg5": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_final_exp": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg3": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_pairing_batch": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg2": [-1, "pointer"], "null_arg4": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_miller_loop_device": {"unknown_curve": [-2, "device"], "n0": [-2, "device"], "null_arg1": [-2, "device"], "null_arg2": [-2, "device"], "null_arg5": [-2, "device"], "valid": [-2, "device"]},
    "mlhip_final_exp_device": {"unknown_curve": [-2, "device"], "n0": [-2, "device"], "null_arg1": [-2, "device"], "null_arg3": [-2, "device"], "valid": [-2, "device"]},
    "mlhip_pairing_batch_device": {"unknown_curve": [-2, "device"], "n0": [-2, "device"], "null_arg1": [-2, "device"], "null_arg2": [-2, "device"], "null_arg4": [-2, "device"], "valid": [-2, "device"]},
    "mlhip_pairing_product": {"unknown_curve": [-1, "curve"], "n0": [-2, "device"], "null_arg1": [-1, "pointer"], "null_arg2": [-1, "pointer"], "null_arg4": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_mul": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg2": [-1, "pointer"], "null_arg4": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_mul_device": {"unknown_curve": [-2, "device"], "n0": [-2, "device"], "null_arg1": [-2, "device"], "null_arg2": [-2, "device"], "null_arg4": [-2, "device"], "valid": [-2, "device"]},
    "mlhip_gt_exp": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg2": [-1, "pointer"], "null_arg5": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_exp_device": {"unknown_curve": [-2, "device"], "n0": [-2, "device"], "null_arg1": [-2, "device"], "null_arg2": [-2, "device"], "null_arg5": [-2, "device"], "valid": [-2, "device"]},
    "mlhip_gt_exp_cyclo": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg2": [-1, "pointer"], "null_arg5": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_exp_cyclo_device": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg2": [-1, "pointer"], "null_arg5": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_from_bytes": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg4": [-1, "pointer"], "null_arg5": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_from_bytes_device": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg4": [-1, "pointer"], "null_arg5": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_to_bytes": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg3": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_to_bytes_device": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg3": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_is_member": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg3": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_is_member_device": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg3": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_inverse": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg3": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_gt_inverse_device": {"unknown_curve": [-1, "curve"], "n0": [0, ""], "null_arg1": [-1, "pointer"], "null_arg3": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_fp_mul_device": {"unknown_curve": [-2, "device"], "n0": [-2, "device"], "null_arg1": [-2, "device"], "null_arg2": [-2, "device"], "null_arg5": [-2, "device"], "valid": [-2, "device"]},
    "mlhip_g2_prepared_create": {"unknown_curve": [-1, "curve"], "n0": [-1, "other"], "null_arg1": [-1, "pointer"], "null_arg3": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_g2_prepared_create_device": {"unknown_curve": [-1, "curve"], "n0": [-1, "other"], "null_arg1": [-1, "pointer"], "null_arg3": [-1, "pointer"], "valid": [-2, "device"]},
    "mlhip_g2_prepared_count": {"unknown_curve": [-1, "handle"], "n0": [-1, "handle"], "null_arg1": [-1, "handle"], "valid": [-1, "handle"]},
    "mlhip_miller_loop_prepared": {"unknown_curve": [-1, "handle"], "n0": [-1, "handle"], "null_arg1": [-1, "handle"], "null_arg5": [-1, "handle"], "valid": [-1, "handle"]},
    "mlhip_miller_loop_prepared_device": {"unknown_curve": [-1, "handle"], "n0": [-1, "handle"], "null_arg1": [-1, "handle"], "null_arg5": [-1, "handle"], "valid": [-1, "handle"]},
    "mlhip_pairing_prepared": {"unknown_curve": [-1, "handle"], "n0": [-1, "handle"], "null_arg1": [-1, "handle"], "null_arg5": [-1, "handle"], "valid": [-1, "handle"]},
    "mlhip_pairing_prepared_device": {"unknown_curve": [-1, "handle"], "n0": [-1, "handle"], "null_arg1": [-1, "handle"], "null_arg5": [-1, "handle"], "valid": [-1, "handle"]},
}
# fmt: on


def cases(pattern):
    """(case name, curve id, n, index of the pointer argument that is null or None)"""
    out = [("unknown_curve", 7, 1, None), ("n0", 1, 0, None)]
    out += [("null_arg%d" % k, 1, 1, k) for k, a in enumerate(pattern) if a == P]
    return out + [("valid", 1, 1, None)]


def names(msg):
    for word, kind in (("curve", "curve"), ("no HIP device", "device"), ("null handle", "handle"), ("null", "pointer")):
        if word in msg:
            return kind
    return "other"


def observe(lib, only=None):
    """{entry point: {case: [status, what the message names]}}; `only(name, case)` = False leaves a call out"""
    table = {}
    for name, pattern in ENTRY_POINTS.items():
        fn = getattr(lib, name)
        for case, curve, n, null in cases(pattern):
            if only and not only(name, case):
                continue
            bufs = [ctypes.create_string_buffer(4096) for _ in pattern]  # larger than any n = 1 argument of any curve
            args = []
            for k, a in enumerate(pattern):
                if a == C:
                    args.append(curve)
                elif a == N:
                    args.append(n)
                elif a == P:
                    args.append(None if k == null else ctypes.cast(bufs[k], fn.argtypes[k]))
                else:
                    args.append(None if a == H else a)
            rc = fn(*args)
            table.setdefault(name, {})[case] = [rc, names(lib.mlhip_last_error().decode()) if rc else ""]
    return table


def test_every_entry_point_is_covered():
    import os
    import re

    from conftest import ROOT

    src = open(os.path.join(ROOT, "mathlib_amd", "csrc", "api_pairing.hip")).read()
    defined = set(re.findall(r"^int (mlhip_\w+)\(", src, re.M)) - {"mlhip_g2_prepared_destroy"}  # (destroy(null) = 0: test_abi)
    assert defined == set(ENTRY_POINTS) == set(EXPECTED)
    for name, pattern in ENTRY_POINTS.items():
        assert [c[0] for c in cases(pattern)] == list(EXPECTED[name]), name


def test_statuses_and_the_order_of_the_checks(mlhip):
    lib = mlhip.load()
    with_device = mlhip.device_count() > 0

    def only(name, case):
        return not (with_device and EXPECTED[name][case][1] == "device")

    got = observe(lib, only)
    want = {name: {case: v for case, v in rows.items() if only(name, case)} for name, rows in EXPECTED.items()}
    assert got == {name: rows for name, rows in want.items() if rows}
    if not with_device:
        # the two orders are both present: argument errors of the older _device forms are hidden behind the missing device
        assert EXPECTED["mlhip_gt_exp_device"]["unknown_curve"][1] == "device"
        assert EXPECTED["mlhip_gt_exp_cyclo_device"]["unknown_curve"][1] == "curve"


if __name__ == "__main__":
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from mathlib_amd import _lib

    print("EXPECTED = {")
    for name, rows in observe(_lib.load()).items():
        print('    "%s": {%s},' % (name, ", ".join('"%s": [%d, "%s"]' % (c, v[0], v[1]) for c, v in rows.items())))
    print("}")
