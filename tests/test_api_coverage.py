"""Every function include/mlhip.h exports is called by name somewhere in the suite: a GPU test in tests/test_*.py or the C++
mirror's test programs in tests/cpp.  The list comes from the header itself, so the next exported function cannot ship
without a test that calls it."""
import glob
import os
import re

from conftest import ROOT


def exported_names():
    with open(os.path.join(ROOT, "include", "mlhip.h")) as f:
        text = f.read()
    # MLHIP_API <return type> <name>(  -- the return type may be a pointer (mlhip_msm_plan* mlhip_bases_plan(...))
    return re.findall(r"^MLHIP_API\b[^(;]*?\b(mlhip_\w+)\s*\(", text, flags=re.M)


def test_header_declares_the_abi():
    names = exported_names()
    assert len(names) == len(set(names)) and len(names) >= 50, names
    assert "mlhip_version" in names and "mlhip_pairing_product" in names and "mlhip_bases_plan" in names


def test_every_exported_function_is_called_by_a_test():
    me = os.path.abspath(__file__)
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py")) + glob.glob(os.path.join(ROOT, "tests", "cpp", "*.cpp")))
    corpus = ""
    for path in files:
        if os.path.abspath(path) != me:
            with open(path) as f:
                corpus += f.read() + "\n"
    # a call: the name right after a non-identifier character (`lib.<name>(`, ` <name>(`), then an opening parenthesis
    missing = [name for name in exported_names() if not re.search(r"(?<![\w])" + re.escape(name) + r"\(", corpus)]
    assert not missing, "exported by include/mlhip.h but called by no test: %s" % ", ".join(missing)
