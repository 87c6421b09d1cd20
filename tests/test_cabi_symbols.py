"""The C-ABI library loads, exports every symbol include/umpr_hip.h declares, and the ctypes signature table in
umpr_amd/_lib.py agrees with the header (no compute calls: runs without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_header():
    txt = open(os.path.join(ROOT, "include", "umpr_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    protos = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(umpr_\w+)\s*\(([^;{]*?)\)\s*;", txt):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3)
        codes = ""
        if args.strip() not in ("", "void"):
            for a in args.split(","):
                a = a.strip()
                if "*" in a or "umpr_block_callback" in a:      # pointers, incl. the function-pointer typedef
                    codes += "p"
                elif "size_t" in a:
                    codes += "z"
                elif "uint64_t" in a:
                    codes += "u"
                elif re.search(r"\blong\b", a):
                    codes += "l"
                elif re.search(r"\bdouble\b", a):
                    codes += "d"
                elif re.search(r"\bfloat\b", a):
                    codes += "f"
                elif re.search(r"\bint\b", a):
                    codes += "i"
                else:
                    raise AssertionError(f"unparsed argument {a!r} of {name}")
        rc = "s" if "char" in ret else ("z" if "size_t" in ret else ("p" if "void*" in ret.replace(" ", "") else
                                                                       ("l" if re.search(r"\blong\b", ret) else "i")))
        protos[name] = (codes, rc)
    return protos


def test_signature_table_matches_header():
    from umpr_amd._lib import SIGNATURES
    protos = parse_header()
    assert len(protos) >= 35
    assert set(protos) == set(SIGNATURES), set(protos) ^ set(SIGNATURES)
    for name, sig in protos.items():
        assert SIGNATURES[name] == sig, (name, SIGNATURES[name], sig)


def test_library_exports_every_declared_symbol():
    path = os.path.join(ROOT, "umpr_amd", "libumpr_hip.so")
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build()
    cdll = ctypes.CDLL(path)
    for name in parse_header():
        assert hasattr(cdll, name), f"{name} declared in include/umpr_hip.h but not exported"
    cdll.umpr_version.restype = ctypes.c_char_p
    assert b"gfx950" in cdll.umpr_version()


def test_every_environment_switch_is_in_the_built_library():
    """Each switch the sources read (umpr_env_on / umpr_env_int / getenv) must appear as a string in libumpr_hip.so.
    Regression guard: hipcc once gave two namespace-scope lambdas that differed only in the getenv literal the same closure
    symbol, and UMPR_WGRAD_STREAM silently read UMPR_FC_SMALL."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    blob = open(os.path.join(root, "umpr_amd", "libumpr_hip.so"), "rb").read()
    names = set()
    for f in glob.glob(os.path.join(root, "umpr_amd", "csrc", "*.hip")) + glob.glob(os.path.join(root, "umpr_amd", "csrc", "*.h")):
        names |= set(re.findall(r'(?:getenv|umpr_env_on|umpr_env_int)\("([A-Z0-9_]+)"', open(f).read()))
    assert len(names) >= 15, names
    missing = sorted(n for n in names if n.encode() + b"\x00" not in blob)
    assert not missing, missing


def test_build_checks_scratch_and_dropped_compiler_requests(tmp_path):
    """`make check-scratch` (no kernel spills to the private segment) and `make check-passes` (hipcc dropped no occupancy target
    and no unroll request: -Wpass-failed) on the nine HIP sources.  Both recompile every file for gfx950 (~1 min each, run side by
    side); hipcc cross-compiles without a GPU."""
    import shutil
    import subprocess
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "umpr_amd", "csrc")
    procs = [(t, subprocess.Popen(["make", "-C", csrc, t, f"CHECK_DIR={tmp_path}"], stdout=subprocess.PIPE,
                                  stderr=subprocess.STDOUT, text=True))
             for t in ("check-scratch", "check-passes")]
    for target, p in procs:
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, (target, out[-3000:])
    assert True
