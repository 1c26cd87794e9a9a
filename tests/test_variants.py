"""Storage formats and kernel variants of the product kernel (csrc/mk_variant.h): one table says which variant a launch takes,
its workgroups per CU and its dynamic LDS.  No GPU."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pykrylov_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("variant") / "variant_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "variant_main.cpp"), "-o", exe], check=True, timeout=120)
    return exe


def test_header_agrees_with_the_rules_it_replaced(program):
    """Variant, LDS bytes, workgroups per CU, compiled-or-not, launch bounds and the start of the x windows: the header against the
    if-chain, the ternaries and the two grid formulas of the launcher before the table, restated in variant_main.cpp, over every
    storage format, launch flag, epilogue class and a spread of sizes."""
    p = subprocess.run([program], capture_output=True, text=True, timeout=20)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr
    m = re.fullmatch(r"cases (\d+) mismatches 0", p.stdout.splitlines()[-1])
    assert m and int(m.group(1)) > 100000, p.stdout[-400:]


def test_no_bare_format_number_outside_the_variant_header():
    pat = re.compile(r"\b(?:\w+(?:\.|->))*(?:fmt|FMT|want_fmt)\s*(?:==|!=|<=|>=|<|>)\s*\d")
    hits = []
    for f in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.basename(f) == "mk_variant.h":
            continue
        for n, line in enumerate(open(f, encoding="utf-8"), 1):
            code = line.split("//")[0]
            if pat.search(code):
                hits.append("%s:%d: %s" % (os.path.basename(f), n, line.strip()))
    assert not hits, "\n".join(hits)


def test_design_table_matches_the_header(program):
    """DESIGN.md 3.1 lists every kernel variant with its storage format and workgroups per CU as the header has them."""
    rows = [[int(x) for x in l.split()] for l in subprocess.run([program, "--table"], capture_output=True, text=True, check=True, timeout=5).stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(17))
    doc = {}
    for line in open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8"):
        m = re.match(r"\|\s*(\d+)(?:, (\d+))?\s*\|[^|]*\|\s*(\d+) `MK_FMT_\w+`\s*\|\s*(\d+)\s*\|", line)
        if m:
            doc[int(m.group(3))] = ([int(m.group(1))] + ([int(m.group(2))] if m.group(2) else []), int(m.group(4)))
    assert sorted(doc) == list(range(17)), sorted(doc)
    for k, storage, min_blocks, *_ in rows:
        assert storage in doc[k][0] and min_blocks == doc[k][1], (k, storage, min_blocks, doc[k])
