"""The library's run-time switches (csrc/mk_switch.h): one table, one parser, one place that reads the environment.  No GPU."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pykrylov_amd", "csrc")
LABELS = ["unset", "empty", "abc", "12abc", "7comma", "7comma_blank", "minus5", "digits40", "commas4k"]

# What the sites did with "12abc", "7," / "7, " and "-5" before the table existed (atoi / atoll and each site's own clamp); every
# other value of the list has no leading number a long holds and gives (not set, default).  MK_PENCIL_MIN_ROWS had no clamp: a
# threshold of -5 rows and one of 0 rows admit the same matrices.
SITES = {
    "MK_CG_FUSE": (1, 12, 7, -5), "MK_CG_XDEFER": (0, 12, 7, 1), "MK_ILU_FUSE_ROWS": (256, 12, 7, 0),
    "MK_SPMV_FORMAT": (11, 11, 7, 0), "MK_SPMV_NT": (0, 12, 7, -5), "MK_PENCIL_MIN_ROWS": (1 << 21, 12, 7, 0),
    "MK_PEN_GEN": (0, 12, 7, -5), "MK_RT_PHASES": (0, 12, 7, 0), "MK_COLBLOCK_KB": (0, 12, 7, 0),
    "MK_GRID_STREAM": (512, 12, 7, 1), "MK_GRID_SPMV": (1024, 12, 7, 1), "MK_COPY_THREADS": (4, 8, 7, 0),
}
FLAGS = {"MK_DEBUG_PLAN"}                                     # set by mere presence, whatever the value


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path_factory.mktemp("switch") / "switch_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "switch_main.cpp"), "-o", exe], check=True, timeout=120)
    return exe


def header_table(program):
    rows = [l.split() for l in subprocess.run([program, "--table"], capture_output=True, text=True, check=True, timeout=5).stdout.splitlines()]
    return {r[0]: r[1:] for r in rows}


def readme_table():
    """rows of README's switch table: name -> 'library' or 'Python' (the column that says who reads the variable)"""
    out = {}
    for line in open(os.path.join(ROOT, "README.md"), encoding="utf-8"):
        m = re.match(r"\|\s*`((?:MK|MIKRYLOV)_[A-Z0-9_]+)`\s*\|\s*(library|Python)\s*\|", line)
        if m:
            out[m.group(1)] = m.group(2)
    return out


def test_getenv_only_in_the_switch_header():
    hits = [os.path.basename(f) for f in sorted(glob.glob(os.path.join(CSRC, "*"))) if "getenv(" in open(f, encoding="utf-8").read()]
    assert hits == ["mk_switch.h"], hits


def test_header_and_readme_list_the_same_switches(program):
    readme = readme_table()
    assert {k for k, v in readme.items() if v == "library"} == set(header_table(program)) == set(SITES) | FLAGS
    py = "".join(open(f, encoding="utf-8").read() for f in glob.glob(os.path.join(ROOT, "pykrylov_amd", "**", "*.py"), recursive=True)
                 + [os.path.join(ROOT, "tests", "conftest.py")])
    for name in (k for k, v in readme.items() if v == "Python"):
        assert re.search("['\"]%s['\"]" % name, py), name


def test_every_switch_that_tests_and_tools_set_is_listed():
    pats = [r'(?:setenv|delenv)\(\s*"(MK_[A-Z0-9_]+)"', r'environ\[\s*"(MK_[A-Z0-9_]+)"', r'environ\.\w+\(\s*"(MK_[A-Z0-9_]+)"',
            r'\b(MK_[A-Z0-9_]+)=', r'"(MK_[A-Z0-9_]+)"\s*:']
    files = [f for d in ("tests", "tools") for f in glob.glob(os.path.join(ROOT, d, "**", "*"), recursive=True)
             if f.endswith((".py", ".sh")) and os.path.abspath(f) != os.path.abspath(__file__)]
    assert len(files) > 40
    used = {m for f in files for p in pats for m in re.findall(p, open(f, encoding="utf-8").read())}
    assert {"MK_CG_FUSE", "MK_CG_XDEFER", "MK_ILU_FUSE_ROWS", "MK_PEN_GEN", "MK_RT_PHASES", "MK_GRID_SPMV"} <= used
    assert used <= set(readme_table()), sorted(used - set(readme_table()))


def test_parser_on_hostile_values(program):
    """Every kind of switch on: unset, empty, abc, 12abc, '7,', '7, ', -5, a 40-digit number and 4 KiB of commas -- under a time
    limit (the parser this replaces did not come back from 'abc')."""
    p = subprocess.run([program], capture_output=True, text=True, timeout=5)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    got = {(l.split()[0], l.split()[1]): (int(l.split()[2]), int(l.split()[3])) for l in lines if not l.startswith(("read", "flag"))}
    want = {}
    for name, (dflt, v12, v7, vneg) in SITES.items():
        for label in LABELS:
            want[(name, label)] = (0, dflt)
        want[(name, "12abc")], want[(name, "7comma")], want[(name, "7comma_blank")], want[(name, "minus5")] = (1, v12), (1, v7), (1, v7), (1, vneg)
    for name in FLAGS:
        for label in LABELS:
            want[(name, label)] = (0, 0) if label == "unset" else (1, 1)
    assert got == want, sorted(set(got.items()) ^ set(want.items()))
    # read time: MK_CG_FUSE at every query, MK_SPMV_FORMAT once per process; a flag is set by an empty value too
    assert lines[-3:] == ["read MK_CG_FUSE 0 MK_SPMV_FORMAT 3", "read MK_CG_FUSE 1 MK_SPMV_FORMAT 3", "flag MK_DEBUG_PLAN 0 1"]
    table = header_table(program)
    assert {k for k, r in table.items() if r[4] == "0"} == {"MK_CG_FUSE", "MK_CG_XDEFER", "MK_ILU_FUSE_ROWS", "MK_COPY_THREADS", "MK_DEBUG_PLAN"}
