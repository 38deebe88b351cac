"""The environment switches of the library (csrc/switches.hpp): one table, parsed by the rule each switch has always had,
sampled at set-up (sector handle, communicator) or where a loop is prepared, never cached per process.  tests/host_switches.cpp
exposes the table and the three snapshots; the expected values below are literals taken from the readers the table
replaced, not from the table.  No GPU."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edipack_amd", "csrc")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_switches") / "host_switches.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           "-I", CSRC, "-o", so, os.path.join(ROOT, "tests", "host_switches.cpp"),
                           os.path.join(CSRC, "switches.cpp")])
    lib = C.CDLL(so)
    lib.sw_name.restype = lib.sw_what.restype = C.c_char_p
    lib.sw_default.restype = lib.sw_lo.restype = lib.sw_hi.restype = lib.sw_ib_min_row_bytes.restype = C.c_longlong
    lib.sw_get.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_double)]
    return lib


def _names(lib):
    return [lib.sw_name(i).decode() for i in range(lib.sw_count())]


def _get(lib, name, slot=0):
    """value of a switch in a fresh set of snapshots; None: the switch has no value (unset, derived default)"""
    lib.sw_take_setup(slot), lib.sw_take_comm(slot), lib.sw_take_loop(slot)
    v = C.c_double(0.0)
    rc = lib.sw_get(slot, name.encode(), C.byref(v))
    assert rc >= 0, name
    return v.value if rc else None


def _clean(lib, monkeypatch):
    for n in _names(lib):
        monkeypatch.delenv(n, raising=False)


# switch, then the value for: unset, "", "0", "1", and a few more texts
ON_OFF = [
    ("EDIGPU_LANCZOS_UNFUSED", 0, 1, 1, 1, {"abc": 1}),           # present
    ("EDIGPU_FORCE_COLLECTIVES", 0, 1, 1, 1, {}),
    ("EDIGPU_LANCZOS_EXACTBETA", 0, 1, 1, 1, {}),
    ("EDIGPU_SHARD_GENERIC", 0, 1, 1, 1, {}),
    ("EDIGPU_NORMAL_EXPLICIT", 0, 0, 0, 1, {"2": 0, "10": 1}),    # first character is 1
    ("EDIGPU_FLAT_HOSTBUILD", 0, 0, 0, 1, {"01": 0}),
    ("EDIGPU_IB_PAIRS", 0, 0, 0, 1, {}),
    ("EDIGPU_BLOCKED", 1, 0, 0, 1, {"abc": 0, "2": 1}),           # on unless atoi gives 0
    ("EDIGPU_ELL16", 1, 0, 0, 1, {}),
    ("EDIGPU_SB", 1, 0, 0, 1, {}),
    ("EDIGPU_IB", 1, 0, 0, 1, {}),
    ("EDIGPU_HANDOVER_FACTOR", 1, 0, 0, 1, {}),
    ("EDIGPU_SHARD_PANEL_LOOP", 1, 0, 0, 1, {}),
    ("EDIGPU_POSROWS", 0, 0, 0, 1, {"2": 1, "abc": 0}),           # off unless atoi gives non-zero
    ("EDIGPU_TILE_PERSIST", 0, 0, 0, 1, {}),
    ("EDIGPU_SB_SPLIT", 0, 0, 0, 1, {}),
    ("EDIGPU_SB_AMODE", 0, 0, 0, 1, {"2": 1}),
    ("EDIGPU_LANCZOS_GRAPH", 0, 0, 0, 1, {}),
]


@pytest.mark.parametrize("name,unset,empty,zero,one,more", ON_OFF, ids=[c[0] for c in ON_OFF])
def test_on_off_rules(shim, monkeypatch, name, unset, empty, zero, one, more):
    _clean(shim, monkeypatch)
    assert _get(shim, name) == unset
    for text, want in [("", empty), ("0", zero), ("1", one)] + list(more.items()):
        monkeypatch.setenv(name, text)
        assert _get(shim, name) == want, (name, text)


NUMBERS = [
    ("EDIGPU_IB_ROWS", 480, {"2": 4, "9999": 480, "24": 24}),
    ("EDIGPU_IB_MIN", 1 << 21, {"0": 0}),
    ("EDIGPU_BLOCKED_MIN", 1 << 21, {"0": 0}),
    ("EDIGPU_PANEL_VEC2_MIN", 1 << 21, {"1": 1}),
    ("EDIGPU_LANCZOS_GRAPH_MAX", 1 << 21, {"5000000000": 5000000000}),
    ("EDIGPU_TILE_ROWS", 32, {"4": 8, "100": 64, "16": 16}),
    ("EDIGPU_IB_NSUB", 1, {"0": 1, "2": 2, "99": 8}),
    ("EDIGPU_IB_PSPAD", 0, {"-3": 0, "16": 16}),
    ("EDIGPU_BLOCKED_LDS_KB", 32, {"4": 4}),
    ("EDIGPU_DIRECT_WGS", 2, {"4": 4}),
    ("EDIGPU_SB_STEP", 1, {"0": 0, "2": 2}),
    ("EDIGPU_IB_NT", 0, {"512": 512}),
    ("EDIGPU_ROWS_TD", None, {"4": 4, "0": 0}),          # no value when unset: the reader derives the default
    ("EDIGPU_ROW_SPLIT", None, {"0": 0, "2": 2}),
    ("EDIGPU_IB_SPLIT", None, {"0": 0, "1": 1}),
    ("EDIGPU_IB_COLS2", None, {"0": 0, "1": 1}),
    ("EDIGPU_PANEL_W", None, {"32": 32}),
    ("EDIGPU_PANEL_BPP", None, {"64": 64}),
    ("EDIGPU_TRL_THR", None, {"1e-5": 1e-5}),
]


@pytest.mark.parametrize("name,unset,given", NUMBERS, ids=[c[0] for c in NUMBERS])
def test_number_rules(shim, monkeypatch, name, unset, given):
    _clean(shim, monkeypatch)
    assert _get(shim, name) == unset
    for text, want in given.items():
        monkeypatch.setenv(name, text)
        assert _get(shim, name) == want, (name, text)


def test_derived_values(shim, monkeypatch):
    _clean(shim, monkeypatch)
    shim.sw_take_setup(0)
    assert shim.sw_ib_min_row_bytes(0) == 40960 and shim.sw_blocked_shift(0) == 7 and shim.sw_sb_cols_gs(0) == 8
    monkeypatch.setenv("EDIGPU_IB_MIN", "0")
    shim.sw_take_setup(0)
    assert shim.sw_ib_min_row_bytes(0) == 0
    monkeypatch.setenv("EDIGPU_IB_MINROW", "1000")
    shim.sw_take_setup(0)
    assert shim.sw_ib_min_row_bytes(0) == 1000
    for text, shift in [("128", 7), ("64", 6), ("32", 5), ("16", 4), ("48", 0), ("0", 0), ("abc", 0), ("", 0)]:
        monkeypatch.setenv("EDIGPU_BLOCKED_W", text)
        shim.sw_take_setup(0)
        assert shim.sw_blocked_shift(0) == shift, text
    for text, gs in [("1", 4), ("2", 8), ("0", 8)]:
        monkeypatch.setenv("EDIGPU_SB_CW", text)
        shim.sw_take_setup(0)
        assert shim.sw_sb_cols_gs(0) == gs, text


def test_no_process_cache(shim, monkeypatch):
    """two snapshots with the environment changed in between differ: of a handle, of a communicator, of a loop"""
    _clean(shim, monkeypatch)
    for name in ("EDIGPU_TILE_PERSIST", "EDIGPU_FORCE_COLLECTIVES", "EDIGPU_LANCZOS_EXACTBETA"):
        before = _get(shim, name, slot=0)
        monkeypatch.setenv(name, "1")
        after = _get(shim, name, slot=1)
        monkeypatch.delenv(name)
        again = _get(shim, name, slot=0)
        assert (before, after, again) == (0, 1, 0), name
        v = C.c_double(-1.0)
        assert shim.sw_get(1, name.encode(), C.byref(v)) == 1 and v.value == 1     # the earlier snapshot keeps what it saw


def test_only_the_table_reads_the_environment():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path) and os.path.basename(path) != "switches.cpp":
            with open(path, errors="replace") as f:
                assert "getenv" not in f.read(), path


# read by the Python side or macros of the header, not switches of the library
NOT_LIBRARY = ("EDIGPU_LIB", "EDIGPU_DIST_BACKEND", "EDIGPU_EXCHANGE", "EDIGPU_FORCE_MULTI")


def test_every_switch_the_tests_use_is_in_the_table(shim):
    table = set(_names(shim))
    assert len(table) == shim.sw_count()                   # one row per switch
    used = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")) + [os.path.join(ROOT, "scripts", "check_switches.sh")]:
        with open(path) as f:
            used |= set(re.findall(r"EDIGPU_[A-Z0-9_]+", f.read()))
    used = {n for n in used if n not in NOT_LIBRARY and not n.startswith("EDIGPU_MAX")}
    assert used <= table, sorted(used - table)


def test_every_switch_is_documented(shim):
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    start = re.search(r"^## [0-9. ]*Environment switches$", text, re.M).end()
    nxt = re.search(r"^## ", text[start:], re.M)
    section = text[start:start + nxt.start()] if nxt else text[start:]
    for i in range(shim.sw_count()):
        name = shim.sw_name(i).decode()
        line = next((l for l in section.splitlines() if "`%s`" % name in l), None)
        assert line is not None, name
        assert ("set-up", "communicator", "loop")[shim.sw_moment(i)] in line, name
