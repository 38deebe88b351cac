"""CPU tests of the shard plan behind edigpu_imp_rdm_flat_sharded (csrc/host_rdm_flat.cpp rdm_flat_shard_plan and its
emulations, through tests/host_rdm_flat_shard.cpp): which rank owns a slab -- the 2^Norb rows of one bath word down -- that
a rank boundary cuts, the halo every rank sends, the buffer the owner fills, the two work lists; and the error paths that
need no device.

The ranks' ranges are those of edigpu_shard_plan over the elements: q = ceil(dim / world) per rank, rank r starts at
min(r q, dim).  The plans are asked for the uncut range (r q, q), so the cut to the sector is part of what is tested.  The
vectors hold integers in -8 .. 8: every product and every sum of the density matrix is then exact in double, whatever the
order, so the sums of the ranks must EQUAL rdm_flat_host_reference of the whole vector."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from edipack_amd import capi
from tests.rdm_flat_cases import MODE, flat_map, flat_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "edipack_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "host_rdm_flat_shard.cpp"), os.path.join(CSRC, "host_rdm_flat.cpp"),
           os.path.join(CSRC, "host_rdm.cpp")]
VP, L, I = C.c_void_p, C.c_int64, C.c_int
MAXSEG = 16

# mode, bath, norb, nbath, sector (Sz / Ntot), seed of make_models -> dim
SECTORS = [
    ("superc", "hybrid", 2, 3, 0, 12),    # 252: slabs [0,21) [21,56) [56,91) [91,126) ...
    ("superc", "hybrid", 2, 3, 3, 12),    # 45: [0,21) spans five ranks of a world of ten
    ("nonsu2", "hybrid", 3, 3, 6, 13),    # 924: blocks of 20, slabs [0,84) [84,210) [210,336) ...
    ("nonsu2", "hybrid", 4, 2, 6, 13),    # 924: blocks of 70, the classes split between workgroups; four slabs
    ("nonsu2", "normal", 2, 2, 4, 13),    # 495: 16 slabs of at most 70
    ("superc", "hybrid", 2, 2, 0, 12),    # 70: [0,15) [15,35) [35,55) [55,70)
]
DIMS = [252, 45, 924, 924, 495, 70]
WORLDS = [1, 2, 3, 5, 10]
IDS = [f"{s[0]}-{s[1]}{s[2]}x{s[3]}-{s[4]}" for s in SECTORS]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_rdm_flat_shard") / "host_rdm_flat_shard.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", so] + SOURCES)
    lib = C.CDLL(so)
    lib.hfs_plan.argtypes = [VP, L, I, I, I, I, I, I, I, I, L, L, VP, VP, VP, VP, I, VP, C.c_char_p]
    lib.hfs_whole_equals_plan.argtypes = [VP, L, I, I, I, I, I, I, I, C.c_char_p]
    lib.hfs_reference.argtypes = [VP, L, I, I, I, I, I, I, VP, VP, C.c_char_p]
    lib.hfs_world.argtypes = [VP, L, I, I, I, I, I, I, I, I, VP, VP, VP, C.c_char_p]
    lib.hfs_ntri.argtypes = [VP, L, I, I, I, I]
    lib.hfs_ntri.restype = L
    return lib


@pytest.fixture(scope="module")
def maps(built):
    out = {}
    for case, dim in zip(SECTORS, DIMS):
        mode, bath, norb, nbath, sec, seed = case
        pm = flat_model(mode, bath, norb, nbath, seed)
        mp = np.ascontiguousarray(flat_map(pm, sec), np.int32)
        assert mp.size == dim
        out[case] = (mp, pm.ns)
    return out


def slabs_of(mp, ns, norb):
    """[(start, length, Bdw)] of the slabs: the runs of equal bath word down of the ascending sector map"""
    bdw = (mp.astype(np.int64) >> ns) >> norb
    starts = [0] + [i for i in range(1, mp.size) if bdw[i] != bdw[i - 1]]
    assert np.all(np.diff(bdw) >= 0)
    return [(s, e - s, int(bdw[s])) for s, e in zip(starts, starts[1:] + [mp.size])]


def plan(shim, case, mp, ns, nblk, cw, world, first, count, target_wgs=2048, expect=0):
    mode, _, norb, _, sec, _ = case
    info, heads, msg = np.zeros(16, np.int64), np.full(world, -1, np.int64), C.create_string_buffer(256)
    pack, fill = np.zeros((MAXSEG, 5), np.int64), np.zeros((MAXSEG, 5), np.int64)
    in_bdw = np.full(1 << (ns - norb), -1, np.int32)
    rc = shim.hfs_plan(mp.ctypes.data, mp.size, ns, norb, MODE[mode], sec, nblk, cw, target_wgs, world, first, count,
                       info.ctypes.data, heads.ctypes.data, pack.ctypes.data, fill.ctypes.data, MAXSEG, in_bdw.ctypes.data, msg)
    if expect:
        return rc, msg.value.decode()
    assert rc == 0, msg.value.decode()
    keys = "first count rank H q nslab_in tail_start tail_len tail_own tail_bdw nin nslab ngroups partial npack nfill".split()
    p = dict(zip(keys, (int(x) for x in info)))
    p.update(heads=[int(h) for h in heads], pack=pack[:p["npack"]].tolist(), fill=fill[:p["nfill"]].tolist(),
             in_bdw=[int(b) for b in in_bdw[:p["nslab_in"]]])
    return p


def world_plans(shim, case, mp, ns, world):
    q = -(-mp.size // world)
    return [plan(shim, case, mp, ns, 1, 1, world, r * q, q) for r in range(world)], q


def integer_vector(n, cplx, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=n * (2 if cplx else 1)).astype(np.float64)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("case", SECTORS, ids=IDS)
def test_every_slab_has_one_owner_and_every_element_is_read_once(shim, maps, case, world):
    mp, ns = maps[case]
    norb, n = case[2], mp.size
    slabs = slabs_of(mp, ns, norb)
    by_bdw = {b: (s, ln) for s, ln, b in slabs}
    plans, q = world_plans(shim, case, mp, ns, world)
    owner = {s: [] for s, _, _ in slabs}
    reads = np.zeros(n, int)
    H = plans[0]["H"]
    assert 0 <= H < max(ln for _, ln, _ in slabs) and (world > 1 or H == 0)
    for r, p in enumerate(plans):
        first, count = min(r * q, n), max(0, min(q, n - min(r * q, n)))
        assert (p["first"], p["count"], p["q"]) == (first, count, q) and p["rank"] == (r if count else -1)
        assert p["H"] == H and p["heads"] == plans[0]["heads"]                     # the same on every rank
        starts_here = [s for s, _, _ in slabs if first <= s < first + count]
        head = (starts_here[0] - first) if starts_here else count
        assert p["heads"][r] == head
        # the halo this rank sends: its head, then zeros up to H
        want = ([[1, 0, 0, 0, head]] if head else []) + ([[0, 0, 0, head, H - head]] if H > head else [])
        assert p["pack"] == want
        # interior slabs: wholly inside
        for b in p["in_bdw"]:
            s, ln = by_bdw[b]
            assert first <= s and s + ln <= first + count
            owner[s].append(r)
            reads[s:s + ln] += 1
        assert (p["nin"] > 0) == (p["nslab_in"] > 0)
        # the tail slab: starts inside, ends beyond; its elements here, then heads of the following ranks in rank order
        cut = [(s, ln, b) for s, ln, b in slabs if first <= s < first + count < s + ln]
        assert len(cut) <= 1
        if not cut:
            assert p["tail_len"] == 0 and p["tail_start"] == -1 and p["fill"] == [] and p["nslab"] == 0
            continue
        s, ln, b = cut[0]
        assert (first + p["tail_start"], p["tail_len"], p["tail_own"], p["tail_bdw"]) == (s, ln, first + count - s, b)
        assert p["nslab"] >= 1
        owner[s].append(r)
        at, prev = s, r
        for k, (sel, rank, src, dst, ln_k) in enumerate(p["fill"]):
            assert dst == at - s and ln_k > 0
            if k == 0:
                assert (sel, first + src, ln_k) == (1, s, p["tail_own"])
            else:
                assert sel == 2 and rank > prev and src == 0 and ln_k <= plans[0]["heads"][rank]
                assert min(rank * q, n) == at
                prev = rank
            reads[at:at + ln_k] += 1
            at += ln_k
        assert at == s + ln
    assert all(len(o) == 1 for o in owner.values()), owner
    assert np.all(reads == 1)
    assert H == max(plans[0]["heads"])


def test_the_geometry_the_gpu_tests_rely_on(shim, maps):
    """asserted from the sector maps, not trusted from a table"""
    def heads(k, world):
        mp, ns = maps[SECTORS[k]]
        return world_plans(shim, SECTORS[k], mp, ns, world)[0]

    mp, ns = maps[SECTORS[0]]
    assert [(s, s + n) for s, n, _ in slabs_of(mp, ns, 2)[:4]] == [(0, 21), (21, 56), (56, 91), (91, 126)]
    p = heads(0, 2)
    assert p[0]["H"] == 0 and p[0]["tail_len"] == 0 and p[0]["pack"] == []          # no cut: no all-gather
    p = heads(0, 3)
    assert p[0]["heads"] == [0, 7, 28] and p[0]["q"] == 84
    assert (p[0]["tail_start"], p[0]["tail_len"], p[0]["tail_own"]) == (56, 35, 28)  # [56, 91) cut at 84
    assert (84 + p[1]["tail_start"], p[1]["tail_len"], p[1]["tail_own"]) == (161, 35, 7)
    p = heads(0, 5)
    assert p[0]["heads"] == [0, 5, 24, 8, 27] and p[0]["q"] == 51 and sum(x["tail_len"] > 0 for x in p) == 4
    mp, ns = maps[SECTORS[1]]
    assert [(s, s + n) for s, n, _ in slabs_of(mp, ns, 2)[:5]] == [(0, 21), (21, 28), (28, 35), (35, 36), (36, 43)]
    p = heads(1, 10)
    assert p[0]["q"] == 5 and p[0]["heads"][:5] == [0, 5, 5, 5, 1] and p[9]["count"] == 0 and p[9]["rank"] == -1
    assert [f[1] for f in p[0]["fill"]] == [0, 1, 2, 3, 4] and p[0]["tail_own"] == 5
    assert all(p[r]["nslab_in"] == 0 and p[r]["tail_len"] == 0 for r in (1, 2, 3))   # all head: they own nothing
    mp, ns = maps[SECTORS[2]]
    assert [(s, s + n) for s, n, _ in slabs_of(mp, ns, 3)[:3]] == [(0, 84), (84, 210), (210, 336)]
    assert heads(2, 3)[0]["heads"] == [0, 28, 98]
    p = heads(2, 10)
    assert p[0]["q"] == 93 and p[0]["heads"] == [0, 93, 24, 57, 90, 93, 30, 63, 93, 3]
    assert [r for r in range(10) if p[r]["nslab_in"] == 0 and p[r]["tail_len"] == 0] == [1, 5, 8]
    assert sum(len(x["fill"]) == 3 for x in p) == 3                                   # three slabs span three ranks each
    mp, ns = maps[SECTORS[3]]
    assert sorted({n for _, n, _ in slabs_of(mp, ns, 4)}) == [210, 252] and len(slabs_of(mp, ns, 4)) == 4
    assert heads(3, 3)[0]["heads"] == [0, 154, 98]
    mp, ns = maps[SECTORS[4]]
    sl = slabs_of(mp, ns, 2)
    assert len(sl) == 16 and max(n for _, n, _ in sl) <= 70
    p = heads(4, 2)
    assert p[0]["q"] == 248 and p[0]["heads"] == [0, 18] and (p[0]["tail_start"], p[0]["tail_len"]) == (210, 56)
    assert heads(4, 3)[0]["heads"] == [0, 17, 0]
    mp, ns = maps[SECTORS[5]]
    assert [(s, s + n) for s, n, _ in slabs_of(mp, ns, 2)] == [(0, 15), (15, 35), (35, 55), (55, 70)]
    assert heads(5, 3)[0]["heads"] == [0, 11, 7] and heads(5, 3)[0]["q"] == 24


@pytest.mark.parametrize("cw", [1, 2])
@pytest.mark.parametrize("nblk", [1, 4])
@pytest.mark.parametrize("case", SECTORS, ids=IDS)
def test_the_ranks_sums_equal_the_reference_exactly(shim, maps, case, nblk, cw):
    mp, ns = maps[case]
    mode, _, norb, _, sec, _ = case
    geo = (mp.ctypes.data, mp.size, ns, norb, MODE[mode], sec)
    v = integer_vector(nblk * mp.size, cw == 2, seed=mp.size + nblk)
    ntri = shim.hfs_ntri(*geo)
    assert ntri > 0
    ref, msg = np.full(ntri * cw, np.nan), C.create_string_buffer(256)
    assert shim.hfs_reference(*geo, nblk, cw, v.ctypes.data, ref.ctypes.data, msg) == 0, msg.value.decode()
    assert np.any(ref != 0.0)
    for wgs in (2048, 3):                                       # two device widths
        # a world of one: the shard plan IS the plan of the whole sector, field by field
        assert shim.hfs_whole_equals_plan(*geo, nblk, cw, wgs, msg) == 0, msg.value.decode()
        for world in WORLDS:
            tri, H = np.full(ntri * cw, np.nan), np.full(1, -1, np.int64)
            rc = shim.hfs_world(*geo, nblk, cw, wgs, world, v.ctypes.data, tri.ctypes.data, H.ctypes.data, msg)
            assert rc == 0, (world, wgs, msg.value.decode())    # no index violation in any emulation
            assert H[0] >= 0 and (world > 1 or H[0] == 0)
            assert np.array_equal(tri, ref), (world, wgs)


def test_ranges_that_are_no_ranks_range_are_refused(shim, maps):
    mp, ns = maps[SECTORS[0]]
    for first, count in ((1, 126), (0, 125), (126, 100), (84, 84)):
        rc, msg = plan(shim, SECTORS[0], mp, ns, 1, 1, 2, first, count, expect=1)
        assert rc == 1 and "not a rank's range" in msg
    assert plan(shim, SECTORS[0], mp, ns, 1, 1, 2, 126, 126)["rank"] == 1


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """host code only: the emulated worlds with their own main, built with -fsanitize=address,undefined and run as a program"""
    exe = str(tmp_path / "host_rdm_flat_shard_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DHFS_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", CSRC, "-o", exe] + SOURCES)
    args = []
    for mode, bath, norb, nbath, sec, seed in SECTORS:
        args += [flat_model(mode, bath, norb, nbath, seed).ns, norb, MODE[mode], sec]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.count("ok ") == len(SECTORS) and "0 failures" in out.stdout and "FAIL" not in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_null_arguments_are_refused_with_a_message(built):
    lib = capi.lib()
    w, buf = np.zeros(5), np.zeros(256)
    info = np.zeros(6, np.int64)
    assert lib.edigpu_imp_rdm_flat_sharded(None, None, None, 1, capi.pd(buf), capi.pd(w)) != 0
    assert "edigpu_imp_rdm_flat_sharded" in capi.last_error() and "NULL" in capi.last_error()
    # nvec is looked at before the handle and the communicator are touched: any non-NULL address stands in for them
    fake = C.c_void_p(buf.ctypes.data)
    for nvec in (0, -3):
        assert lib.edigpu_imp_rdm_flat_sharded(fake, fake, None, nvec, capi.pd(buf), capi.pd(w)) != 0
        assert capi.last_error() == "edigpu_imp_rdm_flat_sharded: nvec must be positive"
    assert lib.edigpu_imp_rdm_flat_sharded(fake, fake, None, 1, None, capi.pd(w)) != 0
    assert capi.last_error() == "edigpu_imp_rdm_flat_sharded: NULL argument"
    pinfo = info.ctypes.data_as(C.POINTER(C.c_int64))
    for h, c, out in ((None, fake, pinfo), (fake, None, pinfo), (fake, fake, None)):
        assert lib.edigpu_imp_rdm_flat_sharded_info(h, c, out) != 0
        assert capi.last_error() == "edigpu_imp_rdm_flat_sharded_info: NULL argument"
