"""CPU tests of the seeds on shards (csrc/shard_src.hpp, csrc/edigpu_shard_seeds.hip): where a source row lives in the
all-gathered shards, against a numpy construction of the concatenated padded chunks, and a host emulation of the window +
source form of the three kernel families (tests/host_shard_seeds.hpp) on integer-valued vectors, whose stitched shards
must EQUAL the whole-sector restatements of tests/axisop_cases.py / tests/pairs_cases.py.  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.axisop_cases import comb_words, forward_table, real_chain, signed_gather

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, L, I = C.c_void_p, C.c_int64, C.c_int
WORLDS = (1, 2, 3, 5, 10)
POISON = 1.0e300       # what the padding of a gathered vector holds: reading it cannot go unnoticed


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_shard_seeds") / "host_shard_seeds.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-o", so,
                           os.path.join(ROOT, "tests", "host_shard_seeds.cpp")])
    lib = C.CDLL(so)
    lib.ss_offset.restype = L
    lib.ss_offset.argtypes = [L, L, L, L, I, L, L]
    lib.ss_axis_window.argtypes = [I, VP, VP, L, L, L, L, L, VP, VP, VP]
    lib.ss_pairs_window.argtypes = [I, VP, VP, C.c_uint32, C.c_uint32, VP, I, L, L, L, L, VP, VP, VP]
    lib.ss_flat_window.argtypes = [L, I, I, C.c_uint32, I, VP, VP, VP, VP, VP, C.c_double, C.c_double, I, VP]
    return lib


def plan(units, world, rank):
    """(first, count, q) of edigpu_shard_plan"""
    q = -(-units // world)
    first = min(rank * q, units)
    return first, max(0, min(q, units - first)), q


def gathered(whole, world, fill):
    """whole [nblk][units][unit_len] -> the ranks' padded chunks one after another: every rank's shard
    [nblk][count][unit_len] at the start of its chunk of q unit_len nblk cells, `fill` in the padding"""
    nblk, units, unit_len = whole.shape
    q = -(-units // world)
    chunk = q * unit_len * nblk
    g = np.full(world * chunk, fill, dtype=whole.dtype)
    for r in range(world):
        first, count, _ = plan(units, world, r)
        g[r * chunk:r * chunk + nblk * count * unit_len] = whole[:, first:first + count, :].reshape(-1)
    return g, np.array([q, units, chunk, unit_len, nblk], dtype=np.int64)


def test_offset_names_the_cell_that_holds_the_row(shim):
    """every (p, g) maps onto the cells that hold it, no two onto the same, none into padding"""
    checked = 0
    for world in WORLDS:
        for units in range(1, 41):
            for nblk in (1, 4):
                for unit_len in (1, 2, 7):
                    ids = np.arange(nblk * units * unit_len, dtype=np.int64).reshape(nblk, units, unit_len)
                    cells, geo = gathered(ids, world, -1)
                    offs = np.array([[shim.ss_offset(*[int(x) for x in geo], p, g) for g in range(units)] for p in range(nblk)])
                    assert offs.min() >= 0 and offs.max() + unit_len <= cells.size
                    got = cells[offs[:, :, None] + np.arange(unit_len)[None, None, :]]
                    assert np.array_equal(got, ids), (world, units, nblk, unit_len)       # (so never -1: not the padding)
                    assert np.unique(offs).size == nblk * units
                    checked += nblk * units
    assert checked > 20000


def test_one_rank_is_the_whole_vector_layout(shim):
    """q = units: (p units + g) unit_len, the layout the single-GPU kernels address"""
    for units in range(1, 41):
        for nblk in (1, 4):
            for unit_len in (1, 2, 7):
                chunk = units * unit_len * nblk
                for p in range(nblk):
                    for g in range(units):
                        assert shim.ss_offset(units, units, chunk, unit_len, nblk, p, g) == (p * units + g) * unit_len


def _int_vector(rng, shape):
    return rng.integers(-9, 10, size=shape).astype(np.float64)


@pytest.mark.parametrize("world", WORLDS + (12,))
def test_axisop_window_stitches_to_the_whole_sector(shim, world):
    """two c_dw terms on (.., 3) -> (.., 2) of five levels, four phonon blocks, rows of 7 elements: a_src = a_dst = 10, so
    world 10 has one row per rank and world 12 two ranks without rows"""
    ns, nblk, I_ = 5, 4, 7
    src_w, dst_w = comb_words(ns, 3), comb_words(ns, 2)
    coefs = [1.0, -2.0]
    parts = np.stack([forward_table(src_w, dst_w, lev, False, True) for lev in (1, 3)])
    rng = np.random.default_rng(5)
    whole = _int_vector(rng, (nblk, src_w.size, I_))
    ref = real_chain(coefs, [signed_gather(p, whole) for p in parts])
    assert np.abs(ref).sum() > 0
    g, geo = gathered(whole, world, POISON)
    got = np.full_like(ref, np.nan)
    coef = np.array(coefs)
    for r in range(world):
        first, count, _ = plan(dst_w.size, world, r)
        out = np.full(nblk * count * I_ + 1, np.nan)
        shim.ss_axis_window(2, parts.ctypes.data, coef.ctypes.data, nblk, dst_w.size, I_, first, count, geo.ctypes.data,
                            g.ctypes.data, out.ctypes.data)
        assert np.isnan(out[-1])
        got[:, first:first + count, :] = out[:-1].reshape(nblk, count, I_)
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("nblk", [1, 3])
def test_pairs_window_stitches_to_the_whole_sector(shim, built, world, nblk):
    """the pair seed of two orbitals (two terms, each c_up c_dw) and the spin-summed exciton channel (an up-up and a
    down-down term: identity tables on either side) against numpy_pairs on the sector maps"""
    from edipack_amd.observables import exct_chi_seeds, pair_chi_seeds
    from tests.common import make_models
    from tests.pairs_cases import NONE, maps_of, numpy_pairs, species_table, term_parts
    _, pm = make_models("normal", "normal", 2, 1, seed=11)
    sec = (2, 2)
    lists = [pair_chi_seeds(0, 1)[0][0], exct_chi_seeds(1, 0, 1)[0][0]]       # coefficients +-1: exact sums
    rng = np.random.default_rng(7)
    for terms in lists:
        (nu, nd), _, _ = term_parts(pm, sec, terms[0])
        mus, mds = maps_of(pm, *sec)
        mud, mdd = maps_of(pm, nu, nd)
        du_dst, dd_dst = mud.size, mdd.size
        pu = np.full((len(terms), du_dst), NONE, dtype=np.uint32)
        pd = np.full((len(terms), dd_dst), NONE, dtype=np.uint32)
        id_up = id_dw = 0
        for k, t in enumerate(terms):
            tu, td = species_table(mus, mud, t, 0), species_table(mds, mdd, t, 1)
            if tu is None:
                id_up |= 1 << k
            else:
                pu[k] = tu
            if td is None:
                id_dw |= 1 << k
            else:
                pd[k] = td
        whole = _int_vector(rng, (nblk, mds.size, mus.size))
        ref = numpy_pairs(pm, sec, terms, whole.reshape(-1), nblk=nblk).reshape(nblk, dd_dst, du_dst)
        assert np.abs(ref).sum() > 0
        g, geo = gathered(whole, world, POISON)
        coef = np.array([t[0] for t in terms])
        got = np.full_like(ref, np.nan)
        for r in range(world):
            first, count, _ = plan(dd_dst, world, r)
            out = np.full(nblk * count * du_dst + 1, np.nan)
            shim.ss_pairs_window(len(terms), pu.ctypes.data, pd.ctypes.data, id_up, id_dw, coef.ctypes.data, nblk, du_dst, dd_dst,
                                 first, count, geo.ctypes.data, g.ctypes.data, out.ctypes.data)
            assert np.isnan(out[-1])
            got[:, first:first + count, :] = out[:-1].reshape(nblk, count, du_dst)
        assert np.array_equal(got, ref)


def flat_sector(ns, ntot):
    """states of 2 ns bits with ntot set, ascending (down word major), with the two tables the flat kernel indexes a source
    with: off_dw[down word] = position of its first state, rk_up[up word] = rank among the words of its popcount"""
    states = np.array([t for t in range(1 << (2 * ns)) if bin(t).count("1") == ntot], dtype=np.int32)
    off_dw = np.zeros(1 << ns, dtype=np.int32)
    seen = set()
    for k, t in enumerate(states):
        if (t >> ns) not in seen:
            seen.add(int(t >> ns))
            off_dw[t >> ns] = k
    rk_up = np.zeros(1 << ns, dtype=np.int32)
    count = {}
    for w in range(1 << ns):
        n = bin(w).count("1")
        rk_up[w] = count.get(n, 0)
        count[n] = rk_up[w] + 1
    return states, off_dw, rk_up


@pytest.mark.parametrize("world", WORLDS)
def test_flat_window_stitches_to_the_whole_sector(shim, world):
    """c_{1,up} - i c_{0,dw} from N = 3 to N = 2 on 2 x 3 levels, four phonon blocks, complex integer-valued vector"""
    ns, nblk = 3, 4
    src, off_dw, rk_up = flat_sector(ns, 3)
    dst, _, _ = flat_sector(ns, 2)
    pos = {int(t): k for k, t in enumerate(src)}
    assert all(pos[int(t)] == off_dw[t >> ns] + rk_up[t & ((1 << ns) - 1)] for t in src)
    rng = np.random.default_rng(9)
    whole = _int_vector(rng, (nblk, src.size)) + 1j * _int_vector(rng, (nblk, src.size))
    ops = [((1.0, 0.0), 1), ((0.0, -1.0), 0 + ns)]          # (coefficient, level)
    ref = np.zeros((nblk, dst.size), dtype=np.complex128)
    for (cre, cim), lev in ops:
        bit = 1 << lev
        for k, t in enumerate(dst):
            t = int(t)
            if t & bit:
                continue                                     # c leaves the level empty
            s = t | bit
            sign = -1.0 if bin(s & (bit - 1)).count("1") & 1 else 1.0
            ref[:, k] += complex(cre, cim) * sign * whole[:, pos[s]]
    assert np.abs(ref).sum() > 0
    g2, geo = gathered(np.ascontiguousarray(whole).view(np.float64).reshape(nblk, src.size, 2), world, POISON)
    geo = np.array([geo[0], geo[1], geo[2] // 2, 1, nblk], dtype=np.int64)        # counted in (re, im) pairs
    got = np.full_like(ref, np.nan)
    for r in range(world):
        first, count, _ = plan(dst.size, world, r)
        out = np.full(2 * nblk * count + 1, np.nan)
        st = np.ascontiguousarray(dst[first:first + count])
        for k, ((cre, cim), lev) in enumerate(ops):
            shim.ss_flat_window(count, nblk, ns, 1 << lev, 0, st.ctypes.data, off_dw.ctypes.data, rk_up.ctypes.data,
                                geo.ctypes.data, g2.ctypes.data, cre, cim, int(k > 0), out.ctypes.data)
        assert np.isnan(out[-1])
        got[:, first:first + count] = out[:-1].view(np.complex128).reshape(nblk, count)
    assert np.array_equal(got, ref)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_emulation_under_asan_ubsan(tmp_path):
    """the same emulation on the library's own host tables (host_axisop.cpp, host_pairs.cpp), worlds 1 - 12, as a
    stand-alone program under the address and undefined-behaviour sanitizers: nothing loaded into Python"""
    exe = str(tmp_path / "host_shard_seeds_sanitize")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    cmd = ["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-std=c++17", "-I", csrc,
           "-I", os.path.join(ROOT, "tests"), "-o", exe, os.path.join(ROOT, "tests", "host_shard_seeds_sanitize_main.cpp"),
           os.path.join(csrc, "host_axisop.cpp"), os.path.join(csrc, "host_pairs.cpp")]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "0 failures" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
