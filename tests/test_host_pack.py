"""The packed tables of the generic kernels (csrc/host_pack.cpp: ELL and SELL images, the chunk plan and the per-row
lists of the panel sweeps), encoded on the CPU through tests/host_pack.cpp and DECODED here the way the kernels of
kernels_normal.hip / kernels_csr.hip / kernels_panel.hip read them: every image must give back the CSR it was made
from, exact in value and sign, and every padding or dead entry must weigh 0 or name the staged row's zero slot."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.common import make_models
from tests.rows_long_cases import MODEL_SEED, SECTORS, SYNTH_DIMUP, ring_hup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
I64, I32, U32, F64 = np.int64, np.int32, np.uint32, np.float64
VP, L, I, D = C.c_void_p, C.c_int64, C.c_int, C.c_double


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    so = str(tmp_path_factory.mktemp("host_pack") / "host_pack.so")
    csrc = os.path.join(ROOT, "edipack_amd", "csrc")
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),   # (-O0: the compile is most of the run)
                           "-I", csrc, "-o", so, os.path.join(ROOT, "tests", "host_pack.cpp"),
                           os.path.join(csrc, "host_pack.cpp"), os.path.join(csrc, "host_build.cpp")])
    lib = C.CDLL(so)
    lib.hp_error.restype = C.c_char_p
    lib.hp_build_normal.argtypes = [VP, I, I, VP]
    lib.hp_get_csr.argtypes = [I, VP, VP, VP]
    lib.hp_get_fac.argtypes = [VP, VP, VP]
    lib.hp_ell.argtypes = [L, VP, VP, VP, I, I, I, VP]
    lib.hp_ell_get.argtypes = [VP] * 5
    lib.hp_sell.argtypes = [L, L, VP, VP, VP, I, I, D, I, VP]
    lib.hp_sell_get.argtypes = [VP] * 6
    lib.hp_chunks.argtypes = [L, VP, VP, VP, L, L, I, VP, VP]
    lib.hp_merged.argtypes = [L, VP, VP, VP, I, VP, VP, L, L, VP]
    lib.hp_merged_get.argtypes = [VP] * 3
    lib.hp_tile.argtypes = [L, VP, VP, VP, I, I, VP, VP, L, L, VP, I, VP]
    lib.hp_tile_get.argtypes = [VP] * 4
    lib.hp_block.argtypes = [L, VP, VP, VP, I, VP, VP, I, L, VP]
    lib.hp_block_get.argtypes = [VP] * 4
    lib.hp_col_halo.argtypes = [L, I, VP]
    return lib


def ptr(a):
    return a.ctypes.data if a.size else None


class Csr:
    """rows: per row a list of (column, value); value a float or, for complex blocks, a (re, im) pair"""

    def __init__(self, rows, w=1):
        self.nrow, self.w = len(rows), w
        self.rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(I64)
        self.col = np.array([c for r in rows for c, _ in r], I32)
        self.val = np.array([v for r in rows for _, v in r], F64).reshape(-1)
        self.rows = rows

    @classmethod
    def from_arrays(cls, rowptr, col, val):
        return cls([[(int(col[k]), float(val[k])) for k in range(rowptr[i], rowptr[i + 1])] for i in range(len(rowptr) - 1)])

    def args(self):
        return ptr(self.rowptr), ptr(self.col), ptr(self.val)

    def row(self, i, drop_zeros=False):
        return sorted((c, v) for c, v in self.rows[i] if not (drop_zeros and v == 0.0))


def triples(rows, cols, vals):
    """(row, column, value) of the entries given, in a canonical order"""
    o = np.lexsort((vals, cols, rows))
    return np.stack([rows[o].astype(F64), cols[o].astype(F64), vals[o]])


# ---------------------------------------------------------------- ELL ----------------------------------------------------------------

def encode_ell(lib, a, lds, allow_typed=True, allow_16=True):
    info = np.zeros(9, I64)
    lib.hp_ell(a.nrow, *a.args(), int(lds), int(allow_typed), int(allow_16), ptr(info))
    img = dict(nrow=int(info[0]), pitch=int(info[1]), width=int(info[2]), typed=int(info[3]), pk=np.zeros(info[4], U32),
               coef=np.zeros(info[5], F64), pk16=np.zeros(info[6], U32), col=np.zeros(info[7], I32), val=np.zeros(info[8], F64))
    lib.hp_ell_get(*[ptr(img[k]) for k in ("pk", "coef", "pk16", "col", "val")])
    return img


def decode_ell(img, lds):
    """The live entries of an ELL image as the rows kernel reads them; asserts that every other entry is harmless."""
    n, pitch, w = img["nrow"], img["pitch"], img["width"]
    assert pitch % 64 == 0 and 0 <= pitch - n < 64
    rows = np.broadcast_to(np.arange(pitch), (w, pitch))
    if img["pk"].size:
        assert img["pk"].size == w * pitch and img["coef"].size == 128 and not img["col"].size and not img["val"].size
        p = img["pk"].reshape(w, pitch).astype(I64)
        off, neg, cid = p & 0xFFFFFF, (p >> 31) & 1, (p >> 24) & 0x7F
        if lds:  # byte offsets into the staged row; its zero slot lies behind the last column
            assert (off % 8 == 0).all()
            c = off // 8
        else:
            c = off
        if img["typed"]:  # one amplitude per slot; a dead entry names the zero slot (LDS) or has the live bit clear
            assert (img["coef"][:w] > 0).all() and (img["coef"][w:] == 0).all()   # slots past the width: amplitude 0
            amp = np.broadcast_to(img["coef"][:w, None], (w, pitch))
            if lds:
                assert (c <= n).all() and (cid == 0).all()
                live = c != n
            else:
                assert (c < n).all() and (cid <= 1).all()
                live = cid != 0
        else:             # amplitude by coefficient id; id 0 = 0.0 pads
            assert img["coef"][0] == 0.0 and (c < n).all() and not img["pk16"].size
            amp = img["coef"][cid]
            live = amp != 0
        val = np.where(neg == 1, -amp, amp)
    else:
        assert img["col"].size == w * pitch and img["val"].size == w * pitch and not img["coef"].size and not img["pk16"].size
        c, val = img["col"].reshape(w, pitch), img["val"].reshape(w, pitch)
        assert ((c >= 0) & (c < n)).all()
        live = val != 0
    assert not live[:, n:].any()              # the rows that round the pitch up
    return triples(rows[live], c[live], val[live])


def csr_triples(a):
    rows = np.repeat(np.arange(a.nrow), np.diff(a.rowptr))
    keep = a.val != 0            # an explicit 0.0 may be stored as a padding entry or dropped
    return triples(rows[keep], a.col[keep], a.val[keep])


def check_ell16(img):
    """the 16-bit image re-encodes the 32-bit one: same slot, same byte offset, same sign; dead half-words name the zero slot"""
    n, pitch, w = img["nrow"], img["pitch"], img["width"]
    npair = (w + 1) // 2
    assert img["pk16"].size == npair * pitch
    p16 = img["pk16"].reshape(npair, pitch).astype(I64)
    p32 = img["pk"].reshape(w, pitch).astype(I64)
    dead = n * 8
    for k in range(2 * npair):
        half = (p16[k >> 1] >> (16 * (k & 1))) & 0xFFFF
        if k < w:
            assert np.array_equal(half[:n] & 0x7FFF, p32[k, :n] & 0xFFFFFF)
            assert np.array_equal(half[:n] >> 15, p32[k, :n] >> 31)
        else:
            assert (half[:n] == dead).all()      # the dead slot that pads an odd width
        assert (half[n:] == dead).all()


def synth(kind, n):
    """kind: 'typed' three |values|, one twice in a row; 'zero' the same with explicit 0.0 entries; 'many' 130 distinct
    |values|; 'dead' ten |values| of which a row holds one (typed form refused: 10 slots > max(2 w, w + 8) = 9)"""
    rows = []
    if kind in ("typed", "zero"):
        pat = [0.7, -0.7, 0.3, -1.9]
        for i in range(n):
            r = [((i + o) % n, v) for o, v in zip((0, 1, 5, 17), pat[:4 - i % 4])]
            if kind == "zero" and i % 3 == 0:
                r.insert(1, ((i + 2) % n, 0.0))
            rows.append(r)
    elif kind == "many":
        per, cnt = max(3, -(-130 // n)), 0
        for i in range(n):
            r = []
            for j in range(per):
                r.append(((i + 3 * j) % n, (1.0 + 0.01 * (cnt % 130)) * (-1) ** cnt))
                cnt += 1
            rows.append(r)
    elif kind == "dead":
        rows = [[((7 * i) % n, (1.0 + i % 10) * (-1) ** i)] for i in range(n)]
    return Csr(rows)


# (a single row holds every one of its values: the typed form cannot be refused for dead slots at n = 1)
@pytest.mark.parametrize("kind,n", [(k, n) for k in ("typed", "zero", "many", "dead") for n in (1, 63, 65, 4095, 4096)
                                    if not (k == "dead" and n == 1)])
def test_ell_images_of_synthetic_matrices(shim, kind, n):
    a = synth(kind, n)
    want = csr_triples(a)
    for lds in (False, True):
        for allow_typed, allow_16 in ((True, True), (False, True), (True, False)):
            img = encode_ell(shim, a, lds, allow_typed, allow_16)
            assert img["nrow"] == n and img["pitch"] == (n + 63) // 64 * 64
            assert np.array_equal(decode_ell(img, lds), want), (kind, n, lds, allow_typed, allow_16)
            typed = kind in ("typed", "zero") and allow_typed
            assert img["typed"] == int(typed)
            assert bool(img["pk"].size) == (kind != "many") and bool(img["col"].size) == (kind == "many")
            if typed:
                assert img["width"] == 4   # 0.7 twice, 0.3, 1.9: one slot per repetition
            assert bool(img["pk16"].size) == (typed and lds and n <= 4095 and allow_16)
            if img["pk16"].size:
                check_ell16(img)


def test_ell16_pads_an_odd_width_with_a_dead_half_word(shim):
    a = Csr([[((i + 1) % 9, 0.5), ((i + 2) % 9, -0.25), ((i + 4) % 9, 0.125)] for i in range(9)])
    img = encode_ell(shim, a, True)
    assert img["typed"] == 1 and img["width"] == 3 and img["pk16"].size == 2 * 64
    check_ell16(img)
    assert np.array_equal(decode_ell(img, True), csr_triples(a))


def model_sector(lib, norb, nbath, nup, ndw, bath="normal", seed=11, **extra):
    _, pm = make_models("normal", bath, norb, nbath, seed=seed, **extra)
    m = pm.to_c()
    dims = np.zeros(5, I64)
    assert lib.hp_build_normal(C.addressof(m), nup, ndw, ptr(dims)) == 0, lib.hp_error().decode()
    du, dd, nu, nd, nt = (int(x) for x in dims)
    out = []
    for which, (n, nnz) in enumerate(((du, nu), (dd, nd))):
        rp, col, val = np.zeros(n + 1, I64), np.zeros(nnz, I32), np.zeros(nnz, F64)
        lib.hp_get_csr(which, ptr(rp), ptr(col), ptr(val))
        out.append(Csr.from_arrays(rp, col, val))
    coef, jdw, jup = np.zeros(max(nt, 0), F64), np.zeros(max(nt, 0) * dd, U32), np.zeros(max(nt, 0) * du, U32)
    lib.hp_get_fac(ptr(coef), ptr(jdw), ptr(jup))
    return out[0], out[1], coef, jdw, jup


@pytest.fixture(scope="module")
def sector44(shim):
    """norb = 2, nbath = 3, (4, 4): Jx = Jp != 0, so the factored Hnd has terms"""
    return model_sector(shim, 2, 3, 4, 4)


@pytest.mark.parametrize("bath,norb,nbath,extra", [("normal", 2, 3, {}), ("hybrid", 3, 2, {}),
                                                   ("normal", 2, 3, dict(zero_dw=(1, 2)))])
def test_ell_images_of_a_spin_split_sector(shim, bath, norb, nbath, extra):
    """Nspin = 2, nup == ndw: H up and H dw have the same pattern (but for a zeroed down amplitude) and different
    numbers; each side's image decodes to its own matrix."""
    n = (norb * (nbath + 1)) // 2 if bath == "normal" else (norb + nbath) // 2
    up, dw = model_sector(shim, norb, nbath, n, n, bath=bath, spin_split=True, **extra)[:2]
    assert up.nrow == dw.nrow
    tu, td = csr_triples(up), csr_triples(dw)
    assert (tu.shape != td.shape) == bool(extra) and not np.array_equal(tu, td)
    for a, want in ((up, tu), (dw, td)):
        for lds in (False, True):
            img = encode_ell(shim, a, lds)
            assert img["typed"] == 1
            assert np.array_equal(decode_ell(img, lds), want)
        check_ell16(img)


@pytest.mark.parametrize("norb,nbath,nup", [(1, 13, 7), (2, 3, 4)])
def test_ell_images_of_a_real_hup(shim, norb, nbath, nup):
    up = model_sector(shim, norb, nbath, nup, 1 if norb == 1 else 4)[0]
    want = csr_triples(up)
    for lds in (False, True):
        img = encode_ell(shim, up, lds)
        assert img["typed"] == 1
        assert np.array_equal(decode_ell(img, lds), want)
    check_ell16(img)
    if norb == 1:   # DimUp = 3432: bit 14 of the byte offset and the sign at bit 15 are both in use
        assert up.nrow == 3432
        half = np.concatenate([img["pk16"] & 0xFFFF, img["pk16"] >> 16])
        live = (half & 0x7FFF) != up.nrow * 8
        assert (half[live] & 0x4000).any() and (half[live] & 0x8000).any()
    img = encode_ell(shim, up, True, allow_16=False)
    assert img["typed"] == 1 and not img["pk16"].size
    img = encode_ell(shim, up, True, allow_typed=False)
    assert img["typed"] == 0 and img["pk"].size and np.array_equal(decode_ell(img, True), want)


def check_long_row_image(lib, up):
    """The image the rows kernel gets for `up`, as tests/test_gpu_rows_long.py assumes it: typed; with a 16-bit form
    whose live half-words use bit 14 of the byte offset and the sign bit beside it for rows of 2049 to 4095 columns;
    without one from 4096 columns on."""
    img = encode_ell(lib, up, True)
    assert img["typed"] == 1 and img["pk"].size
    assert np.array_equal(decode_ell(img, True), csr_triples(up))
    if up.nrow >= 4096:
        assert not img["pk16"].size
        return img
    assert img["pk16"].size
    check_ell16(img)
    if up.nrow > 2048:
        half = np.concatenate([img["pk16"] & 0xFFFF, img["pk16"] >> 16])
        live = (half & 0x7FFF) != up.nrow * 8
        assert (half[live] & 0x4000).any() and (half[live] & 0x8000).any()
    return img


@pytest.mark.parametrize("bath,norb,nbath,sec", SECTORS)
def test_long_row_sectors_have_a_16bit_image(shim, bath, norb, nbath, sec):
    """the Hup of the sectors of test_gpu_rows_long.py, as the library builds it and as the oracle hands it over"""
    from oracle import oracle as O
    up = model_sector(shim, norb, nbath, *sec, bath=bath, seed=MODEL_SEED)[0]
    om, _ = make_models("normal", bath, norb, nbath, seed=MODEL_SEED)
    ho = O.HNormal(om, *sec)
    assert 2048 < up.nrow == ho.dimup <= 4095
    check_long_row_image(shim, up)
    check_long_row_image(shim, Csr.from_arrays(*ho.up))


@pytest.mark.parametrize("n", SYNTH_DIMUP)
def test_synthetic_long_rows_16bit_image_ends_at_4095(shim, n):
    """the ring stencils of test_gpu_rows_long.py: six slots, 16-bit image up to 4095 columns and none beyond"""
    up = Csr.from_arrays(*ring_hup(n))
    dense = {(i, j): v for i in range(n) for j, v in up.rows[i]}
    assert all(dense[(j, i)] == v for (i, j), v in dense.items())                # symmetric
    # the first and last rows reach the last and first columns (three wrapped hops each), with both signs between them
    wrapped = [v for j, v in up.rows[0] if j in (n - 1, n - 7, n - 1031)] + [v for j, v in up.rows[n - 1] if j in (0, 6, 1030)]
    assert len(wrapped) == 6 and {np.sign(v) for v in wrapped} == {-1.0, 1.0}
    img = check_long_row_image(shim, up)
    assert img["width"] == 6 and bool(img["pk16"].size) == (n <= 4095)
    if n == 4095:
        assert n * 8 == 32760 and ((img["pk16"] & 0x7FFF) == 32760).any()        # the largest offset the format holds


# ---------------------------------------------------------------- SELL ---------------------------------------------------------------

def encode_sell(lib, a, ncol, is_loc, max_pad=1.6, allow_packed=True):
    info = np.zeros(9, I64)
    lib.hp_sell(a.nrow, ncol, *a.args(), int(a.w == 2), int(is_loc), max_pad, int(allow_packed), ptr(info))
    img = dict(built=int(info[0]), nslice=int(info[1]), packed=int(info[2]), ptr=np.zeros(info[3], I32), pk=np.zeros(info[4], U32),
               dict=np.zeros(info[5], F64), diag=np.zeros(info[6], F64), col=np.zeros(info[7], I32), val=np.zeros(info[8], F64))
    lib.hp_sell_get(*[ptr(img[k]) for k in ("ptr", "pk", "dict", "diag", "col", "val")])
    return img


def check_sell(img, a, is_loc):
    """rows of the image in slot order == rows of the CSR sorted by column; padding repeats the last column with weight 0"""
    n, w = a.nrow, a.w
    assert img["built"] and img["nslice"] == (n + 63) // 64 and img["ptr"].size == img["nslice"] + 1 and img["ptr"][0] == 0
    split_diag = bool(img["packed"]) and is_loc
    if img["packed"]:
        assert img["dict"].size == 256 * w and (img["dict"][:w] == 0).all() and not img["col"].size and not img["val"].size
        assert img["pk"].size == img["ptr"][-1] * 64 and img["diag"].size == (n * w if is_loc else 0)
    else:
        assert img["col"].size == img["ptr"][-1] * 64 and img["val"].size == img["col"].size * w
        assert not img["pk"].size and not img["dict"].size and not img["diag"].size
    zero = tuple([0.0] * w)
    for i in range(img["nslice"] * 64):
        s, lane = divmod(i, 64)
        got = []
        for k in range(img["ptr"][s], img["ptr"][s + 1]):
            o = k * 64 + lane
            if img["packed"]:
                p = int(img["pk"][o])
                got.append((p & 0xFFFFFF, tuple(img["dict"][(p >> 24) * w:(p >> 24) * w + w])))
            else:
                got.append((int(img["col"][o]), tuple(img["val"][o * w:o * w + w])))
        row = a.rows[i] if i < n else []
        tup = [(c, tuple(np.atleast_1d(np.array(v, F64)))) for c, v in row]
        want = sorted(e for e in tup if not (split_diag and e[0] == i))
        assert got[:len(want)] == want, i
        assert all(e == (want[-1][0] if want else 0, zero) for e in got[len(want):]), i
        if split_diag and i < n:
            d = sum((np.array(v) for c, v in tup if c == i), np.zeros(w))
            assert np.array_equal(img["diag"][i * w:i * w + w], d)
    # every slice as wide as its longest row
    for s in range(img["nslice"]):
        longest = max(len([1 for c, _ in a.rows[i] if not (split_diag and c == i)]) for i in range(s * 64, min(n, s * 64 + 64)))
        assert img["ptr"][s + 1] - img["ptr"][s] == longest


def sell_matrix(n, ncol, w, with_diag, nvals=5):
    rng = np.random.default_rng(3)
    vals = [tuple(rng.uniform(0.5, 2.0, w) * rng.choice([-1, 1], w)) for _ in range(nvals)]
    rows, cnt = [], 0
    for i in range(n):
        cols = list(rng.choice(ncol, 3 + i % 3, replace=False))      # unsorted
        if with_diag and i not in cols:
            cols[0] = i
        r = []
        for c in cols:
            r.append((int(c), vals[cnt % nvals] if w == 2 else vals[cnt % nvals][0]))
            cnt += 1
        rows.append(r)
    return Csr(rows, w)


@pytest.mark.parametrize("w", [1, 2])
@pytest.mark.parametrize("is_loc", [False, True])
def test_sell_images(shim, w, is_loc):
    a = sell_matrix(70, 70 if is_loc else 200, w, is_loc)
    # (the 6 rows of the second slice pad it beyond the 1.6 of the flat blocks: the bound of the Hnd block)
    assert not encode_sell(shim, a, 70 if is_loc else 200, is_loc)["built"]
    img = encode_sell(shim, a, 70 if is_loc else 200, is_loc, max_pad=16.0)
    assert img["packed"] == 1
    check_sell(img, a, is_loc)
    img = encode_sell(shim, a, 70 if is_loc else 200, is_loc, max_pad=16.0, allow_packed=False)
    assert img["packed"] == 0
    check_sell(img, a, is_loc)


def test_sell_special_cases(shim):
    # a diagonal matrix of the loc block: everything lands in diag
    a = Csr([[(i, 1.0 + i)] for i in range(70)])
    img = encode_sell(shim, a, 70, True)
    assert img["built"] and img["packed"] and (img["ptr"] == 0).all() and not img["pk"].size
    assert np.array_equal(img["diag"], 1.0 + np.arange(70))
    check_sell(img, a, True)
    # 257 distinct values: the dictionary overflows, plain form
    a = sell_matrix(70, 200, 1, False, nvals=257)
    img = encode_sell(shim, a, 200, False, max_pad=16.0)
    assert img["built"] and not img["packed"]
    check_sell(img, a, False)
    # 24-bit columns only
    img = encode_sell(shim, sell_matrix(70, 200, 1, False), 1 << 24, False, max_pad=16.0)
    assert img["built"] and not img["packed"]
    # ragged beyond max_pad: one long row in a slice of empty ones
    a = Csr([[(c, 1.0) for c in range(64)]] + [[] for _ in range(69)])
    assert not encode_sell(shim, a, 200, False)["built"]
    img = encode_sell(shim, a, 200, False, max_pad=64.0)
    assert img["built"]
    check_sell(img, a, False)
    # nothing to encode
    assert not encode_sell(shim, Csr([[], []]), 2, False)["built"]


# ------------------------------------------------- chunk plan, tile / block / merged lists -------------------------------------------

def nd_terms(coef, jdw, dim_dw, g):
    """the factored Hnd terms that apply to down row g: (partner row, term, signed coefficient)"""
    out = []
    for t in range(len(coef)):
        jd = int(jdw[t * dim_dw + g])
        if jd != NONE:
            out.append((jd & 0x7FFFFFFF, t, -coef[t] if jd >> 31 else coef[t]))
    return out


def plan(lib, dw, first, count, rmax):
    starts, longest = np.zeros(count + 1, I32), C.c_int(0)
    ns = lib.hp_chunks(dw.nrow, *dw.args(), first, count, rmax, ptr(starts), C.addressof(longest))
    starts = starts[:ns]
    assert starts[0] == 0 and starts[-1] == count                      # the chunks partition [0, count)
    assert (np.diff(starts) >= 1).all() and np.diff(starts).max() == longest.value <= rmax
    return starts


@pytest.mark.parametrize("rmax", [8, 64])
@pytest.mark.parametrize("first,count", [(0, None), (5, 40)])
@pytest.mark.parametrize("with_nd", [False, True])
def test_tile_lists(shim, sector44, rmax, first, count, with_nd):
    _, dw, coef, jdw, _ = sector44
    dd = dw.nrow
    count = dd if count is None else count
    assert len(coef) > 0
    starts = plan(shim, dw, first, count, rmax)
    info = np.zeros(6, I64)
    shim.hp_tile(dd, *dw.args(), int(with_nd), len(coef), ptr(coef), ptr(jdw), first, count, ptr(starts), len(starts), ptr(info))
    meta, col, val, lbeg = np.zeros((info[0], 4), I32), np.zeros(info[1], I32), np.zeros(info[2], F64), np.zeros(info[3], I32)
    shim.hp_tile_get(ptr(meta), ptr(col), ptr(val), ptr(lbeg))
    assert info[0] == count and info[1] == info[2] and bool(info[5]) == with_nd
    end = 0
    for ch in range(len(starts) - 1):
        cs, ce = int(starts[ch]), int(starts[ch + 1])
        assert lbeg[ch] == meta[cs, 0]
        for r in range(cs, ce):
            g = first + r
            x, y, z, nnd = (int(v) for v in meta[r])
            assert x == end and x % 4 == 0 and y % 4 == 0 and z % 4 == 0       # rows follow each other on batch boundaries
            inside = [(int(col[q]), val[q]) for q in range(x, x + y)]
            outside = [(int(col[q]), val[q]) for q in range(x + y, x + y + z)]
            assert all(0 <= c < ce - cs for c, _ in inside)                    # staged row index inside the chunk
            assert all(c == r - cs for c, v in inside if v == 0) and all(c == g for c, v in outside if v == 0)   # padding: own row
            live_out = [(c, v) for c, v in outside if v != 0]
            assert all(not (first + cs <= c < first + ce) for c, _ in live_out)
            assert sorted([(first + cs + c, v) for c, v in inside if v != 0] + live_out) == dw.row(g)
            terms = [((int(col[q]) & 0xFFFFFF), (int(col[q]) >> 24) - 1, val[q]) for q in range(x + y + z, x + y + z + nnd)]
            assert terms == (nd_terms(coef, jdw, dd, g) if with_nd else [])
            end = (x + y + z + nnd + 3) // 4 * 4
            assert (col[x + y + z + nnd:end] == 0).all() and (val[x + y + z + nnd:end] == 0).all()
    assert lbeg.size == len(starts) and lbeg[-1] == end and col.size == end + 8
    assert (col[end:] == 0).all() and (val[end:] == 0).all()                   # the tail batched reads run into
    assert info[4] == max(4, int(np.diff(lbeg).max()))


def block_lists(lib, dw, coef, jdw, shift, lds_kb):
    info = np.zeros(7, I64)
    lib.hp_block(dw.nrow, *dw.args(), len(coef), ptr(coef), ptr(jdw), shift, lds_kb, ptr(info))
    out = dict(fits=int(info[0]), rows=int(info[1]), list_cap=int(info[2]), meta=np.zeros((info[3], 4), I32),
               ent=np.zeros(info[4], U32), wtab=np.zeros(info[5], F64), lend=np.zeros(info[6], I32))
    lib.hp_block_get(*[ptr(out[k]) for k in ("meta", "ent", "wtab", "lend")])
    return out


@pytest.mark.parametrize("shift", [4, 5, 6])
@pytest.mark.parametrize("lds_kb", [4, 32])
def test_block_lists(shim, sector44, shift, lds_kb):
    _, dw, coef, jdw, _ = sector44
    dd = dw.nrow
    b = block_lists(shim, dw, coef, jdw, shift, lds_kb)
    R = max(32, min(lds_kb * 1024 // (8 << shift), 4096) // 32 * 32)
    assert b["fits"] and b["rows"] == R and b["wtab"].size == 256 and b["wtab"][0] == 0.0 and b["meta"].shape[0] == dd
    ent, wtab, meta = b["ent"].astype(I64), b["wtab"], b["meta"]
    end, cap = 0, 4
    for g in range(dd):
        cs = g // R * R
        x, y, z, nnd = (int(v) for v in meta[g])
        assert x == end and y % 4 == 0 and z % 4 == 0
        dec = [(int(e & 0xFFFF), wtab[(e >> 16) & 255], int(e >> 24)) for e in ent[x:x + y + z + nnd]]
        inside, outside, nd = dec[:y], dec[y:y + z], dec[y + z:]
        assert all(t == 0 for _, _, t in inside + outside)
        assert all(0 <= c < R and cs + c < dd for c, _, _ in inside)
        assert all(c == g - cs for c, v, _ in inside if v == 0) and all(c == g for c, v, _ in outside if v == 0)
        live_out = [(c, v) for c, v, _ in outside if v != 0]
        assert all(not (cs <= c < cs + R) for c, _ in live_out)
        assert sorted([(cs + c, v) for c, v, _ in inside if v != 0] + live_out) == dw.row(g)
        assert [(c, t - 1, v) for c, v, t in nd] == nd_terms(coef, jdw, dd, g)
        end = (x + y + z + nnd + 3) // 4 * 4
        assert (ent[x + y + z + nnd:end] == 0).all()
        if g == dd - 1 or (g + 1) % R == 0:
            assert b["lend"][g // R] == end
            cap = max(cap, end - int(meta[cs, 0]))
    assert b["lend"].size == (dd + R - 1) // R and b["list_cap"] == cap
    assert ent.size == end + 8 and (ent[end:] == 0).all()


def test_block_lists_refuse_more_than_256_weights(shim):
    dw = Csr([[((i + 1) % 300, 1.0 + 0.001 * i)] for i in range(300)])
    none = np.zeros(0, F64)
    assert not block_lists(shim, dw, none, np.zeros(0, U32), 4, 32)["fits"]
    few = Csr([[((i + 1) % 300, 1.0 + 0.001 * (i % 100))] for i in range(300)])
    assert block_lists(shim, few, none, np.zeros(0, U32), 4, 32)["fits"]


@pytest.mark.parametrize("first,count", [(0, None), (5, 40)])
def test_merged_list(shim, sector44, first, count):
    _, dw, coef, jdw, _ = sector44
    dd = dw.nrow
    count = dd if count is None else count
    info = np.zeros(3, I64)
    shim.hp_merged(dd, *dw.args(), len(coef), ptr(coef), ptr(jdw), first, count, ptr(info))
    rp, col, val = np.zeros(info[0], I32), np.zeros(info[1], I32), np.zeros(info[2], F64)
    shim.hp_merged_get(ptr(rp), ptr(col), ptr(val))
    assert rp.size == count + 1 and rp[0] == 0 and col.size == val.size == rp[-1] + 8
    for r in range(count):
        g = first + r
        ent = [(int(col[q]) & 0xFFFFFF, (int(col[q]) >> 24) & 0xFF, val[q]) for q in range(rp[r], rp[r + 1])]
        nhop = len(dw.rows[g])
        assert [(c, v) for c, t, v in ent[:nhop] if t == 0] == dw.rows[g]          # Hdw entries first, tag 0, in CSR order
        assert [(c, t - 1, v) for c, t, v in ent[nhop:]] == nd_terms(coef, jdw, dd, g)
    assert (col[rp[-1]:] == 0).all() and (val[rp[-1]:] == 0).all()


def test_col_halo(shim, sector44):
    up, _, coef, _, jup = sector44
    du = up.nrow
    j = jup.reshape(len(coef), du).astype(I64)
    want = max(abs(int(j[t, c] & 0x7FFFFFFF) - c) for t in range(len(coef)) for c in range(du) if j[t, c] != NONE)
    assert shim.hp_col_halo(du, len(coef), ptr(jup)) == want > 0
