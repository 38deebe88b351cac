"""GPU tests of c / c^+ on phonon, complex normal-mode and ed_total_ud=F sectors (kernels_axisop.hip through
edigpu_apply_op_normal / edigpu_apply_cops_normal / edigpu_apply_cops_normal_z) and on superc / nonsu2 phonon sectors
(edigpu_apply_op_flat).

References are numpy restatements on the sector maps (tests/axisop_cases.py): sector_map for ed_total_ud=T, the per-axis
combination bases and v.reshape(dims[::-1]) for ed_total_ud=F; and the library's own earlier path, the phonon-free kind-0
kernel applied block by block.

Arithmetic restated (kernels_axisop.hip).  x_t = the signed gather of term t, 0 without a preimage, t ascending.
Real coefficients: acc = coef_0 x_0, then acc = fma(coef_t, x_t, acc) -- the fma is restated exactly (one rounding).
Complex coefficients: y_t = (cre x.re - cim x.im, cre x.im + cim x.re), every product and sum rounded, acc = y_0, then
acc = y_t + acc.  A single operator is a signed copy, so np.array_equal is an exact test.

The _z bound is derived, not measured: with nterms terms every component of the result is a sum of at most 2 nterms
rounded products, so |err| <= nterms 2^-53 sum_t |coef_t x_t| covers [1, +-i], whose products are exact and whose one sum
per component rounds once.

End to end.  G_aa(i w_n) on 64 Matsubara points: ground state -> seeds -> lanczos_tridiag_dev run to the sector dimension
-> spectral sum, against the dense spectral sum.  The yardstick is the same comparison on the route that existed before
(real, phonon-free, same Norb / Nbath, the half-filled sector, apply_op_normal_kernel): it measured BASELINE_E2E below,
and each new sector is allowed ten times the figure of its own model (the new sectors are up to nph + 1 times larger; the
tridiagonalisation is the same code).  Every case takes the half-filled sector, where the ground state of these
particle-hole symmetric models lives; for ed_total_ud=F that is nups = ndws = (2, 2) of chains of 4 levels, dims 6.
Measured on an MI355X: Holstein 2.6e-14 (yardstick 1.6e-14), complex 8.4e-15 (4.7e-15), ed_total_ud=F 6.3e-14 (1.6e-14).
Away from half filling the full-dimension Lanczos of an ed_total_ud=F sector is less accurate -- nups, ndws =
(2, 1), (1, 2) measured 2.2e-12 with bit-exact seeds -- which DESIGN.md 4.9 records; it is not covered here."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests.axisop_cases import U, comb_words, cplx_chain, forward_table, real_chain, signed_gather
from tests.common import make_models
from tests.ph_cases import set_phonons

pytestmark = pytest.mark.gpu

UP, DW = 0, 1
FILL = 7.0
# relative error max|G - G_dense| / max|G_dense| of the end-to-end comparison on the earlier route, measured on an MI355X
# (test_green_function_end_to_end prints them again), per model; the new sectors are allowed ten times that
BASELINE_E2E = {"holstein": 1.622e-14, "complex": 4.677e-15, "orbs": 1.568e-14}


def _H():
    from edipack_amd.hamiltonian import SectorHamiltonian
    return SectorHamiltonian


class Handles:
    """the sector handles of one model, built on demand and destroyed together"""

    def __init__(self, build):
        self.build, self.h = build, {}

    def __call__(self, *key):
        if key not in self.h:
            self.h[key] = self.build(*key)
        return self.h[key]

    def destroy(self):
        for h in self.h.values():
            h.destroy()
        self.h = {}


def _orbs_models(norb, nbath, seed=11):
    """what ed_total_ud=F requires: no spin exchange / pair hopping, a diagonal real impHloc"""
    om, pm = make_models("normal", "normal", norb, nbath, seed=seed, jxp=0.0)
    hl = np.zeros_like(om.hloc)
    for k in range(norb):
        hl[0, 0, k, k] = om.hloc[0, 0, k, k].real
    om.hloc = hl
    pm.hloc = hl.copy()
    return om, pm


def _complexify(om, pm, seed):
    """complex Hermitian impHloc on an oracle / product model pair"""
    t = np.random.default_rng(seed).uniform(-0.4, 0.4, (om.norb, om.norb))
    t = t - t.T
    for m in (om, pm):
        hl = np.asarray(m.hloc, complex).copy()
        hl[0, 0] = hl[0, 0] + 1j * t
        m.hloc = hl


def _vector(dim, cplx, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(dim) + 1j * rng.standard_normal(dim) if cplx else rng.standard_normal(dim)


def _apply(h_src, h_dst, v, ops, coefs=None):
    """one call on fresh device vectors (destination pre-filled); returns the result, checks that the source is untouched"""
    import torch
    src = torch.from_numpy(np.ascontiguousarray(v)).cuda()
    dst = torch.full((h_dst.dim,), FILL, dtype=src.dtype, device="cuda")
    if coefs is None:
        (create, iorb, ispin), = ops
        h_src.apply_op_to(h_dst, src.data_ptr(), dst.data_ptr(), iorb, ispin, bool(create))
    else:
        h_src.apply_cops_to(h_dst, src.data_ptr(), dst.data_ptr(), coefs, [o[0] for o in ops], [o[1] for o in ops],
                            [o[2] for o in ops])
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy().view(np.float64), np.ascontiguousarray(v).view(np.float64)), "source touched"
    return dst.cpu().numpy()


# ---- restatements --------------------------------------------------------------------------------------------------
def _normal_gathers(pm, sec, ops, v, nblk):
    """[x_t] as float64 tensors [O][A_dst][I] of ed_total_ud=T operators of one spin and direction, and the destination"""
    from edipack_amd.hamiltonian import sector_map
    nup, ndw = sec
    create, _, spin = ops[0]
    assert all(o[0] == create and o[2] == spin for o in ops)
    n_src = sec[spin]
    n_dst = n_src + (1 if create else -1)
    dest = (n_dst, ndw) if spin == UP else (nup, n_dst)
    ws = sector_map(pm, *sec, spin).astype(np.int64)
    wd = sector_map(pm, *dest, spin).astype(np.int64)
    du, dd = sector_map(pm, *sec, 0).size, sector_map(pm, *sec, 1).size
    w = 2 if np.iscomplexobj(v) else 1
    shape = (dd * nblk, du, w) if spin == UP else (nblk, dd, w * du)
    src3 = np.ascontiguousarray(v).view(np.float64).reshape(shape)
    return [signed_gather(forward_table(ws, wd, o[1], bool(create), True), src3) for o in ops], dest


def _orbs_gathers(norb, nlev, nups, ndws, ops, v):
    create, iorb, spin = ops[0]
    assert all(tuple(o) == tuple(ops[0]) for o in ops)
    occ = list(nups) + list(ndws)
    axis = iorb + spin * norb
    dims = [comb_words(nlev, n).size for n in occ]
    n_dst = occ[axis] + (1 if create else -1)
    dest = list(occ)
    dest[axis] = n_dst
    part = forward_table(comb_words(nlev, occ[axis]), comb_words(nlev, n_dst), 0, bool(create), False)
    # v.reshape(dims[::-1]): axis 0 fastest; the operator's axis in the middle of [O][A][I]
    src3 = v.reshape(dims[::-1]).reshape(int(np.prod(dims[axis + 1:], dtype=np.int64)), dims[axis],
                                         int(np.prod(dims[:axis], dtype=np.int64)))
    return [signed_gather(part, src3) for _ in ops], (tuple(dest[:norb]), tuple(dest[norb:]))


def _as(v_like, x):
    """a float64 tensor back to the flat vector type of v_like"""
    flat = np.ascontiguousarray(x).reshape(-1)
    return flat.view(np.complex128) if np.iscomplexobj(v_like) else flat


# ---- the cases of the issue ------------------------------------------------------------------------------------------
# name -> (kind, norb, nbath, nph, [(source sector, spins served from it)])
NORMAL_CASES = {
    "a_phonons_gather": ("ph", 2, 4, 2, [((5, 1), (UP,)), ((1, 5), (DW,))]),     # I = 1 and I = 10 < 64, three blocks
    "b_phonons_rows": ("ph", 2, 4, 2, [((4, 2), (DW,))]),                         # I = 210: rows kernel, tail
    "c_holstein_small": ("ph", 1, 3, 3, [((2, 2), (UP, DW))]),                    # everything < 64
    "d_complex_small": ("z", 2, 2, 0, [((3, 3), (UP, DW))]),                      # I = 2 and 2 * 20 = 40
    "e_complex_rows": ("z", 2, 4, 0, [((5, 2), (DW,))]),                          # I = 2 * 252 = 504
}
ORBS_CASES = {
    "f_orbs_four_axes": (2, 4, (2, 2), (2, 3)),        # dims 10, 10, 10, 10: I = 1, 10, 100, 1000 = 7 * 128 + 104
    "g_orbs_six_axes": (3, 2, (1, 2, 1), (2, 1, 1)),
}


def _normal_setup(kind, norb, nbath, nph, seed=11):
    om, pm = make_models("normal", "normal", norb, nbath, seed=seed)
    if kind == "ph":
        for m in (om, pm):
            set_phonons(m, nph)
        build = lambda nup, ndw: _H().normal_from_model(pm, nup, ndw)      # noqa: E731
    elif kind == "z":
        _complexify(om, pm, seed + 1)
        build = lambda nup, ndw: _H().normal_cmplx_from_model(pm, nup, ndw)  # noqa: E731
    else:
        build = lambda nup, ndw: _H().normal_from_model(pm, nup, ndw)      # noqa: E731
    return om, pm, Handles(build)


@pytest.mark.parametrize("case", sorted(NORMAL_CASES))
def test_single_operators_normal(gpu, case):
    """every (iorb, ispin, create) with an existing destination is the signed copy of the restatement, every element of
    the pre-filled destination written"""
    kind, norb, nbath, nph, sources = NORMAL_CASES[case]
    _, pm, hs = _normal_setup(kind, norb, nbath, nph)
    n_run, seen_i = 0, set()
    try:
        for sec, spins in sources:
            h = hs(*sec)
            v = _vector(h.dim, kind == "z", 100 + sum(sec))
            for spin, iorb, create in itertools.product(spins, range(norb), (0, 1)):
                if not 0 <= sec[spin] + (1 if create else -1) <= pm.ns:
                    continue
                (x,), dest = _normal_gathers(pm, sec, [(create, iorb, spin)], v, nph + 1)
                out = _apply(h, hs(*dest), v, [(create, iorb, spin)])
                assert not np.any(out == FILL), "an element of the destination was not written"
                assert np.array_equal(out, _as(v, x)), (case, sec, spin, iorb, create)
                assert np.any(out)
                seen_i.add(x.shape[2])
                n_run += 1
    finally:
        hs.destroy()
    assert n_run == sum(len(s) for _, s in sources) * norb * 2
    want_i = {"a_phonons_gather": {1, 10}, "b_phonons_rows": {210}, "c_holstein_small": {1, 6}, "d_complex_small": {2, 40},
              "e_complex_rows": {504}}[case]
    assert seen_i == want_i


@pytest.mark.parametrize("case", sorted(ORBS_CASES))
def test_single_operators_orbs(gpu, case):
    norb, nbath, nups, ndws = ORBS_CASES[case]
    _, pm = _orbs_models(norb, nbath)
    hs = Handles(lambda u, d: _H().orbs_from_model(pm, u, d))
    n_run, seen_i = 0, set()
    try:
        h = hs(nups, ndws)
        v = _vector(h.dim, False, 5)
        for spin, iorb, create in itertools.product((UP, DW), range(norb), (0, 1)):
            n = (nups, ndws)[spin][iorb] + (1 if create else -1)
            if not 0 <= n <= 1 + nbath:
                continue
            (x,), dest = _orbs_gathers(norb, 1 + nbath, nups, ndws, [(create, iorb, spin)], v)
            out = _apply(h, hs(*dest), v, [(create, iorb, spin)])
            assert not np.any(out == FILL), "an element of the destination was not written"
            assert np.array_equal(out, x.reshape(-1)), (case, spin, iorb, create)
            assert np.any(out)
            seen_i.add(x.shape[2])
            n_run += 1
    finally:
        hs.destroy()
    assert n_run == 4 * norb
    assert seen_i == ({1, 10, 100, 1000} if case == "f_orbs_four_axes" else {1, 3, 9, 27, 81, 243})


@pytest.mark.parametrize("mode,sector", [("superc", 0), ("nonsu2", 4)])
@pytest.mark.parametrize("form", ["stored", "direct"])
def test_flat_phonon_sectors_block_by_block(gpu, mode, sector, form):
    """case h: whole superc / nonsu2 phonon sectors; every phonon block equals, bit for bit, what the phonon-free handles
    of the same model give through the same entry point"""
    from edipack_amd import capi
    nph = 2
    _, pm0 = make_models(mode, "normal", 1, 3, seed=12)
    _, pm = make_models(mode, "normal", 1, 3, seed=12)
    pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = nph, 0.8, 0.0, np.array([[0.3]])
    build = _H().direct_from_model if form == "direct" else _H().flat_from_model
    hs, hs0 = Handles(lambda s: build(pm, s)), Handles(lambda s: build(pm0, s))
    n_run = 0
    try:
        h, h0 = hs(sector), hs0(sector)
        assert h.dim == 3 * h0.dim
        v = _vector(h.dim, True, 9)
        for spin, create in itertools.product((UP, DW), (0, 1)):
            d = 1 if create else -1
            dest = sector + (d if spin == UP else -d) if mode == "superc" else sector + d
            try:
                hd, hd0 = hs(dest), hs0(dest)
            except capi.EdigpuError:
                continue                                   # no such sector
            out = _apply(h, hd, v, [(create, 0, spin)])
            assert not np.any(out == FILL)
            for p in range(nph + 1):
                ref = _apply(h0, hd0, v[p * h0.dim:(p + 1) * h0.dim], [(create, 0, spin)])
                assert np.array_equal(out[p * hd0.dim:(p + 1) * hd0.dim].view(np.int64), ref.view(np.int64)), (spin, create, p)
            assert np.any(out)
            n_run += 1
    finally:
        hs.destroy()
        hs0.destroy()
    assert n_run == 4


@pytest.mark.parametrize("case", ["a_phonons_gather", "b_phonons_rows", "c_holstein_small"])
def test_phonon_sector_equals_the_phonon_free_kernel_block_by_block(gpu, case):
    """the earlier route (apply_op_normal_kernel through nph = 0 handles of the same model) on every phonon block, on the
    64-bit patterns"""
    kind, norb, nbath, nph, sources = NORMAL_CASES[case]
    _, pm, hs = _normal_setup(kind, norb, nbath, nph)
    _, pm0, hs0 = _normal_setup("real", norb, nbath, 0)
    n_run = 0
    try:
        for sec, spins in sources:
            h, h0 = hs(*sec), hs0(*sec)
            assert h.dim == (nph + 1) * h0.dim
            v = _vector(h.dim, False, 200 + sum(sec))
            for spin, iorb, create in itertools.product(spins, range(norb), (0, 1)):
                dest = list(sec)
                dest[spin] += 1 if create else -1
                if not 0 <= dest[spin] <= pm.ns:
                    continue
                hd, hd0 = hs(*dest), hs0(*dest)
                op = [(create, iorb, spin)]
                out = _apply(h, hd, v, op)
                for p in range(nph + 1):
                    ref = _apply(h0, hd0, v[p * h0.dim:(p + 1) * h0.dim], op)
                    assert np.array_equal(out[p * hd0.dim:(p + 1) * hd0.dim].view(np.int64), ref.view(np.int64))
                # and with a coefficient, as apply_Cops calls it
                out = _apply(h, hd, v, op, coefs=[-0.375])
                for p in range(nph + 1):
                    ref = _apply(h0, hd0, v[p * h0.dim:(p + 1) * h0.dim], op, coefs=[-0.375])
                    assert np.array_equal(out[p * hd0.dim:(p + 1) * hd0.dim].view(np.int64), ref.view(np.int64))
                n_run += 1
    finally:
        hs.destroy()
        hs0.destroy()
    assert n_run == sum(len(s) for _, s in sources) * norb * 2


@pytest.mark.parametrize("case,sec,spin", [("b_phonons_rows", (4, 2), DW), ("c_holstein_small", (2, 2), UP),
                                           ("a_phonons_gather", (5, 1), UP), ("d_complex_small", (3, 3), DW),
                                           ("e_complex_rows", (5, 2), DW)])
def test_several_terms_real_coefficients(gpu, case, sec, spin):
    """apply_cops with 2 terms (c_a + c_b) and 8 terms with random coefficients: bit-equal with the documented chain"""
    kind, norb, nbath, nph, _ = NORMAL_CASES[case]
    _, pm, hs = _normal_setup(kind, norb, nbath, nph)
    rng = np.random.default_rng(77)
    n_eight = 0
    try:
        h = hs(*sec)
        v = _vector(h.dim, kind == "z", 31)
        for create in (0, 1):
            for coefs, orbs in (((1.0, 1.0), (0, norb - 1)), (tuple(rng.standard_normal(8)), tuple(k % norb for k in range(8)))):
                ops = [(create, a, spin) for a in orbs]
                xs, dest = _normal_gathers(pm, sec, ops, v, nph + 1)
                if len(coefs) == 8 and xs[0].size > 20000:
                    continue                    # the exact restatement of the fma is element by element: the smaller destination
                n_eight += len(coefs) == 8
                out = _apply(h, hs(*dest), v, ops, coefs=coefs)
                ref = _as(v, real_chain(coefs, xs))
                assert not np.any(out == FILL)
                assert np.array_equal(out, ref), (case, create, len(coefs))
                assert np.any(out)
    finally:
        hs.destroy()
    assert n_eight >= 1


def test_several_terms_orbs(gpu):
    """ed_total_ud=F: every term must be the same operator; the coefficients add in the documented order"""
    norb, nbath, nups, ndws = ORBS_CASES["g_orbs_six_axes"]
    _, pm = _orbs_models(norb, nbath)
    hs = Handles(lambda u, d: _H().orbs_from_model(pm, u, d))
    rng = np.random.default_rng(78)
    try:
        h = hs(nups, ndws)
        v = _vector(h.dim, False, 6)
        for op in ((1, 2, DW), (0, 1, UP)):
            for coefs in ((1.0, 1.0), tuple(rng.standard_normal(8))):
                ops = [op] * len(coefs)
                xs, dest = _orbs_gathers(norb, 1 + nbath, nups, ndws, ops, v)
                out = _apply(h, hs(*dest), v, ops, coefs=coefs)
                assert np.array_equal(out, real_chain(coefs, xs).reshape(-1))
                assert np.any(out)
    finally:
        hs.destroy()


@pytest.mark.parametrize("case,sec,spin", [("d_complex_small", (3, 3), UP), ("d_complex_small", (3, 3), DW),
                                           ("e_complex_rows", (5, 2), DW)])
def test_complex_coefficients(gpu, case, sec, spin):
    """edigpu_apply_cops_normal_z with [1, i] and [1, -i] (ED_GF_NORMAL.f90:250-263): bit-equal with the restated complex
    arithmetic, and within the derived bound of an extended-precision sum"""
    kind, norb, nbath, nph, _ = NORMAL_CASES[case]
    _, pm, hs = _normal_setup(kind, norb, nbath, nph)
    try:
        h = hs(*sec)
        v = _vector(h.dim, True, 33)
        for create in (0, 1):
            for coefs in ((1.0, 1j), (1.0, -1j)):
                ops = [(create, 0, spin), (create, 1, spin)]
                xs, dest = _normal_gathers(pm, sec, ops, v, 1)
                zs = [_as(v, x) for x in xs]
                out = _apply(h, hs(*dest), v, ops, coefs=coefs)
                assert not np.any(out == FILL)
                assert np.array_equal(out, cplx_chain(coefs, zs)), (case, create, coefs)
                ext = sum(np.clongdouble(c) * z.astype(np.clongdouble) for c, z in zip(coefs, zs))
                mag = sum(np.abs(np.clongdouble(c) * z.astype(np.clongdouble)) for c, z in zip(coefs, zs))
                err = np.abs(out.astype(np.clongdouble) - ext)
                assert np.all(err <= len(coefs) * U * mag)
                assert np.count_nonzero(mag) > out.size // 2
    finally:
        hs.destroy()


def _norm2(x):
    x = np.ascontiguousarray(x).view(np.float64).astype(np.longdouble)
    return float(np.sum(x * x))


def test_sum_rule_every_kind(gpu):
    """|c v|^2 + |c^+ v|^2 = |v|^2 for a normalised random v, wherever both destinations exist: phonon, complex,
    ed_total_ud=F and superc / nonsu2 phonon sectors"""
    from edipack_amd import capi
    n_checked = 0

    def check(h, dest_of, v, norb, label):
        nonlocal n_checked
        v = v / np.sqrt(_norm2(v))
        n2 = _norm2(v)
        for spin, iorb in itertools.product((UP, DW), range(norb)):
            try:
                outs = [_apply(h, dest_of(spin, iorb, create), v, [(create, iorb, spin)]) for create in (0, 1)]
            except (capi.EdigpuError, KeyError):
                continue                                   # one of the two destinations does not exist
            total = _norm2(outs[0]) + _norm2(outs[1])
            assert abs(total - n2) <= h.dim * 2.0 ** -52 * n2, (label, spin, iorb, total)
            n_checked += 1

    for case in ("c_holstein_small", "d_complex_small"):
        kind, norb, nbath, nph, sources = NORMAL_CASES[case]
        _, pm, hs = _normal_setup(kind, norb, nbath, nph)
        try:
            sec = sources[0][0]

            def dest_of(spin, iorb, create, sec=sec, hs=hs, ns=pm.ns):
                d = list(sec)
                d[spin] += 1 if create else -1
                if not 0 <= d[spin] <= ns:
                    raise KeyError
                return hs(*d)
            check(hs(*sec), dest_of, _vector(hs(*sec).dim, kind == "z", 41), norb, case)
        finally:
            hs.destroy()
    norb, nbath, nups, ndws = ORBS_CASES["g_orbs_six_axes"]
    _, pm = _orbs_models(norb, nbath)
    hs = Handles(lambda u, d: _H().orbs_from_model(pm, u, d))
    try:
        def dest_orbs(spin, iorb, create):
            occ = [list(nups), list(ndws)]
            occ[spin][iorb] += 1 if create else -1
            if not 0 <= occ[spin][iorb] <= 1 + nbath:
                raise KeyError
            return hs(tuple(occ[0]), tuple(occ[1]))
        check(hs(nups, ndws), dest_orbs, _vector(hs(nups, ndws).dim, False, 42), norb, "orbs")
    finally:
        hs.destroy()
    for mode, sector in (("superc", 0), ("nonsu2", 4)):
        _, pm = make_models(mode, "normal", 1, 3, seed=12)
        pm.nph, pm.w0_ph, pm.a_ph, pm.g_ph = 2, 0.8, 0.0, np.array([[0.3]])
        hs = Handles(lambda s, pm=pm: _H().flat_from_model(pm, s))
        try:
            def dest_flat(spin, iorb, create, mode=mode, sector=sector, hs=hs):
                d = 1 if create else -1
                return hs(sector + (d if spin == UP else -d) if mode == "superc" else sector + d)
            check(hs(sector), dest_flat, _vector(hs(sector).dim, True, 43), 1, mode)
        finally:
            hs.destroy()
    assert n_checked >= 2 + 4 + 6 + 2 + 2


# ---- end to end ------------------------------------------------------------------------------------------------------
def _ground_state(h):
    import torch
    from edipack_amd import capi
    evec = torch.empty(h.dim, dtype=torch.complex128 if h.is_complex else torch.float64, device="cuda")
    ev, nc, nmv = np.zeros(1), C.c_int(0), C.c_int(0)
    capi.check(capi.lib().edigpu_lanczos_eigh_multi(h._h, 1, 0, 1e-13, 300, None, capi.pd(ev), C.c_void_p(evec.data_ptr()),
                                                    C.byref(nc), C.byref(nmv)), "edigpu_lanczos_eigh_multi")
    return float(ev[0]), evec


def _gf_error(h, dense_of, dests, seed_ref, z):
    """max |G - G_dense| / max |G_dense| of G(z) = sum over the channels (handle, key, create, restated seed function):
    device route = ground state -> apply_op_to -> lanczos_tridiag_dev to the sector dimension -> spectral sum"""
    import torch
    e0, evec = _ground_state(h)
    w0 = np.linalg.eigvalsh(dense_of(h, "src"))
    assert abs(e0 - w0[0]) < 1e-9 and w0[1] - w0[0] > 1e-6, "the ground state must be non-degenerate"
    gs = evec.cpu().numpy()
    g, ref = np.zeros(z.size, complex), np.zeros(z.size, complex)
    for ht, key, (create, iorb, spin) in dests:
        seed = torch.full((ht.dim,), FILL, dtype=evec.dtype, device="cuda")
        h.apply_op_to(ht, evec.data_ptr(), seed.data_ptr(), iorb, spin, bool(create))
        al, bl, nit, nrm2 = ht.lanczos_tridiag_dev(seed.data_ptr(), ht.dim)
        assert nrm2 > 1e-6 and nit >= 1
        print(f"    channel {(create, iorb, spin)}: sector dimension {ht.dim}, Lanczos steps {nit}, |seed|^2 = {nrm2:.6f}")
        isign = 1 if create else -1
        t = np.diag(al[:nit]) + np.diag(bl[1:nit], 1) + np.diag(bl[1:nit], -1)
        ev, zz = np.linalg.eigh(t)
        g += np.sum((nrm2 * zz[0, :] ** 2)[None, :] / (z[:, None] - (isign * (ev - e0))[None, :]), axis=1)
        et, xt = np.linalg.eigh(dense_of(ht, key))
        sd = seed_ref(gs, (create, iorb, spin))
        assert abs(_norm2(sd) - nrm2) < 1e-12 * max(nrm2, 1.0)
        wts = np.abs(xt.conj().T @ sd) ** 2
        ref += np.sum(wts[None, :] / (z[:, None] - (isign * (et - e0))[None, :]), axis=1)
    assert np.max(np.abs(ref)) > 1e-3
    return float(np.max(np.abs(g - ref)) / np.max(np.abs(ref)))


def _dense_from_apply(h, _key=None):
    eye = np.eye(h.dim)
    hd = np.stack([h.apply(eye[:, k].copy()) for k in range(h.dim)], axis=1)
    assert np.max(np.abs(hd - hd.T)) < 1e-13
    return hd


def _gf_normal(kind, norb, nbath, nph, sec, z, seed=11):
    """G_00,up of the lowest state of sector `sec`; the dense H of every sector from the oracle"""
    from oracle import oracle as O
    om, pm, hs = _normal_setup(kind, norb, nbath, nph, seed)
    try:
        h = hs(*sec)
        dests = [(hs(sec[0] + (1 if c else -1), sec[1]), (sec[0] + (1 if c else -1), sec[1]), (c, 0, UP)) for c in (1, 0)]

        def dense_of(_h, key):
            s = sec if key == "src" else key
            return (O.HNormalCmplx if kind == "z" else O.HNormal)(om, *s).dense()

        def seed_ref(gs, op):
            (x,), _ = _normal_gathers(pm, sec, [op], gs, nph + 1)
            return _as(gs, x)
        return _gf_error(h, dense_of, dests, seed_ref, z)
    finally:
        hs.destroy()


def _gf_orbs(norb, nbath, nups, ndws, z):
    """G_00,up of the lowest state of an ed_total_ud=F sector; the dense H column by column from the handle's own apply"""
    _, pm = _orbs_models(norb, nbath)
    hs = Handles(lambda u, d: _H().orbs_from_model(pm, u, d))
    try:
        h = hs(nups, ndws)
        dests = []
        for c in (1, 0):
            u = list(nups)
            u[0] += 1 if c else -1
            dests.append((hs(tuple(u), ndws), None, (c, 0, UP)))

        def seed_ref(gs, op):
            (x,), _ = _orbs_gathers(norb, 1 + nbath, nups, ndws, [op], gs)
            return x.reshape(-1)
        return _gf_error(h, lambda hh, _k: _dense_from_apply(hh), dests, seed_ref, z)
    finally:
        hs.destroy()


def test_green_function_end_to_end(gpu):
    beta = 50.0
    z = 1j * np.pi * (2.0 * np.arange(64) + 1.0) / beta
    # the yardstick: the earlier route on the real, phonon-free models of the same Norb / Nbath
    base = {"holstein": _gf_normal("real", 1, 3, 0, (2, 2), z), "complex": _gf_normal("real", 2, 2, 0, (3, 3), z),
            "orbs": _gf_normal("real", 2, 3, 0, (2, 2), z)}
    new = {"holstein": _gf_normal("ph", 1, 3, 3, (2, 2), z), "complex": _gf_normal("z", 2, 2, 0, (3, 3), z),
           "orbs": _gf_orbs(2, 3, (2, 2), (2, 2), z)}
    for k in base:
        print(f"G(iw) end to end, {k}: earlier route rel err = {base[k]:.3e}, new sector rel err = {new[k]:.3e}")
    for k in new:
        assert new[k] <= 10 * BASELINE_E2E[k], (k, new[k], BASELINE_E2E[k])


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    import torch
    from edipack_amd import capi
    from oracle import oracle as O
    H = _H()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    a, b = buf.data_ptr(), buf.data_ptr() + (1 << 15) * 8
    om, pm, hs = _normal_setup("ph", 1, 3, 2)
    good, up = hs(2, 2), hs(3, 2)

    def refuse(src, dst, match, op=(1, 0, UP), vs=a, vd=b, who="edigpu_apply_op"):
        with pytest.raises(capi.EdigpuError, match=who + ".*" + match):
            src.apply_op_to(dst, vs, vd, op[1], op[2], bool(op[0]))

    try:
        good.apply_op_to(up, a, b, 0, UP, True)         # the served call
        # hand-over handles
        ho = O.HNormal(make_models("normal", "normal", 1, 3, seed=11)[0], 3, 2)
        hand = H.normal_from_arrays(ho.dimup, ho.dimdw, ho.hd, ho.up, ho.dw, ho.nd)
        refuse(good, hand, r"destination handle is a hand-over handle \(edigpu_normal_create\)")
        refuse(hand, good, r"source handle is a hand-over handle \(edigpu_normal_create\)")
        hand.destroy()
        omo, pmo = _orbs_models(2, 2)
        orbs, orbs_up = H.orbs_from_model(pmo, (1, 1), (1, 2)), H.orbs_from_model(pmo, (2, 1), (1, 2))
        hoo = O.HOrbs(omo, (2, 1), (1, 2))
        hand = H.orbs_from_arrays(hoo.dims, hoo.hd, hoo.fac)
        refuse(orbs, hand, r"destination handle is a hand-over handle \(edigpu_orbs_create\)")
        refuse(hand, orbs, r"source handle is a hand-over handle \(edigpu_orbs_create\)")
        hand.destroy()
        # shards
        shard = H.orbs_from_model(pmo, (2, 1), (1, 2), row_first=3, row_count=10)
        refuse(orbs, shard, "destination handle is a shard")
        refuse(shard, orbs, "source handle is a shard")
        shard.destroy()
        # handles of different kinds, models, nph
        _, pmz, hz = _normal_setup("z", 1, 3, 0)
        refuse(good, hz(3, 2), "different kinds: the source is a real normal-mode phonon sector, the destination a complex")
        refuse(hz(2, 2), up, "different kinds")
        refuse(orbs, up, "different kinds")
        _, _, hs4 = _normal_setup("ph", 1, 4, 2)
        refuse(good, hs4(3, 2), "sectors of different models")
        hs4.destroy()
        _, _, hs3 = _normal_setup("ph", 1, 3, 3)
        refuse(good, hs3(3, 2), r"different nph \(2 and 3\)")
        hs3.destroy()
        _, _, hs0 = _normal_setup("real", 1, 3, 0)
        refuse(good, hs0(3, 2), r"different nph \(2 and 0\)")
        refuse(hs0(2, 2), up, r"different nph \(0 and 2\)")
        hs0.destroy()
        # a destination that is not where the operator leads; an operator that leaves the Fock space
        refuse(good, good, r"destination handle is the sector \(2, 2\), the operators lead to \(3, 2\)")
        refuse(good, up, r"destination handle is the sector \(3, 2\), the operators lead to \(2, 1\)", op=(0, 0, DW))
        refuse(orbs, orbs, r"destination handle is the sector \(1 1 \| 1 2\), the operators lead to \(2 1 \| 1 2\)")
        refuse(orbs, orbs_up, r"the operators lead to \(1 2 \| 1 2\)", op=(1, 1, UP))
        full = hs(4, 2)
        refuse(full, full, "leaves the Fock space")
        refuse(good, up, "orbital / spin out of range", op=(1, 1, UP))
        # overlap: the destination starts inside the source, or the source inside the destination
        for vd in (a, a + 8, a + 8 * (good.dim - 1)):
            refuse(good, up, "overlaps", vd=vd)
        refuse(good, up, "overlaps", vs=a + 8 * (up.dim - 1), vd=a)
        good.apply_op_to(up, a, a + 8 * good.dim, 0, UP, True)     # next to each other: served
        # nops outside 1 .. 8 on the new routes
        with pytest.raises(capi.EdigpuError, match="edigpu_apply_cops_normal: nops must be 1 .. 8"):
            good.apply_cops_to(up, a, b, [1.0] * 9, [1] * 9, [0] * 9, [UP] * 9)
        with pytest.raises(capi.EdigpuError, match="edigpu_apply_cops_normal: the operators lead to different destination"):
            good.apply_cops_to(up, a, b, [1.0, 1.0], [1, 1], [0, 0], [UP, DW])
        # complex coefficients on anything but complex normal-mode sectors
        n = 2
        coef = (C.c_double * (2 * n))(1.0, 0.0, 0.0, 1.0)
        i32 = C.c_int32 * n
        for src, dst, what in ((good, up, "source handle is a real normal-mode phonon sector"),
                               (orbs, orbs_up, "source handle is an ed_total_ud=F sector"),
                               (hz(2, 2), up, "destination handle is a real normal-mode phonon sector")):
            rc = capi.lib().edigpu_apply_cops_normal_z(src._h, dst._h, a, b, n, coef, i32(1, 1), i32(0, 0), i32(0, 0), None)
            assert rc != 0 and "edigpu_apply_cops_normal_z: the " + what in capi.last_error()
            assert "complex coefficients are served on complex normal-mode sectors" in capi.last_error()
        rc = capi.lib().edigpu_apply_cops_normal_z(hz(2, 2)._h, hz(3, 2)._h, a, b, 9, coef, i32(1, 1), i32(0, 0), i32(0, 0), None)
        assert rc != 0 and "nops must be 1 .. 8" in capi.last_error()
        hz.destroy()
        for h in (orbs, orbs_up):
            h.destroy()
        # superc phonon sectors: the same nph on both sides
        _, ps0 = make_models("superc", "normal", 1, 3, seed=12)
        _, ps = make_models("superc", "normal", 1, 3, seed=12)
        ps.nph, ps.w0_ph, ps.a_ph, ps.g_ph = 2, 0.8, 0.0, np.array([[0.3]])
        f, f0 = H.flat_from_model(ps, 0), H.flat_from_model(ps0, 1)
        refuse(f, f0, r"different nph \(2 and 0\)")
        refuse(f, up, "superc / nonsu2")
        refuse(good, f, "destination handle is a superc / nonsu2 sector")
        f.destroy()
        f0.destroy()
    finally:
        hs.destroy()
