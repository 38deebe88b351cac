"""GPU tests of the fused two-operator products on device vectors (edigpu_apply_pairs_normal): the seeds of the pair and
exciton susceptibilities.

References are numpy on the host from the sector maps, applying the operators forwards state by state
(tests/pairs_cases.py), and the library's own earlier path: two apply_op_to calls through a built intermediate sector.

What "bit-equal" means here.  An element is acc = 0, then acc = fma(coef_t, +-x_t, acc) for t ascending.  With
coef = +-1 every product is exact, so the numpy sum acc + coef * x in the same order has the same bits, zeros included
(an element without a preimage is +0.0), and the comparison is on the 64-bit patterns.  The chain of two single
operators and apply_occ produce a NEGATIVE zero where a sign meets an empty intermediate element (-(0.0), x * 0.0 with
x < 0); against those two the comparison is on the patterns after adding +0.0, which changes nothing but the sign of a
zero.

With 8 random coefficients the bound is derived, not measured: each fma rounds once, so after n terms
|err_i| <= ((1 + u)^n - 1) sum_t |coef_t x_t| <= 2 n u sum_t |coef_t x_t|, u = 2^-53; the reference is summed in extended
precision.

Single terms: all 16 (kind, spin) combinations with coef = +-1 on the Ns = 6 sectors; the larger sectors take the six
combinations that cover every kind and every spin pattern (each further destination is two more handles to build)."""
import ctypes as C

import numpy as np
import pytest

from tests.common import make_models
from tests.pairs_cases import U, destination, get_chiab, numpy_pairs
from tests.ph_cases import set_phonons

pytestmark = pytest.mark.gpu

GUARD = 3.25
UP, DW = 0, 1

# (create1, create2) of O2 O1: cc, c+c+, c+c (O1 = c), cc+ (O1 = c+); the two operators sit on different orbitals (1, 0)
KINDS = {"cc": (0, 0), "c+c+": (1, 1), "c+c": (0, 1), "cc+": (1, 0)}
SPINS = {"uu": (UP, UP), "dd": (DW, DW), "ud": (UP, DW), "du": (DW, UP)}   # spins of (O1, O2)
ALL16 = [(k, s) for k in KINDS for s in SPINS]
SIX = [("cc", "du"), ("c+c+", "ud"), ("c+c", "uu"), ("cc+", "dd"), ("c+c", "ud"), ("cc", "uu")]


def _term(kind, spins, coef=1.0, orbs=(1, 0)):
    (c1, c2), (s1, s2) = KINDS[kind], SPINS[spins]
    return (coef, (c1, orbs[0], s1), (c2, orbs[1], s2))


def _H():
    from edipack_amd.hamiltonian import SectorHamiltonian
    return SectorHamiltonian


class Handles:
    """the sector handles of one model, built on demand and destroyed together"""

    def __init__(self, pm):
        self.pm, self.h = pm, {}

    def __call__(self, nup, ndw):
        if (nup, ndw) not in self.h:
            self.h[(nup, ndw)] = _H().normal_from_model(self.pm, nup, ndw)
        return self.h[(nup, ndw)]

    def destroy(self):
        for h in self.h.values():
            h.destroy()
        self.h = {}


def _buffers(nsrc, ndst, v, odd=False):
    """one device buffer | guard | src | guard | dst (filled with 7.0) | guard |; odd: both vectors start 8 bytes past a
    16-byte boundary"""
    import torch
    g = 3 if odd else 2
    pad = (nsrc + g) % 2 if odd else nsrc % 2     # keeps dst on the same 16-byte phase as src
    buf = torch.full((3 * g + nsrc + pad + ndst,), GUARD, dtype=torch.float64, device="cuda")
    src = buf[g:g + nsrc]
    d0 = 2 * g + nsrc + pad
    dst = buf[d0:d0 + ndst]
    want = 8 if odd else 0
    assert src.data_ptr() % 16 == want and dst.data_ptr() % 16 == want
    src.copy_(torch.from_numpy(v))
    dst.fill_(7.0)
    return buf, src, dst, [buf[:g], buf[g + nsrc:d0], buf[d0 + ndst:]]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _bits_mod_zero_sign(a):
    return _bits(np.asarray(a, dtype=np.float64) + 0.0)


def _run(hs, src_sec, terms, v, odd=False, chain=True):
    """apply_pairs_to on one set of terms with every check that needs no second opinion; returns the result"""
    import torch
    pm = hs.pm
    nblk = pm.nph + 1
    nu, nd, ok = destination(*src_sec, pm.ns, terms[0])
    assert ok
    h_src, h_dst = hs(*src_sec), hs(nu, nd)
    buf, src, dst, guards = _buffers(h_src.dim, h_dst.dim, v, odd)
    h_src.apply_pairs_to(h_dst, src.data_ptr(), dst.data_ptr(), terms, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert np.array_equal(_bits(src.cpu().numpy()), _bits(v)), "source touched"
    assert not np.any(out == 7.0), "an element of the destination was not written"
    assert all(bool((g == GUARD).all().item()) for g in guards), "write outside the destination"
    if all(abs(t[0]) == 1.0 for t in terms):
        ref = numpy_pairs(pm, src_sec, terms, v, nblk)
        assert np.array_equal(_bits(out), _bits(ref)), (src_sec, terms)
    if chain and len(terms) == 1 and nblk == 1:
        # the earlier device path: O1 into a built intermediate sector, O2 from there
        coef, o1, o2 = terms[0]
        mid = list(src_sec)
        mid[o1[2]] += 1 if o1[0] else -1
        h_mid = hs(*mid)
        tmp = torch.full((h_mid.dim,), 5.0, dtype=torch.float64, device="cuda")
        res = torch.full((h_dst.dim,), 5.0, dtype=torch.float64, device="cuda")
        h_src.apply_op_to(h_mid, src.data_ptr(), tmp.data_ptr(), o1[1], o1[2], bool(o1[0]))
        h_mid.apply_op_to(h_dst, tmp.data_ptr(), res.data_ptr(), o2[1], o2[2], bool(o2[0]))
        torch.cuda.synchronize()
        assert np.array_equal(_bits_mod_zero_sign(out), _bits_mod_zero_sign(coef * res.cpu().numpy())), (src_sec, terms)
    return out


def _vector(dim, seed):
    return np.random.default_rng(seed).standard_normal(dim)


SECTORS = [
    # bath, norb, nbath, source sector, nph, combinations
    ("normal", 2, 2, (3, 3), 0, ALL16),    # 20 x 20, base case
    ("normal", 2, 2, (1, 4), 0, ALL16),    # 6 x 15: rows shorter than a wave (flat kernel)
    ("normal", 2, 2, (2, 2), 0, ALL16),    # 15 x 15: odd dimension
    ("normal", 3, 3, (6, 1), 0, SIX),      # 924 x 12: long rows
    ("normal", 3, 3, (1, 6), 0, SIX),      # 12 x 924: many short rows
    ("normal", 3, 3, (6, 6), 0, SIX),      # 924^2: 8 chunks per row, more units than the grid takes at once (grid stride)
    ("hybrid", 5, 3, (4, 4), 0, SIX),      # 70 x 70, five orbitals: first row length of the rows kernel
    ("hybrid", 5, 3, (3, 3), 0, SIX),      # 56 x 56: last row length of the flat kernel
    ("normal", 2, 2, (3, 3), 2, ALL16),    # phonon blocks
    # 25 blocks of 12 x 924 onto themselves: more elements (277 200) than the flat kernel's grid takes at once (262 144)
    ("normal", 3, 3, (1, 6), 24, SIX[2:4]),
]


@pytest.mark.parametrize("bath,norb,nbath,sec,nph,combos", SECTORS)
def test_single_terms(gpu, bath, norb, nbath, sec, nph, combos):
    _, pm = make_models("normal", bath, norb, nbath, seed=11)
    if nph:
        set_phonons(pm, nph)
    hs = Handles(pm)
    orbs = (1, 0) if norb == 2 else (norb - 1, 0)
    n_run = 0
    try:
        v = _vector(hs(*sec).dim, 100 + sum(sec))
        for kind, spins in combos:
            for coef in (1.0, -1.0):
                term = _term(kind, spins, coef, orbs)
                if not destination(*sec, pm.ns, term)[2]:
                    continue
                _run(hs, sec, [term], v)
                n_run += 1
    finally:
        hs.destroy()
    assert n_run >= len(combos)     # at most the combinations that leave the Fock space were skipped


def test_dimension_one_destinations(gpu):
    """(1, 1) -> (0, 0) by c_up c_dw and (5, 5) -> (6, 6) by c+_dw c+_up: one element"""
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    hs = Handles(pm)
    try:
        for sec, term, dest in (((1, 1), (1.0, (0, 0, DW), (0, 0, UP)), (0, 0)), ((5, 5), (-1.0, (1, 1, UP), (1, 1, DW)), (6, 6))):
            assert destination(*sec, pm.ns, term) == (*dest, True) and hs(*dest).dim == 1
            out = _run(hs, sec, [term], _vector(hs(*sec).dim, 7))
            assert out.shape == (1,) and out[0] != 0.0
    finally:
        hs.destroy()


def test_operator_identities(gpu):
    import torch
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    hs = Handles(pm)
    try:
        sec = (3, 3)
        h = hs(*sec)
        v = _vector(h.dim, 21)
        for a in (0, 1):
            for s in (UP, DW):
                # c+_{a,s} c_{a,s} = n_{a,s}: apply_occ with the one-hot weight
                out = _run(hs, sec, [(1.0, (0, a, s), (1, a, s))], v)
                w = np.zeros(2)
                w[a] = 1.0
                src = torch.from_numpy(v).cuda()
                occ = torch.empty_like(src)
                h.apply_occ(src.data_ptr(), occ.data_ptr(), w if s == UP else 0 * w, w if s == DW else 0 * w)
                torch.cuda.synchronize()
                assert np.array_equal(_bits_mod_zero_sign(out), _bits_mod_zero_sign(occ.cpu().numpy()))
                assert np.count_nonzero(out) == h.dim // 2
                # the same level emptied or filled twice: all zeros, written
                for create in (0, 1):
                    assert not np.any(_run(hs, sec, [(1.0, (create, a, s), (create, a, s))], v))
        # two different operators of one spin anticommute: the swapped product is the exact negative
        for kind in KINDS:
            for spins in ("uu", "dd"):
                (c1, c2), (s1, _) = KINDS[kind], SPINS[spins]
                t12, t21 = (1.0, (c1, 1, s1), (c2, 0, s1)), (1.0, (c2, 0, s1), (c1, 1, s1))
                o12, o21 = _run(hs, sec, [t12], v), _run(hs, sec, [t21], v)
                assert np.array_equal(_bits_mod_zero_sign(o12), _bits_mod_zero_sign(-o21)) and np.any(o12)
    finally:
        hs.destroy()


def _all_seeds():
    from edipack_amd.observables import exct_chi_seeds, pair_chi_seeds
    return ([("pair00", c) for c in pair_chi_seeds(0, 0)] + [("pair01", c) for c in pair_chi_seeds(0, 1)] +
            [(f"exct{i}", c) for i in (1, 2, 3) for c in exct_chi_seeds(i, 0, 1)])


@pytest.mark.parametrize("bath,norb,nbath,sec,nph", [("normal", 2, 2, (3, 3), 0), ("normal", 3, 3, (6, 6), 0),
                                                     ("normal", 2, 2, (3, 3), 2), ("normal", 2, 2, (1, 4), 0)])
def test_susceptibility_seeds_bit_equal(gpu, bath, norb, nbath, sec, nph):
    """all pair and exciton seeds at (iorb, jorb) = (0, 1): coefficients +-1, so the documented fma order is reproducible"""
    _, pm = make_models("normal", bath, norb, nbath, seed=11)
    if nph:
        set_phonons(pm, nph)
    hs = Handles(pm)
    try:
        v = _vector(hs(*sec).dim, 31)
        seeds = _all_seeds()
        assert len(seeds) == 2 + 2 + 2 + 4 + 2
        two_term = 0
        for _, (terms, isign) in seeds:
            assert isign in (+1, -1)
            out = _run(hs, sec, terms, v)
            assert np.any(out)
            two_term += len(terms) == 2
        assert two_term == 6
    finally:
        hs.destroy()


@pytest.mark.parametrize("sec,nph", [((3, 3), 0), ((1, 4), 0), ((3, 3), 2)])
def test_eight_random_coefficients_within_the_derived_bound(gpu, sec, nph):
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    if nph:
        set_phonons(pm, nph)
    hs = Handles(pm)
    try:
        rng = np.random.default_rng(77)
        terms = [(float(rng.standard_normal()), (0, b, s), (1, a, s)) for a in (0, 1) for b in (0, 1) for s in (UP, DW)]
        assert len(terms) == 8
        v = _vector(hs(*sec).dim, 32)
        out = _run(hs, sec, terms, v)
        # extended-precision reference: every term on its own (exact with coefficient 1), then the weighted sum
        ref = np.zeros(out.size, dtype=np.longdouble)
        mag = np.zeros(out.size, dtype=np.longdouble)
        for coef, o1, o2 in terms:
            x = numpy_pairs(pm, sec, [(1.0, o1, o2)], v, pm.nph + 1).astype(np.longdouble)
            ref += np.longdouble(coef) * x
            mag += np.abs(np.longdouble(coef) * x)
        err = np.abs(out.astype(np.longdouble) - ref)
        bound = 2 * len(terms) * U * mag
        print(f"8 random terms on {sec} nph={nph}: max err / bound = {float(np.max(err / np.maximum(bound, 1e-300))):.3f}")
        assert np.all(err <= bound)
        assert np.count_nonzero(mag) > out.size // 2
    finally:
        hs.destroy()


def test_vectors_at_odd_offsets(gpu):
    """source and destination 8 bytes past a 16-byte boundary, rows kernel and flat kernel"""
    from edipack_amd.observables import exct_chi_seeds, pair_chi_seeds
    for bath, norb, nbath, sec in (("normal", 2, 2, (2, 2)), ("hybrid", 5, 3, (4, 4))):
        _, pm = make_models("normal", bath, norb, nbath, seed=11)
        hs = Handles(pm)
        try:
            v = _vector(hs(*sec).dim, 41)
            for terms in (pair_chi_seeds(0, 1)[0][0], exct_chi_seeds(3, 0, 1)[1][0], exct_chi_seeds(2, 0, 1)[2][0]):
                _run(hs, sec, terms, v, odd=True)
        finally:
            hs.destroy()


def test_refusals(gpu):
    import torch
    from edipack_amd import capi
    from edipack_amd.hamiltonian import pairs_sector
    from oracle import oracle as O
    H = _H()
    buf = torch.zeros(8192, dtype=torch.float64, device="cuda")
    a, b = buf.data_ptr(), buf.data_ptr() + 4096 * 8
    same = [(1.0, (0, 1, UP), (1, 0, UP))]           # (3, 3) -> (3, 3)
    om, pm = make_models("normal", "normal", 2, 2, seed=11)
    good = H.normal_from_model(pm, 3, 3)

    def refuse(src, dst, match, terms=same, vs=a, vd=b):
        with pytest.raises(capi.EdigpuError, match="edigpu_apply_pairs_normal: .*" + match):
            src.apply_pairs_to(dst, vs, vd, terms)

    def refuse_both_ways(h, match):
        refuse(h, good, "source handle " + match)
        refuse(good, h, "destination handle " + match)
        h.destroy()

    refuse_both_ways(H.normal_cmplx_from_model(pm, 3, 3), "is a complex normal-mode sector")
    _, ps = make_models("superc", "hybrid", 2, 3, seed=12)
    refuse_both_ways(H.flat_from_model(ps, 0), "is a superc / nonsu2 sector")
    _, pn = make_models("nonsu2", "normal", 1, 4, seed=12)
    refuse_both_ways(H.flat_from_model(pn, 3), "is a superc / nonsu2 sector")
    om0, pm0 = make_models("normal", "normal", 2, 2, seed=11, jxp=0.0)
    hl = np.zeros_like(om0.hloc)
    for k in range(2):
        hl[0, 0, k, k] = om0.hloc[0, 0, k, k].real
    pm0.hloc = hl                                    # what ed_total_ud=F requires
    refuse_both_ways(H.orbs_from_model(pm0, (2, 1), (1, 2)), "is an ed_total_ud=F sector")
    ho = O.HNormal(om, 3, 3)
    refuse_both_ways(H.normal_from_arrays(ho.dimup, ho.dimdw, ho.hd, ho.up, ho.dw, ho.nd), "must be built from a model")
    refuse_both_ways(H.normal_from_model(pm, 3, 3, dw_first=2, dw_count=5), "must hold the whole sector")
    # sectors of different models: another bath size, and a phonon sector against a plain one
    _, pm3 = make_models("normal", "normal", 2, 3, seed=11)
    other = H.normal_from_model(pm3, 3, 3)
    refuse(good, other, "sectors of different models")
    other.destroy()
    _, pmp = make_models("normal", "normal", 2, 2, seed=11)
    set_phonons(pmp, 2)
    other = H.normal_from_model(pmp, 3, 3)
    refuse(good, other, "sectors of different models")
    other.destroy()
    # a destination that is not where the terms lead, terms that disagree, too many terms, no destination at all
    lower = H.normal_from_model(pm, 2, 2)
    refuse(good, lower, r"destination handle is the sector \(2, 2\), the terms lead to \(3, 3\)")
    refuse(good, good, r"destination handle is the sector \(3, 3\), the terms lead to \(2, 2\)", terms=[(1.0, (0, 0, DW), (0, 0, UP))])
    refuse(good, good, "the terms lead to different destination sectors", terms=same + [(1.0, (0, 0, DW), (0, 0, UP))])
    refuse(good, good, "nterms must be 1 .. 8", terms=same * 9)
    refuse(good, good, "nterms must be 1 .. 8", terms=[])
    refuse(good, good, "orbital / spin out of range", terms=[(1.0, (0, 2, UP), (1, 0, UP))])
    empty = H.normal_from_model(pm, 0, 3)
    gone = [(1.0, (0, 1, UP), (1, 0, UP))]
    assert pairs_sector(pm, 0, 3, gone) == (0, 3, False)
    refuse(empty, empty, "leaves the Fock space", terms=gone)
    empty.destroy()
    lower.destroy()
    # overlap: the destination starts inside the source, or the source inside the destination
    for vd in (a, a + 8, a + 8 * (good.dim - 1)):
        refuse(good, good, "overlaps", vd=vd)
    refuse(good, good, "overlaps", vs=a + 8 * (good.dim - 1), vd=a)
    # and the vectors next to each other are served
    v = _vector(good.dim, 3)
    buf[:good.dim].copy_(torch.from_numpy(v))
    good.apply_pairs_to(good, a, a + 8 * good.dim, same)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf[good.dim:2 * good.dim].cpu().numpy()), _bits(numpy_pairs(pm, (3, 3), same, v)))
    good.destroy()


def test_pair_and_exciton_chi_end_to_end(gpu):
    """chi_pair(0,0), the auxiliary chi_pair(0,1), chi_exct triplet-XY (0,1) and singlet (0,1) (with its mirror) of the
    ground state on 8 Matsubara frequencies, eigenvector -> seed -> tridiagonalisation all on the device, against the
    dense spectral sum with the same get_Chiab formula"""
    import torch
    from edipack_amd import capi
    from edipack_amd.observables import chi_channel, exct_chi_seeds, pair_chi_seeds
    _, pm = make_models("normal", "normal", 2, 2, seed=11)
    hs = Handles(pm)
    try:
        sec = (3, 3)
        h = hs(*sec)
        assert h.dim == 400

        def dense(hh):
            eye = np.eye(hh.dim)
            Hd = np.stack([hh.apply(eye[:, k].copy()) for k in range(hh.dim)], axis=1)
            assert np.max(np.abs(Hd - Hd.T)) < 1e-13
            return np.linalg.eigh(Hd)

        spectra = {sec: dense(h)}
        e = spectra[sec][0]
        assert e[1] - e[0] > 1e-6, "the ground state must be non-degenerate"
        evec = torch.empty(h.dim, dtype=torch.float64, device="cuda")
        ev, nc, nmv = np.zeros(1), C.c_int(0), C.c_int(0)
        capi.check(capi.lib().edigpu_lanczos_eigh_multi(h._h, 1, 0, 1e-13, 300, None, capi.pd(ev), C.c_void_p(evec.data_ptr()),
                                                        C.byref(nc), C.byref(nmv)), "edigpu_lanczos_eigh_multi")
        assert abs(ev[0] - e[0]) < 1e-10
        gs = evec.cpu().numpy()
        beta = 50.0
        z = 1j * 2.0 * np.pi * np.arange(8) / beta
        cases = [("pair(0,0)", pair_chi_seeds(0, 0)), ("pair(0,1) auxiliary", pair_chi_seeds(0, 1)),
                 ("exct XY(0,1)", exct_chi_seeds(2, 0, 1)), ("exct S(0,1)", exct_chi_seeds(1, 0, 1))]
        for name, channels in cases:
            chi, chim = np.zeros(z.size, complex), np.zeros(z.size, complex)
            ref, refm = np.zeros(z.size, complex), np.zeros(z.size, complex)
            for ichan, (terms, isign) in enumerate(channels, start=1):
                nu, nd, ok = destination(*sec, pm.ns, terms[0])
                assert ok
                ht = hs(nu, nd)
                seed = torch.full((ht.dim,), 7.0, dtype=torch.float64, device="cuda")
                h.apply_pairs_to(ht, evec.data_ptr(), seed.data_ptr(), terms, torch.cuda.current_stream().cuda_stream)
                al, bl, nit, nrm2 = ht.lanczos_tridiag_dev(seed.data_ptr(), ht.dim)
                assert nrm2 > 1e-6
                c, cm = chi_channel(al[:nit], bl[:nit], nrm2, ev[0], isign, ichan, z, beta, mirror=True)
                chi += c
                chim += cm
                # dense: weights |<j|seed>|^2 with the numpy seed of the device eigenvector, poles isign (E_j - E_0)
                if (nu, nd) not in spectra:
                    spectra[(nu, nd)] = dense(ht)
                et, xt = spectra[(nu, nd)]
                sd = numpy_pairs(pm, sec, terms, gs)
                assert abs(float(sd @ sd) - nrm2) < 1e-12 * max(nrm2, 1.0)
                r, rm = get_chiab((xt.T @ sd) ** 2, isign * (et - ev[0]), ichan, z, beta)
                ref += r
                refm += rm
            err = np.max(np.abs(chi - ref)) / np.max(np.abs(ref))
            errm = np.max(np.abs(chim - refm)) / np.max(np.abs(refm))
            print(f"{name}: max|chi|={np.max(np.abs(ref)):.6e} rel err={err:.3e} mirror rel err={errm:.3e}")
            assert np.max(np.abs(ref)) > 1e-3
            assert err < 1e-9 and errm < 1e-9
    finally:
        hs.destroy()
