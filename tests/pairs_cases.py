"""Shared helpers of the two-operator product tests (tests/test_pairs_host.py, tests/test_gpu_pairs.py): a numpy
restatement that applies the operators state by state, forwards, on the words of the sector maps -- the library's tables
are built backwards from the destination, so the two share no code and no direction."""
from __future__ import annotations

import itertools

import numpy as np

NONE = 0xFFFFFFFF
U = 2.0 ** -53

# every (create, iorb, ispin) of a two-orbital model
OPS2 = [(c, a, s) for c in (0, 1) for a in (0, 1) for s in (0, 1)]
ORDERED_PAIRS2 = list(itertools.product(OPS2, OPS2))


def apply_ops_word(word: int, ops):
    """(word', sign) of the operators applied in order to one species' word, or None when one of them gives zero; the
    sign of an operator is (-1)^(electrons of that species below its level) on the word it acts on"""
    sign = 1
    for create, iorb, _ in ops:
        bit = 1 << iorb
        if bool(word & bit) == bool(create):
            return None
        if bin(word & (bit - 1)).count("1") & 1:
            sign = -sign
        word ^= bit
    return word, sign


def species_table(map_src, map_dst, term, spin):
    """preimage table over the destination's index of one species (entry: source index | minus << 31, NONE), or None
    when the term has no operator of that spin"""
    ops = [o for o in term[1:] if o[2] == spin]
    if not ops:
        return None
    pos = {int(w): j for j, w in enumerate(map_dst)}
    tab = np.full(len(map_dst), NONE, dtype=np.uint32)
    for i, w in enumerate(map_src):
        r = apply_ops_word(int(w), ops)
        if r is not None:
            tab[pos[r[0]]] = i | (0x80000000 if r[1] < 0 else 0)
    return tab


def destination(nup, ndw, ns, term):
    """(nup', ndw', exists): exists is False when a particle number leaves [0, ns] after either operator"""
    n = [nup, ndw]
    ok = True
    for create, _, spin in term[1:]:
        n[spin] += 1 if create else -1
        ok = ok and 0 <= n[spin] <= ns
    return n[0], n[1], ok


def maps_of(pm, nup, ndw):
    from edipack_amd.hamiltonian import sector_map
    return sector_map(pm, nup, ndw, 0), sector_map(pm, nup, ndw, 1)


def term_parts(pm, src_sec, term):
    """(sign * picked source elements as a function of v, live mask) ingredients of one term: index arrays and signs
    over the destination, or None when the destination does not exist"""
    nu, nd, ok = destination(*src_sec, pm.ns, term)
    if not ok:
        return None
    mus, mds = maps_of(pm, *src_sec)
    mud, mdd = maps_of(pm, nu, nd)
    tu, td = species_table(mus, mud, term, 0), species_table(mds, mdd, term, 1)
    if tu is None:
        tu = np.arange(mud.size, dtype=np.uint32)
    if td is None:
        td = np.arange(mdd.size, dtype=np.uint32)
    return (nu, nd), tu, td


def numpy_pairs(pm, src_sec, terms, v, nblk=1, each=False):
    """dst = sum_t coef_t O2_t O1_t v in the kernel's documented order: acc = 0, then for t ascending
    acc = acc + coef_t * (+-x_t) on the elements where term t has a preimage.  With exact products (coef = +-1) this
    is the fma chain bit for bit.  each=True also returns sum_t |coef_t x_t| for the error bound."""
    (nu, nd), _, _ = term_parts(pm, src_sec, terms[0])
    mus, mds = maps_of(pm, *src_sec)
    V = np.asarray(v, dtype=np.float64).reshape(nblk, mds.size, mus.size)
    acc, mag = None, None
    for term in terms:
        dest, tu, td = term_parts(pm, src_sec, term)
        assert dest == (nu, nd)
        if acc is None:
            acc = np.zeros((nblk, td.size, tu.size))
            mag = np.zeros_like(acc)
        live = (td != NONE)[:, None] & (tu != NONE)[None, :]
        iu, idw = (tu & 0x7FFFFFFF).astype(np.int64), (td & 0x7FFFFFFF).astype(np.int64)
        iu[tu == NONE] = 0
        idw[td == NONE] = 0
        minus = ((td >> 31) & 1)[:, None] ^ ((tu >> 31) & 1)[None, :]
        x = V[:, idw][:, :, iu]
        x = np.where(minus.astype(bool)[None], -x, x)
        acc = np.where(live[None], acc + float(term[0]) * x, acc)
        mag = np.where(live[None], mag + np.abs(float(term[0]) * x), mag)
    return (acc.reshape(-1), mag.reshape(-1)) if each else acc.reshape(-1)


def get_chiab(peso, de, ichan, z, beta, axis="m"):
    """loop-by-loop restatement of get_Chiab (ED_CHI_EXCT.f90:427-506) for one channel's poles: returns the shares in
    Chi(iorb, jorb, :) and in Chi(jorb, iorb, :)"""
    chi = np.zeros(len(z), complex)
    chim = np.zeros(len(z), complex)
    for iexc in range(len(peso)):
        p, d = peso[iexc], de[iexc]
        if abs(beta * d) < 1e-8:
            for i in range(len(z)):
                hit = abs(z[i]) < 1e-10 if axis == "m" else abs(z[i].real) < 1e-10
                if hit:
                    chi[i] = chi[i] + 0.5 * p * beta
                    chim[i] = chim[i] + 0.5 * p * beta
        elif (d if ichan % 2 == 1 else -d) > 0:
            for i in range(len(z)):
                if ichan % 2 == 1:
                    chi[i] = chi[i] - p * (1.0 - np.exp(-beta * d)) / (z[i] - d)
                    chim[i] = chim[i] + p * (1.0 - np.exp(-beta * d)) / (z[i] + d)
                else:
                    chi[i] = chi[i] + p * (1.0 - np.exp(beta * d)) / (z[i] - d)
                    chim[i] = chim[i] - p * (1.0 - np.exp(beta * d)) / (z[i] + d)
    return chi, chim
