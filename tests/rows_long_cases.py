"""Sectors and synthetic operators with rows of 2048 to 4097 columns: the one list that tests/test_gpu_rows_long.py
(the LDS rows kernel on them) and tests/test_host_pack.py (the 16-bit image they get, or do not get) both read."""
from types import SimpleNamespace

import numpy as np

MODEL_SEED = 31
SECTORS = [
    # bath, norb, nbath, (nup, ndw): Ns = 14, make_models("normal", bath, norb, nbath, seed=MODEL_SEED)
    ("normal", 2, 6, (7, 1)),    # 3432 x 14: even DimUp (16-byte accesses), Hnd terms
    ("normal", 2, 6, (6, 1)),    # 3003 x 14: odd DimUp (the scalar access path), Hnd terms
    ("normal", 1, 13, (6, 13)),  # 3003 x 14: one orbital, no Hnd: the hand-over image is fusable however it is factored
]
# The short-row pairing (rows kernel in position order) at config 2's row length, with the chunk rows of the block image
# (EDIGPU_IB_ROWS).  3432 x 91 has no block image at 24 rows per chunk (its 21-row runs of down rows leave 7 bath levels
# outside a chunk, the image holds 6: tests/test_host_ib.py); the nearest sector of this DimUp that has one is 3432 x 14.
POS_CASES = [
    (("normal", 2, 6, (7, 2)), 480),
    (("normal", 2, 6, (7, 1)), 24),
]

# DimUp of the synthetic operators: 2048 the last size with one keep-P pass, 2049 / 2050 one column / one double2 in the
# second, 4094 / 4095 the largest (even) sizes of the 16-bit image (dead-slot offset 32760), 4096 / 4097 the 32-bit image only
SYNTH_DIMUP = [2048, 2049, 2050, 4094, 4095, 4096, 4097]
SYNTH_DIMDW = 5
RING = ((1, 0.7), (7, 0.3), (1031, 1.9))   # (|offset|, amplitude): each amplitude twice in a row, typed width 6


def ring_hup(n):
    """Symmetric ring stencil as CSR with sorted columns: entries (i, (i +- o) mod n) of amplitude a(o), sign -1 where
    (i + j) % 3 == 0 -- symmetric in i and j, so the first and last rows reach the last and first columns with both signs."""
    i = np.arange(n)
    col = np.stack([(i + s * o) % n for o, _ in RING for s in (1, -1)], axis=1)
    amp = np.array([a for _, a in RING for _ in (1, -1)])
    val = np.where((i[:, None] + col) % 3 == 0, -amp, amp)
    order = np.argsort(col, axis=1)
    col, val = np.take_along_axis(col, order, 1), np.take_along_axis(val, order, 1)
    assert (np.diff(col, axis=1) > 0).all()      # six distinct columns per row
    return np.arange(n + 1, dtype=np.int64) * col.shape[1], col.ravel().astype(np.int32), val.ravel().astype(np.float64)


def synth_operator(n):
    """hd o v + (1 (x) Hup) v + (Hdw (x) 1) v with Hup = ring_hup(n), a dense symmetric random Hdw (5 x 5), a random hd
    and no Hnd, in the attributes the hand-over takes (those of oracle.HNormal)."""
    rng = np.random.default_rng(5000 + n)
    d = SYNTH_DIMDW
    a = rng.standard_normal((d, d))
    hdw = a + a.T
    dw = (np.arange(d + 1, dtype=np.int64) * d, np.tile(np.arange(d, dtype=np.int32), d), hdw.ravel().copy())
    return SimpleNamespace(dimup=n, dimdw=d, dim=n * d, hd=rng.standard_normal(n * d), up=ring_hup(n), dw=dw, hdw=hdw,
                           has_nd=False, nd=None)


def synth_matvec(op, v, dtype=np.float64):
    """(y, |Hd||v| + |Hup||v| + |Hdw||v|) of a synthetic operator in `dtype`; vectors are V[idw][iup], iup contiguous."""
    n, d = op.dimup, op.dimdw
    w = op.up[0][1]
    col, val = op.up[1].reshape(n, w), op.up[2].reshape(n, w).astype(dtype)
    x = np.asarray(v, dtype).reshape(d, n)
    hd, hdw = op.hd.astype(dtype).reshape(d, n), op.hdw.astype(dtype)
    y = hd * x + (x[:, col] * val).sum(axis=-1) + hdw @ x
    mag = abs(hd) * abs(x) + (abs(x)[:, col] * abs(val)).sum(axis=-1) + abs(hdw) @ abs(x)
    return y.ravel(), mag.ravel()
