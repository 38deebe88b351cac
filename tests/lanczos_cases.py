"""Case tables, hook wrappers and NumPy references of tests/test_gpu_lanczos_kernels.py: the vector kernels of the
three-term recurrence (csrc/kernels_lanczos.hip, csrc/kernels_shard.hip, csrc/kernels_multi.hip) driven one launcher at
a time through the edigpu_lzk_* test hooks, and the public edigpu_vec_* / edigpu_transpose_* functions on torch tensors.

Where the grid-stride loops change behaviour (every kernel runs workgroups of 256 threads), read off the launchers:
  * red_grid, sh_grid(n, kRedBlocks), k_sumsq_multi per column: 1024 workgroups, one trip holds 262 144 doubles;
  * vec_add_dot2 / vec_unpack_add_dot2: 512 workgroups (their two planes of partials share 1024 doubles), 131 072;
  * ew_grid, sh_grid(n, 4096): 4096 workgroups, 1 048 576 doubles;
  * mu_grid: 4096 workgroups; k_interleave / k_deinterleave walk nrow * W elements, the scale and rotate kernels
    nrow * W * EL / 2 chunks of 16 bytes, so the second trip starts at 1 048 576 / W + 1 and 2 097 152 / (W EL) + 1 rows;
  * k_to_blocked / k_from_blocked: 65 536 workgroups.  That cap only wraps past 16.7 M elements (134 MB per buffer) and
    is left out.

The references never touch the device.  Sums whose order of additions is fixed by the code are restated in that order
(block_partials, strided_tree_sum) and compared bit for bit; the same sums are also held to a long-double sum of the
same terms within BOUND_ULPS * EPS * sum |terms| (the summation depth of these kernels at the sizes here is under 32
additions: at most 5 strided trips, 6 shuffle steps, 4 waves, 1 strided trip of the finalizing workgroup, 10 tree steps).
"""
import ctypes as C

import numpy as np

EPS = 2.0 ** -53
BOUND_ULPS = 64
NT = 256                       # threads per workgroup of the vector kernels
RED = 1024                     # kRedBlocks
EW = 4096                      # cap of the elementwise grids
FIN = 1024                     # threads of the finalizing workgroup
SC_ALPHA, SC_BETA, SC_STOP, SC_NDONE, SC_NORM, SC_THR, SC_EXACT, SC_AB = 0, 1, 2, 3, 4, 5, 6, 8
NLANC = 6
NSCAL = SC_AB + 2 * NLANC
TAIL = 5

SMALL_N = (1, 63, 64, 65, 255, 256, 257, 1000)
RED_N = (262144, 262145, 524289)            # exactly one trip of 1024 workgroups, one element more, two trips and one
RED2_N = (131072, 131073)                   # the same of 512 workgroups
EW_N = (1048577,)                           # one element in the second trip of 4096 workgroups
REDUCE_LENGTHS = SMALL_N + RED_N
ELEMENTWISE_LENGTHS = SMALL_N + (262145,) + EW_N
WIDTHS = ((2, 1), (4, 1), (8, 1), (2, 2), (4, 2), (8, 2))     # (W, EL)
NP_CASES = (1, 3, 1023, 1024, 1025)

# (world, du, nrows, q, halo) of test_transposed_fused_vector_kernels (tests/test_gpu_parity.py) ...
EXCHANGE_SMALL = ((1, 10, 4, 4, 0), (2, 11, 3, 5, 2), (3, 20, 7, 7, 3), (5, 9, 2, 2, 1), (7, 10, 3, 3, 3), (4, 924, 231, 231, 2))
# ... one whose nrows * du = 262 905 puts the index arithmetic into the second trip of the 1024- and 512-workgroup
# reductions, and one of 1 049 558 elements for the second trip of the 4096-workgroup rotate
EXCHANGE_RED = (4, 1031, 255, 256, 2)
EXCHANGE_EW = (4, 1031, 1018, 1018, 2)

# (dim_up, dim_dw, shift): dim_up no multiple of the panel, smaller than one panel, 1; dim_dw 1 and 7
BLOCKED_CASES = tuple((du, dd, sh) for sh in (2, 5, 7) for du in (1, (1 << sh) - 1, (1 << sh), (1 << sh) + 1, 3 * (1 << sh) + 5, 1000)
                      for dd in (1, 7))


def pcol_of(world, du):
    return -(-du // world)


def mu_rows_below(W, EL):
    """a row count per (W, EL) inside the first trip: odd, more than one workgroup"""
    return 1000 // W + 3


def mu_rows_second_trip_chunks(W, EL):
    """smallest row count that puts one 16-byte chunk of the scale / rotate kernels into mu_grid's second trip"""
    return 2 * EW * NT // (W * EL) + 1


def mu_rows_second_trip_elems(W):
    """the same for k_interleave / k_deinterleave (one thread per element, double or double2)"""
    return EW * NT // W + 1


def red_blocks(n, cap=RED):
    return max(1, min(-(-n // NT), cap))


def spike_positions(n, nb):
    """0, n - 1, the last element of a workgroup's first trip, the first element of the grid's second trip"""
    pos = []
    for i in (0, NT - 1, NT, nb * NT - 1, nb * NT, n - 1):
        if 0 <= i < n and i not in pos:
            pos.append(i)
    return pos


# ---- bits, sentinels ---------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ulp_diff(a, b):
    """distance in representable doubles (same sign, finite)"""
    return np.abs(bits(np.atleast_1d(a)) - bits(np.atleast_1d(b)))


def guard(v, tail=TAIL):
    """payload followed by NaN: a write past the end shows, a read past the end poisons a sum"""
    return np.concatenate([np.asarray(v, dtype=np.float64).ravel(), np.full(tail, np.nan)])


def nans(n, tail=TAIL):
    return np.full(n + tail, np.nan)


def tail_intact(buf, n):
    return bool(np.all(np.isnan(buf[n:]))) and len(buf) > n


def scalars(alpha=0.0, beta=0.0, stop=0.0, ndone=0.0, norm=0.0, thr=1e-12, nscal=NSCAL, tail=TAIL):
    """a recurrence's scalar block; the recorded alphas / betas and the tail hold NaN (writes there show)"""
    s = np.full(nscal + tail, np.nan)
    s[:SC_AB] = 0.0
    s[SC_ALPHA], s[SC_BETA], s[SC_STOP], s[SC_NDONE], s[SC_NORM], s[SC_THR], s[SC_EXACT] = alpha, beta, stop, ndone, norm, thr, 1.0
    return s


# ---- summation orders --------------------------------------------------------------------------------------------------
def block_partials(terms, nb):
    """one sum per workgroup of a grid of nb workgroups of 256 threads, in the order of block_sum / block_sum3 /
    k_add_dot3 / k_sumsq_multi: thread t of workgroup b adds terms[b * 256 + t + k * nb * 256], k ascending, to 0.0; the
    64 lanes of a wave are combined by the shuffle tree with offsets 32 ... 1; thread 0 adds the four waves in order to
    0.0.  (Elements a thread does not have are added here as +0.0, which changes no bit: a running sum that starts at
    +0.0 is never -0.0.)"""
    terms = np.asarray(terms, dtype=np.float64)
    per = nb * NT
    trips = max(1, -(-len(terms) // per))
    x = np.zeros(trips * per)
    x[:len(terms)] = terms
    x = x.reshape(trips, nb, NT)
    s = np.zeros((nb, NT))
    for k in range(trips):
        s = s + x[k]
    w = s.reshape(nb, NT // 64, 64).copy()
    off = 32
    while off > 0:
        w[:, :, :off] = w[:, :, :off] + w[:, :, off:2 * off]
        off //= 2
    t = np.zeros(nb)
    for i in range(NT // 64):
        t = t + w[:, i, 0]
    return t


def strided_tree_sum(x, nt=FIN):
    """the finalizing workgroup (k_finalize, kv_sum, kv_sum2, ks_sum3, k_norm_finalize_multi, k_finalize_ab[_multi]):
    thread t of 1024 adds x[t], x[t + 1024], ... in that order to 0.0; then the pairwise tree, offsets 512 ... 1"""
    x = np.asarray(x, dtype=np.float64)
    s = np.zeros(nt)
    for j in range(0, len(x), nt):
        part = x[j:j + nt]
        s[:len(part)] = s[:len(part)] + part
    off = nt // 2
    while off > 0:
        s[:off] = s[:off] + s[off:2 * off]
        off //= 2
    return s[0]


def device_sum(terms, nb):
    """(total, partials) as a capped reduction of nb workgroups followed by the finalizing workgroup gives them"""
    p = block_partials(terms, nb)
    return strided_tree_sum(p), p


def long_sum(terms):
    """(sum, sum of magnitudes) in long double"""
    t = np.asarray(terms, dtype=np.float64).astype(np.longdouble)
    return t.sum(), np.abs(t).sum()


def bound_ratio(value, terms):
    """|value - long-double sum| / (BOUND_ULPS * EPS * sum |terms|); 0 when every term is zero and so is the value"""
    s, mag = long_sum(terms)
    err = abs(np.longdouble(value) - s)
    if mag == 0:
        return 0.0 if err == 0 else np.inf
    return float(err / (BOUND_ULPS * EPS * mag))


# ---- alpha, beta from three sums (lanczos_sums.hpp) -------------------------------------------------------------------------
def beta2_from_sums(alpha, qq, vv, sg):
    d = alpha - sg
    return qq - 2.0 * d * (alpha - sg * vv) + d * d * vv


def ab_from_sums(t, tprev):
    sg = tprev[0] if tprev is not None else 0.0
    b2 = beta2_from_sums(t[0], t[1], t[2], sg)
    return t[0], np.sqrt(b2 if b2 > 0.0 else 0.0), b2


def sums_for(alpha, beta2, sg=0.0):
    """t with t[2] = 1 whose ab_from_sums is (alpha, sqrt(beta2)) up to rounding: qq = beta2 + d^2 with d = alpha - sg"""
    d = alpha - sg
    return np.array([alpha, beta2 + d * d, 1.0])


# t / tprev whose beta^2 is exactly 2.25 in double arithmetic: alpha = 0.5, sg = 0.25, d = 0.25, qq = 2.3125:
# 2.3125 - 2 * 0.25 * (0.5 - 0.25) + 0.0625 = 2.25, every step exact
EXACT_T = np.array([0.5, 2.3125, 1.0])
EXACT_TPREV = np.array([0.25, 7.0, 1.0])


# ---- elementwise references (float64, the kernels' own sequence of operations; no contraction) -----------------------------
def ref_rotate(vin, vout, b):
    ib = 1.0 / b
    return vout * ib, -b * vin


def ref_rotate_lazy(p, q, a, b):
    ib = 1.0 / b
    return (q - a * p) * ib, -b * p


def three_terms(v, w, sg):
    """the terms of T = (<v|w>, sum (w - sg v)^2, <v|v>)"""
    d = w - sg * v
    return v * w, d * d, v * v


def three_terms_pairs(v, w, sg):
    """the same as ks_panel_add_dot adds them: one term per pair of doubles"""
    d = w - sg * v
    vw, dd, vv = v * w, d * d, v * v
    return vw[0::2] + vw[1::2], dd[0::2] + dd[1::2], vv[0::2] + vv[1::2]


# ---- layouts -----------------------------------------------------------------------------------------------------------
def interleave(src, n, W, EL, g):
    """Xi[(r * W + j) * EL + c] = src[(j * n + r) * EL + c] for j < g, +0.0 for the columns g .. W - 1"""
    out = np.zeros(n * W * EL)
    r, j, c = np.meshgrid(np.arange(n), np.arange(g), np.arange(EL), indexing="ij")
    out[((r * W + j) * EL + c).ravel()] = np.asarray(src)[((j * n + r) * EL + c).ravel()]
    return out


def deinterleave(xi, n, W, EL, g, dst):
    """the vectors j < g of dst from the interleaved xi; the rest of dst is left as it is"""
    out = np.array(dst, dtype=np.float64)
    r, j, c = np.meshgrid(np.arange(n), np.arange(g), np.arange(EL), indexing="ij")
    out[((j * n + r) * EL + c).ravel()] = np.asarray(xi)[((r * W + j) * EL + c).ravel()]
    return out


def column(xi, n, W, EL, j):
    """column j of an interleaved buffer as its own vector of n * EL doubles"""
    return np.asarray(xi)[:n * W * EL].reshape(n, W, EL)[:, j, :].ravel().copy()


def blocked_len(dim_up, dim_dw, shift):
    return -(-dim_up // (1 << shift)) * (dim_dw << shift)


def to_blocked(src, dim_up, dim_dw, shift):
    """dst[panel * (dim_dw << shift) + (row << shift) + c] = src[row * dim_up + (panel << shift) + c], +0.0 where the
    column (panel << shift) + c lies past dim_up"""
    pw = 1 << shift
    i = np.arange(blocked_len(dim_up, dim_dw, shift))
    panel, rem = i // (dim_dw * pw), i % (dim_dw * pw)
    row, col = rem // pw, panel * pw + rem % pw
    out = np.zeros(len(i))
    ok = col < dim_up
    out[ok] = np.asarray(src)[row[ok] * dim_up + col[ok]]
    return out


def from_blocked(src, dim_up, dim_dw, shift):
    pw = 1 << shift
    i = np.arange(dim_up * dim_dw)
    row, col = i // dim_up, i % dim_up
    return np.asarray(src)[(col // pw) * (dim_dw * pw) + row * pw + col % pw].copy()


def send_slots(du, nrows, q, world, pcol, halo):
    """(slot, element) pairs of the all-to-all send buffer [world][q][pcol + 2 halo]: element (i, col) goes to block c at
    (c q + i)(pcol + 2 halo) + col - c pcol + halo for every block c whose window [c pcol - halo, (c + 1) pcol + halo)
    holds col"""
    pw = pcol + 2 * halo
    slots, elems = [], []
    i, col = np.meshgrid(np.arange(nrows), np.arange(du), indexing="ij")
    i, col = i.ravel(), col.ravel()
    for c in range(world):
        ok = (col >= c * pcol - halo) & (col < (c + 1) * pcol + halo)
        slots.append((c * q + i[ok]) * pw + col[ok] - c * pcol + halo)
        elems.append(i[ok] * du + col[ok])
    return np.concatenate(slots), np.concatenate(elems)


def pack(x, du, nrows, q, world, pcol, halo, send):
    """send with the elements of x written to their slots; positions no column maps to keep what they held"""
    out = np.array(send, dtype=np.float64)
    slots, elems = send_slots(du, nrows, q, world, pcol, halo)
    out[slots] = np.asarray(x)[elems]
    return out


def back_slots(du, nrows, q, pcol, halo):
    """slot of element (i, col) in back[c][i][halo + j], c = col / pcol, j = col - c pcol"""
    i, col = np.meshgrid(np.arange(nrows), np.arange(du), indexing="ij")
    i, col = i.ravel(), col.ravel()
    c = col // pcol
    return (c * q + i) * (pcol + 2 * halo) + halo + col - c * pcol


def _capi():
    from edipack_amd import capi
    return capi


def library_send_map(du, nrows, q, world, pcol, halo):
    capi = _capi()
    src = np.zeros(world * q * (pcol + 2 * halo), dtype=np.int64)
    capi.check(capi.lib().edigpu_exchange_send_map(du, nrows, q, world, pcol, halo, capi.pi64(src)), "edigpu_exchange_send_map")
    return src


def library_back_map(du, nrows, q, world, pcol, halo):
    capi = _capi()
    slot = np.zeros(nrows * du, dtype=np.int64)
    capi.check(capi.lib().edigpu_exchange_back_map(du, nrows, q, world, pcol, halo, capi.pi64(slot)), "edigpu_exchange_back_map")
    return slot


# ---- hook wrappers: every buffer is copied, the copies that the launcher may write are returned ---------------------------
def _b(a):
    return (_capi().pd(a), len(a)) if a is not None else (None, 0)


def _p(a):
    return _capi().pd(np.ascontiguousarray(a, dtype=np.float64)) if a is not None else None


def _call(name, *args):
    capi = _capi()
    capi.check(getattr(capi.lib(), name)(*args), name)


def hook_norm_begin(n, v, partial, scal):
    v, partial, scal = v.copy(), partial.copy(), scal.copy()
    _call("edigpu_lzk_norm_begin", n, *_b(v), *_b(partial), *_b(scal))
    return v, partial, scal


def hook_rotate(lazy, n, vin, vout, scal):
    vin, vout = vin.copy(), vout.copy()
    _call("edigpu_lzk_rotate", lazy, n, *_b(vin), *_b(vout), *_b(scal))
    return vin, vout


def hook_next_vector(lazy, n, P, Q, X, scal):
    X = X.copy()
    _call("edigpu_lzk_next_vector", lazy, n, *_b(P), *_b(Q), *_b(X), *_b(scal))
    return X


def hook_alpha(n, vin, vout, tmp, partial, scal, it, nlanc=NLANC):
    vout, partial, scal = vout.copy(), partial.copy(), scal.copy()
    _call("edigpu_lzk_alpha", n, *_b(vin), *_b(vout), *_b(tmp), *_b(partial), *_b(scal), it, nlanc)
    return vout, partial, scal


def hook_beta(n, vin, vout, partial, scal, it, nlanc=NLANC):
    vout, partial, scal = vout.copy(), partial.copy(), scal.copy()
    _call("edigpu_lzk_beta", n, *_b(vin), *_b(vout), *_b(partial), *_b(scal), it, nlanc)
    return vout, partial, scal


def hook_add_dot3(n, P, Q, tmp, scal, partial):
    Q, partial = Q.copy(), partial.copy()
    cnt = C.c_int32(-1)
    _call("edigpu_lzk_add_dot3", n, *_b(P), *_b(Q), *_b(tmp), *_b(scal), *_b(partial), C.byref(cnt))
    return Q, partial, cnt.value


def hook_axpy(n, acc, vin, coef, scal, it):
    acc = acc.copy()
    _call("edigpu_lzk_axpy", n, *_b(acc), *_b(vin), coef, *_b(scal), it)
    return acc


def hook_blocked(to, dim_up, dim_dw, shift, src, dst):
    dst = dst.copy()
    _call("edigpu_lzk_blocked", to, dim_up, dim_dw, shift, *_b(src), *_b(dst))
    return dst


def hook_shard_rotate3(first, n, geom, vin, vout, t, tprev, send):
    """geom = (world, du, nrows, q, halo) or None (no exchange: send must be None)"""
    vin, vout = vin.copy(), vout.copy()
    send = send.copy() if send is not None else None
    world, du, _, q, halo = geom if geom is not None else (1, 1, 0, 1, 0)
    _call("edigpu_lzk_shard_rotate3", first, n, du, q, world, pcol_of(world, du), halo, *_b(vin), *_b(vout), _p(t), _p(tprev),
          *_b(send))
    return vin, vout, send


def hook_shard_add_dot3(n, geom, vin, vout, tmp, back, tprev, work, sums):
    vout, work, sums = vout.copy(), work.copy(), sums.copy()
    world, du, _, q, halo = geom if geom is not None else (1, 1, 0, 1, 0)
    _call("edigpu_lzk_shard_add_dot3", n, du, q, world, pcol_of(world, du), halo, *_b(vin), *_b(vout), *_b(tmp), *_b(back),
          _p(tprev), *_b(work), *_b(sums))
    return vout, work, sums


def hook_panel_rotate(n2, x, v, t, tprev):
    x = x.copy()
    _call("edigpu_lzk_panel_rotate", n2, *_b(x), *_b(v), _p(t), _p(tprev))
    return x


def hook_panel_add_dot(n2, x, vdst, rowhalf, colhalf, t, tprev, work, sums):
    vdst, work, sums = vdst.copy(), work.copy(), sums.copy()
    _call("edigpu_lzk_panel_add_dot", n2, *_b(x), *_b(vdst), *_b(rowhalf), *_b(colhalf), _p(t), _p(tprev), *_b(work), *_b(sums))
    return vdst, work, sums


def hook_interleave(to, W, EL, nrow, g, src, dst):
    dst = dst.copy()
    _call("edigpu_lzk_interleave", to, W, int(EL == 2), nrow, g, *_b(src), *_b(dst))
    return dst


def hook_norm_begin_multi(W, EL, nrow, P, partial, scal, sstride):
    P, partial, scal = P.copy(), partial.copy(), scal.copy()
    _call("edigpu_lzk_norm_begin_multi", W, int(EL == 2), nrow, *_b(P), *_b(partial), *_b(scal), sstride)
    return P, partial, scal


def hook_rotate_lazy_multi(W, EL, nrow, P, Q, scal, sstride):
    P, Q = P.copy(), Q.copy()
    _call("edigpu_lzk_rotate_lazy_multi", W, int(EL == 2), nrow, *_b(P), *_b(Q), *_b(scal), sstride)
    return P, Q


def hook_finalize_ab_multi(W, EL, nrow, P, Q, partial, npart, scal, sstride, nlanc=NLANC):
    scal = scal.copy()
    _call("edigpu_lzk_finalize_ab_multi", W, int(EL == 2), nrow, *_b(P), *_b(Q), *_b(partial), npart, *_b(scal), sstride, nlanc)
    return scal


def hook_finalize_ab(npart, partial, P, Q, scal, it, nlanc=NLANC):
    """the single-seed finalize kernel (edigpu_finalize_ab, tests/test_gpu_finalize.py)"""
    capi = _capi()
    scal = scal.copy()
    capi.check(capi.lib().edigpu_finalize_ab(npart, capi.pd(partial), len(P), capi.pd(P), capi.pd(Q), len(scal), capi.pd(scal), it,
                                             nlanc), "edigpu_finalize_ab")
    return scal
