// kernels_multi.hip -- W = 2, 4 or 8 vectors per sweep over a flat sector on gfx950: the stored SELL-64 product and
// the on-the-fly product of kernels_csr.hip / kernels_direct.hip on vectors interleaved element by element,
// Xi[row * W + j] (double or double2), and the per-column vector kernels of W independent Lanczos recurrences that
// advance in lock-step (edigpu_batch.hip).
//
// Why: the stored product streams ~27 times more matrix than vector and pulls a whole line through L2 for every
// 16-byte gather of x[c]; the on-the-fly product spends its time on the applicability tests, popcount signs and rank
// look-ups of a row.  Both costs are per (row, entry) and not per vector: with W columns side by side one matrix word
// (or one index computation) and one gathered line of W * 16 bytes serve W products.  The per-row order of the terms is
// that of the single-vector kernels, so a column of the product is the single-vector product bit for bit on the stored
// image.
//
// Scalars: column j of a recurrence has its own block of the SC_* scalars (kernels.hpp) at scal + j * sstride.  A column
// whose stop flag is set (zero seed, |beta| below the threshold) is written as zeros by the next rotate and stays zero:
// no 1/beta of a stopped column is ever formed.
#include "kernels.hpp"

namespace edigpu {

constexpr int kMuNT = 256;       // vector kernels and the SELL sweep (4 slices of 64 rows per workgroup, as kernels_csr.hip)
constexpr int kMuDirMaxTerms = 512;  // term table in LDS, as kernels_direct.hip

static inline dim3 mu_grid(int64_t n) {
  int64_t nb = (n + kMuNT - 1) / kMuNT;
  if (nb > 4096) nb = 4096;
  if (nb < 1) nb = 1;
  return dim3((unsigned)nb);
}

__device__ inline double2 mu_zero(double2) { return make_double2(0.0, 0.0); }
__device__ inline double mu_zero(double) { return 0.0; }

// natural layout (g vectors of n elements, one after another) -> interleaved; columns g .. W-1 are written as zeros.
// One thread per interleaved element: the writes are contiguous, the reads W streams of 64 / W consecutive elements per wave.
template <int W, typename T>
__global__ void __launch_bounds__(kMuNT)
    k_interleave(int64_t n, int g, const T* __restrict__ src, T* __restrict__ dst) {
  for (int64_t i = (int64_t)blockIdx.x * kMuNT + threadIdx.x; i < n * W; i += (int64_t)gridDim.x * kMuNT) {
    const int j = (int)(i & (W - 1));
    dst[i] = j < g ? src[(int64_t)j * n + i / W] : mu_zero(T());
  }
}

template <int W, typename T>
__global__ void __launch_bounds__(kMuNT)
    k_deinterleave(int64_t n, int g, const T* __restrict__ src, T* __restrict__ dst) {
  for (int64_t i = (int64_t)blockIdx.x * kMuNT + threadIdx.x; i < n * W; i += (int64_t)gridDim.x * kMuNT) {
    const int j = (int)(i & (W - 1));
    if (j < g) dst[(int64_t)j * n + i / W] = src[i];
  }
}

template <typename T>
static int interleave_t(bool to, int W, int64_t n, int g, const T* src, T* dst, hipStream_t st) {
  const dim3 grid = mu_grid(n * W), blk(kMuNT);
#define EDIGPU_MU_IL(WW)                                                                   \
  do {                                                                                     \
    if (to)                                                                                \
      hipLaunchKernelGGL((k_interleave<WW, T>), grid, blk, 0, st, n, g, src, dst);         \
    else                                                                                   \
      hipLaunchKernelGGL((k_deinterleave<WW, T>), grid, blk, 0, st, n, g, src, dst);       \
  } while (0)
  if (W == 2)
    EDIGPU_MU_IL(2);
  else if (W == 4)
    EDIGPU_MU_IL(4);
  else
    EDIGPU_MU_IL(8);
#undef EDIGPU_MU_IL
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

static bool mu_width_ok(int W) { return W == 2 || W == 4 || W == 8; }

int launch_interleave_multi(int W, int cplx, int64_t nrow, int g, const double* src, double* dst, hipStream_t st) {
  if (!mu_width_ok(W) || g < 0 || g > W) {
    set_error("launch_interleave_multi: width must be 2, 4 or 8 and hold the vectors");
    return 1;
  }
  if (nrow <= 0) return 0;
  if (cplx) return interleave_t<double2>(true, W, nrow, g, reinterpret_cast<const double2*>(src), reinterpret_cast<double2*>(dst), st);
  return interleave_t<double>(true, W, nrow, g, src, dst, st);
}

int launch_deinterleave_multi(int W, int cplx, int64_t nrow, int g, const double* src, double* dst, hipStream_t st) {
  if (!mu_width_ok(W) || g < 0 || g > W) {
    set_error("launch_deinterleave_multi: width must be 2, 4 or 8 and hold the vectors");
    return 1;
  }
  if (nrow <= 0) return 0;
  if (cplx) return interleave_t<double2>(false, W, nrow, g, reinterpret_cast<const double2*>(src), reinterpret_cast<double2*>(dst), st);
  return interleave_t<double>(false, W, nrow, g, src, dst, st);
}

// The three sums of one column, reduced over the wave as block_dot_partials does (shuffle tree, lane 0 keeps the sum)
// and parked in LDS for the workgroup's thread 0: red[(3 * j + t) * NW + wave].
template <int NW>
__device__ inline void mu_wave_sums(double a, double q, double n, int j, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    q += __shfl_down(q, off, 64);
    n += __shfl_down(n, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red[(3 * j + 0) * NW + w] = a;
    red[(3 * j + 1) * NW + w] = q;
    red[(3 * j + 2) * NW + w] = n;
  }
}

// after a __syncthreads(): partial[(3 * j + t) * gridDim + blockIdx] = sum over the waves, in wave order
template <int W, int NW>
__device__ inline void mu_block_partials(const double* red, double* __restrict__ partial) {
  if (threadIdx.x < 3 * W) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < NW; i++) t += red[threadIdx.x * NW + i];
    partial[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
  }
}

// SELL-64 on W interleaved vectors: one lane = one row of a slice, as sell_rows[_packed]_kernel.  Per entry one read of
// the packed word (PACKED: 24-bit column | 8-bit dictionary id, values from the LDS copy of the dictionary, the diagonal
// as its own stream) or of col + val, then W accumulators fed from the W * (CPLX ? 16 : 8) contiguous bytes at
// Xi[c * W] with 16-byte loads.  LZ: Yi = Q accumulates the product and the workgroup writes, per column, the partials
// <P|Q>, sum (Q - sg_j P)^2 about that column's previous alpha, <P|P>.
template <int W, bool CPLX, bool PACKED, bool LZ>
__global__ void __launch_bounds__(kMuNT)
    sell_rows_multi_kernel(int64_t nrow, int64_t nslice, const int32_t* __restrict__ sptr, const uint32_t* __restrict__ pk,
                           const double* __restrict__ dict, const double* __restrict__ diag,
                           const int32_t* __restrict__ col, const double* __restrict__ val, const double* __restrict__ Xi,
                           double* __restrict__ Yi, double* __restrict__ partial, const double* __restrict__ scal,
                           int64_t sstride) {
  constexpr int EL = CPLX ? 2 : 1;
  constexpr int NA = W * EL;  // doubles per row of the interleaved vectors
  constexpr int NL = NA / 2;  // 16-byte loads per row
  constexpr int NW = kMuNT / 64;
  __shared__ double dict_s[PACKED ? (CPLX ? 512 : 256) : 1];
  __shared__ double red[LZ ? 3 * W * NW : 1];
  if (PACKED) {
    for (int i = threadIdx.x; i < (CPLX ? 512 : 256); i += kMuNT) dict_s[i] = dict[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t slice = (int64_t)blockIdx.x * NW + (threadIdx.x >> 6);
  if (!LZ && slice >= nslice) return;
  const int64_t row = slice * 64 + lane;
  const bool in = slice < nslice;
  const int32_t b = in ? sptr[slice] : 0, e = in ? sptr[slice + 1] : 0;
  const double2* __restrict__ X2 = reinterpret_cast<const double2*>(Xi);
  double acc[NA];
#pragma unroll
  for (int i = 0; i < NA; i++) acc[i] = 0.0;
  constexpr int UNR = 8 / W;  // entries in flight: 8 gathers of 16 bytes (real) or 16 (complex) per lane
#pragma unroll UNR
  for (int32_t k = b; k < e; k++) {
    const int64_t o = (int64_t)k * 64 + lane;
    int64_t c;
    double ar, ai = 0.0;
    if (PACKED) {
      const uint32_t p = pk[o];
      c = p & 0xFFFFFFu;
      const int id = p >> 24;
      ar = CPLX ? dict_s[2 * id] : dict_s[id];
      if (CPLX) ai = dict_s[2 * id + 1];
    } else {
      c = col[o];
      if (CPLX) {
        const double2 a2 = reinterpret_cast<const double2*>(val)[o];
        ar = a2.x;
        ai = a2.y;
      } else {
        ar = val[o];
      }
    }
    double2 xv[NL];
#pragma unroll
    for (int l = 0; l < NL; l++) xv[l] = X2[c * NL + l];
#pragma unroll
    for (int l = 0; l < NL; l++) {
      if (CPLX) {
        acc[2 * l] += ar * xv[l].x - ai * xv[l].y;
        acc[2 * l + 1] += ar * xv[l].y + ai * xv[l].x;
      } else {
        acc[2 * l] += ar * xv[l].x;
        acc[2 * l + 1] += ar * xv[l].y;
      }
    }
  }
  const bool live = in && row < nrow;
  double2* __restrict__ Y2 = reinterpret_cast<double2*>(Yi);
#pragma unroll
  for (int l = 0; l < NL; l++) {
    double2 xo = make_double2(0.0, 0.0), o2 = make_double2(0.0, 0.0);
    if (live) {
      if (LZ || (PACKED && diag != nullptr)) xo = X2[row * NL + l];
      double sx = acc[2 * l], sy = acc[2 * l + 1];
      if (PACKED && diag != nullptr) {
        if (CPLX) {
          const double2 d = reinterpret_cast<const double2*>(diag)[row];
          sx += d.x * xo.x - d.y * xo.y;
          sy += d.x * xo.y + d.y * xo.x;
        } else {
          const double d = diag[row];
          sx += d * xo.x;
          sy += d * xo.y;
        }
      }
      if (LZ) o2 = Y2[row * NL + l];
      o2.x += sx;
      o2.y += sy;
      Y2[row * NL + l] = o2;
    }
    if (LZ) {
      if (CPLX) {
        const double sg = scal[(int64_t)l * sstride + SC_ALPHA];
        mu_wave_sums<NW>(xo.x * o2.x + xo.y * o2.y,
                         (o2.x - sg * xo.x) * (o2.x - sg * xo.x) + (o2.y - sg * xo.y) * (o2.y - sg * xo.y),
                         xo.x * xo.x + xo.y * xo.y, l, red);
      } else {
        const double sg0 = scal[(int64_t)(2 * l) * sstride + SC_ALPHA], sg1 = scal[(int64_t)(2 * l + 1) * sstride + SC_ALPHA];
        mu_wave_sums<NW>(xo.x * o2.x, (o2.x - sg0 * xo.x) * (o2.x - sg0 * xo.x), xo.x * xo.x, 2 * l, red);
        mu_wave_sums<NW>(xo.y * o2.y, (o2.y - sg1 * xo.y) * (o2.y - sg1 * xo.y), xo.y * xo.y, 2 * l + 1, red);
      }
    }
  }
  if (LZ) {
    __syncthreads();
    mu_block_partials<W, NW>(red, partial);
  }
}

template <int W, bool CPLX, bool LZ>
static void sell_multi_launch(const DevCsr& a, int64_t nb, const double* Xi, double* Yi, double* partial, const double* scal,
                              int64_t sstride, hipStream_t st) {
  const dim3 g((unsigned)nb), blk(kMuNT);
  if (a.sell_packed)
    hipLaunchKernelGGL((sell_rows_multi_kernel<W, CPLX, true, LZ>), g, blk, 0, st, a.nrow, a.nslice, a.sell_ptr, a.sell_pk,
                       a.sell_dict, a.sell_diag, (const int32_t*)nullptr, (const double*)nullptr, Xi, Yi, partial, scal, sstride);
  else
    hipLaunchKernelGGL((sell_rows_multi_kernel<W, CPLX, false, LZ>), g, blk, 0, st, a.nrow, a.nslice, a.sell_ptr,
                       (const uint32_t*)nullptr, (const double*)nullptr, (const double*)nullptr, a.sell_col, a.sell_val, Xi, Yi,
                       partial, scal, sstride);
}

// Yi = A Xi (lz = false) or Yi += A Xi with the 3 * W * (*np) partials (lz = true) on the SELL image of a whole square
// block (csr_lanczos_fusable).  cap: doubles in `partial`, checked before anything is enqueued.
int launch_csr_multi(const DevCsr& a, int cplx, int W, const double* Xi, double* Yi, bool lz, double* partial, int64_t cap,
                     int* np, const double* scal, int64_t sstride, hipStream_t st) {
  if (!mu_width_ok(W) || !a.sell || a.nrow <= 0) {
    set_error("launch_csr_multi: needs the SELL image and a width of 2, 4 or 8");
    return 1;
  }
  const int64_t nb = (a.nslice + kMuNT / 64 - 1) / (kMuNT / 64);
  if (lz && (3 * (int64_t)W * nb > cap || !partial || !scal)) {
    set_error("launch_csr_multi: partial buffer too small");
    return 1;
  }
  if (np) *np = (int)nb;
#define EDIGPU_MU_SELL(WW)                                                                     \
  do {                                                                                         \
    if (cplx) {                                                                                \
      if (lz)                                                                                  \
        sell_multi_launch<WW, true, true>(a, nb, Xi, Yi, partial, scal, sstride, st);          \
      else                                                                                     \
        sell_multi_launch<WW, true, false>(a, nb, Xi, Yi, partial, scal, sstride, st);         \
    } else {                                                                                   \
      if (lz)                                                                                  \
        sell_multi_launch<WW, false, true>(a, nb, Xi, Yi, partial, scal, sstride, st);         \
      else                                                                                     \
        sell_multi_launch<WW, false, false>(a, nb, Xi, Yi, partial, scal, sstride, st);        \
    }                                                                                          \
  } while (0)
  if (W == 2)
    EDIGPU_MU_SELL(2);
  else if (W == 4)
    EDIGPU_MU_SELL(4);
  else
    EDIGPU_MU_SELL(8);
#undef EDIGPU_MU_SELL
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

// On-the-fly product on W interleaved complex vectors: direct_rows_kernel with the applicability mask, flip, sign,
// column and coefficient of a (row, term) computed once and the gather + four FMAs run W times.  The terms of a row
// are visited in ascending order, TIF at a time, so a column's FMA chain is the single-vector kernel's.
// Budgets.  VGPRs per lane = 512 / waves per SIMD; a lane holds 4 W accumulators, 4 W TIF gathered doubles and, in
// the fused step, 6 W running sums (TIF = terms in flight per round of the compacted loop).  The single-vector kernel's
// 1024 threads at 8 waves/SIMD (64 VGPRs) hold none of the widths without scratch.  All widths: 512 threads.
//   W = 2: TIF 4, W = 4: TIF 2 (eight 16-byte gathers in flight), 4 waves/SIMD (128 VGPRs): two workgroups of 8 waves per
//          CU, which is also what the LDS holds with the rank tables of Ns = 13 staged (2 x 78 KiB of 160)
//   W = 8: TIF 2, 2 waves/SIMD (256 VGPRs, 220 used): one workgroup per CU.  This width only runs on small, latency-bound
//          sectors (edigpu_batch.hip: widest_kept), where the number of dependent rounds per row counts and occupancy
//          does not: with TIF 1 on 768 threads at 3 waves/SIMD it took 19.7 us per seed and step on 3 432 rows, now 14.4
template <int W>
struct DirMulti {
  static constexpr int NT = 512;
  static constexpr int WAVES = W == 8 ? 2 : 4;
  static constexpr int TIF = W == 2 ? 4 : 2;
};

template <int W, bool LDS_TABLES, bool LZ, bool COMPACT>
__global__ void __launch_bounds__(DirMulti<W>::NT, DirMulti<W>::WAVES)
    direct_rows_multi_kernel(int64_t nrow, int64_t row_first, int ns, int norb, int nterms,
                             const int32_t* __restrict__ states, const int32_t* __restrict__ off_dw,
                             const int32_t* __restrict__ rk_up, const DirectTerm* __restrict__ terms,
                             const uint2* __restrict__ tests, const double* __restrict__ dtab,
                             const double* __restrict__ xtab, const double2* __restrict__ Xi, double2* __restrict__ Yi,
                             double* __restrict__ partial, const double* __restrict__ scal, int64_t sstride) {
  constexpr int NT = DirMulti<W>::NT;
  constexpr int TIF = DirMulti<W>::TIF;
  constexpr int NW = NT / 64;
  extern __shared__ int32_t tabs[];  // [off_dw | rk_up] when LDS_TABLES, then the term table when COMPACT
  __shared__ double red[LZ ? 3 * W * NW : 1];
  double da[LZ ? W : 1], dq[LZ ? W : 1], dn[LZ ? W : 1];
  double sgm[LZ ? W : 1];
  if (LZ) {
#pragma unroll
    for (int k = 0; k < W; k++) {
      da[k] = dq[k] = dn[k] = 0.0;
      sgm[k] = scal[(int64_t)k * sstride + SC_ALPHA];
    }
  }
  const uint32_t lomask = (1u << ns) - 1u, impmask = (1u << norb) - 1u;
  if (LDS_TABLES) {
    const int n = 1 << ns;
    for (int i = threadIdx.x; i < n; i += NT) {
      tabs[i] = off_dw[i];
      tabs[n + i] = rk_up[i];
    }
  }
  const int32_t* __restrict__ t_off = LDS_TABLES ? tabs : off_dw;
  const int32_t* __restrict__ t_rk = LDS_TABLES ? tabs + (1 << ns) : rk_up;
  uint32_t* t_flip = reinterpret_cast<uint32_t*>(tabs + (LDS_TABLES ? (2 << ns) : 0));
  uint32_t* t_smask = t_flip + kMuDirMaxTerms;
  uint32_t* t_csign = t_smask + kMuDirMaxTerms;
  double2* t_coef = reinterpret_cast<double2*>(t_csign + kMuDirMaxTerms);
  if (COMPACT) {
    for (int t = threadIdx.x; t < nterms; t += NT) {
      const DirectTerm tm = terms[t];
      t_flip[t] = tm.flip;
      t_smask[t] = tm.sign_mask;
      t_csign[t] = (uint32_t)tm.csign;
      t_coef[t] = make_double2(tm.cre, tm.cim);
    }
  }
  if (LDS_TABLES || COMPACT) __syncthreads();
  for (int64_t r = (int64_t)blockIdx.x * NT + threadIdx.x; r < nrow; r += (int64_t)gridDim.x * NT) {
    const uint32_t s = (uint32_t)states[r];
    const double dg = dtab[s & 255u] + dtab[256 + ((s >> 8) & 255u)] + dtab[512 + ((s >> 16) & 255u)] +
                      dtab[768 + (s >> 24)] + xtab[(((s >> ns) & impmask) << norb) | (s & impmask)];
    const int64_t own = (row_first + r) * W;
    double ar[W], ai[W];
#pragma unroll
    for (int k = 0; k < W; k++) {
      const double2 x0 = Xi[own + k];
      ar[k] = dg * x0.x;
      ai[k] = dg * x0.y;
    }
    if (COMPACT) {
      for (int g0 = 0; g0 < nterms; g0 += 32) {
        uint32_t mw = 0;
#pragma unroll
        for (int b4 = 0; b4 < 32; b4 += 4) {
          uint2 tq[4];
#pragma unroll
          for (int u = 0; u < 4; u++) tq[u] = tests[g0 + b4 + u];  // padded to a multiple of 32
#pragma unroll
          for (int u = 0; u < 4; u++) mw |= ((s & tq[u].y) == tq[u].x) ? (1u << (b4 + u)) : 0u;
        }
        while (__any(mw != 0u)) {
          // TIF applicable terms of this lane (missing ones: weight 0, own row)
          int64_t j[TIF];
          int sg[TIF];
          double2 cf[TIF];
#pragma unroll
          for (int u = 0; u < TIF; u++) {
            const bool h = mw != 0u;
            const int t = g0 + (h ? __ffs(mw) - 1 : 0);
            mw &= mw - 1u;
            const uint32_t w = s ^ t_flip[t];
            j[u] = h ? ((int64_t)t_off[w >> ns] + t_rk[w & lomask]) * W : own;
            sg[u] = (int)((uint32_t)((__popc(s & t_smask[t]) + (int)t_csign[t]) & 1) << 31);
            cf[u] = h ? t_coef[t] : make_double2(0.0, 0.0);
          }
          double2 x[TIF][W];
#pragma unroll
          for (int u = 0; u < TIF; u++)
#pragma unroll
            for (int k = 0; k < W; k++) x[u][k] = Xi[j[u] + k];
#pragma unroll
          for (int u = 0; u < TIF; u++)
#pragma unroll
            for (int k = 0; k < W; k++) {
              const double xr = __hiloint2double(__double2hiint(x[u][k].x) ^ sg[u], __double2loint(x[u][k].x));
              const double xi = __hiloint2double(__double2hiint(x[u][k].y) ^ sg[u], __double2loint(x[u][k].y));
              ar[k] = fma(cf[u].x, xr, ar[k]);
              ar[k] = fma(-cf[u].y, xi, ar[k]);
              ai[k] = fma(cf[u].x, xi, ai[k]);
              ai[k] = fma(cf[u].y, xr, ai[k]);
            }
        }
      }
    }
    for (int t0 = COMPACT ? nterms : 0; t0 < nterms; t0 += 4) {
      uint2 tq[4];
#pragma unroll
      for (int u = 0; u < 4; u++) tq[u] = tests[t0 + u];  // wave-uniform: scalar loads
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if ((s & tq[u].y) == tq[u].x) {
          const DirectTerm tm = terms[t0 + u];
          const uint32_t w = s ^ tm.flip;
          const int64_t jc = ((int64_t)t_off[w >> ns] + t_rk[w & lomask]) * W;
          const int sg = (int)((uint32_t)((__popc(s & tm.sign_mask) + tm.csign) & 1) << 31);
#pragma unroll
          for (int k = 0; k < W; k++) {
            const double2 x = Xi[jc + k];
            const double xr = __hiloint2double(__double2hiint(x.x) ^ sg, __double2loint(x.x));
            const double xi = __hiloint2double(__double2hiint(x.y) ^ sg, __double2loint(x.y));
            ar[k] = fma(tm.cre, xr, ar[k]);
            ar[k] = fma(-tm.cim, xi, ar[k]);
            ai[k] = fma(tm.cre, xi, ai[k]);
            ai[k] = fma(tm.cim, xr, ai[k]);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < W; k++) {
      if (LZ) {
        const double2 q = Yi[r * W + k];
        const double2 x0 = Xi[own + k];  // (the row's own line: read at the top of the row, still in cache)
        ar[k] += q.x;
        ai[k] += q.y;
        da[k] += x0.x * ar[k] + x0.y * ai[k];
        dq[k] += (ar[k] - sgm[k] * x0.x) * (ar[k] - sgm[k] * x0.x) + (ai[k] - sgm[k] * x0.y) * (ai[k] - sgm[k] * x0.y);
        dn[k] += x0.x * x0.x + x0.y * x0.y;
      }
      Yi[r * W + k] = make_double2(ar[k], ai[k]);
    }
  }
  if (LZ) {
#pragma unroll
    for (int k = 0; k < W; k++) mu_wave_sums<NW>(da[k], dq[k], dn[k], k, red);
    __syncthreads();
    mu_block_partials<W, NW>(red, partial);
  }
}

template <int W, bool LZ>
static int direct_multi_t(const edigpu_sector* s, const double* Xi, double* Yi, double* partial, int64_t cap, int* np,
                          const double* scal, int64_t sstride, hipStream_t st) {
  constexpr int NT = DirMulti<W>::NT;
  const int64_t nrow = s->nloc;
  int64_t nb = (nrow + NT - 1) / NT;
  const int64_t nbmax = (int64_t)256 * s->sw.direct_wgs * 2;  // persistent workgroups of 512 threads sweep the rows
  if (nb > nbmax) nb = nbmax;
  if (LZ && (3 * (int64_t)W * nb > cap || !partial || !scal)) {
    set_error("launch_direct_multi: partial buffer too small");
    return 1;
  }
  if (np) *np = (int)nb;
  const size_t tab_bytes = (size_t)2 * sizeof(int32_t) << s->dir_ns;
  const size_t term_bytes = (size_t)kMuDirMaxTerms * (3 * sizeof(uint32_t) + sizeof(double2));
  const bool compact = !s->sw.direct_termorder && s->dir_nterms <= kMuDirMaxTerms;
  const double2* x2 = reinterpret_cast<const double2*>(Xi);
  double2* y2 = reinterpret_cast<double2*>(Yi);
#define EDIGPU_MU_DIRECT(LT, CP, LDSB)                                                                          \
  do {                                                                                                          \
    auto kern = direct_rows_multi_kernel<W, LT, LZ, CP>;                                                        \
    if (ensure_dynamic_lds((const void*)kern, (LDSB))) return 1;                                                \
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(NT), (LDSB), st, nrow, s->row_first, s->dir_ns,           \
                       s->dir_norb, s->dir_nterms, s->d_dir_states, s->d_dir_offdw, s->d_dir_rkup,              \
                       s->d_dir_terms, s->d_dir_tests, s->d_dir_dtab, s->d_dir_xtab, x2, y2, partial, scal,     \
                       sstride);                                                                                \
  } while (0)
  if (tab_bytes <= 64 * 1024) {
    if (compact)
      EDIGPU_MU_DIRECT(true, true, tab_bytes + term_bytes);
    else
      EDIGPU_MU_DIRECT(true, false, tab_bytes);
  } else {
    if (compact)
      EDIGPU_MU_DIRECT(false, true, term_bytes);
    else
      EDIGPU_MU_DIRECT(false, false, (size_t)0);
  }
#undef EDIGPU_MU_DIRECT
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

// as launch_csr_multi, on a whole on-the-fly sector without phonons
int launch_direct_multi(const edigpu_sector* s, int W, const double* Xi, double* Yi, bool lz, double* partial, int64_t cap,
                        int* np, const double* scal, int64_t sstride, hipStream_t st) {
  if (!mu_width_ok(W) || s->kind != kDirect || s->nph > 0 || s->nloc != s->dim || s->nloc <= 0) {
    set_error("launch_direct_multi: needs a whole on-the-fly sector without phonons and a width of 2, 4 or 8");
    return 1;
  }
  if (W == 2) return lz ? direct_multi_t<2, true>(s, Xi, Yi, partial, cap, np, scal, sstride, st)
                        : direct_multi_t<2, false>(s, Xi, Yi, partial, cap, np, scal, sstride, st);
  if (W == 4) return lz ? direct_multi_t<4, true>(s, Xi, Yi, partial, cap, np, scal, sstride, st)
                        : direct_multi_t<4, false>(s, Xi, Yi, partial, cap, np, scal, sstride, st);
  return lz ? direct_multi_t<8, true>(s, Xi, Yi, partial, cap, np, scal, sstride, st)
            : direct_multi_t<8, false>(s, Xi, Yi, partial, cap, np, scal, sstride, st);
}

// ---- the vector kernels of W recurrences in lock-step; EL doubles per element, column j of row r at (r * W + j) * EL ----

// partial[j * gridDim.x + blockIdx.x] = this workgroup's part of <P_j|P_j>, j = blockIdx.y: element i of column j's real
// view is visited by the thread that visits element i in k_sumsq (kernels_lanczos.hip), and the sums are combined in
// the same order, so a column's norm is the single-seed norm bit for bit
template <int W, int EL>
__global__ void __launch_bounds__(kMuNT)
    k_sumsq_multi(const double* __restrict__ P, int64_t n, double* __restrict__ partial) {
  constexpr int NW = kMuNT / 64;
  __shared__ double ws[NW];
  const int j = blockIdx.y;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kMuNT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kMuNT) {
    const double v = P[((i / EL) * W + j) * EL + i % EL];
    s += v * v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < NW; i++) t += ws[i];
    partial[(int64_t)j * gridDim.x + blockIdx.x] = t;
  }
}

// workgroup j: the norm of column j, as k_finalize in mode 0 (a zero seed sets the stop flag)
__global__ void __launch_bounds__(1024)
    k_norm_finalize_multi(const double* __restrict__ partial, int np, double* __restrict__ scal, int64_t sstride) {
  __shared__ double sh[1024];
  double* sc = scal + (int64_t)blockIdx.x * sstride;
  double s = 0.0;
  for (int i = threadIdx.x; i < np; i += 1024) s += partial[(int64_t)blockIdx.x * np + i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double nrm = sqrt(sh[0]);
    sc[SC_NORM] = nrm;
    sc[SC_STOP] = (nrm > 0.0) ? 0.0 : 1.0;  // zero (or NaN) seed: the column never starts
    sc[SC_NDONE] = 0.0;
  }
}

// One thread per 16-byte chunk; the grid stride is a multiple of W, so a thread stays in its column(s).  A column whose
// stop flag is set is written as zeros: whatever the seed held, the column is zero from here on.
template <int W, int EL>
__global__ void __launch_bounds__(kMuNT)
    k_scale_by_norm_multi(double* __restrict__ P, int64_t nchunk, const double* __restrict__ scal, int64_t sstride) {
  const int64_t i0 = (int64_t)blockIdx.x * kMuNT + threadIdx.x;
  const int j0 = EL == 2 ? (int)(i0 & (W - 1)) : (int)((2 * i0) & (W - 1));
  const int j1 = EL == 2 ? j0 : j0 + 1;
  const double f0 = scal[j0 * sstride + SC_STOP] != 0.0 ? 0.0 : 1.0 / scal[j0 * sstride + SC_NORM];
  const double f1 = scal[j1 * sstride + SC_STOP] != 0.0 ? 0.0 : 1.0 / scal[j1 * sstride + SC_NORM];
  double2* P2 = reinterpret_cast<double2*>(P);
  for (int64_t i = i0; i < nchunk; i += (int64_t)gridDim.x * kMuNT) {
    double2 p = P2[i];
    p.x = f0 != 0.0 ? p.x * f0 : 0.0;
    p.y = f1 != 0.0 ? p.y * f1 : 0.0;
    P2[i] = p;
  }
}

// (P_j, Q_j) <- ((Q_j - alpha_j P_j) / beta_j, -beta_j P_j) per column, as k_rotate_lazy; a stopped column <- (0, 0)
template <int W, int EL>
__global__ void __launch_bounds__(kMuNT)
    k_rotate_lazy_multi(double* __restrict__ P, double* __restrict__ Q, int64_t nchunk, const double* __restrict__ scal,
                        int64_t sstride) {
  const int64_t i0 = (int64_t)blockIdx.x * kMuNT + threadIdx.x;
  const int j0 = EL == 2 ? (int)(i0 & (W - 1)) : (int)((2 * i0) & (W - 1));
  const int j1 = EL == 2 ? j0 : j0 + 1;
  const bool on0 = scal[j0 * sstride + SC_STOP] == 0.0, on1 = scal[j1 * sstride + SC_STOP] == 0.0;
  const double a0 = scal[j0 * sstride + SC_ALPHA], b0 = scal[j0 * sstride + SC_BETA], ib0 = on0 ? 1.0 / b0 : 0.0;
  const double a1 = scal[j1 * sstride + SC_ALPHA], b1 = scal[j1 * sstride + SC_BETA], ib1 = on1 ? 1.0 / b1 : 0.0;
  double2* P2 = reinterpret_cast<double2*>(P);
  double2* Q2 = reinterpret_cast<double2*>(Q);
  for (int64_t i = i0; i < nchunk; i += (int64_t)gridDim.x * kMuNT) {
    const double2 p = P2[i], q = Q2[i];
    double2 pn, qn;
    pn.x = on0 ? (q.x - a0 * p.x) * ib0 : 0.0;
    qn.x = on0 ? -b0 * p.x : 0.0;
    pn.y = on1 ? (q.y - a1 * p.y) * ib1 : 0.0;
    qn.y = on1 ? -b1 * p.y : 0.0;
    P2[i] = pn;
    Q2[i] = qn;
  }
}

// Workgroup j finalizes the step of column j from partial[(3 * j + t) * np + i]: lz_finalize_ab_device (lz_finalize.hpp)
// with the device-side step index, on a strided column.  A stopped column returns at once: its scalars stay as the
// step that stopped it left them.
template <int W, int EL>
__global__ void __launch_bounds__(1024)
    k_finalize_ab_multi(const double* __restrict__ partial, int np, const double* __restrict__ P,
                        const double* __restrict__ Q, int64_t nrow, double* __restrict__ scal, int64_t sstride, int nlanc) {
  constexpr int NT = 1024;
  __shared__ double sa[NT], sq[NT], sn[NT];
  const int j = blockIdx.x;
  double* sc = scal + (int64_t)j * sstride;
  if (sc[SC_STOP] != 0.0) return;
  const int iter = (int)sc[SC_NDONE];
  if (iter >= nlanc) return;
  const double* pa = partial + (int64_t)(3 * j) * np;
  double a = 0.0, q = 0.0, nn = 0.0;
  for (int i = threadIdx.x; i < np; i += NT) {
    a += pa[i];
    q += pa[np + i];
    nn += pa[2 * np + i];
  }
  sa[threadIdx.x] = a;
  sq[threadIdx.x] = q;
  sn[threadIdx.x] = nn;
  __syncthreads();
  for (int off = NT / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      sa[threadIdx.x] += sa[threadIdx.x + off];
      sq[threadIdx.x] += sq[threadIdx.x + off];
      sn[threadIdx.x] += sn[threadIdx.x + off];
    }
    __syncthreads();
  }
  const double alpha = sa[0], qq = sq[0], vv = sn[0], sg = sc[SC_ALPHA];
  const double d = alpha - sg;
  double b2 = qq - 2.0 * d * (alpha - sg * vv) + d * d * vv;
  const bool exact = b2 < 1e-3 * qq;  // the same value in every thread
  __syncthreads();
  if (exact) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < nrow * EL; i += NT) {
      const int64_t o = ((i / EL) * W + j) * EL + i % EL;
      const double w = Q[o] - alpha * P[o];
      s += w * w;
    }
    sa[threadIdx.x] = s;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) sa[threadIdx.x] += sa[threadIdx.x + off];
      __syncthreads();
    }
    b2 = sa[0];
  }
  if (threadIdx.x == 0) {
    sc[SC_ALPHA] = alpha;
    sc[SC_AB + iter] = alpha;
    sc[SC_NDONE] = (double)(iter + 1);
    sc[SC_EXACT] = 0.0;
    const double b = sqrt(b2 > 0.0 ? b2 : 0.0);
    sc[SC_BETA] = b;
    if (!(fabs(b) > 0.0) || fabs(b) < sc[SC_THR])
      sc[SC_STOP] = 1.0;
    else if (iter + 1 < nlanc)
      sc[SC_AB + nlanc + iter + 1] = b;
  }
}

#define EDIGPU_MU_WEL(CALL)            \
  do {                                 \
    if (cplx) {                        \
      if (W == 2) CALL(2, 2);          \
      else if (W == 4) CALL(4, 2);     \
      else CALL(8, 2);                 \
    } else {                           \
      if (W == 2) CALL(2, 1);          \
      else if (W == 4) CALL(4, 1);     \
      else CALL(8, 1);                 \
    }                                  \
  } while (0)

// norms of the W seeds in P (interleaved), then every column scaled to unit length; partial: W * 1024 doubles at most
int lz_norm_begin_multi(int W, int cplx, int64_t nrow, double* P, double* partial, int64_t cap, double* scal,
                        int64_t sstride, hipStream_t st) {
  if (!mu_width_ok(W)) {
    set_error("lz_norm_begin_multi: width must be 2, 4 or 8");
    return 1;
  }
  const int64_t n1 = nrow * (cplx ? 2 : 1);  // doubles of one column
  int64_t nb = (n1 + kMuNT - 1) / kMuNT;
  if (nb > kRedBlocks) nb = kRedBlocks;
  if (nb < 1) nb = 1;
  if ((int64_t)W * nb > cap) {
    set_error("lz_norm_begin_multi: partial buffer too small");
    return 1;
  }
  const int64_t nchunk = n1 * W / 2;
#define EDIGPU_MU_NORM(WW, EE)                                                                                        \
  do {                                                                                                                \
    hipLaunchKernelGGL((k_sumsq_multi<WW, EE>), dim3((unsigned)nb, WW), dim3(kMuNT), 0, st, (const double*)P, n1, partial); \
    hipLaunchKernelGGL(k_norm_finalize_multi, dim3(WW), dim3(1024), 0, st, (const double*)partial, (int)nb, scal, sstride); \
    hipLaunchKernelGGL((k_scale_by_norm_multi<WW, EE>), mu_grid(nchunk), dim3(kMuNT), 0, st, P, nchunk,               \
                       (const double*)scal, sstride);                                                                 \
  } while (0)
  EDIGPU_MU_WEL(EDIGPU_MU_NORM);
#undef EDIGPU_MU_NORM
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

int lz_rotate_lazy_multi(int W, int cplx, int64_t nrow, double* P, double* Q, const double* scal, int64_t sstride,
                         hipStream_t st) {
  if (!mu_width_ok(W)) {
    set_error("lz_rotate_lazy_multi: width must be 2, 4 or 8");
    return 1;
  }
  if (nrow <= 0) return 0;
  const int64_t nchunk = nrow * W * (cplx ? 2 : 1) / 2;
#define EDIGPU_MU_ROT(WW, EE) \
  hipLaunchKernelGGL((k_rotate_lazy_multi<WW, EE>), mu_grid(nchunk), dim3(kMuNT), 0, st, P, Q, nchunk, scal, sstride)
  EDIGPU_MU_WEL(EDIGPU_MU_ROT);
#undef EDIGPU_MU_ROT
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

int lz_finalize_ab_multi(int W, int cplx, int64_t nrow, const double* P, const double* Q, const double* partial, int np,
                         double* scal, int64_t sstride, int nlanc, hipStream_t st) {
  if (!mu_width_ok(W)) {
    set_error("lz_finalize_ab_multi: width must be 2, 4 or 8");
    return 1;
  }
#define EDIGPU_MU_FIN(WW, EE)                                                                                      \
  hipLaunchKernelGGL((k_finalize_ab_multi<WW, EE>), dim3(WW), dim3(1024), 0, st, partial, np, P, Q, nrow, scal, sstride, \
                     nlanc)
  EDIGPU_MU_WEL(EDIGPU_MU_FIN);
#undef EDIGPU_MU_FIN
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

#undef EDIGPU_MU_WEL

}  // namespace edigpu
