// kernels_ph.hip -- phonon operators on device vectors (edigpu_apply_xph, edigpu_ph_rdm).  A vector is DimPh blocks of
// dim_el electronic elements, i = i_el + n dim_el; tables and work list: host_ph.hpp.
//
//   apply_xph: dst(i_el, n) = sqrt(n+1) src(i_el, n+1) + sqrt(n) src(i_el, n-1), the seed (b + b^dagger)|v> of the phonon
//            Green's function (lanc_build_gf_phonon_main, ED_GF_NORMAL.f90:318-333).  A lane owns one item of a block -- 16
//            bytes (two real columns, or one complex column) where both vectors and the block stride allow it, 8 bytes
//            otherwise -- and walks n with a window of three values: every source element is read once, every
//            destination element written once, coalesced along i_el in every block.  Two products and one sum per output,
//            uncontracted (-ffp-contract=off); the edge blocks are one product.
//   ph_rdm:  rho[c][n][m] = sum over the i_el of class c of v(i_el, n) conj v(i_el, m): a Gram matrix of DimPh tall
//            vectors, resolved by class.  A wave (one 64-thread workgroup) owns a work unit, a range of elements of ONE
//            class (PhUnit); a lane fetches the DimPh values of its element and adds the products of a B x B tile of
//            (n, m) into registers.  DimPh <= B: one tile, the triangle n <= m, every element fetched from HBM once and
//            nothing re-read (B = 4, 8, 16 for real vectors: 136 accumulators at B = 16; B = 4, 8 for complex ones).  Past
//            that the (n, m) plane is tiled by 8 x 8: the diagonal tiles and the tiles above them are separate waves that
//            read the unit again, from L2.  At the end of the unit the wave reduces by butterfly and lane 0 writes the
//            tile's sums to the unit's own place; ph_final_kernel adds the units of a class in unit order.  No
//            floating-point atomics: two calls give the same bits.
#include "host_ph.hpp"
#include "kernels.hpp"

namespace edigpu {
namespace {

constexpr int kXphBlock = 256;

// W doubles per item; VEC: one 16-byte access
template <int W, bool VEC>
struct XphItem {
  double x[W];
  __device__ static inline XphItem load(const double* __restrict__ p) {
    XphItem r;
    if (VEC) {
      const double2 t = *reinterpret_cast<const double2*>(p);
      r.x[0] = t.x;
      r.x[W - 1] = t.y;
    } else {
#pragma unroll
      for (int k = 0; k < W; k++) r.x[k] = p[k];
    }
    return r;
  }
  __device__ inline void store(double* p) const {
    if (VEC) {
      *reinterpret_cast<double2*>(p) = make_double2(x[0], x[W - 1]);
    } else {
#pragma unroll
      for (int k = 0; k < W; k++) p[k] = x[k];
    }
  }
};

// stride: doubles per phonon block, nitem: items of W doubles per block
template <int W, bool VEC>
__global__ __launch_bounds__(kXphBlock) void apply_xph_kernel(int dimph, int64_t stride, int64_t nitem, const double* __restrict__ sq,
                                                              const double* __restrict__ src, double* __restrict__ dst) {
  using Item = XphItem<W, VEC>;
  const int64_t nth = (int64_t)gridDim.x * kXphBlock;
  for (int64_t i = (int64_t)blockIdx.x * kXphBlock + threadIdx.x; i < nitem; i += nth) {
    const double* s = src + i * W;
    double* d = dst + i * W;
    Item x0 = Item::load(s), x1 = Item::load(s + stride), o;
    const double c1 = sq[1];
#pragma unroll
    for (int k = 0; k < W; k++) o.x[k] = c1 * x1.x[k];
    o.store(d);
#pragma unroll 4
    for (int n = 1; n < dimph - 1; n++) {
      const Item x2 = Item::load(s + (int64_t)(n + 1) * stride);
      const double up = sq[n + 1], dn = sq[n];
#pragma unroll
      for (int k = 0; k < W; k++) o.x[k] = up * x2.x[k] + dn * x0.x[k];
      o.store(d + (int64_t)n * stride);
      x0 = x1;
      x1 = x2;
    }
    const double cl = sq[dimph - 1];
#pragma unroll
    for (int k = 0; k < W; k++) o.x[k] = cl * x0.x[k];
    o.store(d + (int64_t)(dimph - 1) * stride);
  }
}

template <int CW>
__device__ inline void ph_load(const double* __restrict__ v, int64_t e, bool al16, double* out) {
  if (CW == 1) {
    out[0] = v[e];
  } else if (al16) {
    const double2 t = reinterpret_cast<const double2*>(v)[e];
    out[0] = t.x;
    out[1] = t.y;
  } else {
    out[0] = v[2 * e];
    out[1] = v[2 * e + 1];
  }
}

// One wave per (unit, tile).  DIAG: tile (k, k), k = blockIdx.y, the entries a <= b; else tile (bn, bm), bn < bm, the
// blockIdx.y-th pair in the order (0,1), (0,2), (1,2), (0,3) ...
template <int B, bool DIAG, int CW>
__global__ __launch_bounds__(64) void ph_gram_kernel(PhTables t, const double* __restrict__ v, int al16, double* __restrict__ partial) {
  constexpr int NA = DIAG ? B * (B + 1) / 2 : B * B;
  const PhUnit u = t.units[blockIdx.x];
  int bn = (int)blockIdx.y, bm = (int)blockIdx.y;
  if (!DIAG) {
    bm = 1;
    int k = (int)blockIdx.y;
    while (k >= bm) {
      k -= bm;
      bm++;
    }
    bn = k;
  }
  const int n0 = bn * B, m0 = bm * B, dimph = t.dimph;
  double acc[NA][CW];
#pragma unroll
  for (int k = 0; k < NA; k++)
#pragma unroll
    for (int c = 0; c < CW; c++) acc[k][c] = 0.0;
  const int lane = threadIdx.x;
  const uint32_t nc = (uint32_t)u.ncols, q64 = 64u / nc, r64 = 64u % nc;
  uint32_t p = (uint32_t)u.p0 + lane, r = p / nc, j = p - r * nc;
#pragma unroll 1
  for (; p < (uint32_t)u.p1; p += 64) {
    const int64_t e = (int64_t)t.rorder[u.r0 + r] * t.dim_cols + t.corder[u.c0 + j];
    double x[B][CW], y[B][CW];
#pragma unroll
    for (int a = 0; a < B; a++) {
#pragma unroll
      for (int c = 0; c < CW; c++) x[a][c] = 0.0;
      if (n0 + a < dimph) ph_load<CW>(v, e + (int64_t)(n0 + a) * t.dim_el, al16, x[a]);
    }
    if (!DIAG) {
#pragma unroll
      for (int b = 0; b < B; b++) {
#pragma unroll
        for (int c = 0; c < CW; c++) y[b][c] = 0.0;
        if (m0 + b < dimph) ph_load<CW>(v, e + (int64_t)(m0 + b) * t.dim_el, al16, y[b]);
      }
    }
    int k = 0;
#pragma unroll
    for (int a = 0; a < B; a++)
#pragma unroll
      for (int b = DIAG ? a : 0; b < B; b++, k++) {
        const double* ya = DIAG ? x[b] : y[b];
        if (CW == 1) {
          acc[k][0] = __builtin_fma(x[a][0], ya[0], acc[k][0]);
        } else {  // v_n conj v_m
          acc[k][0] = __builtin_fma(x[a][0], ya[0], acc[k][0]);
          acc[k][0] = __builtin_fma(x[a][CW - 1], ya[CW - 1], acc[k][0]);
          acc[k][CW - 1] = __builtin_fma(x[a][CW - 1], ya[0], acc[k][CW - 1]);
          acc[k][CW - 1] = __builtin_fma(-x[a][0], ya[CW - 1], acc[k][CW - 1]);
        }
      }
    r += q64;
    j += r64;
    if (j >= nc) {
      j -= nc;
      r++;
    }
  }
#pragma unroll
  for (int k = 0; k < NA; k++)
#pragma unroll
    for (int c = 0; c < CW; c++)
      for (int off = 32; off > 0; off >>= 1) acc[k][c] += __shfl_xor(acc[k][c], off, 64);
  if (lane == 0) {
    double* out = partial + (int64_t)blockIdx.x * (dimph * (dimph + 1) / 2) * CW;
    int k = 0;
#pragma unroll
    for (int a = 0; a < B; a++)
#pragma unroll
      for (int b = DIAG ? a : 0; b < B; b++, k++) {
        const int n = n0 + a, m = m0 + b;
        if (n < dimph && m < dimph) {
          const int slot = n * dimph - n * (n - 1) / 2 + (m - n);
#pragma unroll
          for (int c = 0; c < CW; c++) out[slot * CW + c] = acc[k][c];
        }
      }
  }
}

// sums[c][s] = the partial sums of the units of class c, in unit order
__global__ __launch_bounds__(256) void ph_final_kernel(PhTables t, int nslot, const double* __restrict__ partial, double* __restrict__ sums) {
  const int c = blockIdx.x, u0 = t.ubeg[c], u1 = t.ubeg[c + 1];
  for (int s = threadIdx.x; s < nslot; s += 256) {
    double r = 0.0;
    for (int u = u0; u < u1; u++) r += partial[(int64_t)u * nslot + s];
    sums[(int64_t)c * nslot + s] = r;
  }
}

inline bool ph_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int B, int CW>
void launch_gram(const PhTables& t, const double* v, int al16, double* partial, hipStream_t st) {
  const int nb = (t.dimph + B - 1) / B;
  ph_gram_kernel<B, true, CW><<<dim3((unsigned)t.nunits, (unsigned)nb), 64, 0, st>>>(t, v, al16, partial);
}

}  // namespace

int launch_apply_xph(const PhTables& t, const double* src, double* dst, hipStream_t st) {
  const int cw = t.cplx ? 2 : 1;
  const int64_t stride = t.dim_el * cw;
  if (stride <= 0 || t.dimph < 2) return 0;
  const bool al = ph_aligned16(src) && ph_aligned16(dst);
  const bool vec = al && (stride % 2 == 0);
  const int w = (t.cplx || vec) ? 2 : 1;
  const int64_t nitem = stride / w;
  const unsigned grid = (unsigned)std::min<int64_t>((nitem + kXphBlock - 1) / kXphBlock, 1 << 20);
  if (vec) apply_xph_kernel<2, true><<<grid, kXphBlock, 0, st>>>(t.dimph, stride, nitem, t.sq, src, dst);
  else if (w == 2) apply_xph_kernel<2, false><<<grid, kXphBlock, 0, st>>>(t.dimph, stride, nitem, t.sq, src, dst);
  else apply_xph_kernel<1, false><<<grid, kXphBlock, 0, st>>>(t.dimph, stride, nitem, t.sq, src, dst);
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

int launch_ph_rdm(const PhTables& t, const double* v, double* partial, double* sums, hipStream_t st) {
  const int cw = t.cplx ? 2 : 1, nslot = t.dimph * (t.dimph + 1) / 2 * cw;
  const int al16 = ph_aligned16(v) ? 1 : 0;
  if (t.nunits > 0) {
    if (t.cplx) {
      if (t.dimph <= 4) launch_gram<4, 2>(t, v, al16, partial, st);
      else launch_gram<8, 2>(t, v, al16, partial, st);
    } else {
      if (t.dimph <= 4) launch_gram<4, 1>(t, v, al16, partial, st);
      else if (t.dimph <= 8) launch_gram<8, 1>(t, v, al16, partial, st);
      else if (t.dimph <= 16) launch_gram<16, 1>(t, v, al16, partial, st);
      else launch_gram<8, 1>(t, v, al16, partial, st);
    }
    EDIGPU_HIP(hipGetLastError());
    const bool tiled = t.dimph > (t.cplx ? 8 : 16);
    if (tiled) {
      const int nb = (t.dimph + 7) / 8;
      const dim3 grid((unsigned)t.nunits, (unsigned)(nb * (nb - 1) / 2));
      if (t.cplx) ph_gram_kernel<8, false, 2><<<grid, 64, 0, st>>>(t, v, al16, partial);
      else ph_gram_kernel<8, false, 1><<<grid, 64, 0, st>>>(t, v, al16, partial);
      EDIGPU_HIP(hipGetLastError());
    }
  }
  ph_final_kernel<<<(unsigned)t.ncls, 256, 0, st>>>(t, nslot, partial, sums);
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

}  // namespace edigpu
