// kernels_twin.hip -- the ED_TWIN=T reorder of eigenvectors on the device (edigpu_twin.hip; host_twin.hpp): the vector of
// the twin sector B from the vector of the stored sector A, v_B[i] = v_A[order_A(i)] phonon block by phonon block
// (es_return_dvector, ED_EIGENSPACE.f90:652-720; twin_sector_order, ED_SECTOR.f90:1747-1776).  A pure permutation: no
// arithmetic, the results are the source's bits.
//
//   normal mode    B's (iup, idw) is A's (idw, iup): every phonon block [R = DimDw_A][C = DimUp_A] (C fastest) becomes its
//                  transpose [C][R].  twin_transpose_kernel: one workgroup of 256 moves a tile of 512 B x 512 B (64 x 64
//                  doubles, 32 x 32 double2) through the LDS, so both the reads (along C) and the writes (along R) are
//                  whole 512-B row segments.  The tile's rows are padded by one element: the transposed LDS reads of a
//                  32-lane group (ds_read_b64; 16-lane group of ds_read_b128) then fall on 64 different banks.
//   superc         twin_gather_kernel<T, false>: v_dst[i] = v_src[order[i]] with the handle's table.
//   nonsu2         twin_gather_kernel<T, true>:  v_dst[i] = v_src[n - 1 - i].
//
// Both kernels have the two forms of shard_src.hpp: WholeVector, and ShardWindow -- the destination units [first, first +
// count) (B's down rows = A's up columns; rows of superc / nonsu2) written as a rank's shard [nvec][nblk][count][..], the
// source the all-gather of the ranks' chunks, read through shard_src_offset.
#include <algorithm>

#include "kernels.hpp"

namespace edigpu {
namespace {

constexpr int kTwinBlock = 256;

struct TwinShape {
  int64_t R = 0, C = 0;          // source rows (DimDw_A) and columns (DimUp_A)
  int64_t first = 0, count = 0;  // the source columns = destination rows this launch writes
  int64_t vstride = 0;           // elements from one source vector to the next
  int nblk = 1;
};

template <class T>
struct TwinTile {
  static constexpr int kTile = 512 / (int)sizeof(T);
};

// RV / WV: the reads / the writes move 16 bytes.  double: two elements at a time, which needs an even row length, an even
// first column and a 16-byte aligned pointer (launch_transpose); double2: the pointer is 16-byte aligned, else the element
// moves as two doubles.
template <class T, bool RV, bool WV, class Form>
__global__ __launch_bounds__(kTwinBlock) void twin_transpose_kernel(TwinShape g, ShardSrc s, const T* __restrict__ src,
                                                                    T* __restrict__ dst) {
  constexpr int TL = TwinTile<T>::kTile;
  constexpr bool kReal = sizeof(T) == sizeof(double);
  __shared__ T tile[TL][TL + 1];
  __shared__ int64_t rowoff[TL];
  const int tid = threadIdx.x;
  const int64_t k = blockIdx.z / g.nblk, p = blockIdx.z % g.nblk;
  const int64_t c0 = g.first + (int64_t)blockIdx.x * TL, cend = g.first + g.count;
  const int64_t r0 = (int64_t)blockIdx.y * TL;
  if (tid < TL && r0 + tid < g.R) {
    if constexpr (Form::kWindow) rowoff[tid] = shard_src_offset(s, p, r0 + tid);
    else rowoff[tid] = (p * g.R + r0 + tid) * g.C;
  }
  __syncthreads();
  const T* sv = src + k * g.vstride;
  {
    constexpr int NR = (kReal && RV) ? 2 : 1;  // elements per access
    constexpr int APR = TL / NR, RPP = kTwinBlock / APR;
    const int cc = (tid % APR) * NR;
    for (int rr = tid / APR; rr < TL; rr += RPP) {
      if (r0 + rr >= g.R || c0 + cc >= cend) continue;
      const T* ptr = sv + rowoff[rr] + c0 + cc;
      if constexpr (NR == 2) {
        // (C is even and c0 + cc is even: the second element is inside the row, whether or not inside the window)
        const double2 x = *reinterpret_cast<const double2*>(ptr);
        tile[rr][cc] = x.x;
        tile[rr][cc + 1] = x.y;
      } else if constexpr (!kReal && !RV) {
        const double* q = reinterpret_cast<const double*>(ptr);
        tile[rr][cc] = make_double2(q[0], q[1]);
      } else {
        tile[rr][cc] = *ptr;
      }
    }
  }
  __syncthreads();
  const int64_t d0 = ((k * g.nblk + p) * g.count - g.first) * g.R;  // element (c, r) at d0 + c R + r
  if constexpr (kReal && WV) {
    // a 32-lane group reads 16 row pairs of two columns: dword 260 lane16 + 2 colbit (mod 64), 64 banks once
    const int lane16 = tid & 15, colbit = (tid >> 4) & 1, half = (tid >> 5) & 1, wave = tid >> 6;
    const int rr = 2 * (lane16 + 16 * half);
    if (r0 + rr < g.R) {  // (R is even: the pair is inside)
#pragma unroll
      for (int it = 0; it < TL / 8; it++) {
        const int cc = colbit + 2 * wave + 8 * it;
        if (c0 + cc < cend)
          *reinterpret_cast<double2*>(dst + (d0 + (c0 + cc) * g.R + r0 + rr)) = make_double2(tile[rr][cc], tile[rr + 1][cc]);
      }
    }
  } else {
    constexpr int CPP = kTwinBlock / TL;  // columns per pass
    const int rr = tid % TL;
    if (r0 + rr < g.R) {
#pragma unroll
      for (int it = 0; it < TL / CPP; it++) {
        const int cc = tid / TL + CPP * it;
        if (c0 + cc >= cend) continue;
        T* ptr = dst + (d0 + (c0 + cc) * g.R + r0 + rr);
        if constexpr (!kReal && !WV) {
          double* q = reinterpret_cast<double*>(ptr);
          const T x = tile[rr][cc];
          q[0] = x.x;
          q[1] = x.y;
        } else {
          *ptr = tile[rr][cc];
        }
      }
    }
  }
}

struct TwinRows {
  int64_t n = 0;                 // electronic rows of the sector
  int64_t first = 0, count = 0;  // the destination rows this launch writes
  int64_t vstride = 0;           // rows from one source vector to the next
  int nblk = 1;
  int wshift = 0;                // a row is 1 << wshift elements of T (complex rows moved as two doubles)
};

// one thread per destination element: consecutive lanes write consecutive addresses; the reads follow the table
template <class T, bool REVERSE, class Form>
__global__ __launch_bounds__(kTwinBlock) void twin_gather_kernel(TwinRows g, ShardSrc s, const int32_t* __restrict__ order,
                                                                 const T* __restrict__ src, T* __restrict__ dst) {
  const int64_t e = (int64_t)blockIdx.x * kTwinBlock + threadIdx.x;
  if (e >= (g.count << g.wshift)) return;
  const int64_t k = blockIdx.y / g.nblk, p = blockIdx.y % g.nblk;
  const int64_t i = g.first + (e >> g.wshift), j = e & (((int64_t)1 << g.wshift) - 1);
  int64_t from;
  if constexpr (REVERSE) from = g.n - 1 - i;
  else from = order[i];
  int64_t off;
  if constexpr (Form::kWindow) off = shard_src_offset(s, p, from);
  else off = p * g.n + from;
  dst[(((k * g.nblk + p) * g.count) << g.wshift) + e] = src[((k * g.vstride + off) << g.wshift) + j];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <class T, class Form>
void transpose_launch(const TwinShape& g, const ShardSrc& s, bool rv, bool wv, int nvec, const void* src, void* dst, hipStream_t st) {
  constexpr int TL = TwinTile<T>::kTile;
  const dim3 grid((unsigned)((g.count + TL - 1) / TL), (unsigned)((g.R + TL - 1) / TL), (unsigned)(nvec * g.nblk));
  const T* a = static_cast<const T*>(src);
  T* b = static_cast<T*>(dst);
  if (rv && wv) twin_transpose_kernel<T, true, true, Form><<<grid, kTwinBlock, 0, st>>>(g, s, a, b);
  else if (rv) twin_transpose_kernel<T, true, false, Form><<<grid, kTwinBlock, 0, st>>>(g, s, a, b);
  else if (wv) twin_transpose_kernel<T, false, true, Form><<<grid, kTwinBlock, 0, st>>>(g, s, a, b);
  else twin_transpose_kernel<T, false, false, Form><<<grid, kTwinBlock, 0, st>>>(g, s, a, b);
}

template <class Form>
int transpose_any(int cplx, TwinShape g, const ShardSrc& s, int nvec, const void* src, void* dst, hipStream_t st, const char* who) {
  if (g.R <= 0 || g.count <= 0) return 0;
  const int64_t tl = cplx ? TwinTile<double2>::kTile : TwinTile<double>::kTile;
  if (nvec < 1 || g.nblk < 1 || (int64_t)nvec * g.nblk > 65535 || (g.R + tl - 1) / tl > 65535 || g.first < 0 ||
      g.first + g.count > g.C) {
    set_error(std::string(who) + ": bad argument");
    return 1;
  }
  if (cplx) {
    transpose_launch<double2, Form>(g, s, aligned16(src), aligned16(dst), nvec, src, dst, st);
  } else {
    // every row of the source starts on an even element when C is even (shard chunks and vector strides are multiples
    // of C), every row of the destination when R is
    const bool rv = aligned16(src) && g.C % 2 == 0 && g.first % 2 == 0;
    const bool wv = aligned16(dst) && g.R % 2 == 0;
    transpose_launch<double, Form>(g, s, rv, wv, nvec, src, dst, st);
  }
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

template <class T, class Form>
void gather_launch(const TwinRows& g, const ShardSrc& s, const int32_t* order, int nvec, const void* src, void* dst, hipStream_t st) {
  const int64_t nel = g.count << g.wshift;
  const dim3 grid((unsigned)((nel + kTwinBlock - 1) / kTwinBlock), (unsigned)(nvec * g.nblk));
  const T* a = static_cast<const T*>(src);
  T* b = static_cast<T*>(dst);
  if (order) twin_gather_kernel<T, false, Form><<<grid, kTwinBlock, 0, st>>>(g, s, order, a, b);
  else twin_gather_kernel<T, true, Form><<<grid, kTwinBlock, 0, st>>>(g, s, order, a, b);
}

template <class Form>
int gather_any(int cplx, TwinRows g, const ShardSrc& s, const int32_t* order, int nvec, const void* src, void* dst, hipStream_t st,
               const char* who) {
  if (g.count <= 0) return 0;
  if (nvec < 1 || g.nblk < 1 || (int64_t)nvec * g.nblk > 65535 || g.first < 0 || g.first + g.count > g.n ||
      g.count > ((int64_t)1 << 38)) {
    set_error(std::string(who) + ": bad argument");
    return 1;
  }
  if (cplx && aligned16(src) && aligned16(dst)) {
    gather_launch<double2, Form>(g, s, order, nvec, src, dst, st);
  } else {
    g.wshift = cplx ? 1 : 0;
    gather_launch<double, Form>(g, s, order, nvec, src, dst, st);
  }
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

// the gathered source of a window launch: nvec vectors per rank, each rank's part nvec * (q unit_len nblk) elements
bool window_ok(const ShardWindow& w, int64_t units, int64_t unit_len, int nvec, int64_t vstride) {
  const ShardSrc& s = w.s;
  return s.q >= 1 && s.units == units && s.unit_len == unit_len && s.nblk >= 1 && vstride == s.q * s.unit_len * s.nblk &&
         s.chunk == (int64_t)nvec * vstride;
}

}  // namespace

int launch_twin_transpose(int cplx, int64_t R, int64_t C, int nblk, int nvec, const void* src, void* dst, hipStream_t st) {
  TwinShape g;
  g.R = R;
  g.C = C;
  g.first = 0;
  g.count = C;
  g.nblk = nblk;
  g.vstride = R * C * nblk;
  return transpose_any<WholeVector>(cplx, g, ShardSrc(), nvec, src, dst, st, "launch_twin_transpose");
}

int launch_twin_transpose_window(int cplx, int64_t R, int64_t C, int nvec, const ShardWindow& w, int64_t vstride, const void* src,
                                 void* dst, hipStream_t st) {
  if (!window_ok(w, R, C, nvec, vstride)) {
    set_error("launch_twin_transpose_window: bad argument");
    return 1;
  }
  TwinShape g;
  g.R = R;
  g.C = C;
  g.first = w.j_first;
  g.count = w.j_count;
  g.nblk = w.s.nblk;
  g.vstride = vstride;
  return transpose_any<ShardWindow>(cplx, g, w.s, nvec, src, dst, st, "launch_twin_transpose_window");
}

int launch_twin_gather(int cplx, int64_t n, int nblk, int nvec, const int32_t* order, const void* src, void* dst, hipStream_t st) {
  TwinRows g;
  g.n = n;
  g.first = 0;
  g.count = n;
  g.nblk = nblk;
  g.vstride = n * nblk;
  return gather_any<WholeVector>(cplx, g, ShardSrc(), order, nvec, src, dst, st, "launch_twin_gather");
}

int launch_twin_gather_window(int cplx, int64_t n, int nvec, const ShardWindow& w, int64_t vstride, const int32_t* order,
                              const void* src, void* dst, hipStream_t st) {
  if (!window_ok(w, n, 1, nvec, vstride)) {
    set_error("launch_twin_gather_window: bad argument");
    return 1;
  }
  TwinRows g;
  g.n = n;
  g.first = w.j_first;
  g.count = w.j_count;
  g.nblk = w.s.nblk;
  g.vstride = vstride;
  return gather_any<ShardWindow>(cplx, g, w.s, order, nvec, src, dst, st, "launch_twin_gather_window");
}

}  // namespace edigpu
