// kernels_axisop.hip -- c / c^+ (and sums of them, apply_Cops) as a signed partial permutation along ONE axis of a device
// vector: phonon sectors, complex normal-mode sectors and ed_total_ud=F sectors (apply_op_C / apply_op_CDG / apply_Cops,
// reference ED_SECTOR.f90:465-1130: the iph loop, the _c variants, the ed_total_ud branch).  Tables: host_axisop.hpp.
//
// The vector is a tensor [O][A][I] (I, the extent of the faster axes, is the same in source and destination):
//     dst[o][j][i] = sum_t coef_t s_t(j) src[o][part_t(j)][i],   part_t[j] = source index | minus << 31, 0xFFFFFFFF = none.
// Sign: ed_total_ud=T the host counts the species word below the level; ed_total_ud=F it is always plus, because the
// reference applies c(1, .) to the orbital's own chain word (ipos = 1, ED_SECTOR.f90:487-488, 522), whose bit 0 is the
// impurity (build_orbs): the tables then carry no sign bit.
//
// Arithmetic (fixed, the tests restate it).  x_t = the signed gather of term t, 0 without a preimage, t ascending:
//   real coefficients     acc = coef_0 * x_0, then acc = fma(coef_t, x_t, acc): what one launch of apply_op_normal_kernel
//                         per term computes (dst = coef * x, then dst = fma(coef, x, dst)).  Complex vectors with real
//                         coefficients are this on the interleaved doubles.
//   complex coefficients  (element = double2) y_t = (cre x.re - cim x.im, cre x.im + cim x.re), each product and each sum
//                         rounded (no contraction); acc = y_0, then acc = y_t + acc: apply_op_flat_kernel.
//
//   rows kernel, I >= 64 doubles: a wave owns one (o, j) and one chunk of 128 elements of I, grid-stride.  The partner
//       entries of (o, j) are wave-uniform: one scalar table read per term.  A (o, j) no term reaches is stored as
//       (signed) zeros without a read of src.  Lanes l and l + 64 of a chunk: consecutive lanes on consecutive elements,
//       loads and stores alike.
//   gather kernel, I < 64: the partner per lane; four elements per lane and pass, a grid apart (a wave still stores 64
//       consecutive elements), so that four table reads and then four source reads are in flight; the element index is
//       split with 32-bit divisions where the vector has fewer than 2^31 elements.
// Both: capped grid, no LDS, no atomics; every element of dst is written once and never read, src is only read.
//
// Each kernel has two forms, chosen by the policy Win (shard_src.hpp).  WholeVector: the vectors above (what the single-GPU
// calls launch; `if constexpr` leaves its code as it was).  ShardWindow (edigpu_apply_cops_sharded): the destination holds
// the indices [j_first, j_first + j_count) of axis A only, dst[o][j - j_first][i], the partner table is still indexed by
// the global j, and the source row of (o, part_t(j)) is found through shard_src_offset in the all-gathered shards.  In the
// rows kernel that offset is computed on scalars, once per (unit, term), next to the readfirstlane of the partner; in the
// gather kernel per lane.  Arithmetic and term order are the same in both forms.
#include "kernels.hpp"

namespace edigpu {
namespace {

constexpr int kAxisBlock = 256;
constexpr int kAxisPer = 2;                    // elements per lane of a rows-kernel unit
constexpr int kAxisChunk = 64 * kAxisPer;      // elements of a unit
constexpr int kAxisMaxBlocks = 1024;           // 16 waves per CU on 256 CUs; the rest is grid-stride
constexpr int kAxisBatch = 4;                  // elements per lane and pass of the gather kernel
constexpr uint32_t kNone = 0xFFFFFFFFu, kIdx = 0x7FFFFFFFu;

// one element type per coefficient type: double with real coefficients, double2 with complex ones
struct RealAlg {
  using T = double;
  static __device__ __forceinline__ T zero() { return 0.0; }
  static __device__ __forceinline__ T neg(T x) { return -x; }
  static __device__ __forceinline__ T first(const AxisArgs& a, int t, T x) { return a.cre[t] * x; }
  static __device__ __forceinline__ T next(const AxisArgs& a, int t, T x, T acc) { return __builtin_fma(a.cre[t], x, acc); }
};
struct CplxAlg {
  using T = double2;
  static __device__ __forceinline__ T zero() { return make_double2(0.0, 0.0); }
  static __device__ __forceinline__ T neg(T x) { return make_double2(-x.x, -x.y); }
  static __device__ __forceinline__ T first(const AxisArgs& a, int t, T x) {
    return make_double2(a.cre[t] * x.x - a.cim[t] * x.y, a.cre[t] * x.y + a.cim[t] * x.x);
  }
  static __device__ __forceinline__ T next(const AxisArgs& a, int t, T x, T acc) {
    const T y = first(a, t, x);
    return make_double2(y.x + acc.x, y.y + acc.y);
  }
};

// a.I is counted in elements of Alg::T here (launch_apply_axisop halves it for double2)
template <class Alg, class Win>
__global__ __launch_bounds__(kAxisBlock) void axisop_rows_kernel(AxisArgs a, Win w, const typename Alg::T* __restrict__ src,
                                                                 typename Alg::T* __restrict__ dst) {
  using T = typename Alg::T;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  constexpr int kWaves = kAxisBlock / 64;
  const int64_t nchunks = (a.I + kAxisChunk - 1) / kAxisChunk;
  int64_t na = a.a_dst, j0 = 0;  // destination rows per o, the first of them
  if constexpr (Win::kWindow) {
    na = w.j_count;
    j0 = w.j_first;
  }
  const int64_t nunits = a.O * na * nchunks;
  for (int64_t u = (int64_t)blockIdx.x * kWaves + wave; u < nunits; u += (int64_t)gridDim.x * kWaves) {
    const int64_t row = u / nchunks, c0 = (u - row * nchunks) * kAxisChunk;
    const int64_t o = row / na, j = row - o * na + j0;
    T acc[kAxisPer];
    for (int t = 0; t < a.nterms; t++) {
      // the partner of (o, j) under term t: the same for every lane
      const uint32_t p = __builtin_amdgcn_readfirstlane(a.part[t * a.a_dst + j]);
      T x[kAxisPer];
#pragma unroll
      for (int c = 0; c < kAxisPer; c++) x[c] = Alg::zero();
      if (p != kNone) {
        const T* srow;
        if constexpr (Win::kWindow) srow = src + shard_src_offset(w.s, o, (int64_t)(p & kIdx));  // (wave-uniform)
        else srow = src + (o * a.a_src + (int64_t)(p & kIdx)) * a.I;
#pragma unroll
        for (int c = 0; c < kAxisPer; c++) {  // the loads of a term are independent
          const int64_t i = c0 + lane + 64 * c;
          if (i < a.I) x[c] = srow[i];
        }
        if (p >> 31) {
#pragma unroll
          for (int c = 0; c < kAxisPer; c++) x[c] = Alg::neg(x[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < kAxisPer; c++) acc[c] = t == 0 ? Alg::first(a, 0, x[c]) : Alg::next(a, t, x[c], acc[c]);
    }
    T* drow = dst + row * a.I;
#pragma unroll
    for (int c = 0; c < kAxisPer; c++) {
      const int64_t i = c0 + lane + 64 * c;
      if (i < a.I) drow[i] = acc[c];
    }
  }
}

// Ix: the type the element index is split in.  The two divisions per element are what this kernel spends its
// instructions on, so vectors of fewer than 2^31 elements take them in 32 bits; the addresses are 64-bit either way.
template <class Alg, class Ix, class Win>
__global__ __launch_bounds__(kAxisBlock) void axisop_gather_kernel(AxisArgs a, Win w, const typename Alg::T* __restrict__ src,
                                                                   typename Alg::T* __restrict__ dst) {
  using T = typename Alg::T;
  Ix na = (Ix)a.a_dst, j0 = 0;  // destination rows per o, the first of them
  if constexpr (Win::kWindow) {
    na = (Ix)w.j_count;
    j0 = (Ix)w.j_first;
  }
  const Ix nI = (Ix)a.I;
  const Ix nel = (Ix)(a.O * (int64_t)na * a.I), step = (Ix)gridDim.x * kAxisBlock;
  // kAxisBatch elements per lane and pass, a grid apart: the table reads of a batch are in flight together, then its
  // source reads (each element is two dependent loads; one element per pass leaves the memory system waiting)
  for (Ix e0 = (Ix)blockIdx.x * kAxisBlock + threadIdx.x; e0 < nel; e0 += kAxisBatch * step) {
    Ix j[kAxisBatch];
    int64_t base[kAxisBatch];  // offset of (o, row 0, i) in src; window form: i, with the block o kept beside it
    [[maybe_unused]] int64_t blk[kAxisBatch];
    bool in[kAxisBatch];
    T acc[kAxisBatch];
#pragma unroll
    for (int b = 0; b < kAxisBatch; b++) {
      const Ix e = e0 + (Ix)b * step;
      in[b] = e < nel;
      const Ix row = e / nI, i = e - row * nI;
      const Ix o = row / na;
      j[b] = row - o * na + j0;
      if constexpr (Win::kWindow) {
        base[b] = (int64_t)i;
        blk[b] = (int64_t)o;
      } else {
        base[b] = (int64_t)o * a.a_src * a.I + (int64_t)i;
      }
    }
    for (int t = 0; t < a.nterms; t++) {
      uint32_t p[kAxisBatch];
      T x[kAxisBatch];
#pragma unroll
      for (int b = 0; b < kAxisBatch; b++) p[b] = in[b] ? a.part[t * a.a_dst + (int64_t)j[b]] : kNone;
#pragma unroll
      for (int b = 0; b < kAxisBatch; b++) {
        x[b] = Alg::zero();
        if (p[b] != kNone) {
          if constexpr (Win::kWindow) x[b] = src[shard_src_offset(w.s, blk[b], (int64_t)(p[b] & kIdx)) + base[b]];
          else x[b] = src[base[b] + (int64_t)(p[b] & kIdx) * a.I];
        }
      }
#pragma unroll
      for (int b = 0; b < kAxisBatch; b++) {
        if (p[b] != kNone && (p[b] >> 31)) x[b] = Alg::neg(x[b]);
        acc[b] = t == 0 ? Alg::first(a, 0, x[b]) : Alg::next(a, t, x[b], acc[b]);
      }
    }
#pragma unroll
    for (int b = 0; b < kAxisBatch; b++)
      if (in[b]) dst[e0 + (Ix)b * step] = acc[b];
  }
}

template <class Alg, class Win>
void axisop_launch(const AxisArgs& a, const Win& w, bool rows, const double* src, double* dst, hipStream_t st) {
  using T = typename Alg::T;
  int64_t na = a.a_dst;
  if constexpr (Win::kWindow) na = w.j_count;
  const int64_t nrows = a.O * na, nel = nrows * a.I;
  if (rows) {
    const int64_t nunits = nrows * ((a.I + kAxisChunk - 1) / kAxisChunk), per = kAxisBlock / 64;
    const unsigned grid = (unsigned)std::min<int64_t>((nunits + per - 1) / per, kAxisMaxBlocks);
    axisop_rows_kernel<Alg, Win><<<grid, kAxisBlock, 0, st>>>(a, w, reinterpret_cast<const T*>(src), reinterpret_cast<T*>(dst));
  } else {
    const int64_t per = (int64_t)kAxisBlock * kAxisBatch;
    const unsigned grid = (unsigned)std::min<int64_t>((nel + per - 1) / per, kAxisMaxBlocks);
    if (nel < ((int64_t)1 << 31))  // a pass adds at most 4 * 2^18 to an index below 2^31: no wrap in 32 bits
      axisop_gather_kernel<Alg, uint32_t, Win><<<grid, kAxisBlock, 0, st>>>(a, w, reinterpret_cast<const T*>(src), reinterpret_cast<T*>(dst));
    else
      axisop_gather_kernel<Alg, int64_t, Win><<<grid, kAxisBlock, 0, st>>>(a, w, reinterpret_cast<const T*>(src), reinterpret_cast<T*>(dst));
  }
}

}  // namespace

int launch_apply_axisop(const AxisArgs& args, int cplx_coef, const double* src, double* dst, hipStream_t st) {
  if (args.O * args.a_dst * args.I <= 0) return 0;
  if (args.nterms < 1 || args.nterms > 8 || (cplx_coef && (args.I & 1))) {
    set_error("launch_apply_axisop: bad argument");
    return 1;
  }
  const bool rows = args.I >= 64;  // in doubles, whichever the element type
  if (cplx_coef) {
    AxisArgs a = args;
    a.I /= 2;
    axisop_launch<CplxAlg>(a, WholeVector(), rows, src, dst, st);
  } else {
    axisop_launch<RealAlg>(args, WholeVector(), rows, src, dst, st);
  }
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

int launch_apply_axisop_window(const AxisArgs& args, const ShardWindow& win, int cplx_coef, const double* src, double* dst,
                               hipStream_t st) {
  if (args.O * win.j_count * args.I <= 0) return 0;
  const ShardSrc& s = win.s;
  // every source row the tables can name lies inside the gathered vector, every destination row inside the axis
  if (args.nterms < 1 || args.nterms > 8 || (cplx_coef && ((args.I | s.chunk) & 1)) || win.j_first < 0 ||
      win.j_first + win.j_count > args.a_dst || s.nblk != args.O || s.unit_len != args.I || s.units != args.a_src || s.q < 1 ||
      s.chunk != s.q * s.unit_len * s.nblk) {
    set_error("launch_apply_axisop_window: bad argument");
    return 1;
  }
  const bool rows = args.I >= 64;  // in doubles, whichever the element type
  if (cplx_coef) {
    AxisArgs a = args;
    a.I /= 2;
    ShardWindow w = win;
    w.s = shard_src_in_pairs(s);
    axisop_launch<CplxAlg>(a, w, rows, src, dst, st);
  } else {
    axisop_launch<RealAlg>(args, win, rows, src, dst, st);
  }
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

}  // namespace edigpu
