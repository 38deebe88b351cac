// kernels_pairs.hip -- products of two c / c^+ on normal-mode device vectors in one pass (edigpu_apply_pairs_normal): the
// seeds of the pair and exciton susceptibilities, c_{a,up} c_{a,dw}|gs>, c^+_{a,s} c_{b,s}|gs> summed over the spin,
// c^+_{a,dw} c_{b,up}|gs>, ... (ED_NORMAL/ED_CHI_PAIR.f90:129-241, ED_CHI_EXCT.f90:178-235, 513-592).
//
// O2 O1 is a signed partial permutation P_dw (x) P_up of V[idw][iup] (host_pairs.hpp), so for every phonon block p
//     dst[p][jdw][jup] = sum_t coef_t s_t src[p][pd_t(jdw)][pu_t(jup)],   s_t = sign(pd_t(jdw)) xor sign(pu_t(jup)).
// Summation order (fixed, relied on by the tests): acc = 0, then for t ascending acc = fma(coef_t, +-x_t, acc); a term
// without a preimage adds nothing.  The destination is written once and never read; the source is only read.
//
//   rows kernel (rows of at least one wave): a wave owns (destination row, chunk of 128 columns), grid-stride.  The down
//       partners of the row are wave-uniform (one scalar table entry per term); a row in which no term has a down
//       partner is stored as zeros without a read of src.  The up tables are shared by all rows (L2).  On the
//       combination-ordered basis the up partner index rises with the column over the live entries, so a wave's gather
//       touches a short run of the source row: a plain global gather.
//   flat kernel (rows shorter than a wave): one element per lane, grid-stride, both partners per lane.
// Stores are 8 bytes per lane, consecutive lanes on consecutive elements, so vectors need 8-byte alignment only.
#include "kernels.hpp"

namespace edigpu {
namespace {

constexpr int kPairsBlock = 256;
constexpr int kPairsCols = 2;                      // columns per lane of a rows-kernel unit
constexpr int kPairsChunk = 64 * kPairsCols;       // columns of a unit
constexpr int kPairsMaxBlocks = 1024;              // 16 waves per CU on 256 CUs; the rest is grid-stride
constexpr uint32_t kNone = 0xFFFFFFFFu, kIdx = 0x7FFFFFFFu;

// Win (shard_src.hpp): WholeVector = the vectors above; ShardWindow (edigpu_apply_pairs_sharded) = the destination holds
// the down rows [j_first, j_first + j_count) of every block, the down tables are indexed by the global row and the source
// row pd_t(jdw) of block p is found through shard_src_offset in the all-gathered shards (on scalars in the rows kernel,
// per lane in the flat kernel).  The up tables, the arithmetic and the term order are the same in both forms.
template <class Win>
__global__ __launch_bounds__(kPairsBlock) void pairs_rows_kernel(PairsArgs a, Win w, const double* __restrict__ src,
                                                                 double* __restrict__ dst) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  constexpr int kWaves = kPairsBlock / 64;
  const int64_t nchunks = (a.du_dst + kPairsChunk - 1) / kPairsChunk;
  int64_t nd = a.dd_dst, j0 = 0;  // destination rows per block, the first of them
  if constexpr (Win::kWindow) {
    nd = w.j_count;
    j0 = w.j_first;
  }
  const int64_t nunits = nd * a.nblk * nchunks;
  for (int64_t u = (int64_t)blockIdx.x * kWaves + wave; u < nunits; u += (int64_t)gridDim.x * kWaves) {
    const int64_t row = u / nchunks, c0 = (u - row * nchunks) * kPairsChunk;
    const int64_t blk = row / nd, jdw = row - blk * nd + j0;
    double acc[kPairsCols];
#pragma unroll
    for (int c = 0; c < kPairsCols; c++) acc[c] = 0.0;
    for (int t = 0; t < a.nterms; t++) {
      // the row's down partner under term t: the same for every lane
      const uint32_t pd = ((a.id_dw >> t) & 1u) ? (uint32_t)jdw : __builtin_amdgcn_readfirstlane(a.pd[t * a.dd_dst + jdw]);
      if (pd == kNone) continue;
      const double* srow;
      if constexpr (Win::kWindow) srow = src + shard_src_offset(w.s, blk, (int64_t)(pd & kIdx));  // (wave-uniform)
      else srow = src + (blk * a.dd_src + (int64_t)(pd & kIdx)) * a.du_src;
      const bool id_up = (a.id_up >> t) & 1u;
      const uint32_t* put = a.pu + t * a.du_dst;
      const double coef = a.coef[t];
      double x[kPairsCols];
      bool live[kPairsCols];
#pragma unroll
      for (int c = 0; c < kPairsCols; c++) {  // the loads of a term are independent
        const int64_t j = c0 + lane + 64 * c;
        x[c] = 0.0;
        live[c] = false;
        if (j < a.du_dst) {
          const uint32_t pu = id_up ? (uint32_t)j : put[j];
          if (pu != kNone) {
            live[c] = true;
            const double y = srow[pu & kIdx];
            x[c] = ((pu ^ pd) >> 31) ? -y : y;
          }
        }
      }
#pragma unroll
      for (int c = 0; c < kPairsCols; c++)
        if (live[c]) acc[c] = __builtin_fma(coef, x[c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < kPairsCols; c++) {
      const int64_t j = c0 + lane + 64 * c;
      if (j < a.du_dst) dst[row * a.du_dst + j] = acc[c];
    }
  }
}

template <class Win>
__global__ __launch_bounds__(kPairsBlock) void pairs_flat_kernel(PairsArgs a, Win w, const double* __restrict__ src,
                                                                 double* __restrict__ dst) {
  int64_t nd = a.dd_dst, j0 = 0;  // destination rows per block, the first of them
  if constexpr (Win::kWindow) {
    nd = w.j_count;
    j0 = w.j_first;
  }
  const int64_t nel = a.du_dst * nd * a.nblk;
  for (int64_t e = (int64_t)blockIdx.x * kPairsBlock + threadIdx.x; e < nel; e += (int64_t)gridDim.x * kPairsBlock) {
    const int64_t row = e / a.du_dst, j = e - row * a.du_dst;
    const int64_t blk = row / nd, jdw = row - blk * nd + j0;
    double acc = 0.0;
    for (int t = 0; t < a.nterms; t++) {
      const uint32_t pd = ((a.id_dw >> t) & 1u) ? (uint32_t)jdw : a.pd[t * a.dd_dst + jdw];
      const uint32_t pu = ((a.id_up >> t) & 1u) ? (uint32_t)j : a.pu[t * a.du_dst + j];
      if (pd == kNone || pu == kNone) continue;
      int64_t srow;
      if constexpr (Win::kWindow) srow = shard_src_offset(w.s, blk, (int64_t)(pd & kIdx));
      else srow = (blk * a.dd_src + (int64_t)(pd & kIdx)) * a.du_src;
      const double y = src[srow + (int64_t)(pu & kIdx)];
      acc = __builtin_fma(a.coef[t], ((pu ^ pd) >> 31) ? -y : y, acc);
    }
    dst[e] = acc;
  }
}

template <class Win>
int pairs_launch(const PairsArgs& a, const Win& w, const double* src, double* dst, hipStream_t st) {
  int64_t nd = a.dd_dst;
  if constexpr (Win::kWindow) nd = w.j_count;
  const int64_t nrows = nd * a.nblk, nel = nrows * a.du_dst;
  if (nel <= 0) return 0;
  if (a.du_dst >= 64) {
    const int64_t nunits = nrows * ((a.du_dst + kPairsChunk - 1) / kPairsChunk), per = kPairsBlock / 64;
    const unsigned grid = (unsigned)std::min<int64_t>((nunits + per - 1) / per, kPairsMaxBlocks);
    pairs_rows_kernel<Win><<<grid, kPairsBlock, 0, st>>>(a, w, src, dst);
  } else {
    const unsigned grid = (unsigned)std::min<int64_t>((nel + kPairsBlock - 1) / kPairsBlock, kPairsMaxBlocks);
    pairs_flat_kernel<Win><<<grid, kPairsBlock, 0, st>>>(a, w, src, dst);
  }
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

}  // namespace

int launch_apply_pairs(const PairsArgs& a, const double* src, double* dst, hipStream_t st) {
  return pairs_launch(a, WholeVector(), src, dst, st);
}

int launch_apply_pairs_window(const PairsArgs& a, const ShardWindow& w, const double* src, double* dst, hipStream_t st) {
  const ShardSrc& s = w.s;
  // every source row the tables can name lies inside the gathered vector, every destination row inside the sector
  if (w.j_first < 0 || w.j_count < 0 || w.j_first + w.j_count > a.dd_dst || s.nblk != a.nblk || s.unit_len != a.du_src ||
      s.units != a.dd_src || s.q < 1 || s.chunk != s.q * s.unit_len * s.nblk) {
    set_error("launch_apply_pairs_window: bad argument");
    return 1;
  }
  return pairs_launch(a, w, src, dst, st);
}

}  // namespace edigpu
