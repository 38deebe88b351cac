// kernels_rdm_flat.hip -- impurity reduced density matrix of superc / nonsu2 device vectors (edigpu_imp_rdm_flat): rho_imp
// = Tr_bath |v><v| of imp_rdm_superc (ED_RDM_SUPERC.f90:54-183) and imp_rdm_nonsu2 (ED_RDM_NONSU2.f90:54-188).  Tables and
// the work list: host_rdm_flat.hpp, whose rdm_flat_plan_emulate is this file restated on the host.
//
// The 2^norb rows Idw of one bath word down are consecutive rows of v; a tile (Bup, Bdw) is the run of Bup in each of them
// and lands in the block of ONE class.  A workgroup owns a panel (the slabs of one popcount of Bdw x one chunk of bath
// words up), the slabs [j0, j1) of it, and the packed entries [e0, e1) of some consecutive classes.
//   per slab: of every row the segment that holds the chunk's runs is staged in LDS by coalesced reads (the segments and
//            their places are the same for all slabs of the panel);
//   then thread t owns the entries e0 + t, e0 + t + 256, ...: an entry is (c, p, q) with p <= q, and the thread walks the
//            panel's tiles of class c: acc += s x_p conj(x_q), x_p at (place of the row of p) + (start of the tile's run
//            in that row, from LDS) + (rank of the pattern of p), s = -1 iff popcount(Bup) and popcount(Idw_p) +
//            popcount(Idw_q) are odd.  The accumulators of a thread live in its own LDS slots (no register array);
//   at the end the workgroup writes its e1 - e0 sums to its own place.
// rdm_flat_final_kernel adds the workgroups of a group in workgroup order (16 sub-ranges, then those in order): a fixed
// order, no floating-point atomics, the same bits on every call.
// Sharded vectors (edigpu_imp_rdm_flat_sharded; host_rdm_flat.hpp RdmFlatShardPlan): the same two kernels over two work
// lists -- the interior slabs on the caller's shard in place, the tail slab in a buffer that rdm_flat_seg_kernel fills
// from the shard and the gathered halos -- whose partial sums share one buffer.
#include "kernels.hpp"

namespace edigpu {
namespace {

constexpr int kRdmFlatFinalGroups = 16;
constexpr int kRdmFlatPanelWords = (int)(sizeof(RdmFlatPanel) / sizeof(int32_t));

template <int CW>
__global__ __launch_bounds__(kRdmFlatThreads) void rdm_flat_tiles_kernel(RdmFlatArgs a, const double* __restrict__ v,
                                                                         int64_t vstride, double* __restrict__ partial,
                                                                         int64_t pstride) {
  extern __shared__ double sh[];
  __shared__ int32_t spw[kRdmFlatPanelWords];
  const RdmFlatPanel* sp = reinterpret_cast<const RdmFlatPanel*>(spw);
  double* stage = sh;
  double* acc = sh + (size_t)a.stage_max * CW;
  uint16_t* rel = reinterpret_cast<uint16_t*>(acc + (size_t)a.ept_max * kRdmFlatThreads * CW);
  const RdmFlatWork w = a.work[blockIdx.x];
  const RdmFlatPanel* gp = a.panels + w.panel;
  const int tid = threadIdx.x;
  if (tid < kRdmFlatPanelWords) spw[tid] = reinterpret_cast<const int32_t*>(gp)[tid];
  const int ntile = gp->ntile, rel0 = gp->rel0, bdw0 = gp->bdw0, nbdw = gp->nbdw;
  const int nrel = (a.norb + 1) * ntile, nrow = 1 << a.norb;
  for (int i = tid; i < nrel; i += kRdmFlatThreads) rel[i] = a.rel[rel0 + i];
  for (int e = w.e0 + tid, k = 0; e < w.e1; e += kRdmFlatThreads, k++)
    for (int c = 0; c < CW; c++) acc[(k * kRdmFlatThreads + tid) * CW + c] = 0.0;
  const double* vk = v + (int64_t)blockIdx.y * vstride;
  for (int j = w.j0; j < w.j1; j++) {
    const int b = j / nbdw, jj = j - b * nbdw;
    const int64_t row0 = (int64_t)a.bdw[bdw0 + jj] << a.norb;
    __syncthreads();  // the products of the previous slab are done (first pass: the panel, rel, acc are written)
    for (int idw = 0; idw < nrow; idw++) {
      const int kd = __popc((unsigned)idw), len = sp->len[kd] * CW;
      if (len == 0) continue;
      const double* src = vk + ((int64_t)b * a.dim_el + a.rowstart[row0 + idw] + sp->seg[kd]) * CW;
      double* dst = stage + sp->soff[idw] * CW;
      for (int c = tid; c < len; c += kRdmFlatThreads) dst[c] = src[c];
    }
    __syncthreads();
    for (int e = w.e0 + tid, k = 0; e < w.e1; e += kRdmFlatThreads, k++) {
      const uint32_t d = a.ent[e];
      const int cls = d & 15u;
      const int lo = sp->kb[cls], hi = sp->kb[cls + 1];
      if (lo == hi) continue;
      const int offp = sp->soff[(d >> 4) & 15u] + (int)((d >> 8) & 7u);
      const int offq = sp->soff[(d >> 11) & 15u] + (int)((d >> 15) & 7u);
      const uint16_t* relp = rel + (int)((d >> 19) & 7u) * ntile;
      const uint16_t* relq = rel + (int)((d >> 22) & 7u) * ntile;
      const uint32_t par = (d >> 18) & 1u;
      double* slot = acc + (k * kRdmFlatThreads + tid) * CW;
      if (CW == 1) {
        double s = slot[0];
#pragma unroll 4
        for (int i = lo; i < hi; i++) {
          const uint32_t rp = relp[i], rq = relq[i];
          const double sg = (par & (rp >> 15)) ? -1.0 : 1.0;
          s += sg * (stage[offp + (int)(rp & 0x7fffu)] * stage[offq + (int)(rq & 0x7fffu)]);
        }
        slot[0] = s;
      } else {
        double sr = slot[0], si = slot[1];
#pragma unroll 4
        for (int i = lo; i < hi; i++) {
          const uint32_t rp = relp[i], rq = relq[i];
          const double sg = (par & (rp >> 15)) ? -1.0 : 1.0;
          const int ip = offp + (int)(rp & 0x7fffu), iq = offq + (int)(rq & 0x7fffu);
          const double xr = stage[2 * ip], xi = stage[2 * ip + 1];
          const double yr = stage[2 * iq], yi = stage[2 * iq + 1];
          sr += sg * (xr * yr + xi * yi);
          si += sg * (xi * yr - xr * yi);
        }
        slot[0] = sr;
        slot[1] = si;
      }
    }
  }
  double* out = partial + (int64_t)blockIdx.y * pstride + w.pofs * CW;
  for (int e = w.e0 + tid, k = 0; e < w.e1; e += kRdmFlatThreads, k++)
    for (int c = 0; c < CW; c++) out[(int64_t)(e - w.e0) * CW + c] = acc[(k * kRdmFlatThreads + tid) * CW + c];
}

// out[g.e0 cw + t] = the group's workgroups' partial sums, t < n = (e1 - e0) cw, in a fixed order
__global__ __launch_bounds__(64 * kRdmFlatFinalGroups) void rdm_flat_final_kernel(const double* __restrict__ partial,
                                                                                  int64_t pstride, RdmGroup g, int cw,
                                                                                  double* __restrict__ out, int64_t ostride) {
  __shared__ double part[kRdmFlatFinalGroups][64];
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  const int n = (g.e1 - g.e0) * cw, t = blockIdx.x * 64 + lane;
  const int per = (g.nwg + kRdmFlatFinalGroups - 1) / kRdmFlatFinalGroups;
  const int w0 = sub * per, w1 = min(g.nwg, w0 + per);
  double s = 0.0;
  if (t < n) {
    const double* p = partial + (int64_t)blockIdx.y * pstride + g.pbase * cw + t;
#pragma unroll 8
    for (int w = w0; w < w1; w++) s += p[(int64_t)w * n];
  }
  part[sub][lane] = s;
  __syncthreads();
  if (sub == 0 && t < n) {
    double r = 0.0;
    for (int k = 0; k < kRdmFlatFinalGroups; k++) r += part[k][lane];
    out[(int64_t)blockIdx.y * ostride + (int64_t)g.e0 * cw + t] = r;
  }
}

// dst[vec][blk][s.dst + i] <- element s.src + i of the source segment s names (host_rdm_flat.hpp RdmFlatSeg, whose
// rdm_flat_segs_emulate is this kernel on the host): the shard's block, a rank's gathered halo block, or zeros.  One double
// per thread, consecutive threads on consecutive doubles of the segment on both sides (vectors may be 8-byte aligned
// only, heads have any length and offset); blockIdx.y = block x segment, blockIdx.z = vector: the segment is uniform.
__global__ __launch_bounds__(kRdmFlatThreads) void rdm_flat_seg_kernel(const RdmFlatSeg* __restrict__ segs, int nseg, int nblk,
                                                                       int cw, const double* __restrict__ v, int64_t vstride,
                                                                       int64_t count, const double* __restrict__ halos, int64_t H,
                                                                       int64_t rank_stride, double* __restrict__ dst, int64_t dlen) {
  const int b = blockIdx.y / nseg, k = blockIdx.z;
  const RdmFlatSeg s = segs[blockIdx.y - b * nseg];
  const int64_t i = (int64_t)blockIdx.x * kRdmFlatThreads + threadIdx.x;
  if (i >= s.len * cw) return;
  double x = 0.0;
  if (s.sel == 1) x = v[k * vstride + ((int64_t)b * count + s.src) * cw + i];
  else if (s.sel == 2) x = halos[s.rank * rank_stride + (((int64_t)k * nblk + b) * H + s.src) * cw + i];
  dst[(((int64_t)k * nblk + b) * dlen + s.dst) * cw + i] = x;
}

}  // namespace

size_t rdm_flat_lds_bytes(const RdmFlatArgs& a) {
  const size_t doubles = ((size_t)a.stage_max + (size_t)a.ept_max * kRdmFlatThreads) * a.cw;
  return doubles * sizeof(double) + (((size_t)a.rel_max * sizeof(uint16_t) + 15) & ~(size_t)15);
}

static int launch_flat_tiles(const RdmFlatArgs& a, int nwork, const double* v, int64_t vstride, int nvec, double* partial,
                             int64_t pstride, hipStream_t st) {
  const size_t lds = rdm_flat_lds_bytes(a);
  const dim3 grid((unsigned)nwork, (unsigned)nvec);
  if (a.cw == 2) {
    if (ensure_dynamic_lds((const void*)rdm_flat_tiles_kernel<2>, lds)) return 1;
    rdm_flat_tiles_kernel<2><<<grid, kRdmFlatThreads, lds, st>>>(a, v, vstride, partial, pstride);
  } else {
    if (ensure_dynamic_lds((const void*)rdm_flat_tiles_kernel<1>, lds)) return 1;
    rdm_flat_tiles_kernel<1><<<grid, kRdmFlatThreads, lds, st>>>(a, v, vstride, partial, pstride);
  }
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

static int launch_flat_final(const RdmGroup* groups, int ngroups, int cw, int nvec, const double* partial, int64_t pstride,
                             double* out, int64_t ostride, hipStream_t st) {
  for (int k = 0; k < ngroups; k++) {
    const int n = (groups[k].e1 - groups[k].e0) * cw;
    rdm_flat_final_kernel<<<dim3((unsigned)((n + 63) / 64), (unsigned)nvec), 64 * kRdmFlatFinalGroups, 0, st>>>(
        partial, pstride, groups[k], cw, out, ostride);
    EDIGPU_HIP(hipGetLastError());
  }
  return 0;
}

int launch_imp_rdm_flat(const RdmFlatArgs& a, int nwork, const RdmGroup* groups, int ngroups, const double* v, int64_t vstride,
                        int nvec, double* partial, int64_t pstride, double* out, int64_t ostride, hipStream_t st) {
  EDIGPU_HIP(hipMemsetAsync(out, 0, (size_t)nvec * ostride * sizeof(double), st));  // classes the sector does not hold
  if (nwork <= 0) return 0;
  if (launch_flat_tiles(a, nwork, v, vstride, nvec, partial, pstride, st)) return 1;
  return launch_flat_final(groups, ngroups, a.cw, nvec, partial, pstride, out, ostride, st);
}

int launch_imp_rdm_flat_shard(const RdmFlatArgs& in, int nin, const double* v, int64_t vstride, const RdmFlatArgs& slab, int nslab,
                              const double* vslab, int64_t sstride, const RdmGroup* groups, int ngroups, int nvec, double* partial,
                              int64_t pstride, double* out, int64_t ostride, hipStream_t st) {
  EDIGPU_HIP(hipMemsetAsync(out, 0, (size_t)nvec * ostride * sizeof(double), st));  // classes the elements do not hold
  if (nin > 0 && launch_flat_tiles(in, nin, v, vstride, nvec, partial, pstride, st)) return 1;
  if (nslab > 0 && launch_flat_tiles(slab, nslab, vslab, sstride, nvec, partial, pstride, st)) return 1;
  return launch_flat_final(groups, ngroups, in.cw, nvec, partial, pstride, out, ostride, st);
}

int launch_rdm_flat_segs(const RdmFlatSeg* segs, int nseg, int64_t maxlen, int nblk, int cw, int nvec, const double* v,
                         int64_t vstride, int64_t count, const double* halos, int64_t H, double* dst, int64_t dlen, hipStream_t st) {
  if (nseg <= 0 || maxlen <= 0 || nblk <= 0 || nvec <= 0) return 0;
  const int64_t gx = (maxlen * cw + kRdmFlatThreads - 1) / kRdmFlatThreads;
  if (gx > 0x7fffffff || (int64_t)nseg * nblk > 65535 || nvec > 65535) {
    set_error("rdm_flat_segs: the copy does not fit a grid");
    return 1;
  }
  const dim3 grid((unsigned)gx, (unsigned)(nseg * nblk), (unsigned)nvec);
  rdm_flat_seg_kernel<<<grid, kRdmFlatThreads, 0, st>>>(segs, nseg, nblk, cw, v, vstride, count, halos, H,
                                                        (int64_t)nvec * nblk * H * cw, dst, dlen);
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

}  // namespace edigpu
