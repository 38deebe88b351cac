// kernels_rdm.hip -- impurity reduced density matrix of normal-mode device vectors (edigpu_imp_rdm): rho_imp =
// Tr_bath |v><v| of imp_rdm_normal (ED_RDM_NORMAL.f90:146-209).  Tables and the work list: host_rdm.hpp, whose
// rdm_plan_emulate is this file restated on the host.
//
// The vector [rows][dim_up] is tiled into dense Lu x Ld tiles, one per (bath word up, bath word down); rho is the sum over
// tiles of x x^H and lands in the block (ku, kd).  A workgroup owns the down runs [j0, j1) of ONE down class kd, the
// columns of one chunk, and the packed entries [e0, e1) of that class (all up classes, or one where they do not fit).
//   per down run: the Ld rows x clen columns are staged in LDS by coalesced row reads (each element of v is read once
//            by the one workgroup that owns its (class, chunk));
//   then thread t owns the entries e0 + t, e0 + t + 256, ...: an entry is (ku, p, q) with p <= q, and the thread walks
//            the chunk's up runs of class ku (their starts are in LDS), acc += x_p conj(x_q), two LDS reads per product.
//            The accumulators of a thread live in its own LDS slots (no register array, nothing dynamically indexed);
//   at the end the workgroup writes its e1 - e0 sums to its own place.
// rdm_final_kernel adds the workgroups of a group in workgroup order (16 sub-ranges, then those in order): a fixed
// order, no floating-point atomics, the same bits on every call.
//
// Sharded vectors (edigpu_imp_rdm_sharded; host_rdm.hpp RdmShardPlan): the same two kernels over two work lists -- the
// runs inside the rank's rows on the shard in place, the run a rank boundary cuts on a slab -- whose partial sums share
// one buffer; rdm_rows_kernel copies the few rows of the halo a rank sends and of the slab.
#include "kernels.hpp"

namespace edigpu {
namespace {

constexpr int kRdmFinalGroups = 16;

template <int CW>
__global__ __launch_bounds__(kRdmThreads) void rdm_tiles_kernel(RdmArgs a, const double* __restrict__ v, int64_t vstride,
                                                                double* __restrict__ partial, int64_t pstride) {
  extern __shared__ double sh[];
  __shared__ int skb[kRdmMaxOrb + 2];
  double* stage = sh;
  double* acc = sh + (size_t)a.ld_max * a.stride * CW;
  uint16_t* rel = reinterpret_cast<uint16_t*>(acc + (size_t)a.ept_max * kRdmThreads * CW);
  const RdmWork w = a.work[blockIdx.x];
  const int tid = threadIdx.x;
  if (tid < kRdmMaxOrb + 2) skb[tid] = a.work[blockIdx.x].kb[tid];
  const int nrel = w.kb[kRdmMaxOrb + 1];
  for (int i = tid; i < nrel; i += kRdmThreads) rel[i] = a.rel[w.rel0 + i];
  for (int e = w.e0 + tid, k = 0; e < w.e1; e += kRdmThreads, k++)
    for (int c = 0; c < CW; c++) acc[(k * kRdmThreads + tid) * CW + c] = 0.0;
  const uint32_t d0 = w.e0 + tid < w.e1 ? a.ent[w.e0 + tid] : 0u;
  const double* vk = v + (int64_t)blockIdx.y * vstride;
  const int rowlen = w.clen * CW, srow = a.stride * CW;
  const int64_t grow = a.dim_up * CW;
  for (int j = w.j0; j < w.j1; j++) {
    const int b = j / w.nruns, jj = j - b * w.nruns;
    const int64_t row0 = a.rows[w.row_list + jj] + (int64_t)b * a.dim_dw;
    const double* src = vk + (row0 * a.dim_up + w.c0) * CW;
    __syncthreads();  // the products of the previous run are done (first pass: rel, skb, acc are written)
    for (int c = tid; c < rowlen; c += kRdmThreads) {
      double t[kRdmMaxRun];
#pragma unroll
      for (int rd = 0; rd < kRdmMaxRun; rd++)
        if (rd < w.ld) t[rd] = src[rd * grow + c];
#pragma unroll
      for (int rd = 0; rd < kRdmMaxRun; rd++)
        if (rd < w.ld) stage[rd * srow + c] = t[rd];
    }
    __syncthreads();
    for (int e = w.e0 + tid, k = 0; e < w.e1; e += kRdmThreads, k++) {
      const uint32_t d = k == 0 ? d0 : a.ent[e];
      const int ku = d & 15u;
      const int offp = (int)((d >> 8) & 15u) * a.stride + (int)((d >> 4) & 15u);
      const int offq = (int)((d >> 16) & 15u) * a.stride + (int)((d >> 12) & 15u);
      const int lo = skb[ku], hi = skb[ku + 1];
      double* slot = acc + (k * kRdmThreads + tid) * CW;
      if (CW == 1) {
        double s = slot[0];
#pragma unroll 4
        for (int i = lo; i < hi; i++) {
          const int u = rel[i];
          s += stage[offp + u] * stage[offq + u];
        }
        slot[0] = s;
      } else {
        double sr = slot[0], si = slot[1];
#pragma unroll 4
        for (int i = lo; i < hi; i++) {
          const int u = rel[i];
          const double xr = stage[2 * (offp + u)], xi = stage[2 * (offp + u) + 1];
          const double yr = stage[2 * (offq + u)], yi = stage[2 * (offq + u) + 1];
          sr += xr * yr + xi * yi;
          si += xi * yr - xr * yi;
        }
        slot[0] = sr;
        slot[1] = si;
      }
    }
  }
  double* out = partial + (int64_t)blockIdx.y * pstride + w.pofs * CW;
  for (int e = w.e0 + tid, k = 0; e < w.e1; e += kRdmThreads, k++)
    for (int c = 0; c < CW; c++) out[(int64_t)(e - w.e0) * CW + c] = acc[(k * kRdmThreads + tid) * CW + c];
}

// out[g.e0 cw + t] = the group's workgroups' partial sums, t < n = (e1 - e0) cw, in a fixed order
__global__ __launch_bounds__(64 * kRdmFinalGroups) void rdm_final_kernel(const double* __restrict__ partial, int64_t pstride,
                                                                         RdmGroup g, int cw, double* __restrict__ out,
                                                                         int64_t ostride) {
  __shared__ double part[kRdmFinalGroups][64];
  const int lane = threadIdx.x & 63, sub = threadIdx.x >> 6;
  const int n = (g.e1 - g.e0) * cw, t = blockIdx.x * 64 + lane;
  const int per = (g.nwg + kRdmFinalGroups - 1) / kRdmFinalGroups;
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
    for (int k = 0; k < kRdmFinalGroups; k++) r += part[k][lane];
    out[(int64_t)blockIdx.y * ostride + (int64_t)g.e0 * cw + t] = r;
  }
}

// dst[vec][blk][row][0:rowlen) <- the source t names for `row` (host_rdm.hpp RdmRowCopy, whose rdm_rows_emulate is this
// kernel on the host): a row of the shard's block, a row of a rank's gathered halo, or zeros.  One double per thread,
// consecutive threads on consecutive doubles of the row on both sides (the vectors may be 8-byte aligned only).
__global__ __launch_bounds__(kRdmThreads) void rdm_rows_kernel(RdmRowCopy t, int nblk, int rowlen, const double* __restrict__ v,
                                                               int64_t vstride, int64_t count, const double* __restrict__ halos,
                                                               int H, int64_t rank_stride, double* __restrict__ dst) {
  const int c = blockIdx.x * kRdmThreads + threadIdx.x;
  if (c >= rowlen) return;
  const int b = blockIdx.y / t.nrows, r = blockIdx.y - b * t.nrows, k = blockIdx.z;
  const int sel = t.sel[r];
  const int64_t row = t.row[r];
  double x = 0.0;
  if (sel == 1) x = v[k * vstride + ((int64_t)b * count + row) * rowlen + c];
  else if (sel == 2) x = halos[t.rank[r] * rank_stride + (((int64_t)k * nblk + b) * H + row) * rowlen + c];
  dst[(((int64_t)k * nblk + b) * t.nrows + r) * rowlen + c] = x;
}

}  // namespace

size_t rdm_lds_bytes(const RdmArgs& a) {
  const size_t doubles = ((size_t)a.ld_max * a.stride + (size_t)a.ept_max * kRdmThreads) * a.cw;
  return doubles * sizeof(double) + (((size_t)a.rel_max * sizeof(uint16_t) + 15) & ~(size_t)15);
}

static int launch_rdm_tiles(const RdmArgs& a, int nwork, const double* v, int64_t vstride, int nvec, double* partial,
                            int64_t pstride, hipStream_t st) {
  const size_t lds = rdm_lds_bytes(a);
  const dim3 grid((unsigned)nwork, (unsigned)nvec);
  if (a.cw == 2) {
    if (ensure_dynamic_lds((const void*)rdm_tiles_kernel<2>, lds)) return 1;
    rdm_tiles_kernel<2><<<grid, kRdmThreads, lds, st>>>(a, v, vstride, partial, pstride);
  } else {
    if (ensure_dynamic_lds((const void*)rdm_tiles_kernel<1>, lds)) return 1;
    rdm_tiles_kernel<1><<<grid, kRdmThreads, lds, st>>>(a, v, vstride, partial, pstride);
  }
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

static int launch_rdm_final(const RdmGroup* groups, int ngroups, int cw, int nvec, const double* partial, int64_t pstride,
                            double* out, int64_t ostride, hipStream_t st) {
  for (int k = 0; k < ngroups; k++) {
    const int n = (groups[k].e1 - groups[k].e0) * cw;
    rdm_final_kernel<<<dim3((unsigned)((n + 63) / 64), (unsigned)nvec), 64 * kRdmFinalGroups, 0, st>>>(partial, pstride, groups[k],
                                                                                                     cw, out, ostride);
    EDIGPU_HIP(hipGetLastError());
  }
  return 0;
}

int launch_imp_rdm(const RdmArgs& a, int nwork, const RdmGroup* groups, int ngroups, const double* v, int64_t vstride,
                   int nvec, double* partial, int64_t pstride, double* out, int64_t ostride, hipStream_t st) {
  EDIGPU_HIP(hipMemsetAsync(out, 0, (size_t)nvec * ostride * sizeof(double), st));  // classes the sector does not hold
  if (nwork <= 0) return 0;
  if (launch_rdm_tiles(a, nwork, v, vstride, nvec, partial, pstride, st)) return 1;
  return launch_rdm_final(groups, ngroups, a.cw, nvec, partial, pstride, out, ostride, st);
}

int launch_imp_rdm_shard(const RdmArgs& in, int nin, const double* v, int64_t vstride, const RdmArgs& slab, int nslab,
                         const double* vslab, int64_t sstride, const RdmGroup* groups, int ngroups, int nvec, double* partial,
                         int64_t pstride, double* out, int64_t ostride, hipStream_t st) {
  EDIGPU_HIP(hipMemsetAsync(out, 0, (size_t)nvec * ostride * sizeof(double), st));  // classes the rows do not hold
  if (nin > 0 && launch_rdm_tiles(in, nin, v, vstride, nvec, partial, pstride, st)) return 1;
  if (nslab > 0 && launch_rdm_tiles(slab, nslab, vslab, sstride, nvec, partial, pstride, st)) return 1;
  return launch_rdm_final(groups, ngroups, in.cw, nvec, partial, pstride, out, ostride, st);
}

int launch_rdm_rows(const RdmRowCopy& t, int nblk, int rowlen, int nvec, const double* v, int64_t vstride, int64_t count,
                    const double* halos, int H, double* dst, hipStream_t st) {
  if (t.nrows <= 0 || nblk <= 0 || rowlen <= 0 || nvec <= 0) return 0;
  const dim3 grid((unsigned)((rowlen + kRdmThreads - 1) / kRdmThreads), (unsigned)(t.nrows * nblk), (unsigned)nvec);
  rdm_rows_kernel<<<grid, kRdmThreads, 0, st>>>(t, nblk, rowlen, v, vstride, count, halos, H, (int64_t)nvec * nblk * H * rowlen, dst);
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

}  // namespace edigpu
