// kernels_occ.hip -- operators diagonal in the occupation basis on device vectors (edigpu_apply_occ,
// edigpu_occ_moments): the seeds of the density / spin susceptibilities (apply_op_N, apply_op_Sz, ED_SECTOR.f90:1141-1430)
// and the moments sum_i |v_i|^2 n_x(i) n_y(i) behind dens, docc, magz, sz2, n2 (ED_OBSERVABLES_NORMAL.f90:120-185).
//
// Both read the occupation patterns of host_occ.hpp and stream the vector once.
//   apply:   one pass, the weight of an element is wu[up pattern] + wd[down pattern] from two 32-entry tables in LDS.
//   moments, normal mode: a 64-thread workgroup (one wave) owns an equal share of the vector, taken in the order of
//            occ_sort_rows, so a share is at most 2^norb runs of rows with ONE down pattern each.  Inside a run a lane adds
//            |v|^2 into its own LDS bin of the element's up pattern (2^norb bins per lane, no contention, one LDS add per
//            element); at the end of a run the bins are summed over the lanes, every sum slot (lane t = slot t) takes the
//            patterns that hold its up bits, and keeps the result if the run's down pattern holds its down bits.  Lanes
//            walk a run as one index space, so rows shorter than a wave fill the wave with several rows, and rows longer
//            than a share are split between workgroups.
//   moments, flat: grid-stride loop, the upper triangle in registers per thread (templated on norb), butterfly per wave.
//   Every wave writes its 64 slots to its own place; occ_moments_final sums them in wave order: no floating-point
//   atomics reach the result and two calls give the same bits.
#include "kernels.hpp"

namespace edigpu {
namespace {

constexpr int kOccBlock = 256;
constexpr int kOccUnroll = 8;        // loads a lane of the rows kernel keeps in flight: 16 waves x 8 x 512 B = 64 KB per CU
constexpr int kOccFinalGroups = 16;  // occ_moments_final_kernel: groups of 64 threads, each sums a contiguous range of waves

__device__ inline double occ_weight(const OccTables& t, const double* sw, uint32_t e) {
  if (t.flat) {
    const uint32_t i = t.nblk > 1 ? e % (uint32_t)t.dim_up : e;
    const uint32_t p = t.pu[i];
    return sw[p & ((1u << t.norb) - 1u)] + sw[32 + (p >> t.norb)];
  }
  const uint32_t du = (uint32_t)t.dim_up;
  const uint32_t row = e / du, iup = e - row * du;
  const uint32_t idw = t.nblk > 1 ? row % (uint32_t)t.dim_dw : row;
  return sw[t.pu[iup]] + sw[32 + t.pd[idw]];
}

// CW doubles per element (2: interleaved complex); V2: both vectors 16-byte aligned, 16 bytes per lane and access
template <int CW, bool V2>
__global__ __launch_bounds__(kOccBlock) void apply_occ_kernel(OccTables t, OccWeights w, uint32_t nel, const double* __restrict__ src,
                                                              double* dst) {
  __shared__ double sw[64];
  if (threadIdx.x < 32) sw[threadIdx.x] = w.wu[threadIdx.x];
  else if (threadIdx.x < 64) sw[threadIdx.x] = w.wd[threadIdx.x - 32];
  __syncthreads();
  const uint32_t nth = gridDim.x * kOccBlock, tid = blockIdx.x * kOccBlock + threadIdx.x;
  if (CW == 2) {
    for (uint32_t e = tid; e < nel; e += nth) {
      const double f = occ_weight(t, sw, e);
      if (V2) {
        double2 x = reinterpret_cast<const double2*>(src)[e];
        x.x *= f;
        x.y *= f;
        reinterpret_cast<double2*>(dst)[e] = x;
      } else {
        const double re = src[2 * (size_t)e], im = src[2 * (size_t)e + 1];
        dst[2 * (size_t)e] = re * f;
        dst[2 * (size_t)e + 1] = im * f;
      }
    }
  } else if (V2) {
    const uint32_t npair = nel / 2;
    for (uint32_t u = tid; u < npair; u += nth) {
      const double f0 = occ_weight(t, sw, 2 * u), f1 = occ_weight(t, sw, 2 * u + 1);
      double2 x = reinterpret_cast<const double2*>(src)[u];
      x.x *= f0;
      x.y *= f1;
      reinterpret_cast<double2*>(dst)[u] = x;
    }
    if ((nel & 1u) && tid == 0) dst[nel - 1] = src[nel - 1] * occ_weight(t, sw, nel - 1);
  } else {
    for (uint32_t e = tid; e < nel; e += nth) dst[e] = src[e] * occ_weight(t, sw, e);
  }
}

template <int CW, bool V2>
__device__ inline double occ_prob(const double* __restrict__ v, int64_t i) {
  if (CW == 1) {
    const double x = v[i];
    return x * x;
  }
  if (V2) {
    const double2 x = reinterpret_cast<const double2*>(v)[i];
    return x.x * x.x + x.y * x.y;
  }
  const double re = v[2 * i], im = v[2 * i + 1];
  return re * re + im * im;
}

// normal mode (see the head of the file); dynamic LDS: bins[2^norb][64], psum[2^norb]
template <int CW, bool V2>
__global__ __launch_bounds__(64) void occ_moments_rows_kernel(OccTables t, OccSlots sl, OccRuns rn, const double* __restrict__ v,
                                                              int64_t vstride, int nwaves, double* __restrict__ partial) {
  extern __shared__ double sh[];
  const int lane = threadIdx.x, w = blockIdx.x, npat = 1 << t.norb;
  double* bins = sh;
  double* psum = sh + npat * 64;
  for (int p = 0; p < npat; p++) bins[p * 64 + lane] = 0.0;
  const uint32_t du = (uint32_t)t.dim_up;
  const int64_t total = t.dim_dw * t.nblk * (int64_t)du;  // < 2^31
  const int64_t lo = total * w / nwaves, hi = total * (w + 1) / nwaves;
  const double* vk = v + (int64_t)blockIdx.y * vstride;
  const uint32_t q64 = 64u / du, r64 = 64u % du;
  const uint32_t need_up = sl.need_up[lane], need_dw = sl.need_dw[lane];
  double acc = 0.0;
  __syncthreads();
  for (int pd = 0; pd < npat; pd++) {
    const int64_t r0 = (int64_t)rn.run[pd] * du, r1 = (int64_t)rn.run[pd + 1] * du;
    const int64_t a = lo > r0 ? lo : r0, b = hi < r1 ? hi : r1;
    if (a >= b) continue;  // uniform
    // lane's position in the run's index space: sorted row sr, column iup; a step of 64 positions is (q64, r64)
    uint32_t sr = (uint32_t)((a + lane) / du), iup = (uint32_t)((a + lane) - (int64_t)sr * du);
    int64_t base = a;
    for (; base + 64 * kOccUnroll <= b; base += 64 * kOccUnroll) {
      double p[kOccUnroll];
      uint32_t pat[kOccUnroll];
#pragma unroll
      for (int u = 0; u < kOccUnroll; u++) {
        p[u] = occ_prob<CW, V2>(vk, (int64_t)t.order[sr] * du + iup);
        pat[u] = t.pu[iup];
        sr += q64;
        iup += r64;
        if (iup >= du) {
          iup -= du;
          sr++;
        }
      }
#pragma unroll
      for (int u = 0; u < kOccUnroll; u++) atomicAdd(&bins[pat[u] * 64 + lane], p[u]);  // the lane's own bin: never contended
    }
    for (int64_t j = base + lane; j < b; j += 64) {
      atomicAdd(&bins[t.pu[iup] * 64 + lane], occ_prob<CW, V2>(vk, (int64_t)t.order[sr] * du + iup));
      sr += q64;
      iup += r64;
      if (iup >= du) {
        iup -= du;
        sr++;
      }
    }
    __syncthreads();
    // the run's sum per up pattern (lane = pattern; rotated start: no bank conflict, still a fixed order), bins back to 0
    if (lane < npat) {
      double s = 0.0;
      for (int j = 0; j < 64; j++) {
        const int jj = (j + lane) & 63;
        s += bins[lane * 64 + jj];
        bins[lane * 64 + jj] = 0.0;
      }
      psum[lane] = s;
    }
    __syncthreads();
    if (((uint32_t)pd & need_dw) == need_dw) {
      double s = 0.0;
      for (int q = 0; q < npat; q++)
        if (((uint32_t)q & need_up) == need_up) s += psum[q];
      acc += s;
    }
    __syncthreads();
  }
  partial[((int64_t)blockIdx.y * nwaves + w) * 64 + lane] = lane < sl.nslots ? acc : 0.0;
}

// superc / nonsu2: rows of one pattern each, the triangle in registers
template <int NORB, int CW, bool V2>
__global__ __launch_bounds__(kOccBlock) void occ_moments_flat_kernel(OccTables t, const double* __restrict__ v, int64_t vstride,
                                                                     int nwaves, double* __restrict__ partial) {
  constexpr int N2 = 2 * NORB, NT = 1 + N2 * (N2 + 1) / 2;
  double acc[NT];
#pragma unroll
  for (int k = 0; k < NT; k++) acc[k] = 0.0;
  const uint32_t n = (uint32_t)(t.dim_up * t.nblk), del = (uint32_t)t.dim_up;
  const uint32_t nth = gridDim.x * kOccBlock;
  const double* vk = v + (int64_t)blockIdx.y * vstride;
#pragma unroll 2
  for (uint32_t i = blockIdx.x * kOccBlock + threadIdx.x; i < n; i += nth) {
    const uint32_t pat = t.pu[t.nblk > 1 ? i % del : i];
    const double p = occ_prob<CW, V2>(vk, i);
    double bit[N2];
#pragma unroll
    for (int x = 0; x < N2; x++) bit[x] = (pat >> x) & 1u ? 1.0 : 0.0;
    acc[0] += p;
    int k = 1;
#pragma unroll
    for (int x = 0; x < N2; x++) {
      const double px = p * bit[x];
#pragma unroll
      for (int y = x; y < N2; y++, k++) acc[k] = __builtin_fma(px, bit[y], acc[k]);  // exact products: bits are 0 or 1
    }
  }
#pragma unroll
  for (int k = 0; k < NT; k++)
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
  if ((threadIdx.x & 63) == 0) {
    double* out = partial + ((int64_t)blockIdx.y * nwaves + blockIdx.x * (kOccBlock / 64) + threadIdx.x / 64) * 64;
#pragma unroll
    for (int k = 0; k < NT; k++) out[k] = acc[k];
    for (int k = NT; k < 64; k++) out[k] = 0.0;
  }
}

// sums[k][t] = the waves' partials in a fixed order: group g adds the waves [g, g + 1) * ceil(nwaves / groups) in wave
// order (the loads of an unrolled batch are independent, the additions are not reordered), then the groups in group order
__global__ __launch_bounds__(64 * kOccFinalGroups) void occ_moments_final_kernel(const double* __restrict__ partial, int nwaves,
                                                                                 double* __restrict__ sums) {
  __shared__ double part[kOccFinalGroups][64];
  const int t = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int per = (nwaves + kOccFinalGroups - 1) / kOccFinalGroups;
  const int w0 = g * per, w1 = min(nwaves, w0 + per);
  const double* p = partial + (int64_t)blockIdx.x * nwaves * 64 + t;
  double s = 0.0;
#pragma unroll 16
  for (int w = w0; w < w1; w++) s += p[(int64_t)w * 64];
  part[g][t] = s;
  __syncthreads();
  if (g == 0) {
    double r = 0.0;
    for (int k = 0; k < kOccFinalGroups; k++) r += part[k][t];
    sums[blockIdx.x * 64 + t] = r;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int NORB>
int launch_flat_norb(const OccTables& t, const double* v, int nvec, int nwaves, int64_t vstride, bool v2, double* partial,
                     hipStream_t st) {
  const dim3 grid((unsigned)(nwaves / (kOccBlock / 64)), (unsigned)nvec);
  if (!t.cplx) occ_moments_flat_kernel<NORB, 1, false><<<grid, kOccBlock, 0, st>>>(t, v, vstride, nwaves, partial);
  else if (v2) occ_moments_flat_kernel<NORB, 2, true><<<grid, kOccBlock, 0, st>>>(t, v, vstride, nwaves, partial);
  else occ_moments_flat_kernel<NORB, 2, false><<<grid, kOccBlock, 0, st>>>(t, v, vstride, nwaves, partial);
  return 0;
}

}  // namespace

int launch_apply_occ(const OccTables& t, const OccWeights& w, const double* src, double* dst, hipStream_t st) {
  const int64_t nel = t.dim_up * t.dim_dw * t.nblk;
  if (nel <= 0) return 0;
  const bool v2 = aligned16(src) && aligned16(dst);
  const int64_t units = (t.cplx || !v2) ? nel : (nel + 1) / 2;
  const unsigned grid = (unsigned)std::min<int64_t>((units + kOccBlock - 1) / kOccBlock, 4096);
  if (t.cplx) {
    if (v2) apply_occ_kernel<2, true><<<grid, kOccBlock, 0, st>>>(t, w, (uint32_t)nel, src, dst);
    else apply_occ_kernel<2, false><<<grid, kOccBlock, 0, st>>>(t, w, (uint32_t)nel, src, dst);
  } else {
    if (v2) apply_occ_kernel<1, true><<<grid, kOccBlock, 0, st>>>(t, w, (uint32_t)nel, src, dst);
    else apply_occ_kernel<1, false><<<grid, kOccBlock, 0, st>>>(t, w, (uint32_t)nel, src, dst);
  }
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

int occ_moment_waves(const OccTables& t, int ncu) {
  const int64_t nel = t.dim_up * t.dim_dw * t.nblk;
  const int cap = std::max(ncu, 1) * 16;  // waves the device holds at once with the rows kernel's registers and LDS
  if (t.flat) {  // whole workgroups of kOccBlock threads, about 8 elements per thread before the grid grows
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((nel + 8 * kOccBlock - 1) / (8 * kOccBlock), cap / (kOccBlock / 64)));
    return (int)blocks * (kOccBlock / 64);
  }
  return (int)std::max<int64_t>(1, std::min<int64_t>((nel + 2047) / 2048, cap));
}

int launch_occ_moments(const OccTables& t, const OccSlots& sl, const OccRuns& rn, const double* v, int nvec, int nwaves,
                       double* partial, double* sums, hipStream_t st) {
  const int64_t nel = t.dim_up * t.dim_dw * t.nblk;
  const int64_t vstride = nel * (t.cplx ? 2 : 1);
  const bool v2 = t.cplx && aligned16(v);
  if (t.flat) {
    switch (t.norb) {
      case 1: launch_flat_norb<1>(t, v, nvec, nwaves, vstride, v2, partial, st); break;
      case 2: launch_flat_norb<2>(t, v, nvec, nwaves, vstride, v2, partial, st); break;
      case 3: launch_flat_norb<3>(t, v, nvec, nwaves, vstride, v2, partial, st); break;
      case 4: launch_flat_norb<4>(t, v, nvec, nwaves, vstride, v2, partial, st); break;
      default: launch_flat_norb<5>(t, v, nvec, nwaves, vstride, v2, partial, st); break;
    }
  } else {
    const dim3 grid((unsigned)nwaves, (unsigned)nvec);
    const size_t lds = ((size_t)(1 << t.norb) * 65) * sizeof(double);
    if (!t.cplx) occ_moments_rows_kernel<1, false><<<grid, 64, lds, st>>>(t, sl, rn, v, vstride, nwaves, partial);
    else if (v2) occ_moments_rows_kernel<2, true><<<grid, 64, lds, st>>>(t, sl, rn, v, vstride, nwaves, partial);
    else occ_moments_rows_kernel<2, false><<<grid, 64, lds, st>>>(t, sl, rn, v, vstride, nwaves, partial);
  }
  EDIGPU_HIP(hipGetLastError());
  occ_moments_final_kernel<<<(unsigned)nvec, 64 * kOccFinalGroups, 0, st>>>(partial, nwaves, sums);
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

}  // namespace edigpu
