// kernels_shard.hip -- vector kernels of the one-reduction recurrence on shards (the host steps: edigpu_shard.hip).
// Per step the ranks reduce THREE sums, T = (<v|w>, sum (w - sg v)^2, <v|v>), sg = alpha of the previous step (0 on the
// first); alpha and beta follow from them by ab_from_sums (lanczos_sums.hpp, see there for the identity).
#include <algorithm>

#include "exchange_index.hpp"
#include "kernels.hpp"
#include "lanczos_sums.hpp"

namespace edigpu {

constexpr int kShNT = 256;

__device__ inline void block_sum3(double s0, double s1, double s2, double* __restrict__ partial, int stride) {
  __shared__ double ws[3][kShNT / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s0 += __shfl_down(s0, off, 64);
    s1 += __shfl_down(s1, off, 64);
    s2 += __shfl_down(s2, off, 64);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    ws[0][w] = s0;
    ws[1][w] = s1;
    ws[2][w] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int i = 0; i < kShNT / 64; i++) {
      t0 += ws[0][i];
      t1 += ws[1][i];
      t2 += ws[2][i];
    }
    partial[blockIdx.x] = t0;
    partial[stride + blockIdx.x] = t1;
    partial[2 * stride + blockIdx.x] = t2;
  }
}

// w += tmp (+ back, the down half received from the column shards when dim_up > 0); partials of the three sums
__global__ void __launch_bounds__(kShNT)
    ks_add_dot3(int64_t n, int64_t dim_up, int64_t q, int64_t pcol, int halo, const double* __restrict__ vin,
                double* __restrict__ vout, const double* __restrict__ tmp, const double* __restrict__ back,
                const double* __restrict__ tprev, double* __restrict__ partial) {
  const double sg = tprev ? tprev[0] : 0.0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * kShNT + threadIdx.x; e < n; e += (int64_t)gridDim.x * kShNT) {
    double w = vout[e] + tmp[e];
    if (back) {
      const int64_t i = e / dim_up, col = e - i * dim_up;
      w += back[xch_back_slot(i, col, q, pcol, halo)];
    }
    vout[e] = w;
    const double v = vin[e], d = w - sg * v;
    s0 += v * w;
    s1 += d * d;
    s2 += v * v;
  }
  block_sum3(s0, s1, s2, partial, kRedBlocks);
}

// The recurrence on vectors that share one layout element by element (kept in the padded panel layout: the padding holds
// zeros in every buffer, so the three sums are those of the shard).  Two buffers that swap roles every step, eight vector
// passes per step:
//   ks_panel_rotate : x <- (x - alpha v) / beta   in place on the buffer that held w (v = the previous Lanczos vector)
//   ks_panel_add_dot: w = rowhalf + colhalf - beta v, written OVER v (no longer needed), and the three sums with x
__global__ void __launch_bounds__(kShNT)
    ks_panel_rotate(int64_t n2, double2* __restrict__ x, const double2* __restrict__ v, const double* __restrict__ t,
                    const double* __restrict__ tprev) {
  double a, b;
  ab_from_sums(t, tprev, a, b);
  const double ib = 1.0 / b;
  for (int64_t e = (int64_t)blockIdx.x * kShNT + threadIdx.x; e < n2; e += (int64_t)gridDim.x * kShNT) {
    const double2 w = x[e], p = v[e];
    x[e] = make_double2((w.x - a * p.x) * ib, (w.y - a * p.y) * ib);
  }
}

// t / tprev: the reduced sums of the two previous steps (null on the first step, where there is no v: dst = the other buffer)
__global__ void __launch_bounds__(kShNT)
    ks_panel_add_dot(int64_t n2, const double2* __restrict__ x, double2* vdst, const double2* __restrict__ t1,
                     const double2* __restrict__ t2, const double* __restrict__ t, const double* __restrict__ tprev,
                     double* __restrict__ partial) {
  double sg = 0.0, b = 0.0;
  if (t) ab_from_sums(t, tprev, sg, b);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * kShNT + threadIdx.x; e < n2; e += (int64_t)gridDim.x * kShNT) {
    const double2 r = t1[e], c = t2[e], v = x[e];
    double2 w = make_double2(r.x + c.x, r.y + c.y);
    if (t) {
      const double2 p = vdst[e];
      w.x -= b * p.x;
      w.y -= b * p.y;
    }
    vdst[e] = w;
    const double dx = w.x - sg * v.x, dy = w.y - sg * v.y;
    s0 += v.x * w.x + v.y * w.y;
    s1 += dx * dx + dy * dy;
    s2 += v.x * v.x + v.y * v.y;
  }
  block_sum3(s0, s1, s2, partial, kRedBlocks);
}

__global__ void __launch_bounds__(1024) ks_sum3(const double* __restrict__ partial, int np, double* __restrict__ out) {
  __shared__ double sh[3][1024];
  double s[3] = {0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < np; i += 1024)
#pragma unroll
    for (int k = 0; k < 3; k++) s[k] += partial[k * kRedBlocks + i];
#pragma unroll
  for (int k = 0; k < 3; k++) sh[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (threadIdx.x < off)
#pragma unroll
      for (int k = 0; k < 3; k++) sh[k][threadIdx.x] += sh[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x < 3) out[threadIdx.x] = sh[threadIdx.x][0];
}

// (v, w) <- ((w - alpha v) / beta, -beta v) from the reduced sums of the previous step; with send != null the new v
// also goes into the all-to-all send buffer [world][q][pcol + 2 halo] (halo columns into every block that holds them)
__global__ void __launch_bounds__(kShNT)
    ks_rotate3(int first, int64_t n, int64_t dim_up, int64_t q, int world, int64_t pcol, int halo, double* __restrict__ vin,
               double* __restrict__ vout, const double* __restrict__ t, const double* __restrict__ tprev,
               double* __restrict__ send) {
  double a = 0.0, b = 1.0;
  if (!first) ab_from_sums(t, tprev, a, b);
  const double ib = 1.0 / b;
  for (int64_t e = (int64_t)blockIdx.x * kShNT + threadIdx.x; e < n; e += (int64_t)gridDim.x * kShNT) {
    double x = vin[e];
    if (!first) {
      const double p = x;
      x = (vout[e] - a * p) * ib;
      vin[e] = x;
      vout[e] = -b * p;
    }
    if (send) {
      const int64_t i = e / dim_up, col = e - i * dim_up;
      int64_t clo, chi;
      xch_blocks_of(col, pcol, halo, world, clo, chi);
      for (int64_t c = clo; c <= chi; c++) send[xch_send_slot(c, i, col, q, pcol, halo)] = x;
    }
  }
}

static inline dim3 sh_grid(int64_t n, int cap) {
  int64_t nb = (n + kShNT - 1) / kShNT;
  if (nb > cap) nb = cap;
  if (nb < 1) nb = 1;
  return dim3((unsigned)nb);
}

// the three sums of a sweep that left its workgroups' partials in work: out[0..3) <- their totals
static int sum3(const double* work, const dim3& gr, double* out, hipStream_t st) {
  hipLaunchKernelGGL(ks_sum3, dim3(1), dim3(1024), 0, st, work, (int)gr.x, out);
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

int shard_rotate3(bool first, int64_t n, int64_t dim_up, int64_t q, int world, int64_t pcol, int halo, double* vin, double* vout,
                  const double* t, const double* tprev, double* send, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(ks_rotate3, sh_grid(n, 256 * 16), dim3(kShNT), 0, st, first ? 1 : 0, n, dim_up, q, world, pcol, halo, vin,
                     vout, t, tprev, send);
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

int shard_add_dot3(int64_t n, int64_t dim_up, int64_t q, int64_t pcol, int halo, const double* vin, double* vout,
                   const double* tmp, const double* back, const double* tprev, double* work, double* sums, hipStream_t st) {
  const dim3 gr = sh_grid(std::max<int64_t>(n, 1), kRedBlocks);
  hipLaunchKernelGGL(ks_add_dot3, gr, dim3(kShNT), 0, st, n, dim_up, q, pcol, halo, vin, vout, tmp, back, tprev, work);
  return sum3(work, gr, sums, st);
}

int shard_panel_rotate(int64_t n2, double* x, const double* v, const double* t, const double* tprev, hipStream_t st) {
  hipLaunchKernelGGL(ks_panel_rotate, sh_grid(n2, 256 * 16), dim3(kShNT), 0, st, n2, reinterpret_cast<double2*>(x),
                     reinterpret_cast<const double2*>(v), t, tprev);
  EDIGPU_HIP(hipGetLastError());
  return 0;
}

int shard_panel_add_dot(int64_t n2, const double* x, double* vdst, const double* rowhalf, const double* colhalf,
                        const double* t, const double* tprev, double* work, double* sums, hipStream_t st) {
  const dim3 gr = sh_grid(std::max<int64_t>(n2, 1), kRedBlocks);
  hipLaunchKernelGGL(ks_panel_add_dot, gr, dim3(kShNT), 0, st, n2, reinterpret_cast<const double2*>(x),
                     reinterpret_cast<double2*>(vdst), reinterpret_cast<const double2*>(rowhalf),
                     reinterpret_cast<const double2*>(colhalf), t, tprev, work);
  return sum3(work, gr, sums, st);
}

}  // namespace edigpu
