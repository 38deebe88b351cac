// Host emulation of the window + source form of the seed kernels (csrc/kernels_axisop.hip, kernels_pairs.hip,
// kernels_ops.hip) for the CPU suite: the same index arithmetic through csrc/shard_src.hpp, element by element, on plain
// arrays.  Shared by tests/host_shard_seeds.cpp (ctypes shim) and tests/host_shard_seeds_sanitize_main.cpp.  g++, no HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "shard_src.hpp"

namespace seeds_emul {

using edigpu::ShardSrc;
using edigpu::shard_src_offset;

constexpr uint32_t kNone = 0xFFFFFFFFu, kIdx = 0x7FFFFFFFu;

// this rank's (first, count) of `units` over `world` ranks (edigpu_shard_plan)
inline void plan(int64_t units, int world, int rank, int64_t& first, int64_t& count, int64_t& q) {
  q = (units + world - 1) / world;
  first = (int64_t)rank * q < units ? (int64_t)rank * q : units;
  count = units - first < q ? units - first : q;
  if (count < 0) count = 0;
}

// the all-gather of a whole vector [nblk][units][unit_len] cut over `world` ranks: every rank's shard [nblk][count][unit_len]
// at the start of its chunk of q unit_len nblk elements, the padding filled with `poison` (nobody may read it)
inline std::vector<double> gather(const double* whole, int64_t units, int64_t unit_len, int nblk, int world, double poison,
                                  ShardSrc& s) {
  s.units = units;
  s.unit_len = unit_len;
  s.nblk = nblk;
  s.q = (units + world - 1) / world;
  s.chunk = s.q * unit_len * nblk;
  std::vector<double> g((size_t)(s.chunk * world), poison);
  for (int r = 0; r < world; r++) {
    int64_t first, count, q;
    plan(units, world, r, first, count, q);
    for (int p = 0; p < nblk; p++)
      for (int64_t k = 0; k < count; k++)
        for (int64_t i = 0; i < unit_len; i++)
          g[(size_t)(r * s.chunk + (p * count + k) * unit_len + i)] = whole[(p * units + first + k) * unit_len + i];
  }
  return g;
}

// axisop form (real coefficients): dst[o][j - j_first][i] = sum_t coef_t s_t(j) src[o][part_t(j)][i], the source row through
// shard_src_offset; acc = coef_0 x_0, then acc = coef_t x_t + acc (exact on the integer-valued vectors of the tests)
inline void axis_window(int nterms, const uint32_t* part, const double* coef, int64_t O, int64_t a_dst, int64_t I, int64_t j_first,
                        int64_t j_count, const ShardSrc& s, const double* gathered, double* dst) {
  for (int64_t o = 0; o < O; o++)
    for (int64_t jj = 0; jj < j_count; jj++)
      for (int64_t i = 0; i < I; i++) {
        double acc = 0.0;
        for (int t = 0; t < nterms; t++) {
          const uint32_t p = part[t * a_dst + j_first + jj];
          double x = 0.0;
          if (p != kNone) {
            x = gathered[shard_src_offset(s, o, (int64_t)(p & kIdx)) + i];
            if (p >> 31) x = -x;
          }
          acc = t == 0 ? coef[0] * x : coef[t] * x + acc;
        }
        dst[(o * j_count + jj) * I + i] = acc;
      }
}

// pairs form: dst[p][jdw - j_first][jup] = sum_t coef_t s_t src[p][pd_t(jdw)][pu_t(jup)], the source row through
// shard_src_offset; acc = 0, then acc = coef_t (+-x_t) + acc, terms without a preimage skipped
inline void pairs_window(int nterms, const uint32_t* pu, const uint32_t* pd, uint32_t id_up, uint32_t id_dw, const double* coef,
                         int nblk, int64_t du_dst, int64_t dd_dst, int64_t j_first, int64_t j_count, const ShardSrc& s,
                         const double* gathered, double* dst) {
  for (int p = 0; p < nblk; p++)
    for (int64_t jj = 0; jj < j_count; jj++)
      for (int64_t j = 0; j < du_dst; j++) {
        const int64_t jdw = j_first + jj;
        double acc = 0.0;
        for (int t = 0; t < nterms; t++) {
          const uint32_t d = ((id_dw >> t) & 1u) ? (uint32_t)jdw : pd[t * dd_dst + jdw];
          const uint32_t u = ((id_up >> t) & 1u) ? (uint32_t)j : pu[t * du_dst + j];
          if (d == kNone || u == kNone) continue;
          const double y = gathered[shard_src_offset(s, p, (int64_t)(d & kIdx)) + (int64_t)(u & kIdx)];
          acc = coef[t] * (((u ^ d) >> 31) ? -y : y) + acc;
        }
        dst[(p * j_count + jj) * du_dst + j] = acc;
      }
}

// flat form (apply_op_flat_kernel, complex elements as (re, im) pairs): dst[p][k] (=|+=) (cre + i cim) s src[p][i(k)] for
// the ndst destination states `states` of a rank, i = off_dw[sst >> ns] + rk_up[sst & lomask], the element through
// shard_src_offset with unit_len = 1
inline void flat_window(int64_t ndst, int nblk, int ns, uint32_t bit, int create, const int32_t* states, const int32_t* off_dw,
                        const int32_t* rk_up, const ShardSrc& s, const double* gathered2, double cre, double cim, int accumulate,
                        double* dst2) {
  const uint32_t lomask = (1u << ns) - 1u;
  for (int p = 0; p < nblk; p++)
    for (int64_t k = 0; k < ndst; k++) {
      const uint32_t t = (uint32_t)states[k];
      double xr = 0.0, xi = 0.0;
      if (create ? (t & bit) != 0u : (t & bit) == 0u) {
        const uint32_t sst = t ^ bit;
        const int64_t i = (int64_t)off_dw[sst >> ns] + rk_up[sst & lomask];
        const int64_t e = shard_src_offset(s, p, i);
        xr = gathered2[2 * e];
        xi = gathered2[2 * e + 1];
        if (__builtin_popcount(sst & (bit - 1u)) & 1) {
          xr = -xr;
          xi = -xi;
        }
      }
      double yr = cre * xr - cim * xi, yi = cre * xi + cim * xr;
      const int64_t e = p * ndst + k;
      if (accumulate) {
        yr += dst2[2 * e];
        yi += dst2[2 * e + 1];
      }
      dst2[2 * e] = yr;
      dst2[2 * e + 1] = yi;
    }
}

}  // namespace seeds_emul
