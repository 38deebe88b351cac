// extern "C" wrapper of csrc/shard_src.hpp and of the host emulation of the window + source kernels
// (tests/host_shard_seeds.hpp) for tests/test_shard_src_host.py (g++, no HIP).
#include "host_shard_seeds.hpp"

using namespace seeds_emul;

static ShardSrc make(int64_t q, int64_t units, int64_t chunk, int64_t unit_len, int nblk) {
  ShardSrc s;
  s.q = q;
  s.units = units;
  s.chunk = chunk;
  s.unit_len = unit_len;
  s.nblk = nblk;
  return s;
}

extern "C" {

int64_t ss_offset(int64_t q, int64_t units, int64_t chunk, int64_t unit_len, int nblk, int64_t p, int64_t g) {
  return shard_src_offset(make(q, units, chunk, unit_len, nblk), p, g);
}

// geo = q, units, chunk, unit_len, nblk
void ss_axis_window(int nterms, const uint32_t* part, const double* coef, int64_t O, int64_t a_dst, int64_t I, int64_t j_first,
                    int64_t j_count, const int64_t* geo, const double* gathered, double* dst) {
  axis_window(nterms, part, coef, O, a_dst, I, j_first, j_count, make(geo[0], geo[1], geo[2], geo[3], (int)geo[4]), gathered, dst);
}

void ss_pairs_window(int nterms, const uint32_t* pu, const uint32_t* pd, uint32_t id_up, uint32_t id_dw, const double* coef, int nblk,
                     int64_t du_dst, int64_t dd_dst, int64_t j_first, int64_t j_count, const int64_t* geo, const double* gathered,
                     double* dst) {
  pairs_window(nterms, pu, pd, id_up, id_dw, coef, nblk, du_dst, dd_dst, j_first, j_count,
               make(geo[0], geo[1], geo[2], geo[3], (int)geo[4]), gathered, dst);
}

void ss_flat_window(int64_t ndst, int nblk, int ns, uint32_t bit, int create, const int32_t* states, const int32_t* off_dw,
                    const int32_t* rk_up, const int64_t* geo, const double* gathered2, double cre, double cim, int accumulate,
                    double* dst2) {
  flat_window(ndst, nblk, ns, bit, create, states, off_dw, rk_up, make(geo[0], geo[1], geo[2], geo[3], (int)geo[4]), gathered2, cre,
              cim, accumulate, dst2);
}

}  // extern "C"
