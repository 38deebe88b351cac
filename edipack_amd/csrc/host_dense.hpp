// host_dense.hpp -- the small dense symmetric eigensolvers of the Lanczos drivers (host only, no HIP: the CPU tests
// compile host_dense.cpp with g++, tests/host_dense.cpp).
#pragma once
#include <vector>

namespace edigpu {
#pragma GCC visibility push(hidden)

// (arguments and layouts: at the definitions)  tql2 returns 1 when an eigenvalue has not converged after 200 iterations
int tql2(int n, std::vector<double>& d, std::vector<double>& e, std::vector<double>& z);
void jacobi_eigh(int n, std::vector<double>& a, std::vector<double>& w, std::vector<double>& z);

#pragma GCC visibility pop
}  // namespace edigpu
