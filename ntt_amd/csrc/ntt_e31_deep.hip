// Eng31 (primes < 2^31, 4-B elements): the DEEP kernels' instantiations (ntt_deep_points, ntt_matrix_open, ntt_deep_quotient).
#include "ntt_deep_impl.hpp"
namespace ntt {
NTT_INSTANTIATE_DEEP(Eng31)
}  // namespace ntt
