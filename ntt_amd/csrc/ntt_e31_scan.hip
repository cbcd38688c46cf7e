// Eng31 (primes < 2^31, 4-B elements): the scan and batch-inverse kernels' instantiations (ntt_batch_inverse, ntt_matrix_scan).
#include "ntt_scan_impl.hpp"
namespace ntt {
NTT_INSTANTIATE_SCAN(Eng31)
}  // namespace ntt
