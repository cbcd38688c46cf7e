// Eng64G (Goldilocks, 8-B elements): the scan and batch-inverse kernels' instantiations (ntt_batch_inverse, ntt_matrix_scan).
#include "ntt_scan_impl.hpp"
namespace ntt {
NTT_INSTANTIATE_SCAN(Eng64G)
}  // namespace ntt
