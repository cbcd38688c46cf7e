// Eng64G (Goldilocks, 8-B elements): k_pass instantiations for KIND_SINGLE.
#include "ntt_kernels_impl.hpp"
namespace ntt {
NTT_INSTANTIATE_KIND(Eng64G, KIND_SINGLE)
}  // namespace ntt
