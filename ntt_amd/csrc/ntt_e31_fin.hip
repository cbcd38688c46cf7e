// Eng31 (primes below 2^31, 4-B elements): k_pass instantiations for KIND_FINAL.
#include "ntt_kernels_impl.hpp"
namespace ntt {
NTT_INSTANTIATE_KIND(Eng31, KIND_FINAL)
}  // namespace ntt
