// Eng31 (primes below 2^31, 4-B elements): launchers, fill / pack / transpose / pointwise / twiddle-build kernels.
#include "ntt_kernels_impl.hpp"
namespace ntt {
NTT_EXTERN_KIND(Eng31, KIND_ROWS)  // ntt_e31_rows.hip
NTT_INSTANTIATE(Eng31)
}  // namespace ntt
