// Eng31 (primes below 2^31, 4-B elements): launchers, fill / pack / transpose / pointwise / twiddle-build kernels.
#include "ntt_elementwise_impl.hpp"
#include "ntt_inplace_impl.hpp"
#include "ntt_kernels_impl.hpp"
#include "ntt_rivals_impl.hpp"
#include "ntt_tables_impl.hpp"
namespace ntt {
NTT_EXTERN_KIND(Eng31, KIND_ROWS)  // ntt_e31_rows.hip
NTT_INSTANTIATE(Eng31)  // launch_pass
NTT_INSTANTIATE_INPLACE(Eng31)
NTT_INSTANTIATE_TABLES(Eng31)
NTT_INSTANTIATE_RIVALS(Eng31)
NTT_INSTANTIATE_ELEMENTWISE(Eng31)
}  // namespace ntt
