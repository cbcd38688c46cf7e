// Eng384: launchers, fill / pack / transpose / pointwise / twiddle-build kernels.
#include "ntt_elementwise_impl.hpp"
#include "ntt_inplace_impl.hpp"
#include "ntt_kernels_impl.hpp"
#include "ntt_rivals_impl.hpp"
#include "ntt_tables_impl.hpp"
namespace ntt {
NTT_INSTANTIATE(Eng384)  // launch_pass
NTT_INSTANTIATE_INPLACE(Eng384)
NTT_INSTANTIATE_TABLES(Eng384)
NTT_INSTANTIATE_RIVALS(Eng384)
NTT_INSTANTIATE_ELEMENTWISE(Eng384)
}  // namespace ntt
