// Eng256: launchers, fill / pack / transpose / pointwise / twiddle-build kernels.
#include "ntt_elementwise_impl.hpp"
#include "ntt_inplace_impl.hpp"
#include "ntt_kernels_impl.hpp"
#include "ntt_rivals_impl.hpp"
#include "ntt_tables_impl.hpp"
namespace ntt {
NTT_EXTERN_KIND(Eng256, KIND_ROWS)  // ntt_e256_rows.hip
NTT_INSTANTIATE(Eng256)  // launch_pass
NTT_INSTANTIATE_INPLACE(Eng256)
NTT_INSTANTIATE_TABLES(Eng256)
NTT_INSTANTIATE_RIVALS(Eng256)
NTT_INSTANTIATE_ELEMENTWISE(Eng256)
}  // namespace ntt
