// Eng64G (Goldilocks, 8-B elements): launchers, fill / pack / transpose / pointwise / twiddle-build kernels.
#include "ntt_elementwise_impl.hpp"
#include "ntt_inplace_impl.hpp"
#include "ntt_kernels_impl.hpp"
#include "ntt_rivals_impl.hpp"
#include "ntt_tables_impl.hpp"
namespace ntt {
NTT_EXTERN_KIND(Eng64G, KIND_ROWS)  // ntt_eg_rows.hip
NTT_INSTANTIATE(Eng64G)  // launch_pass
NTT_INSTANTIATE_INPLACE(Eng64G)
NTT_INSTANTIATE_TABLES(Eng64G)
NTT_INSTANTIATE_RIVALS(Eng64G)
NTT_INSTANTIATE_ELEMENTWISE(Eng64G)
}  // namespace ntt
