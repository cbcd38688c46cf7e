// EngP: launchers, fill / pack / transpose / pointwise / twiddle-build kernels.
#include "ntt_elementwise_impl.hpp"
#include "ntt_inplace_impl.hpp"
#include "ntt_kernels_impl.hpp"
#include "ntt_rivals_impl.hpp"
#include "ntt_tables_impl.hpp"
namespace ntt {
NTT_EXTERN_KIND(EngP, KIND_ROWS)  // ntt_ep_rows.hip
NTT_INSTANTIATE(EngP)  // launch_pass
NTT_INSTANTIATE_INPLACE(EngP)
NTT_INSTANTIATE_TABLES(EngP)
NTT_INSTANTIATE_RIVALS(EngP)
NTT_INSTANTIATE_ELEMENTWISE(EngP)
}  // namespace ntt
