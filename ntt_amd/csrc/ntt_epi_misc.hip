// EngPI (P with 8-B scratch, NTT_PLAN_IN_PLACE): launchers, fill / pack / transpose / pointwise / twiddle-build kernels.
#include "ntt_elementwise_impl.hpp"
#include "ntt_inplace_impl.hpp"
#include "ntt_kernels_impl.hpp"
#include "ntt_rivals_impl.hpp"
#include "ntt_tables_impl.hpp"
namespace ntt {
NTT_INSTANTIATE(EngPI)  // launch_pass
NTT_INSTANTIATE_INPLACE(EngPI)
NTT_INSTANTIATE_TABLES(EngPI)
NTT_INSTANTIATE_RIVALS(EngPI)
NTT_INSTANTIATE_ELEMENTWISE(EngPI)
}  // namespace ntt
