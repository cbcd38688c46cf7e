// Eng256wI (NTT_PLAN_IN_PLACE plans of the 48-B layout): launchers and element-wise kernels.
#include "ntt_elementwise_impl.hpp"
#include "ntt_inplace_impl.hpp"
#include "ntt_kernels_impl.hpp"
#include "ntt_rivals_impl.hpp"
#include "ntt_tables_impl.hpp"
namespace ntt {
NTT_INSTANTIATE(Eng256wI)  // launch_pass
NTT_INSTANTIATE_INPLACE(Eng256wI)
NTT_INSTANTIATE_TABLES(Eng256wI)
NTT_INSTANTIATE_RIVALS(Eng256wI)
NTT_INSTANTIATE_ELEMENTWISE(Eng256wI)
}  // namespace ntt
