// Eng256T (4096-element tiles: single 2^20 transforms of 4-limb plans, BASELINE config 2): launchers
// and element-wise kernels.
#include "ntt_elementwise_impl.hpp"
#include "ntt_inplace_impl.hpp"
#include "ntt_kernels_impl.hpp"
#include "ntt_rivals_impl.hpp"
#include "ntt_tables_impl.hpp"
namespace ntt {
NTT_INSTANTIATE(Eng256T)  // launch_pass
NTT_INSTANTIATE_INPLACE(Eng256T)
NTT_INSTANTIATE_TABLES(Eng256T)
NTT_INSTANTIATE_RIVALS(Eng256T)
NTT_INSTANTIATE_ELEMENTWISE(Eng256T)
}  // namespace ntt
