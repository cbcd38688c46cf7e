// Eng256w: k_pass instantiations of the low-degree-extension first passes (PRO_LDE: KIND_COLUMN, KIND_SINGLE).
#include "ntt_lde_impl.hpp"
namespace ntt {
NTT_INSTANTIATE_LDE(Eng256w)
}  // namespace ntt
