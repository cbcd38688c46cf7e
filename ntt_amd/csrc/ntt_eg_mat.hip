// Eng64G (Goldilocks, 8-B elements): k_pass_mat instantiations, the row-major matrix passes (strip form: KIND_COLUMN, its PRO_LDE form, KIND_FINAL) and k_mat_naive.
#include "ntt_mat_impl.hpp"
namespace ntt {
NTT_INSTANTIATE_MAT(Eng64G)
}  // namespace ntt
