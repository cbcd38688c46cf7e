// Eng64G (Goldilocks, 8-B elements): k_fri_fold instantiations, the FRI fold of bit-reversed coset evaluations (ntt_fri_fold).
#include "ntt_fold_impl.hpp"
namespace ntt {
NTT_INSTANTIATE_FOLD(Eng64G)
}  // namespace ntt
