// Eng64G (Goldilocks, 8-B elements): launchers, fill / pack / transpose / pointwise / twiddle-build kernels.
#include "ntt_kernels_impl.hpp"
namespace ntt {
NTT_EXTERN_KIND(Eng64G, KIND_ROWS)  // ntt_eg_rows.hip
NTT_INSTANTIATE(Eng64G)
}  // namespace ntt
