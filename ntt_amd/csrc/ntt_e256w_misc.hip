// Eng256w: launchers, fill / pack / transpose / pointwise / twiddle-build kernels.
#include "ntt_elementwise_impl.hpp"
#include "ntt_inplace_impl.hpp"
#include "ntt_kernels_impl.hpp"
#include "ntt_rivals_impl.hpp"
#include "ntt_tables_impl.hpp"
namespace ntt {
NTT_EXTERN_KIND(Eng256w, KIND_ROWS)  // ntt_e256w_rows.hip
NTT_INSTANTIATE(Eng256w)  // launch_pass
NTT_INSTANTIATE_INPLACE(Eng256w)
NTT_INSTANTIATE_TABLES(Eng256w)
NTT_INSTANTIATE_RIVALS(Eng256w)
NTT_INSTANTIATE_ELEMENTWISE(Eng256w)
}  // namespace ntt
