// Eng31 (primes < 2^31, 4-B elements): the Poseidon2 Merkle kernels' instantiations (ntt_poseidon2_permute, ntt_merkle_commit, ntt_merkle_open).
#include "ntt_hash_impl.hpp"
namespace ntt {
NTT_INSTANTIATE_HASH(Eng31)
}  // namespace ntt
