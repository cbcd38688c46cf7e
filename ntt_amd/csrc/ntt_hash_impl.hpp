// The Poseidon2 Merkle kernels (ntt_poseidon2_permute, ntt_merkle_commit, ntt_merkle_open)
// over a row-major matrix M = [N][width] and a tree of 2N - 1 digests of D = T / 2 elements (T = 16 on Eng31,
// 8 on Eng64G: 32 B a digest, 64 B a state on both).  Included by ntt_eg_hash.hip and ntt_e31_hash.hip alone.
//
// Forms.  M, the states and the digests are in the plan's I/O form; a lane's state is in the field's working
// form (poseidon2.hpp: load_form at every absorbed element, store_form at every digest element, both nothing on
// Montgomery plans and on Goldilocks).  The constant table is a kernel argument of its own, const and
// __restrict__, and every index into it is wave-uniform: the constants arrive in SGPRs by scalar loads.
//
//   k_p2_permute    A lane owns a state: 64 B in, the permutation, 64 B out.
//   k_merkle_leaf   A lane owns a row and keeps its T state registers.  A workgroup's BT rows are one contiguous
//                   byte range; it comes through LDS in tiles of CC columns (128 B of a row: four absorptions),
//                   loaded by 16-byte accesses of consecutive lanes along a row where the matrix allows (A.vec),
//                   by element accesses otherwise, and stored at a pitch of CC + 1 elements, so that the lanes'
//                   reads at stride one row touch distinct banks at every width.  Every element is read once.
//                   Rows past N and the short last tile are masked.
//   k_merkle_layer  A lane owns a parent: its two children are 64 contiguous bytes.
//   k_merkle_tail   One workgroup runs the last layers: the first from the tree, the others from the digests its
//                   lanes left in LDS; every digest also goes to the tree.
//   k_merkle_open   A wave owns a query: the row at index & (N - 1) and the sibling (index >> l) ^ 1 of every layer.
// Checked build: an index outside its buffer sets 0x100 and goes to element 0, a non-canonical matrix or state
// element 0x200, a non-canonical digest or output state 0x800.
#pragma once
#include <type_traits>

#include "ntt_kernels.hpp"
#include "poseidon2.hpp"

namespace ntt {

template <class E>
__device__ __forceinline__ size_t hash_idx(size_t idx, [[maybe_unused]] size_t count, [[maybe_unused]] size_t n,
                                           [[maybe_unused]] const HashArgs<E>& A) {
#if NTT_DEBUG_CHECKS
  if (idx + count > n) {
    ntt_dbg_flag(A.dbg, NTT_DBG_BOUNDS);
    return 0;
  }
#endif
  return idx;
}
template <class E>
__device__ __forceinline__ void hash_check([[maybe_unused]] deep_val_t<E> v, [[maybe_unused]] uint32_t bit,
                                           [[maybe_unused]] const HashArgs<E>& A) {
#if NTT_DEBUG_CHECKS
  if (!xf::canonical(v, A.K)) ntt_dbg_flag(A.dbg, bit);
#endif
}
template <class E>
__device__ __forceinline__ deep_val_t<E> hash_ld1(const uint32_t* __restrict__ base, size_t idx) {
  if constexpr (E::MEMW == 1) {
    return base[idx];
  } else {
    const uint2 v = reinterpret_cast<const uint2*>(base)[idx];
    return ((uint64_t)v.y << 32) | v.x;
  }
}
template <class E>
__device__ __forceinline__ void hash_st1(uint32_t* __restrict__ base, size_t idx, deep_val_t<E> v) {
  if constexpr (E::MEMW == 1)
    base[idx] = v;
  else
    reinterpret_cast<uint2*>(base)[idx] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}
// NE elements (a multiple of 16 bytes) from element index at; vec: 16-byte accesses (at NE-aligned, base 16-byte aligned)
template <class E, int NE>
__device__ __forceinline__ void hash_ld(deep_val_t<E> (&x)[NE], const uint32_t* base, size_t at, bool vec) {
  constexpr int NW = NE * E::MEMW;
  static_assert(NW % 4 == 0, "whole 16-byte words");
  if (vec) {
    uint32_t w[NW];
    const uint4* p4 = reinterpret_cast<const uint4*>(base + at * E::MEMW);
#pragma unroll
    for (int q = 0; q < NW / 4; ++q) {
      const uint4 v = p4[q];
      w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      if constexpr (E::MEMW == 1)
        x[j] = w[j];
      else
        x[j] = ((uint64_t)w[2 * j + 1] << 32) | w[2 * j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < NE; ++j) x[j] = hash_ld1<E>(base, at + j);
  }
}
template <class E, int NE>
__device__ __forceinline__ void hash_st(uint32_t* base, size_t at, const deep_val_t<E> (&x)[NE], bool vec) {
  constexpr int NW = NE * E::MEMW;
  static_assert(NW % 4 == 0, "whole 16-byte words");
  if (vec) {
    uint32_t w[NW];
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      if constexpr (E::MEMW == 1) {
        w[j] = x[j];
      } else {
        w[2 * j] = (uint32_t)x[j];
        w[2 * j + 1] = (uint32_t)(x[j] >> 32);
      }
    }
    uint4* p4 = reinterpret_cast<uint4*>(base + at * E::MEMW);
#pragma unroll
    for (int q = 0; q < NW / 4; ++q) p4[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < NE; ++j) hash_st1<E>(base, at + j, x[j]);
  }
}

// the digest of a permuted state -> node `node` of the tree, in the I/O form
template <class E, int T>
__device__ __forceinline__ void hash_put_digest(uint32_t* tree, size_t node, const deep_val_t<E> (&s)[T], deep_val_t<E> (&dig)[T / 2],
                                                const HashArgs<E>& A) {
#pragma unroll
  for (int j = 0; j < T / 2; ++j) {
    dig[j] = p2::store_form(s[j], A.K);
    hash_check<E>(dig[j], NTT_DBG_OUTPUT, A);
  }
  hash_st<E, T / 2>(tree, hash_idx<E>(node * (T / 2), T / 2, A.tree_elems, A), dig, A.vec_tree != 0);
}

// ------------------------------------------------------------------------------ permute
template <class E, int ALPHA>
__global__ __launch_bounds__(MerkleShape::BT) void k_p2_permute(uint32_t* __restrict__ states,
                                                               const deep_val_t<E>* __restrict__ tab, const HashArgs<E> A) {
  using V = deep_val_t<E>;
  constexpr int T = MerkleShape::width_t(E::MEMW);
  const size_t i = (size_t)blockIdx.x * MerkleShape::BT + threadIdx.x;
  if (i >= A.count) return;
  const size_t at = hash_idx<E>(i * T, T, A.st_elems, A);
  V s[T];
  hash_ld<E, T>(s, states, at, A.vec != 0);
#pragma unroll
  for (int j = 0; j < T; ++j) {
    hash_check<E>(s[j], NTT_DBG_INPUT, A);
    s[j] = p2::load_form(s[j], A.K);
  }
  p2::permute<T, ALPHA>(s, tab, A.rounds_f, A.rounds_p, A.K);
#pragma unroll
  for (int j = 0; j < T; ++j) {
    s[j] = p2::store_form(s[j], A.K);
    hash_check<E>(s[j], NTT_DBG_OUTPUT, A);
  }
  hash_st<E, T>(states, at, s, A.vec != 0);
}

// ------------------------------------------------------------------------------ leaves
template <class E, int ALPHA>
__global__ __launch_bounds__(MerkleShape::BT) void k_merkle_leaf(const uint32_t* __restrict__ mat, uint32_t* __restrict__ tree,
                                                                const deep_val_t<E>* __restrict__ tab, const HashArgs<E> A) {
  using V = deep_val_t<E>;
  constexpr int T = MerkleShape::width_t(E::MEMW), D = T / 2;
  constexpr uint32_t BT = MerkleShape::BT, CC = MerkleShape::chunk_cols(E::MEMW), PITCH = CC + 1;
  constexpr uint32_t VE = 4 / E::MEMW;  // elements of a 16-byte access
  __shared__ V lds[BT * PITCH];
  const uint32_t tid = threadIdx.x, W = A.width;
  const size_t n = (size_t)1 << A.log_rows, row0 = (size_t)blockIdx.x * BT;
  const uint32_t nr = n - row0 < BT ? (uint32_t)(n - row0) : BT;  // the workgroup's rows

  V s[T];
#pragma unroll
  for (int j = 0; j < T; ++j) s[j] = 0;
#pragma unroll 1
  for (uint32_t c0 = 0; c0 < W; c0 += CC) {
    const uint32_t cw = W - c0 < CC ? W - c0 : CC;  // the tile's columns
    if (c0) __syncthreads();                        // the previous tile has been absorbed
    if (A.vec) {  // W and so cw are multiples of VE: a row's piece is cw / VE 16-byte words
      const uint32_t q = cw / VE, total = nr * q;
      for (uint32_t e = tid; e < total; e += BT) {
        const uint32_t r = e / q, c = (e - r * q) * VE;
        const size_t at = hash_idx<E>((row0 + r) * W + c0 + c, VE, A.mat_elems, A);
        const uint4 v = *reinterpret_cast<const uint4*>(mat + at * E::MEMW);
        V* dst = lds + r * PITCH + c;
        if constexpr (E::MEMW == 1) {
          dst[0] = v.x, dst[1] = v.y, dst[2] = v.z, dst[3] = v.w;
        } else {
          dst[0] = ((uint64_t)v.y << 32) | v.x;
          dst[1] = ((uint64_t)v.w << 32) | v.z;
        }
      }
    } else {
      const uint32_t total = nr * cw;
      for (uint32_t e = tid; e < total; e += BT) {
        const uint32_t r = e / cw, c = e - r * cw;
        lds[r * PITCH + c] = hash_ld1<E>(mat, hash_idx<E>((row0 + r) * W + c0 + c, 1, A.mat_elems, A));
      }
    }
    __syncthreads();
    if (tid < nr) {
      const V* src = lds + tid * PITCH;
#pragma unroll 1
      for (uint32_t c = 0; c < cw; c += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
          if (c + j < cw) {  // a short last chunk leaves the other positions as they are
            const V x = src[c + j];
            hash_check<E>(x, NTT_DBG_INPUT, A);
            s[j] = p2::load_form(x, A.K);
          }
        }
        p2::permute<T, ALPHA>(s, tab, A.rounds_f, A.rounds_p, A.K);
      }
    }
  }
  if (tid < nr) {
    V dig[D];
    hash_put_digest<E, T>(tree, row0 + tid, s, dig, A);
  }
}

// ------------------------------------------------------------------------------ layers
// the parent of the two adjacent digests in c (I/O form) -> node `node`; dig: the parent's digest
template <class E, int ALPHA, int T>
__device__ __forceinline__ void hash_parent(uint32_t* tree, size_t node, const deep_val_t<E> (&c)[T], deep_val_t<E> (&dig)[T / 2],
                                            const deep_val_t<E>* __restrict__ tab, const HashArgs<E>& A) {
  deep_val_t<E> s[T];
#pragma unroll
  for (int j = 0; j < T; ++j) s[j] = p2::load_form(c[j], A.K);
  p2::permute<T, ALPHA>(s, tab, A.rounds_f, A.rounds_p, A.K);
  hash_put_digest<E, T>(tree, node, s, dig, A);
}

template <class E, int ALPHA>
__global__ __launch_bounds__(MerkleShape::BT) void k_merkle_layer(uint32_t* __restrict__ tree, const deep_val_t<E>* __restrict__ tab,
                                                                 const HashArgs<E> A) {
  using V = deep_val_t<E>;
  constexpr int T = MerkleShape::width_t(E::MEMW), D = T / 2;
  const size_t i = (size_t)blockIdx.x * MerkleShape::BT + threadIdx.x;
  if (i >= A.count) return;
  V c[T], dig[D];
  hash_ld<E, T>(c, tree, hash_idx<E>((A.in_node + 2 * i) * D, T, A.tree_elems, A), A.vec_tree != 0);
  hash_parent<E, ALPHA, T>(tree, A.out_node + i, c, dig, tab, A);
}

template <class E, int ALPHA>
__global__ __launch_bounds__(MerkleShape::BT) void k_merkle_tail(uint32_t* __restrict__ tree, const deep_val_t<E>* __restrict__ tab,
                                                                const HashArgs<E> A) {
  using V = deep_val_t<E>;
  constexpr int T = MerkleShape::width_t(E::MEMW), D = T / 2;
  __shared__ V lds[MerkleShape::BT * D];
  const uint32_t tid = threadIdx.x;
  uint32_t cnt = (1u << A.layers) >> 1;  // parents of the step: at most BT
  size_t out = A.in_node + ((size_t)1 << A.layers);
  V c[T], dig[D];
#pragma unroll
  for (int j = 0; j < T; ++j) c[j] = 0;
  if (tid < cnt) hash_ld<E, T>(c, tree, hash_idx<E>((A.in_node + 2 * tid) * D, T, A.tree_elems, A), A.vec_tree != 0);
#pragma unroll 1
  for (uint32_t l = 0; l < A.layers; ++l) {
    if (tid < cnt) hash_parent<E, ALPHA, T>(tree, out + tid, c, dig, tab, A);
    if (l + 1 == A.layers) break;
    __syncthreads();  // the step's children have been read
    if (tid < cnt) {
#pragma unroll
      for (int j = 0; j < D; ++j) lds[tid * D + j] = dig[j];
    }
    __syncthreads();
    out += cnt;
    cnt >>= 1;
    if (tid < cnt) {
#pragma unroll
      for (int j = 0; j < T; ++j) c[j] = lds[2 * tid * D + j];
    }
  }
}

// ------------------------------------------------------------------------------ open
template <class E>
__global__ __launch_bounds__(MerkleShape::OPEN_BT) void k_merkle_open(const uint32_t* __restrict__ mat, const uint32_t* __restrict__ tree,
                                                                     const uint32_t* __restrict__ index, uint32_t* __restrict__ rows,
                                                                     uint32_t* __restrict__ paths, const HashArgs<E> A) {
  constexpr uint32_t D = MerkleShape::width_t(E::MEMW) / 2, BT = MerkleShape::OPEN_BT;
  const uint32_t tid = threadIdx.x, q = blockIdx.x, L = A.log_rows, W = A.width;
  const size_t n = (size_t)1 << L;
  const size_t idx = index[hash_idx<E>(q, 1, A.idx_elems, A)] & (n - 1);  // an index >= N wraps: nothing can fault
  if (rows) {
    for (uint32_t c = tid; c < W; c += BT)
      hash_st1<E>(rows, hash_idx<E>((size_t)q * W + c, 1, A.rows_elems, A),
                  hash_ld1<E>(mat, hash_idx<E>(idx * W + c, 1, A.mat_elems, A)));
  }
  for (uint32_t e = tid; e < L * D; e += BT) {
    const uint32_t l = e / D, j = e % D;
    const size_t node = MerkleShape::layer_start(L, l) + ((idx >> l) ^ 1);
    hash_st1<E>(paths, hash_idx<E>(((size_t)q * L + l) * D + j, 1, A.paths_elems, A),
                hash_ld1<E>(tree, hash_idx<E>(node * D + j, 1, A.tree_elems, A)));
  }
}

// ------------------------------------------------------------------------------ launchers
#define NTT_HASH_SWITCH_A(a, CALL) \
  switch (a) {                     \
    case 3: CALL(3); break;        \
    case 5: CALL(5); break;        \
    case 7: CALL(7); break;        \
    default: return hipErrorInvalidValue; \
  }

template <class E>
hipError_t launch_p2_permute(unsigned a, uint32_t* states, const deep_val_t<E>* tab, const HashArgs<E>& A, hipStream_t st) {
  const unsigned grid = (unsigned)((A.count + MerkleShape::BT - 1) / MerkleShape::BT);
#define NTT_HASH_CALL(AA) hipLaunchKernelGGL((k_p2_permute<E, AA>), dim3(grid), dim3(MerkleShape::BT), 0, st, states, tab, A)
  NTT_HASH_SWITCH_A(a, NTT_HASH_CALL)
#undef NTT_HASH_CALL
  return hipGetLastError();
}
template <class E>
hipError_t launch_merkle_leaf(unsigned a, const uint32_t* mat, uint32_t* tree, const deep_val_t<E>* tab, const HashArgs<E>& A,
                              hipStream_t st) {
  const size_t n = (size_t)1 << A.log_rows;
  const unsigned grid = (unsigned)((n + MerkleShape::BT - 1) / MerkleShape::BT);
#define NTT_HASH_CALL(AA) hipLaunchKernelGGL((k_merkle_leaf<E, AA>), dim3(grid), dim3(MerkleShape::BT), 0, st, mat, tree, tab, A)
  NTT_HASH_SWITCH_A(a, NTT_HASH_CALL)
#undef NTT_HASH_CALL
  return hipGetLastError();
}
template <class E>
hipError_t launch_merkle_layer(unsigned a, uint32_t* tree, const deep_val_t<E>* tab, const HashArgs<E>& A, hipStream_t st) {
  const unsigned grid = (unsigned)((A.count + MerkleShape::BT - 1) / MerkleShape::BT);
#define NTT_HASH_CALL(AA) hipLaunchKernelGGL((k_merkle_layer<E, AA>), dim3(grid), dim3(MerkleShape::BT), 0, st, tree, tab, A)
  NTT_HASH_SWITCH_A(a, NTT_HASH_CALL)
#undef NTT_HASH_CALL
  return hipGetLastError();
}
template <class E>
hipError_t launch_merkle_tail(unsigned a, uint32_t* tree, const deep_val_t<E>* tab, const HashArgs<E>& A, hipStream_t st) {
#define NTT_HASH_CALL(AA) hipLaunchKernelGGL((k_merkle_tail<E, AA>), dim3(1), dim3(MerkleShape::BT), 0, st, tree, tab, A)
  NTT_HASH_SWITCH_A(a, NTT_HASH_CALL)
#undef NTT_HASH_CALL
  return hipGetLastError();
}
template <class E>
hipError_t launch_merkle_open(const uint32_t* mat, const uint32_t* tree, const uint32_t* index, uint32_t* rows, uint32_t* paths,
                              const HashArgs<E>& A, hipStream_t st) {
  hipLaunchKernelGGL((k_merkle_open<E>), dim3(A.nq), dim3(MerkleShape::OPEN_BT), 0, st, mat, tree, index, rows, paths, A);
  return hipGetLastError();
}

#define NTT_INSTANTIATE_HASH(E)                                                                                          \
  template hipError_t launch_p2_permute<E>(unsigned, uint32_t*, const deep_val_t<E>*, const HashArgs<E>&, hipStream_t);   \
  template hipError_t launch_merkle_leaf<E>(unsigned, const uint32_t*, uint32_t*, const deep_val_t<E>*, const HashArgs<E>&, \
                                            hipStream_t);                                                                \
  template hipError_t launch_merkle_layer<E>(unsigned, uint32_t*, const deep_val_t<E>*, const HashArgs<E>&, hipStream_t); \
  template hipError_t launch_merkle_tail<E>(unsigned, uint32_t*, const deep_val_t<E>*, const HashArgs<E>&, hipStream_t);  \
  template hipError_t launch_merkle_open<E>(const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*,     \
                                            const HashArgs<E>&, hipStream_t);

}  // namespace ntt
