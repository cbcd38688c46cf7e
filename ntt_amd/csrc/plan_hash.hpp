// Poseidon2 Merkle commitments and openings (ntt_plan_set_poseidon2, ntt_poseidon2_permute, ntt_merkle_commit,
// ntt_merkle_open, ntt_merkle_info): the host side.  ntt_plan_set_poseidon2 checks the caller's parameters and
// packs them with poseidon2.hpp's pack -- round constants in the field's working form, the diagonal as Shoup
// pairs on the 4-byte fields -- into the one buffer the calls own: Layout<T>::MAX_ELEMS elements, allocated at
// the first set, whatever N.  The launching calls check their arguments, then enqueue: a commit is one leaf
// launch, one launch per layer down to 2^tail_log nodes, and one workgroup for the last tail_log layers.
// A Prover (plan_prover.hpp) owns one Hash and hands it a reference to itself: X, whose checks and field
// constants the calls share with the other features, and through it the plan P.  Included by plan_prover.hpp alone.
#pragma once
#include <utility>
#include <vector>

namespace {

template <class E, class Plan>
struct Hash {
  static constexpr int MEMW = E::MEMW;
  static constexpr unsigned T = MerkleShape::width_t(E::MEMW), D = T / 2;
  using V = deep_val_t<E>;
  Prover<E, Plan>& X;
  Plan& P;
  DevBuf d_tab;  // the constant table (poseidon2.hpp Layout<T>)
  bool ready = false;
  unsigned alpha = 0, rounds_f = 0, rounds_p = 0;
  explicit Hash(Prover<E, Plan>& prover) : X(prover), P(prover.P) {}

  HashArgs<E> base_args() const {
    HashArgs<E> A{};
    A.K = X.constants();
    A.dbg = P.Ff.dbg;
    A.rounds_f = rounds_f;
    A.rounds_p = rounds_p;
    return A;
  }

  int set(unsigned width, unsigned sbox_degree, unsigned rf, unsigned rp, const uint64_t* ext_rc, const uint64_t* int_rc,
          const uint64_t* int_diag) {
    if (!X.usable() || width != T || !ext_rc || !int_diag || (rp && !int_rc)) return NTT_ERR_ARG;
    if (!p2::shape_ok(X.modulus(), sbox_degree, rf, rp)) return NTT_ERR_ARG;
    std::vector<V> host(p2::Layout<T>::MAX_ELEMS, V(0));
    if (!p2::pack<T>(host.data(), X.modulus(), rf, rp, ext_rc, int_rc, int_diag, X.constants())) return NTT_ERR_ARG;
    if (!d_tab && !d_tab.alloc(host.size() * sizeof(V))) return NTT_ERR_HIP;
    if (hipMemcpy(d_tab.get(), host.data(), host.size() * sizeof(V), hipMemcpyHostToDevice) != hipSuccess) return NTT_ERR_HIP;
    alpha = sbox_degree, rounds_f = rf, rounds_p = rp;
    ready = true;
    return NTT_OK;
  }

  int permute(void* states, uint64_t count, hipStream_t st) {
    if (!X.usable() || !ready || !states || count == 0 || count > (1ull << 32)) return NTT_ERR_ARG;
    HashArgs<E> A = base_args();
    A.count = count;
    A.st_elems = (size_t)count * T;
    A.vec = aligned16(states);
    P.begin(st);
    const hipError_t e = launch_p2_permute<E>(alpha, static_cast<uint32_t*>(states), d_tab.template get<V>(), A, st);
    P.mark(st, "p");
    return Plan::rc_of(e);
  }

  int commit(const void* mat, unsigned width, unsigned log_rows, void* tree, hipStream_t st) {
    if (!X.usable() || !ready || !mat || !tree || !X.shape_ok(width, log_rows)) return NTT_ERR_ARG;
    const size_t eb = (size_t)MEMW * 4, n = (size_t)1 << log_rows;
    if (overlaps(mat, n * width * eb, tree, (2 * n - 1) * D * eb)) return NTT_ERR_ARG;
    HashArgs<E> A = base_args();
    A.log_rows = log_rows;
    A.width = width;
    A.mat_elems = n * width;
    A.tree_elems = (2 * n - 1) * D;
    A.vec = aligned16(mat) && ((size_t)width * eb) % 16 == 0;
    A.vec_tree = aligned16(tree);
    uint32_t* t = static_cast<uint32_t*>(tree);
    const V* tab = d_tab.template get<V>();
    P.begin(st);
    hipError_t e = launch_merkle_leaf<E>(alpha, static_cast<const uint32_t*>(mat), t, tab, A, st);
    P.mark(st, "h");
    const unsigned tail = MerkleShape::tail_log(log_rows);
    for (unsigned l = 1; e == hipSuccess && l + tail <= log_rows; ++l) {  // layers of more than 2^tail nodes' children
      A.in_node = MerkleShape::layer_start(log_rows, l - 1);
      A.out_node = MerkleShape::layer_start(log_rows, l);
      A.count = n >> l;
      e = launch_merkle_layer<E>(alpha, t, tab, A, st);
      P.mark(st, "m", 1);
    }
    if (e == hipSuccess && tail) {
      A.in_node = MerkleShape::layer_start(log_rows, log_rows - tail);
      A.layers = tail;
      e = launch_merkle_tail<E>(alpha, t, tab, A, st);
      P.mark(st, "m", tail);
    }
    return Plan::rc_of(e);
  }

  int open(const void* mat, unsigned width, unsigned log_rows, const void* tree, const uint32_t* index, unsigned nq,
           void* rows, void* paths, hipStream_t st) {
    if (!X.usable() || !ready || !tree || !index || nq == 0 || !X.shape_ok(width, log_rows)) return NTT_ERR_ARG;
    if ((mat == nullptr) != (rows == nullptr)) return NTT_ERR_ARG;
    if (!paths && log_rows) return NTT_ERR_ARG;  // a tree of one node has no path
    const size_t eb = (size_t)MEMW * 4, n = (size_t)1 << log_rows;
    const size_t mat_b = mat ? n * width * eb : 0, tree_b = (2 * n - 1) * D * eb, idx_b = (size_t)nq * 4;
    const size_t rows_b = rows ? (size_t)nq * width * eb : 0, paths_b = (size_t)nq * log_rows * D * eb;
    for (const auto& o : {std::pair<const void*, size_t>{rows, rows_b}, {paths, paths_b}}) {
      if (!o.first || !o.second) continue;
      if ((mat && overlaps(mat, mat_b, o.first, o.second)) || overlaps(tree, tree_b, o.first, o.second) ||
          overlaps(index, idx_b, o.first, o.second))
        return NTT_ERR_ARG;
    }
    HashArgs<E> A = base_args();
    A.log_rows = log_rows;
    A.width = width;
    A.nq = nq;
    A.mat_elems = n * width;
    A.tree_elems = (2 * n - 1) * D;
    A.idx_elems = nq;
    A.rows_elems = (size_t)nq * width;
    A.paths_elems = (size_t)nq * log_rows * D;
    P.begin(st);
    const hipError_t e = launch_merkle_open<E>(static_cast<const uint32_t*>(mat), static_cast<const uint32_t*>(tree), index,
                                               static_cast<uint32_t*>(rows), static_cast<uint32_t*>(paths), A, st);
    P.mark(st, "g");
    return Plan::rc_of(e);
  }

  // the shape alone: needs no parameters
  int info(unsigned width, unsigned log_rows, unsigned* digest_elems, uint64_t* tree_elems, unsigned* launches,
           unsigned* tail_log) const {
    if (!X.usable() || !digest_elems || !tree_elems || !launches || !tail_log || !X.shape_ok(width, log_rows)) return NTT_ERR_ARG;
    *digest_elems = D;
    *tree_elems = ((2ull << log_rows) - 1) * D;
    *launches = MerkleShape::launches(log_rows);
    *tail_log = MerkleShape::tail_log(log_rows);
    return NTT_OK;
  }
};

}  // namespace
