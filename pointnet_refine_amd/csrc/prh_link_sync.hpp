// Piece linking, steps 5-6 on the GPU: edges, clusters and the arc synchronisation, plus the cum of
// the inputs.  The rule is in include/pointnet_refine_hip.h ("Piece linking - the rule"); the device
// algorithm is restated in plain Python ints in tests/_link_sync_oracle.py.
//   link_cum_kernel          one thread per piece: cum[0] = 0, cum[k+1] = cum[k] + sqrt(|e|^2)
//   link_edges_kernel        one thread per candidate: its owner i, edge / rho / delta (step 5) and
//                            the number of edges of every block (ballot / popcount)
//   link_compact_kernel      the edges in candidate order behind the scanned block counts: no sort,
//                            no atomic
//   link_hook_kernel         components, first half of a round: per edge atomicMin of either end's
//                            label into the other's; raises a flag when an atomic lowered a label
//   link_jump_kernel         second half: every piece's label chased to a label that is its own
//   link_tree_init_kernel    level 0, sign +1, offset 0 at the roots (label[p] == p)
//   link_propose_kernel      a tree level, first half: per directed edge a -> b with a at level n
//                            and b not placed, a 64-bit atomicMax of (n_in << 32) | (2^32 - 1 - a)
//   link_place_kernel        second half: the directed edge whose key won writes b's row
// Why the result is bitwise reproducible although the atomics arrive in any order:
//   Components.  Every value ever stored in label[p] is a member of p's component that is <= p, and a
//   label is only ever lowered.  The host stops after a round whose hook kernel lowered nothing.  In
//   such a kernel no word of label changed (an atomicMin that lowers nothing stores the value it
//   found), so every plain load of label in it - whichever cache served it - read the one value that
//   word had for the whole kernel, the value the previous launch left.  Hence label[i] == label[j]
//   over every edge (otherwise an atomic would have lowered one of them), so label is constant on a
//   component; after the jump kernel every label is its own label; and the component's smallest
//   member m has label[m] <= m, a member, so label[m] == m and the constant is m.  The fixed point is
//   unique: every piece holds its component's smallest member, however the rounds got there.  In the
//   other rounds a plain load may return an older, larger label: still a member of the component, so
//   the worst it does is lower something by less than it could, and the flag asks for another round.
//   The jump kernel's loads race with its own stores in the same way: either value of a word that is
//   not its own label is smaller than its index, so the chase descends and ends at a word that is
//   its own label, which the kernel never writes.
//   Tree.  key[b] is only proposed to while b is unplaced, by the neighbours at the current level,
//   and the maximum of a set does not depend on the order it is taken in: largest n_in, then the
//   smallest a.  A pair (a, b) occurs once in the candidate list, so exactly one directed edge
//   matches key[b] and b's row has one writer; it reads a's row, which an earlier launch wrote.
//   sign * delta is exact, so every offset is one rounded addition, as on the host.
// Everything is fp64 with FMA contraction off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prh_link.hpp"

namespace prh {

constexpr int SYNC_THREADS = 256;

// cum [n_pieces*M]: fuse.carrier_cum of every piece
__global__ __launch_bounds__(SYNC_THREADS) void link_cum_kernel(const double* __restrict__ world, int n_pieces, int M,
                                                                double* __restrict__ cum) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * SYNC_THREADS + threadIdx.x;
  if (p >= n_pieces) return;
  const double* v = world + (long long)p * M * 3;
  double* c = cum + (long long)p * M;
  double ax = v[0], ay = v[1], az = v[2], run = 0.0;
  c[0] = 0.0;
  for (int k = 1; k < M; ++k) {
    const double bx = v[3 * k], by = v[3 * k + 1], bz = v[3 * k + 2];
    const double ex = bx - ax, ey = by - ay, ez = bz - az;
    run = run + sqrt((ex * ex + ey * ey) + ez * ez);
    c[k] = run;
    ax = bx; ay = by; az = bz;
  }
}

// Step 5.  pair_count [n_pairs,2], pair_sum [n_pairs,4] as link_stats_kernel leaves them.  Out: pair_i
// (the owner by pair_offsets), edge (0 / 1), rho (+1 / -1), delta, and block_count [gridDim.x] the
// number of edges among the block's SYNC_THREADS candidates.
__global__ __launch_bounds__(SYNC_THREADS) void link_edges_kernel(
    const long long* __restrict__ pair_offsets, int n_pieces, const int* __restrict__ pair_count,
    const double* __restrict__ pair_sum, long long n_pairs, long long min_in, long long out_ratio,
    int* __restrict__ pair_i, unsigned char* __restrict__ edge, signed char* __restrict__ rho, double* __restrict__ delta,
    long long* __restrict__ block_count) {
#pragma clang fp contract(off)
  __shared__ int sh_n[SYNC_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long c = (long long)blockIdx.x * SYNC_THREADS + threadIdx.x;
  bool is_edge = false;
  if (c < n_pairs) {
    const long long n_in = pair_count[2 * c], n_out = pair_count[2 * c + 1];
    const double sum_self = pair_sum[4 * c + 1], sum_other = pair_sum[4 * c + 2], sum_dot = pair_sum[4 * c + 3];
    is_edge = n_in >= min_in && out_ratio * n_out <= n_in;           // counts of -1 (a bad pair_j) are no edge
    const bool plus = sum_dot >= 0.0;                                // -0.0: +1, NaN: -1, as numpy compares
    const double other = plus ? sum_other : -sum_other;              // rho * sum_other, exact
    pair_i[c] = fuse_owner(pair_offsets, n_pieces, c);
    edge[c] = is_edge ? 1 : 0;
    rho[c] = plus ? 1 : -1;
    delta[c] = n_in > 0 ? (sum_self - other) / (double)n_in : 0.0;
  }
  const unsigned long long mask = __ballot(is_edge);
  if (lane == 0) sh_n[wave] = __popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int w = 0; w < SYNC_THREADS / 64; ++w) n += sh_n[w];
    block_count[blockIdx.x] = n;
  }
}

// block_offsets: the exclusive scan of link_edges_kernel's block_count.  Edge e of the compacted list
// is the e-th candidate with edge != 0: edge_ij [n_edges,2] = i j, edge_w [n_edges,2] = n_in rho,
// edge_delta [n_edges].
__global__ __launch_bounds__(SYNC_THREADS) void link_compact_kernel(
    const int* __restrict__ pair_i, const int* __restrict__ pair_j, const int* __restrict__ pair_count,
    const unsigned char* __restrict__ edge, const signed char* __restrict__ rho, const double* __restrict__ delta,
    long long n_pairs, const long long* __restrict__ block_offsets, long long n_edges, int* __restrict__ edge_ij,
    int* __restrict__ edge_w, double* __restrict__ edge_delta) {
  __shared__ int sh_n[SYNC_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long c = (long long)blockIdx.x * SYNC_THREADS + threadIdx.x;
  const bool is_edge = c < n_pairs && edge[c] != 0;
  const unsigned long long mask = __ballot(is_edge);
  if (lane == 0) sh_n[wave] = __popcll(mask);
  __syncthreads();
  if (!is_edge) return;
  long long slot = block_offsets[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) slot += sh_n[w];
  if (slot >= n_edges) return;                         // never past the caller's buffers
  edge_ij[2 * slot] = pair_i[c];
  edge_ij[2 * slot + 1] = pair_j[c];
  edge_w[2 * slot] = pair_count[2 * c];
  edge_w[2 * slot + 1] = rho[c];
  edge_delta[slot] = delta[c];
}

// Components, first half of a round.  The plain loads only decide whether an atomic is worth
// sending: a stale (larger) label[j] can at worst skip a lowering that the flag then asks again for,
// because whoever made it stale lowered something.
__global__ __launch_bounds__(SYNC_THREADS) void link_hook_kernel(const int* __restrict__ edge_ij, long long n_edges,
                                                                 int n_pieces, int* label, int* changed) {
  const long long e = (long long)blockIdx.x * SYNC_THREADS + threadIdx.x;
  if (e >= n_edges) return;
  const int i = edge_ij[2 * e], j = edge_ij[2 * e + 1];
  if ((unsigned)i >= (unsigned)n_pieces || (unsigned)j >= (unsigned)n_pieces) return;
  const int li = label[i], lj = label[j];
  if (lj < li) {
    if (atomicMin(&label[i], lj) > lj) atomicOr(changed, 1);
  } else if (li < lj) {
    if (atomicMin(&label[j], li) > li) atomicOr(changed, 1);
  }
}

// Second half: label[p] chased until it is its own label.  The words that are their own label are
// never written here, so the chase ends at one of them whatever the other threads have stored yet.
__global__ __launch_bounds__(SYNC_THREADS) void link_jump_kernel(int n_pieces, int* label) {
  const int p = blockIdx.x * SYNC_THREADS + threadIdx.x;
  if (p >= n_pieces) return;
  int l = label[p];
  if (l == p || (unsigned)l >= (unsigned)n_pieces) return;             // a label that names no piece is left alone
  for (int n = label[l]; n != l && (unsigned)n < (unsigned)n_pieces; n = label[l]) l = n;
  label[p] = l;
}

__global__ __launch_bounds__(SYNC_THREADS) void link_tree_init_kernel(const int* __restrict__ label, int n_pieces,
                                                                      int* __restrict__ level, int* __restrict__ parent,
                                                                      int* __restrict__ sign, double* __restrict__ offset,
                                                                      unsigned long long* __restrict__ key) {
  const int p = blockIdx.x * SYNC_THREADS + threadIdx.x;
  if (p >= n_pieces) return;
  level[p] = label[p] == p ? 0 : -1;
  parent[p] = -1;
  sign[p] = 1;
  offset[p] = 0.0;
  key[p] = 0ull;
}

__device__ __forceinline__ unsigned long long link_parent_key(int n_in, int a) {
  return ((unsigned long long)(unsigned)n_in << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)a);
}

// A tree level, first half: level is read only (the place kernel of the previous level wrote it).
__global__ __launch_bounds__(SYNC_THREADS) void link_propose_kernel(const int* __restrict__ edge_ij,
                                                                    const int* __restrict__ edge_w, long long n_edges,
                                                                    int n_pieces, int n, const int* __restrict__ level,
                                                                    unsigned long long* key) {
  const long long e = (long long)blockIdx.x * SYNC_THREADS + threadIdx.x;
  if (e >= n_edges) return;
  const int i = edge_ij[2 * e], j = edge_ij[2 * e + 1];
  if ((unsigned)i >= (unsigned)n_pieces || (unsigned)j >= (unsigned)n_pieces) return;
  const int li = level[i], lj = level[j], n_in = edge_w[2 * e];
  if (li == n && lj < 0) atomicMax(&key[j], link_parent_key(n_in, i));
  else if (lj == n && li < 0) atomicMax(&key[i], link_parent_key(n_in, j));
}

// Second half.  key[b] == the key of a -> b with a at level n means that a proposed at this level
// (a piece placed earlier holds the key of a parent at a lower level), so b was unplaced then and
// this thread is its only writer.
__global__ __launch_bounds__(SYNC_THREADS) void link_place_kernel(
    const int* __restrict__ edge_ij, const int* __restrict__ edge_w, const double* __restrict__ edge_delta,
    long long n_edges, int n_pieces, int n, const unsigned long long* __restrict__ key, int* level, int* parent,
    int* sign, double* offset, int* placed) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * SYNC_THREADS + threadIdx.x;
  if (e >= n_edges) return;
  const int i = edge_ij[2 * e], j = edge_ij[2 * e + 1];
  if ((unsigned)i >= (unsigned)n_pieces || (unsigned)j >= (unsigned)n_pieces) return;
  const int li = level[i], lj = level[j], n_in = edge_w[2 * e], rho = edge_w[2 * e + 1];
  int a, b;
  if (li == n && lj != n && key[j] == link_parent_key(n_in, i)) { a = i; b = j; }
  else if (lj == n && li != n && key[i] == link_parent_key(n_in, j)) { a = j; b = i; }
  else return;
  const int sa = sign[a], sb = rho * sa;
  const double d = edge_delta[e], oa = offset[a];
  level[b] = n + 1;
  parent[b] = a;
  sign[b] = sb;
  offset[b] = a == i ? oa + (double)sa * d : oa - (double)sb * d;
  atomicOr(placed, 1);
}

}  // namespace prh
