// Neighbour ties in the reference's order (include/spr.h): the kd-tree replay of a support set, the in-place fix-up
// of a neighbour matrix, and their host twins.  The arithmetic and every decision live in tie_order.h; this file only
// places the work: one wave per cloud for the build (lane 0 walks: the partition's swap sequence is sequential by
// definition), one lane per row for the fix-up, each lane with its own walk stack and pair scratch in the workspace.
#include <vector>

#include "spr_common.h"
#include "tie_order.h"

namespace spr {
namespace {

using tie::Frame;
using tie::Node;

constexpr int kHdrWords = 64;            // [0] deepest tree, [1] build error, [2] ns, [3] nb
constexpr size_t kLaneBudget = 64u << 20;   // bytes of per-lane scratch the fix-up asks for at most (beyond 256 lanes)

struct TreeView {
  int* hdr;
  float* box;    // [nb, 6]
  int* vind;     // [ns]
  Node* nodes;   // [2 ns]: cloud b owns [2 s_cu[b], 2 s_cu[b + 1])
};

TreeView tree_layout(Workspace& w, int ns, int nb) {
  TreeView t;
  t.hdr = w.take<int>(kHdrWords);
  t.box = w.take<float>(6 * (size_t)(nb > 0 ? nb : 0) + 1);
  t.vind = w.take<int>((size_t)(ns > 0 ? ns : 0) + 1);
  t.nodes = w.take<Node>(2 * (size_t)(ns > 0 ? ns : 0) + 1);
  return t;
}

struct FixView {
  Frame* frames;   // [lanes, depth]
  int* idx;        // [lanes, cap]
  float* d2;       // [lanes, cap]
};

int fix_lanes(int nq, int cap, int depth) {
  const size_t per = (size_t)depth * sizeof(Frame) + (size_t)cap * 8;
  size_t lanes = kLaneBudget / per / 256 * 256;
  if (lanes < 256) lanes = 256;
  if (lanes > 65536) lanes = 65536;
  const size_t rows = align_up((size_t)(nq > 0 ? nq : 1), 256);
  return (int)(lanes < rows ? lanes : rows);
}

FixView fix_layout(Workspace& w, int nq, int cap, int depth) {
  const size_t lanes = (size_t)fix_lanes(nq, cap, depth);
  FixView v;
  v.frames = w.take<Frame>(lanes * depth);
  v.idx = w.take<int>(lanes * cap);
  v.d2 = w.take<float>(lanes * cap);
  return v;
}

__global__ __launch_bounds__(64) void k_tie_build(const float* __restrict__ s_xyz, const int* __restrict__ s_cu, int ns,
                                                  int nb, TreeView t) {
  if (threadIdx.x != 0) return;
  const int b = blockIdx.x;
  if (b == 0) t.hdr[2] = ns, t.hdr[3] = nb;
  const int off = s_cu[b], end = s_cu[b + 1];
  if (off < 0 || end < off || end > ns) {
    atomicOr(t.hdr + 1, 1);
    return;
  }
  int depth = 0;
  const int rc = tie::build_cloud(s_xyz + 3 * (size_t)off, end - off, t.vind + off, t.nodes + 2 * (size_t)off,
                                  2 * (end - off), t.box + 6 * (size_t)b, &depth);
  if (rc) atomicOr(t.hdr + 1, 1);
  atomicMax(t.hdr, depth);
}

__global__ __launch_bounds__(256) void k_tie_fix(const float* __restrict__ q_xyz, const int* __restrict__ q_cu, int nq,
                                                 const float* __restrict__ s_xyz, const int* __restrict__ s_cu, int ns,
                                                 int nb, float r2, TreeView t, int depth_cap, int* __restrict__ nbr,
                                                 int stride, int width, int max_count, int cap, int lanes, FixView v,
                                                 int* __restrict__ status) {
  // one decision for the whole grid, before any row is touched
  if (t.hdr[1] != 0 || t.hdr[0] > depth_cap || t.hdr[2] != ns || t.hdr[3] != nb) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status + 3, 1);
    return;
  }
  const int lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= lanes) return;
  Frame* stack = v.frames + (size_t)lane * depth_cap;
  int* s_idx = v.idx + (size_t)lane * cap;
  float* s_d2 = v.d2 + (size_t)lane * cap;
  int fixed = 0, mismatch = 0, overflow = 0;
  for (int i = lane; i < nq; i += lanes) {
    const int b = find_segment(q_cu, nb, i);
    const int off = s_cu[b], end = s_cu[b + 1];
    if (off < 0 || end < off || end > ns) {
      ++mismatch;
      continue;
    }
    tie::CloudTree ct;
    ct.p = s_xyz + 3 * (size_t)off, ct.n = end - off, ct.offset = off;
    ct.vind = t.vind + off, ct.nodes = t.nodes + 2 * (size_t)off, ct.n_nodes = 2 * (end - off);
    ct.rootbox = t.box + 6 * (size_t)b;
    const float* q = q_xyz + 3 * (size_t)i;
    const int rc = tie::fix_row(ct, q[0], q[1], q[2], r2, ns, nbr + (size_t)i * stride, width, max_count, stack,
                                depth_cap, s_idx, s_d2, cap);
    fixed += rc == tie::kRowFixed;
    mismatch += rc == tie::kRowMismatch;
    overflow += rc == tie::kRowOverflow;
  }
  if (fixed) atomicAdd(status + 0, fixed);
  if (mismatch) atomicAdd(status + 1, mismatch);
  if (overflow) atomicAdd(status + 2, overflow);
}

int check_fix_args(const char* what, int nq, int ns, int nb, float radius, int stride, int width, int max_count) {
  SPR_REQUIRE(nq >= 0 && ns >= 0 && nb >= 1, "%s: nq %d, ns %d, nb %d", what, nq, ns, nb);
  SPR_REQUIRE(radius > 0.f, "%s: radius must be positive", what);
  SPR_REQUIRE(width >= 0 && width <= stride, "%s: width %d does not fit rows of %d columns", what, width, stride);
  SPR_REQUIRE(max_count >= 0, "%s: negative max_count %d", what, max_count);
  return 0;
}

}  // namespace
}  // namespace spr

using namespace spr;

extern "C" size_t spr_kdtree_replay_size(int ns, int nb) { return measure(tree_layout, ns, nb); }

extern "C" int spr_kdtree_replay_build(const float* s_xyz, const int* s_cu, int ns, int nb, void* tree,
                                       size_t tree_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  SPR_REQUIRE(ns >= 0 && nb >= 1, "kdtree_replay_build: ns %d, nb %d", ns, nb);
  SPR_REQUIRE(s_cu && tree && (s_xyz || ns == 0), "kdtree_replay_build: null pointer");
  Workspace w(tree, tree_bytes);
  const TreeView t = tree_layout(w, ns, nb);
  SPR_REQUIRE(w.ok(), "kdtree_replay_build: the tree needs %zu bytes, got %zu", spr_kdtree_replay_size(ns, nb),
              tree_bytes);
  SPR_HIP_CHECK(hipMemsetAsync(t.hdr, 0, kHdrWords * sizeof(int), stream));
  hipLaunchKernelGGL(k_tie_build, dim3(nb), dim3(64), 0, stream, s_xyz, s_cu, ns, nb, t);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t spr_tie_order_workspace_size(int nq, int max_count, int depth) {
  return measure(fix_layout, nq, max_count > 0 ? max_count : 1, depth > 0 ? depth : 1);
}

extern "C" int spr_tie_order(const float* q_xyz, const int* q_cu, int nq, const float* s_xyz, const int* s_cu, int ns,
                             int nb, float radius, const void* tree, int depth, int* nbr, int stride, int width,
                             int max_count, int* status, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = check_fix_args("tie_order", nq, ns, nb, radius, stride, width, max_count)) return rc;
  SPR_REQUIRE(status && tree && q_cu && s_cu, "tie_order: null pointer");
  SPR_REQUIRE(depth >= 0, "tie_order: negative depth %d", depth);
  const bool empty = nq == 0 || width == 0 || ns == 0;
  SPR_REQUIRE(empty || (q_xyz && s_xyz && nbr), "tie_order: null pointer");
  const int cap = max_count > 0 ? max_count : 1, depth_cap = depth > 0 ? depth : 1;
  Workspace tw(const_cast<void*>(tree), spr_kdtree_replay_size(ns, nb));
  const TreeView t = tree_layout(tw, ns, nb);
  Workspace w(ws, ws_bytes);
  const FixView v = fix_layout(w, nq, cap, depth_cap);
  SPR_REQUIRE(w.ok(), "tie_order: the workspace needs %zu bytes, got %zu",
              spr_tie_order_workspace_size(nq, max_count, depth), ws_bytes);
  SPR_HIP_CHECK(hipMemsetAsync(status, 0, 4 * sizeof(int), stream));
  if (empty) return 0;
  const int lanes = fix_lanes(nq, cap, depth_cap);
  hipLaunchKernelGGL(k_tie_fix, dim3(cdiv(lanes, 256)), dim3(256), 0, stream, q_xyz, q_cu, nq, s_xyz, s_cu, ns, nb,
                     radius * radius, t, depth_cap, nbr, stride, width, max_count, cap, lanes, v, status);
  SPR_LAUNCH_CHECK();
  return 0;
}

extern "C" int spr_tie_order_host(const float* q_xyz, const int* q_cu, int nq, const float* s_xyz, const int* s_cu,
                                  int ns, int nb, float radius, int* nbr, int stride, int width, int max_count,
                                  int* status) {
  if (int rc = check_fix_args("tie_order_host", nq, ns, nb, radius, stride, width, max_count)) return rc;
  SPR_REQUIRE(status && q_cu && s_cu, "tie_order_host: null pointer");
  status[0] = status[1] = status[2] = status[3] = 0;
  if (nq == 0 || width == 0 || ns == 0) return 0;
  SPR_REQUIRE(q_xyz && s_xyz && nbr, "tie_order_host: null pointer");
  SPR_REQUIRE(q_cu[0] == 0 && q_cu[nb] == nq && s_cu[0] == 0 && s_cu[nb] == ns, "tie_order_host: cu ends");
  for (int b = 0; b < nb; ++b)
    SPR_REQUIRE(q_cu[b + 1] >= q_cu[b] && s_cu[b + 1] >= s_cu[b], "tie_order_host: cu of cloud %d decreases", b);
  std::vector<int> vind((size_t)ns + 1);
  std::vector<Node> nodes(2 * (size_t)ns + 1);
  std::vector<float> box(6 * (size_t)nb);
  int deepest = 0;
  for (int b = 0; b < nb; ++b) {
    const int off = s_cu[b], n = s_cu[b + 1] - off;
    int depth = 0;
    if (tie::build_cloud(s_xyz + 3 * (size_t)off, n, vind.data() + off, nodes.data() + 2 * (size_t)off, 2 * n,
                         box.data() + 6 * (size_t)b, &depth)) {
      status[3] = 1;
      return 0;
    }
    if (depth > deepest) deepest = depth;
  }
  status[3] = 0;
  const int cap = max_count > 0 ? max_count : 1, depth_cap = deepest > 0 ? deepest : 1;
  std::vector<Frame> stack((size_t)depth_cap);
  std::vector<int> s_idx((size_t)cap);
  std::vector<float> s_d2((size_t)cap);
  const float r2 = radius * radius;
  for (int b = 0; b < nb; ++b) {
    const int off = s_cu[b];
    tie::CloudTree ct;
    ct.p = s_xyz + 3 * (size_t)off, ct.n = s_cu[b + 1] - off, ct.offset = off;
    ct.vind = vind.data() + off, ct.nodes = nodes.data() + 2 * (size_t)off, ct.n_nodes = 2 * ct.n;
    ct.rootbox = box.data() + 6 * (size_t)b;
    for (int i = q_cu[b]; i < q_cu[b + 1]; ++i) {
      const float* q = q_xyz + 3 * (size_t)i;
      const int rc = tie::fix_row(ct, q[0], q[1], q[2], r2, ns, nbr + (size_t)i * stride, width, max_count,
                                  stack.data(), depth_cap, s_idx.data(), s_d2.data(), cap);
      status[0] += rc == tie::kRowFixed;
      status[1] += rc == tie::kRowMismatch;
      status[2] += rc == tie::kRowOverflow;
    }
  }
  return 0;
}

extern "C" int spr_std_sort_replay_host(const float* keys, int n, int* perm, int* heap_ranges) {
  SPR_REQUIRE(n >= 0, "std_sort_replay_host: negative n %d", n);
  if (heap_ranges) *heap_ranges = 0;
  if (n == 0) return 0;
  SPR_REQUIRE(keys && perm, "std_sort_replay_host: null pointer");
  std::vector<float> k(keys, keys + n);
  for (int i = 0; i < n; ++i) perm[i] = i;
  SPR_REQUIRE(tie::std_sort_replay(perm, k.data(), n, heap_ranges) == 0, "std_sort_replay_host: range stack exhausted");
  return 0;
}
