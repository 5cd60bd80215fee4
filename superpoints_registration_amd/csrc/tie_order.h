// The reference's order of equal-d2 neighbours, restated: one definition for tie_order.hip's kernels and its host
// twins (include/spr.h, "neighbour ties in the reference's order").
//
// batch_nanoflann_neighbors (neighbors.cpp:211-332) orders a row by three deterministic steps, each replayed here in
// float32 with one rounding per operation (build without FMA contraction):
//   1. the kd-tree of the cloud's supports, in cloud order: leaf size 10, split axis = widest spread among the axes
//      whose box span is within (1 - 1e-5) of the widest, cut = box middle clamped to the points' range, the
//      two-pass in-place partition with its swap sequence, split index from (lim1, lim2, count / 2), boxes tightened
//      on the way up and the children's boxes as divlow / divhigh;
//   2. the radius search: near child first, the far child when mindist + cut - dists[axis] <= r2, leaf entries in the
//      permutation's order, kept when d2 < r2;
//   3. an introsort of the (index, d2) pairs that compares d2 only: median of three to the front, unguarded
//      partition, depth limit 2 floor(log2 n) with a heap sort behind it, ranges of at most 16 left to a final
//      insertion sort.  It is not stable: the order inside an equal-d2 run is whatever these moves leave.
// Everything works on caller memory with explicit capacities; a structure that does not fit is reported, never
// written past.  Plain C++ (also compiles without HIP: the stand-alone host checks).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SPR_TIE_HD __host__ __device__ inline
#else
#define SPR_TIE_HD inline
#endif

namespace spr {
namespace tie {

constexpr int kLeafMax = 10;        // KDTreeSingleIndexAdaptorParams(10), neighbors.cpp:245
constexpr int kSortSmall = 16;      // ranges up to this length are left to the insertion sort
constexpr int kSortStack = 64;      // deferred right halves: at most 2 floor(log2 n) <= 60 for n < 2^31

// return codes of the row functions
constexpr int kRowKept = 0, kRowFixed = 1, kRowMismatch = 2, kRowOverflow = 3;

struct Node {          // 16 words
  int c1, c2;          // children, -1 / -1 for a leaf
  int left, right;     // range of the permutation
  int feat;            // split axis
  int parent;
  int state;           // build only: 0 new, 1 left child under way, 2 right child under way, 3 done
  float cut;           // build only
  float divlow, divhigh;
  float lo[3], hi[3];  // build: the box handed down, then the tightened one
};

struct Frame {         // one level of the search's walk
  int node, state;
  float mind, dst;
};

SPR_TIE_HD float sq_diff(float a, float b) {
  const float d = a - b;
  return d * d;
}

// ((dx dx + dy dy) + dz dz), query - support
SPR_TIE_HD float d2_of(float qx, float qy, float qz, const float* s) {
  const float dx = qx - s[0], dy = qy - s[1], dz = qz - s[2];
  const float xx = dx * dx;
  const float yy = dy * dy;
  const float zz = dz * dz;
  float d = xx + yy;
  d = d + zz;
  return d;
}

// ---- 1. tree -------------------------------------------------------------------------------------------------------
SPR_TIE_HD void min_max(const float* p, const int* ind, int count, int axis, float& mn, float& mx) {
  mn = mx = p[3 * (size_t)ind[0] + axis];
  for (int i = 1; i < count; ++i) {
    const float v = p[3 * (size_t)ind[i] + axis];
    if (v < mn) mn = v;
    if (v > mx) mx = v;
  }
}

// Both passes of the in-place partition around `cut` on `axis`: afterwards ind[0, lim1) < cut, ind[lim1, lim2) == cut,
// ind[lim2, count) > cut.  The scan from the right never moves below position 0 (and gives up there).
SPR_TIE_HD void plane_split(const float* p, int* ind, int count, int axis, float cut, int& lim1, int& lim2) {
  int l = 0, r = count - 1;
  for (;;) {
    while (l <= r && p[3 * (size_t)ind[l] + axis] < cut) ++l;
    while (r && l <= r && p[3 * (size_t)ind[r] + axis] >= cut) --r;
    if (l > r || !r) break;
    const int t = ind[l];
    ind[l] = ind[r];
    ind[r] = t;
    ++l;
    --r;
  }
  lim1 = l;
  r = count - 1;
  for (;;) {
    while (l <= r && p[3 * (size_t)ind[l] + axis] <= cut) ++l;
    while (r && l <= r && p[3 * (size_t)ind[r] + axis] > cut) --r;
    if (l > r || !r) break;
    const int t = ind[l];
    ind[l] = ind[r];
    ind[r] = t;
    ++l;
    --r;
  }
  lim2 = l;
}

SPR_TIE_HD int middle_split(const float* p, int* ind, int count, const float* lo, const float* hi, int& feat,
                            float& cut) {
  const float eps = 0.00001f;
  float max_span = hi[0] - lo[0];
  for (int i = 1; i < 3; ++i) {
    const float span = hi[i] - lo[i];
    if (span > max_span) max_span = span;
  }
  const float keep = 1 - eps;
  const float bar = keep * max_span;
  float max_spread = -1;
  feat = 0;
  for (int i = 0; i < 3; ++i) {
    const float span = hi[i] - lo[i];
    if (span > bar) {
      float mn, mx;
      min_max(p, ind, count, i, mn, mx);
      const float spread = mx - mn;
      if (spread > max_spread) {
        feat = i;
        max_spread = spread;
      }
    }
  }
  const float sum = lo[feat] + hi[feat];
  const float middle = sum / 2;
  float mn, mx;
  min_max(p, ind, count, feat, mn, mx);
  cut = middle < mn ? mn : (middle > mx ? mx : middle);
  int lim1, lim2;
  plane_split(p, ind, count, feat, cut, lim1, lim2);
  const int half = count / 2;
  return lim1 > half ? lim1 : (lim2 < half ? lim2 : half);
}

// Tree of one cloud (n points at p, cloud-local indices in vind[n]); nodes[cap], 2 n are always enough for finite
// coordinates.  rootbox[6] = lo, hi of the cloud.  Returns 0, or 1 when the nodes ran out (nothing is written past
// cap); *depth = nodes on the longest root-to-leaf path (0 for an empty cloud).
SPR_TIE_HD int build_cloud(const float* p, int n, int* vind, Node* nodes, int cap, float* rootbox, int* depth) {
  *depth = 0;
  for (int d = 0; d < 6; ++d) rootbox[d] = 0.f;
  if (n <= 0) return 0;
  if (cap < 1) return 1;
  for (int i = 0; i < n; ++i) vind[i] = i;
  float lo[3], hi[3];
  for (int d = 0; d < 3; ++d) lo[d] = hi[d] = p[d];
  for (int k = 1; k < n; ++k)
    for (int d = 0; d < 3; ++d) {
      const float v = p[3 * (size_t)k + d];
      if (v < lo[d]) lo[d] = v;
      if (v > hi[d]) hi[d] = v;
    }
  for (int d = 0; d < 3; ++d) rootbox[d] = lo[d], rootbox[3 + d] = hi[d];
  int used = 1, cur = 0, level = 1, deepest = 1;
  {
    Node& r = nodes[0];
    r.c1 = r.c2 = -1, r.left = 0, r.right = n, r.feat = 0, r.parent = -1, r.state = 0;
    r.cut = r.divlow = r.divhigh = 0.f;
    for (int d = 0; d < 3; ++d) r.lo[d] = lo[d], r.hi[d] = hi[d];
  }
  while (cur >= 0) {
    Node& nd = nodes[cur];
    if (nd.state == 0) {
      const int count = nd.right - nd.left;
      if (count <= kLeafMax) {       // leaf: the box of its points
        if (count > 0) {
          const float* f = p + 3 * (size_t)vind[nd.left];
          for (int d = 0; d < 3; ++d) nd.lo[d] = nd.hi[d] = f[d];
          for (int k = nd.left + 1; k < nd.right; ++k) {
            const float* g = p + 3 * (size_t)vind[k];
            for (int d = 0; d < 3; ++d) {
              if (nd.lo[d] > g[d]) nd.lo[d] = g[d];
              if (nd.hi[d] < g[d]) nd.hi[d] = g[d];
            }
          }
        }
        nd.state = 3;
        cur = nd.parent;
        --level;
        continue;
      }
      if (used + 2 > cap) return 1;
      int feat;
      float cut;
      const int idx = middle_split(p, vind + nd.left, count, nd.lo, nd.hi, feat, cut);
      nd.feat = feat, nd.cut = cut;
      nd.c1 = used++, nd.c2 = used++;
      for (int s = 0; s < 2; ++s) {   // both children start from the box handed to this node
        Node& c = nodes[s ? nd.c2 : nd.c1];
        c.c1 = c.c2 = -1, c.feat = 0, c.parent = cur, c.state = 0;
        c.left = s ? nd.left + idx : nd.left;
        c.right = s ? nd.right : nd.left + idx;
        c.cut = c.divlow = c.divhigh = 0.f;
        for (int d = 0; d < 3; ++d) c.lo[d] = nd.lo[d], c.hi[d] = nd.hi[d];
        if (s) c.lo[feat] = cut; else c.hi[feat] = cut;
      }
      nd.state = 1;
      cur = nd.c1;
      if (++level > deepest) deepest = level;
    } else if (nd.state == 1) {
      nd.state = 2;
      cur = nd.c2;
      if (++level > deepest) deepest = level;
    } else {
      const Node& a = nodes[nd.c1];
      const Node& b = nodes[nd.c2];
      nd.divlow = a.hi[nd.feat];
      nd.divhigh = b.lo[nd.feat];
      for (int d = 0; d < 3; ++d) {
        nd.lo[d] = b.lo[d] < a.lo[d] ? b.lo[d] : a.lo[d];
        nd.hi[d] = a.hi[d] < b.hi[d] ? b.hi[d] : a.hi[d];
      }
      nd.state = 3;
      cur = nd.parent;
      --level;
    }
  }
  *depth = deepest;
  return 0;
}

// ---- 2. search -----------------------------------------------------------------------------------------------------
// What the walk does with a support in range: collect it (idx / d2 [cap], n counts past cap without storing), or only
// count those with d2 <= bar.
struct Sink {
  int* idx;
  float* d2;
  int cap, n, n_le;
  float bar;
};

// Walk of one query through the tree of its cloud.  stack[stack_cap]: one frame per level, stack_cap >= the tree's
// depth.  Returns 0, or 1 when the stack or a node index does not fit (the sink is then meaningless).
SPR_TIE_HD int search(const float* p, const int* vind, const Node* nodes, int n_nodes, const float* rootbox, float qx,
                      float qy, float qz, float r2, Frame* stack, int stack_cap, Sink& sink) {
  const float q[3] = {qx, qy, qz};
  float dists[3] = {0.f, 0.f, 0.f};
  float start = 0.f;
  for (int i = 0; i < 3; ++i) {
    if (q[i] < rootbox[i]) {
      dists[i] = sq_diff(q[i], rootbox[i]);
      start += dists[i];
    }
    if (q[i] > rootbox[3 + i]) {
      dists[i] = sq_diff(q[i], rootbox[3 + i]);
      start += dists[i];
    }
  }
  if (stack_cap < 1 || n_nodes < 1) return 1;
  int sp = 0;
  stack[0].node = 0, stack[0].state = 0, stack[0].mind = start, stack[0].dst = 0.f;
  while (sp >= 0) {
    Frame& f = stack[sp];
    if ((unsigned)f.node >= (unsigned)n_nodes) return 1;
    const Node& nd = nodes[f.node];
    if (nd.c1 < 0) {
      for (int i = nd.left; i < nd.right; ++i) {
        const int index = vind[i];
        const float dist = d2_of(qx, qy, qz, p + 3 * (size_t)index);
        if (dist < r2) {
          if (sink.idx) {
            if (sink.n < sink.cap) sink.idx[sink.n] = index, sink.d2[sink.n] = dist;
          } else if (dist <= sink.bar) {
            ++sink.n_le;
          }
          ++sink.n;
        }
      }
      --sp;
      continue;
    }
    const int axis = nd.feat;
    if ((unsigned)axis > 2u) return 1;
    const float val = q[axis];
    const float diff1 = val - nd.divlow, diff2 = val - nd.divhigh;
    const bool low_first = (diff1 + diff2) < 0;
    if (f.state == 0) {
      if (sp + 1 >= stack_cap) return 1;
      f.state = 1;
      Frame& g = stack[sp + 1];
      g.node = low_first ? nd.c1 : nd.c2, g.state = 0, g.mind = f.mind, g.dst = 0.f;
      ++sp;
    } else if (f.state == 1) {
      const float cut_dist = low_first ? sq_diff(val, nd.divhigh) : sq_diff(val, nd.divlow);
      const float dst = dists[axis];
      float m = f.mind + cut_dist;
      m = m - dst;
      if (m * 1.0f <= r2) {
        if (sp + 1 >= stack_cap) return 1;
        dists[axis] = cut_dist;
        f.dst = dst;
        f.state = 2;
        Frame& g = stack[sp + 1];
        g.node = low_first ? nd.c2 : nd.c1, g.state = 0, g.mind = m, g.dst = 0.f;
        ++sp;
      } else {
        --sp;
      }
    } else {
      dists[axis] = f.dst;
      --sp;
    }
  }
  return 0;
}

// ---- 3. sort -------------------------------------------------------------------------------------------------------
SPR_TIE_HD void swap_at(int* I, float* K, int a, int b) {
  const int ti = I[a];
  const float tk = K[a];
  I[a] = I[b], K[a] = K[b];
  I[b] = ti, K[b] = tk;
}

SPR_TIE_HD void sift_down_up(int* I, float* K, int first, int hole, int len, int vi, float vk) {
  const int top = hole;
  int child = hole;
  while (child < (len - 1) / 2) {
    child = 2 * (child + 1);
    if (K[first + child] < K[first + child - 1]) --child;
    I[first + hole] = I[first + child], K[first + hole] = K[first + child];
    hole = child;
  }
  if ((len & 1) == 0 && child == (len - 2) / 2) {
    child = 2 * (child + 1);
    I[first + hole] = I[first + child - 1], K[first + hole] = K[first + child - 1];
    hole = child - 1;
  }
  int parent = (hole - 1) / 2;
  while (hole > top && K[first + parent] < vk) {
    I[first + hole] = I[first + parent], K[first + hole] = K[first + parent];
    hole = parent;
    parent = (hole - 1) / 2;
  }
  I[first + hole] = vi, K[first + hole] = vk;
}

SPR_TIE_HD void heap_sort(int* I, float* K, int first, int last) {
  const int len = last - first;
  if (len >= 2)
    for (int parent = (len - 2) / 2;; --parent) {
      sift_down_up(I, K, first, parent, len, I[first + parent], K[first + parent]);
      if (parent == 0) break;
    }
  while (last - first > 1) {
    --last;
    const int vi = I[last];
    const float vk = K[last];
    I[last] = I[first], K[last] = K[first];
    sift_down_up(I, K, first, 0, last - first, vi, vk);
  }
}

SPR_TIE_HD void insert_unguarded(int* I, float* K, int at) {
  const int vi = I[at];
  const float vk = K[at];
  int next = at - 1;
  while (vk < K[next]) {
    I[at] = I[next], K[at] = K[next];
    at = next;
    --next;
  }
  I[at] = vi, K[at] = vk;
}

SPR_TIE_HD void insertion_sort(int* I, float* K, int first, int last) {
  for (int i = first + 1; i < last; ++i) {
    if (K[i] < K[first]) {
      const int vi = I[i];
      const float vk = K[i];
      for (int j = i; j > first; --j) I[j] = I[j - 1], K[j] = K[j - 1];
      I[first] = vi, K[first] = vk;
    } else {
      insert_unguarded(I, K, i);
    }
  }
}

// Sorts the n pairs (I, K) by K as the platform's std::sort does with a comparator on K alone.  *heap_ranges += the
// number of ranges that ran out of depth and were heap-sorted.  Returns 0, or 1 if the deferred-range stack would not
// fit (impossible for n < 2^31; the pairs are then left partly sorted).
SPR_TIE_HD int std_sort_replay(int* I, float* K, int n, int* heap_ranges) {
  if (n <= 0) return 0;
  int lg = 0;
  for (unsigned v = (unsigned)n; v > 1; v >>= 1) ++lg;
  int sf[kSortStack], sl[kSortStack], sd[kSortStack];
  int sp = 0, first = 0, last = n, depth = 2 * lg;
  for (;;) {
    while (last - first > kSortSmall) {
      if (depth == 0) {
        heap_sort(I, K, first, last);
        if (heap_ranges) ++*heap_ranges;
        break;
      }
      --depth;
      // median of (first + 1, middle, last - 1) to the front
      const int a = first + 1, b = first + (last - first) / 2, c = last - 1;
      int m;
      if (K[a] < K[b])
        m = K[b] < K[c] ? b : (K[a] < K[c] ? c : a);
      else
        m = K[a] < K[c] ? a : (K[b] < K[c] ? c : b);
      swap_at(I, K, first, m);
      // partition (first, last) around the front element; both scans are stopped by elements, not bounds
      int lo = first + 1, hi = last;
      const float pivot = K[first];
      for (;;) {
        while (K[lo] < pivot) ++lo;
        --hi;
        while (pivot < K[hi]) --hi;
        if (!(lo < hi)) break;
        swap_at(I, K, lo, hi);
        ++lo;
      }
      if (sp >= kSortStack) return 1;
      sf[sp] = lo, sl[sp] = last, sd[sp] = depth;   // the right part waits; it shares no element with the left one
      ++sp;
      last = lo;
    }
    if (sp == 0) break;
    --sp;
    first = sf[sp], last = sl[sp], depth = sd[sp];
  }
  if (n > kSortSmall) {
    insertion_sort(I, K, 0, kSortSmall);
    for (int i = kSortSmall; i < n; ++i) insert_unguarded(I, K, i);
  } else {
    insertion_sort(I, K, 0, n);
  }
  return 0;
}

// ---- a row ---------------------------------------------------------------------------------------------------------
struct CloudTree {     // the tree of the row's cloud
  const float* p;      // its supports
  int n;               // how many
  int offset;          // index of the first one in the batch
  const int* vind;
  const Node* nodes;
  int n_nodes;
  const float* rootbox;
};

// One row of a neighbour matrix written by the table search: `width` kept columns, ascending (d2, index), global
// indices, padded with `shadow`; max_count = the search's untruncated widest row.  If an equal-d2 run touches the kept
// columns -- two kept entries, or the last kept entry of a cut row and one behind the cut -- the row is replaced by
// the first `width` entries of the replayed search + sort.  scratch: s_idx / s_d2 [cap].  Nothing is written unless
// the replay fitted and holds the row's entries.
SPR_TIE_HD int fix_row(const CloudTree& t, float qx, float qy, float qz, float r2, int shadow, int* row, int width,
                       int max_count, Frame* stack, int stack_cap, int* s_idx, float* s_d2, int cap) {
  int cnt = 0;
  bool tied = false;
  float prev = 0.f;
  for (; cnt < width; ++cnt) {
    const int e = row[cnt];
    if (e == shadow) break;
    if (e < t.offset || e - t.offset >= t.n) return kRowMismatch;
    const float d = d2_of(qx, qy, qz, t.p + 3 * (size_t)(e - t.offset));
    if (cnt && d == prev) tied = true;
    prev = d;
  }
  if (cnt == 0) return kRowKept;
  Sink sink;
  if (!tied) {
    if (cnt < width || max_count <= width) return kRowKept;
    sink.idx = nullptr, sink.d2 = nullptr, sink.cap = 0, sink.n = 0, sink.n_le = 0, sink.bar = prev;
    if (search(t.p, t.vind, t.nodes, t.n_nodes, t.rootbox, qx, qy, qz, r2, stack, stack_cap, sink)) return kRowOverflow;
    if (sink.n_le <= width) return kRowKept;
  }
  sink.idx = s_idx, sink.d2 = s_d2, sink.cap = cap, sink.n = 0, sink.n_le = 0, sink.bar = 0.f;
  if (search(t.p, t.vind, t.nodes, t.n_nodes, t.rootbox, qx, qy, qz, r2, stack, stack_cap, sink)) return kRowOverflow;
  const int n = sink.n;
  if (n > cap) return kRowOverflow;
  if (std_sort_replay(s_idx, s_d2, n, nullptr)) return kRowOverflow;
  if (cnt != (n < width ? n : width)) return kRowMismatch;
  int prev_e = -1;
  for (int j = 0; j < cnt; ++j) {
    const int e = row[j] - t.offset;
    const float d = d2_of(qx, qy, qz, t.p + 3 * (size_t)e);
    if (d != s_d2[j]) return kRowMismatch;
    if (j && d == prev && e <= prev_e) return kRowMismatch;
    prev = d, prev_e = e;
    bool found = false;
    for (int k = j; k >= 0 && s_d2[k] == d && !found; --k) found = s_idx[k] == e;
    for (int k = j + 1; k < n && s_d2[k] == d && !found; ++k) found = s_idx[k] == e;
    if (!found) return kRowMismatch;
  }
  for (int j = 0; j < cnt; ++j) row[j] = s_idx[j] + t.offset;
  return kRowFixed;
}

}  // namespace tie
}  // namespace spr
