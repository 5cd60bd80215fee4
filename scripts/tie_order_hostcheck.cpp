// Stand-alone host check of csrc/tie_order.h for sanitizer builds (scripts/tie_order_hostcheck.py compiles and feeds
// it): every buffer the header works in is a heap block of exactly the size the library would hand it, so a write or
// read past a tree, a walk stack or a row's scratch is an AddressSanitizer report.  Input (binary, stdin), per case:
//   int32 nq ns nb width max_count; float radius; q_cu[nb + 1]; s_cu[nb + 1]; q[nq * 3]; s[ns * 3];
//   rows[nq * width] (index order); want[nq * width] (the reference's).  Exit status 0 = every case literally equal.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../superpoints_registration_amd/csrc/tie_order.h"

using namespace spr::tie;

template <typename T>
static bool rd(T* p, size_t n) {
  return n == 0 || std::fread(p, sizeof(T), n, stdin) == n;
}

template <typename T>
static T* exact(size_t n) {   // no slack: one element past the end is outside the allocation
  return (T*)std::malloc(n ? n * sizeof(T) : 1);
}

int main() {
  int hdr[5], cases = 0, bad = 0;
  long fixed = 0;
  while (std::fread(hdr, sizeof(int), 5, stdin) == 5) {
    const int nq = hdr[0], ns = hdr[1], nb = hdr[2], width = hdr[3], max_count = hdr[4];
    float radius;
    std::vector<int> q_cu(nb + 1), s_cu(nb + 1), rows((size_t)nq * width), want((size_t)nq * width);
    std::vector<float> q((size_t)nq * 3), s((size_t)ns * 3);
    if (!rd(&radius, 1) || !rd(q_cu.data(), nb + 1) || !rd(s_cu.data(), nb + 1) || !rd(q.data(), q.size()) ||
        !rd(s.data(), s.size()) || !rd(rows.data(), rows.size()) || !rd(want.data(), want.size()))
      return 2;
    const float r2 = radius * radius;
    for (int b = 0; b < nb; ++b) {
      const int off = s_cu[b], n = s_cu[b + 1] - off;
      int* vind = exact<int>(n);
      Node* nodes = exact<Node>(2 * (size_t)n);
      float box[6];
      int depth = 0;
      if (build_cloud(s.data() + 3 * (size_t)off, n, vind, nodes, 2 * n, box, &depth)) return 3;
      Frame* stack = exact<Frame>(depth > 0 ? depth : 1);
      int* s_idx = exact<int>(max_count);
      float* s_d2 = exact<float>(max_count);
      CloudTree t{s.data() + 3 * (size_t)off, n, off, vind, nodes, 2 * n, box};
      for (int i = q_cu[b]; i < q_cu[b + 1]; ++i) {
        const int rc = fix_row(t, q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2], r2, ns,
                               rows.data() + (size_t)i * width, width, max_count, stack, depth > 0 ? depth : 1, s_idx,
                               s_d2, max_count);
        if (rc == kRowMismatch || rc == kRowOverflow) ++bad;
        fixed += rc == kRowFixed;
      }
      std::free(vind), std::free(nodes), std::free(stack), std::free(s_idx), std::free(s_d2);
    }
    if (std::memcmp(rows.data(), want.data(), rows.size() * sizeof(int)) != 0) ++bad;
    ++cases;
  }
  // the sort alone on an exact block: a median-of-three killer long enough for the heap path
  const int n = 2000, k = n / 2;
  int* I = exact<int>(n);
  float* K = exact<float>(n);
  for (int i = 1; i <= k; ++i) K[i - 1] = (float)(i % 2 ? i : k + i - 1), K[k + i - 1] = (float)(2 * i);
  for (int i = 0; i < n; ++i) I[i] = i;
  int heap = 0;
  if (std_sort_replay(I, K, n, &heap) || heap < 1) ++bad;
  for (int i = 1; i < n; ++i) bad += K[i - 1] > K[i];
  std::free(I), std::free(K);
  std::printf("tie_order_hostcheck: %d cases, %ld rows fixed, %d heap ranges, %d bad\n", cases, fixed, heap, bad);
  return bad ? 1 : 0;
}
